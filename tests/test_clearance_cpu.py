"""CPU checks of the clearance profile: the numpy reference the GPU tests compare against (tests/clearance_ref.py) pinned
against the reference of the separation check, against itself with a pair removed and over shards; header / exports / ctypes
struct; the switches of the Python surface."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import clearance_ref as clr  # noqa: E402
import separation_ref as sr  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "scp_hip.h")
H, R = 0.2, 0.8
_REFS = {}


def case(N, K, D, seed):
    """host trajectories of a random case and its full reference, made once"""
    key = (N, K, D, seed)
    if key not in _REFS:
        p0, v0, acc = sr.random_case(N, K, D, seed)
        pos, vel = sr.kinematics(p0, v0, acc, H)
        _REFS[key] = ((pos, vel, acc), clr.profile(pos, vel, acc, H, R))
    return _REFS[key]


@pytest.mark.parametrize("N,K,D,seed", [(7, 13, 3, 12), (65, 50, 3, 16), (129, 7, 2, 17)])
def test_reference_agrees_with_the_global_reference(N, K, D, seed):
    host, ref = case(N, K, D, seed)
    st = sr.global_stats(*host, H, R)
    for e in (ref["vehicle"], ref["step"]):
        best = np.lexsort((e["row"], e["f"]))[0]
        assert (e["f"][best], int(e["row"][best]), e["t"][best]) == (st["min_f"], st["argmin_row"], st["argmin_t"])
        assert e["sample"].min() == st["sample_min_dist"]
    assert ref["step"]["n_violating"].sum() == st["n_violating"] and ref["vehicle"]["n_violating"].sum() == 2 * st["n_violating"]
    assert ref["step"]["n_rows"].tolist() == [N * (N - 1) // 2] * K and ref["vehicle"]["n_rows"].tolist() == [(N - 1) * K] * N
    assert abs(ref["s_max"] - st["s_max"]) <= 4 * sr.EPS * st["s_max"]  # (the sums are formed in another order)
    # the structure: a step entry's row lies in the step, a vehicle entry's pair contains the vehicle
    i, j = sr.pair_indices(N)
    k, q = np.divmod(ref["step"]["row"].astype(np.int64), ref["pairs"])
    assert k.tolist() == list(range(K))
    q = ref["vehicle"]["row"].astype(np.int64) % ref["pairs"]
    assert ((i[q] == np.arange(N)) | (j[q] == np.arange(N))).all()
    # second_f: the second smallest of the entry's rows
    v = 3
    mine = np.sort(ref["f"][(i[ref["rows"] % ref["pairs"]] == v) | (j[ref["rows"] % ref["pairs"]] == v)])
    assert (ref["vehicle"]["f"][v], ref["vehicle"]["second_f"][v]) == (mine[0], mine[1])


def test_reference_without_a_nearest_partner_differs_in_two_entries():
    """the comparison can fail: without the pair (v, nearest partner of v) exactly the entries of v and of that partner change"""
    N, K, D, seed = 65, 50, 3, 16
    host, ref = case(N, K, D, seed)
    i, j = sr.pair_indices(N)
    v = 10
    q = int(ref["vehicle"]["row"][v]) % ref["pairs"]
    partner = int(j[q] if i[q] == v else i[q])
    less = clr.profile(*host, H, R, skip_pairs=[q])
    same = clr.equal(ref["vehicle"], less["vehicle"])
    assert np.nonzero(~same)[0].tolist() == sorted([v, partner])
    rest = (ref["rows"] % ref["pairs"] != q) & ((i[ref["rows"] % ref["pairs"]] == v) | (j[ref["rows"] % ref["pairs"]] == v))
    assert less["vehicle"]["f"][v] == ref["f"][rest].min() > ref["vehicle"]["f"][v]
    assert less["vehicle"]["n_rows"][partner] == ref["vehicle"]["n_rows"][partner] - K


def test_reference_shards_merge_to_the_full_range():
    N, K, D, seed = 129, 7, 2, 17
    host, ref = case(N, K, D, seed)
    pairs = ref["pairs"]
    cuts = [0, 1, 70, 70, pairs // 2 - 7, pairs]
    parts = [clr.profile(*host, H, R, a, b) for a, b in zip(cuts[:-1], cuts[1:])]
    for name in ("vehicle", "step"):
        assert clr.equal(clr.merge([p[name] for p in parts]), ref[name]).all()
    assert parts[0]["vehicle"]["n_rows"].tolist() == [K, K] + [0] * (N - 2)  # the shard [0, 1): the pair (0, 1) only
    empty = parts[2]
    assert (empty["vehicle"]["n_rows"] == 0).all() and np.isinf(empty["step"]["f"]).all()
    assert (empty["step"]["row"] == np.uint64(clr.NO_ROW)).all()


def test_abi_header_export_and_struct(tmp_path):
    from path_planning import _hip

    text = open(HEADER).read()
    for sym in ("scp_clearance_profile", "scp_ctx_last_clearance_solved"):
        assert sym in text and sym in _hip.EXPORTS and hasattr(ctypes.CDLL(_hip.library_path()), sym)
    assert "#define SCP_ABI_VERSION 7" in text and _hip.ABI_VERSION == 7  # additive: the version stays
    names = [f for f, _ in _hip.Clearance._fields_]
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "scp_hip.h"\nint main(void){printf("%zu", sizeof(scp_clearance));\n'
                   + "".join(f'printf(" %zu", offsetof(scp_clearance, {f}));\n' for f in names) + "return 0;}\n")
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", os.path.dirname(HEADER), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    S = _hip.Clearance
    assert got == [ctypes.sizeof(S)] + [getattr(S, f).offset for f in names] == [48, 0, 8, 16, 24, 32, 40]
    assert _hip.CLEARANCE_DTYPE.itemsize == 48 and list(_hip.CLEARANCE_DTYPE.names) == names
    assert [_hip.CLEARANCE_DTYPE.fields[f][1] for f in names] == got[1:]


def test_python_surface():
    import inspect

    from path_planning import _hip
    from path_planning.cli import compute_trajectories, compute_trajectories_batch
    from path_planning.solvers.scp import SCP
    from path_planning.viz.plot_trajectories import plot_clearance

    sig = inspect.signature(SCP.validate_solution)
    assert [sig.parameters[k].default for k in ("continuous", "conflicts", "clearance")] == [False, False, False]
    assert "clearance_profile" in dir(_hip.Context) and "last_clearance_solved" in dir(_hip.Context)
    assert callable(plot_clearance)
    for cli in (compute_trajectories, compute_trajectories_batch):
        assert cli.build_parser().parse_args(["--clearance"]).clearance is True
        assert cli.build_parser().parse_args([]).clearance is False
    assert "clearance" not in compute_trajectories_batch.CONFIG
    assert compute_trajectories_batch.CSV_FIELDS == ["N", "trial_index", "status", "time_sec", "K", "T", "h", "error"]
