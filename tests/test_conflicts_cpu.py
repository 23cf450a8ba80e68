"""CPU checks of the conflict list: conflict_windows on hand-made records, header / exports / ctypes struct, the numpy
reference the GPU tests compare against (tests/conflicts_ref.py) pinned against closed forms and a dense scan."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conflicts_ref as cr  # noqa: E402
import separation_ref as sr  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "scp_hip.h")
H = 0.2


def recs(N, items):
    """items: (k, (i, j), min_dist, t_min, t_enter, t_exit, pieces)"""
    from path_planning import _hip

    pair = [(a, b) for a in range(N) for b in range(a + 1, N)]
    out = np.zeros(len(items), dtype=_hip.CONFLICT_DTYPE)
    for e, (k, ij, m, tm, t0, t1, pc) in enumerate(items):
        out[e] = (k * len(pair) + pair.index(ij), m, tm, t0, t1, pc, 0)
    return out


def windows(N, K, items):
    from path_planning.solvers.conflicts import conflict_windows

    return conflict_windows(recs(N, items), N, K, H)


def test_windows_single_segment_and_empty():
    from path_planning import _hip

    assert windows(4, 9, []) == []
    from path_planning.solvers.conflicts import conflict_windows
    assert conflict_windows(np.zeros(0, dtype=_hip.CONFLICT_DTYPE), 4, 9, H) == []
    (w,) = windows(4, 9, [(3, (1, 3), 0.25, 0.1, 0.0275, 0.1725, 1)])
    assert w == {"vehicles": (1, 3), "t_start": 3 * H + 0.0275, "t_end": 3 * H + 0.1725,
                 "duration": (3 * H + 0.1725) - (3 * H + 0.0275), "min_distance": 0.25, "t_min_distance": 3 * H + 0.1,
                 "first_timestep": 3, "n_segments": 1, "pieces": 1}
    assert list(w) == ["vehicles", "t_start", "t_end", "duration", "min_distance", "t_min_distance", "first_timestep",
                       "n_segments", "pieces"]


def test_windows_three_segment_run_merges():
    items = [(5, (0, 2), 0.6, H, 0.05, H, 1), (6, (0, 2), 0.3, 0.12, 0.0, H, 1), (7, (0, 2), 0.5, 0.0, 0.0, 0.07, 1)]
    for order in ([0, 1, 2], [2, 0, 1]):  # the order of the records does not matter
        (w,) = windows(3, 10, [items[e] for e in order])
        assert w["vehicles"] == (0, 2) and w["n_segments"] == 3 and w["first_timestep"] == 5 and w["pieces"] == 1
        assert w["t_start"] == 5 * H + 0.05 and w["t_end"] == 7 * H + 0.07 and w["duration"] == w["t_end"] - w["t_start"]
        assert w["min_distance"] == 0.3 and w["t_min_distance"] == 6 * H + 0.12


def test_windows_two_runs_of_one_pair_stay_two():
    ws = windows(3, 10, [(1, (0, 1), 0.5, H, 0.1, H, 1), (2, (0, 1), 0.5, 0.0, 0.0, 0.1, 1),  # run 1: k = 1, 2
                         (4, (0, 1), 0.4, 0.1, 0.0, H, 1), (5, (0, 1), 0.6, 0.0, 0.0, 0.02, 1)])  # k = 3 is clean
    assert [(w["first_timestep"], w["n_segments"]) for w in ws] == [(1, 2), (4, 2)]
    assert ws[1]["t_start"] == 4 * H and ws[1]["min_distance"] == 0.4


def test_windows_adjacent_segments_that_do_not_touch():
    # k = 2 leaves the conflict before its end (t_exit < h); k = 3 starts inside one: two windows
    ws = windows(3, 10, [(2, (1, 2), 0.5, 0.1, 0.05, 0.15, 1), (3, (1, 2), 0.5, 0.0, 0.0, 0.1, 1)])
    assert [w["n_segments"] for w in ws] == [1, 1]
    # ... and t_exit == h followed by t_enter > 0
    ws = windows(3, 10, [(2, (1, 2), 0.5, H, 0.05, H, 1), (3, (1, 2), 0.5, 0.1, 1e-9, 0.15, 1)])
    assert [w["n_segments"] for w in ws] == [1, 1]


def test_windows_two_pieces_are_a_hull():
    (w,) = windows(3, 10, [(2, (0, 1), 0.2, 0.03, 0.01, 0.19, 2)])
    assert w["pieces"] == 2 and w["t_start"] == 2 * H + 0.01 and w["t_end"] == 2 * H + 0.19
    # merged with its neighbours the window still says so
    (w,) = windows(3, 10, [(1, (0, 1), 0.2, H, 0.1, H, 1), (2, (0, 1), 0.2, 0.03, 0.0, H, 2), (3, (0, 1), 0.2, 0.0, 0.0, 0.1, 1)])
    assert w["pieces"] == 2 and w["n_segments"] == 3


def test_windows_interleaved_pairs_and_ordering():
    ws = windows(4, 10, [(2, (0, 1), 0.5, H, 0.1, H, 1), (2, (2, 3), 0.4, 0.1, 0.05, 0.15, 1), (3, (0, 1), 0.3, 0.1, 0.0, H, 1),
                         (3, (1, 2), 0.6, 0.1, 0.0, 0.15, 1), (4, (0, 1), 0.5, 0.0, 0.0, 0.05, 1), (2, (0, 3), 0.1, 0.1, 0.05, 0.2, 1),
                         (0, (2, 3), 0.7, 0.0, 0.0, 0.01, 1)])
    assert [(w["vehicles"], w["first_timestep"], w["n_segments"]) for w in ws] == [
        ((2, 3), 0, 1), ((0, 3), 2, 1), ((2, 3), 2, 1), ((0, 1), 2, 3), ((1, 2), 3, 1)]
    keys = [(w["t_start"],) + w["vehicles"] for w in ws]
    assert keys == sorted(keys)
    # equal start times: ordered by the vehicles
    ws = windows(4, 10, [(1, (1, 3), 0.5, 0.0, 0.0, 0.1, 1), (1, (0, 2), 0.5, 0.0, 0.0, 0.1, 1)])
    assert [w["vehicles"] for w in ws] == [(0, 2), (1, 3)]


def test_pairs_from_index_is_exact():
    from path_planning.solvers.conflicts import pairs_from_index

    for N in (2, 3, 65, 1024):
        i, j = sr.pair_indices(N)
        gi, gj = pairs_from_index(np.arange(i.size), N)
        assert np.array_equal(gi, i) and np.array_equal(gj, j)


def test_abi_header_export_and_struct(tmp_path):
    from path_planning import _hip

    text = open(HEADER).read()
    assert "scp_list_conflicts" in text and "scp_list_conflicts" in _hip.EXPORTS
    assert "#define SCP_ABI_VERSION 7" in text and _hip.ABI_VERSION == 7  # additive: the version stays
    assert hasattr(ctypes.CDLL(_hip.library_path()), "scp_list_conflicts")
    names = [f for f, _ in _hip.Conflict._fields_]
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "scp_hip.h"\nint main(void){printf("%zu", sizeof(scp_conflict));\n'
                   + "".join(f'printf(" %zu", offsetof(scp_conflict, {f}));\n' for f in names) + "return 0;}\n")
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", os.path.dirname(HEADER), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    S = _hip.Conflict
    assert got == [ctypes.sizeof(S)] + [getattr(S, f).offset for f in names] == [48, 0, 8, 16, 24, 32, 40, 44]
    assert _hip.CONFLICT_DTYPE.itemsize == 48 and list(_hip.CONFLICT_DTYPE.names) == names
    assert [_hip.CONFLICT_DTYPE.fields[f][1] for f in names] == got[1:]


def test_python_surface():
    import inspect

    from path_planning import _hip
    from path_planning.cli import compute_trajectories, compute_trajectories_batch
    from path_planning.solvers.scp import SCP

    sig = inspect.signature(SCP.validate_solution)
    assert sig.parameters["conflicts"].default is False and sig.parameters["continuous"].default is False
    assert "list_conflicts" in dir(_hip.Context)
    for cli in (compute_trajectories, compute_trajectories_batch):
        assert cli.build_parser().parse_args(["--list-conflicts"]).list_conflicts is True
        assert cli.build_parser().parse_args([]).list_conflicts is False
    assert "list_conflicts" not in compute_trajectories_batch.CONFIG
    assert compute_trajectories_batch.CSV_FIELDS == ["N", "trial_index", "status", "time_sec", "K", "T", "h", "error"]


def test_reference_on_the_tunnelling_pair():
    """relative position 0.4 - 4 t on one axis, R = 0.3: |0.4 - 4 t| = 0.29 at t = 0.0275 and t = 0.1725"""
    for N, D, pair in ((2, 2, (0, 1)), (7, 3, (3, 6))):
        pos, vel, acc, row = cr.tunnelling_case(N, D, pair)
        ref = cr.records(pos, vel, acc, H, 0.3)
        assert ref["rows"].tolist() == [row] and ref["pieces"].tolist() == [1]
        assert abs(ref["t_enter"][0] - 0.0275) < 1e-12 and abs(ref["t_exit"][0] - 0.1725) < 1e-12
        assert abs(ref["t_min"][0] - 0.1) < 1e-12


def test_reference_two_pieces_case_has_four_roots():
    d, w, b = cr.TWO_PIECES
    win = cr.window(sr.coefficients(d, w, b), H, 0.29)
    assert win[2] == 2 and len(win[3]) == 4 and 0 < win[3][0] == win[0] and win[1] == win[3][3] < H


@pytest.mark.parametrize("N,K,D,seed", [(2, 9, 2, 11), (65, 50, 3, 16), (129, 7, 2, 17), (130, 9, 3, 21), (60, 25, 2, 14)])
def test_reference_vs_dense_scan(N, K, D, seed):
    """4001 samples per violating segment.  The scan's slack on VALUES is dense_minima's bound: |f'| <= 2 S (|w| + h |b|) and
    the nearest sample is at most h / 8000 away.  (a) every sample outside [t_enter, t_exit] is at or above the threshold;
    (b) for pieces == 1 every sample inside is below it up to that slack (f leaves the threshold only at the ends);
    (c) the ends are on the threshold: the sample next to an interior end is within the slack of it;
    (d) the scan sees at most `pieces` separate runs below the threshold.
    Also the undecided cap of the GPU tests (at most 0.1 % of a case's segments within TOL of the threshold)."""
    R = 0.8
    p0, v0, acc = sr.random_case(N, K, D, seed)
    pos, vel = sr.kinematics(p0, v0, acc, H)
    ref = cr.records(pos, vel, acc, H, R)
    st = ref["stats"]
    thr2 = st["thr"] ** 2
    tol = 32 * sr.EPS * st["s_max"] ** 2
    undecided = np.abs(st["f"] - thr2) <= tol
    assert undecided.sum() <= 1e-3 * st["n_segments"]
    assert ref["rows"].size == st["n_violating"] and (np.diff(ref["rows"]) > 0).all()
    assert N == 2 or st["n_violating"] > 0  # (two vehicles in a 20 m box never meet: the empty list)
    print(f"{N}x{K}x{D}: {st['n_violating']} violating segments, {int(undecided.sum())} undecided of {st['n_segments']}")
    t = np.linspace(0.0, H, 4001)
    n = lambda x: float(np.sqrt((x ** 2).sum()))  # noqa: E731
    for e, row in enumerate(ref["rows"]):
        d, w, b = cr.segment_of_row((pos, vel, acc), row)
        c = sr.coefficients(d, w, b)
        slack = 2 * float(sr.s_bound(d, w, b, H)) * (n(w) + H * n(b)) * H / (2 * 4000) + tol
        fv = cr.f_at(c, t)
        t0, t1, pc = ref["t_enter"][e], ref["t_exit"][e], ref["pieces"][e]
        assert 0.0 <= t0 <= t1 <= H and pc in (1, 2)
        outside = (t < t0) | (t > t1)
        assert (fv[outside] >= thr2 - tol).all()
        if pc == 1:
            assert (fv[~outside] <= thr2 + tol).all()
        for end in (t0, t1):
            if 0.0 < end < H:
                assert abs(cr.f_at(c, end) - thr2) <= tol
                assert abs(fv[np.argmin(np.abs(t - end))] - thr2) <= slack
        runs = np.diff(np.concatenate([[0], (fv < thr2 - tol).astype(int)])) == 1
        assert runs.sum() <= pc
        assert abs(fv.min() - ref["f"][e]) <= slack and fv.min() >= ref["f"][e] - tol
