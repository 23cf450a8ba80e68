"""Shortened reference paths, without a GPU: the properties of the restatement (tests/shorten_ref.py) that the device code is
held to exactly -- visibility is symmetric and agrees with the edge masks, a shortened polyline keeps its clearance and never
gets longer, a vehicle with clearance >= delta has no blocked corridor segment --, the forced cases, the struct layout and the
Python surface."""
import ctypes
import inspect
import os
import subprocess

import numpy as np
import pytest

import corridor_ref as cr
import reference_path_ref as rr
import shorten_cases as sc
import shorten_ref as sr

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "scp_hip.h")

CASES = {c.name: c for c in sc.all_cases()}
RANDOM = [n for n in CASES if n.startswith("rand")]
PER_CASE = 4  # vehicles per case in the per-point checks


def _found(c):
    return np.nonzero(c.want()["info"]["status"] == 0)[0]


@pytest.mark.parametrize("name", RANDOM)
def test_visibility_is_symmetric_and_agrees_with_the_edges(name):
    c = CASES[name]
    w = c.want()
    rng = np.random.default_rng(len(name) + c.nodes)
    A, B = rng.integers(0, c.nodes, 300), rng.integers(0, c.nodes, 300)
    XA, XB = np.array(rr.node_coords(c.L, A)), np.array(rr.node_coords(c.L, B))
    ab = sr.clear_many(c.D, w["sat"], c.stride, c.clearance, XA, XB)
    ba = sr.clear_many(c.D, w["sat"], c.stride, c.clearance, XB, XA)
    np.testing.assert_array_equal(ab, ba)
    # every neighbour of every node, all at once per direction: clear == the edge bit
    node = np.arange(c.nodes, dtype=np.int64)
    X = np.array(rr.node_coords(c.L, node))
    n_pairs = 0
    for n in range(27):
        dirn = rr.direction(n)
        if n == rr.SELF or (c.D == 2 and dirn[2] != 0):
            continue
        Y = X + np.array(dirn)[:, None]
        inside = ((Y >= 0) & (Y < np.array(c.L)[:, None])).all(axis=0)
        bit = (w["edges"][inside] >> np.uint32(n) & np.uint32(1)).astype(bool)
        np.testing.assert_array_equal(sr.clear_many(c.D, w["sat"], c.stride, c.clearance, X[:, inside], Y[:, inside]), bit, err_msg=str(n))
        n_pairs += int(inside.sum())
    assert n_pairs > 0 or c.nodes == 1


def test_a_pair_is_clear_of_itself():
    c = CASES["rand2d_13x11_s1_c0"]
    blocked = int(np.nonzero(~(c.want()["edges"] >> np.uint32(rr.SELF) & np.uint32(1)).astype(bool))[0][0])
    assert sr.clear(c.D, c.want()["sat"], c.L, c.stride, c.clearance, blocked, blocked)  # n = 0 has no step to fail


@pytest.mark.parametrize("name", list(CASES))
def test_polyline_keeps_its_clearance(name):
    """200 points per edge of the shortened polyline: no occupied cell within `clearance` cells of the point's cell"""
    c = CASES[name]
    w, sat = sc.want(c), c.want()["sat"]
    s = (np.arange(201) / 200.0)[:, None]
    for i in _found(c)[:PER_CASE]:
        W = w["W"][i]
        for e in range(W.shape[0] - 1):
            pts = W[e] + s * (W[e + 1] - W[e])
            cell = np.floor((pts - np.asarray(c.origin)[:c.D]) / c.cell).astype(np.int64)
            a, b = [np.zeros(201, dtype=np.int64)] * 3, [np.zeros(201, dtype=np.int64)] * 3
            for d in range(c.D):
                assert (cell[:, d] >= 0).all() and (cell[:, d] < c.dims[d]).all()
                a[d] = np.maximum(cell[:, d] - c.clearance, 0)
                b[d] = np.minimum(cell[:, d] + c.clearance, c.dims[d] - 1)
            assert (rr.occupied_in(sat, a, b) == 0).all(), (i, e)


@pytest.mark.parametrize("name", list(CASES))
def test_kept_lists_records_and_lengths(name):
    c = CASES[name]
    w, info = sc.want(c), c.want()["info"]
    out, kept = w["out"], w["kept"]
    failed = info["status"] != 0
    # a vehicle without a path: untouched rows, a kept row of -1, a record of zeros
    np.testing.assert_array_equal(w["ref"][failed].view(np.uint64), c.want()["ref"][failed].view(np.uint64))
    assert (kept[failed] == -1).all() and not out[failed].view(np.uint8).any()
    for i in _found(c):
        m, n = int(info["n_nodes"][i]), int(out["n_kept"][i])
        k = kept[i]
        assert 1 <= n <= m and out["n_vertices"][i] == max(n, 2) and (k[n:] == -1).all()
        assert k[0] == 0 and k[n - 1] == m - 1 and (np.diff(k[:n]) > 0).all()
        assert out["length"][i] <= out["length_before"][i], (i, out[i])
        np.testing.assert_array_equal(w["ref"][i, 0], c.p0[i])
        np.testing.assert_array_equal(w["ref"][i, c.K], c.pf[i])
        # evenly spaced: consecutive points are at most length / K apart (a few roundings aside)
        step = np.sqrt(((w["ref"][i, 1:] - w["ref"][i, :-1]) ** 2).sum(axis=1))
        assert (step <= out["length"][i] / c.K * (1 + 1e-9) + 1e-12).all()
    # greedy means maximal: the node after a kept one's successor is not seen by it (spot check on a few vehicles)
    sat = c.want()["sat"]
    for i in _found(c)[:PER_CASE]:
        n, m = int(out["n_kept"][i]), int(info["n_nodes"][i])
        X = np.array(rr.node_coords(c.L, c.want()["path"][i, :m].astype(np.int64)))
        for e in range(n - 1):
            a, later = int(kept[i, e]), X[:, int(kept[i, e + 1]) + 1:]
            assert not sr.clear_many(c.D, sat, c.stride, c.clearance, np.repeat(X[:, a:a + 1], later.shape[1], axis=1), later).any()


def test_clearance_at_least_delta_means_no_blocked_segment():
    n_guaranteed, n_other, blocked_other = 0, 0, 0
    for c in CASES.values():
        w, sat = sc.want(c), c.want()["sat"]
        delta = sr.delta_of(w["out"]["length"], c.K, c.cell)
        found = _found(c)
        for i in (found if c.N <= 10 else found[:40]):
            _, n_blocked = cr.corridor_boxes(c.D, c.origin, c.cell, sat, w["ref"][i][None], 0)
            if c.clearance >= delta[i]:
                assert n_blocked == 0, (c.name, i, delta[i])
                n_guaranteed += 1
            else:
                n_other += 1
                blocked_other += n_blocked
    print(f"clearance >= delta: {n_guaranteed} vehicles, none blocked; {n_other} others with {blocked_other} blocked segments")
    assert n_guaranteed >= 30


def test_forced_cases():
    c = CASES["one_node"]
    out = sc.want(c)["out"]
    assert out["n_kept"].tolist() == [1, 1, 0, 0] and out["n_vertices"].tolist() == [2, 2, 0, 0]
    for i in (0, 1):  # the straight line, evenly spaced
        want = c.p0[i] + (np.arange(c.K + 1) / c.K)[:, None] * (c.pf[i] - c.p0[i])
        np.testing.assert_allclose(sc.want(c)["ref"][i], want, rtol=0, atol=1e-14)
    c = CASES["closed_wall"]
    info, out = c.want()["info"], sc.want(c)["out"]
    assert info["status"].tolist() == [3, 0, 0] and out["n_kept"][0] == 0 and (sc.want(c)["kept"][0] == -1).all()
    np.testing.assert_array_equal(sc.want(c)["ref"][0], c.ref_in()[0])
    for K in (1, 2, 3):
        c = CASES[f"long_path_K{K}"]
        w = sc.want(c)
        assert w["ref"].shape == (2, K + 1, 2) and (w["out"]["n_kept"] >= 3).all()
        np.testing.assert_array_equal(w["ref"][:, 0], c.p0)
        np.testing.assert_array_equal(w["ref"][:, K], c.pf)
    c = CASES["serpentine"]
    w = sc.want(c)
    walls = np.array([31, 16])  # crossed by vehicles 0 (y = 0 -> 62) and 1 (y = 32 -> 0), each through a gap at one end
    assert (w["out"]["n_kept"][:2] - 2 >= walls).all() and w["out"]["n_kept"][2] == 1
    assert c.want()["info"]["n_nodes"][0] > 64  # (more than one block of 64 candidates)
    c = CASES["open_40x30"]
    w = sc.want(c)
    assert w["out"]["n_kept"].tolist() == [2] * 4 and w["out"]["n_vertices"].tolist() == [2] * 4
    np.testing.assert_array_equal(w["kept"][:, :2], np.stack([np.zeros(4, dtype=np.int32), c.want()["info"]["n_nodes"] - 1], axis=1))
    np.testing.assert_allclose(w["out"]["length"], np.sqrt(((c.pf - c.p0) ** 2).sum(axis=1)), rtol=1e-15)


def test_struct_layout_matches_the_header(tmp_path):
    from path_planning import _hip

    names = ["n_kept", "n_vertices", "length", "length_before"]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "scp_hip.h"\nint main(void) {\n'
                   'printf("%zu %zu %zu %zu %zu\\n", sizeof(scp_shorten_info), ' +
                   ", ".join(f"offsetof(scp_shorten_info, {f})" for f in names) + ');\nreturn 0; }\n')
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.dirname(HEADER), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    S = _hip.ShortenInfo
    assert got == [ctypes.sizeof(S)] + [getattr(S, f).offset for f in names] == [24, 0, 4, 8, 16]
    assert _hip.SHORTEN_INFO_DTYPE == sr.SHORTEN_INFO_DTYPE and _hip.SHORTEN_INFO_DTYPE.itemsize == 24
    assert [_hip.SHORTEN_INFO_DTYPE.fields[f][1] for f in names] == got[1:]


def test_python_surface():
    from path_planning import _hip
    from path_planning.cli import compute_trajectories as ct
    from path_planning.solvers.scp import SCP

    sig = inspect.signature(SCP.shorten_reference)
    assert [(k, p.default) for k, p in sig.parameters.items()][1:] == [("stride", None), ("clearance", None), ("max_path", None),
                                                                       ("allow_unreachable", False)]
    with open(HEADER) as f:
        text = f.read()
    assert "int scp_shorten_paths(" in text and "scp_shorten_paths" in _hip.EXPORTS
    assert hasattr(ctypes.CDLL(_hip.library_path()), "scp_shorten_paths") and callable(_hip.Context.shorten_paths)
    assert '"shorten_threads"' in text

    # set_corridors(reference="shortened") goes through shorten_reference with its defaults; "search" still through
    # find_reference; any other string is an error
    class OneRank:
        world = 1

    class TwoRanks:
        world = 2

    s = SCP.__new__(SCP)
    s.shard = OneRank()
    calls = []

    def fake(*a, **kw):
        calls.append((a, kw))
        raise RuntimeError("shorten_reference was called")

    s.shorten_reference = fake
    with pytest.raises(RuntimeError, match="shorten_reference was called"):
        s.set_corridors(reference="shortened")
    assert calls == [((), {})]
    for other in ("straight", "shorten", ""):
        with pytest.raises(ValueError, match="shortened"):
            s.set_corridors(reference=other)
    del s.shorten_reference
    s._obstacles = None
    with pytest.raises(ValueError, match="set_obstacles"):
        s.shorten_reference()
    s.shard = TwoRanks()
    with pytest.raises(ValueError, match="one rank"):
        s.shorten_reference()

    parser = ct.build_parser()
    args = parser.parse_args(["--obstacle-discs", "5,5,1", "--corridor-search", "--corridor-shorten"])
    assert args.corridor_shorten and args.corridor_clearance is None and ct.obstacle_discs(parser, args) == [(5.0, 5.0, 1.0)]
    assert not parser.parse_args([]).corridor_shorten
    for argv in (["--corridor-shorten"], ["--obstacle-discs", "5,5,1", "--corridor-shorten"],
                 ["--obstacle-discs", "5,5,1", "--corridor-shorten", "--corridor-clearance", "1"]):
        with pytest.raises(SystemExit):
            ct.obstacle_discs(parser, parser.parse_args(argv))
    fr = {"status": np.array([0, 3]), "n_kept": np.array([4, 0]), "n_nodes": np.array([17, 0]), "length": np.array([8.5, 0.0]),
          "length_before": np.array([9.25, 0.0]), "shorten_ms": 0.25}
    assert ct.shortened_summary(fr) == "; shortened to 4 of 17 nodes, total length 8.50 m (lattice paths 9.25 m), 0.250 ms"
