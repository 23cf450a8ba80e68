"""Goal assignment without a GPU: the promises of the numpy restatement (tests/assignment_ref.py) that the GPU tests compare
the kernels against bit for bit, the C-ABI surface, the struct layouts and the host-side behaviour of the new entry points."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import assignment_ref as R  # noqa: E402

HEADER = os.path.join(ROOT, "include", "scp_hip.h")


def _small_cases():
    """200 seeded cases with N <= 7 in 2-D and 3-D; every fifth on integer points (ties)"""
    rng = np.random.default_rng(2024)
    for k in range(200):
        N, D = int(rng.integers(1, 8)), 2 + k % 2
        s, g = rng.uniform(0.0, 10.0, (N, D)), rng.uniform(0.0, 10.0, (N, D))
        if k % 5 == 0:
            s, g = np.round(s), np.round(g)
        yield s, g


def test_reference_equals_brute_force():
    for s, g in _small_cases():
        r = R.auction(s, g)
        assert r["status"] == 0 and sorted(r["goal_of"].tolist()) == list(range(len(s)))
        assert r["cost_q"] == R.brute_force(r["c"]), (s, g)
        assert r["eps_last"] == 1 or len(s) == 1  # (N = 1: no phase at all)


@pytest.mark.parametrize("N", [64, 65, 257])
def test_reference_equals_scipy_optimum(N):
    lsa = pytest.importorskip("scipy.optimize").linear_sum_assignment
    for D in (2, 3):
        s, g = R.uniform(N, D, 77 + N + D)
        r = R.auction(s, g)
        row, col = lsa(r["c"])
        assert r["cost_q"] == int(r["c"][row, col].sum())
        # in metres^2: within N quanta of the optimum of the unquantised costs
        d2 = ((s[:, None, :] - g[None, :, :]) ** 2).sum(-1)
        row, col = lsa(d2)
        assert d2[np.arange(N), r["goal_of"]].sum() <= d2[row, col].sum() + N * r["quantum"] * (1 + 1e-9)


def _check_consequences(r):
    c, p, phi = r["c"], r["prices"], r["goal_of"]
    N = c.shape[0]
    idx = np.arange(N)
    a = -(N + 1) * c
    # (b) eps-complementary slackness with eps = 1
    assert (a[idx, phi] - p[phi] >= (a - p[None, :]).max(1) - 1).all()
    # (c) no pair gains by swapping its goals
    own = c[idx, phi]
    assert (own[:, None] + own[None, :] <= c[:, phi].T + c[:, phi]).all()
    # (d)
    assert 0 <= p.min() and int(p.max()) < 2 ** 55


def test_consequences_on_small_cases():
    for s, g in _small_cases():
        if len(s) >= 2:
            _check_consequences(R.auction(s, g))


@pytest.mark.parametrize("name", sorted(R.gpu_cases()))
def test_gpu_cases_stay_inside_the_guard(name):
    s, _ = R.gpu_cases()[name]
    r = R.reference(name)
    N = len(s)
    assert r["status"] == 0 and r["longest_phase"] <= 256 * N + 4096
    assert sorted(r["goal_of"].tolist()) == list(range(N))
    if N >= 2:
        _check_consequences(r)
    assert (r["phases"] == 0) == (N == 1) and r["phases"] <= 25


def test_known_answers():
    s, g = R.reversed_lines(8)
    r = R.auction(s, g)
    assert r["goal_of"].tolist() == list(range(7, -1, -1))
    assert R.line_check(s, g, None, 0.5)["n_opposed"] == 28 and R.line_check(s, g, r["goal_of"], 0.5)["n_opposed"] == 0
    assert R.line_check(s, g, None, 0.5)["min_approach"] < 1e-12  # all eight lines meet at (7, 5)
    s, g = R.optimal_identity()
    assert R.auction(s, g)["goal_of"].tolist() == list(range(len(s)))
    s, g = R.identical_points()
    r = R.auction(s, g)
    assert (r["phases"], r["cost_q"], r["quantum"]) == (1, 0, 1.0)
    s, g = R.identical_goals(64)
    r = R.auction(s, g, max_rounds_per_phase=1)
    assert r["status"] == 1 and r["goal_of"].tolist() == list(range(64)) and r["cost_q"] == r["cost_q_identity"]


def test_line_check_reference_matches_host_function():
    from path_planning.scenarios.position_generator import straight_line_min_distance

    for D in (2, 3):
        s, g = R.uniform(50, D, 5 + D)
        lc = R.line_check(s, g, None, 1.0)
        d = straight_line_min_distance(s, g)
        assert abs(lc["min_approach"] - d.min()) <= 1e-12 * max(1.0, d.min())
        assert (lc["arg_i"], lc["arg_j"]) == tuple(int(v) for v in np.unravel_index(np.argmin(d), d.shape))
        assert lc["n_close"] == int((d[np.triu_indices(50, 1)] < 1.0).sum())


def test_header_and_exports_carry_the_two_names():
    from path_planning import _hip

    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r"\b(scp_[a-z0-9_]+)\s*\(", text))
    lib = ctypes.CDLL(_hip.library_path())
    for name in ("scp_assign_goals", "scp_straight_line_check"):
        assert name in declared and name in _hip.EXPORTS and hasattr(lib, name), name
    assert lib.scp_abi_version() == _hip.ABI_VERSION == 7
    assert "#define SCP_ABI_VERSION 7" in open(HEADER).read()


def test_structs_match_the_header(tmp_path):
    from path_planning import _hip

    fields = {"scp_assign_stats": (_hip.AssignStats, _hip.ASSIGN_STATS_DTYPE,
                                   ["cost_q", "cost_q_identity", "quantum", "rounds", "bids", "phases", "status"]),
              "scp_line_stats": (_hip.LineStats, _hip.LINE_STATS_DTYPE,
                                 ["min_approach", "arg_i", "arg_j", "n_close", "n_opposed"])}
    src = ['#include <stddef.h>', '#include <stdio.h>', '#include "scp_hip.h"', "int main(void) {"]
    for name, (_, _, fs) in fields.items():
        src.append(f'  printf("{name} %zu", sizeof({name}));')
        for f in fs:
            src.append(f'  printf(" %zu", offsetof({name}, {f}));')
        src.append('  printf("\\n");')
    src.append("  return 0; }")
    c = tmp_path / "assign_layout.c"
    c.write_text("\n".join(src))
    exe = tmp_path / "assign_layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split("\n")
    got = {ln.split()[0]: [int(v) for v in ln.split()[1:]] for ln in out if ln.strip()}
    assert got["scp_assign_stats"][0] == 48 and got["scp_line_stats"][0] == 32
    for name, (cls, dtype, fs) in fields.items():
        assert got[name] == [ctypes.sizeof(cls)] + [getattr(cls, f).offset for f in fs], name
        assert dtype.itemsize == got[name][0] and [dtype.fields[f][1] for f in fs] == got[name][1:], name


def test_cli_parsers_accept_assign_goals():
    from path_planning.cli import compute_trajectories, compute_trajectories_batch

    assert compute_trajectories.build_parser().parse_args(["--assign-goals"]).assign_goals is True
    assert compute_trajectories.build_parser().parse_args([]).assign_goals is False
    assert compute_trajectories_batch.build_parser().parse_args(["--assign-goals", "--Ns", "16"]).assign_goals is True
    assert compute_trajectories_batch.build_parser().parse_args([]).assign_goals is False


def test_no_cpu_fallback():
    import torch

    from path_planning import _hip
    from path_planning.scenarios import assign_goals, assign_goals_batch

    s, g = R.reversed_lines(8)
    if torch.cuda.is_available():  # (then the same call answers)
        assert assign_goals(s, g)[0].tolist() == list(range(7, -1, -1))
        return
    with pytest.raises(_hip.HipError):
        assign_goals(s, g)
    with pytest.raises(_hip.HipError):
        assign_goals_batch(s[None], g[None])
