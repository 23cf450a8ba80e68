"""CPU checks of the delay margins: header / exports / ctypes struct; the numpy reference the GPU tests compare against
(tests/delay_ref.py) pinned against the clearance reference -- at lag 0 on the fleet as it is, at every lag on the fleet shifted by
hand --, against dense sampling and against the analytic crossing case; the argument checks of validate_solution."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import clearance_ref as clr  # noqa: E402
import delay_ref as dr  # noqa: E402
import separation_ref as sr  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "scp_hip.h")
H, R = 0.2, 0.8
_CASES = {}


def case(N, K, D, seed, S):
    """host trajectories of a random case and its delay reference, made once"""
    key = (N, K, D, seed, S)
    if key not in _CASES:
        p0, v0, acc = sr.random_case(N, K, D, seed)
        pos, vel = sr.kinematics(p0, v0, acc, H)
        _CASES[key] = ((pos, vel, acc), dr.margins(pos, vel, acc, H, R, S))
    return _CASES[key]


def decode(row, pairs, N, a):
    """a row of the clearance profile's entry of vehicle a -> (segment, partner)"""
    i, j = sr.pair_indices(N)
    k, q = divmod(int(row), pairs)
    assert a in (i[q], j[q])
    return k, int(j[q] if i[q] == a else i[q])


# ---- surface ------------------------------------------------------------------------------------------------------------------------
def test_abi_header_export_and_struct(tmp_path):
    from path_planning import _hip

    text = open(HEADER).read()
    for sym in ("scp_delay_margins", "scp_ctx_last_delay_solved"):
        assert sym in text and sym in _hip.EXPORTS and hasattr(ctypes.CDLL(_hip.library_path()), sym)
    assert "#define SCP_ABI_VERSION 7" in text and _hip.ABI_VERSION == 7  # additive: the version stays
    assert "typedef struct scp_delay_margin {" in text and "a purely additive part of abi version 7" in text.lower()
    names = [f for f, _ in _hip.DelayMargin._fields_]
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "scp_hip.h"\nint main(void){printf("%zu", sizeof(scp_delay_margin));\n'
                   + "".join(f'printf(" %zu", offsetof(scp_delay_margin, {f}));\n' for f in names) + "return 0;}\n")
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", os.path.dirname(HEADER), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    S = _hip.DelayMargin
    assert got == [ctypes.sizeof(S)] + [getattr(S, f).offset for f in names] == [32, 0, 8, 16, 20, 24]
    assert _hip.DELAY_DTYPE.itemsize == 32 and list(_hip.DELAY_DTYPE.names) == names
    assert [_hip.DELAY_DTYPE.fields[f][1] for f in names] == got[1:]


def test_python_surface():
    import inspect

    from path_planning import _hip
    from path_planning.cli import compute_trajectories, compute_trajectories_batch
    from path_planning.solvers.scp import SCP
    from path_planning.viz.plot_trajectories import plot_delay_margin

    sig = inspect.signature(SCP.validate_solution)
    assert list(sig.parameters) == ["self", "continuous", "conflicts", "clearance", "delay"]
    assert sig.parameters["delay"].default is None
    assert "delay_margins" in dir(_hip.Context) and "last_delay_solved" in dir(_hip.Context)
    assert callable(plot_delay_margin)
    for cli in (compute_trajectories, compute_trajectories_batch):
        assert cli.build_parser().parse_args(["--delay-tolerance", "3"]).delay_tolerance == 3
        assert cli.build_parser().parse_args([]).delay_tolerance is None
    assert "delay_tolerance" not in compute_trajectories_batch.CONFIG


# ---- the reference against the clearance reference ----------------------------------------------------------------------------------
@pytest.mark.parametrize("N,K,D,seed", [(7, 13, 3, 12), (65, 7, 2, 17)])
def test_reference_at_lag_0_is_the_clearance_reference(N, K, D, seed):
    host, ref = case(N, K, D, seed, 2)
    prof = clr.profile(*host, H, R)
    veh = prof["vehicle"]
    for a in range(N):
        assert ref["f"][a, 0] == veh["f"][a] and ref["t"][a, 0] == veh["t"][a]
        assert ref["second_f"][a, 0] == veh["second_f"][a]
        assert ref["n_violating"][a, 0] == veh["n_violating"][a]
        assert (int(ref["g"][a, 0]), int(ref["b"][a, 0])) == decode(veh["row"][a], prof["pairs"], N, a)


def test_reference_at_every_lag_is_the_clearance_reference_of_the_shifted_fleet():
    N, K, D, seed = 7, 13, 3, 12
    host, ref = case(N, K, D, seed, K)
    checked = 0
    for a in range(N):
        for s in range(K + 1):
            fleet = dr.shifted_fleet(*host, H, a, s)
            assert fleet[0].shape == (N, K + s, D)
            prof = clr.profile(*fleet, H, R)
            veh = prof["vehicle"]
            assert ref["f"][a, s] == veh["f"][a] and ref["t"][a, s] == veh["t"][a]
            assert ref["second_f"][a, s] == veh["second_f"][a]
            assert ref["n_violating"][a, s] == veh["n_violating"][a]
            assert (int(ref["g"][a, s]), int(ref["b"][a, s])) == decode(veh["row"][a], prof["pairs"], N, a)
            checked += 1
    assert checked == N * (K + 1)


def test_shifted_fleet_holds_parks_and_reproduces_pk():
    N, K, D, seed = 7, 13, 3, 12
    (pos, vel, acc), _ = case(N, K, D, seed, K)
    pK = pos[:, K - 1] + (H * vel[:, K - 1] + (0.5 * H * H) * acc[:, K - 1])
    p, v, a = dr.shifted_fleet(pos, vel, acc, H, 2, 3)
    assert (p[2, :3] == pos[2, 0]).all() and not v[2, :3].any() and not a[2, :3].any()
    assert (p[2, 3:] == pos[2]).all() and (v[2, 3:] == vel[2]).all() and (a[2, 3:] == acc[2]).all()
    others = [i for i in range(N) if i != 2]
    assert (p[others, :K] == pos[others]).all() and (p[others, K:] == pK[others, None]).all()
    assert not v[others, K:].any() and not a[others, K:].any()
    same = dr.shifted_fleet(pos, vel, acc, H, 2, 0)
    assert all((x == y).all() for x, y in zip(same, (pos, vel, acc)))


def test_reference_against_dense_sampling():
    N, K, D, seed, S = 7, 13, 3, 12, 13
    host, ref = case(N, K, D, seed, S)
    P, V, A = dr.records(*host, H)
    worst = 0.0
    for a in range(N):
        for s in (0, 1, 6, S):
            g = np.arange(K + s)
            for b in range(N):
                if b == a:
                    continue
                ra, rb = np.maximum(g - s, -1) + 1, np.minimum(g, K) + 1
                d, w, bb = P[a, ra] - P[b, rb], V[a, ra] - V[b, rb], A[a, ra] - A[b, rb]
                dense, slack = sr.dense_minima(d, w, bb, H)
                f = ref["seg_f"][a][s, :K + s, b]
                tol = 32 * sr.EPS * ref["s_max"] ** 2
                assert (f <= dense + tol).all() and (f >= dense - slack - tol).all()
                worst = max(worst, float((dense - f).max()))
            assert np.isinf(ref["seg_f"][a][s, K + s:]).all() and np.isinf(ref["seg_f"][a][s, :, a]).all()
            assert ref["f"][a, s] == ref["seg_f"][a][s].min()
    print(f"dense sampling lies at most {worst:.3e} above the reference")


# ---- the crossing case, analytic ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,D,pair", [(2, 2, (0, 1)), (6, 2, (2, 4)), (7, 3, (3, 6))])
def test_crossing_case_reference(N, D, pair):
    pos, vel, acc = dr.crossing_case(N, D, pair)
    a, b = pair
    ref = dr.margins(pos, vel, acc, dr.CROSS_H, dr.CROSS_R, 6)
    for s in range(7):
        assert abs(np.sqrt(max(ref["f"][a, s], 0.0)) - dr.crossing_margin(s)) <= 1e-12
        assert ref["b"][a, s] == b
        time = ref["g"][a, s] * dr.CROSS_H + ref["t"][a, s]  # halfway between the two passages of the origin
        assert abs(time - (1.1 + 0.1 * s)) <= 1e-6
    assert ref["f"][a, 3] <= 32 * sr.EPS * ref["s_max"] ** 2
    viol = ref["n_violating"][a] > 0
    assert viol.tolist() == [False, False, True, True, True, False, False]  # 0.49 lies between 0.283 and 0.566
    steps = int(np.argmax(viol)) - 1
    assert steps == 1 and ref["b"][a, steps + 1] == b
    # the other vehicle of the pair, late: they cross 3 + s steps apart
    for s in range(7):
        assert abs(np.sqrt(ref["f"][b, s]) - 0.2 * np.sqrt(2.0) * (3 + s)) <= 1e-12 and ref["n_violating"][b, s] == 0
    rest = [v for v in range(N) if v not in pair]
    assert not ref["n_violating"][rest].any() and (np.sqrt(ref["f"][rest]) > 5.0).all()


# ---- argument checks of validate_solution -------------------------------------------------------------------------------------------
class _NoDevice:
    """a context that must not be reached: the argument checks come first"""

    def __getattr__(self, name):
        raise AssertionError(f"the context was asked for {name}")


def test_validate_solution_argument_checks():
    from path_planning.solvers.scp import SCP

    s = SCP.__new__(SCP)
    s.N, s.K, s.D, s.h, s.R = 2, 5, 2, 0.5, 0.8
    z = np.zeros((2, 5, 2))
    s.trajectories = {"positions": z, "velocities": z, "accelerations": z}
    s._ctx = _NoDevice()
    for kw in ({"delay": 2}, {"delay": 0}, {"continuous": False, "delay": 2}):
        with pytest.raises(ValueError, match="continuous=True"):
            s.validate_solution(**kw)
    for bad in (-1, 6, 2.0, "2", True, [1]):
        with pytest.raises(ValueError, match="delay="):
            s.validate_solution(continuous=True, delay=bad)
    with pytest.raises(ValueError, match="clearance=True"):  # the older switch keeps its message
        s.validate_solution(clearance=True, delay=2)
