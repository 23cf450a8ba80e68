"""Case table of the persistent single-step ADMM kernels (settings.persistent) and what tests need around it.

Not a conftest: tests/test_persist_cases_cpu.py checks on the CPU that every case reaches the edge it claims, and
tests/test_persist_iterates_gpu.py runs every case on its kernel and compares the state after m ADMM steps with the oracle
(oracle/qp_oracle.py, admm_structured(snapshots=...)).

A case is one joint QP (scenario, N, K = T / h, dim, working-set margin around the oracle's QP#0 solution) on one kernel:

  persistent  kernel                           agents per workgroup      info["pipeline"]
  4           cg1_persist_kernel<2> / <3>      8 (2-D) / 4 (3-D)         persistent
  3           cg1_persist16_kernel<2,8>/<3,8>  8                         persistent8-lean
  2           cg1_persist16_kernel<2,16>       16 (2-D only)             persistent16
  0           three-launch pipeline (control)  -                         three-launch

Each case states the edge it is there for: N mod agents-per-workgroup (`n_tail`, 1 = a one-agent last workgroup, 0 = a
full one) and K mod 16 (`k_tail`: the last 16-column MFMA tile of the K dimension).
"""
from __future__ import annotations

import dataclasses
import functools

import numpy as np

from oracle import qp_oracle as qo
from oracle import scp_oracle as so

H = 0.2
R = 0.8
LIMITS = [-2.0, 2.0, -15.0, 15.0, -20.0, 20.0]  # vel, acc, jerk bounds of the reference (scp.py:188-195)
STEPS = (1, 2, 6, 7, 12)  # m = 1: the lean kernels' first step; 6 / 7: on and just past a check (check_termination = 6)
CHECK = 6
PIPELINE = {4: "persistent", 3: "persistent8-lean", 2: "persistent16", 0: "three-launch"}
KERNEL_NAME = {4: "cg1_persist_kernel<{D}>", 3: "cg1_persist16_kernel<{D},8>", 2: "cg1_persist16_kernel<2,16>",
               0: "three-launch"}
TOL_REL = 1e-11  # |gpu - oracle| <= 1e-11 * max(1, |oracle|_max), per array


def apb(kernel, D):
    """agents per workgroup of a kernel"""
    return {4: 8 if D == 2 else 4, 3: 8, 2: 16}[kernel]


def kernel_name(kernel, D):
    return KERNEL_NAME[kernel].format(D=D)


@dataclasses.dataclass(frozen=True)
class Scenario:
    gen: str      # "circle": generate_positions (2-D); "grid": generate_grid_swap; "near": short moves on a lattice
    seed: int
    N: int
    K: int
    dim: int
    margin: float = 0.5  # working set: rows with dist - R < margin at the QP#0 solution
    qp0_iters: int = 4000  # cap of the oracle's QP#0 run behind x0 (long horizons: any x0 is a valid start)

    @property
    def T(self):
        return self.K * H + 1e-9

    @property
    def label(self):
        return f"{self.gen}{self.dim}d-N{self.N}-K{self.K}-s{self.seed}"


@dataclasses.dataclass(frozen=True)
class Case:
    scen: Scenario
    kernel: int   # settings.persistent
    n_tail: int   # claimed N mod agents-per-workgroup
    k_tail: int   # claimed K mod 16
    steps: tuple = STEPS

    @property
    def pipeline(self):
        return PIPELINE[self.kernel]

    @property
    def id(self):
        return f"p{self.kernel}-{self.scen.label}"


def _near(N, K, dim, seed):
    """Agents on a jittered lattice (pitch 1 m) with goals a short move away -- reachable even at K = 3 (as
    tests/test_scp_gpu.py::test_edge_sizes) -- so that neighbours come within R of each other."""
    rng = np.random.default_rng(seed)
    side = int(np.ceil(N ** (1.0 / dim)))
    cells = np.stack(np.meshgrid(*[np.arange(side)] * dim, indexing="ij"), -1).reshape(-1, dim)[:N]
    pitch, jitter, move = (0.85, 0.02, 0.15) if K < 10 else (0.95, 0.05, 0.6)
    p0 = 2.0 + cells * pitch + rng.uniform(-jitter, jitter, (N, dim))
    pf = p0 + rng.uniform(-move, move, (N, dim))
    space = [0.0] * dim + [2.0 + side + 2.0] * dim
    return p0, pf, space


def make_problem(scen: Scenario):
    if scen.gen == "circle":
        from path_planning.scenarios.position_generator import generate_positions

        assert scen.dim == 2
        p0, pf = generate_positions(scen.N, R, seed=scen.seed)
        space = [0, 0, 20, 20]
    elif scen.gen == "grid":
        from path_planning.scenarios.position_generator import generate_grid_swap

        p0, pf, space = generate_grid_swap(scen.N, seed=scen.seed, dim=scen.dim)
    else:
        p0, pf, space = _near(scen.N, scen.K, scen.dim, scen.seed)
    prob = so.make_problem(scen.N, scen.T, H, R, space, p0, pf)
    assert prob.K == scen.K
    return prob


@functools.lru_cache(maxsize=None)
def setup(scen: Scenario):
    """(prob, x0, eta, l_col, dist, W): the QP#0 solution of the oracle, the linearisation there and the working set"""
    prob = make_problem(scen)
    x0, _, _ = qo.admm_structured(prob, st=qo.Settings(eps_abs=1e-6, eps_rel=1e-6, max_iter=scen.qp0_iters))
    pos, _ = so.kinematics(prob, x0)
    eta, l_col, dist = so.linearize_pairs(prob, pos)
    W = np.nonzero(dist - prob.R < scen.margin)[0].astype(np.int64)
    return prob, x0, eta, l_col, dist, W


def step_settings(max_iter, **kw):
    """oracle settings of the step-level comparison (the GPU side: gpu_step_settings)"""
    base = dict(cg_iters=1, max_iter=max_iter, check_termination=CHECK, adaptive_rho=False, eps_abs=1e-12, eps_rel=1e-12,
                max_rounds=1)
    base.update(kw)
    return qo.Settings(**base)


def gpu_step_settings(kernel, max_iter, **kw):
    base = dict(cg_iters=1, persistent=kernel, max_iter=max_iter, check_termination=CHECK, adaptive_rho=0, eps_abs=1e-12,
                eps_rel=1e-12)
    base.update(kw)
    return base


def oracle_snapshots(scen: Scenario, steps=STEPS, l_col=None, rows=None, zero_qx=None, **settings):
    """{m: oracle state after m steps} (one oracle run up to max(steps)) and its info; rows: a working set other than the
    scenario's; zero_qx: the oracle's deliberate fault; settings: over step_settings"""
    prob, x0, eta, l0, dist, W = setup(scen)
    snaps = {}
    _, _, info = qo.admm_structured(prob, eta, l0 if l_col is None else l_col, dist, x0=x0,
                                    st=step_settings(max(steps), **settings), rows0=W if rows is None else rows,
                                    snapshots=set(steps), snap_out=snaps, zero_qx=zero_qx)
    return snaps, info


@functools.lru_cache(maxsize=None)
def cached_snapshots(scen: Scenario, steps=STEPS):
    return oracle_snapshots(scen, steps)


# ---- state in the solver's time-major layout (scp_qp_peek) --------------------------------------------------------------
def time_major(a):
    """(N, K', D) -> [K'][N*D] (column i*D + d)"""
    N, Kp, D = a.shape
    return np.ascontiguousarray(a.transpose(1, 0, 2)).reshape(Kp, N * D)


def fixed_time_major(blocks):
    """(jerk, acc, vel, pos) -> [4K-1][C], the layout of "zf", "yf", "fx" """
    return np.concatenate([time_major(b) for b in blocks], axis=0)


def reference_arrays(prob, snap, order=None):
    """the arrays scp_qp_peek returns, from an oracle snapshot; `order`: positions of the GPU's rows in snap["rows"]"""
    ops = qo.FixedOps(prob.K, prob.h)
    x = snap["x"]
    zc, yc = snap["zc"], snap["yc"]
    if order is not None:
        zc, yc = zc[order], yc[order]
    return {
        "x": time_major(x).ravel(),
        "zf": fixed_time_major(snap["zf"]).ravel(),
        "yf": fixed_time_major(snap["yf"]).ravel(),
        "fx": fixed_time_major(ops.apply(x)).ravel(),
        "qx": time_major(np.einsum("km,imd->ikd", ops.S0, x)).ravel(),
        "zc": zc,
        "yc": yc,
    }


def tolerances(prob, ref, rho, floor=0.0, st=None):
    """Per-entry tolerance of every compared array: 1e-11 * max(1, |ref|_max) (at least `floor`).  A dual moves rho_row times
    any difference in its z: y' = y + rho_row (z^ - z'), with rho_row = rho x 1e3 on the final-state equality rows and
    rho x 10 on collision rows.  So y is also allowed rho_row times the tolerance of its z -- the equality-row duals are
    1e3 x worse conditioned than the other fixed rows, and at rho = 0.1 their rounding alone reaches 1e-11 * |y|_max
    (2-D N = 17, K = 50, m = 6: 1.007 x on every pipeline, the three-launch one included)."""
    st = st or qo.Settings()
    K, C = prob.K, prob.N * prob.D
    tol = {k: max(TOL_REL * max(1.0, np.abs(v).max(initial=0.0)), floor) for k, v in ref.items()}
    rr = np.full((4 * K - 1, C), rho)
    rr[(K - 1) + K + K - 1] = rr[(K - 1) + 3 * K - 1] = rho * st.rho_eq_scale  # vel / pos at k = K - 1
    out = {k: np.full(np.shape(v), tol[k]) for k, v in ref.items()}
    out["yf"] = np.maximum(out["yf"], rr.ravel() * tol["zf"])
    out["yc"] = np.maximum(out["yc"], rho * st.rho_col_scale * tol["zc"])
    return out


def where(prob, name, idx, rows=None):
    """an index of a peeked array in words: (agent, time step, axis) or (row id, agent pair, time step)"""
    N, K, D = prob.N, prob.K, prob.D
    C = N * D
    if name in ("zc", "yc"):
        r = int(rows[idx])
        k, i, j = qo.working_rows(prob, np.array([r]))
        return f"row {r} (agents {int(i[0])}-{int(j[0])}, k={int(k[0])})"
    t, c = divmod(int(idx), C)
    a, d = divmod(c, D)
    if name in ("x", "qx"):
        return f"agent {a}, k={t}, axis {d}"
    for blk, n in (("jerk", K - 1), ("acc", K), ("vel", K), ("pos", K)):
        if t < n:
            return f"{blk} row k={t}, agent {a}, axis {d}"
        t -= n
    raise IndexError(idx)


def block_entries(prob, W, per):
    """incident rows of every block of `per` agents (a row joins two agents: it is counted once at each end)"""
    _, wi, wj = qo.working_rows(prob, np.asarray(W, dtype=np.int64))
    nb = (prob.N + per - 1) // per
    return np.bincount(wi // per, minlength=nb) + np.bincount(wj // per, minlength=nb)


def _pad_col(n):
    return ((n + 29) // 32) * 32 + 2


def entry_cap(kernel, N, K, D):
    """LDS entry capacity of a persistent launch: the formula of scp_qp_cg1_persist (csrc/scp_qp_persist.hip) with the
    LDS carve-ups of persist_lds_bytes and Lds16 (csrc/scp_qp_persist16.hip).  A block of agents with more incident rows
    makes the kernel leave with EXIT_OVERFLOW (three-launch pipeline for that working set)."""
    per = apb(kernel, D)
    nb = (N + per - 1) // per + 1
    lean = kernel != 4
    NCHK, CB = 9, 16
    ints = per * K + 1
    if lean:
        nc16 = 16 * ((D * per + 15) // 16)
        rsk, tk, nks = _pad_col(K), (K + 15) >> 4, (K + 3) >> 2
        dbl = 2 * nc16 * rsk + tk * nks * 64 + 2 * nb + per * 32
        if 2 * nc16 * rsk < NCHK * nb:
            dbl += NCHK * nb
    else:
        dbl = 3 * CB * _pad_col(K) + per * 64 * D + NCHK * nb
    fixed = dbl * 8 + ((ints + 1) // 2 * 2) * 4
    per_entry = (4 * D + 4) * 8 + (1 if lean else 3) * 4
    budget = 160 * 1024 - (2048 if lean else 1024)
    return (budget - fixed) // per_entry // 64 * 64


# ---- the table -------------------------------------------------------------------------------------------------------
# (scenario, {kernel: claimed N mod agents-per-workgroup}, claimed K mod 16).  Seeds and margins were chosen with the oracle
# so that every case has working rows across workgroups (where N > agents per workgroup), a row at the last agent that is
# active (A x < l) at every compared step, and a working set within the kernel's LDS entry capacity; the CPU suite checks
# all of it.
def _s(gen, seed, N, K, dim, margin=0.5):
    return Scenario(gen, seed, N, K, dim, margin)


TABLE_2D = [
    # K = 50: full workgroups, one agent over, one-agent tails                     4: N%8  3: N%8  2: N%16
    (_s("circle", 16, 2, 50, 2), {4: 2, 3: 2, 2: 2}, 2),
    (_s("circle", 7, 7, 50, 2), {4: 7, 3: 7, 2: 7}, 2),
    (_s("circle", 1, 8, 50, 2, 1.0), {4: 0, 3: 0, 2: 8}, 2),
    (_s("circle", 9, 9, 50, 2), {4: 1, 3: 1, 2: 9}, 2),
    (_s("circle", 15, 15, 50, 2), {4: 7, 3: 7, 2: 15}, 2),
    (_s("circle", 2, 16, 50, 2), {4: 0, 3: 0, 2: 0}, 2),
    (_s("circle", 17, 17, 50, 2), {4: 1, 3: 1, 2: 1}, 2),
    (_s("circle", 1, 33, 50, 2), {4: 1, 3: 1, 2: 1}, 2),
    # N = 9 and 17: every K tile edge (K mod 16 = 3, 15, 0, 1, 1, 15, 0)
    (_s("near", 2036, 9, 3, 2), {4: 1, 3: 1, 2: 9}, 3),
    (_s("near", 115, 9, 15, 2), {4: 1, 3: 1, 2: 9}, 15),
    (_s("near", 2161, 9, 16, 2), {4: 1, 3: 1, 2: 9}, 0),
    (_s("near", 2171, 9, 17, 2), {4: 1, 3: 1, 2: 9}, 1),
    (_s("near", 2333, 9, 33, 2), {4: 1, 3: 1, 2: 9}, 1),
    (_s("near", 2631, 9, 63, 2, 0.2), {4: 1, 3: 1, 2: 9}, 15),
    (_s("near", 2642, 9, 64, 2, 0.1), {4: 1, 3: 1, 2: 9}, 0),
    (_s("near", 2042, 17, 3, 2), {4: 1, 3: 1, 2: 1}, 3),
    (_s("near", 2151, 17, 15, 2), {4: 1, 3: 1, 2: 1}, 15),
    (_s("near", 116, 17, 16, 2), {4: 1, 3: 1, 2: 1}, 0),
    (_s("near", 117, 17, 17, 2), {4: 1, 3: 1, 2: 1}, 1),
    (_s("near", 2337, 17, 33, 2, 0.2), {4: 1, 3: 1, 2: 1}, 1),
    (_s("near", 2634, 17, 63, 2, 0.0), {4: 1, 3: 1, 2: 1}, 15),
    (_s("near", 2642, 17, 64, 2, 0.05), {4: 1, 3: 1, 2: 1}, 0),
]
TABLE_3D = [
    # kernel 4: 4 agents per workgroup; kernel 3: 8                                 4: N%4  3: N%8
    (_s("near", 3504, 3, 50, 3), {4: 3}, 2),
    (_s("near", 3501, 4, 50, 3), {4: 0}, 2),
    (_s("near", 3502, 5, 50, 3, 0.3), {4: 1, 3: 5}, 2),
    (_s("near", 3501, 7, 50, 3, 0.2), {3: 7}, 2),
    (_s("near", 3513, 8, 50, 3, 0.2), {3: 0}, 2),
    (_s("near", 3501, 9, 50, 3, 0.2), {4: 1, 3: 1}, 2),
    (_s("near", 3501, 17, 50, 3, 0.05), {3: 1}, 2),
    (_s("near", 3165, 5, 16, 3), {4: 1, 3: 5}, 0),
    (_s("near", 3171, 5, 17, 3), {4: 1, 3: 5}, 1),
    (_s("near", 3642, 5, 64, 3, 0.3), {4: 1, 3: 5}, 0),
    (_s("near", 3161, 9, 16, 3), {4: 1, 3: 1}, 0),
    (_s("near", 3176, 9, 17, 3), {4: 1, 3: 1}, 1),
    (_s("near", 3647, 9, 64, 3, 0.1), {4: 1, 3: 1}, 0),
]
# 2-D, N = 17, K = 50: also the shape of the longer runs (adaptive rho switches at step 50)
RHO_2D = TABLE_2D[6][0]
CASES = [Case(sc, kern, tail, kt) for sc, tails, kt in TABLE_2D + TABLE_3D for kern, tail in tails.items()]
SCENARIOS = [sc for sc, _, _ in TABLE_2D + TABLE_3D]
