"""Case table of the ADMM pipelines beyond the persistent kernels, and of the per-rho KKT blocks.

Not a conftest: tests/test_pipeline_cases_cpu.py checks on the CPU that every case reaches the edge it claims, and
tests/test_pipeline_iterates_gpu.py runs every case and compares the state after m ADMM steps with the oracle
(oracle/qp_oracle.py, admm_structured(snapshots=...)).  Scenarios, layouts, tolerances and the oracle settings are those of
tests/persist_cases.py (`pc`); this file only adds the table and what the other pipelines need around it.

  group  info["pipeline"]    what runs                                                     K
  A      three-launch        cg1_col_kernel<2>, cg1_resid_col_kernel<2> (16-column blocks)  65 .. 120
  B      three-launch-bigK   cg1_colK_kernel (one workgroup per column), generic check      121 .. 1024
  C      generic             one product per launch: cg_iters > 1, use_mfma 0 / 2           any
  D      qp0                 qp0_col_kernel<1> / <2>: no rows, all steps up to a check      <= 120
                                                                          in one launch

`band(K)` names the side of the thresholds 64 (one / two time steps per lane), 96 (SCP_INV_LDS_MAX_K: LDS / global
Gauss-Jordan inverse), 120 (SCP_FUSED_MAX_K) and 1024 (SCP_BIGK_MAX_K) a horizon lies on; `expected_pipeline` restates
choose_pipeline (csrc/scp_qp.hip).  Each case claims N D mod 16 (`c_tail`: columns in the last 16-column block, 0 = full),
K mod 16 (`k_tail`) and its band.
"""
from __future__ import annotations

import dataclasses
import functools

import numpy as np

import persist_cases as pc
from oracle import qp_oracle as qo
from oracle import scp_oracle as so

H, R, LIMITS, CHECK, STEPS = pc.H, pc.R, pc.LIMITS, pc.CHECK, pc.STEPS
STEPS_QP0 = (1, 5, 6, 7, 12)  # 5 and 7 split a launch just short of and just past a check
STEPS_1024 = (1, 2)
BANDS = ("<=64", "65..96", "97..120", "121..1024", ">1024")
SIGMA = 1e-6


def band(K):
    return BANDS[(K > 64) + (K > 96) + (K > 120) + (K > 1024)]


def expected_pipeline(K, C, rows, cg_iters=1, use_mfma=1):
    """choose_pipeline of csrc/scp_qp.hip (with settings.persistent = 0, or K > 64 where no persistent kernel runs)"""
    if use_mfma != 1:
        return "generic"
    cols_fit = K <= 120 and (C + 15) // 16 <= 2048
    if not rows:
        return "qp0" if cols_fit else "generic"
    if cg_iters != 1:
        return "generic"
    if cols_fit:
        return "three-launch"
    return "three-launch-bigK" if 120 < K <= 1024 and C <= 2048 else "generic"


@dataclasses.dataclass(frozen=True)
class Case:
    group: str          # "A" .. "D"
    scen: pc.Scenario
    pipeline: str       # info["pipeline"] the solve must report
    c_tail: int         # claimed N D mod 16
    k_tail: int         # claimed K mod 16
    band: str           # claimed side of 64 / 96 / 120 / 1024
    edge: str           # what the case is there for
    persistent: int = 0
    cg_iters: int = 1
    use_mfma: int = 1
    steps: tuple = STEPS
    start: str = "qp0"  # A-C: the oracle's QP#0 point; D: "zero" (reset(None)) or "random" (reset(x0), a random x0)

    @property
    def rows(self):
        return self.group != "D"

    @property
    def carries(self):
        """the pipeline carries F x and S0 x from step to step (peek "fx", "qx"): the single-step pipelines"""
        return self.pipeline in ("three-launch", "three-launch-bigK")

    @property
    def id(self):
        tag = {"A": f"p{self.persistent}", "B": "", "C": f"cg{self.cg_iters}-mfma{self.use_mfma}", "D": self.start}[self.group]
        return f"{self.group}-{self.scen.label}" + (f"-{tag}" if tag else "")

    def gpu_settings(self, max_iter):
        return pc.gpu_step_settings(self.persistent, max_iter, cg_iters=self.cg_iters, use_mfma=self.use_mfma)

    def oracle_settings(self, max_iter):
        return pc.step_settings(max_iter, cg_iters=self.cg_iters, margin=self.scen.margin)


def _s(seed, N, K, dim, margin=0.5, qp0_iters=4000):
    return pc.Scenario("near", seed, N, K, dim, margin, qp0_iters)


def _case(group, sc, edge, **kw):
    C = sc.N * sc.dim
    pipe = expected_pipeline(sc.K, C, group != "D", kw.get("cg_iters", 1), kw.get("use_mfma", 1))
    return Case(group, sc, pipe, C % 16, sc.K % 16, band(sc.K), edge, **kw)


# ---- the scenarios ------------------------------------------------------------------------------------------------------
# Seeds and margins were chosen with the oracle so that every scenario with rows has a working row whose two agents lie in
# different 16-column blocks (where N D > 16) and a row at the last agent that is active (A x < l) at every compared step;
# tests/test_pipeline_cases_cpu.py checks all of it.
K_EDGE = {65: "one time step over a lane's worth", 80: "K mod 16 = 0", 96: "the last K with the LDS inverse",
          97: "the first K with the global inverse", 120: "the largest horizon of the 16-column kernels"}
N_EDGE = {(8, 2): "16 columns: one full block", (9, 2): "18 columns: the last block holds 2",
          (17, 2): "34 columns: three blocks", (6, 3): "18 columns in 3-D", (11, 3): "33 columns: the last block holds 1"}
SCEN_A = {
    # (N, dim, K): scenario
    (9, 2, 65): _s(4661, 9, 65, 2),
    (9, 2, 80): _s(4810, 9, 80, 2),
    (9, 2, 96): _s(4969, 9, 96, 2),
    (9, 2, 97): _s(4979, 9, 97, 2),
    (9, 2, 120): _s(5209, 9, 120, 2),
    (8, 2, 65): _s(4658, 8, 65, 2),
    (8, 2, 120): _s(5209, 8, 120, 2),
    (17, 2, 65): _s(4667, 17, 65, 2),
    (17, 2, 120): _s(5217, 17, 120, 2),
    (6, 3, 65): _s(4656, 6, 65, 3),
    (6, 3, 120): _s(5206, 6, 120, 3),
    (11, 3, 65): _s(4662, 11, 65, 3),
    (11, 3, 120): _s(5211, 11, 120, 3),
}
SCEN_B = {
    (9, 2, 121): _s(5219, 9, 121, 2),
    (9, 2, 128): _s(5300, 9, 128, 2),
    (9, 2, 129): _s(5300, 9, 129, 2),
    (9, 2, 250): _s(6509, 9, 250, 2, qp0_iters=300),
    (6, 3, 121): _s(5217, 6, 121, 3),
    (6, 3, 128): _s(5287, 6, 128, 3),
    (6, 3, 129): _s(5297, 6, 129, 3),
    (6, 3, 250): _s(6510, 6, 250, 3, qp0_iters=300),
}
SCEN_1024 = _s(14244, 3, 1024, 2, qp0_iters=20)  # 2-D, N = 3: the 1024-thread limit of cg1_colK_kernel
SCEN_1025 = _s(14263, 3, 1025, 2, qp0_iters=20)  # one time step more: no column kernel is left
SCEN_C = {
    (9, 2, 17): _s(4180, 9, 17, 2),
    (9, 2, 50): _s(4509, 9, 50, 2),
    (9, 2, 65): _s(7001, 9, 65, 2),
    (9, 2, 130): _s(5311, 9, 130, 2),
    (5, 3, 17): _s(4175, 5, 17, 3),
    (5, 3, 50): _s(4515, 5, 50, 3),
    (5, 3, 65): _s(4658, 5, 65, 3),
    (5, 3, 130): _s(5309, 5, 130, 3),
}
CG_MFMA = ((2, 1), (3, 1), (3, 2), (3, 0), (1, 2), (1, 0))

CASES_A = [_case("A", sc, f"{K_EDGE[K]}; {N_EDGE[N, D]}", persistent=p) for (N, D, K), sc in SCEN_A.items() for p in (0, 1)]
CASES_B = [_case("B", sc, f"one workgroup per column, K mod 64 = {K % 64}") for (N, D, K), sc in SCEN_B.items()]
CASES_B += [_case("B", SCEN_1024, "K = 1024: one thread per time step at the workgroup limit", steps=STEPS_1024),
            _case("B", SCEN_1025, "K = 1025: beyond every column kernel", steps=STEPS_1024)]
CASES_C = [_case("C", SCEN_C[9, 2, 50], "every (cg_iters, use_mfma) pair", cg_iters=cg, use_mfma=mf) for cg, mf in CG_MFMA]
CASES_C += [_case("C", sc, "every K with two PCG steps", cg_iters=2) for (N, D, K), sc in SCEN_C.items() if (N, D, K) != (9, 2, 50)]
CASES_C += [_case("C", SCEN_C[5, 3, 50], "3-D, scalar products", cg_iters=3, use_mfma=0),
            _case("C", SCEN_C[5, 3, 65], "3-D, single PCG step off the column kernels", cg_iters=1, use_mfma=2)]
# QP#0: no rows, so any seed serves; N as in A
SCEN_D = [_s(7000 + K, 9, K, 2) for K in (3, 50, 64, 65, 120)]
SCEN_D += [_s(7000 + K + N, N, K, D) for K in (65, 120) for N, D in ((8, 2), (17, 2), (6, 3), (11, 3))]
CASES_D = [_case("D", sc, f"QP#0, {'one step' if sc.K <= 64 else 'two steps'} per lane", steps=STEPS_QP0, start=st)
           for sc in SCEN_D for st in ("zero", "random")]
CASES_D += [_case("D", _s(7121, 9, 121, 2), "QP#0 beyond the column kernels", steps=STEPS_QP0, start=st)
            for st in ("zero", "random")]
CASES = CASES_A + CASES_B + CASES_C + CASES_D


# ---- the oracle side ----------------------------------------------------------------------------------------------------
def random_x0(sc: pc.Scenario):
    """accelerations of feasible size (|a| <= 1 m/s^2, jerk within its bound) for reset(x0) of a QP#0 case"""
    return np.random.default_rng(sc.seed).uniform(-1.0, 1.0, (sc.N, sc.K, sc.dim))


@functools.lru_cache(maxsize=None)
def problem(case: Case):
    """(prob, x0, eta, l_col, dist, W) of a case; QP#0 cases: no rows (eta = l_col = dist = None, W empty)"""
    if case.rows:
        return pc.setup(case.scen)
    prob = pc.make_problem(case.scen)
    x0 = random_x0(case.scen) if case.start == "random" else None
    return prob, x0, None, None, None, np.zeros(0, dtype=np.int64)


@functools.lru_cache(maxsize=None)
def _snapshots(sc, cg_iters, steps, start):
    if start == "qp0":
        return pc.oracle_snapshots(sc, steps, cg_iters=cg_iters, margin=sc.margin)
    prob = pc.make_problem(sc)
    snaps = {}
    _, _, info = qo.admm_structured(prob, x0=random_x0(sc) if start == "random" else None,
                                    st=pc.step_settings(max(steps), margin=sc.margin), snapshots=set(steps), snap_out=snaps)
    return snaps, info


def snapshots(case: Case):
    """{m: oracle state after m steps} and the run's info (one oracle run per scenario, PCG count, steps and start)"""
    return _snapshots(case.scen, case.cg_iters, case.steps, case.start)


@functools.lru_cache(maxsize=None)
def _d_m(sc, cg_iters, start, m):
    from oracle import c_oracle as co

    st = pc.step_settings(m, cg_iters=cg_iters, margin=sc.margin)
    if start == "qp0":
        prob, x0, eta, l_col, dist, W = pc.setup(sc)
        xc, ic = co.admm(prob, eta, l_col, dist, x0=x0, st=st)  # (its working set: dist - R < st.margin, which is W)
    else:
        xc, ic = co.admm(pc.make_problem(sc), x0=random_x0(sc) if start == "random" else None, st=st)
    assert ic["iter"] == m
    return xc


def d_m(case: Case, m):
    """The largest difference in x between the numpy and the C oracle after m steps with the case's settings: the
    reference's own sensitivity to the order of summation.  100 d_m is the floor under pc.tolerances (the rule of
    tests/test_persist_iterates_gpu.py::test_rho_switch_and_adaptive_cadence)."""
    return float(np.abs(_d_m(case.scen, case.cg_iters, case.start, m) - snapshots(case)[0][m]["x"]).max())


def case_tolerances(case: Case, m, ref):
    """what the GPU comparison allows every entry of the arrays `ref` (pc.reference_arrays of the oracle state after m steps)"""
    prob = problem(case)[0]
    return pc.tolerances(prob, ref, snapshots(case)[0][m]["rho"], floor=100.0 * d_m(case, m))


def column_blocks(i, D):
    """the 16-column blocks that hold the columns of agent i"""
    return {(i * D) // 16, (i * D + D - 1) // 16}


def active_last_rows(case: Case):
    """working rows at the last agent that are active (A x < l) at every compared step of the oracle run, most active first"""
    prob, x0, eta, l_col, dist, W = problem(case)
    snaps, _ = snapshots(case)
    _, wi, wj = qo.working_rows(prob, W)
    ok = (wi == prob.N - 1) | (wj == prob.N - 1)
    slack = np.full(W.size, np.inf)
    for m in case.steps:
        s = so.collision_apply(prob, eta, snaps[m]["x"].ravel())[W] - l_col[W]
        ok &= s < 0
        slack = np.minimum(slack, -s)
    order = np.argsort(-np.where(ok, slack, -np.inf), kind="stable")
    return W[order[: int(ok.sum())]]


# ---- the KKT blocks -------------------------------------------------------------------------------------------------------
KKT_K = (3, 50, 64, 96, 97, 130, 250)   # 96 | 97: the LDS and the global form of the inverse
KKT_RHO = (0.1, 2.0 ** -6, 1.0, 2.0 ** 4)
KKT_CASES = [(K, rho) for K in KKT_K for rho in KKT_RHO]  # (numpy's own inverse passes the 1e-8 precondition at all of them)
INV_RATIO_MAX = 16.0  # Gauss-Jordan without pivoting on an SPD matrix against LAPACK's pivoted LU: the constant's allowance
EVICT_RHOS = tuple(0.1 * 2.0 ** (j / 4.0) for j in range(34))  # more distinct values than SCP_KKT_SLOTS_MAX = 32
EVICT_SCEN = {50: SCEN_C[9, 2, 50], 97: SCEN_A[9, 2, 97]}  # the LDS and the global form of the inverse, both with rows


def kkt_reference(K, rho, h=H, sigma=SIGMA, rho_eq_scale=1e3):
    """H_f of the oracle and S0"""
    ops = qo.FixedOps(K, h)
    rv = np.full(K, rho)
    rv[K - 1] = rho * rho_eq_scale
    return ops.kkt_matrix(sigma, rho, rho, rv, rv.copy()), ops.S0


def inverse_residual(Hf, Minv):
    """|| Hf Minv - I ||_max with the product in extended precision"""
    P = Hf.astype(np.longdouble) @ Minv.astype(np.longdouble)
    return float(np.abs(P - np.eye(Hf.shape[0], dtype=np.longdouble)).max())
