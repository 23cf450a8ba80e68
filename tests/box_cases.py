"""Case table of joint QPs with per-(vehicle, state) position boxes (scp_qp_set_position_boxes), on every pipeline a boxed QP
can take, and what tests need around it.

Not a conftest: tests/test_box_cases_cpu.py checks on the CPU that every case keeps the claims below, and
tests/test_box_iterates_gpu.py runs every case and compares the state after m ADMM steps with the boxed oracle
(oracle/qp_oracle.py, admm_structured(pos_boxes=..., snapshots=...)).  Scenarios, seeds, layouts, tolerances and the oracle
settings are those of tests/persist_cases.py (`pc`) and tests/pipeline_cases.py (`qc`).

  group  info["pipeline"]    what runs                                                          K
  P      persistent          cg1_persist_kernel<D>, whatever settings.persistent in 1..4 asks    <= 64
  T      three-launch        settings.persistent = 0 (control)                                   <= 64
  A      three-launch        cg1_col_kernel<2>, cg1_resid_col_kernel<2>                          65 .. 120
  B      three-launch-bigK   cg1_colK_kernel                                                     121 .. 1024
  C      generic             cg_iters = 2; use_mfma = 0 with cg_iters = 3                        any
  D      qp0 / generic       QP#0: no rows (qp0_col_kernel<1> / <2>; K = 121: generic)           <= 121

`expected_pipeline` restates choose_pipeline (csrc/scp_qp.hip) and persist_variant_for (csrc/scp_qp_persist.hip) for a QP
with boxes: `if (qp->has_boxes) return fits_old ? 0 : -1`, so no lean kernel ever runs it.

Boxes.  Every box derives from positions the ORACLE computes -- groups P, T, A, B, C: the states of x0, the oracle's QP#0
point (pc.setup); group D: the states of the oracle's box-free run after max(steps) steps -- by one of four seeded rules
(`boxes`), never from a GPU result.  An entry no rule sets is -inf / +inf.

  one-sided   one box per agent: a state j in [K / 2, K - 1], a coordinate (the last agent: the last one) and a side drawn
              per agent; the bound lies INSET = 0.25 m past the base position, so the base point violates it
  slab        the same draw with both sides set, SLAB = 0.05 m apart around the point INSET past the base position: both
              clamps of one row are finite and close
  mixed       one-sided, and on other entries (a quarter each) bounds 1 m outside the workspace -- where the workspace bound
              must win -- next to the +-inf ones
  all-states  agent 0: every state j >= 1 and coordinate boxed +-ALL_HALF = 0.3 m around the base position shifted by
              ALL_SHIFT = 0.1 m (sign per coordinate), the way a corridor boxes a whole column; the other agents one-sided.
              Used where the QP moves agent 0 that far (the circle scenarios, QP#0 from a random start): there at least 8 rows
              of its columns sit on their bounds at once (checked); on the short moves of the "near" lattices none would

The draw of a case is seeded by (scenario seed, pattern, salt); salt is 0 but for the two cases of SALT.  The file also holds
the boxed SCP scenarios of tests/test_box_scp_gpu.py and tests/test_box_solves_gpu.py (SCP_SHAPES, waypoint_boxes).

Claims (tests/test_box_cases_cpu.py): solvers.scp.check_position_boxes accepts every case; at every compared m >= 2 the boxed
rows whose z lies exactly on its bound with a non-zero dual include one at the last agent, one in every workgroup of the
round-2 kernel and one in every 16-column block; the boxed and the box-free oracle x differ by >= 1e4 x the comparison
tolerance at every m >= 2 (at m = 1 they are identical: z starts as A x unclamped with y = 0, so a box first acts on x in
step 2); the boxed oracle run takes < 10 s.

Tolerance: pc.tolerances with the floor 100 d_box(m).  d_box(m) is the largest difference in x after m steps between two runs
of the boxed numpy oracle: one from x0, one from x0 * (1 + 2^-52 s), s = +-1 per entry drawn from default_rng(1) (where x0 = 0,
group D "zero": the problem's p0 perturbed the same way) -- the oracle's own sensitivity to rounding, a stand-in for
pipeline_cases.d_m, whose C oracle takes no boxes.
"""
from __future__ import annotations

import dataclasses
import functools

import numpy as np

import persist_cases as pc
import pipeline_cases as qc
from oracle import qp_oracle as qo
from oracle import scp_oracle as so

STEPS, STEPS_QP0 = pc.STEPS, qc.STEPS_QP0
PATTERNS = ("one-sided", "slab", "mixed", "all-states")
INSET, SLAB, ALL_HALF, ALL_SHIFT, WIDER = 0.25, 0.05, 0.3, 0.1, 1.0
STATE = ("x", "zf", "yf", "zc", "yc")
CARRIED = ("fx", "qx")
PERSISTENT_SETTINGS = (1, 2, 3, 4)
DIFFER_MIN = 1e4  # boxed vs box-free oracle, in comparison tolerances


def expected_pipeline(K, C, rows, persistent=1, cg_iters=1, use_mfma=1):
    """choose_pipeline + scp_qp_persist_eligible + persist_variant_for for a QP WITH boxes (up to the round-2 kernel's
    workgroup limit, far beyond the table)"""
    if rows and K <= 64 and persistent and cg_iters == 1 and use_mfma == 1:
        return "persistent"
    return qc.expected_pipeline(K, C, rows, cg_iters, use_mfma)


@dataclasses.dataclass(frozen=True)
class Case:
    group: str          # "P", "T", "A" .. "D"
    scen: pc.Scenario
    pattern: str        # one of PATTERNS
    pipeline: str       # info["pipeline"] the solve must report
    persistent: int = 1
    cg_iters: int = 1
    use_mfma: int = 1
    steps: tuple = STEPS
    start: str = "qp0"  # rows: the oracle's QP#0 point; D: "zero" (reset(None)) or "random" (reset(x0), a random x0)
    salt: int = 0       # another draw of the same rule (chosen with the oracle where draw 0 leaves the last agent's box idle)

    @property
    def rows(self):
        return self.group != "D"

    @property
    def carries(self):
        """F x and S0 x are part of the state between steps (peek "fx", "qx")"""
        return self.pipeline in ("persistent", "three-launch", "three-launch-bigK")

    @property
    def names(self):
        return STATE + (CARRIED if self.carries else ())

    @property
    def persistents(self):
        """the values of settings.persistent the GPU test runs the case with"""
        return PERSISTENT_SETTINGS if self.group == "P" else (self.persistent,)

    @property
    def apb(self):
        """agents per workgroup of the round-2 kernel"""
        return pc.apb(4, self.scen.dim)

    @property
    def id(self):
        tag = {"P": "", "T": "p0", "A": "", "B": "", "C": f"cg{self.cg_iters}-mfma{self.use_mfma}", "D": self.start}[self.group]
        return f"{self.group}-{self.scen.label}-{self.pattern}" + (f"-{tag}" if tag else "")

    def gpu_settings(self, max_iter, persistent=None):
        return pc.gpu_step_settings(self.persistent if persistent is None else persistent, max_iter, cg_iters=self.cg_iters,
                                    use_mfma=self.use_mfma)

    def oracle_settings(self, max_iter):
        return pc.step_settings(max_iter, cg_iters=self.cg_iters, margin=self.scen.margin)


# draw 0 leaves the last agent's box off its bound at some compared step of these (group, scenario, pattern); chosen with the oracle
SALT = {("P", "circle2d-N9-K50-s9", "mixed"): 2, ("C", "near2d-N9-K65-s7001", "mixed"): 2}


def _case(group, sc, pattern, **kw):
    pipe = expected_pipeline(sc.K, sc.N * sc.dim, group != "D", kw.get("persistent", 1), kw.get("cg_iters", 1),
                             kw.get("use_mfma", 1))
    return Case(group, sc, pattern, pipe, salt=SALT.get((group, sc.label, pattern), 0), **kw)


def _find(table, N, K):
    (sc,) = [s for s, _, _ in table if (s.N, s.K) == (N, K)]
    return sc


# ---- the table ----------------------------------------------------------------------------------------------------------
# P: 2-D at K = 50 (N mod 8 = 7, 0, 1, 1 and five workgroups), 2-D N = 9 over the K tile edges, 3-D with 4 agents per workgroup
SCEN_P = ([_find(pc.TABLE_2D, N, 50) for N in (7, 8, 9, 17, 33)] + [_find(pc.TABLE_2D, 9, K) for K in (3, 16, 17, 64)]
          + [_find(pc.TABLE_3D, N, 50) for N in (4, 5, 9)] + [_find(pc.TABLE_3D, 5, K) for K in (16, 17, 64)])
# (all-states with its +-0.3 m only where the joint QP moves the agent that far from x0 -- the circle scenarios -- and on QP#0
# from a random start: on the short moves of the "near" lattices no row of such a box is ever active)
_O, _S, _M, _A = PATTERNS
PATTERN_P = (_O, _S, _M, _A, _O) + (_S, _M, _O, _S) + (_M, _O, _S) + (_O, _S, _M)
CASES_P = [_case("P", sc, pat) for sc, pat in zip(SCEN_P, PATTERN_P)]
CASES_T = [_case("T", pc.RHO_2D, _A, persistent=0), _case("T", _find(pc.TABLE_3D, 5, 17), _S, persistent=0)]
CASES_A = [_case("A", qc.SCEN_A[key], pat) for key, pat in (((8, 2, 65), _O), ((9, 2, 65), _S), ((6, 3, 65), _M),
                                                             ((8, 2, 120), _M), ((9, 2, 120), _O), ((6, 3, 120), _S))]
CASES_B = [_case("B", qc.SCEN_B[key], pat) for key, pat in (((9, 2, 121), _M), ((6, 3, 121), _S), ((9, 2, 250), _O))]
CASES_C = [_case("C", qc.SCEN_C[key], pat, cg_iters=cg, use_mfma=mf)
           for key, pat, cg, mf in (((9, 2, 50), _S, 2, 1), ((9, 2, 50), _O, 3, 0), ((9, 2, 65), _M, 2, 1),
                                    ((9, 2, 65), _O, 3, 0), ((5, 3, 50), _M, 2, 1))]
# QP#0 (any seed serves: no rows); K = 121 lies beyond the column kernels
SCEN_D = [qc._s(7000 + K, 9, K, 2) for K in (50, 65, 120)] + [qc._s(7000 + 65 + 6, 6, 65, 3), qc._s(7121, 9, 121, 2)]
CASES_D = [_case("D", sc, PATTERNS[(2 * i + j) % 4], steps=STEPS_QP0, start=st)
           for i, sc in enumerate(SCEN_D) for j, st in enumerate(("zero", "random"))]
CASES = CASES_P + CASES_T + CASES_A + CASES_B + CASES_C + CASES_D
GROUPS = ("P", "T", "A", "B", "C", "D")


# ---- the boxes -----------------------------------------------------------------------------------------------------------
def _one_per_agent(rng, N, K, D):
    """(state j in [max(1, K / 2), K - 1], coordinate, sign) of every agent; the last agent's coordinate is the last one, so
    that the QP's last column -- alone or nearly so in its 16-column block at N D mod 16 = 1, 2 -- carries a box"""
    j = rng.integers(max(1, K // 2), K, N)
    d = rng.integers(0, D, N)
    d[N - 1] = D - 1
    sgn = np.where(rng.integers(0, 2, N) == 1, 1.0, -1.0)
    return j, d, sgn


def boxes(pattern, seed, pos, pos_min, pos_max, salt=0, inset=INSET):
    """(lo, hi), (N, K, D) by state, of one pattern around the base positions `pos` (N, K, D), seeded by (`seed`, pattern,
    `salt`)"""
    N, K, D = pos.shape
    rng = np.random.default_rng([seed, PATTERNS.index(pattern), salt])
    lo, hi = np.full((N, K, D), -np.inf), np.full((N, K, D), np.inf)
    j, d, sgn = _one_per_agent(rng, N, K, D)
    if pattern == "mixed":
        u = rng.random((2, N, K, D))
        lo = np.where(u[0] < 0.25, np.broadcast_to(pos_min - WIDER, (N, K, D)), lo)
        hi = np.where(u[1] < 0.25, np.broadcast_to(pos_max + WIDER, (N, K, D)), hi)
    for i in range(N):
        cut = pos[i, j[i], d[i]] + sgn[i] * inset  # sign +: a lower bound above the base position; -: an upper bound below
        if pattern == "slab":
            lo[i, j[i], d[i]], hi[i, j[i], d[i]] = cut - SLAB / 2, cut + SLAB / 2
        elif sgn[i] > 0:
            lo[i, j[i], d[i]] = cut
        else:
            hi[i, j[i], d[i]] = cut
    if pattern == "all-states":
        shift = np.where(rng.integers(0, 2, D) == 1, ALL_SHIFT, -ALL_SHIFT)
        lo[0], hi[0] = -np.inf, np.inf
        lo[0, 1:] = pos[0, 1:] + shift - ALL_HALF
        hi[0, 1:] = pos[0, 1:] + shift + ALL_HALF
    return lo, hi


def waypoint_boxes(free_pos, half, disp, reach, widen=0.3):
    """Waypoint boxes of the SCP-level tests, around the box-free plan `free_pos` (N, K, D): every third vehicle and the last
    one must pass, at state K / 2, within +-half of its box-free position displaced by `disp` along coordinate i mod D (even
    vehicles +, odd -); the box widens by `widen` per step over `reach` neighbouring states on either side."""
    N, K, D = free_pos.shape
    lo, hi = np.full((N, K, D), -np.inf), np.full((N, K, D), np.inf)
    j0 = K // 2
    for i in sorted(set(range(0, N, 3)) | {N - 1}):
        c = free_pos[i, j0].copy()
        c[i % D] += disp if i % 2 == 0 else -disp
        for s in range(-reach, reach + 1):
            w = half + widen * abs(s)
            lo[i, j0 + s], hi[i, j0 + s] = c - w, c + w
    return lo, hi


# The boxed SCP scenarios -- name: (n, dim, T, h, half-width, displacement, reach, seed).  Chosen with the oracle: every QP of
# the boxed oracle loop ends "solved", the loop takes at least one iteration and under 10 s.
SCP_R = 0.8
SCP_SHAPES = {
    "n4": (4, 2, 10.0, 0.5, 0.25, 1.0, 2, 1),       # N = 4, K = 20: one workgroup
    "n10": (10, 2, 10.0, 0.25, 0.2, 0.4, 3, 7),     # N = 10, K = 40: two workgroups of the round-2 kernel
    "grid3d": (8, 3, 10.0, 0.5, 0.2, 0.4, 2, 6),    # 3-D grid swap, N = 8, K = 20: two workgroups of 4 agents
    "n6": (6, 2, 10.0, 0.5, 0.25, 1.0, 2, 11),      # (the second shape of the eps = 1e-8 comparison)
}


@functools.lru_cache(maxsize=None)
def scp_scenario(name):
    """(p0, pf, space, prob, lo, hi, box-free oracle positions) of a shape; the boxes are waypoint_boxes around the box-free
    oracle plan (two PCG steps, default tolerances)"""
    from path_planning.scenarios.position_generator import generate_grid_swap, generate_positions

    n, dim, T, h, half, disp, reach, seed = SCP_SHAPES[name]
    if dim == 3:
        p0, pf, space = generate_grid_swap(n, seed=seed, dim=3)
    else:
        p0, pf = generate_positions(n, SCP_R, seed=seed)
        space = [0, 0, 20, 20]
    prob = so.make_problem(n, T, h, SCP_R, space, p0, pf)
    free = qo.scp_solve(prob, 15, qo.Settings(max_iter=10000, cg_iters=2))
    lo, hi = waypoint_boxes(free["positions"], half, disp, reach)
    return p0, pf, space, prob, lo, hi, free["positions"]


@functools.lru_cache(maxsize=None)
def scp_joint_qp(name, cg_iters, it):
    """The joint QP of SCP iteration `it` (1-based) of a boxed shape, as the oracle's loop builds it: (prob, x0, eta, l_col,
    dist, W) with x0 the iterate after it - 1 iterations, the linearisation there and the rows within the default margin"""
    prob, lo, hi = scp_scenario(name)[3:6]
    st = qo.Settings(max_iter=10000, cg_iters=cg_iters)
    out = qo.scp_solve(prob, it - 1, st, pos_boxes=(lo, hi))
    assert out["iterations"] == it - 1 and not out["converged"]
    x0 = out["accelerations"]
    pos, _ = so.kinematics(prob, x0)
    eta, l_col, dist = so.linearize_pairs(prob, pos)
    return prob, x0, eta, l_col, dist, np.nonzero(dist - prob.R < st.margin)[0].astype(np.int64)


def drop_agent(lo, hi, i):
    """the boxes without those of agent i (the sensitivity control)"""
    lo, hi = lo.copy(), hi.copy()
    lo[i], hi[i] = -np.inf, np.inf
    return lo, hi


# ---- the oracle side -----------------------------------------------------------------------------------------------------
def _ulp_noise(a):
    """a * (1 + 2^-52 s), s = +-1 per entry from default_rng(1)"""
    a = np.asarray(a, dtype=np.float64)
    s = np.where(np.random.default_rng(1).integers(0, 2, a.shape) == 1, 1.0, -1.0)
    return a * (1.0 + 2.0 ** -52 * s)


def _run(prob, x0, eta, l_col, dist, W, st, steps, pos_boxes):
    snaps = {}
    kw = {} if pos_boxes is None else {"pos_boxes": pos_boxes}
    if eta is None:
        _, _, info = qo.admm_structured(prob, x0=x0, st=st, snapshots=set(steps), snap_out=snaps, **kw)
    else:
        _, _, info = qo.admm_structured(prob, eta, l_col, dist, x0=x0, st=st, rows0=W, snapshots=set(steps), snap_out=snaps, **kw)
    return snaps, info


@functools.lru_cache(maxsize=None)
def _problem(sc, start):
    if start == "qp0":
        return pc.setup(sc)
    prob = pc.make_problem(sc)
    return prob, (qc.random_x0(sc) if start == "random" else None), None, None, None, np.zeros(0, dtype=np.int64)


def problem(case: Case):
    """(prob, x0, eta, l_col, dist, W) of a case; group D: no rows (eta = l_col = dist = None, W empty)"""
    return _problem(case.scen, case.start)


@functools.lru_cache(maxsize=None)
def _free(sc, cg_iters, steps, start):
    prob, x0, eta, l_col, dist, W = _problem(sc, start)
    return _run(prob, x0, eta, l_col, dist, W, pc.step_settings(max(steps), cg_iters=cg_iters, margin=sc.margin), steps, None)


def free_snapshots(case: Case):
    """the box-free oracle run of the case's QP: ({m: state}, info)"""
    return _free(case.scen, case.cg_iters, case.steps, case.start)


@functools.lru_cache(maxsize=None)
def _boxes(sc, pattern, cg_iters, steps, start, salt):
    prob, x0 = _problem(sc, start)[:2]
    base = x0 if start == "qp0" else _free(sc, cg_iters, steps, start)[0][max(steps)]["x"]
    pos, _ = so.kinematics(prob, base)
    lo, hi = boxes(pattern, sc.seed, pos, prob.pos_min, prob.pos_max, salt)
    lo.setflags(write=False)
    hi.setflags(write=False)
    return lo, hi


def _key(case):
    return case.scen, case.pattern, case.cg_iters, case.steps, case.start, case.salt


def case_boxes(case: Case):
    """(lo, hi) of a case, read-only"""
    return _boxes(*_key(case))


@functools.lru_cache(maxsize=None)
def _boxed(sc, pattern, cg_iters, steps, start, salt, noisy):
    prob, x0, eta, l_col, dist, W = _problem(sc, start)
    pb = _boxes(sc, pattern, cg_iters, steps, start, salt)
    if noisy and x0 is not None:
        x0 = _ulp_noise(x0)
    elif noisy:
        prob = dataclasses.replace(prob, p0=_ulp_noise(prob.p0))
    return _run(prob, x0, eta, l_col, dist, W, pc.step_settings(max(steps), cg_iters=cg_iters, margin=sc.margin), steps, pb)


def snapshots(case: Case):
    """{m: boxed oracle state after m steps} and the run's info"""
    return _boxed(*_key(case), False)


def d_box(case: Case, m):
    """largest difference in x after m steps between the boxed oracle run and its rerun from the start perturbed by one ulp"""
    key = _key(case)
    return float(np.abs(_boxed(*key, True)[0][m]["x"] - _boxed(*key, False)[0][m]["x"]).max())


def perturbation_distance(prob, x0, eta, l_col, dist, W, st, steps, pos_boxes=None):
    """the d_box rule on any QP with a non-zero start, boxed or not: {m: |x_m(x0) - x_m(x0 (1 + 2^-52 s))|_max} over one pair
    of runs with the settings `st` (st.max_iter >= max(steps))"""
    a = _run(prob, x0, eta, l_col, dist, W, st, steps, pos_boxes)[0]
    b = _run(prob, _ulp_noise(x0), eta, l_col, dist, W, st, steps, pos_boxes)[0]
    return {m: float(np.abs(a[m]["x"] - b[m]["x"]).max()) for m in steps}


def oracle_bounds(case: Case):
    """(lf, uf) in the layout of peek "lf" / "uf": [4K-1][C] time-major, flat"""
    b = so.fixed_bounds(problem(case)[0], case_boxes(case))
    return tuple(pc.fixed_time_major([b[k][s] for k in ("jerk", "acc", "vel", "pos")]).ravel() for s in (0, 1))


# ---- the comparison --------------------------------------------------------------------------------------------------------
def worst_ratio(prob, snap, got, gpu_rows, names, floor):
    """largest |got - oracle| / tolerance over the arrays `names` (got: name -> flat array in the layout of scp_qp_peek):
    the comparison of compare_state (tests/test_pipeline_iterates_gpu.py) with the assert turned into a return value"""
    order = np.searchsorted(snap["rows"], gpu_rows)
    assert np.array_equal(snap["rows"][order], gpu_rows)
    ref = pc.reference_arrays(prob, snap, order)
    tols = pc.tolerances(prob, ref, snap["rho"], floor=floor)
    return max(float(np.max(np.abs(np.asarray(got[n]) - ref[n]) / tols[n], initial=0.0)) for n in names)


def active_boxed(case: Case, m, tol_dual=0.0):
    """(agent, state, coordinate) of the boxed position rows whose z lies exactly on a bound the box set, with a non-zero dual,
    in the oracle's snapshot after m steps: (n, 3) int array"""
    prob = problem(case)[0]
    snap = snapshots(case)[0][m]
    free = so.fixed_bounds(prob)["pos"]
    lp, up = so.fixed_bounds(prob, case_boxes(case))["pos"]
    z, y = snap["zf"][3], snap["yf"][3]
    on = (((z == lp) & (lp != free[0])) | ((z == up) & (up != free[1]))) & (np.abs(y) > tol_dual)
    idx = np.argwhere(on)
    idx[:, 1] += 1  # row k holds state k + 1
    return idx
