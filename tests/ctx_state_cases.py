"""One small case per context-taking entry point of include/scp_hip.h, for the tests of what a context carries from one call
to the next (tests/test_ctx_state_cpu.py keeps this table true without a GPU, tests/test_ctx_state_gpu.py runs it).

A case has
  inputs()            host arrays, made once and never changed
  run(ctx, inp)       the calls on a given Context -> the outputs as host arrays in their CANONICAL form: what the header
                      documents as defined (a list up to its returned count, in the order the header promises; the rows of a
                      plane, not the padding of its stride), under fixed names
  reference(inp)      the CPU reference of the same operation (the module its own GPU test file uses)
  from_ref(ref, inp)  the canonical form the reference alone gives (keys the reference does not define are left out)
  compare(out, ref, inp)  the criterion the family's own test file holds the GPU result to
  ws(inp)             {buffer: (low, high)} bounds in bytes of what the case needs of each grown-on-demand buffer of the
                      context: the sizes of DESIGN.md ("What a context owns"), restated below.  Where a size depends on the
                      compute-unit count (the chunks of the continuous-time passes) the bounds differ.
`entries` names the C entry points the case calls.  Every family has a GROWER: larger calls of the same entry points, run first
on a context so that each shared buffer is larger than the case under test needs and no reallocation hides stale contents.

Nothing here touches the GPU or imports torch at import time."""
import contextlib
import functools
import os

import numpy as np

import assign_paths_ref as apr
import assignment_ref as asr
import box_cases as bxc
import clearance_ref as clr
import conflicts_ref as cfr
import corridor_ref as cor
import delay_ref as dlr
import holds_ref as hdr
import obstacle_distance_cases as odc
import rasterize_cases as rzc
import reference_path_cases as rpc
import scenario_device_ref as sdr
import separation_ref as sr
import shard_cases as shc
import shorten_cases as stc
import stagger_ref as sgr
import stagger_search_ref as ssr
import weighted_path_cases as wpc
import weighted_path_ref as wpr
from oracle import qp_oracle as qo
from oracle import scp_oracle as so

EPS = np.finfo(np.float64).eps
NO_ROW = 2**64 - 1
H = 0.2
LIMITS = [-2.0, 2.0, -15.0, 15.0, -20.0, 20.0]
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CANARY = 0xA5


# ---- the harness ------------------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def canary_outputs():
    """Every tensor the binding allocates with torch.empty while this is active is filled with 0xA5 bytes first, on the current
    stream: the output arrays and records, the row lists, the planes of a PairPass, the QP's workspace.  NOT covered: what the
    binding allocates with torch.zeros because the library reads or accumulates into it -- the stats blocks, the counts
    (n_found, n_failed, n_holds, n_blocked, n_open, n_new), a working-set bitmap, a hold table."""
    import torch

    real = torch.empty

    def empty(*args, **kw):
        t = real(*args, **kw)
        if t.is_cuda and t.numel() and t.is_contiguous() and t.dim() >= 1:
            t.view(torch.uint8).fill_(CANARY)
        return t

    torch.empty = empty
    try:
        yield
    finally:
        torch.empty = real


def _leaves(x, where=""):
    if isinstance(x, dict):
        for k in sorted(x):
            yield from _leaves(x[k], f"{where}.{k}" if where else str(k))
    elif isinstance(x, (list, tuple)):
        for i, v in enumerate(x):
            yield from _leaves(v, f"{where}[{i}]")
    else:
        yield where, x


def assert_no_canary(out):
    """no word of a canonical output still holds the bytes the harness put there before the call"""
    for where, v in _leaves(out):
        if not isinstance(v, np.ndarray) or v.size == 0:
            continue
        raw = np.ascontiguousarray(v).view(np.uint8).reshape(-1)
        if v.dtype.itemsize % 4 == 0:
            hit = raw.view(np.uint32) == 0xA5A5A5A5
        elif v.dtype.itemsize == 2:
            hit = raw.view(np.uint16) == 0xA5A5
        else:
            hit = raw == CANARY
        assert not hit.any(), f"{where}: {int(hit.sum())} words still hold the canary the harness wrote before the call"


def assert_same_bits(got, want, label=""):
    """two canonical forms, bit for bit"""
    a, b = dict(_leaves(got)), dict(_leaves(want))
    assert sorted(a) == sorted(b), (label, sorted(set(a) ^ set(b)))
    for k in sorted(a):
        x, y = a[k], b[k]
        if isinstance(x, np.ndarray) or isinstance(y, np.ndarray):
            x, y = np.asarray(x), np.asarray(y)
            assert x.dtype == y.dtype and x.shape == y.shape, (label, k, x.dtype, y.dtype, x.shape, y.shape)
            if x.tobytes() != y.tobytes():
                bad = np.nonzero(np.ascontiguousarray(x).view(np.uint8).reshape(-1) != np.ascontiguousarray(y).view(np.uint8).reshape(-1))[0]
                raise AssertionError(f"{label}: {k} differs in {bad.size} bytes, first at byte {int(bad[0])} of {x.nbytes}")
        elif isinstance(x, float) or isinstance(y, float):
            assert np.float64(x).tobytes() == np.float64(y).tobytes(), (label, k, x, y)
        else:
            assert x == y, (label, k, x, y)


NEVER_POISON_BEFORE = ("scp_ctx_debug_fill", "scp_ctx_debug_state", "scp_ctx_destroy", "scp_last_error")


class RecordingLibrary:
    """libscp_hip.so as a Context sees it, with every entry point that is called written down; with `poison` set, every
    scratch workspace of the context is overwritten (scp_ctx_debug_fill) before EACH call, so that a later call of a case
    cannot live on what an earlier call of the same case left"""

    def __init__(self, lib, handle):
        self._lib, self._handle, self.called, self.poison = lib, handle, set(), None

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not name.startswith("scp_"):
            return fn

        def call(*args):
            self.called.add(name)
            if self.poison is not None and name not in NEVER_POISON_BEFORE:
                assert self._lib.scp_ctx_debug_fill(self._handle, self.poison) == 0
            return fn(*args)

        return call


# families whose cases are chains of stateless entry points: nothing but the invariants may carry over from one call to the
# next, so the workspaces are poisoned between the calls too.  A QP and a solver are objects with a state of their own that
# spans their calls; their cases are poisoned before the first call only.
POISON_BETWEEN_CALLS = ("pairwise", "trajectory", "continuous", "obstacle", "assign")


class Case:
    def __init__(self, name, family, entries, inputs, run, reference=None, from_ref=None, compare=None, ws=None):
        self.name, self.family, self.entries = name, family, tuple(entries)
        self._inputs, self._run, self.reference, self.from_ref, self.compare = inputs, run, reference, from_ref, compare
        self._ws = ws or (lambda inp: {})
        self._made = None
        self._ref = None

    def inputs(self):
        if self._made is None:
            self._made = self._inputs()
        return self._made

    def ref(self):
        """the reference of the case's inputs, computed once and left unchanged"""
        if self._ref is None:
            self._ref = self.reference(self.inputs())
        return self._ref

    def run(self, ctx, poison=None):
        """the case on `ctx` with every output pre-filled by the harness -> its canonical outputs.  The entry points that were
        called are left in self.called; poison: the word every scratch workspace is filled with before every call (families of
        POISON_BETWEEN_CALLS) or before the first one"""
        real = ctx.lib
        rec = RecordingLibrary(real, ctx.h)
        if poison is not None:
            if self.family in POISON_BETWEEN_CALLS:
                rec.poison = poison
            else:
                ctx.debug_fill(poison)
        ctx.lib = rec
        try:
            with canary_outputs():
                out = self._run(ctx, self.inputs())
        finally:
            ctx.lib = real
        self.called = rec.called
        assert_no_canary(out)
        return out

    def ws(self):
        return self._ws(self.inputs())

    def __repr__(self):
        return f"Case({self.name})"


def _grid(D, origin, cell, occ):
    from path_planning import _hip

    return _hip.occupancy_grid(D, origin, cell, occ.shape[::-1])


def _np(t):
    return t.cpu().numpy().copy()


def _align64(b):
    return (int(b) + 63) & ~63


# ---- buffer sizes, restated from the host code ("What a context owns") -------------------------------------------------
SEP_TILE = 64
SEP_PARTIAL, CLR_ENTRY, DLY_ENTRY, HOLD_CAND, CONFLICT_BYTES, HOLD_BYTES = 64, 32, 32, 32, 48, 48
SORT_CHUNK = 1024
CMP_WORDS = 1024


def sep_records(N, K, D):
    return _align64(N * K * (3 * D + 1) * 8)


def dly_records(N, K, D):
    return _align64(N * (K + 2) * (3 * D + 1) * 8)


def sep_tiles(N):
    nt = -(-N // SEP_TILE)
    return nt * (nt + 1) // 2  # the whole pair range: every tile of the upper triangle


def ws_check_separation(N, K, D):
    return {"sep_ws": (sep_records(N, K, D) + sep_tiles(N) * SEP_PARTIAL, sep_records(N, K, D) + sep_tiles(N) * K * SEP_PARTIAL)}


def ws_list_conflicts(N, K, D, capacity):
    span = SORT_CHUNK
    while span < capacity:
        span *= 2
    b = sep_records(N, K, D) + _align64(capacity * CONFLICT_BYTES) + span * 12
    return {"sep_ws": (b, b)}


def ws_clearance(N, K, D):
    fixed = sep_records(N, K, D) + _align64(2 * (N + K) * 8) + K * sep_tiles(N) * CLR_ENTRY
    return {"sep_ws": (fixed + sep_tiles(N) * 2 * SEP_TILE * CLR_ENTRY, fixed + K * sep_tiles(N) * 2 * SEP_TILE * CLR_ENTRY)}


def ws_delay(N, K, D, S):
    ntb = -(-N // SEP_TILE)
    ent = N * (S + 1) * DLY_ENTRY
    return {"sep_ws": (dly_records(N, K, D) + ntb * ent, dly_records(N, K, D) + -(-(K + S) // min(4, K + S)) * ntb * ent)}


def ws_lag(N, K, D):
    return {"sep_ws": (dly_records(N, K, D),) * 2}


def ws_batch(N, B):
    return {"sep_ws": ((N * N * 8,) * 2 if B >= 16 else (0, 0))}


def ws_update_holds(n_c, n_t):
    b = _align64(n_c * HOLD_CAND) + 4 * _align64(n_c * 4) + 64 + _align64((n_t + 2 * n_c) * HOLD_BYTES)
    return {"sep_ws": (b, b)}


def ws_apply_holds(n_t):
    return {"sep_ws": (2 * _align64(n_t * 4) + 64,) * 2}


def ws_paths(N, max_path):
    return {"sep_ws": (N * max_path * 4,) * 2}


def ws_distance(occ):
    nz, ny, nx = occ.shape
    return {"sep_ws": ((occ.size * 4,) * 2 if (ny > 1) + (nz > 1) else (0, 0))}


def ws_pairwise(N, K, D, single_launch=True, linearize_only=False):
    """scp_linearize_pairs always runs as prep + pass + compaction (tm_scratch); the select, check and violations passes of a small
    problem run as one launch, whose workgroups keep their sub-lists in wg_rows"""
    pairs = N * (N - 1) // 2
    words = (K * pairs + 31) // 32
    small = single_launch and not linearize_only and all(shc.pass_forms(N, K, D, pairs))
    out = {"cmp_map_bytes": (words * 4,) * 2, "cmp_tot_bytes": ((-(-words // CMP_WORDS) + 1) * 4,) * 2}
    out["tm_bytes"] = (2 * ((N * K * D + 1) & ~1) * 8,) * 2
    out["wg_rows_bytes"] = (-(-(pairs + 1) // shc.SMALL_ROWS) * K * shc.SMALL_ROWS * 4,) * 2 if small else (0, 0)
    return out


LINE_TILE, LINE_PARTIAL, ASGW_HEADER, ASGW_CTL, ASGW_ENTRY, GEN_ALIGN = 256, 32, 64, 192, 48, 256


def ws_line_check(B, N):
    nt = -(-N // LINE_TILE)
    return {"asg_ws_bytes": (LINE_PARTIAL * B * nt * (nt + 1) // 2,) * 2}


def ws_assign_wide(B, N):
    return {"asgw_ws_bytes": (ASGW_HEADER + ASGW_CTL * B + ASGW_ENTRY * N * B,) * 2}


def ws_generator(B, N):
    """seeds, block table (4 ints per block), members, owners, flags and unmet (one int per scenario and block), swept, min,
    cnt, each aligned to 256 bytes; the blocks are between 1 and N"""
    def total(nblk):
        off = 0
        for b in (8 * B, 16 * nblk, 4 * N, 4 * N, 4 * B * nblk, 4 * B * nblk, 4 * B, 8 * B, 8 * B):
            off = (off + b + GEN_ALIGN - 1) & ~(GEN_ALIGN - 1)
        return off
    return {"gen_ws_bytes": (total(1), total(N))}


def merge_ws(*parts):
    """the needs of several calls on one context: every buffer grows to the largest"""
    out = {}
    for p in parts:
        for k, (lo, hi) in p.items():
            out[k] = (max(lo, out.get(k, (0, 0))[0]), max(hi, out.get(k, (0, 0))[1]))
    return out


# ---- family "pairwise": the O(N^2 K) passes ----------------------------------------------------------------------------------------
def synth(N, K, D, seed, h=0.2, R=0.8):
    """tests/test_kernels_gpu.py's synthetic problem: (oracle problem, accelerations)"""
    rng = np.random.default_rng(seed)
    side = max(4.0, 1.6 * N ** (1.0 / D))
    p0, pf = rng.uniform(0, side, (N, D)), rng.uniform(0, side, (N, D))
    v0, vf = rng.uniform(-0.3, 0.3, (N, D)), rng.uniform(-0.3, 0.3, (N, D))
    prob = so.make_problem(N, K * h + 1e-9, h, R, [-2.0] * D + [side + 2.0] * D, p0, pf, v0, vf)
    assert prob.K == K
    return prob, 0.3 * rng.standard_normal((N, K, D))


MARGIN, FEAS = 0.2, 1e-6


def _pair_inputs(N, K, D, seed, step=0.2):
    prob, acc = synth(N, K, D, seed)
    pos, _ = so.kinematics(prob, acc)
    x = acc + step * np.random.default_rng(seed + 1).standard_normal(acc.shape)
    pos_new, _ = so.kinematics(prob, x)
    return dict(prob=prob, pos=pos, x=x, pos_new=pos_new)


def _bits_of(rows, n_rows):
    b = np.zeros(max((n_rows + 31) // 32, 1) * 32, dtype=np.uint8)
    b[np.asarray(rows, dtype=np.int64)] = 1
    return np.packbits(b, bitorder="little").view(np.uint32).copy()


def _pair_run(ctx, inp, single_launch=True, with_reference=True):
    from path_planning import _hip

    prob = inp["prob"]
    N, K, D = prob.N, prob.K, prob.D
    pos, new, p0, v0 = (ctx.tensor(a) for a in (inp["pos"], inp["pos_new"], prob.p0, prob.v0))
    if not single_launch:
        ctx.lib.scp_ctx_set_option(ctx.h, b"single_launch_passes", 0)  # (the call itself: the binding's flag stays clear)
    try:
        pp = _hip.PairPass(ctx, N, K, D, prob.R, prob.h)
        rows, md, fv = pp.linearize(pos, p0, v0, MARGIN)
        out = {"rows": _np(rows), "min_dist": md, "first": int(fv), "bitmap0": _np(pp.bitmap).view(np.uint32)}
        if with_reference:
            out["eta"], out["l"] = _np(pp.eta_rows()), _np(pp.l_rows())
        w_eta, w_l = pp.gather(rows)
        out["w_eta"], out["w_l"] = _np(w_eta), _np(w_l)
        chk = ctx.check_avoidance(N, K, D, prob.R, pos)
        out["chk_min"], out["chk_first"] = chk[0], int(chk[1])
        new_rows, max_v = pp.violations(new, p0, v0, FEAS, recompute=False)  # scp_collision_violations: the stored rows
        out["new_rows"], out["max_v"], out["bitmap"] = _np(new_rows), max_v, _np(pp.bitmap).view(np.uint32)
        pp2 = _hip.PairPass(ctx, N, K, D, prob.R, prob.h)
        rows2, md2, fv2 = pp2.select(pos, MARGIN)
        out["rows2"], out["min_dist2"], out["first2"] = _np(rows2), md2, int(fv2)
        new2, max_v2 = pp2.violations(new, p0, v0, FEAS)  # scp_collision_violations_at: recomputed
        out["new_rows2"], out["max_v2"], out["bitmap2"] = _np(new2), max_v2, _np(pp2.bitmap).view(np.uint32)
        out["scratch"] = ctx.peek_scratch_map((K * prob.pairs + 31) // 32)
    finally:
        if not single_launch:
            ctx.lib.scp_ctx_set_option(ctx.h, b"single_launch_passes", 1)
    return out


def _pair_reference(inp):
    prob = inp["prob"]
    eta, l, dist = so.linearize_pairs(prob, inp["pos"])
    sel = np.nonzero(dist - prob.R < MARGIN)[0]
    ok, fv = so.check_avoidance(prob, inp["pos"])
    first = NO_ROW
    if not ok:
        iu, ju = so.pair_index(prob.N)
        first = int(fv[0] * prob.pairs + np.nonzero((iu == fv[1]) & (ju == fv[2]))[0][0])
    viol = l - so.collision_apply(prob, eta, inp["x"].ravel())
    held = np.zeros(viol.size, dtype=bool)
    held[sel] = True
    return dict(eta=eta, l=l, sel=sel, min_dist=float(so.min_pair_distance(prob, inp["pos"])), first=first,
                new=np.nonzero((viol > FEAS) & ~held)[0], max_v=float(viol.max()))


def _pair_from_ref(ref, inp):
    prob = inp["prob"]
    n = prob.K * prob.pairs
    both = _bits_of(np.concatenate([ref["sel"], ref["new"]]), n)
    sel, new = ref["sel"].astype(np.int64), ref["new"].astype(np.int64)
    return {"rows": sel, "min_dist": ref["min_dist"], "first": ref["first"], "bitmap0": _bits_of(sel, n), "eta": ref["eta"],
            "l": ref["l"], "w_eta": ref["eta"][sel], "w_l": ref["l"][sel], "chk_min": ref["min_dist"], "chk_first": ref["first"],
            "new_rows": new, "max_v": ref["max_v"], "bitmap": both, "rows2": sel, "min_dist2": ref["min_dist"],
            "first2": ref["first"], "new_rows2": new, "max_v2": ref["max_v"], "bitmap2": both,
            "scratch": np.zeros((n + 31) // 32, dtype=np.uint32)}


def _pair_compare(out, ref, inp):
    """tests/test_kernels_gpu.py: test_linearize_vs_oracle_synthetic and test_collision_violations_pass"""
    np.testing.assert_allclose(out["l"], ref["l"], rtol=0, atol=1e-12)
    np.testing.assert_allclose(out["eta"], ref["eta"], rtol=0, atol=1e-13)
    n = inp["prob"].K * inp["prob"].pairs
    for rows, md, first, bits in (("rows", "min_dist", "first", "bitmap0"), ("rows2", "min_dist2", "first2", None)):
        np.testing.assert_array_equal(np.sort(out[rows]), ref["sel"])
        assert abs(out[md] - ref["min_dist"]) < 1e-13 and out[first] == ref["first"]
        if bits:
            np.testing.assert_array_equal(out[bits], _bits_of(ref["sel"], n))
    assert abs(out["chk_min"] - ref["min_dist"]) < 1e-13 and out["chk_first"] == ref["first"]
    np.testing.assert_array_equal(out["w_eta"], out["eta"][out["rows"]])
    np.testing.assert_array_equal(out["w_l"], out["l"][out["rows"]])
    assert ref["new"].size > 3
    for new_rows, max_v, bits in (("new_rows", "max_v", "bitmap"), ("new_rows2", "max_v2", "bitmap2")):
        np.testing.assert_array_equal(np.sort(out[new_rows]), ref["new"])
        assert abs(out[max_v] - ref["max_v"]) < 1e-11
        np.testing.assert_array_equal(out[bits], _bits_of(np.concatenate([ref["sel"], ref["new"]]), n))
    assert not out["scratch"].any()


PAIR_ENTRIES = ("scp_linearize_pairs", "scp_select_pairs", "scp_check_avoidance", "scp_gather_rows", "scp_collision_violations",
                "scp_collision_violations_at", "scp_ctx_peek_scratch_map")
# (N, K, D, seed, one launch, size of the step to the new positions): 33 runs as one launch; 300 with the one-launch form switched off
# as prep + pass + one-workgroup compaction; 700 x 10 has 2.4 M rows, the three-launch compaction
PAIR_SHAPES = {"pair33": (33, 21, 3, 3, True, 0.2), "pair300": (300, 7, 2, 7, False, 1.0), "pair700": (700, 10, 2, 10, True, 0.2)}


def _pair_case(name):
    N, K, D, seed, single, step = PAIR_SHAPES[name]
    return Case(name, "pairwise", PAIR_ENTRIES, lambda: _pair_inputs(N, K, D, seed, step),
                lambda ctx, inp: _pair_run(ctx, inp, single_launch=single), _pair_reference, _pair_from_ref, _pair_compare,
                lambda inp: ws_pairwise(N, K, D, single))


GROW_PAIR = [(800, 10, 2, 31, 0.2), (320, 8, 2, 32, 1.0)]  # the three-launch compaction; the one-launch form with more sub-lists


def _grow_pairwise():
    def run(ctx, inp):
        return {f"{N}x{K}": _pair_run(ctx, one, with_reference=False)["new_rows"] for (N, K, _, _, _), one in zip(GROW_PAIR, inp)}

    return Case("grow_pairwise", "pairwise", PAIR_ENTRIES, lambda: [_pair_inputs(*s) for s in GROW_PAIR], run,
                ws=lambda inp: merge_ws(*(ws_pairwise(N, K, D) for N, K, D, _, _ in GROW_PAIR)))


# ---- family "trajectory": kinematics, bounds, relative step, products (no grown buffer; d_scratch / h_scratch) -----------------------
def _traj_inputs(name="ref_n4_k20", n_rel=12345, gemm=(50, 50, 130)):
    g = np.load(os.path.join(GOLDEN, name + ".npz"))
    prob = so.make_problem(int(g["N"]), float(g["T"]), float(g["h"]), float(g["R"]), g["space"], g["p0"], g["pf"], g["v0"], g["vf"])
    rng = np.random.default_rng(5)
    R, M, C = gemm
    return dict(g={k: g[k] for k in g.files}, prob=prob, a=rng.standard_normal(n_rel), b=rng.standard_normal(n_rel),
                A=rng.integers(-8, 9, (R, M)).astype(float), X=rng.integers(-8, 9, (M, C)).astype(float))


def _traj_run(ctx, inp):
    g, prob = inp["g"], inp["prob"]
    N, K = prob.N, prob.K
    p0, v0, pf, vf = (ctx.tensor(a) for a in (prob.p0, prob.v0, prob.pf, prob.vf))
    pos, vel = ctx.kinematics(N, K, 2, prob.h, ctx.tensor(g["acc"].reshape(N, K, 2)), p0, v0)
    lo, hi = ctx.fixed_bounds(N, K, 2, prob.h, LIMITS, g["space"], p0, v0, pf, vf)
    d, nb, rel = ctx.rel_step(ctx.tensor(inp["a"]), ctx.tensor(inp["b"]))
    Y = {m: _np(ctx.gemm(ctx.tensor(inp["A"]), ctx.tensor(inp["X"]), m)) for m in (0, 1)}
    return {"pos": _np(pos), "vel": _np(vel), "lo": _np(lo), "hi": _np(hi), "rel": np.array([d, nb, rel]), "Y0": Y[0], "Y1": Y[1]}


def _traj_reference(inp):
    g = inp["g"]
    a, b = inp["a"], inp["b"]
    return {"pos": g["pos_a4"], "vel": g["vel_a4"], "lo": np.hstack([g[f"l_{k}"] for k in ("jerk", "acc", "vel", "pos")]),
            "hi": np.hstack([g[f"u_{k}"] for k in ("jerk", "acc", "vel", "pos")]),
            "rel": np.array([np.linalg.norm(a - b), np.linalg.norm(b), np.linalg.norm(a - b) / np.linalg.norm(b)]),
            "Y0": inp["A"] @ inp["X"], "Y1": inp["A"] @ inp["X"]}


def _traj_compare(out, ref, inp):
    """tests/test_kernels_gpu.py: bitwise against the reference's fixtures, test_rel_step, test_gemm_f64 (whole numbers)"""
    for k in ("pos", "vel", "lo", "hi", "Y0", "Y1"):
        np.testing.assert_array_equal(out[k], ref[k], err_msg=k)
    assert abs(out["rel"][2] - ref["rel"][2]) < 1e-13 and np.abs(out["rel"][:2] - ref["rel"][:2]).max() < 1e-11


TRAJ_ENTRIES = ("scp_kinematics", "scp_fixed_bounds", "scp_rel_step", "scp_gemm_f64")


# ---- family "continuous": the continuous-time passes, the schedules and the holds (sep_ws) -------------------------------------------
R_SEP = 0.8
CT_SHAPE = dict(N=40, K=12, D=2, seed=5, S=4)
CT_GROW = dict(N=130, K=9, D=3, seed=21, S=4)


@functools.lru_cache(maxsize=None)
def _trajectories(N, K, D, seed):
    p0, v0, acc = sr.random_case(N, K, D, seed)
    pos, vel = sr.kinematics(p0, v0, acc, H)
    return pos, vel, acc


def _ct_inputs(shape=None):
    s = shape or CT_SHAPE
    return dict(host=_trajectories(s["N"], s["K"], s["D"], s["seed"]), S=s["S"])


def _dev(ctx, host):
    return tuple(ctx.tensor(np.ascontiguousarray(x)) for x in host)


def _sep_run(ctx, inp):
    pos, vel, acc = _dev(ctx, inp["host"])
    N, K, D = pos.shape
    st = ctx.check_separation(N, K, D, H, R_SEP, pos, vel, acc)
    return {"stats": dict(st), "solved": ctx.last_separation_solved(), "sampled": ctx.check_avoidance(N, K, D, R_SEP, pos)[0]}


def _sep_reference(inp):
    return sr.global_stats(*inp["host"], H, R_SEP)


def _sep_from_ref(ref, inp):
    st = {"min_dist": float(np.sqrt(max(ref["min_f"], 0.0))), "sample_min_dist": float(ref["sample_min_dist"]),
          "argmin_t": ref["argmin_t"], "argmin_row": ref["argmin_row"], "first_violation": ref["first_violation"],
          "n_violating": ref["n_violating"]}
    return {"stats": st, "sampled": float(ref["sample_min_dist"])}


def _sep_compare(out, ref, inp):
    import test_separation_gpu as t

    assert out["stats"]["sample_min_dist"] == out["sampled"]  # bitwise scp_check_avoidance's
    t.compare(out["stats"], inp["host"], H, R_SEP, label="ctx-state separation")


def _conf_run(ctx, inp):
    pos, vel, acc = _dev(ctx, inp["host"])
    N, K, D = pos.shape
    return {"list": ctx.list_conflicts(N, K, D, H, R_SEP, pos, vel, acc, capacity=CONF_CAP)}


CONF_CAP = 256


def _conf_reference(inp):
    return cfr.records(*inp["host"], H, R_SEP)


def _conflict_records(ref):
    from path_planning import _hip

    out = np.zeros(ref["rows"].size, dtype=_hip.CONFLICT_DTYPE)
    out["row"], out["min_dist"] = ref["rows"], np.sqrt(np.maximum(ref["f"], 0.0))
    out["t_min"], out["t_enter"], out["t_exit"], out["pieces"] = ref["t_min"], ref["t_enter"], ref["t_exit"], ref["pieces"]
    return out


def _conf_compare(out, ref, inp):
    import test_conflicts_gpu as t

    assert 0 < ref["rows"].size <= CONF_CAP
    t.compare(out["list"], inp["host"], ref, R_SEP, "ctx-state conflicts")


def _clr_run(ctx, inp):
    pos, vel, acc = _dev(ctx, inp["host"])
    N, K, D = pos.shape
    veh, step = ctx.clearance_profile(N, K, D, H, R_SEP, pos, vel, acc)
    return {"vehicle": veh, "step": step, "solved": ctx.last_clearance_solved()}


def _clr_reference(inp):
    return clr.profile(*inp["host"], H, R_SEP)


def _clr_from_ref(ref, inp):
    from path_planning import _hip

    out = {}
    for which in ("vehicle", "step"):
        e = ref[which]
        a = np.zeros(e["f"].size, dtype=_hip.CLEARANCE_DTYPE)
        a["min_dist"], a["t_min"], a["row"] = np.sqrt(np.maximum(e["f"], 0.0)), e["t"], e["row"]
        a["sample_min_dist"], a["n_violating"] = e["sample"], e["n_violating"]
        out[which] = a
    return out


def _clr_compare(out, ref, inp):
    import test_clearance_gpu as t

    t.compare(out["vehicle"], ref["vehicle"], ref, inp["host"], "vehicle ctx-state")
    t.compare(out["step"], ref["step"], ref, inp["host"], "step ctx-state")


def _dly_run(ctx, inp):
    pos, vel, acc = _dev(ctx, inp["host"])
    N, K, D = pos.shape
    return {"margins": ctx.delay_margins(N, K, D, H, R_SEP, pos, vel, acc, inp["S"]), "solved": ctx.last_delay_solved()}


def _dly_reference(inp):
    return dlr.margins(*inp["host"], H, R_SEP, inp["S"])


def _dly_from_ref(ref, inp):
    from path_planning import _hip

    a = np.zeros(ref["f"].shape, dtype=_hip.DELAY_DTYPE)
    a["min_dist"], a["t_min"], a["partner"], a["segment"] = np.sqrt(np.maximum(ref["f"], 0.0)), ref["t"], ref["b"], ref["g"]
    a["n_violating"] = ref["n_violating"]
    return {"margins": a}


def _dly_compare(out, ref, inp):
    import test_delay_gpu as t

    tol = 32 * sr.EPS * ref["s_max"] ** 2
    assert not t.near_threshold(ref, tol)  # (a condition on the inputs)
    t.compare(out["margins"], ref, inp["host"], "ctx-state delay")


def _lag_run(ctx, inp):
    pos, vel, acc = _dev(ctx, inp["host"])
    N, K, D = pos.shape
    mask = ctx.lag_conflicts(N, K, D, H, R_SEP, pos, vel, acc, inp["S"], device=True)
    delays, stats = ctx.schedule_starts(mask, inp["S"])
    return {"mask": _np(mask).view(np.uint64), "delays": delays, "schedule": stats, "solved": ctx.last_lag_solved()}


def _lag_reference(inp):
    mask, ref = sgr.masks(*inp["host"], H, R_SEP, inp["S"])
    delays, stats = sgr.greedy(mask, inp["S"])
    return dict(mask=mask, margins=ref, delays=delays, stats=stats)


def _lag_from_ref(ref, inp):
    return {"mask": ref["mask"], "delays": np.asarray(ref["delays"], dtype=np.int32), "schedule": dict(ref["stats"])}


def _lag_compare(out, ref, inp):
    """tests/test_stagger_gpu.py: the masks and the schedule of the masks, integers: equality"""
    import test_stagger_gpu as t

    assert t.near_threshold(ref["margins"], 32 * sr.EPS * ref["margins"]["s_max"] ** 2) == 0 and (ref["mask"] != 0).any()
    assert (out["mask"] == ref["mask"]).all()
    assert out["delays"].tolist() == list(ref["delays"]) and out["schedule"] == ref["stats"]


BATCH_SHAPE = (33, 5, 0.10, 1, 36)   # tests/test_stagger_search_gpu.py: a word boundary of `pending`, 36 >= 16 candidates
BATCH_GROW = (130, 20, 0.05, 5, 16)


def _batch_inputs(shape=BATCH_SHAPE):
    from path_planning.solvers.stagger import candidate_orders

    N, S, density, seed, B = shape
    return dict(mask=sgr.random_masks(N, S, density, seed), S=S, orders=np.asarray(candidate_orders(N, B, np.random.default_rng(seed + 100))))


def _batch_run(ctx, inp):
    out = {}
    for objective in ssr.OBJECTIVES:
        delays, stats, best = ctx.schedule_starts_batch(inp["mask"], inp["S"], inp["orders"], objective)
        out[objective] = {"delays": delays, "stats": {f: stats[f] for f in ssr.FIELDS}, "best": best}
    return out


def _batch_reference(inp):
    delays, stats = ssr.schedule_all(inp["mask"], inp["S"], inp["orders"])
    return dict(delays=delays, stats=stats)


def _batch_from_ref(ref, inp):
    from path_planning import _hip

    dt = _hip.START_SCHEDULE_STATS_DTYPE
    return {o: {"delays": np.asarray(ref["delays"], dtype=np.int32),
                "stats": {f: np.array([s[f] for s in ref["stats"]], dtype=dt[f]) for f in ssr.FIELDS},
                "best": ssr.best_of(ref["stats"], o)} for o in ssr.OBJECTIVES}


def _batch_compare(out, ref, inp):
    """tests/test_stagger_search_gpu.py: assert_matches"""
    for o in ssr.OBJECTIVES:
        assert out[o]["delays"].tolist() == [list(d) for d in ref["delays"]]
        for f in ssr.FIELDS:
            assert out[o]["stats"][f].tolist() == [s[f] for s in ref["stats"]], f
        assert out[o]["best"] == ssr.best_of(ref["stats"], o)


def tunnels(N, D, pairs, K=8):
    """tests/test_holds_gpu.py's: disjoint pairs that cross in segment 3, everybody else far apart and at rest"""
    pos, vel, acc = np.zeros((N, K, D)), np.zeros((N, K, D)), np.zeros((N, K, D))
    pos[:, :, 0] = 100.0 * (1 + np.arange(N))[:, None]
    pos[:, :, D - 1] += 3.0 * np.arange(N)[:, None]
    rel = 0.4 + 0.8 * (3 - np.arange(K))
    for i, j in pairs:
        pos[j] = pos[i]
        pos[i, :, 0] += 0.5 * rel
        pos[j, :, 0] -= 0.5 * rel
        vel[i, :, 0], vel[j, :, 0] = -2.0, 2.0
    return pos, vel, acc


R_HOLD, PAD = 0.5, 0.02


def _upd_inputs(N=6, pairs=((0, 4), (2, 3))):
    host = tunnels(N, 2, pairs)
    conflicts = _conflict_records(cfr.records(*host, H, R_HOLD))
    start = np.zeros(2, dtype=hdr.HOLD_DTYPE)  # a table that holds other rows too: they stay, between the new ones
    start["row"], start["margin"] = [1, int(conflicts["row"][3]) + 1], [0.25, 0.5]
    start["eta"][:, 1] = 1.0
    return dict(host=host, conflicts=conflicts, start=start)


def _upd_run(ctx, inp, capacity=None):
    pos, vel, acc = _dev(ctx, inp["host"])
    N, K, D = pos.shape
    t_dev, n_dev = ctx.hold_table(inp["start"], capacity=capacity or inp["start"].size + 2 * inp["conflicts"].size)
    t_dev, n_dev, needed = ctx.update_holds(N, K, D, H, R_HOLD, pos, vel, acc, inp["conflicts"], t_dev, n_dev, PAD, grow=False)
    return {"table": ctx.read_holds(t_dev, n_dev), "needed": needed}


def _upd_reference(inp):
    return hdr.update(inp["start"], *inp["host"], R_HOLD, inp["conflicts"], PAD)


def _upd_compare(out, ref, inp):
    import test_holds_gpu as t

    t.compare_tables(out["table"], ref, "ctx-state holds")
    assert out["needed"] == ref.size > inp["start"].size


APPLY_SHAPE = dict(N=7, K=6, D=2, h=0.3, seed=102, held=3, free=5)
APPLY_GROW = dict(N=90, K=9, D=3, h=0.3, seed=103, held=40, free=90)


def _apply_inputs(shape=None):
    s = shape or APPLY_SHAPE
    N, K, D, h = s["N"], s["K"], s["D"], s["h"]
    rng = np.random.default_rng(s["seed"])
    pos, p0, v0 = rng.uniform(0.0, 4.0, (N, K, D)), rng.uniform(0.0, 4.0, (N, D)), rng.uniform(-1.0, 1.0, (N, D))
    prob = so.make_problem(N, K * h + 1e-9, h, R_SEP, [-2.0] * D + [6.0] * D, p0, p0, v0, v0)
    assert prob.K == K
    eta, l, dist = so.linearize_pairs(prob, pos)
    selected = np.nonzero(dist - R_SEP < 0.5)[0]
    free = np.setdiff1d(np.arange(dist.size), selected)
    assert selected.size >= s["held"] and free.size >= s["free"]
    rows = np.concatenate([rng.choice(selected, s["held"], replace=False), rng.choice(free, s["free"], replace=False)])
    table = np.zeros(rows.size, dtype=hdr.HOLD_DTYPE)
    table["row"] = np.sort(rows)
    e = rng.normal(size=(rows.size, D))
    table["eta"][:, :D] = e / np.linalg.norm(e, axis=1)[:, None]
    table["margin"] = rng.uniform(0.0, 0.4, rows.size)
    return dict(prob=prob, pos=pos, table=table, eta=eta, l=l, selected=selected, n_free=s["free"])


def _apply_run(ctx, inp):
    from path_planning import _hip

    prob = inp["prob"]
    pp = _hip.PairPass(ctx, prob.N, prob.K, prob.D, prob.R, prob.h)
    p0, v0 = ctx.tensor(prob.p0), ctx.tensor(prob.v0)
    pp.linearize(ctx.tensor(inp["pos"]), p0, v0, 0.5)
    t_dev, n_dev = ctx.hold_table(inp["table"])
    new = pp.apply_holds(t_dev, n_dev, p0, v0)
    held = inp["table"]["row"].astype(np.int64)
    return {"new": _np(new), "bitmap": _np(pp.bitmap).view(np.uint32), "eta_held": _np(pp.eta_rows())[held], "l_held": _np(pp.l_rows())[held]}


def _apply_reference(inp):
    prob = inp["prob"]
    bits0 = _bits_of(inp["selected"], prob.K * prob.pairs)
    eta, l, bits, new = hdr.apply(inp["table"], prob.N, prob.K, prob.D, prob.h, prob.R, prob.p0, prob.v0, inp["eta"], inp["l"], bits0)
    return dict(eta=eta, l=l, bits=bits, new=new)


def _apply_from_ref(ref, inp):
    held = inp["table"]["row"].astype(np.int64)
    return {"new": np.asarray(ref["new"], dtype=np.int64), "bitmap": ref["bits"], "eta_held": ref["eta"][held], "l_held": ref["l"][held]}


def _apply_compare(out, ref, inp):
    """tests/test_holds_gpu.py: test_apply_against_the_reference"""
    held = inp["table"]["row"].astype(np.int64)
    assert out["new"].tolist() == np.asarray(ref["new"]).tolist() and (np.diff(out["new"]) > 0).all() and out["new"].size == inp["n_free"]
    assert np.array_equal(out["bitmap"], ref["bits"])
    assert out["eta_held"].tobytes() == ref["eta"][held].tobytes()
    err = np.abs(out["l_held"] - ref["l"][held])
    assert (err <= 4 * EPS * np.maximum(1.0, np.abs(ref["l"][held]))).all()


def _ct(name, entries, run, reference, from_ref, compare, ws, inputs=_ct_inputs):
    return Case(name, "continuous", entries, inputs, run, reference, from_ref, compare, ws)


def _ct_ws(fn):
    s = CT_SHAPE
    return lambda inp: fn(s["N"], s["K"], s["D"])


def _grow_continuous():
    g = CT_GROW
    N, K, D, S = g["N"], g["K"], g["D"], g["S"]
    pairs160 = tuple((2 * m, 2 * m + 1) for m in range(160))

    def inputs():
        return dict(ct=_ct_inputs(g), batch=_batch_inputs(BATCH_GROW), upd=_upd_inputs(320, pairs160), apply=_apply_inputs(APPLY_GROW))

    def run(ctx, inp):
        out = {"sep": _sep_run(ctx, inp["ct"])["stats"]["n_violating"], "conf": _conf_run(ctx, inp["ct"])["list"].size,
               "clr": _clr_run(ctx, inp["ct"])["solved"], "dly": _dly_run(ctx, inp["ct"])["solved"],
               "lag": _lag_run(ctx, inp["ct"])["solved"], "batch": _batch_run(ctx, inp["batch"])["makespan"]["best"],
               "upd": _upd_run(ctx, inp["upd"])["needed"], "apply": _apply_run(ctx, inp["apply"])["new"].size}
        return out

    def ws(inp):
        return merge_ws(ws_check_separation(N, K, D), ws_list_conflicts(N, K, D, CONF_CAP), ws_clearance(N, K, D), ws_delay(N, K, D, S),
                        ws_lag(N, K, D), ws_batch(BATCH_GROW[0], BATCH_GROW[4]), ws_update_holds(inp["upd"]["conflicts"].size, 2),
                        ws_apply_holds(inp["apply"]["table"].size), ws_pairwise(APPLY_GROW["N"], APPLY_GROW["K"], APPLY_GROW["D"], linearize_only=True))

    return Case("grow_continuous", "continuous", (), inputs, run, ws=ws)


# ---- family "obstacle": the map, the searches on it, the distance field (sep_ws, rast_ws) ---------------------------------------------
def _by_name(module, name):
    return {c.name: c for c in module.all_cases()}[name]


def _raster_ws(c):
    from path_planning.scenarios.obstacles import pack_shapes

    packed = pack_shapes(c.D, **c.shapes())
    n_shapes, n_vertices = len(packed["shapes"]), len(np.asarray(packed["vertices"]).reshape(-1, 2))
    o_items = (((n_shapes * 80 + 15) & ~15) + n_vertices * 16 + 15) & ~15
    cells = int(np.prod(c.dims))
    # a shape is one work item of 32 bytes per 1024 cells of its range, rounded up per axis: at most 8 more than cells / 1024
    return {"rast_ws_bytes": (o_items, o_items + n_shapes * (cells // 1024 + 8) * 32)}


def _raster_run(ctx, inp):
    from path_planning import _hip
    from path_planning.scenarios.obstacles import pack_shapes

    c = inp["c"]
    grid = _hip.occupancy_grid(c.D, c.origin, c.cell, c.dims)
    return {"occ": _np(ctx.rasterize_shapes(c.D, grid, pack_shapes(c.D, **c.shapes()), c.margin))}


def _raster_case(name, cname):
    def compare(out, ref, inp):
        """tests/test_rasterize_gpu.py: the grid, cell for cell"""
        assert set(np.unique(out["occ"]).tolist()) <= {0, 1}
        np.testing.assert_array_equal(out["occ"], ref)

    return Case(name, "obstacle", ("scp_rasterize_shapes",), lambda: dict(c=rzc.by_name(cname)), _raster_run, lambda inp: inp["c"].want(),
                lambda ref, inp: {"occ": np.asarray(ref)}, compare, lambda inp: _raster_ws(inp["c"]))


def _paths_run(ctx, inp):
    from path_planning import _hip

    c = inp["c"]
    g = _grid(c.D, c.origin, c.cell, c.occ)
    _, sat = ctx.occupancy_prepare(c.D, g, c.occ)
    edges = ctx.lattice_edges(c.D, g, sat, c.stride, c.clearance)
    p0, pf = ctx.tensor(c.p0), ctx.tensor(c.pf)
    ref = ctx.tensor(c.ref_in())
    path, info, dist, n_failed = ctx.reference_paths(c.N, c.K, c.D, g, c.stride, edges, p0, pf, c.max_path, ref, want_dist=True)
    out = {"sat": _np(sat), "edges": _np(edges).view(np.uint32), "ref": _np(ref), "path": _np(path), "dist": _np(dist).view(np.uint16),
           "info": _np(info).view(_hip.PATH_INFO_DTYPE)[:c.N].copy(), "n_failed": int(n_failed.item())}
    ref2 = ctx.tensor(c.ref_in())  # without the optional outputs the paths live in the context's workspace
    _, info2, _, n2 = ctx.reference_paths(c.N, c.K, c.D, g, c.stride, edges, p0, pf, c.max_path, ref2, want_path=False)
    out.update(ref_ws=_np(ref2), info_ws=_np(info2).view(_hip.PATH_INFO_DTYPE)[:c.N].copy(), n_failed_ws=int(n2.item()))
    hops, src_node, dst_node, hdist = ctx.lattice_distances(c.D, g, c.stride, edges, p0, pf, want_dist=True)
    out.update(hops=_np(hops).view(np.uint16), src_node=_np(src_node), dst_node=_np(dst_node), hop_dist=_np(hdist).view(np.uint16))
    return out


def _paths_reference(inp):
    c = inp["c"]
    want = c.want()
    hops, src, dst, dist, edges = apr.hop_matrix(c.D, c.origin, c.cell, c.occ, c.stride, c.clearance, c.p0, c.pf)
    return dict(want=want, hops=hops, src=src, dst=dst, dist=dist, sat=cor.summed_table(c.occ))


def _paths_from_ref(ref, inp):
    w = ref["want"]
    return {"sat": ref["sat"].astype(np.int32), "edges": w["edges"], "ref": w["ref"], "path": w["path"], "dist": w["dist"], "info": w["info"],
            "n_failed": int(w["n_failed"]), "ref_ws": w["ref"], "info_ws": w["info"], "n_failed_ws": int(w["n_failed"]),
            "hops": ref["hops"], "src_node": ref["src"].astype(np.int32), "dst_node": ref["dst"].astype(np.int32), "hop_dist": ref["dist"]}


def _paths_compare(out, ref, inp):
    """tests/test_reference_path_gpu.py and tests/test_assign_paths_gpu.py: integers exactly, the points bit for bit"""
    w = ref["want"]
    np.testing.assert_array_equal(out["sat"], ref["sat"])
    for k in ("edges", "info", "path", "dist"):
        np.testing.assert_array_equal(out[k], w[k], err_msg=k)
    for k, i, n in (("ref", "info", "n_failed"), ("ref_ws", "info_ws", "n_failed_ws")):
        np.testing.assert_array_equal(out[k].view(np.uint64), w["ref"].view(np.uint64), err_msg=k)
        np.testing.assert_array_equal(out[i], w["info"], err_msg=i)
        assert out[n] == w["n_failed"]
    for k, r in (("hops", "hops"), ("src_node", "src"), ("dst_node", "dst"), ("hop_dist", "dist")):
        np.testing.assert_array_equal(out[k], ref[r], err_msg=k)


PATH_ENTRIES = ("scp_occupancy_prepare", "scp_lattice_edges", "scp_reference_paths", "scp_lattice_distances")


def _weighted_run(ctx, inp):
    from path_planning import _hip

    c = inp["c"]
    g = _grid(c.D, c.origin, c.cell, c.occ)
    occ, sat = ctx.occupancy_prepare(c.D, g, c.occ)
    edges = ctx.lattice_edges(c.D, g, sat, c.stride, c.clearance)
    field = ctx.obstacle_distance(c.D, g, occ, 1)
    pen = ctx.lattice_penalties(c.D, g, field, c.stride, c.prefer, c.weight)
    p0, pf = ctx.tensor(c.p0), ctx.tensor(c.pf)
    out = {"field": _np(field).view(np.uint32), "pen": _np(pen).view(np.uint32)}
    for tag, want_path in (("", True), ("_ws", False)):  # without `path` the paths live in the context's workspace
        ref = ctx.tensor(c.ref_in())
        path, info, path_cost, cost, n_failed = ctx.reference_paths_weighted(c.N, c.K, c.D, g, c.stride, edges, p0, pf, c.max_path, ref,
                                                                             pen=pen, want_path=want_path, want_cost=want_path)
        out.update({"ref" + tag: _np(ref), "info" + tag: _np(info).view(_hip.PATH_INFO_DTYPE)[:c.N].copy(),
                    "path_cost" + tag: _np(path_cost).view(np.uint32)[:c.N].copy(), "n_failed" + tag: int(n_failed.item())})
        if want_path:
            out.update(path=_np(path), cost=_np(cost).view(np.uint32)[:c.N].copy())
    costs, src_node, dst_node, _ = ctx.lattice_costs(c.D, g, c.stride, edges, pf, p0, pen=pen)
    out.update(costs=_np(costs).view(np.uint32), src_node=_np(src_node), dst_node=_np(dst_node))
    return out


def _weighted_reference(inp):
    c = inp["c"]
    want = c.want()
    costs, src, dst, _ = wpr.cost_matrix(c.D, c.origin, c.cell, c.dims, c.stride, want["edges"], want["pen"], c.pf, c.p0)
    return dict(want=want, costs=costs, src=src, dst=dst)


def _weighted_from_ref(ref, inp):
    w = ref["want"]
    out = {"field": w["field"], "pen": w["pen"], "path": w["path"], "cost": w["cost"], "costs": ref["costs"],
           "src_node": ref["src"].astype(np.int32), "dst_node": ref["dst"].astype(np.int32)}
    for tag in ("", "_ws"):
        out.update({"ref" + tag: w["ref"], "info" + tag: w["info"], "path_cost" + tag: w["path_cost"], "n_failed" + tag: int(w["n_failed"])})
    return out


def _weighted_compare(out, ref, inp):
    """tests/test_weighted_path_gpu.py: every output equals the restatement"""
    w = ref["want"]
    for k in ("field", "pen", "path", "cost"):
        np.testing.assert_array_equal(out[k].reshape(w[k].shape), w[k], err_msg=k)
    for tag in ("", "_ws"):
        np.testing.assert_array_equal(out["ref" + tag].view(np.uint64), w["ref"].view(np.uint64))
        np.testing.assert_array_equal(out["info" + tag], w["info"])
        np.testing.assert_array_equal(out["path_cost" + tag], w["path_cost"])
        assert out["n_failed" + tag] == w["n_failed"]
    for k, r in (("costs", "costs"), ("src_node", "src"), ("dst_node", "dst")):
        np.testing.assert_array_equal(out[k], ref[r], err_msg=k)


WEIGHTED_ENTRIES = ("scp_obstacle_distance", "scp_lattice_penalties", "scp_reference_paths_weighted", "scp_lattice_costs")


def _shorten_run(ctx, inp):
    from path_planning import _hip

    c = inp["c"]
    g = _grid(c.D, c.origin, c.cell, c.occ)
    _, sat = ctx.occupancy_prepare(c.D, g, c.occ)
    edges = ctx.lattice_edges(c.D, g, sat, c.stride, c.clearance)
    p0, pf = ctx.tensor(c.p0), ctx.tensor(c.pf)
    out = {}
    for tag, want_kept in (("", True), ("_ws", False)):  # without `kept` the kept nodes live in the context's workspace
        ref = ctx.tensor(c.ref_in())
        path, info, _, _ = ctx.reference_paths(c.N, c.K, c.D, g, c.stride, edges, p0, pf, c.max_path, ref)
        kept, rec = ctx.shorten_paths(c.N, c.K, c.D, g, sat, c.stride, c.clearance, p0, pf, c.max_path, path, info, ref, want_kept=want_kept)
        out.update({"ref" + tag: _np(ref), "out" + tag: _np(rec).view(_hip.SHORTEN_INFO_DTYPE)[:c.N].copy()})
        if want_kept:
            out["kept"] = _np(kept)
    return out


def _shorten_from_ref(ref, inp):
    from path_planning import _hip

    rec = np.zeros(ref["out"].size, dtype=_hip.SHORTEN_INFO_DTYPE)
    for f in ("n_kept", "n_vertices", "length", "length_before"):
        rec[f] = ref["out"][f]
    return {"ref": ref["ref"], "out": rec, "kept": ref["kept"], "ref_ws": ref["ref"], "out_ws": rec}


def _shorten_compare(out, ref, inp):
    """tests/test_shorten_gpu.py: _assert_equal"""
    np.testing.assert_array_equal(out["kept"], ref["kept"])
    for tag in ("", "_ws"):
        np.testing.assert_array_equal(out["ref" + tag].view(np.uint64), ref["ref"].view(np.uint64))
        for f in ("n_kept", "n_vertices"):
            np.testing.assert_array_equal(out["out" + tag][f], ref["out"][f], err_msg=f)
        for f in ("length", "length_before"):
            np.testing.assert_array_equal(out["out" + tag][f].view(np.uint64), ref["out"][f].view(np.uint64), err_msg=f)


FIELD_CASES = {name: (D, occ) for name, D, occ in odc.field_cases()}


def _field_inputs(fname):
    return dict(D=FIELD_CASES[fname][0], occ=FIELD_CASES[fname][1])


def _field_run(ctx, inp):
    D, occ = inp["D"], inp["occ"]
    g = _grid(D, [0.0] * D, 1.0, occ)
    d_occ, _ = ctx.occupancy_prepare(D, g, occ)
    return {f"gap{gap}": _np(ctx.obstacle_distance(D, g, d_occ, gap)).view(np.uint32) for gap in (0, 1)}


def _field_case(name, fname):
    def reference(inp):
        return {f"gap{gap}": odc.field_want(fname, inp["occ"], gap) for gap in (0, 1)}

    def compare(out, ref, inp):
        """tests/test_obstacle_distance_gpu.py: the field, cell for cell"""
        for k in ref:
            np.testing.assert_array_equal(out[k], ref[k], err_msg=k)

    return Case(name, "obstacle", ("scp_obstacle_distance", "scp_occupancy_prepare"), lambda: _field_inputs(fname),
                _field_run, reference, lambda ref, inp: {k: np.asarray(v, dtype=np.uint32) for k, v in ref.items()}, compare,
                lambda inp: ws_distance(inp["occ"]))


def _oclr_run(ctx, inp):
    p = inp["p"]
    g = _grid(p.D, p.origin, p.cell, p.occ)
    d_occ, sat = ctx.occupancy_prepare(p.D, g, p.occ)
    field = ctx.obstacle_distance(p.D, g, d_occ, 1)
    got, steps = ctx.obstacle_clearance(p.N, p.K, p.D, p.h, g, sat, field, p.P, ctx.tensor(p.pos), ctx.tensor(p.vel), ctx.tensor(p.acc))
    return {"records": got, "step_min": steps}


def _oclr_from_ref(ref, inp):
    from path_planning import _hip

    rec = np.zeros(ref[0].size, dtype=_hip.OBSTACLE_STATS_DTYPE)
    for f in ref[0].dtype.names:
        rec[f] = ref[0][f]
    return {"records": rec, "step_min": np.asarray(ref[1], dtype=np.uint64)}


def _oclr_compare(out, ref, inp):
    """tests/test_obstacle_distance_gpu.py: test_clearance_equals_the_reference"""
    for f in ref[0].dtype.names:
        np.testing.assert_array_equal(out["records"][f], ref[0][f], err_msg=f)
    np.testing.assert_array_equal(out["step_min"], ref[1])


def _corridor_inputs(dims=(37, 29), D=2, N=5, K=7):
    import corridor_cases as cc

    rng = np.random.default_rng(17 + len(dims) + dims[0])
    occ = cc.random_grid(rng, dims)
    origin, cell = [-1.5, 0.25, 2.0][:D], 0.4
    ref = cc.random_walk_reference(rng, occ, D, origin, cell, N, K)
    rng = np.random.default_rng(23)
    pos = ref[:, :K] + rng.normal(0, 0.2, (N, K, D))
    return dict(D=D, occ=occ, origin=origin, cell=cell, ref=ref, pos=pos, vel=rng.normal(0, 1.5, (N, K, D)), acc=rng.uniform(-15, 15, (N, K, D)))


GROW, SHRINK, TOL = 3, 0.07, 0.3


def _corridor_run(ctx, inp):
    D, ref = inp["D"], inp["ref"]
    N, K = ref.shape[0], ref.shape[1] - 1
    g = _grid(D, inp["origin"], inp["cell"], inp["occ"])
    _, sat = ctx.occupancy_prepare(D, g, inp["occ"])
    cells, n_blocked = ctx.corridor_boxes(N, K, D, g, sat, ctx.tensor(ref), GROW)
    lo, hi, n_open = ctx.corridor_state_boxes(N, K, D, g, cells, SHRINK)
    chk = ctx.check_corridor(N, K, D, H, g, cells, ctx.tensor(inp["pos"]), ctx.tensor(inp["vel"]), ctx.tensor(inp["acc"]), TOL)
    return {"cells": _np(cells), "n_blocked": int(n_blocked.item()), "lo": _np(lo), "hi": _np(hi), "n_open": int(n_open.item()),
            "check": {f: chk[f].copy() for f in ("max_excess", "segment", "n_blocked", "n_outside")}}


def _corridor_reference(inp):
    D, origin, cell = inp["D"], inp["origin"], inp["cell"]
    cells, blocked = cor.corridor_boxes(D, origin, cell, cor.summed_table(inp["occ"]), inp["ref"], GROW)
    lo, hi, n_open = cor.state_boxes(D, origin, cell, cells, SHRINK)
    return dict(cells=cells, blocked=blocked, lo=lo, hi=hi, n_open=n_open,
                check=cor.check_corridor(D, H, origin, cell, cells, inp["pos"], inp["vel"], inp["acc"], TOL))


def _corridor_from_ref(ref, inp):
    chk = {"max_excess": np.asarray(ref["check"]["max_excess"], dtype=np.float64)}
    chk.update({f: np.asarray(ref["check"][f], dtype=np.uint32) for f in ("segment", "n_blocked", "n_outside")})
    return {"cells": np.asarray(ref["cells"], dtype=np.int32), "n_blocked": int(ref["blocked"]), "lo": ref["lo"], "hi": ref["hi"],
            "n_open": int(ref["n_open"]), "check": chk}


def _corridor_compare(out, ref, inp):
    """tests/test_corridor_gpu.py: the boxes, the state boxes and the check, bit for bit"""
    np.testing.assert_array_equal(out["cells"], ref["cells"])
    assert out["n_blocked"] == ref["blocked"] and out["n_open"] == ref["n_open"]
    for k in ("lo", "hi"):
        np.testing.assert_array_equal(out[k].view(np.uint64), ref[k].view(np.uint64))
    for f in ("segment", "n_blocked", "n_outside"):
        np.testing.assert_array_equal(out["check"][f], ref["check"][f], err_msg=f)
    np.testing.assert_array_equal(out["check"]["max_excess"].view(np.uint64), ref["check"]["max_excess"].view(np.uint64))


OBSTACLE_GROW = dict(paths="rand2d_50x37_s1_c0", weighted="limit", shorten="rand2d_50x37_s1_c0", field2="65x67_corner",
                     field3="20x20x20_one_cell", raster="130x67_300_random")


def _grow_obstacle():
    g = OBSTACLE_GROW

    def inputs():
        return dict(paths=dict(c=_by_name(rpc, g["paths"])), weighted=dict(c=_by_name(wpc, g["weighted"])),
                    shorten=dict(c=_by_name(stc, g["shorten"])), raster=dict(c=rzc.by_name(g["raster"])))

    def run(ctx, inp):
        out = {"paths": _paths_run(ctx, inp["paths"])["n_failed_ws"], "weighted": _weighted_run(ctx, inp["weighted"])["n_failed_ws"],
               "shorten": _shorten_run(ctx, inp["shorten"])["out_ws"]["n_kept"]}
        for f in (g["field2"], g["field3"]):
            out[f] = _field_run(ctx, _field_inputs(f))["gap1"].reshape(-1)[:1]
        out["raster"] = int(_raster_run(ctx, inp["raster"])["occ"].sum())
        return out

    def ws(inp):
        c, w = inp["paths"]["c"], inp["weighted"]["c"]
        return merge_ws(ws_paths(c.N, c.max_path), ws_paths(w.N, w.max_path), ws_distance(FIELD_CASES[g["field2"]][1]),
                        ws_distance(FIELD_CASES[g["field3"]][1]), _raster_ws(inp["raster"]["c"]))

    return Case("grow_obstacle", "obstacle", (), inputs, run, ws=ws)


# ---- family "assign": goal assignment, the line check, the scenario generator (asg_ws, asgw_ws, gen_ws) ------------------------------
ASSIGN_NAME, COSTS_NAME, MIN_SEP = "uniform-2d-65", "random-65", 0.8
STAT_KEYS = ("cost_q", "cost_q_identity", "quantum", "phases", "rounds", "bids", "status")
LINE_KEYS = ("min_approach", "arg_i", "arg_j", "n_close", "n_opposed")


def _assign_inputs():
    start, goal = asr.gpu_cases()[ASSIGN_NAME]
    return dict(start=start, goal=goal)


def _assign_run(ctx, inp, wide=False):
    fn = ctx.assign_goals_wide if wide else ctx.assign_goals
    goal_of, st, prices = fn(inp["start"], inp["goal"], want_prices=True)
    out = {"goal_of": _np(goal_of)[0], "prices": _np(prices)[0], "stats": {k: st[k][:1].copy() for k in STAT_KEYS}}
    if not wide:
        for tag, gof in (("before", None), ("after", goal_of[0])):
            line = ctx.straight_line_check(inp["start"], inp["goal"], gof, MIN_SEP)
            out["line_" + tag] = {k: line[k][:1].copy() for k in LINE_KEYS}
    return out


def _assign_reference(inp):
    ref = asr.reference(ASSIGN_NAME)
    return dict(ref=ref, before=asr.line_check(inp["start"], inp["goal"], None, MIN_SEP),
                after=asr.line_check(inp["start"], inp["goal"], ref["goal_of"], MIN_SEP))


def _assign_from_ref(ref, inp, wide=False):
    from path_planning import _hip

    r = ref["ref"]
    out = {"goal_of": np.asarray(r["goal_of"], dtype=np.int32), "prices": np.asarray(r["prices"], dtype=np.int64),
           "stats": {k: np.array([r[k]], dtype=_hip.ASSIGN_STATS_DTYPE[k]) for k in STAT_KEYS}}
    if not wide:
        for tag in ("before", "after"):
            out["line_" + tag] = {k: np.array([ref[tag][k]], dtype=_hip.LINE_STATS_DTYPE[k]) for k in LINE_KEYS}
    return out


def _bits(x):
    return np.float64(x).view(np.uint64)


def _assign_compare(out, ref, inp, wide=False):
    """tests/test_assignment_gpu.py: _compare_assign and _compare_line, bitwise"""
    r = ref["ref"]
    np.testing.assert_array_equal(out["goal_of"], r["goal_of"])
    np.testing.assert_array_equal(out["prices"], r["prices"])
    for k in STAT_KEYS:
        assert (_bits(out["stats"][k][0]) == _bits(r[k])) if k == "quantum" else (int(out["stats"][k][0]) == int(r[k])), k
    if not wide:
        for tag in ("before", "after"):
            for k in LINE_KEYS:
                got, want = out["line_" + tag][k][0], ref[tag][k]
                assert (_bits(got) == _bits(want)) if k == "min_approach" else (int(got) == int(want)), (tag, k)
        assert int(out["line_after"]["n_opposed"][0]) == 0


def _costs_run(ctx, inp):
    goal_of, st, prices = ctx.assign_costs(inp["c"], want_prices=True)
    return {"goal_of": _np(goal_of)[0], "prices": _np(prices)[0], "stats": {k: st[k][:1].copy() for k in STAT_KEYS}}


GEN_SHAPE, GEN_GROW = (16, 2, (11, 12)), (1000, 2, (11, 12, 13))
GEN_INT = ("sweeps", "unmet_blocks", "conflicts", "ok")


def _gen_run(ctx, inp):
    N, D, seeds = inp["shape"]
    init, goal, space, st = ctx.generate_grid_swap(N, D, list(seeds))
    return {"init": _np(init), "goal": _np(goal), "space": _np(space), "stats": {k: st[k].copy() for k in GEN_INT + ("min_approach",)}}


def _gen_reference(inp):
    N, D, seeds = inp["shape"]
    return [sdr.generate(N, s, D) for s in seeds]


def _gen_from_ref(ref, inp):
    from path_planning import _hip

    dt = _hip.GEN_STATS_DTYPE
    return {"init": np.stack([r[0] for r in ref]), "goal": np.stack([r[1] for r in ref]), "space": np.stack([r[2] for r in ref]),
            "stats": {k: np.array([r[3][k] for r in ref], dtype=dt[k]) for k in GEN_INT + ("min_approach",)}}


def _gen_compare(out, ref, inp):
    """tests/test_scenario_device_gpu.py: _compare"""
    for b, (ri, rg, rs, rst) in enumerate(ref):
        for k, want in (("init", ri), ("goal", rg), ("space", rs)):
            np.testing.assert_array_equal(out[k][b], want, err_msg=f"{k} b={b}")
        for k in GEN_INT:
            assert int(out["stats"][k][b]) == int(rst[k]), (k, b)
        ma, rma = float(out["stats"]["min_approach"][b]), rst["min_approach"]
        assert ma == rma or abs(ma - rma) <= np.spacing(rma), (ma, rma)


def _grow_assign():
    def inputs():
        scen = [asr.uniform(130, 3, 40 + b) for b in range(4)]
        return dict(start=np.stack([s for s, _ in scen]), goal=np.stack([g for _, g in scen]), c=apr.gpu_matrices()["random-130"],
                    shape=GEN_GROW)

    def run(ctx, inp):
        goal_of, st, _ = ctx.assign_goals(inp["start"], inp["goal"])
        wide, _, _ = ctx.assign_goals_wide(inp["start"], inp["goal"])
        line = ctx.straight_line_check(inp["start"], inp["goal"], goal_of, MIN_SEP)
        return {"same": bool((_np(goal_of) == _np(wide)).all()), "line": line["n_close"].copy(), "costs": _costs_run(ctx, inp)["goal_of"],
                "gen": _gen_run(ctx, inp)["stats"]["ok"]}

    return Case("grow_assign", "assign", (), inputs, run,
                ws=lambda inp: merge_ws(ws_line_check(4, 130), ws_assign_wide(4, 130), ws_generator(len(GEN_GROW[2]), GEN_GROW[0])))


# ---- family "qp": the joint QP on a context (ticket words 1 and 2) ---------------------------------------------------------------------
def _qp_problem(n, seed):
    from path_planning.scenarios.position_generator import generate_positions

    p0, pf = generate_positions(n, 0.8, seed=seed)
    return so.make_problem(n, 10.0, 0.2, 0.8, [0, 0, 20, 20], p0, pf)


def _qp_inputs(n=10, seed=7):
    prob = _qp_problem(n, seed)
    x0, _, _ = qo.admm_structured(prob, st=qo.Settings(cg_iters=3))
    pos, _ = so.kinematics(prob, x0)
    eta, l_col, dist = so.linearize_pairs(prob, pos)
    return dict(prob=prob, x0=x0, pos=pos, eta=eta, l=l_col, dist=dist, W=np.nonzero(dist - prob.R < 0.5)[0])


def _make_qp(ctx, prob, row_capacity=None, **kw):
    from path_planning import _hip

    qp = _hip.QP(ctx, prob.N, prob.K, prob.D, prob.h, _hip.default_settings(**kw), row_capacity=row_capacity)
    qp.set_problem(LIMITS, np.concatenate([prob.pos_min, prob.pos_max]), ctx.tensor(prob.p0), ctx.tensor(prob.v0), ctx.tensor(prob.pf),
                   ctx.tensor(prob.vf))
    return qp


INFO_KEYS = ("status_val", "iter", "rho_updates", "cg_iters_total", "working_rows", "pipeline", "persist_gave_up")


def _info(info):
    return {k: info[k] for k in INFO_KEYS}


def _qp_lean_run(ctx, inp, max_iter=10000, fault=False):
    """QP#0, then the joint QP with rows recomputed from the linearisation point (scp_qp_add_rows_at): one PCG step per ADMM
    step, K = 50 <= 64 -- the lean persistent kernel"""
    import torch

    prob = inp["prob"]
    qp = _make_qp(ctx, prob, cg_iters=1, max_iter=max_iter)
    try:
        qp.reset(None)
        out = {"info0": _info(qp.solve()), "x_qp0": _np(qp.solution())}
        qp.reset(ctx.tensor(inp["x0"]))
        qp.add_rows_at(torch.as_tensor(inp["W"], dtype=torch.int64, device=ctx.tdev), ctx.tensor(inp["pos"]), ctx.tensor(prob.p0),
                       ctx.tensor(prob.v0), prob.R)
        if fault:
            assert qp.debug_set("persist_fault", 1) == 1
        out["info"] = _info(qp.solve())
        if fault:
            assert qp.debug_set("persist_fault", -1) == 0
        yf, yc = qp.duals()
        out.update(x=_np(qp.solution()), yf=_np(yf), yc=_np(yc), w_l=_np(qp.peek("w_l")))
    finally:
        qp.close()
    return out


def _qp_lean_reference(inp):
    prob = inp["prob"]
    x_qp0, _, i0 = qo.admm_structured(prob, st=qo.Settings(cg_iters=1))
    st = qo.Settings(cg_iters=1, max_iter=10000, max_rounds=1)
    x, y, io = qo.admm_structured(prob, inp["eta"], inp["l"], inp["dist"], x0=inp["x0"], st=st, rows0=inp["W"])
    return dict(x_qp0=x_qp0, i0=i0, x=x, y=y, io=io)


def _qp_from_ref(ref, inp, cg=1, use_mfma=1):
    prob, io, y = inp["prob"], ref["io"], ref["y"]
    # (2-D, K <= 64, one PCG step, rows: the lean persistent kernel with 8 agents per workgroup; otherwise choose_pipeline)
    lean = cg == 1 and use_mfma == 1 and prob.K <= 64 and prob.D == 2 and prob.N <= 2048
    pipe = "persistent8-lean" if lean else bxc.qc.expected_pipeline(prob.K, prob.N * prob.D, inp["W"].size, cg, use_mfma)
    out = {"info": dict(status_val=io["status_val"], iter=io["iter"], rho_updates=io["rho_updates"], cg_iters_total=cg * io["iter"],
                        working_rows=int(inp["W"].size), pipeline=pipe, persist_gave_up=0),
           "x": ref["x"], "yf": np.hstack([y[k].ravel() for k in ("jerk", "acc", "vel", "pos")]), "yc": y["col"], "w_l": inp["l"][inp["W"]]}
    if "x_qp0" in ref:
        i0 = ref["i0"]
        out["info0"] = dict(status_val=i0["status_val"], iter=i0["iter"], rho_updates=i0["rho_updates"], cg_iters_total=i0["iter"],
                            working_rows=0, pipeline="qp0", persist_gave_up=0)
        out["x_qp0"] = ref["x_qp0"]
    return out


def _qp_compare(out, ref, inp, lean=True):
    """tests/test_qp_gpu.py: test_qp0_matches_oracle, test_collision_qp_matches_oracle (iterate for iterate)"""
    io = ref["io"]
    assert out["info"]["status_val"] == io["status_val"] == 1 and out["info"]["iter"] == io["iter"], (out["info"], io["iter"])
    assert out["info"]["working_rows"] == inp["W"].size > 0
    np.testing.assert_allclose(out["x"], ref["x"], rtol=0, atol=1e-8)
    np.testing.assert_allclose(out["yc"], ref["y"]["col"], rtol=0, atol=1e-7)
    yf = np.hstack([ref["y"][k].ravel() for k in ("jerk", "acc", "vel", "pos")])
    np.testing.assert_allclose(out["yf"], yf, rtol=0, atol=1e-7)  # (tests/test_qp_gpu.py: 1e-8 at eps 1e-8, 1e-7 for duals at 1e-3)
    np.testing.assert_allclose(out["w_l"], inp["l"][inp["W"]], rtol=0, atol=1e-12)
    if lean:
        i0 = ref["i0"]
        assert out["info0"]["status_val"] == i0["status_val"] == 1 and out["info0"]["iter"] == i0["iter"]
        np.testing.assert_allclose(out["x_qp0"], ref["x_qp0"], rtol=0, atol=1e-9)
        assert out["info"]["pipeline"].startswith("persistent") and out["info"]["persist_gave_up"] == 0, out["info"]
    else:
        assert out["info"]["pipeline"] == "generic", out["info"]
        np.testing.assert_array_equal(out["x_clone"], out["x"])


def _qp_generic_run(ctx, inp):
    """three PCG steps per ADMM step: the generic pipeline, rows given (scp_qp_add_rows); boxes as wide as the arena; then the
    state handed to a larger workspace (scp_qp_clone_state)"""
    import torch

    prob = inp["prob"]
    qp = _make_qp(ctx, prob, cg_iters=3, use_mfma=2, max_iter=10000)
    big = _make_qp(ctx, prob, row_capacity=2 * qp.row_capacity, cg_iters=3, use_mfma=2, max_iter=10000)
    try:
        shape = (prob.N, prob.K, prob.D)
        qp.set_position_boxes(ctx.tensor(np.broadcast_to(prob.pos_min, shape)), ctx.tensor(np.broadcast_to(prob.pos_max, shape)))
        qp.reset(ctx.tensor(inp["x0"]))
        W = inp["W"]
        qp.add_rows(torch.as_tensor(W, dtype=torch.int64, device=ctx.tdev), ctx.tensor(inp["eta"][W]), ctx.tensor(inp["l"][W]))
        qp.set_rho(RHO_GENERIC)  # another rho than the settings': the KKT blocks are built again, on the context's stream
        out = {"info": _info(qp.solve())}
        yf, yc = qp.duals()
        out.update(x=_np(qp.solution()), yf=_np(yf), yc=_np(yc), w_l=_np(qp.peek("w_l")))
        big.take_state_of(qp)
        out["x_clone"] = _np(big.solution())
    finally:
        big.close()
        qp.close()
    return out


RHO_GENERIC = 0.3


def _qp_generic_reference(inp):
    st = qo.Settings(cg_iters=3, max_iter=10000, max_rounds=1, rho=RHO_GENERIC)
    x, y, io = qo.admm_structured(inp["prob"], inp["eta"], inp["l"], inp["dist"], x0=inp["x0"], st=st, rows0=inp["W"])
    return dict(x=x, y=y, io=io)


def _qp_generic_from_ref(ref, inp):
    out = _qp_from_ref(ref, inp, cg=3, use_mfma=2)
    out["x_clone"] = ref["x"]
    return out


QP_LEAN_ENTRIES = ("scp_qp_create", "scp_qp_set_problem", "scp_qp_reset", "scp_qp_add_rows_at", "scp_qp_solve", "scp_qp_get_solution",
                   "scp_qp_get_duals", "scp_qp_peek")
QP_GENERIC_ENTRIES = ("scp_qp_create", "scp_qp_set_problem", "scp_qp_set_position_boxes", "scp_qp_reset", "scp_qp_add_rows", "scp_qp_set_rho", "scp_qp_solve",
                      "scp_qp_get_solution", "scp_qp_get_duals", "scp_qp_clone_state", "scp_qp_peek")


def _grow_qp():
    def run(ctx, inp):
        return {"lean": _qp_lean_run(ctx, inp)["info"]["iter"], "generic": _qp_generic_run(ctx, inp)["info"]["iter"]}

    return Case("grow_qp", "qp", (), lambda: _qp_inputs(24, 5), run)


# ---- family "solver": the natively driven loop, the step and the step split at its exchange points ---------------------------------------
SOLVER_SHAPE = dict(n=4, T=10.0, h=0.5, R=0.8, space=[0, 0, 20, 20], seed=1, cg_iters=2)
SOLVER_GROW = dict(n=10, T=10.0, h=0.2, R=0.8, space=[0, 0, 20, 20], seed=7, cg_iters=1)


def _solver_inputs(shape=None):
    from path_planning.scenarios.position_generator import generate_positions

    s = dict(shape or SOLVER_SHAPE)
    s["p0"], s["pf"] = generate_positions(s["n"], s["R"], seed=s["seed"])
    s["prob"] = so.make_problem(s["n"], s["T"], s["h"], s["R"], s["space"], s["p0"], s["pf"])
    return s


@contextlib.contextmanager
def _scp_on(ctx, s):
    """an SCP object that works on the caller's context (SCP(ctx=...)): on exit its device objects are destroyed, `ctx` stays
    open"""
    from path_planning.solvers.scp import SCP

    scp = SCP(n_vehicles=s["n"], time_horizon=s["T"], time_step=s["h"], min_distance=s["R"], space_dims=s["space"], verbose=False,
              qp_settings={"cg_iters": s["cg_iters"]}, ctx=ctx)
    scp.set_initial_states(s["p0"])
    scp.set_final_states(s["pf"])
    try:
        yield scp
    finally:
        scp.close()
        assert getattr(ctx, "h", None), "SCP.close() closed a context it had borrowed"


def _solve_run(ctx, inp, max_iterations=15):
    with _scp_on(ctx, inp) as scp:
        traj = scp.generate_trajectories(max_iterations=max_iterations)
        return {"positions": np.array(traj["positions"]), "velocities": np.array(traj["velocities"]),
                "accelerations": np.array(traj["accelerations"]), "n_iterations": int(scp.last_info["n_iterations"])}


def _solve_reference(inp):
    return qo.scp_solve(inp["prob"], 15, qo.Settings(max_iter=10000, cg_iters=inp["cg_iters"]))


def _solve_from_ref(ref, inp):
    return {"positions": ref["positions"], "velocities": ref["velocities"], "accelerations": ref["accelerations"],
            "n_iterations": int(ref["iterations"])}


def _solve_compare(out, ref, inp):
    """__graft_entry__.smoke(): two PCG steps per ADMM step follow the oracle iterate for iterate"""
    assert out["n_iterations"] == ref["iterations"] >= 1
    for k in ("positions", "velocities", "accelerations"):
        assert float(np.abs(out[k] - ref[k]).max()) < 1e-7, k


def _step_run(ctx, inp):
    with _scp_on(ctx, inp) as scp:
        scp._precompute_constraint_matrices()
        acc0 = scp._solve_initial_trajectory()
        new, info = scp.scp_iteration(acc0)
        import torch

        # a rows buffer of one id: every longer list of the sharded step is fetched again (scp_solver_shard_rows)
        scp._ensure_native()._shard_rows = torch.empty(1, dtype=torch.int64, device=ctx.tdev)
        sharded, info_s = scp.scp_iteration_sharded(acc0)
        keys = ("status_val", "iter", "rho_updates", "working_rows", "rounds")
        return {"acc0": _np(acc0), "acc": _np(new), "acc_sharded": _np(sharded), "info": {k: info[k] for k in keys},
                "info_sharded": {k: info_s[k] for k in keys}, "rel_step": float(info["rel_step"]), "rel_step_sharded": float(info_s["rel_step"])}


def _step_reference(inp):
    st = qo.Settings(max_iter=10000, cg_iters=inp["cg_iters"])
    x0, _, _ = qo.admm_structured(inp["prob"], st=qo.Settings(max_iter=4000, cg_iters=inp["cg_iters"]))
    one = qo.scp_solve(inp["prob"], 1, st, force_iterations=1)
    return dict(acc0=x0, acc=one["accelerations"], rel=one["rel_steps"][0], info=one["infos"][1])


def _step_from_ref(ref, inp):
    i = ref["info"]
    info = dict(status_val=i["status_val"], iter=i["iter"], rho_updates=i["rho_updates"], working_rows=i["working_rows"], rounds=i["rounds"])
    return {"acc0": ref["acc0"], "acc": ref["acc"], "acc_sharded": ref["acc"], "info": info, "info_sharded": dict(info),
            "rel_step": ref["rel"], "rel_step_sharded": ref["rel"]}


def _step_compare(out, ref, inp):
    """tests/test_shard_world_gpu.py: the sharded step is the one-rank step bit for bit; smoke()'s 1e-7 against the oracle"""
    np.testing.assert_array_equal(out["acc_sharded"].view(np.int64), out["acc"].view(np.int64))
    assert out["info_sharded"] == out["info"] and np.float64(out["rel_step"]).tobytes() == np.float64(out["rel_step_sharded"]).tobytes()
    assert float(np.abs(out["acc0"] - ref["acc0"]).max()) < 1e-7 and float(np.abs(out["acc"] - ref["acc"]).max()) < 1e-7
    assert out["info"]["status_val"] == ref["info"]["status_val"] == 1 and out["info"]["iter"] == ref["info"]["iter"]
    assert abs(out["rel_step"] - ref["rel"]) <= 1e-6 * ref["rel"]


SOLVE_ENTRIES = ("scp_solver_create", "scp_solver_solve")
STEP_ENTRIES = ("scp_solver_create", "scp_solver_step", "scp_solver_shard_begin", "scp_solver_shard_rows", "scp_solver_shard_qp",
                "scp_solver_shard_violations", "scp_solver_shard_round_done", "scp_solver_shard_end")


def _grow_solver():
    return Case("grow_solver", "solver", (), lambda: _solver_inputs(SOLVER_GROW),
                lambda ctx, inp: {"n": _solve_run(ctx, inp, max_iterations=2)["n_iterations"]})


# ---- the table -------------------------------------------------------------------------------------------------------------------------
def _build():
    s = CT_SHAPE
    N, K, D, S = s["N"], s["K"], s["D"], s["S"]
    path_c, weighted_c, shorten_c = "rand2d_13x11_s2_c1", "rand2d_13x11_s2", "rand2d_13x11_s1_c0"
    cases = [_pair_case(n) for n in PAIR_SHAPES]
    cases.append(Case("trajectory", "trajectory", TRAJ_ENTRIES, _traj_inputs, _traj_run, _traj_reference, lambda ref, inp: dict(ref), _traj_compare))
    cases += [
        _ct("check_separation", ("scp_check_separation", "scp_ctx_last_separation_solved", "scp_check_avoidance"), _sep_run, _sep_reference,
            _sep_from_ref, _sep_compare, lambda inp: ws_check_separation(N, K, D)),
        _ct("list_conflicts", ("scp_list_conflicts",), _conf_run, _conf_reference, lambda ref, inp: {"list": _conflict_records(ref)},
            _conf_compare, lambda inp: ws_list_conflicts(N, K, D, CONF_CAP)),
        _ct("clearance_profile", ("scp_clearance_profile", "scp_ctx_last_clearance_solved"), _clr_run, _clr_reference, _clr_from_ref,
            _clr_compare, lambda inp: ws_clearance(N, K, D)),
        _ct("delay_margins", ("scp_delay_margins", "scp_ctx_last_delay_solved"), _dly_run, _dly_reference, _dly_from_ref, _dly_compare,
            lambda inp: ws_delay(N, K, D, S)),
        _ct("lag_conflicts", ("scp_lag_conflicts", "scp_ctx_last_lag_solved", "scp_schedule_starts"), _lag_run, _lag_reference, _lag_from_ref,
            _lag_compare, lambda inp: ws_lag(N, K, D)),
        _ct("schedule_starts_batch", ("scp_schedule_starts_batch",), _batch_run, _batch_reference, _batch_from_ref, _batch_compare,
            lambda inp: ws_batch(BATCH_SHAPE[0], BATCH_SHAPE[4]), inputs=_batch_inputs),
        _ct("update_holds", ("scp_update_holds",), _upd_run, _upd_reference, lambda ref, inp: {"table": ref, "needed": int(ref.size)},
            _upd_compare, lambda inp: ws_update_holds(inp["conflicts"].size, inp["start"].size), inputs=_upd_inputs),
        _ct("apply_holds", ("scp_apply_holds", "scp_linearize_pairs"), _apply_run, _apply_reference, _apply_from_ref, _apply_compare,
            lambda inp: merge_ws(ws_apply_holds(inp["table"].size), ws_pairwise(APPLY_SHAPE["N"], APPLY_SHAPE["K"], APPLY_SHAPE["D"], linearize_only=True)),
            inputs=_apply_inputs),
    ]
    cases += [
        _raster_case("rasterize", "65x3_mixed_m0.4"),
        Case("reference_paths", "obstacle", PATH_ENTRIES, lambda: dict(c=_by_name(rpc, path_c)), _paths_run, _paths_reference, _paths_from_ref,
             _paths_compare, lambda inp: ws_paths(inp["c"].N, inp["c"].max_path)),
        Case("reference_paths_weighted", "obstacle", WEIGHTED_ENTRIES + PATH_ENTRIES[:2], lambda: dict(c=_by_name(wpc, weighted_c)),
             _weighted_run, _weighted_reference, _weighted_from_ref, _weighted_compare,
             lambda inp: merge_ws(ws_paths(inp["c"].N, inp["c"].max_path), ws_distance(inp["c"].occ))),
        Case("shorten_paths", "obstacle", ("scp_shorten_paths",) + PATH_ENTRIES[:3], lambda: dict(c=_by_name(stc, shorten_c)), _shorten_run,
             lambda inp: stc.want(inp["c"]), _shorten_from_ref, _shorten_compare, lambda inp: ws_paths(inp["c"].N, inp["c"].max_path)),
        _field_case("field_2d", "40x33_density_0.02"),
        _field_case("field_3d", "33x9x5"),
        _field_case("field_row", "70x1"),  # one row: no envelope pass, no workspace
        Case("obstacle_clearance", "obstacle", ("scp_obstacle_clearance", "scp_obstacle_distance", "scp_occupancy_prepare"),
             lambda: dict(p={p.name: p for p in odc.all_plans()}["2d_n3_k65_p16"]), _oclr_run, lambda inp: inp["p"].want(), _oclr_from_ref,
             _oclr_compare, lambda inp: ws_distance(inp["p"].occ)),
        Case("corridor", "obstacle", ("scp_occupancy_prepare", "scp_corridor_boxes", "scp_corridor_state_boxes", "scp_check_corridor"),
             _corridor_inputs, _corridor_run, _corridor_reference, _corridor_from_ref, _corridor_compare),
    ]
    cases += [
        Case("assign_goals", "assign", ("scp_assign_goals", "scp_straight_line_check"), _assign_inputs, _assign_run, _assign_reference,
             _assign_from_ref, _assign_compare, lambda inp: ws_line_check(1, inp["start"].shape[0])),
        Case("assign_goals_wide", "assign", ("scp_assign_goals_wide",), _assign_inputs, lambda ctx, inp: _assign_run(ctx, inp, wide=True),
             _assign_reference, lambda ref, inp: _assign_from_ref(ref, inp, wide=True),
             lambda out, ref, inp: _assign_compare(out, ref, inp, wide=True), lambda inp: ws_assign_wide(1, inp["start"].shape[0])),
        Case("assign_costs", "assign", ("scp_assign_costs",), lambda: dict(c=apr.gpu_matrices()[COSTS_NAME]), _costs_run,
             lambda inp: dict(ref=apr.reference(COSTS_NAME)), lambda ref, inp: _assign_from_ref(ref, inp, wide=True),
             lambda out, ref, inp: _assign_compare(out, ref, inp, wide=True)),
        Case("generate_grid_swap", "assign", ("scp_generate_grid_swap",), lambda: dict(shape=GEN_SHAPE), _gen_run, _gen_reference,
             _gen_from_ref, _gen_compare, lambda inp: ws_generator(len(GEN_SHAPE[2]), GEN_SHAPE[0])),
    ]
    cases += [
        Case("qp_lean", "qp", QP_LEAN_ENTRIES, _qp_inputs, _qp_lean_run, _qp_lean_reference, _qp_from_ref, _qp_compare),
        Case("qp_generic", "qp", QP_GENERIC_ENTRIES, _qp_inputs, _qp_generic_run, _qp_generic_reference, _qp_generic_from_ref,
             lambda out, ref, inp: _qp_compare(out, ref, inp, lean=False)),
        Case("solver_solve", "solver", SOLVE_ENTRIES, _solver_inputs, _solve_run, _solve_reference, _solve_from_ref, _solve_compare),
        Case("solver_step", "solver", STEP_ENTRIES, _solver_inputs, _step_run, _step_reference, _step_from_ref, _step_compare),
    ]
    return cases


CASES = _build()
CASES_BY_NAME = {c.name: c for c in CASES}
assert len(CASES_BY_NAME) == len(CASES)
FAMILIES = ("pairwise", "trajectory", "continuous", "obstacle", "assign", "qp", "solver")
GROWERS = {"pairwise": _grow_pairwise(), "continuous": _grow_continuous(), "obstacle": _grow_obstacle(), "assign": _grow_assign(),
           "qp": _grow_qp(), "solver": _grow_solver(),
           "trajectory": Case("grow_trajectory", "trajectory", (), lambda: _traj_inputs("ref_n20_k50", 70001, (199, 50, 130)), _traj_run)}

# the twelve users of sep_ws: the case that runs each
SEP_WS_USERS = {"scp_check_separation": "check_separation", "scp_list_conflicts": "list_conflicts", "scp_clearance_profile": "clearance_profile",
                "scp_delay_margins": "delay_margins", "scp_lag_conflicts": "lag_conflicts", "scp_schedule_starts_batch": "schedule_starts_batch",
                "scp_update_holds": "update_holds", "scp_apply_holds": "apply_holds", "scp_reference_paths": "reference_paths",
                "scp_reference_paths_weighted": "reference_paths_weighted", "scp_shorten_paths": "shorten_paths",
                "scp_obstacle_distance": "field_3d"}
# SCP's order on one context: the map, the distance field, the weighted search, the shortening, the solve's checks, the margins,
# the schedules, the holds
PRODUCT_ORDER = ("reference_paths", "field_3d", "reference_paths_weighted", "shorten_paths", "check_separation", "list_conflicts",
                 "clearance_profile", "delay_margins", "lag_conflicts", "schedule_starts_batch", "update_holds", "apply_holds")

# Entry points that need no case, each with its reason: lifecycle, option setters, getters of host-side fields, the two hooks
EXEMPT = {
    "scp_ctx_destroy": "lifecycle", "scp_last_error": "getter of a host-side field (the message)",
    "scp_ctx_synchronize": "lifecycle: drains the stream, launches nothing",
    "scp_ctx_last_pair_ms": "getter of a host-side field (two events of the context)",
    "scp_ctx_set_option": "option setter", "scp_ctx_set_near_pass": "option setter",
    "scp_ctx_near_pass_counts": "getter of host-side fields (two counters)",
    "scp_ctx_debug_fill": "one of the two hooks these tests are built on", "scp_ctx_debug_state": "the other hook",
    "scp_qp_destroy": "lifecycle", "scp_qp_update_settings": "option setter",
    "scp_qp_debug_set": "option setter (test switches, host-side fields)",
    "scp_solver_destroy": "lifecycle", "scp_solver_update_settings": "option setter",
    "scp_solver_set_position_boxes": "option setter: keeps two pointers (host-side fields), the solver applies them with scp_qp_set_position_boxes",
}
