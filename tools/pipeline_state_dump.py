"""The state the ADMM pipelines beyond the persistent kernels leave after a few steps -- x, zf, yf, zc, yc (and the carried
F x, S0 x where the pipeline carries them) as scp_qp_peek returns them, and the solve's info -- on the smallest cases that
reach every instantiation of the column kernels of csrc/scp_qp_columns.hip and the update kernels of the generic pipeline,
to compare two builds of the library bit for bit (the oracle tests allow 1e-11; a change that must not move a bit is
checked here).  The interface is that of tools/persist_state_dump.py:

    SCP_HIP_LIB=<parent build>/libscp_hip.so python tools/pipeline_state_dump.py --dump parent.npz
    python tools/pipeline_state_dump.py --same-as parent.npz        # exit status 1 and the differing arrays if any differs

Every solve runs fixed rho with check_termination = 6 and eps = 1e-12, so max_iter = 12 holds one check that does not end
the solve, and with it the exact refresh of F x / S0 x, and a second one at the end.

  three-launch, K <= 64    cg1_col_kernel<1>, cg1_resid_col_kernel<1>, cg1_update_kernel<2 | 3> (row term summed inline):
                           persist_cases.RHO_2D and the 3-D scenario of tools/persist_state_dump.py, settings.persistent = 0
  three-launch, K > 64     the <2> instantiations: a group-A case of tests/pipeline_cases.py with a partial last column
                           block and K mod 16 != 0, and the group-A case with the most working rows (LARGEST_A: more
                           than SQ_INLINE_MAX = 2048 of them, so cg1_rows_sq_kernel runs)
  qp0                      qp0_col_kernel<1> / <2>: a group-D case each side of K = 64 from a random start, after 5, 7
                           and 12 steps (5 and 7 split a launch just short of and just past a check)
  generic                  admm_fixed_update_kernel, admm_row_update_kernel<2>: a group-C case with two PCG steps

F x and S0 x ("fx", "qx") are part of the state on the three-launch pipeline only (tests/test_pipeline_iterates_gpu.py says
why); elsewhere the two names hold scratch and are left out.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "ba-path-planning_amd")):
    sys.path.insert(0, p)
import persist_cases as pc  # noqa: E402
import pipeline_cases as qc  # noqa: E402

STEPS = 12
PEEK = ("x", "zf", "yf", "zc", "yc")
CARRIED = ("fx", "qx")
INFO = ("status_val", "iter", "rho_updates", "cg_iters_total", "working_rows", "r_prim", "r_dual", "rho", "persist_launches",
        "persist_gave_up", "rho_switches_in_kernel")
LARGEST_A = (17, 120, 2)  # N, K, dim


def _pick(cases, N, K, dim, **want):
    """the one case of a table with that shape and those fields (an error if the table no longer has exactly one)"""
    found = [c for c in cases
             if (c.scen.N, c.scen.K, c.scen.dim) == (N, K, dim) and all(getattr(c, k) == v for k, v in want.items())]
    assert len(found) == 1, (N, K, dim, want, [c.id for c in found])
    return found[0]


def _three_launch(sc):
    """a scenario of the persistent tables on the three-launch pipeline (settings.persistent = 0)"""
    C = sc.N * sc.dim
    return qc.Case("A", sc, qc.expected_pipeline(sc.K, C, True), C % 16, sc.K % 16, qc.band(sc.K), "K <= 64 on three launches")


def cases():
    """(case of tests/pipeline_cases.py, the max_iter values to run it with)"""
    out = [(_three_launch(sc), (STEPS,)) for sc in (pc.RHO_2D, pc.Scenario("near", 3501, 9, 50, 3, 0.2))]
    out.append((_pick(qc.CASES_A, 9, 65, 2, persistent=0), (STEPS,)))
    out.append((_pick(qc.CASES_A, *LARGEST_A, persistent=0), (STEPS,)))
    for K in (50, 65):
        out.append((_pick(qc.CASES_D, 9, K, 2, start="random"), (5, 7, STEPS)))
    out.append((_pick(qc.CASES_C, 9, 50, 2, cg_iters=2, use_mfma=1), (STEPS,)))
    for c, _ in out:
        assert c.pipeline == ("qp0" if c.group == "D" else "generic" if c.group == "C" else "three-launch"), c
    return out


def outputs(ctx):
    import torch
    from path_planning import _hip

    out = {}
    for case, iters in cases():
        prob, x0, eta, l_col, dist, W = qc.problem(case)
        qp = _hip.QP(ctx, prob.N, prob.K, prob.D, prob.h, _hip.default_settings(**case.gpu_settings(1)))
        try:
            qp.set_problem(pc.LIMITS, np.concatenate([prob.pos_min, prob.pos_max]), ctx.tensor(prob.p0), ctx.tensor(prob.v0),
                           ctx.tensor(prob.pf), ctx.tensor(prob.vf))
            for m in iters:
                qp.update_settings(max_iter=m)
                qp.reset(None if x0 is None else ctx.tensor(x0))
                if W.size:
                    qp.add_rows(torch.as_tensor(W, dtype=torch.int64, device=ctx.tdev), ctx.tensor(eta[W]), ctx.tensor(l_col[W]))
                info = qp.solve()
                key = f"{case.pipeline} {case.id} rows={W.size} m={m} "
                assert info["pipeline"] == case.pipeline and info["iter"] == m, (key, info)
                for name in PEEK + (CARRIED if case.carries else ()):
                    out[key + name] = qp.peek(name).cpu().numpy()
                out[key + "info"] = np.array([float(info[k]) for k in INFO])
        finally:
            qp.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    g = ap.add_mutually_exclusive_group(required=True)
    g.add_argument("--dump", metavar="FILE")
    g.add_argument("--same-as", metavar="FILE")
    args = ap.parse_args()
    from path_planning import _hip

    ctx = _hip.Context(0)
    out = outputs(ctx)
    ctx.close()
    lib = _hip.load_library()._name
    if args.dump:
        np.savez(args.dump, **out)
        print(f"{lib}: {len(out)} arrays, {sum(v.size for v in out.values())} values -> {args.dump}")
        return 0
    ref = np.load(args.same_as)
    bad = [k for k in sorted(set(out) | set(ref.files))
           if k not in out or k not in ref.files or out[k].shape != ref[k].shape or out[k].tobytes() != ref[k].tobytes()]
    print(f"{lib}: {len(out)} arrays against {args.same_as}: {len(bad)} differ" + "".join(f"\n  differs: {k}" for k in bad))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
