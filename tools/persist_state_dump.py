"""The state the lean persistent ADMM kernels leave after 12 steps -- x, zf, yf, zc, yc as scp_qp_peek returns them, and the
solve's info -- on three small cases of tests/persist_cases.py, one per instantiation of cg1_persist16_kernel, to compare
two builds of the library bit for bit (the oracle tests allow 1e-11; a change that must not move a bit is checked here).

    SCP_HIP_LIB=<parent build>/libscp_hip.so python tools/persist_state_dump.py --dump parent.npz
    python tools/persist_state_dump.py --same-as parent.npz        # exit status 1 and the differing arrays if any differs
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "ba-path-planning_amd")):
    sys.path.insert(0, p)
import persist_cases as pc  # noqa: E402

STEPS = 12
PEEK = ("x", "zf", "yf", "zc", "yc")
INFO = ("status_val", "iter", "rho_updates", "cg_iters_total", "working_rows", "r_prim", "r_dual", "rho", "persist_launches",
        "persist_gave_up", "rho_switches_in_kernel")
# (scenario, settings.persistent): <2, 16>, <2, 8>, <3, 8>
CASES = [(pc.RHO_2D, 2), (pc.RHO_2D, 3), (pc.Scenario("near", 3501, 9, 50, 3, 0.2), 3)]


def outputs(ctx):
    import torch
    from path_planning import _hip

    out = {}
    for sc, kernel in CASES:
        prob, x0, eta, l_col, dist, W = pc.setup(sc)
        qp = _hip.QP(ctx, prob.N, prob.K, prob.D, prob.h, _hip.default_settings(**pc.gpu_step_settings(kernel, STEPS)))
        try:
            qp.set_problem(pc.LIMITS, np.concatenate([prob.pos_min, prob.pos_max]), ctx.tensor(prob.p0), ctx.tensor(prob.v0),
                           ctx.tensor(prob.pf), ctx.tensor(prob.vf))
            qp.reset(ctx.tensor(x0))
            qp.add_rows(torch.as_tensor(W, dtype=torch.int64, device=ctx.tdev), ctx.tensor(eta[W]), ctx.tensor(l_col[W]))
            info = qp.solve()
            key = f"{pc.kernel_name(kernel, sc.dim)} {sc.label} "
            assert info["pipeline"] == pc.PIPELINE[kernel] and info["iter"] == STEPS, (key, info)
            for name in PEEK:
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
