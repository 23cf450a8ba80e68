"""Host-side plots of a solved SCP instance (headless-safe; MPLBACKEND=Agg works).

Thin counterparts of SCP.visualize_trajectories / visualize_time_snapshots of the reference
(/root/reference/src/path_planning/solvers/scp.py:644-840): same call signatures on the solver, drawn from
the numpy copies in ``solver.trajectories``.  Plot styling is this repo's own; no numeric output."""
import numpy as np


def _axes_limits(solver):
    lo, hi = np.asarray(solver.pos_min, float), np.asarray(solver.pos_max, float)
    pos = solver.trajectories["positions"]
    lo = np.minimum(lo[:2], pos[..., :2].min(axis=(0, 1))) if np.all(np.isfinite(pos)) else lo[:2]
    hi = np.maximum(hi[:2], pos[..., :2].max(axis=(0, 1))) if np.all(np.isfinite(pos)) else hi[:2]
    return lo, hi


def plot_trajectories(solver, show=False, save_path="trajectories.pdf"):
    import matplotlib.pyplot as plt
    from matplotlib.patches import Circle

    pos = solver.trajectories["positions"]
    fig, ax = plt.subplots(figsize=(8, 8))
    cmap = plt.get_cmap("tab20")
    for i in range(solver.N):
        c = cmap(i % 20)
        ax.plot(pos[i, :, 0], pos[i, :, 1], "-", color=c, lw=1.2)
        ax.plot(pos[i, 0, 0], pos[i, 0, 1], "o", color=c, ms=5)
        ax.plot(pos[i, -1, 0], pos[i, -1, 1], "s", color=c, ms=5)
        ax.add_patch(Circle(pos[i, -1, :2], solver.R / 2, fill=False, color=c, lw=0.6))
    lo, hi = _axes_limits(solver)
    ax.set_xlim(lo[0], hi[0])
    ax.set_ylim(lo[1], hi[1])
    ax.set_aspect("equal")
    ax.set_xlabel("x [m]")
    ax.set_ylabel("y [m]")
    ax.set_title(f"SCP trajectories: N={solver.N}, K={solver.K}, R={solver.R}")
    if save_path:
        fig.savefig(save_path, bbox_inches="tight")
    if show:
        plt.show()
    return fig, ax


def plot_time_snapshots(solver, num_snapshots=5, save_path=None):
    import matplotlib.pyplot as plt
    from matplotlib.patches import Circle

    pos = solver.trajectories["positions"]
    ks = np.linspace(0, solver.K - 1, num_snapshots).astype(int)
    fig, axes = plt.subplots(1, num_snapshots, figsize=(4 * num_snapshots, 4), squeeze=False)
    cmap = plt.get_cmap("tab20")
    lo, hi = _axes_limits(solver)
    for ax, k in zip(axes[0], ks):
        for i in range(solver.N):
            c = cmap(i % 20)
            ax.plot(pos[i, : k + 1, 0], pos[i, : k + 1, 1], "-", color=c, lw=0.8, alpha=0.6)
            ax.add_patch(Circle(pos[i, k, :2], solver.R / 2, color=c, alpha=0.8))
        ax.set_xlim(lo[0], hi[0])
        ax.set_ylim(lo[1], hi[1])
        ax.set_aspect("equal")
        ax.set_title(f"t = {k * solver.h:.1f} s")
    if save_path:
        fig.savefig(save_path, bbox_inches="tight")
    return fig, axes


def plot_clearance(solver, save_path="clearance.pdf"):
    """The clearance profiles of validate_solution(continuous=True, clearance=True): left, the fleet's minimum distance over
    the horizon, at the samples and over the whole segments, against R and the tolerated R - 0.01; right, the vehicles'
    clearances in ascending order."""
    import matplotlib.pyplot as plt

    rep = solver.validate_solution(continuous=True, clearance=True)
    sc, vc = rep["step_clearance"], rep["vehicle_clearance"]
    t = solver.h * np.arange(solver.K)
    fig, (ax, bx) = plt.subplots(1, 2, figsize=(13, 4.5))
    ax.step(t, sc["sample_min_distance"], where="post", color="tab:gray", lw=1.0, label="at the samples")
    ax.step(t, sc["min_distance"], where="post", color="tab:blue", lw=1.4, label="over the segments")
    order = np.argsort(vc["min_distance"], kind="stable")
    bx.plot(np.arange(solver.N), vc["sample_min_distance"][order], ".", color="tab:gray", ms=3, label="at the samples")
    bx.plot(np.arange(solver.N), vc["min_distance"][order], "-", color="tab:blue", lw=1.4, label="over the segments")
    for a in (ax, bx):
        a.axhline(solver.R, color="tab:green", lw=0.8, ls="--", label=f"R = {solver.R} m")
        a.axhline(solver.R - 0.01, color="tab:red", lw=0.8, ls=":", label="R - 0.01 m")
        a.set_ylabel("minimum distance [m]")
        a.legend(fontsize=8)
    ax.set_xlabel("t [s]")
    ax.set_title("fleet clearance per time step")
    bx.set_xlabel("vehicles, by clearance")
    n_conf = int((vc["n_violating_segments"] > 0).sum())
    bx.set_title(f"clearance per vehicle ({n_conf} of {solver.N} in conflict)")
    if save_path:
        fig.savefig(save_path, bbox_inches="tight")
    plt.close(fig)
    return rep


def plot_delay_margin(solver, max_lag, save_path="delay.pdf"):
    """The delay margins of validate_solution(continuous=True, delay=max_lag): one curve per vehicle, its smallest distance to
    anybody over the delay of its start (that vehicle alone, in seconds), against the tolerated R - 0.01; the least tolerant
    vehicle is drawn on top."""
    import matplotlib.pyplot as plt

    rep = solver.validate_solution(continuous=True, delay=max_lag)
    dist = rep["delay_margin"]["min_distance"]
    lag = solver.h * np.arange(dist.shape[1])
    fig, ax = plt.subplots(figsize=(7.5, 4.5))
    for v in range(solver.N):
        ax.plot(lag, dist[v], "-", color="tab:blue", lw=0.7, alpha=0.5, marker=".", ms=3)
    lt = rep["least_tolerant_vehicle"]
    if lt is not None:
        ax.plot(lag, dist[lt["vehicle"]], "-", color="tab:orange", lw=1.6, marker=".", ms=4,
                label=f"vehicle {lt['vehicle']}: {lt['steps']} steps")
    ax.axhline(solver.R - 0.01, color="tab:red", lw=0.8, ls=":", label="R - 0.01 m")
    ax.set_xlabel("delay of the vehicle's start [s]")
    ax.set_ylabel("minimum distance to anybody [m]")
    ax.set_title(f"delay margin per vehicle ({solver.N} vehicles, up to {max_lag} steps)")
    ax.legend(fontsize=8)
    if save_path:
        fig.savefig(save_path, bbox_inches="tight")
    plt.close(fig)
    return rep
