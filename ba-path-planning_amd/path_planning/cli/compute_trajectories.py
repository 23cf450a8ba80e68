"""``compute-trajectories``: one demo solve + plots (entry point of the reference,
/root/reference/src/path_planning/cli/compute_trajectories.py:9-99, pyproject.toml:53).

Called without arguments it reproduces the reference demo (N=10, T=100 s, h=0.2 s -> K=500, R=0.8 m, space
200 x 200 m, generator scenario, max_iterations=15, two plots).  The optional flags expose what the
reference hard-codes (its SURVEY "next" item f-1): problem size, scenario family and seed, plot files."""
import argparse
import time

import numpy as np

from ..scenarios.grid_swap_device import generate_grid_swap_device
from ..scenarios.position_generator import generate_grid_swap, generate_positions
from ..solvers.scp import SCP


def add_stagger_search_arguments(p):
    """the four flags of the order search of --stagger-starts (shared with compute-trajectories-batch)"""
    p.add_argument("--stagger-search", type=int, default=None, metavar="B",
                   help="with --stagger-starts: schedule B candidate launch orders per round in one GPU launch (the given order, "
                        "its reverse, random ones) and keep the best; never worse than the schedule by vehicle index")
    p.add_argument("--stagger-rounds", type=int, default=None, metavar="R",
                   help="with --stagger-search: R rounds (default 1); every round after the first derives its candidates from "
                        "the best order so far")
    p.add_argument("--stagger-seed", type=int, default=None, help="with --stagger-search: seed of the random orders (default 0)")
    p.add_argument("--stagger-objective", choices=("makespan", "total"), default=None,
                   help="with --stagger-search: after the fewest unplaced vehicles, prefer the smallest largest delay (makespan, "
                        "default) or the smallest sum of delays (total)")


def stagger_search_keywords(parser, args):
    """the keywords of SCP.stagger_starts the four flags ask for; the flags are errors without --stagger-starts"""
    given = {"search": args.stagger_search, "rounds": args.stagger_rounds, "seed": args.stagger_seed,
             "objective": args.stagger_objective}
    given = {k: v for k, v in given.items() if v is not None}
    if given and args.stagger_starts is None:
        parser.error("--stagger-" + next(iter(given)) + " needs --stagger-starts")
    return given


def build_parser():
    p = argparse.ArgumentParser(prog="compute-trajectories", description=__doc__.split("\n\n")[0])
    p.add_argument("--n-agents", type=int, default=10)
    p.add_argument("--time-horizon", type=float, default=100.0)
    p.add_argument("--time-step", type=float, default=0.2)
    p.add_argument("--min-distance", type=float, default=0.8)
    p.add_argument("--space", type=float, nargs="+", default=None, help="[min..., max...]; default 0 0 200 200")
    p.add_argument("--scenario", choices=["reference", "grid-swap", "grid-swap-device"], default="reference")
    p.add_argument("--dim", type=int, choices=[2, 3], default=2)
    p.add_argument("--seed", type=int, default=None)
    p.add_argument("--max-iterations", type=int, default=15)
    p.add_argument("--polish", action="store_true",
                   help="one more joint QP at 1e-8 after the SCP loop: the result meets every constraint to ~1e-6")
    p.add_argument("--cg-iters", type=int, default=None,
                   help="PCG steps per ADMM step of the joint QP (scp_qp_settings.cg_iters; default 1)")
    p.add_argument("--continuous-check", action="store_true",
                   help="after the solve, print the minimum distance over the whole flight (between the samples too), "
                        "the vehicles and the time of that closest approach")
    p.add_argument("--list-conflicts", action="store_true",
                   help="--continuous-check, and one more line per between-sample conflict: the two vehicles, when they are "
                        "closer than the minimum distance - 0.01 m, and how close they come")
    p.add_argument("--clearance", action="store_true",
                   help="--continuous-check, and one more line: the most exposed vehicle (smallest distance to any other over "
                        "the whole flight) and how many vehicles are in a conflict; with --save-prefix also <prefix>_clearance.pdf")
    p.add_argument("--delay-tolerance", type=int, default=None, metavar="STEPS",
                   help="--continuous-check, and one more line: the vehicle that tolerates the smallest late start (alone, in "
                        "whole time steps up to STEPS) before it comes closer than the minimum distance - 0.01 m to anybody, "
                        "who limits it and where; with --save-prefix also <prefix>_delay.pdf")
    p.add_argument("--stagger-starts", type=int, default=None, metavar="STEPS",
                   help="after the solve, look for late starts of at most STEPS whole time steps that remove the between-sample "
                        "conflicts without changing a plan (pair-lag conflict masks and a greedy schedule by vehicle index) and "
                        "print the summary and the delayed vehicles; the checks and plots still show the plans as solved")
    add_stagger_search_arguments(p)
    p.add_argument("--repair-conflicts", type=int, nargs="?", const=6, default=None, metavar="PASSES",
                   help="after the solve, remove the between-sample conflicts with holds (fixed separating half-planes on the "
                        "two rows around every conflicting segment, at most PASSES passes, default 6) and print the report; "
                        "the checks and plots then show the repaired trajectories")
    p.add_argument("--assign-goals", action="store_true",
                   help="interchangeable vehicles: before the solve, pair vehicles and goals so that the sum of squared "
                        "start-goal distances is minimal (no head-on swaps), and print one line with cost, straight-line "
                        "minimum approach and opposed pairs before and after")
    p.add_argument("--assign-method", choices=("auto", "single", "wide"), default="auto",
                   help="--assign-goals through the one-workgroup auction (single, up to 4096 vehicles), the whole-GPU one (wide, "
                        "up to 65536) or whichever fits (auto); the assignment is the same")
    p.add_argument("--assign-cost", choices=("line", "path", "length"), default="line",
                   help="with --assign-goals: pair by squared straight-line distance (line), or by the length of the paths "
                        "the lattice search finds around the obstacles (path: needs --obstacle-discs, takes --corridor-stride "
                        "and --corridor-clearance; up to 4096 vehicles) -- the line then shows the lattice moves before and "
                        "after; length: as path, by the weighted length of those paths (a diagonal move costs more than a "
                        "straight one) and, with --corridor-keep-clear, their clearance")
    p.add_argument("--obstacle-discs", nargs="+", default=None, metavar="X,Y[,Z],R",
                   help="static obstacles: discs (spheres in 3-D) given as centre and radius; before the solve, safe flight "
                        "corridors around the straight lines from start to goal become per-step position boxes of the QP, and "
                        "after it one line says whether every segment stays inside its box")
    p.add_argument("--obstacle-boxes", nargs="+", default=None, metavar="MIN...,MAX...",
                   help="static obstacles: axis-aligned boxes given as their lower and upper corner (4 numbers, 6 in 3-D).  With "
                        "this flag, --obstacle-capsules or --obstacle-polygons all obstacles, --obstacle-discs included, are "
                        "rasterised on the GPU, and one line says what was rasterised; every flag that needs --obstacle-discs is "
                        "content with any of the four")
    p.add_argument("--obstacle-capsules", nargs="+", default=None, metavar="X0,Y0[,Z0],X1,Y1[,Z1],R",
                   help="static obstacles: capsules, a segment with a radius (an oblique wall, a beam, a pipe)")
    p.add_argument("--obstacle-polygons", nargs="+", default=None, metavar="X,Y,X,Y,...[:Z0,Z1]",
                   help="static obstacles: polygons given by their vertices in the xy plane (at least 3, closed by an implied "
                        "edge, any winding direction, convex or not); in 3-D the prism over the heights Z0 .. Z1")
    p.add_argument("--corridor-cell", type=float, default=None, metavar="METRES",
                   help="with --obstacle-discs: edge length of the occupancy grid's cells (default: a quarter of the minimum "
                        "distance)")
    p.add_argument("--corridor-grow", type=int, default=None, metavar="CELLS",
                   help="with --obstacle-discs: how many cells a corridor box may grow beyond its segment per direction "
                        "(default 8)")
    p.add_argument("--corridor-search", action="store_true",
                   help="with --obstacle-discs: the corridors follow paths found around the obstacles (a breadth-first search on "
                        "a lattice of blocks of cells, one GPU workgroup per vehicle) instead of the straight lines, and one "
                        "line says what was found")
    p.add_argument("--corridor-stride", type=int, default=None, metavar="CELLS",
                   help="with --corridor-search: edge length of a lattice block in cells (default: the smallest that keeps the "
                        "lattice within 32768 nodes and a path across the map within the number of time steps)")
    p.add_argument("--corridor-clearance", type=int, default=None, metavar="CELLS",
                   help="with --corridor-search: free cells required around every lattice block on a path (default 0; with "
                        "--corridor-shorten the stride)")
    p.add_argument("--corridor-metric", choices=("hops", "length"), default=None,
                   help="with --corridor-search: the search counts lattice moves (hops, the default) or weighs them by length, "
                        "a diagonal move 99 / 70 of a straight one (length: run to its fixed point, one GPU workgroup per vehicle)")
    p.add_argument("--corridor-keep-clear", type=int, default=None, metavar="CELLS",
                   help="with --corridor-metric length or --assign-cost length: the clearance from the obstacles, in cells, "
                        "below which a lattice node costs extra (default 0: length only)")
    p.add_argument("--corridor-clear-weight", type=float, default=None, metavar="W",
                   help="with --corridor-keep-clear: how many straight moves one missing cell of clearance costs per node passed "
                        "(default 1)")
    p.add_argument("--corridor-share", type=float, default=None, metavar="W",
                   help="with --corridor-search and --corridor-metric length: the paths avoid each other's routes -- a lattice "
                        "node that more vehicles' paths use than --corridor-share-capacity costs every further vehicle W straight "
                        "moves per vehicle over capacity, the fleet re-routes in groups and the least crowded set of paths is "
                        "kept (negotiated on the GPU, no host read between the rounds); the line then shows the overuse before "
                        "and after")
    p.add_argument("--corridor-share-capacity", type=int, default=None, metavar="C",
                   help="with --corridor-share: the paths one lattice node carries for free (default 1)")
    p.add_argument("--corridor-share-groups", type=int, default=None, metavar="G",
                   help="with --corridor-share: the fleet re-routes in G groups, one per round (default 4)")
    p.add_argument("--corridor-share-rounds", type=int, default=None, metavar="R",
                   help="with --corridor-share: rounds of re-routing, 0 .. 64 (default: twice the groups)")
    p.add_argument("--corridor-shorten", action="store_true",
                   help="with --corridor-search: every path is cut down to the lattice nodes it cannot skip and its reference "
                        "points are spaced evenly by length (one GPU wave per vehicle)")
    p.add_argument("--obstacle-clearance", type=int, nargs="?", const=4, default=None, metavar="PIECES",
                   help="with --obstacle-discs: after the solve (and --repair-conflicts) the plan is judged against the map "
                        "itself, not against its corridor boxes: every segment is cut into PIECES pieces (1 .. 16, default 4) "
                        "and one line gives the fleet's guaranteed clearance from the occupied cells, the vehicle, segment and "
                        "time where it is attained, and how many pieces touch an occupied cell, leave the map or are too "
                        "wide to judge")
    p.add_argument("--no-plots", action="store_true")
    p.add_argument("--save-prefix", default=None, help="write <prefix>_2d.pdf and <prefix>_snapshots.pdf")
    return p


def obstacle_discs(parser, args):
    """the discs of --obstacle-discs as tuples of floats; the corridor flags are errors without it, --corridor-stride and
    --corridor-clearance without --corridor-search or --assign-cost path / length, --corridor-shorten and --corridor-metric
    without --corridor-search, --corridor-keep-clear without one of the two length searches, --corridor-clear-weight without
    --corridor-keep-clear, --corridor-share without both --corridor-search and --corridor-metric length, the other three
    --corridor-share-* flags without --corridor-share"""
    by_path = args.assign_cost in ("path", "length")
    if by_path and not args.assign_goals:
        parser.error("--assign-cost needs --assign-goals")
    if args.corridor_metric is not None and not args.corridor_search:
        parser.error("--corridor-metric needs --corridor-search")
    if args.corridor_keep_clear is not None and args.corridor_metric != "length" and args.assign_cost != "length":
        parser.error("--corridor-keep-clear needs --corridor-metric length or --assign-cost length")
    if args.corridor_keep_clear is not None and args.corridor_keep_clear < 0:
        parser.error(f"--corridor-keep-clear {args.corridor_keep_clear}: a whole number of cells >= 0")
    if args.corridor_clear_weight is not None and args.corridor_keep_clear is None:
        parser.error("--corridor-clear-weight needs --corridor-keep-clear")
    if args.corridor_share is not None and not (args.corridor_search and args.corridor_metric == "length"):
        parser.error("--corridor-share needs --corridor-search and --corridor-metric length")
    for flag in ("capacity", "groups", "rounds"):
        if getattr(args, "corridor_share_" + flag) is not None and args.corridor_share is None:
            parser.error(f"--corridor-share-{flag} needs --corridor-share")
    if not args.corridor_search:
        for flag, value in (("--corridor-stride", None if by_path else args.corridor_stride),
                            ("--corridor-clearance", None if by_path else args.corridor_clearance),
                            ("--corridor-shorten", args.corridor_shorten or None)):
            if value is not None:
                parser.error(f"{flag} needs --corridor-search")
    shaped = any(getattr(args, "obstacle_" + kind, None) is not None for kind in ("boxes", "capsules", "polygons"))
    if args.obstacle_discs is None and not shaped:
        if by_path:
            parser.error(f"--assign-cost {args.assign_cost} needs --obstacle-discs")
        for flag, value in (("--corridor-cell", args.corridor_cell), ("--corridor-grow", args.corridor_grow),
                            ("--corridor-search", args.corridor_search or None), ("--obstacle-clearance", args.obstacle_clearance)):
            if value is not None:
                parser.error(f"{flag} needs --obstacle-discs")
        return None
    if args.obstacle_clearance is not None and not 1 <= args.obstacle_clearance <= 16:
        parser.error(f"--obstacle-clearance {args.obstacle_clearance}: 1 .. 16 pieces per segment")
    if args.obstacle_discs is None:
        return None
    discs = []
    for text in args.obstacle_discs:
        try:
            disc = tuple(float(v) for v in text.split(","))
        except ValueError:
            disc = ()
        if len(disc) != args.dim + 1:
            parser.error(f"--obstacle-discs {text}: {args.dim} centre coordinates and a radius, separated by commas")
        discs.append(disc)
    return discs


def obstacle_shapes(parser, args):
    """the shapes of --obstacle-boxes / --obstacle-capsules / --obstacle-polygons as the keywords of SCP.set_obstacle_shapes,
    or None when none of the three is given (then --obstacle-discs alone goes the host's way, as before)"""
    if args.obstacle_boxes is None and args.obstacle_capsules is None and args.obstacle_polygons is None:
        return None
    D = args.dim

    def numbers(text):
        try:
            return [float(v) for v in text.split(",")]
        except ValueError:
            return None

    out = {"boxes": [], "capsules": [], "polygons": []}
    for text in args.obstacle_boxes or ():
        v = numbers(text)
        if v is None or len(v) != 2 * D:
            parser.error(f"--obstacle-boxes {text}: {D} lower and {D} upper coordinates, separated by commas")
        out["boxes"].append(tuple(v))
    for text in args.obstacle_capsules or ():
        v = numbers(text)
        if v is None or len(v) != 2 * D + 1:
            parser.error(f"--obstacle-capsules {text}: two points of {D} coordinates and a radius, separated by commas")
        out["capsules"].append(tuple(v))
    for text in args.obstacle_polygons or ():
        flat, _, heights = text.partition(":")
        v, z = numbers(flat), numbers(heights) if heights else []
        if v is None or len(v) < 6 or len(v) % 2 or z is None or len(z) != (2 if D == 3 else 0):
            parser.error(f"--obstacle-polygons {text}: X,Y pairs of at least 3 vertices" + (", then :Z0,Z1" if D == 3 else
                                                                                           " (a height range needs --dim 3)"))
        out["polygons"].append((np.asarray(v).reshape(-1, 2),) + tuple(z))
    return out


def obstacle_shapes_summary(oi):
    """the line of the device rasteriser from SCP.obstacle_info"""
    counts = ", ".join(f"{n} {kind}" for kind, n in oi["counts"].items() if n)
    return (f"Obstacles: {oi['n_shapes']} shapes ({counts}) rasterised on the GPU with margin {oi['margin']:g} m: "
            f"{oi['n_occupied']} of {oi['n_cells']} cells occupied ({oi['rasterize_ms']:.3f} ms, summed table "
            f"{oi['prepare_ms']:.3f} ms)")


def shortened_summary(fr):
    """the part of the search's line that --corridor-shorten adds: kept vertices and the two lengths"""
    found = fr["status"] == 0
    return (f"; shortened to {int(fr['n_kept'][found].sum())} of {int(fr['n_nodes'][found].sum())} nodes, total length "
            f"{float(fr['length'][found].sum()):.2f} m (lattice paths {float(fr['length_before'][found].sum()):.2f} m), "
            f"{fr['shorten_ms']:.3f} ms")


def shared_summary(fr):
    """the part of the search's line that --corridor-share adds: the overuse before and after, and the round that was kept"""
    sh = fr.get("sharing")
    if sh is None:
        return ""
    return f", overuse {sh['overuse'][0]} -> {sh['overuse'][sh['best_round']]} (round {sh['best_round']} of {sh['rounds']})"


def obstacle_clearance_summary(oc, time_step):
    """the line of --obstacle-clearance from what SCP.obstacle_clearance returns"""
    v = oc["worst_vehicle"]
    ve = oc["vehicles"]
    if np.isfinite(oc["clearance"]):
        g = int(ve["segment"][v])
        where = (f"at least {oc['clearance']:.4f} m from the occupied cells (vehicle {v}, segment {g}, t = {g * time_step:.2f} .. "
                 f"{(g + 1) * time_step:.2f} s)")
    else:
        where = "no piece judged against an occupied cell"
    return (f"Obstacle clearance: {where}; {oc['n_touch']} pieces touch an occupied cell, {oc['n_off']} off the map, "
            f"{oc['n_wide']} too wide to judge; " + ("clear" if oc["clear"] else "NOT clear")
            + f" (field {oc['field_ms']:.3f} ms, pass {oc['check_ms']:.3f} ms)")


def main(argv=None):
    """Create collision-free trajectories for a set of initial and final positions."""
    parser = build_parser()
    args = parser.parse_args([] if argv is None else argv)
    stagger_search = stagger_search_keywords(parser, args)
    discs = obstacle_discs(parser, args)
    shapes = obstacle_shapes(parser, args)
    print("------ WOW Fleet Collision-Free 2D Trajectory Generation ------")

    n_vehicles = args.n_agents
    time_horizon = args.time_horizon
    time_step = args.time_step
    min_distance = args.min_distance
    if args.scenario in ("grid-swap", "grid-swap-device"):
        gen = generate_grid_swap if args.scenario == "grid-swap" else generate_grid_swap_device
        initial_positions, final_positions, space_dims = gen(n_vehicles, seed=args.seed or 0, dim=args.dim)
        if args.space is not None:
            space_dims = args.space
    else:
        space_dims = args.space if args.space is not None else [0, 0, 200, 200]
        initial_positions, final_positions = generate_positions(n_vehicles, min_distance, seed=args.seed)

    print("Configuration:")
    print(f"  Number of vehicles: {n_vehicles}")
    print(f"  Time horizon: {time_horizon} s")
    print(f"  Time step: {time_step} s")
    print(f"  Minimum margin: {min_distance} m")
    print(f"  Space dimensions: {space_dims} m")
    print()

    try:
        solver = SCP(
            n_vehicles=n_vehicles,
            time_horizon=time_horizon,
            time_step=time_step,
            min_distance=min_distance,
            space_dims=space_dims,
            dim=args.dim,
            polish=args.polish,
            qp_settings={"cg_iters": args.cg_iters} if args.cg_iters else None,
        )
        print(f"Successfully generated positions for {n_vehicles} vehicles")
        solver.set_initial_states(np.asarray(initial_positions))
        solver.set_final_states(np.asarray(final_positions))
        if args.assign_goals and args.assign_cost == "line":
            from ..scenarios.assignment import describe

            solver.assign_goals(method=args.assign_method)
            print(describe(solver.assignment_info))

        if shapes is not None:  # (the device rasteriser takes every kind, the discs too)
            cell = args.corridor_cell or min_distance / 4
            oi = solver.set_obstacle_shapes(cell, discs=discs or (), **shapes)
            n_obstacles, grid_dims = oi["n_shapes"], tuple(oi["dims"]) + (1,) * (3 - args.dim)
            print(obstacle_shapes_summary(oi))
        elif discs is not None:
            from ..scenarios.obstacles import rasterize

            occ, origin, cell = rasterize(space_dims, args.corridor_cell or min_distance / 4, discs=discs, margin=min_distance / 2)
            solver.set_obstacles(occ, origin, cell)
            n_obstacles, grid_dims = len(discs), occ.shape[::-1]
        if discs is not None or shapes is not None:
            if args.corridor_metric == "length" or args.assign_cost == "length":
                solver.set_search_metric("length", keep_clear=args.corridor_keep_clear or 0,
                                         clear_weight=1.0 if args.corridor_clear_weight is None else args.corridor_clear_weight)
            if args.assign_goals and args.assign_cost != "line":  # (the pairing sees the map: after it, before the search)
                from ..scenarios.assignment import describe

                solver.assign_goals(cost=args.assign_cost, stride=args.corridor_stride, clearance=args.corridor_clearance or 0)
                if args.corridor_metric != "length":  # (--assign-cost length alone: the corridors' search still counts moves)
                    solver.set_search_metric("hops")
                print(describe(solver.assignment_info))
            reference = None
            if args.corridor_share is not None:
                solver.set_path_sharing(share=args.corridor_share,
                                        capacity=1 if args.corridor_share_capacity is None else args.corridor_share_capacity,
                                        groups=4 if args.corridor_share_groups is None else args.corridor_share_groups,
                                        rounds=args.corridor_share_rounds)
            if args.corridor_search:
                if args.corridor_shorten:
                    reference, fr = solver.shorten_reference(stride=args.corridor_stride, clearance=args.corridor_clearance)
                else:
                    reference, fr = solver.find_reference(stride=args.corridor_stride, clearance=args.corridor_clearance or 0)
                print(f"Corridor search: lattice of {' x '.join(str(n) for n in fr['lattice'])} blocks of {fr['stride']} cells "
                      f"(clearance {fr['clearance']}), {n_vehicles - fr['n_failed']} of {n_vehicles} paths found, longest "
                      f"E = {fr['max_edges']} for K = {solver.K}" + ("" if fr["guaranteed"] else " (no blocked segment is not "
                      "guaranteed)") + (f", by length (keep clear {fr['keep_clear']} cells): total cost {int(fr['cost'][fr['status'] == 0].sum())}"
                                       if fr["metric"] == "length" else "") + shared_summary(fr)
                      + f", {fr['edges_ms'] + fr['penalties_ms'] + fr['search_ms']:.3f} ms" + (shortened_summary(fr) if args.corridor_shorten else ""))
            co = solver.set_corridors(reference=reference, max_grow=8 if args.corridor_grow is None else args.corridor_grow)

        print("Generating trajectories...")
        start_time = time.time()
        solver.generate_trajectories(max_iterations=args.max_iterations)
        end_time = time.time()

        print("\nTrajectory generation complete!")
        print(f"Total computation time: {end_time - start_time:.3f} seconds")
        print(f"Number of time steps: {solver.K}")
        print(f"Total trajectory duration: {solver.T} seconds")
        if discs is not None or shapes is not None:
            cr = solver.validate_corridor()
            print(f"Corridors: {n_obstacles} obstacles on a grid of {grid_dims[0]} x {grid_dims[1]} x {grid_dims[2]} cells of "
                  f"{cell:g} m, boxes shrunk by {co['shrink']:.4f} m; " + ("every segment stays inside its box" if cr["inside"] else
                  f"{cr['n_outside']} segments leave their box") + f" (largest excess {cr['max_excess']:.4f} m, vehicle "
                  f"{cr['worst_vehicle']})")
        if args.repair_conflicts is not None:
            rep = solver.repair_conflicts(max_passes=args.repair_conflicts)
            counts = " -> ".join(str(n) for n in [rep["conflicts_before"]] + rep["conflicts_per_pass"])
            print(f"Conflict repair: {counts} conflicting segments in {rep['passes']} passes ({rep['holds']} holds, stopped by "
                  f"{rep['stopped_by']}), cost ratio {rep['cost_ratio']:.4f}, {rep['time_sec']:.3f} s"
                  + ("" if rep["repaired"] else "; NOT repaired"))
        if args.obstacle_clearance is not None:
            print(obstacle_clearance_summary(solver.obstacle_clearance(pieces=args.obstacle_clearance), time_step))
        if args.stagger_starts is not None:
            st = solver.stagger_starts(args.stagger_starts, **stagger_search)
            print(f"Staggered starts: {st['n_delayed']} of {n_vehicles} vehicles delayed by up to {st['max_delay']} steps "
                  f"({st['max_delay'] * time_step:.2f} s; {st['total_delay']} steps in all), conflicting segments "
                  f"{st['conflicts_before']} -> {st['conflicts_after']}, minimum distance {st['min_distance_after']:.4f} m over "
                  f"{st['horizon_steps']} steps, {st['time_sec']:.3f} s"
                  + ("" if st["scheduled"] else f"; {st['n_unplaced']} vehicles found NO delay"))
            if "search" in st:
                se = st["search"]
                print(f"  order search ({se['objective']}): {se['candidates']} candidates x {se['rounds_run']} rounds, best is "
                      f"candidate {se['best_candidate']} of round {se['best_round']}; by vehicle index: "
                      f"{se['baseline']['n_unplaced']} unplaced, largest delay {se['baseline']['max_delay']}, "
                      f"{se['baseline']['total_delay']} steps in all" + ("" if se["improved"] else " (not improved)"))
            for v in np.nonzero(st["delays"] > 0)[0]:
                print(f"  vehicle {v}: starts {st['delays'][v]} steps ({st['delays'][v] * time_step:.2f} s) late")
        if args.continuous_check or args.list_conflicts or args.clearance or args.delay_tolerance is not None:
            extras = {k: True for k, on in (("conflicts", args.list_conflicts), ("clearance", args.clearance)) if on}
            if args.delay_tolerance is not None:
                extras["delay"] = args.delay_tolerance
            rep = solver.validate_solution(continuous=True, **extras)
            ca = rep["closest_approach"]
            if ca is None:
                print("Continuous-time check: no pair of vehicles")
            else:
                print(f"Continuous-time check: minimum distance {ca['distance']:.4f} m between vehicles {ca['vehicles'][0]} and "
                      f"{ca['vehicles'][1]} at t = {ca['time']:.4f} s (at the samples: {rep['min_pair_distance']:.4f} m; "
                      f"{rep['n_violating_segments']} segments below {min_distance - 0.01:.2f} m)")
            for w in rep.get("conflicts", ()):
                print(f"  conflict: vehicles {w['vehicles'][0]} and {w['vehicles'][1]} from t = {w['t_start']:.4f} s to "
                      f"t = {w['t_end']:.4f} s, minimum distance {w['min_distance']:.4f} m at t = {w['t_min_distance']:.4f} s"
                      + (" (hull of separate stretches)" if w["pieces"] > 1 else ""))
            me = rep.get("most_exposed_vehicle")
            if me is not None:
                n_conf = int((rep["vehicle_clearance"]["n_violating_segments"] > 0).sum())
                print(f"Clearance: most exposed vehicle {me['vehicle']} comes within {me['distance']:.4f} m of vehicle "
                      f"{me['partner']} at t = {me['time']:.4f} s; {n_conf} of {n_vehicles} vehicles in conflict")
            if args.clearance and args.save_prefix:
                from ..viz.plot_trajectories import plot_clearance

                plot_clearance(solver, f"{args.save_prefix}_clearance.pdf")
            if args.delay_tolerance is not None:
                lt = rep["least_tolerant_vehicle"]
                if lt is None:
                    print("Delay tolerance: no pair of vehicles")
                elif lt["steps"] >= args.delay_tolerance:
                    print(f"Delay tolerance: every vehicle may start {lt['steps']} steps ({lt['seconds']:.2f} s) late; least "
                          f"tolerant vehicle {lt['vehicle']} then still keeps {lt['distance']:.4f} m from vehicle "
                          f"{lt['partner']} at t = {lt['time']:.4f} s")
                else:
                    late = (f"may start {lt['steps']} steps ({lt['seconds']:.2f} s) late" if lt["steps"] >= 0
                            else "is in conflict on schedule")
                    print(f"Delay tolerance: least tolerant vehicle {lt['vehicle']} {late}; one step more and it comes within "
                          f"{lt['distance']:.4f} m of vehicle {lt['partner']} at t = {lt['time']:.4f} s")
                if args.save_prefix:
                    from ..viz.plot_trajectories import plot_delay_margin

                    plot_delay_margin(solver, args.delay_tolerance, f"{args.save_prefix}_delay.pdf")

        if not args.no_plots:
            pre = args.save_prefix
            print("\nVisualizing 2D trajectories...")
            solver.visualize_trajectories(show_animation=pre is None,
                                          save_path=f"{pre}_2d.pdf" if pre else "trajectories.pdf")
            print("\nVisualizing time snapshots")
            solver.visualize_time_snapshots(num_snapshots=5, save_path=f"{pre}_snapshots.pdf" if pre else None)
        return solver
    except Exception as e:  # the reference swallows and prints every error (compute_trajectories.py:98-99)
        print(f"Error during trajectory generation: {e}")
        return None


def console_main():
    import sys

    main(sys.argv[1:])


if __name__ == "__main__":
    console_main()
