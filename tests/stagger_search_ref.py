"""Reference of the order search of the staggered starts (scp_schedule_starts_batch), written from the rule in include/scp_hip.h
(not from the kernel): every candidate order is scheduled by stagger_ref.greedy in Python integers, and the best candidate is
the lexicographic minimum of the rule's key.

  key(stats, objective, b)         "makespan": (n_unplaced, max_delay, total_delay, b); "total": (n_unplaced, total_delay,
                                   max_delay, b);
  best_of(stats_list, objective)   the candidate with the smallest key (ties: the lowest index, by the trailing b);
  schedule_all(mask, S, orders)    (delays, stats) of every candidate, as two lists."""
import stagger_ref as st

OBJECTIVES = ("makespan", "total")
FIELDS = ("n_delayed", "n_unplaced", "max_delay", "first_unplaced", "total_delay")


def key(stats, objective, b):
    u, m, t = int(stats["n_unplaced"]), int(stats["max_delay"]), int(stats["total_delay"])
    if objective == "makespan":
        return (u, m, t, b)
    if objective == "total":
        return (u, t, m, b)
    raise ValueError(objective)


def best_of(stats_list, objective):
    return min(range(len(stats_list)), key=lambda b: key(stats_list[b], objective, b))


def schedule_all(mask, S, orders):
    out = [st.greedy(mask, S, order) for order in orders]
    return [d for d, _ in out], [s for _, s in out]
