"""Inputs shared by tests/test_shorten_cpu.py and tests/test_shorten_gpu.py: every case of tests/reference_path_cases.py plus
one open map, and what tests/shorten_ref.py makes of them (computed once per case, never changed)."""
import numpy as np

import reference_path_cases as rc
import shorten_ref as sr


def open_map():
    """an open 40 x 30 map at stride 1, starts and goals in opposite corners: one long clear test each, no obstacles, so every
    path becomes p0 -> pf"""
    occ = np.zeros((1, 30, 40), dtype=np.uint8)
    p0 = [[0.3, 0.6], [39.5, 0.5], [0.5, 29.2], [39.7, 29.9]]
    pf = [[39.6, 29.4], [0.2, 29.5], [39.5, 0.5], [0.5, 0.1]]
    return rc.Case("open_40x30", 2, occ, [0.0, 0.0], 1.0, 1, 0, 25, p0, pf)


_CASES = None
_WANT = {}


def all_cases():
    """reference_path_cases.all_cases() and the open map, built once per process"""
    global _CASES
    if _CASES is None:
        _CASES = list(rc.all_cases()) + [open_map()]
        assert len({c.name for c in _CASES}) == len(_CASES)
    return _CASES


def want(c):
    """{"ref", "kept", "out", "W"} of the restatement for a case, from the search's expected path and records"""
    if c.name not in _WANT:
        w = c.want()
        ref, kept, out, W = sr.shorten_paths(c.D, c.origin, c.cell, w["sat"], c.stride, c.clearance, c.p0, c.pf, c.K, w["path"],
                                             w["info"], w["ref"])
        for v in (ref, kept, out):
            v.setflags(write=False)
        _WANT[c.name] = {"ref": ref, "kept": kept, "out": out, "W": W}
    return _WANT[c.name]
