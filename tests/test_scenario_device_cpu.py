"""grid-swap-device scenarios without a GPU: the C-ABI surface, the CLI choice, no CPU fallback, and the promises of the
numpy restatement (tests/scenario_device_ref.py) that the GPU tests compare the kernels against bit for bit."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import scenario_device_ref as R  # noqa: E402


def test_library_exports_generator():
    from path_planning import _hip

    lib = ctypes.CDLL(_hip.library_path())
    for name in ("scp_generate_grid_swap", "scp_gen_default_params"):
        assert hasattr(lib, name) and name in _hip.EXPORTS, name
    p = _hip.gen_params()
    assert (p.pitch, p.jitter, p.block, p.layer_gap, p.min_sep, p.max_tries, p.sweeps) == (2.0, 0.2, 4, 2.0, 0.3, 8192, 20)
    with pytest.raises(TypeError):
        _hip.gen_params(bogus=1)


def test_generator_structs_match_the_header(tmp_path):
    from path_planning import _hip

    fields = {"scp_gen_params": (_hip.GenParams, ["pitch", "jitter", "layer_gap", "min_sep", "block", "max_tries", "sweeps"]),
              "scp_gen_stats": (_hip.GenStats, ["sweeps", "unmet_blocks", "conflicts", "min_approach", "ok"])}
    src = ['#include <stddef.h>', '#include <stdio.h>', '#include "scp_hip.h"', "int main(void) {"]
    for name, (_, fs) in fields.items():
        src.append(f'  printf("{name} %zu", sizeof({name}));')
        for f in fs:
            src.append(f'  printf(" %zu", offsetof({name}, {f}));')
        src.append('  printf("\\n");')
    src.append("  return 0; }")
    c = tmp_path / "gen_layout.c"
    c.write_text("\n".join(src))
    exe = tmp_path / "gen_layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split("\n")
    got = {ln.split()[0]: [int(v) for v in ln.split()[1:]] for ln in out if ln.strip()}
    for name, (cls, fs) in fields.items():
        assert got[name] == [ctypes.sizeof(cls)] + [getattr(cls, f).offset for f in fs], name
    st = got["scp_gen_stats"]
    assert _hip.GEN_STATS_DTYPE.itemsize == st[0]
    assert [_hip.GEN_STATS_DTYPE.fields[f][1] for f in fields["scp_gen_stats"][1]] == st[1:]


def test_cli_parsers_accept_grid_swap_device():
    from path_planning.cli import compute_trajectories, compute_trajectories_batch

    assert compute_trajectories.build_parser().parse_args(["--scenario", "grid-swap-device"]).scenario == "grid-swap-device"
    a = compute_trajectories_batch.build_parser().parse_args(["--scenario", "grid-swap-device", "--Ns", "64"])
    assert a.scenario == "grid-swap-device"


def test_no_cpu_fallback():
    import torch

    if torch.cuda.is_available():
        pytest.skip("a GPU is visible")
    from path_planning import _hip
    from path_planning.scenarios import generate_grid_swap_batch, generate_grid_swap_device

    with pytest.raises(_hip.HipError):
        generate_grid_swap_device(128, seed=1)
    with pytest.raises(_hip.HipError):
        generate_grid_swap_batch(128, [1, 2])


@pytest.mark.parametrize("N,dim", [(16, 2), (100, 2), (128, 2), (1000, 2), (64, 3), (128, 3)])
def test_restatement_promises(N, dim):
    from path_planning.scenarios.position_generator import straight_line_min_distance

    p = R.DEFAULTS
    init, goal, space, st = R.generate(N, 7, dim)
    assert init.shape == goal.shape == (N, dim) and space.shape == (2 * dim,)
    layers, per, side, blocks = R.layout(N, dim, p["block"])
    assert sorted(np.concatenate([idx for _, _, idx in blocks]).tolist()) == list(range(N))
    for L, _, idx in blocks:
        assert len(idx) <= p["block"] ** 2
        # goal cells of a block = its start cells, permuted (jitter < pitch / 2: rounding recovers the cell)
        sc = np.rint(init[idx, :2] / p["pitch"]).astype(int)
        gc = np.rint(goal[idx, :2] / p["pitch"]).astype(int)
        assert sorted(map(tuple, sc)) == sorted(map(tuple, gc))
        assert (idx // per == L).all()
    disp = np.linalg.norm(goal[:, :2] - init[:, :2], axis=1)
    assert disp.max() <= (p["block"] - 1) * p["pitch"] * np.sqrt(2) + 2 * p["jitter"] * np.sqrt(2)
    if dim == 3:
        assert np.array_equal(init[:, 2], goal[:, 2])
        assert np.array_equal(init[:, 2], (np.arange(N) // per) * p["layer_gap"])
    assert st["min_approach"] == straight_line_min_distance(init, goal).min()
    assert st["ok"] == (st["min_approach"] >= p["min_sep"])
    assert st["conflicts"] >= 0 and 0 <= st["sweeps"] <= p["sweeps"]
    lo = np.minimum(init.min(0), goal.min(0)) - 2.0
    assert np.array_equal(space, np.concatenate([lo, np.maximum(init.max(0), goal.max(0)) + 2.0]))


def test_restatement_layout_searches():
    for N in range(1, 3000, 37):
        layers, per, side, _ = R.layout(N, 3, 4)
        assert layers ** 3 >= N > (layers - 1) ** 3 and side * side >= per > (side - 1) ** 2
        import math

        assert layers == max(1, math.ceil(round(N ** (1.0 / 3.0), 9)))
