"""scp_qp_reset's two one-launch kernels from identical inputs: the 16-column kernel (qp_reset_kernel, "reset_form" 0 of
scp_qp_debug_set) and the tiled kernel that spreads the same dot products over a (column tile) x (row slab) grid
("reset_form" 1, the default).  Both form every output as one accumulator over k = 0 .. K-1 with the same expression, so the
arrays they leave -- x (time-major), z_f, the carried F x and S0 x, y_f -- agree bit for bit: compared as int64 views, no
tolerance.  Shapes: fewer columns than a tile, exactly the 16 columns of the old workgroup, tail tiles, odd K, D = 3 (tiles
that cut an agent), several tiles and row slabs, and K = SCP_FUSED_MAX_K, where the tile no longer fits the LDS budget and
the reset falls back to the 16-column kernel."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

LIMITS = [-2.0, 2.0, -15.0, 15.0, -20.0, 20.0]
NAMES = ("x", "zf", "fx", "yf", "qx")
SHAPES = [(1, 2, 2), (3, 5, 3), (8, 50, 2), (9, 33, 2), (40, 64, 3), (130, 50, 2), (4, 120, 2)]


@pytest.fixture(scope="module")
def ctx():
    from path_planning import _hip

    c = _hip.Context(0)
    yield c
    c.close()


def reset_state(ctx, form, N, K, D, x0):
    from path_planning import _hip

    rng = np.random.default_rng(7)
    p0, pf = rng.uniform(1.0, 19.0, (2, N, D))
    zeros = np.zeros((N, D))
    qp = _hip.QP(ctx, N, K, D, 0.2, _hip.default_settings(), row_capacity=16)
    assert qp.debug_set("reset_form", form) == form
    qp.set_problem(LIMITS, [0.0] * D + [20.0] * D, ctx.tensor(p0), ctx.tensor(zeros), ctx.tensor(pf), ctx.tensor(zeros))
    qp.reset(None if x0 is None else ctx.tensor(x0))
    out = {n: qp.peek(n).cpu().numpy().copy() for n in NAMES}
    qp.close()
    return out


@pytest.mark.parametrize("warm", [False, True], ids=["zeros", "x0"])
@pytest.mark.parametrize("N,K,D", SHAPES)
def test_reset_forms_agree_bit_for_bit(ctx, N, K, D, warm):
    x0 = None
    if warm:  # seeded, with exact zeros and negative entries
        rng = np.random.default_rng(1000 * N + 10 * K + D)
        x0 = 3.0 * rng.standard_normal((N, K, D))
        x0[rng.random((N, K, D)) < 0.2] = 0.0
        x0[0, 0, 0], x0[-1, -1, -1] = 0.0, -1.25
        assert (x0 == 0.0).any() and (x0 < 0.0).any()
    a = reset_state(ctx, 0, N, K, D, x0)
    b = reset_state(ctx, 1, N, K, D, x0)
    C, Rf = N * D, 4 * K - 1
    for name in NAMES:
        assert a[name].shape == b[name].shape == ((Rf if name in ("zf", "fx", "yf") else K) * C,), name
        np.testing.assert_array_equal(a[name].view(np.int64), b[name].view(np.int64), err_msg=name)
    # what does not depend on the dot products: x is x0 in the QP's layout, y_f is zero, z_f is the carried F x
    want_x = np.zeros((K, C)) if x0 is None else x0.transpose(1, 0, 2).reshape(K, C)
    np.testing.assert_array_equal(b["x"].view(np.int64), want_x.ravel().view(np.int64))
    assert not b["yf"].view(np.int64).any()
    np.testing.assert_array_equal(b["zf"].view(np.int64), b["fx"].view(np.int64))
    if warm:
        assert np.abs(b["zf"]).max() > 0.0 and np.abs(b["qx"]).max() > 0.0
