"""The LDS carve-up of the lean persistent kernels (Lds16 in csrc/scp_qp_persist16.hip) after <2, 8> took on S0 p = T r:
its packed T and an S0 p tile join the fixed part, and every kernel's entry tables shrink to D + 6 doubles per incident row
(signed eta, l, z, y, g, the row value at x, the row value of p).  The restatement is checked against the library's own
size functions, and every lean case of tests/persist_cases.py must still fit."""
import ctypes

import pytest

import persist_cases as pc
from path_planning import _hip

NCHK = 9
AB_STRIDE = 32
BUDGET = 160 * 1024 - 2048  # all the LDS there is, minus the kernel's static __shared__ (scp_qp_cg1_persist)


def nct(D, per):
    return (D * per + 15) // 16


def t_on_mfma(D, per):
    """<2, 8> only: four of its eight waves are idle in the MFMA phase and form T r"""
    return 4 * nct(D, per) < per and per <= 8


def lean_lds_bytes(K, cap, nblk, D, per):
    """Lds16 + the int tables (entry codes, cell offsets), as scp_persist16_lds_bytes computes them"""
    nc16 = 16 * nct(D, per)
    rsk, tk, nks = pc._pad_col(K), (K + 15) >> 4, (K + 3) >> 2
    dbl = 2 * nc16 * rsk + tk * nks * 64  # r, p tiles; packed H_f^{-1}
    if t_on_mfma(D, per):
        dbl += nc16 * rsk + tk * nks * 64  # S0 p tile; packed T
    dbl += 2 * nblk + per * AB_STRIDE
    if 2 * nc16 * rsk < NCHK * nblk:
        dbl += NCHK * nblk
    dbl += cap * (D + 6)
    ints = cap + per * K + 1
    return dbl * 8 + (ints + 1) // 2 * 2 * 4


def entry_bytes(D):
    return (D + 6) * 8 + 4


def lean_entry_cap(kernel, N, K, D):
    """entry capacity of a lean persistent launch: the formula of scp_qp_cg1_persist (csrc/scp_qp_persist.hip)"""
    per = pc.apb(kernel, D)
    nb = (N + per - 1) // per + 1
    return (BUDGET - lean_lds_bytes(K, 0, nb, D, per)) // entry_bytes(D) // 64 * 64


SHAPES = [(2, 8), (2, 16), (3, 8)]
KS = [3, 16, 17, 50, 64]


@pytest.fixture(scope="module")
def lib():
    path = _hip.library_path()
    l = ctypes.CDLL(path)
    f = l._Z23scp_persist16_lds_bytesiiiii  # size_t scp_persist16_lds_bytes(int K, int cap, int nblk, int D, int apb)
    f.restype, f.argtypes = ctypes.c_size_t, [ctypes.c_int] * 5
    g = l._Z25scp_persist16_entry_bytesi  # size_t scp_persist16_entry_bytes(int D)
    g.restype, g.argtypes = ctypes.c_size_t, [ctypes.c_int]
    return f, g


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("D,per", SHAPES)
def test_restatement_matches_the_library(lib, K, D, per):
    lds_bytes, ent = lib
    assert ent(D) == entry_bytes(D)
    for cap in (0, 64, 800):
        for nblk in (2, 129, 257, 513):
            assert lds_bytes(K, cap, nblk, D, per) == lean_lds_bytes(K, cap, nblk, D, per), (cap, nblk)


def old_fixed_bytes(K, nblk, D, per):
    """the fixed part of the carve-up before T r (tests/persist_cases.py::entry_cap restates it inline)"""
    nc16 = 16 * nct(D, per)
    rsk, tk, nks = pc._pad_col(K), (K + 15) >> 4, (K + 3) >> 2
    dbl = 2 * nc16 * rsk + tk * nks * 64 + 2 * nblk + per * AB_STRIDE
    if 2 * nc16 * rsk < NCHK * nblk:
        dbl += NCHK * nblk
    ints = per * K + 1
    return dbl * 8 + (ints + 1) // 2 * 2 * 4


@pytest.mark.parametrize("K", KS)
def test_lean8_capacity_against_the_old_carve_up(K):
    """<2, 8>: the fixed part grows by exactly the two added tiles; the capacity is at least the old formula's with those
    tiles taken out (the entries are smaller now)"""
    D, per, N = 2, 8, 1024
    nb = N // per + 1
    rsk, tk, nks = pc._pad_col(K), (K + 15) >> 4, (K + 3) >> 2
    tiles = (16 * rsk + tk * nks * 64) * 8
    old_fixed = old_fixed_bytes(K, nb, D, per)
    assert (BUDGET - old_fixed) // ((4 * D + 4) * 8 + 4) // 64 * 64 == pc.entry_cap(3, N, K, D)
    assert lean_lds_bytes(K, 0, nb, D, per) == old_fixed + tiles
    old_minus_tiles = (BUDGET - old_fixed - tiles) // ((4 * D + 4) * 8 + 4) // 64 * 64
    new = lean_entry_cap(3, N, K, D)
    assert new >= old_minus_tiles > 0
    if K == 50:  # the bench shape, ~197 incident rows per block of 8 agents on average (12 583 rows x 2 / 128)
        assert (pc.entry_cap(3, N, K, D), old_minus_tiles, new) == (1088, 768, 1088)


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("D,per", [(2, 16), (3, 8)])
def test_other_lean_kernels_only_gain(K, D, per):
    """no added tiles there: the smaller entries only raise their capacity"""
    kernel = 2 if per == 16 else 3
    for N in (per + 1, 1100, 4096):
        assert lean_entry_cap(kernel, N, K, D) >= pc.entry_cap(kernel, N, K, D)


@pytest.mark.parametrize("case", [c for c in pc.CASES if c.kernel in (2, 3)], ids=lambda c: c.id)
def test_every_lean_case_still_fits(case):
    sc = case.scen
    prob, _, _, _, _, W = pc.setup(sc)
    per = pc.apb(case.kernel, sc.dim)
    assert pc.block_entries(prob, W, per).max() < lean_entry_cap(case.kernel, sc.N, sc.K, sc.dim)
