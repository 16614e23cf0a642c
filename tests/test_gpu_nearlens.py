"""The near pass of a one-class split operator needs the OFFSETS of a wave block's rows, and those are the prefix sums of the rows'
lengths from the descriptor's first entry on.  It reads the lengths, one byte per row, from a derived array (KronSplit::len_n,
k_spmv_wave2<.., NL>) and forms the offsets across the lanes; the row pointers stay the stored form.
Entries, their order inside a row, the epilogue arithmetic and the order rows are finished in are unchanged, so every result must
equal BIT FOR BIT the one of the same operator created under QBH_DEBUG=near_lens=0 (the row pointers, which the other test files pin
to the oracle): no tolerance anywhere in this file.

Shapes (row counts per 512-entry near block counted on the host):
  square(4,3) (5,7): S = 792, every near block has 33-43 rows -- the second pass of the row loop always runs;
  square(4,3) (6,4): S = 495, S % 8 = 7: 33-45 rows per block, a narrow last band and a cross part;
  chain(12) 6+6:     S = 924, rows of 3-13 entries: 63 % of the blocks have more than 64 rows (up to 85): the reload round runs;
  one bond, 6+6:     rows of 1-2 entries, up to 339 rows per block: several reload rounds."""
import math
import os

import numpy as np
import pytest

import quantum_basis_amd as q
from quantum_basis_amd import engine, lattices

pytestmark = pytest.mark.gpu
PLAIN = dict(value_dict=0, real_fast_path=0)
SQ = lattices.square(4, 3)
SHAPES = {
    "sq43_5_7": (5, 7, SQ),
    "sq43_6_4": (6, 4, SQ),
    "chain12_6_6": (6, 6, lattices.chain(12)),
    "one_bond_6_6": (6, 6, [(0, 1)]),
}
FIRST, SECOND = "sq43_5_7", "sq43_6_4"


def _rand(n, seed):
    rng = np.random.default_rng(seed)
    return (rng.normal(size=n) + 1j * rng.normal(size=n)).astype(np.complex128)


def _create(make, knob):
    """make() under QBH_DEBUG=knob (None: the default forms); the variable is read when the operator is created"""
    old = os.environ.get("QBH_DEBUG")
    try:
        if knob is None:
            os.environ.pop("QBH_DEBUG", None)
        else:
            os.environ["QBH_DEBUG"] = knob
        return make()
    finally:
        if old is None:
            os.environ.pop("QBH_DEBUG", None)
        else:
            os.environ["QBH_DEBUG"] = old


def _pair(make, knob="near_lens=0"):
    return _create(make, None), _create(make, knob)


def _hubbard(name, rows=None, **opts):
    nu, nd, bonds = SHAPES[name]
    return lambda: q.csr_mat.hubbard(12, nu, nd, bonds, t=1.0, U=1.1, rows=rows, opts=q.make_opts(kron_split=2, **PLAIN, **opts))


def _bits(a):
    return a.view(np.float64) if a.dtype == np.complex128 else a


def _apply(A, x, y0, alpha, beta, gamma, ncols=None):
    xv, yv = engine.DeviceVec(A, ncols or A.dim), A.vec()
    xv.upload(x)
    yv.upload(y0)
    red = A.spmv(xv.ptr, yv.ptr, alpha, beta, gamma, want_red=True)
    y = yv.download()
    xv.free()
    yv.free()
    return y, red


def _same_products(G, P, ncols=None, seed=4):
    x, y0 = _rand(ncols or G.dim, seed), _rand(G.info().nrows, seed + 1)
    for alpha, beta, gamma in [(1.0, 0.0, 0.0), (0.7, -0.3, 0.25)]:
        yg, rg = _apply(G, x, y0, alpha, beta, gamma, ncols)
        yp, rp = _apply(P, x, y0, alpha, beta, gamma, ncols)
        assert np.array_equal(_bits(yg), _bits(yp))                  # every element of y
        assert rg == rp                                              # <x, y> (two sums) and |y|^2
        assert np.abs(yg).max() > 0.0


def _lens_taken(G, P):
    """one byte per near row (+ the zeroed tail of 64) beside the stored form, and nothing else"""
    ig, ip = G.info(), P.info()
    return ig.bytes_matrix - ip.bytes_matrix == ig.nrows + 64


@pytest.mark.parametrize("wave_walk", [2, -1])           # the static chunked walk / the ordered per-XCD counters
@pytest.mark.parametrize("name", list(SHAPES))
def test_products_and_fused_reductions_are_equal(name, wave_walk):
    G, P = _pair(_hubbard(name, deterministic=1, wave_walk=wave_walk))
    ig = G.info()
    assert ig.kron_minor == math.comb(12, SHAPES[name][1]) and ig.kron_far_nnz > 0
    assert _lens_taken(G, P)
    _same_products(G, P)
    G.destroy()
    P.destroy()


@pytest.mark.parametrize("name", [FIRST, SECOND])
def test_default_walk_is_equal(name):
    G, P = _pair(_hubbard(name))
    assert _lens_taken(G, P)
    _same_products(G, P, seed=21)
    G.destroy()
    P.destroy()


@pytest.mark.parametrize("rows", ["inside_a_major_index", "whole_major_indices"])
def test_row_shard(rows):
    """a shard's first and last near block are partial; a cut inside a major index is the case as stated, the cut at whole major
    indices is the one that is split (and takes the lengths)"""
    S, dim = 792, 792 * 792
    r = (100 * S + 17, 431 * S + 401) if rows == "inside_a_major_index" else (100 * S, 431 * S)
    G, P = _pair(_hubbard(FIRST, rows=r, deterministic=1))
    ig = G.info()
    assert ig.nrows == r[1] - r[0] and ig.ncols == dim
    if rows == "whole_major_indices":
        assert ig.kron_minor == S and _lens_taken(G, P)
    _same_products(G, P, ncols=dim)
    G.destroy()
    P.destroy()


def test_twenty_five_lanczos_steps_are_equal():
    G, P = _pair(_hubbard(FIRST, deterministic=1))
    maxit, out = 32, []
    for A in (G, P):
        v = A.vec(2)
        hess = np.zeros(2 * maxit)
        A.randomize(v.at(0), 1)
        m = q.lanczos(0, 25, maxit, A.dim, A, None, hess, "sr_val0", device_v=v)
        out.append((m, hess, v.download()))
        v.free()
    assert out[0][0] == out[1][0] == 25
    assert np.array_equal(out[0][1], out[1][1]) and np.count_nonzero(out[0][1]) >= 49        # a_j and b_j
    assert np.array_equal(_bits(out[0][2]), _bits(out[1][2])) and np.abs(out[0][2]).max() > 0.0     # both vectors
    G.destroy()
    P.destroy()


def test_a_row_longer_than_the_cap_keeps_the_row_pointers():
    """near rows of the first shape reach 19 entries: under near_len_cap=12 the whole operator falls back to the row pointers"""
    C, P = _pair(_hubbard(FIRST, deterministic=1), knob="near_len_cap=12")     # C: default, P: capped
    O = _create(_hubbard(FIRST, deterministic=1), "near_lens=0")
    assert _lens_taken(C, O)
    assert P.info().bytes_matrix == O.info().bytes_matrix
    _same_products(P, O, seed=13)
    for A in (C, P, O):
        A.destroy()
