"""The near part of a two-species operator is 1 (x) T' + D: a down hop's amplitude and fermion sign do not depend on the up
configuration (the generator orders all up operators before all down operators), so the off-diagonal values of a near row are the
same bits in every major index and only the diagonal entry differs.  The near pass then reads the values from the pattern of the
first major index (KronSplit::vp_n, K = near entries per major index, k_spmv_wave2<.., VP>) and the diagonal from one double
(dg_n: its real part; the form is taken only where every stored diagonal has the imaginary part +0.0) and one position byte (dp_n)
per row; the per-entry array stays the stored form.  The operands of every product and the order
of every sum are unchanged, so every result must equal BIT FOR BIT the one of the same operator created under
QBH_DEBUG=near_vals=0 (the per-entry values, which the other test files pin to the oracle): no tolerance anywhere in this file.

Hubbard 4x3: (n_up, n_dn) = (5, 7): S = 792, K = 10,872, about 21 blocks per major index; (6, 4): S = 495, S % 8 = 7, K = 6,255.
Both have thousands of near blocks: blocks that straddle two major indices (the pattern wraps), blocks that start a major index
with a lead that belongs to the one before, a partial last block.  chain(12) 6+6 and one bond 6+6 (tests/test_gpu_nearlens.py)
have blocks of more than 64 rows: the reload round of lengths and diagonal positions runs.

The pattern is taken beside the 2-byte near columns, with the length array or without it: tests/test_gpu_nearlens.py compares the
bytes of a default operator with one created under near_lens=0 and allows exactly the length array between them, so both must hold
the pattern or neither.  Hence near_lens=0 is a case where the pattern IS taken here (the pass form without lengths), and only
kron_cols16=0 one where it is not.  For the same reason the diagonal is held as 8 bytes per row, not 16:
tests/test_gpu_configs.py bounds bytes_matrix of the 4x5 operator at 18 B per nonzero + 64 B per row, which leaves 9.4 B per row."""
import functools
import math
import os

import numpy as np
import pytest

import genforms
import quantum_basis_amd as q
from quantum_basis_amd import engine, lattices

pytestmark = pytest.mark.gpu
PLAIN = dict(value_dict=0, real_fast_path=0)
BONDS = lattices.square(4, 3)
SHAPES = [(5, 7), (6, 4)]
NEAR_PER_MAJOR = {(5, 7): 10872, (6, 4): 6255}           # counted on the host for these shapes when the form was proposed
MANY_ROWS = {"chain12_6_6": lattices.chain(12), "one_bond_6_6": [(0, 1)]}
KNOB = "near_vals=0"
TAIL = 64                    # zeroed entries behind the derived arrays


def _rand(n, seed):
    rng = np.random.default_rng(seed)
    return (rng.normal(size=n) + 1j * rng.normal(size=n)).astype(np.complex128)


def _create(make, debug):
    """make() under QBH_DEBUG=debug (None: unset, the default forms); the variable is read when the operator is created"""
    old = os.environ.get("QBH_DEBUG")
    try:
        if debug is None:
            os.environ.pop("QBH_DEBUG", None)
        else:
            os.environ["QBH_DEBUG"] = debug
        return make()
    finally:
        if old is None:
            os.environ.pop("QBH_DEBUG", None)
        else:
            os.environ["QBH_DEBUG"] = old


def _pair(make, also=None):
    """(pattern, knob off); `also`: a knob both are created under"""
    return _create(make, also), _create(make, KNOB if also is None else also + "," + KNOB)


def _hubbard(shape, rows=None, bonds=BONDS, **opts):
    nu, nd = shape
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


@functools.lru_cache(maxsize=None)
def _near_per_major(n_dn, bonds=None):
    """K: the entries of one major index that stay inside it, from the host generator.  The near block of a major index is T' plus the
    stored diagonal whatever the up sector is, so the generator runs with ONE up particle (12 major indices) and every one of them is
    counted."""
    dim, ia, ja, val = genforms.hubbard_gen(12, 1, n_dn, list(bonds) if bonds else BONDS, 1.0, 1.1)
    S = math.comb(12, n_dn)
    rows = np.repeat(np.arange(dim), np.diff(ia))
    per_major = np.bincount((rows // S)[rows // S == ja // S], minlength=dim // S)
    assert np.all(per_major == per_major[0])
    return int(per_major[0])


def _pattern_bytes(K, nrows):
    """what the three arrays add to bytes_matrix: the pattern and one double and one byte per row, each with its tail"""
    return 16 * (K + TAIL) + 8 * (nrows + TAIL) + (nrows + TAIL)


def _taken(G, P, K):
    extra = G.info().bytes_matrix - P.info().bytes_matrix
    print("K %d nrows %d extra %d" % (K, G.info().nrows, extra))
    return extra == _pattern_bytes(K, G.info().nrows)


# ---------------------------------------------------------------------------------------------------- the form is taken
@pytest.mark.parametrize("shape", SHAPES)
def test_pattern_is_taken(shape):
    K = _near_per_major(shape[1])
    assert K == NEAR_PER_MAJOR[shape] >= 1024
    G, P = _pair(_hubbard(shape))
    ig, ip = G.info(), P.info()
    assert ig.kron_minor == math.comb(12, shape[1]) and ig.kron_cols16 == 3 and ip.kron_cols16 == 3
    assert (ig.nnz - ig.kron_far_nnz) // 512 > 1000                  # thousands of near blocks
    assert _taken(G, P, K)
    G.destroy()
    P.destroy()


@pytest.mark.parametrize("wave_walk", [2, -1])           # the static chunked walk / the ordered per-XCD counters
@pytest.mark.parametrize("deterministic", [1, 0])
@pytest.mark.parametrize("shape", SHAPES)
def test_products_and_fused_reductions_are_equal(shape, deterministic, wave_walk):
    G, P = _pair(_hubbard(shape, deterministic=deterministic, wave_walk=wave_walk))
    assert _taken(G, P, NEAR_PER_MAJOR[shape])
    _same_products(G, P)
    G.destroy()
    P.destroy()


@pytest.mark.parametrize("wave_walk", [2, -1])
@pytest.mark.parametrize("name", list(MANY_ROWS))
def test_blocks_of_more_than_64_rows(name, wave_walk):
    """rows of 3-13 / 1-2 entries: most blocks take a further round of 64 lengths and diagonal positions inside the row loop"""
    bonds = MANY_ROWS[name]
    K = _near_per_major(6, tuple(bonds))
    assert K >= 1024
    G, P = _pair(_hubbard((6, 6), bonds=bonds, deterministic=1, wave_walk=wave_walk))
    assert _taken(G, P, K)
    _same_products(G, P, seed=7)
    G.destroy()
    P.destroy()


@pytest.mark.parametrize("wave_walk", [2, -1])
@pytest.mark.parametrize("shape", SHAPES)
def test_pattern_without_the_row_lengths(shape, wave_walk):
    """near_lens=0: the pass form that reads the row pointers takes the pattern as well (the diagonal's position is loaded beside them)"""
    G, P = _pair(_hubbard(shape, deterministic=1, wave_walk=wave_walk), also="near_lens=0")
    L = _create(_hubbard(shape, deterministic=1, wave_walk=wave_walk), None)
    assert _taken(G, P, NEAR_PER_MAJOR[shape])
    assert L.info().bytes_matrix - G.info().bytes_matrix == G.info().nrows + TAIL      # the length array and nothing else
    _same_products(G, P, seed=9)
    for A in (G, P, L):
        A.destroy()


@pytest.mark.parametrize("shape", SHAPES)
def test_twenty_lanczos_steps_are_equal(shape):
    """the pipelined loop: yin != y, the coefficients on the device"""
    G, P = _pair(_hubbard(shape, deterministic=1))
    assert _taken(G, P, NEAR_PER_MAJOR[shape])
    maxit, out = 32, []
    for A in (G, P):
        v = A.vec(2)
        hess = np.zeros(2 * maxit)
        A.randomize(v.at(0), 1)
        m = engine.lanczos(0, 20, maxit, A.dim, A, None, hess, "sr_val0", device_v=v)
        out.append((m, hess, v.download()))
        v.free()
    assert out[0][0] == out[1][0] == 20
    assert np.array_equal(out[0][1], out[1][1]) and np.count_nonzero(out[0][1]) >= 39       # a_j and b_j
    assert np.array_equal(_bits(out[0][2]), _bits(out[1][2])) and np.abs(out[0][2]).max() > 0.0     # both vectors
    G.destroy()
    P.destroy()


@pytest.mark.parametrize("shape,majors", [((5, 7), (100, 431)), ((6, 4), (0, 307))])
def test_row_shard_of_whole_major_indices(shape, majors):
    """the pattern is the one of the shard's FIRST major index; pass form 2 (one GPU driving the shard with the full-length x)"""
    S, dim = math.comb(12, shape[1]), math.comb(12, shape[0]) * math.comb(12, shape[1])
    G, P = _pair(_hubbard(shape, rows=(majors[0] * S, majors[1] * S), deterministic=1))
    ig = G.info()
    assert ig.kron_cols16 == 3 and ig.nrows == (majors[1] - majors[0]) * S and ig.ncols == dim
    assert _taken(G, P, NEAR_PER_MAJOR[shape])
    _same_products(G, P, ncols=dim)
    G.destroy()
    P.destroy()


@pytest.mark.parametrize("shape", SHAPES)
def test_one_rank_communicator_and_the_merge_back(shape):
    """Under a communicator the near pass has no far addend (pass form 1); afterwards the parts are merged back into rows
    (k_kron_merge_rows reads the per-entry values) and must be the operator that was never split."""
    from quantum_basis_amd import dist as qdist
    G, P = _pair(_hubbard(shape, deterministic=1))
    for A in (G, P):
        qdist.NativeComm(A.dim, rank=0, world=1).attach(A)
    assert G.info().kron_cols16 == 3 and _taken(G, P, NEAR_PER_MAJOR[shape])          # still split, still the pattern
    n_gather = G.stats().n_gather
    _same_products(G, P, seed=11)
    assert G.stats().n_gather > n_gather
    R = q.csr_mat.hubbard(12, shape[0], shape[1], BONDS, t=1.0, U=1.1, opts=q.make_opts(kron_split=0, **PLAIN))
    for u, v in zip(G.download(), R.download()):
        assert np.array_equal(_bits(u), _bits(v))
    for A in (G, P, R):
        A.destroy()


@pytest.mark.parametrize("shape", SHAPES)
def test_download_is_equal(shape):
    G, P = _pair(_hubbard(shape))
    assert _taken(G, P, NEAR_PER_MAJOR[shape])
    for u, v in zip(G.download(), P.download()):
        assert np.array_equal(_bits(u), _bits(v))
    r0, r1 = G.dim // 3, G.dim // 3 + 2000                       # a row range that starts inside a major index
    for u, v in zip(G.download(r0, r1), P.download(r0, r1)):
        assert np.array_equal(_bits(u), _bits(v))
    G.destroy()
    P.destroy()


# ---------------------------------------------------------------------------------------------------- host arrays
@functools.lru_cache(maxsize=None)
def _host_arrays_57():
    """the (5, 7) operator as full host arrays, downloaded once; callers copy what they change"""
    R = q.csr_mat.hubbard(12, 5, 7, BONDS, t=1.0, U=1.1, opts=q.make_opts(kron_split=0, **PLAIN))
    ia, ja, val = R.download()
    dim = R.dim
    R.destroy()
    ja = ja.astype(np.int64)
    rows = np.repeat(np.arange(dim), np.diff(ia))
    S = 792
    hop = ((rows // S) == (ja // S)) & (rows != ja)              # the down hops: near and off the diagonal
    for a in (ia, ja, val, rows, hop):
        a.setflags(write=False)
    return dim, S, ia, ja, val, rows, hop


def _from_host(dim, S, ia, ja, val, **opts):
    return lambda: q.csr_mat(dim, ia, ja, val, sym=False, opts=q.make_opts(kron_minor=S, kron_split=2, **PLAIN, **opts))


def _entry(ia, ja, row, col):
    k = int(ia[row]) + int(np.searchsorted(ja[ia[row]:ia[row + 1]], col))
    assert ja[k] == col
    return k


def _hop_of_major(major, nth=5):
    """(k, k of the transposed entry) of a down hop inside major index `major`"""
    dim, S, ia, ja, val, rows, hop = _host_arrays_57()
    k = int(np.flatnonzero(hop & (rows // S == major))[nth])
    return k, _entry(ia, ja, int(ja[k]), int(rows[k]))


def test_complex_hops_with_a_fixed_phase():
    """every down hop times p(d_row) conj(p(d_col)), p a random unit phase per MINOR index: Hermitian still, complex, and still the
    same bits in every major index"""
    dim, S, ia, ja, val, rows, hop = _host_arrays_57()
    rng = np.random.default_rng(23)
    p = np.exp(2j * np.pi * rng.random(S))
    nval = val.copy()
    nval[hop] = val[hop] * (p[rows[hop] % S] * np.conj(p[ja[hop] % S]))
    assert np.abs(nval[hop].imag).max() > 0.1
    G, P = _pair(_from_host(dim, S, ia, ja, nval))
    assert G.info().kron_minor == S and G.info().kron_cols16 == 3
    assert _taken(G, P, NEAR_PER_MAJOR[(5, 7)])
    _same_products(G, P, seed=29)
    dia, dja, dval = G.download()
    assert np.array_equal(dia, ia) and np.array_equal(dja, ja) and np.array_equal(_bits(dval), _bits(nval))
    G.destroy()
    P.destroy()


# ---------------------------------------------------------------------------------------------------- the form is not taken
def _not_taken(make, seed, nval=None):
    G, P = _pair(make)
    ig, ip = G.info(), P.info()
    assert ig.kron_cols16 == 3 and ip.kron_cols16 == 3
    assert ig.bytes_matrix == ip.bytes_matrix
    _same_products(G, P, seed=seed)
    if nval is not None:
        assert np.array_equal(_bits(G.download()[2]), _bits(nval))
    G.destroy()
    P.destroy()


@pytest.mark.parametrize("major", [413, 0])              # a major index other than the first / the first (the pattern itself)
def test_one_hop_one_ulp_off_keeps_the_per_entry_values(major):
    """one down hop of one major index, and its transposed partner, differ from the other major indices' in the last bit"""
    dim, S, ia, ja, val, rows, hop = _host_arrays_57()
    k, kt = _hop_of_major(major)
    nval = val.copy()
    nval[k] = complex(np.nextafter(val[k].real, 0.0), val[k].imag)
    nval[kt] = np.conj(nval[k])
    assert k != kt and val[kt] == val[k] and np.count_nonzero(_bits(nval) != _bits(val)) == 2
    _not_taken(_from_host(dim, S, ia, ja, nval), 37, nval)


def test_an_imaginary_part_of_1e_300_keeps_the_per_entry_values():
    dim, S, ia, ja, val, rows, hop = _host_arrays_57()
    k, kt = _hop_of_major(413)
    nval = val.copy()
    nval[k] = complex(val[k].real, 1e-300)
    assert np.count_nonzero(_bits(nval) != _bits(val)) == 1
    _not_taken(_from_host(dim, S, ia, ja, nval, check_hermitian=0), 41, nval)


@pytest.mark.parametrize("imag", [1e-300, -0.0])
def test_a_diagonal_with_an_imaginary_part_keeps_the_per_entry_values(imag):
    """the diagonal is kept as one double: an imaginary part that is not +0.0 as bits, -0.0 included, is a violation"""
    dim, S, ia, ja, val, rows, hop = _host_arrays_57()
    r = 413 * S + 101
    k = _entry(ia, ja, r, r)
    nval = val.copy()
    nval[k] = complex(val[k].real, imag)
    assert np.count_nonzero(nval.view(np.int64) != val.view(np.int64)) == 1          # as bits: -0.0 == 0.0 as numbers
    _not_taken(_from_host(dim, S, ia, ja, nval, check_hermitian=0), 59, nval)


def test_a_row_without_its_stored_diagonal_keeps_the_per_entry_values():
    dim, S, ia, ja, val, rows, hop = _host_arrays_57()
    r = 413 * S + 101
    k = _entry(ia, ja, r, r)
    nia = ia.copy()
    nia[r + 1:] -= 1
    nja, nval = np.delete(ja, k), np.delete(val, k)
    G, P = _pair(_from_host(dim, S, nia, nja, nval))
    assert G.info().kron_cols16 == 3 and G.info().bytes_matrix == P.info().bytes_matrix
    _same_products(G, P, seed=43)
    dia, dja, dval = G.download()
    assert np.array_equal(dia, nia) and np.array_equal(dja, nja) and np.array_equal(_bits(dval), _bits(nval))
    G.destroy()
    P.destroy()


@pytest.mark.parametrize("shape,K", [((4, 4), 550), ((3, 5), 416)])
def test_a_pattern_below_1024_entries_is_not_taken(shape, K):
    bonds = lattices.square(4, 2)
    dimg, ia, ja, val = genforms.hubbard_gen(8, shape[0], shape[1], bonds, 1.0, 1.1)
    S = math.comb(8, shape[1])
    rows = np.repeat(np.arange(dimg), np.diff(ia))
    assert np.count_nonzero((rows < S) & (ja < S)) == K < 1024
    make = lambda: q.csr_mat.hubbard(8, shape[0], shape[1], bonds, t=1.0, U=1.1, opts=q.make_opts(kron_split=2, **PLAIN))
    G, P = _pair(make)
    assert G.info().kron_minor == S and G.info().kron_cols16 & 1
    assert G.info().bytes_matrix == P.info().bytes_matrix
    _same_products(G, P, seed=47)
    G.destroy()
    P.destroy()


@pytest.mark.parametrize("shape", SHAPES)
def test_no_pattern_without_two_byte_columns(shape):
    G, P = _pair(_hubbard(shape, kron_cols16=0))
    assert G.info().kron_cols16 == 0 and G.info().bytes_matrix == P.info().bytes_matrix
    _same_products(G, P, seed=53)
    G.destroy()
    P.destroy()
