"""The sliced far part of a T (x) 1 operator holds the same VALUE in all 8 slots of a line of its stream wherever the hop's amplitude
and sign depend on the major index alone (the Hubbard generator orders all up operators before all down operators).  The far pass then
reads that value once per line from a derived array 1/8 the size (KronSplit::v8_f, k_spmv_wave2<.., V8>, taken only beside the grouped
columns c8_f): the 8 lanes of a line load the one address; the per-slot array stays the stored form.  The operands of every
product and the order of every sum are unchanged, so every result must equal BIT FOR BIT the one of the same operator created under
QBH_DEBUG=far_vals8=0 (the per-slot values, which the other test files pin to the oracle): no tolerance anywhere in this file.

Hubbard 4x3: (n_up, n_dn) = (5, 7): S = 792, a multiple of 8; (6, 4): S = 495, S % 8 = 7 -- a cross part and a narrow last band.  Both
have thousands of 512-slot far blocks: groups cut at block boundaries, blocks that span two bands, a partial last block."""
import functools
import math
import os

import numpy as np
import pytest

import quantum_basis_amd as q
from quantum_basis_amd import engine, lattices

pytestmark = pytest.mark.gpu
PLAIN = dict(value_dict=0, real_fast_path=0)
BONDS = lattices.square(4, 3)
SHAPES = [(5, 7), (6, 4)]
KNOB = "far_vals8=0"
TAIL = 64                    # zeroed entries behind the derived arrays


def _rand(n, seed):
    rng = np.random.default_rng(seed)
    return (rng.normal(size=n) + 1j * rng.normal(size=n)).astype(np.complex128)


def _create(make, debug):
    """make() under QBH_DEBUG=debug (None: unset, the grouped streams)"""
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


def _pair(make):
    return _create(make, None), _create(make, KNOB)


def _hubbard(shape, rows=None, **opts):
    nu, nd = shape
    return lambda: q.csr_mat.hubbard(12, nu, nd, BONDS, t=1.0, U=1.1, rows=rows, opts=q.make_opts(kron_split=2, **PLAIN, **opts))


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


def _grouped_bytes(far_nnz):
    """what v8_f adds to bytes_matrix: 16 bytes per 8 far slots + the tail; the far parts here are not padded (slots = nonzeros)"""
    assert far_nnz % 8 == 0
    return 16 * (far_nnz // 8 + TAIL)


@pytest.mark.parametrize("shape", SHAPES)
def test_grouped_form_is_taken(shape):
    G, P = _pair(_hubbard(shape))
    ig, ip = G.info(), P.info()
    assert ig.kron_minor == math.comb(12, shape[1]) and ig.kron_sliced == 1 and ip.kron_sliced == 1
    assert ig.kron_cols16 == 3 and ip.kron_cols16 == 3               # the per-slot arrays stay the stored form
    assert ig.kron_far_nnz == ip.kron_far_nnz > 512 * 1000           # thousands of far blocks
    extra = ig.bytes_matrix - ip.bytes_matrix
    print("far_nnz %d extra %d" % (ig.kron_far_nnz, extra))
    assert 2 * ig.kron_far_nnz <= extra <= 2 * ig.kron_far_nnz + 16 * TAIL
    assert extra == _grouped_bytes(ig.kron_far_nnz)
    G.destroy()
    P.destroy()


@pytest.mark.parametrize("wave_walk", [2, -1])           # the static chunked walk / the ordered per-XCD counters
@pytest.mark.parametrize("deterministic", [1, 0])
@pytest.mark.parametrize("shape", SHAPES)
def test_products_and_fused_reductions_are_equal(shape, deterministic, wave_walk):
    G, P = _pair(_hubbard(shape, deterministic=deterministic, wave_walk=wave_walk))
    assert G.info().bytes_matrix - P.info().bytes_matrix == _grouped_bytes(G.info().kron_far_nnz)
    _same_products(G, P)
    G.destroy()
    P.destroy()


@pytest.mark.parametrize("shape", SHAPES)
def test_twenty_lanczos_steps_are_equal(shape):
    G, P = _pair(_hubbard(shape, deterministic=1))
    assert G.info().bytes_matrix > P.info().bytes_matrix
    maxit, out = 32, []
    for A in (G, P):
        v = A.vec(2)
        hess = np.zeros(2 * maxit)
        A.randomize(v.at(0), 1)
        m = engine.lanczos(0, 20, maxit, A.dim, A, None, hess, "sr_val0", device_v=v)
        v.free()
        out.append((m, hess))
    assert out[0][0] == out[1][0] == 20
    assert np.array_equal(out[0][1], out[1][1]) and np.count_nonzero(out[0][1]) >= 39       # a_j and b_j
    G.destroy()
    P.destroy()


@pytest.mark.parametrize("shape,majors", [((5, 7), (100, 431)), ((6, 4), (0, 307))])
def test_row_shard_of_whole_major_indices(shape, majors):
    S, dim = math.comb(12, shape[1]), math.comb(12, shape[0]) * math.comb(12, shape[1])
    G, P = _pair(_hubbard(shape, rows=(majors[0] * S, majors[1] * S), deterministic=1))
    ig, ip = G.info(), P.info()
    assert ig.kron_cols16 == 3 and ip.kron_cols16 == 3 and ig.nrows == (majors[1] - majors[0]) * S and ig.ncols == dim
    assert ig.bytes_matrix - ip.bytes_matrix == _grouped_bytes(ig.kron_far_nnz)
    _same_products(G, P, ncols=dim)
    G.destroy()
    P.destroy()


@pytest.mark.parametrize("shape", SHAPES)
def test_one_rank_communicator_and_the_merge_back(shape):
    """Under a communicator the far pass follows k_kron_place and the near pass has no far addend; afterwards the parts are merged
    back into rows (k_kron_merge_rows reads the per-slot values) and must be the operator that was never split."""
    from quantum_basis_amd import dist as qdist
    G, P = _pair(_hubbard(shape, deterministic=1))
    for A in (G, P):
        qdist.NativeComm(A.dim, rank=0, world=1).attach(A)
    ig, ip = G.info(), P.info()
    assert ig.kron_cols16 == 3 and ig.bytes_matrix - ip.bytes_matrix == _grouped_bytes(ig.kron_far_nnz)      # still split, still grouped
    n_gather = G.stats().n_gather
    _same_products(G, P, seed=11)
    assert G.stats().n_gather > n_gather
    R = q.csr_mat.hubbard(12, shape[0], shape[1], BONDS, t=1.0, U=1.1, opts=q.make_opts(kron_split=0, **PLAIN))
    for u, v in zip(G.download(), R.download()):
        assert np.array_equal(_bits(u), _bits(v))
    for A in (G, P, R):
        A.destroy()


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
    far = (rows // S) != (ja // S)
    for a in (ia, ja, val, rows, far):
        a.setflags(write=False)
    return dim, S, ia, ja, val, rows, far


def _from_host(dim, S, ia, ja, val, **opts):
    return lambda: q.csr_mat(dim, ia, ja, val, sym=False, opts=q.make_opts(kron_minor=S, kron_split=2, **PLAIN, **opts))


def test_complex_values_uniform_per_line():
    """far values times p(u_row) conj(p(u_col)), p a random unit phase per major index: Hermitian still, complex, and still one
    value per line"""
    dim, S, ia, ja, val, rows, far = _host_arrays_57()
    rng = np.random.default_rng(23)
    p = np.exp(2j * np.pi * rng.random(dim // S))
    nval = val.copy()
    nval[far] = val[far] * (p[rows[far] // S] * np.conj(p[ja[far] // S]))
    assert np.abs(nval[far].imag).max() > 0.1
    G, P = _pair(_from_host(dim, S, ia, ja, nval))
    ig, ip = G.info(), P.info()
    assert ig.kron_minor == S and ig.kron_sliced == 1 and ig.kron_cols16 == 3 and ip.kron_cols16 == 3
    assert ig.bytes_matrix - ip.bytes_matrix == _grouped_bytes(ig.kron_far_nnz)
    _same_products(G, P, seed=29)
    dia, dja, dval = G.download()
    assert np.array_equal(dia, ia) and np.array_equal(dja, ja) and np.array_equal(_bits(dval), _bits(nval))
    G.destroy()
    P.destroy()


def test_uniform_columns_with_values_that_are_not():
    """the far values of the odd minor indices negated (symmetric still: a far entry keeps the minor index): every line of the stream
    names one major index and holds two values -- the columns are grouped, the values are not"""
    dim, S, ia, ja, val, rows, far = _host_arrays_57()
    nval = val.copy()
    odd = far & ((rows % S) % 2 == 1)
    nval[odd] = -val[odd]
    make = _from_host(dim, S, ia, ja, nval)
    G, P = _pair(make)
    C = _create(make, "far_cols8=0")
    ig, ip, ic = G.info(), P.info(), C.info()
    assert ig.kron_sliced == 1 and ig.kron_cols16 == 3 and ip.kron_cols16 == 3
    assert ig.bytes_matrix == ip.bytes_matrix                                        # no grouped values ...
    assert ig.bytes_matrix - ic.bytes_matrix == 2 * (ig.kron_far_nnz // 8 + TAIL)    # ... beside grouped columns
    _same_products(G, P, seed=31)
    dia, dja, dval = G.download()
    assert np.array_equal(dia, ia) and np.array_equal(dja, ja) and np.array_equal(_bits(dval), _bits(nval))
    for A in (G, P, C):
        A.destroy()


@pytest.mark.parametrize("variant", ["real_part_one_ulp", "imaginary_part_1e-300"])
def test_one_deviating_slot_keeps_the_per_slot_values(variant):
    """one slot of the LAST far group (the last 8 rows of the operator: last major index, last band) differs from the 7 others of its
    line in the last bit of its real part / in an imaginary part far below anything a tolerance would see"""
    dim, S, ia, ja, val, rows, far = _host_arrays_57()
    k = int(np.flatnonzero(far & (rows == dim - 3))[-1])         # S is a multiple of 8: rows dim - 8 .. dim - 1 are the last group
    nval = val.copy()
    if variant == "real_part_one_ulp":
        nval[k] = complex(np.nextafter(val[k].real, 0.0), val[k].imag)
    else:
        nval[k] = complex(val[k].real, 1e-300)
    assert nval[k] != val[k] and np.count_nonzero(_bits(nval) != _bits(val)) == 1
    G, P = _pair(_from_host(dim, S, ia, ja, nval, check_hermitian=0))
    ig, ip = G.info(), P.info()
    assert ig.kron_sliced == 1 and ig.kron_cols16 == 3 and ip.kron_cols16 == 3
    assert ig.bytes_matrix == ip.bytes_matrix
    _same_products(G, P, seed=37)
    dval = G.download()[2]
    assert np.array_equal(_bits(dval), _bits(nval))
    G.destroy()
    P.destroy()


@pytest.mark.parametrize("shape", SHAPES)
def test_no_grouped_values_without_grouped_columns(shape):
    A = _create(_hubbard(shape), "far_cols8=0")
    B = _create(_hubbard(shape), "far_cols8=0,far_vals8=0")
    assert A.info().kron_cols16 == 3 and A.info().bytes_matrix == B.info().bytes_matrix
    A.destroy()
    B.destroy()
