"""The sliced far part of a T (x) 1 operator names the same major index in all 8 slots of a line of its stream.  The far pass then
reads that value once per line from a derived array 1/8 the size (KronSplit::c8_f, k_spmv_wave2<.., G8>) and forms the per-slot
values by cross-lane moves; the per-slot array stays the stored form.  Gather addresses and everything behind them are unchanged, so
every result must equal BIT FOR BIT the one of the same operator created under QBH_DEBUG=far_cols8=0 (the per-slot stream, which the
other test files pin to the oracle): no tolerance anywhere in this file.

Hubbard 4x3: (n_up, n_dn) = (5, 7): S = 792, a multiple of 8; (6, 4): S = 495, S % 8 = 7 -- a cross part and a narrow last band.  Both
have thousands of 512-slot far blocks: groups cut at block boundaries, blocks that span two bands, a partial last block."""
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
KNOB = "far_cols8=0"


def _rand(n, seed):
    rng = np.random.default_rng(seed)
    return (rng.normal(size=n) + 1j * rng.normal(size=n)).astype(np.complex128)


def _create(make, grouped):
    """make() with the grouped stream (the default) or under the measurement knob that keeps the per-slot stream"""
    old = os.environ.get("QBH_DEBUG")
    try:
        if grouped:
            os.environ.pop("QBH_DEBUG", None)
        else:
            os.environ["QBH_DEBUG"] = KNOB
        return make()
    finally:
        if old is None:
            os.environ.pop("QBH_DEBUG", None)
        else:
            os.environ["QBH_DEBUG"] = old


def _pair(make):
    return _create(make, True), _create(make, False)


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


@pytest.mark.parametrize("shape", SHAPES)
def test_grouped_form_is_taken(shape):
    G, P = _pair(_hubbard(shape))
    ig, ip = G.info(), P.info()
    assert ig.kron_minor == math.comb(12, shape[1]) and ig.kron_sliced == 1 and ip.kron_sliced == 1
    assert ig.kron_cols16 == 3 and ip.kron_cols16 == 3               # the per-slot array stays the stored form
    assert ig.kron_far_nnz == ip.kron_far_nnz > 512 * 1000           # thousands of far blocks
    extra = ig.bytes_matrix - ip.bytes_matrix                        # 2 bytes per 8 slots (+ the zeroed tail)
    assert ig.kron_far_nnz // 4 <= extra <= ig.kron_far_nnz // 4 + 64 * ig.nrows
    assert ig.bytes_matrix >= 18 * ig.nnz
    G.destroy()
    P.destroy()


@pytest.mark.parametrize("wave_walk", [2, -1])           # the static chunked walk / the ordered per-XCD counters
@pytest.mark.parametrize("deterministic", [1, 0])
@pytest.mark.parametrize("shape", SHAPES)
def test_products_and_fused_reductions_are_equal(shape, deterministic, wave_walk):
    G, P = _pair(_hubbard(shape, deterministic=deterministic, wave_walk=wave_walk))
    assert G.info().bytes_matrix > P.info().bytes_matrix
    _same_products(G, P)
    G.destroy()
    P.destroy()


@pytest.mark.parametrize("shape", SHAPES)
def test_twenty_lanczos_steps_are_equal(shape):
    G, P = _pair(_hubbard(shape, deterministic=1))
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


@pytest.mark.parametrize("shape", SHAPES)
def test_download_returns_the_int32_operator(shape):
    G = _create(_hubbard(shape), True)
    P = q.csr_mat.hubbard(12, shape[0], shape[1], BONDS, t=1.0, U=1.1, opts=q.make_opts(kron_split=2, kron_cols16=0, **PLAIN))
    assert G.info().kron_cols16 == 3 and P.info().kron_cols16 == 0
    for u, v in zip(G.download(), P.download()):
        assert np.array_equal(_bits(u), _bits(v))
    G.destroy()
    P.destroy()


@pytest.mark.parametrize("shape,majors", [((5, 7), (100, 431)), ((6, 4), (0, 307))])
def test_row_shard_of_whole_major_indices(shape, majors):
    S, dim = math.comb(12, shape[1]), math.comb(12, shape[0]) * math.comb(12, shape[1])
    G, P = _pair(_hubbard(shape, rows=(majors[0] * S, majors[1] * S), deterministic=1))
    ig, ip = G.info(), P.info()
    assert ig.kron_cols16 == 3 and ip.kron_cols16 == 3 and ig.nrows == (majors[1] - majors[0]) * S and ig.ncols == dim
    assert ig.kron_far_nnz // 4 <= ig.bytes_matrix - ip.bytes_matrix <= ig.kron_far_nnz // 4 + 64 * ig.nrows
    _same_products(G, P, ncols=dim)
    G.destroy()
    P.destroy()


@pytest.mark.parametrize("shape", SHAPES)
def test_one_rank_communicator_and_the_merge_back(shape):
    """Under a communicator the far pass follows k_kron_place and the near pass has no far addend; afterwards the parts are merged
    back into rows (k_kron_merge_rows reads the per-slot array) and must be the operator that never had 2-byte columns."""
    from quantum_basis_amd import dist as qdist
    G, P = _pair(_hubbard(shape, deterministic=1))
    for A in (G, P):
        qdist.NativeComm(A.dim, rank=0, world=1).attach(A)
    assert G.info().kron_cols16 == 3 and G.info().bytes_matrix > P.info().bytes_matrix       # still split, still grouped
    n_gather = G.stats().n_gather
    _same_products(G, P, seed=11)
    assert G.stats().n_gather > n_gather
    R = q.csr_mat.hubbard(12, shape[0], shape[1], BONDS, t=1.0, U=1.1, opts=q.make_opts(kron_split=0, **PLAIN))
    for u, v in zip(G.download(), R.download()):
        assert np.array_equal(_bits(u), _bits(v))
    for A in (G, P, R):
        A.destroy()


def _host_arrays(shape):
    R = q.csr_mat.hubbard(12, shape[0], shape[1], BONDS, t=1.0, U=1.1, opts=q.make_opts(kron_split=0, **PLAIN))
    ia, ja, val = R.download()
    dim = R.dim
    R.destroy()
    return dim, ia, ja.astype(np.int64), val


def test_ragged_far_rows_keep_the_per_slot_stream():
    """The 4x3 operator without the up hops of the minor indices divisible by 29 (the rule of
    test_ragged_far_rows_pad_their_groups_or_fall_back_to_plain_rows; 3.5 % padding: it stays sliced): the groups are not uniform, the
    far pass must keep the stream it had and apply identically."""
    dim, ia, ja, val = _host_arrays((5, 7))
    S = 792
    rows = np.repeat(np.arange(dim), np.diff(ia))
    far = (rows // S) != (ja // S)
    keep = ~(far & ((rows % S) % 29 == 0))
    nia = np.zeros(dim + 1, dtype=np.int64)
    np.cumsum(np.bincount(rows[keep], minlength=dim), out=nia[1:])
    nja, nval = ja[keep], val[keep]
    G, P = _pair(lambda: q.csr_mat(dim, nia, nja, nval, sym=False, opts=q.make_opts(kron_minor=S, kron_split=2, **PLAIN)))
    ig, ip = G.info(), P.info()
    assert ig.kron_minor == S and ig.kron_sliced == 1 and ip.kron_sliced == 1
    assert ig.bytes_matrix == ip.bytes_matrix and ig.kron_cols16 == ip.kron_cols16
    _same_products(G, P, seed=9)
    G.destroy()
    P.destroy()


def test_lines_that_are_not_uniform_keep_the_per_slot_stream():
    """Same row lengths, so nothing is padded and the far part does get its 2-byte per-slot columns -- but the far entries of the odd
    minor indices point c major indices further (cyclically; c such that none of them lands on the row's own major index): a line of
    the stream then names two major indices, the conversion must notice and the far pass keep reading slot by slot."""
    dim, ia, ja, val = _host_arrays((5, 7))
    S, NU = 792, 792
    rows = np.repeat(np.arange(dim), np.diff(ia))
    far = (rows // S) != (ja // S)
    taken = np.unique((rows[far] // S - ja[far] // S) % NU)
    free = np.setdiff1d(np.arange(1, NU), taken)
    assert free.size > 0
    c = int(free[0])
    move = far & ((rows % S) % 2 == 1)
    nja = ja.copy()
    nja[move] = ((ja[move] // S + c) % NU) * S + ja[move] % S
    order = np.lexsort((nja, rows))                                 # columns ascending inside every row again
    nja, nval = nja[order], val[order]
    G, P = _pair(lambda: q.csr_mat(dim, ia, nja, nval, sym=False,
                                   opts=q.make_opts(kron_minor=S, kron_split=2, check_hermitian=0, **PLAIN)))
    ig, ip = G.info(), P.info()
    assert ig.kron_minor == S and ig.kron_sliced == 1 and ig.kron_cols16 == 3 and ip.kron_cols16 == 3
    assert ig.bytes_matrix == ip.bytes_matrix
    _same_products(G, P, seed=17)
    dia, dja, dval = G.download()
    assert np.array_equal(dia, ia) and np.array_equal(dja, nja) and np.array_equal(_bits(dval), _bits(nval))
    G.destroy()
    P.destroy()
