"""qbh_mf_qudit on the device: the d-level operator applied without a stored matrix, against the stored operator of
qbh_gen_qudit (plain options) and, for the random operators and d = 2, against an independent numpy assembly on the enumerated
sector.  Reference models with their known energies, random complex operators for d = 2 .. 8 on both table paths (LDS and
global memory), words wider than 32 bits, a dimension above one resident grid, ragged row shards and the packed-real drivers."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

import quantum_basis_amd as q
from quantum_basis_amd import _lib, lattices, qudit
import refmodels

pytestmark = pytest.mark.gpu

PLAIN = dict(kron_split=0, sector_cut=-1, value_dict=0, real_fast_path=0)
EPILOGUES = [(1.0, 0.0, 0.0), (1.0, 1.0, 0.0), (0.6, -1.2, 0.0), (1.0, 0.0, -3.0)]


def chain(L):
    return [(i, (i + 1) % L) for i in range(L)]


def square_bonds(Lx, Ly):
    site = lambda x, y: (x % Lx) + Lx * (y % Ly)
    return [b for x in range(Lx) for y in range(Ly) for b in ((site(x, y), site(x + 1, y)), (site(x, y), site(x, y + 1)))]


def _rand(n, seed, real=False):
    rng = np.random.default_rng(seed)
    return (rng.normal(size=n) + (0.0 if real else 1j) * rng.normal(size=n)).astype(np.complex128)


def sector_words(n, d, total):
    """The sector in the generator's order (ascending sum l_s d^s), enumerated without walking all d^n words."""
    out = []

    def rec(s, left, w):                        # sites n-1 .. 0, most significant first, levels ascending: already sorted
        if s < 0:
            if left == 0:
                out.append(tuple(reversed(w)))
            return
        for l in range(max(0, left - s * (d - 1)), min(d - 1, left) + 1):
            rec(s - 1, left - l, w + [l])

    rec(n - 1, total, [])
    return out


def host_sector_csr(n, d, total, pairs, singles):
    """Independent assembly on the enumerated sector (dict lookup of the target words, terms merged by summation)."""
    words = sector_words(n, d, total)
    index = {w: k for k, w in enumerate(words)}
    rows, cols, vals = [], [], []
    mats = [(i, j, np.asarray(M).reshape(d * d, d * d)) for i, j, M in pairs]
    nz = [[np.nonzero(M[:, c])[0] for c in range(d * d)] for _, _, M in mats]
    for k, w in enumerate(words):
        rows.append(k); cols.append(k); vals.append(sum(dg[w[s]] for s, dg in singles) if singles else 0.0)
        for (i, j, M), z in zip(mats, nz):
            cin = w[i] * d + w[j]
            for o in z[cin]:
                t = list(w)
                t[i], t[j] = o // d, o % d
                rows.append(index[tuple(t)]); cols.append(k); vals.append(M[o, cin])
    H = sp.coo_matrix((vals, (rows, cols)), shape=(len(words),) * 2, dtype=np.complex128).tocsr()
    H.sum_duplicates()
    return words, H


def random_pair(rng, d, real=False, p_zero=0.2):
    """A random Hermitian d^2 x d^2 matrix that conserves l_i + l_j (some entries exactly zero)."""
    M = np.zeros((d * d, d * d), dtype=np.complex128)
    for r in range(d * d):
        for c in range(r, d * d):
            if r // d + r % d != c // d + c % d or rng.random() < p_zero:
                continue
            z = rng.normal() + (1j * rng.normal() if r != c and not real else 0.0)
            M[r, c] = z
            M[c, r] = np.conj(z)
    return M


def _both(n, d, total, pairs, singles=(), rows=None):
    A = q.csr_mat.qudit(n, d, total, pairs, singles, rows=rows, opts=q.make_opts(**PLAIN))
    M = q.csr_mat.qudit(n, d, total, pairs, singles, rows=rows, matrix_free=True)
    return A, M


def _assert_same_handle_shape(A, M):
    assert M.dim == A.dim and M.ncols == A.ncols and M.row_offset == A.row_offset and M.nnz == A.nnz
    assert M.info().kernel == _lib.KERNEL_MATRIX_FREE
    assert 0 < M.info().bytes_matrix < 4 << 20


def _assert_spmv_matches(A, M, seed, want=None):
    """y = alpha H x + beta y + gamma x with both reductions, matrix-free against stored (and against `want`(x), if given):
    vectors to 1e-13 of |y|_inf, reductions to 1e-12 relative."""
    n = A.dim
    x, y0 = _rand(n, seed), _rand(n, seed + 1)
    va, vm = A.vec(2), M.vec(2)
    for alpha, beta, gamma in EPILOGUES:
        for v in (va, vm):
            v.upload(x, 0)
            v.upload(y0, n)
        da, na = A.spmv(va.at(0), va.at(n), alpha, beta, gamma, want_red=True)
        dm, nm = M.spmv(vm.at(0), vm.at(n), alpha, beta, gamma, want_red=True)
        ya, ym = va.download(n, n), vm.download(n, n)
        scale = max(np.abs(ya).max(), 1e-300)
        assert np.abs(ym - ya).max() <= 1e-13 * scale, (alpha, beta, gamma, np.abs(ym - ya).max() / scale)
        assert abs(da - dm) <= 1e-12 * max(abs(da), 1.0) and abs(na - nm) <= 1e-12 * max(na, 1e-300)
        if want is not None:
            yw = alpha * want(x) + beta * y0 + gamma * x
            assert np.abs(ym - yw).max() <= 1e-13 * max(np.abs(yw).max(), 1e-300) * 8      # the numpy sum rounds on its own
    va.free()
    vm.free()


@pytest.mark.parametrize("name", ["spin1_chain", "bose_hubbard_3x3"])
def test_reference_models(name):
    if name == "spin1_chain":
        mk = lambda **kw: q.csr_mat.spin_heisenberg(10, 1, 0, chain(10), **kw)
    else:
        mk = lambda **kw: q.csr_mat.bose_hubbard(9, 9, 2, square_bonds(3, 3), t=1.0, U=1.1, **kw)
    A, M = mk(opts=q.make_opts(**PLAIN)), mk(matrix_free=True)
    _assert_same_handle_shape(A, M)
    if name == "spin1_chain":
        assert M.dim == 8953
    _assert_spmv_matches(A, M, 61)
    x = _rand(A.dim, 7)
    ya, ym = np.empty_like(x), np.empty_like(x)
    A.MultMv(x, ya)
    M.MultMv(x, ym)                                                             # the host seam
    assert np.abs(ym - ya).max() <= 1e-13 * np.abs(ya).max()
    M.MultMv2(x, ym)
    assert np.abs(ym - 2 * ya).max() <= 2e-13 * np.abs(ya).max()
    ra, rm = q.locate_E0_lanczos(A, nev=1, ncv=1), q.locate_E0_lanczos(M, nev=1, ncv=1)
    assert abs(rm.E0 - refmodels.KNOWN[name]["E0"]) < 1e-8
    assert abs(ra.steps["E0"] - rm.steps["E0"]) <= 1
    hv = np.empty(A.dim, dtype=np.complex128)
    A.MultMv(rm.eigenvecs, hv)
    assert np.linalg.norm(hv - rm.E0 * rm.eigenvecs) < 1e-8
    assert M.stats().n_spmv_real > 0
    nconv, w, _ = q.iram(A.dim, M, None, 1, 16, 300, "sr")
    assert abs(w[0] - ra.E0) < 1e-9
    with pytest.raises(_lib.QbhError):
        M.download()


def _random_terms(rng, n, d, n_pairs, real=False):
    """Random long-range pairs, every matrix distinct: about half given as (j, i), the pair (0, n-1) always, the first pair given
    twice (the two matrices must merge), single-site diagonals on most sites."""
    all_pairs = [(i, j) for i in range(n) for j in range(i + 1, n) if (i, j) != (0, n - 1)]
    pick = rng.choice(len(all_pairs), size=min(len(all_pairs), n_pairs - 1), replace=False)
    pairs = []
    for i, j in [(0, n - 1)] + [all_pairs[k] for k in pick]:
        if rng.random() < 0.5:
            i, j = j, i
        pairs.append((i, j, random_pair(rng, d, real)))
    pairs.append((pairs[1][1], pairs[1][0], random_pair(rng, d, real)))
    singles = [(s, rng.normal(size=d)) for s in range(n) if rng.random() < 0.7]
    return pairs, singles


# d = 8, n = 12 with 30 site pairs, each with a matrix of its own (the stored reference allows 240 entries per row, so at most
# 34 such pairs): a class holds d^2 = 64 rows of up to 7 off-diagonal entries, stored as 7 slots x 64 entries x 20 bytes + 512
# bytes of diagonal = 9.3 KB, so 30 classes take about 280 KB and cannot sit beside the counting table in the 150 KB LDS
# budget: the term tables are read from global memory.  The other cases (at most 2 n classes; for d = 8, n = 5: 10 classes,
# 93 KB) keep them in LDS.
@pytest.mark.parametrize("d,n,n_pairs,totals", [(2, 12, 24, (0, 1, 6)), (3, 8, 16, (0, 1, 8, 15)), (4, 6, 12, (0, 2, 9)),
                                                (5, 5, 10, (0, 1, 10)), (8, 5, 10, (0, 2, 17, 18)), (8, 12, 30, (0, 1, 4))])
def test_random_complex_operators(d, n, n_pairs, totals):
    rng = np.random.default_rng(4000 + 10 * d + n)
    pairs, singles = _random_terms(rng, n, d, n_pairs)
    assert len({(min(i, j), max(i, j)) for i, j, _ in pairs}) == n_pairs
    assert n * (d - 1) // 2 in totals or (d, n) == (8, 12)
    small = False
    for total in totals:
        words, H = host_sector_csr(n, d, total, pairs, singles)
        A, M = _both(n, d, total, pairs, singles)
        assert M.dim == len(words) == qudit.qudit_dim(n, d, total)
        small = small or 1 < M.dim < 64
        _assert_same_handle_shape(A, M)
        _assert_spmv_matches(A, M, 100 + total, want=lambda x: H @ x)
        if M.dim > 20:
            q.locate_E0_lanczos(M, nev=1, ncv=0, maxit=12)
        assert M.stats().n_spmv_real == 0                                      # complex values: never the real path
    assert totals[0] == 0 and small


@pytest.mark.parametrize("d,n,total,dim", [(3, 20, 2, 210), (5, 21, 2, 231), (8, 21, 3, 1771)])
def test_wide_words_real_operators(d, n, total, dim):
    """40-, 63- and 63-bit words: a 32-bit word, shift or mask anywhere loses the upper sites."""
    rng = np.random.default_rng(5000 + d)
    pairs, singles = _random_terms(rng, n, d, 29, real=True)
    pairs.append((n - 2, n - 1, random_pair(rng, d, True)))
    words, H = host_sector_csr(n, d, total, pairs, singles)
    A, M = _both(n, d, total, pairs, singles)
    assert M.dim == dim == len(words)
    _assert_same_handle_shape(A, M)
    _assert_spmv_matches(A, M, 9, want=lambda x: H @ x)
    w = np.linalg.eigvalsh(H.toarray())
    res = q.locate_E0_lanczos(M, nev=1, ncv=1)                                  # the drivers take the real path
    assert abs(res.E0 - w[0]) < 1e-9 * max(1.0, abs(w[0]))
    assert M.stats().n_spmv_real > 0


def test_real_operator_with_tables_in_global_memory():
    """The 30-class operator of test_random_complex_operators with real matrices: the real fast path on the global-table kernel."""
    rng = np.random.default_rng(77)
    d, n, total = 8, 12, 4
    pairs, singles = _random_terms(rng, n, d, 30, real=True)
    A, M = _both(n, d, total, pairs, singles)
    _assert_same_handle_shape(A, M)
    _assert_spmv_matches(A, M, 3)
    ra, rm = q.locate_E0_lanczos(A, nev=1, ncv=1), q.locate_E0_lanczos(M, nev=1, ncv=1)
    assert abs(ra.E0 - rm.E0) <= 1e-10 * abs(ra.E0)
    assert M.stats().n_spmv_real > 0 and A.stats().n_spmv_real == 0


def test_d2_is_the_heisenberg_operator():
    L, ndn = 16, 8
    bonds = lattices.chain(L)
    A = q.csr_mat.heisenberg(L, ndn, bonds, J=1.0, opts=q.make_opts(**PLAIN))
    B = q.csr_mat.heisenberg(L, ndn, bonds, J=1.0, matrix_free=True)
    M = q.csr_mat.qudit(L, 2, ndn, qudit.heisenberg_terms(0.5, bonds), matrix_free=True)
    assert M.dim == A.dim == B.dim == 12870 and M.nnz == A.nnz
    _assert_spmv_matches(A, M, 21)
    _assert_spmv_matches(B, M, 23)
    _, H = host_sector_csr(L, 2, ndn, qudit.heisenberg_terms(0.5, bonds), [])
    x = _rand(A.dim, 5)
    y = np.empty_like(x)
    M.MultMv(x, y)
    want = H @ x
    assert np.abs(y - want).max() <= 8e-13 * np.abs(want).max()


def test_grid_stride_loop_and_tail():
    """dim 1,787,607 = 3 x 595,869: above one resident grid (256 CUs x 4 workgroups x 512 lanes = 524,288) and odd."""
    L = 15
    A = q.csr_mat.spin_heisenberg(L, 1, 0, chain(L), opts=q.make_opts(**PLAIN))
    M = q.csr_mat.spin_heisenberg(L, 1, 0, chain(L), matrix_free=True)
    assert M.dim == A.dim == 1787607 and M.nnz == A.nnz
    n = A.dim
    x = _rand(n, 15)
    va, vm = A.vec(2), M.vec(2)
    va.upload(x, 0)
    vm.upload(x, 0)
    da, na = A.spmv(va.at(0), va.at(n), want_red=True)
    dm, nm = M.spmv(vm.at(0), vm.at(n), want_red=True)
    ya, ym = va.download(n, n), vm.download(n, n)
    assert np.abs(ym - ya).max() <= 1e-13 * np.abs(ya).max()
    assert abs(da - dm) <= 1e-12 * abs(da) and abs(na - nm) <= 1e-12 * na


def test_row_shards_reproduce_the_rows_of_the_whole_operator():
    n, d, total = 8, 4, 11
    pairs, singles = qudit.bose_hubbard_terms(3, chain(n) + [(0, 4)], 0.7, 1.3, 0.2)
    whole = q.csr_mat.qudit(n, d, total, pairs, singles, matrix_free=True)
    dim = whole.dim
    x, y0 = _rand(dim, 31), _rand(dim, 32)
    vw = whole.vec(2)
    vw.upload(x, 0)
    vw.upload(y0, dim)
    whole.spmv(vw.at(0), vw.at(dim), 0.6, -1.2, 0.3)
    y = vw.download(dim, dim)
    nnz = 0
    for cuts in ([0, dim // 2, dim], [0, 17, 17 + 63, dim // 3 + 1, dim - 5, dim]):
        for r0, r1 in zip(cuts[:-1], cuts[1:]):
            S = q.csr_mat.qudit(n, d, total, pairs, singles, rows=(r0, r1), matrix_free=True)
            i = S.info()
            assert S.dim == i.nrows == r1 - r0 and i.row_offset == r0 and i.ncols == dim and i.kernel == _lib.KERNEL_MATRIX_FREE
            T = q.csr_mat.qudit(n, d, total, pairs, singles, rows=(r0, r1), opts=q.make_opts(**PLAIN))
            assert S.nnz == T.nnz
            nnz += S.nnz
            vx, vy = q.DeviceVec(S, dim), q.DeviceVec(S, r1 - r0)
            vx.upload(x)
            vy.upload(y0[r0:r1])
            S.spmv(vx.ptr, vy.ptr, 0.6, -1.2, 0.3)
            got = vy.download()
            assert np.array_equal(got.view(np.uint64), y[r0:r1].view(np.uint64)), (r0, r1)
            vx.free()
            vy.free()
    assert nnz == 2 * whole.nnz


def test_packed_real_drivers():
    """qbh_lanczos_real_dev (with a continuation after 40 steps) and qbh_eigenvec_cg_real_dev on the matrix-free spin-1 chain
    against the complex interface on the stored operator."""
    L = 10
    A = q.csr_mat.spin_heisenberg(L, 1, 0, chain(L), opts=q.make_opts(**PLAIN))
    M = q.csr_mat.spin_heisenberg(L, 1, 0, chain(L), matrix_free=True)
    n, maxit = A.dim, 400
    ref = q.locate_E0_lanczos(A, nev=1, ncv=1, maxit=maxit)
    vc = A.vec(2)
    A.randomize(vc.at(0), 1)
    hc = np.zeros(2 * maxit)
    mc = q.lanczos(0, maxit - 1, maxit, n, A, None, hc, "sr_val0", device_v=vc)
    buf = q.DeviceVec(M, 2 * n + 2)                            # 4 slots of n packed doubles (n is odd): v, r, p, pp
    at = lambda j: C.c_void_p(buf.ptr.value + 8 * n * j)
    lan = type("V", (), {"ptr": at(0)})()                      # slots 0, 1 are the two Lanczos vectors
    _lib.check(_lib.lib().qbh_vec_randomize_real(M.handle, at(0), C.c_uint32(1)), "qbh_vec_randomize_real")
    hr = np.zeros(2 * maxit)
    m1 = q.lanczos_real(0, 40, maxit, M, lan, hr)
    assert m1 == 40
    m2 = q.lanczos_real(m1, maxit - 1 - m1, maxit, M, lan, hr, state=q.lanczos_real.last["state"])
    assert abs(m2 - mc) <= 1
    assert np.allclose(hr[maxit:maxit + 30], hc[maxit:maxit + 30], rtol=1e-9, atol=1e-11)     # a_0 .. a_29
    assert np.allclose(hr[1:31], hc[1:31], rtol=1e-9, atol=1e-11)                               # b_1 .. b_30
    ritz, _ = q.hess_eigen(hr, maxit, m2, "sr")
    assert abs(ritz[0] - ref.E0) <= 1e-11 * abs(ref.E0)
    assert abs(ritz[0] - refmodels.KNOWN["spin1_chain"]["E0"]) < 1e-8
    _lib.check(_lib.lib().qbh_vec_randomize_real(M.handle, at(0), C.c_uint32(1)), "qbh_vec_randomize_real")
    mcg, accu = q.eigenvec_CG_real(maxit, 0, M, ritz[0], at(0), at(1), at(2), at(3))
    assert accu < 2e-12
    vec = buf.download(0, (n + 1) // 2).view(np.float64)[:n]
    assert abs(np.linalg.norm(vec) - 1.0) < 1e-10
    assert abs(abs(np.dot(vec, ref.eigenvecs.real)) - 1.0) < 1e-8
    assert M.stats().n_spmv_real > 0
