"""qbh_mf_qudit_repr on the device: the momentum sector of a d-level operator applied from its basis, against the stored
sector of qbh_gen_qudit_repr (plain options) and against the explicit projection B^dag H B x, with B the normalised momentum
states written out word by word here and H the full-sector operator of qbh_gen_qudit.  Vectors agree with the stored product to
1e-13 |y|_inf (the stored row sums merged duplicates in another order), reductions to 1e-12 relative, and the numpy product
gets 8 times the vector tolerance, as in tests/test_gpu_qudit_mf.py."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import scipy.sparse as sp

import quantum_basis_amd as q
from quantum_basis_amd import _lib, qudit

pytestmark = pytest.mark.gpu

PLAIN = dict(kron_split=0, sector_cut=-1, value_dict=0, real_fast_path=0)
EPILOGUES = [(1.0, 0.0, 0.0), (1.0, 1.0, 0.0), (0.6, -1.2, 0.0), (1.0, 0.0, -3.0)]
FAKE = 100.0
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "spin1_chain12_momentum.json")
LDS_BUDGET = 150 * 1024                      # translation tables + counting table beyond this are read from global memory


def chain(L):
    return [(i, (i + 1) % L) for i in range(L)]


def chain_group(L, m):
    """Translations of a ring and the characters exp(-i k t) of k = 2 pi m / L."""
    perms = [[(s + t) % L for s in range(L)] for t in range(L)]
    return perms, np.exp(-2j * np.pi * m * np.arange(L) / L)


def torus_group(Lx, Ly, mx, my):
    site = lambda x, y: (x % Lx) + Lx * (y % Ly)
    perms, chars = [], []
    for ty in range(Ly):
        for tx in range(Lx):
            perms.append([site(x + tx, y + ty) for y in range(Ly) for x in range(Lx)])
            chars.append(np.exp(-2j * np.pi * (mx * tx / Lx + my * ty / Ly)))
    return perms, np.array(chars)


def square_bonds(Lx, Ly):
    site = lambda x, y: (x % Lx) + Lx * (y % Ly)
    return [b for x in range(Lx) for y in range(Ly) for b in ((site(x, y), site(x + 1, y)), (site(x, y), site(x, y + 1)))]


def _rand(n, seed):
    rng = np.random.default_rng(seed)
    return (rng.normal(size=n) + 1j * rng.normal(size=n)).astype(np.complex128)


def sector_words(n, d, total):
    """The sector in the generator's order (ascending sum l_s d^s) as an (N, n) array of levels."""
    out = []

    def rec(s, left, w):                        # sites n-1 .. 0, most significant first, levels ascending: already sorted
        if s < 0:
            if left == 0:
                out.append(w[::-1])
            return
        for l in range(max(0, left - s * (d - 1)), min(d - 1, left) + 1):
            rec(s - 1, left - l, w + [l])

    rec(n - 1, total, [])
    return np.array(out, dtype=np.int64).reshape(-1, n)


class Momentum:
    """The explicit momentum states of one sector (as in tests/test_gpu_qudit_repr.py, vectorised): B[:, a] =
    (|G| |S_a|)^(-1/2) sum_g chi(g) T_g |a> for every orbit representative a (the smallest word of its orbit), ascending;
    zero[a] marks the states that vanish at this momentum."""

    def __init__(self, n, d, total, perms, chars):
        W = sector_words(n, d, total)
        N, G = len(W), len(perms)
        assert d ** n < 2 ** 62
        pw = np.array([d ** s for s in range(n)], dtype=np.int64)
        key = W @ pw
        assert np.all(np.diff(key) > 0)
        img = np.empty((G, N), dtype=np.int64)
        for g, p in enumerate(perms):           # T_g moves the level of site s to site p[s]
            img[g] = np.searchsorted(key, W @ pw[np.asarray(p)])
        me = np.arange(N)
        rep = img.min(axis=0) == me
        stab = (img == me[None, :]).sum(axis=0)
        ridx = np.flatnonzero(rep)
        cols = np.tile(np.arange(len(ridx)), G)
        rows = img[:, ridx].reshape(-1)
        vals = (np.asarray(chars)[:, None] / np.sqrt(G * stab[ridx])[None, :]).reshape(-1)
        B = sp.coo_matrix((vals, (rows, cols)), shape=(N, len(ridx)), dtype=np.complex128).tocsc()
        B.sum_duplicates()
        norm = np.sqrt(np.asarray(B.multiply(B.conj()).sum(axis=0)).real.reshape(-1))
        self.zero = norm < 1e-9
        self.B = B.multiply(~self.zero[None, :]).tocsc()
        self.dim = len(ridx)
        self.reps = W[ridx]


def full_csr(A):
    ia, ja, val = A.download()
    return sp.csr_matrix((val, ja, ia), shape=(A.dim, A.dim))


def projection(n, d, total, pairs, singles, perms, chars):
    """x -> B^dag H B x, plus the fake diagonal on the rows whose state vanishes; and the momentum states."""
    H = full_csr(q.csr_mat.qudit(n, d, total, pairs, singles, opts=q.make_opts(**PLAIN)))
    mb = Momentum(n, d, total, perms, chars)
    BH = mb.B.conj().T.tocsr()
    fake = np.where(mb.zero, FAKE + np.arange(mb.dim) / mb.dim, 0.0)
    return (lambda x: BH @ (H @ (mb.B @ x)) + fake * x), mb


def stored(n, d, total, perms, chars, pairs, singles=()):
    return q.csr_mat.qudit_repr(n, d, total, perms, chars, pairs, singles, fake_pos=FAKE, opts=q.make_opts(**PLAIN))


def matrix_free(n, d, total, perms, chars, pairs, singles=(), rows=None):
    return q.csr_mat.qudit_repr(n, d, total, perms, chars, pairs, singles, fake_pos=FAKE, matrix_free=True, rows=rows)


def table_bytes(n, d, total, n_trans):
    bits = 1 if d <= 2 else 2 if d <= 4 else 3
    per = 6 // bits
    return (n_trans * ((n + per - 1) // per) * 64 + n * (total + 1)) * 8


def _assert_spmv_matches(A, M, seed, want=None, epilogues=EPILOGUES):
    """y = alpha H x + beta y + gamma x with both reductions: matrix-free against stored (A, may be None) and against
    `want`(x) (may be None).  Every figure is printed before it is asserted."""
    n = M.dim
    x, y0 = _rand(n, seed), _rand(n, seed + 1)
    vm = M.vec(2)
    va = A.vec(2) if A is not None else None
    for alpha, beta, gamma in epilogues:
        for v in (va, vm):
            if v is not None:
                v.upload(x, 0)
                v.upload(y0, n)
        dm, nm = M.spmv(vm.at(0), vm.at(n), alpha, beta, gamma, want_red=True)
        ym = vm.download(n, n)
        if A is not None:
            da, na = A.spmv(va.at(0), va.at(n), alpha, beta, gamma, want_red=True)
            ya = va.download(n, n)
            scale = max(np.abs(ya).max(), 1e-300)
            print("mf-stored", (alpha, beta, gamma), np.abs(ym - ya).max() / scale, abs(da - dm), abs(na - nm) / max(na, 1e-300))
            assert np.abs(ym - ya).max() <= 1e-13 * scale
            assert abs(da - dm) <= 1e-12 * max(abs(da), 1.0) and abs(na - nm) <= 1e-12 * max(na, 1e-300)
        if want is not None:
            yw = alpha * want(x) + beta * y0 + gamma * x
            scale = max(np.abs(yw).max(), 1e-300)
            print("mf-numpy", (alpha, beta, gamma), np.abs(ym - yw).max() / scale)
            assert np.abs(ym - yw).max() <= 8 * 1e-13 * scale
    vm.free()
    if va is not None:
        va.free()


def spin1_terms(L, K=0.0):
    return qudit.heisenberg_terms(1, chain(L), K=K)


# ---- 1 ----
@pytest.mark.parametrize("m", range(8))
def test_every_momentum_of_the_spin1_ring_L8(m):
    L = 8
    perms, chars = chain_group(L, m)
    pairs = spin1_terms(L)
    want, mb = projection(L, 3, L, pairs, [], perms, chars)
    A, M = stored(L, 3, L, perms, chars, pairs), matrix_free(L, 3, L, perms, chars, pairs)
    assert M.dim == A.dim == mb.dim
    i0 = int(np.flatnonzero((mb.reps == 1).all(axis=1))[0])      # the word 11111111: every translation fixes it
    if m != 0:
        assert mb.zero[i0]                       # its character sum vanishes: the info byte carries the zero-norm bit and the
        e = np.zeros(M.dim, dtype=np.complex128)    # row is the fake diagonal alone
        e[i0] = 1.0
        y = np.empty_like(e)
        M.MultMv(e, y)
        assert abs(y[i0] - (FAKE + i0 / M.dim)) < 1e-12 and not np.delete(y, i0).any()
    else:
        assert not mb.zero.any()
    _assert_spmv_matches(A, M, 10 + m, want)


# ---- 2 ----
def random_pair(rng, d):
    M = rng.normal(size=(d * d, d * d)) + 1j * rng.normal(size=(d * d, d * d))
    q_ = np.add.outer(np.arange(d * d) // d + np.arange(d * d) % d, np.zeros(d * d, dtype=int))
    M[q_ != q_.T] = 0.0                                # charge-conserving
    return 0.5 * (M + M.conj().T)


# (d, L) as the sizes at which the word packing changes (1, 2, 3 bits per site), mid charge, a momentum that is neither 0 nor
# pi; the nearest- and next-nearest-neighbour bonds carry different matrices.  The kernel keeps the translation tables
# (n_trans x n_chunks x 64 words) and the counting table in LDS while they fit 150 KB: for these four rings they take at most
# 4.6 KB whatever the terms are, so all four run the LDS path.  The global-memory path needs a large group: the ring of 44
# spin-1/2 sites has 44 x 8 x 64 words = 180 KB of tables, and its 3-magnon sector is 13244 words.
@pytest.mark.parametrize("d,L,total,m", [(2, 8, 4, 3), (3, 6, 6, 1), (5, 4, 8, 1), (8, 4, 14, 3), (2, 44, 3, 7)])
def test_random_complex_terms_on_both_table_paths(d, L, total, m):
    rng = np.random.default_rng(700 + 10 * d + L)
    M1, M2 = random_pair(rng, d), random_pair(rng, d)
    pairs = [(i, (i + 1) % L, M1) for i in range(L)] + [(i, (i + 2) % L, M2) for i in range(L)]
    dg = rng.normal(size=d)
    singles = [(s, dg) for s in range(L)]
    perms, chars = chain_group(L, m)
    want, mb = projection(L, d, total, pairs, singles, perms, chars)
    A, M = stored(L, d, total, perms, chars, pairs, singles), matrix_free(L, d, total, perms, chars, pairs, singles)
    assert M.dim == A.dim == mb.dim
    in_lds = table_bytes(L, d, total, L) <= LDS_BUDGET
    assert in_lds == (L != 44)
    assert M.info().kron_table_kernel == (1 if in_lds else 0)          # which table path the handle runs
    _assert_spmv_matches(A, M, 200 + d, want)
    assert M.stats().n_spmv_real == 0                                    # complex values: never the real path


# ---- 3 ----
@pytest.mark.parametrize("k", [(1, 2), (0, 0)])
def test_bose_hubbard_on_the_3x3_torus(k):
    Lx = Ly = 3
    n, N, nmax = 9, 4, 3
    perms, chars = torus_group(Lx, Ly, *k)
    assert len(perms) == 9
    pairs, _ = qudit.bose_hubbard_terms(nmax, square_bonds(Lx, Ly), 1.0, 1.1, 0.2)
    nn = np.arange(nmax + 1, dtype=np.float64)
    singles = [(s, 0.55 * nn * (nn - 1) - 0.2 * nn) for s in range(n)]
    want, mb = projection(n, nmax + 1, N, pairs, singles, perms, chars)
    A, M = stored(n, nmax + 1, N, perms, chars, pairs, singles), matrix_free(n, nmax + 1, N, perms, chars, pairs, singles)
    assert M.dim == A.dim == mb.dim
    _assert_spmv_matches(A, M, 31, want)


# ---- 4 ----
def test_words_wider_than_32_bits():
    """Spin-1 ring of 20 sites, charge 3, m = 7: 40-bit words, C(22, 3) - 20 = 1520 of them (no site holds all three quanta)."""
    L, total, m = 20, 3, 7
    perms, chars = chain_group(L, m)
    pairs = spin1_terms(L, K=0.25)
    want, mb = projection(L, 3, total, pairs, [], perms, chars)
    assert len(sector_words(L, 3, total)) == 1520
    A, M = stored(L, 3, total, perms, chars, pairs), matrix_free(L, 3, total, perms, chars, pairs)
    assert M.dim == A.dim == mb.dim
    _assert_spmv_matches(A, M, 41, want)


# ---- 5 ----
@pytest.mark.parametrize("L,n_dn,m", [(12, 6, 0), (24, 11, 5)])
def test_d2_is_the_spin_half_sector(L, n_dn, m):
    perms, chars = chain_group(L, m)
    B = q.csr_mat.heisenberg_repr(L, n_dn, chain(L), perms, chars, J=1.0, fake_pos=FAKE, opts=q.make_opts(**PLAIN))
    M = matrix_free(L, 2, n_dn, perms, chars, qudit.heisenberg_terms(0.5, chain(L)))
    assert M.dim == B.dim
    _assert_spmv_matches(B, M, 51)


# ---- 6 ----
def test_more_rows_than_one_pass_of_the_resident_grid():
    """Spin-1 chain L = 18, S^z = 0, m = 9: about 2.45e6 rows against at most 256 CUs x 2 workgroups x 1024 lanes."""
    L = 18
    perms, chars = chain_group(L, 9)
    pairs = spin1_terms(L)
    A, M = stored(L, 3, L, perms, chars, pairs), matrix_free(L, 3, L, perms, chars, pairs)
    assert M.dim == A.dim and 2.4e6 < M.dim < 2.5e6 and M.dim > 256 * 2 * 1024
    _assert_spmv_matches(A, M, 61, epilogues=EPILOGUES[2:3])


# ---- 7 ----
def test_ragged_row_shards_are_bit_identical_to_the_whole_operator():
    L, m = 12, 3
    perms, chars = chain_group(L, m)
    pairs, singles = spin1_terms(L, K=0.2), qudit.single_ion(1, L, 0.3)
    whole = matrix_free(L, 3, L, perms, chars, pairs, singles)
    dim = whole.dim
    x, y0 = _rand(dim, 71), _rand(dim, 72)
    vw = whole.vec(2)
    vw.upload(x, 0)
    vw.upload(y0, dim)
    whole.spmv(vw.at(0), vw.at(dim), 0.6, -1.2, 0.3)
    y = vw.download(dim, dim)
    cuts = [0, 1, dim // 5 + 7, dim - 129, dim]              # a shard of one row, uneven cuts, a shard that ends at dim
    nnz = 0
    for r, (r0, r1) in enumerate(zip(cuts[:-1], cuts[1:])):
        S = matrix_free(L, 3, L, perms, chars, pairs, singles, rows=(r0, r1))
        T = q.csr_mat.qudit_repr(L, 3, L, perms, chars, pairs, singles, fake_pos=FAKE, shard=(r, len(cuts) - 1), row_cuts=cuts,
                                 opts=q.make_opts(**PLAIN))
        i, j = S.info(), T.info()
        assert (i.nrows, i.row_offset, i.ncols) == (j.nrows, j.row_offset, j.ncols) == (r1 - r0, r0, dim)
        assert S.dim == T.dim == r1 - r0 and i.kernel == _lib.KERNEL_MATRIX_FREE and S.nnz >= T.nnz
        nnz += S.nnz
        vx, vy = q.DeviceVec(S, dim), q.DeviceVec(S, r1 - r0)
        vx.upload(x)
        vy.upload(y0[r0:r1])
        S.spmv(vx.ptr, vy.ptr, 0.6, -1.2, 0.3)
        got = vy.download()
        assert np.array_equal(got, y[r0:r1]), (r0, r1)
        vx.free()
        vy.free()
    assert nnz == whole.nnz


# ---- 8 ----
def all_to_all_spin1(L):
    """Every pair of a ring of L spin-1 sites, bilinear + biquadratic, couplings that depend on the ring distance only."""
    dist = lambda i, j: min((j - i) % L, (i - j) % L)
    pairs = []
    for i in range(L):
        for j in range(i + 1, L):
            r = dist(i, j)
            pairs += qudit.heisenberg_terms(1, [(i, j)], J=1.0 / r, K=0.3 / r ** 2)
    return pairs


# The 12-site operator at S^z = 0 (73789 words); its merged terms count 66 x 2 + 1 = 133 entries per row (a merged spin-1 pair
# has at most 2 off-diagonal entries in a row), which the stored form still takes.  The 14-site operator counts 91 x 2 + 1 =
# 183 > 160: no stored handle exists for it; it is checked in the small sector of charge 3 (560 words).
@pytest.mark.parametrize("L,total,m", [(12, 12, 0), (12, 12, 5), (14, 3, 0), (14, 3, 5)])
def test_all_to_all_operator_beyond_the_row_limit_of_the_stored_form(L, total, m):
    perms, chars = chain_group(L, m)
    pairs = all_to_all_spin1(L)
    want, mb = projection(L, 3, total, pairs, [], perms, chars)
    if L == 14:
        with pytest.raises(_lib.QbhError):
            stored(L, 3, total, perms, chars, pairs)
    M = matrix_free(L, 3, total, perms, chars, pairs)
    assert M.dim == mb.dim
    _assert_spmv_matches(None, M, 81 + m, want)


# ---- 9 ----
def test_solvers_and_real_drivers_on_the_reference_sector_energies():
    ref = json.load(open(GOLDEN))
    L = ref["L"]
    assert L == 12
    for m in range(5):
        perms, chars = chain_group(L, m)
        M = q.csr_mat.spin_heisenberg_repr(L, 1, 0, chain(L), perms, chars, matrix_free=True)
        assert M.info().kernel == _lib.KERNEL_MATRIX_FREE
        n, maxit = M.dim, 400
        v = M.vec(2)
        M.randomize(v.at(0), 1)
        h = np.zeros(2 * maxit)
        steps = q.lanczos(0, maxit - 1, maxit, n, M, None, h, "sr_val0", device_v=v)
        ritz, _ = q.hess_eigen(h, maxit, steps, "sr")
        print("m", m, "E0", ritz[0], "ref", ref["E0_by_m"][str(m)])
        assert abs(ritz[0] - ref["E0_by_m"][str(m)]) < ref["tolerance"] == 1e-8
        v.free()
        if m == 0:
            A = q.csr_mat.spin_heisenberg_repr(L, 1, 0, chain(L), perms, chars, opts=q.make_opts(**PLAIN))
            buf = q.DeviceVec(M, 2 * n + 2)                   # 4 slots of n packed doubles: v, r, p, pp
            at = lambda j: C.c_void_p(buf.ptr.value + 8 * n * j)
            lan = type("V", (), {"ptr": at(0)})()
            _lib.check(_lib.lib().qbh_vec_randomize_real(M.handle, at(0), C.c_uint32(1)), "qbh_vec_randomize_real")
            hr = np.zeros(2 * maxit)
            mr = q.lanczos_real(0, maxit - 1, maxit, M, lan, hr)              # accepted: values_real
            er = q.hess_eigen(hr, maxit, mr, "sr")[0][0]
            assert abs(er - ref["E0_by_m"]["0"]) < ref["tolerance"]
            assert M.stats().n_spmv_real > 0
            _lib.check(_lib.lib().qbh_vec_randomize_real(M.handle, at(0), C.c_uint32(1)), "qbh_vec_randomize_real")
            mcg, accu = q.eigenvec_CG_real(maxit, 0, M, er, at(0), at(1), at(2), at(3))
            vec = buf.download(0, (n + 1) // 2).view(np.float64)[:n].astype(np.complex128)
            res_mf = q.locate_E0_lanczos(A, nev=1, ncv=1)                     # the stored run and its eigenvector
            hv = np.empty(n, dtype=np.complex128)
            A.MultMv(vec, hv)
            r_mf = np.linalg.norm(hv - er * vec)
            vs = np.asarray(res_mf.eigenvecs, dtype=np.complex128).reshape(-1)[:n]
            A.MultMv(vs, hv)
            r_st = np.linalg.norm(hv - res_mf.E0 * vs)
            print("residual matrix-free", r_mf, "stored", r_st, "accu", accu)
            assert abs(r_mf - r_st) <= 1e-10
            buf.free()
        if m == 1:
            buf = q.DeviceVec(M, 2 * n + 2)
            lan = type("V", (), {"ptr": buf.ptr})()
            with pytest.raises(_lib.QbhError):                                # complex characters: the real driver is refused
                q.lanczos_real(0, 10, maxit, M, lan, np.zeros(2 * maxit))
            assert M.stats().n_spmv_real == 0
            buf.free()


# ---- 10 ----
def test_handle_shape():
    L, m = 10, 3
    perms, chars = chain_group(L, m)
    pairs = spin1_terms(L, K=0.2)
    A, M = stored(L, 3, L, perms, chars, pairs), matrix_free(L, 3, L, perms, chars, pairs)
    i = M.info()
    words = len(sector_words(L, 3, L))
    assert i.kernel == _lib.KERNEL_MATRIX_FREE and (i.nrows, i.ncols, i.row_offset) == (A.dim, A.dim, 0)
    assert 9 * M.dim <= i.bytes_matrix <= 9 * M.dim + (4 << 20) + 8 * (words // 4096 + 1)
    assert M.nnz >= A.nnz
    with pytest.raises(_lib.QbhError) as e:
        M.download()
    assert e.value.code == -9                                                 # QBH_EUNSUPP
    with pytest.raises(ValueError):
        q.csr_mat.qudit_repr(L, 3, L, perms, chars, pairs, matrix_free=True, shard=(0, 2))
    with pytest.raises(ValueError):
        q.csr_mat.qudit_repr(L, 3, L, perms, chars, pairs, matrix_free=True, row_cuts=[0, M.dim])
