"""The d-level sector generator qbh_gen_qudit and qbh_mopr_qudit_dev on the device, against independent host assemblies: the
reference's spin-1 chain and Bose-Hubbard examples entry by entry and by their asserted energies, qbh_gen_heisenberg bit for
bit at d = 2, random charge-conserving operators for d = 2..5, row shards, a full-size spin-1 chain (sampled rows), and the
operator x vector step against dense numpy operators."""
import itertools

import numpy as np
import pytest
import scipy.sparse as sp

import quantum_basis_amd as q
from quantum_basis_amd import qudit
import refmodels

pytestmark = pytest.mark.gpu

PLAIN = dict(kron_split=0, sector_cut=-1, value_dict=0, real_fast_path=0)


def chain(L):
    return [(i, (i + 1) % L) for i in range(L)]


def sector_words(n, d, total):
    """The sector in the generator's order: ascending sum l_s d^s (site n-1 most significant)."""
    ws = [w for w in itertools.product(range(d), repeat=n) if sum(w) == total]
    return sorted(ws, key=lambda w: sum(l * d ** s for s, l in enumerate(w)))


def host_sector_csr(n, d, total, pairs, singles):
    """Independent assembly on the enumerated sector (dict lookup of the target words, terms merged by summation)."""
    words = sector_words(n, d, total)
    index = {w: k for k, w in enumerate(words)}
    rows, cols, vals = [], [], []
    for k, w in enumerate(words):
        rows.append(k); cols.append(k); vals.append(sum(dg[w[s]] for s, dg in singles) if singles else 0.0)
        for i, j, M in pairs:
            M = np.asarray(M).reshape(d * d, d * d)
            a, b = (i, j)
            cin = w[a] * d + w[b]
            for o in range(d * d):
                if M[o, cin] != 0:
                    t = list(w)
                    t[a], t[b] = o // d, o % d
                    rows.append(index[tuple(t)]); cols.append(k); vals.append(M[o, cin])
    H = sp.coo_matrix((vals, (rows, cols)), shape=(len(words),) * 2, dtype=np.complex128).tocsr()
    H.sum_duplicates()
    return words, H


def assert_rows_match(A, H, r0=0, rtol=1e-13):
    """Downloaded rows of A against the host matrix H (diagonal always present, no other explicit zero)."""
    ia, ja, val = A.download()
    Hd = H.tocsr()
    for r in range(A.dim):
        c = ja[ia[r]:ia[r + 1]]
        v = val[ia[r]:ia[r + 1]]
        assert np.all(np.diff(c) > 0), r
        hr = Hd.getrow(r0 + r)
        want = dict(zip(hr.indices, hr.data))
        want.setdefault(r0 + r, 0.0)
        want = {k: x for k, x in want.items() if x != 0 or k == r0 + r}
        assert sorted(want) == list(c), (r, sorted(want), list(c))
        scale = max(1.0, np.abs(v).max())
        for k, x in zip(c, v):
            assert abs(x - want[k]) <= rtol * scale, (r, k, x, want[k])


def _perm_from_ref(n, d, total, level_tuple_in_ref_order):
    """Generator index of every refmodels state (refmodels: itertools.product order, site 0 most significant)."""
    gen = {w: k for k, w in enumerate(sector_words(n, d, total))}
    return np.array([gen[w] for w in level_tuple_in_ref_order], dtype=np.int64)


def _compare_ref_model(A, dim, ia, ja, val, perm):
    R = sp.csr_matrix((val, ja, ia), shape=(dim, dim))
    P = sp.csr_matrix((np.ones(dim), (perm, np.arange(dim))), shape=(dim, dim))
    G = (P @ R @ P.T).tocsr()
    G.sort_indices()
    gia, gja, gval = A.download()
    assert A.dim == dim
    assert np.array_equal(gia, G.indptr) and np.array_equal(gja, G.indices)
    assert np.allclose(gval, G.data, rtol=0, atol=1e-13)        # refmodels' 1e-300 diagonal fill is far below atol


def test_spin1_chain_and_bose_hubbard_match_refmodels_entry_by_entry():
    L = 10
    dim, ia, ja, val, _ = refmodels.spin1_chain(upper=False)
    ref_words = [tuple(1 - m for m in s) for s in itertools.product((1, 0, -1), repeat=L) if sum(s) == 0]
    A = q.csr_mat.spin_heisenberg(L, 1, 0, chain(L))
    _compare_ref_model(A, dim, ia, ja, val, _perm_from_ref(L, 3, L, ref_words))
    dim, ia, ja, val, _ = refmodels.bose_hubbard_3x3(upper=False)
    ref_words = [s for s in itertools.product(range(3), repeat=9) if sum(s) == 9]
    B = q.csr_mat.bose_hubbard(9, 9, 2, square_bonds(3, 3), t=1.0, U=1.1)
    _compare_ref_model(B, dim, ia, ja, val, _perm_from_ref(9, 3, 9, ref_words))


def square_bonds(Lx, Ly):
    site = lambda x, y: (x % Lx) + Lx * (y % Ly)
    return [b for x in range(Lx) for y in range(Ly) for b in ((site(x, y), site(x + 1, y)), (site(x, y), site(x, y + 1)))]


@pytest.mark.parametrize("plain", [False, True])
def test_known_answers_of_the_reference(plain):
    opts = q.make_opts(value_dict=0, real_fast_path=0) if plain else None
    A = q.csr_mat.spin_heisenberg(10, 1, 0, chain(10), opts=opts)
    res = q.locate_E0_lanczos(A, nev=2, ncv=2)
    assert abs(res.E0 - refmodels.KNOWN["spin1_chain"]["E0"]) < 1e-8
    assert abs(res.E1 - refmodels.KNOWN["spin1_chain"]["E1"]) < 1e-8
    B = q.csr_mat.bose_hubbard(9, 9, 2, square_bonds(3, 3), t=1.0, U=1.1, opts=opts)
    res = q.locate_E0_lanczos(B, nev=1, ncv=1)
    assert abs(res.E0 - refmodels.KNOWN["bose_hubbard_3x3"]["E0"]) < 1e-8


def _download_chunks(A, step):
    for r0 in range(0, A.dim, step):
        yield r0, A.download(r0, min(A.dim, r0 + step))


@pytest.mark.parametrize("n,n_dn,bonds", [(12, 5, [(0, 3), (3, 7), (7, 11), (1, 2), (2, 9), (9, 1), (4, 5), (5, 11), (6, 8), (8, 10), (10, 0), (3, 4)]),
                                          (28, 14, chain(28))])
def test_d2_is_qbh_gen_heisenberg(n, n_dn, bonds):
    opts = q.make_opts(**PLAIN)
    A = q.csr_mat.heisenberg(n, n_dn, bonds, opts=opts)
    B = q.csr_mat.qudit(n, 2, n_dn, qudit.heisenberg_terms(0.5, bonds), opts=q.make_opts(**PLAIN))
    assert A.dim == B.dim == qudit.qudit_dim(n, 2, n_dn) and A.nnz == B.nnz
    assert B.info().basis_internal == 0 and B.info().kron_minor == 0
    step = 1 << 22
    for r0, (ia, ja, val) in _download_chunks(A, step):
        ib, jb, vb = B.download(r0, min(A.dim, r0 + step))
        assert np.array_equal(ia, ib) and np.array_equal(ja, jb) and np.array_equal(val, vb), r0


def random_pair(rng, d):
    """A random Hermitian d^2 x d^2 matrix with complex entries that conserves l_i + l_j (some entries exactly zero)."""
    M = np.zeros((d * d, d * d), dtype=np.complex128)
    for r in range(d * d):
        for c in range(r, d * d):
            if r // d + r % d != c // d + c % d or rng.random() < 0.2:
                continue
            z = rng.normal() + (1j * rng.normal() if r != c else 0.0)
            M[r, c] = z
            M[c, r] = np.conj(z)
    return M


@pytest.mark.parametrize("d,n", [(2, 7), (3, 6), (4, 5), (5, 4)])
def test_random_operators_against_dense(d, n):
    rng = np.random.default_rng(1000 + 10 * d + n)
    all_pairs = [(i, j) for i in range(n) for j in range(i + 1, n)]
    pick = rng.choice(len(all_pairs), size=min(len(all_pairs), 2 * n), replace=False)
    pairs = []
    for k in pick:
        i, j = all_pairs[k]
        if rng.random() < 0.5:
            i, j = j, i                                     # given as (j, i): transposed by the generator
        pairs.append((i, j, random_pair(rng, d)))
    pairs.append((pairs[0][0], pairs[0][1], random_pair(rng, d)))          # a repeated pair is summed
    singles = [(s, rng.normal(size=d)) for s in range(n) if rng.random() < 0.7]
    for total in sorted({1, (n * (d - 1)) // 2, n * (d - 1) - 1}):
        words, H = host_sector_csr(n, d, total, pairs, singles)
        for plain in (True, False):
            A = q.csr_mat.qudit(n, d, total, pairs, singles, opts=q.make_opts(**PLAIN) if plain else None)
            assert A.dim == len(words)
            assert_rows_match(A, H, rtol=1e-13)
            x = (rng.normal(size=A.dim) + 1j * rng.normal(size=A.dim)).astype(np.complex128)
            y = np.empty_like(x)
            A.MultMv(x, y)
            want = H @ x
            assert np.abs(y - want).max() <= 1e-12 * max(1.0, np.abs(want).max())


def test_row_shards_concatenate_to_the_whole_operator():
    n, d, total = 8, 4, 11
    pairs, singles = qudit.bose_hubbard_terms(3, chain(n) + [(0, 4)], 0.7, 1.3, 0.2)
    whole = q.csr_mat.qudit(n, d, total, pairs, singles, opts=q.make_opts(**PLAIN))
    ia, ja, val = whole.download()
    dim = whole.dim
    for cuts in ([0, dim // 2, dim], [0, 17, dim // 3, dim]):
        parts = []
        for r0, r1 in zip(cuts[:-1], cuts[1:]):
            S = q.csr_mat.qudit(n, d, total, pairs, singles, rows=(r0, r1), opts=q.make_opts(**PLAIN))
            assert S.dim == r1 - r0 and S.row_offset == r0 and S.ncols == dim
            parts.append(S.download())
        ja2 = np.concatenate([p[1] for p in parts])
        val2 = np.concatenate([p[2] for p in parts])
        ia2 = np.concatenate([[0]] + [p[0][1:] + sum(len(x[1]) for x in parts[:k]) for k, p in enumerate(parts)])
        assert np.array_equal(ia, ia2) and np.array_equal(ja, ja2) and np.array_equal(val, val2)


class Ranker:
    """Host rank / unrank of the generator's basis, from the counting table (independent of the device code)."""

    def __init__(self, n, d, total):
        self.n, self.d, self.total = n, d, total
        cnt = [1] + [0] * total
        self.cum = []
        for _ in range(n):
            self.cum.append(np.cumsum(cnt).tolist())
            cnt = [sum(cnt[qq - l] for l in range(min(d - 1, qq) + 1)) for qq in range(total + 1)]
        self.dim = cnt[total]

    def unrank(self, r):
        w, Q = [0] * self.n, self.total
        for s in range(self.n - 1, -1, -1):
            c = self.cum[s]
            for l in range(min(self.d - 1, Q), -1, -1):
                if c[Q] - c[Q - l] <= r:
                    break
            r -= c[Q] - c[Q - l]
            Q -= l
            w[s] = l
        return w

    def rank(self, w):
        r, Q = 0, sum(w)
        for s in range(self.n - 1, -1, -1):
            r += self.cum[s][Q] - self.cum[s][Q - w[s]]
            Q -= w[s]
        return r


def test_full_size_spin1_chain_L18():
    L, d = 18, 3
    A = q.csr_mat.spin_heisenberg(L, 1, 0, chain(L))
    rk = Ranker(L, d, L)
    assert A.dim == rk.dim == qudit.qudit_dim(L, d, L) and A.dim > 4.0e7
    M = qudit.heisenberg_terms(1, [(0, 1)])[0][2]
    rng = np.random.default_rng(18)
    for r in sorted(rng.choice(A.dim, size=2000, replace=False).tolist()) + [0, A.dim - 1]:
        w = rk.unrank(r)
        assert rk.rank(w) == r
        want = {r: 0.0}
        for i, j in chain(L):
            cin = w[i] * d + w[j]
            want[r] += M[cin, cin].real
            for o in range(d * d):
                if o != cin and M[o, cin] != 0:
                    t = list(w)
                    t[i], t[j] = o // d, o % d
                    want[rk.rank(t)] = M[o, cin]
        ia, ja, val = A.download(r, r + 1)
        assert list(ja) == sorted(want), r
        assert np.allclose(val, [want[c] for c in ja], rtol=0, atol=1e-14), r
    res = q.locate_E0_lanczos(A, nev=1, ncv=0, maxit=30)
    assert np.isfinite(res.E0) and res.steps["E0"] >= 20
    x = (rng.normal(size=A.dim) + 1j * rng.normal(size=A.dim)).astype(np.complex128)
    y = (rng.normal(size=A.dim) + 1j * rng.normal(size=A.dim)).astype(np.complex128)
    hx, hy = np.empty_like(x), np.empty_like(y)
    A.MultMv(x, hx)
    A.MultMv(y, hy)
    lhs, rhs = np.vdot(x, hy), np.vdot(hx, y)
    assert abs(lhs - rhs) <= 1e-10 * abs(lhs)


def dense_site_sum(n, d, total_old, total_new, coef, local):
    """sum_s coef[s] O_s from the sector total_old to total_new, dense, in the generator's order."""
    old, new = sector_words(n, d, total_old), sector_words(n, d, total_new)
    index = {w: k for k, w in enumerate(new)}
    O = np.zeros((len(new), len(old)), dtype=np.complex128)
    for k, w in enumerate(old):
        for s in range(n):
            for lp in range(d):
                if local[lp, w[s]] != 0:
                    t = list(w)
                    t[s] = lp
                    O[index[tuple(t)], k] += coef[s] * local[lp, w[s]]
    return O


def _apply(A, n, d, total_old, dq, coef, local, x):
    vx = q.DeviceVec(A, len(x))
    vx.upload(x)
    dim_new = qudit.qudit_dim(n, d, total_old + dq)
    vy = q.DeviceVec(A, dim_new)
    try:
        assert q.moprXvec_qudit(n, d, total_old, dq, coef, local, vx.ptr, vy.ptr) == dim_new
        return vy.download()
    finally:
        vx.free()
        vy.free()


def test_mopr_qudit_against_dense_operators():
    rng = np.random.default_rng(7)
    L, d = 8, 3
    sz, spl, smi = qudit.spin_matrices(1)
    A = q.csr_mat.spin_heisenberg(L, 1, 0, chain(L))
    coef = np.exp(1j * np.pi * 3 * np.arange(L) / 4) / np.sqrt(L) * (1 + 0.1 * rng.normal(size=L))
    for total in (L, L - 1, L + 2):
        x = (rng.normal(size=qudit.qudit_dim(L, d, total)) + 1j * rng.normal(size=qudit.qudit_dim(L, d, total)))
        for local, dq in ((sz, 0), (spl, -1), (smi, 1)):
            y = _apply(A, L, d, total, dq, coef, local, x)
            want = dense_site_sum(L, d, total, total + dq, coef, local) @ x
            assert np.abs(y - want).max() <= 1e-13 * np.abs(want).max()
    b, bd, nn = qudit.boson_matrices(3)
    n = 6
    for total in (5, 6):
        x = rng.normal(size=qudit.qudit_dim(n, 4, total)) + 1j * rng.normal(size=qudit.qudit_dim(n, 4, total))
        c = rng.normal(size=n) + 1j * rng.normal(size=n)
        for local, dq in ((b, -1), (nn, 0), (bd, 1)):
            y = _apply(A, n, 4, total, dq, c, local, x)
            want = dense_site_sum(n, 4, total, total + dq, c, local) @ x
            assert np.abs(y - want).max() <= 1e-13 * np.abs(want).max()
    with pytest.raises(q._lib.QbhError):
        _apply(A, n, 4, 5, 0, c, b, np.zeros(qudit.qudit_dim(n, 4, 5), dtype=np.complex128))


def test_measure_full_dynamic_spin1_chain_at_pi():
    L, d = 8, 3
    sz, spl, smi = qudit.spin_matrices(1)
    pairs = qudit.heisenberg_terms(1, chain(L))
    _, H0 = host_sector_csr(L, d, L, pairs, [])
    w, V = np.linalg.eigh(H0.toarray())
    phi = V[:, 0].astype(np.complex128)
    A = q.csr_mat.spin_heisenberg(L, 1, 0, chain(L))
    B = q.csr_mat.spin_heisenberg(L, 1, 2, chain(L))             # S^+ raises S^z to 1: charge L - 1
    assert B.dim == qudit.qudit_dim(L, d, L - 1)
    coef = np.exp(1j * np.pi * np.arange(L)) / np.sqrt(L)
    vphi = q.DeviceVec(A, A.dim)
    vphi.upload(phi)
    try:
        m, norm, hess = q.measure_full_dynamic_dev(B, lambda dst: q.moprXvec_qudit(L, d, L, -1, coef, spl, vphi.ptr, dst), 100)
    finally:
        vphi.free()
    Sp = dense_site_sum(L, d, L, L - 1, coef, spl)
    want = np.vdot(Sp @ phi, Sp @ phi).real                      # <phi| S^-_{-q} S^+_q |phi>
    assert abs(norm ** 2 - want) <= 1e-8 * want
    assert m > 10 and np.all(np.isfinite(hess[:2 * m]))
