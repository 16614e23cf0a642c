"""qbh_mf_kondo_repr on the device: the momentum sector of the Kondo lattice applied from its basis, against (a) the stored
sector of qbh_gen_kondo_repr on the same vectors and (b) the explicit projection B^dag H B x, with B the normalised momentum
states written out word by word here (the construction of tests/test_gpu_kondo.py, vectorised) and H assembled here in numpy
from the operator's definition; (b) is evaluated in longdouble.

Bounds.  With M the reference matrix (the downloaded stored operator for (a), B^dag H B for (b)), n_i the entries of its row i
and u = 2^-53, a row must satisfy
    |dy_i| <= 4 (n_i + 4) u (|alpha| (|M||x|)_i + |beta| |y_i| + |gamma| |x_i|):
a sum of n_i products and the three epilogue terms, evaluated in any order, is off by at most (n_i + 4) u times the sum of the
absolute terms; the factor 4 covers the complex products (each entry is itself a product of an amplitude, a character and a
square root) and the different merge order of duplicates.  The bound is computed by the test in longdouble.  The reductions
are compared with the longdouble sums over the vector the device wrote: (N + 8) u sum |terms| for N rows.
Every figure is printed before it is asserted."""
import ctypes as C
import json
import os
from fractions import Fraction
from functools import lru_cache

import numpy as np
import pytest
import scipy.sparse as sp

import quantum_basis_amd as q
from quantum_basis_amd import _lib, kondo

pytestmark = pytest.mark.gpu

PLAIN = dict(value_dict=0, real_fast_path=0)
EPILOGUES = [(1.0, 0.0, 0.0), (1.0, 1.0, 0.0), (0.6, -1.2, 0.0), (1.0, 0.0, -3.0), (-0.7, 0.4, 1.5)]
FAKE = 100.0
GOLDEN = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "kondo_reference_answers.json")))
LD, CLD = np.longdouble, np.clongdouble
U53 = LD(2.0) ** -53
PI_LD = 4 * np.arctan(LD(1))


# ---- lattices and groups: (perms, turns) with the character of translation g = exp(-2 pi i turns[g]) ----
def chain(L):
    return [(i, (i + 1) % L) for i in range(L)]


def chain_group(L, m):
    return [[(s + t) % L for s in range(L)] for t in range(L)], [Fraction(m * t, L) % 1 for t in range(L)]


def torus_site(Lx, Ly, x, y):
    return (x % Lx) + Lx * (y % Ly)


def torus_group(Lx, Ly, mx, my):
    perms, turns = [], []
    for ty in range(Ly):
        for tx in range(Lx):
            perms.append([torus_site(Lx, Ly, x + tx, y + ty) for y in range(Ly) for x in range(Lx)])
            turns.append((Fraction(mx * tx, Lx) + Fraction(my * ty, Ly)) % 1)
    return perms, turns


def square_bonds(Lx, Ly):
    return [b for x in range(Lx) for y in range(Ly)
            for b in ((torus_site(Lx, Ly, x, y), torus_site(Lx, Ly, x + 1, y)), (torus_site(Lx, Ly, x, y), torus_site(Lx, Ly, x, y + 1)))]


def chars_of(turns):
    """the characters as the caller of the library computes them, in double"""
    return np.exp(-2j * np.pi * np.array([float(t) for t in turns]))


def chars_ld(turns):
    a = np.array([LD(t.numerator) / LD(t.denominator) for t in turns], dtype=LD) * (2 * PI_LD)
    return np.cos(a).astype(CLD) - 1j * np.sin(a).astype(CLD)


def flux_terms(L, phi, t_up=1.0, t_dn=0.8, mu=0.3):
    """flux_terms of tests/test_gpu_kondo.py: complex hops (a flux through the ring), species-dependent, with a chemical potential"""
    ph = np.exp(1j * phi)
    hops = []
    for i in range(L):
        j = (i + 1) % L
        hops += [(j, i, -t_up * ph, -t_dn * ph), (i, j, -t_up * np.conj(ph), -t_dn * np.conj(ph))]
        hops.append((i, i, -mu, -mu))
    return hops


def all_to_all_terms(n):
    """the operator of tests/test_kondo_repr_mf_cpu.py: hops -1/r between every pair of a ring, r the ring distance"""
    dist = lambda i, j: min((j - i) % n, (i - j) % n)
    hops = [(i, j, -1.0 / dist(i, j), -1.0 / dist(i, j)) for i in range(n) for j in range(n) if i != j]
    return kondo.Terms(hops, [1.1] * n, [1.1] * n, [])


# ---- the operator from its definition, vectorised over the words of the sector ----
def popcount(a):
    a = np.asarray(a, dtype=np.int64)
    c = np.zeros(a.shape, dtype=np.int64)
    for b in range(3 * kondo.MAX_SITES):
        c += (a >> b) & 1
    return c


@lru_cache(maxsize=4)
def sector_fields(n, n_elec, two_sz):
    """(w, u, d, s) of the sector's words, ascending; shared, never written to"""
    w = kondo.words(n, n_elec, two_sz).astype(np.int64)
    m = (1 << n) - 1
    return w, w & m, (w >> n) & m, w >> (2 * n)


def numpy_H(n, n_elec, two_sz, T, U):
    """(rows, cols, vals) of <row| H |col> on the sector's words, ascending; the string is all up operators, then all down,
    sites ascending, so a hop inside one species picks up (-1)^(particles of that species strictly between the two sites) and
    the Kondo flip on site i the operators it passes: c+_dn c_up (or c+_up c_dn) on one site."""
    w, u, d, s = sector_fields(n, n_elec, two_sz)
    N = len(w)
    bit = lambda f, i: (f >> i) & 1
    rows, cols, vals = [], [], []

    def add(mask, u2, d2, s2, amp):
        idx = np.flatnonzero(mask)
        new = u2[idx] | (d2[idx] << n) | (s2[idx] << (2 * n))
        r = np.searchsorted(w, new)
        assert np.array_equal(w[r], new)
        rows.append(r); cols.append(idx); vals.append(np.broadcast_to(amp, (N,))[idx].astype(np.complex128))

    diag = (U * popcount(u & d)).astype(np.complex128)
    for (i, j, au, ad) in T.hops:
        for sp_, amp in ((0, au), (1, ad)):
            if amp == 0:
                continue
            occ = d if sp_ else u
            if i == j:
                diag += amp * bit(occ, i)
                continue
            lo, hi = min(i, j), max(i, j)
            between = ((1 << hi) - 1) & ~((2 << lo) - 1)
            sign = 1 - 2 * (popcount(occ & between) & 1)
            occ2 = occ ^ (1 << i) ^ (1 << j)                 # c+_i c_j |col>: j occupied, i empty
            add((bit(occ, j) == 1) & (bit(occ, i) == 0), u if sp_ else occ2, occ2 if sp_ else d, s, amp * sign)
    for i in range(n):
        b, low = 1 << i, (1 << i) - 1
        diag += T.kz[i] * (0.5 - bit(s, i)) * 0.5 * (bit(u, i) - bit(d, i))
        if T.kxy[i] != 0:
            # S+_i s-_i (local spin down, up electron alone on i): destroy (i, up), create (i, dn)
            par = popcount(u & low) + popcount(u) - 1 + popcount(d & low)
            add((bit(s, i) == 1) & (bit(u, i) == 1) & (bit(d, i) == 0), u ^ b, d ^ b, s ^ b, 0.5 * T.kxy[i] * (1 - 2 * (par & 1)))
            # S-_i s+_i (local spin up, down electron alone on i): destroy (i, dn), create (i, up)
            par = popcount(u) + popcount(d & low) + popcount(u & low)
            add((bit(s, i) == 0) & (bit(d, i) == 1) & (bit(u, i) == 0), u ^ b, d ^ b, s ^ b, 0.5 * T.kxy[i] * (1 - 2 * (par & 1)))
    for (i, j, bz, bxy) in T.sbonds:
        anti = bit(s, i) != bit(s, j)
        diag += bz * np.where(anti, -0.25, 0.25)
        if bxy != 0:
            add(anti, u, d, s ^ (1 << i) ^ (1 << j), np.full(N, 0.5 * bxy))
    rows.append(np.arange(N)); cols.append(np.arange(N)); vals.append(diag)
    return np.concatenate(rows), np.concatenate(cols), np.concatenate(vals), N


def spmv_ld(rows, cols, vals, x, n):
    y = np.zeros(n, dtype=CLD)
    np.add.at(y, rows, vals * x[cols])
    return y


class Momentum:
    """B[:, a] = (|G| |S_a|)^(-1/2) sum_g chi(g) T_g |a> for every orbit representative a (the smallest word of its orbit),
    ascending; T_g moves every operator to its image and putting each electron species back in order costs the parity of the
    sorting permutation; zero[a] marks the states that vanish at this momentum.  Held as triplets in longdouble and as a
    scipy matrix in double."""

    def __init__(self, n, n_elec, two_sz, perms, turns):
        w, u, d, s = sector_fields(n, n_elec, two_sz)
        N, G = len(w), len(perms)
        img = np.empty((G, N), dtype=np.int64)
        sgn = np.empty((G, N), dtype=np.int64)
        for g, p in enumerate(perms):
            par = np.zeros(N, dtype=np.int64)
            out = []
            for f, fermion in ((u, True), (d, True), (s, False)):
                o = np.zeros(N, dtype=np.int64)
                for i in range(n):
                    o |= ((f >> i) & 1) << p[i]
                    if fermion:
                        for j in range(i + 1, n):
                            if p[i] > p[j]:
                                par ^= (f >> i) & (f >> j) & 1
                out.append(o)
            new = out[0] | (out[1] << n) | (out[2] << (2 * n))
            img[g] = np.searchsorted(w, new)
            assert np.array_equal(w[img[g]], new)
            sgn[g] = 1 - 2 * par
        me = np.arange(N)
        ridx = np.flatnonzero(img.min(axis=0) == me)
        stab = (img == me[None, :]).sum(axis=0)[ridx]
        self.dim = len(ridx)
        self.reps = w[ridx]
        self.N = N
        self.rows = img[:, ridx].reshape(-1)
        self.cols = np.tile(np.arange(self.dim), G)
        norm = np.sqrt((LD(G) * stab.astype(LD)))
        self.vals = (chars_ld(turns)[:, None] * sgn[:, ridx].astype(LD) / norm[None, :]).reshape(-1)
        key = self.rows * self.dim + self.cols               # the norm of every column: entries on the same word add first
        order = np.argsort(key, kind="stable")
        ks, vs = key[order], self.vals[order]
        first = np.concatenate([[True], np.diff(ks) != 0])
        merged = np.add.reduceat(vs, np.flatnonzero(first))
        mcols = ks[first] % self.dim
        n2 = np.zeros(self.dim, dtype=LD)
        np.add.at(n2, mcols, (merged.real ** 2 + merged.imag ** 2))
        self.zero = np.sqrt(n2) < 1e-9
        self.vals = np.where(self.zero[self.cols], 0, self.vals)
        self.B = sp.coo_matrix((self.vals.astype(np.complex128), (self.rows, self.cols)), shape=(N, self.dim)).tocsc()
        self.fake = np.where(self.zero, FAKE + np.arange(self.dim) / self.dim, 0.0)


class Reference:
    """One sector: x -> B^dag H B x + fake diagonal in longdouble, and the same matrix in double for the bound."""

    def __init__(self, n, n_elec, two_sz, T, U, perms, turns, H=None):
        self.mb = Momentum(n, n_elec, two_sz, perms, turns)
        self.H = H if H is not None else numpy_H(n, n_elec, two_sz, T, U)
        hr, hc, hv, N = self.H
        Hd = sp.coo_matrix((hv, (hr, hc)), shape=(N, N)).tocsr()
        M = (self.mb.B.conj().T @ Hd @ self.mb.B + sp.diags(self.mb.fake)).tocsr()
        M.eliminate_zeros()
        self.M = M
        self.dim = self.mb.dim

    def apply(self, x):
        mb = self.mb
        hr, hc, hv, N = self.H
        xl = x.astype(CLD)
        t = spmv_ld(mb.rows, mb.cols, mb.vals, xl, N)
        t = spmv_ld(hr, hc, hv.astype(CLD), t, N)
        return spmv_ld(mb.cols, mb.rows, np.conj(mb.vals), t, mb.dim) + mb.fake.astype(LD) * xl


def row_bound(M, x, y0, alpha, beta, gamma):
    """4 (n_i + 4) u (|alpha| (|M||x|)_i + |beta| |y_i| + |gamma| |x_i|) in longdouble from the CSR matrix M"""
    M = M.tocsr()
    n_i = np.diff(M.indptr).astype(LD)
    prod = np.abs(M.data).astype(LD) * np.abs(x).astype(LD)[M.indices]
    ax = np.zeros(M.shape[0], dtype=LD)
    np.add.at(ax, np.repeat(np.arange(M.shape[0]), np.diff(M.indptr)), prod)
    return 4 * (n_i + 4) * U53 * (abs(LD(alpha)) * ax + abs(LD(beta)) * np.abs(y0).astype(LD) + abs(LD(gamma)) * np.abs(x).astype(LD))


def full_csr(A):
    ia, ja, val = A.download()
    return sp.csr_matrix((val, ja, ia), shape=(len(ia) - 1, A.info().ncols))


def stored(n, n_elec, two_sz, T, U, perms, turns, **kw):
    return q.csr_mat.kondo_repr(n, n_elec, two_sz, None, perms, chars_of(turns), U=U, terms=T, fake_pos=FAKE, opts=q.make_opts(**PLAIN), **kw)


def matrix_free(n, n_elec, two_sz, T, U, perms, turns, rows=None):
    return q.csr_mat.kondo_repr(n, n_elec, two_sz, None, perms, chars_of(turns), U=U, terms=T, fake_pos=FAKE, matrix_free=True, rows=rows)


def _rand(n, seed):
    rng = np.random.default_rng(seed)
    return (rng.normal(size=n) + 1j * rng.normal(size=n)).astype(np.complex128)


def _worst(diff, bound):
    r = np.max(np.where(bound > 0, diff / np.where(bound > 0, bound, 1), np.where(diff > 0, np.inf, 0)))
    return float(r)


def assert_reductions(x, ym, dot, nrm, tag):
    """the fused reductions against longdouble sums over the vector the device wrote"""
    N = len(x)
    xl, yl = x.astype(CLD), ym.astype(CLD)
    terms = np.conj(xl) * yl
    dref, dabs = terms.sum(), np.abs(terms).sum()
    nref = (yl.real ** 2 + yl.imag ** 2).sum()
    e_dot, e_nrm = abs(CLD(dot) - dref), abs(LD(nrm) - nref)
    print(tag, "dot err %.3e bound %.3e | norm err %.3e bound %.3e" % (e_dot, (N + 8) * U53 * dabs, e_nrm, (N + 8) * U53 * nref))
    assert e_dot <= (N + 8) * U53 * dabs
    assert e_nrm <= (N + 8) * U53 * nref


def assert_spmv(M, seed, A=None, A_csr=None, ref=None, epilogues=EPILOGUES, x=None):
    """y = alpha H x + beta y + gamma x with both reductions: the matrix-free handle M against the stored handle A (row bound
    from its downloaded matrix A_csr) and against the longdouble projection ref."""
    n = M.dim
    x = _rand(n, seed) if x is None else x
    y0 = _rand(n, seed + 1)
    vm = M.vec(2)
    va = A.vec(2) if A is not None else None
    Px = ref.apply(x) if ref is not None else None
    for alpha, beta, gamma in epilogues:
        for v in (va, vm):
            if v is not None:
                v.upload(x, 0)
                v.upload(y0, n)
        dm, nm = M.spmv(vm.at(0), vm.at(n), alpha, beta, gamma, want_red=True)
        ym = vm.download(n, n)
        assert_reductions(x, ym, dm, nm, "reductions %s" % ((alpha, beta, gamma),))
        if A is not None:
            A.spmv(va.at(0), va.at(n), alpha, beta, gamma)
            ya = va.download(n, n)
            bound = row_bound(A_csr, x, y0, alpha, beta, gamma)
            diff = np.abs(ym.astype(CLD) - ya.astype(CLD))
            print("mf-stored", (alpha, beta, gamma), "max |dy| %.3e, worst |dy|/bound %.3f" % (diff.max(), _worst(diff, bound)))
            assert np.all(diff <= bound)
        if ref is not None:
            yw = LD(alpha) * Px + LD(beta) * y0.astype(CLD) + LD(gamma) * x.astype(CLD)
            bound = row_bound(ref.M, x, y0, alpha, beta, gamma)
            diff = np.abs(ym.astype(CLD) - yw)
            print("mf-projection", (alpha, beta, gamma), "max |dy| %.3e, worst |dy|/bound %.3f" % (diff.max(), _worst(diff, bound)))
            assert np.all(diff <= bound)
    vm.free()
    if va is not None:
        va.free()


def check_sector(n, n_elec, two_sz, T, U, perms, turns, seed, H=None):
    ref = Reference(n, n_elec, two_sz, T, U, perms, turns, H)
    A, M = stored(n, n_elec, two_sz, T, U, perms, turns), matrix_free(n, n_elec, two_sz, T, U, perms, turns)
    assert M.dim == A.dim == ref.dim
    assert M.info().kernel == _lib.KERNEL_MATRIX_FREE and M.nnz >= A.nnz
    assert_spmv(M, seed, A, full_csr(A), ref)
    return ref, A, M


# ---- 1 ----
CHAIN6 = (6, 6, 0, kondo.terms(6, chain(6), 1.0, 1.1, 0.3), 0.8)


@lru_cache(maxsize=1)
def chain6_H():
    n, n_elec, two_sz, T, U = CHAIN6
    return numpy_H(n, n_elec, two_sz, T, U)


@lru_cache(maxsize=1)
def chain6_zero_counts():
    n, n_elec, two_sz, T, U = CHAIN6
    return tuple(int(np.count_nonzero(Momentum(n, n_elec, two_sz, *chain_group(n, m)).zero)) for m in range(n))


def test_the_numpy_operator_is_the_one_the_full_generator_assembles():
    n, n_elec, two_sz, T, U = CHAIN6
    hr, hc, hv, N = chain6_H()
    got = full_csr(q.csr_mat.kondo(n, n_elec, two_sz, None, U=U, terms=T, opts=q.make_opts(**PLAIN)))
    diff = abs(got - sp.coo_matrix((hv, (hr, hc)), shape=(N, N)).tocsr())
    print("dim %d, max |delta| %.3e" % (N, diff.max()))
    assert N == 15184 and diff.max() <= 1e-15


def test_the_chain_has_sectors_with_zero_norm_representatives():
    """u = 111111, s = 111111 is fixed by every translation with the sign of a 6-cycle: it survives at k = pi alone."""
    z = chain6_zero_counts()
    print("zero-norm representatives by momentum:", z)
    assert z[3] < z[0] and all(z[m] > 0 for m in (0, 1, 2, 4, 5))


@pytest.mark.parametrize("m", range(6))
def test_every_momentum_of_the_chain_L6(m):
    n, n_elec, two_sz, T, U = CHAIN6
    perms, turns = chain_group(n, m)
    ref, A, M = check_sector(n, n_elec, two_sz, T, U, perms, turns, 10 + m, chain6_H())
    dim = M.dim
    assert 2500 < dim < 2560                               # 15184 words in orbits of 6, a few shorter ones
    if m not in (0, 3):
        assert M.stats().n_spmv_real == 0                  # complex characters: never the real path
    zero = ref.mb.zero
    assert np.count_nonzero(zero) == chain6_zero_counts()[m]
    if chain6_zero_counts()[m] == 0:
        return
    assert zero.any()                                      # not vacuous in this sector
    fake = FAKE + np.arange(dim) / dim
    # columns: the indicator of the zero-norm rows comes back as their fake diagonals and reaches no live row
    e = zero.astype(np.complex128)
    y = np.empty_like(e)
    M.MultMv(e, y)
    assert np.all(np.abs(y[zero] - fake[zero]) <= 4 * 5 * float(U53) * fake[zero]) and not y[~zero].any()
    # rows: a random vector comes back on a zero-norm row as fake x_i, whatever the other components are
    x = _rand(dim, 90 + m)
    M.MultMv(x, y)
    assert np.all(np.abs(y[zero] - fake[zero] * x[zero]) <= 4 * 5 * float(U53) * np.abs(fake[zero] * x[zero]))


# ---- 2 ----
@pytest.mark.parametrize("m", [0, 1])
def test_flux_ring_complex_hops(m):
    """complex hops, t_up != t_dn, an on-site term, anisotropic couplings, odd filling: the complex kernel at a real and at a
    complex momentum, up and down hop amplitudes and their signs"""
    L, n_elec, two_sz, U = 6, 5, 1, 1.2
    T = kondo.Terms(flux_terms(L, 0.41), [0.7] * L, [1.3] * L, [(i, (i + 1) % L, 0.2, 0.5) for i in range(L)])
    perms, turns = chain_group(L, m)
    ref, A, M = check_sector(L, n_elec, two_sz, T, U, perms, turns, 20 + m)
    assert M.stats().n_spmv_real == 0                      # complex values: never the real path


# ---- 3 ----
@pytest.mark.parametrize("k", [(1, 1), (2, 0), (0, 0)])
def test_torus_3x2_with_two_generators(k):
    """translations that are not cyclic shifts of the site index: the fermion sign of g* != 0, and U != 0"""
    Lx, Ly = 3, 2
    n = Lx * Ly
    T = kondo.terms(n, square_bonds(Lx, Ly), 1.0, 1.1)
    perms, turns = torus_group(Lx, Ly, *k)
    assert len(perms) == 6
    check_sector(n, 6, 0, T, 1.7, perms, turns, 30 + k[0])


# ---- 4 ----
@pytest.mark.parametrize("m", [0, 2])
def test_anisotropic_couplings_and_local_spin_bonds(m):
    """kz != kxy and bz != bxy on a ring of 5 sites at odd filling: the Kondo flip and the local-spin exchange"""
    L = 5
    T = kondo.Terms(kondo.hop_terms(chain(L), 1.0), [0.7] * L, [1.9] * L,
                    [(i, (i + 1) % L, 0.4, 0.9) for i in range(L)] + [(i, (i + 2) % L, 0.2, -0.3) for i in range(L)])
    perms, turns = chain_group(L, m)
    check_sector(L, 4, 1, T, 0.0, perms, turns, 40 + m)


def table_bytes(n, n_trans):
    """what the kernel stages in LDS: the byte-sliced translation tables (one 64-entry table per translation and six-bit chunk
    of a field) and the two counting tables of 22 x 22 words"""
    return (n_trans * ((n + 5) // 6) * 64 + 2 * 22 * 22) * 8


def test_wide_words_on_the_large_table_path():
    """A ring of 21 sites: the s field sits in bits 42 .. 62 (a 32-bit shift or mask anywhere loses it), and 21 translations
    of 4 chunks make 50,752 B of tables: fewer than four workgroups of 256 lanes fit a CU beside them, so the kernel runs
    with workgroups of 1024 lanes, the shape no smaller lattice reaches.  2 electrons, 2 S^z = -19: 53571 words."""
    n, n_elec, two_sz = 21, 2, -19
    assert 4 * (table_bytes(n, n) + 1024) > 160 * 1024 >= 4 * (table_bytes(13, 13) + 1024)
    T = kondo.Terms(kondo.hop_terms(chain(n), 1.0), [1.1] * n, [0.9] * n, [(i, (i + 1) % n, 0.4, 0.7) for i in range(n)])
    perms, turns = chain_group(n, 5)
    ref, A, M = check_sector(n, n_elec, two_sz, T, 1.3, perms, turns, 45)
    assert M.dim == 2551 and kondo.sector_dim(n, n_elec, two_sz) == 53571
    assert int(ref.mb.reps.max()) >> 42 > 0


# ---- 5 ----
def test_more_rows_than_one_pass_of_the_resident_grid():
    """Chain L = 10, n_elec = 8, S^z = 0, k = 0: about 2.6e6 rows against at most 256 CUs x 5 workgroups x 256 lanes.  Against
    the stored operator only; x has unit modulus so that (|M||x|)_i is the absolute row sum of the downloaded values."""
    L, n_elec = 10, 8
    T = kondo.terms(L, chain(L), 1.0, 1.1)
    perms, turns = chain_group(L, 0)
    A, M = stored(L, n_elec, 0, T, 0.0, perms, turns), matrix_free(L, n_elec, 0, T, 0.0, perms, turns)
    dim = M.dim
    print("dim", dim, "nnz stored", A.nnz, "contributions", M.nnz)
    assert dim == A.dim and 2.5e6 < dim < 2.8e6 and dim > 256 * 5 * 256 and M.nnz >= A.nnz
    ia = np.empty(dim + 1, dtype=np.int64)
    val = np.empty(A.nnz, dtype=np.complex128)
    _lib.check(_lib.lib().qbh_csr_download(A.handle, C.c_int64(0), C.c_int64(dim), ia.ctypes.data, None, val.ctypes.data),
               "qbh_csr_download")
    n_i = np.diff(ia).astype(LD)
    ax = np.add.reduceat(np.abs(val), ia[:-1]).astype(LD)      # every row holds its diagonal: no empty row
    assert np.all(np.diff(ia) > 0)
    rng = np.random.default_rng(51)
    x = np.exp(2j * np.pi * rng.random(dim))
    y0 = _rand(dim, 52)
    alpha, beta, gamma = 0.6, -1.2, 0.3
    vm, va = M.vec(2), A.vec(2)
    for v in (va, vm):
        v.upload(x, 0)
        v.upload(y0, dim)
    dm, nm = M.spmv(vm.at(0), vm.at(dim), alpha, beta, gamma, want_red=True)
    A.spmv(va.at(0), va.at(dim), alpha, beta, gamma)
    ym, ya = vm.download(dim, dim), va.download(dim, dim)
    bound = 4 * (n_i + 4) * U53 * (abs(LD(alpha)) * ax + abs(LD(beta)) * np.abs(y0).astype(LD) + abs(LD(gamma)))
    diff = np.abs(ym.astype(CLD) - ya.astype(CLD))
    print("mf-stored max |dy| %.3e, worst |dy|/bound %.3f" % (diff.max(), _worst(diff, bound)))
    assert np.all(diff <= bound)
    assert_reductions(x, ym, dm, nm, "reductions")
    vm.free()
    va.free()


# ---- 6 ----
@pytest.mark.parametrize("m", [0, 1])
def test_ragged_row_shards_are_bit_identical_to_the_whole_operator(m):
    """m = 0: real characters and a real x; m = 1: complex characters"""
    n, n_elec, two_sz, T, U = CHAIN6
    perms, turns = chain_group(n, m)
    whole = matrix_free(n, n_elec, two_sz, T, U, perms, turns)
    dim = whole.dim
    x, y0 = _rand(dim, 61), _rand(dim, 62)
    if m == 0:
        x, y0 = x.real.astype(np.complex128), y0.real.astype(np.complex128)
    vw = whole.vec(2)
    vw.upload(x, 0)
    vw.upload(y0, dim)
    whole.spmv(vw.at(0), vw.at(dim), 0.6, -1.2, 0.3)
    y = vw.download(dim, dim)
    vw.free()
    cuts = [0, 1, 67, dim // 5 + 7, dim - 257 - 129, dim - 129, dim]      # one row; no cut a multiple of 64 or of 256
    assert all(c % 64 for c in cuts[1:-1])
    nnz = 0
    for r, (r0, r1) in enumerate(zip(cuts[:-1], cuts[1:])):
        S = matrix_free(n, n_elec, two_sz, T, U, perms, turns, rows=(r0, r1))
        Tst = stored(n, n_elec, two_sz, T, U, perms, turns, shard=(r, len(cuts) - 1), row_cuts=cuts)
        i, j = S.info(), Tst.info()
        assert (i.nrows, i.row_offset, i.ncols) == (j.nrows, j.row_offset, j.ncols) == (r1 - r0, r0, dim)
        assert i.kernel == _lib.KERNEL_MATRIX_FREE and S.nnz >= Tst.nnz
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


# ---- 7 ----
@pytest.mark.parametrize("m", [0, 5])
def test_all_to_all_operator_beyond_the_row_limit_of_the_stored_form(m):
    """13 sites, hops between every pair: 2 * 78 + 13 + 1 = 170 > 160 entries in the worst row, so no stored handle exists.
    Checked in the sector of 2 electrons, 2 S^z = 11 (8359 words) against the projection."""
    n, n_elec, two_sz = 13, 2, 11
    T = all_to_all_terms(n)
    assert kondo.sector_dim(n, n_elec, two_sz) == 8359
    perms, turns = chain_group(n, m)
    with pytest.raises(_lib.QbhError) as e:
        stored(n, n_elec, two_sz, T, 0.0, perms, turns)
    assert e.value.code == -9
    ref = Reference(n, n_elec, two_sz, T, 0.0, perms, turns)
    M = matrix_free(n, n_elec, two_sz, T, 0.0, perms, turns)
    assert M.dim == ref.dim == 643 and not ref.mb.zero.any()    # 13 is prime and no word is fixed: 8359 / 13 orbits
    # nnz: one diagonal per row plus every off-diagonal entry of H out of a representative (every target has nonzero norm)
    hr, hc, hv, N = ref.H
    w = sector_fields(n, n_elec, two_sz)[0]
    is_rep = np.zeros(N, dtype=bool)
    is_rep[np.searchsorted(w, ref.mb.reps)] = True
    assert M.nnz == M.dim + np.count_nonzero(is_rep[hc] & (hr != hc))
    assert_spmv(M, 70 + m, ref=ref)


# ---- 8 ----
def _lanczos_E0(M, maxit=400):
    n = M.dim
    v = M.vec(2)
    M.randomize(v.at(0), 1)
    h = np.zeros(2 * maxit)
    steps = q.lanczos(0, maxit - 1, maxit, n, M, None, h, "sr_val0", device_v=v)
    ritz, _ = q.hess_eigen(h, maxit, steps, "sr")
    v.free()
    return ritz[0]


def test_solvers_on_the_reference_sector_energies():
    ref = GOLDEN["chain_L8_sz0_by_momentum"]
    L = ref["L"]
    assert L == 8 and GOLDEN["tolerance"] == 1e-8
    T = kondo.terms(L, chain(L), ref["t"], ref["J_K"])
    E = {}
    for m in range(L):
        perms, turns = chain_group(L, m)
        M = matrix_free(L, ref["n_elec"], ref["two_sz"], T, 0.0, perms, turns)
        A = stored(L, ref["n_elec"], ref["two_sz"], T, 0.0, perms, turns)
        E[m] = _lanczos_E0(M)
        Es = _lanczos_E0(A)
        print("k = %d: dim %d, E0 = %.10f, stored %.10f" % (m, M.dim, E[m], Es))
        assert abs(E[m] - Es) <= 1e-10
        if m in (0, L // 2):                               # the packed-real drivers at k = 0 and pi
            n, maxit = M.dim, 400
            buf = q.DeviceVec(M, 2 * n + 2)                # 4 slots of n packed doubles: v, r, p, pp
            at = lambda j: C.c_void_p(buf.ptr.value + 8 * n * j)
            lan = type("V", (), {"ptr": at(0)})()
            _lib.check(_lib.lib().qbh_vec_randomize_real(M.handle, at(0), C.c_uint32(1)), "qbh_vec_randomize_real")
            hr = np.zeros(2 * maxit)
            mr = q.lanczos_real(0, maxit - 1, maxit, M, lan, hr)
            er = q.hess_eigen(hr, maxit, mr, "sr")[0][0]
            print("k = %d: real Lanczos E0 = %.10f" % (m, er))
            assert abs(er - Es) <= 1e-10 and M.stats().n_spmv_real > 0
            _lib.check(_lib.lib().qbh_vec_randomize_real(M.handle, at(0), C.c_uint32(1)), "qbh_vec_randomize_real")
            q.eigenvec_CG_real(maxit, 0, M, er, at(0), at(1), at(2), at(3))
            vec = buf.download(0, (n + 1) // 2).view(np.float64)[:n].astype(np.complex128)
            hv = np.empty(n, dtype=np.complex128)
            A.MultMv(vec, hv)
            rayleigh = np.vdot(vec, hv).real / np.vdot(vec, vec).real
            resid = np.linalg.norm(hv - rayleigh * vec) / np.linalg.norm(vec)
            print("k = %d: CG eigenvector Rayleigh quotient %.10f residual %.3e" % (m, rayleigh, resid))
            assert abs(rayleigh - Es) < GOLDEN["tolerance"]
            buf.free()
        elif m == 1:
            buf = q.DeviceVec(M, 2 * M.dim + 2)
            lan = type("V", (), {"ptr": buf.ptr})()
            with pytest.raises(_lib.QbhError):             # complex characters: the real driver is refused
                q.lanczos_real(0, 10, 400, M, lan, np.zeros(800))
            assert M.stats().n_spmv_real == 0
            buf.free()
    for m, e in ref["E0_by_k"].items():
        assert abs(E[int(m)] - e) < GOLDEN["tolerance"], (m, E[int(m)], e)
        assert abs(E[(L - int(m)) % L] - e) < GOLDEN["tolerance"]


# ---- 9 ----
def test_handle_shape():
    n, n_elec, two_sz, T, U = CHAIN6
    perms, turns = chain_group(n, 1)
    A, M = stored(n, n_elec, two_sz, T, U, perms, turns), matrix_free(n, n_elec, two_sz, T, U, perms, turns)
    dim_out = M.dim
    i = M.info()
    words = kondo.sector_dim(n, n_elec, two_sz)
    assert i.kernel == _lib.KERNEL_MATRIX_FREE and (i.nrows, i.ncols, i.row_offset) == (A.dim, A.dim, 0) and dim_out == A.dim
    nchunks = (words + 4095) // 4096
    tables = i.bytes_matrix - 9 * M.dim - 8 * (nchunks + 1)      # the family's struct and the translation tables
    print("bytes_matrix", i.bytes_matrix, "tables", tables)
    assert 6 * 1 * 64 * 8 + 2 * 22 * 22 * 8 <= tables <= 64 << 10
    assert M.nnz >= A.nnz
    with pytest.raises(_lib.QbhError) as e:
        M.download()
    assert e.value.code == -9                              # QBH_EUNSUPP
    # without duplicate targets the count equals the stored nnz: 13 sites (prime: every orbit is free), one electron,
    # nearest-neighbour hops.  Two terms of a row reach the same representative only if the two target words are translates
    # of each other; asserted on the reference: no row of B^dag H B merges two entries of H.
    n, n_elec, two_sz = 13, 1, 10
    T = kondo.terms(n, chain(n), 1.0, 1.1)
    perms, turns = chain_group(n, 2)
    ref = Reference(n, n_elec, two_sz, T, 0.0, perms, turns)
    hr, hc, hv, N = ref.H
    w = sector_fields(n, n_elec, two_sz)[0]
    is_rep = np.zeros(N, dtype=bool)
    is_rep[np.searchsorted(w, ref.mb.reps)] = True
    contributions = ref.dim + np.count_nonzero(is_rep[hc] & (hr != hc))
    assert not ref.mb.zero.any()
    A, M = stored(n, n_elec, two_sz, T, 0.0, perms, turns), matrix_free(n, n_elec, two_sz, T, 0.0, perms, turns)
    assert ref.M.nnz == contributions                      # the reference merges nothing ...
    assert M.nnz == A.nnz == contributions                 # ... so neither does the stored row
    with pytest.raises(ValueError):
        q.csr_mat.kondo_repr(n, n_elec, two_sz, chain(n), perms, chars_of(turns), matrix_free=True, shard=(0, 2))
    with pytest.raises(ValueError):
        q.csr_mat.kondo_repr(n, n_elec, two_sz, chain(n), perms, chars_of(turns), matrix_free=True, row_cuts=[0, M.dim])
    with pytest.raises(ValueError):
        q.csr_mat.kondo_repr(n, n_elec, two_sz, chain(n), perms, chars_of(turns), rows=(0, 5))
