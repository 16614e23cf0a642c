"""The Kondo-lattice generators on the device, each against something computed another way: qbh_gen_kondo entry by entry
against a numpy assembly written here from the operator's definition (operators applied one at a time, signs by counting
the operators to the left), the energies the reference asserts, qbh_gen_hubbard at J_K = 0, qbh_gen_kondo_repr against
explicit momentum states B^dag H B, joined sector spectra, formats and shards, the operator x vector step, a local
observable, and the L = 10 chain through both generators."""
import json
import os
import time
from math import comb

import numpy as np
import pytest
import scipy.sparse as sp

import quantum_basis_amd as q
from quantum_basis_amd import kondo

pytestmark = pytest.mark.gpu

PLAIN = dict(value_dict=0, real_fast_path=0)
FAKE = 100.0
GOLDEN = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "kondo_reference_answers.json")))
UP, DN = 0, 1


def chain(L):
    return [(i, (i + 1) % L) for i in range(L)]


def chain_group(L, m):
    perms = [[(s + t) % L for s in range(L)] for t in range(L)]
    return perms, np.exp(-2j * np.pi * m * np.arange(L) / L)


def torus_site(Lx, Ly, x, y):
    return (x % Lx) + Lx * (y % Ly)


def torus_group(Lx, Ly, mx, my):
    perms, chars = [], []
    for ty in range(Ly):
        for tx in range(Lx):
            perms.append([torus_site(Lx, Ly, x + tx, y + ty) for y in range(Ly) for x in range(Lx)])
            chars.append(np.exp(-2j * np.pi * (mx * tx / Lx + my * ty / Ly)))
    return perms, np.array(chars)


def square_bonds(Lx, Ly):
    return [b for x in range(Lx) for y in range(Ly)
            for b in ((torus_site(Lx, Ly, x, y), torus_site(Lx, Ly, x + 1, y)), (torus_site(Lx, Ly, x, y), torus_site(Lx, Ly, x, y + 1)))]


# ---- the operator from its definition: a state is (u, d, s), the string is all up operators then all down, sites ascending ----
def popcount(x):
    return bin(int(x)).count("1")


def left_of(u, d, site, spin):
    """operators standing left of (site, spin) in the state's string"""
    low = (1 << site) - 1
    return popcount(u & low) if spin == UP else popcount(u) + popcount(d & low)


def destroy(state, site, spin):
    u, d, s = state
    occ = u if spin == UP else d
    if not (occ >> site) & 1:
        return None
    sign = -1 if left_of(u, d, site, spin) & 1 else 1
    return sign, ((u ^ (1 << site), d, s) if spin == UP else (u, d ^ (1 << site), s))


def create(state, site, spin):
    u, d, s = state
    occ = u if spin == UP else d
    if (occ >> site) & 1:
        return None
    sign = -1 if left_of(u, d, site, spin) & 1 else 1
    return sign, ((u | (1 << site), d, s) if spin == UP else (u, d | (1 << site), s))


def apply_string(ops, state):
    """ops = [(fn, site, spin), ...] written left to right; applied right to left.  Returns (sign, state) or None."""
    sign = 1
    for fn, site, spin in reversed(ops):
        r = fn(state, site, spin)
        if r is None:
            return None
        sign *= r[0]
        state = r[1]
    return sign, state


def apply_H(T, U, n, state):
    """H |state> as {state': coefficient}"""
    out = {}

    def add(st, c):
        out[st] = out.get(st, 0.0) + c

    u, d, s = state
    add(state, U * popcount(u & d))
    for (i, j, au, ad) in T.hops:
        for spin, amp in ((UP, au), (DN, ad)):
            r = apply_string([(create, i, spin), (destroy, j, spin)], state)
            if r is not None and amp != 0:
                add(r[1], amp * r[0])
    for i in range(n):
        Sz = -0.5 if (s >> i) & 1 else 0.5
        sz = 0.5 * (((u >> i) & 1) - ((d >> i) & 1))
        add(state, T.kz[i] * Sz * sz)
        if (s >> i) & 1:                               # S^+_i s^-_i,  s^- = c+_dn c_up
            r = apply_string([(create, i, DN), (destroy, i, UP)], state)
            if r is not None:
                add((r[1][0], r[1][1], s ^ (1 << i)), 0.5 * T.kxy[i] * r[0])
        else:                                          # S^-_i s^+_i,  s^+ = c+_up c_dn
            r = apply_string([(create, i, UP), (destroy, i, DN)], state)
            if r is not None:
                add((r[1][0], r[1][1], s ^ (1 << i)), 0.5 * T.kxy[i] * r[0])
    for (i, j, bz, bxy) in T.sbonds:
        si, sj = (s >> i) & 1, (s >> j) & 1
        add(state, bz * (0.25 if si == sj else -0.25))
        if si != sj:
            add((u, d, s ^ (1 << i) ^ (1 << j)), 0.5 * bxy)
    return out


def states_of(n, n_elec, two_sz):
    w = kondo.words(n, n_elec, two_sz)
    u, d, s = kondo.fields(w, n)
    return [(int(a), int(b), int(c)) for a, b, c in zip(u, d, s)]


def reference_H(n, n_elec, two_sz, T, U=0.0):
    states = states_of(n, n_elec, two_sz)
    index = {st: k for k, st in enumerate(states)}
    rows, cols, vals = [], [], []
    for k, st in enumerate(states):
        for st2, c in apply_H(T, U, n, st).items():
            rows.append(index[st2]); cols.append(k); vals.append(c)    # <st2| H |st>
    return sp.csr_matrix((vals, (rows, cols)), shape=(len(states), len(states)), dtype=np.complex128)


def full_csr(A):
    ia, ja, val = A.download()
    return sp.csr_matrix((val, ja, ia), shape=(len(ia) - 1, A.info().ncols))


def dense(A):
    return full_csr(A).toarray()


def flux_terms(L, phi, t_up=1.0, t_dn=0.8, mu=0.3):
    """complex hops (a flux through the ring), species-dependent, with a chemical potential"""
    ph = np.exp(1j * phi)
    hops = []
    for i in range(L):
        j = (i + 1) % L
        hops += [(j, i, -t_up * ph, -t_dn * ph), (i, j, -t_up * np.conj(ph), -t_dn * np.conj(ph))]
        hops.append((i, i, -mu, -mu))
    return hops


CASES = {
    "chain4_half": (4, 4, 0, kondo.terms(4, chain(4), 1.0, 4.0), 0.0),
    "chain6_half": (6, 6, 0, kondo.terms(6, chain(6), 1.0, 1.1), 0.0),
    "odd_filling_sz_plus": (4, 3, 1, kondo.terms(4, chain(4), 1.0, 1.1), 0.0),
    "odd_filling_sz_minus": (6, 5, -1, kondo.terms(6, chain(6), 1.0, 1.1), 0.0),
    "torus_3x2": (6, 6, 0, kondo.terms(6, square_bonds(3, 2), 1.0, 1.1), 0.0),
    "hubbard_U": (4, 4, 2, kondo.terms(4, chain(4), 1.0, 1.1), 2.5),
    "anisotropic": (5, 4, 1, kondo.Terms(kondo.hop_terms(chain(5), 1.0), [0.7] * 5, [1.9] * 5, []), 0.0),
    "rkky": (5, 6, -1, kondo.Terms(kondo.hop_terms(chain(5), 1.0), [1.1] * 5, [1.1] * 5,
                                   [(i, (i + 1) % 5, 0.4, 0.9) for i in range(5)] + [(3, 1, 0.2, -0.3)]), 0.0),
    "flux": (5, 5, 0, kondo.Terms(flux_terms(5, 0.37), [1.1, 0.9, 1.3, 0.0, 1.0], [1.1, 0.0, 0.5, 0.8, 1.0],
                                  [(0, 2, 0.3, 0.6)]), 1.7),
    "single_block": (3, 6, -1, kondo.terms(3, chain(3), 1.0, 1.1, 0.5), 1.0),
}


def assert_entries(got, want):
    scale = max(1.0, np.abs(want).max())
    diff = np.abs((got - want)).max() if got.nnz + want.nnz else 0.0
    print("max |delta| = %.3e, scale %.3g, dim %d, nnz %d" % (diff, scale, got.shape[0], got.nnz))
    assert diff <= 1e-12 * scale


@pytest.mark.parametrize("name", sorted(CASES))
def test_full_generator_entry_by_entry(name):
    n, n_elec, two_sz, T, U = CASES[name]
    A = q.csr_mat.kondo(n, n_elec, two_sz, None, U=U, terms=T, opts=q.make_opts(**PLAIN))
    assert A.dim == kondo.sector_dim(n, n_elec, two_sz)
    want = reference_H(n, n_elec, two_sz, T, U)
    assert_entries(full_csr(A), want)
    ia, ja, val = A.download()
    for r in range(A.dim):                             # columns ascending, the diagonal always stored
        c = ja[ia[r]:ia[r + 1]]
        assert np.all(np.diff(c) > 0) and r in c
    off = val[ja != np.repeat(np.arange(A.dim), np.diff(ia))]
    assert np.all(off != 0)                            # no stored zeros off the diagonal


def test_the_default_arguments_are_the_examples_model():
    L = 4
    A = q.csr_mat.kondo(L, L, 0, chain(L), t=1.0, J_K=4.0, J_RKKY=0.25, U=0.5, opts=q.make_opts(**PLAIN))
    assert_entries(full_csr(A), reference_H(L, L, 0, kondo.terms(L, chain(L), 1.0, 4.0, 0.25), 0.5))


def test_row_block():
    n, n_elec, two_sz, T, U = CASES["chain6_half"]
    whole = full_csr(q.csr_mat.kondo(n, n_elec, two_sz, None, terms=T, opts=q.make_opts(**PLAIN)))
    want = reference_H(n, n_elec, two_sz, T, U)
    for r0, r1 in ((0, 100), (1234, 9001), (15000, 15184)):
        B = q.csr_mat.kondo(n, n_elec, two_sz, None, terms=T, rows=(r0, r1), opts=q.make_opts(**PLAIN))
        assert B.dim == r1 - r0 and B.info().ncols == 15184 and B.row_offset == r0
        got = full_csr(B)
        assert_entries(got, want[r0:r1])
        assert (got != whole[r0:r1]).nnz == 0


def test_reference_energies_of_the_L4_chain():
    ref = GOLDEN["chain_L4_all_sz"]
    L = ref["L"]
    A = q.csr_mat.kondo(L, ref["n_elec"], 0, chain(L), t=ref["t"], J_K=ref["J_K"])
    assert A.dim == 346
    res = q.locate_E0_lanczos(A, nev=2, ncv=1)
    print("Lanczos E0 %.10f E1 %.10f" % (res.E0, res.E1))
    assert abs(res.E0 - ref["E0"]) < GOLDEN["tolerance"] and abs(res.E1 - ref["E1"]) < GOLDEN["tolerance"]
    ev = np.linalg.eigvalsh(dense(q.csr_mat.kondo(L, ref["n_elec"], 0, chain(L), t=ref["t"], J_K=ref["J_K"], opts=q.make_opts(**PLAIN))))
    distinct = ev[np.concatenate([[True], np.diff(ev) > 1e-9])]
    print("dense E0 %.10f E1 %.10f" % (distinct[0], distinct[1]))
    assert abs(distinct[0] - ref["E0"]) < GOLDEN["tolerance"] and abs(distinct[1] - ref["E1"]) < GOLDEN["tolerance"]


@pytest.mark.parametrize("n,n_elec,two_sz", [(4, 4, 0), (5, 4, 1), (4, 5, 1)])
def test_without_coupling_the_spectrum_is_hubbards(n, n_elec, two_sz):
    """J_K = J_RKKY = 0: the local spins idle, so every Hubbard level of block (n_up, n_dn, m) appears C(n, m) times."""
    U = 1.3
    A = q.csr_mat.kondo(n, n_elec, two_sz, chain(n), t=1.0, J_K=0.0, U=U, opts=q.make_opts(**PLAIN))
    got = np.sort(np.linalg.eigvalsh(dense(A)))
    want = []
    for (n_up, n_dn, m) in kondo.sector_blocks(n, n_elec, two_sz):
        H = q.csr_mat.hubbard(n, n_up, n_dn, chain(n), t=1.0, U=U, opts=q.make_opts(**PLAIN))
        want.extend(list(np.linalg.eigvalsh(dense(H))) * comb(n, m))
    want = np.sort(want)
    assert got.shape == want.shape
    assert np.abs(got - want).max() <= 1e-10 * max(1.0, np.abs(want).max())


# ---- explicit momentum states ----
def sort_parity(seq):
    """parity of the permutation that sorts seq (inversions mod 2)"""
    return sum(1 for a in range(len(seq)) for b in range(a + 1, len(seq)) if seq[a] > seq[b]) & 1


def translate_state(state, perm, n):
    """T_g |u d s> = sign |g(u) g(d) g(s)>: every operator moves to its image; putting each species back in order costs a sign"""
    u, d, s = state
    out = []
    par = 0
    for f, fermion in ((u, True), (d, True), (s, False)):
        imgs = [perm[i] for i in range(n) if (f >> i) & 1]
        if fermion:
            par ^= sort_parity(imgs)
        out.append(sum(1 << i for i in imgs))
    return (-1 if par else 1), tuple(out)


def word_of(state, n):
    return state[0] | (state[1] << n) | (state[2] << (2 * n))


class Momentum:
    """B[:, a] = (|G| |S_a|)^(-1/2) sum_g chi(g) T_g |a> for every orbit representative a (smallest word), ascending;
    zero[a] marks the states that vanish."""

    def __init__(self, n, n_elec, two_sz, perms, chars):
        self.states = states_of(n, n_elec, two_sz)
        index = {st: k for k, st in enumerate(self.states)}
        G = len(perms)
        rows, cols, vals, self.reps, zero = [], [], [], [], []
        for k, st in enumerate(self.states):
            imgs = [translate_state(st, p, n) for p in perms]
            idx = [index[t] for _, t in imgs]
            if min(idx) < k:
                continue
            a = len(self.reps)
            self.reps.append(word_of(st, n))
            stab = sum(1 for i in idx if i == k)
            col = {}
            for g, i in enumerate(idx):
                col[i] = col.get(i, 0.0) + imgs[g][0] * chars[g] / np.sqrt(G * stab)
            zero.append(np.linalg.norm(list(col.values())) < 1e-9)
            for i, v in col.items():
                rows.append(i); cols.append(a); vals.append(v)
        self.zero = np.array(zero)
        self.B = sp.csc_matrix((vals, (rows, cols)), shape=(len(self.states), len(self.reps)), dtype=np.complex128)
        self.B = self.B.multiply(~self.zero[None, :]).tocsc()

    @property
    def dim(self):
        return len(self.reps)


def check_against_projection(n, n_elec, two_sz, T, U, perms, chars, H, opts):
    mb = Momentum(n, n_elec, two_sz, perms, chars)
    A = q.csr_mat.kondo_repr(n, n_elec, two_sz, None, perms, chars, U=U, terms=T, fake_pos=FAKE, opts=opts)
    assert A.dim == mb.dim
    got = dense(A)
    want = (mb.B.conj().T @ (H @ mb.B)).toarray()
    live = ~mb.zero
    scale = max(1.0, np.abs(want).max())
    diff = np.abs(got[np.ix_(live, live)] - want[np.ix_(live, live)]).max()
    left_out = mb.dim - np.count_nonzero(live)
    print("dim %d, %d zero-norm rows, max |delta| %.3e" % (mb.dim, left_out, diff))
    assert diff <= 1e-12 * scale
    fake_rows = [i for i in range(mb.dim) if abs(got[i, i] - (FAKE + i / mb.dim)) < 1e-12 and np.count_nonzero(got[i]) == 1]
    assert left_out == np.count_nonzero(mb.zero) == len(fake_rows)      # the rows left out are exactly the device's fake rows
    for i in np.flatnonzero(mb.zero):                  # decoupled rows: the fake diagonal only, and no column points at them
        row = got[i].copy()
        assert abs(row[i] - (FAKE + i / mb.dim)) < 1e-12
        row[i] = 0
        assert not row.any()
        assert not got[live][:, i].any()
    return mb, got


def test_chain6_sectors_against_explicit_momentum_states():
    L, n_elec, two_sz, U = 6, 6, 0, 0.8
    T = kondo.terms(L, chain(L), 1.0, 1.1, 0.3)
    H = full_csr(q.csr_mat.kondo(L, n_elec, two_sz, None, U=U, terms=T, opts=q.make_opts(**PLAIN)))
    n_zero = 0
    for m in range(L):
        perms, chars = chain_group(L, m)
        mb, _ = check_against_projection(L, n_elec, two_sz, T, U, perms, chars, H, None if m % 2 else q.make_opts(**PLAIN))
        n_zero += np.count_nonzero(mb.zero)
    assert n_zero > 0                                  # the zero-norm branch was exercised


def test_torus_3x2_sectors_against_explicit_momentum_states():
    Lx, Ly, n_elec, two_sz = 3, 2, 6, 0
    n = Lx * Ly
    T = kondo.terms(n, square_bonds(Lx, Ly), 1.0, 1.1)
    H = full_csr(q.csr_mat.kondo(n, n_elec, two_sz, None, terms=T, opts=q.make_opts(**PLAIN)))
    n_zero = 0
    for my in range(Ly):
        for mx in range(Lx):
            perms, chars = torus_group(Lx, Ly, mx, my)
            mb, _ = check_against_projection(n, n_elec, two_sz, T, 0.0, perms, chars, H, q.make_opts(**PLAIN))
            n_zero += np.count_nonzero(mb.zero)
    assert n_zero > 0


def test_flux_ring_sectors_against_explicit_momentum_states():
    """complex amplitudes and odd filling through the sector generator"""
    L, n_elec, two_sz, U = 4, 3, -1, 1.2
    T = kondo.Terms(flux_terms(L, 0.41), [0.7] * L, [1.3] * L, [(i, (i + 1) % L, 0.2, 0.5) for i in range(L)])
    H = full_csr(q.csr_mat.kondo(L, n_elec, two_sz, None, U=U, terms=T, opts=q.make_opts(**PLAIN)))
    assert_entries(H, reference_H(L, n_elec, two_sz, T, U))
    for m in range(L):
        perms, chars = chain_group(L, m)
        check_against_projection(L, n_elec, two_sz, T, U, perms, chars, H, q.make_opts(**PLAIN))


def test_joined_sector_spectra_equal_the_full_sector():
    L, n_elec, two_sz = 6, 4, 0
    T = kondo.terms(L, chain(L), 1.0, 1.1)
    full = np.linalg.eigvalsh(dense(q.csr_mat.kondo(L, n_elec, two_sz, None, terms=T, opts=q.make_opts(**PLAIN))))
    ev, removed = [], 0
    for m in range(L):
        perms, chars = chain_group(L, m)
        A = q.csr_mat.kondo_repr(L, n_elec, two_sz, None, perms, chars, terms=T, fake_pos=FAKE, opts=q.make_opts(**PLAIN))
        mb = Momentum(L, n_elec, two_sz, perms, chars)
        M = dense(A)[np.ix_(~mb.zero, ~mb.zero)]
        removed += np.count_nonzero(mb.zero)
        ev.extend(np.linalg.eigvalsh(M))
    got = np.sort(ev)
    print("full dim %d, joined %d, fake rows removed %d" % (full.size, got.size, removed))
    assert got.shape == full.shape and np.abs(got - full).max() <= 1e-10 * max(1.0, np.abs(full).max())


def test_reference_energies_of_the_L8_chain_by_momentum():
    ref = GOLDEN["chain_L8_sz0_by_momentum"]
    L = ref["L"]
    E = {}
    for m in range(L):
        perms, chars = chain_group(L, m)
        A = q.csr_mat.kondo_repr(L, ref["n_elec"], ref["two_sz"], chain(L), perms, chars, t=ref["t"], J_K=ref["J_K"])
        E[m] = q.locate_E0_lanczos(A, nev=1, ncv=0).E0
        print("k = %d: dim %d, E0 = %.10f" % (m, A.dim, E[m]))
        A.destroy()
    for m, e in ref["E0_by_k"].items():
        assert abs(E[int(m)] - e) < GOLDEN["tolerance"], (m, E[int(m)], e)
    for m in range(1, L // 2):
        assert abs(E[m] - E[L - m]) < 1e-9, m


def spmv(A, x):
    y = np.empty_like(x)
    A.MultMv(x, y)
    return y


def test_coded_and_plain_formats_and_shards():
    L, m = 6, 1
    perms, chars = chain_group(L, m)
    kw = dict(t=1.0, J_K=1.1, J_RKKY=0.3, U=0.7)
    rng = np.random.default_rng(5)
    for make in (lambda **o: q.csr_mat.kondo(L, L, 0, chain(L), **kw, **o),
                 lambda **o: q.csr_mat.kondo_repr(L, L, 0, chain(L), perms, chars, **kw, **o)):
        P, Cd = make(opts=q.make_opts(**PLAIN)), make()
        assert P.info().value_dict == 0 and Cd.info().value_dict > 0
        x = rng.normal(size=P.dim) + 1j * rng.normal(size=P.dim)
        yp, yc = spmv(P, x), spmv(Cd, x)
        print("coded vs plain: %.3e relative" % (np.abs(yp - yc).max() / np.abs(yp).max()))
        assert np.abs(yp - yc).max() <= 1e-12 * np.abs(yp).max()
    P = q.csr_mat.kondo_repr(L, L, 0, chain(L), perms, chars, opts=q.make_opts(**PLAIN), **kw)
    ia, ja, val = P.download()
    dim = P.dim
    uniform = [q.csr_mat.kondo_repr(L, L, 0, chain(L), perms, chars, shard=(r, 3), opts=q.make_opts(**PLAIN), **kw) for r in range(3)]
    cuts = [0, dim // 5, dim // 5 + 7, dim]
    custom = [q.csr_mat.kondo_repr(L, L, 0, chain(L), perms, chars, shard=(r, 3), row_cuts=cuts, opts=q.make_opts(**PLAIN), **kw)
              for r in range(3)]
    for parts in (uniform, custom):
        rows = [p.download() for p in parts]
        assert all(p.info().ncols == dim for p in parts)
        got_ia = np.concatenate([[0]] + [r[0][1:] + sum(x[0][-1] for x in rows[:k]) for k, r in enumerate(rows)])
        assert np.array_equal(got_ia, ia)
        assert np.array_equal(np.concatenate([r[1] for r in rows]), ja)
        assert np.array_equal(np.concatenate([r[2] for r in rows]), val)


@pytest.mark.parametrize("kind", ["local_sz", "electron_sz", "density"])
def test_operator_times_vector_against_dense_projection(kind):
    L, n_elec, two_sz = 6, 6, 0
    rng = np.random.default_rng(17)
    mat = q.csr_mat.kondo(L, n_elec, two_sz, chain(L))               # any handle of the device: vectors are allocated through it
    states = states_of(L, n_elec, two_sz)
    for m, mq in ((0, 3), (1, 2), (2, 5), (3, 3), (4, 1)):
        perms, chars = chain_group(L, m)
        phase = np.exp(2j * np.pi * mq * np.arange(L) / L)
        c = 0.7 * phase
        zero = np.zeros(L)
        cu, cd, cs = {"local_sz": (zero, zero, c), "electron_sz": (0.5 * c, -0.5 * c, zero), "density": (c, c, zero)}[kind]
        chars_new = chars * phase                                    # eta(t) = c_{s+t} / c_s
        src, dst = Momentum(L, n_elec, two_sz, perms, chars), Momentum(L, n_elec, two_sz, perms, chars_new)
        assert src.dim == dst.dim
        diag = np.array([sum(cu[i] * ((u >> i) & 1) + cd[i] * ((d >> i) & 1) + cs[i] * (-0.5 if (s >> i) & 1 else 0.5) for i in range(L))
                         for (u, d, s) in states])
        x = rng.normal(size=src.dim) + 1j * rng.normal(size=src.dim)
        vx, vy = q.DeviceVec(mat, src.dim), q.DeviceVec(mat, dst.dim)
        try:
            vx.upload(x)
            assert q.moprXvec_diag_kondo_repr(L, n_elec, two_sz, perms, chars_new, cu, cd, cs, vx.ptr, vy.ptr) == dst.dim
            y = vy.download()
        finally:
            vx.free()
            vy.free()
        want = dst.B.conj().T @ (diag * (src.B @ x))
        err = np.abs(y - want).max() / max(1.0, np.abs(want).max())
        print("k %d -> q %d: %.3e relative, %d zero-norm targets" % (m, mq, err, np.count_nonzero(dst.zero)))
        assert err <= 1e-12, (m, mq)
        assert not y[dst.zero].any()


def test_local_singlet_correlation_of_the_ground_state():
    """<psi0| S_i . s_i |psi0> through an operator with no hops, spmv and dotc, against the dense ground state"""
    L, J_K = 4, 4.0
    H = dense(q.csr_mat.kondo(L, L, 0, chain(L), t=1.0, J_K=J_K, opts=q.make_opts(**PLAIN)))
    ev, vec = np.linalg.eigh(H)
    assert ev[1] - ev[0] > 1e-3
    psi = np.ascontiguousarray(vec[:, 0])
    for i in range(L):
        T = kondo.local_singlet_terms(L, i)
        O = q.csr_mat.kondo(L, L, 0, None, terms=T)
        vp, vt = q.DeviceVec(O, O.dim), q.DeviceVec(O, O.dim)
        try:
            vp.upload(psi)
            O.spmv(vp.ptr, vt.ptr)
            got = O.dotc(vp.ptr, vt.ptr)
        finally:
            vp.free()
            vt.free()
        want = np.vdot(psi, reference_H(L, L, 0, T) @ psi)
        print("site %d: <S.s> = %.12f (dense %.12f)" % (i, got.real, want.real))
        assert abs(got - want) < 1e-10
        assert -0.75 - 1e-12 <= got.real < 0.0                        # antiferromagnetic coupling; -3/4 is the local singlet


def test_L10_chain_full_sector_against_its_momentum_sectors():
    """Chain L = 10, n_elec = 10, S^z = 0 (38,165,260 states): E0 of the full sector (qbh_gen_kondo) equals the minimum over
    all ten momenta of the E0 of qbh_gen_kondo_repr, to 1e-9.  Two device paths that share only the term checks.
    Measured on one MI355X: the full sector (nnz 552,723,100) builds in 0.2 s, every k-sector (dim 3,816,756) in 0.1 s, the
    whole test takes under 4 s, so no sector is left out; E0 = -14.3299002203 lies at k = pi."""
    L = 10
    t0 = time.time()
    F = q.csr_mat.kondo(L, L, 0, chain(L), t=1.0, J_K=1.1)
    assert F.dim == kondo.sector_dim(L, L, 0) == 38165260
    print("full sector: dim %d nnz %d built in %.1f s" % (F.dim, F.nnz, time.time() - t0))
    E_full = q.locate_E0_lanczos(F, nev=1, ncv=0, maxit=300).E0
    F.destroy()
    print("full sector E0 = %.10f after %.1f s" % (E_full, time.time() - t0))
    E = []
    for m in range(L):
        perms, chars = chain_group(L, m)
        A = q.csr_mat.kondo_repr(L, L, 0, chain(L), perms, chars, t=1.0, J_K=1.1)
        E.append(q.locate_E0_lanczos(A, nev=1, ncv=0, maxit=300).E0)
        print("k = %d: dim %d nnz %d E0 = %.10f (%.1f s)" % (m, A.dim, A.nnz, E[-1], time.time() - t0))
        A.destroy()
    assert abs(min(E) - E_full) < 1e-9, (min(E), E_full)
