"""tests/kondoops.py pinned by algebra, on L = 3 and 4 across sectors: the canonical anticommutators of the electrons, the
electron's spin flip as the product of its two factors, the commutator of the local spins' flips, and the orthonormality of
the momentum states.  No device."""
import itertools

import numpy as np
import pytest

import kondoops as ko
from quantum_basis_amd import kondo


def e(L, i):
    c = np.zeros(L, dtype=np.complex128)
    c[i] = 1.0
    return c


def sectors(L):
    """every nonempty (n_elec, two_sz)"""
    return [(ne, sz) for ne in range(2 * L + 1) for sz in range(-ne - L, ne + L + 1) if kondo.sector_dim(L, ne, sz) > 0]


def sec(L, ne, sz, _cache={}):
    if (L, ne, sz) not in _cache:
        _cache[(L, ne, sz)] = ko.Sector(L, ne, sz) if kondo.sector_dim(L, ne, sz) > 0 else None
    return _cache[(L, ne, sz)]


def mat(L, ne, sz, op, i, spin=False):
    """O_i from (ne, sz), or None if either sector is empty"""
    src, dst = sec(L, ne, sz), sec(L, *ko.target(ne, sz, op))
    if src is None or dst is None:
        return None
    if spin:
        return ko.operator(src, dst, op, None, e(L, i)).tocsr()
    return ko.operator(src, dst, op, e(L, i), None).tocsr()


def chain_ops(L, ne, sz, steps):
    """the product of one-site operators, applied right to left, from (ne, sz); steps = [(op, site, spin), ...] left to right;
    None if the path leaves the nonempty sectors (the product is then zero on this sector)"""
    M = None
    for op, i, spin in reversed(steps):
        m = mat(L, ne, sz, op, i, spin)
        if m is None:
            return None
        M = m if M is None else m @ M
        ne, sz = ko.target(ne, sz, op)
    return M


def dense(L, ne, sz, steps):
    """chain_ops as a dense array; a path through an empty sector is the zero map onto the final sector"""
    M = chain_ops(L, ne, sz, steps)
    if M is not None:
        return M.toarray()
    fe, fs = ne, sz
    for op, _, _ in steps:
        fe, fs = ko.target(fe, fs, op)
    return np.zeros((kondo.sector_dim(L, fe, fs), sec(L, ne, sz).N))


def test_targets():
    for op in ko.OPS:
        assert kondo.mopr_target(5, 1, op) == ko.target(5, 1, op)
    assert [ko.target(4, 0, op) for op in ko.OPS] == [(3, -1), (3, 1), (5, 1), (5, -1), (4, 2), (4, -2)]


@pytest.mark.parametrize("L", [3, 4])
def test_canonical_anticommutators(L):
    """{c_{i,s}, c^dag_{j,s'}} = delta_ij delta_ss' on every sector"""
    ann, cre = {0: ko.C_UP, 1: ko.C_DN}, {0: ko.CDAG_UP, 1: ko.CDAG_DN}
    checked = 0
    for (ne, sz) in sectors(L):
        N = sec(L, ne, sz).N
        for (i, si), (j, sj) in itertools.product(itertools.product(range(L), (0, 1)), repeat=2):
            a = dense(L, ne, sz, [(ann[si], i, False), (cre[sj], j, False)])
            b = dense(L, ne, sz, [(cre[sj], j, False), (ann[si], i, False)])
            want = np.eye(N) if (i, si) == (j, sj) else np.zeros(a.shape)      # si != sj: both orders end in (ne, sz -+ 2)
            assert np.array_equal(a + b, want), (L, ne, sz, i, si, j, sj)
            checked += 1
    assert checked > 100


@pytest.mark.parametrize("L", [3, 4])
def test_annihilators_anticommute(L):
    """{c_{i,s}, c_{j,s'}} = 0: the sign of the down operators counts the whole up field"""
    ann = {0: ko.C_UP, 1: ko.C_DN}
    for (ne, sz) in sectors(L):
        for (i, si), (j, sj) in itertools.product(itertools.product(range(L), (0, 1)), repeat=2):
            a = dense(L, ne, sz, [(ann[si], i, False), (ann[sj], j, False)])
            b = dense(L, ne, sz, [(ann[sj], j, False), (ann[si], i, False)])
            assert not (a + b).any(), (L, ne, sz, i, si, j, sj)


@pytest.mark.parametrize("L", [3, 4])
def test_electron_flip_is_the_product_of_its_factors(L):
    for (ne, sz) in sectors(L):
        for i in range(L):
            for op, steps in ((ko.SPIN_PLUS, [(ko.CDAG_UP, i, False), (ko.C_DN, i, False)]),
                              (ko.SPIN_MINUS, [(ko.CDAG_DN, i, False), (ko.C_UP, i, False)])):
                got, want = mat(L, ne, sz, op, i), dense(L, ne, sz, steps)
                if got is None:                            # no target sector: the product vanishes as well
                    assert not want.any()
                else:
                    assert np.array_equal(got.toarray(), want), (L, ne, sz, i, op)


@pytest.mark.parametrize("L", [3, 4])
def test_local_spin_flips_commute_to_twice_sz(L):
    """[S^+_i, S^-_j] = 2 S^z_i delta_ij, S^z = +1/2 where the bit of s is clear"""
    for (ne, sz) in sectors(L):
        s = sec(L, ne, sz)
        for i, j in itertools.product(range(L), repeat=2):
            a = dense(L, ne, sz, [(ko.SPIN_PLUS, i, True), (ko.SPIN_MINUS, j, True)])
            b = dense(L, ne, sz, [(ko.SPIN_MINUS, j, True), (ko.SPIN_PLUS, i, True)])
            want = np.diag(1.0 - 2.0 * ((s.s >> i) & 1)) if i == j else np.zeros((s.N, s.N))
            assert np.array_equal(a - b, want), (L, ne, sz, i, j)


@pytest.mark.parametrize("L", [3, 4])
def test_momentum_states_are_orthonormal(L):
    some_zero = False
    for (ne, sz) in sectors(L):
        s = sec(L, ne, sz)
        for m in range(L):
            mo = ko.Momentum(s, *ko.chain_group(L, m))
            B = mo.matrix()
            gram = (B.conj().T @ B).toarray()
            want = np.diag((~mo.zero).astype(float))
            assert np.abs(gram - want).max() < 1e-14, (L, ne, sz, m)
            some_zero |= bool(mo.zero.any())
            # expand / contract are B and B^dag
            x = np.random.default_rng(m).normal(size=mo.dim) + 0j
            assert np.abs(mo.expand(x.astype(ko.CLD)).astype(np.complex128) - B @ x).max() < 1e-14
        # the orbits of all momenta together span the sector
        assert sum(int((~ko.Momentum(s, *ko.chain_group(L, m)).zero).sum()) for m in range(L)) == s.N
    assert some_zero


def test_project_is_the_matrix_product():
    """project() against the explicit B_new^dag O B_old on the ring of 4, with its count and absolute sum"""
    L, ne, sz = 4, 4, 0
    src = sec(L, ne, sz)
    rng = np.random.default_rng(3)
    for op, m, qm in ((ko.C_UP, 1, 2), (ko.SPIN_MINUS, 0, 1), (ko.CDAG_DN, 2, 0)):
        dst = sec(L, *ko.target(ne, sz, op))
        ce = ko.chain_coef(L, qm)
        cs = ko.chain_coef(L, qm, 0.4) if op >= ko.SPIN_PLUS else None
        mo, mn = ko.Momentum(src, *ko.chain_group(L, m)), ko.Momentum(dst, *ko.chain_group(L, m - qm))
        x = rng.normal(size=mo.dim) + 1j * rng.normal(size=mo.dim)
        got, n_i, ab = ko.project(mo, mn, op, ce, cs, x)
        M = (mn.matrix().conj().T @ ko.operator(src, dst, op, ce, cs).tocsr() @ mo.matrix()).tocsr()
        assert np.abs(got.astype(np.complex128) - M @ x).max() < 1e-13
        assert np.all(ab.astype(float) + 1e-13 >= np.abs(M) @ np.abs(x))
        assert np.all(n_i >= np.diff(M.indptr)) and n_i.max() <= 2 * L      # duplicates merge in M, never the reverse
        # the coefficients carry the momentum to m - qm and to nowhere else
        other = ko.Momentum(dst, *ko.chain_group(L, m - qm + 1))
        leak = (other.matrix().conj().T @ ko.operator(src, dst, op, ce, cs).tocsr() @ mo.matrix())
        assert abs(leak).max() < 1e-13 if leak.nnz else True
