"""Pins tests/kondocorrreprref.py (the longdouble reference of qbh_corr_kondo_repr_dev, from representatives) against the explicit
route: unfold the sector state to the full sector with kondoops.Momentum.expand and evaluate the operator definitions of
tests/kondocorrref.py on the full state.  Both sides are longdouble; they share the enumeration of kondoops.Momentum and the
one-site primitives of kondoops, and nothing of the formulas: the explicit route knows no representative, no character and no
sqrt(|S_b|/|S_a|).  Also pins that the comparison rejects the faults a Kondo sector formula invites, and the edges the GPU test
relies on: zero-norm representatives, a class of site pairs that is its own mirror, le terms that cross the blocks of popcount(s)."""
import functools

import numpy as np
import pytest

import kondocorrref as kc
import kondocorrreprref as kr
import kondoops as ko

TOL = 2e-16                  # both routes sum at most a few thousand longdouble terms (2^-64 each) of a vector of norm2 ~ dim

CASES = {
    # name: (n, n_elec, two_sz, (perms, turns), representatives, zero-norm representatives)   (None: not pinned)
    "ring4_k0": (4, 2, 0, kr.ring(4, 0), 36, None),
    "ring4_k1": (4, 2, 0, kr.ring(4, 1), 36, None),
    "ring6_k0": (6, 6, 0, kr.ring(6, 0), 2544, 20),
    "ring6_k1": (6, 6, 0, kr.ring(6, 1), 2544, 6),
    "ring6_k3": (6, 6, 0, kr.ring(6, 3), 2544, 0),
    "torus3x2_k00": (6, 3, 1, kr.torus(3, 2, 0, 0), 595, None),
    "torus3x2_k11": (6, 3, 1, kr.torus(3, 2, 1, 1), 595, None),
    "dihedral6_trivial": (6, 4, 0, kr.dihedral(6, False), 714, 36),
    "dihedral6_sign": (6, 4, 0, kr.dihedral(6, True), 714, 12),
    "no_symmetry": (5, 3, 0, kr.identity(5), 1100, 0),
}


def _vector(dim, seed):
    """random, complex, NOT normalised, garbage at the zero-norm representatives included (both routes ignore it)"""
    rng = np.random.default_rng(seed)
    return (rng.normal(size=dim) + 1j * rng.normal(size=dim)) * 0.3


def _dim(name):
    n, ne, tz, (perms, turns) = CASES[name][:4]
    return ko.Momentum(ko.Sector(n, ne, tz), perms, turns).dim


@functools.lru_cache(maxsize=None)
def _explicit(name, seed):
    """kondocorrref.correlations on the unfolded state (clongdouble all the way)"""
    n, ne, tz, (perms, turns) = CASES[name][:4]
    mo = ko.Momentum(ko.Sector(n, ne, tz), perms, turns)
    full = mo.expand(_vector(mo.dim, seed).astype(kr.CLD))
    return kc.correlations(n, ne, tz, full)


def _worst(a, b):
    return max(float(np.max(np.abs(np.asarray(a[k]) - np.asarray(b[k])))) for k in kr.KEYS)


@pytest.mark.parametrize("name", sorted(CASES))
def test_reference_equals_the_unfolded_state(name):
    n, ne, tz, (perms, turns), dim, n_zero = CASES[name]
    x = _vector(_dim(name), 5)
    ref, exp = kr.kondo_repr(n, ne, tz, perms, turns, x), _explicit(name, 5)
    assert ref["dim"] == dim
    if n_zero is not None:
        assert int(ref["zero"].sum()) == n_zero
    scale = float(ref["norm2"])
    err = _worst(ref, exp) / scale
    print("%s: dim %d, %d zero-norm, worst |reference - explicit| / norm2 = %.3g" % (name, ref["dim"], int(ref["zero"].sum()), err))
    assert err < TOL
    # what the call promises of its arrays
    for k in ("hop", "ee", "ll"):
        assert np.max(np.abs(ref[k] - np.conj(np.swapaxes(ref[k], -1, -2)))) < TOL * scale
    assert np.max(np.abs(ref["nn"][1] - ref["nn"][2].T)) < TOL * scale and np.max(np.abs(ref["zz"] - ref["zz"].T)) < TOL * scale
    for pg in perms:
        pg = np.asarray(pg)
        for k in ("nn", "zn", "zz", "hop", "ee", "ll", "le"):
            assert np.max(np.abs(ref[k][..., pg, :][..., :, pg] - ref[k])) < TOL * scale, k
    for k in kr.KEYS[1:]:
        assert np.all(np.abs(ref[k]) <= ref["A"][k] * (1 + 1e-15) + 1e-18 * scale), k
    assert abs(float(np.sum(ref["site"][0] + ref["site"][1])) - ne * scale) < 1e-14 * scale * n
    sz_tot = float(np.sum(ref["site"][3]) + 0.5 * np.sum(ref["site"][0] - ref["site"][1]))
    assert abs(sz_tot - 0.5 * tz * scale) < 1e-14 * scale * n


FAULT_CASES = [("chi_not_conjugated", "ring6_k1"), ("chi_not_conjugated", "torus3x2_k11"), ("no_sigma", "ring6_k1"),
               ("no_sigma", "ring4_k1"), ("no_op_sign", "ring6_k0"), ("no_sqrt", "ring6_k0"), ("no_sqrt", "dihedral6_trivial"),
               ("zero_norm_counted", "ring6_k0"), ("zero_norm_counted", "dihedral6_sign"), ("le_transposed", "ring6_k1"),
               ("le_transposed", "no_symmetry"), ("zn_swapped", "torus3x2_k11"), ("zn_swapped", "ring6_k3"),
               ("s_untranslated", "ring6_k0"), ("s_untranslated", "ring4_k1")]


@pytest.mark.parametrize("fault,name", FAULT_CASES)
def test_comparison_rejects_the_faults(fault, name):
    n, ne, tz, (perms, turns) = CASES[name][:4]
    x = _vector(_dim(name), 9)
    exp = _explicit(name, 9)
    keys = {"le_transposed": ("norm2", "le"), "zn_swapped": ("norm2", "zn"), "zero_norm_counted": ("norm2", "site")}.get(fault, kr.KEYS)
    bad = kr.kondo_repr(n, ne, tz, perms, turns, x, fault=fault, keys=keys)
    rel = max(float(np.max(np.abs(np.asarray(bad[k]) - np.asarray(exp[k])))) for k in keys) / float(exp["norm2"])
    print("%s on %s: worst |faulty - explicit| / norm2 = %.3g" % (fault, name, rel))
    assert rel > 1e-4                                        # an error of the size of the values, not of their rounding


def test_a_class_that_is_its_own_mirror():
    """under the dihedral group (0, 1) and (1, 0) lie in one orbit: hop, ee and ll are real and symmetric; le is symmetric and, not
    being Hermitian, stays complex"""
    n, ne, tz, (perms, turns) = CASES["dihedral6_sign"][:4]
    assert any(pg[0] == 1 and pg[1] == 0 for pg in perms)
    ref = kr.kondo_repr(n, ne, tz, perms, turns, _vector(_dim("dihedral6_sign"), 5))
    scale = float(ref["norm2"])
    for k in ("hop", "ee", "ll", "le"):
        assert np.max(np.abs(ref[k] - np.swapaxes(ref[k], -1, -2))) < TOL * scale
        assert np.max(np.abs(ref[k].real)) > 1e-3 * scale
        if k != "le":                                            # symmetric and Hermitian: real; le is only symmetric
            assert np.max(np.abs(ref[k].imag)) < TOL * scale
    assert np.max(np.abs(ref["le"].imag)) > 1e-3 * scale


def test_le_terms_cross_the_blocks_of_the_sector():
    """every candidate of S^+_i s^-_j has one more down local spin and one more up electron than its row: its representative lies
    in another block (popcount(s), n_up) of the sector, and the entries are not small"""
    n, ne, tz, (perms, turns) = CASES["ring6_k1"][:4]
    sec = ko.Sector(n, ne, tz)
    mo = ko.Momentum(sec, perms, turns)
    U, D, S = sec.u[mo.reps], sec.d[mo.reps], sec.s[mo.reps]
    rows, pq, amp, cu, cd, cs = kr._candidates("le", n, U, D, S)
    assert len(rows) > 0
    assert np.all(ko.popcount(cs) == ko.popcount(S[rows]) + 1) and np.all(ko.popcount(cu) == ko.popcount(U[rows]) + 1)
    assert len(set(ko.popcount(S).tolist())) > 1               # the sector is a union of several blocks
    ref = kr.kondo_repr(n, ne, tz, perms, turns, _vector(mo.dim, 5), keys=("norm2", "le"))
    assert np.min(np.abs(ref["le"])) > 1e-4 * float(ref["norm2"])
    assert np.max(np.abs(ref["le"] - np.conj(ref["le"].T))) > 1e-4 * float(ref["norm2"])      # not Hermitian
