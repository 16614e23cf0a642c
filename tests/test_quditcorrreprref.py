"""Pins tests/quditcorrreprref.py (the longdouble reference of qbh_corr_qudit_repr_dev, from representatives and classes) against
the explicit route: unfold the sector state to the full sector in generator order and evaluate the operator definitions of
tests/quditcorrref.py there.  Both sides are longdouble; they share the packing of the words and nothing of the formulas.  Also pins
that the comparison rejects the faults a sector formula with classes invites, and that d = 2 is the spin-1/2 sector reference."""
import numpy as np
import pytest

import corrreprref
import quditcorrreprref as qr
import quditforms as qf

TOL = 1e-15                  # both routes sum at most a few thousand longdouble terms of a vector of norm below 1

# tables with a zero and negative entries in g, an h that changes sign, and a lower with a zero entry where d allows one
def _tables(d, K=2):
    rng = np.random.default_rng(100 + d)
    diag = rng.normal(size=(K, d))
    h = np.linspace(1.0, -0.75, d)
    g = np.where(np.arange(d) % 3 == 1, 0.0, np.where(np.arange(d) % 2 == 0, -1.25, 0.5))
    lower = np.append(0.0, np.sqrt(np.arange(1, d)) * np.where(np.arange(1, d) == 3, 0.0, 1.0))
    return diag, (h, g), lower


CASES = {
    # name: (n, d, total, (perms, chars))
    "ring5_d3_k0": (5, 3, 5, qr.ring(5, 0)),
    "ring5_d3_k1": (5, 3, 5, qr.ring(5, 1)),
    "ring5_d3_k2": (5, 3, 4, qr.ring(5, 2)),
    "ring6_d3_k0": (6, 3, 6, qr.ring(6, 0)),
    "ring6_d3_k1": (6, 3, 6, qr.ring(6, 1)),
    "ring6_d3_k2": (6, 3, 5, qr.ring(6, 2)),
    "ring6_d3_k3": (6, 3, 6, qr.ring(6, 3)),
    "ring5_d4_k1": (5, 4, 6, qr.ring(5, 1)),
    "ring6_d4_k3": (6, 4, 7, qr.ring(6, 3)),
    "ring6_d4_k0": (6, 4, 9, qr.ring(6, 0)),
    "cells3x2_d3_k0": (6, 3, 6, qr.cells_chain(3, 2, 0)),
    "cells3x2_d3_k1": (6, 3, 5, qr.cells_chain(3, 2, 1)),
    "cells2x3_d4_k1": (6, 4, 8, qr.cells_chain(2, 3, 1)),
    "dihedral6_d3_plus": (6, 3, 6, qr.dihedral(6, False)),
    "dihedral6_d3_minus": (6, 3, 6, qr.dihedral(6, True)),
    "dihedral5_d4_minus": (5, 4, 7, qr.dihedral(5, True)),
    "torus3x2_d3_k11": (6, 3, 6, qr.torus(3, 2, 1, 1)),
    "torus3x2_d4_k00": (6, 4, 5, qr.torus(3, 2, 0, 0)),
    "trivial_d3": (4, 3, 4, qr.identity(4)),
    "trivial_d5": (4, 5, 7, qr.identity(4)),
    "ring6_d2_k1": (6, 2, 3, qr.ring(6, 1)),
    "ring6_d2_k3": (6, 2, 3, qr.ring(6, 3)),
    "ring4_d5_k1": (4, 5, 8, qr.ring(4, 1)),
    "ring4_d5_k2": (4, 5, 7, qr.ring(4, 2)),
    "ring4_d8_k0": (4, 8, 13, qr.ring(4, 0)),
    "ring4_d8_k1": (4, 8, 14, qr.ring(4, 1)),
    "ring3_d8_k1": (3, 8, 10, qr.ring(3, 1)),
}


def _vector(dim, seed):
    """random, complex, NOT normalised, garbage at the zero-norm representatives included (both routes ignore it)"""
    rng = np.random.default_rng(seed)
    return (rng.normal(size=dim) + 1j * rng.normal(size=dim)) * 0.3


def _worst(a, b):
    return max(float(np.max(np.abs(np.asarray(a[k]) - np.asarray(b[k])))) for k in qr.KEYS)


def _both(name, x=None, fault=None, real=False):
    n, d, total, (perms, chars) = CASES[name]
    S = qr.sector(n, d, total, perms, chars)
    x = _vector(S.dim, 5) if x is None else x
    if real:
        x = x.real
    diag, string, lower = _tables(d)
    ref = qr.qudit_repr(n, d, total, perms, chars, x, diag=diag, string=string, lower=lower, fault=fault)
    exp = qr.explicit(n, d, total, perms, chars, x, diag=diag, string=string, lower=lower)
    return S, ref, exp


@pytest.mark.parametrize("name", sorted(CASES))
def test_reference_equals_the_unfolded_state(name):
    n, d, total, (perms, chars) = CASES[name]
    S, ref, exp = _both(name)
    assert np.array_equal(qr.sector_keys(n, d, total), qf.words(n, d, total)[1])
    scale = float(ref["norm2"])
    err = _worst(ref, exp) / scale
    print("%s: dim %d, %d zero-norm, worst |reference - explicit| / norm2 = %.3g" % (name, S.dim, int(S.zero.sum()), err))
    assert err < TOL
    # what the call promises of its arrays
    assert np.max(np.abs(ref["aa"] - ref["aa"].conj().T)) < TOL and np.max(np.abs(ref["str"] - ref["str"].T)) < TOL
    assert np.max(np.abs(ref["dd"] - ref["dd"].transpose(1, 0, 3, 2))) < TOL
    for g in range(len(perms)):
        pg = np.asarray(perms[g])
        assert np.max(np.abs(ref["aa"][np.ix_(pg, pg)] - ref["aa"])) < TOL and np.max(np.abs(ref["pop"][pg] - ref["pop"])) < TOL
        assert np.max(np.abs(ref["dd"][:, :, pg][:, :, :, pg] - ref["dd"])) < TOL
    for k in ("pop", "dd", "str", "aa"):
        assert np.all(np.abs(ref[k]) <= ref["A"][k] * (1 + 1e-15))
    assert abs(float(np.sum(ref["pop"] @ np.arange(d))) - total * scale) < 1e-14 * scale * n * d


@pytest.mark.parametrize("name", [n for n in sorted(CASES) if np.all(np.asarray(CASES[n][3][1]).imag == 0)])
def test_real_vectors_at_real_characters_have_real_values(name):
    S, ref, exp = _both(name, real=True)
    assert _worst(ref, exp) / float(ref["norm2"]) < TOL
    assert np.max(np.abs(ref["aa"].imag)) < TOL * float(ref["norm2"])


def test_some_cases_have_zero_norm_representatives_and_self_mirror_classes():
    n, d, total, (perms, chars) = CASES["dihedral6_d3_minus"]
    assert qr.sector(n, d, total, perms, chars).zero.any()
    assert all(own for (_, _, own) in qr.pair_classes(6, np.asarray(perms)).values())
    own = [own for (_, _, own) in qr.pair_classes(6, np.asarray(CASES["ring6_d3_k1"][3][0])).values()]
    assert any(own) and not all(own)                         # the class r = N / 2 of a ring with rotations only
    # the images of an index interval on a torus are not all intervals
    mem = qr.string_members(6, np.asarray(CASES["torus3x2_d3_k11"][3][0]), 0, 2)
    assert any(m[2] != tuple(range(m[0] + 1, m[1])) for m in mem)


FAULT_CASES = [("zero_norm_counted", "ring6_d3_k1"), ("zero_norm_counted", "dihedral6_d3_minus"), ("chi_conjugated", "ring6_d3_k1"),
               ("chi_conjugated", "torus3x2_d3_k11"), ("no_sqrt", "ring6_d3_k0"), ("no_sqrt", "dihedral6_d3_plus"),
               ("one_orientation_in_self_mirror", "ring6_d3_k1"), ("one_orientation_in_self_mirror", "ring6_d4_k3"),
               ("string_middle_not_translated", "ring6_d3_k0"), ("string_middle_not_translated", "torus3x2_d3_k11"),
               ("dd_not_swapped_on_mirror", "ring6_d3_k2"), ("dd_not_swapped_on_mirror", "trivial_d3")]


@pytest.mark.parametrize("fault,name", FAULT_CASES)
def test_comparison_rejects_the_faults(fault, name):
    S, bad, exp = _both(name, x=None, fault=fault)
    rel = _worst(bad, exp) / float(exp["norm2"])
    print("%s on %s: worst |faulty - explicit| / norm2 = %.3g" % (fault, name, rel))
    assert rel > 1e-4                                        # an error of the size of the values, not of their rounding


@pytest.mark.parametrize("name", sorted(CASES))
def test_the_permutations_are_groups_so_orbits_are_images(name):
    n, _, _, (perms, _) = CASES[name]
    perms = np.asarray(perms)
    for i in range(n):
        for j in range(i + 1, n):
            assert qr.string_members(n, perms, i, j) == qr.string_members(n, perms, i, j, orbit=qr._closure)
            act = lambda g, x: (int(perms[g][x[0]]), int(perms[g][x[1]]))      # noqa: E731
            assert qr._orbit((i, j), act, len(perms)) == qr._closure((i, j), act, len(perms))


def test_every_fault_is_covered():
    assert {f for f, _ in FAULT_CASES} == set(qr.FAULTS)


@pytest.mark.parametrize("n,n_dn,sym", [(6, 3, qr.ring(6, 1)), (6, 2, qr.ring(6, 3)), (6, 3, qr.dihedral(6, True)),
                                        (6, 2, qr.torus(3, 2, 1, 0))])
def test_two_levels_are_the_spin_half_sector_reference(n, n_dn, sym):
    """d = 2, level 1 = bit set = spin down, lower = {0, 1} (A = S^+), diag = (S^z,): aa is pm, dd is zz, pop gives sz"""
    perms, chars = sym
    S = qr.sector(n, 2, n_dn, perms, chars)
    x = _vector(S.dim, 11)
    m = np.array([0.5, -0.5])
    ref = qr.qudit_repr(n, 2, n_dn, perms, chars, x, diag=(m,), lower=(0.0, 1.0))
    spin = corrreprref.spin_repr(n, n_dn, perms, chars, x)
    assert ref["dim"] == spin["dim"] and np.array_equal(ref["zero"], spin["zero"])
    scale = float(ref["norm2"])
    assert abs(ref["norm2"] - spin["norm2"]) < TOL * scale
    assert np.max(np.abs(ref["pop"] @ m - spin["sz"])) < TOL * scale and np.max(np.abs(ref["dd"][0, 0] - spin["zz"])) < TOL * scale
    assert np.max(np.abs(ref["aa"] - spin["pm"])) < TOL * scale
