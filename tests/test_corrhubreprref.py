"""Pins tests/corrhubreprref.py (the longdouble reference of qbh_corr_hubbard_repr_dev, from representatives) against the explicit
route: unfold the sector state to the full space with the fermion signs, move it to the order of qbh_gen_hubbard and evaluate the
operator definitions of tests/corrref.py there.  Both sides are longdouble; they share the enumeration (secforms._images: images
and parities) and nothing of the formulas.  Dimensions and zero-norm counts are checked against secforms.build.  Also pins that the
comparison rejects the faults a fermion sector formula invites."""
import numpy as np
import pytest

import corrhubreprref as hr
import secforms

TOL = 1e-15                  # both routes sum at most a few thousand longdouble terms of a vector of norm 1

K42 = [(kx, ky) for kx in range(4) for ky in range(2)]
CASES = {
    # name: (n, nu, nd, (perms, chars), no_double, dim, zero-norm representatives)   (None: not pinned)
    "ring6_k0": (6, 2, 2, hr.ring(6, 0), False, 39, 0),
    "ring6_k1": (6, 2, 2, hr.ring(6, 1), False, 39, 3),
    "ring6_k3": (6, 2, 2, hr.ring(6, 3), False, 39, 3),
    "ring4_2+0_k0": (4, 2, 0, hr.ring(4, 0), False, 2, 1),           # {0, 2} is dead only because T^2 carries the sign -1
    "ring4_2+0_k1": (4, 2, 0, hr.ring(4, 1), False, 2, 0),
    "torus3x2_k00": (6, 2, 1, hr.torus(3, 2, 0, 0), False, 15, None),
    "torus3x2_k11": (6, 2, 1, hr.torus(3, 2, 1, 1), False, 15, None),
    "dihedral6_trivial": (6, 2, 2, hr.dihedral(6, False), False, 24, 2),
    "dihedral6_sign": (6, 2, 2, hr.dihedral(6, True), False, 24, 7),
    "no_symmetry": (5, 2, 1, hr.identity(5), False, 50, 0),
    "ring6_3+0_k0": (6, 3, 0, hr.ring(6, 0), False, None, None),      # one species empty
    "ring6_3+0_k2": (6, 3, 0, hr.ring(6, 2), False, None, None),
    "ring6_tj_k0": (6, 2, 2, hr.ring(6, 0), True, None, None),
    "ring6_tj_k1": (6, 2, 2, hr.ring(6, 1), True, None, None),
}
for _kx, _ky in K42:
    CASES["4x2_k%d%d" % (_kx, _ky)] = (8, 4, 4, hr.torus(4, 2, _kx, _ky), False, 628, None)


def _vector(dim, seed):
    """random, complex, NOT normalised, garbage at the zero-norm representatives included (both routes ignore it)"""
    rng = np.random.default_rng(seed)
    return (rng.normal(size=dim) + 1j * rng.normal(size=dim)) * 0.3


def _worst(a, b):
    return max(float(np.max(np.abs(np.asarray(a[k]) - np.asarray(b[k])))) for k in hr.KEYS)


def _explicit(case, x):
    """corrref.hubbard on the unfolded state, with norm2 = the weight of the live representatives (the unfolded columns are
    orthonormal, so the two agree -- which is part of what is pinned)"""
    n, nu, nd, (perms, chars), nod = case[:5]
    return hr.explicit(n, nu, nd, perms, chars, x, nod)


@pytest.mark.parametrize("name", sorted(CASES))
def test_reference_equals_the_unfolded_state(name):
    n, nu, nd, (perms, chars), nod, dim, n_zero = CASES[name]
    S = hr.sector(n, nu, nd, perms, chars, nod)
    if dim is not None:
        assert S.dim == dim
    if n_zero is not None:
        assert int(S.zero.sum()) == n_zero
    x = _vector(S.dim, 5)
    ref, exp = hr.hubbard_repr(n, nu, nd, perms, chars, x, nod), _explicit(CASES[name], x)
    scale = float(ref["norm2"])
    err = _worst(ref, exp) / scale
    print("%s: dim %d, %d zero-norm, worst |reference - explicit| / norm2 = %.3g" % (name, S.dim, int(S.zero.sum()), err))
    assert err < TOL
    # what the call promises of its arrays
    assert np.max(np.abs(ref["hop"] - ref["hop"].conj().transpose(0, 2, 1))) < TOL and np.max(np.abs(ref["flip"] - ref["flip"].conj().T)) < TOL
    assert np.max(np.abs(ref["nn"][1] - ref["nn"][2].T)) < TOL
    assert np.max(np.abs(ref["nn"][0] - ref["nn"][0].T)) < TOL and np.max(np.abs(ref["nn"][3] - ref["nn"][3].T)) < TOL
    for g in range(len(perms)):
        pg = np.asarray(perms[g])
        assert np.max(np.abs(ref["flip"][np.ix_(pg, pg)] - ref["flip"])) < TOL
        assert np.max(np.abs(ref["hop"][:, pg][:, :, pg] - ref["hop"])) < TOL and np.max(np.abs(ref["nn"][:, pg][:, :, pg] - ref["nn"])) < TOL
    for k in ("dens", "nn", "hop", "flip"):
        assert np.all(np.abs(ref[k]) <= ref["A"][k] * (1 + 1e-15))
    assert abs(float(np.sum(ref["dens"][0])) - nu * scale) < 1e-14 * scale * n and abs(float(np.sum(ref["dens"][1])) - nd * scale) < 1e-14 * scale * n


def test_zero_norm_counts_of_the_4x2_momenta():
    counts = sorted(int(hr.sector(8, 4, 4, *hr.torus(4, 2, kx, ky)).zero.sum()) for kx, ky in K42)
    assert counts == [0, 4, 20, 20, 20, 20, 20, 20]
    assert int(hr.sector(8, 4, 4, *hr.torus(4, 2, 0, 0)).zero.sum()) == 0


def test_ring4_two_up_particles_by_hand():
    """ring of 4, two up particles: the representatives are {0,1} (word 3) and {0,2} (word 5).  T^2 maps {0,2} to itself with the
    sign -1 (the two images swap), so its norm is 1 + (-1) chi(2): zero at k = 0 (a spin state there is alive), 2 at k = 1."""
    for k, dead in ((0, True), (1, False)):
        S = hr.sector(4, 2, 0, *hr.ring(4, k))
        assert list(S.reps) == [3, 5] and list(S.nstab) == [1, 2]
        assert bool(S.zero[1]) == dead and not S.zero[0]


@pytest.mark.parametrize("name,case,ik", [("ring6", "ring6", None), ("4x2", "4x2_4+4", 3), ("4x2", "4x2_4+4", 0)])
def test_enumeration_equals_secforms_build(name, case, ik):
    """dim, representatives, |S_a| and the live rows against the assembly reference of the sector operator"""
    if name == "ring6":
        todo = [(6, 2, 2, hr.ring(6, k)) for k in (0, 1, 3)] + [(6, 2, 2, hr.dihedral(6, s)) for s in (False, True)] + \
               [(6, 2, 1, hr.torus(3, 2, 1, 1))]
    else:
        perms, chars = secforms.symmetry(case, ik)
        todo = [(8, 4, 4, (np.asarray(perms, dtype=np.int32), np.asarray(chars, dtype=np.complex128)))]
    for n, nu, nd, (perms, chars) in todo:
        sec = secforms.build(n, nu, nd, perms, chars, [], 0.0)
        S = hr.sector(n, nu, nd, perms, chars)
        assert S.dim == sec.dim and np.array_equal(S.reps, sec.reps) and np.array_equal(S.nstab, sec.S)
        assert np.array_equal(~S.zero, sec.alive)


FAULT_CASES = [("chi_not_conjugated", "ring6_k1"), ("no_sigma", "ring6_k1"), ("no_sigma", "4x2_k10"), ("no_hop_sign", "ring6_k0"),
               ("no_sqrt", "ring6_k0"), ("no_sqrt", "dihedral6_trivial"), ("zero_norm_counted", "ring6_k1"),
               ("zero_norm_counted", "ring4_2+0_k0"), ("ud_swapped", "torus3x2_k11")]


@pytest.mark.parametrize("fault,name", FAULT_CASES)
def test_comparison_rejects_the_faults(fault, name):
    n, nu, nd, (perms, chars), nod = CASES[name][:5]
    S = hr.sector(n, nu, nd, perms, chars, nod)
    x = _vector(S.dim, 9)
    exp = _explicit(CASES[name], x)
    bad = hr.hubbard_repr(n, nu, nd, perms, chars, x, nod, fault=fault)
    rel = _worst(bad, exp) / float(exp["norm2"])
    print("%s on %s: worst |faulty - explicit| / norm2 = %.3g" % (fault, name, rel))
    assert rel > 1e-4                                        # an error of the size of the values, not of their rounding
