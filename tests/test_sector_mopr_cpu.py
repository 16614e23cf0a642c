"""CPU checks of the operators between momentum sectors of the spin-1/2 and Hubbard families (qbh_mopr_sz_repr_dev,
qbh_mopr_flip_repr_dev, qbh_mopr_diag_hubrepr_dev, qbh_mopr_c_hubrepr_dev): every argument, symmetry, character and size check
returns its documented code before the device is looked for (QBH_ENODEVICE = -2 here once all of them pass).  The Kondo and
d-level entry points of the same file are pinned by test_kondo_cpu.py and test_qudit_repr_cpu.py."""
import ctypes as C
from math import comb

import numpy as np
import pytest

from quantum_basis_amd import _lib

EINVAL, ENODEVICE, EUNSUPP = -1, -2, -9
OK_HERE = (0, ENODEVICE)                     # ok on a GPU box, no device here
L = 6
FAKE = C.c_void_p(64)                        # never dereferenced: every refusal asked for here comes before the device is looked for
_VECS = []


def _vectors():
    """The two vectors of a call.  Where there is a device a call that passes every check runs, so they are real there (the
    largest sector a test lets through has fewer than 2^20 representatives); without one nothing ever looks at them."""
    lib = _lib.lib()
    if lib.qbh_device_count() <= 0:
        return FAKE, FAKE
    while len(_VECS) < 2:
        v = C.c_void_p()
        assert lib.qbh_vec_alloc(C.byref(v), C.c_int64(1 << 20)) == 0
        _VECS.append(v)
    return _VECS[0], _VECS[1]


@pytest.fixture(scope="module", autouse=True)
def _free_vectors():
    yield
    while _VECS:
        _lib.lib().qbh_vec_free(_VECS.pop())


def translations(n, count=None):
    count = n if count is None else count
    perms = np.array([[(s + t) % n for s in range(n)] for t in range(count)], dtype=np.int32)
    chars = np.exp(-2j * np.pi * np.arange(count) / n)
    return perms, chars


def _err():
    return _lib.lib().qbh_last_error().decode()


def _a(x, dtype):
    return None if x is None else np.ascontiguousarray(x, dtype=dtype)


def _p(x):
    return None if x is None else x.ctypes.data


class Call:
    """One entry point with valid default arguments on the ring of 6; keyword arguments replace single ones."""

    def __init__(self, name):
        self.name = name
        perms, chars = translations(L)
        q1 = np.exp(2j * np.pi * np.arange(L) / L)
        self.defaults = dict(n_sites=L, n_a=3, n_b=3, species=0, kind=-1, n_trans=None, perms=perms, chars_old=chars, chars_new=chars * q1,
                             coef=q1, coef_dn=q1, vec_old=_vectors()[0], vec_new=_vectors()[1])

    def __call__(self, **kw):
        a = dict(self.defaults, **kw)
        perms, co, cn = _a(a["perms"], np.int32), _a(a["chars_old"], np.complex128), _a(a["chars_new"], np.complex128)
        cf, cd = _a(a["coef"], np.complex128), _a(a["coef_dn"], np.complex128)
        nt = a["n_trans"] if a["n_trans"] is not None else len(cn)
        lib = _lib.lib()
        n, vo, vn = a["n_sites"], a["vec_old"], a["vec_new"]
        if self.name == "sz":
            return lib.qbh_mopr_sz_repr_dev(n, a["n_a"], nt, _p(perms), _p(cn), _p(cf), vo, vn, None)
        if self.name == "flip":
            return lib.qbh_mopr_flip_repr_dev(n, a["n_a"], a["kind"], nt, _p(perms), _p(co), _p(cn), _p(cf), vo, vn, None, None)
        if self.name == "diag":
            return lib.qbh_mopr_diag_hubrepr_dev(n, a["n_a"], a["n_b"], nt, _p(perms), _p(cn), _p(cf), _p(cd), vo, vn, None)
        return lib.qbh_mopr_c_hubrepr_dev(n, a["n_a"], a["n_b"], a["species"], a["kind"], nt, _p(perms), _p(co), _p(cn), _p(cf), vo, vn,
                                          None, None)


NAMES = ["sz", "flip", "diag", "c"]


@pytest.mark.parametrize("name", NAMES)
def test_null_pointers_and_bad_counts(name):
    call = Call(name)
    for key in ("perms", "chars_new", "coef", "vec_old", "vec_new") + (("chars_old",) if name in ("flip", "c") else ()) + \
            (("coef_dn",) if name == "diag" else ()):
        assert call(**{key: None, "n_trans": L}) == EINVAL, key
        assert "invalid argument" in _err()
    for kw in (dict(n_sites=0), dict(n_sites=63 if name in ("sz", "flip") else 32), dict(n_a=-1), dict(n_a=L + 1), dict(n_trans=0)):
        assert call(**kw) == EINVAL, kw
        assert "invalid argument" in _err()
    if name in ("diag", "c"):
        assert call(n_b=-1) == EINVAL and call(n_b=L + 1) == EINVAL
    if name in ("flip", "c"):
        assert call(kind=0) == EINVAL and call(kind=2) == EINVAL
    if name == "c":
        assert call(species=2) == EINVAL and "species" in _err()


@pytest.mark.parametrize("name", NAMES)
def test_symmetry_refusals(name):
    call = Call(name)
    perms, chars = translations(L)
    p2 = perms.copy()
    p2[2, 0] = p2[2, 1]
    assert call(perms=p2) == EINVAL and "not a site permutation" in _err()
    p2 = perms.copy()
    p2[3, 4] = L                              # an image outside the lattice
    assert call(perms=p2) == EINVAL and "not a site permutation" in _err()
    p2 = perms.copy()
    p2[0] = p2[1]
    assert call(perms=p2) == EINVAL and "identity" in _err()
    # 65 translations (a ring of 13 walked five times round); 64 pass
    p65, c65 = translations(13, 65)
    big = dict(n_sites=13, n_a=6, n_b=6, coef=np.ones(13), coef_dn=np.ones(13))
    assert call(perms=p65, chars_old=c65, chars_new=c65, **big) == EINVAL and "invalid argument" in _err()
    assert call(perms=p65[:64], chars_old=c65[:64], chars_new=c65[:64], **big) in OK_HERE


def test_a_target_sector_that_does_not_exist():
    assert Call("flip")(n_a=L, kind=-1) == EINVAL and "invalid argument" in _err()          # S^- with every spin down already
    assert Call("flip")(n_a=0, kind=+1) == EINVAL
    assert Call("c")(n_a=0, species=0, kind=-1) == EINVAL and "does not exist" in _err()
    assert Call("c")(n_b=L, species=1, kind=+1) == EINVAL and "does not exist" in _err()
    assert Call("c")(n_a=0, species=1, kind=-1) in OK_HERE                                  # the other species is there


def test_hubbard_diagonal_coefficients_must_transform_with_one_character():
    call = Call("diag")
    q1 = np.exp(2j * np.pi * np.arange(L) / L)
    zero = np.zeros(L)
    lumpy = q1.copy()
    lumpy[3] *= 1.5
    assert call(coef=lumpy, coef_dn=zero) == EINVAL and "character" in _err() and "translation 1" in _err()
    assert call(coef=zero, coef_dn=lumpy) == EINVAL and "character" in _err()
    # each set transforms with a character, but not with the same one
    assert call(coef=q1, coef_dn=q1 ** 2) == EINVAL and "character" in _err()
    assert call(coef=q1, coef_dn=zero) in OK_HERE
    assert call(coef=zero, coef_dn=zero) in OK_HERE
    assert call(coef=1e3 * q1, coef_dn=-1e3 * q1) in OK_HERE
    # the permutations are looked at first: a bad one is reported as such, whatever the coefficients
    p2 = translations(L)[0].copy()
    p2[2, 0] = L
    assert call(perms=p2, coef=lumpy) == EINVAL and "not a site permutation" in _err()


def test_the_other_three_take_their_target_characters_from_the_caller():
    lumpy = np.exp(2j * np.pi * np.arange(L) / L)
    lumpy[3] *= 1.5
    for name in ("sz", "flip", "c"):
        assert Call(name)(coef=lumpy) in OK_HERE, name


def test_sectors_too_large_to_enumerate():
    one = (np.arange(44, dtype=np.int32)[None, :], np.ones(1))
    big = dict(n_sites=44, perms=one[0], chars_old=one[1], chars_new=one[1], coef=np.ones(44), coef_dn=np.ones(44))
    assert comb(44, 22) >= 2 ** 40 and comb(44, 19) >= 2 ** 40 > comb(44, 18)
    assert Call("sz")(n_a=22, **big) == EUNSUPP and "too large" in _err()
    assert Call("flip")(n_a=22, **big) == EUNSUPP and "too large" in _err()
    assert Call("flip")(n_a=18, kind=-1, **big) == EUNSUPP and "too large" in _err()        # the target alone is too large
    assert Call("flip")(n_a=19, kind=+1, **big) == EUNSUPP and "too large" in _err()        # the source alone
    hub = dict(big, n_sites=24, perms=one[0][:, :24], coef=np.ones(24), coef_dn=np.ones(24))
    assert comb(24, 12) ** 2 >= 2 ** 40 > comb(24, 12) * comb(24, 7) and comb(24, 12) * comb(24, 8) >= 2 ** 40
    assert Call("diag")(n_a=12, n_b=12, **hub) == EUNSUPP and "too large" in _err()
    assert Call("c")(n_a=12, n_b=12, **hub) == EUNSUPP and "too large" in _err()
    assert Call("c")(n_a=12, n_b=7, species=1, kind=+1, **hub) == EUNSUPP and "too large" in _err()      # the target alone


@pytest.mark.parametrize("name", NAMES)
def test_a_valid_call_passes_every_check(name):
    assert Call(name)() in OK_HERE, _err()
    assert Call(name)(kind=+1) in OK_HERE, _err()
