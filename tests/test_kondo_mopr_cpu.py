"""CPU checks of the operators between Kondo sectors, qbh_mopr_kondo_dev and qbh_mopr_kondo_repr_dev: the C ABI declares and
exports them, a fully valid call passes every check and then asks for the device (QBH_ENODEVICE = -2 here), and every refusal
comes back with its documented code and message BEFORE the device is looked for."""
import ctypes as C
import os
import re

import numpy as np

from quantum_basis_amd import _lib, kondo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, ENODEVICE, EUNSUPP = -1, -2, -9
OK_HERE = (0, ENODEVICE)                     # ok on a GPU box, no device here
FAKE_PTR = C.c_void_p(64)                    # stands for a device vector in calls that are refused before any device work
NAMES = ("qbh_mopr_kondo_dev", "qbh_mopr_kondo_repr_dev")


def test_header_declares_and_library_exports_both():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "qbhip.h")).read(), flags=re.S)
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, text)
        assert name in _lib.EXPORTS
        assert hasattr(_lib.lib(), name)
    for k, name in enumerate(("C_UP", "C_DN", "CDAG_UP", "CDAG_DN", "SPIN_PLUS", "SPIN_MINUS")):
        assert re.search(r"#define\s+QBH_KONDO_%s\s+%d\b" % (name, k), text)
        assert getattr(kondo, name) == k
    assert _lib.lib().qbh_version() == 601


def translations(L, n=None, m=0):
    n = L if n is None else n
    perms = np.array([[(s + t) % L for s in range(L)] for t in range(n)], dtype=np.int32)
    chars = np.exp(-2j * np.pi * m * np.arange(n) / L)
    return perms, chars


def wave(L, q, amp=1.0):
    return amp * np.exp(2j * np.pi * q * np.arange(L) / L)


def _ptr(a):
    return None if a is None else a.ctypes.data


def _call(name, n_sites, n_elec, two_sz, op, ce, cs, perms=None, chars=None, vec=True):
    """the raw entry point on host coefficient arrays, for calls that are refused: the vectors are never touched"""
    ce = None if ce is None else np.ascontiguousarray(ce, dtype=np.complex128)
    cs = None if cs is None else np.ascontiguousarray(cs, dtype=np.complex128)
    d0, d1 = C.c_int64(-1), C.c_int64(-1)
    v = FAKE_PTR if vec else None
    if name == "qbh_mopr_kondo_dev":
        return _lib.lib().qbh_mopr_kondo_dev(n_sites, n_elec, two_sz, op, _ptr(ce), _ptr(cs), v, v, C.byref(d0), C.byref(d1), None)
    if perms is None:
        perms, chars = translations(n_sites)
    p = np.ascontiguousarray(perms, dtype=np.int32)
    c = np.ascontiguousarray(chars, dtype=np.complex128)
    return _lib.lib().qbh_mopr_kondo_repr_dev(n_sites, n_elec, two_sz, op, len(c), p.ctypes.data, c.ctypes.data, _ptr(ce), _ptr(cs), v, v,
                                              C.byref(d0), C.byref(d1), None)


def _err():
    return _lib.lib().qbh_last_error().decode()


def _refused(code, text, *a, names=NAMES, **k):
    for name in names:
        rc = _call(name, *a, **k)
        assert rc == code, (name, rc, code, _err())
        assert name in _err() and text in _err(), (name, _err())


NO_DEVICE = _lib.lib().qbh_device_count() <= 0


def _valid(name, n_sites, n_elec, two_sz, op, ce, cs, perms=None, chars=None):
    """a call that passes every check: QBH_ENODEVICE without a device; with one it runs, on device vectors of the two sectors'
    word counts (the representatives are fewer)"""
    if NO_DEVICE:
        assert _call(name, n_sites, n_elec, two_sz, op, ce, cs, perms, chars) == ENODEVICE and "no HIP device" in _err(), (name, op)
        return
    from quantum_basis_amd import DeviceVec
    x = DeviceVec(None, kondo.sector_dim(n_sites, n_elec, two_sz))
    y = DeviceVec(None, kondo.sector_dim(n_sites, *kondo.mopr_target(n_elec, two_sz, op)))
    ce = None if ce is None else np.ascontiguousarray(ce, dtype=np.complex128)
    cs = None if cs is None else np.ascontiguousarray(cs, dtype=np.complex128)
    d0, d1 = C.c_int64(-1), C.c_int64(-1)
    if name == NAMES[0]:
        rc = _lib.lib().qbh_mopr_kondo_dev(n_sites, n_elec, two_sz, op, _ptr(ce), _ptr(cs), x.ptr, y.ptr, C.byref(d0), C.byref(d1), None)
    else:
        if perms is None:
            perms, chars = translations(n_sites)
        p = np.ascontiguousarray(perms, dtype=np.int32)
        c = np.ascontiguousarray(chars, dtype=np.complex128)
        rc = _lib.lib().qbh_mopr_kondo_repr_dev(n_sites, n_elec, two_sz, op, len(c), p.ctypes.data, c.ctypes.data, _ptr(ce), _ptr(cs),
                                                x.ptr, y.ptr, C.byref(d0), C.byref(d1), None)
    assert rc == 0, (name, op, _err())
    assert 0 < d0.value <= x.n and 0 < d1.value <= y.n
    x.free()
    y.free()


def test_a_valid_call_returns_ok_or_no_device():
    L = 6
    for op in range(4):
        for name in NAMES:
            _valid(name, L, 6, 0, op, wave(L, 1), None)
    for op in (4, 5):
        for ce, cs in ((wave(L, 2), None), (None, wave(L, 2)), (wave(L, 2), wave(L, 2, 0.3))):
            for name in NAMES:
                _valid(name, L, 6, 0, op, ce, cs)
    if NO_DEVICE:                                          # sizes nobody runs inside a test: only their checks
        # the chain L = 13 at half filling: 1.5e10 words, beyond the int32 columns of the stored form
        assert kondo.sector_dim(13, 13, 0) >= 2 ** 31
        for name in NAMES:
            _valid(name, 13, 13, 0, kondo.C_UP, wave(13, 1), None)
        # 64 translations are admitted (a ring of 13 walked nearly five times round)
        p64, c64 = translations(13, 64)
        _valid(NAMES[1], 13, 13, 0, kondo.C_UP, wave(13, 0), None, p64, c64)


def test_op_and_coefficient_sets():
    L = 4
    _refused(EINVAL, "op = 6", L, 4, 0, 6, wave(L, 0), None)
    _refused(EINVAL, "op = -1", L, 4, 0, -1, wave(L, 0), None)
    for op in range(4):
        _refused(EINVAL, "coef_spin must be NULL", L, 4, 0, op, wave(L, 0), wave(L, 0))
        _refused(EINVAL, "coef_elec", L, 4, 0, op, None, None)
    for op in (4, 5):
        _refused(EINVAL, "needs coef_elec, coef_spin or both", L, 4, 0, op, None, None)
    _refused(EINVAL, "a vector is NULL", L, 4, 0, 0, wave(L, 0), None, vec=False)


def test_bad_shape_and_parity():
    _refused(EINVAL, "n_sites", 0, 0, 0, 0, np.ones(1), None, perms=[[0]], chars=[1.0])
    _refused(EINVAL, "n_sites", 22, 22, 0, 0, np.ones(22), None)
    _refused(EINVAL, "n_elec", 4, -1, 1, 2, wave(4, 0), None)
    _refused(EINVAL, "n_elec", 4, 9, 1, 0, wave(4, 0), None)
    _refused(EINVAL, "odd", 4, 4, 1, 0, wave(4, 0), None)                  # 4 electrons + 4 spins: two_sz is even
    _refused(EINVAL, "odd", 4, 3, 0, 4, wave(4, 0), None)
    _refused(EUNSUPP, "empty", 4, 4, 10, 1, wave(4, 0), None)              # the source itself has no word


def test_a_missing_target_is_einval():
    L, text = 4, "the target sector does not exist"
    _refused(EINVAL, text, L, 0, 0, kondo.C_UP, wave(L, 0), None)          # nothing to annihilate
    _refused(EINVAL, text, L, 0, 0, kondo.C_DN, wave(L, 0), None)
    _refused(EINVAL, text, L, 2 * L, 0, kondo.CDAG_UP, wave(L, 0), None)   # every orbital full
    _refused(EINVAL, text, L, 2 * L, 0, kondo.CDAG_DN, wave(L, 0), None)
    _refused(EINVAL, text, L, L, 2 * L, kondo.SPIN_PLUS, wave(L, 0), wave(L, 0))       # fully polarised
    _refused(EINVAL, text, L, L, -2 * L, kondo.SPIN_MINUS, None, wave(L, 0))
    _refused(EINVAL, text, L, L, 2 * L, kondo.C_DN, wave(L, 0), None)      # no down electron in the polarised sector
    for op in range(6):                                                    # and the table of targets
        assert kondo.mopr_target(5, 1, op) == [(4, 0), (4, 2), (6, 2), (6, 0), (5, 3), (5, -1)][op]


def test_symmetry_and_coefficient_character():
    L = 6
    sec = (NAMES[1],)
    perms, chars = translations(L)
    p2 = perms.copy()
    p2[0] = p2[1]
    _refused(EINVAL, "identity", L, 6, 0, 0, wave(L, 1), None, p2, chars, names=sec)
    p2 = perms.copy()
    p2[2, 0] = p2[2, 1]
    _refused(EINVAL, "not a site permutation", L, 6, 0, 0, wave(L, 1), None, p2, chars, names=sec)
    p65, c65 = translations(13, 65)
    _refused(EUNSUPP, "65 translations", 13, 13, 0, 0, wave(13, 1), None, p65, c65, names=sec)
    # a coefficient set without a character: one site stronger than the others
    bad = wave(L, 1)
    bad[2] *= 1.5
    _refused(EINVAL, "do not transform with a character", L, 6, 0, kondo.C_UP, bad, None, names=sec)
    _refused(EINVAL, "do not transform with a character", L, 6, 0, kondo.SPIN_MINUS, None, bad, names=sec)
    # two sets with different characters
    _refused(EINVAL, "do not transform with a character", L, 6, 0, kondo.SPIN_PLUS, wave(L, 1), wave(L, 2), names=sec)
    # the full sector asks for no character
    assert _call(NAMES[0], L, 6, 0, kondo.C_UP, bad, None, vec=False) == EINVAL and "a vector is NULL" in _err()
    # the order of the checks: the shape comes before the symmetry, the symmetry before the character
    _refused(EINVAL, "the target sector does not exist", L, 0, 0, kondo.C_UP, bad, None, p2, chars, names=sec)
    _refused(EINVAL, "not a site permutation", L, 6, 0, 0, bad, None, p2, chars, names=sec)


def test_a_sector_of_2_to_the_40_words_is_unsupported():
    assert kondo.sector_dim(16, 16, 0) >= 2 ** 40
    _refused(EUNSUPP, "too large", 16, 16, 0, kondo.C_UP, wave(16, 1), None)
    _refused(EUNSUPP, "too large", 16, 16, 0, kondo.SPIN_MINUS, wave(16, 1), wave(16, 1))
    # the character is checked before the size
    bad = wave(16, 1)
    bad[3] = 0.0
    _refused(EINVAL, "do not transform with a character", 16, 16, 0, kondo.C_UP, bad, None, names=(NAMES[1],))
