"""CPU checks of qbh_corr_kondo_repr_dev (all-pair correlations of a Kondo-lattice momentum-sector state): the symbol is exported,
declared and bound, and every invalid argument is refused with its code and a message that names it BEFORE the device is looked
for, in the documented order -- so these run without a GPU.  Every case that breaks a rule is combined with a LATER fault as well,
which shows that the earlier check fires first.  The vector pointers below are never dereferenced: every call here fails in the
argument checks (or, on a host without a device, at the device check)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import quantum_basis_amd as q
from quantum_basis_amd import _lib

EINVAL, ENODEVICE, EUNSUPP = -1, -2, -9
X = C.c_void_p(0x1000)           # stands for a device vector
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "qbhip.h")
WHO = "qbh_corr_kondo_repr_dev"
OUTPUTS = ("site", "nn", "zn", "zz", "hop", "ee", "ll", "le")


def _msg():
    return _lib.lib().qbh_last_error().decode()


def _ring(n, k=0):
    perms = np.array([[(s + g) % n for s in range(n)] for g in range(n)], dtype=np.int32)
    chars = np.exp(-2j * np.pi * k * np.arange(n) / n).astype(np.complex128)
    return perms, chars


def _call(n_sites, n_elec, two_sz, perms, chars, vec, vec_re, n_trans=None, norm2=True):
    p = None if perms is None else np.ascontiguousarray(perms, dtype=np.int32)
    c = None if chars is None else np.ascontiguousarray(chars, dtype=np.complex128)
    N = max(n_sites, 1)
    n2, dim = C.c_double(-7.0), C.c_int64(-7)
    z = -7.0 - 7.0j
    out = {"site": np.full((4, N), -7.0), "nn": np.full((4, N, N), -7.0), "zn": np.full((2, N, N), -7.0), "zz": np.full((N, N), -7.0),
           "hop": np.full((2, N, N), z), "ee": np.full((N, N), z), "ll": np.full((N, N), z), "le": np.full((N, N), z)}
    ptr = [out[k].ctypes.data_as(C.c_void_p) for k in OUTPUTS]
    rc = _lib.lib().qbh_corr_kondo_repr_dev(n_sites, n_elec, two_sz, (len(p) if n_trans is None else n_trans),
                                            None if p is None else p.ctypes.data_as(C.c_void_p),
                                            None if c is None else c.ctypes.data_as(C.c_void_p), vec, vec_re,
                                            C.byref(n2) if norm2 else None, *ptr, C.byref(dim), None)
    untouched = n2.value == -7.0 and dim.value == -7 and all(np.all(v.view(np.float64) == -7.0) for v in out.values())
    return rc, untouched


def test_symbol_is_exported_declared_and_bound():
    L = _lib.lib()
    assert WHO in _lib.EXPORTS and hasattr(L, WHO)
    vp = C.c_void_p
    assert L.qbh_corr_kondo_repr_dev.argtypes == [C.c_int] * 4 + [vp] * 13 + [C.POINTER(C.c_int64), vp]
    with open(HEADER) as f:
        text = f.read()
    assert re.search(r"\bint\s+qbh_corr_kondo_repr_dev\s*\(\s*int n_sites, int n_elec, int two_sz, int n_trans, const int32_t \*perms, "
                     r"const double \*chars,\s*const qbh_z \*d_vec, const double \*d_vec_re, double \*norm2,", text)
    assert hasattr(q, "kondo_repr_correlations")
    # the call is described, and no other correlation call still sends its reader away from the momentum sectors of this family
    assert "momentum-sector states are out of scope" not in text
    assert "communicators and the Kondo sector family are out of scope" not in re.sub(r"\s*\n \* ", " ", text)


def test_version_is_unchanged():
    assert _lib.lib().qbh_version() == 601


P6, C6 = _ring(6)
_, C6K1 = _ring(6, 1)
NOT_A_PERMUTATION = P6.copy()
NOT_A_PERMUTATION[3, 2] = NOT_A_PERMUTATION[3, 5]            # translation 3 sends two sites to one
OUT_OF_RANGE = P6.copy()
OUT_OF_RANGE[2, 0] = 6
SHIFTED = np.roll(P6, 1, axis=0)                             # translation 0 is not the identity
P21, C21 = _ring(21)

# in the documented order of the checks; a case that breaks several rules names the FIRST one.  (n, n_elec, two_sz) = (6, 6, 0) is a
# valid shape, (6, 6, 1) has the wrong parity, (6, 0, 14) and (6, 12, 8) have the right parity and no block.
BAD = [
    ("perms NULL", (6, 6, 0, None, C6, X, None), {"n_trans": 6}, EINVAL, "perms and chars"),
    ("chars NULL and n_sites 0", (0, 6, 0, P6, None, X, None), {}, EINVAL, "perms and chars"),
    ("n_sites 0", (0, 0, 0, P6, C6, X, None), {}, EINVAL, "n_sites = 0"),
    ("n_sites 22 and no translations", (22, 4, 0, P6, C6, X, None), {"n_trans": 0}, EINVAL, "n_sites = 22"),
    ("n_elec negative and both vectors", (6, -1, 1, P6, C6, X, X), {}, EINVAL, "n_elec = -1"),
    ("n_elec above 2 n_sites", (6, 13, 1, P6, C6, X, None), {}, EINVAL, "n_elec = 13"),
    ("wrong parity and 65 translations", (6, 6, 1, P6, C6, X, None), {"n_trans": 65}, EINVAL, "is odd"),
    ("empty sector and no translations", (6, 0, 14, P6, C6, X, None), {"n_trans": 0}, EUNSUPP, "is empty"),
    ("empty sector and norm2 NULL", (6, 12, 8, P6, C6, X, None), {"norm2": False}, EUNSUPP, "is empty"),
    ("no translations and both vectors", (6, 6, 0, P6, C6, X, X), {"n_trans": 0}, EINVAL, "n_trans = 0"),
    ("65 translations and neither vector", (6, 6, 0, P6, C6, None, None), {"n_trans": 65}, EINVAL, "n_trans = 65"),
    ("both vectors and norm2 NULL", (6, 6, 0, P6, C6, X, X), {"norm2": False}, EINVAL, "exactly one"),
    ("neither vector and not a permutation", (6, 6, 0, NOT_A_PERMUTATION, C6, None, None), {}, EINVAL, "exactly one"),
    ("norm2 NULL and not a permutation", (6, 6, 0, NOT_A_PERMUTATION, C6, X, None), {"norm2": False}, EINVAL, "norm2 is NULL"),
    ("norm2 NULL and a shifted group", (6, 6, 0, SHIFTED, C6, None, X), {"norm2": False}, EINVAL, "norm2 is NULL"),
    ("translation 0 not the identity and a complex character", (6, 6, 0, SHIFTED, C6K1, None, X), {}, EINVAL,
     "translation 0 must be the identity"),
    ("not a permutation and a complex character", (6, 6, 0, NOT_A_PERMUTATION, C6K1, None, X), {}, EINVAL,
     "translation 3 is not a site permutation"),
    ("image out of range", (6, 6, 0, OUT_OF_RANGE, C6, X, None), {}, EINVAL, "translation 2 is not a site permutation"),
    ("packed real with a complex character", (6, 6, 0, P6, C6K1, None, X), {}, EINVAL, "real characters"),
    ("packed real with a complex character and 2^40 words", (21, 21, 0, P21, _ring(21, 1)[1], None, X), {}, EINVAL, "real characters"),
    ("2^40 words", (21, 21, 0, P21, C21, X, None), {}, EUNSUPP, "too large to enumerate"),
]


@pytest.mark.parametrize("label,args,kw,code,text", BAD, ids=[b[0].replace(" ", "_") for b in BAD])
def test_arguments_are_checked_before_the_device_in_the_documented_order(label, args, kw, code, text):
    rc, untouched = _call(*args, **kw)
    assert rc == code, (label, _msg())
    assert WHO in _msg() and text in _msg(), _msg()
    assert untouched                                         # nothing was written


def test_rounding_of_a_real_character_is_not_a_complex_character():
    if _lib.lib().qbh_device_count() > 0:
        return
    perms, chars = _ring(6, 3)                               # exp(-i pi g): imaginary parts of 1e-16, the rounding of sin(pi g)
    assert np.any(chars.imag != 0.0) and np.max(np.abs(chars.imag)) < 1e-14
    assert _call(6, 6, 0, perms, chars, None, X)[0] == ENODEVICE


def test_valid_arguments_without_a_device_fail_last_and_loudly():
    if _lib.lib().qbh_device_count() > 0:
        return                                               # with a device the call would run: tests/test_gpu_kondo_corr_repr.py
    for args in [(6, 6, 0, P6, C6, X, None), (6, 6, 0, P6, C6, None, X), (6, 4, 2, P6, C6K1, X, None), (6, 0, 0, P6, C6, X, None),
                 (6, 12, 0, P6, C6, X, None), (6, 6, 12, P6, C6, X, None), (21, 1, -18, P21, C21, X, None)]:
        rc, untouched = _call(*args)
        assert rc == ENODEVICE and untouched, _msg()
    # 42 group elements x 4 chunks of tables with the counting tables: the largest footprint of the tests, no refusal for its size
    rot = [[(s + t) % 21 for s in range(21)] for t in range(21)]
    ref = [[(t - s) % 21 for s in range(21)] for t in range(21)]
    assert _call(21, 1, -18, np.array(rot + ref, dtype=np.int32), np.ones(42, dtype=np.complex128), X, None)[0] == ENODEVICE
    with pytest.raises(_lib.QbhError):
        q.kondo_repr_correlations(6, 6, 0, P6, C6, X)


def test_python_layer_checks_its_arguments():
    with pytest.raises(ValueError):
        q.kondo_repr_correlations(6, 6, 0, P6, C6[:4], X)    # four characters for six translations
    with pytest.raises(ValueError):
        q.kondo_repr_correlations(6, 6, 0, P6, C6, X, want=("dens", "flip"))
