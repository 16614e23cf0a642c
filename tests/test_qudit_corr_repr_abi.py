"""CPU checks of qbh_corr_qudit_repr_dev (all-pair correlations and string order of a d-level momentum-sector state): the symbol is
exported, declared and bound, and every invalid argument is refused with its code and a message that names it BEFORE the device is
looked for, in the documented order -- so these run without a GPU.  The vector pointers below are never dereferenced: every call
here fails in the argument checks (or, on a host without a device, at the device check)."""
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
WHO = "qbh_corr_qudit_repr_dev"
D3 = np.array([1.0, 0.0, -1.0, 1.0, 0.0, 1.0])             # two diagonal tables of d = 3
T3 = np.array([1.0, 0.5, -1.0])
NAN3 = np.array([1.0, np.nan, -1.0])
INF0 = np.array([np.inf, 1.0, 1.0])                        # lower[0] is ignored
OUTPUTS = ("pop", "dd", "str", "aa")


def _msg():
    return _lib.lib().qbh_last_error().decode()


def _ring(n, k=0):
    perms = np.array([[(s + g) % n for s in range(n)] for g in range(n)], dtype=np.int32)
    chars = np.exp(-2j * np.pi * k * np.arange(n) / n).astype(np.complex128)
    return perms, chars


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def _call(n_sites, d, total, perms, chars, vec, vec_re, n_diag=0, diag=None, he=None, gm=None, low=None, want=OUTPUTS, n_trans=None):
    p = None if perms is None else np.ascontiguousarray(perms, dtype=np.int32)
    c = None if chars is None else np.ascontiguousarray(chars, dtype=np.complex128)
    n2, dim = C.c_double(-7.0), C.c_int64(-7)
    out = np.full(4 * 4 * 64 * 64 * 2, -7.0)                 # room for any output array
    o = {k: (_p(out) if k in want else None) for k in OUTPUTS}
    rc = _lib.lib().qbh_corr_qudit_repr_dev(n_sites, d, total, (len(p) if n_trans is None else n_trans), _p(p), _p(c), vec, vec_re,
                                            n_diag, _p(diag), _p(he), _p(gm), _p(low), C.byref(n2), o["pop"], o["dd"], o["str"],
                                            o["aa"], C.byref(dim), None)
    untouched = n2.value == -7.0 and dim.value == -7 and bool(np.all(out == -7.0))
    return rc, untouched


def test_symbol_is_exported_declared_and_bound():
    L = _lib.lib()
    assert WHO in _lib.EXPORTS and hasattr(L, WHO)
    vp = C.c_void_p
    assert L.qbh_corr_qudit_repr_dev.argtypes == [C.c_int] * 4 + [vp] * 4 + [C.c_int] + [vp] * 9 + [C.POINTER(C.c_int64), vp]
    with open(HEADER) as f:
        text = f.read()
    assert re.search(r"\bint\s+qbh_corr_qudit_repr_dev\s*\(\s*int n_sites, int d, int total, int n_trans, const int32_t \*perms, "
                     r"const double \*chars,\s*const qbh_z \*d_vec, const double \*d_vec_re, int n_diag, const double \*diag", text)
    for name in ("qudit_repr_correlations", "spin_s_repr_correlations", "bose_repr_correlations"):
        assert hasattr(q, name)
    # the sibling headers no longer call the d-level sectors out of scope; the Kondo family still is
    assert "d-level and Kondo sector families" not in text and "other sector families are out of scope" not in text
    assert text.count("Kondo sector family are out of scope") + text.count("Kondo sector family are out of scope".replace(" are", "\n * are")) >= 1


P6, C6 = _ring(6)
_, C6K1 = _ring(6, 1)
NOT_A_PERMUTATION = P6.copy()
NOT_A_PERMUTATION[3, 2] = NOT_A_PERMUTATION[3, 5]            # translation 3 sends two sites to one
OUT_OF_RANGE = P6.copy()
OUT_OF_RANGE[2, 0] = 6
SHIFTED = np.roll(P6, 1, axis=0)                             # translation 0 is not the identity
P32, C32 = _ring(32)
FULL = dict(n_diag=2, diag=D3, he=T3, gm=T3, low=T3)
FULL_2 = dict(n_diag=1, diag=T3[:2], he=T3[:2], gm=T3[:2], low=T3[:2])

# in the documented order of the checks; a case that breaks several rules names the FIRST one
BAD = [
    ("perms NULL", (6, 3, 6, None, C6, X, None), {"n_trans": 6}, EINVAL, "perms and chars"),
    ("chars NULL and n_sites 0", (0, 3, 0, P6, None, X, None), {}, EINVAL, "perms and chars"),
    ("n_sites 0", (0, 3, 0, P6, C6, X, None), {}, EINVAL, "n_sites"),
    ("one level", (6, 1, 0, P6, C6, X, None), {}, EINVAL, "d >= 2"),
    ("nine levels and total negative", (6, 9, -1, P6, C6, X, None), {}, EUNSUPP, "at most 8"),
    ("33 sites of two bits", (33, 3, 4, P6, C6, X, None), {}, EUNSUPP, "64 bits"),
    ("22 sites of three bits and no translations", (22, 8, 4, P6, C6, X, None), {"n_trans": 0}, EUNSUPP, "64 bits"),
    ("total negative", (6, 3, -1, P6, C6, X, None), {}, EINVAL, "total = -1"),
    ("total above n (d - 1) and 65 translations", (6, 3, 13, P6, C6, X, None), {"n_trans": 65}, EINVAL, "total = 13"),
    ("no translations", (6, 3, 6, P6, C6, X, None), {"n_trans": 0}, EINVAL, "n_trans = 0"),
    ("65 translations and both vectors", (6, 3, 6, P6, C6, X, X), {"n_trans": 65}, EINVAL, "n_trans = 65"),
    ("both vectors and n_diag 9", (6, 3, 6, P6, C6, X, X), {"n_diag": 9}, EINVAL, "exactly one"),
    ("neither vector and not a permutation", (6, 3, 6, NOT_A_PERMUTATION, C6, None, None), {}, EINVAL, "exactly one"),
    ("n_diag negative", (6, 3, 6, P6, C6, X, None), {"n_diag": -1, "diag": D3}, EINVAL, "n_diag = -1"),
    ("n_diag 5 and one string table", (6, 3, 6, P6, C6, X, None), {"n_diag": 5, "diag": D3, "he": T3}, EINVAL, "n_diag = 5"),
    ("diag NULL and one string table", (6, 3, 6, P6, C6, X, None), {"n_diag": 2, "he": T3}, EINVAL, "diag is NULL"),
    ("string_end only", (6, 3, 6, P6, C6, X, None), {"he": T3, "want": ("dd",)}, EINVAL, "string_end and string_mid"),
    ("string_mid only", (6, 3, 6, P6, C6, None, X), {"gm": T3}, EINVAL, "string_end and string_mid"),
    ("dd without tables", (6, 3, 6, P6, C6, X, None), {"he": NAN3, "gm": T3, "want": ("dd",)}, EINVAL, "dd is wanted"),
    ("str without tables", (6, 3, 6, P6, C6, X, None), {"n_diag": 2, "diag": D3, "want": ("str", "aa")}, EINVAL, "str is wanted"),
    ("aa without lower", (6, 3, 6, P6, C6, X, None), {"n_diag": 2, "diag": D3, "he": T3, "gm": T3, "want": ("aa",)}, EINVAL, "aa is wanted"),
    ("diag not finite", (6, 3, 6, P6, C6, X, None), {"n_diag": 2, "diag": np.append(D3[:5], np.inf), "want": ()}, EINVAL, "diag[5]"),
    ("string_end not finite", (6, 3, 6, P6, C6, X, None), {"he": NAN3, "gm": NAN3, "want": ()}, EINVAL, "string_end[1]"),
    ("string_mid not finite", (6, 3, 6, P6, C6, X, None), {"he": T3, "gm": NAN3, "low": NAN3, "want": ()}, EINVAL, "string_mid[1]"),
    ("lower not finite and not a permutation", (6, 3, 6, NOT_A_PERMUTATION, C6, X, None), {"low": NAN3, "want": ()}, EINVAL, "lower[1]"),
    ("not a permutation", (6, 3, 6, NOT_A_PERMUTATION, C6, X, None), FULL, EINVAL, "translation 3 is not a site permutation"),
    ("image out of range", (6, 3, 6, OUT_OF_RANGE, C6, X, None), FULL, EINVAL, "translation 2 is not a site permutation"),
    ("translation 0 not the identity", (6, 3, 6, SHIFTED, C6K1, None, X), FULL, EINVAL, "translation 0 must be the identity"),
    ("packed real with a complex character", (6, 3, 6, P6, C6K1, None, X), FULL, EINVAL, "real characters"),
    ("2^40 words", (32, 4, 48, P32, C32, X, None), FULL, EUNSUPP, "too large to enumerate"),
    ("2^40 words, packed real with a complex character", (32, 4, 48, P32, _ring(32, 1)[1], None, X), {"want": ()}, EINVAL, "real characters"),
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
    assert _call(6, 3, 6, perms, chars, None, X, **FULL)[0] == ENODEVICE


def test_valid_arguments_without_a_device_fail_last_and_loudly():
    if _lib.lib().qbh_device_count() > 0:
        return                                               # with a device the call would run: tests/test_gpu_qudit_corr_repr.py
    for args, kw in [((6, 3, 6, P6, C6, X, None), FULL), ((6, 3, 6, P6, C6, None, X), FULL), ((6, 3, 6, P6, C6K1, X, None), FULL),
                     ((6, 3, 6, P6, C6, X, None), {"want": ()}), ((6, 3, 0, P6, C6, X, None), {"low": INF0, "want": ("aa",)}),      # lower[0] is ignored
                     ((32, 4, 2, P32, C32, X, None), {"want": ("pop",)})]:
        rc, untouched = _call(*args, **kw)
        assert rc == ENODEVICE and untouched, _msg()
    # 64 sites with 64 translations: 360 KB of translation tables, no refusal for the size of the tables
    p64, c64 = _ring(64)
    assert _call(64, 2, 2, p64, c64, X, None, **FULL_2)[0] == ENODEVICE
    with pytest.raises(_lib.QbhError):
        q.qudit_repr_correlations(6, 3, 6, P6, C6, X)
    with pytest.raises(_lib.QbhError):
        q.spin_s_repr_correlations(6, 1, 0, P6, C6, X)
    with pytest.raises(_lib.QbhError):
        q.bose_repr_correlations(6, 6, 2, P6, C6, X, real=True)


def test_python_layer_checks_its_arguments():
    with pytest.raises(ValueError):
        q.qudit_repr_correlations(6, 3, 6, P6, C6[:4], X)    # four characters for six translations
    with pytest.raises(ValueError):
        q.qudit_repr_correlations(6, 3, 6, P6, C6, X, diag=([1.0, 2.0],))      # a table of the wrong length
    with pytest.raises(_lib.QbhError) as e:
        q.qudit_repr_correlations(6, 3, 13, P6, C6, X)
    assert "total" in str(e.value)
