"""CPU checks of the matrix-free d-level momentum sector qbh_mf_qudit_repr: the C ABI declares and exports it, every refusal
that tests/test_qudit_repr_cpu.py exercises for qbh_gen_qudit_repr returns the same code from it before the device is looked
for, a bad row range is refused, and the limit of 160 entries per row of the stored form is not."""
import ctypes as C
import os
import re

import numpy as np

from quantum_basis_amd import _lib, qudit

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, ENODEVICE, ENOTHERM, EUNSUPP = -1, -2, -5, -9
OK_HERE = (0, ENODEVICE)                     # ok on a GPU box, no device here


def test_header_declares_and_library_exports_qbh_mf_qudit_repr():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "qbhip.h")).read(), flags=re.S)
    assert re.search(r"\bqbh_mf_qudit_repr\s*\(", text)
    assert "qbh_mf_qudit_repr" in _lib.EXPORTS
    assert hasattr(_lib.lib(), "qbh_mf_qudit_repr")


def chain(L):
    return [(i, (i + 1) % L) for i in range(L)]


def translations(L):
    perms = np.array([[(s + t) % L for s in range(L)] for t in range(L)], dtype=np.int32)
    chars = np.exp(-2j * np.pi * np.arange(L) / L)
    return perms, chars


def _call(name, n_sites, d, total, pairs=(), singles=(), perms=None, chars=None, rows=(0, -1)):
    """Call qbh_gen_qudit_repr (whole sector) or qbh_mf_qudit_repr (rows) on host arrays; returns (rc, dim_out)."""
    if perms is None:
        perms, chars = translations(n_sites)
    ps = np.ascontiguousarray(np.array([(p[0], p[1]) for p in pairs], dtype=np.int32).reshape(-1, 2))
    pm = np.ascontiguousarray(np.array([np.asarray(p[2], dtype=np.complex128) for p in pairs], dtype=np.complex128).reshape(-1))
    ss = np.ascontiguousarray(np.array([s[0] for s in singles], dtype=np.int32))
    sd = np.ascontiguousarray(np.array([s[1] for s in singles], dtype=np.float64).reshape(-1))
    p = np.ascontiguousarray(perms, dtype=np.int32)
    c = np.ascontiguousarray(chars, dtype=np.complex128)
    h = C.c_void_p()
    dim = C.c_int64(-1)
    head = (C.byref(h), n_sites, d, total, len(pairs), ps.ctypes.data, pm.ctypes.data, len(singles), ss.ctypes.data, sd.ctypes.data,
            len(c), p.ctypes.data, c.ctypes.data, 100.0)
    if name == "qbh_gen_qudit_repr":
        rc = _lib.lib().qbh_gen_qudit_repr(*head, 0, 1, C.byref(dim), None)
    else:
        rc = _lib.lib().qbh_mf_qudit_repr(*head, rows[0], rows[1], C.byref(dim), None)
    assert rc != 0 or h.value
    if rc == 0:
        _lib.lib().qbh_csr_destroy(h)
    return rc, dim.value


def _mf(*a, **k):
    return _call("qbh_mf_qudit_repr", *a, **k)


def _err():
    return _lib.lib().qbh_last_error().decode()


def _same_refusal(code, *a, **k):
    """Both entry points refuse the call with `code` (and leave the same dimension); the last error is qbh_mf_qudit_repr's."""
    want = _call("qbh_gen_qudit_repr", *a, **k)
    assert "qbh_gen_qudit_repr" in _err()
    got = _mf(*a, **k)
    assert got == want and got[0] == code, (got, want, code)
    assert "qbh_mf_qudit_repr" in _err()
    return got


def spin1_chain(L):
    return qudit.heisenberg_terms(1, chain(L))


def all_to_all_spin1(L=12):
    """Every pair of a ring of L spin-1 sites, bilinear + biquadratic with a coupling that depends on the ring distance only:
    translation invariant; a merged spin-1 pair has at most 2 off-diagonal entries in a row of its matrix."""
    dist = lambda i, j: min((j - i) % L, (i - j) % L)
    pairs = []
    for i in range(L):
        for j in range(i + 1, L):
            r = dist(i, j)
            pairs += qudit.heisenberg_terms(1, [(i, j)], J=1.0 / r, K=0.3 / r ** 2)
    return pairs


def test_a_valid_call_passes_every_check():
    assert _mf(6, 3, 6, spin1_chain(6))[0] in OK_HERE
    assert _mf(6, 3, 6, spin1_chain(6), qudit.single_ion(1, 6, 0.3))[0] in OK_HERE


def test_bad_d_and_words_wider_than_64_bits():
    _same_refusal(EUNSUPP, 4, 9, 4)
    assert "at most 8" in _err()
    _same_refusal(EINVAL, 4, 1, 0)
    _same_refusal(EUNSUPP, 22, 5, 20)                                          # 22 sites x 3 bits
    assert "64 bits" in _err()
    _same_refusal(EINVAL, 4, 3, 9, spin1_chain(4))                             # charge out of range
    L = 70
    _same_refusal(EUNSUPP, L, 2, 35, perms=np.arange(L)[None, :], chars=[1.0])  # more than 64 sites
    dim = C.c_int64(0)
    assert _lib.lib().qbh_mf_qudit_repr(None, 4, 3, 4, 0, None, None, 0, None, None, 1, None, None, 100.0, 0, -1, C.byref(dim),
                                        None) == EINVAL


def test_charge_violating_pair_is_einval():
    M = np.zeros((9, 9), dtype=np.complex128)
    M[1 * 3 + 1, 0 * 3 + 1] = 1.0            # |0 1> -> |1 1>: charge 1 -> 2
    M[0 * 3 + 1, 1 * 3 + 1] = 1.0
    _same_refusal(EINVAL, 4, 3, 4, [(i, j, M) for i, j in chain(4)])
    assert "charge" in _err()


def test_non_hermitian_merged_pair_is_enotherm():
    sz, sp, sm = qudit.spin_matrices(1)
    _same_refusal(ENOTHERM, 4, 3, 4, [(i, j, np.kron(sp, sm)) for i, j in chain(4)])


def test_bad_sites_and_too_many_pairs():
    M = qudit.heisenberg_terms(1, [(0, 1)])[0][2]
    _same_refusal(EINVAL, 4, 3, 4, [(0, 4, M)])                                # site out of range
    _same_refusal(EINVAL, 4, 3, 4, [(2, 2, M)])
    _same_refusal(EINVAL, 4, 3, 4, [(-1, 2, M)])
    _same_refusal(EINVAL, 4, 3, 4, singles=[(5, np.zeros(3))])
    many = [(i, j) for i in range(50) for j in range(i + 1, 50)][:1100]
    _same_refusal(EUNSUPP, 50, 2, 25, [(i, j, np.eye(4)) for i, j in many], perms=np.arange(50)[None, :], chars=[1.0])
    assert "1024" in _err()


def test_terms_that_are_not_translation_invariant_are_einval():
    L = 6
    pairs = spin1_chain(L)
    _same_refusal(EINVAL, L, 3, L, pairs[:-1])                                          # open chain
    assert "invariant" in _err()
    J2 = [(i, j, 1.5 * M if i == 2 else M) for i, j, M in pairs]                       # one bond stronger
    _same_refusal(EINVAL, L, 3, L, J2)
    assert "invariant" in _err()
    _same_refusal(EINVAL, L, 3, L, pairs, [(0, [0.0, 0.1, 0.0])])
    assert "single-site" in _err()
    # a translation group the terms do not respect: every translation of a chain with alternating bonds
    alt = [(i, j, (1.0 if i % 2 == 0 else 0.5) * M) for i, j, M in pairs]
    perms, chars = translations(L)
    assert _mf(L, 3, L, alt, perms=perms[::2], chars=chars[::2] ** 0)[0] in OK_HERE
    _same_refusal(EINVAL, L, 3, L, alt)


def test_bad_permutations_and_too_many_translations():
    L = 6
    perms, chars = translations(L)
    bad = perms.copy()
    bad[[0, 1]] = bad[[1, 0]]                # translation 0 is not the identity
    _same_refusal(EINVAL, L, 3, L, spin1_chain(L), perms=bad, chars=chars)
    assert "identity" in _err()
    bad = perms.copy()
    bad[2, 1] = bad[2, 0]                    # two sites onto one
    _same_refusal(EINVAL, L, 3, L, spin1_chain(L), perms=bad, chars=chars)
    assert "permutation" in _err()
    bad = perms.copy()
    bad[3, 0] = L                            # out of range
    _same_refusal(EINVAL, L, 3, L, spin1_chain(L), perms=bad, chars=chars)
    L = 8
    many = np.array([[(s + t) % L for s in range(L)] for t in range(65)], dtype=np.int32)
    _same_refusal(EINVAL, L, 3, L, spin1_chain(L), perms=many, chars=np.ones(65))      # more than 64 translations
    # a sector of 2^40 words or more cannot be enumerated (32 spin-1 sites, S^z = 0: 1.1e14 words)
    _same_refusal(EUNSUPP, 32, 3, 32, spin1_chain(32))
    assert "enumerate" in _err()


def test_bad_row_range_is_einval():
    """The spin-1 ring of 6 sites at S^z = 0 has 141 words: these ranges lie in no sector of it."""
    L = 6
    for rows in ((-1, 5), (5, 5), (7, 3), (0, -2), (141, -1), (0, 142), (0, 100000)):
        rc, _ = _mf(L, 3, L, spin1_chain(L), rows=rows)
        assert rc == EINVAL and "row range" in _err() and "qbh_mf_qudit_repr" in _err(), rows
    assert _mf(L, 3, L, spin1_chain(L), rows=(0, 5))[0] in OK_HERE
    assert _mf(L, 3, L, spin1_chain(L), rows=(3, -1))[0] in OK_HERE


def test_the_row_limit_of_the_stored_form_is_not_refused():
    """All-to-all spin-1 with a biquadratic term.  A merged spin-1 pair has at most 2 off-diagonal entries in a row (the
    charge-2 block |02>, |11>, |20>), so the 66 pairs of 12 sites count 133 entries and the stored form still takes them; the 91
    pairs of 14 sites count 183 > 160: the stored call refuses them, the matrix-free call passes every check with both."""
    pairs = all_to_all_spin1(12)
    assert _call("qbh_gen_qudit_repr", 12, 3, 12, pairs)[0] in OK_HERE
    assert _mf(12, 3, 12, pairs)[0] in OK_HERE
    pairs = all_to_all_spin1(14)
    assert _call("qbh_gen_qudit_repr", 14, 3, 14, pairs)[0] == EUNSUPP and "row" in _err()
    assert _mf(14, 3, 14, pairs)[0] in OK_HERE
    assert _mf(14, 3, 3, pairs, rows=(5, 60))[0] in OK_HERE


def test_a_valid_call_without_a_device_fails_loudly():
    if _lib.lib().qbh_device_count() > 0:
        return                               # a GPU is present: tests/test_gpu_qudit_repr_mf.py covers the call
    got = _mf(6, 3, 6, spin1_chain(6), qudit.single_ion(1, 6, 0.3))
    assert got == _call("qbh_gen_qudit_repr", 6, 3, 6, spin1_chain(6), qudit.single_ion(1, 6, 0.3)) and got[0] == ENODEVICE
    assert _mf(6, 3, 6, spin1_chain(6))[0] == ENODEVICE and "no HIP device" in _err()
