"""CPU checks of the d-level momentum-sector generator: the C ABI declares and exports qbh_gen_qudit_repr(_cuts) and
qbh_mopr_qudit_repr_dev, and every argument, term and symmetry check returns its documented code before the device is
looked for (QBH_ENODEVICE = -2 here once all of them pass)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from quantum_basis_amd import _lib, qudit

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, ENODEVICE, ENOTHERM, EUNSUPP = -1, -2, -5, -9
OK_HERE = (0, ENODEVICE)                     # ok on a GPU box, no device here


def test_header_declares_and_library_exports_the_qudit_repr_symbols():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "qbhip.h")).read(), flags=re.S)
    for sym in ("qbh_gen_qudit_repr", "qbh_gen_qudit_repr_cuts", "qbh_mopr_qudit_repr_dev"):
        assert re.search(r"\b%s\s*\(" % sym, text), sym
        assert sym in _lib.EXPORTS
        assert hasattr(_lib.lib(), sym)


def chain(L):
    return [(i, (i + 1) % L) for i in range(L)]


def translations(L):
    perms = np.array([[(s + t) % L for s in range(L)] for t in range(L)], dtype=np.int32)
    chars = np.exp(-2j * np.pi * np.arange(L) / L)
    return perms, chars


def _gen(n_sites, d, total, pairs=(), singles=(), perms=None, chars=None, shard=(0, 1)):
    """Call qbh_gen_qudit_repr on host arrays; returns rc."""
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
    rc = _lib.lib().qbh_gen_qudit_repr(C.byref(h), n_sites, d, total, len(pairs), ps.ctypes.data, pm.ctypes.data, len(singles),
                                       ss.ctypes.data, sd.ctypes.data, len(c), p.ctypes.data, c.ctypes.data, 100.0, shard[0],
                                       shard[1], C.byref(dim), None)
    assert rc != 0 or h.value
    if rc == 0:
        _lib.lib().qbh_csr_destroy(h)
    return rc


_VECS = []


def _vectors():
    """The two vectors of a call.  Where there is a device a call that passes every check runs and reads and writes them, so they
    are real there (the sectors the tests let through have a few dozen representatives); without one nothing ever looks at them."""
    lib = _lib.lib()
    if lib.qbh_device_count() <= 0:
        return C.c_void_p(64), C.c_void_p(64)
    while len(_VECS) < 2:
        v = C.c_void_p()
        assert lib.qbh_vec_alloc(C.byref(v), C.c_int64(1 << 16)) == 0
        _VECS.append(v)
    return _VECS[0], _VECS[1]


@pytest.fixture(scope="module", autouse=True)
def _free_vectors():
    yield
    while _VECS:
        _lib.lib().qbh_vec_free(_VECS.pop())


def _mopr(n_sites, d, total_old, dq, coef, local, perms=None, chars=None):
    if perms is None:
        perms, chars = translations(n_sites)
    p = np.ascontiguousarray(perms, dtype=np.int32)
    ch = np.ascontiguousarray(chars, dtype=np.complex128)
    c = np.ascontiguousarray(coef, dtype=np.complex128)
    o = np.ascontiguousarray(np.asarray(local, dtype=np.complex128).reshape(-1))
    old, new = _vectors()
    return _lib.lib().qbh_mopr_qudit_repr_dev(n_sites, d, total_old, dq, len(ch), p.ctypes.data, ch.ctypes.data, c.ctypes.data,
                                              o.ctypes.data, old, new, None, None, None)


def _err():
    return _lib.lib().qbh_last_error().decode()


def spin1_chain(L):
    return qudit.heisenberg_terms(1, chain(L))


def test_a_valid_call_passes_every_check():
    assert _gen(6, 3, 6, spin1_chain(6)) in OK_HERE
    assert _gen(6, 3, 6, spin1_chain(6), qudit.single_ion(1, 6, 0.3)) in OK_HERE


def test_charge_violating_pair_is_einval():
    M = np.zeros((9, 9), dtype=np.complex128)
    M[1 * 3 + 1, 0 * 3 + 1] = 1.0            # |0 1> -> |1 1>: charge 1 -> 2
    M[0 * 3 + 1, 1 * 3 + 1] = 1.0
    assert _gen(4, 3, 4, [(i, j, M) for i, j in chain(4)]) == EINVAL and "charge" in _err()


def test_non_hermitian_merged_pair_is_enotherm():
    sz, sp, sm = qudit.spin_matrices(1)
    M = np.kron(sp, sm)
    assert _gen(4, 3, 4, [(i, j, M) for i, j in chain(4)]) == ENOTHERM


def test_terms_that_are_not_translation_invariant_are_einval():
    L = 6
    pairs = spin1_chain(L)
    assert _gen(L, 3, L, pairs[:-1]) == EINVAL and "invariant" in _err()               # open chain
    J2 = [(i, j, 1.5 * M if i == 2 else M) for i, j, M in pairs]                       # one bond stronger
    assert _gen(L, 3, L, J2) == EINVAL and "invariant" in _err()
    assert _gen(L, 3, L, pairs, [(0, [0.0, 0.1, 0.0])]) == EINVAL and "single-site" in _err()
    # a pair term that is not symmetric under exchange of its sites: S^z_i on (i, i+1) is invariant only in that orientation
    sz = qudit.spin_matrices(1)[0]
    A = np.kron(sz, np.eye(3))
    assert _gen(L, 3, L, pairs + [(i, j, A) for i, j in chain(L)]) in OK_HERE
    assert _gen(L, 3, L, pairs + [(i, (i + 1) % L, A) for i in range(L - 1)] + [(0, L - 1, A)]) == EINVAL
    # a translation group the terms do not respect: next-nearest-neighbour translations of a chain with alternating bonds
    alt = [(i, j, (1.0 if i % 2 == 0 else 0.5) * M) for i, j, M in pairs]
    perms, chars = translations(L)
    assert _gen(L, 3, L, alt, perms=perms[::2], chars=chars[::2] ** 0) in OK_HERE
    assert _gen(L, 3, L, alt) == EINVAL


def test_bad_permutations_are_einval():
    L = 6
    perms, chars = translations(L)
    bad = perms.copy()
    bad[[0, 1]] = bad[[1, 0]]                # translation 0 is not the identity
    assert _gen(L, 3, L, spin1_chain(L), perms=bad, chars=chars) == EINVAL and "identity" in _err()
    bad = perms.copy()
    bad[2, 1] = bad[2, 0]                    # two sites onto one
    assert _gen(L, 3, L, spin1_chain(L), perms=bad, chars=chars) == EINVAL and "permutation" in _err()
    bad = perms.copy()
    bad[3, 0] = L                            # out of range
    assert _gen(L, 3, L, spin1_chain(L), perms=bad, chars=chars) == EINVAL


def test_limits_are_refused_before_the_device_check():
    assert _gen(4, 9, 4) == EUNSUPP and "at most 8" in _err()
    assert _gen(4, 1, 0) == EINVAL
    assert _gen(22, 5, 20) == EUNSUPP and "64 bits" in _err()                         # 22 sites x 3 bits
    assert _gen(4, 3, 9, spin1_chain(4)) == EINVAL                                     # charge out of range
    L = 70
    assert _gen(L, 2, 35, perms=np.arange(L)[None, :], chars=[1.0]) == EUNSUPP         # more than 64 sites
    L = 8
    many = np.array([[(s + t) % L for s in range(L)] for t in range(65)], dtype=np.int32)
    assert _gen(L, 3, L, spin1_chain(L), perms=many, chars=np.ones(65)) == EINVAL      # more than 64 translations
    assert _gen(L, 3, L, spin1_chain(L), shard=(2, 2)) == EINVAL
    # more entries per row than the row kernels hold: every pair of a 16-site chain (120 pairs, two moves each)
    L = 16
    allpairs = qudit.heisenberg_terms(1, [(i, j) for i in range(L) for j in range(i + 1, L)], K=0.3)
    assert _gen(L, 3, L, allpairs) == EUNSUPP and "row" in _err()
    # a sector of 2^40 words or more cannot be enumerated (32 spin-1 sites, S^z = 0: 1.1e14 words)
    L = 32
    assert _gen(L, 3, L, spin1_chain(L)) == EUNSUPP and "enumerate" in _err()


def test_mopr_argument_checks():
    L = 6
    sz, sp, sm = qudit.spin_matrices(1)
    coef = np.exp(1j * np.pi * np.arange(L) / 3)
    assert _mopr(L, 3, L, 0, coef, sz) in OK_HERE
    assert _mopr(L, 3, L, 1, coef, sm) in OK_HERE
    assert _mopr(L, 3, L, -1, coef, sp) in OK_HERE
    assert _mopr(L, 3, L, 0, np.zeros(L), sz) in OK_HERE
    assert _mopr(L, 3, L, 0, coef, sp) == EINVAL and "dq" in _err()                    # S^+ does not keep the charge
    assert _mopr(L, 3, L, 1, coef, sp) == EINVAL
    eh = coef.copy()
    eh[2] *= 1.01                            # no longer c_{g(s)} = eta(g) c_s
    assert _mopr(L, 3, L, 0, eh, sz) == EINVAL and "character" in _err()
    assert _mopr(L, 3, L, 0, np.arange(L) + 1.0, sz) == EINVAL
    assert _mopr(L, 3, 2 * L, 1, coef, sm) == EINVAL                                   # target charge out of range
    perms, chars = translations(L)
    bad = perms.copy()
    bad[1, 0] = bad[1, 1]
    assert _mopr(L, 3, L, 0, coef, sz, perms=bad, chars=chars) == EINVAL
    assert _mopr(4, 9, 4, 0, np.ones(4), np.eye(9)) == EUNSUPP
