"""CPU checks of the d-level (qudit) sector generator: the C ABI declares and exports qbh_gen_qudit / qbh_mopr_qudit_dev, every
argument and term check returns its documented code before the device is looked for, and the pure-numpy term builders of
quantum_basis_amd.qudit match dense operators written out here."""
import ctypes as C
import itertools
import os
import re

import numpy as np
import pytest

from quantum_basis_amd import _lib, qudit

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, ENOTHERM, EUNSUPP = -1, -5, -9


def test_header_declares_and_library_exports_the_qudit_symbols():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "qbhip.h")).read(), flags=re.S)
    for sym in ("qbh_gen_qudit", "qbh_mopr_qudit_dev"):
        assert re.search(r"\b%s\s*\(" % sym, text), sym
        assert sym in _lib.EXPORTS
        assert hasattr(_lib.lib(), sym)


def _gen(n_sites, d, total, pairs=(), singles=(), rows=(0, -1)):
    """Call qbh_gen_qudit on host arrays; returns (rc, dim_out)."""
    ps = np.ascontiguousarray(np.array([(p[0], p[1]) for p in pairs], dtype=np.int32).reshape(-1, 2))
    pm = np.ascontiguousarray(np.array([np.asarray(p[2], dtype=np.complex128) for p in pairs], dtype=np.complex128).reshape(-1))
    ss = np.ascontiguousarray(np.array([s[0] for s in singles], dtype=np.int32))
    sd = np.ascontiguousarray(np.array([s[1] for s in singles], dtype=np.float64).reshape(-1))
    h = C.c_void_p()
    dim = C.c_int64(-1)
    rc = _lib.lib().qbh_gen_qudit(C.byref(h), n_sites, d, total, len(pairs), ps.ctypes.data, pm.ctypes.data, len(singles),
                                  ss.ctypes.data, sd.ctypes.data, rows[0], rows[1], C.byref(dim), None)
    assert rc != 0 or h.value
    if rc == 0:
        _lib.lib().qbh_csr_destroy(h)
    return rc, dim.value


def _err():
    return _lib.lib().qbh_last_error().decode()


def test_charge_violating_pair_is_einval():
    M = np.zeros((9, 9), dtype=np.complex128)
    M[1 * 3 + 1, 0 * 3 + 1] = 1.0            # |0 1> -> |1 1>: charge 1 -> 2
    M[0 * 3 + 1, 1 * 3 + 1] = 1.0
    rc, _ = _gen(4, 3, 4, [(0, 1, M)])
    assert rc == EINVAL and "charge" in _err()


def test_non_hermitian_merged_pair_is_enotherm():
    sz, sp, sm = qudit.spin_matrices(1)
    M = np.kron(sp, sm)                      # S+_i S-_j alone is not Hermitian
    rc, _ = _gen(4, 3, 4, [(0, 1, M)])
    assert rc == ENOTHERM
    # ... but with its conjugate given on the reversed pair it is: (1, 0) is transposed into (0, 1) order first
    rc, _ = _gen(4, 3, 4, [(0, 1, M), (1, 0, M)])
    assert rc in (0, -2)                     # ok on a GPU box, no device here
    # two halves that are Hermitian only after merging
    rc, _ = _gen(4, 3, 4, [(0, 1, np.kron(sp, sm)), (0, 1, np.kron(sm, sp))])
    assert rc in (0, -2)
    # an imaginary diagonal
    D = np.zeros((9, 9), dtype=np.complex128)
    D[4, 4] = 1j
    assert _gen(4, 3, 4, [(0, 1, D)])[0] == ENOTHERM


def test_limits_are_refused_before_the_device_check():
    M = qudit.heisenberg_terms(1, [(0, 1)])[0][2]
    assert _gen(4, 9, 4)[0] == EUNSUPP and "at most 8" in _err()
    assert _gen(4, 1, 0)[0] == EINVAL
    assert _gen(22, 5, 20)[0] == EUNSUPP and "64 bits" in _err()           # 22 sites x 3 bits
    assert _gen(21, 5, 20)[0] in (0, -2, EUNSUPP)                            # 63 bits pack; the dimension may still be too big
    bonds = [(i, (i + 1) % 22) for i in range(22)]
    rc, dim = _gen(22, 3, 22, [(i, j, M) for i, j in bonds])
    assert rc == EUNSUPP and "int32" in _err()
    assert dim == qudit.qudit_dim(22, 3, 22) == 3_241_135_527 > 2 ** 31
    assert _gen(4, 3, 9)[0] == EINVAL                                       # charge above n (d - 1)
    assert _gen(4, 3, -1)[0] == EINVAL
    assert _gen(4, 3, 4, [(0, 4, M)])[0] == EINVAL                          # site out of range
    assert _gen(4, 3, 4, [(2, 2, M)])[0] == EINVAL
    assert _gen(4, 3, 4, singles=[(5, np.zeros(3))])[0] == EINVAL
    rc, dim = _gen(4, 3, 4, [(0, 1, M)], rows=(0, 100))
    assert rc == EINVAL and dim == 19
    # more distinct pairs than the cap, and a worst-case row above the cap
    many = [(i, j, M) for i in range(50) for j in range(i + 1, 50)][:1100]
    assert _gen(50, 2, 25, [(i, j, np.eye(4)) for i, j, _ in many])[0] == EUNSUPP and "1024" in _err()
    Mk = qudit.heisenberg_terms(1, [(0, 1)], K=0.5)[0][2]                   # at most 2 off-diagonal entries per pair and row
    dense = [(i, j, Mk) for i in range(16) for j in range(i + 1, 16)]       # 120 pairs x 2 + 1 > 240
    assert _gen(16, 3, 16, dense)[0] == EUNSUPP and "240" in _err()
    assert _gen(16, 3, 16, dense[:-1])[0] in (0, -2)                        # 239 + 1 fits


def test_mopr_argument_checks_before_the_device():
    L = _lib.lib()
    coef = np.ones(4, dtype=np.complex128)
    sz, sp, sm = qudit.spin_matrices(1)
    dim = C.c_int64(0)
    x = C.c_void_p(16)                       # never dereferenced: every call below fails before the device
    assert L.qbh_mopr_qudit_dev(4, 3, 4, 0, coef.ctypes.data, np.ascontiguousarray(sp).ctypes.data, x, x, C.byref(dim), None) == EINVAL
    assert L.qbh_mopr_qudit_dev(4, 3, 0, -1, coef.ctypes.data, np.ascontiguousarray(sp).ctypes.data, x, x, C.byref(dim), None) == EINVAL
    assert L.qbh_mopr_qudit_dev(4, 9, 4, 0, coef.ctypes.data, np.ascontiguousarray(np.eye(9, dtype=complex)).ctypes.data, x, x,
                                C.byref(dim), None) == EUNSUPP


def test_mopr_local_matrix_must_sit_on_the_dq_diagonal():
    """|dq| >= d: no level can change by dq, so every nonzero entry is off the diagonal and refused, although the target charge
    exists; dq = +-2: an entry one off the dq diagonal is refused and named, the matrix without it passes every check."""
    L = _lib.lib()
    coef = np.ones(4, dtype=np.complex128)
    x = C.c_void_p(16)                       # never dereferenced
    dim = C.c_int64(-1)

    def call(d, total_old, dq, loc):
        loc = np.ascontiguousarray(loc, dtype=np.complex128)
        return L.qbh_mopr_qudit_dev(4, d, total_old, dq, coef.ctypes.data, loc.ctypes.data, x, x, C.byref(dim), None)

    for dq, total in ((3, 4), (-3, 4), (4, 2)):                        # d = 3: charges 0 .. 8, so total + dq is a sector
        loc = np.zeros((3, 3), dtype=np.complex128)
        loc[2, 0] = 1.0
        assert call(3, total, dq, loc) == EINVAL
        msg = L.qbh_last_error().decode()
        assert "qbh_mopr_qudit_dev" in msg and "local[2][0]" in msg and "dq = %d" % dq in msg
    for dq, good, off in ((2, (2, 0), (1, 0)), (-2, (0, 2), (0, 1)), (2, (3, 1), (3, 2)), (-2, (1, 3), (1, 2))):
        loc = np.zeros((4, 4), dtype=np.complex128)
        loc[good] = 0.5 - 1j
        if L.qbh_device_count() <= 0:                                     # with a device the call would run on the fake addresses
            assert call(4, 6, dq, loc) == -2 and dim.value == {2: 31, -2: 31}[dq]
        loc[off] = 1e-300
        assert call(4, 6, dq, loc) == EINVAL
        msg = L.qbh_last_error().decode()
        assert "qbh_mopr_qudit_dev" in msg and "local[%d][%d]" % off in msg and "dq = %d" % dq in msg


@pytest.mark.parametrize("S", [0.5, 1, 1.5, 2])
def test_spin_matrices_algebra(S):
    sz, sp, sm = qudit.spin_matrices(S)
    d = int(round(2 * S)) + 1
    assert sz.shape == (d, d)
    assert np.allclose(sp @ sm - sm @ sp, 2 * sz, atol=1e-13)
    sx, sy = (sp + sm) / 2, (sp - sm) / 2j
    assert np.allclose(sx @ sx + sy @ sy + sz @ sz, S * (S + 1) * np.eye(d), atol=1e-13)
    assert np.allclose(np.diag(sz).real, S - np.arange(d))                 # level 0 is m = +S
    assert np.allclose(sp, sm.conj().T)


def _site_op(op, s, n, d):
    mats = [np.eye(d)] * n
    mats[s] = op
    out = np.ones((1, 1))
    for m in mats:                            # site 0 leftmost in np.kron: index = sum l_s d^(n-1-s)
        out = np.kron(out, m)
    return out


def _assemble(n, d, pairs, singles):
    """Dense operator of pair / single terms, index = sum l_s d^(n-1-s) (site 0 most significant)."""
    H = np.zeros((d ** n, d ** n), dtype=np.complex128)
    for i, j, M in pairs:
        M = np.asarray(M).reshape(d, d, d, d)
        for a2, b2, a1, b1 in itertools.product(range(d), repeat=4):
            if M[a2, b2, a1, b1] != 0:
                ei = np.zeros((d, d)); ei[a2, a1] = 1
                ej = np.zeros((d, d)); ej[b2, b1] = 1
                H += M[a2, b2, a1, b1] * _site_op(ei, i, n, d) @ _site_op(ej, j, n, d)
    for s, dg in singles:
        H += _site_op(np.diag(dg), s, n, d)
    return H


@pytest.mark.parametrize("S", [0.5, 1, 1.5])
def test_heisenberg_terms_against_dense(S):
    n, bonds = 3, [(0, 1), (1, 2), (2, 0)]
    J, Jz, K, D = 0.7, 1.3, 0.4, 0.25
    sz, sp, sm = qudit.spin_matrices(S)
    d = sz.shape[0]
    ops = [[_site_op(o, s, n, d) for s in range(n)] for o in (sz, sp, sm)]
    H = np.zeros((d ** n, d ** n), dtype=np.complex128)
    for i, j in bonds:
        xy = 0.5 * (ops[1][i] @ ops[2][j] + ops[2][i] @ ops[1][j])
        zz = ops[0][i] @ ops[0][j]
        H += J * xy + Jz * zz + K * (xy + zz) @ (xy + zz)
    for s in range(n):
        H += D * ops[0][s] @ ops[0][s]
    got = _assemble(n, d, qudit.heisenberg_terms(S, bonds, J, Jz, K), qudit.single_ion(S, n, D))
    assert np.allclose(got, H, atol=1e-12)
    # every pair matrix conserves the charge and is Hermitian
    for _, _, M in qudit.heisenberg_terms(S, bonds, J, Jz, K):
        assert np.allclose(M, M.conj().T)
        for r, c in zip(*np.nonzero(np.abs(M) > 1e-15)):
            assert r // d + r % d == c // d + c % d


def test_bose_hubbard_terms_against_dense():
    n_max, n, t, U, mu = 2, 3, 0.8, 1.1, 0.3
    d = n_max + 1
    b = np.diag(np.sqrt(np.arange(1, d)), 1)
    bonds = [(0, 1), (1, 2)]
    B = [_site_op(b, s, n, d) for s in range(n)]
    H = np.zeros((d ** n, d ** n), dtype=np.complex128)
    for i, j in bonds:
        H += -t * (B[i].T @ B[j] + B[j].T @ B[i])
    for s in range(n):
        N = B[s].T @ B[s]
        H += 0.5 * U * N @ (N - np.eye(d ** n)) - mu * N
    pairs, singles = qudit.bose_hubbard_terms(n_max, bonds, t, U, mu)
    assert sorted(s for s, _ in singles) == [0, 1, 2]
    assert np.allclose(_assemble(n, d, pairs, singles), H, atol=1e-12)


@pytest.mark.parametrize("n,d", [(1, 2), (5, 2), (4, 3), (5, 4), (3, 8), (6, 5)])
def test_qudit_dim_against_enumeration(n, d):
    hist = np.bincount([sum(w) for w in itertools.product(range(d), repeat=n)], minlength=n * (d - 1) + 1)
    for total in range(n * (d - 1) + 1):
        assert qudit.qudit_dim(n, d, total) == hist[total]
    assert qudit.qudit_dim(n, d, n * (d - 1) + 1) == 0
    assert qudit.qudit_dim(n, d, -1) == 0


def test_spin_charge():
    assert qudit.spin_charge(10, 1, 0) == 10
    assert qudit.spin_charge(4, 0.5, 2) == 1          # 3 up, 1 down: n_dn of qbh_gen_heisenberg
    assert qudit.spin_charge(14, 1.5, 0) == 21
    with pytest.raises(ValueError):
        qudit.spin_charge(3, 0.5, 0)


def test_row_capacity_and_dimension_at_their_edges():
    """d = 2: every pair adds one entry to the longest row.  239 pairs give 240 entries, the capacity; 240 give 241.  The largest
    dimension with int32 columns: C(34, 15) passes, C(34, 16) >= 2^31 - 1 does not."""
    X = np.zeros((4, 4))
    X[1, 2] = X[2, 1] = 0.5
    sites = [(i, j) for i in range(64) for j in range(i + 1, 64)]
    assert _gen(64, 2, 63, [(i, j, X) for i, j in sites[:239]])[0] in (0, -2)
    assert _gen(64, 2, 63, [(i, j, X) for i, j in sites[:240]])[0] == EUNSUPP and "241" in _err()
    rc, dim = _gen(34, 2, 15, [(0, 1, X)], rows=(0, 1))
    assert rc in (0, -2) and dim == 1_855_967_520 < 2 ** 31 - 1
    rc, dim = _gen(34, 2, 16, [(0, 1, X)], rows=(0, 1))
    assert rc == EUNSUPP and dim == 2_203_961_430 and "int32" in _err()
