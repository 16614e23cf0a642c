"""qbh_mf_kondo on the device: the Kondo-lattice operator applied without a stored matrix, against the stored operator of
qbh_gen_kondo (plain options) and against the numpy assembly of tests/test_gpu_kondo.py written from the operator's
definition.  Every case of that file, the reference's energies, 63-bit words, a row longer than the stored form allows, a
dimension above one resident grid, ragged row shards bit for bit, rows above 2^33, the packed-real drivers and the decoupled
limit against qbh_mf_hubbard."""
import ctypes as C
from math import comb

import numpy as np
import pytest

import quantum_basis_amd as q
from quantum_basis_amd import _lib, kondo
from test_gpu_kondo import CASES, GOLDEN, reference_H

pytestmark = pytest.mark.gpu

PLAIN = dict(kron_split=0, sector_cut=-1, value_dict=0, real_fast_path=0)
EPILOGUES = [(1.0, 0.0, 0.0), (1.0, 1.0, 0.0), (0.6, -1.2, 0.0), (1.0, 0.0, -3.0)]


def chain(L):
    return [(i, (i + 1) % L) for i in range(L)]


def _rand(n, seed, real=False):
    rng = np.random.default_rng(seed)
    return (rng.normal(size=n) + (0.0 if real else 1j) * rng.normal(size=n)).astype(np.complex128)


def _both(n, n_elec, two_sz, T, U=0.0, rows=None):
    A = q.csr_mat.kondo(n, n_elec, two_sz, None, U=U, terms=T, rows=rows, opts=q.make_opts(**PLAIN))
    M = q.csr_mat.kondo(n, n_elec, two_sz, None, U=U, terms=T, rows=rows, matrix_free=True)
    return A, M


def _assert_same_handle_shape(A, M):
    assert M.dim == A.dim and M.ncols == A.ncols and M.row_offset == A.row_offset and M.nnz == A.nnz
    assert M.info().kernel == _lib.KERNEL_MATRIX_FREE
    assert 0 < M.info().bytes_matrix < 4 << 20


def _assert_spmv_matches(A, M, seed, want=None):
    """y = alpha H x + beta y + gamma x with both reductions, matrix-free against stored (A may be None) and against
    `want` = H x of an independent assembly for the same seed, if given: vectors to 1e-13 of |y|_inf, reductions to 1e-12
    relative, x 8 against the numpy sum, which rounds on its own."""
    n = M.dim
    x, y0 = _rand(n, seed), _rand(n, seed + 1)
    hx = want(x) if want is not None else None
    va, vm = (A.vec(2) if A is not None else None), M.vec(2)
    for alpha, beta, gamma in EPILOGUES:
        for v in (va, vm):
            if v is not None:
                v.upload(x, 0)
                v.upload(y0, n)
        dm, nm = M.spmv(vm.at(0), vm.at(n), alpha, beta, gamma, want_red=True)
        ym = vm.download(n, n)
        if A is not None:
            da, na = A.spmv(va.at(0), va.at(n), alpha, beta, gamma, want_red=True)
            ya = va.download(n, n)
            scale = max(np.abs(ya).max(), 1e-300)
            print("epilogue %s: max |delta| / |y|_inf = %.3e" % ((alpha, beta, gamma), np.abs(ym - ya).max() / scale))
            assert np.abs(ym - ya).max() <= 1e-13 * scale, (alpha, beta, gamma, np.abs(ym - ya).max() / scale)
            assert abs(da - dm) <= 1e-12 * max(abs(da), 1.0) and abs(na - nm) <= 1e-12 * max(na, 1e-300)
        if hx is not None:
            yw = alpha * hx + beta * y0 + gamma * x
            print("epilogue %s: against numpy %.3e" % ((alpha, beta, gamma), np.abs(ym - yw).max() / max(np.abs(yw).max(), 1e-300)))
            assert np.abs(ym - yw).max() <= 1e-13 * max(np.abs(yw).max(), 1e-300) * 8
            dw, nw = np.vdot(x, yw), np.vdot(yw, yw).real
            assert abs(dw - dm) <= 1e-12 * max(abs(dw), 1.0) * 8 and abs(nw - nm) <= 1e-12 * max(nw, 1e-300) * 8
    if va is not None:
        va.free()
    vm.free()


# ---- 1. every case of tests/test_gpu_kondo.py ----

@pytest.mark.parametrize("name", sorted(CASES))
def test_every_case_against_stored_and_numpy(name):
    n, n_elec, two_sz, T, U = CASES[name]
    A, M = _both(n, n_elec, two_sz, T, U)
    assert M.dim == kondo.sector_dim(n, n_elec, two_sz)
    _assert_same_handle_shape(A, M)
    H = reference_H(n, n_elec, two_sz, T, U)
    _assert_spmv_matches(A, M, 40, want=lambda x: H @ x)
    if name == "flux":
        q.locate_E0_lanczos(M, nev=1, ncv=0, maxit=12)
        assert M.stats().n_spmv > 0 and M.stats().n_spmv_real == 0           # complex hops: never the real path


def test_the_cases_cover_what_they_should():
    assert len(CASES) == 10
    dims = sorted(kondo.sector_dim(*CASES[k][:3]) for k in CASES)
    assert dims[0] == 3 and dims[-1] == 15184
    assert any(np.iscomplexobj(np.array([h[2] for h in CASES[k][3].hops])) for k in CASES)


# ---- 2. the reference's model ----

def test_reference_model():
    ref = GOLDEN["chain_L4_all_sz"]
    L = ref["L"]
    mk = lambda **kw: q.csr_mat.kondo(L, ref["n_elec"], 0, chain(L), t=ref["t"], J_K=ref["J_K"], **kw)
    A, M = mk(opts=q.make_opts(**PLAIN)), mk(matrix_free=True)
    _assert_same_handle_shape(A, M)
    assert M.dim == 346
    _assert_spmv_matches(A, M, 61)
    x = _rand(A.dim, 7)
    ya, ym = np.empty_like(x), np.empty_like(x)
    A.MultMv(x, ya)
    M.MultMv(x, ym)                                                             # the host seam
    assert np.abs(ym - ya).max() <= 1e-13 * np.abs(ya).max()
    M.MultMv2(x, ym)
    assert np.abs(ym - 2 * ya).max() <= 2e-13 * np.abs(ya).max()
    ra, rm = q.locate_E0_lanczos(A, nev=2, ncv=1), q.locate_E0_lanczos(M, nev=2, ncv=1)
    print("E0 %.10f E1 %.10f in %d steps (stored: %d)" % (rm.E0, rm.E1, rm.steps["E0"], ra.steps["E0"]))
    assert abs(rm.E0 - ref["E0"]) < 1e-8 and abs(rm.E1 - ref["E1"]) < 1e-8
    assert abs(ra.steps["E0"] - rm.steps["E0"]) <= 1
    hv = np.empty(A.dim, dtype=np.complex128)
    A.MultMv(rm.eigenvecs, hv)
    assert np.linalg.norm(hv - rm.E0 * rm.eigenvecs) < 1e-8
    assert M.stats().n_spmv_real > 0
    nconv, w, _ = q.iram(A.dim, M, None, 1, 16, 300, "sr")
    assert abs(w[0] - ra.E0) < 1e-9
    with pytest.raises(_lib.QbhError):
        M.download()


# ---- 3. 63-bit words ----

@pytest.mark.parametrize("n_elec,two_sz", [(2, -19), (40, 19)])
def test_wide_words(n_elec, two_sz):
    """n = 21: the s field sits in bits 42 .. 62.  A 32-bit shift or mask anywhere loses the upper field."""
    n = 21
    T = kondo.Terms(kondo.hop_terms(chain(n), 1.0), [1.1] * n, [0.9] * n, [(0, 20, 0.4, 0.7), (3, 17, 0.2, -0.3), (20, 19, 0.5, 0.5),
                                                                           (7, 8, 0.1, 0.6)])
    A, M = _both(n, n_elec, two_sz, T, U=1.3)
    assert M.dim == 53571
    _assert_same_handle_shape(A, M)
    _assert_spmv_matches(A, M, 9)
    ra, rm = q.locate_E0_lanczos(A, nev=1, ncv=0), q.locate_E0_lanczos(M, nev=1, ncv=0)
    assert abs(ra.E0 - rm.E0) <= 1e-10 * abs(ra.E0)
    assert M.stats().n_spmv_real > 0


# ---- 4. a row longer than the stored form allows ----

_PC16 = np.array([bin(i).count("1") for i in range(1 << 16)], dtype=np.int64)


def _popcount(a):
    """of fields below 2^32"""
    return _PC16[a & 0xffff] + _PC16[a >> 16]


class NumpyKondo:
    """H x and the entry count from the operator's definition, one term at a time over the whole enumerated sector (no
    matrix is held: 170 entries x 524,238 rows would not be quick).  The string of a state is all up operators, then all
    down, sites ascending; an operator on (site, spin) passes those on lower sites of its species, a down one every up
    operator too.  Independent of kd_row_terms: operators act on the column state and the target is looked up by word."""

    def __init__(self, n, n_elec, two_sz, T, U):
        self.n, self.T, self.U = n, T, U
        self.w = kondo.words(n, n_elec, two_sz)
        u, d, s = kondo.fields(self.w, n)
        self.u, self.d, self.s = u.astype(np.int64), d.astype(np.int64), s.astype(np.int64)
        self.pu = _popcount(self.u)
        # occ[spin][site]: the states with that orbital occupied (every move starts from one of these)
        self.occ = [[np.flatnonzero((f >> i) & 1) for i in range(n)] for f in (self.u, self.d)]

    def _index(self, u, d, s):
        w = (u | (d << self.n) | (s << (2 * self.n))).astype(np.uint64)
        k = np.searchsorted(self.w, w)
        assert np.array_equal(self.w[k], w)
        return k

    def _left(self, u, d, pu, site, spin):
        low = (1 << site) - 1
        return _popcount(u & low) if spin == 0 else pu + _popcount(d & low)

    def _move(self, i, j, spin):
        """c+_{i,spin} c_{j,spin}: (states it does not annihilate, sign, u', d')"""
        sel = self.occ[spin][j]
        if i != j:
            sel = sel[(((self.d if spin else self.u)[sel] >> i) & 1) == 0]
        u, d, pu = self.u[sel], self.d[sel], self.pu[sel]
        par = self._left(u, d, pu, j, spin)
        if spin == 0:
            u = u ^ (1 << j)
            pu = pu - 1
        else:
            d = d ^ (1 << j)
        par = par + self._left(u, d, pu, i, spin)
        if spin == 0:
            u = u | (1 << i)
        else:
            d = d | (1 << i)
        return sel, 1 - 2 * (par & 1), u, d

    def apply(self, x):
        """(H x, stored entries: the diagonal of every row + the off-diagonal entries with a nonzero merged amplitude)"""
        n, T = self.n, self.T
        allst = np.arange(self.w.size)
        diag = self.U * _popcount(self.u & self.d).astype(np.float64)
        for i in range(n):
            Sz = 0.5 - ((self.s >> i) & 1)
            sz = 0.5 * (((self.u >> i) & 1) - ((self.d >> i) & 1))
            diag = diag + T.kz[i] * Sz * sz
        for (i, j, bz, bxy) in T.sbonds:
            same = ((self.s >> i) & 1) == ((self.s >> j) & 1)
            diag = diag + bz * np.where(same, 0.25, -0.25)
        y = diag * x
        # off-diagonal amplitudes merged by (kind, sites) as the generator merges them, then y[target] += amp * x[source]
        hop, exch = {}, {}
        for (i, j, au, ad) in T.hops:
            a = hop.setdefault((i, j), [0.0, 0.0])
            a[0] += au
            a[1] += ad
        for (i, j, bz, bxy) in T.sbonds:
            exch[(min(i, j), max(i, j))] = exch.get((min(i, j), max(i, j)), 0.0) + bxy
        entries = self.w.size
        for (i, j), amps in sorted(hop.items()):
            for spin in (0, 1):
                if amps[spin] == 0:
                    continue
                sel, sign, u2, d2 = self._move(i, j, spin)
                if i == j:
                    y[sel] += amps[spin] * x[sel]
                    continue
                y[self._index(u2, d2, self.s[sel])] += amps[spin] * sign * x[sel]
                entries += sel.size
        for i in range(n):
            if T.kxy[i] == 0:
                continue
            # local spin down (bit set): S^+_i s^-_i with s^- = c+_dn c_up; local spin up: S^-_i s^+_i with s^+ = c+_up c_dn
            for sbit, (cr, de) in ((1, (1, 0)), (0, (0, 1))):
                sel = self.occ[de][i]
                sel = sel[((((self.u if cr == 0 else self.d)[sel] >> i) & 1) == 0) & (((self.s[sel] >> i) & 1) == sbit)]
                u, d, pu = self.u[sel], self.d[sel], self.pu[sel]
                par = self._left(u, d, pu, i, de)
                if de == 0:
                    u, pu = u ^ (1 << i), pu - 1
                else:
                    d = d ^ (1 << i)
                par = par + self._left(u, d, pu, i, cr)
                if cr == 0:
                    u = u | (1 << i)
                else:
                    d = d | (1 << i)
                y[self._index(u, d, self.s[sel] ^ (1 << i))] += 0.5 * T.kxy[i] * (1 - 2 * (par & 1)) * x[sel]
                entries += sel.size
        for (i, j), bxy in sorted(exch.items()):
            if bxy == 0:
                continue
            sel = allst[((self.s >> i) & 1) != ((self.s >> j) & 1)]
            y[self._index(self.u[sel], self.d[sel], self.s[sel] ^ (1 << i) ^ (1 << j))] += 0.5 * bxy * x[sel]
            entries += sel.size
        return y, entries


@pytest.mark.parametrize("name", ["flux", "rkky", "odd_filling_sz_minus"])
def test_the_term_by_term_numpy_apply_is_the_definition(name):
    """NumpyKondo against reference_H (which applies the operators one state at a time), so that it can stand in for it where
    that loop would take minutes."""
    n, n_elec, two_sz, T, U = CASES[name]
    H = reference_H(n, n_elec, two_sz, T, U)
    x = _rand(H.shape[0], 3)
    y, entries = NumpyKondo(n, n_elec, two_sz, T, U).apply(x)
    want = H @ x
    assert np.abs(y - want).max() <= 1e-13 * np.abs(want).max()
    off = H.copy()
    off.setdiag(0)
    off.eliminate_zeros()
    assert entries == off.nnz + H.shape[0]


def test_a_row_longer_than_the_stored_form_allows():
    """(13, 2, 1) with all-to-all hops: 2 * 78 + 13 + 1 = 170 entries in the worst row, above the 160 of qbh_gen_kondo."""
    n, n_elec, two_sz = 13, 2, 1
    bonds = [(i, j) for i in range(n) for j in range(i + 1, n)]
    T = kondo.terms(n, bonds, 1.0, 1.1)
    with pytest.raises(_lib.QbhError):
        q.csr_mat.kondo(n, n_elec, two_sz, None, terms=T, opts=q.make_opts(**PLAIN))
    M = q.csr_mat.kondo(n, n_elec, two_sz, None, terms=T, matrix_free=True)
    assert M.dim == kondo.sector_dim(n, n_elec, two_sz) == 524238
    assert M.info().kernel == _lib.KERNEL_MATRIX_FREE
    ref = NumpyKondo(n, n_elec, two_sz, T, 0.0)
    seen = {}

    def want(x):
        y, seen["entries"] = ref.apply(x)
        return y

    _assert_spmv_matches(None, M, 13, want=want)
    assert M.nnz == seen["entries"]


# ---- 5. grid-stride loop and tail ----

def test_grid_stride_loop_and_tail():
    """Chain L = 8 at half filling, dim 739,162 = 2887 x 256 + 90.  The resident grid of k_mf_kondo is at most 7 workgroups of
    256 lanes on each of 256 CUs = 458,752 lanes (and no device holds more than 2048 lanes per CU = 524,288), so L = 8 already
    sends lanes round the loop a second time and leaves a ragged last workgroup; L = 9 is not needed.
    The full sector's E0 is the lowest over all momenta, so it cannot lie above any E0_by_k the reference asserts."""
    ref = GOLDEN["chain_L8_sz0_by_momentum"]
    L = ref["L"]
    mk = lambda **kw: q.csr_mat.kondo(L, ref["n_elec"], ref["two_sz"], chain(L), t=ref["t"], J_K=ref["J_K"], **kw)
    A, M = mk(opts=q.make_opts(**PLAIN)), mk(matrix_free=True)
    assert M.dim == A.dim == 739162 and M.nnz == A.nnz
    assert M.dim > 256 * 2048 and M.dim % 256 != 0
    n = A.dim
    x = _rand(n, 15)
    va, vm = A.vec(2), M.vec(2)
    va.upload(x, 0)
    vm.upload(x, 0)
    da, na = A.spmv(va.at(0), va.at(n), want_red=True)
    dm, nm = M.spmv(vm.at(0), vm.at(n), want_red=True)
    ya, ym = va.download(n, n), vm.download(n, n)
    va.free()
    vm.free()
    assert np.abs(ym - ya).max() <= 1e-13 * np.abs(ya).max()
    assert abs(da - dm) <= 1e-12 * abs(da) and abs(na - nm) <= 1e-12 * na
    ra, rm = q.locate_E0_lanczos(A, nev=1, ncv=0), q.locate_E0_lanczos(M, nev=1, ncv=0)
    print("L = 8: E0 = %.10f (stored %.10f)" % (rm.E0, ra.E0))
    assert abs(ra.E0 - rm.E0) <= 1e-10 * abs(ra.E0)
    assert rm.E0 <= min(ref["E0_by_k"].values()) + 1e-8


# ---- 6. ragged row shards ----

def test_row_shards_reproduce_the_rows_of_the_whole_operator():
    n = 6
    T = kondo.terms(n, chain(n), 1.0, 1.1, 0.3)
    mk = lambda **kw: q.csr_mat.kondo(n, n, 0, None, U=0.7, terms=T, **kw)
    whole = mk(matrix_free=True)
    dim = whole.dim
    assert dim == 15184
    x, y0 = _rand(dim, 31), _rand(dim, 32)
    vw = whole.vec(2)
    vw.upload(x, 0)
    vw.upload(y0, dim)
    whole.spmv(vw.at(0), vw.at(dim), 0.6, -1.2, 0.3)
    y = vw.download(dim, dim)
    vw.free()
    # s is the most significant field and a block of one s holds at most C(6,3)^2 = 400 words: the shards span many blocks of
    # different n_up, and the cuts fall inside a block (its rows on both sides of the cut) unless they hit its first row
    _, _, s = kondo.fields(kondo.words(n, n, 0), n)
    inside = [bool(s[c - 1] == s[c]) for c in (dim // 2, 17, 80, dim // 3 + 1, dim - 5)]
    print("cuts inside a block of s:", inside)
    assert any(inside) and len(set(s[80:dim // 3 + 1].tolist())) > 1
    nnz = 0
    for cuts in ([0, dim // 2, dim], [0, 17, 80, dim // 3 + 1, dim - 5, dim]):
        for r0, r1 in zip(cuts[:-1], cuts[1:]):
            S = mk(rows=(r0, r1), matrix_free=True)
            i = S.info()
            assert S.dim == i.nrows == r1 - r0 and i.row_offset == r0 and i.ncols == dim and i.kernel == _lib.KERNEL_MATRIX_FREE
            Ts = mk(rows=(r0, r1), opts=q.make_opts(**PLAIN))
            assert S.nnz == Ts.nnz
            nnz += S.nnz
            vx, vy = q.DeviceVec(S, dim), q.DeviceVec(S, r1 - r0)
            vx.upload(x)
            vy.upload(y0[r0:r1])
            S.spmv(vx.ptr, vy.ptr, 0.6, -1.2, 0.3)
            got = vy.download()
            assert np.array_equal(got.view(np.uint64), y[r0:r1].view(np.uint64)), (r0, r1)
            vx.free()
            vy.free()
    assert nnz == 2 * whole.nnz


# ---- 7. rows above 2^33 ----

def test_deep_rows_of_the_L13_sector():
    """(13, 13, 0) on the chain, rows [15,000,000,000, 15,000,004,096) of 15,148,345,760: the handle holds its tables and no
    vector, and its nnz, counted on the device, equals the count made here from kondo.unrank and the moves each word allows.
    This is the one device check of 64-bit unranking above 2^33 that needs no 121 GB vector: nothing is applied."""
    import torch
    n, r0, r1 = 13, 15_000_000_000, 15_000_004_096
    free0 = torch.cuda.mem_get_info()[0]
    M = q.csr_mat.kondo(n, n, 0, chain(n), t=1.0, J_K=1.1, rows=(r0, r1), matrix_free=True)
    used = free0 - torch.cuda.mem_get_info()[0]
    i = M.info()
    assert i.ncols == 15_148_345_760 and i.nrows == r1 - r0 and i.row_offset == r0 and i.kernel == _lib.KERNEL_MATRIX_FREE
    assert 0 < i.bytes_matrix < 4 << 20
    assert used < 64 << 20, used                                               # a vector of the sector has 121 GB and more
    pairs = sorted({(a, b) for (a, b) in chain(n)} | {(b, a) for (a, b) in chain(n)})
    want = 0
    for r in range(r0, r1):
        u, d, s = kondo.unrank(n, n, 0, r)
        assert kondo.rank(n, n, 0, u, d, s) == r
        c = 1
        for occ in (u, d):
            c += sum(1 for (a, b) in pairs if (occ >> a) & 1 and not (occ >> b) & 1)
        for k in range(n):
            iu, idn, isd = (u >> k) & 1, (d >> k) & 1, (s >> k) & 1
            c += 1 if iu != idn and iu == isd else 0                           # electron and local spin antiparallel
        want += c
    assert M.nnz == want


# ---- 8. packed-real drivers ----

def test_packed_real_drivers():
    """qbh_lanczos_real_dev (with a continuation after 40 steps) and qbh_eigenvec_cg_real_dev on the matrix-free chain L = 6
    against the complex interface on the stored operator."""
    L = 6
    A = q.csr_mat.kondo(L, L, 0, chain(L), t=1.0, J_K=1.1, opts=q.make_opts(**PLAIN))
    M = q.csr_mat.kondo(L, L, 0, chain(L), t=1.0, J_K=1.1, matrix_free=True)
    n, maxit = A.dim, 400
    ref = q.locate_E0_lanczos(A, nev=1, ncv=1, maxit=maxit)
    vc = A.vec(2)
    A.randomize(vc.at(0), 1)
    hc = np.zeros(2 * maxit)
    mc = q.lanczos(0, maxit - 1, maxit, n, A, None, hc, "sr_val0", device_v=vc)
    buf = q.DeviceVec(M, 2 * n + 2)                            # 4 slots of n packed doubles: v, r, p, pp
    at = lambda j: C.c_void_p(buf.ptr.value + 8 * n * j)
    lan = type("V", (), {"ptr": at(0)})()                      # slots 0, 1 are the two Lanczos vectors
    _lib.check(_lib.lib().qbh_vec_randomize_real(M.handle, at(0), C.c_uint32(1)), "qbh_vec_randomize_real")
    hr = np.zeros(2 * maxit)
    m1 = q.lanczos_real(0, 40, maxit, M, lan, hr)
    assert m1 == 40
    m2 = q.lanczos_real(m1, maxit - 1 - m1, maxit, M, lan, hr, state=q.lanczos_real.last["state"])
    assert abs(m2 - mc) <= 1
    assert np.allclose(hr[maxit:maxit + 30], hc[maxit:maxit + 30], rtol=1e-9, atol=1e-11)     # a_0 .. a_29
    assert np.allclose(hr[1:31], hc[1:31], rtol=1e-9, atol=1e-11)                               # b_1 .. b_30
    ritz, _ = q.hess_eigen(hr, maxit, m2, "sr")
    assert abs(ritz[0] - ref.E0) <= 1e-11 * abs(ref.E0)
    _lib.check(_lib.lib().qbh_vec_randomize_real(M.handle, at(0), C.c_uint32(1)), "qbh_vec_randomize_real")
    mcg, accu = q.eigenvec_CG_real(maxit, 0, M, ritz[0], at(0), at(1), at(2), at(3))
    assert accu < 2e-12
    vec = buf.download(0, (n + 1) // 2).view(np.float64)[:n]
    assert abs(np.linalg.norm(vec) - 1.0) < 1e-10
    assert abs(abs(np.vdot(ref.eigenvecs, vec)) - 1.0) < 1e-8
    assert M.stats().n_spmv_real > 0
    vc.free()
    buf.free()


# ---- 9. the decoupled limit ----

def _dense_through_spmv(H):
    out = np.empty((H.dim, H.dim), dtype=np.complex128)
    e, y = np.zeros(H.dim, dtype=np.complex128), np.empty(H.dim, dtype=np.complex128)
    for k in range(H.dim):
        e[:] = 0
        e[k] = 1.0
        H.MultMv(e, y)
        out[:, k] = y
    return out


def test_without_coupling_the_lowest_energy_is_hubbards():
    """J_K = 0 and no exchange at (4, 4, 0): the local spins idle, so E0 is the lowest Hubbard E0 over the blocks
    (n_up, n_dn) = (m, 4 - m).  The Hubbard side is qbh_mf_hubbard, which shares nothing with kd_row_terms: this guards the
    fermion sign and the column of the hop shortcut on their own."""
    n, U = 4, 1.3
    M = q.csr_mat.kondo(n, 4, 0, chain(n), t=1.0, J_K=0.0, U=U, matrix_free=True)
    assert M.dim == 346
    got = np.linalg.eigvalsh(_dense_through_spmv(M))
    want = []
    for (n_up, n_dn, m) in kondo.sector_blocks(n, 4, 0):
        H = q.csr_mat.hubbard(n, n_up, n_dn, chain(n), t=1.0, U=U, matrix_free=True)
        assert H.info().kernel == _lib.KERNEL_MATRIX_FREE
        want.extend(list(np.linalg.eigvalsh(_dense_through_spmv(H))) * comb(n, m))
    want = np.sort(want)
    assert got.shape == want.shape and np.abs(got - want).max() <= 1e-10 * max(1.0, np.abs(want).max())
    res = q.locate_E0_lanczos(M, nev=1, ncv=0)
    assert abs(res.E0 - want[0]) <= 1e-9 * max(1.0, abs(want[0]))
