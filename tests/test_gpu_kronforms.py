"""The complex128 Kronecker split H = H_near + H_far (+ H_cross), element by element.

kron_build accepts any operator from host arrays that names kron_minor and whose entries each keep the major or the minor index, so
the synthetic product-structured operators of tests/kronforms.py reach every path of k_spmv_wave2 (pass forms 0 to 4, both column
widths, static and dynamic walks, the wave-private row buffer, cut groups, the row-at-a-time path) and of the kernels of
qbh_kron.hip / qbh_kron_prep.hip at a few thousand rows.  Every case first asserts the route it claims against the mirror
(kronforms.route: kron_minor, kron_band, kron_sliced, kron_inplace, kron_far_nnz, kron_cross_nnz, kron_cols16), then compares every
row with a long-double reference within the bounds derived in kronforms (one GPU: csrforms.epilogue's (nnz_i + 4) eps S_i unchanged).
|a_ij| >= 0.5 and |x_j| >= 0.5, so a dropped, doubled or misplaced term of any row is far outside its bound
(tests/test_kronforms.py).  A failure names the worst row as (u, d), its near and far lengths and its error / bound.

Largest error / bound seen on an MI355X: a. qbh_spmv_dev 0.16 (wide_major), c. the solver's step 0.10 (near_600), d. row shards 0.14
(near_300), e. one-rank communicator 0.061 (edge), f. several classes 0.084 (chain16); b. the downloads are exact.  Every test prints
its own figure (pytest -s); the slowest case takes 4.7 s (the first communicator case, which loads RCCL), every other under 2 s.
"""
import numpy as np
import pytest

import kronforms as kf
import quantum_basis_amd as q
from quantum_basis_amd import _lib, lattices

pytestmark = pytest.mark.gpu

L = np.longdouble
TRIPLES = [(1.0, 0.0, 0.0), (1.0, 1.0, 0.0), (0.7, -1.3, 0.0), (1.0, 0.0, -2.5), (-0.6, 0.8, 1.75)]
COMMON = dict(value_dict=0, real_fast_path=0, check_hermitian=0, basis_detect=0, autotune=0, kron_split=2)
WALKS = (-1, 0, 1, 2)


def _bits(a):
    return np.ascontiguousarray(a).view(np.float64)


def _operator(name, rows=None, **kw):
    """-> (operator, mirror) of a profile created with the common options, the profile's own and kw."""
    dim, ia, ja, val, S, NU = kf.make(name)
    o = dict(kf.profile_opts(name))
    o.update(kw)
    r = kf.route(ia, ja, S, o, rows=rows)
    A = q.csr_mat(dim, ia, ja, val, sym=False, opts=q.make_opts(kron_minor=S, **dict(COMMON, **o)), rows=rows)
    return A, r


def _assert_route(what, info, r):
    got = {k: int(getattr(info, k)) for k in kf.INFO_FIELDS}
    want = {k: int(r[k]) for k in kf.INFO_FIELDS}
    assert got == want, "%s: qbh_csr_info reports %r, the mirror says %r" % (what, got, want)
    assert info.kron_classes == 1


def _check_rows(what, got, ref, S, near, far):
    ratio, text = kf.worst_row(got, ref, S, near, far)
    assert ratio <= 1.0, "%s: %s" % (what, text)
    return ratio


def _check_red(what, dot, nrm, ref):
    d = abs(complex(dot) - complex(ref["dot"]))
    assert d <= float(ref["t_dot"]), "%s: <x, y> = %r, reference %r (|diff| %.3e > %.3e)" % (what, dot, complex(ref["dot"]), d,
                                                                                            float(ref["t_dot"]))
    d = abs(nrm - float(ref["nrm"]))
    assert d <= float(ref["t_nrm"]), "%s: |y|^2 = %r, reference %r (|diff| %.3e > %.3e)" % (what, nrm, float(ref["nrm"]), d,
                                                                                           float(ref["t_nrm"]))


class _Run:
    """x (ncols) and y (nrows) in one device buffer of the operator."""

    def __init__(self, A, x):
        self.A, self.n, self.ncols = A, A.dim, len(x)
        self.v = q.DeviceVec(A, self.ncols + self.n)
        self.v.upload(x, 0)

    def __call__(self, y0, alpha, beta, gamma, red):
        self.v.upload(y0, self.ncols)
        out = self.A.spmv(self.v.at(0), self.v.at(self.ncols), alpha, beta, gamma, want_red=red)
        return self.v.download(self.ncols, self.n), out

    def free(self):
        self.v.free()


class _Case:
    """Reference of a profile (or of rows [r0, r1) of it) for the five triples: computed once per test."""

    def __init__(self, name, rows=None, extra=0):
        self.name = name
        self.dim, self.ia, self.ja, self.val, self.S, self.NU = kf.make(name)
        r0, r1 = (0, self.dim) if rows is None else rows
        self.rows = (r0, r1)
        self.x = kf.probe(name, self.dim, 1)
        self.y0 = kf.probe(name, self.dim, 2)[r0:r1]
        near, far = kf.structure(self.ia, self.ja, self.S, self.dim)
        self.near, self.far = near[r0:r1], far[r0:r1]
        s, abs_s = kf.row_sums(self.ia, self.ja, self.val, self.x)
        self.nnz_row = np.diff(self.ia)[r0:r1]
        self.refs = [kf.epilogue(s[r0:r1], abs_s[r0:r1], self.nnz_row, self.x[r0:r1], self.y0, a, b, g, extra=extra) for a, b, g in TRIPLES]
        self.nan = np.full(r1 - r0, np.nan + 1j * np.nan)

    def sweep(self, what, A, repeat=True):
        """The five triples on A: rows and reductions within their bounds; at the third triple three calls bit-identical in y and in
        the reductions (every walk: the dynamic walk reduces per chunk of blocks in a fixed order) and y the same without the
        reductions.  -> ([y per triple], largest error / bound)."""
        run = _Run(A, self.x)
        ys, top = [], 0.0
        try:
            for t, (alpha, beta, gamma) in enumerate(TRIPLES):
                yin = self.nan if beta == 0.0 else self.y0            # beta = 0 must never read y
                y, (dot, nrm) = run(yin, alpha, beta, gamma, True)
                tag = "%s (alpha, beta, gamma) = %r" % (what, (alpha, beta, gamma))
                top = max(top, _check_rows(tag, y, self.refs[t], self.S, self.near, self.far))
                _check_red(tag, dot, nrm, self.refs[t])
                if t == 2 and repeat:
                    for _ in range(2):
                        y2, (dot2, nrm2) = run(yin, alpha, beta, gamma, True)
                        assert np.array_equal(_bits(y2), _bits(y)), "%s: y differs between calls" % tag
                        assert (dot2, nrm2) == (dot, nrm), "%s: reductions differ between calls: %r, %r" % (tag, (dot, nrm), (dot2, nrm2))
                    y3, _ = run(yin, alpha, beta, gamma, False)
                    assert np.array_equal(_bits(y3), _bits(y)), "%s: y differs without the reductions" % tag
                ys.append(y)
        finally:
            run.free()
        return ys, top


def _same(what, ys, base, S, mask=None):
    for t, (y, b) in enumerate(zip(ys, base)):
        diff = np.nonzero((_bits(y).reshape(-1, 2) != _bits(b).reshape(-1, 2)).any(axis=1) & (True if mask is None else mask))[0]
        assert len(diff) == 0, "%s, triple %d: %d rows differ in the last bits, first (u, d) = (%d, %d): %r against %r" % (
            what, t, len(diff), diff[0] // S, diff[0] % S, y[diff[0]], b[diff[0]])


# ------------------------------------------------------------------------------------------------- a. qbh_spmv_dev --
@pytest.mark.parametrize("name", kf.PROFILES)
def test_spmv_every_walk_and_column_width(name):
    """Static and dynamic walks x deterministic x both column widths (uniform: every band width too): every row and both fused
    reductions within their bounds; y bit-identical between calls, with and without the reductions, and ACROSS all walks and both
    column widths (a row's products are summed inside one block in the same way whichever wavefront takes it; a cut group is two
    addends, and the cuts are the same slots for every walk and width)."""
    c = _Case(name)
    variants = [dict(wave_walk=w, deterministic=det, kron_cols16=c16) for w in WALKS for det in (0, 1) for c16 in (0, 1)]
    base = None
    top = 0.0
    for v in variants:
        what = "%s %r" % (name, v)
        A, r = _operator(name, **v)
        try:
            _assert_route(what, A.info(), r)
            ys, ratio = c.sweep(what, A)
        finally:
            A.destroy()
        top = max(top, ratio)
        if base is None:
            base = ys
        else:
            _same(what + " against " + str(variants[0]), ys, base, c.S)
    if name == "uniform":
        for band in (2, 4, 8, 16):
            ref_band = None
            for c16 in (0, 1):
                what = "%s band %d cols16 %d" % (name, band, c16)
                A, r = _operator(name, kron_band=band, kron_cols16=c16)
                try:
                    _assert_route(what, A.info(), r)
                    ys, ratio = c.sweep(what, A)
                finally:
                    A.destroy()
                top = max(top, ratio)
                if ref_band is None:
                    ref_band = ys
                else:
                    _same(what, ys, ref_band, c.S)
    print("a. %s: largest error / bound %.3g" % (name, top))


# ----------------------------------------------------------------------------------------------- b. qbh_csr_download --
@pytest.mark.parametrize("name", kf.PROFILES)
def test_download_returns_the_input_rows(name):
    """The whole operator and three row ranges -- starting inside a group of 8, starting inside the edge band (the last band where
    none is narrow), a single row -- merged back from the parts: the input arrays bit for bit, no padding slot among them."""
    dim, ia, ja, val, S, NU = kf.make(name)
    u = min(2, NU - 1)
    ranges = [(0, dim), (min(S + 3, dim - 1), min(3 * S + 8, dim)), (u * S + S - 1, min(dim, u * S + 2 * S + 1)), (dim // 2 + 1, dim // 2 + 2)]
    for c16 in (0, 1):
        A, r = _operator(name, kron_cols16=c16)
        try:
            _assert_route("%s cols16 %d" % (name, c16), A.info(), r)
            for r0, r1 in ranges:
                dia, dja, dval = A.download(r0, r1)
                what = "%s cols16 %d rows [%d, %d)" % (name, c16, r0, r1)
                assert np.array_equal(dia, ia[r0:r1 + 1] - ia[r0]), what + ": row pointers"
                assert np.array_equal(dja.astype(np.int64), ja[ia[r0]:ia[r1]]), what + ": columns"
                assert np.array_equal(_bits(dval), _bits(val[ia[r0]:ia[r1]])), what + ": values"
            assert A.info().kron_minor == S                     # still split: the download merges into scratch arrays
        finally:
            A.destroy()


# ------------------------------------------------------------------------------------------------ c. the solver's step --
MAXIT = 4
B1 = 1.3


@pytest.mark.parametrize("pipeline", [1, 0])
@pytest.mark.parametrize("name", ["uniform", "graded", "edge", "ragged_light", "near_600"])
def test_lanczos_two_steps_element_by_element(name, pipeline):
    """Two continuation steps (k = 1, np = 2) on slot 0 = z, slot 1 = x with hess[1] = b1.  In the pipelined loop the second SpMV takes
    its coefficients from device memory, reads its beta vector out of place and gathers its far part from the tiled copy the axpy
    before it wrote; no statistic of the library tells which loop ran (lanczos_core falls back to the unpipelined one by itself, e.g.
    without room for its third vector), so lanczos_pipeline = 1 asks for that route and the test does not verify that it was taken.
    (H v2)_i = b3 v3_i + a2 v2_i + b2 x_i is compared with the long-double product of the input arrays and the v2 the solver hands
    back, a1, b2 (first step) and a2, b3 (second) with their references (kronforms.step_bound)."""
    dim, ia, ja, val, S, NU = kf.make(name)
    near, far = kf.structure(ia, ja, S, dim)
    nnz_row = np.diff(ia)
    x = kf.probe(name, dim, 3)
    x = x / np.linalg.norm(x)
    z = kf.probe(name, dim, 4)
    A, r = _operator(name, lanczos_pipeline=pipeline)
    what = "%s lanczos_pipeline %d" % (name, pipeline)
    try:
        _assert_route(what, A.info(), r)
        vv = np.concatenate([z, x]).astype(np.complex128)
        hess = np.zeros(2 * MAXIT)
        hess[1] = B1
        m = q.lanczos(1, 2, MAXIT, dim, A, vv, hess, "dnmcs")
        assert A.info().kron_minor == S
    finally:
        A.destroy()
    assert m == 3
    v2, v3 = vv[:dim].copy(), vv[dim:].copy()
    a1, a2, b2, b3 = hess[MAXIT + 1], hess[MAXIT + 2], hess[2], hess[3]
    s1, abs1 = kf.row_sums(ia, ja, val, x)
    ref1 = kf.step_bound(s1, abs1, nnz_row, x, a1, z, B1)
    assert abs(a1 - float(ref1["a"])) <= float(ref1["t_a"]), "%s: a1 = %.17g, reference %.17g (bound %.3e)" % (what, a1, float(ref1["a"]), float(ref1["t_a"]))
    assert abs(b2 - float(ref1["b"])) <= float(ref1["t_b"]), "%s: b2 = %.17g, reference %.17g (bound %.3e)" % (what, b2, float(ref1["b"]), float(ref1["t_b"]))
    s2, abs2 = kf.row_sums(ia, ja, val, v2)
    ref2 = kf.step_bound(s2, abs2, nnz_row, v2, a2, x, b2)
    recon = L(b3) * v3.astype(kf.CL) + L(a2) * v2.astype(kf.CL) + L(b2) * x.astype(kf.CL)
    ratio = _check_rows(what + ": b3 v3 + a2 v2 + b2 x against H v2", recon, ref2, S, near, far)
    assert abs(a2 - float(ref2["a"])) <= float(ref2["t_a"]), "%s: a2 = %.17g, reference %.17g (bound %.3e)" % (what, a2, float(ref2["a"]), float(ref2["t_a"]))
    assert abs(b3 - float(ref2["b"])) <= float(ref2["t_b"]), "%s: b3 = %.17g, reference %.17g (bound %.3e)" % (what, b3, float(ref2["b"]), float(ref2["t_b"]))
    print("c. %s: largest error / bound %.3g; a1 %.3g, b2 %.3g, a2 %.3g, b3 %.3g of their bounds" % (
        what, ratio, abs(a1 - float(ref1["a"])) / float(ref1["t_a"]), abs(b2 - float(ref1["b"])) / float(ref1["t_b"]),
        abs(a2 - float(ref2["a"])) / float(ref2["t_a"]), abs(b3 - float(ref2["b"])) / float(ref2["t_b"])))


# ----------------------------------------------------------------------------------------------------- d. row shards --
@pytest.mark.parametrize("name", ["uniform", "edge", "near_300"])
def test_row_shards_of_whole_major_indices(name):
    """rows = (u0 * S, u1 * S) of the same host arrays, driven with the full-length x: the rows of the reference within their bounds,
    and bit-identical to the same rows of the whole operator -- except the rows whose far group a block boundary cuts in either of
    the two: a cut group is two partial sums added, and a shard's sliced far stream is cut at other slots than the whole operator's
    (qbh_spmv_wave.hip documents the two addends; where they fall is the layout's business).  Those rows are held to their bounds."""
    dim, ia, ja, val, S, NU = kf.make(name)
    whole = _Case(name)
    A, r = _operator(name)
    try:
        _assert_route(name, A.info(), r)
        base, _ = whole.sweep(name, A, repeat=False)
    finally:
        A.destroy()
    cut_whole = kf.cut_rows(r)
    cuts = [0, NU // 3, 2 * (NU // 3), NU]
    top = 0.0
    for k in range(3):
        rows = (cuts[k] * S, cuts[k + 1] * S)
        c = _Case(name, rows=rows)
        for c16 in (0, 1):
            what = "%s shard [%d, %d) cols16 %d" % (name, rows[0], rows[1], c16)
            A, rs = _operator(name, rows=rows, kron_cols16=c16)
            try:
                assert (A.dim, A.row_offset, A.ncols) == (rows[1] - rows[0], rows[0], dim)
                _assert_route(what, A.info(), rs)
                ys, ratio = c.sweep(what, A)
            finally:
                A.destroy()
            top = max(top, ratio)
            uncut = ~(kf.cut_rows(rs) | cut_whole[rows[0]:rows[1]])
            assert uncut.sum() > len(uncut) // 2
            _same(what + " against the whole operator", ys, [b[rows[0]:rows[1]] for b in base], S, mask=uncut)
    print("d. %s: largest error / bound %.3g" % (name, top))


# ---------------------------------------------------------------------------------------- e. one-rank communicator --
@pytest.mark.parametrize("name", ["uniform", "edge", "ragged_light"])
def test_one_rank_native_communicator(name):
    """Under a communicator: near pass without far addend (OPS 1), k_kron_place, far pass, cross rows, k_kron_combine; the bounds
    carry the one rounding more that kronforms derives for this form."""
    from quantum_basis_amd import dist as qdist
    dim, ia, ja, val, S, NU = kf.make(name)
    c = _Case(name, extra=kf.COMBINE_EXTRA)
    top = 0.0
    for c16 in (0, 1):
        what = "%s one-rank communicator cols16 %d" % (name, c16)
        A, r = _operator(name, kron_cols16=c16)
        try:
            qdist.NativeComm(dim, rank=0, world=1).attach(A)
            _assert_route(what, A.info(), r)                     # still split
            n_gather = A.stats().n_gather
            ys, ratio = c.sweep(what, A)
            assert A.stats().n_gather >= n_gather + len(TRIPLES), "%s: the SpMV did not go through the gather" % what
        finally:
            A.destroy()
        top = max(top, ratio)
    print("e. %s: largest error / bound %.3g" % (name, top))


# ------------------------------------------------------------------------------------------------ f. several classes --
SECTORS = {"chain16": (16, 8, lattices.chain(16), 8), "kagome18": (18, 9, lattices.kagome(3, 2), 9)}


@pytest.mark.parametrize("cross_in_near", [1, 0])
@pytest.mark.parametrize("name", ["chain16", "kagome18"])
def test_cut_sector_element_by_element(name, cross_in_near):
    """A single-species sector cut into classes (OPS 4; kron_cross_in_near = 0: the entries across the cut as a third pass) against the
    long-double product of the unsplit operator's downloaded arrays, in the caller's order."""
    n, k, bonds, h = SECTORS[name]
    plain = dict(value_dict=0, real_fast_path=0)
    P = q.csr_mat.heisenberg(n, k, bonds, J=1.0, opts=q.make_opts(kron_split=0, **plain))
    ia, ja, val = P.download()
    dim = P.dim
    P.destroy()
    ja = ja.astype(np.int64)
    K = q.csr_mat.heisenberg(n, k, bonds, J=1.0, opts=q.make_opts(kron_split=2, basis_kind=_lib.BASIS_SPIN_SECTOR, n_sites=n, n_up=h, n_dn=k,
                                                                  kron_cross_in_near=cross_in_near, **plain))
    what = "%s h = %d kron_cross_in_near %d" % (name, h, cross_in_near)
    try:
        info = K.info()
        assert info.kron_classes > 1 and info.kron_inplace == 1 and info.kron_sliced == 1 and info.nnz == ia[-1], what
        assert (info.kron_cross_nnz == 0) if cross_in_near else (0 < info.kron_cross_nnz < 0.4 * info.nnz), what
        x, y0 = kf.probe_vector(dim, 5), kf.probe_vector(dim, 6)
        s, abs_s = kf.row_sums(ia, ja, val, x)
        nnz_row = np.diff(ia)
        v = K.vec(2)
        top = 0.0
        try:
            for alpha, beta, gamma in TRIPLES:
                ref = kf.epilogue(s, abs_s, nnz_row, x, y0, alpha, beta, gamma, extra=0 if cross_in_near else kf.CROSS_PASS_EXTRA)
                v.upload(x, 0)
                v.upload(np.full(dim, np.nan + 1j * np.nan) if beta == 0.0 else y0, dim)
                dot, nrm = K.spmv(v.at(0), v.at(dim), alpha, beta, gamma, want_red=True)
                y = v.download(dim, dim)
                tag = "%s (alpha, beta, gamma) = %r" % (what, (alpha, beta, gamma))
                # the rows of a cut sector belong to classes with (u, d) of their own, which only the library knows: the caller's row
                # and its length name the row here
                i, ratio, over, err = kf.worst(y, ref)
                assert ratio <= 1.0, "%s: row %d (%d entries): |y - ref| = %.3e, bound %.3e, error / bound %.3g; %d rows over" % (
                    tag, i, int(nnz_row[i]), err, float(ref["bound"][i]), ratio, over)
                _check_red(tag, dot, nrm, ref)
                top = max(top, ratio)
        finally:
            v.free()
    finally:
        K.destroy()
    print("f. %s: largest error / bound %.3g" % (what, top))
