"""The complex CSR SpMV forms and their fused epilogue, element by element.

qbh_spmv_dev on an operator without product structure runs k_spmv_stream, k_spmv_vector, k_spmv_rows or k_spmv_wave, coded or
uncoded, and fuses y <- alpha*Hx + beta*y + gamma*x_local with <x_local, y> and |y|^2.  Every case here first asserts the route
it claims (info.kernel, info.value_dict, info.n_blocks against the mirror in tests/csrforms.py, which also names the TPR
instance), then compares every row with a long-double reference within the bound derived in csrforms.epilogue:

    |y_i - ref_i| <= (nnz_i + 4) eps (|alpha| sum_j |a_ij||x_j| + |beta||y_i| + |gamma||x_i|)

and both reductions within bounds built from those.  |x_j| >= 0.5 and |a_ij| >= 0.5, so a dropped, doubled or misplaced term of
any row is far outside its bound.  A failure names the worst row, its length and its error / bound.
"""
import ctypes as C
import time

import numpy as np
import pytest

import csrforms as cf
import quantum_basis_amd as q
from quantum_basis_amd import _lib

pytestmark = pytest.mark.gpu

L = np.longdouble
TRIPLES = [(1.0, 0.0, 0.0), (1.0, 1.0, 0.0), (0.7, -1.3, 0.0), (1.0, 0.0, -2.5), (-0.6, 0.8, 1.75)]
BASE = dict(check_hermitian=0, kron_split=0, basis_detect=0, autotune=0)


def _opts(f, **kw):
    o = dict(BASE)
    o.update(f)
    o.update(kw)
    return q.make_opts(**o)


def _assert_route(what, info, r):
    assert info.kernel == r["info_kernel"], "%s: ran kernel %d, the mirror says %s" % (what, info.kernel, r["kernel"])
    assert info.value_dict == r["n_dict"], "%s: value_dict %d, the mirror says %d" % (what, info.value_dict, r["n_dict"])
    assert info.n_blocks == r["n_blocks"], "%s: %d row blocks, the mirror says %d" % (what, info.n_blocks, r["n_blocks"])


def _check_rows(what, got, ref, ia):
    i, ratio, over, err = cf.worst(got, ref)
    assert ratio <= 1.0, "%s: row %d (length %d): |y - ref| = %.3e, bound %.3e, error / bound %.3g; %d rows over" % (
        what, i, int(ia[i + 1] - ia[i]), err, float(ref["bound"][i]), ratio, over)


def _check_red(what, dot, nrm, ref):
    d = abs(complex(dot) - complex(ref["dot"]))
    assert d <= float(ref["t_dot"]), "%s: <x, y> = %r, reference %r (|diff| %.3e > %.3e)" % (what, dot, complex(ref["dot"]), d,
                                                                                            float(ref["t_dot"]))
    d = abs(nrm - float(ref["nrm"]))
    assert d <= float(ref["t_nrm"]), "%s: |y|^2 = %r, reference %r (|diff| %.3e > %.3e)" % (what, nrm, float(ref["nrm"]), d,
                                                                                           float(ref["t_nrm"]))


class _Run:
    """x (ncols) and y (nrows) in one device buffer of the operator."""

    def __init__(self, A, x, ncols):
        self.A, self.n, self.ncols = A, A.dim, ncols
        self.v = q.DeviceVec(A, ncols + self.n)
        self.v.upload(x, 0)

    def __call__(self, y0, alpha, beta, gamma, red):
        self.v.upload(y0, self.ncols)
        out = self.A.spmv(self.v.at(0), self.v.at(self.ncols), alpha, beta, gamma, want_red=red)
        return self.v.download(self.ncols, self.n), out

    def free(self):
        self.v.free()


def _sweep_one(what, A, r, ia_rows, x, xl, y0, s, abs_s, refs, nnz_row, ncols):
    run = _Run(A, x, ncols)
    nan = np.full(A.dim, np.nan + 1j * np.nan)
    try:
        for t, (alpha, beta, gamma) in enumerate(TRIPLES):
            ref = refs[t]
            yin = nan if beta == 0.0 else y0                 # beta = 0 must never read y
            y, (dot, nrm) = run(yin, alpha, beta, gamma, True)
            tag = "%s (alpha, beta, gamma) = %r" % (what, (alpha, beta, gamma))
            _check_rows(tag, y, ref, ia_rows)
            _check_red(tag, dot, nrm, ref)
            if t == 2:
                # bit-identical over three calls, without the reductions too; static walks: the reductions as well
                for _ in range(2):
                    y2, (dot2, nrm2) = run(yin, alpha, beta, gamma, True)
                    assert np.array_equal(y2.view(np.float64), y.view(np.float64)), "%s: y differs between calls" % tag
                    if r["walk"] != 3:
                        assert (dot2, nrm2) == (dot, nrm), "%s: reductions differ between calls" % tag
                y3, _ = run(yin, alpha, beta, gamma, False)
                assert np.array_equal(y3, y), "%s: y differs without the reductions" % tag
    finally:
        run.free()


def _refs(s, abs_s, nnz_row, xl, y0):
    return [cf.epilogue(s, abs_s, nnz_row, xl, y0, a, b, g) for a, b, g in TRIPLES]


@pytest.mark.parametrize("case", cf.all_profile_cases(), ids=lambda c: "%s-%s" % c)
def test_every_form_on_every_profile(case):
    name, kind = case
    d = cf.make(name, kind)
    ia, ja, val = d["full"]
    n = d["n"]
    x = cf.probe_vector(n, 1)
    y0 = cf.probe_vector(n, 2)
    s, abs_s = cf.row_sums(ia, ja, val, x)
    nnz_row = np.diff(ia)
    refs = _refs(s, abs_s, nnz_row, x, y0)
    for f, r in cf.sweep(ia, val):
        what = "%s/%s %s -> %s" % (name, kind, f, r["key"])
        A = q.csr_mat(n, d["ia"], d["ja"], d["val"], sym=d["sym"], opts=_opts(f))
        try:
            _assert_route(what, A.info(), r)
            _sweep_one(what, A, r, ia, x, x, y0, s, abs_s, refs, nnz_row, n)
            if f.get("deterministic"):
                # two handles of the same arrays: bit-identical y and reductions
                B = q.csr_mat(n, d["ia"], d["ja"], d["val"], sym=d["sym"], opts=_opts(f))
                try:
                    ra, rb = _Run(A, x, n), _Run(B, x, n)
                    ya, red_a = ra(y0, 0.7, -1.3, 0.5, True)
                    yb, red_b = rb(y0, 0.7, -1.3, 0.5, True)
                    ra.free(), rb.free()
                    assert np.array_equal(ya.view(np.float64), yb.view(np.float64)) and red_a == red_b, what
                finally:
                    B.destroy()
        finally:
            A.destroy()


SHARD_FORMS = [dict(spmv_kernel=cf.KERNEL_WAVE, value_dict=0), dict(spmv_kernel=cf.KERNEL_WAVE, value_dict=0, wave_walk=3),
               dict(spmv_kernel=cf.KERNEL_ROWS, value_dict=0), dict(spmv_kernel=cf.KERNEL_ROWS, value_dict=1),
               dict(spmv_kernel=cf.KERNEL_STREAM, value_dict=1), dict(spmv_kernel=cf.KERNEL_VECTOR, value_dict=0)]


@pytest.mark.parametrize("case", [("const20", "few"), ("empty_runs", "complex"), ("sym_rand", "complex"), ("bimodal300", "complex")],
                         ids=lambda c: "%s-%s" % c)
def test_row_shards_use_their_own_x_block(case):
    """csr_mat(..., rows=(r0, r1)) with r0 on no block boundary: y and the gamma / reduction terms use x[r0:r1]."""
    name, kind = case
    d = cf.make(name, kind)
    ia, ja, val = d["full"]
    n = d["n"]
    r0, r1 = 777, n - 333
    x = cf.probe_vector(n, 3)
    sia = ia[r0:r1 + 1] - ia[r0]
    sja, sval = ja[ia[r0]:ia[r1]], val[ia[r0]:ia[r1]]
    s, abs_s = cf.row_sums(sia, sja, sval, x)
    xl = x[r0:r1]
    y0 = cf.probe_vector(r1 - r0, 4)
    refs = _refs(s, abs_s, np.diff(sia), xl, y0)
    for f in SHARD_FORMS:
        r = cf.route(f["spmv_kernel"], f["value_dict"], sia, sval, wave_walk=f.get("wave_walk", -1))
        what = "%s/%s shard [%d, %d) %s -> %s" % (name, kind, r0, r1, f, r["key"])
        A = q.csr_mat(n, d["ia"], d["ja"], d["val"], sym=d["sym"], opts=_opts(f), rows=(r0, r1))
        try:
            assert (A.dim, A.row_offset, A.ncols) == (r1 - r0, r0, n)
            _assert_route(what, A.info(), r)
            _sweep_one(what, A, r, sia, x, xl, y0, s, abs_s, refs, np.diff(sia), n)
        finally:
            A.destroy()


# ------------------------------------------------------------------------------------------- device-built operators --
def _adopt(torch, nrows, ncols, ia, ja, val, f):
    # the operator runs on a stream of its own: callers synchronise the device between torch's writes and its launches
    o = _opts(f)
    h = C.c_void_p()
    _lib.check(_lib.lib().qbh_csr_create_device(C.byref(h), nrows, ncols, 0, int(ja.numel()), ia.data_ptr(), ja.data_ptr(),
                                                val.data_ptr(), 0, C.byref(o)), "qbh_csr_create_device")
    return q.csr_mat(0, None, None, None, opts=o, _handle=h)


def _formula_operator(torch, n, rowlen, dev, periodic, chunk=1 << 25):
    """Full-storage CSR of n rows of rowlen entries on the device: columns csrforms.formula_cols, values formula_vals(offset)."""
    nnz = n * rowlen
    ia = torch.arange(n + 1, dtype=torch.int64, device=dev) * rowlen
    ja = torch.empty(nnz, dtype=torch.int32, device=dev)
    val = torch.empty(2 * nnz, dtype=torch.float64, device=dev)
    rows_per = max(1, chunk // rowlen)
    k = torch.arange(rowlen, dtype=torch.int64, device=dev)
    for r0 in range(0, n, rows_per):
        r1 = min(n, r0 + rows_per)
        r = torch.arange(r0, r1, dtype=torch.int64, device=dev)[:, None]
        p = (r * rowlen + k[None, :]).reshape(-1)
        ja[r0 * rowlen:r1 * rowlen] = cf.formula_cols(r, k[None, :], n, 5 if periodic else 12345).reshape(-1).to(torch.int32)
        re, im = cf.formula_vals(p)
        v = val[2 * r0 * rowlen:2 * r1 * rowlen].view(-1, 2)
        v[:, 0] = re.to(torch.float64)
        v[:, 1] = im.to(torch.float64)
        del r, p, re, im
    return ia, ja, val


def _host_row_sums(rows, rowlen, n, xfun, periodic):
    """Exact row sums (complex128 of exact integers) and sum |a||x| of the formula operator for the given rows."""
    r = rows.astype(np.int64)[:, None]
    k = np.arange(rowlen, dtype=np.int64)[None, :]
    c = cf.formula_cols(r, k, n, 5 if periodic else 12345)
    vr, vi = cf.formula_vals(r * rowlen + k)
    xr, xi = xfun(c)
    sr = (vr * xr - vi * xi).sum(axis=1)
    si = (vr * xi + vi * xr).sum(axis=1)
    mag = (np.sqrt((vr * vr + vi * vi).astype(L)) * np.sqrt((xr * xr + xi * xi).astype(L))).sum(axis=1)
    return (sr.astype(L) + 1j * si.astype(L)).astype(cf.CL), mag


def _xvec(xfun, j):
    xr, xi = xfun(j)
    return xr.astype(np.float64) + 1j * xi.astype(np.float64)


MULTI_N, MULTI_LEN = 8_000_000, 8              # 6.4e7 nonzeros
MULTI_FORMS = ([dict(spmv_kernel=cf.KERNEL_WAVE, value_dict=0, wave_walk=w) for w in (0, 1, 2, 3)]
               + [dict(spmv_kernel=cf.KERNEL_WAVE, value_dict=0, xcd_swizzle=3, deterministic=1)]
               + [dict(spmv_kernel=cf.KERNEL_ROWS, value_dict=vd, nnz_per_block=1024, xcd_swizzle=s) for vd in (0, 1) for s in (0, 1, 2)]
               + [dict(spmv_kernel=cf.KERNEL_STREAM, value_dict=vd, xcd_swizzle=s) for vd in (0, 1) for s in (0, 1, 2, 3)]
               + [dict(spmv_kernel=cf.KERNEL_VECTOR, value_dict=vd, xcd_swizzle=s) for vd in (0, 1) for s in (0, 1, 2)])


def test_multi_trip_walks():
    """6.4e7 nonzeros: every persistent workgroup (wave: wavefront) walks >= 4 blocks under any grid the caps allow, the dynamic walk
    hands over >= 2 chunks per wavefront of every XCD region; every walk and swizzle, coded and uncoded, row by row."""
    torch = pytest.importorskip("torch")
    dev = torch.device("cuda", 0)
    n, ln = MULTI_N, MULTI_LEN
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    ia, ja, val = _formula_operator(torch, n, ln, dev, periodic=False)
    torch.cuda.synchronize()
    s = np.empty(n, dtype=cf.CL)
    abs_s = np.empty(n, dtype=L)
    for r0 in range(0, n, 1 << 20):
        rows = np.arange(r0, min(n, r0 + (1 << 20)))
        s[rows], abs_s[rows] = _host_row_sums(rows, ln, n, cf.formula_x, False)
    x = _xvec(cf.formula_x, np.arange(n))
    y0 = cf.probe_vector(n, 5)
    nnz_row = np.full(n, ln)
    triples = [(1.0, 0.0, 0.0), (0.7, -1.3, 0.5)]
    refs = [cf.epilogue(s, abs_s, nnz_row, x, y0, *t) for t in triples]
    ia_h = np.arange(n + 1, dtype=np.int64) * ln
    vals_h = np.array([complex(*cf.formula_vals(t)) for t in range(251)])      # the 251 distinct values, for the mirror
    seen_multi = set()
    for f in MULTI_FORMS:
        r = cf.route(f["spmv_kernel"], f["value_dict"], ia_h, vals_h, npb_opt=f.get("nnz_per_block", 0),
                     xcd_swizzle=f.get("xcd_swizzle", 2), wave_walk=f.get("wave_walk", -1), deterministic=f.get("deterministic", 0),
                     ncu=ncu, nd=251)
        what = "multi-trip %s -> %s walk %d" % (f, r["key"], r["walk"])
        mw = cf.min_walk(r)
        if r["walk"] == 3:
            assert mw >= 2, "%s: %.2f chunks per wavefront" % (what, mw)
        elif f["value_dict"] == 0 or r["kernel"] != "rows":
            assert mw >= 4, "%s: a workgroup may walk only %d blocks" % (what, mw)
        seen_multi.add((r["kernel"], r["walk"]))
        A = _adopt(torch, n, n, ia, ja, val, f)
        try:
            _assert_route(what, A.info(), r)
            run = _Run(A, x, n)
            try:
                prev = None
                for t, (alpha, beta, gamma) in enumerate(triples):
                    yin = np.full(n, np.nan + 1j * np.nan) if beta == 0.0 else y0
                    y, (dot, nrm) = run(yin, alpha, beta, gamma, True)
                    tag = "%s (alpha, beta, gamma) = %r" % (what, triples[t])
                    _check_rows(tag, y, refs[t], ia_h)
                    _check_red(tag, dot, nrm, refs[t])
                    prev = (y, dot, nrm)
                for _ in range(2):
                    y2, (dot2, nrm2) = run(y0, *triples[1], True)
                    assert np.array_equal(y2.view(np.float64), prev[0].view(np.float64)), "%s: y differs between calls" % what
                    if r["walk"] != 3:
                        assert (dot2, nrm2) == prev[1:], "%s: reductions differ between calls" % what
                    else:
                        _check_red(what, dot2, nrm2, refs[1])
            finally:
                run.free()
            if f.get("deterministic"):
                B = _adopt(torch, n, n, ia, ja, val, f)
                try:
                    ra, rb = _Run(A, x, n), _Run(B, x, n)
                    ya, red_a = ra(y0, *triples[1], True)
                    yb, red_b = rb(y0, *triples[1], True)
                    ra.free(), rb.free()
                    assert np.array_equal(ya.view(np.float64), yb.view(np.float64)) and red_a == red_b, what
                finally:
                    B.destroy()
        finally:
            A.destroy()
    assert {("wave", w) for w in (0, 1, 2, 3)} <= seen_multi
    del ia, ja, val
    torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------------------- above 2^32 --
BIG_LEN = 63                                     # 2^31 and 2^32 fall inside rows (2^31 = 2 mod 63)
BIG_N = 7 * -(-4_400_000_000 // (BIG_LEN * 7))   # a multiple of 7: column residues mod 7 depend on the row alone
BIG_PERIOD = 7 * 97 * 251                        # row sums depend on r mod 7 (columns), r mod 97 (stride), r mod 251 (values)
BIG_FORMS = [dict(spmv_kernel=cf.KERNEL_WAVE, value_dict=0), dict(spmv_kernel=cf.KERNEL_WAVE, value_dict=0, wave_walk=3),
             dict(spmv_kernel=cf.KERNEL_ROWS, value_dict=0), dict(spmv_kernel=cf.KERNEL_STREAM, value_dict=0),
             dict(spmv_kernel=cf.KERNEL_VECTOR, value_dict=0), dict(spmv_kernel=cf.KERNEL_WAVE, value_dict=1)]


def test_above_2_32_nonzeros():
    """An uncoded, unsplit operator of 4.4e9 nonzeros (complex128) adopted from device arrays: rows around the nonzero offsets
    2^31 - 1, 2^31, 2^32 - 1, 2^32, the last rows and 2000 random rows against the closed formula; the reductions against a
    long-double sum over the whole vector (the row sums are periodic in the row, so one period of them gives the sum)."""
    torch = pytest.importorskip("torch")
    n, ln = BIG_N, BIG_LEN
    nnz = n * ln
    need = nnz * 20 + nnz + n * 8 * 6 + (6 << 30)     # ja + values, 1-byte codes, ia + x + y + y0, generation chunks and slack
    free, _ = torch.cuda.mem_get_info(0)
    if free < need:
        pytest.skip("needs %.1f GB of free HBM, %.1f GB free" % (need / 1e9, free / 1e9))
    dev = torch.device("cuda", 0)
    t0 = time.time()
    torch.cuda.reset_peak_memory_stats(0)
    ia, ja, val = _formula_operator(torch, n, ln, dev, periodic=True, chunk=1 << 27)
    j = torch.arange(n, dtype=torch.int64, device=dev)
    xr, xi = cf.periodic_x(j)
    xd = torch.complex(xr.to(torch.float64), xi.to(torch.float64))
    y0d = xd * (2.0 - 1.0j)
    del j, xr, xi
    yd = torch.empty_like(xd)
    torch.cuda.synchronize()
    # reference: one period of rows
    per = np.arange(BIG_PERIOD, dtype=np.int64)
    T, absT = _host_row_sums(per, ln, n, cf.periodic_x, True)
    xp = _xvec(cf.periodic_x, per)
    weights = np.full(BIG_PERIOD, n // BIG_PERIOD, dtype=np.int64) + (per < n % BIG_PERIOD)
    triples = [(1.0, 0.0, 0.0), (0.75, -1.25, 0.5)]
    refs = [cf.epilogue(T, absT, np.full(BIG_PERIOD, ln), xp, xp * (2 - 1j), a, b, g, weights=weights) for a, b, g in triples]
    rng = np.random.default_rng(2024)
    check = set()
    for off in (2 ** 31 - 1, 2 ** 31, 2 ** 32 - 1, 2 ** 32):
        check |= {off // ln - 1, off // ln, off // ln + 1}
    check |= set(range(n - 64, n)) | set(rng.integers(0, n, 2000).tolist())
    rows = np.array(sorted(check), dtype=np.int64)
    rows_d = torch.from_numpy(rows).to(dev)
    ph = rows % BIG_PERIOD
    ia_rows = np.arange(len(rows) + 1, dtype=np.int64) * ln       # row lengths for the messages
    times = {}
    for f in BIG_FORMS:
        A = _adopt(torch, n, n, ia, ja, val, f)
        try:
            info = A.info()
            want_kernel = cf.KERNEL_ROWS if f["value_dict"] else f["spmv_kernel"]
            assert info.kernel == want_kernel and (info.value_dict == 251) == bool(f["value_dict"]), (f, info.kernel, info.value_dict)
            for t, (alpha, beta, gamma) in enumerate(triples):
                if beta != 0.0:
                    yd.copy_(y0d)
                else:
                    yd.fill_(float("nan"))
                torch.cuda.synchronize()
                t1 = time.time()
                dot, nrm = A.spmv(C.c_void_p(xd.data_ptr()), C.c_void_p(yd.data_ptr()), alpha, beta, gamma, want_red=True)
                torch.cuda.synchronize()
                times[str(f)] = time.time() - t1
                got = yd.index_select(0, rows_d).cpu().numpy()
                ref = refs[t]
                sub = dict(y=ref["y"][ph], bound=ref["bound"][ph])
                tag = "2^32 %s (alpha, beta, gamma) = %r" % (f, triples[t])
                i, ratio, over, err = cf.worst(got, sub)
                assert ratio <= 1.0, "%s: row %d: |y - ref| = %.3e, bound %.3e, error / bound %.3g; %d rows over" % (
                    tag, int(rows[i]), err, float(sub["bound"][i]), ratio, over)
                _check_red(tag, dot, nrm, ref)
        finally:
            A.destroy()
    peak = torch.cuda.max_memory_allocated(0)
    print("2^32 case: %d nonzeros, %.1f s, torch peak %.1f GB, SpMV wall s %s" % (nnz, time.time() - t0, peak / 1e9, times))
    del ia, ja, val, xd, y0d, yd
    torch.cuda.empty_cache()
