"""Every vector kernel of the solvers, launched directly (tests/cxx/vecops_main.cpp calls the qbh::launch_* functions) and
compared element by element with a longdouble reference (tests/vecops.py: the references and how each tolerance follows from
the kernel's arithmetic).  One driver process per test; guard zones around every written buffer, const inputs compared after
the launch, every partial-sum buffer pre-filled with a NaN sentinel and reduced over the number of partials the callers use.

kernel                         case
-----------------------------  ----------------------------------------------------------------
k_reduce_partials              test_reduce_partials (and the second stage of every reduction below)
k_lanczos_tail                 test_lanczos_tail
k_dotc, k_nrm2sq<d2>,          test_complex_reductions
  k_imag_norm
k_scal<d2>, k_scal_to,         test_complex_elementwise
  k_xpby, k_fill_const,
  k_pack_real, k_unpack_real
k_axpy_norm                    test_axpy_norm, test_real_part_flags
k_cg_update                    test_cg_update
k_dot_re, k_nrm2sq<double>,    test_packed_real
  k_scal<double>, k_xpby_re,
  k_axpy_norm_re,
  k_cg_update_re
k_basis_scatter,               test_basis_maps
  k_basis_gather,
  k_basis_scatter_re
k_multi_dot<8>                 test_multi_dot
k_multi_axpy                   test_multi_axpy
k_basis_rotate<32>, <64>       test_basis_rotate, test_basis_rotate_second_trip
k_kron_tile8,                  test_tiles_band8 (k_axpy_norm_tile8<0> / <1> as well), test_tile_launchers_reject_a_minor_size_below_8
  k_kron_tile_edge
k_kron_tile_re,                test_packed_real_tiles
  k_axpy_norm_re (yt, 32-bit
  and generic index path)
k_randomize                    test_randomize
"""
import functools
import tempfile

import numpy as np
import pytest

import vecops as vo
from vecops import Batch, cin, io, out

pytestmark = pytest.mark.gpu

SIZES = [1, 63, 64, 255, 256, 257, 4900, 524288, 524289, 1310731]
F8, C16, I4 = np.float64, np.complex128, np.int32
WORST = {}


def note(family, ratio):
    """keep the largest error of a family as a fraction of its bound (printed; shown with pytest -s)"""
    WORST[family] = max(WORST.get(family, 0.0), float(ratio))
    return ratio


def report(*families):
    for f in families:
        print("vecops worst error / bound  %-28s %.4f" % (f, WORST.get(f, 0.0)))


def run(batch, timeout=120, expect_rc=0):
    """every launcher returns expect_rc, no guard word and no const input changed"""
    with tempfile.TemporaryDirectory() as tmp:
        res = batch.run(vo.driver(), tmp, timeout=timeout)
    for k, r in enumerate(res):
        assert (r.rc, r.guard, r.const) == (expect_rc, 0, 0), (k, batch.cases[k][0], batch.cases[k][2], r.rc, r.guard, r.const)
    return res


@functools.lru_cache(maxsize=None)
def data(n):
    g = vo.rng(1000 + n % 9973)
    return {k: vo.cvec(g, n) for k in ("x", "y", "p", "pp")}


@functools.lru_cache(maxsize=None)
def rdata(n):
    g = vo.rng(2000 + n % 9973)
    return {k: vo.rvec(g, n) for k in ("x", "y", "p", "pp")}


def red_bufs(n, ncomp=1):
    """partials (sentinel) and the reduced result; post entry for buffers at (ip, ir)"""
    return out(F8, vo.blas_grid(n) * ncomp), out(F8, ncomp)


def check_red(fam, got, ref, n, sumabs, L=None, gridn=None):
    nparts = vo.blas_grid(n if gridn is None else gridn)
    r = note(fam, vo.reduction_ratio(got, ref, n, nparts, sumabs, L))
    assert r <= 1.0, (fam, n, got, float(ref), r)


def check_el(fam, got, ref, k, sumabs, what=None):
    r = note(fam, vo.elementwise_ratio(got, ref, k, sumabs))
    assert r <= 1.0, (fam, what, r)


# ---------------------------------------------------------------------------------------------- complex streaming kernels
def test_complex_reductions():
    b, idx = Batch(), {}
    for n in SIZES:
        d = data(n)
        P, R = red_bufs(n, 2)
        idx["dotc", n] = b.add("dotc", [cin(d["x"]), cin(d["y"]), P, R], [n, 0, 1, 2], post=[(2, n, 2, 3)])
        for op in ("nrm2sq", "imag_norm"):
            P, R = red_bufs(n)
            idx[op, n] = b.add(op, [cin(d["x"]), P, R], [n, 0, 1], post=[(1, n, 1, 2)])
    res = run(b)
    for n in SIZES:
        d = data(n)
        (re, im), (sre, sim) = vo.ref_dotc(d["x"], d["y"])
        got = res[idx["dotc", n]].out[3]
        check_red("dotc", got[0], re, n, sre)
        check_red("dotc", got[1], im, n, sim)
        ref = vo.ref_nrm2sq(d["x"])
        check_red("nrm2sq", res[idx["nrm2sq", n]].out[2][0], ref, n, float(ref))
        xi = d["x"].imag.astype(vo.LD)
        ref = np.sum(xi * xi)
        check_red("imag_norm", res[idx["imag_norm", n]].out[2][0], ref, n, float(ref))
    report("dotc", "nrm2sq", "imag_norm")


def test_complex_elementwise():
    b, idx = Batch(), {}
    a, bb, fill = -0.8125 + 2.0 ** -30, 1.37109375 + 2.0 ** -29, 0.577215664901532
    for n in SIZES:
        d = data(n)
        re = np.ascontiguousarray(d["y"].real)
        idx["scal", n] = b.add("scal", [io(d["x"])], [n, 0], [a])
        idx["scal_to", n] = b.add("scal_to", [cin(d["x"]), out(C16, n)], [n, 0, 1], [a])
        idx["xpby", n] = b.add("xpby", [cin(d["x"]), io(d["y"]), io(np.zeros(1, I4))], [n, 0, 1, -1, 2], [bb])
        idx["xpby_yr", n] = b.add("xpby", [cin(d["x"]), io(d["y"]), out(F8, n), io(np.zeros(1, I4))], [n, 0, 1, 2, 3], [bb])
        idx["fill", n] = b.add("fill_const", [out(C16, n)], [n, 0], [fill])
        idx["pack", n] = b.add("pack_real", [cin(d["x"]), out(F8, n), io(np.zeros(1, I4))], [n, 0, 1, 2])
        idx["unpack", n] = b.add("unpack_real", [cin(re), out(C16, n)], [n, 0, 1])
    res = run(b)
    for n in SIZES:
        d = data(n)
        ref, sa = vo.CLD(a) * d["x"].astype(vo.CLD), abs(a) * vo.cabs(d["x"])
        check_el("scal", res[idx["scal", n]].out[0], ref, 1, sa, n)
        check_el("scal", res[idx["scal_to", n]].out[1], ref, 1, sa, n)
        ref, sa = d["x"].astype(vo.CLD) + vo.CLD(bb) * d["y"].astype(vo.CLD), vo.cabs(d["x"]) + abs(bb) * vo.cabs(d["y"])
        r = res[idx["xpby", n]]
        check_el("xpby", r.out[1], ref, 2, sa, n)
        assert r.out[2][0] == 0                               # no yr: the flag is not touched
        r2 = res[idx["xpby_yr", n]]
        assert vo.exact(r2.out[1], r.out[1]) and vo.exact(r2.out[2], np.ascontiguousarray(r2.out[1].real)) and r2.out[3][0] == 1
        assert vo.exact(res[idx["fill", n]].out[0], np.full(n, complex(fill, 0.0), dtype=C16))
        r = res[idx["pack", n]]
        assert vo.exact(r.out[1], np.ascontiguousarray(d["x"].real)) and r.out[2][0] == 1
        want = np.zeros(n, dtype=C16)
        want.real = d["y"].real
        assert vo.exact(res[idx["unpack", n]].out[1], want)
    report("scal", "xpby")


AXPY_VARIANTS = ("plain", "alpha_dev", "alpha_scale_dev", "yr")


def _axpy_alpha(variant):
    """(alpha passed by value, alpha_dev, scale_dev, the coefficient the kernel then forms in double)"""
    alpha = complex(0.7109375 + 2.0 ** -31, -0.4140625)
    adev, sdev = np.float64(-1.3203125 + 2.0 ** -33), np.float64(0.8828125 + 2.0 ** -35)
    if variant == "alpha_dev":
        return alpha, adev, None, complex(np.float64(alpha.real) * adev, 0.0)
    if variant == "alpha_scale_dev":                          # alpha.x is replaced by scale_dev[0], alpha.y ignored
        return alpha, adev, sdev, complex(sdev * adev, 0.0)
    return alpha, None, None, alpha


def test_axpy_norm():
    b, idx = Batch(), {}
    for n in SIZES:
        d = data(n)
        for v in AXPY_VARIANTS:
            alpha, adev, sdev, _ = _axpy_alpha(v)
            P, R = red_bufs(n)
            bufs = [cin(d["x"]), io(d["y"]), P, R, io(np.zeros(1, I4))]
            ia = isd = iyr = -1
            if adev is not None:
                bufs.append(cin(np.array([adev, 7.0])))
                ia = len(bufs) - 1
            if sdev is not None:
                bufs.append(cin(np.array([sdev, 9.0])))
                isd = len(bufs) - 1
            if v == "yr":
                bufs.append(out(F8, n))
                iyr = len(bufs) - 1
            idx[v, n] = (b.add("axpy_norm", bufs, [n, ia, 0, 1, 2, iyr, 4, isd], [alpha.real, alpha.imag], post=[(2, n, 1, 3)]), iyr)
    res = run(b)
    for n in SIZES:
        d = data(n)
        for v in AXPY_VARIANTS:
            coef = _axpy_alpha(v)[3]
            ref, sa = vo.ref_axpy(coef, d["x"], d["y"])
            k, iyr = idx[v, n]
            r = res[k]
            check_el("axpy_norm", r.out[1], ref, 4, sa, (v, n))
            check_red("axpy_norm |y|^2", r.out[3][0], vo.ref_nrm2sq(ref), n, vo.norm_terms(sa))
            if v == "yr":
                assert vo.exact(r.out[iyr], np.ascontiguousarray(r.out[1].real)) and r.out[4][0] == 1
            else:
                assert r.out[4][0] == 0
    report("axpy_norm", "axpy_norm |y|^2")


def test_cg_update():
    b, idx = Batch(), {}
    alpha, accu2, delta = complex(0.3984375 + 2.0 ** -32, 0.2421875), 1.6171875 + 2.0 ** -30, complex(1.2265625 + 2.0 ** -31, -0.6953125)
    for n in SIZES:
        d = data(n)
        for v in ("plain", "delta_dev"):
            P, R = red_bufs(n)
            bufs = [cin(d["p"]), cin(d["pp"]), io(d["x"]), io(d["y"]), P, R]
            idl = -1
            if v == "delta_dev":
                bufs.append(cin(np.array([delta.real, delta.imag])))
                idl = 6
            idx[v, n] = b.add("cg_update", bufs, [n, 0, 1, 2, 3, 4, idl], [alpha.real, alpha.imag, accu2], post=[(4, n, 1, 5)])
    res = run(b)
    for n in SIZES:
        d = data(n)
        for v in ("plain", "delta_dev"):
            a = alpha if v == "plain" else vo.cg_alpha_from_delta(accu2, delta)
            r = res[idx[v, n]]
            ref, sa = vo.ref_axpy(a, d["p"], d["x"])
            check_el("cg_update", r.out[2], ref, 4, sa, (v, n, "v"))
            ref, sa = vo.ref_axpy(-a, d["pp"], d["y"])
            check_el("cg_update", r.out[3], ref, 4, sa, (v, n, "r"))
            check_red("cg_update |r|^2", r.out[5][0], vo.ref_nrm2sq(ref), n, vo.norm_terms(sa))
    report("cg_update", "cg_update |r|^2")


def test_real_part_flags():
    """the flag of axpy_norm(yr), xpby(yr) and pack_real: 0 while every imaginary part is +-0, 1 for one that is not"""
    b, cases = Batch(), []
    for n in (257, 524289):
        g = vo.rng(77 + n)
        x, y = vo.rvec(g, n).astype(C16), vo.rvec(g, n).astype(C16)
        y.imag = np.where(g.uniform(size=n) < 0.5, -0.0, 0.0)
        x.imag = np.where(g.uniform(size=n) < 0.5, -0.0, 0.0)
        for at in (None, 0, n // 2, n - 1):
            yy = y.copy()
            if at is not None:
                yy[at] = complex(yy[at].real, 2.0 ** -1060)          # a subnormal imaginary part is not zero
            want = int(at is not None)
            P, R = red_bufs(n)
            k = b.add("axpy_norm", [cin(x), io(yy), P, R, io(np.zeros(1, I4)), out(F8, n)], [n, -1, 0, 1, 2, 5, 4, -1], [0.75, 0.0], post=[(2, n, 1, 3)])
            cases.append((k, 4, want))
            k = b.add("xpby", [cin(x), io(yy), out(F8, n), io(np.zeros(1, I4))], [n, 0, 1, 2, 3], [1.0])
            cases.append((k, 3, want))
            k = b.add("pack_real", [cin(yy), out(F8, n), io(np.zeros(1, I4))], [n, 0, 1, 2])
            cases.append((k, 2, want))
    res = run(b)
    for k, iflag, want in cases:
        assert res[k].out[iflag][0] == want, (b.cases[k][0], b.cases[k][2], want)


# ---------------------------------------------------------------------------------------------- packed-real streaming kernels
def test_packed_real():
    b, idx = Batch(), {}
    a, bb, adev = -0.6640625 + 2.0 ** -31, 1.1328125 + 2.0 ** -30, np.float64(1.4453125 + 2.0 ** -34)
    for n in SIZES:
        d = rdata(n)
        P, R = red_bufs(n)
        idx["dot", n] = b.add("dot_re", [cin(d["x"]), cin(d["y"]), P, R], [n, 0, 1, 2], post=[(2, n, 1, 3)])
        P, R = red_bufs(n)
        idx["nrm", n] = b.add("nrm2sq_re", [cin(d["x"]), P, R], [n, 0, 1], post=[(1, n, 1, 2)])
        idx["scal", n] = b.add("scal_re", [io(d["x"])], [n, 0], [a])
        idx["xpby", n] = b.add("xpby_re", [cin(d["x"]), io(d["y"])], [n, 0, 1], [bb])
        for v in ("plain", "alpha_dev"):
            P, R = red_bufs(n)
            bufs = [cin(d["x"]), io(d["y"]), P, R] + ([cin(np.array([adev, 3.0]))] if v == "alpha_dev" else [])
            idx["axpy", v, n] = b.add("axpy_norm_re", bufs, [n, 4 if v == "alpha_dev" else -1, 0, 1, 2, -1, 1, 1, 1], [a], post=[(2, n, 1, 3)])
        P, R = red_bufs(n)
        idx["cg", n] = b.add("cg_update_re", [cin(d["p"]), cin(d["pp"]), io(d["x"]), io(d["y"]), P, R], [n, 0, 1, 2, 3, 4], [a], post=[(4, n, 1, 5)])
    res = run(b)
    for n in SIZES:
        d = rdata(n)
        x, y = d["x"].astype(vo.LD), d["y"].astype(vo.LD)
        check_red("dot_re", res[idx["dot", n]].out[3][0], np.sum(x * y), n, float(np.sum(np.abs(x * y))))
        check_red("nrm2sq_re", res[idx["nrm", n]].out[2][0], np.sum(x * x), n, float(np.sum(x * x)))
        check_el("scal_re", res[idx["scal", n]].out[0], vo.LD(a) * x, 1, abs(a) * np.abs(x), n)
        check_el("xpby_re", res[idx["xpby", n]].out[1], x + vo.LD(bb) * y, 2, np.abs(x) + abs(bb) * np.abs(y), n)
        for v in ("plain", "alpha_dev"):
            coef = a if v == "plain" else float(np.float64(a) * adev)
            ref, sa = vo.ref_axpy_re(coef, d["x"], d["y"])
            r = res[idx["axpy", v, n]]
            check_el("axpy_norm_re", r.out[1], ref, 2, sa, (v, n))
            check_red("axpy_norm_re |y|^2", r.out[3][0], np.sum(ref * ref), n, vo.norm_terms(sa))
        r = res[idx["cg", n]]
        ref, sa = vo.ref_axpy_re(a, d["p"], d["x"])
        check_el("cg_update_re", r.out[2], ref, 2, sa, (n, "v"))
        ref, sa = vo.ref_axpy_re(-a, d["pp"], d["y"])
        check_el("cg_update_re", r.out[3], ref, 2, sa, (n, "r"))
        check_red("cg_update_re |r|^2", r.out[5][0], np.sum(ref * ref), n, vo.norm_terms(sa))
    report("dot_re", "nrm2sq_re", "scal_re", "xpby_re", "axpy_norm_re", "axpy_norm_re |y|^2", "cg_update_re", "cg_update_re |r|^2")


def test_basis_maps():
    """scatter / gather through a random permutation, a third of the entries with the sign bit: exact"""
    b, idx, maps = Batch(), {}, {}
    for n in SIZES:
        g = vo.rng(31 + n)
        perm = g.permutation(n).astype(np.uint32)
        neg = g.uniform(size=n) < 1.0 / 3.0
        maps[n] = (perm.astype(np.int64), neg)
        m = cin(perm | (neg.astype(np.uint32) << np.uint32(31)))
        d, rd = data(n), rdata(n)
        idx["scatter", n] = b.add("basis_scatter", [m, cin(d["x"]), out(C16, n)], [n, 0, 1, 2])
        idx["gather", n] = b.add("basis_gather", [m, cin(d["x"]), out(C16, n)], [n, 0, 1, 2])
        idx["scatter_re", n] = b.add("basis_scatter_re", [m, cin(rd["x"]), out(F8, n)], [n, 0, 1, 2])
    res = run(b)
    for n in SIZES:
        perm, neg = maps[n]
        x, xr = data(n)["x"], rdata(n)["x"]
        want = np.empty(n, dtype=C16)
        want[perm] = np.where(neg, -x, x)
        assert vo.exact(res[idx["scatter", n]].out[2], want), n
        assert vo.exact(res[idx["gather", n]].out[2], np.where(neg, -x[perm], x[perm])), n
        want = np.empty(n, dtype=F8)
        want[perm] = np.where(neg, -xr, xr)
        assert vo.exact(res[idx["scatter_re", n]].out[2], want), n


# ---------------------------------------------------------------------------------------------- second stage, Lanczos tail
def test_reduce_partials():
    b, idx = Batch(), {}
    g = vo.rng(5)
    for ncomp in (1, 2, 3, 16):
        for nparts in (1, 63, 1024, 1025, 2048):
            p = vo.rvec(g, nparts * ncomp)
            idx[ncomp, nparts] = (b.add("reduce_partials", [cin(p), out(F8, ncomp)], [nparts, 0, ncomp, 1]), p)
    res = run(b)
    for (ncomp, nparts), (k, p) in idx.items():
        pl = p.astype(vo.LD).reshape(nparts, ncomp)
        for c in range(ncomp):
            r = note("reduce_partials", vo.reduction_ratio(res[k].out[1][c], np.sum(pl[:, c]), nparts, nparts, float(np.sum(np.abs(pl[:, c]))), L=0))
            assert r <= 1.0, (ncomp, nparts, c, r)
    report("reduce_partials")


def test_lanczos_tail():
    """all eight outputs against the formulas of the source; |w'|^2 bit-equal to launch_reduce_partials on the same partials.
    The derived scalars are compared with the formulas evaluated in longdouble from the device's own |w'|^2."""
    b, idx = Batch(), {}
    g = vo.rng(6)
    sc_host, state0, dot, sq_ready = 0.8359375 + 2.0 ** -33, np.array([9.0, 8.0, 7.0, 1.2890625 + 2.0 ** -31]), np.array([-0.9140625 + 2.0 ** -32, 5.0]), 3.3203125 + 2.0 ** -30
    for nparts in (1, 1025, 2048):
        p = np.abs(vo.rvec(g, nparts))
        for use_host in (0, 1):
            for ready in (False, True):
                bufs = [cin(p), cin(dot), io(state0), out(F8, 4, host=True), out(F8, 1)] + ([cin(np.array([sq_ready, 2.0]))] if ready else [])
                idx[nparts, use_host, ready] = (b.add("lanczos_tail", bufs, [nparts, 0, 1, 2, 3, use_host, 5 if ready else -1], [sc_host],
                                                      post=[(0, nparts * 256, 1, 4)]), p)
    res = run(b)
    for (nparts, use_host, ready), (k, p) in idx.items():
        state, log, red = res[k].out[2], res[k].out[3], res[k].out[4][0]
        sq = log[1]
        if ready:
            assert vo.exact(np.array([sq]), np.array([sq_ready]))
        else:
            assert vo.exact(np.array([sq]), np.array([red])), (nparts, sq, red)               # the same summation order
            pl = p.astype(vo.LD)
            r = note("lanczos_tail |w'|^2", vo.reduction_ratio(sq, np.sum(pl), nparts, nparts, float(np.sum(pl)), L=0))
            assert r <= 1.0
        sc_x = vo.LD(sc_host if use_host else state0[3])
        d, bref = vo.LD(dot[0]), np.sqrt(vo.LD(sq))
        # bounds in units of u: a product rounds once (u), sqrt and the division are within one ulp (2 u), and the error of
        # sc_new = 1 / sqrt(sq) (4 u) enters sc_new^2 twice
        want = {"state0": (1 / bref, 4), "state1": (-bref * sc_x, 3), "state2": (-1 / (bref * bref), 9), "state3": (1 / bref, 4),
                "log0": (d, 0), "log2": (sc_x * d, 1), "log3": (bref, 2)}
        gotv = {"state0": state[0], "state1": state[1], "state2": state[2], "state3": state[3], "log0": log[0], "log2": log[2], "log3": log[3]}
        for name, (ref, nu) in want.items():
            err = abs(vo.LD(gotv[name]) - ref)
            if nu == 0:
                assert err == 0, name
            else:
                r = note("lanczos_tail scalars", float(err / (nu * vo.U * abs(ref))))
                assert r <= 1.0, (name, nparts, use_host, ready, r)
    report("lanczos_tail |w'|^2", "lanczos_tail scalars")


# ---------------------------------------------------------------------------------------------- Krylov basis
MD_SIZES = (1, 257, 4900, 524289)            # 524289: the first size at which a thread takes a second trip
MD_COEF = vo.cvec(vo.rng(8), 8)


@functools.lru_cache(maxsize=None)
def krylov_inputs(n, pad):
    """eight basis vectors with leading dimension n + pad (the padding holds data as well) and w"""
    g = vo.rng(8000 + 10 * pad + n % 9973)
    Vf, w = vo.cvec(g, 7 * (n + pad) + n), vo.cvec(g, n)
    return Vf, np.stack([Vf[i * (n + pad):i * (n + pad) + n] for i in range(8)]), w


@pytest.mark.parametrize("pad", [0, 3])
def test_multi_dot(pad):
    b, idx = Batch(), {}
    for n in MD_SIZES:
        Vf, _, w = krylov_inputs(n, pad)
        for nv in range(1, 9):
            P, R = red_bufs(n, 16)
            idx[n, nv] = b.add("multi_dot8", [cin(Vf), cin(w), P, R], [n, 0, n + pad, 1, nv, 2], post=[(2, n, 16, 3)])
    res = run(b)
    for n in MD_SIZES:
        _, V, w = krylov_inputs(n, pad)
        dots = vo.ref_multi_dot(V, w)
        for nv in range(1, 9):
            got = res[idx[n, nv]].out[3]
            for i in range(nv):
                (re, im), (sre, sim) = dots[i]
                check_red("multi_dot8", got[2 * i], re, n, sre)
                check_red("multi_dot8", got[2 * i + 1], im, n, sim)
            assert np.all(got[2 * nv:] == 0.0) and got.size == 16, (n, pad, nv, got)
    report("multi_dot8")


@pytest.mark.parametrize("pad", [0, 3])
def test_multi_axpy(pad):
    b, idx = Batch(), {}
    cd = np.ascontiguousarray(MD_COEF).view(F8)
    for n in MD_SIZES:
        Vf, _, w = krylov_inputs(n, pad)
        for nv in range(1, 9):
            P, R = red_bufs(n)
            idx[n, nv] = b.add("multi_axpy8", [cin(Vf), io(w), P, R], [n, 0, n + pad, nv, 1, 2], cd, post=[(2, n, 1, 3)])
            idx[n, nv, "null"] = b.add("multi_axpy8", [cin(Vf), io(w), out(F8, vo.blas_grid(n))], [n, 0, n + pad, nv, 1, -1], cd)
    res = run(b)
    for n in MD_SIZES:
        _, V, w = krylov_inputs(n, pad)
        prefixes = vo.ref_multi_axpy(V, MD_COEF, w)
        for nv in range(1, 9):
            ref, sa = prefixes[nv - 1]
            r = res[idx[n, nv]]
            check_el("multi_axpy8", r.out[1], ref, 4 * nv, sa, (n, pad, nv))
            check_red("multi_axpy8 |w|^2", r.out[3][0], vo.ref_nrm2sq(ref), n, vo.norm_terms(sa))
            r0 = res[idx[n, nv, "null"]]
            assert vo.exact(r0.out[1], r.out[1]) and vo.is_sentinel(r0.out[2])        # a null partials pointer: nothing written
    report("multi_axpy8", "multi_axpy8 |w|^2")


ROT_M = (1, 2, 31, 32, 33, 64)
ROT_BIG = 262145                             # 2n doubles per vector: the first size with a second trip


@functools.lru_cache(maxsize=1)
def rotate_inputs(n, m):
    """V (m x n), S (m x m, column-major; a smaller keep takes its first columns) and the reference of keep = m with its
    sum|terms|, which serves every keep and both ldv; only the latest (n, m) is kept"""
    g = vo.rng(9000 + 100 * m + n % 9973)
    V, S = np.stack([vo.cvec(g, n) for _ in range(m)]), vo.rvec(g, m * m)
    return (V, S) + vo.ref_rotate(V, S, m)


def _rotate(sizes, ms, pads, timeout=120):
    """every keep of {1, m - 1, m} for each n, m and ldv = n + pad"""
    b, idx, inputs = Batch(), {}, {}
    g = vo.rng(9)
    for n in sizes:
        for m in ms:
            inputs[n, m] = V, S, _, _ = rotate_inputs(n, m)
            for pad in pads:
                Vf = np.empty(m * (n + pad), dtype=C16)
                Vf.reshape(m, n + pad)[:, :n] = V
                Vf.reshape(m, n + pad)[:, n:] = vo.cvec(g, m * pad).reshape(m, pad)          # the padding element holds data as well
                for keep in sorted({k for k in (1, m - 1, m) if k >= 1}):
                    idx[n, pad, m, keep] = (b.add("basis_rotate", [io(Vf), cin(S[:m * keep])], [n, 0, n + pad, m, keep, 1]), Vf)
    res = run(b, timeout)
    for (n, pad, m, keep), (k, Vf) in idx.items():
        _, _, ref, sa = inputs[n, m]
        got, was = res[k].out[0].reshape(m, n + pad), Vf.reshape(m, n + pad)
        fam = "basis_rotate<32>" if m <= 32 else "basis_rotate<64>"
        r = note(fam, vo.elementwise_ratio_rows(got[:keep, :n], ref[:keep], 2 * m, sa[:keep]))
        assert r <= 1.0, (n, pad, m, keep, r)
        assert vo.exact(got[keep:], was[keep:]) and vo.exact(got[:, n:], was[:, n:]), (n, pad, m, keep)     # columns >= keep, the padding
    report("basis_rotate<32>", "basis_rotate<64>")


def test_basis_rotate():
    _rotate((1, 129, 4900), ROT_M, (0, 1))


@pytest.mark.parametrize("m,pad", [(m, pad) for m in ROT_M for pad in (0, 1)])
def test_basis_rotate_second_trip(m, pad):
    """n = 262145 with every m, keep and ldv; one driver process per (m, ldv), the widest of which moves 3 x 268 MB"""
    _rotate((ROT_BIG,), (m,), (pad,), timeout=300)


# ---------------------------------------------------------------------------------------------- tiles
TILE8 = [(8, 1), (9, 1), (15, 7), (16, 8), (17, 9), (8, 64), (12, 100), (70, 70), (255, 33), (256, 8), (265, 17)]


def _tile_inputs(S, NU):
    g = vo.rng(100 * S + NU)
    n = S * NU
    return vo.cvec(g, n), vo.cvec(g, n), vo.rvec(g, n).astype(C16), vo.rvec(g, n).astype(C16)


def test_tiles_band8():
    b, idx = Batch(), {}
    alpha, bb = complex(0.7109375 + 2.0 ** -31, -0.4140625), 1.37109375 + 2.0 ** -29
    _, adev, sdev, _ = _axpy_alpha("alpha_scale_dev")
    for S, NU in TILE8:
        n, T = S * NU, [S, NU, 8]
        x, y, xre, yre = _tile_inputs(S, NU)
        flag = lambda: io(np.zeros(1, I4))
        idx["tile", S, NU] = b.add("kron_tile", [cin(x), out(C16, n)], [n, 0, 1] + T + [0, -1])
        idx["axpy", S, NU] = b.add("axpy_norm_tile", [cin(x), io(y), out(C16, n)] + list(red_bufs(n)), [n, -1, 0, 1, 2] + T + [3, -1, 0, -1],
                                   [alpha.real, alpha.imag], post=[(3, n, 1, 4)])
        idx["axpy_dev", S, NU] = b.add("axpy_norm_tile", [cin(x), io(y), out(C16, n)] + list(red_bufs(n)) + [cin(np.array([adev, 1.0])), cin(np.array([sdev, 1.0]))],
                                       [n, 5, 0, 1, 2] + T + [3, 6, 0, -1], [alpha.real, alpha.imag], post=[(3, n, 1, 4)])
        idx["xpby", S, NU] = b.add("xpby_tile", [cin(x), io(y), out(C16, n)], [n, 0, 1, 2] + T + [0, -1], [bb])
        for at in (None, 0, n // 2, n - 1):                  # real wire: the tiled copy as packed real parts + the flag
            xx, yy = xre.copy(), yre.copy()
            if at is not None:
                xx[at] = complex(xx[at].real, 2.0 ** -1060)
                yy[at] = complex(yy[at].real, 2.0 ** -1060)
            idx["tile_re", S, NU, at] = (b.add("kron_tile", [cin(xx), out(F8, n), flag()], [n, 0, 1] + T + [1, 2]), xx)
            idx["axpy_re", S, NU, at] = b.add("axpy_norm_tile", [cin(xre), io(yy), out(F8, n)] + list(red_bufs(n)) + [flag()],
                                              [n, -1, 0, 1, 2] + T + [3, -1, 1, 5], [0.75, 0.0], post=[(3, n, 1, 4)])
            idx["xpby_re", S, NU, at] = b.add("xpby_tile", [cin(xre), io(yy), out(F8, n), flag()], [n, 0, 1, 2] + T + [1, 3], [1.0])
    res = run(b)
    for S, NU in TILE8:
        n = S * NU
        tm = vo.tile_map(S, NU, 8)
        x, y, xre, yre = _tile_inputs(S, NU)
        assert vo.tiled_exact(res[idx["tile", S, NU]].out[1], x, tm), (S, NU)
        # the chain of a thread: 8 elements per item, ceil(items / grid) items, and its share of the narrow band
        grid = vo.blas_grid(n)
        items = -(-NU // 8) * -(-(S // 8) // 32)
        L = 8 * -(-items // grid) + -(-(NU * (S % 8)) // (grid * 256))
        for name, coef in (("axpy", alpha), ("axpy_dev", complex(sdev * adev, 0.0))):
            r = res[idx[name, S, NU]]
            ref, sa = vo.ref_axpy(coef, x, y)
            check_el("axpy_norm_tile", r.out[1], ref, 4, sa, (name, S, NU))
            assert vo.tiled_exact(r.out[2], r.out[1], tm), (name, S, NU)
            check_red("axpy_norm_tile |y|^2", r.out[4][0], vo.ref_nrm2sq(ref), n, vo.norm_terms(sa), L=L)
        r = res[idx["xpby", S, NU]]
        ref, sa = x.astype(vo.CLD) + vo.CLD(bb) * y.astype(vo.CLD), vo.cabs(x) + abs(bb) * vo.cabs(y)
        check_el("xpby_tile", r.out[1], ref, 2, sa, (S, NU))
        assert vo.tiled_exact(r.out[2], r.out[1], tm), (S, NU)
        for at in (None, 0, n // 2, n - 1):
            want = int(at is not None)
            k, xx = idx["tile_re", S, NU, at]
            assert vo.tiled_exact(res[k].out[1], np.ascontiguousarray(xx.real), tm) and res[k].out[2][0] == want, (S, NU, at)
            r = res[idx["axpy_re", S, NU, at]]
            assert vo.tiled_exact(r.out[2], np.ascontiguousarray(r.out[1].real), tm) and r.out[5][0] == want, (S, NU, at)
            yy = yre.copy()
            if at is not None:
                yy[at] = complex(yy[at].real, 2.0 ** -1060)
            ref, sa = vo.ref_axpy(0.75, xre, yy)
            check_el("axpy_norm_tile", r.out[1], ref, 4, sa, ("axpy_re", S, NU, at))
            check_red("axpy_norm_tile |y|^2", r.out[4][0], vo.ref_nrm2sq(ref), n, vo.norm_terms(sa), L=L)
            r = res[idx["xpby_re", S, NU, at]]
            assert vo.tiled_exact(r.out[2], np.ascontiguousarray(r.out[1].real), tm) and r.out[3][0] == want, (S, NU, at)
    report("axpy_norm_tile", "axpy_norm_tile |y|^2", "xpby_tile")


def test_tile_launchers_reject_a_minor_size_below_8():
    """S = 7: QBH_EINVAL from both launchers and nothing launched -- y, the tiled copy and the partials keep their bits"""
    S, NU = 7, 5
    n = S * NU
    x, y, _, _ = _tile_inputs(S, NU)
    b = Batch()
    b.add("axpy_norm_tile", [cin(x), io(y), out(C16, n), out(F8, vo.blas_grid(n))], [n, -1, 0, 1, 2, S, NU, 8, 3, -1, 0, -1], [0.5, 0.25])
    b.add("xpby_tile", [cin(x), io(y), out(C16, n)], [n, 0, 1, 2, S, NU, 8, 0, -1], [0.5])
    res = run(b, expect_rc=vo.QBH_EINVAL)
    for r in res:
        assert vo.exact(r.out[1], y) and vo.is_sentinel(r.out[2])
    assert vo.is_sentinel(res[0].out[3])


def test_packed_real_tiles():
    """B = 16: the 32-bit index path of k_axpy_norm_re; B = 8: the generic tile() path; k_kron_tile_re for both"""
    b, idx = Batch(), {}
    a = -0.6640625 + 2.0 ** -31
    shapes = [(16, 1), (17, 5), (31, 5), (33, 70), (70, 70)]
    for S, NU in shapes:
        n = S * NU
        g = vo.rng(7 * S + NU)
        x, y = vo.rvec(g, n), vo.rvec(g, n)
        for B in (16, 8):
            idx["tile", S, NU, B] = b.add("kron_tile_re", [cin(x), out(F8, n)], [n, 0, 1, S, NU, B])
            P, R = red_bufs(n)
            idx["axpy", S, NU, B] = (b.add("axpy_norm_re", [cin(x), io(y), P, R, out(F8, n)], [n, -1, 0, 1, 2, 4, S, NU, B], [a], post=[(2, n, 1, 3)]), x, y)
    res = run(b)
    for S, NU in shapes:
        n = S * NU
        for B in (16, 8):
            tm = vo.tile_map(S, NU, B)
            k, x, y = idx["axpy", S, NU, B]
            assert vo.tiled_exact(res[idx["tile", S, NU, B]].out[1], x, tm), (S, NU, B)
            r = res[k]
            ref, sa = vo.ref_axpy_re(a, x, y)
            check_el("axpy_norm_re(yt)", r.out[1], ref, 2, sa, (S, NU, B))
            assert vo.tiled_exact(r.out[4], r.out[1], tm), (S, NU, B)
            check_red("axpy_norm_re(yt) |y|^2", r.out[3][0], np.sum(ref * ref), n, vo.norm_terms(sa))
    report("axpy_norm_re(yt)", "axpy_norm_re(yt) |y|^2")


# ---------------------------------------------------------------------------------------------- start vector
def test_randomize():
    """bit-equal to the Lehmer stream in Python integers, complex and packed-real form; |x|^2 by the reduction rule with a chain of
    16 elements per run"""
    b, cases = Batch(), []
    g = vo.rng(11)
    sizes, seeds = (1, 15, 16, 17, 4099), (1, 8, 2147483647, 4294967295)
    for n in sizes:
        nruns = -(-n // 16)
        for seed in seeds:
            specs = [(off, None, 0) for off in (0, 1, 2147483645, 5000000000)]
            specs += [(0, g.permutation(-(-n // S)).astype(np.int32), S) for S in (1, 5, 16, 23)]
            for off, inv, S in specs:
                want = vo.lehmer_stream(n, seed, off, inv, S)
                for real in (False, True):
                    P, R = out(F8, vo.blas_grid(nruns)), out(F8, 1)
                    bufs = [out(F8 if real else C16, n), P, R] + ([cin(inv)] if inv is not None else [])
                    k = b.add("randomize", bufs, [n, -1 if real else 0, 0 if real else -1, off, seed, 1, 3 if inv is not None else -1, S], post=[(1, nruns, 1, 2)])
                    cases.append((k, n, nruns, real, want))
    res = run(b)
    for k, n, nruns, real, want in cases:
        got = res[k].out[0]
        assert vo.exact(got, want if real else want.astype(C16)), b.cases[k][2]
        wl = want.astype(vo.LD)
        grid = vo.blas_grid(nruns)
        r = note("randomize |x|^2", vo.reduction_ratio(res[k].out[2][0], np.sum(wl * wl), n, grid, float(np.sum(wl * wl)), L=16 * vo.chain(nruns, grid)))
        assert r <= 1.0, (b.cases[k][2], r)
    report("randomize |x|^2")
