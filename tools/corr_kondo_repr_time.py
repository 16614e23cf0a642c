#!/usr/bin/env python3
"""Times of qbh_corr_kondo_repr_dev (all-pair correlations of a Kondo momentum-sector state), HIP events around whole calls on the
null stream, on the chain at half filling (n_elec = L, S^z = 0) at k = 0, packed real and complex, in one process per size.  Beside
them, for scale, one apply of qbh_mf_kondo_repr built with a hop on every ordered site pair, a local-spin exchange bond on every pair
and the Kondo flip on every site -- the operator whose rows issue the gathers of hop, ll and the diagonal of le in one go (it has no
ee and no off-diagonal le term: the correlation call gathers more than it).  No ratio is a pass criterion.

Per size one JSON line, printed and appended to profiles/corr_kondo_repr_time.txt (--out):
  enumerate_ms       the call with only norm2 asked for: the enumeration of the sector, the tables and the site pass
  corr_complex_ms    the full call on a complex vector; every call enumerates the sector again, so corr - enumerate is the passes
  corr_real_ms       the same on the packed real parts
  group_ms           the call with one group alone (site, nn, zn, zz, hop, ee, ll, le), complex; each includes the enumeration
  mf_apply_ms        one y = H x of the all-pairs operator, complex vectors (real_fast_path = 0); mf_apply_real_ms with the packed-
                     real fast path; mf_build_ms the creation of the handle (wall)
  gathers_per_row    candidate gathers per row: of the correlation call per group from the occupation counts, averaged over the
                     WORDS of the sector (hop: n_s (N - n_s) per species; ee: n_up (N - n_up) n_dn (N - n_dn) / (N (N - 1)); ll:
                     m (N - m); le: (N - m) n_dn (N - n_up) / N; m = popcount(s)), and of the apply from the handle's count of
                     contributions (diagonal included) / dim

Sizes: L10, L12 (one sector each) and L13 (1.17e9 representatives: 19 GB of vector beside 15 GB of code bytes during the
enumeration and the matrix-free handle; left out with --sizes when memory or time does not allow it).  Each size runs in a fresh
child process under its own time limit; a size that fails or runs out of time ends the run.
Usage: python tools/corr_kondo_repr_time.py [--sizes L10 L12 L13] [--reps 3]"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time
from math import comb

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = {"L10": (10, 300), "L12": (12, 600), "L13": (13, 1100)}      # name: (sites, time limit in seconds)
GROUPS = ("site", "nn", "zn", "zz", "hop", "ee", "ll", "le")


def timed(fn):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), out


def median_ms(fn, reps):
    if reps > 1:
        fn()                                                 # warm-up
    ms = [timed(fn)[0] for _ in range(reps)]
    return round(statistics.median(ms), 3), [round(x, 3) for x in ms]


def corr_call(L, p, c, t, want):
    import torch
    from quantum_basis_amd import _lib
    real = t.dtype == torch.float64
    n2, dim = C.c_double(), C.c_int64()
    z = np.complex128
    bufs = {"site": np.zeros((4, L)), "nn": np.zeros((4, L, L)), "zn": np.zeros((2, L, L)), "zz": np.zeros((L, L)),
            "hop": np.zeros((2, L, L), dtype=z), "ee": np.zeros((L, L), dtype=z), "ll": np.zeros((L, L), dtype=z), "le": np.zeros((L, L), dtype=z)}
    ptr = [bufs[k].ctypes.data_as(C.c_void_p) if k in want else None for k in GROUPS]
    addr = C.c_void_p(t.data_ptr())
    _lib.check(_lib.lib().qbh_corr_kondo_repr_dev(L, L, 0, len(p), p.ctypes.data_as(C.c_void_p), c.ctypes.data_as(C.c_void_p),
                                                  None if real else addr, addr if real else None, C.byref(n2), *ptr, C.byref(dim), None),
               "qbh_corr_kondo_repr_dev")
    return n2.value, dim.value


def gathers_per_word(L):
    """the candidate gathers of one row per group, averaged over the words of the sector (n_elec = L, S^z = 0)"""
    from quantum_basis_amd import kondo
    tot, g = 0, dict(hop=0.0, ee=0.0, ll=0.0, le=0.0)
    for nu, nd, m in kondo.sector_blocks(L, L, 0):
        w = comb(L, m) * comb(L, nu) * comb(L, nd)
        tot += w
        g["hop"] += w * (nu * (L - nu) + nd * (L - nd))
        g["ee"] += w * (nu * (L - nu) * nd * (L - nd) / (L * (L - 1)))
        g["ll"] += w * m * (L - m)
        g["le"] += w * ((L - m) * nd * (L - nu) / L)
    return {k: round(v / tot, 3) for k, v in g.items()}


def all_pairs_terms(L):
    """a hop on every ordered pair, a local-spin exchange bond on every pair (both by ring distance: translation invariant) and
    the Kondo couplings on every site"""
    from quantum_basis_amd import kondo
    dist = lambda i, j: min((j - i) % L, (i - j) % L)
    hops = [(i, j, -1.0 / dist(i, j), -1.0 / dist(i, j)) for i in range(L) for j in range(L) if i != j]
    sb = [(i, j, 0.4 / dist(i, j), 0.9 / dist(i, j)) for i in range(L) for j in range(i + 1, L)]
    return kondo.Terms(hops, [1.1] * L, [1.1] * L, sb)


def one(name, reps):
    import torch
    import quantum_basis_amd as q
    L = SIZES[name][0]
    perms = np.array([[(s + t) % L for s in range(L)] for t in range(L)], dtype=np.int32)
    chars = np.ones(L, dtype=np.complex128)
    out = {"size": name, "n_sites": L, "n_elec": L, "two_sz": 0, "k": 0, "n_trans": L, "reps": reps}
    T = all_pairs_terms(L)
    t0 = time.perf_counter()
    M = q.csr_mat.kondo_repr(L, L, 0, None, perms, chars, terms=T, matrix_free=True)
    M.sync()
    out["mf_build_ms"] = round(1e3 * (time.perf_counter() - t0), 1)
    dim = int(M.dim)
    out.update(dim=dim, mf_contributions=int(M.nnz))
    v = M.vec(2)
    M.randomize(v.at(0), 1)
    med, runs = median_ms(lambda: (M.spmv(v.at(0), v.at(dim), 1.0, 0.0, 0.0), M.sync()), reps)
    out.update(mf_apply_real_ms=med, mf_apply_real_ms_runs=runs)
    v.free()
    M.destroy()
    Mc = q.csr_mat.kondo_repr(L, L, 0, None, perms, chars, terms=T, matrix_free=True, opts=q.make_opts(real_fast_path=0))
    v = Mc.vec(2)
    Mc.randomize(v.at(0), 1)
    med, runs = median_ms(lambda: (Mc.spmv(v.at(0), v.at(dim), 1.0, 0.0, 0.0), Mc.sync()), reps)
    out.update(mf_apply_ms=med, mf_apply_ms_runs=runs)
    v.free()
    Mc.destroy()
    print("%s dim %d: apply %.1f ms complex, %.1f ms packed real" % (name, dim, out["mf_apply_ms"], out["mf_apply_real_ms"]), file=sys.stderr, flush=True)
    gen = torch.Generator(device="cuda").manual_seed(1)
    x = torch.randn(dim, 2, dtype=torch.float64, device="cuda", generator=gen)
    x /= torch.linalg.norm(x)
    xc = torch.view_as_complex(x).contiguous()
    xr = x[:, 0].contiguous()
    del x
    torch.cuda.synchronize()
    med, runs = median_ms(lambda: corr_call(L, perms, chars, xc, ()), reps)
    out.update(enumerate_ms=med, enumerate_ms_runs=runs)
    med, runs = median_ms(lambda: corr_call(L, perms, chars, xc, GROUPS), reps)
    out.update(corr_complex_ms=med, corr_complex_ms_runs=runs)
    med, runs = median_ms(lambda: corr_call(L, perms, chars, xr, GROUPS), reps)
    out.update(corr_real_ms=med, corr_real_ms_runs=runs)
    print("%s correlations: %.1f ms complex, %.1f ms packed real, enumeration %.1f ms" % (
        name, out["corr_complex_ms"], out["corr_real_ms"], out["enumerate_ms"]), file=sys.stderr, flush=True)
    out["group_ms"] = {g: median_ms(lambda: corr_call(L, perms, chars, xc, (g,)), reps)[0] for g in GROUPS}
    n2, d = corr_call(L, perms, chars, xc, ())
    assert d == dim
    gp = gathers_per_word(L)
    gp["corr_total"] = round(sum(gp.values()), 3)
    gp["mf_apply"] = round(out["mf_contributions"] / dim, 3)
    out.update(norm2=n2, gathers_per_row=gp)
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", nargs="+", default=["L10", "L12", "L13"], choices=sorted(SIZES))
    ap.add_argument("--reps", type=int, default=3, help="timed runs per call at L10 and L12; L13 is timed once")
    ap.add_argument("--one", help=argparse.SUPPRESS)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "corr_kondo_repr_time.txt"))
    a = ap.parse_args()
    if a.one:
        one(a.one, 1 if a.one == "L13" else a.reps)
        return 0
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    for name in a.sizes:
        cmd = [sys.executable, os.path.abspath(__file__), "--one", name, "--reps", str(a.reps)]
        try:
            r = subprocess.run(cmd, stdout=subprocess.PIPE, timeout=SIZES[name][1], text=True)
            line = r.stdout.strip().splitlines()[-1] if r.returncode == 0 and r.stdout.strip() else json.dumps({"size": name, "status": "exit %d" % r.returncode})
            ok = r.returncode == 0
        except subprocess.TimeoutExpired:
            line, ok = json.dumps({"size": name, "status": "not finished within %d s" % SIZES[name][1]}), False
        print(line, flush=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")
        if not ok:
            return 1                                         # nothing more is started on the device after a failure
    return 0


if __name__ == "__main__":
    sys.exit(main())
