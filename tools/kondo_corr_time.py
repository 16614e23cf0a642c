#!/usr/bin/env python3
"""Time of the Kondo all-pair correlation pass (qbh_corr_kondo_dev) on a packed-real vector beside one apply of the matrix-free
operator of the same sector (qbh_mf_kondo, the yardstick) with all N (N - 1) directed hops of both species, all N (N - 1) / 2
local-spin bonds with bxy != 0 and kxy != 0 on every site, in one process.

The two sides do not issue the same number of gathers, so the candidate gathers per row are printed beside the times:
  pass       hop N (N - 1) (i < j, both species) + ee N (N - 1) / 2 + ll N (N - 1) / 2 + le N^2
  yardstick  hops 2 N (N - 1) + local-spin exchange N (N - 1) / 2 + Kondo flips N          (no ee, N of the le gathers)
and the aim is parity per candidate gather: time ratio <= gather ratio.

For a workload (a periodic chain at half filling, two_sz = 0) the tool builds the yardstick handle, takes a normalised random real
vector (qbh_vec_randomize_real) and prints, and appends to profiles/kondo_corr_time.txt (--out):
  corr_ms        the full pass (every group), HIP events around the whole call on the null stream, median of --reps (5) runs after
                 one warm-up; the call includes building and uploading its tables, the second stages and the download
  apply_ms       ms per apply of the yardstick handle on packed-real vectors (the SpMV of qbh_lanczos_real_dev steps, the library's
                 events), ratio = corr_ms / apply_ms, and gather_ratio
  energy         <v| H |v> of the yardstick operator from the correlations beside the first Lanczos coefficient a_1 = <v| H v>.

Workloads: L10 (3.8e7 rows), L12 (2.05e9 rows, 16 GB a packed-real vector), L13 (1.5e10 rows, 121 GB).
Usage: python tools/kondo_corr_time.py <workload> [--reps 5] [--steps 6] [--out FILE]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import quantum_basis_amd as q  # noqa: E402
from quantum_basis_amd import _lib, kondo  # noqa: E402

WORKLOADS = {"L10": 10, "L12": 12, "L13": 13}
MAXIT = 40


def yardstick_terms(N):
    hops = [(i, j, -1.0, -1.0) for i in range(N) for j in range(N) if i != j]
    sbonds = [(i, j, 1.0, 1.0) for i in range(N) for j in range(i + 1, N)]
    return kondo.Terms(hops, [1.0] * N, [1.0] * N, sbonds)


def gathers(N):
    """candidate gathers per row: (the pass, the yardstick apply)"""
    return N * (N - 1) + N * (N - 1) // 2 + N * (N - 1) // 2 + N * N, 2 * N * (N - 1) + N * (N - 1) // 2 + N


def random_real(M, v):
    _lib.check(_lib.lib().qbh_vec_randomize_real(M.handle, v.ptr, C.c_uint32(1)), "qbh_vec_randomize_real")
    M.sync()


def apply_ms(M, v, steps):
    """(ms per apply on packed-real vectors, a_1 = <v| H v>) from `steps` steps of qbh_lanczos_real_dev started at v's first slot"""
    hess = np.zeros(2 * MAXIT)
    M.stats(reset=True)
    m = q.lanczos_real(0, steps, MAXIT, M, v, hess)
    M.sync()
    s = M.stats()
    assert m >= 1 and s.n_spmv_real == s.n_spmv > 0
    return s.ms_spmv / s.n_spmv, float(hess[MAXIT])


def corr_pass(N, v, reps):
    import torch

    def once():
        return q.kondo_correlations(N, N, 0, v.ptr, real=True, normalize=False)

    once()                                                   # warm-up
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        corr = once()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return statistics.median(ms), ms, corr


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("workload", choices=sorted(WORKLOADS))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--steps", type=int, default=6, help="Lanczos steps of the yardstick run")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kondo_corr_time.txt"))
    a = ap.parse_args()
    N = WORKLOADS[a.workload]
    T = yardstick_terms(N)
    t0 = time.perf_counter()
    M = q.csr_mat.kondo(N, N, 0, None, terms=T, opts=q.make_opts(profile=1), matrix_free=True)
    g_pass, g_apply = gathers(N)
    out = {"workload": a.workload, "n_sites": N, "dim": int(M.dim), "vector_bytes_packed": 8 * int(M.dim),
           "build_ms": round(1e3 * (time.perf_counter() - t0), 1), "reps": a.reps, "gathers_per_row_pass": g_pass,
           "gathers_per_row_apply": g_apply, "gather_ratio": round(g_pass / g_apply, 4)}
    assert M.info().basis_internal == 0                      # the handle's vectors are in the generator's order
    v = M.vec(1)                                             # two slots of dim doubles
    random_real(M, v)
    med, ms, corr = corr_pass(N, v, a.reps)
    out.update(corr_ms=round(med, 3), corr_ms_runs=[round(x, 3) for x in ms], norm2=corr["norm2"])
    e_corr = q.kondo_energy_from_correlations(corr, T)
    ms_apply, a1 = apply_ms(M, v, a.steps)
    out.update(yardstick_apply_ms=round(ms_apply, 3), ratio_corr_over_apply=round(med / ms_apply, 4), energy_from_correlations=e_corr,
               energy_lanczos_a1=a1, energy_diff=abs(e_corr - a1), total_spin=corr["total_spin"])
    v.free()
    M.destroy()
    line = json.dumps(out)
    print(line, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
