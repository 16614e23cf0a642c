#!/usr/bin/env python3
"""Time of the d-level all-pair correlation pass (qbh_corr_qudit_dev) on a packed-real vector beside one apply of the matrix-free
operator of the same sector with ALL N (N - 1) / 2 pairs as bonds (qbh_mf_qudit, the yardstick: it issues two gathers per pair
where the pass issues one), in one process.

For a workload the tool builds the all-pairs matrix-free handle, takes a normalised random real vector (qbh_vec_randomize_real)
and prints, and appends to profiles/qudit_corr_time.txt (--out):
  corr_ms        the full pass (pop, dd with K = 2, str, aa), HIP events around the whole call on the null stream, median of --reps
                 (5) runs after one warm-up; the call includes building and uploading its tables, the second stages and the download
  apply_ms       ms per apply of the all-pairs handle on packed-real vectors (the SpMV of qbh_lanczos_real_dev steps, the
                 library's events), and ratio = corr_ms / apply_ms
  energy         <v| H_allpairs |v> from the correlations beside the first Lanczos coefficient a_1 = <v| H v> of that run.

Workloads: spin1_16, spin1_20, spin1_22 (spin-1, S^z = 0), bose_12 (12 sites, 12 bosons, at most 3 per site).
Usage: python tools/qudit_corr_time.py <workload> [--reps 5] [--out FILE]"""
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
from quantum_basis_amd import _lib  # noqa: E402
from quantum_basis_amd import qudit as qd  # noqa: E402

WORKLOADS = {
    "spin1_16": dict(kind="spin", n_sites=16, S=1),
    "spin1_20": dict(kind="spin", n_sites=20, S=1),
    "spin1_22": dict(kind="spin", n_sites=22, S=1),
    "bose_12": dict(kind="bose", n_sites=12, n_bosons=12, n_max=3, t=1.0, U=1.1),
}
MAXIT = 40


def all_pairs(N):
    return [(i, j) for i in range(N) for j in range(i + 1, N)]


def build(w):
    o = q.make_opts(profile=1)
    if w["kind"] == "spin":
        return q.csr_mat.spin_heisenberg(w["n_sites"], w["S"], 0, all_pairs(w["n_sites"]), J=1.0, opts=o, matrix_free=True)
    return q.csr_mat.bose_hubbard(w["n_sites"], w["n_bosons"], w["n_max"], all_pairs(w["n_sites"]), t=w["t"], U=w["U"], opts=o, matrix_free=True)


def tables(w):
    """(d, total, diag, string, lower) of the full pass"""
    if w["kind"] == "spin":
        d = qd._two_s(w["S"]) + 1
        m = w["S"] - np.arange(d, dtype=np.float64)
        lower = np.real(np.append(0.0, np.diag(qd.spin_matrices(w["S"])[1], 1)))
        return d, qd.spin_charge(w["n_sites"], w["S"], 0), (m, m * m), (m, np.cos(np.pi * m)), lower
    n = np.arange(w["n_max"] + 1, dtype=np.float64)
    return w["n_max"] + 1, w["n_bosons"], (n, n * (n - 1)), (np.ones_like(n), 1.0 - 2.0 * (n % 2)), np.sqrt(n)


def energy(w, c):
    """<v| H_allpairs |v> from the raw arrays"""
    iu = np.triu_indices(w["n_sites"], 1)
    if w["kind"] == "spin":
        return float(np.sum(c["dd"][0, 0][iu] + c["aa"][iu].real))
    n = np.arange(w["n_max"] + 1, dtype=np.float64)
    return float(-w["t"] * 2.0 * np.sum(c["aa"][iu].real) + 0.5 * w["U"] * np.sum(c["pop"] @ (n * (n - 1))))


def random_real(M, v):
    _lib.check(_lib.lib().qbh_vec_randomize_real(M.handle, v.ptr, C.c_uint32(1)), "qbh_vec_randomize_real")
    M.sync()


def apply_ms(M, v, steps=6):
    """(ms per apply on packed-real vectors, a_1 = <v| H v>) from `steps` steps of qbh_lanczos_real_dev started at v's first slot"""
    hess = np.zeros(2 * MAXIT)
    M.stats(reset=True)
    m = q.lanczos_real(0, steps, MAXIT, M, v, hess)
    M.sync()
    s = M.stats()
    assert m >= 1 and s.n_spmv_real == s.n_spmv > 0
    return s.ms_spmv / s.n_spmv, float(hess[MAXIT])


def corr_pass(w, v, reps):
    import torch
    d, total, diag, string, lower = tables(w)

    def once():
        return q.qudit_correlations(w["n_sites"], d, total, v.ptr, diag=diag, string=string, lower=lower, real=True, normalize=False)

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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "qudit_corr_time.txt"))
    a = ap.parse_args()
    w = WORKLOADS[a.workload]
    t0 = time.perf_counter()
    M = build(w)
    N = w["n_sites"]
    out = {"workload": a.workload, "dim": int(M.dim), "vector_bytes_packed": 8 * int(M.dim), "pairs": N * (N - 1) // 2,
           "build_ms": round(1e3 * (time.perf_counter() - t0), 1), "reps": a.reps}
    assert M.info().basis_internal == 0                      # the handle's vectors are in the generator's order
    v = M.vec(1)                                             # two slots of dim doubles
    random_real(M, v)
    med, ms, corr = corr_pass(w, v, a.reps)
    out.update(corr_ms=round(med, 3), corr_ms_runs=[round(x, 3) for x in ms], norm2=corr["norm2"])
    e_corr = energy(w, corr)
    ms_apply, a1 = apply_ms(M, v)
    out.update(allpairs_apply_ms=round(ms_apply, 3), ratio_corr_over_allpairs_apply=round(med / ms_apply, 4), energy_from_correlations=e_corr,
               energy_lanczos_a1=a1, energy_diff=abs(e_corr - a1))
    v.free()
    M.destroy()
    line = json.dumps(out)
    print(line, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
