#!/usr/bin/env python3
"""Time of the all-pair correlation pass (qbh_corr_spin_dev / qbh_corr_hubbard_dev) on a packed-real vector beside one apply of
the matrix-free operator of the same sector, in one process.

For a workload the tool builds the matrix-free handle, takes a normalised random real vector (qbh_vec_randomize_real) and prints,
and appends to profiles/correlations_time.txt (--out):
  corr_ms        the correlation pass (all groups), HIP events around the call on the null stream, median of --reps (5) runs after
                 one warm-up; the call includes building and uploading its tables and the second-stage reduction
  apply_ms       ms per apply of the handle on packed-real vectors (the SpMV of qbh_lanczos_real_dev steps, the library's events)
  energy         <v| H |v> from the correlations (energy_from_correlations) beside the first Lanczos coefficient a_1 = <v| H v> of
                 that run -- the SpMV and the dot product of the existing path on the same vector -- and their difference.
                 This stands in for spmv + dotc: the library's stand-alone spmv and dotc take complex vectors only, and the
                 workloads here are packed real (a complex pair would not fit beside the state at kagome_36a); the first step of
                 qbh_lanczos_real_dev is the packed-real SpMV followed by the packed-real dot product, the same two operations.
                 tests/test_gpu_corr.py checks the identity against spmv + dotc proper on complex vectors.
Heisenberg workloads also build qbh_mf_heisenberg on the same sector with the ALL-PAIRS bond list (N (N - 1) / 2 bonds): that
kernel issues every gather of the correlation pass and as many again, so its apply is the yardstick (allpairs_apply_ms, ratio =
corr_ms / allpairs_apply_ms).  --no-yardstick leaves it out (kagome_36a: the second handle costs another 2 x 72.6 GB run).

Workloads: heis_24 (chain, Sz = 0), kagome_30, kagome_36a, hubbard_4x5_n7.
Usage: python tools/correlations_time.py <workload> [--reps 5] [--out FILE] [--no-yardstick]"""
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
from quantum_basis_amd import _lib, lattices  # noqa: E402

WORKLOADS = {
    "heis_24": dict(kind="heisenberg", n_sites=24, n_dn=12, bonds=lattices.chain(24)),
    "kagome_30": dict(kind="heisenberg", n_sites=30, n_dn=15, bonds=lattices.kagome(5, 2)),
    "kagome_36a": dict(kind="heisenberg", n_sites=36, n_dn=18, bonds=lattices.kagome_torus((4, 2), (2, 4))),
    "hubbard_4x5_n7": dict(kind="hubbard", n_sites=20, n_up=7, n_dn=7, bonds=lattices.square(4, 5), t=1.0, U=1.1),
}
MAXIT = 40


def build(w, bonds=None):
    o = q.make_opts(profile=1)
    if w["kind"] == "heisenberg":
        return q.csr_mat.heisenberg(w["n_sites"], w["n_dn"], bonds if bonds is not None else w["bonds"], J=1.0, opts=o, matrix_free=True)
    return q.csr_mat.hubbard(w["n_sites"], w["n_up"], w["n_dn"], w["bonds"], t=w["t"], U=w["U"], opts=o, matrix_free=True)


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

    def once():
        if w["kind"] == "heisenberg":
            return q.spin_correlations(w["n_sites"], w["n_dn"], v.ptr, real=True, normalize=False)
        return q.hubbard_correlations(w["n_sites"], w["n_up"], w["n_dn"], v.ptr, real=True, normalize=False)

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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "correlations_time.txt"))
    ap.add_argument("--no-yardstick", action="store_true")
    a = ap.parse_args()
    w = WORKLOADS[a.workload]
    t0 = time.perf_counter()
    M = build(w)
    out = {"workload": a.workload, "dim": int(M.dim), "vector_bytes_packed": 8 * int(M.dim), "build_ms": round(1e3 * (time.perf_counter() - t0), 1),
           "reps": a.reps}
    assert M.info().basis_internal == 0                      # the handle's vectors are in the generators' order
    v = M.vec(1)                                             # two slots of dim doubles
    random_real(M, v)
    med, ms, corr = corr_pass(w, v, a.reps)
    out.update(corr_ms=round(med, 3), corr_ms_runs=[round(x, 3) for x in ms], norm2=corr["norm2"])
    if w["kind"] == "heisenberg":
        e_corr = q.energy_from_correlations(corr, w["bonds"], J=1.0)
    else:
        e_corr = q.energy_from_correlations(corr, w["bonds"], t=w["t"], U=w["U"])
    ms_apply, a1 = apply_ms(M, v)
    out.update(apply_ms=round(ms_apply, 3), n_bonds=len(w["bonds"]), energy_from_correlations=e_corr, energy_lanczos_a1=a1,
               energy_diff=abs(e_corr - a1))
    v.free()
    M.destroy()
    if w["kind"] == "heisenberg" and not a.no_yardstick:
        N = w["n_sites"]
        pairs = [(i, j) for i in range(N) for j in range(i + 1, N)]
        Y = build(w, pairs)
        v = Y.vec(1)
        random_real(Y, v)
        ms_all, _ = apply_ms(Y, v)
        v.free()
        Y.destroy()
        out.update(allpairs_bonds=len(pairs), allpairs_apply_ms=round(ms_all, 3), ratio_corr_over_allpairs_apply=round(med / ms_all, 4))
    line = json.dumps(out)
    print(line, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
