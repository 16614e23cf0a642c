#!/usr/bin/env python3
"""Time per application of the operators between Kondo momentum sectors (qbh_mopr_kondo_repr_dev) beside the time per apply of
the sector operator of the target sector (qbh_mf_kondo_repr), in one process.  The ring at half filling (n_elec = L,
S^z = 0, t = 1, J_K = 1.1), source momentum k = 0, operator momentum q = 2 pi / L:

  c_up      c_{q,up}: (L, 0) -> (L - 1, -1)
  s_minus   the total S^-_q, electrons and local spins: (L, 0) -> (L, -2)

A call enumerates both sectors before its one kernel runs; what is recorded is the wall time of a whole call.  Beside it, for
scale: the build time of the matrix-free sector operator of the source and of the target sector (each holds one such
enumeration and a count pass) and its ms per apply (y = H x - 0.3 y with both reductions, complex vectors) on the target sector.

One JSON line per measurement, printed and written to the output file.
Usage: python tools/kondo_mopr_time.py [L] [--out profiles/kondo_mopr_time.txt]"""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import quantum_basis_amd as q  # noqa: E402
from quantum_basis_amd import kondo  # noqa: E402


def chain(L):
    return [(i, (i + 1) % L) for i in range(L)]


def chain_group(L, m):
    return [[(s + t) % L for s in range(L)] for t in range(L)], np.exp(-2j * np.pi * ((m * np.arange(L)) % L) / L)


def sector_operator(L, n_elec, two_sz, m):
    t0 = time.perf_counter()
    A = q.csr_mat.kondo_repr(L, n_elec, two_sz, chain(L), *chain_group(L, m), t=1.0, J_K=1.1, opts=q.make_opts(profile=1, real_fast_path=0),
                             matrix_free=True)
    A.sync()
    return A, 1e3 * (time.perf_counter() - t0)


def apply_ms(A, reps=5):
    v = A.vec(2)
    try:
        A.randomize(v.at(0), 1)
        A.randomize(v.at(A.dim), 2)
        A.spmv(v.at(0), v.at(A.dim), 1.0, -0.3, 0.0, want_red=True)
        A.stats(reset=True)
        for _ in range(reps):
            A.spmv(v.at(0), v.at(A.dim), 1.0, -0.3, 0.0, want_red=True)
        A.sync()
        s = A.stats()
        return s.ms_spmv / max(1, s.n_spmv)
    finally:
        v.free()


def call_ms(L, op, perms, chars, ce, cs, x, y, reps=3):
    """wall ms of a whole call (it synchronises before it returns), the best of reps after one warm-up"""
    best = None
    for r in range(reps + 1):
        t0 = time.perf_counter()
        dims = q.moprXvec_kondo_repr(L, L, 0, op, perms, chars, ce, cs, x, y)
        ms = 1e3 * (time.perf_counter() - t0)
        if r:
            best = ms if best is None else min(best, ms)
    return best, dims


def main():
    args = sys.argv[1:]
    out_path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "kondo_mopr_time.txt")
    if "--out" in args:
        i = args.index("--out")
        out_path = args[i + 1]
        del args[i:i + 2]
    L = int(args[0]) if args else 12
    lines = ["# python tools/kondo_mopr_time.py %d   (one MI355X, one process)" % L]

    def emit(d):
        lines.append(json.dumps(d))
        print(lines[-1], flush=True)

    perms, chars = chain_group(L, 0)
    wave = np.exp(2j * np.pi * np.arange(L) / L) / np.sqrt(L)
    S, source_build_ms = sector_operator(L, L, 0, 0)
    x = S.vec(1)
    S.randomize(x.at(0), 1)
    S.sync()
    for name, op, ce, cs in (("c_up", kondo.C_UP, wave, None), ("s_minus", kondo.SPIN_MINUS, wave, wave)):
        ne, sz = kondo.mopr_target(L, 0, op)
        T, build_ms = sector_operator(L, ne, sz, L - 1)        # k - q = -1
        y = q.DeviceVec(T, T.dim + T.dim // 8 + 1024)      # room to spare: the call, not this tool, decides the target momentum
        ms, dims = call_ms(L, op, perms, chars, ce, cs, x.ptr, y.ptr)
        assert dims == (S.dim, T.dim), (dims, S.dim, T.dim)
        norm = T.nrm2(y.ptr)
        emit({"case": "ring_L%d_k0_q1" % L, "op": name, "dim_old": int(dims[0]), "dim_new": int(dims[1]), "call_ms": round(ms, 1),
              "norm_ratio": norm / S.nrm2(x.ptr), "source_sector_build_ms": round(source_build_ms, 1),
              "target_sector_build_ms": round(build_ms, 1), "target_sector_apply_ms": round(apply_ms(T), 3)})
        y.free()
        T.destroy()
    x.free()
    S.destroy()
    os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
