#!/usr/bin/env python3
"""Build time, size and SpMV time of the Kondo-lattice generators (qbh_gen_kondo, qbh_gen_kondo_repr) at full size.

Cases (by name): chain_L12_k0 (chain L = 12, n_elec = 12, S^z = 0, t = 1, J_K = 1.1, the k = 0 momentum sector: 2.05e9 words
enumerated) and chain_L10_full (the whole L = 10, n_elec = 10, S^z = 0 sector, 38,165,260 states), each in the default
format (value codes + real vectors where the operator is real) and as complex128 (value_dict = 0, real_fast_path = 0).
One JSON line per case and format, as tools/qudit_repr_time.py prints them: build ms (wall: host tables, enumeration,
count / scan / fill, adoption), dim, nnz, bytes held, SpMV ms from the library's HIP events (Lanczos form
y = H x - 0.3 y), the fraction of 8 TB/s that bytes_algorithmic / SpMV time reaches and, in the default format, E0 with
its Lanczos step count.  A case that does not fit prints the library's refusal instead.  The lines are also written to
--out (default profiles/kondo_time.txt) under the command that made them.
Usage: python tools/kondo_time.py [--out FILE] [chain_L12_k0 chain_L10_full]"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import quantum_basis_amd as q  # noqa: E402

PEAK = 8.0e12


def chain(L):
    return [(i, (i + 1) % L) for i in range(L)]


def chain_group(L, m):
    return [[(s + t) % L for s in range(L)] for t in range(L)], np.exp(-2j * np.pi * m * np.arange(L) / L)


CASES = {
    "chain_L12_k0": lambda opts: q.csr_mat.kondo_repr(12, 12, 0, chain(12), *chain_group(12, 0), t=1.0, J_K=1.1, opts=opts),
    "chain_L10_full": lambda opts: q.csr_mat.kondo(10, 10, 0, chain(10), t=1.0, J_K=1.1, opts=opts),
}
FORMATS = {"default": {}, "complex128": {"value_dict": 0, "real_fast_path": 0}}


def run(name, fmt, reps=10):
    opts = q.make_opts(profile=1, **FORMATS[fmt])
    t0 = time.perf_counter()
    A = CASES[name](opts)
    A.sync()
    build_ms = 1e3 * (time.perf_counter() - t0)
    info = A.info()
    out = {"case": name, "format": fmt, "build_ms": round(build_ms, 1), "dim": int(A.dim), "nnz": int(A.nnz),
           "bytes_matrix": int(info.bytes_matrix), "bytes_algorithmic": int(info.bytes_algorithmic), "value_dict": int(info.value_dict)}
    v = A.vec(2)
    try:
        A.randomize(v.at(0), 1)
        A.randomize(v.at(A.dim), 2)
        for _ in range(2):
            A.spmv(v.at(0), v.at(A.dim), 1.0, -0.3, 0.0, want_red=True)
        A.stats(reset=True)
        for _ in range(reps):
            A.spmv(v.at(0), v.at(A.dim), 1.0, -0.3, 0.0, want_red=True)
        A.sync()
        s = A.stats()
        ms = s.ms_spmv / max(1, s.n_spmv)
        out.update(spmv_ms=round(ms, 3), spmv_launches=int(s.n_spmv), frac_8TBs=round(info.bytes_algorithmic / (ms * 1e-3) / PEAK, 3))
    finally:
        v.free()
    if fmt == "default":
        t0 = time.perf_counter()
        res = q.locate_E0_lanczos(A, nev=1, ncv=0)
        out.update(E0=res.E0, lanczos_steps=int(res.steps["E0"]), lanczos_s=round(time.perf_counter() - t0, 2))
    A.destroy()
    return out


def main():
    args = sys.argv[1:]
    path = os.path.join(ROOT, "profiles", "kondo_time.txt")
    if args[:1] == ["--out"]:
        path, args = args[1], args[2:]
    lines = ["# python tools/kondo_time.py " + " ".join(args)]
    for name in args or list(CASES):
        for fmt in FORMATS:
            try:
                line = json.dumps(run(name, fmt))
            except q._lib.QbhError as e:                      # e.g. out of memory: reported, the next case still runs
                line = json.dumps({"case": name, "format": fmt, "error": str(e)})
            print(line, flush=True)
            lines.append(line)
            with open(path, "w") as f:                        # after every case: a later failure keeps what was measured
                f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
