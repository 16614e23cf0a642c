#!/usr/bin/env python3
"""Build time, size, SpMV time and ground-state energy of the d-level sector generator (qbh_gen_qudit) at full size.

Models (by name): spin1_L20 (spin-1 Heisenberg chain, L = 20, S^z = 0), spin1_L18 (its fallback), bh4x4 (Bose-Hubbard 4x4,
16 bosons, n_max = 3, t = 1, U = 1.1).  For each model and each format (default: value codes + real vectors; complex128:
value_dict = 0, real_fast_path = 0) it prints one JSON line: build ms (wall, host tables + device count / scan / fill +
adoption), dim, nnz, bytes held, SpMV ms from the library's HIP events (Lanczos form y = H x - 0.3 y), the fraction of
8 TB/s that bytes_algorithmic / SpMV time reaches, and, in the default format, E0 with its Lanczos step count.
Usage: python tools/qudit_time.py [spin1_L20 bh4x4 ...]"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import quantum_basis_amd as q  # noqa: E402

PEAK = 8.0e12


def chain(L):
    return [(i, (i + 1) % L) for i in range(L)]


def square(Lx, Ly):
    site = lambda x, y: (x % Lx) + Lx * (y % Ly)
    return [b for x in range(Lx) for y in range(Ly) for b in ((site(x, y), site(x + 1, y)), (site(x, y), site(x, y + 1)))]


MODELS = {
    "spin1_L20": lambda opts: q.csr_mat.spin_heisenberg(20, 1, 0, chain(20), opts=opts),
    "spin1_L18": lambda opts: q.csr_mat.spin_heisenberg(18, 1, 0, chain(18), opts=opts),
    "bh4x4": lambda opts: q.csr_mat.bose_hubbard(16, 16, 3, square(4, 4), t=1.0, U=1.1, opts=opts),
}
FORMATS = {"default": {}, "complex128": {"value_dict": 0, "real_fast_path": 0}}


def run(name, fmt, reps=10):
    opts = q.make_opts(profile=1, **FORMATS[fmt])
    t0 = time.perf_counter()
    A = MODELS[name](opts)
    A.sync()
    build_ms = 1e3 * (time.perf_counter() - t0)
    info = A.info()
    out = {"model": name, "format": fmt, "build_ms": round(build_ms, 1), "dim": int(A.dim), "nnz": int(A.nnz),
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
    names = sys.argv[1:] or ["spin1_L20", "bh4x4"]
    for name in names:
        for fmt in FORMATS:
            try:
                print(json.dumps(run(name, fmt)), flush=True)
            except q._lib.QbhError as e:                      # e.g. out of memory: reported, the next model still runs
                print(json.dumps({"model": name, "format": fmt, "error": str(e)}), flush=True)


if __name__ == "__main__":
    main()
