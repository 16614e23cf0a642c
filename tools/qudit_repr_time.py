#!/usr/bin/env python3
"""Build time, size, SpMV time and ground-state energy of the d-level momentum-sector generator (qbh_gen_qudit_repr) at
full size.

Cases (by name): spin1_L22_k0 and spin1_L22_kpi (spin-1 Heisenberg chain, L = 22, S^z = 0, k = 0 / pi), spin1_L22_sz1_kpi
(the same chain at S^z = 1, k = pi; with spin1_L22_k0 in the same run it also prints the gap E(pi, 1) - E(0, 0)),
bh4x4_k00 (Bose-Hubbard 4x4 torus, 16 bosons, n_max = 3, t = 1, U = 1.1, k = (0, 0)).  Formats: default (value codes +
real vectors) for every case, complex128 (value_dict = 0, real_fast_path = 0) for the S^z = 0 chain sectors.  One JSON
line per case and format, as tools/qudit_time.py prints them: build ms (wall: host tables, enumeration, count / scan /
fill, adoption), dim, nnz, bytes held, SpMV ms from the library's HIP events (Lanczos form y = H x - 0.3 y), the fraction
of 8 TB/s that bytes_algorithmic / SpMV time reaches and, in the default format, E0 with its Lanczos step count.
A case that does not fit prints the library's refusal instead.
Usage: python tools/qudit_repr_time.py [spin1_L22_k0 spin1_L22_kpi ...]"""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import quantum_basis_amd as q  # noqa: E402

PEAK = 8.0e12


def chain(L):
    return [(i, (i + 1) % L) for i in range(L)]


def chain_group(L, m):
    return [[(s + t) % L for s in range(L)] for t in range(L)], np.exp(-2j * np.pi * m * np.arange(L) / L)


def square(Lx, Ly):
    site = lambda x, y: (x % Lx) + Lx * (y % Ly)
    return [b for x in range(Lx) for y in range(Ly) for b in ((site(x, y), site(x + 1, y)), (site(x, y), site(x, y + 1)))]


def torus_group(Lx, Ly):
    site = lambda x, y: (x % Lx) + Lx * (y % Ly)
    perms = [[site(x + tx, y + ty) for y in range(Ly) for x in range(Lx)] for ty in range(Ly) for tx in range(Lx)]
    return perms, np.ones(len(perms), dtype=np.complex128)


def spin1(L, two_sz, m):
    return lambda opts: q.csr_mat.spin_heisenberg_repr(L, 1, two_sz, chain(L), *chain_group(L, m), opts=opts)


CASES = {
    "spin1_L22_k0": (spin1(22, 0, 0), ("default", "complex128")),
    "spin1_L22_kpi": (spin1(22, 0, 11), ("default", "complex128")),
    "spin1_L22_sz1_kpi": (spin1(22, 2, 11), ("default",)),
    "bh4x4_k00": (lambda opts: q.csr_mat.bose_hubbard_repr(16, 16, 3, square(4, 4), *torus_group(4, 4), t=1.0, U=1.1, opts=opts),
                  ("default",)),
}
FORMATS = {"default": {}, "complex128": {"value_dict": 0, "real_fast_path": 0}}


def run(name, fmt, reps=10):
    opts = q.make_opts(profile=1, **FORMATS[fmt])
    t0 = time.perf_counter()
    A = CASES[name][0](opts)
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
    names = sys.argv[1:] or list(CASES)
    E0 = {}
    for name in names:
        for fmt in CASES[name][1]:
            try:
                out = run(name, fmt)
                if "E0" in out:
                    E0[name] = out["E0"]
                print(json.dumps(out), flush=True)
            except q._lib.QbhError as e:                      # e.g. out of memory: reported, the next case still runs
                print(json.dumps({"case": name, "format": fmt, "error": str(e)}), flush=True)
    if "spin1_L22_k0" in E0 and "spin1_L22_sz1_kpi" in E0:
        print(json.dumps({"gap": "E(pi, S^z = 1) - E(0, S^z = 0)", "L": 22, "value": E0["spin1_L22_sz1_kpi"] - E0["spin1_L22_k0"]}),
              flush=True)


if __name__ == "__main__":
    main()
