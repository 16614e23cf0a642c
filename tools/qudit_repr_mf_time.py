#!/usr/bin/env python3
"""Build time and time per apply of the matrix-free d-level momentum sector (qbh_mf_qudit_repr) beside the stored sector of
qbh_gen_qudit_repr, in one process.

  spin1_L22_k0, spin1_L22_kpi   spin-1 Heisenberg chain, L = 22, S^z = 0, k = 0 / pi: build ms (wall: host tables,
                                enumeration, the count pass, adoption), bytes held, ms per apply on complex vectors and on
                                packed-real vectors (Lanczos form y = H x - 0.3 y with both reductions, HIP events), the
                                stored operator's coded SpMV beside them, and E0 of the k = 0 sector from the packed-real
                                Lanczos run against -30.8398988799
  spin1_L24_k0                  L = 24, S^z = 0, k = 0, matrix-free only (the stored form does not fit): packed-real Lanczos
                                to convergence, E0 / L and the time per step

One JSON line per measurement.  Usage: python tools/qudit_repr_mf_time.py [spin1_L22_k0 spin1_L22_kpi spin1_L24_k0]"""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import quantum_basis_amd as q  # noqa: E402
from quantum_basis_amd import _lib  # noqa: E402

E0_L22 = -30.8398988799


def chain(L):
    return [(i, (i + 1) % L) for i in range(L)]


def chain_group(L, m):
    return [[(s + t) % L for s in range(L)] for t in range(L)], np.exp(-2j * np.pi * m * np.arange(L) / L)


def build(L, m, matrix_free, **fmt):
    t0 = time.perf_counter()
    A = q.csr_mat.spin_heisenberg_repr(L, 1, 0, chain(L), *chain_group(L, m), opts=q.make_opts(profile=1, **fmt),
                                       matrix_free=matrix_free)
    A.sync()
    return A, 1e3 * (time.perf_counter() - t0)


def apply_ms(A, reps=5):
    """ms per y = H x - 0.3 y with both reductions on complex vectors (the real fast path packs x when the operator is real)."""
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


def lanczos_real(A, maxit=300):
    """Packed-real Lanczos to convergence on two vectors of dim doubles: (E0, steps, seconds, ms per apply)."""
    n = A.dim
    buf = q.DeviceVec(A, n + 1)                                # two slots of n packed doubles
    try:
        lan = type("V", (), {"ptr": buf.ptr})()
        _lib.check(_lib.lib().qbh_vec_randomize_real(A.handle, buf.ptr, C.c_uint32(1)), "qbh_vec_randomize_real")
        h = np.zeros(2 * maxit)
        A.stats(reset=True)
        t0 = time.perf_counter()
        m = q.lanczos_real(0, maxit - 1, maxit, A, lan, h)
        A.sync()
        sec = time.perf_counter() - t0
        s = A.stats()
        ritz, _ = q.hess_eigen(h, maxit, m, "sr")
        return float(ritz[0]), int(m), sec, s.ms_spmv / max(1, s.n_spmv)
    finally:
        buf.free()


def run_L22(name, m):
    M, build_ms = build(22, m, True)
    i = M.info()
    out = {"case": name, "form": "matrix_free", "build_ms": round(build_ms, 1), "dim": int(M.dim), "contributions": int(M.nnz),
           "bytes_matrix": int(i.bytes_matrix), "tables_in_lds": int(i.kron_table_kernel)}
    Mc, _ = build(22, m, True, real_fast_path=0)
    out["apply_ms_complex"] = round(apply_ms(Mc), 3)
    Mc.destroy()
    E0, steps, sec, ms = lanczos_real(M)
    out.update(apply_ms_packed_real=round(ms, 3), lanczos_steps=steps, lanczos_s=round(sec, 2), E0=E0)
    if m == 0:
        out["E0_error"] = abs(E0 - E0_L22)
        assert out["E0_error"] < 1e-8, out
    print(json.dumps(out), flush=True)
    M.destroy()
    A, build_ms = build(22, m, False)
    print(json.dumps({"case": name, "form": "stored_coded", "build_ms": round(build_ms, 1), "dim": int(A.dim), "nnz": int(A.nnz),
                      "bytes_matrix": int(A.info().bytes_matrix), "spmv_ms": round(apply_ms(A, 10), 3)}), flush=True)
    A.destroy()


def run_L24():
    L = 24
    M, build_ms = build(L, 0, True)
    i = M.info()
    E0, steps, sec, ms = lanczos_real(M)
    print(json.dumps({"case": "spin1_L24_k0", "form": "matrix_free", "build_ms": round(build_ms, 1), "dim": int(M.dim),
                      "contributions": int(M.nnz), "bytes_matrix": int(i.bytes_matrix), "tables_in_lds": int(i.kron_table_kernel),
                      "E0": E0, "E0_per_site": E0 / L, "lanczos_steps": steps, "lanczos_s": round(sec, 1),
                      "step_ms": round(1e3 * sec / max(1, steps), 1), "apply_ms_packed_real": round(ms, 3)}), flush=True)
    M.destroy()


def main():
    for name in sys.argv[1:] or ["spin1_L22_k0", "spin1_L22_kpi", "spin1_L24_k0"]:
        try:
            if name == "spin1_L24_k0":
                run_L24()
            else:
                run_L22(name, {"spin1_L22_k0": 0, "spin1_L22_kpi": 11}[name])
        except _lib.QbhError as e:                            # e.g. out of memory: reported, the next case still runs
            print(json.dumps({"case": name, "error": str(e)}), flush=True)


if __name__ == "__main__":
    main()
