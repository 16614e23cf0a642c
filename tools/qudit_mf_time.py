#!/usr/bin/env python3
"""Time per apply of the matrix-free d-level operator (qbh_mf_qudit) beside the stored operator of qbh_gen_qudit, and the
full-size run the stored form cannot reach.

Models (by name): spin1_L20 (spin-1 Heisenberg chain, L = 20, S^z = 0), bh4x4 (Bose-Hubbard 4x4, 16 bosons, n_max = 3, t = 1,
U = 1.1).  For each it prints one JSON line with: the build time of the matrix-free handle (host tables + the device count
pass for nnz), the bytes of its tables, ms per apply on complex vectors (y = H x - 0.3 y with both reductions, from the
library's HIP events) and on packed-real vectors (the SpMV of qbh_lanczos_real_dev steps), and, measured in the same process
right after, the stored operator's SpMV ms in its default format (the numbers of profiles/qudit_time.txt).
spin1_L22: spin-1 chain L = 22, S^z = 0, full basis (3.2e9 states, beyond int32 columns): packed-real Lanczos to convergence on
the matrix-free handle, then E0 of the k = 0 momentum sector of the same chain from the stored csr_mat.spin_heisenberg_repr, and
their difference.
Usage: python tools/qudit_mf_time.py [spin1_L20 bh4x4 spin1_L22 ...]"""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import quantum_basis_amd as q  # noqa: E402
from quantum_basis_amd import _lib  # noqa: E402


def chain(L):
    return [(i, (i + 1) % L) for i in range(L)]


def chain_group(L, m):
    return [[(s + t) % L for s in range(L)] for t in range(L)], np.exp(-2j * np.pi * m * np.arange(L) / L)


def square(Lx, Ly):
    site = lambda x, y: (x % Lx) + Lx * (y % Ly)
    return [b for x in range(Lx) for y in range(Ly) for b in ((site(x, y), site(x + 1, y)), (site(x, y), site(x, y + 1)))]


MODELS = {
    "spin1_L20": lambda **kw: q.csr_mat.spin_heisenberg(20, 1, 0, chain(20), **kw),
    "bh4x4": lambda **kw: q.csr_mat.bose_hubbard(16, 16, 3, square(4, 4), t=1.0, U=1.1, **kw),
}


def spmv_ms(A, reps=10):
    """ms per y = H x - 0.3 y on complex vectors, from the handle's HIP events (as tools/qudit_time.py)."""
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
        return s.ms_spmv / max(1, s.n_spmv)
    finally:
        v.free()


def real_lanczos(A, steps, maxit, chunk=None, log=None):
    """qbh_lanczos_real_dev on two slots of A.dim packed doubles: returns (steps run, hessenberg, ms per SpMV, ms per step)."""
    v = A.vec(1)                                             # dim complex128 = 2 dim doubles
    try:
        _lib.check(_lib.lib().qbh_vec_randomize_real(A.handle, v.ptr, C.c_uint32(1)), "qbh_vec_randomize_real")
        hess = np.zeros(2 * maxit)
        A.stats(reset=True)
        t0 = time.perf_counter()
        m, state = 0, None
        while m < steps:
            want = min(chunk or steps, steps - m)
            m2 = q.lanczos_real(m, want, maxit, A, v, hess, state=state)
            state = q.lanczos_real.last["state"]
            if log:
                log(m2, hess)
            if m2 < m + want:                                # converged
                m = m2
                break
            m = m2
        A.sync()
        wall = 1e3 * (time.perf_counter() - t0)
        s = A.stats()
        assert s.n_spmv_real == s.n_spmv > 0
        return m, hess, s.ms_spmv / s.n_spmv, wall / max(1, m)
    finally:
        v.free()


def compare(name):
    t0 = time.perf_counter()
    M = MODELS[name](matrix_free=True, opts=q.make_opts(profile=1))
    M.sync()
    out = {"model": name, "mf_build_ms": round(1e3 * (time.perf_counter() - t0), 1), "dim": int(M.dim), "nnz": int(M.nnz),
           "mf_bytes_tables": int(M.info().bytes_matrix)}
    out["mf_ms_complex"] = round(spmv_ms(M), 3)
    _, _, ms_real, _ = real_lanczos(M, 12, 40)
    out["mf_ms_real"] = round(ms_real, 3)
    M.destroy()
    A = MODELS[name](opts=q.make_opts(profile=1))
    out.update(stored_bytes_matrix=int(A.info().bytes_matrix), stored_ms_default=round(spmv_ms(A), 3))
    assert (A.dim, A.nnz) == (out["dim"], out["nnz"])
    A.destroy()
    return out


def full_size(L=22):
    maxit = 400
    t0 = time.perf_counter()
    M = q.csr_mat.spin_heisenberg(L, 1, 0, chain(L), matrix_free=True, opts=q.make_opts(profile=1))
    out = {"model": "spin1_L%d" % L, "mf_build_ms": round(1e3 * (time.perf_counter() - t0), 1), "dim": int(M.dim), "nnz": int(M.nnz),
           "mf_bytes_tables": int(M.info().bytes_matrix), "vector_bytes_packed": 8 * int(M.dim)}

    def log(m, hess):
        print("# step %d  E0 ~ %.12f" % (m, q.hess_eigen(hess, maxit, m, "sr")[0][0]), flush=True)

    m, hess, ms_spmv, ms_step = real_lanczos(M, maxit - 1, maxit, chunk=20, log=log)
    e_full = float(q.hess_eigen(hess, maxit, m, "sr")[0][0])
    out.update(lanczos_steps=int(m), mf_ms_real=round(ms_spmv, 2), ms_per_step=round(ms_step, 2), E0=e_full)
    M.destroy()
    S = q.csr_mat.spin_heisenberg_repr(L, 1, 0, chain(L), *chain_group(L, 0))
    res = q.locate_E0_lanczos(S, nev=1, ncv=0)
    out.update(sector_k0_dim=int(S.dim), sector_k0_E0=res.E0, E0_minus_sector=e_full - res.E0)
    S.destroy()
    return out


def main():
    for name in sys.argv[1:] or ["spin1_L20", "bh4x4", "spin1_L22"]:
        try:
            print(json.dumps(full_size(int(name[7:])) if name.startswith("spin1_L") and name not in MODELS else compare(name)), flush=True)
        except q._lib.QbhError as e:                          # e.g. out of memory: reported, the next model still runs
            print(json.dumps({"model": name, "error": str(e)}), flush=True)


if __name__ == "__main__":
    main()
