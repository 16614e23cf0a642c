#!/usr/bin/env python3
"""Time per apply of the matrix-free Kondo-lattice operator (qbh_mf_kondo) beside the stored operator of qbh_gen_kondo, and
the full-size runs the stored form cannot reach.  One process, one JSON line per case.

chain_L10: chain L = 10 at half filling, S^z = 0 (dim 38,165,260).  Build time of the matrix-free handle (host tables + the
device count pass for nnz), bytes of its tables, ms per apply on complex vectors (y = H x - 0.3 y with both reductions, from
the library's HIP events) and on packed-real vectors (the SpMV of qbh_lanczos_real_dev steps), and, measured in the same
process right after, the stored operator's SpMV ms in the default (coded) format and in complex128 (the numbers of
profiles/kondo_time.txt).
chain_L12: chain L = 12 at half filling, S^z = 0 (2,046,924,400 words, 16.4 GB per packed-real vector), matrix-free:
packed-real Lanczos to convergence, then E0 of each of the twelve momentum sectors from the stored csr_mat.kondo_repr, their
minimum, the momentum it lies at and the difference.
chain_L13: chain L = 13 at half filling, S^z = 0 (15,148,345,760 words, 2 x 121 GB packed): the same Lanczos, if the card's
free memory allows (else reported as skipped).
Usage: python tools/kondo_mf_time.py [chain_L10 chain_L12 chain_L13 ...]"""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import quantum_basis_amd as q  # noqa: E402
from quantum_basis_amd import _lib, kondo  # noqa: E402

T_HOP, J_K = 1.0, 1.1


def chain(L):
    return [(i, (i + 1) % L) for i in range(L)]


def chain_group(L, m):
    return [[(s + t) % L for s in range(L)] for t in range(L)], np.exp(-2j * np.pi * m * np.arange(L) / L)


def spmv_ms(A, reps=10):
    """ms per y = H x - 0.3 y on complex vectors, from the handle's HIP events (as tools/kondo_time.py)."""
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


def compare(L=10):
    mk = lambda **kw: q.csr_mat.kondo(L, L, 0, chain(L), t=T_HOP, J_K=J_K, **kw)
    t0 = time.perf_counter()
    M = mk(matrix_free=True, opts=q.make_opts(profile=1))
    M.sync()
    out = {"case": "chain_L%d" % L, "mf_build_ms": round(1e3 * (time.perf_counter() - t0), 1), "dim": int(M.dim), "nnz": int(M.nnz),
           "mf_bytes_tables": int(M.info().bytes_matrix)}
    out["mf_ms_complex"] = round(spmv_ms(M), 3)
    _, _, ms_real, _ = real_lanczos(M, 12, 40)
    out["mf_ms_real"] = round(ms_real, 3)
    # the least traffic of one apply: x once and y once (beta != 0: y twice) -- against 8 TB/s
    out["mf_vector_bytes_real"] = 3 * 8 * int(M.dim)
    M.destroy()
    for fmt, o in (("default", dict(profile=1)), ("complex128", dict(profile=1, value_dict=0, real_fast_path=0))):
        A = mk(opts=q.make_opts(**o))
        assert (A.dim, A.nnz) == (out["dim"], out["nnz"])
        out["stored_bytes_matrix_" + fmt] = int(A.info().bytes_matrix)
        out["stored_ms_" + fmt] = round(spmv_ms(A), 3)
        A.destroy()
    return out


def full_size(L, sectors=True):
    import torch
    maxit = 400
    dim = kondo.sector_dim(L, L, 0)
    out = {"case": "chain_L%d" % L, "dim": int(dim), "vector_bytes_packed": 8 * int(dim)}
    free = torch.cuda.mem_get_info()[0]
    need = 2 * 8 * dim + (1 << 30)                           # the two Lanczos vectors and room for the workspace
    if free < need:
        out.update(skipped="free device memory %d < %d" % (free, need))
        return out
    t0 = time.perf_counter()
    M = q.csr_mat.kondo(L, L, 0, chain(L), t=T_HOP, J_K=J_K, matrix_free=True, opts=q.make_opts(profile=1))
    out.update(mf_build_ms=round(1e3 * (time.perf_counter() - t0), 1), nnz=int(M.nnz), mf_bytes_tables=int(M.info().bytes_matrix))

    def log(m, hess):
        print("# step %d  E0 ~ %.12f" % (m, q.hess_eigen(hess, maxit, m, "sr")[0][0]), flush=True)

    m, hess, ms_spmv, ms_step = real_lanczos(M, maxit - 1, maxit, chunk=20, log=log)
    e_full = float(q.hess_eigen(hess, maxit, m, "sr")[0][0])
    out.update(lanczos_steps=int(m), mf_ms_real=round(ms_spmv, 2), ms_per_step=round(ms_step, 2), E0=e_full)
    M.destroy()
    if sectors:
        E = []
        for k in range(L):
            S = q.csr_mat.kondo_repr(L, L, 0, chain(L), *chain_group(L, k), t=T_HOP, J_K=J_K)
            E.append(float(q.locate_E0_lanczos(S, nev=1, ncv=0).E0))
            print("# k = %d: dim %d E0 = %.10f" % (k, S.dim, E[-1]), flush=True)
            S.destroy()
        out.update(sector_E0_by_k=E, sector_E0_min=min(E), sector_k_of_min=int(np.argmin(E)), E0_minus_sector_min=e_full - min(E))
    return out


def main():
    for name in sys.argv[1:] or ["chain_L10", "chain_L12", "chain_L13"]:
        L = int(name[7:])
        try:
            print(json.dumps(compare(L) if L <= 10 else full_size(L, sectors=L <= 12)), flush=True)
        except q._lib.QbhError as e:                          # e.g. out of memory: reported, the next case still runs
            print(json.dumps({"case": name, "error": str(e)}), flush=True)


if __name__ == "__main__":
    main()
