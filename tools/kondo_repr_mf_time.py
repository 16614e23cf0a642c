#!/usr/bin/env python3
"""Build time and time per apply of the matrix-free Kondo momentum sector (qbh_mf_kondo_repr) beside the stored sector of
qbh_gen_kondo_repr, in one process.  The chain at half filling (n_elec = L, S^z = 0, t = 1, J_K = 1.1):

  L12_k0, L12_kpi   L = 12, k = 0 / pi: build ms (wall: host tables, enumeration, the count pass, adoption), bytes held, ms per
                    apply on complex vectors and on packed-real vectors (Lanczos form y = H x - 0.3 y with both reductions,
                    HIP events), the stored operator's coded SpMV beside them, and E0 from the packed-real Lanczos run of the
                    matrix-free handle against E0 from the stored operator
  L13_k0_mf         L = 13, k = 0, matrix-free only (1.17e9 representatives; the stored form does not fit): the same times

A case is L<sites>_k0 or L<sites>_kpi, with _mf for the matrix-free handle alone.  One JSON line per measurement.
Usage: python tools/kondo_repr_mf_time.py [L12_k0 L12_kpi L13_k0_mf]"""
import ctypes as C
import json
import os
import re
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


def build(L, m, matrix_free, **fmt):
    t0 = time.perf_counter()
    A = q.csr_mat.kondo_repr(L, L, 0, chain(L), *chain_group(L, m), t=1.0, J_K=1.1, opts=q.make_opts(profile=1, **fmt),
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


def run(name, L, m, with_stored):
    M, build_ms = build(L, m, True)
    i = M.info()
    out = {"case": name, "form": "matrix_free", "build_ms": round(build_ms, 1), "dim": int(M.dim), "contributions": int(M.nnz),
           "bytes_matrix": int(i.bytes_matrix)}
    Mc, _ = build(L, m, True, real_fast_path=0)
    out["apply_ms_complex"] = round(apply_ms(Mc), 3)
    Mc.destroy()
    E0, steps, sec, ms = lanczos_real(M)
    out.update(apply_ms_packed_real=round(ms, 3), lanczos_steps=steps, lanczos_s=round(sec, 2), E0=E0, E0_per_site=E0 / L)
    M.destroy()
    if not with_stored:
        print(json.dumps(out), flush=True)
        return
    A, build_ms = build(L, m, False)
    E0s = float(q.locate_E0_lanczos(A, nev=1, ncv=0, maxit=300).E0)
    out["E0_error_vs_stored"] = abs(E0 - E0s)
    print(json.dumps(out), flush=True)
    print(json.dumps({"case": name, "form": "stored_coded", "build_ms": round(build_ms, 1), "dim": int(A.dim), "nnz": int(A.nnz),
                      "bytes_matrix": int(A.info().bytes_matrix), "spmv_ms": round(apply_ms(A, 10), 3), "E0": E0s}), flush=True)
    A.destroy()
    assert out["E0_error_vs_stored"] < 1e-8, out


def main():
    for name in sys.argv[1:] or ["L12_k0", "L12_kpi", "L13_k0_mf"]:
        g = re.fullmatch(r"L(\d+)_k(0|pi)(_mf)?", name)
        if not g or (g.group(2) == "pi" and int(g.group(1)) % 2):
            sys.exit("unknown case %r: L<sites>_k0 or L<even sites>_kpi, with _mf for the matrix-free handle alone" % name)
        L = int(g.group(1))
        try:
            run(name, L, 0 if g.group(2) == "0" else L // 2, g.group(3) is None)
        except _lib.QbhError as e:                            # e.g. out of memory: reported, the next case still runs
            print(json.dumps({"case": name, "error": str(e)}), flush=True)


if __name__ == "__main__":
    main()
