#!/usr/bin/env python3
"""Times of qbh_corr_spin_repr_dev (all-pair correlations of a spin-1/2 momentum-sector state) in one process, HIP events around
whole calls on the null stream, and for scale the only other route to the same numbers: the sector operator of
qbh_gen_heisenberg_repr with ALL N (N - 1) / 2 site pairs as bonds (it canonicalises the same flipped words), built and applied
once.  A sector operator holds at most 159 distinct bonds, so the pairs are split into batches of --batch bonds, one operator each,
built, applied and destroyed one after the other; with --max-batches fewer are measured and the total is the measured mean per
bond times the number of pairs, printed as `extrapolated`.

Printed, and appended to profiles/corr_repr_time.txt (--out), one JSON line:
  enumerate_ms     the call with only norm2 asked for: the enumeration of the sector, the tables and one pass without gathers
  corr_complex_ms  the full call (norm2, sz, zz, pm) on a complex vector, median of --reps runs after one warm-up; every call
                   enumerates the sector again, so corr - enumerate is the pass over the representatives
  corr_real_ms     the same on the packed real parts (only at real characters)
  yardstick        per batch: bonds, nnz, build_ms (enumeration + assembly), apply_ms (one y = H x after a warm-up)
  energy           sum over all pairs of (zz + Re pm) beside <x| H x> summed over the batches (all batches measured only; the two
                   agree where no representative has zero norm: the operator adds fake_pos |x|^2 on those rows)

Usage: python tools/corr_repr_time.py chain 24 --ndn 12 --k 0
       python tools/corr_repr_time.py triangular 6 5 --ndn 15 --k 0 0 [--batch 159] [--max-batches 1]"""
import argparse
import ctypes as C
import itertools
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import quantum_basis_amd as q  # noqa: E402
from quantum_basis_amd import _lib, lattices  # noqa: E402


def symmetry(lattice, size, k):
    if lattice == "chain":
        (L,) = size
        perms, shifts = lattices.translations(L)
        return L, perms, lattices.characters(shifts, (k[0], 0), (L, 1))
    Lx, Ly = size
    n_sub = 3 if lattice == "kagome" else 1
    perms, shifts = lattices.translations(Lx, Ly, n_sub)
    return Lx * Ly * n_sub, perms, lattices.characters(shifts, k, (Lx, Ly))


def timed(fn):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), out


def corr_call(N, n_dn, p, c, t, want_all):
    import torch
    real = t.dtype == torch.float64
    n2, dim = C.c_double(), C.c_int64()
    sz, zz, pm = np.zeros(N), np.zeros((N, N)), np.zeros((N, N), dtype=np.complex128)
    ptr = (lambda a: a.ctypes.data_as(C.c_void_p)) if want_all else (lambda a: None)
    addr = C.c_void_p(t.data_ptr())
    _lib.check(_lib.lib().qbh_corr_spin_repr_dev(N, n_dn, len(p), p.ctypes.data_as(C.c_void_p), c.ctypes.data_as(C.c_void_p),
                                                 None if real else addr, addr if real else None, C.byref(n2), ptr(sz), ptr(zz), ptr(pm),
                                                 C.byref(dim), None), "qbh_corr_spin_repr_dev")
    return {"norm2": n2.value, "sz": sz, "zz": zz, "pm": pm, "dim": dim.value}


def median_ms(fn, reps):
    fn()                                                     # warm-up
    ms, out = [], None
    for _ in range(reps):
        t, out = timed(fn)
        ms.append(t)
    return statistics.median(ms), [round(x, 3) for x in ms], out


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("lattice", choices=["chain", "triangular", "kagome"])
    ap.add_argument("size", type=int, nargs="+")
    ap.add_argument("--ndn", type=int, required=True)
    ap.add_argument("--k", type=int, nargs="+", default=[0, 0])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--batch", type=int, default=159)
    ap.add_argument("--max-batches", type=int, default=0, help="0: all")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "corr_repr_time.txt"))
    a = ap.parse_args()
    k = (a.k + [0])[:2]
    N, perms, chars = symmetry(a.lattice, a.size, k)
    p = np.ascontiguousarray(perms, dtype=np.int32)
    c = np.ascontiguousarray(chars, dtype=np.complex128)
    real_chars = bool(np.all(c.imag == 0.0))
    pairs = list(itertools.combinations(range(N), 2))
    batches = [pairs[i:i + a.batch] for i in range(0, len(pairs), a.batch)]
    out = {"lattice": a.lattice, "size": a.size, "n_sites": N, "n_dn": a.ndn, "k": k, "n_trans": len(p), "real_characters": real_chars,
           "reps": a.reps}

    probe = q.csr_mat.heisenberg_repr(N, a.ndn, pairs[:1], perms, chars)      # the dimension is only known after an enumeration
    dim = int(probe.dim)
    probe.destroy()
    out["dim"] = dim
    gen = torch.Generator(device="cuda").manual_seed(1)
    x = torch.randn(dim, 2, dtype=torch.float64, device="cuda", generator=gen)
    x /= torch.linalg.norm(x)
    xc = torch.view_as_complex(x).contiguous()
    xr = x[:, 0].contiguous()
    torch.cuda.synchronize()

    med, runs, _ = median_ms(lambda: corr_call(N, a.ndn, p, c, xc, False), a.reps)
    out.update(enumerate_ms=round(med, 3), enumerate_ms_runs=runs)
    print("dim %d: enumerate %.1f ms" % (dim, med), file=sys.stderr, flush=True)
    med, runs, corr = median_ms(lambda: corr_call(N, a.ndn, p, c, xc, True), a.reps)
    out.update(corr_complex_ms=round(med, 3), corr_complex_ms_runs=runs, norm2=corr["norm2"],
               gathers_per_row=a.ndn * (N - a.ndn))
    assert corr["dim"] == dim
    print("correlations, complex: %.1f ms" % med, file=sys.stderr, flush=True)
    if real_chars:
        med, runs, _ = median_ms(lambda: corr_call(N, a.ndn, p, c, xr, True), a.reps)
        out.update(corr_real_ms=round(med, 3), corr_real_ms_runs=runs)

    n_meas = len(batches) if a.max_batches <= 0 else min(a.max_batches, len(batches))
    yard, bonds_done, build_sum, apply_sum, e_op = [], 0, 0.0, 0.0, 0.0
    for bi in range(n_meas):
        bonds = batches[bi]
        t_build, H = timed(lambda: q.csr_mat.heisenberg_repr(N, a.ndn, bonds, perms, chars))
        assert int(H.dim) == dim
        v = H.vec(2)
        v.upload(xc.cpu().numpy())
        H.spmv(v.at(0), v.at(dim))
        H.sync()
        t_apply, _ = timed(lambda: (H.spmv(v.at(0), v.at(dim)), H.sync()))
        e_op += H.dotc(v.at(0), v.at(dim)).real              # the row formula is linear in the bonds: the batches add up to the all-pairs operator
        yard.append({"bonds": len(bonds), "nnz": int(H.info().nnz), "build_ms": round(t_build, 3), "apply_ms": round(t_apply, 3)})
        bonds_done += len(bonds)
        print("yardstick batch %d: %s" % (bi, yard[-1]), file=sys.stderr, flush=True)
        build_sum += t_build
        apply_sum += t_apply
        v.free()
        H.destroy()
    scale = len(pairs) / bonds_done
    out.update(yardstick=yard, yardstick_pairs=len(pairs), yardstick_bonds_measured=bonds_done,
               yardstick_build_ms=round(build_sum * scale, 3), yardstick_apply_ms=round(apply_sum * scale, 3),
               yardstick_extrapolated=bonds_done < len(pairs))
    if bonds_done == len(pairs):                             # equal where no representative has zero norm (the operator adds fake_pos |x|^2 there)
        b = np.asarray(pairs)
        out.update(energy_from_correlations=float(np.sum(corr["zz"][b[:, 0], b[:, 1]] + corr["pm"][b[:, 0], b[:, 1]].real)),
                   energy_all_pairs_operator=e_op)
    line = json.dumps(out)
    print(line, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
