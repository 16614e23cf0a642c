#!/usr/bin/env python3
"""Times of qbh_corr_qudit_repr_dev (all-pair correlations and string order of a d-level momentum-sector state) for the spin-1 ring
at S^z = 0, k = 0 on the packed real vector, HIP events around whole calls on the null stream, and for scale one apply of
qbh_mf_qudit_repr for the operator with a Heisenberg bond on EVERY pair of sites: it canonicalises the same kind of moved words,
issues a comparable number of gathers per row, and was the only route to the pair part before this call (one translation-averaged
sector operator per class and kind would have to be applied; the string correlator has no such route at all).

Printed, and appended to profiles/corr_qudit_repr_time.txt (--out), one JSON line per L:
  enumerate_ms      the call with only norm2 and pop asked for: the enumeration of the sector, the tables and the site passes
  corr_real_ms      the full call (norm2, pop, dd with S^z, the den Nijs-Rommelse string, aa with S^+) on the packed real vector,
                    median of --reps runs after one warm-up; every call enumerates the sector again
  corr_gathers_per_row   the forward orientations (p, q) of all pair classes with l_p >= 1 and l_q <= 1, averaged over the words of
                    the sector (counted exactly on the host; the representatives are a fair sample of the words)
  mf_build_ms       creation of the matrix-free all-pairs operator (enumeration and one counting walk)
  mf_apply_ms       one y = H x of it (median of --reps after one warm-up) on complex vectors: the operator is real, so the handle's
                    real fast path applies it to the packed parts
  mf_gathers_per_row     its off-diagonal contributions per row, from the handle's count
  string_0_half, ss_0_1  two values of the measured state, a fixed random vector (nothing is solved here)

Usage: python tools/corr_qudit_repr_time.py 18 20 [--reps 3] [--out FILE]"""
import argparse
import itertools
import json
import os
import statistics
import sys


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import quantum_basis_amd as q  # noqa: E402
from quantum_basis_amd import lattices  # noqa: E402


def timed(fn):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), out


def median_ms(fn, reps):
    fn()                                                     # warm-up
    ms, out = [], None
    for _ in range(reps):
        t, out = timed(fn)
        ms.append(t)
    return statistics.median(ms), [round(x, 3) for x in ms], out


def words_with(n, d, total, fixed):
    """the words of n sites with d levels and charge `total` whose first len(fixed) sites hold the given levels"""
    rest, q_left = n - len(fixed), total - sum(fixed)
    cnt = [1] + [0] * max(q_left, 0)
    for _ in range(rest):
        cnt = [sum(cnt[c - l] for l in range(d) if c - l >= 0) for c in range(len(cnt))]
    return cnt[q_left] if 0 <= q_left < len(cnt) else 0


def corr_gathers_per_row(L):
    """a ring under its L rotations: L / 2 - 1 classes with L forward ordered pairs each and the class r = L / 2, its own mirror, with
    both orientations of its L / 2 pairs; an orientation gathers when the first site can go down and the second up"""
    forward = L * (L // 2 - 1) + L if L % 2 == 0 else L * (L // 2)
    hit = sum(words_with(L, 3, L, (lp, lq)) for lp in (1, 2) for lq in (0, 1))
    return forward * hit / words_with(L, 3, L, ())


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("L", type=int, nargs="+")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "corr_qudit_repr_time.txt"))
    a = ap.parse_args()
    for L in a.L:
        perms, shifts = lattices.translations(L)
        chars = lattices.characters(shifts, (0, 0), (L, 1))
        out = {"case": "spin1_ring_sz0_k0", "L": L, "n_trans": len(perms), "reps": a.reps, "vector": "packed real"}
        pairs = list(itertools.combinations(range(L), 2))
        t_build, M = timed(lambda: q.csr_mat.spin_heisenberg_repr(L, 1, 0, pairs, perms, chars, matrix_free=True))
        M.sync()
        dim = int(M.dim)
        out.update(dim=dim, mf_build_ms=round(t_build, 3), mf_gathers_per_row=round((int(M.nnz) - dim) / dim, 2))
        v = M.vec(2)
        M.randomize(v.at(0), 1)
        M.randomize(v.at(dim), 2)

        def apply():
            M.spmv(v.at(0), v.at(dim))
            M.sync()

        med, runs, _ = median_ms(apply, a.reps)
        out.update(mf_apply_ms=round(med, 3), mf_apply_ms_runs=runs)
        print("L %d dim %d: all-pairs operator built in %.1f ms, applied in %.1f ms" % (L, dim, t_build, med), file=sys.stderr, flush=True)
        v.free()
        M.destroy()
        x = torch.randn(dim, dtype=torch.float64, device="cuda", generator=torch.Generator(device="cuda").manual_seed(1))
        x /= torch.linalg.norm(x)
        torch.cuda.synchronize()

        med, runs, part = median_ms(lambda: q.qudit_repr_correlations(L, 3, L, perms, chars, x, real=True, normalize=False), a.reps)
        assert part["dim"] == dim
        out.update(enumerate_ms=round(med, 3), enumerate_ms_runs=runs)
        print("enumeration and site passes: %.1f ms" % med, file=sys.stderr, flush=True)
        med, runs, c = median_ms(lambda: q.spin_s_repr_correlations(L, 1, 0, perms, chars, x, real=True, normalize=False), a.reps)
        out.update(corr_real_ms=round(med, 3), corr_real_ms_runs=runs, corr_gathers_per_row=round(corr_gathers_per_row(L), 2),
                   norm2=c["norm2"], string_0_half=float(c["string"][0, L // 2]), ss_0_1=float(c["ss"][0, 1]))
        print("correlations, packed real: %.1f ms" % med, file=sys.stderr, flush=True)
        line = json.dumps(out)
        print(line, flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
