#!/usr/bin/env python3
"""Times of qbh_corr_hubbard_repr_dev (all-pair correlations of a Hubbard momentum-sector state), HIP events around whole calls on
the null stream, and for scale the only other route to the same numbers: measure_repr_static_hubbard, which assembles a
translation-averaged sector operator per observable, applies it once and destroys it.  That route is timed for ONE site pair of each
kind (an up hop, a down hop, one density product, one spin exchange) and EXTRAPOLATED to all pairs and groups:
    yardstick_all_pairs_ms = N (N - 1) / 2 * (hop_up + hop_dn + 3 * nn + exchange)          (uu, dd and ud per unordered pair; the
diagonal, the second orientation of ud and the imaginary parts of flip, which the exchange operator does not give, are not even
counted).  The figure is printed with "extrapolated": true.

Sizes (each runs in a fresh child process under its own time limit; a size that fails or runs out of time ends the run):
    4x4      4x4 at half filling (8 + 8), k = (0, 0):      1.04e7 representatives     limit 300 s
    4x5_8+8  4x5 with 8 + 8 electrons, k = (pi, 0):        7.93e8 representatives     limit 900 s
    4x5      4x5 at half filling (10 + 10), k = (0, 0):    1.71e9 representatives     limit 1100 s   (34 GB of code bytes during the
             enumeration beside 27 GB of vector; left out with --sizes when memory or time does not allow it)

Per size one JSON line, printed and appended to profiles/corr_hubrepr_time.txt (--out):
  enumerate_ms     the call with only norm2 asked for: the enumeration of the sector, the tables and the site pass
  corr_complex_ms  the full call (norm2, dens, nn, hop, flip) on a complex vector; every call enumerates the sector again, so
                   corr - enumerate is the pass over the representatives
  corr_real_ms     the same on the packed real parts (only at real characters)
  yardstick        the four timed measure_repr_static_hubbard calls with their values beside the one-pass ones (equal up to rounding,
                   plus one constant where the sector has zero-norm rows: the operator's fake diagonal i / dim on them), or the
                   error that ended them (an operator of 1e9 rows may not fit beside the vector)

Usage: python tools/corr_hubrepr_time.py [--sizes 4x4 4x5_8+8 4x5] [--reps 3]"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = {
    # name: (Lx, Ly, n_up, n_dn, k, time limit in seconds)
    "4x4": (4, 4, 8, 8, (0, 0), 300),
    "4x5_8+8": (4, 5, 8, 8, (2, 0), 900),
    "4x5": (4, 5, 10, 10, (0, 0), 1100),
}


def timed(fn):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), out


def corr_call(N, nu, nd, p, c, t, want_all):
    import torch
    from quantum_basis_amd import _lib
    real = t.dtype == torch.float64
    n2, dim = C.c_double(), C.c_int64()
    dens, nn = np.zeros((2, N)), np.zeros((4, N, N))
    hop, flip = np.zeros((2, N, N), dtype=np.complex128), np.zeros((N, N), dtype=np.complex128)
    ptr = (lambda a: a.ctypes.data_as(C.c_void_p)) if want_all else (lambda a: None)
    addr = C.c_void_p(t.data_ptr())
    _lib.check(_lib.lib().qbh_corr_hubbard_repr_dev(N, nu, nd, 0, len(p), p.ctypes.data_as(C.c_void_p), c.ctypes.data_as(C.c_void_p),
                                                    None if real else addr, addr if real else None, C.byref(n2), ptr(dens), ptr(nn),
                                                    ptr(hop), ptr(flip), C.byref(dim), None), "qbh_corr_hubbard_repr_dev")
    return {"norm2": n2.value, "dens": dens, "nn": nn, "hop": hop, "flip": flip, "dim": dim.value}


def median_ms(fn, reps):
    if reps > 1:
        fn()                                                 # warm-up
    ms, out = [], None
    for _ in range(reps):
        t, out = timed(fn)
        ms.append(t)
    return statistics.median(ms), [round(x, 3) for x in ms], out


def one(name, reps, skip_yardstick):
    import torch
    import quantum_basis_amd as q
    from quantum_basis_amd import _lib, lattices
    Lx, Ly, nu, nd, k, _ = SIZES[name]
    N = Lx * Ly
    perms, shifts = lattices.translations(Lx, Ly)
    chars = lattices.characters(shifts, k, (Lx, Ly))
    p = np.ascontiguousarray(perms, dtype=np.int32)
    c = np.ascontiguousarray(chars, dtype=np.complex128)
    real_chars = bool(np.all(c.imag == 0.0))
    out = {"size": name, "n_sites": N, "n_up": nu, "n_dn": nd, "k": list(k), "n_trans": len(p), "real_characters": real_chars, "reps": reps}
    probe = q.csr_mat.hubbard_repr_mf(N, nu, nd, lattices.square(Lx, Ly), perms, chars)      # the dimension is only known after an enumeration
    dim = int(probe.dim)
    probe.destroy()
    out["dim"] = dim
    gen = torch.Generator(device="cuda").manual_seed(1)
    x = torch.randn(dim, 2, dtype=torch.float64, device="cuda", generator=gen)
    x /= torch.linalg.norm(x)
    xc = torch.view_as_complex(x).contiguous()
    torch.cuda.synchronize()
    med, runs, _ = median_ms(lambda: corr_call(N, nu, nd, p, c, xc, False), reps)
    out.update(enumerate_ms=round(med, 3), enumerate_ms_runs=runs)
    print("%s dim %d: enumerate %.1f ms" % (name, dim, med), file=sys.stderr, flush=True)
    med, runs, corr = median_ms(lambda: corr_call(N, nu, nd, p, c, xc, True), reps)
    assert corr["dim"] == dim
    out.update(corr_complex_ms=round(med, 3), corr_complex_ms_runs=runs, norm2=corr["norm2"])
    print("%s correlations, complex: %.1f ms" % (name, med), file=sys.stderr, flush=True)
    if real_chars:
        xr = x[:, 0].contiguous()
        torch.cuda.synchronize()
        med, runs, _ = median_ms(lambda: corr_call(N, nu, nd, p, c, xr, True), reps)
        out.update(corr_real_ms=round(med, 3), corr_real_ms_runs=runs)
        del xr
    if not skip_yardstick:
        i, j = 0, 1
        kinds = [("hop_up", dict(one_body=[(i, j, 1.0, 0.0)]), lambda: corr["hop"][0, i, j]),
                 ("hop_dn", dict(one_body=[(i, j, 0.0, 1.0)]), lambda: corr["hop"][1, i, j]),
                 ("nn_ud", dict(two_body=[(i, j, 0.0, 1.0, 0.0, 0.0)]), lambda: corr["nn"][1, i, j]),
                 ("exchange", dict(spin_exchange=[(i, j, 1.0)]), lambda: corr["flip"][i, j] + corr["flip"][j, i])]
        yard = {}
        try:
            for kind, kw, mine in kinds:
                t, val = timed(lambda: q.measure_repr_static_hubbard(N, nu, nd, perms, chars, C.c_void_p(xc.data_ptr()), **kw))
                # the sector operator keeps the diagonal i / dim on its zero-norm rows (fake_pos = 0), which the random vector does
                # not avoid: where such rows exist, all four values exceed the one-pass ones by the same sum_dead (i / dim) |x_i|^2
                yard[kind] = {"ms": round(t, 3), "value": [val.real, val.imag], "one_pass": [complex(mine()).real, complex(mine()).imag]}
                print("%s yardstick %s: %.1f ms" % (name, kind, t), file=sys.stderr, flush=True)
            pairs = N * (N - 1) // 2
            total = pairs * (yard["hop_up"]["ms"] + yard["hop_dn"]["ms"] + 3 * yard["nn_ud"]["ms"] + yard["exchange"]["ms"])
            out.update(yardstick=yard, yardstick_all_pairs_ms=round(total, 1), extrapolated=True, yardstick_pairs=pairs)
        except _lib.QbhError as e:
            out.update(yardstick=yard, yardstick_error=str(e))
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", nargs="+", default=["4x4", "4x5_8+8", "4x5"], choices=sorted(SIZES))
    ap.add_argument("--reps", type=int, default=3, help="timed runs per call at 4x4; the 4x5 sizes are timed once")
    ap.add_argument("--skip-yardstick", action="store_true")
    ap.add_argument("--one", help=argparse.SUPPRESS)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "corr_hubrepr_time.txt"))
    a = ap.parse_args()
    if a.one:
        one(a.one, a.reps if a.one == "4x4" else 1, a.skip_yardstick)
        return 0
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    for name in a.sizes:
        cmd = [sys.executable, os.path.abspath(__file__), "--one", name, "--reps", str(a.reps)] + (["--skip-yardstick"] if a.skip_yardstick else [])
        try:
            r = subprocess.run(cmd, stdout=subprocess.PIPE, timeout=SIZES[name][5], text=True)
            line = r.stdout.strip().splitlines()[-1] if r.returncode == 0 and r.stdout.strip() else json.dumps({"size": name, "status": "exit %d" % r.returncode})
            ok = r.returncode == 0
        except subprocess.TimeoutExpired:
            line, ok = json.dumps({"size": name, "status": "not finished within %d s" % SIZES[name][5]}), False
        print(line, flush=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")
        if not ok:
            return 1                                         # nothing more is started on the device after a failure
    return 0


if __name__ == "__main__":
    sys.exit(main())
