#!/usr/bin/env python3
"""Whole-call time of the six operators between momentum sectors (qbh_sector_mopr.hip).

Cases (by name):
  c_hubrepr       c_{q,up} from the Hubbard 4x4 half-filling k = (0,0) sector to the (7, 8) sector at q = (1, 0)
  diag_hubrepr    N_q in the same k = (0,0) sector, to k = (1, 0)
  sz_repr         S^z_q in the 24-site spin ring, n_dn = 12, k = 0 -> 1
  flip_repr       S^+_q in the same ring, n_dn 12 -> 11, k = 0 -> 1
  qudit_repr      S^-_q in the spin-1 chain L = 12, S^z = 0 -> -1, k = 0 -> pi
  diag_kondo_repr the local-spin S^z_q in the Kondo chain L = 10, n_elec = 10, S^z = 0, k = 0 -> 1
The entry points return after their own synchronise and expose neither their enumeration nor their kernel, so the time is the
wall time of the whole call on a random source vector: one warm-up, then three repeats.  The stream of
qbh_mopr_qudit_repr_dev does not help: the enumeration of both sectors runs inside the same call, before the kernel, and
ends with a device synchronise, so events recorded outside bracket the whole call there too.  One JSON line per case with the three
times in ms, their median and spread (max - min) and the two dimensions; the lines also go to --out (default: stdout only),
under the command that made them.
Usage: python tools/sector_mopr_time.py [--out FILE] [case ...]"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import quantum_basis_amd as q  # noqa: E402
from quantum_basis_amd import lattices, qudit  # noqa: E402


def ring(L, m):
    return [[(s + t) % L for s in range(L)] for t in range(L)], np.exp(-2j * np.pi * m * np.arange(L) / L)


def plane_wave(L, m):
    return np.exp(2j * np.pi * m * np.arange(L) / L) / np.sqrt(L)


def hubbard_4x4(qv):
    perms, shifts = lattices.translations(4, 4)
    coef = np.array([np.exp(-2j * np.pi * (qv[0] * (s % 4) + qv[1] * (s // 4)) / 4) for s in range(16)]) / 4.0
    return perms, lattices.characters(shifts, (0, 0), (4, 4)), lattices.characters(shifts, qv, (4, 4)), coef


def c_hubrepr(x, y):
    perms, ch0, chq, coef = hubbard_4x4((1, 0))
    return q.moprXvec_c_hubrepr(16, 8, 8, 0, -1, perms, ch0, chq, coef, x, y)


def diag_hubrepr(x, y):
    perms, ch0, chq, coef = hubbard_4x4((1, 0))
    d = q.moprXvec_diag_hubrepr(16, 8, 8, perms, chq, coef, coef, x, y)
    return d, d


def sz_repr(x, y):
    perms, ch1 = ring(24, 1)
    d = q.moprXvec_sz_repr(24, 12, perms, ch1, plane_wave(24, 1), x, y)
    return d, d


def flip_repr(x, y):
    perms, ch0 = ring(24, 0)
    return q.moprXvec_flip_repr(24, 12, +1, perms, ch0, ring(24, 1)[1], plane_wave(24, 1), x, y)


def qudit_repr(x, y):
    perms, ch0 = ring(12, 0)
    return q.moprXvec_qudit_repr(12, 3, 12, 1, perms, ch0, plane_wave(12, 6), qudit.spin_matrices(1)[2], x, y)


def diag_kondo_repr(x, y):
    perms, ch1 = ring(10, 1)
    zero = np.zeros(10)
    d = q.moprXvec_diag_kondo_repr(10, 10, 0, perms, ch1, zero, zero, plane_wave(10, 1), x, y)
    return d, d


# name -> (call, an upper bound of the dimensions of both sectors)
CASES = {"c_hubrepr": (c_hubrepr, 10353252), "diag_hubrepr": (diag_hubrepr, 10353252), "sz_repr": (sz_repr, 200000),
         "flip_repr": (flip_repr, 200000), "qudit_repr": (qudit_repr, 73789), "diag_kondo_repr": (diag_kondo_repr, 4000000)}


def run(name, handle, repeats=3):
    call, cap = CASES[name]
    x, y = q.DeviceVec(handle, cap), q.DeviceVec(handle, cap)
    try:
        rng = np.random.default_rng(1)
        x.upload(rng.standard_normal(cap) + 1j * rng.standard_normal(cap))
        dims = call(x.ptr, y.ptr)                               # warm-up
        assert max(dims) <= cap, (dims, cap)
        ms = []
        for _ in range(repeats):
            t0 = time.perf_counter()
            call(x.ptr, y.ptr)
            ms.append(1e3 * (time.perf_counter() - t0))
    finally:
        x.free()
        y.free()
    return {"case": name, "dim_old": int(dims[0]), "dim_new": int(dims[1]), "call_ms": [round(t, 2) for t in ms],
            "median_ms": round(float(np.median(ms)), 2), "spread_ms": round(max(ms) - min(ms), 2)}


def main():
    args = sys.argv[1:]
    path = None
    if args[:1] == ["--out"]:
        path, args = args[1], args[2:]
    lines = ["# python tools/sector_mopr_time.py " + " ".join(args)]
    handle = q.csr_mat.heisenberg(4, 2, lattices.chain(4))      # only a handle for device vectors
    for name in args or list(CASES):
        try:
            line = json.dumps(run(name, handle))
        except q._lib.QbhError as e:                            # reported, the next case still runs
            line = json.dumps({"case": name, "error": str(e)})
        print(line, flush=True)
        lines.append(line)
        if path:
            with open(path, "w") as f:                          # after every case: a later failure keeps what was measured
                f.write("\n".join(lines) + "\n")
    handle.destroy()


if __name__ == "__main__":
    main()
