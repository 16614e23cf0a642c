"""Independent host reference for the all-pair correlations of Kondo-lattice states (qbh_corr_kondo_dev), written from the operator
definitions: every expectation value is a product of one-site operators (the primitives of tests/kondoops.py: fermion,
electron_flip, local_flip, each written from the SOURCE word) applied right to left to the live rows of the vector, the target row
is found by SEARCH among kondo.words (not by a rank formula), and the sum is taken in longdouble / clongdouble.  Nothing here shares
a formula with the kernel: no rank differences, no Hermitian mirror, no diagonal shortcut -- every (i, j) of every array is
computed on its own.  Rows whose amplitude is exactly zero contribute exactly nothing and are skipped, so the cost is proportional
to the nonzero rows of the vector.  tests/test_kondocorrref.py pins it against Jordan-Wigner operators on the full 8^n space.

Also here, because the CPU pins and the GPU test share them: the bound of the comparison and the comparison itself.
All values are raw bilinear forms <psi| O |psi>: nothing is divided by <psi|psi>."""
from functools import lru_cache

import numpy as np

import kondoops as ko

LD, CLD = np.longdouble, np.clongdouble
KEYS = ("norm2", "site", "nn", "zn", "zz", "hop", "ee", "ll", "le")


@lru_cache(maxsize=8)
def sector(n, n_elec, two_sz):
    return ko.Sector(n, n_elec, two_sz)


class Vec:
    """a vector of the sector prepared once for many expectation values: its nonzero rows, their fields and amplitudes"""

    def __init__(self, sec, psi):
        psi = np.asarray(psi)
        assert len(psi) == sec.N
        self.sec = sec
        self.src = np.flatnonzero(psi != 0)
        self.p = psi.astype(CLD)
        self.w2 = (np.abs(self.p[self.src]) ** 2).astype(LD)
        self.u, self.d, self.s = sec.u[self.src], sec.d[self.src], sec.s[self.src]


# one-site operators: ("n", i, species) ("sz", i) ("c", i, species) ("cdag", i, species) ("e+", i) ("e-", i) ("S+", i) ("S-", i)
def expect(v, ops):
    """<psi| O_0 O_1 ... |psi>, O_0 the leftmost factor (the rightmost acts first); the product must return to the sector"""
    sec = v.sec
    idx = np.arange(len(v.src))
    u, d, s = v.u, v.d, v.s
    amp = np.ones(len(idx), dtype=LD)
    moved = False
    for op in reversed(list(ops)):
        kind, i = op[0], op[1]
        if kind == "sz":                                        # +1/2 where the local spin is up (bit clear)
            amp = amp * (LD(0.5) - ((s >> i) & 1).astype(LD))
            continue
        if kind == "n":                                         # c^dag c: the sign of the two factors cancels
            keep = np.flatnonzero((((d if op[2] else u) >> i) & 1) == 1)
            idx, u, d, s, amp = idx[keep], u[keep], d[keep], s[keep], amp[keep]
            continue
        if kind == "c" or kind == "cdag":
            cols, u, d, s, sign = ko.fermion(u, d, s, i, op[2], 1 if kind == "cdag" else 0)
        elif kind == "e+" or kind == "e-":
            cols, u, d, s, sign = ko.electron_flip(u, d, s, i, kind == "e+")
        else:
            assert kind in ("S+", "S-")
            cols, u, d, s, sign = ko.local_flip(u, d, s, i, kind == "S+")
        idx, amp = idx[cols], amp[cols] * np.asarray(sign).astype(LD)
        moved = True
    if len(idx) == 0:
        return CLD(0)
    if not moved:
        return CLD(np.sum(amp * v.w2[idx]))
    new = u | (d << sec.n) | (s << (2 * sec.n))
    tgt = np.minimum(np.searchsorted(sec.w, new), sec.N - 1)
    assert np.array_equal(sec.w[tgt], new), "the product leaves the sector"
    return np.sum(np.conj(v.p[tgt]) * amp * v.p[v.src[idx]])


def correlations(n, n_elec, two_sz, psi, keys=KEYS):
    """the arrays of qbh_corr_kondo_dev in longdouble: dict(norm2, site[4][N], nn[4][N][N], zn[2][N][N], zz, hop[2][N][N], ee, ll, le)"""
    v = Vec(sector(n, n_elec, two_sz), psi)
    out = {"norm2": LD(np.sum(v.w2))}
    R = range(n)
    if "site" in keys:
        out["site"] = np.array([[expect(v, [("n", i, 0)]).real for i in R], [expect(v, [("n", i, 1)]).real for i in R],
                                [expect(v, [("n", i, 0), ("n", i, 1)]).real for i in R], [expect(v, [("sz", i)]).real for i in R]], dtype=LD)
    if "nn" in keys:
        out["nn"] = np.array([[[expect(v, [("n", i, a), ("n", j, b)]).real for j in R] for i in R] for a in (0, 1) for b in (0, 1)], dtype=LD)
    if "zn" in keys:
        out["zn"] = np.array([[[expect(v, [("sz", i), ("n", j, sp)]).real for j in R] for i in R] for sp in (0, 1)], dtype=LD)
    if "zz" in keys:
        out["zz"] = np.array([[expect(v, [("sz", i), ("sz", j)]).real for j in R] for i in R], dtype=LD)
    if "hop" in keys:
        out["hop"] = np.array([[[expect(v, [("cdag", i, sp), ("c", j, sp)]) for j in R] for i in R] for sp in (0, 1)], dtype=CLD)
    if "ee" in keys:
        out["ee"] = np.array([[expect(v, [("e+", i), ("e-", j)]) for j in R] for i in R], dtype=CLD)
    if "ll" in keys:
        out["ll"] = np.array([[expect(v, [("S+", i), ("S-", j)]) for j in R] for i in R], dtype=CLD)
    if "le" in keys:
        out["le"] = np.array([[expect(v, [("S+", i), ("e-", j)]) for j in R] for i in R], dtype=CLD)
    return out


# ------------------------------------------------------------------------------------------------------- comparison --
def bound(rows, norm2):
    """|got - want| <= 4 (rows + 4) 2^-53 norm2: an entry is a sum of at most `rows` products whose moduli sum to at most norm2
    (Cauchy-Schwarz for the gathered ones; every matrix element is +-1 or +-1/2, no table weight enters), each a complex
    product (the factor 4), summed in any order."""
    return 4.0 * (rows + 4) * 2.0 ** -53 * float(norm2)


def compare(label, got, ref, rows, keys=None):
    """every entry of every array within `bound`; entries (and real / imaginary parts) that must vanish exactly, exactly.
    Prints the worst ratio per array and returns them."""
    keys = [k for k in KEYS if k in ref] if keys is None else keys
    tol = bound(rows, ref["norm2"])
    worst, arrays = {}, {}
    for k in keys:
        w = np.asarray(ref[k])
        g = np.asarray(got[k]).reshape(w.shape)
        arrays[k] = (g, w)
        err = float(np.max(np.abs(g.astype(w.dtype) - w))) if w.size else 0.0
        worst[k] = err / tol if tol > 0 else (0.0 if err == 0 else np.inf)
    print("%s rows %d: worst |got - want| / bound  %s" % (label, rows, "  ".join("%s %.3g" % kv for kv in worst.items())))
    for k in keys:
        g, w = arrays[k]
        assert worst[k] <= 1.0, (label, k, worst[k])
        assert np.all(g[w == 0] == 0), (label, k, "an entry that must vanish exactly does not")
        if np.iscomplexobj(w):
            assert np.all(g.real[w.real == 0] == 0) and np.all(g.imag[w.imag == 0] == 0), (label, k)
    return worst
