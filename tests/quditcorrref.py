"""Independent host reference for the all-pair correlations of d-level states (qbh_corr_qudit_dev), written from the operator
definitions: a local operator is a d x d matrix with at most one nonzero per column, it changes the level of its site in the words
of quditforms.words, the target row is found by SEARCH among the packed words (not by the rank formula), and every expectation
value is summed in longdouble / clongdouble.  Nothing here shares a formula with the kernel (no running products, no rank
differences, no pop shortcut for the diagonals); tests/test_quditcorrref.py pins it against np.kron operators restricted to the
sector.  Rows whose amplitude is exactly zero contribute exactly nothing and are skipped, which keeps a sparse vector in a large
sector cheap.

Also here, because the CPU pins and the GPU test share them: the bound of the comparison and the comparison itself.
All values are raw bilinear forms <psi| O |psi>: nothing is divided by <psi|psi>."""
import numpy as np

import quditforms as qf

LD, CLD = np.longdouble, np.clongdouble
U64 = np.uint64


class Sector:
    def __init__(self, n, d, total):
        self.n, self.d, self.total = n, d, total
        self.levels, self.keys = qf.words(n, d, total)
        self.bits = qf.bits_per_level(d)
        self.dim = len(self.keys)


class Vec:
    """a vector of the sector prepared once for many expectation values: its nonzero rows and their amplitudes in clongdouble"""

    def __init__(self, sec, psi):
        psi = np.asarray(psi)
        assert len(psi) == sec.dim
        self.src = np.flatnonzero(psi != 0)
        self.p = psi.astype(CLD)
        self.w2 = (np.abs(self.p[self.src]) ** 2).astype(LD)                               # |psi|^2 of the live rows
        self.levels = np.ascontiguousarray(sec.levels[self.src].T).astype(np.int64)      # [site][live row]
        self.keys = sec.keys[self.src]


class Op:
    """a local operator prepared once: M[l', l] = <l'|O|l> with at most one nonzero per column -> the level it sends l to (-1:
    nowhere) and the matrix element"""

    def __init__(self, M):
        M = np.asarray(M)
        d = len(M)
        self.tgt = np.full(d, -1, dtype=np.int64)
        self.val = np.zeros(d, dtype=LD)
        for l in range(d):
            nz = np.flatnonzero(M[:, l] != 0)
            assert len(nz) <= 1
            if len(nz):
                self.tgt[l], self.val[l] = nz[0], LD(M[nz[0], l])
        self.diagonal = bool(np.all((self.tgt < 0) | (self.tgt == np.arange(d))))


def lowering(lower):
    """the matrix of A: <l-1| A |l> = lower[l], lower[0] ignored"""
    d = len(lower)
    M = np.zeros((d, d))
    for l in range(1, d):
        M[l - 1, l] = lower[l]
    return M


def expect(sec, psi, ops):
    """<psi| O_0 O_1 ... |psi> for ops = [(site, M), ...], O_0 the leftmost factor (the rightmost acts first); M[l', l] = <l'|O|l>
    with at most one nonzero per column; the product must return to the sector."""
    v = psi if isinstance(psi, Vec) else Vec(sec, psi)
    src = v.src
    if len(src) == 0:
        return CLD(0)
    cur = {}                                                    # site -> current levels of the live rows
    key = v.keys.copy()
    amp = np.ones(len(src), dtype=LD)
    alive = np.ones(len(src), dtype=bool)
    moved = False
    for site, M in reversed(list(ops)):
        op = M if isinstance(M, Op) else Op(M)
        old = cur.get(site, v.levels[site])
        amp = amp * op.val[old]
        if op.diagonal:                                         # a matrix element of 0 removes the row through its amplitude
            continue
        new = op.tgt[old]
        alive &= new >= 0
        new = np.where(new >= 0, new, old)
        moved = True
        sh = U64(site * sec.bits)
        key = key ^ (old.astype(U64) << sh) ^ (new.astype(U64) << sh)
        cur[site] = new
    if not alive.any():
        return CLD(0)
    if moved:
        idx = np.searchsorted(sec.keys, key)
        idx = np.where(alive & (idx < sec.dim), idx, 0)
        assert np.all(sec.keys[idx[alive]] == key[alive]), "the product leaves the sector"
    else:
        return CLD(np.sum(amp * v.w2))                          # a diagonal product: sum |psi|^2 (product of the matrix elements)
    p, a = v.p, alive
    return np.sum(np.conj(p[idx[a]]) * amp[a] * p[src[a]])


def string_ops(h, g, i, j, last=None):
    """h at i, g on the sites strictly between, h at j (i < j); last: where the g's stop (the fault 'one site too far' sets j + 1)"""
    last = j if last is None else last
    H, Gm = (h if isinstance(h, Op) else Op(np.diag(h))), (g if isinstance(g, Op) else Op(np.diag(g)))
    return [(i, H)] + [(k, Gm) for k in range(i + 1, last)] + [(j, H)]


def correlations(n, d, total, psi, diag=None, string=None, lower=None):
    """dict(norm2, pop[N][d], dd[K][K][N][N], str[N][N], aa[N][N]) of a vector of the sector, for the tables that are given"""
    sec = Sector(n, d, total)
    psi = Vec(sec, psi)
    out = {"norm2": np.sum(np.abs(psi.p) ** 2).real.astype(LD), "pop": np.zeros((n, d), dtype=LD)}
    for s in range(n):
        for l in range(d):
            e = np.zeros(d)
            e[l] = 1.0
            out["pop"][s, l] = expect(sec, psi, [(s, np.diag(e))]).real
    if diag is not None:
        f = [Op(np.diag(t)) for t in np.asarray(diag, dtype=np.float64).reshape(-1, d)]
        K = len(f)
        out["dd"] = np.zeros((K, K, n, n), dtype=LD)
        for a in range(K):
            for b in range(K):
                for i in range(n):
                    for j in range(n):
                        out["dd"][a, b, i, j] = expect(sec, psi, [(i, f[a]), (j, f[b])]).real
    if string is not None:
        h, g = (Op(np.diag(np.asarray(t, dtype=np.float64))) for t in string)
        out["str"] = np.zeros((n, n), dtype=LD)
        for i in range(n):
            out["str"][i, i] = expect(sec, psi, [(i, h), (i, h)]).real
            for j in range(i + 1, n):
                out["str"][i, j] = out["str"][j, i] = expect(sec, psi, string_ops(h, g, i, j)).real
    if lower is not None:
        A = lowering(np.asarray(lower, dtype=np.float64))
        A, At = Op(A), Op(A.T)
        out["aa"] = np.zeros((n, n), dtype=CLD)
        for i in range(n):
            for j in range(n):
                out["aa"][i, j] = expect(sec, psi, [(i, A), (j, At)])
    return out


# ------------------------------------------------------------------------------------------------------- comparison --
def weights(n, diag=None, string=None, lower=None):
    """W per array: the largest modulus a weight of that array can take, from the tables"""
    W = {"norm2": 1.0, "pop": 1.0}
    if diag is not None:
        W["dd"] = float(np.max(np.abs(diag))) ** 2
    if string is not None:
        h, g = (float(np.max(np.abs(t))) for t in string)
        W["str"] = h * h * max(1.0, g) ** max(n - 2, 0)
    if lower is not None:
        W["aa"] = float(np.max(np.abs(np.asarray(lower)[1:]))) ** 2
    return W


def bound(dim, n_sites, norm2, W):
    """|got - want| <= 4 (dim + n_sites + 4) 2^-53 norm2 W: an entry is a sum of at most dim terms whose moduli sum to at most
    W norm2 (Cauchy-Schwarz for the gathered ones), each term a product of up to n_sites table values (the n_sites term) times a
    complex product (the factor 4), summed in any order."""
    return 4.0 * (dim + n_sites + 4) * 2.0 ** -53 * float(norm2) * W


def compare(label, got, ref, dim, n_sites, W, keys=None):
    """every entry of every array within `bound`; entries (and real / imaginary parts) that must vanish exactly, exactly.
    Prints the worst ratio per array and returns them."""
    keys = [k for k in ("norm2", "pop", "dd", "str", "aa") if k in ref] if keys is None else keys
    worst = {}
    arrays = {}
    for k in keys:
        w = np.asarray(ref[k])
        g = np.asarray(got[k]).reshape(w.shape)
        arrays[k] = (g, w)
        tol = bound(dim, n_sites, ref["norm2"], W[k])
        err = np.abs(g.astype(w.dtype) - w).astype(np.float64)
        worst[k] = float(err.max() / tol) if tol > 0 else (0.0 if err.max() == 0 else np.inf)
    print("%s dim %d: worst |got - want| / bound  %s" % (label, dim, "  ".join("%s %.3g" % kv for kv in worst.items())))
    for k in keys:
        g, w = arrays[k]
        assert worst[k] <= 1.0, (label, k, worst[k])
        assert np.all(g[w == 0] == 0), (label, k, "an entry that must vanish exactly does not")
        if np.iscomplexobj(w):
            assert np.all(g.real[w.real == 0] == 0) and np.all(g.imag[w.imag == 0] == 0), (label, k)
    return worst
