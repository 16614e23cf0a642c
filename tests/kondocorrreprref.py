"""Independent host reference for the all-pair static correlations of a Kondo-lattice MOMENTUM-SECTOR state
(qbh_corr_kondo_repr_dev), in numpy longdouble, written from the formulas of the call with their sums over the group elements g left
in place: no pair classes, no Hermitian mirror, no site orbits, no diagonal shortcut -- the diagonal entries of hop, ee, ll and le go
through the same code as every other (i, j).  tests/test_kondocorrreprref.py pins it against the explicit route: unfold the state
with kondoops.Momentum.expand and evaluate the operator definitions of tests/kondocorrref.py on the full state.

Conventions (those of qbh_gen_kondo_repr): word = u | d << n | s << 2n (s: local spin DOWN), operator order "all up (ascending
site), then all down", the local spins commute with everything; G = the n_trans site permutations perms[g][site]; T_g moves all
three fields, sigma(g) = the sorting parity of the two electron fields, none from s (kondoops.translate); the basis is ALL orbit
representatives, ascending; a representative whose signed character sum over its stabiliser vanishes has zero norm and is ignored
(kondoops.Momentum: reps, stab, zero).  The matrix elements are NOT taken from the 'between' masks of the kernel: the candidate
word c and <a| X |c> come from applying the factors of X^dagger to the representative word a with the primitives of
tests/kondoops.py (fermion, electron_flip, local_flip, each written from the source word), the representative of c from
kondoops.translate over all g, and its row by SEARCH among the representatives (no rank formula).

With w_a = |psi_a|^2 over the representatives of nonzero norm, every value comes with A = the sum of the absolute values of the
terms it is a sum of (the scale of its rounding error):
  norm2            sum_a w_a                                                                            A = norm2
  site[c][i]       sum_a w_a (1/|G|) sum_g f_c(g(i))(a),  f = n_up, n_dn, n_up n_dn, S^z = +-1/2       A: with |S^z| = 1/2
  nn[2A+B][i][j]   sum_a w_a (1/|G|) sum_g n_{g(i),A}(a) n_{g(j),B}(a)                                  A = the value
  zn[B][i][j]      sum_a w_a (1/|G|) sum_g S^z_{g(i)}(a) n_{g(j),B}(a)                                  A: with |S^z| = 1/2
  zz[i][j]         sum_a w_a (1/|G|) sum_g S^z_{g(i)}(a) S^z_{g(j)}(a)                                  A = norm2 / 4
  X[i][j]          (1/|G|) sum_a sum_g conj(psi_a) <a| X_{g(i) g(j)} |c> sigma(g*) conj(chi(g*)) sqrt(|S_b|/|S_a|) psi_b,
                   T_{g*} |c> = sigma |b>, zero-norm targets skipped                                    A = sum of the |terms|
                   X = hop[s]: c+_{i,s} c_{j,s};  ee: s^+_i s^-_j;  ll: S^+_i S^-_j;  le: S^+_i s^-_j (not Hermitian)

Bound of the GPU test: |got - want| <= (dim |G| + C_ROUND) 2^-53 A.  dim |G| bounds the number of terms of an entry (every
representative contributes at most one term per group element), so it covers the additions of the sum in any order -- the per-lane
sums, the wavefront and workgroup reductions and k_corr_reduce together add every term exactly once.  C_ROUND counts the roundings
of ONE term in k_corr_kondorepr before it is added, and the host's division afterwards:
  gathered term (hop, ee, ll, le): |S_b| / |S_a| (1), its square root (1), the product with the character (1; the sign is exact),
  the complex product with psi_b (two products and an addition per component: 3), the product with conj(psi_a) (3), the division
  by 2 n_u or n_o on the host (1): 10.
  diagonal groups: w_a = fma(re, re, im * im) (2), w_a times the signed integer count (1; the count itself is exact), the division by
  n_s, 2 n_s, n_u, 2 n_o or 4 n_u (1): 4.  The diagonals the host fills: zz[i][i] = norm2 / 4 (exact scaling); hop[s][i][i] and
  nn[.][i][i] are site sums (4); ee[i][i] = n_up - docc and ll[i][i] = norm2 / 2 + S^z subtract or add two such values (5), and
  their A is the sum of the two A's.
C_ROUND = 10.  Entries with A = 0 must be exactly 0."""
import types

import numpy as np

import kondoops as ko

LD, CLD = np.longdouble, np.clongdouble
C_ROUND = 10
KEYS = ("norm2", "site", "nn", "zn", "zz", "hop", "ee", "ll", "le")
FAULTS = ("chi_not_conjugated", "no_sigma", "no_op_sign", "no_sqrt", "zero_norm_counted", "le_transposed", "zn_swapped",
          "s_untranslated")


# ------------------------------------------------------------------------------------------------------------ lattices --
def ring(n, k):
    """(perms, turns) of the n translations of a ring at momentum 2 pi k / n"""
    return ko.chain_group(n, k)


def torus(lx, ly, kx, ky):
    return ko.torus_group(lx, ly, kx, ky)


def dihedral(n, sign):
    """the n rotations and n reflections of a ring; the trivial representation, or the one that is -1 on the reflections"""
    rot = [[(s + t) % n for s in range(n)] for t in range(n)]
    ref = [[(t - s) % n for s in range(n)] for t in range(n)]
    return rot + ref, [0] * n + [ko.Fraction(1, 2) if sign else 0] * n


def identity(n):
    return [list(range(n))], [0]


# ------------------------------------------------------------------------------------------------------------ reference --
def _adjoint_steps(kind, p, q):
    """the factors of X^dagger_{pq}, the rightmost (first to act on the representative word a) first; X^dagger |a> = amp |c>, so
    <a| X |c> = amp"""
    if kind in ("hop0", "hop1"):                                 # X = c+_p c_q, X^dagger = c+_q c_p
        sp = int(kind[-1])
        return [lambda u, d, s: ko.fermion(u, d, s, p, sp, 0), lambda u, d, s: ko.fermion(u, d, s, q, sp, 1)]
    if kind == "ee":                                             # X = s^+_p s^-_q, X^dagger = s^+_q s^-_p
        return [lambda u, d, s: ko.electron_flip(u, d, s, p, False), lambda u, d, s: ko.electron_flip(u, d, s, q, True)]
    if kind == "ll":                                             # X = S^+_p S^-_q, X^dagger = S^+_q S^-_p
        return [lambda u, d, s: ko.local_flip(u, d, s, p, False), lambda u, d, s: ko.local_flip(u, d, s, q, True)]
    assert kind == "le"                                          # X = S^+_p s^-_q, X^dagger = s^+_q S^-_p
    return [lambda u, d, s: ko.local_flip(u, d, s, p, False), lambda u, d, s: ko.electron_flip(u, d, s, q, True)]


def _candidates(kind, n, U, D, S):
    """for all (p, q) at once: the rows a, the flat pair index p * n + q, <a| X_pq |c> and the fields of c"""
    rows, pq, amp, cu, cd, cs = [], [], [], [], [], []
    for p in range(n):
        for q in range(n):
            idx = np.arange(len(U))
            u, d, s, a = U, D, S, np.ones(len(U), dtype=np.int64)
            for step in _adjoint_steps(kind, p, q):
                cols, u, d, s, sign = step(u, d, s)
                idx, a = idx[cols], a[cols] * np.asarray(sign, dtype=np.int64)
            rows.append(idx); pq.append(np.full(len(idx), p * n + q)); amp.append(a); cu.append(u); cd.append(d); cs.append(s)
    return [np.concatenate(v) for v in (rows, pq, amp, cu, cd, cs)]


def _canonical(n, perms, cu, cd, cs, s_untranslated):
    """the smallest image of every word over the group, the FIRST element that reaches it and the sign of that element on the word"""
    words = types.SimpleNamespace(n=n, u=cu, d=cd, s=cs)
    best = cu | (cd << n) | (cs << (2 * n))
    gstar, sigma = np.zeros(len(cu), dtype=np.int64), np.ones(len(cu), dtype=np.int64)
    for g in range(1, len(perms)):
        u2, d2, s2, sg = ko.translate(words, perms[g])
        im = u2 | (d2 << n) | ((cs if s_untranslated else s2) << (2 * n))
        lt = im < best
        best[lt], gstar[lt], sigma[lt] = im[lt], g, np.broadcast_to(sg, im.shape)[lt]
    return best, gstar, sigma


def _spread(T, perms):
    """out[..., i, j] = (1/|G|) sum_g T[..., g(i), g(j)]"""
    out = np.zeros_like(T)
    for pg in perms:
        pg = np.asarray(pg)
        out += T[..., pg, :][..., :, pg] / LD(len(perms))
    return out


def kondo_repr(n, n_elec, two_sz, perms, turns, psi, chars=None, fault=None, keys=KEYS):
    """dict(norm2, site, nn, zn, zz, hop, ee, ll, le, A=dict(the same keys), dim, zero, mo) from the representatives alone.
    chars: the characters the vector was measured with (the doubles handed to the library); None: the longdouble ones of `turns`.
    fault: one of FAULTS, a deliberately wrong variant that the comparison with the explicit route has to reject."""
    assert fault is None or fault in FAULTS
    sec = ko.Sector(n, n_elec, two_sz)
    mo = ko.Momentum(sec, perms, turns)
    G, N = len(perms), n
    assert len(psi) == mo.dim
    chi = ko.chars_ld(turns) if chars is None else np.asarray(chars).astype(CLD)
    chi_used = chi if fault == "chi_not_conjugated" else np.conj(chi)
    p = np.asarray(psi).astype(CLD)
    live = np.ones(mo.dim, dtype=bool) if fault == "zero_norm_counted" else ~mo.zero
    w = np.where(live, np.abs(p) ** 2, LD(0)).astype(LD)
    U, D, S = sec.u[mo.reps], sec.d[mo.reps], sec.s[mo.reps]
    rep_words = sec.w[mo.reps]
    assert np.all(np.diff(rep_words) > 0)
    norm2 = np.sum(w)
    out = {"norm2": norm2, "dim": mo.dim, "zero": mo.zero, "mo": mo}
    A = {"norm2": norm2}
    nu = [((U >> i) & 1).astype(LD) for i in range(N)]
    nd = [((D >> i) & 1).astype(LD) for i in range(N)]
    sz = [LD(0.5) - ((S >> i) & 1).astype(LD) for i in range(N)]
    if True:                                                     # the site sums also scale the diagonals of ee and ll below
        raw = np.array([[np.sum(w * f[i]) for i in range(N)] for f in (nu, nd, [a * b for a, b in zip(nu, nd)], sz)], dtype=LD)
        rawA = np.array([[np.sum(w * np.abs(f[i])) for i in range(N)] for f in (nu, nd, [a * b for a, b in zip(nu, nd)], sz)], dtype=LD)
        out["site"], A["site"] = np.zeros((4, N), dtype=LD), np.zeros((4, N), dtype=LD)
        for pg in perms:
            out["site"] += raw[:, np.asarray(pg)] / LD(G)
            A["site"] += rawA[:, np.asarray(pg)] / LD(G)
    if "nn" in keys:
        occ = (nu, nd)
        raw = np.array([[[np.sum(w * occ[a][i] * occ[b][j]) for j in range(N)] for i in range(N)] for a in (0, 1) for b in (0, 1)], dtype=LD)
        out["nn"] = _spread(raw, perms)
        A["nn"] = out["nn"].copy()
    if "zn" in keys:
        occ = (nd, nu) if fault == "zn_swapped" else (nu, nd)
        raw = np.array([[[np.sum(w * sz[i] * occ[b][j]) for j in range(N)] for i in range(N)] for b in (0, 1)], dtype=LD)
        rawA = np.array([[[np.sum(w * LD(0.5) * occ[b][j]) for j in range(N)] for i in range(N)] for b in (0, 1)], dtype=LD)
        out["zn"], A["zn"] = _spread(raw, perms), _spread(rawA, perms)
    if "zz" in keys:
        raw = np.array([[np.sum(w * sz[i] * sz[j]) for j in range(N)] for i in range(N)], dtype=LD)
        out["zz"], A["zz"] = _spread(raw, perms), np.full((N, N), norm2 / 4, dtype=LD)
    ok_row = ~mo.zero
    stab = mo.stab.astype(LD)

    def gathered(kind):
        rows, pq, amp, cu, cd, cs = _candidates(kind, N, U, D, S)
        keep = ok_row[rows]
        rows, pq, amp, cu, cd, cs = (v[keep] for v in (rows, pq, amp, cu, cd, cs))
        T, TA = np.zeros(N * N, dtype=CLD), np.zeros(N * N, dtype=LD)
        if len(rows):
            b, g, sigma = _canonical(N, perms, cu, cd, cs, fault == "s_untranslated")
            tgt = np.minimum(np.searchsorted(rep_words, b), mo.dim - 1)
            if fault != "s_untranslated":
                assert np.array_equal(rep_words[tgt], b), "the smallest image of a candidate is not a representative"
            if fault == "no_sigma":
                sigma = np.ones_like(sigma)
            if fault == "no_op_sign":
                amp = np.ones_like(amp)
            ratio = np.ones(len(rows), dtype=LD) if fault == "no_sqrt" else np.sqrt(stab[tgt] / stab[rows])
            term = np.conj(p[rows]) * (amp * sigma).astype(LD) * chi_used[g] * ratio * p[tgt]
            ok = ~mo.zero[tgt]
            np.add.at(T, pq[ok], term[ok])
            np.add.at(TA, pq[ok], np.abs(term[ok]))
        return _spread(T.reshape(N, N), perms), _spread(TA.reshape(N, N), perms)

    if "hop" in keys:
        h0, h1 = gathered("hop0"), gathered("hop1")
        out["hop"], A["hop"] = np.array([h0[0], h1[0]]), np.array([h0[1], h1[1]])
    for k in ("ee", "ll", "le"):
        if k in keys:
            out[k], A[k] = gathered(k)
    # the diagonals the call takes from the site sums (qbh_corr_kondo_dev does the same): the VALUES above come from the gathered
    # route like every other entry, the scale of the rounding error is that of the two site sums
    for i in range(N):
        if "ee" in keys:
            A["ee"][i, i] = A["site"][0, i] + A["site"][2, i]
        if "ll" in keys:
            A["ll"][i, i] = norm2 / 2 + A["site"][3, i]
    if fault == "le_transposed" and "le" in keys:
        out["le"] = out["le"].T.copy()
    out["A"] = A
    return out


# ------------------------------------------------------------------------------------------------------- comparison --
def tolerance(ref, n_trans, key):
    return (ref["dim"] * n_trans + C_ROUND) * 2.0 ** -53 * np.asarray(ref["A"][key]).astype(np.float64)


def compare(label, got, ref, n_trans, keys=KEYS):
    """every entry of every array within (dim |G| + C_ROUND) 2^-53 A; entries with A = 0 exactly 0.  Prints the worst ratio per
    group and returns them."""
    worst = {}
    for k in keys:
        w = np.asarray(ref[k])
        g = np.asarray(got[k]).reshape(w.shape)
        err = np.abs(g.astype(w.dtype) - w).astype(np.float64)
        tol = tolerance(ref, n_trans, k)
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = np.where(tol > 0, err / tol, np.where(err == 0, 0.0, np.inf))      # exact zeros stay exact
        worst[k] = float(np.max(ratio))
    print("%s dim %d |G| %d: worst |got - want| / bound  %s" % (label, ref["dim"], n_trans, "  ".join("%s %.3g" % kv for kv in worst.items())))
    for k in keys:
        assert worst[k] <= 1.0, (label, k, worst[k])
    return worst
