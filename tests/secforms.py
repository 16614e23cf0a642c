"""Host-only helpers for the element-wise tests of the matrix-free Hubbard sector operator (qbh_mf_hubbard_repr: k_mf_sector,
k_mf_sector_orb, k_sec_remainder, k_sec_reduce in qbh_sector_mf.hip) and of the generator it shares its rows with
(qbh_gen_hubbard_repr), in the style of tests/csrforms.py and tests/kronforms.py.

Four parts, none of which needs a GPU:

* `build`: the sector operator assembled from its definition in vectorised numpy, with the conventions of qbh_gen_hubbard_repr
  (operator order all up then all down; representatives = smallest word u | d << n of each orbit, ascending; representatives whose
  norm vanishes kept as decoupled rows fake_pos + i / dim).  Entry: amp * hop sign * translation sign * conj(chi(g*)) *
  sqrt(|S_b| / |S_a|).  It gives the merged CSR and the UNMERGED term list, one (row, column, value) per hop and per diagonal
  contribution: the kernels sum term by term, so the scale S_i and the term count of a row's bound come from the unmerged list;
* `projected`: Psi^H O Psi with scipy sparse (O: tests/fastham.py for the plain operator, `full_operator` for the others; Psi: the
  momentum states with their fermion signs) -- used only to check `build`.  The two routes share the enumeration (`_images`: the
  translated patterns and their parities, the representatives, |S_a| and which norms vanish); what is independent is the operator
  (hop signs, amplitudes, diagonal) and how characters, translation signs and norms enter an entry.  The shared part is checked
  against the dense projection of tests/test_gpu_hubrepr.py at 8 sites and by the 4x2 sectors adding up to the full space;
* `blocks`: a mirror of the block structure of qbh_mf_hubbard_repr (down blocks regular or stabilised, rows and items per block,
  w_up, regular down hops per block, blocks with entries in the remainder, rows and entries of the remainder);
* the bounds (`reference`).

Bounds.  A row's result is a sum over its unmerged terms; terms_i counts them.  Roundings per term (u = eps / 2), counted in the
kernels; csrforms.epilogue's constant 4 is product (2) + alpha (1) + the two additions of beta y and gamma x, beside the
terms_i - 1 additions of the sum:

  * a hop applied by k_mf_sector / k_mf_sector_orb: the coefficient amp * conj(chi(g*)) is formed on the host in double (two
    products and one addition per component: 2), the sign of the translated up pattern is exact; product with x_j (2); the sum
    starts from the diagonal product and takes one addition per hop (<= m_mf, the terms applied by this kernel); alpha (1), the
    two additions of the epilogue (2); where the row also has entries in the remainder, the second pass y += alpha * remainder
    adds once more (1, and then m_mf <= terms_i - 1).  At most terms_i + 7.
  * the diagonal: U * popcount (1), every further contribution one addition (the four products of a density-density term with
    0 / 1 are exact and listed as terms of their own), the product with x_i (1), then the additions of the hops.  Fewer than above.
  * an entry of the stored remainder (hubrepr_row / hubrepr_row_rem): sqrt(|S_b| / |S_a|) is a division and a square root (2), the
    amplitude-character product (2), the scaling by the square root (1); product with x_j (2); the m_rem terms of the row are
    added in some order by row_merge, the eight lanes and the shuffle tree (m_rem - 1); alpha (1) and the addition into y (1).
    m_rem + 8 <= terms_i + 8.
  * beta * y and gamma * x: a product and two additions, one more addition in the second pass: 4.

Every component of y_i errs by <= gamma_{terms_i + 8} S_i, the modulus by sqrt(2) times that, and sqrt(2) * 1.01 * (k + 8) u <
0.72 (k + 8) eps, so

    |y_i - ref_i| <= (terms_i + 4 + EXTRA) eps S_i,   S_i = |alpha| sum_terms |a||x_j| + |beta||y_i| + |gamma||x_i|,   EXTRA = 4.

The reductions (k_sec_reduce: a two-level sum over the finished y) take csrforms.epilogue's t_dot / t_nrm with this row bound.
The generator's stored values carry the roundings of the third item before any product: an entry merged from m terms lies within
(m + GEN_EXTRA) eps sum |terms| with GEN_EXTRA = 5 (`value_bound`).

Probe vectors have 0.5 <= |x_j| <= 1 (csrforms.probe_vector) and every amplitude of every case has |a| >= 0.1, so a dropped,
doubled, mis-signed or misplaced term is orders of magnitude outside its row's bound (tests/test_secforms.py).

Time to build one reference on the host (`build`, one momentum and variant, on one CPU core): 4x2 0.02 s,
4x3 0.2 s, 4x4 with 4+2 0.3 s, 4x4 with 5+2 0.7 s, 13x1 0.1 s, the ring of 10 0.03 s; the five epilogues of `reference` add at most
0.4 s; the second route (`full_operator` + `projected`) takes up to 2.1 s (4x4 with 5+2, 524,160 words).
"""
from functools import lru_cache
from types import SimpleNamespace

import numpy as np
import scipy.sparse as sp

import csrforms as cf
import kronforms as kf
from csrforms import CL, EPS, L, probe_vector, worst      # noqa: F401  (re-exported for the tests)
from quantum_basis_amd import lattices
from refham import bit_patterns

EXTRA = 4
GEN_EXTRA = 5
TILE = 1024                 # kSecTile
DROP = 1e-28                # |v|^2 below which row_finish drops an off-diagonal entry
U_DEFAULT = 1.3
PHI = 0.3                   # Peierls phase of the down species' x hops
T_Y = 0.7
MU_UP, MU_DN = -0.35, 0.45  # uniform number terms of the anisotropic variant
DIAG, UP, DOWN = 0, 1, 2    # kinds of an unmerged term


# --------------------------------------------------------------------------------------------------------------- cases --
def _dihedral(Lr):
    rot = [[(s + t) % Lr for s in range(Lr)] for t in range(Lr)]
    ref = [[(t - s) % Lr for s in range(Lr)] for t in range(Lr)]
    return rot + ref


# name -> lattice (Lx, Ly) or ("ring", L), particle numbers, the momenta run on the GPU (real characters first), the variants
CASES = {
    "4x2_4+4": dict(lat=(4, 2), nu=4, nd=4, ks=[(kx, ky) for kx in range(4) for ky in range(2)], variants=("plain",)),
    "4x3_4+3": dict(lat=(4, 3), nu=4, nd=3, ks=[(0, 0), (2, 0), (1, 1)], variants=("plain", "aniso", "peierls")),
    "4x4_4+2": dict(lat=(4, 4), nu=4, nd=2, ks=[(0, 0), (2, 2), (1, 3)], variants=("plain", "aniso", "peierls")),
    "4x4_5+2": dict(lat=(4, 4), nu=5, nd=2, ks=[(0, 0), (1, 2)], variants=("plain",)),
    "13x1_6+2": dict(lat=(13, 1), nu=6, nd=2, ks=[(0, 0), (5, 0)], variants=("plain",)),
    "ring10_4+3": dict(lat=("ring", 10), nu=4, nd=3, ks=["trivial", "sign"], variants=("plain",)),
}
# what each case is there for (the mirror asserts it: tests/test_secforms.py)
PROPERTIES = {
    "4x2_4+4": dict(cu=70, regular=7, stabilised=5, w_up=12, max_nhop=6),
    "4x3_4+3": dict(cu=495, regular=18, stabilised=1, w_up=16, max_nhop=12, flagged=2, items_per_block={256: 2, 1024: 1}),
    "4x4_4+2": dict(cu=1820, regular=6, stabilised=3, max_nhop=8, flagged=4, items_per_block={1024: 2}, last_item={1024: 796}),
    "4x4_5+2": dict(cu=4368, w_up=20, items_per_block={1024: 5}, last_item={1024: 272}),
    "13x1_6+2": dict(cu=1716, stabilised=0, n_rrows=0, items_per_block={1024: 2}),
    "ring10_4+3": dict(cu=210, n_trans=20),
}


def all_keys():
    """(case, momentum index, variant) of every reference the GPU tests use."""
    return [(c, ik, v) for c, s in CASES.items() for ik in range(len(s["ks"])) for v in s["variants"]]


def has_real_characters(case, ik):
    return all(abs(complex(c).imag) == 0.0 for c in symmetry(case, ik)[1])


def _xy_bonds(Lx, Ly):
    bx, by = [], []
    for x in range(Lx):
        for y in range(Ly):
            s = x + Lx * y
            bx.append((s, (x + 1) % Lx + Lx * y))
            if Ly > 1:
                by.append((s, x + Lx * ((y + 1) % Ly)))
    return bx, by


def symmetry(case, ik):
    """-> (perms, chars) of the case's group and its ik-th representation."""
    lat = CASES[case]["lat"]
    k = CASES[case]["ks"][ik]
    if lat[0] == "ring":
        Lr = lat[1]
        return _dihedral(Lr), [1.0 + 0j] * (2 * Lr) if k == "trivial" else [1.0 + 0j] * Lr + [-1.0 + 0j] * Lr
    perms, shifts = lattices.translations(*lat)
    return perms, lattices.characters(shifts, k, lat)


def operator(case, variant):
    """-> dict(n, bonds, terms, U, pairs): the arguments of csr_mat.hubbard_repr / hubbard_repr_mf (terms always explicit)."""
    lat = CASES[case]["lat"]
    if lat[0] == "ring":
        n = lat[1]
        bx, by = lattices.chain(n), []
    else:
        n = lat[0] * lat[1]
        bx, by = _xy_bonds(*lat)
        assert sorted(bx + by) == sorted(lattices.chain(lat[0]) if lat[1] == 1 else lattices.square(*lat))
    t = 1.0
    terms, pairs = [], []
    if variant == "plain":
        for (i, j) in bx + by:
            terms += [(i, j, -t, -t), (j, i, -t, -t)]
    elif variant == "aniso":
        for (i, j) in bx:
            terms += [(i, j, -t, -t), (j, i, -t, -t)]
        for (i, j) in by:
            terms += [(i, j, -T_Y, -T_Y), (j, i, -T_Y, -T_Y)]
        terms += [(s, s, MU_UP, MU_DN) for s in range(n)]
        pairs = [(i, j, 0.2, 0.1, 0.1, 0.2) for (i, j) in bx + by]
    elif variant == "peierls":
        ph = complex(np.cos(PHI), np.sin(PHI))
        for (i, j) in bx:
            terms += [(i, j, -t, -t * ph), (j, i, -t, -t * ph.conjugate())]
        for (i, j) in by:
            terms += [(i, j, -t, -t), (j, i, -t, -t)]
    else:
        raise KeyError(variant)
    return dict(n=n, bonds=bx + by, terms=terms, U=U_DEFAULT, pairs=pairs)


# ------------------------------------------------------------------------------------------------------------ assembly --
def _images(pat, perms, n):
    """-> (image pattern [G, P], parity 0 / 1 of the permutation that sorts the images of the occupied sites [G, P])."""
    bits = ((pat[None, :] >> np.arange(n, dtype=np.int64)[:, None]) & 1).astype(np.int64)          # [n, P]
    img = np.zeros((len(perms), len(pat)), dtype=np.int64)
    par = np.zeros((len(perms), len(pat)), dtype=np.int64)
    s = np.arange(n)
    for g, p in enumerate(perms):
        p = np.asarray(p, dtype=np.int64)
        img[g] = (bits << p[:, None]).sum(axis=0)
        inv = ((s[:, None] < s[None, :]) & (p[:, None] > p[None, :])).astype(np.int64)             # pairs s < s' whose images swap
        par[g] = (bits * (inv.T @ bits)).sum(axis=0) & 1
    return img, par


def _between(occ, i, j):
    lo, hi = min(i, j), max(i, j)
    mask = ((1 << hi) - 1) & ~((2 << lo) - 1)
    return _popcount(occ & mask) & 1


def _popcount(a):
    a = a.astype(np.uint64)
    out = np.zeros(a.shape, dtype=np.int64)
    while np.any(a):
        out += (a & np.uint64(1)).astype(np.int64)
        a = a >> np.uint64(1)
    return out


def merge_terms(terms):
    """Directed one-body terms merged by (i, j), ascending, as the library's merge_terms does: [(i, j, amp_up, amp_dn)]."""
    acc = {}
    for (i, j, au, ad) in terms:
        a = acc.setdefault((int(i), int(j)), [0j, 0j])
        a[0] += complex(au)
        a[1] += complex(ad)
    return [(i, j, a[0], a[1]) for (i, j), a in sorted(acc.items())]


def build(n, nu, nd, perms, chars, terms, U, pairs=(), fake_pos=100.0):
    """The sector operator from its definition.  -> namespace with
    dim, reps (words), row_u / row_d (ranks of the up / down pattern of every row), S (|S_a|), alive,
    ia, ja, val               merged CSR (columns sorted, the diagonal always stored, cancelled off-diagonal entries dropped), val in CL
    t_ia, t_ja, t_val, t_kind unmerged terms ordered by row (CSR layout with repeated columns)
    and the enumeration tables the mirror needs (ups, dns, img_u, img_d, rank_u, rank_d)."""
    perms = np.asarray(perms, dtype=np.int64)
    G = len(perms)
    assert np.array_equal(perms[0], np.arange(n)), "the first group element must be the identity"
    chi = np.asarray(chars, dtype=np.complex128)
    ups, dns = bit_patterns(n, nu), bit_patterns(n, nd)
    cu, cd = len(ups), len(dns)
    img_u, par_u = _images(ups, perms, n)
    img_d, par_d = _images(dns, perms, n)
    rank_u, rank_d = np.searchsorted(ups, img_u), np.searchsorted(dns, img_d)
    N = cu * cd
    me = np.arange(N, dtype=np.int64)
    wd, wu = np.divmod(me, cu)
    best, gstar = me.copy(), np.zeros(N, dtype=np.int64)
    nstab, csum = np.zeros(N, dtype=np.int64), np.zeros(N, dtype=np.complex128)
    for g in range(G):
        im = rank_d[g][wd] * cu + rank_u[g][wu]
        lt = im < best
        best[lt] = im[lt]
        gstar[lt] = g
        eq = im == me
        nstab += eq
        csum[eq] += chi[g] * (1 - 2 * (par_u[g][wu[eq]] ^ par_d[g][wd[eq]]))
    reps = np.nonzero(best == me)[0]
    dim = len(reps)
    pos = np.full(N, -1, dtype=np.int64)
    pos[reps] = np.arange(dim)
    S = nstab[reps]
    alive = np.abs(csum[reps]) > 0.5
    assert np.all(np.abs(np.abs(csum[reps]) - np.where(alive, S, 0)) < 1e-9)
    row_d, row_u = wd[reps], wu[reps]
    Ur, Dr = ups[row_u], dns[row_d]
    chi_l = chi.astype(CL)
    rows, cols, vals, kinds = [], [], [], []

    def add(r, c, v, kind):
        rows.append(r)
        cols.append(c)
        vals.append(np.asarray(v, dtype=CL))
        kinds.append(np.full(len(r), kind, dtype=np.int8))

    live = np.nonzero(alive)[0]
    dead = np.nonzero(~alive)[0]
    add(dead, dead, fake_pos + dead.astype(np.float64) / float(dim), DIAG)
    if U != 0.0:
        dbl = _popcount(Ur & Dr)
        r = live[dbl[live] > 0]
        add(r, r, L(U) * dbl[r].astype(L), DIAG)
    for (i, j, vuu, vud, vdu, vdd) in pairs:
        iu, idn, ju, jd = (Ur >> i) & 1, (Dr >> i) & 1, (Ur >> j) & 1, (Dr >> j) & 1
        for v, m in ((vuu, iu & ju), (vud, iu & jd), (vdu, idn & ju), (vdd, idn & jd)):
            if v != 0.0:
                r = live[m[live] == 1]
                add(r, r, np.full(len(r), L(v)), DIAG)
    merged = merge_terms(terms)
    for (i, j, au, ad) in merged:
        for sp_, amp in ((0, au), (1, ad)):
            if amp == 0:
                continue
            occ = Dr if sp_ else Ur
            if i == j:
                r = live[((occ >> i) & 1)[live] == 1]
                add(r, r, np.full(len(r), CL(amp)), DIAG)
                continue
            r = live[(((occ >> i) & 1) & (1 - ((occ >> j) & 1)))[live] == 1]       # the particle moves from i to j
            o = occ[r]
            hop = _between(o, i, j)
            o2 = o ^ (1 << i) ^ (1 << j)
            if sp_:
                cd_, cu_ = np.searchsorted(dns, o2), row_u[r]
            else:
                cd_, cu_ = row_d[r], np.searchsorted(ups, o2)
            c = cd_ * cu + cu_
            g = gstar[c]
            tsg = par_u[g, cu_] ^ par_d[g, cd_]
            col = pos[best[c]]
            ok = alive[col]
            r, col, g, sg = r[ok], col[ok], g[ok], (1 - 2 * (hop ^ tsg)[ok]).astype(L)
            v = CL(amp) * sg * np.conj(chi_l[g]) * np.sqrt(S[col].astype(L) / S[r].astype(L))
            add(r, col, v, DOWN if sp_ else UP)
    row = np.concatenate(rows)
    col = np.concatenate(cols)
    val = np.concatenate(vals)
    kind = np.concatenate(kinds)
    o = np.argsort(row, kind="stable")
    t_row, t_ja, t_val, t_kind = row[o], col[o], val[o], kind[o]
    t_ia = np.zeros(dim + 1, dtype=np.int64)
    np.cumsum(np.bincount(t_row, minlength=dim), out=t_ia[1:])
    # merged: the diagonal always, columns ascending
    mrow = np.concatenate([t_row, np.arange(dim)])
    mcol = np.concatenate([t_ja, np.arange(dim)])
    mval = np.concatenate([t_val, np.zeros(dim, dtype=CL)])
    mcnt = np.concatenate([np.ones(len(t_row), dtype=np.int64), np.zeros(dim, dtype=np.int64)])
    o = np.lexsort((mcol, mrow))
    mrow, mcol, mval, mcnt = mrow[o], mcol[o], mval[o], mcnt[o]
    first = np.concatenate([[True], (mrow[1:] != mrow[:-1]) | (mcol[1:] != mcol[:-1])])
    idx = np.nonzero(first)[0]
    v = np.add.reduceat(mval, idx)
    va = np.add.reduceat(np.abs(mval), idx)
    cnt = np.add.reduceat(mcnt, idx)
    r, c = mrow[idx], mcol[idx]
    keep = (r == c) | ((v.real * v.real + v.imag * v.imag) >= DROP)
    r, c, v, va, cnt = r[keep], c[keep], v[keep], va[keep], cnt[keep]
    ia = np.zeros(dim + 1, dtype=np.int64)
    np.cumsum(np.bincount(r, minlength=dim), out=ia[1:])
    return SimpleNamespace(n=n, nu=nu, nd=nd, G=G, cu=cu, cd=cd, dim=dim, reps=ups[row_u] | (dns[row_d] << n), row_u=row_u, row_d=row_d,
                           S=S, alive=alive, ia=ia, ja=c, val=v, val_abs=va, val_terms=cnt, t_ia=t_ia, t_ja=t_ja, t_val=t_val,
                           t_kind=t_kind, terms_row=np.diff(t_ia), ups=ups, dns=dns, img_u=img_u, img_d=img_d, rank_u=rank_u,
                           rank_d=rank_d, chars=chi, perms=perms, merged_terms=merged, U=U, pairs=list(pairs), fake_pos=fake_pos)


@lru_cache(maxsize=None)
def sector(case, ik, variant):
    """`build` of a case, cached for the whole session.  The arrays are shared between tests: leave them unchanged."""
    spec = CASES[case]
    op = operator(case, variant)
    perms, chars = symmetry(case, ik)
    sec = build(op["n"], spec["nu"], spec["nd"], perms, chars, op["terms"], op["U"], op["pairs"])
    for a in (sec.ia, sec.ja, sec.val, sec.t_ia, sec.t_ja, sec.t_val):
        a.setflags(write=False)
    return sec


def value_bound(sec):
    """Bound on |stored value - sec.val| per merged entry for a generator that forms every term in double (module docstring)."""
    return (sec.val_terms.astype(L) + GEN_EXTRA) * L(EPS) * sec.val_abs


# ----------------------------------------------------------------------------------------------------- second route --
def _species_matrix(n, cnt, terms, which):
    """T[new, old] = sum amp * sign over the directed terms amp * c+_i c_j (i != j) of one species, patterns ascending."""
    pat = bit_patterns(n, cnt)
    rows, cols, vals = [], [], []
    for t in terms:
        i, j, amp = t[0], t[1], complex(t[2 + which])
        if i == j or amp == 0:
            continue
        ok = np.nonzero(((pat >> j) & 1) & (1 - ((pat >> i) & 1)))[0]
        old = pat[ok]
        rows.append(np.searchsorted(pat, old ^ (1 << i) ^ (1 << j)))
        cols.append(ok)
        vals.append(amp * (1 - 2 * _between(old, i, j)))
    m = len(pat)
    if not rows:
        return sp.csr_matrix((m, m), dtype=np.complex128)
    return sp.csr_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(m, m))


def full_operator(n, nu, nd, terms, U, pairs=()):
    """The full-space operator in the order of the words u | d << n (index = rank(d) * C(n, nu) + rank(u)): fastham.hubbard_full
    generalised to directed complex terms, number terms and density-density terms."""
    ups, dns = bit_patterns(n, nu), bit_patterns(n, nd)
    cu, cd = len(ups), len(dns)
    O = sp.kron(sp.identity(cd), _species_matrix(n, nu, terms, 0), format="csr") + \
        sp.kron(_species_matrix(n, nd, terms, 1), sp.identity(cu), format="csr")
    u, d = np.tile(ups, cd), np.repeat(dns, cu)
    diag = U * _popcount(u & d).astype(np.complex128)
    for (i, j, vuu, vud, vdu, vdd) in pairs:
        iu, idn, ju, jd = (u >> i) & 1, (d >> i) & 1, (u >> j) & 1, (d >> j) & 1
        diag += vuu * (iu & ju) + vud * (iu & jd) + vdu * (idn & ju) + vdd * (idn & jd)
    for t in terms:
        if t[0] == t[1]:
            diag += complex(t[2]) * ((u >> t[0]) & 1) + complex(t[3]) * ((d >> t[0]) & 1)
    return (O + sp.diags(diag)).tocsr()


def plain_operator(n, nu, nd, bonds, t, U):
    """fastham.hubbard_full (index = rank(u) * C(n, nd) + rank(d)) moved to the order of the words."""
    import fastham
    H = fastham.hubbard_full(n, nu, nd, bonds, t=t, U=U).tocsr()
    cu, cd = len(bit_patterns(n, nu)), len(bit_patterns(n, nd))
    rd, ru = np.divmod(np.arange(cu * cd), cu)
    p = ru * cd + rd
    return H[p][:, p].astype(np.complex128).tocsr()


def projected(sec, O):
    """Psi^H O Psi as scipy CSR, the rows of the representatives without norm replaced by their fake diagonal.  Psi[g(a), a] =
    chi(g) sgn(g, a) / sqrt(|G| |S_a|)."""
    cu = sec.cu
    G = sec.G
    _, par_u = _images(sec.ups, sec.perms, sec.n)
    _, par_d = _images(sec.dns, sec.perms, sec.n)
    rows, vals = [], []
    for g in range(G):
        rows.append(sec.rank_d[g][sec.row_d] * cu + sec.rank_u[g][sec.row_u])
        vals.append(sec.chars[g] * (1 - 2 * (par_u[g][sec.row_u] ^ par_d[g][sec.row_d])) / np.sqrt(G * sec.S.astype(np.float64)))
    Psi = sp.csr_matrix((np.concatenate(vals), (np.concatenate(rows), np.tile(np.arange(sec.dim), G))), shape=(O.shape[0], sec.dim))
    keep = sp.diags(sec.alive.astype(np.float64))
    Psi = (Psi @ keep).tocsr()
    Hk = (Psi.conj().T @ (O @ Psi)).tocsr()
    dead = np.nonzero(~sec.alive)[0]
    fake = np.zeros(sec.dim)
    fake[dead] = sec.fake_pos + dead.astype(np.float64) / float(sec.dim)
    return (Hk + sp.diags(fake)).tocsr()


def merged_scipy(sec):
    return sp.csr_matrix((sec.val.astype(np.complex128), sec.ja, sec.ia), shape=(sec.dim, sec.dim))


# -------------------------------------------------------------------------------------------------------------- mirror --
def blocks(sec, tile=TILE):
    """The block structure qbh_mf_hubbard_repr builds for this sector, from the rules of its host code: canonical down patterns
    (no translation g >= 1 gives a smaller image), stabilised where one gives the same; rows of a stabilised block = the up
    patterns no stabiliser element makes smaller; one work item per `tile` rows; per regular block the down hops whose target
    block is regular (one per (target block, g*)), the others flagged for the stored remainder."""
    cu, G, n = sec.cu, sec.G, sec.n
    dns, ups = sec.dns, sec.ups
    canon = np.all(sec.img_d[1:] >= dns[None, :], axis=0) if G > 1 else np.ones(len(dns), dtype=bool)
    bd = np.nonzero(canon)[0]                                        # ranks of the blocks' down patterns, ascending
    stab = sec.img_d[:, bd] == dns[bd][None, :]
    stab[0] = False
    regular = ~stab.any(axis=0)
    nrows = np.full(len(bd), cu, dtype=np.int64)
    for b in np.nonzero(~regular)[0]:
        gs = np.nonzero(stab[:, b])[0]
        nrows[b] = int(np.all(sec.img_u[gs] >= ups[None, :], axis=0).sum())
    row0 = np.concatenate([[0], np.cumsum(nrows)])
    block_of_rank = np.full(len(dns), -1, dtype=np.int64)
    block_of_rank[bd] = np.arange(len(bd))
    # up hops: the widest row of the ELL table
    w = np.zeros(cu, dtype=np.int64)
    for (i, j, au, ad) in sec.merged_terms:
        if i != j and abs(au) ** 2 >= DROP:
            w += ((ups >> i) & 1) & (1 - ((ups >> j) & 1))
    n_amp_up = len({abs(complex(au)) for (i, j, au, ad) in sec.merged_terms if i != j and au != 0})
    # down hops of the regular blocks
    nhop = np.zeros(len(bd), dtype=np.int64)
    flagged = np.zeros(len(bd), dtype=bool)
    complex_hop = False
    for b in np.nonzero(regular)[0]:
        d = int(dns[bd[b]])
        keys = set()
        for (i, j, au, ad) in sec.merged_terms:
            if i == j or ad == 0 or not (d >> i) & 1 or (d >> j) & 1:
                continue
            r2 = int(np.searchsorted(dns, d ^ (1 << i) ^ (1 << j)))
            im = sec.img_d[:, r2]
            gb = int(np.argmin(im))                                  # the first translation that gives the smallest image
            tb = block_of_rank[np.searchsorted(dns, im[gb])]
            if not regular[tb]:
                flagged[b] = True
                continue
            c = complex(ad) * np.conj(sec.chars[gb])
            if abs(c) ** 2 >= DROP:
                keys.add((int(tb), gb))
                complex_hop = complex_hop or (c.imag != 0.0 and complex(ad).imag != 0.0)
        nhop[b] = len(keys)
    # the remainder: every row of a stabilised block; of a regular row the down hops into stabilised blocks
    blk_of_row = np.searchsorted(row0, np.arange(sec.dim), side="right") - 1
    t_row = np.repeat(np.arange(sec.dim), np.diff(sec.t_ia))
    reg_row = regular[blk_of_row]
    into_stab = reg_row[t_row] & ~reg_row[sec.t_ja]
    assert np.all(sec.t_kind[into_stab] == DOWN)
    pairs_reg = np.unique(t_row[into_stab] * sec.dim + sec.t_ja[into_stab])
    rows_reg = np.unique(pairs_reg // sec.dim)
    rows_stab = np.nonzero(~reg_row)[0]
    rnnz = len(pairs_reg) + int(np.diff(sec.ia)[rows_stab].sum())
    items = -(-nrows // tile)
    return SimpleNamespace(d=dns[bd], d_rank=bd, regular=regular, nrows=nrows, row0=row0, items=items, n_items=int(items.sum()),
                           w_up=int(w.max()) if cu else 0, n_amp_up=n_amp_up, nhop=nhop, flagged=flagged & regular, complex_hop=complex_hop,
                           blk_of_row=blk_of_row, rows_reg=rows_reg, rows_stab=rows_stab, n_rrows=len(rows_reg) + len(rows_stab),
                           rnnz=rnnz, tile=tile, has_number_terms=any(i == j for (i, j, au, ad) in sec.merged_terms))


def mf_bytes_ascending(sec, b):
    """info().bytes_matrix of the operator created with sector_orbit = 0 (adopt_mf_sector: 32-byte block descriptors, 8 bytes per
    item, 12 per remainder row, 20 per remainder entry, 4 (1 + w_up + |G|) per up pattern)."""
    return len(b.d) * 32 + b.n_items * 8 + b.n_rrows * 12 + b.rnnz * 20 + sec.cu * 4 * (1 + b.w_up + sec.G)


def name_row(sec, b, i, internal=None):
    """Row i of the caller's order as text: the block's down pattern, the up pattern, and -- from the position `internal` of the row
    in the operator's own order (i itself in the ascending order) -- the work item and the row inside it."""
    blk = int(b.blk_of_row[i])
    p = int((i if internal is None else internal) - b.row0[blk])
    return "block %d (d = 0x%x, %s), u = 0x%x, item %d of the block, row %d of the item" % (
        blk, int(b.d[blk]), "regular" if b.regular[blk] else "stabilised", int(sec.ups[sec.row_u[i]]), p // b.tile, p % b.tile)


# -------------------------------------------------------------------------------------------------------------- bounds --
def row_sums(sec, x):
    """(sum over the unmerged terms a x_j, sum |a||x_j|) per row in long double."""
    return cf.row_sums(sec.t_ia, sec.t_ja, sec.t_val, x)


def reference(sec, sums, x, y0, alpha, beta, gamma):
    """csrforms.epilogue over the unmerged terms with the constant 4 + EXTRA (module docstring): y, bound, dot, nrm, t_dot, t_nrm."""
    return kf.epilogue(sums[0], sums[1], sec.terms_row, x, y0, alpha, beta, gamma, extra=EXTRA)


def tampered(sec, row, how):
    """(t_ja, t_val) with one off-diagonal term of `row` (its only term where it has no other) dropped, sign-flipped or moved to the
    neighbouring column: what a kernel with one wrong table entry would apply."""
    ja, val = sec.t_ja.copy(), sec.t_val.copy()
    p0, p1 = int(sec.t_ia[row]), int(sec.t_ia[row + 1])
    off = [p for p in range(p0, p1) if ja[p] != row]
    p = off[len(off) // 2] if off else p0
    if how == "dropped":
        val[p] = 0
    elif how == "flipped":
        val[p] = -val[p]
    elif how == "moved":
        ja[p] = ja[p] + 1 if ja[p] + 1 < sec.dim else ja[p] - 1
    else:
        raise KeyError(how)
    return ja, val
