"""Synthetic real symmetric Kronecker-sum operators  H = T (x) 1_S + 1_NU (x) T' + D  (host only, numpy).

Index = u * S + d (species-major, what qbh_opts.kron_minor = S describes).  The knobs reach the limits of the coded split's
table route (qbh_split.cpp kronc_table_route) and of the row-staged kernel it runs (k_mf_hubbard_row):

    NU, S           major / minor size
    wu              entries of the widest row of T (the up-hop width; the route takes <= 64)
    band            T' couples d to d +- 1 .. d +- band
    far             T' couples d to d +- (S // 2 - 1 - k) for k < far as well: hops that leave the kernel's window once S > 19200
    n_amp           distinct hop amplitudes over T and T' together (the table kernel holds 15 besides zero)
    n_diag          distinct diagonal values (with the amplitudes: 1-byte codes up to 256 dictionary entries, 2-byte above)
    empty_t         the last `empty_t` major indices have no T entry

Also the ground-truth helpers of the element-wise SpMV checks: the long-double row sums of the reference and their bound.
"""
import numpy as np


def _sym_edges(n, pairs):
    """Unique undirected edges (a < b) of `pairs`, self-loops dropped."""
    if len(pairs) == 0:
        return np.zeros((0, 2), dtype=np.int64)
    p = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    p = p[p[:, 0] != p[:, 1]]
    p = np.sort(p, axis=1)
    return np.unique(p, axis=0)


def _csr_from_edges(n, edges, amp_of_edge):
    """Symmetric CSR (int64 indptr / indices, float64 data) without diagonal, sorted columns."""
    r = np.concatenate([edges[:, 0], edges[:, 1]])
    c = np.concatenate([edges[:, 1], edges[:, 0]])
    v = np.concatenate([amp_of_edge, amp_of_edge])
    order = np.lexsort((c, r))
    r, c, v = r[order], c[order], v[order]
    ia = np.zeros(n + 1, dtype=np.int64)
    np.add.at(ia, r + 1, 1)
    return np.cumsum(ia), c.astype(np.int64), v.astype(np.float64)


def amplitudes(n_amp):
    """n_amp distinct non-zero hop amplitudes, both signs, none an integer (none collides with a diagonal value below)."""
    k = np.arange(n_amp)
    return np.where(k % 2 == 0, -1.0, 1.0) * (0.375 + 0.0625 * (k // 2) + 0.001953125 * k)


def diagonals(n_diag):
    """n_diag distinct diagonal values, disjoint from amplitudes(): 2.5 + k / 64 (exact binary fractions above 2)."""
    return 2.5 + np.arange(n_diag) / 64.0


def kronsum(NU, S, wu=3, band=2, far=0, n_amp=3, n_diag=4, empty_t=0, seed=0):
    """Returns dict(ia, ja, val, dim, NU, S, T=(ia, ja, val), Tp=(ia, ja, val), D, wu, n_amp, n_dict): the operator as int64 CSR
    (full storage, sorted columns, every diagonal entry stored) and what the table route sees of it: the live width of T's widest
    row, the number of distinct hop amplitudes, the number of distinct values (the value dictionary)."""
    rng = np.random.default_rng(seed)
    assert NU >= 1 and S >= 2 and 1 <= n_amp and 1 <= n_diag
    live = NU - empty_t
    # T: a path over the live major indices, plus a star from 0 that makes row 0 the widest (wu entries)
    tp = [(u, u + 1) for u in range(live - 1)]
    if wu > 1:
        assert wu <= live - 1, "the star needs wu other live major indices"
        tp += [(0, v) for v in range(2, wu + 1)]
    te = _sym_edges(NU, tp)
    # T': a band plus `far` long-range hops per minor index
    dp = [(d, d + k) for k in range(1, band + 1) for d in range(S - k)]
    for k in range(far):
        off = S // 2 - 1 - k
        if off >= 1:
            dp += [(d, (d + off) % S) for d in range(S)]
    de = _sym_edges(S, dp)
    amps = amplitudes(n_amp)
    ta = rng.choice(amps, len(te))
    da = rng.choice(amps, len(de))
    # every amplitude present at least once (in T' when there is room, else in T)
    if len(de) >= n_amp:
        da[rng.choice(len(de), n_amp, replace=False)] = amps
    else:
        assert len(te) + len(de) >= n_amp
        ta[:n_amp - len(de)] = amps[len(de):]
        da[:] = amps[:len(de)]
    T = _csr_from_edges(NU, te, ta)
    Tp = _csr_from_edges(S, de, da)
    dim = NU * S
    dvals = diagonals(n_diag)
    D = rng.choice(dvals, dim)
    D[rng.choice(dim, n_diag, replace=False)] = dvals          # each value used at least once
    # assemble row by row in blocks: row (u, d) = T row u (columns u' * S + d), T' row d (columns u * S + d'), the diagonal
    t_ia, t_ja, t_v = T
    s_ia, s_ja, s_v = Tp
    t_len, s_len = np.diff(t_ia), np.diff(s_ia)
    u = np.repeat(np.arange(NU, dtype=np.int64), S)
    d = np.tile(np.arange(S, dtype=np.int64), NU)
    row_len = t_len[u] + s_len[d] + 1
    ia = np.zeros(dim + 1, dtype=np.int64)
    ia[1:] = np.cumsum(row_len)
    nnz = int(ia[-1])
    rows = np.repeat(np.arange(dim, dtype=np.int64), row_len)
    k = np.arange(nnz, dtype=np.int64) - ia[rows]                  # position inside the row
    ur, dr = u[rows], d[rows]
    in_t = k < t_len[ur]
    in_s = (~in_t) & (k < t_len[ur] + s_len[dr])
    ja = np.empty(nnz, dtype=np.int64)
    val = np.empty(nnz, dtype=np.float64)
    kt = t_ia[ur[in_t]] + k[in_t]
    ja[in_t] = t_ja[kt] * S + dr[in_t]
    val[in_t] = t_v[kt]
    ks = s_ia[dr[in_s]] + (k[in_s] - t_len[ur[in_s]])
    ja[in_s] = ur[in_s] * S + s_ja[ks]
    val[in_s] = s_v[ks]
    dg = ~(in_t | in_s)
    ja[dg] = rows[dg]
    val[dg] = D[rows[dg]]
    # sort the columns of every row
    order = np.lexsort((ja, rows))
    ja, val = ja[order], val[order]
    wu_live = int(t_len.max()) if NU else 0
    n_dict = len(np.unique(val))
    return dict(ia=ia, ja=ja, val=val, dim=dim, NU=NU, S=S, T=T, Tp=Tp, D=D, wu=wu_live,
                n_amp=len(np.unique(np.concatenate([t_v, s_v]))), n_dict=n_dict)


def dense(K):
    """np.kron form of the operator (small sizes only)."""
    def todense(n, c):
        ia, ja, v = c
        M = np.zeros((n, n))
        for r in range(n):
            M[r, ja[ia[r]:ia[r + 1]]] = v[ia[r]:ia[r + 1]]
        return M
    NU, S = K["NU"], K["S"]
    return np.kron(todense(NU, K["T"]), np.eye(S)) + np.kron(np.eye(NU), todense(S, K["Tp"])) + np.diag(K["D"])


def row_sums(ia, ja, val, x):
    """(H x, |H| |x|) in np.longdouble, rows summed by np.add.reduceat (empty rows give 0)."""
    ia = np.asarray(ia, dtype=np.int64)
    n = len(ia) - 1
    nnz = int(ia[-1])
    v = np.asarray(val, dtype=np.longdouble)
    xl = np.asarray(x, dtype=np.longdouble)[np.asarray(ja, dtype=np.int64)]
    out, absout = np.zeros(n, dtype=np.longdouble), np.zeros(n, dtype=np.longdouble)
    if nnz == 0:
        return out, absout
    full = np.diff(ia) > 0
    starts = ia[:-1][full]
    out[full] = np.add.reduceat(v * xl, starts)
    absout[full] = np.add.reduceat(np.abs(v) * np.abs(xl), starts)
    return out, absout


def probe_vector(n, seed):
    """A real vector with 0.25 <= |x_j| <= 1 and random signs, normalised: every term of every row is well above rounding."""
    rng = np.random.default_rng(seed)
    x = rng.uniform(0.25, 1.0, n) * rng.choice([-1.0, 1.0], n)
    return x / np.linalg.norm(x)
