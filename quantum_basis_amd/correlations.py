"""All-pair static correlations of a device-resident state in one pass (qbh_corr_spin_dev / qbh_corr_hubbard_dev /
qbh_corr_qudit_dev / qbh_corr_kondo_dev / qbh_corr_spin_repr_dev / qbh_corr_hubbard_repr_dev / qbh_corr_qudit_repr_dev /
qbh_corr_kondo_repr_dev), and the host arithmetic that follows them: structure factor, momentum distribution, the energy as a sum of two-site expectation values.

The device calls reduce over the state without a temporary vector, so they run next to a state that fills most of HBM; the
reference's measure_full_static (src/model.cc:1660-1694) applies one product of operators per call into sector-sized temporaries.
The momentum-sector states of all four families are covered (spin_repr_correlations, hubbard_repr_correlations,
qudit_repr_correlations with spin_s_repr_correlations and bose_repr_correlations, kondo_repr_correlations: from the orbit
representatives alone).
"""
import ctypes as C

import numpy as np

from ._lib import check, lib


def _addr(d_vec):
    """device address of a DeviceVec, a torch tensor on the device, a ctypes pointer or an integer"""
    if hasattr(d_vec, "data_ptr"):
        return C.c_void_p(d_vec.data_ptr())
    p = getattr(d_vec, "ptr", d_vec)
    return p if isinstance(p, C.c_void_p) else C.c_void_p(int(p))


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def _generator_order(d_vec, real, source):
    """(device address in the generators' order, buffer to free afterwards)"""
    if source is None or source.info().basis_internal == 0:
        return _addr(d_vec), None
    if real:
        raise ValueError("a packed-real vector of a handle that keeps another basis order internally (basis_internal != 0) cannot be "
                         "translated: pass the complex vector, or a vector in the generators' order without `source`")
    conv = source.vec(1)
    source.from_internal(conv.ptr, _addr(d_vec))
    source.sync()
    return conv.ptr, conv


def _nonzero_norm(norm2, who):
    if not norm2 > 0.0:
        raise ValueError("%s: <psi|psi> = %r, nothing to normalise by (normalize=False returns the raw sums)" % (who, norm2))


def spin_correlations(n_sites, n_dn, d_vec, real=False, source=None, normalize=True, stream=None):
    """<S^z_i>, <S^z_i S^z_j> and <S^+_i S^-_j> for ALL pairs of sites of a spin-1/2 state with n_dn down spins (basis of
    csr_mat.heisenberg), one pass over the state.  d_vec: device address (or DeviceVec) of the whole sector, complex128, or its
    packed real parts (real=True: n doubles).  source: the handle the vector belongs to -- needed when that handle keeps another
    order internally (info().basis_internal != 0); the vector is translated first (a packed-real one cannot be: ValueError).
    Returns dict(norm2, sz[N], zz[N][N], pm[N][N], ss[N][N]) with ss = <S_i . S_j> = zz + Re pm (3/4 on the diagonal); with
    normalize the arrays are divided by norm2 = <psi|psi> (norm2 itself is returned as measured)."""
    N = int(n_sites)
    addr, conv = _generator_order(d_vec, real, source)
    try:
        n2 = C.c_double()
        sz, zz, pm = np.zeros(N), np.zeros((N, N)), np.zeros((N, N), dtype=np.complex128)
        check(lib().qbh_corr_spin_dev(N, int(n_dn), None if real else addr, addr if real else None, C.byref(n2), _p(sz), _p(zz), _p(pm),
                                      stream), "qbh_corr_spin_dev")
    finally:
        if conv is not None:
            conv.free()
    norm2 = n2.value
    ss = zz + pm.real
    ss[np.diag_indices(N)] = 0.75 * norm2
    out = {"norm2": norm2, "sz": sz, "zz": zz, "pm": pm, "ss": ss}
    if normalize:
        _nonzero_norm(norm2, "spin_correlations")
        for k in ("sz", "zz", "pm", "ss"):
            out[k] = out[k] / norm2
    return out


def spin_repr_correlations(n_sites, n_dn, perms, chars, d_vec, real=False, source=None, normalize=True, stream=None):
    """spin_correlations for a state of a MOMENTUM SECTOR: d_vec is indexed like the rows of csr_mat.heisenberg_repr for the same
    (n_sites, n_dn, perms, chars) -- all orbit representatives, ascending -- and the result is what spin_correlations gives on
    the unfolded full-space state, computed from the representatives in one pass (qbh_corr_spin_repr_dev).  perms [n_trans][N]
    (translation 0 the identity), chars [n_trans] complex.  real=True: d_vec holds packed real parts; every character must be
    real.  Entries at representatives whose norm vanishes at this momentum (the decoupled fake rows) are ignored.  source as in
    spin_correlations.  Returns dict(norm2, sz, zz, pm, ss, dim), dim the number of representatives; structure_factor and
    energy_from_correlations take it as it is."""
    N = int(n_sites)
    p = np.ascontiguousarray(perms, dtype=np.int32).reshape(-1, N)
    ch = np.ascontiguousarray(np.asarray(chars, dtype=np.complex128).reshape(-1))
    if ch.shape[0] != p.shape[0]:
        raise ValueError("spin_repr_correlations: %d characters for %d translations" % (ch.shape[0], p.shape[0]))
    addr, conv = _generator_order(d_vec, real, source)
    try:
        n2, dim = C.c_double(), C.c_int64()
        sz, zz, pm = np.zeros(N), np.zeros((N, N)), np.zeros((N, N), dtype=np.complex128)
        check(lib().qbh_corr_spin_repr_dev(N, int(n_dn), int(p.shape[0]), _p(p), _p(ch.view(np.float64)), None if real else addr,
                                           addr if real else None, C.byref(n2), _p(sz), _p(zz), _p(pm), C.byref(dim), stream),
              "qbh_corr_spin_repr_dev")
    finally:
        if conv is not None:
            conv.free()
    norm2 = n2.value
    ss = zz + pm.real
    ss[np.diag_indices(N)] = 0.75 * norm2
    out = {"norm2": norm2, "sz": sz, "zz": zz, "pm": pm, "ss": ss, "dim": int(dim.value)}
    if normalize:
        _nonzero_norm(norm2, "spin_repr_correlations")
        for k in ("sz", "zz", "pm", "ss"):
            out[k] = out[k] / norm2
    return out


def hubbard_correlations(n_sites, n_up, n_dn, d_vec, real=False, source=None, normalize=True, want=("dens", "nn", "hop", "flip"), stream=None):
    """<n_{i,s}>, <n_{i,a} n_{j,b}>, <c+_{i,s} c_{j,s}> and <S^+_i S^-_j> for ALL pairs of sites of a two-species fermion state
    (basis, operator order and signs of csr_mat.hubbard / moprXvec_terms family 1), one pass over the state.  d_vec / real /
    source / normalize as in spin_correlations.  want: the groups to compute (a group left out costs nothing, its gathers are not
    issued).  Returns dict(norm2, dens[2][N], nn[4][N][N] (uu, ud, du, dd), hop[2][N][N], flip[N][N]) for the wanted groups, and
    derived from them: docc[N] = <n_up n_dn>, szsz[N][N], nn_total[N][N] (from nn); ss[N][N] = <S_i . S_j> (from nn and flip)."""
    N = int(n_sites)
    want = set(want)
    unknown = want - {"dens", "nn", "hop", "flip"}
    if unknown:
        raise ValueError("hubbard_correlations: unknown group(s) %s" % sorted(unknown))
    addr, conv = _generator_order(d_vec, real, source)
    try:
        n2 = C.c_double()
        dens = np.zeros((2, N)) if "dens" in want else None
        nn = np.zeros((4, N, N)) if "nn" in want else None
        hop = np.zeros((2, N, N), dtype=np.complex128) if "hop" in want else None
        flip = np.zeros((N, N), dtype=np.complex128) if "flip" in want else None
        check(lib().qbh_corr_hubbard_dev(N, int(n_up), int(n_dn), None if real else addr, addr if real else None, C.byref(n2), _p(dens),
                                         _p(nn), _p(hop), _p(flip), stream), "qbh_corr_hubbard_dev")
    finally:
        if conv is not None:
            conv.free()
    out = {"norm2": n2.value}
    for k, a in (("dens", dens), ("nn", nn), ("hop", hop), ("flip", flip)):
        if a is not None:
            out[k] = a
    _hubbard_derived(out, nn, flip, N)
    if normalize:
        _nonzero_norm(out["norm2"], "hubbard_correlations")
        for k in out:
            if k != "norm2":
                out[k] = out[k] / out["norm2"]
    return out


def _hubbard_derived(out, nn, flip, N):
    """docc, szsz, nn_total and ss of hubbard_correlations from the raw groups, each where its inputs are present"""
    if nn is not None:
        out["docc"] = np.diag(nn[1]).copy()
        out["szsz"] = 0.25 * (nn[0] - nn[1] - nn[2] + nn[3])
        out["nn_total"] = nn[0] + nn[1] + nn[2] + nn[3]
        if flip is not None:
            ss = out["szsz"] + flip.real
            ss[np.diag_indices(N)] = 3.0 * np.diag(out["szsz"])        # S_i^2 = 3 (S^z_i)^2 for a spin-1/2 or an empty / doubly occupied site
            out["ss"] = ss
    return out


def hubbard_repr_correlations(n_sites, n_up, n_dn, perms, chars, d_vec, real=False, source=None, normalize=True,
                              want=("dens", "nn", "hop", "flip"), no_double=False, stream=None):
    """hubbard_correlations for a state of a MOMENTUM SECTOR: d_vec is indexed like the rows of csr_mat.hubbard_repr (tj_repr with
    no_double=True) for the same (n_sites, n_up, n_dn, perms, chars) -- all orbit representatives, ascending -- and the result is
    what hubbard_correlations gives on the unfolded full-space state, computed from the representatives in one pass without a second
    vector (qbh_corr_hubbard_repr_dev).  perms [n_trans][N] (element 0 the identity; reflections allowed), chars [n_trans] complex.
    real=True: d_vec holds packed real parts; every character must be real.  Entries at representatives whose norm vanishes at this
    momentum (the decoupled fake rows) are ignored.  source: the handle the vector belongs to; a device vector of a hubbard_repr_mf
    handle is kept in the orbit order (info().basis_internal != 0) and is translated first.  want as in hubbard_correlations.
    Returns the dict of hubbard_correlations (norm2, dens, nn, hop, flip, docc, szsz, nn_total, ss) plus dim, the number of
    representatives; momentum_distribution, structure_factor and energy_from_correlations take the arrays as they are."""
    N = int(n_sites)
    want = set(want)
    unknown = want - {"dens", "nn", "hop", "flip"}
    if unknown:
        raise ValueError("hubbard_repr_correlations: unknown group(s) %s" % sorted(unknown))
    p = np.ascontiguousarray(perms, dtype=np.int32).reshape(-1, N)
    ch = np.ascontiguousarray(np.asarray(chars, dtype=np.complex128).reshape(-1))
    if ch.shape[0] != p.shape[0]:
        raise ValueError("hubbard_repr_correlations: %d characters for %d translations" % (ch.shape[0], p.shape[0]))
    addr, conv = _generator_order(d_vec, real, source)
    try:
        n2, dim = C.c_double(), C.c_int64()
        dens = np.zeros((2, N)) if "dens" in want else None
        nn = np.zeros((4, N, N)) if "nn" in want else None
        hop = np.zeros((2, N, N), dtype=np.complex128) if "hop" in want else None
        flip = np.zeros((N, N), dtype=np.complex128) if "flip" in want else None
        check(lib().qbh_corr_hubbard_repr_dev(N, int(n_up), int(n_dn), int(bool(no_double)), int(p.shape[0]), _p(p), _p(ch.view(np.float64)),
                                              None if real else addr, addr if real else None, C.byref(n2), _p(dens), _p(nn), _p(hop),
                                              _p(flip), C.byref(dim), stream), "qbh_corr_hubbard_repr_dev")
    finally:
        if conv is not None:
            conv.free()
    out = {"norm2": n2.value}
    for k, a in (("dens", dens), ("nn", nn), ("hop", hop), ("flip", flip)):
        if a is not None:
            out[k] = a
    _hubbard_derived(out, nn, flip, N)
    if normalize:
        _nonzero_norm(out["norm2"], "hubbard_repr_correlations")
        for k in out:
            if k != "norm2":
                out[k] = out[k] / out["norm2"]
    out["dim"] = int(dim.value)
    return out


def qudit_correlations(n_sites, d, total, d_vec, diag=(), string=None, lower=None, real=False, normalize=True, stream=None):
    """The thin wrapper of qbh_corr_qudit_dev: a state of the sector `total` of csr_mat.qudit (d levels per site, l_s the level of
    site s), complex128 or its packed real parts (real=True), in the generator's order.  diag: up to four tables f_a[l];
    string = (h[l], g[l]); lower[l] = <l-1| A |l> of an operator that lowers the level by one.  Returns dict(norm2, pop[N][d]) and,
    for the tables that were given, dd[K][K][N][N] = <f_a(i) f_b(j)>, str[N][N] = <h_i prod_{i<k<j} g_k h_j> (diagonal <h_i^2>),
    aa[N][N] = <A_i A+_j>; with normalize the arrays are divided by norm2 (norm2 itself is returned as measured)."""
    N, d = int(n_sites), int(d)
    f = np.ascontiguousarray(np.asarray(diag, dtype=np.float64).reshape(-1, d)) if len(diag) else None
    K = 0 if f is None else f.shape[0]
    h = g = None
    if string is not None:
        h, g = (np.ascontiguousarray(t, dtype=np.float64).reshape(d) for t in string)
    low = np.ascontiguousarray(lower, dtype=np.float64).reshape(d) if lower is not None else None
    addr = _addr(d_vec)
    n2 = C.c_double()
    pop = np.zeros((N, d))
    dd = np.zeros((K, K, N, N)) if K else None
    st = np.zeros((N, N)) if string is not None else None
    aa = np.zeros((N, N), dtype=np.complex128) if low is not None else None
    check(lib().qbh_corr_qudit_dev(N, d, int(total), None if real else addr, addr if real else None, K, _p(f), _p(h), _p(g), _p(low),
                                   C.byref(n2), _p(pop), _p(dd), _p(st), _p(aa), stream), "qbh_corr_qudit_dev")
    out = {"norm2": n2.value, "pop": pop}
    for k, a in (("dd", dd), ("str", st), ("aa", aa)):
        if a is not None:
            out[k] = a
    if normalize:
        _nonzero_norm(out["norm2"], "qudit_correlations")
        for k in out:
            if k != "norm2":
                out[k] = out[k] / out["norm2"]
    return out


def _spin_s_from_raw(S, raw):
    """host arithmetic of spin_s_correlations on the raw arrays of qudit_correlations (diag = (m,), A = S^+)"""
    from . import qudit as qd
    d = qd._two_s(S) + 1
    Sv = (d - 1) / 2.0
    m = Sv - np.arange(d)
    zz, pm = raw["dd"][0, 0], raw["aa"]
    ss = zz + pm.real
    ss[np.diag_indices(len(zz))] = Sv * (Sv + 1) * raw["norm2"]
    return {"norm2": raw["norm2"], "sz": raw["pop"] @ m, "sz2": raw["pop"] @ (m * m), "zz": zz, "pm": pm, "ss": ss,
            "string": raw.get("str")}


def spin_s_correlations(n_sites, S, two_sz, d_vec, real=False, normalize=True):
    """<S^z_i>, <(S^z_i)^2>, <S^z_i S^z_j>, <S^+_i S^-_j>, <S_i . S_j> = zz + Re pm (S(S+1) on the diagonal) and, for integer S, the
    den Nijs-Rommelse string correlator <S^z_i exp(i pi sum_{i<k<j} S^z_k) S^z_j> of a spin-S state with 2 S^z = two_sz (basis of
    csr_mat.spin_heisenberg), all pairs in one pass.  Returns dict(norm2, sz, sz2, zz, pm, ss, string); string is None for
    half-integer S (its phases are complex).  With the keys zz and pm, energy_from_correlations gives <H> of the spin-S Heisenberg
    operator."""
    from . import qudit as qd
    d, m, string, lower = _spin_s_tables(S)
    raw = qudit_correlations(n_sites, d, qd.spin_charge(n_sites, S, two_sz), d_vec, diag=(m,), string=string, lower=lower, real=real,
                             normalize=False)
    out = _spin_s_from_raw(S, raw)
    if normalize:
        _nonzero_norm(out["norm2"], "spin_s_correlations")
        for k in out:
            if k != "norm2" and out[k] is not None:
                out[k] = out[k] / out["norm2"]
    return out


def _bose_from_raw(n_max, raw):
    """host arithmetic of bose_correlations on the raw arrays of qudit_correlations (diag = (n,), A = b, string = (1, (-1)^n))"""
    n = np.arange(n_max + 1, dtype=np.float64)
    obdm = raw["aa"].T.copy()                                 # <b+_i b_j> = <b_j b+_i> off the diagonal
    k = np.diag_indices(len(obdm))
    obdm[k] = raw["aa"][k] - raw["norm2"]                     # b+ b = b b+ - 1 (exact while level n_max carries no weight; dens is <n> always)
    return {"norm2": raw["norm2"], "dens": raw["pop"] @ n, "nn": raw["dd"][0, 0], "obdm": obdm, "parity": raw["str"]}


def bose_correlations(n_sites, n_bosons, n_max, d_vec, real=False, normalize=True):
    """<n_i>, <n_i n_j>, the one-body density matrix obdm[i][j] = <b+_i b_j> and the parity string <prod_{i<k<j} (-1)^{n_k}> of a
    state of n_bosons bosons with at most n_max per site (basis of csr_mat.bose_hubbard), all pairs in one pass.  Returns
    dict(norm2, dens, nn, obdm, parity); momentum_distribution(obdm, ...) and structure_factor(nn, ...) take them as they are."""
    n = np.arange(n_max + 1, dtype=np.float64)
    raw = qudit_correlations(n_sites, n_max + 1, n_bosons, d_vec, diag=(n,), string=(np.ones(n_max + 1), 1.0 - 2.0 * (np.arange(n_max + 1) % 2)),
                             lower=np.sqrt(n), real=real, normalize=False)
    out = _bose_from_raw(n_max, raw)
    if normalize:
        _nonzero_norm(out["norm2"], "bose_correlations")
        for k in out:
            if k != "norm2":
                out[k] = out[k] / out["norm2"]
    return out


def qudit_repr_correlations(n_sites, d, total, perms, chars, d_vec, diag=(), string=None, lower=None, real=False, normalize=True,
                            stream=None):
    """qudit_correlations for a state of a MOMENTUM SECTOR: d_vec is indexed like the rows of csr_mat.qudit_repr (stored or
    matrix_free) for the same (n_sites, d, total, perms, chars) -- all orbit representatives, ascending -- and the result is what qudit_correlations
    gives on the unfolded full-space state, computed from the representatives in one pass without a second vector
    (qbh_corr_qudit_repr_dev).  perms [n_trans][N] (element 0 the identity; reflections allowed), chars [n_trans] complex.
    real=True: d_vec holds packed real parts; every character must be real.  Entries at representatives whose norm vanishes at
    this momentum are ignored.  The string correlator str[i][j] is the average over the group of the index-ordered string of
    qudit_correlations (on a ring: of all strings of that length, wrapped ones included).  Returns dict(norm2, pop) and, for the
    tables that were given, dd, str, aa, plus dim, the number of representatives."""
    N, d = int(n_sites), int(d)
    p = np.ascontiguousarray(perms, dtype=np.int32).reshape(-1, N)
    ch = np.ascontiguousarray(np.asarray(chars, dtype=np.complex128).reshape(-1))
    if ch.shape[0] != p.shape[0]:
        raise ValueError("qudit_repr_correlations: %d characters for %d translations" % (ch.shape[0], p.shape[0]))
    f = np.ascontiguousarray(np.asarray(diag, dtype=np.float64).reshape(-1, d)) if len(diag) else None
    K = 0 if f is None else f.shape[0]
    h = g = None
    if string is not None:
        h, g = (np.ascontiguousarray(t, dtype=np.float64).reshape(d) for t in string)
    low = np.ascontiguousarray(lower, dtype=np.float64).reshape(d) if lower is not None else None
    addr = _addr(d_vec)
    n2, dim = C.c_double(), C.c_int64()
    pop = np.zeros((N, d))
    dd = np.zeros((K, K, N, N)) if K else None
    st = np.zeros((N, N)) if string is not None else None
    aa = np.zeros((N, N), dtype=np.complex128) if low is not None else None
    check(lib().qbh_corr_qudit_repr_dev(N, d, int(total), int(p.shape[0]), _p(p), _p(ch.view(np.float64)), None if real else addr,
                                        addr if real else None, K, _p(f), _p(h), _p(g), _p(low), C.byref(n2), _p(pop), _p(dd), _p(st),
                                        _p(aa), C.byref(dim), stream), "qbh_corr_qudit_repr_dev")
    out = {"norm2": n2.value, "pop": pop}
    for k, a in (("dd", dd), ("str", st), ("aa", aa)):
        if a is not None:
            out[k] = a
    if normalize:
        _nonzero_norm(out["norm2"], "qudit_repr_correlations")
        for k in out:
            if k != "norm2":
                out[k] = out[k] / out["norm2"]
    out["dim"] = int(dim.value)
    return out


def _spin_s_tables(S):
    """(d, diag, string, lower) of spin_s_correlations: m = S - l, the den Nijs-Rommelse string for integer S, <l-1| S^+ |l>"""
    from . import qudit as qd
    two_s = qd._two_s(S)
    d, Sv = two_s + 1, two_s / 2.0
    m = Sv - np.arange(d)
    lower = np.real(np.append(0.0, np.diag(qd.spin_matrices(S)[1], 1)))            # <l-1| S^+ |l>
    string = (m, np.where(np.arange(d) % 2 == (two_s // 2) % 2, 1.0, -1.0)) if two_s % 2 == 0 else None      # (-1)^m, m = S - l
    return d, m, string, lower


def _normalized(out, who):
    _nonzero_norm(out["norm2"], who)
    for k in out:
        if k not in ("norm2", "dim") and out[k] is not None:
            out[k] = out[k] / out["norm2"]
    return out


def spin_s_repr_correlations(n_sites, S, two_sz, perms, chars, d_vec, real=False, normalize=True):
    """spin_s_correlations for a state of a MOMENTUM SECTOR of csr_mat.spin_heisenberg's d-level form (rows of qudit_repr for the
    charge of 2 S^z = two_sz): the same dict plus dim, from the representatives alone (qudit_repr_correlations); string is the
    den Nijs-Rommelse correlator averaged over the group."""
    from . import qudit as qd
    d, m, string, lower = _spin_s_tables(S)
    raw = qudit_repr_correlations(n_sites, d, qd.spin_charge(n_sites, S, two_sz), perms, chars, d_vec, diag=(m,), string=string,
                                  lower=lower, real=real, normalize=False)
    out = _spin_s_from_raw(S, raw)
    out["dim"] = raw["dim"]
    return _normalized(out, "spin_s_repr_correlations") if normalize else out


def bose_repr_correlations(n_sites, n_bosons, n_max, perms, chars, d_vec, real=False, normalize=True):
    """bose_correlations for a state of a MOMENTUM SECTOR (rows of csr_mat.bose_hubbard_repr for the same n_sites, n_bosons, n_max, perms, chars): the same
    dict plus dim, from the representatives alone (qudit_repr_correlations)."""
    n = np.arange(n_max + 1, dtype=np.float64)
    raw = qudit_repr_correlations(n_sites, n_max + 1, n_bosons, perms, chars, d_vec, diag=(n,),
                                  string=(np.ones(n_max + 1), 1.0 - 2.0 * (np.arange(n_max + 1) % 2)), lower=np.sqrt(n), real=real,
                                  normalize=False)
    out = _bose_from_raw(n_max, raw)
    out["dim"] = raw["dim"]
    return _normalized(out, "bose_repr_correlations") if normalize else out


_KONDO_GROUPS = ("dens", "docc", "sz_local", "nn", "zn", "zz_ll", "hop", "pm_ee", "pm_ll", "pm_le")


def _kondo_derived(out):
    """the derived quantities of kondo_correlations, each where its inputs are present (host arithmetic on the raw groups)"""
    if "dens" in out:
        out["sz_elec"] = 0.5 * (out["dens"][0] - out["dens"][1])
    if "zn" in out:
        out["zz_le"] = 0.5 * (out["zn"][0] - out["zn"][1])
    if "nn" in out:
        nn = out["nn"]
        out["zz_ee"] = 0.25 * (nn[0] - nn[1] - nn[2] + nn[3])
    if "zz_ll" in out and "pm_ll" in out:
        out["ss_ll"] = out["zz_ll"] + out["pm_ll"].real
    if "zz_ee" in out and "pm_ee" in out:
        out["ss_ee"] = out["zz_ee"] + out["pm_ee"].real
    if "zz_le" in out and "pm_le" in out:
        out["ss_le"] = out["zz_le"] + out["pm_le"].real
    if "ss_ll" in out and "ss_ee" in out and "ss_le" in out:
        out["total_spin"] = float(np.sum(out["ss_ll"] + out["ss_ee"] + 2.0 * out["ss_le"]))
    return out


def kondo_correlations(n_sites, n_elec, two_sz, d_vec, real=False, normalize=True, want=_KONDO_GROUPS, stream=None):
    """Every one- and two-site expectation value of a Kondo-lattice state (basis, operator order and signs of csr_mat.kondo /
    moprXvec_kondo: words u | d << n | s << 2n ascending), one pass over the state and no second vector: qbh_corr_kondo_dev.
    d_vec: device address (or DeviceVec) of the WHOLE sector (n_elec, two_sz), complex128, or its packed real parts (real=True).
    want: the groups to compute (a group left out costs nothing, its passes and gathers are not issued).  S is the local spin, s
    the electron's.  Raw groups: norm2; dens[2][N] = <n_{i,s}>; docc[N] = <n_up n_dn>; sz_local[N] = <S^z_i>; nn[4][N][N]
    (uu, ud, du, dd); zn[2][N][N] = <S^z_i n_{j,s}>; zz_ll[N][N] = <S^z_i S^z_j>; hop[2][N][N] = <c+_{i,s} c_{j,s}>; pm_ee =
    <s^+_i s^-_j>; pm_ll = <S^+_i S^-_j>; pm_le[i][j] = <S^+_i s^-_j> (all ordered pairs, not Hermitian).  Derived, each where its
    inputs were asked for: sz_elec = (n_up - n_dn) / 2; zz_le[i][j] = <S^z_i s^z_j>; zz_ee = <s^z_i s^z_j>; ss_ll, ss_ee, ss_le =
    zz + Re pm (<S_i . S_j>, <s_i . s_j>, <S_i . s_j>; ss_le[i][i] is the Kondo singlet); total_spin = <S_tot^2>.  With normalize
    the arrays are divided by norm2 (norm2 itself is returned as measured)."""
    N = int(n_sites)
    want = set(want)
    unknown = want - set(_KONDO_GROUPS)
    if unknown:
        raise ValueError("kondo_correlations: unknown group(s) %s" % sorted(unknown))
    addr = _addr(d_vec)
    n2 = C.c_double()
    bufs = _kondo_buffers(N, want)
    check(lib().qbh_corr_kondo_dev(N, int(n_elec), int(two_sz), None if real else addr, addr if real else None, C.byref(n2),
                                   *[_p(a) for a in bufs], stream), "qbh_corr_kondo_dev")
    return _kondo_result(n2.value, bufs, want, normalize, "kondo_correlations")


def _kondo_buffers(N, want):
    """the output arrays of the wanted groups in the order of the C calls (site, nn, zn, zz, hop, ee, ll, le), None where not wanted"""
    z = np.complex128
    return (np.zeros((4, N)) if want & {"dens", "docc", "sz_local"} else None,
            np.zeros((4, N, N)) if "nn" in want else None, np.zeros((2, N, N)) if "zn" in want else None,
            np.zeros((N, N)) if "zz_ll" in want else None, np.zeros((2, N, N), dtype=z) if "hop" in want else None,
            np.zeros((N, N), dtype=z) if "pm_ee" in want else None, np.zeros((N, N), dtype=z) if "pm_ll" in want else None,
            np.zeros((N, N), dtype=z) if "pm_le" in want else None)


def _kondo_result(norm2, bufs, want, normalize, who):
    """the dict of kondo_correlations from the filled arrays of _kondo_buffers"""
    site = bufs[0]
    out = {"norm2": norm2}
    if "dens" in want:
        out["dens"] = site[0:2].copy()
    if "docc" in want:
        out["docc"] = site[2].copy()
    if "sz_local" in want:
        out["sz_local"] = site[3].copy()
    for k, a in zip(("nn", "zn", "zz_ll", "hop", "pm_ee", "pm_ll", "pm_le"), bufs[1:]):
        if a is not None:
            out[k] = a
    _kondo_derived(out)
    if normalize:
        _nonzero_norm(out["norm2"], who)
        for k in out:
            if k != "norm2":
                out[k] = out[k] / out["norm2"]
    return out


def kondo_repr_correlations(n_sites, n_elec, two_sz, perms, chars, d_vec, real=False, normalize=True, want=_KONDO_GROUPS, stream=None):
    """kondo_correlations for a state of a MOMENTUM SECTOR: d_vec is indexed like the rows of csr_mat.kondo_repr / kondo_repr_mf for
    the same (n_sites, n_elec, two_sz, perms, chars) -- all orbit representatives, ascending -- and the result is what
    kondo_correlations gives on the unfolded full-space state, computed from the representatives in one pass per launch without a
    second vector (qbh_corr_kondo_repr_dev).  perms [n_trans][N] (element 0 the identity; reflections allowed), chars [n_trans]
    complex.  real=True: d_vec holds packed real parts; every character must be real.  Entries at representatives whose norm
    vanishes at this momentum (the decoupled fake rows) are ignored.  want and the returned keys as in kondo_correlations, plus dim,
    the number of representatives; kondo_energy_from_correlations, momentum_distribution and structure_factor take the arrays as
    they are."""
    N = int(n_sites)
    want = set(want)
    unknown = want - set(_KONDO_GROUPS)
    if unknown:
        raise ValueError("kondo_repr_correlations: unknown group(s) %s" % sorted(unknown))
    p = np.ascontiguousarray(perms, dtype=np.int32).reshape(-1, N)
    ch = np.ascontiguousarray(np.asarray(chars, dtype=np.complex128).reshape(-1))
    if ch.shape[0] != p.shape[0]:
        raise ValueError("kondo_repr_correlations: %d characters for %d translations" % (ch.shape[0], p.shape[0]))
    addr = _addr(d_vec)
    n2, dim = C.c_double(), C.c_int64()
    bufs = _kondo_buffers(N, want)
    check(lib().qbh_corr_kondo_repr_dev(N, int(n_elec), int(two_sz), int(p.shape[0]), _p(p), _p(ch.view(np.float64)),
                                        None if real else addr, addr if real else None, C.byref(n2), *[_p(a) for a in bufs],
                                        C.byref(dim), stream), "qbh_corr_kondo_repr_dev")
    out = _kondo_result(n2.value, bufs, want, normalize, "kondo_repr_correlations")
    out["dim"] = int(dim.value)
    return out


def kondo_energy_from_correlations(corr, terms, U=0.0):
    """<psi| H |psi> of the Kondo-lattice operator of a kondo.Terms (and U sum_i n_up n_dn) from the arrays of kondo_correlations,
    for ANY vector, in the units of `corr` (raw or normalised):  sum_hops (a_up hop[0][i][j] + a_dn hop[1][i][j]) + U sum docc +
    sum_i (kz_i zz_le[i][i] + kxy_i Re pm_le[i][i]) + sum_sbonds (bz zz_ll[i][j] + bxy Re pm_ll[i][j]).  The imaginary parts cancel
    for a Hermitian set of hops; the real part is returned."""
    e = 0.0 + 0.0j
    for (i, j, a_up, a_dn) in terms.hops:
        e += a_up * corr["hop"][0][int(i), int(j)] + a_dn * corr["hop"][1][int(i), int(j)]
    if U != 0.0:
        e += U * np.sum(corr["docc"])
    kz, kxy = np.asarray(terms.kz, dtype=np.float64), np.asarray(terms.kxy, dtype=np.float64)
    if np.any(kz != 0.0):
        e += np.sum(kz * np.diag(corr["zz_le"]))
    if np.any(kxy != 0.0):
        e += np.sum(kxy * np.diag(corr["pm_le"]).real)
    for (i, j, bz, bxy) in terms.sbonds:
        if bz != 0.0:
            e += bz * corr["zz_ll"][int(i), int(j)]
        if bxy != 0.0:
            e += bxy * corr["pm_ll"][int(i), int(j)].real
    return float(np.real(e))


# ------------------------------------------------------------------------------------------------------- host helpers --
def _phases(positions, qs):
    r, q = np.asarray(positions, dtype=float), np.asarray(qs, dtype=float)
    if r.ndim == 1:
        r = r[:, None]                                  # positions on a line
    if q.ndim == 1:
        q = q[:, None] if r.shape[1] == 1 else q[None, :]
    return np.exp(1j * (q @ r.T))                       # [n_q][N]: e^{i q . r_i}


def structure_factor(corr, positions, qs):
    """S(q) = (1/N) sum_ij e^{i q . (r_i - r_j)} corr[i][j] for a Hermitian N x N correlation matrix (ss, zz, nn_total, ...);
    positions [N][d] (or [N] in one dimension), qs [n_q][d].  Returns n_q real numbers."""
    c = np.asarray(corr)
    ph = _phases(positions, qs)
    return np.einsum("qi,ij,qj->q", ph, c, ph.conj()).real / c.shape[-1]


def momentum_distribution(hop, positions, ks):
    """n(k) = <c+_k c_k> = (1/N) sum_ij e^{i k . (r_i - r_j)} <c+_i c_j>, c+_k = N^{-1/2} sum_i e^{i k . r_i} c+_i.  hop: [N][N], or
    [2][N][N] for both species (returns [2][n_k])."""
    h = np.asarray(hop)
    if h.ndim == 3:
        return np.stack([momentum_distribution(x, positions, ks) for x in h])
    return structure_factor(h, positions, ks)


def energy_from_correlations(corr, bonds, J=1.0, t=1.0, U=0.0):
    """<psi| H |psi> from the two-site expectation values, for ANY vector (not only eigenvectors), in the units of `corr` (raw or
    normalised).  bonds: the list the operator was built from (a bond listed twice counts twice, as in csr_mat.heisenberg /
    csr_mat.hubbard).  Spin correlations (a dict with "pm"):    H = J sum_bonds S_i . S_j,  <H> = J sum_bonds (zz + Re pm).
    Fermion correlations (a dict with "hop" and "nn"):  H = -t sum_bonds,s (c+_i c_j + h.c.) + U sum_i n_up n_dn,
    <H> = -t sum_bonds,s 2 Re hop[s][i][j] + U sum_i nn_ud[i][i]."""
    b = np.asarray(bonds, dtype=np.int64).reshape(-1, 2)
    i, j = b[:, 0], b[:, 1]
    if "pm" in corr:
        return float(J * np.sum(corr["zz"][i, j] + corr["pm"][i, j].real))
    hop, nn = corr["hop"], corr["nn"]
    return float(-t * 2.0 * np.sum(hop[0][i, j].real + hop[1][i, j].real) + U * np.trace(nn[1]))
