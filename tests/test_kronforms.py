"""Host-only checks of tests/kronforms.py: the generator's structure, the path coverage of the profiles, the hand-worked values of the
mirror, and fault injection: the per-row bounds and both reduction bounds must reject a dropped, doubled or misplaced term."""
import numpy as np
import pytest

import kronforms as kf

L = kf.L
TRIPLES = [(1.0, 0.0, 0.0), (-0.6, 0.8, 1.75)]

# what each profile is there for: the test fails when a profile stops reaching its path
REACHES = {
    "tiny": {"one_block_pass", "empty_xcd_region", "sliced"},
    "uniform": {"sliced", "cols16_near", "cols16_far", "two_chunks_per_region"},
    "graded": {"sliced", "cols16_near", "cols16_far", "two_chunks_per_region"},
    "edge": {"cross_rows", "cross_own_arrays", "tile_edge", "tile8_ragged_nu", "sliced"},
    "edge_small": {"cross_rows", "cross_behind_far", "tile_edge"},
    "narrow": {"minor_below_8", "far_plain", "tile_edge", "cross_rows"},
    "ragged_light": {"sliced", "sliced_padded", "far_own_arrays"},
    "ragged_heavy": {"far_plain", "rows_no_far", "rows_no_near", "rows_empty"},
    "ragged_heavy_s2": {"sliced", "sliced_padded", "groups_empty", "rows_no_far", "rows_no_near", "rows_empty"},
    "far_1": {"far_64_groups", "far_direct_store"},
    "far_2": {"far_buffer_overflow"},
    "far_4": {"far_buffer_overflow"},
    # 64 rows per block: the four blocks of a chunk fill the 256-row buffer exactly, and open_block flushes only ABOVE 256.  A run
    # overflows only where one wavefront draws two neighbouring chunks, which depends on the run: nothing the mirror can promise
    "far_8": {"sliced"},
    "far_17": {"far_cut_groups"},
    "far_63": {"far_cut_groups", "far_group_at_limit"},
    "far_64": {"over_group_limit", "far_plain"},
    "near_200": {"near_window_by_maxlen", "near_tpr8", "near_rbase_tpr8"},
    "near_300": {"near_window_249", "near_tpr8"},
    "near_600": {"near_window_249", "near_rowpath", "near_tpr8"},
    "near_40": {"near_tpr4"},
    "far_plain_long": {"far_plain", "far_rowpath"},
    "wide_major": {"cols32_far_wide", "sliced"},
    "wide_minor": {"cols32_near_wide", "cols16_far"},
}


@pytest.mark.parametrize("name", kf.PROFILES)
def test_profile_structure_and_paths(name):
    dim, ia, ja, val, S, NU = kf.make(name)
    assert dim == NU * S
    near, far = kf.structure(ia, ja, S, dim)
    assert near.sum() + far.sum() == ia[-1] and far.sum() > 0
    a = np.abs(val) / (1.0 if kf.row_scale(name, dim) is None else np.repeat(kf.row_scale(name, dim), np.diff(ia)))
    assert a.min() >= 0.5 and a.max() <= 2.0
    r = kf.route(ia, ja, S, kf.profile_opts(name))
    assert r["active"] and r["kron_far_nnz"] + r["kron_cross_nnz"] == far.sum()
    assert ia[-1] <= 1.1e6
    got = kf.paths(ia, ja, S, kf.profile_opts(name))
    assert REACHES[name] <= got, "%s no longer reaches %s" % (name, sorted(REACHES[name] - got))
    assert got <= kf.ALL_PATHS


def test_profiles_cover_every_path():
    seen = set()
    for name in kf.PROFILES:
        dim, ia, ja, val, S, NU = kf.make(name)
        seen |= kf.paths(ia, ja, S, kf.profile_opts(name))
    assert seen == kf.ALL_PATHS, "paths no profile reaches: %s" % sorted(kf.ALL_PATHS - seen)
    assert set(REACHES) == set(kf.PROFILES)
    # the int32 forms of both parts of an operator that would otherwise take 2-byte columns
    dim, ia, ja, val, S, NU = kf.make("uniform")
    assert kf.route(ia, ja, S, dict(kron_cols16=0))["kron_cols16"] == 0
    for band in (2, 4, 8, 16):
        r = kf.route(ia, ja, S, dict(kron_band=band))
        assert r["kron_band"] == band and r["kron_sliced"] == int(band == 8) and r["kron_cols16"] == (3 if band == 8 else 1)


def test_mirror_hand_worked_values():
    # tiny: 2 x 8, one band of 8, one far entry per row: 2 groups of 8 slots, no padding, nothing across the band edge
    dim, ia, ja, val, S, NU = kf.make("tiny")
    r = kf.route(ia, ja, S)
    assert {k: r[k] for k in kf.INFO_FIELDS} == dict(kron_minor=8, kron_band=8, kron_sliced=1, kron_inplace=1, kron_far_nnz=16,
                                                      kron_cross_nnz=0, kron_cols16=3)
    assert list(r["gia"]) == [0, 8, 16] and r["nwb_n"] == 1 and r["nwb_f"] == 1 and not r["own_far"]
    # edge_small: 3 x 9: rows d = 8 are the narrow band; 24 rows x 2 far entries in 3 groups of 16 slots, 3 x 2 cross entries (< 32:
    # behind the far part, which therefore stays inside the operator's arrays and takes 2-byte columns), 27 x 2 near entries
    dim, ia, ja, val, S, NU = kf.make("edge_small")
    r = kf.route(ia, ja, S)
    assert {k: r[k] for k in kf.INFO_FIELDS} == dict(kron_minor=9, kron_band=8, kron_sliced=1, kron_inplace=1, kron_far_nnz=48,
                                                      kron_cross_nnz=6, kron_cols16=3)
    assert list(r["gia"]) == [0, 16, 32, 48] and r["nnz_n"] == 54 and not r["own_x"] and not r["own_far"]
    assert list(np.nonzero(r["cx"])[0]) == [8, 17, 26]
    # a shard of whole major indices keeps the band and the column width of the whole operator
    rs = kf.route(ia, ja, S, rows=(9, 27))
    assert (rs["NU"], rs["NUg"], rs["U0"], rs["kron_far_nnz"], rs["kron_cross_nnz"]) == (2, 3, 1, 32, 4)
    # an entry that changes both indices: unsplit
    bad = ja.copy()
    bad[ia[4]] = S + 5                                        # row (0, 4) gets a column (1, 5)
    assert not kf.route(ia, bad, S)["active"]
    # tile / orig of the band-major order, narrow band included: (u, d) = (1, 8) of 3 x 9 sits behind the 24 elements of band 0
    assert int(kf._tile(np.array([17]), 9, 3, 8)[0]) == 24 + 1 and int(kf._tile(np.array([9 + 3]), 9, 3, 8)[0]) == 8 + 3


def _fault_rows(name, ia, S, B, rng, allowed=None):
    nnz_row = np.diff(ia)
    ok = nnz_row > 0 if allowed is None else (nnz_row > 0) & allowed
    idx = np.nonzero(ok)[0]
    d = idx % S
    edge = idx[d >= (S // B) * B] if S % B else idx[d >= S - B]      # the narrow band, or the last band where none is narrow
    return [int(idx[np.argmax(nnz_row[idx])]), int(rng.choice(idx)), int(rng.choice(edge))]


@pytest.mark.parametrize("name", kf.PROFILES)
def test_bounds_reject_injected_faults(name):
    """In the reference: drop the smallest term of a row, double it, move it to the neighbouring row -- for the row with the most
    entries, a random row and a row of the edge band.  Every per-row bound must reject each (error / bound > 1), for the one-GPU
    constant and for the larger constants of the communicator and solver forms, and so must both reduction bounds.
    graded: the reductions sum rows whose scales differ by 2^40 and cannot see a row scaled by 2^-20 (that is what the per-row check
    is for); their rejection is asserted on the rows scaled by 2^10 or more, chosen the same way."""
    dim, ia, ja, val, S, NU = kf.make(name)
    r = kf.route(ia, ja, S, kf.profile_opts(name))
    x = kf.probe(name, dim, 1)
    y0 = kf.probe(name, dim, 2)
    s, abs_s = kf.row_sums(ia, ja, val, x)
    nnz_row = np.diff(ia)
    rng = np.random.default_rng(99)
    sc = kf.row_scale(name, dim)
    rows = _fault_rows(name, ia, S, r["B"], rng)
    red_rows = rows if sc is None else _fault_rows(name, ia, S, r["B"], rng, sc >= 1024.0)
    for alpha, beta, gamma in TRIPLES:
        for extra in (0, kf.COMBINE_EXTRA, kf.STEP_EXTRA):
            ref = kf.epilogue(s, abs_s, nnz_row, x, y0, alpha, beta, gamma, extra=extra)
            clean = ref["y"].astype(np.complex128)
            assert kf.worst(clean, ref)[1] <= 1.0
            for i in sorted(set(rows + red_rows)):
                p = np.arange(ia[i], ia[i + 1])
                terms = val[p].astype(kf.CL) * x[ja[p]].astype(kf.CL)
                k = int(np.argmax(np.abs(terms))) if (sc is not None and i in red_rows and i not in rows) else int(np.argmin(np.abs(terms)))
                t = L(alpha) * terms[k]
                j = i + 1 if i + 1 < dim else i - 1
                for fault, di, dj in (("dropped", -t, 0), ("doubled", t, 0), ("moved", -t, t)):
                    y = ref["y"].copy()
                    y[i] += di
                    y[j] += dj
                    got = y.astype(np.complex128)
                    what = "%s: term %d of row %d %s, (alpha, beta, gamma) = %r, extra %d" % (name, k, i, fault, (alpha, beta, gamma), extra)
                    ratio = kf.worst(got, ref)[1]
                    assert ratio > 1.0, "%s: error / bound %.3g" % (what, ratio)
                    if i in red_rows:
                        xl = x.astype(kf.CL)
                        dot = np.sum(np.conj(xl) * y)
                        nrm = np.sum(y.real * y.real + y.imag * y.imag)
                        assert abs(dot - ref["dot"]) > ref["t_dot"], "%s: <x, y> off by %.3e, bound %.3e" % (what, float(abs(dot - ref["dot"])), float(ref["t_dot"]))
                        assert abs(nrm - ref["nrm"]) > ref["t_nrm"], "%s: |y|^2 off by %.3e, bound %.3e" % (what, float(abs(nrm - ref["nrm"])), float(ref["t_nrm"]))


def test_step_bound_rejects_injected_faults():
    """The solver form: a fault in H v shows in the reconstruction b' v' + a v + b v_prev, in a and in b'."""
    name = "edge"
    dim, ia, ja, val, S, NU = kf.make(name)
    v = kf.probe(name, dim, 3)
    v /= np.linalg.norm(v)
    vp = kf.probe(name, dim, 4)
    s, abs_s = kf.row_sums(ia, ja, val, v)
    nnz_row = np.diff(ia)
    b = 1.3
    w = s - L(b) * vp.astype(kf.CL)
    a = float(np.sum(np.conj(v.astype(kf.CL)) * w).real)
    ref = kf.step_bound(s, abs_s, nnz_row, v, a, vp, b)
    assert abs(ref["a"] - a) <= ref["t_a"] and kf.worst(s.astype(np.complex128), ref)[1] <= 1.0
    rng = np.random.default_rng(5)
    for i in _fault_rows(name, ia, S, 8, rng):
        p = np.arange(ia[i], ia[i + 1])
        terms = val[p].astype(kf.CL) * v[ja[p]].astype(kf.CL)
        t = terms[int(np.argmin(np.abs(terms)))]
        for di, dj in ((-t, 0), (t, 0), (-t, t)):
            y = s.copy()
            y[i] += di
            y[i + 1 if i + 1 < dim else i - 1] += dj
            assert kf.worst(y.astype(np.complex128), ref)[1] > 1.0
            wf = y - L(b) * vp.astype(kf.CL)
            af = np.sum(np.conj(v.astype(kf.CL)) * wf).real
            assert abs(af - ref["a"]) > ref["t_a"]
            res = wf - L(a) * v.astype(kf.CL)
            bf = np.sqrt(np.sum(res.real ** 2 + res.imag ** 2))
            assert abs(bf - ref["b"]) > ref["t_b"]
