"""CPU tier of tests/genforms.py: the vectorised references against the Python loops of tests/fastham.py, the permutation
P D H D P^T against tests/refham.py on every reorder case (the conventions check, without a GPU), the survey's checksums through
that path, the comparator against the faults it is there to catch, and -- on the references -- every property a case of
tests/test_gpu_genforms.py relies on to reach its kernel branch.  No GPU needed."""
import math

import numpy as np
import pytest

import fastham
import genforms as gf
import refham

FASTHAM_HEIS = [k for k, (L, nd, b, J) in gf.HEIS_GEN.items() if math.comb(L, nd) * len(b) <= 500000]


@pytest.mark.parametrize("name", sorted(gf.HUBBARD_GEN))
def test_vectorised_hubbard_is_fastham_entry_by_entry(name):
    L, nu, nd, bonds, t, U = gf.HUBBARD_GEN[name]
    dim, ia, ja, val = gf.fastham_csr(fastham.hubbard_full(L, nu, nd, bonds, t, U))
    got = gf.hubbard_gen_case(name)
    assert got[0] == dim == math.comb(L, nu) * math.comb(L, nd)
    gf.assert_same_csr(got[1:], (ia, ja, val), exact=True)


@pytest.mark.parametrize("name", FASTHAM_HEIS)
def test_vectorised_heisenberg_is_fastham_entry_by_entry(name):
    """both sum the diagonal over the merged bonds in the same order: exact at every J"""
    L, nd, bonds, J = gf.HEIS_GEN[name]
    dim, ia, ja, val = gf.fastham_csr(fastham.heisenberg_full(L, nd, bonds, J))
    got = gf.heis_gen_case(name)
    assert got[0] == dim == math.comb(L, nd)
    gf.assert_same_csr(got[1:], (ia, ja, val), exact=True)


def test_every_heisenberg_case_is_pinned_by_fastham_or_by_its_counts():
    assert set(gf.HEIS_GEN) - set(FASTHAM_HEIS) == {"long17"}
    assert "192_bonds" in FASTHAM_HEIS and "L63_2" in FASTHAM_HEIS and "L34_33" in FASTHAM_HEIS


# ------------------------------------------------------------------------------ conventions
def _generator_operator(kind, name):
    """fastham's loops where they finish in a second or two, the vectorised assembly (pinned to fastham above) beyond"""
    if kind == 1:
        L, nu, nd, bonds = gf.REF_ELECTRON[name]
        return gf.fastham_csr(fastham.hubbard_full(L, nu, nd, bonds, 1.0, 1.1))
    L, nd, bonds = gf.REF_SPIN[name]
    if math.comb(L, nd) * len(bonds) <= 500000:
        return gf.fastham_csr(fastham.heisenberg_full(L, nd, bonds, 1.0))
    return gf.spin_gen(name)


@pytest.mark.parametrize("name", sorted(gf.REF_ELECTRON))
def test_permuted_generator_operator_is_refhams_electron_operator(name):
    L, nu, nd, bonds = gf.REF_ELECTRON[name]
    dim, ia, ja, val = _generator_operator(1, name)
    gf.assert_same_csr(gf.electron_gen(name)[1:], (ia, ja, val), exact=True)
    want = gf.electron_ref_full(name)
    assert want[0] == dim
    gf.assert_same_csr(gf.permute_expected(ia, ja, val, 1, L, nu, nd), want[1:], exact=True)


@pytest.mark.parametrize("name", sorted(gf.REF_SPIN))
def test_permuted_generator_operator_is_refhams_spin_operator(name):
    L, nd, bonds = gf.REF_SPIN[name]
    dim, ia, ja, val = _generator_operator(0, name)
    want = gf.spin_ref_full(name)
    assert want[0] == dim
    gf.assert_same_csr(gf.permute_expected(ia, ja, val, 0, L, 0, nd), want[1:], exact=True)


def test_the_5x1_lattice_is_the_chain():
    """refham's own 5x1 square lattice names every site as its own y-neighbour; those bonds move nothing"""
    assert [b for b in refham.square_bonds(5, 1) if b[0] != b[1]] == gf.REF_ELECTRON["5x1_2+3"][3]
    dim, ia, ja, val, _ = refham.hubbard_csr(5, 1, 2, 3, t=1.0, U=1.1)
    want = gf.electron_ref_upper("5x1_2+3")
    assert dim == want[0]
    gf.assert_same_csr((ia, ja, val), want[1:], exact=True)


def test_lin_order_is_refhams_basis_order():
    """the keys themselves: the state at reference row r is refham's r-th basis state"""
    for (L, nu, nd) in [(9, 4, 3), (5, 2, 3), (8, 3, 5)]:
        order, _, _ = gf.lin_order(1, L, nu, nd)
        up, dn = gf.patterns(L, nu), gf.patterns(L, nd)
        word = np.zeros(len(order), dtype=np.int64)
        for s in range(L):
            word |= (((up[order // len(dn)] >> s) & 1) << (2 * s)) | (((dn[order % len(dn)] >> s) & 1) << (2 * s + 1))
        assert np.array_equal(word, refham.electron_basis(L, nu, nd))
    for (L, nd) in [(15, 6), (32, 2)]:
        order, _, _ = gf.lin_order(0, L, 0, nd)
        assert np.array_equal(gf.patterns(L, nd)[order], refham.spin_half_basis(L, nd))


def _upper_checksums(ia, ja, val):
    dim = len(ia) - 1
    rows = np.repeat(np.arange(dim), np.diff(ia))
    keep = ja >= rows
    uia = np.zeros(dim + 1, dtype=np.int64)
    np.cumsum(np.bincount(rows[keep], minlength=dim), out=uia[1:])
    return refham.csr_checksums(uia, ja[keep].astype(np.int64), val[keep])


def test_survey_checksums_hold_through_the_permutation():
    """the index checksums of the reference's own matrices (pinned on the device path in test_gpu_reforder.py)"""
    dim, ia, ja, val = gf.hubbard_gen(8, 4, 4, refham.square_bonds(4, 2), 1.0, 1.1)
    cs = _upper_checksums(*gf.permute_expected(ia, ja, val, 1, 8, 4, 4))
    assert (cs["sum_ia"], cs["sum_ja_w"]) == (104757230, 419558689)
    dim, ia, ja, val = gf.heisenberg_gen(16, 8, refham.chain_bonds(16), 1.0)
    cs = _upper_checksums(*gf.permute_expected(ia, ja, val, 0, 16, 0, 8))
    assert (cs["sum_ia"], cs["sum_ja_w"]) == (483762205, 1934832532)


# ------------------------------------------------------------------------------ sensitivity of the comparator
def _perturbations(ia, ja, val):
    """single faults of the expected arrays, each one entry, pointer or bit"""
    r = len(ia) // 2
    p = int(ia[r])
    assert ia[r + 1] - p >= 3 and ia[r] - ia[r - 1] >= 1
    out = {}
    v = val.copy()
    k = p if ja[p] != r else p + 1
    assert v[k] != 0
    v[k] = -v[k]
    out["sign of one value"] = (ia, ja, v)
    j, v = ja.copy(), val.copy()
    j[[p, p + 1]] = j[[p + 1, p]]
    v[[p, p + 1]] = v[[p + 1, p]]
    out["two adjacent columns swapped with their values"] = (ia, j, v)
    i = ia.copy()
    i[r] += 1
    out["one row pointer off by one"] = (i, ja, val)
    i = ia.copy()
    i[r] -= 1                                         # the last entry of row r - 1 now belongs to row r: arrays untouched
    out["one entry moved to the neighbouring row"] = (i, ja, val)
    v = val.copy()
    d = int(np.flatnonzero((ja[ia[r]:ia[r + 1]] == r))[0]) + p
    assert v[d].real != 0
    v[d] = complex(np.nextafter(v[d].real, np.inf), v[d].imag)
    out["one diagonal value changed in the last bit"] = (ia, ja, v)
    return out


@pytest.mark.parametrize("exact", [True, False])
def test_comparator_rejects_every_single_fault(exact):
    # 3x3 with 4 + 3 at U = 4: row dim / 2 has hops on both sides of a non-zero diagonal
    dim, ia, ja, val = gf.hubbard_gen_case("3x3_4+3_t0.7_U4")
    tol = None if exact else 4 * gf.EPS
    gf.assert_same_csr((ia.copy(), ja.copy(), val.copy()), (ia, ja, val), exact, tol)
    faults = _perturbations(ia, ja, val)
    assert len(faults) == 5
    for what, bad in faults.items():
        if not exact and what.endswith("last bit"):
            gf.assert_same_csr(bad, (ia, ja, val), exact, tol)          # one ulp of a diagonal of order 4 is inside 4 eps: by design
            continue
        with pytest.raises(AssertionError, match="first differing row"):
            gf.assert_same_csr(bad, (ia, ja, val), exact, tol)


def test_comparator_names_the_row_and_prints_both_sides():
    dim, ia, ja, val = gf.hubbard_gen_case("3x3_4+3")
    v = val.copy()
    v[ia[77]] = 5.0
    with pytest.raises(AssertionError) as e:
        gf.assert_same_csr((ia, ja, v), (ia, ja, val), exact=True)
    assert "first differing row 77" in str(e.value) and "got " in str(e.value) and "want " in str(e.value)
    with pytest.raises(AssertionError, match="rows, expected"):
        gf.assert_same_csr((ia[:-1], ja, val), (ia, ja, val), exact=True)


# ------------------------------------------------------------------------------ the edges the GPU cases rely on
def test_long_row_operators_straddle_the_tile_of_k_ref_fill():
    dim, ia, ja, val = gf.electron_gen("long13")
    assert (dim, int(ia[-1])) == (gf.LONG13_DIM, gf.LONG13_NNZ) == (133848, 8370648)
    assert gf.row_histogram(ia) == gf.LONG13_ROWS == {60: 3360, 61: 19824, 62: 42000, 63: 42936, 64: 21504, 65: 4224}
    assert min(gf.LONG13_ROWS) < gf.REF_MAX_ROW and gf.REF_MAX_ROW in gf.LONG13_ROWS and gf.REF_MAX_ROW + 1 in gf.LONG13_ROWS
    assert dim > gf.TRIP_GEN_HUBBARD and gf.LONG13["L"] % 2 == 1             # a second trip of k_gen_hubbard, an odd site count
    assert gf.electron_gen("long13") is gf.electron_gen("long13")              # built once, shared
    dim, ia, ja, val = gf.spin_gen("long17")
    assert (dim, int(ia[-1])) == (gf.LONG17_DIM, gf.LONG17_NNZ) == (24310, 1594450)
    assert gf.row_histogram(ia) == gf.LONG17_ROWS == {64: 2002, 65: 9009, 66: 10296, 67: 3003}
    assert gf.heis_gen_case("long17")[1][-1] == gf.LONG17_NNZ
    # in the reference's order the rows are the same rows: the inverse direction sees the same lengths
    rdim, ria, rja, rval = gf.electron_ref_full("long13")
    assert gf.row_histogram(ria) == gf.LONG13_ROWS


def test_the_larger_spin_case_needs_second_trips():
    L, nd, bonds = gf.REF_SPIN["chain23_11"]
    dim = math.comb(L, nd)
    assert dim == gf.CHAIN23_DIM == 1352078 and dim > gf.TRIP_REF_FILL > gf.TRIP_REF_KEYS and dim < 2 * gf.TRIP_REF_FILL
    assert gf.TRIP_REF_KEYS == 524288 and gf.TRIP_REF_FILL == 1048576 and gf.TRIP_GEN_HUBBARD == 131072
    assert dim + 2 * len(bonds) * math.comb(L - 2, nd - 1) == 17577014        # about 1.8e7 entries


def test_keys_and_site_counts_of_the_reorder_cases():
    odd = [k for k, c in gf.REF_ELECTRON.items() if c[0] % 2 == 1]
    assert {"3x3_4+3", "3x3_2+5", "5x1_2+3", "chain31_1+1", "long13"} <= set(odd) and "4x2_3+5" in gf.REF_ELECTRON
    assert any(c[1] != c[2] and c[1] % 2 == 1 and c[2] % 2 == 1 for c in gf.REF_ELECTRON.values())       # unequal, odd particle numbers
    keys, sign = gf.lin_keys(1, 31, 1, 1)
    assert int(keys.max()).bit_length() == 62 and len(keys) == 961
    keys, _ = gf.lin_keys(0, 32, 0, 2)
    assert int(keys.max()).bit_length() == 32                                  # bit 31 of a 32-bit key
    for name, (L, nu, nd, _) in gf.REF_ELECTRON.items():
        _, sign = gf.lin_keys(1, L, nu, nd)
        assert 0 < sign.sum() < len(sign), name                                                       # both signs occur
    assert gf.REF_SPIN["chain15_6"][0] % 2 == 1 and gf.REF_SPIN["long17"][0] % 2 == 1 and gf.REF_SPIN["chain23_11"][0] % 2 == 1


def test_shards_sit_on_the_edges_they_are_named_for():
    L, nu, nd, bonds, t, U = gf.HUBBARD_GEN[gf.HUBBARD_SHARD_CASE]
    Nd, dim = math.comb(L, nd), math.comb(L, nu) * math.comb(L, nd)
    assert Nd == gf.HUBBARD_ND
    s = gf.HUBBARD_SHARDS
    assert s["first_row"] == (0, 1) and s["last_row"] == (dim - 1, dim)
    r0, r1 = s["inside_a_block"]
    assert r0 // Nd == (r1 - 1) // Nd and r0 % Nd and r1 % Nd
    r0, r1 = s["inside_to_boundary"]
    assert r0 % Nd and r1 % Nd == 0
    r0, r1 = s["boundary_to_inside"]
    assert r0 % Nd == 0 and r1 % Nd and r1 // Nd - r0 // Nd >= 2
    r0, r1 = s["boundary_to_boundary"]
    assert r0 % Nd == 0 and r1 % Nd == 0
    L, nd, bonds, J = gf.HEIS_SHARD_CASE
    assert math.comb(L, nd) == gf.HEIS_SHARD_DIM
    h = gf.HEIS_SHARDS
    assert h["first_row"] == (0, 1) and h["last_row"] == (gf.HEIS_SHARD_DIM - 1, gf.HEIS_SHARD_DIM)
    assert gf.HEIS_SHARD_START % 256 != 0
    for n in (gf.SCAN_CHUNK - 1, gf.SCAN_CHUNK, gf.SCAN_CHUNK + 1, 2 * gf.SCAN_CHUNK + 1):
        r0, r1 = h[str(n)]
        assert r0 == gf.HEIS_SHARD_START and r1 - r0 == n and r1 <= gf.HEIS_SHARD_DIM
    # the rows of a shard do not all have one length: a wrong offset shows in ia
    dim, ia, ja, val = gf.heisenberg_gen(*gf.HEIS_SHARD_CASE)
    assert len(gf.row_histogram(ia[301:301 + 2048])) > 1


def test_limits_of_the_heisenberg_generator_are_met_exactly():
    assert len(gf.merge(gf.HEIS_GEN["192_bonds"][2])) == gf.MAX_BONDS == 192
    assert len(gf.merge(gf.HEIS_REFUSED_BONDS[2])) == 193
    assert gf.HEIS_GEN["L63_2"][0] == 63 and int(gf.patterns(63, 2).max()).bit_length() == 63          # site 62: the top bit of a 63-site pattern
    assert gf.HEIS_GEN["L34_33"][:2] == (34, 33) and gf.HEIS_GEN["L40_3"][:2] == (40, 3)
    w = [x for _, x in gf.merge(gf.HEIS_GEN["repeated_bonds"][2])]
    assert sorted(set(w)) == [1.0, 2.0, 3.0, 4.0]                                                       # non-uniform weights
    for name, (L, nd, bonds, J) in gf.HEIS_GEN.items():
        assert math.comb(L, nd) < 2 ** 31 - 1 and L <= 63 and nd <= 33, name


def test_species_without_hops_and_weighted_bonds():
    for name in gf.HUBBARD_DIAGONAL_ONLY:
        dim, ia, ja, val = gf.hubbard_gen_case(name)
        assert dim == 1 and ia.tolist() == [0, 1] and ja.tolist() == [0]
    for name, species in [("no_up", 1), ("no_dn", 2), ("up_full", 1)]:
        L, nu, nd, bonds, t, U = gf.HUBBARD_GEN[name]
        assert len(gf.hop_entries(L, (nu, nd)[species - 1], bonds, t)[1]) == 0
        assert len(gf.hop_entries(L, (nu, nd)[2 - species], bonds, t)[1]) > 0
    assert dict(gf.merge(gf.HUBBARD_GEN["weight3"][3]))[(0, 1)] == 3.0
    dim, ia, ja, val = gf.hubbard_gen_case("weight3")
    assert np.any(np.abs(val.real) == abs(-0.7 * 3.0))                                                # -t * 3 among the hops


def test_drop_rule_of_the_heisenberg_reference():
    """|0.5 J w| < 1e-14 stores nothing off the diagonal; the bond still adds to the diagonal"""
    for name in ("J0", "J1e-15"):
        dim, ia, ja, val = gf.heis_gen_case(name)
        assert ia[-1] == dim and np.array_equal(ja, np.arange(dim))
    assert np.any(gf.heis_gen_case("J1e-15")[3] != 0)
    dim, ia, ja, val = gf.heis_gen_case("J1e-15_weight_over_the_rule")
    L, nd = 8, 3
    assert ia[-1] == dim + 2 * math.comb(L - 2, nd - 1) and abs(0.5 * 1e-15 * 30) >= gf.DROP > 0.5 * 1e-15


def test_hints_right_and_wrong():
    """the inverse direction's own check (k_ref_precheck), asked of the reference arrays on the CPU: every right hint has the
    product structure, the swapped fillings of the wrong-hint case do not"""
    for name in gf.INVERSE:
        L, nu, nd, _ = gf.REF_ELECTRON[name]
        dim, ia, ja, val = gf.electron_ref_upper(name)
        assert gf.product_structure(ia, ja, gf.lin_order(1, L, nu, nd)[0], math.comb(L, nd)), name
        assert math.comb(L, nd) >= 2 and math.comb(L, nu) >= 2
    name, (L, nu, nd) = gf.WRONG_HINT
    dim, ia, ja, val = gf.electron_ref_upper(name)
    assert math.comb(L, nu) * math.comb(L, nd) == dim and (nu, nd) == gf.REF_ELECTRON[name][1:3][::-1]
    assert not gf.product_structure(ia, ja, gf.lin_order(1, L, nu, nd)[0], math.comb(L, nd))


def test_long_double_product_and_its_bound():
    dim, ia, ja, val = gf.electron_ref_full("3x3_4+3")
    x = gf.probe_x(dim, 3)
    assert np.abs(x).min() >= 0.25 and np.abs(x).max() <= 1.0
    import scipy.sparse as sp
    y = sp.csr_matrix((val, ja, ia), shape=(dim, dim)) @ x
    gf.assert_multmv(y, ia, ja, val, x)
    y[dim // 2] *= 1 + 1e-13
    with pytest.raises(AssertionError, match="row %d" % (dim // 2)):
        gf.assert_multmv(y, ia, ja, val, x)
