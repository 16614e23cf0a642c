"""The device generators (qbh_gen.hip: k_gen_hubbard, k_heis_count, k_heis_fill, the closed-form row pointers) and the basis
reordering kernels (qbh_reorder.hip: k_ref_keys, k_ref_pos, k_ref_fill, k_inv_maps, k_ref_precheck) entry by entry against the host
references of tests/genforms.py, at the edges test_genforms.py asserts on those references: rows on both sides of k_ref_fill's
64-entry tile, odd site counts and unequal odd fillings, dimensions past one trip of every grid-stride loop, 62- and 32-bit keys,
species without hops, weighted bonds, the limits of qbh_gen_heisenberg (63 sites, n_dn = 33, 192 bonds), row shards around an up
block and around the scan chunk, and the |v| < 1e-14 drop rule.

Generated operators are compared with np.array_equal semantics (every amplitude is one IEEE product on both sides); only the
Heisenberg diagonal at J != 1 has a bound, genforms.heisenberg_diag_tol.  A permutation with sign flips rounds nothing: exact.
The inverse direction is checked through MultMv within (nnz_i + 8) eps (|H||x|)_i against a long-double product."""
import math

import numpy as np
import pytest

import quantum_basis_amd as q
from quantum_basis_amd import _lib

import genforms as gf

pytestmark = pytest.mark.gpu
PLAIN = dict(value_dict=0, real_fast_path=0, kron_split=0)


def _plain():
    return q.make_opts(**PLAIN)


def _hubbard(name, **kw):
    L, nu, nd, bonds, t, U = gf.HUBBARD_GEN[name]
    return q.csr_mat.hubbard(L, nu, nd, bonds, t=t, U=U, **kw)


def _heisenberg(name, **kw):
    L, nd, bonds, J = gf.HEIS_GEN[name]
    return q.csr_mat.heisenberg(L, nd, bonds, J=J, **kw)


def _heis_tol(ia, ja, bonds, J):
    """0 off the diagonal (one product), the summation bound on it"""
    rows = np.repeat(np.arange(len(ia) - 1, dtype=np.int64), np.diff(ia))
    return np.where(ja == rows, gf.heisenberg_diag_tol(bonds, J), 0.0)


def _assert_heis(got, want, bonds, J):
    if J in (1.0, 0.0):
        gf.assert_same_csr(got, want, exact=True)
    else:
        gf.assert_same_csr(got, want, exact=False, tol=_heis_tol(want[0], want[1], bonds, J))


# ------------------------------------------------------------------------------ generators, whole operators
@pytest.mark.parametrize("name", sorted(gf.HUBBARD_GEN))
def test_hubbard_generator_entry_by_entry(name):
    dim, ia, ja, val = gf.hubbard_gen_case(name)
    A = _hubbard(name, opts=_plain())
    assert (A.dim, A.ncols, A.row_offset, A.nnz) == (dim, dim, 0, ia[-1])
    gf.assert_same_csr(A.download(), (ia, ja, val), exact=True)
    A.destroy()


def test_hubbard_generator_past_one_trip_with_rows_around_64():
    """13 sites, 6 + 2 on the complete graph minus three bonds: dim 133,848 > 131,072 rows of one trip, rows of 60..65 entries"""
    L, nu, nd, bonds = gf.REF_ELECTRON["long13"]
    dim, ia, ja, val = gf.electron_gen("long13")
    A = q.csr_mat.hubbard(L, nu, nd, bonds, t=1.0, U=1.1, opts=_plain())
    assert (A.dim, A.nnz) == (gf.LONG13_DIM, gf.LONG13_NNZ)
    gf.assert_same_csr(A.download(), (ia, ja, val), exact=True)
    A.destroy()


@pytest.mark.parametrize("name", sorted(gf.HEIS_GEN))
def test_heisenberg_generator_entry_by_entry(name):
    """includes J = 0 and J = 1e-15 (nothing stored off the diagonal) and a weight that lifts 0.5 J w over the rule"""
    L, nd, bonds, J = gf.HEIS_GEN[name]
    dim, ia, ja, val = gf.heis_gen_case(name)
    A = _heisenberg(name, opts=_plain())
    assert (A.dim, A.ncols, A.row_offset, A.nnz) == (dim, dim, 0, ia[-1])
    _assert_heis(A.download(), (ia, ja, val), bonds, J)
    A.destroy()


def test_heisenberg_generator_refuses_beyond_its_limits():
    """all on the host, before any launch"""
    L, nd, bonds, J = gf.HEIS_REFUSED_BONDS                                   # 193 distinct bonds
    with pytest.raises(_lib.QbhError):
        q.csr_mat.heisenberg(L, nd, bonds, J=J, opts=_plain())
    with pytest.raises(_lib.QbhError):
        q.csr_mat.heisenberg(40, 34, gf.refham.chain_bonds(40), opts=_plain())          # n_dn = 34 (dim 3,838,380 would fit)
    with pytest.raises(_lib.QbhError):
        q.csr_mat.heisenberg(64, 1, gf.refham.chain_bonds(64), opts=_plain())


# ------------------------------------------------------------------------------ row shards
@pytest.mark.parametrize("shard", sorted(gf.HUBBARD_SHARDS))
def test_hubbard_row_shard_is_the_slice_of_the_reference(shard):
    r0, r1 = gf.HUBBARD_SHARDS[shard]
    ref = gf.hubbard_gen_case(gf.HUBBARD_SHARD_CASE)
    S = _hubbard(gf.HUBBARD_SHARD_CASE, rows=(r0, r1), opts=_plain())
    sia, sja, sval = gf.shard_of(ref, r0, r1)
    assert (S.dim, S.ncols, S.row_offset, S.nnz) == (r1 - r0, ref[0], r0, sia[-1]) and sia[0] == 0
    gf.assert_same_csr(S.download(), (sia, sja, sval), exact=True)
    S.destroy()


@pytest.mark.parametrize("shard", sorted(gf.HEIS_SHARDS))
def test_heisenberg_row_shard_is_the_slice_of_the_reference(shard):
    r0, r1 = gf.HEIS_SHARDS[shard]
    L, nd, bonds, J = gf.HEIS_SHARD_CASE
    ref = gf.heisenberg_gen(L, nd, bonds, J)
    S = q.csr_mat.heisenberg(L, nd, bonds, J=J, rows=(r0, r1), opts=_plain())
    sia, sja, sval = gf.shard_of(ref, r0, r1)
    assert (S.dim, S.ncols, S.row_offset, S.nnz) == (r1 - r0, ref[0], r0, sia[-1]) and sia[0] == 0
    _assert_heis(S.download(), (sia, sja, sval), bonds, J)
    S.destroy()


def test_bad_row_ranges_are_refused():
    L, nu, nd, bonds, t, U = gf.HUBBARD_GEN[gf.HUBBARD_SHARD_CASE]
    dim = math.comb(L, nu) * math.comb(L, nd)
    hl, hnd, hbonds, hJ = gf.HEIS_SHARD_CASE
    for rows in [(5, 5), (7, 3), (0, dim + 1), (dim, dim + 1)]:
        for mf in (False, True):
            with pytest.raises(_lib.QbhError):
                q.csr_mat.hubbard(L, nu, nd, bonds, rows=rows, opts=_plain(), matrix_free=mf)
    for rows in [(5, 5), (7, 3), (0, gf.HEIS_SHARD_DIM + 1), (gf.HEIS_SHARD_DIM, gf.HEIS_SHARD_DIM + 1)]:
        for mf in (False, True):
            with pytest.raises(_lib.QbhError):
                q.csr_mat.heisenberg(hl, hnd, hbonds, J=hJ, rows=rows, opts=_plain(), matrix_free=mf)


# ------------------------------------------------------------------------------ default format, matrix-free counts
@pytest.mark.parametrize("model,name", [("hubbard", "3x3_4+3_t0.7_U4"), ("heisenberg", "repeated_bonds_J0.7")])
def test_default_format_downloads_the_same_columns_and_value_bits(model, name):
    make = _hubbard if model == "hubbard" else _heisenberg
    P = make(name, opts=_plain())
    D = make(name)                                                            # default options: value codes
    assert D.info().value_dict > 0
    pia, pja, pval = P.download()
    dia, dja, dval = D.download()
    assert np.array_equal(dia, pia) and np.array_equal(dja, pja)
    assert np.array_equal(dval.view(np.uint64), pval.view(np.uint64))
    P.destroy()
    D.destroy()


@pytest.mark.parametrize("name", sorted(gf.HUBBARD_GEN))
def test_matrix_free_hubbard_reports_the_references_dimension_and_count(name):
    dim, ia, ja, val = gf.hubbard_gen_case(name)
    M = _hubbard(name, matrix_free=True)
    assert (M.dim, M.ncols, M.nnz) == (dim, dim, ia[-1])
    M.destroy()


@pytest.mark.parametrize("name", sorted(gf.HEIS_GEN))
def test_matrix_free_heisenberg_reports_the_references_dimension_and_count(name):
    """qbh_mf_heisenberg takes 62 sites at the most: the 63-site cases are refused (on the host); J = 0 and J = 1e-15 count no
    off-diagonal entry, as the stored operator holds none"""
    L, nd, bonds, J = gf.HEIS_GEN[name]
    if L > 62:
        with pytest.raises(_lib.QbhError):
            _heisenberg(name, matrix_free=True)
        return
    dim, ia, ja, val = gf.heis_gen_case(name)
    M = _heisenberg(name, matrix_free=True)
    assert (M.dim, M.ncols, M.nnz) == (dim, dim, ia[-1])
    M.destroy()


# ------------------------------------------------------------------------------ reference order, forward
def _forward(G, kind, L, nu, nd, gen, ref_full):
    R = G.reference_order(kind, L, nu, nd, opts=_plain())
    g = G.download()
    gf.assert_same_csr(g, gen[1:], exact=True)
    r = R.download()
    assert R.dim == ref_full[0] and R.nnz == ref_full[1][-1]
    gf.assert_same_csr(r, gf.permute_expected(g[0], g[1], g[2], kind, L, nu, nd), exact=True)      # (a) the kernels permuted what they were given
    gf.assert_same_csr(r, ref_full[1:], exact=True)                                                # (b) ... into the reference's operator
    R.destroy()
    G.destroy()


@pytest.mark.parametrize("name", sorted(gf.REF_ELECTRON))
def test_electron_operator_in_reference_order(name):
    """odd site counts, unequal and odd fillings, 62-bit keys; long13: rows of 60..65 entries, both branches of k_ref_fill"""
    L, nu, nd, bonds = gf.REF_ELECTRON[name]
    G = q.csr_mat.hubbard(L, nu, nd, bonds, t=1.0, U=1.1, opts=_plain())
    _forward(G, 1, L, nu, nd, gf.electron_gen(name), gf.electron_ref_full(name))


@pytest.fixture(scope="module")
def chain23():
    """the one larger case: its host references built once"""
    return gf.spin_gen("chain23_11"), gf.spin_ref_full("chain23_11")


@pytest.mark.parametrize("name", ["chain15_6", "chain32_2", "long17"])
def test_spin_operator_in_reference_order(name):
    """odd site counts, a 32-bit key with bit 31 set; long17: every row longer than the tile (64..67 entries)"""
    L, nd, bonds = gf.REF_SPIN[name]
    G = q.csr_mat.heisenberg(L, nd, bonds, J=1.0, opts=_plain())
    _forward(G, 0, L, 0, nd, gf.spin_gen(name), gf.spin_ref_full(name))


def test_spin_operator_in_reference_order_past_one_trip(chain23):
    """L = 23, n_dn = 11: dim 1,352,078 -- second trips of k_ref_keys / k_ref_pos (524,288 a trip) and k_ref_fill (1,048,576)"""
    L, nd, bonds = gf.REF_SPIN["chain23_11"]
    G = q.csr_mat.heisenberg(L, nd, bonds, J=1.0, opts=_plain())
    assert G.dim == gf.CHAIN23_DIM
    _forward(G, 0, L, 0, nd, chain23[0], chain23[1])


def test_reference_order_refuses_shards_codes_splits_and_other_bases():
    L, nu, nd, bonds, t, U = gf.HUBBARD_GEN["3x3_4+3"]
    for make in (lambda: q.csr_mat.hubbard(L, nu, nd, bonds, rows=(84, 840), opts=_plain()),            # a row shard
                 lambda: q.csr_mat.hubbard(L, nu, nd, bonds),                                           # value codes
                 lambda: q.csr_mat.hubbard(L, nu, nd, bonds, opts=q.make_opts(value_dict=0, real_fast_path=0, kron_split=2))):      # split
        G = make()
        with pytest.raises(_lib.QbhError):
            G.reference_order(1, L, nu, nd, opts=_plain())
        G.destroy()
    G = q.csr_mat.hubbard(L, nu, nd, bonds, opts=q.make_opts(value_dict=0, real_fast_path=0, kron_split=2))
    assert G.info().kron_minor == math.comb(L, nd)                             # ... it was the split that was refused
    G.destroy()
    G = q.csr_mat.hubbard(L, nu, nd, bonds, opts=_plain())
    for other in [(1, 9, 4, 4), (1, 10, 4, 3), (0, 9, 0, 4)]:                                            # another dimension
        with pytest.raises(_lib.QbhError):
            G.reference_order(*other, opts=_plain())
    G.destroy()


# ------------------------------------------------------------------------------ reference order, inverse
def _hint(L, nu, nd):
    return q.make_opts(basis_kind=_lib.BASIS_REF_FERMION2, n_sites=L, n_up=nu, n_dn=nd, kron_split=2, value_dict=0, real_fast_path=0)


@pytest.mark.parametrize("name", gf.INVERSE)
def test_reference_ordered_host_arrays_under_the_hint(name):
    """k_ref_keys, k_inv_maps, k_ref_precheck and k_ref_fill (long13: its long branch) in the inverse direction, and the signed
    scatter / gather of the vectors: y = H x comes back in the caller's order"""
    L, nu, nd, _ = gf.REF_ELECTRON[name]
    dim, ia, ja, val = gf.electron_ref_upper(name)
    A = q.csr_mat(dim, ia, ja, val, sym=True, opts=_hint(L, nu, nd))
    info = A.info()
    assert info.basis_internal == _lib.BASIS_REF_FERMION2 and (info.basis_n_sites, info.basis_n_up, info.basis_n_dn) == (L, nu, nd)
    x = gf.probe_x(dim, 11)
    y = np.empty(dim, dtype=np.complex128)
    A.MultMv(x, y)
    fdim, fia, fja, fval = gf.electron_ref_full(name)
    gf.assert_multmv(y, fia, fja, fval, x, what=name)
    A.destroy()


def test_a_wrong_hint_leaves_the_operator_as_given():
    name, (L, nu, nd) = gf.WRONG_HINT
    dim, ia, ja, val = gf.electron_ref_upper(name)
    A = q.csr_mat(dim, ia, ja, val, sym=True, opts=_hint(L, nu, nd))
    info = A.info()
    assert info.basis_internal == 0 and info.kron_minor == 0
    fdim, fia, fja, fval = gf.electron_ref_full(name)
    gf.assert_same_csr(A.download(), (fia, fja, fval), exact=True)
    x = gf.probe_x(dim, 12)
    y = np.empty(dim, dtype=np.complex128)
    A.MultMv(x, y)
    gf.assert_multmv(y, fia, fja, fval, x, what="wrong hint")
    A.destroy()
