"""Host-only checks of tests/secforms.py: the assembly of the sector operator against a second, sparse route (Psi^H O Psi) and against
the dense explicit projection of tests/test_gpu_hubrepr.py, the structural properties every case is there for (computed by the mirror
of qbh_mf_hubbard_repr's block structure), and fault injection: the per-row bound must reject a reference with one term dropped, one
sign flipped and one term moved to the neighbouring column, in the longest and in the shortest row.

Time here: the whole file about 30 s; the slowest tests are the second route of 4x4 with 4+2 (three momenta, three variants: 10 s) and of
4x4 with 5+2 (two momenta: 9 s; its full space has 524,160 words, more than the 3.8e5 of the other cases, and still fits) and the
dense projection (7 s).
"""
import itertools

import numpy as np
import pytest

import secforms as sf
from quantum_basis_amd import lattices

L = sf.L
TRIPLES = [(1.0, 0.0, 0.0), (-0.6, 0.8, 1.75)]


def _max_diff(A, B):
    D = (A - B).tocsr()
    return float(np.abs(D.data).max()) if D.nnz else 0.0


@pytest.mark.parametrize("case", list(sf.CASES))
def test_assembly_equals_the_projected_full_space_operator(case):
    """(a) = (b) to 1e-13 entry by entry for every momentum the GPU tests use and every variant; for the plain operator the
    full-space operator of (b) is fastham.hubbard_full itself, and the generalisation used for the variants must reproduce it."""
    spec = sf.CASES[case]
    op = sf.operator(case, "plain")
    F = sf.plain_operator(op["n"], spec["nu"], spec["nd"], op["bonds"], 1.0, op["U"])
    O = sf.full_operator(op["n"], spec["nu"], spec["nd"], op["terms"], op["U"])
    assert _max_diff(F, O) == 0.0
    for variant in spec["variants"]:
        opv = sf.operator(case, variant)
        Ov = O if variant == "plain" else sf.full_operator(opv["n"], spec["nu"], spec["nd"], opv["terms"], opv["U"], opv["pairs"])
        assert _max_diff(Ov, Ov.conj().T.tocsr()) < 1e-15                       # every variant is Hermitian
        alive = 0
        for ik in range(len(spec["ks"])):
            sec = sf.sector(case, ik, variant)
            d = _max_diff(sf.projected(sec, Ov), sf.merged_scipy(sec))
            assert d <= 1e-13, (case, variant, spec["ks"][ik], d)
            # the merged form: columns ascending and distinct, the diagonal always stored
            row = np.repeat(np.arange(sec.dim), np.diff(sec.ia))
            same = row[1:] == row[:-1]
            assert np.all(sec.ja[1:][same] > sec.ja[:-1][same]) and np.all(np.bincount(row[sec.ja == row], minlength=sec.dim) == 1)
            assert float(np.abs(sec.t_val).min()) >= 0.1 - 1e-15                 # no term is small enough to hide
            alive += int(sec.alive.sum())
        if case == "4x2_4+4" and variant == "plain":
            assert alive == O.shape[0] == 4900                                   # the eight sectors together span the full space


def test_assembly_equals_the_dense_explicit_projection():
    """The dense projection of tests/test_gpu_hubrepr.py (translation operators as matrices) on the 4x2 torus with 2+2 electrons
    (784 words, stabilised representatives and representatives without norm), all eight momenta, the anisotropic terms included."""
    from test_gpu_hubrepr import _sector_reference
    perms, shifts = lattices.translations(4, 2)
    terms = []
    for (i, j) in lattices.square(4, 2):
        a = -1.0 if abs(i - j) != 4 else -0.7
        terms += [(i, j, a, a * (1 + 0.25j)), (j, i, a, a * (1 - 0.25j))]
    total = 0
    for k in itertools.product(range(4), range(2)):
        chars = lattices.characters(shifts, k, (4, 2))
        reps, alive, Hk = _sector_reference(8, 2, 2, terms, 1.3, perms, chars)
        sec = sf.build(8, 2, 2, perms, chars, terms, 1.3)
        assert list(sec.reps) == reps and np.array_equal(sec.alive, alive)
        assert np.abs(sf.merged_scipy(sec).toarray() - Hk).max() <= 1e-13, k
        total += int(alive.sum())
    assert total == 28 * 28


@pytest.mark.parametrize("case", list(sf.CASES))
def test_every_case_has_the_structure_it_is_there_for(case):
    """The table of tests/test_gpu_secforms.py, re-derived by the mirror for every momentum and variant of the case."""
    want = sf.PROPERTIES[case]
    for (c, ik, variant) in sf.all_keys():
        if c != case:
            continue
        sec = sf.sector(case, ik, variant)
        b = sf.blocks(sec)
        what = (case, ik, variant)
        # the mirror's block rule against the enumeration of the representatives
        cnt = np.bincount(np.searchsorted(b.d, sec.dns[sec.row_d]), minlength=len(b.d))
        assert np.array_equal(cnt, b.nrows) and b.row0[-1] == sec.dim, what
        assert sec.cu == want["cu"], what
        got = dict(regular=int(b.regular.sum()), stabilised=int((~b.regular).sum()), w_up=b.w_up, max_nhop=int(b.nhop.max()),
                   flagged=int(b.flagged.sum()), n_rrows=b.n_rrows, n_trans=sec.G)
        for key, v in want.items():
            if key in got:
                assert got[key] == v, (what, key, got[key], v)
        for tile, n in want.get("items_per_block", {}).items():
            bt = sf.blocks(sec, tile)
            assert np.all(bt.items[bt.regular] == n), (what, tile, bt.items)
            if tile in want.get("last_item", {}):
                assert sec.cu - (n - 1) * tile == want["last_item"][tile], what
        # regular blocks hold every up pattern; a stabilised block fewer; no block is empty
        assert np.all(b.nrows[b.regular] == sec.cu) and np.all(b.nrows[~b.regular] < sec.cu) and b.nrows.min() > 0, what
        assert b.nhop.max() <= 128 and sec.G <= 64
        if variant == "aniso":
            assert b.n_amp_up == 2 and b.has_number_terms, what              # a second up amplitude (ext slots), number terms
        else:
            # (the 4x2 torus lists its y bonds twice: -2t beside -t)
            assert b.n_amp_up == (2 if case == "4x2_4+4" else 1) and not b.has_number_terms, what
        assert b.complex_hop == (variant == "peierls"), what                   # a down-hop amplitude that is complex by itself
        if case == "4x3_4+3":
            # j = 1 with a partial last wavefront; exactly two rounds of eight up hops; a second, partial round of down hops
            assert 495 == 256 + 3 * 64 + 47 and b.w_up == 16 and 8 < b.nhop.max() < 16
            bt = sf.blocks(sec, 256)
            assert bt.n_items == 2 * 18 + int(bt.items[~bt.regular].sum()) and bt.n_items > 2 * 8      # sec_grid = 8: workgroups take several items
        if case == "4x4_4+2":
            assert 1820 == 1024 + 796 and 796 == 3 * 256 + 28 and set(b.nhop[b.regular & ~b.flagged]) == {8}     # one full round, no more
            assert len(b.rows_reg) > 0 and len(b.rows_stab) > 0                    # remainder rows of both kinds
            assert sec.dim > 13000
        if case == "4x4_5+2":
            assert 4368 == 4 * 1024 + 272 and 16 < b.w_up <= 24                    # three rounds of up hops, the last partial
        if case == "13x1_6+2":
            assert b.rnnz == 0 and np.all(b.regular) and 1716 == 1024 + 692
        if case == "ring10_4+3":
            # a non-commuting group: rotation then reflection differs from reflection then rotation
            p = sec.perms
            assert not np.array_equal(p[1][p[10]], p[10][p[1]])
            assert len({tuple(np.nonzero(sec.img_u[:, r] == sec.ups[r])[0]) for r in range(sec.cu)}) >= 3      # several stabiliser kinds


REAL_MOMENTA = {"4x2_4+4": 4, "4x3_4+3": 2, "4x4_4+2": 2, "4x4_5+2": 1, "13x1_6+2": 1, "ring10_4+3": 2}


def test_momenta_are_of_the_kind_the_table_names():
    """has_real_characters asks for imaginary parts that are exactly zero: the number of momenta the real-form tests run at is
    pinned here, so that a change of lattices.characters cannot quietly take some away."""
    for case, spec in sf.CASES.items():
        real = [sf.has_real_characters(case, ik) for ik in range(len(spec["ks"]))]
        assert real[0] and sum(real) == REAL_MOMENTA[case], (case, real)
        if spec["lat"][0] != "ring":
            assert not all(real), case                                         # one momentum is genuinely complex
    assert all(len(s["ks"]) in (2, 3, 8) for s in sf.CASES.values())


@pytest.mark.parametrize("case,ik,variant", [("4x3_4+3", 2, "peierls"), ("4x4_4+2", 1, "aniso"), ("ring10_4+3", 1, "plain")])
def test_row_bound_accepts_double_precision_and_rejects_a_wrong_term(case, ik, variant):
    """A product formed in plain double precision lies within every row's bound and both reduction bounds; one term dropped,
    sign-flipped or moved to the neighbouring column, in the longest and in the shortest row, does not."""
    sec = sf.sector(case, ik, variant)
    x, y0 = sf.probe_vector(sec.dim, 1), sf.probe_vector(sec.dim, 2)
    sums = sf.row_sums(sec, x)
    longest, shortest = int(np.argmax(sec.terms_row)), int(np.argmin(sec.terms_row))
    assert sec.terms_row[shortest] >= 1
    for alpha, beta, gamma in TRIPLES:
        ref = sf.reference(sec, sums, x, y0, alpha, beta, gamma)

        def product(ja, val):
            s = np.zeros(sec.dim, dtype=np.complex128)
            np.add.at(s, np.repeat(np.arange(sec.dim), np.diff(sec.t_ia)), val.astype(np.complex128) * x[ja])
            return alpha * s + beta * y0 + gamma * x
        y = product(sec.t_ja, sec.t_val)
        i, ratio, over, err = sf.worst(y, ref)
        assert ratio <= 1.0 and over == 0, (i, ratio)
        assert abs(np.vdot(x, y) - complex(ref["dot"])) <= float(ref["t_dot"])
        assert abs(np.vdot(y, y).real - float(ref["nrm"])) <= float(ref["t_nrm"])
        for row in (longest, shortest):
            for how in ("dropped", "flipped", "moved"):
                ja, val = sf.tampered(sec, row, how)
                i, ratio, over, err = sf.worst(product(ja, val), ref)
                assert i == row and over == 1 and ratio > 1e6, (row, how, i, ratio, over)


def test_value_bound_rejects_a_wrong_value():
    """The bound on the generator's stored values: a value one part in 1e12 off, or a conjugated one, is outside it."""
    sec = sf.sector("4x3_4+3", 2, "peierls")
    vb = sf.value_bound(sec)
    v = sec.val.astype(np.complex128)
    assert np.all(np.abs(v.astype(sf.CL) - sec.val) <= vb)
    p = int(np.argmax(np.abs(v.imag)))
    assert abs(np.conj(v[p]) - sec.val[p]) > 1e6 * vb[p] and abs(v[p] * (1 + 1e-12) - sec.val[p]) > vb[p]
