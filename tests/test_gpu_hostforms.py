"""Operator creation from host arrays, entry by entry at its edges.

qbh_csr_create / qbh_csr_create_rows stream the caller's arrays through qbh_build.hip (mirror count, exclusive scan, fill, the two
sort kernels of the mirrored parts), may code the values (qbh_csrprep.hip k_dict_collect / k_dict_encode) and split a shard by
column when a communicator is attached (k_split_count / k_split_fill); qbh_csr_reference_order permutes a stored operator
(qbh_reorder.hip k_ref_fill).  Every case creates an operator from a profile of tests/hostforms.py, which asserts the edge it sits
on, and compares the download with the independent reference there: row pointers and columns exactly, values bit for bit
(hostforms.csr_mismatch; tests/test_hostforms.py shows that it rejects a swapped pair, a lost conjugation, a merged signed zero, a
last-bit neighbour, a shifted row pointer and a dropped sign).  Where the operator is applied, every row of y is compared with a
long-double reference within the row bound of tests/csrforms.py, the only tolerance in this file.

Which case reaches which branch:
  k_sort_lower_short / _long   a. mirror_lengths (L = 95, 96 | 97, 255, 256, 257, 600, 1500, several long rows with their tmp_off),
                               many_long (4100 long rows, grid 4096); b. a long row first / last in a shard, alone in a shard
  exclusive_scan               a. scan_edges(n), n = 1, 2, 2047, 2048, 2049, 4096, 4097, 6145; b. scan_edges(4097) shards
  staged upload                a. mirror_lengths under create_chunk = 1024 and 1500
  value dictionary             d. dict_n / dict_upper at 1, 255, 256, 257, 65535, 65536, 65537 bit patterns
  shard column split           e. two ranks (host-staged hooks; native communicator), 1-byte codes, 2-byte codes, uncoded
  k_ref_fill, rows > 64        f. reorder_long (kinds 0 and 1, even and odd number of sites)
  unseen inputs                a. unsorted (and its full-storage form through check_hermitian_host), full_storage;
                               b. full_storage with rows=, shards without a stored entry

Measured on an MI355X (47 cases, 11 s together): the largest error / bound seen is 0.188 (d. dict_n_65536; a. to c. stay below
0.19, e. at 0.142); the slowest cases are the two of e. (3.8 s and 2.7 s: two rank processes each), every other case takes at most
0.33 s (d. at 65535 to 65537 bit patterns, a. mirror_lengths).  No case found a fault in the library.
"""
import socket
import tempfile

import numpy as np
import pytest

import csrforms as cf
import hostforms as hf
import quantum_basis_amd as q
from quantum_basis_amd import _lib
from test_gpu_csrforms import _Run, _check_red

pytestmark = pytest.mark.gpu

BASE = dict(value_dict=0, real_fast_path=0, kron_split=0, basis_detect=0, autotune=0)
KERNELS = (cf.KERNEL_ROWS, cf.KERNEL_WAVE)


def _opts(name, **kw):
    o = dict(BASE)
    if name.startswith("scan_edges"):
        o["check_hermitian"] = 0                          # free row lengths: the profile is not Hermitian
    o.update(kw)
    return q.make_opts(**o)


def _create(name, rows=None, **kw):
    dim, ia, ja, val, sym, _ = hf.make(name)
    return q.csr_mat(dim, ia, ja, val, sym=bool(sym), opts=_opts(name, **kw), rows=rows)


def _reference(name, r0=0, r1=None):
    dim, ia, ja, val, sym, _ = hf.make(name)
    return hf.expand(dim, ia, ja, val, sym, r0, dim if r1 is None else r1)


def _assert_download(what, A, want):
    bad = hf.csr_mismatch(A.download(), want)
    assert bad is None, "%s: %s" % (what, bad)
    assert A.info().nnz == want[0][-1] == A.nnz, what


def _apply(what, A, want, x, r0, r1, kernel_name, red=True):
    """One y = 0.7 H x - 1.3 y + 0.5 x_local with its reductions against the long-double reference of the rows `want`; -> error / bound.
    red = False: the reductions are computed but not compared (a profile holding 1e300 overflows |y|^2 in any arithmetic)."""
    xl = x[r0:r1]
    y0 = hf.probe_vector(r1 - r0, 2)
    ref = hf.spmv_reference(want, x, xl, y0)
    run = _Run(A, x, len(x))
    try:
        y, (dot, nrm) = run(y0, *hf.TRIPLE, True)
    finally:
        run.free()
    i, ratio, over, err = cf.worst(y, ref)
    tag = "%s %s" % (what, kernel_name)
    assert ratio <= 1.0, "%s: row %d (length %d): |y - ref| = %.3e, bound %.3e, error / bound %.3g; %d rows over" % (
        tag, i, int(want[0][i + 1] - want[0][i]), err, float(ref["bound"][i]), ratio, over)
    if red:
        _check_red(tag, dot, nrm, ref)
    return ratio, y


# ---------------------------------------------------------------------------------------------- a. expansion, bit for bit --
EXPAND = ["mirror_lengths", "many_long", "unsorted", "full_storage"] + ["scan_edges_%d" % n for n in hf.SCAN_N]


@pytest.mark.parametrize("name", EXPAND)
def test_expansion_bit_for_bit(name):
    want = _reference(name)
    A = _create(name)
    try:
        dim = hf.make(name)[0]
        info = A.info()
        assert (info.nrows, info.ncols, info.row_offset) == (dim, dim, 0)
        _assert_download(name, A, want)
    finally:
        A.destroy()


def test_unsorted_full_storage_passes_the_hermitian_check_and_keeps_its_order():
    """Full storage whose rows are not sorted by column: check_hermitian_host falls back to its linear search, the device keeps
    every row in the order given."""
    dim = hf.make("unsorted")[0]
    fia, fja, fval = _reference("unsorted")
    assert any(np.any(np.diff(fja[fia[r]:fia[r + 1]]) < 0) for r in range(dim))
    A = q.csr_mat(dim, fia, fja, fval, sym=False, opts=q.make_opts(check_hermitian=1, **BASE))
    try:
        _assert_download("unsorted, full storage", A, (fia, fja, fval))
    finally:
        A.destroy()
    bad = fval.copy()
    k = int(np.argmax(fja != np.repeat(np.arange(dim), np.diff(fia))))
    bad[k] = np.conj(bad[k]) + 1e-9
    with pytest.raises(_lib.QbhError) as e:
        q.csr_mat(dim, fia, fja, bad, sym=False, opts=q.make_opts(check_hermitian=1, **BASE))
    assert e.value.code == -5


def test_expansion_does_not_depend_on_the_upload_chunk_or_the_atomic_order(monkeypatch):
    """mirror_lengths: the 1500 sources of one column arrive from ~30 chunks of 1024 nonzeros; chunks of 1500 end inside rows at
    other places.  Two creations under the default chunk give the same bytes (the mirrored parts arrive in atomic order)."""
    want = _reference("mirror_lengths")
    first = None
    for chunk in (None, None, "1024", "1500"):
        if chunk is not None:
            monkeypatch.setenv("QBH_DEBUG", "create_chunk=" + chunk)          # a measurement knob, not a form: the debug list
        A = _create("mirror_lengths")
        try:
            got = A.download()
        finally:
            A.destroy()
        bad = hf.csr_mismatch(got, want)
        assert bad is None, "create_chunk %s: %s" % (chunk, bad)
        if first is None:
            first = got
        assert all(a.tobytes() == b.tobytes() for a, b in zip(first, got)), chunk


# ------------------------------------------------------------------------------------------------------- b. row shards --
SHARDED = ["mirror_lengths", "full_storage", "scan_edges_4097"]


@pytest.mark.parametrize("name", SHARDED)
def test_row_shards_bit_for_bit(name):
    dim = hf.make(name)[0]
    for label, (r0, r1) in hf.shard_cuts(name).items():
        what = "%s rows [%d, %d) (%s)" % (name, r0, r1, label)
        assert 0 <= r0 < r1 <= dim, what
        want = _reference(name, r0, r1)
        A = _create(name, rows=(r0, r1))
        try:
            info = A.info()
            assert (info.nrows, info.ncols, info.row_offset) == (r1 - r0, dim, r0), what
            _assert_download(what, A, want)
        finally:
            A.destroy()


@pytest.mark.parametrize("value_dict", [0, 1])
def test_a_shard_without_a_stored_entry_is_an_operator_and_leaves_no_error_behind(value_dict):
    """nnz = 0 flows through the scan, the (skipped) dictionary and the geometry: y = beta y + gamma x_local, and an ordinary
    creation right afterwards succeeds (no sticky HIP error)."""
    dim, _, _, _, _, f = hf.make("mirror_lengths")
    x = hf.probe_vector(dim, 1)
    top = 0.0
    for r0, r1 in ((0, 1), (dim - 1, dim), (f["empty_run"][0], f["empty_run"][-1] + 1)):
        want = _reference("mirror_lengths", r0, r1)
        assert want[0][-1] == 0
        for k in KERNELS:
            A = _create("mirror_lengths", rows=(r0, r1), value_dict=value_dict, spmv_kernel=k)
            try:
                assert A.info().value_dict == 0
                _assert_download("empty shard [%d, %d)" % (r0, r1), A, want)
                ratio, y = _apply("empty shard [%d, %d)" % (r0, r1), A, want, x, r0, r1, cf.KERNEL_NAMES[k])
                top = max(top, ratio)
            finally:
                A.destroy()
        B = _create("mirror_small", value_dict=value_dict)
        try:
            _assert_download("creation after an empty shard", B, _reference("mirror_small"))
        finally:
            B.destroy()
    print("b. empty shards: largest error / bound %.3g" % top)


# -------------------------------------------------------------------------------------------- c. the operator applies --
@pytest.mark.parametrize("name", ["mirror_lengths", "unsorted"])
def test_the_created_operator_applies(name):
    """Unsorted host rows are supported as they are: no CSR kernel form relies on the column order inside a row (the forms that
    do, the Kronecker split and the basis map, are not created here and build their own order), so the rows stay as given and
    every y_i must be right."""
    dim = hf.make(name)[0]
    want = _reference(name)
    x = hf.probe_vector(dim, 1)
    top = 0.0
    for k in KERNELS:
        A = _create(name, spmv_kernel=k)
        try:
            assert A.info().kernel == k
            ratio, _ = _apply(name, A, want, x, 0, dim, cf.KERNEL_NAMES[k])
            top = max(top, ratio)
        finally:
            A.destroy()
    print("c. %s: largest error / bound %.3g" % (name, top))


@pytest.mark.parametrize("name", SHARDED)
def test_the_created_shards_apply(name):
    dim = hf.make(name)[0]
    x = hf.probe_vector(dim, 3)
    top = 0.0
    for label, (r0, r1) in hf.shard_cuts(name).items():
        want = _reference(name, r0, r1)
        for k in KERNELS:
            what = "%s rows [%d, %d) (%s)" % (name, r0, r1, label)
            A = _create(name, rows=(r0, r1), spmv_kernel=k)
            try:
                assert A.info().kernel == k
                ratio, _ = _apply(what, A, want, x, r0, r1, cf.KERNEL_NAMES[k])
                top = max(top, ratio)
            finally:
                A.destroy()
    print("c. %s shards: largest error / bound %.3g" % (name, top))


# --------------------------------------------------------------------------------------- d. value dictionary at its caps --
DICTS = (["dict_n_%d" % n for n in hf.DICT_N] + ["dict_upper_%d" % n for n in hf.DICT_N]
         + ["dict_n_256_real", "dict_n_257_real", "dict_upper_256_real", "dict_upper_65536_real"])


@pytest.mark.parametrize("name", DICTS)
def test_value_dictionary_at_its_caps(name):
    dim, ia, ja, val, sym, f = hf.make(name)
    n = f["n_values"]
    want = _reference(name)
    assert hf.distinct_bits(want[2]) == n
    x = hf.probe_vector(dim, 5)
    A0 = _create(name)                                             # uncoded
    try:
        assert A0.info().value_dict == 0
        ratio0, y_plain = _apply(name + " uncoded", A0, want, x, 0, dim, "auto", red=False)
    finally:
        A0.destroy()
    ref = hf.spmv_reference(want, x, x, hf.probe_vector(dim, 2))
    top, ys = ratio0, []
    for vd, cap in ((1, hf.DICT_MAX), (2, 256), (1, hf.DICT_MAX)):
        A = _create(name, value_dict=vd)
        try:
            what = "%s value_dict %d" % (name, vd)
            assert A.info().value_dict == (n if n <= cap else 0), "%s: info().value_dict = %d with %d bit patterns" % (
                what, A.info().value_dict, n)
            _assert_download(what, A, want)                        # a merged +0.0 / -0.0 or last-bit neighbour shows here
            ratio, y = _apply(what, A, want, x, 0, dim, "auto", red=False)
            top = max(top, ratio)
            # coded against uncoded: the same products of the same doubles, within the bound of one of them
            d = np.abs(y.astype(cf.CL) - y_plain.astype(cf.CL))
            assert np.all(d <= ref["bound"]), "%s: y differs from the uncoded operator's by %.3g bounds" % (
                what, float(np.max(d / np.maximum(ref["bound"], np.finfo(np.float64).tiny))))
            if vd == 1:
                ys.append(y)
        finally:
            A.destroy()
    assert hf.same_bits(ys[0], ys[1]), "%s: two creations give different y: the codes depend on the atomic order" % name
    print("d. %s (%d bit patterns, code width %d): largest error / bound %.3g" % (name, n, hf.code_width(n), top))


# ---------------------------------------------------------------------------- e. shard column split with each code width --
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


SPLIT = ["dict_n_255", "dict_n_257", "dict_n_65535", "mirror_lengths"]
# code widths of the two uniform shards: those of dict_n(257) hold 256 and 257 bit patterns, the two sides of the switch
SPLIT_WIDTHS = {"dict_n_255": (1, 1), "dict_n_257": (1, 2), "dict_n_65535": (2, 2)}


@pytest.mark.parametrize("native", [False, True], ids=["gloo_hooks", "native_communicator"])
def test_shard_column_split_with_each_code_width(native, monkeypatch):
    """The split is made when a communicator is attached to a row shard, and a one-rank communicator owns every column (its shard
    is the whole operator and is not split): two ranks on this GPU, through the host-staged hooks as test_gpu_dist.py runs them
    and through the library's native communicator on the librccl stand-in of test_gpu_native_ranks.py.  1-byte codes, 2-byte
    codes and complex128 values; the download is unchanged by the attachment and y is the unsharded reference's rows."""
    import torch.multiprocessing as mp
    import dist_worker
    world = 2
    if native:
        from test_rccl_stub import STUB, _stub
        _stub()                                                    # builds the stand-in when the .so is not there
        monkeypatch.setenv("QBH_RCCL_LIB", STUB)
        monkeypatch.setenv("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    for name, widths in SPLIT_WIDTHS.items():                      # the code widths the shards are claimed to reach
        dim = hf.make(name)[0]
        nblk = (dim + world - 1) // world
        for r in range(world):
            n_shard = hf.distinct_bits(_reference(name, r * nblk, min(dim, (r + 1) * nblk))[2])
            assert hf.code_width(n_shard) == widths[r], (name, r, n_shard)
    with tempfile.TemporaryDirectory() as tmp:
        if native:
            monkeypatch.setenv("TMPDIR", tmp)
        mp.spawn(dist_worker.gpu_hostforms_shards, args=(world, _free_port(), "gloo", tmp, SPLIT, native), nprocs=world, join=True)
        res = {(name, r): dict(np.load("%s/%s_%d.npz" % (tmp, name, r))) for name in SPLIT for r in range(world)}
    top = 0.0
    for name in SPLIT:
        dim = hf.make(name)[0]
        x = hf.probe_vector(dim, 11)
        y0 = hf.probe_vector(dim, 12)
        assert res[(name, 0)]["r0"] == 0 and res[(name, 0)]["r1"] == res[(name, 1)]["r0"] and res[(name, 1)]["r1"] == dim
        for r in range(world):
            d = res[(name, r)]
            r0, r1 = int(d["r0"]), int(d["r1"])
            what = "%s rank %d rows [%d, %d)" % (name, r, r0, r1)
            want = _reference(name, r0, r1)
            assert int(d["n_dict"]) == (hf.distinct_bits(want[2]) if name.startswith("dict_") else 0), what
            inside = (want[1] >= r0) & (want[1] < r1)
            assert inside.any() and not inside.all(), what         # both parts of the split hold entries
            # a split shard holds a second array of row pointers (qbh_csr_get_info: bytes_matrix counts the pointer arrays,
            # 4 bytes per column, the values or codes and 12 bytes per row block)
            nnz = int(want[0][-1])
            fixed = nnz * 4 + (nnz + 256 * 16 if int(d["n_dict"]) else nnz * 16)
            arrays = [(int(d["bytes_" + t]) - fixed - (int(d["blocks_" + t]) + 2) * 12) / ((r1 - r0 + 1) * 8) for t in ("before", "after")]
            assert arrays == [1, 2], "%s: pointer arrays before and after the attachment %r: the shard was not split" % (what, arrays)
            for tag, key in (("before", "b"), ("after", "a")):
                bad = hf.csr_mismatch((d[key + "ia"], d[key + "ja"], d[key + "val"]), want)
                assert bad is None, "%s, download %s the attachment: %s" % (what, tag, bad)
            ref = hf.spmv_reference(want, x, x[r0:r1], y0[r0:r1])
            i, ratio, over, err = cf.worst(d["y"], ref)
            assert ratio <= 1.0, "%s: row %d: |y - ref| = %.3e, bound %.3e, error / bound %.3g; %d rows over" % (
                what, i, err, float(ref["bound"][i]), ratio, over)
            top = max(top, ratio)
    print("e. split shards (%s): largest error / bound %.3g" % ("native communicator" if native else "gloo hooks", top))


# ------------------------------------------------------------------------------------ f. reference order with long rows --
@pytest.mark.parametrize("name", list(hf.REORDER))
def test_reference_order_with_long_rows(name):
    dim, ia, ja, val, sym, f = hf.make(name)
    lens = f["lengths"]
    assert {1, 63, 64, 65} <= set(lens.tolist()) and lens.max() >= 90
    perm, sign = hf.ref_order(f["kind"], f["n_sites"], f["n_up"], f["n_dn"])
    want = hf.reordered(dim, ia, ja, val, perm, sign)
    assert sorted(np.diff(want[0]).tolist()) == sorted(lens.tolist())
    A = _create(name)
    try:
        _assert_download(name + " as created", A, (ia, ja, val))
        R = A.reference_order(f["kind"], f["n_sites"], f["n_up"], f["n_dn"], opts=q.make_opts(**BASE))
        try:
            _assert_download(name + " in reference order", R, want)
        finally:
            R.destroy()
    finally:
        A.destroy()
