"""integration/qbhip_reference.patch: what can be checked from the patch and include/qbhip.h alone.  Applying it needs the
reference's own sources, which are not part of this repository (integration/README.md says how to apply and build it)."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATCH = os.path.join(ROOT, "integration", "qbhip_reference.patch")
HEADER = os.path.join(ROOT, "include", "qbhip.h")


def _hunks():
    """{basename: {"+": added lines, "-": removed lines}} of the patch."""
    out, cur = {}, None
    for ln in open(PATCH).read().splitlines():
        if ln.startswith("+++ "):
            cur = out.setdefault(os.path.basename(ln.split()[1]), {"+": [], "-": []})
        elif ln.startswith("--- ") or ln.startswith("diff "):
            continue
        elif cur is not None and ln[:1] in ("+", "-"):
            cur[ln[0]].append(ln[1:])
    return out


def test_patch_only_touches_the_two_translation_units():
    files = [ln.split()[1] for ln in open(PATCH) if ln.startswith("+++ ")]
    assert sorted(os.path.basename(f) for f in files) == ["lanczos.cc", "sparse.cc"]
    assert all("qbasis.h" not in ln for ln in open(PATCH) if ln.startswith(("+++", "---")))


def test_patch_binds_the_c_abi_of_the_header():
    h = _hunks()
    sp, lz = "\n".join(h["sparse.cc"]["+"]), "\n".join(h["lanczos.cc"]["+"])
    # both translation units include the library's header, and every qbh_ entry point they call is declared there
    for added in (sp, lz):
        assert '#include "qbhip.h"' in added
    declared = set(re.findall(r"\b(qbh_[a-z0-9_]+)\s*\(", open(HEADER).read()))
    called = set(re.findall(r"\b(qbh_[a-z0-9_]+)\s*\(", sp + "\n" + lz))
    assert called and called <= declared, sorted(called - declared)
    # sparse.cc: the complex operator is created, applied and destroyed through the C ABI ...
    for needle in ("qbh_csr_create(", "qbh_csr_destroy(", "qbh_multmv2(", "qbh_multmv("):
        assert needle in sp, needle
    assert sp.count("create_handle(&handle, dim, nnz, sym, ia, ja, val)") == 2
    # ... and the complex MKL sparse calls are taken out, none put back
    removed = "\n".join(h["sparse.cc"]["-"])
    for mkl in ("mkl_sparse_z_mv", "mkl_sparse_z_create_csr"):
        assert mkl in removed and mkl not in sp and mkl not in lz
    # lanczos.cc: the csr_mat<complex> solvers are the fused device solvers; the device IRAM only under QBHIP_DEVICE_IRAM
    for needle in ("qbh_lanczos(", "qbh_lanczos_ckpt(", "qbh_eigenvec_cg("):
        assert needle in lz, needle
    guarded = re.search(r"#ifdef QBHIP_DEVICE_IRAM(.*?)#else", lz, re.S)
    assert guarded and "qbh_iram(" in guarded.group(1)
    assert "qbh_iram(" not in lz.replace(guarded.group(1), "")
    assert lz.count("#endif") >= 1
