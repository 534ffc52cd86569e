"""CPU suite of aggregate verification with one message per request
(include/handel_gpu.h: hg_verify_aggregate_msgs, hg_verify_aggregate_msgs_device,
hg_verify_multisig_msgs): the ABI surface, the new kernels'
register, LDS and scratch figures from the compiled code object, and the Go
source and INTEGRATION.md naming the entry points with the header's argument
order. No GPU needed."""

import ctypes
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
LIB = os.path.join(ROOT, "handel_amd", "_build", "libhandel_gpu.so")
HEADER = open(os.path.join(ROOT, "include", "handel_gpu.h")).read()

NEW_SYMBOLS = ("hg_verify_aggregate_msgs", "hg_verify_aggregate_msgs_device", "hg_verify_multisig_msgs")
HG_ERR_ARG = 100


def _lib():
    from handel_amd import _lib as B

    return B.load()


def _params(name):
    """The parameter names of `name`'s declaration in the header, in order."""
    m = re.search(r"\bint\s+%s\s*\(([^;]*?)\)\s*;" % name, HEADER, flags=re.S)
    assert m, name
    return [re.sub(r"\[.*\]", "", p.split()[-1].lstrip("*")) for p in m.group(1).replace("\n", " ").split(",")]


def test_header_declares_and_library_exports_the_entry_points():
    from handel_amd import _lib as B

    L = _lib()
    for name in NEW_SYMBOLS:
        assert hasattr(L, name), name
        assert len(B.SIGNATURES[name][1]) == len(_params(name)), name
        # each entry cites the reference lines it mirrors
        decl = HEADER.index("int %s(" % name)
        comment = HEADER[HEADER.rindex("/*", 0, decl):decl]
        assert "crypto.go:120-137" in comment, name
    assert _params("hg_verify_aggregate_msgs") == ["ctx", "pool", "pool_len", "msg_off", "msg_len", "reqs", "n", "words",
                                                   "nwords", "sigs", "codes", "agg_pk_out"]
    assert _params("hg_verify_aggregate_msgs_device") == ["ctx", "d_pool", "pool_len", "d_msg_off", "d_msg_len", "d_reqs",
                                                          "n", "d_words", "d_sigs", "d_codes", "d_agg_pk_out", "stream"]
    assert _params("hg_verify_multisig_msgs") == ["ctx", "pool", "pool_len", "msg_off", "msg_len", "bitlens",
                                                  "word_offsets", "n", "words", "nwords", "sigs", "codes"]
    # the header says which pairing form runs, and why the tables cannot serve
    comment = HEADER[HEADER.rindex("/*", 0, HEADER.index("int hg_verify_aggregate_msgs(")):]
    assert "one-kernel form" in comment[:3000] and "hg_set_verify_split" in comment[:3000]


def test_null_handles_are_refused_without_gpu():
    L = _lib()
    one = ctypes.create_string_buffer(128)
    assert L.hg_verify_aggregate_msgs(None, None, 0, None, None, None, 0, None, 0, None, None, None) == HG_ERR_ARG
    assert L.hg_verify_aggregate_msgs(None, one, 1, one, one, one, 1, one, 1, one, one, None) == HG_ERR_ARG
    assert L.hg_verify_aggregate_msgs_device(None, None, 0, None, None, None, 0, None, None, None, None,
                                             None) == HG_ERR_ARG
    assert L.hg_verify_multisig_msgs(None, None, 0, None, None, None, None, 0, None, 0, None, None) == HG_ERR_ARG
    assert L.hg_verify_multisig_msgs(None, one, 1, one, one, one, one, 1, one, 1, one, one) == HG_ERR_ARG


def test_engine_and_plugin_mirror_bind_the_calls():
    from handel_amd.engine import Engine
    from handel_amd.processing import BatchVerifier

    for name in ("verify_aggregate_msgs", "verify_aggregate_msgs_pool", "verify_aggregate_msgs_device",
                 "verify_multisig_msgs"):
        assert callable(getattr(Engine, name)), name
    assert callable(BatchVerifier.verify_multisignatures_msgs)


# ---------------------------------------------------------------- kernel resources
# mangled-name fragment: (LDS bytes, VGPR ceiling). One thread per request and
# no shared memory; the merge kernel's registers are decode_g1_one's on-curve
# check (k_decode_g1's), well inside the 128 that keep four waves on a SIMD.
NEW_KERNELS = {
    "k_aggmsgs_levels": (0, 16),
    "k_aggmsgs_merge": (0, 128),
}


@pytest.fixture(scope="module")
def res():
    if not os.path.exists(LIB):
        pytest.skip("libhandel_gpu.so not built")
    import kernel_sizes

    r = kernel_sizes.resources(LIB)
    if not r:
        pytest.skip("no gfx950 code object metadata found")
    return r


def _one(res, part):
    hits = {k: v for k, v in res.items() if part in k}
    assert len(hits) == 1, (part, sorted(hits))
    return next(iter(hits.values()))


@pytest.mark.parametrize("part", sorted(NEW_KERNELS))
def test_new_kernels_keep_their_budgets(res, part):
    r = _one(res, part)
    lds, vgpr = NEW_KERNELS[part]
    assert r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0 and r["scratch"] == 0, (part, r)
    assert r["lds"] == lds, (part, r)
    assert r["vgpr"] <= vgpr, (part, r)


def test_new_names_leave_the_existing_lookups_unique(res):
    """The resource tests find kernels by name fragment and want exactly one
    hit: the new kernels' names hold none of the fragments in use."""
    for part in ("k_verify_mlILi4E", "k_verifyILi4E", "k_msgs_verify", "k_msgs_miller", "k_merge_hash_codes",
                 "k_hash_scalars", "k_hash_points", "k_agg_finish", "k_agg_plan"):
        assert len([k for k in res if part in k]) == 1, part


# ---------------------------------------------------------------- the Go source and the documents
def _go(name):
    return open(os.path.join(ROOT, "go", "bn256", "hip", name)).read()


def test_go_source_calls_the_abi_in_the_header_order():
    """No Go toolchain here (tests/test_go_shim.py): what can be held is that
    the cgo call passes one argument per header parameter, in the header's
    order, by the names the Go code gives them."""
    src = _go("engine.go")
    assert re.search(r"func \(e \*Engine\) VerifyMultiSignaturesMsgs\(msgs \[\]\[\]byte, bitLens \[\]int, "
                     r"words \[\]\[\]uint64, sigs \[\]byte\) \(\[\]int32, error\)", src)
    call = src[src.index("C.hg_verify_multisig_msgs("):]
    call = call[:call.index("\n\tif rc")]
    order = ["e.ctx", "bytePtr(pool)", "len(pool)", "&off[0]", "&ln[0]", "&lens[0]", "&woff[0]", "C.size_t(n)",
             "wordPtr(all)", "len(all)", "bytePtr(sigs)", "codePtr(codes)"]
    assert len(order) == len(_params("hg_verify_multisig_msgs"))
    at = [call.index(a) for a in order]
    assert at == sorted(at), at
    reg = _go("registry.go")
    assert re.search(r"func \(r \*Registry\) VerifyMultiSignaturesMsgs\(msgs \[\]\[\]byte, "
                     r"ms \[\]\*handel\.MultiSignature\) \[\]error", reg)
    body = reg[reg.index("func (r *Registry) VerifyMultiSignaturesMsgs("):]
    # the registry-generation check and the error texts of VerifyMultiSignatures
    assert "r.current()" in body and "hip: registry is no longer loaded on its engine" in body
    assert "r.e.VerifyMultiSignaturesMsgs(" in body and "r.e.CodeError(codes[j])" in body


def test_documents_name_the_entry_points():
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in NEW_SYMBOLS + ("VerifyMultiSignaturesMsgs", "verify_aggregate_msgs", "verify_multisig_msgs"):
        assert name in integration, name
    for name in NEW_SYMBOLS:  # the table row gives the header's arguments, in its order
        row = next(line for line in integration.splitlines() if line.startswith("| `%s(" % name))
        args = row[row.index("(") + 1:row.index(")")]
        assert [a.strip() for a in args.split(",")] == _params(name), name
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "3k" in design and "hg_verify_aggregate_msgs" in design
    assert "hg_verify_aggregate_msgs" in open(os.path.join(ROOT, "README.md")).read()
