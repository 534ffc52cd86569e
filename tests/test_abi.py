"""CPU suite: the C-ABI library loads and exports every symbol
include/handel_gpu.h declares (no compute calls without a GPU), and the
Python binding declares exactly that set. One test at the end is marked gpu:
the refusals of the GT read-back calls that need a context."""

import ctypes
import os
import re

import pytest

from handel_amd import _lib
from handel_amd import build as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_symbols(header="handel_gpu.h"):
    text = open(os.path.join(ROOT, "include", header)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return set(re.findall(r"^\s*(?:const\s+)?[A-Za-z_]\w*\s*\**\s*(hg_\w+)\s*\(", text, flags=re.M))


def test_header_declares_expected_entry_points():
    syms = declared_symbols()
    for s in ("hg_create", "hg_verify_batch", "hg_verify_aggregate", "hg_pair", "hg_registry_load",
              "hg_set_message", "hg_combine_g1", "hg_aggregate_pk", "hg_keygen", "hg_sign"):
        assert s in syms


def test_library_exports_every_declared_symbol():
    path = B.build_library()
    lib = ctypes.CDLL(path)
    for s in declared_symbols():
        assert hasattr(lib, s), s
    assert set(_lib.SIGNATURES) == declared_symbols()


def test_version_and_code_strings_without_gpu():
    L = _lib.load(build_if_missing=False)
    assert L.hg_version() >= 1
    assert L.hg_code_string(1, 0) == b"bn256: signature invalid"
    assert L.hg_code_string(3, 0) == b"handel: inconsistent bitset with given level"
    assert L.hg_code_string(2, 0) == b"EOF"
    assert L.hg_code_string(7, 1) == b"bn256: coordinate exceeds modulus"


def test_exact_error_strings_without_gpu():
    """Every code's text (hg_code_string) and the verifySignature wrapping
    (hg_processing_error_string), against the reference's error values."""
    L = _lib.load(build_if_missing=False)
    go, cf = _lib.HG_FLAVOR_GO, _lib.HG_FLAVOR_CF
    code = lambda c, f=go: L.hg_code_string(c, f).decode()  # noqa: E731
    proc = lambda c, f=go: L.hg_processing_error_string(c, f).decode()  # noqa: E731
    assert code(_lib.HG_OK) == "" and proc(_lib.HG_OK) == ""
    # bn256/go/bn256.go:91,117,186; processing.go:351; crypto.go:123
    assert code(_lib.HG_ERR_PK_UNMARSHAL) == "unable to unmarshal"
    assert code(_lib.HG_ERR_SIG_UNMARSHAL) == "bn256: multisig can't unmarshal"
    assert code(_lib.HG_ERR_MULTI_SIZES) == "verify multisignature: inconsistent sizes"
    # cloudflare wraps the G1 error in SigBLS.UnmarshalBinary (bn256/cf/bn256.go:183-190)
    assert code(_lib.HG_ERR_SIG_CF_EXCEEDS, cf) == "bn256: multisig can't unmarshal: bn256: coordinate exceeds modulus"
    assert code(_lib.HG_ERR_SIG_CF_MALFORMED, cf) == "bn256: multisig can't unmarshal: bn256: malformed point"
    assert code(_lib.HG_ERR_SIG_CF_SHORT, cf) == "bn256: multisig can't unmarshal: bn256: not enough data"
    assert code(_lib.HG_ERR_CF_MALFORMED, cf) == "bn256: malformed point"
    # processing.go:361-365 wraps VerifySignature's errors; the level error is returned as is (:350-352)
    assert proc(_lib.HG_ERR_SIG_INVALID) == "handel: bn256: signature invalid"
    assert proc(_lib.HG_ERR_HASH_EOF) == "handel: EOF"
    assert proc(_lib.HG_ERR_LEVEL) == "handel: inconsistent bitset with given level"
    assert "handel: handel:" not in "".join(proc(c) for c in range(14))


def test_null_handles_are_refused_without_gpu():
    """Entry points that take a context or lane refuse NULL before touching
    the device (no GPU here: nothing else may run)."""
    L = _lib.load(build_if_missing=False)
    assert L.hg_context_simds(None) == 0
    assert L.hg_lane_set_latency_form(None, 2048) == _lib.HG_ERR_ARG
    assert L.hg_lane_set_pairing_padding(None, 1) == _lib.HG_ERR_ARG
    assert L.hg_sig_pairing_device(None, None, 0, None, 0, None) == _lib.HG_ERR_ARG
    assert L.hg_set_verify_split(None, 1) == _lib.HG_ERR_ARG
    assert L.hg_set_fold_overlap(None, 1) == _lib.HG_ERR_ARG


def test_gt_read_back_refuses_null_without_gpu():
    """hg_debug_gt_layout, hg_debug_gt_entries and hg_debug_gt_fold refuse a
    NULL context or NULL buffers before touching anything."""
    import numpy as np

    L = _lib.load(build_if_missing=False)
    out = np.full(_lib.HG_GT_LAYOUT_WORDS + 240, 0xA5A5A5A5, dtype=np.uint32)
    codes = np.full(2, -7, dtype=np.int32)
    reqs = np.zeros(8, dtype=np.uint32)
    words = np.zeros(2, dtype=np.uint64)
    p = lambda a: a.ctypes.data  # noqa: E731
    assert L.hg_debug_gt_layout(None, p(out)) == _lib.HG_ERR_ARG
    assert L.hg_debug_gt_entries(None, 0, 0, 1, p(out)) == _lib.HG_ERR_ARG
    assert L.hg_debug_gt_fold(None, p(reqs), 2, p(words), 2, 8, p(out), p(codes)) == _lib.HG_ERR_ARG
    assert (out == 0xA5A5A5A5).all() and (codes == -7).all()


@pytest.mark.gpu
def test_gt_read_back_refusals_leave_out_untouched():
    """With a context: NULL buffers, no tables (a fresh context; a registry and
    a message but nothing built), an unknown table, a range past a table's end,
    a 16-key read below level 2, a chunk outside 1..64, n = 0, a request whose
    words leave the bitset: HG_ERR_ARG every time, nothing written."""
    import numpy as np

    from handel_amd.engine import REQ_DTYPE, Engine
    from oracle import ref_lib as R
    from tests import _fixtures as F

    e = Engine(device=0, flavor="go")
    try:
        L, ctx, ARG = e.L, e.ctx, _lib.HG_ERR_ARG
        out = np.full((2, 120), 0xA5A5A5A5, dtype=np.uint32)
        codes = np.full(2, -7, dtype=np.int32)
        reqs = np.array([(0, 9, 9, 0), (1, 5, 5, 1)], dtype=REQ_DTYPE)
        words = np.array([3, 1], dtype=np.uint64)
        p = lambda a: a.ctypes.data  # noqa: E731

        def refused():
            assert L.hg_debug_gt_layout(ctx, p(out)) == ARG
            for table in range(4):
                assert L.hg_debug_gt_entries(ctx, table, 0, 1, p(out)) == ARG, table
            assert L.hg_debug_gt_fold(ctx, p(reqs), 2, p(words), 2, 8, p(out), p(codes)) == ARG
            assert (out == 0xA5A5A5A5).all() and (codes == -7).all()

        refused()  # a fresh context
        assert not e.registry_load(R.g2_scalar_base(F.scalar_bytes(F.scalars(9, seed=b"abi-gt")))).any()
        assert e.set_message(F.LIB_MESSAGE) == 0
        refused()  # a registry and a message, no tables
        e.set_aggregate_level(1)
        assert e.prepare_aggregate() == 0 and e.aggregate_tables() == 1
        assert L.hg_debug_gt_layout(ctx, None) == ARG
        assert L.hg_debug_gt_entries(ctx, 0, 0, 1, None) == ARG
        bad = [(4, 0, 1), (-1, 0, 1), (0, 9, 1), (0, 8, 2), (0, 0, 10), (1, 2 * 256, 1), (1, 511, 2), (2, 0, 1),
               (3, 0, 2), (0, 1 << 63, 1 << 63)]  # 9 keys: two 8-key windows, one block (level 4), no 16-key table
        for table, first, count in bad:
            assert L.hg_debug_gt_entries(ctx, table, first, count, p(out)) == ARG, (table, first, count)
        for chunk in (0, -1, 65):
            assert L.hg_debug_gt_fold(ctx, p(reqs), 2, p(words), 2, chunk, p(out), p(codes)) == ARG, chunk
        assert L.hg_debug_gt_fold(ctx, p(reqs), 0, p(words), 2, 8, p(out), p(codes)) == ARG
        assert L.hg_debug_gt_fold(ctx, None, 2, p(words), 2, 8, p(out), p(codes)) == ARG
        assert L.hg_debug_gt_fold(ctx, p(reqs), 2, p(words), 2, 8, None, p(codes)) == ARG
        assert L.hg_debug_gt_fold(ctx, p(reqs), 2, p(words), 2, 8, p(out), None) == ARG
        assert L.hg_debug_gt_fold(ctx, p(reqs), 2, p(words), 1, 8, p(out), p(codes)) == ARG  # request 1's word
        assert (out == 0xA5A5A5A5).all() and (codes == -7).all()
        # and what is allowed: the last entry of each built table, an empty range at the end
        assert L.hg_debug_gt_entries(ctx, 0, 9, 0, p(out)) == 0 and (out == 0xA5A5A5A5).all()
        lay = e.gt_layout()
        assert (lay["level"], lay["torus"], lay["nreg"], lay["nwin8"], lay["nwin16"]) == (1, False, 9, 2, 1)
        assert lay["blocks"] == {4: (0, 1)}
        assert e.gt_entries(e.GT_KEYS, 8, 1).shape == (1, 120) and e.gt_entries(e.GT_WIN8, 511, 1).any()
        assert e.gt_entries(e.GT_BLOCKS, 0, 1).any()
    finally:
        e.close()
