"""CPU suite of the multi-message batch (include/handel_gpu.h:
hg_verify_batch_msgs and its companions): hashedMessage's scalar by the code
the device runs (hg_debug_hash_scalar: SHA-256 and the crypto/rand.Int rule,
bn256/go/bn256.go:210-216) against hashlib and the Order rule, the ABI surface,
and the new kernels' register and LDS budgets. No GPU needed."""

import ctypes
import os
import re
import sys

import numpy as np
import pytest

from tests import _msgs_fixtures as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
LIB = os.path.join(ROOT, "handel_amd", "_build", "libhandel_gpu.so")

NEW_SYMBOLS = ("hg_verify_batch_msgs", "hg_verify_batch_msgs_device", "hg_hash_messages", "hg_debug_g1_base_mul",
               "hg_debug_hash_scalar")
HG_OK, HG_ERR_HASH_EOF, HG_ERR_ARG = 0, 2, 100


def _lib():
    from handel_amd import _lib as B

    return B.load()


def _hash_scalar(L, msg: bytes):
    k = (ctypes.c_uint32 * 8)()
    buf = ctypes.create_string_buffer(msg, len(msg)) if msg else None
    rc = L.hg_debug_hash_scalar(buf, len(msg), k)
    return rc, sum(int(w) << (32 * i) for i, w in enumerate(k))


def test_boundary_set_has_both_kinds_at_every_length():
    msgs = M.boundary_set()
    M.check_boundary_set(msgs)
    assert len(msgs) == 2 * len(M.LENGTHS) + 1


def test_hash_scalar_matches_hashlib_and_the_order_rule():
    L = _lib()
    rng = np.random.default_rng(2024)
    msgs = [m for m, _ in M.boundary_set()]
    msgs += [rng.bytes(int(rng.integers(0, 150))) for _ in range(300)]
    kinds = set()
    for m in msgs:
        rc, k = _hash_scalar(L, m)
        d = M.digest_int(m)
        assert k == d, (len(m), m[:8])  # the words are the digest as an integer, whatever the code
        assert rc == (HG_OK if 0 < d < M.ORDER else HG_ERR_HASH_EOF), (len(m), m[:8])
        kinds.add(rc)
    assert kinds == {HG_OK, HG_ERR_HASH_EOF}


def test_hash_scalar_refuses_null_arguments():
    L = _lib()
    k = (ctypes.c_uint32 * 8)()
    assert L.hg_debug_hash_scalar(None, 3, k) == HG_ERR_ARG
    assert L.hg_debug_hash_scalar(ctypes.create_string_buffer(b"abc", 3), 3, None) == HG_ERR_ARG
    assert L.hg_debug_hash_scalar(None, 0, k) == HG_ERR_HASH_EOF  # the empty message


def test_header_declares_and_library_exports_the_entry_points():
    header = open(os.path.join(ROOT, "include", "handel_gpu.h")).read()
    L = _lib()
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert hasattr(L, name), name
    # each entry cites the reference lines it mirrors
    for name in NEW_SYMBOLS:
        decl = header.index("int %s(" % name)
        comment = header[header.rindex("/*", 0, decl):decl]
        assert "bn256/go/bn256.go:" in comment, name


def test_null_handles_are_refused_without_gpu():
    L = _lib()
    one = ctypes.create_string_buffer(128)
    assert L.hg_verify_batch_msgs(None, None, 0, None, None, None, None, 0, None) == HG_ERR_ARG
    assert L.hg_verify_batch_msgs(None, one, 1, one, one, one, one, 1, one) == HG_ERR_ARG
    assert L.hg_verify_batch_msgs_device(None, None, 0, None, None, None, None, 0, None, None) == HG_ERR_ARG
    assert L.hg_hash_messages(None, None, 0, None, None, 0, None, None) == HG_ERR_ARG
    assert L.hg_debug_g1_base_mul(None, None, 0, None) == HG_ERR_ARG


# ---------------------------------------------------------------- kernel resources
# mangled-name fragment: (LDS bytes or the kernel whose LDS it shares, VGPR ceiling)
NEW_KERNELS = {
    "k_hash_scalars": (0, None),
    "k_g1_base_table": (0, None),
    "k_hash_points": (0, None),
    "k_merge_hash_codes": (0, None),
    "k_msgs_verify": ("k_verifyILi4E", None),   # the one-kernel form: k_verify<4>'s LDS
    "k_msgs_miller": (20480, 256),              # the split form's Miller loop: k_verify_ml<4>'s budget
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
    if isinstance(lds, str):
        lds = _one(res, lds)["lds"]
        assert lds == 33600
    assert r["lds"] == lds, (part, r)
    if vgpr is not None:
        assert r["vgpr"] <= vgpr, (part, r)


def test_new_names_leave_the_existing_lookups_unique(res):
    """tests/test_kernel_resources.py finds the pairing kernels by name
    fragment and wants exactly one hit: the new kernels' names hold none."""
    for part in ("k_verify_mlILi4E", "k_verifyILi4E", "k_verify_sig12ILb0E", "k_sig12_ninv", "k_sig12_norm"):
        assert len([k for k in res if part in k]) == 1, part
