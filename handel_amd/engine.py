"""Host wrapper around one hg_ctx (include/handel_gpu.h).

`Engine` is the batched replacement for the reference's one-at-a-time crypto
calls: it owns a GPU context, the decoded registry and the
hashed message, and exposes every C-ABI entry point with numpy/bytes
arguments. Device-resident variants take raw device pointers (e.g. from
torch tensors) and a HIP stream handle.
"""

from __future__ import annotations

import ctypes
import os
import weakref
from typing import Optional, Sequence, Tuple

import numpy as np

from . import _lib
from ._lib import HandelGPUError

FLAVORS = {"go": _lib.HG_FLAVOR_GO, "bn256/go": _lib.HG_FLAVOR_GO,
           "cf": _lib.HG_FLAVOR_CF, "bn256/cf": _lib.HG_FLAVOR_CF, "bn256": _lib.HG_FLAVOR_CF}

REQ_DTYPE = np.dtype([("offset", "<u4"), ("bitlen", "<u4"), ("level_size", "<u4"), ("word_offset", "<u4")])
# hg_packet (include/handel_gpu.h): one received Handel packet, marshals as pool ranges
PACKET_DTYPE = np.dtype([("origin", "<i4"), ("receiver", "<u4"), ("level", "<u4"), ("flags", "<u4"),
                         ("ms_off", "<u4"), ("ms_len", "<u4"), ("ind_off", "<u4"), ("ind_len", "<u4")])
# hg_store_update (include/handel_gpu.h): one (receiver, level) state pushed to the device stores
STORE_UPDATE_DTYPE = np.dtype([("receiver", "<u4"), ("level", "<u4"), ("flags", "<u4"), ("best_off", "<u4"),
                               ("indiv_off", "<u4")])
# hg_store_sig / hg_store_query (include/handel_gpu.h): a signature loaded into, a Combined query of, merge-enabled stores
STORE_SIG_DTYPE = np.dtype([("receiver", "<u4"), ("level", "<u4"), ("index", "<u4"), ("sig_off", "<u4")])
STORE_QUERY_DTYPE = np.dtype([("receiver", "<u4"), ("level", "<u4")])


def _ptr(a) -> Optional[int]:
    if a is None:
        return None
    if isinstance(a, (bytes, bytearray)):
        return ctypes.cast(ctypes.c_char_p(bytes(a)), ctypes.c_void_p).value
    return a.ctypes.data


def _u8(b) -> np.ndarray:
    if isinstance(b, np.ndarray):
        return np.ascontiguousarray(b, dtype=np.uint8)
    return np.frombuffer(bytes(b), dtype=np.uint8).copy()


class Engine:
    """One verification context on one GPU (hg_create)."""

    def __init__(self, device: int = 0, flavor: str = "go"):
        self.L = _lib.load()
        self.flavor_name = flavor
        self.flavor = FLAVORS[flavor]
        h = ctypes.c_void_p()
        rc = self.L.hg_create(device, self.flavor, ctypes.byref(h))
        if rc != 0:
            raise HandelGPUError(f"hg_create failed: code {rc}")
        self.ctx = h
        self.device = device

    def close(self):
        if getattr(self, "ctx", None):
            for ref in getattr(self, "_stores", []):  # device stores go before their context
                st = ref()
                if st is not None:
                    st.close()
            self.L.hg_destroy(self.ctx)
            self.ctx = None

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc: int, what: str, ok=(0,)):
        if rc not in ok:
            err = self.L.hg_last_error(self.ctx)
            raise HandelGPUError(f"{what}: code {rc}: {err.decode() if err else ''}")
        return rc

    def code_string(self, code: int) -> str:
        return self.L.hg_code_string(int(code), self.flavor).decode()

    def processing_error_string(self, code: int) -> str:
        """The text processing.go's verifySignature returns for `code`
        (hg_processing_error_string): VerifySignature errors wrapped "handel: ..."."""
        return self.L.hg_processing_error_string(int(code), self.flavor).decode()

    # ----------------------------------------------------------- setup
    def set_message(self, msg: bytes) -> int:
        """hashedMessage once per message; returns HG_OK or HG_ERR_HASH_EOF."""
        m = _u8(msg)
        return self._check(self.L.hg_set_message(self.ctx, _ptr(m) if len(m) else None, len(m)),
                           "hg_set_message", ok=(0, _lib.HG_ERR_HASH_EOF))

    def prepare_aggregate(self) -> int:
        """Builds the GT tables of aggregate verification for the current
        message and registry now (hg_prepare_aggregate); HG_OK or HG_ERR_HASH_EOF."""
        return self._check(self.L.hg_prepare_aggregate(self.ctx), "hg_prepare_aggregate",
                           ok=(0, _lib.HG_ERR_HASH_EOF))

    def prepare_aggregate_msg(self, msg: bytes) -> int:
        """set_message + prepare_aggregate under one lock hold
        (hg_prepare_aggregate_msg); HG_OK or HG_ERR_HASH_EOF."""
        m = _u8(msg)
        return self._check(self.L.hg_prepare_aggregate_msg(self.ctx, _ptr(m) if len(m) else None, len(m)),
                           "hg_prepare_aggregate_msg", ok=(0, _lib.HG_ERR_HASH_EOF))

    def set_aggregate_level(self, level: int) -> None:
        """Pins the GT table level of aggregate submissions (0..2) or returns
        them to the volume policy (-1) (hg_set_aggregate_level)."""
        self._check(self.L.hg_set_aggregate_level(self.ctx, int(level)), "hg_set_aggregate_level")

    def set_fold_overlap(self, on: bool) -> None:
        """GT fold beside (True) or before (False) the pairing kernel
        (hg_set_fold_overlap); same verdicts."""
        self._check(self.L.hg_set_fold_overlap(self.ctx, int(bool(on))), "hg_set_fold_overlap")

    def set_verify_split(self, on: bool) -> None:
        """Config 2's form (hg_set_verify_split): True = the split form for
        batches in flight on several contexts; same verdicts."""
        self._check(self.L.hg_set_verify_split(self.ctx, int(bool(on))), "hg_set_verify_split")

    def set_table_budget(self, nbytes: int) -> None:
        """Upper bound for this context's GT tables (hg_set_table_budget)."""
        self._check(self.L.hg_set_table_budget(self.ctx, int(nbytes)), "hg_set_table_budget")

    def registry_non_g2(self) -> int:
        """Registry keys on the twist but outside G2 (hg_registry_non_g2)."""
        return int(self.L.hg_registry_non_g2(self.ctx))

    def context_bytes(self) -> int:
        """Device memory the context holds (hg_context_bytes)."""
        return int(self.L.hg_context_bytes(self.ctx))

    def aggregate_tables(self) -> int:
        """Table level aggregate requests run at (hg_aggregate_tables): 0 = G2
        fold, 1 = GT fold over 8-key windows, 2 = over 16-key windows."""
        return int(self.L.hg_aggregate_tables(self.ctx))

    def aggregate_tables_torus(self) -> bool:
        """Whether the level-2 tables are kept in torus form
        (hg_aggregate_tables_torus); False for a registry with a window subset
        or block of keys that sums to zero, which has no such form."""
        return bool(self.L.hg_aggregate_tables_torus(self.ctx))

    def registry_load(self, pks: bytes) -> np.ndarray:
        a = _u8(pks)
        n = len(a) // 128
        codes = np.zeros(n, dtype=np.int32)
        rc = self.L.hg_registry_load(self.ctx, _ptr(a), n, _ptr(codes))
        self._check(rc, "hg_registry_load", ok=(0, _lib.HG_ERR_PK_UNMARSHAL))
        return codes

    # ----------------------------------------------------------- batch verification
    def verify_batch(self, pks: bytes, sigs: bytes) -> np.ndarray:
        a, b = _u8(pks), _u8(sigs)
        n = len(b) // 64
        if len(a) != 128 * n:
            raise ValueError("pks must hold 128 bytes per signature")
        codes = np.zeros(n, dtype=np.int32)
        self._check(self.L.hg_verify_batch(self.ctx, _ptr(a), _ptr(b), n, _ptr(codes)), "hg_verify_batch")
        return codes

    def verify_batch_msg(self, msg: bytes, pks: bytes, sigs: bytes) -> np.ndarray:
        """PublicKey.VerifySignature(msg, sig) x n, hashing and verifying under
        one lock hold of the context (hg_verify_batch_msg)."""
        m, a, b = _u8(msg), _u8(pks), _u8(sigs)
        n = len(b) // 64
        if len(a) != 128 * n:
            raise ValueError("pks must hold 128 bytes per signature")
        codes = np.zeros(n, dtype=np.int32)
        rc = self.L.hg_verify_batch_msg(self.ctx, _ptr(m) if len(m) else None, len(m), _ptr(a) if n else None,
                                        _ptr(b) if n else None, n, _ptr(codes) if n else None)
        self._check(rc, "hg_verify_batch_msg")
        return codes

    def verify_batch_device(self, d_pks: int, d_sigs: int, n: int, d_codes: int, stream: int = 0):
        self._check(self.L.hg_verify_batch_device(self.ctx, d_pks, d_sigs, n, d_codes, stream or None),
                    "hg_verify_batch_device")

    # ----------------------------------------------------------- checks on their own messages
    @staticmethod
    def pack_messages(msgs: Sequence[bytes]) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """(pool, msg_off, msg_len) of hg_verify_batch_msgs: the messages end
        to end, equal messages stored once."""
        off = np.zeros(len(msgs), dtype=np.uint32)
        ln = np.zeros(len(msgs), dtype=np.uint32)
        seen, parts, at = {}, [], 0
        for i, m in enumerate(msgs):
            m = bytes(m)
            if m not in seen:
                seen[m] = at
                parts.append(m)
                at += len(m)
            off[i], ln[i] = seen[m], len(m)
        if at >= 1 << 32:
            raise ValueError("the messages of one batch must stay below 2^32 bytes")
        return np.frombuffer(b"".join(parts), dtype=np.uint8).copy(), off, ln

    def verify_batch_msgs_pool(self, pool, msg_off, msg_len, pks: bytes, sigs: bytes) -> np.ndarray:
        """hg_verify_batch_msgs on a caller-built pool: check i's message is
        pool[msg_off[i] : msg_off[i] + msg_len[i]]."""
        pool, a, b = _u8(pool), _u8(pks), _u8(sigs)
        off = np.ascontiguousarray(msg_off, dtype=np.uint32)
        ln = np.ascontiguousarray(msg_len, dtype=np.uint32)
        n = len(b) // 64
        if len(a) != 128 * n or len(off) != n or len(ln) != n:
            raise ValueError("one message range, 128 key bytes and 64 signature bytes per check")
        codes = np.zeros(n, dtype=np.int32)
        if n:
            self._check(self.L.hg_verify_batch_msgs(self.ctx, _ptr(pool) if len(pool) else None, len(pool), _ptr(off),
                                                    _ptr(ln), _ptr(a), _ptr(b), n, _ptr(codes)),
                        "hg_verify_batch_msgs")
        return codes

    def verify_batch_msgs(self, msgs: Sequence[bytes], pks: bytes, sigs: bytes) -> np.ndarray:
        """PublicKey.VerifySignature(msgs[i], sigs[i]) for n checks that each
        carry their own message, in one batch (hg_verify_batch_msgs); the
        context's current message and tables stay as they are."""
        pool, off, ln = self.pack_messages(msgs)
        return self.verify_batch_msgs_pool(pool, off, ln, pks, sigs)

    def verify_batch_msgs_device(self, d_pool: int, pool_len: int, d_msg_off: int, d_msg_len: int, d_pks: int,
                                 d_sigs: int, n: int, d_codes: int, stream: int = 0) -> None:
        """hg_verify_batch_msgs_device on raw device pointers (asynchronous); a
        range past pool_len gives that check HG_ERR_ARG."""
        self._check(self.L.hg_verify_batch_msgs_device(self.ctx, d_pool or None, pool_len, d_msg_off, d_msg_len, d_pks,
                                                       d_sigs, n, d_codes, stream or None),
                    "hg_verify_batch_msgs_device")

    def hash_messages(self, msgs: Sequence[bytes]) -> Tuple[bytes, np.ndarray]:
        """hashedMessage x n (hg_hash_messages): (n x 64 bytes of G1 marshals,
        codes); an HG_ERR_HASH_EOF entry holds the generator as a placeholder."""
        pool, off, ln = self.pack_messages(msgs)
        return self.hash_messages_pool(pool, off, ln)

    def hash_messages_pool(self, pool, msg_off, msg_len) -> Tuple[bytes, np.ndarray]:
        pool = _u8(pool)
        off = np.ascontiguousarray(msg_off, dtype=np.uint32)
        ln = np.ascontiguousarray(msg_len, dtype=np.uint32)
        n = len(off)
        out = np.zeros(n * 64, dtype=np.uint8)
        codes = np.zeros(n, dtype=np.int32)
        if n:
            self._check(self.L.hg_hash_messages(self.ctx, _ptr(pool) if len(pool) else None, len(pool), _ptr(off),
                                                _ptr(ln), n, _ptr(out), _ptr(codes)), "hg_hash_messages")
        return out.tobytes(), codes

    def debug_g1_base_mul(self, scalars: Sequence[int]) -> bytes:
        """k * G1 marshals by the fixed-base kernel alone (hg_debug_g1_base_mul)."""
        n = len(scalars)
        k = np.array([[(int(s) >> (32 * w)) & 0xFFFFFFFF for w in range(8)] for s in scalars],
                     dtype=np.uint32).reshape(n, 8)
        out = np.zeros(n * 64, dtype=np.uint8)
        if n:
            self._check(self.L.hg_debug_g1_base_mul(self.ctx, _ptr(k), n, _ptr(out)), "hg_debug_g1_base_mul")
        return out.tobytes()

    def pack_verdicts_device(self, d_codes: int, n: int, d_bits: int, stream: int = 0):
        """Device verdict bitset (hg_pack_verdicts_device): ceil(n/8) bytes,
        bit j of byte b = check 8b+j passed."""
        self._check(self.L.hg_pack_verdicts_device(self.ctx, d_codes, n, d_bits, stream or None),
                    "hg_pack_verdicts_device")

    # hg_sig_pairing_device kernels
    SIG_K16_PAD, SIG_K16, SIG_K12_PAD, SIG_K12, SIG_W2 = 0, 1, 2, 3, 4

    def sig_pairing_device(self, d_sigs: int, n: int, d_fe: int, kernel: int, stream: int = 0):
        """FE(Miller(G2Base at -sig)) of n signature marshals into d_fe (n x 480
        bytes) with one chosen pairing kernel (hg_sig_pairing_device): the
        per-kernel roofline and the cross-kernel check."""
        self._check(self.L.hg_sig_pairing_device(self.ctx, d_sigs, n, d_fe, int(kernel), stream or None),
                    "hg_sig_pairing_device")

    def verify_aggregate(self, reqs: np.ndarray, words: np.ndarray, sigs: bytes, want_agg: bool = False):
        reqs = np.ascontiguousarray(reqs, dtype=REQ_DTYPE)
        words = np.ascontiguousarray(words, dtype=np.uint64)
        s = _u8(sigs)
        n = len(reqs)
        codes = np.zeros(n, dtype=np.int32)
        agg = np.zeros(n * 128, dtype=np.uint8) if want_agg else None
        self._check(self.L.hg_verify_aggregate(self.ctx, _ptr(reqs), n, _ptr(words) if len(words) else None,
                                               len(words), _ptr(s), _ptr(codes), _ptr(agg)),
                    "hg_verify_aggregate")
        return (codes, agg.tobytes()) if want_agg else codes

    # ------------------------------------------------------------ random linear combination
    # The default group: profiles/rlc_bench.json (README "Random linear combination")
    RLC_GROUP = 64

    @staticmethod
    def _seed(seed: Optional[bytes]) -> np.ndarray:
        seed = os.urandom(32) if seed is None else bytes(seed)
        if len(seed) != 32:
            raise ValueError("seed: 32 bytes")
        return _u8(seed)

    def verify_aggregate_rlc(self, reqs: np.ndarray, words: np.ndarray, sigs: bytes, seed: Optional[bytes] = None,
                             group: int = RLC_GROUP) -> np.ndarray:
        """verify_aggregate with one pairing per `group` checks under random
        coefficients (hg_verify_aggregate_rlc): the same codes, an invalid
        signature accepted with probability <= 2^-64 over `seed`, which the
        signatures' sender must not predict (None: os.urandom(32))."""
        reqs = np.ascontiguousarray(reqs, dtype=REQ_DTYPE)
        words = np.ascontiguousarray(words, dtype=np.uint64)
        s = _u8(sigs)
        sd = self._seed(seed)
        n = len(reqs)
        codes = np.zeros(n, dtype=np.int32)
        self._check(self.L.hg_verify_aggregate_rlc(self.ctx, _ptr(reqs), n, _ptr(words) if len(words) else None,
                                                   len(words), _ptr(s), _ptr(sd), int(group), _ptr(codes)),
                    "hg_verify_aggregate_rlc")
        return codes

    def verify_aggregate_rlc_device(self, d_reqs: int, n: int, d_words: int, d_sigs: int, d_codes: int,
                                    seed: Optional[bytes] = None, group: int = RLC_GROUP, stream: int = 0):
        """Device-resident verify_aggregate_rlc; synchronises `stream` once (the
        failed groups' member count sizes their exact recheck)."""
        sd = self._seed(seed)
        self._check(self.L.hg_verify_aggregate_rlc_device(self.ctx, d_reqs, n, d_words, d_sigs, _ptr(sd), int(group),
                                                          d_codes, stream or None),
                    "hg_verify_aggregate_rlc_device")

    def rlc_stats(self) -> Tuple[int, int, int]:
        """The last verify_aggregate_rlc* call: (groups checked, groups that
        failed, checks re-verified one by one); zeros when the exact path ran."""
        v = [ctypes.c_uint64() for _ in range(3)]
        self._check(self.L.hg_rlc_stats(self.ctx, *[ctypes.byref(x) for x in v]), "hg_rlc_stats")
        return tuple(int(x.value) for x in v)

    # ------------------------------------------------------------ ... of independent checks on arbitrary keys
    def verify_batch_rlc(self, pks: bytes, sigs: bytes, seed: Optional[bytes] = None,
                         group: int = RLC_GROUP) -> np.ndarray:
        """verify_batch with one final exponentiation per `group` checks under
        random coefficients (hg_verify_batch_rlc): the same codes, an invalid
        signature accepted with probability <= 2^-64 over `seed`, which the
        signatures' sender must not predict (None: os.urandom(32)). Each
        check's Miller loop also decides whether its key lies in G2; a group
        holding a key that does not is verified check by check.
        batch_rlc_stats() reports on the call."""
        a, b = _u8(pks), _u8(sigs)
        n = len(b) // 64
        if len(a) != 128 * n:
            raise ValueError("pks must hold 128 bytes per signature")
        sd = self._seed(seed)
        codes = np.zeros(n, dtype=np.int32)
        self._check(self.L.hg_verify_batch_rlc(self.ctx, _ptr(a) if n else None, _ptr(b) if n else None, n, _ptr(sd),
                                               int(group), _ptr(codes) if n else None), "hg_verify_batch_rlc")
        return codes

    def verify_batch_rlc_device(self, d_pks: int, d_sigs: int, n: int, d_codes: int, seed: Optional[bytes] = None,
                                group: int = RLC_GROUP, stream: int = 0) -> None:
        """hg_verify_batch_rlc_device on raw device pointers; synchronises
        `stream` once (the failed groups' member count sizes their recheck)."""
        sd = self._seed(seed)
        self._check(self.L.hg_verify_batch_rlc_device(self.ctx, d_pks, d_sigs, n, _ptr(sd), int(group), d_codes,
                                                      stream or None), "hg_verify_batch_rlc_device")

    def verify_batch_msgs_rlc_pool(self, pool, msg_off, msg_len, pks: bytes, sigs: bytes,
                                   seed: Optional[bytes] = None, group: int = RLC_GROUP) -> np.ndarray:
        """hg_verify_batch_msgs_rlc on a caller-built pool."""
        pool, a, b = _u8(pool), _u8(pks), _u8(sigs)
        off = np.ascontiguousarray(msg_off, dtype=np.uint32)
        ln = np.ascontiguousarray(msg_len, dtype=np.uint32)
        n = len(b) // 64
        if len(a) != 128 * n or len(off) != n or len(ln) != n:
            raise ValueError("one message range, 128 key bytes and 64 signature bytes per check")
        sd = self._seed(seed)
        codes = np.zeros(n, dtype=np.int32)
        self._check(self.L.hg_verify_batch_msgs_rlc(self.ctx, _ptr(pool) if len(pool) else None, len(pool),
                                                    _ptr(off) if n else None, _ptr(ln) if n else None,
                                                    _ptr(a) if n else None, _ptr(b) if n else None, n, _ptr(sd),
                                                    int(group), _ptr(codes) if n else None),
                    "hg_verify_batch_msgs_rlc")
        return codes

    def verify_batch_msgs_rlc(self, msgs: Sequence[bytes], pks: bytes, sigs: bytes, seed: Optional[bytes] = None,
                              group: int = RLC_GROUP) -> np.ndarray:
        """verify_batch_msgs with one final exponentiation per `group` checks
        under random coefficients (hg_verify_batch_msgs_rlc): the same codes;
        seed and membership as verify_batch_rlc."""
        pool, off, ln = self.pack_messages(msgs)
        return self.verify_batch_msgs_rlc_pool(pool, off, ln, pks, sigs, seed, group)

    def verify_batch_msgs_rlc_device(self, d_pool: int, pool_len: int, d_msg_off: int, d_msg_len: int, d_pks: int,
                                     d_sigs: int, n: int, d_codes: int, seed: Optional[bytes] = None,
                                     group: int = RLC_GROUP, stream: int = 0) -> None:
        """hg_verify_batch_msgs_rlc_device on raw device pointers; synchronises
        `stream` once; a range past pool_len gives that check HG_ERR_ARG."""
        sd = self._seed(seed)
        self._check(self.L.hg_verify_batch_msgs_rlc_device(self.ctx, d_pool or None, pool_len, d_msg_off, d_msg_len,
                                                           d_pks, d_sigs, n, _ptr(sd), int(group), d_codes,
                                                           stream or None), "hg_verify_batch_msgs_rlc_device")

    def batch_rlc_stats(self) -> Tuple[int, int, int, int]:
        """The last verify_batch*_rlc* call: (groups checked, groups that
        failed, checks re-verified one by one, live checks whose key was not
        proven in G2)."""
        v = [ctypes.c_uint64() for _ in range(4)]
        self._check(self.L.hg_batch_rlc_stats(self.ctx, *[ctypes.byref(x) for x in v]), "hg_batch_rlc_stats")
        return tuple(int(x.value) for x in v)

    def g2_members(self, pks: bytes) -> Tuple[np.ndarray, np.ndarray]:
        """(flags, codes) of hg_debug_g2_member: the keys decoded by the
        context's flavor, flags[i] = 1 where the membership Miller loop proves
        key i in G2 (or it is the infinity key), 0 elsewhere."""
        a = _u8(pks)
        n = len(a) // 128
        flags = np.zeros(n, dtype=np.uint32)
        codes = np.zeros(n, dtype=np.int32)
        if n:
            self._check(self.L.hg_debug_g2_member(self.ctx, _ptr(a), n, _ptr(flags), _ptr(codes)),
                        "hg_debug_g2_member")
        return flags, codes

    def debug_batch_rlc_groups(self, msgs: Optional[Sequence[bytes]], pks: bytes, sigs: bytes, coeffs, group: int):
        """Everything up to the group verdicts with caller-given coefficients
        (hg_debug_batch_rlc_groups): (codes, group_codes, group_live). msgs
        None: every check on the context's message."""
        a, b = _u8(pks), _u8(sigs)
        k = np.ascontiguousarray(coeffs, dtype=np.uint64)
        n = len(b) // 64
        if len(a) != 128 * n or len(k) != n or (msgs is not None and len(msgs) != n):
            raise ValueError("one key, one signature, one coefficient (and one message) per check")
        ng = (n + int(group) - 1) // int(group) if group else 0
        codes = np.zeros(n, dtype=np.int32)
        gcodes = np.zeros(ng, dtype=np.int32)
        glive = np.zeros(ng, dtype=np.uint32)
        if msgs is None:
            pool, off, ln = np.zeros(0, dtype=np.uint8), None, None
        else:
            pool, off, ln = self.pack_messages(msgs)
        self._check(self.L.hg_debug_batch_rlc_groups(self.ctx, _ptr(pool) if len(pool) else None, len(pool),
                                                     _ptr(off) if off is not None else None,
                                                     _ptr(ln) if ln is not None else None, _ptr(a), _ptr(b), n,
                                                     _ptr(k), int(group), _ptr(codes), _ptr(gcodes), _ptr(glive)),
                    "hg_debug_batch_rlc_groups")
        return codes, gcodes, glive

    @staticmethod
    def debug_rlc_coeffs(seed: bytes, first: int, n: int) -> np.ndarray:
        """r_first .. r_(first+n-1) by the code the device runs (host only: no context, no GPU)."""
        out = np.zeros(n, dtype=np.uint64)
        rc = _lib.load().hg_debug_rlc_coeffs(_ptr(Engine._seed(seed)), int(first), n, _ptr(out))
        if rc != 0:
            raise HandelGPUError(f"hg_debug_rlc_coeffs: code {rc}")
        return out

    def debug_rlc_g1(self, sigs: bytes, coeffs, group: int) -> bytes:
        """Per group the marshal of sum coeffs[i] sigs[i] (hg_debug_rlc_g1)."""
        s = _u8(sigs)
        n = len(s) // 64
        k = np.ascontiguousarray(np.array([int(c) for c in coeffs], dtype=np.uint64))
        assert len(k) == n
        out = np.zeros(((n + group - 1) // group) * 64, dtype=np.uint8)
        self._check(self.L.hg_debug_rlc_g1(self.ctx, _ptr(s), n, _ptr(k), int(group), _ptr(out)), "hg_debug_rlc_g1")
        return out.tobytes()

    def debug_rlc_groups(self, reqs: np.ndarray, words: np.ndarray, sigs: bytes, coeffs, group: int):
        """The combination up to the group comparison with the given coefficients
        (hg_debug_rlc_groups): (codes, group_codes, group_live)."""
        reqs = np.ascontiguousarray(reqs, dtype=REQ_DTYPE)
        words = np.ascontiguousarray(words, dtype=np.uint64)
        s = _u8(sigs)
        n = len(reqs)
        k = np.ascontiguousarray(np.array([int(c) for c in coeffs], dtype=np.uint64))
        assert len(k) == n
        ng = (n + group - 1) // group
        codes = np.zeros(n, dtype=np.int32)
        gcodes = np.zeros(ng, dtype=np.int32)
        glive = np.zeros(ng, dtype=np.uint32)
        self._check(self.L.hg_debug_rlc_groups(self.ctx, _ptr(reqs), n, _ptr(words) if len(words) else None,
                                               len(words), _ptr(s), _ptr(k), int(group), _ptr(codes), _ptr(gcodes),
                                               _ptr(glive)), "hg_debug_rlc_groups")
        return codes, gcodes, glive

    # ------------------------------------------------------------ packet intake
    def packet_stride_words(self) -> int:
        """Bitset words per request slot of hg_parse_packets (largest level / 64)."""
        return int(self.L.hg_packet_stride_words(self.ctx))

    def parse_packets(self, pool, pkts: np.ndarray, stride: Optional[int] = None):
        """Handel.NewPacket's parse step for n packets (hg_parse_packets):
        returns (reqs[2n], words, sigs[2n*64], codes[2n]); slot i is packet i's
        multisignature, slot n + i its individual signature."""
        pkts = np.ascontiguousarray(pkts, dtype=PACKET_DTYPE)
        pool = _u8(pool)
        n = len(pkts)
        stride = self.packet_stride_words() if stride is None else int(stride)
        reqs, words, sigs, codes = _parse_outputs(n, stride)
        self._check(self.L.hg_parse_packets(self.ctx, _ptr(pool) if len(pool) else None, len(pool), _ptr(pkts), n,
                                            stride, _ptr(reqs), _ptr(words), _ptr(sigs), _ptr(codes)),
                    "hg_parse_packets")
        return reqs, words, sigs.tobytes(), codes

    def parse_packets_device(self, d_pool: int, pool_len: int, d_pkts: int, n: int, stride: int, d_reqs: int,
                             d_words: int, d_sigs: int, d_codes: int, stream: int = 0) -> None:
        """hg_parse_packets_device on raw device pointers (asynchronous)."""
        self._check(self.L.hg_parse_packets_device(self.ctx, d_pool or None, pool_len, d_pkts, n, stride, d_reqs,
                                                   d_words, d_sigs, d_codes, stream or None),
                    "hg_parse_packets_device")

    def packet_error(self, code: int, pkt) -> str:
        """The reference's text for a packet code (hg_packet_error)."""
        p = np.ascontiguousarray(np.asarray(pkt, dtype=PACKET_DTYPE).reshape(1))
        buf = ctypes.create_string_buffer(256)
        self.L.hg_packet_error(self.ctx, int(code), _ptr(p), buf, 256)
        return buf.value.decode()

    def verify_aggregate_msg(self, msg: bytes, reqs: np.ndarray, words: np.ndarray, sigs: bytes):
        """verify_aggregate with the message given per call: hashing and the
        batch under one lock hold of the context (hg_verify_aggregate_msg)."""
        reqs = np.ascontiguousarray(reqs, dtype=REQ_DTYPE)
        words = np.ascontiguousarray(words, dtype=np.uint64)
        m, s = _u8(msg), _u8(sigs)
        n = len(reqs)
        codes = np.zeros(n, dtype=np.int32)
        self._check(self.L.hg_verify_aggregate_msg(self.ctx, _ptr(m) if len(m) else None, len(m),
                                                   _ptr(reqs) if n else None, n,
                                                   _ptr(words) if len(words) else None, len(words),
                                                   _ptr(s) if n else None, _ptr(codes) if n else None, None),
                    "hg_verify_aggregate_msg")
        return codes

    def verify_multisig(self, bitlens, word_offsets, words: np.ndarray, sigs: bytes) -> np.ndarray:
        """VerifyMultiSignature (crypto.go:120-137) x n (hg_verify_multisig)."""
        bl = np.ascontiguousarray(bitlens, dtype=np.uint32)
        wo = np.ascontiguousarray(word_offsets, dtype=np.uint32)
        words = np.ascontiguousarray(words, dtype=np.uint64)
        s = _u8(sigs)
        n = len(bl)
        codes = np.zeros(n, dtype=np.int32)
        if n:
            self._check(self.L.hg_verify_multisig(self.ctx, _ptr(bl), _ptr(wo), n, _ptr(words) if len(words) else None,
                                                  len(words), _ptr(s), _ptr(codes)), "hg_verify_multisig")
        return codes

    # ----------------------------------------------------------- aggregates on their own messages
    def verify_aggregate_msgs_pool(self, pool, msg_off, msg_len, reqs: np.ndarray, words: np.ndarray, sigs: bytes,
                                   want_agg: bool = False):
        """hg_verify_aggregate_msgs on a caller-built pool: request i's message
        is pool[msg_off[i] : msg_off[i] + msg_len[i]]."""
        pool, s = _u8(pool), _u8(sigs)
        off = np.ascontiguousarray(msg_off, dtype=np.uint32)
        ln = np.ascontiguousarray(msg_len, dtype=np.uint32)
        reqs = np.ascontiguousarray(reqs, dtype=REQ_DTYPE)
        words = np.ascontiguousarray(words, dtype=np.uint64)
        n = len(reqs)
        if len(s) != 64 * n or len(off) != n or len(ln) != n:
            raise ValueError("one message range and 64 signature bytes per request")
        codes = np.zeros(n, dtype=np.int32)
        agg = np.zeros(n * 128, dtype=np.uint8) if want_agg else None
        if n:
            self._check(self.L.hg_verify_aggregate_msgs(self.ctx, _ptr(pool) if len(pool) else None, len(pool),
                                                        _ptr(off), _ptr(ln), _ptr(reqs), n,
                                                        _ptr(words) if len(words) else None, len(words), _ptr(s),
                                                        _ptr(codes), _ptr(agg)),
                        "hg_verify_aggregate_msgs")
        return (codes, agg.tobytes()) if want_agg else codes

    def verify_aggregate_msgs(self, msgs: Sequence[bytes], reqs: np.ndarray, words: np.ndarray, sigs: bytes,
                              want_agg: bool = False):
        """verify_aggregate for n requests that each carry their own message,
        in one batch (hg_verify_aggregate_msgs); the context's current message
        and tables stay as they are."""
        pool, off, ln = self.pack_messages(msgs)
        return self.verify_aggregate_msgs_pool(pool, off, ln, reqs, words, sigs, want_agg)

    def verify_aggregate_msgs_device(self, d_pool: int, pool_len: int, d_msg_off: int, d_msg_len: int, d_reqs: int,
                                     n: int, d_words: int, d_sigs: int, d_codes: int, d_agg: int = 0,
                                     stream: int = 0) -> None:
        """hg_verify_aggregate_msgs_device on raw device pointers (asynchronous);
        a message range past pool_len gives that request HG_ERR_ARG."""
        self._check(self.L.hg_verify_aggregate_msgs_device(self.ctx, d_pool or None, pool_len, d_msg_off, d_msg_len,
                                                           d_reqs, n, d_words or None, d_sigs, d_codes, d_agg or None,
                                                           stream or None),
                    "hg_verify_aggregate_msgs_device")

    def verify_multisig_msgs(self, msgs: Sequence[bytes], bitlens, word_offsets, words: np.ndarray,
                             sigs: bytes) -> np.ndarray:
        """VerifyMultiSignature(msgs[i], ...) (crypto.go:120-137) x n, each on
        its own message (hg_verify_multisig_msgs)."""
        pool, off, ln = self.pack_messages(msgs)
        bl = np.ascontiguousarray(bitlens, dtype=np.uint32)
        wo = np.ascontiguousarray(word_offsets, dtype=np.uint32)
        words = np.ascontiguousarray(words, dtype=np.uint64)
        s = _u8(sigs)
        n = len(bl)
        if len(s) != 64 * n or len(off) != n or len(wo) != n:
            raise ValueError("one message, one word offset and 64 signature bytes per multisignature")
        codes = np.zeros(n, dtype=np.int32)
        if n:
            self._check(self.L.hg_verify_multisig_msgs(self.ctx, _ptr(pool) if len(pool) else None, len(pool),
                                                       _ptr(off), _ptr(ln), _ptr(bl), _ptr(wo), n,
                                                       _ptr(words) if len(words) else None, len(words), _ptr(s),
                                                       _ptr(codes)), "hg_verify_multisig_msgs")
        return codes

    # ----------------------------------------------------------- ... one final exponentiation per group
    def verify_aggregate_msgs_rlc_pool(self, pool, msg_off, msg_len, reqs: np.ndarray, words: np.ndarray,
                                       sigs: bytes, seed: Optional[bytes] = None, group: int = RLC_GROUP):
        """hg_verify_aggregate_msgs_rlc on a caller-built pool."""
        pool, s = _u8(pool), _u8(sigs)
        off = np.ascontiguousarray(msg_off, dtype=np.uint32)
        ln = np.ascontiguousarray(msg_len, dtype=np.uint32)
        reqs = np.ascontiguousarray(reqs, dtype=REQ_DTYPE)
        words = np.ascontiguousarray(words, dtype=np.uint64)
        sd = self._seed(seed)
        n = len(reqs)
        if len(s) != 64 * n or len(off) != n or len(ln) != n:
            raise ValueError("one message range and 64 signature bytes per request")
        codes = np.zeros(n, dtype=np.int32)
        self._check(self.L.hg_verify_aggregate_msgs_rlc(self.ctx, _ptr(pool) if len(pool) else None, len(pool),
                                                        _ptr(off) if n else None, _ptr(ln) if n else None,
                                                        _ptr(reqs) if n else None, n,
                                                        _ptr(words) if len(words) else None, len(words),
                                                        _ptr(s) if n else None, _ptr(sd), int(group),
                                                        _ptr(codes) if n else None),
                    "hg_verify_aggregate_msgs_rlc")
        return codes

    def verify_aggregate_msgs_rlc(self, msgs: Sequence[bytes], reqs: np.ndarray, words: np.ndarray, sigs: bytes,
                                  seed: Optional[bytes] = None, group: int = RLC_GROUP) -> np.ndarray:
        """verify_aggregate_msgs (codes only) with one final exponentiation per
        `group` requests under random coefficients (hg_verify_aggregate_msgs_rlc):
        the same codes, an invalid signature accepted with probability <= 2^-64
        over `seed`, which the signatures' sender must not predict (None:
        os.urandom(32)). rlc_stats() reports on the call."""
        pool, off, ln = self.pack_messages(msgs)
        return self.verify_aggregate_msgs_rlc_pool(pool, off, ln, reqs, words, sigs, seed, group)

    def verify_aggregate_msgs_rlc_device(self, d_pool: int, pool_len: int, d_msg_off: int, d_msg_len: int,
                                         d_reqs: int, n: int, d_words: int, d_sigs: int, d_codes: int,
                                         seed: Optional[bytes] = None, group: int = RLC_GROUP,
                                         stream: int = 0) -> None:
        """hg_verify_aggregate_msgs_rlc_device on raw device pointers; synchronises
        `stream` once (the failed groups' member count sizes their exact recheck)."""
        sd = self._seed(seed)
        self._check(self.L.hg_verify_aggregate_msgs_rlc_device(self.ctx, d_pool or None, pool_len, d_msg_off,
                                                               d_msg_len, d_reqs, n, d_words or None, d_sigs,
                                                               _ptr(sd), int(group), d_codes, stream or None),
                    "hg_verify_aggregate_msgs_rlc_device")

    def verify_multisig_msgs_rlc(self, msgs: Sequence[bytes], bitlens, word_offsets, words: np.ndarray, sigs: bytes,
                                 seed: Optional[bytes] = None, group: int = RLC_GROUP) -> np.ndarray:
        """verify_multisig_msgs with one final exponentiation per `group`
        multisignatures (hg_verify_multisig_msgs_rlc)."""
        pool, off, ln = self.pack_messages(msgs)
        bl = np.ascontiguousarray(bitlens, dtype=np.uint32)
        wo = np.ascontiguousarray(word_offsets, dtype=np.uint32)
        words = np.ascontiguousarray(words, dtype=np.uint64)
        s = _u8(sigs)
        sd = self._seed(seed)
        n = len(bl)
        if len(s) != 64 * n or len(off) != n or len(wo) != n:
            raise ValueError("one message, one word offset and 64 signature bytes per multisignature")
        codes = np.zeros(n, dtype=np.int32)
        self._check(self.L.hg_verify_multisig_msgs_rlc(self.ctx, _ptr(pool) if len(pool) else None, len(pool),
                                                       _ptr(off) if n else None, _ptr(ln) if n else None,
                                                       _ptr(bl) if n else None, _ptr(wo) if n else None, n,
                                                       _ptr(words) if len(words) else None, len(words),
                                                       _ptr(s) if n else None, _ptr(sd), int(group),
                                                       _ptr(codes) if n else None), "hg_verify_multisig_msgs_rlc")
        return codes

    def debug_msgs_rlc_groups(self, msgs: Sequence[bytes], reqs: np.ndarray, words: np.ndarray, sigs: bytes, coeffs,
                              group: int):
        """The combination up to the group verdicts with the given coefficients
        (hg_debug_msgs_rlc_groups): (codes, group_codes, group_live)."""
        pool, off, ln = self.pack_messages(msgs)
        reqs = np.ascontiguousarray(reqs, dtype=REQ_DTYPE)
        words = np.ascontiguousarray(words, dtype=np.uint64)
        s = _u8(sigs)
        n = len(reqs)
        k = np.ascontiguousarray(np.array([int(c) for c in coeffs], dtype=np.uint64))
        assert len(k) == n and len(off) == n
        ng = (n + group - 1) // group
        codes = np.zeros(n, dtype=np.int32)
        gcodes = np.zeros(ng, dtype=np.int32)
        glive = np.zeros(ng, dtype=np.uint32)
        self._check(self.L.hg_debug_msgs_rlc_groups(self.ctx, _ptr(pool) if len(pool) else None, len(pool), _ptr(off),
                                                    _ptr(ln), _ptr(reqs), n, _ptr(words) if len(words) else None,
                                                    len(words), _ptr(s), _ptr(k), int(group), _ptr(codes),
                                                    _ptr(gcodes), _ptr(glive)), "hg_debug_msgs_rlc_groups")
        return codes, gcodes, glive

    def debug_msgs_rlc_points(self, msgs: Sequence[bytes], coeffs) -> bytes:
        """Per message the marshal of coeffs[i] hashedMessage(msgs[i]), zeros where
        the message cannot be hashed (hg_debug_msgs_rlc_points)."""
        pool, off, ln = self.pack_messages(msgs)
        n = len(off)
        k = np.ascontiguousarray(np.array([int(c) for c in coeffs], dtype=np.uint64))
        assert len(k) == n
        out = np.zeros(64 * n, dtype=np.uint8)
        if n:
            self._check(self.L.hg_debug_msgs_rlc_points(self.ctx, _ptr(pool) if len(pool) else None, len(pool),
                                                        _ptr(off), _ptr(ln), _ptr(k), n, _ptr(out)),
                        "hg_debug_msgs_rlc_points")
        return out.tobytes()

    def verify_aggregate_device(self, d_reqs: int, n: int, d_words: int, d_sigs: int, d_codes: int,
                                d_agg: int = 0, stream: int = 0):
        self._check(self.L.hg_verify_aggregate_device(self.ctx, d_reqs, n, d_words, d_sigs, d_codes,
                                                      d_agg or None, stream or None),
                    "hg_verify_aggregate_device")

    def verify_aggregate_device_bits(self, d_reqs: int, n: int, d_words: int, d_sigs: int, d_codes: int,
                                     d_bits: int, stream: int = 0):
        """verify_aggregate_device + the verdict bitset in one submission."""
        self._check(self.L.hg_verify_aggregate_device_bits(self.ctx, d_reqs, n, d_words, d_sigs, d_codes, d_bits,
                                                           stream or None),
                    "hg_verify_aggregate_device_bits")

    def aggregate_pk(self, reqs: np.ndarray, words: np.ndarray) -> Tuple[bytes, np.ndarray]:
        reqs = np.ascontiguousarray(reqs, dtype=REQ_DTYPE)
        words = np.ascontiguousarray(words, dtype=np.uint64)
        n = len(reqs)
        codes = np.zeros(n, dtype=np.int32)
        out = np.zeros(n * 128, dtype=np.uint8)
        self._check(self.L.hg_aggregate_pk(self.ctx, _ptr(reqs), n, _ptr(words) if len(words) else None,
                                           len(words), _ptr(out), _ptr(codes)), "hg_aggregate_pk")
        return out.tobytes(), codes

    def combine_g1(self, a: bytes, b: bytes) -> Tuple[bytes, np.ndarray]:
        x, y = _u8(a), _u8(b)
        n = len(x) // 64
        out = np.zeros(n * 64, dtype=np.uint8)
        codes = np.zeros(n, dtype=np.int32)
        self._check(self.L.hg_combine_g1(self.ctx, _ptr(x), _ptr(y), n, _ptr(out), _ptr(codes)), "hg_combine_g1")
        return out.tobytes(), codes

    def combine_g2(self, a: bytes, b: bytes) -> Tuple[bytes, np.ndarray]:
        x, y = _u8(a), _u8(b)
        n = len(x) // 128
        out = np.zeros(n * 128, dtype=np.uint8)
        codes = np.zeros(n, dtype=np.int32)
        self._check(self.L.hg_combine_g2(self.ctx, _ptr(x), _ptr(y), n, _ptr(out), _ptr(codes)), "hg_combine_g2")
        return out.tobytes(), codes

    def pair(self, g1s: bytes, g2s: bytes) -> Tuple[bytes, np.ndarray]:
        x, y = _u8(g1s), _u8(g2s)
        n = len(x) // 64
        out = np.zeros(n * 384, dtype=np.uint8)
        codes = np.zeros(n, dtype=np.int32)
        self._check(self.L.hg_pair(self.ctx, _ptr(x), _ptr(y), n, _ptr(out), _ptr(codes)), "hg_pair")
        return out.tobytes(), codes

    def keygen(self, scalars_be: bytes) -> bytes:
        s = _u8(scalars_be)
        n = len(s) // 32
        out = np.zeros(n * 128, dtype=np.uint8)
        self._check(self.L.hg_keygen(self.ctx, _ptr(s), n, _ptr(out)), "hg_keygen")
        return out.tobytes()

    def sign(self, scalars_be: bytes) -> bytes:
        s = _u8(scalars_be)
        n = len(s) // 32
        out = np.zeros(n * 64, dtype=np.uint8)
        self._check(self.L.hg_sign(self.ctx, _ptr(s), n, _ptr(out)), "hg_sign")
        return out.tobytes()

    def sign_msg(self, msg: bytes, scalars_be: bytes) -> bytes:
        """SecretKey.Sign(msg) x n under one lock hold (hg_sign_msg); raises on EOF."""
        m, sc = _u8(msg), _u8(scalars_be)
        n = len(sc) // 32
        out = np.zeros(n * 64, dtype=np.uint8)
        rc = self.L.hg_sign_msg(self.ctx, _ptr(m) if len(m) else None, len(m), _ptr(sc) if n else None, n,
                                _ptr(out) if n else None)
        self._check(rc, "hg_sign_msg")
        return out.tobytes()

    def fp12_op(self, op: int, a: bytes, b: bytes = None) -> bytes:
        """Team Fp12 building-block probe (hg_debug_fp12); 384-byte GT marshals."""
        x = _u8(a)
        y = _u8(b) if b is not None else x
        n = len(x) // 384
        out = np.zeros(n * 384, dtype=np.uint8)
        self._check(self.L.hg_debug_fp12(self.ctx, op, _ptr(x), _ptr(y), n, _ptr(out)), "hg_debug_fp12")
        return out.tobytes()

    def xinst_region_elems(self, inst: int, form: int = 0) -> int:
        """Elements of the team region of instance `inst` in `form` (hg_debug_xinst with n = 0)."""
        e = ctypes.c_int()
        self._check(self.L.hg_debug_xinst(self.ctx, int(inst), int(form), None, 0, None, ctypes.byref(e)),
                    "hg_debug_xinst")
        return e.value

    def xinst(self, inst: int, regions: np.ndarray, form: int = 0) -> np.ndarray:
        """One bound team-program instance on raw team regions (hg_debug_xinst):
        regions and the result are uint32 arrays (n, region_elems, 10)."""
        r = np.ascontiguousarray(regions, dtype=np.uint32)
        elems = self.xinst_region_elems(inst, form)
        if r.ndim != 3 or r.shape[1:] != (elems, 10):
            raise ValueError(f"regions of shape {r.shape}, want (n, {elems}, 10)")
        out = np.zeros_like(r)
        n = r.shape[0]
        self._check(self.L.hg_debug_xinst(self.ctx, int(inst), int(form), _ptr(r) if n else None, n,
                                          _ptr(out) if n else None, None), "hg_debug_xinst")
        return out

    def field_words(self, op: int) -> Tuple[int, int]:
        """Words of one case of per-thread probe `op` going in and coming out (hg_debug_field with n = 0)."""
        wi, wo = ctypes.c_int(), ctypes.c_int()
        self._check(self.L.hg_debug_field(self.ctx, int(op), None, 0, None, ctypes.byref(wi), ctypes.byref(wo)),
                    "hg_debug_field")
        return wi.value, wo.value

    def field_op(self, op: int, cases: np.ndarray) -> np.ndarray:
        """One per-thread primitive of bn256_fp.h / bn256_curve.h on raw limbs
        (hg_debug_field): cases is a uint32 array (n, in_words), the result (n, out_words)."""
        a = np.ascontiguousarray(cases, dtype=np.uint32)
        wi, wo = self.field_words(op)
        if a.ndim != 2 or a.shape[1] != wi:
            raise ValueError(f"cases of shape {a.shape}, want (n, {wi})")
        n = a.shape[0]
        out = np.zeros((n, wo), dtype=np.uint32)
        self._check(self.L.hg_debug_field(self.ctx, int(op), _ptr(a) if n else None, n, _ptr(out) if n else None,
                                          None, None), "hg_debug_field")
        return out

    # hg_debug_gt_entries' tables
    GT_KEYS, GT_WIN8, GT_WIN16, GT_BLOCKS = 0, 1, 2, 3

    def gt_layout(self) -> dict:
        """The current message's GT table set as built (hg_debug_gt_layout):
        level, torus, nreg, nwin8, nwin16 and blocks = {k: (base, count)}."""
        out = np.zeros(_lib.HG_GT_LAYOUT_WORDS, dtype=np.int32)
        self._check(self.L.hg_debug_gt_layout(self.ctx, _ptr(out)), "hg_debug_gt_layout")
        top = int(out[5])
        return {"level": int(out[0]), "torus": bool(out[1]), "nreg": int(out[2]), "nwin8": int(out[3]),
                "nwin16": int(out[4]), "blocks": {k: (int(out[6 + k]), int(out[30 + k])) for k in range(4, top + 1)}}

    def gt_entries(self, table: int, first: int, count: int) -> np.ndarray:
        """count entries from `first` of one GT table, raw (hg_debug_gt_entries): uint32 (count, 120)."""
        out = np.zeros((int(count), 120), dtype=np.uint32)
        self._check(self.L.hg_debug_gt_entries(self.ctx, int(table), int(first), int(count), _ptr(out)),
                    "hg_debug_gt_entries")
        return out

    def gt_fold(self, reqs: np.ndarray, words: np.ndarray, chunk: int):
        """The GT fold alone over the built tables in `chunk` terms per chunk
        (hg_debug_gt_fold): (y uint32 (n, 120), codes)."""
        reqs = np.ascontiguousarray(reqs, dtype=REQ_DTYPE)
        words = np.ascontiguousarray(words, dtype=np.uint64)
        n = len(reqs)
        y = np.zeros((n, 120), dtype=np.uint32)
        codes = np.zeros(n, dtype=np.int32)
        self._check(self.L.hg_debug_gt_fold(self.ctx, _ptr(reqs), n, _ptr(words) if len(words) else None, len(words),
                                            int(chunk), _ptr(y), _ptr(codes)), "hg_debug_gt_fold")
        return y, codes

    def fp_mul(self, a: np.ndarray, b: np.ndarray) -> np.ndarray:
        a = np.ascontiguousarray(a, dtype=np.uint32)
        b = np.ascontiguousarray(b, dtype=np.uint32)
        n = a.shape[0]
        out = np.zeros((n, 8), dtype=np.uint32)
        self._check(self.L.hg_debug_fp_mul(self.ctx, _ptr(a), _ptr(b), n, _ptr(out)), "hg_debug_fp_mul")
        return out

    def timing_enable(self, on: bool = True):
        self._check(self.L.hg_timing_enable(self.ctx, int(on)), "hg_timing_enable")

    def timing_read(self) -> Tuple[float, int]:
        ms = ctypes.c_double()
        k = ctypes.c_int()
        self._check(self.L.hg_timing_read(self.ctx, ctypes.byref(ms), ctypes.byref(k)), "hg_timing_read")
        return ms.value, k.value

    def timing_read_phase(self, phase: int) -> Tuple[float, int]:
        ms = ctypes.c_double()
        k = ctypes.c_int()
        self._check(self.L.hg_timing_read_phase(self.ctx, int(phase), ctypes.byref(ms), ctypes.byref(k)),
                    "hg_timing_read_phase")
        return ms.value, k.value

    def sync(self):
        self._check(self.L.hg_sync(self.ctx), "hg_sync")


def _parse_outputs(n: int, stride: int):
    return (np.zeros(2 * n, dtype=REQ_DTYPE), np.zeros(2 * n * stride, dtype=np.uint64),
            np.zeros(2 * n * 64, dtype=np.uint8), np.zeros(2 * n, dtype=np.int32))


class Batcher:
    """The native launch-merging queue on one engine (hg_batcher_*): callers
    (one thread per Handel instance) submit single aggregate requests; a
    dispatcher thread merges what is queued into one launch per message.
    The engine must outlive the batcher."""

    def __init__(self, engine: Engine, max_batch: int = 4096, max_wait_us: int = 200):
        self.engine = engine
        self.L = engine.L
        h = ctypes.c_void_p()
        rc = self.L.hg_batcher_create(engine.ctx, max_batch, max_wait_us, ctypes.byref(h))
        if rc != 0:
            raise HandelGPUError(f"hg_batcher_create: code {rc}")
        self.b = h

    def close(self):
        if getattr(self, "b", None):
            self.L.hg_batcher_destroy(self.b)
            self.b = None

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass

    def submit(self, msg: bytes, offset: int, bitlen: int, level_size: int, words, sig: bytes) -> int:
        """Queues one request (hg_batcher_submit); returns the ticket handle."""
        m = _u8(msg)
        req = np.array([(offset, bitlen, level_size, 0)], dtype=REQ_DTYPE)
        w = np.ascontiguousarray(words, dtype=np.uint64)
        if len(w) < (int(bitlen) + 63) // 64:  # hg_batcher_submit copies ceil(bitlen / 64) words
            raise ValueError(f"{bitlen} bits need {(int(bitlen) + 63) // 64} words, got {len(w)}")
        sg = _u8(sig)
        if len(sg) != 64:
            raise ValueError("signature must be 64 bytes")
        t = ctypes.c_void_p()
        rc = self.L.hg_batcher_submit(self.b, _ptr(m) if len(m) else None, len(m), _ptr(req),
                                      _ptr(w) if len(w) else None, _ptr(sg), ctypes.byref(t))
        if rc != 0:
            raise HandelGPUError(f"hg_batcher_submit: code {rc}")
        return t.value

    def wait(self, ticket: int) -> int:
        """The request's hg_code (hg_batcher_wait); releases the ticket."""
        code = ctypes.c_int32(-1)
        rc = self.L.hg_batcher_wait(self.b, ctypes.c_void_p(ticket), ctypes.byref(code))
        if rc != 0:
            raise HandelGPUError(f"hg_batcher_wait: code {rc}")
        return int(code.value)

    def verify(self, msg: bytes, offset: int, bitlen: int, level_size: int, words, sig: bytes) -> int:
        """One processing.go verifySignature through the queue (blocking)."""
        return self.wait(self.submit(msg, offset, bitlen, level_size, words, sig))

    def stats(self) -> Tuple[int, int]:
        """(batches launched, requests verified) so far."""
        b, r = ctypes.c_uint64(), ctypes.c_uint64()
        self.L.hg_batcher_stats(self.b, ctypes.byref(b), ctypes.byref(r))
        return b.value, r.value


class Stores:
    """The device-resident stores of the Handel instances `receivers` on one
    engine (hg_stores_*): per receiver and level the best bitset, whether there
    is one, and the verified individual signatures. Scores parsed packet slots
    (store.go:111-183) and picks the k best per store (processing.go:171-220).
    The engine must outlive the stores; they die with the registry they were
    created on."""

    def __init__(self, engine: Engine, receivers, max_packets: int):
        self.engine = engine
        self.L = engine.L
        self.receivers = np.ascontiguousarray(receivers, dtype=np.uint32)
        self.max_packets = int(max_packets)
        self.stride = engine.packet_stride_words()
        h = ctypes.c_void_p()
        rc = self.L.hg_stores_create(engine.ctx, _ptr(self.receivers) if len(self.receivers) else None,
                                     len(self.receivers), self.max_packets, ctypes.byref(h))
        if rc != 0:
            raise HandelGPUError(f"hg_stores_create: code {rc}")
        self.h = h
        engine.__dict__.setdefault("_stores", []).append(weakref.ref(self))

    def close(self):
        if getattr(self, "h", None):
            for ref in getattr(self, "_pools", []):  # pools go before their stores
                pool = ref()
                if pool is not None:
                    pool.close()
            self.L.hg_stores_destroy(self.h)
            self.h = None

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass

    def update(self, ups: np.ndarray, words: np.ndarray) -> None:
        """Replaces the state of the named (receiver, level) pairs (hg_stores_update)."""
        ups = np.ascontiguousarray(ups, dtype=STORE_UPDATE_DTYPE)
        words = np.ascontiguousarray(words, dtype=np.uint64)
        self.engine._check(self.L.hg_stores_update(self.h, _ptr(ups) if len(ups) else None, len(ups),
                                                   _ptr(words) if len(words) else None, len(words)),
                           "hg_stores_update")

    def read(self, receiver: int, level: int) -> Tuple[np.ndarray, np.ndarray, bool]:
        """(best words, verified-individual words, has best) of one level (hg_stores_read)."""
        best = np.zeros(self.stride, dtype=np.uint64)
        indiv = np.zeros(self.stride, dtype=np.uint64)
        has = ctypes.c_int()
        self.engine._check(self.L.hg_stores_read(self.h, int(receiver), int(level), _ptr(best), _ptr(indiv),
                                                 ctypes.byref(has)), "hg_stores_read")
        return best, indiv, bool(has.value)

    def evaluate(self, pkts: np.ndarray, words: np.ndarray, codes: np.ndarray, live=None,
                 stride: Optional[int] = None) -> np.ndarray:
        """Scores of the 2n slots hg_parse_packets wrote (hg_stores_evaluate)."""
        pkts = np.ascontiguousarray(pkts, dtype=PACKET_DTYPE)
        words = np.ascontiguousarray(words, dtype=np.uint64)
        codes = np.ascontiguousarray(codes, dtype=np.int32)
        live = None if live is None else np.ascontiguousarray(live, dtype=np.uint8)
        n = len(pkts)
        stride = self.stride if stride is None else int(stride)
        if len(words) != 2 * n * stride or len(codes) != 2 * n or (live is not None and len(live) != 2 * n):
            raise ValueError("words, codes and live must cover 2n slots")
        scores = np.zeros(2 * n, dtype=np.int32)
        if n:
            self.engine._check(self.L.hg_stores_evaluate(self.h, _ptr(pkts), n, stride, _ptr(words), _ptr(codes),
                                                         _ptr(live), _ptr(scores)), "hg_stores_evaluate")
        return scores

    def evaluate_device(self, d_pkts: int, n: int, stride: int, d_words: int, d_codes: int, d_live: int,
                        d_scores: int, stream: int = 0) -> None:
        """hg_stores_evaluate_device on raw device pointers (asynchronous)."""
        self.engine._check(self.L.hg_stores_evaluate_device(self.h, d_pkts, n, stride, d_words, d_codes,
                                                            d_live or None, d_scores, stream or None),
                           "hg_stores_evaluate_device")

    def select_capacity(self, n: int, k: int) -> int:
        return int(self.L.hg_stores_select_capacity(self.h, int(n), int(k)))

    def select_device(self, d_pkts: int, n: int, d_scores: int, k: int, d_reqs: int, d_sigs: int, d_sel: int,
                      d_count: int, d_out_reqs: int, d_out_sigs: int, stream: int = 0) -> None:
        """hg_stores_select_device on raw device pointers (asynchronous): the k
        best slots per store, gathered into verification requests."""
        self.engine._check(self.L.hg_stores_select_device(self.h, d_pkts, n, d_scores, int(k), d_reqs, d_sigs, d_sel,
                                                          d_count, d_out_reqs, d_out_sigs, stream or None),
                           "hg_stores_select_device")

    # -- the opt-in device store: merge and Combined (hg_merge.hip)
    def enable_merge(self) -> None:
        """Allocates the signature tables (hg_stores_enable_merge): the set then
        also runs store.go's Store / unsafeCheckMerge and Combined."""
        self.engine._check(self.L.hg_stores_enable_merge(self.h), "hg_stores_enable_merge")

    def update_sigs(self, recs: np.ndarray, sigs) -> None:
        """Loads signatures from the host (hg_stores_update_sigs): recs of
        STORE_SIG_DTYPE, sigs the 64-byte marshals recs' sig_off index."""
        recs = np.ascontiguousarray(recs, dtype=STORE_SIG_DTYPE)
        sigs = _u8(sigs)
        if len(sigs) % 64:
            raise ValueError("sigs must hold 64-byte marshals")
        self.engine._check(self.L.hg_stores_update_sigs(self.h, _ptr(recs) if len(recs) else None, len(recs),
                                                        _ptr(sigs) if len(sigs) else None, len(sigs) // 64),
                           "hg_stores_update_sigs")

    def read_best(self, receiver: int, level: int) -> Tuple[np.ndarray, bytes, int]:
        """(best words, best signature, HG_STORE_HAS_BEST | HG_STORE_BEST_SIG
        flags) of one level; level 0 is the own signature (hg_stores_read_best)."""
        best = np.zeros(self.stride, dtype=np.uint64)
        sig = np.zeros(64, dtype=np.uint8)
        flags = ctypes.c_int()
        self.engine._check(self.L.hg_stores_read_best(self.h, int(receiver), int(level), _ptr(best), _ptr(sig),
                                                      ctypes.byref(flags)), "hg_stores_read_best")
        return best, sig.tobytes(), int(flags.value)

    def merge_device(self, d_pkts: int, n: int, d_sel: int, d_count: int, capacity: int, d_vcodes: int, stride: int,
                     d_words: int, d_sigs: int, d_results: int, d_changed: int, d_nchanged: int,
                     stream: int = 0) -> None:
        """hg_stores_merge_device on raw device pointers (asynchronous):
        store.go:82-99 Store for the verified picks of one intake step."""
        self.engine._check(self.L.hg_stores_merge_device(self.h, d_pkts or None, n, d_sel or None, d_count or None,
                                                         int(capacity), d_vcodes or None, int(stride),
                                                         d_words or None, d_sigs or None, d_results or None,
                                                         d_changed or None, d_nchanged or None, stream or None),
                           "hg_stores_merge_device")

    def combined_device(self, d_queries: int, m: int, words_stride: int, d_codes: int, d_bitlens: int, d_words: int,
                        d_sigs: int, stream: int = 0) -> None:
        """hg_stores_combined_device on raw device pointers (asynchronous)."""
        self.engine._check(self.L.hg_stores_combined_device(self.h, d_queries or None, int(m), int(words_stride),
                                                            d_codes or None, d_bitlens or None, d_words or None,
                                                            d_sigs or None, stream or None),
                           "hg_stores_combined_device")

    def combined(self, queries, words_stride: Optional[int] = None):
        """store.go:248-262 Combined / :238-246 FullSignature for (receiver,
        level) queries (level HG_STORE_LEVEL_FULL: the full signature):
        (codes, bit lengths, words[m, words_stride], signatures[m, 64])."""
        q = np.ascontiguousarray(queries, dtype=STORE_QUERY_DTYPE)
        m = len(q)
        ws = (int(self.engine.L.hg_registry_size(self.engine.ctx)) + 63) // 64 if words_stride is None else int(words_stride)
        codes = np.zeros(m, dtype=np.int32)
        bitlens = np.zeros(m, dtype=np.uint32)
        words = np.zeros((m, ws), dtype=np.uint64)
        sigs = np.zeros((m, 64), dtype=np.uint8)
        if m:
            self.engine._check(self.L.hg_stores_combined(self.h, _ptr(q), m, ws, _ptr(codes), _ptr(bitlens),
                                                         _ptr(words), _ptr(sigs)), "hg_stores_combined")
        return codes, bitlens, words, sigs


class Pool:
    """Handel's queue of parsed signatures kept in HBM across intake steps
    (hg_stores_pool_*): `append_device` adds the admitted slots of a parsed
    batch, `step_device` is one readTodos pass over the whole queue whose picks
    come out as a parsed batch. The stores must outlive the pool (closing them
    closes their pools first)."""

    def __init__(self, stores: Stores, capacity_slots: int):
        self.stores = stores
        self.engine = stores.engine
        self.L = stores.L
        self.capacity_slots = int(capacity_slots)
        h = ctypes.c_void_p()
        rc = self.L.hg_stores_pool_create(stores.h, self.capacity_slots, ctypes.byref(h))
        if rc != 0:
            raise HandelGPUError(f"hg_stores_pool_create: code {rc}")
        self.h = h
        stores.__dict__.setdefault("_pools", []).append(weakref.ref(self))

    def close(self):
        if getattr(self, "h", None):
            self.L.hg_stores_pool_destroy(self.h)
            self.h = None

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass

    def bytes(self) -> int:
        """Device memory the pool holds (hg_stores_pool_bytes)."""
        return int(self.L.hg_stores_pool_bytes(self.h))

    def append_device(self, d_pkts: int, n: int, stride: int, d_reqs: int, d_words: int, d_sigs: int, d_codes: int,
                      d_live: int, stream: int = 0) -> None:
        """hg_stores_pool_append_device on raw device pointers (asynchronous):
        the outputs of one hg_parse_packets_device call."""
        self.engine._check(self.L.hg_stores_pool_append_device(self.h, d_pkts or None, int(n), int(stride),
                                                               d_reqs or None, d_words or None, d_sigs or None,
                                                               d_codes or None, d_live or None, stream or None),
                           "hg_stores_pool_append_device")

    def select_capacity(self, k: int) -> int:
        return int(self.L.hg_stores_pool_select_capacity(self.h, int(k)))

    def step_device(self, k: int, capacity: int, d_out_pkts: int, d_sel: int, d_count: int, d_out_reqs: int,
                    d_out_words: int, d_out_sigs: int, d_out_scores: int, stream: int = 0) -> None:
        """hg_stores_pool_step_device on raw device pointers (asynchronous)."""
        self.engine._check(self.L.hg_stores_pool_step_device(self.h, int(k), int(capacity), d_out_pkts or None,
                                                             d_sel or None, d_count or None, d_out_reqs or None,
                                                             d_out_words or None, d_out_sigs or None,
                                                             d_out_scores or None, stream or None),
                           "hg_stores_pool_step_device")

    def count(self) -> int:
        """Slots queued now (hg_stores_pool_count; synchronous)."""
        n = ctypes.c_size_t()
        self.engine._check(self.L.hg_stores_pool_count(self.h, ctypes.byref(n)), "hg_stores_pool_count")
        return int(n.value)

    def read(self, receiver: int) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """(packet records, individual flags, last marks) of the receiver's
        queued slots in queue order (hg_stores_pool_read)."""
        cap = self.capacity_slots
        pkts = np.zeros(cap, dtype=PACKET_DTYPE)
        ind = np.zeros(cap, dtype=np.uint8)
        scores = np.zeros(cap, dtype=np.int32)
        n = ctypes.c_size_t()
        self.engine._check(self.L.hg_stores_pool_read(self.h, int(receiver), cap, _ptr(pkts), _ptr(ind), _ptr(scores),
                                                      ctypes.byref(n)), "hg_stores_pool_read")
        m = int(n.value)
        return pkts[:m], ind[:m], scores[:m]

    def clear(self) -> None:
        self.engine._check(self.L.hg_stores_pool_clear(self.h), "hg_stores_pool_clear")


class DeviceLane:
    """One hg_lane of an engine for batches already in HBM
    (hg_lane_submit_device): each lane has its own streams and workspaces over
    the engine's one registry and table set, so several lanes keep several
    batches in flight. pad=False: the unpadded pairing kernel (two batches'
    waves share the SIMDs). The engine must outlive the lane."""

    def __init__(self, engine: Engine, max_batch: int, pad: bool = True, overlap: bool = True):
        self.engine = engine
        self.L = engine.L
        h = ctypes.c_void_p()
        # staging capacity for host batches: 64 words (4096 bits) per request
        rc = self.L.hg_lane_create(engine.ctx, max_batch, max_batch * 64, 1 if overlap else 0, ctypes.byref(h))
        if rc != 0:
            raise HandelGPUError(f"hg_lane_create: code {rc}")
        self.h = h
        if not pad:
            engine._check(self.L.hg_lane_set_pairing_padding(self.h, 0), "hg_lane_set_pairing_padding")

    def set_latency_form(self, max_checks: int):
        """hg_lane_set_latency_form: padded batches of at most max_checks
        checks run the two-wave pairing kernel (0: never)."""
        self.engine._check(self.L.hg_lane_set_latency_form(self.h, int(max_checks)), "hg_lane_set_latency_form")

    def close(self):
        if getattr(self, "h", None):
            self.L.hg_lane_destroy(self.h)
            self.h = None

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass

    def submit_device(self, d_reqs: int, n: int, d_words: int, d_sigs: int, d_codes: int, d_bits: int = 0,
                      stream: int = 0):
        """Enqueues the batch after `stream`'s earlier work; `stream` waits for its verdicts."""
        self.engine._check(self.L.hg_lane_submit_device(self.h, d_reqs, n, d_words, d_sigs, d_codes, d_bits or None,
                                                        stream or None), "hg_lane_submit_device")

    def wait(self):
        self.engine._check(self.L.hg_lane_wait(self.h), "hg_lane_wait")

    @property
    def stream(self) -> int:
        """The lane's launch stream (hipStream_t as int): as submit_device's
        `stream`, the batch is ordered only after the lane's own earlier ones."""
        return int(self.L.hg_lane_stream(self.h) or 0)


def requests_array(items: Sequence[Tuple[int, int, int, int]]) -> np.ndarray:
    return np.array(items, dtype=REQ_DTYPE)
