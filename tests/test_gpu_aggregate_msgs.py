"""GPU parity of aggregate verification with one message per request
(hg_verify_aggregate_msgs, hg_verify_aggregate_msgs_device,
hg_verify_multisig_msgs) against the C oracle, called once per
request with that request's message and n = 1 (oracle/bn256_ref.c's
ref_verify_aggregate has DESIGN §1's precedence for one message, so no special
case is needed). Codes and aggregate-key marshals: the bar is exact equality.

Registries of 67 keys (a ragged last 8-key window, a ragged last 64-bit word,
level ranges clipped at N) and 300 keys (requests over several words, the
widest lane class of the fold). Signatures are (sum of sk) h_i G1 through
hg_debug_g1_base_mul, h_i from hg_debug_hash_scalar: no per-message hashing
route is used to make them."""

import ctypes
from typing import NamedTuple

import numpy as np
import pytest

from handel_amd import partitioner as P
from oracle import bn256_oracle as O
from oracle import ref_lib as R
from tests import _fixtures as F
from tests import _msgs_fixtures as M

pytestmark = pytest.mark.gpu

HG_OK, SIG_INVALID, HASH_EOF, LEVEL, SIG_UNMARSHAL, EMPTY_AGG, MULTI_SIZES, HG_ERR_ARG = 0, 1, 2, 3, 5, 6, 13, 100
OFF_CURVE_G1 = (1).to_bytes(32, "big") + (1).to_bytes(32, "big")
SIZES = (67, 300)


@pytest.fixture(scope="module", autouse=True)
def torch_first():
    """torch's HIP runtime before the engines' (as tests/conftest.py does for
    the session engines): the device variant's test moves tensors to the GPU."""
    import torch

    if torch.cuda.is_available():
        torch.cuda.set_device(0)
        torch.zeros(1, device="cuda")


@pytest.fixture(scope="module")
def msgs():
    out = M.boundary_set()
    M.check_boundary_set(out)
    return out


# ---------------------------------------------------------------- the requests
class Case(NamedTuple):
    what: str
    msg: bytes     # the request's message
    off: int
    size: int      # level_size
    bits: tuple    # the bitset (len(bits) is the request's bitlen)
    sig: str       # valid | tamper | undecodable
    signed: bytes  # the message the signature is made for (hashable)
    expect: int    # the code this request is in the batch for


def _level_ranges(N):
    """Handel level ranges (partitioner.go rangeLevel) of three nodes: every
    size from one key up, clipped at N for the last ids, then the registry."""
    out = []
    for node in (0, N - 1, N // 2 + 1):
        for level in range(1, P.log2_ceil(N) + 1):
            try:
                lo, hi = P.range_level(node, N, level)
            except P.PartitionerError:
                continue
            if (lo, hi - lo) not in out:
                out.append((lo, hi - lo))
    out.append((0, N))
    return out


def _build(N, msgs):
    good = [m for m, h in msgs if h]
    eof = [m for m, h in msgs if not h]
    rng = np.random.default_rng(N)
    ranges = _level_ranges(N)
    assert {s for _, s in ranges} >= {1, 2, 4, 8, 16, 32, 64, N}
    assert any(o + s == N and s & (s - 1) for o, s in ranges[:-1])  # a range clipped at N
    def some(s):  # a random bitset of s bits, never empty
        bits = rng.random(s) < 0.6
        bits[int(rng.integers(s))] = True
        return tuple(bool(b) for b in bits)

    full, sparse = (True,) * N, tuple(i % 5 == 0 for i in range(N))
    nearly = tuple(i not in (3, N - 2) for i in range(N))
    mid = ranges[4]
    cases = [  # the first five are of five kinds: n = 1, 4, 5 take prefixes
        Case("valid level range", good[0], *mid, some(mid[1]), "valid", good[0], HG_OK),
        Case("EOF message", eof[0], *mid, some(mid[1]), "valid", good[0], HASH_EOF),
        Case("valid for another request's message", good[1], *mid, some(mid[1]), "valid", good[0], SIG_INVALID),
        Case("full registry, block complement", good[2], 0, N, nearly, "valid", good[2], HG_OK),
        Case("EOF + undecodable signature", eof[1], *mid, some(mid[1]), "undecodable", good[0], SIG_UNMARSHAL),
        Case("full registry, every bit", good[3], 0, N, full, "valid", good[3], HG_OK),
        Case("full registry, sparse (no complement)", good[4], 0, N, sparse, "valid", good[4], HG_OK),
        Case("single key", good[5], N - 1, 1, (True,), "valid", good[5], HG_OK),
        Case("off the window grid", good[6], 3, 13, some(13), "valid", good[6], HG_OK),
        Case("tampered", good[7], *mid, some(mid[1]), "tamper", good[7], SIG_INVALID),
        Case("undecodable signature", good[8], *mid, some(mid[1]), "undecodable", good[8], SIG_UNMARSHAL),
        Case("bitlen != level_size", good[0], 0, 16, some(15), "valid", good[0], LEVEL),
        Case("range past the registry", good[1], N - 8, 16, some(16), "valid", good[1], LEVEL),
        Case("empty bitset", good[2], *mid, (False,) * mid[1], "valid", good[2], EMPTY_AGG),
        Case("EOF (empty message)", b"", 0, N, full, "valid", good[0], HASH_EOF),
        Case("EOF + tampered", eof[2], *mid, some(mid[1]), "tamper", good[0], HASH_EOF),
        Case("EOF + level error", eof[3], 0, 16, some(17), "valid", good[0], LEVEL),
        Case("EOF + empty bitset", eof[4], *mid, (False,) * mid[1], "valid", good[0], HASH_EOF),
        Case("level error + undecodable signature", good[3], 0, 16, some(15), "undecodable", good[3], SIG_UNMARSHAL),
        Case("empty bitset + undecodable signature", good[4], 8, 8, (False,) * 8, "undecodable", good[4], SIG_UNMARSHAL),
        Case("EOF + level error + undecodable", eof[5], 0, 8, some(9), "undecodable", good[0], SIG_UNMARSHAL),
    ]
    for i, (o, s) in enumerate(ranges):  # every level range, valid, messages of every boundary length
        m = msgs[i % len(msgs)][0]
        cases.append(Case("level range %d+%d" % (o, s), m, o, s, some(s), "valid", m if M.hashable(m) else good[0],
                          HG_OK if M.hashable(m) else HASH_EOF))
    i = 0
    while len(cases) < 67:
        (o, s), m = ranges[(3 * i) % len(ranges)], good[i % len(good)]
        cases.append(Case("filler", m, o, s, some(s), "tamper" if i % 4 == 3 else "valid", m,
                          SIG_INVALID if i % 4 == 3 else HG_OK))
        i += 1
    assert len(cases) == 67
    return cases


def _hash_scalar(eng, msg):
    k = (ctypes.c_uint32 * 8)()
    rc = eng.L.hg_debug_hash_scalar(ctypes.create_string_buffer(msg, len(msg)) if msg else None, len(msg), k)
    assert rc == HG_OK, "signatures are made on hashable messages"
    return sum(int(w) << (32 * i) for i, w in enumerate(k))


def _sign(eng, ks, cases):
    """(sum of sk over the request's set bits inside the registry) * h * G1,
    + G1 when tampered: one fixed-base launch for the batch."""
    scalars = []
    for c in cases:
        sk = sum(ks[c.off + i] for i, b in enumerate(c.bits) if b and c.off + i < len(ks) and ks[c.off + i] is not None)
        scalars.append((sk * _hash_scalar(eng, c.signed) + (c.sig == "tamper")) % O.ORDER)
    out = eng.debug_g1_base_mul(scalars)
    return b"".join(OFF_CURVE_G1 if c.sig == "undecodable" else out[64 * i:64 * i + 64] for i, c in enumerate(cases))


def _pack(cases):
    from handel_amd.engine import REQ_DTYPE

    reqs, words = F.pack_requests([(c.off, c.size) for c in cases], [list(c.bits) for c in cases])
    return np.array(reqs, dtype=REQ_DTYPE), words


def _oracle(reg, cases, sigs, fast=True):
    """One oracle call per request, on its own message, n = 1."""
    codes, aggs = [], []
    for i, c in enumerate(cases):
        w = np.array(O.bitset_words(list(c.bits)), dtype=np.uint64)
        code, agg = R.verify_aggregate(c.msg, reg, [c.off], [len(c.bits)], [c.size], w, [0], sigs[64 * i:64 * i + 64],
                                       fast=fast, want_agg=True)
        codes.append(int(code[0]))
        aggs.append(agg)
    return np.array(codes, dtype=np.int32), b"".join(aggs)


def _fold_cf(eng, got, sigs):
    """The engine's codes in the C oracle's terms: the oracle knows one code
    for a signature that does not unmarshal (5); the cloudflare engine names
    the failure (10..12), held here against the Python oracle's text first."""
    out = np.array(got).copy()
    for i, c in enumerate(got):
        if 10 <= c <= 12:
            assert eng.flavor_name == "cf", i
            text = "bn256: multisig can't unmarshal: " + O.g1_unmarshal(sigs[64 * i:64 * i + 64], "cf")[1]
            assert eng.code_string(int(c)) == text, i
            out[i] = SIG_UNMARSHAL
    return out


class Ctx(NamedTuple):
    eng: object
    N: int
    ks: list
    reg: bytes
    cases: list
    sigs: bytes
    want: np.ndarray
    want_agg: bytes


_ORACLE = {}  # N -> (sigs, codes, aggs): the oracle runs once per registry, both flavors share it


@pytest.fixture(scope="module", params=[(f, n) for f in ("go", "cf") for n in SIZES], ids=lambda p: "%s-%d" % p)
def ctx(request, torch_first, msgs):
    from handel_amd.engine import Engine

    flavor, N = request.param
    eng = Engine(device=0, flavor=flavor)
    ks = F.scalars(N, seed=b"agg-msgs-%d" % N)
    reg = R.g2_scalar_base(F.scalar_bytes(ks))
    assert not eng.registry_load(reg).any()
    cases = _build(N, msgs)
    sigs = _sign(eng, ks, cases)
    if N not in _ORACLE:
        _ORACLE[N] = (sigs,) + _oracle(reg, cases, sigs)
    assert _ORACLE[N][0] == sigs
    _, want, want_agg = _ORACLE[N]
    # on the CPU, before any verdict of the GPU is looked at: the oracle gives
    # every request the code it is in the batch for, and every code occurs
    assert [int(c) for c in want] == [c.expect for c in cases], [(c.what, int(w)) for c, w in zip(cases, want) if w != c.expect]
    assert set(int(c) for c in want) == {HG_OK, SIG_INVALID, HASH_EOF, LEVEL, SIG_UNMARSHAL, EMPTY_AGG}
    assert len(set(int(c) for c in want[:5])) == 4 and len({c.msg for c in cases}) >= 16
    yield Ctx(eng, N, ks, reg, cases, sigs, want, want_agg)
    eng.close()


def _run(c, idx, want_agg=True):
    cases = [c.cases[i] for i in idx]
    sigs = b"".join(c.sigs[64 * i:64 * i + 64] for i in idx)
    reqs, words = _pack(cases)
    got = c.eng.verify_aggregate_msgs([k.msg for k in cases], reqs, words, sigs, want_agg=want_agg)
    codes, agg = got if want_agg else (got, None)
    return _fold_cf(c.eng, codes, sigs), agg


# ---------------------------------------------------------------- 1. the mixed batch
@pytest.mark.parametrize("n", [67, 1, 4, 5])
def test_mixed_batch_matches_oracle_per_request(ctx, n):
    got, agg = _run(ctx, range(n))
    assert np.array_equal(got, ctx.want[:n]), [(k.what, int(g), int(w)) for k, g, w in
                                              zip(ctx.cases, got, ctx.want) if g != w]
    assert agg == ctx.want_agg[:128 * n]
    # the keys do not depend on the message, and without want_agg the codes are the same
    assert np.array_equal(_run(ctx, range(n), want_agg=False)[0], got)


# ---------------------------------------------------------------- 2. permutation
def test_permuted_batch_gives_permuted_codes(ctx):
    perm = np.random.default_rng(11).permutation(len(ctx.cases))
    got, agg = _run(ctx, perm)
    assert np.array_equal(got, ctx.want[perm])
    assert agg == b"".join(ctx.want_agg[128 * i:128 * i + 128] for i in perm)


# ---------------------------------------------------------------- 3. one message for all
@pytest.mark.parametrize("hashes", [True, False], ids=["hashable", "eof"])
def test_one_message_equals_verify_aggregate_msg(ctx, msgs, hashes):
    """Every request on one message: hg_verify_aggregate_msg's codes, with the
    context pinned to level 0 (the same algorithm) and, on the small registry,
    to level 2 (the GT path, the other algorithm)."""
    e = ctx.eng
    msg = next(m for m, h in msgs if h == hashes and len(m) == 65)
    cases = [k._replace(msg=msg, signed=msg if hashes and k.expect != SIG_INVALID else k.signed) for k in ctx.cases]
    sigs = _sign(e, ctx.ks, cases)
    reqs, words = _pack(cases)
    got = e.verify_aggregate_msgs([msg] * len(cases), reqs, words, sigs)
    assert len(set(int(c) for c in got)) == (5 if hashes else 3)  # EOF hides OK, invalid and empty
    try:
        for level in (0, 2) if ctx.N == 67 else (0,):
            e.set_aggregate_level(level)
            want = e.verify_aggregate_msg(msg, reqs, words, sigs)
            assert e.aggregate_tables() == (level if hashes else 0)
            assert np.array_equal(got, want), level
    finally:
        e.set_aggregate_level(-1)


# ---------------------------------------------------------------- 4. the multisig form
def test_multisig_form(ctx, msgs):
    e, N = ctx.eng, ctx.N
    good = [m for m, h in msgs if h]
    eof = [m for m, h in msgs if not h]
    full, part = (True,) * N, tuple(i % 3 != 1 for i in range(N))
    items = [  # (message, bits, signature kind, code)
        (good[0], full, "valid", HG_OK), (good[1], part, "valid", HG_OK), (good[2], full, "tamper", SIG_INVALID),
        (good[3], full[:-1], "valid", MULTI_SIZES), (good[4], full + (True,), "valid", MULTI_SIZES),
        (eof[0], part, "valid", HASH_EOF), (eof[1], full[:-1], "valid", MULTI_SIZES),
        (good[5], part[:-1], "undecodable", SIG_UNMARSHAL), (good[6], (False,) * N, "valid", EMPTY_AGG),
        (good[1], part, "tamper", SIG_INVALID), (good[7], part, "valid", HG_OK),
    ]
    cases = [Case("multisig", m, 0, N, b, s, m if M.hashable(m) else good[0], x) for m, b, s, x in items]
    sigs = _sign(e, ctx.ks, cases)
    want, _ = _oracle(ctx.reg, cases, sigs)
    want[want == LEVEL] = MULTI_SIZES
    assert [int(c) for c in want] == [x for _, _, _, x in items]
    reqs, words = _pack(cases)
    got = e.verify_multisig_msgs([k.msg for k in cases], reqs["bitlen"], reqs["word_offset"], words, sigs)
    assert np.array_equal(_fold_cf(e, got, sigs), want)
    # the plugin mirror: the reference's texts per entry, whatever the
    # verifier's own message is (here one that cannot be hashed)
    from handel_amd.processing import BatchVerifier

    bv = BatchVerifier(e, ctx.reg, F.REJECT_MESSAGES[0])
    texts = bv.verify_multisignatures_msgs([(k.msg, list(k.bits), sigs[64 * i:64 * i + 64]) for i, k in enumerate(cases)])
    assert texts == [None if c == HG_OK else e.code_string(int(c)) for c in got]
    assert texts[3] == "verify multisignature: inconsistent sizes" and texts[5] == "EOF"


# ---------------------------------------------------------------- 5. a key outside G2
def test_non_g2_registry_keeps_reference_verdicts(msgs):
    """A go-flavor registry with keys 10, 11, 12 = A, B, -(A + B) outside G2
    (tests/test_gpu_gt_scope.py): this call is the point path, whose verdicts
    are the reference algorithm's (fast=False) for such keys."""
    from handel_amd.engine import Engine

    good = [m for m, h in msgs if h]
    ks = F.scalars(64, seed=b"non-g2")
    pts = [O.g2_mul(O.G2_GEN, k) for k in ks]
    a, b = F.non_g2_points(2, seed=3)
    pts[10], pts[11], pts[12] = a, b, O.g2_neg(O.g2_add(a, b))
    for i in (10, 11, 12):
        ks[i] = None
    reg = b"".join(O.g2_marshal(p) for p in pts)
    bits = lambda off, size, idx: tuple(off + i in idx for i in range(size))  # noqa: E731
    cases = [
        Case("A + B + C = inf, sig inf", good[0], 8, 8, bits(8, 8, (10, 11, 12)), "valid", good[0], HG_OK),
        Case("... any other sig", good[1], 8, 8, bits(8, 8, (10, 11, 12)), "tamper", good[1], SIG_INVALID),
        Case("honest sum + (A + B + C)", good[2], 0, 64, (True,) * 64, "valid", good[2], HG_OK),
        Case("inside a level block", good[3], 8, 8, bits(8, 8, (8, 9, 10, 11, 12, 13)), "valid", good[3], HG_OK),
        Case("A alone, sig inf", good[4], 8, 8, bits(8, 8, (10,)), "valid", good[4], SIG_INVALID),
        Case("honest keys only", good[5], 0, 8, bits(0, 8, (0, 3, 5)), "valid", good[5], HG_OK),
        Case("honest, another message", good[6], 32, 32, (True,) * 32, "valid", good[5], SIG_INVALID),
    ]
    e = Engine(device=0, flavor="go")
    try:
        assert list(e.registry_load(reg)) == [0] * 64
        assert e.registry_non_g2() == 3
        sigs = _sign(e, ks, cases)
        want, want_agg = _oracle(reg, cases, sigs, fast=False)
        assert [int(c) for c in want] == [c.expect for c in cases]
        reqs, words = _pack(cases)
        got, agg = e.verify_aggregate_msgs([c.msg for c in cases], reqs, words, sigs, want_agg=True)
        assert list(got) == list(want)
        assert agg == want_agg and agg[:128] == bytes(128)
    finally:
        e.close()


# ---------------------------------------------------------------- 6. the device variant
def test_device_variant_on_a_stream_and_range_errors(ctx):
    import torch

    from handel_amd._lib import HandelGPUError

    e, n = ctx.eng, 21
    cases, sigs = ctx.cases[:n], ctx.sigs[:64 * n]
    dev = torch.device("cuda:0")
    pool, off, ln = e.pack_messages([k.msg for k in cases])
    reqs, words = _pack(cases)
    want, want_agg = e.verify_aggregate_msgs_pool(pool, off, ln, reqs, words, sigs, want_agg=True)
    assert np.array_equal(_fold_cf(e, want, sigs), ctx.want[:n])

    def run(off, ln):
        t = lambda a, dt: torch.frombuffer(bytearray(a), dtype=dt).to(dev)  # noqa: E731
        d_pool, d_sigs, d_reqs = t(pool.tobytes(), torch.uint8), t(sigs, torch.uint8), t(reqs.tobytes(), torch.uint8)
        d_words = t(words.tobytes(), torch.uint8)
        d_off, d_len = t(off.tobytes(), torch.int32), t(ln.tobytes(), torch.int32)
        d_codes = torch.full((n,), -1, dtype=torch.int32, device=dev)
        d_agg = torch.full((128 * n,), 0xEE, dtype=torch.uint8, device=dev)
        s = torch.cuda.Stream(dev)
        torch.cuda.synchronize()
        e.verify_aggregate_msgs_device(d_pool.data_ptr(), len(pool), d_off.data_ptr(), d_len.data_ptr(),
                                       d_reqs.data_ptr(), n, d_words.data_ptr(), d_sigs.data_ptr(), d_codes.data_ptr(),
                                       d_agg.data_ptr(), s.cuda_stream)
        s.synchronize()
        return d_codes.cpu().numpy(), d_agg.cpu().numpy().tobytes()

    got, agg = run(off, ln)
    assert np.array_equal(got, want) and agg == want_agg
    # a valid request (0), an undecodable signature (10), a level error (11) and
    # an empty bitset (13) with their message ranges past the pool: HG_ERR_ARG
    # stands where the hash code stands, for those requests alone
    assert [int(want[i]) for i in (0, 11, 13)] == [HG_OK, LEVEL, EMPTY_AGG] and ctx.want[10] == SIG_UNMARSHAL
    bad_off, bad_len = off.copy(), ln.copy()
    bad_len[0] = len(pool) - off[0] + 1
    bad_off[10], bad_len[10] = 0xFFFFFFF0, 0x20
    bad_len[11] = len(pool) + 1
    bad_off[13] = len(pool)
    assert bad_len[13] > 0
    expect = want.copy()
    expect[0] = expect[13] = HG_ERR_ARG
    got, agg = run(bad_off, bad_len)
    assert np.array_equal(got, expect) and agg == want_agg
    # the host variant refuses such input as a whole and names the request
    with pytest.raises(HandelGPUError, match="code 100.*message 0"):
        e.verify_aggregate_msgs_pool(pool, bad_off, bad_len, reqs, words, sigs)
    short = reqs.copy()
    short["word_offset"][3] = len(words)
    with pytest.raises(HandelGPUError, match="code 100.*request 3"):
        e.verify_aggregate_msgs_pool(pool, off, ln, short, words, sigs)
    assert len(e.verify_aggregate_msgs([], reqs[:0], words, b"")) == 0


# ---------------------------------------------------------------- 7. the hash beside the fold, or before it
def test_overlap_on_and_off_give_the_same_codes(ctx):
    try:
        ctx.eng.set_fold_overlap(False)
        off, off_agg = _run(ctx, range(67))
        ctx.eng.set_fold_overlap(True)
        on, on_agg = _run(ctx, range(67))
    finally:
        ctx.eng.set_fold_overlap(True)
    assert np.array_equal(off, ctx.want) and np.array_equal(on, ctx.want)
    assert off_agg == on_agg == ctx.want_agg


# ---------------------------------------------------------------- 8. the context is untouched
def test_context_state_is_untouched(msgs):
    """A context with a message and level-2 torus tables on a 64-key registry
    gives the same answers, at the same level, after calls on other messages."""
    from handel_amd.engine import REQ_DTYPE, Engine

    e = Engine(device=0, flavor="go")
    try:
        msg = F.LIB_MESSAGE
        ks, reg, _ = F.keys_and_sigs(64, msg=msg, seed=b"aggmsgs-ctx")
        assert not e.registry_load(reg).any()
        assert e.set_message(msg) == 0
        e.set_aggregate_level(2)
        assert e.prepare_aggregate() == 0
        agg = R.sign(msg, (sum(ks[i] for i in (0, 2, 5, 33)) % O.ORDER).to_bytes(32, "big"))
        reqs = np.array([(0, 64, 64, 0), (0, 64, 64, 1), (0, 64, 64, 2)], dtype=REQ_DTYPE)
        words = np.array([0b100101 | 1 << 33, 0b100111 | 1 << 33, 0], dtype=np.uint64)

        def state():
            return (e.aggregate_tables(), e.aggregate_tables_torus(), list(e.verify_aggregate(reqs, words, agg * 3)))

        before = state()
        assert before[0] == 2 and before[2] == [0, 1, 6]
        others = [m for m, h in msgs if h][:2] + [F.REJECT_MESSAGES[0]]
        assert not M.hashable(others[2])
        cases = [Case("other", m, 0, 64, tuple(i in (0, 2, 5, 33) for i in range(64)), "valid",
                      m if M.hashable(m) else others[0], 0) for m in others]
        got = e.verify_aggregate_msgs(others, reqs, np.array([words[0]] * 3, dtype=np.uint64), _sign(e, ks, cases))
        assert list(got) == [HG_OK, HG_OK, HASH_EOF]
        # the context's own message, given per request, gives its own verdicts
        assert list(e.verify_aggregate_msgs([msg] * 3, reqs, words, agg * 3)) == before[2]
        assert state() == before
    finally:
        e.close()
