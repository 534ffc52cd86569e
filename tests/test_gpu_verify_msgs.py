"""GPU parity of the batches whose checks each carry their own message
(hg_verify_batch_msgs, hg_verify_batch_msgs_device, hg_hash_messages,
hg_debug_g1_base_mul) against the CPU oracles: the fixed-base
k * G1 against the Python oracle, hashedMessage x n and the per-check verdicts
against the C oracle called once per check with that check's message. Byte and
code comparisons: the bar is exact equality."""

import numpy as np
import pytest

from oracle import bn256_oracle as O
from oracle import ref_lib as R
from tests import _fixtures as F
from tests import _msgs_fixtures as M

pytestmark = pytest.mark.gpu

HG_OK, HG_ERR_SIG_INVALID, HG_ERR_HASH_EOF, HG_ERR_ARG = 0, 1, 2, 100
G1_BYTES = O.g1_marshal(O.G1_GEN)
FLAVOR_ID = {"go": 0, "cf": 1}


@pytest.fixture(scope="module", autouse=True)
def torch_first():
    """torch's HIP runtime before the engine's (as tests/conftest.py does for
    the session engines): the device variant's test moves tensors to the GPU
    whichever test ran first."""
    import torch

    if torch.cuda.is_available():
        torch.cuda.set_device(0)
        torch.zeros(1, device="cuda")


@pytest.fixture(scope="module", params=["go", "cf"])
def eng(request, torch_first):
    """A context of its own per flavor: the tests switch its form
    (hg_set_verify_split)."""
    from handel_amd.engine import Engine

    e = Engine(device=0, flavor=request.param)
    yield e
    e.close()


@pytest.fixture(scope="module")
def msgs():
    out = M.boundary_set()
    M.check_boundary_set(out)
    return out


# ---------------------------------------------------------------- 1. k * G1 from the table
def _base_mul_scalars():
    fixed = [1, 15, 16, 1 << 252, O.ORDER - 1,
             sum(((l % 15) + 1) << (4 * (4 * l + l % 4)) for l in range(16)),  # one nonzero nibble per lane
             0xFFFF << (16 * 5)]                                                # all in lane 5's windows
    digests = [M.digest_int(b"base-mul:%d" % i) for i in range(200)]
    return fixed, digests


@pytest.fixture(scope="module")
def base_mul_case():
    fixed, digests = _base_mul_scalars()
    ks = fixed + digests
    # the digests alone reach every (window, digit) entry of the table
    seen = {(j, (k >> (4 * j)) & 15) for k in digests for j in range(64)}
    assert {(j, d) for j in range(64) for d in range(1, 16)} <= seen
    want = [O.g1_marshal(O.g1_mul(O.G1_GEN, k)) for k in ks]
    return ks, want


def test_lazy_table_counts_in_context_bytes():
    """The G1 base table is built by the first multi-message call, not by
    hg_create: the context's bytes grow by at least the table then."""
    from handel_amd.engine import Engine

    e = Engine(device=0, flavor="go")
    try:
        before = e.context_bytes()
        assert e.debug_g1_base_mul([1]) == G1_BYTES
        assert e.context_bytes() - before >= 960 * 96
    finally:
        e.close()


@pytest.mark.parametrize("n", [1, 5, None], ids=["n1", "n5_ragged_wave", "all"])
def test_g1_base_mul_matches_oracle(eng, base_mul_case, n):
    ks, want = base_mul_case
    # n = 5 takes scalars of every kind: small, top window, one nibble per lane, one lane, a digest
    pick = {1: [4], 5: [0, 3, 5, 6, 7], None: range(len(ks))}[n]
    got = eng.debug_g1_base_mul([ks[i] for i in pick])
    for j, i in enumerate(pick):
        assert got[64 * j:64 * j + 64] == want[i], hex(ks[i])


def test_g1_base_mul_multiples_of_order_are_infinity(eng):
    got = eng.debug_g1_base_mul([0, O.ORDER, O.ORDER + 1])
    assert got[:128] == bytes(128)
    assert got[128:] == G1_BYTES


# ---------------------------------------------------------------- 2. hashedMessage x n
def test_hash_messages_on_boundary_set(eng, msgs):
    """Every boundary message at an odd pool offset, one of them twice."""
    order = [m for m, _ in msgs] + [msgs[2][0]]
    pool, off, ln = b"", [], []
    for m in order:
        pool += b"\xa5" * (1 if len(pool) % 2 == 0 else 2)  # the next offset is odd
        off.append(len(pool))
        ln.append(len(m))
        pool += m
    assert all(o % 2 == 1 for o in off)
    out, codes = eng.hash_messages_pool(np.frombuffer(pool, dtype=np.uint8), off, ln)
    one = (1).to_bytes(32, "big")
    for i, m in enumerate(order):
        h = out[64 * i:64 * i + 64]
        if O.hash_scalar(m)[1] is None:
            assert codes[i] == HG_OK and h == R.sign(m, one), (i, len(m))
        else:
            assert codes[i] == HG_ERR_HASH_EOF and h == G1_BYTES, (i, len(m))
    assert out[64 * 2:64 * 3] == out[-64:]
    # the packing wrapper gives the same
    out2, codes2 = eng.hash_messages(order)
    assert out2 == out and np.array_equal(codes2, codes)


# ---------------------------------------------------------------- 3. the mixed batch
OFF_CURVE_G1 = (1).to_bytes(32, "big") + (1).to_bytes(32, "big")
OFF_CURVE_G2 = bytes(127) + b"\x01"
# the generator with x + p: x/crypto reduces it, cloudflare refuses it
EXCEEDS_G1 = (O.P + 1).to_bytes(32, "big") + (O.P - 2).to_bytes(32, "big")


def _oracle_code(m, p, s, flavor, hashable_msg):
    """The C oracle's code of one check on its own message, in the reference's
    order. ref_verify_batch hashes once per call, BEFORE it decodes, so for an
    EOF message it answers EOF (2) whatever the key and the signature are; the
    reference unmarshals both before VerifySignature is ever called (DESIGN §1,
    and hg_verify_batch_msg answers that way: 4 / 5 for an undecodable pk / sig
    on an EOF message, where the one-call oracle says 2). So for an EOF message
    the oracle's own decode of this pk and sig is asked for as well, on a
    message it can hash: an unmarshal code there comes first."""
    c = R.verify_batch(m, p, s, flavor=flavor)[0]
    if c == HG_ERR_HASH_EOF:
        d = R.verify_batch(hashable_msg, p, s, flavor=flavor)[0]
        if d not in (HG_OK, HG_ERR_SIG_INVALID):
            c = d
    return c


def _mixed_batch(msgs, flavor, n=67):
    """n checks (msg, pk, sig) over 12 distinct messages, the first five of
    every kind, and the C oracle's code of each on its own message."""
    good = [m for m, h in msgs if h][:9]
    eof = [m for m, h in msgs if not h][:2] + [b""]
    ks = F.scalars(n, seed=b"msgs-batch")
    pks = R.g2_scalar_base(F.scalar_bytes(ks))
    pk = lambda i: pks[128 * i:128 * i + 128]  # noqa: E731
    sig = lambda i, m: R.sign(m, ks[i].to_bytes(32, "big"))  # noqa: E731
    z128, z64 = bytes(128), bytes(64)
    cases = [
        (good[0], pk(0), sig(0, good[0])),            # valid
        (eof[0], pk(1), sig(1, good[0])),             # EOF message, well-formed signature
        (good[1], pk(2), sig(2, good[2])),            # valid for ANOTHER message of the batch
        (good[2], pk(3), sig(3, good[2])),            # valid, on that other message
        (good[3], pk(5), sig(4, good[3])),            # wrong key
        (good[4], OFF_CURVE_G2, sig(5, good[4])),     # undecodable pk, hashable message
        (eof[1], OFF_CURVE_G2, sig(6, good[4])),      # undecodable pk, EOF message
        (good[5], pk(7), OFF_CURVE_G1),               # undecodable sig, hashable message
        (eof[2], pk(8), OFF_CURVE_G1),                # undecodable sig, EOF (empty) message
        (good[6], OFF_CURVE_G2, OFF_CURVE_G1),        # both: the pk's error
        (good[7], z128, z64),                         # pk and sig at infinity
        (eof[0], z128, z64),                          # the same on an EOF message
        (good[8], pk(12), z64),                       # sig at infinity alone
        (good[0], pk(13), EXCEEDS_G1),                # decode rules differ by flavor
        (eof[1], pk(14), EXCEEDS_G1),
    ]
    for i in range(len(cases), n):                    # valid signatures, messages repeating
        m = good[i % len(good)]
        cases.append((m, pk(i), sig(i, m)))
    assert len({m for m, _, _ in cases}) == 12
    want = np.array([_oracle_code(m, p, s, FLAVOR_ID[flavor], good[0]) for m, p, s in cases], dtype=np.int32)
    return cases, want


@pytest.fixture(scope="module")
def mixed(eng, msgs):
    cases, want = _mixed_batch(msgs, eng.flavor_name)
    # the oracle's codes cover what the batch is meant to mix
    assert want[0] == HG_OK and want[1] == HG_ERR_HASH_EOF and want[2] == HG_ERR_SIG_INVALID
    assert want[4] == HG_ERR_SIG_INVALID and want[10] == HG_OK and want[11] == HG_ERR_HASH_EOF
    assert want[5] == want[6] == want[9] and want[5] not in (HG_OK, HG_ERR_SIG_INVALID, HG_ERR_HASH_EOF)
    assert want[7] == want[8] and want[7] not in (HG_OK, HG_ERR_SIG_INVALID, HG_ERR_HASH_EOF, want[5])
    assert (want[15:] == HG_OK).all()
    return cases, want


def _run(e, cases):
    """The engine's codes in the C oracle's terms. The oracle knows one code
    per unmarshal failure (4: pk, 5: sig) in both flavors; the engine's
    cloudflare codes name the failure (7..9: pk, 10..12: sig), so those are
    first held against the Python oracle's cloudflare error text, then folded."""
    got = e.verify_batch_msgs([m for m, _, _ in cases], b"".join(p for _, p, _ in cases),
                              b"".join(s for _, _, s in cases))
    out = got.copy()
    for i, (_, p, s) in enumerate(cases):
        if 7 <= got[i] <= 9:
            assert e.flavor_name == "cf" and e.code_string(int(got[i])) == O.g2_unmarshal(p, "cf")[1], i
            out[i] = 4
        elif 10 <= got[i] <= 12:
            assert e.flavor_name == "cf" and O.g2_unmarshal(p, "cf")[1] is None, i
            assert e.code_string(int(got[i])) == "bn256: multisig can't unmarshal: " + O.g1_unmarshal(s, "cf")[1], i
            out[i] = 5
    return out


@pytest.mark.parametrize("split", [False, True], ids=["one_kernel", "split"])
@pytest.mark.parametrize("n", [67, 1, 4, 5])
def test_mixed_batch_matches_oracle_per_check(eng, mixed, split, n):
    cases, want = mixed
    eng.set_verify_split(split)
    try:
        got = _run(eng, cases[:n])
    finally:
        eng.set_verify_split(False)
    assert np.array_equal(got, want[:n]), (list(got), list(want[:n]))


@pytest.mark.parametrize("split", [False, True], ids=["one_kernel", "split"])
def test_permuted_batch_gives_permuted_codes(eng, mixed, split):
    cases, want = mixed
    perm = np.random.default_rng(5).permutation(len(cases))
    eng.set_verify_split(split)
    try:
        got = _run(eng, [cases[i] for i in perm])
    finally:
        eng.set_verify_split(False)
    assert np.array_equal(got, want[perm])


# ---------------------------------------------------------------- 4. one message for all
@pytest.mark.parametrize("hashes", [True, False], ids=["hashable", "eof"])
def test_one_message_equals_verify_batch_msg(eng, msgs, hashes):
    msg = next(m for m, h in msgs if h == hashes and len(m) == 65)
    signed = msg if hashes else F.LIB_MESSAGE
    _, pks, sigs = F.keys_and_sigs(9, msg=signed, seed=b"msgs-one")
    sigs = F.tamper(sigs, every=4)
    pks = pks[:128] + OFF_CURVE_G2 + pks[256:]
    want = eng.verify_batch_msg(msg, pks, sigs)
    got = eng.verify_batch_msgs([msg] * 9, pks, sigs)
    assert np.array_equal(got, want)
    assert len(set(want)) == (3 if hashes else 2)


# ---------------------------------------------------------------- 5. the device variant
def test_device_variant_on_a_stream_and_range_errors(eng, mixed):
    import torch

    from handel_amd._lib import HandelGPUError

    cases, want = mixed
    cases, want = cases[:21], want[:21].copy()
    n = len(cases)
    dev = torch.device("cuda:0")
    pool, off, ln = eng.pack_messages([m for m, _, _ in cases])
    pks = b"".join(p for _, p, _ in cases)
    sigs = b"".join(s for _, _, s in cases)
    assert np.array_equal(_run(eng, cases), want)
    want = eng.verify_batch_msgs_pool(pool, off, ln, pks, sigs)  # the host variant, in the engine's own codes

    def run(off, ln):
        t = lambda a, dt: torch.frombuffer(bytearray(a), dtype=dt).to(dev)  # noqa: E731
        d_pool, d_pks, d_sigs = t(pool.tobytes(), torch.uint8), t(pks, torch.uint8), t(sigs, torch.uint8)
        d_off, d_len = t(off.tobytes(), torch.int32), t(ln.tobytes(), torch.int32)
        d_codes = torch.full((n,), -1, dtype=torch.int32, device=dev)
        s = torch.cuda.Stream(dev)
        torch.cuda.synchronize()
        eng.verify_batch_msgs_device(d_pool.data_ptr(), len(pool), d_off.data_ptr(), d_len.data_ptr(),
                                     d_pks.data_ptr(), d_sigs.data_ptr(), n, d_codes.data_ptr(), s.cuda_stream)
        s.synchronize()
        return d_codes.cpu().numpy()

    assert np.array_equal(run(off, ln), want)
    # check 3 (valid) and check 0's neighbour ranges: one byte past the pool, and an offset near 2^32
    bad_off, bad_len = off.copy(), ln.copy()
    bad_len[3] = len(pool) - off[3] + 1
    bad_off[16], bad_len[16] = 0xFFFFFFF0, 0x20
    assert want[3] == HG_OK and want[16] == HG_OK
    expect = want.copy()
    expect[3] = expect[16] = HG_ERR_ARG
    assert np.array_equal(run(bad_off, bad_len), expect)
    # an unmarshal error still comes first
    bad_len2 = ln.copy()
    bad_len2[5] = len(pool) + 1
    assert np.array_equal(run(off, bad_len2), want)
    # the host variant refuses the same input as a whole
    with pytest.raises(HandelGPUError, match="code 100.*message 3"):
        eng.verify_batch_msgs_pool(pool, bad_off, bad_len, pks, sigs)
    with pytest.raises(HandelGPUError, match="code 100"):
        eng.hash_messages_pool(pool, bad_off, bad_len)


# ---------------------------------------------------------------- 6. the context is untouched
def test_context_state_is_untouched(msgs):
    """A context with a message, level-1 tables on a 64-key registry and work
    done gives the same answers after multi-message calls on other messages."""
    from handel_amd.engine import REQ_DTYPE, Engine

    e = Engine(device=0, flavor="go")
    try:
        msg = F.LIB_MESSAGE
        ks, reg, sigs = F.keys_and_sigs(64, msg=msg, seed=b"msgs-ctx")
        assert not e.registry_load(reg).any()
        assert e.set_message(msg) == 0
        e.set_aggregate_level(1)
        assert e.prepare_aggregate() == 0
        assert e.aggregate_tables() == 1
        agg = R.sign(msg, (sum(ks[i] for i in (0, 2, 5, 33)) % O.ORDER).to_bytes(32, "big"))
        reqs = np.array([(0, 64, 64, 0), (0, 64, 64, 1), (0, 64, 64, 2)], dtype=REQ_DTYPE)
        words = np.array([0b100101 | 1 << 33, 0b100111 | 1 << 33, 0], dtype=np.uint64)
        batch_sigs = F.tamper(sigs[:64 * 16], every=5)

        def state():
            return (e.aggregate_tables(), list(e.verify_batch(reg[:128 * 16], batch_sigs)),
                    list(e.verify_aggregate(reqs, words, agg * 3)))

        before = state()
        assert before[1].count(1) == 4 and before[2] == [0, 1, 6]
        # messages the context never saw, three hashable and one EOF, in both forms
        others = [m for m, h in msgs if h][:3] + [F.REJECT_MESSAGES[0]]
        own = b"".join(R.sign(m, ks[i].to_bytes(32, "big")) for i, m in enumerate(others[:3]))
        for split in (False, True):
            e.set_verify_split(split)
            got = e.verify_batch_msgs(others + [msg], reg[:128 * 5], own + sigs[64 * 3:64 * 5])
            assert list(got) == [0, 0, 0, HG_ERR_HASH_EOF, 0]
        e.set_verify_split(False)
        assert state() == before
    finally:
        e.close()
