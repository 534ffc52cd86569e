"""GPU test that the host-pointer entry families of an aggregate batch agree:
hg_verify_aggregate (G2 fold and GT path), hg_verify_aggregate_rlc,
hg_verify_aggregate_msgs and hg_aggregate_pk stage one batch through the same
helper (HostStage, handel_amd/csrc/hg_aggregate.h) and check its requests by
the same rule (hg_requests.h). One batch of seven requests over a 24-key
registry (one 16-key block level) and one message; codes and aggregate-key
marshals against the C oracle, the bar exact equality. Then the batch with its
bitset one word short: every family refuses it as a whole, names the request,
and leaves the context fit for the next call. Last, the two multisignature
entry points on the three inputs where their renames of the size error show."""

import numpy as np
import pytest

from oracle import bn256_oracle as O
from oracle import ref_lib as R
from tests import _fixtures as F

pytestmark = pytest.mark.gpu

HG_OK, SIG_INVALID, LEVEL, SIG_UNMARSHAL, EMPTY_AGG, MULTI_SIZES = 0, 1, 3, 5, 6, 13
OFF_CURVE_G1 = (1).to_bytes(32, "big") + (1).to_bytes(32, "big")
N = 24
MSG = F.LIB_MESSAGE
SEED = bytes(range(32))
PARTIAL = [True, False, True, True, False, False, True, False]
# (offset, level_size, bits, signature kind, the code the request is in the batch for)
BATCH = [
    (0, 16, [True] * 16, "valid", HG_OK),
    (16, 8, PARTIAL, "valid", HG_OK),
    (0, 16, [True] * 15, "valid", LEVEL),           # bitlen != level_size
    (17, 8, [True] * 8, "valid", LEVEL),            # offset + bitlen = 25
    (8, 8, [False] * 8, "valid", EMPTY_AGG),
    (0, 8, [i % 3 != 0 for i in range(8)], "tamper", SIG_INVALID),
    (16, 8, PARTIAL, "undecodable", SIG_UNMARSHAL),
]
NO_KEY = (2, 3, 4)  # the requests without an aggregate key: level errors and the empty bitset


def _sign(ks, off, bits, kind, msg=MSG):
    if kind == "undecodable":
        return OFF_CURVE_G1
    sk = sum(ks[off + i] for i, b in enumerate(bits) if b and off + i < len(ks)) % O.ORDER
    sig = R.sign(msg, sk.to_bytes(32, "big"))
    return R.g1_add(sig, O.g1_marshal(O.G1_GEN)) if kind == "tamper" else sig


class Fix:
    pass


@pytest.fixture(scope="module")
def fx():
    import torch

    from handel_amd.engine import REQ_DTYPE, Engine

    if torch.cuda.is_available():  # torch's HIP runtime before the engine's, as tests/conftest.py does
        torch.cuda.set_device(0)
        torch.zeros(1, device="cuda")
    f = Fix()
    f.ks, f.reg, _ = F.keys_and_sigs(N, msg=MSG, seed=b"host-staging")
    f.sigs = b"".join(_sign(f.ks, off, bits, kind) for off, _, bits, kind, _ in BATCH)
    reqs, words = F.pack_requests([(off, size) for off, size, _, _, _ in BATCH], [bits for _, _, bits, _, _ in BATCH])
    assert len(words) == len(BATCH)  # one word each
    # request 2's word goes last, so a bitset one word short cuts off that request alone
    reqs = [list(r) for r in reqs]
    order = [0] + list(range(2, len(BATCH))) + [1]
    for pos, i in enumerate(order):
        reqs[i][3] = pos
    f.reqs = np.array([tuple(r) for r in reqs], dtype=REQ_DTYPE)
    f.words = np.array([words[i] for i in order], dtype=np.uint64)
    assert int(f.reqs["word_offset"][1]) == len(f.words) - 1
    # the oracle, one call per request (as tests/test_gpu_aggregate_msgs.py builds its `want`)
    codes, aggs = [], []
    for i, (off, size, bits, _, _) in enumerate(BATCH):
        w = np.array(O.bitset_words(bits), dtype=np.uint64)
        code, agg = R.verify_aggregate(MSG, f.reg, [off], [len(bits)], [size], w, [0], f.sigs[64 * i:64 * i + 64],
                                       want_agg=True)
        codes.append(int(code[0]))
        aggs.append(agg)
    f.want, f.want_agg = np.array(codes, dtype=np.int32), b"".join(aggs)
    assert codes == [x for _, _, _, _, x in BATCH]
    for i in range(len(BATCH)):
        assert (f.want_agg[128 * i:128 * i + 128] == bytes(128)) == (i in NO_KEY), i
    f.eng = Engine(device=0, flavor="go")
    assert not f.eng.registry_load(f.reg).any()
    assert f.eng.set_message(MSG) == 0
    yield f
    f.eng.close()


def _families(f, reqs, words):
    """Every host-pointer family on one batch: (name, thunk giving codes)."""
    e = f.eng

    def at(level, fn):
        def run():
            e.set_aggregate_level(level)
            try:
                return fn()
            finally:
                e.set_aggregate_level(-1)
        return run

    return [
        ("hg_verify_aggregate, level 0", at(0, lambda: e.verify_aggregate(reqs, words, f.sigs))),
        ("hg_verify_aggregate, level 2", at(2, lambda: e.verify_aggregate(reqs, words, f.sigs))),
        ("hg_verify_aggregate_rlc, groups of 2", at(2, lambda: e.verify_aggregate_rlc(reqs, words, f.sigs, SEED, 2))),
        ("hg_verify_aggregate_rlc, groups of 7", at(2, lambda: e.verify_aggregate_rlc(reqs, words, f.sigs, SEED, 7))),
        ("hg_verify_aggregate_msgs", lambda: e.verify_aggregate_msgs([MSG] * len(reqs), reqs, words, f.sigs)),
    ]


def test_every_family_returns_the_oracle_codes(fx):
    for name, run in _families(fx, fx.reqs, fx.words):
        got = run()
        assert np.array_equal(got, fx.want), (name, list(got), list(fx.want))
        if "level 2" in name:
            assert fx.eng.aggregate_tables() == 2, name  # the GT path ran
        if "rlc" in name:
            assert fx.eng.aggregate_tables() == 2 and fx.eng.rlc_stats()[0] > 0, name  # the combination ran


def test_aggregate_keys_agree_and_are_zero_without_a_key(fx):
    e = fx.eng
    keys = {}
    for level in (0, 2):
        e.set_aggregate_level(level)
        try:
            codes, keys[level] = e.verify_aggregate(fx.reqs, fx.words, fx.sigs, want_agg=True)
        finally:
            e.set_aggregate_level(-1)
        assert np.array_equal(codes, fx.want), level
    pk, pk_codes = e.aggregate_pk(fx.reqs, fx.words)
    mcodes, mkeys = e.verify_aggregate_msgs([MSG] * len(BATCH), fx.reqs, fx.words, fx.sigs, want_agg=True)
    assert np.array_equal(mcodes, fx.want)
    assert keys[0] == keys[2] == pk == mkeys == fx.want_agg
    assert list(pk_codes) == [HG_OK, HG_OK, LEVEL, LEVEL, EMPTY_AGG, HG_OK, HG_OK]
    for i in NO_KEY:
        assert pk[128 * i:128 * i + 128] == bytes(128), i
    assert all(pk[128 * i:128 * i + 128] != bytes(128) for i in range(len(BATCH)) if i not in NO_KEY)


def test_a_bitset_one_word_short_is_refused_whole_and_leaves_nothing_behind(fx):
    from handel_amd._lib import HandelGPUError

    e = fx.eng
    short = fx.words[:-1]  # one word short of what request 2 (index 1) needs
    runs = _families(fx, fx.reqs, short) + [("hg_aggregate_pk", lambda: e.aggregate_pk(fx.reqs, short))]
    for (name, bad), (_, good) in zip(runs, _families(fx, fx.reqs, fx.words) + [(None, None)]):
        with pytest.raises(HandelGPUError, match=r"code 100: hg_\w+: request 1 \(word offset 6, 8 bits\).* 6 bitset words"):
            bad()
        # the next valid call on the same context
        if good is not None:
            assert np.array_equal(good(), fx.want), name
        else:
            pk, pk_codes = e.aggregate_pk(fx.reqs, fx.words)
            assert pk == fx.want_agg and pk_codes[4] == EMPTY_AGG, name
    # the level errors' words are not held to the bitset: request 4's word offset outside it changes nothing
    far = fx.reqs.copy()
    far["word_offset"][3] = len(fx.words) + 5
    assert np.array_equal(e.verify_aggregate(far, fx.words, fx.sigs), fx.want)
    assert np.array_equal(e.verify_aggregate_msgs([MSG] * len(far), far, fx.words, fx.sigs), fx.want)


def test_multisignature_entry_points_keep_their_renames(fx):
    """Full size and valid; one bit short; one bit short with a signature that
    does not unmarshal. The codes are the parent commit's, recorded by running
    this body there. The last case is where the two entry points differ:
    hg_verify_multisig gives every multisignature of the wrong size
    HG_ERR_MULTI_SIZES, hg_verify_multisig_msgs renames the level error only,
    so the signature's own error stands."""
    e = fx.eng
    items = [([True] * N, "valid"), ([True] * (N - 1), "valid"), ([True] * (N - 1), "undecodable")]
    sigs = b"".join(_sign(fx.ks, 0, bits, kind) for bits, kind in items)
    reqs, words = F.pack_requests([(0, N)] * 3, [bits for bits, _ in items])
    bitlens, offs = [r[1] for r in reqs], [r[3] for r in reqs]
    assert list(e.verify_multisig(bitlens, offs, words, sigs)) == [HG_OK, MULTI_SIZES, MULTI_SIZES]
    assert list(e.verify_multisig_msgs([MSG] * 3, bitlens, offs, words, sigs)) == [HG_OK, MULTI_SIZES, SIG_UNMARSHAL]
