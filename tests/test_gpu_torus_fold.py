"""GPU suite: the GT fold over tables in torus form (handel_amd/csrc:
bn256_gttab.hip k_tor_scan, k_tor_convert; bn256_gt.hip k_tor_chunks,
k_tor_compare_bits; hg_aggregate.cpp).

At table level 2 the 16-key window table and the block table keep each entry
g = a + b w as alpha = (1 + a)/b, and the fold multiplies a running X (value
X/conj(X)) by alpha + w. Every verdict here is compared with the C
restatement of the reference (oracle.ref_lib.verify_aggregate), under both
flavors, with one aggregate in four tampered, on the smallest registries that
reach each path of the new kernels: 33 keys (a ragged last window), 64 keys
(four windows, an aligned block to complement), 160 keys (chunks of exactly
eight and of nine terms, and one wave of chunk lengths 1, 2, 3, 7, 8 for the
padding restore). Registries in which a window subset or a block of keys sums
to zero have an entry without a torus form: their set must stay as it was and
still give the oracle's verdicts.
"""

import numpy as np
import pytest

from handel_amd import _lib
from handel_amd.engine import REQ_DTYPE, DeviceLane, Engine
from oracle import bn256_oracle as O
from oracle import ref_lib as R
from tests import _fixtures as F

pytestmark = pytest.mark.gpu

MSG = F.LIB_MESSAGE
CF_CODES = {O.ERR_CF_EXCEEDS: _lib.HG_ERR_SIG_CF_EXCEEDS, O.ERR_CF_MALFORMED: _lib.HG_ERR_SIG_CF_MALFORMED,
            O.ERR_CF_NOT_ENOUGH: _lib.HG_ERR_SIG_CF_SHORT}
OFF_CURVE = (1).to_bytes(32, "big") * 2  # (1, 1): 1 != 1 + 3
INFINITY = bytes(64)


def _sign(msg, ks, ranges, bitsets):
    """The aggregate signature of every request's set keys (an empty set: any signature)."""
    scal = b""
    for (off, _), bits in zip(ranges, bitsets):
        k = sum(ks[off + i] for i, b in enumerate(bits) if b) % O.ORDER
        scal += (k or 1).to_bytes(32, "big")
    return R.sign(msg, scal)


def _batch(msg, ks, ranges, bitsets, special=()):
    """reqs, words, sigs: one signature in four tampered, then the special
    signatures ((index, 64 bytes)) put in."""
    sigs = bytearray(F.tamper(_sign(msg, ks, ranges, bitsets), every=4))
    for i, s in special:
        sigs[64 * i:64 * i + 64] = s
    reqs, words = F.pack_requests(ranges, bitsets)
    return np.array(reqs, dtype=REQ_DTYPE), words, bytes(sigs)


def _want(msg, reg, reqs, words, sigs, flavor):
    want = R.verify_aggregate(msg, reg, reqs["offset"], reqs["bitlen"], reqs["level_size"], words,
                              reqs["word_offset"].astype(np.uint64), sigs, nthreads=8)
    if flavor == "cf":  # the restatement decodes as go: cloudflare's decode errors have their own codes
        for i in range(len(reqs)):
            _, err = O.g1_unmarshal(sigs[64 * i:64 * i + 64], "cf")
            assert (err is not None) == (want[i] == _lib.HG_ERR_SIG_UNMARSHAL), i
            if err is not None:
                want[i] = CF_CODES[err]
    return want


def _ones(size, unset=()):
    bits = [True] * size
    for i in unset:
        bits[i] = False
    return bits


@pytest.fixture(scope="module", params=["go", "cf"])
def eng(request):
    import torch

    if torch.cuda.is_available():  # torch's HIP runtime before the engine's (the lanes test moves tensors)
        torch.cuda.set_device(0)
        torch.zeros(1, device="cuda")
    e = Engine(device=0, flavor=request.param)
    e.flavor_name = request.param
    e.set_aggregate_level(2)
    yield e
    e.close()


def _load(e, ks, msg=MSG):
    reg = R.g2_scalar_base(F.scalar_bytes(ks))
    assert not e.registry_load(reg).any()
    assert e.prepare_aggregate_msg(msg) == 0 and e.aggregate_tables() == 2
    return reg


@pytest.mark.parametrize("n_reg", [33, 64])
def test_small_registries_match_oracle(eng, n_reg):
    ks = F.scalars(n_reg, seed=b"torus-%d" % n_reg)
    reg = _load(eng, ks)
    assert eng.aggregate_tables_torus()
    last = n_reg - 1
    ranges = [(1, 5), (10, 12), (0, 32), (0, 32), (16, 16), (3, 30), (0, n_reg), (0, n_reg), (last, 1), (32, n_reg - 32),
              (2, 9), (0, 16)]
    bitsets = [_ones(5), _ones(12),                   # one term, two terms
               _ones(32, (0, 17)),                    # complement: block term and two unset windows
               _ones(32, range(1, 32)),               # plain fold of an aligned block: one conjugated term
               _ones(16, (5,)),                       # complement inside one window
               _ones(30), _ones(n_reg), _ones(n_reg, (7, 20, last)),
               _ones(1), _ones(n_reg - 32),           # the ragged window's key(s)
               [False] * 9,                           # empty bitset
               _ones(16)]
    special = [(1, INFINITY), (5, OFF_CURVE)]
    reqs, words, sigs = _batch(MSG, ks, ranges, bitsets, special)
    want = _want(MSG, reg, reqs, words, sigs, eng.flavor_name)
    assert list(eng.verify_aggregate(reqs, words, sigs)) == list(want)
    assert want[10] == _lib.HG_ERR_EMPTY_AGG and want[5] not in (0, 1) and want[1] == 1
    assert (want == 0).sum() >= 6 and (want == 1).sum() >= 3
    # the sequential flow, the flow that also returns the aggregate keys, and
    # VerifyMultiSignature over the whole registry: the stored pairing form and
    # the torus comparison
    eng.set_fold_overlap(False)
    try:
        assert list(eng.verify_aggregate(reqs, words, sigs)) == list(want)
    finally:
        eng.set_fold_overlap(True)
    codes, _ = eng.verify_aggregate(reqs, words, sigs, want_agg=True)
    assert list(codes) == list(want)
    full = [i for i, (off, size) in enumerate(ranges) if (off, size) == (0, n_reg)]
    multi = eng.verify_multisig(reqs["bitlen"][full], reqs["word_offset"][full], words,
                                b"".join(sigs[64 * i:64 * i + 64] for i in full))
    assert list(multi) == [want[i] for i in full]


def test_chunk_boundary_and_padding(eng):
    """160 keys, ranges off the block grid (never complemented: a term per
    window touched). Terms 8 and 9: one full chunk; a full chunk and a
    one-term chunk joined by k_gt_combine. Then a batch whose five chunks (1,
    2, 3, 7, 8 terms) share one wave: the shorter teams restore X in each
    round they sit out. And the complement of a 128-key block with an unset
    bit in every window: nine terms, the second chunk's first term not
    conjugated."""
    ks = F.scalars(160, seed=b"torus-160")
    reg = _load(eng, ks)
    assert eng.aggregate_tables_torus()
    ranges = [(1, 126), (1, 142), (0, 128), (1, 126), (1, 142)]
    bitsets = [_ones(126), _ones(142), _ones(128, range(3, 128, 16)), _ones(126, range(0, 126, 2)),
               _ones(142, range(1, 142, 3))]
    reqs, words, sigs = _batch(MSG, ks, ranges, bitsets)
    want = _want(MSG, reg, reqs, words, sigs, eng.flavor_name)
    assert list(eng.verify_aggregate(reqs, words, sigs)) == list(want)
    assert list(want) == [1, 0, 0, 0, 1]
    ranges = [(1, 5), (10, 12), (10, 30), (1, 110), (1, 126)]
    bitsets = [_ones(s) for _, s in ranges]
    reqs, words, sigs = _batch(MSG, ks, ranges, bitsets)
    want = _want(MSG, reg, reqs, words, sigs, eng.flavor_name)
    assert list(eng.verify_aggregate(reqs, words, sigs)) == list(want)
    assert list(want) == [1, 0, 0, 0, 1]


def test_four_lanes_in_flight(eng):
    """Four unpadded lanes, two alternating batches of 37 requests (a partial
    last wave of pairing teams, a partial last verdict byte)."""
    import torch

    import bench

    ks = F.scalars(64, seed=b"torus-lanes")
    reg = _load(eng, ks)
    assert eng.aggregate_tables_torus()
    rng = np.random.default_rng(21)
    n, batches, wants = 37, [], []
    for _ in range(2):
        ranges = [[(0, 64), (0, 32), (32, 32), (16, 16), (48, 8), (5, 40)][int(rng.integers(6))] for _ in range(n)]
        bitsets = F.random_bitsets(rng, [s for _, s in ranges])
        for b in bitsets:
            b[int(rng.integers(len(b)))] = True
        batches.append(_batch(MSG, ks, ranges, bitsets))
        wants.append(_want(MSG, reg, *batches[-1], eng.flavor_name))
    dev = torch.device("cuda", 0)
    dbs = [(bench._dev_bytes(r.tobytes(), dev), bench._dev_bytes(w.tobytes(), dev), bench._dev_bytes(s, dev))
           for r, w, s in batches]
    lanes = [DeviceLane(eng, n, pad=False) for _ in range(4)]
    try:
        codes = [torch.full((n,), -7, dtype=torch.int32, device=dev) for _ in lanes]
        bits = [torch.full(((n + 7) // 8,), 0x5A, dtype=torch.uint8, device=dev) for _ in lanes]
        last = [None] * 4
        for rnd in range(10):
            i, b = rnd % 4, rnd % 2 if rnd < 8 else (rnd + 1) % 2
            d_r, d_w, d_s = dbs[b]
            lanes[i].submit_device(d_r.data_ptr(), n, d_w.data_ptr(), d_s.data_ptr(), codes[i].data_ptr(),
                                   bits[i].data_ptr(), lanes[i].stream)
            last[i] = b
        torch.cuda.synchronize(dev)
        for i in range(4):
            want = wants[last[i]]
            assert list(codes[i].cpu().numpy()) == list(want), i
            assert list(bits[i].cpu().numpy()) == list(np.packbits(want == 0, bitorder="little")), i
    finally:
        for lane in lanes:
            lane.close()


@pytest.mark.parametrize("kind", ["pair", "triple"])
def test_degenerate_registry_stays_unconverted(eng, kind):
    """Keys k and r - k in one window, or three keys that sum to zero: some
    subset's product is e(H, 0) = 1, which has no alpha. The scan finds it
    before anything is written, the set is reported unconverted and folds
    through k_gt_chunks."""
    ks = F.scalars(33, seed=b"torus-degenerate")
    if kind == "pair":
        ks[3] = O.ORDER - ks[2]
    else:
        ks[21] = (-ks[18] - ks[19]) % O.ORDER
    reg = _load(eng, ks)
    assert not eng.aggregate_tables_torus()
    ranges = [(0, 33), (0, 16), (2, 2), (16, 16), (18, 4), (0, 32), (1, 20), (32, 1)]
    bitsets = [_ones(33), _ones(16, (9,)), _ones(2), _ones(16, (0, 1)), _ones(4), _ones(32, (2, 18)), _ones(20),
               _ones(1)]
    special = [(2, INFINITY)] if kind == "pair" else [(3, INFINITY)]  # the aggregate key is zero there
    reqs, words, sigs = _batch(MSG, ks, ranges, bitsets, special)
    want = _want(MSG, reg, reqs, words, sigs, eng.flavor_name)
    assert list(eng.verify_aggregate(reqs, words, sigs)) == list(want)
    assert (want == 0).sum() >= 4 and (want == 1).sum() >= 2
    # a registry without such keys converts again
    _load(eng, F.scalars(33, seed=b"torus-after"))
    assert eng.aggregate_tables_torus()


def test_two_messages_keep_their_form(eng):
    ks = F.scalars(64, seed=b"torus-two")
    msgs = [F.LIB_MESSAGE, F.TEST_MESSAGES[1]]
    reg = R.g2_scalar_base(F.scalar_bytes(ks))
    assert not eng.registry_load(reg).any()
    ranges = [(0, 64), (0, 32), (32, 32), (7, 50), (16, 16)]
    bitsets = [_ones(64, (1, 2, 40)), _ones(32, range(0, 32, 2)), _ones(32), _ones(50, (3,)), _ones(16, (4,))]
    batches = [_batch(m, ks, ranges, bitsets) for m in msgs]
    wants = [_want(m, reg, *b, eng.flavor_name) for m, b in zip(msgs, batches)]
    for m in msgs:
        assert eng.prepare_aggregate_msg(m) == 0 and eng.aggregate_tables_torus()
    for i in range(4):
        k = i % 2
        assert list(eng.verify_aggregate_msg(msgs[k], *batches[k])) == list(wants[k]), i
        assert eng.aggregate_tables() == 2 and eng.aggregate_tables_torus(), i
        # the other message's signatures fail under this one
        assert not (np.asarray(eng.verify_aggregate(*batches[1 - k])) == 0).any(), i
