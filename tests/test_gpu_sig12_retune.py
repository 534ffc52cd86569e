"""The retuned 12-lane pairing programs on the GPU (tools/gen_g2_schedule.py
KARATSUBA_MIN_PROG, REDC_FUSE: Karatsuba products in the cyclotomic squaring,
products-then-REDC in SQR12_12 / LINE_FIX_12 / MUL12_12) against the unchanged
16-lane k_verify_sig: hg_sig_pairing_device's kernels 2 and 3 (k_verify_sig12
padded, and the unpadded split form k_sig12_miller / k_sig12_ninv / k_sig12_fe)
write the FE values — canonical Montgomery bytes — that kernel 0 writes, and
kernel 1 (k_verify_sig unpadded) with them.

Sizes: 1; 5 and 6 (one full wave of five teams, then one team of the next);
60 (twelve waves, every team full); 257 (past the 256-check block of the
batched norm inversion). Every batch holds the point at infinity and a
signature equal to the G1 generator (coordinates 1 and p - 2: the smallest
and nearly the largest limbs the line evaluation sees); at n = 1 the two
are separate batches. One verdict run takes 61 config-3-shaped requests
through an unpadded device lane against the reference algorithm.
"""

import numpy as np
import pytest

from oracle import bn256_oracle as O
from oracle import ref_lib as R
from tests import _fixtures as F

pytestmark = pytest.mark.gpu

SIZES = (1, 5, 6, 60, 257)


def _batches(eng, n):
    import bench

    sigs = bytearray(eng.sign(bench.seeded_scalars(n, 2700 + n)))
    gen = O.g1_marshal(O.G1_GEN)
    if n == 1:
        return [bytes(64), gen]
    sigs[0:64] = bytes(64)               # the point at infinity
    sigs[64 * (n - 1):64 * n] = gen      # the last team of the last wave
    return [bytes(sigs)]


@pytest.mark.parametrize("flavor", ["go", "cf"])
def test_retuned_12_lane_kernels_match_k_verify_sig(request, flavor):
    import torch

    import bench

    eng = request.getfixturevalue("engine" if flavor == "go" else "engine_cf")
    dev = torch.device("cuda", 0)
    assert eng.set_message(F.LIB_MESSAGE) == 0
    stream = torch.cuda.current_stream(dev).cuda_stream
    for n in SIZES:
        for sigs in _batches(eng, n):
            d_sigs = bench._dev_bytes(sigs, dev)
            outs = []
            for k in range(4):
                fe = torch.full((n * 480,), 0x5A, dtype=torch.uint8, device=dev)
                eng.sig_pairing_device(d_sigs.data_ptr(), n, fe.data_ptr(), k, stream)
                torch.cuda.synchronize(dev)
                outs.append(fe.cpu().numpy())
            for k in (1, 2, 3):
                bad = np.flatnonzero((outs[0] != outs[k]).reshape(n, 480).any(axis=1))
                assert bad.size == 0, f"{flavor} n={n} kernel {k}: checks {bad[:8]} differ from kernel 0"
            # every value was written, and is canonical: ten 26-bit limbs
            # (the top one 20 bits) below p in Montgomery form
            v = outs[0].view(np.uint32).reshape(n * 12, 10)
            assert (v[:, :9] < (1 << 26)).all() and (v[:, 9] <= (O.P >> 234)).all(), (flavor, n)
            if sigs[:64] == bytes(64):  # e(inf, G2Base) = 1: only c0.y (one in Montgomery form) nonzero
                first = v[:12]
                assert [e for e in range(12) if first[e].any()] == [1], (flavor, n)


def test_unpadded_lane_verdicts_match_the_reference(engine):
    """61 multisignatures over a 500-key registry (random node and level, 1/8
    tampered) through DeviceLane(pad=False): k_sig12_miller / k_sig12_fe feed
    the comparison with the GT fold, so a wrong FE value is a wrong verdict."""
    import torch

    import bench
    from handel_amd.engine import DeviceLane

    n = 61
    assert engine.set_message(F.LIB_MESSAGE) == 0
    reqs, words, sigs, expect, _, reg = bench.make_aggregate_batch(engine, 500, n, seed=977)
    assert engine.prepare_aggregate() == 0 and engine.aggregate_tables() == 2
    want = R.verify_aggregate(F.LIB_MESSAGE, reg, reqs["offset"], reqs["bitlen"], reqs["level_size"], words,
                              reqs["word_offset"].astype(np.uint64), sigs, nthreads=16)
    assert 0 < np.count_nonzero(want) < n, "some tampered, most valid"
    dev = torch.device("cuda", 0)
    d_r, d_w, d_s = (bench._dev_bytes(b, dev) for b in (reqs.tobytes(), words.tobytes(), sigs))
    lane = DeviceLane(engine, n, pad=False)
    try:
        codes = torch.full((n,), -7, dtype=torch.int32, device=dev)
        bits = torch.full(((n + 7) // 8,), 0x5A, dtype=torch.uint8, device=dev)
        lane.submit_device(d_r.data_ptr(), n, d_w.data_ptr(), d_s.data_ptr(), codes.data_ptr(), bits.data_ptr(),
                           lane.stream)
        torch.cuda.synchronize(dev)
        got = codes.cpu().numpy()
    finally:
        lane.close()
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:8]
