"""GPU suite: the 12-lane pairing with its line pairs fused (LINE2_FIX_12,
team_miller_sig12: one round per nonzero NAF digit's two lines and per the
two Frobenius lines, f seeded with the first line).

hg_sig_pairing_device's FE(Miller(G2Base at -sig)) bytes of the 12-lane
kernels — kernel 2: the monolithic k_verify_sig12, kernel 3: the split
k_sig12_miller / k_sig12_ninv / k_sig12_fe — against the unchanged 16-lane
k_verify_sig (kernels 0 and 1), which multiplies line by line, and against the
oracle's Fuentes-Castaneda value. Batch sizes 1, 5, 6 and 11: padding teams, a
full wave, a second wave with one team, a ragged third wave. Both flavors; a
signature at infinity and one that fails to decode (its value is never
compared with anything by the verifier: the 12-lane kernels give it the
scalars of infinity, hence the identity, the 16-lane one whatever its
coordinates give). Then the verdicts of a tiny aggregate batch on an unpadded
lane, the headline's path. Last the round itself through the instance probe
(hg_debug_xinst, probe instance PROBE_EXTRA_BASE): word for word the
generator's limb model on the thirteen edge regions of tests/test_xinst_edges.py
and on a region with every element at the limb bound.
"""

import ctypes

import numpy as np
import pytest

from oracle import bn256_oracle as O
from tests import _fixtures as F
from tests._gt_model import fe_bytes as _fe_bytes

pytestmark = pytest.mark.gpu

# n -> (index of the signature at infinity, index of the undecodable one)
CASES = {1: (None, None), 5: (1, None), 6: (2, 4), 11: (3, 7)}



def _oracle_fe(sig: bytes, flavor: str):
    pt, err = O.g1_unmarshal(sig, flavor)
    assert err is None
    if pt is None:
        return _fe_bytes(O.F12_ONE)
    return _fe_bytes(O.final_exponentiation_fc(O.miller(O.G2_GEN, O.g1_neg(pt))))


@pytest.mark.parametrize("flavor", ["go", "cf"])
def test_fused_pairing_matches_the_16_lane_kernel_and_the_oracle(request, flavor):
    import torch

    import bench

    eng = request.getfixturevalue("engine" if flavor == "go" else "engine_cf")
    dev = torch.device("cuda", 0)
    assert eng.set_message(F.LIB_MESSAGE) == 0
    one = _fe_bytes(O.F12_ONE)
    for n, (inf, bad) in CASES.items():
        sigs = bytearray(eng.sign(bench.seeded_scalars(n, 2600 + n)))
        if inf is not None:
            sigs[64 * inf:64 * inf + 64] = bytes(64)
        if bad is not None:
            sigs[64 * bad:64 * bad + 32] = b"\xff" * 32  # x >= p
            assert O.g1_unmarshal(bytes(sigs[64 * bad:64 * bad + 64]), flavor)[1] is not None
        d_sigs = bench._dev_bytes(bytes(sigs), dev)
        outs = []
        for k in range(4):
            fe = torch.full((n * 480,), 0x5A, dtype=torch.uint8, device=dev)
            eng.sig_pairing_device(d_sigs.data_ptr(), n, fe.data_ptr(), k, torch.cuda.current_stream(dev).cuda_stream)
            torch.cuda.synchronize(dev)
            outs.append(fe.cpu().numpy().reshape(n, 480))
        compared = [i for i in range(n) if i != bad]
        for k in (2, 3):
            assert np.array_equal(outs[k][compared], outs[0][compared]), (flavor, n, k)
            assert np.array_equal(outs[k][compared], outs[1][compared]), (flavor, n, k)
            if inf is not None:
                assert np.array_equal(outs[k][inf], one), (flavor, n, k)
            if bad is not None:
                assert np.array_equal(outs[k][bad], one), (flavor, n, k)
        # the oracle's value: every signature of the smallest batches, two of the others
        for i in (compared if n <= 5 else [0, n - 1]):
            want = _oracle_fe(bytes(sigs[64 * i:64 * i + 64]), flavor)
            assert np.array_equal(outs[2][i], want) and np.array_equal(outs[3][i], want), (flavor, n, i)


def test_tiny_aggregate_batch_on_an_unpadded_lane(engine):
    """11 multisignatures on a 64-key registry through DeviceLane(pad=False)
    (k_sig_scalars, k_sig_lines, the split 12-lane pairing): tampered, and
    one undecodable signature, against the reference algorithm."""
    import torch

    import bench
    from handel_amd.engine import DeviceLane
    from tests.test_gpu_headline_path import _oracle

    dev = torch.device("cuda", 0)
    n = 11
    assert engine.set_message(F.LIB_MESSAGE) == 0
    reqs, words, sigs, expect, _, reg = bench.make_aggregate_batch(engine, 64, n, seed=977)
    assert engine.prepare_aggregate() == 0
    s = bytearray(sigs)
    s[64 * 5:64 * 5 + 32] = b"\xff" * 32
    sigs = bytes(s)
    want = _oracle(reg, reqs, words, sigs, "go")
    assert want[5] == 5 and {0, 1} <= set(want.tolist())
    assert np.array_equal(np.delete(want, 5), np.delete(expect, 5))
    lane = DeviceLane(engine, n, pad=False)
    try:
        d = [bench._dev_bytes(b, dev) for b in (reqs.tobytes(), words.tobytes(), sigs)]
        codes = torch.full((n,), -7, dtype=torch.int32, device=dev)
        bits = torch.full(((n + 7) // 8,), 0x5A, dtype=torch.uint8, device=dev)
        lane.submit_device(d[0].data_ptr(), n, d[1].data_ptr(), d[2].data_ptr(), codes.data_ptr(), bits.data_ptr(),
                           lane.stream)
        torch.cuda.synchronize(dev)
    finally:
        lane.close()
    assert np.array_equal(codes.cpu().numpy(), want)
    assert np.array_equal(bits.cpu().numpy(),
                          np.packbits(np.concatenate([want == 0, np.zeros((-n) % 8, bool)]), bitorder="little"))


def test_probe_of_the_pair_round_equals_the_limb_model(engine):
    """As tests/test_gpu_xinst.py for the numbered instances: the whole region
    after LINE2_FIX_12_T<F, F>, pre-pass scratch and untouched elements
    included; lazy operands, operands at the limb bound and the guarded rare
    subtraction are among the cases (tests/test_line_pairs.py)."""
    from tests import test_line_pairs as LP

    G = LP.G
    inst = G.PROBE_EXTRA_BASE
    runs = LP.line2_runs()
    assert sum(r.subs["csub_rare"][1] for r in runs) >= 1
    assert engine.xinst_region_elems(inst) == LP.E.region_elems()["T"]
    got = engine.xinst(inst, np.array([r.mem_in for r in runs], dtype=np.uint32))
    want = np.array([r.mem_out for r in runs], dtype=np.uint32)
    if not np.array_equal(got, want):
        c, e, l = (int(v[0]) for v in np.nonzero(got != want))
        pytest.fail(f"case {c} ({runs[c].case!r}), element {e}, limb {l}: GPU 0x{int(got[c, e, l]):08x}, "
                    f"model 0x{int(want[c, e, l]):08x}; {int((got != want).any(axis=2).sum())} elements differ")
    # the numbered cases end where they did, and nothing lies behind the extra one
    re = ctypes.c_int(-77)
    for bad in (len(G.ALL_INSTANCES), inst + len(G.PAIR_INSTANCES), inst - 1):
        assert engine.L.hg_debug_xinst(engine.ctx, bad, 0, None, 0, None, ctypes.byref(re)) == 100 and re.value == -77
    assert engine.L.hg_debug_xinst(engine.ctx, inst, 1, None, 0, None, ctypes.byref(re)) == 100  # no split form
