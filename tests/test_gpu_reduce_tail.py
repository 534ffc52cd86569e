"""The one-chain reduction tail of the 12-lane pairing programs (bn256_redq.h:
the linear-term rounds of CYC_SQR_X_12 and LINE_FIX_12) on the GPU, against
the 16-lane k_verify_sig, whose programs keep acc_reduce_wide:
hg_sig_pairing_device's kernel 3 (the split k_sig12_miller / k_sig12_ninv /
k_sig12_fe) and kernel 2 (k_verify_sig12 padded) write the FE bytes —
canonical Montgomery limbs — that kernel 0 writes, for every signature that
decodes (HG_OK by the oracle's SigBLS decoding).

n = 7 (two waves of five teams, the second with two) and n = 65 (thirteen
waves, every team full), both flavors; every batch holds the point at
infinity and one signature that fails to decode (a point off the curve),
whose FE value no path compares.
"""

import numpy as np
import pytest

from oracle import bn256_oracle as O
from tests import _fixtures as F

pytestmark = pytest.mark.gpu

SIZES = (7, 65)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("flavor", ["go", "cf"])
def test_split_12_lane_kernels_match_the_16_lane_kernel(request, flavor, n):
    import torch

    import bench

    eng = request.getfixturevalue("engine" if flavor == "go" else "engine_cf")
    dev = torch.device("cuda", 0)
    assert eng.set_message(F.LIB_MESSAGE) == 0
    stream = torch.cuda.current_stream(dev).cuda_stream
    sigs = bytearray(eng.sign(bench.seeded_scalars(n, 4100 + n)))
    sigs[64 * 2:64 * 3] = bytes(64)                                       # the point at infinity
    sigs[64 * (n - 2):64 * (n - 1)] = (1).to_bytes(32, "big") + (1).to_bytes(32, "big")  # 1 != 1 + 3: off the curve
    ok = np.array([O.sig_unmarshal_error(bytes(sigs[64 * i:64 * i + 64]), flavor) is None for i in range(n)])
    assert np.flatnonzero(~ok).tolist() == [n - 2], "exactly the planted signature fails to decode"
    d_sigs = bench._dev_bytes(bytes(sigs), dev)
    outs = {}
    for k in (0, 2, 3):
        fe = torch.full((n * 480,), 0x5A, dtype=torch.uint8, device=dev)
        eng.sig_pairing_device(d_sigs.data_ptr(), n, fe.data_ptr(), k, stream)
        torch.cuda.synchronize(dev)
        outs[k] = fe.cpu().numpy().reshape(n, 480)
    for k in (2, 3):
        bad = np.flatnonzero((outs[0] != outs[k]).any(axis=1) & ok)
        assert bad.size == 0, f"{flavor} n={n} kernel {k}: checks {bad[:8]} differ from kernel 0"
    # canonical values: ten 26-bit limbs, the top one at most p's
    v = outs[3][ok].view(np.uint32).reshape(-1, 10)
    assert (v[:, :9] < (1 << 26)).all() and (v[:, 9] <= (O.P >> 234)).all(), (flavor, n)
    # e(inf, G2Base) = 1: only c0.y (one in Montgomery form) nonzero
    first = outs[3][2].view(np.uint32).reshape(12, 10)
    assert [e for e in range(12) if first[e].any()] == [1], (flavor, n)
