"""bench.py's plain run and --dump-outputs.

A plain `bench.py --gpus 1 --steps N --warmup W` prints the headline's line
alone (everything else it measures sits behind --full), and --dump-outputs DIR
writes the verdicts of the last timed step as DIR/<name>.npy in float32: the
inputs are seeded, so two builds are compared output for output.
"""

import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL_ONLY = ("roofline", "roofline_k_verify", "roofline_k_verify_sig12", "roofline_gt_fold", "effective_rate",
             "cpu_baseline", "sequential", "single", "single_registry", "full_registry", "pipelined",
             "packet_intake", "batch_latency", "handel_run_volume", "config4_proxy")


def test_dump_outputs_float32_and_seeded_sample(tmp_path, monkeypatch):
    import torch

    import bench

    codes = torch.arange(10, dtype=torch.int32)
    bits = torch.tensor([254, 3], dtype=torch.uint8)
    got = bench.dump_outputs(str(tmp_path / "a"), {"verdict_codes": codes, "verdict_bitset": bits})
    assert got == {"verdict_codes": 10, "verdict_bitset": 2}
    c = np.load(tmp_path / "a" / "verdict_codes.npy")
    assert c.dtype == np.float32 and np.array_equal(c, np.arange(10))
    assert np.array_equal(np.load(tmp_path / "a" / "verdict_bitset.npy"), [254, 3])
    # over the size limit: a fixed sample, in order, the same on every run
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 4 * 2 * 4)
    for d in ("b", "c"):
        assert bench.dump_outputs(str(tmp_path / d), {"verdict_codes": codes, "verdict_bitset": bits}) == {
            "verdict_codes": 4, "verdict_bitset": 2}
    b, c = (np.load(tmp_path / d / "verdict_codes.npy") for d in ("b", "c"))
    assert np.array_equal(b, c) and len(b) == 4 and np.all(np.diff(b) > 0)


def _env():
    return {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "HG_BENCH_BACKEND",
                                                             "HG_BENCH_FORCE_PG", "HG_BENCH_LAUNCHED")}


@pytest.mark.gpu
def test_plain_run_prints_the_headline_alone_and_dumps_its_verdicts(tmp_path):
    env = _env()
    out = tmp_path / "out"
    r = subprocess.run([sys.executable, "-u", os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3",
                        "--warmup", "1", "--prewarm", "0.05", "--dump-outputs", str(out)],
                       capture_output=True, text=True, timeout=280, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    line = json.loads(lines[0])
    assert line["metric"] == "BN254 aggregate-sig verifications/sec (batch 4096)"
    assert line["unit"] == "verifications/s" and line["higher_is_better"] is True and line["dtype"]
    assert line["steps"] == 3 and line["warmup"] == 1 and line["full"] is False
    assert line["value"] > 0 and line["ms_per_step"] > 0
    # value is the batch over the step time
    assert line["value"] == pytest.approx(4096 / (line["ms_per_step"] * 1e-3), rel=1e-3)
    assert not [k for k in FULL_ONLY if k in line]
    # the last timed step's verdicts: every 8th aggregate tampered (code 1),
    # bit i of the bitset = check i valid
    assert line["outputs"] == {"verdict_codes": 4096, "verdict_bitset": 512}
    assert sorted(os.listdir(out)) == ["verdict_bitset.npy", "verdict_codes.npy"]
    codes = np.load(out / "verdict_codes.npy")
    assert codes.dtype == np.float32 and codes.shape == (4096,)
    assert np.array_equal(codes, (np.arange(4096) % 8 == 0).astype(np.float32))
    bits = np.load(out / "verdict_bitset.npy")
    assert bits.dtype == np.float32 and np.array_equal(bits, np.full(512, 254.0))


@pytest.mark.gpu
def test_full_run_adds_what_moved():
    """--full (trimmed to stay short: no CPU baselines, no process-model
    lines, no second pipelined context): the same headline fields, then the
    rooflines, the sequential line and the sub-lines."""
    r = subprocess.run([sys.executable, "-u", os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2",
                        "--warmup", "1", "--prewarm", "0.05", "--full", "--no-cpu", "--no-service", "--pipeline", "1"],
                       capture_output=True, text=True, timeout=280, env=_env(), cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    line = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert line["full"] is True and line["steps"] == 2 and line["value"] > 0 and line["ms_per_step"] > 0
    assert line["cpu_baseline"] is None and "config4_proxy" not in line and "pipelined" not in line
    for k in FULL_ONLY:
        if k not in ("cpu_baseline", "config4_proxy", "pipelined"):
            assert line[k], k
    assert 0 < line["roofline"]["frac"] < 1
