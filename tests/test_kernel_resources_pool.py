"""The standing queue's kernels (handel_amd/csrc/hg_pool.hip) keep what
DESIGN.md §3i states for them: integer and memory kernels without LDS (the
replay holds its k candidates one per lane), none of them spills or uses
scratch. Reads the library's metadata notes (tools/kernel_sizes.py); no GPU
needed (skipped when the library is not built)."""

import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
LIB = os.path.join(ROOT, "handel_amd", "_build", "libhandel_gpu.so")

# mangled-name fragment: (LDS bytes, VGPR ceiling: eight waves per SIMD fit below 64)
POOL = {
    "k_pool_admit": (0, 64),
    "k_pool_copy": (0, 64),
    "k_pool_bump": (0, 64),
    "k_pool_score": (0, 64),
    "k_pool_runs": (0, 64),
    "k_pool_replay": (0, 64),
    "k_pool_move": (0, 64),
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


@pytest.mark.parametrize("part", sorted(POOL))
def test_pool_kernels_keep_their_budgets(res, part):
    hits = {k: v for k, v in res.items() if part in k}
    assert len(hits) == 1, (part, sorted(hits))
    r = next(iter(hits.values()))
    lds, vgpr = POOL[part]
    assert r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0 and r["scratch"] == 0, (part, r)
    assert r["lds"] == lds, (part, r)
    assert r["vgpr"] <= vgpr, (part, r)


def test_every_pool_kernel_is_listed(res):
    names = {k for k in res if "k_pool_" in k}
    assert len(names) == len(POOL), sorted(names)
