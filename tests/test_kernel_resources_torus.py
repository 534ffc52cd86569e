"""The torus fold's kernels (handel_amd/csrc/bn256_gt.hip; the table
conversion: bn256_gttab.hip) keep the budgets
DESIGN.md §3a argues from: k_tor_chunks runs in k_gt_chunks' place, so it has
its LDS (12 000 B: five 12-lane teams of the 60-element fold region) and at
most its 212 VGPRs, and a fold workgroup still fits beside eight pairing waves
in a CU's LDS; k_tor_compare_bits has k_gt_combine's four-team region; none of
the new kernels spills or uses scratch, the table conversion included. Reads
the library's metadata notes (tools/kernel_sizes.py); no GPU needed (skipped
when the library is not built)."""

import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
LIB = os.path.join(ROOT, "handel_amd", "_build", "libhandel_gpu.so")

# mangled-name fragment: (LDS bytes, VGPR ceiling or None)
TORUS = {
    "k_tor_chunks": (12000, 212),
    "k_tor_compare_bits": (9600, 256),
    "k_tor_convert": (0, None),
    "k_tor_scan": (0, None),
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


@pytest.mark.parametrize("part", sorted(TORUS))
def test_torus_kernels_keep_their_budgets(res, part):
    hits = {k: v for k, v in res.items() if part in k}
    assert len(hits) == 1, (part, sorted(hits))
    r = next(iter(hits.values()))
    lds, vgpr = TORUS[part]
    assert r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0 and r["scratch"] == 0, (part, r)
    assert r["lds"] == lds, (part, r)
    if vgpr is not None:
        assert r["vgpr"] <= vgpr, (part, r)


def test_new_names_leave_the_classical_fold_kernels_unique(res):
    """tests/test_kernel_resources.py looks the classical fold kernels up by
    name fragment: the new kernels' names contain neither."""
    for part in ("k_gt_chunks", "k_gt_combine"):
        assert len([k for k in res if part in k]) == 1, part
