"""The MOG2 kernels exist in the built library and hold their resources (CPU only: reads the gfx950 code
objects' metadata, tools/kernel_resources.py): no scratch, no spill, no LDS (DESIGN.md §5 "MOG2": every pixel
is independent, nothing is shared), and the register counts at what the build shows (a kernel that grows
fails here and the bound is then set on purpose).  No scratch is the point: a pixel's modes live in
registers only while every index into them is a constant after unrolling."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
LIB = os.path.join(ROOT, "opencv_amd", "lib", "libtbdk.so")

pytestmark = pytest.mark.skipif(not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf"),
                                reason="llvm-readelf missing")

# (channels, nmixtures) -> VGPRs the build shows
APPLY = {(1, 1): 34, (1, 2): 50, (1, 3): 63, (1, 4): 76, (1, 5): 93, (1, 6): 103, (1, 7): 118, (1, 8): 139,
         (3, 1): 46, (3, 2): 74, (3, 3): 97, (3, 4): 124, (3, 5): 141, (3, 6): 188, (3, 7): 234, (3, 8): 207}
BACKGROUND = {1: 19, 3: 31}


@pytest.fixture(scope="module")
def res():
    import kernel_resources

    assert os.path.exists(LIB), "the library is not built"
    return {k: v for k, v in kernel_resources.kernel_resources(LIB).items() if "mog2_" in k}


def clean(v):
    assert v["private_segment_fixed_size"] == 0 and v["vgpr_spill_count"] == 0 and v["sgpr_spill_count"] == 0, v
    assert v["group_segment_fixed_size"] == 0, v


@pytest.mark.parametrize("cn,k", sorted(APPLY))
def test_apply_kernel(res, cn, k):
    ks = [n for n in res if f"mog2_apply_kernelILi{cn}ELi{k}EE" in n]
    assert len(ks) == 1, ks
    clean(res[ks[0]])
    assert res[ks[0]]["vgpr_count"] <= APPLY[cn, k], res[ks[0]]


def test_the_other_kernels(res):
    assert len([n for n in res if "mog2_apply_kernel" in n]) == len(APPLY)
    for cn, vgpr in BACKGROUND.items():
        ks = [n for n in res if f"mog2_background_kernelILi{cn}EE" in n]
        assert len(ks) == 1, ks
        clean(res[ks[0]])
        assert res[ks[0]]["vgpr_count"] <= vgpr
    ks = [n for n in res if "mog2_model_kernel" in n]
    assert len(ks) == 1, ks
    clean(res[ks[0]])
