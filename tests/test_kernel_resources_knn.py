"""The KNN kernels exist in the built library and hold their resources (CPU only: reads the gfx950 code objects'
metadata, tools/kernel_resources.py): no scratch and no spill anywhere, no LDS in the apply, background and model
kernels (DESIGN.md §5 "KNN": every pixel is independent, nothing is shared), and the register counts at what the
build shows (a kernel that grows fails here and the bound is then set on purpose).  No scratch is the point: the
sample loop has a run-time bound, and what a lane keeps between samples is a few counters per pixel, never an
array indexed by the sample."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
LIB = os.path.join(ROOT, "opencv_amd", "lib", "libtbdk.so")

pytestmark = pytest.mark.skipif(not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf"),
                                reason="llvm-readelf missing")

# channels -> VGPRs the build shows
APPLY = {1: 49, 3: 64}
BACKGROUND = {1: 20, 3: 20}
MODEL, RANDU = 25, 22


@pytest.fixture(scope="module")
def res():
    import kernel_resources

    assert os.path.exists(LIB), "the library is not built"
    return {k: v for k, v in kernel_resources.kernel_resources(LIB).items() if "knn_" in k and "klt" not in k}


def no_scratch(v):
    assert v["private_segment_fixed_size"] == 0 and v["vgpr_spill_count"] == 0 and v["sgpr_spill_count"] == 0, v


def one(res, name):
    ks = [n for n in res if name in n]
    assert len(ks) == 1, (name, ks)
    return res[ks[0]]


@pytest.mark.parametrize("cn", sorted(APPLY))
def test_apply_kernel(res, cn):
    v = one(res, f"knn_apply_kernelILi{cn}EE")
    no_scratch(v)
    assert v["group_segment_fixed_size"] == 0, v
    assert v["vgpr_count"] <= APPLY[cn], v


def test_the_other_kernels(res):
    assert len([n for n in res if "knn_apply_kernel" in n]) == len(APPLY)
    for cn, vgpr in BACKGROUND.items():
        v = one(res, f"knn_background_kernelILi{cn}EE")
        no_scratch(v)
        assert v["group_segment_fixed_size"] == 0 and v["vgpr_count"] <= vgpr, v
    v = one(res, "knn_model_kernel")
    no_scratch(v)
    assert v["group_segment_fixed_size"] == 0 and v["vgpr_count"] <= MODEL, v
    v = one(res, "knn_randu_kernel")
    no_scratch(v)
    assert v["vgpr_count"] <= RANDU, v
