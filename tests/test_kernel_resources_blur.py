"""The blur and threshold kernels exist in the built library and hold their resources (CPU only: reads the gfx950
code objects' metadata, tools/kernel_resources.py): the five instances of the blur kernel (3, 5, 7, 11 and the
run-time-size one), no scratch and no spill anywhere (the run-time tap loops index the kernel arguments, never a
private array), the blur's LDS at what DESIGN.md §5 "GaussianBlur and threshold" states (248 x 62 source bytes and
128 x 62 words, five workgroups a CU), and the register counts at what the build shows (a kernel that grows fails here
and the bound is then set on purpose)."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
LIB = os.path.join(ROOT, "opencv_amd", "lib", "libtbdk.so")

pytestmark = pytest.mark.skipif(not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf"),
                                reason="llvm-readelf missing")

BLUR_VGPRS = {0: 32, 3: 32, 5: 32, 7: 41, 11: 61}  # taps (0: run-time sizes) -> VGPRs the build shows
BLUR_LDS = 4 * (62 * 62 + 1) + 8 * 32 * 62
OTHERS = {"thresh_u8_kernel": 11, "thresh_f32_kernel": 4, "hist_u8_kernel": 8, "otsu_scan_kernel": 60}


@pytest.fixture(scope="module")
def res():
    import kernel_resources

    assert os.path.exists(LIB), "the library is not built"
    return {k: v for k, v in kernel_resources.kernel_resources(LIB).items()
            if "blur_kernel" in k or any(n in k for n in OTHERS)}


def no_scratch(v):
    assert v["private_segment_fixed_size"] == 0 and v["vgpr_spill_count"] == 0 and v["sgpr_spill_count"] == 0, v


def test_blur_instances(res):
    names = [n for n in res if "blur_kernel" in n]
    assert len(names) == len(BLUR_VGPRS), names
    for k, vgpr in BLUR_VGPRS.items():
        ks = [n for n in names if f"blur_kernelILi{k}ELi{k}EE" in n]
        assert len(ks) == 1, (k, names)
        v = res[ks[0]]
        no_scratch(v)
        assert v["group_segment_fixed_size"] == BLUR_LDS and 5 * BLUR_LDS <= 160 * 1024, v
        assert v["vgpr_count"] <= vgpr, (k, v)


def test_threshold_kernels(res):
    for name, vgpr in OTHERS.items():
        ks = [n for n in res if name in n]
        assert len(ks) == 1, (name, ks)
        no_scratch(res[ks[0]])
        assert res[ks[0]]["vgpr_count"] <= vgpr, (name, res[ks[0]])
    assert res[[n for n in res if "hist_u8_kernel" in n][0]]["group_segment_fixed_size"] == 1024
