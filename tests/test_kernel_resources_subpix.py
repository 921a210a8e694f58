"""The cornerSubPix kernel exists in the built library for the three pixel types
and holds its resources (CPU only: reads the gfx950 code objects' metadata,
tools/kernel_resources.py): no scratch, no spill, and only the five sums as
static LDS (the patch, the mask and the terms are dynamic LDS sized by the window)."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
LIB = os.path.join(ROOT, "opencv_amd", "lib", "libtbdk.so")

pytestmark = pytest.mark.skipif(not os.path.exists(LIB) or not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf"),
                                reason="library or llvm-readelf missing")


def test_corner_sub_pix_instances():
    import kernel_resources

    res = kernel_resources.kernel_resources(LIB)
    ks = sorted(k for k in res if "corner_sub_pix_kernel" in k)
    # <pix>: 0 = TBDK_PIX_U8, 1 = TBDK_PIX_U16, 2 = TBDK_PIX_F32
    assert len(ks) == 3 and all(any(f"corner_sub_pix_kernelILi{p}E" in k for k in ks) for p in (0, 1, 2)), ks
    for k in ks:
        v = res[k]
        assert v["private_segment_fixed_size"] == 0 and v["vgpr_spill_count"] == 0 and v["sgpr_spill_count"] == 0, (k, v)
        assert v["group_segment_fixed_size"] == 40, (k, v)  # s_res[5]
        assert v["vgpr_count"] <= 64, (k, v)
