"""The KLT point tracker's three kernels exist in the built library and hold their
resources (CPU only: reads the gfx950 code objects' metadata,
tools/kernel_resources.py): no scratch memory and no spills, VGPR or SGPR.  The
compaction and append kernels are one workgroup of 1024 threads (four waves per
SIMD), so they must stay within 128 VGPRs to launch at all; the bounds below are
what the build shows.  The compaction's LDS is its tile's two 1024-entry lists
and the 16 wave sums; the other two use none (KLT point tracker)."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
LIB = os.path.join(ROOT, "opencv_amd", "lib", "libtbdk.so")

pytestmark = pytest.mark.skipif(not os.path.exists(LIB) or not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf"),
                                reason="library or llvm-readelf missing")


@pytest.fixture(scope="module")
def res():
    import kernel_resources

    return kernel_resources.kernel_resources(LIB)


def one(res, name):
    ks = [k for k in res if name in k]
    assert len(ks) == 1, (name, ks)
    v = res[ks[0]]
    assert v["private_segment_fixed_size"] == 0 and v["vgpr_spill_count"] == 0 and v["sgpr_spill_count"] == 0, (name, v)
    return v


def test_compact_kernel(res):
    v = one(res, "klt_compact_kernel")
    assert v["group_segment_fixed_size"] == 2 * 1024 * 4 + 16 * 4, v  # s_src, s_len, s_wsum: 8,256 bytes as built
    assert v["vgpr_count"] <= 48, v  # 46 as built


def test_append_kernel(res):
    v = one(res, "klt_append_kernel")
    assert v["group_segment_fixed_size"] == 0, v
    assert v["vgpr_count"] <= 16, v  # 14 as built


def test_mask_circles_kernel(res):
    v = one(res, "klt_mask_circles_kernel")
    assert v["group_segment_fixed_size"] == 0, v
    assert v["vgpr_count"] <= 32, v  # 32 as built
