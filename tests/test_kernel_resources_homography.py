"""The findHomography kernel exists in the built library and holds its resources
(CPU only: reads the gfx950 code objects' metadata, tools/kernel_resources.py): no
scratch, no spill, LDS at the figure DESIGN.md §5 "findHomography" documents, and
the register count at what the build shows (a kernel that grows fails here and the
bound is then set on purpose)."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
LIB = os.path.join(ROOT, "opencv_amd", "lib", "libtbdk.so")

pytestmark = pytest.mark.skipif(not os.path.exists(LIB) or not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf"),
                                reason="library or llvm-readelf missing")

# 4096 pairs (2 x 32 KB), 64 solver columns of 135 doubles, 64 models of 9 doubles, 4 x 64 subset indices, 64 flags
LDS = 2 * 4096 * 8 + 135 * 64 * 8 + 64 * 9 * 8 + 4 * 64 * 4 + 64 * 4
VGPR = 256  # one wave per SIMD, which the LDS footprint (one workgroup per CU) allows anyway


def test_find_homography_kernel():
    import kernel_resources

    res = kernel_resources.kernel_resources(LIB)
    ks = [k for k in res if "find_homography_kernel" in k]
    assert len(ks) == 1, ks
    v = res[ks[0]]
    assert v["private_segment_fixed_size"] == 0 and v["vgpr_spill_count"] == 0 and v["sgpr_spill_count"] == 0, v
    assert v["group_segment_fixed_size"] == LDS == 140544, v
    assert LDS <= 160 * 1024
    assert v["vgpr_count"] <= VGPR, v


def test_box_fit_kernels_kept_their_resources():
    # RansacRng moved to ransac_rng.hpp: the kernels that use it are what they were
    import kernel_resources

    res = kernel_resources.kernel_resources(LIB)
    k = next(k for k in res if "box_propagate_ransac_kernel" in k)
    v = res[k]
    assert v["private_segment_fixed_size"] == 0 and v["vgpr_spill_count"] == 0 and v["sgpr_spill_count"] == 0, v
    assert v["group_segment_fixed_size"] == 2 * 1024 * 8, v
