"""The morphology and connected-component kernels exist in the built library and hold their resources (CPU only:
reads the gfx950 code objects' metadata, tools/kernel_resources.py): no private segment, no spills, LDS and VGPRs
at what the build shows (a kernel that grows fails here and the bound is then set on purpose).  The morphology
kernel's LDS is its 64 x 16 tile plus a 30-pixel halo each way, in bytes; the scans' is one word per wave, the relabel kernel's its table of 128 labels' sums."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
LIB = os.path.join(ROOT, "opencv_amd", "lib", "libtbdk.so")

pytestmark = pytest.mark.skipif(not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf"),
                                reason="llvm-readelf missing")

# kernel -> (VGPRs, LDS bytes) the build shows
KERNELS = {
    "morph_kernelILb0EE": (16, (64 + 30) * (16 + 30)), "morph_kernelILb1EE": (16, (64 + 30) * (16 + 30)),
    "cc_init_kernel": (16, 0), "cc_merge_kernel": (14, 0), "cc_compress_kernel": (12, 0), "cc_flag_kernel": (4, 0),
    "cc_reduce_kernel": (38, 64), "cc_scan_tiles_kernel": (49, 64), "cc_scan_kernel": (28, 64),
    "cc_relabel_kernel": (32, 128 * 4 + 128 * 40), "cc_finish_kernel": (18, 0),
}


@pytest.fixture(scope="module")
def res():
    import kernel_resources

    assert os.path.exists(LIB), "the library is not built"
    return {k: v for k, v in kernel_resources.kernel_resources(LIB).items() if "morph_kernel" in k or "cc_" in k}


@pytest.mark.parametrize("name", sorted(KERNELS))
def test_kernel(res, name):
    ks = [n for n in res if name in n]
    assert len(ks) == 1, ks
    v = res[ks[0]]
    assert v["private_segment_fixed_size"] == 0 and v["vgpr_spill_count"] == 0 and v["sgpr_spill_count"] == 0, v
    vgpr, lds = KERNELS[name]
    assert v["vgpr_count"] <= vgpr and v["group_segment_fixed_size"] == lds, v


def test_no_other_kernel_arrived(res):
    assert len(res) == len(KERNELS), sorted(res)
