"""The wide GFTT selection's kernels exist in the built library and hold their
resources (CPU only: reads the gfx950 code objects' metadata,
tools/kernel_resources.py): no scratch memory and no spills, VGPR or SGPR; the gather
kernels use no LDS; the partition kernel's LDS is its 2048 bucket counters; the walk kernel's LDS is its 4096-key chunk, the 2048 bucket
ends, the radix histogram and a few words, and it stays within 128 VGPRs, so its 512-thread
workgroup (two waves per SIMD) leaves room for a second one, or for the waves
of other kernels, on the same CU (whole-frame GFTT)."""
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


def test_gather_instances(res):
    ks = sorted(k for k in res if "gftt_wide_gather_kernel" in k)
    # <masked>
    assert len(ks) == 2 and all(any(f"gftt_wide_gather_kernelILb{m}E" in k for k in ks) for m in (0, 1)), ks
    for k in ks:
        v = res[k]
        assert v["private_segment_fixed_size"] == 0 and v["vgpr_spill_count"] == 0 and v["sgpr_spill_count"] == 0, (k, v)
        assert v["group_segment_fixed_size"] == 0, (k, v)
        assert v["vgpr_count"] <= 64, (k, v)


def test_partition_kernel(res):
    ks = [k for k in res if "gftt_wide_partition_kernel" in k]
    assert len(ks) == 1, ks
    v = res[ks[0]]
    assert v["private_segment_fixed_size"] == 0 and v["vgpr_spill_count"] == 0 and v["sgpr_spill_count"] == 0, v
    assert 2048 * 4 <= v["group_segment_fixed_size"] <= 2048 * 4 + 64, v  # the bucket counters, the waves' sums
    assert v["vgpr_count"] <= 64, v


def test_walk_kernel(res):
    ks = [k for k in res if "gftt_wide_walk_kernel" in k]
    assert len(ks) == 1, ks
    v = res[ks[0]]
    assert v["private_segment_fixed_size"] == 0 and v["vgpr_spill_count"] == 0 and v["sgpr_spill_count"] == 0, v
    # lk[4096] + pos[2048] + hist[256] + a few words: 42,016 bytes as built
    assert 4096 * 8 + 2048 * 4 + 256 * 4 <= v["group_segment_fixed_size"] <= 4096 * 8 + 2048 * 4 + 256 * 4 + 128, v
    assert v["vgpr_count"] <= 128, v  # 98 as built; the kernel asks for four waves per SIMD
