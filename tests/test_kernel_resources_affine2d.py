"""The estimateAffine2D kernel and the device-matrix warpAffine kernels exist in
the built library and hold their resources (CPU only: reads the gfx950 code
objects' metadata, tools/kernel_resources.py): no scratch, no spill, LDS at the
figure DESIGN.md §5 "estimateAffine2D" derives, and the register counts at what
the build shows (a kernel that grows fails here and the bound is then set on
purpose)."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
LIB = os.path.join(ROOT, "opencv_amd", "lib", "libtbdk.so")

pytestmark = pytest.mark.skipif(not os.path.exists(LIB) or not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf"),
                                reason="library or llvm-readelf missing")


def lds(nparams):
    """4096 pairs (2 x 32 KB), four error strips of 4096 floats, 64 models of 6 doubles, one solver column of 135
    doubles, the LM sums (K doubles) and the four waves' partial sums (4 K), one exchange double per parameter, 64
    scores and 4 wave counts"""
    k = nparams * (nparams + 1) // 2 + nparams + 2
    return 2 * 4096 * 8 + 4 * 4096 * 4 + 64 * 6 * 8 + 135 * 8 + k * 8 + 4 * k * 8 + nparams * 8 + 64 * 4 + 4 * 4


# model points -> (LM parameters, VGPRs the build shows)
INSTANCES = {3: (6, 240), 2: (4, 156)}


@pytest.mark.parametrize("mp", sorted(INSTANCES))
def test_estimate_affine2d_kernel(mp):
    import kernel_resources

    nparams, vgpr = INSTANCES[mp]
    res = kernel_resources.kernel_resources(LIB)
    ks = [k for k in res if f"estimate_affine2d_kernelILi{mp}E" in k]
    assert len(ks) == 1, ks
    assert len([k for k in res if "estimate_affine2d_kernel" in k]) == len(INSTANCES)
    v = res[ks[0]]
    assert v["private_segment_fixed_size"] == 0 and v["vgpr_spill_count"] == 0 and v["sgpr_spill_count"] == 0, v
    # the 6-parameter instance carries 8 bytes of alignment padding between its arrays
    pad = {3: 8, 2: 0}[mp]
    assert v["group_segment_fixed_size"] == lds(nparams) + pad == {3: 136712, 2: 136168}[mp], v
    assert lds(nparams) <= 160 * 1024
    assert v["vgpr_count"] <= vgpr, v


def test_warp_affine_dev_kernels():
    import kernel_resources

    res = kernel_resources.kernel_resources(LIB)
    ks = [k for k in res if "warp_affine_dev_kernel" in k]
    assert len(ks) == 3, ks  # NEAREST, LINEAR, CUBIC
    for k in ks:
        v = res[k]
        assert v["private_segment_fixed_size"] == 0 and v["vgpr_spill_count"] == 0 and v["sgpr_spill_count"] == 0, v
        assert v["group_segment_fixed_size"] == 0, v
    # the host-matrix kernels are what they were
    assert len([k for k in res if "warp_affine_kernel" in k]) == 3
