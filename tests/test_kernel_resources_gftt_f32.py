"""The 16U / 32F GFTT kernels exist in the built library and hold their
resources (CPU only: reads the gfx950 code objects' metadata,
tools/kernel_resources.py): the eigenvalue walk's eight instances (compact /
dense x masked / unmasked x 16U / 32F) and the two covariance kernels of the
generic response, under names of their own, with no scratch and no spill; the
eigenvalue walk keeps the 8-bit kernels' LDS."""
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


def clean(res, k):
    v = res[k]
    assert v["private_segment_fixed_size"] == 0 and v["vgpr_spill_count"] == 0 and v["sgpr_spill_count"] == 0, (k, v)


def test_eigenvalue_walk_instances(res):
    ks = sorted(k for k in res if "gftt_eigpx_kernel" in k)
    # <compact, masked, pix>: pix 1 = TBDK_PIX_U16, 2 = TBDK_PIX_F32
    want = sorted(f"gftt_eigpx_kernelILb{c}ELb{m}ELi{p}E" for c in (0, 1) for m in (0, 1) for p in (1, 2))
    assert len(ks) == 8 and all(any(w in k for k in ks) for w in want), ks
    u8 = [k for k in res if "gftt_eig_kernelILb1E" in k]
    assert len(u8) == 1 and not any("gftt_eig_kernel" in k or "gftt_eig_masked_kernel" in k for k in ks)
    for k in ks:
        clean(res, k)
        assert res[k]["group_segment_fixed_size"] == res[u8[0]]["group_segment_fixed_size"], (k, res[k])


def test_covariance_instances(res):
    ks = [k for k in res if "gftt_resp_covpx_kernel" in k]
    assert len(ks) == 2, ks
    for k in ks:
        clean(res, k)
        assert res[k]["group_segment_fixed_size"] == 0
