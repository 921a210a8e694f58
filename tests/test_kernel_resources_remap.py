"""The remap kernels exist in the built library for both pixel types, 1 to 4
channels and the interpolations each takes, and hold their resources (CPU only:
reads the gfx950 code objects' metadata, tools/kernel_resources.py): no LDS, no
scratch, no spill, and VGPR counts at what the build shows (the bounds leave no
room: a kernel that grows fails here and the bound is then set on purpose)."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
LIB = os.path.join(ROOT, "opencv_amd", "lib", "libtbdk.so")

pytestmark = pytest.mark.skipif(not os.path.exists(LIB) or not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf"),
                                reason="library or llvm-readelf missing")

# remap_kernel<T, CN, INTER>: T h = uint8_t, f = float; INTER 0 NEAREST, 1 LINEAR, 2 CUBIC (8U only)
VGPR = {("h", 0): 32, ("h", 1): 36, ("h", 2): 46, ("f", 0): 36, ("f", 1): 39}


def test_remap_kernel_instances():
    import kernel_resources

    res = kernel_resources.kernel_resources(LIB)
    ks = sorted(k for k in res if "remap_kernelI" in k)
    want = [f"remap_kernelI{t}Li{cn}ELi{inter}EE" for t in "hf" for cn in (1, 2, 3, 4)
            for inter in ((0, 1, 2) if t == "h" else (0, 1))]
    assert len(ks) == len(want) == 20, ks
    for w in want:
        k = next(k for k in ks if w in k)
        v = res[k]
        assert v["private_segment_fixed_size"] == 0 and v["vgpr_spill_count"] == 0 and v["sgpr_spill_count"] == 0, (k, v)
        assert v["group_segment_fixed_size"] == 0, (k, v)
        t, inter = w[len("remap_kernelI")], int(w[-3])
        assert v["vgpr_count"] <= VGPR[(t, inter)], (k, v)
