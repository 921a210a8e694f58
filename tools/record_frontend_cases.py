#!/usr/bin/env python3
"""Records the real cv::cvtColor / cv::resize(INTER_LINEAR) on the cases of
tests/golden/frontend_cases.npz through tools/frontend_driver.cpp (how to build
it: tools/record_frontend_cases.md).

    python tools/record_frontend_cases.py /path/to/frontend_driver [out.npz]

The inputs are tests/_frontend_oracle.pattern(w, h, cn, seed) images and are not
stored.  Outputs are stored whole where they are small; a large output is
stored as one CRC-32 per row (the fixture's limit is 256 KB).  Nothing in the
test suite runs this; the fixture is committed."""
import os
import subprocess
import sys
import tempfile
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _frontend_oracle as F  # noqa: E402

CVT_SIZES = [(97, 61), (6, 5)]
# (sw, sh, dw, dh, channel counts, channel counts stored whole)
RESIZE_CASES = [
    (97, 61, 31, 20, (1, 3, 4), (1, 3, 4)),
    (50, 40, 123, 77, (1, 3, 4), (1, 3, 4)),
    (400, 300, 320, 240, (1, 3, 4), (1,)),
    (64, 48, 32, 24, (1, 3, 4), (1, 3, 4)),   # both scales exactly 2: INTER_AREA
    (33, 7, 32, 7, (1, 3, 4), (1, 3, 4)),
    (5, 5, 9, 3, (1, 3, 4), (1, 3, 4)),
    (640, 480, 610, 457, (1,), ()),
    (1242, 375, 621, 188, (1, 3), ()),        # x scale exactly 2, y not
    (40, 30, 40, 30, (3,), (3,)),             # equal sizes: a copy
    (2, 2, 7, 5, (1,), (1,)),
    (31, 1, 13, 4, (4,), (4,)),
]


def row_crcs(a):
    return np.array([zlib.crc32(np.ascontiguousarray(r).tobytes()) for r in a], np.uint32)


def run(driver, tmp, kind, img, *args):
    h, w = img.shape[:2]
    cn = 1 if img.ndim == 2 else img.shape[2]
    pin, pout = os.path.join(tmp, "in.raw"), os.path.join(tmp, "out.raw")
    np.ascontiguousarray(img).tofile(pin)
    subprocess.run([driver, kind, pin, str(w), str(h), str(cn), *map(str, args), pout], check=True)
    return np.fromfile(pout, np.uint8)


def main():
    driver = sys.argv[1]
    out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "tests", "golden", "frontend_cases.npz")
    arrays, cvt_meta, rs_meta = {}, [], []
    with tempfile.TemporaryDirectory() as tmp:
        for w, h in CVT_SIZES:
            for code in sorted(F.SRC_CN):
                i, seed = len(cvt_meta), 100 + len(cvt_meta)
                img = F.pattern(w, h, F.SRC_CN[code], seed)
                arrays[f"cvt_{i}"] = run(driver, tmp, "cvt", img, code).reshape(h, w, -1).squeeze()
                cvt_meta.append((w, h, code, seed))
        for sw, sh, dw, dh, cns, whole in RESIZE_CASES:
            for cn in cns:
                i, seed = len(rs_meta), 200 + len(rs_meta)
                img = F.pattern(sw, sh, cn, seed)
                res = run(driver, tmp, "resize", img, dw, dh).reshape(dh, dw * cn)
                full = cn in whole
                arrays[f"rs_{i}"] = res if full else row_crcs(res)
                rs_meta.append((sw, sh, cn, dw, dh, seed, int(full)))
    np.savez_compressed(out, cvt_meta=np.array(cvt_meta, np.int32), rs_meta=np.array(rs_meta, np.int32), **arrays)
    print(f"{out}: {len(cvt_meta)} cvtColor + {len(rs_meta)} resize cases, {os.path.getsize(out)} bytes")
    assert os.path.getsize(out) <= 256 * 1024


if __name__ == "__main__":
    main()
