"""Child process of tests/test_gpu_lk_int_origin.py's trace case: run with
TBDK_LIB naming the trace build of the library (-DTBDK_LK_TRACE), it tracks the
point lists of cases 1 to 3 and prints, as one JSON line, per case and wave the
levels whose setup took the integer-origin arm (bits 56.. of word 5 of the
wave's trace record, klt_lk_multi.hip)."""
import ctypes as C
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import test_gpu_lk_int_origin as T  # noqa: E402


def main():
    from opencv_amd import klt

    ctx = klt.Context.get(0)
    lib = ctx.lib
    cap = 4096  # records of sixteen u64
    buf = torch.zeros(16 * cap, dtype=torch.int64, device="cuda")
    out = {}
    for name, case in (("interior", T.case_interior()), ("patterns", T.case_patterns()), ("edges", T.case_edges()[0])):
        a, b, pts, win, ml = case
        buf.zero_()
        torch.cuda.synchronize()
        assert lib.tbdk_probe_lk_trace(C.c_void_p(buf.data_ptr()), C.c_uint(16 * cap)) == 0
        T.run(ctx, a, b, pts, win, ml)
        n = C.c_uint()
        assert lib.tbdk_probe_lk_trace_count(C.byref(n)) == 0
        waves = (len(pts) + 64 // win - 1) // (64 // win)
        assert n.value == waves, (n.value, waves)
        rec = buf[: 16 * waves].view(-1, 16).cpu().numpy().view(np.uint64)
        assert (rec[:, 0] != 0).all() and (rec[:, 3] & np.uint64(0xFFFFFFFF) == np.arange(waves)).all()
        out[name] = [int(v) for v in (rec[:, 5] >> np.uint64(56))]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
