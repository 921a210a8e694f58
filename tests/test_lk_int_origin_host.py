"""The PyrLK level setup for integer window origins (opencv_amd/csrc/lk_int_origin.hpp,
the text the several-points-per-wave kernels compile) against calcSharrDeriv
followed by the general setup's bilinear with the weights (16384, 0, 0, 0): a
stand-alone host program, built with AddressSanitizer +
UndefinedBehaviorSanitizer.  CPU only."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_int_origin_column_equals_scharr_then_bilinear(tmp_path):
    """ic / packed I pairs / gxk / gyk of a window column for window heights
    7 .. 31 (odd and even): all 512 3 x 3 neighbourhoods from {0, 255} (the
    +-4080 extremes and the modulo-2^16 wrap), 0/255 stripes and checkerboards
    over the whole column, 2 * 10^5 random columns; the two shift identities
    for every I in 0..255 and every v in [-4080, 4080]; zero mismatches"""
    exe = str(tmp_path / "lk_int_origin_check")
    subprocess.check_call(["g++", "-O0", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "opencv_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "lk_int_origin_check.cpp"), "-o", exe])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "lk int origin ok" in p.stdout, p.stdout + p.stderr
