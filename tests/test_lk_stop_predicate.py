"""The PyrLK Newton step's single-precision stopping tests (opencv_amd/csrc/lk_stop.hpp,
the text the several-points-per-wave kernels compile) against the reference's
double expressions: a stand-alone host program, built with AddressSanitizer +
UndefinedBehaviorSanitizer and without floating-point contraction.  CPU only."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_stop_predicates_equal_the_double_expressions(tmp_path):
    """|s| <= 0.01f against (double)|s| < 0.01 on every float within 64 ulp of
    +-0.01; the epsilon prefilter (q < lo true, q > hi false, else the double
    expression) against (double)ddx^2 + (double)ddy^2 <= eps2 for eps2 in
    {0, 1e-40, 1e-12, 1e-4, 0.25, 1e30, inf}: 10^7 random pairs each and pairs
    built on the boundary; zero disagreements, and the ambiguous band hit at
    least once for every finite eps2"""
    exe = str(tmp_path / "lk_stop_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "opencv_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "lk_stop_check.cpp"), "-o", exe])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "lk stop predicates ok" in p.stdout, p.stdout + p.stderr
