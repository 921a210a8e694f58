"""The identities behind the GFTT eigenvalue walk's shorter row arithmetic
(opencv_amd/csrc/gftt_row_math.hpp, the text klt_gftt.hip compiles): a
stand-alone host program, built with AddressSanitizer +
UndefinedBehaviorSanitizer.  CPU only."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_row_arithmetic_identities(tmp_path):
    """rx = s2 - s0 against the literal three-tap Sobel row for all 256^3
    (s0, s1, s2); dx, dy without the "+ 0.f", the covariances and the min
    eigenvalue against the literal form over 5 x 5 neighbourhoods of 8-bit and
    16-bit pixels (random and extreme), no -0 and no NaN among them;
    fkey(max(a, b)) == max(fkey(a), fkey(b)) over those eigenvalues; zero
    mismatches"""
    exe = str(tmp_path / "gftt_row_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-ffp-contract=off",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I", os.path.join(ROOT, "opencv_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "gftt_row_check.cpp"), "-o", exe])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "gftt row check ok" in p.stdout, p.stdout + p.stderr
