"""CPU check of the matchers' packed-key best / second-best rule (csrc/best2.h): tests/native/best2_check.cpp, a
stand-alone program built under AddressSanitizer and UBSan, checks exhaustively over small inputs that folding keys with
Best2Take gives (min, second min) of the set, that Best2Merge of the parts' answers equals the fold of the whole for
every split into two or three parts in every order (the order independence the kernels rely on), that ties in distance
go to the lower index, that Hamming256 equals a bit-by-bit count, and the decode and Best2ResultOk on their boundary
values.  No GPU, no HIP."""
import math
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_best2_native_check(tmp_path):
    exe = tmp_path / "best2_check"
    csrc = os.path.join(ROOT, "slam-robot_amd", "csrc")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-Wall", "-Werror", "-I" + csrc, os.path.join(ROOT, "tests", "native", "best2_check.cpp"),
                    "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    lines = out.stdout.strip().split("\n")
    assert lines[-1] == "best2_check OK"
    counts = re.match(r"folds (\d+) merges (\d+) distances (\d+)$", lines[-2])
    assert counts, out.stdout
    folds, merges, distances = map(int, counts.groups())
    # sequences of length up to 6 with k distinct keys of 7 in C(len, k) places and padding elsewhere; 3^n assignments
    # x 6 orders over the 127 subsets of up to 6 keys; 256 single-bit and 2000 random pairs
    want_folds = sum(math.comb(n, k) * math.perm(7, k) for n in range(7) for k in range(n + 1))
    assert folds == want_folds == 49294 and merges == 6 * (4 ** 7 - 3 ** 7) and distances == 2256
