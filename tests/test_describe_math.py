"""CPU check of the descriptor arithmetic (csrc/describe_math.h): tests/native/describe_math_check.cpp, a stand-alone
program built under AddressSanitizer and UBSan, describes the keypoints of a file this test writes (the device cases
and the texture case of describe_cases.py on their oracle pyramids, and a constant level) with the header's plain
per-keypoint function, and its answers must equal the numpy reference exactly: status and descriptor on every
keypoint, the bin (and so the descriptor) wherever the reference's gap is 1e-9 or more, which
test_describe_reference_bounds.py shows to be every accepted keypoint of these cases.  The program also checks the disc
list, the direction table and the bin rule on known centroids.  No GPU, no HIP."""
import os
import struct
import subprocess

import numpy as np

import describe_cases as dc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cases():
    """[(pyramid level, level array)], keypoints (x, y, index of the level array), the expected answers."""
    arrays, kps, want = [], [], []
    sets = [(dc.oracle_levels(dc.device_case(nm).img, dc.device_case(nm).depth), dc.device_case(nm).xy,
             dc.device_case(nm).levels) for nm in dc.DEVICE_CASES]
    tc = dc.texture_case()
    sets.append((tc.pyr, tc.xy[:150], tc.levels[:150]))
    const = [np.full((37, 45), 0.25, dtype=np.float32)]
    sets.append((const, np.array([[20.0, 18.0], [29.4, 15.0], [14.0, 18.0]], dtype=np.float32), np.zeros(3, np.int32)))
    for pyr, xy, lv in sets:
        base = len(arrays)
        arrays += [(l, np.ascontiguousarray(a, dtype=np.float32)) for l, a in enumerate(pyr)]
        kps += [(float(x), float(y), base + int(l)) for (x, y), l in zip(xy, lv)]
        want.append(dc.reference(pyr, xy, lv))
    want = {k: np.concatenate([w[k] for w in want]) for k in want[0]}
    return arrays, kps, want


def test_describe_math_native_check(tmp_path, oracle_lib):
    exe = tmp_path / "describe_math_check"
    csrc = os.path.join(ROOT, "slam-robot_amd", "csrc")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-Wall", "-I" + csrc, "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "native", "describe_math_check.cpp"), "-o", str(exe)], check=True)
    arrays, kps, want = _cases()
    blob = [struct.pack("<i", len(arrays))]
    for l, a in arrays:
        blob += [struct.pack("<iii", l, a.shape[1], a.shape[0]), a.astype("<f4").tobytes()]
    blob.append(struct.pack("<i", len(kps)))
    blob += [struct.pack("<ffi", x, y, i) for x, y, i in kps]
    cases = tmp_path / "cases.bin"
    cases.write_bytes(b"".join(blob))
    out = subprocess.run([str(exe), str(cases)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    lines = out.stdout.strip().split("\n")
    assert lines[-1] == "describe_math_check OK" and len(lines) == len(kps) + 1
    got = [ln.split() for ln in lines[:-1]]
    status = np.array([int(g[0]) for g in got], dtype=np.int32)
    ang = np.array([int(g[1]) for g in got], dtype=np.int32)
    desc = np.array([[int(v, 16) for v in g[2:6]] for g in got], dtype=np.uint64)
    np.testing.assert_array_equal(status, want["status"])
    sure = want["gap"] >= dc.GAP
    assert sure.sum() > 400 and (status[~sure] == 0).all()
    assert (want["status"] == 1).sum() > 100 and sure[want["status"] == 1].all()
    np.testing.assert_array_equal(ang[sure], want["angle_bin"][sure])
    np.testing.assert_array_equal(desc[sure], want["desc"][sure])
    # the constant level (the last three keypoints): zero moments give bin 0, ties give no bit; the third is refused
    assert list(status[-3:]) == [0, 0, 1] and list(ang[-3:]) == [0, 0, -1] and not desc[-3:].any()
    assert (want["gap"][-3:] == np.inf).all()
    # a keypoint the reference is not sure of may differ in its bin, but then only to a neighbouring bin
    d = (ang[~sure] - want["angle_bin"][~sure]) % 32
    assert np.isin(d, (0, 1, 31)).all()
