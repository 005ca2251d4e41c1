"""CPU check of the relative-pose planner (csrc/relpose_plan.cpp): tests/native/relpose_plan_check.cpp plans generated
maps (disabled observations, points seen twice in one frame, observations not grouped by frame) and recomputes the
record lists by brute force; a pair with 7 records, n = 0, the launch shape and every SG_EINVAL case of the contract.
The numpy restatement of the record rule (relpose_cases.pair_obs) is held to the same counts on C1.  The planner and
the check are built into one stand-alone program under AddressSanitizer and UBSan.  No GPU, no HIP."""
import os
import subprocess

import relpose_cases as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_relpose_planner_matches_brute_force(tmp_path):
    exe = tmp_path / "relpose_plan_check"
    csrc = os.path.join(ROOT, "slam-robot_amd", "csrc")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-Wall", "-I" + csrc, "-I" + os.path.join(ROOT, "include"), os.path.join(csrc, "relpose_plan.cpp"),
                    os.path.join(ROOT, "tests", "native", "relpose_plan_check.cpp"), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "relpose_plan_check OK" in out.stdout


def test_numpy_record_rule_on_a_point_seen_twice_and_disabled_observations():
    m = rc.base_scene("exact")
    oa, ob = rc.pair_obs(m, 4, 5)
    n = len(oa)
    m.obs_disabled[oa[0]] = 1                      # a disabled observation in a: the record goes
    oa1, ob1 = rc.pair_obs(m, 4, 5)
    assert len(oa1) == n - 1 and oa1[0] == oa[1] and ob1[0] == ob[1]
    # a point seen twice in a and twice in b: a later observation of each frame is re-pointed at record 1's point
    # (each loses a record of its own); record 1 keeps the first observation in each frame
    p = m.obs_point[oa[1]]
    assert oa[-1] > oa[1] and ob[-2] > ob[1]
    m.obs_point[oa[-1]] = p
    m.obs_point[ob[-2]] = p
    oa2, ob2 = rc.pair_obs(m, 4, 5)
    assert len(oa2) == n - 3 and oa2[0] == oa[1] and ob2[0] == ob[1]
    assert oa[-1] not in oa2 and ob[-2] not in ob2
    assert (m.obs_point[oa2] == m.obs_point[ob2]).all() and len(set(m.obs_point[oa2])) == len(oa2)
    # with the first of the two disabled, the second takes its place
    m.obs_disabled[ob[1]] = 1
    oa3, ob3 = rc.pair_obs(m, 4, 5)
    assert oa3[0] == oa[1] and ob3[0] == ob[-2]
