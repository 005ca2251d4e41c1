"""Diagnostic: the separator hand-off of the dissected k_chol_tiles (SG_STAMP=1), cycles per launch.
Top workgroup: the wave that owns column m at the poll (the chain wave of phase m - 1).  Bottom workgroup:
thread 0, from its last phase's barrier to its flag store.  Usage: handoff_stamps.py [C2|C5] [tag]"""
import ctypes as C, os, sys
os.environ["SG_STAMP"] = "1"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "slam-robot_amd"))
from slamgpu import ba
from slamgpu.capi import default_solver_options
from slamgpu.scene import make_config
name = sys.argv[1] if len(sys.argv) > 1 else "C2"
tag = sys.argv[2] if len(sys.argv) > 2 else ""
m = make_config(name)
pa = ba.problem_from_map_frames(m, m.num_frames - 2, m.num_frames, 2.0)
g = ba.BundleAdjuster(); g.load(pa)
info = g.info()
g.begin(default_solver_options(max_num_iterations=10**6, disable_termination=1))
g.iterate(40); g.sync()
TRACE_K = 128
NW = 64 + 2 * TRACE_K * 16
buf = (C.c_ulonglong * NW)()
g.lib.sg_ba_debug_stamps.argtypes = [C.c_void_p, C.c_void_p, C.c_int32]
g.lib.sg_ba_debug_stamps(g.h, buf, NW)
top = 64 + (TRACE_K - 1) * 16
bot = top + TRACE_K * 16
nt_, nb_ = max(buf[top + 2], 1), max(buf[bot + 4], 1)
nd, ns = info["cholesky_split"], info["cholesky_separator"]
nt = (6 * (m.num_frames - 2) + 15) // 16
print("%s %s n=%d NT=%d m=%d ns=%d nd=%d launches top %d bottom %d" %
      (tag, name, 6 * (m.num_frames - 2), nt, nt - nd - ns, ns, nd, buf[top + 2], buf[bot + 4]))
print("  top chain wave: poll arrival -> match   %8.0f" % (buf[top] / nt_))
print("  top chain wave: match -> sep_merge done %8.0f" % (buf[top + 1] / nt_))
print("  bottom: start -> last phase's barrier   %8.0f  (%.0f per phase)" % (buf[bot + 5] / nb_, buf[bot + 5] / nb_ / max(nd, 1)))
for i, lab in enumerate(["tile_final + sep_write", "barrier + z' copy", "drain / release + barrier", "flag store"]):
    print("  bottom: %-30s %8.0f" % (lab, buf[bot + i] / nb_))
print("  bottom: hand-off total                  %8.0f" % (sum(buf[bot:bot + 4]) / nb_))
