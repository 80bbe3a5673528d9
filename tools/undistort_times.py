"""Cost of cv::undistort in front of the extractor at the EuRoC size (752x480, BASELINE configs[3] coefficients).

  python3 tools/undistort_times.py [--out DIR]
      1. runs `rocprofv3 --kernel-trace --stats` over this script's `kernels` mode in a child process (its own time limit) and
         reports the average k_undistort and k_copy_image times of synchronous 752x480 extractions with and without the map;
      2. pipelined asd_extract_submit frames/s (queue kept full) with and without the map, device-resident and pinned frames.
  One JSON line on stdout.  Every measured loop is preceded by an untimed warm-up.
  python3 tools/undistort_times.py kernels N      (the profiled child: N extractions with the map, N without)
"""
import csv
import ctypes as C
import glob
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as g  # noqa: E402

W, H = 752, 480
K = (458.654, 457.296, 367.215, 248.375)
D = (-0.28340811, 0.07395907, 0.00019359, 1.76187114e-05)


def _context(pkg):
    hip = pkg.AsdHip(n_features=1000, max_width=W, max_height=H, max_patches=4096)
    hip.load_weights(pkg.synth.asdnet_weights(0))
    return hip


def _frames(pkg, hip, pinned):
    out = []
    for t in range(8):
        f = pkg.synth.scene_frame(t, w=W, h=H)
        if pinned:
            p = hip.host_alloc(f.nbytes)
            C.memmove(p.value, f.ctypes.data, f.nbytes)
        else:
            p = hip.device_alloc(f.nbytes)
            hip.h2d(p, f)
        out.append(p)
    return out


def kernels(n):
    pkg = g.load_package()
    hip = _context(pkg)
    fr = _frames(pkg, hip, pinned=False)
    for with_map in (True, False):
        hip.set_undistortion(K, D if with_map else None, W, H)
        for i in range(10 + n):   # (the first ten are the warm-up; the stats cover them too, the average hardly moves)
            hip.extract_device(fr[i % 8], W, H, W)
    hip.close()


def throughput(pkg, hip, frames, pinned, n=200, depth=3):
    def run(m):
        for i in range(min(depth, m)):
            hip.extract_submit(frames[i % 8], W, H, W, device_resident=not pinned)
        t0 = time.perf_counter()
        for i in range(m):
            hip.extract_wait(view=True)
            if i + depth < m:
                hip.extract_submit(frames[(i + depth) % 8], W, H, W, device_resident=not pinned)
        return time.perf_counter() - t0
    run(30)
    return n / run(n)


def main():
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "undistort_times_out")
    os.makedirs(out, exist_ok=True)
    res = {"size": [W, H]}
    prof = os.path.join(out, "prof")
    cmd = ["timeout", "-k", "10", "300", "rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", prof, "-o", "und",
           "--", sys.executable, os.path.abspath(__file__), "kernels", "200"]
    p = subprocess.run(cmd, capture_output=True, text=True)
    if p.returncode != 0:
        print(p.stdout[-2000:], p.stderr[-3000:], file=sys.stderr)
        sys.exit(f"profiled run failed with exit status {p.returncode}")
    stats = glob.glob(os.path.join(prof, "**", "*kernel_stats.csv"), recursive=True)
    for f in glob.glob(os.path.join(prof, "**", "*kernel_trace.csv"), recursive=True):
        os.remove(f)
    for row in csv.DictReader(open(stats[0])):
        for k in ("k_undistort", "k_copy_image"):
            if f"::{k}(" in row["Name"]:
                res[f"{k}_avg_us"] = round(float(row["AverageNs"]) / 1e3, 2)
                res[f"{k}_calls"] = int(row["Calls"])
    pkg = g.load_package()
    hip = _context(pkg)
    for pinned in (False, True):
        frames = _frames(pkg, hip, pinned)
        src = "pinned" if pinned else "device"
        for with_map in (False, True):
            hip.set_undistortion(K, D if with_map else None, W, H)
            res[f"fps_{src}_{'map' if with_map else 'nomap'}"] = round(throughput(pkg, hip, frames, pinned), 1)
    hip.close()
    print(json.dumps(res))


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "kernels":
        kernels(int(sys.argv[2]))
    else:
        main()
