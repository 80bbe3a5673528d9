"""Times asd_update_local_map and asd_map_shared_counts (wall, call to return, through a prepared ctypes call) for 200 / 1000 / 4000
live keyframes of 2000 keypoints with a 2000-keypoint frame, and the same steps restated in C++ on the host over flat tables
(tools/local_map_cpu.cpp, -O2, one thread) as the only available comparison.  Writes profiles/local_map_times.json.

    python tools/local_map_times.py [--sizes 200,1000,4000] [--reps 200] [--out profiles/local_map_times.json]

The lists of the library and of the host program are compared through a checksum.  The map is a trajectory: keyframe k sees 1400 of the
5000 points around point 250 k, so a point has some 5-6 observations and a frame votes for some 40 keyframes."""
import argparse
import ctypes as C
import json
import os
import platform
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as entry  # noqa: E402

N_KP = 2000


def make_map(n_kf, seed):
    rng = np.random.default_rng(seed)
    n_rows = 250 * n_kf + 5000
    rows = np.full((n_kf, N_KP), -1, np.int32)
    for k in range(n_kf):
        rows[k, rng.choice(N_KP, 1400, replace=False)] = 250 * k + rng.choice(5000, 1400, replace=False)
    mid = n_kf // 2
    pool = np.unique(rows[mid - 2:mid + 3][rows[mid - 2:mid + 3] >= 0])
    cur = np.full(N_KP, -1, np.int32)
    cur[rng.choice(N_KP, 1500, replace=False)] = rng.choice(pool, 1500, replace=False)
    seen = rng.choice(pool, 60, replace=False).astype(np.int32)
    return rows, n_rows, cur, seen, mid


def links(k, n_kf):
    cov = [x for d in range(1, 6) for x in (k - d, k + d) if 0 <= x < n_kf]
    return cov[:10], ([k + 1] if k + 1 < n_kf else []), k - 1


def checksum(out, ref):
    cs = len(out["local_kfs"]) + 3 * len(out["local_rows"]) + 7 * len(out["search_rows"]) + ref
    for i, p in enumerate(out["local_rows"]):
        cs = (cs + int(p) * (i % 97 + 1)) % 2147483647
    for i, k in enumerate(out["local_kfs"]):
        cs = (cs + int(k) * (i % 89 + 1)) % 2147483647
    return cs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="200,1000,4000")
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "local_map_times.json"))
    a = ap.parse_args()
    pkg = entry.load_package()
    exe = os.path.join(ROOT, "tools", "local_map_cpu")
    if not os.path.exists(exe):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-o", exe, exe + ".cpp"])
    import torch
    res = dict(device=torch.cuda.get_device_name(0), host=platform.processor() or platform.machine(), keypoints=N_KP, reps=a.reps, sizes=[])
    hip = pkg.AsdHip(n_features=2000, max_width=1241, max_height=376, max_patches=4096)
    try:
        for n_kf in (int(s) for s in a.sizes.split(",")):
            rows, n_rows, cur, seen, mid = make_map(n_kf, n_kf)
            hip.map_clear()
            t0 = time.perf_counter()
            for k in range(n_kf):
                hip.map_put(k, rows[k])
            put_ms = (time.perf_counter() - t0) * 1e3 / n_kf
            for k in range(n_kf):
                hip.map_kf_links(k, *links(k, n_kf))
            out = hip.update_local_map(cur, seen)          # warm-up: code objects, every buffer at its final size
            for _ in range(10):
                hip.update_local_map(cur, seen)
                hip.map_shared_counts(mid)
            # the calls themselves, arguments prepared once
            prev = np.zeros(1, np.int32)
            kfs, lrows, srch = np.empty(1024, np.int32), np.empty(1 << 17, np.int32), np.empty(1 << 17, np.int32)
            args = pkg.capi.asd_local_map_args()
            args.n_cur, args.cur_rows, args.n_seen, args.seen_rows, args.n_prev, args.prev_kfs = len(cur), cur.ctypes.data, len(seen), seen.ctypes.data, 0, prev.ctypes.data
            args.max_kfs, args.kf_capacity, args.local_kfs = 80, len(kfs), kfs.ctypes.data
            args.row_capacity, args.local_rows, args.search_capacity, args.search_rows = len(lrows), lrows.ctypes.data, len(srch), srch.ctypes.data
            ck, cc, cn = np.empty(n_kf, np.int32), np.empty(n_kf, np.int32), C.c_int32(0)
            t_map, t_cnt = [], []
            for _ in range(a.reps):
                t0 = time.perf_counter()
                rc = hip.lib.asd_update_local_map(hip.ctx, C.byref(args))
                t1 = time.perf_counter()
                assert rc == 0, hip.last_error()
                t_map.append((t1 - t0) * 1e3)
                t0 = time.perf_counter()
                rc = hip.lib.asd_map_shared_counts(hip.ctx, mid, n_kf, ck.ctypes.data_as(C.c_void_p), cc.ctypes.data_as(C.c_void_p), C.byref(cn))
                t1 = time.perf_counter()
                assert rc == 0, hip.last_error()
                t_cnt.append((t1 - t0) * 1e3)
            cs = (checksum(out, out["ref_kf"]) + int((ck[:cn.value].astype(np.int64) * cc[:cn.value]).sum())) % 2147483647
            with tempfile.TemporaryDirectory() as tmp:
                path = os.path.join(tmp, "map.bin")
                with open(path, "wb") as f:
                    f.write(np.array([n_kf, N_KP, n_rows, len(cur), len(seen), mid], "<i4").tobytes())
                    f.write(rows.astype("<i4").tobytes() + cur.astype("<i4").tobytes() + seen.astype("<i4").tobytes())
                cpu = json.loads(subprocess.check_output([exe, path, str(a.reps)]).decode())
            res["sizes"].append(dict(
                keyframes=n_kf, table_entries=int(n_kf) * N_KP, local_kfs=len(out["local_kfs"]), local_points=len(out["local_rows"]),
                search_points=len(out["search_rows"]), shared_keyframes=int(cn.value), map_put_ms_per_keyframe=put_ms,
                update_local_map_ms_median=float(np.median(t_map)), update_local_map_ms_p90=float(np.percentile(t_map, 90)),
                update_local_map_ms_min=float(np.min(t_map)), shared_counts_ms_median=float(np.median(t_cnt)),
                shared_counts_ms_p90=float(np.percentile(t_cnt, 90)), host_update_local_map_ms_median=cpu["update_local_map_ms"],
                host_shared_counts_ms_median=cpu["shared_counts_ms"], lists_agree=cpu["checksum"] == cs and cpu["n_local"] == len(out["local_rows"])))
            print(json.dumps(res["sizes"][-1]), flush=True)
    finally:
        hip.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
