"""Times asd_keyframe_culling (wall, call to return, through a prepared ctypes call, apply = 0) for 200 / 1000 / 4000 live keyframes of
2000 keypoints with 1, 30 and 100 candidates, and the same step restated in C++ on the host over flat tables (tools/culling_cpu.cpp,
-O2, one thread) as the only available comparison.  Writes profiles/culling_times.json.

    python tools/culling_times.py [--sizes 200,1000,4000] [--cands 1,30,100] [--reps 200] [--out profiles/culling_times.json]

The outputs of the library and of the host program are compared through a checksum.  The map is a trajectory: keyframe k sees 1400 of
the 2500 points around point 125 k, so a point has some 11 observations; a keyframe's octaves are clip(b + U{-1 .. 2}, 0, 7) around a
base level b in 0 .. 4.  The candidates are the keyframes nearest to the middle one, nearest first."""
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
    n_rows = 125 * n_kf + 2500
    rows = np.full((n_kf, N_KP), -1, np.int32)
    octaves = np.zeros((n_kf, N_KP), np.uint8)
    for k in range(n_kf):
        rows[k, rng.choice(N_KP, 1400, replace=False)] = 125 * k + rng.choice(2500, 1400, replace=False)
        octaves[k] = np.clip(int(rng.integers(0, 5)) + rng.integers(-1, 3, N_KP), 0, 7)
    return rows, octaves, n_rows


def candidates(n_kf, n):
    mid = n_kf // 2
    order = [mid] + [x for d in range(1, n_kf) for x in (mid - d, mid + d) if 0 <= x < n_kf]
    return np.array(order[:n], np.int32)


def checksum(decision, n_mps, n_red, bad):
    cs = 0
    for c in range(len(decision)):
        cs = (cs + (int(decision[c] == 1) + 3 * int(n_mps[c]) + 7 * int(n_red[c])) * (c % 97 + 1)) % 2147483647
    for i, p in enumerate(bad):
        cs = (cs + int(p) * (i % 89 + 1)) % 2147483647
    return cs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="200,1000,4000")
    ap.add_argument("--cands", default="1,30,100")
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "culling_times.json"))
    a = ap.parse_args()
    pkg = entry.load_package()
    exe = os.path.join(ROOT, "tools", "culling_cpu")
    if not os.path.exists(exe):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-o", exe, exe + ".cpp"])
    import torch
    res = dict(device=torch.cuda.get_device_name(0), host=platform.processor() or platform.machine(), keypoints=N_KP, reps=a.reps, apply=0, cases=[])
    hip = pkg.AsdHip(n_features=2000, max_width=1241, max_height=376, max_patches=4096)
    try:
        for n_kf in (int(s) for s in a.sizes.split(",")):
            rows, octaves, n_rows = make_map(n_kf, n_kf)
            hip.map_clear()
            for k in range(n_kf):                              # (table ids are k + 1: id 0 is never a candidate of the reference)
                hip.map_put(k + 1, rows[k])
                hip.map_put_octaves(k + 1, octaves[k])
            for n_cand in (int(s) for s in a.cands.split(",")):
                cand0 = candidates(n_kf, n_cand)
                cand = (cand0 + 1).astype(np.int32)
                flags = np.zeros(len(cand), np.uint8)
                out = hip.keyframe_culling(cand, flags, False, bad_capacity=1 << 16)     # warm-up: code objects, every buffer at its final size
                for _ in range(10):
                    hip.keyframe_culling(cand, flags, False, bad_capacity=1 << 16)
                dec, nm, nr, bad = np.empty(len(cand), np.uint8), np.empty(len(cand), np.int32), np.empty(len(cand), np.int32), np.empty(1 << 16, np.int32)
                args = pkg.capi.asd_kf_culling_args()
                args.n_cand, args.cand, args.cand_flags, args.apply = len(cand), cand.ctypes.data, flags.ctypes.data, 0
                args.decision, args.n_mps, args.n_redundant = dec.ctypes.data, nm.ctypes.data, nr.ctypes.data
                args.bad_capacity, args.bad_rows = len(bad), bad.ctypes.data
                t = []
                for _ in range(a.reps):
                    t0 = time.perf_counter()
                    rc = hip.lib.asd_keyframe_culling(hip.ctx, C.byref(args))
                    t1 = time.perf_counter()
                    assert rc == 0, hip.last_error()
                    t.append((t1 - t0) * 1e3)
                cs = checksum(dec, nm, nr, bad[:args.n_bad])
                assert cs == checksum(out["decision"], out["n_mps"], out["n_redundant"], out["bad_rows"])
                with tempfile.TemporaryDirectory() as tmp:
                    path = os.path.join(tmp, "map.bin")
                    with open(path, "wb") as f:
                        f.write(np.array([n_kf, N_KP, n_rows, len(cand0)], "<i4").tobytes())
                        f.write(rows.astype("<i4").tobytes() + octaves.tobytes() + cand0.astype("<i4").tobytes())
                    cpu = json.loads(subprocess.check_output([exe, path, str(a.reps)]).decode())
                res["cases"].append(dict(
                    keyframes=n_kf, table_entries=int(n_kf) * N_KP, candidates=len(cand), culled=int((dec == 1).sum()), turned_bad=int(args.n_bad),
                    keyframe_culling_ms_median=float(np.median(t)), keyframe_culling_ms_p90=float(np.percentile(t, 90)),
                    keyframe_culling_ms_min=float(np.min(t)), host_keyframe_culling_ms_median=cpu["culling_ms"],
                    outputs_agree=cpu["checksum"] == cs and cpu["culled"] == int((dec == 1).sum()) and cpu["n_bad"] == int(args.n_bad)))
                print(json.dumps(res["cases"][-1]), flush=True)
    finally:
        hip.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
