"""Times asd_fuse_apply (wall, call to return, through a prepared ctypes call, apply = 0, mode 0) for 200 / 1000 / 4000 live keyframes of
2000 keypoints, and the same rule in C++ over flat host tables (asd-slam_amd/host/fuse_apply.hpp through tools/fuse_apply_cpu.cpp, -O2,
one thread, the observer lists handed over for free) on the same box.  Writes profiles/fuse_apply_times.json.

    python tools/fuse_apply_times.py [--sizes 200,1000,4000] [--reps 200] [--out profiles/fuse_apply_times.json]

The map is the trajectory of tools/culling_times.py: keyframe k sees 1400 of the 2500 points around point 125 k.  Two calls into the
middle keyframe: `neighbour` -- 2000 candidates (the row of a keyframe as SearchInNeighbors hands it to a target), of which about 300
carry a best_idx; `current` -- 16 000 candidates (vpFuseCandidates gathered from the nearest keyframes outwards until the list is full),
every tenth of those the keyframe does not hold carrying one.  The outputs of the library and of the host program are compared through a checksum."""
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
    for k in range(n_kf):
        rows[k, rng.choice(N_KP, 1400, replace=False)] = 125 * k + rng.choice(2500, 1400, replace=False)
    return rows, n_rows


def make_call(rows, mid, kind, seed):
    """-> (cand, best_idx) for the keyframe with index mid"""
    rng = np.random.default_rng(seed)
    in_kf = set(int(p) for p in rows[mid] if p >= 0)
    if kind == "neighbour":
        cand = rows[mid + 1].copy()                                  # a neighbour's GetMapPointMatches(), -1 included
        share = 300.0 / max(1, sum(1 for p in cand if p >= 0 and int(p) not in in_kf))
    else:
        seen, cand = set(), []
        for k in [mid + s * d for d in range(1, mid) for s in (-1, 1)]:   # vpFuseCandidates: the neighbours' points at their first occurrence,
            if len(cand) >= 16000:                                       # nearest keyframes first, until the list is full
                break
            for p in rows[k]:
                if p >= 0 and int(p) not in seen:
                    seen.add(int(p)); cand.append(int(p))
        cand = np.array(cand[:16000], np.int32)
        share = 0.1
    best = np.full(len(cand), -1, np.int32)
    for i, p in enumerate(cand):
        if p >= 0 and int(p) not in in_kf and rng.uniform() < share:
            best[i] = int(rng.integers(0, N_KP))
    return cand.astype(np.int32), best


def checksum(o):
    cs = 0
    for i in range(len(o["action"])):
        v = int(o["action"][i]) + 3 * (int(o["other"][i]) + 2) + 7 * int(o["n_moved"][i]) + 11 * int(o["n_dropped"][i]) + 13 * int(o["obs_cand"][i]) + 17 * int(o["obs_other"][i])
        cs = (cs + v % 2147483647 * (i % 97 + 1)) % 2147483647
    return cs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="200,1000,4000")
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fuse_apply_times.json"))
    a = ap.parse_args()
    pkg = entry.load_package()
    exe = os.path.join(ROOT, "tools", "fuse_apply_cpu")
    if not os.path.exists(exe):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-o", exe, exe + ".cpp"])
    import torch
    res = dict(device=torch.cuda.get_device_name(0), host=platform.processor() or platform.machine(), keypoints=N_KP, reps=a.reps, apply=0, mode=0, cases=[])
    hip = pkg.AsdHip(n_features=2000, max_width=1241, max_height=376, max_patches=4096)
    try:
        for n_kf in (int(s) for s in a.sizes.split(",")):
            rows, n_rows = make_map(n_kf, n_kf)
            hip.map_clear()
            for k in range(n_kf):
                hip.map_put(k + 1, rows[k])
            mid = n_kf // 2
            for kind in ("neighbour", "current"):
                cand, best = make_call(rows, mid, kind, 7)
                out = hip.fuse_apply(mid + 1, cand, best, 0, False)  # warm-up: code objects, every buffer at its final size
                for _ in range(10):
                    hip.fuse_apply(mid + 1, cand, best, 0, False)
                n = len(cand)
                act = np.empty(n, np.uint8)
                oth, oc, oo, mv, dr = (np.empty(n, np.int32) for _ in range(5))
                args = pkg.capi.asd_fuse_apply_args()
                args.kf, args.mode, args.n, args.cand, args.best_idx, args.apply = mid + 1, 0, n, cand.ctypes.data, best.ctypes.data, 0
                args.action, args.other, args.obs_cand, args.obs_other = act.ctypes.data, oth.ctypes.data, oc.ctypes.data, oo.ctypes.data
                args.n_moved, args.n_dropped = mv.ctypes.data, dr.ctypes.data
                t = []
                for _ in range(a.reps):
                    t0 = time.perf_counter()
                    rc = hip.lib.asd_fuse_apply(hip.ctx, C.byref(args))
                    t1 = time.perf_counter()
                    assert rc == 0, hip.last_error()
                    t.append((t1 - t0) * 1e3)
                got = dict(action=act, other=oth, obs_cand=oc, obs_other=oo, n_moved=mv, n_dropped=dr)
                cs = checksum(got)
                assert cs == checksum(out) and args.n_fused == out["n_fused"]
                with tempfile.TemporaryDirectory() as tmp:
                    path = os.path.join(tmp, "map.bin")
                    with open(path, "wb") as f:
                        f.write(np.array([n_kf, N_KP, n_rows, mid, 0, n], "<i4").tobytes())
                        f.write(rows.astype("<i4").tobytes() + cand.astype("<i4").tobytes() + best.astype("<i4").tobytes())
                    cpu = json.loads(subprocess.check_output([exe, path, str(a.reps)]).decode())
                steps = int(((act >= 1) & (act <= 3)).sum())
                res["cases"].append(dict(
                    keyframes=n_kf, table_entries=int(n_kf) * N_KP, call=kind, candidates=n, with_best_idx=int((best >= 0).sum()), steps=steps,
                    added=int((act == 1).sum()), replaced=int(((act == 2) | (act == 3)).sum()), moved=int(mv.sum()), dropped=int(dr.sum()),
                    fuse_apply_ms_median=float(np.median(t)), fuse_apply_ms_p90=float(np.percentile(t, 90)), fuse_apply_ms_min=float(np.min(t)),
                    host_fuse_apply_ms_median=cpu["fuse_ms"],
                    outputs_agree=cpu["checksum"] == cs and cpu["n_fused"] == int(args.n_fused) and cpu["steps"] == steps))
                print(json.dumps(res["cases"][-1]), flush=True)
    finally:
        hip.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
