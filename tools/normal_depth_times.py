"""Times the write-back of a LocalBA over the resident tables -- asd_map_kf_centers for 20 keyframes, then asd_update_normal_and_depth with
Xw given (wall, first call to second return, through prepared ctypes calls) -- for 200 / 1000 / 4000 live keyframes of 2000 keypoints and
2000 / 8000 points per call, and the same rule restated in C++ on the host over flat point-major tables (tools/normal_depth_cpu.cpp, -O2,
one thread, the observer lists given for free) plus the asd_mpbank_put of its result, as the only available comparison.  Writes
profiles/normal_depth_times.json.

    python tools/normal_depth_times.py [--sizes 200,1000,4000] [--points 2000,8000] [--reps 200] [--out profiles/normal_depth_times.json]

Every table size is measured in a process of its own, under a time limit of its own (--limit seconds); the first one that fails ends the
run.  The outputs of the library and of the host program are compared through a checksum of their bit patterns.  The map is a
trajectory: keyframe k sees 1400 of the 1500 points around point 233 k, so a point has some 6 observers; the points of a call are a
contiguous run of bank rows around the middle keyframe (which lets the comparison push its result with ONE asd_mpbank_put)."""
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

N_KP, STEP, WINDOW, SEEN, N_CENTRES = 2000, 233, 1500, 1400, 20


def make_map(n_kf, seed):
    rng = np.random.default_rng(seed)
    n_rows = STEP * n_kf + WINDOW
    rows = np.full((n_kf, N_KP), -1, np.int32)
    octaves = np.zeros((n_kf, N_KP), np.uint8)
    for k in range(n_kf):
        rows[k, rng.choice(N_KP, SEEN, replace=False)] = STEP * k + rng.choice(WINDOW, SEEN, replace=False)
        octaves[k] = np.clip(int(rng.integers(0, 5)) + rng.integers(-1, 3, N_KP), 0, 7)
    # the camera moves along x; the points lie some metres in front of the keyframes that see them
    centres = np.stack([np.arange(n_kf) * 0.5, rng.uniform(-0.2, 0.2, n_kf), rng.uniform(-0.2, 0.2, n_kf)], 1).astype(np.float32)
    Xw = np.stack([np.arange(n_rows) * (0.5 / STEP) + rng.uniform(-1, 1, n_rows), rng.uniform(-8, 8, n_rows), rng.uniform(4, 40, n_rows)], 1).astype(np.float32)
    return rows, octaves, centres, Xw, n_rows


def observers(rows, octaves, first, n_pts, seed):
    """point-major lists for bank rows [first, first + n_pts): start, observers (ascending keyframe), ref index, ref keyframe, ref octave"""
    kf, kp = np.nonzero((rows >= first) & (rows < first + n_pts))          # row-major: ascending keyframe
    pt = rows[kf, kp] - first
    order = np.argsort(pt, kind="stable")
    kf, kp, pt = kf[order], kp[order], pt[order]
    start = np.zeros(n_pts + 1, np.int32)
    np.add.at(start, pt + 1, 1)
    start = np.cumsum(start).astype(np.int32)
    cnt = np.diff(start)
    assert cnt.min() >= 1
    rng = np.random.default_rng(seed)
    ref = (rng.uniform(size=n_pts) * cnt).astype(np.int32)
    at = start[:-1] + ref
    return start, kf.astype(np.int32), ref, kf[at].astype(np.int32), octaves[kf[at], kp[at]]


def checksum(normal, mn, mx):
    words = np.concatenate([normal.reshape(-1, 3), mn[:, None], mx[:, None]], 1).astype(np.float32).view(np.uint32).astype(np.int64) % 1000003
    p = np.arange(len(mn), dtype=np.int64)[:, None]
    k = np.arange(3, 8, dtype=np.int64)[None, :]
    terms = (words * ((p * 5 + k) % 89 + 1)) % 2147483647
    cs = 0
    for v in terms.ravel().tolist():
        cs = (cs + v) % 2147483647
    return cs


def run_case(n_kf, points, reps):
    """one table size, every call size; prints one JSON line per case"""
    pkg = entry.load_package()
    exe = os.path.join(ROOT, "tools", "normal_depth_cpu")
    if not os.path.exists(exe):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-o", exe, exe + ".cpp"])
    import torch
    device = torch.cuda.get_device_name(0)
    rows, octaves, centres, Xw, n_rows = make_map(n_kf, n_kf)
    hip = pkg.AsdHip(n_features=2000, max_width=1241, max_height=376, max_patches=4096)
    try:
        scale = hip.scale_tables()["scale"]
        ids = np.arange(1, n_kf + 1, dtype=np.int32)               # table ids are k + 1
        for k in range(n_kf):
            hip.map_put(int(ids[k]), rows[k])
            hip.map_put_octaves(int(ids[k]), octaves[k])
        hip.map_kf_centers(ids, centres)
        zeros = np.zeros(n_rows, np.float32)
        hip.mpbank_put(0, Xw, np.zeros((n_rows, 3), np.float32), zeros, zeros)
        hip.sync()
        mid = n_kf // 2
        for n_pts in points:
            first = max(0, min(STEP * mid - n_pts // 2 + WINDOW // 2, n_rows - n_pts))
            start, obs_kf, ref, ref_kf, ref_oct = observers(rows, octaves, first, n_pts, n_pts)
            req = np.arange(first, first + n_pts, dtype=np.int32)
            ref_ids = (ref_kf + 1).astype(np.int32)
            rng = np.random.default_rng(n_pts)
            new_Xw = (Xw[first:first + n_pts] + rng.uniform(-0.05, 0.05, (n_pts, 3))).astype(np.float32)
            near = np.arange(max(0, mid - N_CENTRES // 2), max(0, mid - N_CENTRES // 2) + min(N_CENTRES, n_kf))
            c_ids, c_val = ids[near].copy(), np.ascontiguousarray(centres[near])
            out = hip.update_normal_and_depth(req, ref_ids, new_Xw)    # warm-up: code objects, every buffer at its final size
            assert (out["status"] == 0).all()
            for _ in range(10):
                hip.map_kf_centers(c_ids, c_val)
                hip.update_normal_and_depth(req, ref_ids, new_Xw)
            normal, mn, mx = np.empty((n_pts, 3), np.float32), np.empty(n_pts, np.float32), np.empty(n_pts, np.float32)
            status = np.empty(n_pts, np.uint8)
            args = pkg.capi.asd_normal_depth_args()
            args.n, args.rows, args.ref_kf, args.Xw = n_pts, req.ctypes.data, ref_ids.ctypes.data, new_Xw.ctypes.data
            args.normal, args.min_dist, args.max_dist, args.status = normal.ctypes.data, mn.ctypes.data, mx.ctypes.data, status.ctypes.data
            p_ids, p_val = c_ids.ctypes.data_as(C.c_void_p), c_val.ctypes.data_as(C.c_void_p)
            t, t_c = [], []
            for _ in range(reps):
                t0 = time.perf_counter()
                rc0 = hip.lib.asd_map_kf_centers(hip.ctx, len(c_ids), p_ids, p_val)
                t1 = time.perf_counter()
                rc1 = hip.lib.asd_update_normal_and_depth(hip.ctx, C.byref(args))
                t2 = time.perf_counter()
                assert rc0 == 0 and rc1 == 0, hip.last_error()
                t.append((t2 - t0) * 1e3)
                t_c.append((t1 - t0) * 1e3)
            cs = checksum(normal, mn, mx)
            assert cs == checksum(out["normal"], out["min_dist"], out["max_dist"])
            # the comparison: the rule on the host, then its result through asd_mpbank_put (call to return, and with the copy waited for)
            with tempfile.TemporaryDirectory() as tmp:
                path = os.path.join(tmp, "points.bin")
                with open(path, "wb") as f:
                    f.write(np.array([n_kf, n_pts, len(obs_kf)], "<i4").tobytes())
                    f.write(centres.astype("<f4").tobytes() + new_Xw.astype("<f4").tobytes() + start.astype("<i4").tobytes())
                    f.write(obs_kf.astype("<i4").tobytes() + ref.astype("<i4").tobytes())
                    f.write(scale[ref_oct].astype("<f4").tobytes() + np.float32(scale[-1]).tobytes())
                cpu = json.loads(subprocess.check_output([exe, path, str(reps)]).decode())
            t_put, t_put_sync = [], []
            for _ in range(reps):
                t0 = time.perf_counter()
                hip.mpbank_put(first, new_Xw, normal, mn, mx)
                t1 = time.perf_counter()
                hip.sync()
                t2 = time.perf_counter()
                t_put.append((t1 - t0) * 1e3)
                t_put_sync.append((t2 - t0) * 1e3)
            case = dict(
                device=device, keyframes=n_kf, table_entries=int(n_kf) * N_KP, points=n_pts, observations=int(len(obs_kf)),
                observers_mean=float(len(obs_kf)) / n_pts, centres_per_call=int(len(c_ids)),
                write_back_ms_median=float(np.median(t)), write_back_ms_p90=float(np.percentile(t, 90)), write_back_ms_min=float(np.min(t)),
                kf_centers_ms_median=float(np.median(t_c)),
                host_update_ms_median=cpu["update_ms"], host_mpbank_put_ms_median=float(np.median(t_put)),
                host_mpbank_put_synced_ms_median=float(np.median(t_put_sync)),
                host_total_ms_median=cpu["update_ms"] + float(np.median(t_put)),
                outputs_agree=cpu["checksum"] == cs)
            print(json.dumps(case), flush=True)
    finally:
        hip.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="200,1000,4000")
    ap.add_argument("--points", default="2000,8000")
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--limit", type=int, default=240, help="seconds one table size may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "normal_depth_times.json"))
    ap.add_argument("--case", type=int, default=0, help="internal: measure this table size in this process")
    a = ap.parse_args()
    points = [int(s) for s in a.points.split(",")]
    if a.case:
        run_case(a.case, points, a.reps)
        return
    res = dict(host=platform.processor() or platform.machine(), keypoints=N_KP, reps=a.reps, cases=[])
    for n_kf in (int(s) for s in a.sizes.split(",")):
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--case", str(n_kf), "--points", a.points, "--reps", str(a.reps)],
                           capture_output=True, text=True, timeout=a.limit)
        if r.returncode != 0:                                       # nothing more is started on the device after a failure
            sys.stderr.write(r.stdout + r.stderr)
            raise SystemExit(f"table size {n_kf} failed with status {r.returncode}")
        for line in r.stdout.splitlines():
            if line.startswith("{"):
                case = json.loads(line)
                res["device"] = case.pop("device")
                res["cases"].append(case)
                print(json.dumps(case), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
