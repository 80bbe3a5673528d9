"""Times asd_local_ba_graph (with Xw) and asd_local_ba_apply over the resident observation table -- wall, call to return, through prepared
ctypes calls, median of --reps -- for 200 / 1000 / 4000 live keyframes of 2000 keypoints with 20 and 100 neighbours, and the same two
steps restated in C++ on the host over flat tables (tools/local_ba_graph_cpu.cpp, -O2, one thread, the observation lists given for free),
as the only available comparison.  Writes profiles/local_ba_graph_times.json.

    python tools/local_ba_graph_times.py [--sizes 200,1000,4000] [--neigh 20,100] [--reps 200] [--out profiles/local_ba_graph_times.json]

Every table size is measured in a process of its own, under a time limit of its own (--limit seconds); the first one that fails ends the
run.  The lists of the library and of the host program are compared through a checksum.  The map is the trajectory of
tools/normal_depth_times.py: keyframe k sees 1400 of the 1500 points around point 233 k, so a point has some 6 observers; the keyframe is
the middle one, its neighbours the nearest ids on both sides in a shuffled order; every 20th edge is flagged.  asd_local_ba_apply is timed
with apply = 0 (apply = 1 consumes the graph, so it cannot be repeated without a graph call): the pass that writes the table is not in
that number; one apply = 1 call per case is timed on its own as apply_once_ms."""
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

N_KP, STEP, WINDOW, SEEN = 2000, 233, 1500, 1400


def make_map(n_kf, seed):
    rng = np.random.default_rng(seed)
    n_rows = STEP * n_kf + WINDOW
    rows = np.full((n_kf, N_KP), -1, np.int32)
    octaves = np.zeros((n_kf, N_KP), np.uint8)
    for k in range(n_kf):
        rows[k, rng.choice(N_KP, SEEN, replace=False)] = STEP * k + rng.choice(WINDOW, SEEN, replace=False)
        octaves[k] = np.clip(int(rng.integers(0, 5)) + rng.integers(-1, 3, N_KP), 0, 7)
    kf_bad = (rng.uniform(size=n_kf) < 0.02).astype(np.uint8)
    pt_bad = (rng.uniform(size=n_rows) < 0.02).astype(np.uint8)
    Xw = rng.uniform(-40, 40, (n_rows, 3)).astype(np.float32)
    return rows, octaves, kf_bad, pt_bad, Xw, n_rows


def checksum(lists):
    v = np.concatenate([np.asarray(x, np.int64).ravel() for x in lists]) if lists else np.zeros(0, np.int64)
    i = np.arange(len(v), dtype=np.int64)
    terms = (((v + 1) % 1000003) * (i % 89 + 1)) % 2147483647
    cs = 0
    for t in terms.tolist():
        cs = (cs + t) % 2147483647
    return cs


def run_case(n_kf, neighs, reps):
    """one table size, every neighbour count; prints one JSON line per case"""
    pkg = entry.load_package()
    exe = os.path.join(ROOT, "tools", "local_ba_graph_cpu")
    if not os.path.exists(exe):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-o", exe, exe + ".cpp"])
    import torch
    device = torch.cuda.get_device_name(0)
    rows, octaves, kf_bad, pt_bad, Xw, n_rows = make_map(n_kf, n_kf)
    mid = n_kf // 2
    kf_bad[mid] = 0
    hip = pkg.AsdHip(n_features=2000, max_width=1241, max_height=376, max_patches=4096)
    try:
        for k in range(n_kf):                                       # table ids are k + 1
            hip.map_put(k + 1, rows[k])
            hip.map_put_octaves(k + 1, octaves[k])
            if kf_bad[k]:
                hip.map_kf_bad(k + 1, True)
        hip.map_point_bad(np.nonzero(pt_bad)[0], True)
        zeros = np.zeros(n_rows, np.float32)
        hip.mpbank_put(0, Xw, np.zeros((n_rows, 3), np.float32), zeros, zeros)
        hip.sync()
        for n_neigh in neighs:
            rng = np.random.default_rng(n_neigh)
            near = sorted((k for k in range(n_kf) if k != mid), key=lambda k: (abs(k - mid), k))[:min(n_neigh, n_kf - 1)]
            neigh = rng.permutation(near).astype(np.int32)
            g = hip.local_ba_graph(mid + 1, neigh + 1, want_Xw=True)        # warm-up: code objects, every buffer at its final size
            P, E = len(g["local_rows"]), len(g["e_kf"])
            caps = (len(g["local_kfs"]), P, len(g["fixed_kfs"]), len(g["pose_kfs"]), E)
            flags = (np.arange(E) % 20 == 7).astype(np.uint8)
            dry = hip.local_ba_apply(flags, P, apply=False, bad_capacity=P)
            # prepared calls
            i32 = lambda n: np.zeros(max(n, 1), np.int32)
            bufs = dict(kfs=i32(caps[0]), rows=i32(P), rank=i32(P), fixed=i32(caps[2]), pose=i32(caps[3]), pfix=np.zeros(max(caps[3], 1), np.uint8),
                        ep=i32(E), eq=i32(E), ek=i32(E), ei=i32(E), eo=np.zeros(max(E, 1), np.uint8), xw=np.zeros((max(P, 1), 3)))
            ids = (neigh + 1).astype(np.int32)
            a = pkg.capi.asd_ba_graph_args()
            a.kf, a.n_neigh, a.neigh = mid + 1, len(ids), ids.ctypes.data
            a.kf_capacity, a.local_kfs = caps[0], bufs["kfs"].ctypes.data
            a.point_capacity, a.local_rows, a.point_rank = P, bufs["rows"].ctypes.data, bufs["rank"].ctypes.data
            a.fixed_capacity, a.fixed_kfs = caps[2], bufs["fixed"].ctypes.data
            a.pose_capacity, a.pose_kfs, a.pose_fixed = caps[3], bufs["pose"].ctypes.data, bufs["pfix"].ctypes.data
            a.edge_capacity, a.e_point, a.e_pose, a.e_kf, a.e_idx, a.e_octave = (E, bufs["ep"].ctypes.data, bufs["eq"].ctypes.data, bufs["ek"].ctypes.data,
                                                                                 bufs["ei"].ctypes.data, bufs["eo"].ctypes.data)
            a.Xw = bufs["xw"].ctypes.data
            bad, new_ref = i32(P), i32(P)
            b = pkg.capi.asd_ba_apply_args()
            b.n_edges, b.erase, b.apply, b.bad_capacity, b.bad_rows, b.n_points, b.new_ref = E, flags.ctypes.data, 0, P, bad.ctypes.data, P, new_ref.ctypes.data
            for _ in range(10):
                assert hip.lib.asd_local_ba_graph(hip.ctx, C.byref(a)) == 0 and hip.lib.asd_local_ba_apply(hip.ctx, C.byref(b)) == 0, hip.last_error()
            t_g, t_a = [], []
            for _ in range(reps):
                t0 = time.perf_counter()
                rc0 = hip.lib.asd_local_ba_graph(hip.ctx, C.byref(a))
                t1 = time.perf_counter()
                rc1 = hip.lib.asd_local_ba_apply(hip.ctx, C.byref(b))
                t2 = time.perf_counter()
                assert rc0 == 0 and rc1 == 0, hip.last_error()
                t_g.append((t1 - t0) * 1e3)
                t_a.append((t2 - t1) * 1e3)
            cs_g = checksum([g[k] for k in ("local_kfs", "local_rows", "fixed_kfs", "pose_kfs", "pose_fixed", "point_rank")] +
                            [np.stack([g[k].astype(np.int64) for k in ("e_point", "e_pose", "e_kf", "e_idx", "e_octave")], 1)])
            cs_a = checksum([[dry["n_erased"]], dry["bad_rows"], dry["new_ref"]])
            assert cs_g == checksum([bufs["kfs"][:caps[0]], bufs["rows"][:P], bufs["fixed"][:caps[2]], bufs["pose"][:caps[3]], bufs["pfix"][:caps[3]], bufs["rank"][:P],
                                     np.stack([bufs[k][:E].astype(np.int64) for k in ("ep", "eq", "ek", "ei", "eo")], 1)])
            with tempfile.TemporaryDirectory() as tmp:
                path = os.path.join(tmp, "map.bin")
                with open(path, "wb") as f:
                    f.write(np.array([n_kf, N_KP, n_rows, mid, len(neigh)], "<i4").tobytes())
                    f.write(rows.astype("<i4").tobytes() + octaves.tobytes() + kf_bad.tobytes() + pt_bad.tobytes() + neigh.astype("<i4").tobytes())
                cpu = json.loads(subprocess.check_output([exe, path, str(reps)]).decode())
            # one apply = 1: the table changes, so it is the last thing this case does, and the rows are put back behind it
            b.apply = 1
            t0 = time.perf_counter()
            rc = hip.lib.asd_local_ba_apply(hip.ctx, C.byref(b))
            t_once = (time.perf_counter() - t0) * 1e3
            assert rc == 0, hip.last_error()
            case = dict(device=device, keyframes=n_kf, table_entries=int(n_kf) * N_KP, neighbours=int(len(neigh)), local_keyframes=caps[0], points=P,
                        fixed_keyframes=caps[2], poses=caps[3], edges=E, erased=int(dry["n_erased"]), turned_bad=int(len(dry["bad_rows"])),
                        graph_ms_median=float(np.median(t_g)), graph_ms_p90=float(np.percentile(t_g, 90)), graph_ms_min=float(np.min(t_g)),
                        apply0_ms_median=float(np.median(t_a)), apply0_ms_p90=float(np.percentile(t_a, 90)), apply_once_ms=float(t_once),
                        host_graph_ms_median=cpu["graph_ms"], host_erase_ms_median=cpu["erase_ms"],
                        outputs_agree=bool(cpu["graph_checksum"] == cs_g and cpu["erase_checksum"] == cs_a))
            print(json.dumps(case), flush=True)
            # put the table back as it was for the next neighbour count
            for k in range(n_kf):
                hip.map_put(k + 1, rows[k])
            hip.map_point_bad(np.nonzero(pt_bad == 0)[0], False)
    finally:
        hip.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="200,1000,4000")
    ap.add_argument("--neigh", default="20,100")
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--limit", type=int, default=240, help="seconds one table size may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "local_ba_graph_times.json"))
    ap.add_argument("--case", type=int, default=0, help="internal: measure this table size in this process")
    a = ap.parse_args()
    neighs = [int(s) for s in a.neigh.split(",")]
    if a.case:
        run_case(a.case, neighs, a.reps)
        return
    res = dict(host=platform.processor() or platform.machine(), keypoints=N_KP, reps=a.reps, cases=[])
    for n_kf in (int(s) for s in a.sizes.split(",")):
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--case", str(n_kf), "--neigh", a.neigh, "--reps", str(a.reps)],
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
