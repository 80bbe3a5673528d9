#!/usr/bin/env python3
"""bench.py -- frames/s of the per-frame hot path + LocalBA on MI355X (BASELINE.json metric).

One "step" = one frame of the synthetic KITTI-00-shaped stream (1241x376 u8, 2000 keypoints) through the
full HIP path (BASELINE.json configs[2]): extract (pyramid, FAST, quadtree, orientation, blur, patch
gather, ASDNet) -> frame grid -> SearchByProjection vs the previous frame -> PoseOptimization ->
isInFrustum + SearchByProjection vs a local map -> PoseOptimization; every 15th step (the reference's
--max_step_KF=15, run_vslam_kitti.sh:7) also runs LocalBundleAdjustment on the SURVEY 8(d) nominal problem
(24 free + 12 fixed keyframes, 6000 map points, ~29k edges).  Frames are resident in HBM before the timed
region.  SLAM is sequential per trajectory, so N GPUs = N independent sequences (replicas, no collective on
the data path; a gloo barrier brackets the timed region).  `--gpus N` without torchrun's environment starts the N ranks
itself (fresh child processes, before this one has made any HIP call).  `--sequences S` is BASELINE configs[4]: S
sequences of different lengths (the 11 KITTI odometry sequences, scaled by --seq-scale) handed out longest-first to
whichever rank is free, value = sum of frames / wall time.

Prints ONE JSON line (rank 0).  A plain run sets up, warms up, times the K steps (`--steps`) and prints the line: the
headline, `steady_state` and the ASDNet figures the timed window itself collects (`roofline`, `asdnet_layers`).
`--full` adds the passes of their own the headline does not need -- the variants (`lane_variant`,
`one_submission_variant`, `local_map_sweep`, `do_mapping_variant`, `h2d_variant`) and `cpu_baseline`, which times the
same step with the CPU restatement (oracle/: front-end, matchers, pose optimisation; PyTorch-CPU ASDNet run per level
like the reference) and, when oracle/_ref is present, the reference's own g2o for LocalBA -- as a reported baseline,
never the product.  `--dump-outputs DIR` writes what the last timed step returned (its statistics: keypoints, matches of
both stages, inliers, LocalBA chi2 on a keyframe) as DIR/<name>.npy; the inputs are seeded, so two builds compare output
for output.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
import __graft_entry__ as graft  # noqa: E402

KF_INTERVAL = 15
LOOKAHEAD = int(os.environ.get("ASD_BENCH_LOOKAHEAD", "3"))          # frames of read-ahead for the pipelined extractor (asd_extract_submit queue)
N_FRAMES = 30          # distinct synthetic frames kept resident in HBM, cycled
PRIME_FRAMES = 30      # untimed frames before the timed region at least (allocations on first use, streams, clocks): warm-up + priming
BOUNDS = (0.0, 1241.0, 0.0, 376.0)
PEAK_F32_MFMA_TFLOPS = 157.3   # MI355X_MICROARCH.md, chip-level parameters (dense f32 matrix)
PEAK_BF16_MFMA_TFLOPS = 2516.6  # dense bf16: 256 CU x 4 SIMD x 1024 FLOP/clk x 2.4 GHz (the guide's "~2.5 PF dense")
SPLIT_PRODUCTS = {2: 3, 3: 6}   # 16-bit MFMA products per f32 multiply-add in the split-operand kernels (asdnet.hip, K1s), by piece count
L2_MACS = 9_437_184            # conv2 (32->32 @32x32) MACs per patch, SURVEY 8(a) E6


# ------------------------------------------------------------------ distributed plumbing (control plane only)
def dist_env():
    return int(os.environ.get("RANK", "0")), int(os.environ.get("LOCAL_RANK", "0")), int(os.environ.get("WORLD_SIZE", "1"))


class Dist:
    """gloo process group used ONLY for the barrier and the max-over-ranks of the timed region."""

    def __init__(self, world):
        self.world = world
        self.rank, self.local_rank, _ = dist_env()
        self.pg = None
        if world > 1:
            import torch.distributed as dist
            os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
            os.environ.setdefault("MASTER_PORT", "29533")
            dist.init_process_group(backend="gloo", rank=self.rank, world_size=world)
            self.pg = dist

    def barrier(self):
        if self.pg:
            self.pg.barrier()

    def max(self, v):
        if not self.pg:
            return v
        import torch
        t = torch.tensor([v], dtype=torch.float64)
        self.pg.all_reduce(t, op=self.pg.ReduceOp.MAX)
        return float(t[0])

    def sum(self, v):
        if not self.pg:
            return v
        import torch
        t = torch.tensor([v], dtype=torch.float64)
        self.pg.all_reduce(t, op=self.pg.ReduceOp.SUM)
        return float(t[0])

    def next_ticket(self, key="ticket"):
        """shared counter (control plane only): the sequence queue of --sequences.  0, 1, 2, ... across all ranks."""
        if not self.pg:
            self._local = getattr(self, "_local", -1) + 1
            return self._local
        if getattr(self, "store", None) is None:
            from torch.distributed import distributed_c10d
            self.store = distributed_c10d._get_default_store()
        return int(self.store.add(key, 1)) - 1

    def gather_json(self, obj):
        """every rank's small report on rank 0 (all ranks call it)"""
        if not self.pg:
            return [obj]
        out = [None] * self.world
        self.pg.all_gather_object(out, obj)
        return out

    def close(self):
        if self.pg:
            self.pg.destroy_process_group()


def free_port():
    import socket
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def spawn_ranks(n, argv):
    """`python bench.py --gpus N` without a launcher: N fresh child processes, rank i on GPU i (LOCAL_RANK), gloo
    rendezvous on 127.0.0.1.  Called before this process has loaded the HIP library or asked torch about the GPU, and
    the children are new processes (no exec of a process that has touched the GPU).  Rank 0's stdout is this
    process's stdout (the one JSON line); the exit code is the worst child's."""
    import subprocess
    port = free_port()
    procs = []
    for r in range(n):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n), MASTER_ADDR="127.0.0.1",
                   MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + argv, env=env,
                                      stdout=None if r == 0 else sys.stderr))
    rc = 0
    try:
        pending = set(range(n))
        while pending:
            for r in sorted(pending):
                code = procs[r].poll()
                if code is not None:
                    pending.discard(r)
                    if code != 0 and rc == 0:
                        rc = code
                        print(f"bench: rank {r} exited with {code}; stopping the others", file=sys.stderr)
                        for q in pending:
                            procs[q].terminate()
            time.sleep(0.05)
    finally:
        for pr in procs:
            if pr.poll() is None:
                pr.kill()
    return rc


def gpu_local_cpus(device):
    """CPUs on the NUMA node of GPU `device` (the amdgpu render node's PCI device, /sys .../local_cpulist), or None when the box
    does not say.  Read from sysfs only: no HIP call."""
    try:
        cards = sorted(d for d in os.listdir("/sys/class/drm") if d.startswith("renderD"))
        path = f"/sys/class/drm/{cards[device]}/device/local_cpulist"
        cpus = set()
        for part in open(path).read().strip().split(","):
            if part:
                a, _, b = part.partition("-")
                cpus.update(range(int(a), int(b or a) + 1))
        return cpus or None
    except Exception:
        return None


def rank_cpu_set(rank, world, device=None):
    """The CPUs rank `rank` of `world` pins itself to: an equal, DISJOINT slice of what this process may use (each rank runs three host
    threads whose turn-around is on the critical path: tracker, extraction workers, optional LocalBA lane), taken from the GPU's own
    NUMA node where sysfs names one and every rank's slice still fits there."""
    if not hasattr(os, "sched_getaffinity"):
        return None
    avail = sorted(os.sched_getaffinity(0))
    if world <= 1 or len(avail) < world:
        return None
    per = len(avail) // world
    mine = avail[rank * per:(rank + 1) * per]
    local = gpu_local_cpus(device if device is not None else rank)
    if local:
        near = [c for c in avail if c in local]
        share = len(near) // max(1, sum(1 for r in range(world) if gpu_local_cpus(r) == local))
        if share >= 3:   # ranks whose GPUs share this node split its CPUs among themselves, in rank order
            peers = [r for r in range(world) if gpu_local_cpus(r) == local]
            k = peers.index(rank) if rank in peers else 0
            mine = near[k * share:(k + 1) * share]
    return set(mine)


def pin_rank(rank, world, device=None):
    """Called before anything touches the GPU (threads started later inherit the mask).  ASD_BENCH_NO_AFFINITY=1 leaves the process alone."""
    if os.environ.get("ASD_BENCH_NO_AFFINITY"):
        return None
    cpus = rank_cpu_set(rank, world, device)
    if cpus:
        try:
            os.sched_setaffinity(0, cpus)
        except OSError:
            return None
    return cpus


def host_cores():
    """CPU threads this process may really use: affinity mask capped by the cgroup CPU quota."""
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    try:
        quota, period = open("/sys/fs/cgroup/cpu.max").read().split()
        if quota != "max":
            n = min(n, max(1, int(float(quota) / float(period) + 0.5)))
    except Exception:
        pass
    return max(1, min(n, 64))


def device_sync(device=0):
    try:
        import torch
        if torch.cuda.is_available():
            torch.cuda.synchronize(device)
    except Exception:
        pass


# ------------------------------------------------------------------ synthetic tracking inputs
def backproject_identity(K, uv, depth):
    fx, fy, cx, cy = K
    return np.stack([(uv[:, 0] - cx) / fx * depth, (uv[:, 1] - cy) / fy * depth,
                     np.full(len(uv), depth)], 1).astype(np.float32)


def predicted_uv(kps):
    """where frame t's keypoints land in frame t+1 of synth.scene_frame (3 px drift, 0.3 % zoom)"""
    z = 1.003
    return np.stack([(kps["x"] - 620.5) * z + 620.5 - 3 * z, (kps["y"] - 188.0) * z + 188.0 - 0.2 * z], 1).astype(np.float32)


# BASELINE configs[4]: the 11 KITTI odometry sequences (frames in image_0, image size, intrinsics file of the reference's
# cameraconfig/KITTI/: kitti00-02.txt, kitti03.txt, kitti04-12.txt); a replay is kitti.cc:116-155 over one of them
KITTI_CAM = {"00-02": (1241, 376, (718.856, 718.856, 607.1928, 185.2157)),
             "03": (1242, 375, (721.5377, 721.5377, 609.5593, 172.854)),
             "04-12": (1226, 370, (707.0912, 707.09127, 601.8873, 183.1104))}
KITTI_SEQUENCES = [("00", 4541, "00-02"), ("01", 1101, "00-02"), ("02", 4661, "00-02"), ("03", 801, "03"), ("04", 271, "04-12"),
                   ("05", 2761, "04-12"), ("06", 1101, "04-12"), ("07", 1101, "04-12"), ("08", 4071, "04-12"),
                   ("09", 1591, "04-12"), ("10", 1201, "04-12")]


def sequence_table(n, scale):
    """n sequences (the KITTI table, repeated if n > 11), lengths scaled, LONGEST FIRST: the order the shared queue hands
    them out in, so the long ones start first and the short ones fill the tail (list scheduling)"""
    seqs = []
    for i in range(n):
        name, frames, cam = KITTI_SEQUENCES[i % len(KITTI_SEQUENCES)]
        seqs.append({"name": name if i < len(KITTI_SEQUENCES) else f"{name}+{i // len(KITTI_SEQUENCES)}",
                     "frames": max(KF_INTERVAL, int(round(frames * scale))), "cam": cam})
    return sorted(seqs, key=lambda q: (-q["frames"], q["name"]))


class Workload:
    def __init__(self, synth, seed_offset=0, cams=()):
        self.K32 = np.array(synth.KITTI_K, np.float32)
        self.K64 = np.array(synth.KITTI_K, np.float64)
        # further camera / image-size classes (--sequences): frames of each class resident in HBM too
        self.cam_frames = {c: [synth.scene_frame(t + 3 * seed_offset, seed=21 + k, w=KITTI_CAM[c][0], h=KITTI_CAM[c][1])
                               for t in range(N_FRAMES)] for k, c in enumerate(cams)}
        self.T = np.eye(4, dtype=np.float32)
        self.pose0 = np.array([0.002, -0.001, 0.0015, 1.0, 0.01, -0.02, 0.03])
        self.pose0[:4] /= np.linalg.norm(self.pose0[:4])
        self.ba = synth.ba_problem(seed=1 + seed_offset)
        self.inv_sigma2 = (1.0 / (np.float32(1.2) ** np.arange(8)) ** 2).astype(np.float64)
        self.scale32 = (np.float32(1.2) ** np.arange(8)).astype(np.float32)   # level scale table, f32 like mvScaleFactors
        self.frames = [synth.scene_frame(t + 3 * seed_offset) for t in range(N_FRAMES)]


def ba_problem_for_keyframe(ba, kf):
    """The LocalBA problem of keyframe number kf: the nominal problem with every observation moved by a deterministic
    +-0.1 px that depends on (edge, keyframe) -- a real map changes between keyframes, so no two runs are the same problem (the
    number of Levenberg trials then varies too).  Integer hash in uint32 arithmetic, mirrored term by term in host/track_loop.cpp."""
    E = len(ba["e_point"])
    i = np.arange(2 * E, dtype=np.uint32)
    with np.errstate(over="ignore"):
        h = i * np.uint32(2654435761) + np.uint32(kf) * np.uint32(40503) + np.uint32(12345)
        h ^= h >> np.uint32(15)
        h = h * np.uint32(2246822519)
        h ^= h >> np.uint32(13)
    u = ((h >> np.uint32(8)) & np.uint32(0xFFFF)).astype(np.float64)
    p = dict(ba)
    p["e_obs"] = np.ascontiguousarray(ba["e_obs"], np.float64) + ((u / 65536.0 - 0.5) * 0.2).reshape(E, 2)
    return p


def track_step(be, wl, image_handle, last, do_ba, next_handles=(), t=0):
    """One frame through extract -> TrackWithMotionModel body (M1 + P1) -> UpdateLocalMap stand-in -> TrackLocalMap body (isInFrustum +
    M2 + P1) (-> LocalBA, in line).  `be` is a backend (HIP or CPU restatement) exposing the same operations.  ExtractDesc of the NEXT
    frame does not depend on this frame's tracking, so the HIP backend reads ahead (asd_extract_submit, own streams + worker thread:
    the replay knows its next images, Examples/Monocular/kitti.cc:116-155) as soon as this frame's descriptors are adopted; every frame
    still goes through every stage.  Data flow between the stages as in the reference: the local-map stage starts from the pose
    the motion-model stage optimised and works on the matches it kept (Tracking.cc:693-714, 725-736); the local map is put together
    AFTER the motion-model stage, from its matches (UpdateLocalMap, Tracking.cc:726)."""
    kps, desc = be.extract(image_handle)   # results stay valid through the next step (own arrays / library views)
    cur = be.make_frame(kps, desc)
    if next_handles:
        be.prefetch(next_handles)
    stats = {"n_kp": len(kps)}
    has_next = np.ones(len(kps), np.uint8)   # bootstrap frame: as after initialisation, every keypoint holds a map point
    if last is not None:
        lk, ld, lframe, has = last
        nl, n_cur = len(lk), len(kps)
        uv = wl.predicted_uv(lk) if hasattr(wl, "predicted_uv") else predicted_uv(lk)
        Xw = backproject_identity(wl.K32, uv, 20.0)
        # `has` = the map points the last frame held when it became mLastFrame: its FINAL matches (kept motion-model matches and local-map
        # matches minus the second PoseOptimization's outliers, Tracking.cc:296-349) -- derived from that frame's results, see the end of this function
        # map point descriptors: the HIP backend keeps them in the device-resident bank (rows 0..n-1 = the last
        # frame's descriptors, rows n..2n-1 = the same again for the displaced copy), the CPU backend gets the table
        be.set_map_descriptors(lframe, ld)
        # attributes of the map points around the frame (they exist before the frame is tracked: MapPoint::mWorldPos, mNormalVector,
        # mfMin/MaxDistance): the last frame's points plus a second, displaced copy (~2x keypoints, like a local map)
        Xw2 = np.concatenate([Xw, Xw + np.float32(0.02)])
        nrm = (Xw2 / np.linalg.norm(Xw2, axis=1, keepdims=True)).astype(np.float32)
        dist = np.linalg.norm(Xw2, axis=1).astype(np.float32)
        lv = np.concatenate([lk["octave"], lk["octave"]])
        maxd = dist * wl.scale32[lv]            # f32 * f32, mirrored term by term in host/track_loop.cpp
        mind = maxd / wl.scale32[7]
        fused = getattr(be, "fused", False)   # search + claim replay + PoseOptimization as one submission (asd_track_*)
        # ---- TrackWithMotionModel (Tracking.cc:664-723): SearchByProjection against the last frame, PoseOptimization
        outl1 = np.zeros(n_cur, np.uint8)
        pose1 = wl.pose0.copy()
        if fused:
            m1, n1, pose1, outl1, _ = be.track_motion_model(cur, lframe, n_cur, has, Xw, wl.T, wl.K32, 15.0, wl.pose0)
        else:
            m1, n1 = be.match_frame(cur, lframe, n_cur, has, Xw, ld, wl.T, wl.K32, 15.0)
            j = np.nonzero(m1 >= 0)[0]
            if len(j) >= 3:
                obs = np.stack([kps["x"][j], kps["y"][j]], 1).astype(np.float64)
                pose1, o, _ = be.pose_opt(wl.pose0, Xw[m1[j]].astype(np.float64), obs, wl.inv_sigma2[kps["octave"][j]], wl.K64)
                outl1[j] = o
        stats["m1"] = int(n1)
        keep = (m1 >= 0) & (outl1 == 0)       # Tracking.cc:695-714: matches the optimisation marked as outliers are dropped
        # the frame's pose from here on = the optimised one (mCurrentFrame.SetPose, Optimizer.cc:405-407)
        T1 = be.pose7_to_tcw(pose1) if (m1 >= 0).sum() >= 3 else wl.T
        # ---- UpdateLocalMap stand-in (Tracking.cc:726, 907-): the local points = the candidates that are not in the frame already
        # (SearchLocalPoints skips those, Tracking.cc:811-823)
        in_frame = np.zeros(2 * nl, bool)
        in_frame[m1[m1 >= 0]] = True       # kept matches (:811-823) AND the dropped outliers' map points (mnLastFrameSeen, :705-707)
        sel = np.nonzero(~in_frame)[0].astype(np.int32)
        occ = keep.astype(np.uint8)
        cur_Xw = Xw[np.maximum(m1, 0)]
        # ---- TrackLocalMap (Tracking.cc:725-736): isInFrustum + SearchByProjection(frame, points) + PoseOptimization from pose1
        if fused:   # frustum test, level prediction and search windows on the device too (asd_track_local_points)
            m2, n2, _, outl2, ninl = be.track_local_points(cur, n_cur, Xw2[sel], nrm[sel], mind[sel], maxd[sel], sel, occ, cur_Xw, 1.0, 0.8, T1, wl.K32, pose1)
            stats["m2"] = int(n2)
            if (keep | (m2 >= 0)).sum() >= 3:
                stats["inliers"] = int(ninl)
            else:
                outl2 = np.zeros(n_cur, np.uint8)
        else:
            fr = be.frustum(cur, Xw2[sel], nrm[sel], mind[sel], maxd[sel], T1, wl.K32)
            m2, n2 = be.match_points(cur, n_cur, fr, (ld, ld), sel, occ, 1.0, 0.8)
            stats["m2"] = int(n2)
            jj = np.nonzero(keep | (m2 >= 0))[0]
            outl2 = np.zeros(n_cur, np.uint8)
            if len(jj) >= 3:
                X = np.where(keep[jj][:, None], Xw[np.maximum(m1[jj], 0)], Xw2[sel[np.maximum(m2[jj], 0)]])
                obs = np.stack([kps["x"][jj], kps["y"][jj]], 1).astype(np.float64)
                _, o2, ninl = be.pose_opt(pose1, X.astype(np.float64), obs, wl.inv_sigma2[kps["octave"][jj]], wl.K64)
                outl2[jj] = o2
                stats["inliers"] = int(ninl)
        # what the frame holds when it becomes the last frame (Tracking.cc:345-349: the local-map stage's outliers are dropped)
        has_next = ((keep | (m2 >= 0)) & (np.asarray(outl2) == 0)).astype(np.uint8)
    if do_ba:
        prob = ba_problem_for_keyframe(wl.ba, t // KF_INTERVAL)
        if getattr(be, "async_ba", False):
            # variant only (--lane-ba): LocalBA on the library's lane, beside the next frames' tracking -- NOT the reference's order
            # (Tracking.cc:797 -> LocalMapping.cc:89 is an in-line call): submitted here, collected before the next submission
            be.local_ba_collect()
            be.local_ba_submit(prob)
            stats["ba_submitted"] = True
        else:
            r = be.local_ba(prob)
            stats["ba_chi2"] = float(r["chi2_second"])
    return (kps, desc, cur, has_next), stats


class asd_track_stats(__import__("ctypes").Structure):
    _fields_ = [("n_kp", __import__("ctypes").c_int32), ("m1", __import__("ctypes").c_int32), ("m2", __import__("ctypes").c_int32),
                ("inliers", __import__("ctypes").c_int32), ("ba_chi2", __import__("ctypes").c_double),
                ("has_m1", __import__("ctypes").c_int32), ("has_m2", __import__("ctypes").c_int32),
                ("has_inliers", __import__("ctypes").c_int32), ("has_ba", __import__("ctypes").c_int32),
                ("stereo_matched", __import__("ctypes").c_int32), ("has_stereo", __import__("ctypes").c_int32)]


class asd_do_mapping_inputs(__import__("ctypes").Structure):
    _C = __import__("ctypes")
    _fields_ = [("slot_cur", _C.c_int32), ("has_mp_cur", _C.c_void_p), ("Tcw_cur", _C.c_void_p), ("K_cur", _C.c_void_p),
                ("n_nb", _C.c_int32), ("nb", _C.c_void_p), ("n_fuse_calls", _C.c_int32), ("fuse_calls", _C.c_void_p),
                ("n_fuse_total", _C.c_int32), ("valid", _C.c_void_p), ("Xw", _C.c_void_p), ("normal", _C.c_void_p), ("min_dist", _C.c_void_p),
                ("max_dist", _C.c_void_p), ("desc_rows", _C.c_void_p), ("th", _C.c_float),
                ("n_sets", _C.c_int32), ("set_start", _C.c_void_p), ("set_desc", _C.c_void_p)]


def build_do_mapping_inputs(pkg, hip, n_nb=20, n_kp=2000, slot0=8, bank_row0=20000):
    """Stand-in keyframe neighbourhood for the per-keyframe stage in front of LocalBA (LocalMapping::DoMapping, LocalMapping.cc:59-113):
    a current keyframe and nn = 20 covisible keyframes observing the same points (LocalMapping.cc:303-307), resident in frame slots
    slot0 .. slot0 + 20 with their FeatureVectors; Fuse candidates = 1200 points into each neighbour + 2400 into the current keyframe
    (SearchInNeighbors, :557-636), descriptors in the bank; 600 touched map points for ComputeDistinctiveDescriptors.  Returns the
    struct and everything that must stay alive."""
    import ctypes as C
    from tests.test_mapping import K_KITTI, _kf_with_neighbours
    from tests.test_matcher import SCALES, backproject, perturbed_descriptors
    capi = pkg.capi
    kc, dc, Tc, nodes_c, has_c, nbs = _kf_with_neighbours(n_kp, n_nb, 77)
    hip.frame_set(slot0, kc, dc, BOUNDS); hip.frame_set_bow(slot0, nodes_c)
    keep = [np.ascontiguousarray(has_c, np.uint8), np.ascontiguousarray(Tc, np.float32), np.ascontiguousarray(K_KITTI, np.float32)]
    nb = (capi.asd_kf_neighbor * n_nb)()
    for b, d in enumerate(nbs):
        hip.frame_set(slot0 + 1 + b, d["kps"], d["desc"], BOUNDS); hip.frame_set_bow(slot0 + 1 + b, d["nodes"])
        h = np.ascontiguousarray(d["has"], np.uint8); keep.append(h)
        nb[b].slot, nb[b].has_mp = slot0 + 1 + b, h.ctypes.data
        nb[b].F12 = (C.c_float * 9)(*[float(v) for v in np.asarray(d["F12"], np.float32).ravel()])
        nb[b].ex, nb[b].ey = float(d["ex"]), float(d["ey"])
        nb[b].Tcw = (C.c_float * 16)(*[float(v) for v in np.asarray(d["T"], np.float32).ravel()])
        nb[b].K = (C.c_float * 4)(*[float(v) for v in K_KITTI])
    rng = np.random.default_rng(5)
    calls = (capi.asd_fuse_call * (n_nb + 1))()
    tabs, first = [], 0
    for c in range(n_nb + 1):
        kk, dd, Tk = (nbs[c]["kps"], nbs[c]["desc"], nbs[c]["T"]) if c < n_nb else (kc, dc, Tc)
        n_mp = 1200 if c < n_nb else 2400
        src = rng.integers(0, n_kp, n_mp)
        uv = np.stack([kk["x"][src], kk["y"][src]], 1) + rng.uniform(-1.5, 1.5, (n_mp, 2)).astype(np.float32)
        X = backproject(Tk, K_KITTI, uv, rng.uniform(3, 60, n_mp))
        O = -(Tk[:3, :3].astype(np.float64).T @ Tk[:3, 3].astype(np.float64))
        nv = X.astype(np.float64) - O
        dv = np.linalg.norm(nv, axis=1)
        mx = (dv * SCALES[kk["octave"][src]]).astype(np.float32)
        tabs.append((np.ones(n_mp, np.uint8), X, (nv / dv[:, None]).astype(np.float32), (mx / np.float32(SCALES[7])).astype(np.float32), mx,
                     perturbed_descriptors(dd[src], 0.04, 800 + c)))
        calls[c].slot_kf, calls[c].first, calls[c].n = (slot0 + 1 + c if c < n_nb else slot0), first, n_mp
        calls[c].Tcw = (C.c_float * 16)(*[float(v) for v in np.asarray(Tk, np.float32).ravel()])
        calls[c].K = (C.c_float * 4)(*[float(v) for v in K_KITTI])
        first += n_mp
    cat = [np.ascontiguousarray(np.concatenate([t[k] for t in tabs])) for k in range(6)]
    hip.bank_put(bank_row0, cat[5])
    rows = np.arange(bank_row0, bank_row0 + first, dtype=np.int32)
    sizes = np.random.default_rng(9).integers(2, 16, 600)
    set_start = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    set_desc = np.ascontiguousarray(np.concatenate([perturbed_descriptors(np.repeat(dc[k:k + 1], n, 0), 0.05, 100 + k) for k, n in enumerate(sizes)]), np.float32)
    keep += [nb, calls, rows, set_start, set_desc] + cat[:5]
    D = asd_do_mapping_inputs()
    D.slot_cur, D.has_mp_cur, D.Tcw_cur, D.K_cur = slot0, keep[0].ctypes.data, keep[1].ctypes.data, keep[2].ctypes.data
    D.n_nb, D.nb = n_nb, C.addressof(nb)
    D.n_fuse_calls, D.fuse_calls, D.n_fuse_total = n_nb + 1, C.addressof(calls), first
    D.valid, D.Xw, D.normal, D.min_dist, D.max_dist = (cat[k].ctypes.data for k in range(5))
    D.desc_rows, D.th = rows.ctypes.data, 3.0
    D.n_sets, D.set_start, D.set_desc = 600, set_start.ctypes.data, set_desc.ctypes.data
    return D, keep, n_kp


class NativeHost:
    """The same tracking step as track_step(), run by C++ host code (asd-slam_amd/host/track_loop.cpp -> libasdtrack.so)
    over the C ABI: the reference's host side is C++, the Python loop costs ~0.25 ms of a ~2 ms step."""

    def __init__(self, pkg, be, wl, pipeline, cam=None, frames_on_host=False, size=None, drift=None, stereo=None):
        """size = (W, H) of the frames (default KITTI 00-02); drift = (cx, cy, z, dx, dy) of the stand-in map's motion (default: the mono stream's);
        stereo = (right context, right frames resident in HBM, mb, mbf): BASELINE configs[3]"""
        import ctypes as C
        self.C = C
        path = os.path.join(ROOT, "asd-slam_amd", "libasdtrack.so")
        if not os.path.exists(path):
            raise FileNotFoundError(f"{path} not built: run `python -c 'import __graft_entry__ as g; g.build()'`")
        self.lib = C.CDLL(path)
        self.lib.asd_track_create.restype = C.c_void_p
        capi = pkg.capi
        ba = wl.ba
        self.keep = [np.ascontiguousarray(ba["poses"], np.float64), np.ascontiguousarray(ba["fixed"], np.uint8),
                     np.ascontiguousarray(ba["points"], np.float64), np.ascontiguousarray(ba["e_point"], np.int32),
                     np.ascontiguousarray(ba["e_pose"], np.int32), np.ascontiguousarray(ba["e_obs"], np.float64),
                     np.ascontiguousarray(ba["e_info"], np.float64)]
        k = self.keep
        self.prob = capi.asd_ba_problem(len(k[0]), len(k[2]), len(k[3]), k[0].ctypes.data, k[1].ctypes.data, k[2].ctypes.data,
                                        k[3].ctypes.data, k[4].ctypes.data, k[5].ctypes.data, k[6].ctypes.data,
                                        (C.c_double * 4)(*[float(x) for x in ba["K"]]), 5, 10)
        d_frames, W, H, K32 = (be.host_frames() if frames_on_host else be.d_frames), 1241, 376, wl.K32
        if size is not None:
            W, H = size
        if cam is not None:   # a sequence of another camera class (image size + intrinsics)
            d_frames, (W, H, K) = be.d_cam_frames[cam], KITTI_CAM[cam]
            K32 = np.array(K, np.float32)
        self.keep.append(K32)
        frames = (C.c_void_p * len(d_frames))(*[f.value for f in d_frames])
        self.h = C.c_void_p(self.lib.asd_track_create(be.hip.ctx, len(d_frames), frames, W, H,
                                                      K32.ctypes.data_as(C.c_void_p), wl.T.ctypes.data_as(C.c_void_p),
                                                      wl.pose0.ctypes.data_as(C.c_void_p), wl.inv_sigma2.ctypes.data_as(C.c_void_p),
                                                      wl.scale32.ctypes.data_as(C.c_void_p), C.byref(self.prob), KF_INTERVAL,
                                                      LOOKAHEAD if pipeline else 0))
        if not self.h:
            raise RuntimeError("asd_track_create failed")
        self.lib.asd_track_set_fused(self.h, int(getattr(be, "fused", True)))
        self.lib.asd_track_set_async_ba(self.h, int(getattr(be, "async_ba", False)))
        self.lib.asd_track_set_split(self.h, int(getattr(be, "split", True)))
        self.lib.asd_track_set_chain(self.h, int(getattr(be, "chain", False)))
        self.lib.asd_track_set_frames_on_host(self.h, int(frames_on_host))
        if drift is not None:
            self.lib.asd_track_set_drift(self.h, *[C.c_float(v) for v in drift])
        if stereo is not None:
            ctx_r, frames_r, mb, mbf = stereo
            fr = (C.c_void_p * len(frames_r))(*[f.value for f in frames_r])
            if self.lib.asd_track_set_stereo(self.h, ctx_r, fr, C.c_float(mb), C.c_float(mbf)) != 0:
                raise RuntimeError("asd_track_set_stereo failed")
        self.be = be

    def times(self):
        """accumulated since creation: (ms inside LocalBA, ms blocked on the extractor, steps)"""
        C = self.C
        ba, wait, steps = C.c_double(), C.c_double(), C.c_int64()
        self.lib.asd_track_get_times(self.h, C.byref(ba), C.byref(wait), C.byref(steps))
        return ba.value, wait.value, steps.value

    def run(self, t0, n, prefetch_beyond):
        st = asd_track_stats()
        rc = self.lib.asd_track_run(self.h, t0, n, int(prefetch_beyond), self.C.byref(st))
        if rc != 0:
            raise RuntimeError(f"asd_track_run failed ({rc}): {self.be.hip.lib.asd_last_error(self.be.hip.ctx).decode()}")
        out = {"n_kp": st.n_kp}
        for k in ("m1", "m2", "inliers"):
            if getattr(st, "has_" + k):
                out[k] = int(getattr(st, k))
        if st.has_ba:
            out["ba_chi2"] = float(st.ba_chi2)
        if st.has_stereo:
            out["stereo_matched"] = int(st.stereo_matched)
        return out

    def close(self):
        if self.h:
            self.lib.asd_track_destroy(self.h)
            self.h = None


class HipBackend:
    def __init__(self, pkg, wl, device, pipeline=True):
        mw = max([1241] + [KITTI_CAM[c][0] for c in wl.cam_frames])
        mh = max([376] + [KITTI_CAM[c][1] for c in wl.cam_frames])
        self.hip = pkg.AsdHip(n_features=2000, max_width=mw, max_height=mh, max_patches=4096, device=device)
        self.hip.load_weights(pkg.synth.asdnet_weights(0))

        def upload(frames):   # frames resident in HBM before the timed region
            out = []
            for f in frames:
                p = self.hip.device_alloc(f.nbytes)
                self.hip.h2d(p, f)
                out.append(p)
            return out
        self.d_frames = upload(wl.frames)
        self.wl_frames = wl.frames
        self.d_cam_frames = {c: upload(fr) for c, fr in wl.cam_frames.items()}
        self.slot = 0
        self.pending = []          # handles of submitted, not yet waited extractions (in order)
        self.pipeline = pipeline
        self.fused = True          # asd_track_motion_model / asd_track_local_map instead of matcher + solver calls
        self.async_ba = False      # True: LocalBA on the library's lane (asd_local_ba_submit / _wait) instead of in line (the reference's order)
        self.ba_out = False

    def host_frames(self):
        """the same frames in page-locked host memory (h2d_variant: the image crosses PCIe inside the step)"""
        if not hasattr(self, "_h_frames"):
            import ctypes as C
            self._h_frames = []
            for f in self.wl_frames:
                p = self.hip.host_alloc(f.nbytes)
                C.memmove(p, np.ascontiguousarray(f).ctypes.data, f.nbytes)
                self._h_frames.append(p)
        return self._h_frames

    def image(self, t):
        return self.d_frames[t % len(self.d_frames)]

    def extract(self, h):
        if self.pending and self.pending[0].value == h.value:
            self.pending.pop(0)
            # zero-copy views of the library's buffers for this submission: valid for two further submissions,
            # the tracker needs them for one (the "last frame" of the next step)
            return self.hip.extract_wait(view=True)
        self.drain()                      # something else was read ahead: drop it
        k, d = self.hip.extract_device(h, 1241, 376, 1241)
        return k.copy(), d.copy()

    def drain(self):
        while self.pending:
            self.hip.extract_wait()
            self.pending.pop(0)

    def prefetch(self, handles):
        """keep the extractions of the next frames queued (read-ahead depth = len(handles) <= LOOKAHEAD)"""
        if not self.pipeline:
            return
        have = [p.value for p in self.pending]
        if have != [h.value for h in handles[:len(have)]]:
            self.drain()
            have = []
        for h in handles[len(have):]:
            self.hip.extract_submit(h, 1241, 376, 1241, device_resident=True)
            self.pending.append(h)

    def make_frame(self, kps, desc):
        self.slot ^= 1
        self.hip.frame_set(self.slot, kps, None, BOUNDS)   # adopts the device-resident descriptors
        return self.slot

    def set_map_descriptors(self, last_slot, ld):
        n = len(ld)
        self.hip.bank_put_from_frame(last_slot, 0, n)      # device to device, no PCIe
        self.hip.bank_put_from_frame(last_slot, n, n)
        self.rows = np.arange(2 * n, dtype=np.int32)

    def match_frame(self, cur, last, n_cur, has, Xw, mp_desc, T, K, th):
        return self.hip.match_project_frame_bank(cur, last, n_cur, has, Xw, self.rows[:len(has)], T, K, th, True)

    def pose_opt(self, pose, Xw, obs, info, K):
        return self.hip.pose_optimize(pose, Xw, obs, info, K)

    def frustum(self, cur, Xw, normal, mind, maxd, T, K):
        return self.hip.frustum(cur, Xw, normal, mind, maxd, T, K)

    def match_points(self, cur, n_cur, fr, desc, sel, occ, th, ratio):
        return self.hip.match_project_points_bank(cur, n_cur, fr[0], fr[1], fr[2], fr[3], self.rows[sel], occ, th, ratio)

    def track_motion_model(self, cur, last, n_cur, has, Xw, T, K, th, pose0):
        return self.hip.track_motion_model(cur, last, n_cur, has, Xw, self.rows[:len(has)], T, K, th, pose0, True)

    def track_local_points(self, cur, n_cur, Xw, normal, mind, maxd, sel, occ, cur_Xw, th, ratio, T, K, pose0):
        return self.hip.track_local_points(cur, n_cur, Xw, normal, mind, maxd, self.rows[sel], T, K, occ, cur_Xw, th, ratio, pose0)

    def pose7_to_tcw(self, pose):
        return self.hip.pose7_to_tcw(pose)

    def local_ba(self, prob):
        # in line: no further ASDNet forward is enqueued meanwhile (host/track_loop.cpp::submit_ba does the same; the reference does nothing
        # else during LocalBundleAdjustment either)
        self.hip.extract_hold(True)
        try:
            return self.hip.local_ba(prob)
        finally:
            self.hip.extract_hold(False)

    def local_ba_submit(self, prob):
        self.hip.local_ba_submit(prob)
        self.ba_out = True

    def local_ba_collect(self):
        if not self.ba_out:
            return None
        self.ba_out = False
        return self.hip.local_ba_wait()

    def close(self):
        if getattr(self, "native", None) is not None:
            self.native.close()      # drains its own read-ahead queue and LocalBA lane
        self.drain()
        self.local_ba_collect()
        self.hip.close()


class CpuBackend:
    """CPU restatement (oracle/) -- baseline only."""

    def __init__(self, pkg, wl, nfeatures=2000):
        po = graft.load_oracle()
        po.build()
        self.orc = po.Oracle()
        self.ex = self.orc.extractor(nfeatures)
        self.ref = po.RefG2O() if po.RefG2O.available() else None
        from oracle import asdnet_torch
        import torch
        self.torch = torch
        self.cores = host_cores()
        torch.set_num_threads(self.cores)
        self.at = asdnet_torch
        self.net = asdnet_torch.build(pkg.synth.asdnet_weights(0))
        self.frames = wl.frames

    def image(self, t):
        return self.frames[t % len(self.frames)]

    def prefetch(self, h):
        pass

    def extract(self, img):
        kps, patches = self.ex.extract(img)
        return kps, self.at.describe_per_level(self.net, patches, kps["octave"])

    def make_frame(self, kps, desc):
        return self.orc.frame(kps, desc, BOUNDS)

    def match_frame(self, cur, last, n_cur, has, Xw, mp_desc, T, K, th):
        return self.orc.match_project_frame(cur, last, has, Xw, mp_desc, T, K, th, True)

    def pose_opt(self, pose, Xw, obs, info, K):
        return self.orc.pose_optimize(pose, Xw, obs, info, K)

    def frustum(self, cur, Xw, normal, mind, maxd, T, K):
        return self.orc.frustum(cur, Xw, normal, mind, maxd, T, K)

    def set_map_descriptors(self, last, ld):
        pass

    def match_points(self, cur, n_cur, fr, desc, sel, occ, th, ratio):
        return self.orc.match_project_points(cur, fr[0], fr[1], fr[2], fr[3], np.concatenate(desc)[sel], occ, th, ratio)

    def pose7_to_tcw(self, pose):
        return self.orc.pose7_to_tcw(pose)

    def local_ba(self, prob):
        return (self.ref or self.orc).local_ba(prob)


def run_steps(be, wl, t0, n, last, prefetch_beyond=False):
    if getattr(be, "native", None) is not None:   # C++ host loop: same step, same statistics
        return None, be.native.run(t0, n, prefetch_beyond)
    return run_steps_python(be, wl, t0, n, last, prefetch_beyond)


def run_steps_python(be, wl, t0, n, last, prefetch_beyond=False):
    """n frames t0 .. t0+n-1.  The extractions of frames t+1 .. t+LOOKAHEAD are queued during frame t; frames after
    the last one are only read ahead when the replay continues (prefetch_beyond) -- the timed region does, so that
    it starts and ends in the same pipeline state and contains n frames' worth of every stage."""
    stats = {}
    for i in range(n):
        t = t0 + i
        nxt = [be.image(t + k) for k in range(1, LOOKAHEAD + 1) if (i + k < n or prefetch_beyond)]
        last, stats = track_step(be, wl, be.image(t), last, do_ba=(t % KF_INTERVAL == KF_INTERVAL - 1), next_handles=nxt, t=t)
    if getattr(be, "async_ba", False):   # the run ends with its LocalBA finished (and reported if the last step started it)
        r = be.local_ba_collect()
        if stats.pop("ba_submitted", False) and r is not None:
            stats["ba_chi2"] = float(r["chi2_second"])
    stats.pop("ba_submitted", None)
    return last, stats


def dump_outputs(out_dir, stats):
    """--dump-outputs: what the last timed step returned to its caller (asd_track_stats, or the same dict from the Python loop), one
    float64 array of one element per field"""
    os.makedirs(out_dir, exist_ok=True)
    for k, v in stats.items():
        np.save(os.path.join(out_dir, f"{k}.npy"), np.array([v], np.float64))


def selftest_dist(args):
    """CPU-only rehearsal of the N>1 control plane (gloo): rendezvous, barrier, max-over-ranks, aggregation."""
    d = Dist(args.gpus)
    d.barrier()
    t0 = time.perf_counter()
    time.sleep(0.05 * (1 + d.rank))
    dt = time.perf_counter() - t0
    d.barrier()
    tmax = d.max(dt)
    total = d.sum(float(args.steps))
    # the --sequences queue: every ticket 0..10 handed out exactly once across the ranks
    seqs = sequence_table(11, 0.1)
    mine = []
    while True:
        k = d.next_ticket("sequence")
        if k >= len(seqs):
            break
        mine.append(k)
        time.sleep(0.002 * (1 + d.rank))
    tickets = d.gather_json(mine)
    affinity = d.gather_json(sorted(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else [])
    if d.rank == 0:
        print(json.dumps({"selftest": "dist", "n_gpus": args.gpus, "t_max": tmax, "frames_total": total,
                          "value": total / tmax, "tickets": tickets, "queue": [q["name"] for q in seqs], "affinity": affinity}))
    d.close()


EUROC = {"w": 752, "h": 480, "K": (458.654, 457.296, 367.215, 248.375), "mb": 0.11, "disparity": 9}


class EurocWorkload:
    """BASELINE configs[3]: EuRoC MH-shaped synthetic stereo stream -- 752x480 (cameraconfig/MH_EUROC/EuRoC_config.txt: fx 458.654,
    fy 457.296, cx 367.215, cy 248.375), baseline 0.11 m, left / right = two crops of one synthetic scene 9 px apart."""

    def __init__(self, synth, seed_offset=0):
        W, H = EUROC["w"], EUROC["h"]
        self.K32 = np.array(EUROC["K"], np.float32)
        self.K64 = np.array(EUROC["K"], np.float64)
        self.T = np.eye(4, dtype=np.float32)
        self.pose0 = np.array([0.002, -0.001, 0.0015, 1.0, 0.01, -0.02, 0.03])
        self.pose0[:4] /= np.linalg.norm(self.pose0[:4])
        self.ba = synth.ba_problem(seed=1 + seed_offset)
        self.inv_sigma2 = (1.0 / (np.float32(1.2) ** np.arange(8)) ** 2).astype(np.float64)
        self.scale32 = (np.float32(1.2) ** np.arange(8)).astype(np.float32)
        wide = [synth.scene_frame(t + 3 * seed_offset, seed=31, w=W + 96, h=H) for t in range(N_FRAMES)]
        self.left = [np.ascontiguousarray(f[:, 32:32 + W]) for f in wide]
        self.right = [np.ascontiguousarray(f[:, 32 + EUROC["disparity"]:32 + EUROC["disparity"] + W]) for f in wide]
        self.bounds = (0.0, float(W), 0.0, float(H))

    def predicted_uv(self, kps):
        # the scene drifts about the centre of the WIDE render: (W + 96) / 2 - 32 in the left crop's coordinates
        z, cx, cy = 1.003, EUROC["w"] / 2 + 16.0, EUROC["h"] / 2.0
        return np.stack([(kps["x"] - cx) * z + cx - 3 * z, (kps["y"] - cy) * z + cy - 0.2 * z], 1).astype(np.float32)


class StereoBackend:
    """Two contexts = the reference's left and right extractors (Frame.cc:64-121 would take two ORBextractors in a stereo
    build); Frame::ComputeStereoMatches after both extractions, then the monocular tracking chain on the left frame."""

    def __init__(self, pkg, wl, device):
        W, H = EUROC["w"], EUROC["h"]
        self.W, self.H, self.wl = W, H, wl
        self.L = pkg.AsdHip(n_features=2000, max_width=W, max_height=H, max_patches=4096, device=device)
        self.R = pkg.AsdHip(n_features=2000, max_width=W, max_height=H, max_patches=4096, device=device)
        for c in (self.L, self.R):
            c.load_weights(pkg.synth.asdnet_weights(0))
        self.hip = self.L
        self.dL, self.dR = [], []
        for fl, fr in zip(wl.left, wl.right):
            for ctx, f, dst in ((self.L, fl, self.dL), (self.R, fr, self.dR)):
                p = ctx.device_alloc(f.nbytes)
                ctx.h2d(p, f)
                dst.append(p)
        self.slot = 0
        self.native = None
        self.stereo_matched = 0
        self.d_frames = self.dL   # (NativeHost: the left frames; the right ones go in through asd_track_set_stereo)
        self.fused = True         # the stages as asd_track_motion_model / asd_track_local_points (both hosts)
        self.async_ba = False
        self.split = True
        self.chain = False        # two calls per frame with the host between them (the form the reference's Tracking can bind)

    def native_host(self, pkg, pipeline=True):
        """the C++ host loop in stereo mode: both extractors read ahead, asd_stereo_match during frame construction"""
        W, H, mb = EUROC["w"], EUROC["h"], EUROC["mb"]
        nh = NativeHost(pkg, self, self.wl, pipeline=pipeline, size=(W, H), drift=(W / 2 + 16.0, H / 2.0, 1.003, 3.0, 0.2),
                        stereo=(self.R.ctx, self.dR, mb, mb * EUROC["K"][0]))
        return nh

    def image(self, t):
        return t % len(self.dL)

    def prefetch(self, handles):
        pass

    def extract(self, i):
        kl, dl = self.L.extract_device(self.dL[i], self.W, self.H, self.W)
        kr, dr = self.R.extract_device(self.dR[i], self.W, self.H, self.W)
        self.right = (kr.copy(), dr.copy())
        return kl.copy(), dl.copy()

    def make_frame(self, kps, desc):
        self.slot ^= 1
        self.L.frame_set(self.slot, kps, None, self.wl.bounds)              # left: adopts the device-resident descriptors
        self.L.frame_set(2, self.right[0], self.right[1], self.wl.bounds)   # the right frame's keypoints + descriptors
        mb = EUROC["mb"]
        _, _, self.stereo_matched = self.L.stereo_match(self.R, self.slot, 2, len(kps), mb, mb * EUROC["K"][0])
        return self.slot

    def set_map_descriptors(self, last_slot, ld):
        n = len(ld)
        self.L.bank_put_from_frame(last_slot, 0, n)
        self.L.bank_put_from_frame(last_slot, n, n)
        self.rows = np.arange(2 * n, dtype=np.int32)

    def match_frame(self, cur, last, n_cur, has, Xw, mp_desc, T, K, th):
        return self.L.match_project_frame_bank(cur, last, n_cur, has, Xw, self.rows[:len(has)], T, K, th, True)

    def pose_opt(self, pose, Xw, obs, info, K):
        return self.L.pose_optimize(pose, Xw, obs, info, K)

    def frustum(self, cur, Xw, normal, mind, maxd, T, K):
        return self.L.frustum(cur, Xw, normal, mind, maxd, T, K)

    def match_points(self, cur, n_cur, fr, desc, sel, occ, th, ratio):
        return self.L.match_project_points_bank(cur, n_cur, fr[0], fr[1], fr[2], fr[3], self.rows[sel], occ, th, ratio)

    def track_motion_model(self, cur, last, n_cur, has, Xw, T, K, th, pose0):
        return self.L.track_motion_model(cur, last, n_cur, has, Xw, self.rows[:len(has)], T, K, th, pose0, True)

    def track_local_points(self, cur, n_cur, Xw, normal, mind, maxd, sel, occ, cur_Xw, th, ratio, T, K, pose0):
        return self.L.track_local_points(cur, n_cur, Xw, normal, mind, maxd, self.rows[sel], T, K, occ, cur_Xw, th, ratio, pose0)

    def pose7_to_tcw(self, pose):
        return self.L.pose7_to_tcw(pose)

    def local_ba(self, prob):
        return self.L.local_ba(prob)

    def close(self):
        self.L.close()
        self.R.close()


def stereo_steps(be, wl, t0, n, last):
    """n frames through the stereo backend: the C++ host (be.native) or the Python loop; per-frame stats carry stereo_matched"""
    if be.native is not None:
        return None, be.native.run(t0, n, True)
    last, stats = run_steps_python(be, wl, t0, n, last)
    stats["stereo_matched"] = int(be.stereo_matched)
    return last, stats


def run_euroc_stereo(args, pkg, dist, rank, world, device):
    """BASELINE configs[3] (secondary bench line): stereo association + the tracking chain + LocalBA at the EuRoC image size.
    What the reference would run in a stereo build and what it does not: the stereo optimiser edges
    (types_six_dof_expmap.cpp:256-340, 405-470) are never constructed by this fork (Optimizer.cc:266-269, 521-528 loop over
    empty vectors), so PoseOptimization / LocalBA run on monocular edges exactly as in the mono configs."""
    wl = EurocWorkload(pkg.synth, seed_offset=rank)
    be = StereoBackend(pkg, wl, device)
    if args.host == "cxx":
        be.native = be.native_host(pkg, pipeline=not args.no_pipeline)
    be.L.local_ba(wl.ba)                     # untimed: the solver's buffers come into being with the first run
    warm = max(args.warmup, PRIME_FRAMES)
    last, _ = stereo_steps(be, wl, 0, warm, None)
    be.L.sync(); be.R.sync(); device_sync(device); dist.barrier()
    t0 = time.perf_counter()
    last, stats = stereo_steps(be, wl, warm, args.steps, last)
    be.L.sync(); be.R.sync(); device_sync(device); dist.barrier()
    dt = time.perf_counter() - t0
    tmax = dist.max(dt)
    total = dist.sum(float(args.steps))
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, stats)
    if be.native is not None:
        be.native.lib.asd_track_drain(be.native.h)
        be.native.close()
        be.native = None
    be.close()
    if rank == 0:
        print(json.dumps({
            "metric": "frames/sec end-to-end tracking+LocalBA, EuRoC MH stereo @2000 keypoints (BASELINE configs[3])",
            "value": total / tmax, "unit": "frames/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": 1e3 * tmax / args.steps, "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "dtype": "f32", "data": "synthetic",
            "config": {"workload": "BASELINE configs[3]: EuRoC-MH-shaped synthetic stereo stream 752x480, 2000 kpts per image: two "
                                   "extractions (left / right contexts), Frame::ComputeStereoMatches (asd_stereo_match), then the left "
                                   "frame through SearchByProjection(frame) + PoseOptimization + isInFrustum + SearchByProjection(map) + "
                                   "PoseOptimization, LocalBA every 15 frames",
                       "not_included": "stereo optimiser edges: dead code in the reference (Optimizer.cc:266-269, 521-528), mono edges only",
                       "host": ("C++ host loop over the C ABI (libasdtrack, stereo mode): both extractors read ahead, asd_stereo_match during frame "
                                "construction on the second stream, asd_track_frame per frame" if args.host == "cxx" else
                                "Python loop (ctypes), sequential extraction (no read-ahead)"), "kf_interval": KF_INTERVAL,
                       "parallelism": f"replicas x{world}"},
            "last_step": stats}))
    dist.close()


def run_sequences(args, pkg, dist, rank, world, device):
    """BASELINE configs[4]: S independent sequences over `world` GPUs.  Every rank owns one device and one context; the
    sequences sit in one shared queue, longest first, and a rank that finishes one takes the next (a ticket counter in the
    rendezvous store -- control plane only, nothing on the data path).  A sequence is a replay from scratch
    (kitti.cc:116-155): fresh tracker state, its own image size and intrinsics, read-ahead extraction inside it only."""
    seqs = sequence_table(args.sequences, args.seq_scale)
    cams = sorted({q["cam"] for q in seqs})
    wl = Workload(pkg.synth, seed_offset=rank, cams=cams)
    be = HipBackend(pkg, wl, device=device, pipeline=not args.no_pipeline)
    be.native = None

    def replay(cam, n):
        h = NativeHost(pkg, be, wl, pipeline=not args.no_pipeline, cam=cam)
        try:
            return h.run(0, n, False)
        finally:
            h.close()
    replay(cams[0], args.warmup)                       # untimed: code objects, clocks, allocations
    be.hip.sync(); device_sync(device); dist.barrier()
    t0 = time.perf_counter()
    mine, frames, stats = [], 0, {}
    while True:
        k = dist.next_ticket("sequence")
        if k >= len(seqs):
            break
        q = seqs[k]
        ts = time.perf_counter()
        stats = replay(q["cam"], q["frames"])
        mine.append({"seq": q["name"], "frames": q["frames"], "s": round(time.perf_counter() - ts, 4)})
        frames += q["frames"]
    be.hip.sync(); device_sync(device)
    busy = time.perf_counter() - t0
    dist.barrier()
    dt = time.perf_counter() - t0
    tmax = dist.max(dt)
    total = dist.sum(float(frames))
    reports = dist.gather_json({"rank": rank, "device": device, "busy_s": round(busy, 4), "sequences": mine})
    if args.dump_outputs and rank == 0:   # the last frame of the last sequence this rank replayed
        dump_outputs(args.dump_outputs, stats)
    be.close()
    if rank == 0:
        assert int(total) == sum(q["frames"] for q in seqs), "a sequence was lost or run twice"
        print(json.dumps({
            "metric": "frames/sec end-to-end tracking+LocalBA, KITTI 00 mono @2000 keypoints",
            "value": total / tmax, "unit": "frames/s", "n_gpus": world, "steps": int(total), "warmup": args.warmup,
            "ms_per_step": 1e3 * tmax / total, "higher_is_better": True, "scaling": "strong", "vs_baseline": None,
            "dtype": "f32", "data": "synthetic",
            "config": {"workload": f"BASELINE configs[4]: {len(seqs)} independent KITTI-odometry-shaped sequences "
                                   f"(lengths x{args.seq_scale}, image sizes / intrinsics of cameraconfig/KITTI) handed out "
                                   f"longest-first to {world} GPU(s), one context per GPU, no RCCL; value = sum of frames / wall",
                       "sequences": [{k: q[k] for k in ("name", "frames", "cam")} for q in seqs],
                       "kf_interval": KF_INTERVAL, "parallelism": f"{world} rank(s), shared sequence queue, no collective"},
            "wall_s": tmax, "ranks": reports}))
    dist.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=45)
    ap.add_argument("--cpu-frames", type=int, default=15, help="--full: frames of the CPU baseline sample (0 = skip)")
    ap.add_argument("--full", action="store_true",
                    help="also run the passes the headline does not need: the variants (N = 1 only, each can be skipped with its --no-* "
                         "switch) and the CPU baselines")
    ap.add_argument("--dump-outputs", metavar="DIR",
                    help="after the timed steps, write the statistics the last timed step returned as DIR/<name>.npy (float64)")
    ap.add_argument("--selftest-dist", action="store_true")
    ap.add_argument("--sequences", type=int, default=0,
                    help="BASELINE configs[4]: this many independent sequences (11 = KITTI odometry 00-10) in a shared "
                         "longest-first queue over the ranks; value = sum of frames / wall")
    ap.add_argument("--seq-scale", type=float, default=0.1, help="--sequences: fraction of the real sequence lengths")
    ap.add_argument("--workload", choices=["kitti-mono", "euroc-stereo"], default="kitti-mono",
                    help="kitti-mono = the headline configuration (BASELINE configs[2]); euroc-stereo = configs[3], a secondary line")
    ap.add_argument("--no-pipeline", action="store_true", help="do not overlap ExtractDesc(t+1) with tracking(t)")
    ap.add_argument("--no-split", action="store_true", help="C++ host: run each asd_track_* stage to completion before any other host work (no asd_track_async / asd_track_finish)")
    ap.add_argument("--chain", action="store_true", help="C++ host: both tracking stages as ONE submission (asd_track_frame) with the next frame constructed on a "
                                                          "second stream.  Not the default: the reference selects its local map BETWEEN the stages "
                                                          "(Tracking::UpdateLocalMap, Tracking.cc:730), which this form cannot host; measured as `one_submission_variant`")
    ap.add_argument("--no-chain", action="store_true", help="(default since round 5, kept for old command lines) two submissions with the host in between")
    ap.add_argument("--no-one-submission-variant", action="store_true", help="skip the extra pass that measures asd_track_frame (N = 1 only)")
    ap.add_argument("--no-local-map-sweep", action="store_true", help="skip the extra passes with 8 k and 16 k local-map candidates per frame (N = 1 only)")
    ap.add_argument("--lane-ba", action="store_true",
                    help="variant: LocalBA on the library's lane (asd_local_ba_submit / _wait) beside the next frames, which then track against the "
                         "pre-BA map -- not the reference's order (Tracking.cc:797 -> LocalMapping.cc:89 runs it in line, the default here)")
    ap.add_argument("--sync-ba", action="store_true", help="(default since round 3, kept for old command lines) LocalBA in line with tracking")
    ap.add_argument("--no-do-mapping-variant", action="store_true", help="skip the extra pass with the batched per-keyframe stage in front of LocalBA (N = 1 only)")
    ap.add_argument("--no-h2d-variant", action="store_true", help="skip the extra pass with the frames handed over in page-locked host memory (N = 1 only)")
    ap.add_argument("--no-lane-variant", action="store_true", help="skip the extra untimed-for-the-headline pass that measures the lane variant (N = 1 only)")
    ap.add_argument("--no-fuse", action="store_true", help="matcher and PoseOptimization as separate calls (two host round trips per stage)")
    ap.add_argument("--host", choices=["cxx", "python"], default="cxx",
                    help="who drives the per-frame step: C++ host code over the C ABI (default, as in the reference) or the Python loop")
    args = ap.parse_args()
    if args.gpus < 1:
        raise SystemExit("--gpus must be >= 1")
    # N > 1 without a launcher: start the ranks ourselves.  Nothing in this process has touched the GPU yet.
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        sys.exit(spawn_ranks(args.gpus, sys.argv[1:]))
    rank, local_rank, world = dist_env()
    world = max(world, 1)
    if world != args.gpus:   # never report a GPU count that is not the one asked for
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}")
    # every rank keeps to its own CPUs (its GPU's NUMA node where sysfs says which): set before any HIP call, inherited by the
    # library's worker threads
    pinned = pin_rank(rank, world)
    if args.selftest_dist:
        return selftest_dist(args)

    if not all(os.path.exists(os.path.join(ROOT, "asd-slam_amd", f)) for f in ("libasdhip.so", "libasdtrack.so")):
        graft.build()
    pkg = graft.load_package()
    dist = Dist(world)
    # ASD_BENCH_DEVICE pins every rank to one device: rehearsal of the N > 1 path on a single-GPU box only
    device = int(os.environ["ASD_BENCH_DEVICE"]) if "ASD_BENCH_DEVICE" in os.environ else (local_rank if world > 1 else 0)
    if args.sequences > 0:
        return run_sequences(args, pkg, dist, rank, world, device)
    if args.workload == "euroc-stereo":
        return run_euroc_stereo(args, pkg, dist, rank, world, device)
    wl = Workload(pkg.synth, seed_offset=rank)
    be = HipBackend(pkg, wl, device=device, pipeline=not args.no_pipeline)
    be.fused = not args.no_fuse
    be.async_ba = bool(args.lane_ba)
    be.split = not args.no_split
    be.chain = bool(args.chain) and not args.no_chain
    be.native = None
    if args.host == "cxx":
        try:
            be.native = NativeHost(pkg, be, wl, pipeline=not args.no_pipeline)
        except (OSError, FileNotFoundError) as e:   # host-side convenience library only: the Python loop drives the same C ABI
            print(f"bench: C++ host loop unavailable ({e}); using the Python loop", file=sys.stderr)
            args.host = "python"

    # one-time initialisation that a short --warmup would otherwise leave inside the timed region: the LocalBA solver's device
    # buffers, pinned staging and (--lane-ba) the lane's thread + stream come into being with the first run (21 ms against 4 ms
    # for every later one), and the first keyframe is frame 14 ...
    if be.async_ba:
        be.hip.local_ba_submit(wl.ba); be.hip.local_ba_wait()
    else:
        be.hip.local_ba(wl.ba)
    # ... and the same for the per-frame path: buffers that grow on first use, the extractor's slots and streams, kernel
    # attributes, clocks.  A replay runs for thousands of frames; a `--warmup 5` run reaches that state through PRIME_FRAMES extra
    # untimed frames in front of the W warm-up frames (none when W >= PRIME_FRAMES).  The K timed frames follow the warm-up directly.
    prime = max(0, PRIME_FRAMES - args.warmup)
    # The LocalBA share of the timed window must not depend on where the window happens to start: a keyframe is every KF_INTERVAL-th
    # frame, so K frames hold floor or ceil of K / KF_INTERVAL of them.  The window is placed (a few more priming frames) so that it
    # holds the CEILING -- never fewer LocalBAs than the steady-state share (round 3's 20-frame window held 1 where 1.33 is the share:
    # 4 % in the headline's favour).  `steady_state` below reports tracking and LocalBA from separately accumulated times as well.
    def kf_in(t_first, n):
        return sum(1 for t in range(t_first, t_first + n) if t % KF_INTERVAL == KF_INTERVAL - 1)
    want_kf = -(-args.steps // KF_INTERVAL)
    while kf_in(prime + args.warmup, args.steps) < want_kf:
        prime += 1
    last, _ = run_steps(be, wl, 0, prime + args.warmup, None, prefetch_beyond=True)    # untimed: prime + W warm-up steps
    tm0 = be.native.times() if be.native is not None else None
    be.hip.profile_enable(True)
    be.hip.sync(); device_sync(device); dist.barrier()
    t0 = time.perf_counter()
    # EXACTLY K timed steps; the replay keeps reading ahead across both ends of the timed region (steady state);
    # the device-wide synchronize below also waits for whatever read-ahead work is in flight
    last, stats = run_steps(be, wl, prime + args.warmup, args.steps, last, prefetch_beyond=True)
    be.hip.sync(); device_sync(device); dist.barrier()
    dt = time.perf_counter() - t0
    be.hip.profile_enable(False)   # the per-layer ASDNet figures below cover the timed window only
    tmax = dist.max(dt)
    frames_total = dist.sum(float(args.steps))
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, stats)
    n_kf = kf_in(prime + args.warmup, args.steps)
    steady = None
    if tm0 is not None:
        tm1 = be.native.times()
        ba_ms, wait_ms = tm1[0] - tm0[0], tm1[1] - tm0[1]
        track_ms = (1e3 * dt - ba_ms) / args.steps
        ba_each = ba_ms / max(n_kf, 1)
        steady = {"ms_tracking_per_frame": track_ms, "ms_per_local_ba": ba_each, "local_ba_in_window": n_kf,
                  "local_ba_share_of_window": n_kf / args.steps, "steady_share": 1.0 / KF_INTERVAL,
                  "ms_per_step": track_ms + ba_each / KF_INTERVAL, "frames_per_s": 1e3 / (track_ms + ba_each / KF_INTERVAL),
                  "ms_waiting_for_extractor_per_frame": wait_ms / args.steps,
                  "what": "tracking (window time minus the time inside asd_local_ba) per frame + one LocalBA / kf_interval, from separately "
                          "accumulated host timers of this rank; `value` is K / window time with the window placed to hold ceil(K / kf_interval) LocalBAs"}

    # --full only: the variants and the CPU baselines below are passes of their own after the timed window, each an extra key.
    # The optional lane (asd_local_ba_submit): the same K frames once more with LocalBA running beside the next frames' tracking.  It
    # changes the data dependency (frames t+1.. read the pre-BA map), so it is reported as an extra key and never as `value`.
    lane_variant = None
    if args.full and world == 1 and not args.lane_ba and not args.no_lane_variant:
        be.async_ba = True
        if be.native is not None:
            be.native.lib.asd_track_set_async_ba(be.native.h, 1)
        be.hip.local_ba_submit(wl.ba); be.hip.local_ba_wait()      # untimed: the lane's thread + stream come into being here
        tl = prime + args.warmup + args.steps
        last, _ = run_steps(be, wl, tl, KF_INTERVAL, last, prefetch_beyond=True)
        be.hip.sync(); device_sync(device)
        l0 = time.perf_counter()
        last, _ = run_steps(be, wl, tl + KF_INTERVAL, args.steps, last, prefetch_beyond=True)
        be.hip.sync(); device_sync(device)
        ldt = time.perf_counter() - l0
        lane_variant = {"value": args.steps / ldt, "unit": "frames/s", "ms_per_step": 1e3 * ldt / args.steps, "steps": args.steps,
                        "what": "asd_local_ba_submit at the keyframe, own thread + stream, collected before the next submission and at the end "
                                "of the run; frames t+1.. are tracked against the map as it was BEFORE that LocalBA -- not the reference's "
                                "order, so poses on a real sequence differ from the reference's; optional entry point, never the headline"}
        be.async_ba = False
        if be.native is not None:
            be.native.lib.asd_track_set_async_ba(be.native.h, 0)

    # per-kernel device time of the dominant kernel (ASDNet conv2, f32 MFMA), hipEvents on the ctx stream
    layer_names = ["norm+conv1", "conv2", "conv3", "conv4", "conv5", "conv6", "conv7(fc)", "l2norm"]
    layers = {}
    for l, name in enumerate(layer_names):
        ms, calls, patches = be.hip.profile_get(l)
        layers[name] = {"avg_us": 1e3 * ms / max(calls, 1), "calls": calls, "patches_per_call": patches / max(calls, 1)}
    ms2, calls2, patches2 = be.hip.profile_get(1)
    achieved = (2.0 * L2_MACS * patches2) / (ms2 * 1e-3) / 1e12 if ms2 > 0 else 0.0
    asdnet_ms = sum(be.hip.profile_get(l)[0] for l in range(8)) / max(calls2, 1)
    split = bool(be.hip.asdnet_split_mask() & 1)   # conv2 on the split-operand kernel (default) or on the f32 MFMA kernel
    # roofline.traffic is NOT measured in this run: PMC counters need their own rocprofv3 passes (tools/collect_traffic.py).  The
    # figure is read from the committed summary of that tool for the same kernel family and labelled with its source.
    traffic, traffic_source = None, None
    tp = os.path.join(ROOT, "profiles", "traffic_conv2.json")
    if os.path.exists(tp):
        tj = json.load(open(tp))
        if ("k_conv_x3" in tj.get("kernel", "")) == split:   # PMC figure of the kernel family that actually ran
            traffic = tj.get("hbm_bytes_per_launch")
            traffic_source = "profiles/traffic_conv2.json (separate rocprofv3 --pmc passes via tools/collect_traffic.py; not measured in this run)"
    pieces = be.hip.asdnet_pieces()
    if split:
        # f32 work on the 16-bit matrix pipe: the ceiling for ALGORITHMIC f32 FLOP is the dense f16/bf16 peak / products per multiply-add
        nprod = SPLIT_PRODUCTS[pieces]
        form = "2 fp16 terms, 3 f16 MFMA products" if pieces == 2 else "3 bf16 terms, 6 bf16 MFMA products"
        peak = PEAK_BF16_MFMA_TFLOPS / nprod
        pair = pieces == 2 and os.environ.get("ASD_ASDNET_PAIR", "1") != "0"
        roof_kernel = (f"k_conv_x3<32,32,32,1,8,4,1,1,true,{pieces}{',true' if pair else ''}> (ASDNet input_norm+conv1+conv2; f32 operands split into {form} per "
                       f"multiply-add, f32 accumulate{'; output stored as the fp16 piece pairs of 16 x, 4 B per element like f32' if pair else ''})")
        roof_extra = {"peak_basis": f"dense f16/bf16 MFMA {PEAK_BF16_MFMA_TFLOPS} TFLOP/s / {nprod} products",
                      "executed_16bit_tflops": nprod * achieved, "vs_f32_mfma_peak": achieved / PEAK_F32_MFMA_TFLOPS}
    else:
        peak = PEAK_F32_MFMA_TFLOPS
        roof_kernel = "k_conv_mfma<32,32,32,1,...> (ASDNet conv2, f32 MFMA)"
        roof_extra = {}
    # Both stages as one submission (asd_track_frame): the host trip between the stages -- where the reference runs UpdateLocalMap() --
    # is gone, so the local map must be known before the frame is tracked.  The stand-in map allows that; the reference's Tracking does
    # not in general (include/asd_slam.h).  An extra key, never `value`.
    one_submission_variant = None
    if args.full and world == 1 and be.native is not None and not be.chain and not args.no_one_submission_variant:
        be.native.lib.asd_track_drain(be.native.h)
        be.native.lib.asd_track_set_chain(be.native.h, 1)
        tl = prime + args.warmup + 3 * args.steps + 8 * KF_INTERVAL
        while kf_in(tl + 2 * KF_INTERVAL, args.steps) < want_kf:
            tl += 1
        run_steps(be, wl, tl, 2 * KF_INTERVAL, None, prefetch_beyond=True)
        be.hip.sync(); device_sync(device)
        o0 = time.perf_counter()
        run_steps(be, wl, tl + 2 * KF_INTERVAL, args.steps, None, prefetch_beyond=True)
        be.hip.sync(); device_sync(device)
        odt = time.perf_counter() - o0
        one_submission_variant = {"value": args.steps / odt, "unit": "frames/s", "ms_per_step": 1e3 * odt / args.steps, "steps": args.steps,
                                  "local_ba_in_window": kf_in(tl + 2 * KF_INTERVAL, args.steps),
                                  "what": "asd_track_frame: both stages in one submission, the outlier drop / pose hand-over / skip flags between them on the "
                                          "device, the next frame constructed on a second stream (asd_prep_async).  Superset contract: the local map is a "
                                          "candidate list known BEFORE the frame is tracked -- valid for localisation against a fixed map or a caller that "
                                          "tracks against the previous frame's local map, NOT for Tracking::UpdateLocalMap as the reference runs it "
                                          "(Tracking.cc:730, between the stages)"}
        be.native.lib.asd_track_drain(be.native.h)
        be.native.lib.asd_track_set_chain(be.native.h, 0)

    # Larger local maps (Tracking.cc:881-905 collects every map point of up to 80 local keyframes): the headline form with 2 / 4 / 8 candidates
    # per point of the last frame = 4 k / 8 k / 16 k local-map candidates per frame.  Extra key; `value` keeps the 4 k stand-in.
    local_map_sweep = None
    if args.full and world == 1 and be.native is not None and not args.no_local_map_sweep:
        local_map_sweep = {"what": "the headline's two-call form with k candidates per point of the last frame in the stand-in local map (k x 2000 candidates per frame; "
                                   "the claim replay runs over the map points that have a candidate list, in chunks of 4096)", "runs": []}
        nsw = max(2 * KF_INTERVAL, args.steps // 2)
        for copies in (2, 4, 8):
            be.native.lib.asd_track_drain(be.native.h)
            be.native.lib.asd_track_set_map_copies(be.native.h, copies)
            tl = prime + args.warmup + 5 * args.steps + 16 * KF_INTERVAL
            run_steps(be, wl, tl, 2 * KF_INTERVAL, None, prefetch_beyond=True)
            be.hip.sync(); device_sync(device)
            tm_a = be.native.times()
            s0 = time.perf_counter()
            _, st_sw = run_steps(be, wl, tl + 2 * KF_INTERVAL, nsw, None, prefetch_beyond=True)
            be.hip.sync(); device_sync(device)
            sdt = time.perf_counter() - s0
            tm_b = be.native.times()
            local_map_sweep["runs"].append({"candidates_per_frame": copies * int(st_sw.get("n_kp", 0)), "value": nsw / sdt, "unit": "frames/s", "steps": nsw,
                                            "ms_tracking_per_frame": (1e3 * sdt - (tm_b[0] - tm_a[0])) / nsw, "local_map_matches_last_frame": int(st_sw.get("m2", 0))})
        be.native.lib.asd_track_drain(be.native.h)
        be.native.lib.asd_track_set_map_copies(be.native.h, 2)

    # The per-keyframe stage of LocalMapping::DoMapping in front of LocalBA (CreateNewMapPoints against 20 neighbours, SearchInNeighbors'
    # Fuse calls, distinctive descriptors) as the library's three batched submissions at every keyframe: reference order
    # (LocalMapping.cc:59-113).  An extra key: the metric -- and `value` -- is tracking + LocalBA.
    do_mapping_variant = None
    if args.full and world == 1 and be.native is not None and not args.no_do_mapping_variant:
        import ctypes as C
        D, dm_keep, dm_n = build_do_mapping_inputs(pkg, be.hip)
        be.native.lib.asd_track_set_do_mapping(be.native.h, C.byref(D), dm_n)
        tl = prime + args.warmup + 2 * args.steps + 4 * KF_INTERVAL
        while kf_in(tl + KF_INTERVAL, args.steps) < want_kf:
            tl += 1
        run_steps(be, wl, tl, KF_INTERVAL, None, prefetch_beyond=True)
        be.hip.sync(); device_sync(device)
        ms0, calls0 = C.c_double(), C.c_int64()
        be.native.lib.asd_track_get_do_mapping_times(be.native.h, C.byref(ms0), C.byref(calls0))
        d0 = time.perf_counter()
        run_steps(be, wl, tl + KF_INTERVAL, args.steps, None, prefetch_beyond=True)
        be.hip.sync(); device_sync(device)
        ddt = time.perf_counter() - d0
        ms1, calls1 = C.c_double(), C.c_int64()
        be.native.lib.asd_track_get_do_mapping_times(be.native.h, C.byref(ms1), C.byref(calls1))
        be.native.lib.asd_track_set_do_mapping(be.native.h, None, 0)
        nkf = max(1, calls1.value - calls0.value)
        do_mapping_variant = {"value": args.steps / ddt, "unit": "frames/s", "ms_per_step": 1e3 * ddt / args.steps, "steps": args.steps,
                              "keyframes": int(calls1.value - calls0.value), "ms_per_keyframe_stage": (ms1.value - ms0.value) / nkf,
                              "what": "the headline chain with LocalMapping::DoMapping's per-keyframe work in front of LocalBA at every keyframe (reference "
                                      "order, LocalMapping.cc:59-113): asd_create_map_points_batch (20 neighbours x 2000 keypoints), asd_fuse_search_batch "
                                      "(21 calls, 26400 candidate points, descriptors by bank row), asd_distinctive_descriptor_batch (600 points) on a "
                                      "stand-in neighbourhood"}

    # The same K frames with every image handed over in page-locked HOST memory (asd_extract_submit(device_resident = 0): the front
    # half's stream copies it, 467 KB per frame over PCIe) -- how kitti.cc:116-155 hands images to the tracker.  An extra key: `value`
    # keeps its definition (inputs resident in HBM when the timed region starts).
    h2d_variant = None
    if args.full and world == 1 and be.native is not None and not args.no_h2d_variant:
        be.native.lib.asd_track_drain(be.native.h)   # its read-ahead submissions go back to the library before another handle runs
        nh = NativeHost(pkg, be, wl, pipeline=not args.no_pipeline, frames_on_host=True)
        keep_native, be.native = be.native, nh
        tl = prime + args.warmup + args.steps
        run_steps(be, wl, tl, 2 * KF_INTERVAL, None, prefetch_beyond=True)
        be.hip.sync(); device_sync(device)
        h0 = time.perf_counter()
        run_steps(be, wl, tl + 2 * KF_INTERVAL, args.steps, None, prefetch_beyond=True)
        be.hip.sync(); device_sync(device)
        hdt = time.perf_counter() - h0
        h2d_variant = {"value": args.steps / hdt, "unit": "frames/s", "ms_per_step": 1e3 * hdt / args.steps, "steps": args.steps,
                       "local_ba_in_window": kf_in(tl + 2 * KF_INTERVAL, args.steps),
                       "what": "the same step with every frame's image (1241x376 u8) in page-locked host memory: host -> device copy on the "
                               "front half's stream inside the timed region"}
        nh.lib.asd_track_drain(nh.h)
        nh.close()
        be.native = keep_native

    be_chain = bool(be.chain)
    be.close()

    out = None
    if rank == 0:
        out = {
            "metric": "frames/sec end-to-end tracking+LocalBA, KITTI 00 mono @2000 keypoints",
            "value": frames_total / tmax, "unit": "frames/s", "n_gpus": world, "steps": args.steps,
            "warmup": args.warmup, "ms_per_step": 1e3 * tmax / args.steps, "higher_is_better": True,
            "scaling": "weak", "vs_baseline": None, "dtype": "f32", "data": "synthetic",
            "config": {"workload": "BASELINE configs[2]: KITTI-00-shaped synthetic stream 1241x376, 2000 kpts/frame, "
                                   "full HIP path: extract(E1-E7)+grid+SearchByProjection(frame)+PoseOptimization+"
                                   "isInFrustum+SearchByProjection(map)+PoseOptimization per frame, LocalBA "
                                   "(24+12 KF, 6000 MP, ~29k edges) every 15 frames",
                       "keypoints": int(stats.get("n_kp", 0)), "kf_interval": KF_INTERVAL,
                       "untimed": f"one LocalBA (solver buffers, lane) + {prime} priming frames + {args.warmup} warm-up frames",
                       "asdnet_math": (("f32 results on the f16 matrix pipe: every f32 operand = h + l in two fp16 terms (22 bits), products lh, hl, hh, f32 accumulate "
                                        if pieces == 2 else
                                        "f32 results on the bf16 matrix pipe: every f32 operand = exact sum of 3 bf16 terms, 6 cross products, f32 accumulate ") +
                                       "(error against a float64 forward at the level of the f32 MFMA chain, tests/test_asdnet.py; "
                                       "ASD_ASDNET_MATH=f16x2|bf16x3|f32 selects the kernels)") if split
                                      else "f32 MFMA (v_mfma_f32_32x32x2_f32)",
                       "parallelism": f"replicas x{world} (independent sequences, no collective)",
                       "host": "C++ host loop over the C ABI (asd-slam_amd/host/track_loop.cpp)" if args.host == "cxx" else "Python loop (ctypes)",
                       "stages": ("each asd_track_* stage run to completion" if (args.no_split or args.no_fuse or args.host != "cxx") else
                                  "two calls per frame, the host between them where Tracking::UpdateLocalMap sits (Tracking.cc:725-736): "
                                  "asd_track_motion_model_bank -> results on the host -> outlier drop, local-map stand-in selected from them -> "
                                  "asd_track_local_points_bank; split-phase (asd_track_async / asd_track_finish): the next frame's extraction hand-over, grid, "
                                  "descriptor adoption and read-ahead submission run under the local-map stage; the next frame's has_mp[] comes from this "
                                  "frame's final matches after asd_track_finish (Tracking.cc:296-349)"
                                  if not be_chain else
                                  "one submission per frame (asd_track_frame: motion-model stage, the outlier drop / pose hand-over / local-map selection between "
                                  "the stages on the device, local-map stage); the next frame is constructed (extraction hand-over, grid, descriptor adoption, "
                                  "map rows of the banks, read-ahead submission) on the context's second stream beside it (asd_prep_async)"),
                       "local_ba": ("on the library's optional lane (asd_local_ba_submit at the keyframe, own thread + stream; later frames read "
                                    "the pre-BA map: NOT the reference's order); every run is collected inside the timed region" if args.lane_ba else
                                    "in line (reference order): asd_local_ba at the keyframe, before the next frame is tracked "
                                    "(Tracking.cc:797 -> LocalMapping::DoMapping, LocalMapping.cc:59-113, BA at :89; the reference has no mapping thread)"),
                       "pipeline": f"ExtractDesc read-ahead of {LOOKAHEAD} frames on separate HIP streams (front half of t+2 under ASDNet of t+1 under tracking of t, one finished frame in hand)" if not args.no_pipeline else "none (sequential)"},
            "roofline": {"bound": "mfma", "kernel": roof_kernel,
                         "achieved": achieved, "peak": peak, "unit": "TFLOP/s",
                         "frac": achieved / peak, "traffic": traffic, "traffic_source": traffic_source,
                         "avg_launch_us": layers["conv2"]["avg_us"], "asdnet_forward_ms": asdnet_ms,
                         "asdnet_tflops": (2.0 * 39_092_224 * layers["conv2"]["patches_per_call"]) / (asdnet_ms * 1e-3) / 1e12 if asdnet_ms > 0 else 0.0,
                         **roof_extra},
            "asdnet_layers": layers,
            "last_step": stats,
        }
        if lane_variant is not None:
            out["lane_variant"] = lane_variant
        if one_submission_variant is not None:
            out["one_submission_variant"] = one_submission_variant
        if local_map_sweep is not None:
            out["local_map_sweep"] = local_map_sweep
        if h2d_variant is not None:
            out["h2d_variant"] = h2d_variant
        if do_mapping_variant is not None:
            out["do_mapping_variant"] = do_mapping_variant
        if steady is not None:
            out["steady_state"] = steady
        if args.full and args.cpu_frames > 0 and world == 1:   # reported baseline: rank 0 at N = 1 only
            cb = CpuBackend(pkg, wl)
            nf = args.cpu_frames
            cl, _ = run_steps(cb, wl, 0, 1, None)        # one untimed frame (torch warm-up, page-in)
            t0 = time.perf_counter()
            run_steps(cb, wl, KF_INTERVAL - nf, nf, cl)  # nf frames ending on a keyframe -> exactly one LocalBA
            cdt = time.perf_counter() - t0
            # BASELINE configs[0] (500 keypoints per frame, the reference's own CPU-runnable case): the same port, a shorter sample,
            # LocalBA on the 500-keypoint-scale problem of SURVEY 8(d) (1500 map points)
            cb5 = CpuBackend(pkg, wl, nfeatures=500)
            wl5 = Workload.__new__(Workload)
            wl5.__dict__.update(wl.__dict__)
            wl5.ba = pkg.synth.ba_problem(n_points=1500, seed=1)
            nf5 = max(2, min(nf, 8))
            cl5, _ = run_steps(cb5, wl5, 0, 1, None)
            t5 = time.perf_counter()
            run_steps(cb5, wl5, KF_INTERVAL - nf5, nf5, cl5)
            c5dt = time.perf_counter() - t5
            out["cpu_baseline_500"] = {"value": nf5 / c5dt, "unit": "frames/s", "cores": cb5.cores, "kind": "port",
                                       "sample": f"{nf5} frames at 500 keypoints per frame incl. 1 LocalBA (1500 map points): BASELINE configs[0]"}
            out["cpu_baseline"] = {
                "value": nf / cdt, "unit": "frames/s", "cores": cb.cores, "kind": "port",
                "sample": f"{nf} frames of the same workload incl. 1 LocalBA: oracle/ C++ restatement single-thread "
                          f"(front-end, matchers, pose optimisation), PyTorch-CPU ASDNet per level on {cb.torch.get_num_threads()} threads, "
                          + ("LocalBA by the reference's own g2o (oracle/_ref, single thread)" if cb.ref else "LocalBA by the oracle port"),
            }
            out["speedup_vs_cpu_baseline"] = out["value"] / out["cpu_baseline"]["value"]
        print(json.dumps(out))
    dist.close()
    if os.environ.get("ASD_DUMP_MAPS"):   # diagnostics: module load bases, to resolve a native stack printed at exit
        with open(os.environ["ASD_DUMP_MAPS"], "w") as f:
            f.write(open("/proc/self/maps").read())


if __name__ == "__main__":
    main()
