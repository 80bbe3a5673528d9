"""Times one loop query of the keyframe database at map size (default 4096 keyframes x 1500 words) on the GPU -- the "kfdb" stage
(device events around the upload and the scoring kernel) and the wall time of asd_kfdb_query_loop + asd_kfdb_select -- and the same
query in the CPU implementation's form (tools/kfdb_query_cpu.cpp: inverted lists, std::list, std::map, -O2) on the same host.

    python tools/kfdb_query_time.py [--entries 4096] [--words 1500] [--reps 200] [--out FILE]

The candidates of the library and of the CPU program are compared through a checksum."""
import argparse
import json
import os
import struct
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as entry  # noqa: E402


def make_db(n_entries, n_words, n_vocab, seed):
    """keyframes in groups of 8 per place: 70 % of a keyframe's words come from its place's pool (2 x n_words words), the rest from
    the whole vocabulary, as the words of revisited places and of clutter do"""
    rng = np.random.default_rng(seed)
    n_places = (n_entries + 7) // 8
    pools = [rng.choice(n_vocab, 2 * n_words, replace=False) for _ in range(n_places)]

    def one(place):
        own = rng.choice(pools[place], int(0.7 * n_words), replace=False)
        ids = np.unique(np.concatenate([own, rng.integers(0, n_vocab, n_words - len(own))])).astype(np.int32)
        vals = rng.uniform(0.2, 3.0, len(ids))
        return ids, vals / vals.sum()

    entries = [one(i // 8) for i in range(n_entries)]
    queries = [one(int(p)) for p in rng.integers(0, n_places, 16)]
    return entries, queries


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--entries", type=int, default=4096)
    ap.add_argument("--words", type=int, default=1500)
    ap.add_argument("--vocab", type=int, default=1000000)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    pkg = entry.load_package()
    entries, queries = make_db(a.entries, a.words, a.vocab, 0)
    hip = pkg.AsdHip(n_features=2000, max_width=1241, max_height=376, max_patches=4096)
    res = dict(entries=a.entries, words_per_entry=a.words, vocabulary=a.vocab, reps=a.reps)
    try:
        hip.kfdb_clear(0)
        t0 = time.perf_counter()
        for i, e in enumerate(entries):
            hip.kfdb_add(i, e)
        res["add_ms_per_keyframe"] = (time.perf_counter() - t0) * 1e3 / len(entries)

        def neigh(kf):
            return [j for j in range(kf - 5, kf + 6) if j != kf and 0 <= j < a.entries]

        def query(q):
            kf, sc = hip.kfdb_query_loop(q, [], 0.01)
            return kf, hip.kfdb_select(0, [neigh(int(k)) for k in kf])

        for q in queries:   # warm-up: code objects, staging buffers at their final size
            query(q)
        stage, wall, wall_query, checksum, n_scored = [], [], [], 0, 0
        for r in range(a.reps):
            q = queries[r % len(queries)]
            t0 = time.perf_counter()
            kf, sc = hip.kfdb_query_loop(q, [], 0.01)
            t1 = time.perf_counter()
            cand = hip.kfdb_select(0, [neigh(int(k)) for k in kf])
            t2 = time.perf_counter()
            stage.append(hip.last_stage_ms("kfdb"))
            wall_query.append((t1 - t0) * 1e3)
            wall.append((t2 - t0) * 1e3)
            checksum += int(cand.sum()) + len(cand)
            n_scored += len(kf)
        res.update(kfdb_stage_ms_median=float(np.median(stage)), kfdb_stage_ms_min=float(np.min(stage)), kfdb_stage_ms_max=float(np.max(stage)),
                   query_call_wall_ms_median=float(np.median(wall_query)), query_and_select_wall_ms_median=float(np.median(wall)),
                   query_and_select_wall_ms_p90=float(np.percentile(wall, 90)), scored_per_query=n_scored / a.reps, checksum=checksum)
        # eight named entries: DetectLoop's minScore loop
        t0 = time.perf_counter()
        for r in range(50):
            hip.kfdb_score(queries[r % len(queries)], list(range(8)))
        res["score_8_entries_wall_ms"] = (time.perf_counter() - t0) * 1e3 / 50
    finally:
        hip.close()
    exe = os.path.join(ROOT, "tools", "kfdb_query_cpu")
    if not os.path.exists(exe):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-o", exe, exe + ".cpp"])
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "db.bin")
        with open(path, "wb") as f:
            f.write(struct.pack("<3i", a.vocab, len(entries), len(queries)))
            for ids, vals in entries + queries:
                f.write(struct.pack("<i", len(ids)) + ids.astype("<i4").tobytes() + vals.astype("<f8").tobytes())
        cpu = json.loads(subprocess.check_output([exe, path, str(a.reps)]).decode())
    res.update(cpu_query_ms=cpu["cpu_query_ms"], cpu_checksum=cpu["checksum"], candidates_agree=cpu["checksum"] == checksum)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
