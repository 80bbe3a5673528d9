"""Case builder shared by the local-map tests: random maps that satisfy the table's precondition (a point at most once per keyframe),
the frames queried against them, and the two ways a case reaches the code under test (the ctypes binding, the C++ driver's problem file)."""
import numpy as np

from tests.local_map_ref import RefMap


def random_map(n_kf, n_kp, seed, ids=None, n_points=None, row0=0, fill=0.7, absent_links=True, bad_kf=0.08, bad_pt=0.05):
    """-> RefMap of n_kf keyframes with n_kp keypoints each.  ids: the keyframe ids (default 0 .. n_kf-1); points are bank rows
    row0 .. row0 + n_points - 1; links name other keyframes and, with absent_links, ids the map does not hold."""
    rng = np.random.default_rng(seed)
    ids = list(range(n_kf)) if ids is None else [int(i) for i in ids]
    n_points = n_points or max(8, n_kf * n_kp // 4)
    m = RefMap()
    centre = rng.uniform(0, n_points, n_kf)
    for k, kf in enumerate(ids):
        n_obs = min(int(fill * n_kp), n_points)
        # keyframes see a window of the point range, so neighbours in the list share points and far ones do not
        w = min(n_points, max(n_obs * 2, n_points // 6))
        pool = (np.arange(w) + int(centre[k])) % n_points
        pts = rng.choice(pool, n_obs, replace=False)
        row = np.full(n_kp, -1, np.int64)
        row[rng.choice(n_kp, n_obs, replace=False)] = pts + row0
        m.put_keyframe(kf, row)
    held = set(ids)                                       # three ids the map does not hold (inside int32)
    start = max(ids) + 1000 if max(ids) < 2 ** 31 - 2000 else 1
    far = [x for x in range(start, start + n_kf + 4) if x not in held][:3]
    for kf in ids:
        others = [i for i in ids if i != kf]
        pool = others + (far if absent_links else [])
        cov = list(rng.choice(pool, min(len(pool), int(rng.integers(0, 11))), replace=False))
        ch = list(rng.choice(pool, min(len(pool), int(rng.integers(0, 5))), replace=False))
        par = int(rng.choice(pool)) if rng.uniform() < 0.8 else -1
        m.set_links(kf, cov, ch, par)
        if rng.uniform() < bad_kf:
            m.kf_bad.add(kf)
    for p in range(row0, row0 + n_points):
        if rng.uniform() < bad_pt:
            m.pt_bad.add(p)
    return m


def random_frame(m, n_cur, seed, around=None, n_seen=6):
    """-> (cur_rows, seen_rows): the frame holds points of a few keyframes (some twice, some bad, some keypoints without a point), and
    carries stage-1 outliers' points in seen_rows"""
    rng = np.random.default_rng(seed)
    kfs = sorted(m.kf_points)
    base = kfs[int(rng.integers(len(kfs)))] if around is None else around
    near = [k for k in kfs if abs(kfs.index(k) - kfs.index(base)) <= 2]
    pool = np.array(sorted({p for k in near for p in m.kf_points[k] if p >= 0}), np.int64)
    cur = np.full(n_cur, -1, np.int64)
    if len(pool):
        take = rng.choice(pool, min(len(pool), n_cur // 2), replace=False)
        cur[rng.choice(n_cur, len(take), replace=False)] = take
        free = np.nonzero(cur < 0)[0]
        dup = min(3, len(free), len(take))
        cur[free[:dup]] = take[:dup]                     # a point the frame holds twice votes twice
    seen = rng.choice(pool, min(n_seen, len(pool)), replace=False) if len(pool) else np.zeros(0, np.int64)
    return cur.astype(np.int32), np.asarray(seen, np.int32)


def load(hip, m):
    """the whole RefMap into a cleared observation table"""
    hip.map_clear()
    for kf in sorted(m.kf_points):
        hip.map_put(kf, m.kf_points[kf])
    for kf in sorted(m.kf_points):
        hip.map_kf_links(kf, m.cov.get(kf, []), m.children.get(kf, []), m.parent.get(kf, -1))
        if kf in m.kf_bad:
            hip.map_kf_bad(kf, True)
    if m.pt_bad:
        hip.map_point_bad(sorted(m.pt_bad), True)


def assert_same(got, exp):
    assert list(got["local_kfs"]) == list(exp["local_kfs"])
    assert int(got["ref_kf"]) == int(exp["ref_kf"])
    assert list(got["local_rows"]) == list(exp["local_rows"])
    assert list(got["search_rows"]) == list(exp["search_rows"])


def problem_text(m, queries, connections):
    """the problem file of host/test_local_map: the map, then `queries` = [(cur_rows, seen_rows, prev_kfs, max_kfs)] and
    `connections` = keyframe ids for UpdateConnections"""
    out = [f"{len(m.kf_points)} {len(m.pt_bad)}"]
    for kf in sorted(m.kf_points):
        row, cov, ch = m.kf_points[kf], m.cov.get(kf, []), m.children.get(kf, [])
        out.append(f"{kf} {int(kf in m.kf_bad)} {m.parent.get(kf, -1)} {len(row)} {len(cov)} {len(ch)}")
        out.append(" ".join(str(int(x)) for x in row))
        out.append(" ".join(str(int(x)) for x in cov))
        out.append(" ".join(str(int(x)) for x in ch))
    out.append(" ".join(str(p) for p in sorted(m.pt_bad)))
    out.append(str(len(queries)))
    for cur, seen, prev, max_kfs in queries:
        out.append(f"{len(cur)} {len(seen)} {len(prev)} {max_kfs}")
        for v in (cur, seen, prev):
            out.append(" ".join(str(int(x)) for x in v))
    out.append(str(len(connections)))
    out.append(" ".join(str(int(k)) for k in connections))
    return "\n".join(out) + "\n"
