"""Cases shared by the culling tests: the hand-worked maps with their expected numbers written out (tests/test_culling_ref.py pins the
restatement on them, tests/test_culling.py runs the device on them), the random maps with octaves, and the ways a case reaches the
code under test."""
import numpy as np

from tests.culling_ref import CullingMap
from tests.local_map_cases import load as load_table
from tests.local_map_cases import random_map


def mk(kfs, octaves=None, bad_points=()):
    """kfs: keyframe -> point list; octaves: keyframe -> octave list (default: level 0 everywhere)"""
    m = CullingMap()
    for kf, pts in kfs.items():
        m.put_keyframe(kf, pts)
        m.put_octaves(kf, (octaves or {}).get(kf, [0] * len(pts)))
    m.pt_bad |= set(bad_points)
    return m


def _threshold(n_mps, n_red):
    """keyframe 1 holds n_mps points, of which the first n_red are observed by keyframes 2, 3 and 4 too"""
    pts = list(range(100, 100 + n_mps))
    return mk({1: pts, 2: pts[:n_red], 3: pts[:n_red], 4: pts[:n_red]})


def _cascade():
    """keyframe 10: point 200 (observed by 10, 11, 12) and ten redundant points; keyframe 11: point 200 and nine redundant points"""
    a, b = list(range(300, 310)), list(range(320, 329))
    kfs = {10: [200] + a, 11: [200] + b, 12: [200]}
    for kf in (20, 21, 22, 23):
        kfs[kf] = a + b
    return mk(kfs)


def hand_cases():
    """-> [(name, map, cand, flags, expected)]; expected = (decision, n_mps, n_redundant, bad_rows), worked by hand against
    LocalMapping.cc:739-809"""
    out = []
    four = {1: [100], 2: [100], 3: [100], 4: [100]}
    # the octave rule: three others at L + 1 make the point redundant, one of them at L + 2 does not
    out.append(("octave L+1", mk(four, {1: [2], 2: [3], 3: [3], 4: [3]}), [1], [0], ([1], [1], [1], [])))
    out.append(("octave L+2", mk(four, {1: [2], 2: [3], 3: [3], 4: [4]}), [1], [0], ([0], [1], [0], [])))
    # octave 15: L + 1 = 16 names no level and still compares
    out.append(("octave 15", mk(four, {1: [15], 2: [15], 3: [15], 4: [15]}), [1], [0], ([1], [1], [1], [])))
    out.append(("octave 14 under 15", mk(four, {1: [14], 2: [15], 3: [15], 4: [15]}), [1], [0], ([1], [1], [1], [])))
    out.append(("octave 13 under 15", mk(four, {1: [13], 2: [15], 3: [15], 4: [15]}), [1], [0], ([0], [1], [0], [])))
    # Observations() == 3 is not > 3
    out.append(("observations 3", mk({1: [100], 2: [100], 3: [100]}), [1], [0], ([0], [1], [0], [])))
    out.append(("observations 4", mk(four), [1], [0], ([1], [1], [1], [])))
    # the candidate's own observation is not one of the three: 4 observations, two others at a level <= 1
    out.append(("own observation", mk(four, {1: [0], 2: [0], 3: [0], 4: [5]}), [1], [0], ([0], [1], [0], [])))
    # nRedundantObservations > 0.9 nMPs
    out.append(("threshold 10 9", _threshold(10, 9), [1], [0], ([0], [10], [9], [])))
    out.append(("threshold 10 10", _threshold(10, 10), [1], [0], ([1], [10], [10], [])))
    out.append(("threshold 11 10", _threshold(11, 10), [1], [0], ([1], [11], [10], [110])))     # (its own point 110 is left with nobody)
    out.append(("threshold 0 0", mk({1: [-1, -1], 2: [100]}), [1], [0], ([0], [0], [0], [])))
    # id 0 and GetGlobalMapFlag() are skipped; 6 is judged with all five observations in place
    five = {0: [100], 5: [100], 6: [100], 7: [100], 8: [100]}
    out.append(("skipped", mk(five), [0, 5, 6], [0, 1, 0], ([3, 3, 1], [0, 0, 1], [0, 0, 1], [])))
    # mbNotErase: decision 2 erases nothing, so 7 still sees four observations; without it 6 goes and 7 is left with three
    pair = {5: [100], 6: [100], 7: [100], 8: [100]}
    out.append(("not erase", mk(pair), [6, 7], [2, 0], ([2, 1], [1, 1], [1, 1], [])))
    out.append(("order 6 7", mk(pair), [6, 7], [0, 0], ([1, 0], [1, 1], [1, 0], [])))
    out.append(("order 7 6", mk(pair), [7, 6], [0, 0], ([1, 0], [1, 1], [1, 0], [])))
    # culling 10 leaves point 200 with two observations: it turns bad, leaves 11's nMPs (10 -> 9), and only therefore 11 is culled
    out.append(("cascade", _cascade(), [10, 11], [0, 0], ([1, 1], [11, 9], [10, 9], [200])))
    out.append(("no cascade", _cascade(), [11], [0], ([0], [10], [9], [])))
    # a bad point (which still has entries) and a -1 entry count in no nMPs
    out.append(("bad and empty", mk({1: [100, -1, 101], 2: [100, 101], 3: [100], 4: [100]}, bad_points=[101]), [1], [0], ([1], [1], [1], [])))
    return out


def random_case(n_kf, n_kp, n_points, seed, fill, ids=None, row0=0, n_cand=30):
    """-> (CullingMap, candidates): tests.local_map_cases.random_map without bad keyframes, 3 % bad points; per keyframe a base level
    b in 0 .. 4 and octaves clip(b + U{-1 .. 2}, 0, 7); the candidates are a random permutation of up to n_cand ids"""
    m = CullingMap.from_map(random_map(n_kf, n_kp, seed, ids=ids, n_points=n_points, row0=row0, fill=fill, bad_kf=0, bad_pt=0.03))
    rng = np.random.default_rng(5000 + seed)
    kfs = sorted(m.kf_points)
    for kf in kfs:
        b = int(rng.integers(0, 5))
        m.put_octaves(kf, np.clip(b + rng.integers(-1, 3, n_kp), 0, 7))
    cand = [int(k) for k in rng.permutation(kfs)[:n_cand]]
    return m, cand


RANDOM_SHAPES = [(12, 16, 24, 0.7), (40, 48, 200, 0.8), (64, 64, 300, 0.7), (97, 64, 400, 0.8), (120, 47, 350, 0.7)]


def without_erasure(m, cand):
    """the rule evaluated per candidate on the map as it stands: what a reduction that ignores the in-loop SetBadFlag would cull"""
    return [int(m._copy().keyframe_culling([kf], [0], False)["decision"][0] == 1) for kf in cand]


def load(hip, m):
    """the whole CullingMap into a cleared observation table"""
    load_table(hip, m)
    for kf in sorted(m.octave):
        hip.map_put_octaves(kf, m.octave[kf])


def assert_same(got, exp):
    for k in ("decision", "n_mps", "n_redundant", "bad_rows"):
        assert [int(x) for x in got[k]] == [int(x) for x in exp[k]], k


def problem_text(m, calls, recent, n_current_kf_id, rows):
    """the problem file of host/test_culling: the map with its octaves, `calls` = [(cand, flags, apply)], the records of
    MapPointCulling and the rows whose Observations() the driver prints at the end"""
    out = [f"{len(m.kf_points)} {len(m.pt_bad)}"]
    for kf in sorted(m.kf_points):
        out.append(f"{kf} {int(kf in m.kf_bad)} {len(m.kf_points[kf])}")
        out.append(" ".join(str(int(x)) for x in m.kf_points[kf]))
        out.append(" ".join(str(int(x)) for x in m.octave[kf]))
    out.append(" ".join(str(p) for p in sorted(m.pt_bad)))
    out.append(str(len(calls)))
    for cand, flags, apply in calls:
        out.append(f"{len(cand)} {int(apply)}")
        out.append(" ".join(str(int(x)) for x in cand))
        out.append(" ".join(str(int(x)) for x in flags))
    out.append(f"{len(recent)} {n_current_kf_id}")
    for rec in recent:
        out.append(" ".join(str(int(x)) for x in rec))
    out.append(str(len(rows)))
    out.append(" ".join(str(int(x)) for x in rows))
    return "\n".join(out) + "\n"
