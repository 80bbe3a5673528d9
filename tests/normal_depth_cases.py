"""Cases shared by the UpdateNormalAndDepth tests: the hand-worked maps with their expected numbers written out as literals
(tests/test_normal_depth_ref.py pins the restatement on them, tests/test_normal_depth.py runs the device on them), and the ways a case
reaches the code under test.  Every hand case uses the default scale table (scaleFactor 1.2, 8 levels)."""
import numpy as np

from tests.culling_cases import mk
from tests.normal_depth_ref import BAD, NO_OBSERVATIONS, NO_REFERENCE, UPDATED

OLD = [9.0, 9.0, 9.0, -1.0, -2.0]     # normal, min, max of every row before a hand case runs: what an untouched row still holds
NAN = float("nan")


def bits(*words):
    return np.array(words, np.uint32).view(np.float32)


def _case(name, m, centres, pos, rows, ref_kf, status, normal, min_dist, max_dist):
    bank = np.zeros((max(pos) + 1, 8), np.float32)
    bank[:, 3:8] = OLD
    for r, p in pos.items():
        bank[r, 0:3] = p
    return dict(name=name, map=m, centres={k: np.array(c, np.float32) for k, c in centres.items()}, bank=bank, rows=rows, ref_kf=ref_kf,
                status=np.array(status, np.uint8), normal=np.array(normal, np.float32).reshape(-1, 3), min_dist=np.array(min_dist, np.float32),
                max_dist=np.array(max_dist, np.float32))


def hand_cases():
    out = []
    # one observer on the x axis, two units away, octave 1: normal (1, 0, 0), dist 2, max = 2 * 1.2f, min = max / 1.2^7 (3.5831816f)
    out.append(_case("axis", mk({1: [100]}, {1: [1]}), {1: [1, 0, 0]}, {100: [3, 0, 0]}, [100], [1], [UPDATED],
                     [[1.0, 0.0, 0.0]], bits(0x3f2b77bd), bits(0x4019999a)))                    # 0.66979581, 2.4000001
    # three observers whose f32 sum depends on the order in the last bit, put in the order 30, 10, 20; the walk is 10, 20, 30.
    # ref 20 at octave 3: d = (5, 6, 12), dist = sqrt(205) = 14.317822f, max = dist * 1.7280002f, min = max / 3.5831816f
    m = mk({30: [-1, 100], 10: [100], 20: [-1, -1, 100]}, {30: [0, 2], 10: [5], 20: [0, 0, 3]})
    out.append(_case("order", m, {10: [7, 3, 0], 20: [-4, -4, -9], 30: [-8, -9, -6]}, {100: [1, 2, 3]}, [100], [20], [UPDATED],
                     bits(0xb91a8555, 0x3e9df3a4, 0x3f1aead2), bits(0x40dcf43a), bits(0x41c5edf9)))   # 6.9048128, 24.741198
    # the four statuses.  100: observers 1 at (0, 0, 0) and 2 at (0, 3, 0), Pos (0, 3, 4): units (0, .6, .8) and (0, 0, 1), mean (0, .3, .9);
    # ref 1 at octave 0: dist 5, max 5, min 5 / 3.5831816f.  101 is bad; 103 is observed by nobody; 1 does not observe 102; 77 is no keyframe
    m = mk({1: [100, 101, -1], 2: [100, 102, 104]}, {1: [0, 1, 2], 2: [3, 4, 5]}, bad_points=[101])
    pos = {100: [0, 3, 4], 101: [1, 1, 1], 102: [2, 2, 2], 103: [3, 3, 3], 104: [4, 4, 4]}
    out.append(_case("statuses", m, {1: [0, 0, 0], 2: [0, 3, 0]}, pos, [101, 100, 103, 102, 104], [1, 1, 1, 1, 77],
                     [BAD, UPDATED, NO_OBSERVATIONS, NO_REFERENCE, NO_REFERENCE],
                     [OLD[:3], bits(0x0, 0x3e99999a, 0x3f666666), OLD[:3], OLD[:3], OLD[:3]],     # (0, 0.3f, 0.9f)
                     [OLD[3], bits(0x3fb29cba)[0], OLD[3], OLD[3], OLD[3]], [OLD[4], 5.0, OLD[4], OLD[4], OLD[4]]))   # 1.3954079
    # a point on a camera centre: 0 * inf = NaN in that observer's unit and so in the mean; the range comes from ref alone.
    # 100 sits on keyframe 1, ref 2 at (0, 0, 0), octave 2: dist 3, max 3 * 1.44f, min = max / 3.5831816f.  101 sits on its only observer: 0, 0
    m = mk({1: [100], 2: [100, 101]}, {1: [0], 2: [2, 0]})
    out.append(_case("on a centre", m, {1: [3, 0, 0], 2: [0, 0, 0]}, {100: [3, 0, 0], 101: [0, 0, 0]}, [100, 101], [2, 2], [UPDATED, UPDATED],
                     [[NAN, NAN, NAN], [NAN, NAN, NAN]], [bits(0x3f9a522a)[0], 0.0], [bits(0x408a3d71)[0], 0.0]))   # 1.2056324, 4.3200002
    return out


def load_all(hip, m, centres, bank):
    """the map with its octaves into a cleared observation table, the centres, and the bank rows [0, len(bank))"""
    from tests.culling_cases import load
    load(hip, m)
    kfs = sorted(centres)
    if kfs:
        hip.map_kf_centers(kfs, np.array([centres[k] for k in kfs], np.float32))
    hip.mpbank_put(0, bank[:, 0:3], bank[:, 3:6], bank[:, 6], bank[:, 7])


def ref_kfs(m, rows, seed):
    """an mpRefKF per point: one of its observers (the lowest id for a point nobody observes has no meaning: keyframe 0 then)"""
    rng = np.random.default_rng(seed)
    out = []
    for r in rows:
        obs = sorted(m.obs.get(int(r), {}))
        out.append(obs[int(rng.integers(len(obs)))] if obs else 0)
    return out


def problem_text(m, centres, bank, calls):
    """the problem file of host/test_normal_depth: the map with octaves and centres, the bank rows, `calls` = [(rows, ref_kf, Xw or None)]"""
    out = [f"{len(m.kf_points)} {len(m.pt_bad)} {len(bank)}"]
    for kf in sorted(m.kf_points):
        c = centres[kf]
        out.append(f"{kf} {len(m.kf_points[kf])} {float(c[0])!r} {float(c[1])!r} {float(c[2])!r}")
        out.append(" ".join(str(int(x)) for x in m.kf_points[kf]))
        out.append(" ".join(str(int(x)) for x in m.octave[kf]))
    out.append(" ".join(str(p) for p in sorted(m.pt_bad)))
    for row in bank:
        out.append(" ".join(repr(float(x)) for x in row))
    out.append(str(len(calls)))
    for rows, ref, Xw in calls:
        out.append(f"{len(rows)} {int(Xw is not None)}")
        out.append(" ".join(str(int(x)) for x in rows))
        out.append(" ".join(str(int(x)) for x in ref))
        if Xw is not None:
            out.append(" ".join(repr(float(x)) for x in np.asarray(Xw, np.float32).ravel()))
    return "\n".join(out) + "\n"
