"""The active structure of a bundle adjustment round (asd-slam_amd/csrc/ba_structure.h) stated from its definition, with sorting and
dictionaries -- not the loops of the header.

  pose_h      rank of a pose among the non-fixed poses that have an edge, else -1
  pt_h        rank of a point among the points that have an edge, else -1
  act         the edges sorted by (pt_h of their point, pose_h of their pose -- fixed = -1 --, edge id); pt_start = where each landmark begins
  ps_edges    per free pose, the act positions of its edges in ascending order; ps_h = the landmark of each
  blocks      (i, j) with i <= j row-major: all of them, or the diagonal ones plus the off-diagonal ones that have a pair
  pairs       per block, ordered by (landmark, a, b): act positions a <= b of two edges of one landmark to free poses i = pose of a,
              j = pose of b; for i == j and a != b the pair (b, a) directly behind (a, b); pair_h = the landmark of each pair
"""
from itertools import combinations_with_replacement


def structure(P, L, fixed, e_pose, e_point, all_blocks):
    E = len(e_pose)
    free = sorted({p for p in e_pose if not fixed[p]})
    seen = sorted(set(e_point))
    pose_h = [free.index(p) if p in free else -1 for p in range(P)]
    pt_h = [seen.index(l) if l in seen else -1 for l in range(L)]
    act = sorted(range(E), key=lambda e: (pt_h[e_point[e]], pose_h[e_pose[e]], e))
    lm = [pt_h[e_point[e]] for e in act]        # landmark of every act position
    ph = [pose_h[e_pose[e]] for e in act]       # pose h-index of every act position
    pt_start = [sum(h < x for h in lm) for x in range(len(seen) + 1)]
    per_pose = {i: [k for k in range(E) if ph[k] == i] for i in range(len(free))}
    ps_start, ps_edges = [0], []
    for i in range(len(free)):
        ps_edges += per_pose[i]
        ps_start.append(len(ps_edges))
    ps_h = [lm[k] for k in ps_edges]
    in_block = {}
    for a, b in combinations_with_replacement(range(E), 2):     # a <= b, lexicographic; within a landmark act order = landmark order
        if lm[a] == lm[b] and ph[a] >= 0 and ph[b] >= 0:
            lst = in_block.setdefault((ph[a], ph[b]), [])       # (ph[a] <= ph[b]: act is sorted by pose inside a landmark)
            lst.append((lm[a], a, b))
            if ph[a] == ph[b] and a != b:
                lst.append((lm[a], b, a))
    n = len(free)
    blocks = [(i, j) for i in range(n) for j in range(i, n) if all_blocks or i == j or (i, j) in in_block]
    pair_start, pairs, pair_h = [0], [], []
    for blk in blocks:
        lst = sorted(in_block.get(blk, []), key=lambda t: (t[0], min(t[1], t[2]), max(t[1], t[2]), t[1] > t[2]))
        pairs += [(a, b) for _, a, b in lst]
        pair_h += [h for h, _, _ in lst]
        pair_start.append(len(pairs))
    return {"counts": [n, len(seen), E, len(blocks), len(pairs)], "pose_h": pose_h, "pt_h": pt_h, "pose_of_h": free, "pt_of_h": seen,
            "pt_start": pt_start, "act": act, "ps_start": ps_start, "ps_edges": ps_edges, "ps_h": ps_h,
            "blk_i": [i for i, _ in blocks], "blk_j": [j for _, j in blocks], "pair_start": pair_start, "pairs": pairs, "pair_h": pair_h}
