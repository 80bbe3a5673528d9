"""numpy / plain-Python restatement of the extractor front half, ORBextractor::ExtractDesc up to the patch gather
(ORBextractor.cc), for tests/test_frontend_exits.py.  Written from the reference's source text, independently of
oracle/frontend.cpp, of csrc/frontend.hip and of csrc/quadtree.cpp:

  constructor tables       (:452-512)    scale / sigma tables, per-level quotas, umax
  ComputePyramid           (:1251-1276)  level sizes cvRound(float(w) * inv_scale), every level resized from the previous one
  ComputeKeyPointsOctTree  (:813-904)    the cell loop, literally: one window per cell, cv::FAST on the window alone
  DistributeOctTree        (:587-811)    lists of nodes that own lists of keys;  DivideNode (:529-585)
  IC_Angle                 (:80-107)     integer moments over the umax disc, cv::fastAtan2
  ExtractDesc tail         (:1217-1245)  GaussianBlur 7x7, the 32 x 32 patch (:1113-1115), rescale, level-major output

OpenCV is not available here, so the arithmetic INSIDE the OpenCV 3.2.0 calls (cv::resize's 11-bit fixed point, the 8-bit
Gaussian kernel and its fixed-point column pass, cornerScore<16>, fastAtan2's polynomial) is taken from the same statement
the rest of the project uses: oracle/frontend.cpp's header and DESIGN.md section 2.  PARITY UNPINNED for those.  What is
independent here is the structure: whole-array integer numpy for resize and blur, the FAST score straight from its
definition (maximum over the 16 arcs of the one-sided minimum -- no early exits, no doubling), a window cut per cell and
scored and suppressed inside that window alone (no score map shared between cells, no "interior" of a cell), Python lists
for the quadtree, f32 one operation per step (np.float32 scalars: numpy never fuses a multiply into an add).

Where the reference has undefined behaviour the library defines the result and this file states the same rule:
  * SORT RULE: :732 sorts pair<int, ExtractorNode*>, so equal sizes are ordered by pointer value.  The library orders equal
    sizes by node creation order (what a monotonically growing heap gives the reference); see _sort_key.
  * TALL IMAGE: nIni = round(width / height) < 1 makes :593 divide by zero.  The library returns no keypoints for that
    level; its raw corners are still listed.
  * LEVEL WITHOUT CELLS: nCols < 1 or nRows < 1 makes :835-836 divide by zero.  The library finds no corners there.
  * ROOT CLAMP: :617 indexes vpIniNodes[kp.pt.x / hX] unchecked.  The library clamps the index to nIni - 1; see the
    argument at `root_clamp` below for why no key can reach it.

Every branch the extraction takes is counted, in source order (COUNTERS).  The small module-level functions and constants
(_is_corner, _nms_greater, SKIP_X, _sort_key, ...) are the places a test mutates to show that its inputs discriminate.
"""
import operator

import numpy as np

F32 = np.float32
PATCH_SIZE, HALF_PATCH_SIZE, EDGE_THRESHOLD = 31, 15, 19
CELL_W = F32(30)
SKIP_X, SKIP_Y = 6, 3            # :851 `iniX >= maxBorderX-6`, :842 `iniY >= maxBorderY-3`
FIRST_SCALED_LEVEL_TEST = operator.ne   # :1236 `if (level != 0)`

KP_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"), ("response", "<f4"), ("octave", "<i4")])

_ATAN_NAMES = tuple(f"atan_{rel}_x{sx}_y{sy}" for rel in ("gt", "lt", "tie") for sx in "pn" for sy in "pn")
COUNTERS = (
    # ---- ComputeKeyPointsOctTree
    "level_no_cells",            # nCols < 1 || nRows < 1 (library rule)
    "row_skipped_y",             # :842
    "cell_skipped_x",            # :851
    "window_under_7",            # cv::FAST on a window narrower or lower than 7 finds nothing
    "interior_w1", "interior_w2", "interior_w3",   # window width 7 / 8 / 9: 1 / 2 / 3 columns a corner can sit on
    "cell_first_pass_hit",       # :858 found corners at iniThFAST
    "retry_taken",               # :861
    "retry_empty_again",         # :863 found nothing either
    # ---- DistributeOctTree
    "nini_lt_1",                 # library rule
    "root_boundary_key",         # :617 kp.pt.x / hX is a whole number >= 1: the key belongs to the root on its right
    "root_clamp",                # :617 index >= nIni.  UNREACHABLE: a corner's x is at most w - 36 (FAST needs 3 pixels inside a
                                 # window that ends at maxBorderX = w - 16, minBorderX = 16 is subtracted), hX * nIni = w - 32, so
                                 # x / hX <= nIni * (w - 36) / (w - 32) < nIni - 4 * nIni / w, far more than an f32 rounding below nIni
    "root_empty",                # :629
    "root_single",               # :624
    "stop_no_growth",            # :717 lNodes.size() == prevSize (fewer corners than N: every node holds one key)
    "stop_n_first_sweep",        # :717 lNodes.size() >= N
    "first_sweep_again",         # neither :717 nor :721: another sweep over all nodes
    "second_phase",              # :721
    "second_break_mid",          # :778 break with nodes of the sorted list still unsplit
    "second_stop_n",             # :782 >= N
    "second_stop_no_growth",     # :782 == prevSize
    "second_phase_repeat",       # :724 the loop runs again
    "sort_equal_sizes",          # :732 two entries of one sorted list have the same size (SORT RULE applies)
    "sort_tie_decides",          # ... and the break of :778 falls between two of them: the tie chose which node was split
    "pick_equal_responses",      # :800 the maximum response of a final node is shared: the first in list order wins
    # ---- fastAtan2 (m_01, m_10)
    "atan_zero", "atan_x0_yp", "atan_x0_yn", "atan_y0_xp", "atan_y0_xn",
) + _ATAN_NAMES                  # gt: |x| > |y|, lt: |x| < |y|, tie: |x| == |y|; sign of x (m_10) and of y (m_01)


def new_counters():
    return {k: 0 for k in COUNTERS}


def cv_round(v):
    """cvRound: lrint of a double, ties to even"""
    return int(np.rint(np.float64(v)))


# ------------------------------------------------------------------ constructor (:452-512)
def tables(n_features, scale_factor, n_levels):
    sf = np.float64(F32(scale_factor))          # `double scaleFactor` initialised from the float argument
    scale = np.zeros(n_levels, F32)
    sigma2 = np.zeros(n_levels, F32)
    scale[0] = sigma2[0] = F32(1)
    for i in range(1, n_levels):
        scale[i] = F32(np.float64(scale[i - 1]) * sf)
        sigma2[i] = scale[i] * scale[i]
    inv_scale = F32(1) / scale
    inv_sigma2 = F32(1) / sigma2
    factor = F32(np.float64(1.0) / sf)
    n_desired = F32(F32(n_features) * (F32(1) - factor)) / (F32(1) - F32(np.float64(factor) ** np.float64(n_levels)))
    quota = np.zeros(n_levels, np.int32)
    total = 0
    for level in range(n_levels - 1):
        quota[level] = cv_round(n_desired)
        total += int(quota[level])
        n_desired = n_desired * factor
    quota[n_levels - 1] = max(n_features - total, 0)
    half_diag = F32(HALF_PATCH_SIZE) * np.sqrt(F32(2)) / F32(2)
    vmax = int(np.floor(half_diag + F32(1)))
    vmin = int(np.ceil(half_diag))
    umax = np.zeros(HALF_PATCH_SIZE + 1, np.int32)
    for v in range(vmax + 1):
        umax[v] = cv_round(np.sqrt(np.float64(HALF_PATCH_SIZE * HALF_PATCH_SIZE - v * v)))
    v0 = 0
    for v in range(HALF_PATCH_SIZE, vmin - 1, -1):
        while umax[v0] == umax[v0 + 1]:
            v0 += 1
        umax[v] = v0
        v0 += 1
    return dict(scale=scale, inv_scale=inv_scale, sigma2=sigma2, inv_sigma2=inv_sigma2, features_per_level=quota, umax=umax)


# ------------------------------------------------------------------ cv::resize 8U INTER_LINEAR, whole arrays
def _resize_coeffs(src_n, dst_n, clamp):
    scale = 1.0 / (np.float64(dst_n) / np.float64(src_n))
    f = ((np.arange(dst_n, dtype=np.float64) + 0.5) * scale - 0.5).astype(F32)
    s = np.floor(f).astype(np.int64)
    f = f - s.astype(F32)
    if clamp:                                      # the x table: outside columns take the border pixel with weight 1
        lo, hi = s < 0, s >= src_n - 1
        f = np.where(lo | hi, F32(0), f)
        s = np.where(lo, 0, np.where(hi, src_n - 1, s))
    c0 = np.clip(np.rint(((F32(1) - f) * F32(2048)).astype(np.float64)), -32768, 32767).astype(np.int64)
    c1 = np.clip(np.rint((f * F32(2048)).astype(np.float64)), -32768, 32767).astype(np.int64)
    return s, c0, c1


def resize_linear(src, dw, dh):
    sh, sw = src.shape
    S = src.astype(np.int64)
    sx, a0, a1 = _resize_coeffs(sw, dw, True)
    sy, b0, b1 = _resize_coeffs(sh, dh, False)
    rows = S[:, sx] * a0[None, :] + S[:, np.minimum(sx + 1, sw - 1)] * a1[None, :]     # [sh, dw], horizontal pass
    r0 = rows[np.clip(sy, 0, sh - 1)]
    r1 = rows[np.clip(sy + 1, 0, sh - 1)]
    out = (((b0[:, None] * (r0 >> 4)) >> 16) + ((b1[:, None] * (r1 >> 4)) >> 16) + 2) >> 2
    return out.astype(np.uint8)


def pyramid(image, inv_scale):
    h, w = image.shape
    levels = []
    for level, s in enumerate(inv_scale):
        lw, lh = cv_round(F32(w) * s), cv_round(F32(h) * s)
        levels.append(np.array(image, np.uint8) if level == 0 else resize_linear(levels[level - 1], lw, lh))
        assert levels[level].shape == (lh, lw)
    return levels


# ------------------------------------------------------------------ cv::GaussianBlur 7x7, sigma 2, 8U
def _border_index(p, n):
    """BORDER_REFLECT_101: ... 2 1 | 0 1 2 ... n-1 | n-2 n-3 ..."""
    if n == 1:
        return 0
    while p < 0 or p >= n:
        p = -p if p < 0 else 2 * n - 2 - p
    return p


def gauss_kernel7():
    x = np.arange(7, dtype=np.float64) - 3.0
    cf = np.exp(-0.5 / (2.0 * 2.0) * x * x).astype(F32)
    inv = 1.0 / np.sum(cf.astype(np.float64))
    cf = (cf.astype(np.float64) * inv).astype(F32)
    return [cv_round(c * F32(256)) for c in cf]


def gaussian_blur7(img):
    h, w = img.shape
    k = gauss_kernel7()
    S = img.astype(np.int64)
    cols = [np.array([_border_index(x + i - 3, w) for x in range(w)]) for i in range(7)]
    tmp = sum(k[i] * S[:, cols[i]] for i in range(7))
    rows = [np.array([_border_index(y + i - 3, h) for y in range(h)]) for i in range(7)]
    acc = sum(k[i] * tmp[rows[i], :] for i in range(7))
    return np.clip((acc + (1 << 15)) >> 16, 0, 255).astype(np.uint8)


# ------------------------------------------------------------------ cv::FAST (9 of 16, non-max suppression) on one window
RING = ((0, 3), (1, 3), (2, 2), (3, 1), (3, 0), (3, -1), (2, -2), (1, -3),
        (0, -3), (-1, -3), (-2, -2), (-3, -1), (-3, 0), (-3, 1), (-2, 2), (-1, 3))


def arc_strength(win):
    """For every pixel at least 3 inside `win`: the largest t such that 9 contiguous ring pixels are all darker than v - t + 1 or all
    brighter than v + t - 1, i.e. max over the 16 arcs of min over the arc of (v - p), and the same for (p - v).  [h-6, w-6] int."""
    h, w = win.shape
    W = win.astype(np.int32)
    v = W[3:h - 3, 3:w - 3]
    d = [v - W[3 + dy:h - 3 + dy, 3 + dx:w - 3 + dx] for dx, dy in RING]
    best = np.full(v.shape, -256, np.int32)
    for k in range(16):
        arc = np.stack([d[(k + i) % 16] for i in range(9)])
        best = np.maximum(best, np.maximum(arc.min(axis=0), (-arc).min(axis=0)))
    return best


def _is_corner(strength, th):
    """the segment test at threshold th: 9 contiguous pixels differ from the centre by MORE than th"""
    return strength > th


_nms_greater = np.greater        # :fast.cpp `score > neighbour`, all eight


def fast_window(win, th):
    """cv::FAST(win, keys, th, true) -> ([(x, y, score)] in row-major order, number of pixels that pass the segment test).
    cornerScore of a corner = its arc strength - 1; non-corners score 0; a corner survives if its score is greater than all
    eight neighbours' inside the window."""
    h, w = win.shape
    if w < 7 or h < 7:
        return [], 0
    strength = arc_strength(win)
    corner = _is_corner(strength, th)
    score = np.zeros((h, w), np.int32)
    score[3:h - 3, 3:w - 3] = np.where(corner, strength - 1, 0)
    keep = np.zeros((h, w), bool)
    keep[3:h - 3, 3:w - 3] = corner
    c = score[1:h - 1, 1:w - 1]
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            if dx or dy:
                keep[1:h - 1, 1:w - 1] &= _nms_greater(c, score[1 + dy:h - 1 + dy, 1 + dx:w - 1 + dx])
    ys, xs = np.nonzero(keep)
    return [(int(x), int(y), int(score[y, x])) for y, x in zip(ys, xs)], int(corner.sum())


def _detect_window(level_img, x0, y0, x1, y1, th):
    """FAST(mvImagePyramid[level].rowRange(iniY, maxY).colRange(iniX, maxX), ...): the window is all cv::FAST sees"""
    return fast_window(level_img[y0:y1, x0:x1], th)


def _retry_needed(keys, n_passing):
    """:861 `if (vKeysCell.empty())` -- the list AFTER non-max suppression"""
    return len(keys) == 0


def cell_corners(level_img, ini_th, min_th, cnt):
    """the cell loop of ComputeKeyPointsOctTree (:817-879) -> [(x, y, response)] relative to minBorder, in list order"""
    rows, cols = level_img.shape
    min_bx = min_by = EDGE_THRESHOLD - 3
    max_bx, max_by = cols - EDGE_THRESHOLD + 3, rows - EDGE_THRESHOLD + 3
    width, height = F32(max_bx - min_bx), F32(max_by - min_by)
    n_cols, n_rows = int(width / CELL_W), int(height / CELL_W)
    keys = []
    if n_cols < 1 or n_rows < 1:
        cnt["level_no_cells"] += 1
        return keys
    w_cell, h_cell = int(np.ceil(width / F32(n_cols))), int(np.ceil(height / F32(n_rows)))
    for i in range(n_rows):
        ini_y = F32(min_by + i * h_cell)
        max_y = ini_y + F32(h_cell + 6)
        if ini_y >= max_by - SKIP_Y:
            cnt["row_skipped_y"] += 1
            continue
        if max_y > max_by:
            max_y = F32(max_by)
        for j in range(n_cols):
            ini_x = F32(min_bx + j * w_cell)
            max_x = ini_x + F32(w_cell + 6)
            if ini_x >= max_bx - SKIP_X:
                cnt["cell_skipped_x"] += 1
                continue
            if max_x > max_bx:
                max_x = F32(max_bx)
            box = (int(ini_x), int(ini_y), int(max_x), int(max_y))
            cw, ch = box[2] - box[0], box[3] - box[1]
            if cw < 7 or ch < 7:
                cnt["window_under_7"] += 1
            elif cw <= 9:
                cnt[f"interior_w{cw - 6}"] += 1
            cell, n_pass = _detect_window(level_img, *box, ini_th)
            if _retry_needed(cell, n_pass):
                cnt["retry_taken"] += 1
                cell, _ = _detect_window(level_img, *box, min_th)
                if not cell:
                    cnt["retry_empty_again"] += 1
            else:
                cnt["cell_first_pass_hit"] += 1
            for x, y, s in cell:
                keys.append((F32(x) + F32(j * w_cell), F32(y) + F32(i * h_cell), F32(s)))
    return keys


# ------------------------------------------------------------------ DistributeOctTree (:587-811)
class Node:
    __slots__ = ("keys", "ul", "ur", "bl", "br", "no_more", "seq")

    def __init__(self):
        self.keys, self.no_more, self.seq = [], False, -1
        self.ul = self.ur = self.bl = self.br = (0, 0)


def divide_node(nd):
    """ExtractorNode::DivideNode (:529-585)"""
    half_x = int(np.ceil(F32(nd.ur[0] - nd.ul[0]) / F32(2)))
    half_y = int(np.ceil(F32(nd.br[1] - nd.ul[1]) / F32(2)))
    n1, n2, n3, n4 = Node(), Node(), Node(), Node()
    n1.ul, n1.ur = nd.ul, (nd.ul[0] + half_x, nd.ul[1])
    n1.bl, n1.br = (nd.ul[0], nd.ul[1] + half_y), (nd.ul[0] + half_x, nd.ul[1] + half_y)
    n2.ul, n2.ur, n2.bl, n2.br = n1.ur, nd.ur, n1.br, (nd.ur[0], nd.ul[1] + half_y)
    n3.ul, n3.ur, n3.bl, n3.br = n1.bl, n1.br, nd.bl, (n1.br[0], nd.bl[1])
    n4.ul, n4.ur, n4.bl, n4.br = n3.ur, n2.br, n3.br, nd.br
    for kp in nd.keys:
        if kp[0] < n1.ur[0]:
            (n1 if kp[1] < n1.br[1] else n3).keys.append(kp)
        elif kp[1] < n1.br[1]:
            n2.keys.append(kp)
        else:
            n4.keys.append(kp)
    for n in (n1, n2, n3, n4):
        if len(n.keys) == 1:
            n.no_more = True
    return n1, n2, n3, n4


def _push_child(nodes, child):
    nodes.insert(0, child)       # lNodes.push_front


def _sort_key(entry):
    """SORT RULE: (size, creation order) ascending -- the list is then walked from its back"""
    return (entry[0], entry[1].seq)


_response_greater = operator.gt  # :800


def _index_of(nodes, nd):
    for i, n in enumerate(nodes):
        if n is nd:
            return i
    raise ValueError("node not in list")


def distribute_octtree(keys, min_x, max_x, min_y, max_y, n_wanted, cnt):
    """keys: [(x, y, response)] f32 -> the retained keys, in the order of the final node list"""
    ratio = F32(max_x - min_x) / F32(max_y - min_y)
    n_ini = int(np.floor(np.float64(ratio) + 0.5))     # C round() of a positive value: half away from zero (exact in f64)
    if n_ini < 1:
        cnt["nini_lt_1"] += 1
        return []
    h_x = F32(max_x - min_x) / F32(n_ini)
    nodes, roots = [], []
    seq = 0
    for i in range(n_ini):
        ni = Node()
        ni.ul, ni.ur = (int(h_x * F32(i)), 0), (int(h_x * F32(i + 1)), 0)
        ni.bl, ni.br = (ni.ul[0], max_y - min_y), (ni.ur[0], max_y - min_y)
        ni.seq = seq
        seq += 1
        nodes.append(ni)
        roots.append(ni)
    for kp in keys:
        q = F32(kp[0]) / h_x
        idx = int(q)
        if idx >= 1 and q == F32(idx):
            cnt["root_boundary_key"] += 1
        if idx >= n_ini:
            cnt["root_clamp"] += 1
            idx = n_ini - 1
        roots[idx].keys.append(kp)
    pos = 0
    while pos < len(nodes):
        if len(nodes[pos].keys) == 1:
            cnt["root_single"] += 1
            nodes[pos].no_more = True
            pos += 1
        elif not nodes[pos].keys:
            cnt["root_empty"] += 1
            del nodes[pos]
        else:
            pos += 1

    expand = []                  # vSizeAndPointerToNode

    def add_children(children):
        nonlocal seq
        n_expand = 0
        for c in children:
            if len(c.keys) > 0:
                c.seq = seq
                seq += 1
                _push_child(nodes, c)
                if len(c.keys) > 1:
                    n_expand += 1
                    expand.append((len(c.keys), c))
        return n_expand

    finish = False
    while not finish:
        prev_size = len(nodes)
        n_to_expand = 0
        expand.clear()
        for nd in list(nodes):   # children go to the front, behind the iterator: one sweep visits the nodes it started with
            if nd.no_more:
                continue
            n_to_expand += add_children(divide_node(nd))
            del nodes[_index_of(nodes, nd)]
        if len(nodes) >= n_wanted or len(nodes) == prev_size:
            cnt["stop_n_first_sweep" if len(nodes) >= n_wanted else "stop_no_growth"] += 1
            finish = True
        elif len(nodes) + n_to_expand * 3 > n_wanted:
            cnt["second_phase"] += 1
            while not finish:
                prev_size = len(nodes)
                order = sorted(list(expand), key=_sort_key)
                expand.clear()
                sizes = [e[0] for e in order]
                if len(set(sizes)) < len(sizes):
                    cnt["sort_equal_sizes"] += 1
                for j in range(len(order) - 1, -1, -1):
                    nd = order[j][1]
                    add_children(divide_node(nd))
                    del nodes[_index_of(nodes, nd)]
                    if len(nodes) >= n_wanted:
                        if j > 0:
                            cnt["second_break_mid"] += 1
                            if sizes[j - 1] == sizes[j]:
                                cnt["sort_tie_decides"] += 1
                        break
                if len(nodes) >= n_wanted or len(nodes) == prev_size:
                    cnt["second_stop_n" if len(nodes) >= n_wanted else "second_stop_no_growth"] += 1
                    finish = True
                else:
                    cnt["second_phase_repeat"] += 1
        else:
            cnt["first_sweep_again"] += 1
    result = []
    for nd in nodes:
        best = nd.keys[0]
        for kp in nd.keys[1:]:
            if _response_greater(kp[2], best[2]):
                best = kp
        top = max(kp[2] for kp in nd.keys)
        if sum(1 for kp in nd.keys if kp[2] == top) > 1:
            cnt["pick_equal_responses"] += 1
        result.append(best)
    return result


# ------------------------------------------------------------------ IC_Angle (:80-107) and cv::fastAtan2
_DEG = F32(180.0 / np.pi)
ATAN_P1 = F32(0.9997878412794807) * _DEG
ATAN_P3 = F32(-0.3258083974640975) * _DEG
ATAN_P5 = F32(0.1555786518463281) * _DEG
ATAN_P7 = F32(-0.04432655554792128) * _DEG
_EPS = F32(2.220446049250313e-16)     # (float)DBL_EPSILON


def _mul_add(a, b, c, step):
    """a * b + c the way unfused f32 code computes it: the product is rounded, then the sum (step: 0, 1, 2 = which of the three)"""
    return F32(F32(a * b) + c)


_first_of = operator.ge               # `if (ax >= ay)`


def fast_atan2(y, x, cnt=None):
    y, x = F32(y), F32(x)
    ax, ay = np.abs(x), np.abs(y)
    if cnt is not None:
        if x == 0 and y == 0:
            cnt["atan_zero"] += 1
        elif x == 0:
            cnt["atan_x0_yp" if y > 0 else "atan_x0_yn"] += 1
        elif y == 0:
            cnt["atan_y0_xp" if x > 0 else "atan_y0_xn"] += 1
        else:
            rel = "gt" if ax > ay else ("lt" if ax < ay else "tie")
            cnt[f"atan_{rel}_x{'p' if x > 0 else 'n'}_y{'p' if y > 0 else 'n'}"] += 1
    if _first_of(ax, ay):
        c = F32(ay / F32(ax + _EPS))
    else:
        c = F32(ax / F32(ay + _EPS))
    c2 = F32(c * c)
    a = _mul_add(ATAN_P7, c2, ATAN_P5, 0)
    a = _mul_add(a, c2, ATAN_P3, 1)
    a = _mul_add(a, c2, ATAN_P1, 2)
    a = F32(a * c)
    if not _first_of(ax, ay):
        a = F32(F32(90) - a)
    if x < 0:
        a = F32(F32(180) - a)
    if y < 0:
        a = F32(F32(360) - a)
    return a


def ic_moments(img, x, y, umax):
    m01 = m10 = 0
    for v in range(-HALF_PATCH_SIZE, HALF_PATCH_SIZE + 1):
        d = int(umax[abs(v)])
        line = img[y + v, x - d:x + d + 1].astype(np.int64)
        m10 += int((np.arange(-d, d + 1) * line).sum())
        m01 += v * int(line.sum())
    return m01, m10


# ------------------------------------------------------------------ ExtractDesc
def extract(image, n_features, scale_factor=1.2, n_levels=8, ini_th=20, min_th=7):
    """-> dict: tables, levels (u8 images), raw (per level [(x, y, response)] relative to minBorder, list order), kps (KP_DTYPE,
    level-major), patches (u8 [n, 32, 32]), blurred ({level: image}, levels that hold keypoints), counters"""
    image = np.asarray(image, np.uint8)
    t = tables(n_features, scale_factor, n_levels)
    cnt = new_counters()
    levels = pyramid(image, t["inv_scale"])
    min_b = EDGE_THRESHOLD - 3
    raw, per_level = [], []
    for level, img in enumerate(levels):
        h, w = img.shape
        keys = cell_corners(img, ini_th, min_th, cnt)
        raw.append(keys)
        kept = distribute_octtree(keys, min_b, w - EDGE_THRESHOLD + 3, min_b, h - EDGE_THRESHOLD + 3,
                                  int(t["features_per_level"][level]), cnt)
        size = F32(int(F32(PATCH_SIZE) * t["scale"][level]))
        per_level.append([[kx + F32(min_b), ky + F32(min_b), size, F32(-1), r, level] for kx, ky, r in kept])
    for level, kps in enumerate(per_level):
        for kp in kps:
            m01, m10 = ic_moments(levels[level], cv_round(kp[0]), cv_round(kp[1]), t["umax"])
            kp[3] = fast_atan2(F32(m01), F32(m10), cnt)
    out, patches, blurred = [], [], {}
    for level, kps in enumerate(per_level):
        if not kps:
            continue
        blurred[level] = gaussian_blur7(levels[level])
        h, w = levels[level].shape
        for kp in kps:
            x, y = cv_round(kp[0]), cv_round(kp[1])
            assert x - 16 > 0 and x + 16 < w and y - 16 > 0 and y + 16 < h      # :1113, always true for FAST corners
            patches.append(blurred[level][y - 16:y + 16, x - 16:x + 16])
        if FIRST_SCALED_LEVEL_TEST(level, 0):
            s = t["scale"][level]
            for kp in kps:
                kp[0], kp[1] = F32(kp[0] * s), F32(kp[1] * s)
        out.extend(kps)
    arr = np.zeros(len(out), KP_DTYPE)
    for i, kp in enumerate(out):
        arr[i] = tuple(kp)
    return dict(tables=t, levels=levels, raw=raw, kps=arr, blurred=blurred, counters=cnt,
                patches=np.array(patches, np.uint8).reshape(-1, 32, 32))
