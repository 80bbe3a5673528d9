"""Crafted inputs for tests/test_frontend_exits.py.  Every image is a valid input of the extractor.

The building block is an isolated bright pixel ("dot") on a flat background of BG: all 16 ring pixels are darker by the same
amount, so the dot is the only FAST corner near it and its response is contrast - 1.  Two dots side by side (a "bar") have
equal scores and are not on each other's ring (radius 3).  A case is a dict: name, img (u8 [h, w]), n_levels, n_features."""
import numpy as np

BG = 100


def canvas(w, h, bg=BG):
    return np.full((h, w), bg, np.uint8)


def put(img, dots, bg=BG):
    """dots: (x, y, contrast).  Dots closer than 4 pixels (Chebyshev) must be adjacent (a bar): anything in between would sit on a ring."""
    for i, (x, y, c) in enumerate(dots):
        for (x2, y2, _) in dots[:i]:
            d = max(abs(x - x2), abs(y - y2))
            assert d == 1 or d >= 4, ((x, y), (x2, y2))
        img[y, x] = bg + c
    return img


def case(name, img, n_levels=1, n_features=2000):
    return dict(name=name, img=np.ascontiguousarray(img, np.uint8), n_levels=n_levels, n_features=n_features)


# ------------------------------------------------------------------ cell geometry
def _edge_dots(n, other):
    """dot pattern along one axis of length n (the other axis offers positions other[0..5], at least 6 apart): every position of the
    last three valid ones (n-20, n-21, n-22), the first invalid one (n-19), and both sides of the last three cell boundaries --
    single dots left and right of it and a bar across it."""
    out = [(n - 20, other[3], 50), (n - 21, other[4], 50), (n - 22, other[5], 50), (n - 19, other[0], 50)]
    span = n - 32
    ncell = int(np.float32(span) / np.float32(30))
    size = int(np.ceil(np.float32(span) / np.float32(ncell)))
    for j in range(ncell - 3, ncell):
        b = 16 + j * size + 3            # first position a window starting at 16 + j * size can report
        if b + 1 > n - 20 or b - 1 < 19:
            continue
        if abs(b - (n - 21)) < 6:        # keep clear of the edge dots: use the free `other` positions
            out += [(b - 1, other[1], 40), (b, other[2], 40)]
        else:
            out += [(b - 1, other[0], 40), (b, other[1], 40), (b - 1, other[2], 60), (b, other[2], 60)]
    return out


def cells_x():
    cases = []
    rows = (20, 27, 34, 41, 48, 55)
    for w in (723, 753, 783, 813, 843):
        img = canvas(w, 78)
        dots = [(x, y, c) for x, y, c in _edge_dots(w, rows)]
        dots += [(19, 58, 45), (18, 30, 45), (40, 19, 45), (60, 18, 45), (80, 58, 45), (100, 59, 45)]
        cases.append(case(f"cells_x_{w}", put(img, dots)))
    return cases


def cells_y():
    cases = []
    cols = (30, 37, 44, 51, 58, 65)
    for h in (813, 903):
        img = canvas(480, h)
        dots = [(x, y, c) for y, x, c in _edge_dots(h, cols)]
        dots += [(460, 19, 45), (461, 30, 45), (440, 18, 45), (19, 100, 45), (18, 120, 45)]
        cases.append(case(f"cells_y_{h}", put(img, dots)))
    return cases


def no_cells(synth):
    return [case("no_cells_200x164", synth.scene_frame(1, w=200, h=164), n_levels=8, n_features=500)]


# ------------------------------------------------------------------ NMS ties, thresholds, borders
def nms_ties():
    """224 x 140, one level: 6 x 3 cells; cell (j, i) reports x in [19 + 32 j, 50 + 32 j], y in [19 + 36 i, 54 + 36 i]"""
    w, h = 224, 140
    img = canvas(w, h)
    img[88:140, 0:83] = 0                # dark block under cells (0, 2) and (1, 2), for the 0 -> 255 dot
    dots = [
        # cell (0, 0): a 2-pixel bar of equal brightness inside one cell: both die (and the retry meets the same tie: nothing)
        (30, 30, 50), (31, 30, 50),
        # cells (1, 0) | (2, 0): the same bar across the boundary x = 82 | 83: both live
        (82, 28, 50), (83, 28, 50),
        # cells (1, 0) / (1, 1): a vertical bar across the boundary y = 54 | 55: both live
        (60, 54, 50), (60, 55, 50),
        # cell (3, 0): the only strong corners are a bar, plus one weak dot: the weak dot appears, through the retry
        (125, 30, 50), (126, 30, 50), (135, 40, 12),
        # cell (4, 0): one strong and one weak dot: the weak one must not appear
        (155, 30, 50), (165, 40, 12),
        # cell (2, 1): contrast 21 (score 20 = iniThFAST exactly) with a weak dot: the first pass succeeds, the weak one must not appear
        (95, 70, 21), (105, 80, 12),
        # cells (3, 1), (4, 1): contrast 21 / 20 alone in their cells: score 20 (first pass) / 19 (retry only)
        (130, 70, 21), (160, 70, 20),
        # cells (5, 1), (5, 2): contrast 8 / 7 alone in their cells: score 7 (retry) / 6 (no corner, the retry stays empty)
        (190, 70, 8), (190, 105, 7),
        # first / last valid column and row (in), and one beyond each (out)
        (19, 70, 50), (18, 80, 50), (w - 20, 30, 50), (w - 19, 40, 50),
        (100, 19, 50), (110, 18, 50), (130, h - 20, 50), (140, h - 19, 50),
    ]
    put(img, dots)
    img[105, 40] = 255                   # cell (0, 2): score 254
    return [case("nms_ties", img)]


# ------------------------------------------------------------------ quadtree
def random_dots(w, h, n, seed, contrasts=(30, 30, 30, 40, 50), x_range=None, pitch=6):
    """n dots on a grid of `pitch` pixels (so no two are closer than that), contrasts drawn from a short list: equal responses are common"""
    rng = np.random.default_rng(seed)
    xs = np.arange(19, w - 19, pitch)
    if x_range is not None:
        xs = xs[(xs >= x_range[0]) & (xs < x_range[1])]
    ys = np.arange(19, h - 19, pitch)
    pick = rng.choice(len(xs) * len(ys), size=min(n, len(xs) * len(ys)), replace=False)
    img = canvas(w, h)
    for p in pick:
        img[ys[p // len(xs)], xs[p % len(xs)]] = BG + contrasts[int(rng.integers(len(contrasts)))]
    return img


# (w, h, dots, seed, N): chosen by running tests/frontend_ref.py over seeds until its quadtree counters were all reached
QUADTREE_RANDOM = ((332, 120, 60, 1, 80), (332, 120, 120, 2, 40), (332, 120, 200, 3, 70), (332, 120, 90, 4, 25),
                   (332, 120, 150, 5, 10), (120, 110, 80, 6, 30))


def quadtree():
    cases = [case(f"quadtree_{w}x{h}_s{seed}_N{N}", random_dots(w, h, n, seed), n_features=N)
             for w, h, n, seed, N in QUADTREE_RANDOM]
    # 332 x 120: maxX - minX = 300, nIni = 3, hX = 100 exactly.  Root 0 (raw x < 100) stays empty, root 1 holds one key, which sits
    # exactly on the boundary x / hX = 1, root 2 holds the rest
    img = random_dots(332, 120, 40, 11, x_range=(222, 313))
    img[60, 116] = BG + 50
    cases.append(case("quadtree_roots", img, n_features=20))
    # taller than wide: nIni = round(78 / 228) = 0
    cases.append(case("quadtree_tall_110x260", random_dots(110, 260, 50, 12), n_features=30))
    return cases


# ------------------------------------------------------------------ orientation
ANGLE_EXTRAS = (
    (),                                                       # (0, 0)
    ((5, 5),), ((-5, 5),), ((5, -5),), ((-5, -5),),           # |m01| == |m10|, four sign combinations
    ((0, 6),), ((0, -6),), ((6, 0),), ((-6, 0),),             # m10 == 0, m01 == 0
    ((8, 4),), ((-8, 4),), ((8, -4),), ((-8, -4),),           # |m10| > |m01|
    ((4, 8),), ((-4, 8),), ((4, -8),), ((-4, -8),),           # |m10| < |m01|
    ((9, 2), (-3, 7)),                                        # two extras: m10 = 6 d, m01 = 9 d
)


def angles(synth):
    """dots 40 pixels apart; each has extra pixels of contrast 5 (not a corner at threshold 7, never on a ring, inside the radius-15
    disc): the flat background and the dot itself contribute nothing to the moments, an extra at (u, v) adds (5 u, 5 v) to (m10, m01)"""
    w, h = 280, 140
    img = canvas(w, h)
    for k, extras in enumerate(ANGLE_EXTRAS):
        cx, cy = 30 + 40 * (k % 6), 30 + 40 * (k // 6)
        img[cy, cx] = BG + 60
        for u, v in extras:
            img[cy + v, cx + u] = BG + 5
    return [case("angles_dots", img), case("angles_texture", synth.scene_frame(6, w=160, h=120))]


def scene_small(synth):
    return [case("scene_333x251", synth.scene_frame(3, w=333, h=251), n_levels=8, n_features=2000),
            case("scene_crop_640x240", synth.scene_frame(4)[60:300, 300:940], n_levels=8, n_features=1000)]


def all_cases(synth):
    return cells_x() + cells_y() + no_cells(synth) + nms_ties() + quadtree() + angles(synth) + scene_small(synth)
