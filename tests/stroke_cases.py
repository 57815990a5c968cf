"""Case families for the stroke tests (test_stroke_model.py on the CPU, test_gpu_stroke.py on the device), and the plumbing
that turns bare f32 polylines into an append: flatten work items in which every point is the start of a spline of its own, so
the device strokes exactly the points given (zero-length lines and exact U-turns included, which a PathBuilder would merge)."""
import math

import numpy as np

import stroke_model as SM

NONE = SM.NONE


# ---- an append of bare polylines -------------------------------------------------------------------------------------------------
def tables_of(contours):
    """contours: [[(x, y), ...]] -> (flatten tables dict, x, y, contour_first): point i is PointCommand::Start of spline i"""
    pts = [p for c in contours for p in c]
    n = len(pts)
    assert n < (1 << 22)
    x = np.asarray([p[0] for p in pts], np.float32); y = np.asarray([p[1] for p in pts], np.float32)
    z32, zf = np.zeros(0, np.uint32), np.zeros(0, np.float32)
    t = dict(point_commands=(np.uint32(0x7F800000) | np.arange(n, dtype=np.uint32)), point_indices=np.zeros(n, np.uint32),
             quad_indices=np.zeros(n, np.uint32), n_points=n, qx=zf, qy=zf, qw=zf, x0=zf, dx_recip=zf, k0=zf, dk=zf, curvatures_recip=zf,
             partial_spline=z32, partial_curv=zf, n_quads=0, sp0x=x, sp0y=y, sp2x=x, sp2y=y, n_splines=n)
    firsts = np.concatenate(([0], np.cumsum([len(c) for c in contours]))).astype(np.int64)
    return t, x, y, firsts


def slots_of(contours, slot_of_contour):
    ls = []
    for c, s in zip(contours, slot_of_contour):
        ls += [s] * (len(c) - 1) + [NONE]
    return np.asarray(ls, np.uint32)


class Case:
    """contours + one stroke range over all of them (or `strokes` given as ranges of contour indices)"""

    def __init__(self, name, contours, hw, join, cap, limit=4.0, slots=None, stroke_contours=None, affines=()):
        self.name, self.contours = name, [list(map(tuple, c)) for c in contours]
        self.slots = list(slots) if slots is not None else [0] * len(contours)
        self.t, self.x, self.y, self.firsts = tables_of(self.contours)
        self.line_slot = slots_of(self.contours, self.slots)
        rng = stroke_contours if stroke_contours is not None else [(0, len(contours), hw, limit, join, cap)]
        self.strokes = [(int(self.firsts[a]), int(self.firsts[b] - self.firsts[a]), h, l, j, c) for a, b, h, l, j, c in rng]
        self.affines = list(affines)

    def source(self):
        """the f32 points the device strokes: x, y with the affine ranges applied in the host's arithmetic"""
        x, y = self.x.copy(), self.y.copy()
        for first, count, m in self.affines:
            m = [np.float32(v) for v in m]
            for i in range(first, first + count):
                px, py = x[i], y[i]
                x[i] = _fmaf(m[0], px, _fmaf(m[2], py, m[4])); y[i] = _fmaf(m[1], px, _fmaf(m[3], py, m[5]))
        return x, y

    def model(self):
        x, y = self.source()
        return SM.stroke_append(x, y, self.line_slot, self.strokes)


def _fmaf(a, b, c):
    """fmaf on f32 values: the product of two f32 is exact in float64, and one float64 addition of an f32 to it rounds once
    more before the cast — which can differ from fmaf only by double rounding, ruled out for the exact affines used here"""
    return np.float32(float(a) * float(b) + float(c))


# ---- families whose geometry is exact in f32 -----------------------------------------------------------------------------------
def exact_families():
    """Axis-aligned and Pythagorean polylines, every line an integer multiple m of (3,4), (5,12), (8,15) or of an axis vector,
    half width = 5 (13, 17; 1 on the axes) * 2^-k: len is exact, s = hw / len is a power of two over m and o is exact.
    Joins: bevel everywhere, miter at axis-aligned right angles; caps butt and square.  Coordinates stay positive."""
    cases = []
    dirs = {"345": ((3, 4), 5), "51213": ((5, 12), 13), "81517": ((8, 15), 17)}
    for name, ((a, b), h) in dirs.items():
        for k, cap in ((1, SM.BUTT), (3, SM.SQUARE)):
            # a zig-zag through the direction, its mirror images and quarter turns
            steps = [(a, b), (b, -a), (a, b), (-b, a), (2 * a, 2 * b), (a, -b), (-2 * a, -2 * b)]
            p, pts = (100.0, 100.0), [(100.0, 100.0)]
            for dx, dy in steps:
                p = (p[0] + dx, p[1] + dy); pts.append(p)
            cases.append(Case(f"{name}-open-k{k}-cap{cap}", [pts], h * 2.0 ** -k, SM.BEVEL, cap))
        # closed: the direction's square, every side of length 2 h, ending where it began
        ring = [(60.0, 60.0), (60.0 + 2 * a, 60.0 + 2 * b), (60.0 + 2 * a + 2 * b, 60.0 + 2 * b - 2 * a), (60.0 + 2 * b, 60.0 - 2 * a), (60.0, 60.0)]
        cases.append(Case(f"{name}-closed", [ring], h * 0.25, SM.BEVEL, SM.BUTT))
        cases.append(Case(f"{name}-closed-reversed", [ring[::-1]], h * 0.5, SM.BEVEL, SM.BUTT))
    sq = [(16.0, 16.0), (48.0, 16.0), (48.0, 48.0), (16.0, 48.0), (16.0, 16.0)]
    stairs = [(8.0, 8.0), (24.0, 8.0), (24.0, 20.0), (40.0, 20.0), (40.0, 12.0), (56.0, 12.0)]
    for join in (SM.BEVEL, SM.MITER):
        cases.append(Case(f"square-closed-join{join}", [sq], 4.0, join, SM.BUTT))
        cases.append(Case(f"square-reversed-join{join}", [sq[::-1]], 2.0, join, SM.SQUARE))
        for cap in (SM.BUTT, SM.SQUARE):
            cases.append(Case(f"stairs-join{join}-cap{cap}", [stairs], 1.5, join, cap))
    # a miter beyond its limit falls back to the bevel: a right angle has 1 / cos(45 deg) = 1.414 > 1.25
    cases.append(Case("square-miter-limited", [sq], 4.0, SM.MITER, SM.BUTT, limit=1.25))
    # zero-length lines before a join and at both ends, an exact U-turn, a contour that is one point, one that is all one point
    cases.append(Case("zero-lengths", [[(10.0, 10.0), (10.0, 10.0), (30.0, 10.0), (30.0, 10.0), (30.0, 10.0), (30.0, 40.0), (30.0, 40.0)],
                                        [(50.0, 50.0)], [(60.0, 60.0), (60.0, 60.0), (60.0, 60.0)],
                                        [(70.0, 20.0), (90.0, 20.0), (80.0, 20.0)], [(70.0, 70.0), (90.0, 70.0), (70.0, 70.0)]], 2.0, SM.BEVEL, SM.SQUARE))
    return cases


def pixel_aligned():
    """the shapes whose outline lies on whole pixels, with their exact ink"""
    line = [(10.0, 20.0), (50.0, 20.0)]
    sq = [(16.0, 16.0), (48.0, 16.0), (48.0, 48.0), (16.0, 48.0), (16.0, 16.0)]
    return [(Case("line-butt", [line], 2.0, SM.MITER, SM.BUTT), 160), (Case("line-square", [line], 2.0, SM.MITER, SM.SQUARE), 176),
            (Case("square-miter", [sq], 4.0, SM.MITER, SM.BUTT), 40 * 40 - 24 * 24)]


def sixteenth_aligned():
    """bevel and round joins, round caps, inputs on the sixteenth grid: single shapes whose union's area is known analytically from
    the flattened polygons (pieces that overlap only along edges, or whose overlaps are computed)"""
    s = 1.0 / 16.0
    return [Case("bevel-corner", [[(10 + 3 * s, 40 + 5 * s), (40 + 3 * s, 40 + 5 * s), (40 + 3 * s, 10 + 5 * s)]], 3.0, SM.BEVEL, SM.BUTT),
            Case("round-corner", [[(10 + 3 * s, 40 + 5 * s), (40 + 3 * s, 40 + 5 * s), (40 + 3 * s, 10 + 5 * s)]], 3.0, SM.ROUND, SM.BUTT),
            Case("round-caps", [[(12 + 7 * s, 30 + 9 * s), (50 + 7 * s, 30 + 9 * s)]], 5.0, SM.BEVEL, SM.ROUND_CAP)]


# ---- random f32 polylines ------------------------------------------------------------------------------------------------------
def _near_tie(pts, limit):
    """a turn whose |sin| is below 2^-10, or a miter ratio within 2^-10 of the limit"""
    for i in range(1, len(pts) - 1):
        a = (float(pts[i][0]) - float(pts[i - 1][0]), float(pts[i][1]) - float(pts[i - 1][1]))
        b = (float(pts[i + 1][0]) - float(pts[i][0]), float(pts[i + 1][1]) - float(pts[i][1]))
        la, lb = math.hypot(*a), math.hypot(*b)
        if la == 0.0 or lb == 0.0:
            return True
        cross, dot = a[0] * b[1] - a[1] * b[0], a[0] * b[0] + a[1] * b[1]
        if abs(cross) / (la * lb) < 2.0 ** -10:
            return True
        theta = abs(math.atan2(cross, dot))
        if abs(1.0 / math.cos(theta / 2.0) - limit) < 2.0 ** -10:
            return True
    return False


def random_polyline(rng, n, lo=8.0, hi=248.0, limit=4.0, closed=False):
    """n f32 points in [lo, hi)^2 without near-ties: a point that would make one is drawn again, so every case stays in"""
    pts = []
    while len(pts) < n:
        p = (np.float32(rng.uniform(lo, hi)), np.float32(rng.uniform(lo, hi)))
        trial = pts[-2:] + [p]
        if len(trial) >= 2 and trial[-1] == trial[-2]:
            continue
        if len(trial) == 3 and _near_tie(trial, limit):
            continue
        if closed and len(pts) == n - 1:
            p = pts[0]
            if _near_tie(pts[-2:] + [p], limit) or _near_tie([pts[-1], p, pts[1]], limit):
                pts.pop()                                  # draw the point before the closing one again
                continue
        pts.append(p)
    return [(float(a), float(b)) for a, b in pts]


def random_cases(seed=20261019, count=24):
    rng = np.random.default_rng(seed)
    cases = []
    for k in range(count):
        join, cap = k % 3, (k // 3) % 3
        limit = [1.5, 2.5, 4.0][k % 3]
        hw = float(np.float32(rng.uniform(0.3, 12.0)))
        contours = [random_polyline(rng, int(rng.integers(4 if j % 2 else 2, 12)), limit=limit, closed=bool(j % 2)) for j in range(int(rng.integers(1, 4)))]
        cases.append(Case(f"random-{k}", contours, hw, join, cap, limit=limit))
    return cases


# ---- the oracle drawing polygons: the model's pieces pushed as ordinary fill paths ------------------------------------------------
def ref_render(layers, w, h, clear=(1.0, 1.0, 1.0, 1.0)):
    """layers: [(polygons, (r, g, b, a), "NonZero" | "EvenOdd")] bottom to top, a polygon = [(x, y), ...] (closed implicitly, as
    every reference path); returns the oracle's RGBA8 image [h, w, 4]"""
    import ref_api as R
    comp = R.Composition()
    for order, (polys, color, rule) in enumerate(layers):
        lay = comp.get_mut_or_insert_default(R.Order(order))
        for poly in polys:
            pb = R.PathBuilder()
            pb.move_to(R.Point(float(np.float32(poly[0][0])), float(np.float32(poly[0][1]))))
            for px, py in poly[1:]:
                pb.line_to(R.Point(float(np.float32(px)), float(np.float32(py))))
            lay.insert(pb.build())
        lay.set_props(R.Props(fill_rule=rule, func=R.Func.Draw(R.Style(fill=R.Fill.Solid(R.Color(*color))))))
    img = np.zeros(w * h * 4, np.uint8)
    R.Renderer().render(comp, R.BufferBuilder(img, R.LinearLayout(w, w * 4, h)).build(), R.RGBA, R.Color(*clear), None)
    return img.reshape(h, w, 4)


def piece_polys(pieces):
    return [p.pts for p in pieces]


# ---- scenes through the public API: the same layers for the product and, as the model's pieces, for the oracle ------------------
def api_scene(exact=False):
    """[(kind, contours, closed flags, style or None, colour, rule)], bottom to top; polylines only, no collinear neighbours, so the
    flattened points of a path are its points.  style = (width, join, cap, miter_limit).  exact=True: shapes of the exact families."""
    if exact:
        return [("fill", [[(70.0, 70.0), (120.0, 70.0), (120.0, 120.0)]], [True], None, (0.8, 0.1, 0.1, 1.0), "NonZero"),
                ("stroke", [[(16.0, 16.0), (48.0, 16.0), (48.0, 48.0), (16.0, 48.0)]], [True], (8.0, SM.MITER, SM.BUTT, 4.0), (0.0, 0.0, 0.0, 1.0), "NonZero"),
                ("stroke", [[(8.0, 72.0), (24.0, 72.0), (24.0, 84.0), (40.0, 84.0), (40.0, 76.0), (56.0, 76.0)]], [False], (3.0, SM.BEVEL, SM.SQUARE, 4.0),
                 (0.1, 0.2, 0.9, 0.5), "NonZero"),
                ("stroke", [[(64.0, 8.0), (70.0, 16.0), (78.0, 10.0), (84.0, 18.0), (100.0, 6.0)]], [False], (2.5, SM.BEVEL, SM.BUTT, 4.0),
                 (0.1, 0.6, 0.2, 1.0), "NonZero")]
    return [("fill", [[(10.5, 12.25), (60.0, 20.0), (30.0, 70.5)]], [True], None, (0.8, 0.1, 0.1, 1.0), "NonZero"),
            ("stroke", [[(20.0, 20.5), (100.25, 14.0), (112.0, 60.0), (70.5, 100.0), (18.0, 80.0)]], [True], (5.0, SM.MITER, SM.BUTT, 4.0),
             (0.1, 0.1, 0.8, 1.0), "NonZero"),
            ("stroke", [[(12.0, 110.0), (40.0, 90.5), (60.0, 116.0), (90.0, 88.0), (116.0, 112.5)]], [False], (7.0, SM.ROUND, SM.ROUND_CAP, 4.0),
             (0.1, 0.7, 0.2, 0.6), "NonZero"),
            ("stroke", [[(8.0, 40.0), (50.0, 44.5), (30.0, 60.0), (80.5, 66.0)]], [False], (4.0, SM.BEVEL, SM.SQUARE, 4.0), (0.9, 0.6, 0.0, 1.0), "NonZero"),
            ("stroke", [[(64.0, 30.0), (70.0, 50.0), (88.0, 52.0), (74.0, 64.0), (80.0, 84.0), (64.0, 72.0), (48.0, 84.0), (54.0, 64.0), (40.0, 52.0), (58.0, 50.0)]],
             [True], (3.0, SM.MITER, SM.BUTT, 2.0), (0.5, 0.0, 0.5, 0.8), "NonZero"),
            ("stroke", [[(100.0, 70.0), (120.0, 80.0), (104.0, 96.0)], [(96.0, 104.0), (122.0, 120.5)]], [False, False], (2.5, SM.ROUND, SM.BUTT, 4.0),
             (0.0, 0.0, 0.0, 1.0), "NonZero")]


def scene_path(api, layer):
    """the product path of one api_scene layer"""
    kind, contours, closed, style, _, _ = layer
    pb = api.PathBuilder(open_contours=(kind == "stroke"))
    for pts, cl in zip(contours, closed):
        pb.move_to(api.Point(*pts[0]))
        for p in pts[1:]:
            pb.line_to(api.Point(*p))
        if kind == "stroke" and cl:
            pb.close()
    path = pb.build()
    return path.stroke(api.StrokeStyle(*style)) if kind == "stroke" else path


def scene_composition(api, layers, orders=None):
    comp = api.Composition()
    for k, layer in enumerate(layers):
        rule = api.FillRule.EvenOdd if layer[5] == "EvenOdd" else api.FillRule.NonZero
        comp.get_mut_or_insert_default(api.Order(k if orders is None else orders[k])).insert(scene_path(api, layer)).set_props(
            api.Props(fill_rule=rule, func=api.Func.Draw(api.Style(fill=api.Fill.Solid(api.Color(*layer[4]))))))
    return comp


def scene_source(layer):
    """the flattened points of a layer's path as contours: a closed contour ends where it began"""
    return [list(pts) + ([pts[0]] if cl else []) for pts, cl in zip(layer[1], layer[2])]


def scene_model(layers):
    """per layer the polygons the oracle fills: the path itself, or the model's pieces of its stroke"""
    out = []
    for layer in layers:
        src = scene_source(layer)
        if layer[0] == "fill":
            polys = src
        else:
            w, join, cap, limit = layer[3]
            polys = piece_polys(Case("layer", src, w * 0.5, join, cap, limit=limit).model()[3])
        out.append((polys, layer[4], layer[5]))
    return out
