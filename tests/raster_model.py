"""What stages 1 and 2 compute, exactly: a model of curves and of pixel area written from geometry and from the reference's
formulas (segment.rs, cpu/rasterizer.rs, cpu/pixel_segment.rs, path.rs) -- not from lines.hip and not from the oracle.  The
oracle (test_raster_model.py) and every HIP route (test_gpu_raster_model.py) are held to it.

Stage 2.  A line from p0 to p1 is cut at every integer x and y strictly inside it; every cut point and both ends are rounded
to sixteenths of a pixel with floor(16 v + 1/2); a piece belongs to the pixel its midpoint lies in and has
    cover        = y1s - y0s
    doubled area = cover * (2 * 16 * (px + 1) - x0s - x1s)      (twice the area, in 1/256 px^2, to the right of the piece)
All of it in exact integer arithmetic (an f32 is a dyadic rational).  What a painter accumulates along a row, and what the
model and a u64 segment stream are compared by, is
    A(px, py) = sum of the doubled areas of the pixel's pieces + 32 * sum of the covers of the pixels to its left.

Three behaviours of the reference are restated or left out as they are, each marked QUIRK below."""
from __future__ import annotations

import math
from fractions import Fraction

import numpy as np

import painter_model as PM
from oracle import oracle as orc

MAX_ERROR = 1.0 / 16.0                                       # path.rs:40


# ---- stage 2: lines ------------------------------------------------------------------------------------------------------
def f32_fma(a, b, c):
    """f32 a * b + c of f32 operands with one rounding: the product is exact in float64"""
    return float(np.float32(float(a) * float(b) + float(c)))


def transform_point(p, xf):
    """transform_point (segment.rs:30-39) on the f32 table values xf = (ux, uy, vx, vy, tx, ty): float64 products and sums,
    rounded to f32 where the reference's mul_add rounds -> the f32 endpoint the line is made of"""
    if xf is None:
        return (float(np.float32(p[0])), float(np.float32(p[1])))
    ux, uy, vx, vy, tx, ty = (float(np.float32(v)) for v in xf)
    x, y = float(np.float32(p[0])), float(np.float32(p[1]))
    return (f32_fma(ux, x, f32_fma(vx, y, tx)), f32_fma(uy, x, f32_fma(vy, y, ty)))


def culled(p0, p1, width, height):
    """The culling rules (segment.rs:41-52): horizontal lines, lines wholly at or above y = 0, wholly at or beyond the height or
    the width.  The left edge is NOT culled: a line left of the canvas carries cover into it."""
    return (p0[1] == p1[1] or (p0[1] >= height and p1[1] >= height) or (p0[0] >= width and p1[0] >= width)
            or (p0[1] <= 0.0 and p1[1] <= 0.0))


def _ints(p0, p1):
    fr = [Fraction(float(v)) for v in (p0[0], p0[1], p1[0], p1[1])]
    s = max(f.denominator for f in fr)
    return [int(f * s) for f in fr] + [s]


def pieces(p0, p1):
    """-> ([(px, py, cover, doubled_area)], through_corner): the pieces of the line p0 -> p1 (f32 values) in order along it;
    `through_corner`: an x cut and a y cut coincide strictly inside the line"""
    x0, y0, x1, y1, s = _ints(p0, p1)
    dx, dy = x1 - x0, y1 - y0
    ax, ay = abs(dx) or 1, abs(dy) or 1
    d = ax * ay                                                  # the line's parameter t = n / d, n an integer at every cut
    cuts = {0, d}
    n_x = n_y = 0
    if dx:
        lo, hi = (x0, x1) if dx > 0 else (x1, x0)
        for X in range(lo // s + 1, -(-hi // s)):                # integers strictly between
            cuts.add(abs(X * s - x0) * ay); n_x += 1
    if dy:
        lo, hi = (y0, y1) if dy > 0 else (y1, y0)
        for Y in range(lo // s + 1, -(-hi // s)):
            cuts.add(abs(Y * s - y0) * ax); n_y += 1
    through_corner = len(cuts) < 2 + n_x + n_y
    cuts = sorted(cuts)
    sd = s * d

    def sixteenths(n):                                           # floor(16 v + 1/2) of the point at n / d, both coordinates
        return ((32 * (x0 * d + n * dx) + sd) // (2 * sd), (32 * (y0 * d + n * dy) + sd) // (2 * sd))
    out = []
    xa, ya = sixteenths(0)
    for na, nb in zip(cuts[:-1], cuts[1:]):
        xb, yb = sixteenths(nb)
        m = na + nb                                              # the midpoint is at m / (2 d)
        px = (x0 * 2 * d + m * dx) // (2 * sd)
        py = (y0 * 2 * d + m * dy) // (2 * sd)
        cover = yb - ya
        out.append((px, py, cover, cover * (32 * (px + 1) - xa - xb)))
        xa, ya = xb, yb
    return out, through_corner


AREA_DTYPE = np.dtype([("layer", "<i8"), ("py", "<i8"), ("px", "<i8"), ("cover", "<i8"), ("area", "<i8")])


def _canonical(rec):
    """rows py < 0 dropped, columns px < 0 folded into px = -1 with their covers alone, one record per (layer, py, px)"""
    rec = rec[rec["py"] >= 0]
    left = rec["px"] < 0
    rec["px"][left] = -1                                         # tiles clamp to -1 (pixel_segment.rs:47-52): only the row's
    rec["area"][left] = 0                                        # carried cover is comparable there
    if len(rec) == 0:
        return rec
    order = np.lexsort((rec["px"], rec["py"], rec["layer"]))
    rec = rec[order]
    new = np.ones(len(rec), bool)
    new[1:] = (rec["layer"][1:] != rec["layer"][:-1]) | (rec["py"][1:] != rec["py"][:-1]) | (rec["px"][1:] != rec["px"][:-1])
    start = np.flatnonzero(new)
    out = rec[start].copy()
    out["cover"] = np.add.reduceat(rec["cover"], start)
    out["area"] = np.add.reduceat(rec["area"], start)
    return out


def row_area(layered_pieces):
    """[(layer, px, py, cover, doubled_area)] -> the canonical table A and the rows' cover totals are read from (`difference`,
    `dense`)"""
    rec = np.zeros(len(layered_pieces), AREA_DTYPE)
    if len(layered_pieces):
        a = np.asarray(layered_pieces, np.int64).reshape(-1, 5)
        rec["layer"], rec["px"], rec["py"], rec["cover"], rec["area"] = a.T
    return _canonical(rec)


def line_area(lines, width, height):
    """[(layer, p0, p1, xf or None)] -> (table, [through_corner per line]); culled lines give nothing"""
    out, corners = [], []
    for layer, p0, p1, xf in lines:
        a, b = transform_point(p0, xf), transform_point(p1, xf)
        if culled(a, b, width, height):
            corners.append(False)
            continue
        ps, corner = pieces(a, b)
        corners.append(corner)
        out.extend((layer, px, py, c, ar) for px, py, c, ar in ps if c != 0 or ar != 0)
    return row_area(out), corners


def decode(stream):
    """any u64 segment stream, in any order -> the same table, by the field layout of oracle.seg_fields"""
    f = orc.seg_fields(np.asarray(stream, np.uint64))
    rec = np.zeros(len(f["cover"]), AREA_DTYPE)
    rec["layer"] = f["layer"]
    rec["py"] = f["tile_y"] * 16 + f["local_y"]
    rec["px"] = f["tile_x"] * 16 + f["local_x"]
    rec["cover"] = f["cover"]
    rec["area"] = f["double_area"]
    return _canonical(rec)


def difference(a, b):
    """two tables -> {layer: (rows whose cover totals differ, max |A_a - A_b| over every pixel px >= 0 of every row)} for the
    layers where either is non-zero.  A is compared at every pixel: the listed ones and the ones between them."""
    nb = b.copy()
    nb["cover"] = -nb["cover"]; nb["area"] = -nb["area"]
    d = _canonical(np.concatenate([a, nb]))
    if len(d) == 0:
        return {}
    row_start = np.ones(len(d), bool)
    row_start[1:] = (d["layer"][1:] != d["layer"][:-1]) | (d["py"][1:] != d["py"][:-1])
    starts = np.flatnonzero(row_start)
    incl = np.cumsum(d["cover"])
    base = np.repeat(incl[starts] - d["cover"][starts], np.diff(np.append(starts, len(d))))
    incl = incl - base                                           # covers up to and including this pixel, within the row
    excl = incl - d["cover"]
    at = np.where(d["px"] >= 0, np.abs(d["area"] + 32 * excl), 0)            # A at a listed pixel
    row_end = np.append(row_start[1:], True)
    next_listed = np.zeros(len(d), bool)
    next_listed[:-1] = ~row_end[:-1] & (d["px"][1:] == d["px"][:-1] + 1)
    after = np.where(next_listed, 0, np.abs(32 * incl))                     # A at the pixel to its right, where that one is not listed
    worst = np.maximum(at, after)
    out = {}
    for layer in np.unique(d["layer"]):
        m = d["layer"] == layer
        bad_rows = int(np.count_nonzero(incl[m & row_end]))
        w = int(worst[m].max())
        if bad_rows or w:
            out[int(layer)] = (bad_rows, w)
    return out


def row_totals(table, layer):
    """{py: the row's cover total} of one layer"""
    t = table[table["layer"] == layer]
    rows, start = np.unique(t["py"], return_index=True)
    return dict(zip(rows.tolist(), np.add.reduceat(t["cover"], start).tolist())) if len(t) else {}


def dense(table, layer, width, height):
    """A of one layer on the pixels of a width x height canvas, [height, width] int64"""
    t = table[(table["layer"] == layer) & (table["py"] < height) & (table["px"] < width)]
    area = np.zeros((height, width + 1), np.int64)
    cover = np.zeros((height, width + 1), np.int64)
    np.add.at(area, (t["py"], t["px"] + 1), t["area"])
    np.add.at(cover, (t["py"], t["px"] + 1), t["cover"])
    carried = np.cumsum(cover, 1) - cover
    return (area + 32 * carried)[:, 1:]


# ---- polygons ------------------------------------------------------------------------------------------------------------
def polygon_lines(contours, layer=0, xf=None):
    """closed contours [[(x, y), ...]] -> their edges as lines of `line_area`"""
    return [(layer, c[i], c[(i + 1) % len(c)], xf) for c in contours for i in range(len(c))]


def polygon_area(contours, width, height, layer=0, xf=None):
    """A of closed contours: the sum over their edges"""
    return line_area(polygon_lines(contours, layer, xf), width, height)[0]


def image(layers, width, height, clear=(1.0, 1.0, 1.0, 1.0)):
    """[(contours, rgba, even_odd)] in paint order, every layer a solid fill composited Over -> the sRGB8 image [height, width * 4].
    Coverage, the blend and the encode are painter_model's."""
    img = np.empty((height, width, 4), np.float64)
    img[:] = PM.f32(clear)
    for order, (contours, rgba, even_odd) in enumerate(layers):
        a = dense(polygon_area(contours, width, height, order), order, width, height)
        cov = PM.coverage(a, even_odd)[..., None]
        fill = np.broadcast_to(PM.f32(rgba), (height, width, 4))
        img = PM.blend_at(img, fill, fill[..., 3:4] * cov, PM.OVER)
    return PM.encode_srgb8(img, clear=clear)


# ---- the reference's three behaviours that are not geometry ---------------------------------------------------------------
# QUIRK (corner ties, cpu/rasterizer.rs:32-61): `find` estimates how many crossings of either kind precede the i-th with `ceil`
# of f64 products.  Where an x crossing and a y crossing coincide (a line through a pixel corner: c == d and a == 2 b, or the
# like) the estimate can slip by one and the last piece runs from beyond the line's end back to it.  The pinned example:
CORNER_TIE_LINE = ((58.875, 172.25), (76.25, 137.5))             # ends with a piece of cover +8 in pixel (76, 137) ...
CORNER_TIE_COVER_SUM = -548                                      # ... and its covers sum to this, not to 16 * (137.5 - 172.25)
CORNER_TIE_LAST = (76, 137, 8)                                   # (px, py, cover) of the stream's last segment
# `pieces` does not model it; lines through a corner are a family of their own (raster_cases.corner_lines).
#
# QUIRK (boundary slivers, cpu/rasterizer.rs:128-145): a piece whose two ends both round onto its pixel's RIGHT edge is filed in
# the right neighbour, at full width (border_x = min(x0_sub, x1_sub) >> 4 of the ROUNDED ends, double_area_multiplier 32).  By
# geometry it lies in the left pixel at zero width.  A is the same either way, per-pixel (cover, area) pairs are not: tables are
# compared with `difference`, never record by record.
#
# QUIRK (doubled-back quadratic, path.rs:218-236, :259-266, :322-332): control points on one line, p2 on the far side of p0 from
# p1.  cross == 0 makes the curvature estimate non-finite, so the `collinear` branch gives the quadratic one interior point, at
# t = 0.5.  The closing line p2 -> p0 then runs exactly against the curve's last direction; `diff` folds opposite directions
# together, so no new spline is started, push_line moves the SAME spline's end to p0, and the contour flattens to p0, the
# interior point, p0: the quadratic's own end p2 (22.9 px away in raster_cases.DOUBLED_BACK) is not emitted.  The contour
# encloses no area, so nothing is painted wrong; only measure (c) below is asserted for it.


# ---- stage 1: curves -----------------------------------------------------------------------------------------------------
KINDS = {"line": 2, "quad": 3, "cubic": 4, "rat_quad": 3, "rat_cubic": 4}


def homogeneous(ctrl, weights=None):
    """control points as the caller names them (x, y) and their weights -> [n, 3] float64 of the f32 values the path stores:
    (x * w, y * w, w), the products rounded to f32 (path.rs:873-912)"""
    ctrl = np.asarray(ctrl, np.float32)
    w = np.ones(len(ctrl), np.float32) if weights is None else np.asarray(weights, np.float32)
    return np.stack([(ctrl[:, 0] * w), (ctrl[:, 1] * w), w], 1).astype(np.float64)


def curve_point(kind, ctrl, weights, t):
    """the point at parameter t (a float or an array) of a line, quadratic, cubic, rational quadratic or rational cubic Bezier,
    float64: de Casteljau on the homogeneous points, then the division -> [..., 2]"""
    assert len(ctrl) == KINDS[kind]
    return _eval_h(homogeneous(ctrl, weights), t)


def transformed(segments, t9):
    """a projective 3x3 (row-major, as Path::transform takes it, path.rs:744-759) applied to the homogeneous control points:
    segments [(kind, ctrl, weights)] -> the same in homogeneous form [(kind, h [n, 3])]"""
    m = np.asarray(t9, np.float32).astype(np.float64).reshape(3, 3)
    return [(k, homogeneous(c, w) @ m.T) for k, c, w in segments]


def _eval_h_raw(h, t):
    t = np.asarray(t, np.float64)[..., None]
    level = [h[i] for i in range(len(h))]
    while len(level) > 1:
        level = [(1.0 - t) * a + t * b for a, b in zip(level[:-1], level[1:])]
    return np.broadcast_to(level[0], t.shape[:-1] + (3,))


def _eval_h(h, t):
    p = _eval_h_raw(h, t)
    return p[..., :2] / p[..., 2:3]


def _as_h(segments):
    return [(s[0], s[1]) if len(s) == 2 else (s[0], homogeneous(s[1], s[2])) for s in segments]


_GOLD = (math.sqrt(5.0) - 1.0) / 2.0


def _golden(f, lo, hi, steps=36):
    """vectorised golden-section search for the minimum of f on [lo, hi] (arrays) -> (t, f(t))"""
    a, b = lo.copy(), hi.copy()
    c = b - _GOLD * (b - a); d = a + _GOLD * (b - a)
    fc, fd = f(c), f(d)
    for _ in range(steps):                                       # one new evaluation a step: the kept inner point is reused
        left = fc < fd
        b = np.where(left, d, b); a = np.where(left, a, c)
        new = np.where(left, b - _GOLD * (b - a), a + _GOLD * (b - a))
        fn = f(new)
        c, d, fc, fd = np.where(left, new, d), np.where(left, c, new), np.where(left, fn, fd), np.where(left, fc, fn)
    t = 0.5 * (a + b)
    return t, f(t)


def _seg_dist(p, a, b):
    """distance of the points p [m, 2] to the segments a[k] -> b[k]: [m, k]"""
    ab = b - a
    den = (ab * ab).sum(-1)
    ap = p[:, None, :] - a[None, :, :]
    u = np.clip((ap * ab[None]).sum(-1) / np.where(den > 0, den, 1.0), 0.0, 1.0)
    d = ap - u[..., None] * ab[None]
    return np.sqrt((d * d).sum(-1))


def _hull_gap(p, h):
    """a lower bound of the distance of the points p [m, 2] to the curve: their distance to the bounding box of its control points
    (weights are positive, so the curve lies inside it)"""
    e = h[:, :2] / h[:, 2:3]
    lo, hi = e.min(0), e.max(0)
    d = np.maximum(np.maximum(lo - p, p - hi), 0.0)
    return np.sqrt((d * d).sum(-1))


def vertex_distance(segments, x, y, coarse=128):
    """measure (a): the largest distance of an emitted vertex to the curve.  Per vertex and segment: a coarse scan, then a golden-
    section search around EVERY local minimum of the scan that could still be the nearest (a curve that turns back on itself has
    two branches close to each other, and the nearest sample may sit on the wrong one)."""
    segs = _as_h(segments)
    p = np.stack([np.asarray(x, np.float64), np.asarray(y, np.float64)], 1)
    if len(p) == 0:
        return 0.0
    ts = np.linspace(0.0, 1.0, coarse + 1)
    ends = np.stack([_eval_h(h, np.array([0.0, 0.5, 1.0])) for _, h in segs])          # a first upper bound from three points each
    best = np.sqrt(((p[:, None, None, :] - ends[None]) ** 2).sum(-1)).min((1, 2))
    scans = []
    for _, h in segs:
        near = np.flatnonzero(_hull_gap(p, h) <= best)
        if len(near) == 0:
            scans.append(None)
            continue
        c = _eval_h(h, ts)
        d = np.sqrt(((p[near, None, :] - c[None]) ** 2).sum(-1))
        best[near] = np.minimum(best[near], d.min(1))
        scans.append((near, d, float(np.sqrt(((c[1:] - c[:-1]) ** 2).sum(-1)).max())))
    for (_, h), scan in zip(segs, scans):
        if scan is None:
            continue
        near, d, spacing = scan
        low = np.ones(d.shape, bool)
        low[:, 1:] &= d[:, 1:] <= d[:, :-1]; low[:, :-1] &= d[:, :-1] <= d[:, 1:]
        low &= d <= (best[near] + spacing)[:, None]
        vi, ki = np.nonzero(low)
        if len(vi) == 0:
            continue
        q = p[near[vi]]
        f = lambda t: np.sqrt(((_eval_h(h, t) - q) ** 2).sum(-1))
        _, fd = _golden(f, np.clip(ts[ki] - 1.0 / coarse, 0.0, 1.0), np.clip(ts[ki] + 1.0 / coarse, 0.0, 1.0))
        np.minimum.at(best, near[vi], fd)
    return float(best.max())


def curve_distance(segments, x, y, coarse=96):
    """measure (b): the largest distance of a point of the curve to the polyline.  Per segment: a coarse scan, then a golden-
    section search (for the maximum) around every local maximum of the scan that reaches half the scan's largest value.  Only
    the polyline's edges that can be the nearest one to a point of the segment take part: a point of the segment is no farther
    from the polyline than a sampled point is, plus the diagonal of the control points' bounding box."""
    a = np.stack([np.asarray(x, np.float64), np.asarray(y, np.float64)], 1)
    if len(a) == 1:
        a = np.concatenate([a, a])
    pa, pb = a[:-1], a[1:]
    ts = np.linspace(0.0, 1.0, coarse + 1)
    scans = []
    for _, h in _as_h(segments):
        e = h[:, :2] / h[:, 2:3]
        rough = float(_seg_dist(_eval_h(h, np.array([0.0, 0.5, 1.0])), pa, pb).min(1).max())
        margin = rough + float(np.sqrt(((e.max(0) - e.min(0)) ** 2).sum()))
        keep = ((np.maximum(pa, pb) >= e.min(0) - margin) & (np.minimum(pa, pb) <= e.max(0) + margin)).all(1)
        # a point between two samples is within `gap` of one of them, so its nearest edge is within (largest sampled distance + 2 gap)
        # of that sample: first on 9 samples, to thin the edges out, then on the scan itself
        ka, kb = pa[keep], pb[keep]
        for t in (np.linspace(0.0, 1.0, 9), ts):
            c = _eval_h(h, t)
            full = _seg_dist(c, ka, kb)
            d = full.min(1)
            spacing = float(np.sqrt(((c[1:] - c[:-1]) ** 2).sum(-1)).max())
            close = full.min(0) <= d.max() + 2.0 * spacing
            ka, kb = ka[close], kb[close]
        scans.append((float(d.max()), spacing, h, d, ka, kb))
    worst = max(s[0] for s in scans) if scans else 0.0
    for top, spacing, h, d, ka, kb in sorted(scans, key=lambda s: -s[0]):
        if top + 0.5 * spacing <= worst:                         # the distance is 1-Lipschitz in the point: no point of this
            continue                                             # segment is farther than a sample plus half the spacing
        f = lambda t: _seg_dist(_eval_h(h, t), ka, kb).min(1)
        peak = np.ones(len(ts), bool)
        peak[1:] &= d[1:] >= d[:-1]; peak[:-1] &= d[:-1] >= d[1:]
        peak &= d >= 0.5 * d.max()
        k = np.flatnonzero(peak)
        k = k[np.argsort(-d[k], kind="stable")[:6]]              # (a straight segment is all peaks: the six highest will do)
        _, fd = _golden(lambda t: -f(t), np.clip(ts[k] - 1.0 / coarse, 0.0, 1.0), np.clip(ts[k] + 1.0 / coarse, 0.0, 1.0))
        worst = max(worst, float((-fd).max()))
    return worst


_GL_X, _GL_W = np.polynomial.legendre.leggauss(12)


def _quadrature_nodes(panels):
    edges = np.linspace(0.0, 1.0, panels + 1)
    half = 0.5 * np.diff(edges)[:, None]
    return (edges[:-1, None] + half * (_GL_X[None] + 1.0)).ravel(), (half * _GL_W[None]).ravel()


def _derivative(h, t):
    """d/dt of the rational curve, analytically from the homogeneous hodograph"""
    n = len(h) - 1
    p = _eval_h_raw(h, t)
    dp = n * _eval_h_raw(h[1:] - h[:-1], t)
    return (dp[..., :2] * p[..., 2:3] - p[..., :2] * dp[..., 2:3]) / (p[..., 2:3] ** 2)


def curve_area_and_length(segments, panels=64):
    """the signed area enclosed by a closed chain of segments (1/2 the integral of x dy - y dx) and the chain's length, by
    Gauss-Legendre quadrature on `panels` panels per segment"""
    t, w = _quadrature_nodes(panels)
    area = length = 0.0
    for _, h in _as_h(segments):
        p = _eval_h(h, t); d = _derivative(h, t)
        area += 0.5 * float((w * (p[:, 0] * d[:, 1] - p[:, 1] * d[:, 0])).sum())
        length += float((w * np.sqrt((d * d).sum(-1))).sum())
    return area, length


def polyline_area(x, y):
    """the signed area of the closed polyline (shoelace), float64"""
    x = np.asarray(x, np.float64); y = np.asarray(y, np.float64)
    return 0.5 * float((x * np.roll(y, -1) - np.roll(x, -1) * y).sum())


def ulp32(v):
    """spacing of f32 at |v|"""
    return float(np.spacing(np.float32(abs(v))))
