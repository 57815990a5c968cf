"""The families raster_model.py is compared on, all small: lattice lines (every grid crossing a sixteenth, so the model and a
correct rasterizer agree exactly), random f32 lines, lines through pixel corners, polygons for the image test and the curves of
stage 1.  Everything is seeded or literal; which line passes through a pixel corner is decided by the model
(`raster_model.pieces`), not by construction."""
from __future__ import annotations

import json
import math
import os
from fractions import Fraction

import numpy as np

import raster_model as RM
from oracle import oracle as orc

NONE = 0xFFFFFFFF
LATTICE_CANVAS = (72, 40)                    # 4.5 x 2.5 tiles
GENERAL_CANVAS = (300, 300)
GENERAL_SEEDS = (11, 12, 13, 14)
GENERAL_LINES_PER_SEED = 400


# ---- tables a backend loads: one geom (one layer) per line, so that every line is compared on its own --------------------------
def line_tables(lines):
    """[(layer, p0, p1, xf or None)] -> x, y, line_slot, geoms, styles: two points per line, the joins between lines unowned"""
    n = len(lines)
    x = np.zeros(2 * n, np.float32); y = np.zeros(2 * n, np.float32)
    ls = np.full(2 * n, NONE, np.uint32)
    geoms = np.zeros(max(n, 1), orc.GEOM_DTYPE)
    geoms["order"] = NONE
    top = 0
    for i, (layer, p0, p1, xf) in enumerate(lines):
        x[2 * i], y[2 * i] = p0
        x[2 * i + 1], y[2 * i + 1] = p1
        ls[2 * i] = i
        geoms[i]["order"] = layer
        top = max(top, layer)
        if xf is not None:
            geoms[i]["flags"] = 1                                # FORMA_GEOM_HAS_XF
            geoms[i]["xf"] = xf
    words = np.array([0, 0] + [int(np.float32(v).view(np.uint32)) for v in (0.0, 0.0, 0.0, 1.0)], np.uint32)   # one solid style
    return dict(x=x, y=y, line_slot=ls[: max(2 * n - 1, 0)], geoms=geoms, style_offsets=np.zeros(top + 1, np.uint32),
                style_words=words, unchanged=np.zeros(top + 1, np.uint8), images=np.zeros(0, orc.IMAGE_DTYPE),
                texels=np.zeros((0, 4), np.uint16))


def load(backend, t):
    backend.set_geometry(t["x"], t["y"], t["line_slot"])
    backend.set_geoms(t["geoms"])
    backend.set_styles(t["style_offsets"], t["style_words"], t["unchanged"])
    backend.set_images(t["images"], t["texels"])


def numbered(pairs, xf=None, first=0):
    """[(p0, p1)] -> lines of layers first, first + 1, ..."""
    return [(first + i, p0, p1, xf) for i, (p0, p1) in enumerate(pairs)]


def n_segments(line, width, height):
    """pixel segments the line owns: its pieces, none if it is culled"""
    _, p0, p1, xf = line
    a, b = RM.transform_point(p0, xf), RM.transform_point(p1, xf)
    return 0 if RM.culled(a, b, width, height) else len(RM.pieces(a, b)[0])


# ---- stage 2: the lattice ------------------------------------------------------------------------------------------------------
SLOPES = [(k, s) for k in (-2, -1, 0, 1, 2) for s in (1, -1)] + [(None, 1)]        # dy/dx = s * 2^k; None: vertical


def _unit(k, s):
    """(grid, step): endpoints are multiples of `grid` = 2^|k| / 16, a line is a whole number of `step`s long"""
    if k is None:
        return 1.0 / 16.0, (0.0, 1.0 / 16.0)
    g = 2.0 ** abs(k) / 16.0
    return g, ((g, s * g * 2.0 ** k) if k >= 0 else (g * 2.0 ** -k, s * g))


def _snap(v, g, integer):
    """v moved onto the grid g: onto an integer, or onto a grid point that is none"""
    if integer:
        return float(round(v))
    v = math.floor(v / g) * g
    return v + g if float(v).is_integer() else v


def lattice_pairs():
    """Every lattice line of the family, corners and all, in both directions; see `no_corner_lines` / `corner_lines`"""
    rng = np.random.default_rng(20261)
    w, h = LATTICE_CANVAS
    out = []

    def add(p0, k, s, m):                                        # m steps from p0
        _, (ux, uy) = _unit(k, s)
        p1 = (p0[0] + m * ux, p0[1] + m * uy)
        out.append((p0, p1)); out.append((p1, p0))

    def add_to(p1, k, s, m):                                     # m steps that end on p1
        _, (ux, uy) = _unit(k, s)
        add((p1[0] - m * ux, p1[1] - m * uy), k, s, m)

    def through(p, k, s, m):                                     # m steps to either side of p
        _, (ux, uy) = _unit(k, s)
        add((p[0] - m * ux, p[1] - m * uy), k, s, 2 * m)
    for k, s in SLOPES:
        g, (ux, uy) = _unit(k, s)
        per_px = 1.0 / max(abs(ux), abs(uy))                     # steps per pixel along the longer axis
        for start in range(4):                                   # starts anywhere, on an integer x, on an integer y, on both
            for _ in range(10):
                x0 = _snap(rng.uniform(-6, w + 4), g, start & 1)
                y0 = _snap(rng.uniform(-5, h + 4), g, start & 2)
                for px_len in (0.4, 0.9, 1.0, 2.0, 3.5, 9.0, 17.0, 30.0):
                    add((x0, y0), k, s, max(1, int(px_len * per_px) + int(rng.integers(0, 2))))
        for fx, fy in ((0.25, 0.25), (0.5, 0.0), (0.0, 0.5), (0.75, 0.5)):
            add((10.0 + fx, 7.0 + fy), k, s, 1)                  # inside one pixel, or out of it by one step
            add((10.0 + fx, 7.0 + fy), k, s, 2)
            through((33.0, 20.0 + fy) if k is not None else (33.0 + fx, 20.0), k, s, 1)      # straddling one boundary
        for f in (0.25, 0.5):
            n = int(6 * per_px)
            add_to((float(w), 11.0 + f), k, s, n)                # ends exactly on x == width
            add((float(w), 11.0 + f), k, s, n)                   # starts on it and leaves: wholly beyond the width
            add_to((20.0 + f, float(h)), k, s, n)                # ends exactly on y == height (or comes from beyond it)
            add((20.0 + f, float(h)), k, s, n)
            add_to((9.0 + f, 0.0), k, s, n); add((9.0 + f, 0.0), k, s, n)                    # touches y == 0 from either side
            through((float(w) - f, 13.0 + f), k, s, n)           # through the right edge
            through((22.0 + f, float(h) - f), k, s, n)           # through the bottom edge
            through((24.0 + f, f), k, s, n)                      # through the top edge: starts above 0
            through((f, 17.0 + f), k, s, n)                      # through the left edge: starts left of 0
            add((-9.0 - f, 5.0 + f), k, s, int(3 * per_px))      # wholly left of 0: nothing but carried cover
    # vertical lines exactly on a pixel boundary and on a tile boundary (a = inf), and on the canvas's own edges
    for x in (5.0, 16.0, 32.0, 0.0, float(w)):
        for y0, y1 in ((3.25, 3.75), (3.25, 9.5), (14.5, 33.0), (-2.5, 6.0), (30.0, h + 3.5), (16.0, 32.0)):
            out.append(((x, y0), (x, y1))); out.append(((x, y1), (x, y0)))
    return out


_cache = {}


def _split():
    if "split" not in _cache:
        plain, corner = [], []
        for p0, p1 in lattice_pairs():
            a, b = RM.transform_point(p0, None), RM.transform_point(p1, None)
            (corner if RM.pieces(a, b)[1] else plain).append((p0, p1))
        _cache["split"] = (plain, corner)
    return _cache["split"]


def no_corner_lines():
    return _split()[0]


def corner_lines():
    """lattice lines through a pixel corner, the pinned line first"""
    return [RM.CORNER_TIE_LINE] + _split()[1]


def endpoint_kinds(pairs):
    """how many lines start / end on an integer x only, an integer y only, on both: the `c == 0` / `d == 0` index shift"""
    out = {"start_x": 0, "start_y": 0, "start_xy": 0, "end_x": 0, "end_y": 0, "end_xy": 0}
    for p0, p1 in pairs:
        for tag, p in (("start", p0), ("end", p1)):
            ix, iy = float(p[0]).is_integer(), float(p[1]).is_integer()
            if ix or iy:
                out[tag + ("_xy" if ix and iy else "_x" if ix else "_y")] += 1
    return out


# geoms with FORMA_GEOM_HAS_XF whose transform keeps the lattice: (ux, uy, vx, vy, tx, ty), x' = ux x + vx y + tx
LATTICE_XFS = {
    "scale2": (2.0, 0.0, 0.0, 2.0, 0.0, 0.0),
    "half": (0.5, 0.0, 0.0, 0.5, 0.0, 0.0),
    "translate": (1.0, 0.0, 0.0, 1.0, 3.0 + 5.0 / 16.0, -2.0 - 11.0 / 16.0),
    "rot90": (0.0, 1.0, -1.0, 0.0, float(LATTICE_CANVAS[0]) - 8.0, 0.0),
    "rot180": (-1.0, 0.0, 0.0, -1.0, float(LATTICE_CANVAS[0]), float(LATTICE_CANVAS[1])),
    "rot270": (0.0, -1.0, 1.0, 0.0, 0.0, float(LATTICE_CANVAS[1]) + 16.0),
    "mirror": (-1.0, 0.0, 0.0, 1.0, float(LATTICE_CANVAS[0]), 0.0),
}


def _inverse(xf, p):
    ux, uy, vx, vy, tx, ty = (Fraction(v) for v in xf)
    det = ux * vy - vx * uy
    x, y = Fraction(p[0]) - tx, Fraction(p[1]) - ty
    q = ((vy * x - vx * y) / det, (ux * y - uy * x) / det)
    out = (float(q[0]), float(q[1]))
    assert Fraction(np.float32(out[0]).item()) == q[0] and Fraction(np.float32(out[1]).item()) == q[1]    # exact in f32
    return out


def xf_lines(name, count=120):
    """no-corner lattice lines as the TARGET of the transform: the table holds their exact pre-images"""
    xf = LATTICE_XFS[name]
    pairs = no_corner_lines()
    step = max(1, len(pairs) // count)
    return numbered([(_inverse(xf, a), _inverse(xf, b)) for a, b in pairs[::step]], xf)


# ---- stage 2: streams with a shape of their own ----------------------------------------------------------------------------------
LONG_LINE = ((1.25, 1.5), (3401.25, 851.5))          # slope 1/4 from a 64 x 64 canvas to far off it: 4 250 segments, no corner


def short_lines(count=700):
    """lines of fewer than 3 pixel segments in a row: a workgroup's 256-line window refills"""
    w, h = LATTICE_CANVAS
    out = [p for p in no_corner_lines() if 0 < n_segments((0, p[0], p[1], None), w, h) < 3]
    assert len(out) >= 100
    return [out[i % len(out)] for i in range(count)]


def last_block_lines(last_block, block=2048):
    """a trimmed list of no-corner lattice lines whose stream ends `last_block` segments beyond a multiple of `block`: lines are
    taken in order and one is left out where it would overshoot"""
    w, h = LATTICE_CANVAS
    want = 2 * block + last_block
    out, total = [], 0
    pairs = no_corner_lines()
    for rep in range(4):
        for p in pairs:
            n = n_segments((0, p[0], p[1], None), w, h)
            if 0 < n <= want - total:
                out.append(p); total += n
            if total == want:
                return out
    raise AssertionError("the family cannot be trimmed to %d segments" % want)


# ---- stage 2: general position ---------------------------------------------------------------------------------------------------
def general_pairs(seed, n=GENERAL_LINES_PER_SEED):
    """random f32 lines in 0..300, every third shorter than 3 px"""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        p0 = rng.uniform(0, 300, 2).astype(np.float32)
        p1 = (p0 + rng.uniform(-3, 3, 2)).astype(np.float32) if i % 3 == 0 else rng.uniform(0, 300, 2).astype(np.float32)
        out.append(((float(p0[0]), float(p0[1])), (float(p1[0]), float(p1[1]))))
    return out


def general_lines(seed, affine=False):
    """the lines of one seed; `affine`: every line through a random affine geom of its own (rotation, scale 0.5..1.5, a little
    shear, a translation that keeps most of it on the canvas)"""
    pairs = general_pairs(seed)
    if not affine:
        return numbered(pairs)
    rng = np.random.default_rng(seed + 1000)
    out = []
    for i, (p0, p1) in enumerate(pairs):
        th = rng.uniform(0, 2 * np.pi); sc = rng.uniform(0.5, 1.5); sh = rng.uniform(-0.2, 0.2)
        ux, uy = sc * np.cos(th), sc * np.sin(th)
        vx, vy = -sc * np.sin(th) + sh * ux, sc * np.cos(th) + sh * uy
        cx, cy = 150.0, 150.0
        tx = cx - (ux * cx + vx * cy) + rng.uniform(-20, 20); ty = cy - (uy * cx + vy * cy) + rng.uniform(-20, 20)
        xf = tuple(float(np.float32(v)) for v in (ux, uy, vx, vy, tx, ty))
        out.append((i, p0, p1, xf))
    return out


# ---- polygons for the image test -------------------------------------------------------------------------------------------------
# edge directions, each a lattice slope; every template closes
_TRI_A = [(1, 2), (1, -1), (-2, -1)]
_TRI_B = [(1, 4), (1, -2), (-2, -2)]
_TRI_C = [(0, 3), (1, -1), (-1, -2)]
_STAR = [(8, 2), (-6, 3), (1, -4), (2, 4), (-5, -5)]             # turns through 720 degrees: the middle is wound twice


def _contour(template, origin, scale, reverse=False):
    pts, (x, y) = [], origin
    for dx, dy in template:
        pts.append((x, y))
        x, y = x + dx * scale, y + dy * scale
    assert (x, y) == origin
    return pts[::-1] if reverse else pts


def _corner_free(contours):
    for c in contours:
        for i in range(len(c)):
            a, b = c[i], c[(i + 1) % len(c)]
            if a[1] != b[1] and RM.pieces(RM.transform_point(a, None), RM.transform_point(b, None))[1]:
                return False
    return True


def _place(make, near):
    """the first origin on the quarter-pixel grid at or after `near` (scanning x, then y) at which no edge passes through a pixel
    corner -- decided by the model"""
    for j in range(16):
        for i in range(16):
            cs = make((near[0] + 0.25 * i, near[1] + 0.25 * j))
            if _corner_free(cs):
                return cs
    raise AssertionError("no corner-free placement near %r" % (near,))


def polygon_scenes():
    """name -> (width, height, [(contours, rgba, even_odd)]).  Vertices sit on the quarter-pixel grid, which
    every slope of the family keeps on sixteenths.  Every canvas edge cuts a polygon; one polygon starts at negative x."""
    out = {}
    tri = lambda t, s, rev=False: (lambda o: [_contour(t, o, s, rev)])
    ring = lambda o: [_contour(_TRI_A, o, 8.0), _contour(_TRI_A, (o[0] + 6.0, o[1] + 5.0), 2.5, reverse=True)]
    star = lambda s: (lambda o: [_contour(_STAR, o, s)])
    out["64x64"] = (64, 64, [
        (_place(tri(_TRI_A, 9.0), (5.0, 4.0)), (0.9, 0.1, 0.1, 1.0), False),
        (_place(star(4.0), (12.0, 20.0)), (0.1, 0.5, 0.9, 0.6), False),
        (_place(star(4.0), (20.0, 28.0)), (0.1, 0.8, 0.2, 0.7), True),
        (_place(ring, (30.0, 6.0)), (0.2, 0.2, 0.2, 0.5), False),
        (_place(tri(_TRI_B, 6.0), (-7.0, 30.0)), (0.8, 0.7, 0.1, 0.8), False),          # left part at negative x
        (_place(tri(_TRI_C, 9.0, True), (57.0, 40.0)), (0.5, 0.1, 0.7, 1.0), True),     # cut by the right and bottom edges
        (_place(tri(_TRI_B, 5.0), (40.0, -9.0)), (0.0, 0.0, 0.0, 0.4), False),          # cut by the top edge
    ])
    out["72x40"] = (72, 40, [
        (_place(star(5.0), (20.0, 1.0)), (0.7, 0.2, 0.3, 1.0), True),
        (_place(star(5.0), (28.0, 6.0)), (0.2, 0.3, 0.8, 0.5), False),
        (_place(ring, (-5.0, 8.0)), (0.1, 0.6, 0.4, 0.9), False),
        (_place(tri(_TRI_A, 12.0, True), (52.0, 18.0)), (0.9, 0.6, 0.0, 0.7), False),
        (_place(tri(_TRI_C, 7.0), (10.0, -6.0)), (0.3, 0.3, 0.3, 1.0), False),
    ])
    out["33x17"] = (33, 17, [
        (_place(tri(_TRI_A, 5.0), (-3.0, -2.0)), (0.2, 0.4, 0.9, 1.0), False),
        (_place(star(2.0), (10.0, 3.0)), (0.9, 0.2, 0.2, 0.8), True),
        (_place(tri(_TRI_B, 3.0, True), (28.0, 7.0)), (0.1, 0.7, 0.1, 0.6), False),
    ])
    return out


def polygon_tables(layers):
    """one geom per layer, its contours closed explicitly"""
    xs, ys, ls = [], [], []
    geoms = np.zeros(len(layers), orc.GEOM_DTYPE)
    words, offsets = [], []
    for order, (contours, rgba, even_odd) in enumerate(layers):
        geoms[order]["order"] = order
        offsets.append(len(words))
        words += [(1 << 6) if even_odd else 0, 0] + [int(np.float32(v).view(np.uint32)) for v in rgba]
        for c in contours:
            pts = list(c) + [c[0]]
            xs += [p[0] for p in pts]; ys += [p[1] for p in pts]
            ls += [order] * (len(pts) - 1) + [NONE]
    return dict(x=np.asarray(xs, np.float32), y=np.asarray(ys, np.float32), line_slot=np.asarray(ls[:-1], np.uint32), geoms=geoms,
                style_offsets=np.asarray(offsets, np.uint32), style_words=np.asarray(words, np.uint32),
                unchanged=np.zeros(len(layers), np.uint8), images=np.zeros(0, orc.IMAGE_DTYPE), texels=np.zeros((0, 4), np.uint16))


# ---- stage 1 ---------------------------------------------------------------------------------------------------------------------
# A path is a command list: ("M", x, y) ("L", x, y) ("Q", x1, y1, x2, y2) ("C", ...6) ("RQ", x1, y1, x2, y2, w) ("RC", ...6, w1, w2)
CURVE_KINDS = ("quad", "cubic", "rat_quad", "rat_cubic")
CURVE_SCALES = (4.0, 60.0, 600.0)
CURVE_SEEDS = {"quad": 101, "cubic": 102, "rat_quad": 103, "rat_cubic": 104}
CURVES_PER_FAMILY = 40
SIMILARITY9 = [0.8, 0.1, 5.0, -0.1, 0.8, 7.0, 0.0, 0.0, 1.0]
PROJECTIVE9 = [1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0005, 0.0, 1.0]
DOUBLED_BACK = [("M", 34.06514358520508, 35.70985794067383),
                ("Q", 48.53334426879883, 46.82200241088867, 15.889239311218262, 21.767059326171875)]


def _f(v):
    return float(np.float32(v))


def curve_family(kind, scale):
    """CURVES_PER_FAMILY closed contours of one curve each, control points uniform in [0, scale]^2"""
    rng = np.random.default_rng(CURVE_SEEDS[kind] * 1000 + int(scale))
    out = []
    for _ in range(CURVES_PER_FAMILY):
        p = [_f(v) for v in rng.uniform(0, scale, 8)]
        w = [_f(v) for v in rng.uniform(0.3, 2.5, 2)]
        tail = {"quad": ("Q", *p[2:6]), "cubic": ("C", *p[2:8]), "rat_quad": ("RQ", *p[2:6], w[0]),
                "rat_cubic": ("RC", *p[2:8], w[0], w[1])}[kind]
        out.append([("M", p[0], p[1]), tail])
    return out


def edge_shapes():
    """name -> (commands, 3x3 or None): the shapes a random draw never makes"""
    s2 = _f(np.sqrt(np.float32(2.0)) / np.float32(2.0))
    out = {
        "collinear_quad": ([("M", 2.0, 3.0), ("Q", 10.0, 7.0, 26.0, 15.0), ("L", 5.0, 20.0)], None),
        "collinear_cubic": ([("M", 1.0, 0.5), ("C", 0.0, 0.5, 3.0, 0.5, 2.0, 0.5), ("L", 1.5, 4.0)], None),
        "doubled_back_quad": (DOUBLED_BACK, None),
        "p0_is_p1": ([("M", 4.0, 4.0), ("Q", 4.0, 4.0, 30.0, 12.0), ("L", 10.0, 30.0)], None),
        "p1_is_p2": ([("M", 4.0, 4.0), ("Q", 30.0, 12.0, 30.0, 12.0), ("L", 10.0, 30.0)], None),
        "all_equal": ([("M", 4.0, 4.0), ("Q", 4.0, 4.0, 4.0, 4.0), ("C", 4.0, 4.0, 4.0, 4.0, 4.0, 4.0), ("L", 20.0, 9.0), ("L", 8.0, 25.0)], None),
        "cusp_cubic": ([("M", 10.0, 10.0), ("C", 60.0, 60.0, 10.0, 60.0, 60.0, 10.0)], None),
        "loop_cubic": ([("M", 10.0, 10.0), ("C", 90.0, 70.0, -20.0, 70.0, 60.0, 10.0)], None),
        "tiny": ([("M", 7.0, 7.0), ("Q", 7.03125, 7.015625, 7.0, 7.046875), ("C", 6.98, 7.05, 6.97, 7.02, 6.99, 7.0)], None),
        "weight_0.2": ([("M", 5.0, 40.0), ("RQ", 30.0, -20.0, 55.0, 40.0, _f(0.2))], None),
        "weight_3": ([("M", 5.0, 40.0), ("RQ", 30.0, -20.0, 55.0, 40.0, 3.0)], None),
        "circle": ([("M", 50.0, 10.0), ("RQ", 50.0, -30.0, 10.0, -30.0, s2), ("RQ", -30.0, -30.0, -30.0, 10.0, s2),
                    ("RQ", -30.0, 50.0, 10.0, 50.0, s2), ("RQ", 50.0, 50.0, 50.0, 10.0, s2)], None),
        "rat_cubic_weights": ([("M", 5.0, 5.0), ("RC", 40.0, 0.0, 60.0, 50.0, 10.0, 45.0, _f(0.2), 3.0)], None),
        "near_30000": ([("M", 29990.0, -29950.0), ("Q", 30040.0, -29990.0, 30010.0, -29900.0),
                        ("C", 29950.0, -29850.0, 29900.0, -29990.0, 29960.0, -30020.0)], None),
    }
    rng = np.random.default_rng(300)                             # 300 curves in one path: several 256-thread blocks of the flattener
    cmds = [("M", 100.0, 100.0)]
    x, y = 100.0, 100.0
    for i in range(300):
        p = [_f(v) for v in rng.uniform(-25, 25, 6)]
        nx, ny = _f(min(max(x + p[4], 5.0), 400.0)), _f(min(max(y + p[5], 5.0), 400.0))
        k = i % 3
        if k == 0:
            cmds.append(("Q", _f(x + p[0]), _f(y + p[1]), nx, ny))
        elif k == 1:
            cmds.append(("C", _f(x + p[0]), _f(y + p[1]), _f(x + p[2]), _f(y + p[3]), nx, ny))
        else:
            cmds.append(("RQ", _f(x + p[0]), _f(y + p[1]), nx, ny, _f(rng.uniform(0.4, 2.0))))
        x, y = nx, ny
    out["300_curves"] = (cmds, None)
    for name in ("cusp_cubic", "circle", "rat_cubic_weights", "300_curves"):
        out[name + "/similarity"] = (out[name][0], SIMILARITY9)
        out[name + "/projective"] = (out[name][0], PROJECTIVE9)
    return out


def is_affine9(t9):
    return t9 is not None and t9[6] == 0.0 and t9[7] == 0.0 and t9[8] == 1.0


def oracle_path(cmds, t9=None):
    """the command list as an oracle path; an affine 3x3 that keeps geometry becomes the path's per-point transform (path.rs:726-
    732), any other one transforms the control points"""
    p = orc.Path()
    for c in cmds:
        k, a = c[0], c[1:]
        {"M": p.move_to, "L": p.line_to, "Q": p.quad_to, "C": p.cubic_to, "RQ": p.rat_quad_to, "RC": p.rat_cubic_to}[k](*a)
    p.build()
    if t9 is not None:
        if is_affine9(t9):
            p.affine = (t9[0], t9[3], t9[1], t9[4], t9[2], t9[5])
        else:
            p.transform9(t9)
    return p


def product_path(cmds, t9=None):
    """the same through the product's PathBuilder"""
    from forma_amd import api
    P = api.Point
    b = api.PathBuilder()
    for c in cmds:
        k, a = c[0], c[1:]
        if k == "M": b.move_to(P(*a))
        elif k == "L": b.line_to(P(*a))
        elif k == "Q": b.quad_to(P(a[0], a[1]), P(a[2], a[3]))
        elif k == "C": b.cubic_to(P(a[0], a[1]), P(a[2], a[3]), P(a[4], a[5]))
        elif k == "RQ": b.rat_quad_to(P(a[0], a[1]), P(a[2], a[3]), a[4])
        elif k == "RC": b.rat_cubic_to(P(a[0], a[1]), P(a[2], a[3]), P(a[4], a[5]), a[6], a[7])
    path = b.build()
    return path if t9 is None else path.transform(t9)


def model_segments(cmds, t9=None):
    """the command list as the model's closed chain of segments [(kind, homogeneous control points [n, 3])], the closing chord
    last (PathData::close, path.rs:596-615), the 3x3 applied to the control points"""
    segs, cur, start = [], None, None
    for c in cmds:
        k, a = c[0], c[1:]
        if k == "M":
            assert cur is None, "one contour per path"
            cur = start = (a[0], a[1])
        elif k == "L":
            segs.append(("line", [cur, (a[0], a[1])], None)); cur = (a[0], a[1])
        elif k == "Q":
            segs.append(("quad", [cur, (a[0], a[1]), (a[2], a[3])], None)); cur = (a[2], a[3])
        elif k == "C":
            segs.append(("cubic", [cur, (a[0], a[1]), (a[2], a[3]), (a[4], a[5])], None)); cur = (a[4], a[5])
        elif k == "RQ":
            segs.append(("rat_quad", [cur, (a[0], a[1]), (a[2], a[3])], [1.0, a[4], 1.0])); cur = (a[2], a[3])
        elif k == "RC":
            segs.append(("rat_cubic", [cur, (a[0], a[1]), (a[2], a[3]), (a[4], a[5])], [1.0, a[6], a[7], 1.0])); cur = (a[4], a[5])
    if cur != start:
        segs.append(("line", [cur, start], None))
    return RM.transformed(segs, t9 if t9 is not None else [1, 0, 0, 0, 1, 0, 0, 0, 1])


# ---- how a backend is held to the model: shared by the oracle's tests and the HIP routes' ---------------------------------------
BOUNDS_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "raster_model_bounds.json")
FLOOR = 1e-9          # px: below this a distance is the float64 measures' own rounding (coordinates <= 3e4, eps 2.2e-16, 48 golden steps)


STAGE2 = ["lattice", "lattice_xf", "long_line", "short_lines", "last_block_1", "last_block_63", "last_block_64", "last_block_65",
          "last_block_2047", "general", "general_affine", "corner"]
SHAPES = ["collinear_quad", "collinear_cubic", "doubled_back_quad", "p0_is_p1", "p1_is_p2", "all_equal", "cusp_cubic", "loop_cubic",
          "tiny", "weight_0.2", "weight_3", "circle", "rat_cubic_weights", "near_30000", "300_curves", "cusp_cubic/similarity",
          "cusp_cubic/projective", "circle/similarity", "circle/projective", "rat_cubic_weights/similarity",
          "rat_cubic_weights/projective", "300_curves/similarity", "300_curves/projective"]


def bounds():
    if "bounds" not in _cache:
        with open(BOUNDS_PATH) as f:
            _cache["bounds"] = json.load(f)
    return _cache["bounds"]


def stage2_scenes():
    """name -> (lines, width, height, kind) of every stage-2 family; kind: 'exact' (A and row totals equal the model's),
    'general' (row totals equal, |dA| bounded) or 'corner' (only the lines that agree are exact)"""
    if "scenes" not in _cache:
        w, h = LATTICE_CANVAS
        out = {"lattice": (numbered(no_corner_lines()), w, h, "exact")}
        xf, first = [], 0
        for name in LATTICE_XFS:
            ls = xf_lines(name)
            xf += [(first + i, p0, p1, m) for i, (_, p0, p1, m) in enumerate(ls)]
            first += len(ls)
        out["lattice_xf"] = (xf, w, h, "exact")
        out["long_line"] = (numbered([LONG_LINE, LONG_LINE[::-1]]), 64, 64, "exact")
        out["short_lines"] = (numbered(short_lines()), w, h, "exact")
        for lb in (1, 63, 64, 65, 2047):
            out["last_block_%d" % lb] = (numbered(last_block_lines(lb)), w, h, "exact")
        gw, gh = GENERAL_CANVAS
        for affine in (False, True):
            ls, first = [], 0
            for seed in GENERAL_SEEDS:
                ls += [(first + i, p0, p1, m) for i, (_, p0, p1, m) in enumerate(general_lines(seed, affine))]
                first += GENERAL_LINES_PER_SEED
            out["general_affine" if affine else "general"] = (ls, gw, gh, "general")
        out["corner"] = (numbered(corner_lines()), gw, gh, "corner")
        _cache["scenes"] = out
    return _cache["scenes"]


def model_table(name):
    key = ("model", name)
    if key not in _cache:
        lines, w, h, _ = stage2_scenes()[name]
        _cache[key] = RM.line_area(lines, w, h)[0]
    return _cache[key]


def stream_figures(name, stream):
    """-> (lines that differ from the model, rows whose cover totals differ, max |dA|, the differing layers)"""
    d = RM.difference(model_table(name), RM.decode(stream))
    return len(d), sum(v[0] for v in d.values()), max((v[1] for v in d.values()), default=0), sorted(d)


def check_stream(name, stream, who=""):
    """the assertions of one stage-2 family on one u64 stream (in any order)"""
    lines, w, h, kind = stage2_scenes()[name]
    n_diff, bad_rows, worst, layers = stream_figures(name, stream)
    print("%s %s: %d segments, %d of %d lines differ from the model, %d row totals, max |dA| %d" % (who, name, len(stream), n_diff, len(lines), bad_rows, worst))
    if kind == "exact":
        assert n_diff == 0, (who, name, [lines[k] for k in layers[:4]])
    elif kind == "general":
        b = bounds()["general"]
        assert bad_rows == 0, (who, name, layers[:4])
        assert worst <= b["max_abs_dA"], (who, name, worst)
        assert n_diff <= 0.05 * len(lines), (who, name, n_diff)             # a condition, not a measurement
    else:
        # every line that is not among the differing ones is exact (`difference` lists a line as soon as one pixel differs); how
        # many differ is the oracle's record, and the pinned line is one of them.  Nothing is asserted of the others.
        assert n_diff == bounds()["corner"]["differ"] and 0 in layers, (who, name, n_diff, layers[:4])
        f = orc.seg_fields(np.asarray(stream, np.uint64))
        assert int(f["cover"][f["layer"] == 0].sum()) == RM.CORNER_TIE_COVER_SUM
    return n_diff, bad_rows, worst, layers


def check_polygons(name, image, sorted_stream, who=""):
    """one polygon scene: the image within 1 code value of the model's, the stream's doubled areas equal to the polygons'"""
    w, h, layers = polygon_scenes()[name]
    key = ("polygon", name)
    if key not in _cache:
        table = np.concatenate([RM.polygon_area(cs, w, h, order) for order, (cs, _, _) in enumerate(layers)])
        _cache[key] = (RM.image(layers, w, h), table)
    want, table = _cache[key]
    d = np.abs(np.asarray(image).reshape(h, w * 4).astype(int) - want.astype(int))
    print("%s %s: %d of %d values differ from the model's image (max %d)" % (who, name, int((d > 0).sum()), d.size, int(d.max())))
    assert d.max() <= 1, (who, name, int(d.max()), np.argwhere(d > 1)[:6])
    if sorted_stream is not None:
        assert not RM.difference(table, RM.decode(sorted_stream)), (who, name)


def curve_measures(cmds, t9, x, y):
    """-> dict of the three measures of one flattened contour (x, y: the emitted vertices, the closing point included); the same
    vertices of the same contour are measured once"""
    key = ("measures", repr(cmds), repr(t9), np.asarray(x).tobytes(), np.asarray(y).tobytes())
    if key not in _cache:
        _cache[key] = _curve_measures(cmds, t9, x, y)
    return _cache[key]


def _curve_measures(cmds, t9, x, y):
    segs = model_segments(cmds, t9)
    area, length = RM.curve_area_and_length(segs)
    big = max(float(np.abs(x).max()), float(np.abs(y).max())) if len(x) else 0.0
    a = RM.vertex_distance(segs, x, y)
    return {"a": a, "a_ulps": a / RM.ulp32(big) if big else 0.0, "b": RM.curve_distance(segs, x, y) if len(x) else 0.0,
            "c": abs(RM.polyline_area(x, y) - area), "c_over_length": abs(RM.polyline_area(x, y) - area) / length if length else 0.0}


def worst_of(ms):
    return {k: max(m[k] for m in ms) for k in ms[0]}


ON_CURVE = ("quad", "rat_quad")          # their vertices are evaluated ON the curve (path.rs:447-471): measure (a) is f32 rounding


def check_measures(name, m, rec, on_curve=False, only_c=False, who=""):
    """one family's or shape's worst measures against the recorded ones x the file's margin; measure (c) also against its derived
    bound MAX_ERROR x length"""
    margin = bounds()["stage1"]["margin"]
    print("%s %s: a %.3g px (%.2f ulp of the largest coordinate), b %.3g px, c %.3g px^2 (%.3g px per px of length)" % (
        who, name, m["a"], m["a_ulps"], m["b"], m["c"], m["c_over_length"]))
    assert m["c_over_length"] <= RM.MAX_ERROR, (who, name, m)
    assert m["c"] <= max(rec["c"] * margin, FLOOR), (who, name, m, rec)
    if only_c:
        return
    if on_curve:
        assert m["a_ulps"] <= rec["a_ulps"] * margin, (who, name, m, rec)
    assert m["a"] <= max(rec["a"] * margin, FLOOR), (who, name, m, rec)
    assert m["b"] <= max(rec["b"] * margin, FLOOR), (who, name, m, rec)
