"""A float64 model of stroking, written from geometry: what the outline of a polyline IS, not how the kernels compute it.

A stroke of half width hw around a polyline is the union of
  * a BODY per line of non-zero length: the rectangle of all points within hw of the line, measured across it;
  * a JOIN at every vertex where the direction turns, on the OUTER side of the turn (the inner side is covered by the bodies):
    BEVEL the triangle between the vertex and the two body corners; MITER that triangle extended to where the two outer edges
    meet, at distance hw / cos(theta / 2) from the vertex along the bisector (theta = the turn angle), unless that ratio
    exceeds the miter limit; ROUND the circular sector, flattened into the fewest equal steps whose chords stay within
    1/16 px of the circle;
  * a CAP at both ends of an open contour: nothing (BUTT), half a square (SQUARE) or half a disc (ROUND).
A contour is closed when its first and last point are the same f32 values bit for bit; then the first vertex gets a join too.
Lines of zero length draw nothing and joins look through them.

The LAYOUT rule (include/forma_hip.h, forma_hip_geometry_append_stroked), restated: every piece of k lines is k + 1 points, the
last one repeats the first and carries NONE, the others carry the slot of the source line (a join: the line that leaves the
vertex; a cap: its end's line).  Pieces come in source-point order: for point i its join or start cap, then the body of line i;
the end cap comes with the contour's last point.  Points outside every stroke range pass through.  All pieces are wound the same
way: with y up, clockwise (a body runs p0+o, p1+o, p1-o, p0-o with o = hw * the left normal).

The model takes the f32 points the device strokes and works in float64; `stroke_append` returns float64 coordinates.  Rounded
to f32 they equal the device's bit for bit wherever the geometry is exact in f32 (stroke_cases.exact_families).
"""
import math

import numpy as np

NONE = 0xFFFFFFFF
BEVEL, MITER, ROUND = 0, 1, 2
BUTT, SQUARE, ROUND_CAP = 0, 1, 2
MAX_ERROR = 1.0 / 16.0                           # the flattener's kMaxError


def min_steps(phi, hw):
    """the fewest equal steps over the angle phi whose chord's sagitta hw * (1 - cos(step / 2)) is <= 1/16"""
    c = 1.0 - MAX_ERROR / hw
    step = 2.0 * math.pi if c <= -1.0 else 2.0 * math.acos(c)
    return max(1, math.ceil(phi / step - 1e-12))


def _left_normal(d):
    n = math.hypot(d[0], d[1])
    return (-d[1] / n, d[0] / n)


def _rot_cw(u, a):
    """u turned clockwise (y up) by a"""
    c, s = math.cos(a), math.sin(a)
    return (u[0] * c + u[1] * s, u[1] * c - u[0] * s)


class Piece:
    def __init__(self, kind, src, pts, slot, centre=None, angle=None, steps=None):
        self.kind, self.src, self.pts, self.slot = kind, src, pts, slot
        self.centre, self.angle, self.steps = centre, angle, steps     # joins and caps: the vertex; fans: the angle and step count

    def area2(self):
        """twice the signed area (y up: negative = clockwise)"""
        p = self.pts
        return sum(p[i][0] * p[i + 1][1] - p[i + 1][0] * p[i][1] for i in range(len(p) - 1))


def _fan(kind, src, v, us, ue, phi, hw, slot):
    n = min_steps(phi, hw)
    pts = [v, (v[0] + us[0], v[1] + us[1])]
    for k in range(1, n):
        u = _rot_cw(us, k * phi / n)
        pts.append((v[0] + u[0], v[1] + u[1]))
    pts += [(v[0] + ue[0], v[1] + ue[1]), v]
    return Piece(kind, src, pts, slot, centre=v, angle=phi, steps=n)


def stroke_contour(x, y, slots, first, last, hw, join, cap, miter_limit):
    """the pieces of the contour of points first .. last (inclusive) of the f32 arrays x, y, in layout order"""
    X = [float(v) for v in x[first:last + 1]]
    Y = [float(v) for v in y[first:last + 1]]
    n = len(X)
    closed = n > 1 and np.float32(x[first]).tobytes() == np.float32(x[last]).tobytes() and \
        np.float32(y[first]).tobytes() == np.float32(y[last]).tobytes()
    d = [(X[i + 1] - X[i], Y[i + 1] - Y[i]) for i in range(n - 1)]
    live = [i for i in range(n - 1) if d[i] != (0.0, 0.0)]
    out = []
    if not live:
        return out
    for idx, i in enumerate(live):
        v = (X[i], Y[i])
        s = int(slots[first + i])
        nb = _left_normal(d[i])
        ob = (hw * nb[0], hw * nb[1])
        eb = (hw * nb[1], -hw * nb[0])                # hw * the direction of line i
        prev = live[idx - 1] if idx > 0 else (live[-1] if closed else None)
        if prev is None:                              # the start of an open contour
            if cap == SQUARE:
                b = (v[0] - eb[0], v[1] - eb[1])
                out.append(Piece("cap_square", first + i, [(b[0] + ob[0], b[1] + ob[1]), (v[0] + ob[0], v[1] + ob[1]), (v[0] - ob[0], v[1] - ob[1]),
                                                           (b[0] - ob[0], b[1] - ob[1]), (b[0] + ob[0], b[1] + ob[1])], s, centre=v))
            elif cap == ROUND_CAP:
                out.append(_fan("cap_round", first + i, v, (-ob[0], -ob[1]), ob, math.pi, hw, s))
        else:
            a = d[prev]
            cross = a[0] * d[i][1] - a[1] * d[i][0]
            dot = a[0] * d[i][0] + a[1] * d[i][1]
            if not (cross == 0.0 and dot > 0.0):
                na = _left_normal(a)
                oa = (hw * na[0], hw * na[1])
                # the outer side: right of the path on a left turn, left of it on a right turn; an exact U-turn takes the left
                if cross > 0.0:
                    us, ue = (-ob[0], -ob[1]), (-oa[0], -oa[1])
                else:
                    us, ue = oa, ob
                theta = abs(math.atan2(cross, dot))   # the turn angle
                kind = "bevel"
                if join == ROUND:
                    out.append(_fan("round", first + i, v, us, ue, theta, hw, s))
                    kind = None
                elif join == MITER and theta < math.pi and 1.0 / math.cos(theta / 2.0) <= miter_limit:
                    bis = (us[0] + ue[0], us[1] + ue[1])
                    bl = math.hypot(bis[0], bis[1])
                    r = hw / math.cos(theta / 2.0)
                    tip = (v[0] + r * bis[0] / bl, v[1] + r * bis[1] / bl)
                    out.append(Piece("miter", first + i, [v, (v[0] + us[0], v[1] + us[1]), tip, (v[0] + ue[0], v[1] + ue[1]), v], s,
                                     centre=v, angle=theta))
                    kind = None
                if kind:
                    out.append(Piece("bevel", first + i, [v, (v[0] + us[0], v[1] + us[1]), (v[0] + ue[0], v[1] + ue[1]), v], s, centre=v, angle=theta))
        w = (X[i + 1], Y[i + 1])
        out.append(Piece("body", first + i, [(v[0] + ob[0], v[1] + ob[1]), (w[0] + ob[0], w[1] + ob[1]), (w[0] - ob[0], w[1] - ob[1]),
                                             (v[0] - ob[0], v[1] - ob[1]), (v[0] + ob[0], v[1] + ob[1])], s))
    if not closed and cap != BUTT:
        i = live[-1]
        v = (X[i + 1], Y[i + 1])
        s = int(slots[first + i])
        nb = _left_normal(d[i])
        ob = (hw * nb[0], hw * nb[1])
        eb = (hw * nb[1], -hw * nb[0])
        if cap == SQUARE:
            f = (v[0] + eb[0], v[1] + eb[1])
            out.append(Piece("cap_square", last, [(v[0] + ob[0], v[1] + ob[1]), (f[0] + ob[0], f[1] + ob[1]), (f[0] - ob[0], f[1] - ob[1]),
                                                  (v[0] - ob[0], v[1] - ob[1]), (v[0] + ob[0], v[1] + ob[1])], s, centre=v))
        else:
            out.append(_fan("cap_round", last, v, ob, (-ob[0], -ob[1]), math.pi, hw, s))
    return out


def stroke_append(x, y, line_slot, strokes):
    """One append: x, y f32 points (after flattening and affines), line_slot one entry per point (NONE ends a contour), strokes =
    [(first, count, half_width, miter_limit, join, cap)] ascending.  Returns (x64, y64, slot, pieces): the store's new points
    in layout order and the pieces, each with .at = its first output point."""
    x = np.asarray(x, np.float32); y = np.asarray(y, np.float32)
    ox, oy, os_, pieces = [], [], [], []
    i, n = 0, len(x)
    for first, count, hw, limit, join, cap in list(strokes) + [(n, 0, 0, 0, 0, 0)]:
        while i < first:                              # outside every range: as it is
            ox.append(float(x[i])); oy.append(float(y[i])); os_.append(int(line_slot[i])); i += 1
        end = first + count
        while i < end:
            last = i
            while int(line_slot[last]) != NONE:
                last += 1
            for p in stroke_contour(x, y, line_slot, i, last, float(np.float32(hw)), join, cap, float(np.float32(limit))):
                p.at = len(ox)
                pieces.append(p)
                for k, (px, py) in enumerate(p.pts):
                    ox.append(px); oy.append(py); os_.append(NONE if k == len(p.pts) - 1 else p.slot)
            i = last + 1
    return np.asarray(ox, np.float64), np.asarray(oy, np.float64), np.asarray(os_, np.uint32), pieces


def union_area(polys):
    """The area of the union of closed polygons ([(x, y), ...], first point repeated at the end) that are all wound the same
    way, i.e. of the set where the winding number is not zero — exactly, up to float64 rounding.  The plane is cut into
    horizontal slabs at every vertex and every crossing of two edges; inside a slab no two edges cross, so the covered spans are
    trapezoids between neighbouring edges."""
    edges = []
    for p in polys:
        for (x0, y0), (x1, y1) in zip(p[:-1], p[1:]):
            if y0 < y1:
                edges.append((x0, y0, x1, y1, 1))      # (x, y) of the lower end, of the upper end, the winding it adds
            elif y0 > y1:
                edges.append((x1, y1, x0, y0, -1))
    ys = {e[1] for e in edges} | {e[3] for e in edges}
    for i, a in enumerate(edges):
        for b in edges[i + 1:]:
            lo, hi = max(a[1], b[1]), min(a[3], b[3])
            if lo >= hi:
                continue
            # a: x = ax + (y - ay) * sa
            sa, sb = (a[2] - a[0]) / (a[3] - a[1]), (b[2] - b[0]) / (b[3] - b[1])
            if sa == sb:
                continue
            yc = ((b[0] - b[1] * sb) - (a[0] - a[1] * sa)) / (sa - sb)
            if lo < yc < hi:
                ys.add(yc)
    ys = sorted(ys)
    area = 0.0
    for y0, y1 in zip(ys[:-1], ys[1:]):
        ym = 0.5 * (y0 + y1)
        live = []
        for e in edges:
            if e[1] <= y0 and e[3] >= y1:
                sl = (e[2] - e[0]) / (e[3] - e[1])
                live.append((e[0] + (ym - e[1]) * sl, e[0] + (y0 - e[1]) * sl, e[0] + (y1 - e[1]) * sl, e[4]))
        live.sort()
        wind = 0
        for k, (_, xa0, xa1, w) in enumerate(live[:-1]):
            wind += w
            if wind != 0:
                _, xb0, xb1, _ = live[k + 1]
                area += 0.5 * ((xb0 - xa0) + (xb1 - xa1)) * (y1 - y0)
    return area
