"""Strokes expanded on the device (forma_hip_geometry_append_stroked, `Path.stroke`, `svg.load(strokes=True)`) against
stroke_model.py, which test_stroke_model.py pins to the oracle on the CPU.

  1  families whose geometry is exact in f32: the store equals the model bit for bit, in order, slots included;
  2  random f32 polylines: every vertex within a bound derived from the f32 roundings of the source points (below), piece
     counts and kinds as the model's, fans with the minimal step count or one more;
  3  sizes at which the count, the scan or the emit pass can go wrong, checked as in 2;
  4  the store's invariant: an append leaves the store what a from-scratch build of the surviving pushes would hold;
  5  one scene through every route of the public API: the same store everywhere, the image within one code value of the
     oracle drawing the model's pieces.

Bounds (u = 2^-24, M = the largest coordinate magnitude involved, hw = the half width):
  body / cap vertex   half an ulp on the stored point (u * M) plus 5.5 relative roundings through d, len, s, o (5.5 u * hw):
                      within 2^-21 * (M + hw) of the model's vertex, in each coordinate, and so of its distance hw from the
                      centre line's end.  The far corners of a square cap add two such offsets: 2^-20 * (M + hw).
  miter tip           hw * r from the vertex, r = 1 / cos(theta / 2), within 2^-20 * (M + hw * r^3): the cancellation in
                      hw^2 + oa . ob costs a factor r^2.
  round vertex        hw from the vertex within 2^-20 * (M + hw); chord midpoints never more than 1/16 + that inside.
"""
import ctypes as C
import math

import numpy as np
import pytest

import stroke_cases as SC
import stroke_model as SM

pytestmark = pytest.mark.gpu

NONE = SM.NONE
E_ARG = -1
CLEAR = (1.0, 1.0, 1.0, 1.0)


def _api():
    from forma_amd import api
    return api


@pytest.fixture(scope="module")
def ctx():
    import forma_amd
    c = forma_amd.Context(0)
    yield c
    c.close()


def empty(c):
    c.set_geometry(np.zeros(0, np.float32), np.zeros(0, np.float32), np.zeros(0, np.uint32))
    c.n_points = 0


def stroked(c, case):
    """the case appended to an EMPTY store; returns (x, y, slot with the last NONE appended)"""
    empty(c)
    added = c.geometry_append_stroked(case.t, case.line_slot, case.affines, case.strokes)
    x, y, ls = c.read_geometry()
    assert len(x) == added
    return x, y, np.concatenate((ls, [NONE])).astype(np.uint32) if len(x) else ls


def same_bits(a, b):
    return all(len(p) == len(q) and np.array_equal(np.ascontiguousarray(p).view(np.uint32), np.ascontiguousarray(q).view(np.uint32))
               for p, q in zip(a, b))


# 1 ----------------------------------------------------------------------------------------------------------------------------------
def test_exact_families_bit_for_bit(ctx):
    cases = SC.exact_families()
    assert len(cases) >= 15
    for case in cases:
        x, y, slot = stroked(ctx, case)
        mx, my, ms, pieces = case.model()
        assert len(pieces) > 0
        want = (mx.astype(np.float32), my.astype(np.float32), ms)
        assert np.array_equal(want[0].astype(np.float64), mx) and np.array_equal(want[1].astype(np.float64), my), case.name + ": the family is not exact in f32"
        assert same_bits((x, y, slot), want), (case.name, [p.kind for p in pieces])


# 2 ----------------------------------------------------------------------------------------------------------------------------------
def check_against_source(case, x, y, slot):
    """device output of one case against the model and the source points, in float64; returns the number of pieces checked"""
    mx, my, ms, pieces = case.model()
    sx, sy = case.source()
    X, Y = x.astype(np.float64), y.astype(np.float64)
    M = max(float(np.abs(sx).max()), float(np.abs(sy).max()), float(np.abs(X).max()) if len(X) else 0.0, float(np.abs(Y).max()) if len(Y) else 0.0)
    style_of = {}
    for first, count, hw, limit, join, cap in case.strokes:
        for i in range(first, first + count):
            style_of[i] = float(np.float32(hw))
    at = 0                                            # walks the device output
    mat = 0                                           # walks the model output (points outside the ranges pass through)
    for p in pieces:
        while mat < p.at:                             # passed-through points: bit for bit
            assert X[at] == mx[mat] and Y[at] == my[mat] and slot[at] == ms[mat], (case.name, "pass-through", at)
            at += 1; mat += 1
        mat += len(p.pts)
        end = at
        while slot[end] != NONE:
            end += 1
        n = end - at + 1                              # the device's piece: points at .. end
        hw = style_of[p.src]
        b_body = 2.0 ** -21 * (M + hw)
        what = (case.name, p.kind, p.src)
        assert list(slot[at:end]) == [p.slot] * (n - 1), what
        assert X[at] == X[end] and Y[at] == Y[end], what                        # closed: the last point repeats the first
        dev = list(zip(X[at:end + 1], Y[at:end + 1]))
        if p.kind in ("body", "bevel", "miter", "cap_square"):
            assert n == len(p.pts), what + (n,)
            for k, (d, m) in enumerate(zip(dev, p.pts)):
                bound = b_body
                if p.kind == "cap_square" and math.hypot(m[0] - p.centre[0], m[1] - p.centre[1]) > 1.2 * hw:
                    bound = 2.0 ** -20 * (M + hw)                               # a far corner: two offsets
                if p.kind == "miter" and k == 2:
                    r = 1.0 / math.cos(p.angle / 2.0)
                    bound = 2.0 ** -20 * (M + hw * r ** 3)
                    assert abs(math.hypot(d[0] - p.centre[0], d[1] - p.centre[1]) - hw * r) <= bound, what
                assert abs(d[0] - m[0]) <= bound and abs(d[1] - m[1]) <= bound, what + (k, d, m)
            if p.kind == "body":                                                # at hw from its centre line's end
                ends = [p.src, p.src + 1, p.src + 1, p.src]
                for d, e in zip(dev[:4], ends):
                    assert abs(math.hypot(d[0] - float(sx[e]), d[1] - float(sy[e])) - hw) <= b_body, what
        else:                                                                   # a fan: v, n + 1 rim points, v
            steps = n - 3
            assert p.steps <= steps <= p.steps + 1, what + (steps, p.steps)
            v = p.centre
            b_round = 2.0 ** -20 * (M + hw)
            assert dev[0] == v and dev[-1] == v, what
            rim = dev[1:-1]
            for d in rim:
                assert abs(math.hypot(d[0] - v[0], d[1] - v[1]) - hw) <= b_round, what
            for d, m in ((rim[0], p.pts[1]), (rim[-1], p.pts[-2])):             # the fan starts and ends on the bodies' corners
                assert abs(d[0] - m[0]) <= b_body and abs(d[1] - m[1]) <= b_body, what
            chords = []
            for a, b in zip(rim[:-1], rim[1:]):
                mid = (0.5 * (a[0] + b[0]), 0.5 * (a[1] + b[1]))
                assert math.hypot(mid[0] - v[0], mid[1] - v[1]) >= hw - SM.MAX_ERROR - b_round, what
                chords.append(math.hypot(b[0] - a[0], b[1] - a[1]))
            assert max(chords) - min(chords) <= 4.0 * b_round, what              # equal angular steps
            # the fan turns the way the model's does: its signed area has the model's sign
            a2 = sum(dev[i][0] * dev[i + 1][1] - dev[i + 1][0] * dev[i][1] for i in range(len(dev) - 1))
            assert a2 <= 1e-6 * (1.0 + abs(a2)), what
        at = end + 1
    while mat < len(mx):
        assert X[at] == mx[mat] and Y[at] == my[mat] and slot[at] == ms[mat], (case.name, "pass-through", at)
        at += 1; mat += 1
    assert at == len(X), (case.name, at, len(X))
    return len(pieces)


def test_random_polylines_within_the_derived_bounds(ctx):
    cases = SC.random_cases()
    n = sum(check_against_source(case, *stroked(ctx, case)) for case in cases)
    assert len(cases) == 24 and n > 200


# 3 ----------------------------------------------------------------------------------------------------------------------------------
def _long(rng, n, closed=False):
    return SC.random_polyline(rng, n, lo=16.0, hi=1000.0, closed=closed)


@pytest.mark.parametrize("n", [255, 256, 257, 1023, 1025, 4097])
def test_round_joins_around_the_workgroup_sizes(ctx, n):
    rng = np.random.default_rng(1000 + n)
    case = SC.Case(f"round-{n}", [_long(rng, n)], 2.5, SM.ROUND, SM.ROUND_CAP)
    assert check_against_source(case, *stroked(ctx, case)) >= n


def _shape_cases():
    rng = np.random.default_rng(77)
    out = [SC.Case("one-contour-of-5000", [_long(rng, 5000, closed=True)], 2.0, SM.ROUND, SM.BUTT)]
    two = [[(16.0 + 8.0 * (k % 100), 16.0 + 12.0 * (k // 100)), (21.5 + 8.0 * (k % 100), 20.25 + 12.0 * (k // 100))] for k in range(2000)]
    out.append(SC.Case("2000-two-point-contours", two, 1.5, SM.ROUND, SM.ROUND_CAP, slots=[k % 7 for k in range(2000)]))
    # a contour break exactly on a workgroup edge: the first contour fills workgroup 0, the second starts workgroup 1
    out.append(SC.Case("break-on-a-workgroup-edge", [_long(rng, 256), _long(rng, 256, closed=True), _long(rng, 40)], 3.0, SM.ROUND, SM.SQUARE, slots=[0, 1, 2]))
    z = _long(rng, 6)
    zl = [z[0], z[0], z[1], z[2], z[2], z[2], z[3], z[4], z[5], z[5]]           # zero-length lines at the start, before joins, at the end
    out.append(SC.Case("zero-lengths", [zl, [z[0], z[0]], _long(rng, 5)], 2.0, SM.ROUND, SM.ROUND_CAP))
    # a stroked range between two filled ranges in one call: contours 0 and 3 pass through
    fill_a, fill_b = [(5.0, 5.0), (9.0, 5.0), (9.0, 9.0), (5.0, 5.0)], [(15.0, 5.0), (19.0, 5.0), (19.0, 9.0), (15.0, 5.0)]
    out.append(SC.Case("stroked-between-filled", [fill_a, _long(rng, 300), _long(rng, 9, closed=True), fill_b], 0, 0, 0, slots=[0, 1, 1, 2],
                       stroke_contours=[(1, 2, 2.0, 4.0, SM.MITER, SM.SQUARE), (2, 3, 3.5, 2.0, SM.ROUND, SM.BUTT)]))
    # an affine range on a stroked range (and one on a filled one): the stroke is of the transformed points
    aff = SC.Case("affine-on-a-stroked-range", [fill_a, _long(rng, 200), fill_b], 0, 0, 0, slots=[0, 1, 2],
                  stroke_contours=[(1, 2, 2.0, 4.0, SM.BEVEL, SM.ROUND_CAP)])
    aff.affines = [(0, 4, [0.5, 0.0, 0.0, 0.5, 3.0, 5.0]), (4, 200, [0.8, 0.1, -0.1, 0.8, 5.0, 7.0])]
    out.append(aff)
    return out


def test_shapes_where_count_scan_and_emit_can_go_wrong(ctx):
    for case in _shape_cases():
        x, y, slot = stroked(ctx, case)
        n = check_against_source(case, x, y, slot)
        print(case.name, len(case.x), "source points ->", len(x), "points in", n, "pieces")
        assert n > 0


# 4 ----------------------------------------------------------------------------------------------------------------------------------
def _fill_case(dx=0.0, slot=0):
    return SC.Case("fill", [[(5.0 + dx, 5.0), (9.0 + dx, 5.0), (9.0 + dx, 9.0), (5.0 + dx, 5.0)]], 0, 0, 0, slots=[slot], stroke_contours=[])


def test_no_stroke_ranges_is_the_plain_append(ctx):
    rng = np.random.default_rng(5)
    case = SC.Case("plain", [_long(rng, 300), _long(rng, 7, closed=True)], 0, 0, 0, slots=[0, 1], stroke_contours=[])
    case.affines = [(0, 300, [0.8, 0.1, -0.1, 0.8, 5.0, 7.0])]
    empty(ctx)
    ctx.geometry_append(case.t, case.line_slot, case.affines)
    a = ctx.read_geometry()
    c0 = ctx.counters()
    empty(ctx)
    assert ctx.geometry_append_stroked(case.t, case.line_slot, case.affines, ()) == 307
    assert same_bits(ctx.read_geometry(), a) and len(a[0]) == 307
    assert ctx.counters()["geometry_appends"] == c0["geometry_appends"] + 1


def test_an_append_leaves_what_a_from_scratch_build_would_hold(ctx):
    rng = np.random.default_rng(6)
    line = _long(rng, 120)
    S = SC.Case("S", [line], 2.0, SM.ROUND, SM.ROUND_CAP, slots=[1])
    F0, F2 = _fill_case(0.0, 0), _fill_case(20.0, 2)
    # behind existing content, call by call ...
    empty(ctx)
    for case in (F0, S, F2):
        ctx.geometry_append_stroked(case.t, case.line_slot, case.affines, case.strokes)
    apart = ctx.read_geometry()
    # ... against one call on an empty store that holds the same pushes
    both = SC.Case("F0+S+F2", F0.contours + S.contours + F2.contours, 0, 0, 0, slots=[0, 1, 2], stroke_contours=[(1, 2, 2.0, 4.0, SM.ROUND, SM.ROUND_CAP)])
    together = stroked(ctx, both)
    assert same_bits(apart, (together[0], together[1], together[2][:-1]))
    alone = stroked(ctx, S)
    n_s = len(alone[0])
    assert same_bits([a[4:4 + n_s] for a in apart[:2]], alone[:2]) and np.array_equal(apart[2][4:4 + n_s], alone[2])
    # forma_hip_geometry_retain over ranges that include stroked pushes: drop F0, keep S and F2, slots renumbered
    empty(ctx)
    for case in (F0, S, F2):
        ctx.geometry_append_stroked(case.t, case.line_slot, case.affines, case.strokes)
    assert same_bits(ctx.read_geometry(), apart)
    ctx.geometry_retain([(4, n_s + 4)], np.array([NONE, 0, 1], np.uint32))
    kept = ctx.read_geometry()
    empty(ctx)
    S0 = SC.Case("S0", [line], 2.0, SM.ROUND, SM.ROUND_CAP, slots=[0])
    for case in (S0, _fill_case(20.0, 1)):
        ctx.geometry_append_stroked(case.t, case.line_slot, case.affines, case.strokes)
    assert same_bits(kept, ctx.read_geometry())
    assert ctx.counters()["geometry_points"] == n_s + 4


def test_argument_errors_leave_the_store_alone(ctx):
    from forma_amd import FormaError
    rng = np.random.default_rng(7)
    stroked(ctx, SC.Case("content", [_long(rng, 30)], 2.0, SM.ROUND, SM.ROUND_CAP))
    before = ctx.read_geometry()
    n_before = ctx.n_points
    case = SC.Case("args", [_long(rng, 10), _long(rng, 12), _long(rng, 8)], 0, 0, 0, slots=[0, 1, 2], stroke_contours=[])
    ok = (2.0, 4.0, SM.MITER, SM.BUTT)
    bad = {
        "ranges out of order": [(10, 12) + ok, (0, 10) + ok],
        "overlapping ranges": [(0, 22) + ok, (10, 12) + ok],
        "a range beyond the points": [(22, 9) + ok],
        "a range that does not begin at a contour start": [(3, 7) + ok],
        "a range that does not end on a NONE": [(0, 9) + ok],
        "zero width": [(0, 10, 0.0, 4.0, SM.MITER, SM.BUTT)],
        "negative width": [(0, 10, -1.0, 4.0, SM.MITER, SM.BUTT)],
        "NaN width": [(0, 10, float("nan"), 4.0, SM.MITER, SM.BUTT)],
        "infinite width": [(0, 10, float("inf"), 4.0, SM.MITER, SM.BUTT)],
        "miter limit below 1": [(0, 10, 2.0, 0.99, SM.MITER, SM.BUTT)],
        "NaN miter limit": [(0, 10, 2.0, float("nan"), SM.MITER, SM.BUTT)],
        "unknown join": [(0, 10, 2.0, 4.0, 3, SM.BUTT)],
        "unknown cap": [(0, 10, 2.0, 4.0, SM.MITER, 7)],
    }
    for what, strokes in bad.items():
        with pytest.raises(FormaError) as e:
            ctx.geometry_append_stroked(case.t, case.line_slot, (), strokes)
        assert e.value.code == E_ARG, what
        assert same_bits(ctx.read_geometry(), before), what
    ctx.n_points = n_before
    # ... and a well-formed call with the same tables goes through
    assert ctx.geometry_append_stroked(case.t, case.line_slot, (), [(10, 12) + ok]) > 18
    after = ctx.read_geometry()
    assert same_bits([a[:len(before[0])] for a in after[:2]], before[:2])


# 5 ----------------------------------------------------------------------------------------------------------------------------------
W = H = 128


def _render_host(r, comp, w=W, h=H):
    api = _api()
    img = np.zeros(w * h * 4, np.uint8)
    r.render(comp, api.BufferBuilder(img, api.LinearLayout(w, w * 4, h)).build(), api.RGBA, api.Color(*CLEAR), None)
    return img.reshape(h, w, 4)


def _near(a, b, tol, what):
    d = np.abs(a.astype(int) - b.astype(int))
    assert d.max() <= tol, (what, int(d.max()), int((d > tol).sum()))


_ORACLE = {}


def oracle_image(exact):
    if exact not in _ORACLE:
        _ORACLE[exact] = SC.ref_render(SC.scene_model(SC.api_scene(exact)), W, H)
    return _ORACLE[exact]


_BASE = {}


def base_route(exact):
    """the scene through Renderer(): its store and image, computed once"""
    if exact not in _BASE:
        api = _api()
        r = api.Renderer(0)
        img = _render_host(r, SC.scene_composition(api, SC.api_scene(exact)))
        geo = r.read_geometry()
        assert same_bits(geo, [r.host_tables[k] for k in ("x", "y", "line_slot")])          # the host's copy is the device's store
        r._ctx.close()
        _BASE[exact] = (geo, img)
    return _BASE[exact]


@pytest.mark.parametrize("exact", [False, True])
def test_default_renderer_against_the_model(exact):
    geo, img = base_route(exact)
    want = oracle_image(exact)
    d = np.abs(img.astype(int) - want.astype(int))
    print("exact" if exact else "general", "scene: max |image - oracle| =", int(d.max()), "pixels off:", int((d > 0).sum()))
    _near(img, want, 1, "default renderer vs oracle")
    # the store against the model, layer by layer: what the routes below are compared with is right
    layers = SC.api_scene(exact)
    polys = SC.scene_model(layers)
    mx = np.asarray([p[0] for lay in polys for poly in lay[0] for p in poly])
    my = np.asarray([p[1] for lay in polys for poly in lay[0] for p in poly])
    if exact:
        assert same_bits(geo[:2], (mx.astype(np.float32), my.astype(np.float32)))
        # identical geometry, identical pixels: the same pieces pushed as fill paths through the same renderer
        api = _api()
        comp = api.Composition()
        for k, (pl, color, _) in enumerate(polys):
            lay = comp.get_mut_or_insert_default(api.Order(k))
            for poly in pl:
                pb = api.PathBuilder()
                pb.move_to(api.Point(float(np.float32(poly[0][0])), float(np.float32(poly[0][1]))))
                for p in poly[1:]:
                    pb.line_to(api.Point(float(np.float32(p[0])), float(np.float32(p[1]))))
                lay.insert(pb.build())
            lay.set_props(api.Props(func=api.Func.Draw(api.Style(fill=api.Fill.Solid(api.Color(*color))))))
        r = api.Renderer(0)
        assert np.array_equal(_render_host(r, comp), img)
        r._ctx.close()
        assert np.array_equal(img, want), "exact families: the image is the oracle's"
    else:
        assert len(geo[0]) >= len(mx) and len(geo[0]) - len(mx) <= 40           # (a fan may take one step more than the model's)


@pytest.mark.parametrize("exact", [False, True])
def test_resident_renderer_after_inserting_and_removing_stroked_layers(exact):
    import gc
    api = _api()
    layers = SC.api_scene(exact)
    geo, img = base_route(exact)
    r = api.Renderer(0, resident_geometry=True)
    comp = SC.scene_composition(api, layers[:2])
    _render_host(r, comp)
    # two stroked layers that go away again, with the rest of the scene inserted behind them
    # (compact_geom collects once the garbage is half the store, counted in SOURCE lines: 30 + 12 of them against the scene's)
    zig = [(4.0 + 4.0 * k, 60.0 + 20.0 * (k % 2) + 0.25 * k) for k in range(31)]
    ring = [(64.0 + 40.0 * math.cos(0.5 * k), 64.0 + 40.0 * math.sin(0.5 * k)) for k in range(12)]
    extra = [("stroke", [zig], [False], (6.0, SM.ROUND, SM.ROUND_CAP, 4.0), (0, 0, 0, 1), "NonZero"),
             ("stroke", [ring], [True], (3.0, SM.MITER, SM.BUTT, 4.0), (0, 0, 0, 1), "NonZero")]
    for k, lay in enumerate(extra):
        comp.get_mut_or_insert_default(api.Order(100 + k)).insert(SC.scene_path(api, lay))
    _render_host(r, comp)
    for k, lay in enumerate(layers[2:]):
        comp.get_mut_or_insert_default(api.Order(2 + k)).insert(SC.scene_path(api, lay)).set_props(
            api.Props(func=api.Func.Draw(api.Style(fill=api.Fill.Solid(api.Color(*lay[4]))))))
    _render_host(r, comp)
    for k in range(len(extra)):
        gone = comp.remove(api.Order(100 + k))
        del gone
    gc.collect()
    got = _render_host(r, comp)
    c = r.counters()
    assert c["geometry_retains"] >= 1 and c["geometry_uploads"] <= 1
    assert same_bits(r.read_geometry(), geo)
    assert np.array_equal(got, img)
    _near(got, oracle_image(exact), 1, "resident renderer vs oracle")
    r._ctx.close()


def test_three_frame_slots_and_device_targets():
    import torch
    from test_gpu_device_target import encode
    api = _api()
    geo, img = base_route(False)
    want = oracle_image(False)
    comp = SC.scene_composition(api, SC.api_scene(False))
    dev = torch.device("cuda", 0)
    r = api.Renderer(0, frames_in_flight=3)
    outs = [torch.zeros((H, W, 4), dtype=torch.uint8, device=dev) for _ in range(4)]
    for out in outs:
        r.render_to_device(comp, out, clear_color=api.Color(*CLEAR))
    r._ctx.sync()
    torch.cuda.synchronize()
    assert same_bits(r.read_geometry(), geo)
    for out in outs:
        a = out.cpu().numpy()
        assert np.array_equal(a, img)
        _near(a, want, 1, "three frame slots vs oracle")
    r._ctx.close()
    r = api.Renderer(0)
    u8 = r.render_to_device(comp, torch.zeros((H, W, 4), dtype=torch.uint8, device=dev), clear_color=api.Color(*CLEAR))
    f16 = r.render_to_device(comp, torch.zeros((H, W, 4), dtype=torch.float16, device=dev), clear_color=api.Color(*CLEAR))
    torch.cuda.synchronize()
    assert same_bits(r.read_geometry(), geo)
    assert np.array_equal(u8.cpu().numpy(), img)
    enc = encode(f16.cpu().numpy().view(np.uint16)).reshape(H, W, 4)
    _near(enc, img, 1, "encoded f16 vs u8")
    _near(enc, want, 1, "encoded f16 vs oracle")
    r._ctx.close()


@pytest.mark.parametrize("layout", ["exchange", "bands"])
def test_two_emulated_devices(layout):
    api = _api()
    geo, img = base_route(False)
    for resident in (False, True):
        r = api.Renderer(devices=[0, 0], resident_geometry=resident)
        r._ctx.set_layout(layout)
        got = _render_host(r, SC.scene_composition(api, SC.api_scene(False)))
        assert same_bits(r.read_geometry(), geo), (layout, resident)
        assert np.array_equal(got, img), (layout, resident)
        _near(got, oracle_image(False), 1, "two devices vs oracle")
        r._ctx.close()


def test_pixel_aligned_shapes_give_their_exact_pixel_counts():
    api = _api()
    r = api.Renderer(0)
    for case, ink in SC.pixel_aligned():
        first, count, hw, limit, join, cap = case.strokes[0]
        pts = case.contours[0]
        closed = pts[0] == pts[-1]
        layer = ("stroke", [pts[:-1] if closed else pts], [closed], (2.0 * hw, join, cap, limit), (0.0, 0.0, 0.0, 1.0), "NonZero")
        img = _render_host(r, SC.scene_composition(api, [layer]), 64, 64)
        red = img[..., 0]
        assert set(np.unique(red)) <= {0, 255} and int((red == 0).sum()) == ink, (case.name, int((red == 0).sum()))
        assert np.array_equal(img[..., 3], np.full((64, 64), 255, np.uint8))
    r._ctx.close()


SVG = """<svg xmlns="http://www.w3.org/2000/svg" width="128" height="128">
<path d="M20 20 L100 14 L112 60 L70 100 L18 80 Z" fill="#d33" stroke="#118" stroke-width="5" stroke-linejoin="miter"/>
<g transform="matrix(0 1 -1 0 128 0)">
<path d="M12 10 L40 30 L60 8 L90 36" fill="none" stroke="#173" stroke-width="6" stroke-linecap="round" stroke-linejoin="round" stroke-opacity="0.6"/>
</g>
<path d="M8 104 l30 8 l-10 10 l50 -4" fill="none" stroke="black" stroke-width="3" stroke-linejoin="bevel" stroke-linecap="square"/>
<path d="M100 100 L120 100 L120 120 Z" fill="#00f"/>
</svg>"""


def test_svg_with_strokes_renders_like_the_models_pieces():
    from forma_amd import svg
    api = _api()
    doc = svg.load(SVG, is_text=True, strokes=True)
    assert len(doc.paths) == 5 and sorted(doc.strokes) == [1, 2, 3]
    r = api.Renderer(0)
    comp = api.Composition()
    for k, (path, rule, fill, blend) in enumerate(doc.paths):
        comp.get_mut_or_insert_default(api.Order(k)).insert(path).set_props(api.Props(fill_rule=rule, func=api.Func.Draw(api.Style(fill=fill, blend_mode=blend))))
    got = _render_host(r, comp)
    r._ctx.close()
    lin = lambda rgb: tuple(float(v) for v in (svg.to_linear(rgb).r, svg.to_linear(rgb).g, svg.to_linear(rgb).b))
    pent = [(20.0, 20.0), (100.0, 14.0), (112.0, 60.0), (70.0, 100.0), (18.0, 80.0)]
    zig = [(128.0 - y, x) for x, y in [(12.0, 10.0), (40.0, 30.0), (60.0, 8.0), (90.0, 36.0)]]      # matrix(0 1 -1 0 128 0): (x, y) -> (128 - y, x)
    rel = [(8.0, 104.0), (38.0, 112.0), (28.0, 122.0), (78.0, 118.0)]
    layers = [("fill", [pent], [True], None, lin((0xDD, 0x33, 0x33)) + (1.0,), "NonZero"),
              ("stroke", [pent], [True], (5.0, SM.MITER, SM.BUTT, 4.0), lin((0x11, 0x11, 0x88)) + (1.0,), "NonZero"),
              ("stroke", [zig], [False], (6.0, SM.ROUND, SM.ROUND_CAP, 4.0), lin((0x11, 0x77, 0x33)) + (0.6,), "NonZero"),
              ("stroke", [rel], [False], (3.0, SM.BEVEL, SM.SQUARE, 4.0), (0.0, 0.0, 0.0, 1.0), "NonZero"),
              ("fill", [[(100.0, 100.0), (120.0, 100.0), (120.0, 120.0)]], [True], None, lin((0, 0, 255)) + (1.0,), "NonZero")]
    _near(got, SC.ref_render(SC.scene_model(layers), W, H), 1, "svg strokes vs oracle")
