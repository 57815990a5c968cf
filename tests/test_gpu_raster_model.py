"""Every HIP route of stages 1 and 2 against raster_model.py, on the cases and with the bounds of test_raster_model.py, and bit for
bit against the oracle on each of them.

Stage 2: the staged-parameter route (`prepare_lines` + `rasterize_lines`), and the frame route (`render`, then the unsorted and the
sorted stream) on its synchronous first frame and on a read-back-free one, under the FORMA_HIP_DEBUG switches that change how
k_rasterize files its segments -- the rank switches also with `fuse_digit=2`, since the ranked partition only runs in a fused frame.
Stage 1: the product's PathBuilder through `Renderer._upload_geometry` (k_flatten) and through the resident store
(k_flatten_store, whose `/similarity` shapes carry a per-range affine).  The polygon images also run on the emulated three-device
context under both layouts: BANDS culls lines by tile-row band."""
import numpy as np
import pytest

import raster_cases as RC
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

STAGE2, SHAPES = RC.STAGE2, RC.SHAPES
CLEAR = (1.0, 1.0, 1.0, 1.0)
SWITCHES = ["", "no_ras_hist", "ras_rank=0", "ras_rank=2", "digit_bits=4", "fuse_digit=2,ras_rank=0", "fuse_digit=2,ras_rank=2"]
_oracle = {}


def oracle_streams(name):
    """(unsorted, sorted) of the oracle, once per scene"""
    if name not in _oracle:
        lines, w, h, _ = RC.stage2_scenes()[name]
        o = orc.Oracle()
        RC.load(o, RC.line_tables(lines))
        o.prepare_lines(w, h)
        _oracle[name] = (o.rasterize(), o.sort())
    return _oracle[name]


@pytest.fixture(scope="module")
def ctx():
    import forma_amd
    c = forma_amd.Context(0)
    yield c
    c.close()


# ---- stage 2, route 1: staged parameters -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", STAGE2)
def test_staged_route_against_model_and_oracle(ctx, name):
    lines, w, h, _ = RC.stage2_scenes()[name]
    RC.load(ctx, RC.line_tables(lines))
    got = ctx.rasterize_lines(ctx.prepare_lines(w, h))
    RC.check_stream(name, got, "staged")
    assert np.array_equal(got, oracle_streams(name)[0]), name


# ---- stage 2, route 2: the frame ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=SWITCHES)
def switched(request):
    """a context created under one value of FORMA_HIP_DEBUG (the library parses it when a context is created)"""
    import forma_amd
    mp = pytest.MonkeyPatch()
    mp.setenv("FORMA_HIP_DEBUG", request.param)
    c = forma_amd.Context(0)
    yield request.param, c
    c.close()
    mp.undo()


@pytest.mark.parametrize("name", STAGE2)
def test_frame_route_against_model_and_oracle(switched, name):
    switch, c = switched
    lines, w, h, _ = RC.stage2_scenes()[name]
    unsorted, want_sorted = oracle_streams(name)
    RC.load(c, RC.line_tables(lines))
    for frame in range(3):                                               # synchronous, then read-back-free
        c.render(w, h, clear=CLEAR, device_only=True)
        if frame == 1:
            continue
        who = "frame %d [%s]" % (frame, switch)
        s0, s1 = c.segments(0), c.segments(1)
        RC.check_stream(name, s0, who + " unsorted")
        RC.check_stream(name, s1, who + " sorted")
        assert np.array_equal(np.sort(s0), np.sort(unsorted)), (who, name)      # the same segments, whatever order the partition leaves
        assert np.array_equal(s1, want_sorted), (who, name)


# ---- polygons: one device and the emulated three ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["64x64", "72x40", "33x17"])
def test_polygon_images_and_areas(ctx, name):
    w, h, layers = RC.polygon_scenes()[name]
    t = RC.polygon_tables(layers)
    o = orc.Oracle()
    RC.load(o, t); RC.load(ctx, t)
    want = o.render(w, h, clear=CLEAR)
    for frame in range(2):
        got = ctx.render(w, h, clear=CLEAR)
        RC.check_polygons(name, got, ctx.segments(1), "frame %d" % frame)
        assert np.array_equal(ctx.segments(1), o.segments(1)) and np.array_equal(got, want), (name, frame)


@pytest.mark.parametrize("layout", ["exchange", "bands"])
def test_polygon_images_on_three_devices(layout):
    import forma_amd
    c = forma_amd.Context(devices=[0, 0, 0], layout=layout)
    try:
        for name, (w, h, layers) in RC.polygon_scenes().items():
            t = RC.polygon_tables(layers)
            o = orc.Oracle()
            RC.load(o, t); RC.load(c, t)
            want = o.render(w, h, clear=CLEAR)
            for frame in range(2):
                got = c.render(w, h, clear=CLEAR)
                RC.check_polygons(name, got, None, "%s frame %d" % (layout, frame))
                assert np.array_equal(got, want), (layout, name, frame)
    finally:
        c.close()


# ---- stage 1 ---------------------------------------------------------------------------------------------------------------------
def _stage1_cases():
    out = [("%s/%g" % (kind, scale), i, c, None) for kind in RC.CURVE_KINDS for scale in RC.CURVE_SCALES
           for i, c in enumerate(RC.curve_family(kind, scale))]
    shapes = RC.edge_shapes()
    return out + [(name, 0, shapes[name][0], shapes[name][1]) for name in SHAPES]


@pytest.fixture(scope="module")
def flattened():
    """route -> [(x, y)] per case, and the oracle's: every case is one layer's one path; one upload per route"""
    from forma_amd import api
    cases = _stage1_cases()
    o = orc.Oracle()
    want = [o.flatten(RC.oracle_path(cmds, t9))[:2] for _, _, cmds, t9 in cases]
    ends = np.cumsum([len(x) for x, _ in want])
    out = {"oracle": want}
    for route in ("upload", "resident"):
        comp = api.Composition()
        for i, (_, _, cmds, t9) in enumerate(cases):
            comp.get_mut_or_insert_default(api.Order(i)).insert(RC.product_path(cmds, t9))
        r = api.Renderer(0, resident_geometry=route == "resident")
        try:
            if route == "upload":
                r._upload_geometry(comp)
                x, y = r.host_tables["x"], r.host_tables["y"]
            else:
                r._upload_resident(comp)
                x, y, _ = r.read_geometry()
        finally:
            r._ctx.close()
        assert len(x) == ends[-1], (route, len(x), int(ends[-1]))
        out[route] = [(x[a:b], y[a:b]) for a, b in zip(np.concatenate([[0], ends[:-1]]), ends)]
    return cases, out


@pytest.mark.parametrize("route", ["upload", "resident"])
def test_flattened_points_are_the_oracles_bit_for_bit(flattened, route):
    cases, out = flattened
    for (name, i, _, _), (x, y), (wx, wy) in zip(cases, out[route], out["oracle"]):
        assert np.array_equal(x.view(np.uint32), wx.view(np.uint32)) and np.array_equal(y.view(np.uint32), wy.view(np.uint32)), (route, name, i)


@pytest.mark.parametrize("route", ["upload", "resident"])
@pytest.mark.parametrize("scale", RC.CURVE_SCALES)
@pytest.mark.parametrize("kind", RC.CURVE_KINDS)
def test_flattened_families_against_their_curves(flattened, kind, scale, route):
    cases, out = flattened
    fam = "%s/%g" % (kind, scale)
    ms = [RC.curve_measures(cmds, t9, x, y) for (name, _, cmds, t9), (x, y) in zip(cases, out[route]) if name == fam]
    assert len(ms) == RC.CURVES_PER_FAMILY
    RC.check_measures(fam, RC.worst_of(ms), RC.bounds()["stage1"]["families"][fam], on_curve=kind in RC.ON_CURVE, who=route)


@pytest.mark.parametrize("route", ["upload", "resident"])
@pytest.mark.parametrize("name", SHAPES)
def test_flattened_edge_shapes_against_their_curves(flattened, name, route):
    cases, out = flattened
    (_, _, cmds, t9), (x, y) = next((c, p) for c, p in zip(cases, out[route]) if c[0] == name)
    RC.check_measures(name, RC.curve_measures(cmds, t9, x, y), RC.bounds()["stage1"]["edge_shapes"][name],
                      only_c=name == "doubled_back_quad", who=route)
