"""The sort's first digit pass fused into the rasterizer (csrc/sort.hip, SliceSrc), forced on and off.

`FORMA_HIP_DEBUG=fuse_digit=2` fuses the pass on every read-back-free frame whose plan allows it, `fuse_digit=0` never does.
Both must give the same images, the same sorted segment stream and (put back in stream order for the caller) the same unsorted
stream.  Every case also checks, from the kernels of a timed read-back-free frame, whether the fused path ran (`k_slice_scan`,
one `k_onesweep` per pass after the first) and how many passes the plan had, so that each case provably reaches what it names:
two-pass plans at 720p, 1080p and 4K; a three-pass plan whose fused pass is not the last one (layers out of paint order); a
biased plan (tile fields relative to their minima, 8-bit digits on an 8192^2 canvas); a frame that leaves the span the biased
plan was speculated for (void, rendered again synchronously); more than 8 192 blocks per digit (the slice scan's rounds); three
frame slots; and the plans that keep the plain first pass (a 512-bin first digit)."""
import numpy as np
import pytest

from forma_amd import api, scenes

pytestmark = pytest.mark.gpu

CLEAR = (1.0, 1.0, 1.0, 1.0)


def _kernels(ctx, w, h):
    """one timed read-back-free frame: (kernel names, timings)"""
    _img, tm = ctx.render(w, h, clear=CLEAR, timings=True)
    return [k[0] for k in ctx.kernel_times()], tm


def _frames(monkeypatch, switch, comp, w, h, frames=4, slots=1):
    monkeypatch.setenv("FORMA_HIP_DEBUG", switch)
    image = np.zeros((h, w * 4), np.uint8)
    r = api.Renderer(device=0)
    try:
        r.render(comp, api.BufferBuilder(image.reshape(-1), api.LinearLayout(w, w * 4, h)).build(), api.RGBA,
                 api.Color(*CLEAR), None)
        ctx = r._ctx
        out = [image.copy()]
        for _ in range(frames):                              # frame 0 was synchronous; these are read-back-free
            out.append(ctx.render(w, h, clear=CLEAR).copy())
        if slots > 1:
            ctx.set_frames_in_flight(slots)
            for _ in range(3 * slots):
                ctx.render(w, h, clear=CLEAR, device_only=True)
            out.append(ctx.read_image(w, h).copy())
            sorted_slots = ctx.segments(1).copy()
            ctx.set_frames_in_flight(1)
            for _ in range(2):
                ctx.render(w, h, clear=CLEAR)
        names, tm = _kernels(ctx, w, h)
        out.append(ctx.render(w, h, clear=CLEAR).copy())
        streams = [ctx.segments(0).copy(), ctx.segments(1).copy()] + ([sorted_slots] if slots > 1 else [])
        return out, streams, names, tm
    finally:
        r._ctx.close()


def _same_both_ways(monkeypatch, comp, w, h, fused=True, passes=None, extra="", **kw):
    off = _frames(monkeypatch, "fuse_digit=0" + extra, comp, w, h, **kw)
    on = _frames(monkeypatch, "fuse_digit=2" + extra, comp, w, h, **kw)
    assert "k_slice_scan" not in off[2]
    assert ("k_slice_scan" in on[2]) == fused, on[2]
    n_pass = int(on[3]["n_sort_passes"])
    assert off[2].count("k_onesweep") == n_pass
    assert on[2].count("k_onesweep") == n_pass - (1 if fused else 0)
    if passes is not None:
        assert n_pass == passes, n_pass
    for k, (a, b) in enumerate(zip(off[0], on[0])):
        assert np.array_equal(a, b), ("image", k)
    for k, (a, b) in enumerate(zip(off[1], on[1])):
        assert np.array_equal(a, b), ("stream", k)        # unsorted, sorted (and sorted with three slots)
    return on


def _triangles(n, x0, x1, y0, y1, seed, orders=None):
    comp = api.Composition()
    rng = np.random.default_rng(seed)
    for i in range(n):
        order = int(orders[i]) if orders is not None else i
        x, y = float(rng.uniform(x0, x1)), float(rng.uniform(y0, y1))
        s = float(rng.uniform(8, 120))
        comp.get_mut_or_insert_default(order).insert(
            api.PathBuilder().move_to(api.Point(x, y)).line_to(api.Point(x + s, y + s / 3))
            .line_to(api.Point(x + s / 2, y + s)).build()).set_props(scenes._solid(api.Color(0.2, 0.4, (i % 7) / 7.0, 0.7)))
    return comp


@pytest.mark.parametrize("n_layers,w,h", [(3000, 1920, 1080), (30000, 3840, 2160)])
def test_headline_stand_in(monkeypatch, n_layers, w, h):
    _same_both_ways(monkeypatch, scenes.paris_like(n_layers=n_layers, width=w, height=h), w, h, passes=2)


def test_headline_stand_in_three_frame_slots(monkeypatch):
    _same_both_ways(monkeypatch, scenes.paris_like(n_layers=8000, width=3840, height=2160), 3840, 2160, passes=2, slots=3)


def test_more_than_8192_blocks_per_digit(monkeypatch):
    """N > 8 192 x 2 048: k_slice_scan reads a digit's row of the slice table in more than one round."""
    on = _same_both_ways(monkeypatch, scenes.paris_like(n_layers=42000, width=3840, height=2160), 3840, 2160, passes=2)
    assert on[3]["n_segments"] > 8192 * 2048, on[3]["n_segments"]


@pytest.mark.parametrize("w,h", [(1920, 1080), (1280, 720)])
def test_random_cubics(monkeypatch, w, h):
    _same_both_ways(monkeypatch, scenes.random_cubics(n=400, width=w, height=h, seed=71), w, h, passes=2)


def test_8192_canvas_with_8_bit_digits(monkeypatch):
    """10 + 10 live tile bits in 8-bit digits: three passes, the first of them fused."""
    _same_both_ways(monkeypatch, scenes.random_cubics(n=400, width=8192, height=8192, seed=71), 8192, 8192, passes=3,
                    extra=",digit_bits=8")


@pytest.mark.parametrize("w,h", [(8192, 8192), (4096, 2048)])
def test_plans_with_a_512_bin_first_digit_keep_the_plain_pass(monkeypatch, w, h):
    _same_both_ways(monkeypatch, scenes.random_cubics(n=400, width=w, height=h, seed=71), w, h, fused=False)


def test_layers_out_of_paint_order(monkeypatch):
    """256 layers inserted against paint order at 4K: a layer digit, then tile_x, then tile_y — the fused pass is the first of
    three, and the pass that reads the slices is followed by a plain one."""
    rng = np.random.default_rng(5)
    comp = _triangles(256, 0, 3700, 0, 2000, seed=6, orders=rng.permutation(256))
    _same_both_ways(monkeypatch, comp, 3840, 2160, passes=3)


def test_biased_plan(monkeypatch):
    """Geometry in a 1 000-pixel square around (4 000, 4 000) of an 8192^2 canvas, 8-bit digits: tile + 1 crosses 256, so plain
    digits need 9 + 9 bits (three passes); relative to the fields' minima two passes remain, the first one fused."""
    _same_both_ways(monkeypatch, _triangles(500, 3600, 4500, 3600, 4500, seed=8), 8192, 8192, passes=2, extra=",digit_bits=8")


def test_a_fused_frame_that_leaves_its_planned_span_is_rendered_again(monkeypatch):
    """The biased scene, then every layer moved 1 500 pixels right by a transform (no new geometry, so the next frame is
    read-back-free with the plan speculated from the old span): the fused frame is void and rendered again synchronously."""
    res = {}
    for switch in ("fuse_digit=0,digit_bits=8", "fuse_digit=2,digit_bits=8"):
        monkeypatch.setenv("FORMA_HIP_DEBUG", switch)
        comp = _triangles(500, 3600, 4500, 3600, 4500, seed=8)
        image = np.zeros((8192, 8192 * 4), np.uint8)
        r = api.Renderer(device=0)
        try:
            buf = api.BufferBuilder(image.reshape(-1), api.LinearLayout(8192, 8192 * 4, 8192)).build()
            out = []
            for k in range(5):
                r.render(comp, buf, api.RGBA, api.Color(*CLEAR), None)
                out.append(image.copy())
            names_before = [k[0] for k in (r._ctx.render(8192, 8192, clear=CLEAR, timings=True), r._ctx.kernel_times())[1]]
            for layer in comp.layers.values():
                layer.set_transform(api.GeomPresTransform.try_from([1.0, 0.0, 0.0, 1.0, 1500.0, 0.0]))
            for k in range(3):                                   # the first: void, rendered again synchronously
                r.render(comp, buf, api.RGBA, api.Color(*CLEAR), None)
                out.append(image.copy())
            # a biased plan that met a void frame is banned for a while (ban_bias): the plain three-pass plan proves the void
            _img, tm = r._ctx.render(8192, 8192, clear=CLEAR, timings=True)
            res[switch] = (out, r._ctx.segments(1).copy(), names_before, int(tm["n_sort_passes"]))
        finally:
            r._ctx.close()
    a, b = res["fuse_digit=0,digit_bits=8"], res["fuse_digit=2,digit_bits=8"]
    assert "k_slice_scan" not in a[2] and "k_slice_scan" in b[2], b[2]
    assert a[3] == 3 and b[3] == 3, (a[3], b[3])
    for k, (x, y) in enumerate(zip(a[0], b[0])):
        assert np.array_equal(x, y), ("frame", k)
    assert np.array_equal(a[1], b[1])
