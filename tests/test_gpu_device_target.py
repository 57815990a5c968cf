"""Frames painted straight into caller DEVICE memory (forma_hip_render_device, Renderer.render_to_device): the GPU backend's
`render_to_texture` (reference gpu/renderer/mod.rs:462-520).  SRGB8 targets hold exactly the bytes forma_hip_render writes into
host memory; LINEAR_F16 targets hold the painter's linear colour as binary16 (gpu/painter/paint.wgsl:954) — checked bit for bit
on scenes whose halves are known by hand, and through a host-side sRGB encode against the u8 path everywhere else."""
import os

import numpy as np
import pytest

import scene as S
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

CLEAR = (0.9, 0.95, 1.0, 1.0)
ORDERS = [(0, 1, 2, 3), (2, 1, 0, 3), (0, 1, 2, 4), (2, 1, 0, 4), (0, 1, 2, 5), (2, 1, 0, 5)]   # RGBA BGRA RGB0 BGR0 RGB1 BGR1
GOLD = np.load(os.path.join(os.path.dirname(__file__), "golden", "e2e_cpu_64x64.npz"))
E_ARG, E_STATE = -1, -5


def _torch():
    import torch
    return torch


def _dev():
    torch = _torch()
    return torch.device("cuda", 0)


def _target(w, h, fmt, fill=0):
    torch = _torch()
    return torch.full((h, w, 4), fill, dtype=torch.uint8 if fmt == "srgb8" else torch.float16, device=_dev())


def dev_render(c, w, h, fmt="srgb8", out=None, **kw):
    """one frame into a fresh (or the given) device tensor; returns the tensor"""
    torch = _torch()
    out = _target(w, h, fmt) if out is None else out
    c.render_device(out.data_ptr(), fmt, w, h, out.stride(0) * out.element_size(),
                    wait_stream=torch.cuda.current_stream(_dev()).cuda_stream, **kw)
    return out


def host_of(t):
    """device tensor -> numpy (u8: [H, W * 4]; f16: the raw binary16 bits [H, W, 4])"""
    torch = _torch()
    torch.cuda.synchronize()
    a = t.cpu().numpy()
    return a.reshape(a.shape[0], -1) if a.dtype == np.uint8 else a.view(np.uint16)


def encode(f16_bits):
    """numpy restatement of the painters' encode (paint.hip linear_to_srgb / to_u8_x4 / to_u8_x8): bytes 0..2 sRGB, byte 3 linear"""
    v = f16_bits.view(np.float16).astype(np.float64)
    s = np.sqrt(np.maximum(v, 0.0))
    n = 0.20101772 * v * s + (-0.51280147 * v + (1.344401 * s - 0.030656587))
    srgb = np.where(v <= 0.0031308, v * 12.92, n)
    out = np.where(np.arange(4) < 3, srgb, v)
    return np.rint(np.clip(out * 255.0, 0.0, 255.0)).astype(np.uint8).reshape(v.shape[0], -1)


def near(a, b, tol, what):
    d = np.abs(a.astype(int) - b.astype(int))
    assert d.max() <= tol, (what, int(d.max()), int((d > tol).sum()))


@pytest.fixture(scope="module")
def ctx():
    import forma_amd
    c = forma_amd.Context(0)
    yield c
    c.close()


def _scenes():
    out = [(n, c, 64, 64) for n, c in S.e2e_scenes().items()]
    out.append(("mixed", S.random_mixed(n=200, width=1000, height=563, seed=71), 1000, 563))
    out.append(("translucent-cubics", S.random_cubics(n=120, width=1000, height=563, seed=72, alpha=0.55), 1000, 563))
    return out


@pytest.fixture(scope="module")
def scenes():
    o = orc.Oracle()
    return [(n, comp.tables(o), w, h) for n, comp, w, h in _scenes()]


# 1 + 5 ----------------------------------------------------------------------------------------------------------------
def test_srgb8_parity_and_linear_f16_against_the_u8_path(ctx, scenes):
    o = orc.Oracle()
    for name, t, w, h in scenes:
        S.load(o, t); S.load(ctx, t)
        crop = (16 * 3 + 5, w - 37, 16 * 2 + 9, h - 21) if w > 64 else (5, 59, 9, 43)
        for ch in ORDERS if w > 64 or name in ("linear_gradient", "clipping") else ORDERS[:1]:
            for cr in (None, crop):
                for frame in range(2):                              # a synchronous frame, then a read-back-free one
                    host = ctx.render(w, h, channels=ch, clear=CLEAR, crop=cr)   # (zeroed like the tensor outside the crop)
                    got = host_of(dev_render(ctx, w, h, channels=ch, clear=CLEAR, crop=cr))
                    assert np.array_equal(got, host), (name, ch, cr, frame, "SRGB8 device frame != host frame")
                    lin = host_of(dev_render(ctx, w, h, fmt="linear_f16", channels=ch, clear=CLEAR, crop=cr))
                    near(encode(lin), host, 1, (name, ch, cr, frame, "encoded f16 vs u8"))
                near(got, o.render(w, h, channels=ch, clear=CLEAR, crop=cr), 1, (name, ch, cr, "oracle"))
        if name in GOLD.files:                                      # reference PNG goldens: clear (1, 1, 1, 0), RGBA
            lin = host_of(dev_render(ctx, w, h, fmt="linear_f16"))
            near(encode(lin).reshape(h, w, 4), GOLD[name], 8, (name, "golden"))   # e2e-tests/tests/test_env.rs:278


# 2 --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["srgb8", "linear_f16"])
def test_strided_offset_target_keeps_every_other_byte(ctx, scenes, fmt):
    torch = _torch()
    name, t, w, h = [s for s in scenes if s[0] == "mixed"][0]
    S.load(ctx, t)
    sent = 77
    for crop in (None, (16 * 3 + 5, w - 37, 16 * 2 + 9, h - 21)):
        big = _target(w + 37, h + 3, fmt, fill=sent)
        view = big[1:1 + h, 5:5 + w, :]
        ref = host_of(dev_render(ctx, w, h, fmt=fmt, clear=CLEAR, crop=crop))
        dev_render(ctx, w, h, fmt=fmt, out=view, clear=CLEAR, crop=crop)
        torch.cuda.synchronize()
        b = big.cpu().numpy()
        b = b if b.dtype == np.uint8 else b.view(np.uint16)
        sv = np.array(sent, b.dtype) if fmt == "srgb8" else np.array(sent, np.float16).view(np.uint16)
        inside = np.zeros(b.shape[:2], bool)
        x0, x1, y0, y1 = (0, w, 0, h) if crop is None else ((crop[0] // 16) * 16, min(-(-crop[1] // 16) * 16, w),
                                                           (crop[2] // 16) * 16, min(-(-crop[3] // 16) * 16, h))
        inside[1 + y0:1 + y1, 5 + x0:5 + x1] = True
        assert (b[~inside] == sv).all(), (fmt, crop, "bytes outside the written crop changed")
        got = b[1:1 + h, 5:5 + w].reshape(h, -1) if fmt == "srgb8" else b[1:1 + h, 5:5 + w]
        bpx = 4 if fmt == "srgb8" else 1                            # (u8 rows are bytes, f16 rows are pixels)
        sub = (slice(y0, y1), slice(x0 * bpx, x1 * bpx))
        assert np.array_equal(got[sub], ref[sub]), (fmt, crop)


# 3 --------------------------------------------------------------------------------------------------------------------
def test_a_device_frame_launches_the_kernels_of_a_device_resident_frame(scenes):
    import forma_amd
    name, t, w, h = [s for s in scenes if s[0] == "mixed"][0]
    lists = {}
    for how in ("null", "srgb8", "linear_f16"):
        c = forma_amd.Context(0)
        try:
            S.load(c, t)
            seq = []
            for frame in range(3):
                if how == "null":
                    c.render(w, h, clear=CLEAR, device_only=True, timings=True)
                else:
                    dev_render(c, w, h, fmt=how, clear=CLEAR, timings=True)
                seq.append([k[0] for k in c.kernel_times()])
            lists[how] = seq
        finally:
            c.close()
    assert all(len(s) > 3 for s in lists["null"])
    assert lists["srgb8"] == lists["null"]
    assert lists["linear_f16"] == lists["null"]


# 4 --------------------------------------------------------------------------------------------------------------------
def _blend(d, f, sa):                                               # blend_at with BlendMode::Over, f32 like the painter
    d = np.asarray(d, np.float32); f = np.asarray(f, np.float32); sa = np.float32(sa)
    da = d[3]
    k1, isa, k2 = (np.float32(1) - da) * sa, np.float32(1) - sa, da * sa
    rgb = d[:3] * isa + (f[:3] * k1 + f[:3] * k2)
    return np.concatenate([rgb, [da * isa + sa]]).astype(np.float32)


@pytest.mark.parametrize("clear", [(0.5, 0.25, 1.0, 1.0), (0.75, 0.5, 0.25, 0.5)])
def test_linear_f16_exact_halves(ctx, clear):
    w, h = 64, 48
    sq = (8.0, 8.0, 40.0, 40.0)                                     # pixel-aligned edges: coverage is exactly 0 or 1
    for colour in ((0.25, 0.5, 0.75, 1.0), (0.75, 0.25, 0.5, 0.5)):
        comp = S.Composition()
        comp.get_mut_or_insert_default(0).insert(S.custom_square(-4.0, 16.0, 72.0, 32.0)).set_props(S.solid((0.5, 0.75, 0.25, 0.5)))
        comp.get_mut_or_insert_default(1).insert(S.custom_square(*sq)).set_props(S.solid(colour))
        S.load(ctx, comp.tables(orc.Oracle()))
        cl = np.asarray(clear, np.float32)
        band = _blend(cl, (0.5, 0.75, 0.25, 0.5), 0.5)
        img = np.tile(cl, (h, w, 1))
        img[16:32, :] = band                                        # the full-width band (solid tiles and painted ones)
        ys, xs = slice(8, 40), slice(8, 40)
        img[ys, xs] = _blend(img[ys, xs][0, 0], colour, colour[3]) if colour[3] < 1 else np.asarray(colour, np.float32)
        img[16:32, 8:40] = _blend(band, colour, colour[3]) if colour[3] < 1 else np.asarray(colour, np.float32)
        for ch in ((0, 1, 2, 3), (2, 1, 0, 4), (0, 1, 2, 5), (3, 4, 5, 0), (4, 3, 1, 5)):
            eff = [5 if (c == 3 and clear[3] == 1.0) else c for c in ch]   # renderer.rs:85-92
            sel = np.stack([img[..., c] if c < 4 else np.full((h, w), 0.0 if c == 4 else 1.0, np.float32) for c in eff], -1)
            want = sel.astype(np.float16).view(np.uint16)
            for frame in range(2):
                got = host_of(dev_render(ctx, w, h, fmt="linear_f16", channels=ch, clear=clear))
                assert np.array_equal(got, want), (colour, ch, clear, frame, np.argwhere(got != want)[:4])


# 6 --------------------------------------------------------------------------------------------------------------------
SWITCHES = ["", "strip_tiles=100000000", "strip_tiles=0", "paint_quad=2", "paint_quad=0", "force_cull", "no_cull", "order_thr=1"]


def _frames_under(monkeypatch, switch, t, w, h):
    import forma_amd
    monkeypatch.setenv("FORMA_HIP_DEBUG", switch)
    c = forma_amd.Context(0)
    try:
        S.load(c, t)
        f16, u8 = [], []
        for frame in range(3):
            host = c.render(w, h, clear=CLEAR)
            dev = host_of(dev_render(c, w, h, clear=CLEAR))
            assert np.array_equal(dev, host), (switch, frame)
            f16.append(host_of(dev_render(c, w, h, fmt="linear_f16", clear=CLEAR)))
            u8.append(host)
        return f16, u8
    finally:
        c.close()


def test_every_painter_writes_f16(monkeypatch, scenes):
    o = orc.Oracle()
    fams = [("opaque-cubics", S.random_cubics(n=300, width=1000, height=563, seed=73).tables(o), 1000, 563),
            ("translucent-cubics", [s for s in scenes if s[0] == "translucent-cubics"][0][1], 1000, 563),
            ("mixed", [s for s in scenes if s[0] == "mixed"][0][1], 1000, 563)]
    for name, t, w, h in fams:
        base = None
        for sw in SWITCHES:
            f16, u8 = _frames_under(monkeypatch, sw, t, w, h)
            for k in range(3):
                near(encode(f16[k]), u8[k], 1, (name, sw, k))
                assert np.array_equal(f16[k], f16[0]), (name, sw, k)
            if base is None:
                base = f16[0]
            assert np.array_equal(f16[0], base), (name, sw, "f16 differs from the default schedule")


@pytest.mark.parametrize("layers", [120, 1100, 4200])
def test_f16_through_the_deep_painters(layers):
    import forma_amd
    rng = np.random.default_rng(1000 + layers)
    comp = S.Composition()
    for order in range(layers):                                    # the scene of test_every_tier_of_the_deep_painters
        x1 = 16.0 + float(rng.uniform(0, 112)) * (order % 3 != 0)
        comp.get_mut_or_insert_default(order).insert(S.custom_square(1.0, 1.0 + float(rng.uniform(0, 6)), x1, 15.0)).set_props(
            S.solid((float(rng.random()), float(rng.random()), float(rng.random()), 0.03)))
    t = comp.tables(orc.Oracle())
    c = forma_amd.Context(0)
    try:
        S.load(c, t)
        first = None
        for frame in range(3):
            host = c.render(160, 32)
            assert np.array_equal(host_of(dev_render(c, 160, 32)), host), (layers, frame)
            lin = host_of(dev_render(c, 160, 32, fmt="linear_f16"))
            near(encode(lin), host, 1, (layers, frame))
            first = lin if first is None else first
            assert np.array_equal(lin, first), (layers, frame)
    finally:
        c.close()


# 7 --------------------------------------------------------------------------------------------------------------------
def test_frames_in_flight_fill_their_own_targets():
    """Three frame slots, u8 and f16 frames into four rotating tensors each; the clear colour differs per frame, and after a few
    frames the layers' transform triples the geometry (set_geoms keeps the predictions: the next read-back-free frame on every
    slot is void and re-run into its target when it is settled)."""
    import forma_amd
    torch = _torch()
    o = orc.Oracle()
    w, h = 640, 360
    t = S.random_cubics(n=150, width=w // 3, height=h // 3, seed=74, alpha=0.7).tables(o)
    big = t["geoms"].copy()
    big["flags"] = 1
    big["xf"] = (3.0, 0.0, 0.0, 3.0, 0.0, 0.0)
    ref = forma_amd.Context(0)
    c = forma_amd.Context(0, frames_in_flight=3)
    try:
        S.load(ref, t); S.load(c, t)
        outs = {f: [_target(w, h, f) for _ in range(4)] for f in ("srgb8", "linear_f16")}
        want = {f: [None] * 4 for f in outs}
        k = 0
        for step in range(14):
            if step == 8:
                c.set_geoms(big); ref.set_geoms(big)
            clear = (0.1 * (step % 7), 0.5, 1.0 - 0.05 * step, 1.0)
            for f in ("srgb8", "linear_f16"):
                i = k % 4
                dev_render(c, w, h, fmt=f, out=outs[f][i], clear=clear)
                want[f][i] = host_of(dev_render(ref, w, h, fmt=f, clear=clear))
            k += 1
        c.sync()
        torch.cuda.synchronize()
        for f in outs:
            for i in range(4):
                assert np.array_equal(host_of(outs[f][i]), want[f][i]), (f, i)
    finally:
        c.close(); ref.close()


# 8 --------------------------------------------------------------------------------------------------------------------
def _ship_frames(n_frames, w, h, device):
    import forma_amd
    from forma_amd import api, spaceship
    r = api.Renderer(0)
    comp = api.Composition()
    ship = spaceship.Spaceship(api, width=w, height=h, seed=43)
    cache = r.create_buffer_layer_cache()
    torch = _torch()
    out = torch.zeros((h, w, 4), dtype=torch.uint8, device=_dev()) if device else np.zeros((h, w * 4), np.uint8)
    frames = []
    for f in range(n_frames):
        ship.compose(comp)
        if device:
            r.render_to_device(comp, out, clear_color=api.Color(0.1, 0.1, 0.2, 1.0), layer_cache=cache)
            frames.append(host_of(out))
        else:
            r.render(comp, api.BufferBuilder(out, api.LinearLayout(w, w * 4, h)).layer_cache(cache).build(),
                     clear_color=api.Color(0.1, 0.1, 0.2, 1.0))
            frames.append(out.copy())
    return frames, r, cache, out


def test_cache_spaceship_device_equals_host():
    w, h = 640, 360
    host, *_ = _ship_frames(30, w, h, device=False)
    dev, *_ = _ship_frames(30, w, h, device=True)
    for f in range(30):
        assert np.array_equal(dev[f], host[f]), f


def test_cache_skipped_tiles_keep_the_target_and_switching_targets_repaints(ctx, scenes):
    torch = _torch()
    name, t, w, h = [s for s in scenes if s[0] == "mixed"][0]
    t = dict(t); t["unchanged"] = np.ones_like(t["unchanged"])
    S.load(ctx, t)
    ctx.cache_clear(3)
    out = _target(w, h, "srgb8")
    dev_render(ctx, w, h, out=out, clear=CLEAR, cache_id=3)
    first = host_of(out).copy()
    flags = ctx.tiles_written(w, h)
    assert flags.all()
    out[0:16, 0:16] = 201                                           # poke tile (0, 0); nothing changed: the cache skips every tile
    dev_render(ctx, w, h, out=out, clear=CLEAR, cache_id=3)
    assert not ctx.tiles_written(w, h).any()
    got = host_of(out)
    assert (got[0:16, 0:64] == 201).all()
    assert np.array_equal(got[16:], first[16:])
    # host buffer with the same cache: a new target -> everything repainted, like a fresh cache
    host = ctx.render(w, h, clear=CLEAR, cache_id=3)
    assert ctx.tiles_written(w, h).all()
    ctx.cache_clear(4)
    assert np.array_equal(host, ctx.render(w, h, clear=CLEAR, cache_id=4))
    # ... and back to a device target (another tensor): repainted again
    out2 = _target(w, h, "srgb8", fill=9)
    dev_render(ctx, w, h, out=out2, clear=CLEAR, cache_id=3)
    assert ctx.tiles_written(w, h).all()
    assert np.array_equal(host_of(out2), host)


# 9 --------------------------------------------------------------------------------------------------------------------
def test_wait_stream_orders_the_frame_after_torch_work(scenes):
    torch = _torch()
    from forma_amd import api
    r = api.Renderer(0)
    comp = api.Composition()
    pb = api.PathBuilder()
    pb.move_to(api.Point(-10, -10)); pb.line_to(api.Point(300, -10)); pb.line_to(api.Point(300, 300)); pb.line_to(api.Point(-10, 300))
    comp.get_mut_or_insert_default(api.Order(0)).insert(pb.build()).set_props(
        api.Props(func=api.Func.Draw(api.Style(fill=api.Fill.Solid(api.Color(0.25, 0.5, 0.75, 1.0))))))
    w, h = 256, 192
    ref = r.render_to_device(comp, torch.zeros((h, w, 4), dtype=torch.uint8, device=_dev()))
    torch.cuda.synchronize()
    want = ref.cpu().numpy()
    assert not (want == 7).any()
    out = torch.zeros((h, w, 4), dtype=torch.uint8, device=_dev())
    torch.cuda.synchronize()
    torch.cuda._sleep(50_000_000)                                    # tens of milliseconds on torch's current stream ...
    out.fill_(7)                                                     # ... then a write the frame must come after
    r.render_to_device(comp, out)
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), want)


# 10 -------------------------------------------------------------------------------------------------------------------
def test_errors(ctx, scenes):
    import forma_amd
    from forma_amd import api
    from forma_amd._lib import FormaError
    torch = _torch()
    name, t, w, h = [s for s in scenes if s[0] == "mixed"][0]
    S.load(ctx, t)

    def code(fn):
        with pytest.raises(FormaError) as e:
            fn()
        return e.value.code

    host = np.zeros((h, w * 8), np.uint8)
    assert code(lambda: ctx.render_device(host.ctypes.data, "srgb8", w, h, w * 4)) == E_ARG
    pinned = torch.zeros((h, w, 4), dtype=torch.uint8).pin_memory()
    assert code(lambda: ctx.render_device(pinned.data_ptr(), "srgb8", w, h, w * 4)) == E_ARG
    out = _target(w + 8, h, "linear_f16")
    assert code(lambda: ctx.render_device(out.data_ptr(), "linear_f16", w, h, w * 8, cache_id=0)) == E_ARG
    assert code(lambda: ctx.render_device(out.data_ptr(), "linear_f16", w, h, w * 8 - 8)) == E_ARG     # stride < width * bpp
    assert code(lambda: ctx.render_device(out.data_ptr(), "linear_f16", w, h, w * 8 + 4)) == E_ARG     # not a multiple of bpp
    assert code(lambda: ctx.render_device(out.data_ptr() + 4, "linear_f16", w, h, w * 8)) == E_ARG     # misaligned
    assert code(lambda: ctx.render_device(out.data_ptr() + 2, "srgb8", w, h, w * 4)) == E_ARG
    assert code(lambda: ctx.render_device(out.data_ptr(), "srgb8", w, h, 1 << 30)) == E_ARG            # beyond the allocation
    dev_render(ctx, w, h, fmt="linear_f16", out=out[:, :w])
    assert code(lambda: ctx.read_image(w, h)) == E_STATE
    ctx.render(w, h, device_only=True)
    ctx.read_image(w, h)                                            # a dst == NULL frame: readable again
    m = forma_amd.Context(devices=[0, 0])
    try:
        S.load(m, t)
        assert code(lambda: m.render_device(out.data_ptr(), "linear_f16", w, h, (w + 8) * 8)) == E_STATE
    finally:
        m.close()
    r = api.Renderer(0)
    comp = api.Composition()
    for bad in (torch.zeros((h, w, 4), dtype=torch.float32, device=_dev()),
                torch.zeros((h, w, 3), dtype=torch.uint8, device=_dev()),
                torch.zeros((h, w, 4), dtype=torch.uint8),
                torch.zeros((h, 4, w), dtype=torch.uint8, device=_dev()).permute(0, 2, 1)):
        with pytest.raises(ValueError):
            r.render_to_device(comp, bad)
