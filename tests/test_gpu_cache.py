"""Buffer-layer cache (BASELINE config 5): tile_unchanged pass, unchanged-visible-layers skip, cached
solid colours, "TileWriteOp::None leaves the caller's buffer untouched" — multi-frame scripts, the GPU backend against the
CPU oracle, buffers carried from frame to frame on both sides (reference forma/src/cpu/buffer/mod.rs:113-197,
cpu/painter/mod.rs:629-715, passes/tile_unchanged.rs, composition/mod.rs tests `render_changed_layers_only`,
`clear_emptied_tiles`, `separate_layer_caches`, `draw_if_width_or_height_change`)."""
import os

import numpy as np
import pytest

import scene as S
from oracle import oracle as orc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import forma_amd
    c = forma_amd.Context(0)
    yield c
    c.close()


def frame(o, ctx, comp, bufs, w, h, clear, cache_id, reload_geometry):
    """Render one frame on both backends into their own persistent buffers; returns (oracle_buf, gpu_buf)."""
    t = comp.tables(o)
    S.load(o, t)
    if reload_geometry:
        S.load(ctx, t)
    else:                                                  # geometry stays resident: only layer table + styles change
        ctx.set_geoms(t["geoms"])
        ctx.set_styles(t["style_offsets"], t["style_words"], t["unchanged"])
    o.render(w, h, clear=clear, cache_id=cache_id, dst=bufs[0])
    ctx.render(w, h, clear=clear, cache_id=cache_id, dst=bufs[1])
    return bufs


def build(n=40, seed=9, w=256, h=192, opaque=True):
    rng = np.random.default_rng(seed)
    comp = S.Composition()
    for i in range(n):
        x0, y0 = rng.uniform(-20, w), rng.uniform(-20, h)
        a = 1.0 if (opaque and i % 3 == 0) else 0.6
        shape = S.custom_square(float(x0), float(y0), float(x0 + rng.uniform(20, 120)), float(y0 + rng.uniform(20, 120))) \
            if i % 2 == 0 else S.custom_circle(float(x0), float(y0), float(rng.uniform(8, 50)))
        comp.get_mut_or_insert_default(i).insert(shape).set_props(S.solid((float(rng.random()), float(rng.random()), float(rng.random()), a)))
    return comp


def set_unchanged(comp, value, except_orders=()):
    for order, layer in comp.layers.items():
        layer.unchanged = value and order not in except_orders


def test_static_scene_second_frame_touches_nothing(ctx):
    w, h = 256, 192
    o = orc.Oracle()
    comp = build()
    clear = (1.0, 1.0, 1.0, 1.0)
    bufs = [np.full((h, w * 4), 7, np.uint8), np.full((h, w * 4), 7, np.uint8)]
    set_unchanged(comp, False)
    frame(o, ctx, comp, bufs, w, h, clear, 3, True)
    assert np.abs(bufs[0].astype(int) - bufs[1].astype(int)).max() <= 1 and (bufs[1] != 7).any()
    # nothing changed; the caller wipes its buffer: the renderer must not touch it (doc test of BufferLayerCache)
    set_unchanged(comp, True)
    bufs = [np.full((h, w * 4), 9, np.uint8), np.full((h, w * 4), 9, np.uint8)]
    frame(o, ctx, comp, bufs, w, h, clear, 3, False)
    assert (bufs[0] == 9).all() and (bufs[1] == 9).all()
    # a different clear colour repaints everything
    frame(o, ctx, comp, bufs, w, h, (0.0, 0.0, 0.0, 1.0), 3, False)
    assert np.abs(bufs[0].astype(int) - bufs[1].astype(int)).max() <= 1 and (bufs[1] != 9).any()


def test_changed_layers_repaint_only_their_tiles(ctx):
    w, h = 256, 192
    o = orc.Oracle()
    comp = build(seed=21)
    clear = (0.2, 0.3, 0.4, 1.0)
    bufs = [np.zeros((h, w * 4), np.uint8), np.zeros((h, w * 4), np.uint8)]
    set_unchanged(comp, False)
    frame(o, ctx, comp, bufs, w, h, clear, 0, True)
    rng = np.random.default_rng(2)
    for step in range(6):
        moved = set(int(v) for v in rng.choice(40, size=3, replace=False))
        set_unchanged(comp, True, except_orders=moved)
        for m in moved:
            comp.layers[m].set_transform([1.0, 0.0, 0.0, 1.0, float(rng.uniform(-40, 40)), float(rng.uniform(-30, 30))])
        t = comp.tables(o); S.load(o, t); ctx.set_geoms(t["geoms"]); ctx.set_styles(t["style_offsets"], t["style_words"], t["unchanged"])
        # which tiles does each backend WRITE?  Both render into a sentinel-filled buffer: a tile the optimizer skips
        # (TileWriteOp::None) keeps the sentinel.  (A value no pixel of this scene takes in all four channels.)
        sent = [np.full((h, w * 4), 201, np.uint8), np.full((h, w * 4), 201, np.uint8)]
        o.render(w, h, clear=clear, cache_id=0, dst=sent[0])
        ctx.render(w, h, clear=clear, cache_id=0, dst=sent[1])
        tiles_o = (sent[0] != 201).reshape(h // 16, 16, w // 16, 16, 4).any(axis=(1, 3, 4))
        tiles_g = (sent[1] != 201).reshape(h // 16, 16, w // 16, 16, 4).any(axis=(1, 3, 4))
        assert np.array_equal(tiles_o, tiles_g), (step, "the two backends rewrote different tiles")
        assert np.array_equal(tiles_g.reshape(-1) != 0, ctx.tiles_written(w, h) != 0)
        assert 0 < tiles_g.sum() < tiles_g.size                         # partial damage: some tiles skipped, some repainted
        # the caller's carried buffers take exactly those tiles
        for k in range(2):
            m = np.repeat(np.repeat([tiles_o, tiles_g][k], 16, axis=0), 16 * 4, axis=1)
            bufs[k][m] = sent[k][m]
        d = np.abs(bufs[0].astype(int) - bufs[1].astype(int))
        assert d.max() <= 1, (step, d.max())


def test_solid_tiles_and_size_change(ctx):
    """Opaque full covers fold to TileWriteOp::Solid; an unchanged solid colour is skipped; a new canvas size clears the
    cache (renderer.rs:94-111)."""
    o = orc.Oracle()
    comp = S.Composition()
    comp.get_mut_or_insert_default(0).insert(S.custom_square(-10, -10, 500, 500)).set_props(S.solid((0.2, 0.4, 0.6, 1.0)))
    comp.get_mut_or_insert_default(1).insert(S.custom_circle(100, 80, 30)).set_props(S.solid((0.9, 0.1, 0.1, 0.5)))
    set_unchanged(comp, False)
    for (w, h) in ((200, 160), (200, 160), (144, 96), (144, 96)):
        bufs = [np.full((h, w * 4), 33, np.uint8), np.full((h, w * 4), 33, np.uint8)]
        frame(o, ctx, comp, bufs, w, h, (1, 1, 1, 1), 5, True)
        assert np.array_equal(bufs[0] == 33, bufs[1] == 33), (w, h)      # same tiles skipped / written
        assert np.abs(bufs[0].astype(int) - bufs[1].astype(int)).max() <= 1
        set_unchanged(comp, False)                                        # layers reported changed: only solid-colour caching applies


def test_separate_caches_do_not_interfere(ctx):
    w, h = 160, 128
    o = orc.Oracle()
    comp = build(n=20, seed=4, w=w, h=h)
    set_unchanged(comp, False)
    b0 = [np.zeros((h, w * 4), np.uint8), np.zeros((h, w * 4), np.uint8)]
    b1 = [np.zeros((h, w * 4), np.uint8), np.zeros((h, w * 4), np.uint8)]
    frame(o, ctx, comp, b0, w, h, (1, 1, 1, 1), 1, True)
    frame(o, ctx, comp, b1, w, h, (0, 0, 0, 1), 2, False)
    set_unchanged(comp, True)
    s0 = [np.full((h, w * 4), 5, np.uint8), np.full((h, w * 4), 5, np.uint8)]
    frame(o, ctx, comp, s0, w, h, (1, 1, 1, 1), 1, False)                 # cache 1: unchanged, same clear -> untouched
    assert (s0[0] == 5).all() and (s0[1] == 5).all()
    s1 = [np.full((h, w * 4), 5, np.uint8), np.full((h, w * 4), 5, np.uint8)]
    frame(o, ctx, comp, s1, w, h, (1, 1, 1, 1), 2, False)                 # cache 2: clear colour differs -> repainted
    assert np.abs(s1[0].astype(int) - s1[1].astype(int)).max() <= 1 and (s1[1] != 5).any()
    ctx._check(ctx._L.forma_hip_cache_clear(ctx._h, 1)); o.cache_clear(1)
    s0 = [np.full((h, w * 4), 5, np.uint8), np.full((h, w * 4), 5, np.uint8)]
    frame(o, ctx, comp, s0, w, h, (1, 1, 1, 1), 1, False)                 # cleared cache: everything is drawn again
    assert np.abs(s0[0].astype(int) - s0[1].astype(int)).max() <= 1 and (s0[1] != 5).any()


def test_written_tile_count_is_reported(ctx):
    """forma_timings_t.n_tiles_written = the damage: every tile without a cache, only the rewritten ones with one."""
    w, h = 256, 192
    o = orc.Oracle()
    comp = build()
    set_unchanged(comp, False)
    t = comp.tables(o)
    S.load(ctx, t)
    _, tm = ctx.render(w, h, clear=(1, 1, 1, 1), timings=True)
    assert tm["n_tiles_written"] == (w // 16) * (h // 16)
    buf = np.zeros((h, w * 4), np.uint8)
    ctx.cache_clear(5)
    _, tm = ctx.render(w, h, clear=(1, 1, 1, 1), cache_id=5, dst=buf, timings=True)
    assert tm["n_tiles_written"] == (w // 16) * (h // 16)
    set_unchanged(comp, True)
    t = comp.tables(o)
    ctx.set_styles(t["style_offsets"], t["style_words"], t["unchanged"])
    _, tm = ctx.render(w, h, clear=(1, 1, 1, 1), cache_id=5, dst=buf, timings=True)
    assert tm["n_tiles_written"] == 0


def _written(buf, sentinel, w, h):
    """tiles a frame wrote into a sentinel-filled buffer, [tiles_h][tiles_w] (partial edge tiles included)"""
    tw, th = (w + 15) // 16, (h + 15) // 16
    out = np.zeros((th, tw), bool)
    px = (buf.reshape(h, w, 4) != sentinel).any(axis=2)
    for ty in range(th):
        for tx in range(tw):
            out[ty, tx] = px[ty * 16: ty * 16 + 16, tx * 16: tx * 16 + 16].any()
    return out


def test_damage_set_on_a_canvas_whose_height_is_not_a_multiple_of_16(ctx):
    """VERDICT r2 (weak 2): layers that cross the BOTTOM edge of a 1080p-style canvas keep a non-zero cover on the invisible
    pixel rows of the partial last tile row, and the reference carries them through every tile to their right — so they
    count in those tiles' layer_count (what `passes/tile_unchanged.rs` compares between frames), they block the solid-tile
    fold, and a change that only concerns them still rewrites those tiles.  With a buffer-layer cache attached the HIP path
    carries them exactly like the reference: the written-tile set equals the oracle's frame by frame, including nested /
    overlapping clips that cross the edge (a dropped clip span would leave a stale clip mask)."""
    w, h = 320, 200                                        # 12.5 tile rows: the last one shows 8 of its 16 pixel rows
    rng = np.random.default_rng(12)
    comp = S.Composition()
    comp.get_mut_or_insert_default(0).insert(S.custom_square(-5, -5, w + 5, h + 40)).set_props(S.solid((0.85, 0.9, 0.8, 1.0)))
    order = 1
    for i in range(24):                                    # shapes hanging over the bottom edge, some entirely below the visible rows
        x0 = float(rng.uniform(-10, w - 30)); y0 = float(rng.uniform(150, 204))
        shape = S.custom_square(x0, y0, x0 + float(rng.uniform(10, 60)), y0 + float(rng.uniform(10, 50))) if i % 2 else \
            S.custom_circle(x0 + 20, y0 + 20, float(rng.uniform(6, 30)))
        a = 1.0 if i % 4 == 0 else 0.5
        comp.get_mut_or_insert_default(order).insert(shape).set_props(S.solid((float(rng.random()), float(rng.random()), float(rng.random()), a)))
        order += 1
    # two overlapping clip ranges crossing the edge, and clipped layers inside both
    comp.get_mut_or_insert_default(order).insert(S.custom_circle(60, 196, 30)).set_props(S.Props(clip=6)); order += 1
    comp.get_mut_or_insert_default(order).insert(S.custom_square(20, 150, 200, 260)).set_props(S.Props(fill=(0.9, 0.1, 0.1, 1.0), is_clipped=True)); order += 1
    comp.get_mut_or_insert_default(order).insert(S.custom_square(70, 194, 140, 230)).set_props(S.Props(clip=3)); order += 1   # visible rows: empty
    comp.get_mut_or_insert_default(order).insert(S.custom_square(30, 160, 300, 240)).set_props(S.Props(fill=(0.1, 0.1, 0.9, 0.8), is_clipped=True)); order += 1
    comp.get_mut_or_insert_default(order).insert(S.custom_circle(250, 150, 40)).set_props(S.solid((0.2, 0.7, 0.3, 0.7))); order += 1
    n = order
    o = orc.Oracle()
    clear = (1.0, 1.0, 1.0, 1.0)
    bufs = [np.zeros((h, w * 4), np.uint8), np.zeros((h, w * 4), np.uint8)]
    set_unchanged(comp, False)
    frame(o, ctx, comp, bufs, w, h, clear, 7, True)
    assert np.abs(bufs[0].astype(int) - bufs[1].astype(int)).max() <= 1
    moves = [set(), {3}, {5, 9}, set(), {24}, {25, 26}, {27}, {2, 11, 13}, set()]
    for step, moved in enumerate(moves):
        set_unchanged(comp, True, except_orders=moved)
        for m in moved:
            comp.layers[m].set_transform([1.0, 0.0, 0.0, 1.0, float(rng.uniform(-25, 25)), float(rng.uniform(-6, 6))])
        t = comp.tables(o); S.load(o, t); ctx.set_geoms(t["geoms"]); ctx.set_styles(t["style_offsets"], t["style_words"], t["unchanged"])
        sent = [np.full((h, w * 4), 201, np.uint8), np.full((h, w * 4), 201, np.uint8)]
        o.render(w, h, clear=clear, cache_id=7, dst=sent[0])
        ctx.render(w, h, clear=clear, cache_id=7, dst=sent[1])
        wo, wg = _written(sent[0], 201, w, h), _written(sent[1], 201, w, h)
        assert np.array_equal(wo, wg), (step, "written tiles differ", np.argwhere(wo != wg)[:8].tolist())
        assert np.array_equal(wg.reshape(-1), ctx.tiles_written(w, h) != 0), step
        if not moved:
            assert not wg.any(), step                      # nothing changed: nothing written (also in the partial last row)
        d = np.abs(sent[0].astype(int) - sent[1].astype(int))
        assert d.max() <= 1, (step, int(d.max()))
    # and without a cache the picture is the oracle's, invisible carries dropped or not
    want = o.render(w, h, clear=clear)
    got = ctx.render(w, h, clear=clear)
    assert np.abs(want.astype(int) - got.astype(int)).max() <= 1


def test_small_damage_leaves_the_device_as_packed_tiles(ctx):
    """A cache frame that rewrites a few tiles copies out only those (k_written_list / k_pack_written: the written tiles of the
    crop, packed on the device, dropped into place on the host) instead of the whole canvas.  Canvas and crop are not
    multiples of the tile size (partial edge tiles), one small layer moves per frame: buffers and written-tile sets equal the
    oracle's frame after frame; the frame that moves everything takes the whole-crop path again."""
    w, h = 602, 330
    o = orc.Oracle()
    comp = build(n=60, seed=33, w=w, h=h)
    clear = (0.9, 0.8, 0.7, 1.0)
    crop = (35, 571, 20, 317)                                           # x0, x1, y0, y1: cuts tiles on all four sides
    bufs = [np.zeros((h, w * 4), np.uint8), np.zeros((h, w * 4), np.uint8)]
    set_unchanged(comp, False)
    t = comp.tables(o); S.load(o, t); S.load(ctx, t)
    o.render(w, h, clear=clear, cache_id=1, dst=bufs[0], crop=crop); ctx.render(w, h, clear=clear, cache_id=1, dst=bufs[1], crop=crop)
    assert np.array_equal(bufs[0], bufs[1])
    rng = np.random.default_rng(5)
    for step in range(8):
        moved = {int(rng.integers(0, 60))} if step != 5 else set(range(60))
        set_unchanged(comp, True, except_orders=moved)
        for m in moved:
            comp.layers[m].set_transform([1.0, 0.0, 0.0, 1.0, float(rng.uniform(-25, 25)), float(rng.uniform(-20, 20))])
        t = comp.tables(o); S.load(o, t); ctx.set_geoms(t["geoms"]); ctx.set_styles(t["style_offsets"], t["style_words"], t["unchanged"])
        sent = [np.full((h, w * 4), 201, np.uint8), np.full((h, w * 4), 201, np.uint8)]
        o.render(w, h, clear=clear, cache_id=1, dst=sent[0], crop=crop); ctx.render(w, h, clear=clear, cache_id=1, dst=sent[1], crop=crop)
        assert np.array_equal(sent[0], sent[1]), step
        wr = _written(sent[1], 201, w, h)
        assert np.array_equal(wr.reshape(-1), ctx.tiles_written(w, h) != 0), step
        if step != 5:
            assert 0 < wr.sum() < wr.size // 4, (step, wr.sum())        # few tiles: the packed path
        o.render(w, h, clear=clear, cache_id=1, dst=bufs[0], crop=crop); ctx.render(w, h, clear=clear, cache_id=1, dst=bufs[1], crop=crop)
        assert np.array_equal(bufs[0], bufs[1]), step


@pytest.mark.parametrize("seed", list(range(int(os.environ.get("FORMA_TEST_FUZZ_SEEDS", "12")))))
def test_damage_sets_of_random_scenes(seed):
    """Written-tile sets with a buffer-layer cache, randomised: all-features scenes (clips, clipped layers, gradients,
    textures, blend modes, both fill rules, shapes over every canvas edge) on canvases off the tile grid, random crops, a
    random subset of layers moving / toggling / restyled per frame.  Frame after frame the buffer a renderer carries and the
    set of tiles it rewrote (sentinel buffer) equal the oracle's — `CachedTile` state (layer count, solid colour) is compared
    by the reference itself on the next frame, so any drift shows up as a different damage set."""
    import forma_amd
    rng = np.random.default_rng(1000 + seed)
    w, h = int(rng.integers(40, 700)), int(rng.integers(40, 420))
    n = int(rng.integers(5, 140))
    comp = S.random_mixed(n=n, width=w, height=h, seed=500 + seed)
    if seed % 4 == 3:                                     # all solid / Over / unclipped: the painter's kernel for such scenes
        for layer in comp.layers.values():
            layer.set_props(S.Props(fill_rule=layer.props.fill_rule,
                                    fill=tuple(float(v) for v in rng.random(3)) + ((1.0,) if rng.random() < 0.4 else (float(rng.random()),))))
    orders = sorted(comp.layers.keys())
    crop = None
    if seed % 3 == 1:
        x0, y0 = int(rng.integers(0, w // 2)), int(rng.integers(0, h // 2))
        crop = (x0, int(rng.integers(x0 + 1, w + 1)), y0, int(rng.integers(y0 + 1, h + 1)))
    clear = tuple(float(v) for v in rng.random(3)) + (1.0,)
    o = orc.Oracle(); c = forma_amd.Context(0)
    try:
        bufs = [np.full((h, w * 4), 77, np.uint8), np.full((h, w * 4), 77, np.uint8)]
        for frame_no in range(7):
            if frame_no == 0:
                set_unchanged(comp, False)
            else:
                k = int(rng.integers(0, max(2, len(orders) // 6)))
                moved = set(int(v) for v in rng.choice(orders, size=min(k, len(orders)), replace=False))
                set_unchanged(comp, True, except_orders=moved)
                for m in moved:
                    kind = int(rng.integers(0, 3))
                    L = comp.layers[m]
                    if kind == 0:
                        L.set_transform([1.0, 0.0, 0.0, 1.0, float(rng.uniform(-60, 60)), float(rng.uniform(-40, 40))])
                    elif kind == 1:
                        L.enabled = not L.enabled
                    elif L.props.clip is None and isinstance(L.props.fill, tuple):
                        L.props.fill = tuple(float(v) for v in rng.random(3)) + (L.props.fill[3],)
                if frame_no == 4:
                    clear = tuple(float(v) for v in rng.random(3)) + (1.0,)      # a new clear colour repaints everything
            t = comp.tables(o)
            S.load(o, t)
            if frame_no == 0:
                S.load(c, t)
            else:
                c.set_geoms(t["geoms"]); c.set_styles(t["style_offsets"], t["style_words"], t["unchanged"])
            sent = [np.full((h, w * 4), 201, np.uint8), np.full((h, w * 4), 201, np.uint8)]
            # two renders per frame and backend would advance the cache twice: the sentinel pair is the frame, the carried
            # buffers are patched from it (a sentinel pixel = the renderer left the tile alone)
            o.render(w, h, clear=clear, cache_id=2, dst=sent[0], crop=crop); c.render(w, h, clear=clear, cache_id=2, dst=sent[1], crop=crop)
            wo, wg = _written(sent[0], 201, w, h), _written(sent[1], 201, w, h)
            assert np.array_equal(wo, wg), (seed, frame_no, int(wo.sum()), int(wg.sum()))
            assert np.abs(sent[0].astype(int) - sent[1].astype(int)).max() <= 1, (seed, frame_no)
            assert np.array_equal(wg.reshape(-1), c.tiles_written(w, h) != 0), (seed, frame_no)
    finally:
        c.close()


def test_copy_out_buffers_grow_and_shrink_on_one_context():
    """One context, cache frames into host memory at 64 x 64, then 256 x 192, then 64 x 64 again: the page-locked buffers behind the
    copy-out (written-tile flags, staging image) are kept at the largest size seen and must serve the smaller canvas after the larger
    one.  Per size: a fully repainted frame (one strided copy), a frame with one small changed layer (the packed tiles), one
    with two larger changed layers, and a device-resident frame whose flags `tiles_written` fetches afterwards."""
    import forma_amd
    c = forma_amd.Context(0)
    o = orc.Oracle()
    clear = (0.9, 0.8, 0.7, 1.0)
    dot = 10                                               # a small circle inside tile (1, 1), wherever it moves below
    try:
        for n_size, (w, h) in enumerate(((64, 64), (256, 192), (64, 64))):
            comp = build(n=10, seed=40 + n_size, w=w, h=h)
            comp.get_mut_or_insert_default(dot).insert(S.custom_circle(23.0, 23.0, 4.0)).set_props(S.solid((0.9, 0.1, 0.2, 1.0)))
            tiles = ((w + 15) // 16) * ((h + 15) // 16)
            for step, moved in enumerate((None, {dot}, {2, 5}, {dot})):
                device_only = step == 3
                set_unchanged(comp, moved is not None, except_orders=moved or ())
                for k, m in enumerate(sorted(moved or ())):
                    comp.layers[m].set_transform([1.0, 0.0, 0.0, 1.0, float(step), 1.0] if m == dot else [1.0, 0.0, 0.0, 1.0, 9.0 + 4 * k, -7.0])
                t = comp.tables(o); S.load(o, t)
                if moved is None:
                    S.load(c, t)
                else:
                    c.set_geoms(t["geoms"]); c.set_styles(t["style_offsets"], t["style_words"], t["unchanged"])
                sent = [np.full((h, w * 4), 201, np.uint8), np.full((h, w * 4), 201, np.uint8)]
                o.render(w, h, clear=clear, cache_id=4, dst=sent[0])
                if device_only:
                    c.render(w, h, clear=clear, cache_id=4, device_only=True)
                else:
                    c.render(w, h, clear=clear, cache_id=4, dst=sent[1])
                wo = _written(sent[0], 201, w, h)
                assert np.array_equal(wo.reshape(-1), c.tiles_written(w, h) != 0), (w, h, step)
                if step == 0:
                    assert wo.all(), (w, h)                                # everything painted: the strided copy
                elif moved == {dot}:
                    assert 0 < wo.sum() <= max(tiles // 4, 1), (w, h, step, int(wo.sum()))    # few tiles: the packed copy
                got = c.read_image(w, h) if device_only else sent[1]
                if device_only:                                            # (the cache's image: compared where this frame wrote)
                    m = np.repeat(np.repeat(wo, 16, axis=0), 16 * 4, axis=1)[:h, :w * 4]
                    assert np.abs(got[m].astype(int) - sent[0][m].astype(int)).max() <= 1, (w, h, step)
                else:
                    assert np.array_equal(wo, _written(got, 201, w, h)), (w, h, step)
                    assert np.abs(got.astype(int) - sent[0].astype(int)).max() <= 1, (w, h, step)
    finally:
        c.close()
