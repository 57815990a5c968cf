"""The context's state by owner (csrc/ctx.h): the scene's scalars (`SceneFacts`) reach every frame slot with the borrowed buffers,
and a frame slot's FORMA_HIP_DEBUG switches are its owner's.  A 96 x 80 canvas (no multiple of the tile size, more than one tile
row and column), a dozen layers; images against the oracle within the parity contract's one RGBA8 step, frame slots against a
fresh one-slot context bit for bit."""
import numpy as np
import pytest

import scene as S
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

NONE = 0xFFFFFFFF
W, H = 96, 80
CLEAR = (1.0, 1.0, 1.0, 1.0)
EXTRA = 12                                                 # an order (and table slot) without geometry: the append draws into it


def _scene(seed):
    comp = S.random_cubics(n=12, width=W, height=H, seed=seed, alpha=0.8)
    comp.get_mut_or_insert_default(EXTRA).set_props(S.solid((0.1, 0.6, 0.3, 0.7)))
    return comp


def _device_frame(c, crop=None):
    c.render(W, H, clear=CLEAR, crop=crop, device_only=True)
    return c.read_image(W, H)


def _check_slots(m, t, what, band=None, oracle=None):
    """six device-resident frames of the three-slot context `m` (every slot renders twice), each bit for bit the frame of a fresh
    one-slot context loaded with the tables `t`.  A band frame is painted with the band's crop, as a multi-device context does:
    only those rows are the frame's."""
    import forma_amd
    crop, rows = (None, slice(0, H)) if band is None else ((0, W, band[0] * 16, band[1] * 16), slice(band[0] * 16, band[1] * 16))
    f = forma_amd.Context(0)
    try:
        S.load(f, t)
        if band is not None:
            f.set_band(*band)
        want = _device_frame(f, crop)[rows]
    finally:
        f.close()
    if oracle is not None:
        S.load(oracle, t)
        d = np.abs(want.astype(int) - oracle.render(W, H, clear=CLEAR).astype(int)).max()
        print(what, "fresh context against the oracle: max difference", d)
        assert d <= 1, what
    for k in range(6):
        got = _device_frame(m, crop)[rows]
        assert np.array_equal(got, want), (what, "frame", k, int((got != want).sum()))


def test_every_scene_fact_reaches_every_slot():
    import forma_amd
    from forma_amd import api
    o = orc.Oracle()
    comp = _scene(5)
    t = comp.tables(o)
    m = forma_amd.Context(0, frames_in_flight=3)
    try:
        S.load(m, t)
        # set_geometry: other points under the same layer table
        t2 = _scene(6).tables(o)
        for k in ("x", "y", "line_slot"):
            t[k] = t2[k]
        m.set_geometry(t["x"], t["y"], t["line_slot"])
        _check_slots(m, t, "set_geometry", oracle=o)
        # set_geoms: a layer disabled, one transformed
        g = t["geoms"].copy()
        g[3]["order"] = NONE
        g[5]["flags"] = 1; g[5]["xf"] = (0.9, 0.1, -0.1, 0.9, 4.0, -3.0)
        t["geoms"] = g
        m.set_geoms(g)
        _check_slots(m, t, "set_geoms")

        def restyle(images=False):
            s = comp.tables(o)
            for k in ("style_offsets", "style_words", "unchanged") + (("images", "texels") if images else ()):
                t[k] = s[k]
            m.set_styles(t["style_offsets"], t["style_words"], t["unchanged"])
            if images:
                m.set_images(t["images"], t["texels"])
        # set_styles: a clip layer and layers clipped by it
        comp.layers[1].set_props(S.Props(clip=3))
        for k in (2, 3, 4):
            comp.layers[k].props.is_clipped = True
        restyle()
        _check_slots(m, t, "set_styles: clip")
        # set_styles: a blend mode other than Over
        comp.layers[8].props.blend_mode = "Multiply"
        restyle()
        _check_slots(m, t, "set_styles: blend")
        # set_images: a texture fill
        rng = np.random.default_rng(3)
        img = S.Image.from_srgba([[int(v) for v in rng.integers(0, 256, 4)] for _ in range(16)], 4, 4)
        comp.layers[9].props.fill = S.Texture((0.1, 0.02, -0.03, 0.1, 1.0, 2.0), img)
        restyle(images=True)
        _check_slots(m, t, "set_images: texture")
        # set_band
        m.set_band(1, 4)
        _check_slots(m, t, "set_band(1, 4)", band=(1, 4))
        m.set_band(0, 0)
        _check_slots(m, t, "set_band(0, 0)")
        # geometry_append: a triangle into the empty slot; geometry_retain: the first layer's points go
        tri = api.PathBuilder().move_to(api.Point(10, 12)).line_to(api.Point(70, 20)).line_to(api.Point(30, 66)).build()
        m.geometry_append_paths([(tri, EXTRA)])
        t["x"], t["y"], t["line_slot"] = m.read_geometry()
        assert (t["line_slot"] == EXTRA).sum() >= 3
        _check_slots(m, t, "geometry_append")
        n = len(t["x"])
        first = int(np.argmax(t["line_slot"] == NONE)) + 1          # points of the first path (its last one starts no line)
        assert 0 < first < n
        m.geometry_retain([(first, n - first)], np.arange(EXTRA + 1, dtype=np.uint32))
        t["x"], t["y"], t["line_slot"] = m.read_geometry()
        assert len(t["x"]) == n - first
        _check_slots(m, t, "geometry_retain")
    finally:
        m.close()


def _nine_frames(c, want):
    before = c.counters()["frames_learned"]
    for k in range(9):
        d = np.abs(_device_frame(c).astype(int) - want.astype(int)).max()
        assert d <= 1, (k, d)
    return c.counters()["frames_learned"] - before


def test_a_slots_switches_are_its_owners(monkeypatch):
    """FORMA_HIP_DEBUG is parsed when a context is created; frame slots made later, under another environment, follow their owner.
    `sync` shows in the counters: every frame of such a context is a learning (synchronous) frame."""
    import forma_amd
    o = orc.Oracle()
    t = _scene(5).tables(o)
    S.load(o, t)
    want = o.render(W, H, clear=CLEAR)
    # created under sync, slots made without it: all nine frames are synchronous
    monkeypatch.setenv("FORMA_HIP_DEBUG", "sync")
    c = forma_amd.Context(0)
    try:
        monkeypatch.delenv("FORMA_HIP_DEBUG")
        S.load(c, t)
        c.set_frames_in_flight(3)
        assert _nine_frames(c, want) == 9
    finally:
        c.close()
    # created without it, slots made under sync: the slots enqueue like their owner — what a one-slot context learns, never nine
    a = forma_amd.Context(0); b = forma_amd.Context(0)
    try:
        monkeypatch.setenv("FORMA_HIP_DEBUG", "sync")
        grew = []
        for c, slots in ((a, 3), (b, 1)):
            S.load(c, t)
            c.set_frames_in_flight(slots)
            for _ in range(3):
                _device_frame(c)
            grew.append(_nine_frames(c, want))
        print("frames_learned grew by", grew, "(three slots, one slot)")
        assert grew[0] in (0, grew[1]) and grew[0] != 9, grew
    finally:
        a.close(); b.close()
