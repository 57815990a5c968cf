"""The device-resident geometry store as an incremental store (forma_hip_geometry_append / _retain, `Renderer(resident_geometry=
True)`): after any sequence of edits the device arrays are bit for bit what a from-scratch flatten and upload of the surviving
pushes holds, an edit costs in proportion to the edit, and the frame behind it is enqueued like any other."""
import gc

import numpy as np
import pytest

import scene as S
from oracle import oracle as orc
from test_gpu_host import rand_cmds

pytestmark = pytest.mark.gpu

NONE = 0xFFFFFFFF
E_ARG = -1
W = H = 640
CLEAR = (1.0, 1.0, 1.0, 1.0)


def _api():
    from forma_amd import api
    return api


def build_path(api, cmds):
    pb = api.PathBuilder()
    for c in cmds:
        k, a = c[0], c[1:]
        if k == "M": pb.move_to(api.Point(*a))
        elif k == "L": pb.line_to(api.Point(*a))
        elif k == "Q": pb.quad_to(api.Point(a[0], a[1]), api.Point(a[2], a[3]))
        elif k == "C": pb.cubic_to(api.Point(a[0], a[1]), api.Point(a[2], a[3]), api.Point(a[4], a[5]))
        elif k == "RQ": pb.rat_quad_to(api.Point(a[0], a[1]), api.Point(a[2], a[3]), a[4])
        elif k == "RC": pb.rat_cubic_to(api.Point(a[0], a[1]), api.Point(a[2], a[3]), api.Point(a[4], a[5]), a[6], a[7])
    return pb.build()


class Walk:
    """A seeded random walk of edits on one composition of `rand_cmds` paths (lines, quads, cubics, rational forms, several
    contours; every fifth path through Path.transform, the affine and the projective branch in turn)."""
    KINDS = ["new_order", "second_path", "clear_insert", "remove", "nothing"]
    MIX = [0.22, 0.10, 0.40, 0.18, 0.10]

    def __init__(self, seed, start_layers=12):
        self.api = _api()
        self.rng = np.random.default_rng(seed)
        self.comp = self.api.Composition()
        self.n_paths = 0
        self.next_order = 0
        for _ in range(start_layers):
            self._new_order()

    def path(self):
        api, i = self.api, self.n_paths
        self.n_paths += 1
        p = build_path(api, rand_cmds(self.rng, int(self.rng.integers(1, 9))))
        if i % 5 == 0:
            p = p.transform([0.8, 0.1, 5.0, -0.1, 0.8, 7.0, 0.0, 0.0, 1.0] if i % 10 == 0 else [1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0005, 0.0, 1.0])
        return p

    def _props(self):
        api = self.api
        c = [float(v) for v in self.rng.random(3, dtype=np.float32)]
        return api.Props(fill_rule=api.FillRule.EvenOdd if self.rng.random() < 0.3 else api.FillRule.NonZero,
                         func=api.Func.Draw(api.Style(fill=api.Fill.Solid(api.Color(c[0], c[1], c[2], 1.0 if self.rng.random() < 0.5 else 0.6)))))

    def _new_order(self):
        self.comp.get_mut_or_insert_default(self.api.Order(self.next_order)).insert(self.path()).set_props(self._props())
        self.next_order += 1

    def step(self):
        kind = self.KINDS[int(self.rng.choice(len(self.KINDS), p=self.MIX))]
        orders = sorted(self.comp.layers)
        if kind != "new_order" and kind != "nothing" and not orders:
            kind = "new_order"
        if kind == "new_order":
            self._new_order()
        elif kind == "second_path":
            self.comp.get_mut(self.api.Order(int(self.rng.choice(orders)))).insert(self.path())
        elif kind == "clear_insert":
            lay = self.comp.get_mut(self.api.Order(int(self.rng.choice(orders))))
            lay.clear(); lay.insert(self.path())
        elif kind == "remove":
            gone = self.comp.remove(self.api.Order(int(self.rng.choice(orders))))
            del gone                                              # `impl Drop for Layer`: its lines become garbage
            gc.collect()
        return kind


def render_host(r, comp, w=W, h=H):
    api = _api()
    img = np.zeros(w * h * 4, np.uint8)
    r.render(comp, api.BufferBuilder(img, api.LinearLayout(w, w * 4, h)).build(), api.RGBA, api.Color(*CLEAR), None)
    return img.reshape(h, w * 4)


def same_bits(a, b):
    return all(len(p) == len(q) and np.array_equal(np.ascontiguousarray(p).view(np.uint32), np.ascontiguousarray(q).view(np.uint32))
               for p, q in zip(a, b))


def oracle_of(r):
    """the oracle loaded from the renderer's store as the device holds it, plus the remaining host tables"""
    t = dict(r.host_tables)
    t["x"], t["y"], t["line_slot"] = r.read_geometry()
    o = orc.Oracle()
    S.load(o, t)
    return o


_WALK = {}


def walk_300():
    """the 300-step walk, run once: after every step the resident renderer and a FRESH default renderer draw the composition"""
    if _WALK:
        return _WALK
    api = _api()
    wk = Walk(seed=20260)
    rr = api.Renderer(0, resident_geometry=True)
    store_diff, geoms_diff, image_diff, parity = [], [], [], []
    for step in range(300):
        kind = wk.step()
        a = render_host(rr, wk.comp)
        rd = api.Renderer(0)
        b = render_host(rd, wk.comp)
        if not same_bits(rr.read_geometry(), rd.read_geometry()) or not same_bits(rd.read_geometry(), [rd.host_tables[k] for k in ("x", "y", "line_slot")]):
            store_diff.append((step, kind))
        if not np.array_equal(rr.host_tables["geoms"], rd.host_tables["geoms"]):
            geoms_diff.append((step, kind))
        if not np.array_equal(a, b):
            image_diff.append((step, kind))
        rd._ctx.close()
        if step % 25 == 24:                                       # parity with the oracle after edits (the standing contract)
            o = oracle_of(rr)
            want = o.render(W, H, clear=CLEAR)
            parity.append((step, bool(np.array_equal(o.segments(0), rr._ctx.segments(0))), bool(np.array_equal(o.segments(1), rr._ctx.segments(1))),
                           int(np.abs(want.astype(np.int16).reshape(H, W * 4) - a.astype(np.int16)).max())))
    _WALK.update(store_diff=store_diff, geoms_diff=geoms_diff, image_diff=image_diff, parity=parity, counters=rr.counters(),
                 in_store=any(k in rr.host_tables for k in ("x", "y", "line_slot")))
    rr._ctx.close()
    return _WALK


def test_store_equals_a_fresh_upload_after_every_random_edit():
    res = walk_300()
    c = res["counters"]
    print("counters after 300 steps:", c)
    assert res["store_diff"] == [], res["store_diff"][:5]        # x, y, line_slot bit-identical (compared as uint32)
    assert res["geoms_diff"] == [], res["geoms_diff"][:5]
    assert res["image_diff"] == [], res["image_diff"][:5]
    assert not res["in_store"]                                    # the resident mode keeps no geometry on the host
    assert c["geometry_retains"] >= 3 and c["geometry_appends"] >= 100, c
    assert c["geometry_uploads"] == 1, c                          # the empty store of the first frame, nothing after it


def test_parity_with_the_oracle_after_edits():
    res = walk_300()
    print("step, unsorted equal, sorted equal, max image diff:", res["parity"])
    assert len(res["parity"]) == 12
    for step, unsorted_ok, sorted_ok, diff in res["parity"]:
        assert unsorted_ok and sorted_ok, step                    # both streams bit-exact
        assert diff <= 1, (step, diff)                            # image within 1 code value


def _polygon(api, cx, cy, rad, k):
    pb = api.PathBuilder().move_to(api.Point(cx + rad, cy))
    for j in range(1, k):
        pb.line_to(api.Point(float(np.float32(cx + rad * np.cos(2 * np.pi * j / k))), float(np.float32(cy + rad * np.sin(2 * np.pi * j / k)))))
    return pb.build()


def test_an_append_costs_the_same_on_a_small_and_on_a_large_store():
    from forma_amd import scenes
    api = _api()
    extra = _polygon(api, 300.0, 300.0, 40.0, 39)                 # 39 vertices, closed: 40 points
    assert int(api._host().forma_host_path_points(extra._h)) == 40
    deltas = []
    for n_layers, lo, hi in ((20, 300, 3000), (20000, 800_000, 1_400_000)):
        comp = scenes.paris_like(n_layers=n_layers)
        r = api.Renderer(0, resident_geometry=True)
        r._upload_scene(comp, None)
        c0 = r.counters()
        assert lo <= c0["geometry_points"] <= hi, c0
        comp.get_mut_or_insert_default(api.Order(n_layers)).insert(extra)
        r._upload_scene(comp, None)
        c1 = r.counters()
        print(n_layers, "layers:", c0, "->", c1)
        assert c1["geometry_points"] == c0["geometry_points"] + 40
        assert c1["geometry_appends"] == c0["geometry_appends"] + 1
        assert c1["geometry_bytes_d2h"] == c0["geometry_bytes_d2h"] == 0       # nothing comes back
        assert c1["geometry_uploads"] == c0["geometry_uploads"]
        deltas.append(c1["geometry_bytes_h2d"] - c0["geometry_bytes_h2d"])
        r._ctx.close()
    assert deltas[0] == deltas[1] > 0, deltas


def _shape_cmds(W_, H_, n, seed):
    from forma_amd import scenes
    return list(scenes._paris_like_shapes(n, W_, H_, seed))


def test_predictions_survive_an_edit():
    """After an append the next frame is read-back-free: no learning frame, at most one void frame (the new path may break
    the "layers already sorted" shortcut); an insert that doubles N costs one re-run at most."""
    from forma_amd import scenes
    api = _api()
    W_, H_ = 1920, 1080
    comp = scenes.paris_like(n_layers=300, width=W_, height=H_, seed=7)
    for o in (150, 151):                                          # two free orders inside the order range
        gone = comp.remove(api.Order(o)); del gone
    gc.collect()
    r = api.Renderer(0, resident_geometry=True)

    def frame():
        img = render_host(r, comp, W_, H_)
        want = oracle_of(r).render(W_, H_, clear=CLEAR).reshape(H_, W_ * 4)
        d = int(np.abs(want.astype(np.int16) - img.astype(np.int16)).max())
        return d

    diffs = [frame() for _ in range(3)]
    c0 = r.counters()
    small = api.PathBuilder().move_to(api.Point(900, 500)).line_to(api.Point(930, 500)).line_to(api.Point(915, 530)).build()
    comp.get_mut_or_insert_default(api.Order(150)).insert(small).set_props(
        api.Props(func=api.Func.Draw(api.Style(fill=api.Fill.Solid(api.Color(0.1, 0.7, 0.2, 1.0))))))
    diffs += [frame() for _ in range(3)]                          # the edit's frame and the next two
    c1 = r.counters()
    print("small insert:", c0, "->", c1, "image diffs", diffs)
    assert c1["geometry_appends"] == c0["geometry_appends"] + 1 and c1["geometry_uploads"] == c0["geometry_uploads"]
    assert c1["frames"] == c0["frames"] + 3
    assert c1["frames_learned"] == c0["frames_learned"], (c0, c1)
    assert c1["frames_rerun"] <= c0["frames_rerun"] + 1, (c0, c1)
    assert max(diffs) == 0, diffs                                 # the images equal the oracle's
    # an insert that doubles N: every shape of the scene once more, in one path, a few pixels aside
    cmds = []
    for sh in _shape_cmds(W_, H_, 300, 7):
        cmds += [(c[0],) + tuple(float(np.float32(v + (5.0 if i % 2 == 0 else 3.0))) for i, v in enumerate(c[1:])) for c in sh["cmds"]]
    n_before = r.counters()["geometry_points"]
    comp.get_mut_or_insert_default(api.Order(151)).insert(build_path(api, cmds)).set_props(
        api.Props(func=api.Func.Draw(api.Style(fill=api.Fill.Solid(api.Color(0.3, 0.2, 0.8, 0.5))))))
    diffs2 = [frame() for _ in range(3)]
    c2 = r.counters()
    print("doubling insert:", c1, "->", c2, "image diffs", diffs2)
    assert c2["geometry_points"] >= 2 * n_before - 64
    assert (c2["frames_learned"] + c2["frames_rerun"]) - (c1["frames_learned"] + c1["frames_rerun"]) <= 1, (c1, c2)
    assert max(diffs2) == 0, diffs2
    r._ctx.close()


def test_frame_slots_see_every_edit():
    """the walk on a renderer with three frames in flight, through render_to_device: every enqueued frame shows its own edit"""
    import torch
    api = _api()
    wk = Walk(seed=20261)
    rr = api.Renderer(0, frames_in_flight=3, resident_geometry=True)
    outs, wants = [], []
    for step in range(60):
        wk.step()
        out = torch.zeros((H, W, 4), dtype=torch.uint8, device=torch.device("cuda", 0))
        rr.render_to_device(wk.comp, out, clear_color=api.Color(*CLEAR))
        outs.append(out)
        rd = api.Renderer(0)
        wants.append(render_host(rd, wk.comp))
        rd._ctx.close()
    rr._ctx.sync()
    torch.cuda.synchronize()
    bad = [i for i, (o, w) in enumerate(zip(outs, wants)) if not np.array_equal(o.cpu().numpy().reshape(H, W * 4), w)]
    c = rr.counters()
    print("frame slots:", c)
    assert bad == [], bad
    assert c["frames"] == 60 and c["geometry_appends"] >= 20
    rr._ctx.close()


@pytest.mark.parametrize("layout", ["exchange", "bands"])
@pytest.mark.parametrize("devices", [[0, 0], [0, 0, 0]])
def test_emulated_devices_hold_the_same_store(devices, layout):
    api = _api()
    wk = Walk(seed=20262)
    rm = api.Renderer(devices=devices, resident_geometry=True)
    rm._ctx.set_layout(layout)
    r1 = api.Renderer(0, resident_geometry=True)
    for step in range(20):
        wk.step()
        a, b = render_host(rm, wk.comp), render_host(r1, wk.comp)
        assert np.array_equal(a, b), step
        assert same_bits(rm.read_geometry(), r1.read_geometry()), step
    cm, c1 = rm.counters(), r1.counters()
    print("multi:", cm, "single:", c1)
    assert cm["geometry_appends"] == c1["geometry_appends"] and cm["geometry_points"] == c1["geometry_points"]
    assert cm["geometry_bytes_h2d"] == len(devices) * c1["geometry_bytes_h2d"]     # byte counters are summed over the devices
    rm._ctx.close(); r1._ctx.close()


def _small_store():
    """a context whose store holds three pushes (slots 0, 1, 2) of 4 points each, appended through the host batch"""
    import forma_amd
    api = _api()
    c = forma_amd.Context(0)
    tris = [api.PathBuilder().move_to(api.Point(1 + 10 * i, 1)).line_to(api.Point(9 + 10 * i, 1)).line_to(api.Point(9 + 10 * i, 9)).build() for i in range(3)]
    c.geometry_append_paths([(t, i) for i, t in enumerate(tris)])
    return c, tris


def test_argument_errors_leave_the_store_alone():
    from forma_amd import FormaError
    c, tris = _small_store()
    before = c.read_geometry()
    assert len(before[0]) == 12 and list(before[2]) == [0, 0, 0, NONE, 1, 1, 1, NONE, 2, 2, 2]
    remap = np.arange(3, dtype=np.uint32)
    bad_calls = {
        "overlapping keep ranges": lambda: c.geometry_retain([(0, 8), (4, 8)], remap),
        "descending keep ranges": lambda: c.geometry_retain([(8, 4), (0, 4)], remap),
        "a range past the end": lambda: c.geometry_retain([(0, 4), (8, 8)], remap),
        "a remap shorter than the largest slot": lambda: c.geometry_retain([(0, 4), (8, 4)], remap[:2]),
    }
    for what, call in bad_calls.items():
        with pytest.raises(FormaError) as e:
            call()
        assert e.value.code == E_ARG, what
        assert same_bits(c.read_geometry(), before), what
    # an append whose last line slot is not NONE (push_path ends every path with None)
    H_ = _api()._host()
    batch = H_.forma_host_batch_new()
    H_.forma_host_batch_add(batch, tris[0]._h, 3)
    from forma_amd._lib import FlattenTablesT
    import ctypes as C
    ft = FlattenTablesT()
    H_.forma_host_batch_tables(batch, C.byref(ft))
    ls = np.full(ft.n_points, 3, np.uint32)
    rc = c._L.forma_hip_geometry_append(c._h, C.byref(ft), ls.ctypes.data_as(C.c_void_p), None, 0)
    assert rc == E_ARG
    assert same_bits(c.read_geometry(), before)
    ls[-1] = NONE                                                 # ... and the same call with a proper last slot goes through
    assert c._L.forma_hip_geometry_append(c._h, C.byref(ft), ls.ctypes.data_as(C.c_void_p), None, 0) == 0
    H_.forma_host_batch_free(batch)
    after = c.read_geometry()
    assert len(after[0]) == 16 and list(after[2]) == [0, 0, 0, NONE, 1, 1, 1, NONE, 2, 2, 2, NONE, 3, 3, 3]
    assert same_bits([a[:12] for a in after[:2]], before[:2])
    # a well-formed retain: the middle push goes, slot 2 becomes 1, slot 3 becomes 2
    c.geometry_retain([(0, 4), (8, 8)], np.array([0, NONE, 1, 2], np.uint32))
    kept = c.read_geometry()
    assert list(kept[2]) == [0, 0, 0, NONE, 1, 1, 1, NONE, 2, 2, 2]
    assert same_bits([kept[0], kept[1]], [np.concatenate((after[0][:4], after[0][8:])), np.concatenate((after[1][:4], after[1][8:]))])
    cnt = c.counters()
    assert cnt["geometry_points"] == 12 and cnt["geometry_retains"] == 1 and cnt["geometry_appends"] == 2
    c.close()
