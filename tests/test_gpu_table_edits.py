"""The layer table edited with frames in flight (forma_hip_update_geoms / _update_geoms_xf / _read_geoms, `Renderer(
resident_tables=True)`): after any sequence of edits every later frame renders what one forma_hip_set_geoms with the edited
table renders, a frame already enqueued keeps the table it was enqueued with, and the edit settles no frame in flight."""
import ctypes as C

import numpy as np
import pytest

import scene as S
from oracle import oracle as orc
from test_gpu_geometry_store import Walk, render_host

pytestmark = pytest.mark.gpu

NONE = 0xFFFFFFFF
E_ARG = -1
LAYER_LIMIT = 0x1FFFFF
W = H = 640
CLEAR = (1.0, 1.0, 1.0, 1.0)
IDENTITY = (1.0, 0.0, 0.0, 1.0, 0.0, 0.0)


def _fa():
    import forma_amd
    return forma_amd


_TABLES = {}


def base_tables(seed=4711, layers=24):
    """the flat tables of a `rand_cmds` composition (the geometry-store walk's start), built once per seed"""
    key = (seed, layers)
    if key not in _TABLES:
        from forma_amd import api
        wk = Walk(seed=seed, start_layers=layers)
        r = api.Renderer(0)
        render_host(r, wk.comp)
        _TABLES[key] = {k: np.array(v) for k, v in r.host_tables.items()}
        r._ctx.close()
    return {k: v.copy() for k, v in _TABLES[key].items()}


def new_ctx(t, **kw):
    c = _fa().Context(0, **kw) if "devices" not in kw else _fa().Context(**kw)
    S.load(c, t)
    return c


def words(g):
    return np.ascontiguousarray(g).view(np.uint32)


def same_table(c, mirror):
    got = c.read_geoms()
    return len(got) == len(mirror) and np.array_equal(words(got), words(mirror))


def rand_xf(rng, spread=30.0):
    s = rng.uniform(0.8, 1.2); th = rng.uniform(-0.2, 0.2)
    return tuple(float(np.float32(v)) for v in (s * np.cos(th), s * np.sin(th), -s * np.sin(th), s * np.cos(th),
                                                rng.uniform(-spread, spread), rng.uniform(-spread, spread)))


def apply_xf(mirror, first, count, xf):
    """what forma_hip_update_geoms_xf does to the table: flags bit 0 and xf; the order stays"""
    mirror["flags"][first:first + count] = (mirror["flags"][first:first + count] & ~np.uint32(1)) | np.uint32(0 if xf is None else 1)
    mirror["xf"][first:first + count] = IDENTITY if xf is None else xf


def oracle_image(t, geoms, w=W, h=H):
    o = orc.Oracle()
    tt = dict(t); tt["geoms"] = geoms
    S.load(o, tt)
    return o.render(w, h, clear=CLEAR).reshape(h, w * 4)


# 1 --------------------------------------------------------------------------------------------------------------------
def test_random_walk_of_edits_equals_set_geoms():
    t = base_tables()
    n = len(t["geoms"])
    rng = np.random.default_rng(20271)
    a = new_ctx(t, frames_in_flight=3)
    b = new_ctx(t)
    mirror = t["geoms"].copy()
    home = mirror["order"].copy()                                 # the order every slot started with
    assert same_table(a, mirror)                                  # read_geoms before any edit: what set_geoms was given
    kinds = ["entry_xf", "order_none", "order_back", "swap", "xf_range", "xf_identity", "same_slot_thrice", "overlap", "empty"]
    seen, table_diff, image_diff, oracle_diff = set(), [], [], []
    for step in range(320):
        kind = kinds[int(rng.integers(len(kinds)))] if step >= len(kinds) else kinds[step]
        seen.add(kind)
        if kind == "entry_xf":
            slots = rng.choice(n, size=int(rng.integers(1, 6)), replace=False).astype(np.uint32)
            e = mirror[slots].copy()
            for i in range(len(slots)):
                e[i]["flags"] = 1; e[i]["xf"] = rand_xf(rng)
            a.update_geoms(slots, e); mirror[slots] = e
        elif kind == "order_none":
            s = int(rng.integers(n)); e = mirror[[s]].copy(); e["order"] = NONE
            a.update_geoms([s], e); mirror[s] = e[0]
        elif kind == "order_back":
            slots = np.flatnonzero(mirror["order"] == NONE).astype(np.uint32)
            if len(slots):
                e = mirror[slots].copy(); e["order"] = home[slots]
                taken = set(int(o) for o in mirror["order"] if o != NONE)
                keep = [i for i in range(len(slots)) if int(e[i]["order"]) not in taken]
                a.update_geoms(slots[keep], e[keep]); mirror[slots[keep]] = e[keep]
        elif kind == "swap":
            s0, s1 = (int(v) for v in rng.choice(n, size=2, replace=False))
            e = mirror[[s0, s1]].copy(); e["order"] = e["order"][::-1].copy()
            a.update_geoms([s0, s1], e); mirror[[s0, s1]] = e
        elif kind in ("xf_range", "xf_identity"):
            first = int(rng.integers(n)); count = int(rng.integers(1, n - first + 1))
            xf = None if kind == "xf_identity" else rand_xf(rng)
            a.update_geoms_xf(first, count, xf); apply_xf(mirror, first, count, xf)
        elif kind == "same_slot_thrice":                          # within one call the later record wins
            s = int(rng.integers(n)); other = int((s + 1) % n)
            e = mirror[[s, other, s, s]].copy()
            for i in range(4):
                e[i]["flags"] = 1; e[i]["xf"] = rand_xf(rng)
            a.update_geoms([s, other, s, s], e); mirror[other] = e[1]; mirror[s] = e[3]
        elif kind == "overlap":                                   # range, entries inside it, a range across its edge: call order
            first = int(rng.integers(max(n - 6, 1))); xf0, xf1 = rand_xf(rng), rand_xf(rng)
            a.update_geoms_xf(first, 6, xf0); apply_xf(mirror, first, min(6, n - first), xf0)
            inside = np.array([first + 1, first + 4], np.uint32)
            e = mirror[inside].copy(); e["flags"] = 0; e["xf"] = 0
            a.update_geoms(inside, e); mirror[inside] = e
            a.update_geoms_xf(first + 3, 3, xf1); apply_xf(mirror, first + 3, 3, xf1)
        else:                                                     # n == 0 and count == 0 are no-ops
            a.update_geoms(np.zeros(0, np.uint32), np.zeros(0, mirror.dtype)); a.update_geoms_xf(int(rng.integers(n)), 0, rand_xf(rng))
        if not same_table(a, mirror):
            table_diff.append((step, kind))
        if step % 10 == 9:
            a.render(W, H, clear=CLEAR, device_only=True)         # enqueued on the next of the three frame slots
            img = a.read_image(W, H)
            b.set_geoms(mirror)
            twin = b.render(W, H, clear=CLEAR)
            if not np.array_equal(img, twin):
                image_diff.append(step)
            d = int(np.abs(oracle_image(t, mirror).astype(np.int16) - img.astype(np.int16)).max())
            if d > 1:
                oracle_diff.append((step, d))
    cnt = a.counters()
    print("walk:", cnt, "kinds", sorted(seen))
    assert seen == set(kinds)
    assert table_diff == [], table_diff[:5]                       # read_geoms == the numpy mirror after every step, as uint32 words
    assert image_diff == [], image_diff[:5]                       # byte-identical to a context that got the mirror through set_geoms
    assert oracle_diff == [], oracle_diff[:5]                     # within one code value of the oracle
    assert cnt["table_edits"] > 250 and cnt["table_edit_bytes_h2d"] > 0
    a.close(); b.close()


# 2 --------------------------------------------------------------------------------------------------------------------
def _pan_tables(t, k):
    g = t["geoms"].copy()
    apply_xf(g, 0, len(g), (1.0, 0.0, 0.0, 1.0, 3.0 * (k + 1), -2.0 * (k + 1)))
    return g


def _enqueue_loop(t, route, frames=12, slots=3, versions=_pan_tables):
    c = new_ctx(t, frames_in_flight=slots)
    c.render(W, H, clear=CLEAR, device_only=True); c.sync()       # the first frame of a geometry learns N and J synchronously
    bufs = [np.zeros((H, W * 4), np.uint8) for _ in range(frames)]
    for bf in bufs:
        c.register_buffer(bf)
    c0 = c.counters()
    for k in range(frames):
        g = versions(t, k)
        if route == "set_geoms":
            c.set_geoms(g)
        elif route == "xf":
            c.update_geoms_xf(0, len(g), g["xf"][0])
        else:
            c.update_geoms(np.arange(len(g), dtype=np.uint32), g)
        c.render_enqueue(W, H, bufs[k], clear=CLEAR)
    c1 = c.counters()                                             # (before sync: what the loop itself did)
    c.sync()
    c2 = c.counters()
    for bf in bufs:
        c.unregister_buffer(bf)
    c.close()
    return bufs, c0, c1, c2


@pytest.mark.parametrize("route", ["xf", "entries"])
def test_frames_in_flight_keep_the_table_they_were_enqueued_with(route):
    t = base_tables()
    bufs, c0, c1, c2 = _enqueue_loop(t, route)
    ref = new_ctx(t)
    bad = []
    for k in range(12):
        ref.set_geoms(_pan_tables(t, k))
        if not np.array_equal(bufs[k], ref.render(W, H, clear=CLEAR)):
            bad.append(k)
    ref.close()
    print(route, "before:", c0, "after the loop:", c1, "after sync:", c2)
    assert bad == [], bad                                         # buffer k shows table version k, byte for byte
    assert c1["scene_drains"] == c0["scene_drains"]               # no edit settled a frame in flight
    assert c1["table_edits"] - c0["table_edits"] == 12
    assert c2["frames"] - c0["frames"] == 12
    # the same loop through set_geoms: every upload settles the frames enqueued before it
    bufs_s, s0, s1, _ = _enqueue_loop(t, "set_geoms")
    assert all(np.array_equal(p, q) for p, q in zip(bufs, bufs_s))
    print("set_geoms route:", s0, "->", s1)
    assert s1["scene_drains"] > s0["scene_drains"] and s1["table_edits"] == s0["table_edits"]    # (a slot's first frame is synchronous: nothing to settle behind it)


# 3 --------------------------------------------------------------------------------------------------------------------
def _zoom_tables(t, k):
    g = t["geoms"].copy()
    s = 1.0 if k < 6 else 1.5                                     # all layers grow by half in the middle of the sequence
    apply_xf(g, 0, len(g), (s, 0.0, 0.0, s, 2.0 * (k + 1), 0.0))
    return g


def test_a_frame_that_outgrows_its_predictions_is_rerun_like_after_set_geoms():
    t = base_tables()
    bufs_e, e0, _, e2 = _enqueue_loop(t, "xf", versions=_zoom_tables)
    bufs_s, s0, _, s2 = _enqueue_loop(t, "set_geoms", versions=_zoom_tables)
    print("edits:", e0, "->", e2, "set_geoms:", s0, "->", s2)
    bad = [k for k in range(12) if not np.array_equal(bufs_e[k], bufs_s[k])]
    assert bad == [], bad
    ref = new_ctx(t)
    for k in (5, 6, 11):
        ref.set_geoms(_zoom_tables(t, k))
        assert np.array_equal(bufs_e[k], ref.render(W, H, clear=CLEAR)), k
    ref.close()
    # same frames on the same slots under the same predictions: the same frames are voided and re-run, none learns anew
    assert e2["frames_rerun"] - e0["frames_rerun"] == s2["frames_rerun"] - s0["frames_rerun"]
    assert e2["frames_learned"] - e0["frames_learned"] == s2["frames_learned"] - s0["frames_learned"]


# 4 --------------------------------------------------------------------------------------------------------------------
def test_one_frame_slot_edit_then_render_timings_and_cache():
    t = base_tables()
    n = len(t["geoms"])
    a, b = new_ctx(t), new_ctx(t)
    mirror = t["geoms"].copy()
    rng = np.random.default_rng(5)
    assert np.array_equal(a.render(W, H, clear=CLEAR), b.render(W, H, clear=CLEAR))
    c0 = a.counters()
    for frame in range(6):
        xf = rand_xf(rng)
        if frame % 2:
            a.update_geoms_xf(0, n, xf); apply_xf(mirror, 0, n, xf)
        else:
            s = int(rng.integers(n)); e = mirror[[s]].copy(); e["flags"] = 1; e["xf"] = xf
            a.update_geoms([s], e); mirror[s] = e[0]
        b.set_geoms(mirror)
        if frame < 2:                                             # a plain frame into caller memory
            ia, ib = a.render(W, H, clear=CLEAR), b.render(W, H, clear=CLEAR)
        elif frame < 4:                                           # a frame with timings
            (ia, ta), (ib, tb) = a.render(W, H, clear=CLEAR, timings=True), b.render(W, H, clear=CLEAR, timings=True)
            assert ta["n_segments"] == tb["n_segments"] and ta["n_runs"] == tb["n_runs"]
        else:                                                     # a frame with a buffer-layer cache
            ia, ib = a.render(W, H, clear=CLEAR, cache_id=0), b.render(W, H, clear=CLEAR, cache_id=0)
        assert np.array_equal(ia, ib), frame
        assert same_table(a, mirror)
    c1 = a.counters()
    print("one slot:", c0, "->", c1)
    assert c1["table_edits"] - c0["table_edits"] == 6 and c1["scene_drains"] == c0["scene_drains"]
    # a single entry costs a record, not the table
    assert 0 < c1["table_edit_bytes_h2d"] - c0["table_edit_bytes_h2d"] < 6 * 32 * n
    a.close(); b.close()


# 5 --------------------------------------------------------------------------------------------------------------------
def test_edits_mix_with_the_other_scene_calls():
    from forma_amd import api
    t = base_tables()
    n = len(t["geoms"])
    rng = np.random.default_rng(6)
    a, b = new_ctx(t, frames_in_flight=3), new_ctx(t)
    mirror = t["geoms"].copy()

    def edit():
        xf = rand_xf(rng)
        first = int(rng.integers(len(mirror) - 1))
        a.update_geoms_xf(first, len(mirror) - first, xf); apply_xf(mirror, first, len(mirror) - first, xf)
        s = int(rng.integers(len(mirror))); e = mirror[[s]].copy(); e["flags"] = 1; e["xf"] = rand_xf(rng)
        a.update_geoms([s], e); mirror[s] = e[0]

    def check(what):
        assert same_table(a, mirror), what
        a.render(W, H, clear=CLEAR, device_only=True)
        b.set_geoms(mirror)
        assert np.array_equal(a.read_image(W, H), b.render(W, H, clear=CLEAR)), what

    edit(); check("edits")
    # set_geoms with another size after edits (two more slots, unused by the lines), then further edits — the new slots included
    bigger = np.zeros(n + 2, mirror.dtype); bigger[:n] = mirror; bigger["order"][n:] = NONE
    a.render(W, H, clear=CLEAR, device_only=True)                 # (a frame in flight when the table is replaced)
    a.set_geoms(bigger); mirror = bigger.copy()
    check("set_geoms after edits")
    edit(); tail_xf = rand_xf(rng)
    a.update_geoms_xf(n, 2, tail_xf); apply_xf(mirror, n, 2, tail_xf); check("edits after set_geoms")
    # geometry_append / _retain between edits
    tri = api.PathBuilder().move_to(api.Point(100, 100)).line_to(api.Point(300, 120)).line_to(api.Point(200, 330)).build()
    n_before = len(t["x"])
    for c in (a, b):
        c.geometry_append_paths([(tri, 1)])
    edit(); check("append between edits")
    for c in (a, b):
        c.geometry_retain([(0, n_before)], np.arange(len(mirror), dtype=np.uint32))
    edit(); check("retain between edits")
    # forma_hip_trim between edits
    edit(); a.trim(); edit(); check("trim between edits")
    # a stage entry point after an edit sees the edited table
    edit()
    b.set_geoms(mirror)
    la, lb = a.prepare_lines(W, H), b.prepare_lines(W, H)
    for k in la:
        assert np.array_equal(words(la[k]), words(lb[k])), k
    check("after prepare_lines")
    a.close(); b.close()


# 6 --------------------------------------------------------------------------------------------------------------------
def test_argument_errors_change_nothing():
    from forma_amd import FormaError
    t = base_tables()
    n = len(t["geoms"])
    c = new_ctx(t)
    ok = t["geoms"][[0]].copy(); ok["flags"] = 1; ok["xf"] = (1, 0, 0, 1, 5, 5)
    too_high = ok.copy(); too_high["order"] = LAYER_LIMIT + 1
    limit = ok.copy(); limit["order"] = LAYER_LIMIT
    two = np.concatenate((ok, ok))
    before = c.read_geoms()
    c.render(W, H, clear=CLEAR)
    xf = np.array((1, 0, 0, 1, 2, 2), np.float32)
    u32 = lambda v: np.array(v, np.uint32)
    bad_calls = {
        "a slot beyond n_geoms": lambda: c.update_geoms([n], ok),
        "a good record, then a slot beyond n_geoms": lambda: c.update_geoms([0, n + 7], two),
        "an order above LAYER_LIMIT": lambda: c.update_geoms([0], too_high),
        "a good record, then an order above LAYER_LIMIT": lambda: c.update_geoms([1, 0], np.concatenate((ok, too_high))),
        "a range that ends beyond n_geoms": lambda: c.update_geoms_xf(n - 1, 2, xf),
        "a range that starts beyond n_geoms": lambda: c.update_geoms_xf(n + 1, 1, xf),
        "a range that wraps around 2^32": lambda: c.update_geoms_xf(2, 0xFFFFFFFF, xf),
        "null slots": lambda: c._check(c._L.forma_hip_update_geoms(c._h, None, ok.ctypes.data_as(C.c_void_p), 1)),
        "null entries": lambda: c._check(c._L.forma_hip_update_geoms(c._h, u32([0]).ctypes.data_as(C.c_void_p), None, 1)),
        "null out_n": lambda: c._check(c._L.forma_hip_read_geoms(c._h, None, 0, None)),
    }
    for what, call in bad_calls.items():
        with pytest.raises(FormaError) as e:
            call()
        assert e.value.code == E_ARG, what
        assert np.array_equal(words(c.read_geoms()), words(before)), what
    cnt = c.counters()
    assert cnt["table_edits"] == 0
    # the limit itself and FORMA_NONE are orders like any other; null pointers with n == 0 are no-ops
    assert c._L.forma_hip_update_geoms(c._h, None, None, 0) == 0 and c._L.forma_hip_update_geoms_xf(c._h, n + 5, 0, None) == 0
    assert np.array_equal(words(c.read_geoms()), words(before))
    gone = ok.copy(); gone["order"] = NONE
    c.update_geoms([2, 3], np.concatenate((limit, gone)))
    after = before.copy(); after[2] = limit[0]; after[3] = gone[0]
    assert np.array_equal(words(c.read_geoms()), words(after))
    # a capacity that is too small reports the size
    got = C.c_size_t(0)
    assert c._L.forma_hip_read_geoms(c._h, None, 0, C.byref(got)) == -4 and got.value == n
    c.close()


# 7 --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["exchange", "bands"])
def test_emulated_devices_take_the_edits(layout):
    t = base_tables()
    n = len(t["geoms"])
    rng = np.random.default_rng(7)
    m = new_ctx(t, devices=[0, 0])
    m.set_layout(layout)
    one = new_ctx(t)
    mirror = t["geoms"].copy()
    assert np.array_equal(m.render(W, H, clear=CLEAR), one.render(W, H, clear=CLEAR))
    for step in range(8):
        if step % 2:
            xf = rand_xf(rng)
            for c in (m, one):
                c.update_geoms_xf(0, n, xf)
            apply_xf(mirror, 0, n, xf)
        else:
            slots = rng.choice(n, size=3, replace=False).astype(np.uint32)
            e = mirror[slots].copy(); e["flags"] = 1
            for i in range(3):
                e[i]["xf"] = rand_xf(rng)
            if step == 4:
                e["order"][0] = NONE
            for c in (m, one):
                c.update_geoms(slots, e)
            mirror[slots] = e
        assert same_table(m, mirror) and same_table(one, mirror), step
        assert np.array_equal(m.render(W, H, clear=CLEAR), one.render(W, H, clear=CLEAR)), step
    with pytest.raises(_fa().FormaError) as e:
        m.update_geoms_xf(n, 1, None)
    assert e.value.code == E_ARG and same_table(m, mirror)
    m.close(); one.close()


# 8 --------------------------------------------------------------------------------------------------------------------
def test_spaceship_through_resident_tables_equals_the_default_renderer():
    import torch
    from forma_amd import api, spaceship
    w, h = 640, 360
    clear = api.Color(0.1, 0.1, 0.2, 1.0)
    rr = api.Renderer(0, frames_in_flight=3, resident_geometry=True, resident_tables=True)
    rd = api.Renderer(0)
    comp = api.Composition()
    ship = spaceship.Spaceship(api, width=w, height=h, seed=43)
    outs, wants, moved_only, grew, drained = [], [], [], [], []
    for f in range(60):
        sh = comp._shared
        tv, xv = sh.table_version, sh.xf_version
        ship.compose(comp)
        only_xf = f > 0 and sh.table_version - tv == sh.xf_version - xv > 0
        c0 = rr.counters()
        out = torch.zeros((h, w, 4), dtype=torch.uint8, device=torch.device("cuda", 0))
        rr.render_to_device(comp, out, clear_color=clear)
        c1 = rr.counters()
        outs.append(out)
        img = np.zeros((h, w * 4), np.uint8)
        rd.render(comp, api.BufferBuilder(img, api.LinearLayout(w, w * 4, h)).build(), clear_color=clear)
        wants.append(img)
        assert np.array_equal(words(rr.host_tables["geoms"]), words(rd.host_tables["geoms"])), f
        if only_xf:
            moved_only.append(f)
            grew.append(c1["table_edits"] - c0["table_edits"])
            drained.append(c1["scene_drains"] - c0["scene_drains"])
    rr._ctx.sync()
    torch.cuda.synchronize()
    bad = [f for f in range(60) if not np.array_equal(outs[f].cpu().numpy().reshape(h, w * 4), wants[f])]
    print("spaceship:", rr.counters(), "frames with transforms only:", len(moved_only))
    assert bad == [], bad
    assert len(moved_only) >= 20                                  # once the first enemy is there, most frames only move the actors
    assert all(g == 1 for g in grew), list(zip(moved_only, grew))
    assert all(d == 0 for d in drained), list(zip(moved_only, drained))
    rr._ctx.close(); rd._ctx.close()


# 9 --------------------------------------------------------------------------------------------------------------------
def test_a_uniform_pan_through_the_renderer_matches_the_oracle():
    from forma_amd import api, scenes
    w, h = 640, 360
    comp = scenes.paris_like(n_layers=200, width=w, height=h, seed=11)
    rr, rd = api.Renderer(0, resident_tables=True), api.Renderer(0)
    c_start = None
    for f in range(10):
        if f:
            xf = api.GeomPresTransform.try_from([1, 0, 0, 1, 3.0 * f, -2.0 * f])
            for layer in comp.layers.values():
                layer.set_transform(xf)
        a = np.zeros((h, w * 4), np.uint8); b = np.zeros((h, w * 4), np.uint8)
        rr.render(comp, api.BufferBuilder(a, api.LinearLayout(w, w * 4, h)).build(), clear_color=api.Color(*CLEAR))
        rd.render(comp, api.BufferBuilder(b, api.LinearLayout(w, w * 4, h)).build(), clear_color=api.Color(*CLEAR))
        if f == 0:
            c_start = rr.counters()
        assert np.array_equal(a, b), f
        assert np.array_equal(words(rr.host_tables["geoms"]), words(rd.host_tables["geoms"])), f
        assert np.array_equal(words(rr._ctx.read_geoms()), words(rr.host_tables["geoms"])), f
        want = oracle_image(rd.host_tables, rd.host_tables["geoms"], w, h)
        assert int(np.abs(want.astype(np.int16) - a.astype(np.int16)).max()) <= 1, f
    c_end = rr.counters()
    print("pan:", c_start, "->", c_end)
    assert c_end["table_edits"] - c_start["table_edits"] == 9
    assert c_end["table_edit_bytes_h2d"] - c_start["table_edit_bytes_h2d"] == 9 * 48     # one range record per frame
    rr._ctx.close(); rd._ctx.close()


# 10 -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("slots", [1, 3])
def test_the_first_edit_call_on_a_large_table_renders_at_once(slots):
    """A table of 40 000 entries (1.25 MB: a copy of it takes tens of microseconds): the first edit call — which gives every
    frame slot its own table — is followed by a frame at once, with frames pending on the slots, and so is every edit after
    it.  Nothing a slot sends may still be on its way when the slot packs its next block."""
    t = base_tables()
    n, big_n = len(t["geoms"]), 40000
    big = np.zeros(big_n, t["geoms"].dtype); big["order"] = NONE; big[:n] = t["geoms"]
    a, b = new_ctx(t, frames_in_flight=slots), new_ctx(t)
    a.set_geoms(big); b.set_geoms(big)
    mirror = big.copy()
    for _ in range(2 * slots):                                    # every slot's learning frame, then one enqueued frame per slot: pending
        a.render(W, H, clear=CLEAR, device_only=True)
    c0 = a.counters()
    bad = []
    for k in range(8):
        xf = (1.0, 0.0, 0.0, 1.0, 2.0 * (k + 1), -1.0 * (k + 1))
        a.update_geoms_xf(0, big_n, xf); apply_xf(mirror, 0, big_n, xf)      # a range leaves the orders to what the slot holds
        if k == 4:                                                # ... and entries in between, the first slot among them
            e = mirror[[0, 3]].copy(); e["xf"][:, 4] += 7.0
            a.update_geoms([0, 3], e); mirror[[0, 3]] = e
        a.render(W, H, clear=CLEAR, device_only=True)             # at once: no read, no sync in between
        if k in (0, 1, 3, 7):
            img = a.read_image(W, H)
            b.set_geoms(mirror)
            if not np.array_equal(img, b.render(W, H, clear=CLEAR)):
                bad.append(k)
    c1 = a.counters()
    print("large table,", slots, "slots:", c0, "->", c1)
    assert bad == [], bad
    assert same_table(a, mirror)
    assert c1["scene_drains"] == c0["scene_drains"]
    # the device tables themselves, slot by slot: stage entry points read the owner's, which has caught up by then
    b.set_geoms(mirror)
    la, lb = a.prepare_lines(W, H), b.prepare_lines(W, H)
    assert all(np.array_equal(words(la[k]), words(lb[k])) for k in la)
    a.close(); b.close()
