"""CPU-only checks of the layer table edited with frames in flight (forma_hip_update_geoms / _update_geoms_xf / _read_geoms):
the boundary declares the same thing on all of its faces, and `Renderer(resident_tables=True)` sends exactly the entries that
Layer.set_transform / set_is_enabled touched — host logic, exercised with a recording context."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "forma_hip.h")
NEW = ["forma_hip_update_geoms", "forma_hip_update_geoms_xf", "forma_hip_read_geoms"]
NEW_COUNTERS = ["table_edits", "table_edit_bytes_h2d", "scene_drains"]
NONE = 0xFFFFFFFF


def test_the_entry_points_are_declared_exported_bound_and_named_by_the_shim():
    from forma_amd import _lib
    hdr = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    ffi = open(os.path.join(ROOT, "rust", "forma_hip", "ffi.rs")).read()
    L = C.CDLL(_lib.SO_PATH)
    for name in NEW:
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr), name + " is not declared in include/forma_hip.h"
        assert name in _lib.SYMBOLS, name + " is missing in the ctypes binding table"
        assert hasattr(L, name), name + " is not exported by libforma_hip.so"
        assert re.search(r"pub fn " + name + r"\b", ffi), name + " is missing in rust/forma_hip/ffi.rs"
    # argument counts: header, ctypes table and ffi.rs agree
    for name in NEW:
        n_hdr = re.search(r"\bint\s+" + name + r"\s*\((.*?)\)\s*;", hdr, flags=re.S).group(1).count(",") + 1
        n_ffi = re.search(r"pub fn " + name + r"\s*\((.*?)\)\s*->", ffi, flags=re.S).group(1).strip().rstrip(",").count(",") + 1
        assert n_hdr == len(_lib.SYMBOLS[name][1]) == n_ffi, name
    from forma_amd.context import Context
    for m in ("update_geoms", "update_geoms_xf", "read_geoms"):
        assert callable(getattr(Context, m))
    shim = open(os.path.join(ROOT, "rust", "forma_hip", "mod.rs")).read()
    assert "forma_hip_update_geoms" in shim                      # the shim's set_transform path names the edit call


def test_the_counters_grew_at_their_end_on_every_face():
    from forma_amd import _lib
    fields = [k for k, _ in _lib.CountersT._fields_]
    assert fields[-3:] == NEW_COUNTERS and fields[8] == "frames_rerun"
    hdr = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    body = re.search(r"typedef struct forma_counters_t\s*\{(.*?)\}\s*forma_counters_t;", hdr, flags=re.S).group(1)
    names = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            assert decl.startswith("uint64_t"), decl
            names += [n.strip() for n in decl[len("uint64_t"):].split(",")]
    assert names == fields
    ffi = open(os.path.join(ROOT, "rust", "forma_hip", "ffi.rs")).read()
    r = re.search(r"pub struct forma_counters_t\s*\{(.*?)\n\}", ffi, flags=re.S)
    assert re.findall(r"pub (\w+)\s*:\s*u64", r.group(1)) == fields
    assert C.sizeof(_lib.CountersT) == 8 * len(fields)


def test_the_counters_layout_matches_the_compiler(tmp_path):
    from forma_amd import _lib
    gcc = shutil.which("gcc")
    if not gcc:
        pytest.skip("no gcc")
    fields = [k for k, _ in _lib.CountersT._fields_]
    offs = "".join(f", offsetof(forma_counters_t, {f})" for f in fields)
    prog = tmp_path / "abi.c"
    prog.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "forma_hip.h"\nint main(void) {\n'
                    f'    printf("{" ".join(["%zu"] * (1 + len(fields)))}\\n", sizeof(forma_counters_t){offs});\n    return 0;\n}}\n')
    exe = tmp_path / "abi"
    flags = ["-std=c11", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include")]
    subprocess.run([gcc] + flags + [str(prog), "-o", str(exe)], check=True)
    # the prototypes, as a C compiler reads them (compiled, not linked)
    proto = tmp_path / "proto.c"
    proto.write_text('#include "forma_hip.h"\n'
                     'int (*const a)(forma_hip_ctx*, const uint32_t*, const forma_geom_t*, size_t) = forma_hip_update_geoms;\n'
                     'int (*const b)(forma_hip_ctx*, uint32_t, uint32_t, const float*) = forma_hip_update_geoms_xf;\n'
                     'int (*const c)(forma_hip_ctx*, forma_geom_t*, size_t, size_t*) = forma_hip_read_geoms;\n')
    subprocess.run([gcc] + flags + ["-c", str(proto), "-o", str(tmp_path / "proto.o")], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [C.sizeof(_lib.CountersT)] + [getattr(_lib.CountersT, f).offset for f in fields]


# ---- Renderer(resident_tables=True) against a recording context ---------------------------------------------------------
class _FakeCtx:
    """Stands in for forma_amd.Context: records what the renderer asks of the layer table, renders nothing."""
    def __init__(self):
        self.calls = []
        self._h = None

    def _check(self, rc): pass
    def set_geometry(self, *a): pass
    def set_geoms(self, g): self.calls.append(("set_geoms", np.array(g)))
    def update_geoms(self, slots, entries): self.calls.append(("update_geoms", [int(s) for s in slots], np.array(entries)))
    def update_geoms_xf(self, first, count, xf): self.calls.append(("update_geoms_xf", int(first), int(count), None if xf is None else [float(v) for v in xf]))
    def set_styles(self, *a): self.calls.append(("set_styles",))
    def set_images(self, *a): pass

    def render(self, w, h, **kw):
        return (None, {}) if kw.get("timings") else None

    def take(self):
        c, self.calls = self.calls, []
        return c


def _renderer(resident_tables):
    from forma_amd import api
    r = api.Renderer.__new__(api.Renderer)
    r._ctx = _FakeCtx(); r._caches = set(); r._geom_owner = None; r._geom_version = -1; r._slot_of = {}
    r.last_timings = {}; r.host_tables = {}; r._tables_key = None; r._marked_key = None
    if resident_tables is not None:                               # (None: a renderer made the way older tests make it, without the attribute)
        r._resident_tables = resident_tables
    def upload_geometry(comp):
        r._geom_owner = comp._shared; r._geom_version = comp._shared.geometry_version
        slot_of = {}
        for g, _, _ in comp._shared.pushes:
            slot_of.setdefault(g, len(slot_of))
        r._slot_of = slot_of
    r._upload_geometry = upload_geometry
    return r


def _tri(api, x=1.0):
    return api.PathBuilder().move_to(api.Point(x, 1)).line_to(api.Point(x + 8, 1)).line_to(api.Point(x + 8, 9)).build()


def _buf(api, cache=None):
    b = api.BufferBuilder(np.zeros(64 * 64 * 4, np.uint8), api.LinearLayout(64, 256, 64))
    return b.layer_cache(cache).build() if cache else b.build()


def _comp(api, n=8):
    comp = api.Composition()
    for o in range(n):
        comp.get_mut_or_insert_default(api.Order(o)).insert(_tri(api, float(o)))
    return comp


def _xf(api, tx, ty=0.0, s=1.0):
    return api.GeomPresTransform.try_from([s, 0, 0, s, tx, ty])


def _full_geoms(api, r, comp):
    """host_tables["geoms"] as _upload_tables builds it for the composition as it is now, from a renderer of the default kind"""
    d = _renderer(False)
    d._slot_of = dict(r._slot_of); d._geom_owner = comp._shared; d._geom_version = comp._shared.geometry_version
    d._upload_tables(comp, None)
    return d.host_tables["geoms"]


def _same(a, b):
    return a.dtype == b.dtype and len(a) == len(b) and np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def test_transform_and_enable_edits_send_exactly_the_dirty_slots():
    from forma_amd import api
    r = _renderer(True)
    comp = _comp(api)
    r.render(comp, _buf(api))
    first = r._ctx.take()
    assert [c[0] for c in first] == ["set_geoms", "set_styles"]
    r.render(comp, _buf(api))
    assert r._ctx.take() == []                                    # a static scene sends nothing
    comp.get_mut(api.Order(2)).set_transform(_xf(api, 3.0))
    comp.get_mut(api.Order(5)).set_transform(_xf(api, -1.0, 2.0))
    comp.get_mut(api.Order(5)).set_transform(_xf(api, -2.0, 2.0))    # the same layer twice: one entry, the last value
    comp.get_mut(api.Order(6)).disable()
    r.render(comp, _buf(api))
    calls = r._ctx.take()
    assert len(calls) == 1 and calls[0][0] == "update_geoms", calls
    assert calls[0][1] == [2, 5, 6]
    e = calls[0][2]
    assert list(e["order"]) == [2, 5, NONE] and list(e["flags"]) == [1, 1, 0]
    assert list(e["xf"][1]) == [1, 0, 0, 1, -2, 2]
    assert _same(r.host_tables["geoms"], _full_geoms(api, r, comp))
    # back to identity and enabled again: still entry edits, and the table still equals the full build
    comp.get_mut(api.Order(2)).set_transform(api.GeomPresTransform())
    comp.get_mut(api.Order(6)).enable()
    r.render(comp, _buf(api))
    calls = r._ctx.take()
    assert len(calls) == 1 and calls[0][0] == "update_geoms" and calls[0][1] == [2, 6]
    assert list(calls[0][2]["flags"]) == [0, 0] and list(calls[0][2]["order"]) == [2, 6]
    assert _same(r.host_tables["geoms"], _full_geoms(api, r, comp))
    comp.get_mut(api.Order(2)).set_transform(api.GeomPresTransform())   # same value: not a change
    r.render(comp, _buf(api))
    assert r._ctx.take() == []


def test_a_uniform_pan_is_one_update_geoms_xf():
    from forma_amd import api
    r = _renderer(True)
    comp = _comp(api)
    r.render(comp, _buf(api)); r._ctx.take()
    for frame in range(1, 4):
        for layer in comp.layers.values():
            layer.set_transform(_xf(api, 2.0 * frame, 1.0))
        r.render(comp, _buf(api))
        calls = r._ctx.take()
        assert calls == [("update_geoms_xf", 0, 8, [1.0, 0.0, 0.0, 1.0, 2.0 * frame, 1.0])], calls
        assert _same(r.host_tables["geoms"], _full_geoms(api, r, comp))
    # some of the slots with one transform, or all of them with two: entries
    for o in (3, 4, 5):
        comp.get_mut(api.Order(o)).set_transform(_xf(api, 9.0))
    r.render(comp, _buf(api))
    calls = r._ctx.take()
    assert [c[0] for c in calls] == ["update_geoms"] and calls[0][1] == [3, 4, 5]
    for o, layer in comp.layers.items():
        layer.set_transform(_xf(api, 1.0 if o < 4 else 2.0))
    r.render(comp, _buf(api))
    calls = r._ctx.take()
    assert [c[0] for c in calls] == ["update_geoms"] and calls[0][1] == list(range(8))
    # a pan that also switches a layer off changes an order: entries, not a range
    for layer in comp.layers.values():
        layer.set_transform(_xf(api, 30.0))
    comp.get_mut(api.Order(0)).disable()
    r.render(comp, _buf(api))
    calls = r._ctx.take()
    assert [c[0] for c in calls] == ["update_geoms"] and calls[0][1] == list(range(8))
    assert _same(r.host_tables["geoms"], _full_geoms(api, r, comp))


def test_everything_else_takes_the_full_path():
    from forma_amd import api
    r = _renderer(True)
    comp = _comp(api)
    r.render(comp, _buf(api)); r._ctx.take()

    def full_after(change):
        change()
        r.render(comp, _buf(api))
        calls = r._ctx.take()
        assert [c[0] for c in calls] == ["set_geoms", "set_styles"], calls
        assert _same(r.host_tables["geoms"], _full_geoms(api, r, comp))

    # a style change, alone and together with a transform
    full_after(lambda: comp.get_mut(api.Order(1)).set_props(api.Props(fill_rule=api.FillRule.EvenOdd)))
    full_after(lambda: (comp.get_mut(api.Order(1)).set_transform(_xf(api, 1.0)),
                        comp.get_mut(api.Order(2)).set_props(api.Props(fill_rule=api.FillRule.EvenOdd))))
    # insert (a new order, a second path) and remove
    full_after(lambda: comp.get_mut_or_insert_default(api.Order(8)).insert(_tri(api)))
    full_after(lambda: (comp.get_mut(api.Order(3)).insert(_tri(api, 4.0)), comp.get_mut(api.Order(3)).set_transform(_xf(api, 2.0))))
    full_after(lambda: comp.remove(api.Order(4)))
    # ... after which transform edits are edits again
    comp.get_mut(api.Order(0)).set_transform(_xf(api, 5.0))
    r.render(comp, _buf(api))
    assert [c[0] for c in r._ctx.take()] == ["update_geoms"]
    # a frame with a buffer-layer cache, and the cache-less frame after it
    cache = api.BufferLayerCache(0, r)
    comp.get_mut(api.Order(0)).set_transform(_xf(api, 6.0))
    r.render(comp, _buf(api, cache))
    assert [c[0] for c in r._ctx.take()] == ["set_geoms", "set_styles"]
    comp.get_mut(api.Order(0)).set_transform(_xf(api, 7.0))
    r.render(comp, _buf(api))
    assert [c[0] for c in r._ctx.take()] == ["set_geoms", "set_styles"]
    comp.get_mut(api.Order(0)).set_transform(_xf(api, 8.0))
    r.render(comp, _buf(api))
    assert [c[0] for c in r._ctx.take()] == ["update_geoms"]
    # another composition in between
    other = _comp(api, 3)
    r.render(other, _buf(api)); r._ctx.take()
    comp.get_mut(api.Order(0)).set_transform(_xf(api, 9.0))
    r.render(comp, _buf(api))
    assert [c[0] for c in r._ctx.take()] == ["set_geoms", "set_styles"]
    assert _same(r.host_tables["geoms"], _full_geoms(api, r, comp))


@pytest.mark.parametrize("kind", [False, None])
def test_the_default_renderer_uploads_whole_tables_as_before(kind):
    from forma_amd import api
    r = _renderer(kind)
    comp = _comp(api)
    r.render(comp, _buf(api)); r._ctx.take()
    comp.get_mut(api.Order(2)).set_transform(_xf(api, 3.0))
    r.render(comp, _buf(api))
    assert [c[0] for c in r._ctx.take()] == ["set_geoms", "set_styles"]
    for layer in comp.layers.values():
        layer.set_transform(_xf(api, 4.0))
    r.render(comp, _buf(api))
    assert [c[0] for c in r._ctx.take()] == ["set_geoms", "set_styles"]
    assert api.Renderer.__init__.__defaults__[-1] is False       # resident_tables is opt-in


def test_a_long_history_of_moves_falls_back_to_the_full_path_once():
    """the composition keeps the layers of the last moves only: a renderer that has not drawn for longer than that rebuilds"""
    from forma_amd import api
    r = _renderer(True)
    comp = _comp(api, 2)
    r.render(comp, _buf(api)); r._ctx.take()
    lay = comp.get_mut(api.Order(0))
    for i in range((1 << 16) + 10):
        lay.set_transform(_xf(api, float(i + 1)))
    assert comp._shared.xf_log_base > 0
    r.render(comp, _buf(api))
    assert [c[0] for c in r._ctx.take()] == ["set_geoms", "set_styles"]
    lay.set_transform(_xf(api, -1.0))
    r.render(comp, _buf(api))
    assert [c[0] for c in r._ctx.take()] == ["update_geoms"]
