"""CPU-only checks of the incremental geometry store (forma_hip_geometry_append / _retain / _read_geometry / _counters):
the boundary declares the same thing on all of its faces, and `Renderer(resident_geometry=True)` reconciles the device's
store with the composition's pushes at the cost of the difference — host logic, exercised with a recording context."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "forma_hip.h")
NEW = ["forma_hip_counters", "forma_hip_geometry_append", "forma_hip_geometry_retain", "forma_hip_read_geometry"]
NONE = 0xFFFFFFFF


def test_the_four_entry_points_are_declared_exported_and_named_by_the_shim():
    from forma_amd import _lib
    hdr = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    ffi = open(os.path.join(ROOT, "rust", "forma_hip", "ffi.rs")).read()
    L = C.CDLL(_lib.SO_PATH)
    for name in NEW:
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr), name + " is not declared in include/forma_hip.h"
        assert name in _lib.SYMBOLS, name + " is missing in the ctypes binding table"
        assert hasattr(L, name), name + " is not exported by libforma_hip.so"
        assert re.search(r"pub fn " + name + r"\b", ffi), name + " is missing in rust/forma_hip/ffi.rs"
    assert hasattr(L, "forma_host_batch_append")
    for struct, fields in (("forma_affine_range_t", ["first", "count", "m"]), ("forma_keep_range_t", ["first", "count"]),
                           ("forma_counters_t", [k for k, _ in _lib.CountersT._fields_])):
        r = re.search(r"pub struct " + struct + r"\s*\{(.*?)\n\}", ffi, flags=re.S)
        assert r, struct + " missing in ffi.rs"
        assert re.findall(r"pub (\w+)\s*:", r.group(1)) == fields, struct


def test_struct_layouts_match_the_ctypes_mirrors(tmp_path):
    from forma_amd import _lib
    gcc = shutil.which("gcc")
    if not gcc:
        pytest.skip("no gcc")
    mirrors = {"forma_counters_t": _lib.CountersT, "forma_affine_range_t": _lib.AffineRangeT, "forma_keep_range_t": _lib.KeepRangeT}
    lines = []
    for cname, mirror in mirrors.items():
        offs = "".join(f', offsetof({cname}, {f})' for f, _ in mirror._fields_)
        fmt = " ".join(["%zu"] * (1 + len(mirror._fields_)))
        lines.append(f'    printf("{cname} {fmt}\\n", sizeof({cname}){offs});')
    prog = tmp_path / "abi.c"
    prog.write_text("#include <stddef.h>\n#include <stdio.h>\n#include \"forma_hip.h\"\nint main(void) {\n" + "\n".join(lines) + "\n    return 0;\n}\n")
    exe = tmp_path / "abi"
    subprocess.run([gcc, "-std=c11", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)], check=True)
    out = dict(line.split(" ", 1) for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    for cname, mirror in mirrors.items():
        want = [C.sizeof(mirror)] + [getattr(mirror, f).offset for f, _ in mirror._fields_]
        assert [int(v) for v in out[cname].split()] == want, cname


# ---- reconciliation against a recording context -----------------------------------------------------------------------
class _FakeCtx:
    """Stands in for forma_amd.Context: records what the renderer asks of the geometry store, renders nothing."""
    def __init__(self):
        self.calls = []
        self._h = None

    def _check(self, rc): pass
    def set_geometry(self, x, y, ls): self.calls.append(("set_geometry", len(x)))
    def geometry_append_paths(self, items): self.calls.append(("append", list(items)))
    def geometry_retain(self, keep, remap): self.calls.append(("retain", [tuple(k) for k in keep], [int(v) for v in remap]))
    def set_geoms(self, g): self.geoms = np.array(g)
    def set_styles(self, *a): pass
    def set_images(self, *a): pass

    def render(self, w, h, **kw):
        return (None, {}) if kw.get("timings") else None

    def take(self):
        c, self.calls = self.calls, []
        return c


def _renderer(resident):
    from forma_amd import api
    r = api.Renderer.__new__(api.Renderer)
    r._ctx = _FakeCtx(); r._caches = set(); r._geom_owner = None; r._geom_version = None; r._slot_of = {}
    r.last_timings = {}; r.host_tables = {}; r._tables_key = None; r._marked_key = None
    r._resident = resident; r._dev_pushes = []; r._dev_points = []; r._dev_epoch = None
    return r


def _tri(api, x=1.0):
    return api.PathBuilder().move_to(api.Point(x, 1)).line_to(api.Point(x + 8, 1)).line_to(api.Point(x + 8, 9)).build()


def _buf(api):
    return api.BufferBuilder(np.zeros(64 * 64 * 4, np.uint8), api.LinearLayout(64, 256, 64)).build()


def _points(api, path):
    return int(api._host().forma_host_path_points(path._h))


def _scratch_slots(pushes):
    slot_of = {}
    for g, _, _ in pushes:
        slot_of.setdefault(g, len(slot_of))
    return slot_of


def test_one_more_insert_is_one_append_of_one_path():
    from forma_amd import api
    r = _renderer(True)
    comp = api.Composition()
    for o in range(1000):
        comp.get_mut_or_insert_default(api.Order(o)).insert(_tri(api, float(o % 50)))
    r.render(comp, _buf(api))
    first = r._ctx.take()
    assert [c[0] for c in first] == ["set_geometry", "append"] and first[0][1] == 0 and len(first[1][1]) == 1000
    r.render(comp, _buf(api))
    assert r._ctx.take() == []                                   # a static scene touches the store no more
    extra = _tri(api, 3.0)
    comp.get_mut_or_insert_default(api.Order(1000)).insert(extra)
    r.render(comp, _buf(api))
    calls = r._ctx.take()
    assert len(calls) == 1 and calls[0][0] == "append"
    assert len(calls[0][1]) == 1 and calls[0][1][0][0] is extra and calls[0][1][0][1] == 1000
    assert r._slot_of == _scratch_slots(comp._shared.pushes)
    # a second path into an existing layer reuses the layer's slot
    comp.get_mut(api.Order(7)).insert(extra)
    r.render(comp, _buf(api))
    calls = r._ctx.take()
    assert len(calls) == 1 and calls[0] == ("append", [(extra, 7)])
    assert "x" not in r.host_tables and "line_slot" not in r.host_tables and "geoms" in r.host_tables


def test_compaction_is_one_retain_numbered_like_a_fresh_upload():
    from forma_amd import api
    r = _renderer(True)
    comp = api.Composition()
    for o in range(10):
        comp.get_mut_or_insert_default(api.Order(o)).insert(_tri(api, float(o)))
    r.render(comp, _buf(api)); r._ctx.take()
    retains = 0
    for step in range(40):
        lay = comp.get_mut(api.Order(3 if step % 2 else 0))
        lay.clear(); lay.insert(_tri(api, 20.0 + step))
        before = list(comp._shared.pushes)                        # (the pushes still hold the one inserted just now)
        on_device = list(r._dev_pushes); old_slots = dict(r._slot_of)
        r.render(comp, _buf(api))
        calls = r._ctx.take()
        after = comp._shared.pushes
        assert r._slot_of == _scratch_slots(after), step          # always the numbering of a from-scratch upload
        assert r._dev_pushes == after and r._dev_points == [_points(api, p[1]) for p in after]
        geoms = r.host_tables["geoms"]
        assert len(geoms) == max(len(_scratch_slots(after)), 1)
        if len(after) == len(before):                             # no compaction: the pure append of the new push
            assert [c[0] for c in calls] == ["append"] and len(calls[0][1]) == 1, step
            continue
        retains += 1
        assert [c[0] for c in calls] == ["retain", "append"], step
        # what SegmentBuffer::retain must keep: the surviving pushes that were on the device, as merged point ranges
        survivors = {id(p) for p in after}
        want_keep, at = [], 0
        for p in on_device:
            n = _points(api, p[1])
            if id(p) in survivors:
                if want_keep and want_keep[-1][0] + want_keep[-1][1] == at:
                    want_keep[-1] = (want_keep[-1][0], want_keep[-1][1] + n)
                else:
                    want_keep.append((at, n))
            at += n
        fresh = _scratch_slots([p for p in on_device if id(p) in survivors])
        want_remap = [NONE] * len(old_slots)
        for g, old in old_slots.items():
            if g in fresh:
                want_remap[old] = fresh[g]
        assert calls[0][1] == want_keep and calls[0][2] == want_remap, step
        new = [p for p in after if not any(p is q for q in on_device)]
        assert [it[0] for it in calls[1][1]] == [p[1] for p in new]
    assert retains >= 2


def test_another_composition_in_between_takes_the_full_path():
    from forma_amd import api
    r = _renderer(True)
    a, b = api.Composition(), api.Composition()
    for o in range(5):
        a.get_mut_or_insert_default(api.Order(o)).insert(_tri(api, float(o)))
    b.get_mut_or_insert_default(api.Order(0)).insert(_tri(api))
    r.render(a, _buf(api)); r._ctx.take()
    r.render(b, _buf(api))
    calls = r._ctx.take()
    assert [c[0] for c in calls] == ["set_geometry", "append"] and len(calls[1][1]) == 1
    a.get_mut_or_insert_default(api.Order(5)).insert(_tri(api))
    r.render(a, _buf(api))
    calls = r._ctx.take()
    assert [c[0] for c in calls] == ["set_geometry", "append"] and len(calls[1][1]) == 6
    assert r._slot_of == _scratch_slots(a._shared.pushes)


def test_the_default_mode_replaces_the_store_as_before():
    from forma_amd import api
    r = _renderer(False)
    comp = api.Composition()
    for o in range(5):
        comp.get_mut_or_insert_default(api.Order(o)).insert(_tri(api, float(o)))
    r.render(comp, _buf(api))
    comp.get_mut_or_insert_default(api.Order(5)).insert(_tri(api))
    r.render(comp, _buf(api))
    calls = r._ctx.take()
    assert [c[0] for c in calls] == ["set_geometry", "set_geometry"] and calls[1][1] > calls[0][1] > 0
    assert all(k in r.host_tables for k in ("x", "y", "line_slot", "geoms"))
    assert api.Renderer.__init__.__defaults__[-1] is False       # resident_geometry is opt-in
