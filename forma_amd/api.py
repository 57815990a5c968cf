"""Python face of forma's public API for the MI355X backend — same names, argument meaning and
error behaviour as the reference (`forma::prelude`, reference forma/src/lib.rs:117-154):

    PathBuilder / Path / Point            forma/src/path.rs:773-925, math/point.rs
    Order, Color, FillRule, BlendMode, GradientBuilder, Gradient, GradientType, Image, Texture,
    Fill, Style, Func, Props              forma/src/styling.rs, utils/order.rs
    GeomPresTransform, AffineTransform    forma/src/math/transform.rs
    Composition / Layer                   forma/src/composition/{mod,layer}.rs
    hip.Renderer  (drop-in for cpu::Renderer: new / create_buffer_layer_cache / render,
                   forma/src/cpu/renderer.rs:61-224), BufferBuilder, LinearLayout, RGBA.., Rect

Path construction and the sequential half of curve flattening run in the C++ host library
(csrc/host_path.cpp); everything per-frame runs in HIP kernels behind the C ABI.  There is no CPU
fallback and no dependency on oracle/.
"""
from __future__ import annotations

import ctypes as C
import math
import struct
import weakref
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import _lib
from ._lib import FormaError
from .context import Context, GEOM_DTYPE, IMAGE_DTYPE

LAYER_LIMIT = (1 << 21) - 1          # consts.rs:107-109
LINES_GARBAGE_THRESHOLD = 2          # composition/mod.rs:33
MAX_WIDTH, MAX_HEIGHT = 1 << 16, 1 << 15
NONE = 0xFFFFFFFF

_host_bound = False


def _host():
    global _host_bound
    L = _lib.lib()
    if not _host_bound:
        vp, f, sz = C.c_void_p, C.c_float, C.c_size_t
        L.forma_host_builder_new.restype = vp
        L.forma_host_builder_free.argtypes = [vp]
        L.forma_host_move_to.argtypes = [vp, f, f]
        L.forma_host_line_to.argtypes = [vp, f, f]
        L.forma_host_quad_to.argtypes = [vp, f, f, f, f]
        L.forma_host_cubic_to.argtypes = [vp, f, f, f, f, f, f]
        L.forma_host_rat_quad_to.argtypes = [vp, f, f, f, f, f]
        L.forma_host_rat_cubic_to.argtypes = [vp, f, f, f, f, f, f, f, f]
        L.forma_host_build.argtypes = [vp]; L.forma_host_build.restype = vp
        L.forma_host_path_free.argtypes = [vp]
        L.forma_host_path_transform.argtypes = [vp, vp]; L.forma_host_path_transform.restype = vp
        L.forma_host_path_points.argtypes = [vp]; L.forma_host_path_points.restype = sz
        L.forma_host_path_lines.argtypes = [vp]; L.forma_host_path_lines.restype = sz
        L.forma_host_batch_new.restype = vp
        L.forma_host_batch_free.argtypes = [vp]
        L.forma_host_batch_add.argtypes = [vp, vp, C.c_uint32]
        L.forma_host_batch_points.argtypes = [vp]; L.forma_host_batch_points.restype = sz
        L.forma_host_batch_flatten.argtypes = [vp, vp, vp, vp, vp]; L.forma_host_batch_flatten.restype = C.c_int
        L.forma_host_batch_tables.argtypes = [vp, vp]
        if hasattr(L, "forma_host_path_stroke"):          # (as below: absent in an older build)
            L.forma_host_builder_open_contours.argtypes = [vp, C.c_int]
            L.forma_host_close.argtypes = [vp]
            L.forma_host_path_stroke.argtypes = [vp, f, f, C.c_uint32, C.c_uint32]; L.forma_host_path_stroke.restype = vp
            L.forma_host_path_is_stroked.argtypes = [vp]; L.forma_host_path_is_stroked.restype = C.c_int
            L.forma_host_batch_append_stroked.argtypes = [vp, vp, vp]; L.forma_host_batch_append_stroked.restype = C.c_int
            L.forma_host_batch_strokes.argtypes = [vp]; L.forma_host_batch_strokes.restype = sz
        if hasattr(L, "forma_host_batch_append"):         # (absent in an older build loaded through FORMA_HIP_LIB: tools' A/B runs)
            L.forma_host_batch_append.argtypes = [vp, vp]; L.forma_host_batch_append.restype = C.c_int
        _host_bound = True
    return L


# ---- math ---------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Point:
    x: float
    y: float


@dataclass(frozen=True)
class AffineTransform:                       # math/transform.rs:22-57
    ux: float = 1.0
    uy: float = 0.0
    vx: float = 0.0
    vy: float = 1.0
    tx: float = 0.0
    ty: float = 0.0

    def to_array(self):
        return [self.ux, self.uy, self.vx, self.vy, self.tx, self.ty]

    def transform(self, p: "Point") -> "Point":        # math/transform.rs:43-48 (f32, fused multiply-adds)
        f = np.float32
        def fma(a, b, c):                               # exact for f32 operands: the product of two f32 fits an f64
            return f(np.float64(f(a)) * np.float64(f(b)) + np.float64(f(c)))
        return Point(float(fma(self.ux, p.x, fma(self.vx, p.y, self.tx))), float(fma(self.uy, p.x, fma(self.vy, p.y, self.ty))))


class GeomPresTransformError(ValueError):
    pass


class GeomPresTransform:
    """Affine transform that does not scale geometry up (math/transform.rs:151-222)."""

    def __init__(self, t: AffineTransform = AffineTransform()):
        self.t = t

    @staticmethod
    def try_from(a: Sequence[float]) -> "GeomPresTransform":   # [ux, vx, uy, vy, tx, ty], transform.rs:80-91
        f = [float(np.float32(v)) for v in a]
        t = AffineTransform(ux=f[0], uy=f[2], vx=f[1], vy=f[3], tx=f[4], ty=f[5])
        max_x = np.float32(1.0) + np.float32(1.0 / 16.0) / np.float32(MAX_WIDTH)
        max_y = np.float32(1.0) + np.float32(1.0 / 16.0) / np.float32(MAX_HEIGHT)
        sx = np.float32(t.ux) * np.float32(t.ux) + np.float32(t.uy) * np.float32(t.uy) > max_x
        sy = np.float32(t.vx) * np.float32(t.vx) + np.float32(t.vy) * np.float32(t.vy) > max_y
        if sx or sy:
            raise GeomPresTransformError(f"exceeded scaling factor (x: {bool(sx)}, y: {bool(sy)})")
        return GeomPresTransform(t)

    def is_identity(self) -> bool:
        return self.t == AffineTransform()

    def transform(self, p: "Point") -> "Point":
        return self.t.transform(p)

    def to_array(self):
        t = self.t
        return [t.ux, t.vx, t.uy, t.vy, t.tx, t.ty]


# ---- paths ----------------------------------------------------------------------------------------
class StrokeJoin:
    Bevel = 0; Miter = 1; Round = 2


class StrokeCap:
    Butt = 0; Square = 1; Round = 2


@dataclass(frozen=True)
class StrokeStyle:
    """How `Path.stroke` outlines a path (no reference counterpart: forma only fills).  `width` is the full width, in the units
    of the path as it is when it is stroked; a miter join whose 1 / cos(turn / 2) exceeds `miter_limit` becomes a bevel."""
    width: float
    join: int = StrokeJoin.Miter
    cap: int = StrokeCap.Butt
    miter_limit: float = 4.0

    def __post_init__(self):
        if not (math.isfinite(self.width) and 0.0 < self.width <= 131072.0):
            raise ValueError("stroke width must be finite, > 0 and <= 131072")
        if not (math.isfinite(self.miter_limit) and self.miter_limit >= 1.0):
            raise ValueError("miter_limit must be finite and >= 1")
        if self.join not in (0, 1, 2) or self.cap not in (0, 1, 2):
            raise ValueError("unknown join or cap")


class Path:
    def __init__(self, handle, stroke_of: Optional["Path"] = None, style: Optional[StrokeStyle] = None):
        self._h = handle
        self._stroke_of = stroke_of          # a stroked path: the path it outlines ...
        self.stroke_style = style            # ... and how

    def __del__(self):
        try:
            _host().forma_host_path_free(self._h)
        except Exception:
            pass

    def stroke(self, style: StrokeStyle) -> "Path":
        """The outline of this path as a path of its own: inserted into a layer, its flattened points are expanded on the
        device into closed pieces (bodies, joins, caps) whose union under FillRule.NonZero is the stroke — EvenOdd is wrong
        for it.  Contours are closed only where the path closes them (`PathBuilder(open_contours=True)`, `close()`); dashes
        do not exist; a contour without a line of non-zero length (a dot) draws nothing.  A stroked path is terminal:
        transform first, then stroke."""
        if self._stroke_of is not None:
            raise ValueError("a stroked path cannot be stroked again")
        h = _host().forma_host_path_stroke(self._h, float(style.width) * 0.5, float(style.miter_limit), int(style.join), int(style.cap))
        return Path(h, stroke_of=self, style=style)

    def transform(self, t9: Sequence[float]) -> "Path":           # path.rs:725-771
        if self._stroke_of is not None:
            raise ValueError("a stroked path is terminal: transform the path first, then stroke it")
        t = np.ascontiguousarray(t9, np.float32)
        assert t.size == 9
        return Path(_host().forma_host_path_transform(self._h, t.ctypes.data))


class PathBuilder:
    def __init__(self, open_contours: bool = False):
        """`open_contours`: neither `move_to` nor `build` closes a contour with an implicit line (the default does, as the
        reference: a fill needs it); `close()` closes the current contour with a real line.  What a stroke wants."""
        self._h = _host().forma_host_builder_new()
        if open_contours:
            _host().forma_host_builder_open_contours(self._h, 1)

    def close(self):
        _host().forma_host_close(self._h); return self

    def __del__(self):
        try:
            _host().forma_host_builder_free(self._h)
        except Exception:
            pass

    def move_to(self, p: Point):
        _host().forma_host_move_to(self._h, p.x, p.y); return self

    def line_to(self, p: Point):
        _host().forma_host_line_to(self._h, p.x, p.y); return self

    def quad_to(self, p1: Point, p2: Point):
        _host().forma_host_quad_to(self._h, p1.x, p1.y, p2.x, p2.y); return self

    def cubic_to(self, p1: Point, p2: Point, p3: Point):
        _host().forma_host_cubic_to(self._h, p1.x, p1.y, p2.x, p2.y, p3.x, p3.y); return self

    def rat_quad_to(self, p1: Point, p2: Point, weight: float):
        _host().forma_host_rat_quad_to(self._h, p1.x, p1.y, p2.x, p2.y, weight); return self

    def rat_cubic_to(self, p1: Point, p2: Point, p3: Point, w1: float, w2: float):
        _host().forma_host_rat_cubic_to(self._h, p1.x, p1.y, p2.x, p2.y, p3.x, p3.y, w1, w2); return self

    def build(self) -> Path:
        return Path(_host().forma_host_build(self._h))


# ---- styling (forma/src/styling.rs) --------------------------------------------------------------
class OrderError(ValueError):
    pass


class Order(int):
    MAX = LAYER_LIMIT

    def __new__(cls, v: int):
        if v < 0 or v > LAYER_LIMIT:
            raise OrderError(f"exceeded layer limit ({LAYER_LIMIT})")        # utils/order.rs:27-31
        return super().__new__(cls, v)

    @staticmethod
    def new(v: int) -> "Order":
        return Order(v)

    def as_u32(self) -> int:
        return int(self)


@dataclass(frozen=True)
class Color:
    r: float = 0.0
    g: float = 0.0
    b: float = 0.0
    a: float = 1.0


class FillRule:
    NonZero = "NonZero"
    EvenOdd = "EvenOdd"


class GradientType:
    Linear = "Linear"
    Radial = "Radial"


BLEND_MODES = ["Over", "Multiply", "Screen", "Overlay", "Darken", "Lighten", "ColorDodge", "ColorBurn", "HardLight",
               "SoftLight", "Difference", "Exclusion", "Hue", "Saturation", "Color", "Luminosity"]


class BlendMode:
    pass


for _i, _n in enumerate(BLEND_MODES):
    setattr(BlendMode, _n, _n)


@dataclass(frozen=True)
class Gradient:
    type: str
    start: Point
    end: Point
    stops: Tuple[Tuple[Color, float], ...]


class GradientBuilder:                        # styling.rs:80-134
    def __init__(self, start: Point, end: Point):
        self._type = GradientType.Linear
        self._start, self._end = start, end
        self._stops: List[Tuple[Color, Optional[float]]] = []

    def type(self, t):
        self._type = t; return self

    def color(self, color: Color):
        self._stops.append((color, None)); return self

    def color_with_stop(self, color: Color, stop: float):
        if not (0.0 <= stop <= 1.0):
            raise ValueError("gradient stops must be between 0.0 and 1.0")
        self._stops.append((color, stop)); return self

    def build(self) -> Optional[Gradient]:
        if len(self._stops) < 2:
            return None
        inc = np.float32(1.0) / np.float32(len(self._stops) - 1)
        stops = tuple((c, float(np.float32(i) * inc) if s is None else float(np.float32(s))) for i, (c, s) in enumerate(self._stops))
        return Gradient(self._type, self._start, self._end, stops)


class ImageError(ValueError):
    pass


def _to_linear(l8: np.ndarray) -> np.ndarray:                 # styling.rs:252-259 (powf = libm powf)
    l = l8.astype(np.float32) * (np.float32(1.0) / np.float32(255.0))
    lo = l * (np.float32(1.0) / np.float32(12.92))
    hi = np.power((l + np.float32(0.055)) * (np.float32(1.0) / np.float32(1.055)), np.float32(2.4), dtype=np.float32)
    return np.where(l <= np.float32(0.04045), lo, hi).astype(np.float32)


def _to_f16(v: np.ndarray) -> np.ndarray:                     # bias-shifted half, styling.rs:242-250
    b = np.ascontiguousarray(v, np.float32).view(np.uint32)
    return np.where(v != 0, ((b - np.uint32(0x38000000)) >> np.uint32(13)) & np.uint32(0xFFFF), 0).astype(np.uint16)


class Image:
    _next_id = 0

    def __init__(self, texels: np.ndarray, width: int, height: int):
        if width * height != len(texels):
            raise ImageError(f"buffer has {len(texels)} pixels, which does not match the specified width ({width}) and height ({height})")
        self.texels, self.width_, self.height_ = texels, width, height
        self.id = Image._next_id; Image._next_id += 1

    @staticmethod
    def from_srgba(data, width: int, height: int) -> "Image":
        d = np.asarray(data, np.uint8).reshape(-1, 4)
        lin = np.empty(d.shape, np.float32)
        lin[:, :3] = _to_linear(d[:, :3])
        lin[:, 3] = d[:, 3].astype(np.float32) * (np.float32(1.0) / np.float32(255.0))
        return Image(_to_f16(lin), width, height)

    @staticmethod
    def from_linear_rgba(data, width: int, height: int) -> "Image":
        return Image(_to_f16(np.asarray(data, np.float32).reshape(-1, 4)), width, height)

    def width(self):
        return self.width_

    def height(self):
        return self.height_


@dataclass(frozen=True)
class Texture:
    transform: AffineTransform
    image: Image


class Fill:
    @staticmethod
    def Solid(color: Color):
        return ("solid", color)

    @staticmethod
    def Gradient(g: Gradient):
        return ("gradient", g)

    @staticmethod
    def Texture(t: Texture):
        return ("texture", t)


@dataclass(frozen=True)
class Style:
    is_clipped: bool = False
    fill: tuple = ("solid", Color())
    blend_mode: str = "Over"


class Func:
    @staticmethod
    def Draw(style: Style = Style()):
        return ("draw", style)

    @staticmethod
    def Clip(n: int):
        return ("clip", int(n))


@dataclass(frozen=True)
class Props:
    fill_rule: str = FillRule.NonZero
    func: tuple = ("draw", Style())


def _f32bits(v: float) -> int:
    return struct.unpack("<I", struct.pack("<f", v))[0]


def _encode_props(p: Props, images: List[Image]) -> List[int]:
    """Props -> style words (layout: include/forma_hip.h)."""
    h = (1 << 6) if p.fill_rule == FillRule.EvenOdd else 0
    kind, payload = p.func
    if kind == "clip":
        return [h | (1 << 8), payload]
    st: Style = payload
    h |= BLEND_MODES.index(st.blend_mode)
    if st.is_clipped:
        h |= 1 << 7
    fk, fv = st.fill
    if fk == "gradient":
        g: Gradient = fv
        h |= (2 if g.type == GradientType.Radial else 1) << 4
        h |= len(g.stops) << 16
        w = [h, 0] + [_f32bits(v) for v in (g.start.x, g.start.y, g.end.x, g.end.y)]
        for c, s in g.stops:
            w += [_f32bits(v) for v in (c.r, c.g, c.b, c.a, s)]
        return w
    if fk == "texture":
        t: Texture = fv
        idx = next((i for i, im in enumerate(images) if im is t.image), None)
        if idx is None:
            images.append(t.image); idx = len(images) - 1
        return [h | (3 << 4), 0] + [_f32bits(v) for v in t.transform.to_array()] + [idx]
    c: Color = fv
    return [h, 0] + [_f32bits(v) for v in (c.r, c.g, c.b, c.a)]


# ---- composition (forma/src/composition/{mod,layer,state}.rs) -------------------------------------------
class _Shared:
    def __init__(self):
        self.pushes: List[Tuple[int, Path, int]] = []   # (geom_id, path, lines) in SegmentBuffer order
        self.geom_id_to_order: Dict[int, Optional[int]] = {}
        self.next_geom_id = 1
        self.geometry_version = 0
        self.pushes_epoch = 0          # bumped whenever `pushes` changes other than by an append at its end (compact_geom)
        self.table_version = 0         # bumped by every change that the per-frame layer / style tables depend on
        self.unchanged_version = 0     # bumped when a render call changes some layer's is_unchanged set
        # changes through Layer.set_transform / set_is_enabled, kept apart from everything else the tables depend on: they touch
        # one entry of the layer table each, and `Renderer(resident_tables=True)` sends just those.  xf_version counts them
        # (each also bumps table_version); xf_log holds the layers of the changes xf_log_base .. xf_version, weakly
        self.xf_version = 0
        self.xf_log: list = []
        self.xf_log_base = 0

    def note_xf(self, layer: "Layer"):
        self.table_version += 1
        self.xf_version += 1
        self.xf_log.append(weakref.ref(layer))
        if len(self.xf_log) > 1 << 16:                    # (nobody reads that far back: a renderer that old takes the full path)
            drop = len(self.xf_log) // 2
            del self.xf_log[:drop]
            self.xf_log_base += drop

    def new_geom_id(self) -> int:
        g = self.next_geom_id; self.next_geom_id += 1; return g


def _drop_layer(shared: "_Shared", gid_cell):
    shared.geom_id_to_order.pop(gid_cell[0], None)
    shared.table_version += 1


class Layer:
    def __init__(self, shared: _Shared):
        self._shared = shared
        self.is_enabled_ = True
        self.affine_transform: Optional[GeomPresTransform] = None
        self.order: Optional[int] = None
        self.geom_id_ = shared.new_geom_id()
        self.props_ = Props()
        self.is_unchanged_: set = set()
        self.lines_count = 0
        # `impl Drop for Layer` (layer.rs:356-363): a layer that goes away takes its geometry id out of
        # geom_id_to_order, which is what lets compact_geom collect its lines.  The id lives in a one-element
        # list because Layer::clear replaces it.
        self._gid_cell = [self.geom_id_]
        self._drop = weakref.finalize(self, _drop_layer, shared, self._gid_cell)

    def geom_id(self) -> int:                                 # layer.rs:143-145
        return self.geom_id_

    def insert(self, path: Path) -> "Layer":                  # layer.rs:90-111
        n = _host().forma_host_path_points(path._h)
        lines = _host().forma_host_path_lines(path._h)        # ids that are Some: what SegmentBuffer::len counts
        if path._stroke_of is not None:
            # a stroke's pieces are counted on the device, not here: the garbage estimate of compact_geom takes the SOURCE path's
            # lines instead.  That threshold is a heuristic; an undercount only delays a compaction.
            lines = _host().forma_host_path_lines(path._stroke_of._h)
        self._shared.pushes.append((self.geom_id_, path, lines))
        self._shared.geom_id_to_order[self.geom_id_] = self.order
        if n:
            self._shared.geometry_version += 1
        self._shared.table_version += 1
        self.lines_count += lines
        self.is_unchanged_.clear()
        return self

    def clear(self) -> "Layer":                               # layer.rs:113-129
        self._shared.geom_id_to_order.pop(self.geom_id_, None)
        self.geom_id_ = self._shared.new_geom_id()
        self._gid_cell[0] = self.geom_id_
        self._shared.geom_id_to_order[self.geom_id_] = self.order
        self._shared.geometry_version += 1
        self._shared.table_version += 1
        self.lines_count = 0
        self.is_unchanged_.clear()
        return self

    def _set_order(self, order: Optional[int]):               # layer.rs:131-141
        if order is not None and self.order != order:
            self.order = order
            self.is_unchanged_.clear()
        self._shared.geom_id_to_order[self.geom_id_] = order
        self._shared.table_version += 1

    def is_enabled(self) -> bool:
        return self.is_enabled_

    def set_is_enabled(self, v: bool) -> "Layer":
        changed = self.is_enabled_ != v
        self.is_enabled_ = v
        if changed:
            self._shared.note_xf(self)
        return self

    def disable(self):
        return self.set_is_enabled(False)

    def enable(self):
        return self.set_is_enabled(True)

    def transform(self) -> GeomPresTransform:
        return self.affine_transform or GeomPresTransform()

    def set_transform(self, t: GeomPresTransform) -> "Layer":  # layer.rs:206-217
        new = None if t.is_identity() else t
        old = self.affine_transform
        if (old is None) != (new is None) or (old is not None and old.t != new.t):
            self.is_unchanged_.clear()
            self.affine_transform = new
            self._shared.note_xf(self)
        return self

    def props(self) -> Props:
        return self.props_

    def set_props(self, props: Props) -> "Layer":             # layer.rs:225-233
        if self.props_ != props:
            self.is_unchanged_.clear()
            self.props_ = props
            self._shared.table_version += 1
        return self


class Composition:
    def __init__(self):
        self._shared = _Shared()
        self.layers: Dict[int, Layer] = {}

    def create_layer(self) -> Layer:
        return Layer(self._shared)

    def is_empty(self) -> bool:
        return not self.layers

    def __len__(self):
        return len(self.layers)

    def insert(self, order: Order, layer: Layer) -> Optional[Layer]:     # composition/mod.rs:146-161
        if layer._shared is not self._shared:
            raise AssertionError("Layer was crated by a different Composition")
        layer._set_order(int(order))
        old = self.layers.get(int(order))
        self.layers[int(order)] = layer
        self._shared.table_version += 1
        if old is not None and old is not layer:
            old._set_order(None)
        return old

    def remove(self, order: Order) -> Optional[Layer]:
        layer = self.layers.pop(int(order), None)
        if layer is not None:
            layer._set_order(None)
        return layer

    def get_order_if_stored(self, geom_id: int) -> Optional[Order]:      # composition/mod.rs:234-241
        o = self._shared.geom_id_to_order.get(geom_id)
        return None if o is None else Order(o)

    def builder_len(self) -> int:                                         # composition/mod.rs:345-352
        return sum(n for _, _, n in self._shared.pushes)

    def actual_len(self) -> int:                                          # composition/mod.rs:354-356
        return sum(l.lines_count for l in self.layers.values())

    def compact_geom(self) -> bool:
        """Geometry garbage collection (composition/mod.rs:372-384): drops the pushes of geometry ids nobody can reach
        any more once they make up at least half of the store.  Returns True if anything was dropped."""
        sh = self._shared
        if self.builder_len() >= self.actual_len() * LINES_GARBAGE_THRESHOLD:
            live = [p for p in sh.pushes if p[0] in sh.geom_id_to_order]
            if len(live) != len(sh.pushes):
                sh.pushes = live
                sh.pushes_epoch += 1
                sh.geometry_version += 1
                return True
        return False

    def get(self, order: Order) -> Optional[Layer]:
        return self.layers.get(int(order))

    def get_mut(self, order: Order) -> Optional[Layer]:
        return self.layers.get(int(order))

    def get_mut_or_insert_default(self, order: Order) -> Layer:
        if int(order) not in self.layers:
            self.insert(order, self.create_layer())
        return self.layers[int(order)]

    def layers_iter(self):
        return self.layers.items()


# ---- buffers (forma/src/cpu/buffer) ---------------------------------------------------------------------
RGBA = (0, 1, 2, 3)      # cpu/channel.rs:57-62
BGRA = (2, 1, 0, 3)
RGB0 = (0, 1, 2, 4)
BGR0 = (2, 1, 0, 4)
RGB1 = (0, 1, 2, 5)
BGR1 = (2, 1, 0, 5)


@dataclass
class Rect:                                   # pixels; rounded out to tiles by the backend (renderer.rs:43-52)
    horizontal: range
    vertical: range


class TileFill:
    """What `Layout.write` receives (cpu/buffer/layout/mod.rs:36-44): ("solid", [u8; 4]) or ("full", colors) with colors a
    [256][4] uint8 array in COLUMN-major order (index = x * TILE_HEIGHT + y), exactly the reference's `TileFill::Full`."""

    @staticmethod
    def Solid(color):
        return ("solid", color)

    @staticmethod
    def Full(colors):
        return ("full", colors)


class Layout:
    """A buffer's layout description (reference trait `Layout`, cpu/buffer/layout/mod.rs:51-163).  Subclass it to describe
    a non-linear buffer: the renderer then hands every written tile to `write` (the generic, host-side path);
    `LinearLayout` is the fast path (one strided device-to-host copy straight into the caller's buffer)."""

    def width(self) -> int:
        raise NotImplementedError

    def height(self) -> int:
        raise NotImplementedError

    def slices_per_tile(self) -> int:
        raise NotImplementedError

    def slices(self, buffer: np.ndarray) -> list:
        """writable views of `buffer`, tile-major: tiles ordered by (tile_y, tile_x), `slices_per_tile()` views each"""
        raise NotImplementedError

    @staticmethod
    def write(slices: list, flusher, fill) -> None:
        raise NotImplementedError

    def width_in_tiles(self) -> int:
        return (self.width() + 15) >> 4

    def height_in_tiles(self) -> int:
        return (self.height() + 15) >> 4


class LinearLayout(Layout):                   # cpu/buffer/layout/mod.rs:167-295
    def __init__(self, width: int, width_stride: int, height: int):
        if width * 4 > width_stride:
            raise AssertionError(f"width exceeds width stride: {width} * 4 > {width_stride}")
        self._w, self.width_stride, self._h = width, width_stride, height

    def width(self) -> int:
        return self._w

    def height(self) -> int:
        return self._h

    def slices_per_tile(self) -> int:
        return 16

    def slices(self, buffer: np.ndarray) -> list:                        # :186-213: rows of every tile, sorted by (tile_y, tile_x)
        flat = buffer.reshape(-1)
        assert self._h * self.width_stride <= flat.size, "height * width_stride exceeds buffer length"
        out = []
        for ty in range(self.height_in_tiles()):
            for tx in range(self.width_in_tiles()):
                for y in range(ty * 16, ty * 16 + 16):
                    if y >= self._h:
                        out.append(flat[0:0])                            # (edge tiles: fewer rows; keep slices_per_tile entries)
                        continue
                    o = y * self.width_stride + tx * 64
                    out.append(flat[o: o + min(64, (self._w - tx * 16) * 4)])
        return out

    @staticmethod
    def write(slices: list, flusher, fill) -> None:                      # :264-295
        kind, payload = fill
        for y, row in enumerate(slices):
            px = row.reshape(-1, 4)
            if kind == "solid":
                px[:] = np.asarray(payload, np.uint8)
            else:
                px[:] = np.asarray(payload, np.uint8).reshape(-1, 4)[np.arange(len(px)) * 16 + y]
        if flusher is not None:
            for row in slices:
                if len(row):
                    flusher.flush(row[:64])


class BufferLayerCache:                       # cpu/buffer/mod.rs:165-197
    def __init__(self, cache_id: int, renderer: "Renderer"):
        self.id = cache_id
        self._renderer = renderer

    def clear(self):
        self._renderer._ctx.cache_clear(self.id)

    def __del__(self):                        # IdDropper (cpu/buffer/mod.rs:98-111): the id returns to the renderer's pool
        try:
            r = self._renderer
            if self.id in r._caches:
                r._caches.discard(self.id)
                r._ctx.cache_clear(self.id)   # the next owner of the id starts from an empty cache
                r._tables_key = None
        except Exception:
            pass


@dataclass
class Buffer:
    buffer: np.ndarray
    layout: LinearLayout
    layer_cache: Optional[BufferLayerCache] = None
    flusher: Optional[object] = None


class BufferBuilder:
    def __init__(self, buffer: np.ndarray, layout: LinearLayout):
        self._b = Buffer(buffer, layout)

    def layer_cache(self, cache: BufferLayerCache):
        self._b.layer_cache = cache; return self

    def flusher(self, flusher):
        self._b.flusher = flusher; return self

    def build(self) -> Buffer:
        return self._b


# ---- the renderer (drop-in for cpu::Renderer) -----------------------------------------------------------------
class Renderer:
    """`forma::hip::Renderer`: same three methods as `cpu::Renderer` (cpu/renderer.rs:61-224)."""

    def __init__(self, device: int = 0, devices=None, frames_in_flight: int = 1, resident_geometry: bool = False,
                 resident_tables: bool = False):
        """`Renderer::new()` (cpu/renderer.rs:63-65).  `devices`: one renderer over several GPUs of this process
        (forma_hip_create_multi — the Rust shim's `Renderer::with_devices`); `frames_in_flight`: device-resident frames
        are pipelined inside the renderer (forma_hip_set_frames_in_flight); `resident_geometry`: the setting for scenes
        whose geometry changes — the device's geometry store is appended to and compacted in place, at the cost of the
        edit, instead of being flattened and uploaded again as a whole (`host_tables` then holds no geometry: see
        `read_geometry`); `resident_tables`: the setting for scenes whose layers move — when nothing but transforms and
        enabled flags changed since the last frame, only those entries of the layer table are sent (forma_hip_update_geoms /
        _update_geoms_xf), and they travel with the frame instead of stopping the frames in flight."""
        self._ctx = Context(device, devices=devices, frames_in_flight=frames_in_flight)
        self._resident = bool(resident_geometry)
        self._dev_pushes: list = []                      # resident mode: the pushes on the device, in store order ...
        self._dev_points: List[int] = []                 # ... their point counts ...
        self._dev_epoch = None                           # ... and the _Shared.pushes_epoch they were taken at
        self._caches = set()
        self._geom_version = None
        self._geom_owner = None
        self._slot_of: Dict[int, int] = {}
        self.last_timings = None
        self.host_tables: Dict[str, np.ndarray] = {}     # last uploaded scene tables (inspection / tests / bench)
        self._tables_key = None                          # (composition, table version, unchanged version, cache) on the device
        self._marked_key = None                          # (composition, table version, cache) whose layers are all marked unchanged
        self._resident_tables = bool(resident_tables)
        self._tables_mark = None                         # resident tables: (table version, xf version, slot map) the device tables were built at

    def create_buffer_layer_cache(self) -> Optional[BufferLayerCache]:     # at most 32 (SmallBitSet)
        for i in range(32):
            if i not in self._caches:
                self._caches.add(i)
                return BufferLayerCache(i, self)
        return None

    # -- geometry store: flatten every live path in one HIP launch, keep the result resident on the device
    def _append_pushes(self, pushes) -> List[int]:
        """append pushes (geom_id, path, lines) to the device's store in order; returns the points each one added.  Filled pushes
        that follow each other go in one call, their counts known on the host; a stroked push goes in a call of its own,
        because only the device knows what its pieces come to (forma_hip_geometry_append_stroked's out_points_added)."""
        H = _host()
        counts: List[int] = []
        run: list = []

        def flush():
            if run:
                self._ctx.geometry_append_paths(run)
                del run[:]
        for p in pushes:
            item = (p[1], self._slot_of.setdefault(p[0], len(self._slot_of)))
            if p[1]._stroke_of is None:
                run.append(item)
                counts.append(int(H.forma_host_path_points(p[1]._h)))
            else:
                flush()
                counts.append(int(self._ctx.geometry_append_paths([item])))
        flush()
        return counts

    def _upload_geometry(self, comp: Composition):
        sh = comp._shared
        if any(p._stroke_of is not None for _, p, _ in sh.pushes):
            # stroked pushes: their pieces exist on the device only, so the store is built there through appends and the host's
            # copy is read back from it
            self._ctx.set_geometry(np.zeros(0, np.float32), np.zeros(0, np.float32), np.zeros(0, np.uint32))
            self._slot_of = {}
            self._append_pushes(sh.pushes)
            x, y, ls = self._ctx.read_geometry()
            self.host_tables.update(x=x, y=y, line_slot=ls)
            self._geom_version = sh.geometry_version
            self._geom_owner = sh
            return
        live = [(g, p) for g, p, _ in sh.pushes]      # garbage is kept until compact_geom drops it; its slots get order NONE
        slot_of: Dict[int, int] = {}
        H = _host()
        batch = H.forma_host_batch_new()
        try:
            for g, p in live:
                slot = slot_of.setdefault(g, len(slot_of))
                H.forma_host_batch_add(batch, p._h, slot)
            n = H.forma_host_batch_points(batch)
            x = np.zeros(n, np.float32); y = np.zeros(n, np.float32); ls = np.zeros(n, np.uint32)
            if n:
                rc = H.forma_host_batch_flatten(batch, self._ctx._h, x.ctypes.data, y.ctypes.data, ls.ctypes.data)
                self._ctx._check(rc)
        finally:
            H.forma_host_batch_free(batch)
        self._ctx.set_geometry(x, y, ls[: max(n - 1, 0)])
        self.host_tables.update(x=x, y=y, line_slot=ls[: max(n - 1, 0)].copy())
        self._slot_of = slot_of
        self._geom_version = sh.geometry_version
        self._geom_owner = sh

    # -- resident mode: reconcile the device's store with the composition's pushes, at the cost of the difference
    def _reconcile_geometry(self, comp: Composition):
        sh = comp._shared
        dev = self._dev_pushes
        if self._geom_owner is not sh or self._dev_epoch is None:
            return self._upload_resident(comp)
        if self._dev_epoch != sh.pushes_epoch:
            # pushes went away (compact_geom): the survivors must be the device's pushes in their order, new ones behind them
            kept, j = [], 0
            for i, p in enumerate(dev):
                if j < len(sh.pushes) and sh.pushes[j] is p:
                    kept.append(i); j += 1
            known = {id(p) for p in dev}
            if any(id(q) in known for q in sh.pushes[j:]):
                return self._upload_resident(comp)        # (an old push behind a new one, or another order: the full path)
            # SegmentBuffer::retain: ranges of whole pushes, merged where they touch; slots renumbered densely in order of
            # first appearance among the survivors — what a from-scratch upload of them would number
            starts = np.concatenate(([0], np.cumsum(self._dev_points))).astype(np.int64) if dev else np.zeros(1, np.int64)
            ranges: List[List[int]] = []
            slot_of: Dict[int, int] = {}
            for i in kept:
                first, count = int(starts[i]), self._dev_points[i]
                slot_of.setdefault(dev[i][0], len(slot_of))
                if ranges and ranges[-1][0] + ranges[-1][1] == first:
                    ranges[-1][1] += count
                else:
                    ranges.append([first, count])
            remap = np.full(max(len(self._slot_of), 1), NONE, np.uint32)
            for g, old in self._slot_of.items():
                if g in slot_of:
                    remap[old] = slot_of[g]
            self._ctx.geometry_retain([(f, c) for f, c in ranges], remap[: len(self._slot_of)])
            self._dev_pushes = [dev[i] for i in kept]
            self._dev_points = [self._dev_points[i] for i in kept]
            self._slot_of = slot_of
            self._dev_epoch = sh.pushes_epoch
            dev = self._dev_pushes
        elif len(sh.pushes) < len(dev) or (dev and sh.pushes[len(dev) - 1] is not dev[-1]):
            return self._upload_resident(comp)
        new = sh.pushes[len(dev):]                        # the pure append: O(new pushes)
        if new:
            self._dev_points.extend(self._append_pushes(new))
            self._dev_pushes.extend(new)
        self._geom_version = sh.geometry_version

    def _upload_resident(self, comp: Composition):
        """the full path of the resident mode: an empty store, then every push appended (flattened on the device, no copy back)"""
        sh = comp._shared
        self._ctx.set_geometry(np.zeros(0, np.float32), np.zeros(0, np.float32), np.zeros(0, np.uint32))
        self._slot_of = {}
        self._dev_points = self._append_pushes(sh.pushes)
        self._dev_pushes = list(sh.pushes)
        self._dev_epoch = sh.pushes_epoch
        self._geom_version = sh.geometry_version
        self._geom_owner = sh
        for k in ("x", "y", "line_slot"):
            self.host_tables.pop(k, None)

    def read_geometry(self):
        """(x, y, line_slot) of the device's geometry store, read back (forma_hip_read_geometry) — in both modes what
        forma_hip_set_geometry was, or would have been, given"""
        return self._ctx.read_geometry()

    def counters(self) -> Dict[str, int]:
        """forma_hip_counters: points in the store, uploads / appends / retains and their bytes, frames rendered, learned
        (synchronous) and re-run"""
        return self._ctx.counters()

    def _upload_tables(self, comp: Composition, cache_id: Optional[int]):
        sh = comp._shared
        geoms = np.zeros(max(len(self._slot_of), 1), GEOM_DTYPE)
        geoms["order"] = NONE
        by_geom = {l.geom_id_: l for l in comp.layers.values()}
        for g, slot in self._slot_of.items():
            layer = by_geom.get(g)
            order = sh.geom_id_to_order.get(g)
            if layer is None or order is None or not layer.is_enabled_:
                continue
            geoms[slot]["order"] = order
            if layer.affine_transform is not None:
                geoms[slot]["flags"] = 1
                geoms[slot]["xf"] = layer.affine_transform.t.to_array()
        n_orders = (max(comp.layers) + 1) if comp.layers else 0
        offsets = np.full(n_orders, NONE, np.uint32)
        unchanged = np.zeros(n_orders, np.uint8)
        words: List[int] = []
        images: List[Image] = []
        interned: Dict[Props, int] = {}
        for order, layer in comp.layers.items():
            off = interned.get(layer.props_)
            if off is None:
                off = len(words); interned[layer.props_] = off
                words += _encode_props(layer.props_, images)
            offsets[order] = off
            unchanged[order] = 1 if (cache_id is not None and cache_id in layer.is_unchanged_) else 0
        self._ctx.set_geoms(geoms)
        self._ctx.set_styles(offsets, np.asarray(words, np.uint32), unchanged)
        img_tab = np.zeros(len(images), IMAGE_DTYPE)
        tex, off = [], 0
        for i, im in enumerate(images):
            img_tab[i] = (off, im.width_, im.height_)
            tex.append(im.texels); off += len(im.texels)
        texels = np.concatenate(tex) if tex else np.zeros((0, 4), np.uint16)
        self._ctx.set_images(img_tab, texels)
        self.host_tables.update(geoms=geoms, style_offsets=offsets, style_words=np.asarray(words, np.uint32),
                                unchanged=unchanged, images=img_tab, texels=texels)

    def render(self, composition: Composition, buffer: Buffer, channels=RGBA, clear_color: Color = Color(1, 1, 1, 1),
               crop: Optional[Rect] = None, timings: bool = False):
        lay = buffer.layout
        W, H = lay.width(), lay.height()
        if W > MAX_WIDTH or H > MAX_HEIGHT:
            raise FormaError(-1, "canvas exceeds MAX_WIDTH x MAX_HEIGHT")
        cache_id = buffer.layer_cache.id if buffer.layer_cache else None
        sh = self._upload_scene(composition, cache_id)
        dst = buffer.buffer
        rect = None if crop is None else (crop.horizontal.start, crop.horizontal.stop, crop.vertical.start, crop.vertical.stop)
        clear = (clear_color.r, clear_color.g, clear_color.b, clear_color.a)
        cid = -1 if cache_id is None else cache_id
        if type(lay) is LinearLayout:                         # fast path: one strided copy of what was written
            assert dst.dtype == np.uint8 and dst.size >= lay.width_stride * H
            out = self._ctx.render(W, H, channels=channels, clear=clear, crop=rect, cache_id=cid, dst=dst.reshape(-1),
                                   stride=lay.width_stride, timings=timings)
            if buffer.flusher is not None:                    # Flusher::flush on every row slice of every written tile
                flat = dst.reshape(-1)                        # (layout/mod.rs:283-294, painter/mod.rs:537-548)
                tw = (W + 15) >> 4
                for t in np.flatnonzero(self._ctx.tiles_written(W, H)):
                    ty, tx = divmod(int(t), tw)
                    n = min(64, (W - tx * 16) * 4)
                    for y in range(ty * 16, min(ty * 16 + 16, H)):
                        o = y * lay.width_stride + tx * 64
                        buffer.flusher.flush(flat[o: o + n])
        else:                                                 # generic Layout: every written tile goes through Layout::write
            out = self._ctx.render(W, H, channels=channels, clear=clear, crop=rect, cache_id=cid, dst=None, timings=timings,
                                   device_only=True)
            img = self._ctx.read_image(W, H).reshape(H, W, 4)
            slices = lay.slices(dst)
            spt = lay.slices_per_tile()
            tw = (W + 15) >> 4
            for t in np.flatnonzero(self._ctx.tiles_written(W, H)):
                ty, tx = divmod(int(t), tw)
                tile = np.zeros((16, 16, 4), np.uint8)        # [x][y]: column-major like TileFill::Full
                blk = img[ty * 16: ty * 16 + 16, tx * 16: tx * 16 + 16]
                tile[: blk.shape[1], : blk.shape[0]] = blk.transpose(1, 0, 2)
                type(lay).write(slices[int(t) * spt: (int(t) + 1) * spt], buffer.flusher, TileFill.Full(tile.reshape(256, 4)))
        if timings:
            self.last_timings = out[1] if isinstance(out, tuple) else out
        self._mark_unchanged(composition, sh, cache_id)

    def _upload_scene(self, composition: Composition, cache_id: Optional[int]):
        composition.compact_geom()                            # renderer.rs:113
        sh = composition._shared
        if getattr(self, "_resident", False):
            # (a path without points bumps no geometry version but still takes a slot, like in a from-scratch upload)
            if self._geom_owner is not sh or self._geom_version != sh.geometry_version or len(sh.pushes) != len(self._dev_pushes):
                self._reconcile_geometry(composition)
        elif self._geom_owner is not sh or self._geom_version != sh.geometry_version:
            self._upload_geometry(composition)
        # the layer / style / unchanged tables stay resident: they are rebuilt only when something they depend on changed
        key = (sh, sh.table_version, sh.unchanged_version if cache_id is not None else -1, cache_id)
        if key != self._tables_key:
            if not self._edit_tables(composition, cache_id):
                self._upload_tables(composition, cache_id)
            self._tables_key = key
            self._tables_mark = (sh.table_version, getattr(sh, "xf_version", 0), self._slot_of)
        return sh

    def _edit_tables(self, comp: Composition, cache_id: Optional[int]) -> bool:
        """resident tables: when only Layer.set_transform / set_is_enabled changed the composition since its tables were
        uploaded (no cache involved, same slot map), build just those entries of the layer table and send them as one
        update_geoms — or one update_geoms_xf when every slot got the same transform — and bring
        host_tables["geoms"] up to date in place.  False: the caller takes the full path."""
        if not getattr(self, "_resident_tables", False) or cache_id is not None:
            return False
        sh = comp._shared
        mark, key = getattr(self, "_tables_mark", None), self._tables_key
        if mark is None or key is None or key[0] is not sh or key[3] is not None or mark[2] is not self._slot_of:
            return False
        moved = sh.xf_version - mark[1]
        if moved <= 0 or sh.table_version - mark[0] != moved or mark[1] < sh.xf_log_base:
            return False
        geoms = self.host_tables.get("geoms")
        if geoms is None or len(geoms) != max(len(self._slot_of), 1):
            return False
        dirty: Dict[int, Layer] = {}
        for ref in sh.xf_log[mark[1] - sh.xf_log_base:]:
            layer = ref()
            if layer is not None:
                slot = self._slot_of.get(layer.geom_id_)
                if slot is not None:
                    dirty[slot] = layer
        slots = np.array(sorted(dirty), np.uint32)
        entries = np.zeros(len(slots), GEOM_DTYPE)
        entries["order"] = NONE
        for i, slot in enumerate(slots):
            layer = dirty[int(slot)]
            order = sh.geom_id_to_order.get(layer.geom_id_)
            if order is None or not layer.is_enabled_ or comp.layers.get(layer.order) is not layer:
                continue
            entries[i]["order"] = order
            if layer.affine_transform is not None:
                entries[i]["flags"] = 1
                entries[i]["xf"] = layer.affine_transform.t.to_array()
        if len(slots):
            xf_bits = np.ascontiguousarray(entries["xf"]).view(np.uint32)
            one_xf = (len(slots) == len(geoms) and bool((entries["flags"] == 1).all())
                      and bool((xf_bits == xf_bits[0]).all()) and np.array_equal(entries["order"], geoms["order"][slots]))
            if one_xf:                                        # the demo's pan: 24 bytes, however many layers
                self._ctx.update_geoms_xf(int(slots[0]), len(slots), entries["xf"][0])
            else:
                self._ctx.update_geoms(slots, entries)
            geoms[slots] = entries
        return True

    def _mark_unchanged(self, composition: Composition, sh, cache_id: Optional[int]):
        if cache_id is not None:                              # renderer.rs:217-223
            mkey = (sh, sh.table_version, cache_id)
            if mkey != self._marked_key:                      # (nothing to do when this exact state was marked already)
                changed = False
                for layer in composition.layers.values():
                    if layer.is_enabled_:
                        if cache_id not in layer.is_unchanged_:
                            layer.is_unchanged_.add(cache_id); changed = True
                    elif cache_id in layer.is_unchanged_:
                        layer.is_unchanged_.discard(cache_id); changed = True
                if changed:
                    sh.unchanged_version += 1
                self._marked_key = mkey

    def render_to_device(self, composition: Composition, out, channels=RGBA, clear_color: Color = Color(1, 1, 1, 1),
                         crop: Optional[Rect] = None, layer_cache: Optional[BufferLayerCache] = None, timings: bool = False):
        """The GPU backend's `Renderer::render_to_texture` (reference gpu/renderer/mod.rs:462-520): paint straight into `out`, a
        torch tensor [H, W, 4] on the renderer's device — uint8: the sRGB bytes `render` writes; float16: the painter's linear
        colour (forma_hip_render_device).  Rows may be padded (`out` may be a view into a wider tensor): the pitch is
        `out.stride(0)`.  The frame waits for the work already enqueued on torch's current stream.  With several frames in
        flight and no cache / timings the frame is enqueued: `out` is complete after `sync()` of the renderer's context."""
        import torch
        if not isinstance(out, torch.Tensor):
            raise ValueError("out must be a torch.Tensor")
        fmt = {torch.uint8: "srgb8", torch.float16: "linear_f16"}.get(out.dtype)
        if fmt is None:
            raise ValueError(f"out must be uint8 (sRGB8) or float16 (linear), not {out.dtype}")
        if out.dim() != 3 or out.shape[2] != 4:
            raise ValueError(f"out must have shape [H, W, 4], not {list(out.shape)}")
        dev = torch.device("cuda", self._ctx.device)
        if out.device != dev:
            raise ValueError(f"out must live on {dev} (the renderer's device), not {out.device}")
        if out.stride(2) != 1 or out.stride(1) != 4:
            raise ValueError("out must have contiguous pixels: stride(2) == 1 and stride(1) == 4")
        H, W = int(out.shape[0]), int(out.shape[1])
        if W > MAX_WIDTH or H > MAX_HEIGHT:
            raise FormaError(-1, "canvas exceeds MAX_WIDTH x MAX_HEIGHT")
        cache_id = layer_cache.id if layer_cache else None
        sh = self._upload_scene(composition, cache_id)
        rect = None if crop is None else (crop.horizontal.start, crop.horizontal.stop, crop.vertical.start, crop.vertical.stop)
        clear = (clear_color.r, clear_color.g, clear_color.b, clear_color.a)
        t = self._ctx.render_device(out.data_ptr(), fmt, W, H, out.stride(0) * out.element_size(), channels=channels, clear=clear,
                                    crop=rect, cache_id=-1 if cache_id is None else cache_id,
                                    wait_stream=torch.cuda.current_stream(dev).cuda_stream, timings=timings)
        if timings:
            self.last_timings = t
        self._mark_unchanged(composition, sh, cache_id)
        return out
