"""The oracle against raster_model.py: what a pixel segment IS (how much of which pixel lies to the right of which piece of a
line) and how far a flattened contour may stray from its curve, stated by a model written from geometry -- not by a second
restatement of the reference.  test_gpu_raster_model.py holds every HIP route to the same model on the same cases.

Bars: on lattice lines that pass through no pixel corner, the accumulated doubled area A and every row's cover total equal the
model's exactly; on random f32 lines the row totals are exact and |dA| stays within the recorded bound (one sixteenth of x over
one pixel of cover = 16 of 512), with at most 5 % of the lines differing at all; the polygon images are within 1 code value.
Stage 1 is held to the figures recorded in golden/raster_model_bounds.json x 1.25, and to two derived bounds.

`python tests/test_raster_model.py --record` measures the oracle and writes that file."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import raster_cases as RC
import raster_model as RM
from oracle import oracle as orc

STAGE2, SHAPES = RC.STAGE2, RC.SHAPES


def oracle_stream(name):
    lines, w, h, _ = RC.stage2_scenes()[name]
    o = orc.Oracle()
    RC.load(o, RC.line_tables(lines))
    o.prepare_lines(w, h)
    return o.rasterize()


# ---- the model on cases worked by hand -----------------------------------------------------------------------------------------
def test_pieces_of_a_line_worked_by_hand():
    """(0, 0) -> (3, 2): cut at x = 1 (y = 2/3 -> 11 sixteenths), at y = 1 (x = 3/2 -> 24) and at x = 2 (y = 4/3 -> 21)"""
    ps, corner = RM.pieces((0.0, 0.0), (3.0, 2.0))
    assert not corner
    assert ps == [(0, 0, 11, 11 * (32 - 0 - 16)), (1, 0, 5, 5 * (64 - 16 - 24)), (1, 1, 5, 5 * (64 - 24 - 32)), (2, 1, 11, 11 * (96 - 32 - 48))]
    back, _ = RM.pieces((3.0, 2.0), (0.0, 0.0))
    assert [(px, py, -c, -a) for px, py, c, a in reversed(back)] == ps      # the other direction: the sign of cover, nothing else
    assert RM.pieces((0.5, 0.5), (2.5, 2.5))[1] and not RM.pieces((0.5, 0.25), (2.5, 2.25))[1]
    # a vertical line on a pixel boundary belongs to the pixel on its right, at full width
    assert RM.pieces((5.0, 1.25), (5.0, 1.75))[0] == [(5, 1, 8, 8 * 32)]
    t = RM.row_area([(3, px, py, c, a) for px, py, c, a in ps])
    assert RM.row_totals(t, 3) == {0: 16, 1: 16} and RM.dense(t, 3, 4, 2).tolist() == [[176, 11 * 32 + 120, 512, 512], [0, 40, 5 * 32 + 176, 512]]


def test_a_full_pixel_is_512_and_a_square_is_its_edges():
    sq = [(2.0, 1.0), (2.0, 3.0), (4.5, 3.0), (4.5, 1.0)]
    a = RM.dense(RM.polygon_area([sq], 8, 4), 0, 8, 4)
    want = np.zeros((4, 8), np.int64)
    want[1:3, 2:4] = 512; want[1:3, 4] = 256
    assert np.array_equal(a, want)
    assert np.array_equal(RM.dense(RM.polygon_area([sq[::-1]], 8, 4), 0, 8, 4), -want)


def test_culling_rules():
    assert RM.culled((1.0, 2.0), (5.0, 2.0), 8, 8)                          # horizontal
    assert RM.culled((1.0, -2.0), (5.0, 0.0), 8, 8)                         # wholly at or above y = 0
    assert RM.culled((1.0, 8.0), (5.0, 9.0), 8, 8) and RM.culled((8.0, 1.0), (9.0, 5.0), 8, 8)
    assert not RM.culled((-9.0, 1.0), (-5.0, 5.0), 8, 8)                    # the left edge is not culled
    assert not RM.culled((1.0, -2.0), (5.0, 0.5), 8, 8) and not RM.culled((7.5, 1.0), (9.0, 5.0), 8, 8)


def test_decode_does_not_depend_on_the_order_of_the_stream():
    s = oracle_stream("short_lines")
    rng = np.random.default_rng(0)
    assert np.array_equal(RM.decode(s), RM.decode(rng.permutation(s)))
    assert not RM.difference(RM.decode(s), RM.decode(np.sort(s)))


def test_the_family_holds_what_it_claims():
    plain = RC.no_corner_lines()
    kinds = RC.endpoint_kinds(plain)
    assert min(kinds.values()) >= 100, kinds                                # the c == 0 / d == 0 shifts, at both ends
    assert all(not RM.pieces(a, b)[1] for a, b in plain[::37])
    w, h = RC.LATTICE_CANVAS
    assert any(a[0] == w and b[0] < w for a, b in plain) and any(a[1] == h and b[1] < h for a, b in plain)
    assert any(a[0] < 0 for a, b in plain) and any(a[1] < 0 for a, b in plain)
    assert any(a[0] == b[0] and a[0] in (16.0, 32.0) for a, b in plain)     # vertical, on a tile boundary
    assert len({(a, b) for a, b in plain} & {(b, a) for a, b in plain}) == len(set(plain))          # both directions of every line
    assert len(RC.short_lines()) >= 600
    assert RC.n_segments((0,) + RC.LONG_LINE + (None,), 64, 64) > 4096
    assert all(len(RC.stage2_scenes()[n][0]) <= 8000 for n in STAGE2)


# ---- stage 2 -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", STAGE2)
def test_oracle_stream_against_the_model(name):
    s = oracle_stream(name)
    if name.startswith("last_block_"):
        assert len(s) % 2048 == int(name.rsplit("_", 1)[1]) and len(s) > 2048
    n_diff, _, worst, _ = RC.check_stream(name, s, "oracle")
    b = RC.bounds()
    if name.startswith("general"):
        assert worst == b["general"][name]["max_abs_dA"] and n_diff == b["general"][name]["lines_that_differ"]     # the record is the oracle's
    if name == "corner":
        assert n_diff == b["corner"]["differ"]


def test_the_pinned_corner_tie():
    """QUIRK (raster_model.CORNER_TIE_LINE): the stream of (58.875, 172.25) -> (76.25, 137.5) ends with a piece of cover +8 in
    pixel (76, 137) -- a piece that runs from beyond the line's end back to it -- and its covers sum to -548, not to -556"""
    o = orc.Oracle()
    RC.load(o, RC.line_tables(RC.numbered([RM.CORNER_TIE_LINE])))
    o.prepare_lines(300, 300)
    f = orc.seg_fields(o.rasterize())
    last = (int(f["tile_x"][-1] * 16 + f["local_x"][-1]), int(f["tile_y"][-1] * 16 + f["local_y"][-1]), int(f["cover"][-1]))
    assert last == RM.CORNER_TIE_LAST
    assert int(f["cover"].sum()) == RM.CORNER_TIE_COVER_SUM
    ps, corner = RM.pieces(*RM.CORNER_TIE_LINE)
    assert corner and sum(p[2] for p in ps) == -556 == round(16 * (137.5 - 172.25))


@pytest.mark.parametrize("name", ["64x64", "72x40", "33x17"])
def test_polygon_images_and_areas(name):
    w, h, layers = RC.polygon_scenes()[name]
    o = orc.Oracle()
    RC.load(o, RC.polygon_tables(layers))
    got = o.render(w, h, clear=(1.0, 1.0, 1.0, 1.0))
    RC.check_polygons(name, got, o.segments(1), "oracle")


def test_polygon_scenes_are_cut_by_every_edge():
    for name, (w, h, layers) in RC.polygon_scenes().items():
        pts = np.array([p for cs, _, _ in layers for c in cs for p in c])
        assert pts[:, 0].min() < 0 and pts[:, 1].min() < 0 and pts[:, 0].max() > w and pts[:, 1].max() > h, name


# ---- stage 1 -------------------------------------------------------------------------------------------------------------------
def _flat(o, cmds, t9):
    x, y, nc = o.flatten(RC.oracle_path(cmds, t9))
    assert nc[-1] and not nc[:-1].any()
    return x, y


@pytest.mark.parametrize("scale", RC.CURVE_SCALES)
@pytest.mark.parametrize("kind", RC.CURVE_KINDS)
def test_flattened_families_against_their_curves(kind, scale):
    o = orc.Oracle()
    ms = [RC.curve_measures(c, None, *_flat(o, c, None)) for c in RC.curve_family(kind, scale)]
    RC.check_measures("%s/%g" % (kind, scale), RC.worst_of(ms), RC.bounds()["stage1"]["families"]["%s/%g" % (kind, scale)],
                      on_curve=kind in RC.ON_CURVE, who="oracle")


@pytest.mark.parametrize("name", SHAPES)
def test_flattened_edge_shapes_against_their_curves(name):
    cmds, t9 = RC.edge_shapes()[name]
    x, y = _flat(orc.Oracle(), cmds, t9)
    RC.check_measures(name, RC.curve_measures(cmds, t9, x, y), RC.bounds()["stage1"]["edge_shapes"][name],
                      only_c=name == "doubled_back_quad", who="oracle")


def test_the_doubled_back_quadratic_drops_its_far_end():
    """QUIRK (raster_model, path.rs:218-236, :259-266, :322-332): the contour flattens to one point of the curve plus the closing
    point; the quadratic's own end, 22.9 px away, is not emitted.  The contour encloses no area, so nothing is painted wrong."""
    x, y = _flat(orc.Oracle(), RC.DOUBLED_BACK, None)
    assert len(x) == 3 and (x[0], y[0]) == (x[2], y[2])
    far = RM.curve_distance(RC.model_segments(RC.DOUBLED_BACK), x, y)
    assert 22.8 < far < 23.0, far
    assert abs(RM.polyline_area(x, y)) < 0.1


def test_shape_list_is_complete():
    assert sorted(SHAPES) == sorted(RC.edge_shapes())


# ---- the record ----------------------------------------------------------------------------------------------------------------
def record():
    """measure the oracle on every committed family and write golden/raster_model_bounds.json"""
    head = subprocess.run(["git", "rev-parse", "--short", "HEAD"], capture_output=True, text=True,
                          cwd=os.path.dirname(os.path.abspath(__file__))).stdout.strip()
    out = {"measured_on": {"commit": head, "what": "oracle/forma_oracle.cpp (CPU) at that commit"},
           "general": {"seeds": list(RC.GENERAL_SEEDS), "lines_per_seed": RC.GENERAL_LINES_PER_SEED, "canvas": list(RC.GENERAL_CANVAS)},
           "corner": {}, "stage1": {
               "margin": 1.25,
               "margin_note": "the families are seeded, but a libm change may move an f32 sqrt by an ulp and with it a vertex: every "
                              "recorded figure is asserted x 1.25.  c_over_length is also held to the derived bound MAX_ERROR = 1/16; "
                              "a_ulps (quadratics and rational quadratics) is measure (a) in ulps of the contour's largest coordinate.",
               "curves_per_family": RC.CURVES_PER_FAMILY, "seeds": RC.CURVE_SEEDS, "families": {}, "edge_shapes": {}}}
    worst_all = 0
    for name in ("general", "general_affine"):
        n_diff, bad_rows, worst, _ = RC.stream_figures(name, oracle_stream(name))
        assert bad_rows == 0 and worst <= 32, (name, bad_rows, worst)       # more than 32 wants an explanation, not a record
        out["general"][name] = {"lines": len(RC.stage2_scenes()[name][0]), "lines_that_differ": n_diff, "max_abs_dA": worst}
        worst_all = max(worst_all, worst)
    out["general"]["max_abs_dA"] = worst_all
    n_diff, _, _, layers = RC.stream_figures("corner", oracle_stream("corner"))
    out["corner"] = {"lines": len(RC.stage2_scenes()["corner"][0]), "differ": n_diff}
    o = orc.Oracle()
    for kind in RC.CURVE_KINDS:
        for scale in RC.CURVE_SCALES:
            ms = [RC.curve_measures(c, None, *_flat(o, c, None)) for c in RC.curve_family(kind, scale)]
            out["stage1"]["families"]["%s/%g" % (kind, scale)] = RC.worst_of(ms)
    for name, (cmds, t9) in RC.edge_shapes().items():
        out["stage1"]["edge_shapes"][name] = RC.curve_measures(cmds, t9, *_flat(o, cmds, t9))
    with open(RC.BOUNDS_PATH, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", RC.BOUNDS_PATH)


if __name__ == "__main__":
    if "--record" in sys.argv:
        record()
