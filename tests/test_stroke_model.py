"""stroke_model.py pinned against the oracle before anything on the GPU leans on it, and the host-only parts of the stroke
feature: the ABI struct, the open path builder, the SVG loader's strokes.

The model's pieces are pushed as ordinary fill paths through ref_api (the oracle) and rendered black on white.  Shapes whose
outline lies on whole pixels must give exact ink; for bevel and round joins and round caps on sixteenth-aligned inputs the summed
ink equals the analytic area of the union of the flattened pieces within one u8 step per partially covered pixel."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import stroke_cases as SC
import stroke_model as SM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BLACK = (0.0, 0.0, 0.0, 1.0)


def _linear(v):
    """sRGB code value(s) -> linear light"""
    s = np.asarray(v, np.float64) / 255.0
    return np.where(s <= 0.04045, s / 12.92, ((s + 0.055) / 1.055) ** 2.4)


def _render(case, size=64):
    _, _, _, pieces = case.model()
    return SC.ref_render([(SC.piece_polys(pieces), BLACK, "NonZero")], size, size), pieces


# ---- the model, worked by hand ---------------------------------------------------------------------------------------------------
def test_layout_worked_by_hand():
    """(10,10) -> (20,10) -> (20,20), half width 1, bevel, square caps: start cap, body, bevel join + body, end cap.  The turn is to
    the left with y up, so the join lies on the right of the path: the first line's left normal is (0,1), the second's (-1,0),
    and the outer corners at v = (20,10) are v - ob = (21,10) and v - oa = (20,9)."""
    c = SC.Case("hand", [[(10.0, 10.0), (20.0, 10.0), (20.0, 20.0)]], 1.0, SM.BEVEL, SM.SQUARE, slots=[7])
    x, y, slot, pieces = c.model()
    assert [p.kind for p in pieces] == ["cap_square", "body", "bevel", "body", "cap_square"]
    assert [p.src for p in pieces] == [0, 0, 1, 1, 2]
    assert pieces[0].pts == [(9.0, 11.0), (10.0, 11.0), (10.0, 9.0), (9.0, 9.0), (9.0, 11.0)]
    assert pieces[1].pts == [(10.0, 11.0), (20.0, 11.0), (20.0, 9.0), (10.0, 9.0), (10.0, 11.0)]
    assert pieces[2].pts == [(20.0, 10.0), (21.0, 10.0), (20.0, 9.0), (20.0, 10.0)]
    assert pieces[4].pts == [(19.0, 20.0), (19.0, 21.0), (21.0, 21.0), (21.0, 20.0), (19.0, 20.0)]
    assert len(x) == 5 + 5 + 4 + 5 + 5 and list(slot) == [7, 7, 7, 7, SM.NONE] * 2 + [7, 7, 7, SM.NONE] + [7, 7, 7, 7, SM.NONE] * 2
    assert [p.at for p in pieces] == [0, 5, 10, 14, 19]
    # a miter at the same corner reaches (21, 9); beyond its limit it is the bevel again
    m = SC.Case("hand-miter", c.contours, 1.0, SM.MITER, SM.BUTT).model()[3]
    assert [p.kind for p in m] == ["body", "miter", "body"] and m[1].pts[2] == pytest.approx((21.0, 9.0), abs=1e-12)
    assert [p.kind for p in SC.Case("hand-limit", c.contours, 1.0, SM.MITER, SM.BUTT, limit=1.4).model()[3]] == ["body", "bevel", "body"]


def test_fan_steps_keep_the_sagitta():
    for hw in (0.01, 0.05, 0.3, 1.0, 7.5, 100.0, 65536.0):
        for phi in (0.01, 1.0, np.pi / 2, np.pi):
            n = SM.min_steps(phi, hw)
            sag = lambda k: hw * (1.0 - np.cos(phi / (2 * k)))
            assert sag(n) <= SM.MAX_ERROR * (1 + 1e-9) and (n == 1 or sag(n - 1) > SM.MAX_ERROR), (hw, phi, n)


def test_union_area_of_known_shapes():
    sq = lambda x, y, s: [(x, y), (x, y + s), (x + s, y + s), (x + s, y), (x, y)]
    assert SM.union_area([sq(0, 0, 4)]) == 16.0
    assert SM.union_area([sq(0, 0, 4), sq(2, 2, 4)]) == 28.0                      # overlap counted once
    assert SM.union_area([sq(0, 0, 4), sq(1, 1, 2), sq(10, 0, 1)]) == 17.0
    assert SM.union_area([[(0, 0), (0, 4), (4, 0), (0, 0)], [(0, 0), (4, 4), (4, 0), (0, 0)]]) == pytest.approx(8 + 8 - 4)


# ---- against the oracle ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(3))
def test_pixel_aligned_shapes_give_exact_ink(k):
    case, ink = SC.pixel_aligned()[k]
    img, _ = _render(case)
    assert np.array_equal(img[..., 3], np.full(img.shape[:2], 255, np.uint8))
    red = img[..., 0]
    assert set(np.unique(red)) <= {0, 255}, case.name                              # no partially covered pixel at all
    assert int((red == 0).sum()) == ink, case.name


@pytest.mark.parametrize("k", range(3))
def test_sixteenth_aligned_ink_equals_the_analytic_area(k):
    case = SC.sixteenth_aligned()[k]
    img, pieces = _render(case)
    red = img[..., 0].astype(np.int64)
    cover = 1.0 - _linear(red)
    partial = (red > 0) & (red < 255)
    # one u8 step of a partially covered pixel, in units of coverage: the wider of the two steps next to its value
    step = np.maximum(_linear(np.minimum(red + 1, 255)) - _linear(red), _linear(red) - _linear(np.maximum(red - 1, 0)))
    tol = float(step[partial].sum())
    want = SM.union_area(SC.piece_polys(pieces))
    got = float(cover.sum())
    print(f"{case.name}: ink {got:.4f} area {want:.4f} partial pixels {int(partial.sum())} tolerance {tol:.4f}")
    assert partial.sum() > 0
    assert abs(got - want) <= tol, case.name


def test_every_piece_has_the_same_winding():
    cases = SC.exact_families() + SC.random_cases() + SC.sixteenth_aligned() + [c for c, _ in SC.pixel_aligned()]
    n = 0
    for case in cases:
        for p in case.model()[3]:
            a2 = p.area2()
            assert a2 <= 1e-9 * (1.0 + abs(a2)), (case.name, p.kind, p.src, a2)  # clockwise with y up (an exact U-turn's bevel has no area)
            assert p.pts[0] == p.pts[-1]
            n += 1
    assert n > 500


def test_exact_families_are_exact_in_f32():
    """what test_gpu_stroke.py compares bit for bit: the model's float64 coordinates of these families are f32 values, positive
    (no signed zero to argue about), and the families hold both caps, bevels, miters and limited miters"""
    cases = SC.exact_families()
    kinds = set()
    for case in cases:
        mx, my, _, pieces = case.model()
        assert len(pieces) > 0, case.name
        for v in (mx, my):
            assert np.array_equal(v.astype(np.float32).astype(np.float64), v), case.name
            assert (v > 0).all(), case.name
        kinds |= {p.kind for p in pieces}
    assert len(cases) >= 15 and kinds == {"body", "bevel", "miter", "cap_square"}


def test_random_cases_leave_nothing_out():
    """the generator redraws near-ties instead of dropping cases: every join / cap combination is there, open and closed"""
    cases = SC.random_cases()
    assert len(cases) == 24 and {(c.strokes[0][4], c.strokes[0][5]) for c in cases} == {(j, k) for j in range(3) for k in range(3)}
    kinds = {p.kind for c in cases for p in c.model()[3]}
    assert kinds == {"body", "bevel", "miter", "round", "cap_square", "cap_round"}


# ---- host only -------------------------------------------------------------------------------------------------------------------
def test_stroke_range_layout_matches_the_ctypes_mirror(tmp_path):
    from forma_amd import _lib
    gcc = shutil.which("gcc")
    if not gcc:
        pytest.skip("no gcc")
    m = _lib.StrokeRangeT
    offs = "".join(f", offsetof(forma_stroke_range_t, {f})" for f, _ in m._fields_)
    fmt = " ".join(["%zu"] * (1 + len(m._fields_)))
    prog = tmp_path / "abi.c"
    prog.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "forma_hip.h"\nint main(void) {\n'
                    f'    printf("{fmt} %u %u %u %u %u %u\\n", sizeof(forma_stroke_range_t){offs}, FORMA_JOIN_BEVEL, FORMA_JOIN_MITER, FORMA_JOIN_ROUND,\n'
                    '           FORMA_CAP_BUTT, FORMA_CAP_SQUARE, FORMA_CAP_ROUND);\n    return 0;\n}\n')
    exe = tmp_path / "abi"
    subprocess.run([gcc, "-std=c11", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)], check=True)
    out = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert out[:-6] == [C.sizeof(m)] + [getattr(m, f).offset for f, _ in m._fields_] == [32, 0, 8, 16, 20, 24, 28]
    from forma_amd import api
    assert out[-6:] == [api.StrokeJoin.Bevel, api.StrokeJoin.Miter, api.StrokeJoin.Round, api.StrokeCap.Butt, api.StrokeCap.Square, api.StrokeCap.Round]
    assert out[-6:] == [SM.BEVEL, SM.MITER, SM.ROUND, SM.BUTT, SM.SQUARE, SM.ROUND_CAP]
    assert _lib.SYMBOLS["forma_hip_geometry_append_stroked"] and hasattr(_lib.lib(), "forma_hip_geometry_append_stroked")


def _counts(path):
    from forma_amd import api
    H = api._host()
    return int(H.forma_host_path_points(path._h)), int(H.forma_host_path_lines(path._h))


def test_open_builder_adds_no_closing_line():
    from forma_amd import api
    P = api.Point
    tri = lambda b: b.move_to(P(1, 1)).line_to(P(9, 1)).line_to(P(9, 9))
    assert _counts(tri(api.PathBuilder()).build()) == (4, 3)                      # the default closes: 3 lines
    assert _counts(tri(api.PathBuilder(open_contours=True)).build()) == (3, 2)    # open: what was drawn
    assert _counts(tri(api.PathBuilder(open_contours=True)).close().build()) == (4, 3)
    assert _counts(tri(api.PathBuilder(open_contours=True)).close().close().build()) == (4, 3)      # closing a closed contour adds nothing
    # move_to does not close either: two open contours
    two = tri(api.PathBuilder(open_contours=True)).move_to(P(20, 20)).line_to(P(30, 20)).build()
    assert _counts(two) == (5, 3)
    assert _counts(tri(api.PathBuilder()).move_to(P(20, 20)).line_to(P(30, 20)).line_to(P(30, 30)).build()) == (8, 6)


def test_stroked_paths_are_terminal_and_count_their_source_lines():
    from forma_amd import api
    P = api.Point
    p = api.PathBuilder(open_contours=True).move_to(P(1, 1)).line_to(P(9, 1)).line_to(P(9, 9)).build()
    st = p.transform([2, 0, 0, 0, 2, 0, 0, 0, 1]).stroke(api.StrokeStyle(2.0, api.StrokeJoin.Round, api.StrokeCap.Round))
    assert st.stroke_style.width == 2.0 and st.stroke_style.miter_limit == 4.0
    with pytest.raises(ValueError):
        st.transform([1, 0, 0, 0, 1, 0, 0, 0, 1])
    with pytest.raises(ValueError):
        st.stroke(api.StrokeStyle(1.0))
    for bad in (dict(width=0.0), dict(width=float("nan")), dict(width=1.0, miter_limit=0.5), dict(width=1.0, join=3), dict(width=1.0, cap=9)):
        with pytest.raises(ValueError):
            api.StrokeStyle(**bad)
    comp = api.Composition()
    lay = comp.get_mut_or_insert_default(api.Order(0)).insert(st)
    assert lay.lines_count == 2 and comp._shared.pushes[0][2] == 2                # the source path's lines


SVG = """<svg xmlns="http://www.w3.org/2000/svg" width="64" height="64">
<path d="M8 8 L40 8 L40 40 Z" fill="#f00" fill-rule="evenodd" stroke="#00f" stroke-width="2" stroke-linejoin="round"/>
<g transform="matrix(0 2 -2 0 60 0)">
<path d="M4 20 L20 20" fill="none" stroke="black" stroke-width="3" stroke-linecap="square" stroke-opacity="0.5" stroke-dasharray="4 2"/>
</g>
<path d="M1 1 L5 1 L5 5" fill="green"/>
<rect x="10" y="50" width="8" height="4" fill="none" stroke="#0f0" stroke-miterlimit="2"/>
<path d="M1 1 L5 1" stroke="none" fill="blue"/>
</svg>"""


def test_svg_loader_with_and_without_strokes():
    from forma_amd import api, svg
    plain = svg.load(SVG, is_text=True)
    assert len(plain.paths) == 2 and not plain.strokes                            # today's behaviour: stroked shapes are skipped
    old = svg.Svg(SVG, is_text=True)
    assert [(_counts(p), fr, fl, bm) for p, fr, fl, bm in old.paths] == [(_counts(p), fr, fl, bm) for p, fr, fl, bm in plain.paths]
    s = svg.load(SVG, 2.0, is_text=True, strokes=True)
    # fill + outline, outline (fill none), fill, outline (rect, fill none), fill
    assert len(s.paths) == 6 and sorted(s.strokes) == [1, 2, 4]
    assert [fr for _, fr, _, _ in s.paths] == [api.FillRule.EvenOdd] + [api.FillRule.NonZero] * 5
    assert [p._stroke_of is not None for p, *_ in s.paths] == [False, True, True, False, True, False]
    st = s.strokes
    assert (st[1].width, st[1].join, st[1].cap, st[1].miter_limit) == (4.0, api.StrokeJoin.Round, api.StrokeCap.Butt, 4.0)
    assert (st[2].width, st[2].join, st[2].cap) == (12.0, api.StrokeJoin.Miter, api.StrokeCap.Square)     # 3 * sqrt(|det|) = 3 * 2, * scale 2
    assert (st[4].width, st[4].miter_limit) == (2.0, 2.0)
    assert s.paths[1][0].stroke_style == st[1]
    assert s.paths[2][2][1].a == 0.5 and s.paths[1][2][1].b == 1.0                # stroke-opacity; the stroke's colour
    # Z closes the outline with a real line: the triangle's outline has 3 lines like its fill, the open polyline keeps 1
    assert _counts(s.paths[1][0]._stroke_of) == (4, 3) and _counts(s.paths[2][0]._stroke_of) == (2, 1)
    comp = s.compose(api.Composition())
    assert len(comp) == 6
