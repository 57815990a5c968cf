"""The rasterizer's fused digit partition under its three rank forms (csrc/lines.hip ras_partition, FORMA_HIP_DEBUG=ras_rank).

`ras_rank=0` ranks every row of 64 keys with the 8-ballot match-any, `ras_rank=1` (the default) by its runs of equal digit where
that is exact, `ras_rank=2` makes the run test and fails it.  Every scene is rendered with `fuse_digit=2` under the three, read-
back-free with one frame slot and with three; the sorted stream and the image must equal the `fuse_digit=0` frame's and the
oracle's byte for byte.  The kernels of a timed frame prove that the fused rasterizer ran (`k_slice_scan` follows it, one
`k_onesweep` fewer).  The scenes are the rows the run rule has to survive: digits that come back inside 64 consecutive segments
(A,B,A), nearly every key a head, rows of one run and blocks of one digit, a last block of 1 / 63 / 64 / 65 / 2 047 keys, a
first digit relative to its minimum, and a first digit in the key's low word (layers out of paint order).

The 4 112 x 64 canvas: with 64 rows the plain digits of that canvas need two passes, as many as the biased plan, so the library
keeps the plain plan there (make_segment_sort_plan takes the bias only where it saves a pass) — the case runs as the fused two-
pass plan it gets; `test_biased_first_digit` is the same geometry on a 4 112 x 4 112 canvas, where the bias saves the third
pass and the fused first digit is `tile_x - min`."""
import numpy as np
import pytest

import scene as S
from forma_amd import api, scenes
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

CLEAR = (1.0, 1.0, 1.0, 1.0)
RANKS = ("ras_rank=0", "ras_rank=1", "ras_rank=2")


def _run(monkeypatch, switch, comp, w, h):
    """the synchronous first frame, read-back-free frames with one slot (the last one timed), then with three slots"""
    monkeypatch.setenv("FORMA_HIP_DEBUG", switch)
    image = np.zeros((h, w * 4), np.uint8)
    r = api.Renderer(device=0)
    try:
        r.render(comp, api.BufferBuilder(image.reshape(-1), api.LinearLayout(w, w * 4, h)).build(), api.RGBA,
                 api.Color(*CLEAR), None)
        ctx = r._ctx
        for _ in range(3):
            ctx.render(w, h, clear=CLEAR, device_only=True)
        img1, tm = ctx.render(w, h, clear=CLEAR, timings=True)
        names = [k[0] for k in ctx.kernel_times()]
        s1 = ctx.segments(1).copy()
        ctx.set_frames_in_flight(3)
        for _ in range(9):
            ctx.render(w, h, clear=CLEAR, device_only=True)
        img3 = ctx.read_image(w, h).copy()
        s3 = ctx.segments(1).copy()
        ctx.set_frames_in_flight(1)
        return {"images": [image, img1.copy(), img3], "streams": [s1, s3], "names": names, "tm": tm,
                "tables": dict(r.host_tables)}
    finally:
        r._ctx.close()


def _check(monkeypatch, comp, w, h, extra="", passes=None, oracle_image=True):
    ref = _run(monkeypatch, "fuse_digit=0" + extra, comp, w, h)
    assert "k_slice_scan" not in ref["names"]
    o = orc.Oracle()
    S.load(o, ref["tables"])
    if oracle_image:
        want = o.render(w, h, clear=CLEAR)
        want_sorted = o.segments(1)
    else:
        want = None
        o.prepare_lines(w, h); o.rasterize()
        want_sorted = o.sort()
    n_pass = int(ref["tm"]["n_sort_passes"])
    if passes is not None:
        assert n_pass == passes, n_pass
    assert ref["names"].count("k_onesweep") == n_pass
    for s in ref["streams"]:
        assert np.array_equal(s, want_sorted)
    for k, img in enumerate(ref["images"]):
        if want is not None:
            print("fuse_digit=0 image", k, "max difference from the oracle", int(np.abs(img.astype(int) - want.astype(int)).max()))
            assert np.array_equal(img, want), ("oracle image", k)
    for rank in RANKS:
        got = _run(monkeypatch, "fuse_digit=2," + rank + extra, comp, w, h)
        # the fused instantiation ran: the rasterizer, the slice scan behind it, one plain digit pass fewer
        assert "k_rasterize" in got["names"] and "k_slice_scan" in got["names"], (rank, got["names"])
        assert int(got["tm"]["n_sort_passes"]) == n_pass and got["names"].count("k_onesweep") == n_pass - 1, (rank, got["names"])
        assert int(got["tm"]["n_segments"]) == int(ref["tm"]["n_segments"])
        for k, s in enumerate(got["streams"]):
            assert np.array_equal(s, want_sorted), (rank, "stream", k)
        for k, (a, b) in enumerate(zip(ref["images"], got["images"])):
            assert np.array_equal(a, b), (rank, "image", k)
            if want is not None:
                assert np.array_equal(b, want), (rank, "oracle image", k)
    return ref


def _fill(comp, order, points, color=(0.1, 0.3, 0.8, 1.0)):
    pb = api.PathBuilder().move_to(api.Point(*points[0]))
    for p in points[1:]:
        pb = pb.line_to(api.Point(*p))
    comp.get_mut_or_insert_default(order).insert(pb.build()).set_props(scenes._solid(api.Color(*color)))


def _zigzag(comp, order, x_mid, amp, step, y0, y1, color):
    """a ribbon 1.5 pixels wide whose edges swing `amp` pixels to either side of x_mid every `step` pixels of y: every line
    crosses the tile-column boundary at x_mid"""
    ys = np.arange(y0, y1, step)
    down = [(x_mid + (amp if i & 1 else -amp) + 0.3, float(y) + 0.4) for i, y in enumerate(ys)]
    up = [(x + 1.5, y) for x, y in reversed(down)]
    _fill(comp, order, down + up, color)


def _tiny_triangles(comp, first_order, n, w, h, seed):
    rng = np.random.default_rng(seed)
    for i in range(n):
        x, y = float(rng.uniform(1, w - 4)), float(rng.uniform(1, h - 4))
        s = float(rng.uniform(0.8, 2.0))
        _fill(comp, first_order + i, [(x, y), (x + s, y + s / 3), (x + s / 2, y + s)], (0.2, 0.4, (i % 7) / 7.0, 1.0))


def test_digits_that_come_back_inside_a_row(monkeypatch):
    """ribbons zig-zagging across the tile-column boundary x = 256: a swing of 12 pixels gives runs of ~13-30 segments, A,B,A
    with three or four heads (the pairwise digit test decides); a swing of 3 pixels gives A,B,A,B.. with a period of a few
    segments (the head count decides)"""
    comp = api.Composition()
    _zigzag(comp, 0, 256.0, 12.0, 3.0, 8, 500, (0.8, 0.2, 0.1, 1.0))
    _zigzag(comp, 1, 256.0, 3.0, 2.0, 8, 500, (0.1, 0.6, 0.3, 1.0))
    _zigzag(comp, 2, 128.0, 12.0, 3.0, 8, 500, (0.3, 0.2, 0.7, 1.0))
    _check(monkeypatch, comp, 512, 512, passes=2)


def test_nearly_every_key_a_head(monkeypatch):
    comp = api.Composition()
    _tiny_triangles(comp, 0, 3000, 512, 512, seed=11)
    _check(monkeypatch, comp, 512, 512, passes=2)


def test_rows_of_one_run_and_blocks_of_one_digit(monkeypatch):
    """one long, nearly horizontal edge (512 segments, a new tile column every 16: rows of four runs of distinct digits) and
    slivers 500 pixels tall inside one pixel column each, seven of them in one tile column: 7 000 consecutive segments of one
    first digit — rows of a single run, whole blocks of one digit"""
    comp = api.Composition()
    _fill(comp, 0, [(0.5, 300.2), (511.5, 300.9), (511.5, 303.0), (0.5, 302.5)], (0.7, 0.1, 0.2, 1.0))
    for i in range(7):
        x = 100.1 + 2.0 * i
        _fill(comp, 1 + i, [(x, 5.5), (x, 505.5), (x + 0.8, 505.5), (x + 0.8, 5.5)], (0.1, 0.2 + 0.1 * i, 0.6, 1.0))
    _fill(comp, 8, [(400.3, 20.5), (440.2, 470.5), (402.7, 475.5)], (0.2, 0.7, 0.2, 1.0))
    _check(monkeypatch, comp, 512, 512, passes=2)


def _trim_base():
    comp = api.Composition()
    _zigzag(comp, 0, 256.0, 12.0, 3.0, 8, 500, (0.8, 0.2, 0.1, 1.0))
    _tiny_triangles(comp, 1, 400, 512, 512, seed=12)
    return comp, 401


@pytest.fixture(scope="module")
def trim_base_segments():
    """pixel segments of the untrimmed scene (counted by the library: one synchronous frame)"""
    comp, _ = _trim_base()
    image = np.zeros((512, 512 * 4), np.uint8)
    r = api.Renderer(device=0)
    try:
        r.render(comp, api.BufferBuilder(image.reshape(-1), api.LinearLayout(512, 512 * 4, 512)).build(), api.RGBA,
                 api.Color(*CLEAR), None)
        _img, tm = r._ctx.render(512, 512, clear=CLEAR, timings=True)
        return int(tm["n_segments"])
    finally:
        r._ctx.close()


@pytest.mark.parametrize("last_block", [1, 63, 64, 65, 2047])
def test_keys_in_the_last_block(monkeypatch, trim_base_segments, last_block):
    """the scene, then slivers whose line lengths bring the stream to `last_block` keys beyond a multiple of 2 048.  A vertical
    line at a fractional x from y = 10.5 to 10.5 + k owns k + 1 pixel segments, so a sliver of two owns 2 k + 2; a three-line
    sliver with a vertex at height 1 owns 2 k + 3."""
    comp, order = _trim_base()
    need = (last_block - trim_base_segments) % 2048
    if need < 64:
        need += 2048
    col = 0
    if need & 1:
        x = 300.25
        _fill(comp, order, [(x, 10.5), (x + 0.25, 12.5), (x + 0.5, 11.5)])
        need -= 7; order += 1; col += 1
    while need:
        c = min(need, 600)
        if need - c == 2:
            c -= 2
        k = c // 2 - 1
        x = 300.25 + 2.0 * col
        _fill(comp, order, [(x, 10.5), (x, 10.5 + k), (x + 0.5, 10.5 + k), (x + 0.5, 10.5)])
        need -= c; order += 1; col += 1
    ref = _check(monkeypatch, comp, 512, 512, passes=2)
    assert int(ref["tm"]["n_segments"]) % 2048 == last_block, ref["tm"]["n_segments"]


def _far_right(comp, y0, y1, seed):
    """shapes whose tile_x + 1 crosses 256 (x around 4 080)"""
    rng = np.random.default_rng(seed)
    for i in range(300):
        x, y = float(rng.uniform(3900, 4090)), float(rng.uniform(y0, y1))
        s = float(rng.uniform(4, 18))
        _fill(comp, i, [(x, y), (x + s, y + s / 3), (x + s / 2, y + s)], (0.2, 0.4, (i % 7) / 7.0, 1.0))


def test_wide_canvas_4112_by_64(monkeypatch):
    comp = api.Composition()
    _far_right(comp, 1, 45, seed=13)
    _check(monkeypatch, comp, 4112, 64, extra=",digit_bits=8", passes=2)


def test_biased_first_digit(monkeypatch):
    """8-bit digits, tile_x + 1 and tile_y + 1 both across 256: three plain passes, two relative to the fields' minima — the
    fused first digit is tile_x - min.  (The oracle's stream; the 16.9-megapixel image against the unfused frame's.)"""
    comp = api.Composition()
    _far_right(comp, 3900, 4090, seed=14)
    _check(monkeypatch, comp, 4112, 4112, extra=",digit_bits=8", passes=2, oracle_image=False)
    plain = _run(monkeypatch, "fuse_digit=0,digit_bits=8,no_bias", comp, 4112, 4112)
    assert int(plain["tm"]["n_sort_passes"]) == 3, plain["tm"]["n_sort_passes"]


def test_layers_out_of_paint_order(monkeypatch):
    """256 layers inserted against paint order: the layer digit (the key's low word) is the plan's first, fused digit"""
    rng = np.random.default_rng(5)
    orders = rng.permutation(256)
    comp = api.Composition()
    for i in range(256):
        x, y = float(rng.uniform(0, 440)), float(rng.uniform(0, 440))
        s = float(rng.uniform(8, 60))
        comp.get_mut_or_insert_default(int(orders[i])).insert(
            api.PathBuilder().move_to(api.Point(x, y)).line_to(api.Point(x + s, y + s / 3))
            .line_to(api.Point(x + s / 2, y + s)).build()).set_props(scenes._solid(api.Color(0.2, 0.4, (i % 7) / 7.0, 1.0)))
    _check(monkeypatch, comp, 512, 512, passes=3)


# ---- the cases of test_gpu_fused_digit.py under the other two rank forms.  That file sets FORMA_HIP_DEBUG itself, so a switch in
# the environment of a whole-suite run does not reach it: its comparison runs here with the switch appended to both of its strings.
_FD_CASES = {
    "stand-in-1080p": lambda: (scenes.paris_like(n_layers=3000, width=1920, height=1080), 1920, 1080, 2, ""),
    "cubics-720p": lambda: (scenes.random_cubics(n=400, width=1280, height=720, seed=71), 1280, 720, 2, ""),
    "biased-8192": lambda: (None, 8192, 8192, 2, ",digit_bits=8"),
    "out-of-paint-order-4k": lambda: (None, 3840, 2160, 3, ""),
}


@pytest.mark.parametrize("rank", ["ras_rank=0", "ras_rank=2"])
@pytest.mark.parametrize("case", sorted(_FD_CASES))
def test_fused_digit_cases_under_the_other_rank_forms(monkeypatch, case, rank):
    from tests import test_gpu_fused_digit as fd
    comp, w, h, passes, extra = _FD_CASES[case]()
    if case == "biased-8192":
        comp = fd._triangles(500, 3600, 4500, 3600, 4500, seed=8)
    elif case == "out-of-paint-order-4k":
        comp = fd._triangles(256, 0, 3700, 0, 2000, seed=6, orders=np.random.default_rng(5).permutation(256))
    fd._same_both_ways(monkeypatch, comp, w, h, passes=passes, extra=extra + "," + rank)
