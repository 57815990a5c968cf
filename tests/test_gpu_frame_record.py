"""The frame in flight has one record (csrc/ctx.h: `Guesses`, `HandOffs`, `Enqueued`, the `FrameMode` argument): nothing a frame
guessed, handed from stage to stage or left for its delivery reaches the next frame of the same context.  A 96 x 80 canvas (no
multiple of the tile size, five tile rows) and the dozen layers of test_gpu_context_state.py; every frame bit for bit the same
request on a fresh one-slot context, that context's plain frame against the oracle within the parity contract's one RGBA8 step."""
import numpy as np
import pytest

import scene as S
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

W, H = 96, 80
TILES_H = (H + 15) // 16
CLEAR = (1.0, 1.0, 1.0, 1.0)
CROP = (16, 80, 16, 64)
POINT = (np.zeros(1, np.float32), np.zeros(1, np.float32), np.zeros(0, np.uint32))   # one point: no line, an empty stream


# ---- the requests: each returns the image the caller sees
def device(c):
    c.render(W, H, clear=CLEAR, device_only=True)
    return c.read_image(W, H)


def into_dst(c):
    return c.render(W, H, clear=CLEAR, dst=np.full((H, W * 4), 7, np.uint8))


def cropped_cache(c):
    return c.render(W, H, clear=CLEAR, crop=CROP, cache_id=0, dst=np.full((H, W * 4), 7, np.uint8))


def stages(c):
    """forma_hip_rasterize_frame, the stream handed back through _reserve_segments, _sort_paint_frame"""
    import torch
    c.rasterize_frame(W, H)
    seg = c.unsorted_view()
    recv = c.reserve_view(int(seg.numel()))
    recv.copy_(seg)
    torch.cuda.synchronize()
    return c.sort_paint_frame(int(recv.numel()), W, H, clear=CLEAR, device_only=False)


def parity_paint(c):
    """forma_hip_paint of the last frame's sorted stream, read back"""
    return c.paint(c.segments(1), W, H, clear=CLEAR)


def empty_geometry(c, t):
    c.set_geometry(*POINT)
    img = device(c)
    c.set_geometry(t["x"], t["y"], t["line_slot"])
    return img


def fresh(t, *requests):
    """the images of `requests` on a new one-slot context"""
    import forma_amd
    c = forma_amd.Context(0)
    try:
        S.load(c, t)
        return [r(c) for r in requests]
    finally:
        c.close()


@pytest.fixture(scope="module")
def ref():
    """the scene's tables and what a fresh context renders for every kind of request: computed once, read only"""
    o = orc.Oracle()
    comp = S.random_cubics(n=12, width=W, height=H, seed=5, alpha=0.8)
    t = comp.tables(o)
    S.load(o, t)
    want = {}
    want["device"], = fresh(t, device)
    d = int(np.abs(want["device"].astype(int) - o.render(W, H, clear=CLEAR).astype(int)).max())
    print("fresh context against the oracle: max difference", d)
    assert d <= 1
    want["empty"], = fresh(t, lambda c: empty_geometry(c, t))
    assert (want["empty"] == 255).all()
    want["dst"], = fresh(t, into_dst)
    want["crop1"], want["crop2"] = fresh(t, cropped_cache, cropped_cache)
    want["stages"], = fresh(t, stages)
    _, want["paint"] = fresh(t, device, parity_paint)
    for k in ("dst", "stages", "paint"):
        assert np.array_equal(want[k], want["device"]), k
    return t, want


def same(got, want, what):
    assert np.array_equal(got, want), (what, int((got != want).sum()))


def resident_and_dst(c, t, want, what):
    """three device-resident frames (the third read-back-free), the empty stream, the scene again, two frames into `dst`"""
    for k in range(3):
        same(device(c), want["device"], (what, "device", k))
    same(empty_geometry(c, t), want["empty"], (what, "empty"))
    same(device(c), want["device"], (what, "device after empty"))
    for k in range(2):
        same(into_dst(c), want["dst"], (what, "dst", k))


def test_nothing_leaks_from_one_frame_into_the_next(ref):
    """Every kind of frame on ONE context, then the first again: each image is the fresh context's.  A prediction that fails costs a
    re-run: the parent commit's library re-runs 0 frames of this sequence, and so may this one."""
    import forma_amd
    t, want = ref
    c = forma_amd.Context(0)
    try:
        S.load(c, t)
        before = c.counters()["frames_rerun"]
        resident_and_dst(c, t, want, "first")
        same(cropped_cache(c), want["crop1"], "crop, cache 0")
        same(cropped_cache(c), want["crop2"], "crop, cache 0, again")
        same(stages(c), want["stages"], "rasterize_frame + sort_paint_frame")
        same(device(c), want["device"], "device after the stage calls")
        same(parity_paint(c), want["paint"], "paint")
        same(into_dst(c), want["dst"], "dst")
        for k in range(3):
            same(device(c), want["device"], ("device, at the end", k))
        grew = c.counters()["frames_rerun"] - before
        print("frames_rerun grew by", grew)
        assert grew <= 0
    finally:
        c.close()


@pytest.mark.parametrize("switches", ["fuse_digit=2", "runs_chain=1", "runs_blk=1,runs_chain=0,blk_round=2", "paint_split=3", "order_thr=0",
                                      "no_prezero", "poison_frame=165"])
def test_the_paths_that_carry_the_hand_offs(ref, monkeypatch, switches):
    """the device-resident and `dst` frames under the switches that force a fused digit, the chain and BLOCKS numbering, split
    bands, the heavy-first order, no clearing ahead and poisoned frame buffers: the default context's images"""
    import forma_amd
    t, want = ref
    monkeypatch.setenv("FORMA_HIP_DEBUG", switches)
    c = forma_amd.Context(0)
    try:
        S.load(c, t)
        resident_and_dst(c, t, want, switches)
    finally:
        c.close()


def test_frame_slots(ref):
    """nine device-resident frames on three slots, the empty stream among them: every slot enqueues at least twice"""
    import forma_amd
    t, want = ref
    c = forma_amd.Context(0, frames_in_flight=3)
    try:
        S.load(c, t)
        for k in range(4):
            same(device(c), want["device"], ("slots", k))
        same(empty_geometry(c, t), want["empty"], "slots, empty")
        for k in range(4):
            same(device(c), want["device"], ("slots, after empty", k))
    finally:
        c.close()


@pytest.mark.parametrize("switches", ["", "xgather"])
def test_the_exchange_hands_over_across_two_calls(ref, monkeypatch, switches):
    """a one-rank plan: from the second frame on both calls are read-back-free, and what forma_hip_rasterize_bucket_frame's first
    kernel cleared is taken by forma_hip_gather_sort_paint_frame"""
    import forma_amd
    t, want = ref
    if switches:
        monkeypatch.setenv("FORMA_HIP_DEBUG", switches)
    c = forma_amd.Context(0)
    try:
        S.load(c, t)
        c.rasterize_frame(W, H)
        n = len(c.segments(0))
        c.exchange_plan([0, TILES_H], 2 * n + 4096)
        for k in range(4):
            c.rasterize_bucket_frame(W, H)
            c.gather_sort_paint_frame(W, H, clear=CLEAR)
            same(c.read_image(W, H), want["device"], ("exchange", switches, k))
    finally:
        c.close()


def test_a_frame_without_runs_records_its_own_plan(ref, monkeypatch):
    """carry_slices=3: the scene's frames settle on three slices; the empty frame has no runs, settles nothing and records the plan
    it made (one slice) instead of keeping the frame before's; the scene comes back without a re-run"""
    import forma_amd
    t, want = ref
    monkeypatch.setenv("FORMA_HIP_DEBUG", "carry_slices=3")
    c = forma_amd.Context(0)
    try:
        S.load(c, t)
        for k in range(3):
            same(device(c), want["device"], ("carry_slices=3", k))
        same(empty_geometry(c, t), want["empty"], "carry_slices=3, empty")
        before = c.counters()["frames_rerun"]
        for k in range(3):
            same(device(c), want["device"], ("carry_slices=3, after empty", k))
        assert c.counters()["frames_rerun"] == before
    finally:
        c.close()
