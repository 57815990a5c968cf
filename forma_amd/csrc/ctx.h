// ctx.h — the context behind the C ABI (include/forma_hip.h), shared by api.cpp (one device) and multi.cpp (several
// devices behind one context).  Private to libforma_hip.so.
#pragma once
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <utility>
#include <vector>

#include "common.h"
#include "debug.h"
#include "geom_edit.h"

struct DevBuf {
    void* p = nullptr;
    size_t cap = 0;
    bool borrowed = false;                  // a frame slot's view of its owner's scene buffer: never grown or freed here
    hipError_t ensure(size_t bytes) {
        if (bytes <= cap && p) return hipSuccess;
        if (borrowed) return hipErrorInvalidValue;
        size_t want = std::max(bytes, cap + cap / 2);
        want = std::max<size_t>(want, 256);
        if (p) { hipError_t e = hipFree(p); p = nullptr; cap = 0; if (e != hipSuccess) return e; }
        hipError_t e = hipMalloc(&p, want);
        if (e == hipSuccess) {
            cap = want;
            // FORMA_HIP_DEBUG=poison=<byte>: every fresh device allocation is filled with that byte — a kernel that reads what
            // nothing wrote this frame then misbehaves on every run instead of once per fresh box (tests/, tools/)
            static const int poison = forma_debug_parse().poison;
            if (poison >= 0) { e = hipMemset(p, poison, want); if (e == hipSuccess) e = hipDeviceSynchronize(); }
        }
        return e;
    }
    // growth that KEEPS the first `used` bytes (the geometry store is appended to): a device-to-device copy into the new
    // allocation on `s`, which is drained before the old one is freed; geometric like ensure
    hipError_t grow_keep(size_t bytes, size_t used, hipStream_t s) {
        if (bytes <= cap && p) return hipSuccess;
        if (borrowed) return hipErrorInvalidValue;
        size_t want = std::max(bytes, cap + cap / 2);
        want = std::max<size_t>(want, 256);
        void* q = nullptr;
        hipError_t e = hipMalloc(&q, want);
        if (e != hipSuccess) return e;
        static const int poison = forma_debug_parse().poison;
        if (poison >= 0) e = hipMemsetAsync(q, poison, want, s);
        used = std::min(used, cap);
        if (e == hipSuccess && p && used) e = hipMemcpyAsync(q, p, used, hipMemcpyDeviceToDevice, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        if (e != hipSuccess) { (void)hipFree(q); return e; }
        if (p) (void)hipFree(p);
        p = q; cap = want;
        return hipSuccess;
    }
    void release() { if (p && !borrowed) (void)hipFree(p); p = nullptr; cap = 0; borrowed = false; }
    void borrow(const DevBuf& o) { release(); p = o.p; cap = o.cap; borrowed = true; }
    template <class T> T* as() const { return (T*)p; }
};

// page-locked host memory that grows on demand and is kept: to exactly `bytes`, to at least `min_bytes`, or geometrically
struct PinnedBuf {
    void* p = nullptr;
    size_t cap = 0;
    hipError_t ensure(size_t bytes, size_t min_bytes = 0, bool geometric = false) {
        if (bytes <= cap && p) return hipSuccess;
        const size_t want = std::max(std::max(bytes, min_bytes), geometric ? cap + cap / 2 : 0);
        release();
        const hipError_t e = hipHostMalloc(&p, want, hipHostMallocDefault);
        if (e == hipSuccess) cap = want; else p = nullptr;
        return e;
    }
    void release() { if (p) (void)hipHostFree(p); p = nullptr; cap = 0; }
    template <class T> T* as() const { return (T*)p; }
};

constexpr uint32_t PAINT_WAVES_PER_CU = 24;     // wave slots of the general painter per CU (6 per SIMD): frames of at most n_cus x 24 painted
                                                // tiles — every tile gets a slot at once — are painted by strips (api.cpp paint_by_strips)
constexpr size_t SEG_PAD = 16;          // segment buffers are over-allocated: stream kernels read whole 64-byte lane pieces
enum { ST_PREPARE = 0, ST_RASTER, ST_SORT, ST_CARRY, ST_PAINT, ST_D2H, ST_XCHG, ST_COUNT };

struct PaintArgs {
    uint32_t width, height;
    const uint8_t* channels;
    const float* clear;
    const forma_rect_t* crop;
    int cache_id = -1;
    // forma_hip_render_device: the painters write straight into the caller's device memory (pitch in bytes, FORMA_FORMAT_*);
    // nullptr: into the context's scratch image or the cache's own image, as RGBA8
    uint8_t* target = nullptr;
    size_t target_pitch = 0;
    uint32_t fmt = FORMA_FORMAT_SRGB8;
    uint32_t tiles_w() const { return (width + 15) / 16; }  uint32_t tiles_h() const { return (height + 15) / 16; }
};

// One frame as its caller asked for it.  It OWNS its arguments (the caller's arrays need not outlive the call: a frame in flight
// is parked in its slot, forma_hip_ctx::parked) and hands out the PaintArgs view of itself — valid while the request stays put.
struct FrameRequest {
    uint32_t width = 0, height = 0;
    uint8_t channels[4] = {0, 1, 2, 3};
    float clear[4] = {0, 0, 0, 0};
    bool has_crop = false;
    forma_rect_t crop = {0, 0, 0, 0};
    int cache_id = -1;
    uint8_t* target = nullptr; size_t target_pitch = 0; uint32_t fmt = FORMA_FORMAT_SRGB8;   // forma_hip_render_device: the caller's device target
    uint8_t* dst = nullptr; size_t stride = 0;              // the frame also travels to caller memory
    forma_timings_t* timings = nullptr;
    uint32_t bN = 0, bJ = 0;                                // a read-back-free frame: the bounds its buffers were provisioned for
    FrameRequest() = default;
    FrameRequest(uint8_t* dst_, uint32_t w, uint32_t h, size_t stride_, const uint8_t ch[4], const float clear_[4], const forma_rect_t* crop_or_null,
                 int cache, forma_timings_t* t) : width(w), height(h), has_crop(crop_or_null != nullptr), cache_id(cache), dst(dst_), stride(stride_), timings(t) {
        memcpy(channels, ch, 4); memcpy(clear, clear_, 16);
        if (crop_or_null) crop = *crop_or_null;
    }
    PaintArgs paint() const { return PaintArgs{width, height, channels, clear, has_crop ? &crop : nullptr, cache_id, target, target_pitch, fmt}; }
    bool timing() const { return timings != nullptr; }
};

// What the uploaded scene IS, as far as the frame path needs scalars of it.  Written by the scene setters on the owner of the
// frame slots; share_scene hands the whole struct to every slot with the borrowed buffers, so a fact added here reaches them all
// (layer-table edits: a slot's n_geoms and max_geom_order then follow the table it holds, tables_catch_up).
struct SceneFacts {
    size_t n_points = 0, n_geoms = 0, n_orders = 0, n_words = 0, n_images = 0;
    uint32_t max_geom_order = 0;            // largest order any geom slot names (FORMA_NONE slots aside)
    uint32_t max_image_index = 0;           // largest image index a texture style names
    bool any_texture = false;
    bool scene_has_clips = false;
    bool scene_simple = false;              // all layers solid + Over + unclipped: the painter's specialised kernel
    size_t costly_layers = 0;               // layers with a gradient / texture fill, a blend mode other than Over, or clipped (strip painters: api.cpp)
    bool have_unchanged = false;            // set_styles supplied per-order Layer::is_unchanged bytes
    uint32_t band_row0 = 0, band_row1 = 0;  // band
    // a sub-range [line_lo, line_hi) of the uploaded lines (line i joins points i and i + 1) when line_ranged.
    // A multi-device context uploads the whole geometry to every device and gives each its share of the LINES (multi.cpp).
    bool line_ranged = false;
    size_t line_lo = 0, line_hi = 0;
};

// What verified frames taught a context (every frame slot learns for itself), and the events that un-teach it.  Read-back-free
// frames are enqueued under these predictions and checked against them on the device; a synchronous frame re-learns them.
struct Learned {
    // sort-plan speculation: the varying-bit mask and the layer-sortedness of a scene rarely change between frames, so a frame
    // plans its sort from the previous frame's values and verifies them when it is done (verify_speculation writes all three)
    bool pred_valid = false, pred_layer_sorted = false;
    uint64_t pred_live44 = 0;
    // counts.  pred_N / pred_J: a frame's segments and runs (run_sync, judge_frame); pred_counts_valid: set by run_sync, dropped by
    // judge_frame with a void frame; pred_w / pred_h: own_canvas.  xpred_*: the local count of the last bucket frame of the
    // exchange layout and its canvas (forma_hip_rasterize_bucket_frame, bucket_canvas)
    bool pred_counts_valid = false, xpred_valid = false;
    uint32_t pred_N = 0, pred_J = 0, pred_w = 0, pred_h = 0;
    uint32_t xpred_N = 0, xpred_w = 0, xpred_h = 0;
    // shapes of the last verified frame
    uint32_t pred_max_row = 0xFFFFFFFFu;    // most runs in one tile row (unknown: no local sort): judge_frame, replan_carry
    uint32_t pred_row_spans = 0;            // spans per painted tile row: group lists pay above SPAN_GROUP_MIN_ROW (finish_frame)
    uint32_t pred_slice_n = 0, pred_max_slice = 0;              // carry slices per tile row and the most runs in one (finish_frame)
    bool pred_slice_small = false, pred_slice_half = false;     // ... under the small / the 512-lane carry kernel (finish_frame)
    uint32_t pred_slice_len = 0;            // mean keys per (digit, block) slice of the last fused frame, 0: not measured (finish_frame)
    bool pred_no_deep = false;              // it sent no tile to k_paint_deep (finish_frame)
    KeyRange pred_range{0, 0, 0, 0, false}; // what its tile fields spanned (value-range digits, SortPlan::bias): finish_frame
    // bans and probes
    bool small_banned = false, covl_banned = false;   // a frame that guessed the small / the COVL carry variant was void (judge_frame)
    uint32_t bias_banned = 0, bias_ban_len = 0;       // frames left of a ban on biased digits (judge_frame counts down) / length of the last one: re-armed
                                                      // with back-off by ban_bias — an animated scene that left its span once gets the cheaper plan back
    uint32_t fuse_skipped = 0;              // frames not fused since the slices were measured too short (fuse_first_digit, FUSE_PROBE)
    // painter steering (PaintParams::order_*, ::cull)
    struct OrderSig { uint32_t tiles_w = 0, tiles_h = 0, x0 = 0, x1 = 0, y0 = 0, y1 = 0;
                      bool operator==(const OrderSig& o) const { return tiles_w == o.tiles_w && tiles_h == o.tiles_h && x0 == o.x0 && x1 == o.x1 && y0 == o.y0 && y1 == o.y1; } };
    int order_cur = -1;                     // the set of order lists that is valid, -1: none (take_over_order; dropped by heavy_order, a void frame and trim)
    OrderSig order_sig;                     // ... and the canvas / crop it was written for (take_over_order)
    uint32_t order_flat = 0, order_off = 0; // frames in a row without a tail (take_over_order) / frames left with the order switched off (heavy_order counts down)
    uint32_t order_thr = 1u << 16;          // shader clocks that make a tile heavy, steered per frame (take_over_order)
    bool cull_on = false;                   // this geometry has had tiles beyond the wave painter's lists: occlusion culling is on (finish_frame)

    // new geometry, band, line range or trim: the next frame re-learns N and J synchronously, bans and steering start over
    void new_geometry() {
        pred_counts_valid = false; xpred_valid = false; small_banned = false; covl_banned = false; bias_banned = 0; bias_ban_len = 0; pred_range.valid = false;
        order_off = 0; order_flat = 0; order_cur = -1; cull_on = false; pred_slice_len = 0;
    }
    void store_edited() { xpred_valid = false; }            // (api.cpp geometry_edited says why the rest stays)
    void new_exchange_plan() { pred_valid = false; pred_counts_valid = false; xpred_valid = false; }
    // canvas changed: counts learned at another size predict nothing
    void own_canvas(uint32_t w, uint32_t h) { if (w != pred_w || h != pred_h) { pred_counts_valid = false; pred_w = w; pred_h = h; } }
    void bucket_canvas(uint32_t w, uint32_t h) { if (w != xpred_w || h != xpred_h) { xpred_valid = false; xpred_w = w; xpred_h = h; } }
};

// ---- the frame being enqueued right now: what belongs to it, by lifetime ("The context's state by owner") ----
// 1. An argument of ONE CALL: what enqueue_own knows about its frame, by value down to run_sort (sort_workgroups) and run_paint
//    (heavy_order, split_plan).  Default: every other caller (run_sync, enqueue_received, the stage entry points).
struct FrameMode {
    bool tail = false;                      // the frame ends with k_frame_tail: its painters may leave their order lists (heavy_order)
    bool may_split = false;                 // into caller memory and verified at once: the painter may run in bands (split_plan)
    bool has_dst = false;                   // a parked frame whose image leaves behind its kernels: its digit passes keep the whole chip (sort_workgroups)
};
// How the frame's runs are numbered (launch_runs) and which carry kernel orders them (launch_carry_rows): plan_carry, settle_carry
struct CarryPlan {
    bool local_sort = false;                // the rows' runs are ordered inside k_carry_rows (else by a global radix sort)
    bool chain = false, chain_zero = false, blk = false;   // numbered per tile row (its status words cleared by the frame's first kernel) / per 2 048-segment tile
    uint32_t rows_painted = 1, n_slices = 1;               // tile rows the carry pre-pass visits, its workgroups per row
    bool small = false, half = false, covl = false;        // the carry kernel's variant
};
// 2. The frame's GUESSES, written while it is enqueued and read back by its verdict
struct Guesses {
    bool speculated = false;                // the sort is planned from learned.pred_live44 / pred_layer_sorted (run_rasterize_frame, enqueue_received) — run_sort, number_runs, verify_speculation
    bool plan_biased = false;               // ... and leans on learned.pred_range (run_sort) — judge_frame: a void frame bans the bias
    CarryPlan plan;                         // the carry plan as run_paint settled it — judge_frame bans .small / .covl of a void frame, finish_frame
    bool read_back_free = false;            //   learns .rows_painted, .n_slices, .small, .half; ... and whether that frame was enqueued (bound_j != 0)
};
// 3. HAND-OFFS from one stage of a stream to a later one.  begin_stream (api.cpp) resets them all: "nothing handed over"; the stage
//    named first produces, the one named last TAKES — nobody else clears
template <class T> inline T take(T& x) { return std::exchange(x, T{}); }
struct Cleared {                            // words the frame's FIRST kernel cleared on behalf of a later stage (ZeroJobs, common.h)
    const void* p = nullptr; size_t words = 0;
    bool covers(const void* q, size_t n) const { return p == q && words >= n; }    // (else the stage clears for itself)
};
struct PreZero { Cleared sort, tab, chain, slice; };
struct HandOffs {
    PreZero pz;                             // plan_zero_jobs, through run_rasterize_frame — .sort: run_sort, .tab: run_paint, .chain: plan_carry (.slice is only read)
    bool ras_hist_on = false, ras_fused = false;   // the rasterizer counted the digits of ras_plan into the sort's histograms (RasHist) / and wrote its blocks
    SortPlan ras_plan{};                           //   partitioned by that plan's first digit (SliceSrc): run_rasterize_frame — run_sort, if its plan is the same
    const uint32_t* sort_range = nullptr; uint32_t sort_range_n = 0;   // run_sort: the tile-field spans it leaves behind, a record per k_sort_hist workgroup — number_runs
    PendingMasks pending_masks{nullptr, 0u, 0u};   // key masks per workgroup that nobody has combined (run_rasterize_frame, enqueue_received) — number_runs
    const uint32_t* chain_rows = nullptr; uint32_t n_chain_rows = 0;   // number_runs: runs numbered per tile row or tile, the row counts — frame_tail sums them
    const uint32_t* order_cnt_dev = nullptr; uint32_t* order_keep_dev = nullptr;   // heavy_order: the order counts and where they are kept — frame_tail copies
};
// 4. What run_paint's frame LEFT BEHIND for its verification and delivery: reset as a whole when run_paint starts.  Every member is
//    dead by then — its readers run between this frame's run_paint and its delivery — and split_sent is false: every path from
//    send_split_bands to the next frame passes settle_split (enqueue_own, judge_frame, deliver), a failed wait for the stream aside
constexpr int SPLIT_MAX = 8;
struct Enqueued {
    int order_pending = -1;                 // heavy_order: the set of order lists this frame's painters write (-1: none) — take_over_order, a void frame (judge_frame)
    Learned::OrderSig order_pending_sig; uint32_t order_tiles = 0;   // ... the canvas / crop they are for, the tiles painted (heavy_order) — take_over_order
    int split_n = 0; uint32_t split_row[SPLIT_MAX + 1] = {};         // run_paint: bands of the painter (0: not split), their tile-row boundaries — send_split_bands
    bool split_sent = false;                // send_split_bands: copies are on copy_stream, wait for it before `dst` is touched again — settle_split
    bool image_sent = false;                // send_split_bands, enqueue_own: the image left behind the kernels, before the frame was verified — deliver
    struct HugeArgs { PaintParams P; DevCount jc; TileCacheArgs tc; uint32_t fmt; } huge{};   // run_paint: what of the painter launch the context does not hold — finish_paint
};

struct forma_hip_ctx {
    int device = 0;
    uint32_t n_cus = 256;                   // hipDeviceProp_t::multiProcessorCount of `device` (MI355X: 256)
    hipStream_t stream = nullptr;
    char err[512] = {0};

    // scene
    DevBuf x, y, line_slot, geoms, style_off, style_words, unchanged, images, texels;
    DevBuf layer_sf, layer_col;             // per order: style summary for the carry pre-pass (set_styles)
    std::vector<uint32_t> h_layer_sf, h_layer_col;
    SceneFacts scene;
    // the geometry store as an incremental store (forma_hip_geometry_append / _retain): line_slot holds n_points entries on
    // the device, the last one FORMA_NONE (frames use n_points - 1 of them); retain compacts into the spare set and swaps
    DevBuf x_spare, y_spare, line_slot_spare;
    DevBuf geo_blob;                        // one append's work items / one retain's tables, as uploaded
    DevBuf geo_flag;                        // k_geom_retain: a stored slot beyond the remap table
    DevBuf stroke_tmp;                      // a stroked append: its flattened source points, their output counts, the scan's sums and total
    PinnedBuf h_geo;                        // staging of geo_blob (grown geometrically, kept); its first word receives geo_flag
    // the layer table edited with frames in flight (forma_hip_update_geoms / _update_geoms_xf; api.cpp "layer-table edits").
    // The OWNER of the frame slots keeps the table on the host (h_tab: always, forma_hip_read_geoms answers from it) and, from
    // the first edit call on (tab_on), a journal of what changed at which sequence number; every slot then owns a table
    // (geoms_own; `geoms` is a view of it) and brings it up to date on its own stream when its next frame starts.
    std::vector<forma_geom_t> h_tab;        // owner: the table the NEXT frame will see
    bool tab_on = false;                    // owner: an edit call has been made — the slots own their tables
    uint32_t tab_max_order = 0;             // owner: max_geom_order of h_tab (a slot takes it over with the table)
    uint64_t tab_seq = 0, tab_full_seq = 0; // owner: number of the last edit / a slot that has seen less than tab_full_seq copies the whole table
    std::vector<uint64_t> tab_ent_seq;      // owner, per table slot: the last edit that replaced the whole entry
    struct TabEnt { uint64_t seq; uint32_t slot; };
    struct TabRng { uint64_t seq; uint32_t first, count, has_xf; float xf[6]; };
    std::vector<TabEnt> tab_ent_log;        // owner: entry edits, ascending seq (an item is stale when tab_ent_seq[slot] is newer)
    std::vector<TabRng> tab_rng_log;        // owner: _xf ranges, ascending seq; a range that a later one covers is dropped
    uint64_t tab_seen = 0;                  // every slot: the edit its table is up to date with
    DevBuf geoms_own;                       // every slot, the owner included: its table
    DevBuf geoms_shared;                    // owner: the table the slots shared before the first edit call (frames enqueued then still read it)
    DevBuf tab_blob;                        // every slot: one catch-up's records on the device
    PinnedBuf h_tab_stage;                  // every slot: the records / the whole table on their way (free again once the slot's frame is settled)
    forma_counters_t cnt{};                 // forma_hip_counters (frame counters: kept by the owner of the frame slots)
    DevBuf run_lt;                  // one word per run: layer16 | open | tile_x + 1 (RunStyle, common.h)
    DevBuf rec_sp, run_lt_sp, row_sp;       // launch_runs' BLOCKS numbering (BlkRuns, common.h): records and digests indexed like the segments (N entries)
    DevBuf grp_tab, grp_list;       // span group lists (SpanGroups, common.h): table per (row, slice, group) and the entry pool
    // lines
    DevBuf l_order, l_x0, l_y0, l_dx, l_dy, l_a, l_b, l_c, l_d, l_len, scan_tmp;   // parity entry points only
    DevBuf cl_idx, cl_start, block_first, prep_scratch;                              // frame path: compacted line table
    // the painters' heaviest-first order (PaintParams::order_*): two sets of {counts, lists}; a read-back-free frame reads the set
    // the last verified frame of the same canvas / crop wrote and writes the other one
    DevBuf order_buf;
    DevBuf slice_buf;                       // fused first digit pass (SliceSrc): slice table, tiles' first slices, slice list
    DevBuf ras_masks;                       // k_rasterize: key masks per workgroup (8 words), combined by k_reduce_masks or, on read-back-free frames, by k_runs_count
    size_t n_lines = 0, n_compact = 0;
    // segments
    DevBuf seg_u, seg_a, seg_b, sort_counters;
    uint64_t* sorted = nullptr;
    size_t n_seg = 0;
    bool have_unsorted = false;
    uint64_t live44 = 0xFFFFFFFFFFFull;     // varying bits of (v >> 20)
    bool layer_sorted = false;              // rasterizer stream is non-decreasing in layer
    // paint
    DevBuf info_init;                       // pristine FrameInfo (reset template)
    // buffer-layer caches (reference cpu/buffer/mod.rs:113-197): per cache the CachedTile table, the device image the
    // cache's buffer shows (tiles the painter skips keep last frame's pixels), and the cached clear colour
    struct TileCache {
        DevBuf tiles, image;
        uint32_t w = 0, h = 0;
        bool has_clear = false;
        float clear[4] = {0, 0, 0, 0};
        // what the cache last painted into: its own image (nullptr) or a caller's device target (forma_hip_render_device) with
        // its pitch.  A BufferLayerCache belongs to one Buffer: when the target changes, the tile state is cleared
        const void* target = nullptr; size_t target_pitch = 0;
    };
    TileCache caches[32];
    DevBuf pack_list, pack_pix;             // cache frames: written tiles of the crop (list + count word in front), their pixels packed
    DevBuf cache_written;                   // one byte per tile: written this frame
    PinnedBuf h_written;                    // copy of cache_written
    PinnedBuf h_stage;                      // staging image for tile-granular copy-out (released by trim: a whole 4K image after a cache frame)
    // A synchronous frame into caller memory (one frame in flight, no cache): the painter runs as two launches (tests: up to SPLIT_MAX) over
    // bands of tile rows, each followed by an event; the bands' copies go out on `copy_stream` behind those events, so the image
    // crosses PCIe while the rest of it is still being painted (api.cpp: run_paint, send_split_bands).
    hipStream_t copy_stream = nullptr;      // created on first use
    hipEvent_t  split_ev[SPLIT_MAX] = {};
    std::vector<std::pair<void*, size_t>> registered;   // caller buffers pinned by forma_hip_register_buffer
    int cur_cache = -1;                     // cache of the frame in flight
    uint8_t* cur_image = nullptr;           // device image of the frame in flight / last frame
    bool image_external = false;            // ... is the caller's device target (forma_hip_render_device): forma_hip_read_image refuses it
    hipEvent_t wait_ev = nullptr;           // forma_hip_render_device's wait_stream: recorded there, waited for on the frame's stream
    Learned learned;                        // what verified frames taught this slot
    Guesses guess;                          // the frame being enqueued: what it guessed,
    HandOffs hand;                          //   what its stages hand to one another,
    Enqueued left;                          //   and what it leaves for its verification and delivery
    bool seg_u_fused = false; uint32_t fused_w = 0, fused_h = 0;   // seg_u holds a fused frame's partitioned blocks (restore_unsorted)
    DevBuf info, records, rk_u, rk_a, rk_b, blk_edge, runs_scratch, row_tab, span_key, span_cov, image;
    uint32_t img_w = 0, img_h = 0;
    FrameInfo* h_info = nullptr;            // pinned
    uint32_t*  h_seq = nullptr;             // pinned (behind h_info): the number of the last read-back-free frame whose k_frame_tail has run
    uint32_t   tail_seq = 0;                // ... and of the last one enqueued
    bool info_clean = false;                // the device FrameInfo is pristine: the last frame ended with k_frame_tail (reset_info is then free)
    ForMaDebug dbg;                         // FORMA_HIP_DEBUG as it stood when the context was created (a frame slot: its owner's) — the switches' one home
    // radix digit width: 0 = 8, or 9 where that saves a pass (default); 4 / 8 / 9 forced (digit_bits=)
    int digit_bits() const { return dbg.digit_bits == 4 || dbg.digit_bits == 8 || dbg.digit_bits == 9 ? dbg.digit_bits : 0; }
    // carry_slices=N: that many workgroups per tile row in the carry pre-pass (0: by policy)
    uint32_t force_slices() const { return dbg.carry_slices > 0 ? (uint32_t)std::min(dbg.carry_slices, (int)CR_MAX_SLICES_HOST) : 0u; }
    uint32_t* h_rows = nullptr;             // pinned: runs per tile row (synchronous frames), 2049 words
    DevBuf huge_offs, huge_key, huge_tmp, huge_flag;   // finish_paint: the scratch lists of tiles deeper than the painter's LDS lists (Enqueued::huge)
    // frames in flight inside ONE context (forma_hip_set_frames_in_flight): slots[0] is the context itself, the others are
    // full contexts (own stream, own per-frame buffers) that BORROW the scene buffers.  A device-resident, cache-less frame
    // is enqueued on the next slot and verified when that slot is needed again (or at any call that needs the result).
    forma_hip_ctx* owner = nullptr;         // extra slots: the context they belong to
    std::vector<forma_hip_ctx*> slots;      // of the owner (empty = one frame in flight)
    unsigned next_slot = 0;
    forma_hip_ctx* last = nullptr;          // the slot that holds the most recent frame (inspection calls read it)
    bool pending = false;                   // this slot holds an enqueued frame nobody has verified yet
    FrameRequest parked;                    // ... that frame (and the exchange frame of `xpending`)
    // several devices behind this context (forma_hip_create_multi): the context is then a shell, the work happens in
    // multi->kid[g] (one full context per device)
    struct MultiState* multi = nullptr;
    // multi-GPU exchange (forma_hip_exchange_plan): owner bands, per-pair capacity, send / receive buckets and their counts
    OwnerBands xbands{};
    uint32_t xcap = 0;
    bool xplanned = false;
    DevBuf xsend, xrecv, xscratch, xmask;         // buckets: n_ranks x (xcap data words + 1 header word {count | overflow << 32})
    bool xpending = false;                    // a deferred owner's half (fd_gsp_defer) nobody has settled yet
    bool xoverflowed = false;                 // the last owner's half failed because a bucket outgrew the plan (FORMA_E_CAPACITY: re-plan)
    bool xuse_recv = false;                   // one rank, but a collective DID run (RCCL rehearsal): the buckets are in xrecv
    uint32_t* h_xlocal = nullptr;           // pinned: [0] = local segment count of the last bucket frame (copied on the stream), [1] = 1 when pending
    // timing
    hipEvent_t ev0[ST_COUNT], ev1[ST_COUNT];
    KernelTimer kt;                          // per-kernel events of a timed frame (FORMA_LAUNCH, common.h) ...
    float kt_dur_us[KernelTimer::CAP] = {0}, kt_start_us[KernelTimer::CAP] = {0}; int kt_n_done = 0;   // ... resolved by finish_frame
    bool stage_used[ST_COUNT];
    int n_passes = 0;
    uint32_t last_runs = 0, last_entries = 0, last_written = 0;
    // what the last frame wrote, for forma_hip_tiles_written (host-side Flusher / generic Layout::write)
    uint32_t lw_tiles_w = 0, lw_tiles_h = 0, lw_tx0 = 0, lw_tx1 = 0, lw_ty0 = 0, lw_ty1 = 0;
    bool lw_valid = false, lw_cache = false, lw_flags_on_host = false;

    // The device buffers by lifetime (the caches' aside); forma_hip_destroy releases all four.  The scene: frame slots borrow it
    std::vector<DevBuf*> scene_bufs() { return {&x, &y, &line_slot, &geoms, &style_off, &style_words, &unchanged, &images, &texels, &layer_sf, &layer_col}; }
    // per-frame scratch that a frame writes before it reads: poison_frame_buffers refills it, forma_hip_trim releases it
    std::vector<DevBuf*> frame_bufs() { return {&scan_tmp, &cl_idx, &cl_start, &block_first, &prep_scratch, &seg_u, &seg_a, &seg_b, &sort_counters,
        &records, &rk_u, &rk_a, &rk_b, &blk_edge, &runs_scratch, &row_tab, &span_key, &span_cov, &ras_masks, &huge_offs, &huge_key, &huge_tmp,
        &huge_flag, &grp_tab, &grp_list, &run_lt, &rec_sp, &run_lt_sp, &row_sp, &pack_list, &pack_pix, &slice_buf}; }
    // released by trim, not refilled: parity line parameters, the scratch image (a cropped frame leaves the rest alone), exchange scratch, order lists
    std::vector<DevBuf*> trimmed_bufs() { return {&l_order, &l_x0, &l_y0, &l_dx, &l_dy, &l_a, &l_b, &l_c, &l_d, &l_len, &image, &xscratch, &xmask, &order_buf,
        &x_spare, &y_spare, &line_slot_spare, &geo_blob, &geo_flag, &stroke_tmp}; }
    // kept by trim, like the scene: FrameInfo and its template, cache frames' written-tile flags, the exchange's buckets
    std::vector<DevBuf*> kept_bufs() { return {&info, &info_init, &cache_written, &xsend, &xrecv}; }
    std::vector<PinnedBuf*> pinned_bufs() { return {&h_written, &h_stage, &h_geo, &h_tab_stage}; }   // the growing page-locked ones
};

// the owner of the frame slots and every slot of it, the owner first (one frame in flight: the owner alone)
inline std::vector<forma_hip_ctx*> frame_slots(forma_hip_ctx* o) { return o->slots.empty() ? std::vector<forma_hip_ctx*>{o} : o->slots; }
inline uint32_t paint_strip_tiles(const forma_hip_ctx* c) { return c->n_cus * PAINT_WAVES_PER_CU; }

#define FORMA_RETRY 1     /* internal: a speculation of the read-back-free path was wrong, run the frame again synchronously */

// ---- internals shared by api.cpp and multi.cpp -------------------------------------------------------------------------
int fd_fail(forma_hip_ctx* c, int code, const char* what, hipError_t e = hipSuccess);
// every frame the context still owes (frames in flight) is finished; the first error of a deferred frame is returned
int fd_drain(forma_hip_ctx* ctx);
// restrict the context to lines [lo, hi) of the uploaded geometry (ranged == false: all of them)
int fd_set_line_range(forma_hip_ctx* ctx, bool ranged, size_t lo, size_t hi);
// inclusive prefix sums of the pixel-segment counts of ALL uploaded lines at this canvas size (the reference's `lengths`
// after prefix_sum, segment.rs:90-98,400) — what the line shares of a multi-device plan are cut from
int fd_line_sums(forma_hip_ctx* ctx, uint32_t width, uint32_t height, std::vector<uint32_t>& sums);
// stages 1-2 on the context's line range (synchronous), then pixel segments per tile row -> hist[0 .. 2048)
int fd_row_histogram(forma_hip_ctx* ctx, uint32_t width, uint32_t height, uint32_t* hist /* 2048 */, uint32_t* n_segments);
// forma_hip_gather_sort_paint_frame with a buffer-layer cache
int fd_gather_sort_paint(forma_hip_ctx* ctx, uint8_t* dst, uint32_t width, uint32_t height, size_t stride_bytes,
                         const uint8_t channels[4], const float clear_color[4], const forma_rect_t* crop_or_null, int cache_id,
                         forma_timings_t* timings);
// the same frame for a multi-device context with frames in flight (device-resident, no cache): enqueue now, settle later
int fd_gsp_defer(forma_hip_ctx* ctx, uint32_t width, uint32_t height, const uint8_t channels[4], const float clear_color[4],
                 const forma_rect_t* crop_or_null);
int fd_gsp_settle(forma_hip_ctx* ctx);
// rows [y0, y1) of the context's last image -> dst (row-major, stride bytes per row, dst addresses row 0)
int fd_copy_image_rows(forma_hip_ctx* ctx, uint8_t* dst, size_t stride_bytes, uint32_t y0, uint32_t y1);
// layer-table edits on one device of a multi-device context: the edit, then EVERY frame slot's table brought up to date and
// waited for (the caller has settled the frames)
int fd_update_geoms_now(forma_hip_ctx* ctx, const uint32_t* slots, const forma_geom_t* entries, size_t n);
int fd_update_geoms_xf_now(forma_hip_ctx* ctx, uint32_t first, uint32_t count, const float* xf);
// the frame slot that holds the context's most recent frame (the context itself without frame slots)
forma_hip_ctx* fd_last_slot(forma_hip_ctx* ctx);

// the stream (0 unsorted, 1 sorted) / the written-tile flags of exactly this context's last frame
int fd_read_stream(forma_hip_ctx* ctx, int which, uint64_t* out, size_t capacity, size_t* out_n);
int fd_read_sorted(forma_hip_ctx* ctx, uint64_t* out, size_t capacity, size_t* out_n);
int fd_tiles_written(forma_hip_ctx* ctx, uint8_t* flags, size_t n_tiles);

// multi.cpp: the entry points of a multi-device context (ctx->multi != nullptr)
int  multi_set_frames_in_flight(forma_hip_ctx* ctx, int n);
int  multi_set_layout(forma_hip_ctx* ctx, int layout);
int  multi_sync(forma_hip_ctx* ctx);
void multi_info(forma_hip_ctx* ctx, forma_context_info_t* out);
int  multi_create(forma_hip_ctx** out, const int* devices, int n);
void multi_destroy(forma_hip_ctx* ctx);
int  multi_set_geometry(forma_hip_ctx* ctx, const float* x, const float* y, const uint32_t* line_slot, size_t n_points);
int  multi_set_geoms(forma_hip_ctx* ctx, const forma_geom_t* geoms, size_t n_geoms);
int  multi_update_geoms(forma_hip_ctx* ctx, const uint32_t* slots, const forma_geom_t* entries, size_t n);
int  multi_update_geoms_xf(forma_hip_ctx* ctx, uint32_t first, uint32_t count, const float* xf);
int  multi_geometry_append(forma_hip_ctx* ctx, const forma_flatten_tables_t* t, const uint32_t* line_slot,
                           const forma_affine_range_t* affines, size_t n_affines);
int  multi_geometry_append_stroked(forma_hip_ctx* ctx, const forma_flatten_tables_t* t, const uint32_t* line_slot,
                                   const forma_affine_range_t* affines, size_t n_affines,
                                   const forma_stroke_range_t* strokes, size_t n_strokes, size_t* out_points_added);
int  multi_geometry_retain(forma_hip_ctx* ctx, const forma_keep_range_t* keep, size_t n_keep, const uint32_t* slot_remap, size_t n_slots);
int  multi_counters(forma_hip_ctx* ctx, forma_counters_t* out);
int  multi_set_styles(forma_hip_ctx* ctx, const uint32_t* style_offsets, size_t n_orders, const uint32_t* style_words,
                      size_t n_words, const uint8_t* unchanged);
int  multi_set_images(forma_hip_ctx* ctx, const forma_image_t* images, size_t n_images, const uint16_t* texels, size_t n_texels);
int  multi_render(forma_hip_ctx* ctx, uint8_t* dst, uint32_t width, uint32_t height, size_t stride_bytes,
                  const uint8_t channels[4], const float clear_color[4], const forma_rect_t* crop_or_null, int cache_id,
                  forma_timings_t* timings);
int  multi_cache_clear(forma_hip_ctx* ctx, int cache_id);
int  multi_trim(forma_hip_ctx* ctx);
int  multi_read_segments(forma_hip_ctx* ctx, int which, uint64_t* out, size_t capacity, size_t* out_n);
int  multi_read_image(forma_hip_ctx* ctx, uint8_t* dst, size_t stride_bytes);
int  multi_tiles_written(forma_hip_ctx* ctx, uint8_t* flags, size_t n_tiles);
forma_hip_ctx* multi_first(forma_hip_ctx* ctx);      // the device-0 context (stage entry points run there)
