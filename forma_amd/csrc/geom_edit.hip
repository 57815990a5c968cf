// geom_edit.hip — k_geom_edit: apply one block of layer-table edit records to a frame slot's table (gfx950).
// The block arrives on the slot's stream right in front of the frame that is to see it (api.cpp tables_catch_up), so stream
// order is the only ordering there is.  Plain C++ and 16-byte vector loads / stores; no LDS, no atomics.
#include "geom_edit.h"

// one thread per ENTRY record: the 32-byte entry as two 16-byte stores;
// RANGE records grid-strided over their slots: flags bit 0 and xf, `order` untouched
__global__ __launch_bounds__(GE_THREADS) void k_geom_edit(const uint4* __restrict__ recs, uint32_t n_range, uint32_t n_entry,
                                                          uint4* __restrict__ table, uint32_t n_geoms) {
    const uint32_t tid = blockIdx.x * GE_THREADS + threadIdx.x, total = gridDim.x * GE_THREADS;
    if (tid < n_entry) {
        const uint4* r = recs + (size_t)(n_range + tid) * 3;
        const uint4 head = r[0], lo = r[1], hi = r[2];
        if (head.y < n_geoms) { table[(size_t)head.y * 2] = lo; table[(size_t)head.y * 2 + 1] = hi; }
    }
    for (uint32_t k = 0; k < n_range; k++) {
        const uint4* r = recs + (size_t)k * 3;
        const uint4 head = r[0], lo = r[1], hi = r[2];        // lo = {order, flags, xf0, xf1}, hi = {xf2 .. xf5}
        const uint32_t first = head.y, count = head.z;
        for (uint32_t i = tid; i < count; i += total) {
            const uint32_t slot = first + i;
            if (slot < first || slot >= n_geoms) break;
            uint4 cur = table[(size_t)slot * 2];
            cur.y = (cur.y & ~FORMA_GEOM_HAS_XF) | (lo.y & FORMA_GEOM_HAS_XF);
            cur.z = lo.z; cur.w = lo.w;
            table[(size_t)slot * 2] = cur;
            table[(size_t)slot * 2 + 1] = hi;
        }
    }
}

void launch_geom_edit(hipStream_t s, const GeomEditRec* recs, uint32_t n_range, uint32_t n_entry, uint32_t max_range_count,
                      forma_geom_t* table, uint32_t n_geoms) {
    if (!n_range && !n_entry) return;
    const uint32_t want = n_entry > max_range_count ? n_entry : max_range_count;
    uint32_t blocks = (want + GE_THREADS - 1) / GE_THREADS;
    if (blocks < 1) blocks = 1;
    // (entries need a thread each; ranges stride, so only they may be capped)
    const uint32_t need_entry = (n_entry + GE_THREADS - 1) / GE_THREADS;
    if (blocks > GE_MAX_BLOCKS) blocks = need_entry > GE_MAX_BLOCKS ? need_entry : GE_MAX_BLOCKS;
    hipLaunchKernelGGL(k_geom_edit, dim3(blocks), dim3(GE_THREADS), 0, s, reinterpret_cast<const uint4*>(recs), n_range, n_entry,
                       reinterpret_cast<uint4*>(table), n_geoms);
}
