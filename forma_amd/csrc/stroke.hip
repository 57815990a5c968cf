// stroke.hip — stroke expansion for gfx950: the flattened points of one append in, closed polygonal pieces out.
//
// One thread per SOURCE point.  A point outside every stroked contour is copied.  A point i of a stroked contour emits, in this
// order: the join at i (or the start cap of an open contour), then the body of the line i -> i + 1; the last point of an open
// contour emits the end cap.  Every piece of k lines is k + 1 points: the last repeats the first and carries FORMA_NONE, the
// others carry the slot of the source line (a join: the line that leaves the vertex; a cap: its end's line).
//
//   k_stroke_count   what each source point will write, and the sum per workgroup
//   k_stroke_scan    exclusive scan of the workgroups' sums (one workgroup), and the total the host sizes the store with
//   k_stroke_emit    the same walk again, writing x, y and slot at store + base + offset
//
// Count and emit run ONE function (stroke_point<EMIT>), so they cannot disagree; every store is bounds-checked against the end
// of the store all the same.  f32, no contraction, true division and sqrtf (the build asks for correctly rounded ones), plain
// vector stores, LDS for the scans only.
//
// All pieces are wound alike (the body p0+o, p1+o, p1-o, p0-o with o the left normal times the half width; joins and caps turn
// the same way), so overlapping pieces add under NonZero and never cancel.
#include "stroke.h"

namespace {

struct Sink {
    float* x; float* y; uint32_t* slot;
    uint32_t at, limit;
};
template <bool EMIT> __device__ __forceinline__ void put(Sink& k, float px, float py, uint32_t s) {
    if (EMIT) {
        if (k.at < k.limit) { k.x[k.at] = px; k.y[k.at] = py; k.slot[k.at] = s; }
    }
    k.at++;
}

struct Line { float dx, dy, ox, oy, ex, ey; };     // d = p1 - p0; o = left normal * half width; e = direction * half width
__device__ __forceinline__ Line line_of(const StrokeArgs& A, uint32_t j, float hw) {
    Line l;
    l.dx = A.sx[j + 1] - A.sx[j]; l.dy = A.sy[j + 1] - A.sy[j];
    const float len = sqrtf(l.dx * l.dx + l.dy * l.dy);
    const float s = hw / len;
    l.ox = -l.dy * s; l.oy = l.dx * s;
    l.ex = l.dx * s;  l.ey = l.dy * s;
    return l;
}
__device__ __forceinline__ bool nonzero(const StrokeArgs& A, uint32_t j) {
    return A.sx[j] != A.sx[j + 1] || A.sy[j] != A.sy[j + 1];
}

// equal angular steps of a fan over the angle phi: the fewest whose chord's sagitta is <= 1/16 px (the flattener's kMaxError).
// hw * (1 - cos(step / 2)) <= 1/16  <=>  step <= 4 * asin(sqrt(1 / (32 * hw))): the form without cancellation.
__device__ __forceinline__ uint32_t fan_steps(float phi, float hw) {
    float q = 1.0f / (32.0f * hw);
    if (!(q < 1.0f)) q = 1.0f;
    const float step = 4.0f * asinf(sqrtf(q));
    const float r = ceilf(phi / step);
    if (!(r >= 1.0f)) return 1u;
    if (r > 4096.0f) return 4096u;
    return (uint32_t)r;
}

// the fan v, v + us, (n - 1 points between, us turned clockwise by k * phi / n), v + ue, v: n + 2 lines, n + 3 points
template <bool EMIT>
__device__ __forceinline__ void fan(Sink& k, float vx, float vy, float usx, float usy, float uex, float uey, float phi, uint32_t n, uint32_t s) {
    put<EMIT>(k, vx, vy, s);
    put<EMIT>(k, vx + usx, vy + usy, s);
    for (uint32_t j = 1; j < n; j++) {
        float sn = 0.0f, cs = 1.0f;
        if (EMIT) sincosf((float)j * phi / (float)n, &sn, &cs);
        put<EMIT>(k, vx + (usx * cs + usy * sn), vy + (usy * cs - usx * sn), s);
    }
    put<EMIT>(k, vx + uex, vy + uey, s);
    put<EMIT>(k, vx, vy, FORMA_NONE);
}

// everything source point i writes; returns the number of points
template <bool EMIT> __device__ uint32_t stroke_point(const StrokeArgs& A, uint32_t i, uint32_t at) {
    Sink k{A.x, A.y, A.slot, at, A.limit};
    uint32_t lo = 0, hi = A.n_contours;                            // contours[lo - 1].first <= i < contours[lo].first
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (A.contours[3 * mid] <= i) lo = mid + 1; else hi = mid;
    }
    if (lo == 0 || A.contours[3 * (lo - 1) + 1] < i) {             // not stroked: the point as it is
        put<EMIT>(k, A.sx[i], A.sy[i], A.sslot[i]);
        return k.at - at;
    }
    const uint32_t first = A.contours[3 * (lo - 1)], last = A.contours[3 * (lo - 1) + 1];
    const uint32_t* st = A.styles + 4 * A.contours[3 * (lo - 1) + 2];
    const float hw = __uint_as_float(st[0]), limit = __uint_as_float(st[1]);
    const uint32_t join = st[2], cap = st[3];
    const bool closed = last > first && __float_as_uint(A.sx[first]) == __float_as_uint(A.sx[last]) &&
                        __float_as_uint(A.sy[first]) == __float_as_uint(A.sy[last]);
    const float PI = 3.14159265358979323846f;

    if (i == last) {                                               // the end cap of an open contour
        if (closed || cap == FORMA_CAP_BUTT) return 0;
        uint32_t p = last;
        while (p > first && !nonzero(A, p - 1)) p--;
        if (p == first) return 0;                                  // no line of non-zero length
        p--;
        const Line l = line_of(A, p, hw);
        const float vx = A.sx[p + 1], vy = A.sy[p + 1];
        const uint32_t s = A.sslot[p];
        if (cap == FORMA_CAP_SQUARE) {
            put<EMIT>(k, vx + l.ox, vy + l.oy, s);
            put<EMIT>(k, (vx + l.ex) + l.ox, (vy + l.ey) + l.oy, s);
            put<EMIT>(k, (vx + l.ex) - l.ox, (vy + l.ey) - l.oy, s);
            put<EMIT>(k, vx - l.ox, vy - l.oy, s);
            put<EMIT>(k, vx + l.ox, vy + l.oy, FORMA_NONE);
        } else {
            fan<EMIT>(k, vx, vy, l.ox, l.oy, -l.ox, -l.oy, PI, fan_steps(PI, hw), s);
        }
        return k.at - at;
    }
    if (!nonzero(A, i)) return 0;                                  // zero-length lines emit nothing; joins look through them

    const Line b = line_of(A, i, hw);
    const float vx = A.sx[i], vy = A.sy[i];
    const uint32_t s = A.sslot[i];
    // the nearest line of non-zero length in front of i: back to the contour's first point, then — closed — round from its end
    uint32_t p = FORMA_NONE;
    for (uint32_t j = i; j > first; j--)
        if (nonzero(A, j - 1)) { p = j - 1; break; }
    if (p == FORMA_NONE && closed)
        for (uint32_t j = last; j > i + 1; j--)
            if (nonzero(A, j - 1)) { p = j - 1; break; }

    if (p == FORMA_NONE) {                                         // the start cap of an open contour
        if (!closed && cap == FORMA_CAP_SQUARE) {
            put<EMIT>(k, (vx - b.ex) + b.ox, (vy - b.ey) + b.oy, s);
            put<EMIT>(k, vx + b.ox, vy + b.oy, s);
            put<EMIT>(k, vx - b.ox, vy - b.oy, s);
            put<EMIT>(k, (vx - b.ex) - b.ox, (vy - b.ey) - b.oy, s);
            put<EMIT>(k, (vx - b.ex) + b.ox, (vy - b.ey) + b.oy, FORMA_NONE);
        } else if (!closed && cap == FORMA_CAP_ROUND) {
            fan<EMIT>(k, vx, vy, -b.ox, -b.oy, b.ox, b.oy, PI, fan_steps(PI, hw), s);
        }
    } else {                                                       // the join, on the outer side of the turn
        const Line a = line_of(A, p, hw);
        const float cross = a.dx * b.dy - a.dy * b.dx, dot = a.dx * b.dx + a.dy * b.dy;
        if (!(cross == 0.0f && dot >= 0.0f)) {                     // (collinear and the same way: nothing)
            // a left turn's outer side is the right one; a right turn and the exact U-turn take the left side
            const bool left = cross > 0.0f;
            const float usx = left ? -b.ox : a.ox, usy = left ? -b.oy : a.oy;
            const float uex = left ? -a.ox : b.ox, uey = left ? -a.oy : b.oy;
            bool done = false;
            if (join == FORMA_JOIN_ROUND) {
                const float phi = atan2f(fabsf(cross), dot);
                fan<EMIT>(k, vx, vy, usx, usy, uex, uey, phi, fan_steps(phi, hw), s);
                done = true;
            } else if (join == FORMA_JOIN_MITER) {
                // tip = v + (us + ue) * hw^2 / (hw^2 + oa . ob); 1 / cos^2(theta / 2) = 2 hw^2 / (hw^2 + oa . ob)
                const float hw2 = hw * hw, den = hw2 + (a.ox * b.ox + a.oy * b.oy);
                const float m = hw2 / den;
                if (den > 0.0f && 2.0f * m <= limit * limit) {
                    put<EMIT>(k, vx, vy, s);
                    put<EMIT>(k, vx + usx, vy + usy, s);
                    put<EMIT>(k, vx + (usx + uex) * m, vy + (usy + uey) * m, s);
                    put<EMIT>(k, vx + uex, vy + uey, s);
                    put<EMIT>(k, vx, vy, FORMA_NONE);
                    done = true;
                }
            }
            if (!done) {                                           // bevel
                put<EMIT>(k, vx, vy, s);
                put<EMIT>(k, vx + usx, vy + usy, s);
                put<EMIT>(k, vx + uex, vy + uey, s);
                put<EMIT>(k, vx, vy, FORMA_NONE);
            }
        }
    }
    // the body of line i
    const float wx = A.sx[i + 1], wy = A.sy[i + 1];
    put<EMIT>(k, vx + b.ox, vy + b.oy, s);
    put<EMIT>(k, wx + b.ox, wy + b.oy, s);
    put<EMIT>(k, wx - b.ox, wy - b.oy, s);
    put<EMIT>(k, vx - b.ox, vy - b.oy, s);
    put<EMIT>(k, vx + b.ox, vy + b.oy, FORMA_NONE);
    return k.at - at;
}

// inclusive scan of one value per thread over a workgroup of N threads; every thread of the workgroup calls it
template <uint32_t N> __device__ __forceinline__ uint32_t block_scan(uint32_t v, uint32_t* sh) {
    const uint32_t t = threadIdx.x;
    sh[t] = v;
    __syncthreads();
    for (uint32_t d = 1; d < N; d <<= 1) {
        const uint32_t add = t >= d ? sh[t - d] : 0u;
        __syncthreads();
        sh[t] += add;
        __syncthreads();
    }
    return sh[t];
}

}  // namespace

__global__ __launch_bounds__(SK_THREADS) void k_stroke_count(StrokeArgs A) {
    __shared__ uint32_t sh[SK_THREADS];
    const uint32_t i = blockIdx.x * SK_THREADS + threadIdx.x;
    const uint32_t c = i < A.n_src ? stroke_point<false>(A, i, 0u) : 0u;
    if (i < A.n_src) A.counts[i] = c;
    const uint32_t incl = block_scan<SK_THREADS>(c, sh);
    if (threadIdx.x == SK_THREADS - 1) A.block_base[blockIdx.x] = incl;
}

constexpr uint32_t SK_SCAN_THREADS = 1024;
__global__ __launch_bounds__(SK_SCAN_THREADS) void k_stroke_scan(uint32_t* __restrict__ block_base, uint32_t n_blocks,
                                                                 unsigned long long* __restrict__ total) {
    __shared__ uint32_t sh[SK_SCAN_THREADS];
    unsigned long long carry = 0;                                  // (the same in every thread)
    for (uint32_t c0 = 0; c0 < n_blocks; c0 += SK_SCAN_THREADS) {
        const uint32_t j = c0 + threadIdx.x;
        const uint32_t v = j < n_blocks ? block_base[j] : 0u;
        const uint32_t incl = block_scan<SK_SCAN_THREADS>(v, sh);
        if (j < n_blocks) block_base[j] = (uint32_t)(carry + (incl - v));   // (exact while the total stays below 2^32: the host checks 2^30)
        carry += sh[SK_SCAN_THREADS - 1];
        __syncthreads();
    }
    if (threadIdx.x == 0) *total = carry;
}

__global__ __launch_bounds__(SK_THREADS) void k_stroke_emit(StrokeArgs A) {
    __shared__ uint32_t sh[SK_THREADS];
    const uint32_t i = blockIdx.x * SK_THREADS + threadIdx.x;
    const uint32_t c = i < A.n_src ? A.counts[i] : 0u;
    const uint32_t incl = block_scan<SK_THREADS>(c, sh);
    if (i < A.n_src && c) stroke_point<true>(A, i, A.base + A.block_base[blockIdx.x] + (incl - c));
}

void launch_stroke_count(hipStream_t s, const StrokeArgs& A) {
    if (A.n_src == 0) return;
    const uint32_t blocks = stroke_blocks(A.n_src);
    hipLaunchKernelGGL(k_stroke_count, dim3(blocks), dim3(SK_THREADS), 0, s, A);
    hipLaunchKernelGGL(k_stroke_scan, dim3(1), dim3(SK_SCAN_THREADS), 0, s, A.block_base, blocks, A.total);
}

void launch_stroke_emit(hipStream_t s, const StrokeArgs& A) {
    if (A.n_src == 0) return;
    hipLaunchKernelGGL(k_stroke_emit, dim3(stroke_blocks(A.n_src)), dim3(SK_THREADS), 0, s, A);
}
