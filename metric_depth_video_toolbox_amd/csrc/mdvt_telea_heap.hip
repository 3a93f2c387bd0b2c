// mdvt_telea_heap.hip -- the infill-mask completion in cv2.inpaint's own order (mdvt_finish_infill_mask_heap, opt-in).
//
// cv2.inpaint(INPAINT_TELEA) pops one pixel at a time from a heap ordered by arrival time T (ties: first in, first out) and
// estimates the unknown 4-neighbours of each pop, in OpenCV's neighbour order (up, left, down, right), from everything that is
// not INSIDE at that moment (orc_telea_fmm).  The level path (k_telea_fill) keeps the per-pixel arithmetic but not that order.
// This file reproduces the order exactly, with the decomposition of orc_telea_windows (held equal to orc_telea_fmm by
// tests/test_oracle_golden.py):
//
//   A pixel activated by a pop of the window [0.7 k, 0.7 (k + 1)) has T >= T(pop) + 1/sqrt(2), so it is popped in a later window.
//   Per window:
//     1. the pops = the band pixels with T below the window's end, sorted by (T, push number);
//     2. every INSIDE 4-neighbour of a pop is activated with the key A = 4 rank(parent) + direction, parent = its adjacent pop of
//        least rank: an atomic minimum, order-free; the activated pixels, listed in A order, get the next push numbers;
//     3. T and colour of the activated pixels, each reading what was activated before it: a pixel depends on the pixels of the
//        same window with a smaller A within its read set (kNeedOffsets: the radius-3 disc and the 4-neighbours its gradients
//        read).  That graph is walked by readiness: a pixel is estimated in the round after its last predecessor.
//
// One workgroup owns one image for the whole march: nothing passes between workgroups, every step is a barrier-synchronised
// round inside the workgroup, and every loop has a bound derived from the pixel count -- if one trips, the image's remaining
// entry becomes 0xFFFFFFFF and the workgroup returns.  An image stops as soon as all its key-coloured pixels have their
// estimates (later pops cannot change an earlier estimate); key-coloured pixels that are never reached keep the seed's value,
// as in telea_fmm, and are counted in remaining.
//
// Memory: words written by atomics (the activation keys and the predecessor counts) are read back with L2 loads; every other
// plane is written and read by the waves of this workgroup only, on one CU, with a barrier in between.
#include "mdvt_internal.h"
#include "mdvt_telea_common.h"

namespace mdvt {

constexpr int kHeapThreads = 512;
constexpr int kHeapHalfWaves = kHeapThreads / 32;
constexpr uint32_t kHeapLdsKeys = 16384;       // windows of up to this many pops are sorted in LDS (128 KiB), larger ones in place
constexpr uint8_t kHeapInside = 1, kHeapKeyPx = 2;
constexpr uint32_t kHeapNoKey = 0xFFFFFFFFu;
constexpr double kHeapWindow = 0.70;           // < 1/sqrt(2): the look-ahead of orc_telea_windows

// The planes of one image, in one block of telea_heap_image_bytes(W, H): pops' sort keys (later the ready lists), T, activation
// keys, predecessor counts, push numbers, push number -> pixel, two band lists, the activated pixels of a window, the work
// image (u8 RGB, + 4 bytes: pixels are fetched as unaligned dwords) and the flags (INSIDE, key-coloured).  44 B per pixel.
struct HeapPlanes {
    uint64_t* keys; float* T; uint32_t *akey, *cnt, *seq, *seq2idx, *band0, *band1, *acts; uint8_t *img, *flags;
};

__host__ __device__ inline size_t heap_plane(size_t bytes) { return (bytes + 255) & ~(size_t)255; }

__host__ __device__ inline size_t heap_img_offset(size_t npx) { return heap_plane(8 * npx) + 8 * heap_plane(4 * npx); }

__device__ inline HeapPlanes heap_planes(uint8_t* base, size_t npx)
{
    HeapPlanes p;
    p.keys = reinterpret_cast<uint64_t*>(base);
    uint8_t* q = base + heap_plane(8 * npx);
    uint32_t** u32[] = {&p.akey, &p.cnt, &p.seq, &p.seq2idx, &p.band0, &p.band1, &p.acts};
    p.T = reinterpret_cast<float*>(q); q += heap_plane(4 * npx);
    for (uint32_t** w : u32) { *w = reinterpret_cast<uint32_t*>(q); q += heap_plane(4 * npx); }
    p.img = q; q += heap_plane(3 * npx + 4);
    p.flags = q;
    return p;
}

size_t telea_heap_image_bytes(int W, int H)
{
    const size_t npx = (size_t)W * H;
    return heap_img_offset(npx) + heap_plane(3 * npx + 4) + heap_plane(npx);
}

size_t telea_heap_img_offset(int W, int H) { return heap_img_offset((size_t)W * H); }

// a word last written by an atomic: read at L2
__device__ __forceinline__ uint32_t ld_l2(const uint32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// Exclusive prefix sum of one value per thread over the workgroup; *total = the sum.  Every thread calls it.
__device__ uint32_t heap_scan(uint32_t v, uint32_t* s_wave, uint32_t* total)
{
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    uint32_t x = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t y = __shfl_up(x, o, 64);
        if (lane >= o) x += y;
    }
    if (lane == 63) s_wave[wv] = x;
    __syncthreads();
    uint32_t before = 0, sum = 0;
#pragma unroll
    for (int w = 0; w < kHeapThreads / 64; ++w) {
        const uint32_t s = s_wave[w];
        if (w < wv) before += s;
        sum += s;
    }
    __syncthreads();                                      // (s_wave is reused by the next call)
    *total = sum;
    return before + x - v;
}

// Ascending sort of p[0 .. n): a bitonic network over the next power of two in which every comparator puts the smaller key at
// the lower index (the first step of each merge compares i with i ^ (k - 1)), so the positions >= n act as +infinity and are
// never touched.  Every thread calls it; n is the same in all of them.
template <typename K>
__device__ void heap_sort_keys(K* p, uint32_t n)
{
    uint32_t P = 1;
    while (P < n) P <<= 1;
    for (uint32_t k = 2; k <= P; k <<= 1)
        for (uint32_t j = k >> 1; j > 0; j >>= 1) {
            for (uint32_t c = threadIdx.x; c < P / 2; c += kHeapThreads) {
                const uint32_t i = ((c & ~(j - 1)) << 1) | (c & (j - 1));
                const uint32_t l = j == (k >> 1) ? (i ^ (k - 1)) : (i + j);
                if (l >= n) continue;
                const K u = p[i], v = p[l];
                if (v < u) { p[i] = v; p[l] = u; }
            }
            __syncthreads();
        }
}

struct HeapArgs { uint8_t* ws; size_t image_bytes; uint32_t* remaining; int W, H; uint32_t key_rgb; };

__global__ void __launch_bounds__(kHeapThreads) k_telea_heap(ImageSet seed, HeapArgs a)
{
    // LDS: the sort keys of a window, or -- at another time -- the estimate's per-half-wave neighbourhoods and running sums
    constexpr int kRedBytes = kHeapHalfWaves * 10 * kRedStride * 4, kColBytes = kHeapHalfWaves * 81 * 4;
    static_assert(kRedBytes + 2 * kColBytes + kHeapHalfWaves * 84 <= (int)kHeapLdsKeys * 8, "the estimate's tiles fit the sort area");
    __shared__ __attribute__((aligned(16))) uint8_t s_raw[kHeapLdsKeys * 8];
    __shared__ uint32_t s_wave[kHeapThreads / 64];
    // (every counter has a barrier between its last read and its next reset; the initial band has a counter of its own, read by
    //  every thread right before the first window's resets)
    __shared__ uint32_t s_nb0, s_np, s_nk, s_nr, s_next[2], s_tmin, s_keys_left, s_fail;
    const int W = a.W, H = a.H, im = blockIdx.x, tid = threadIdx.x;
    const uint32_t npx = (uint32_t)W * (uint32_t)H;
    const HeapPlanes P = heap_planes(a.ws + (size_t)im * a.image_bytes, npx);
    const int dx4[4] = {0, -1, 0, 1}, dy4[4] = {-1, 0, 1, 0};        // OpenCV's neighbour order: up, left, down, right

    // the seed -> flags, work image, T = 0, no activation key; the key-coloured pixels are counted
    if (tid == 0) { s_keys_left = 0u; s_fail = 0u; s_nb0 = 0u; }
    __syncthreads();
    {
        const uint8_t* sbase = seed.image(im);
        uint32_t nkey = 0;
        for (uint32_t k = tid; k < npx; k += kHeapThreads) {
            const uint32_t y = k / (uint32_t)W, x = k - y * (uint32_t)W;
            const uint32_t px = load_px_bytes(sbase + (size_t)y * seed.pitch, (int)x);
            const bool key = px == a.key_rgb;
            P.flags[k] = (key || px == 0u) ? (uint8_t)(kHeapInside | (key ? kHeapKeyPx : 0)) : (uint8_t)0;   // sr:803-805
            store_px_bytes(P.img, (int)k, px);
            P.T[k] = 0.0f;
            P.akey[k] = kHeapNoKey;
            nkey += key ? 1u : 0u;
        }
        if (nkey) atomicAdd(&s_keys_left, nkey);
    }
    __syncthreads();
    // the initial band: known pixels next to the mask, T = 0, pushed in raster order (push number = pixel index)
    for (uint32_t k = tid; k < npx; k += kHeapThreads) {
        if (P.flags[k] & kHeapInside) continue;
        const int y = (int)(k / (uint32_t)W), x = (int)(k - (uint32_t)y * (uint32_t)W);
        bool band = false;
        for (int d = 0; d < 4; ++d) {
            const int xx = x + dx4[d], yy = y + dy4[d];
            if (xx >= 0 && xx < W && yy >= 0 && yy < H && (P.flags[(uint32_t)yy * W + xx] & kHeapInside)) band = true;
        }
        if (band) { P.band0[atomicAdd(&s_nb0, 1u)] = k; P.seq[k] = k; }
    }
    __syncthreads();

    uint32_t nb = s_nb0, seq_next = 0;
    uint32_t* band = P.band0;
    uint32_t* band_next = P.band1;
    uint32_t* ready[2] = {reinterpret_cast<uint32_t*>(P.keys), reinterpret_cast<uint32_t*>(P.keys) + npx};
    bool failed = false;
    // (the values that steer the loops are read from LDS after a barrier: the same in every thread)
    for (uint32_t win = 0; nb != 0u && s_keys_left != 0u; ++win) {
        if (win > npx || s_fail) { failed = true; break; }                // (every window pops at least one pixel)
        // 1. the window's end: from the least T in the band (T >= 0: its bits order like the values)
        if (tid == 0) { s_tmin = 0x7F800000u; s_np = 0u; s_nk = 0u; s_next[0] = 0u; s_next[1] = 0u; s_nr = 0u; }
        __syncthreads();
        uint32_t mn = 0x7F800000u;
        for (uint32_t q = tid; q < nb; q += kHeapThreads) mn = min(mn, __float_as_uint(P.T[band[q]]));
        atomicMin(&s_tmin, mn);
        __syncthreads();
        const double hi = (floor((double)__uint_as_float(s_tmin) / kHeapWindow) + 1.0) * kHeapWindow;
        // the pops (sort key: T bits, push number) and the rest of the band
        for (uint32_t q = tid; q < nb; q += kHeapThreads) {
            const uint32_t k = band[q];
            const float t = P.T[k];
            if ((double)t < hi) P.keys[atomicAdd(&s_np, 1u)] = ((uint64_t)__float_as_uint(t) << 32) | P.seq[k];
            else band_next[atomicAdd(&s_nk, 1u)] = k;
        }
        __syncthreads();
        const uint32_t np = s_np, nk = s_nk;
        // sorted: then keys[r] = the pixel of rank r
        if (np <= kHeapLdsKeys) {
            uint64_t* sk = reinterpret_cast<uint64_t*>(s_raw);
            for (uint32_t r = tid; r < np; r += kHeapThreads) sk[r] = P.keys[r];
            __syncthreads();
            heap_sort_keys(sk, np);
            for (uint32_t r = tid; r < np; r += kHeapThreads) {
                const uint32_t s = (uint32_t)sk[r];
                P.keys[r] = s < npx ? s : P.seq2idx[s - npx];
            }
        } else {
            heap_sort_keys(P.keys, np);
            for (uint32_t r = tid; r < np; r += kHeapThreads) {
                const uint32_t s = (uint32_t)P.keys[r];
                P.keys[r] = s < npx ? s : P.seq2idx[s - npx];
            }
        }
        __syncthreads();
        // 2. activation: per INSIDE neighbour the least 4 rank + direction
        for (uint32_t r = tid; r < np; r += kHeapThreads) {
            const uint32_t k = (uint32_t)P.keys[r];
            const int y = (int)(k / (uint32_t)W), x = (int)(k - (uint32_t)y * (uint32_t)W);
            for (int d = 0; d < 4; ++d) {
                const int xx = x + dx4[d], yy = y + dy4[d];
                if (xx < 0 || xx >= W || yy < 0 || yy >= H) continue;
                const uint32_t q = (uint32_t)yy * W + xx;
                if (P.flags[q] & kHeapInside) atomicMin(&P.akey[q], 4u * r + (uint32_t)d);
            }
        }
        __syncthreads();
        // the activated pixels in A order (a pop's winning directions, then a prefix sum over the ranks) get the next push numbers
        uint32_t na = 0;
        for (uint32_t r0 = 0; r0 < np; r0 += kHeapThreads) {
            const uint32_t r = r0 + tid;
            uint32_t won = 0, k = 0;
            if (r < np) {
                k = (uint32_t)P.keys[r];
                const int y = (int)(k / (uint32_t)W), x = (int)(k - (uint32_t)y * (uint32_t)W);
                for (int d = 0; d < 4; ++d) {
                    const int xx = x + dx4[d], yy = y + dy4[d];
                    if (xx < 0 || xx >= W || yy < 0 || yy >= H) continue;
                    const uint32_t q = (uint32_t)yy * W + xx;
                    if ((P.flags[q] & kHeapInside) && ld_l2(&P.akey[q]) == 4u * r + (uint32_t)d) won |= 1u << d;
                }
            }
            uint32_t total;
            uint32_t pos = na + heap_scan((uint32_t)__popc(won), s_wave, &total);
            if (won) {
                const int y = (int)(k / (uint32_t)W), x = (int)(k - (uint32_t)y * (uint32_t)W);
                for (int d = 0; d < 4; ++d) {
                    if (!((won >> d) & 1u)) continue;
                    const uint32_t q = (uint32_t)(y + dy4[d]) * W + (uint32_t)(x + dx4[d]);
                    if (seq_next + pos >= npx) { s_fail = 1u; break; }    // (cannot happen: a pixel is activated once)
                    P.acts[pos] = q;
                    P.seq[q] = npx + seq_next + pos;
                    P.seq2idx[seq_next + pos] = q;
                    ++pos;
                }
            }
            na += total;
        }
        __syncthreads();
        if (s_fail || seq_next + na > npx) { failed = true; break; }
        // 3. T and colour of the activated pixels by readiness: predecessors = same window, smaller A, inside the read set
        for (uint32_t i = tid; i < na; i += kHeapThreads) {
            const uint32_t q = P.acts[i], A = ld_l2(&P.akey[q]);
            const int y = (int)(q / (uint32_t)W), x = (int)(q - (uint32_t)y * (uint32_t)W);
            uint32_t c = 0;
            for (int o = 0; o < kNeedOffsets.n; ++o) {
                const int xx = x + kNeedOffsets.dx[o], yy = y + kNeedOffsets.dy[o];
                if (xx < 0 || xx >= W || yy < 0 || yy >= H) continue;
                if (ld_l2(&P.akey[(uint32_t)yy * W + xx]) < A) ++c;
            }
            P.cnt[q] = c;
            if (c == 0u) ready[0][atomicAdd(&s_nr, 1u)] = q;
        }
        __syncthreads();
        uint32_t nr = s_nr, rc = 0, done = 0;
        const int lane32 = tid & 31, hw = tid >> 5;
        float (*red)[kRedStride] = reinterpret_cast<float (*)[10][kRedStride]>(s_raw)[hw];
        uint32_t* wcol = reinterpret_cast<uint32_t*>(s_raw + kRedBytes) + 81 * hw;
        float* wt = reinterpret_cast<float*>(s_raw + kRedBytes + kColBytes) + 81 * hw;
        uint8_t* wkn = s_raw + kRedBytes + 2 * kColBytes + 84 * hw;
        const DiscPixel dp = kDisc[lane32];
        const int qv = 4 + ((lane32 & 1) ? 9 : -9), qh = 4 * 9 + 4 + ((lane32 & 2) ? 1 : -1);     // this lane's quadrant
        for (uint32_t round = 0; nr != 0u; ++round) {
            if (round > na) { failed = true; break; }
            // the ready pixels, one half-wave each: the 9 x 9 neighbourhood into LDS, then the shared estimate
            for (uint32_t j = (uint32_t)hw; j < nr; j += kHeapHalfWaves) {
                const uint32_t q = ready[rc][j];
                const int y = (int)(q / (uint32_t)W), x = (int)(q - (uint32_t)y * (uint32_t)W);
#pragma unroll
                for (int it = 0; it < 3; ++it) {
                    const int cell = lane32 + 32 * it;
                    if (cell >= 81) continue;
                    const int wy = cell / 9, wx = cell - 9 * wy;
                    const int xx = x - 4 + wx, yy = y - 4 + wy;
                    const bool inb = xx >= 0 && xx < W && yy >= 0 && yy < H;
                    const uint32_t oo = inb ? (uint32_t)yy * W + xx : q;
                    uint32_t col;
                    __builtin_memcpy(&col, P.img + 3 * (size_t)oo, 4);
                    wcol[cell] = col & 0xFFFFFFu;
                    wt[cell] = P.T[oo];
                    wkn[cell] = (inb && !(P.flags[oo] & kHeapInside)) ? 1 : 0;
                }
                __builtin_amdgcn_wave_barrier();
                const uint32_t out = telea_tile_estimate(wkn, wt, wcol, red, dp, lane32, qv, qh, [&](float t) { if (lane32 == 0) P.T[q] = t; });
                if (lane32 == 0) {
                    store_px_bytes(P.img, (int)q, out);
                    const uint8_t f = P.flags[q];
                    P.flags[q] = (uint8_t)(f & ~kHeapInside);
                    if (f & kHeapKeyPx) atomicSub(&s_keys_left, 1u);
                }
                __builtin_amdgcn_wave_barrier();               // (the half-wave's tile is rewritten for its next pixel)
            }
            __syncthreads();
            if (tid == 0) s_next[(round + 1) & 1] = 0u;      // (everybody has read it, as nr, before the barrier above)
            // their successors lose a predecessor; who takes the last one lists the pixel for the next round
            uint32_t* nxt = ready[rc ^ 1u];
            for (uint32_t j = tid; j < nr; j += kHeapThreads) {
                const uint32_t q = ready[rc][j], A = ld_l2(&P.akey[q]);
                const int y = (int)(q / (uint32_t)W), x = (int)(q - (uint32_t)y * (uint32_t)W);
                for (int o = 0; o < kNeedOffsets.n; ++o) {
                    const int xx = x + kNeedOffsets.dx[o], yy = y + kNeedOffsets.dy[o];
                    if (xx < 0 || xx >= W || yy < 0 || yy >= H) continue;
                    const uint32_t m = (uint32_t)yy * W + xx, am = ld_l2(&P.akey[m]);
                    if (am == kHeapNoKey || am < A) continue;
                    if (atomicSub(&P.cnt[m], 1u) == 1u) {
                        const uint32_t pos = atomicAdd(&s_next[round & 1], 1u);
                        if (pos < npx) nxt[pos] = m; else s_fail = 1u;
                    }
                }
            }
            __syncthreads();
            done += nr;
            nr = s_next[round & 1];
            rc ^= 1u;
        }
        if (failed || done != na) { failed = true; break; }
        // the next band: what was not popped, and the activated pixels (their keys go back to "none")
        for (uint32_t i = tid; i < na; i += kHeapThreads) {
            const uint32_t q = P.acts[i];
            P.akey[q] = kHeapNoKey;
            band_next[nk + i] = q;
        }
        __syncthreads();
        nb = nk + na;
        seq_next += na;
        uint32_t* t = band; band = band_next; band_next = t;
    }
    if (tid == 0) a.remaining[im] = failed ? 0xFFFFFFFFu : s_keys_left;
}

hipError_t launch_telea_heap(const ImageSet& seed, uint8_t* ws, size_t image_bytes, uint32_t* remaining, int n, int W, int H,
                             uint32_t key_rgb, hipStream_t s)
{
    const HeapArgs a{ws, image_bytes, remaining, W, H, key_rgb};
    hipLaunchKernelGGL(k_telea_heap, dim3(n), dim3(kHeapThreads), 0, s, seed, a);
    return hipGetLastError();
}

}  // namespace mdvt
