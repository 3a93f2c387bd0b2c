// mdvt_telea_levels.hip -- the infill-mask completion in level order (mdvt_finish_infill_mask's default; the heap order of
// cv2.inpaint is mdvt_telea_heap.hip, the per-pixel arithmetic both share mdvt_telea_common.h) and the masked blur behind it.
// Depends neither on the sub-pixel grid nor on MDVT_TUNING: compiled once and linked into both libraries; its run-time hooks
// (TUNE_TELEA_BLOCKS, TUNE_TELEA_DUMP, TUNE_BLUR_ONE_PASS) go through tuning_env(), which the link resolves.
//
// Compiled with -ffp-contract=off: see the arithmetic decree in mdvt_device.h / DESIGN.md.
#include "mdvt_telea_common.h"

#include <vector>
#include <stdio.h>
#include <stdlib.h>

namespace mdvt {

// =================================================================================================
// infill-mask completion (sr:803-808, 114-153): level-synchronous Telea inpaint + masked Gaussian
// =================================================================================================
// State per image: stamp u16 (0 known from the start, 0xFFFF unknown, r = filled in round r), T f32 (written by the fill pass only: known pixels read as 0), the work
// image (seed copy, filled in place).  Round r reads only pixels with stamp < r, so the in-place writes of the
// same round (stamp = r) are never observed: one launch = one Jacobi step, no double buffering.
constexpr uint16_t kTeleaUnknown = 0xFFFFu;
constexpr uint32_t kTeleaNeedBit = 0x8000u;        // from the list scatter on: top bit of a level word = "this pixel's estimate is needed"
constexpr uint32_t kTeleaLevelMask = 0x7FFFu;      // (levels stay below 32767: max_rounds <= 32766)
#ifndef MDVT_NC_STRIDE
#define MDVT_NC_STRIDE 32
#endif
// The per-level counters of needed pixels take the appends of every workgroup of a launch: atomics on one address serialise at
// ~4 ns each, and neighbouring levels' counters in one cache line queue behind each other -- one counter per 128-byte line.
constexpr uint32_t kNcStride = MDVT_NC_STRIDE;

// The level of a pixel -- the round in which the level-synchronous front reaches it -- is its 4-connected distance to the
// nearest known pixel: an L1 distance transform, two separable passes (A) instead of one dependent launch per level.
// Then, level by level, so that the expensive estimate only runs where the result can reach a hole:
//   A  k_telea_dt_rows / k_telea_dt_cols   stamp = L1 distance to the nearest known pixel (0 = known), capped at max_rounds;
//                                   per image last_round = the level of its deepest key-coloured pixel (later levels
//                                   are never needed) and remaining = key-coloured pixels beyond max_rounds;
//      (level sizes: last sweep of the transform) / k_telea_scan / k_telea_sort   offsets, and the key-coloured pixels
//                                   of level r appended to nlist[offs[r] ..) -- the first needed pixels of each level.
//   B  k_telea_need    r = R .. 2   which estimates are needed: key-coloured pixels, and every pixel of a lower
//                                   level that a needed pixel reads (its radius-3 disc and their 4-neighbours) -- which
//                                   also closes the set under "T of a pixel needs T of its lower 4-neighbours".  The launch
//                                   for level r walks the needed pixels of that level only (complete by then: levels are
//                                   1-Lipschitz, so they were all marked by levels r+1 .. r+5) and appends what it marks to
//                                   the lists of levels r-5 .. r-1; a pixel is appended by whoever sets its need flag first.
//   C  k_telea_fill    r = 1 .. R   T (FastMarching_solve over the four quadrants) and Telea's estimate for the needed
//                                   pixels of level r, reading levels < r.
// A black (non-hole) pixel that no key-coloured pixel depends on is never estimated -- it returns to black at
// sr:807 anyway -- which removes ~90 % of the estimates (and T solves) of a front that also grows outwards from the
// holes.  R (the deepest level any image needs) is read back by the host after pass A: passes B and C are launched
// for exactly the levels that exist (round 1 launched all max_rounds levels of all three passes, 768 launches of which
// ~620 found nothing to do).
struct TeleaArgs {
    uint16_t* stamp; float* T; uint8_t* img;      // [n][H*W] / [n][H*W*3]
    uint8_t* need;                                // [n][H*W] 1 = this pixel's estimate is needed (and it is in nlist)
    uint32_t* nlist;                              // the needed pixels of each level; level r owns [offs[r], offs[r] + counts[r])
    uint32_t* counts;                             // [max_rounds + 2] level sizes (all pixels of the level: the capacity of its nlist part)
    uint32_t* offs;                               // [max_rounds + 2] level offsets into nlist
    uint32_t* ncounts;                            // [max_rounds + 2] needed pixels per level so far
    uint32_t* remaining;                          // [n] key-coloured pixels not reached yet
    uint32_t* last_round;                         // [n]
    int W, H, n;
    uint32_t key_rgb;
};

constexpr int kDtInf = 1 << 20;          // "no known pixel in this direction" (any real distance is < 2^17)

// T is zeroed with a memset beforehand; this pass writes 0 (known) / 0xFFFF (to fill) stamps, the need flags (key-coloured
// pixels) and the work image.
template <int PX>
__global__ void __launch_bounds__(128) k_telea_init(ImageSet seed, TeleaArgs a)
{
    const int g = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y, im = blockIdx.z;
    const int W = a.W, H = a.H;
    if (g * PX >= W) return;
    const size_t o = (size_t)im * W * H + (size_t)y * W + (size_t)g * PX;
    uint32_t px[PX];
    RowIO<PX>::load(seed.image(im) + (size_t)y * seed.pitch, g, px);
    uint32_t st = 0, nd = 0;
#pragma unroll
    for (int q = 0; q < PX; ++q) {
        const bool green = px[q] == a.key_rgb;
        if (green || px[q] == 0u) {                                        // sr:803-805: key-coloured or black = to inpaint
            if (PX == 4) { if (q < 2) st |= (uint32_t)kTeleaUnknown << (16 * q); }
            else a.stamp[o + q] = kTeleaUnknown;
        } else if (PX != 4) a.stamp[o + q] = 0;
        if (PX == 4) nd |= (green ? 1u : 0u) << (8 * q); else a.need[o + q] = green ? 1 : 0;
    }
    if (PX == 4) {
        uint32_t st1 = 0;
#pragma unroll
        for (int q = 2; q < 4; ++q) if (px[q] == a.key_rgb || px[q] == 0u) st1 |= (uint32_t)kTeleaUnknown << (16 * (q - 2));
        *reinterpret_cast<uint2*>(a.stamp + o) = make_uint2(st, st1);
        *reinterpret_cast<uint32_t*>(a.need + o) = nd;
    }
    RowIO<PX>::store_rgb(a.img + 3 * ((size_t)im * W * H + (size_t)y * W), g, px);
}

// Pass A, rows: stamp[x] = distance to the nearest known pixel of the same row (0xFFFF: none), in place.  One workgroup per
// (row, image); a thread owns a contiguous segment, the nearest known pixels outside it come from a block-wide scan.
__global__ void __launch_bounds__(256) k_telea_dt_rows(uint16_t* __restrict__ stamp, int W, int H)
{
    __shared__ int sl[256], sf[256];
    uint16_t* d = stamp + ((size_t)blockIdx.y * H + blockIdx.x) * W;
    const int t = threadIdx.x;
    const int seg = (W + 255) / 256, x0 = min(t * seg, W), x1 = min(x0 + seg, W);
    int last = -kDtInf, first = kDtInf;
    for (int x = x0; x < x1; ++x)
        if (d[x] == 0) { last = x; if (first == kDtInf) first = x; }
    sl[t] = last; sf[t] = first;
    __syncthreads();
    for (int off = 1; off < 256; off <<= 1) {            // inclusive prefix max of `last`, inclusive suffix min of `first`
        const int vl = t >= off ? sl[t - off] : -kDtInf, vf = t + off < 256 ? sf[t + off] : kDtInf;
        __syncthreads();
        sl[t] = max(sl[t], vl); sf[t] = min(sf[t], vf);
        __syncthreads();
    }
    int run = t > 0 ? sl[t - 1] : -kDtInf;                // nearest known pixel left of the segment
    for (int x = x0; x < x1; ++x) {
        if (d[x] == 0) run = x;
        const int v = x - run;
        d[x] = (uint16_t)(v < 0xFFFF ? v : 0xFFFF);
    }
    run = t < 255 ? sf[t + 1] : kDtInf;                   // ... and right of it
    for (int x = x1 - 1; x >= x0; --x) {
        if (d[x] == 0) run = x;
        const int v = run - x;
        if (v < (int)d[x]) d[x] = (uint16_t)v;
    }
}

// The same with 16-byte row accesses: a thread owns 8 * VEC consecutive pixels (W % 8 == 0, W <= 2048 * VEC).
template <int VEC>
__global__ void __launch_bounds__(256) k_telea_dt_rows_vec(uint16_t* __restrict__ stamp, int W, int H)
{
    __shared__ int sl[256], sf[256];
    uint16_t* d = stamp + ((size_t)blockIdx.y * H + blockIdx.x) * W;
    const int t = threadIdx.x;
    constexpr int N = 8 * VEC;
    const int x0 = t * N;
    uint32_t w[4 * VEC];
#pragma unroll
    for (int v = 0; v < VEC; ++v) {
        uint4 q = make_uint4(~0u, ~0u, ~0u, ~0u);                       // past the row end: "unknown", never a zero
        if (x0 + 8 * v < W) q = *reinterpret_cast<const uint4*>(d + x0 + 8 * v);
        w[4 * v] = q.x; w[4 * v + 1] = q.y; w[4 * v + 2] = q.z; w[4 * v + 3] = q.w;
    }
    auto val = [&](int k) { return (w[k >> 1] >> (16 * (k & 1))) & 0xFFFFu; };
    int last = -kDtInf, first = kDtInf;
#pragma unroll
    for (int k = 0; k < N; ++k)
        if (val(k) == 0u) { last = x0 + k; if (first == kDtInf) first = x0 + k; }
    sl[t] = last; sf[t] = first;
    __syncthreads();
    for (int off = 1; off < 256; off <<= 1) {            // inclusive prefix max of `last`, inclusive suffix min of `first`
        const int vl = t >= off ? sl[t - off] : -kDtInf, vf = t + off < 256 ? sf[t + off] : kDtInf;
        __syncthreads();
        sl[t] = max(sl[t], vl); sf[t] = min(sf[t], vf);
        __syncthreads();
    }
    int out[N];
    int run = t > 0 ? sl[t - 1] : -kDtInf;
#pragma unroll
    for (int k = 0; k < N; ++k) {
        if (val(k) == 0u) run = x0 + k;
        out[k] = min(x0 + k - run, 0xFFFF);
    }
    run = t < 255 ? sf[t + 1] : kDtInf;
#pragma unroll
    for (int k = N - 1; k >= 0; --k) {
        if (val(k) == 0u) run = x0 + k;
        out[k] = min(out[k], run - (x0 + k));
    }
#pragma unroll
    for (int v = 0; v < VEC; ++v) {
        if (x0 + 8 * v >= W) continue;
        uint4 q;
        q.x = (uint32_t)out[8 * v] | ((uint32_t)out[8 * v + 1] << 16); q.y = (uint32_t)out[8 * v + 2] | ((uint32_t)out[8 * v + 3] << 16);
        q.z = (uint32_t)out[8 * v + 4] | ((uint32_t)out[8 * v + 5] << 16); q.w = (uint32_t)out[8 * v + 6] | ((uint32_t)out[8 * v + 7] << 16);
        *reinterpret_cast<uint4*>(d + x0 + 8 * v) = q;
    }
}

constexpr int kLevelBins = 4096;      // levels counted / slotted in LDS; deeper ones go straight to the global counters

// Pass A, columns: the two sweeps of the L1 transform (down: D[y] = min(D[y-1] + 1, d[y]); up the same from below), in
// place.  One workgroup = 64 columns x 16 row segments; the value entering a segment comes from a scan over the segments'
// exit values.  The last sweep also caps the level at max_rounds and collects, per image, the deepest key-coloured level
// (last_round) and the number of key-coloured pixels beyond the cap (remaining).
__global__ void __launch_bounds__(1024) k_telea_dt_cols(TeleaArgs a, uint32_t max_rounds)
{
    __shared__ int ex[16][64], carry[16][64];
    __shared__ uint32_t s_rem, s_max;
    __shared__ uint32_t hist[kLevelBins];          // the level sizes (every reached pixel), added to a.counts at the end
    const int W = a.W, H = a.H;
    const int cx = threadIdx.x & 63, sg = threadIdx.x >> 6;
    const int x = blockIdx.x * 64 + cx, im = blockIdx.y;
    const bool act = x < W;
    const int seglen = (H + 15) / 16, y0 = min(sg * seglen, H), y1 = min(y0 + seglen, H);
    const size_t base = (size_t)im * W * H + (act ? x : 0);
    uint16_t* d = a.stamp + base;
    if (threadIdx.x == 0) { s_rem = 0u; s_max = 0u; }
    for (int b = threadIdx.x; b < kLevelBins; b += 1024) hist[b] = 0u;
    auto val = [&](int y) { const int v = d[(size_t)y * W]; return v == 0xFFFF ? kDtInf : v; };
    auto put = [&](int y, int v) { d[(size_t)y * W] = (uint16_t)(v < 0xFFFF ? v : 0xFFFF); };
    // ---- down ----
    int run = kDtInf;
    if (act) for (int y = y0; y < y1; ++y) run = min(run + 1, val(y));
    ex[sg][cx] = run;
    __syncthreads();
    if (sg == 0) {
        int c = kDtInf;
        for (int q = 0; q < 16; ++q) {
            carry[q][cx] = c;
            const int len = min((q + 1) * seglen, H) - min(q * seglen, H);
            c = min(ex[q][cx], c + len);
        }
    }
    __syncthreads();
    run = carry[sg][cx];
    if (act) for (int y = y0; y < y1; ++y) { run = min(run + 1, val(y)); put(y, run); }
    __syncthreads();            // (a column's segments are all in this workgroup: its writes above are visible below)
    // ---- up ----
    run = kDtInf;
    if (act) for (int y = y1 - 1; y >= y0; --y) run = min(run + 1, val(y));
    ex[sg][cx] = run;
    __syncthreads();
    if (sg == 0) {
        int c = kDtInf;
        for (int q = 15; q >= 0; --q) {
            carry[q][cx] = c;
            const int len = min((q + 1) * seglen, H) - min(q * seglen, H);
            c = min(ex[q][cx], c + len);
        }
    }
    __syncthreads();
    run = carry[sg][cx];
    uint32_t rem = 0, lmax = 0;
    if (act) {
        const uint8_t* key = a.need + base;
        for (int y = y1 - 1; y >= y0; --y) {
            run = min(run + 1, val(y));
            const bool reached = run <= (int)max_rounds;
            d[(size_t)y * W] = reached ? (uint16_t)run : kTeleaUnknown;
            if (reached && run >= 1) { if (run < kLevelBins) atomicAdd(&hist[run], 1u); else atomicAdd(&a.counts[run], 1u); }
            if (key[(size_t)y * W]) { if (reached) lmax = max(lmax, (uint32_t)run); else ++rem; }
        }
    }
    if (rem) atomicAdd(&s_rem, rem);
    if (lmax) atomicMax(&s_max, lmax);
    __syncthreads();
    if (threadIdx.x == 0) {
        if (s_rem) atomicAdd(&a.remaining[im], s_rem);
        if (s_max) atomicMax(&a.last_round[im], s_max);
    }
    for (int b = threadIdx.x; b < kLevelBins; b += 1024)
        if (hist[b]) atomicAdd(&a.counts[b], hist[b]);
}

// The same with a column segment held in registers between the sweeps (H <= 16 * SEG): the stamps are read once and
// written once instead of four times and twice.
template <int SEG>
__global__ void __launch_bounds__(1024) k_telea_dt_cols_reg(TeleaArgs a, uint32_t max_rounds)
{
    __shared__ int ex[16][64], carry[16][64];
    __shared__ uint32_t s_rem, s_max;
    __shared__ uint32_t hist[kLevelBins];          // the level sizes (every reached pixel), added to a.counts at the end
    const int W = a.W, H = a.H;
    const int cx = threadIdx.x & 63, sg = threadIdx.x >> 6;
    const int x = blockIdx.x * 64 + cx, im = blockIdx.y;
    const bool act = x < W;
    const int seglen = (H + 15) / 16, y0 = min(sg * seglen, H), y1 = min(y0 + seglen, H);
    const int len = act ? y1 - y0 : 0;
    const size_t base = (size_t)im * W * H + (act ? x : 0);
    uint16_t* d = a.stamp + base;
    if (threadIdx.x == 0) { s_rem = 0u; s_max = 0u; }
    for (int b = threadIdx.x; b < kLevelBins; b += 1024) hist[b] = 0u;
    int v[SEG];
#pragma unroll
    for (int k = 0; k < SEG; ++k) {
        v[k] = kDtInf;
        if (k < len) { const int q = d[(size_t)(y0 + k) * W]; v[k] = q == 0xFFFF ? kDtInf : q; }
    }
    // ---- down ----
    int run = kDtInf;
#pragma unroll
    for (int k = 0; k < SEG; ++k) if (k < len) run = min(run + 1, v[k]);
    ex[sg][cx] = run;
    __syncthreads();
    if (sg == 0) {
        int c = kDtInf;
        for (int q = 0; q < 16; ++q) {
            carry[q][cx] = c;
            const int l = min((q + 1) * seglen, H) - min(q * seglen, H);
            c = min(ex[q][cx], c + l);
        }
    }
    __syncthreads();
    run = carry[sg][cx];
#pragma unroll
    for (int k = 0; k < SEG; ++k) if (k < len) { run = min(run + 1, v[k]); v[k] = run; }
    __syncthreads();
    // ---- up ----
    run = kDtInf;
#pragma unroll
    for (int k = SEG - 1; k >= 0; --k) if (k < len) run = min(run + 1, v[k]);
    ex[sg][cx] = run;
    __syncthreads();
    if (sg == 0) {
        int c = kDtInf;
        for (int q = 15; q >= 0; --q) {
            carry[q][cx] = c;
            const int l = min((q + 1) * seglen, H) - min(q * seglen, H);
            c = min(ex[q][cx], c + l);
        }
    }
    __syncthreads();
    run = carry[sg][cx];
    uint32_t rem = 0, lmax = 0;
    const uint8_t* key = a.need + base;
#pragma unroll
    for (int k = SEG - 1; k >= 0; --k) {
        if (k >= len) continue;
        run = min(run + 1, v[k]);
        const bool reached = run <= (int)max_rounds;
        d[(size_t)(y0 + k) * W] = reached ? (uint16_t)run : kTeleaUnknown;
        if (reached && run >= 1) { if (run < kLevelBins) atomicAdd(&hist[run], 1u); else atomicAdd(&a.counts[run], 1u); }
        if (key[(size_t)(y0 + k) * W]) { if (reached) lmax = max(lmax, (uint32_t)run); else ++rem; }
    }
    if (rem) atomicAdd(&s_rem, rem);
    if (lmax) atomicMax(&s_max, lmax);
    __syncthreads();
    if (threadIdx.x == 0) {
        if (s_rem) atomicAdd(&a.remaining[im], s_rem);
        if (s_max) atomicMax(&a.last_round[im], s_max);
    }
    for (int b = threadIdx.x; b < kLevelBins; b += 1024)
        if (hist[b]) atomicAdd(&a.counts[b], hist[b]);
}

// counts[0] = the deepest level any image needs (the host reads it back: passes B and C get exactly that many launches)
__global__ void k_telea_rmax(TeleaArgs a)
{
    uint32_t m = 0;
    for (int im = 0; im < a.n; ++im) m = max(m, a.last_round[im]);
    a.counts[0] = m;
}

// The first entries of the level lists: the key-coloured pixels.  (The level sizes -- every reached pixel of a level, the room
// its list may need -- are counted by the last sweep of the distance transform.)  A workgroup takes a 64 x 64 tile of one
// image -- so that the pixels of a level stay together tile by tile in the list, and the half-waves that later work through
// consecutive list entries read overlapping 9 x 9 neighbourhoods --; levels below kLevelBins are slotted in LDS first (one
// global atomic per occupied level and workgroup), deeper ones directly.
constexpr int kSortTile = 64;

__global__ void __launch_bounds__(256) k_telea_sort(TeleaArgs a)
{
    __shared__ uint32_t hist[kLevelBins];
    __shared__ uint32_t slot[kLevelBins];
    const int im = blockIdx.y;
    const uint32_t lr = a.last_round[im];
    if (lr == 0u) return;                                   // nothing key-coloured (or nothing reachable): nothing to do
    const uint32_t npx = (uint32_t)a.W * (uint32_t)a.H;
    const int tiles_x = (a.W + kSortTile - 1) / kSortTile;
    const int tx0 = (int)(blockIdx.x % tiles_x) * kSortTile, ty0 = (int)(blockIdx.x / tiles_x) * kSortTile;
    // a thread takes four consecutive pixels of a row (one dword of need flags where the row allows it): 16 threads per tile
    // row, 16 rows per step, 4 steps
    const int lx = (threadIdx.x & 15) * 4, ly0 = threadIdx.x >> 4;
    const uint16_t* st = a.stamp + (size_t)im * npx;
    const uint8_t* nd = a.need + (size_t)im * npx;
    const bool dwords = (a.W & 3) == 0;                     // (then every row starts on a dword of the flag plane)
    for (int b = threadIdx.x; b < kLevelBins; b += 256) hist[b] = 0u;
    __syncthreads();
    constexpr int kSteps = kSortTile / 16;
    uint32_t lv[kSteps][4];
#pragma unroll
    for (int k = 0; k < kSteps; ++k) {
        const int px = tx0 + lx, py = ty0 + ly0 + 16 * k;
        const uint32_t o = (uint32_t)py * (uint32_t)a.W + (uint32_t)px;
        uint32_t flags = 0;
        if (py < a.H) {
            if (dwords && px + 3 < a.W) flags = *reinterpret_cast<const uint32_t*>(nd + o);
            else {
#pragma unroll
                for (int q = 0; q < 4; ++q) if (px + q < a.W && nd[o + q]) flags |= 1u << (8 * q);
            }
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            lv[k][q] = 0u;
            if ((flags >> (8 * q)) & 0xFFu) {               // key-coloured (~4 % of the pixels): only those look their level up
                const uint32_t sv = st[o + q];
                if (sv >= 1u && sv <= lr) {
                    lv[k][q] = sv;
                    a.stamp[(size_t)im * npx + o + q] = (uint16_t)(sv | kTeleaNeedBit);      // needed from the start
                    if (sv < (uint32_t)kLevelBins) atomicAdd(&hist[sv], 1u);
                }
            }
        }
    }
    __syncthreads();
    for (int b = threadIdx.x; b < kLevelBins; b += 256) {
        const uint32_t c = hist[b];
        if (!c) continue;
        slot[b] = atomicAdd(&a.ncounts[(uint32_t)b * kNcStride], c); hist[b] = 0u;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < kSteps; ++k)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const uint32_t l = lv[k][q];
            if (!l) continue;
            const uint32_t e = (uint32_t)im * npx + (uint32_t)(ty0 + ly0 + 16 * k) * (uint32_t)a.W + (uint32_t)(tx0 + lx + q);
            const uint32_t pos = l < (uint32_t)kLevelBins ? slot[l] + atomicAdd(&hist[l], 1u) : atomicAdd(&a.ncounts[l * kNcStride], 1u);
            a.nlist[a.offs[l] + pos] = e;
        }
}

// offs[r] = counts[1] + ... + counts[r-1] for r = 1 .. n_levels + 1 (level 1 starts at 0).  One workgroup.
__global__ void __launch_bounds__(1024) k_telea_scan(TeleaArgs a, int n_levels)
{
    __shared__ uint32_t part[1024];
    const int t = threadIdx.x, n = n_levels + 1;             // entries 1 .. n
    const int per = (n + 1023) / 1024, lo = min(1 + t * per, n + 1), hi = min(lo + per, n + 1);
    uint32_t sum = 0;
    for (int k = lo; k < hi; ++k) sum += a.counts[k];
    part[t] = sum;
    __syncthreads();
    for (int off = 1; off < 1024; off <<= 1) {
        const uint32_t v = t >= off ? part[t - off] : 0u;
        __syncthreads();
        part[t] += v;
        __syncthreads();
    }
    uint32_t run = part[t] - sum;
    for (int k = lo; k < hi; ++k) { a.offs[k] = run; run += a.counts[k]; }
}

// (telea_solve and kNeedOffsets, the read set of an estimate: mdvt_telea_common.h)
constexpr int kNeedLanes = 8;            // lanes sharing the 56 offsets of one needed pixel
constexpr int kNeedStage = 512;          // newly marked pixels a workgroup collects per target level before it appends them

__global__ void __launch_bounds__(256) k_telea_need(TeleaArgs a, uint32_t r)
{
    __shared__ uint32_t stage[5][kNeedStage];
    __shared__ uint32_t cnt[5], base[5];
    const uint32_t count = a.ncounts[r * kNcStride], off = a.offs[r];
    constexpr uint32_t per_block = 256 / kNeedLanes;
    // XCD-aware dealing (workgroup b runs on XCD b % 8, each XCD has its own L2): every XCD walks one contiguous eighth of the
    // level's list -- neighbouring entries are neighbouring pixels, whose 9 x 9 windows share their cache lines
    const uint32_t xcd = blockIdx.x & 7u, slot = blockIdx.x >> 3, nslot = gridDim.x >> 3;
    const uint32_t per_xcd = (count + 7u) >> 3, lo_x = xcd * per_xcd, hi_x = min(lo_x + per_xcd, count);
    if (lo_x + slot * per_block >= hi_x) return;                       // (workgroup-uniform)
    const int W = a.W, H = a.H;
    const uint32_t npx = (uint32_t)W * (uint32_t)H;
    if (threadIdx.x < 5) cnt[threadIdx.x] = 0u;
    __syncthreads();
    const int sub = threadIdx.x & (kNeedLanes - 1);
    // (from the list scatter on, "needed" is the top bit of a pixel's level word: one load tells level and flag)
    uint32_t* stamp_words = reinterpret_cast<uint32_t*>(a.stamp);
    uint32_t idx = lo_x + slot * per_block + threadIdx.x / kNeedLanes;
    uint32_t e_next = idx < hi_x ? a.nlist[off + idx] : 0u;
    for (; idx < hi_x; idx += nslot * per_block) {
        const uint32_t e = e_next, im = e / npx, o = e - im * npx;
        if (idx + nslot * per_block < hi_x) e_next = a.nlist[off + idx + nslot * per_block];     // (in flight during this entry)
        const int y = (int)(o / (uint32_t)W), x = (int)(o - (uint32_t)y * (uint32_t)W);
        const size_t ib = (size_t)im * npx;
        // three rounds with everything of a round in flight together (a loop over the lane's offsets with the flag test, the
        // atomic and the append inside is seven dependent round trips to L2 per entry: the floor of a level's launch)
        constexpr int kPer = (56 + kNeedLanes - 1) / kNeedLanes;
        static_assert(kPer * kNeedLanes >= 56, "every offset has a lane");
        uint32_t uu[kPer], su[kPer], old[kPer];
        bool want[kPer];
#pragma unroll
        for (int k = 0; k < kPer; ++k) {
            const int q = sub + k * kNeedLanes;
            const int xx = x + kNeedOffsets.dx[q < kNeedOffsets.n ? q : 0], yy = y + kNeedOffsets.dy[q < kNeedOffsets.n ? q : 0];
            const bool in = q < kNeedOffsets.n && xx >= 0 && xx < W && yy >= 0 && yy < H;
            uu[k] = in ? (uint32_t)(ib + (size_t)yy * W + xx) : e;           // (the entry itself: level r, never marked)
            const uint32_t sw = a.stamp[uu[k]];
            su[k] = sw & kTeleaLevelMask;
            want[k] = su[k] != 0u && su[k] < r && !(sw & kTeleaNeedBit);
        }
#pragma unroll
        for (int k = 0; k < kPer; ++k) {
            const uint32_t bit = kTeleaNeedBit << (16u * (uu[k] & 1u));
            old[k] = bit;                                                      // "already set"
            if (want[k]) old[k] = atomicOr(stamp_words + (uu[k] >> 1), bit);
        }
#pragma unroll
        for (int k = 0; k < kPer; ++k) {
            if (old[k] & (kTeleaNeedBit << (16u * (uu[k] & 1u)))) continue;    // flag was set: somebody else appends (or has appended) it
            const uint32_t d = r - 1u - su[k];
            const uint32_t pos = d < 5u ? atomicAdd(&cnt[d], 1u) : (uint32_t)kNeedStage;
            if (pos < (uint32_t)kNeedStage) stage[d][pos] = uu[k];
            else a.nlist[a.offs[su[k]] + atomicAdd(&a.ncounts[su[k] * kNcStride], 1u)] = uu[k];
        }
    }
    __syncthreads();
    if (threadIdx.x < 5) {
        const uint32_t n = min(cnt[threadIdx.x], (uint32_t)kNeedStage);
        cnt[threadIdx.x] = n;
        base[threadIdx.x] = n ? a.offs[r - 1u - threadIdx.x] + atomicAdd(&a.ncounts[(r - 1u - threadIdx.x) * kNcStride], n) : 0u;
    }
    __syncthreads();
#pragma unroll
    for (int d = 0; d < 5; ++d)
        for (uint32_t i = threadIdx.x; i < cnt[d]; i += 256) a.nlist[base[d] + i] = stage[d][i];
}

// Pass C, lane-parallel: one half-wave (32 lanes) per needed pixel, lane j < 28 = disc pixel j.  The 9 x 9 neighbourhood is
// fetched once into LDS, coalesced along its rows; T comes from four lanes solving one quadrant each; every lane weighs
// its own disc pixel; the 10 running sums (Ia, Jx, Jy per channel and the weight) are then added up in the oracle's order
// j = 0..27 by 10 lanes reading the terms back from LDS -- the same left-to-right f32 chain as the oracle's loop, so the
// result is bit-identical to it (telea_tile_estimate, mdvt_telea_common.h).  (The level's latency is what bounds the deep levels,
// instruction issue the first ones.)
__global__ void __launch_bounds__(256) k_telea_fill(TeleaArgs a, uint32_t r)
{
    const uint32_t off = a.offs[r];
    const int W = a.W, H = a.H;
    const uint32_t npx = (uint32_t)W * (uint32_t)H;
    __shared__ __attribute__((aligned(16))) float red[8][10][kRedStride];
    __shared__ uint32_t wcol[8][81];
    __shared__ float wt[8][81];
    __shared__ uint8_t wkn[8][84];
    const int lane32 = threadIdx.x & 31, hw = threadIdx.x >> 5;
    const uint32_t nneed = a.ncounts[r * kNcStride];
    const DiscPixel dp = kDisc[lane32];
    const int qv = 4 + ((lane32 & 1) ? 9 : -9), qh = 4 * 9 + 4 + ((lane32 & 2) ? 1 : -1);     // this lane's quadrant: cells (0, +-1) and (+-1, 0)
    // every entry of nlist is a pixel to estimate: they are dealt round-robin to all half-waves of the grid
    // (XCD-aware dealing as in the need pass: one contiguous eighth of the list per XCD)
    const uint32_t xcd = blockIdx.x & 7u, slot = blockIdx.x >> 3, nslot = gridDim.x >> 3;
    const uint32_t per_xcd = (nneed + 7u) >> 3, lo_x = xcd * per_xcd, hi_x = min(lo_x + per_xcd, nneed);
    // Software pipeline over a half-wave's pixels: the neighbourhood of pixel i + 1 (loads into registers) and the list index of
    // pixel i + 2 are in flight while pixel i is worked out from LDS -- pixels of one level never read each other's results.
    struct Cells { uint32_t c[3]; float t[3]; uint32_t sv[3]; bool inb[3]; };
    auto fetch = [&](uint32_t e, Cells& p) {
        const uint32_t im = e / npx, o = e - im * npx;
        const int y = (int)(o / (uint32_t)W), x = (int)(o - (uint32_t)y * (uint32_t)W);
        const size_t ib = (size_t)im * npx;
        const uint16_t* stamp = a.stamp + ib;
        const float* Tm = a.T + ib;
        const uint8_t* img = a.img + 3 * ib;
#pragma unroll
        for (int it = 0; it < 3; ++it) {
            const int q = min(lane32 + 32 * it, 80);                  // (lanes past cell 80 repeat it: their values are not committed)
            const int wy = q / 9, wx = q - 9 * wy;
            const int xx = x - 4 + wx, yy = y - 4 + wy;
            p.inb[it] = xx >= 0 && xx < W && yy >= 0 && yy < H;
            const size_t oo = (size_t)(p.inb[it] ? yy : y) * W + (p.inb[it] ? xx : x);
            __builtin_memcpy(&p.c[it], img + 3 * oo, 4);              // unaligned dword: the work image is padded by 4 bytes
            p.sv[it] = stamp[oo];
            p.t[it] = Tm[oo];
        }
    };
    auto commit = [&](const Cells& p) {
#pragma unroll
        for (int it = 0; it < 3; ++it) {
            const int q = lane32 + 32 * it;
            if (q >= 81) continue;
            const uint32_t sv = p.sv[it] & kTeleaLevelMask;           // (an unreached pixel, 0xFFFF, stays beyond every level)
            wcol[hw][q] = p.c[it] & 0xFFFFFFu;
            wt[hw][q] = sv == 0u ? 0.0f : p.t[it];                    // T = 0 at every originally known pixel (nobody writes it there)
            wkn[hw][q] = (p.inb[it] && sv < r) ? 1 : 0;
        }
    };
    const uint32_t stride = nslot * 8;
    uint32_t k = lo_x + slot * 8 + hw;
    uint32_t e_cur = k < hi_x ? a.nlist[off + k] : 0u;
    uint32_t e_next = k + stride < hi_x ? a.nlist[off + k + stride] : 0u;
    Cells cells;
    if (k < hi_x) fetch(e_cur, cells);
    for (; k < hi_x; k += stride) {                                                         // half-wave uniform
        const uint32_t e = e_cur, im = e / npx, o = e - im * npx;
        const size_t ib = (size_t)im * npx;
        commit(cells);
        e_cur = e_next;
        if (k + stride < hi_x) fetch(e_cur, cells);
        if (k + 2 * stride < hi_x) e_next = a.nlist[off + k + 2 * stride];
        __builtin_amdgcn_wave_barrier();                   // LDS is in order within a wave: the reads below see these writes
        const uint8_t* kn = wkn[hw];
        const float* tt = wt[hw];
        const uint32_t* cc = wcol[hw];
        const uint32_t out = telea_tile_estimate(kn, tt, cc, red[hw], dp, lane32, qv, qh, [&](float t) { if (lane32 == 0) a.T[e] = t; });
        if (lane32 == 0) store_px_bytes(a.img + 3 * ib, (int)o, out);
    }
}

// sr:807: only the key-coloured pixels take the inpainted value, black ones go back to black; then masked_blur.
// Both in one pass: the 36 taps read the work image and zero it on the fly where the seed was black.
struct BlurSrc { const uint8_t* ibase; const uint8_t* sbase; size_t img_pitch, seed_pitch; bool masked; };

__device__ __forceinline__ uint32_t blur_px(const BlurSrc& b, int x, int y)
{
    uint32_t c = load_px_bytes(b.ibase + (size_t)y * b.img_pitch, x);
    if (b.masked && load_px_bytes(b.sbase + (size_t)y * b.seed_pitch, x) == 0u) c = 0u;
    return c;
}

// The 6 x 6 correlation around a non-black pixel (a black pixel stays black whatever surrounds it, sr:151).
__device__ __forceinline__ uint32_t masked_blur_pixel(const BlurSrc& b, int x, int y, int W, int H, const BlurKernel& K)
{
    float acc[3] = {0.0f, 0.0f, 0.0f}, wsum = 0.0f;
    uint32_t centre = 0;
#pragma unroll
    for (int ky = 0; ky < 6; ++ky) {
        const int sy = y + ky - 3;
        if (sy < 0 || sy >= H) continue;
#pragma unroll
        for (int kx = 0; kx < 6; ++kx) {
            const int sx = x + kx - 3;
            if (sx < 0 || sx >= W) continue;
            const uint32_t px = blur_px(b, sx, sy);
            const float k = K.k[6 * ky + kx];
#pragma unroll
            for (int c = 0; c < 3; ++c) acc[c] = acc[c] + k * (float)((px >> (8 * c)) & 0xFF);
            if (px) wsum = wsum + k;
            if (ky == 3 && kx == 3) centre = px;
        }
    }
    uint32_t o = 0;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        float v = (wsum == 0.0f || centre == 0u) ? 0.0f : acc[c] / wsum;
        v = fminf(fmaxf(v, 0.0f), 255.0f);
        o |= (uint32_t)v << (8 * c);
    }
    return o;
}

__device__ __forceinline__ BlurSrc blur_src(const ImageSet& imgs, const ImageSet& seeds, int im, uint32_t key_rgb)
{
    return BlurSrc{imgs.image(im), seeds.base ? seeds.image(im) : nullptr, imgs.pitch, seeds.pitch, seeds.base != nullptr && key_rgb != 0u};
}

__global__ void __launch_bounds__(256) k_masked_blur(ImageSet imgs, ImageSet seeds, ImageSet outs, int W, int H, BlurKernel K,
                                                     uint32_t key_rgb)
{
    const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y, im = blockIdx.z;
    if (x >= W) return;
    const BlurSrc b = blur_src(imgs, seeds, im, key_rgb);
    uint8_t* orow = outs.image(im) + (size_t)y * outs.pitch;
    if (blur_px(b, x, y) == 0u) { store_px_bytes(orow, x, 0u); return; }
    store_px_bytes(orow, x, masked_blur_pixel(b, x, y, W, H, K));
}

// The same in two passes, for images that are mostly black (an infill mask is: ~4 % of its pixels are not, in strips a few
// pixels wide -- a wave of 64 consecutive pixels that meets one runs all 36 taps for a handful of lanes): the first pass
// writes the black pixels and lists the columns of the others row by row (a counter per image row: one counter for the whole
// pass serialised 3 * 10^5 atomics on one address, 1.2 ms), the second gives every lane of a row's wave a listed pixel.
template <int PX>      // 4: rows addressable as dwords (12 bytes per lane), 1: any width / alignment
__global__ void __launch_bounds__(128) k_masked_blur_scan(ImageSet imgs, ImageSet seeds, ImageSet outs, int W, int H, uint32_t key_rgb,
                                                          uint32_t* __restrict__ list, uint32_t* __restrict__ row_count)
{
    const int g = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y, im = blockIdx.z;
    uint32_t c[PX];
#pragma unroll
    for (int q = 0; q < PX; ++q) c[q] = 0u;
    const bool in = g * PX < W;
    uint8_t* orow = outs.image(im) + (size_t)y * outs.pitch;
    if (in) {
        uint8_t* irow = imgs.image(im) + (size_t)y * imgs.pitch;
        RowIO<PX>::load(irow, g, c);
        if (seeds.base && key_rgb != 0u) {
            uint32_t sd[PX];
            RowIO<PX>::load(seeds.image(im) + (size_t)y * seeds.pitch, g, sd);
#pragma unroll
            for (int q = 0; q < PX; ++q)
                if (sd[q] == 0u && c[q] != 0u) {           // an estimate nobody keeps (sr:807): black in the work image too, so that the
                    c[q] = 0u;                              // second pass reads one image per tap instead of two
                    store_px_bytes(irow, g * PX + q, 0u);
                }
        }
        bool any = false;
#pragma unroll
        for (int q = 0; q < PX; ++q) any |= c[q] != 0u;
        if (!any) { const uint32_t z[PX] = {}; RowIO<PX>::store_rgb(orow, g, z); }
        else {
#pragma unroll
            for (int q = 0; q < PX; ++q) if (c[q] == 0u) store_px_bytes(orow, g * PX + q, 0u);
        }
    }
    u64 m[PX];
    uint32_t total = 0;
#pragma unroll
    for (int q = 0; q < PX; ++q) { m[q] = __ballot(c[q] != 0u); total += (uint32_t)__popcll(m[q]); }
    if (total) {
        const size_t row = (size_t)im * H + y;
        const int lane = threadIdx.x & 63;
        uint32_t base = 0;
        if (lane == 0) base = atomicAdd(&row_count[row], total);
        base = __shfl(base, 0);
#pragma unroll
        for (int q = 0; q < PX; ++q) {
            if (c[q] != 0u) list[row * (size_t)W + base + (uint32_t)__popcll(m[q] & ((1ull << lane) - 1ull))] = (uint32_t)(g * PX + q);
            base += (uint32_t)__popcll(m[q]);
        }
    }
}

__global__ void __launch_bounds__(64) k_masked_blur_list(ImageSet imgs, ImageSet seeds, ImageSet outs, int W, int H, BlurKernel K,
                                                         uint32_t key_rgb, const uint32_t* __restrict__ list, const uint32_t* __restrict__ row_count)
{
    const int y = blockIdx.x, im = blockIdx.y;
    const size_t row = (size_t)im * H + y;
    const uint32_t n = row_count[row];
    if (n == 0u) return;
    const BlurSrc b{imgs.image(im), nullptr, imgs.pitch, 0, false};          // (the scan pass has merged the seed's black pixels into the work image)
    uint8_t* orow = outs.image(im) + (size_t)y * outs.pitch;
    for (uint32_t k = threadIdx.x; k < n; k += 64) {
        const int x = (int)list[row * (size_t)W + k];
        store_px_bytes(orow, x, masked_blur_pixel(b, x, y, W, H, K));
    }
}

size_t telea_counter_words(int max_rounds) { return (2 + (size_t)kNcStride) * ((size_t)max_rounds + 2); }

static TeleaArgs telea_args(const TeleaWorkspace& ws, int n, int W, int H, uint32_t key_rgb)
{
    return TeleaArgs{ws.stamp, ws.T, ws.img, ws.need, ws.nlist, ws.counts, ws.offs, ws.ncounts, ws.remaining, ws.last_round, W, H, n, key_rgb};
}

// Per-call part: reset the counters, copy the seeds into the work image, pass A (levels by distance transform, level
// lists by counting sort).  h_levels (pinned host word) receives the deepest level any image needs -- the call waits for
// it, once per pass, so that passes B and C can be launched for exactly the levels that exist.
hipError_t launch_telea_init(const ImageSet& seed, const TeleaWorkspace& ws, int n, int W, int H, int max_rounds, uint32_t key_rgb,
                             uint32_t* h_levels, hipStream_t s)
{
    const TeleaArgs a = telea_args(ws, n, W, H, key_rgb);
    hipError_t e = hipMemsetAsync(ws.remaining, 0, (size_t)kTeleaMaxImages * sizeof(uint32_t), s);
    if (e != hipSuccess) return e;
    if ((e = hipMemsetAsync(ws.last_round, 0, (size_t)kTeleaMaxImages * sizeof(uint32_t), s)) != hipSuccess) return e;
    e = hipMemsetAsync(ws.counts, 0, (2 + (size_t)kNcStride) * ((size_t)max_rounds + 2) * sizeof(uint32_t), s);      // counts, offs and ncounts (adjacent)
    if (e != hipSuccess) return e;
    if (W % 4 == 0 && (((uintptr_t)seed.base | seed.pitch | seed.stride | (size_t)seed.eye_offset) & 3) == 0)
        hipLaunchKernelGGL(k_telea_init<4>, dim3((W / 4 + 127) / 128, H, n), dim3(128), 0, s, seed, a);
    else
        hipLaunchKernelGGL(k_telea_init<1>, dim3((W + 127) / 128, H, n), dim3(128), 0, s, seed, a);
    if (W % 8 == 0 && W <= 2048) hipLaunchKernelGGL(k_telea_dt_rows_vec<1>, dim3(H, n), dim3(256), 0, s, ws.stamp, W, H);
    else if (W % 8 == 0 && W <= 4096) hipLaunchKernelGGL(k_telea_dt_rows_vec<2>, dim3(H, n), dim3(256), 0, s, ws.stamp, W, H);
    else hipLaunchKernelGGL(k_telea_dt_rows, dim3(H, n), dim3(256), 0, s, ws.stamp, W, H);
    if (H <= 16 * 68) hipLaunchKernelGGL(k_telea_dt_cols_reg<68>, dim3((W + 63) / 64, n), dim3(1024), 0, s, a, (uint32_t)max_rounds);
    else hipLaunchKernelGGL(k_telea_dt_cols, dim3((W + 63) / 64, n), dim3(1024), 0, s, a, (uint32_t)max_rounds);
    hipLaunchKernelGGL(k_telea_rmax, dim3(1), dim3(1), 0, s, a);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    int R = max_rounds;
    if (h_levels) {       // (NULL: the asynchronous form -- every level up to max_rounds gets its launches; the ones that do not exist have empty lists)
        if ((e = hipMemcpyAsync(h_levels, ws.counts, sizeof(uint32_t), hipMemcpyDeviceToHost, s)) != hipSuccess) return e;
        if ((e = hipStreamSynchronize(s)) != hipSuccess) return e;
        R = (int)*h_levels;
        if (R == 0) return hipSuccess;
    }
    if ((e = hipMemsetAsync(ws.counts, 0, sizeof(uint32_t), s)) != hipSuccess) return e;         // counts[0] carried R; level 0 is empty
    const dim3 grid_s((unsigned)(((W + kSortTile - 1) / kSortTile) * ((H + kSortTile - 1) / kSortTile)), n);
    hipLaunchKernelGGL(k_telea_scan, dim3(1), dim3(1024), 0, s, a, R);
    hipLaunchKernelGGL(k_telea_sort, grid_s, dim3(256), 0, s, a);
    return hipGetLastError();
}

// Passes B and C: one launch per existing level each (a captured HIP graph replays them no faster: the ~4 us between
// dependent kernels is the device's, not the host's; one cooperative launch with grid-wide barriers is 3 x slower).
hipError_t launch_telea_rounds(const TeleaWorkspace& ws, int W, int H, int levels, uint32_t key_rgb, hipStream_t s)
{
    const TeleaArgs a = telea_args(ws, kTeleaMaxImages, W, H, key_rgb);
    // both passes wait on memory, not on arithmetic (PMC: `need` spends 90 % of its wave cycles waiting): a grid large enough
    // for one entry per thread takes 7.1 -> 5.8 ms off a 32-image pass compared with 512 workgroups looping
    int nb = 2048;
    if (const char* e = tuning_env(TUNE_TELEA_BLOCKS)) { const int v = atoi(e); if (v > 0) nb = (v + 7) & ~7; }      // tuning hook (a multiple of 8: XCDs)
    const dim3 grid(nb), block(256);
    for (int r = levels; r >= 2; --r) hipLaunchKernelGGL(k_telea_need, grid, block, 0, s, a, (uint32_t)r);
    for (int r = 1; r <= levels; ++r) hipLaunchKernelGGL(k_telea_fill, dim3(4 * nb), block, 0, s, a, (uint32_t)r);
    if (tuning_env(TUNE_TELEA_DUMP)) {         // tuning hook: level sizes / needed pixels of this pass on stderr
        std::vector<uint32_t> c(levels + 2), nc((size_t)(levels + 2) * kNcStride);
        hipError_t e = hipStreamSynchronize(s);
        if (e == hipSuccess) e = hipMemcpy(c.data(), ws.counts, c.size() * 4, hipMemcpyDeviceToHost);
        if (e == hipSuccess) e = hipMemcpy(nc.data(), ws.ncounts, nc.size() * 4, hipMemcpyDeviceToHost);
        if (e != hipSuccess) return e;
        for (int r = 1; r <= levels; ++r) fprintf(stderr, "level %d count %u need %u\n", r, c[r], nc[(size_t)r * kNcStride]);
    }
    return hipGetLastError();
}

hipError_t launch_masked_blur(const ImageSet& img, const ImageSet* seed, const ImageSet& out, int n, int W, int H,
                              const BlurKernel& K, uint32_t key_rgb, hipStream_t s, uint32_t* list, uint32_t* count)
{
    const dim3 grid((W + 255) / 256, H, n), block(256);
    const ImageSet none{nullptr, 0, 0, 0, 1};
    if (list && count && tuning_env(TUNE_BLUR_ONE_PASS) == nullptr) {          // list: n * W * H entries, count: n * H row counters
        hipError_t e = hipMemsetAsync(count, 0, (size_t)n * H * sizeof(uint32_t), s);
        if (e != hipSuccess) return e;
        auto dwords = [](const ImageSet& i) { return !i.base || (((uintptr_t)i.base | i.pitch | i.stride | (size_t)i.eye_offset) & 3) == 0; };
        if (W % 4 == 0 && dwords(img) && dwords(out) && (!seed || dwords(*seed)))
            hipLaunchKernelGGL(k_masked_blur_scan<4>, dim3((W / 4 + 127) / 128, H, n), dim3(128), 0, s, img, seed ? *seed : none, out, W, H, key_rgb, list, count);
        else
            hipLaunchKernelGGL(k_masked_blur_scan<1>, dim3((W + 127) / 128, H, n), dim3(128), 0, s, img, seed ? *seed : none, out, W, H, key_rgb, list, count);
        hipLaunchKernelGGL(k_masked_blur_list, dim3(H, n), dim3(64), 0, s, img, seed ? *seed : none, out, W, H, K, key_rgb, list, count);
        return hipGetLastError();
    }
    hipLaunchKernelGGL(k_masked_blur, grid, block, 0, s, img, seed ? *seed : none, out, W, H, K, key_rgb);
    return hipGetLastError();
}

}  // namespace mdvt
