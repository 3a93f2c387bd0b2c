// mdvt_points_edge_rows.hip -- the row kernels of a pure-shift POINTS render and the edge-point pass that follows a pure-shift row
// render of either mode: k_points_rows and k_points_rows_fast (one workgroup per (frame, row), z-buffer in LDS) with the hole-mask
// compaction (k_pack_mask), the count reductions and k_divcheck, then k_edge_rows_exact / k_edge_rows_pure.  Each launcher sits
// below its kernel; launch_render (mdvt_render_dispatch.hip) calls the ones declared in mdvt_grid_decls.h.
//
// Replaces, for such frames, decode (dfh:63-75, 13-24) -> master scale (sr:541) -> unproject (dmt:1112-1133) -> eye transform
// (sr:724-725, 832-836) -> z-buffered render (dmt:1422-1572) -> colour-key hole mask (sr:740, 793) -> edge-point splat (sr:745-814).
//
// The two families share this unit because their device code depends on it: the seed-image helpers of mdvt_device.h (seed_pixel,
// edge_normal_colour, removed_vertex_normal) take `of_by_one`, 0 from the points kernels and 1 from the mesh ones, and the points
// rows compiled without a caller of the other kind come out with another instruction schedule (DESIGN.md "Open" item 5;
// profiles/r11_raster_units.md).  k_edge_rows_exact<true> and k_edge_rows_pure are such callers.
//
// Compiled with -ffp-contract=off: see the arithmetic decree in mdvt_device.h / DESIGN.md.
#include "mdvt_device.h"
#include <type_traits>

#include <stdlib.h>

namespace mdvt {
namespace MDVT_GRID {      // one copy per sub-pixel grid (mdvt_internal.h)
// =================================================================================================
// POINT MODE, pure stereo shift: one workgroup per (frame,row), z-buffer in LDS
// =================================================================================================
//
// Row locality: with K == Krender, no pose and no toe-in, v = i exactly and u = j +- dl/Z, so an
// output row depends on one input row.  Z is strictly monotone in the 16-bit depth code, so the
// whole fragment fits one 64-bit LDS word
//        key = code16 << 40 | j << 24 | R | G<<8 | B<<16
// whose unsigned minimum is "nearest Z, ties to the lower source column" -- and it carries the
// colour, so the resolve phase is a plain LDS read (no gather, no second pass over the inputs).
// HBM traffic = algorithmic bytes: 6 B/px in, 8 B/px out (+8 B/px with the optional depth planes).

// FLAGS bit 0: optional depth planes, bit 1: `unused` vertices are not drawn (remove_edges),
// bit 2: edge points splatted into holes.
// `need`: bit 2 q + eye set for the edge points whose column the f32 estimate cannot decide (inside the guard band): the caller
// runs the reference's chain for those in ONE loop behind its unrolled ones (points_edge_chain) -- inlined at each of the 32
// (group, pixel, eye) sites the chain made the edge variants 9 600 instructions, 77 KB, more than the instruction cache.
template <int PX, int FLAGS>
__device__ __forceinline__ uint32_t points_splat_group(int g, const uint32_t (&dpx)[PX], const uint32_t (&cpx)[PX],
                                                       const uint32_t (&un)[PX], u64* zb, uint32_t* eb, int W,
                                                       float mult, float scale, float dl, const FrameDev& fp, bool edge_on, float guard)
{
    uint32_t need = 0;
    constexpr bool UNUSED = FLAGS & 2, EDGE = FLAGS & 4;
#pragma unroll
    for (int q = 0; q < PX; ++q) {
        const int j = g * PX + q;
        const uint32_t code = code16_of(dpx[q]);
        const float z = decode_z(code, mult, scale);
        if (!(z > kNear)) continue;
        const float d = dl / z;
        const float fj = (float)j;
        if (!(UNUSED && un[q])) {
            const u64 key = ((u64)code << 40) | ((u64)(uint32_t)j << 24) | (u64)cpx[q];
            const int xL = point_col_row_kernel(fj + d), xR = point_col_row_kernel(fj - d);        // (the row: point_row(f32(i)) == i)
            if ((uint32_t)xL < (uint32_t)W) atomicMin(&zb[xL], key);
            if ((uint32_t)xR < (uint32_t)W) atomicMin(&zb[W + xR], key);
        } else if (EDGE && edge_on) {
            // sr:599-600, 746: the column the reference's f64 chain rounds to (mdvt_device.h "edge points")
            const uint32_t ekey = (code << 16) | (uint32_t)j;
            const int xL = edge_col_estimate(fp, 0, fj, d, W, guard), xR = edge_col_estimate(fp, 1, fj, d, W, guard);
            if (xL >= 0) atomicMin(&eb[xL], ekey);
            if (xR >= 0) atomicMin(&eb[W + xR], ekey);
            need |= (xL == -2 ? 1u : 0u) << (2 * q) | (xR == -2 ? 2u : 0u) << (2 * q);
        }
    }
    return need;
}

// the edge points points_splat_group left undecided: bit (it * PX + q) * 2 + eye of `need`, group of iteration `it` = g0 + it * gstep
template <int PX, int NIT>
__device__ __forceinline__ void points_edge_chain(uint32_t need, int g0, int gstep, const uint32_t (&dpx)[NIT][PX], uint32_t* eb, int W,
                                                  float mult, float scale, const FrameDev& fp)
{
#pragma unroll 1
    while (need) {
        const int b = __ffs((int)need) - 1, eye = b & 1, q = (b >> 1) % PX, it = (b >> 1) / PX;
        need &= need - 1u;
        uint32_t px = dpx[0][0];
#pragma unroll
        for (int k = 0; k < NIT; ++k)
#pragma unroll
            for (int r = 0; r < PX; ++r)
                if (k == it && r == q) px = dpx[k][r];
        const int j = (g0 + it * gstep) * PX + q;
        const uint32_t code = code16_of(px);
        const int x = edge_col_chain(fp, eye, (float)j, decode_z(code, mult, scale), W);
        if (x >= 0 && x < W) atomicMin(&eb[eye * W + x], (code << 16) | (uint32_t)j);
    }
}

// TPB threads; ITERS > 0: every thread owns exactly ITERS groups (ngroups <= TPB*ITERS) whose HBM
// loads are all issued before the LDS clear, so 2*ITERS 768-byte wave loads are in flight per wave
// while the z-buffer is initialised.  ITERS == 0: plain strided loop (any W).
template <int PX, int FLAGS, int TPB, int ITERS>
__global__ void __launch_bounds__(TPB, ((FLAGS & 5) == 4) ? 6 : 1) k_points_rows(RenderArgs a)
{
    constexpr bool ZOUT = FLAGS & 1, UNUSED = FLAGS & 2, EDGE = FLAGS & 4, SEED = FLAGS & 8;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int W = a.W;
    u64* zb = (u64*)smem;                        // [2][W] main z keys, left then right eye
    uint32_t* eb = (uint32_t*)(zb + 2 * (size_t)W);   // [2][W] edge-point keys (code16<<16 | j), EDGE only

    const int fr = blockIdx.x / a.H;
    const int i = blockIdx.x - fr * a.H;
    const int f = a.frame0 + fr;
    const FrameDev& fp = a.fp[f];
    const float mult = fp.mult, scale = fp.scale, dl = fp.dl;
    const int tid = threadIdx.x;
    const int ngroups = W / PX;

    const uint8_t* drow = a.depth + (size_t)f * a.depth_stride + (size_t)i * a.depth_pitch;
    const uint8_t* crow = a.color + (size_t)f * a.color_stride + (size_t)i * a.color_pitch;
    const uint8_t* urow = UNUSED ? a.unused + (size_t)fr * a.ws_stride_px + (size_t)i * W : nullptr;
    // (the edge points of scanlines erow_lo .. erow_hi are k_edge_rows_exact's: their row is not the source row)
    const bool edge_on = EDGE && !edge_row_deferred(fp, i);
    const float guard = edge_col_guard(W);

    constexpr int NIT = ITERS > 0 ? ITERS : 1;
    uint32_t dpx[NIT][PX], cpx[NIT][PX], un[NIT][PX];
    if (ITERS > 0) {
#pragma unroll
        for (int it = 0; it < NIT; ++it) {
            const int g = tid + it * TPB;
            if (g < ngroups) {
                RowIO<PX>::load_nt(drow, g, dpx[it]);
                RowIO<PX>::load_nt(crow, g, cpx[it]);
                if (UNUSED) RowIO<PX>::load_u8(urow, g, un[it]);
            }
        }
    }

    // clear the z-buffers (16 B per store where the layout allows)
    {
        uint4* z4 = (uint4*)zb;
        const int n4 = W;                        // 2*W u64 = W uint4
        for (int x = tid; x < n4; x += TPB) z4[x] = make_uint4(~0u, ~0u, ~0u, ~0u);
        if (EDGE) for (int x = tid; x < 2 * W; x += TPB) eb[x] = kEmpty32;
    }
    __syncthreads();

    if (ITERS > 0) {
        uint32_t need = 0;
#pragma unroll
        for (int it = 0; it < NIT; ++it) {
            const int g = tid + it * TPB;
            if (g < ngroups)
                need |= points_splat_group<PX, FLAGS>(g, dpx[it], cpx[it], un[it], zb, eb, W, mult, scale, dl, fp, edge_on, guard) << (2 * PX * it);
        }
        if (EDGE) points_edge_chain<PX, NIT>(need, tid, TPB, dpx, eb, W, mult, scale, fp);
    } else {
        for (int g = tid; g < ngroups; g += TPB) {
            RowIO<PX>::load_nt(drow, g, dpx[0]);
            RowIO<PX>::load_nt(crow, g, cpx[0]);
            if (UNUSED) RowIO<PX>::load_u8(urow, g, un[0]);
            const uint32_t need = points_splat_group<PX, FLAGS>(g, dpx[0], cpx[0], un[0], zb, eb, W, mult, scale, dl, fp, edge_on, guard);
            if (EDGE) points_edge_chain<PX, NIT>(need, g, 0, dpx, eb, W, mult, scale, fp);
        }
    }
    __syncthreads();

#pragma unroll
    for (int eye = 0; eye < 2; ++eye) {
        uint8_t* orow = a.rgb[eye] + (size_t)f * a.rgb_stride + (size_t)i * a.rgb_pitch;
        uint8_t* mrow = a.mask[eye] + (size_t)f * a.mask_stride + (size_t)i * a.mask_pitch;
        float* zrow = ZOUT && a.zout[eye]
                          ? (float*)((uint8_t*)a.zout[eye] + (size_t)f * a.zout_stride + (size_t)i * a.zout_pitch)
                          : nullptr;
        const u64* zrow_lds = zb + (size_t)eye * W;
        for (int g = tid; g < ngroups; g += TPB) {
            uint32_t opx[PX], om[PX], spx[PX], eseed = 0;
            float oz[PX];
#pragma unroll
            for (int q = 0; q < PX; ++q) {
                const int x = g * PX + q;
                const u64 key = zrow_lds[x];
                const uint32_t rgb = (uint32_t)key & 0xFFFFFFu;
                const bool covered = key != kEmpty64;
                const bool hole = !covered || rgb == a.key_rgb;       // sr:740 colour-key compare
                uint32_t out = hole ? 0u : rgb;                       // sr:793
                if (EDGE && hole && edge_on) {
                    const uint32_t ek = eb[(size_t)eye * W + x];
                    if (ek != kEmpty32 && a.edge_paint) {
                        // colour of source column (ek & 0xFFFF) of this row (sr:813-814)
                        out = load_px_bytes(crow, (int)(ek & 0xFFFFu));
                    }
                }
                opx[q] = out;
                om[q] = hole ? 255u : 0u;
                if (ZOUT) oz[q] = covered ? decode_z((uint32_t)(key >> 40), mult, scale) : 0.0f;
                if (SEED && a.seed[eye]) {
                    spx[q] = seed_pixel(a, fp, f, eye, x, i, hole, ~0u, 0);
                    if (EDGE && hole && edge_on) { const uint32_t ek = eb[(size_t)eye * W + x]; if (ek != kEmpty32) eseed |= 1u << q; }
                }
            }
            if (SEED && EDGE) {
                // the pixels whose seed colour is an edge point's normal (f64, a few hundred instructions): one copy of that code
#pragma unroll 1
                while (eseed) {
                    const int q = __ffs((int)eseed) - 1;
                    eseed &= eseed - 1u;
                    const uint32_t c = edge_normal_colour(a, fp, f, eye, i, (int)(eb[(size_t)eye * W + g * PX + q] & 0xFFFFu), 0);
#pragma unroll
                    for (int k = 0; k < PX; ++k) if (k == q) spx[k] = c;
                }
            }
            RowIO<PX>::store_rgb(orow, g, opx);
            RowIO<PX>::store_mask(mrow, g, om);
            if (ZOUT && zrow) RowIO<PX>::store_z(zrow, g, oz);
            if (SEED && a.seed[eye]) RowIO<PX>::store_rgb(a.seed[eye] + (size_t)f * a.seed_stride + (size_t)i * a.seed_pitch, g, spx);
        }
    }
}

template <int PX, int TPB, int ITERS>
static hipError_t launch_points_rows_cfg(const RenderPlan& plan, const RenderArgs& a, hipStream_t s)
{
    const size_t lds = render_lds_bytes(plan, a.W);
    const dim3 grid((unsigned)(plan.n * a.H)), block(TPB);
    const bool zout = a.zout[0] || a.zout[1];
    const int flags = (zout ? 1 : 0) | (plan.remove_edges ? 2 : 0) | (plan.remove_edges && plan.edge_points ? 4 : 0) |
                      (plan.remove_edges && a.seed[0] ? 8 : 0);
#define MDVT_CASE(F)                                                                                   \
    case F:                                                                                            \
        if (lds > 48 * 1024)                                                                           \
            (void)hipFuncSetAttribute((const void*)k_points_rows<PX, F, TPB, ITERS>,                   \
                                      hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);           \
        hipLaunchKernelGGL((k_points_rows<PX, F, TPB, ITERS>), grid, block, lds, s, a);                \
        break;
    switch (flags) {
        MDVT_CASE(0) MDVT_CASE(1) MDVT_CASE(2) MDVT_CASE(3) MDVT_CASE(6) MDVT_CASE(7)
        MDVT_CASE(10) MDVT_CASE(11) MDVT_CASE(14) MDVT_CASE(15)
        default: return hipErrorInvalidValue;
    }
#undef MDVT_CASE
    return hipGetLastError();
}

// Wavefront hole-mask compaction.  Each lane holds the hole flags of 4 consecutive pixels (nib, LSB = lowest
// x; lane & 7 == g & 7).  Eight lanes' nibbles are OR-combined into one dword of the packed 1-bit/px mask with three DPP
// operands on the VALU (two quad permutes and a row shift: no LDS round trip -- __shfl_xor compiles to ds_bpermute_b32 here,
// three of them per eye behind the row's 8-byte LDS atomics were most of what the fused variant cost in r05); the hole count
// of the wave is the popcount of four 64-lane ballots (scalar unit).  The dword is valid in the lanes with g & 7 == 0.
template <int CTRL>
__device__ __forceinline__ uint32_t or_dpp(uint32_t v)
{
    return v | (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, 0xF, 0xF, true);
}

__device__ __forceinline__ uint32_t mask_dword_of_8_lanes(uint32_t nib, int g)
{
    uint32_t v = nib << (4 * (g & 7));
    v = or_dpp<0xB1>(v);          // quad_perm [1,0,3,2]: lane ^ 1
    v = or_dpp<0x4E>(v);          // quad_perm [2,3,0,1]: lane ^ 2
    return or_dpp<0x104>(v);      // row_shl:4: lane i takes lane i + 4 (of its row of 16)
}

__device__ __forceinline__ int wave_hole_count(uint32_t nib)
{
    return __popcll(__ballot(nib & 1)) + __popcll(__ballot(nib & 2)) + __popcll(__ballot(nib & 4)) + __popcll(__ballot(nib & 8));
}

__device__ __forceinline__ int compact_hole_nibble(uint32_t nib, int g, bool act, uint8_t* bits_row, bool want_count)
{
    if (bits_row) {
        const uint32_t v = mask_dword_of_8_lanes(nib, g);
        if (act && (g & 7) == 0) ((uint32_t*)bits_row)[g >> 3] = v;
    }
    return want_count ? wave_hole_count(nib) : 0;
}

// The fused points kernel's hole counts: every WAVE stores its two counts as one dword (left | right << 16: at most 256 each) to
// wave_counts[(frame * H + row) * waves + wave] -- a plain fire-and-forget store, no LDS total, no barrier, no atomic -- and
// k_reduce_wave_counts adds them up per frame.  r06 measured the alternatives on 128 frames of 1080p (595 us without counts):
// LDS totals + barrier + row store + reduce launch 664; LDS totals without a barrier + one RETURNING atomic per workgroup into
// per-frame accumulators that the last arrival finishes (no second launch) 664 -> 639 without the atomics; fire-and-forget atomics per
// wave with the frame's last workgroup waiting for the arrivals: dropped -- its wait has to read with read-modify-write atomics (a
// load may be served from the XCD's own L2, which is not coherent with the other XCDs' atomics within a kernel: the first version hung
// at 1080p on stale values) and with 128 frames in flight the waiting workgroups' polling stalled the launch.
// wave_counts[(frame * H + row) * waves + wave], waves = threads per workgroup / 64: a frame's counts are H * waves consecutive dwords
__global__ void __launch_bounds__(256) k_reduce_wave_counts(const uint32_t* __restrict__ wave_counts, uint32_t* __restrict__ hole_counts,
                                                            int H, int waves, int frame0)
{
    __shared__ uint32_t part[2][4];
    const int fr = blockIdx.x;
    const int n = H * waves;                                       // (a multiple of 4: waves is 4, 8 or 16)
    const uint4* src = reinterpret_cast<const uint4*>(wave_counts + (size_t)fr * n);
    uint32_t l = 0, r = 0;
    for (int k = threadIdx.x; k < n / 4; k += 256) {
        const uint4 v = src[k];
        l += (v.x & 0xFFFFu) + (v.y & 0xFFFFu) + (v.z & 0xFFFFu) + (v.w & 0xFFFFu);
        r += (v.x >> 16) + (v.y >> 16) + (v.z >> 16) + (v.w >> 16);
    }
    for (int off = 32; off > 0; off >>= 1) { l += __shfl_down((int)l, off); r += __shfl_down((int)r, off); }
    if ((threadIdx.x & 63) == 0) { part[0][threadIdx.x >> 6] = l; part[1][threadIdx.x >> 6] = r; }
    __syncthreads();
    if (threadIdx.x < 2) hole_counts[2 * (size_t)(frame0 + fr) + threadIdx.x] = part[threadIdx.x][0] + part[threadIdx.x][1] + part[threadIdx.x][2] + part[threadIdx.x][3];
}

// row_counts[(2*frame + eye)*H + row] -> hole_counts[2*frame + eye]
__global__ void __launch_bounds__(256) k_reduce_counts(const uint32_t* __restrict__ row_counts, uint32_t* __restrict__ hole_counts,
                                                       int H, int frame0)
{
    __shared__ uint32_t part[4];
    const int fe = blockIdx.x;                       // 2*fr + eye within this launch
    uint32_t c = 0;
    for (int i = threadIdx.x; i < H; i += 256) c += row_counts[(size_t)fe * H + i];
    for (int off = 32; off > 0; off >>= 1) c += __shfl_down((int)c, off);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) hole_counts[2 * (size_t)frame0 + fe] = part[0] + part[1] + part[2] + part[3];
}

// Post-pass for the kernels that do not compact in place: byte mask -> packed bits + per-row counts.
// One workgroup per (row, frame, eye).
__global__ void __launch_bounds__(256) k_pack_mask(RenderArgs a)
{
    __shared__ uint32_t wcount[4];
    const int W = a.W;
    const int ngroups = (W + 3) / 4;
    const int i = blockIdx.x;
    const int fr = blockIdx.y >> 1, eye = blockIdx.y & 1;
    const int f = a.frame0 + fr;
    const uint8_t* mrow = a.mask[eye] + (size_t)f * a.mask_stride + (size_t)i * a.mask_pitch;
    uint8_t* brow = a.maskbits[eye] ? a.maskbits[eye] + (size_t)f * a.maskbits_stride + (size_t)i * a.maskbits_pitch : nullptr;
    int cnt = 0;
    for (int g0 = 0; g0 < ngroups; g0 += 256) {
        const int g = g0 + threadIdx.x;
        const bool act = g < ngroups;
        uint32_t nib = 0;
        if (act)
            for (int q = 0; q < 4; ++q) if (4 * g + q < W && mrow[4 * g + q]) nib |= 1u << q;
        cnt += compact_hole_nibble(nib, g, act, brow, a.hole_counts != nullptr);
    }
    if (a.hole_counts) {
        if ((threadIdx.x & 63) == 0) wcount[threadIdx.x >> 6] = (uint32_t)cnt;
        __syncthreads();
        if (threadIdx.x == 0) a.row_counts[(2 * (size_t)fr + eye) * a.H + i] = wcount[0] + wcount[1] + wcount[2] + wcount[3];
    }
}

hipError_t launch_pack_mask(const RenderArgs& a, int n, hipStream_t s)
{
    dim3 grid(a.H, n * 2);
    hipLaunchKernelGGL(k_pack_mask, grid, dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_reduce_counts(const RenderArgs& a, int n, hipStream_t s)
{
    hipLaunchKernelGGL(k_reduce_counts, dim3(2 * n), dim3(256), 0, s, a.row_counts, a.hole_counts, a.H, a.frame0);
    return hipGetLastError();
}

// The headline kernel's division, proven per parameter set.  d = dl / z is IEEE-correctly rounded by decree, and hipcc's expansion of it
// is 10 VALU instructions of the ~220 a lane spends on its four pixels -- with the kernel at ~80 % of the VALU issue rate next to
// ~78 % of HBM peak (r06: every instruction added to it shows up in its time).  But a frame's z has only 65535 values:
// z = (f32(code << 16) * mult) * scale.  points_div_short is v_rcp_f32, one multiply and two fma -- Markstein's correction step from the
// raw reciprocal, faithful in general and correctly rounded unless the quotient sits within ~2^-23 ulp of a rounding boundary --
// and k_divcheck compares it with the IEEE division for every code of one (mult, scale, dl): a counter of 0 is a proof for that frame's
// operands, anything else leaves the frame on the expansion.  (tools/probe/div_probe.hip: 0 mismatches in 336 parameter sets.)
__device__ __forceinline__ float points_div_short(float dl, float z)
{
    const float y = __builtin_amdgcn_rcpf(z);
    const float q = dl * y;
    return __builtin_fmaf(__builtin_fmaf(-z, q, dl), y, q);
}

__global__ void __launch_bounds__(256) k_divcheck(float mult, float scale, float dl, uint32_t* __restrict__ bad)
{
    const uint32_t code = blockIdx.x * 256u + threadIdx.x;           // 0 .. 65535
    const float z = ((float)(code << 16) * mult) * scale;
    bool differs = false;
    if (z > kNear) differs = __float_as_uint(points_div_short(dl, z)) != __float_as_uint(dl / z);
    if (__ballot(differs) && (threadIdx.x & 63) == 0) atomicAdd(bad, (uint32_t)__popcll(__ballot(differs)));
}

hipError_t launch_divcheck(float mult, float scale, float dl, uint32_t* bad, hipStream_t s)
{
    hipLaunchKernelGGL(k_divcheck, dim3(256), dim3(256), 0, s, mult, scale, dl, bad);
    return hipGetLastError();
}

// -------------------------------------------------------------------------------------------------
// Hand-scheduled variant of the row kernel for the headline case (4 px/lane, one group per thread, no
// edge filter): byte shuffles are single v_perm_b32 ops, out-of-range fragments are steered to a trash
// LDS word instead of branching (no exec-mask traffic).  Same arithmetic, same results as k_points_rows.
// -------------------------------------------------------------------------------------------------
// BITS: 0 = byte mask only (the headline); 1 = packed mask and / or hole counts, whichever of the optional buffers are there (run-time
// tests; the wave counts its holes by ballots); 8 | mask | 2 pack | 4 count = the same with the set of outputs fixed at compile time
// (r06: the generic form ran the CU's scalar unit at ~70 % -- null tests, branches and exec masks around the optional stores: 267 SALU
// instructions per wave against the headline's 161; counting from the packed mask in a kernel afterwards instead of by ballots here
// was measured too: 37 us per 128 frames against 6).
template <int TPB, bool ZOUT, int BITS, int NT = 3>
__global__ void __launch_bounds__(TPB) k_points_rows_fast(RenderArgs a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int W = a.W, W4 = W >> 2;
    u64* zb = (u64*)smem;                        // [2W] keys (left, right) + [1] trash word
    const int fr = blockIdx.x / a.H;
    const int i = blockIdx.x - fr * a.H;
    const int f = a.frame0 + fr;
    const FrameDev& fp = a.fp[f];
    const float mult = fp.mult, scale = fp.scale, dl = fp.dl;
    const int g = threadIdx.x;
    const bool act = g < W4;

    uint32_t d0 = 0, d1 = 0, d2 = 0, c0 = 0, c1 = 0, c2 = 0;
    if (act) {
        const uint32_t* dp = (const uint32_t*)(a.depth + (size_t)f * a.depth_stride + (size_t)i * a.depth_pitch) + 3 * g;
        const uint32_t* cp = (const uint32_t*)(a.color + (size_t)f * a.color_stride + (size_t)i * a.color_pitch) + 3 * g;
        if (NT & 1) {                              // every input byte is read exactly once: non-temporal (161 -> 148 us per 32 frames with both)
            d0 = __builtin_nontemporal_load(dp); d1 = __builtin_nontemporal_load(dp + 1); d2 = __builtin_nontemporal_load(dp + 2);
            c0 = __builtin_nontemporal_load(cp); c1 = __builtin_nontemporal_load(cp + 1); c2 = __builtin_nontemporal_load(cp + 2);
        } else {
            d0 = dp[0]; d1 = dp[1]; d2 = dp[2];
            c0 = cp[0]; c1 = cp[1]; c2 = cp[2];
        }
    }
    {
        uint4* z4 = (uint4*)zb;
        for (int x = g; x < W; x += TPB) z4[x] = make_uint4(~0u, ~0u, ~0u, ~0u);
    }
    __syncthreads();

    if (act) {
        // R<<24 | B<<16 of each pixel (dfh:67-69): one byte permute each
        uint32_t c32[4], cpx[4];
        c32[0] = __builtin_amdgcn_perm(d0, d0, 0x00020c0cu);
        c32[1] = __builtin_amdgcn_perm(d1, d0, 0x03050c0cu);
        c32[2] = __builtin_amdgcn_perm(d2, d1, 0x02040c0cu);
        c32[3] = __builtin_amdgcn_perm(d2, d2, 0x01030c0cu);
        cpx[0] = c0 & 0xFFFFFFu;
        cpx[1] = __builtin_amdgcn_perm(c1, c0, 0x0c050403u);
        cpx[2] = __builtin_amdgcn_perm(c2, c1, 0x0c040302u);
        cpx[3] = c2 >> 8;
        const float fj0 = (float)(g << 2);
        const uint32_t jhi = (uint32_t)g >> 6, jlo = ((uint32_t)g << 2) & 0xFFu;
        const int trash = 2 * W;
        auto splat = [&](auto short_div) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const float z = ((float)c32[q] * mult) * scale;
                const bool ok = z > kNear;
                const float d = decltype(short_div)::value ? points_div_short(dl, z) : dl / z;
                const float fj = fj0 + (float)q;
                const int xL = point_col_row_kernel(fj + d), xR = point_col_row_kernel(fj - d);
                const bool okL = ok && (uint32_t)xL < (uint32_t)W;
                const bool okR = ok && (uint32_t)xR < (uint32_t)W;
                const int sL = okL ? xL : trash;
                const int sR = okR ? W + xR : trash;
                const uint32_t hi = __builtin_amdgcn_perm(c32[q], jhi, 0x0c070600u);      // code16 << 8 | j >> 8
                const uint32_t lo = __builtin_amdgcn_perm(jlo + (uint32_t)q, cpx[q], 0x04020100u);   // (j & 255) << 24 | rgb
                const u64 key = ((u64)hi << 32) | lo;
                atomicMin(&zb[sL], key);
                atomicMin(&zb[sR], key);
            }
        };
        // (wave-uniform: the frame's parameter set has been proven, or it has not)
        if (fp.div_slot >= 0 && a.divcheck[fp.div_slot] == 0u && !(MDVT_DEBUG_SKIP(a) & 128)) splat(std::true_type{});      // (128: tuning build's A/B)
        else splat(std::false_type{});
    }
    __syncthreads();

    constexpr bool kSpec = (BITS & 8) != 0;
    const bool counting = kSpec ? (BITS & 4) != 0 : (BITS && a.hole_counts && !(MDVT_DEBUG_SKIP(a) & 32));
    uint32_t cnt[2] = {0u, 0u};
    if (act || BITS) {
#pragma unroll
        for (int eye = 0; eye < 2; ++eye) {
            uint4 k01 = make_uint4(0, 0, 0, 0), k23 = make_uint4(0, 0, 0, 0);
            if (act) {
                const uint4* zq = (const uint4*)(zb + (size_t)eye * W) + 2 * g;
                k01 = zq[0]; k23 = zq[1];
            }
            const uint32_t hi[4] = {k01.y, k01.w, k23.y, k23.w};
            const uint32_t lo[4] = {k01.x, k01.z, k23.x, k23.z};
            uint32_t o[4], mw = 0, nib = 0;
            float oz[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const bool covered = hi[q] != ~0u;                 // code16<<8 | j>>8 < 2^24 when covered
                const uint32_t rgb = lo[q] & 0xFFFFFFu;
                const bool hole = !covered || rgb == a.key_rgb;    // sr:740
                o[q] = hole ? 0u : rgb;                            // sr:793
                if (BITS) {
                    nib |= hole ? (1u << q) : 0u;
                    // the compare's lane mask IS the ballot: the wave's count costs scalar instructions only
                    if (counting && !(MDVT_DEBUG_SKIP(a) & 64)) cnt[eye] += (uint32_t)__popcll(__ballot(hole && act));
                } else {
                    mw |= hole ? (0xFFu << (8 * q)) : 0u;
                }
                if (ZOUT) oz[q] = covered ? decode_z(hi[q] >> 8, mult, scale) : 0.0f;
            }
            uint8_t* mbase = a.mask[eye];                          // (NULL with BITS: the caller takes the packed mask only)
            const bool has_mask = kSpec ? (BITS & 1) != 0 : (!BITS || mbase != nullptr);
            const bool has_pack = kSpec ? (BITS & 2) != 0 : (BITS && a.maskbits[eye] != nullptr && !(MDVT_DEBUG_SKIP(a) & 64));
            if (BITS && has_mask) {                                // nibble -> four bytes of 0 / 255
                const uint32_t b = __umul24(nib, 0x204081u) & 0x01010101u;
                mw = (b << 8) - b;
            }
            if (act) {
                uint32_t* op = (uint32_t*)(a.rgb[eye] + (size_t)f * a.rgb_stride + (size_t)i * a.rgb_pitch) + 3 * g;
                uint32_t* mp = (uint32_t*)(mbase + (size_t)f * a.mask_stride + (size_t)i * a.mask_pitch) + g;
                if (NT & 2) {                          // ... and every output byte written once
                    __builtin_nontemporal_store(__builtin_amdgcn_perm(o[1], o[0], 0x04020100u), op);
                    __builtin_nontemporal_store(__builtin_amdgcn_perm(o[2], o[1], 0x05040201u), op + 1);
                    __builtin_nontemporal_store(__builtin_amdgcn_perm(o[3], o[2], 0x06050402u), op + 2);
                    if (has_mask) __builtin_nontemporal_store(mw, mp);
                } else {
                op[0] = __builtin_amdgcn_perm(o[1], o[0], 0x04020100u);
                op[1] = __builtin_amdgcn_perm(o[2], o[1], 0x05040201u);
                op[2] = __builtin_amdgcn_perm(o[3], o[2], 0x06050402u);
                if (has_mask) *mp = mw;
                }
                if (ZOUT && a.zout[eye]) {
                    float4* zp = (float4*)((uint8_t*)a.zout[eye] + (size_t)f * a.zout_stride + (size_t)i * a.zout_pitch) + g;
                    typedef float f32x4 __attribute__((ext_vector_type(4)));
                    f32x4 v = {oz[0], oz[1], oz[2], oz[3]};
                    if (NT & 2) __builtin_nontemporal_store(v, (f32x4*)zp);
                    else *zp = make_float4(oz[0], oz[1], oz[2], oz[3]);
                }
            }
            if (BITS && has_pack) {
                if (!act) nib = 0u;
                const uint32_t v = mask_dword_of_8_lanes(nib, g);
                if (act && (g & 7) == 0 && !(MDVT_DEBUG_SKIP(a) & 8))
                    ((uint32_t*)(a.maskbits[eye] + (size_t)f * a.maskbits_stride + (size_t)i * a.maskbits_pitch))[g >> 3] = v;
            }
        }
    }
    if (counting && (g & 63) == 0)
        a.wave_counts[((size_t)fr * a.H + i) * (TPB / 64) + (g >> 6)] = cnt[0] | (cnt[1] << 16);
}

// Tuning override for experiments (tools/kbench.py): MDVT_POINTS_CFG = "<TPB>x<ITERS>" (e.g. 512x1) selects the
// templated kernel with that geometry instead of the defaults.  Re-read on every launch.
static int points_cfg_override()
{
    const char* e = tuning_env(TUNE_POINTS_CFG);
    int t = 0, it = 0;
    if (e && sscanf(e, "%dx%d", &t, &it) == 2) return t * 16 + it;
    return 0;
}

template <int TPB, bool ZOUT, int BITS>
static hipError_t launch_points_rows_fast_cfg(const RenderPlan& plan, const RenderArgs& a_in, hipStream_t s)
{
    RenderArgs a = a_in;
    if (const char* e = tuning_env(TUNE_DEBUG_SKIP)) a.debug_skip = atoi(e);      // (tuning build: the BITS tail's ablations, 8 / 16 / 32 / 64)
    const size_t lds = (2 * (size_t)a.W + 2) * sizeof(u64);
    const dim3 grid((unsigned)(plan.n * a.H)), block(TPB);
    if (lds > 48 * 1024)
        (void)hipFuncSetAttribute((const void*)k_points_rows_fast<TPB, ZOUT, BITS>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (!ZOUT && !BITS && lds <= 48 * 1024) {       // tuning hook (tools/kbench.py --env MDVT_POINTS_NT): 0 = temporal loads and stores
        const char* e = tuning_env(TUNE_POINTS_NT);
        if (e && *e) {
            const int nt = atoi(e);
            if (nt == 0) { hipLaunchKernelGGL((k_points_rows_fast<TPB, false, 0, 0>), grid, block, lds, s, a); return hipGetLastError(); }
            if (nt == 1) { hipLaunchKernelGGL((k_points_rows_fast<TPB, false, 0, 1>), grid, block, lds, s, a); return hipGetLastError(); }
            if (nt == 2) { hipLaunchKernelGGL((k_points_rows_fast<TPB, false, 0, 2>), grid, block, lds, s, a); return hipGetLastError(); }
        }
    }
    hipLaunchKernelGGL((k_points_rows_fast<TPB, ZOUT, BITS>), grid, block, lds, s, a);
    if (BITS && a.hole_counts && !(MDVT_DEBUG_SKIP(a) & 16)) {
        hipLaunchKernelGGL(k_reduce_wave_counts, dim3(plan.n), dim3(256), 0, s, a.wave_counts, a.hole_counts, a.H, TPB / 64, a.frame0);
    }
    return hipGetLastError();
}

template <int TPB>
static hipError_t launch_points_rows_fast(RenderPlan& plan, const RenderArgs& a, hipStream_t s)
{
    const bool zout = a.zout[0] || a.zout[1];
    const bool pack = a.maskbits[0] != nullptr, count = a.hole_counts != nullptr, mask = a.mask[0] != nullptr;
    const bool bits = pack || count;
    plan.fused_bits = bits;
    if (zout) return bits ? launch_points_rows_fast_cfg<TPB, true, 1>(plan, a, s) : launch_points_rows_fast_cfg<TPB, true, 0>(plan, a, s);
    if (!bits) return launch_points_rows_fast_cfg<TPB, false, 0>(plan, a, s);
    if (tuning_env(TUNE_DEBUG_SKIP)) return launch_points_rows_fast_cfg<TPB, false, 1>(plan, a, s);      // (the ablations live in the generic form)
    switch ((mask ? 1 : 0) | (pack ? 2 : 0) | (count ? 4 : 0)) {           // the set of outputs fixed at compile time
        case 2: return launch_points_rows_fast_cfg<TPB, false, 8 | 2>(plan, a, s);
        case 3: return launch_points_rows_fast_cfg<TPB, false, 8 | 3>(plan, a, s);
        case 6: return launch_points_rows_fast_cfg<TPB, false, 8 | 6>(plan, a, s);
        case 7: return launch_points_rows_fast_cfg<TPB, false, 8 | 7>(plan, a, s);
        case 5: return launch_points_rows_fast_cfg<TPB, false, 8 | 5>(plan, a, s);
        default: return launch_points_rows_fast_cfg<TPB, false, 1>(plan, a, s);
    }
}

// Will this launch be rendered by k_points_rows_fast with the mask compaction fused in (the one kernel that can leave the byte
// mask out)?  The same conditions as the dispatch below.
bool points_fused_bits_applies(const RenderPlan& plan, const RenderArgs& a)
{
    return plan.mode == MDVT_MODE_POINTS && !plan.general && plan.vec4 && !plan.remove_edges && points_cfg_override() == 0 &&
           a.W / 4 <= 1024 && (a.maskbits[0] || a.maskbits[1]);
}

hipError_t launch_points_rows_vec4(RenderPlan& plan, const RenderArgs& a, hipStream_t s)
{
    const int ngroups = a.W / 4;
    int cfg = points_cfg_override();
    if (cfg == 0 && !plan.remove_edges) {          // the headline kernel
        if (ngroups <= 256) return launch_points_rows_fast<256>(plan, a, s);
        if (ngroups <= 512) return launch_points_rows_fast<512>(plan, a, s);
        if (ngroups <= 1024) return launch_points_rows_fast<1024>(plan, a, s);
    }
    if (cfg == 0 || (cfg % 16 != 0 && (cfg / 16) * (cfg % 16) < ngroups)) {
        if (ngroups <= 256) cfg = 256 * 16 + 1;
        else if (ngroups <= 512) cfg = 512 * 16 + 1;        // 1080p: measured best (tools/kbench.py)
        else if (ngroups <= 1024) cfg = 512 * 16 + 2;
        else if (ngroups <= 2048) cfg = 1024 * 16 + 2;
        else cfg = 256 * 16 + 0;
    }
#define MDVT_CFG(T, I) case T * 16 + I: return launch_points_rows_cfg<4, T, I>(plan, a, s);
    switch (cfg) {
        MDVT_CFG(128, 4) MDVT_CFG(256, 1) MDVT_CFG(256, 2) MDVT_CFG(512, 1) MDVT_CFG(512, 2) MDVT_CFG(1024, 2)
        default: return launch_points_rows_cfg<4, 256, 0>(plan, a, s);
    }
#undef MDVT_CFG
}

// rows that are not dword-addressable: a pixel per lane, plain strided loop
hipError_t launch_points_rows_px1(const RenderPlan& plan, const RenderArgs& a, hipStream_t s)
{
    return launch_points_rows_cfg<1, 256, 0>(plan, a, s);
}

// =================================================================================================
// EDGE POINTS placed after a pure-shift row render (either mode)
// =================================================================================================

// Edge points of the scanlines the LDS row kernels leave out (pure-shift frames, scanlines erow_lo .. erow_hi of the frame's
// FrameDev): there the chain puts a point of source row i on row i or i + 1, so scanline y collects the vertices of removed
// triangles of source rows y - 1 and y whose chain row is y -- nearest first (depth code; then the lower source index) --
// and paints them where the render left a hole (sr:776, 813-814), after the row kernel wrote the scanline.  One workgroup
// per (frame, scanline of the range, eye); W x 8 B of LDS.
template <bool MESH>
__global__ void __launch_bounds__(1024) k_edge_rows_exact(RenderArgs a, int rows_max)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    u64* ek = (u64*)smem;
    const int W = a.W, H = a.H, tid = threadIdx.x;
    const int fr = blockIdx.x / rows_max, r = blockIdx.x - fr * rows_max;
    const int eye = blockIdx.y;
    const int f = a.frame0 + fr;
    const FrameDev& fp = a.fp[f];
    if (fp.erow_lo >= fp.erow_hi) return;
    const int y = fp.erow_lo + r;
    if (y > fp.erow_hi || y >= H) return;
    for (int x = tid; x < W; x += 1024) ek[x] = kEmpty64;
    __syncthreads();
    const uint8_t* dbase = a.depth + (size_t)f * a.depth_stride;
    for (int si = y - 1; si <= y; ++si) {
        if (si < 0) continue;
        const uint8_t* urow = a.unused + (size_t)fr * a.ws_stride_px + (size_t)si * W;
        const uint8_t* drow = dbase + (size_t)si * a.depth_pitch;
        for (int j = tid; j < W; j += 1024) {
            if (!urow[j]) continue;
            const uint32_t code = code16_of(load_px_bytes(drow, j));
            const float z = decode_z(code, fp.mult, fp.scale);
            EdgePx ep;
            edge_point_pixels(fp, W, H, si, j, MESH ? 1 : 0, z, ep);
            if (ep.ok[eye] && ep.y[eye] == y)
                atomicMin(&ek[ep.x[eye]], ((u64)code << 17) | ((u64)(uint32_t)(si - (y - 1)) << 16) | (u64)(uint32_t)j);
        }
    }
    __syncthreads();
    const uint8_t* mrow = a.mask[eye] + (size_t)f * a.mask_stride + (size_t)y * a.mask_pitch;
    uint8_t* orow = a.rgb[eye] + (size_t)f * a.rgb_stride + (size_t)y * a.rgb_pitch;
    for (int x = tid; x < W; x += 1024) {
        const u64 k = ek[x];
        if (k == kEmpty64 || !mrow[x]) continue;
        const int sj = (int)(k & 0xFFFFu), si = y - 1 + (int)((k >> 16) & 1u);
        if (a.edge_paint) store_px_bytes(orow, x, load_px_bytes(a.color + (size_t)f * a.color_stride + (size_t)si * a.color_pitch, sj));
        if (a.seed[eye])
            store_px_bytes(a.seed[eye] + (size_t)f * a.seed_stride + (size_t)y * a.seed_pitch, x, edge_normal_colour(a, fp, f, eye, si, sj, MESH ? 1 : 0));
    }
}

hipError_t launch_edge_rows_exact(const RenderPlan& plan, const RenderArgs& a, hipStream_t s)
{
    if (!(plan.remove_edges && plan.edge_points) || plan.edge_rows_max <= 0) return hipSuccess;
    const dim3 grid((unsigned)(plan.n * plan.edge_rows_max), 2u), block(1024);
    const size_t lds = (size_t)a.W * sizeof(u64);
    if (plan.mode == MDVT_MODE_MESH) hipLaunchKernelGGL(k_edge_rows_exact<true>, grid, block, lds, s, a, plan.edge_rows_max);
    else hipLaunchKernelGGL(k_edge_rows_exact<false>, grid, block, lds, s, a, plan.edge_rows_max);
    return hipGetLastError();
}

// Edge points of every OTHER scanline of a pure-shift frame (sr:589-606, 745-781, 813-814): there a point of source row y lands
// on scanline y, in the column edge_col_pure gives (f32 estimate, the reference's f64 chain inside the guard band), nearest first
// (depth code, then the lower column), and is painted where the render left a hole -- after the row kernel, which then renders
// WITHOUT edge points: inside k_mesh_band they cost 11 us per 1080p frame (keys through the z-buffer row's LDS, two more barriers
// per scanline and eye, 17 VGPRs at the 128 limit).  One workgroup per (kEdgeRowsPer scanlines, frame), both eyes; 2 x W x 4 B of LDS.
constexpr int kEdgeRowsPer = 8;           // scanlines per workgroup of k_edge_rows_pure (<= 16: hit list entries)
constexpr int kEdgeHitCap = 1024;         // entries of its hit list (a workgroup with more paints the rest where it finds them)

// what a thread of k_edge_rows_pure<., true> reads from memory for one scanline: flags, depth codes, both eyes' hole masks of its 4-column groups
template <int NIT> struct EdgeRowRegs { uint32_t u4[NIT], dw[NIT][3], m0[NIT], m1[NIT]; };
template <int NIT>
__device__ __forceinline__ void edge_row_fetch(const RenderArgs& a, int fr, int f, int y, int tid, EdgeRowRegs<NIT>& r)
{
    const int W = a.W;
    const uint8_t* urow = a.unused + (size_t)fr * a.ws_stride_px + (size_t)y * W;
    const uint8_t* drow = a.depth + (size_t)f * a.depth_stride + (size_t)y * a.depth_pitch;
    const uint8_t* mrow0 = a.mask[0] + (size_t)f * a.mask_stride + (size_t)y * a.mask_pitch;
    const uint8_t* mrow1 = a.mask[1] + (size_t)f * a.mask_stride + (size_t)y * a.mask_pitch;
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
        const int j0 = tid * 4 + it * 1024;
        r.u4[it] = 0; r.m0[it] = r.m1[it] = 0; r.dw[it][0] = r.dw[it][1] = r.dw[it][2] = 0;
        if (j0 < W && y < a.H) {
            r.u4[it] = *(const uint32_t*)(urow + j0);
            const uint32_t* dp = (const uint32_t*)(drow + 3 * (size_t)j0);
            r.dw[it][0] = dp[0]; r.dw[it][1] = dp[1]; r.dw[it][2] = dp[2];
            r.m0[it] = *(const uint32_t*)(mrow0 + j0); r.m1[it] = *(const uint32_t*)(mrow1 + j0);
        }
    }
}

// NIT: 4-column groups per thread (W <= 1024 NIT), 0: rows that are not dword-addressable, column by column
template <bool MESH, int NIT>
__global__ void __launch_bounds__(256, 5) k_edge_rows_pure(RenderArgs a, int rows_per)      // (5 waves per SIMD: 94 VGPRs without a spill; unhinted the compiler takes 128)
{
    constexpr bool VEC = NIT > 0;
    constexpr int NR = NIT > 0 ? NIT : 1;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    uint32_t* ek = (uint32_t*)smem;                       // [2][W]: depth code << 16 | source column; EMPTY between scanlines
    const int W = a.W, H = a.H, fr = blockIdx.y, tid = threadIdx.x;
    // the workgroup's hits (a key in a hole), painted together at the end: x | source column << 16, scanline - y0 | eye << 4
    uint2* hitq = (uint2*)(ek + 2 * W);
    __shared__ uint32_t nhit;
    if (tid == 0) nhit = 0u;
    const int f = a.frame0 + fr;
    const FrameDev& fp = a.fp[f];
    const int y0 = blockIdx.x * rows_per, y1 = min(y0 + rows_per, H);          // (rows_per <= kEdgeRowsPer)
    // VEC (dword-addressable rows, W <= 4096): everything a scanline needs from memory -- flags, depth codes, both hole masks -- is
    // requested together, and a scanline ahead: taken one after the other (flags, then the flagged columns' depth, then the mask
    // under a key) by a workgroup per scanline, the round trips made this a 14 us workgroup for a microsecond of work
    EdgeRowRegs<NR> cur, nxt;
    if (VEC) edge_row_fetch(a, fr, f, y0, tid, cur);
    for (int x = tid; x < 2 * W; x += 256) ek[x] = kEmpty32;
    __syncthreads();
    const float guard = edge_col_guard(W);
    auto paint = [&](int eye, int x, int y, int sj) {                          // sr:776, 813-814: the caller has seen the hole
        if (a.edge_paint)
            store_px_bytes(a.rgb[eye] + (size_t)f * a.rgb_stride + (size_t)y * a.rgb_pitch, x,
                           load_px_bytes(a.color + (size_t)f * a.color_stride + (size_t)y * a.color_pitch, sj));
        if (a.seed[eye])
            store_px_bytes(a.seed[eye] + (size_t)f * a.seed_stride + (size_t)y * a.seed_pitch, x, edge_normal_colour(a, fp, f, eye, y, sj, MESH ? 1 : 0));
    };
#pragma unroll 1
    for (int y = y0; y < y1; ++y) {
        if (VEC) edge_row_fetch(a, fr, f, y + 1 < y1 ? y + 1 : H, tid, nxt);      // (row H: nothing is read)
        bool any = false;
        if (!edge_row_deferred(fp, y)) {                  // (those are k_edge_rows_exact's)
            const uint8_t* drow = a.depth + (size_t)f * a.depth_stride + (size_t)y * a.depth_pitch;
            auto splat = [&](int j, uint32_t px) {
                const uint32_t code = code16_of(px);
                const float z = decode_z(code, fp.mult, fp.scale);
                if (!(z > kNear)) return;
                const float gx = (float)j * fp.sx, d = fp.dl / z;
#pragma unroll
                for (int eye = 0; eye < 2; ++eye) {
                    const int x = edge_col_pure(fp, eye, gx, z, d, W, guard);      // sr:599-600, 746
                    if (x >= 0) { atomicMin(&ek[eye * W + x], (code << 16) | (uint32_t)j); any = true; }
                }
            };
            if (VEC) {
                // the flagged columns of the thread, one bit each; ONE copy of the splat code walks them (unrolled over the 16 columns
                // the kernel was 14 000 instructions, 110 KB: every wave stalled on instruction fetch)
                uint32_t todo = 0;
#pragma unroll
                for (int it = 0; it < NR; ++it)
#pragma unroll
                    for (int q = 0; q < 4; ++q)
                        if ((cur.u4[it] >> (8 * q)) & 0xFFu) todo |= 1u << (it * 4 + q);
#pragma unroll 1
                while (todo) {
                    const int b = __ffs((int)todo) - 1, it = b >> 2, q = b & 3;
                    todo &= todo - 1u;
                    uint32_t d0 = cur.dw[0][0], d1 = cur.dw[0][1], d2 = cur.dw[0][2];
#pragma unroll
                    for (int k = 1; k < NR; ++k)
                        if (it == k) { d0 = cur.dw[k][0]; d1 = cur.dw[k][1]; d2 = cur.dw[k][2]; }
                    const u64 lo = (u64)d0 | ((u64)d1 << 32), hi = (u64)d1 | ((u64)d2 << 32);
                    const uint32_t px = (q < 2 ? (uint32_t)(lo >> (24 * q)) : (uint32_t)(hi >> (24 * q - 32))) & 0xFFFFFFu;
                    splat(tid * 4 + it * 1024 + q, px);
                }
            } else {
                const uint8_t* urow = a.unused + (size_t)fr * a.ws_stride_px + (size_t)y * W;
                for (int j = tid; j < W; j += 256)
                    if (urow[j]) splat(j, load_px_bytes(drow, j));
            }
        }
        if (__syncthreads_or((int)any)) {                 // (workgroup uniform)
            if (VEC) {
                uint32_t hits = 0;                       // bit (it * 2 + eye) * 4 + q: a key in a hole
#pragma unroll
                for (int it = 0; it < NR; ++it) {
                    const int x0 = tid * 4 + it * 1024;
                    if (x0 >= W) continue;
#pragma unroll
                    for (int eye = 0; eye < 2; ++eye) {
                        const uint32_t m = eye ? cur.m1[it] : cur.m0[it];
                        if (!m) continue;                                           // no hole among the four
                        const uint4 k4 = *(const uint4*)(ek + eye * W + x0);
                        const uint32_t kq[4] = {k4.x, k4.y, k4.z, k4.w};
#pragma unroll
                        for (int q = 0; q < 4; ++q)
                            if (kq[q] != kEmpty32 && ((m >> (8 * q)) & 0xFFu)) hits |= 1u << ((it * 2 + eye) * 4 + q);
                    }
                }
                // the hits go to the workgroup's list and are painted when all its scanlines are through: painting is a chain of
                // dependent loads (source colour; for the seed image the 3 x 3 neighbourhood of the vertex) that a lane walking its own
                // hits one after the other waited 5 us per scanline for
#pragma unroll 1
                while (hits) {
                    const int b = __ffs((int)hits) - 1, it = b >> 3, eye = (b >> 2) & 1, q = b & 3;
                    hits &= hits - 1u;
                    const int x = tid * 4 + it * 1024 + q;
                    const int sj = (int)(ek[eye * W + x] & 0xFFFFu);
                    const uint32_t slot = atomicAdd(&nhit, 1u);
                    if (slot < (uint32_t)kEdgeHitCap) hitq[slot] = make_uint2((uint32_t)x | ((uint32_t)sj << 16), (uint32_t)(y - y0) | ((uint32_t)eye << 4));
                    else paint(eye, x, y, sj);           // (list full: at once)
                }
#pragma unroll
                for (int it = 0; it < NR; ++it) {         // (every thread leaves its own words EMPTY for the next scanline)
                    const int x0 = tid * 4 + it * 1024;
                    if (x0 >= W) continue;
                    *(uint4*)(ek + x0) = make_uint4(kEmpty32, kEmpty32, kEmpty32, kEmpty32);
                    *(uint4*)(ek + W + x0) = make_uint4(kEmpty32, kEmpty32, kEmpty32, kEmpty32);
                }
            } else {
                for (int eye = 0; eye < 2; ++eye) {
                    const uint8_t* mrow = a.mask[eye] + (size_t)f * a.mask_stride + (size_t)y * a.mask_pitch;
                    for (int x = tid; x < W; x += 256) {
                        const uint32_t key = ek[eye * W + x];
                        ek[eye * W + x] = kEmpty32;
                        if (key != kEmpty32 && mrow[x]) paint(eye, x, y, (int)(key & 0xFFFFu));
                    }
                }
            }
            __syncthreads();
        }
        if (VEC) cur = nxt;
    }
    __syncthreads();
    const uint32_t nh = min(nhit, (uint32_t)kEdgeHitCap);
    for (uint32_t e = tid; e < nh; e += 256) {
        const uint2 h = hitq[e];
        paint((int)(h.y >> 4), (int)(h.x & 0xFFFFu), y0 + (int)(h.y & 15u), (int)(h.x >> 16));
    }
}

hipError_t launch_edge_rows_pure(const RenderPlan& plan, const RenderArgs& a, hipStream_t s)
{
    // (scanlines per workgroup: 8 for a launch of 32 frames, fewer for small launches -- as launch_mesh_band's bands)
    int rows_per = (2 * plan.n * a.H + 2880) / (2 * 2880);
    rows_per = rows_per < 1 ? 1 : (rows_per > kEdgeRowsPer ? kEdgeRowsPer : rows_per);
    const dim3 grid((unsigned)((a.H + rows_per - 1) / rows_per), (unsigned)plan.n), block(256);
    const size_t lds = 2 * (size_t)a.W * sizeof(uint32_t) + (size_t)kEdgeHitCap * sizeof(uint2);
    const int nit = !(plan.vec4 && a.W <= 4096) ? 0 : a.W <= 1024 ? 1 : a.W <= 2048 ? 2 : 4;
#define MDVT_CASE(M, N) hipLaunchKernelGGL((k_edge_rows_pure<M, N>), grid, block, lds, s, a, rows_per)
    if (plan.mode != MDVT_MODE_MESH) return hipErrorInvalidValue;          // (points: see launch_render)
    if (nit == 0) MDVT_CASE(true, 0); else if (nit == 1) MDVT_CASE(true, 1); else if (nit == 2) MDVT_CASE(true, 2); else MDVT_CASE(true, 4);
#undef MDVT_CASE
    return hipGetLastError();
}

}  // namespace MDVT_GRID
}  // namespace mdvt
