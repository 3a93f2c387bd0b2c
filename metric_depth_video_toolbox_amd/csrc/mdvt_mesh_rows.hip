// mdvt_mesh_rows.hip -- MESH MODE, pure stereo shift, one workgroup per (frame, output row): k_mesh_rows with MeshVert, VertStore and
// RegularCell.  It renders the launches that k_mesh_band / k_mesh_band3 (mdvt_mesh_band.hip, mdvt_mesh_band3.hip) do not take
// (mesh_band_supported), among them the frames whose 16-byte vertex rows do not fit the LDS.  Its launchers are below it; launch_render (mdvt_render_dispatch.hip) calls launch_mesh_rows.
//
// Compiled with -ffp-contract=off: see the arithmetic decree in mdvt_device.h / DESIGN.md.
#include "mdvt_device.h"

#include <stdlib.h>

namespace mdvt {
namespace MDVT_GRID {      // one copy per sub-pixel grid (mdvt_internal.h)
// =================================================================================================
// MESH MODE, pure stereo shift: one workgroup per (frame, output row), z-buffer in LDS
// =================================================================================================
//
// With v = grid_y (depth independent) every vertex row is a horizontal line on screen, so an output
// scanline k is covered by exactly ONE row of grid cells: the row c whose snapped span (Yt, Yb]
// contains the scanline (a scanline lying exactly on a vertex row belongs to the cells ABOVE it: the
// row below touches it only with top edges / a top vertex, which the fill rule -- left and bottom edges
// own their pixel centres, edge_in -- excludes for either orientation).  The 2-D rasterisation
// collapses to interval coverage along x.
//
//   stage    the two vertex rows c, c+1 once per workgroup: decode, d = dl/Z, 1/Z, snapped x for BOTH
//            eyes, packed colour -> 16 B per vertex in LDS (coalesced 12 B/lane HBM reads)
//   raster   per eye: one thread per cell walks the pixel centres inside its two triangles, shades each
//            covered fragment perspective-correctly and posts
//               key = ~bits(1/Z interpolated) << 32 | R | G<<8 | B<<16
//            with ds_min_u64 (min == nearest; an exact 1/Z tie between overlapping triangles of different
//            colour is detected and settled by draw order in two more passes over the row -- RowTies in
//            mdvt_device.h).  Spans longer than kShortSpan (rubber-sheet triangles
//            across depth edges) are handed to the whole wave: one lane's triangle is broadcast with
//            v_readlane and 64 lanes test 64 pixel centres at a time.
//   resolve  per eye: plain LDS reads -> colour-key hole test -> coalesced dwordx3 / dword stores.
// The z-buffer holds one eye at a time (the resolve of the left eye resets it), so LDS is
// 2*16*W + 8*W (+4*W with edge points) bytes: 77 KB at 1080p -> two workgroups per CU.

// One covered fragment of a row kernel: interpolated 1/Z and shaded colour into the row's z-buffer.
__device__ __forceinline__ void mesh_row_fragment(u64* zb, int px, float q0, float q1, float q2, uint32_t c0, uint32_t c1, uint32_t c2,
                                                  uint32_t draw, const RowTies& ties)
{
    const float iz = (q0 + q1) + q2;
    const float riz = rcp_exact(iz);
    post_row_fragment(zb, px, iz, shade_px(q0, q1, q2, riz, c0, c1, c2), draw, ties);
}

struct MeshVert { int XL, XR; float iz; uint32_t rgb; };
static_assert(sizeof(MeshVert) == 16, "MeshVert is one ds_read_b128");
constexpr int kShortSpan = 4;

__device__ __forceinline__ MeshVert mesh_vertex(uint32_t dpx, uint32_t cpx, int j, const FrameDev& fp)
{
    MeshVert v;
    const float z = decode_z(code16_of(dpx), fp.mult, fp.scale);
    const bool ok = z > kNear;
    float iz, d;
    rcp_div_exact(fp.dl, fast_operand(fp.dl), z, iz, d);
    const float gx = (float)j * fp.sx;
    v.XL = snap(gx + d);
    v.XR = snap(gx - d);
    v.iz = ok ? iz : 0.0f;                  // iz == 0 flags a vertex behind the near plane
    v.rgb = cpx;
    return v;
}

// Triangle `pass` (0: tri1 = A,B,C; 1: tri2 = A,C,D) of cell column j for one eye from the LDS vertices.
__device__ __forceinline__ bool mesh_tri_lds(TriSetup& t, const MeshVert& A, const MeshVert& B, const MeshVert& Cv,
                                             const MeshVert& D, int pass, int eye, int Yt, int Yb, int cull)
{
    const int XA = eye == 0 ? A.XL : A.XR, XB = eye == 0 ? B.XL : B.XR;
    const int XC = eye == 0 ? Cv.XL : Cv.XR, XD = eye == 0 ? D.XL : D.XR;
    // vertex order of the reference: tri1 = (v[i,j], v[i+1,j], v[i+1,j+1]); tri2 = (v[i,j], v[i+1,j+1], v[i,j+1])
    if (pass == 0) return tri_setup_snapped(t, XA, Yt, A.iz, XB, Yb, B.iz, XC, Yb, Cv.iz, cull);
    return tri_setup_snapped(t, XA, Yt, A.iz, XC, Yb, Cv.iz, XD, Yt, D.iz, cull);
}

// LDS vertex array with 16-byte (colour inside) or 12-byte (colour re-read from the frame in the
// resolve phase; for wide frames whose 16-byte rows would not fit the 160 KB LDS) records.
template <bool VRGB>
struct VertStore {
    static constexpr int kDwords = VRGB ? 4 : 3;
    int* base;
    __device__ __forceinline__ void put(int idx, const MeshVert& v) const
    {
        int* p = base + (size_t)idx * kDwords;
        if (VRGB) *(int4*)p = make_int4(v.XL, v.XR, __float_as_int(v.iz), (int)v.rgb);
        else { p[0] = v.XL; p[1] = v.XR; p[2] = __float_as_int(v.iz); }
    }
    __device__ __forceinline__ MeshVert get(int idx) const
    {
        const int* p = base + (size_t)idx * kDwords;
        MeshVert v;
        if (VRGB) { const int4 q = *(const int4*)p; v.XL = q.x; v.XR = q.y; v.iz = __int_as_float(q.z); v.rgb = (uint32_t)q.w; }
        else { v.XL = p[0]; v.XR = p[1]; v.iz = __int_as_float(p[2]); v.rgb = 0; }
        return v;
    }
};

// Regular cell (both triangles in the grid's own orientation): on the scanline the cell is the interval
// between its two column edges, split by the diagonal A-C.  With
//   E_col_j(X) = h (X - XA) - (XB - XA) t,   E_diag(X) = h (X - XA) - (XC - XA) t
// tri1 = {E_col_j >= 0, E_diag < 0}, tri2 = {E_diag >= 0, E_col_j+1 < 0} (left edges own their centres), and the integer
// barycentric weights are these same edge values -- identical to the generic edge functions, three 64-bit
// subtractions per pixel instead of two triangle set-ups.
struct RegularCell {
    int XA, XB, XC, XD;
    float izA, izB, izC, izD;
    uint32_t cA, cB, cC, cD;
    int flags;              // bit0: tri1 removed, bit1: tri2 removed (dmt:1372)
    int j;                  // cell column (draw order)
};

__device__ __forceinline__ void regular_cell_pixel(const RegularCell& r, int px, int tt, int bb, int hh,
                                                   i64 kcol0, i64 kcol1, i64 kdiag, u64* zb, const RowTies& ties)
{
    const i64 hX = mul64(hh, px * kSubpix + kSubpix / 2);
    const i64 e0 = hX - kcol0, e1 = hX - kcol1, ed = hX - kdiag;
    const bool in1 = e0 >= 0 && ed < 0 && !(r.flags & 1);
    const bool in2 = ed >= 0 && e1 < 0 && !(r.flags & 2);
    if (!(in1 || in2)) return;
    const int wd = in1 ? r.XC - r.XB : r.XD - r.XA;          // the triangle's horizontal edge (operands selected, not products)
    const i64 area2 = mul64(hh, wd);
    const i64 wh = mul64(wd, in1 ? bb : tt);
    const i64 w0 = in1 ? wh : -e1;
    const i64 w1 = in1 ? -ed : wh;
    const i64 w2 = in1 ? e0 : ed;
    float q0, q1, q2;
    tri_weights(area2, r.izA, in1 ? r.izB : r.izC, in1 ? r.izC : r.izD, w0, w1, w2, q0, q1, q2);
    mesh_row_fragment(zb, px, q0, q1, q2, r.cA, in1 ? r.cB : r.cC, in1 ? r.cC : r.cD, ((in1 ? 0u : 1u) << 16) | (uint32_t)r.j, ties);
}

template <int PX, int FLAGS, int TPB, bool VRGB>
__global__ void __launch_bounds__(TPB) k_mesh_rows(RenderArgs a)
{
    constexpr bool ZOUT = FLAGS & 1, EDGES = FLAGS & 2, EDGEPTS = FLAGS & 4, SEED = FLAGS & 8;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int W = a.W, H = a.H;
    u64* zb = (u64*)smem;                              // [W] z keys of the eye being rendered
    VertStore<VRGB> verts{(int*)(zb + W)};             // [2][W]: vertex rows c and c+1
    uint32_t* eb = (uint32_t*)(verts.base + 2 * (size_t)W * VertStore<VRGB>::kDwords);   // [W] edge-point keys (EDGEPTS)
    uint8_t* cfl = (uint8_t*)(eb + (EDGEPTS ? W : 0));  // [W] per-column flags (EDGES): bit0 tri1 removed, bit1 tri2 removed, bit2 vertex (k,j) unused
    uint16_t* kcode = (uint16_t*)(cfl + (EDGES ? (((size_t)W + 15) & ~(size_t)15) : 0));   // [W] 16-bit depth codes of source row k (EDGEPTS)
    RowTies ties;                                       // [W/32 + 1] tie bits + flag (exact depth ties, mdvt_device.h)
    ties.bits = (uint32_t*)(((uintptr_t)(kcode + (EDGEPTS ? W : 0)) + 15) & ~(uintptr_t)15);
    ties.nwords = (W + 31) / 32;
    ties.mode = 0;
    ties.force = (MDVT_DEBUG_SKIP(a) & 32) != 0;

    const int fr = blockIdx.x / H;
    const int k = blockIdx.x - fr * H;                 // output row
    const int f = a.frame0 + fr;
    const FrameDev& fp = a.fp[f];
    const int tid = threadIdx.x;
    const int lane = tid & 63;

    // ---- the cell row covering scanline k (uniform) ----
    const int Yc = k * kSubpix + kSubpix / 2;
    int ilo = (int)(((float)k + 0.5f) / fp.sy);
    ilo = ilo < 0 ? 0 : (ilo > H - 1 ? H - 1 : ilo);
    while (ilo > 0 && snap((float)ilo * fp.sy) >= Yc) --ilo;
    while (ilo + 1 <= H - 1 && snap((float)(ilo + 1) * fp.sy) < Yc) ++ilo;
    const int c = (ilo <= H - 2) ? ilo : -1;           // largest i with Ys(i) < Yc (fill rule: bottom edges own their centres); -1: below the last vertex row
    const int Yt = c >= 0 ? snap((float)c * fp.sy) : 0;
    const int Yb = c >= 0 ? snap((float)(c + 1) * fp.sy) : 0;
    const int tt = Yc - Yt, bb = Yb - Yc, hh = Yb - Yt;     // scanline position inside the cell row (sub-pixels)
    const float tf = c >= 0 ? (float)tt / (float)hh : 0.0f; // scanline height inside the cell row, for the candidate estimate only

    // ---- stage the two vertex rows, clear the z-buffer ----
    if (c >= 0 && !(MDVT_DEBUG_SKIP(a) & 4)) {
        const int ngroups = W / PX;
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            const uint8_t* drow = a.depth + (size_t)f * a.depth_stride + (size_t)(c + r) * a.depth_pitch;
            const uint8_t* crow = a.color + (size_t)f * a.color_stride + (size_t)(c + r) * a.color_pitch;
            for (int g = tid; g < ngroups; g += TPB) {
                uint32_t dpx[PX], cpx[PX];
                RowIO<PX>::load(drow, g, dpx);
                RowIO<PX>::load(crow, g, cpx);
#pragma unroll
                for (int q = 0; q < PX; ++q) {
                    verts.put(r * W + g * PX + q, mesh_vertex(dpx[q], cpx[q], g * PX + q, fp));
                    if (EDGEPTS && c + r == k) kcode[g * PX + q] = (uint16_t)code16_of(dpx[q]);
                }
            }
        }
    }
    for (int x = tid; x < W; x += TPB) zb[x] = kEmpty64;
    for (int x = tid; x <= ties.nwords; x += TPB) ties.bits[x] = 0u;
    if (EDGEPTS) for (int x = tid; x < W; x += TPB) eb[x] = kEmpty32;
    if (EDGES) {
        // removed-triangle flags of this cell row and unused-vertex flags of source row k: one coalesced pass
        const size_t ncell_ = (size_t)(W - 1) * (H - 1);
        const uint8_t* ti = c >= 0 ? a.tri_invalid + (size_t)fr * a.ws_stride_tri + (size_t)c * (W - 1) : nullptr;
        const uint8_t* ur = a.unused + (size_t)fr * a.ws_stride_px + (size_t)k * W;
        for (int x = tid; x < W; x += TPB) {
            uint32_t fl = 0;
            if (ti && x < W - 1) fl = (ti[x] ? 1u : 0u) | (ti[ncell_ + x] ? 2u : 0u);
            if (EDGEPTS && ur[x]) fl |= 4u;
            cfl[x] = (uint8_t)fl;
        }
    }
    __syncthreads();

    const uint8_t* crow_k = a.color + (size_t)f * a.color_stride + (size_t)k * a.color_pitch;

#pragma unroll 1
    for (int eye = 0; eye < 2; ++eye) {
        // ---- rasterise this eye (passes 1 and 2 only for a row with exact depth ties, see RowTies) ----
#pragma unroll 1
        for (ties.mode = 0; ties.mode < 3; ++ties.mode) {
        if (c >= 0 && !(MDVT_DEBUG_SKIP(a) & 1)) {
            for (int j0 = 0; j0 < W - 1; j0 += TPB) {
                const int j = j0 + tid;
                TriSetup t[2];
                int px0[2], px1[2];
                uint32_t col[2][3];
                bool lng[2] = {false, false};
                RegularCell rc;
                int rp0 = 0, rp1 = -1;
                bool lngcell = false;
                if (j < W - 1) {
                    const MeshVert A = verts.get(j), D = verts.get(j + 1), B = verts.get(W + j), Cv = verts.get(W + j + 1);
                    const int XA = eye == 0 ? A.XL : A.XR, XB = eye == 0 ? B.XL : B.XR;
                    const int XC = eye == 0 ? Cv.XL : Cv.XR, XD = eye == 0 ? D.XL : D.XR;
                    const uint32_t fl = EDGES ? cfl[j] : 0u;
                    const bool inv1 = fl & 1u, inv2 = fl & 2u;                                       // dmt:1372
                    uint32_t cA = A.rgb, cB = B.rgb, cC = Cv.rgb, cD = D.rgb;
                    if (!VRGB) {
                        const uint8_t* cr0 = a.color + (size_t)f * a.color_stride + (size_t)c * a.color_pitch;
                        const uint8_t* cr1 = cr0 + a.color_pitch;
                        cA = load_px_bytes(cr0, j); cD = load_px_bytes(cr0, j + 1);
                        cB = load_px_bytes(cr1, j); cC = load_px_bytes(cr1, j + 1);
                    }
                    col[0][0] = cA; col[0][1] = cB; col[0][2] = cC;
                    col[1][0] = cA; col[1][1] = cC; col[1][2] = cD;
                    const bool allok = A.iz > 0.0f && B.iz > 0.0f && Cv.iz > 0.0f && D.iz > 0.0f;
                    int p0 = floordiv_subpix(min(XA, XB) - kSubpix / 2 + kSubpix - 1);
                    int p1 = floordiv_subpix(max(XC, XD) - kSubpix / 2);
                    if (p0 < 0) p0 = 0;
                    if (p1 > W - 1) p1 = W - 1;
                    rc.XA = XA; rc.XB = XB; rc.XC = XC; rc.XD = XD;
                    rc.izA = A.iz; rc.izB = B.iz; rc.izC = Cv.iz; rc.izD = D.iz;
                    rc.cA = cA; rc.cB = cB; rc.cC = cC; rc.cD = cD;
                    rc.flags = (inv1 ? 1 : 0) | (inv2 ? 2 : 0);
                    rc.j = j;
                    if (allok && XC > XB && XD > XA) {
                        if (a.cull == 2) rc.flags = 3;                 // a regular cell is two front faces
                        if (rc.flags != 3) {
                            const i64 kcol0 = mul64(XB - XA, tt) + mul64(hh, XA);
                            const i64 kcol1 = mul64(XC - XD, tt) + mul64(hh, XD);
                            // The cell meets the scanline in [kcol0/h, kcol1/h) -- for a cell sheared across a
                            // horizontal depth edge that is ~1 px although its bounding box spans the whole
                            // disparity jump.  Candidate pixels from a float estimate of the two crossings,
                            // widened by one pixel (the estimate is good to ~0.1 px inside the snap range); the
                            // exact integer tests in regular_cell_pixel decide.
                            // crossings XA + (XB-XA) t/h and XD + (XC-XD) t/h from 32-bit conversions (the 64-bit kcol values
                            // would cost ~10 instructions each to convert); only the estimate, the integer tests decide
                            constexpr float kHalf = (float)(kSubpix / 2), kInv = 1.0f / (float)kSubpix;
                            int q0 = (int)floorf((((float)XA + (float)(XB - XA) * tf) - kHalf) * kInv);
                            int q1 = (int)floorf((((float)XD + (float)(XC - XD) * tf) - kHalf) * kInv) + 1;
                            if (q0 < p0) q0 = p0;
                            if (q1 > p1) q1 = p1;
                            rp0 = q0; rp1 = q1;
                            if (q1 - q0 >= kShortSpan) {
                                lngcell = true;           // rubber-sheet cell across a vertical depth edge: whole-wave path below
                            } else if (!(MDVT_DEBUG_SKIP(a) & 16)) {
                                const i64 kdiag = mul64(XC - XA, tt) + mul64(hh, XA);
                                for (int px = q0; px <= q1; ++px) regular_cell_pixel(rc, px, tt, bb, hh, kcol0, kcol1, kdiag, zb, ties);
                            }
                        }
                    } else {
                        // folded / degenerate / near-plane / long-span cells: the generic triangle path
#pragma unroll
                        for (int pass = 0; pass < 2; ++pass) {
                            if (pass == 0 ? inv1 : inv2) continue;
                            if (!mesh_tri_lds(t[pass], A, B, Cv, D, pass, eye, Yt, Yb, a.cull)) continue;
                            const TriSetup& tr = t[pass];
                            int q0p = floordiv_subpix(tr.minX - kSubpix / 2 + kSubpix - 1), q1p = floordiv_subpix(tr.maxX - kSubpix / 2);
                            if (q0p < 0) q0p = 0;
                            if (q1p > W - 1) q1p = W - 1;
                            px0[pass] = q0p; px1[pass] = q1p;
                            if (q1p - q0p >= kShortSpan) { lng[pass] = true; continue; }
                            for (int px = q0p; px <= q1p; ++px) {
                                float q0, q1, q2;
                                if (!tri_sample(tr, px, k, q0, q1, q2)) continue;
                                mesh_row_fragment(zb, px, q0, q1, q2, col[pass][0], col[pass][1], col[pass][2], ((uint32_t)pass << 16) | (uint32_t)j, ties);
                            }
                        }
                    }
                }
                // long regular cells: the whole wave works on one lane's cell at a time (64 pixel centres per step)
                {
                    u64 m = (MDVT_DEBUG_SKIP(a) & 8) ? 0ull : __ballot(lngcell);
                    while (m) {
                        const int l = __builtin_amdgcn_readfirstlane(__ffsll((long long)m) - 1);
                        m &= m - 1;
                        RegularCell b;
#define MDVT_BI(fld) b.fld = __builtin_amdgcn_readlane(rc.fld, l)
#define MDVT_BF(fld) b.fld = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(rc.fld), l))
#define MDVT_BU(fld) b.fld = (uint32_t)__builtin_amdgcn_readlane((int)rc.fld, l)
                        MDVT_BI(XA); MDVT_BI(XB); MDVT_BI(XC); MDVT_BI(XD); MDVT_BI(flags); MDVT_BI(j);
                        MDVT_BF(izA); MDVT_BF(izB); MDVT_BF(izC); MDVT_BF(izD);
                        MDVT_BU(cA); MDVT_BU(cB); MDVT_BU(cC); MDVT_BU(cD);
#undef MDVT_BI
#undef MDVT_BF
#undef MDVT_BU
                        const int bp0 = __builtin_amdgcn_readlane(rp0, l), bp1 = __builtin_amdgcn_readlane(rp1, l);
                        const i64 kcol0 = mul64(b.XB - b.XA, tt) + mul64(hh, b.XA);
                        const i64 kcol1 = mul64(b.XC - b.XD, tt) + mul64(hh, b.XD);
                        const i64 kdiag = mul64(b.XC - b.XA, tt) + mul64(hh, b.XA);
                        for (int px = bp0 + lane; px <= bp1; px += 64) regular_cell_pixel(b, px, tt, bb, hh, kcol0, kcol1, kdiag, zb, ties);
                    }
                }
                // long spans of irregular cells: the whole wave works on one lane's triangle at a time
#pragma unroll
                for (int pass = 0; pass < 2; ++pass) {
                    u64 m = (MDVT_DEBUG_SKIP(a) & 8) ? 0ull : __ballot(lng[pass]);
                    while (m) {
                        const int l = __builtin_amdgcn_readfirstlane(__ffsll((long long)m) - 1);
                        m &= m - 1;
                        TriSetup b;
#define MDVT_BCAST(fld) b.fld = __builtin_amdgcn_readlane(t[pass].fld, l)
                        MDVT_BCAST(dx0); MDVT_BCAST(dy0); MDVT_BCAST(dx1); MDVT_BCAST(dy1); MDVT_BCAST(dx2); MDVT_BCAST(dy2);
                        MDVT_BCAST(bx0); MDVT_BCAST(by0); MDVT_BCAST(bx1); MDVT_BCAST(by1); MDVT_BCAST(bx2); MDVT_BCAST(by2);
#undef MDVT_BCAST
                        const uint32_t alo = __builtin_amdgcn_readlane((int)(uint32_t)t[pass].area2, l);
                        const uint32_t ahi = __builtin_amdgcn_readlane((int)(uint32_t)((u64)t[pass].area2 >> 32), l);
                        b.area2 = (i64)(((u64)ahi << 32) | alo);
                        b.iz0 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(t[pass].iz0), l));
                        b.iz1 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(t[pass].iz1), l));
                        b.iz2 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(t[pass].iz2), l));
                        const int bp0 = __builtin_amdgcn_readlane(px0[pass], l), bp1 = __builtin_amdgcn_readlane(px1[pass], l);
                        const uint32_t bc0 = __builtin_amdgcn_readlane((int)col[pass][0], l);
                        const uint32_t bc1 = __builtin_amdgcn_readlane((int)col[pass][1], l);
                        const uint32_t bc2 = __builtin_amdgcn_readlane((int)col[pass][2], l);
                        const int bj = __builtin_amdgcn_readlane(j, l);
                        for (int px = bp0 + lane; px <= bp1; px += 64) {
                            float q0, q1, q2;
                            if (!tri_sample(b, px, k, q0, q1, q2)) continue;
                            mesh_row_fragment(zb, px, q0, q1, q2, bc0, bc1, bc2, ((uint32_t)pass << 16) | (uint32_t)bj, ties);
                        }
                    }
                }
            }
        }
        if (ties.mode == 0) {
        // ---- edge points of source row k (sr:589-606, 745-781): vertices of removed triangles ----
        if (EDGEPTS && !edge_row_deferred(fp, k)) {        // (scanlines erow_lo .. erow_hi: k_edge_rows_exact)
            const uint8_t* drow_k = a.depth + (size_t)f * a.depth_stride + (size_t)k * a.depth_pitch;
            const bool k_staged = c >= 0 && (k == c || k == c + 1) && !(MDVT_DEBUG_SKIP(a) & 4);
            const float guard = edge_col_guard(W);
            for (int j = tid; j < W; j += TPB) {
                if (!(cfl[j] & 4u)) continue;
                const uint32_t code = k_staged ? (uint32_t)kcode[j] : code16_of(load_px_bytes(drow_k, j));
                const float z = decode_z(code, fp.mult, fp.scale);
                if (!(z > kNear)) continue;
                const int x = edge_col_pure(fp, eye, (float)j * fp.sx, z, fp.dl / z, W, guard);     // sr:599-600, 746
                if (x >= 0) atomicMin(&eb[x], (code << 16) | (uint32_t)j);
            }
        }
        }
        __syncthreads();
        if (ties.mode == 0) {
            if (ties.bits[ties.nwords] == 0u) break;
            row_ties_prepare(zb, W, ties, tid, TPB);
            __syncthreads();
        }
        }
        const bool had_ties = ties.mode == 3;            // the loop ran to its end (a row without ties leaves it at mode 0)
        ties.mode = 0;

        // ---- resolve this eye ----
        uint8_t* orow = a.rgb[eye] + (size_t)f * a.rgb_stride + (size_t)k * a.rgb_pitch;
        uint8_t* mrow = a.mask[eye] + (size_t)f * a.mask_stride + (size_t)k * a.mask_pitch;
        float* zrow = ZOUT && a.zout[eye]
                          ? (float*)((uint8_t*)a.zout[eye] + (size_t)f * a.zout_stride + (size_t)k * a.zout_pitch)
                          : nullptr;
        for (int g = tid; g < W / PX && !(MDVT_DEBUG_SKIP(a) & 2); g += TPB) {
            uint32_t opx[PX], om[PX], spx[PX];
            float oz[PX];
#pragma unroll
            for (int q = 0; q < PX; ++q) {
                const int x = g * PX + q;
                const u64 key = zb[x];
                const bool covered = key != kEmpty64;
                const uint32_t rgb = covered ? (uint32_t)key & 0xFFFFFFu : 0u;
                float zval = 0.0f;
                if (ZOUT && covered) zval = 1.0f / row_word_iz((uint32_t)(key >> 32));
                const bool hole = !covered || rgb == a.key_rgb;
                uint32_t out = hole ? 0u : rgb;
                uint32_t esrc = ~0u;
                if (EDGEPTS) {
                    const uint32_t ek = eb[x];
                    if (hole && ek != kEmpty32) { if (a.edge_paint) out = load_px_bytes(crow_k, (int)(ek & 0xFFFFu)); esrc = ((uint32_t)k << 16) | (ek & 0xFFFFu); }
                    if (eye == 0) eb[x] = kEmpty32;
                }
                if (SEED && a.seed[eye]) spx[q] = seed_pixel(a, fp, f, eye, x, k, hole, esrc, 1);
                if (eye == 0) zb[x] = kEmpty64;               // ready for the right eye
                opx[q] = out;
                om[q] = hole ? 255u : 0u;
                if (ZOUT) oz[q] = zval;
            }
            RowIO<PX>::store_rgb(orow, g, opx);
            RowIO<PX>::store_mask(mrow, g, om);
            if (ZOUT && zrow) RowIO<PX>::store_z(zrow, g, oz);
            if (SEED && a.seed[eye]) RowIO<PX>::store_rgb(a.seed[eye] + (size_t)f * a.seed_stride + (size_t)k * a.seed_pitch, g, spx);
        }
        if (had_ties) for (int x = tid; x <= ties.nwords; x += TPB) ties.bits[x] = 0u;
        if (eye == 0) __syncthreads();
    }
}

template <int PX, int TPB>
static hipError_t launch_mesh_rows_tpb(const RenderPlan& plan, const RenderArgs& a, size_t lds, bool vrgb, hipStream_t s)
{
    const dim3 grid((unsigned)(plan.n * a.H)), block(TPB);
    const bool zout = a.zout[0] || a.zout[1];
    const int flags = (zout ? 1 : 0) | (plan.remove_edges ? 2 : 0) | (plan.remove_edges && plan.edge_points ? 4 : 0) |
                      (plan.remove_edges && a.seed[0] ? 8 : 0);
#define MDVT_CASE(F)                                                                                   \
    case F:                                                                                            \
        if (vrgb) {                                                                                    \
            if (lds > 48 * 1024)                                                                       \
                (void)hipFuncSetAttribute((const void*)k_mesh_rows<PX, F, TPB, true>,                  \
                                          hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);       \
            hipLaunchKernelGGL((k_mesh_rows<PX, F, TPB, true>), grid, block, lds, s, a);               \
        } else {                                                                                       \
            (void)hipFuncSetAttribute((const void*)k_mesh_rows<PX, F, TPB, false>,                     \
                                      hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);           \
            hipLaunchKernelGGL((k_mesh_rows<PX, F, TPB, false>), grid, block, lds, s, a);              \
        }                                                                                              \
        break;
    switch (flags) {
        MDVT_CASE(0) MDVT_CASE(1) MDVT_CASE(2) MDVT_CASE(3) MDVT_CASE(6) MDVT_CASE(7)
        MDVT_CASE(10) MDVT_CASE(11) MDVT_CASE(14) MDVT_CASE(15)
        default: return hipErrorInvalidValue;
    }
#undef MDVT_CASE
    return hipGetLastError();
}

template <int PX>
static hipError_t launch_mesh_rows_px(const RenderPlan& plan, const RenderArgs& a_in, hipStream_t s)
{
    RenderArgs a = a_in;
    if (const char* e = tuning_env(TUNE_DEBUG_SKIP)) a.debug_skip = atoi(e);
    const size_t lds = render_lds_bytes(plan, a.W);
    if (lds > kMaxLds) return hipErrorNotSupported;         // W > ~4300 with edge points (5120 without)
    const bool vrgb = lds == 2 * (size_t)a.W * 16 + (size_t)a.W * 8 + (plan.edge_points ? (size_t)a.W * 4 + 2 * (size_t)a.W + 16 : 0) +
                             (plan.remove_edges ? (((size_t)a.W + 15) & ~(size_t)15) : 0) + mesh_rows_tie_bytes(a.W);
    // two 512-thread workgroups per CU when two fit in the 160 KB LDS, otherwise one 1024-thread workgroup:
    // either way 16 waves per CU
    int tpb = (2 * lds <= kMaxLds) ? 512 : 1024;
    if (const char* e = tuning_env(TUNE_MESH_TPB)) tpb = atoi(e);
    if (tpb == 1024) return launch_mesh_rows_tpb<PX, 1024>(plan, a, lds, vrgb, s);
    return launch_mesh_rows_tpb<PX, 512>(plan, a, lds, vrgb, s);
}

hipError_t launch_mesh_rows(const RenderPlan& plan, const RenderArgs& a, hipStream_t s)
{
    return plan.vec4 ? launch_mesh_rows_px<4>(plan, a, s) : launch_mesh_rows_px<1>(plan, a, s);
}

}  // namespace MDVT_GRID
}  // namespace mdvt
