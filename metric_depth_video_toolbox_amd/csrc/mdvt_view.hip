// mdvt_view.hip -- the per-frame centre of the vertices (mdvt_view_centers, include/mdvt_view.h): what the reference's
// 3d_view_depthfile.py:231 reads with draw_mesh.get_center() to aim its camera, the mean of every transformed vertex of a frame.
//
// The vertices.  dmt.create_point_cloud_from_depth (dmt:1112-1133) as NumPy >= 2 evaluates it: the f32 depth (code << 16 times
// f32(max_depth / 255^4), times f32(depth_scale)) widened to f64, ((g - c) * z) / f per axis with the f32 grid of the mesh mode
// (vertex_f64, mdvt_device.h: the edge filter's own vertices).  With a pose, Open3D's point transform: the 4 x 4 times (x, y, z, 1),
// sums left to right, divided by its w.  Points mode with remove_edges: a vertex of a removed triangle is then parked at
// (-0.2, -0.2, -0.2) (dmt:1091).  One IEEE f64 operation per node, no contraction (Makefile).
//
// The order.  Each coordinate's N = W H values are summed as np.sum sums a contiguous f64 array: consecutive chunks of 8192 elements,
// each by the pairwise routine, the chunk sums added one after the other from 0 (include/mdvt_convergence.h states the routine; it
// does not depend on the element type).  The three coordinates of a vertex share one walk: mdvt_pairwise.h is instantiated on a triple
// of doubles that adds element by element.  No floating-point atomics, no dependence on the launch geometry.
//
//   k_view_chunk_sums   one workgroup of four waves per chunk of 8192 vertices and frame.  A full chunk: four threads per leaf of
//                       128, thread q of a leaf keeps the accumulators r[2 q] and r[2 q + 1] -- 32 vertices, computed where they are
//                       summed (8192 x 24 B would not fit a workgroup's LDS) --, the four join as ((r0 + r1) + (r2 + r3)) +
//                       ((r4 + r5) + (r6 + r7)) by two butterfly steps, then the balanced tree over the wave's 16 leaves and over
//                       the four waves (IEEE add is commutative: both sides of a step hold the same bits).  A shorter chunk: the
//                       general shape of mdvt_pairwise.h.  A vertex is 6 bytes read against some 60 f64 operations, two of
//                       them divisions: the vertices are read with plain byte loads (profiles/r15_view_centers.md: 680 GB/s of
//                       input at 4K).
//   k_view_centers      one wave per frame: the chunk sums in order, the division by N
#include "mdvt_device.h"
#include "mdvt_pairwise.h"

namespace mdvt {
namespace {

using pairwise::kChunk;
using pairwise::kLeaf;

struct D3 { double x, y, z; };        // (an aggregate: D3() is zero)
__device__ __forceinline__ D3 operator+(const D3& a, const D3& b) { return D3{a.x + b.x, a.y + b.y, a.z + b.z}; }
__device__ __forceinline__ D3& operator+=(D3& a, const D3& b) { a.x += b.x; a.y += b.y; a.z += b.z; return a; }
__device__ __forceinline__ D3 shfl_xor_d3(const D3& v, int m) { return D3{__shfl_xor(v.x, m), __shfl_xor(v.y, m), __shfl_xor(v.z, m)}; }

// vertex i of the chunk that starts at vertex `first` of the frame
struct Vertices {
    const FrameDev& fp;
    const uint8_t* frame; size_t pitch;
    const uint8_t* unused;            // the frame's flags, or null: nothing is parked
    uint32_t W, first;
    int of_by_one;
    __device__ __forceinline__ D3 operator()(int i) const
    {
        const uint32_t v = first + (uint32_t)i;
        const uint32_t row = v / W, col = v - row * W;
        const float z = decode_z(code16_of(load_px_bytes(frame + (size_t)row * pitch, (int)col)), fp.mult, fp.scale);
        double p[3];
        vertex_f64(fp, (int)row, (int)col, of_by_one, z, p);
        if (fp.has_T) {
            const double* T = fp.Td;
            double hh[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) hh[r] = ((T[4 * r] * p[0] + T[4 * r + 1] * p[1]) + T[4 * r + 2] * p[2]) + T[4 * r + 3] * 1.0;
            if (hh[3] != 1.0) { hh[0] = hh[0] / hh[3]; hh[1] = hh[1] / hh[3]; hh[2] = hh[2] / hh[3]; }     // (x / 1.0 == x)
            p[0] = hh[0]; p[1] = hh[1]; p[2] = hh[2];
        }
        if (unused && unused[v]) p[0] = p[1] = p[2] = -0.2;                  // dmt:1091
        return D3{p[0], p[1], p[2]};
    }
};

constexpr int kSumThreads = 256;      // four per leaf of a full chunk

__global__ void __launch_bounds__(kSumThreads) k_view_chunk_sums(ViewCentersArgs a)
{
    __shared__ pairwise::ShapeT<D3> s_shape;
    __shared__ D3 s_val[4];
    const int tid = (int)threadIdx.x;
    const uint32_t c = blockIdx.x;
    const int fr = (int)blockIdx.y;
    const uint32_t first = c * (uint32_t)kChunk;
    if (first >= a.npx) return;
    const int n = (int)(a.npx - first < (uint32_t)kChunk ? a.npx - first : (uint32_t)kChunk);
    const int f = a.frame0 + fr;
    const Vertices v{a.fp[f], a.depth + (size_t)f * a.depth_stride, a.depth_pitch,
                     a.unused ? a.unused + (size_t)fr * a.unused_stride : nullptr, (uint32_t)a.W, first, a.of_by_one};
    D3* const out = reinterpret_cast<D3*>(a.sums) + ((size_t)fr * a.nchunks + c);

    if (n == kChunk) {
        const int base = (tid >> 2) * kLeaf + 2 * (tid & 3);
        D3 r0 = v(base), r1 = v(base + 1);
#pragma unroll 1
        for (int i = 8; i < kLeaf; i += 8) {
            r0 += v(base + i);
            r1 += v(base + i + 1);
        }
        D3 res = r0 + r1;
#pragma unroll
        for (int m = 1; m < 64; m <<= 1) res = res + shfl_xor_d3(res, m);
        if ((tid & 63) == 0) s_val[tid >> 6] = res;
        __syncthreads();
        if (tid == 0) *out = (s_val[0] + s_val[1]) + (s_val[2] + s_val[3]);
        return;
    }
    if (tid == 0) pairwise::shape_list(s_shape, n);
    __syncthreads();
    pairwise::shape_leaves(s_shape, v, tid);
    __syncthreads();
    if (tid == 0) *out = pairwise::shape_join(s_shape);
}

__global__ void __launch_bounds__(64) k_view_centers(ViewCentersArgs a)
{
    const int lane = (int)threadIdx.x;
    const int fr = (int)blockIdx.x;
    const D3* sums = reinterpret_cast<const D3*>(a.sums) + (size_t)fr * a.nchunks;
    D3 acc = D3();
    for (uint32_t base = 0; base < a.nchunks; base += 64u) {
        const D3 s = base + (uint32_t)lane < a.nchunks ? sums[base + (uint32_t)lane] : D3();
        const int m = (int)(a.nchunks - base < 64u ? a.nchunks - base : 64u);
        for (int j = 0; j < m; ++j) acc += D3{__shfl(s.x, j), __shfl(s.y, j), __shfl(s.z, j)};
    }
    if (lane == 0) {
        double* o = a.centers + 3 * (size_t)(a.frame0 + fr);
        const double n = (double)a.npx;
        o[0] = acc.x / n; o[1] = acc.y / n; o[2] = acc.z / n;
    }
}

}  // namespace

static_assert(sizeof(D3) == kViewSumBytes, "the host sizes the chunk sums");

hipError_t launch_view_centers(const ViewCentersArgs& a, hipStream_t s)
{
    hipLaunchKernelGGL(k_view_chunk_sums, dim3(a.nchunks, (unsigned)a.n_frames), dim3(kSumThreads), 0, s, a);
    hipLaunchKernelGGL(k_view_centers, dim3((unsigned)a.n_frames), dim3(64), 0, s, a);
    return hipGetLastError();
}

}  // namespace mdvt
