// mdvt_pairwise.h -- NumPy's float32 order of summation as device code over a value functor: what mdvt_convergence.hip (per-frame
// means) and mdvt_metric_align.hip (the five sums of the scale-and-shift fit) share.  include/mdvt_convergence.h states the order.
// The order is the same for every element type (the ufunc buffer counts elements): mdvt_view.hip instantiates the routines on a
// triple of doubles (the three coordinate sums of a frame's vertices, which share one walk); T = float is what the names without
// a template argument mean.
//
// A sum of n contiguous values runs in consecutive chunks of kChunk (the ufunc buffer), each summed by the pairwise routine
// pw(a, n) -- n < 8: in order; n <= kLeaf: eight strided accumulators, ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7)), then the last n % 8 in
// order; else pw(a, n2) + pw(a + n2, n - n2) with n2 = n / 2 rounded down to a multiple of 8 -- and the chunk sums are added one
// after the other.  A full chunk is a balanced tree over 64 leaves of 128 values: the units build it themselves from butterfly
// steps (IEEE add is commutative: both sides of a step hold the same bits).  A shorter chunk has at most 128 leaves at depths of at
// most 7 and is walked in the general shape below by one workgroup of at least 128 threads.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mdvt {
namespace pairwise {

constexpr int kChunk = 8192;          // NumPy's ufunc buffer, in elements
constexpr int kLeaf = 128;            // the pairwise routine's block

// pw for n <= kLeaf values v(i0) .. v(i0 + n - 1)
// (T: float, or a type with T(), operator+ and += that adds like its scalar, element by element; T() is zero)
template <class T, class V>
__device__ T leaf_sum_t(const V& v, int i0, int n)
{
    if (n < 8) {
        T r = T();
        for (int i = 0; i < n; ++i) r += v(i0 + i);
        return r;
    }
    T r[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) r[k] = v(i0 + k);
    int i = 8;
    for (; i < n - (n % 8); i += 8) {
#pragma unroll
        for (int k = 0; k < 8; ++k) r[k] += v(i0 + i + k);
    }
    T res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
    for (; i < n; ++i) res += v(i0 + i);
    return res;
}
template <class V>
__device__ float leaf_sum(const V& v, int i0, int n) { return leaf_sum_t<float>(v, i0, n); }

// The general shape of a chunk of n <= kChunk values, in LDS: its leaves from left to right with their depths in the tree.
template <class T>
struct ShapeT {
    T leaf_sum[128], val[16];
    uint16_t leaf_at[128], leaf_n[128], at[16], n[16];
    uint8_t leaf_depth[128], depth[16];
    int leaves;
};
using Shape = ShapeT<float>;

// One thread lists the leaves (a stack of at most 8 pending right halves); the workgroup synchronises before it reads them.
template <class T>
__device__ inline void shape_list(ShapeT<T>& s, int n)
{
    int sp = 0, nl = 0;
    s.at[0] = 0; s.n[0] = (uint16_t)n; s.depth[0] = 0; sp = 1;
    while (sp > 0) {
        --sp;
        const int at = s.at[sp], m = s.n[sp], d = s.depth[sp];
        if (m <= kLeaf) {
            s.leaf_at[nl] = (uint16_t)at; s.leaf_n[nl] = (uint16_t)m; s.leaf_depth[nl] = (uint8_t)d;
            ++nl;
        } else {
            int m2 = m / 2;
            m2 -= m2 % 8;
            s.at[sp] = (uint16_t)(at + m2); s.n[sp] = (uint16_t)(m - m2); s.depth[sp] = (uint8_t)(d + 1);
            s.at[sp + 1] = (uint16_t)at; s.n[sp + 1] = (uint16_t)m2; s.depth[sp + 1] = (uint8_t)(d + 1);
            sp += 2;
        }
    }
    s.leaves = nl;                                               // at most 128: a leaf of a split node holds at least 64 values
}

// A thread each sums the listed leaves (tid < 128 suffices); the workgroup synchronises before shape_join.
template <class T, class V>
__device__ inline void shape_leaves(ShapeT<T>& s, const V& v, int tid)
{
    if (tid < s.leaves) s.leaf_sum[tid] = leaf_sum_t<T>(v, s.leaf_at[tid], s.leaf_n[tid]);
}

// One thread joins neighbours of equal depth, which is the tree: every inner node has two children.  -> the chunk's sum.
// leaf_sum: the sums of the listed leaves; val, depth: a stack of 16 entries.  With leaf sums and stacks of their own, several
// sums over one shape are joined side by side, a thread each.
template <class T>
__device__ inline T shape_join(const ShapeT<T>& s, const T* leaf_sum, T* val, uint8_t* depth)
{
    int sp = 0;
    for (int j = 0; j < s.leaves; ++j) {
        val[sp] = leaf_sum[j]; depth[sp] = s.leaf_depth[j];
        ++sp;
        while (sp >= 2 && depth[sp - 1] == depth[sp - 2]) {
            val[sp - 2] = val[sp - 2] + val[sp - 1];
            --depth[sp - 2];
            --sp;
        }
    }
    return val[0];
}

template <class T>
__device__ inline T shape_join(ShapeT<T>& s) { return shape_join(s, s.leaf_sum, s.val, s.depth); }

}  // namespace pairwise
}  // namespace mdvt
