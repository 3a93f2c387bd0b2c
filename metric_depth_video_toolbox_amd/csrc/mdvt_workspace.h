// mdvt_workspace.h -- the layout of the render workspace (general path / edge filter), stated once for ensure_workspace, bind_workspace
// and mdvt_debug_read (mdvt_api_render.hip) and launch_mesh_raster_general.  Plain C++17 without HIP: tests/workspace_layout_host.cpp checks it.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace mdvt {
constexpr int kTieTile = 32;          // pixels: side of the tiles whose "holds a pixel marked as tied" bits gate the second rasteriser pass of the general mesh path
inline size_t tie_words_of(int W, int H) { return ((size_t)((W + kTieTile - 1) / kTieTile) * (size_t)((H + kTieTile - 1) / kTieTile) + 31) / 32; }
constexpr int kHugeCap = 1 << 17;     // row-block entries of huge triangles per launch set (overflow: the queue kernel keeps the triangle)
constexpr int kBigRecDwords = 2;      // a queued triangle: draw id, frame slot << 1 | eye
// What the workspace budget (mdvt_config.workspace_mib) divides by, per pixel and slot of the general mesh path: 16 B of z keys, 16 B
// of tie side words, 32 B of triangle queue; with edge points 28 B of edge keys, their list and the vertex list; with edge removal
// 3 B of filter flags.  The budget's contract (include/mdvt.h; tests restate it), deliberately not the exact sizes below.
constexpr size_t kNominalSlotBytesPerPx = 16 + 16 + 32, kNominalEdgePointBytesPerPx = 28, kNominalEdgeFlagBytesPerPx = 3;
inline size_t nominal_slot_bytes(int W, int H, bool edge_points, bool remove_edges)
{
    return (size_t)W * (size_t)H * (kNominalSlotBytesPerPx + (edge_points ? kNominalEdgePointBytesPerPx : 0) + (remove_edges ? kNominalEdgeFlagBytesPerPx : 0));
}
// Queue entry indices are 32-bit, a slot has 4 entries per pixel: the slots one queue serves; chunk_of gives a launch set no more (0: frame too large).
inline size_t queue_slots_max(int W, int H) { return (size_t)0xFFFFFFF0u / (4 * (size_t)W * (size_t)H); }
// A launch set's n H segment counters, then its coarse sums: a word per block of 2^bigq_shift segments and one more, at most n H + 1.
inline size_t queue_coarse_at(int n, int H) { return (size_t)n * (size_t)H; }
// The workspace of `slots` frame slots of a W x H context.  Sizes in bytes; `_at` offsets and strides in elements of their buffer.
struct RenderWorkspaceLayout {
    size_t W, H, slots, huge_lists;   // huge_lists: huge lists inside the queue block (2: tuning layout "joint")
    size_t npx, ntri, tie_words;      // npx: also the slot stride of keys, ekeys, cbuf, vlist, unused; ntri: of tri_invalid
    RenderWorkspaceLayout(int W_, int H_, int slots_, int huge_lists_)
        : W((size_t)W_), H((size_t)H_), slots((size_t)slots_), huge_lists((size_t)huge_lists_), npx(W * H), ntri(2 * (W - 1) * (H - 1)),
          tie_words(tie_words_of(W_, H_)) {}
    size_t plane_bytes() const { return slots * npx * sizeof(unsigned long long); }      // per eye: z keys, edge keys or tie side words
    size_t tri_invalid_bytes() const { return slots * ntri; }
    size_t unused_bytes() const { return slots * npx; }
    // the elist block (dwords): per slot the edge-key list (2 W entries per source row; slot stride 2 npx), its counters (one per slot
    // and source row), the vertex list of the mesh path's edge-point splat (npx entries per slot), that list's counters (one per slot)
    size_t elist_stride() const { return 2 * npx; }
    size_t elist_count_at() const { return slots * elist_stride(); }
    size_t vlist_at() const { return elist_count_at() + slots * H; }
    size_t vlist_count_at() const { return vlist_at() + slots * npx; }
    size_t elist_bytes() const { return (vlist_count_at() + slots) * sizeof(uint32_t); }
    // the queue block (dwords): one segment per (frame slot, cell row) with room for all four triangles of every cell of the row and
    // its own counter -- the queue cannot overflow; then the huge triangles' row blocks + their counters, the tie flags, the tile bits
    size_t queue_slots() const { const size_t m = queue_slots_max((int)W, (int)H); return m < slots ? m : slots; }
    size_t bigq_cap() const { return queue_slots() * npx * 4; }                 // entries; allocation and counter offset use this ONE value
    size_t queue_stride() const { return 4 * npx * kBigRecDwords; }             // per slot
    size_t counters_at() const { return bigq_cap() * kBigRecDwords; }
    // Counters and coarse sums: a set of n frames takes 2 n H + 1 words.  Two banks of b slots, 2 b <= slots: bank 1 starts behind
    // bank 0's words -- "+ 2": the word by which they pass 2 b H and one of plain slack, "+ 3 & ~3": rounded up to 16 bytes, at most
    // 2 b H + 4 -- and ends at most 4 b H + 5 <= 2 slots H + 5 words in: "+ 8" holds that and keeps the huge list 8-byte aligned (uint2).
    size_t counter_words() const { return 2 * slots * H + 8; }
    size_t bank_counters_at(int bank, int bank_slots) const { return (size_t)bank * ((2 * (size_t)bank_slots * H + 2 + 3) & ~(size_t)3); }
    size_t huge_at() const { return counters_at() + counter_words(); }
    static constexpr size_t huge_list_dwords() { return 2 * (size_t)kHugeCap + 2; }     // entries, counter, overflow slack (also the second bank's own list)
    size_t tie_flag_at() const { return huge_at() + huge_lists * huge_list_dwords(); }
    size_t tie_tiles_at() const { return tie_flag_at() + slots; }
    size_t tie_tiles_stride() const { return 2 * tie_words; }                   // per slot
    size_t queue_bytes() const { return (tie_tiles_at() + slots * tie_tiles_stride()) * sizeof(uint32_t); }     // without tuning padding
};
}  // namespace mdvt
