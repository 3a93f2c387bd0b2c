// mdvt_context.h -- what the host units of the C ABI share: the context (mdvt_ctx), its error text, its device memory (the
// process-wide pools of mdvt_context.hip, the scratch blocks and their one growth rule) and a few facts read off its
// configuration.  Host only: included by mdvt_context.hip, mdvt_api_render.hip, mdvt_api.hip, mdvt_api_depth_engines.hip, mdvt_api_video_mask.hip, mdvt_api_mvsa.hip, mdvt_api_scene.hip, mdvt_api_megasam.hip and mdvt_api_inspatio.hip, never by a unit that defines kernels.
#pragma once

#include "mdvt_internal.h"
#include "mdvt_lanczos_table.h"
#include "mdvt_area_table.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <array>
#include <map>
#include <string>
#include <unordered_map>
#include <vector>

namespace mdvt::host {

constexpr int kParamSlots = 8;        // pinned staging ring for per-frame constants

struct ParamSlot {
    FrameDev* host = nullptr;         // pinned
    FrameDev* dev = nullptr;
    size_t capacity = 0;              // frames
    hipEvent_t done = nullptr;        // H2D copy + the kernels reading it have been submitted/finished
    bool used = false;
};

// A block of device memory that one kind of call sizes for itself and that grows on demand (scratch_reserve).
struct Scratch {
    uint8_t* p = nullptr;
    size_t bytes = 0;                 // what was asked for, not the pool's size class
    template <class T> T* as() const { return reinterpret_cast<T*>(p); }
};

// The context's scratch blocks, in the order mdvt_destroy hands them back to the pool.
enum ScratchId {
    SCR_ROW_COUNTS,                   // hole counts: [frames][2][H] u32
    SCR_WAVE_COUNTS,                  //              [frames][H][16] u32 (RenderArgs.wave_counts)
    // multisampled render (mdvt_config.samples = 4): the sample key planes of the frames in flight, [slot][eye][H*W][4] u64
    SCR_MSAA_KEYS,
    // near-plane clipping (mdvt_set_near_clip; mdvt_near_clip.hip).  With samples = 4 it uses SCR_MSAA_KEYS; single-sample: the key
    // planes of the frames in flight, [slot][eye][H*W] u64, and one u32 flag per slot and eye (an eye where some triangle straddles the plane)
    SCR_CLIP_KEYS, SCR_CLIP_FLAGS,
    // infill-mask completion (mdvt::TeleaWorkspace): per image stamp u16 + T f32 + work image u8x3 + need u8 + nlist u32, the level
    // counters (sized by max_rounds) and the per-image counters of a full pass
    SCR_TELEA_STAMP, SCR_TELEA_T, SCR_TELEA_IMG, SCR_TELEA_NEED, SCR_TELEA_NLIST, SCR_TELEA_COUNTS, SCR_TELEA_REMAINING, SCR_TELEA_LAST_ROUND,
    // infill-mask completion in the heap order: one block of mdvt::telea_heap_image_bytes per image of a pass, + remaining
    SCR_HEAP_WS, SCR_HEAP_REMAINING,
    SCR_NI,                           // normal_infill / infill_using_mask_normals / model_infill_finish (at its own size): about 16 B/px per image in flight
    SCR_FFV1,                         // mdvt_encode_video_frames: the running packet offset, then per slice of a pass its size word and scratch
    SCR_FFV1_DEC,                     // mdvt_decode_video_frames: per slice of a pass its offset, payload bytes and cell claim
    SCR_CONV,                         // mdvt_convergence_depths: per frame of a launch set its chunk sums; with a mask also the ballot words, codes and unit counts
    SCR_FIT,                          // mdvt_scale_shift_fit: the running totals (32 B), then per chunk of a launch set its five sums
    SCR_ADAPTER,                      // mdvt_adapter_composite_eye: the listed-pixel workspace of one eye-sized image, its marks image, grown plane and row-blurred plane
    SCR_FFV1_STREAM,                  // mdvt_decode_video_stream: per slice of the call its offset, payload bytes and cell claim, per frame its kind
    SCR_VIEW,                         // mdvt_view_centers: per frame of a launch set its chunk sums (24 B per 8192 vertices); parking: also the edge filter's vertex flags (1 B/px)
    SCR_GEOMETRY,                     // mdvt_export_geometry_batch: per frame of a launch set the filter's triangle flags (2 B per cell) and the compaction's workgroup totals (4 B per 256 triangles / vertices)
    SCR_FOCAL,                        // mdvt_focal_from_points: per frame of a launch set the selected values of both axes (8 B per point), their chunk sums, unit counts and offsets
    SCR_LANCZOS_TABLES,               // include/mdvt_video_mask.h: the resampler's bounds and coefficient tables of the latest size pair (ctx->lanczos_resident)
    SCR_MASK_WS,                      // include/mdvt_video_mask.h: per frame of a launch set the intermediate image of the two-launch form, the resized frame or byte plane, the frame's maximum, table or minimum and maximum
    SCR_MVSA,                         // mdvt_ratio_median: per frame of a launch set the 256 histogram words of a radix pass and the selection's state (1040 B)
    SCR_AREA_TABLES,                  // include/mdvt_megasam.h: the area resize's first, count and weight tables of the latest size pair (ctx->area_resident)
    SCR_INSPATIO,                     // mdvt_masked_shift_grid: 64 B per cell of the call, the largest rounding distance, then per interior cell of a launch set three complex float64 planes
    SCR_COUNT
};

}  // namespace mdvt::host

struct mdvt_ctx {
    int device = 0;
    int pool_tag = 0;                 // the GPU whose pooled workspace blocks this context may take (= device; tuning build: MDVT_POOL_TAG)
    int W = 0, H = 0;
    mdvt_config cfg{};
    bool cfg_set = false;
    std::string err;
    mdvt::host::ParamSlot slots[mdvt::host::kParamSlots];
    int next_slot = 0;
    // the most recently staged parameter block: clips with constant parameters re-use the device copy
    std::vector<mdvt::FrameDev> last_staged;
    mdvt::host::ParamSlot* last_slot = nullptr;
    hipStream_t last_stream = nullptr;
    // workspace for the general path / edge filter, sized for ws_frames frames (ensure_workspace, mdvt_api_render.hip)
    int ws_frames = 0;
    int ws_eyes = 0;                  // eyes the per-eye planes (z keys, edge keys, tie side words) are allocated for: 1 after view renders only
    bool ws_keys = false, ws_ekeys = false, ws_edges = false;
    unsigned long long* keys[2] = {nullptr, nullptr};
    unsigned long long* ekeys[2] = {nullptr, nullptr};
    uint32_t* elist = nullptr;        // written edge-key words per (slot, source row) + counters (behind the entries)
    unsigned long long* cbuf[2] = {nullptr, nullptr};
    bool ws_mesh = false;
    bool keys_dirty = false;          // a general-path submission was interrupted between splat and resolve
    bool eye1_stale = false;          // view renders have flipped the slots' parity without touching eye 1's z keys: the next stereo render resets the planes first
    uint32_t key_parity = 0;          // bit s: parity of the next use of z-key slot s (mdvt_device.h, parity scheme)
    uint8_t* tri_invalid = nullptr;
    uint8_t* unused = nullptr;
    uint32_t* bigq = nullptr;         // general mesh path: queue of large triangles + its counter (last dword)
    size_t bigq_bytes = 0, bigq_counters_at = 0;      // the queue block as laid out (without tuning padding), the dword offset of its counters
    int huge_lists = 1;               // huge lists inside the queue block (2: tuning layout "joint")
    mdvt::RowCell* rowcell = nullptr; // [H] scanline -> cell row table of the mesh grid (pure-shift band kernel)
    int rowcell_bits = 0;             // the sub-pixel grid that table was built for
    uint32_t* divcheck = nullptr;     // [kDivSlots] (RenderArgs.divcheck), zeroed when allocated; slot k belongs to div_keys[k]
    std::vector<std::array<uint32_t, 3>> div_keys;      // bits of (mult, scale, dl) of the parameter sets checked so far
    hipEvent_t div_done = nullptr;    // recorded after the latest division check (every earlier check and the table's fill before it) ...
    hipStream_t div_stream = nullptr; // ... on this stream: a render on another stream waits for it before it reads the table
    // the blocks that grow on demand (scratch_reserve), by ScratchId
    mdvt::host::Scratch scratch[mdvt::host::SCR_COUNT];
    bool msaa_dirty = false;          // a submission stopped between raster and resolve: the planes of SCR_MSAA_KEYS are not all empty
    bool clip_dirty = false;          // likewise SCR_CLIP_KEYS
    int32_t near_clip = 0;            // mdvt_set_near_clip
    uint32_t* telea_levels_host = nullptr;      // pinned: the deepest level of a pass of the infill-mask completion, read back once per pass
    // edge_row_range() of the most recent camera matrix (a clip's frames mostly share it)
    double erow_key[5] = {0, 0, 0, 0, 0};
    int erow_val[3] = {0, 0, 0};
    bool erow_cached = false;
    // every device allocation the context owns, by size (mdvt_workspace_bytes)
    std::unordered_map<void*, size_t> allocs;
    size_t ws_bytes = 0;
    bool opt_mesh_conv = false;       // MDVT_MESH_CONV=1 in the environment of mdvt_create (the opt-in kernel of mdvt_mesh_conv.hip)
    // posed / converged mesh runs of more than one launch set: the sets alternate between the caller's stream and this one, each on
    // its own half of the workspace slots (mdvt_render_stereo_batch); made on first use
    hipStream_t side = nullptr;
    uint32_t* hugeq2 = nullptr;
    hipEvent_t ev_start = nullptr, ev_join = nullptr, ev_vert[2] = {nullptr, nullptr};
    // Pillow's Lanczos tables (mdvt_api_video_mask.hip): built once per (in, out) pair and kept on the host; the pairs whose tables
    // SCR_LANCZOS_TABLES holds on the device: (in_w, out_w, in_h, out_h), all 0 = none
    std::map<std::pair<int, int>, mdvt::host::LanczosTable> lanczos_tables;
    int lanczos_resident[4] = {0, 0, 0, 0};
    // cv2's area tables (mdvt_api_megasam.hip), kept and uploaded by the same rule: SCR_AREA_TABLES, (in_w, out_w, in_h, out_h)
    std::map<std::pair<int, int>, mdvt::host::AreaTable> area_tables;
    int area_resident[4] = {0, 0, 0, 0};
};

namespace mdvt::host {

// Records the error text (of the context, or of the calling thread when there is none: mdvt_create) and returns `code`.
int fail(mdvt_ctx* c, int code, const char* fmt, ...);

#define MDVT_HIP(c, call)                                                                         \
    do {                                                                                          \
        hipError_t e_ = (call);                                                                   \
        if (e_ != hipSuccess) return fail((c), MDVT_ERR_HIP, "%s failed: %s", #call, hipGetErrorString(e_)); \
    } while (0)

struct DeviceGuard {
    int prev = -1;
    explicit DeviceGuard(int dev) { if (hipGetDevice(&prev) != hipSuccess) prev = -1; if (prev != dev) (void)hipSetDevice(dev); else prev = -1; }
    ~DeviceGuard() { if (prev >= 0) (void)hipSetDevice(prev); }
};

// The render launchers exist once per sub-pixel grid (mdvt_internal.h); a context uses the set of its mdvt_config.subpixel_bits.
inline int grid_bits(const mdvt_ctx* c) { return c->cfg.subpixel_bits == 4 ? 4 : 8; }
#define MDVT_GRID_CALL(c, fn, ...) (grid_bits(c) == 4 ? mdvt::grid4::fn(__VA_ARGS__) : mdvt::grid8::fn(__VA_ARGS__))

inline uint32_t packed_key_rgb(const mdvt_ctx* c) { return (uint32_t)c->cfg.key_rgb[0] | ((uint32_t)c->cfg.key_rgb[1] << 8) | ((uint32_t)c->cfg.key_rgb[2] << 16); }
inline size_t workspace_budget_bytes(const mdvt_ctx* c) { return (size_t)(c->cfg.workspace_mib ? c->cfg.workspace_mib : 4096u) << 20; }
// the slots of per_slot bytes each that the budget affords: at least one, at most cap
inline int slots_afforded(const mdvt_ctx* c, size_t per_slot, int cap)
{
    const size_t afford = workspace_budget_bytes(c) / per_slot;
    return (size_t)cap > afford ? (afford < 1 ? 1 : (int)afford) : cap;
}

// ---- the entry points' vocabulary for layouts, launch sets and scratch blocks --------------------------------------------------
// What a vector path asks of an array: every pointer, pitch, stride (or row length) listed is a multiple of k.
template <class... A> bool multiples_of(size_t k, A... a) { return (((uintptr_t)a % k == 0) && ...); }
constexpr size_t up16(size_t v) { return (v + 15) & ~(size_t)15; }
constexpr int kGridFrames = 32768;    // frames of one launch where a grid's second or third dimension holds them
// the frames of the launch set that starts at frame f0 of n, cap at the most
inline int set_len(int n, int f0, int cap) { return n - f0 < cap ? n - f0 : cap; }
// carves a scratch block: the next `bytes` bytes from w on as T*; w moves behind them (the caller rounds where its layout does)
template <class T> T* take(uint8_t*& w, size_t bytes)
{
    T* p = reinterpret_cast<T*>(w);
    w += bytes;
    return p;
}

// ---- mdvt_context.hip: the process-wide pools (their reasons are told there) -------------------------------------------------
// device memory owned by a context, accounted for mdvt_workspace_bytes; `s`: the stream the fresh-block fill goes to
hipError_t ws_malloc(mdvt_ctx* c, void** p, size_t bytes, hipStream_t s);
// (the caller has made sure no submitted work still uses the block; takes a null pointer)
void ws_free(mdvt_ctx* c, void* p);
// The growth rule of every scratch block, stated here once.
//  - bytes >= need: nothing happens.  A scratch block never shrinks.
//  - Otherwise a block that is held goes back first: hipDeviceSynchronize (earlier submissions, on any stream, may still use it, and
//    the pool may hand it to another context at once), then ws_free.  The old block leaves before the new one is taken, so the
//    peak is the new size.  With no block held there is nothing to wait for and nothing is synchronised (six of the nine call
//    sites this rule replaced synchronised the device on their first call too): ws_malloc fills a fresh block and synchronises
//    the stream for it, and a recycled block was synchronised when it was freed.
//  - Then ws_malloc(need).  On failure the Scratch is {nullptr, 0} and the error is returned; only on success bytes = need
//    and *grew = true (the caller's cue to re-establish what the block has to hold between calls).
hipError_t scratch_reserve(mdvt_ctx* c, Scratch& b, size_t need, hipStream_t s, bool* grew = nullptr);
// A pinned host block of at least `bytes`, with a device block of the same size on GPU `device` if with_dev.
hipError_t pool_take(size_t bytes, bool with_dev, int device, void** host, void** dev, size_t* got);
void pool_give(void* host, void* dev, size_t bytes, int device);
// idle blocks of the two pools as GPU `tag` sees them: parameter blocks with device memory of this / another GPU, workspace blocks of this / another
void pool_idle_blocks(int tag, uint64_t counts[4]);
// the banks' side stream and events into the context (process-wide, never destroyed)
hipError_t bank_res_take(mdvt_ctx* c);

}  // namespace mdvt::host
