// mdvt_internal.h -- shared between the C-ABI host code (mdvt_context.hip, mdvt_api_render.hip, mdvt_api.hip; what only they
// share is mdvt_context.h) and the kernel translation units (the other *.hip).  Not part of the public interface (that is include/mdvt.h).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>

#include "mdvt.h"
#include "mdvt_workspace.h"

namespace mdvt {

// Tuning / ablation / test hooks.  The PRODUCT library (libmdvt_hip.so) has none: tuning_env() is `return nullptr` there
// (mdvt_tuning_off.hip) and not even the hooks' names are in the binary; its one opt-in switch, MDVT_MESH_CONV, is read
// once, in mdvt_create.  `make tuning` links the same objects with mdvt_tuning_on.hip into libmdvt_hip_tuning.so, where
// tuning_env(TUNE_X) is getenv("MDVT_X"), re-read per launch: that library is what tools/ and the tests that force a kernel
// family load (MDVT_LIB_VARIANT=tuning, _lib.py).  Some hooks change results by design (MDVT_DEBUG_SKIP bits 0-4, MDVT_NI_SKIP).
enum TuneKey { TUNE_BLUR_ONE_PASS, TUNE_DEBUG_SKIP, TUNE_EDGE_INBAND, TUNE_FORCE_GLOBAL, TUNE_LDS_PAD, TUNE_MESH_BAND, TUNE_MESH_BAND3, TUNE_MESH_CONV, TUNE_MESH_OLD, TUNE_MESH_TPB, TUNE_NI_DUMP, TUNE_NI_SKIP, TUNE_PARAM_UPLOAD, TUNE_POINTS_CFG, TUNE_POINTS_NT, TUNE_POOL_TAG, TUNE_QUEUE_DUMP, TUNE_RASTER_CONV_OFF, TUNE_TELEA_BLOCKS, TUNE_TELEA_DUMP, TUNE_WS_CHUNK, TUNE_WS_FRESH, TUNE_WS_LAYOUT, TUNE_WS_PAD, TUNE_WS_POOL, TUNE_COUNT };
const char* tuning_env(TuneKey k);
bool tuning_build();
// The ablation hooks inside the kernels (RenderArgs.debug_skip, NormalInfillArgs.debug_skip) exist in the objects of the tuning
// library only (-DMDVT_TUNING, Makefile): the product kernels are compiled with the constant 0 and carry no such test.
#ifdef MDVT_TUNING
#define MDVT_DEBUG_SKIP(a) ((a).debug_skip)
#else
#define MDVT_DEBUG_SKIP(a) 0
#endif

// Near plane of the reference's render call: ctr.set_constant_z_near(0.0001) (dmt:1520).
constexpr float kNear = 1e-4f;
// Rasteriser sub-pixel grid (GL_SUBPIXEL_BITS) and the clamp applied before snapping (DESIGN.md "Arithmetic decree").
// The rasterising translation units are compiled once per supported grid (Makefile): 8 bits, what desktop GPUs report
// and the default of mdvt_config.subpixel_bits, and 4 bits, the grid of the GL the fixtures of tests/golden/render_gl_*.npz
// were rendered with.  Everything they define lives in namespace mdvt::MDVT_GRID; the host code picks per context (MDVT_GRID_CALL).
#ifndef MDVT_SUBPIX_BITS
#define MDVT_SUBPIX_BITS 8
#endif
#if MDVT_SUBPIX_BITS == 8
#define MDVT_GRID grid8
#elif MDVT_SUBPIX_BITS == 4
#define MDVT_GRID grid4
#else
#error "MDVT_SUBPIX_BITS must be 4 or 8"
#endif
constexpr int kSubpixBits = MDVT_SUBPIX_BITS;
constexpr int kSubpix = 1 << kSubpixBits;
constexpr float kSnapLimit = 2097152.0f;   // 2^21 px: snapped coordinates fit int32, differences too

// Per-frame constants, derived on the host in f64 and rounded once (see fill_frame_dev()).
struct FrameDev {
    float mult;          // f32(max_depth / 255^4)                          dfh:22
    float scale;         // f32(master_fov_scale_depth)                     sr:541
    float dl;            // f32(Krender.fx * ipd/2): pure-shift disparity numerator
    float fx, fy, cx, cy;        // input camera (f32)
    float fxr, fyr, cxr, cyr;    // render camera (f32)
    float sx, sy;        // (W+1)/W, (H+1)/H in f32 for the mesh grid, 1 for points   dmt:1117-1122
    float sW, sH;        // (W-1)/W, (H-1)/H in f32: the pure-shift column estimate of an edge point (edge_col_pure)
    int32_t general;     // 0: pure +-ipd/2 shift, 1: pose / convergence / K != Krender
    int32_t conv_band;   // general, but nothing except a toe-in about the y axis small enough for k_mesh_conv (mdvt_mesh_conv.hip)
    float M[2][12];      // per eye 3x4 = Translate(+-ipd/2) * Ry(-+a) * T, f32       sr:615-619, 724-725, 832-836
    double Kd[4];        // fx, fy, cx, cy in f64 for the 89-degree edge filter       dmt:1127-1128, 1283-1294
    double rKd[2];       // 1/fx, 1/fy in f64: the edge filter's screening pass only (never the exact path)
    // The edge points' f64 chain (mdvt_device.h "edge points"): the operands of the reference's own operations
    // (sr:599-600, 615-619, 727-732, 838-847; dmt:1058) -- nothing composed, nothing pre-multiplied.
    double sWd, sHd;     // (W-1)/W, (H-1)/H                                          sr:599-600
    double hd;           // ipd/2 (the translate of sr:731, 839, 846)
    double Td[16];       // the pose, row major (has_T)                               sr:615-619
    double cs[2];        // cos, sin of the convergence angle (has_conv)             sr:719-722
    int32_t has_T, has_conv;
    // pure-shift frames: an edge point of source row i lands on row i except for i in [erow_lo, erow_hi), where it lands on
    // i or i + 1 (which of the two the chain decides per point); the LDS row kernels leave the edge points of scanlines
    // erow_lo .. erow_hi to k_edge_rows_exact.  erow_wild: some row's offset is neither (a camera matrix with cy far
    // from H/2): the frame is rendered by the global-key kernels, whose edge points take the whole chain.
    int32_t erow_lo, erow_hi, erow_wild;
    // pure-shift point frames: index of this frame's (mult, scale, dl) in the context's table of division checks (RenderArgs.divcheck), -1:
    // none.  The disparity dl / z of a frame has 65535 possible operands z -- the depth codes --: k_divcheck has tried all of them, and
    // where the 4-instruction sequence (v_rcp_f32, one multiply, two fma) gave the bits of the IEEE division every time the counter is 0
    // and the row kernel takes it instead of the 10-instruction expansion.
    int32_t div_slot;
};

// Which row of grid cells covers output scanline k of a pure-shift mesh frame, and that row's snapped extent (depends on
// H and the grid scale only: one table per context, built on the host with the decree's own f32 operations).
struct RowCell { int32_t c, Yt, Yb, pad; };     // c = -1: the scanline lies below the last vertex row

struct RenderArgs {
    const uint8_t* depth; size_t depth_pitch, depth_stride;
    const uint8_t* color; size_t color_pitch, color_stride;
    uint8_t* rgb[2];  size_t rgb_pitch, rgb_stride;
    uint8_t* mask[2]; size_t mask_pitch, mask_stride;
    float* zout[2];   size_t zout_pitch, zout_stride;
    uint8_t* maskbits[2]; size_t maskbits_pitch, maskbits_stride;   // optional 1 bit/px hole mask
    uint32_t* hole_counts;       // optional [n_frames][2]
    uint8_t* seed[2]; size_t seed_pitch, seed_stride;            // optional infill-mask seed images
    uint32_t* row_counts;        // workspace [frames in launch][2][H], zeroed per launch (when hole_counts)
    const uint32_t* divcheck;    // [kDivSlots] mismatches of the short division per parameter set (FrameDev.div_slot); 0 = proven
    uint32_t* wave_counts;       // workspace [frames in launch][H][16]: the fused points kernel's hole counts per wave (left | right << 16)
    const FrameDev* fp;          // device array, one per frame of the batch
    int32_t W, H;
    int32_t frame0;              // first frame of this launch within the batch
    uint32_t key_rgb;            // R | G<<8 | B<<16
    // workspace (general path / edge filter); per frame-in-flight slices
    unsigned long long* keys[2]; // [slot][H*W] 64-bit z keys per eye (parity scheme: mdvt_device.h)
    uint32_t key_parity;         // bit s = parity of slot s in this launch
    unsigned long long* ekeys[2];// edge-point keys per eye
    uint32_t* elist;             // the edge-key words written since the last resolve, one segment of 2 W entries (eye << 31 | pixel) per
    uint32_t* elist_count;       //   (slot, source row) and its counter: k_edge_keys_reset empties exactly those words
    uint32_t* vlist;             // mesh, general path: the vertices of removed triangles of a slot's frame as a list (source row << 16 | column),
    uint32_t* vlist_count;       //   [slot][H*W] entries + [slot] counters: what k_edge_points_splat_list runs the f64 chain over
    unsigned long long* cbuf[2]; // general mesh path: per-eye side words of the pixels with an exact depth tie between colours (draw id << 32 | rgb,
                                 //   minimum over the fragments at the winning depth); touched at those pixels only
    uint32_t* tie_flag;          // [slot]: a pixel of the slot's frame was marked as tied in this use (zeroed per launch set)
    uint32_t* tie_tiles;         // [slot][2][tie_words]: bit per kTieTile x kTieTile tile of an eye holding a marked pixel (zeroed per launch set)
    int32_t tie_words, tie_tiles_x;
    uint8_t* tri_invalid;        // [slot][2*(H-1)*(W-1)]
    uint8_t* unused;             // [slot][H*W]
    // general mesh path: queue of the triangles that are not small (kBigRecDwords dwords each), rasterised by k_mesh_raster_queue
    uint32_t* bigq; uint32_t* bigq_count; uint32_t bigq_cap;
    uint32_t* bigq_coarse;       // [(segments >> bigq_shift) + 1] queued triangles per block of 2^bigq_shift segments (behind the segment counters;
    int32_t bigq_shift;          //   set by launch_mesh_raster_general): the queue walk's first search level, summed up in LDS
    uint32_t* hugeq;             // [kHugeCap] x 2 dwords + counter + overflow slack: row blocks of the queued triangles too large for 16 lanes (k_mesh_raster_huge)
    size_t ws_stride_px;         // H*W (elements) between slots
    size_t ws_stride_tri;        // 2*(H-1)*(W-1)
    int32_t edge_paint;          // 1: edge points are painted into the holes (sr:813-814); 0: seed image only (--do_basic_infill, sr:809-812)
    const RowCell* rowcell;      // [H], mesh mode
    int32_t cull;                // 0 none, 1 back faces, 2 front faces (mdvt_config.cull)
    int32_t debug_skip;          // ablation hook for tools/kbench.py (env MDVT_DEBUG_SKIP): 1 raster, 2 resolve, 4 staging
};

// launchers of mdvt_formats.hip (codec, zero_bytes) and mdvt_edge_filter.hip; all return hipError_t from hipGetLastError()
hipError_t launch_decode_depth(const uint8_t* rgb, size_t rgb_pitch, float* out, size_t out_pitch, int W, int H,
                               float mult, float scale, hipStream_t s);
hipError_t launch_encode_depth(const float* depth, size_t depth_pitch, uint8_t* rgb, size_t rgb_pitch, int W, int H,
                               double max_depth, int bgr, hipStream_t s);
hipError_t launch_zero_bytes(void* p, size_t bytes, hipStream_t s);
hipError_t launch_edge_filter(const uint8_t* depth_rgb, size_t pitch, size_t stride, const FrameDev* fp, int frame0,
                              int n, int W, int H, int of_by_one, uint8_t* tri_invalid, size_t tri_stride,
                              uint8_t* unused, size_t unused_stride, hipStream_t s);

constexpr int kDivSlots = 256;        // parameter sets (mult, scale, dl) a context keeps division checks for; later ones take the IEEE division
// (kTieTile, tie_words_of, kHugeCap, kBigRecDwords: mdvt_workspace.h)

struct RenderPlan {
    int mode;            // mdvt_mode
    int remove_edges;
    int edge_points;
    int general;         // any frame of the launch needs the general path
    int conv;            // mesh: every frame of the launch is convergence-only (FrameDev.conv_band): k_mesh_conv instead of the global-key kernels
    int conv_raster;     // general mesh path, every frame of the launch convergence-only: k_mesh_raster_conv instead of k_mesh_raster_small
    int vec4;            // W%4==0 and every pointer/pitch 4-byte aligned
    int fused_bits;      // set by launch_render when the render kernel itself produced maskbits / hole_counts
    int n;               // frames in this launch
    int allow_conv;      // MDVT_MESH_CONV=1 when the context was created (mdvt_create): k_mesh_conv may take convergence-only frames
    int edge_rows_max;   // pure-shift launches with edge points: the most scanlines any frame leaves to k_edge_rows_exact (0: none)
    int eyes;            // 1: a view render (mdvt_render_view_batch) -- eye 0 only, general path, holes keep the key colour, RenderArgs.hole_counts is [n_frames]; else both eyes
    hipEvent_t after_vertices;   // general paths: recorded on the launch's stream behind the first pass (the mesh's cell walk, the points' splat; nullptr: none)
};
// mdvt_msaa.hip: the opt-in 4x multisampled render (mdvt_config.samples = 4), one launch set of frames [frame0, frame0 + n).
struct MsaaArgs {
    const uint8_t* depth; size_t depth_pitch, depth_stride;
    const uint8_t* color; size_t color_pitch, color_stride;
    uint8_t* rgb[2];  size_t rgb_pitch, rgb_stride;
    uint8_t* mask[2]; size_t mask_pitch, mask_stride;
    uint32_t* hole_counts;       // optional [n_frames][2], zeroed by the caller before the first launch set
    const FrameDev* fp;          // device array, one per frame of the batch
    unsigned long long* keys;    // [slot][eye][H*W][4 samples]: ~bits(1/Z) << 32 | draw id, all ones = empty (left empty again by the resolve)
    const uint8_t* tri_invalid;  // [slot][2*(H-1)*(W-1)] or nullptr (no edge removal)
    const uint8_t* unused;       // [slot][H*W] or nullptr
    size_t ws_stride_px, ws_stride_tri;
    int32_t W, H;
    int32_t frame0;              // first frame of this launch set within the batch
    int32_t mode, cull, pattern, resolve;     // mdvt_config: mode, cull, sample_pattern, sample_resolve
    uint32_t key_rgb;            // R | G<<8 | B<<16
};
// The rasterising translation units (mdvt_points_edge_rows.hip, mdvt_general_paths.hip, mdvt_mesh_*.hip, mdvt_msaa.hip, mdvt_near_clip.hip)
// and launch_render's dispatch (mdvt_render_dispatch.hip) are compiled once per sub-pixel grid;
// what they define is declared in mdvt_grid_decls.h, once per grid namespace (below, after the shared declarations).
// (mdvt_normal_infill.hip; workspace: normal_infill_workspace_bytes(1, W, H))
hipError_t launch_infill_normals(const uint8_t* color, size_t color_pitch, const uint8_t* hole, size_t hole_pitch,
                                 const float* normal, size_t normal_pitch, uint8_t* out, size_t out_pitch, int W, int H,
                                 int max_steps, uint8_t* workspace, hipStream_t s);
hipError_t launch_mark_lower_side(const uint8_t* img, size_t img_pitch, uint8_t* out, size_t out_pitch, int W, int H,
                                  int max_steps, uint8_t* workspace, hipStream_t s);
// (mdvt_formats.hip)
hipError_t launch_touchly_depth(const float* depth, size_t depth_pitch, uint8_t* rgb, size_t rgb_pitch, int W, int H,
                                float tmax, float tmin, float k, int zero_is_far, hipStream_t s);
hipError_t launch_equirect_remap(const uint8_t* src, size_t src_pitch, size_t src_stride, uint8_t* dst, size_t dst_pitch,
                                 size_t dst_stride, int n, int W, int H, const float* mx, const float* my, hipStream_t s);
// n images addressed as `per_eye` frames x (1 or 2) eyes: image im = frame (im % per_eye) of eye (im / per_eye).
struct ImageSet {
    uint8_t* base; size_t pitch, stride; ptrdiff_t eye_offset; int per_eye;
    __host__ __device__ uint8_t* image(int im) const { return base + (size_t)(im % per_eye) * stride + (ptrdiff_t)(im / per_eye) * eye_offset; }
};

// mdvt_telea_levels.hip: the infill-mask completion in level order and the masked blur behind it
struct TeleaWorkspace {              // per image pixel: stamp u16, T f32, work image u8x3, need u8, nlist u32 (14 B)
    uint16_t* stamp; float* T; uint8_t* img; uint8_t* need; uint32_t* nlist;
    uint32_t* counts;                // [max_rounds + 2], followed by
    uint32_t* offs;                  // [max_rounds + 2] and
    uint32_t* ncounts;               // [max_rounds + 2] x kNcStride words, one counter per cache line (one allocation: telea_counter_words)
    uint32_t* remaining;             // [images]
    uint32_t* last_round;            // [images]
};
constexpr int kTeleaMaxImages = 32;  // images per pass
size_t telea_counter_words(int max_rounds);      // counts + offs + the strided ncounts
hipError_t launch_telea_init(const ImageSet& seed, const TeleaWorkspace& ws, int n, int W, int H, int max_rounds, uint32_t key_rgb,
                             uint32_t* h_levels, hipStream_t s);
hipError_t launch_telea_rounds(const TeleaWorkspace& ws, int W, int H, int levels, uint32_t key_rgb, hipStream_t s);
hipError_t launch_swap_rb(const ImageSet& src, const ImageSet& dst, int n, int W, int H, hipStream_t s);      // (mdvt_formats.hip)
// mdvt_telea_heap.hip: the same completion in the heap order of cv2.inpaint, one workgroup per image (opt-in).  Workspace: one
// block of telea_heap_image_bytes(W, H) per image (44 B/px), the work image at telea_heap_img_offset inside it (pitch 3 W).
constexpr int kTeleaHeapMaxImages = 256;  // images per launch at most (one workgroup each: one per CU)
size_t telea_heap_image_bytes(int W, int H);
size_t telea_heap_img_offset(int W, int H);
hipError_t launch_telea_heap(const ImageSet& seed, uint8_t* ws, size_t image_bytes, uint32_t* remaining, int n, int W, int H,
                             uint32_t key_rgb, hipStream_t s);
struct BlurKernel { float k[36]; };      // masked_blur's 6x6 Gaussian, f32, row major (built on the host in f64)
hipError_t launch_masked_blur(const ImageSet& img, const ImageSet* seed, const ImageSet& out, int n, int W, int H,
                              const BlurKernel& K, uint32_t key_rgb, hipStream_t s, uint32_t* list = nullptr, uint32_t* count = nullptr);
// mdvt_normal_infill.hip: basic_nomal_infill.normal_infill for n images (workspace: normal_infill_workspace_bytes)
size_t normal_infill_workspace_bytes(int n, int W, int H);
hipError_t launch_normal_infill(const ImageSet& img, const ImageSet& mask, const ImageSet& out, uint8_t* workspace, int n, int W, int H,
                                const BlurKernel& K, hipStream_t s);
hipError_t launch_infill_mask_normals(const ImageSet& img, const ImageSet& hole, const ImageSet& mask, uint8_t* workspace, int n, int W, int H,
                                      int max_steps, hipStream_t s);
// the tail of normal_infill behind a model's dense image (mdvt_model_infill_finish, include/mdvt_infill_engines.h); workspace as above
hipError_t launch_model_infill_finish(const ImageSet& img, const ImageSet& model, const ImageSet& mask, const ImageSet& out, uint8_t* workspace,
                                      int n, int W, int H, const BlurKernel& K, hipStream_t s);
// mdvt_ffv1.hip: FFV1 encoding of device frames (mdvt_encode_video_frames).  A slice's size word holds its payload bytes or one of
// the flags below; a frame's size word the packet bytes or the flag of its first flagged slice.
constexpr uint32_t kSliceTooLarge = 0xFFFFFFFEu;     // the payload does not fit the 24-bit slice size
constexpr uint32_t kSliceOverflow = 0xFFFFFFFFu;     // the payload passes the slice's capacity, or the packet the caller's buffer
struct Ffv1StateTables { uint8_t zero[256], one[256]; };
struct Ffv1CodeArgs {
    const uint8_t* src; size_t pitch, frame_stride;
    int channels, ri, gi, bi;                        // bytes per pixel and the byte of R, G, B in a pixel (grey: all 0)
    int W, H, nh, nv;
    uint8_t* scratch; size_t slice_stride;           // per slice of the pass: slice_stride bytes of scratch
    uint32_t cap;                                    // payload bytes a slice may take (at most 2^24 - 1)
    int cap_is_24bit;                                // cap is the 24-bit limit: passing it is kSliceTooLarge
    uint32_t* slice_n;                               // [slices of the pass]
};
struct Ffv1LayoutArgs {
    const uint32_t* slice_n; int spf, n_frames;
    uint32_t* sizes; unsigned long long* offsets;    // the caller's arrays, at the pass's first frame
    unsigned long long* used; unsigned long long packets_cap;
};
struct Ffv1EmitArgs {
    const uint32_t* slice_n; const uint8_t* scratch; size_t slice_stride; int spf;
    const uint32_t* sizes; const unsigned long long* offsets; uint8_t* packets;
};
Ffv1StateTables ffv1_default_states();
hipError_t launch_ffv1_code(const Ffv1CodeArgs& a, const Ffv1StateTables& tab, int n_slices, hipStream_t s);
hipError_t launch_ffv1_layout(const Ffv1LayoutArgs& a, hipStream_t s);
hipError_t launch_ffv1_emit(const Ffv1EmitArgs& a, int n_slices, hipStream_t s);
// mdvt_ffv1_decode.hip, mdvt_ffv1_stream_decode.hip: FFV1 decoding of packets in device memory (mdvt_decode_video_frames,
// include/mdvt_ffv1_decode.h: key frames only, a pass of frames at a time; mdvt_decode_video_stream,
// include/mdvt_ffv1_stream_decode.h: inter frames and Golomb-Rice coding, consecutive packets).  The first call leaves the last
// seven fields zero.
struct Ffv1DecodeArgs {
    const uint8_t* packets; unsigned long long packets_bytes;      // the packet buffer and its size: no packet may pass it
    const unsigned long long* offsets; const uint32_t* sizes;      // the caller's arrays, at the pass's first frame
    int n_frames, W, H, nh, nv, ec;
    uint8_t* dst; size_t pitch, frame_stride; int ri, bi;          // the pass's first stored frame; the byte of R and of B in a pixel
    uint32_t* status;                                              // the caller's status words, at the pass's first frame
    uint32_t* table;                                               // workspace [2][frames of the pass * slices]: slice offsets, payload bytes
    uint32_t* claims;                                              // workspace [frames of the pass * slices], zeroed: a cell's claim
    int line_stride;                                               // samples per row slot in LDS: the widest slice + 2
    int first_out, coder, micro;                                   // the first frame that is stored; the record's coder_type and micro_version
    uint32_t* kind;                                                // workspace [n_frames]: mdvt_ffv1::kFrameInter / Key / Bad
    int planar, hs, vs;                                            // a YCbCr stream (SliceDec's planar mode) and its log2 chroma subsampling
};
size_t ffv1_decode_lds_bytes(int line_stride);                     // dynamic LDS of k_ffv1_dec_slice: the row slots
size_t ffv1_stream_lds_bytes(int coder, int line_stride);          // dynamic LDS of k_ffv1_stream_chain: the context state, then the row slots
// static LDS of k_ffv1_stream_chain, rounded up.  k_ffv1_dec_slice keeps its context state (coder_type 1) there as well, so this +
// ffv1_stream_lds_bytes(coder, line_stride) is the whole LDS of either kernel: what is left of a CU's 160 KiB bounds the widest slice
size_t ffv1_decode_static_lds_bytes();
hipError_t launch_ffv1_decode(const Ffv1DecodeArgs& a, const Ffv1StateTables& tab, hipStream_t s);
hipError_t launch_ffv1_stream_decode(const Ffv1DecodeArgs& a, const Ffv1StateTables& tab, hipStream_t s);
// mdvt_convergence.hip: per-frame masked depth means (mdvt_convergence_depths, include/mdvt_convergence.h)
struct ConvergenceArgs {
    const uint8_t* depth; size_t depth_pitch, depth_stride; int depth_bgr, depth_vec;     // the set's first frame; _vec: 12-byte loads are aligned
    const uint8_t* mask; size_t mask_pitch, mask_stride; int mask_bgr, mask_vec;
    uint32_t depth_W, mask_W;                                      // pixels per row; npx where the pitch is 3 * width (one long row)
    uint32_t npx, nchunks, nunits;                                 // pixels, chunks of 8192 values and units of 2048 pixels of a frame
    int n_frames, n_masked;                                        // frames of the set; its first n_masked have a mask frame
    float div;                                                     // float(255^4 / max_depth)
    unsigned long long* bits;                                      // workspace [n_masked][nunits][32]: the selection as ballot words
    uint16_t* compact; size_t compact_stride;                      // workspace [n_masked][compact_stride]: the selected codes in order
    float* sums;                                                   // workspace [n_frames][nchunks]
    uint32_t *unit_cnt, *unit_off, *totals;                        // workspace [n_masked][nunits] twice, [n_masked]
    float* means; uint32_t* counts;                                // the caller's, at the set's first frame; counts may be null
};
hipError_t launch_convergence(const ConvergenceArgs& a, hipStream_t s);
// mdvt_view.hip: the per-frame centre of the vertices (mdvt_view_centers, include/mdvt_view.h), one launch set
constexpr size_t kViewSumBytes = 3 * sizeof(double);               // a chunk's three coordinate sums
struct ViewCentersArgs {
    const uint8_t* depth; size_t depth_pitch, depth_stride;        // the batch's first frame
    const FrameDev* fp;                                            // device array, one per frame of the batch
    int frame0, n_frames;                                          // the set's first frame within the batch, its frames
    int W, H, of_by_one;
    uint32_t npx, nchunks;                                         // vertices and chunks of 8192 vertices of a frame
    const uint8_t* unused; size_t unused_stride;                   // workspace [n_frames][npx]: the edge filter's flags of the set, or null (nothing is parked)
    double* sums;                                                  // workspace [n_frames][nchunks][3]
    double* centers;                                               // the caller's, at the batch's first frame
};
hipError_t launch_view_centers(const ViewCentersArgs& a, hipStream_t s);
// mdvt_geometry.hip: the geometry export (mdvt_export_geometry_batch, mdvt_depth_grey_batch; include/mdvt_geometry.h), one launch set
constexpr uint32_t kGeomBlock = 256;                               // items (triangles, or vertices) a workgroup of the compaction counts and scatters
constexpr uint32_t kGeomScan = 256;                                // workgroup totals one step of the scan takes
struct GeometryArgs {
    const uint8_t* depth; size_t depth_pitch, depth_stride;        // the batch's first frame
    const uint8_t* color; size_t color_pitch, color_stride;        // likewise, or null
    double* vertices; size_t vertices_stride;                      // the caller's outputs at the batch's first frame; each may be null
    int32_t* triangles; size_t triangles_stride;
    int32_t* used_index; size_t used_stride;
    double* points; size_t points_stride;
    uint8_t* point_rgb; size_t point_rgb_stride;
    uint32_t* counts;                                              // [batch][2] = {U, M}
    const FrameDev* fp;                                            // device array, one per frame of the batch: mult (decode 0: the divisor), scale, Kd, rKd, sx, sy, has_T, Td
    int frame0, n_frames;                                          // the set's first frame within the batch, its frames
    int W, H, decode;
    uint32_t npx, ncell;                                           // vertices and cells of a frame (2 ncell triangles)
    uint32_t nbt, nbv;                                             // workgroups of kGeomBlock triangles / vertices of a frame
    uint8_t* flags; size_t flags_stride;                           // workspace [n_frames][2 ncell]: 1 = removed, in draw order; null: nothing is removed
    uint32_t* totals;                                              // workspace [n_frames][nbt + nbv]: kept items per workgroup, after the scan those before it
};
hipError_t launch_export_geometry(const GeometryArgs& a, hipStream_t s);
hipError_t launch_depth_grey(const uint8_t* depth, size_t pitch, size_t stride, float divisor, float mult, int bits, void* out,
                             size_t out_pitch, size_t out_stride, int W, int H, int n_frames, hipStream_t s);
// mdvt_metric_align.hip: the scale-and-shift fit and the metric depth codes (include/mdvt_metric_align.h)
constexpr uint32_t kFitSetChunks = 1024;                           // chunks of 8192 elements per launch set of the fit
struct FitPlane {
    const uint8_t* p; size_t pitch, stride;                        // the first plane; bytes between rows and between planes
    uint32_t W, HW, n;                                             // values per row and per plane, and in all; W = HW = n where nothing is padded (one long row)
    int vec;                                                       // four values from a multiple of 4 on are one aligned 16-byte (mask: 4-byte) load
};
struct FitArgs {
    FitPlane pred, target, mask;                                   // mask.p null: none
    int target_is_depth;
    uint32_t n, chunk0, nchunks_set;                               // elements in all; the set's first chunk and its chunks (<= kFitSetChunks)
    int first_set, last_set;
    float* sums; uint32_t sums_stride;                             // workspace [5][sums_stride]: the chunk sums of a set, sum by sum
    float* state;                                                  // workspace [5]: the totals up to this set
    float* out;                                                    // the caller's 8 floats
};
hipError_t launch_scale_shift_fit(const FitArgs& a, hipStream_t s);
// what the two steps that write a depth video's codes share (mdvt_depth_code.h); each one's own pair, a factor on the device and a
// 0 / 1 flag, stands in the same place
struct DepthCodesArgs {
    const uint8_t* src; size_t src_pitch, src_stride; int in_w, in_h, src_vec;       // float32 planes; _vec: 16-byte loads are aligned
    union { const float* scale_shift;                              // mdvt_metric_depth_codes: the fit's two floats
            const float* scale; };                                 // mdvt_depth_video_codes: one float, or null: no factor
    union { int style; int nan_to_max; };                          // likewise
    float fmax; double multi;                                      // float(max_depth), 255^4 / max_depth
    int out_w, out_h, resize; double ratio_x, ratio_y;             // in / out per axis
    uint8_t* codes; size_t codes_pitch, codes_stride; int bgr, codes_vec;
    uint8_t* plane; size_t plane_pitch, plane_stride; int plane_vec;          // null: no depth planes
    uint32_t gw, groups;                                           // groups of four pixels per output row and per image
    int frame0;                                                    // the launch's first frame
};
// mdvt_metric_align.hip: relative planes to metric depth codes (include/mdvt_metric_align.h)
hipError_t launch_metric_codes(const DepthCodesArgs& a, int n_frames, hipStream_t s);
// mdvt_depth_sink.hip: metric depth planes to a depth video's codes (mdvt_depth_video_codes; include/mdvt_depth_sink.h)
hipError_t launch_depth_sink(const DepthCodesArgs& a, int n_frames, hipStream_t s);
// mdvt_normal_infill.hip: the six cross dilations of normal_infill (bni:112) on their own.  marks: an image as mdvt_mark_lower_side
// writes it ((0,0,255) at a mark); grown: H rows of W bytes without padding, zeroed here, 1 within L1 distance 6 of a mark.
hipError_t launch_grow_marks(const uint8_t* marks, size_t marks_pitch, uint8_t* grown, int W, int H, hipStream_t s);
// mdvt_infill_adapter.hip: the frame preparation, colour match and compositing around an in-painting model (include/mdvt_infill_adapter.h)
struct AdapterImage { const uint8_t* p; size_t pitch, stride; };   // frame k at p + k * stride; u8 RGB rows unless said otherwise
struct AdapterResize { int in_w, in_h, out_w, out_h, mode; double rx, ry; };     // mode 0 copy, 1 the 2 x 2 area mean, 2 linear; rx, ry = in / out
AdapterResize adapter_resize(int in_w, int in_h, int out_w, int out_h);
// mdvt_scene.hip: the hue, saturation and value difference sums of consecutive frames (mdvt_scene_frame_sums, include/mdvt_scene.h)
struct SceneArgs {
    const uint8_t* frames; size_t pitch, stride;                   // n_frames frames of W x H packed pixels
    const uint8_t* prev; size_t prev_pitch;                        // the frame before them, or null
    int n_frames, bgr;
    uint32_t W, gw, units;                                         // vector kernel: groups of 16 pixels per row, groups of a frame; pixel kernel: units = analysed pixels
    AdapterResize rs;                                              // frame -> analysed image (mode 0 where factor is 1)
    unsigned long long* sums;                                      // the caller's [pairs][3], zeroed before the launch
};
hipError_t launch_scene_sums(const SceneArgs& a, bool vec, hipStream_t s);
struct AdapterPrepareArgs {
    AdapterImage color, mask;                                      // the eye's half of the side-by-side frames (p at the eye's first column)
    int mirror;                                                    // the eye is read right to left
    AdapterResize rs;                                              // eye -> model
    uint8_t* image; size_t image_pitch, image_stride;              // the model's image
    uint8_t* mmask; size_t mmask_pitch, mmask_stride;              // the model's mask, one byte per pixel
    uint32_t* holes;                                               // [n], zeroed before the launch
};
hipError_t launch_adapter_prepare(const AdapterPrepareArgs& a, int n, hipStream_t s);
constexpr uint32_t kMomentsWiden = 65536;                          // pixels a lane may sum in 32 bits: 65536 * 255 * 255 < 2^32
struct LhmMomentsArgs {
    AdapterImage img, mask;                                        // mask.p null: every pixel counts; else one byte per pixel, 0 = counts
    int W, H, vec;                                                 // vec: four pixels are three aligned dwords (mask: one)
    unsigned long long* out;                                       // [n][10], zeroed before the launch
};
hipError_t launch_lhm_moments(const LhmMomentsArgs& a, int n, hipStream_t s);
struct LhmApplyArgs {
    AdapterImage img; int W, H, vec;
    const double* params;                                          // [n][15]: A row-major, mu_x, mu_r
    uint8_t* out; size_t out_pitch, out_stride;
};
hipError_t launch_lhm_apply(const LhmApplyArgs& a, int n, hipStream_t s);
struct AdapterGauss { float w[15]; };                              // cv2.getGaussianKernel(15, 0) rounded to f32 (built on the host in f64)
struct AdapterCompositeArgs {
    AdapterImage model; int mirror; AdapterResize rs;              // one model frame -> eye
    AdapterImage color, mask;                                      // the eye's half of one side-by-side frame
    const uint8_t* grown;                                          // [eh][ew] 0 / 1
    float* hblur;                                                  // [eh][ew] the horizontal pass
    uint8_t* pasted; size_t pasted_pitch;                          // the eye's half of the two outputs
    uint8_t* blended; size_t blended_pitch;
    AdapterGauss g;
};
hipError_t launch_adapter_composite(const AdapterCompositeArgs& a, hipStream_t s);
// mdvt_infill_engines.hip: the three model inputs of the m2svid infill step (include/mdvt_infill_engines.h)
constexpr int kM2sPrepareFrames = 21845;                           // frames per launch: 3 * frames in the grid's third dimension
struct M2sPrepareArgs {
    AdapterImage color, mask;                                      // the eye's half of the side-by-side frames (p at the eye's first column)
    AdapterImage org;                                              // the original colour frames, whole
    int mirror;                                                    // the eye and the original frame are read right to left
    AdapterResize rs_image, rs_org, rs_mask;                       // eye -> image, original -> image, eye -> mask
    uint8_t* image; size_t image_pitch, image_stride;
    uint8_t* org_image; size_t org_image_pitch, org_image_stride;
    uint8_t* mmask; size_t mmask_pitch, mmask_stride;              // the model's mask, one byte per pixel
    uint32_t* holes;                                               // [n], zeroed before the launch
};
hipError_t launch_m2s_prepare(const M2sPrepareArgs& a, int n, hipStream_t s);
// mdvt_depth_engines.hip: frames into a model, PromptDA's prompt and UniK3D's focal estimate (include/mdvt_depth_engines.h)
struct ModelFramesArgs {
    const uint8_t* src; size_t src_pitch, src_stride; int bgr, src_vec;       // _vec: four pixels of a row are three aligned dwords
    AdapterResize rs;                                              // frame -> model
    uint8_t* dst; size_t dst_pitch, dst_plane, dst_stride; int as_float, dst_vec;     // _vec: four values of a plane are one aligned store
    uint32_t gw, groups;                                           // groups of four pixels per output row and per frame
    int frame0;                                                    // the launch's first frame
};
hipError_t launch_model_frames(const ModelFramesArgs& a, int n_frames, hipStream_t s);
struct DepthPromptArgs {
    const uint8_t* src; size_t src_pitch, src_stride; int in_w, in_h, bgr, src_vec;
    float mult;                                                    // float(max_depth / 255^4)
    int out_w, out_h, resize; double ratio_x, ratio_y;             // in / out per axis
    uint8_t* dst; size_t dst_pitch, dst_stride; int dst_vec;
    uint32_t gw, groups;                                           // groups of four values per output row and per frame
    int frame0;                                                    // the launch's first frame
};
hipError_t launch_depth_prompt(const DepthPromptArgs& a, int n_frames, hipStream_t s);
constexpr uint32_t kFocalUnit = 2048;                              // points a wave counts / compacts
struct FocalArgs {
    const uint8_t* points; size_t pitch, stride;                   // the set's first frame; bytes between rows and frames
    size_t chan_bytes, point_bytes;                                // bytes between the coordinates of a point, and between points of a row
    uint32_t W, npx, nunits, nchunks;                              // points per row and per frame; units of 2048 points, chunks of 8192 values
    float half_w, half_h;                                          // width / 2, height / 2 (exact)
    int n_frames;                                                  // frames of the set; list 2 f is frame f's ex, list 2 f + 1 its ey
    uint32_t *unit_cnt, *unit_off, *totals;                        // workspace [2 n_frames][nunits] twice, [2 n_frames]
    float* compact; size_t compact_stride;                         // workspace [2 n_frames][compact_stride]: the selected values in order
    float* sums;                                                   // workspace [2 n_frames][nchunks]
    float* focal; uint32_t* counts;                                // the caller's, at the set's first frame; counts may be null
};
hipError_t launch_focal_from_points(const FocalArgs& a, hipStream_t s);
// mdvt_video_mask.hip: Pillow's 8-bit Lanczos resampler and the mask step's two normalisations (include/mdvt_video_mask.h)
constexpr int kLzStrip = 8;                                        // output columns a workgroup of the fused form takes
constexpr size_t kLzFusedLds = 65536;                              // the LDS a workgroup of the fused form may ask for
struct LzAxis {                                                    // one axis' table on the device (mdvt_lanczos_table.h)
    const int32_t* bounds;                                         // [out][2]: the first source sample, the number of taps
    const int32_t* coef;                                           // [ksize][out]
};
struct LzArgs {
    const uint8_t* src; size_t src_pitch, src_stride;              // the launch's first frame
    uint8_t* dst; size_t dst_pitch, dst_stride;
    int C, rep;                                                    // interleaved channels; 3 with C = 1: a value is written as three equal bytes
    int in_w, in_h, out_w, out_h;                                  // a single pass leaves the other axis' sizes equal
    LzAxis h, v;
};
hipError_t launch_lz_rows(const LzArgs& a, int n_frames, hipStream_t s);      // the horizontal pass: in_w -> out_w on in_h rows
hipError_t launch_lz_cols(const LzArgs& a, int n_frames, hipStream_t s);      // the vertical pass: in_h -> out_h on out_w columns
hipError_t launch_lz_copy(const LzArgs& a, int n_frames, hipStream_t s);      // both passes skipped
hipError_t launch_lz_fused(const LzArgs& a, int n_frames, hipStream_t s);     // both passes, the intermediate strip in LDS
struct MaskInputArgs {
    const uint8_t* img; size_t img_pitch, img_stride; int w, h, bgr;          // the resized frames, packed 3 bytes per pixel
    uint32_t* max_byte;                                            // workspace [n]: zeroed, then each frame's maximum byte
    float* lut;                                                    // workspace [n][3][256]: plane c's value of byte v
    double mean[3], std[3];
    uint8_t* dst; size_t dst_pitch, dst_plane, dst_stride; int dst_vec;       // _vec: four values of a plane are one aligned 16-byte store
};
hipError_t launch_mask_model_input(const MaskInputArgs& a, int n_frames, hipStream_t s);
struct MaskPredArgs {
    const uint8_t* pred; size_t pred_pitch, pred_stride; int w, h;            // float32 planes
    uint32_t* stats;                                               // workspace [n][4]: ordered keys of min and max, the non-finite flag
    uint8_t* dst; size_t dst_pitch, dst_stride; int rep;           // the byte planes; rep as in LzArgs
};
hipError_t launch_mask_pred_bytes(const MaskPredArgs& a, int n_frames, hipStream_t s);
// mdvt_mvsa.hip: torch's bilinear resize into a model, two nearest resizes to depth codes and the masked median ratio (include/mdvt_mvsa.h)
struct NearAxis { float to_mid, to_src; int mid, src; };           // an output index -> near(near(x, mid, out), src, mid): the two scales, the two clamps
struct BilinearFramesArgs {
    const uint8_t* src; size_t src_pitch, src_stride; int in_w, in_h, bgr;
    float scale_x, scale_y;                                        // fl(float(in) / float(out)) per axis
    int small;                                                     // out_w + out_h <= 128: torch's CPU kernel for small outputs, four weights summed in order
    uint8_t* dst; size_t dst_pitch, dst_plane, dst_stride; int out_w, dst_vec;        // _vec: four values of a plane are one aligned 16-byte store
    uint32_t gw, groups;                                           // groups of four pixels per output row and per frame
    int frame0;                                                    // the launch's first frame
};
hipError_t launch_bilinear_frames(const BilinearFramesArgs& a, int n_frames, hipStream_t s);
struct NearestCodesArgs {
    DepthCodesArgs c;                                              // the source planes and the tail's outputs; resize, ratio_x, ratio_y and scale unused
    NearAxis x, y;
    const uint8_t* scales; size_t scales_stride;                   // frame k's factor at scales + k * scales_stride; null: no factor
};
hipError_t launch_nearest_codes(const NearestCodesArgs& a, int n_frames, hipStream_t s);
constexpr uint32_t kMedianFrameWords = 260;                        // a frame's scratch: 256 histogram words, then prefix, sought index, count, unused
struct RatioMedianArgs {
    const uint8_t* cv; size_t cv_pitch, cv_stride; uint32_t cv_w, npx;                // the set's first frame; npx = cv_w * cv_h
    const uint8_t* ref; size_t ref_pitch, ref_stride; float ref_sx, ref_sy; int ref_w, ref_h;     // near(x, ref_w, cv_w): the scale and the clamp
    const uint8_t* mask; size_t mask_pitch, mask_stride; float mask_sx, mask_sy; int mask_w, mask_h;      // null: every pixel counts
    uint32_t* work;                                                // workspace [n_frames][kMedianFrameWords], zeroed before the first pass
    int n_frames;
    float* median; uint32_t* counts;                               // the caller's, at the set's first frame; counts may be null
};
hipError_t launch_ratio_median(const RatioMedianArgs& a, hipStream_t s);
// mdvt_megasam.hip: cv2's area resize, torch's nearest-exact and bilinear resizes into the camera tracker and its planes out to video
// frames (include/mdvt_megasam.h)
constexpr size_t kAreaLds = 65536;                                 // the LDS a workgroup of the area kernel may ask for
struct AreaAxis {                                                  // one axis' table on the device (mdvt_area_table.h)
    const int32_t* first; const int32_t* count; const float* w; int ktaps;
};
struct AreaFramesArgs {
    const uint8_t* src; size_t src_pitch, src_stride; int in_w, bgr, src_vec;        // _vec: rows are staged with aligned 16-byte loads
    AreaAxis x, y;
    uint8_t* dst; size_t dst_pitch, dst_plane, dst_stride; int out_w, out_h;         // the cropped size
    int tile_w;                                                    // output columns of a workgroup
    uint32_t lds_row;                                              // bytes a staged source row may take in LDS (a multiple of 16)
    int frame0;                                                    // the launch's first frame
};
hipError_t launch_area_frames(const AreaFramesArgs& a, int n_frames, hipStream_t s);
struct TrackerPlaneArgs {                                          // packed frames -> a float32 plane through one of torch's resizes and a crop
    const uint8_t* src; size_t src_pitch, src_stride; int in_w, in_h, bgr;
    float scale_x, scale_y;                                        // fl(float(in) / float(mid)) per axis
    int small;                                                     // the mask: mid_w + mid_h <= 128 (BilinearFramesArgs.small)
    float divisor;                                                 // the depth: float32(255^4 / max_depth)
    uint8_t* dst; size_t dst_pitch, dst_stride; int out_w, dst_vec;
    uint32_t gw, groups;                                           // groups of four pixels per output row and per frame
    int frame0;
};
hipError_t launch_tracker_depth(const TrackerPlaneArgs& a, int n_frames, hipStream_t s);
hipError_t launch_tracker_mask(const TrackerPlaneArgs& a, int n_frames, hipStream_t s);
struct TrackerOutArgs {
    DepthCodesArgs c;                                              // the source planes and the frames (codes); mode 1: resize, ratio_x, ratio_y, fmax = m
    float scale_x, scale_y;                                        // mode 0: fl(float(in) / float(out)) per axis
};
hipError_t launch_tracker_codes(const TrackerOutArgs& a, int n_frames, hipStream_t s);      // mode 0: nearest-exact, clip, the 16-bit code
hipError_t launch_tracker_grey(const TrackerOutArgs& a, int n_frames, hipStream_t s);       // mode 1: linear resize, clip / m * 255, three equal bytes
// mdvt_inspatio.hip: the 4 x 4 grid of masked cross-correlation shifts (mdvt_masked_shift_grid, include/mdvt_inspatio.h)
constexpr int kShiftMaxCell = 1024;                                // the longest cell side
constexpr int kShiftDirectPixels = 16384;                          // the largest cell the direct kernel holds in LDS
constexpr int kShiftAutoDirectPixels = 4096;                       // the largest cell MDVT_SHIFT_PATH_AUTO sums directly
struct ShiftCellState {                                            // one cell of the call, zeroed before the first launch
    unsigned long long max_den, max_n, max_c, count;               // the bits of max den, max N, the key of max c, the maxima of c
    long long sum_dy, sum_dx;                                      // the maxima's index sums
    uint32_t n_valid, active, pad[2];
};
struct ShiftGridArgs {
    const uint8_t* render; size_t render_pitch, render_stride;
    const uint8_t* infilled; size_t infilled_pitch, infilled_stride;
    const uint8_t* valid; size_t valid_pitch, valid_stride;
    int W, H, n_frames;
    int hmax, wmax;                                                // the largest cell: ceil(H / 4) x ceil(W / 4)
    int transform;                                                 // 0: the direct kernel, Ly = 2 hmax - 1, Lx = 2 wmax - 1; 1: powers of two
    int Ly, Lx, log_ly, log_lx;
    size_t plane;                                                  // Ly * Lx
    double2* planes;                                               // [unit of the set][3][plane]
    ShiftCellState* state;                                         // [n_frames][16]
    unsigned long long* round_err;                                 // the bits of the largest |x - rint(x)|, zeroed before the first launch
    unsigned long long* round_err_out;                             // the caller's, or null
    int unit0, n_units;                                            // the launch set: interior cells unit0 .. unit0 + n_units - 1 of 8 per frame
    double* shift; uint8_t* status;                                // the caller's
};
// columns a workgroup of the column pass transforms at once (its LDS: (lines * L + L / 2) * 16 bytes <= 48 KiB)
inline int shift_fft_lines(int L) { return L >= 2048 ? 1 : (L >= 1024 ? 2 : 4); }
hipError_t launch_shift_gate(const ShiftGridArgs& a, hipStream_t s);        // the gate and the border columns, all frames
hipError_t launch_shift_units(const ShiftGridArgs& a, hipStream_t s);       // one launch set of interior cells: sums, then maxima
hipError_t launch_shift_finish(const ShiftGridArgs& a, hipStream_t s);      // all frames: shift and status
struct FlowWarpArgs {                                              // mdvt_flow_warp
    const float* grids; const uint8_t* has_grid;                   // [n][4][4][2] (dx, dy); [n]
    const uint8_t* src; size_t src_pitch, src_stride;
    uint8_t* dst; size_t dst_pitch, dst_stride;
    int W, H, frame0;
};
hipError_t launch_flow_warp(const FlowWarpArgs& a, int n_frames, hipStream_t s);
struct InspatioPrepareArgs {                                       // mdvt_inspatio_prepare_eye; mask.p null: mdvt_inspatio_model_frames
    AdapterImage color, mask;                                      // the eye's half of the side-by-side frames (p at the eye's first column), or whole frames
    AdapterResize rs;                                              // eye -> model
    uint8_t* valid; size_t valid_pitch, valid_stride;              // the eye's validity plane, one byte per pixel
    uint8_t* render; size_t render_pitch, render_stride;           // the eye's render, holes black
    uint8_t* m_valid; size_t m_valid_pitch, m_valid_stride;        // both at the model's size
    uint8_t* m_render; size_t m_render_pitch, m_render_stride;
    uint32_t* holes;                                               // [n], zeroed before the launch
    int frame0;
};
hipError_t launch_inspatio_prepare(const InspatioPrepareArgs& a, int n_frames, hipStream_t s);
struct InspatioCompositeArgs {                                     // mdvt_inspatio_composite_eye, one frame of one eye
    const uint8_t* aligned; size_t aligned_pitch;                  // the aligned frame at the eye's size
    const uint8_t* color; size_t color_pitch;                      // the eye's half of the render and of the infill mask
    const uint8_t* mask; size_t mask_pitch;
    const uint8_t* grown;                                          // [H][W] 0 / 1 (blending)
    uint8_t* pasted; size_t pasted_pitch;                          // the eye's half of the outputs; blended null: no blending
    uint8_t* blended; size_t blended_pitch;
    int W, H;
};
hipError_t launch_inspatio_grow(const uint8_t* marks, size_t marks_pitch, uint8_t* grown, int W, int H, hipStream_t s);
hipError_t launch_inspatio_composite(const InspatioCompositeArgs& a, hipStream_t s);
hipError_t launch_selftest(int which, unsigned long long seed, unsigned long long* d_mism, hipStream_t s);
hipError_t launch_coherence_test(uint32_t* blk, size_t dwords, uint32_t tag, uint32_t* d_xcc, uint32_t* d_out, hipStream_t s);     // (mdvt_selftest.hip; r05 diagnosis)

namespace grid8 {
#include "mdvt_grid_decls.h"
}
namespace grid4 {
#include "mdvt_grid_decls.h"
}

}  // namespace mdvt
