// mdvt_api.hip -- the C ABI of include/mdvt.h: context, parameter preparation, launch sequencing.
// Host code only; the kernels are in the other *.hip units.  Compiled with -ffp-contract=off (the f64
// composition of the eye matrices below is part of the arithmetic decree).
#include "mdvt_internal.h"
#include "mdvt_ffv1_core.h"
#include "mdvt_ffv1_decode.h"
#include "mdvt_convergence.h"

#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <mutex>
#include <new>
#include <algorithm>
#include <string>
#include <unordered_map>
#include <array>
#include <map>
#include <vector>

using namespace mdvt;
using namespace mdvt::grid8;          // grid-independent launchers of the rasterising translation units; the renders are dispatched:
// The render launchers exist once per sub-pixel grid (mdvt_internal.h); a context uses the set of its mdvt_config.subpixel_bits.
#define MDVT_GRID_CALL(c, fn, ...) (grid_bits(c) == 4 ? mdvt::grid4::fn(__VA_ARGS__) : mdvt::grid8::fn(__VA_ARGS__))

namespace {

thread_local std::string g_create_error;

constexpr int kParamSlots = 8;        // pinned staging ring for per-frame constants
constexpr int kWorkspaceChunk = 8;    // frames per launch when a global workspace is needed

struct ParamSlot {
    FrameDev* host = nullptr;         // pinned
    FrameDev* dev = nullptr;
    size_t capacity = 0;              // frames
    hipEvent_t done = nullptr;        // H2D copy + the kernels reading it have been submitted/finished
    bool used = false;
};

}  // namespace

struct mdvt_ctx {
    int device = 0;
    int pool_tag = 0;                 // the GPU whose pooled workspace blocks this context may take (= device; tuning build: MDVT_POOL_TAG)
    int W = 0, H = 0;
    mdvt_config cfg{};
    bool cfg_set = false;
    std::string err;
    ParamSlot slots[kParamSlots];
    int next_slot = 0;
    // the most recently staged parameter block: clips with constant parameters re-use the device copy
    std::vector<FrameDev> last_staged;
    ParamSlot* last_slot = nullptr;
    hipStream_t last_stream = nullptr;
    // workspace for the general path / edge filter, sized for ws_frames frames
    int ws_frames = 0;
    bool ws_keys = false, ws_ekeys = false, ws_edges = false;
    unsigned long long* keys[2] = {nullptr, nullptr};
    unsigned long long* ekeys[2] = {nullptr, nullptr};
    uint32_t* elist = nullptr;        // written edge-key words per (slot, source row) + counters (behind the entries)
    unsigned long long* cbuf[2] = {nullptr, nullptr};
    bool ws_mesh = false;
    bool keys_dirty = false;          // a general-path submission was interrupted between splat and resolve
    uint32_t key_parity = 0;          // bit s: parity of the next use of z-key slot s (mdvt_device.h, parity scheme)
    uint8_t* tri_invalid = nullptr;
    uint8_t* unused = nullptr;
    uint32_t* bigq = nullptr;         // general mesh path: queue of large triangles + its counter (last dword)
    size_t bigq_bytes = 0, bigq_counters_at = 0;      // the queue block as laid out (without tuning padding), the dword offset of its counters
    int huge_lists = 1;               // huge lists inside the queue block (2: tuning layout "joint")
    mdvt::RowCell* rowcell = nullptr; // [H] scanline -> cell row table of the mesh grid (pure-shift band kernel)
    int rowcell_bits = 0;             // the sub-pixel grid that table was built for
    uint32_t* row_counts = nullptr;   // [row_counts_frames][2][H]
    uint32_t* wave_counts = nullptr;  // [row_counts_frames][H][16] (RenderArgs.wave_counts)
    uint32_t* divcheck = nullptr;     // [kDivSlots] (RenderArgs.divcheck), zeroed when allocated; slot k belongs to div_keys[k]
    std::vector<std::array<uint32_t, 3>> div_keys;      // bits of (mult, scale, dl) of the parameter sets checked so far
    hipEvent_t div_done = nullptr;    // recorded after the latest division check (every earlier check and the table's fill before it) ...
    hipStream_t div_stream = nullptr; // ... on this stream: a render on another stream waits for it before it reads the table
    int row_counts_frames = 0;
    // infill-mask completion: per image stamp u16 + T f32 + work image u8x3, and the per-image counters
    int telea_images = 0, telea_rounds = 0;
    mdvt::TeleaWorkspace telea{};
    uint32_t* telea_levels_host = nullptr;      // pinned: the deepest level of a pass, read back once per pass
    // infill-mask completion in the heap order: one block of mdvt::telea_heap_image_bytes per image of a pass, + remaining
    int heap_images = 0;
    uint8_t* heap_ws = nullptr;
    uint32_t* heap_remaining = nullptr;
    // FFV1 encoding (mdvt_encode_video_frames): the running packet offset (8 B), then per slice of a pass its size word and scratch
    uint8_t* ffv1_ws = nullptr;
    size_t ffv1_bytes = 0;
    // FFV1 decoding (mdvt_decode_video_frames): per slice of a pass its offset, payload bytes and cell claim
    uint8_t* ffv1_dec_ws = nullptr;
    size_t ffv1_dec_bytes = 0;
    // convergence depths (mdvt_convergence_depths): per frame of a launch set its chunk sums; with a mask also the selection's ballot
    // words, the selected codes and the unit counts
    uint8_t* conv_ws = nullptr;
    size_t conv_bytes = 0;
    // normal_infill / infill_using_mask_normals: about 16 B/px per image in flight
    uint8_t* ni_ws = nullptr;
    int ni_images = 0;
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
    // multisampled render (mdvt_config.samples = 4): the sample key planes of msaa_frames frames in flight, [slot][eye][H*W][4]
    unsigned long long* msaa_keys = nullptr;
    int msaa_frames = 0;
    bool msaa_dirty = false;          // a submission stopped between raster and resolve: the planes are not all empty
    // near-plane clipping (mdvt_set_near_clip; mdvt_near_clip.hip).  With samples = 4 it uses msaa_keys; single-sample: the key planes
    // of clip_frames frames in flight, [slot][eye][H*W], and one flag per slot and eye (an eye where some triangle straddles the plane)
    int32_t near_clip = 0;
    unsigned long long* clip_keys = nullptr;
    uint32_t* clip_flags = nullptr;
    int clip_frames = 0;
    bool clip_dirty = false;
};

namespace {

int fail(mdvt_ctx* c, int code, const char* fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (c) c->err = buf; else g_create_error = buf;
    return code;
}

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

// ---- Device workspace: a process-wide pool ---------------------------------------------------------------------------------
// A context's workspace blocks are NOT returned to the driver when the context goes: they wait here for the next context (of
// the same GPU) that asks for the same size class.  Why: the r04 soak found one FIRST render of a fresh context in ~3 000
// (12 processes sharing the GPU, a context created and destroyed per render) that lost entries of the triangle queue, and
// one process killed by a GPU memory fault -- only when the queue's block was larger than 2 MB, i.e. when it no longer came
// out of the runtime's own cache of sub-2 MB fragments but was mapped by hipMalloc and unmapped by hipFree once per context;
// never on a context's later renders, never with HSA_ENABLE_SDMA=0.  DESIGN.md section 9 has the diagnosis (r05: what the
// lost words held, which treatments of a fresh block stop it; tools/probe/fresh_alloc_probe.hip is the pattern without the
// library).  Whatever the cause below the HIP API, the library no longer creates the condition: (1) a block that does come
// fresh from hipMalloc is filled and the stream synchronised before anything uses it, (2) blocks are recycled here instead of
// freed, so in steady state no render ever runs on memory that was mapped microseconds earlier, (3) idle blocks are only given
// back to the driver beyond kDevPoolIdleCap bytes (oldest first) or on mdvt_release_cached_memory, each time behind a
// hipDeviceSynchronize.  A recycled block holds a previous user's data: nothing in the library reads a workspace word before
// the same call has written it (the soaks' sub-2 MB blocks always were recycled this way, by the runtime).
// The same treatment the pinned parameter blocks got in r03 (pool_take / pool_give below).
// Tuning build: MDVT_WS_POOL=off -> hipMalloc / hipFree per context as until r04; MDVT_WS_FRESH=none|canary|devsync|memset picks
// the treatment of a fresh block (product: memset); MDVT_POOL_TAG=n labels this context's blocks as GPU n's (tests).
struct DevBlock { void* p; size_t bytes; int tag; unsigned long long stamp; };
std::mutex g_dev_pool_mutex;
std::vector<DevBlock>& dev_pool() { static std::vector<DevBlock> p; return p; }
std::map<int, size_t>& dev_pool_idle() { static std::map<int, size_t> m; return m; }      // idle bytes per pool tag (= per GPU)
unsigned long long g_dev_pool_stamp = 0;
// Idle bytes kept PER GPU before that GPU's oldest blocks go back to the driver (mdvt_set_cached_memory_limit; default 4 GiB = the
// default workspace_mib budget, i.e. one context's worth of the largest workspace the library allocates by default).
size_t g_dev_pool_idle_cap = (size_t)4 << 30;

// Size classes: 4 KiB steps up to 64 KiB, 16 steps per power of two up to 1 MiB (at most 6.25 % over the request), 64 KiB steps
// above (the large blocks are what mdvt_config.workspace_mib budgets: they stay what was asked for; a clip's contexts share
// one frame size, so their blocks match exactly anyway).
size_t ws_size_class(size_t bytes)
{
    if (bytes <= ((size_t)64 << 10)) return (bytes + 4095) & ~(size_t)4095;
    if (bytes > ((size_t)1 << 20)) return (bytes + 65535) & ~(size_t)65535;
    size_t step = (size_t)4096;
    while ((step << 5) < bytes) step <<= 1;              // bytes in (16 step, 32 step]
    return (bytes + step - 1) / step * step;
}
// Gives the idle blocks that `pick` chooses (called under the pool's lock, oldest block first) back to the driver.
template <class Pick>
void drain_dev_pool(Pick pick, const size_t* new_idle_cap = nullptr)
{
    std::vector<DevBlock> out;
    {
        std::lock_guard<std::mutex> lock(g_dev_pool_mutex);
        if (new_idle_cap) g_dev_pool_idle_cap = *new_idle_cap;
        auto& pool = dev_pool();
        for (size_t k = 0; k < pool.size();) {
            if (!pick(pool[k])) { ++k; continue; }
            out.push_back(pool[k]);
            dev_pool_idle()[pool[k].tag] -= pool[k].bytes;
            pool.erase(pool.begin() + (long)k);
        }
    }
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess) count = 0;
    for (const DevBlock& b : out) {
        // (a block tagged for a GPU this process does not have -- the tuning build's MDVT_POOL_TAG -- lives on the current one)
        DeviceGuard g(b.tag >= 0 && b.tag < count ? b.tag : 0);
        (void)hipDeviceSynchronize();
        (void)hipFree(b.p);
    }
}

bool dev_pool_off() { const char* e = tuning_env(TUNE_WS_POOL); return e && (strcmp(e, "off") == 0 || strcmp(e, "delay") == 0); }

// device memory owned by a context, accounted for mdvt_workspace_bytes; `s`: the stream the fresh-block fill goes to
hipError_t ws_malloc(mdvt_ctx* c, void** p, size_t bytes, hipStream_t s)
{
    *p = nullptr;
    const bool pooled = !dev_pool_off();
    const size_t want = pooled ? ws_size_class(bytes) : bytes;
    if (pooled) {
        std::lock_guard<std::mutex> lock(g_dev_pool_mutex);
        auto& pool = dev_pool();
        for (size_t k = pool.size(); k-- > 0;)            // newest first
            if (pool[k].bytes == want && pool[k].tag == c->pool_tag) {
                *p = pool[k].p;
                dev_pool_idle()[c->pool_tag] -= want;
                pool.erase(pool.begin() + (long)k);
                break;
            }
    }
    if (!*p) {
        const char* fresh0 = tuning_env(TUNE_WS_FRESH);
        hipError_t e;
        if (fresh0 && strcmp(fresh0, "uncached") == 0) e = hipExtMallocWithFlags(p, want, hipDeviceMallocUncached);          // (r05 diagnosis)
        else if (fresh0 && strcmp(fresh0, "finegrained") == 0) e = hipExtMallocWithFlags(p, want, hipDeviceMallocFinegrained);
        else e = hipMalloc(p, want);
        if (e != hipSuccess && pooled) {                  // out of memory with idle blocks of other classes around: give them back, once
            (void)hipGetLastError();
            mdvt_release_cached_memory(-1);
            e = hipMalloc(p, want);
        }
        if (e != hipSuccess) return e;
        const char* fresh = tuning_env(TUNE_WS_FRESH);
        if (!fresh || strcmp(fresh, "memset") == 0) {
            if ((e = hipMemsetAsync(*p, 0, want, s)) != hipSuccess || (e = hipStreamSynchronize(s)) != hipSuccess) { (void)hipFree(*p); *p = nullptr; return e; }
        } else if (strcmp(fresh, "canary") == 0) {
            if ((e = hipMemsetAsync(*p, 0xC5, want, s)) != hipSuccess) { (void)hipFree(*p); *p = nullptr; return e; }
        } else if (strcmp(fresh, "devsync") == 0) {
            if ((e = hipDeviceSynchronize()) != hipSuccess) { (void)hipFree(*p); *p = nullptr; return e; }
        }                                                 // "none": as until r04
    }
    c->allocs[*p] = want; c->ws_bytes += want;
    return hipSuccess;
}
// (the caller has made sure no submitted work still uses the block: mdvt_destroy and the growing paths synchronise the device)
void ws_free(mdvt_ctx* c, void* p)
{
    if (!p) return;
    size_t bytes = 0;
    auto it = c->allocs.find(p);
    if (it != c->allocs.end()) { bytes = it->second; c->ws_bytes -= bytes; c->allocs.erase(it); }
    if (dev_pool_off() || bytes == 0 || bytes != ws_size_class(bytes)) {
        // (r05 diagnosis, tuning build: MDVT_WS_POOL=delay -> a freed block waits behind the next 64 before it goes back to the driver,
        //  so its address range is not handed out again at once)
        const char* e = tuning_env(TUNE_WS_POOL);
        if (e && strcmp(e, "delay") == 0) {
            static std::vector<void*> ring;
            ring.push_back(p);
            if (ring.size() > 64) { (void)hipFree(ring.front()); ring.erase(ring.begin()); }
            return;
        }
        (void)hipFree(p);
        return;
    }
    std::vector<void*> out;
    {
        std::lock_guard<std::mutex> lock(g_dev_pool_mutex);
        auto& pool = dev_pool();
        pool.push_back({p, bytes, c->pool_tag, ++g_dev_pool_stamp});
        size_t& idle = dev_pool_idle()[c->pool_tag];                                     // (accounted and capped per GPU)
        idle += bytes;
        for (size_t k = 0; idle > g_dev_pool_idle_cap && k < pool.size();) {             // oldest first (the vector is in stamp order)
            if (pool[k].tag != c->pool_tag) { ++k; continue; }                           // (this GPU's only: the device guard is the caller's)
            out.push_back(pool[k].p);
            idle -= pool[k].bytes;
            pool.erase(pool.begin() + (long)k);
        }
    }
    if (!out.empty()) {
        (void)hipDeviceSynchronize();
        for (void* q : out) (void)hipFree(q);
    }
}

// Everything the kernels need about one frame, derived in f64 and rounded once to f32.
// Pure-shift frames: on which row does the chain (mdvt_device.h "edge points") put an edge point of source row i?  Without
// pose and convergence the row is round( ((gy - cy) z / fy sH) (1/z) fyr + cyr ): in exact arithmetic independent of z,
//   v*(i) = (gy_i - cy) sH (fyr / fy) + cyr  ~  i + 1/2 - i / H^2   (mesh grid, cy = H/2),
// a hair below the tie i + 1/2 -- by less than the f32 rounding of fy (dmt:1058) moves it for the first rows, which then land
// on i + 1 -- and the eight f64 roundings of the chain move v by at most 8 H 2^-53.  Rows whose v* keeps a margin of four
// times that from a tie have their row decided here, once per camera matrix; the others (a tie in exact arithmetic: the
// roundings of each point decide) and the rows that land on i + 1 form [erow_lo, erow_hi), left to k_edge_rows_exact.
static void edge_row_range(FrameDev& f, int H)
{
    const long double fy = f.Kd[1], cy = f.Kd[3], sH = f.sHd, fyr = (long double)f.fyr, cyr = (long double)f.cyr;
    const long double margin = 32.0L * 1.1102230246251565e-16L * ((long double)H + fabsl(cyr) + 1.0L);
    int lo = H, hi = 0;
    bool wild = false;
    for (int i = 0; i < H; ++i) {
        const long double gy = f.sy == 1.0f ? (long double)i : (long double)((float)i * f.sy);
        const long double v = (gy - cy) * sH * (fyr / fy) + cyr;
        const long double fl = floorl(v);
        const bool undecided = fabsl(v - (fl + 0.5L)) <= margin;
        const long double row = undecided ? fl : floorl(v + 0.5L);           // undecided: fl or fl + 1
        const bool plain = !undecided && row == (long double)i;
        if (plain) continue;
        if (row != (long double)i && !(!undecided && row == (long double)i + 1.0L)) { wild = true; break; }
        if (i < lo) lo = i;
        if (i + 1 > hi) hi = i + 1;
    }
    f.erow_wild = wild ? 1 : 0;
    f.erow_lo = (wild || lo >= hi) ? 0 : lo;
    f.erow_hi = (wild || lo >= hi) ? 0 : hi;
}

int fill_frame_dev(mdvt_ctx* c, const mdvt_frame_params& p, FrameDev& f)
{
    const mdvt_config& cfg = c->cfg;
    const int W = c->W, H = c->H;
    const double fx = p.K[0], fy = p.K[4], cx = p.K[2], cy = p.K[5];
    const double fxr = p.Krender[0], fyr = p.Krender[4], cxr = p.Krender[2], cyr = p.Krender[5];
    if (!(fx > 0.0) || !(fy > 0.0) || !(fxr > 0.0) || !(fyr > 0.0))
        return fail(c, MDVT_ERR_INVALID_ARG, "camera matrix needs positive focal lengths");
    if (cxr * 2.0 != (double)W || cyr * 2.0 != (double)H)
        return fail(c, MDVT_ERR_UNSUPPORTED,
                    "render size (2*cx, 2*cy) = (%g, %g) differs from the frame size %dx%d (--vr180 is not built)",
                    cxr * 2.0, cyr * 2.0, W, H);
    if (!(p.depth_scale > 0.0)) return fail(c, MDVT_ERR_INVALID_ARG, "depth_scale must be > 0");
    memset(&f, 0, sizeof f);
    f.mult = (float)(cfg.max_depth / 4228250625.0);
    f.scale = (float)p.depth_scale;
    const double half = cfg.ipd_m / 2.0;
    f.dl = (float)(fxr * half);
    f.fx = (float)fx; f.fy = (float)fy; f.cx = (float)cx; f.cy = (float)cy;
    f.fxr = (float)fxr; f.fyr = (float)fyr; f.cxr = (float)cxr; f.cyr = (float)cyr;
    const bool mesh = cfg.mode == MDVT_MODE_MESH;
    f.sx = mesh ? (float)(((double)W + 1.0) / (double)W) : 1.0f;
    f.sy = mesh ? (float)(((double)H + 1.0) / (double)H) : 1.0f;
    f.sW = (float)(((double)W - 1.0) / (double)W);
    f.sH = (float)(((double)H - 1.0) / (double)H);
    f.Kd[0] = fx; f.Kd[1] = fy; f.Kd[2] = cx; f.Kd[3] = cy;
    f.rKd[0] = 1.0 / fx; f.rKd[1] = 1.0 / fy;
    const double conv = (p.convergence_angle == p.convergence_angle) ? p.convergence_angle : 0.0;   // NaN -> none
    const bool same_k = fx == fxr && fy == fyr && cx == cxr && cy == cyr;
    f.general = (p.has_T || conv != 0.0 || !same_k) ? 1 : 0;
    double T[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    if (p.has_T) {
        memcpy(T, p.T, sizeof T);
        if (fabs(T[12]) > 1e-12 || fabs(T[13]) > 1e-12 || fabs(T[14]) > 1e-12 || fabs(T[15] - 1.0) > 1e-12)
            return fail(c, MDVT_ERR_UNSUPPORTED, "pose matrix must be affine (last row 0 0 0 1)");
    }
    for (int eye = 0; eye < 2; ++eye) {
        // M = Translate(+-ipd/2) * Ry(-+a) * T;  Ry(t) = [[c,0,s],[0,1,0],[-s,0,c]]
        const double t = eye == 0 ? -conv : conv;
        const double cs = cos(t), sn = sin(t);
        const double R[3][3] = {{cs, 0.0, sn}, {0.0, 1.0, 0.0}, {-sn, 0.0, cs}};
        const double shift[3] = {eye == 0 ? half : -half, 0.0, 0.0};
        for (int r = 0; r < 3; ++r) {
            for (int col = 0; col < 3; ++col)
                f.M[eye][4 * r + col] = (float)((R[r][0] * T[0 + col] + R[r][1] * T[4 + col]) + R[r][2] * T[8 + col]);
            f.M[eye][4 * r + 3] = (float)(((R[r][0] * T[3] + R[r][1] * T[7]) + R[r][2] * T[11]) + shift[r]);
        }
    }
    // The edge points' chain takes the reference's operands as they are (mdvt_device.h "edge points")
    f.sWd = ((double)W - 1.0) / (double)W;
    f.sHd = ((double)H - 1.0) / (double)H;
    f.hd = half;
    f.has_T = p.has_T ? 1 : 0;
    memcpy(f.Td, T, sizeof T);
    f.has_conv = conv != 0.0 ? 1 : 0;
    f.cs[0] = cos(conv); f.cs[1] = sin(conv);
    if (!f.general && cfg.remove_edges && cfg.edge_points) {
        const double key[5] = {f.Kd[1], f.Kd[3], (double)f.fyr, (double)f.cyr, (double)f.sy};
        if (!(c->erow_cached && memcmp(key, c->erow_key, sizeof key) == 0)) {
            edge_row_range(f, H);
            memcpy(c->erow_key, key, sizeof key);
            c->erow_val[0] = f.erow_lo; c->erow_val[1] = f.erow_hi; c->erow_val[2] = f.erow_wild;
            c->erow_cached = true;
        }
        f.erow_lo = c->erow_val[0]; f.erow_hi = c->erow_val[1]; f.erow_wild = c->erow_val[2];
    }
    // Convergence and nothing else (sr:707-726: rotation about the camera's y axis, shift along x): the projected row of a
    // vertex is depth independent, v = (gy - cy) / rz(j) + cy with rz(j) = m10 + m8 (gx_j - cx) / fx, which k_mesh_conv
    // (mdvt_mesh_conv.hip) builds on.  It takes the frame if the vertex rows stay low staircases: at most 12 rows of tilt
    // across the frame (its row tags are 5 bits, its column pairs expect neighbouring brackets to differ by one).
    f.conv_band = 0;
    if (mesh && !p.has_T && conv != 0.0 && same_k) {
        bool ok = true;
        for (int eye = 0; eye < 2 && ok; ++eye) {
            const float* M = f.M[eye];
            ok = M[1] == 0.0f && M[4] == 0.0f && M[5] == 1.0f && M[6] == 0.0f && M[7] == 0.0f && M[9] == 0.0f && M[11] == 0.0f;
            const double rz0 = (double)M[10] + (double)M[8] * ((0.0 - cx) / fx);
            const double rz1 = (double)M[10] + (double)M[8] * (((double)(W - 1) * ((double)W + 1.0) / (double)W - cx) / fx);
            if (!(rz0 > 0.5 && rz1 > 0.5 && rz0 < 2.0 && rz1 < 2.0)) ok = false;
            else if (fabs(1.0 / rz0 - 1.0 / rz1) * ((double)H * 0.5 + 1.0) * (fyr / fy) > 12.0) ok = false;
        }
        f.conv_band = ok ? 1 : 0;
    }
    return MDVT_OK;
}

// Pinned host staging memory is NEVER returned to the driver while the process lives.  The r03 parity soak found one frame in
// ~20 000 context create / render / destroy cycles (14 processes sharing the GPU) rendered with the PREVIOUS context's
// parameter block: a hipHostMalloc'ed buffer that recycles the address of one just hipHostFree'd can be read by the GPU --
// copy engine or kernel alike, even with a stream synchronisation after the copy -- with the old allocation's content
// (tests/dbg_param_stress.py reproduces it: 12 wrong frames in 191 000 contexts with per-context hipHostMalloc /
// hipHostFree, 0 in 1 064 000 with this pool, and a context is created 5 x faster).  MDVT_PARAM_UPLOAD=recycle restores
// the per-context allocation for that A/B.
struct PoolBlock { void* host; void* dev; size_t bytes; int device; };     // device: the GPU `dev` was allocated on (-1: no device block)
std::mutex g_pool_mutex;
std::vector<PoolBlock>& param_pool() { static std::vector<PoolBlock> p; return p; }
bool param_pool_off()
{
    const char* e = tuning_env(TUNE_PARAM_UPLOAD);
    return e && strcmp(e, "recycle") == 0;
}
// A pinned host block of at least `bytes`, with a device block of the same size on GPU `device` if with_dev (a block that
// carries device memory only ever goes back to a context on the GPU it was allocated on: contexts of two GPUs share the pool).
hipError_t pool_take(size_t bytes, bool with_dev, int device, void** host, void** dev, size_t* got)
{
    if (!param_pool_off()) {
        std::lock_guard<std::mutex> lock(g_pool_mutex);
        auto& pool = param_pool();
        for (size_t k = 0; k < pool.size(); ++k)
            if (pool[k].bytes >= bytes && pool[k].device == (with_dev ? device : -1)) {
                *host = pool[k].host; *dev = pool[k].dev; *got = pool[k].bytes;
                pool.erase(pool.begin() + (long)k);
                return hipSuccess;
            }
    }
    *host = nullptr; *dev = nullptr; *got = bytes;
    hipError_t e = hipHostMalloc(host, bytes, hipHostMallocDefault);
    if (e == hipSuccess && with_dev) {
        e = hipMalloc(dev, bytes);                       // (the caller's DeviceGuard has made `device` current)
        if (e != hipSuccess) { (void)hipHostFree(*host); *host = nullptr; *dev = nullptr; }
    }
    return e;
}
void pool_give(void* host, void* dev, size_t bytes, int device)
{
    if (!host) return;
    if (param_pool_off()) { (void)hipHostFree(host); if (dev) (void)hipFree(dev); return; }
    std::lock_guard<std::mutex> lock(g_pool_mutex);
    param_pool().push_back({host, dev, bytes, dev ? device : -1});
}

// Stage n FrameDev records to the device through the pinned ring; returns the device pointer.
int stage_params(mdvt_ctx* c, const std::vector<FrameDev>& v, hipStream_t s, const FrameDev** dev, ParamSlot** slot_out)
{
    if (c->last_slot && c->last_stream == s && c->last_staged.size() == v.size() &&
        memcmp(c->last_staged.data(), v.data(), v.size() * sizeof(FrameDev)) == 0) {
        // identical to what already sits on the device (stream order keeps the earlier copy ahead of us)
        *dev = c->last_slot->dev;
        *slot_out = c->last_slot;
        return MDVT_OK;
    }
    ParamSlot& sl = c->slots[c->next_slot];
    c->next_slot = (c->next_slot + 1) % kParamSlots;
    if (sl.used) MDVT_HIP(c, hipEventSynchronize(sl.done));     // slot is being reused: its last user must be done
    if (sl.capacity < v.size()) {
        pool_give(sl.host, sl.dev, sl.capacity * sizeof(FrameDev), c->pool_tag);
        sl.host = nullptr; sl.dev = nullptr; sl.capacity = 0;
        size_t cap = 16;
        while (cap < v.size()) cap *= 2;
        void *h = nullptr, *d = nullptr;
        size_t got = 0;
        MDVT_HIP(c, pool_take(cap * sizeof(FrameDev), true, c->pool_tag, &h, &d, &got));
        sl.host = (FrameDev*)h; sl.dev = (FrameDev*)d; sl.capacity = got / sizeof(FrameDev);
    }
    if (!sl.done) MDVT_HIP(c, hipEventCreateWithFlags(&sl.done, hipEventDisableTiming));
    memcpy(sl.host, v.data(), v.size() * sizeof(FrameDev));
    MDVT_HIP(c, hipMemcpyAsync(sl.dev, sl.host, v.size() * sizeof(FrameDev), hipMemcpyHostToDevice, s));
    sl.used = true;
    c->last_staged = v;
    c->last_slot = &sl;
    c->last_stream = s;
    *dev = sl.dev;
    *slot_out = &sl;
    return MDVT_OK;
}

RenderWorkspaceLayout layout_of(const mdvt_ctx* c) { return RenderWorkspaceLayout(c->W, c->H, c->ws_frames, c->huge_lists); }
// (the EMPTY fill of fresh key buffers goes on the caller's stream: PyTorch's pool streams do not synchronise with the
//  legacy null stream, so a fill issued there could land after the first splat)
int ensure_workspace(mdvt_ctx* c, int frames, bool need_keys, bool need_ekeys, bool need_edges, bool need_mesh_ws, hipStream_t s)
{
    const bool grow = frames > c->ws_frames;
    // (blocks that are replaced go back to the pool, where another context may pick them up at once: whatever was submitted
    //  with them -- to any stream -- has to be through first; hipFree used to wait for that implicitly)
    if (grow && c->ws_bytes) MDVT_HIP(c, hipDeviceSynchronize());
    // (not growing, yet a group that is not complete holds a buffer: an earlier call failed half-way through allocating it -- its
    //  asynchronous fill may still be pending, and the block must not reach the pool before that is through)
    if (!grow && ((need_keys && !c->ws_keys && (c->keys[0] || c->keys[1])) || (need_ekeys && !c->ws_ekeys && (c->ekeys[0] || c->ekeys[1] || c->elist)) ||
                  (need_edges && !c->ws_edges && (c->tri_invalid || c->unused)) || (need_mesh_ws && !c->ws_mesh && (c->cbuf[0] || c->cbuf[1]))))
        MDVT_HIP(c, hipDeviceSynchronize());
    auto drop = [c](auto*& p) { ws_free(c, p); p = nullptr; };      // (ws_free takes a null pointer)
    if (grow || (need_keys && !c->ws_keys)) { drop(c->keys[0]); drop(c->keys[1]); c->ws_keys = false; }
    if (grow || (need_ekeys && !c->ws_ekeys)) { drop(c->ekeys[0]); drop(c->ekeys[1]); drop(c->elist); c->ws_ekeys = false; }
    if (grow || (need_edges && !c->ws_edges)) { drop(c->tri_invalid); drop(c->unused); c->ws_edges = false; }
    if (grow || (need_mesh_ws && !c->ws_mesh)) { drop(c->cbuf[0]); drop(c->cbuf[1]); c->ws_mesh = false; }
    if (grow) c->ws_frames = frames;
    // (tuning build, the r04 diagnosis: MDVT_WS_LAYOUT=joint puts the second bank's huge list back into the queue block, as at 47b4117 --
    //  2.2 MB for a 100 x 31 frame; it takes effect when that block is made, so it is read before the layout is)
    if (need_mesh_ws && !c->ws_mesh) { const char* e = tuning_env(TUNE_WS_LAYOUT); c->huge_lists = (e && strcmp(e, "joint") == 0) ? 2 : 1; }
    const RenderWorkspaceLayout L = layout_of(c);
    if (need_keys && !c->ws_keys) {
        for (int e = 0; e < 2; ++e) {
            MDVT_HIP(c, ws_malloc(c, (void**)&c->keys[e], L.plane_bytes(), s));
            MDVT_HIP(c, hipMemsetAsync(c->keys[e], 0xFF, L.plane_bytes(), s));     // parity 0's empty value
        }
        c->key_parity = 0;
        c->ws_keys = true;
    }
    if (need_ekeys && !c->ws_ekeys) {
        for (int e = 0; e < 2; ++e) {
            MDVT_HIP(c, ws_malloc(c, (void**)&c->ekeys[e], L.plane_bytes(), s));
            MDVT_HIP(c, hipMemsetAsync(c->ekeys[e], 0xFF, L.plane_bytes(), s));
        }
        MDVT_HIP(c, ws_malloc(c, (void**)&c->elist, L.elist_bytes(), s));
        MDVT_HIP(c, hipMemsetAsync(c->elist + L.elist_count_at(), 0, L.slots * L.H * sizeof(uint32_t), s));   // counters; the reset pass keeps them 0
        c->ws_ekeys = true;
    }
    if (need_mesh_ws && !c->ws_mesh) {
        for (int e = 0; e < 2; ++e) MDVT_HIP(c, ws_malloc(c, (void**)&c->cbuf[e], L.plane_bytes(), s));   // tie side words: a word is initialised by the fragment that marks its pixel, so the plane needs no clearing
        drop(c->bigq);
        // (entry indices are 32-bit: chunk_of() keeps a launch set's slots * npx * 4 below 2^32)
        if (queue_slots_max(c->W, c->H) < 1) return fail(c, MDVT_ERR_UNSUPPORTED, "general mesh path: a %d x %d frame exceeds the 32-bit triangle queue", c->W, c->H);
        size_t pad = 0;      // (tuning build: MDVT_WS_PAD=n appends n unused bytes to the queue block)
        if (const char* e = tuning_env(TUNE_WS_PAD)) pad = (size_t)strtoull(e, nullptr, 10);
        c->bigq_bytes = L.queue_bytes(); c->bigq_counters_at = L.counters_at();
        MDVT_HIP(c, ws_malloc(c, (void**)&c->bigq, c->bigq_bytes + pad, s));
        c->ws_mesh = true;
    }
    if (need_edges && !c->ws_edges) {
        MDVT_HIP(c, ws_malloc(c, (void**)&c->tri_invalid, L.tri_invalid_bytes(), s));
        MDVT_HIP(c, ws_malloc(c, (void**)&c->unused, L.unused_bytes(), s));
        c->ws_edges = true;
    }
    return MDVT_OK;
}

bool aligned(const void* p, size_t a) { return ((uintptr_t)p % a) == 0; }

// The decree's snap (mdvt_device.h) on the host: same IEEE operations (this file is compiled with -ffp-contract=off).
int host_snap(float x, int subpix)
{
    x = fminf(fmaxf(x, -kSnapLimit), kSnapLimit);
    return (int)rintf(x * (float)subpix);
}

int grid_bits(const mdvt_ctx* c) { return c->cfg.subpixel_bits == 4 ? 4 : 8; }

// Scanline k (centre S k + S/2) is covered by the cell row c = largest i with snap(f32(i) * sy) < centre (a centre ON a vertex
// row belongs to the cells above it: bottom edges own their centres, mdvt_device.h edge_in), if that is not the last vertex
// row (k_mesh_rows derives the same per workgroup).
int ensure_rowcell(mdvt_ctx* c, hipStream_t s)
{
    if (c->rowcell && c->rowcell_bits == grid_bits(c)) return MDVT_OK;
    const int H = c->H;
    const int kSubpix = 1 << grid_bits(c);        // (shadows the compile-time grid of this translation unit on purpose)
    const float sy = (float)(((double)H + 1.0) / (double)H);
    std::vector<mdvt::RowCell> t((size_t)H);
    for (int k = 0; k < H; ++k) {
        const int Yc = k * kSubpix + kSubpix / 2;
        int ilo = (int)(((float)k + 0.5f) / sy);
        ilo = ilo < 0 ? 0 : (ilo > H - 1 ? H - 1 : ilo);
        while (ilo > 0 && host_snap((float)ilo * sy, kSubpix) >= Yc) --ilo;
        while (ilo + 1 <= H - 1 && host_snap((float)(ilo + 1) * sy, kSubpix) < Yc) ++ilo;
        mdvt::RowCell r{};
        r.c = (ilo <= H - 2) ? ilo : -1;
        r.Yt = r.c >= 0 ? host_snap((float)r.c * sy, kSubpix) : 0;
        r.Yb = r.c >= 0 ? host_snap((float)(r.c + 1) * sy, kSubpix) : 1;
        t[(size_t)k] = r;
    }
    if (!c->rowcell) MDVT_HIP(c, ws_malloc(c, (void**)&c->rowcell, (size_t)H * sizeof(mdvt::RowCell), s));
    else MDVT_HIP(c, hipDeviceSynchronize());     // a render of the other grid may still read the table
    c->rowcell_bits = grid_bits(c);
    MDVT_HIP(c, hipMemcpyAsync(c->rowcell, t.data(), (size_t)H * sizeof(mdvt::RowCell), hipMemcpyHostToDevice, s));
    MDVT_HIP(c, hipStreamSynchronize(s));      // `t` is pageable host memory
    return MDVT_OK;
}

uint32_t packed_key_rgb(const mdvt_ctx* c) { return (uint32_t)c->cfg.key_rgb[0] | ((uint32_t)c->cfg.key_rgb[1] << 8) | ((uint32_t)c->cfg.key_rgb[2] << 16); }
size_t workspace_budget_bytes(const mdvt_ctx* c) { return (size_t)(c->cfg.workspace_mib ? c->cfg.workspace_mib : 4096u) << 20; }
// the slots of per_slot bytes each that the budget affords: at least one, at most cap
int slots_afforded(const mdvt_ctx* c, size_t per_slot, int cap)
{
    const size_t afford = workspace_budget_bytes(c) / per_slot;
    return (size_t)cap > afford ? (afford < 1 ? 1 : (int)afford) : cap;
}

// What RenderArgs and MsaaArgs share: the caller's images, the staged parameters, the frame size and the slot strides.
template <class Args>
void bind_io(Args& a, const mdvt_ctx* c, const mdvt_io* io, const FrameDev* dfp)
{
    a.depth = io->depth_rgb; a.depth_pitch = io->depth_pitch; a.depth_stride = io->depth_stride;
    a.color = io->color_rgb; a.color_pitch = io->color_pitch; a.color_stride = io->color_stride;
    a.rgb[0] = io->left_rgb; a.rgb[1] = io->right_rgb; a.rgb_pitch = io->rgb_pitch; a.rgb_stride = io->rgb_stride;
    a.mask[0] = io->left_mask; a.mask[1] = io->right_mask; a.mask_pitch = io->mask_pitch; a.mask_stride = io->mask_stride;
    a.hole_counts = io->hole_counts; a.fp = dfp; a.key_rgb = packed_key_rgb(c);
    a.W = c->W; a.H = c->H; a.ws_stride_px = (size_t)c->W * c->H; a.ws_stride_tri = 2 * (size_t)(c->W - 1) * (c->H - 1);
}

// The edge filter's flags of the n frames from a.frame0 on, into the workspace slots that tri_invalid / unused start at.
template <class Args>
int filter_edges(mdvt_ctx* c, const Args& a, int n, uint8_t* tri_invalid, uint8_t* unused, hipStream_t s)
{
    MDVT_HIP(c, launch_zero_bytes(unused, (size_t)n * a.ws_stride_px, s));
    MDVT_HIP(c, launch_edge_filter(a.depth, a.depth_pitch, a.depth_stride, a.fp, a.frame0, n, a.W, a.H, c->cfg.mode == MDVT_MODE_MESH,
                                   tri_invalid, a.ws_stride_tri, unused, a.ws_stride_px, s));
    return MDVT_OK;
}

// ---- 4x multisampled render (mdvt_config.samples = 4; mdvt_msaa.hip) ---------------------------------------------------------
// What the mode does not cover is refused before anything is checked or launched, with the output named.
int msaa_refusal(mdvt_ctx* c, const mdvt_io* io, const char* mode = "multisampling (samples = 4)")
{
    const char* what = nullptr;
    if (c->cfg.edge_points) what = "edge points (mdvt_config.edge_points != 0)";
    else if (io->left_depth || io->right_depth) what = "depth planes (left_depth / right_depth)";
    else if (io->left_seed || io->right_seed) what = "seed images (left_seed / right_seed)";
    else if (io->left_maskbits || io->right_maskbits) what = "packed mask bits (left_maskbits / right_maskbits)";
    else if (!io->left_mask || !io->right_mask) what = "a NULL byte mask (left_mask / right_mask are required)";
    if (!what) return MDVT_OK;
    return fail(c, MDVT_ERR_UNSUPPORTED, "%s does not cover %s", mode, what);
}

// Launch sets of up to 16 frames, as many as workspace_mib affords (64 B/px of sample keys, 3 B/px of edge-filter flags).
int render_msaa(mdvt_ctx* c, int n_frames, const std::vector<FrameDev>& fd, const mdvt_io* io, hipStream_t s)
{
    const int W = c->W, H = c->H;
    const size_t npx = (size_t)W * (size_t)H;
    if (2 * npx >= (size_t)0xFFFFFFFFu)
        return fail(c, MDVT_ERR_UNSUPPORTED, "multisampling: a %d x %d frame has more triangles than its 32-bit draw ids can name", W, H);
    const bool rm = c->cfg.remove_edges != 0;
    int chunk = slots_afforded(c, npx * (2 * 4 * sizeof(unsigned long long) + (rm ? kNominalEdgeFlagBytesPerPx : 0)), 16);
    if (chunk > n_frames) chunk = n_frames;

    const FrameDev* dfp = nullptr;
    ParamSlot* slot = nullptr;
    int rc = stage_params(c, fd, s, &dfp, &slot);
    if (rc != MDVT_OK) return rc;
    if (rm && (rc = ensure_workspace(c, chunk, false, false, true, false, s)) != MDVT_OK) return rc;
    const bool clip = c->near_clip && c->cfg.mode == MDVT_MODE_MESH;      // (the clipping render of every frame, mdvt_near_clip.hip)
    const size_t plane_bytes = npx * 2 * 4 * sizeof(unsigned long long);       // one slot, both eyes
    if (c->msaa_frames < chunk) {
        if (c->msaa_keys) { MDVT_HIP(c, hipDeviceSynchronize()); ws_free(c, c->msaa_keys); }     // (earlier submissions may still use it)
        c->msaa_keys = nullptr; c->msaa_frames = 0;
        MDVT_HIP(c, ws_malloc(c, (void**)&c->msaa_keys, (size_t)chunk * plane_bytes, s));
        c->msaa_frames = chunk;
        c->msaa_dirty = true;
    }
    if (c->msaa_dirty) MDVT_HIP(c, hipMemsetAsync(c->msaa_keys, 0xFF, (size_t)c->msaa_frames * plane_bytes, s));
    c->msaa_dirty = false;
    if (io->hole_counts) MDVT_HIP(c, hipMemsetAsync(io->hole_counts, 0, 2 * (size_t)n_frames * sizeof(uint32_t), s));

    MsaaArgs a{};
    bind_io(a, c, io, dfp);
    a.keys = c->msaa_keys;
    a.tri_invalid = rm ? c->tri_invalid : nullptr; a.unused = rm ? c->unused : nullptr;
    a.mode = c->cfg.mode; a.cull = c->cfg.cull; a.pattern = c->cfg.sample_pattern; a.resolve = c->cfg.sample_resolve;
    for (int f0 = 0; f0 < n_frames; f0 += chunk) {
        const int n = n_frames - f0 < chunk ? n_frames - f0 : chunk;
        a.frame0 = f0;
        if (rm && (rc = filter_edges(c, a, n, c->tri_invalid, c->unused, s)) != MDVT_OK) return rc;
        c->msaa_dirty = true;
        if (clip) MDVT_HIP(c, MDVT_GRID_CALL(c, launch_near_clip_render, a, n, 4, nullptr, s));
        else MDVT_HIP(c, MDVT_GRID_CALL(c, launch_msaa_render, a, n, s));
        c->msaa_dirty = false;
    }
    MDVT_HIP(c, hipEventRecord(slot->done, s));
    return MDVT_OK;
}

// ---- near-plane clipping, single sample (mdvt_set_near_clip; mdvt_near_clip.hip) -------------------------------------------------
// Runs after the single-sample kernels have rendered every frame of the batch, on the same stream: a detect kernel flags the (frame,
// eye) where some triangle may straddle the plane, and the key-plane kernels re-render only those eyes (the others leave at once;
// nothing is read back).  Launch sets of up to 16 frames, as many as workspace_mib affords (16 B/px of keys; with remove_edges the
// edge filter's flags of the slots the render before has already allocated).
int render_near_clip_gate(mdvt_ctx* c, int n_frames, const FrameDev* dfp, const mdvt_io* io, hipStream_t s)
{
    const int W = c->W, H = c->H;
    const size_t npx = (size_t)W * (size_t)H;
    const bool rm = c->cfg.remove_edges != 0;
    const size_t per_slot = npx * 2 * sizeof(unsigned long long);
    int chunk = slots_afforded(c, per_slot, 16);
    if (rm && chunk > c->ws_frames) chunk = c->ws_frames;        // (the render before has made at least one slot of edge flags)
    if (chunk > n_frames) chunk = n_frames;
    if (chunk < 1) return fail(c, MDVT_ERR_INVALID_ARG, "near-plane clipping: no workspace slot for the edge filter");
    if (c->clip_frames < chunk) {
        if (c->clip_keys) { MDVT_HIP(c, hipDeviceSynchronize()); ws_free(c, c->clip_keys); ws_free(c, c->clip_flags); }     // (earlier submissions may still use them)
        c->clip_keys = nullptr; c->clip_flags = nullptr; c->clip_frames = 0;
        MDVT_HIP(c, ws_malloc(c, (void**)&c->clip_keys, (size_t)chunk * per_slot, s));
        MDVT_HIP(c, ws_malloc(c, (void**)&c->clip_flags, (size_t)chunk * 2 * sizeof(uint32_t), s));
        c->clip_frames = chunk;
        c->clip_dirty = true;
    }
    if (c->clip_dirty) MDVT_HIP(c, hipMemsetAsync(c->clip_keys, 0xFF, (size_t)c->clip_frames * per_slot, s));
    c->clip_dirty = false;

    MsaaArgs a{};
    bind_io(a, c, io, dfp);
    a.keys = c->clip_keys;
    a.tri_invalid = rm ? c->tri_invalid : nullptr; a.unused = rm ? c->unused : nullptr;
    a.mode = c->cfg.mode; a.cull = c->cfg.cull;
    for (int f0 = 0; f0 < n_frames; f0 += chunk) {
        const int n = n_frames - f0 < chunk ? n_frames - f0 : chunk;
        a.frame0 = f0;
        MDVT_HIP(c, hipMemsetAsync(c->clip_flags, 0, (size_t)n * 2 * sizeof(uint32_t), s));
        if (rm) { if (int rc = filter_edges(c, a, n, c->tri_invalid, c->unused, s)) return rc; }      // (mesh mode: near_clip)
        c->clip_dirty = true;
        MDVT_HIP(c, MDVT_GRID_CALL(c, launch_near_clip_render, a, n, 1, c->clip_flags, s));
        c->clip_dirty = false;
    }
    return MDVT_OK;
}

}  // namespace

extern "C" {

int mdvt_version(void) { return MDVT_VERSION; }

const char* mdvt_last_error(const mdvt_ctx* ctx) { return ctx ? ctx->err.c_str() : g_create_error.c_str(); }

int mdvt_create(mdvt_ctx** out, int device, int width, int height, uint32_t flags)
{
    if (!out) return fail(nullptr, MDVT_ERR_INVALID_ARG, "out is NULL");
    *out = nullptr;
    if (flags != 0) return fail(nullptr, MDVT_ERR_INVALID_ARG, "flags must be 0");
    if (width < 1 || height < 1 || width > 65535 || height > 32767)
        return fail(nullptr, MDVT_ERR_INVALID_ARG, "frame size %dx%d out of range (1..65535 x 1..32767)", width, height);
    int count = 0;
    hipError_t e = hipGetDeviceCount(&count);
    if (e != hipSuccess || count <= 0)
        return fail(nullptr, MDVT_ERR_NO_DEVICE, "no HIP device available (%s); this library has no CPU fallback",
                    e == hipSuccess ? "device count is 0" : hipGetErrorString(e));
    if (device < 0 || device >= count) return fail(nullptr, MDVT_ERR_INVALID_ARG, "device %d out of range (0..%d)", device, count - 1);
    hipDeviceProp_t prop;
    if ((e = hipGetDeviceProperties(&prop, device)) != hipSuccess)
        return fail(nullptr, MDVT_ERR_HIP, "hipGetDeviceProperties: %s", hipGetErrorString(e));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(nullptr, MDVT_ERR_NO_DEVICE, "device %d is %s; this library is built for gfx950 (MI355X) only", device, prop.gcnArchName);
    mdvt_ctx* c = new (std::nothrow) mdvt_ctx();
    if (!c) return fail(nullptr, MDVT_ERR_OOM, "out of host memory");
    c->device = device; c->W = width; c->H = height;
    c->pool_tag = device;
    if (const char* t = tuning_env(TUNE_POOL_TAG)) c->pool_tag = atoi(t);
    { const char* e = getenv("MDVT_MESH_CONV"); c->opt_mesh_conv = e && e[0] == '1'; }     // the library's one switch, read here and nowhere else
    c->cfg.mode = MDVT_MODE_POINTS; c->cfg.ipd_m = 0.063; c->cfg.max_depth = 100.0;   // argparse defaults (sr:284, 288)
    *out = c;
    return MDVT_OK;
}

// ---- The banks' side stream and events: process-wide, never destroyed ------------------------------------------------------
// r05: three soak processes in ~3 000 multi-frame sweep jobs (300 k contexts that had used banks) died of a signal -- never one of
// 3 500 single-frame jobs (1.4 M contexts) -- and the native backtrace of the third (tools/probe/segv_trace.c) is the HSA runtime's
// own callback thread faulting inside libamdhip64, not a frame of this library.  What only the bank path has is a stream and four
// events created by a context and destroyed with it; whatever the runtime's handler still holds of them after the
// hipDeviceSynchronize of mdvt_destroy, the library no longer destroys them: they wait here for the next context of the same GPU
// that uses banks (the treatment the pinned parameter blocks and the workspace blocks got for their own reasons).
struct BankRes { hipStream_t side; hipEvent_t ev[4]; int device; };
static std::mutex g_bank_mutex;
static std::vector<BankRes>& bank_pool() { static std::vector<BankRes>* p = new std::vector<BankRes>(); return *p; }      // (leaked on purpose)

static hipError_t bank_res_take(mdvt_ctx* c)
{
    {
        std::lock_guard<std::mutex> lock(g_bank_mutex);
        auto& pool = bank_pool();
        for (size_t k = pool.size(); k-- > 0;)
            if (pool[k].device == c->device) {
                c->side = pool[k].side; c->ev_start = pool[k].ev[0]; c->ev_join = pool[k].ev[1]; c->ev_vert[0] = pool[k].ev[2]; c->ev_vert[1] = pool[k].ev[3];
                pool.erase(pool.begin() + (long)k);
                return hipSuccess;
            }
    }
    // built in locals, handed to the context only when complete: a half-made set must not leave c->side set (every later banked
    // render would skip this function and record a null event); what was made of it is abandoned, like everything of this kind
    BankRes r{};
    hipError_t e = hipStreamCreateWithFlags(&r.side, hipStreamNonBlocking);
    for (hipEvent_t& ev : r.ev)
        if (e == hipSuccess) e = hipEventCreateWithFlags(&ev, hipEventDisableTiming);
    if (e != hipSuccess) return e;
    c->side = r.side; c->ev_start = r.ev[0]; c->ev_join = r.ev[1]; c->ev_vert[0] = r.ev[2]; c->ev_vert[1] = r.ev[3];
    return hipSuccess;
}
// (the caller has synchronised the device: nothing submitted still uses them)
static void bank_res_give(mdvt_ctx* c)
{
    if (!c->side) return;
    if (c->ev_start && c->ev_join && c->ev_vert[0] && c->ev_vert[1]) {
        std::lock_guard<std::mutex> lock(g_bank_mutex);
        bank_pool().push_back({c->side, {c->ev_start, c->ev_join, c->ev_vert[0], c->ev_vert[1]}, c->device});
    }       // (a half-created set -- an error in bank_res_take -- is abandoned, not destroyed)
    c->side = nullptr; c->ev_start = c->ev_join = c->ev_vert[0] = c->ev_vert[1] = nullptr;
}

static void free_telea(mdvt_ctx* c)
{
    mdvt::TeleaWorkspace& w = c->telea;
    void* ptrs[] = {w.stamp, w.T, w.img, w.need, w.nlist, w.counts, w.remaining, w.last_round};   // offs / ncounts live inside counts
    for (void* p : ptrs) if (p) ws_free(c, p);
    w = mdvt::TeleaWorkspace{};
    c->telea_images = 0; c->telea_rounds = 0;
}

static void free_telea_heap(mdvt_ctx* c)
{
    if (c->heap_ws) ws_free(c, c->heap_ws);
    if (c->heap_remaining) ws_free(c, c->heap_remaining);
    c->heap_ws = nullptr; c->heap_remaining = nullptr; c->heap_images = 0;
}

int mdvt_destroy(mdvt_ctx* c)
{
    if (!c) return MDVT_OK;
    DeviceGuard g(c->device);
    (void)hipDeviceSynchronize();
    bank_res_give(c);
    for (auto& sl : c->slots) {
        pool_give(sl.host, sl.dev, sl.capacity * sizeof(FrameDev), c->pool_tag);
        if (sl.done) (void)hipEventDestroy(sl.done);
    }
    void* const render_ws[] = {c->hugeq2, c->keys[0], c->ekeys[0], c->cbuf[0], c->keys[1], c->ekeys[1], c->cbuf[1], c->bigq, c->tri_invalid, c->unused, c->elist,
                               c->row_counts, c->wave_counts, c->divcheck, c->rowcell, c->msaa_keys, c->clip_keys, c->clip_flags};
    for (void* p : render_ws) ws_free(c, p);      // (ws_free takes a null pointer)
    if (c->div_done) (void)hipEventDestroy(c->div_done);
    pool_give(c->telea_levels_host, nullptr, 64, -1);
    free_telea(c);
    free_telea_heap(c);
    void* const other_ws[] = {c->ni_ws, c->ffv1_ws, c->ffv1_dec_ws, c->conv_ws};
    for (void* p : other_ws) ws_free(c, p);
    delete c;
    return MDVT_OK;
}

int mdvt_set_config(mdvt_ctx* c, const mdvt_config* cfg)
{
    if (!c) return MDVT_ERR_INVALID_ARG;
    if (!cfg) return fail(c, MDVT_ERR_INVALID_ARG, "cfg is NULL");
    if (cfg->mode != MDVT_MODE_POINTS && cfg->mode != MDVT_MODE_MESH) return fail(c, MDVT_ERR_INVALID_ARG, "unknown mode %d", cfg->mode);
    if (!(cfg->max_depth > 0.0)) return fail(c, MDVT_ERR_INVALID_ARG, "max_depth must be > 0");
    if (!(cfg->ipd_m >= 0.0)) return fail(c, MDVT_ERR_INVALID_ARG, "ipd_m must be >= 0");
    if (cfg->edge_points < 0 || cfg->edge_points > 2) return fail(c, MDVT_ERR_INVALID_ARG, "edge_points must be 0, 1 or 2");
    if (cfg->edge_points && !cfg->remove_edges) return fail(c, MDVT_ERR_INVALID_ARG, "edge_points needs remove_edges (sr:589)");
    if (cfg->cull < 0 || cfg->cull > 2) return fail(c, MDVT_ERR_INVALID_ARG, "cull must be 0 (none), 1 (back) or 2 (front)");
    if (cfg->subpixel_bits != 0 && cfg->subpixel_bits != 4 && cfg->subpixel_bits != 8)
        return fail(c, MDVT_ERR_INVALID_ARG, "subpixel_bits must be 0 (default: 8), 4 or 8 -- the grids this build's rasterisers are compiled for");
    if (cfg->samples != 0 && cfg->samples != 1 && cfg->samples != 4)
        return fail(c, MDVT_ERR_INVALID_ARG, "samples must be 0 or 1 (single sample) or 4 (4x multisampled), got %d", (int)cfg->samples);
    if (cfg->sample_pattern > 1) return fail(c, MDVT_ERR_INVALID_ARG, "sample_pattern must be 0 (standard) or 1 (SwiftShader), got %d", (int)cfg->sample_pattern);
    if (cfg->sample_resolve > 1) return fail(c, MDVT_ERR_INVALID_ARG, "sample_resolve must be 0 (rounded mean) or 1 (SwiftShader), got %d", (int)cfg->sample_resolve);
    // (advisor r04: the field took over a reserved one -- a caller built against 0.11 that left it uninitialised must not get an
    //  arbitrary budget silently: anything above 1 TiB is refused, small values are honoured down to one slot)
    if (cfg->workspace_mib > (1u << 20)) return fail(c, MDVT_ERR_INVALID_ARG, "workspace_mib %u out of range (0 = default 4096, at most 1048576)", cfg->workspace_mib);
    c->cfg = *cfg;
    c->cfg_set = true;
    return MDVT_OK;
}

int mdvt_set_near_clip(mdvt_ctx* c, int32_t near_clip)
{
    if (!c) return MDVT_ERR_INVALID_ARG;
    if (near_clip != 0 && near_clip != 1)
        return fail(c, MDVT_ERR_INVALID_ARG, "near_clip must be 0 (drop a triangle that crosses the near plane) or 1 (clip it), got %d", (int)near_clip);
    c->near_clip = near_clip;
    return MDVT_OK;
}

int mdvt_selftest(mdvt_ctx* c, int which, uint64_t seed, uint64_t* h_mismatches)
{
    if (!c) return MDVT_ERR_INVALID_ARG;
    if (!h_mismatches || which < 0 || which > 2) return fail(c, MDVT_ERR_INVALID_ARG, "mdvt_selftest: which must be 0..2, h_mismatches not NULL");
    DeviceGuard g(c->device);
    unsigned long long* d = nullptr;
    MDVT_HIP(c, hipMalloc((void**)&d, sizeof(unsigned long long)));
    hipError_t e = launch_selftest(which, (unsigned long long)seed, d, nullptr);
    unsigned long long h = 0;
    if (e == hipSuccess) e = hipMemcpy(&h, d, sizeof h, hipMemcpyDeviceToHost);
    (void)hipFree(d);
    if (e != hipSuccess) return fail(c, MDVT_ERR_HIP, "mdvt_selftest: %s", hipGetErrorString(e));
    *h_mismatches = (uint64_t)h;
    return MDVT_OK;
}

// ---- The steps of mdvt_render_stereo_batch, in its order ---------------------------------------------------------------------
struct BatchFlags { bool no_byte_mask, zout, want_bits, near_clip; };

// Everything that is refused before the device is touched.
static int validate_batch(mdvt_ctx* c, int n_frames, const mdvt_frame_params* params, const mdvt_io* io, BatchFlags& f)
{
    if (n_frames <= 0 || !params || !io) return fail(c, MDVT_ERR_INVALID_ARG, "n_frames/params/io invalid");
    if (!io->depth_rgb || !io->color_rgb || !io->left_rgb || !io->right_rgb)
        return fail(c, MDVT_ERR_INVALID_ARG, "depth_rgb, color_rgb and left/right rgb buffers are required");
    if (c->cfg.samples == 4) { if (int rc = msaa_refusal(c, io)) return rc; }
    f.near_clip = c->near_clip && c->cfg.mode == MDVT_MODE_MESH;     // (points: a GL drops a point behind the plane, as the decree does)
    if (f.near_clip) {
        if (int rc = msaa_refusal(c, io, "near-plane clipping (near_clip = 1)")) return rc;
        // fan triangle f of source triangle d is drawn as 2 d + f: 4 (W - 1) (H - 1) ids in the 32 bits of a key
        if (c->W >= 2 && c->H >= 2 && 4 * (uint64_t)(c->W - 1) * (uint64_t)(c->H - 1) >= (uint64_t)0xFFFFFFFFu)
            return fail(c, MDVT_ERR_UNSUPPORTED, "near-plane clipping: a %d x %d frame has more fan triangles than its 32-bit draw ids can name", c->W, c->H);
    }
    // The byte masks may be left out (both NULL) by a caller that takes the packed mask instead -- where the compaction is fused
    // into the render kernel (pure-shift point frames: checked per launch set in submit_run); everywhere else they are required.
    f.no_byte_mask = !io->left_mask && !io->right_mask && io->left_maskbits && io->right_maskbits;
    if (!f.no_byte_mask && (!io->left_mask || !io->right_mask))
        return fail(c, MDVT_ERR_INVALID_ARG, "left/right mask buffers are required (both may be NULL only when maskbits are given)");
    const int W = c->W, H = c->H;
    if (W < 2 || H < 2) return fail(c, MDVT_ERR_INVALID_ARG, "rendering needs at least a 2x2 frame");
    if (io->depth_pitch < (size_t)3 * W || io->color_pitch < (size_t)3 * W || io->rgb_pitch < (size_t)3 * W ||
        (!f.no_byte_mask && io->mask_pitch < (size_t)W))
        return fail(c, MDVT_ERR_INVALID_ARG, "a pitch is smaller than one row");   // sr:507 shape assert
    f.zout = io->left_depth || io->right_depth;
    if (f.zout && io->zout_pitch < (size_t)4 * W) return fail(c, MDVT_ERR_INVALID_ARG, "zout_pitch smaller than one row");
    if (io->left_seed || io->right_seed) {
        if (!io->left_seed || !io->right_seed) return fail(c, MDVT_ERR_INVALID_ARG, "seed images need both eyes");
        if (!c->cfg.remove_edges) return fail(c, MDVT_ERR_INVALID_ARG, "seed images need remove_edges (the infill-mask mode of sr:568-570)");
        if (io->seed_pitch < (size_t)3 * W) return fail(c, MDVT_ERR_INVALID_ARG, "seed_pitch smaller than one row");
    }
    f.want_bits = io->left_maskbits || io->right_maskbits;
    if (f.want_bits) {
        if (!io->left_maskbits || !io->right_maskbits) return fail(c, MDVT_ERR_INVALID_ARG, "maskbits need both eyes");
        if (io->maskbits_pitch < (size_t)4 * (((size_t)W + 31) / 32) || io->maskbits_pitch % 4 != 0 || io->maskbits_stride % 4 != 0 ||
            ((uintptr_t)io->left_maskbits % 4) || ((uintptr_t)io->right_maskbits % 4))
            return fail(c, MDVT_ERR_INVALID_ARG, "maskbits rows must be dword aligned and at least 4*ceil(W/32) bytes");
    }
    return MDVT_OK;
}

// Pure-shift point frames: the disparity's division proven short per parameter set (FrameDev.div_slot).  A new set costs one
// launch of 65536 threads on this stream, once per context; clips have one set, or one per distinct field of view.
// The checks run on the stream of the call that brought their set in; a call on another stream (a pure-shift point render
// without hole counts uses no other workspace, so nothing else orders it after that call) first waits for the latest check,
// and with it for every earlier one and the table's fill: each check is recorded after a wait for the one before it, whichever
// stream that was on.
static int assign_div_slots(mdvt_ctx* c, std::vector<FrameDev>& fd, hipStream_t s)
{
    bool ordered = false;
    for (FrameDev& f : fd) {
        if (f.general) continue;
        if (!ordered && c->div_done && c->div_stream != s) MDVT_HIP(c, hipStreamWaitEvent(s, c->div_done, 0));
        ordered = true;
        std::array<uint32_t, 3> key;
        memcpy(&key[0], &f.mult, 4); memcpy(&key[1], &f.scale, 4); memcpy(&key[2], &f.dl, 4);
        int slot = -1;
        for (size_t q = c->div_keys.size(); q-- > 0;) if (c->div_keys[q] == key) { slot = (int)q; break; }
        if (slot < 0 && c->div_keys.size() < (size_t)mdvt::kDivSlots) {
            if (!c->divcheck) {
                MDVT_HIP(c, ws_malloc(c, (void**)&c->divcheck, mdvt::kDivSlots * sizeof(uint32_t), s));
                MDVT_HIP(c, hipMemsetAsync(c->divcheck, 0, mdvt::kDivSlots * sizeof(uint32_t), s));
            }
            if (!c->div_done) MDVT_HIP(c, hipEventCreateWithFlags(&c->div_done, hipEventDisableTiming));
            slot = (int)c->div_keys.size();
            MDVT_HIP(c, MDVT_GRID_CALL(c, launch_divcheck, f.mult, f.scale, f.dl, c->divcheck + slot, s));
            MDVT_HIP(c, hipEventRecord(c->div_done, s));
            c->div_stream = s;
            c->div_keys.push_back(key);
        }
        f.div_slot = slot;
    }
    return MDVT_OK;
}

// The arithmetic of a frame (pure shift or general) is its own property, never its batch
// neighbours': consecutive frames of one kind form a run, every run gets its own launches.
struct Run { int f0, f1, general, conv, craster; };  // general = "takes the global-key kernels"; conv = k_mesh_conv (mesh, convergence only);
                                                     // craster = general, but every frame convergence-only: k_mesh_raster_conv
static void build_runs(const mdvt_ctx* c, const RenderPlan& plan, const std::vector<FrameDev>& fd, std::vector<Run>& runs)
{
    const int W = c->W, H = c->H;
    // A pure-shift frame wider than the LDS row kernels can hold (10 240 px for points, ~4 300 for the mesh with edge
    // points) is rendered by the global-key kernels instead -- with its own pure-shift arithmetic (FrameDev.general
    // stays 0), so the pixels do not depend on which kernels ran.  MDVT_FORCE_GLOBAL=1 sends every frame that way (tests).
    const bool wide = !MDVT_GRID_CALL(c, render_fits_lds, plan, W) || tuning_env(TUNE_FORCE_GLOBAL) != nullptr;
    bool conv_kernel = false;
    if (plan.mode == MDVT_MODE_MESH && !wide) {
        RenderArgs probe{};
        probe.W = W; probe.H = H;
        conv_kernel = MDVT_GRID_CALL(c, mesh_conv_supported, plan, probe);
    }
    for (int k = 0; k < (int)fd.size(); ++k) {
        const int cv = (conv_kernel && fd[(size_t)k].conv_band) ? 1 : 0;
        const int g = (!cv && (wide || fd[(size_t)k].general || fd[(size_t)k].erow_wild)) ? 1 : 0;
        const int cr = (g && !wide && plan.mode == MDVT_MODE_MESH && fd[(size_t)k].conv_band) ? 1 : 0;
        if (runs.empty() || runs.back().general != g || runs.back().conv != cv || runs.back().craster != cr) runs.push_back({k, k + 1, g, cv, cr});
        else runs.back().f1 = k + 1;
    }
}

// frames per launch set.  Point splat, general: two frames keep the 64-bit key buffers (33 MB per 1080p frame)
// inside the 256 MiB Infinity Cache between splat and resolve (measured +12 %); the mesh needs the slack of
// eight (rows full of slivers leave a long tail), and the edge filter alone streams, so 8 as well.
static int chunk_of(const mdvt_ctx* c, const RenderPlan& plan, const Run& r, int tuned_chunk)
{
    const int n = r.f1 - r.f0;
    if (!(r.general || plan.remove_edges || (r.conv && plan.edge_points))) return n;                  // no workspace: the whole run in one launch
    // (points, general path: four slots -- one launch set of four frames, or banks of two (submit_run); two slots until r04:
    //  1080p convergence 26.7 k -> 28.2 k frames/s, 4K pose + contention 5.4 k -> 6.1 k)
    int ws_chunk = (r.general && plan.mode == MDVT_MODE_POINTS) ? 4 : kWorkspaceChunk;
    if (r.general && plan.mode == MDVT_MODE_MESH) {
        ws_chunk = 2 * kWorkspaceChunk;      // 16: measured -4 % (convergence) / -11 % (pose) vs 8
        // ~64 B/px per slot (z keys, tie side words, triangle queue; until r04 also 32 B/px of vertex records): 2.1 GB at 1080p,
        // 8.5 GB at 4K; the queue's entry indices are 32-bit, so very large frames get fewer slots (4 entries per pixel and slot)
        const size_t fit = queue_slots_max(c->W, c->H);
        if ((size_t)ws_chunk > fit) ws_chunk = fit < 1 ? 1 : (int)fit;
        // ... and the slots have to fit the context's workspace budget (mdvt_config.workspace_mib, default 4 GiB: 16 slots at
        // 1080p, 8 at 3840 x 2160 -- where 16 would be 8.5 GB): per slot and pixel 16 B of z keys, 16 B of tie side words,
        // 32 B of triangle queue, with edge points 28 B of edge keys, their list and the vertex list, 3 B of filter flags
        ws_chunk = slots_afforded(c, nominal_slot_bytes(c->W, c->H, plan.edge_points, plan.remove_edges), ws_chunk);
    }
    // pure-shift mesh rows with edge removal: a launch is (frames x 135 bands) workgroups for 512 slots -- 8 frames
    // leave the chip 30 % idle in the last wave of workgroups (476 -> see DESIGN.md); the workspace is 11 B/px per frame
    // (points with edge removal likewise since r04: every launch set ends with k_edge_rows_exact, a handful of workgroups the
    //  stream waits for -- once per 32 frames instead of once per 8)
    if (!r.general) ws_chunk = 4 * kWorkspaceChunk;
    if (tuned_chunk) ws_chunk = tuned_chunk;
    if (r.general && ws_chunk > 32) ws_chunk = 32;        // one parity bit per z-key slot (uint32_t key_parity)
    return n < ws_chunk ? n : ws_chunk;
}

// The hole counts' per-row and per-wave counters of `frames` frames in flight, grown on demand.
static int ensure_count_buffers(mdvt_ctx* c, int frames, hipStream_t s)
{
    if (c->row_counts_frames >= frames) return MDVT_OK;
    if (c->row_counts) { MDVT_HIP(c, hipDeviceSynchronize()); ws_free(c, c->row_counts); ws_free(c, c->wave_counts); }     // (earlier submissions may still count into it)
    c->row_counts = nullptr; c->wave_counts = nullptr; c->row_counts_frames = 0;
    MDVT_HIP(c, ws_malloc(c, (void**)&c->row_counts, (size_t)frames * 2 * c->H * sizeof(uint32_t), s));
    MDVT_HIP(c, ws_malloc(c, (void**)&c->wave_counts, (size_t)frames * c->H * 16 * sizeof(uint32_t), s));
    c->row_counts_frames = frames;
    return MDVT_OK;
}

// An earlier general-path submission stopped between splat and resolve: re-establish the EMPTY invariant the resolve pass normally maintains.
static int reset_dirty_keys(mdvt_ctx* c, const RenderWorkspaceLayout& L, hipStream_t s)
{
    for (int e = 0; e < 2; ++e) {
        if (c->keys[e]) MDVT_HIP(c, hipMemsetAsync(c->keys[e], 0xFF, L.plane_bytes(), s));
        if (c->ekeys[e]) MDVT_HIP(c, hipMemsetAsync(c->ekeys[e], 0xFF, L.plane_bytes(), s));
    }
    if (c->elist) MDVT_HIP(c, hipMemsetAsync(c->elist + L.elist_count_at(), 0, L.slots * L.H * sizeof(uint32_t), s));
    c->key_parity = 0;
    return MDVT_OK;
}

// Points RenderArgs at the workspace slots [slot0, ...) of a launch set: the whole workspace (slot0 = 0, bank 0) or a bank's half
// (slot0 = bank * bank_slots).  Allocates nothing: the second bank's separate huge list is made by submit_run.
static void bind_workspace(RenderArgs& a, const mdvt_ctx* c, const RenderWorkspaceLayout& L, int slot0, int bank, int bank_slots)
{
    const size_t s0 = (size_t)slot0;
    auto at = [](auto* p, size_t off) -> decltype(p) { return p ? p + off : nullptr; };
    for (int e = 0; e < 2; ++e) {
        a.keys[e] = at(c->keys[e], s0 * L.npx);
        a.ekeys[e] = at(c->ekeys[e], s0 * L.npx);
        a.cbuf[e] = at(c->cbuf[e], s0 * L.npx);
    }
    a.elist = at(c->elist, s0 * L.elist_stride());
    a.elist_count = at(c->elist, L.elist_count_at() + s0 * L.H);
    a.vlist = at(c->elist, L.vlist_at() + s0 * L.npx);
    a.vlist_count = at(c->elist, L.vlist_count_at() + s0);
    a.tri_invalid = at(c->tri_invalid, s0 * L.ntri);
    a.unused = at(c->unused, s0 * L.npx);
    if (!c->bigq) return;
    a.bigq = c->bigq + s0 * L.queue_stride(); a.bigq_cap = (uint32_t)L.bigq_cap();
    a.bigq_count = c->bigq + L.counters_at() + L.bank_counters_at(bank, bank_slots);      // (counters and prefix sums of a set; 16-byte aligned)
    // The second bank's own huge list: a separate allocation, made when banks are first used (r04: with both lists in the
    // queue's block a 100 x 31 frame's block passed 2 MB and left the runtime's fragment cache -- see the workspace pool above).
    a.hugeq = c->bigq + L.huge_at();      // (8-byte aligned: entries are uint2)
    if (bank) a.hugeq = L.huge_lists == 2 ? a.hugeq + L.huge_list_dwords() : c->hugeq2;
    a.tie_flag = c->bigq + L.tie_flag_at() + s0;
    a.tie_tiles = c->bigq + L.tie_tiles_at() + s0 * L.tie_tiles_stride();
    a.tie_words = (int32_t)L.tie_words; a.tie_tiles_x = (c->W + mdvt::kTieTile - 1) / mdvt::kTieTile;
}

// (every way out of the bank loop joins the side stream back into the caller's: an error return must not leave the side
//  stream working on its half of the workspace -- and on the caller's output buffers -- behind the caller's back; advisor, r04)
struct BankJoin {
    mdvt_ctx* c; hipStream_t s_call; bool armed;
    ~BankJoin() {
        if (!armed) return;
        if (hipEventRecord(c->ev_join, c->side) != hipSuccess || hipStreamWaitEvent(s_call, c->ev_join, 0) != hipSuccess) (void)hipStreamSynchronize(c->side);
    }
};

// One run's launch sets of up to `chunk` frames; `base`: everything of RenderArgs but the workspace.
static int submit_run(mdvt_ctx* c, RenderPlan plan, const Run& r, int chunk, const RenderArgs& base, const RenderWorkspaceLayout& L,
               const std::vector<FrameDev>& fd, const BatchFlags& bf, hipStream_t s_call)
{
    const int W = c->W, H = c->H;
    plan.general = r.general; plan.conv = r.conv; plan.conv_raster = r.craster;
    // Posed / converged mesh frames in more than one launch set: the sets take turns on two halves ("banks") of the workspace slots
    // and on two streams, a set starting when the vertex pass of the set before it is through -- the path's stages wait for
    // different things (the vertex pass for its stores, the rasteriser for its atomics), and the next set's vertex pass and edge
    // filter fill the rasteriser's waits: 32 frames of 1080p product default +3 %, mesh + convergence +4 %, mesh under a pose +7 %,
    // 8 frames of 4K pose + contention (C4) +10 %; a run that fits ONE launch set stays as it is (16 frames: two sets of 8 lose 1.5 %).
    // Points on the general path likewise (splat, then resolve: the next set's splat beside this set's resolve): C4 points +13 %.
    const bool bankable = r.general && !r.conv && !bf.want_bits && !base.hole_counts && tuning_env(TUNE_WS_CHUNK) == nullptr;
    bool banks = bankable && chunk >= 2 && r.f1 - r.f0 > chunk;
    int bank_slots = chunk / 2;
    // r05: a posed mesh run that FITS one launch set is split into two sets on the two banks all the same when each half is large
    // enough to fill the chip by itself (3 frames of 4K = 24.9 M pixels: 6 to 8 frames of C4's shape) -- since the vertex records went (64 B/px per slot, was 96) the
    // 8 frames of C4 are one set of 8 slots, and its cell walk (VALU) and resolve (HBM) ran one after the other again
    if (bankable && !banks && plan.mode == MDVT_MODE_MESH && r.f1 - r.f0 <= chunk && r.f1 - r.f0 >= 4 &&
        (size_t)((r.f1 - r.f0) / 2) * (size_t)W * (size_t)H >= (size_t)3 * 3840 * 2160) {
        banks = true;
        bank_slots = (r.f1 - r.f0) / 2;
    }
    BankJoin bank_join{c, s_call, false};
    if (banks) {
        chunk = bank_slots;
        if (!c->side) MDVT_HIP(c, bank_res_take(c));        // (process-wide: see bank_res_take)
        MDVT_HIP(c, hipEventRecord(c->ev_start, s_call));            // (the inputs, the parameter block, the runs before this one)
        MDVT_HIP(c, hipStreamWaitEvent(c->side, c->ev_start, 0));
        bank_join.armed = true;
    }
    int set = 0;
    for (int f0 = r.f0; f0 < r.f1; f0 += chunk, ++set) {
        plan.n = (r.f1 - f0 < chunk) ? r.f1 - f0 : chunk;
        const int bank = banks ? (set & 1) : 0, slot0 = bank * bank_slots;
        hipStream_t const s_set = bank ? c->side : s_call;
        if (bank && c->bigq && c->huge_lists != 2 && !c->hugeq2) MDVT_HIP(c, ws_malloc(c, (void**)&c->hugeq2, L.huge_list_dwords() * sizeof(uint32_t), s_set));
        RenderArgs a = base;
        bind_workspace(a, c, L, slot0, bank, bank_slots);
        if (banks) {
            if (set > 0) MDVT_HIP(c, hipStreamWaitEvent(s_set, c->ev_vert[bank ^ 1], 0));      // (the set before this one has projected its vertices / splatted its points)
            plan.after_vertices = c->ev_vert[bank];
        }
        a.frame0 = f0;
        if (plan.remove_edges) { if (int rc = filter_edges(c, a, plan.n, a.tri_invalid, a.unused, s_set)) return rc; }
        if (bf.no_byte_mask && !MDVT_GRID_CALL(c, points_fused_bits_applies, plan, a))
            return fail(c, MDVT_ERR_INVALID_ARG, "the byte masks may be NULL only where the mask compaction is fused into the render "
                        "(points mode, pure stereo shift, no edge removal, W %% 4 == 0, W <= 4096, dword-aligned image pointers, pitches and strides)");
        a.key_parity = c->key_parity >> slot0;
        plan.edge_rows_max = 0;
        if (!r.general && !r.conv && plan.edge_points)
            for (int k = f0; k < f0 + plan.n; ++k)
                if (fd[(size_t)k].erow_lo < fd[(size_t)k].erow_hi)
                    plan.edge_rows_max = std::max(plan.edge_rows_max, fd[(size_t)k].erow_hi - fd[(size_t)k].erow_lo + 1);
        hipError_t e = MDVT_GRID_CALL(c, launch_render, plan, a, s_set);
        plan.after_vertices = nullptr;
        if (r.general && e == hipSuccess) c->key_parity ^= (plan.n >= 32 ? 0xFFFFFFFFu : ((1u << plan.n) - 1u)) << slot0;   // these slots' next use has the other parity
        if (e == hipErrorNotSupported) return fail(c, MDVT_ERR_UNSUPPORTED, "render mode %d is not built yet", plan.mode);
        if (e != hipSuccess) return fail(c, MDVT_ERR_HIP, "render launch failed: %s", hipGetErrorString(e));
        if ((bf.want_bits || a.hole_counts) && !plan.fused_bits) MDVT_HIP(c, launch_pack_mask(a, plan.n, s_set));
        if (a.hole_counts && !plan.fused_bits) MDVT_HIP(c, launch_reduce_counts(a, plan.n, s_set));
    }
    if (banks) {
        MDVT_HIP(c, hipEventRecord(c->ev_join, c->side));
        MDVT_HIP(c, hipStreamWaitEvent(s_call, c->ev_join, 0));
        bank_join.armed = false;
    }
    return MDVT_OK;
}

int mdvt_render_stereo_batch(mdvt_ctx* c, int n_frames, const mdvt_frame_params* params, const mdvt_io* io, void* stream)
{
    if (!c) return MDVT_ERR_INVALID_ARG;
    BatchFlags bf{};
    int rc = validate_batch(c, n_frames, params, io, bf);
    if (rc != MDVT_OK) return rc;
    DeviceGuard g(c->device);
    hipStream_t const s = (hipStream_t)stream;
    std::vector<FrameDev> fd((size_t)n_frames);
    int any_general_frame = 0;
    for (int k = 0; k < n_frames; ++k) {
        if ((rc = fill_frame_dev(c, params[k], fd[(size_t)k])) != MDVT_OK) return rc;
        any_general_frame |= fd[(size_t)k].general;
        fd[(size_t)k].div_slot = -1;
    }
    if (c->cfg.samples == 4) return render_msaa(c, n_frames, fd, io, s);
    if (c->cfg.mode == MDVT_MODE_POINTS && (rc = assign_div_slots(c, fd, s)) != MDVT_OK) return rc;

    const FrameDev* dfp = nullptr;
    ParamSlot* slot = nullptr;
    if ((rc = stage_params(c, fd, s, &dfp, &slot)) != MDVT_OK) return rc;

    RenderPlan plan{};
    plan.mode = c->cfg.mode;
    plan.remove_edges = c->cfg.remove_edges;
    plan.edge_points = c->cfg.remove_edges && c->cfg.edge_points;
    plan.general = any_general_frame;
    plan.allow_conv = c->opt_mesh_conv ? 1 : 0;
    if (tuning_build()) { const char* e = tuning_env(TUNE_MESH_CONV); plan.allow_conv = (e && e[0] == '1') ? 1 : 0; }   // (tests toggle it per call)
    plan.vec4 = (c->W % 4 == 0) && aligned(io->depth_rgb, 4) && aligned(io->color_rgb, 4) && aligned(io->left_rgb, 4) &&
                aligned(io->right_rgb, 4) && aligned(io->left_mask, 4) && aligned(io->right_mask, 4) &&
                io->depth_pitch % 4 == 0 && io->color_pitch % 4 == 0 && io->rgb_pitch % 4 == 0 && io->mask_pitch % 4 == 0 &&
                io->depth_stride % 4 == 0 && io->color_stride % 4 == 0 && io->rgb_stride % 4 == 0 && io->mask_stride % 4 == 0 &&
                (!io->left_seed || (aligned(io->left_seed, 4) && aligned(io->right_seed, 4) && io->seed_pitch % 4 == 0 && io->seed_stride % 4 == 0)) &&
                (!bf.zout || ((!io->left_depth || aligned(io->left_depth, 16)) && (!io->right_depth || aligned(io->right_depth, 16)) &&
                              io->zout_pitch % 16 == 0 && io->zout_stride % 16 == 0));

    std::vector<Run> runs;
    build_runs(c, plan, fd, runs);
    bool any_global = false, uses_global_ws = false;          // some run takes the global-key kernels / uses the global workspace
    for (const Run& r : runs) { any_global |= r.general != 0; uses_global_ws |= r.general || r.conv; }
    int tuned_chunk = 0;
    if (const char* e = tuning_env(TUNE_WS_CHUNK)) { const int v = atoi(e); if (v > 0) tuned_chunk = v; }   // tuning hook
    int ws_frames = 0, count_frames = 0;
    for (const Run& r : runs) {
        const int ch = chunk_of(c, plan, r, tuned_chunk);
        if ((r.general || r.conv || plan.remove_edges) && ch > ws_frames) ws_frames = ch;
        if (ch > count_frames) count_frames = ch;
    }
    if (ws_frames && (rc = ensure_workspace(c, ws_frames, any_global, uses_global_ws && plan.edge_points, plan.remove_edges,
                                            any_global && plan.mode == MDVT_MODE_MESH, s)) != MDVT_OK) return rc;
    RenderArgs base{};
    bind_io(base, c, io, dfp);
    base.zout[0] = io->left_depth; base.zout[1] = io->right_depth; base.zout_pitch = io->zout_pitch; base.zout_stride = io->zout_stride;
    base.maskbits[0] = io->left_maskbits; base.maskbits[1] = io->right_maskbits;
    base.maskbits_pitch = io->maskbits_pitch; base.maskbits_stride = io->maskbits_stride;
    base.seed[0] = io->left_seed; base.seed[1] = io->right_seed; base.seed_pitch = io->seed_pitch; base.seed_stride = io->seed_stride;
    if (io->hole_counts) {
        if ((rc = ensure_count_buffers(c, count_frames, s)) != MDVT_OK) return rc;
        base.row_counts = c->row_counts; base.wave_counts = c->wave_counts;
    }
    base.divcheck = c->divcheck; base.edge_paint = c->cfg.edge_points != 2; base.cull = c->cfg.cull;
    if (c->cfg.mode == MDVT_MODE_MESH) { if ((rc = ensure_rowcell(c, s)) != MDVT_OK) return rc; base.rowcell = c->rowcell; }
    const RenderWorkspaceLayout L = layout_of(c);
    if (uses_global_ws && c->keys_dirty && (rc = reset_dirty_keys(c, L, s)) != MDVT_OK) return rc;
    if (uses_global_ws) c->keys_dirty = true;
    for (const Run& r : runs)
        if ((rc = submit_run(c, plan, r, chunk_of(c, plan, r, tuned_chunk), base, L, fd, bf, s)) != MDVT_OK) return rc;
    if (uses_global_ws) c->keys_dirty = false;
    if (bf.near_clip && (rc = render_near_clip_gate(c, n_frames, dfp, io, s)) != MDVT_OK) return rc;
    MDVT_HIP(c, hipEventRecord(slot->done, s));
    return MDVT_OK;
}

int mdvt_render_stereo(mdvt_ctx* c, const mdvt_frame_params* params, const mdvt_io* io, void* stream)
{
    return mdvt_render_stereo_batch(c, 1, params, io, stream);
}

int mdvt_decode_depth(mdvt_ctx* c, const uint8_t* d_rgb, size_t rgb_pitch, float* d_depth, size_t depth_pitch,
                      double max_depth, double depth_scale, void* stream)
{
    if (!c) return MDVT_ERR_INVALID_ARG;
    if (!d_rgb || !d_depth) return fail(c, MDVT_ERR_INVALID_ARG, "NULL buffer");
    if (rgb_pitch < (size_t)3 * c->W || depth_pitch < (size_t)4 * c->W) return fail(c, MDVT_ERR_INVALID_ARG, "pitch smaller than one row");
    if (!(max_depth > 0.0)) return fail(c, MDVT_ERR_INVALID_ARG, "max_depth must be > 0");
    DeviceGuard g(c->device);
    MDVT_HIP(c, launch_decode_depth(d_rgb, rgb_pitch, d_depth, depth_pitch, c->W, c->H,
                                    (float)(max_depth / 4228250625.0), (float)depth_scale, (hipStream_t)stream));
    return MDVT_OK;
}

int mdvt_encode_depth(mdvt_ctx* c, const float* d_depth, size_t depth_pitch, uint8_t* d_rgb, size_t rgb_pitch,
                      double max_depth, int bgr, void* stream)
{
    if (!c) return MDVT_ERR_INVALID_ARG;
    if (!d_rgb || !d_depth) return fail(c, MDVT_ERR_INVALID_ARG, "NULL buffer");
    if (rgb_pitch < (size_t)3 * c->W || depth_pitch < (size_t)4 * c->W) return fail(c, MDVT_ERR_INVALID_ARG, "pitch smaller than one row");
    if (!(max_depth > 0.0)) return fail(c, MDVT_ERR_INVALID_ARG, "max_depth must be > 0");
    DeviceGuard g(c->device);
    MDVT_HIP(c, launch_encode_depth(d_depth, depth_pitch, d_rgb, rgb_pitch, c->W, c->H, max_depth, bgr, (hipStream_t)stream));
    return MDVT_OK;
}

int mdvt_release_cached_memory(int device)
{
    drain_dev_pool([&](const DevBlock& b) { return device < 0 || b.tag == device; });
    return MDVT_OK;
}

int mdvt_set_cached_memory_limit(uint64_t bytes_per_gpu)
{
    const size_t cap = (size_t)bytes_per_gpu;
    drain_dev_pool([](const DevBlock& b) { return dev_pool_idle()[b.tag] > g_dev_pool_idle_cap; }, &cap);      // per GPU, while its idle bytes pass the limit
    return MDVT_OK;
}

int mdvt_cached_memory(int device, uint64_t* idle_bytes, uint64_t* idle_blocks)
{
    uint64_t bytes = 0, blocks = 0;
    {
        std::lock_guard<std::mutex> lock(g_dev_pool_mutex);
        for (const DevBlock& b : dev_pool()) if (device < 0 || b.tag == device) { bytes += b.bytes; ++blocks; }
    }
    if (idle_bytes) *idle_bytes = bytes;
    if (idle_blocks) *idle_blocks = blocks;
    return MDVT_OK;
}

int mdvt_debug_read(mdvt_ctx* c, int what, void* h_dst, uint64_t capacity, uint64_t info[8])
{
    if (!c) return MDVT_ERR_INVALID_ARG;
    if (!tuning_build()) return fail(c, MDVT_ERR_UNSUPPORTED, "mdvt_debug_read: tuning build only");
    if (what < 0 || what > 2 || !info) return fail(c, MDVT_ERR_INVALID_ARG, "mdvt_debug_read: what must be 0, 1 or 2, info not NULL");
    if (what == 2) {
        // the two process-wide pools as this context's GPU sees them (its pool tag: the device, or MDVT_POOL_TAG): idle parameter
        // blocks that carry device memory of this / of another GPU, idle workspace blocks of this / of another GPU
        for (int k = 0; k < 8; ++k) info[k] = 0;
        {
            std::lock_guard<std::mutex> lock(g_pool_mutex);
            for (const PoolBlock& b : param_pool()) if (b.device >= 0) ++info[b.device == c->pool_tag ? 0 : 1];
        }
        {
            std::lock_guard<std::mutex> lock(g_dev_pool_mutex);
            for (const DevBlock& b : dev_pool()) ++info[b.tag == c->pool_tag ? 2 : 3];
        }
        info[4] = (uint64_t)c->pool_tag;
        return MDVT_OK;
    }
    DeviceGuard g(c->device);
    MDVT_HIP(c, hipDeviceSynchronize());
    if (what == 1) {
        // the coherence test of mdvt_selftest.hip on the queue block itself (it OVERWRITES the block: the next render rewrites what it
        // reads): h_dst receives 80 dwords; info[0] = the tag used
        if (!c->bigq || !h_dst || capacity < 80 * sizeof(uint32_t)) return fail(c, MDVT_ERR_INVALID_ARG, "mdvt_debug_read: no queue block / 320 bytes needed");
        static uint32_t tag = 0x1234567u;
        tag = tag * 1664525u + 1013904223u;
        uint32_t *d_xcc = nullptr, *d_out = nullptr;
        MDVT_HIP(c, hipMalloc((void**)&d_xcc, (c->bigq_bytes / 256 + 1) * sizeof(uint32_t)));
        MDVT_HIP(c, hipMalloc((void**)&d_out, 80 * sizeof(uint32_t)));
        hipError_t e = launch_coherence_test(c->bigq, c->bigq_bytes / 4, tag, d_xcc, d_out, nullptr);
        if (e == hipSuccess) e = hipMemcpy(h_dst, d_out, 80 * sizeof(uint32_t), hipMemcpyDeviceToHost);
        (void)hipFree(d_xcc); (void)hipFree(d_out);
        if (e != hipSuccess) return fail(c, MDVT_ERR_HIP, "mdvt_debug_read: %s", hipGetErrorString(e));
        info[0] = tag;
        return MDVT_OK;
    }
    const RenderWorkspaceLayout L = layout_of(c);
    info[0] = c->bigq ? c->bigq_bytes : 0;                                   // bytes of the queue block
    info[1] = c->bigq_counters_at;                                           // dword offset of the segment counters (as the block was made)
    info[2] = L.slots * L.H;                                                 // segments the block has room for
    info[3] = info[1] + L.counter_words();                                   // dword offset of the (first) huge list
    info[4] = info[3] + L.huge_lists * L.huge_list_dwords();                 // dword offset of the tie flags
    info[5] = (uint64_t)c->W; info[6] = (uint64_t)c->H; info[7] = (uint64_t)c->ws_frames;
    if (h_dst && c->bigq) {
        if (capacity < c->bigq_bytes) return fail(c, MDVT_ERR_INVALID_ARG, "mdvt_debug_read: %zu bytes needed", c->bigq_bytes);
        MDVT_HIP(c, hipMemcpy(h_dst, c->bigq, c->bigq_bytes, hipMemcpyDeviceToHost));
    }
    return MDVT_OK;
}

int mdvt_workspace_bytes(mdvt_ctx* c, uint64_t* bytes)
{
    if (!c) return MDVT_ERR_INVALID_ARG;
    if (!bytes) return fail(c, MDVT_ERR_INVALID_ARG, "NULL argument");
    *bytes = (uint64_t)c->ws_bytes;
    return MDVT_OK;
}

int mdvt_edge_point_pixels(mdvt_ctx* c, const mdvt_frame_params* params, const uint8_t* d_depth_rgb, size_t depth_pitch,
                           int how, int32_t* d_px, void* stream)
{
    if (!c) return MDVT_ERR_INVALID_ARG;
    if (!c->cfg_set) return fail(c, MDVT_ERR_INVALID_ARG, "mdvt_set_config has not been called");
    if (!params || !d_depth_rgb || !d_px) return fail(c, MDVT_ERR_INVALID_ARG, "NULL argument");
    if (depth_pitch < (size_t)3 * c->W) return fail(c, MDVT_ERR_INVALID_ARG, "pitch smaller than one row");
    if (how != 0 && how != 1) return fail(c, MDVT_ERR_INVALID_ARG, "how must be 0 (the chain) or 1 (as the row kernels take it)");
    DeviceGuard g(c->device);
    hipStream_t s = (hipStream_t)stream;
    std::vector<FrameDev> fd(1);
    // (the row range is only worked out for configurations that splat edge points; this entry point always wants it)
    mdvt_config saved = c->cfg;
    c->cfg.remove_edges = 1; c->cfg.edge_points = 1;
    const int rc0 = fill_frame_dev(c, *params, fd[0]);
    c->cfg = saved;
    if (rc0 != MDVT_OK) return rc0;
    if (how == 1 && (fd[0].general || fd[0].erow_wild))
        return fail(c, MDVT_ERR_INVALID_ARG, "how = 1 needs a pure-shift frame whose rows the row kernels take");
    const FrameDev* dfp = nullptr;
    ParamSlot* slot = nullptr;
    const int rc = stage_params(c, fd, s, &dfp, &slot);
    if (rc != MDVT_OK) return rc;
    MDVT_HIP(c, launch_edge_point_pixels(d_depth_rgb, depth_pitch, dfp, c->W, c->H, c->cfg.mode == MDVT_MODE_MESH ? 1 : 0, how, d_px, s));
    MDVT_HIP(c, hipEventRecord(slot->done, s));
    return MDVT_OK;
}

int mdvt_edge_filter(mdvt_ctx* c, const uint8_t* d_depth_rgb, size_t depth_pitch, const double K[9], double depth_scale,
                     int of_by_one, uint8_t* d_tri_invalid, uint8_t* d_unused, void* stream)
{
    if (!c) return MDVT_ERR_INVALID_ARG;
    if (!d_depth_rgb || !K) return fail(c, MDVT_ERR_INVALID_ARG, "NULL buffer");
    if (depth_pitch < (size_t)3 * c->W) return fail(c, MDVT_ERR_INVALID_ARG, "pitch smaller than one row");
    if (c->W < 2 || c->H < 2) return fail(c, MDVT_ERR_INVALID_ARG, "the edge filter needs at least a 2x2 frame");
    DeviceGuard g(c->device);
    hipStream_t s = (hipStream_t)stream;
    std::vector<FrameDev> fd(1);
    FrameDev& f = fd[0];
    memset(&f, 0, sizeof f);
    f.mult = (float)(c->cfg.max_depth / 4228250625.0);
    f.scale = (float)depth_scale;
    f.Kd[0] = K[0]; f.Kd[1] = K[4]; f.Kd[2] = K[2]; f.Kd[3] = K[5];
    f.rKd[0] = 1.0 / K[0]; f.rKd[1] = 1.0 / K[4];
    const FrameDev* dfp = nullptr;
    ParamSlot* slot = nullptr;
    int rc = stage_params(c, fd, s, &dfp, &slot);
    if (rc != MDVT_OK) return rc;
    if (d_unused) MDVT_HIP(c, hipMemsetAsync(d_unused, 0, (size_t)c->W * c->H, s));
    MDVT_HIP(c, launch_edge_filter(d_depth_rgb, depth_pitch, 0, dfp, 0, 1, c->W, c->H, of_by_one ? 1 : 0,
                                   d_tri_invalid, 0, d_unused, 0, s));
    MDVT_HIP(c, hipEventRecord(slot->done, s));
    return MDVT_OK;
}

static int ensure_ni_workspace(mdvt_ctx* c, int chunk, hipStream_t s);      // (the listed-pixel stages' workspace, below)

int mdvt_infill_using_normals(mdvt_ctx* c, const uint8_t* d_color, size_t color_pitch, const uint8_t* d_hole,
                              size_t hole_pitch, const float* d_normal, size_t normal_pitch, uint8_t* d_out,
                              size_t out_pitch, int max_steps, void* stream)
{
    if (!c) return MDVT_ERR_INVALID_ARG;
    if (!d_color || !d_hole || !d_normal || !d_out) return fail(c, MDVT_ERR_INVALID_ARG, "NULL buffer");
    if (d_out == d_color) return fail(c, MDVT_ERR_INVALID_ARG, "d_out may not alias d_color (sources are read from the input image)");
    if (color_pitch < (size_t)3 * c->W || out_pitch < (size_t)3 * c->W || hole_pitch < (size_t)c->W ||
        normal_pitch < (size_t)12 * c->W || normal_pitch % 4 != 0)
        return fail(c, MDVT_ERR_INVALID_ARG, "pitch smaller than one row");
    if (max_steps < 0) return fail(c, MDVT_ERR_INVALID_ARG, "max_steps must be >= 0");
    if (hole_pitch >= (1u << 24) || (unsigned long long)hole_pitch * c->H > 0xFFFFFFFFull)
        return fail(c, MDVT_ERR_UNSUPPORTED, "hole plane too large for the march's 32-bit offsets (pitch %zu, %d rows)", hole_pitch, c->H);
    DeviceGuard g(c->device);
    if (int rc = ensure_ni_workspace(c, 1, (hipStream_t)stream)) return rc;
    MDVT_HIP(c, launch_infill_normals(d_color, color_pitch, d_hole, hole_pitch, d_normal, normal_pitch, d_out, out_pitch,
                                      c->W, c->H, max_steps, c->ni_ws, (hipStream_t)stream));
    return MDVT_OK;
}

int mdvt_mark_lower_side(mdvt_ctx* c, const uint8_t* d_normals_img, size_t img_pitch, uint8_t* d_out, size_t out_pitch,
                         int max_steps, void* stream)
{
    if (!c) return MDVT_ERR_INVALID_ARG;
    if (!d_normals_img || !d_out) return fail(c, MDVT_ERR_INVALID_ARG, "NULL buffer");
    if (d_out == d_normals_img) return fail(c, MDVT_ERR_INVALID_ARG, "d_out may not alias the input image");
    if (img_pitch < (size_t)3 * c->W || out_pitch < (size_t)3 * c->W) return fail(c, MDVT_ERR_INVALID_ARG, "pitch smaller than one row");
    if (max_steps < 0) return fail(c, MDVT_ERR_INVALID_ARG, "max_steps must be >= 0");
    if (img_pitch >= (1u << 24) || (unsigned long long)img_pitch * c->H > 0xFFFFFFFFull)
        return fail(c, MDVT_ERR_UNSUPPORTED, "image too large for the march's 32-bit offsets (pitch %zu, %d rows)", img_pitch, c->H);
    DeviceGuard g(c->device);
    if (int rc = ensure_ni_workspace(c, 1, (hipStream_t)stream)) return rc;
    MDVT_HIP(c, launch_mark_lower_side(d_normals_img, img_pitch, d_out, out_pitch, c->W, c->H, max_steps, c->ni_ws, (hipStream_t)stream));
    return MDVT_OK;
}

int mdvt_touchly_depth(mdvt_ctx* c, const float* d_depth, size_t depth_pitch, uint8_t* d_rgb, size_t rgb_pitch,
                       double touchly_max_depth, double touchly_min_depth, int zero_is_far, void* stream)
{
    if (!c) return MDVT_ERR_INVALID_ARG;
    if (!d_depth || !d_rgb) return fail(c, MDVT_ERR_INVALID_ARG, "NULL buffer");
    if (depth_pitch < (size_t)4 * c->W || rgb_pitch < (size_t)3 * c->W) return fail(c, MDVT_ERR_INVALID_ARG, "pitch smaller than one row");
    if (!(touchly_max_depth > touchly_min_depth)) return fail(c, MDVT_ERR_INVALID_ARG, "touchly_max_depth must exceed touchly_min_depth");
    DeviceGuard g(c->device);
    // NumPy: f32 array (op) python float -> the scalar is rounded to f32 first
    MDVT_HIP(c, launch_touchly_depth(d_depth, depth_pitch, d_rgb, rgb_pitch, c->W, c->H, (float)touchly_max_depth,
                                     (float)touchly_min_depth, (float)(255.0 / (touchly_max_depth - touchly_min_depth)),
                                     zero_is_far, (hipStream_t)stream));
    return MDVT_OK;
}

int mdvt_equirect_tables(int width, int height, double input_fov_deg, float* h_map_x, float* h_map_y)
{
    if (width < 2 || height < 2 || !h_map_x || !h_map_y) return MDVT_ERR_INVALID_ARG;
    if (!(input_fov_deg > 0.0 && input_fov_deg < 180.0)) return MDVT_ERR_INVALID_ARG;
    // f64 throughout, rounded to f32 at the end like map_x.astype(np.float32) (sr:77-78)
    const double pi = 3.141592653589793;
    const double cx = ((double)width - 1.0) / 2.0, cy = ((double)height - 1.0) / 2.0;
    const double half = (input_fov_deg / 2.0) * (pi / 180.0);
    const double fx = cx / tan(half), fy = cy / tan(half);
    for (int x = 0; x < width; ++x) {
        const double theta = ((double)x - cx) / cx * (pi / 2.0);
        h_map_x[x] = fabs(theta) <= half ? (float)(fx * tan(theta) + cx) : -1.0f;
    }
    for (int y = 0; y < height; ++y) {
        const double phi = ((double)y - cy) / cy * (pi / 2.0);
        h_map_y[y] = fabs(phi) <= half ? (float)(fy * tan(phi) + cy) : -1.0f;
    }
    return MDVT_OK;
}

int mdvt_equirect_remap(mdvt_ctx* c, const uint8_t* d_src, size_t src_pitch, size_t src_stride, uint8_t* d_dst,
                        size_t dst_pitch, size_t dst_stride, int n_images, const float* d_map_x, const float* d_map_y,
                        void* stream)
{
    if (!c) return MDVT_ERR_INVALID_ARG;
    if (!d_src || !d_dst || !d_map_x || !d_map_y) return fail(c, MDVT_ERR_INVALID_ARG, "NULL buffer");
    if (n_images < 1) return fail(c, MDVT_ERR_INVALID_ARG, "n_images must be >= 1");
    if (src_pitch < (size_t)3 * c->W || dst_pitch < (size_t)3 * c->W) return fail(c, MDVT_ERR_INVALID_ARG, "pitch smaller than one row");
    if (d_src == d_dst) return fail(c, MDVT_ERR_INVALID_ARG, "d_dst may not alias d_src");
    DeviceGuard g(c->device);
    MDVT_HIP(c, launch_equirect_remap(d_src, src_pitch, src_stride, d_dst, dst_pitch, dst_stride, n_images, c->W, c->H,
                                      d_map_x, d_map_y, (hipStream_t)stream));
    return MDVT_OK;
}

namespace {
// cv2.getGaussianKernel(6, 0) as published: sigma = 0.3*((n-1)*0.5 - 1) + 0.8, exp in f64, scaled by 1/sum; the
// 2-D kernel is the f64 outer product (sr:124-125) rounded to f32 (what filter2D does for an f32 image).
mdvt::BlurKernel masked_blur_kernel()
{
    double g[6], sum = 0.0;
    const double sigma = 0.3 * ((6 - 1) * 0.5 - 1.0) + 0.8, scale2 = -0.5 / (sigma * sigma);
    for (int i = 0; i < 6; ++i) { const double x = (double)i - (6 - 1) * 0.5; g[i] = exp(scale2 * x * x); sum += g[i]; }
    sum = 1.0 / sum;
    for (int i = 0; i < 6; ++i) g[i] *= sum;
    mdvt::BlurKernel K;
    for (int y = 0; y < 6; ++y) for (int x = 0; x < 6; ++x) K.k[6 * y + x] = (float)(g[y] * g[x]);
    return K;
}
constexpr int kTeleaChunk = mdvt::kTeleaMaxImages;      // images per pass (14 B/px of workspace each)

}  // namespace

int mdvt_swap_rb(mdvt_ctx* c, const uint8_t* d_src, size_t src_pitch, size_t src_stride, uint8_t* d_dst, size_t dst_pitch,
                 size_t dst_stride, int n_images, void* stream)
{
    if (!c) return MDVT_ERR_INVALID_ARG;
    if (!d_src || !d_dst) return fail(c, MDVT_ERR_INVALID_ARG, "NULL buffer");
    if (n_images < 1) return fail(c, MDVT_ERR_INVALID_ARG, "n_images must be >= 1");
    if (src_pitch < (size_t)3 * c->W || dst_pitch < (size_t)3 * c->W) return fail(c, MDVT_ERR_INVALID_ARG, "pitch smaller than one row");
    DeviceGuard g(c->device);
    const mdvt::ImageSet in{const_cast<uint8_t*>(d_src), src_pitch, src_stride, 0, n_images}, out{d_dst, dst_pitch, dst_stride, 0, n_images};
    MDVT_HIP(c, launch_swap_rb(in, out, n_images, c->W, c->H, (hipStream_t)stream));
    return MDVT_OK;
}

int mdvt_masked_blur(mdvt_ctx* c, const uint8_t* d_img, size_t img_pitch, uint8_t* d_out, size_t out_pitch, void* stream)
{
    if (!c) return MDVT_ERR_INVALID_ARG;
    if (!d_img || !d_out) return fail(c, MDVT_ERR_INVALID_ARG, "NULL buffer");
    if (img_pitch < (size_t)3 * c->W || out_pitch < (size_t)3 * c->W) return fail(c, MDVT_ERR_INVALID_ARG, "pitch smaller than one row");
    if (d_img == d_out) return fail(c, MDVT_ERR_INVALID_ARG, "d_out may not alias d_img");
    DeviceGuard g(c->device);
    const mdvt::ImageSet in{const_cast<uint8_t*>(d_img), img_pitch, 0, 0, 1}, out{d_out, out_pitch, 0, 0, 1};
    MDVT_HIP(c, launch_masked_blur(in, nullptr, out, 1, c->W, c->H, masked_blur_kernel(), 0u, (hipStream_t)stream));
    return MDVT_OK;
}

constexpr int kNormalInfillChunk = 16;       // images per launch set

static int ensure_ni_workspace(mdvt_ctx* c, int chunk, hipStream_t s)
{
    if (c->ni_images >= chunk) return MDVT_OK;
    MDVT_HIP(c, hipDeviceSynchronize());                 // earlier submissions may still use the old workspace
    if (c->ni_ws) ws_free(c, c->ni_ws);
    c->ni_ws = nullptr; c->ni_images = 0;
    MDVT_HIP(c, ws_malloc(c, (void**)&c->ni_ws, mdvt::normal_infill_workspace_bytes(chunk, c->W, c->H), s));
    c->ni_images = chunk;
    return MDVT_OK;
}


int mdvt_normal_infill(mdvt_ctx* c, const uint8_t* d_img, size_t img_pitch, size_t img_stride, const uint8_t* d_infill_mask,
                       size_t mask_pitch, size_t mask_stride, uint8_t* d_out, size_t out_pitch, size_t out_stride, int n_images,
                       void* stream)
{
    if (!c) return MDVT_ERR_INVALID_ARG;
    if (!d_img || !d_infill_mask || !d_out) return fail(c, MDVT_ERR_INVALID_ARG, "NULL buffer");
    if (n_images < 1) return fail(c, MDVT_ERR_INVALID_ARG, "n_images must be >= 1");
    if (img_pitch < (size_t)3 * c->W || mask_pitch < (size_t)3 * c->W || out_pitch < (size_t)3 * c->W)
        return fail(c, MDVT_ERR_INVALID_ARG, "pitch smaller than one row");
    if (d_out == d_img || d_out == d_infill_mask) return fail(c, MDVT_ERR_INVALID_ARG, "d_out may not alias an input");
    if (mask_pitch >= (1u << 24) || (unsigned long long)mask_pitch * c->H > 0xFFFFFFFFull || (unsigned long long)c->W * c->H > 0xFFFFFFFFull)
        return fail(c, MDVT_ERR_UNSUPPORTED, "image too large for the marches' 32-bit offsets (pitch %zu, %d x %d)", mask_pitch, c->W, c->H);
    DeviceGuard g(c->device);
    hipStream_t s = (hipStream_t)stream;
    const int chunk = n_images < kNormalInfillChunk ? n_images : kNormalInfillChunk;
    if (int rc = ensure_ni_workspace(c, chunk, s)) return rc;
    const mdvt::BlurKernel K = masked_blur_kernel();
    for (int i0 = 0; i0 < n_images; i0 += chunk) {
        const int n = n_images - i0 < chunk ? n_images - i0 : chunk;
        const mdvt::ImageSet img{const_cast<uint8_t*>(d_img) + (size_t)i0 * img_stride, img_pitch, img_stride, 0, n};
        const mdvt::ImageSet mask{const_cast<uint8_t*>(d_infill_mask) + (size_t)i0 * mask_stride, mask_pitch, mask_stride, 0, n};
        const mdvt::ImageSet out{d_out + (size_t)i0 * out_stride, out_pitch, out_stride, 0, n};
        MDVT_HIP(c, launch_normal_infill(img, mask, out, c->ni_ws, n, c->W, c->H, K, s));
    }
    return MDVT_OK;
}

int mdvt_infill_using_mask_normals(mdvt_ctx* c, uint8_t* d_img, size_t img_pitch, size_t img_stride, const uint8_t* d_hole,
                                   size_t hole_pitch, size_t hole_stride, const uint8_t* d_mask_img, size_t mask_pitch,
                                   size_t mask_stride, int n_images, int max_steps, void* stream)
{
    if (!c) return MDVT_ERR_INVALID_ARG;
    if (!d_img || !d_hole || !d_mask_img) return fail(c, MDVT_ERR_INVALID_ARG, "NULL buffer");
    if (n_images < 1) return fail(c, MDVT_ERR_INVALID_ARG, "n_images must be >= 1");
    if (img_pitch < (size_t)3 * c->W || mask_pitch < (size_t)3 * c->W || hole_pitch < (size_t)c->W)
        return fail(c, MDVT_ERR_INVALID_ARG, "pitch smaller than one row");
    if (max_steps < 0) return fail(c, MDVT_ERR_INVALID_ARG, "max_steps must be >= 0");
    if (d_img == d_mask_img) return fail(c, MDVT_ERR_INVALID_ARG, "d_img may not alias d_mask_img");
    if (hole_pitch >= (1u << 24) || (unsigned long long)hole_pitch * c->H > 0xFFFFFFFFull)
        return fail(c, MDVT_ERR_UNSUPPORTED, "hole plane too large for the march's 32-bit offsets (pitch %zu, %d rows)", hole_pitch, c->H);
    DeviceGuard g(c->device);
    const int chunk = n_images < kNormalInfillChunk ? n_images : kNormalInfillChunk;
    if (int rc = ensure_ni_workspace(c, chunk, (hipStream_t)stream)) return rc;
    for (int i0 = 0; i0 < n_images; i0 += chunk) {
        const int n = n_images - i0 < chunk ? n_images - i0 : chunk;
        const mdvt::ImageSet img{d_img + (size_t)i0 * img_stride, img_pitch, img_stride, 0, n};
        const mdvt::ImageSet hole{const_cast<uint8_t*>(d_hole) + (size_t)i0 * hole_stride, hole_pitch, hole_stride, 0, n};
        const mdvt::ImageSet mask{const_cast<uint8_t*>(d_mask_img) + (size_t)i0 * mask_stride, mask_pitch, mask_stride, 0, n};
        MDVT_HIP(c, launch_infill_mask_normals(img, hole, mask, c->ni_ws, n, c->W, c->H, max_steps, (hipStream_t)stream));
    }
    return MDVT_OK;
}

static int finish_infill_mask(mdvt_ctx* c, const uint8_t* d_seed, const uint8_t* d_seed_right, size_t seed_pitch, size_t seed_stride,
                              uint8_t* d_out, uint8_t* d_out_right, size_t out_pitch, size_t out_stride, int n_frames, int max_rounds,
                              uint32_t* d_remaining, void* stream)
{
    if (!c) return MDVT_ERR_INVALID_ARG;
    if (!d_seed || !d_out) return fail(c, MDVT_ERR_INVALID_ARG, "NULL buffer");
    if ((d_seed_right == nullptr) != (d_out_right == nullptr)) return fail(c, MDVT_ERR_INVALID_ARG, "right-eye seed and output go together");
    if (n_frames < 1) return fail(c, MDVT_ERR_INVALID_ARG, "n_images must be >= 1");
    if (seed_pitch < (size_t)3 * c->W || out_pitch < (size_t)3 * c->W) return fail(c, MDVT_ERR_INVALID_ARG, "pitch smaller than one row");
    if (d_seed == d_out || (d_seed_right && d_seed_right == d_out_right)) return fail(c, MDVT_ERR_INVALID_ARG, "d_out may not alias d_seed");
    // max_rounds < 0: |max_rounds| levels, every one of them launched without asking the device how many exist (no wait on the stream)
    const bool no_wait = max_rounds < 0;
    if (no_wait) max_rounds = -max_rounds;
    if (max_rounds == 0) max_rounds = 256;
    if (max_rounds > 32766) return fail(c, MDVT_ERR_INVALID_ARG, "max_rounds must be <= 32766");
    DeviceGuard g(c->device);
    hipStream_t s = (hipStream_t)stream;
    const int W = c->W, H = c->H;
    const size_t npx = (size_t)W * H;
    if ((unsigned long long)kTeleaChunk * npx > 0xFFFFFFFFull)      // work-list entries are 32-bit pixel indices over a full pass
        return fail(c, MDVT_ERR_UNSUPPORTED, "frame too large for the infill-mask completion (%d x %d)", W, H);
    const int eyes_ = d_seed_right ? 2 : 1;
    const int want_images = n_frames * eyes_ < kTeleaChunk ? n_frames * eyes_ : kTeleaChunk;
    if (c->telea_images < want_images || c->telea_rounds < max_rounds) {
        MDVT_HIP(c, hipDeviceSynchronize());                 // earlier submissions may still use the old workspace
        const int images = want_images > c->telea_images ? want_images : c->telea_images;   // per-pixel arrays; the counters hold a full pass
        const int rounds = max_rounds > c->telea_rounds ? max_rounds : c->telea_rounds;
        free_telea(c);
        mdvt::TeleaWorkspace& w = c->telea;
        MDVT_HIP(c, ws_malloc(c, (void**)&w.stamp, (size_t)images * npx * sizeof(uint16_t), s));
        MDVT_HIP(c, ws_malloc(c, (void**)&w.T, (size_t)images * npx * sizeof(float), s));
        MDVT_HIP(c, ws_malloc(c, (void**)&w.img, (size_t)images * npx * 3 + 4, s));      // + 4: pixels are fetched as unaligned dwords
        MDVT_HIP(c, ws_malloc(c, (void**)&w.need, (size_t)images * npx, s));
        MDVT_HIP(c, ws_malloc(c, (void**)&w.nlist, (size_t)images * npx * sizeof(uint32_t), s));
        MDVT_HIP(c, ws_malloc(c, (void**)&w.counts, mdvt::telea_counter_words(rounds) * sizeof(uint32_t), s));
        MDVT_HIP(c, ws_malloc(c, (void**)&w.remaining, (size_t)kTeleaChunk * sizeof(uint32_t), s));
        MDVT_HIP(c, ws_malloc(c, (void**)&w.last_round, (size_t)kTeleaChunk * sizeof(uint32_t), s));
        c->telea_images = images; c->telea_rounds = rounds;
    }
    c->telea.offs = c->telea.counts + (max_rounds + 2);
    c->telea.ncounts = c->telea.offs + (max_rounds + 2);
    if (!c->telea_levels_host) {
        void *h = nullptr, *d = nullptr;
        size_t got = 0;
        MDVT_HIP(c, pool_take(64, false, -1, &h, &d, &got));          // pinned, from the process-wide pool (see pool_take)
        c->telea_levels_host = (uint32_t*)h;
    }
    const uint32_t key = packed_key_rgb(c);
    const mdvt::BlurKernel K = masked_blur_kernel();
    const int eyes = d_seed_right ? 2 : 1;
    const int fchunk = kTeleaChunk / eyes;                   // frames per pass: both eyes of a frame travel together
    for (int f0 = 0; f0 < n_frames; f0 += fchunk) {
        const int nf = n_frames - f0 < fchunk ? n_frames - f0 : fchunk, n = nf * eyes;
        const mdvt::ImageSet seed{const_cast<uint8_t*>(d_seed) + (size_t)f0 * seed_stride, seed_pitch, seed_stride,
                                  d_seed_right ? d_seed_right - d_seed : 0, nf};
        const mdvt::ImageSet out{d_out + (size_t)f0 * out_stride, out_pitch, out_stride, d_out_right ? d_out_right - d_out : 0, nf};
        const mdvt::ImageSet work{c->telea.img, (size_t)3 * W, 3 * npx, 0, n};
        MDVT_HIP(c, launch_telea_init(seed, c->telea, n, W, H, max_rounds, key, no_wait ? nullptr : c->telea_levels_host, s));
        MDVT_HIP(c, launch_telea_rounds(c->telea, W, H, no_wait ? max_rounds : (int)*c->telea_levels_host, key, s));               // sr:806, inpaintRadius = 3
        // (the level lists and T are done with: their storage serves the blur's per-row pixel lists and row counters)
        MDVT_HIP(c, launch_masked_blur(work, &seed, out, n, W, H, K, key, s, c->telea.nlist, reinterpret_cast<uint32_t*>(c->telea.T)));   // sr:807-808
        if (d_remaining) {      // image order of the result: left eyes of all frames, then right eyes
            for (int e = 0; e < eyes; ++e)
                MDVT_HIP(c, hipMemcpyAsync(d_remaining + (size_t)e * n_frames + f0, c->telea.remaining + (size_t)e * nf,
                                           (size_t)nf * sizeof(uint32_t), hipMemcpyDeviceToDevice, s));
        }
    }
    return MDVT_OK;
}

// The same completion in the heap order of cv2.inpaint (mdvt_telea_heap.hip): one launch per pass, no host read-back.  Images per
// pass: below.
static int finish_infill_mask_heap(mdvt_ctx* c, const uint8_t* d_seed, const uint8_t* d_seed_right, size_t seed_pitch, size_t seed_stride,
                                   uint8_t* d_out, uint8_t* d_out_right, size_t out_pitch, size_t out_stride, int n_frames,
                                   uint32_t* d_remaining, void* stream)
{
    if (!c) return MDVT_ERR_INVALID_ARG;
    if (!d_seed || !d_out) return fail(c, MDVT_ERR_INVALID_ARG, "NULL buffer");
    if ((d_seed_right == nullptr) != (d_out_right == nullptr)) return fail(c, MDVT_ERR_INVALID_ARG, "right-eye seed and output go together");
    if (n_frames < 1) return fail(c, MDVT_ERR_INVALID_ARG, "n_images must be >= 1");
    if (seed_pitch < (size_t)3 * c->W || out_pitch < (size_t)3 * c->W) return fail(c, MDVT_ERR_INVALID_ARG, "pitch smaller than one row");
    if (d_seed == d_out || (d_seed_right && d_seed_right == d_out_right)) return fail(c, MDVT_ERR_INVALID_ARG, "d_out may not alias d_seed");
    DeviceGuard g(c->device);
    hipStream_t s = (hipStream_t)stream;
    const int W = c->W, H = c->H;
    const size_t npx = (size_t)W * H;
    if (npx >= ((size_t)1 << 29))          // activation keys 4 rank + direction and push numbers (< 2 npx) are 32-bit
        return fail(c, MDVT_ERR_UNSUPPORTED, "frame too large for the heap-order completion (%d x %d)", W, H);
    const size_t per_image = mdvt::telea_heap_image_bytes(W, H);
    // images per pass: what fits a quarter of the device's memory and what is free now (the workspace this ctx already holds
    // counts as free: it is reused or handed back first), at most kTeleaHeapMaxImages; both eyes of a frame travel together
    size_t free_b = 0, total_b = 0;
    MDVT_HIP(c, hipMemGetInfo(&free_b, &total_b));
    const size_t held = (size_t)c->heap_images * per_image;
    size_t budget = total_b / 4;
    if (free_b + held < budget) budget = free_b + held;
    size_t cap = budget / per_image;
    if (cap < (size_t)c->heap_images) cap = (size_t)c->heap_images;
    if (cap > (size_t)mdvt::kTeleaHeapMaxImages) cap = mdvt::kTeleaHeapMaxImages;
    const int eyes = d_seed_right ? 2 : 1;
    int fchunk = cap / eyes >= 1 ? (int)(cap / eyes) : 1;                // frames per pass
    const int want_images = (n_frames < fchunk ? n_frames : fchunk) * eyes;
    if (c->heap_images < want_images) {
        MDVT_HIP(c, hipDeviceSynchronize());                 // earlier submissions may still use the old workspace
        free_telea_heap(c);
        // if the block does not fit after all (another process took the memory meanwhile), fewer images per pass
        int images = want_images;
        for (;;) {
            const hipError_t e = ws_malloc(c, (void**)&c->heap_ws, (size_t)images * per_image, s);
            if (e == hipSuccess) break;
            (void)hipGetLastError();
            if (images <= eyes)
                return fail(c, MDVT_ERR_OOM, "heap-order completion: no room for the workspace of one %s (%zu bytes): %s",
                            eyes == 2 ? "frame" : "image", (size_t)eyes * per_image, hipGetErrorString(e));
            images = images / 2 / eyes * eyes;
            if (images < eyes) images = eyes;
        }
        MDVT_HIP(c, ws_malloc(c, (void**)&c->heap_remaining, (size_t)images * sizeof(uint32_t), s));
        c->heap_images = images;
    }
    if (fchunk > c->heap_images / eyes) fchunk = c->heap_images / eyes;
    const uint32_t key = packed_key_rgb(c);
    const mdvt::BlurKernel K = masked_blur_kernel();
    for (int f0 = 0; f0 < n_frames; f0 += fchunk) {
        const int nf = n_frames - f0 < fchunk ? n_frames - f0 : fchunk, n = nf * eyes;
        const mdvt::ImageSet seed{const_cast<uint8_t*>(d_seed) + (size_t)f0 * seed_stride, seed_pitch, seed_stride,
                                  d_seed_right ? d_seed_right - d_seed : 0, nf};
        const mdvt::ImageSet out{d_out + (size_t)f0 * out_stride, out_pitch, out_stride, d_out_right ? d_out_right - d_out : 0, nf};
        const mdvt::ImageSet work{c->heap_ws + mdvt::telea_heap_img_offset(W, H), (size_t)3 * W, per_image, 0, n};
        MDVT_HIP(c, launch_telea_heap(seed, c->heap_ws, per_image, c->heap_remaining, n, W, H, key, s));     // sr:806, inpaintRadius = 3
        MDVT_HIP(c, launch_masked_blur(work, &seed, out, n, W, H, K, key, s));                                // sr:807-808
        if (d_remaining) {      // image order of the result: left eyes of all frames, then right eyes
            for (int e = 0; e < eyes; ++e)
                MDVT_HIP(c, hipMemcpyAsync(d_remaining + (size_t)e * n_frames + f0, c->heap_remaining + (size_t)e * nf,
                                           (size_t)nf * sizeof(uint32_t), hipMemcpyDeviceToDevice, s));
        }
    }
    return MDVT_OK;
}

int mdvt_finish_infill_mask_heap(mdvt_ctx* c, const uint8_t* d_seed, size_t seed_pitch, size_t seed_stride, uint8_t* d_out,
                                 size_t out_pitch, size_t out_stride, int n_images, uint32_t* d_remaining, void* stream)
{
    return finish_infill_mask_heap(c, d_seed, nullptr, seed_pitch, seed_stride, d_out, nullptr, out_pitch, out_stride, n_images,
                                   d_remaining, stream);
}

int mdvt_finish_infill_mask_heap_stereo(mdvt_ctx* c, const uint8_t* d_left_seed, const uint8_t* d_right_seed, size_t seed_pitch,
                                        size_t seed_stride, uint8_t* d_left_out, uint8_t* d_right_out, size_t out_pitch,
                                        size_t out_stride, int n_frames, uint32_t* d_remaining, void* stream)
{
    if (c && (!d_right_seed || !d_right_out)) return fail(c, MDVT_ERR_INVALID_ARG, "NULL buffer");
    return finish_infill_mask_heap(c, d_left_seed, d_right_seed, seed_pitch, seed_stride, d_left_out, d_right_out, out_pitch,
                                   out_stride, n_frames, d_remaining, stream);
}

int mdvt_finish_infill_mask(mdvt_ctx* c, const uint8_t* d_seed, size_t seed_pitch, size_t seed_stride, uint8_t* d_out,
                            size_t out_pitch, size_t out_stride, int n_images, int max_rounds, uint32_t* d_remaining, void* stream)
{
    return finish_infill_mask(c, d_seed, nullptr, seed_pitch, seed_stride, d_out, nullptr, out_pitch, out_stride, n_images, max_rounds,
                              d_remaining, stream);
}

int mdvt_finish_infill_mask_stereo(mdvt_ctx* c, const uint8_t* d_left_seed, const uint8_t* d_right_seed, size_t seed_pitch,
                                   size_t seed_stride, uint8_t* d_left_out, uint8_t* d_right_out, size_t out_pitch, size_t out_stride,
                                   int n_frames, int max_rounds, uint32_t* d_remaining, void* stream)
{
    if (c && (!d_right_seed || !d_right_out)) return fail(c, MDVT_ERR_INVALID_ARG, "NULL buffer");
    return finish_infill_mask(c, d_left_seed, d_right_seed, seed_pitch, seed_stride, d_left_out, d_right_out, out_pitch, out_stride,
                              n_frames, max_rounds, d_remaining, stream);
}

// FFV1 packets of device frames (mdvt_ffv1.hip).  Passes: as many frames as the ctx's workspace budget affords, at least one.
int mdvt_encode_video_frames(mdvt_ctx* c, int width, int height, int slices_h, int slices_v, const uint8_t* d_src, size_t pitch,
                            size_t frame_stride, int channels, int order, int n_frames, uint64_t slice_capacity, uint8_t* d_packets,
                            uint64_t packets_cap, uint64_t* d_offsets, uint32_t* d_sizes, void* stream)
{
    if (!c) return MDVT_ERR_INVALID_ARG;
    if (!d_src || !d_packets || !d_offsets || !d_sizes) return fail(c, MDVT_ERR_INVALID_ARG, "NULL buffer");
    if (width < 1 || height < 1) return fail(c, MDVT_ERR_INVALID_ARG, "bad frame size %d x %d", width, height);
    if (slices_h < 1 || slices_v < 1 || slices_h > width || slices_v > height || slices_h * slices_v > 1024)
        return fail(c, MDVT_ERR_INVALID_ARG, "bad slice counts %d x %d for %d x %d (each >= 1 and <= the frame's size, product <= 1024)",
                    slices_h, slices_v, width, height);
    if (channels != 1 && channels != 3) return fail(c, MDVT_ERR_INVALID_ARG, "channels must be 1 or 3, got %d", channels);
    if (order != 0 && order != 1) return fail(c, MDVT_ERR_INVALID_ARG, "order must be 0 (RGB) or 1 (BGR), got %d", order);
    if (n_frames < 1) return fail(c, MDVT_ERR_INVALID_ARG, "n_frames must be >= 1");
    if (pitch < (size_t)width * (size_t)channels) return fail(c, MDVT_ERR_INVALID_ARG, "pitch smaller than one row");
    if (n_frames > 1 && frame_stride < pitch * (size_t)height) return fail(c, MDVT_ERR_INVALID_ARG, "frame_stride smaller than one frame");
    if ((uint64_t)width * (uint64_t)height > ((uint64_t)1 << 28))      // (a slice's sample count is a 32-bit word)
        return fail(c, MDVT_ERR_UNSUPPORTED, "frame too large for the device FFV1 encoder (%d x %d)", width, height);
    DeviceGuard g(c->device);
    hipStream_t s = (hipStream_t)stream;
    const int spf = slices_h * slices_v;
    // the largest slice: widths and heights of the slices differ by at most one
    const uint64_t max_raw = (uint64_t)((width + slices_h - 1) / slices_h) * (uint64_t)((height + slices_v - 1) / slices_v) * 3u;
    const uint64_t limit = ((uint64_t)1 << 24) - 1;                    // the 24-bit slice size
    const uint64_t want_cap = slice_capacity ? slice_capacity : 2 * max_raw + 4096;
    const uint32_t cap = (uint32_t)(want_cap < limit ? want_cap : limit);
    const size_t slice_stride = ((size_t)cap + 15) & ~(size_t)15;
    const size_t per_frame = (size_t)spf * (slice_stride + sizeof(uint32_t)) + 256;
    const int fchunk = slots_afforded(c, per_frame, n_frames);
    const size_t head = 256;                                           // the running offset, alone on its line
    const size_t words = ((size_t)fchunk * spf * sizeof(uint32_t) + 255) & ~(size_t)255;
    const size_t need = head + words + (size_t)fchunk * spf * slice_stride;
    if (c->ffv1_bytes < need) {
        MDVT_HIP(c, hipDeviceSynchronize());                 // earlier submissions may still use the old workspace
        if (c->ffv1_ws) ws_free(c, c->ffv1_ws);
        c->ffv1_ws = nullptr; c->ffv1_bytes = 0;
        MDVT_HIP(c, ws_malloc(c, (void**)&c->ffv1_ws, need, s));
        c->ffv1_bytes = need;
    }
    unsigned long long* used = reinterpret_cast<unsigned long long*>(c->ffv1_ws);
    uint32_t* slice_n = reinterpret_cast<uint32_t*>(c->ffv1_ws + head);
    uint8_t* scratch = c->ffv1_ws + head + words;
    MDVT_HIP(c, hipMemsetAsync(used, 0, sizeof(unsigned long long), s));
    static const mdvt::Ffv1StateTables tab = mdvt::ffv1_default_states();
    mdvt::Ffv1CodeArgs ca{};
    ca.pitch = pitch; ca.frame_stride = frame_stride; ca.channels = channels;
    ca.ri = channels == 1 ? 0 : (order == 1 ? 2 : 0); ca.gi = channels == 1 ? 0 : 1; ca.bi = channels == 1 ? 0 : (order == 1 ? 0 : 2);
    ca.W = width; ca.H = height; ca.nh = slices_h; ca.nv = slices_v;
    ca.scratch = scratch; ca.slice_stride = slice_stride; ca.cap = cap; ca.cap_is_24bit = cap == (uint32_t)limit; ca.slice_n = slice_n;
    for (int f0 = 0; f0 < n_frames; f0 += fchunk) {
        const int nf = n_frames - f0 < fchunk ? n_frames - f0 : fchunk;
        ca.src = d_src + (size_t)f0 * frame_stride;
        MDVT_HIP(c, mdvt::launch_ffv1_code(ca, tab, nf * spf, s));
        const mdvt::Ffv1LayoutArgs la{slice_n, spf, nf, d_sizes + f0, reinterpret_cast<unsigned long long*>(d_offsets) + f0, used,
                                      (unsigned long long)packets_cap};
        MDVT_HIP(c, mdvt::launch_ffv1_layout(la, s));
        const mdvt::Ffv1EmitArgs ea{slice_n, scratch, slice_stride, spf, d_sizes + f0, reinterpret_cast<unsigned long long*>(d_offsets) + f0,
                                    d_packets};
        MDVT_HIP(c, mdvt::launch_ffv1_emit(ea, nf * spf, s));
    }
    return MDVT_OK;
}

const char* mdvt_ffv1_decode_supported(const uint8_t* h_config, size_t config_size)
{
    mdvt_ffv1::StreamClass sc{};
    return mdvt_ffv1::parse_stream_class(h_config, config_size, &sc);
}

// FFV1 packets in device memory -> frames (mdvt_ffv1_decode.hip).  Passes: as many frames as the ctx's workspace budget affords.
int mdvt_decode_video_frames(mdvt_ctx* c, int width, int height, const uint8_t* h_config, size_t config_size, const uint8_t* d_packets,
                             uint64_t packets_bytes, const uint64_t* d_offsets, const uint32_t* d_sizes, int n_frames, uint8_t* d_dst,
                             size_t pitch, size_t frame_stride, int order, uint32_t* d_status, void* stream)
{
    if (!c) return MDVT_ERR_INVALID_ARG;
    if (!h_config || !d_packets || !d_offsets || !d_sizes || !d_dst || !d_status) return fail(c, MDVT_ERR_INVALID_ARG, "NULL buffer");
    if (width < 1 || height < 1) return fail(c, MDVT_ERR_INVALID_ARG, "bad frame size %d x %d", width, height);
    if (order != 0 && order != 1) return fail(c, MDVT_ERR_INVALID_ARG, "order must be 0 (RGB) or 1 (BGR), got %d", order);
    if (n_frames < 1) return fail(c, MDVT_ERR_INVALID_ARG, "n_frames must be >= 1");
    if (pitch < (size_t)width * 3u) return fail(c, MDVT_ERR_INVALID_ARG, "pitch smaller than one row");
    if (n_frames > 1 && frame_stride < pitch * (size_t)height) return fail(c, MDVT_ERR_INVALID_ARG, "frame_stride smaller than one frame");
    mdvt_ffv1::StreamClass sc{};
    if (const char* why = mdvt_ffv1::parse_stream_class(h_config, config_size, &sc))
        return fail(c, MDVT_ERR_UNSUPPORTED, "FFV1 stream outside the device decoder's class: %s", why);
    if (sc.nh > width || sc.nv > height)
        return fail(c, MDVT_ERR_UNSUPPORTED, "FFV1 stream outside the device decoder's class: num_h_slices / num_v_slices %d x %d for a frame of %d x %d",
                    sc.nh, sc.nv, width, height);
    if ((uint64_t)width * (uint64_t)height > ((uint64_t)1 << 28))
        return fail(c, MDVT_ERR_UNSUPPORTED, "frame too large for the device FFV1 decoder (%d x %d)", width, height);
    const int line_stride = (width + sc.nh - 1) / sc.nh + 2;           // the widest slice, its left and right neighbours
    if (mdvt::ffv1_decode_static_lds_bytes() + mdvt::ffv1_decode_lds_bytes(line_stride) > (size_t)160 * 1024)
        return fail(c, MDVT_ERR_UNSUPPORTED, "a slice of %d pixels' width does not fit the device FFV1 decoder's row buffers (num_h_slices %d)",
                    line_stride - 2, sc.nh);
    DeviceGuard g(c->device);
    hipStream_t s = (hipStream_t)stream;
    const int spf = sc.nh * sc.nv;
    const size_t per_frame = (size_t)spf * 3 * sizeof(uint32_t);
    const int fchunk = slots_afforded(c, per_frame, n_frames);
    const size_t need = (size_t)fchunk * per_frame;
    if (c->ffv1_dec_bytes < need) {
        MDVT_HIP(c, hipDeviceSynchronize());                 // earlier submissions may still use the old workspace
        if (c->ffv1_dec_ws) ws_free(c, c->ffv1_dec_ws);
        c->ffv1_dec_ws = nullptr; c->ffv1_dec_bytes = 0;
        MDVT_HIP(c, ws_malloc(c, (void**)&c->ffv1_dec_ws, need, s));
        c->ffv1_dec_bytes = need;
    }
    static const mdvt::Ffv1StateTables tab = mdvt::ffv1_default_states();
    mdvt::Ffv1DecodeArgs a{};
    a.packets = d_packets; a.packets_bytes = packets_bytes;
    a.W = width; a.H = height; a.nh = sc.nh; a.nv = sc.nv; a.ec = sc.ec;
    a.pitch = pitch; a.frame_stride = frame_stride; a.ri = order == 1 ? 2 : 0; a.bi = order == 1 ? 0 : 2;
    a.line_stride = line_stride;
    for (int f0 = 0; f0 < n_frames; f0 += fchunk) {
        const int nf = n_frames - f0 < fchunk ? n_frames - f0 : fchunk;
        a.n_frames = nf;
        a.offsets = reinterpret_cast<const unsigned long long*>(d_offsets) + f0; a.sizes = d_sizes + f0;
        a.dst = d_dst + (size_t)f0 * frame_stride; a.status = d_status + f0;
        a.table = reinterpret_cast<uint32_t*>(c->ffv1_dec_ws);
        a.claims = a.table + (size_t)2 * nf * spf;
        MDVT_HIP(c, hipMemsetAsync(a.claims, 0, (size_t)nf * spf * sizeof(uint32_t), s));
        MDVT_HIP(c, mdvt::launch_ffv1_decode(a, tab, s));
    }
    return MDVT_OK;
}

// Per-frame masked depth means (mdvt_convergence.hip).  Launch sets: as many frames as the ctx's workspace budget affords.
int mdvt_convergence_depths(mdvt_ctx* c, int width, int height, const uint8_t* d_depth, size_t depth_pitch, size_t depth_stride, int depth_order,
                            const uint8_t* d_mask, size_t mask_pitch, size_t mask_stride, int mask_order, int n_frames, int n_mask_frames,
                            double max_depth, float* d_means, uint32_t* d_counts, void* stream)
{
    if (!c) return MDVT_ERR_INVALID_ARG;
    if (!d_depth || !d_means) return fail(c, MDVT_ERR_INVALID_ARG, "NULL buffer");
    if (width < 1 || height < 1) return fail(c, MDVT_ERR_INVALID_ARG, "bad frame size %d x %d", width, height);
    if (depth_order != 0 && depth_order != 1) return fail(c, MDVT_ERR_INVALID_ARG, "depth_order must be 0 (RGB) or 1 (BGR), got %d", depth_order);
    if (n_frames < 1) return fail(c, MDVT_ERR_INVALID_ARG, "n_frames must be >= 1");
    if (n_mask_frames < 0 || n_mask_frames > n_frames) return fail(c, MDVT_ERR_INVALID_ARG, "n_mask_frames %d outside [0, n_frames = %d]", n_mask_frames, n_frames);
    if (n_mask_frames > 0 && !d_mask) return fail(c, MDVT_ERR_INVALID_ARG, "n_mask_frames %d without a mask", n_mask_frames);
    if (!(max_depth > 0.0)) return fail(c, MDVT_ERR_INVALID_ARG, "max_depth must be > 0");
    if (depth_pitch < (size_t)width * 3u) return fail(c, MDVT_ERR_INVALID_ARG, "depth_pitch smaller than one row");
    if (n_frames > 1 && depth_stride < depth_pitch * (size_t)height) return fail(c, MDVT_ERR_INVALID_ARG, "depth_stride smaller than one frame");
    const bool with_mask = d_mask && n_mask_frames > 0;
    if (with_mask) {
        if (mask_order != 0 && mask_order != 1) return fail(c, MDVT_ERR_INVALID_ARG, "mask_order must be 0 (RGB) or 1 (BGR), got %d", mask_order);
        if (mask_pitch < (size_t)width * 3u) return fail(c, MDVT_ERR_INVALID_ARG, "mask_pitch smaller than one row");
        if (n_mask_frames > 1 && mask_stride < mask_pitch * (size_t)height) return fail(c, MDVT_ERR_INVALID_ARG, "mask_stride smaller than one frame");
    }
    if ((uint64_t)width * (uint64_t)height > ((uint64_t)1 << 28))
        return fail(c, MDVT_ERR_UNSUPPORTED, "frame too large for the convergence depths (%d x %d)", width, height);
    DeviceGuard g(c->device);
    hipStream_t s = (hipStream_t)stream;
    const uint32_t npx = (uint32_t)width * (uint32_t)height;
    const uint32_t nchunks = (npx + 8191u) / 8192u, nunits = (npx + 2047u) / 2048u;
    auto up16 = [](size_t v) { return (v + 15) & ~(size_t)15; };
    // per frame of a set: the chunk sums; with a mask the ballot words (1 bit/px), the selected codes (2 B/px), unit counts and offsets, the count
    const size_t bits_bytes = with_mask ? (size_t)nunits * 32 * sizeof(unsigned long long) : 0;
    const size_t compact_stride = ((size_t)npx + 7) & ~(size_t)7;
    const size_t compact_bytes = with_mask ? compact_stride * sizeof(uint16_t) : 0;
    const size_t sums_bytes = up16((size_t)nchunks * sizeof(float));
    const size_t unit_bytes = with_mask ? up16((size_t)nunits * sizeof(uint32_t)) : 0;
    const size_t per_frame = bits_bytes + compact_bytes + sums_bytes + 2 * unit_bytes + (with_mask ? 16 : 0);
    const int fchunk = slots_afforded(c, per_frame, n_frames < 4096 ? n_frames : 4096);
    const size_t need = (size_t)fchunk * per_frame;
    if (c->conv_bytes < need) {
        MDVT_HIP(c, hipDeviceSynchronize());                 // earlier submissions may still use the old workspace
        if (c->conv_ws) ws_free(c, c->conv_ws);
        c->conv_ws = nullptr; c->conv_bytes = 0;
        MDVT_HIP(c, ws_malloc(c, (void**)&c->conv_ws, need, s));
        c->conv_bytes = need;
    }
    // rows without padding are one long row of npx pixels: no division per pixel, and the 12-byte loads need npx % 4 == 0 only
    const uint32_t depth_W = depth_pitch == (size_t)width * 3u ? npx : (uint32_t)width;
    const uint32_t mask_W = with_mask && mask_pitch == (size_t)width * 3u ? npx : (uint32_t)width;
    auto vec_ok = [&](const uint8_t* p, uint32_t row, size_t pitch, size_t stride) {
        return row % 4 == 0 && pitch % 4 == 0 && stride % 4 == 0 && (uintptr_t)p % 4 == 0;
    };
    mdvt::ConvergenceArgs a{};
    a.depth_pitch = depth_pitch; a.depth_stride = depth_stride; a.depth_bgr = depth_order; a.depth_W = depth_W;
    a.depth_vec = vec_ok(d_depth, depth_W, depth_pitch, depth_stride);
    a.mask_pitch = mask_pitch; a.mask_stride = mask_stride; a.mask_bgr = mask_order; a.mask_W = mask_W;
    a.mask_vec = with_mask && vec_ok(d_mask, mask_W, mask_pitch, mask_stride);
    a.npx = npx; a.nchunks = nchunks; a.nunits = nunits;
    a.div = (float)(4228250625.0 / max_depth);               // 255^4 / max_depth in double, rounded once (fcd:60)
    a.compact_stride = compact_stride;
    uint8_t* w = c->conv_ws;
    a.bits = reinterpret_cast<unsigned long long*>(w); w += (size_t)fchunk * bits_bytes;
    a.compact = reinterpret_cast<uint16_t*>(w); w += (size_t)fchunk * compact_bytes;
    a.sums = reinterpret_cast<float*>(w); w += (size_t)fchunk * sums_bytes;
    a.unit_cnt = reinterpret_cast<uint32_t*>(w); w += (size_t)fchunk * unit_bytes;
    a.unit_off = reinterpret_cast<uint32_t*>(w); w += (size_t)fchunk * unit_bytes;
    a.totals = reinterpret_cast<uint32_t*>(w);
    for (int f0 = 0; f0 < n_frames; f0 += fchunk) {
        a.n_frames = n_frames - f0 < fchunk ? n_frames - f0 : fchunk;
        a.n_masked = n_mask_frames - f0 < 0 ? 0 : n_mask_frames - f0 < a.n_frames ? n_mask_frames - f0 : a.n_frames;
        a.depth = d_depth + (size_t)f0 * depth_stride;
        a.mask = a.n_masked ? d_mask + (size_t)f0 * mask_stride : nullptr;
        a.means = d_means + f0; a.counts = d_counts ? d_counts + f0 : nullptr;
        MDVT_HIP(c, mdvt::launch_convergence(a, s));
    }
    return MDVT_OK;
}

}  // extern "C"
