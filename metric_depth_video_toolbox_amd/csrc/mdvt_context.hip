// mdvt_context.hip -- the context's life cycle and the memory the library owns: the process-wide pool of device workspace blocks,
// the pool of pinned parameter blocks, the banks' stream and events, the scratch blocks' growth rule (stated in mdvt_context.h),
// and mdvt_create / destroy / set_config / set_near_clip / last_error / version / selftest / workspace_bytes / *cached_memory*.
// Host code only.
#include "mdvt_context.h"

#include <stdarg.h>

#include <map>
#include <mutex>
#include <new>

using namespace mdvt;
using namespace mdvt::host;

static thread_local std::string g_create_error;       // mdvt_create's error text: there is no context to hold it

int mdvt::host::fail(mdvt_ctx* c, int code, const char* fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (c) c->err = buf; else g_create_error = buf;
    return code;
}

namespace {

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

}  // namespace

// device memory owned by a context, accounted for mdvt_workspace_bytes; `s`: the stream the fresh-block fill goes to
hipError_t mdvt::host::ws_malloc(mdvt_ctx* c, void** p, size_t bytes, hipStream_t s)
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
void mdvt::host::ws_free(mdvt_ctx* c, void* p)
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

hipError_t mdvt::host::scratch_reserve(mdvt_ctx* c, Scratch& b, size_t need, hipStream_t s, bool* grew)
{
    if (b.bytes >= need) return hipSuccess;
    if (b.p) {
        const hipError_t e = hipDeviceSynchronize();
        if (e != hipSuccess) return e;
        ws_free(c, b.p);
    }
    b = Scratch{};
    void* p = nullptr;
    const hipError_t e = ws_malloc(c, &p, need, s);
    if (e != hipSuccess) return e;
    b.p = (uint8_t*)p; b.bytes = need;
    if (grew) *grew = true;
    return hipSuccess;
}

namespace {

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

}  // namespace

// A pinned host block of at least `bytes`, with a device block of the same size on GPU `device` if with_dev (a block that
// carries device memory only ever goes back to a context on the GPU it was allocated on: contexts of two GPUs share the pool).
hipError_t mdvt::host::pool_take(size_t bytes, bool with_dev, int device, void** host, void** dev, size_t* got)
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
void mdvt::host::pool_give(void* host, void* dev, size_t bytes, int device)
{
    if (!host) return;
    if (param_pool_off()) { (void)hipHostFree(host); if (dev) (void)hipFree(dev); return; }
    std::lock_guard<std::mutex> lock(g_pool_mutex);
    param_pool().push_back({host, dev, bytes, dev ? device : -1});
}

void mdvt::host::pool_idle_blocks(int tag, uint64_t counts[4])
{
    for (int k = 0; k < 4; ++k) counts[k] = 0;
    { std::lock_guard<std::mutex> lock(g_pool_mutex); for (const PoolBlock& b : param_pool()) if (b.device >= 0) ++counts[b.device == tag ? 0 : 1]; }
    { std::lock_guard<std::mutex> lock(g_dev_pool_mutex); for (const DevBlock& b : dev_pool()) ++counts[b.tag == tag ? 2 : 3]; }
}

// ---- The banks' side stream and events: process-wide, never destroyed ------------------------------------------------------
// r05: three soak processes in ~3 000 multi-frame sweep jobs (300 k contexts that had used banks) died of a signal -- never one of
// 3 500 single-frame jobs (1.4 M contexts) -- and the native backtrace of the third (tools/probe/segv_trace.c) is the HSA runtime's
// own callback thread faulting inside libamdhip64, not a frame of this library.  What only the bank path has is a stream and four
// events created by a context and destroyed with it; whatever the runtime's handler still holds of them after the
// hipDeviceSynchronize of mdvt_destroy, the library no longer destroys them: they wait here for the next context of the same GPU
// that uses banks (the treatment the pinned parameter blocks and the workspace blocks got for their own reasons).
namespace {
struct BankRes { hipStream_t side; hipEvent_t ev[4]; int device; };
std::mutex g_bank_mutex;
std::vector<BankRes>& bank_pool() { static std::vector<BankRes>* p = new std::vector<BankRes>(); return *p; }      // (leaked on purpose)
}  // namespace

hipError_t mdvt::host::bank_res_take(mdvt_ctx* c)
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
    // (the order in which the blocks reach the pool is the order it hands them out again, newest first: kept as it has been)
    void* const render_ws[] = {c->hugeq2, c->keys[0], c->ekeys[0], c->cbuf[0], c->keys[1], c->ekeys[1], c->cbuf[1], c->bigq, c->tri_invalid, c->unused, c->elist};
    for (void* p : render_ws) ws_free(c, p);      // (ws_free takes a null pointer)
    for (int k = 0; k < SCR_COUNT; ++k) {
        if (k == SCR_MSAA_KEYS) { ws_free(c, c->divcheck); ws_free(c, c->rowcell); }     // (made once, not grown: their place in that order)
        ws_free(c, c->scratch[k].p);
    }
    if (c->div_done) (void)hipEventDestroy(c->div_done);
    pool_give(c->telea_levels_host, nullptr, 64, -1);
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

int mdvt_workspace_bytes(mdvt_ctx* c, uint64_t* bytes)
{
    if (!c) return MDVT_ERR_INVALID_ARG;
    if (!bytes) return fail(c, MDVT_ERR_INVALID_ARG, "NULL argument");
    *bytes = (uint64_t)c->ws_bytes;
    return MDVT_OK;
}

}  // extern "C"
