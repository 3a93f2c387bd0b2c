// mdvt_inspatio.hip -- the alignment of the reference's InSpatio-World infill step (include/mdvt_inspatio.h): the 4 x 4 grid of
// masked cross-correlation shifts between a blacked render and the video model's frame (mdvt_masked_shift_grid).
//
// The unit is compiled with -ffp-contract=off, IEEE division and without fast-math (Makefile): every `*`, `+`, `-` and `/` below is
// one IEEE operation, rounded before the next; the square root is __dsqrt_rn.  The header states the arithmetic; this is how the
// work is laid out.
//
// k_shift_gate     a workgroup per cell: its valid pixels and whether it is computed at all.
// k_shift_border   a workgroup per border cell (gx = 0, 3): the row means, then a thread per dy, everything in LDS.
// Interior cells (gx = 1, 2), a "unit" each, in launch sets; a unit owns three complex float64 planes of Ly x Lx, the displacement
// (dy, dx) at row (dy + Ly) % Ly, column (dx + Lx) % Lx:  plane 0 = (N, FR), plane 1 = (SF, FF), plane 2 = (SR, RR).
//   direct:     k_shift_direct, a thread per displacement, the cell's a = gI V, b = gR V and V in LDS, 32-bit integer sums (a cell
//               of at most 16384 pixels: 255^2 * 16384 < 2^32); Ly = 2 hmax - 1, Lx = 2 wmax - 1.
//   transform:  Ly, Lx powers of two.  k_shift_rows_fwd fills a row of V, a + i a^2, b - i b^2 and transforms it; k_shift_cols
//               transforms columns (the rows past the cell's are zero and are not read); k_shift_product forms, in place,
//               V V* + i A B*, (A + i A2) V* and V (B - i B2)* -- only the first needs A and B apart, from the plane's mirror
//               element, so a thread takes a frequency and its mirror; k_shift_cols and k_shift_rows_inv transform back.  A line is
//               transformed in LDS: loaded in bit-reversed order, log2 L radix-2 passes in place, twiddles from sincospi.
// k_shift_peak<1>  rounds the six sums (transform: rint, and the largest distance rounded), num and den; the maxima of den and N.
// k_shift_peak<2>  c, its maximum.   k_shift_peak<3>  the number and index sums of the maxima.   k_shift_finish  the division.
// The maxima are integer maxima of order-preserving keys and the index sums integer sums: no floating-point atomics.
//
// k_flow_warp      mdvt_flow_warp: a thread per output pixel (below, at the kernel).
// k_insp_grow, k_insp_composite   mdvt_inspatio_composite_eye: the marks' three dilations, then the paste and the blend per pixel.
// k_insp_eye, k_insp_model   mdvt_inspatio_prepare_eye and mdvt_inspatio_model_frames: a thread per eye pixel / per model pixel.
#include "mdvt_internal.h"
#include "mdvt_device.h"
#include "mdvt_depth_code.h"
#include "mdvt_adapter_resize.h"

namespace mdvt {
namespace {

struct Cell { int y0, x0, h, w; };

__device__ __forceinline__ Cell cell_of(const ShiftGridArgs& a, int gy, int gx)
{
    Cell c;
    c.y0 = gy * a.H / 4; c.x0 = gx * a.W / 4;
    c.h = (gy + 1) * a.H / 4 - c.y0; c.w = (gx + 1) * a.W / 4 - c.x0;
    return c;
}

// the interior cell of unit u: frame u / 8, gy = (u % 8) / 2, gx = 1 + u % 2
__device__ __forceinline__ Cell unit_cell(const ShiftGridArgs& a, uint32_t u, size_t& f, uint32_t& cid)
{
    f = u / 8u;
    const int gy = (int)((u % 8u) / 2u), gx = 1 + (int)(u & 1u);
    cid = (uint32_t)f * 16u + (uint32_t)(gy * 4 + gx);
    return cell_of(a, gy, gx);
}

__device__ __forceinline__ uint32_t grey_at(const uint8_t* img, size_t pitch, int y, int x)
{
    const uint8_t* p = img + (size_t)y * pitch + (size_t)x * 3u;
    return (4899u * p[0] + 9617u * p[1] + 1868u * p[2] + 8192u) >> 14;
}

// the displacement of a plane's row or column index: i < nmax ? i : i - L
__device__ __forceinline__ int disp_of(int i, int nmax, int L) { return i < nmax ? i : i - L; }

__device__ __forceinline__ void num_den(double N, double SF, double SR, double FR, double FF, double RR, double& num, double& den)
{
    if (N == 0.0) { num = 0.0; den = 0.0; return; }
    num = FR - (SF * SR) / N;
    double fd = FF - (SF * SF) / N, rd = RR - (SR * SR) / N;
    fd = fd > 0.0 ? fd : 0.0;
    rd = rd > 0.0 ? rd : 0.0;
    den = __dsqrt_rn(fd * rd);
}

__device__ __forceinline__ double corr_of(double num, double den, double N, double max_den, double max_n)
{
    const double tol = 0x1.f4p-14 * max_den;                        // 1000 * 2^-23
    double c = 0.0;
    if (den > tol) {
        c = num / den;
        c = c < -1.0 ? -1.0 : c;
        c = c > 1.0 ? 1.0 : c;
    }
    if (N < 0.3 * max_n) c = 0.0;
    return c == 0.0 ? 0.0 : c;                                      // one zero
}

// a float64 as an integer of the same order
__device__ __forceinline__ unsigned long long key_of(double c)
{
    const unsigned long long u = (unsigned long long)__double_as_longlong(c);
    return (u >> 63) ? ~u : (u | (1ull << 63));
}

// ---- the gate ----------------------------------------------------------------------------------------------------------------------

__global__ void __launch_bounds__(256) k_shift_gate(ShiftGridArgs a)
{
    __shared__ uint32_t s_n;
    const uint32_t cid = blockIdx.x;
    const size_t f = cid / 16u;
    const Cell c = cell_of(a, (int)(cid % 16u) / 4, (int)(cid % 4u));
    if (threadIdx.x == 0) s_n = 0;
    __syncthreads();
    const uint8_t* v = a.valid + f * a.valid_stride;
    uint32_t n = 0;
    for (int i = (int)threadIdx.x; i < c.h * c.w; i += 256) {
        const int y = i / c.w, x = i - y * c.w;
        n += v[(size_t)(c.y0 + y) * a.valid_pitch + (size_t)(c.x0 + x)] != 0;
    }
    atomicAdd(&s_n, n);
    __syncthreads();
    if (threadIdx.x == 0) {
        // (an active cell has at least one valid pixel, so a border cell that passes this gate has a row with a valid pixel: the
        // header's second condition for border columns, "no row has a valid pixel", needs no test of its own in k_shift_border)
        a.state[cid].n_valid = s_n;
        a.state[cid].active = ((double)s_n / (double)(c.h * c.w) < 0.2) ? 0u : 1u;
    }
}

// ---- border columns ----------------------------------------------------------------------------------------------------------------

__global__ void __launch_bounds__(256) k_shift_border(ShiftGridArgs a)
{
    __shared__ float s_r[kShiftMaxCell], s_q[kShiftMaxCell];
    __shared__ uint8_t s_m[kShiftMaxCell];
    __shared__ double s_num[2 * kShiftMaxCell], s_den[2 * kShiftMaxCell];      // s_num holds c from the third phase on
    __shared__ int s_nn[2 * kShiftMaxCell];
    __shared__ unsigned long long s_max[3], s_count;
    __shared__ long long s_sum;
    const uint32_t b = blockIdx.x;
    const size_t f = b / 8u;
    const int gy = (int)(b % 8u) / 2, gx = (b & 1u) ? 3 : 0;
    const uint32_t cid = (uint32_t)f * 16u + (uint32_t)(gy * 4 + gx);
    if (!a.state[cid].active) return;
    const Cell c = cell_of(a, gy, gx);
    const uint8_t* R = a.render + f * a.render_stride;
    const uint8_t* I = a.infilled + f * a.infilled_stride;
    const uint8_t* V = a.valid + f * a.valid_stride;
    if (threadIdx.x < 3) s_max[threadIdx.x] = 0;
    if (threadIdx.x == 3) { s_count = 0; s_sum = 0; }
    for (int y = (int)threadIdx.x; y < c.h; y += 256) {
        uint32_t sr = 0, sq = 0, ny = 0;
        for (int x = 0; x < c.w; ++x) {
            if (V[(size_t)(c.y0 + y) * a.valid_pitch + (size_t)(c.x0 + x)]) {
                sr += grey_at(R, a.render_pitch, c.y0 + y, c.x0 + x);
                sq += grey_at(I, a.infilled_pitch, c.y0 + y, c.x0 + x);
                ++ny;
            }
        }
        const float cnt = ny ? (float)ny : 1e-8f;
        s_r[y] = (float)sr / cnt;
        s_q[y] = (float)sq / cnt;
        s_m[y] = ny != 0;
    }
    __syncthreads();
    const int D = 2 * c.h - 1;
    for (int i = (int)threadIdx.x; i < D; i += 256) {
        const int dy = i - (c.h - 1);
        const int ya = dy > 0 ? dy : 0, yb = dy < 0 ? c.h + dy : c.h;
        double N = 0.0, SF = 0.0, SR = 0.0, FR = 0.0, FF = 0.0, RR = 0.0;
        int nn = 0;
        for (int y = ya; y < yb; ++y) {
            if (s_m[y] && s_m[y - dy]) {
                const double p = (double)s_q[y], q = (double)s_r[y - dy];
                ++nn;
                SF = SF + p; SR = SR + q; FR = FR + p * q; FF = FF + p * p; RR = RR + q * q;
            }
        }
        N = (double)nn;
        double num, den;
        num_den(N, SF, SR, FR, FF, RR, num, den);
        s_num[i] = num; s_den[i] = den; s_nn[i] = nn;
        atomicMax(&s_max[0], (unsigned long long)__double_as_longlong(den));    // den >= 0: its bits order as it does
        atomicMax(&s_max[1], (unsigned long long)nn);
    }
    __syncthreads();
    const double max_den = __longlong_as_double((long long)s_max[0]), max_n = (double)s_max[1];
    for (int i = (int)threadIdx.x; i < D; i += 256) {
        const double cc = corr_of(s_num[i], s_den[i], (double)s_nn[i], max_den, max_n);
        s_num[i] = cc;
        atomicMax(&s_max[2], key_of(cc));
    }
    __syncthreads();
    for (int i = (int)threadIdx.x; i < D; i += 256) {
        if (key_of(s_num[i]) == s_max[2]) {
            atomicAdd(&s_count, 1ull);
            atomicAdd((unsigned long long*)&s_sum, (unsigned long long)(long long)(i - (c.h - 1)));
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        a.state[cid].count = s_count;
        a.state[cid].sum_dy = s_sum;
        a.state[cid].sum_dx = 0;
    }
}

// ---- interior columns: the sums in integers ----------------------------------------------------------------------------------------

__global__ void __launch_bounds__(256) k_shift_direct(ShiftGridArgs a)
{
    __shared__ uint8_t s_a[kShiftDirectPixels], s_b[kShiftDirectPixels], s_v[kShiftDirectPixels];
    size_t f;
    uint32_t cid;
    const Cell c = unit_cell(a, (uint32_t)a.unit0 + blockIdx.z, f, cid);
    if (!a.state[cid].active) return;
    const uint8_t* R = a.render + f * a.render_stride;
    const uint8_t* I = a.infilled + f * a.infilled_stride;
    const uint8_t* V = a.valid + f * a.valid_stride;
    for (int i = (int)threadIdx.x; i < c.h * c.w; i += 256) {       // h * w <= hmax * wmax <= kShiftDirectPixels (the host's check)
        const int y = i / c.w, x = i - y * c.w;
        const bool v = V[(size_t)(c.y0 + y) * a.valid_pitch + (size_t)(c.x0 + x)] != 0;
        s_v[i] = v;
        s_a[i] = v ? (uint8_t)grey_at(I, a.infilled_pitch, c.y0 + y, c.x0 + x) : (uint8_t)0;
        s_b[i] = v ? (uint8_t)grey_at(R, a.render_pitch, c.y0 + y, c.x0 + x) : (uint8_t)0;
    }
    __syncthreads();
    const uint32_t p = blockIdx.x * 256u + threadIdx.x;
    if (p >= (uint32_t)(a.Ly * a.Lx)) return;
    const int iy = (int)(p / (uint32_t)a.Lx), ix = (int)(p - (uint32_t)iy * (uint32_t)a.Lx);
    const int dy = disp_of(iy, a.hmax, a.Ly), dx = disp_of(ix, a.wmax, a.Lx);
    if (dy > c.h - 1 || -dy > c.h - 1 || dx > c.w - 1 || -dx > c.w - 1) return;
    const int ya = dy > 0 ? dy : 0, yb = dy < 0 ? c.h + dy : c.h;
    const int xa = dx > 0 ? dx : 0, xb = dx < 0 ? c.w + dx : c.w;
    uint32_t N = 0, SF = 0, SR = 0, FR = 0, FF = 0, RR = 0;
    for (int y = ya; y < yb; ++y) {
        const int ra = y * c.w, rb = (y - dy) * c.w - dx;
        for (int x = xa; x < xb; ++x) {
            const uint32_t pa = s_a[ra + x], pb = s_b[rb + x], va = s_v[ra + x], vb = s_v[rb + x];
            N += va & vb; SF += pa * vb; SR += pb * va; FR += pa * pb; FF += pa * pa * vb; RR += pb * pb * va;
        }
    }
    double2* pl = a.planes + (size_t)blockIdx.z * 3u * a.plane;
    pl[p] = make_double2((double)N, (double)FR);
    pl[a.plane + p] = make_double2((double)SF, (double)FF);
    pl[2u * a.plane + p] = make_double2((double)SR, (double)RR);
}

// ---- interior columns: the sums by transform ---------------------------------------------------------------------------------------

__device__ __forceinline__ double2 cmul(double2 x, double2 y) { return make_double2(x.x * y.x - x.y * y.y, x.x * y.y + x.y * y.x); }

// exp(-2 pi i j / L), j < L / 2
__device__ __forceinline__ void twiddles(double2* tw, int L)
{
    for (int j = (int)threadIdx.x; j < L / 2; j += 256) {
        double sn, cs;
        sincospi(-2.0 * (double)j / (double)L, &sn, &cs);
        tw[j] = make_double2(cs, sn);
    }
}

// nl lines of L = 1 << logL values each, in bit-reversed order on entry, transformed in place (inv: the conjugate twiddles, no scale)
__device__ __forceinline__ void fft_lines(double2* s, const double2* tw, int logL, int nl, bool inv)
{
    const int L = 1 << logL, halfL = L >> 1;
    for (int st = 1; st <= logL; ++st) {
        const int half = 1 << (st - 1), tstep = L >> st;
        for (int i = (int)threadIdx.x; i < nl * halfL; i += 256) {
            const int line = i >> (logL - 1), t = i & (halfL - 1);
            const int j = t & (half - 1), k0 = ((t >> (st - 1)) << st) + j;
            double2 w = tw[j * tstep];
            if (inv) w.y = -w.y;
            double2* x = s + line * L;
            const double2 u = x[k0], v = cmul(x[k0 + half], w);
            x[k0] = make_double2(u.x + v.x, u.y + v.y);
            x[k0 + half] = make_double2(u.x - v.x, u.y - v.y);
        }
        __syncthreads();
    }
}

__device__ __forceinline__ int bitrev(int i, int logL) { return (int)(__brev((uint32_t)i) >> (32 - logL)); }

// grid (hmax, 3, units): row y of plane k from the images, transformed
__global__ void __launch_bounds__(256) k_shift_rows_fwd(ShiftGridArgs a)
{
    extern __shared__ double2 s_fft[];                              // [lines][L] values, then [L / 2] twiddles
    size_t f;
    uint32_t cid;
    const Cell c = unit_cell(a, (uint32_t)a.unit0 + blockIdx.z, f, cid);
    const int y = (int)blockIdx.x, k = (int)blockIdx.y;
    if (!a.state[cid].active || y >= c.h) return;
    double2* tw = s_fft + a.Lx;
    twiddles(tw, a.Lx);
    const uint8_t* V = a.valid + f * a.valid_stride + (size_t)(c.y0 + y) * a.valid_pitch + (size_t)c.x0;
    const uint8_t* img = k == 1 ? a.infilled + f * a.infilled_stride : a.render + f * a.render_stride;
    const size_t pitch = k == 1 ? a.infilled_pitch : a.render_pitch;
    for (int x = (int)threadIdx.x; x < a.Lx; x += 256) {
        double2 z = make_double2(0.0, 0.0);
        if (x < c.w && V[x]) {
            if (k == 0) {
                z.x = 1.0;
            } else {
                const double g = (double)grey_at(img, pitch, c.y0 + y, c.x0 + x);
                z = make_double2(g, k == 1 ? g * g : -(g * g));
            }
        }
        s_fft[bitrev(x, a.log_lx)] = z;
    }
    __syncthreads();
    fft_lines(s_fft, tw, a.log_lx, 1, false);
    double2* row = a.planes + ((size_t)blockIdx.z * 3u + (size_t)k) * a.plane + (size_t)y * (size_t)a.Lx;
    for (int x = (int)threadIdx.x; x < a.Lx; x += 256) row[x] = s_fft[x];
}

// grid (Lx / nl, 3, units): nl columns of plane k; forward: the rows from the cell's h on are zero and are not read
__global__ void __launch_bounds__(256) k_shift_cols(ShiftGridArgs a, int nl, int inv)
{
    extern __shared__ double2 s_fft[];                              // [lines][L] values, then [L / 2] twiddles
    size_t f;
    uint32_t cid;
    const Cell c = unit_cell(a, (uint32_t)a.unit0 + blockIdx.z, f, cid);
    if (!a.state[cid].active) return;
    double2* tw = s_fft + nl * a.Ly;
    twiddles(tw, a.Ly);
    const int x0 = (int)blockIdx.x * nl, rows_in = inv ? a.Ly : c.h;
    double2* pl = a.planes + ((size_t)blockIdx.z * 3u + (size_t)blockIdx.y) * a.plane;
    for (int i = (int)threadIdx.x; i < nl * a.Ly; i += 256) {
        const int y = i / nl, l = i - y * nl;
        s_fft[l * a.Ly + bitrev(y, a.log_ly)] = y < rows_in ? pl[(size_t)y * (size_t)a.Lx + (size_t)(x0 + l)] : make_double2(0.0, 0.0);
    }
    __syncthreads();
    fft_lines(s_fft, tw, a.log_ly, nl, inv != 0);
    for (int i = (int)threadIdx.x; i < nl * a.Ly; i += 256) {
        const int y = i / nl, l = i - y * nl;
        pl[(size_t)y * (size_t)a.Lx + (size_t)(x0 + l)] = s_fft[l * a.Ly + y];
    }
}

__device__ __forceinline__ double2 conj_of(double2 z) { return make_double2(z.x, -z.y); }

// what the three planes hold at one frequency, from their values there (v, z1, z2) and at the mirror frequency (m1, m2)
__device__ __forceinline__ void products(double2 v, double2 z1, double2 z2, double2 m1, double2 m2, double2& p0, double2& p1, double2& p2)
{
    const double2 A = make_double2((z1.x + m1.x) * 0.5, (z1.y - m1.y) * 0.5);          // the transform of a: (z1 + conj(m1)) / 2
    const double2 B = make_double2((z2.x + m2.x) * 0.5, (z2.y - m2.y) * 0.5);
    const double2 ab = cmul(A, conj_of(B));
    p0 = make_double2((v.x * v.x + v.y * v.y) - ab.y, ab.x);                           // V V* + i A B*
    p1 = cmul(z1, conj_of(v));
    p2 = cmul(v, conj_of(z2));
}

// grid (ceil(Ly * Lx / 256), 1, units): a thread per frequency whose index is not above its mirror's, in place
__global__ void __launch_bounds__(256) k_shift_product(ShiftGridArgs a)
{
    size_t f;
    uint32_t cid;
    unit_cell(a, (uint32_t)a.unit0 + blockIdx.z, f, cid);
    if (!a.state[cid].active) return;
    const uint32_t p = blockIdx.x * 256u + threadIdx.x;
    if (p >= (uint32_t)(a.Ly * a.Lx)) return;
    const uint32_t ky = p >> a.log_lx, kx = p & (uint32_t)(a.Lx - 1);
    const uint32_t pm = ((((uint32_t)a.Ly - ky) & (uint32_t)(a.Ly - 1)) << a.log_lx) | (((uint32_t)a.Lx - kx) & (uint32_t)(a.Lx - 1));
    if (p > pm) return;
    double2* pl0 = a.planes + (size_t)blockIdx.z * 3u * a.plane;
    double2* pl1 = pl0 + a.plane;
    double2* pl2 = pl1 + a.plane;
    const double2 v = pl0[p], z1 = pl1[p], z2 = pl2[p], vm = pl0[pm], m1 = pl1[pm], m2 = pl2[pm];
    double2 p0, p1, p2;
    products(v, z1, z2, m1, m2, p0, p1, p2);
    pl0[p] = p0; pl1[p] = p1; pl2[p] = p2;
    if (pm != p) {
        products(vm, m1, m2, z1, z2, p0, p1, p2);
        pl0[pm] = p0; pl1[pm] = p1; pl2[pm] = p2;
    }
}

// grid (Ly, 3, units): row r of plane k back, scaled by 1 / (Lx Ly) (a power of two: exact); rows of no displacement are skipped
__global__ void __launch_bounds__(256) k_shift_rows_inv(ShiftGridArgs a)
{
    extern __shared__ double2 s_fft[];                              // [lines][L] values, then [L / 2] twiddles
    size_t f;
    uint32_t cid;
    const Cell c = unit_cell(a, (uint32_t)a.unit0 + blockIdx.z, f, cid);
    const int dy = disp_of((int)blockIdx.x, a.hmax, a.Ly);
    if (!a.state[cid].active || dy > c.h - 1 || -dy > c.h - 1) return;
    double2* tw = s_fft + a.Lx;
    twiddles(tw, a.Lx);
    double2* row = a.planes + ((size_t)blockIdx.z * 3u + (size_t)blockIdx.y) * a.plane + (size_t)blockIdx.x * (size_t)a.Lx;
    for (int x = (int)threadIdx.x; x < a.Lx; x += 256) s_fft[bitrev(x, a.log_lx)] = row[x];
    __syncthreads();
    fft_lines(s_fft, tw, a.log_lx, 1, true);
    const double scale = 1.0 / ((double)a.Lx * (double)a.Ly);
    for (int x = (int)threadIdx.x; x < a.Lx; x += 256) row[x] = make_double2(s_fft[x].x * scale, s_fft[x].y * scale);
}

// ---- interior columns: from the sums to the maxima ---------------------------------------------------------------------------------

__device__ __forceinline__ double rounded(double x, double& err)
{
    const double r = rint(x);
    const double e = fabs(x - r);
    err = e > err ? e : err;
    return r;
}

// grid (ceil(Ly * Lx / 256), 1, units).  PHASE 1: planes -> rounded sums, plane 1 = (num, den); 2: plane 2 = (c, .); 3: the maxima's sums
template <int PHASE>
__global__ void __launch_bounds__(256) k_shift_peak(ShiftGridArgs a)
{
    __shared__ unsigned long long s_red[3];
    __shared__ long long s_sum[2];
    size_t f;
    uint32_t cid;
    const Cell c = unit_cell(a, (uint32_t)a.unit0 + blockIdx.z, f, cid);
    ShiftCellState& st = a.state[cid];
    if (!st.active) return;
    if (threadIdx.x < 3) s_red[threadIdx.x] = 0;
    if (threadIdx.x < 2) s_sum[threadIdx.x] = 0;
    __syncthreads();
    const uint32_t p = blockIdx.x * 256u + threadIdx.x;
    bool live = p < (uint32_t)(a.Ly * a.Lx);
    int dy = 0, dx = 0;
    if (live) {
        const int iy = (int)(p / (uint32_t)a.Lx), ix = (int)(p - (uint32_t)iy * (uint32_t)a.Lx);
        dy = disp_of(iy, a.hmax, a.Ly); dx = disp_of(ix, a.wmax, a.Lx);
        live = !(dy > c.h - 1 || -dy > c.h - 1 || dx > c.w - 1 || -dx > c.w - 1);
    }
    double2* pl0 = a.planes + (size_t)blockIdx.z * 3u * a.plane;
    double2* pl1 = pl0 + a.plane;
    double2* pl2 = pl1 + a.plane;
    if (PHASE == 1) {
        if (live) {
            double err = 0.0;
            const double2 z0 = pl0[p], z1 = pl1[p], z2 = pl2[p];
            const double N = rounded(z0.x, err), FR = rounded(z0.y, err), SF = rounded(z1.x, err), FF = rounded(z1.y, err);
            const double SR = rounded(z2.x, err), RR = rounded(z2.y, err);
            double num, den;
            num_den(N, SF, SR, FR, FF, RR, num, den);
            pl0[p] = make_double2(N, FR);
            pl1[p] = make_double2(num, den);
            atomicMax(&s_red[0], (unsigned long long)__double_as_longlong(den));
            atomicMax(&s_red[1], (unsigned long long)N);
            atomicMax(&s_red[2], (unsigned long long)__double_as_longlong(err));
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            atomicMax(&st.max_den, s_red[0]);
            atomicMax(&st.max_n, s_red[1]);
            atomicMax(a.round_err, s_red[2]);
        }
    } else if (PHASE == 2) {
        if (live) {
            const double2 nd = pl1[p];
            const double cc = corr_of(nd.x, nd.y, pl0[p].x, __longlong_as_double((long long)st.max_den), (double)st.max_n);
            pl2[p] = make_double2(cc, 0.0);
            atomicMax(&s_red[0], key_of(cc));
        }
        __syncthreads();
        if (threadIdx.x == 0 && s_red[0]) atomicMax(&st.max_c, s_red[0]);
    } else {
        if (live && key_of(pl2[p].x) == st.max_c) {
            atomicAdd(&s_red[0], 1ull);
            atomicAdd((unsigned long long*)&s_sum[0], (unsigned long long)(long long)dy);
            atomicAdd((unsigned long long*)&s_sum[1], (unsigned long long)(long long)dx);
        }
        __syncthreads();
        if (threadIdx.x == 0 && s_red[0]) {
            atomicAdd(&st.count, s_red[0]);
            atomicAdd((unsigned long long*)&st.sum_dy, (unsigned long long)s_sum[0]);
            atomicAdd((unsigned long long*)&st.sum_dx, (unsigned long long)s_sum[1]);
        }
    }
}

// a thread per cell of the call: the one division per axis; thread 0: the largest distance rounded
__global__ void __launch_bounds__(256) k_shift_finish(ShiftGridArgs a)
{
    const uint32_t cid = blockIdx.x * 256u + threadIdx.x;
    if (cid == 0 && a.round_err_out) *a.round_err_out = *a.round_err;
    if (cid >= (uint32_t)a.n_frames * 16u) return;
    const ShiftCellState st = a.state[cid];
    const bool done = st.active && st.count;
    const double n = (double)st.count;
    a.shift[2u * (size_t)cid] = done ? (double)(-st.sum_dy) / n : 0.0;
    a.shift[2u * (size_t)cid + 1u] = done ? (double)(-st.sum_dx) / n : 0.0;
    a.status[cid] = done ? 1 : 0;
}

// ---- mdvt_flow_warp ------------------------------------------------------------------------------------------------------------------

// a thread per output pixel, a frame per blockIdx.y: the flow at the pixel through cv2.resize(INTER_LINEAR)'s tables on float32
// (depth_code::tap; horizontal pass, then vertical), map = fl32(x - flow), then cv2.remap's fixed-point bilinear -- k_equirect_remap's
// arithmetic (mdvt_formats.hip) with the four taps' coordinates clamped to the image where that kernel reads black
__global__ void __launch_bounds__(256) k_flow_warp(FlowWarpArgs a)
{
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    if (t >= (uint32_t)a.W * (uint32_t)a.H) return;
    const int y = (int)(t / (uint32_t)a.W), x = (int)(t - (uint32_t)y * (uint32_t)a.W);
    const size_t f = (size_t)a.frame0 + blockIdx.y;
    const uint8_t* src = a.src + f * a.src_stride;
    uint8_t* out = a.dst + f * a.dst_stride + (size_t)y * a.dst_pitch + (size_t)x * 3u;
    if (!a.has_grid[f]) {
        const uint8_t* p = src + (size_t)y * a.src_pitch + (size_t)x * 3u;
        out[0] = p[0]; out[1] = p[1]; out[2] = p[2];
        return;
    }
    const float* g = a.grids + f * 32u;                             // [4][4][2]: dx, dy
    int s0, s1, y0, y1;
    float a0, a1, b0, b1;
    depth_code::tap(x, 4.0 / (double)a.W, 4, s0, s1, a0, a1);
    depth_code::tap(y, 4.0 / (double)a.H, 4, y0, y1, b0, b1);
    float flow[2];
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const float h0 = g[(y0 * 4 + s0) * 2 + k] * a0 + g[(y0 * 4 + s1) * 2 + k] * a1;
        const float h1 = g[(y1 * 4 + s0) * 2 + k] * a0 + g[(y1 * 4 + s1) * 2 + k] * a1;
        flow[k] = h0 * b0 + h1 * b1;
    }
    const float mx = (float)x - flow[0], my = (float)y - flow[1];
    // (a NaN or a flow beyond the int range converts to some int; the clamps below keep every tap inside the image)
    const int sx = (int)rintf(mx * 32.0f), sy = (int)rintf(my * 32.0f);
    const int ix = sx >> 5, iy = sy >> 5, fx = sx & 31, fy = sy & 31;
    const int w00 = (32 - fx) * (32 - fy) * 32, w10 = fx * (32 - fy) * 32, w01 = (32 - fx) * fy * 32, w11 = fx * fy * 32;
    const int xa = ix < 0 ? 0 : (ix > a.W - 1 ? a.W - 1 : ix), xb = ix + 1 < 0 ? 0 : (ix + 1 > a.W - 1 ? a.W - 1 : ix + 1);
    const int ya = iy < 0 ? 0 : (iy > a.H - 1 ? a.H - 1 : iy), yb = iy + 1 < 0 ? 0 : (iy + 1 > a.H - 1 ? a.H - 1 : iy + 1);
    const uint8_t* ra = src + (size_t)ya * a.src_pitch;
    const uint8_t* rb = src + (size_t)yb * a.src_pitch;
    const uint32_t p00 = load_px_bytes(ra, xa), p10 = load_px_bytes(ra, xb), p01 = load_px_bytes(rb, xa), p11 = load_px_bytes(rb, xb);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const int sh = 8 * c;
        const int acc = w00 * (int)((p00 >> sh) & 0xFF) + w10 * (int)((p10 >> sh) & 0xFF) + w01 * (int)((p01 >> sh) & 0xFF) + w11 * (int)((p11 >> sh) & 0xFF);
        out[c] = (uint8_t)((acc + (1 << 14)) >> 15);
    }
}

// ---- mdvt_inspatio_prepare_eye, mdvt_inspatio_model_frames -----------------------------------------------------------------------

// iwi:385-426 at the eye's size: V = 255 where the three mask bytes are 0, the render blacked where V = 0, the frame's holes.
// Grid (columns / 256, rows, frames).
__global__ void __launch_bounds__(256) k_insp_eye(InspatioPrepareArgs a)
{
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
    const size_t f = (size_t)a.frame0 + blockIdx.z;
    bool hole = false;
    if (x < a.rs.in_w) {
        const uint32_t m = load_px_bytes(a.mask.p + f * a.mask.stride + (size_t)y * a.mask.pitch, x);
        hole = m != 0u;
        const uint32_t c = hole ? 0u : load_px_bytes(a.color.p + f * a.color.stride + (size_t)y * a.color.pitch, x);
        a.valid[f * a.valid_stride + (size_t)y * a.valid_pitch + (size_t)x] = hole ? 0 : 255;
        store_px_bytes(a.render + f * a.render_stride + (size_t)y * a.render_pitch, x, c);
    }
    const unsigned long long b = __ballot(hole);
    if ((threadIdx.x & 63) == 0 && b) atomicAdd(a.holes + f, (uint32_t)__popcll(b));
}

// The model's images through THE U8 RESIZE (mdvt_adapter_resize.h): with a mask, the blacked render and the validity plane (resized
// as a one-channel image, not thresholded); without (a.mask.p null), the colour frames as they are.  Grid as above, over the model's size.
__global__ void __launch_bounds__(256) k_insp_model(InspatioPrepareArgs a)
{
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
    const size_t f = (size_t)a.frame0 + blockIdx.z;
    if (x >= a.rs.out_w) return;
    const uint8_t* color = a.color.p + f * a.color.stride;
    if (!a.mask.p) {
        const uint32_t c = adapter_resize_px(a.rs, x, y, [&](int sx, int sy) { return load_px_bytes(color + (size_t)sy * a.color.pitch, sx); });
        store_px_bytes(a.m_render + f * a.m_render_stride + (size_t)y * a.m_render_pitch, x, c);
        return;
    }
    const uint8_t* mask = a.mask.p + f * a.mask.stride;
    const uint32_t c = adapter_resize_px(a.rs, x, y, [&](int sx, int sy) {
        return load_px_bytes(mask + (size_t)sy * a.mask.pitch, sx) != 0u ? 0u : load_px_bytes(color + (size_t)sy * a.color.pitch, sx);
    });
    const uint32_t v = adapter_resize_px(a.rs, x, y, [&](int sx, int sy) {
        return load_px_bytes(mask + (size_t)sy * a.mask.pitch, sx) != 0u ? 0u : 255u;
    });
    store_px_bytes(a.m_render + f * a.m_render_stride + (size_t)y * a.m_render_pitch, x, c);
    a.m_valid[f * a.m_valid_stride + (size_t)y * a.m_valid_pitch + (size_t)x] = (uint8_t)(v & 0xFFu);
}

// ---- mdvt_inspatio_composite_eye -------------------------------------------------------------------------------------------------

// iwi:504-507: three 4-neighbour dilations of the lower-side marks, the border as background: a pixel is set where a mark lies within
// L1 distance 3.  marks: an image as mdvt_mark_lower_side writes it ((0, 0, 255) at a mark); grown: H rows of W bytes, 0 / 1.
__global__ void __launch_bounds__(256) k_insp_grow(const uint8_t* __restrict__ marks, size_t marks_pitch, uint8_t* __restrict__ grown, int W, int H)
{
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
    if (x >= W) return;
    uint8_t on = 0;
    for (int dy = -3; dy <= 3; ++dy) {
        const int yy = y + dy, r = 3 - (dy < 0 ? -dy : dy);
        if (yy < 0 || yy >= H) continue;
        for (int dx = -r; dx <= r; ++dx) {
            const int xx = x + dx;
            if (xx >= 0 && xx < W && marks[(size_t)yy * marks_pitch + 3u * (size_t)xx + 2u] == 255) on = 1;
        }
    }
    grown[(size_t)y * W + x] = on;
}

__device__ __forceinline__ int reflect101(int i, int n) { return i < 0 ? -i : (i >= n ? 2 * n - 2 - i : i); }

// iwi:485-516 for one frame of one eye: pasted = hole ? aligned : render; with a grown plane also blended = trunc(clip(fl(fl(alpha A)
// + fl(fl(1 - alpha) pasted)), 0, 255)), alpha = cv2.GaussianBlur(grown, (5, 5), 0) in float32 with BORDER_REFLECT_101: the fixed
// table 1 4 6 4 1 / 16 per axis.  On a 0 / 1 plane every product and sum is a multiple of 2^-8 below 2: exact, whatever the order.
__global__ void __launch_bounds__(256) k_insp_composite(InspatioCompositeArgs a)
{
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
    if (x >= a.W) return;
    const uint32_t m = load_px_bytes(a.mask + (size_t)y * a.mask_pitch, x);
    const uint32_t A = load_px_bytes(a.aligned + (size_t)y * a.aligned_pitch, x);
    const uint32_t p = m != 0u ? A : load_px_bytes(a.color + (size_t)y * a.color_pitch, x);
    store_px_bytes(a.pasted + (size_t)y * a.pasted_pitch, x, p);
    if (!a.blended) return;
    const float w[5] = {0.0625f, 0.25f, 0.375f, 0.25f, 0.0625f};
    float alpha = 0.0f;
#pragma unroll
    for (int j = 0; j < 5; ++j) {
        const uint8_t* row = a.grown + (size_t)reflect101(y + j - 2, a.H) * (size_t)a.W;
        float h = 0.0f;
#pragma unroll
        for (int i = 0; i < 5; ++i) h = h + w[i] * (float)row[reflect101(x + i - 2, a.W)];
        alpha = alpha + w[j] * h;
    }
    const float beta = 1.0f - alpha;
    uint32_t o = 0;
#pragma unroll
    for (int k = 0; k < 24; k += 8) {
        float v = alpha * (float)((A >> k) & 0xFFu) + beta * (float)((p >> k) & 0xFFu);
        v = v < 0.0f ? 0.0f : (v > 255.0f ? 255.0f : v);
        o |= (uint32_t)v << k;
    }
    store_px_bytes(a.blended + (size_t)y * a.blended_pitch, x, o);
}

size_t fft_lds(int nl, int L) { return ((size_t)nl * (size_t)L + (size_t)L / 2u) * sizeof(double2); }

}  // namespace

hipError_t launch_shift_gate(const ShiftGridArgs& a, hipStream_t s)
{
    hipLaunchKernelGGL(k_shift_gate, dim3((unsigned)a.n_frames * 16u), dim3(256), 0, s, a);
    if (hipError_t e = hipGetLastError()) return e;
    hipLaunchKernelGGL(k_shift_border, dim3((unsigned)a.n_frames * 8u), dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_shift_units(const ShiftGridArgs& a, hipStream_t s)
{
    const unsigned units = (unsigned)a.n_units, cells = ((unsigned)(a.Ly * a.Lx) + 255u) / 256u;
    if (!a.transform) {
        hipLaunchKernelGGL(k_shift_direct, dim3(cells, 1, units), dim3(256), 0, s, a);
    } else {
        const int nl = shift_fft_lines(a.Ly);
        hipLaunchKernelGGL(k_shift_rows_fwd, dim3((unsigned)a.hmax, 3, units), dim3(256), fft_lds(1, a.Lx), s, a);
        if (hipError_t e = hipGetLastError()) return e;
        hipLaunchKernelGGL(k_shift_cols, dim3((unsigned)(a.Lx / nl), 3, units), dim3(256), fft_lds(nl, a.Ly), s, a, nl, 0);
        if (hipError_t e = hipGetLastError()) return e;
        hipLaunchKernelGGL(k_shift_product, dim3(cells, 1, units), dim3(256), 0, s, a);
        if (hipError_t e = hipGetLastError()) return e;
        hipLaunchKernelGGL(k_shift_cols, dim3((unsigned)(a.Lx / nl), 3, units), dim3(256), fft_lds(nl, a.Ly), s, a, nl, 1);
        if (hipError_t e = hipGetLastError()) return e;
        hipLaunchKernelGGL(k_shift_rows_inv, dim3((unsigned)a.Ly, 3, units), dim3(256), fft_lds(1, a.Lx), s, a);
    }
    if (hipError_t e = hipGetLastError()) return e;
    hipLaunchKernelGGL(k_shift_peak<1>, dim3(cells, 1, units), dim3(256), 0, s, a);
    if (hipError_t e = hipGetLastError()) return e;
    hipLaunchKernelGGL(k_shift_peak<2>, dim3(cells, 1, units), dim3(256), 0, s, a);
    if (hipError_t e = hipGetLastError()) return e;
    hipLaunchKernelGGL(k_shift_peak<3>, dim3(cells, 1, units), dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_shift_finish(const ShiftGridArgs& a, hipStream_t s)
{
    hipLaunchKernelGGL(k_shift_finish, dim3(((unsigned)a.n_frames * 16u + 255u) / 256u), dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_inspatio_prepare(const InspatioPrepareArgs& a, int n_frames, hipStream_t s)
{
    if (a.mask.p) {
        hipLaunchKernelGGL(k_insp_eye, dim3((unsigned)(a.rs.in_w + 255) / 256u, (unsigned)a.rs.in_h, (unsigned)n_frames), dim3(256), 0, s, a);
        if (hipError_t e = hipGetLastError()) return e;
    }
    hipLaunchKernelGGL(k_insp_model, dim3((unsigned)(a.rs.out_w + 255) / 256u, (unsigned)a.rs.out_h, (unsigned)n_frames), dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_inspatio_grow(const uint8_t* marks, size_t marks_pitch, uint8_t* grown, int W, int H, hipStream_t s)
{
    hipLaunchKernelGGL(k_insp_grow, dim3((unsigned)(W + 255) / 256u, (unsigned)H), dim3(256), 0, s, marks, marks_pitch, grown, W, H);
    return hipGetLastError();
}

hipError_t launch_inspatio_composite(const InspatioCompositeArgs& a, hipStream_t s)
{
    hipLaunchKernelGGL(k_insp_composite, dim3((unsigned)(a.W + 255) / 256u, (unsigned)a.H), dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_flow_warp(const FlowWarpArgs& a, int n_frames, hipStream_t s)
{
    const dim3 grid(((unsigned)a.W * (unsigned)a.H + 255u) / 256u, (unsigned)n_frames);
    hipLaunchKernelGGL(k_flow_warp, grid, dim3(256), 0, s, a);
    return hipGetLastError();
}

}  // namespace mdvt
