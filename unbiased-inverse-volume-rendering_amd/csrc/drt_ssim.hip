// drt_ssim.hip -- structural similarity of two films x, y (N,H,W,C), float32, channels last; the definition stands in include/drt_hip.h
// ("SSIM"), DESIGN.md "SSIM and D-SSIM" has the measurements.
// Shape: a film row is WC = W C contiguous floats and a horizontal tap a stride of C floats, so one kernel serves every C with coalesced
// loads.  A workgroup of kPT threads owns a tile of kTY rows x kTW floats of one image.
//   forward   loads the tile of x and y with a halo of 5 rows and 5 C floats (zeros outside the film) into LDS; the horizontal pass writes
//             the five windowed sums of x, y, xx, yy, xy of the kTY + 10 rows to LDS; the vertical pass runs one column per lane, kRows rows
//             per thread, each moment row read once and added to the outputs it belongs to in ascending tap order.  Every sum is
//             acc = acc + g[i] * v with both operations rounded, and xy takes the operations of xx and yy in their order: where x and y hold
//             the same bits numerator and denominator of S are the same float and S is 1.0f.
//             Per entry it stores S (optional) and the three derivative maps (optional), and the tile's sum of S over the entries that count
//             goes as one double to partials[tile]; ssim_finish_kernel, ONE workgroup, adds them in a fixed order: no float atomics.
//   backward  the same two passes over the three derivative maps, masked to the entries that count (the window is symmetric: the transpose
//             of the stencil is the stencil), then grad = scale (a + 2 x b + y c): a gather, no atomics, the same bits on every call.
// LDS: forward (2 (kTY + 10) kEW + 5 (kTY + 10) kTW) floats = 63232 bytes, backward (3 ... + 3 ...) = 64896 bytes: two workgroups per CU.
#include "drt_launch.h"
#include <cmath>

namespace drt {

namespace {

constexpr int kPT = 256;                        // threads per workgroup
constexpr int kTY = 16, kTW = 64;               // tile: rows x floats of a row
constexpr int kR = 5;                           // window radius (11 taps)
constexpr int kHalo = kR * kSsimMaxChannels;    // LDS halo columns on each side
constexpr int kEW = kTW + 2 * kHalo;            // input rows: columns [w0 - kHalo, w0 + kTW + kHalo)
constexpr int kER = kTY + 2 * kR;               // rows [y0 - 5, y0 + kTY + 5)
constexpr int kRows = kTY * kTW / kPT;          // output rows per thread of the vertical pass
constexpr int kSpan = kRows + 2 * kR;           // moment rows such a thread reads
constexpr int kFill = (kER * kEW + kPT - 1) / kPT;   // input entries a thread loads
constexpr size_t kFwdLds = (size_t) (2 * kER * kEW + 5 * kER * kTW) * sizeof(float);
constexpr size_t kBwdLds = (size_t) (3 * kER * kEW + 3 * kER * kTW) * sizeof(float);

static_assert(kPT % kTW == 0 && kRows * kPT == kTY * kTW && kPT * sizeof(double) <= kFwdLds, "tile geometry");
static_assert(kFwdLds <= 64 * 1024 && kBwdLds <= 64 * 1024, "two workgroups per CU, and no more dynamic LDS than a kernel gets without asking");

struct SsimArgs {
    const float *x, *y;
    float *map, *dmaps;          // forward outputs (either may be null); backward: dmaps is read
    const float *upstream;       // backward
    float *grad;                 // backward
    double *partials;
    size_t plane;                // N H W C: the floats of one derivative map
    int H, C, WC;                // WC = W C floats per row
    uint32_t tiles_w, tiles_y;
    int valid;
    float c1, c2, inv_count;
    float g[2 * kR + 1];
};

// does entry (row, f) take part in the mean?
__device__ inline bool ssim_counts(const SsimArgs &A, int row, int f)
{
    if (row >= A.H || f >= A.WC) return false;
    if (!A.valid) return true;
    return row >= kR && row < A.H - kR && f >= kR * A.C && f < A.WC - kR * A.C;
}

__global__ void __launch_bounds__(kPT) ssim_forward_kernel(SsimArgs A)
{
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float *X = lds, *Y = lds + kER * kEW, *M = lds + 2 * kER * kEW;       // M[k][row][col], k = x, y, xx, yy, xy
    const int t = (int) threadIdx.x;
    uint32_t b = blockIdx.x;
    const uint32_t tw = b % A.tiles_w; b /= A.tiles_w;
    const uint32_t ty = b % A.tiles_y, img = b / A.tiles_y;
    const int y0 = (int) ty * kTY, w0 = (int) tw * kTW;
    const int C = A.C, WC = A.WC, H = A.H;
    const size_t base = (size_t) img * (size_t) H * (size_t) WC;

    // every load of the thread is issued before the first LDS store waits for one
    float xv[kFill], yv[kFill];
#pragma unroll
    for (int i = 0; i < kFill; ++i) {
        const int idx = t + i * kPT, ly = idx / kEW, j = idx - ly * kEW;
        const int row = y0 - kR + ly, f = w0 - kHalo + j;
        xv[i] = 0.0f; yv[i] = 0.0f;
        if (idx < kER * kEW && j >= kHalo - kR * C && j < kHalo + kTW + kR * C && row >= 0 && row < H && f >= 0 && f < WC) {
            const size_t off = base + (size_t) row * (size_t) WC + (size_t) f;
            xv[i] = A.x[off]; yv[i] = A.y[off];
        }
    }
#pragma unroll
    for (int i = 0; i < kFill; ++i) {
        const int idx = t + i * kPT;
        if (idx < kER * kEW) { X[idx] = xv[i]; Y[idx] = yv[i]; }
    }
    __syncthreads();

    for (int idx = t; idx < kER * kTW; idx += kPT) {
        const int ly = idx / kTW, j = idx - ly * kTW;
        const float *xr = X + ly * kEW + kHalo + j - kR * C, *yr = Y + ly * kEW + kHalo + j - kR * C;
        float sx = 0.0f, sy = 0.0f, sxx = 0.0f, syy = 0.0f, sxy = 0.0f;
#pragma unroll
        for (int i = 0; i <= 2 * kR; ++i) {
            const float xv = xr[i * C], yv = yr[i * C], gi = A.g[i];
            sx = sx + gi * xv; sy = sy + gi * yv;
            sxx = sxx + gi * (xv * xv); syy = syy + gi * (yv * yv); sxy = sxy + gi * (xv * yv);
        }
        M[idx] = sx; M[kER * kTW + idx] = sy; M[2 * kER * kTW + idx] = sxx; M[3 * kER * kTW + idx] = syy; M[4 * kER * kTW + idx] = sxy;
    }
    __syncthreads();

    const int j = t % kTW, r0 = (t / kTW) * kRows;
    float acc[kRows][5];
#pragma unroll
    for (int o = 0; o < kRows; ++o)
#pragma unroll
        for (int k = 0; k < 5; ++k) acc[o][k] = 0.0f;
#pragma unroll
    for (int r = 0; r < kSpan; ++r) {
        float v[5];
#pragma unroll
        for (int k = 0; k < 5; ++k) v[k] = M[k * kER * kTW + (r0 + r) * kTW + j];
#pragma unroll
        for (int o = 0; o < kRows; ++o) {
            const int i = r - o;
            if (i >= 0 && i <= 2 * kR) {
#pragma unroll
                for (int k = 0; k < 5; ++k) acc[o][k] = acc[o][k] + A.g[i] * v[k];
            }
        }
    }

    double sum = 0.0;
    const int f = w0 + j;
    const size_t plane = A.plane;
#pragma unroll
    for (int o = 0; o < kRows; ++o) {
        const int row = y0 + r0 + o;
        if (row >= H || f >= WC) continue;
        const float mx = acc[o][0], my = acc[o][1];
        const float mxx = mx * mx, myy = my * my, mxy = mx * my;
        const float vx = acc[o][2] - mxx, vy = acc[o][3] - myy, vxy = acc[o][4] - mxy;
        const float a1 = 2.0f * mxy + A.c1, a2 = 2.0f * vxy + A.c2;
        const float b1 = (mxx + myy) + A.c1, b2 = (vx + vy) + A.c2;
        const float den = b1 * b2;
        const float s = (a1 * a2) / den;
        const size_t off = base + (size_t) row * (size_t) WC + (size_t) f;
        if (A.map) A.map[off] = s;
        if (A.dmaps) {
            // total derivatives of S: Exy and Exx enter through the covariances alone; mu_x directly and through -mu_x mu_y and -mu_x^2
            const float d_exy = (2.0f * a1) / den;
            const float d_exx = -(s / b2);
            const float d_mu = ((2.0f * my) * a2) / den - ((2.0f * mx) * s) / b1 - my * d_exy - (2.0f * mx) * d_exx;
            A.dmaps[off] = d_mu; A.dmaps[plane + off] = d_exx; A.dmaps[2 * plane + off] = d_exy;
        }
        if (ssim_counts(A, row, f)) sum += (double) s;
    }

    __syncthreads();                                 // the moments are read: LDS becomes the reduction's
    double *red = reinterpret_cast<double *>(lds);
    red[t] = sum;
    for (int s = kPT / 2; s > 0; s >>= 1) {
        __syncthreads();
        if (t < s) red[t] += red[t + s];
    }
    if (t == 0) A.partials[blockIdx.x] = red[0];
}

// one workgroup: thread i sums partials i, i + 256, ... in order, then the fixed tree
__global__ void __launch_bounds__(256) ssim_finish_kernel(const double *partials, uint64_t n_partials, double count, double *value)
{
    __shared__ double red[256];
    double s = 0.0;
    for (uint64_t i = threadIdx.x; i < n_partials; i += 256) s += partials[i];
    red[threadIdx.x] = s;
    for (int w = 128; w > 0; w >>= 1) {
        __syncthreads();
        if ((int) threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
    }
    if (threadIdx.x == 0) value[0] = red[0] / count;
}

__global__ void __launch_bounds__(kPT) ssim_backward_kernel(SsimArgs A)
{
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float *D = lds, *M = lds + 3 * kER * kEW;         // D[k][row][col] the masked derivative maps, M[k][row][col] their horizontal sums
    const int t = (int) threadIdx.x;
    uint32_t b = blockIdx.x;
    const uint32_t tw = b % A.tiles_w; b /= A.tiles_w;
    const uint32_t ty = b % A.tiles_y, img = b / A.tiles_y;
    const int y0 = (int) ty * kTY, w0 = (int) tw * kTW;
    const int C = A.C, WC = A.WC, H = A.H;
    const size_t base = (size_t) img * (size_t) H * (size_t) WC;
    const size_t plane = A.plane;

    float d0[kFill], d1[kFill], d2[kFill];           // (all loads in flight before the first LDS store, as in the forward kernel)
#pragma unroll
    for (int i = 0; i < kFill; ++i) {
        const int idx = t + i * kPT, ly = idx / kEW, j = idx - ly * kEW;
        const int row = y0 - kR + ly, f = w0 - kHalo + j;
        d0[i] = 0.0f; d1[i] = 0.0f; d2[i] = 0.0f;
        if (idx < kER * kEW && j >= kHalo - kR * C && j < kHalo + kTW + kR * C && row >= 0 && f >= 0 && ssim_counts(A, row, f)) {
            const size_t off = base + (size_t) row * (size_t) WC + (size_t) f;
            d0[i] = A.dmaps[off]; d1[i] = A.dmaps[plane + off]; d2[i] = A.dmaps[2 * plane + off];
        }
    }
#pragma unroll
    for (int i = 0; i < kFill; ++i) {
        const int idx = t + i * kPT;
        if (idx < kER * kEW) { D[idx] = d0[i]; D[kER * kEW + idx] = d1[i]; D[2 * kER * kEW + idx] = d2[i]; }
    }
    __syncthreads();

    for (int idx = t; idx < kER * kTW; idx += kPT) {
        const int ly = idx / kTW, j = idx - ly * kTW;
        const float *dr = D + ly * kEW + kHalo + j - kR * C;
        float s0 = 0.0f, s1 = 0.0f, s2 = 0.0f;
#pragma unroll
        for (int i = 0; i <= 2 * kR; ++i) {
            const float gi = A.g[i];
            s0 = s0 + gi * dr[i * C]; s1 = s1 + gi * dr[kER * kEW + i * C]; s2 = s2 + gi * dr[2 * kER * kEW + i * C];
        }
        M[idx] = s0; M[kER * kTW + idx] = s1; M[2 * kER * kTW + idx] = s2;
    }
    __syncthreads();

    const int j = t % kTW, r0 = (t / kTW) * kRows;
    const int f = w0 + j;
    float xc[kRows], yc[kRows];                      // the images at this thread's outputs, in flight during the vertical pass
#pragma unroll
    for (int o = 0; o < kRows; ++o) {
        const int row = y0 + r0 + o;
        xc[o] = 0.0f; yc[o] = 0.0f;
        if (row < H && f < WC) {
            const size_t off = base + (size_t) row * (size_t) WC + (size_t) f;
            xc[o] = A.x[off]; yc[o] = A.y[off];
        }
    }
    float acc[kRows][3];
#pragma unroll
    for (int o = 0; o < kRows; ++o)
#pragma unroll
        for (int k = 0; k < 3; ++k) acc[o][k] = 0.0f;
#pragma unroll
    for (int r = 0; r < kSpan; ++r) {
        float v[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) v[k] = M[k * kER * kTW + (r0 + r) * kTW + j];
#pragma unroll
        for (int o = 0; o < kRows; ++o) {
            const int i = r - o;
            if (i >= 0 && i <= 2 * kR) {
#pragma unroll
                for (int k = 0; k < 3; ++k) acc[o][k] = acc[o][k] + A.g[i] * v[k];
            }
        }
    }

    const float scale = A.upstream[0] * A.inv_count;
#pragma unroll
    for (int o = 0; o < kRows; ++o) {
        const int row = y0 + r0 + o;
        if (row >= H || f >= WC) continue;
        const size_t off = base + (size_t) row * (size_t) WC + (size_t) f;
        A.grad[off] = scale * ((acc[o][0] + (2.0f * xc[o]) * acc[o][1]) + yc[o] * acc[o][2]);
    }
}

struct SsimPlan {
    uint32_t tiles_w, tiles_y;
    uint64_t wgs;
};

SsimPlan ssim_plan(int n, int h, int w, int c)
{
    SsimPlan L;
    const int64_t wc = (int64_t) w * c;
    L.tiles_w = (uint32_t) ((wc + kTW - 1) / kTW);
    L.tiles_y = (uint32_t) ((h + kTY - 1) / kTY);
    L.wgs = (uint64_t) L.tiles_w * L.tiles_y * (uint64_t) n;
    return L;
}

SsimArgs ssim_args(const SsimPlan &L, const float *x, const float *y, int n, int h, int w, int c, double data_range, bool valid)
{
    SsimArgs A = {};
    A.x = x; A.y = y;
    A.plane = (size_t) n * (size_t) h * (size_t) w * (size_t) c;
    A.H = h; A.C = c; A.WC = w * c;
    A.tiles_w = L.tiles_w; A.tiles_y = L.tiles_y;
    A.valid = valid ? 1 : 0;
    A.c1 = (float) ((0.01 * data_range) * (0.01 * data_range));
    A.c2 = (float) ((0.03 * data_range) * (0.03 * data_range));
    A.inv_count = (float) (1.0 / ssim_count(n, h, w, c, valid));
    ssim_window(A.g);
    return A;
}

template <typename K> hipError_t ssim_launch(K kernel, size_t lds_bytes, const SsimArgs &A, uint64_t wgs, hipStream_t stream)
{
    hipLaunchKernelGGL(kernel, dim3((unsigned) wgs), dim3(kPT), lds_bytes, stream, A);
    return hipGetLastError();
}

}  // namespace

void ssim_window(float g[11])
{
    double e[2 * kR + 1], sum = 0.0;
    for (int i = 0; i <= 2 * kR; ++i) {
        e[i] = std::exp(-(double) ((i - kR) * (i - kR)) / (2.0 * 1.5 * 1.5));
        sum += e[i];
    }
    for (int i = 0; i <= 2 * kR; ++i) g[i] = (float) (e[i] / sum);
}

double ssim_count(int n, int h, int w, int c, bool valid)
{
    return valid ? (double) n * (double) (h - 2 * kR) * (double) (w - 2 * kR) * (double) c : (double) n * (double) h * (double) w * (double) c;
}

bool ssim_supported(int64_t n, int64_t h, int64_t w, int64_t c)
{
    if (n < 1 || h < 1 || w < 1 || c < 1 || c > kSsimMaxChannels) return false;
    if (n >= (1ll << 31) || h >= (1ll << 31) || w >= (1ll << 31)) return false;
    const double entries = (double) n * (double) h * (double) w * (double) c;
    return entries < 2147483648.0;
}

uint64_t ssim_partials(int n, int h, int w, int c)
{
    return ssim_supported(n, h, w, c) ? ssim_plan(n, h, w, c).wgs : 0;
}

hipError_t launch_ssim_forward(const float *x, const float *y, int n, int h, int w, int c, double data_range, bool valid, double *value,
                               float *map, float *dmaps, double *partials, hipStream_t stream)
{
    if (!ssim_supported(n, h, w, c) || (valid && (h < 2 * kR + 1 || w < 2 * kR + 1))) return hipErrorInvalidValue;
    const SsimPlan L = ssim_plan(n, h, w, c);
    SsimArgs A = ssim_args(L, x, y, n, h, w, c, data_range, valid);
    A.map = map; A.dmaps = dmaps; A.partials = partials;
    const hipError_t e = ssim_launch(ssim_forward_kernel, kFwdLds, A, L.wgs, stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(ssim_finish_kernel, dim3(1), dim3(256), 0, stream, (const double *) partials, L.wgs, ssim_count(n, h, w, c, valid), value);
    return hipGetLastError();
}

hipError_t launch_ssim_backward(const float *x, const float *y, const float *dmaps, const float *upstream, int n, int h, int w, int c, bool valid,
                                float *grad, hipStream_t stream)
{
    if (!ssim_supported(n, h, w, c) || (valid && (h < 2 * kR + 1 || w < 2 * kR + 1))) return hipErrorInvalidValue;
    const SsimPlan L = ssim_plan(n, h, w, c);
    SsimArgs A = ssim_args(L, x, y, n, h, w, c, 1.0, valid);
    A.dmaps = const_cast<float *>(dmaps); A.upstream = upstream; A.grad = grad;
    return ssim_launch(ssim_backward_kernel, kBwdLds, A, L.wgs, stream);
}

}  // namespace drt
