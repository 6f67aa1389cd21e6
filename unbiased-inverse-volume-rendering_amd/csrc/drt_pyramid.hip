// drt_pyramid.hip -- multi-scale (box pyramid) residual losses of two films x, y (N,H,W,C), float32, channels last; the definition stands in
// include/drt_hip.h ("Pyramid losses"), DESIGN.md "Multi-scale pyramid losses" has the measurements.
// Shape: a workgroup of kPT threads owns a tile of 32 x 32 pixels of one film.  Tiles start at multiples of 2^5, so every cell of every
// level 0..5 lies in exactly one tile and no level map ever goes to HBM.
//   load      the tile's residual r_0 = x - y (0 outside the film) goes to LDS, pixel-major with the channels innermost as in the film: a
//             tile row is 32 C contiguous floats of a film row, loaded with 16-byte accesses where the pointers and W C allow (kVec), with
//             4-byte ones otherwise; every load of a thread is issued before its first LDS store.
//   reduce    level l = 1..L from level l - 1, one barrier each: a cell adds its four children in the order (2i,2j), (2i,2j+1), (2i+1,2j),
//             (2i+1,2j+1) - the missing ones hold 0 - and multiplies by 1, 0.5 or 0.25.  A cell that does not exist stores 0.
//   sums      every thread adds rho(r) of the cells it produced, per level, as doubles; a fixed wave shuffle tree, then the four waves in
//             order, give partials[tile][level].  pyramid_finish_kernel, ONE workgroup, adds the tiles in a fixed order: no float atomics.
//   gradient  comes down the levels in LDS, one barrier each: a cell of level l replaces its residual by a_l = (weight_l / N_l) rho'(r_l) +
//             a_{l+1}[parent] / count(parent), the division an exact power of two, a term of weight 0 not added; a_0 is the gradient,
//             stored with the load's access width.  (A first version let every entry walk its five ancestors: 2.7 x the time of the
//             value alone on 63 x 512^2 x 3; DESIGN.md.)
// LDS: 1365 C floats (1024 + 256 + 64 + 16 + 4 + 1 cells per channel) + 24 doubles: 5.6 KB at C = 1, 43.9 KB at C = 8, static.
// Banks: the level-0 stores and the gradient's own-level accesses are contiguous per wave, its parent reads shared by neighbouring cells.
// The child reads of the reduce step have a stride of 2 C floats between neighbouring cells, which folds the 32 lanes of a ds_read_b32
// group onto half the banks: 2-way, on the reads of 1365 C of the words (computed from the bank rule, not measured).  A channel-planar
// layout would take that away and pay it back 2- to 8-fold on the level-0 stores (stride C), so the film's layout is kept.
#include "drt_launch.h"
#include <cmath>

namespace drt {

namespace {

constexpr int kPT = 256;                         // threads per workgroup
constexpr int kTile = 32;                        // pixels per tile side = 2^kPyramidMaxLevels
constexpr int kCells = 1365;                     // cells of all six levels of a tile, per channel
constexpr int kLv = kPyramidMaxLevels + 1;
constexpr int kWaves = kPT / 64;
constexpr int kFinish = 1024;                     // threads of the single workgroup that adds the tiles' sums

static_assert(kTile == (1 << kPyramidMaxLevels) && kCells == 1024 + 256 + 64 + 16 + 4 + 1, "tile geometry");

struct PyramidArgs {
    const float *x, *y;
    float *grad;                 // may be null
    double *partials;            // [tiles][levels + 1]
    int H, W;
    uint32_t tiles_x, tiles_y;
    int levels, kind;
    float delta, half_delta;     // huber
    float coef[kLv];             // float(weight_l / N_l); 0: the level is not added
};

// first cell of level l in the tile's LDS image, in cells per channel
__device__ __forceinline__ constexpr int level_offset(int l)
{
    return l == 0 ? 0 : l == 1 ? 1024 : l == 2 ? 1280 : l == 3 ? 1344 : l == 4 ? 1360 : 1364;
}

__device__ __forceinline__ float rho(int kind, float r, float delta, float half_delta)
{
    if (kind == kPyramidL1) return fabsf(r);
    if (kind == kPyramidL2) return r * r;
    return r < delta ? 0.5f * (r * r) : delta * fabsf(r) - half_delta;
}

__device__ __forceinline__ float rho_prime(int kind, float r, float delta)
{
    const float sign = r > 0.0f ? 1.0f : (r < 0.0f ? -1.0f : 0.0f);
    if (kind == kPyramidL1) return sign;
    if (kind == kPyramidL2) return 2.0f * r;
    return r < delta ? r : delta * sign;
}

// extent of level l of a film side
__device__ __forceinline__ int level_extent(int n, int l)
{
    return (n + (1 << l) - 1) >> l;
}

// the wave's sum of `s` by a fixed shuffle tree (every lane takes part), left in out[wave]
__device__ __forceinline__ void wave_sum(double s, double *out, int t)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_down(s, o, 64);
    if ((t & 63) == 0) out[t >> 6] = s;
}

template <int C, bool kVec>
__global__ void __launch_bounds__(kPT) pyramid_kernel(PyramidArgs A)
{
    __shared__ __attribute__((aligned(16))) float R[kCells * C];
    __shared__ double red[kLv][kWaves];
    constexpr int kRow = kTile * C;                       // floats of a tile row
    constexpr int kWidth = kVec ? 4 : 1;                  // floats per access
    constexpr int kPer = kTile * kRow / (kPT * kWidth);   // accesses per thread: C (16-byte) or 4 C (4-byte)
    const int t = (int) threadIdx.x;
    uint32_t b = blockIdx.x;
    const uint32_t tx = b % A.tiles_x; b /= A.tiles_x;
    const uint32_t ty = b % A.tiles_y, img = b / A.tiles_y;
    const int y0 = (int) ty * kTile, x0 = (int) tx * kTile;
    const int H = A.H, W = A.W, WC = W * C;
    const size_t base = (size_t) img * (size_t) H * (size_t) WC;
    const int kind = A.kind;
    const float delta = A.delta, half_delta = A.half_delta;

    double sum = 0.0;

    // level 0: access i of thread t covers floats [idx * kWidth, idx * kWidth + kWidth) of the tile image, idx = t + i kPT
    float xv[kPer][kWidth], yv[kPer][kWidth];
#pragma unroll
    for (int i = 0; i < kPer; ++i) {
        const int e = (t + i * kPT) * kWidth, row = e / kRow, col = e - row * kRow;
        const int gy = y0 + row, f = x0 * C + col;
#pragma unroll
        for (int k = 0; k < kWidth; ++k) { xv[i][k] = 0.0f; yv[i][k] = 0.0f; }
        if (gy < H && f < WC) {                           // (kVec: W C is a multiple of 4, so are f and the tile's origin: all four or none)
            const size_t off = base + (size_t) gy * (size_t) WC + (size_t) f;
            if constexpr (kVec) {
                const float4 a = *reinterpret_cast<const float4 *>(A.x + off), c = *reinterpret_cast<const float4 *>(A.y + off);
                xv[i][0] = a.x; xv[i][1] = a.y; xv[i][2] = a.z; xv[i][3] = a.w;
                yv[i][0] = c.x; yv[i][1] = c.y; yv[i][2] = c.z; yv[i][3] = c.w;
            } else {
                xv[i][0] = A.x[off]; yv[i][0] = A.y[off];
            }
        }
    }
#pragma unroll
    for (int i = 0; i < kPer; ++i) {
        const int e = (t + i * kPT) * kWidth, row = e / kRow, col = e - row * kRow;
        const bool inside = y0 + row < H && x0 * C + col < WC;
        float r[kWidth];
#pragma unroll
        for (int k = 0; k < kWidth; ++k) {
            r[k] = xv[i][k] - yv[i][k];
            if (inside) sum += (double) rho(kind, r[k], delta, half_delta);
        }
        if constexpr (kVec) *reinterpret_cast<float4 *>(R + e) = make_float4(r[0], r[1], r[2], r[3]);
        else R[e] = r[0];
    }
    wave_sum(sum, red[0], t);

    // levels 1..L, each from the level below
    for (int l = 1; l <= A.levels; ++l) {
        __syncthreads();
        const int side = kTile >> l, below = side * 2;
        const int he = level_extent(H, l), we = level_extent(W, l), hb = level_extent(H, l - 1), wb = level_extent(W, l - 1);
        const float *src = R + level_offset(l - 1) * C;
        float *dst = R + level_offset(l) * C;
        sum = 0.0;
        for (int idx = t; idx < side * side * C; idx += kPT) {
            const int cell = idx / C, ch = idx - cell * C, i = cell / side, j = cell - i * side;
            const int cy = (y0 >> l) + i, cx = (x0 >> l) + j;
            float r = 0.0f;
            if (cy < he && cx < we) {
                const float *p = src + ((2 * i) * below + 2 * j) * C + ch;
                const float kids = ((p[0] + p[C]) + p[below * C]) + p[below * C + C];
                const float inv = (2 * cy + 1 < hb ? 0.5f : 1.0f) * (2 * cx + 1 < wb ? 0.5f : 1.0f);
                r = kids * inv;
                sum += (double) rho(kind, r, delta, half_delta);
            }
            dst[idx] = r;
        }
        wave_sum(sum, red[l], t);
    }

    // the tile's sums: the waves in order
    __syncthreads();                                      // (also: the last level is written before the gradient reads it)
    if (t <= A.levels) {
        double s = red[t][0];
#pragma unroll
        for (int w = 1; w < kWaves; ++w) s += red[t][w];
        A.partials[(size_t) blockIdx.x * (size_t) (A.levels + 1) + (size_t) t] = s;
    }

    if (!A.grad) return;                                  // (uniform: no barrier is skipped by a part of the workgroup)

    // the gradient comes down: a cell of level l replaces its residual by a_l = coef_l rho'(r_l) + a_{l+1}[parent] / count(parent)
    for (int l = A.levels; l >= 1; --l) {
        const int side = kTile >> l;
        const int hb = level_extent(H, l), wb = level_extent(W, l);          // the extents the parent's children are counted in
        float *lev = R + level_offset(l) * C;
        const float *up = R + level_offset(l + 1) * C;                       // (read only where l < levels)
        const float k = A.coef[l];
        for (int idx = t; idx < side * side * C; idx += kPT) {
            const int cell = idx / C, ch = idx - cell * C, i = cell / side, j = cell - i * side;
            float a = 0.0f;
            if (k != 0.0f) a = k * rho_prime(kind, lev[idx], delta);
            if (l < A.levels) {
                const int pi = i >> 1, pj = j >> 1;
                const int cy = (y0 >> (l + 1)) + pi, cx = (x0 >> (l + 1)) + pj;
                const float inv = (2 * cy + 1 < hb ? 0.5f : 1.0f) * (2 * cx + 1 < wb ? 0.5f : 1.0f);
                a = a + up[(pi * (side >> 1) + pj) * C + ch] * inv;
            }
            lev[idx] = a;
        }
        __syncthreads();
    }
    const float k0 = A.coef[0];
#pragma unroll
    for (int i = 0; i < kPer; ++i) {
        const int e = (t + i * kPT) * kWidth, row = e / kRow, col = e - row * kRow;
        const int gy = y0 + row, f = x0 * C + col;
        if (gy >= H || f >= WC) continue;
        float g[kWidth];
#pragma unroll
        for (int q = 0; q < kWidth; ++q) {
            const int px = (col + q) / C, ch = (col + q) - px * C;
            float a = 0.0f;
            if (k0 != 0.0f) a = k0 * rho_prime(kind, R[e + q], delta);
            if (A.levels >= 1) {
                const int cy = gy >> 1, cx = (x0 + px) >> 1;
                const float inv = (2 * cy + 1 < H ? 0.5f : 1.0f) * (2 * cx + 1 < W ? 0.5f : 1.0f);
                a = a + R[(level_offset(1) + (row >> 1) * (kTile / 2) + (px >> 1)) * C + ch] * inv;
            }
            g[q] = a;
        }
        const size_t off = base + (size_t) gy * (size_t) WC + (size_t) f;
        if constexpr (kVec) *reinterpret_cast<float4 *>(A.grad + off) = make_float4(g[0], g[1], g[2], g[3]);
        else A.grad[off] = g[0];
    }
}

struct PyramidFinishArgs {
    const double *partials;
    uint64_t tiles;
    int levels;
    double count[kLv], weight[kLv];
    double *values;              // [levels + 2]: the level losses, then the total
};

// one workgroup of kFinish threads: thread i sums tiles i, i + kFinish, ... in order, all levels in one pass (the loads of the levels
// are independent of each other); then the fixed shuffle tree per wave and the waves in order; thread 0 adds the weighted levels in order
__global__ void __launch_bounds__(kFinish) pyramid_finish_kernel(PyramidFinishArgs F)
{
    __shared__ double red[kLv][kFinish / 64];
    const int t = (int) threadIdx.x, stride = F.levels + 1;
    double s[kLv];
#pragma unroll
    for (int l = 0; l < kLv; ++l) s[l] = 0.0;
    for (uint64_t i = (uint64_t) t; i < F.tiles; i += kFinish) {
        const double *p = F.partials + i * (uint64_t) stride;
#pragma unroll
        for (int l = 0; l < kLv; ++l)
            if (l <= F.levels) s[l] += p[l];
    }
#pragma unroll
    for (int l = 0; l < kLv; ++l) wave_sum(s[l], red[l], t);
    __syncthreads();
    if (t == 0) {
        double total = 0.0;
        for (int l = 0; l <= F.levels; ++l) {
            double v = red[l][0];
            for (int w = 1; w < kFinish / 64; ++w) v += red[l][w];
            v = v / F.count[l];
            F.values[l] = v;
            if (F.weight[l] != 0.0) total += F.weight[l] * v;
        }
        F.values[F.levels + 1] = total;
    }
}

template <int C> hipError_t pyramid_launch_c(const PyramidArgs &A, bool vec, uint64_t tiles, hipStream_t stream)
{
    if (vec) hipLaunchKernelGGL((pyramid_kernel<C, true>), dim3((unsigned) tiles), dim3(kPT), 0, stream, A);
    else hipLaunchKernelGGL((pyramid_kernel<C, false>), dim3((unsigned) tiles), dim3(kPT), 0, stream, A);
    return hipGetLastError();
}

}  // namespace

bool pyramid_supported(int64_t n, int64_t h, int64_t w, int64_t c, int64_t levels)
{
    if (n < 1 || h < 1 || w < 1 || c < 1 || c > kPyramidMaxChannels || levels < 0 || levels > kPyramidMaxLevels) return false;
    if (n >= (1ll << 31) || h >= (1ll << 31) || w >= (1ll << 31)) return false;
    return (double) n * (double) h * (double) w * (double) c < 2147483648.0;
}

uint64_t pyramid_tiles(int n, int h, int w)
{
    return (uint64_t) ((w + kTile - 1) / kTile) * (uint64_t) ((h + kTile - 1) / kTile) * (uint64_t) n;
}

double pyramid_count(int n, int h, int w, int c, int level)
{
    const int64_t hl = ((int64_t) h + (1ll << level) - 1) >> level, wl = ((int64_t) w + (1ll << level) - 1) >> level;
    return (double) n * (double) hl * (double) wl * (double) c;
}

hipError_t launch_pyramid_loss(int kind, const float *x, const float *y, int n, int h, int w, int c, int levels, const double *weights,
                               double delta, double *values, float *grad, double *partials, hipStream_t stream)
{
    if (!pyramid_supported(n, h, w, c, levels) || kind < kPyramidL1 || kind > kPyramidHuber) return hipErrorInvalidValue;
    PyramidArgs A = {};
    A.x = x; A.y = y; A.grad = grad; A.partials = partials;
    A.H = h; A.W = w;
    A.tiles_x = (uint32_t) ((w + kTile - 1) / kTile);
    A.tiles_y = (uint32_t) ((h + kTile - 1) / kTile);
    A.levels = levels; A.kind = kind;
    A.delta = (float) delta; A.half_delta = (float) (0.5 * delta);
    PyramidFinishArgs F = {};
    for (int l = 0; l <= levels; ++l) {
        F.count[l] = pyramid_count(n, h, w, c, l);
        F.weight[l] = weights[l];
        A.coef[l] = (float) (weights[l] / F.count[l]);
    }
    const uint64_t tiles = pyramid_tiles(n, h, w);
    const bool vec = ((int64_t) w * c) % 4 == 0 && ((((uintptr_t) x) | ((uintptr_t) y) | ((uintptr_t) grad)) & 15u) == 0;
    hipError_t e = hipErrorInvalidValue;
    switch (c) {
    case 1: e = pyramid_launch_c<1>(A, vec, tiles, stream); break;
    case 2: e = pyramid_launch_c<2>(A, vec, tiles, stream); break;
    case 3: e = pyramid_launch_c<3>(A, vec, tiles, stream); break;
    case 4: e = pyramid_launch_c<4>(A, vec, tiles, stream); break;
    case 5: e = pyramid_launch_c<5>(A, vec, tiles, stream); break;
    case 6: e = pyramid_launch_c<6>(A, vec, tiles, stream); break;
    case 7: e = pyramid_launch_c<7>(A, vec, tiles, stream); break;
    case 8: e = pyramid_launch_c<8>(A, vec, tiles, stream); break;
    }
    if (e != hipSuccess) return e;
    F.partials = partials; F.tiles = tiles; F.levels = levels; F.values = values;
    hipLaunchKernelGGL(pyramid_finish_kernel, dim3(1), dim3(kFinish), 0, stream, F);
    return hipGetLastError();
}

}  // namespace drt
