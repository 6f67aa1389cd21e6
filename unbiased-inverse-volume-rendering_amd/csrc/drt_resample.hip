// drt_resample.hip -- R: a dense grid (Zs,Ys,Xs,C), channels last, evaluated by the lookup convention of axis_setup (drt_device.h: cell-centred,
// clamped) at the voxel centres of a target lattice (Zt,Yt,Xt), and its transpose (DESIGN.md "Resampled colour grids").
// Separable per axis; on an axis with ns source and nt target voxels the stencil of target index t comes from integers:
//   num = (2t + 1) ns - nt,  den = 2 nt,  f = floor(num / den),  r = num - f den,  w1 = float(r) / float(den),  w0 = 1 - w1,
//   i0 = clamp(f, 0, ns - 1),  i1 = clamp(f + 1, 0, ns - 1)                            (extents <= 4096: num < 2^26; num > -den: f >= -1)
// The value is interpolated along x, then y, then z, every step a w0 + b w1 rounded per operation; a term whose weight is exactly 0 is not
// added, so an axis with ns == nt copies and equal lattices copy the words.
// Forward: one lane per target (voxel, channel or channel quad), x fastest; a workgroup takes a piece of kRows consecutive target rows,
// so a lane's x stencil is computed once for them and the y and z stencils are uniform (LDS only hands the rows' y stencils round).
// Transpose: a gather, one lane per source (voxel, channel or quad).  f is monotone in t, so the targets whose stencil holds source index i
// are the contiguous range  first(i - 1) <= t < first(i + 1)  with  first(k) = min t with f(t) >= k = ceil(((2k + 1) nt - ns) / (2 ns)),
// open below at i = 0 and above at i = ns - 1; inside it f is i - 1 or i, so the weight needs one compare and no integer division.  The
// sum runs in ascending (tz, ty, tx) order, each term ((wz wy) wx) g: no atomics, the same bits on every call.
#include "drt_launch.h"

namespace drt {

namespace {

constexpr int kMaxThreads = 1024;
constexpr int kRows = 8;                        // forward: target rows per workgroup

struct ResampleArgs {
    const float *in;
    float *out;
    int sz, sy, sx;              // source lattice
    int tz, ty, tx;              // target lattice
    int C;
    int accumulate;              // transpose: add to `out`
};

struct AxisStencil {
    int i0, i1;
    float w0, w1;
};

__device__ __forceinline__ AxisStencil axis_stencil(int t, int ns, int nt)
{
    const int den = 2 * nt, num = (2 * t + 1) * ns - nt;
    const int f = num >= 0 ? num / den : -1;
    const int r = num - f * den;
    AxisStencil s;
    s.w1 = (float) r / (float) den;
    s.w0 = 1.0f - s.w1;
    s.i0 = min(max(f, 0), ns - 1);
    s.i1 = min(f + 1, ns - 1);
    return s;
}

// first target index whose f reaches k (k >= 0); may lie past the axis
__host__ __device__ __forceinline__ int axis_first(int k, int ns, int nt)
{
    const int n = (2 * k + 1) * nt - ns;
    return n <= 0 ? 0 : (n + 2 * ns - 1) / (2 * ns);
}

// targets [first, last] whose stencil holds source index i; empty: last < first
__host__ __device__ __forceinline__ void axis_range(int i, int ns, int nt, int &first, int &last)
{
    first = i == 0 ? 0 : axis_first(i - 1, ns, nt);
    const int end = i == ns - 1 ? nt : axis_first(i + 1, ns, nt);
    last = (end < nt ? end : nt) - 1;
}

// weight of source index i in the stencil of target t, t inside axis_range(i); 0: i is not added there
__device__ __forceinline__ float axis_weight(int i, int t, int ns, int nt)
{
    const int den = 2 * nt, num = (2 * t + 1) * ns - nt;
    const int f = num >= i * den ? i : i - 1;
    const int r = num - f * den;
    const float w1 = (float) r / (float) den, w0 = 1.0f - w1;
    const int i0 = max(f, 0), i1 = min(f + 1, ns - 1);
    float w = 0.0f;
    if (i0 == i) w = w0;
    if (i1 == i && r != 0) w = i0 == i ? w0 + w1 : w1;
    return w;
}

__device__ __forceinline__ float mix(float a, float b, float w0, float w1) { return a * w0 + b * w1; }
__device__ __forceinline__ float4 mix(float4 a, float4 b, float w0, float w1)
{
    return make_float4(a.x * w0 + b.x * w1, a.y * w0 + b.y * w1, a.z * w0 + b.z * w1, a.w * w0 + b.w * w1);
}
// a w0 + b w1, or a itself where w1 is exactly 0 (b is not added: a select, not a branch, so that a lane's loads are in flight together)
__device__ __forceinline__ float pick(float a, float b, float w0, float w1) { return w1 != 0.0f ? mix(a, b, w0, w1) : a; }
__device__ __forceinline__ float4 pick(float4 a, float4 b, float w0, float w1)
{
    const float4 m = mix(a, b, w0, w1);
    return w1 != 0.0f ? m : a;
}
__device__ __forceinline__ void add_scaled(float &s, float w, float g) { s += w * g; }
__device__ __forceinline__ void add_scaled(float4 &s, float w, float4 g) { s.x += w * g.x; s.y += w * g.y; s.z += w * g.z; s.w += w * g.w; }
__device__ __forceinline__ void add_to(float &s, float a) { s += a; }
__device__ __forceinline__ void add_to(float4 &s, float4 a) { s.x += a.x; s.y += a.y; s.z += a.z; s.w += a.w; }
template <class T> __device__ __forceinline__ T zero();
template <> __device__ __forceinline__ float zero<float>() { return 0.0f; }
template <> __device__ __forceinline__ float4 zero<float4>() { return make_float4(0.0f, 0.0f, 0.0f, 0.0f); }

__device__ __forceinline__ int uniform(int v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ float uniform(float v) { return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(v))); }

// T = float: one lane per (voxel, channel); T = float4: per (voxel, channel quad), both grids 16-byte aligned and C % 4 == 0.
// A workgroup owns a piece of kRows consecutive target rows: a lane's x stencil serves all of them, the rows' y stencils are computed by
// the first lanes and shared through LDS, and the row bases stay in scalar registers.
template <class T> __global__ void __launch_bounds__(kMaxThreads) grid_resample_kernel(ResampleArgs A)
{
    __shared__ AxisStencil ys[kRows];
    const int Q = A.C / (int) (sizeof(T) / sizeof(float));           // lanes per voxel
    const int y_first = (int) blockIdx.y * kRows, tz = (int) blockIdx.z;
    const int rows = min(kRows, A.ty - y_first);
    if ((int) threadIdx.x < rows) ys[threadIdx.x] = axis_stencil(y_first + (int) threadIdx.x, A.sy, A.ty);
    __syncthreads();
    const int w = (int) (blockIdx.x * blockDim.x + threadIdx.x);
    if (w >= A.tx * Q) return;
    const int x = w / Q, q = w - x * Q;
    const AxisStencil X = axis_stencil(x, A.sx, A.tx), Z = axis_stencil(tz, A.sz, A.tz);
    const int o0 = X.i0 * Q + q, o1 = X.i1 * Q + q;                  // (< 4096 * 32)
    const T *__restrict__ in = reinterpret_cast<const T *>(A.in);
    const int64_t row = (int64_t) A.sx * Q, out_row = (int64_t) A.tx * Q;
    T *__restrict__ out = reinterpret_cast<T *>(A.out) + ((int64_t) tz * A.ty + y_first) * out_row + w;
    auto value = [&](int r) {
        const int yi0 = uniform(ys[r].i0), yi1 = uniform(ys[r].i1);
        const float yw0 = uniform(ys[r].w0), yw1 = uniform(ys[r].w1);
        auto along_x = [&](int z, int y) {
            const T *p = in + ((int64_t) z * A.sy + y) * row;
            return pick(p[o0], p[o1], X.w0, X.w1);
        };
        auto along_y = [&](int z) {
            return pick(along_x(z, yi0), along_x(z, yi1), yw0, yw1);
        };
        return pick(along_y(Z.i0), along_y(Z.i1), Z.w0, Z.w1);
    };
    constexpr int kBatch = sizeof(T) == 16 ? 2 : kRows;             // rows whose loads are in flight together (8 loads a row)
    if (rows == kRows) {
        for (int r0 = 0; r0 < kRows; r0 += kBatch) {
            T v[kBatch];
#pragma unroll
            for (int r = 0; r < kBatch; ++r) v[r] = value(r0 + r);
#pragma unroll
            for (int r = 0; r < kBatch; ++r) out[(r0 + r) * out_row] = v[r];
        }
    } else {
        for (int r = 0; r < rows; ++r) out[r * out_row] = value(r);
    }
}

// in: the target-lattice gradient (tz, ty, tx, C); out: the source-lattice gradient (sz, sy, sx, C)
// NX > 0: no x range of the call is longer than NX, and a lane keeps its x weights in registers; 0: any length
template <class T, int NX> __global__ void __launch_bounds__(kMaxThreads) grid_resample_transpose_kernel(ResampleArgs A)
{
    const int Q = A.C / (int) (sizeof(T) / sizeof(float));
    const int w = (int) (blockIdx.x * blockDim.x + threadIdx.x);
    if (w >= A.sx * Q) return;
    const int x = w / Q, q = w - x * Q;
    const int y = (int) blockIdx.y, z = (int) blockIdx.z;
    int x0, x1, y0, y1, z0, z1;
    axis_range(x, A.sx, A.tx, x0, x1);
    axis_range(y, A.sy, A.ty, y0, y1);
    axis_range(z, A.sz, A.tz, z0, z1);
    const T *__restrict__ g = reinterpret_cast<const T *>(A.in);
    const int64_t row = (int64_t) A.tx * Q;
    T acc = zero<T>();
    if (NX > 0) {
        const int nx = x1 - x0 + 1;
        float wx[NX > 0 ? NX : 1];
        int ox[NX > 0 ? NX : 1];                                     // every tap's offset in its row, clamped into it: a tap past the range
#pragma unroll                                                       // has weight 0 and is loaded (so that the loads go out together) but not added
        for (int k = 0; k < NX; ++k) {
            wx[k] = k < nx ? axis_weight(x, x0 + k, A.sx, A.tx) : 0.0f;
            ox[k] = min(max(x0 + k, 0), A.tx - 1) * Q + q;
        }
        for (int tz = z0; tz <= z1; ++tz) {
            const float wz = axis_weight(z, tz, A.sz, A.tz);
            if (wz == 0.0f) continue;
            for (int ty = y0; ty <= y1; ++ty) {
                const float wy = axis_weight(y, ty, A.sy, A.ty);
                if (wy == 0.0f) continue;
                const float wzy = wz * wy;
                const T *p = g + ((int64_t) tz * A.ty + ty) * row;
                T gv[NX > 0 ? NX : 1];
#pragma unroll
                for (int k = 0; k < NX; ++k) gv[k] = p[ox[k]];
#pragma unroll
                for (int k = 0; k < NX; ++k)
                    if (wx[k] != 0.0f) add_scaled(acc, wzy * wx[k], gv[k]);
            }
        }
    } else {
        for (int tz = z0; tz <= z1; ++tz) {
            const float wz = axis_weight(z, tz, A.sz, A.tz);
            if (wz == 0.0f) continue;
            for (int ty = y0; ty <= y1; ++ty) {
                const float wy = axis_weight(y, ty, A.sy, A.ty);
                if (wy == 0.0f) continue;
                const float wzy = wz * wy;
                const T *p = g + ((int64_t) tz * A.ty + ty) * row + q;
                for (int tx = x0; tx <= x1; ++tx) {
                    const float wxx = axis_weight(x, tx, A.sx, A.tx);
                    if (wxx != 0.0f) add_scaled(acc, wzy * wxx, p[(int64_t) tx * Q]);
                }
            }
        }
    }
    T *out = reinterpret_cast<T *>(A.out) + ((int64_t) z * A.sy + y) * ((int64_t) A.sx * Q) + w;
    if (A.accumulate) {
        T v = *out;
        add_to(v, acc);
        acc = v;
    }
    *out = acc;
}

// workgroups of whole waves that share a row of `lanes` lanes evenly
void row_launch(int lanes, unsigned &blocks, unsigned &threads)
{
    blocks = (unsigned) ((lanes + kMaxThreads - 1) / kMaxThreads);
    const unsigned per = ((unsigned) lanes + blocks - 1) / blocks;
    threads = (per + 63u) / 64u * 64u;
}

}  // namespace

bool grid_resample_supported(int64_t sz, int64_t sy, int64_t sx, int64_t tz, int64_t ty, int64_t tx, int64_t nc)
{
    const int64_t e[6] = {sz, sy, sx, tz, ty, tx};
    for (int64_t v : e)
        if (v < 1 || v > kResampleMaxExtent) return false;
    return nc >= 1 && nc <= kPriorMaxChannels;
}

hipError_t launch_grid_resample(const float *src, int sz, int sy, int sx, float *dst, int tz, int ty, int tx, int nc, hipStream_t stream)
{
    if (!grid_resample_supported(sz, sy, sx, tz, ty, tx, nc)) return hipErrorInvalidValue;
    ResampleArgs A;
    A.in = src; A.out = dst;
    A.sz = sz; A.sy = sy; A.sx = sx; A.tz = tz; A.ty = ty; A.tx = tx; A.C = nc; A.accumulate = 0;
    // 16-byte accesses need 16-byte aligned bases and whole quads per voxel; any other float grid takes the 4-byte path
    const bool vec = nc % 4 == 0 && ((uintptr_t) src | (uintptr_t) dst) % 16 == 0;
    unsigned blocks, threads;
    row_launch(tx * (vec ? nc / 4 : nc), blocks, threads);
    const dim3 grid(blocks, (unsigned) ((ty + kRows - 1) / kRows), (unsigned) tz);
    if (vec) hipLaunchKernelGGL(grid_resample_kernel<float4>, grid, dim3(threads), 0, stream, A);
    else hipLaunchKernelGGL(grid_resample_kernel<float>, grid, dim3(threads), 0, stream, A);
    return hipGetLastError();
}

hipError_t launch_grid_resample_transpose(const float *g_dst, int tz, int ty, int tx, float *g_src, int sz, int sy, int sx, int nc,
                                          bool accumulate, hipStream_t stream)
{
    if (!grid_resample_supported(sz, sy, sx, tz, ty, tx, nc)) return hipErrorInvalidValue;
    ResampleArgs A;
    A.in = g_dst; A.out = g_src;
    A.sz = sz; A.sy = sy; A.sx = sx; A.tz = tz; A.ty = ty; A.tx = tx; A.C = nc; A.accumulate = accumulate ? 1 : 0;
    const bool vec = nc % 4 == 0 && ((uintptr_t) g_dst | (uintptr_t) g_src) % 16 == 0;
    unsigned blocks, threads;
    row_launch(sx * (vec ? nc / 4 : nc), blocks, threads);
    const dim3 grid(blocks, (unsigned) sy, (unsigned) sz);
    int longest = 0;                                                 // the longest x range (at most 4096 closed forms on the host)
    for (int i = 0; i < sx; ++i) {
        int first, last;
        axis_range(i, sx, tx, first, last);
        if (last - first + 1 > longest) longest = last - first + 1;
    }
    const int nx = longest <= 2 ? 2 : longest <= 4 ? 4 : longest <= 8 ? 8 : 0;
    const dim3 block(threads);
    switch (nx * 2 + (vec ? 1 : 0)) {
        case 4: hipLaunchKernelGGL((grid_resample_transpose_kernel<float, 2>), grid, block, 0, stream, A); break;
        case 5: hipLaunchKernelGGL((grid_resample_transpose_kernel<float4, 2>), grid, block, 0, stream, A); break;
        case 8: hipLaunchKernelGGL((grid_resample_transpose_kernel<float, 4>), grid, block, 0, stream, A); break;
        case 9: hipLaunchKernelGGL((grid_resample_transpose_kernel<float4, 4>), grid, block, 0, stream, A); break;
        case 16: hipLaunchKernelGGL((grid_resample_transpose_kernel<float, 8>), grid, block, 0, stream, A); break;
        case 17: hipLaunchKernelGGL((grid_resample_transpose_kernel<float4, 8>), grid, block, 0, stream, A); break;
        case 0: hipLaunchKernelGGL((grid_resample_transpose_kernel<float, 0>), grid, block, 0, stream, A); break;
        default: hipLaunchKernelGGL((grid_resample_transpose_kernel<float4, 0>), grid, block, 0, stream, A); break;
    }
    return hipGetLastError();
}

}  // namespace drt
