// drt_priors.hip -- regularisers of a dense voxel grid p (Z,Y,X,C), channels last and independent of each other (DESIGN.md "Grid priors"):
//   tv          R = (1/N) sum sqrt(eps + dx^2 + dy^2 + dz^2)      d* = forward differences, 0 where the upper index leaves the grid
//   smoothness  R = (1/N) sum (dx^2 + dy^2 + dz^2)
//   sparsity    R = (1/N) sum |p|                                  gradient sign(p) / N, sign(0) = 0 (torch's convention)
// One pass: reads p, ADDS weight dR/dp into the caller's gradient grid g (optional) and sums R per workgroup into doubles, which ONE workgroup
// then adds in a fixed order (the scheme of drt_loss.hip): the same bits on every call, no float atomics.
// The gradient of the stencil kinds is a gather: with r = 1 / sqrt(eps + ...) (tv) or 2 (smoothness) and a_d = r d_d,
//   dR/dp[v] = (1/N) (-(a_x + a_y + a_z)[v] + a_x[v - e_x] + a_y[v - e_y] + a_z[v - e_z]),     terms below index 0 absent.
// Shape: a row is W = X C contiguous floats, the x-neighbour sits at +-C.  A workgroup owns a tile of kTY rows x kTW floats and marches along
// z.  LDS holds the value planes z and z + 1 with a halo of one row and C floats on every side (plane z + 2 is fetched into registers while
// plane z is worked on, and replaces it), and the plane of r at z (tile + the low-side halo, whose a_x / a_y the gather needs); a_z of the
// plane below stays in registers.  The stencil runs one column per lane (consecutive lanes on consecutive banks: no LDS conflict for any C);
// on the vector path the voxel gradients then cross LDS once more so that g is read and written 16 bytes per lane.
// Grids with few tiles are cut along z into chunks so that the device fills; a chunk that does not start at z = 0 first runs the plane
// below it without output, for its a_z.
#include "drt_launch.h"
#include <atomic>

namespace drt {

namespace {

constexpr int kPT = 512;                        // threads per workgroup
constexpr int kTY = 8, kTW = 512;               // tile: rows x floats of a row; one column per thread
constexpr int kH = 32;                          // LDS halo columns on each side (>= the largest C)
constexpr int kEW = kTW + 2 * kH;               // value plane: (kTY + 2) rows [y0 - 1, y0 + kTY] x kEW columns [w0 - kH, w0 + kTW + kH)
constexpr int kER = kTY + 2;
constexpr int kPlane = kER * kEW;
constexpr int kRW = kTW + kH;                   // r plane: (kTY + 1) rows [y0 - 1, y0 + kTY) x kRW columns [w0 - kH, w0 + kTW), same origin
constexpr int kRPlane = (kTY + 1) * kRW;
constexpr int kChunks = kPlane / 4;             // 16-byte chunks of a value plane; chunk i sits at float 4 i
constexpr int kPre = (kChunks + kPT - 1) / kPT;
constexpr int kGV = kTY * kTW / 4 / kPT;        // 16-byte chunks of the tile per thread
constexpr size_t kPriorLds = (size_t) (2 * kPlane + kRPlane) * sizeof(float);
constexpr int kMinChunkZ = 16;                  // planes per z chunk at least (one extra plane is run per chunk)
constexpr uint64_t kWantWgs = 2048;

static_assert(kRPlane >= kTY * kTW, "the voxel gradients of a tile are staged in the r plane");
static_assert(kPT * sizeof(double) <= kPriorLds && kTW == kPT && kGV * kPT * 4 == kTY * kTW && kH >= 32 && kEW % 4 == 0, "tile geometry");

struct PriorArgs {
    const float *p;
    float *g;
    double *partials;
    int nz, ny, W, C;            // W = X * C floats per row
    uint32_t tiles_w, tiles_y;
    int zc;                      // planes per z chunk
    float scale, eps;            // scale = weight / N
};

// torch.sign: 0 for 0 and NaN
__device__ inline float prior_sign(float x) { return (float) ((0.0f < x) - (x < 0.0f)); }

// chunk `idx` of value plane zz of the tile at (y0, w0): zeros where the grid ends or the stencil does not reach
template <bool VEC> __device__ inline float4 fetch_chunk(const PriorArgs &A, int zz, int y0, int w0, int idx)
{
    float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (idx >= kChunks || zz >= A.nz) return v;
    const int ly = idx / (kEW / 4), j = (idx - ly * (kEW / 4)) * 4;
    const int y = y0 - 1 + ly;
    if (y < 0 || y >= A.ny || j + 4 <= kH - A.C || j >= kH + kTW + A.C) return v;
    const int w = w0 - kH + j;
    const float *row = A.p + ((int64_t) zz * A.ny + y) * (int64_t) A.W;
    if (VEC) {                                   // W, w0, kH and j are multiples of 4: a chunk lies inside the row or outside
        if (w >= 0 && w < A.W) v = *reinterpret_cast<const float4 *>(row + w);
    } else {
        if (w >= 0 && w < A.W) v.x = row[w];
        if (w + 1 >= 0 && w + 1 < A.W) v.y = row[w + 1];
        if (w + 2 >= 0 && w + 2 < A.W) v.z = row[w + 2];
        if (w + 3 >= 0 && w + 3 < A.W) v.w = row[w + 3];
    }
    return v;
}

template <int KIND, bool VEC> __global__ void __launch_bounds__(kPT) grid_prior_kernel(PriorArgs A)
{
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int t = (int) threadIdx.x;
    uint32_t b = blockIdx.x;
    const uint32_t tw = b % A.tiles_w; b /= A.tiles_w;
    const uint32_t ty = b % A.tiles_y, zk = b / A.tiles_y;
    const int y0 = (int) ty * kTY, w0 = (int) tw * kTW;
    const int z0 = (int) zk * A.zc, z1 = min(A.nz, z0 + A.zc);
    const int C = A.C, W = A.W, ny = A.ny;
    double acc = 0.0;

    if (KIND == kPriorSparsity) {
        for (int z = z0; z < z1; ++z) {
            if (VEC) {
                for (int m = 0; m < kGV; ++m) {
                    const int c = t + m * kPT, y = y0 + c / (kTW / 4), w = w0 + (c % (kTW / 4)) * 4;
                    if (y >= ny || w >= W) continue;
                    const int64_t off = ((int64_t) z * ny + y) * (int64_t) W + w;
                    const float4 v = *reinterpret_cast<const float4 *>(A.p + off);
                    acc += (double) fabsf(v.x); acc += (double) fabsf(v.y); acc += (double) fabsf(v.z); acc += (double) fabsf(v.w);
                    if (A.g) {
                        float4 gv = *reinterpret_cast<float4 *>(A.g + off);
                        gv.x += A.scale * prior_sign(v.x); gv.y += A.scale * prior_sign(v.y);
                        gv.z += A.scale * prior_sign(v.z); gv.w += A.scale * prior_sign(v.w);
                        *reinterpret_cast<float4 *>(A.g + off) = gv;
                    }
                }
            } else {
                const int w = w0 + t;
                for (int k = 0; k < kTY; ++k) {
                    const int y = y0 + k;
                    if (y >= ny || w >= W) continue;
                    const int64_t off = ((int64_t) z * ny + y) * (int64_t) W + w;
                    const float v = A.p[off];
                    acc += (double) fabsf(v);
                    if (A.g) A.g[off] += A.scale * prior_sign(v);
                }
            }
        }
    } else {
        float *R = lds + 2 * kPlane;
        const int zs = z0 > 0 ? z0 - 1 : 0;          // a chunk above the first starts one plane early: that step only leaves its a_z
        for (int i = 0; i < kPre; ++i) {
            const int idx = t + i * kPT;
            if (idx < kChunks) {
                reinterpret_cast<float4 *>(lds)[idx] = fetch_chunk<VEC>(A, zs, y0, w0, idx);
                reinterpret_cast<float4 *>(lds + kPlane)[idx] = fetch_chunk<VEC>(A, zs + 1, y0, w0, idx);
            }
        }
        __syncthreads();
        float az[kTY];
        for (int k = 0; k < kTY; ++k) az[k] = 0.0f;
        const int w = w0 + t, j = kH + t;            // this thread's column, in the grid and in the LDS planes
        for (int z = zs; z < z1; ++z) {
            float *P0 = lds + ((z - zs) & 1) * kPlane, *P1 = lds + (((z - zs) & 1) ^ 1) * kPlane;
            const bool emit = z >= z0, more = z + 1 < z1, hz = z + 1 < A.nz;
            float4 pre[kPre], gpre[kGV];
            if (more)                                // plane z + 2, in flight while plane z is worked on
                for (int i = 0; i < kPre; ++i) pre[i] = fetch_chunk<VEC>(A, z + 2, y0, w0, t + i * kPT);
            if (VEC && emit && A.g)
                for (int m = 0; m < kGV; ++m) {
                    const int c = t + m * kPT, y = y0 + c / (kTW / 4), wc = w0 + (c % (kTW / 4)) * 4;
                    gpre[m] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                    if (y < ny && wc < W) gpre[m] = *reinterpret_cast<const float4 *>(A.g + ((int64_t) z * ny + y) * (int64_t) W + wc);
                }
            if (KIND == kPriorTV) {
                for (int idx = t; idx < kRPlane; idx += kPT) {
                    const int ly = idx / kRW, jj = idx - ly * kRW;
                    if (jj < kH - C) continue;
                    const int y = y0 - 1 + ly, ww = w0 - kH + jj;
                    float r = 0.0f;
                    if (y >= 0 && y < ny && ww >= 0 && ww < W) {
                        const float c = P0[ly * kEW + jj];
                        const float dx = ww + C < W ? P0[ly * kEW + jj + C] - c : 0.0f;
                        const float dy = y + 1 < ny ? P0[(ly + 1) * kEW + jj] - c : 0.0f;
                        const float dz = hz ? P1[ly * kEW + jj] - c : 0.0f;
                        r = __builtin_amdgcn_rsqf(A.eps + dx * dx + dy * dy + dz * dz);      // v_rsq_f32, 1 ulp; eps is a normal float: no denormal reaches it
                    }
                    R[idx] = r;
                }
                __syncthreads();
            }
            float gr[kTY];
            for (int k = 0; k < kTY; ++k) {
                const int y = y0 + k, ly = k + 1;
                float gv = 0.0f, azn = 0.0f;
                if (w < W && y < ny) {
                    const float c = P0[ly * kEW + j];
                    const float dx = w + C < W ? P0[ly * kEW + j + C] - c : 0.0f;
                    const float dy = y + 1 < ny ? P0[(ly + 1) * kEW + j] - c : 0.0f;
                    const float dz = hz ? P1[ly * kEW + j] - c : 0.0f;
                    const float ss = dx * dx + dy * dy + dz * dz;
                    float r = 2.0f, term = ss, rl = 2.0f, rd = 2.0f;
                    if (KIND == kPriorTV) {
                        r = R[ly * kRW + j];
                        term = (A.eps + dx * dx + dy * dy + dz * dz) * r;      // sqrt(s) = s / sqrt(s)
                        if (w >= C) rl = R[ly * kRW + j - C];
                        if (y >= 1) rd = R[(ly - 1) * kRW + j];
                    }
                    azn = r * dz;
                    float s = -((r * dx + r * dy) + azn);
                    if (w >= C) s += rl * (c - P0[ly * kEW + j - C]);
                    if (y >= 1) s += rd * (c - P0[(ly - 1) * kEW + j]);
                    s += az[k];
                    gv = A.scale * s;
                    if (emit) acc += (double) term;
                }
                az[k] = azn;
                gr[k] = gv;
            }
            __syncthreads();                         // plane z and its r are read: both make room
            if (emit && A.g) {
                if (VEC) {
                    for (int k = 0; k < kTY; ++k) R[k * kTW + t] = gr[k];
                } else if (w < W) {
                    for (int k = 0; k < kTY; ++k)
                        if (y0 + k < ny) A.g[((int64_t) z * ny + (y0 + k)) * (int64_t) W + w] += gr[k];
                }
            }
            if (more)
                for (int i = 0; i < kPre; ++i)
                    if (t + i * kPT < kChunks) reinterpret_cast<float4 *>(P0)[t + i * kPT] = pre[i];
            __syncthreads();
            if (VEC && emit && A.g) {
                for (int m = 0; m < kGV; ++m) {
                    const int c = t + m * kPT, y = y0 + c / (kTW / 4), wc = w0 + (c % (kTW / 4)) * 4;
                    if (y >= ny || wc >= W) continue;
                    const float4 d = reinterpret_cast<const float4 *>(R)[c];
                    float4 gv = gpre[m];
                    gv.x += d.x; gv.y += d.y; gv.z += d.z; gv.w += d.w;
                    *reinterpret_cast<float4 *>(A.g + ((int64_t) z * ny + y) * (int64_t) W + wc) = gv;
                }
                if (KIND == kPriorTV) __syncthreads();   // (the next step's r overwrites the staged gradients; smoothness writes them behind a barrier)
            }
        }
        __syncthreads();
    }

    // fixed-order tree over the workgroup's doubles
    double *red = reinterpret_cast<double *>(lds);
    red[t] = acc;
    for (int s = kPT / 2; s > 0; s >>= 1) {
        __syncthreads();
        if (t < s) red[t] += red[t + s];
    }
    if (t == 0) A.partials[blockIdx.x] = red[0];
}

// one workgroup: thread i sums partials i, i + 256, ... in order, then the fixed tree
__global__ void __launch_bounds__(256) grid_prior_finish_kernel(const double *partials, uint64_t n_partials, double n_entries, double weight,
                                                                double *value)
{
    __shared__ double red[256];
    double s = 0.0;
    for (uint64_t i = threadIdx.x; i < n_partials; i += 256) s += partials[i];
    red[threadIdx.x] = s;
    for (int w = 128; w > 0; w >>= 1) {
        __syncthreads();
        if ((int) threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
    }
    if (threadIdx.x == 0) value[0] = weight * (red[0] / n_entries);
}

struct PriorPlan {
    uint32_t tiles_w, tiles_y, z_chunks;
    int zc;
    uint64_t wgs;
};

PriorPlan prior_plan(int nz, int ny, int nx, int nc)
{
    PriorPlan L;
    const int64_t W = (int64_t) nx * nc;
    L.tiles_w = (uint32_t) ((W + kTW - 1) / kTW);
    L.tiles_y = (uint32_t) ((ny + kTY - 1) / kTY);
    const uint64_t tiles = (uint64_t) L.tiles_w * L.tiles_y;
    uint64_t want = (kWantWgs + tiles - 1) / tiles, most = ((uint64_t) nz + kMinChunkZ - 1) / kMinChunkZ;
    if (want > most) want = most;
    if (want < 1) want = 1;
    L.zc = (int) (((uint64_t) nz + want - 1) / want);
    L.z_chunks = (uint32_t) ((nz + L.zc - 1) / L.zc);
    L.wgs = tiles * L.z_chunks;
    return L;
}

template <int KIND, bool VEC> hipError_t prior_launch(const PriorArgs &A, uint64_t wgs, hipStream_t stream)
{
    static std::atomic<bool> done[64];
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) dev = 63;
    if (!done[dev] || dev == 63) {
        const hipError_t e = hipFuncSetAttribute((const void *) grid_prior_kernel<KIND, VEC>, hipFuncAttributeMaxDynamicSharedMemorySize, (int) kPriorLds);
        if (e != hipSuccess) return e;
        done[dev] = true;
    }
    hipLaunchKernelGGL((grid_prior_kernel<KIND, VEC>), dim3((unsigned) wgs), dim3(kPT), kPriorLds, stream, A);
    return hipGetLastError();
}

}  // namespace

bool grid_prior_supported(int64_t nz, int64_t ny, int64_t nx, int64_t nc)
{
    if (nz < 1 || ny < 1 || nx < 1 || nc < 1 || nc > kPriorMaxChannels) return false;
    if (nz > (1 << 30) || ny > (1 << 30) || nx * nc > (1 << 30)) return false;
    return prior_plan((int) nz, (int) ny, (int) nx, (int) nc).wgs <= 0x7fffffffull;
}

uint64_t grid_prior_partials(int nz, int ny, int nx, int nc)
{
    return grid_prior_supported(nz, ny, nx, nc) ? prior_plan(nz, ny, nx, nc).wgs : 0;
}

hipError_t launch_grid_prior(int kind, const float *p, float *g, double *value, double *partials, int nz, int ny, int nx, int nc, double weight,
                             float eps, hipStream_t stream)
{
    if (!grid_prior_supported(nz, ny, nx, nc) || kind < kPriorTV || kind > kPriorSparsity) return hipErrorInvalidValue;
    const PriorPlan L = prior_plan(nz, ny, nx, nc);
    const double n = (double) nz * (double) ny * (double) nx * (double) nc;
    PriorArgs A;
    A.p = p; A.g = g; A.partials = partials;
    A.nz = nz; A.ny = ny; A.W = nx * nc; A.C = nc;
    A.tiles_w = L.tiles_w; A.tiles_y = L.tiles_y; A.zc = L.zc;
    A.scale = (float) (weight / n); A.eps = eps;
    // 16-byte accesses need 16-byte aligned bases and rows that keep the alignment; any other float grid takes the scalar path
    const bool vec = A.W % 4 == 0 && ((uintptr_t) p | (uintptr_t) g) % 16 == 0;
    hipError_t e;
    switch (kind * 2 + (vec ? 1 : 0)) {
        case kPriorTV * 2: e = prior_launch<kPriorTV, false>(A, L.wgs, stream); break;
        case kPriorTV * 2 + 1: e = prior_launch<kPriorTV, true>(A, L.wgs, stream); break;
        case kPriorSmoothness * 2: e = prior_launch<kPriorSmoothness, false>(A, L.wgs, stream); break;
        case kPriorSmoothness * 2 + 1: e = prior_launch<kPriorSmoothness, true>(A, L.wgs, stream); break;
        case kPriorSparsity * 2: e = prior_launch<kPriorSparsity, false>(A, L.wgs, stream); break;
        default: e = prior_launch<kPriorSparsity, true>(A, L.wgs, stream); break;
    }
    if (e != hipSuccess || !value) return e;
    hipLaunchKernelGGL(grid_prior_finish_kernel, dim3(1), dim3(256), 0, stream, (const double *) partials, L.wgs, n, weight, value);
    return hipGetLastError();
}

}  // namespace drt
