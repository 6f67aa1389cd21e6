// drt_hull.hip -- visual-hull support (DESIGN.md "Visual-hull support"): which voxels of a box the sensors' alpha mattes allow, and the
// optimizer step that stays inside them.
//
// visual_hull_kernel: counts[z][y][x] = {seen, hit} over the sensors of a table (16 floats each, the layout of batch_raygen_kernel) and the
// summed-area tables of their binary mattes, (n_sensors, H + 1, W + 1) int32 with a zero first row and column.  Lattice node (i, j, k) lies
// at bbox_min + (i / X, j / Y, k / Z) (bbox_max - bbox_min); for sensor s and node p, inverting sensor_ray (drt_device.h):
//   v = p - origin,  z = v.dir,  a = (v.left) / z,  b = (v.up) / z,  fx = (1 - a / tan_x) 0.5 W,  fy = (1 - b / tan_y) 0.5 H
// and the node is in front iff z > near = 1e-3 x the box's longest side.  A sensor sees a voxel iff its 8 nodes are in front and the pixel
// rectangle [floor(min fx) - margin, floor(max fx) + margin] x [floor(min fy) - margin, floor(max fy) + margin] lies inside the film; it
// hits the voxel iff the matte has a set pixel in that rectangle (four taps of the table).  Integers only: the same bytes on every call.
// Shape: a workgroup owns a brick of kBX x kBY x kBZ voxels, one per thread.  The sensor loop is uniform (a sensor's 16 floats are scalar
// loads); per sensor the workgroup projects the brick's (kBX + 1)(kBY + 1)(kBZ + 1) nodes once into LDS - a node that is not in front, or
// whose coordinates are not numbers, is stored as fx = +inf, which no film contains - and every voxel takes min / max over its 8 nodes
// from there.  Two LDS buffers alternate, so one barrier per sensor suffices.  Workgroups are dealt round-robin over the 8 XCDs: the block
// index is remapped so that each XCD works on one contiguous run of bricks, whose footprints are neighbours in the tables.
//
// adam_masked_kernel: the update of adam_step_kernel (drt_kernels.hip; the same expressions, -ffp-contract=off: the same bits) on the
// entries of a grid (voxels x C, channels last) whose voxel has support != 0 and - with skip_zero - whose gradient is not exactly 0;
// every other entry keeps the bits of p, m and v.  A 16-byte group whose voxels are all outside is skipped after reading the mask alone.
#include "drt_launch.h"

namespace drt {

namespace {

constexpr int kBX = 8, kBY = 8, kBZ = 4;                         // the brick: one voxel per thread
constexpr int kHT = kBX * kBY * kBZ;                             // 256 threads
constexpr int kNX = kBX + 1, kNY = kBY + 1, kNZ = kBZ + 1;
constexpr int kNodes = kNX * kNY * kNZ;                          // 405 nodes of a brick
constexpr unsigned kXcds = 8;

struct HullArgs {
    const float *sensors;
    const int32_t *sat;
    int32_t *counts;
    int n_sensors, height, width, margin;
    int X, Y, Z;
    uint32_t bricks_x, bricks_y, n_bricks, per_xcd;
    float bmin[3], ext[3], near;
    int wide;                                                    // counts is 8-byte aligned: one store per voxel
};

__global__ void __launch_bounds__(kHT) visual_hull_kernel(HullArgs A)
{
    __shared__ float2 nodes[2][kNodes];
    // blocks b, b + 8, ... share an XCD: give that XCD the bricks [r * per_xcd, (r + 1) * per_xcd)
    const uint32_t brick = (blockIdx.x % kXcds) * A.per_xcd + blockIdx.x / kXcds;
    if (brick >= A.n_bricks) return;                             // (uniform: the whole workgroup leaves before any barrier)
    const uint32_t bxi = brick % A.bricks_x, rest = brick / A.bricks_x;
    const int x0 = (int) bxi * kBX, y0 = (int) (rest % A.bricks_y) * kBY, z0 = (int) (rest / A.bricks_y) * kBZ;
    const int t = (int) threadIdx.x;
    const int tx = t % kBX, ty = (t / kBX) % kBY, tz = t / (kBX * kBY);
    const int x = x0 + tx, y = y0 + ty, z = z0 + tz;
    const bool live = x < A.X && y < A.Y && z < A.Z;
    const int n0 = (tz * kNY + ty) * kNX + tx;                   // the voxel's lowest node
    // this thread's nodes (at most two of the brick's), in world space; they depend on the node index alone
    float px[2], py[2], pz[2];
    for (int r = 0; r < 2; ++r) {
        const int n = t + r * kHT;
        const int i = x0 + n % kNX, j = y0 + (n / kNX) % kNY, k = z0 + n / (kNX * kNY);
        px[r] = A.bmin[0] + ((float) i / (float) A.X) * A.ext[0];
        py[r] = A.bmin[1] + ((float) j / (float) A.Y) * A.ext[1];
        pz[r] = A.bmin[2] + ((float) k / (float) A.Z) * A.ext[2];
    }
    const int64_t sat_row = (int64_t) A.width + 1, sat_plane = ((int64_t) A.height + 1) * sat_row;
    const float half_w = 0.5f * (float) A.width, half_h = 0.5f * (float) A.height;
    const float inf = __builtin_huge_valf();
    int seen = 0, hit = 0, turn = 0;
    for (int s = 0; s < A.n_sensors; ++s) {
        const float *sn = A.sensors + 16 * (int64_t) s;
        if ((int) sn[14] != A.width || (int) sn[15] != A.height) continue;      // (uniform) another film: this sensor sees nothing
        float2 *buf = nodes[turn];                                               // (alternates per sensor that is worked on)
        turn ^= 1;
        for (int r = 0; r < 2; ++r) {
            const int n = t + r * kHT;
            if (n >= kNodes) break;
            const float vx = px[r] - sn[0], vy = py[r] - sn[1], vz = pz[r] - sn[2];
            const float zc = vx * sn[9] + vy * sn[10] + vz * sn[11];
            float fx = inf, fy = inf;
            if (zc > A.near) {
                const float a = (vx * sn[3] + vy * sn[4] + vz * sn[5]) / zc;
                const float b = (vx * sn[6] + vy * sn[7] + vz * sn[8]) / zc;
                fx = (1.0f - a / sn[12]) * half_w;
                fy = (1.0f - b / sn[13]) * half_h;
                if (!(fx == fx) || !(fy == fy)) fx = inf;
            }
            buf[n] = make_float2(fx, fy);
        }
        __syncthreads();       // (the other buffer was last read before the previous barrier)
        if (!live) continue;
        float lx = inf, ly = inf, hx = -inf, hy = -inf;
        for (int c = 0; c < 8; ++c) {
            const float2 f = buf[n0 + (c & 1) + ((c >> 1) & 1) * kNX + (c >> 2) * (kNX * kNY)];
            lx = fminf(lx, f.x); hx = fmaxf(hx, f.x);
            ly = fminf(ly, f.y); hy = fmaxf(hy, f.y);
        }
        // floats this large are integers; the range test keeps the conversions to int exact
        if (!(lx >= -2.0f && ly >= -2.0f && hx < 2.0e9f && hy < 2.0e9f)) continue;
        const int fx0 = (int) floorf(lx) - A.margin, fx1 = (int) floorf(hx) + A.margin;
        const int fy0 = (int) floorf(ly) - A.margin, fy1 = (int) floorf(hy) + A.margin;
        if (fx0 < 0 || fy0 < 0 || fx1 > A.width - 1 || fy1 > A.height - 1) continue;
        ++seen;
        const int32_t *S = A.sat + (int64_t) s * sat_plane;
        const int64_t r0 = (int64_t) fy0 * sat_row, r1 = (int64_t) (fy1 + 1) * sat_row;
        const int32_t sum = S[r1 + fx1 + 1] - S[r0 + fx1 + 1] - S[r1 + fx0] + S[r0 + fx0];
        hit += sum > 0;
    }
    if (!live) return;
    const int64_t o = (((int64_t) z * A.Y + y) * A.X + x) * 2;
    if (A.wide) *reinterpret_cast<int2 *>(A.counts + o) = make_int2(seen, hit);
    else { A.counts[o] = seen; A.counts[o + 1] = hit; }
}

struct AdamArgs {
    float *p; const float *g; float *m, *v;
    const uint8_t *support;
    uint64_t n;                  // entries = voxels x channels
    uint32_t channels;
    int skip_zero;
    float b1, a1, b2, a2, eps, lr_t, lo, hi;
};

__device__ __forceinline__ void adam_update(const AdamArgs &A, float &pp, float gg, float &mm, float &vv)
{
    mm = mm * A.b1 + A.a1 * gg;
    vv = vv * A.b2 + A.a2 * (gg * gg);
    pp = pp - A.lr_t * (mm / (sqrtf(vv) + A.eps));
    pp = pp < A.lo ? A.lo : (pp > A.hi ? A.hi : pp);
}

// C > 0: the channel count at compile time; 0: A.channels
template <int C, bool VEC> __global__ void __launch_bounds__(256) adam_masked_kernel(AdamArgs A)
{
    const uint64_t stride = (uint64_t) gridDim.x * 256;
    const uint64_t ch = C > 0 ? (uint64_t) C : (uint64_t) A.channels;
    const bool skip = A.skip_zero != 0;
    if (VEC) {
        const uint64_t n4 = A.n / 4;
        float4 *p4 = reinterpret_cast<float4 *>(A.p), *m4 = reinterpret_cast<float4 *>(A.m), *v4 = reinterpret_cast<float4 *>(A.v);
        const float4 *g4 = reinterpret_cast<const float4 *>(A.g);
        for (uint64_t i = (uint64_t) blockIdx.x * 256 + threadIdx.x; i < n4; i += stride) {
            bool in[4] = {true, true, true, true};
            if (A.support) {
                const uint64_t e = 4 * i;
                if (C == 1) {                                                // (one 4-byte load of the four bytes measured no faster)
                    for (int k = 0; k < 4; ++k) in[k] = A.support[e + k] != 0;
                } else {
                    uint64_t vox = e / ch;
                    uint32_t c = (uint32_t) (e - vox * ch);
                    for (int k = 0; k < 4; ++k) {
                        in[k] = A.support[vox] != 0;
                        if (++c == (uint32_t) ch) { c = 0; ++vox; }
                    }
                }
                if (!(in[0] | in[1] | in[2] | in[3])) continue;              // nothing but the mask was read
            }
            float4 P = p4[i], M = m4[i], V = v4[i]; const float4 G = g4[i];
            if (in[0] && !(skip && G.x == 0.0f)) adam_update(A, P.x, G.x, M.x, V.x);
            if (in[1] && !(skip && G.y == 0.0f)) adam_update(A, P.y, G.y, M.y, V.y);
            if (in[2] && !(skip && G.z == 0.0f)) adam_update(A, P.z, G.z, M.z, V.z);
            if (in[3] && !(skip && G.w == 0.0f)) adam_update(A, P.w, G.w, M.w, V.w);
            p4[i] = P; m4[i] = M; v4[i] = V;                                 // (entries that took no update: the words just read)
        }
    }
    // the entries the 16-byte path does not take: all of them, or the last n % 4
    const uint64_t first = VEC ? (A.n / 4) * 4 : 0;
    for (uint64_t e = first + (uint64_t) blockIdx.x * 256 + threadIdx.x; e < A.n; e += stride) {
        if (A.support && A.support[e / ch] == 0) continue;
        const float gg = A.g[e];
        if (skip && gg == 0.0f) continue;
        adam_update(A, A.p[e], gg, A.m[e], A.v[e]);
    }
}

template <bool VEC> void adam_masked_dispatch(const AdamArgs &A, unsigned blocks, hipStream_t stream)
{
    switch (A.channels) {
        case 1: hipLaunchKernelGGL((adam_masked_kernel<1, VEC>), dim3(blocks), dim3(256), 0, stream, A); break;
        case 3: hipLaunchKernelGGL((adam_masked_kernel<3, VEC>), dim3(blocks), dim3(256), 0, stream, A); break;
        case 4: hipLaunchKernelGGL((adam_masked_kernel<4, VEC>), dim3(blocks), dim3(256), 0, stream, A); break;
        default: hipLaunchKernelGGL((adam_masked_kernel<0, VEC>), dim3(blocks), dim3(256), 0, stream, A); break;
    }
}

}  // namespace

hipError_t launch_visual_hull(const float *sensors, int n_sensors, const int32_t *sat, int height, int width, const float bbox_min[3],
                              const float bbox_max[3], int X, int Y, int Z, int margin, int32_t *counts, hipStream_t stream)
{
    HullArgs A;
    A.sensors = sensors; A.sat = sat; A.counts = counts;
    A.n_sensors = n_sensors; A.height = height; A.width = width; A.margin = margin;
    A.X = X; A.Y = Y; A.Z = Z;
    A.bricks_x = (uint32_t) ((X + kBX - 1) / kBX);
    A.bricks_y = (uint32_t) ((Y + kBY - 1) / kBY);
    const uint64_t bricks = (uint64_t) A.bricks_x * A.bricks_y * (uint64_t) ((Z + kBZ - 1) / kBZ);
    const uint64_t per_xcd = (bricks + kXcds - 1) / kXcds;
    if (per_xcd * kXcds > 0x7fffffffull) return hipErrorInvalidValue;
    A.n_bricks = (uint32_t) bricks; A.per_xcd = (uint32_t) per_xcd;
    float longest = 0.0f;
    for (int a = 0; a < 3; ++a) {
        A.bmin[a] = bbox_min[a];
        A.ext[a] = bbox_max[a] - bbox_min[a];
        if (A.ext[a] > longest) longest = A.ext[a];
    }
    A.near = 1e-3f * longest;
    A.wide = ((uintptr_t) counts & 7u) == 0;
    hipLaunchKernelGGL(visual_hull_kernel, dim3((unsigned) (per_xcd * kXcds)), dim3(kHT), 0, stream, A);
    return hipGetLastError();
}

hipError_t launch_adam_step_masked(float *p, const float *g, float *m, float *v, uint64_t n_voxels, int channels, const uint8_t *support,
                                   bool skip_zero_grad, double b1, double b2, double eps, double lr_t, float lo, float hi, hipStream_t stream)
{
    if (n_voxels == 0) return hipSuccess;
    AdamArgs A;
    A.p = p; A.g = g; A.m = m; A.v = v; A.support = support;
    A.n = n_voxels * (uint64_t) channels; A.channels = (uint32_t) channels; A.skip_zero = skip_zero_grad ? 1 : 0;    // (1 - beta in double, THEN to float, as launch_adam_step forms them)
    A.b1 = (float) b1; A.a1 = (float) (1.0 - b1); A.b2 = (float) b2; A.a2 = (float) (1.0 - b2);
    A.eps = (float) eps; A.lr_t = (float) lr_t; A.lo = lo; A.hi = hi;
    const bool vec = (((uintptr_t) p | (uintptr_t) g | (uintptr_t) m | (uintptr_t) v) & 15u) == 0;
    const uint64_t items = vec ? (A.n + 3) / 4 : A.n;
    const unsigned blocks = (unsigned) ((items + 255) / 256 < 16384 ? (items + 255) / 256 : 16384);
    if (vec) adam_masked_dispatch<true>(A, blocks, stream);
    else adam_masked_dispatch<false>(A, blocks, stream);
    return hipGetLastError();
}

}  // namespace drt
