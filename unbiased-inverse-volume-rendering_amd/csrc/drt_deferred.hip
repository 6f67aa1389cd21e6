// drt_deferred.hip -- deferred, tile-binned gradient splatting for the adjoint pass.
//
// The adjoint tracer emits ~14 trilinear splats per ray (volpathsimple.py:170,489,580,594,607).  As
// global fp32 atomics they cost one L2 atomic request per splat and plane, and the chip retires only
// ~21 G requests/s: 8.6 of the adjoint's 21.8 ms.  Here the tracer appends
// records to two streams instead (emit_record, drt_device.h) - stream 0: 16 bytes {p, g_sigma_t}; stream 1:
// 32 bytes {p, g_sigma_t, g_r, g_g, g_b} for the splats that carry all four channels at one point (scatter
// events, nerf queries) - and this file turns them into gradients with streaming passes only:
//
//   bin_histogram  records -> per-(workgroup, tile) counts            (LDS histogram)
//   bin_offsets    counts  -> exclusive offsets, tile bases, reduce units
//   bin_scatter    records -> tile-sorted copy: a workgroup sorts each batch of 2048 records by tile in LDS and writes one run per tile,
//                  consecutive lanes to consecutive slots (bin_scatter_staged_kernel).  Grids of more than 2368 tiles,
//                  whose cursors leave no room for the stage: one store per record from LDS cursors (bin_scatter_kernel)
//   tile_reduce    workgroups walk runs of <= kUnitRecords-record units of ONE tile and ONE gradient plane
//                  (stream 0 -> sigma_t; stream 1 -> sigma_t, r, g, b: four passes over the sorted records, which
//                  stay in the memory-side cache): trilinear weights recomputed (same axis_setup / stencil_weights
//                  as the lookup), 8 LDS adds per record into a (32+1)x(16+1)x(16+1) tile, then one coalesced
//                  flush of the non-zero tile entries into the caller's gradient grid (+=, fp32 atomics: ~10^7
//                  per launch instead of ~10^9 lane-atomics).
//
// The LDS accumulators are 64-bit FIXED POINT: on gfx950 ds_add_f32 retires 0.2 T lane-atomics/s but
// ds_add_u64 3.4 T/s (tools/ubench/lds_atomic_rate.hip; the fp32 version of this kernel took 5.3 ms,
// 4.9 of them in ds_add_f32).  Every float product w*v is scaled by a power of two chosen from the
// plane's max |v| (found by the histogram pass) so that |w*v| * scale < 2^30 and rounded to an
// integer: quantisation 2^-31 max|v| per add, exact and order-independent sums inside a tile.
// A non-finite value poisons its plane's maximum: the tile then takes a float path that PROPAGATES the
// NaN / inf into the gradient exactly as the atomic path would (no silent clamping).
//
// A tile is addressed by the BASE corner cell of the splat, so its footprint is the tile plus a
// one-voxel apron on the high side.  The sigma_t values already carry the medium `scale`.  Sum order differs
// from the atomic path (as it does between two runs of the atomic path); the parity tolerance on gradients
// is unchanged.
#include <atomic>
#include "drt_device.h"
#include "drt_launch.h"

#ifndef DRT_PART_NT
#define DRT_PART_NT 5              // non-temporal accesses of the passes that stream the records: bit 0 the histogram's and the scatter's loads of the emitted records,
                                   // bit 2 tile_reduce's loads of stream 0's sorted records (read once; stream 1's are read by four planes and stay cached),
                                   // bit 1 the scatter's stores.  Measured, alternating runs on one box (headline Msamples/s / reductions ms; default = 0):
                                   // 0: 939-943 / 1.99   1: 948-962 / 1.82-1.95   4: 947 / 1.94   5: 955-960 / 1.76-1.88   2: 883 / 2.54   3: 886 / 2.52
                                   // - the loads leave the L2 to the scatter's open output lines; non-temporal STORES lose their write combining
                                   // The staged scatter (ms per headline step / reductions ms, two alternating runs): 5: 8.497 8.506 / 1.68   7: 8.737 8.764 / 1.93
                                   // - its runs still end inside lines that the workgroup's next batch completes: bit 1 stays off
#endif
#ifndef DRT_PART_UNROLL
#define DRT_PART_UNROLL 4
#endif
#ifndef DRT_PART_BATCH
#define DRT_PART_BATCH 2           // staged scatter: stream-0 records per thread and LDS batch (2: 32 KB of stage; 3 measured the same, 4 - one workgroup per CU - slower)
#endif
#ifndef DRT_PART_LDS_KB
#define DRT_PART_LDS_KB 64         // LDS budget of a staged scatter workgroup: the staged kernel is taken where cursors + counters + stage fit it
#endif
#ifndef DRT_PART_STAGED
#define DRT_PART_STAGED 1          // 0: bin_scatter_kernel for every grid
#endif

namespace drt {

namespace {

typedef float nt_f4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ float4 nt_load4(const float4 *p) { const nt_f4 v = __builtin_nontemporal_load((const nt_f4 *) p); return make_float4(v.x, v.y, v.z, v.w); }
__device__ __forceinline__ void nt_store4(float4 v, float4 *p) { nt_f4 w = { v.x, v.y, v.z, v.w }; __builtin_nontemporal_store(w, (nt_f4 *) p); }

constexpr int kLdsTile = (kTileX + 1) * (kTileY + 1) * (kTileZ + 1);

// Workgroup barrier AFTER no-return LDS atomics.  __syncthreads() alone compiles to a bare s_barrier here
// (the memory model treats LDS as in-order and waits for nothing), and the reads that follow were
// observed to overtake ds_add_u64 operations still in flight: a few records' worth of gradient lost per
// launch, one launch in ten.  Drain this wave's LDS queue first.
__device__ __forceinline__ void lds_atomics_barrier()
{
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __syncthreads();
}
constexpr int kPartUnroll = DRT_PART_UNROLL;   // chunks a partition thread keeps in flight
constexpr uint32_t kRideRecords = 4096;  // stream-1 records per tile that plane 0 takes along (a quarter of a reduce unit)
#ifndef DRT_REDUCE_WGS
#define DRT_REDUCE_WGS 512         // tile_reduce workgroups per plane, each a contiguous slice of the plane's reduce units: one round of the 2 x 256 that are resident at once.
                                   // A slice boundary inside a tile costs a second zero and flush of that tile.  Reductions ms per headline step, two alternating runs on
                                   // one box: 256: 1.542 1.539   512: 1.536 1.540 / 1.536 1.533   1024: 1.562 1.555   2048: 1.580 1.575
#endif
constexpr uint32_t kReduceWGs = DRT_REDUCE_WGS;

struct Cell { int x0, x1, y0, y1, z0, z1; float w[8]; };

// base corner cell + weights of a record position: the SAME arithmetic as the lookups / the atomic path
__device__ __forceinline__ void cell_of(const Params &P, float px, float py, float pz, int &x0, int &y0, int &z0)
{
    int i1; float w0, w1;
    axis_setup(px, P.bmin[0], P.inv_ext[0], P.rx, x0, i1, w0, w1);
    axis_setup(py, P.bmin[1], P.inv_ext[1], P.ry, y0, i1, w0, w1);
    axis_setup(pz, P.bmin[2], P.inv_ext[2], P.rz, z0, i1, w0, w1);
}

__device__ __forceinline__ int bin_of(const Params &P, const DeferredPlan &D, float4 r)
{
    int x0, y0, z0;
    cell_of(P, r.x, r.y, r.z, x0, y0, z0);
    return ((z0 / kTileZ) * D.nty + (y0 / kTileY)) * D.ntx + (x0 / kTileX);
}

// max |v| over finite values; a non-finite value returns +inf bits so that the plane is reduced on the
// propagating float path (tile_reduce)
__device__ __forceinline__ float plane_max(float vmax, float v)
{
    const float a = fabsf(v);
    if (!(a <= 3.0e38f)) return kInf;                            // inf or NaN
    return a > vmax ? a : vmax;
}

// part 0: every chunk; part 1: the chunks below the split (D.cursor[2 + S], launch_deferred_split) - what the adjoint
// tracer's main launch wrote -; part 2: the chunks from the split on, ADDED to part 1's counts
template <int S>
__device__ __forceinline__ void bin_histogram_stream(const Params &P, const DeferredPlan &D, uint32_t *h, int part)
{
    constexpr int kPlanes = S == 0 ? 1 : 4, kQuads = S == 0 ? 1 : 2;
    for (int b = threadIdx.x; b < D.n_bins; b += blockDim.x) h[b] = 0;
    __syncthreads();
    const uint32_t all = min(D.cursor[S], D.cap_chunks[S]), split = min(D.cursor[2 + S], all);
    const uint32_t lo = part == 2 ? split : 0u, used = part == 1 ? split : all;
    float vmax[kPlanes];
#pragma unroll
    for (int c = 0; c < kPlanes; ++c) vmax[c] = 0.0f;
    static_assert(kRecChunk == 256, "one record per thread and chunk");
    // chunk -> workgroup map (shared with the scatter pass): workgroup g owns chunks g*kSub + sub (mod stride)
    constexpr uint32_t kSub = kPartThreads / 256;                  // chunks a workgroup reads side by side
    const uint32_t sub = threadIdx.x >> 8, rec = threadIdx.x & 255u;
    for (uint32_t c0 = blockIdx.x * kSub + sub; c0 < used; c0 += kPartUnroll * kSub * gridDim.x) {
        float4 r[kPartUnroll], q[kPartUnroll]; bool ok[kPartUnroll];
#pragma unroll
        for (int k = 0; k < kPartUnroll; ++k) {                   // kPartUnroll chunks in flight per thread
            const uint32_t c = c0 + k * kSub * gridDim.x;
            ok[k] = c >= lo && c < used && rec < D.chunk_count[S][c];
            if (ok[k]) {
                const float4 *src = D.in[S] + ((size_t) c * kRecChunk + rec) * kQuads;
                r[k] = DRT_PART_NT & 1 ? nt_load4(src) : src[0];
                if constexpr (S == 1) q[k] = DRT_PART_NT & 1 ? nt_load4(src + 1) : src[1];
            }
        }
#pragma unroll
        for (int k = 0; k < kPartUnroll; ++k) {
            if (!ok[k]) continue;
            atomicAdd(&h[bin_of(P, D, r[k])], 1u);
            vmax[0] = plane_max(vmax[0], r[k].w);
            if constexpr (S == 1) { vmax[1] = plane_max(vmax[1], q[k].x); vmax[2] = plane_max(vmax[2], q[k].y); vmax[3] = plane_max(vmax[3], q[k].z); }
        }
    }
    __shared__ uint32_t wg_vmax[4];                              // one global atomic per workgroup and plane, not per wave
    if (threadIdx.x < 4) wg_vmax[threadIdx.x] = 0u;
    __syncthreads();
#pragma unroll
    for (int c = 0; c < kPlanes; ++c) {
        float v = vmax[c];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_down(v, off, 64));
        if ((threadIdx.x & 63) == 0 && v > 0.0f) atomicMax(&wg_vmax[c], __float_as_uint(v));
    }
    lds_atomics_barrier();
    if (threadIdx.x < kPlanes && wg_vmax[threadIdx.x]) atomicMax(D.vmax + (S == 0 ? 0 : 1) + threadIdx.x, wg_vmax[threadIdx.x]);
    uint32_t *dst = D.hist + ((size_t) S * gridDim.x + blockIdx.x) * D.n_bins;
    if (part == 2) { for (int b = threadIdx.x; b < D.n_bins; b += blockDim.x) dst[b] += h[b]; }
    else for (int b = threadIdx.x; b < D.n_bins; b += blockDim.x) dst[b] = h[b];
}

// per tile: exclusive prefix over the partition workgroups (in place) and the tile total.  One wave
// per (stream, tile): lane l owns workgroups [l * per, (l + 1) * per) - independent loads, a wave scan
// of the lane sums, independent stores.
__global__ void __launch_bounds__(256) bin_offsets_kernel(const DeferredPlan D, int n_wgs)
{
    const int lane = threadIdx.x & 63, s = blockIdx.y;
    const int b = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (b >= D.n_bins) return;
    uint32_t *col = D.hist + (size_t) s * n_wgs * D.n_bins + b;
    constexpr int kPer = kPartWGs / 64;
    uint32_t v[kPer], sum = 0;
#pragma unroll
    for (int k = 0; k < kPer; ++k) { v[k] = col[(size_t) (lane * kPer + k) * D.n_bins]; sum += v[k]; }
    uint32_t incl = sum;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) { uint32_t t = __shfl_up(incl, off, 64); if (lane >= off) incl += t; }
    uint32_t run = incl - sum;
#pragma unroll
    for (int k = 0; k < kPer; ++k) { col[(size_t) (lane * kPer + k) * D.n_bins] = run; run += v[k]; }
    if (lane == 63) D.bin_base[(size_t) s * (D.n_bins + 1) + b] = incl;      // total for now
}

#ifdef DRT_TEST_HOOKS
// kHookFewPartWGs: bin_offsets_kernel for a handful of partition workgroups, one row per lane (the production kernel's lanes own kPartWGs / 64 rows each)
constexpr int kFewPartWGs = 3;
static_assert(kFewPartWGs <= 64, "bin_offsets_few_kernel: one row per lane of a wave");
__global__ void __launch_bounds__(256) bin_offsets_few_kernel(const DeferredPlan D, int n_wgs)
{
    const int lane = threadIdx.x & 63, s = blockIdx.y;
    const int b = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (b >= D.n_bins) return;
    uint32_t *col = D.hist + (size_t) s * n_wgs * D.n_bins + b;
    const uint32_t v = lane < n_wgs ? col[(size_t) lane * D.n_bins] : 0u;   // (n_wgs <= 64: one row per lane)
    uint32_t incl = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) { uint32_t t = __shfl_up(incl, off, 64); if (lane >= off) incl += t; }
    if (lane < n_wgs) col[(size_t) lane * D.n_bins] = incl - v;
    if (lane == 63) D.bin_base[(size_t) s * (D.n_bins + 1) + b] = incl;      // total for now
}
#endif

// one workgroup per stream: exclusive scan of the tile totals -> bin_base, and of the reduce-unit counts
__global__ void __launch_bounds__(1024) bin_scan_kernel(const DeferredPlan D)
{
    __shared__ uint32_t sa[1024], sb[1024];
    const int s = blockIdx.x, t = threadIdx.x;
    uint32_t *base = D.bin_base + (size_t) s * (D.n_bins + 1);
    uint32_t *ustart = D.unit_start + (size_t) s * (D.n_bins + 1);
    const int per = (D.n_bins + 1023) / 1024;
    uint32_t tot[kMaxBins / 1024], ua = 0, ub = 0;
    for (int k = 0; k < per; ++k) {
        const int b = t * per + k;
        tot[k] = b < D.n_bins ? base[b] : 0u;
        ua += tot[k]; ub += (tot[k] + kUnitRecords - 1) / kUnitRecords;
    }
    sa[t] = ua; sb[t] = ub;
    __syncthreads();
    for (int off = 1; off < 1024; off <<= 1) {
        uint32_t a = t >= off ? sa[t - off] : 0u, b = t >= off ? sb[t - off] : 0u;
        __syncthreads();
        sa[t] += a; sb[t] += b;
        __syncthreads();
    }
    uint32_t ra = sa[t] - ua, rb = sb[t] - ub;                    // exclusive
    for (int k = 0; k < per; ++k) {
        const int b = t * per + k;
        if (b < D.n_bins) { base[b] = ra; ustart[b] = rb; }
        ra += tot[k]; rb += (tot[k] + kUnitRecords - 1) / kUnitRecords;
    }
    if (t == 1023) { base[D.n_bins] = sa[t]; ustart[D.n_bins] = sb[t]; }
}

// both streams in one launch (blockIdx.y): the small stream's workgroups fill the tail of the large one's
__global__ void __launch_bounds__(kPartThreads) bin_histogram_kernel(const Params P, const DeferredPlan D, int part)
{
    extern __shared__ uint32_t h[];
    if (blockIdx.y == 0) bin_histogram_stream<0>(P, D, h, part); else bin_histogram_stream<1>(P, D, h, part);
}

// snapshot of the chunk cursors: the chunks below it are complete once the launch that precedes this kernel has ended
__global__ void rec_split_kernel(const DeferredPlan D)
{
    if (threadIdx.x < kRecStreams) D.cursor[2 + threadIdx.x] = min(D.cursor[threadIdx.x], D.cap_chunks[threadIdx.x]);
}

template <int S>
__device__ __forceinline__ void bin_scatter_stream(const Params &P, const DeferredPlan &D, uint32_t *cur)
{
    constexpr int kQuads = S == 0 ? 1 : 2;
    const uint32_t *off = D.hist + ((size_t) S * gridDim.x + blockIdx.x) * D.n_bins;
    const uint32_t *base = D.bin_base + (size_t) S * (D.n_bins + 1);
    for (int b = threadIdx.x; b < D.n_bins; b += blockDim.x) cur[b] = base[b] + off[b];
    __syncthreads();
    const uint32_t used = min(D.cursor[S], D.cap_chunks[S]);
    float4 *dst = D.out[S];
    constexpr uint32_t kSub = kPartThreads / 256;
    const uint32_t sub = threadIdx.x >> 8, rec = threadIdx.x & 255u;
    for (uint32_t c0 = blockIdx.x * kSub + sub; c0 < used; c0 += kPartUnroll * kSub * gridDim.x) {   // same map as the histogram
        float4 r[kPartUnroll], q[kPartUnroll]; bool ok[kPartUnroll];
#pragma unroll
        for (int k = 0; k < kPartUnroll; ++k) { r[k] = make_float4(0.f, 0.f, 0.f, 0.f); q[k] = r[k]; }
#pragma unroll
        for (int k = 0; k < kPartUnroll; ++k) {
            const uint32_t c = c0 + k * kSub * gridDim.x;
            ok[k] = c < used && rec < D.chunk_count[S][c];
            if (ok[k]) {
                const float4 *src = D.in[S] + ((size_t) c * kRecChunk + rec) * kQuads;
                r[k] = DRT_PART_NT & 1 ? nt_load4(src) : src[0];
                if constexpr (S == 1) q[k] = DRT_PART_NT & 1 ? nt_load4(src + 1) : src[1];
            }
        }
        uint32_t slot[kPartUnroll];
#pragma unroll
        for (int k = 0; k < kPartUnroll; ++k) slot[k] = ok[k] ? atomicAdd(&cur[bin_of(P, D, r[k])], 1u) : 0u;
#pragma unroll
        for (int k = 0; k < kPartUnroll; ++k) if (ok[k]) {
            float4 *o = dst + (size_t) slot[k] * kQuads;
            if (DRT_PART_NT & 2) { nt_store4(r[k], o); if constexpr (S == 1) nt_store4(q[k], o + 1); }
            else { o[0] = r[k]; if constexpr (S == 1) o[1] = q[k]; }
        }
    }
}

__global__ void __launch_bounds__(kPartThreads) bin_scatter_kernel(const Params P, const DeferredPlan D)
{
    extern __shared__ uint32_t cur[];
    if (blockIdx.y == 0) bin_scatter_stream<0>(P, D, cur); else bin_scatter_stream<1>(P, D, cur);
}

// The staged scatter: a batch of kStageQuads float4s (kPartThreads x kPartBatch records of stream 0, half as many of stream 1) is sorted by
// tile in LDS and leaves as one contiguous run per tile, consecutive lanes writing consecutive 16-byte slots - the same (workgroup, tile)
// sub-ranges as bin_scatter_stream, the records of a batch in rank order instead of cursor-arrival order.
//   LDS: cur[n_bins] | cnt[n_bins] | dlt[n_bins] | wsum[64] | stage[kStageQuads] float4 | tid[kStageQuads] uint16  (staged_lds_bytes)
// Per batch: (1) rank = returning add on cnt[tile]; (2) exclusive scan of cnt over the tiles - thread t owns the bins [t * per, (t + 1) * per),
// a wave scan of the threads' sums and one cross-wave step -, which leaves start in cnt, dlt = cur - start, cur += count; (3) record -> stage[start
// + rank], its tile -> tid; (4) staged quad i -> global quad of record dlt[tile] + i / quads, and cnt[tile] = 0 again.  Barriers only.
constexpr int kPartBatch = DRT_PART_BATCH;                      // stream-0 records per thread and batch
static_assert(kPartBatch >= 2, "stream 1 takes half as many records per batch (rounded down)");
constexpr uint32_t kStageQuads = kPartThreads * kPartBatch;
constexpr int kPartWaves = kPartThreads / 64;
static_assert(kPartThreads % 64 == 0 && kPartWaves <= 64, "one cross-wave step");

__host__ __device__ constexpr size_t staged_words(int n_bins) { return ((size_t) 3 * n_bins + 64 + 3) & ~(size_t) 3; }   // cur, cnt, dlt, wsum: the stage behind them is 16-byte aligned
__host__ __device__ constexpr size_t staged_lds_bytes(int n_bins)
{
    return staged_words(n_bins) * sizeof(uint32_t) + (size_t) kStageQuads * (sizeof(float4) + sizeof(uint16_t));
}
// The host takes the staged kernel where its LDS fits this budget - a function of n_bins alone.  64 KB: two workgroups of kPartThreads = 1024
// threads fill a CU's 32 wave slots with 120 of its 160 KB (DESIGN.md section 6.7 has the occupancy arithmetic beside the overlapped tail launch)
constexpr size_t kStagedLdsBudget = (size_t) DRT_PART_LDS_KB << 10;
static_assert(DRT_PART_LDS_KB <= 64, "dynamic LDS beyond 64 KB needs hipFuncAttributeMaxDynamicSharedMemorySize on the kernel (the 78 and 96 KB batches measured that way were not kept)");
static_assert(kMaxBins <= 65536, "tile ids travel as 16 bits");

template <int S>
__device__ __forceinline__ void bin_scatter_staged_stream(const Params &P, const DeferredPlan &D, uint32_t *lds)
{
    constexpr int kQuads = S == 0 ? 1 : 2;
    constexpr int kRecs = kPartBatch / kQuads;                   // records per thread and batch (stream 1: the same bytes, rounded down)
    const int n_bins = D.n_bins;
    uint32_t *cur = lds, *cnt = lds + n_bins, *dlt = lds + 2 * n_bins, *wsum = lds + 3 * n_bins;
    float4 *stage = (float4 *) (lds + staged_words(n_bins));
    uint16_t *tid = (uint16_t *) (stage + kStageQuads);
    const uint32_t *off = D.hist + ((size_t) S * gridDim.x + blockIdx.x) * n_bins;
    const uint32_t *base = D.bin_base + (size_t) S * (n_bins + 1);
    for (int b = threadIdx.x; b < n_bins; b += blockDim.x) { cur[b] = base[b] + off[b]; cnt[b] = 0u; }
    __syncthreads();
    const uint32_t used = min(D.cursor[S], D.cap_chunks[S]);
    float4 *dst = D.out[S];
    constexpr uint32_t kSub = kPartThreads / 256;
    const uint32_t sub = threadIdx.x >> 8, rec = threadIdx.x & 255u;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const int per = (n_bins + kPartThreads - 1) / kPartThreads, b_lo = min((int) threadIdx.x * per, n_bins), b_hi = min(b_lo + per, n_bins);
    // Same chunk -> workgroup map as the histogram: this thread's chunks are first + sub + m * step, m = 0, 1, ...  A batch takes kRecs of them;
    // the next batch's records are in flight while this one is staged.  The loop bound is the WORKGROUP's (barriers inside): a thread's own
    // chunks end with okn[]
    const uint32_t first = blockIdx.x * kSub, step = kSub * gridDim.x;
    float4 rn[kRecs], qn[kRecs]; bool okn[kRecs];
    auto fetch = [&](uint32_t m0) {
#pragma unroll
        for (int j = 0; j < kRecs; ++j) {
            const uint32_t c = first + sub + (m0 + j) * step;
            okn[j] = c < used && rec < D.chunk_count[S][c];
            if (okn[j]) {
                const float4 *src = D.in[S] + ((size_t) c * kRecChunk + rec) * kQuads;
                rn[j] = DRT_PART_NT & 1 ? nt_load4(src) : src[0];
                if constexpr (S == 1) qn[j] = DRT_PART_NT & 1 ? nt_load4(src + 1) : src[1];
            }
        }
    };
    fetch(0u);
    for (uint32_t m0 = 0; first + m0 * step < used; m0 += kRecs) {
        float4 r[kRecs], q[kRecs]; int bin[kRecs]; uint32_t rank[kRecs];
        // (1) rank within the batch
#pragma unroll
        for (int j = 0; j < kRecs; ++j) {
            r[j] = rn[j];
            if constexpr (S == 1) q[j] = qn[j];
            bin[j] = okn[j] ? bin_of(P, D, r[j]) : -1;
            rank[j] = okn[j] ? atomicAdd(&cnt[bin[j]], 1u) : 0u;
        }
        fetch(m0 + kRecs);
        lds_atomics_barrier();
        // (2) exclusive scan of the batch counters over the tiles
        uint32_t sum = 0;
        for (int b = b_lo; b < b_hi; ++b) sum += cnt[b];
        uint32_t incl = sum;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) { const uint32_t t = __shfl_up(incl, o, 64); if (lane >= (uint32_t) o) incl += t; }
        if (lane == 63u) wsum[wave] = incl;
        __syncthreads();
        uint32_t w = lane < (uint32_t) kPartWaves ? wsum[lane] : 0u, winc = w;
#pragma unroll
        for (int o = 1; o < kPartWaves; o <<= 1) { const uint32_t t = __shfl_up(winc, o, 64); if (lane >= (uint32_t) o) winc += t; }
        const uint32_t total = __shfl(winc, kPartWaves - 1, 64);
        uint32_t run = __shfl(winc - w, (int) wave, 64) + incl - sum;
        for (int b = b_lo; b < b_hi; ++b) {
            const uint32_t c = cnt[b];
            if (c) { cnt[b] = run; dlt[b] = cur[b] - run; cur[b] += c; run += c; }
        }
        __syncthreads();
        // (3) records to their places in the stage
#pragma unroll
        for (int j = 0; j < kRecs; ++j) if (bin[j] >= 0) {
            const uint32_t pos = cnt[bin[j]] + rank[j];
            stage[pos * kQuads] = r[j];
            if constexpr (S == 1) stage[pos * kQuads + 1] = q[j];
            tid[pos] = (uint16_t) bin[j];
        }
        __syncthreads();
        // (4) the stage to the tiles' runs: consecutive lanes, consecutive 16-byte slots
        const uint32_t n_quads = total * kQuads;
#pragma unroll
        for (int j = 0; j < kPartBatch; ++j) {
            const uint32_t i = threadIdx.x + j * kPartThreads;
            if (i < n_quads) {
                const uint32_t rec_i = i / kQuads, t = tid[rec_i];
                float4 *o = dst + ((size_t) (dlt[t] + rec_i) * kQuads + (i % kQuads));
                if (DRT_PART_NT & 2) nt_store4(stage[i], o); else *o = stage[i];
                cnt[t] = 0u;
            }
        }
        __syncthreads();
    }
}

__global__ void __launch_bounds__(kPartThreads, 8) bin_scatter_staged_kernel(const Params P, const DeferredPlan D)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];   // the float4 stage behind the counters is written with 16-byte LDS stores
    if (blockIdx.y == 0) bin_scatter_staged_stream<0>(P, D, lds); else bin_scatter_staged_stream<1>(P, D, lds);
}

// blockIdx.y = reduce plane: 0: sigma_t of stream 0 AND of stream 1 (for every tile that has stream-0 records: the
// workgroup that starts such a tile's first unit also adds stream 1's sigma_t values of that tile - one zero / flush
// of the LDS tile instead of two); 1: sigma_t of stream 1 for the tiles WITHOUT stream-0 records; 2..4: r, g, b of stream 1
//
// A workgroup owns the reduce units [u_begin, u_end) of its plane's stream.  bin_base is a prefix sum and the units are consecutive, so
// these are ONE contiguous slice of the sorted records: the workgroup finds its first tile once (unit_tile), then walks forward - tile ends
// from bin_base, 64 entries per load where tiles are empty -, and only a tile boundary (flush, zero) interrupts the record loop.  That loop
// is software-pipelined: the loads of group n + 1 (four records per thread) are issued before the adds of group n, with clamped addresses
// instead of branches (a lane past its end re-reads the unit's last record and adds a zero), and it runs on across the unit boundaries
// inside a tile.  The body is compiled per plane kind (reduce_slice<KIND, FINITE>): no run-time choice of stream, quads or path per record.
#ifndef DRT_REDUCE_TRANSPOSE
#define DRT_REDUCE_TRANSPOSE 1     // 0: every unit in arrival order
#endif
#ifndef DRT_REDUCE_PLANE_ORDER
#define DRT_REDUCE_PLANE_ORDER 0   // 0: plane 0's workgroups (stream 0: four fifths of the records) are dispatched first; 1: last
#endif
#ifndef DRT_REDUCE_THREADS
#define DRT_REDUCE_THREADS 512      // (256: 1.15 ms per headline launch, 512 / 1024: 0.85 ms - more waves per CU behind the LDS tile)
#endif
constexpr int kKindS0 = 0, kKindS1Sigma = 1, kKindS1Colour = 2;   // stream 0 (one quad, non-temporal) | stream 1's sigma_t | stream 1's r, g or b
constexpr int kLdsRowBytes = (kTileX + 1) * 8, kLdsSlabBytes = (kTileX + 1) * (kTileY + 1) * 8;
typedef float rec_f3 __attribute__((ext_vector_type(3)));

// largest tile with ustart[tile] <= u (u < ustart[n_bins]): a 64-ary search, one load per lane and step - two dependent loads for 2048 tiles
__device__ __forceinline__ int unit_tile(const uint32_t *ustart, int n_bins, uint32_t u)
{
    const int lane = threadIdx.x & 63;
    int lo = 0, hi = n_bins;                                      // ustart[lo] <= u < ustart[hi]
    while (hi - lo > 1) {
        const int step = (hi - lo + 63) >> 6, idx = lo + lane * step;
        const bool le = idx < hi && ustart[idx] <= u;             // (lane 0 reads ustart[lo]: at least one lane holds)
        const int cnt = __popcll(__ballot(le));                   // ustart is non-decreasing: the lanes that hold are a prefix
        lo = __builtin_amdgcn_readfirstlane(lo + (cnt - 1) * step);
        hi = min(hi, lo + step);
    }
    return lo;
}

// one record {position, value}: 8 LDS adds of round(w * (val * scale)) - vs is val * scale, the power-of-two scale applied once per record,
// which gives the bits of (w * val) * scale wherever w * val is a normal number - or, on the non-finite path (vs is val), 8 float atomics
// into the caller's grid, as the atomic path does: NaN / inf propagate instead of being clamped away
template <bool FINITE>
__device__ __forceinline__ void add_record(const Params &P, unsigned long long *tile, float px, float py, float pz, float vs,
                                           int X0, int Y0, int Z0, float *dst, int stride)
{
    if (vs == 0.0f) return;                                       // adding exact zeros changes nothing
    Stencil st;
    axis_setup(px, P.bmin[0], P.inv_ext[0], P.rx, st.x0, st.x1, st.wx0, st.wx1);
    axis_setup(py, P.bmin[1], P.inv_ext[1], P.ry, st.y0, st.y1, st.wy0, st.wy1);
    axis_setup(pz, P.bmin[2], P.inv_ext[2], P.rz, st.z0, st.z1, st.wz0, st.wz1);
    float w[8];
    stencil_weights(st, w);
    if constexpr (!FINITE) {
        const int gx[2] = { st.x0, st.x1 }, gy[2] = { st.y0, st.y1 }, gz[2] = { st.z0, st.z1 };
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            const size_t vox = ((size_t) gz[c >> 2] * P.ry + gy[(c >> 1) & 1]) * P.rx + gx[c & 1];
            atomicAdd(dst + (size_t) stride * vox, w[c] * vs);
        }
    } else {
        // byte offsets into the LDS tile; the row and slab strides as 24-bit multiplies (full rate; the operands are below 2^6)
        const int x0 = (st.x0 - X0) << 3, x1 = (st.x1 - X0) << 3;
        const int y0 = __mul24(st.y0 - Y0, kLdsRowBytes), y1 = __mul24(st.y1 - Y0, kLdsRowBytes);
        const int z0 = __mul24(st.z0 - Z0, kLdsSlabBytes), z1 = __mul24(st.z1 - Z0, kLdsSlabBytes);
        const int o[8] = { z0 + y0 + x0, z0 + y0 + x1, z0 + y1 + x0, z0 + y1 + x1,
                           z1 + y0 + x0, z1 + y0 + x1, z1 + y1 + x0, z1 + y1 + x1 };
        char *tb = (char *) tile;
#pragma unroll
        for (int c = 0; c < 8; ++c)                               // |w * vs| < 2^30: round to nearest even, sign-extend
            atomicAdd((unsigned long long *) (tb + o[c]), (unsigned long long) (long long) __float2int_rn(w[c] * vs));
    }
}

template <int KIND, bool FINITE>
__device__ __forceinline__ void reduce_slice(const Params &P, const DeferredPlan &D, unsigned long long *tile, const int plane, const float vmax)
{
    constexpr int s = KIND == kKindS0 ? 0 : 1, quads = s == 0 ? 1 : 2;
    const int ch = KIND == kKindS1Colour ? plane - 1 : 0;        // channel of the record: 0 sigma_t, 1..3 r, g, b
    // scale = 2^(30 - e) with max|v| < 2^e: every product |w * v| * scale < 2^30 is rounded to a 32-bit integer (one
    // multiply + one conversion; the 64-bit route through double cost ~12 instructions per corner, i.e. most of this
    // kernel's VALU time) and sign-extended into the 64-bit accumulator, which holds 2^33 such adds.  Quantisation
    // 2^-31 max|v| per add (an fp32 atomic add rounds at 2^-24 of the running sum).  The two sigma_t planes share one
    // scale (plane 0 adds values of both streams)
    int e = 0;
    (void) frexpf(FINITE ? vmax : 1.0f, &e);
    const float scale = FINITE ? ldexpf(1.0f, 30 - e) : 1.0f;
    const double inv_scale = ldexp(1.0, e - 30);
    const int n_bins = D.n_bins, lane = threadIdx.x & 63;
    const uint32_t *base = D.bin_base + (size_t) s * (n_bins + 1);
    const uint32_t *ustart = D.unit_start + (size_t) s * (n_bins + 1);
    const uint32_t *base0 = D.bin_base, *base1 = D.bin_base + (n_bins + 1);
    const uint32_t n_units = ustart[n_bins];
    // persistent workgroups (empty ones are not free to dispatch), each a CONTIGUOUS run of units: the
    // units of a heavy tile follow one another, so the LDS tile is zeroed / flushed once per run
    const uint32_t u_begin = (uint32_t) (((uint64_t) n_units * blockIdx.x) / gridDim.x);
    const uint32_t u_end = (uint32_t) (((uint64_t) n_units * (blockIdx.x + 1)) / gridDim.x);
    if (u_begin >= u_end) return;                                 // no units at all for this workgroup
    float *dst = ch == 0 ? P.g_sigma : P.g_albedo + (ch - 1);
    const int stride = ch == 0 ? 1 : 3;
    const float4 *src = D.out[s];
    const uint32_t T = blockDim.x;

    int b = unit_tile(ustart, n_bins, u_begin);                   // the slice's first tile: it holds records
    uint32_t t_begin = base[b];
    uint32_t pos = t_begin + (u_begin - ustart[b]) * kUnitRecords;   // the slice is [pos, ...): n_left units, walked tile by tile
    uint32_t n_left = u_end - u_begin;

    // this thread's records of a unit [first, last): group g is a + (4 g + k) * step, k < 4, where that is below lim.  Arrival order: lane
    // after lane (a = first + thread, step = threads).  Transposed: one contiguous segment of n_rows records per thread
    uint32_t first = 0, last = 0, a = 0, step = 0, lim = 0, g = 0, n_groups = 0;
    auto unit_setup = [&](uint32_t f, uint32_t p_end, bool transposed) {
        first = f; last = p_end - f > kUnitRecords ? f + kUnitRecords : p_end;
        const uint32_t n_rows = (last - first + T - 1) / T;
        n_groups = (n_rows + 3) >> 2; g = 0;
        if (transposed) { a = first + threadIdx.x * n_rows; step = 1; lim = min(last, a + n_rows); }
        else { a = first + threadIdx.x; step = T; lim = last; }
    };
    // Records that arrive together may share their voxels - one march step of neighbouring nerf rays: 64 lanes on the same
    // LDS words, the adds serialise (nerf: 3.75 ms per plane and sub-batch).  Every wave looks at the unit's first 64 records
    // (the same records, so the same answer in every wave): when a quarter of them fall into their neighbour's cell the unit
    // is read TRANSPOSED - one contiguous segment per thread, so that the records a wave adds together lie n_rows apart in
    // arrival order (nerf 174 -> 203, fused nerf + DRT 142 -> 163 Msamples/s).  Scatter-event records do not (headline:
    // coalesced order 2.42 ms, transposed 2.66 ms).  The probe of a unit is loaded while the unit before it is reduced.
    auto probed = [&](uint32_t f, uint32_t p_end) { return DRT_REDUCE_TRANSPOSE && p_end - f >= 4096u; };   // (the unit [f, ...) holds >= 4096 records)
    auto probe_load = [&](uint32_t f) { return *(const rec_f3 *) (src + (size_t) (f + lane) * quads); };
    auto probe_eval = [&](const rec_f3 r) {
        int x0, y0, z0;
        cell_of(P, r.x, r.y, r.z, x0, y0, z0);
        const int id = (z0 * P.ry + y0) * P.rx + x0, left = __shfl_up(id, 1, 64);
        return __popcll(__ballot(lane > 0 && id == left)) >= 16;
    };
    // one group: four loads per thread, no branches and nothing that waits for them.  .w is the plane's value; bit k of the mask: record k is
    // this thread's to add (a lane past its end holds a copy of the unit's last record)
    auto load_group = [&](float4 (&r)[4], uint32_t &okm) {
        okm = 0u;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const uint32_t i = a + k * step;
            const bool ok = i < lim;
            const float4 *rp = src + (size_t) (ok ? i : last - 1u) * quads;
            if constexpr (KIND == kKindS1Colour) {
                const rec_f3 p = *(const rec_f3 *) rp;
                r[k] = make_float4(p.x, p.y, p.z, ((const float *) rp)[3 + ch]);
            } else r[k] = (DRT_PART_NT & 4) && KIND == kKindS0 ? nt_load4(rp) : rp[0];
            okm |= ok ? 1u << k : 0u;
        }
        a += 4 * step; ++g;
    };
    auto add_group = [&](const float4 (&r)[4], const uint32_t okm, int X0, int Y0, int Z0) {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            add_record<FINITE>(P, tile, r[k].x, r[k].y, r[k].z, (okm >> k) & 1u ? r[k].w * scale : 0.0f, X0, Y0, Z0, dst, stride);
    };

    while (n_left > 0) {
        // tile b holds the records [t_begin, t_end), the slice's next one is pos.  One load per lane: the ends of the tiles b .. b + 63 -
        // this tile's end and, past the empty tiles, the next tile with records
        int X0 = 0, Y0 = 0, Z0 = 0, b_next = -1;
        uint32_t t_end;
        {
            const uint32_t en = base[min(b + 1 + lane, n_bins)];
            t_end = __builtin_amdgcn_readfirstlane(en);
            const unsigned long long m = __ballot(en > t_end);
            if (m) b_next = b + (int) __ffsll(m) - 1;
        }
        const uint64_t want = (uint64_t) pos + (uint64_t) n_left * kUnitRecords;
        const uint32_t p_end = want < t_end ? (uint32_t) want : t_end;   // the slice's part of this tile: [pos, p_end), whole units or up to the tile's end
        n_left -= (p_end - pos + kUnitRecords - 1) / kUnitRecords;
        // stream 1's sigma_t values of tile b ride along with stream 0's when they are few (scatter events next to
        // the transmittance splats); when they are many (nerf queries) they keep their own plane and units
        bool ride = false;
        uint32_t r1_begin = 0, r1_end = 0;
        if constexpr (KIND == kKindS0) { r1_begin = base1[b]; r1_end = base1[b + 1]; ride = r1_end - r1_begin <= kRideRecords; }
        if constexpr (KIND == kKindS1Sigma) ride = base0[b + 1] > base0[b] && t_end - t_begin <= kRideRecords;
        const bool live = !(KIND == kKindS1Sigma && ride);       // the LDS tile will hold sums of tile b that must be flushed
        if (live) {
            rec_f3 probe = { 0.f, 0.f, 0.f };
            bool transposed = false;
            const bool probe_first = probed(pos, p_end);
            if (probe_first) probe = probe_load(pos);
            X0 = (b % D.ntx) * kTileX; Y0 = ((b / D.ntx) % D.nty) * kTileY; Z0 = (b / (D.ntx * D.nty)) * kTileZ;
            if constexpr (FINITE) {
                for (int j = threadIdx.x; j < kLdsTile; j += T) tile[j] = 0ull;
                __syncthreads();
            }
            if (KIND == kKindS0 && ride && pos == t_begin) {     // first unit of this tile: stream 1's sigma_t values come along
                const float4 *src1 = D.out[1];
                for (uint32_t i0 = r1_begin + threadIdx.x; i0 < r1_end; i0 += 4 * T) {
                    float4 r[4]; uint32_t okm = 0u;
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        const uint32_t i = i0 + k * T;
                        r[k] = src1[2 * (size_t) (i < r1_end ? i : r1_end - 1u)];
                        okm |= i < r1_end ? 1u << k : 0u;
                    }
                    add_group(r, okm, X0, Y0, Z0);
                }
            }
            if (probe_first) transposed = probe_eval(probe);
            unit_setup(pos, p_end, transposed);
            float4 nxt[4]; uint32_t nxt_ok;
            load_group(nxt, nxt_ok);
            bool probe_next = last < p_end && probed(last, p_end);
            if (probe_next) probe = probe_load(last);
            for (bool more = true; more; ) {
                float4 cur[4]; const uint32_t cur_ok = nxt_ok;
#pragma unroll
                for (int k = 0; k < 4; ++k) cur[k] = nxt[k];
                if (g == n_groups) {                              // the unit's last group is in cur: on to the next unit of this tile
                    if (last < p_end) {
                        unit_setup(last, p_end, probe_next && probe_eval(probe));
                        probe_next = last < p_end && probed(last, p_end);
                        if (probe_next) probe = probe_load(last);
                    } else more = false;
                }
                if (more) load_group(nxt, nxt_ok);
                add_group(cur, cur_ok, X0, Y0, Z0);
            }
            if (FINITE && !dbg(P.debug_flags, kHookReduceNoFlush)) {   // flush the finished tile (+=)
                lds_atomics_barrier();
                for (int j = threadIdx.x; j < kLdsTile; j += T) {
                    const long long q = (long long) tile[j];
                    if (q == 0) continue;
                    const float v = (float) ((double) q * inv_scale);
                    const int lx = j % (kTileX + 1), ly = (j / (kTileX + 1)) % (kTileY + 1), lz = j / ((kTileX + 1) * (kTileY + 1));
                    const size_t vox = ((size_t) (Z0 + lz) * P.ry + (Y0 + ly)) * P.rx + (X0 + lx);
                    atomicAdd(dst + (size_t) stride * vox, v);
                }
                __syncthreads();
            }
        }
        if (n_left == 0) break;
        // units are left, so the slice took this tile to its end and a later tile holds records: past a stretch of more than 63 empty
        // tiles, 64 tile ends per step
        for (int j = b + 64; b_next < 0 && j < n_bins; j += 64) {
            const unsigned long long m = __ballot(base[min(j + 1 + lane, n_bins)] > t_end);
            if (m) b_next = j + (int) __ffsll(m) - 1;
        }
        if (b_next < 0) break;                                    // (cannot happen: unit_start and bin_base come from the same counts)
        b = b_next; t_begin = t_end; pos = t_end;
    }
}

__global__ void __launch_bounds__(DRT_REDUCE_THREADS) tile_reduce_kernel(const Params P, const DeferredPlan D)
{
    extern __shared__ unsigned long long tile[];                 // kLdsTile signed 64-bit fixed-point accumulators
    const int plane = DRT_REDUCE_PLANE_ORDER ? 4 - (int) blockIdx.y : (int) blockIdx.y;
    const float vmax = plane <= 1 ? fmaxf(__uint_as_float(D.vmax[0]), __uint_as_float(D.vmax[1])) : __uint_as_float(D.vmax[plane]);
    if (vmax == 0.0f) return;                                    // nothing but zeros in this plane
    if (vmax <= 3.0e38f) {
        switch (plane) {
        case 0: reduce_slice<kKindS0, true>(P, D, tile, plane, vmax); break;
        case 1: reduce_slice<kKindS1Sigma, true>(P, D, tile, plane, vmax); break;
        default: reduce_slice<kKindS1Colour, true>(P, D, tile, plane, vmax); break;
        }
    } else {                                                     // a NaN / inf anywhere in the plane: the float path, a loop of its own
        switch (plane) {
        case 0: reduce_slice<kKindS0, false>(P, D, tile, plane, vmax); break;
        case 1: reduce_slice<kKindS1Sigma, false>(P, D, tile, plane, vmax); break;
        default: reduce_slice<kKindS1Colour, false>(P, D, tile, plane, vmax); break;
        }
    }
}

}  // namespace

hipError_t launch_deferred_split(const DeferredPlan &D, hipStream_t stream)
{
    hipLaunchKernelGGL(rec_split_kernel, dim3(1), dim3(64), 0, stream, D);
    return hipGetLastError();
}

// partition workgroups per stream (histogram, offsets, scatter).  kHookFewPartWGs: three, so that a test scene of a few thousand rays gives every
// workgroup several batches per stream - the carry of the cursors from batch to batch
inline int part_wgs(const Params &P)
{
#ifdef DRT_TEST_HOOKS
    if (dbg(P.debug_flags, kHookFewPartWGs)) return kFewPartWGs;
#endif
    (void) P;
    return kPartWGs;
}

hipError_t launch_deferred_early_histogram(const Params &P, const DeferredPlan &D, hipStream_t side)
{
    const size_t lds = (size_t) D.n_bins * sizeof(uint32_t);
    hipLaunchKernelGGL(bin_histogram_kernel, dim3(part_wgs(P), kRecStreams), dim3(kPartThreads), lds, side, P, D, 1);
    return hipGetLastError();
}

// phase 0: everything; 1: the partition only (histogram, offsets, scan, scatter: the passes that do not touch the caller's gradient grids - the
// queued tracer runs them on a side stream beside its tail launch); 2: tile_reduce only (the partition has been made)
hipError_t launch_deferred_reduce(const Params &P, const DeferredPlan &D, hipStream_t stream, hipEvent_t *ev, bool early_hist, int phase)
{
    const size_t lds = (size_t) D.n_bins * sizeof(uint32_t);
    auto mark = [&](int k) { if (ev) (void) hipEventRecord(ev[k], stream); };
    mark(0);
    if (phase != 2) {
        const int wgs = part_wgs(P);
        hipLaunchKernelGGL(bin_histogram_kernel, dim3(wgs, kRecStreams), dim3(kPartThreads), lds, stream, P, D, early_hist ? 2 : 0);
        mark(1);
#ifdef DRT_TEST_HOOKS
        if (wgs != kPartWGs) hipLaunchKernelGGL(bin_offsets_few_kernel, dim3((D.n_bins + 3) / 4, kRecStreams), dim3(256), 0, stream, D, wgs);
        else
#endif
        hipLaunchKernelGGL(bin_offsets_kernel, dim3((D.n_bins + 3) / 4, kRecStreams), dim3(256), 0, stream, D, kPartWGs);
        hipLaunchKernelGGL(bin_scan_kernel, dim3(kRecStreams), dim3(1024), 0, stream, D);
        mark(2);
        // the staged scatter where its cursors, counters and stage fit the LDS budget - a function of n_bins alone (the headline's 2048 tiles: 60.25 KB;
        // beyond 2368 tiles, 512^3 among them: the per-record scatter, whose cursors alone take up to 64 KB)
        const size_t staged = staged_lds_bytes(D.n_bins);
        if (DRT_PART_STAGED && staged <= kStagedLdsBudget) {
            hipLaunchKernelGGL(bin_scatter_staged_kernel, dim3(wgs, kRecStreams), dim3(kPartThreads), staged, stream, P, D);
        } else
            hipLaunchKernelGGL(bin_scatter_kernel, dim3(wgs, kRecStreams), dim3(kPartThreads), lds, stream, P, D);
        mark(3);
    }
    if (phase == 1) return hipGetLastError();
    {   // (the attribute belongs to the function on a device: set once per device)
        static std::atomic<bool> attr_set[64];                   // (zero-initialised; handles may be driven from several host threads)
        int dev = 0;
        if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) dev = 63;
        if (!attr_set[dev] || dev == 63) {
            const hipError_t attr = hipFuncSetAttribute((const void *) tile_reduce_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, kLdsTile * 8);
            if (attr != hipSuccess) return attr;
            attr_set[dev] = true;
        }
    }
    uint32_t wgs = D.max_units < kReduceWGs ? D.max_units : kReduceWGs;
#ifdef DRT_TEST_HOOKS
    if (dbg(P.debug_flags, kHookFewPartWGs)) wgs = kFewPartWGs;  // a small scene's slices then span units and tiles (a workgroup without units returns)
#endif
    hipLaunchKernelGGL(tile_reduce_kernel, dim3(wgs, 5), dim3(DRT_REDUCE_THREADS), (size_t) kLdsTile * 8, stream, P, D);
    mark(4);
    return hipGetLastError();
}

}  // namespace drt
