// drt_nerf_dist.hip -- NeRFIntegrator.sample with opacity, depth and a third output that depends on sigma_t only: the distortion regulariser
// of mip-NeRF 360 in its O(N) form (DVGO v2), the tool against floaters and semi-transparent fog ALONG the ray:
//
//     Z = sum_i sum_j w_i w_j |tau_i - tau_j|  +  (1/3) sum_i w_i^2 dt_i          over the non-last queries, in world units of length (like D)
//
// w_j = weight_j = (1 - a_j) T_j, tau_j = t_in + t_b,j, dt_j the query's step - the march's own variables (drt_nerf_kernel.h).  A ray that
// misses the box has Z = 0.  Every per-ray and per-pixel buffer holds six interleaved floats [r, g, b, A, D, Z]; the first five are the bits of
// the opacity / depth calls (drt_nerf_aov.hip).  Z is quadratic in the weights, which never leave the kernel: it cannot be composed from the
// other outputs, it has to be integrated in the march.
//
// Primal, one pass in query order; W = weights_sum and Dp = depth_sum as they stand BEFORE query j is added, every operation rounded to fp32
// (-ffp-contract=off):
//     tau = t_in + t_b;  m = tau * W;  m = m - Dp;  m = 2 * m;  s = w_j * dt_j;  s = s / 3;  Z = Z + w_j * (m + s)
// A query the occupancy mask skips has w = 0 and changes none of Z, W, Dp.
// Adjoint: dZ/dw_j = 2 sum_i w_i |tau_j - tau_i| + (2/3) w_j dt_j = 2 (tau_j (2 W - A_in) - (2 Dp - D_in)) + (2/3) w_j dt_j, the totals from L_in.
// Times dZ it joins the "emission" q_j of the opacity / depth term: q = (dA + dD tau_j) + q_Z; the sigma_t splat is that term's, unchanged.
// Z is homogeneous of degree 2 in the weights, sum_i w_i dZ/dw_i = 2 Z (Euler), so the running remainder S starts from the primal's own output:
//     S = (dA A_in + dD D_in) + (2 dZ) Z_in
// Forward mode: dZ += dw_j (2 (tau W - Dp) + ((2/3) w_j) dt_j) + (2 w_j) (tau dW - dDp), dW and dDp the prefixes' tangents.
//
// Kernels - the march exists once, in the shared headers; this unit instantiates it with AOV = true and a policy that carries kDist = true
// (DistEmission / DistWindow; the template parameter lists, and with them every other unit's instantiations, are untouched):
//   nerf_kernel<DistEmission, false, false, false, true>      primal, one ray per lane, with the occupancy skip                (drt_nerf_kernel.h)
//   nerf_kernel<DistEmission, true, false, DEFER, true>       adjoint of EXPLICIT ray batches: the record route, or - without record memory - atomics
//   nerf_fwd_kernel<DistEmission, true>                       forward mode: one write per ray, no atomics: repeats bit for bit
//   nerf_tile_adjoint_kernel<DistWindow<.>, true>             adjoint of SENSOR rays - the hot path: the LDS window of the opacity / depth kernel
//                                                             (same window, planes and LDS bytes), five more floats per ray (dZ, A_in, D_in, W, Dp)
//   nerf_tile_bounds_aov_kernel<6>                            max |dZ|, max |Z_in| -> bounds words 12, 13
// The film: launch_film_develop_n / launch_film_backward_n (drt_nerf_aov.hip) with 6 channels.
#include "drt_device.h"
#include "drt_launch.h"
#include "drt_nerf_kernel.h"
#include "drt_nerf_tile_kernel.h"

namespace drt {

// this unit's cells of the three nerf launchers (no counting kernels: drt_get_counters does not count these calls)
template struct NerfLaneUnit<NerfOut::kDist, false>;
template struct NerfTileUnit<NerfOut::kDist>;

}  // namespace drt
