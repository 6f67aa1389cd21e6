// drt_own.hip -- the kernels for scenes whose COLOUR grids (albedo; the nerf integrator's emission) live on their own lattice
// (drt_set_colour_resolution): Mitsuba interpolates every GridVolume on its own resolution, and the reference's janga-smoke pairs a
// 264 x 136 x 136 density with 256 x 128 x 128 albedo / emission grids (python/scene_config.py:108-110).
//
// The OWN = true cells (as in the _hg, _hg2 and _tab flavours): eval_rgb<true> builds its stencil from Params::crx / cry / crz and the colour gradient
// splats go to the caller's grid as fp32 atomics on that lattice (drt_device.h: make_stencil_colour<true>, splat_colour_own), because the tile
// partition, the LDS reduction tiles and the apron scratch are laid out on sigma_t's lattice.  Everything else - the wave-cooperative tracer
// with a global majorant, its own-lane walk through a majorant supergrid, path cache, sigma_t record streams, every estimator, both emitters,
// the nerf march - is the code of the other units, instantiated here once more with the lattice as a template argument.  A scene with equal lattices never gets
// here: its kernels, and the benchmark, are untouched by this unit.  Parity: tests/test_gpu_lattice.py against the oracle.
#include "drt_coop_kernel.h"
#include "drt_nerf_kernel.h"

namespace drt {

template struct CoopUnit<Phase::kIso, false, true>;
template struct CoopUnit<Phase::kIso, true, true>;
template struct NerfLaneUnit<NerfOut::kPlain, true>;

}  // namespace drt
