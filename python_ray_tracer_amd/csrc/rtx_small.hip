// rtx_small.hip — the k_render_fast instantiations of scenes below kTreeMinSpheres (TP 0: no culling
// tree, no persistent loop; the README and main.py scenes, BASELINE configs C1/C2), in a translation
// unit of their own: they compile beside the culled kernels of rtx_kernels.hip, not after them, and
// an A/B can give them flags of their own (_build.SMALL_FLAGS). The launch sites in rtx_kernels.hip
// call rtx_launch_small.
#include "rtx_device.h"
#include "rtx_internal.h"

namespace {

template <int B, int DEEP, bool STATS, bool IMG = false, int NSPH = 0>
hipError_t go(const void* params, dim3 grid, uint32_t lds, hipStream_t s, hipEvent_t e0, hipEvent_t e1) {
  Params p = *static_cast<const Params*>(params);
  p.tile_div = grid.x > 1 ? (uint32_t)((uint64_t(1) << 32) / grid.x) : 0xFFFFFFFFu;  // small_wave's tile_order division
  rtx_note_launch(B, true, DEEP, STATS, 0, IMG, NSPH, 0, grid, p.n_fetch, p.tile_order != nullptr, lds);
  hipExtLaunchKernelGGL((k_render_fast<B, true, DEEP, STATS, 0, IMG, NSPH>), grid, dim3(fast_block<false>()), lds, s,
                        e0, e1, 0u, p);
  return hipSuccess;  // launch errors reach the caller's check_launch through hipGetLastError
}

// The kernels without counters or image textures (the timed capped ones and the DEEP ones of
// unbounded renders) of each sphere count below kTreeMinSpheres, with the count a compile-time
// constant (fast_tile's NSPH: the sphere loops unroll; A/B r6b, C2 -2.7%); the counter and
// texturing kernels keep the run-time count.
template <int B, int DEEP>
hipError_t go_ns(const void* params, dim3 grid, uint32_t lds, hipStream_t s, hipEvent_t e0, hipEvent_t e1) {
  static_assert(kTreeMinSpheres == 8, "one instantiation per sphere count 1..7");
  switch (static_cast<const Params*>(params)->nsph) {
    case 1: return go<B, DEEP, false, false, 1>(params, grid, lds, s, e0, e1);
    case 2: return go<B, DEEP, false, false, 2>(params, grid, lds, s, e0, e1);
    case 3: return go<B, DEEP, false, false, 3>(params, grid, lds, s, e0, e1);
    case 4: return go<B, DEEP, false, false, 4>(params, grid, lds, s, e0, e1);
    case 5: return go<B, DEEP, false, false, 5>(params, grid, lds, s, e0, e1);
    case 6: return go<B, DEEP, false, false, 6>(params, grid, lds, s, e0, e1);
    case 7: return go<B, DEEP, false, false, 7>(params, grid, lds, s, e0, e1);
    default: return go<B, DEEP, false>(params, grid, lds, s, e0, e1);
  }
}

// the (stats, img) instantiations launch_fast_b can request for a scene below kTreeMinSpheres: the
// counter kernels, the capped counter-free texturing kernels, and the timed ones (go_ns)
template <int B, int DEEP>
hipError_t go_b(bool stats, bool img, const void* params, dim3 grid, uint32_t lds, hipStream_t s, hipEvent_t e0,
                hipEvent_t e1) {
  if (img) {  // image textures shaded in place: capped, counter-free launches only
    if constexpr (DEEP) return hipErrorInvalidValue;
    else return stats ? hipErrorInvalidValue : go<B, DEEP, false, true>(params, grid, lds, s, e0, e1);
  }
  return stats ? go<B, DEEP, true>(params, grid, lds, s, e0, e1) : go_ns<B, DEEP>(params, grid, lds, s, e0, e1);
}

}  // namespace

hipError_t rtx_launch_small(int B, int deep, bool stats, bool img, const void* params, dim3 grid, uint32_t lds,
                            hipStream_t s, hipEvent_t e0, hipEvent_t e1) {
  if (deep) {  // 1: an uncapped render's first pass, 2: its continuation pass
    if (B != kDeepLevels) return hipErrorInvalidValue;
    return deep == 2 ? go_b<kDeepLevels, 2>(stats, img, params, grid, lds, s, e0, e1)
                     : go_b<kDeepLevels, 1>(stats, img, params, grid, lds, s, e0, e1);
  }
  switch (B) {
    case 0: return go_b<0, false>(stats, img, params, grid, lds, s, e0, e1);
    case 1: return go_b<1, false>(stats, img, params, grid, lds, s, e0, e1);
    case 2: return go_b<2, false>(stats, img, params, grid, lds, s, e0, e1);
    case 3: return go_b<3, false>(stats, img, params, grid, lds, s, e0, e1);
    case 4: return go_b<4, false>(stats, img, params, grid, lds, s, e0, e1);
    case 5: return go_b<5, false>(stats, img, params, grid, lds, s, e0, e1);
    case 6: return go_b<6, false>(stats, img, params, grid, lds, s, e0, e1);
    default: return hipErrorInvalidValue;
  }
}
