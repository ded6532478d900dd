// rtx_device.h — the device text that more than one translation unit of librtx_hip.so compiles:
// the tuning constants, Params, every __device__ helper of the render path and the k_render_fast
// templates (emitted only where a unit instantiates them). No kernel that is not a template lives
// here: each of those is defined, and so emitted, in the one unit that launches it.
//
// One thread = one ray (one pixel in camera mode); 64-lane waves cover 8x8 pixel tiles so the
// rays of a wave stay coherent through the bounce chain. All geometry is float64 (SURVEY.md §7
// hard part 1: the R=99999 ground sphere flips checker cells in fp32) and every expression keeps
// the reference's operation order (file:line cited at each step); the library is compiled with
// -ffp-contract=off because NumPy never fuses a multiply into an add.
//
//   k_render_fast<B, LDS, DEEP>  The reference's recursion
//                     raytrace_scene -> create -> _calculate_reflection -> raytrace_scene
//                     (base.py:91-121, shader.py:63-161) becomes an in-register loop over bounce
//                     levels that accumulates the chain's colour forwards: every level adds its own
//                     colour with a black reflection, weighted by the chain's throughput
//                         col = sum_k T_k L_k,  T_0 = 1,  T_{k+1} = (T_k * 0.5) * g_k
//                     (shader.py:106-110 reassociated), so nothing is kept per level. Sphere geometry
//                     is read by the wave-uniform loops through the scalar cache (s_load); the per-lane
//                     hit-sphere/material records come from an LDS copy of the scene table (LDS = S <=
//                     kLdsMaxSpheres). Scenes of >= 8 spheres carry a tree of boxes that the loops walk
//                     wave-uniformly (exact culling). Tile rows are dispatched bottom-up (longest work
//                     first). A cap B <= RTX_FAST_MAX_BOUNCES ends the chain at level B (DEEP 0). Under
//                     a larger cap or none, the DEEP first pass (DEEP 1) follows a chain to level
//                     kFirstPassLevels (30) and defers what is still alive with a resume record; one
//                     continuation pass (DEEP 2) takes those chains on to level kDeepLevel3 (60) and
//                     defers again. A ray that meets a tie (two shapes at the same nearest distance,
//                     base.py:103 — both get shaded and summed) is appended to the deferred list too.
#pragma once

#include <hip/hip_ext.h>
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <type_traits>

#include "../../include/rtx_hip.h"
#include "rtx_internal.h"

#define FARAWAY 1.0e39  // base.py:12
#define RTX_PI 3.141592653589793  // np.pi

namespace {

constexpr int kBlock = 256;   // threads per block of the elementwise boundary kernels
// ---- tuning constants (each value chosen by an A/B on identical output, profiles/r1_ab_variants.txt;
// tools/ab_build.py builds variants by rewriting these lines) ----
constexpr int kWaveW = 8;       // pixels per wave row: a wave renders a kWaveW x (64 / kWaveW) tile
// ... in scenes below kTreeMinSpheres (the TREE = false kernels; A/B profiles/r3_ab_variants.txt r3x-r3z:
// C2 -0.8%, C2main -1.1%, C1 -6%; the culled kernels keep 8 x 8: C5 +0.6%, C4 +3% at 16 x 4, the
// wave frustum and beam bounds are tighter on square tiles)
constexpr int kWaveWSmall = 16;
constexpr int kFastWaves = 4;   // waves per k_render_fast block (1, 2 or 4) of the culled kernels
// ... and of the TREE = false kernels (scenes below kTreeMinSpheres): one wave per block, so the
// hardware hands out single 16x4 wave tiles in the learnt longest-first order (rtx_render_camera_sched;
// A/B r4f, C2: 52.8 against 54.5 us per frame with four-wave blocks, 54.7 / 55.7 without the order)
constexpr int kFastWavesSmall = 1;
// k_render_fast single-frame launches of scenes with at least this many spheres: persistent waves
// fetching wave tiles (A/B: 65 spheres -14%, 17 spheres +-0, 3-16 spheres without the culling tree
// +12%: their tiles are short, so the ramp-up of the fetch counters and the drain cost more than
// the balancing gains)
constexpr int kPersistMinSpheres = 32;
constexpr int kMaxFetch = 32;   // tile counters (one 128-byte line each) shared round-robin by the waves
// general-kernel threads: ties only (caps <= RTX_FAST_MAX_BOUNCES; an empty launch costs more with
// more blocks), or ties and deep chains (A/B for unbounded renders: 4096, 16384, 65536)
constexpr int kDeferredWorkers = 4096;
constexpr int kDeepWorkers = 16384;
constexpr int kDeepWaves = 4;        // waves/SIMD of the persistent DEEP kernel (with the beam at 3 its persistent kernel takes
                                     // 134 VGPRs; at 4, 128: A/B r6ap, unbounded C4 -14%)
constexpr int kDeepWavesTile = 5;    // ... of the one-tile first passes (TP 1 and 0; A/B r6ar, unbounded: C3 -5.1%,
                                     // C2 -2.0%, C2main -5.0% against 4, the persistent C4 +-0)
// Every kernel accumulates the bounce chain's colour forwards, col = sum_k T_k L_k with T_0 = 1,
// T_{k+1} = (T_k * 0.5) * g_k and L_k level k's colour with a black reflection, instead of storing
// every non-terminal level's colour inputs and folding them back from the deepest level (the
// reference's association, shader.py:106-110: col_k = ((A_k + (spec_k + col_{k+1} * 0.5) * g_k) +
// I_k)). Same terms, reassociated: the result moves by a few ulp of the colour (<= ~1e-13 absolute
// at the brightest unclipped values, under the 1e-12 parity bar), and no level's inputs live in LDS
// or registers across the chain. A/B r5c against the backward fold (one box, tools/ab.py, frames
// identical): C2 55.20 -> 52.94 us (-4.1%), C4 2,055 -> 1,874 us (-8.8%: 41 spilled VGPRs -> 0),
// C3 273.1 -> 265.7 us (-2.7%, at 5 waves/SIMD; 283.9 at 4)
constexpr int kFwdWavesPersist = 4;  // waves/SIMD of the capped persistent kernels (TP 2; C4: 5 waves 2,025 us)
constexpr int kFwdWaves = 5;         // ... of the culled one-tile-per-block kernels (TP 1; C3: 4 waves 283.9 us)
// ... and of their launches of at least kWavesLargeMinPixels pixels (A/B r6aw, 6 waves against 5: C3 (8.3 M
// pixels) -3.3%, C5's 32-frame launches -3.5%, but one 1080p frame of C5's scene +4%: 80 VGPRs spill)
constexpr int kFwdWavesLarge = 6;
constexpr int64_t kWavesLargeMinPixels = int64_t(4) << 20;
constexpr int kFwdWavesSmall = 5;    // ... and of the TREE = false kernels (TP 0; C2: 6 waves 56.0 us, spills)
constexpr int kDeepLevels = 5;       // fast-kernel levels before a longer chain is deferred (A/B: 3, 5, 8; the
                                     // 8-level instantiation spills, 3 defers too many pixels)
constexpr int kCappedMax = RTX_FAST_MAX_BOUNCES;  // caps rendered entirely by k_render_fast<cap>
// Shading-only terms (the view vector, the half vector and the specular's internal divisions and
// square roots; none of them decides a hit, a shadow, a checker cell or a reflected ray): the
// specular's divisions and square roots take shorter Newton sequences (within ~1 ulp,
// tools/approx_probe), V and H are normalised by the correctly rounded cores (div_shade, sqrt_shade,
// inv_mag_shade; A/B on identical parity against the correctly rounded cores throughout: C2 -6.4%,
// C2main -8.5%, C5 -2.9%, C3 -2.8%).
// The small-scene wave (small_wave, TP 0; profiles/optimistic_C2_ab.json, C2 50.05 -> 47.81 us with
// both): the counter-free capped builds run an optimistic first body, one guard verdict per wave
// instead of a ballot and a branch per helper (alone -3.4%); and the sphere table is requested with
// the header words and held in registers until the level-0 search has found a hit, so an all-sky wave
// never waits for it (alone -3.1%).
// Wave-uniform terms kept out of the vector unit (profiles/uniform_terms_C2.json, identical frames):
// the level-0 search of the small-scene kernels takes camera - centre and the sign of the camera's c
// from the packer's table (RTX_H_CAMREL) instead of three subtractions of scalars per sphere and lane;
// and in their camera ray a wave whose tile ends before the frame's last column and row (a scalar
// decision from the tile's position) computes the linspace points without the stop-word selects, the
// fix words of the others being tested by their bits (f64_nonzero_bits: a scalar test where the
// compare of doubles is a vector instruction; same verdict for every double). The latter relies on one
// wave tile per block (a static_assert in fast_tile_body ties it to kFastWavesSmall = 1).
// (Built, measured and taken out again, profiles/uniform_terms_C2.json: the sine's polynomial with its
// coefficients as scalar operands of v_fma_f64, and the header's counts read as bit patterns. Neither
// moved C2's time, and with both the culled kernels, which share shade, lost 0.3-0.6%.)
// ---- derived ----
constexpr int kWaveH = 64 / kWaveW;
static_assert(kFastWaves == 1 || kFastWaves == 2 || kFastWaves == 4, "kFastWaves");
static_assert(kFastWavesSmall == 1 || kFastWavesSmall == 2 || kFastWavesSmall == 4, "kFastWavesSmall");
static_assert((kMaxFetch & (kMaxFetch - 1)) == 0, "kMaxFetch must be a power of two");
constexpr int kFastBlock = 64 * kFastWaves;
constexpr int kWavesX = kFastWavesSmall == 1 ? 1 : 2;  // block tile of the small kernels: kWavesX x kWavesY waves
constexpr int kWavesXTree = kFastWaves;  // ... of the culled kernels: one row of waves (A/B r3o: C5 -3.0%, C3 +-0.3%; C1 +9% for the small ones)
static_assert(kWaveWSmall > 0 && kWaveWSmall <= 64 && 64 % kWaveWSmall == 0, "kWaveWSmall");
template <bool TREE>
__host__ __device__ constexpr int wave_w() { return TREE ? kWaveW : kWaveWSmall; }
template <bool TREE>
__host__ __device__ constexpr int waves_x() { return TREE ? kWavesXTree : kWavesX; }
template <bool TREE>
__host__ __device__ constexpr int fast_waves() { return TREE ? kFastWaves : kFastWavesSmall; }
template <bool TREE>
__host__ __device__ constexpr int fast_block() { return 64 * fast_waves<TREE>(); }
static_assert(kFastWavesSmall % kWavesX == 0 && kFastWaves % kWavesXTree == 0, "block wave layout");
constexpr int kFrameWords = 20;  // general-kernel stack frame (float64 words)
constexpr int kFetchStride = 32;  // uint32 words between counters
constexpr int kSphWords = RTX_GEOM_WORDS + RTX_MAT_WORDS;
constexpr int kLdsMaxSpheres = 128;  // scene table staged in LDS up to this size (32 KiB)
// The one-tile culled kernels (TP 1, capped) accumulate the pixel colour in LDS
// after the scene table ([3][block] doubles, each lane its own slots) instead of three VGPR pairs:
// at 96 VGPRs (5 waves/SIMD) one of them spilled to scratch on every level (C3 traffic 1.5x).
constexpr size_t kColourLdsBytes = 3 * sizeof(double) * 256;
// the general kernel's nearest pass walks the culling tree from this many spheres on (A/B: 65
// spheres -11%, 17 spheres +2..6%: its depth-first lanes diverge, so a wave-uniform walk pays less)
constexpr int kGeneralTreeMin = 32;
// scenes of fewer spheres never carry a culling tree (scene_pack.BVH_MIN_SPHERES): the fast kernel's
// TREE = false instantiations serve them
constexpr int kTreeMinSpheres = 8;

// Wave-uniform loads through the scalar cache: the constant address space makes hipcc emit s_load
// even though the kernel also stores (it cannot prove the scene blob is not aliased otherwise).
typedef const double __attribute__((address_space(4))) cdouble;

struct Params {
  const double* scene;
  int nsph;
  int mode;  // 0: camera rays, 1: explicit rays, 2: continuation of deferred chains (in_list),
             // 3: explicit rays whose level-0 hit is given (hit_shape at hit_t: Shader.create)
  // camera mode: local rows of parts part .. part + part_run - 1 of the n_parts-way row interleave
  int width, height, row_block, n_parts, part, n_rows;
  int part_run = 1;
  // explicit-ray mode
  const double* org;
  int64_t org_stride;
  const double* dir;
  const double* hit_t;  // mode 3: level-0 distance per ray
  int hit_shape;        // mode 3: the shape every ray hit
  // common
  int64_t n;  // rays in this launch (= width * n_rows in camera mode)
  int max_bounces;
  void* out;
  int out_kind;
  uint8_t* ws;
  int64_t list_cap;  // capacity of each deferred list
  // Deferred lists (workspace). A launch appends to dlist (counter dcount); a chain deferred for
  // depth after level drec_level also gets a resume record (slot < rec_cap) in drec. The
  // continuation pass (mode 2) and the general kernel read in_list (counter in_count), whose deep
  // entries of level in_level resume from in_rec.
  uint64_t* dlist;
  uint32_t* dcount;
  double* drec;
  int drec_level;
  const uint64_t* in_list;
  const uint32_t* in_count;
  const double* in_rec;
  int in_level;
  int64_t rec_cap;     // records drec holds
  int64_t in_rec_cap;  // records in_rec holds
  double* stack;
  int64_t n_workers;
  int stack_levels;
  unsigned long long* stats;
  int n_tiles_x, n_tiles_y;  // persistent launch of k_render_fast (wave tiles; 0: one block tile per block)
  // persistent waves (n_fetch > 0): wave tiles (kWaveW x kWaveH) handed out by n_fetch counters
  uint32_t* fetch;
  int n_fetch;
  // multi-frame launch (rtx_render_frames): frame f reads scene + f * scene_stride and writes
  // out + f * (one frame's output); n counts the pixels of ONE frame
  int64_t scene_stride;
  int n_frames;
  int frame;  // set per block / per deferred ray (kernel side)
  uint32_t* deferred_out;  // the launch's deferred-ray count (rtx_render_camera_ex), or null
  int no_general;  // RTX_F_NO_GENERAL: no general kernel follows, so nothing may be deferred
  int images;      // RTX_F_IMAGES: the capped LDS kernels shade image-textured spheres themselves
  // camera launches of one frame (rtx_render_camera_sched): the dispatch units (the persistent
  // launch's wave tiles, else the grid's block tiles) in dispatch order (null: bottom-up row order),
  // and per-unit render times to record (s_memrealtime ticks), or null
  const uint32_t* tile_order;
  uint32_t* tile_cost;
  int reserve;  // RTX_F_RESERVE: block slots the persistent launch leaves free (host side only)
  // small-scene launches (rtx_small.hip sets it): floor(2^32 / grid.x), or 2^32 - 1 for grid.x == 1;
  // small_wave divides a tile_order entry by grid.x with it
  uint32_t tile_div;
};

// Deferred-list entry (uint64): pixel | frame << 40 | (rays counted through level a) + 1 << 56 |
// (hits counted through level b) + 1 << 60. The general kernel re-renders the pixel from level 0
// and skips the per-level counts the fast kernel already made (a, b = -1: none).
constexpr int kFrameShift = 34;
constexpr int kRaysShift = 50;
constexpr int kHitsShift = 57;
constexpr int kLevelMask = 0x7F;  // 7-bit level fields (level + 1)
// Resume record of a pixel deferred for depth at level L: the next level's ray (origin, direction),
// the colour accumulated through level L and the throughput of level L + 1, 10 words whatever L;
// the continuation pass and the general kernel continue the chain at level L + 1 instead of
// re-rendering it from level 0.
constexpr int kRecWords = 10;
// the first DEEP pass's record level (a runtime level, no storage per level; A/B r5zo
// on unbounded renders end to end, 5 / 9 / 14 levels: C2 98.7 / 93.7 / 77.8 us, C3 378 / 367 / 326 us,
// C4 2,514 / 2,485 / 2,440 us; r5zp, 14 / 16 / 30 with the continuation pass to 60: C2 77.8 / 77.5 /
// 77.4, C3 327 / 310 / 304, C4 2,437 / 2,380 / 2,166 us)
constexpr int kFirstPassLevels = 30;
constexpr int kDeepLevel3 = 60;  // the continuation pass's record level
static_assert(kFirstPassLevels >= kDeepLevels && kFirstPassLevels < kDeepLevel3, "first-pass record level");
static_assert(kDeepLevel3 + 2 < kLevelMask, "deferred-entry level fields hold 7 bits");
// Resume-record capacities of the first pass and (cont) of the continuation pass: at least 2^18 /
// 2^14, or one per 32 / 2048 pixels, whichever is more. Chains alive at level 5 are 0.2-1.4% of the
// pixels in the bench scenes (C4: 467,657 of 33.2 M), far fewer at the record levels. An entry
// beyond the capacity is re-rendered from level 0 by the general kernel: correct, but slow.
constexpr int64_t records_cap(int64_t n, bool cont) {
  const int64_t lo = int64_t(1) << (cont ? 14 : 18);
  const int64_t by_n = n / (cont ? 2048 : 32);
  const int64_t want = by_n > lo ? by_n : lo;
  return n < want ? n : want;
}

// append one entry to the launch's deferred list; returns its slot (or -1 when the list is full).
// Under RTX_F_NO_GENERAL no general kernel follows: the entry is dropped and RTX_ST_UNRENDERED raised
// (the pixel stays unwritten, the list and its counter stay clean for the next call).
__device__ __forceinline__ int64_t append_deferred(const Params& p, uint64_t entry) {
  if (p.no_general) {
    atomicOr((uint32_t*)p.ws + RTX_WS_STATUS, (uint32_t)RTX_ST_UNRENDERED);
    return -1;
  }
  const uint32_t slot = atomicAdd(p.dcount, 1u);
  if ((int64_t)slot < p.list_cap) {
    p.dlist[slot] = entry;
    return slot;
  }
  atomicOr((uint32_t*)p.ws + RTX_WS_STATUS, (uint32_t)RTX_ST_LIST_OVERFLOW);
  return -1;
}
__device__ __forceinline__ uint64_t deferred_entry(int64_t i, int frame, int rays_through, int hits_through) {
  return (uint64_t)i | ((uint64_t)frame << kFrameShift) | ((uint64_t)(rays_through + 1) << kRaysShift) |
         ((uint64_t)(hits_through + 1) << kHitsShift);
}

// Parameters of frame f of a multi-frame launch (the identity for f == 0).
__device__ __forceinline__ Params frame_view(const Params& p, int f) {
  Params q = p;
  q.scene = p.scene + (int64_t)f * p.scene_stride;
  q.out = (uint8_t*)p.out + (int64_t)f * p.n * out_bytes_per_pixel(p.out_kind);
  q.frame = f;
  return q;
}

// ------------------------------------------------------------------------------------------
// arithmetic helpers (reference semantics)
// ------------------------------------------------------------------------------------------

__device__ __forceinline__ double dot3(double ax, double ay, double az, double bx, double by, double bz) {
  return ((ax * bx) + (ay * by)) + (az * bz);  // NumpyVector3D.dot, base.py:34-35
}

// Wave-uniform header words as bit patterns: gfx9 has no scalar floating point, so a compare of a
// double that sits in scalar registers is a vector instruction in every lane; its integer reading is
// scalar.
__device__ __forceinline__ uint64_t f64_bits(double v) { return (uint64_t)__double_as_longlong(v); }
// v != 0.0 (true for NaN, false for either zero) by its bits
// (as two dwords: the compiler turns the 64-bit form back into the compare of doubles)
__device__ __forceinline__ bool f64_nonzero_bits(double v) {
  return (((uint32_t)__double2hiint(v) << 1) | (uint32_t)__double2loint(v)) != 0;
}

// The range-checked helpers below (sph_test, inv_mag, inv_mag_unit, sin_ref and what calls them) take
// their guard as the type of their `tame` argument. A double (the half-b threshold, or NaN) is the
// guarded form: one ballot and one wave-uniform branch per helper, the full expansion if any active
// lane is out of range. Sticky is the optimistic form (fast_tile's first body in the counter-free
// capped small-scene kernels, tame camera launches only): every helper takes its exact fast core
// unconditionally and ORs its own guard's failure into the lane's flag, nothing branches on it, and
// the wave takes one verdict after the bounce loop. A tripped lane's values are garbage from there
// on, but only values: every index derived downstream (the hit sphere, the LDS offsets, the texture
// key) comes from comparisons and loop counters, never from arithmetic on such a value.
struct Sticky {
  bool& bad;
  __device__ __forceinline__ operator double() const { return 0x1.0p-350; }  // the tame threshold
  __device__ __forceinline__ void trip(bool failed) const { bad = bad || failed; }
};
template <typename Tm>
constexpr bool kSticky = std::is_same<Tm, Sticky>::value;

// Correctly rounded sqrt and division, fast paths. LLVM lowers f64 sqrt / fdiv for gfx9 to a
// correctly rounded sequence (v_rsq_f64 / v_rcp_f64 + Newton-Raphson FMAs) wrapped in operand
// scaling (v_ldexp, v_div_scale) and special-value fix-ups (v_cmp_class, v_div_fixup). For operands
// where the scaling is provably the identity and no special value occurs, the cores below are the
// very same instruction sequence without the wrapping, hence bit-identical; every other operand
// takes the full expansion. (k_selftest_math checks both paths bit for bit on the device.)
__device__ __forceinline__ double sqrt_core(double x) {  // x in [2^-767, DBL_MAX]
  const double y = __builtin_amdgcn_rsq(x);
  double g = x * y;
  double h = y * 0.5;
  const double r = __builtin_fma(-h, g, 0.5);
  g = __builtin_fma(g, r, g);
  h = __builtin_fma(h, r, h);
  double d = __builtin_fma(-g, g, x);
  g = __builtin_fma(d, h, g);
  d = __builtin_fma(-g, g, x);
  return __builtin_fma(d, h, g);
}
__device__ __forceinline__ double sqrt_cr(double x) {
  // wave-uniform choice (one ballot): the fast core unless some active lane is out of range
  if (__ballot(!(x >= 0x1.0p-767 && x <= 0x1.fffffffffffffp+1023)) == 0) return sqrt_core(x);
  return __builtin_sqrt(x);
}
// a / b for a, b with |.| in [2^-300, 2^300] (v_div_scale leaves them unchanged and clears VCC, so
// v_div_fmas is a plain fma; the quotient is normal, so v_div_fixup returns it unchanged)
__device__ __forceinline__ double div_core(double a, double b) {
  double r = __builtin_amdgcn_rcp(b);
  double e = __builtin_fma(-b, r, 1.0);
  r = __builtin_fma(r, e, r);
  e = __builtin_fma(-b, r, 1.0);
  r = __builtin_fma(r, e, r);
  const double q = a * r;
  const double rem = __builtin_fma(-b, q, a);
  return __builtin_fma(rem, r, q);
}
__device__ __forceinline__ bool div_range(double x) {
  const double ax = fabs(x);
  return ax >= 0x1.0p-300 && ax <= 0x1.0p+300;
}
__device__ __forceinline__ double div_cr(double a, double b) {
  if (__ballot(!(div_range(b) && (a == 0.0 || div_range(a)))) == 0)  // wave-uniform choice
    return a == 0.0 ? a * __builtin_copysign(1.0, b) : div_core(a, b);
  return a / b;
}

// 1.0 / where(mag == 0, 1, mag) with mag = sqrt(d), d = |v|^2 (NumpyVector3D.norm, base.py:61-64).
// d in [2^-600, 2^600] puts sqrt's operand and the quotient's divisor (mag in [2^-300, 2^300],
// non-zero) in both cores' exact ranges: one wave-uniform check instead of three.
template <typename Tm = double>
__device__ __forceinline__ double inv_mag(double d, Tm tame = Tm()) {
  if constexpr (kSticky<Tm>) {
    tame.trip(!(d >= 0x1.0p-600 && d <= 0x1.0p+600));
    return div_core(1.0, sqrt_core(d));
  }
  if (__ballot(!(d >= 0x1.0p-600 && d <= 0x1.0p+600)) == 0) return div_core(1.0, sqrt_core(d));
  const double mag = sqrt_cr(d);
  return div_cr(1.0, mag == 0.0 ? 1.0 : mag);
}

template <typename Tm = double>
__device__ __forceinline__ void norm3(double& x, double& y, double& z, Tm tame = Tm()) {
  // NumpyVector3D.norm, base.py:61-64: v * (1.0 / where(mag == 0, 1, mag))
  const double r = inv_mag(dot3(x, y, z, x, y, z), tame);
  x = x * r;
  y = y * r;
  z = z * r;
}

// 1.0 / where(mag == 0, 1, mag), mag = sqrt(d), for d = |v|^2 within 2^-30 of 1: the norm of a
// vector that is already unit up to rounding (a direction normalised before, or the reflection of
// one). Write d = 1 + j 2^-53 (j an integer, even when positive). The correctly rounded sqrt(d) is
// 1 + floor(j/4) 2^-52 for j >= 0 and 1 - ceil(-j/2) 2^-53 for j < 0, and the correctly rounded
// reciprocal of either is 1 - floor(j/4) 2^-52: the second-order terms stay far below half an ulp
// for |j| <= 2^23. (d - 1) * 2^51 = j/4 exactly, floor is exact and so is the fma, so the result is
// bit-identical to div(1, sqrt(d)) (tests/test_unit_norm.py checks every such d against IEEE sqrt
// and division; k_selftest_math checks this path on the device).
__device__ __forceinline__ double inv_mag_near1(double d) {
  return __builtin_fma(-__builtin_floor((d - 1.0) * 0x1.0p51), 0x1.0p-52, 1.0);
}
template <typename Tm = double>
__device__ __forceinline__ double inv_mag_unit(double d, Tm tame = Tm()) {
  if constexpr (kSticky<Tm>) {
    tame.trip(!(fabs(d - 1.0) <= 0x1.0p-30));
    return inv_mag_near1(d);
  }
  // wave-uniform: the closed form unless some active lane is out of its range
  if (__ballot(!(fabs(d - 1.0) <= 0x1.0p-30)) == 0) return inv_mag_near1(d);
  return inv_mag(d);
}
template <typename Tm = double>
__device__ __forceinline__ void norm3_unit(double& x, double& y, double& z, Tm tame = Tm()) {
  // NumpyVector3D.norm (base.py:61-64) of a vector expected to be unit up to rounding
  const double r = inv_mag_unit(dot3(x, y, z, x, y, z), tame);
  x = x * r;
  y = y * r;
  z = z * r;
}

// np.clip(x, 0, 1) and np.maximum(x, 0) as v_max_f64 / v_min_f64. They differ from the reference
// only for NaN inputs and in the sign of a zero result, which never reaches the output: every such
// value is squared, scaled into a sum with the 0.004 ambient term, or compared with <= 0.
__device__ __forceinline__ double clip01(double x) { return __builtin_fmin(__builtin_fmax(x, 0.0), 1.0); }

__device__ __forceinline__ double max0(double x) { return __builtin_fmax(x, 0.0); }

__device__ __forceinline__ int trunc_parity(double x) {
  // (x).astype(int) % 2 (shader.py:30): truncation to int64, then floor-mod 2 == (k & 1).
  // |x| >= 2^53 doubles are even integers; NaN / |x| >= 2^63 convert to INT64_MIN (even).
  const double k = trunc(x);
  const double h = k * 0.5;
  return (x == x) && (h != trunc(h));
}

// b > 0 and c >= 0 (the sphere lies behind an origin outside it): the reference's root is never
// positive, so the test is FARAWAY without a square root. Proof: disc = fl(fl(b*b) - 4c) <= fl(b*b),
// and for b with b*b a normal double (1e-150 <= b <= 1e150) the correctly rounded sqrt(fl(b*b)) is b
// itself (b*b*(1 + 2^-53) has a root below b + ulp(b)/2), so sq <= b and s1 = (-b + sq) / 2 <= 0.
// Below 1e-150, b*b may round up by far more than an ulp in the subnormal range (b = 1.6e-162, c = 0:
// the reference reports a hit at 3.1e-163, tests/golden/intersect_kat.json), so those take the root.
__device__ __forceinline__ bool behind(double b, double c) {
  return b >= 1e-150 && c >= 0.0 && b <= 1e150;
}

// NumpySphere.intersect, shape.py:28-51, for a ray with precomputed oo = O.O.
// b = 2 * D.(O - C);  c = ((C.C + O.O) - 2 * C.O) - r*r;  disc = b^2 - 4c.
template <typename P>
__device__ __forceinline__ double isect(const P* g, double ox, double oy, double oz, double oo, double dx, double dy,
                                        double dz) {
  const double cx = g[RTX_G_CX], cy = g[RTX_G_CY], cz = g[RTX_G_CZ];
  const double b = 2.0 * dot3(dx, dy, dz, ox - cx, oy - cy, oz - cz);
  const double c = ((g[RTX_G_CC] + oo) - 2.0 * dot3(cx, cy, cz, ox, oy, oz)) - g[RTX_G_RR];
  const double disc = (b * b) - (4.0 * c);
  double t = FARAWAY;
  if (disc > 0.0 && !behind(b, c)) {  // np.where((disc > 0) & (sol > 0), sol, FARAWAY); sqrt(max(0, disc)) == sqrt(disc) here
    const double sq = sqrt_cr(disc);
    const double s0 = (-b - sq) * 0.5;  // == / 2 exactly
    const double s1 = (-b + sq) * 0.5;
    // (s0 > 0) & (s0 < s1) ? s0 : s1 — with sq > 0, s0 <= s1 and s0 == s1 only as equal values
    const double sol = s0 > 0.0 ? s0 : s1;
    if (sol > 0.0) t = sol;
  }
  return t;
}

// The same test split in two halves so that two spheres' dependency chains interleave (and their
// scalar loads share one wait): isect_disc computes the quadratic's coefficients, isect_sol the rest.
//
// Half-b form. With h = D.(O - C) the reference's b is 2h exactly, b*b = 4 fl(h*h), 4c is exact,
// disc = 4 fl(fl(h*h) - c) = 4q, sqrt(disc) = 2 sqrt(q) and its roots (-b -+ sqrt(disc)) / 2 are
// fl(-h -+ sqrt(q)): bit for bit the same numbers, four multiplications and the range checks
// fewer. Each step is an exact scaling by a power of two as long as nothing leaves the normal
// range: h*h must be normal and not overflow, 4c must not overflow. The host marks a scene "tame"
// (RTX_H_TAME) when every coordinate and radius is below 2^60, so that |O|, |O - C| stay below
// ~2^140 for every origin a hit can produce (t < FARAWAY ~ 2^130) and |h| < 2^141, |c| < 2^284;
// the lower end is checked per wave: |h| >= 2^-350 in every active lane. Then q is 0 or at least
// 2^-753 in magnitude (h*h >= 2^-700; a nonzero q = fl(h*h) - c is either above half of h*h or an
// exact Sterbenz difference, a multiple of ulp(h*h)/2), so q is inside sqrt_core's exact range,
// and -h -+ sqrt(q) is 0 or normal. Explicit-ray launches and untamed scenes, and any wave with a
// lane at |h| < 2^-350 (a ray at right angles to O - C, such as tests/golden/intersect_kat.json's
// b = 1.6e-162 case), evaluate the reference expressions instead.
struct SphTest {
  double h, d;  // h = D.(O - C); d: q (half) or the reference's disc = (2h)^2 - 4c
  bool skip;    // no hit in this lane: d <= 0, or the sphere lies behind the origin
  int half;     // wave-uniform (an int: a uniform bool carried across blocks costs VALU copies)
};
// h > 0 and c >= 0 (|h| >= 2^-350): q <= fl(h*h) and sqrt(fl(h*h)) == h, so -h + sqrt(q) <= 0
// tame: the lower bound 2^-350 in a tame launch, NaN otherwise (no |h| passes; a double threshold
// keeps the uniform flag out of lane-mask copies)
template <typename Tm>
__device__ __forceinline__ SphTest sph_test(double h, double c, Tm tame) {
  SphTest t;
  if constexpr (kSticky<Tm>) {  // the half-b form whatever |h| is; a lane below the bound is flagged
    tame.trip(!(fabs(h) >= 0x1.0p-350));
    t.half = 1;
  } else {
    t.half = __ballot(!(fabs(h) >= tame)) == 0 ? 1 : 0;
  }
  t.h = h;
  if (t.half) {
    t.d = (h * h) - c;
    t.skip = !(t.d > 0.0) || (h > 0.0 && c >= 0.0);
  } else {
    const double b = 2.0 * h;  // b = 2.0 * D.(O - C), shape.py:33-37
    t.d = (b * b) - (4.0 * c);
    t.skip = !(t.d > 0.0) || behind(b, c);
  }
  return t;
}
// sph_test with c >= 0.0 decided by the caller (cpos, wave-uniform: the host's verdict on the camera's
// c, RTX_H_CAMREL) instead of a compare in every lane; everything else as above
template <typename Tm>
__device__ __forceinline__ SphTest sph_test_cpos(double h, double c, bool cpos, Tm tame) {
  SphTest t;
  if constexpr (kSticky<Tm>) {
    tame.trip(!(fabs(h) >= 0x1.0p-350));
    t.half = 1;
  } else {
    t.half = __ballot(!(fabs(h) >= tame)) == 0 ? 1 : 0;
  }
  t.h = h;
  if (t.half) {
    t.d = (h * h) - c;
    // (no short circuit: the verdict's load then stays with the record's, outside a branch of its own)
    t.skip = !(t.d > 0.0) | ((h > 0.0) & cpos);
  } else {
    const double b = 2.0 * h;
    t.d = (b * b) - (4.0 * c);
    t.skip = !(t.d > 0.0) || (b >= 1e-150 && cpos && b <= 1e150);  // behind(b, c)
  }
  return t;
}
template <typename P, typename Tm>
__device__ __forceinline__ SphTest isect_disc(const P* g, double ox, double oy, double oz, double oo, double dx,
                                              double dy, double dz, Tm tame) {
  const double cx = g[RTX_G_CX], cy = g[RTX_G_CY], cz = g[RTX_G_CZ];
  const double h = dot3(dx, dy, dz, ox - cx, oy - cy, oz - cz);
  const double c = ((g[RTX_G_CC] + oo) - 2.0 * dot3(cx, cy, cz, ox, oy, oz)) - g[RTX_G_RR];
  return sph_test(h, c, tame);
}
// level-0 camera origin: O - C from uniform values, c precomputed on the host (same expressions)
template <typename P, typename Tm>
__device__ __forceinline__ SphTest isect_disc_cam(const P* g, double ox, double oy, double oz, double dx, double dy,
                                                  double dz, Tm tame) {
  const double h = dot3(dx, dy, dz, ox - g[RTX_G_CX], oy - g[RTX_G_CY], oz - g[RTX_G_CZ]);
  return sph_test(h, g[RTX_G_C0], tame);
}
// ... and O - C too (r: the sphere's RTX_H_CAMREL record, the host's float64 camera - centre and
// its verdict on c >= 0.0): h starts at the dot product, with each difference as the multiplication's
// one scalar operand, and the behind test needs no compare of c
template <typename Tm>
__device__ __forceinline__ SphTest isect_disc_rel(const cdouble* g, const cdouble* r, double dx, double dy, double dz,
                                                  Tm tame) {
  const double h = dot3(dx, dy, dz, r[0], r[1], r[2]);
  // the verdict word is 1.0 or 0.0: its high dword alone, so that the test is a 32-bit scalar compare
  const uint32_t cpos = ((const uint32_t __attribute__((address_space(4)))*)r)[2 * 3 + 1];
  return sph_test_cpos(h, g[RTX_G_C0], cpos != 0, tame);
}
// The rest of the test, as a root and a validity flag instead of the FARAWAY sentinel (no f64
// selects of a non-inline constant): valid <=> the reference returns the root, not FARAWAY. With
// s0 <= s1 (rounding is monotone), (s0 > 0 ? s0 : s1) > 0 <=> s1 > 0. Lanes without a root take
// the square root of |disc|, a discarded dummy.
__device__ __forceinline__ double isect_sol(const SphTest& t, bool& valid) {
  if (t.half) {
    // s1 = fl(-h + sq) > 0 <=> sq > h and s0 > 0 <=> -h > sq (a sum of two doubles rounds to 0 only
    // when it is 0); the root is -h + (s0 > 0 ? -sq : sq), -sq by flipping the high word's sign.
    // (skip covers q <= 0; its other half, behind, implies s1 <= 0, so valid needs no q > 0 test.)
    const double sq = sqrt_core(fabs(t.d));
    valid = !t.skip && sq > t.h;
    const uint32_t hi = __double2hiint(sq), lo = __double2loint(sq);
    const uint32_t shi = (-t.h > sq) ? (hi ^ 0x80000000u) : hi;
    return -t.h + __hiloint2double(shi, lo);
  }
  const double b = 2.0 * t.h;
  const double sq = sqrt_cr(fabs(t.d));
  const double s0 = (-b - sq) * 0.5;  // == / 2 exactly
  const double s1 = (-b + sq) * 0.5;
  valid = !t.skip && s1 > 0.0;  // behind (in skip) implies s1 <= 0
  return s0 > 0.0 ? s0 : s1;
}
// One sphere / two spheres at once: the square roots run only if some lane may hit, and the
// consumer f(t, valid[, t1, valid1]) runs inside that branch, so an invalid root is never carried
// out of it (a placeholder root would cost a move per test; an uninitialised one would be
// undefined behaviour, which the compiler exploits by deleting the skip test). Lanes outside the
// branch have no valid root for either sphere.
template <typename F>
__device__ __forceinline__ void isect_one(const SphTest& a, F&& f) {
  if (!a.skip) {
    bool v;
    const double t = isect_sol(a, v);
    f(t, v);
  }
}
template <typename F>
__device__ __forceinline__ void isect_pair(const SphTest& a, const SphTest& b, F&& f) {
  if (!a.skip || !b.skip) {
    bool v0, v1;
    const double t0 = isect_sol(a, v0);
    const double t1 = isect_sol(b, v1);
    f(t0, v0, t1, v1);
  }
}
// isect (the reference's root or FARAWAY) through the split test
template <typename P, typename Tm>
__device__ __forceinline__ double isect_t(const P* g, double ox, double oy, double oz, double oo, double dx, double dy,
                                          double dz, Tm tame) {
  double r = FARAWAY;
  isect_one(isect_disc(g, ox, oy, oz, oo, dx, dy, dz, tame), [&](double t, bool v) {
    if (v) r = t;
  });
  return r;
}

// nearest-hit bookkeeping in scene order (base.py:97-103): the first strictly smaller t wins; an
// equal t marks a tie, which is cleared by any later strictly smaller t. tmin starts at FARAWAY and
// only decreases, so an invalid test (FARAWAY) never updates it. A valid root equal to FARAWAY
// itself would flag a tie here: the pixel then goes to the general kernel, which is exact.
__device__ __forceinline__ void nearest_update(bool valid, double t, int s, double& tmin, int& hit, bool& tie) {
  if (valid && t < tmin) {
    tmin = t;
    hit = s;
    tie = false;
  } else if (valid && t == tmin) {
    tie = true;
  }
}

// Executed-work counters of the stats launch (bench.py's executed-FLOP model): ray-sphere tests
// and culling-node tests performed by each live lane. Work<false> (the timed kernels) compiles to
// nothing.
template <bool ON>
struct Work {
  __device__ __forceinline__ void test(int) {}
  __device__ __forceinline__ void node() {}
  __device__ __forceinline__ void box() {}
  __device__ __forceinline__ void beam() {}
};
template <>
struct Work<true> {
  uint32_t tests = 0, nodes = 0;
  uint32_t tests1 = 0, nodes1 = 0;  // of the nearest-hit searches of reflected rays (levels >= 1)
  uint32_t boxes = 0;  // of the node tests, the culling tree's box tests (the rest: frustum planes and
                       // shadow-grid lookups, priced as node tests)
  uint32_t beamt = 0;  // reflected-ray beam tests: one per live lane and beam pass (RTX_S_BEAMT)
  __device__ __forceinline__ void test(int k) { tests += (uint32_t)k; }
  __device__ __forceinline__ void node() { ++nodes; }
  __device__ __forceinline__ void box() { ++boxes; }
  __device__ __forceinline__ void beam() { ++beamt; }
};

// Shadow any-hit: does test j (root t, validity v) come strictly before the shape's own distance
// t_self? An invalid test is FARAWAY, which is before t_self only when t_self > FARAWAY (far_self).
__device__ __forceinline__ bool shadows(bool valid, double t, double tself, bool far_self) {
  return valid ? t < tself : far_self;
}

// Records first .. end - 1 of a geometry table (the scene's, or the culled list), wave-uniform, two
// at a time through isect_pair and an odd one left through isect_one: disc(g) starts a record's test,
// sph(g, k) names its sphere, use(s, root, valid) consumes it, record k before k + 1 (the tie flag
// depends on scene order). readfirstlane keeps k scalar in divergent loops. Callers count their work.
template <typename P, typename Disc, typename Sph, typename Use>
__device__ __forceinline__ void scan_range(const P* geo, int first, int end, Disc&& disc, Sph&& sph, Use&& use) {
  int k = first;
  for (; k + 1 < end; k += 2) {
    const P* g0 = geo + __builtin_amdgcn_readfirstlane(k) * RTX_GEOM_WORDS;
    const P* g1 = g0 + RTX_GEOM_WORDS;
    const SphTest a0 = disc(g0), a1 = disc(g1);
    const int s0 = sph(g0, k), s1 = sph(g1, k + 1);
    isect_pair(a0, a1, [&](double t0, bool v0, double t1, bool v1) {
      use(s0, t0, v0);
      use(s1, t1, v1);
    });
  }
  if (k < end) {
    const P* g0 = geo + __builtin_amdgcn_readfirstlane(k) * RTX_GEOM_WORDS;
    const SphTest a0 = disc(g0);
    const int s0 = sph(g0, k);
    isect_one(a0, [&](double t0, bool v0) { use(s0, t0, v0); });
  }
}

// Stackless depth-first walk of the culling tree: a node is entered when may(node) holds in any lane,
// else its subtree is skipped (RTX_N_SKIP). leaf(first, cnt) takes an entered node's range of the
// culled list (cnt == 0: an inner node) and returns whether to go on (wave-uniform).
template <typename May, typename Leaf>
__device__ __forceinline__ void tree_walk(const cdouble* nodes, int nn, May&& may, Leaf&& leaf) {
  int i = 0;
  while (i < nn) {
    const cdouble* nd = nodes + __builtin_amdgcn_readfirstlane(i) * RTX_NODE_WORDS;
    if (__ballot(may(nd)) != 0) {
      if (!leaf((int)nd[RTX_N_FIRST], (int)nd[RTX_N_COUNT])) break;
      ++i;
    } else {
      i = (int)nd[RTX_N_SKIP];
    }
  }
}

// ---- culling hierarchy ---------------------------------------------------------------------
// Conservative test: may any sphere inside a node's box produce, through the reference formula
// (shape.py:34-51), a hit with 0 < t <= tlim? If this returns false, every such sphere provably
// yields FARAWAY (or a t > tlim), so skipping it changes neither the nearest hit nor the tie test
// nor the shadow test.
// Error budget: the reference's discriminant carries an absolute error err <= ~64 eps * scale,
// scale = |Cn-O|^2 + (|Cn|+R)^2 + |O|^2 + R^2 for a sphere inside the bounding sphere (Cn, R) of
// the box (cancellation in c = |C|^2 + |O|^2 - 2 C.O - r^2). A root it reports is therefore within
// sqrt(err) <= lm = 1e-7 (scale + 1) of a point of the sphere's ball, i.e. of the box expanded by
// lm. With |Cn-O|^2 <= 2 (|Cn|+R)^2 + 2 |O|^2, lm <= 1e-7 (3 (|Cn|+R)^2 + R^2 + 1) + 3e-7 |O|^2; the
// box is expanded by twice that (N_MARGIN + 6e-7 |O|^2), which also absorbs the slab arithmetic's
// own rounding (~1e-15 relative) and |D| = 1 +- 1e-15.
struct RaySlab {
  double ix, iy, iz;  // 1 / direction component, components below 1e-200 in magnitude nudged to it
  double mo;          // 6e-7 |O|^2
};
__device__ __forceinline__ double slab_inv(double d) {
  // the reciprocal only places slab boundaries: rcp + one Newton step (~1e-16 relative) suffices;
  // the nudge keeps 0 * inf out of the slab products (a shift of 1e-200 * t is far below lm)
  const double dd = fabs(d) < 1e-200 ? __builtin_copysign(1e-200, d) : d;
  const double r = __builtin_amdgcn_rcp(dd);
  return __builtin_fma(r, __builtin_fma(-dd, r, 1.0), r);
}
__device__ __forceinline__ RaySlab ray_slab(double dx, double dy, double dz, double oo) {
  return RaySlab{slab_inv(dx), slab_inv(dy), slab_inv(dz), 6e-7 * oo};
}
__device__ __forceinline__ bool node_may_hit(const cdouble* nd, double ox, double oy, double oz, const RaySlab& r,
                                             double tlim) {
  const double m = nd[RTX_N_MARGIN] + r.mo;
  const double ax = ((nd[RTX_N_LOX] - m) - ox) * r.ix, bx = ((nd[RTX_N_HIX] + m) - ox) * r.ix;
  const double ay = ((nd[RTX_N_LOY] - m) - oy) * r.iy, by = ((nd[RTX_N_HIY] + m) - oy) * r.iy;
  const double az = ((nd[RTX_N_LOZ] - m) - oz) * r.iz, bz = ((nd[RTX_N_HIZ] + m) - oz) * r.iz;
  // a NaN slab (non-finite origin) is dropped by fmin/fmax: unconstrained, hence conservative
  const double tn = __builtin_fmax(__builtin_fmax(__builtin_fmin(ax, bx), __builtin_fmin(ay, by)), __builtin_fmin(az, bz));
  const double tf = __builtin_fmin(__builtin_fmin(__builtin_fmax(ax, bx), __builtin_fmax(ay, by)), __builtin_fmax(az, bz));
  return tn <= tf && tf >= 0.0 && tn <= tlim;
}

// Nearest hit over entries [first, first + cnt) of the culled geometry list.
template <bool CAM, typename Wk>
__device__ __forceinline__ void nearest_range(const cdouble* cg, int first, int cnt, double ox, double oy, double oz,
                                              double oo, double dx, double dy, double dz, double& tmin, int& hit,
                                              bool& tie, double tame, Wk& wk) {
  wk.test(cnt);
  scan_range(
      cg, first, first + cnt,
      [&](const cdouble* g) {
        return CAM ? isect_disc_cam(g, ox, oy, oz, dx, dy, dz, tame) : isect_disc(g, ox, oy, oz, oo, dx, dy, dz, tame);
      },
      [](const cdouble* g, int) { return (int)g[RTX_G_IDX]; },
      [&](int s, double t, bool v) { nearest_update(v, t, s, tmin, hit, tie); });
}

// Nearest hit through the culling tree: the always-tested spheres, then the walk, entering a node
// when any lane of the wave may hit it before its current nearest t.
// Evaluation order differs from scene order, which the result does not depend on: the nearest t
// is a minimum, `hit` is its unique owner unless tied, and a tie is flagged whatever the order.
template <bool CAM, typename Wk>
__device__ __forceinline__ void nearest_bvh(const cdouble* sc, double ox, double oy, double oz, double dx, double dy,
                                            double dz, double& tmin, int& hit, bool& tie, double tame, Wk& wk) {
  const cdouble* cg = sc + (int)sc[RTX_H_CGEO];
  const cdouble* nodes = sc + (int)sc[RTX_H_NODES];
  const int nn = (int)sc[RTX_H_NNODES];
  const double oo = dot3(ox, oy, oz, ox, oy, oz);
  tmin = FARAWAY;
  hit = -1;
  tie = false;
  nearest_range<CAM>(cg, 0, (int)sc[RTX_H_NALWAYS], ox, oy, oz, oo, dx, dy, dz, tmin, hit, tie, tame, wk);
  const RaySlab rs = ray_slab(dx, dy, dz, oo);
  tree_walk(
      nodes, nn,
      [&](const cdouble* nd) {
        wk.node();
        wk.box();
        return node_may_hit(nd, ox, oy, oz, rs, tmin);
      },
      [&](int first, int cnt) {
        if (cnt > 0) nearest_range<CAM>(cg, first, cnt, ox, oy, oz, oo, dx, dy, dz, tmin, hit, tie, tame, wk);
        return true;
      });
}

// The general kernel's nearest pass through the culling tree: the nearest distance, how many
// shapes share it and the first of them in scene order (base.py:97-103). Traversal order does not
// matter: the minimum is order-free, equal distances are all counted, and the smallest scene index
// among them is kept. A sphere at exactly the current nearest distance is never culled (its box is
// reached at t <= tlim).
__device__ __forceinline__ void count_update(bool valid, double t, int s, double& tmin, int& nh, int& first) {
  if (valid && t < tmin) {
    tmin = t;
    nh = 1;
    first = s;
  } else if (valid && t == tmin) {
    ++nh;
    first = s < first ? s : first;
  }
}
__device__ __forceinline__ void nearest_count_bvh(const cdouble* sc, double ox, double oy, double oz, double oo,
                                                  double dx, double dy, double dz, double& tmin, int& nh,
                                                  int& first) {
  const cdouble* cg = sc + (int)sc[RTX_H_CGEO];
  const cdouble* nodes = sc + (int)sc[RTX_H_NODES];
  const int nn = (int)sc[RTX_H_NNODES];
  auto range = [&](int k, int end) {
    for (; k < end; ++k) {
      const cdouble* g0 = cg + __builtin_amdgcn_readfirstlane(k) * RTX_GEOM_WORDS;
      const int s0 = (int)g0[RTX_G_IDX];
      isect_one(isect_disc(g0, ox, oy, oz, oo, dx, dy, dz, __builtin_nan("")),
                [&](double t0, bool v0) { count_update(v0, t0, s0, tmin, nh, first); });
    }
  };
  range(0, (int)sc[RTX_H_NALWAYS]);
  const RaySlab rs = ray_slab(dx, dy, dz, oo);
  tree_walk(
      nodes, nn, [&](const cdouble* nd) { return node_may_hit(nd, ox, oy, oz, rs, tmin); },
      [&](int f, int cnt) {
        if (cnt > 0) range(f, f + cnt);
        return true;
      });
}
// The same of the pass kernels (aov, glass): through the tree when `tree` (wave-uniform) says so, else
// the table in scene order. tmin, nh and first come in as FARAWAY, 0 and nsph.
__device__ __forceinline__ void nearest_count(const cdouble* sc, int nsph, bool tree, double ox, double oy, double oz,
                                              double oo, double dx, double dy, double dz, double& tmin, int& nh,
                                              int& first) {
  if (tree) {
    nearest_count_bvh(sc, ox, oy, oz, oo, dx, dy, dz, tmin, nh, first);
  } else {
    const cdouble* geo = sc + RTX_HDR_WORDS;
    for (int s = 0; s < nsph; ++s) {
      const cdouble* g = geo + __builtin_amdgcn_readfirstlane(s) * RTX_GEOM_WORDS;
      isect_one(isect_disc(g, ox, oy, oz, oo, dx, dy, dz, __builtin_nan("")),
                [&](double t, bool v) { count_update(v, t, s, tmin, nh, first); });
    }
  }
}

// Shadow any-hit through the culling tree (shader.py:126-128 in its any-hit form): lit stays true
// unless some sphere is strictly nearer than the shape itself along the light direction. hs: the
// wave-uniform shape of every lane (nsph when the lanes differ), whose own test cannot shadow it.
// Callers guarantee t_self <= FARAWAY in every lane (an invalid test then never shadows).
// (Written out: through tree_walk and scan_range 43 rows of tools/resource_usage.py move, <6,1,0,0,1,1,0,0>
// from 0 to 3 spilled VGPRs; so do the three mask loops, nearest_masked, nearest_beam and min_masked.)
template <typename Wk>
__device__ __forceinline__ bool lit_bvh(const cdouble* sc, double qx, double qy, double qz, double qq, double lx,
                                        double ly, double lz, double tself, int hs, double tame, Wk& wk) {
  const cdouble* cg = sc + (int)sc[RTX_H_CGEO];
  const cdouble* nodes = sc + (int)sc[RTX_H_NODES];
  const int nn = (int)sc[RTX_H_NNODES];
  const int nal = (int)sc[RTX_H_NALWAYS];
  bool lit = true;
  for (int k = 0; k < nal; ++k) {
    const cdouble* g0 = cg + __builtin_amdgcn_readfirstlane(k) * RTX_GEOM_WORDS;
    if ((int)g0[RTX_G_IDX] == hs) continue;
    wk.test(1);
    isect_one(isect_disc(g0, qx, qy, qz, qq, lx, ly, lz, tame), [&](double t0, bool v0) {
      if (v0 && t0 < tself) lit = false;
    });
  }
  const RaySlab rs = ray_slab(lx, ly, lz, qq);
  int i = 0;
  while (i < nn) {
    const cdouble* nd = nodes + __builtin_amdgcn_readfirstlane(i) * RTX_NODE_WORDS;
    wk.node();
    wk.box();
    if (__ballot(lit && node_may_hit(nd, qx, qy, qz, rs, tself)) != 0) {
      const int cnt = (int)nd[RTX_N_COUNT];
      if (cnt > 0) {
        wk.test(cnt);
        const int first = (int)nd[RTX_N_FIRST], end = first + cnt;
        int k = first;
        for (; k + 1 < end; k += 2) {
          const cdouble* g0 = cg + __builtin_amdgcn_readfirstlane(k) * RTX_GEOM_WORDS;
          const cdouble* g1 = g0 + RTX_GEOM_WORDS;
          isect_pair(isect_disc(g0, qx, qy, qz, qq, lx, ly, lz, tame),
                     isect_disc(g1, qx, qy, qz, qq, lx, ly, lz, tame), [&](double t0, bool v0, double t1, bool v1) {
                       if ((v0 && t0 < tself) || (v1 && t1 < tself)) lit = false;
                     });
        }
        if (k < end) {
          const cdouble* g0 = cg + __builtin_amdgcn_readfirstlane(k) * RTX_GEOM_WORDS;
          isect_one(isect_disc(g0, qx, qy, qz, qq, lx, ly, lz, tame), [&](double t0, bool v0) {
            if (v0 && t0 < tself) lit = false;
          });
        }
      }
      if (__ballot(lit) == 0) break;  // every lane of the wave is in shadow
      ++i;
    } else {
      i = (int)nd[RTX_N_SKIP];
    }
  }
  return lit;
}

// Any-hit of the ray (q, d) from a hit (the pass kernels: aov's shadow mask, occlusion): true unless
// some shape is strictly nearer than tself. hs: a shape whose own test is skipped (nsph: none).
// Through the culling tree where the scene has one and no lane's tself lies beyond FARAWAY (the tree
// skips missing spheres, which shadow such a lane), else the table in scene order; the two agree.
__device__ __forceinline__ bool nothing_nearer(const cdouble* sc, int nsph, double qx, double qy, double qz, double qq,
                                               double dx, double dy, double dz, double tself, int hs) {
  const cdouble* geo = sc + RTX_HDR_WORDS;
  const double nan = __builtin_nan("");  // the reference expressions in every sphere test (SphTest)
  const bool far_self = tself > FARAWAY;
  bool open = true;
  if (sc[RTX_H_NNODES] != 0.0 && __ballot(far_self) == 0) {
    Work<false> wk;
    open = lit_bvh(sc, qx, qy, qz, qq, dx, dy, dz, tself, hs, nan, wk);
  } else {
    for (int s = 0; s < nsph; ++s) {
      if (s == hs) continue;
      const cdouble* g = geo + __builtin_amdgcn_readfirstlane(s) * RTX_GEOM_WORDS;
      bool sh = far_self;  // lanes without a valid root
      isect_one(isect_disc(g, qx, qy, qz, qq, dx, dy, dz, nan),
                [&](double t, bool v) { sh = shadows(v, t, tself, far_self); });
      if (sh) open = false;
      if (__ballot(open) == 0) break;  // every lane of the wave is decided
    }
  }
  return open;
}

// Nearest hit of ray (O, D) over all spheres, geometry through
// the scalar cache. CAM: O is the camera (level 0), using the host-precomputed c.
template <bool CAM, typename P, typename Wk, typename Tm>
__device__ __forceinline__ void nearest_hit(const P* geo, int nsph, double ox, double oy, double oz, double dx,
                                            double dy, double dz, double& tmin, int& hit, bool& tie, Tm tame,
                                            Wk& wk) {
  wk.test(nsph);
  tmin = FARAWAY;
  hit = -1;
  tie = false;
  const double oo = CAM ? 0.0 : dot3(ox, oy, oz, ox, oy, oz);
  scan_range(
      geo, 0, nsph,
      [&](const P* g) {
        return CAM ? isect_disc_cam(g, ox, oy, oz, dx, dy, dz, tame) : isect_disc(g, ox, oy, oz, oo, dx, dy, dz, tame);
      },
      [](const P*, int s) { return s; }, [&](int s, double t, bool v) { nearest_update(v, t, s, tmin, hit, tie); });
}

// The camera-relative centres of a small scene (RTX_H_CAMREL), or null: a blob without them, or with
// them elsewhere than in the header's spare words (where the packer puts the table of a scene of up to
// kCamRelHeaderSpheres spheres), takes the per-lane subtractions. The address is that fixed place, so
// the table's loads wait for no header word: the header only says whether the table is there. nsph:
// the blob's checked sphere count.
constexpr int kCamRelAt = RTX_H_CAMREL + 1;
constexpr int kCamRelHeaderSpheres = (RTX_HDR_WORDS - kCamRelAt) / RTX_CAMREL_WORDS;
template <int NSPH>
__device__ __forceinline__ const cdouble* camrel_table(const cdouble* sc, int nsph) {
  if constexpr (NSPH > kCamRelHeaderSpheres) return nullptr;
  if (NSPH == 0 && nsph > kCamRelHeaderSpheres) return nullptr;
  return f64_bits(sc[RTX_H_CAMREL]) == f64_bits((double)kCamRelAt) ? sc + kCamRelAt : nullptr;
}
// nearest_hit<true> with O - C and the sign of c from the table `rel` (camrel_table)
template <typename Wk, typename Tm>
__device__ __forceinline__ void nearest_hit_rel(const cdouble* geo, const cdouble* rel, int nsph, double dx, double dy,
                                                double dz, double& tmin, int& hit, bool& tie, Tm tame, Wk& wk) {
  static_assert(RTX_GEOM_WORDS == 2 * RTX_CAMREL_WORDS, "a geometry record's offset halves to its table record's");
  wk.test(nsph);
  tmin = FARAWAY;
  hit = -1;
  tie = false;
  scan_range(
      geo, 0, nsph, [&](const cdouble* g) { return isect_disc_rel(g, rel + (g - geo) / 2, dx, dy, dz, tame); },
      [](const cdouble*, int s) { return s; }, [&](int s, double t, bool v) { nearest_update(v, t, s, tmin, hit, tie); });
}

// (x)^5 and (x)^2.5 for x in [0, 1] (shader.py:291, :310). NumPy evaluates these with its SIMD pow;
// both are ~1 ulp, not correctly rounded, so neither side is "exact" here.
// np.sin (shader.py:211) for |x| <= 2^20. Neither side is correctly rounded (NumPy's SIMD sin is
// ~1 ulp); this one is <= 2 ulp (tests/test_sin.py: 1.9 ulp measured against long-double sin).
// x - n*pi with n = rint(x/pi): the first fma is exact (x and n*P1 are multiples of 2^-52 and
// their difference is below 2), the next two add the rest of pi to ~160 bits. Then
// sin(r) = r + r^3 * p(r^2) on [-pi/2, pi/2] with the Taylor coefficients up to r^21 (truncation
// 1.2e-18 relative), and sin(x) = (-1)^n sin(r).
__device__ __forceinline__ double sin_reduced(double x) {
  const double n = __builtin_rint(x * 0x1.45f306dc9c883p-2);
  double r = __builtin_fma(-n, 0x1.921fb54442d18p+1, x);
  r = __builtin_fma(-n, 0x1.1a62633145c07p-53, r);
  r = __builtin_fma(-n, -0x1.f1976b7ed8fbcp-109, r);
  const double z = r * r;
  double q = 0x1.71b8ef6dcf572p-66;  // 1/21!
  q = __builtin_fma(z, q, -0x1.2f49b46814157p-57);
  q = __builtin_fma(z, q, 0x1.952c77030ad4ap-49);
  q = __builtin_fma(z, q, -0x1.ae7f3e733b81fp-41);
  q = __builtin_fma(z, q, 0x1.6124613a86d09p-33);
  q = __builtin_fma(z, q, -0x1.ae64567f544e4p-26);
  q = __builtin_fma(z, q, 0x1.71de3a556c734p-19);
  q = __builtin_fma(z, q, -0x1.a01a01a01a01ap-13);
  q = __builtin_fma(z, q, 0x1.1111111111111p-7);
  q = __builtin_fma(z, q, -0x1.5555555555555p-3);  // -1/3!
  const double s = __builtin_fma(r * z, q, r);
  return ((int)n & 1) ? -s : s;
}
template <typename Tm = double>
__device__ __forceinline__ double sin_ref(const cdouble* sc, double x, Tm tame = Tm()) {
  if constexpr (kSticky<Tm>) {
    tame.trip(!(sc[RTX_H_SINRED] != 0.0 || fabs(x) <= 0x1.0p20));
    return sin_reduced(x);
  }
  // the reduction above when the host bounded every material's phase (RTX_H_SINRED), else
  // wave-uniform: unless some active lane is out of its range (or NaN / inf)
  if (sc[RTX_H_SINRED] != 0.0 || __ballot(!(fabs(x) <= 0x1.0p20)) == 0) return sin_reduced(x);
  return sin(x);
}

// Shading-only arithmetic: operands are non-negative and far from the overflow range
// by construction (denominators >= 1e-8, square-root arguments in [0, 2], |V|^2 and |H|^2 the
// squared lengths of finite vectors; a zero argument is selected around the core). The cores are
// bit-identical to the range-checked paths for operands above ~2^-900; below, only terms that are
// themselves below ~1e-250 can differ.
// rcp: the hardware estimate (~2^-24) and two Newton steps, correctly rounded on 4 M random
// operands (tools/approx_probe); a * rcp(b) is then within ~1 ulp of a / b.
__device__ __forceinline__ double div_shade(double a, double b) {
  double r = __builtin_amdgcn_rcp(b);
  r = __builtin_fma(r, __builtin_fma(-b, r, 1.0), r);
  r = __builtin_fma(r, __builtin_fma(-b, r, 1.0), r);
  return a * r;
}
// sqrt: the library core without its second correction (correctly rounded on the same sample);
// 0 stays 0 (rsq(0) = inf)
__device__ __forceinline__ double sqrt_shade(double x) {
  const double y = __builtin_amdgcn_rsq(x);
  double g = x * y, h = y * 0.5;
  const double r = __builtin_fma(-h, g, 0.5);
  g = __builtin_fma(g, r, g);
  h = __builtin_fma(h, r, h);
  const double d = __builtin_fma(-g, g, x);
  g = __builtin_fma(d, h, g);
  return x == 0.0 ? 0.0 : g;
}
// 1 / where(|v| == 0, 1, |v|) for d = |v|^2, the normalisation of the view vector V and the half
// vector H, by the correctly rounded cores. Not by rsq and Newton steps (~1 ulp) like the two above:
// N.V near grazing amplifies the shorter sequence's rounding (4 N.V + 1e-8 and G1(N.V) divide by it),
// and C4 and 1080p colour moved by 1.4e-12, over the 1e-12 parity bar, with V and H or H alone so.
__device__ __forceinline__ double inv_mag_shade(double d) {
  return d == 0.0 ? 1.0 : div_core(1.0, sqrt_core(d));
}

__device__ __forceinline__ double pow5(double x) {
  const double x2 = x * x;
  return (x2 * x2) * x;
}
__device__ __forceinline__ double pow25(double x) { return (x * x) * sqrt_shade(x); }

// A level's key: the hit sphere (RTX_MAX_SPHERES <= 2^kKeyShift) and its texture key above it.
constexpr int kKeyShift = 11;
__device__ __forceinline__ int level_key(int hit, int tk) { return hit | (tk << kKeyShift); }
__device__ __forceinline__ int key_hit(int key) { return key & ((1 << kKeyShift) - 1); }
__device__ __forceinline__ int key_tex(int key) { return (int)((unsigned)key >> kKeyShift); }
static_assert(RTX_MAX_SPHERES <= (1 << kKeyShift) && RTX_MAX_TEXELS <= (1 << (31 - kKeyShift)), "level key");

// Image texture (HipTexturedSphere / ImageTexture): the texel of hit point P on sphere (centre C)
// at the spherical coordinates of NumpyTexturedSphere.diffusecolor (shape.py:66-79): n = (P - C)
// normalised, u = 0.5 + atan2(n.z, n.x) / (2 pi), v = 0.5 - asin(n.y) / pi, each mod 1, texel
// (int(v (h-1)), int(u (w-1))). atan2/asin are ROCm's (not correctly rounded, like NumPy's), so
// a point within an ulp of a texel edge may take the neighbour texel: parity unpinned (the reference
// class cannot render).
template <typename T, typename G>
__device__ __forceinline__ int image_texel(const T* mh, const G* gh, double px, double py, double pz) {
  double nx = px - gh[RTX_G_CX], ny = py - gh[RTX_G_CY], nz = pz - gh[RTX_G_CZ];
  norm3(nx, ny, nz);
  double u = 0.5 + atan2(nz, nx) / (2.0 * RTX_PI);
  double v = 0.5 - asin(ny) / RTX_PI;
  u = u - floor(u);  // % 1 (Python / NumPy remainder: non-negative)
  v = v - floor(v);
  if (!(u >= 0.0 && u < 1.0)) u = 0.0;  // NaN (a degenerate point): texel 0
  if (!(v >= 0.0 && v < 1.0)) v = 0.0;
  const int w = (int)mh[RTX_M_TG], h = (int)mh[RTX_M_TB];
  const int i = (int)(u * (double)(w - 1)), j = (int)(v * (double)(h - 1));
  return j * w + i;
}

// The inputs of one shaded hit's colour terms (everything else comes from the material record).
struct Hit {
  double dli;    // max(N.L, 0)                                shader.py:138
  double di;     // sum_domes intensity * max(N.(0,1,0), 0)     shader.py:239-242
  double spec;   // physical specular (0 unless lit && g != 0)  shader.py:100-104
  double va;     // clip(N.V, 0, 1) (iridescence input)         shader.py:201
  double g;      // specular_gain
  int h;         // hit sphere
  int tk;        // texture key: the checker cell (shader.py:30) or the image texel (shape.py:66-79)
  bool lit;      //                                              shader.py:79-84
  double qx, qy, qz;  // nudged hit point = reflected ray origin  shader.py:77
  double nx, ny, nz;  // normal
};

// _calculate_physical_specular, shader.py:246-320, for unit-ish L (once normalised) and V.
// Sums of non-negative terms here and in hit_color are fused multiply-adds (one rounding fewer,
// within an ulp of the term; A/B r5e: C2 -1.6%, C2main -1.4%, C3 -1.2%, C4 -0.6%): none of them
// decides anything, and none cancels, so the colour moves by at most a few ulp.
template <typename M, typename Tm = double>
__device__ __forceinline__ double specular(const M* mh, double g, double nx, double ny, double nz, double lx,
                                           double ly, double lz, double vx, double vy, double vz, Tm tame = Tm()) {
  double Lx = lx, Ly = ly, Lz = lz;
  norm3_unit(Lx, Ly, Lz, tame);  // :278 (normalised a second time; an ulp of L moves a sharp highlight's
                           // D by ~2500 ulp: skipping it put main.py's 1080p frame 6e-10 off, r4s2)
  double Vx = vx, Vy = vy, Vz = vz;
  norm3_unit(Vx, Vy, Vz, tame);  // :279 (likewise)
  double Hx = Lx + Vx, Hy = Ly + Vy, Hz = Lz + Vz;
  {  // :280
    const double dh = dot3(Hx, Hy, Hz, Hx, Hy, Hz);
    const double rh = inv_mag_shade(dh);
    Hx = Hx * rh;
    Hy = Hy * rh;
    Hz = Hz * rh;
  }
  const double NdotV = clip01(dot3(nx, ny, nz, Vx, Vy, Vz));  // :283
  // :318 (the select at the end, taken early: a wave whose hits all face away from the camera
  // skips the rest; A/B C2 -0.2%, C2main -0.5%, C1 -0.8%)
  if (!(NdotV > 0.0)) return 0.0;
  const double NdotH = clip01(dot3(nx, ny, nz, Hx, Hy, Hz));  // :284
  const double VdotH = clip01(dot3(Vx, Vy, Vz, Hx, Hy, Hz));  // :285
  const double NdotL = clip01(dot3(nx, ny, nz, Lx, Ly, Lz));  // :287
  const double F = __builtin_fma(mh[RTX_M_1MF0], pow5(1.0 - VdotH), mh[RTX_M_F0]);  // :291
  const double a2 = mh[RTX_M_A2];
  const double denom = (NdotH * NdotH) * mh[RTX_M_A2M1] + 1.0;  // :295 (not fused: the sum cancels
  // to ~a^2 near the highlight's peak, and D amplifies the product's rounding by ~1/a^2)
  const double Dd = RTX_PI * __builtin_fma(denom, denom, 1e-8);  // :296
  const double oma2 = mh[RTX_M_1MA2];
  const double dL = (NdotL + sqrt_shade(__builtin_fma(oma2, NdotL * NdotL, a2))) + 1e-8;  // :299-301
  const double dV = (NdotV + sqrt_shade(__builtin_fma(oma2, NdotV * NdotV, a2))) + 1e-8;
  // G = G1L * G1V and spec_base = (F D G) / (4 N.V + 1e-8) with D = a2 / Dd: the four quotients
  // of :296-306 as two reciprocals (a few ulp, like the single quotients' Newton sequences; the
  // 1e-12 parity bar holds on every test and 8,600 random scenes)
  const double spec_base = ((F * a2) * ((2.0 * NdotL) * (2.0 * NdotV))) *
                           div_shade(1.0, (dL * dV) * (Dd * __builtin_fma(4.0, NdotV, 1e-8)));  // :303-306
  // (G = G1L G1V and spec_base = F D G / (4 N.V + 1e-8) with D = a2 / Dd share one reciprocal;
  // A/B r5h: C2 -0.6%, C3 -0.7%, C4 -0.5%)
  const double glint = pow25(1.0 - NdotV) * NdotL;  // :310-312
  const double sf = __builtin_fma(g, glint, spec_base);  // :315
  return (NdotV <= 0.0) ? 0.0 : sf;  // :318
}

// Colour of one shaded hit given the reflected colour R (shader.py:86-110):
//   ((((0.004 + diffuse) + dome) + (spec + R*0.5)*g*lit) + irid)
// `weighted` = lit && g != 0; otherwise the specular/reflection term is x*0 == 0 (R is finite).
// IMG: image textures are handled (the general kernel, and k_render_fast's texturing build for
// RTX_F_IMAGES launches); the other k_render_fast builds defer every pixel that meets an
// image-textured sphere and compile no texture lookup (A/B: carrying it cost C2 +3.4%, C2main +7%).
template <bool IMG = false, typename M, typename Tm = double>
__device__ __forceinline__ void hit_color(const M* mh, const cdouble* sc, double dli, double di, int tk, bool lit,
                                          bool weighted, double spec, double va, double Rr, double Rg, double Rb,
                                          double& cr, double& cg, double& cb, Tm tame = Tm()) {
  const double litf = lit ? 1.0 : 0.0;
  double tr, tg, tb;
  const double tex = mh[RTX_M_TEX];
  if (tex == RTX_TEX_CHECKER) {  // TextureChecker.get_color (:29-32): white * checker
    tr = tg = tb = tk ? 1.0 : 0.0;
  } else if (IMG && tex == RTX_TEX_IMAGE) {  // the texel shade() picked (texel table in the blob)
    const cdouble* t = sc + ((int64_t)mh[RTX_M_TR] + 3 * (int64_t)tk);
    tr = t[0];
    tg = t[1];
    tb = t[2];
  } else {  // Texture.get_color (:17-19)
    tr = mh[RTX_M_TR];
    tg = mh[RTX_M_TG];
    tb = mh[RTX_M_TB];
  }
  const double dg = mh[RTX_M_DG];
  // ambient + diffuse (:86-88, :138-141), dome (:98, :244)
  const double ar = __builtin_fma(sc[RTX_H_DOMEC + 0], di, __builtin_fma((tr * dli) * litf, dg, 0.004));
  const double ag = __builtin_fma(sc[RTX_H_DOMEC + 1], di, __builtin_fma((tg * dli) * litf, dg, 0.004));
  const double ab = __builtin_fma(sc[RTX_H_DOMEC + 2], di, __builtin_fma((tb * dli) * litf, dg, 0.004));
  // specular + reflection (:106)
  const double g = mh[RTX_M_G];
  const double xr = weighted ? (spec + Rr * 0.5) * g : 0.0;
  const double xg = weighted ? (spec + Rg * 0.5) * g : 0.0;
  const double xb = weighted ? (spec + Rb * 0.5) * g : 0.0;
  // thin-film iridescence (:186-232); zero when iridescence_gain == 0 (x * 0 == 0)
  double ir = 0.0, ig = 0.0, ib = 0.0;
  const double igain = mh[RTX_M_IG];
  if (igain != 0.0) {
    const double af = fabs(va - 0.5) * 2.0;  // :204
    const double phase = ((af * RTX_PI) * mh[RTX_M_TFT]) * 10.0;  // :208
    const double ip = sin_ref(sc, phase, tame);  // :211
    const double hs = mh[RTX_M_HS], omhs = mh[RTX_M_1MHS];
    const double r = __builtin_fma(ip, hs, omhs * (1.0 - ip));  // :221
    const double gg = __builtin_fma(ip, omhs, hs * (1.0 - ip));  // :222
    const double b = __builtin_fma(0.5, ip, 0.5);  // :223
    const double w = mh[RTX_M_TFW];
    ir = (r * w) * igain;  // :229-232
    ig = (gg * w) * igain;
    ib = (b * w) * igain;
  }
  cr = (ar + xr) + ir;
  cg = (ag + xg) + ig;
  cb = (ab + xb) + ib;
}

// ---- shadow grid (RTX_H_SHGRID, scene_pack._append_shadow_grid) ---------------------------
// The union, over the wave's lanes, of the masks of their shadow rays (origin q, direction L_dir):
// a lane whose q lies in the grid takes its voxel's mask (the spheres that may shadow any point of
// it); a lane outside takes the huge spheres' mask if its ray's line passes the small spheres'
// bounding ball at more than its radius plus the rounding reach (distance^2 from the centre: |w|^2 -
// (w.L_dir)^2, whose rounding, <= 4.4e-16 |w|^2, the 3e-8 (|w|^2 + 1) term covers; the host grows
// the radius by 1e-6 (|Cb| + Rb + 1), the lane adds 1e-6 |q| <= 5e-7 (|q|^2 + 1)). The wave-uniform
// own shape hs is removed. False (use the culling tree or the linear loop) when some lane fails
// both, has |N|^2 > 4 (the voxel masks' nudge bound) or NaNs, or when the lanes span more than
// kGridWaterfall distinct masks.
constexpr int kGridWaterfall = 16;  // (A/B r6ac/r6ad against 8: C4 -0.7/-1.0%, C3 -0.4%, C5 -1.1%; 32: C4 +-0)
__device__ __forceinline__ bool grid_mask(const cdouble* sc, double qx, double qy, double qz, double qq, double lx,
                                          double ly, double lz, double n2, int hs, uint64_t& m0, uint64_t& m1) {
  const cdouble* gr = sc + (int)sc[RTX_H_SHGRID];
  const double fx = (qx - gr[0]) * gr[3], fy = (qy - gr[1]) * gr[4], fz = (qz - gr[2]) * gr[5];
  const bool in = fx >= 0.0 && fx < gr[6] && fy >= 0.0 && fy < gr[7] && fz >= 0.0 && fz < gr[8] && n2 <= 4.0;
  const int nx = (int)gr[6], ny = (int)gr[7];
  int key = ((int)fz * ny + (int)fy) * nx + (int)fx;
  bool ok = in;
  if (!in) {
    const double wx = gr[9] - qx, wy = gr[10] - qy, wz = gr[11] - qz;
    const double ww = (wx * wx + wy * wy) + wz * wz;
    const double hh = (wx * lx + wy * ly) + wz * lz;
    const double R = (gr[12] + 5e-7 * (qq + 1.0)) + 3e-8 * (ww + 1.0);
    ok = ww - hh * hh > R * R;
    key = nx * ny * (int)gr[8];  // the huge spheres' mask
  }
  if (__ballot(!ok) != 0) return false;
  const cdouble* masks = gr + RTX_SHGRID_WORDS;
  m0 = 0;
  m1 = 0;
  bool pend = true;
  for (int it = 0;; ++it) {
    const uint64_t b = __ballot(pend);
    if (b == 0) break;
    if (it == kGridWaterfall) return false;
    const int k0 = __builtin_amdgcn_readlane(key, (int)__builtin_ctzll(b));
    m0 |= (uint64_t)__double_as_longlong(masks[2 * k0]);
    m1 |= (uint64_t)__double_as_longlong(masks[2 * k0 + 1]);
    pend = pend && key != k0;
  }
  if (hs < 64) m0 &= ~(uint64_t(1) << hs);
  else if (hs < 128) m1 &= ~(uint64_t(1) << (hs - 64));
  return true;
}

// The smallest valid root over the candidate spheres of masks m0/m1 (scene order, pairs) and
// whether there is one: the shadow test's candidates before t_self (shade's grid path).
template <typename G, typename Wk>
__device__ __forceinline__ void min_masked(const G* geo, uint64_t m0, uint64_t m1, double qx, double qy, double qz,
                                           double qq, double lx, double ly, double lz, double tame, double& tsh,
                                           bool& anyv, Wk& wk) {
  wk.test(__builtin_popcountll(m0) + __builtin_popcountll(m1));
  tsh = FARAWAY;
  anyv = false;
  for (int half = 0; half < 2; ++half) {
    uint64_t m = half ? m1 : m0;
    const int base = half * 64;
    while (m) {
      const int s0 = base + __builtin_ctzll(m);
      m &= m - 1;
      const SphTest a0 = isect_disc(geo + s0 * RTX_GEOM_WORDS, qx, qy, qz, qq, lx, ly, lz, tame);
      if (m) {
        const int s1 = base + __builtin_ctzll(m);
        m &= m - 1;
        isect_pair(a0, isect_disc(geo + s1 * RTX_GEOM_WORDS, qx, qy, qz, qq, lx, ly, lz, tame),
                   [&](double t0, bool v0, double t1, bool v1) {
                     if (v0) tsh = __builtin_fmin(tsh, t0);
                     if (v1) tsh = __builtin_fmin(tsh, t1);
                     anyv = anyv || v0 || v1;
                   });
      } else {
        isect_one(a0, [&](double t0, bool v0) {
          if (v0) tsh = __builtin_fmin(tsh, t0);
          anyv = anyv || v0;
        });
      }
    }
  }
}

// NumpyShader.create (shader.py:63-112) for a hit of sphere h at distance t, minus the colour
// assembly (hit_color) and the reflection recursion (driven by the caller).
// geo: scalar-cache view of the sphere table (wave-uniform loops); tab: the per-lane view of the
// same table (LDS copy or global).
// mat: a material record replacing sphere h's own (Shader.create on another shape's shader), or null.
// TREE = false: the scene has no culling tree (fewer than kTreeMinSpheres spheres), compiled out.
template <bool IMG = false, bool TREE = true, typename T, typename G, typename Wk, typename Tm>
__device__ __forceinline__ void shade(const cdouble* sc, const G* geo, const T* tab, int nsph, int h, double ox,
                                      double oy, double oz, double dx, double dy, double dz, double t, Hit& s,
                                      Tm tame, Wk& wk, const T* mat = nullptr) {
  const T* gh = tab + h * RTX_GEOM_WORDS;
  const T* mh = mat ? mat : tab + nsph * RTX_GEOM_WORDS + h * RTX_MAT_WORDS;
  const double px = ox + dx * t, py = oy + dy * t, pz = oz + dz * t;  // :73
  const double inv_r = gh[RTX_G_INVR];
  const double nx = (px - gh[RTX_G_CX]) * inv_r;  // :74 (not renormalised)
  const double ny = (py - gh[RTX_G_CY]) * inv_r;
  const double nz = (pz - gh[RTX_G_CZ]) * inv_r;
  double lx = sc[RTX_H_LIGHT + 0] - px, ly = sc[RTX_H_LIGHT + 1] - py, lz = sc[RTX_H_LIGHT + 2] - pz;
  norm3(lx, ly, lz, tame);  // :75
  const double qx = px + nx * 0.0001, qy = py + ny * 0.0001, qz = pz + nz * 0.0001;  // :77

  // _calculate_shadow (:114-128): lit == (t_self == min_j t_j), no light-distance cutoff.
  // Equivalent any-hit form: lit unless some sphere is strictly nearer than the shape itself.
  const double qq = dot3(qx, qy, qz, qx, qy, qz);
  // The shape's own test is t_self itself (same expression), and t_self < t_self never holds: when
  // every active lane hit the same sphere, the loops skip it (wave-uniform index remap below).
  const int h0 = __builtin_amdgcn_readfirstlane(h);
  const int hs = __ballot(h != h0) == 0 ? h0 : nsph;
  bool lit = true;
  uint64_t m0, m1;
  // The shadow grid (tame scenes: t_self < 2^62 < FARAWAY, so no lane is far_self): only the
  // candidate occluders are tested, and t_self only if there is one (with none, t_self is the
  // minimum whatever it is: lit). Scenes with a culling tree only: below kTreeMinSpheres the linear
  // loop is as cheap as the lookup (A/B: C2 +0.7%, C2main +2.7%, C1 +5% with the grid).
  if (TREE && sc[RTX_H_SHGRID] != 0.0 && sc[RTX_H_TAME] != 0.0 &&
      grid_mask(sc, qx, qy, qz, qq, lx, ly, lz, dot3(nx, ny, nz, nx, ny, nz), hs, m0, m1)) {
    wk.node();  // the voxel lookup, priced as one node test
    if ((m0 | m1) != 0) {
      // the candidates first (each lane's smallest valid root), t_self only where some lane has one:
      // lit <=> no valid candidate root below t_self, and a lane without one is lit whatever t_self is
      // (round 6, as the small-scene loop below; A/B r6z: C4 -2.0%, C3 -0.4%, C5 within noise)
      double tsh;
      bool anyv;
      min_masked(geo, m0, m1, qx, qy, qz, qq, lx, ly, lz, tame, tsh, anyv, wk);
      if (__ballot(anyv) != 0) {
        const double tself = isect_t(gh, qx, qy, qz, qq, lx, ly, lz, tame);
        wk.test(1);
        lit = !(anyv && tsh < tself);
      }
    }
  } else if (!TREE && (kSticky<Tm> || sc[RTX_H_TAME] != 0.0)) {  // (the optimistic body: tame launches only)
    // Scenes without a culling tree, tame: the other spheres first, and t_self only when some lane
    // has a valid root (t_self < 2^62 < FARAWAY in a tame scene, so an invalid test never shadows
    // and a lane without a valid root is lit whatever t_self is). lit <=> no valid root strictly
    // below t_self <=> !(smallest valid root < t_self); a lane's own shape, tested when the wave's
    // shapes differ, gives t_self itself, which is not below it.
    const int nshadow = nsph - (hs < nsph);
    double tsh = FARAWAY;
    bool anyv = false;
    int j = 0;
    for (; j + 1 < nshadow; j += 2) {  // (written out, not scan_range: the skip-hs remap takes both indices)
      const G* g0 = geo + __builtin_amdgcn_readfirstlane(j + (j >= hs)) * RTX_GEOM_WORDS;
      const G* g1 = geo + __builtin_amdgcn_readfirstlane(j + 1 + (j + 1 >= hs)) * RTX_GEOM_WORDS;
      wk.test(2);
      isect_pair(isect_disc(g0, qx, qy, qz, qq, lx, ly, lz, tame), isect_disc(g1, qx, qy, qz, qq, lx, ly, lz, tame),
                 [&](double t0, bool v0, double t1, bool v1) {
                   if (v0) tsh = __builtin_fmin(tsh, t0);
                   if (v1) tsh = __builtin_fmin(tsh, t1);
                   anyv = anyv || v0 || v1;
                 });
    }
    if (j < nshadow) {
      const G* g0 = geo + __builtin_amdgcn_readfirstlane(j + (j >= hs)) * RTX_GEOM_WORDS;
      wk.test(1);
      isect_one(isect_disc(g0, qx, qy, qz, qq, lx, ly, lz, tame), [&](double t0, bool v0) {
        if (v0) tsh = __builtin_fmin(tsh, t0);
        anyv = anyv || v0;
      });
    }
    if (__ballot(anyv) != 0) {
      const double tself = isect_t(gh, qx, qy, qz, qq, lx, ly, lz, tame);
      wk.test(1);
      lit = !(anyv && tsh < tself);
    }
  } else {
    const double tself = isect_t(gh, qx, qy, qz, qq, lx, ly, lz, tame);
    wk.test(1);
    // t_self beyond FARAWAY (a hit past the reference's sentinel distance): every missing sphere
    // shadows. The linear loop handles it exactly; the culling tree skips missing spheres, so such
    // a wave takes the linear loop.
    const bool far_self = tself > FARAWAY;
    const bool culled = TREE && sc[RTX_H_NNODES] != 0.0 && __ballot(far_self) == 0;
    if (culled) lit = lit_bvh(sc, qx, qy, qz, qq, lx, ly, lz, tself, hs, tame, wk);
    const int nshadow = culled ? 0 : nsph - (hs < nsph);
    int j = 0;
    for (; j + 1 < nshadow; j += 2) {  // (written out: the remap as above, and a lane leaves at its first shadow)
      const int j0 = __builtin_amdgcn_readfirstlane(j + (j >= hs));
      const int j1 = __builtin_amdgcn_readfirstlane(j + 1 + (j + 1 >= hs));
      const G* g0 = geo + j0 * RTX_GEOM_WORDS;
      const G* g1 = geo + j1 * RTX_GEOM_WORDS;
      wk.test(2);
      bool sh = far_self;  // lanes without a valid root in either test
      isect_pair(isect_disc(g0, qx, qy, qz, qq, lx, ly, lz, tame), isect_disc(g1, qx, qy, qz, qq, lx, ly, lz, tame),
                 [&](double t0, bool v0, double t1, bool v1) {
                   sh = shadows(v0, t0, tself, far_self) || shadows(v1, t1, tself, far_self);
                 });
      if (sh) {
        lit = false;
        break;
      }
    }
    if (lit && j < nshadow) {
      const G* g0 = geo + __builtin_amdgcn_readfirstlane(j + (j >= hs)) * RTX_GEOM_WORDS;
      wk.test(1);
      bool sh = far_self;
      isect_one(isect_disc(g0, qx, qy, qz, qq, lx, ly, lz, tame),
                [&](double t0, bool v0) { sh = shadows(v0, t0, tself, far_self); });
      if (sh) lit = false;
    }
  }

  const double dli = max0(dot3(nx, ny, nz, lx, ly, lz));  // :138
  // dome (:239-242): light_direction (0, 1, 0)
  // N.(0, 1, 0) = ((nx*0) + ny*1) + nz*0 is ny itself for finite N (N is finite: P and C are), up to
  // the sign of a zero, which max0 and the sum below (0.0 + I*(+-0) = +0) erase
  const double up = ny;
  const int ndome = (int)sc[RTX_H_NDOME];
  double di = 0.0;
  for (int j = 0; j < ndome; ++j) di = di + sc[RTX_H_DOMEI + j] * max0(up);

  const double g = mh[RTX_M_G];
  const bool weighted = lit && g != 0.0;
  const bool need_irid = mh[RTX_M_IG] != 0.0;
  double spec = 0.0, va = 0.0;
  if (weighted || need_irid) {
    double vx = sc[RTX_H_CAM + 0] - px, vy = sc[RTX_H_CAM + 1] - py, vz = sc[RTX_H_CAM + 2] - pz;
    {  // :76 (towards the camera on every level); V only feeds the specular and the iridescence
      const double rv = inv_mag_shade(dot3(vx, vy, vz, vx, vy, vz));
      vx = vx * rv;
      vy = vy * rv;
      vz = vz * rv;
    }
    if (weighted) spec = specular(mh, g, nx, ny, nz, lx, ly, lz, vx, vy, vz, tame);
    if (need_irid) va = clip01(dot3(nx, ny, nz, vx, vy, vz));  // :201
  }
  s.dli = dli;
  s.di = di;
  s.spec = spec;
  s.va = va;
  s.g = g;
  s.h = h;
  const double tex = mh[RTX_M_TEX];
  s.tk = tex == RTX_TEX_CHECKER ? (trunc_parity(px * 2.0) == trunc_parity(pz * 2.0))  // :30
         : tex != RTX_TEX_IMAGE ? 0
         : IMG ? image_texel(mh, gh, px, py, pz) : -1;  // -1: an untextured k_render_fast build defers the ray
  s.lit = lit;
  s.qx = qx; s.qy = qy; s.qz = qz;
  s.nx = nx; s.ny = ny; s.nz = nz;
}

// Reflected direction (shader.py:151): norm(D - (N*2) * (D.N))
template <typename Tm = double>
__device__ __forceinline__ void reflect_dir(double& dx, double& dy, double& dz, double nx, double ny, double nz,
                                            Tm tame = Tm()) {
  const double dn = dot3(dx, dy, dz, nx, ny, nz);
  double rx = dx - (nx * 2.0) * dn, ry = dy - (ny * 2.0) * dn, rz = dz - (nz * 2.0) * dn;
  norm3_unit(rx, ry, rz, tame);  // |D| = |N| = 1 up to rounding, so |R| too
  dx = rx;
  dy = ry;
  dz = rz;
}

// ------------------------------------------------------------------------------------------
// ray setup / output
// ------------------------------------------------------------------------------------------

__device__ __forceinline__ int global_row(const Params& p, int lr) {
  if (p.n_parts == 1) return lr;  // a whole frame (uniform branch: no integer divisions)
  // a run of part_run consecutive parts owns part_run * row_block consecutive rows of every cycle of
  // n_parts * row_block rows, from row part * row_block of the cycle (part_run == 1: one row block)
  const int own = p.row_block * p.part_run;
  return (lr / own) * (p.n_parts * p.row_block) + p.part * p.row_block + (lr % own);
}

// get_ray_directions (base.py:123-141) for pixel (col, global row r).
template <typename Tm = double>
__device__ __forceinline__ void camera_dir(const cdouble* sc, int col, int r, int W, int H, double& dx, double& dy,
                                           double& dz, Tm tame = Tm()) {
  // np.linspace: i*step + start, last element set to stop exactly
  const double x = (sc[RTX_H_XFIX] != 0.0 && col == W - 1) ? sc[RTX_H_XSTOP]
                                                            : (double)col * sc[RTX_H_XSTEP] + sc[RTX_H_XSTART];
  const double y = (sc[RTX_H_YFIX] != 0.0 && r == H - 1) ? sc[RTX_H_YSTOP]
                                                          : (double)r * sc[RTX_H_YSTEP] + sc[RTX_H_YSTART];
  const double vx = x - sc[RTX_H_CAM + 0];
  const double vy = y - sc[RTX_H_CAM + 1];
  const double vz = sc[RTX_H_VZ];
  const double rr = inv_mag(((vx * vx) + (vy * vy)) + sc[RTX_H_VZ2], tame);
  dx = vx * rr;
  dy = vy * rr;
  dz = vz * rr;
}
// camera_dir of the small-scene kernels (a function of its own, so that every other
// caller compiles from unchanged text). inner (wave-uniform): no lane of the wave is in the frame's
// last column or row, so the linspace stops are not even asked about; the other waves take the selects
// above with the fix words read by their bits.
template <typename Tm>
__device__ __forceinline__ void camera_dir_small(const cdouble* sc, int col, int r, int W, int H, bool inner,
                                                 double& dx, double& dy, double& dz, Tm tame) {
  double x, y;
  if (inner) {
    x = (double)col * sc[RTX_H_XSTEP] + sc[RTX_H_XSTART];
    y = (double)r * sc[RTX_H_YSTEP] + sc[RTX_H_YSTART];
  } else {
    x = (f64_nonzero_bits(sc[RTX_H_XFIX]) && col == W - 1) ? sc[RTX_H_XSTOP]
                                                            : (double)col * sc[RTX_H_XSTEP] + sc[RTX_H_XSTART];
    y = (f64_nonzero_bits(sc[RTX_H_YFIX]) && r == H - 1) ? sc[RTX_H_YSTOP]
                                                          : (double)r * sc[RTX_H_YSTEP] + sc[RTX_H_YSTART];
  }
  const double vx = x - sc[RTX_H_CAM + 0];
  const double vy = y - sc[RTX_H_CAM + 1];
  const double vz = sc[RTX_H_VZ];
  const double rr = inv_mag(((vx * vx) + (vy * vy)) + sc[RTX_H_VZ2], tame);
  dx = vx * rr;
  dy = vy * rr;
  dz = vz * rr;
}

// the camera ray of pixel (col, local row lr) of the launch's tile
template <typename Tm = double>
__device__ __forceinline__ void camera_ray(const Params& p, int col, int lr, double& ox, double& oy, double& oz,
                                           double& dx, double& dy, double& dz, Tm tame = Tm()) {
  const cdouble* sc = (const cdouble*)p.scene;
  camera_dir(sc, col, global_row(p, lr), p.width, p.height, dx, dy, dz, tame);
  ox = sc[RTX_H_CAM + 0];
  oy = sc[RTX_H_CAM + 1];
  oz = sc[RTX_H_CAM + 2];
}

// spheres [nb, nsph) are all huge (RTX_H_NBEAM): candidates of every tile and beam without a test
__device__ __forceinline__ int huge_tail(const cdouble* sc, int nsph) {
  const int nb = (int)sc[RTX_H_NBEAM];
  return nb > 0 && nb < nsph ? nb : nsph;
}

// ---- level-0 candidates of a wave tile ------------------------------------------------------
// The camera rays of a wave's pixels leave one origin O through points (x, y, 0) of the image
// plane (camera_dir, base.py:123-141), and x (y) is monotone in the column (row), so the plane
// points of the tile's lanes lie in the rectangle of its extreme columns and rows (a lane's ray
// passes through O + (fl(x - Ox), fl(y - Oy), VZ), within an ulp of (x, y, 0)). The host gives every
// sphere an image-plane box for this camera (RTX_H_SBOX, scene_pack.sphere_plane_boxes): a camera
// ray through a plane point outside it yields FARAWAY for that sphere. The box is built from the
// sphere's radius expanded by the culling margin lm (node_may_hit: a root the reference reports lies
// within lm of the ball), with scale = |C - O|^2 + 2|C|^2 + 3r^2 + |O|^2 (>= node_may_hit's scale for
// a single sphere) and lm = 1e-7 (scale + 1), doubled like the node margin: that also absorbs
// |D| = 1 +- 1e-15 and the plane point's ulp. A sphere whose box misses the tile's rectangle is
// skipped by the tile's level-0 nearest hit: the nearest hit and the tie flag are unchanged.
// Comparisons are written so that NaN keeps the sphere; the huge tail (RTX_H_NBEAM) is kept without
// a test. One lane tests one sphere (two passes for 65..128 spheres); the ballots are the tile's
// candidate masks. Needs the full wave (call before any lane diverges). (Rounds 3-4 tested each
// sphere against the tile's four frustum planes, ~40 VALU a lane; A/B r5q: the boxes take C3 -7.6%,
// C4 -4.9%, C5 -3.8%.)
__device__ __forceinline__ bool wave_frustum(const Params& p, int c0, int lr0, uint64_t& m0, uint64_t& m1) {
  const cdouble* sc = (const cdouble*)p.scene;
  const int W = p.width;
  if (c0 >= W || lr0 >= p.n_rows) return false;  // no pixel of this wave lies in the frame
  const int c1 = c0 + kWaveW - 1 < W - 1 ? c0 + kWaveW - 1 : W - 1;
  const int l1 = lr0 + kWaveH - 1 < p.n_rows - 1 ? lr0 + kWaveH - 1 : p.n_rows - 1;
  const int H = p.height;
  auto xv = [&](int c) {
    return (sc[RTX_H_XFIX] != 0.0 && c == W - 1) ? sc[RTX_H_XSTOP] : (double)c * sc[RTX_H_XSTEP] + sc[RTX_H_XSTART];
  };
  auto yv = [&](int r) {
    return (sc[RTX_H_YFIX] != 0.0 && r == H - 1) ? sc[RTX_H_YSTOP] : (double)r * sc[RTX_H_YSTEP] + sc[RTX_H_YSTART];
  };
  const double xa = xv(c0), xb = xv(c1), ya = yv(global_row(p, lr0)), yb = yv(global_row(p, l1));
  const double xlo = __builtin_fmin(xa, xb), xhi = __builtin_fmax(xa, xb);
  const double ylo = __builtin_fmin(ya, yb), yhi = __builtin_fmax(ya, yb);
  const double* bx = p.scene + (int64_t)sc[RTX_H_SBOX];  // per-lane loads: a generic pointer
  const int lane = (int)__lane_id();
  const int nb = huge_tail(sc, p.nsph);
  auto may = [&](int s) {
    if (s >= p.nsph) return false;
    if (s >= nb) return true;
    const double* e = bx + 4 * s;
    return !(e[1] < xlo || e[0] > xhi || e[3] < ylo || e[2] > yhi);
  };
  m0 = __ballot(may(lane));
  // the second pass only when a sphere above 63 needs its test (C4: 65 spheres, the 65th the ground)
  m1 = p.nsph <= 64 ? 0ull
       : nb > 64    ? __ballot(may(64 + lane))
                    : (p.nsph >= 128 ? ~0ull : (uint64_t(1) << (p.nsph - 64)) - 1);
  return true;
}

// Nearest hit over the candidate spheres of masks m0 (spheres 0..63) and m1 (64..127), in scene
// order, pairs at a time like nearest_hit. CAM: camera rays (level 0, the host's c).
template <bool CAM, typename P, typename Wk>
__device__ __forceinline__ void nearest_masked(const P* geo, uint64_t m0, uint64_t m1, double ox, double oy,
                                               double oz, double dx, double dy, double dz, double& tmin, int& hit,
                                               bool& tie, double tame, Wk& wk) {
  wk.test(__builtin_popcountll(m0) + __builtin_popcountll(m1));
  tmin = FARAWAY;
  hit = -1;
  tie = false;
  const double oo = CAM ? 0.0 : dot3(ox, oy, oz, ox, oy, oz);
  auto disc = [&](const P* g) {
    return CAM ? isect_disc_cam(g, ox, oy, oz, dx, dy, dz, tame) : isect_disc(g, ox, oy, oz, oo, dx, dy, dz, tame);
  };
  auto run = [&](uint64_t m, int base) {
    while (m) {
      const int s0 = base + __builtin_ctzll(m);
      m &= m - 1;
      const P* g0 = geo + s0 * RTX_GEOM_WORDS;
      const SphTest a0 = disc(g0);
      if (m) {
        const int s1 = base + __builtin_ctzll(m);
        m &= m - 1;
        const SphTest a1 = disc(geo + s1 * RTX_GEOM_WORDS);
        isect_pair(a0, a1, [&](double t0, bool v0, double t1, bool v1) {
          nearest_update(v0, t0, s0, tmin, hit, tie);
          nearest_update(v1, t1, s1, tmin, hit, tie);
        });
      } else {
        isect_one(a0, [&](double t0, bool v0) { nearest_update(v0, t0, s0, tmin, hit, tie); });
      }
    }
  };
  run(m0, 0);
  run(m1, 64);
}

// ---- candidates of a wave's reflected rays (levels >= 1 of tree scenes) --------------------------
// The wave's active rays (O, D) leave from a ball around the first active lane's origin Oc, of
// radius rho >= |O - Oc|, in directions within angle theta of that lane's direction A
// (1 - cos theta >= 1 - D.A in every lane). A point X = O + tD (t > 0) within R' of a centre C puts
// Oc + tD within R = R' + rho of it, so D lies within phi = asin(R / |W|) of W = C - Oc and A
// within theta + phi: A.W >= |W| cos(theta + phi) = cos theta sqrt(|W|^2 - R^2) - sin theta R
// (theta, phi <= 90 degrees). With R' = r + lm (the culling margin of wave_frustum, doubled again and
// taken over the whole ball: |C - O|^2 <= 2|W|^2 + 2 rho^2, |O|^2 <= 2|Oc|^2 + 2 rho^2), a sphere
// failing that test (and not reaching the ball itself) yields FARAWAY for every ray of the wave, so
// the nearest hit (and the tie flag) over the others is unchanged. The test is evaluated squared,
// without a square root of |W|^2 - R^2 (round 6): with t1 = A.W + sin theta R (plus an absolute
// slack for its rounding), a sphere is dropped when t1 < 0 (the right side is >= 0) or when
// t1^2 < (|W|^2 - R^2) cos^2 theta, the difference lowered by its rounding bound and the product
// by a relative 1e-12, so every rounding keeps the sphere. rho^2 and 1 - cos theta are bounded by
// powers of two, the wave maxima of the lanes' exponents (wave_max_jump: exact under any exec mask,
// no cross-lane arithmetic). Comparisons keep the sphere on NaN.
// Only the active lanes run here (the bounce loop's lanes leave it one by one), so the spheres are
// dealt out by rank: the active lane of rank k tests spheres k, k + n, k + 2n (n active lanes), and
// pass j's ballot holds sphere j n + rank(lane) at the lane's bit. False (take the culling tree)
// when that needs more than kBeamPasses passes, the beam is wider than 60 degrees, the ball larger
// than 2^6 or the candidates more than kBeamMaxCand.
constexpr int kBeamPasses = 3;
constexpr int kBeamMaxCand = 24;
// The beam kernels with an LDS copy of the sphere table stage in it each sphere's own part of the
// test's radius, in geometry word RTX_G_IDX (unused in the main table): r (bounded above) plus the
// margin's per-sphere terms, beam_word below. The per-lane test then needs no square root of its own.
// (Without the copy, LDS = false: more than kLdsMaxSpheres spheres, the test computes that part itself.)
static_assert(RTX_GEOM_WORDS == 8 && RTX_G_IDX == 7, "beam word: the last geometry word");
struct Beam {
  uint64_t m[kBeamPasses];  // pass j: candidate bits at the testing lanes' positions
  uint64_t ex;              // the active lanes
  int n;                    // their count
  int passes;
  int nb;                   // spheres [nb, nsph): the huge tail, candidates without a test
};
__device__ __forceinline__ double rfl_d(double x) {
  const int hi = __builtin_amdgcn_readfirstlane(__double2hiint(x));
  const int lo = __builtin_amdgcn_readfirstlane(__double2loint(x));
  return __hiloint2double(hi, lo);
}
// Max over the active lanes of a small int v: start from the last active lane's value and jump to
// a larger value some lane holds until no lane holds one (exact under any exec mask; one or two
// ballots for the nearby origins and directions of a wave tile, where the binary search of rounds
// 3-5 took seven and six).
__device__ __forceinline__ int wave_max_jump(int v) {
  const uint64_t ex = __ballot(1);
  int cur = __builtin_amdgcn_readlane(v, 63 - __builtin_clzll(ex));
  for (;;) {
    const uint64_t b = __ballot(v > cur);
    if (b == 0) return cur;
    cur = __builtin_amdgcn_readlane(v, __builtin_ctzll(b));
  }
}
// e with x < 2^e for x in [0, 2^hi): exponents below lo report lo; NaN and anything larger hi + 1
__device__ __forceinline__ int pow2_above(double x, int lo, int hi) {
  if (!(x < __builtin_ldexp(1.0, hi))) return hi + 1;
  if (x < __builtin_ldexp(1.0, lo - 1)) return lo;
  const int e = __builtin_amdgcn_frexp_exp(x);  // x = m 2^e, m in [0.5, 1)
  return e < lo ? lo : e;
}
// sqrt for the beam's culling test: the hardware reciprocal square root (~2^-24 relative) and one
// Newton step (~1e-15 relative: quadratic in the estimate's error); callers scale by 1 + 1e-11
// towards keeping the sphere. 0 and inf give NaN, which the test's comparisons read as "keep".
__device__ __forceinline__ double sqrt_cull(double x) {
  const double y = __builtin_amdgcn_rsq(x);
  return x * (y * __builtin_fma(-0.5 * x * y, y, 1.5));
}
// r (bounded above) + 4e-7 (2 C.C + 3 r^2) (1 + 1e-12): the sphere's own part of R (the same sum as
// wave_beam's unstaged R, reassociated; the test's outer 1 + 1e-12 covers the reassociation)
__device__ __forceinline__ double beam_word(double cc, double rr) {
  return sqrt_cull(rr) * (1.0 + 1e-11) + 4e-7 * ((2.0 * cc + 3.0 * rr) * (1.0 + 1e-12));
}
// STAGED: tab is the LDS copy whose word RTX_G_IDX holds beam_word (k_render_fast's staging loop)
template <bool STAGED, typename T>
__device__ __forceinline__ bool wave_beam(const T* tab, int nb, double ox, double oy, double oz, double dx,
                                          double dy, double dz, Beam& bm) {
  bm.ex = __ballot(1);
  bm.n = __builtin_popcountll(bm.ex);
  bm.nb = nb;
  bm.passes = (nb + bm.n - 1) / bm.n;  // the huge tail [nb, nsph) is dealt out to nobody
  if (bm.passes > kBeamPasses) return false;
  const double Ox = rfl_d(ox), Oy = rfl_d(oy), Oz = rfl_d(oz);
  const double Ax = rfl_d(dx), Ay = rfl_d(dy), Az = rfl_d(dz);
  const double wox = ox - Ox, woy = oy - Oy, woz = oz - Oz;
  const int er = wave_max_jump(pow2_above((wox * wox + woy * woy) + woz * woz, -60, 12));
  const double omc = 1.0 - ((dx * Ax + dy * Ay) + dz * Az);
  const int ea = wave_max_jump(pow2_above(omc, -60, -1));
  if (er > 12 || ea > -1) return false;
  const double rho2 = __builtin_ldexp(1.0, er);                 // > |O - Oc|^2 in every lane
  const double rho = sqrt_cull(rho2) * (1.0 + 1e-11);            // >= its square root
  const double ct = 1.0 - __builtin_ldexp(1.0, ea);              // <= cos theta (>= 1/2)
  const double ct2 = (ct * ct) * (1.0 - 1e-12);                  // <= cos^2 theta
  const double st = sqrt_cull(__builtin_ldexp(1.0, ea + 1)) * (1.0 + 1e-11);  // >= sin theta
  // the margin's terms common to every sphere: 2 rho^2 of |C - O|^2 and the bound on |O|^2
  const double lmk = ((2.0 * rho2 + 2.0 * ((Ox * Ox + Oy * Oy) + Oz * Oz)) + 2.0 * rho2) + 1.0;
  const int rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(bm.ex >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)bm.ex, 0));
  auto may = [&](int s) {
    if (s >= nb) return false;
    const T* e = tab + s * RTX_GEOM_WORDS;
    const double wx = e[RTX_G_CX] - Ox, wy = e[RTX_G_CY] - Oy, wz = e[RTX_G_CZ] - Oz;
    const double ww = (wx * wx + wy * wy) + wz * wz;  // |W|^2
    double R;
    if constexpr (STAGED) {
      R = ((e[RTX_G_IDX] + 4e-7 * ((2.0 * ww + lmk) * (1.0 + 1e-12))) + rho) * (1.0 + 1e-12);
    } else {
      const double rr = e[RTX_G_RR];
      const double lm = 4e-7 * ((((2.0 * ww + 2.0 * e[RTX_G_CC]) + 3.0 * rr) + lmk) * (1.0 + 1e-12));
      R = ((sqrt_cull(rr) * (1.0 + 1e-11) + lm) + rho) * (1.0 + 1e-12);
    }
    const double R2 = R * R;
    if (!(ww > R2 * (1.0 + 1e-12))) return true;  // the ball may reach the sphere
    const double aw = (Ax * wx + Ay * wy) + Az * wz;
    const double t1 = (aw + st * R) + 1e-9 * ((ww + R2) + 2.0);  // (the slack: >= 1e-9 (|W| + R + 1))
    if (t1 < 0.0) return false;
    return !(t1 * t1 < (((ww - R2) - 1e-15 * (ww + R2)) * ct2));
  };
  int cand = 0;
#pragma unroll
  for (int j = 0; j < kBeamPasses; ++j) {
    bm.m[j] = j < bm.passes ? __ballot(may(j * bm.n + rank)) : 0ull;
    cand += __builtin_popcountll(bm.m[j]);
  }
  return cand <= kBeamMaxCand;
}

// Nearest hit over a wave beam's candidates (pass j, bit b: sphere j n + popcount(ex below b)),
// pairs at a time like nearest_hit; in scene order.
template <typename P, typename Wk>
__device__ __forceinline__ void nearest_beam(const P* geo, int nsph, const Beam& bm, double ox, double oy, double oz,
                                             double dx, double dy, double dz, double& tmin, int& hit, bool& tie,
                                             double tame, Wk& wk) {
  tmin = FARAWAY;
  hit = -1;
  tie = false;
  const double oo = dot3(ox, oy, oz, ox, oy, oz);
  auto sph = [&](uint64_t& m, int base) {
    const int b = __builtin_ctzll(m);
    m &= m - 1;
    return base + __builtin_popcountll(bm.ex & ((uint64_t(1) << b) - 1));
  };
#pragma unroll
  for (int j = 0; j < kBeamPasses; ++j) {
    uint64_t m = bm.m[j];
    wk.test(__builtin_popcountll(m));
    const int base = j * bm.n;
    while (m) {
      const int s0 = sph(m, base);
      const SphTest a0 = isect_disc(geo + s0 * RTX_GEOM_WORDS, ox, oy, oz, oo, dx, dy, dz, tame);
      if (m) {
        const int s1 = sph(m, base);
        const SphTest a1 = isect_disc(geo + s1 * RTX_GEOM_WORDS, ox, oy, oz, oo, dx, dy, dz, tame);
        isect_pair(a0, a1, [&](double t0, bool v0, double t1, bool v1) {
          nearest_update(v0, t0, s0, tmin, hit, tie);
          nearest_update(v1, t1, s1, tmin, hit, tie);
        });
      } else {
        isect_one(a0, [&](double t0, bool v0) { nearest_update(v0, t0, s0, tmin, hit, tie); });
      }
    }
  }
  // the huge tail, tested by every ray (wave-uniform bounds)
  wk.test(nsph - bm.nb);
  int s = bm.nb;
  for (; s + 1 < nsph; s += 2) {
    const P* g0 = geo + s * RTX_GEOM_WORDS;
    const SphTest a0 = isect_disc(g0, ox, oy, oz, oo, dx, dy, dz, tame);
    const SphTest a1 = isect_disc(g0 + RTX_GEOM_WORDS, ox, oy, oz, oo, dx, dy, dz, tame);
    isect_pair(a0, a1, [&](double t0, bool v0, double t1, bool v1) {
      nearest_update(v0, t0, s, tmin, hit, tie);
      nearest_update(v1, t1, s + 1, tmin, hit, tie);
    });
  }
  if (s < nsph) {
    const SphTest a0 = isect_disc(geo + s * RTX_GEOM_WORDS, ox, oy, oz, oo, dx, dy, dz, tame);
    isect_one(a0, [&](double t0, bool v0) { nearest_update(v0, t0, s, tmin, hit, tie); });
  }
}

__device__ __forceinline__ void load_ray(const Params& p, int64_t i, double& ox, double& oy, double& oz, double& dx,
                                         double& dy, double& dz) {
  if (p.mode == 0) {
    camera_ray(p, (int)(i % p.width), (int)(i / p.width), ox, oy, oz, dx, dy, dz);
  } else {
    const int64_t n = p.n;
    dx = p.dir[i];
    dy = p.dir[n + i];
    dz = p.dir[2 * n + i];
    const int64_t s = p.org_stride;
    const int64_t j = s ? i : 0;
    ox = p.org[j];
    oy = p.org[s + j + (s ? 0 : 1)];
    oz = p.org[2 * s + j + (s ? 0 : 2)];
  }
}

__device__ __forceinline__ unsigned char quant_u8(double c) {
  // (255 * np.clip(c, 0, 1)).astype(np.uint8)  (base.py:147): truncation (NaN -> 0)
  const double v = 255.0 * clip01(c);
  return v >= 0.0 ? (unsigned char)(int)v : (unsigned char)0;
}

// The lane's index in its wave by two VALU instructions the compiler cannot merge with an earlier
// lane id, so that a value derived from it is recomputed instead of kept live (fast_tile's tail).
__device__ __forceinline__ int lane_id_fresh() {
  int l;
  asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(l));
  return l;
}

// (the colour by reference: fast_tile's accumulators then stay memory objects until this call is
// inlined, and are promoted to registers together with the level's colour; taken by value they are
// promoted one pass earlier and the one-tile culled kernels come out scheduled differently: A/B,
// identical frames, C3 +0.4%)
__device__ __forceinline__ void write_out(const Params& p, int64_t i, const double& r, const double& g,
                                          const double& b) {
  // the frame is written once and never read back by the kernel: streaming (nontemporal) stores
  // (A/B, identical output: C5 -1.5..-1.9%, C3 -0.9%, C2 -0.4..-0.8%)
  if (p.out_kind == RTX_OUT_F32_SOA) {
    float* o = (float*)p.out;
    __builtin_nontemporal_store((float)r, o + i);
    __builtin_nontemporal_store((float)g, o + p.n + i);
    __builtin_nontemporal_store((float)b, o + 2 * p.n + i);
  } else if (p.out_kind == RTX_OUT_F64_SOA) {
    double* o = (double*)p.out;
    __builtin_nontemporal_store(r, o + i);
    __builtin_nontemporal_store(g, o + p.n + i);
    __builtin_nontemporal_store(b, o + 2 * p.n + i);
  } else {
    unsigned char* o = (unsigned char*)p.out + 3 * i;
    o[0] = quant_u8(r);
    o[1] = quant_u8(g);
    o[2] = quant_u8(b);
  }
}

__device__ __forceinline__ void stat_add(unsigned long long* st, int word, unsigned long long v) {
  atomicAdd(st + word, v);
}

// one count per wave (from its first active lane): how many waves execute a stage
__device__ __forceinline__ void stat_wave(unsigned long long* st, int word) {
  const unsigned long long m = __ballot(1);
  if ((int)__lane_id() == __ffsll((long long)m) - 1) atomicAdd(st + word, 1ull);
}

// ------------------------------------------------------------------------------------------
// k_render_fast<B, LDS, DEEP>
// ------------------------------------------------------------------------------------------

// One block tile: (bx, by) in camera mode, block bx of 256 rays (64 in the small-scene kernels) in
// explicit-ray mode, as many entries of in_list in continuation mode. The level-0 nearest-hit test
// reads the scalar cache only, so the LDS table need not be complete before stage(hit) (fast_tile:
// the block's barrier on its first tile; small_wave: the wave's own late staging). DEEP (caps above RTX_FAST_MAX_BOUNCES or none): chains
// still alive at the launch's record level are deferred with a resume record, and the continuation
// mode exists; the capped instantiations compile none of it.
// IMG: image-textured spheres are shaded here (the texel lookup compiled in, RTX_F_IMAGES launches)
// instead of deferred to the general kernel.
// NSPH > 0: the scene has exactly NSPH spheres, a compile-time count (the timed small-scene kernels,
// rtx_small.hip: their sphere loops unroll; A/B r6b, C2 -2.7%); 0: p.nsph at run time.
// guard: a double (ignored) renders the tile through the guarded helpers and returns false. A Sticky
// (small_tile, DEEP 0 only) renders it through their unconditional fast cores; if some lane's flag is
// set after the bounce loop the whole wave returns true, before anything is written or appended: the
// caller renders the tile again, guarded.
// stage(hit): called by the whole wave after the level-0 search, before any lane uses the LDS table.
template <int B, bool LDS, int DEEP, bool STATS, bool TREE, bool BEAM, bool IMG = false, int NSPH = 0,
          typename Tm, typename Stage>
__device__ __forceinline__ bool fast_tile_body(const Params& p, int bx, int by, const double* lds_tab,
                                               bool wave_tile, Tm guard, Stage&& stage) {
  static_assert(!kSticky<Tm> || (DEEP == 0 && !TREE && !STATS), "the optimistic body: capped, counter-free, TP 0");
  constexpr int FB = fast_block<TREE>();  // threads per block of this instantiation
  const cdouble* sc = (const cdouble*)p.scene;
  const cdouble* geo = sc + RTX_HDR_WORDS;
  const int nsph = NSPH > 0 ? NSPH : p.nsph;
  const int nb = TREE ? huge_tail(sc, nsph) : nsph;  // the beams' tested spheres
  // the half-b sphere test (SphTest): origins the kernel generates itself, in a tame scene
  const auto tame = [&] {
    if constexpr (kSticky<Tm>) return guard;
    else return p.mode != 1 && p.mode != 3 && sc[RTX_H_TAME] != 0.0 ? 0x1.0p-350 : __builtin_nan("");
  }();

  int64_t i = 0;
  bool active;
  int kb = 0;                  // absolute level of this launch's first ray (mode 2: the resumed level)
  const double* rin = nullptr;  // mode 2: the chain's resume record
  int col = 0, lr = 0;         // mode 0: the pixel's column and local row
  // WX x WY waves per block; wave w -> WW x WH sub-tile, lane -> (l % WW, l / WW)
  // (wave_tile: (bx, by) is this wave's own WW x WH tile; TREE only, so WW = kWaveW there)
  constexpr int WW = wave_w<TREE>(), WH = 64 / WW, WX = waves_x<TREE>(), WY = fast_waves<TREE>() / WX;
  const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));  // the wave in the block
  // The pixel index (modes 0, 1, 3) from the block's tile, the wave and a lane id. The culled
  // kernels' write-out recomputes it from a fresh lane id (lane_id_fresh): kept live across the
  // bounce loop, the 64-bit index spilled in the one-tile culled kernels (C3) and cost the persistent
  // one registers (A/B r5v: C4 -1.8%); the small-scene kernels keep it (C2 +1.4% recomputed).
  auto pixel_index = [&](int lane) -> int64_t {
    if (p.mode == 0) {
      const int c = wave_tile ? bx * WW + (lane % WW) : bx * (WX * WW) + (wv % WX) * WW + (lane % WW);
      const int r = wave_tile ? by * WH + (lane / WW) : by * (WY * WH) + (wv / WX) * WH + (lane / WW);
      return (int64_t)r * p.width + c;
    }
    return (int64_t)bx * FB + wv * 64 + lane;
  };
  if (DEEP != 2 && p.mode == 0) {
    const int lane = threadIdx.x & 63, w = TREE ? wv : (int)(threadIdx.x >> 6);
    col = wave_tile ? bx * WW + (lane % WW) : bx * (WX * WW) + (w % WX) * WW + (lane % WW);
    lr = wave_tile ? by * WH + (lane / WW) : by * (WY * WH) + (w / WX) * WH + (lane / WW);
    active = col < p.width && lr < p.n_rows;
    if constexpr (!TREE) i = (int64_t)lr * p.width + col;  // (kept live: A/B r5v C2 +1.4% recomputed)
  } else if (DEEP != 2) {  // (modes 1 and 3)
    i = (int64_t)bx * FB + threadIdx.x;
    active = i < p.n;
  } else {  // continuation: entry `item` of in_list
    const int64_t item = (int64_t)bx * FB + threadIdx.x;
    active = item < (int64_t)*p.in_count;
    if (active) {
      const uint64_t e = p.in_list[item];
      i = (int64_t)(e & ((uint64_t(1) << kFrameShift) - 1));
      const int rt = (int)((e >> kRaysShift) & kLevelMask) - 1, ht = (int)((e >> kHitsShift) & kLevelMask) - 1;
      if (rt == p.in_level && ht == rt && item < p.in_rec_cap) {
        rin = p.in_rec + item * kRecWords;
        kb = rt + 1;
      } else {  // a tie, or a chain without a record: on to the general kernel unchanged
        append_deferred(p, e);
        active = false;
      }
    }
  }
  const bool cam0 = DEEP != 2 && p.mode == 0;
  // per-level counters: the stats instantiation only (the timed kernels compile none of it)
  unsigned long long* const st = STATS ? p.stats : nullptr;
  Work<STATS> wk;
  double ox = 0.0, oy = 0.0, oz = 0.0, dx = 0.0, dy = 0.0, dz = 1.0;
  // nearest hit of the current level's ray over all shapes (base.py:97-103): wave-uniform loop,
  // geometry via s_load
  double tmin = FARAWAY;
  int hit = -1;
  bool tie = false;
  // level-0 candidate spheres of the wave tile (wave_frustum) instead of the culling tree: camera
  // rays of a tame scene with a tree and at most 128 spheres
  uint64_t fm0 = 0, fm1 = 0;
  bool fr = false;
  if constexpr (TREE) {
    if (cam0 && nsph <= 128 && sc[RTX_H_NNODES] != 0.0 && sc[RTX_H_SBOX] != 0.0 && sc[RTX_H_TAME] != 0.0 &&
        sc[RTX_H_VZ] != 0.0) {
      const int lane = threadIdx.x & 63;
      fr = wave_frustum(p, __builtin_amdgcn_readfirstlane(col - lane % kWaveW),
                        __builtin_amdgcn_readfirstlane(lr - lane / kWaveW), fm0, fm1);
    }
  }
  if (active) {
    if (rin) {
      ox = rin[0]; oy = rin[1]; oz = rin[2];
      dx = rin[3]; dy = rin[4]; dz = rin[5];
    } else if (cam0) {
      if constexpr (!TREE) {
        // a whole-frame launch's tile that ends before the frame's last column and row (so it is not
        // clipped either): the straight-line camera ray. Row tiles (n_parts > 1) keep the selects.
        static_assert(WX == 1 && WY == 1, "one wave tile per block: (bx, by) is the wave's tile");
        const bool inner = p.n_parts == 1 && bx * WW + WW < p.width && by * WH + WH < p.height;
        camera_dir_small(sc, col, global_row(p, lr), p.width, p.height, inner, dx, dy, dz, tame);
        ox = sc[RTX_H_CAM + 0];
        oy = sc[RTX_H_CAM + 1];
        oz = sc[RTX_H_CAM + 2];
      } else {
        camera_ray(p, col, lr, ox, oy, oz, dx, dy, dz, tame);  // no division of the pixel index
      }
    } else {
      load_ray(p, i, ox, oy, oz, dx, dy, dz);
    }
    if (st) {
      if (!rin) stat_add(st, RTX_S_PIXELS, 1);
      if (kb < RTX_S_LEVELS) {
        stat_add(st, RTX_S_RAYS + kb, 1);
        stat_wave(st, RTX_S_WTRACE + kb);
      }
    }
    if (p.mode == 3) {  // NumpyShader.create: the hit is given (shader.py:63-73)
      tmin = p.hit_t[i];
      hit = p.hit_shape;
      // create on another shape's shader (RTX_H_MAT0): the general kernel shades this level-0 hit
      // with that material, deferred like a tie
      tie = sc[RTX_H_MAT0] != 0.0;
    } else if (TREE && sc[RTX_H_NNODES] != 0.0) {
      if (fr) {  // (the image-plane boxes' comparisons are not priced)
        nearest_masked<true>(geo, fm0, fm1, ox, oy, oz, dx, dy, dz, tmin, hit, tie, tame, wk);
      } else if (cam0) {
        nearest_bvh<true>(sc, ox, oy, oz, dx, dy, dz, tmin, hit, tie, tame, wk);
      } else {
        nearest_bvh<false>(sc, ox, oy, oz, dx, dy, dz, tmin, hit, tie, tame, wk);
      }
    } else if (cam0) {
      // (the small-scene kernels: O - C from the packer's table where the blob has it)
      const cdouble* const rel = TREE ? nullptr : camrel_table<NSPH>(sc, nsph);
      if (rel) nearest_hit_rel(geo, rel, nsph, dx, dy, dz, tmin, hit, tie, tame, wk);
      else nearest_hit<true>(geo, nsph, ox, oy, oz, dx, dy, dz, tmin, hit, tie, tame, wk);
    } else {
      nearest_hit<false>(geo, nsph, ox, oy, oz, dx, dy, dz, tmin, hit, tie, tame, wk);
    }
  }
  stage(hit);
  // (the optimistic body keeps its inactive lanes, hit < 0, to the verdict: the wave stays whole for
  // the second pass)
  if constexpr (!kSticky<Tm>) {
    if (!active) return false;
  }
  constexpr bool CL = !DEEP && LDS && TREE && !BEAM;  // colour in LDS (kColourLdsBytes)
  static_assert(!CL || 3 * sizeof(double) * FB == kColourLdsBytes, "colour LDS");
  double* const cl = CL ? const_cast<double*>(lds_tab) + nsph * kSphWords + threadIdx.x : nullptr;
  if constexpr (CL) {
    cl[0] = 0.0;
    cl[FB] = 0.0;
    cl[2 * FB] = 0.0;
  }

  // the colour accumulated level by level, thr = T_k
  double cr = 0.0, cg = 0.0, cb = 0.0;
  double thr = 1.0;
  if constexpr (DEEP == 2) {  // a continued chain: its colour so far and the next level's weight
    if (rin) {
      cr = rin[6];
      cg = rin[7];
      cb = rin[8];
      thr = rin[9];
    }
  }
  bool deferred = false, appended = false;
  int rays_through = 0, hits_through = -1;  // per-level counts already made for this pixel

  for (int k = 0;; ++k) {
    if (hit < 0) break;  // nothing hit: NumpyRGBColor(0, 0, 0) (base.py:100), a black reflection adds nothing
    if (tie) {  // several shapes shaded and summed: the general kernel takes this ray
      deferred = true;
      rays_through = kb + k;
      hits_through = kb + k - 1;
      if (st && !(p.mode == 3 && kb + k == 0)) stat_add(st, RTX_S_TIES, 1);  // (not the RTX_H_MAT0 deferral)
      break;
    }
    Hit s;
    if constexpr (LDS) {
      shade<IMG, TREE>(sc, geo, (const double*)lds_tab, nsph, hit, ox, oy, oz, dx, dy, dz, tmin, s, tame, wk);
    } else {
      shade<IMG, TREE>(sc, geo, p.scene + RTX_HDR_WORDS, nsph, hit, ox, oy, oz, dx, dy, dz, tmin, s, tame, wk);
    }
    if (s.tk < 0) {  // an image-textured sphere: so is this one (the texel lookup stays out of here)
      deferred = true;
      rays_through = kb + k;
      hits_through = kb + k - 1;
      break;
    }
    if (st && kb + k < RTX_S_LEVELS) {
      stat_add(st, RTX_S_HITS + kb + k, 1);
      stat_wave(st, RTX_S_WSHADE + kb + k);
    }
    const bool weighted = s.lit && s.g != 0.0;
    // the cap itself (absolute level; a continuation pass may run into a cap of 9 or 10)
    const bool at_cap = DEEP && p.max_bounces >= 0 && kb + k >= p.max_bounces;
    {  // (a scope of its own: lr_, lg_, lb_ and kmax end before the next level's search. The DEEP kernels'
       // register allocation follows it: without the braces their spills move by a few VGPRs either way)
      // this level's colour with a black reflection, weighted by the chain's throughput (at level 0
      // cr = 0 + 1 * L_0 = L_0 exactly: a chain of one level has the reference's association)
      const double* tab = LDS ? (const double*)lds_tab : p.scene + RTX_HDR_WORDS;
      double lr_, lg_, lb_;
      hit_color<IMG>(tab + nsph * RTX_GEOM_WORDS + hit * RTX_MAT_WORDS, sc, s.dli, s.di, s.tk, s.lit, weighted, s.spec,
                     s.va, 0.0, 0.0, 0.0, lr_, lg_, lb_, tame);
      if constexpr (CL) {
        cl[0] = __builtin_fma(thr, lr_, cl[0]);
        cl[FB] = __builtin_fma(thr, lg_, cl[FB]);
        cl[2 * FB] = __builtin_fma(thr, lb_, cl[2 * FB]);
      } else {
        cr = __builtin_fma(thr, lr_, cr);
        cg = __builtin_fma(thr, lg_, cg);
        cb = __builtin_fma(thr, lb_, cb);
      }
      // a DEEP launch goes on to its record level (the first pass: kFirstPassLevels; the continuation
      // pass: kDeepLevel3, the registers holding nothing per level), then defers the chain with a record
      const int kmax = DEEP ? p.drec_level - kb : B;
      if (DEEP && weighted && k >= kmax && !at_cap) {  // the chain goes on beyond this launch's levels
        deferred = true;
        appended = true;
        rays_through = hits_through = kb + kmax;
        const int64_t slot = append_deferred(p, deferred_entry(DEEP == 2 || !TREE ? i : pixel_index(lane_id_fresh()),
                                                               p.frame, kb + kmax, kb + kmax));
        if (p.drec && slot >= 0 && slot < p.rec_cap) {
          double* rec = p.drec + slot * kRecWords;
          double rx = dx, ry = dy, rz = dz;
          reflect_dir(rx, ry, rz, s.nx, s.ny, s.nz);
          rec[0] = s.qx; rec[1] = s.qy; rec[2] = s.qz;
          rec[3] = rx; rec[4] = ry; rec[5] = rz;
          rec[6] = cr; rec[7] = cg; rec[8] = cb;
          rec[9] = (thr * 0.5) * s.g;  // the next level's weight, as below
        }
        break;
      }
      if (!weighted || k >= kmax || at_cap) break;
      thr = (thr * 0.5) * s.g;  // the reflection's weight, (R * 0.5) * g (shader.py:106)
    }
    // the reflected ray becomes the next level (the level's colour is already in cr, cg, cb)
    reflect_dir(dx, dy, dz, s.nx, s.ny, s.nz, tame);
    ox = s.qx;
    oy = s.qy;
    oz = s.qz;
    if (st && kb + k + 1 < RTX_S_LEVELS) {
      stat_add(st, RTX_S_RAYS + kb + k + 1, 1);
      stat_wave(st, RTX_S_WTRACE + kb + k + 1);
    }
    [[maybe_unused]] uint32_t tests0 = 0, nodes0 = 0;
    if constexpr (STATS) {
      tests0 = wk.tests;
      nodes0 = wk.nodes;
    }
    if (TREE && sc[RTX_H_NNODES] != 0.0) {
      // the wave's beam candidates (tame scenes up to 128 spheres), else the culling tree
      Beam bm;
      const double* btab = LDS ? (const double*)lds_tab : p.scene + RTX_HDR_WORDS;
      if (BEAM && sc[RTX_H_TAME] != 0.0 && wave_beam<LDS>(btab, nb, ox, oy, oz, dx, dy, dz, bm)) {
        if (st) stat_wave(st, RTX_S_BEAMW);
        for (int j = 0; j < bm.passes; ++j) wk.beam();  // a lane's cone test of one sphere per pass
        nearest_beam(geo, nsph, bm, ox, oy, oz, dx, dy, dz, tmin, hit, tie, tame, wk);
      } else {
        nearest_bvh<false>(sc, ox, oy, oz, dx, dy, dz, tmin, hit, tie, tame, wk);
      }
    } else {
      nearest_hit<false>(geo, nsph, ox, oy, oz, dx, dy, dz, tmin, hit, tie, tame, wk);
    }
    if constexpr (STATS) {
      wk.tests1 += wk.tests - tests0;
      wk.nodes1 += wk.nodes - nodes0;
    }
  }

  if constexpr (STATS) {
    if (st) {
      stat_add(st, RTX_S_TESTS, wk.tests);
      stat_add(st, RTX_S_NODES, wk.nodes);
      stat_add(st, RTX_S_TESTS1, wk.tests1);
      stat_add(st, RTX_S_NODES1, wk.nodes1);
      stat_add(st, RTX_S_BOXES, wk.boxes);
      stat_add(st, RTX_S_BEAMT, wk.beamt);
    }
  }
  if constexpr (kSticky<Tm>) {
    // one verdict per wave: a lane outside some fast core's exact range sends the whole wave to the
    // guarded body (nothing was written, and a tie is appended only below)
    if (__ballot(guard.bad) != 0) return true;
    if (!active) return false;
  }
  const int64_t io = DEEP == 2 || !TREE ? i : pixel_index(lane_id_fresh());
  if constexpr (CL) {
    cr = cl[0];
    cg = cl[FB];
    cb = cl[2 * FB];
  }
  if (deferred) {
    // a tie (deep deferrals were appended with their resume record)
    if (!appended) append_deferred(p, deferred_entry(io, p.frame, rays_through, hits_through));
    if (st && !rin) stat_add(st, RTX_S_DEFERRED, 1);
    return false;
  }
  write_out(p, io, cr, cg, cb);
  return false;
}

// the culled kernels' tile (and the small-scene continuation pass's): guarded, the block's LDS table
// staged by k_render_fast and complete at the barrier after the first tile's level-0 search
template <int B, bool LDS, int DEEP, bool STATS, bool TREE, bool BEAM, bool IMG = false, int NSPH = 0>
__device__ __forceinline__ void fast_tile(const Params& p, int bx, int by, bool first, const double* lds_tab,
                                          bool wave_tile = false) {
  fast_tile_body<B, LDS, DEEP, STATS, TREE, BEAM, IMG, NSPH>(p, bx, by, lds_tab, wave_tile, 0.0, [&](int) {
    if constexpr (LDS) {
      if (first) __syncthreads();
    }
  });
}

// TP: 0 = no culling tree and no persistent launch (scenes below kTreeMinSpheres), 1 = culling tree,
// one tile per block (the launch is not persistent), 2 = both (persistent launches)
// DEEP: 0 capped (the chain ends at level B), 1 the first pass of an uncapped render (chains alive at
// its record level are deferred with a resume record), 2 a continuation pass (mode 2: chains resumed
// from their records; its own instantiation, so that the first pass compiles no resume code)
template <int B, bool LDS, int DEEP, bool STATS, int TP, bool IMG, int NSPH>
__device__ __forceinline__ void k_render_fast_tiles(const Params& p, const double* lds_tab);
template <int B, int DEEP, bool STATS, bool IMG, int NSPH>
__device__ __forceinline__ void small_wave(const Params& p, double* lds_tab);

// WAVES > 0: that many waves/SIMD instead of the rule below (kFwdWavesLarge)
template <int B, bool LDS, int DEEP, bool STATS = false, int TP = 2, bool IMG = false, int NSPH = 0, int WAVES = 0>
__global__ __launch_bounds__(fast_block<(TP >= 1)>(),
                             WAVES > 0 ? WAVES
                             : DEEP    ? (TP >= 2 || DEEP == 2 ? kDeepWaves : kDeepWavesTile)
                                       : (TP >= 2 ? kFwdWavesPersist : TP ? kFwdWaves : kFwdWavesSmall)) void
k_render_fast(Params p0) {
  constexpr bool TREE = TP >= 1;
  // reflected-ray beams (wave_beam): the persistent launches, scenes of kPersistMinSpheres and more
  // (A/B: C4 -5.3%; with 16 spheres the tree walk is cheaper than the beam, C3 +7%, C5 +4%), capped
  // or not (the DEEP first pass since round 6, with kDeepWaves 4: A/B r6ap, unbounded C4 2,101 ->
  // 1,800 us)
  constexpr bool BEAM = TP >= 2;
  extern __shared__ double lds_tab[];
  const Params p = frame_view(p0, blockIdx.z);  // frame of a multi-frame launch (grid z)
  if constexpr (TP == 0 && DEEP != 2) {  // one-wave blocks with a start-up of their own
    static_assert(LDS, "the small-scene kernels stage the table in LDS");
    small_wave<B, DEEP, STATS, IMG, NSPH>(p, lds_tab);
    return;
  }
  {
    // a blob that is not a packed scene of p.nsph spheres (the LDS table and every sphere loop are
    // sized by p.nsph): render nothing and flag it (block-uniform, so the persistent launch's
    // fetch counters stay untouched)
    const cdouble* sc = (const cdouble*)p.scene;
    if (sc[RTX_H_MAGIC] != RTX_MAGIC || sc[RTX_H_NSPH] != (double)p.nsph || (NSPH > 0 && p.nsph != NSPH)) {
      if (threadIdx.x == 0) atomicOr((uint32_t*)p.ws + RTX_WS_STATUS, (uint32_t)RTX_ST_BAD_SCENE);
      return;
    }
  }
  if constexpr (LDS) {  // per-lane view of the sphere table: one LDS copy per block (the culled kernels
                        // and the continuation pass; the barrier is fast_tile's, after the first tile's
                        // level-0 nearest-hit test. small_wave above stages its own)
    const double* src = p.scene + RTX_HDR_WORDS;
    for (int k = threadIdx.x; k < p.nsph * kSphWords; k += fast_block<TREE>()) {
      // (the beam kernels: geometry word RTX_G_IDX of the copy holds beam_word, see wave_beam)
      const bool bw = BEAM && k < p.nsph * RTX_GEOM_WORDS && (k & (RTX_GEOM_WORDS - 1)) == RTX_G_IDX;
      lds_tab[k] = bw ? beam_word(src[k - RTX_G_IDX + RTX_G_CC], src[k - RTX_G_IDX + RTX_G_RR]) : src[k];
    }
  }
  if constexpr (DEEP == 2) {  // continuation pass (mode 2): 256 entries of in_list per tile, grid-stride
    const int64_t count = (int64_t)*p.in_count;
    for (int64_t t = blockIdx.x; t * fast_block<TREE>() < count; t += gridDim.x) {
      fast_tile<B, LDS, DEEP, STATS, TREE, BEAM, IMG, NSPH>(p, (int)t, 0, t == (int64_t)blockIdx.x, lds_tab);
    }
  } else {
    k_render_fast_tiles<B, LDS, DEEP, STATS, TP, IMG, NSPH>(p, lds_tab);
  }
}

// the camera / explicit-ray launches of k_render_fast (every instantiation but the continuation's)
template <int B, bool LDS, int DEEP, bool STATS, int TP, bool IMG, int NSPH>
__device__ __forceinline__ void k_render_fast_tiles(const Params& p, const double* lds_tab) {
  constexpr bool TREE = TP >= 1;
  constexpr bool BEAM = TP >= 2;
  if (TP >= 2 && p.n_fetch > 0) {  // (persistent launches are for scenes of kPersistMinSpheres and more)
    // Persistent waves fetching kWaveW x kWaveH tiles, bottom-up (longest work first, as below).
    // Counter c (of n_fetch) hands out tiles c, c + n_fetch, ... . Waves are numbered XCD-major
    // (pw; block b runs on XCD b % 8) and wave pw uses counter pw % n_fetch, so every counter's
    // waves are spread over all XCDs. Wave pw renders tile pw first (static, no fetch); the next
    // tile's atomic is always issued before the current tile renders, hiding its latency. Each
    // wave makes exactly one out-of-range fetch, so the wave receiving a counter's last value is
    // its last user and resets it to 0 for the next launch (no per-launch memset).
    if constexpr (LDS) __syncthreads();  // the table staged above
    const int lane = threadIdx.x & 63;
    const int nc = p.n_fetch;
    const int nx = (gridDim.x % 8 == 0) ? 8 : 1;
    const int pw = ((int)(blockIdx.x % nx) * (int)(gridDim.x / nx) + (int)(blockIdx.x / nx)) * kFastWaves +
                   (threadIdx.x >> 6);
    const int waves_c = (int)(gridDim.x * kFastWaves) / nc;  // the host makes nc divide the waves per XCD
    const int c = pw % nc;
    const int nt = p.n_tiles_x * p.n_tiles_y;
    const int tiles_c = (nt - c + nc - 1) / nc;
    uint32_t* const ctr = p.fetch + c * kFetchStride;
    uint32_t nxt = 0;
    if (lane == 0) nxt = atomicAdd(ctr, 1u);
    int k = pw / nc;
    int v = 0;
    // the host's dispatch order (longest tiles first, learnt from an earlier launch's tile_cost), read
    // through the scalar cache: the index is wave-uniform
    const uint32_t __attribute__((address_space(4)))* const order =
        (const uint32_t __attribute__((address_space(4)))*)p.tile_order;
    while (k < tiles_c) {
      const int t = order ? (int)order[c + k * nc] : c + k * nc;
      // (an order entry outside the launch's tiles — a stale or foreign order buffer — renders nothing
      // rather than writing outside the frame)
      if ((unsigned)t < (unsigned)nt) {
        const int row = t / p.n_tiles_x;
        // the tile's time as -start + end in its cost word. Cost records are kept to the STATS
        // instantiations (run_render picks one for a launch that records them): in the timed kernel
        // the record costs C4 six more spilled VGPRs and 2.5% (A/B r4h)
        if (STATS && p.tile_cost && lane == 0) p.tile_cost[t] = 0u - (uint32_t)__builtin_amdgcn_s_memrealtime();
        fast_tile<B, LDS, DEEP, STATS, TREE, BEAM, IMG, NSPH>(p, t - row * p.n_tiles_x, p.n_tiles_y - 1 - row, false,
                                                              lds_tab, true);
        if (STATS && p.tile_cost && lane == 0) atomicAdd(p.tile_cost + t, (uint32_t)__builtin_amdgcn_s_memrealtime());
      }
      v = __builtin_amdgcn_readfirstlane(nxt);
      k = waves_c + v;
      if (k < tiles_c && lane == 0) nxt = atomicAdd(ctr, 1u);
    }
    if (k == pw / nc) v = __builtin_amdgcn_readfirstlane(nxt);  // no tile rendered: the first fetch
    const int dyn = tiles_c > waves_c ? tiles_c - waves_c : 0;  // in-range fetches on this counter
    if (lane == 0 && v == dyn + waves_c - 1) atomicExch(ctr, 0u);
    return;
  }
  // one tile per block. Bottom tile rows are dispatched first: they hold the ground and the
  // spheres, whose pixels run long bounce chains, while sky rows finish at level 0 and so fill the
  // end of the grid (longest-first order; A/B: C2 -10%, C5 -8%, C4 -2%). Output does not depend on
  // the order. Blocks are dispatched in blockIdx order: a host order (camera launches,
  // rtx_render_camera_sched) maps dispatch slot b to block tile order[b], block tile t being
  // (t % gridDim.x, bottom-up row t / gridDim.x), and a cost record takes each block's time.
  const uint64_t t_entry = STATS && p.tile_cost ? __builtin_amdgcn_s_memrealtime() : 0;  // (learning the order)
  int bx = blockIdx.x, by = gridDim.y - 1 - blockIdx.y, tb = blockIdx.y * gridDim.x + blockIdx.x;
  if (p.tile_order) {
    tb = (int)((const uint32_t __attribute__((address_space(4)))*)p.tile_order)[tb];
    if ((unsigned)tb >= gridDim.x * gridDim.y) return;  // (block-uniform: a stale order renders nothing)
    bx = tb % gridDim.x;
    by = gridDim.y - 1 - tb / gridDim.x;
  }
  fast_tile<B, LDS, DEEP, STATS, TREE, BEAM, IMG, NSPH>(p, bx, by, true, lds_tab);
  if (STATS && p.tile_cost && (threadIdx.x & 63) == 0)  // the block's time: the slowest of its waves
    atomicMax(p.tile_cost + tb, (uint32_t)(__builtin_amdgcn_s_memrealtime() - t_entry));
}

// One wave of a small-scene kernel (TP 0: scenes below kTreeMinSpheres, one wave per block, one
// 16 x 4 tile or 64 explicit rays per wave; the continuation pass keeps k_render_fast's order).
//
// Start-up. A wave lives ~17 k cycles and a third of them render sky only, so the dependent memory
// round trips before its first f64 instruction count. After the kernarg, everything the prologue
// needs is requested in one round: the header's magic and sphere count, the tile-order entry, and
// the wave's share of the sphere table, which stays in registers (at most kSmallStage words a lane)
// while the level-0 search runs on the scalar cache. The magic check is consumed after those
// requests (the table read is sized by the caller's p.nsph, as the sphere loops are; it only reads).
// The table is written to LDS after the level-0 search, and only if some lane hit something: an
// all-sky wave writes its zeros and ends without waiting for the table.
//
// Guards. The counter-free, texture-free capped builds (OPT) render a camera tile of a tame scene
// through the optimistic body first (Sticky: no ballot or branch per helper) and fall back to the
// guarded body, today's code, when the wave's verdict says some lane left a fast core's exact range;
// untamed scenes and explicit-ray launches go straight to the guarded body. The fast cores return
// their guarded expansions' bits on in-range operands and no lane's value depends on another lane,
// so the frame is the same either way. The STATS builds have the guarded body only: their counters
// count a tile once.
constexpr int kSmallStage = ((kTreeMinSpheres - 1) * kSphWords + 63) / 64;
template <int B, int DEEP, bool STATS, bool IMG, int NSPH>
__device__ __forceinline__ void small_wave(const Params& p, double* lds_tab) {
  static_assert(kFastWavesSmall == 1 && fast_block<false>() == 64, "small_wave: one wave per block");
  static_assert(DEEP != 2, "the continuation pass is k_render_fast's");
  const uint64_t t_entry = STATS && p.tile_cost ? __builtin_amdgcn_s_memrealtime() : 0;  // (learning the order)
  const cdouble* sc = (const cdouble*)p.scene;
  const double magic = sc[RTX_H_MAGIC], hn = sc[RTX_H_NSPH];
  // the wave's share of the table: words lane, lane + 64, ...
  constexpr int NL = NSPH > 0 ? (NSPH * kSphWords + 63) / 64 : kSmallStage;
  const double* src = p.scene + RTX_HDR_WORDS;
  const int nw0 = p.nsph * kSphWords;
  const int lane = threadIdx.x;
  double tv[NL];
#pragma unroll
  for (int j = 0; j < NL; ++j) tv[j] = lane + 64 * j < nw0 ? src[lane + 64 * j] : 0.0;
  // One tile per block. Bottom tile rows are dispatched first: they hold the ground and the
  // spheres, whose pixels run long bounce chains, while sky rows finish at level 0 and so fill the
  // end of the grid (longest-first order; A/B: C2 -10%). Output does not depend on the order. Blocks
  // are dispatched in blockIdx order: a host order (camera launches, rtx_render_camera_sched) maps
  // dispatch slot b to block tile order[b], block tile t being (t % gridDim.x, bottom-up row
  // t / gridDim.x), and a cost record takes each block's time.
  uint32_t tb = blockIdx.y * gridDim.x + blockIdx.x;
  {  // (the kernarg fields the tile needs further down, in the batch of the ones needed here)
    const uint32_t gy = gridDim.y;
    asm volatile("" ::"s"(p.tile_div), "s"(gy), "s"(p.n), "s"(p.part_run), "s"(p.out), "s"(p.no_general));
  }
  if (p.tile_order) tb = ((const uint32_t __attribute__((address_space(4)))*)p.tile_order)[tb];
  // ... and the header words of the camera ray (camera_dir reads the same addresses: these loads serve
  // it) and of the guard choice. The empty statement takes all of them as scalar operands, so they are
  // requested together and waited for once, here, with the table loads in flight. (The linspace stop
  // words are left to camera_dir, whose last column and row alone read them: with them here the
  // NSPH 3, B 3 build spills.)
  {
    const double htame = sc[RTX_H_TAME], c0 = sc[RTX_H_CAM + 0], c1 = sc[RTX_H_CAM + 1], c2 = sc[RTX_H_CAM + 2];
    const double x0 = sc[RTX_H_XSTART], x1 = sc[RTX_H_XSTEP], y0 = sc[RTX_H_YSTART], y1 = sc[RTX_H_YSTEP];
    const double xf = sc[RTX_H_XFIX], yf = sc[RTX_H_YFIX];
    const double vz = sc[RTX_H_VZ], vz2 = sc[RTX_H_VZ2];
    if constexpr (NSPH >= 1 && NSPH <= 3) {  // (... and the word that says whether the table is there)
      const double crel = sc[RTX_H_CAMREL];
      asm volatile("" ::"s"(magic), "s"(hn), "s"(htame), "s"(tb), "s"(c0), "s"(c1), "s"(c2), "s"(x0), "s"(x1), "s"(y0),
                   "s"(y1), "s"(xf), "s"(yf), "s"(vz), "s"(vz2), "s"(crel));
    } else {  // (more spheres, or a run-time count: with the camera words held from here these builds spill)
      asm volatile("" ::"s"(magic), "s"(hn), "s"(htame), "s"(tb));
    }
  }
  // a blob that is not a packed scene of p.nsph spheres: render nothing and flag it
  if (magic != RTX_MAGIC || hn != (double)p.nsph || (NSPH > 0 && p.nsph != NSPH)) {
    if (threadIdx.x == 0) atomicOr((uint32_t*)p.ws + RTX_WS_STATUS, (uint32_t)RTX_ST_BAD_SCENE);
    return;
  }
  const int nw = NSPH > 0 ? NSPH * kSphWords : nw0;  // (the check above: p.nsph == NSPH)
  int bx = blockIdx.x, by = gridDim.y - 1 - blockIdx.y;
  if (p.tile_order) {
    if (tb >= gridDim.x * gridDim.y) return;  // (block-uniform: a stale order renders nothing)
    // tb / gridDim.x without a division: q' = hi32(tb * floor(2^32 / g)) is the quotient or one
    // below it (tb / g - tb * floor(2^32 / g) / 2^32 < tb / 2^32 < 1), so one correction settles it
    uint32_t q = __umulhi(tb, p.tile_div), r = tb - q * gridDim.x;
    if (r >= gridDim.x) {
      r -= gridDim.x;
      ++q;
    }
    bx = (int)r;
    by = (int)(gridDim.y - 1 - q);
  }
  bool staged = false;  // wave-uniform: the LDS table is complete
  auto stage_regs = [&](int hit) {
    if (nw > 64 * NL) {  // (a run-time count beyond the small scenes': straight from memory)
      for (int k = lane; k < nw; k += 64) lds_tab[k] = src[k];
      __syncthreads();
      staged = true;
    } else if (__ballot(hit >= 0) != 0) {
#pragma unroll
      for (int j = 0; j < NL; ++j)
        if (lane + 64 * j < nw) lds_tab[lane + 64 * j] = tv[j];
      __syncthreads();  // (one wave: the lanes' writes before any lane's read)
      staged = true;
    }
  };
  // (NSPH > 0: every scene below kTreeMinSpheres has a build of its own count, go_ns; the run-time-count
  // build serves none of them and would spill with two bodies)
  constexpr bool OPT = DEEP == 0 && !STATS && !IMG && NSPH > 0;
  bool redo = true;
  if constexpr (OPT) {
    if (p.mode == 0 && sc[RTX_H_TAME] != 0.0) {
      bool bad = false;
      redo = fast_tile_body<B, true, DEEP, STATS, false, false, IMG, NSPH>(p, bx, by, lds_tab, false, Sticky{bad},
                                                                          stage_regs);
    }
  }
  if (redo) {
    if constexpr (OPT) {  // the cold body: the table again from memory unless the first pass staged it
      // (through a scene pointer the compiler cannot connect with the first body's: no header word
      // stays in a register across the optimistic body for the sake of this one)
      Params q = p;
      asm volatile("" : "+s"(q.scene));
      fast_tile_body<B, true, DEEP, STATS, false, false, IMG, NSPH>(q, bx, by, lds_tab, false, 0.0, [&](int hit) {
        if (!staged && __ballot(hit >= 0) != 0) {
          for (int k = lane; k < nw; k += 64) lds_tab[k] = src[k];
          __syncthreads();
        }
      });
    } else {
      fast_tile_body<B, true, DEEP, STATS, false, false, IMG, NSPH>(p, bx, by, lds_tab, false, 0.0, stage_regs);
    }
  }
  if (STATS && p.tile_cost && (threadIdx.x & 63) == 0)  // the block's time
    atomicMax(p.tile_cost + tb, (uint32_t)(__builtin_amdgcn_s_memrealtime() - t_entry));
}

}  // namespace
