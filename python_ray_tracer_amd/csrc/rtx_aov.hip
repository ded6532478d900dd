// rtx_aov.hip — the primary-hit render passes (rtx_primary_aovs, rtx_primary_aovs_rays): depth,
// object id, hit count, hit position, surface normal, diffuse albedo and shadow mask of the level-0
// ray of every pixel (or of every explicit ray). Each value is an intermediate of the reference's own
// arithmetic (base.py:97-103, shader.py:73-84, Texture.get_color) that the render kernels compute
// and discard; here they are written out, by one kernel of its own beside the render kernels, in a
// translation unit of its own over the shared device text (rtx_device.h), so the render kernels
// compile from untouched text with untouched flags.
#include "rtx_device.h"
#include "rtx_internal.h"

namespace {

// Output planes of a launch; a null pointer is a pass that was not requested (wave-uniform: kernel
// arguments), which then costs no store, and no shadow ray (lit) or texel lookup (albedo) either.
struct AovOut {
  double* depth;         // [n]
  int* id;               // [n]
  int* hits;             // [n]
  double* position;      // [3][n]
  double* normal;        // [3][n]
  double* albedo;        // [3][n]
  unsigned char* lit;    // [n]
  int lit_words;         // lit is 4-byte aligned: whole waves store it as dwords
};

// One lane per ray, ray i = blockIdx.x * kBlock + threadIdx.x: the 64 lanes of a wave hold 64
// consecutive rays, so every store instruction of a wave writes one contiguous run (512 B of a
// double plane, 256 B of an int plane), and its camera rays are 64 neighbours of a pixel row
// (coherent enough for the wave-uniform walk of the culling tree). Sphere geometry is read
// wave-uniformly through the scalar cache; the hit sphere's own records per lane from the blob.
__global__ __launch_bounds__(kBlock) void k_primary_aovs(Params p, AovOut o) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  const bool live = i < p.n;
  const cdouble* sc = (const cdouble*)p.scene;
  // a blob that is not a packed scene of p.nsph spheres is traced as an empty scene: every ray misses
  const int nsph = (sc[RTX_H_MAGIC] == RTX_MAGIC && sc[RTX_H_NSPH] == (double)p.nsph) ? p.nsph : 0;
  const double* tab = p.scene + RTX_HDR_WORDS;
  const double nan = __builtin_nan("");  // the reference expressions in every sphere test (SphTest)
  bool lit = false;
  if (live) {
    double ox, oy, oz, dx, dy, dz;
    load_ray(p, i, ox, oy, oz, dx, dy, dz);
    const double oo = dot3(ox, oy, oz, ox, oy, oz);
    // base.py:97-103: the nearest distance, how many shapes share it, the first of them in scene order
    double tmin = FARAWAY;
    int nh = 0, first = nsph;
    // (without a culling tree, fewer than kTreeMinSpheres spheres: the table in scene order)
    nearest_count(sc, nsph, nsph > 0 && sc[RTX_H_NNODES] != 0.0, ox, oy, oz, oo, dx, dy, dz, tmin, nh, first);
    const bool hit = nh > 0 && tmin != FARAWAY;  // (nearest != FARAWAY) & (distance == nearest), base.py:102-103
    if (o.depth) __builtin_nontemporal_store(tmin, o.depth + i);
    if (o.id) __builtin_nontemporal_store(hit ? first : -1, o.id + i);
    if (o.hits) __builtin_nontemporal_store(hit ? nh : 0, o.hits + i);

    double px = 0.0, py = 0.0, pz = 0.0, nx = 0.0, ny = 0.0, nz = 0.0, ar = 0.0, ag = 0.0, ab = 0.0;
    if (hit && (o.position || o.normal || o.albedo || o.lit)) {
      const int h = first;
      const double* gh = tab + h * RTX_GEOM_WORDS;
      const double* mh = tab + nsph * RTX_GEOM_WORDS + h * RTX_MAT_WORDS;
      px = ox + dx * tmin, py = oy + dy * tmin, pz = oz + dz * tmin;  // shader.py:73
      const double inv_r = gh[RTX_G_INVR];
      nx = (px - gh[RTX_G_CX]) * inv_r;  // shader.py:74
      ny = (py - gh[RTX_G_CY]) * inv_r;
      nz = (pz - gh[RTX_G_CZ]) * inv_r;
      if (o.albedo) {  // diffuse_color.get_color(P)
        const double tex = mh[RTX_M_TEX];
        if (tex == RTX_TEX_CHECKER) {  // shader.py:30-32
          ar = ag = ab = trunc_parity(px * 2.0) == trunc_parity(pz * 2.0) ? 1.0 : 0.0;
        } else if (tex == RTX_TEX_IMAGE) {  // shape.py:66-79
          const double* t = p.scene + ((int64_t)mh[RTX_M_TR] + 3 * (int64_t)image_texel(mh, gh, px, py, pz));
          ar = t[0], ag = t[1], ab = t[2];
        } else {  // shader.py:17-19
          ar = mh[RTX_M_TR], ag = mh[RTX_M_TG], ab = mh[RTX_M_TB];
        }
      }
      if (o.lit) {
        // shader.py:75-84, 126-128: lit == (light_distances[id] == min(light_distances)), in its
        // any-hit form as in shade(): lit unless some sphere is strictly nearer than the shape
        // itself along L from the nudged point. The shape's own test is t_self itself, so the loops
        // skip it when every lane of the wave hit the same shape (hs).
        double lx = sc[RTX_H_LIGHT + 0] - px, ly = sc[RTX_H_LIGHT + 1] - py, lz = sc[RTX_H_LIGHT + 2] - pz;
        norm3(lx, ly, lz);  // :75
        const double qx = px + nx * 0.0001, qy = py + ny * 0.0001, qz = pz + nz * 0.0001;  // :77
        const double qq = dot3(qx, qy, qz, qx, qy, qz);
        const int h0 = __builtin_amdgcn_readfirstlane(h);
        const int hs = __ballot(h != h0) == 0 ? h0 : nsph;
        const double tself = isect_t(gh, qx, qy, qz, qq, lx, ly, lz, nan);
        lit = nothing_nearer(sc, nsph, qx, qy, qz, qq, lx, ly, lz, tself, hs);
      }
    }
    const int64_t n = p.n;
    if (o.position) {
      __builtin_nontemporal_store(px, o.position + i);
      __builtin_nontemporal_store(py, o.position + n + i);
      __builtin_nontemporal_store(pz, o.position + 2 * n + i);
    }
    if (o.normal) {
      __builtin_nontemporal_store(nx, o.normal + i);
      __builtin_nontemporal_store(ny, o.normal + n + i);
      __builtin_nontemporal_store(nz, o.normal + 2 * n + i);
    }
    if (o.albedo) {
      __builtin_nontemporal_store(ar, o.albedo + i);
      __builtin_nontemporal_store(ag, o.albedo + n + i);
      __builtin_nontemporal_store(ab, o.albedo + 2 * n + i);
    }
  }
  if (o.lit) {
    // one byte per ray: a whole wave (64 consecutive rays from a multiple of 64) stores its 64 bytes
    // as 16 dwords built from one ballot instead of 64 byte stores; a wave that crosses the end of
    // the batch, or an unaligned plane, stores bytes
    const int lane = (int)(threadIdx.x & 63u);
    const int64_t base = i - lane;
    const uint64_t m = __ballot(live && lit);
    if (o.lit_words && base + 64 <= p.n) {
      if (lane < 16) {
        const uint32_t b = (uint32_t)(m >> (4 * lane)) & 0xFu;
        const uint32_t w = (b & 1u) | ((b & 2u) << 7) | ((b & 4u) << 14) | ((b & 8u) << 21);
        __builtin_nontemporal_store(w, (uint32_t*)(o.lit + base) + lane);
      }
    } else if (live) {
      __builtin_nontemporal_store((unsigned char)(lit ? 1 : 0), o.lit + i);
    }
  }
}

int launch_aovs(const Params& p, double* depth, int32_t* id, int32_t* hits, double* position, double* normal,
                double* albedo, uint8_t* lit, void* stream) {
  AovOut o{depth, (int*)id, (int*)hits, position, normal, albedo, lit, (uintptr_t)lit % 4 == 0 ? 1 : 0};
  hipLaunchKernelGGL(k_primary_aovs, dim3((unsigned)((p.n + kBlock - 1) / kBlock)), dim3(kBlock), 0,
                     (hipStream_t)stream, p, o);
  return rtx_launched("k_primary_aovs");
}

}  // namespace

extern "C" {

int rtx_primary_aovs(const double* scene, int n_spheres, int width, int height, int row_block, int n_parts, int part,
                     int part_run, int n_local_rows, double* depth, int32_t* id, int32_t* hits, double* position,
                     double* normal, double* albedo, uint8_t* lit, void* stream) {
  if (!scene) return rtx_fail(RTX_E_ARG, "null scene pointer");
  if (!depth && !id && !hits && !position && !normal && !albedo && !lit)
    return rtx_fail(RTX_E_ARG, "no pass requested: every output pointer is null");
  if (n_spheres < 1 || n_spheres > RTX_MAX_SPHERES) return rtx_fail(RTX_E_ARG, "n_spheres out of range");
  if (!tile_geometry_ok(width, height, row_block, n_parts, part, part_run, n_local_rows))
    return rtx_fail(RTX_E_ARG, "bad frame/tile geometry");
  Params p{};
  camera_params(p, scene, n_spheres, width, height, row_block, n_parts, part, part_run, n_local_rows);
  if (p.n == 0) return RTX_OK;
  return launch_aovs(p, depth, id, hits, position, normal, albedo, lit, stream);
}

int rtx_primary_aovs_rays(const double* scene, int n_spheres, const double* origins, int64_t origin_stride,
                          const double* dirs, int64_t n, double* depth, int32_t* id, int32_t* hits, double* position,
                          double* normal, double* albedo, uint8_t* lit, void* stream) {
  if (!scene) return rtx_fail(RTX_E_ARG, "null scene pointer");
  if (!origins || !dirs) return rtx_fail(RTX_E_ARG, "null ray pointer");
  if (!depth && !id && !hits && !position && !normal && !albedo && !lit)
    return rtx_fail(RTX_E_ARG, "no pass requested: every output pointer is null");
  if (n_spheres < 1 || n_spheres > RTX_MAX_SPHERES) return rtx_fail(RTX_E_ARG, "n_spheres out of range");
  if (n < 0) return rtx_fail(RTX_E_ARG, "negative ray count");
  if (origin_stride != 0 && origin_stride != n) return rtx_fail(RTX_E_ARG, "origin_stride must be 0 or n");
  if (n == 0) return RTX_OK;
  Params p{};
  ray_params(p, scene, n_spheres, 1, origins, origin_stride, dirs, n);
  return launch_aovs(p, depth, id, hits, position, normal, albedo, lit, stream);
}

}  // extern "C"
