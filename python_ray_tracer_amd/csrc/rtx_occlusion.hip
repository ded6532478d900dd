// rtx_occlusion.hip — the occlusion passes (rtx_occlusion): ambient occlusion and soft shadows of
// the primary hit of every ray, a bundle of side x side any-hit rays from each hit, computed from the
// id, position and normal passes rtx_primary_aovs* wrote. Every decision is one of the reference's
// own sphere tests (shape.py:28-51) in the reference expressions, and each result is a count of
// samples; the contract is in include/rtx_hip.h. A translation unit of its own over the shared device
// text (rtx_device.h), like rtx_aov.hip: the render kernels compile from untouched text with
// untouched flags.
#include "rtx_device.h"
#include "rtx_internal.h"

namespace {

struct OccParams {
  const double* scene;
  int nsph;
  const int* id;           // [n]
  const double* position;  // [3][n]
  const double* normal;    // [3][n]
  int64_t n;
  const double* table;     // [3][side*side]: the hemisphere table (rows 0, 1: the unit disk)
  int side;
  const double* rot;       // [2][64]: the per-hit rotations (cos, sin)
  double max_distance;
  double light_radius;
  float* ao;               // [n] or null
  float* soft;             // [n] or null
};

__device__ __forceinline__ uint64_t rotl64(uint64_t x, int k) { return (x << k) | (x >> (64 - k)); }

// The per-hit rotation index: a hash of the bit patterns of the hit point alone (no pixel index), so
// a row tile, an explicit ray and the whole frame rotate a hit's samples alike.
__device__ __forceinline__ int rotation_index(double px, double py, double pz) {
  const uint64_t w = (uint64_t)__double_as_longlong(px) ^ rotl64((uint64_t)__double_as_longlong(py), 21) ^
                     rotl64((uint64_t)__double_as_longlong(pz), 42);
  uint32_t x = (uint32_t)(w ^ (w >> 32));
  x ^= x >> 16;
  x *= 0x7feb352du;
  x ^= x >> 15;
  x *= 0x846ca68bu;
  x ^= x >> 16;
  return (int)(x & 63u);
}

// The branch-free orthonormal frame around a unit vector n (Duff et al.): |s + n.z| >= 1, so no
// direction is singular.
struct Frame {
  double tx, ty, tz, bx, by, bz;
};
__device__ __forceinline__ Frame frame_around(double nx, double ny, double nz) {
  const double s = __builtin_copysign(1.0, nz);
  const double a = div_cr(-1.0, s + nz);
  const double b = (nx * ny) * a;
  Frame f;
  f.tx = 1.0 + ((s * nx) * nx) * a;
  f.ty = s * b;
  f.tz = (-s) * nx;
  f.bx = b;
  f.by = s + (ny * ny) * a;
  f.bz = -ny;
  return f;
}

// One lane per ray, ray i = blockIdx.x * kBlock + threadIdx.x: the 64 lanes of a wave hold 64
// consecutive rays, so its id / position / normal loads and its float stores are contiguous runs.
// The sample loop is wave-uniform (the table row through the scalar cache); only the rotation is a
// per-lane gather, once before the loops. The frame, the normal and the nudged point stay in
// registers across a loop. No LDS, no atomics.
__global__ __launch_bounds__(kBlock) void k_occlusion(OccParams p) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  const bool live = i < p.n;
  const cdouble* sc = (const cdouble*)p.scene;
  // a blob that is not a packed scene of p.nsph spheres: every ray a miss
  const int nsph = (sc[RTX_H_MAGIC] == RTX_MAGIC && sc[RTX_H_NSPH] == (double)p.nsph) ? p.nsph : 0;
  const int h = live ? p.id[i] : -1;
  const bool hit = h >= 0 && h < nsph;
  float ao = 1.0f, soft = 0.0f;
  if (__ballot(hit) != 0) {  // (a wave without a hit writes the miss values and ends)
    if (hit) {
      const int64_t n = p.n;
      const double px = p.position[i], py = p.position[n + i], pz = p.position[2 * n + i];
      const double nx = p.normal[i], ny = p.normal[n + i], nz = p.normal[2 * n + i];
      const double qx = px + nx * 0.0001, qy = py + ny * 0.0001, qz = pz + nz * 0.0001;  // shader.py:77
      const double qq = dot3(qx, qy, qz, qx, qy, qz);
      const int r = rotation_index(px, py, pz);
      const double cr = p.rot[r], sr = p.rot[64 + r];
      const int ns = p.side * p.side;
      const cdouble* tb = (const cdouble*)p.table;
      if (p.ao) {
        const Frame f = frame_around(nx, ny, nz);
        int occluded = 0;
        for (int j = 0; j < ns; ++j) {
          const int ju = __builtin_amdgcn_readfirstlane(j);
          const double x = tb[ju], y = tb[ns + ju], z = tb[2 * ns + ju];
          const double xr = x * cr - y * sr, yr = x * sr + y * cr;
          double dx = (f.tx * xr + f.bx * yr) + nx * z;
          double dy = (f.ty * xr + f.by * yr) + ny * z;
          double dz = (f.tz * xr + f.bz * yr) + nz * z;
          norm3(dx, dy, dz);
          if (!nothing_nearer(sc, nsph, qx, qy, qz, qq, dx, dy, dz, p.max_distance, nsph)) ++occluded;
        }
        ao = (float)div_cr((double)(ns - occluded), (double)ns);
      }
      if (p.soft) {
        const double Lx = sc[RTX_H_LIGHT + 0], Ly = sc[RTX_H_LIGHT + 1], Lz = sc[RTX_H_LIGHT + 2];
        double wx = Lx - px, wy = Ly - py, wz = Lz - pz;
        norm3(wx, wy, wz);
        const Frame f = frame_around(wx, wy, wz);
        const double* gh = p.scene + RTX_HDR_WORDS + h * RTX_GEOM_WORDS;
        const int h0 = __builtin_amdgcn_readfirstlane(h);
        const int hs = __ballot(h != h0) == 0 ? h0 : nsph;
        const double nan = __builtin_nan("");
        int lit = 0;
        for (int j = 0; j < ns; ++j) {
          const int ju = __builtin_amdgcn_readfirstlane(j);
          const double a = tb[ju], b = tb[ns + ju];
          const double ar = a * cr - b * sr, br = a * sr + b * cr;
          double lx = (Lx + (f.tx * ar + f.bx * br) * p.light_radius) - px;
          double ly = (Ly + (f.ty * ar + f.by * br) * p.light_radius) - py;
          double lz = (Lz + (f.tz * ar + f.bz * br) * p.light_radius) - pz;
          norm3(lx, ly, lz);
          // shader.py:126-128 in its any-hit form, as k_primary_aovs' lit: lit unless some shape is
          // strictly nearer than the hit shape itself along l from the nudged point
          const double tself = isect_t(gh, qx, qy, qz, qq, lx, ly, lz, nan);
          if (nothing_nearer(sc, nsph, qx, qy, qz, qq, lx, ly, lz, tself, hs)) ++lit;
        }
        soft = (float)div_cr((double)lit, (double)ns);
      }
    }
  }
  if (live) {
    if (p.ao) __builtin_nontemporal_store(ao, p.ao + i);
    if (p.soft) __builtin_nontemporal_store(soft, p.soft + i);
  }
}

}  // namespace

extern "C" int rtx_occlusion(const double* scene, int n_spheres, const int32_t* id, const double* position,
                             const double* normal, int64_t n, const double* table, int side, const double* rot,
                             double max_distance, double light_radius, float* ao, float* soft_lit, void* stream) {
  if (!scene) return rtx_fail(RTX_E_ARG, "null scene pointer");
  if (!id || !position || !normal) return rtx_fail(RTX_E_ARG, "null primary-hit pass pointer (id, position, normal)");
  if (!table || !rot) return rtx_fail(RTX_E_ARG, "null sample table pointer (table, rot)");
  if (!ao && !soft_lit) return rtx_fail(RTX_E_ARG, "no pass requested: both output pointers are null");
  if (n_spheres < 1 || n_spheres > RTX_MAX_SPHERES) return rtx_fail(RTX_E_ARG, "n_spheres out of range");
  if (side < 1 || side > 8) return rtx_fail(RTX_E_ARG, "side out of range (1..8)");
  if (n < 0) return rtx_fail(RTX_E_ARG, "negative ray count");
  if (!(max_distance > 0.0 && max_distance <= FARAWAY))
    return rtx_fail(RTX_E_ARG, "max_distance must lie in (0, 1e39]");
  if (!(light_radius >= 0.0 && light_radius <= 1.7976931348623157e308))
    return rtx_fail(RTX_E_ARG, "light_radius must be finite and not negative");
  if (n == 0) return RTX_OK;
  OccParams p{scene, n_spheres, (const int*)id, position, normal, n, table, side, rot, max_distance, light_radius,
              ao, soft_lit};
  hipLaunchKernelGGL(k_occlusion, dim3((unsigned)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, (hipStream_t)stream, p);
  return rtx_launched("k_occlusion");
}
