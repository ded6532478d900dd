// rtx_mesh_aov.hip — the primary-hit render passes of a mesh scene (rtx_mesh_aovs): depth, shape id, hit
// count, position, shading and geometric normal, albedo, a shadow bit per light, triangle number and
// barycentrics of the level-0 hit of every explicit ray through the spheres of a scene and the triangles of
// a mesh table. Each value is an intermediate of k_trace_mesh's own arithmetic (rtx_mesh_walk.inc) written out
// instead of shaded: k_primary_aovs' shape (rtx_aov.hip) over the walks of rtx_mesh_device.h. The contract
// is in include/rtx_hip.h; DESIGN.md §20 has the rest. A translation unit of its own, like rtx_aov.hip: the
// other kernels compile from untouched text with untouched flags.
#include "rtx_device.h"
#include "rtx_internal.h"
#include "rtx_mesh_device.h"

namespace {

constexpr int kLightWords = 6;  // a lights table row: position, e = intensity * colour
// waves per SIMD the kernel is compiled for: 88 VGPRs, 86 SGPRs, nothing spilled, no scratch, which is also what
// the compiler takes without the attribute; 6 waves need 80 VGPRs and spill 6 of them (28 bytes of scratch per
// lane), 4 give nothing back
constexpr int kMeshAovWaves = 5;

struct MeshAovParams {
  const double* scene;
  int nsph;
  const double* mesh;
  int64_t mesh_words;
  const double* lights;  // [n_lights][6]: px, py, pz, e_r, e_g, e_b
  int n_lights;
  const int* shape_ids;  // [nsph + the table's meshes], or null: s, and nsph + mesh
  const double* org;
  int64_t org_stride;
  const double* dir;
  int64_t n;
};

// Output planes of a launch; a null pointer is a pass that was not requested (wave-uniform: kernel
// arguments), which then costs no store, and no shadow walk (lit) or texel lookup (albedo) either.
struct MeshAovOut {
  double* depth;       // [n]
  int* id;             // [n]
  int* hits;           // [n]
  double* position;    // [3][n]
  double* normal;      // [3][n]
  double* geo_normal;  // [3][n]
  double* albedo;      // [3][n]
  unsigned char* lit;  // [n]
  int* triangle;       // [n]
  double* bary;        // [2][n]
  int lit_words;       // lit is 4-byte aligned: whole waves store it as dwords
};

__device__ __forceinline__ void store3(double* plane, int64_t n, int64_t i, double x, double y, double z) {
  __builtin_nontemporal_store(x, plane + i);
  __builtin_nontemporal_store(y, plane + n + i);
  __builtin_nontemporal_store(z, plane + 2 * n + i);
}

// One lane per ray, ray i = blockIdx.x * kBlock + threadIdx.x, k_primary_aovs' linear mapping: every store
// of a wave writes one contiguous run, and a frame's rays are 64 neighbours of a pixel row, coherent enough
// for the wave-uniform walks. Sphere geometry, nodes and triangle rows of the walks come through the scalar
// cache; the hit's own row, material and texels per lane. The planes but lit are stored before the shadow
// walks, which then hold the nudged point and the hit alone.
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(kMeshAovWaves, kMeshAovWaves)))
void k_mesh_aovs(MeshAovParams p, MeshAovOut o) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  const int64_t n = p.n;
  const bool live = i < n;
  const cdouble* sc = (const cdouble*)p.scene;
  const cdouble* lt = (const cdouble*)p.lights;
  // a blob that is not a packed scene of p.nsph spheres: no spheres
  const int nsph = (sc[RTX_H_MAGIC] == RTX_MAGIC && sc[RTX_H_NSPH] == (double)p.nsph) ? p.nsph : 0;
  const MeshView m = mesh_view(p.mesh, p.mesh_words);
  const double* tab = p.scene + RTX_HDR_WORDS;
  const double* mtab = tab + nsph * RTX_GEOM_WORDS;
  const double nan = __builtin_nan("");  // the reference expressions in every sphere test (SphTest)
  unsigned litb = 0;  // bit li: the light of row li reaches the first hit
  if (live) {
    double ox, oy, oz;
    {
      const int64_t s = p.org_stride;
      const int64_t j = s ? i : 0;
      ox = p.org[j], oy = p.org[s + j + (s ? 0 : 1)], oz = p.org[2 * s + j + (s ? 0 : 2)];
    }
    const double dx = p.dir[i], dy = p.dir[n + i], dz = p.dir[2 * n + i];
    const double oo = dot3(ox, oy, oz, ox, oy, oz);
    // the spheres' nearest distance (base.py:97-98), how many share it and the first in scene order
    double tmin = FARAWAY;
    int nh = 0, first = nsph;
    nearest_count(sc, nsph, sc[RTX_H_NNODES] != 0.0 && nsph >= kGeneralTreeMin, ox, oy, oz, oo, dx, dy, dz, tmin, nh,
                  first);
    // the triangle group at or before it
    double tt = FARAWAY;
    int num = 0x7fffffff, trow = 0;
    nearest_tri(m, ox, oy, oz, oo, dx, dy, dz, tmin, tt, num, trow);
    const bool tri = tt != FARAWAY && tt <= tmin;  // the group is at the nearest distance
    const bool on_tri = tri && tt < tmin;          // ... and no sphere is: the first hit is the triangle
    if (on_tri) tmin = tt;
    const bool hit = tmin != FARAWAY && (on_tri || nh > 0);
    const double* r = p.mesh + (m.tris_at + (int64_t)trow * RTX_TRI_WORDS);  // (read by the lanes on a triangle only)
    int mi = 0;
    if (on_tri) {
      mi = (int)r[RTX_T_MESH];
      mi = mi < 0 ? 0 : (mi < m.nmesh ? mi : m.nmesh - 1);
    }
    if (o.depth) __builtin_nontemporal_store(tmin, o.depth + i);
    if (o.id) {
      int id = -1;
      if (hit) {
        const int k = on_tri ? p.nsph + mi : first;
        id = p.shape_ids ? p.shape_ids[k] : k;
      }
      __builtin_nontemporal_store(id, o.id + i);
    }
    if (o.hits) __builtin_nontemporal_store(hit ? (on_tri ? 1 : nh + (tri ? 1 : 0)) : 0, o.hits + i);
    if (o.triangle) __builtin_nontemporal_store(on_tri ? num : -1, o.triangle + i);

    double px = 0.0, py = 0.0, pz = 0.0, nx = 0.0, ny = 0.0, nz = 0.0, gx = 0.0, gy = 0.0, gz = 0.0;
    double ar = 0.0, ag = 0.0, ab = 0.0, bu = 0.0, bv = 0.0;
    const int h = on_tri ? nsph : first;  // the sphere of the first hit; nsph: the triangle
    const double* gh = tab;               // (read by the lanes on a sphere only)
    if (hit && (o.position || o.normal || o.geo_normal || o.albedo || o.lit || o.bary)) {
      px = ox + dx * tmin, py = oy + dy * tmin, pz = oz + dz * tmin;  // shader.py:73
      const double* mh;
      if (on_tri) {
        mh = m.mats + mi * RTX_MAT_WORDS;
        gx = r[RTX_T_NG], gy = r[RTX_T_NG + 1], gz = r[RTX_T_NG + 2];
        if (dot3(gx, gy, gz, dx, dy, dz) > 0.0) {  // the face normal opposes the ray
          gx = -gx;
          gy = -gy;
          gz = -gz;
        }
        nx = gx;
        ny = gy;
        nz = gz;
        if (o.normal || o.albedo || o.bary) {  // u, v of the hit again, from the row (the same bits)
          double t;
          tri_test(r, ox, oy, oz, dx, dy, dz, t, bu, bv);
        }
        if (o.normal && r[RTX_T_SMOOTH] != 0.0) {
          const double w0 = (1.0 - bu) - bv;
          nx = (w0 * r[RTX_T_N0] + bu * r[RTX_T_N1]) + bv * r[RTX_T_N2];
          ny = (w0 * r[RTX_T_N0 + 1] + bu * r[RTX_T_N1 + 1]) + bv * r[RTX_T_N2 + 1];
          nz = (w0 * r[RTX_T_N0 + 2] + bu * r[RTX_T_N1 + 2]) + bv * r[RTX_T_N2 + 2];
          norm3(nx, ny, nz, nan);
          if (dot3(nx, ny, nz, gx, gy, gz) < 0.0) {
            nx = -nx;
            ny = -ny;
            nz = -nz;
          }
        }
      } else {
        gh = tab + h * RTX_GEOM_WORDS;
        mh = mtab + h * RTX_MAT_WORDS;
        const double inv_r = gh[RTX_G_INVR];
        gx = nx = (px - gh[RTX_G_CX]) * inv_r;  // shader.py:74 (not renormalised)
        gy = ny = (py - gh[RTX_G_CY]) * inv_r;
        gz = nz = (pz - gh[RTX_G_CZ]) * inv_r;
      }
      if (o.albedo) {  // the texture's colour at the hit (TextureChecker :29-32, ImageTexture shape.py:66-79, Texture :17-19)
        const double tex = mh[RTX_M_TEX];
        if (tex == RTX_TEX_CHECKER) {
          ar = ag = ab = (trunc_parity(px * 2.0) == trunc_parity(pz * 2.0)) ? 1.0 : 0.0;
        } else if (tex == RTX_TEX_IMAGE && !on_tri) {
          const double* t = p.scene + ((int64_t)mh[RTX_M_TR] + 3 * (int64_t)image_texel(mh, gh, px, py, pz));
          ar = t[0], ag = t[1], ab = t[2];
        } else if (tex == RTX_TEX_IMAGE) {  // a table without a UV part (wave-uniform): black, as mesh_uv_colour has it
          const MeshUvParts uvp = mesh_uv_parts(p.mesh, p.mesh_words, m);
          mesh_uv_colour(p.mesh, p.mesh_words, uvp, mh, trow, bu, bv, ar, ag, ab);
        } else {
          ar = mh[RTX_M_TR], ag = mh[RTX_M_TG], ab = mh[RTX_M_TB];
        }
      }
      if (!on_tri) bu = bv = 0.0;
    }
    if (o.position) store3(o.position, n, i, px, py, pz);
    if (o.normal) store3(o.normal, n, i, nx, ny, nz);
    if (o.geo_normal) store3(o.geo_normal, n, i, gx, gy, gz);
    if (o.albedo) store3(o.albedo, n, i, ar, ag, ab);
    if (o.bary) {
      __builtin_nontemporal_store(bu, o.bary + i);
      __builtin_nontemporal_store(bv, o.bary + n + i);
    }
    if (o.lit && hit) {
      // rtx_trace_mesh's shadow rule per row of the lights table (rtx_mesh_walk.inc): along L from the nudged
      // point Q = P + N_g * 0.0001, lit unless a sphere or a triangle is strictly nearer than the hit sphere
      // itself; a triangle's own distance is FARAWAY. The hit sphere's own test is skipped where the lanes of
      // the wave agree on it (a lane on a triangle agrees with none).
      const double qx = px + gx * 0.0001, qy = py + gy * 0.0001, qz = pz + gz * 0.0001;  // :77
      const double qq = dot3(qx, qy, qz, qx, qy, qz);
      const int h0 = __builtin_amdgcn_readfirstlane(h);
      const int hs = __ballot(h != h0) == 0 ? h0 : nsph;
      for (int li = 0; li < p.n_lights; ++li) {
        const cdouble* row = lt + __builtin_amdgcn_readfirstlane(li) * kLightWords;
        double lx = row[0] - px, ly = row[1] - py, lz = row[2] - pz;
        norm3(lx, ly, lz, nan);  // :75
        double tself = FARAWAY;
        if (!on_tri) tself = isect_t(gh, qx, qy, qz, qq, lx, ly, lz, nan);
        bool lit = nothing_nearer(sc, nsph, qx, qy, qz, qq, lx, ly, lz, tself, hs);
        // (no lane of the wave still needs the triangles of this light when the spheres shadow them all)
        if (__ballot(lit) != 0) lit = lit_tri(m, qx, qy, qz, qq, lx, ly, lz, tself, lit);
        litb |= (lit ? 1u : 0u) << li;
      }
    }
  }
  if (o.lit) {
    // one byte per ray: a whole wave (64 consecutive rays from a multiple of 64) stores its 64 bytes as 16
    // dwords built from one ballot per lights row instead of 64 byte stores; a wave that crosses the end of
    // the batch, or an unaligned plane, stores bytes
    const int lane = (int)(threadIdx.x & 63u);
    const int64_t base = i - lane;
    if (o.lit_words && base + 64 <= n) {
      uint32_t w = 0;
      for (int li = 0; li < p.n_lights; ++li) {
        const uint64_t mk = __ballot((litb >> li) & 1u);
        const uint32_t b = (uint32_t)(mk >> (4 * (lane & 15))) & 0xFu;
        w |= ((b & 1u) | ((b & 2u) << 7) | ((b & 4u) << 14) | ((b & 8u) << 21)) << li;
      }
      if (lane < 16) __builtin_nontemporal_store(w, (uint32_t*)(o.lit + base) + lane);
    } else if (live) {
      __builtin_nontemporal_store((unsigned char)litb, o.lit + i);
    }
  }
}

}  // namespace

extern "C" int rtx_mesh_aovs(const double* scene, int n_spheres, const double* mesh, int64_t mesh_words,
                             const double* lights, int n_lights, const int32_t* shape_ids, const double* origins,
                             int64_t origin_stride, const double* dirs, int64_t n, double* depth, int32_t* id,
                             int32_t* hits, double* position, double* normal, double* geometric_normal,
                             double* albedo, uint8_t* lit, int32_t* triangle, double* bary, void* stream) {
  if (!scene) return rtx_fail(RTX_E_ARG, "null scene pointer");
  if (!mesh) return rtx_fail(RTX_E_ARG, "null mesh table pointer");
  if (!lights) return rtx_fail(RTX_E_ARG, "null lights table pointer");
  if (!origins || !dirs) return rtx_fail(RTX_E_ARG, "null ray pointer (origins, dirs)");
  if (!depth && !id && !hits && !position && !normal && !geometric_normal && !albedo && !lit && !triangle && !bary)
    return rtx_fail(RTX_E_ARG, "no pass requested: every output pointer is null");
  if (n_spheres < 0 || n_spheres > RTX_MAX_SPHERES) return rtx_fail(RTX_E_ARG, "n_spheres out of range");
  if (mesh_words < RTX_MESH_HDR_WORDS || mesh_words > INT32_MAX)
    return rtx_fail(RTX_E_ARG, "mesh_words out of range (%d..2^31 - 1)", (int)RTX_MESH_HDR_WORDS);
  if (n_lights < 1 || n_lights > RTX_MAX_POINT_LIGHTS)
    return rtx_fail(RTX_E_ARG, "n_lights out of range (1..%d)", (int)RTX_MAX_POINT_LIGHTS);
  if (n < 0) return rtx_fail(RTX_E_ARG, "negative ray count");
  if (origin_stride != 0 && origin_stride != n)
    return rtx_fail(RTX_E_ARG, "origin_stride must be 0 (a shared origin) or n");
  if (n == 0) return RTX_OK;
  const MeshAovParams p{scene, n_spheres, mesh, mesh_words, lights, n_lights, shape_ids, origins, origin_stride, dirs, n};
  const MeshAovOut o{depth, id, hits, position, normal, geometric_normal, albedo, lit, triangle, bary,
                     (uintptr_t)lit % 4 == 0 ? 1 : 0};
  hipLaunchKernelGGL(k_mesh_aovs, dim3((unsigned)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, (hipStream_t)stream,
                     p, o);
  return rtx_launched("k_mesh_aovs");
}
