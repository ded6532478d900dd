// rtx_mesh.hip — triangle meshes (rtx_trace_mesh): explicit rays through the spheres of a scene and the
// triangles of a mesh table, lit by a table of point lights as rtx_trace_lights lights its spheres (the
// reference's only Shape is the sphere, domain.py:43-50). The triangle test, the group rule, the normals
// and the shadow rule are written out in include/rtx_hip.h; DESIGN.md §17 has the rest. A translation
// unit of its own over the shared device text (rtx_device.h), like rtx_lights.hip: the other kernels
// compile from untouched text with untouched flags.
#include "rtx_device.h"
#include "rtx_internal.h"

namespace {

constexpr int kLightWords = 6;      // a lights table row: position, e = intensity * colour
constexpr int kMeshRayWords = 10;   // a pending ray: origin, direction, RGB weight, level
// Pending-ray stacks live in the workspace, kMeshRayWords * mesh_stack_entries(B) words per worker; the
// pool of workers is bounded by this budget and by kMeshMaxWorkers, whatever the ray count (the lights
// kernel's rule and figures)
constexpr size_t kMeshStackBudget = size_t(256) << 20;
constexpr int64_t kMeshMaxWorkers = 196608;
// waves per SIMD the kernel is compiled for: 168 VGPRs, 12 spilled. Measured against 2 (181 VGPRs, none
// spilled) and 4 (128, 77 spilled) on mesh_spec 1080p at cap 3, icosphere level 2 / 4 / 6: 1,148 / 1,391 /
// 3,582 us against 1,255 / 1,734 / 4,123 and 1,213 / 1,499 / 3,686 (profiles/mesh_waves_ab.json)
constexpr int kMeshWaves = 3;

// A hit pushes at most one ray, and a ray's hits are the spheres at its nearest distance and the triangle
// group if it ties with them: the lights kernel's count (2B + 1 for ties of three at every level).
__host__ __device__ constexpr int mesh_stack_entries(int B) { return 2 * B + 2; }

int64_t mesh_workers(int64_t n, int B) {
  const int64_t per = (int64_t)mesh_stack_entries(B) * kMeshRayWords * 8;
  int64_t w = (int64_t)(kMeshStackBudget / (size_t)per) / 64 * 64;
  if (w > kMeshMaxWorkers) w = kMeshMaxWorkers;
  const int64_t need = (n + 63) / 64 * 64;
  return need < w ? need : w;
}

struct MeshParams {
  const double* scene;
  int nsph;
  const double* mesh;
  int64_t mesh_words;
  const double* lights;  // [n_lights][6]: px, py, pz, e_r, e_g, e_b
  int n_lights;
  const double* org;
  int64_t org_stride;
  const double* dir;
  int64_t n;
  int max_bounces;
  void* out;
  int out_kind;
  uint32_t* status;  // the workspace's RTX_WS_STATUS word
  double* stack;
  int64_t n_workers;
};

// The lane's stack of pending rays, lane-interleaved like the lights kernel's
struct MeshRayStack {
  double* base;
  int64_t nw;
  int64_t w;
  __device__ __forceinline__ double& at(int e, int f) const {
    return base[((int64_t)e * kMeshRayWords + f) * nw + w];
  }
  __device__ __forceinline__ void push(int e, double ox, double oy, double oz, double dx, double dy, double dz,
                                       double wr, double wg, double wb, int level) const {
    at(e, 0) = ox; at(e, 1) = oy; at(e, 2) = oz;
    at(e, 3) = dx; at(e, 4) = dy; at(e, 5) = dz;
    at(e, 6) = wr; at(e, 7) = wg; at(e, 8) = wb;
    at(e, 9) = (double)level;
  }
};

// The checked parts of a mesh table: ntri == 0 for a table whose header does not fit its length
struct MeshView {
  const cdouble* tris;
  const cdouble* nodes;
  const double* mats;
  int ntri, nmesh, nnodes;
  int tris_at;  // the rows' word offset in the table
};

__device__ __forceinline__ MeshView mesh_view(const double* mesh, int64_t words) {
  const cdouble* h = (const cdouble*)mesh;
  MeshView m{(const cdouble*)mesh, (const cdouble*)mesh, mesh, 0, 0, 0, 0};
  const double ntri = h[RTX_MH_NTRI], nmesh = h[RTX_MH_NMESH], nnodes = h[RTX_MH_NNODES];
  const double ta = h[RTX_MH_TRIS], ma = h[RTX_MH_MATS], na = h[RTX_MH_NODES];
  const double w = (double)words;  // (at most 2^31 - 1: every product below is exact)
  const bool ok = h[RTX_MH_MAGIC] == RTX_MESH_MAGIC && h[RTX_MH_WORDS] == w && ntri >= 1.0 &&
                  ntri <= (double)RTX_MAX_TRIANGLES && nmesh >= 1.0 && nmesh <= ntri && nnodes >= 1.0 &&
                  nnodes <= 2.0 * ntri && ta >= (double)RTX_MESH_HDR_WORDS && ta + ntri * RTX_TRI_WORDS <= w &&
                  ma >= (double)RTX_MESH_HDR_WORDS && ma + nmesh * RTX_MAT_WORDS <= w &&
                  na >= (double)RTX_MESH_HDR_WORDS && na + nnodes * RTX_NODE_WORDS <= w &&
                  ta == __builtin_floor(ta) && ma == __builtin_floor(ma) && na == __builtin_floor(na) &&
                  ntri == __builtin_floor(ntri) && nmesh == __builtin_floor(nmesh) &&
                  nnodes == __builtin_floor(nnodes);
  if (ok) {
    m.tris = h + (int)ta;
    m.nodes = h + (int)na;
    m.mats = mesh + (int)ma;
    m.ntri = (int)ntri;
    m.nmesh = (int)nmesh;
    m.nnodes = (int)nnodes;
    m.tris_at = (int)ta;
  }
  return m;
}

// The triangle test of include/rtx_hip.h on a row (v0, e1, e2): whether the ray hits, and t, u, v
template <typename P>
__device__ __forceinline__ bool tri_test(const P* r, double ox, double oy, double oz, double dx, double dy, double dz,
                                         double& t, double& u, double& v) {
  const double e1x = r[RTX_T_E1], e1y = r[RTX_T_E1 + 1], e1z = r[RTX_T_E1 + 2];
  const double e2x = r[RTX_T_E2], e2y = r[RTX_T_E2 + 1], e2z = r[RTX_T_E2 + 2];
  const double tx = ox - r[RTX_T_V0], ty = oy - r[RTX_T_V0 + 1], tz = oz - r[RTX_T_V0 + 2];
  const double px = dy * e2z - dz * e2y, py = dz * e2x - dx * e2z, pz = dx * e2y - dy * e2x;
  const double det = dot3(e1x, e1y, e1z, px, py, pz);
  const double f = 1.0 / det;
  u = f * dot3(tx, ty, tz, px, py, pz);
  const double qx = ty * e1z - tz * e1y, qy = tz * e1x - tx * e1z, qz = tx * e1y - ty * e1x;
  v = f * dot3(dx, dy, dz, qx, qy, qz);
  t = f * dot3(e2x, e2y, e2z, qx, qy, qz);
  return det != 0.0 && u >= 0.0 && v >= 0.0 && u + v <= 1.0 && t > 0.0 && t < FARAWAY;
}

// A node's range of rows, clamped to the table's
__device__ __forceinline__ void leaf_range(const cdouble* nd, int ntri, int& k, int& end) {
  const int first = (int)nd[RTX_N_FIRST], cnt = (int)nd[RTX_N_COUNT];
  k = first < 0 ? 0 : first;
  end = cnt > 0 && first <= ntri - cnt ? first + cnt : (cnt > 0 ? ntri : k);
}
// Where the walk goes on after a node that no lane may hit: its skip link, at least the next node
__device__ __forceinline__ int skip_link(const cdouble* nd, int i) {
  const int s = (int)nd[RTX_N_SKIP];
  return s > i ? s : i + 1;
}

// The group's hit nearer than or at tlim: the smallest t, the lowest triangle number among equal t, and
// that triangle's row. tt comes in as FARAWAY. Stackless and wave-uniform: node and triangle rows come
// through the scalar cache, a node is entered when any lane may hit it at or before min(tlim, tt).
__device__ __forceinline__ void nearest_tri(const MeshView& m, double ox, double oy, double oz, double oo, double dx,
                                            double dy, double dz, double tlim, double& tt, int& num, int& row) {
  const RaySlab rs = ray_slab(dx, dy, dz, oo);
  int i = 0;
  while (i < m.nnodes) {
    const cdouble* nd = m.nodes + __builtin_amdgcn_readfirstlane(i) * RTX_NODE_WORDS;
    if (__ballot(node_may_hit(nd, ox, oy, oz, rs, __builtin_fmin(tlim, tt))) != 0) {
      int k, end;
      leaf_range(nd, m.ntri, k, end);
      for (; k < end; ++k) {
        const cdouble* r = m.tris + __builtin_amdgcn_readfirstlane(k) * RTX_TRI_WORDS;
        double t, u, v;
        if (tri_test(r, ox, oy, oz, dx, dy, dz, t, u, v)) {
          const int id = (int)r[RTX_T_NUM];
          if (t < tt || (t == tt && id < num)) {
            tt = t;
            num = id;
            row = k;
          }
        }
      }
      ++i;
    } else {
      i = skip_link(nd, i);
    }
  }
}

// Shadow any-hit over the triangles: `lit` stays true unless some triangle has a hit strictly nearer
// than tself along (q, l). The walk ends once no lane of the wave is still lit.
__device__ __forceinline__ bool lit_tri(const MeshView& m, double qx, double qy, double qz, double qq, double lx,
                                        double ly, double lz, double tself, bool lit) {
  const RaySlab rs = ray_slab(lx, ly, lz, qq);
  int i = 0;
  while (i < m.nnodes) {
    const cdouble* nd = m.nodes + __builtin_amdgcn_readfirstlane(i) * RTX_NODE_WORDS;
    if (__ballot(lit && node_may_hit(nd, qx, qy, qz, rs, tself)) != 0) {
      int k, end;
      leaf_range(nd, m.ntri, k, end);
      for (; k < end; ++k) {
        const cdouble* r = m.tris + __builtin_amdgcn_readfirstlane(k) * RTX_TRI_WORDS;
        double t, u, v;
        if (tri_test(r, qx, qy, qz, lx, ly, lz, t, u, v) && t < tself) lit = false;
      }
      if (__ballot(lit) == 0) break;  // every lane of the wave is in shadow
      ++i;
    } else {
      i = skip_link(nd, i);
    }
  }
  return lit;
}

// One lane per ray item; a bounded pool of workers loops over the items (the lights kernel's walk: a
// stack of pending rays and a forward-folded weight per channel). A popped ray's hits are the spheres at
// its nearest distance, in scene order, then the triangle group's if it is as near; the lanes shade one
// hit per round. A lane on a triangle takes its point's terms from the triangle's row, its material from
// the mesh's row and a shadow test with t_self = FARAWAY; everything after that is one text for both.
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(kMeshWaves, kMeshWaves)))
void k_trace_mesh(MeshParams p) {
  const int64_t w = (int64_t)blockIdx.x * 64 + threadIdx.x;
  if (w >= p.n_workers) return;
  const cdouble* sc = (const cdouble*)p.scene;
  const cdouble* lt = (const cdouble*)p.lights;
  // a blob that is not a packed scene of p.nsph spheres: no spheres
  const int nsph = (sc[RTX_H_MAGIC] == RTX_MAGIC && sc[RTX_H_NSPH] == (double)p.nsph) ? p.nsph : 0;
  const MeshView m = mesh_view(p.mesh, p.mesh_words);
  const double* tab = p.scene + RTX_HDR_WORDS;
  const double* mtab = tab + nsph * RTX_GEOM_WORDS;
  const int B = p.max_bounces;
  const int nl = p.n_lights;
  const int cap = mesh_stack_entries(B);
  const bool tree = sc[RTX_H_NNODES] != 0.0 && nsph >= kGeneralTreeMin;
  const double nan = __builtin_nan("");  // the reference expressions in every sphere test (SphTest)
  const MeshRayStack S{p.stack, p.n_workers, w};
  Params po{};  // what write_out reads
  po.out = p.out;
  po.out_kind = p.out_kind;
  po.n = p.n;
  for (int64_t i = w; i < p.n; i += p.n_workers) {
    {
      const int64_t s = p.org_stride;
      const int64_t j = s ? i : 0;
      S.push(0, p.org[j], p.org[s + j + (s ? 0 : 1)], p.org[2 * s + j + (s ? 0 : 2)], p.dir[i], p.dir[p.n + i],
             p.dir[2 * p.n + i], 1.0, 1.0, 1.0, 0);
    }
    int sp = 1;  // pending rays
    double ar = 0.0, ag = 0.0, ab = 0.0;
    // the ray whose hits are being shaded: `left` spheres to go, the next one at or after `next`, then
    // the triangle of row `trow` if `tri`
    double ox = 0.0, oy = 0.0, oz = 0.0, dx = 0.0, dy = 0.0, dz = 0.0, oo = 0.0, tmin = FARAWAY;
    double wr = 0.0, wg = 0.0, wb = 0.0;
    int level = 0, left = 0, next = 0, trow = 0;
    bool tri = false;
    for (;;) {
      int h = nsph;  // the sphere shaded this round; nsph: the triangle
      if (left == 0 && !tri) {
        if (sp == 0) break;
        --sp;
        ox = S.at(sp, 0); oy = S.at(sp, 1); oz = S.at(sp, 2);
        dx = S.at(sp, 3); dy = S.at(sp, 4); dz = S.at(sp, 5);
        wr = S.at(sp, 6); wg = S.at(sp, 7); wb = S.at(sp, 8);
        level = (int)S.at(sp, 9);
        oo = dot3(ox, oy, oz, ox, oy, oz);
        // the spheres' nearest distance (base.py:97-98), how many share it and the first in scene order
        tmin = FARAWAY;
        int nh = 0, first = nsph;
        nearest_count(sc, nsph, tree, ox, oy, oz, oo, dx, dy, dz, tmin, nh, first);
        // the triangle group at or before it
        double tt = FARAWAY;
        int num = 0x7fffffff;
        nearest_tri(m, ox, oy, oz, oo, dx, dy, dz, tmin, tt, num, trow);
        tri = tt != FARAWAY && tt <= tmin;
        if (tt < tmin) {  // (the spheres are farther: none shades)
          tmin = tt;
          nh = 0;
        }
        left = tmin != FARAWAY ? nh : 0;  // (nearest != FARAWAY) & (t == nearest), base.py:102-103
        if (left == 0 && !tri) continue;
        next = first;
      }
      if (left > 0) {  // the next sphere in scene order at the nearest distance
        for (int s = next; s < nsph; ++s) {
          if (isect(tab + s * RTX_GEOM_WORDS, ox, oy, oz, oo, dx, dy, dz) == tmin) {
            h = s;
            break;
          }
        }
        if (h == nsph) {  // (cannot happen: `left` counted it)
          left = 0;
          continue;
        }
        next = h + 1;
        --left;
      } else {
        tri = false;
      }
      const bool on_tri = h == nsph;

      // NumpyShader.create (shader.py:63-112) of the hit, the light's terms once per table row
      const double px = ox + dx * tmin, py = oy + dy * tmin, pz = oz + dz * tmin;  // :73
      const double* gh = tab;  // (read by the lanes on a sphere only)
      const double* mh;
      double nx, ny, nz, qx, qy, qz;
      if (on_tri) {
        const double* r = p.mesh + (m.tris_at + (int64_t)trow * RTX_TRI_WORDS);
        int mi = (int)r[RTX_T_MESH];
        mi = mi < 0 ? 0 : (mi < m.nmesh ? mi : m.nmesh - 1);
        mh = m.mats + mi * RTX_MAT_WORDS;
        double gx = r[RTX_T_NG], gy = r[RTX_T_NG + 1], gz = r[RTX_T_NG + 2];
        if (dot3(gx, gy, gz, dx, dy, dz) > 0.0) {  // the face normal opposes the ray
          gx = -gx;
          gy = -gy;
          gz = -gz;
        }
        nx = gx;
        ny = gy;
        nz = gz;
        if (r[RTX_T_SMOOTH] != 0.0) {
          double t, u, v;
          tri_test(r, ox, oy, oz, dx, dy, dz, t, u, v);
          const double w0 = (1.0 - u) - v;
          nx = (w0 * r[RTX_T_N0] + u * r[RTX_T_N1]) + v * r[RTX_T_N2];
          ny = (w0 * r[RTX_T_N0 + 1] + u * r[RTX_T_N1 + 1]) + v * r[RTX_T_N2 + 1];
          nz = (w0 * r[RTX_T_N0 + 2] + u * r[RTX_T_N1 + 2]) + v * r[RTX_T_N2 + 2];
          norm3(nx, ny, nz, nan);
          if (dot3(nx, ny, nz, gx, gy, gz) < 0.0) {
            nx = -nx;
            ny = -ny;
            nz = -nz;
          }
        }
        qx = px + gx * 0.0001;  // :77 with the face normal
        qy = py + gy * 0.0001;
        qz = pz + gz * 0.0001;
      } else {
        gh = tab + h * RTX_GEOM_WORDS;
        mh = mtab + h * RTX_MAT_WORDS;
        const double inv_r = gh[RTX_G_INVR];
        nx = (px - gh[RTX_G_CX]) * inv_r;  // :74 (not renormalised)
        ny = (py - gh[RTX_G_CY]) * inv_r;
        nz = (pz - gh[RTX_G_CZ]) * inv_r;
        qx = px + nx * 0.0001;  // :77
        qy = py + ny * 0.0001;
        qz = pz + nz * 0.0001;
      }
      const double qq = dot3(qx, qy, qz, qx, qy, qz);
      // the sphere whose own test the shadow searches skip: the wave's, when its lanes agree (a lane on a
      // triangle agrees with none)
      const int h0 = __builtin_amdgcn_readfirstlane(h);
      const int hs = __ballot(h != h0) == 0 ? h0 : nsph;
      const double g = mh[RTX_M_G];
      const double dg = mh[RTX_M_DG];
      const double igain = mh[RTX_M_IG];
      double vx = sc[RTX_H_CAM + 0] - px, vy = sc[RTX_H_CAM + 1] - py, vz = sc[RTX_H_CAM + 2] - pz;
      {  // :76 (towards the camera on every level)
        const double rv = inv_mag_shade(dot3(vx, vy, vz, vx, vy, vz));
        vx = vx * rv;
        vy = vy * rv;
        vz = vz * rv;
      }
      // the texture's colour at the hit (TextureChecker :29-32, ImageTexture shape.py:66-79, Texture :17-19)
      double tr, tg, tb;
      const double tex = mh[RTX_M_TEX];
      if (tex == RTX_TEX_CHECKER) {
        tr = tg = tb = (trunc_parity(px * 2.0) == trunc_parity(pz * 2.0)) ? 1.0 : 0.0;
      } else if (tex == RTX_TEX_IMAGE && !on_tri) {
        const double* t = p.scene + ((int64_t)mh[RTX_M_TR] + 3 * (int64_t)image_texel(mh, gh, px, py, pz));
        tr = t[0];
        tg = t[1];
        tb = t[2];
      } else {
        tr = mh[RTX_M_TR];
        tg = mh[RTX_M_TG];
        tb = mh[RTX_M_TB];
      }
      double dr = 0.0, dgr = 0.0, db = 0.0;  // diffuse, summed over the lights
      double xr = 0.0, xg = 0.0, xb = 0.0;   // glossy with a black reflection
      double er = 0.0, eg = 0.0, eb = 0.0;   // sum_i lit_i e_i: what the reflected colour is weighted by
      for (int li = 0; li < nl; ++li) {
        const cdouble* row = lt + __builtin_amdgcn_readfirstlane(li) * kLightWords;
        const double e0 = row[3], e1 = row[4], e2 = row[5];
        double lx = row[0] - px, ly = row[1] - py, lz = row[2] - pz;
        norm3(lx, ly, lz, nan);  // :75
        // _calculate_shadow (:126-128) in its any-hit form: lit unless some shape is strictly nearer than
        // the hit sphere itself along L from the nudged point; a triangle's own distance is FARAWAY
        double tself = FARAWAY;
        if (!on_tri) tself = isect_t(gh, qx, qy, qz, qq, lx, ly, lz, nan);
        bool lit = nothing_nearer(sc, nsph, qx, qy, qz, qq, lx, ly, lz, tself, hs);
        if (__ballot(lit) != 0) lit = lit_tri(m, qx, qy, qz, qq, lx, ly, lz, tself, lit);
        if (__ballot(lit) == 0) continue;  // no lane of the wave is lit by this light: every term is x * 0
        const double litf = lit ? 1.0 : 0.0;
        const double dli = max0(dot3(nx, ny, nz, lx, ly, lz));  // :138
        dr = dr + (((tr * dli) * litf) * dg) * e0;
        dgr = dgr + (((tg * dli) * litf) * dg) * e1;
        db = db + (((tb * dli) * litf) * dg) * e2;
        if (__ballot(lit && g != 0.0) != 0) {
          const double spec = (lit && g != 0.0) ? specular(mh, g, nx, ny, nz, lx, ly, lz, vx, vy, vz, nan) : 0.0;
          const double sg = (spec * g) * litf;  // :106 with R = 0
          xr = xr + sg * e0;
          xg = xg + sg * e1;
          xb = xb + sg * e2;
        }
        er = er + litf * e0;
        eg = eg + litf * e1;
        eb = eb + litf * e2;
      }
      // dome (:239-242), light_direction (0, 1, 0): N.(0, 1, 0) is ny for finite N
      const int ndome = (int)sc[RTX_H_NDOME];
      double di = 0.0;
      for (int j = 0; j < ndome; ++j) di = di + sc[RTX_H_DOMEI + j] * max0(ny);
      // thin-film iridescence (:186-232); zero when iridescence_gain == 0
      double ir = 0.0, ig = 0.0, ib = 0.0;
      if (igain != 0.0) {
        const double va = clip01(dot3(nx, ny, nz, vx, vy, vz));  // :201
        const double af = fabs(va - 0.5) * 2.0;  // :204
        const double phase = ((af * RTX_PI) * mh[RTX_M_TFT]) * 10.0;  // :208
        const double ip = sin_ref(sc, phase, nan);  // :211
        const double hsh = mh[RTX_M_HS], omhs = mh[RTX_M_1MHS];
        const double r = ip * hsh + omhs * (1.0 - ip);  // :221
        const double gg = ip * omhs + hsh * (1.0 - ip);  // :222
        const double b = 0.5 + 0.5 * ip;  // :223
        const double tw = mh[RTX_M_TFW];
        ir = (r * tw) * igain;  // :229-232
        ig = (gg * tw) * igain;
        ib = (b * tw) * igain;
      }
      const double cr = (((0.004 + dr) + sc[RTX_H_DOMEC + 0] * di) + xr) + ir;
      const double cg = (((0.004 + dgr) + sc[RTX_H_DOMEC + 1] * di) + xg) + ig;
      const double cb = (((0.004 + db) + sc[RTX_H_DOMEC + 2] * di) + xb) + ib;
      ar = ar + wr * cr;
      ag = ag + wg * cg;
      ab = ab + wb * cb;
      if (level >= B) continue;  // the next level is black
      // the reflected ray, (R * 0.5) * g per light that reaches the hit (shader.py:106); not traced where
      // it is multiplied by zero
      if (g != 0.0 && (er != 0.0 || eg != 0.0 || eb != 0.0)) {
        if (sp < cap) {
          double rx = dx, ry = dy, rz = dz;
          reflect_dir(rx, ry, rz, nx, ny, nz, nan);
          S.push(sp, qx, qy, qz, rx, ry, rz, ((wr * 0.5) * g) * er, ((wg * 0.5) * g) * eg, ((wb * 0.5) * g) * eb,
                 level + 1);
          ++sp;
        } else {
          atomicOr(p.status, (uint32_t)RTX_ST_STACK_OVERFLOW);
        }
      }
    }
    write_out(po, i, ar, ag, ab);
  }
}

}  // namespace

extern "C" size_t rtx_mesh_workspace_bytes(int64_t n_rays, int max_bounces) {
  if (n_rays < 0 || max_bounces < 0 || max_bounces > RTX_MESH_MAX_BOUNCES) return 0;
  return (size_t)RTX_WS_HDR_BYTES +
         (size_t)mesh_workers(n_rays, max_bounces) * mesh_stack_entries(max_bounces) * kMeshRayWords * 8;
}

extern "C" int rtx_trace_mesh(const double* scene, int n_spheres, const double* mesh, int64_t mesh_words,
                              const double* lights, int n_lights, const double* origins, int64_t origin_stride,
                              const double* dirs, int64_t n, int max_bounces, void* out, int out_kind, void* workspace,
                              size_t workspace_bytes, void* stream) {
  if (!scene) return rtx_fail(RTX_E_ARG, "null scene pointer");
  if (!mesh) return rtx_fail(RTX_E_ARG, "null mesh table pointer");
  if (!lights) return rtx_fail(RTX_E_ARG, "null lights table pointer");
  if (!origins || !dirs) return rtx_fail(RTX_E_ARG, "null ray pointer (origins, dirs)");
  if (!out) return rtx_fail(RTX_E_ARG, "null output pointer");
  if (!workspace) return rtx_fail(RTX_E_ARG, "null workspace pointer");
  if (n_spheres < 0 || n_spheres > RTX_MAX_SPHERES) return rtx_fail(RTX_E_ARG, "n_spheres out of range");
  if (mesh_words < RTX_MESH_HDR_WORDS || mesh_words > INT32_MAX)
    return rtx_fail(RTX_E_ARG, "mesh_words out of range (%d..2^31 - 1)", (int)RTX_MESH_HDR_WORDS);
  if (n_lights < 1 || n_lights > RTX_MAX_POINT_LIGHTS)
    return rtx_fail(RTX_E_ARG, "n_lights out of range (1..%d)", (int)RTX_MAX_POINT_LIGHTS);
  if (max_bounces < 0 || max_bounces > RTX_MESH_MAX_BOUNCES)
    return rtx_fail(RTX_E_ARG, "max_bounces out of range (0..%d): a mesh scene needs a finite cap",
                    (int)RTX_MESH_MAX_BOUNCES);
  if (out_kind != RTX_OUT_F32_SOA && out_kind != RTX_OUT_F64_SOA && out_kind != RTX_OUT_U8_HWC)
    return rtx_fail(RTX_E_ARG, "bad out_kind %d", out_kind);
  if (n < 0) return rtx_fail(RTX_E_ARG, "negative ray count");
  if (origin_stride != 0 && origin_stride != n)
    return rtx_fail(RTX_E_ARG, "origin_stride must be 0 (a shared origin) or n");
  const size_t need = rtx_mesh_workspace_bytes(n, max_bounces);
  if (workspace_bytes < need)
    return rtx_fail(RTX_E_WORKSPACE, "workspace too small: %zu < %zu bytes (rtx_mesh_workspace_bytes)",
                    workspace_bytes, need);
  if (n == 0) return RTX_OK;
  MeshParams p{};
  p.scene = scene;
  p.nsph = n_spheres;
  p.mesh = mesh;
  p.mesh_words = mesh_words;
  p.lights = lights;
  p.n_lights = n_lights;
  p.org = origins;
  p.org_stride = origin_stride;
  p.dir = dirs;
  p.n = n;
  p.max_bounces = max_bounces;
  p.out = out;
  p.out_kind = out_kind;
  p.status = (uint32_t*)workspace + RTX_WS_STATUS;
  p.stack = (double*)((uint8_t*)workspace + RTX_WS_HDR_BYTES);
  p.n_workers = mesh_workers(n, max_bounces);
  hipLaunchKernelGGL(k_trace_mesh, dim3((unsigned)(p.n_workers / 64)), dim3(64), 0, (hipStream_t)stream, p);
  return rtx_launched("k_trace_mesh");
}
