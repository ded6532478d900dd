// rtx_mesh_device.h — the device text that the units over a mesh table share (rtx_mesh.hip: rtx_trace_mesh,
// rtx_trace_mesh_uv; rtx_mesh_aov.hip: rtx_mesh_aovs): the checked view of a table, the triangle test, the
// wave-uniform stackless walks and the image lookup. Moved here from rtx_mesh.hip with its text unchanged, so
// that k_trace_mesh and k_trace_mesh_uv keep their machine code (profiles/mesh_aov_isa_identity.txt). The
// contract is in include/rtx_hip.h; DESIGN.md §17, §18 and §20 have the rest.
#pragma once

#include "rtx_device.h"

namespace {

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

// The two parts that rtx_trace_mesh_uv's table has after the nodes, checked against the table's length: the
// word offsets of the UV part (RTX_UV_WORDS per row of m) and of the first texel block; both 0 unless both fit
struct MeshUvParts {
  int uv_at, tex_at;
};

__device__ __forceinline__ MeshUvParts mesh_uv_parts(const double* mesh, int64_t words, const MeshView& m) {
  const cdouble* h = (const cdouble*)mesh;
  const double ua = h[RTX_MH_UVS], xa = h[RTX_MH_TEXELS], w = (double)words;
  const bool ok = m.ntri > 0 && ua >= (double)RTX_MESH_HDR_WORDS && ua == __builtin_floor(ua) &&
                  ua + (double)m.ntri * RTX_UV_WORDS <= w && xa >= (double)RTX_MESH_HDR_WORDS &&
                  xa == __builtin_floor(xa) && xa <= w;
  return ok ? MeshUvParts{(int)ua, (int)xa} : MeshUvParts{0, 0};
}

// A wrapped texel index as an int: 0 for a value outside 0..n - 1 (only a table whose coordinates exceed
// RTX_MESH_UV_MAX can make one), so that no table makes the lookup read outside its block
__device__ __forceinline__ int texel_index(double i, double n) { return i >= 0.0 && i < n ? (int)i : 0; }

// The image colour of include/rtx_hip.h at (u, v) of row `trow`: the mesh's material row `mh` names the
// texel block (word offset in the table, width, height). Black where the table has no UV part or the block
// does not lie inside the table's texel part. Per-lane loads: the row's six coordinates and four texels.
__device__ __forceinline__ void mesh_uv_colour(const double* mesh, int64_t words, const MeshUvParts& parts,
                                               const double* mh, int trow, double u, double v, double& tr,
                                               double& tg, double& tb) {
  tr = tg = tb = 0.0;
  const double off = mh[RTX_M_TR], W = mh[RTX_M_TG], H = mh[RTX_M_TB];
  const bool ok = parts.uv_at != 0 && off >= (double)parts.tex_at && off == __builtin_floor(off) && W >= 1.0 &&
                  H >= 1.0 && W == __builtin_floor(W) && H == __builtin_floor(H) &&
                  W * H <= (double)RTX_MAX_TEXELS && off + 3.0 * (W * H) <= (double)words;
  if (!ok) return;
  const double* c = mesh + (parts.uv_at + (int64_t)trow * RTX_UV_WORDS);
  const double w0 = (1.0 - u) - v;
  const double s = (w0 * c[0] + u * c[2]) + v * c[4];
  const double t = (w0 * c[1] + u * c[3]) + v * c[5];
  const double x = s * W - 0.5, y = (1.0 - t) * H - 0.5;
  const double x0 = __builtin_floor(x), y0 = __builtin_floor(y);
  const double fx = x - x0, fy = y - y0;
  const double i0 = x0 - W * __builtin_floor(x0 / W), j0 = y0 - H * __builtin_floor(y0 / H);
  const double i1 = i0 + 1.0 == W ? 0.0 : i0 + 1.0, j1 = j0 + 1.0 == H ? 0.0 : j0 + 1.0;
  const int wi = (int)W;
  const int a0 = texel_index(i0, W), a1 = texel_index(i1, W);
  const int b0 = texel_index(j0, H) * wi, b1 = texel_index(j1, H) * wi;
  const double* tx = mesh + (int64_t)off;
  const double* c00 = tx + 3 * (b0 + a0);
  const double* c01 = tx + 3 * (b0 + a1);
  const double* c10 = tx + 3 * (b1 + a0);
  const double* c11 = tx + 3 * (b1 + a1);
  const double gx = 1.0 - fx, gy = 1.0 - fy;
  tr = (c00[0] * gx + c01[0] * fx) * gy + (c10[0] * gx + c11[0] * fx) * fy;
  tg = (c00[1] * gx + c01[1] * fx) * gy + (c10[1] * gx + c11[1] * fx) * fy;
  tb = (c00[2] * gx + c01[2] * fx) * gy + (c10[2] * gx + c11[2] * fx) * fy;
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

}  // namespace
