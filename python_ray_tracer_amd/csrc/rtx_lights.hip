// rtx_lights.hip — several point lights with intensity and colour (rtx_trace_lights): explicit rays
// through a scene that every point light of a table lights, each with e = intensity * colour per
// channel (the reference lights with scene.lights[0] alone, white, of strength 1: main.py "TODO: use
// multiple lights", domain.py "class PointLight:  # TODO: add intensity"). The arithmetic of a hit is
// written out in include/rtx_hip.h; DESIGN.md §15 has the rest. A translation unit of its own over the
// shared device text (rtx_device.h), like rtx_glass.hip: the render kernels compile from untouched text
// with untouched flags.
#include "rtx_device.h"
#include "rtx_internal.h"

namespace {

constexpr int kLightWords = 6;    // a table row: position, e = intensity * colour
constexpr int kLightRayWords = 10;  // a pending ray: origin, direction, RGB weight, level
// Pending-ray stacks live in the workspace, kLightRayWords * lights_stack_entries(B) words per worker;
// the pool of workers is bounded by this budget and by kLightsMaxWorkers, whatever the ray count (the
// glass kernel's rule)
constexpr size_t kLightsStackBudget = size_t(256) << 20;
// 3,072 waves: kLightsWaves per SIMD on a 256-CU part, all resident (the glass kernel's pool; not
// measured against another for this kernel)
constexpr int64_t kLightsMaxWorkers = 196608;
// waves per SIMD the kernel is compiled for: 168 VGPRs, 8 spilled. Measured against 2 (189 VGPRs, none
// spilled) and 4 (128, 51 spilled) on lights_spec 1080p at cap 3, one light / three / eight: 111.6 / 170.6 /
// 319.5 us against 144.4 / 218.4 / 409.4 and 179.4 / 230.0 / 372.4 (profiles/lights_waves_ab.json)
constexpr int kLightsWaves = 3;

// A hit pushes at most one ray (the reflected one), and a ray's hits are the shapes at its nearest
// distance. A chain needs 1 entry; in a tree whose every ray meets t shapes each popped ray leaves
// t - 1 siblings below it, so after the pushes of level k (the last that pushes is B - 1) the stack holds
// (t - 1) k + t: B + 1 for ties of two at every level, 2B + 1 for ties of three.
__host__ __device__ constexpr int lights_stack_entries(int B) { return 2 * B + 2; }

int64_t lights_workers(int64_t n, int B) {
  const int64_t per = (int64_t)lights_stack_entries(B) * kLightRayWords * 8;
  int64_t w = (int64_t)(kLightsStackBudget / (size_t)per) / 64 * 64;
  if (w > kLightsMaxWorkers) w = kLightsMaxWorkers;
  const int64_t need = (n + 63) / 64 * 64;
  return need < w ? need : w;
}

struct LightsParams {
  const double* scene;
  int nsph;
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

// The lane's stack of pending rays, lane-interleaved like the glass kernel's: word f of entry e of 64
// consecutive workers is one contiguous run.
struct LightRayStack {
  double* base;
  int64_t nw;
  int64_t w;
  __device__ __forceinline__ double& at(int e, int f) const {
    return base[((int64_t)e * kLightRayWords + f) * nw + w];
  }
  __device__ __forceinline__ void push(int e, double ox, double oy, double oz, double dx, double dy, double dz,
                                       double wr, double wg, double wb, int level) const {
    at(e, 0) = ox; at(e, 1) = oy; at(e, 2) = oz;
    at(e, 3) = dx; at(e, 4) = dy; at(e, 5) = dz;
    at(e, 6) = wr; at(e, 7) = wg; at(e, 8) = wb;
    at(e, 9) = (double)level;
  }
};

// One lane per ray item; a bounded pool of workers loops over the items. A lane walks its ray tree with
// a stack of pending rays and a forward-folded weight per channel (the glass kernel's walk): every
// shaded hit adds W[c] * (its colour with a black reflection) and pushes the reflected ray with weight
// ((W[c] * 0.5) * g) * sum_i lit_i e_i[c]. The lanes of a wave that need a new ray pop and search
// together; a lane at a tie shades its shapes one per round in scene order. The loop over the lights is
// wave-uniform (the table row comes through the scalar cache): one any-hit shadow search per light, and
// the specular of a light only where some lane of the wave is lit by it.
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(kLightsWaves, kLightsWaves)))
void k_trace_lights(LightsParams p) {
  const int64_t w = (int64_t)blockIdx.x * 64 + threadIdx.x;
  if (w >= p.n_workers) return;
  const cdouble* sc = (const cdouble*)p.scene;
  const cdouble* lt = (const cdouble*)p.lights;
  // a blob that is not a packed scene of p.nsph spheres: every ray a miss
  const int nsph = (sc[RTX_H_MAGIC] == RTX_MAGIC && sc[RTX_H_NSPH] == (double)p.nsph) ? p.nsph : 0;
  const double* tab = p.scene + RTX_HDR_WORDS;
  const double* mtab = tab + nsph * RTX_GEOM_WORDS;
  const int B = p.max_bounces;
  const int nl = p.n_lights;
  const int cap = lights_stack_entries(B);
  const bool tree = sc[RTX_H_NNODES] != 0.0 && nsph >= kGeneralTreeMin;
  const double nan = __builtin_nan("");  // the reference expressions in every sphere test (SphTest)
  const LightRayStack S{p.stack, p.n_workers, w};
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
    // the ray whose hits are being shaded: `left` of them to go, the next one at or after shape `next`
    double ox = 0.0, oy = 0.0, oz = 0.0, dx = 0.0, dy = 0.0, dz = 0.0, oo = 0.0, tmin = FARAWAY;
    double wr = 0.0, wg = 0.0, wb = 0.0;
    int level = 0, left = 0, next = 0;
    for (;;) {
      int h = nsph;
      if (left == 0) {
        if (sp == 0) break;
        --sp;
        ox = S.at(sp, 0); oy = S.at(sp, 1); oz = S.at(sp, 2);
        dx = S.at(sp, 3); dy = S.at(sp, 4); dz = S.at(sp, 5);
        wr = S.at(sp, 6); wg = S.at(sp, 7); wb = S.at(sp, 8);
        level = (int)S.at(sp, 9);
        oo = dot3(ox, oy, oz, ox, oy, oz);
        // the nearest distance (base.py:97-98), how many shapes share it and the first in scene order
        tmin = FARAWAY;
        int nh = 0, first = nsph;
        nearest_count(sc, nsph, tree, ox, oy, oz, oo, dx, dy, dz, tmin, nh, first);
        left = tmin != FARAWAY ? nh : 0;  // (nearest != FARAWAY) & (t == nearest), base.py:102-103
        if (left == 0) continue;
        h = first;
      } else {  // a tie: the next shape in scene order at the nearest distance
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
      }
      next = h + 1;
      --left;

      // NumpyShader.create (shader.py:63-112) of the hit, the light's terms once per table row
      const double* gh = tab + h * RTX_GEOM_WORDS;
      const double* mh = mtab + h * RTX_MAT_WORDS;
      const double px = ox + dx * tmin, py = oy + dy * tmin, pz = oz + dz * tmin;  // :73
      const double inv_r = gh[RTX_G_INVR];
      const double nx = (px - gh[RTX_G_CX]) * inv_r;  // :74 (not renormalised)
      const double ny = (py - gh[RTX_G_CY]) * inv_r;
      const double nz = (pz - gh[RTX_G_CZ]) * inv_r;
      const double qx = px + nx * 0.0001, qy = py + ny * 0.0001, qz = pz + nz * 0.0001;  // :77
      const double qq = dot3(qx, qy, qz, qx, qy, qz);
      // the shape whose own test the shadow searches skip: the wave's, when its lanes agree
      const int h0 = __builtin_amdgcn_readfirstlane(h);
      const int hs = __ballot(h != h0) == 0 ? h0 : nsph;
      const double g = mh[RTX_M_G];
      const double dg = mh[RTX_M_DG];
      const double igain = mh[RTX_M_IG];
      double vx = sc[RTX_H_CAM + 0] - px, vy = sc[RTX_H_CAM + 1] - py, vz = sc[RTX_H_CAM + 2] - pz;
      {  // :76 (towards the camera on every level); V only feeds the specular and the iridescence
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
      } else if (tex == RTX_TEX_IMAGE) {
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
        // _calculate_shadow (:126-128) in its any-hit form: lit unless some shape is strictly nearer
        // than the hit shape itself along L from the nudged point (k_occlusion's soft_lit call)
        const double tself = isect_t(gh, qx, qy, qz, qq, lx, ly, lz, nan);
        const bool lit = nothing_nearer(sc, nsph, qx, qy, qz, qq, lx, ly, lz, tself, hs);
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

extern "C" size_t rtx_lights_workspace_bytes(int64_t n_rays, int max_bounces) {
  if (n_rays < 0 || max_bounces < 0 || max_bounces > RTX_LIGHTS_MAX_BOUNCES) return 0;
  return (size_t)RTX_WS_HDR_BYTES +
         (size_t)lights_workers(n_rays, max_bounces) * lights_stack_entries(max_bounces) * kLightRayWords * 8;
}

extern "C" int rtx_trace_lights(const double* scene, int n_spheres, const double* lights, int n_lights,
                                const double* origins, int64_t origin_stride, const double* dirs, int64_t n,
                                int max_bounces, void* out, int out_kind, void* workspace, size_t workspace_bytes,
                                void* stream) {
  if (!scene) return rtx_fail(RTX_E_ARG, "null scene pointer");
  if (!lights) return rtx_fail(RTX_E_ARG, "null lights table pointer");
  if (!origins || !dirs) return rtx_fail(RTX_E_ARG, "null ray pointer (origins, dirs)");
  if (!out) return rtx_fail(RTX_E_ARG, "null output pointer");
  if (!workspace) return rtx_fail(RTX_E_ARG, "null workspace pointer");
  if (n_spheres < 1 || n_spheres > RTX_MAX_SPHERES) return rtx_fail(RTX_E_ARG, "n_spheres out of range");
  if (n_lights < 1 || n_lights > RTX_MAX_POINT_LIGHTS)
    return rtx_fail(RTX_E_ARG, "n_lights out of range (1..%d)", (int)RTX_MAX_POINT_LIGHTS);
  if (max_bounces < 0 || max_bounces > RTX_LIGHTS_MAX_BOUNCES)
    return rtx_fail(RTX_E_ARG, "max_bounces out of range (0..%d): a multi-light scene needs a finite cap",
                    (int)RTX_LIGHTS_MAX_BOUNCES);
  if (out_kind != RTX_OUT_F32_SOA && out_kind != RTX_OUT_F64_SOA && out_kind != RTX_OUT_U8_HWC)
    return rtx_fail(RTX_E_ARG, "bad out_kind %d", out_kind);
  if (n < 0) return rtx_fail(RTX_E_ARG, "negative ray count");
  if (origin_stride != 0 && origin_stride != n)
    return rtx_fail(RTX_E_ARG, "origin_stride must be 0 (a shared origin) or n");
  const size_t need = rtx_lights_workspace_bytes(n, max_bounces);
  if (workspace_bytes < need)
    return rtx_fail(RTX_E_WORKSPACE, "workspace too small: %zu < %zu bytes (rtx_lights_workspace_bytes)",
                    workspace_bytes, need);
  if (n == 0) return RTX_OK;
  LightsParams p{};
  p.scene = scene;
  p.nsph = n_spheres;
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
  p.n_workers = lights_workers(n, max_bounces);
  hipLaunchKernelGGL(k_trace_lights, dim3((unsigned)(p.n_workers / 64)), dim3(64), 0, (hipStream_t)stream, p);
  return rtx_launched("k_trace_lights");
}
