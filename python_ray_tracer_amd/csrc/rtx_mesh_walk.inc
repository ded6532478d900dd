// rtx_mesh_walk.inc — the body of k_trace_mesh and k_trace_mesh_uv, included into both (not a unit, not a
// header): `p` is the kernel's parameter and UV whether a lane on a triangle of an image-textured mesh takes
// its texture colour from the table's UV part and texel blocks (mesh_uv_colour). One text, so that
// k_trace_mesh compiles from the tokens it had before (the pattern of rtx_lights_walk.inc, DESIGN.md §16).
  const int64_t w = (int64_t)blockIdx.x * 64 + threadIdx.x;
  if (w >= p.n_workers) return;
  const cdouble* sc = (const cdouble*)p.scene;
  const cdouble* lt = (const cdouble*)p.lights;
  // a blob that is not a packed scene of p.nsph spheres: no spheres
  const int nsph = (sc[RTX_H_MAGIC] == RTX_MAGIC && sc[RTX_H_NSPH] == (double)p.nsph) ? p.nsph : 0;
  const MeshView m = mesh_view(p.mesh, p.mesh_words);
  MeshUvParts uvp{0, 0};  // (read by the UV build alone)
  if constexpr (UV) uvp = mesh_uv_parts(p.mesh, p.mesh_words, m);
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
      } else if (UV && tex == RTX_TEX_IMAGE) {  // on a triangle: u, v of the hit again, from the row (the same bits)
        double t, u, v;
        tri_test(p.mesh + (m.tris_at + (int64_t)trow * RTX_TRI_WORDS), ox, oy, oz, dx, dy, dz, t, u, v);
        mesh_uv_colour(p.mesh, p.mesh_words, uvp, mh, trow, u, v, tr, tg, tb);
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
