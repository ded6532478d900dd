// rtx_glass_walk.inc — the body of k_trace_glass and k_trace_glass_env, included into both (not a unit, not a
// header): `p` is the kernel's parameter, `env` the environment's fields and ENV whether a popped ray that
// meets no shape adds env(D) (rtx_env.h). One text, so that k_trace_glass compiles from the tokens it had
// before the environment: a template function inlined into it changed its machine code (DESIGN.md §16).
  const int64_t w = (int64_t)blockIdx.x * 64 + threadIdx.x;
  if (w >= p.n_workers) return;
  const cdouble* sc = (const cdouble*)p.scene;
  // a blob that is not a packed scene of p.nsph spheres: every ray a miss
  const int nsph = (sc[RTX_H_MAGIC] == RTX_MAGIC && sc[RTX_H_NSPH] == (double)p.nsph) ? p.nsph : 0;
  const cdouble* geo = sc + RTX_HDR_WORDS;
  const double* tab = p.scene + RTX_HDR_WORDS;
  const double* mtab = tab + nsph * RTX_GEOM_WORDS;
  const int B = p.max_bounces;
  const int cap = glass_stack_entries(B);
  const bool tree = sc[RTX_H_NNODES] != 0.0 && nsph >= kGeneralTreeMin;
  const double nan = __builtin_nan("");  // the reference expressions in every sphere test (SphTest)
  const RayStack S{p.stack, p.n_workers, w};
  Params po{};  // what write_out reads
  po.out = p.out;
  po.out_kind = p.out_kind;
  po.n = p.n;
  for (int64_t i = w; i < p.n; i += p.n_workers) {
    {
      const int64_t s = p.org_stride;
      const int64_t j = s ? i : 0;
      S.push(0, p.org[j], p.org[s + j + (s ? 0 : 1)], p.org[2 * s + j + (s ? 0 : 2)], p.dir[i], p.dir[p.n + i],
             p.dir[2 * p.n + i], 1.0, 0);
    }
    int sp = 1;  // pending rays
    double ar = 0.0, ag = 0.0, ab = 0.0;
    // the ray whose hits are being shaded: `left` of them to go, the next one at or after shape `next`
    double ox = 0.0, oy = 0.0, oz = 0.0, dx = 0.0, dy = 0.0, dz = 0.0, oo = 0.0, wt = 0.0, tmin = FARAWAY;
    int level = 0, left = 0, next = 0;
    for (;;) {
      int h = nsph;
      if (left == 0) {
        if (sp == 0) break;
        --sp;
        ox = S.at(sp, 0); oy = S.at(sp, 1); oz = S.at(sp, 2);
        dx = S.at(sp, 3); dy = S.at(sp, 4); dz = S.at(sp, 5);
        wt = S.at(sp, 6);
        level = (int)S.at(sp, 7);
        oo = dot3(ox, oy, oz, ox, oy, oz);
        // the nearest distance (base.py:97-98), how many shapes share it and the first in scene order
        tmin = FARAWAY;
        int nh = 0, first = nsph;
        nearest_count(sc, nsph, tree, ox, oy, oz, oo, dx, dy, dz, tmin, nh, first);
        left = tmin != FARAWAY ? nh : 0;  // (nearest != FARAWAY) & (t == nearest), base.py:102-103
        if (left == 0) {
          if constexpr (ENV) {  // a miss: the environment in the ray's direction, summed like a hit's colour
            double er, eg, eb;
            env_radiance(env, dx, dy, dz, er, eg, eb);
            ar = __builtin_fma(wt, er, ar);
            ag = __builtin_fma(wt, eg, ag);
            ab = __builtin_fma(wt, eb, ab);
          }
          continue;
        }
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
      Hit s;
      Work<false> nowk;
      shade<true>(sc, geo, tab, nsph, h, ox, oy, oz, dx, dy, dz, tmin, s, nan, nowk);
      const bool weighted = s.lit && s.g != 0.0;
      double xr, xg, xb;
      hit_color<true>(mtab + h * RTX_MAT_WORDS, sc, s.dli, s.di, s.tk, s.lit, weighted, s.spec, s.va, 0.0, 0.0, 0.0,
                      xr, xg, xb);
      ar = __builtin_fma(wt, xr, ar);
      ag = __builtin_fma(wt, xg, ag);
      ab = __builtin_fma(wt, xb, ab);
      if (level >= B) continue;  // the next level is black
      if (weighted) {  // the reflected ray, (R * 0.5) * g (shader.py:106)
        if (sp < cap) {
          double rx = dx, ry = dy, rz = dz;
          reflect_dir(rx, ry, rz, s.nx, s.ny, s.nz);
          S.push(sp, s.qx, s.qy, s.qz, rx, ry, rz, (wt * 0.5) * s.g, level + 1);
          ++sp;
        } else {
          atomicOr(p.status, (uint32_t)RTX_ST_STACK_OVERFLOW);
        }
      }
      const double tg = p.glass[h];
      if (tg != 0.0) {
        const double c = dot3(dx, dy, dz, s.nx, s.ny, s.nz);
        if (c < 0.0) {  // met from outside (a hit from inside gets no transmitted ray)
          if (sp < cap) {
            const double* gh = tab + h * RTX_GEOM_WORDS;
            const double px = ox + dx * tmin, py = oy + dy * tmin, pz = oz + dz * tmin;  // :73, as shade has it
            double qx, qy, qz, rx, ry, rz;
            through_ball(px, py, pz, dx, dy, dz, s.nx, s.ny, s.nz, c, gh[RTX_G_CX], gh[RTX_G_CY], gh[RTX_G_CZ],
                         gh[RTX_G_INVR], p.glass[nsph + h], qx, qy, qz, rx, ry, rz);
            S.push(sp, qx, qy, qz, rx, ry, rz, wt * tg, level + 1);
            ++sp;
          } else {
            atomicOr(p.status, (uint32_t)RTX_ST_STACK_OVERFLOW);
          }
        }
      }
    }
    write_out(po, i, ar, ag, ab);
  }
