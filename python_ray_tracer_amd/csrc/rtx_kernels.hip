// rtx_kernels.hip — the main translation unit of librtx_hip.so: the hand-written CDNA4 (gfx950)
// kernels of the python_ray_tracer render path that are launched from here, the host side of every
// render call, and the extern "C" entry points declared in include/rtx_hip.h. The device text it
// shares with the other units (rtx_small.hip, rtx_aov.hip, rtx_adaptive.hip) is csrc/rtx_device.h;
// the units are separate so that they compile in parallel and can take flags of their own when an
// A/B wants them (_build.UNIT_FLAGS).
//
// Kernels (k_render_fast: rtx_device.h; this unit instantiates and launches the culled ones, TP 1
// and 2, and rtx_small.hip the TREE = false ones of scenes below kTreeMinSpheres, TP 0)
//   k_render_general  Any bounce cap, ties included: an explicit depth-first walk of the ray tree
//                     with per-worker frame stacks in the workspace (HBM). Renders the ties of the
//                     deferred list from level 0 and resumes its deep chains from their records. Its
//                     last block resets the list counter, so the workspace is left zeroed for the
//                     next call (no per-frame memset).
//   k_ray_dirs, k_intersect, k_quantize — the remaining boundary functions.
//   k_resolve         The supersampling box filter of a k x k sample frame (rtx_resolve_samples).
#include <cstdarg>

#include "rtx_device.h"
#include "rtx_internal.h"

namespace {

// ------------------------------------------------------------------------------------------
// k_render_general: explicit depth-first ray tree (ties and any bounce cap)
// ------------------------------------------------------------------------------------------

// frame fields: the ray, its nearest distance, the next shape to examine (-1: new ray), the
// weight of its hits (the product of (0.5 g) along the path to it), the hit whose reflection is
// being traced, and the hits of the ray not yet shaded.
enum { F_OX = 0, F_OY, F_OZ, F_DX, F_DY, F_DZ, F_TMIN, F_NEXT, F_THR, F_KEY, F_LEFT };
static_assert(F_LEFT < kFrameWords, "frame layout");

struct Stack {
  double* base;
  int64_t nw;
  int64_t w;
  __device__ __forceinline__ double& at(int d, int f) const { return base[((int64_t)d * kFrameWords + f) * nw + w]; }
};

// rays_through / hits_through: per-level counts the fast kernel already made for this pixel.
// The walk sums every shaded hit's colour with a black reflection, weighted by the product of
// (0.5 g) along its path (shader.py:106-110 unrolled: the sum over the tree of hits, ties included,
// base.py:100-119), in depth-first order: on a chain without ties these are the fast kernels'
// forward-fold operations in their order, so a pixel's colour does not depend on which kernel
// traced which of its levels. rec: a resume record (deep deferral: the next ray, the colour summed
// through level L and level L + 1's weight), the walk starting at depth L + 1; or null.
template <typename Stk>
__device__ void trace_general(const Params& p, const Stk& S, double ox0, double oy0, double oz0, double dx0,
                              double dy0, double dz0, double& cr, double& cg, double& cb, int rays_through,
                              int hits_through, const double* rec = nullptr, int h_given = -1,
                              double t_given = 0.0) {
  const cdouble* sc = (const cdouble*)p.scene;
  const cdouble* geo = sc + RTX_HDR_WORDS;
  const double* tab = p.scene + RTX_HDR_WORDS;
  const double* mtab = tab + p.nsph * RTX_GEOM_WORDS;
  const int nsph = p.nsph;
  const int B = p.max_bounces;  // < 0: unbounded (bounded by the stack depth)
  // Shader.create on another shape's shader: level 0 shades with that material (RTX_H_MAT0)
  const double* mat0 = (h_given >= 0 && sc[RTX_H_MAT0] != 0.0) ? p.scene + (int64_t)sc[RTX_H_MAT0] : nullptr;
  unsigned long long* st = p.stats;

  int d = 0;
  double ar = 0.0, ag = 0.0, ab = 0.0, thr0 = 1.0;
  if (rec) {
    d = rays_through + 1;
    ar = rec[6];
    ag = rec[7];
    ab = rec[8];
    thr0 = rec[9];
    ox0 = rec[0]; oy0 = rec[1]; oz0 = rec[2];
    dx0 = rec[3]; dy0 = rec[4]; dz0 = rec[5];
  }
  const int d0 = d;  // the depth whose finished ray ends the walk
  S.at(d, F_OX) = ox0; S.at(d, F_OY) = oy0; S.at(d, F_OZ) = oz0;
  S.at(d, F_DX) = dx0; S.at(d, F_DY) = dy0; S.at(d, F_DZ) = dz0;
  S.at(d, F_NEXT) = -1.0;
  S.at(d, F_THR) = thr0;
  for (;;) {
    const double ox = S.at(d, F_OX), oy = S.at(d, F_OY), oz = S.at(d, F_OZ);
    const double dx = S.at(d, F_DX), dy = S.at(d, F_DY), dz = S.at(d, F_DZ);
    const double oo = dot3(ox, oy, oz, ox, oy, oz);
    const int next = (int)S.at(d, F_NEXT);
    double tmin;
    int left;   // hits of this ray not yet shaded, this one included
    int h = nsph;  // the shape shaded now (nsph: the ray is done)
    if (next < 0) {  // new ray: nearest distance (base.py:97-98) and its first shape in scene order
      if (st && d < RTX_S_LEVELS && d > rays_through) stat_add(st, RTX_S_RAYS + d, 1);
      tmin = FARAWAY;
      int nh = 0, first = nsph;
      if (d == 0 && h_given >= 0) {  // Shader.create's ray: the level-0 hit is given
        tmin = t_given;
        nh = 1;
        first = h_given;
      } else if (sc[RTX_H_NNODES] != 0.0 && nsph >= kGeneralTreeMin) {
        nearest_count_bvh(sc, ox, oy, oz, oo, dx, dy, dz, tmin, nh, first);
      } else {
        for (int s = 0; s < nsph; ++s) {
          const double t = isect(tab + s * RTX_GEOM_WORDS, ox, oy, oz, oo, dx, dy, dz);
          if (t < tmin) {
            tmin = t;
            nh = 1;
            first = s;
          } else if (t == tmin && t != FARAWAY) {
            ++nh;
          }
        }
      }
      if (st && nh > 1 && d > rays_through) stat_add(st, RTX_S_TIES, 1);
      left = (tmin != FARAWAY || (d == 0 && h_given >= 0)) ? nh : 0;  // (nearest != FARAWAY) & (t == nearest), base.py:102-103
      S.at(d, F_TMIN) = tmin;
      S.at(d, F_LEFT) = (double)left;
      if (left > 0) h = first;
    } else {
      tmin = S.at(d, F_TMIN);
      left = (int)S.at(d, F_LEFT);
      if (left > 0) {  // a tie: the next shape (scene order) with t == nearest
        for (int s = next; s < nsph; ++s) {
          if (isect(tab + s * RTX_GEOM_WORDS, ox, oy, oz, oo, dx, dy, dz) == tmin) {
            h = s;
            break;
          }
        }
      }
    }
    if (h == nsph) {  // this ray is done (its hits' colours are in the sum)
      if (d == d0) {
        cr = ar; cg = ag; cb = ab;
        return;
      }
      --d;  // back to the parent ray: on to its next hit
      S.at(d, F_NEXT) = (double)(key_hit((int)S.at(d, F_KEY)) + 1);
      S.at(d, F_LEFT) = S.at(d, F_LEFT) - 1.0;
      continue;
    }
    if (st && d < RTX_S_LEVELS && d > hits_through) stat_add(st, RTX_S_HITS + d, 1);
    Hit s;
    Work<false> nowk;
    shade<true>(sc, geo, tab, nsph, h, ox, oy, oz, dx, dy, dz, tmin, s, __builtin_nan(""), nowk,
                d == 0 ? mat0 : nullptr);
    const bool weighted = s.lit && s.g != 0.0;
    bool descend = weighted && (B < 0 || d < B);
    if (descend && d + 1 >= p.stack_levels) {  // deeper than the stack: RecursionError on the host
      atomicOr((uint32_t*)p.ws + RTX_WS_STATUS, (uint32_t)RTX_ST_STACK_OVERFLOW);
      descend = false;
    }
    // this hit's colour with a black reflection, weighted (the fast kernels' forward fold)
    const double thr = S.at(d, F_THR);
    double xr, xg, xb;
    hit_color<true>((d == 0 && mat0) ? mat0 : mtab + h * RTX_MAT_WORDS, sc, s.dli, s.di, s.tk, s.lit, weighted,
                    s.spec, s.va, 0.0, 0.0, 0.0, xr, xg, xb);
    ar = __builtin_fma(thr, xr, ar);
    ag = __builtin_fma(thr, xg, ag);
    ab = __builtin_fma(thr, xb, ab);
    if (!descend) {
      S.at(d, F_NEXT) = (double)(h + 1);
      S.at(d, F_LEFT) = (double)(left - 1);
      continue;
    }
    S.at(d, F_KEY) = (double)level_key(h, s.tk);
    double rx = dx, ry = dy, rz = dz;
    reflect_dir(rx, ry, rz, s.nx, s.ny, s.nz);
    ++d;
    S.at(d, F_OX) = s.qx; S.at(d, F_OY) = s.qy; S.at(d, F_OZ) = s.qz;
    S.at(d, F_DX) = rx; S.at(d, F_DY) = ry; S.at(d, F_DZ) = rz;
    S.at(d, F_NEXT) = -1.0;
    S.at(d, F_THR) = (thr * 0.5) * s.g;  // the reflection's weight, (R * 0.5) * g (shader.py:106)
  }
}

__global__ __launch_bounds__(64) void k_render_general(Params p0) {
  const int64_t w = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const Params& p = p0;
  uint32_t* hdr = (uint32_t*)p.ws;
  // Nothing deferred in this launch (the rule for capped renders): every counter is already zero,
  // so there is nothing to render and nothing to reset, and no block touches the done counter
  // (its 64 returning atomics on one address were most of this launch's 5 us).
  if (p.deferred_out && blockIdx.x == 0 && threadIdx.x == 0) *p.deferred_out = hdr[RTX_WS_COUNT];  // before any reset
  if (hdr[RTX_WS_COUNT] == 0u && hdr[RTX_WS_COUNT2] == 0u && hdr[RTX_WS_COUNT3] == 0u) return;
  int64_t count = (int64_t)*p.in_count;
  if (count > p.list_cap) count = p.list_cap;
  const uint64_t* list = p.in_list;
  if (w < p.n_workers) {
    Stack S{p.stack, p.n_workers, w};
    for (int64_t item = w; item < count; item += p.n_workers) {
      const uint64_t e = list[item];
      const int64_t i = (int64_t)(e & ((uint64_t(1) << kFrameShift) - 1));
      const int f = (int)((e >> kFrameShift) & 0xFFFF);
      const int rays_through = (int)((e >> kRaysShift) & kLevelMask) - 1;
      const int hits_through = (int)((e >> kHitsShift) & kLevelMask) - 1;
      // The scene is read through the scalar cache (wave-uniform pointers) while a wave's lanes may
      // hold rays of different frames of a multi-frame launch: lanes sharing the first active
      // lane's frame run together, then the next frame (a waterfall over the wave's frames).
      for (bool todo = true; todo;) {
        const int f0 = __builtin_amdgcn_readfirstlane(f);
        if (f == f0) {
          const Params q = frame_view(p0, f0);
          // a chain deferred for depth (rays and hits counted through the same level) resumes from
          // its record when it has one
          const bool resume = p.in_rec && rays_through == p.in_level && hits_through == rays_through &&
                              item < p.in_rec_cap;
          double ox = 0.0, oy = 0.0, oz = 0.0, dx = 0.0, dy = 0.0, dz = 0.0;
          if (!resume) load_ray(q, i, ox, oy, oz, dx, dy, dz);
          double cr, cg, cb;
          const bool given = q.mode == 3;
          trace_general(q, S, ox, oy, oz, dx, dy, dz, cr, cg, cb, rays_through, hits_through,
                        resume ? p.in_rec + item * kRecWords : nullptr, given ? q.hit_shape : -1,
                        given ? q.hit_t[i] : 0.0);
          write_out(q, i, cr, cg, cb);
          todo = false;
        }
      }
    }
  }
  // leave the workspace clean for the next call: the last block to finish zeroes the counter
  // (every block has read it before arriving; the next kernel on the stream sees the store)
  __syncthreads();
  if (threadIdx.x == 0) {
    if (gridDim.x == 1) {  // one block: no other reader of the counters
      hdr[RTX_WS_COUNT] = 0u;
      hdr[RTX_WS_COUNT2] = 0u;
      hdr[RTX_WS_COUNT3] = 0u;
    } else if (atomicAdd(hdr + RTX_WS_DONE, 1u) == gridDim.x - 1) {
      hdr[RTX_WS_COUNT] = 0u;
      hdr[RTX_WS_COUNT2] = 0u;
      hdr[RTX_WS_COUNT3] = 0u;
      hdr[RTX_WS_DONE] = 0u;
    }
  }
}

// ------------------------------------------------------------------------------------------
// boundary helpers
// ------------------------------------------------------------------------------------------

__global__ __launch_bounds__(kBlock) void k_ray_dirs(Params p, double* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= p.n) return;
  const int lr = (int)(i / p.width), col = (int)(i % p.width);
  double dx, dy, dz;
  camera_dir((const cdouble*)p.scene, col, global_row(p, lr), p.width, p.height, dx, dy, dz);
  out[i] = dx;
  out[p.n + i] = dy;
  out[2 * p.n + i] = dz;
}

__global__ __launch_bounds__(kBlock) void k_intersect(const double* __restrict__ g, const double* __restrict__ org,
                                                      int64_t s, const double* __restrict__ dir, int64_t n,
                                                      double* __restrict__ t) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  const int64_t j = s ? i : 0;
  const double ox = org[j], oy = org[s + j + (s ? 0 : 1)], oz = org[2 * s + j + (s ? 0 : 2)];
  const double dx = dir[i], dy = dir[n + i], dz = dir[2 * n + i];
  t[i] = isect(g, ox, oy, oz, dot3(ox, oy, oz, ox, oy, oz), dx, dy, dz);
}

// bit-exactness check of the sqrt / division fast paths against the compiler's full expansions
__global__ __launch_bounds__(kBlock) void k_selftest_math(const double* __restrict__ a, const double* __restrict__ b,
                                                          int64_t n, double* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  const double x = a[i], y = b[i];
  out[i] = sqrt_cr(x);
  out[n + i] = __builtin_sqrt(x);
  out[2 * n + i] = div_cr(x, y);
  out[3 * n + i] = x / y;
  out[4 * n + i] = inv_mag_unit(x);  // the closed form where every lane of the wave is near 1
  out[5 * n + i] = 1.0 / (x == 0.0 ? 1.0 : __builtin_sqrt(x));
}

// the render kernels' sine (sin_reduced) on a list of phases
__global__ __launch_bounds__(kBlock) void k_sin_reduced(const double* __restrict__ x, int64_t n,
                                                        double* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  out[i] = sin_reduced(x[i]);
}

template <typename T>
__global__ __launch_bounds__(kBlock) void k_quantize(const T* __restrict__ c, int64_t n, uint8_t* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  out[3 * i + 0] = quant_u8((double)c[i]);
  out[3 * i + 1] = quant_u8((double)c[n + i]);
  out[3 * i + 2] = quant_u8((double)c[2 * n + i]);
}

// Supersampling resolve (HipRenderer(samples=k), rtx_resolve_samples): the box filter of a sample
// frame rendered at (k*width) x (k*n_rows) as RTX_OUT_F64_SOA. Per output pixel and channel the
// k*k samples of its block are clipped to [0, 1] (as save_image would have clipped that pixel,
// base.py:147; clip01 sends a NaN to 0 where np.clip keeps it: no sample of a valid scene is NaN),
// added to 0.0 top row first and left to right, and divided once by k*k: the order is the
// contract, so the result is the same for every launch shape.
// A streaming kernel: every sample is read once and every output written once (nontemporal both
// ways), no LDS, no atomics. A lane's k samples of a row are contiguous; for an even k they start
// 16-byte aligned (row and plane starts are multiples of 2 doubles), so VEC loads them as double2.
// K > 0: k at compile time (the loops unroll, all of a pixel's loads are in flight at once);
// K == 0: k at run time.
typedef double f64x2 __attribute__((ext_vector_type(2)));
constexpr int kResolveBlocksPerCu = 8;  // grid cap of k_resolve (blocks per CU), grid-strided beyond it
// One thread per output pixel with its three planes, for every output kind: the u8 output needs a pixel's
// three channels in one lane (its bytes are neighbours), and the mapping already runs at 4.9-5.9 TB/s,
// above a plain streaming read of the sample frame (3.7 TB/s).

template <int K, bool VEC>
__device__ __forceinline__ double resolve_block(const double* __restrict__ s, int64_t row_stride, int k) {
  const int kk = K ? K : k;
  constexpr int kUnroll = K ? K : 1;  // the run-time loops (K == 0) stay rolled
  double acc = 0.0;
#pragma unroll kUnroll
  for (int sy = 0; sy < kk; ++sy) {
    const double* row = s + sy * row_stride;
    if (VEC) {
#pragma unroll kUnroll
      for (int sx = 0; sx < kk; sx += 2) {
        const f64x2 v = __builtin_nontemporal_load((const f64x2*)(row + sx));
        acc = acc + clip01(v.x);
        acc = acc + clip01(v.y);
      }
    } else {
#pragma unroll kUnroll
      for (int sx = 0; sx < kk; ++sx) acc = acc + clip01(__builtin_nontemporal_load(row + sx));
    }
  }
  return acc / (double)(kk * kk);
}

// samples: n_frames x [3][k*n_rows][k*width]; out: n_frames x (width * n_rows pixels as out_kind
// says). k*k*width*n_rows*n_frames < 2^31 (checked by the host), so pixel indices fit 32 bits; the
// word offsets (three planes) are 64-bit.
template <int K, bool VEC>
__global__ __launch_bounds__(kBlock) void k_resolve(const double* __restrict__ samples, int k, unsigned width,
                                                    unsigned n_rows, unsigned n_frames, void* __restrict__ out,
                                                    int out_kind) {
  const int kk = K ? K : k;
  const unsigned n = width * n_rows;                // pixels of a frame
  const int64_t row_stride = (int64_t)kk * width;   // samples of a sample row
  const int64_t ns = row_stride * kk * n_rows;      // samples of a plane
  const int64_t items = (int64_t)n * n_frames;
  for (int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x; t < items; t += (int64_t)gridDim.x * kBlock) {
    const unsigned px = (unsigned)t;  // frame-major pixel index
    const unsigned f = px / n, i = px - f * n;
    const unsigned r = i / width, c = i - r * width;
    const double* s = samples + (int64_t)f * 3 * ns + (int64_t)r * kk * row_stride + (int64_t)c * kk;
    const double cr = resolve_block<K, VEC>(s, row_stride, k);
    const double cg = resolve_block<K, VEC>(s + ns, row_stride, k);
    const double cb = resolve_block<K, VEC>(s + 2 * ns, row_stride, k);
    if (out_kind == RTX_OUT_F32_SOA) {
      float* o = (float*)out + (int64_t)f * 3 * n + i;
      __builtin_nontemporal_store((float)cr, o);
      __builtin_nontemporal_store((float)cg, o + n);
      __builtin_nontemporal_store((float)cb, o + 2 * (int64_t)n);
    } else if (out_kind == RTX_OUT_F64_SOA) {
      double* o = (double*)out + (int64_t)f * 3 * n + i;
      __builtin_nontemporal_store(cr, o);
      __builtin_nontemporal_store(cg, o + n);
      __builtin_nontemporal_store(cb, o + 2 * (int64_t)n);
    } else {
      unsigned char* o = (unsigned char*)out + 3 * (int64_t)px;
      o[0] = quant_u8(cr);
      o[1] = quant_u8(cg);
      o[2] = quant_u8(cb);
    }
  }
}

// Un-permute of gathered row tiles (the multi-GPU frame, application.render_frame_distributed):
// rank r's buffer (at tiles + r * part_stride) holds the rows of its run of parts in local order, as
// rtx_render_camera_sched wrote them, [planes][rows_r][row_bytes]; the frame is
// [planes][height][row_bytes]. One block per (frame row, plane): a contiguous row copy, 16 B per
// lane when the row and buffers allow it.
__global__ __launch_bounds__(kBlock) void k_assemble_rows(const uint8_t* __restrict__ tiles, int64_t part_stride,
                                                          int n_parts, int root_run, int run, int height,
                                                          int row_block, int64_t row_bytes, bool vec16,
                                                          uint8_t* __restrict__ out) {
  const int g = blockIdx.x;  // frame row
  const int c = blockIdx.y;  // plane
  const int cyc = n_parts * row_block;
  const int pos = g % cyc;
  int r, first, len;
  run_owner(pos / row_block, root_run, run, r, first, len);
  const int lr = (g / cyc) * len * row_block + pos - first * row_block;
  const int rows_r = tile_local_rows(height, row_block, n_parts, first, len);
  const uint8_t* src = tiles + r * part_stride + ((int64_t)c * rows_r + lr) * row_bytes;
  uint8_t* dst = out + ((int64_t)c * height + g) * row_bytes;
  if (vec16) {
    typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
    const u32x4* s4 = (const u32x4*)src;
    u32x4* d4 = (u32x4*)dst;
    for (int64_t k = threadIdx.x; k < row_bytes / 16; k += kBlock) __builtin_nontemporal_store(s4[k], d4 + k);
  } else {
    for (int64_t k = threadIdx.x; k < row_bytes; k += kBlock) dst[k] = src[k];
  }
}

}  // namespace

// ------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------

static thread_local char g_err[512] = "";  // rtx_last_error: the message of every unit's failures

int rtx_fail(int code, const char* fmt, ...) {
  va_list args;
  va_start(args, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, args);
  va_end(args);
  return code;
}

namespace {

thread_local hipError_t g_small_err = hipSuccess;  // a launch rtx_launch_small refused

int check_launch(const char* what) {
  const hipError_t refused = g_small_err;
  g_small_err = hipSuccess;
  return rtx_launched(what, refused);
}

// Optional live timing of the dominant kernel (bench.py's roofline): a pool of event pairs handed to
// the k_render_fast launch itself (hipExtLaunchKernelGGL), so they time the dispatch from its start
// to its end, as rocprofv3's kernel trace does, without the gap an event recorded before it adds.
// The state belongs to the calling thread: render calls from other threads are never timed by it
// and never touch it (the entry points stay re-entrant).
struct Prof {
  int cap = 0;
  int used = 0;
  hipEvent_t* ev = nullptr;  // 2 * cap
  int every = 1;             // record one launch in `every` (rtx_profile_sample)
  long long seen = 0;        // launches since rtx_profile_enable
  bool on = false;           // the current launch is recorded
};
thread_local Prof g_prof;

void prof_free() {
  for (int i = 0; i < 2 * g_prof.cap; ++i) (void)hipEventDestroy(g_prof.ev[i]);
  delete[] g_prof.ev;
  const int every = g_prof.every;
  g_prof = Prof{};
  g_prof.every = every;
}

inline void prof_mark(int which, hipStream_t) {
  // launches every-1, 2*every-1, ...: not the first one after rtx_profile_enable, which follows an
  // idle GPU in bench.py (barrier + synchronize) and runs a few µs slow
  if (which == 0)
    g_prof.on = g_prof.cap && g_prof.used < g_prof.cap && g_prof.seen++ % g_prof.every == g_prof.every - 1;
}
// the start / stop event of the launch being timed (null: not timed)
inline hipEvent_t prof_event(int which) { return g_prof.on ? g_prof.ev[2 * g_prof.used + which] : nullptr; }
inline void prof_next() {
  if (g_prof.on) ++g_prof.used;
  g_prof.on = false;
}

// rtx_last_launches: the calling thread's latest render call (cleared on its entry; a render call
// launches k_render_fast once, an uncapped one twice with its continuation pass)
struct LaunchLog {
  int n = 0;        // k_render_fast launches
  int general = 0;  // k_render_general was launched
  int rec[RTX_LAUNCH_MAX][RTX_LAUNCH_WORDS];
};
thread_local LaunchLog g_launches;
inline void launches_clear() { g_launches.n = g_launches.general = 0; }

int device_cus() {  // compute units of the current device (cached per device)
  static int cus[64] = {0};
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 256;
  if (cus[dev] == 0) {
    int v = 0;
    if (hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || v <= 0) v = 256;
    cus[dev] = v;
  }
  return cus[dev];
}

int stack_levels_for(int max_bounces) {
  return max_bounces < 0 ? RTX_UNBOUNDED_LEVELS : max_bounces + 1;
}

constexpr size_t kStackBudget = size_t(512) << 20;  // general-kernel frame stacks: <= 512 MiB
constexpr int64_t kMaxWorkers = 65536;

int64_t workers_for(int64_t n, int max_bounces) {
  const size_t per = (size_t)stack_levels_for(max_bounces) * kFrameWords * sizeof(double);
  int64_t w = (int64_t)(kStackBudget / per);
  if (w > kMaxWorkers) w = kMaxWorkers;
  const bool capped = max_bounces >= 0 && max_bounces <= kCappedMax;
  const int64_t cap = capped ? kDeferredWorkers : kDeepWorkers;
  if (w > cap) w = cap;
  const int64_t need = ((n + 63) / 64) * 64;
  if (w > need) w = need;
  w = (w / 64) * 64;
  return w < 64 ? 64 : w;
}

size_t list_bytes(int64_t n) { return (size_t)n * sizeof(int64_t); }

// resume records of the first pass or (cont) the continuation pass: only when chains are deferred for depth
int64_t records_for(int64_t n, int max_bounces, bool cont = false) {
  const bool capped = max_bounces >= 0 && max_bounces <= kCappedMax;
  return capped ? 0 : records_cap(n, cont);
}

size_t round256(size_t b) { return (b + 255) / 256 * 256; }

// Workspace: header | tile counters | list 1 | (deep chains:) the continuation pass's list | the
// first pass's records | the continuation pass's records | general-kernel stacks
struct WsLayout {
  size_t fetch, list1, cont_list, rec1, cont_rec, stack, total;
};
WsLayout ws_layout(int64_t n, int max_bounces) {
  WsLayout w{};
  const int64_t nrec = records_for(n, max_bounces);
  const int64_t ncont = records_for(n, max_bounces, true);
  w.fetch = RTX_WS_HDR_BYTES;
  w.list1 = w.fetch + (size_t)kMaxFetch * kFetchStride * sizeof(uint32_t);
  w.cont_list = w.list1 + round256(list_bytes(n));
  w.rec1 = w.cont_list + (nrec ? round256(list_bytes(n)) : 0);
  w.cont_rec = w.rec1 + round256((size_t)nrec * kRecWords * sizeof(double));
  w.stack = w.cont_rec + round256((size_t)ncont * kRecWords * sizeof(double));
  w.total = w.stack + (size_t)workers_for(n, max_bounces) * stack_levels_for(max_bounces) * kFrameWords * 8;
  return w;
}

size_t ws_bytes(int64_t n, int max_bounces) { return ws_layout(n, max_bounces).total; }
static_assert(RTX_WS_COUNTER_BYTES == RTX_WS_HDR_BYTES + kMaxFetch * kFetchStride * sizeof(uint32_t),
              "RTX_WS_COUNTER_BYTES: the header and the tile-fetch counters (ws_layout().list1)");

// The block-tile grid of a camera launch that is not persistent: the TREE = false kernels (scenes below
// kTreeMinSpheres, launch_fast_lds) use wave_w<false>() pixels per wave row.
void block_grid(int nsph, int width, int n_rows, int64_t& gx, int64_t& gy) {
  const bool small = nsph < kTreeMinSpheres;
  const int wx = small ? waves_x<false>() : waves_x<true>();
  const int tw = wx * (small ? wave_w<false>() : wave_w<true>());
  const int th = ((small ? fast_waves<false>() : fast_waves<true>()) / wx) * (64 / (small ? wave_w<false>() : wave_w<true>()));
  gx = (width + tw - 1) / tw;
  gy = (n_rows + th - 1) / th;
}

// Persistent launch (p.n_fetch > 0 on entry): as many blocks as the device holds at once, at most one
// wave per tile; sets n_fetch to the counters in use (every counter needs at least one wave).
template <typename K>
dim3 persistent_grid(K kernel, size_t lds, Params& p) {
  int per_cu = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, kFastBlock, lds) != hipSuccess || per_cu < 1)
    per_cu = 1;
  const int64_t nt = (int64_t)p.n_tiles_x * p.n_tiles_y;
  int64_t blocks = (int64_t)per_cu * device_cus() - p.reserve;  // (room for a concurrent collective)
  if (blocks < 8) blocks = 8;
  const int64_t need = (nt + kFastWaves - 1) / kFastWaves;
  if (blocks > need) blocks = need;
  if (blocks >= 8) blocks -= blocks % 8;  // whole XCD groups (the kernel numbers waves XCD-major)
  const int64_t per_xcd = blocks * kFastWaves / (blocks % 8 == 0 ? 8 : 1);
  int nc = kMaxFetch;  // a power of two dividing the waves per XCD
  while (nc > 1 && per_xcd % nc != 0) nc /= 2;
  p.n_fetch = nc;
  if (getenv("RTX_DEBUG_GRID"))
    fprintf(stderr, "persistent grid: %d blocks/CU x %d CUs -> %lld blocks, %d counters, %lld tiles\n", per_cu,
            device_cus(), (long long)blocks, p.n_fetch, (long long)nt);
  return dim3((unsigned)blocks);
}

// One k_render_fast launch of this unit and its launch record: the template arguments (defaults as
// the kernel's) are named once, so the record tells the instantiation that ran.
template <int B, bool LDS, int DEEP, bool STATS = false, int TP = 2, bool IMG = false, int NSPH = 0, int WAVES = 0>
void launch_k(const Params& p, dim3 grid, uint32_t lds, hipStream_t s) {
  rtx_note_launch(B, LDS, DEEP, STATS, TP, IMG, NSPH, WAVES, grid, p.n_fetch, p.tile_order != nullptr, lds);
  hipExtLaunchKernelGGL((k_render_fast<B, LDS, DEEP, STATS, TP, IMG, NSPH, WAVES>), grid, dim3(kFastBlock), lds, s,
                        prof_event(0), prof_event(1), 0u, p);
}

// STATS: the instantiation with the per-level and executed-work counters (stats buffer given) and
// the per-unit cost records (tile_cost given; counters only where p.stats is set).
// Launches that are not persistent run instantiations without the persistent tile loop (TP 1), and
// scenes below kTreeMinSpheres, which carry no culling tree (scene_pack.BVH_MIN_SPHERES), ones
// without the tree walks either (TP 0) (A/B in DESIGN.md §4).
template <int B, int DEEP, bool STATS, bool IMG = false>
void launch_fast_lds(Params& p, dim3 grid, hipStream_t s) {
  const bool small = p.nsph < kTreeMinSpheres;  // the TREE = false kernels: fast_block<false>() threads
  const size_t lds = (size_t)p.nsph * kSphWords * sizeof(double) +
                     (!DEEP && !small && p.n_fetch == 0 ? kColourLdsBytes : 0);  // TP 1
  if (p.n_fetch == 0) {  // one tile per block: the instantiations without the persistent loop
    if (p.nsph < kTreeMinSpheres) {  // TP 0: the rtx_small.hip unit
      const hipError_t e =
          rtx_launch_small(B, DEEP, STATS, IMG, &p, grid, (uint32_t)lds, s, prof_event(0), prof_event(1));
      if (e != hipSuccess) g_small_err = e;
    } else {
      if constexpr (!DEEP && !STATS && !IMG) {
        if ((int64_t)p.n * p.n_frames >= kWavesLargeMinPixels) {  // a large launch: more waves (kFwdWavesLarge)
          launch_k<B, true, DEEP, STATS, 1, IMG, 0, kFwdWavesLarge>(p, grid, (uint32_t)lds, s);
          return;
        }
      }
      launch_k<B, true, DEEP, STATS, 1, IMG>(p, grid, (uint32_t)lds, s);
    }
    return;
  }
  if (p.n_fetch > 0) grid = persistent_grid(k_render_fast<B, true, DEEP, STATS, 2, IMG>, lds, p);
  launch_k<B, true, DEEP, STATS, 2, IMG>(p, grid, (uint32_t)lds, s);
}

template <int B, int DEEP = 0>
void launch_fast_b(const Params& p0, dim3 grid, hipStream_t s) {
  Params p = p0;
  if (p.nsph <= kLdsMaxSpheres) {
    if (p.stats || p.tile_cost) {  // (the cost records of a learning launch live in the STATS kernels)
      launch_fast_lds<B, DEEP, true>(p, grid, s);
    } else if (!DEEP && p.images) {  // image textures shaded in place (capped renders only)
      launch_fast_lds<B, DEEP, false, !DEEP>(p, grid, s);
    } else {
      launch_fast_lds<B, DEEP, false>(p, grid, s);
    }
  } else {
    if (p.stats || p.tile_cost) {
      if (p.n_fetch > 0) grid = persistent_grid(k_render_fast<B, false, DEEP, true>, 0, p);
      launch_k<B, false, DEEP, true>(p, grid, 0u, s);
    } else {
      if (p.n_fetch > 0) grid = persistent_grid(k_render_fast<B, false, DEEP>, 0, p);
      launch_k<B, false, DEEP>(p, grid, 0u, s);
    }
  }
}

// caps above kCappedMax or none: kDeepLevels levels, longer chains deferred with a record
void launch_fast_deep(const Params& p, dim3 grid, hipStream_t s) { launch_fast_b<kDeepLevels, 1>(p, grid, s); }
// ... and their continuation pass (mode 2)
void launch_fast_cont(const Params& p, dim3 grid, hipStream_t s) { launch_fast_b<kDeepLevels, 2>(p, grid, s); }

void launch_fast(int B, const Params& p, dim3 grid, hipStream_t s) {
  switch (B) {
    case 0: launch_fast_b<0>(p, grid, s); break;
    case 1: launch_fast_b<1>(p, grid, s); break;
    case 2: launch_fast_b<2>(p, grid, s); break;
    case 3: launch_fast_b<3>(p, grid, s); break;
    case 4: launch_fast_b<4>(p, grid, s); break;
    case 5: launch_fast_b<5>(p, grid, s); break;
    default: launch_fast_b<6>(p, grid, s); break;
  }
}
static_assert(RTX_FAST_MAX_BOUNCES == 6, "launch_fast switch covers 0..6");

// what a render call adds to its launch's camera_params / ray_params
void render_target(Params& p, int max_bounces, void* out, int out_kind, uint64_t* stats) {
  p.max_bounces = max_bounces;
  p.out = out;
  p.out_kind = out_kind;
  p.stats = (unsigned long long*)stats;
}

// no_general: the caller knows this exact render defers no ray (rtx_render_camera_ex): no general
// kernel, and for an uncapped render no continuation pass either
int run_render(Params& p, void* workspace, size_t workspace_bytes, hipStream_t s, bool no_general = false) {
  if (p.nsph <= 0 || p.nsph > RTX_MAX_SPHERES) return rtx_fail(RTX_E_ARG, "n_spheres out of range (%d)", p.nsph);
  if (!p.scene || !workspace) return rtx_fail(RTX_E_ARG, "null pointer argument");
  if (p.out_kind < 0 || p.out_kind > 2) return rtx_fail(RTX_E_ARG, "bad out_kind %d", p.out_kind);
  if (p.max_bounces < RTX_UNBOUNDED) return rtx_fail(RTX_E_ARG, "bad max_bounces %d", p.max_bounces);
  if (p.n_frames <= 0) p.n_frames = 1;
  if (p.n_frames > 65535) return rtx_fail(RTX_E_ARG, "at most 65535 frames per launch (%d)", p.n_frames);
  if (p.n <= 0) return RTX_OK;  // (an empty tile, e.g. a rank's share of a small frame: out may be null)
  if (!p.out) return rtx_fail(RTX_E_ARG, "null pointer argument");
  if (p.n >= (int64_t(1) << kFrameShift))
    return rtx_fail(RTX_E_ARG, "too many pixels per frame (%lld)", (long long)p.n);
  const int64_t n_all = p.n * p.n_frames;  // pixels of the whole launch
  const size_t need = ws_bytes(n_all, p.max_bounces);
  if (workspace_bytes < need)
    return rtx_fail(RTX_E_WORKSPACE, "workspace too small (need %lld bytes)", (long long)need);
  p.ws = (uint8_t*)workspace;
  p.list_cap = n_all;
  const WsLayout lay = ws_layout(n_all, p.max_bounces);
  uint32_t* const hdr = (uint32_t*)p.ws;
  uint64_t* const list1 = (uint64_t*)(p.ws + lay.list1);
  double* const rec1 = (double*)(p.ws + lay.rec1);
  p.rec_cap = records_for(n_all, p.max_bounces);
  p.in_rec_cap = p.rec_cap;
  p.stack = (double*)(p.ws + lay.stack);
  // The fast kernel renders every ray up to min(cap, RTX_FAST_MAX_BOUNCES) levels; a pixel whose
  // chain outlives that (a larger or no cap) is deferred, like a tie, to the general kernel.
  const bool capped = p.max_bounces >= 0 && p.max_bounces <= kCappedMax;
  p.no_general = no_general ? 1 : 0;
  p.n_workers = workers_for(n_all, p.max_bounces);
  p.stack_levels = stack_levels_for(p.max_bounces);
  {
    dim3 grid;
    const int64_t fb = p.nsph < kTreeMinSpheres ? fast_block<false>() : fast_block<true>();
    int64_t tx = (p.n + fb - 1) / fb, ty = 1;
    if (p.mode == 0) block_grid(p.nsph, p.width, p.n_rows, tx, ty);
    p.n_fetch = 0;
    if (p.nsph >= kPersistMinSpheres && p.mode == 0 && p.n_frames == 1) {
      p.n_tiles_x = (p.width + kWaveW - 1) / kWaveW;  // wave tiles
      p.n_tiles_y = (p.n_rows + kWaveH - 1) / kWaveH;
      p.fetch = (uint32_t*)(p.ws + lay.fetch);
      p.n_fetch = kMaxFetch;  // launch_fast_b sizes the grid and the counters in use
      grid = dim3(1);
    } else {
      p.n_tiles_x = p.n_tiles_y = 0;
      grid = dim3((unsigned)tx, (unsigned)ty, (unsigned)p.n_frames);
    }
    p.dlist = list1;
    p.dcount = hdr + RTX_WS_COUNT;
    p.drec = capped ? nullptr : rec1;
    p.drec_level = kFirstPassLevels;
    prof_mark(0, s);
    if (capped) {
      launch_fast(p.max_bounces, p, grid, s);
    } else {
      launch_fast_deep(p, grid, s);
    }
    prof_mark(1, s);
    prof_next();
    if (int e = check_launch("k_render_fast")) return e;
  }
  p.in_list = list1;
  p.in_count = hdr + RTX_WS_COUNT;
  p.in_rec = capped ? nullptr : rec1;
  p.in_level = kFirstPassLevels;
  if (!capped && p.n_frames == 1 && !no_general) {
    // the continuation pass: chains deferred for depth go on from level kFirstPassLevels + 1 to
    // kDeepLevel3 in the register-resident kernel; ties and what is still alive after it go to the
    // general kernel
    Params q = p;
    q.mode = 2;
    q.n_tiles_x = q.n_tiles_y = 0;
    q.n_fetch = 0;
    q.dlist = (uint64_t*)(p.ws + lay.cont_list);
    q.dcount = hdr + RTX_WS_COUNT3;
    q.drec = (double*)(p.ws + lay.cont_rec);
    q.drec_level = kDeepLevel3;
    q.rec_cap = records_for(n_all, p.max_bounces, true);
    const int64_t fb = p.nsph < kTreeMinSpheres ? fast_block<false>() : fast_block<true>();
    const int64_t tiles = (n_all + fb - 1) / fb;
    const int64_t cap = 4 * (int64_t)device_cus();
    launch_fast_cont(q, dim3((unsigned)(tiles < cap ? tiles : cap)), s);
    if (int e = check_launch("k_render_fast (continuation)")) return e;
    p.in_list = q.dlist;
    p.in_count = q.dcount;
    p.in_rec = q.drec;
    p.in_level = q.drec_level;
    p.in_rec_cap = q.rec_cap;
  }
  // deferred rays: ties, and chains longer than the fast kernel's levels
  if (no_general) return RTX_OK;  // (an uncapped render: nor the continuation pass)
  g_launches.general = 1;
  hipLaunchKernelGGL(k_render_general, dim3((unsigned)(p.n_workers / 64)), dim3(64), 0, s, p);
  return check_launch("k_render_general");
}

}  // namespace

void rtx_note_launch(int B, int lds, int deep, int stats, int tp, int img, int nsph, int waves, dim3 grid, int n_fetch,
                     int ordered, uint32_t lds_bytes) {
  if (g_launches.n < RTX_LAUNCH_MAX) {
    const int v[RTX_LAUNCH_WORDS] = {B, lds, deep, stats, tp, img, nsph, waves, (int)grid.x, (int)grid.y, (int)grid.z,
                                     n_fetch, ordered, (int)lds_bytes};
    for (int k = 0; k < RTX_LAUNCH_WORDS; ++k) g_launches.rec[g_launches.n][k] = v[k];
  }
  ++g_launches.n;
}

// ------------------------------------------------------------------------------------------
// C ABI
// ------------------------------------------------------------------------------------------

extern "C" {

int rtx_abi_version(int* layout, int n) {
  const int v[] = {RTX_HDR_WORDS, RTX_GEOM_WORDS, RTX_MAT_WORDS, RTX_MAX_DOMES, RTX_S_WORDS, RTX_WS_HDR_BYTES,
                   RTX_FAST_MAX_BOUNCES, RTX_UNBOUNDED_LEVELS};
  for (int i = 0; layout && i < n && i < (int)(sizeof(v) / sizeof(v[0])); ++i) layout[i] = v[i];
  return RTX_ABI_VERSION;
}

const char* rtx_last_error(void) { return g_err; }

int rtx_profile_enable(int max_launches) {
  prof_free();
  if (max_launches <= 0) return RTX_OK;
  g_prof.ev = new hipEvent_t[2 * (size_t)max_launches];
  // timing-only events: no system-scope fence when they are recorded (the default fence writes back
  // and invalidates the caches around the timed dispatch, which lengthened the timed launches by
  // ~0.6 us and read ~0.8 us more on C2, session r6s; the HIP header recommends the flag for
  // events used only to measure time)
  for (int i = 0; i < 2 * max_launches; ++i) {
    if (hipEventCreateWithFlags(&g_prof.ev[i], hipEventDisableSystemFence) != hipSuccess) {
      g_prof.cap = i / 2;
      prof_free();
      return rtx_fail(RTX_E_LAUNCH, "hipEventCreate failed");
    }
  }
  g_prof.cap = max_launches;
  return RTX_OK;
}

int rtx_profile_sample(int every) {
  if (every < 1) return rtx_fail(RTX_E_ARG, "profile sampling stride must be >= 1 (%d)", every);
  g_prof.every = every;
  return RTX_OK;
}

int rtx_profile_collect(double* total_ms, int* n_launches) {
  double tot = 0.0;
  for (int i = 0; i < g_prof.used; ++i) {
    if (hipEventSynchronize(g_prof.ev[2 * i + 1]) != hipSuccess) return check_launch("hipEventSynchronize");
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, g_prof.ev[2 * i], g_prof.ev[2 * i + 1]) != hipSuccess)
      return check_launch("hipEventElapsedTime");
    tot += ms;
  }
  if (total_ms) *total_ms = tot;
  if (n_launches) *n_launches = g_prof.used;
  g_prof.used = 0;
  return RTX_OK;
}

size_t rtx_workspace_bytes(int64_t n_rays, int max_bounces) {
  if (n_rays < 1) n_rays = 1;
  if (max_bounces < RTX_UNBOUNDED) max_bounces = RTX_UNBOUNDED;
  return ws_bytes(n_rays, max_bounces);
}

int rtx_sched_tiles(int width, int n_local_rows, int n_spheres, int64_t* n_tiles) {
  if (!n_tiles) return rtx_fail(RTX_E_ARG, "null pointer argument");
  *n_tiles = 0;
  if (width <= 0 || n_local_rows <= 0 || n_spheres <= 0) return RTX_OK;
  if (n_spheres >= kPersistMinSpheres) {  // persistent launch: wave tiles
    *n_tiles = (int64_t)((width + kWaveW - 1) / kWaveW) * ((n_local_rows + kWaveH - 1) / kWaveH);
    return RTX_OK;
  }
  int64_t gx, gy;  // one block tile per block (run_render's grid)
  block_grid(n_spheres, width, n_local_rows, gx, gy);
  *n_tiles = gx * gy;
  return RTX_OK;
}

int rtx_render_camera_ex(const double* scene, int n_spheres, int width, int height, int row_block, int n_parts,
                         int part, int n_local_rows, int max_bounces, void* out, int out_kind, void* workspace,
                         size_t workspace_bytes, uint64_t* stats, void* stream, unsigned flags,
                         uint32_t* deferred_out) {
  return rtx_render_camera_sched(scene, n_spheres, width, height, row_block, n_parts, part, 1, n_local_rows,
                                 max_bounces, out, out_kind, workspace, workspace_bytes, stats, stream, flags,
                                 deferred_out, nullptr, nullptr);
}

int rtx_render_camera_sched(const double* scene, int n_spheres, int width, int height, int row_block, int n_parts,
                            int part, int part_run, int n_local_rows, int max_bounces, void* out, int out_kind,
                            void* workspace,
                            size_t workspace_bytes, uint64_t* stats, void* stream, unsigned flags,
                            uint32_t* deferred_out, const uint32_t* tile_order, uint32_t* tile_cost) {
  launches_clear();
  if (!tile_geometry_ok(width, height, row_block, n_parts, part, part_run, n_local_rows))
    return rtx_fail(RTX_E_ARG, "bad frame/tile geometry");
  if (flags & ~(unsigned)(RTX_F_NO_GENERAL | RTX_F_IMAGES | RTX_F_RESERVE(0xFFF)))
    return rtx_fail(RTX_E_ARG, "unknown flags (%lld)", (long long)flags);
  Params p{};
  camera_params(p, scene, n_spheres, width, height, row_block, n_parts, part, part_run, n_local_rows);
  render_target(p, max_bounces, out, out_kind, stats);
  p.images = (flags & RTX_F_IMAGES) ? 1 : 0;
  p.deferred_out = deferred_out;
  p.tile_order = tile_order;  // rtx_sched_tiles units of this launch (the first pass: mode 0, one frame)
  p.tile_cost = tile_cost;
  p.reserve = (int)((flags >> RTX_F_RESERVE_SHIFT) & 0xFFFu);
  // a launch with counters or cost records runs the STATS kernels, which have no texturing build:
  // they defer image-textured hits, so the general kernel must follow whatever the caller learnt
  // from the texturing build's deferral count
  const bool no_general = (flags & RTX_F_NO_GENERAL) && !(p.images && (stats || tile_cost));
  return run_render(p, workspace, workspace_bytes, (hipStream_t)stream, no_general);
}

int rtx_render_camera(const double* scene, int n_spheres, int width, int height, int row_block, int n_parts,
                      int part, int n_local_rows, int max_bounces, void* out, int out_kind, void* workspace,
                      size_t workspace_bytes, uint64_t* stats, void* stream) {
  return rtx_render_camera_ex(scene, n_spheres, width, height, row_block, n_parts, part, n_local_rows, max_bounces,
                              out, out_kind, workspace, workspace_bytes, stats, stream, 0u, nullptr);
}

int rtx_render_frames(const double* scenes, int64_t scene_stride, int n_frames, int n_spheres, int width, int height,
                      int max_bounces, void* out, int out_kind, void* workspace, size_t workspace_bytes,
                      uint64_t* stats, void* stream) {
  launches_clear();
  if (width <= 0 || height <= 0) return rtx_fail(RTX_E_ARG, "bad frame geometry");
  if (n_frames < 0) return rtx_fail(RTX_E_ARG, "bad n_frames (%d)", n_frames);
  if (n_frames > 1 && scene_stride < RTX_HDR_WORDS)
    return rtx_fail(RTX_E_ARG, "bad scene_stride (%lld)", (long long)scene_stride);
  if (n_frames == 0) return RTX_OK;
  Params p{};
  camera_params(p, scenes, n_spheres, width, height, 1, 1, 0, 1, height);  // whole frames
  render_target(p, max_bounces, out, out_kind, stats);
  p.scene_stride = scene_stride;
  p.n_frames = n_frames;
  return run_render(p, workspace, workspace_bytes, (hipStream_t)stream);
}

int rtx_trace_rays(const double* scene, int n_spheres, const double* origins, int64_t origin_stride,
                   const double* dirs, int64_t n, int max_bounces, void* out, int out_kind, void* workspace,
                   size_t workspace_bytes, uint64_t* stats, void* stream) {
  launches_clear();
  if (!origins || !dirs) return rtx_fail(RTX_E_ARG, "null ray pointer");
  if (origin_stride != 0 && origin_stride != n) return rtx_fail(RTX_E_ARG, "origin_stride must be 0 or n");
  Params p{};
  ray_params(p, scene, n_spheres, 1, origins, origin_stride, dirs, n);
  render_target(p, max_bounces, out, out_kind, stats);
  return run_render(p, workspace, workspace_bytes, (hipStream_t)stream);
}

int rtx_shade_hits(const double* scene, int n_spheres, int shape, const double* origins, int64_t origin_stride,
                   const double* dirs, const double* t, int64_t n, int max_bounces, void* out, int out_kind,
                   void* workspace, size_t workspace_bytes, uint64_t* stats, void* stream) {
  launches_clear();
  if (!origins || !dirs || !t) return rtx_fail(RTX_E_ARG, "null ray pointer");
  if (origin_stride != 0 && origin_stride != n) return rtx_fail(RTX_E_ARG, "origin_stride must be 0 or n");
  if (shape < 0 || shape >= n_spheres) return rtx_fail(RTX_E_ARG, "shape index out of range (%d)", shape);
  Params p{};
  ray_params(p, scene, n_spheres, 3, origins, origin_stride, dirs, n);
  render_target(p, max_bounces, out, out_kind, stats);
  p.hit_t = t;
  p.hit_shape = shape;
  return run_render(p, workspace, workspace_bytes, (hipStream_t)stream);
}

int rtx_ray_directions(const double* scene, int width, int height, int row_block, int n_parts, int part,
                       int n_local_rows, double* dirs_out, void* stream) {
  if (!scene || !dirs_out) return rtx_fail(RTX_E_ARG, "null pointer argument");
  if (!tile_geometry_ok(width, height, row_block, n_parts, part, 1, n_local_rows))
    return rtx_fail(RTX_E_ARG, "bad frame/tile geometry");
  Params p{};
  camera_params(p, scene, 0, width, height, row_block, n_parts, part, 1, n_local_rows);
  if (p.n == 0) return RTX_OK;
  hipLaunchKernelGGL(k_ray_dirs, dim3((unsigned)((p.n + kBlock - 1) / kBlock)), dim3(kBlock), 0,
                     (hipStream_t)stream, p, dirs_out);
  return check_launch("k_ray_dirs");
}

int rtx_sphere_intersect(const double* sphere, const double* origins, int64_t origin_stride, const double* dirs,
                         int64_t n, double* t_out, void* stream) {
  if (!sphere || !origins || !dirs || !t_out) return rtx_fail(RTX_E_ARG, "null pointer argument");
  if (origin_stride != 0 && origin_stride != n) return rtx_fail(RTX_E_ARG, "origin_stride must be 0 or n");
  if (n <= 0) return RTX_OK;
  hipLaunchKernelGGL(k_intersect, dim3((unsigned)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, (hipStream_t)stream,
                     sphere, origins, origin_stride, dirs, n, t_out);
  return check_launch("k_intersect");
}

int rtx_last_launches(int* records, int max_records, int* general_out) {
  if (max_records < 0 || (max_records > 0 && !records))
    return rtx_fail(RTX_E_ARG, "rtx_last_launches: null records or a negative count (%d)", max_records);
  const int have = g_launches.n < RTX_LAUNCH_MAX ? g_launches.n : RTX_LAUNCH_MAX;
  for (int i = 0; i < have && i < max_records; ++i)
    for (int k = 0; k < RTX_LAUNCH_WORDS; ++k) records[i * RTX_LAUNCH_WORDS + k] = g_launches.rec[i][k];
  if (general_out) *general_out = g_launches.general;
  return g_launches.n;
}

int rtx_selftest_math(const double* a, const double* b, int64_t n, double* out, void* stream) {
  if (!a || !b || !out) return rtx_fail(RTX_E_ARG, "null pointer argument");
  if (n <= 0) return RTX_OK;
  hipLaunchKernelGGL(k_selftest_math, dim3((unsigned)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0,
                     (hipStream_t)stream, a, b, n, out);
  return check_launch("k_selftest_math");
}

int rtx_selftest_sin(const double* x, int64_t n, double* out, void* stream) {
  if (!x || !out) return rtx_fail(RTX_E_ARG, "null pointer argument");
  if (n <= 0) return RTX_OK;
  hipLaunchKernelGGL(k_sin_reduced, dim3((unsigned)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, (hipStream_t)stream,
                     x, n, out);
  return check_launch("k_sin_reduced");
}

int rtx_quantize_u8(const void* color, int color_kind, int64_t n, uint8_t* out, void* stream) {
  if (!color || !out) return rtx_fail(RTX_E_ARG, "null pointer argument");
  if (n <= 0) return RTX_OK;
  const dim3 grid((unsigned)((n + kBlock - 1) / kBlock));
  if (color_kind == RTX_OUT_F32_SOA) {
    hipLaunchKernelGGL(k_quantize<float>, grid, dim3(kBlock), 0, (hipStream_t)stream, (const float*)color, n, out);
  } else if (color_kind == RTX_OUT_F64_SOA) {
    hipLaunchKernelGGL(k_quantize<double>, grid, dim3(kBlock), 0, (hipStream_t)stream, (const double*)color, n, out);
  } else {
    return rtx_fail(RTX_E_ARG, "bad color_kind %d", color_kind);
  }
  return check_launch("k_quantize");
}

int rtx_resolve_samples(const double* samples, int k, int width, int n_rows, int n_frames, void* out, int out_kind,
                        void* stream) {
  if (!samples || !out) return rtx_fail(RTX_E_ARG, "null pointer argument");
  if (k < 1 || k > 8) return rtx_fail(RTX_E_ARG, "samples per pixel side must be in 1..8, got %d", k);
  if (width <= 0 || n_rows <= 0 || n_frames <= 0) return rtx_fail(RTX_E_ARG, "bad frame geometry");
  if (out_kind != RTX_OUT_F32_SOA && out_kind != RTX_OUT_F64_SOA && out_kind != RTX_OUT_U8_HWC)
    return rtx_fail(RTX_E_ARG, "bad out_kind %d", out_kind);
  // k*k*width*n_rows*n_frames < 2^31, without overflowing on the way (nested floor divisions are exact)
  int64_t room = (((int64_t)1 << 31) - 1) / (k * k);
  const bool fits = width <= room && n_rows <= (room /= width) && n_frames <= (room /= n_rows);
  if (!fits) return rtx_fail(RTX_E_ARG, "k*k*width*n_rows*n_frames must stay below 2^31 samples per plane");
  const bool vec = k % 2 == 0 && (uintptr_t)samples % 16 == 0;
  const int64_t items = (int64_t)width * n_rows * n_frames;
  const int64_t cap = (int64_t)device_cus() * kResolveBlocksPerCu, want = (items + kBlock - 1) / kBlock;
  const dim3 grid((unsigned)(want < cap ? want : cap));
#define RTX_RESOLVE(K, VEC)                                                                              \
  hipLaunchKernelGGL((k_resolve<K, VEC>), grid, dim3(kBlock), 0, (hipStream_t)stream, samples, k,        \
                     (unsigned)width, (unsigned)n_rows, (unsigned)n_frames, out, out_kind)
  if (k == 2 && vec) {
    RTX_RESOLVE(2, true);
  } else if (k == 2) {
    RTX_RESOLVE(2, false);
  } else if (k == 3) {
    RTX_RESOLVE(3, false);
  } else if (k == 4 && vec) {
    RTX_RESOLVE(4, true);
  } else if (k == 4) {
    RTX_RESOLVE(4, false);
  } else if (vec) {
    RTX_RESOLVE(0, true);
  } else {
    RTX_RESOLVE(0, false);
  }
#undef RTX_RESOLVE
  return check_launch("k_resolve");
}

int rtx_assemble_rows(const void* tiles, int64_t part_stride_bytes, int n_parts, int width, int height,
                      int row_block, int kind, void* out, void* stream) {
  return rtx_assemble_runs(tiles, part_stride_bytes, n_parts, 1, 1, width, height, row_block, kind, out, stream);
}

int rtx_assemble_runs(const void* tiles, int64_t part_stride_bytes, int n_ranks, int root_run, int run, int width,
                      int height, int row_block, int kind, void* out, void* stream) {
  if (!tiles || !out) return rtx_fail(RTX_E_ARG, "null pointer argument");
  if (width <= 0 || height <= 0 || row_block <= 0 || n_ranks <= 0 || root_run <= 0 || run <= 0)
    return rtx_fail(RTX_E_ARG, "bad frame/tile geometry");
  const int n_parts = root_run + (n_ranks - 1) * run;
  int planes = 3;
  int64_t row_bytes;
  if (kind == RTX_OUT_F32_SOA) {
    row_bytes = 4 * (int64_t)width;
  } else if (kind == RTX_OUT_F64_SOA) {
    row_bytes = 8 * (int64_t)width;
  } else if (kind == RTX_OUT_U8_HWC) {
    row_bytes = 3 * (int64_t)width;
    planes = 1;
  } else {
    return rtx_fail(RTX_E_ARG, "bad kind %d", kind);
  }
  int rmax = 0;  // the longest run's rows
  for (int r = 0; r < n_ranks; ++r) {
    const int len = r == 0 ? root_run : run, first = r == 0 ? 0 : root_run + (r - 1) * run;
    const int rows = tile_local_rows(height, row_block, n_parts, first, len);
    rmax = rows > rmax ? rows : rmax;
  }
  if (part_stride_bytes < planes * rmax * row_bytes)
    return rtx_fail(RTX_E_ARG, "part_stride too small (need %lld bytes)", (long long)(planes * rmax * row_bytes));
  const bool vec16 = row_bytes % 16 == 0 && part_stride_bytes % 16 == 0 && (uintptr_t)tiles % 16 == 0 &&
                     (uintptr_t)out % 16 == 0;
  hipLaunchKernelGGL(k_assemble_rows, dim3((unsigned)height, (unsigned)planes), dim3(kBlock), 0, (hipStream_t)stream,
                     (const uint8_t*)tiles, part_stride_bytes, n_parts, root_run, run, height, row_block, row_bytes,
                     vec16, (uint8_t*)out);
  return check_launch("k_assemble_rows");
}

}  // extern "C"
