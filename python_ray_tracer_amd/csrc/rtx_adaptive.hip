// rtx_adaptive.hip — adaptive anti-aliasing (HipRenderer(samples=k, adaptive=True)):
// the three kernels between the plain W x H render and the k x k samples of its edge pixels.
//   k_edge_mask       which pixels are refined: a tie, or an 8-neighbour of another shape, of the other
//                     side of a shadow edge, or of a colour further away than `contrast`
//   k_sample_dirs     the k x k sample rays of the listed pixels: camera_dir on the sample scene
//   k_resolve_scatter the resolve of each listed pixel's samples, written over that
//                     pixel of the frame
// A translation unit of its own, like rtx_aov.hip, over the shared device text (rtx_device.h): the
// render kernels compile from untouched text with untouched flags, and camera_dir / clip01 /
// quant_u8 here are the render path's own.
#include "rtx_device.h"
#include "rtx_internal.h"

namespace {

// k_edge_mask: one lane per pixel; a block is a tile of kMaskW x kMaskH pixels, one wave per tile row,
// so the 64 lanes of a wave are 64 neighbours of a pixel row and every load and the mask store of a
// wave is one contiguous run. The 3 x 3 neighbourhoods come from an LDS tile with a one-pixel halo,
// not from the L2: read straight from memory every pixel costs 46 load instructions (27 colour words,
// 9 ids, 9 lit bytes, its hit count), and the 1080p frame then takes 44 us, bound by the rate the
// vector memory pipeline takes load instructions, not by bytes (the L2 does serve the re-reads).
// With the tile a pixel is loaded 1.55 times ((64 + 2) (4 + 2) / 256), its colour clipped once instead
// of nine times, and the neighbourhood reads are LDS reads of consecutive words. No atomics: a
// pixel's flag depends on the inputs only.
constexpr int kMaskW = 64, kMaskH = kBlock / 64;        // the tile: a wave per row
constexpr int kHaloW = kMaskW + 2, kHaloH = kMaskH + 2;  // with its one-pixel border
constexpr unsigned short kOutside = 0x100;              // "lit" of a halo cell outside the frame (lit is a byte)

__global__ __launch_bounds__(kBlock) void k_edge_mask(const double* __restrict__ color, const int* __restrict__ id,
                                                      const int* __restrict__ hits,
                                                      const unsigned char* __restrict__ lit, int width, int height,
                                                      double contrast, unsigned char* __restrict__ mask) {
  __shared__ double tc[3][kHaloH][kHaloW];  // clip01 of the colour (a NaN is 0, as in the resolve)
  __shared__ int ti[kHaloH][kHaloW];
  __shared__ unsigned short tl[kHaloH][kHaloW];
  const int64_t n = (int64_t)width * height;  // < 2^31 (checked by the host)
  const unsigned tiles_x = ((unsigned)width + kMaskW - 1) / kMaskW;
  const int c0 = (int)(blockIdx.x % tiles_x) * kMaskW, r0 = (int)(blockIdx.x / tiles_x) * kMaskH;
#pragma unroll  // (two rounds: both rounds' loads are in flight together)
  for (int e = threadIdx.x; e < kHaloH * kHaloW; e += kBlock) {
    const int hr = e / kHaloW, hc = e - hr * kHaloW;
    const int rr = r0 + hr - 1, cc = c0 + hc - 1;
    unsigned short l = kOutside;
    if (rr >= 0 && rr < height && cc >= 0 && cc < width) {
      const int64_t q = (int64_t)rr * width + cc;
      tc[0][hr][hc] = clip01(color[q]);
      tc[1][hr][hc] = clip01(color[n + q]);
      tc[2][hr][hc] = clip01(color[2 * n + q]);
      ti[hr][hc] = id[q];
      l = lit[q];
    }
    tl[hr][hc] = l;
  }
  __syncthreads();
  const int tx = (int)(threadIdx.x & 63u), ty = (int)(threadIdx.x >> 6);
  const int r = r0 + ty, c = c0 + tx;
  if (r >= height || c >= width) return;
  const int64_t i = (int64_t)r * width + c;
  bool flag = hits[i] > 1;  // a tie: two shapes share the pixel's first hit
  const int id0 = ti[ty + 1][tx + 1];
  const unsigned short lit0 = tl[ty + 1][tx + 1];
  const double cr = tc[0][ty + 1][tx + 1], cg = tc[1][ty + 1][tx + 1], cb = tc[2][ty + 1][tx + 1];
#pragma unroll
  for (int dr = 0; dr <= 2; ++dr) {
#pragma unroll
    for (int dc = 0; dc <= 2; ++dc) {
      if (dr == 1 && dc == 1) continue;
      const int hr = ty + dr, hc = tx + dc;
      const unsigned short lq = tl[hr][hc];
      // strict, in float64, on the clipped colours; branch-free (a wave's lanes rarely agree)
      const bool far = (__builtin_fabs(tc[0][hr][hc] - cr) > contrast) | (__builtin_fabs(tc[1][hr][hc] - cg) > contrast) |
                       (__builtin_fabs(tc[2][hr][hc] - cb) > contrast);
      // (no neighbour beyond the frame's border)
      flag |= (lq != kOutside) & ((ti[hr][hc] != id0) | (lq != lit0) | far);
    }
  }
  mask[i] = flag ? 1 : 0;
}

// One lane per sample ray t = j * k*k + sy * k + sx of listed pixel j: consecutive lanes store
// consecutive words of each plane of dirs. The direction is camera_dir of pixel (k*c + sx, k*r + sy)
// of the sample scene's (k*width, k*height) camera: what k_ray_dirs and the render kernels compute
// for that pixel of the sample frame. A listed index outside the frame gives a zero direction.
__global__ __launch_bounds__(kBlock) void k_sample_dirs(const double* __restrict__ scene, int k, int width,
                                                        int height, const int* __restrict__ pixels, int n_rays,
                                                        double* __restrict__ dirs) {
  const int64_t t64 = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (t64 >= n_rays) return;
  const int t = (int)t64;
  const int kk = k * k;
  const int j = t / kk, s = t - j * kk;
  const int sy = s / k, sx = s - sy * k;
  const int px = pixels[j];
  double dx = 0.0, dy = 0.0, dz = 0.0;
  if (px >= 0 && px < width * height) {
    const int r = px / width, c = px - r * width;
    camera_dir((const cdouble*)scene, k * c + sx, k * r + sy, k * width, k * height, dx, dy, dz);
  }
  dirs[t] = dx;
  dirs[(int64_t)n_rays + t] = dy;
  dirs[2 * (int64_t)n_rays + t] = dz;
}

// k_resolve_scatter: one lane per listed pixel with its three planes (the uint8 triple of a pixel
// stays in one lane). The k*k samples of a pixel and plane are contiguous in ray order (sy * k + sx),
// so the 64 pixels of a wave own one contiguous run of 64 * k*k doubles per plane. Read lane by lane
// (each lane walking its own k*k doubles) every load instruction of a wave touches 64 cache lines
// for 512 bytes; instead the wave copies the run into LDS with contiguous loads, kScatterChunk
// samples of every pixel at a time (a pixel's piece is then 128 bytes), and each lane adds its own
// pixel's samples from there, in order. A pixel's row in LDS is padded by one double, so the lanes'
// reads fall into different banks.
constexpr int kScatterChunk = 16;
constexpr int kScatterRow = kScatterChunk + 1;

// the resolve of the wave's `cnt` pixels for one plane (s: the wave's run of that plane): each sample
// clipped, added to 0.0 in ray order (rows top to bottom, left to right), divided once by k*k:
// resolve_block's chain. Every thread of the block calls it (block barriers), cnt may be 0.
__device__ __forceinline__ double scatter_plane(const double* __restrict__ s, int kk, int cnt, int lane,
                                                double* __restrict__ st) {
  double acc = 0.0;
  for (int a0 = 0; a0 < kk; a0 += kScatterChunk) {
    const int len = kk - a0 < kScatterChunk ? kk - a0 : kScatterChunk;
    // word t = u * 64 + lane of the chunk is sample a0 + t % len of pixel t / len: all of a lane's
    // loads (at most kScatterChunk, fewer words than that only in the last wave) are issued before the
    // first is stored, and (t / len, t % len) advance by (64 / len, 64 % len) instead of a division
    const int dq = 64 / len, dr = 64 - dq * len, words = cnt * len;
    double v[kScatterChunk];
    int p = lane / len, a = lane - p * len;
    const int p0 = p, a_0 = a;
#pragma unroll
    for (int u = 0; u < kScatterChunk; ++u) {
      v[u] = u * 64 + lane < words ? __builtin_nontemporal_load(s + (int64_t)p * kk + a0 + a) : 0.0;
      a += dr, p += dq;
      if (a >= len) a -= len, ++p;
    }
    __syncthreads();  // the previous chunk (or plane) has been read
    p = p0, a = a_0;
#pragma unroll
    for (int u = 0; u < kScatterChunk; ++u) {
      if (u * 64 + lane < words) st[p * kScatterRow + a] = v[u];
      a += dr, p += dq;
      if (a >= len) a -= len, ++p;
    }
    __syncthreads();
    if (lane < cnt)
      for (int a1 = 0; a1 < len; ++a1) acc = acc + clip01(st[lane * kScatterRow + a1]);
  }
  return acc / (double)kk;
}

// Writes the listed pixels of `out` only; an index outside the frame is skipped.
__global__ __launch_bounds__(kBlock) void k_resolve_scatter(const double* __restrict__ samples, int k,
                                                            const int* __restrict__ pixels, int n_flagged,
                                                            int width, int height, void* __restrict__ out,
                                                            int out_kind) {
  __shared__ double stage[kBlock / 64][64 * kScatterRow];
  const int lane = (int)(threadIdx.x & 63u), wave = (int)(threadIdx.x >> 6);
  const int64_t j0 = (int64_t)blockIdx.x * kBlock + wave * 64;  // the wave's first listed pixel
  const int64_t left = (int64_t)n_flagged - j0;
  const int cnt = left <= 0 ? 0 : left < 64 ? (int)left : 64;  // (the last block's tail waves: 0)
  const int kk = k * k;
  const int64_t ns = (int64_t)n_flagged * kk;  // samples of a plane (< 2^31)
  const int64_t n = (int64_t)width * height;
  const double* s = samples + j0 * kk;  // (not dereferenced when cnt == 0)
  const double cr = scatter_plane(s, kk, cnt, lane, stage[wave]);
  const double cg = scatter_plane(s + ns, kk, cnt, lane, stage[wave]);
  const double cb = scatter_plane(s + 2 * ns, kk, cnt, lane, stage[wave]);
  if (lane >= cnt) return;
  const int px = pixels[j0 + lane];
  if (px < 0 || px >= n) return;
  if (out_kind == RTX_OUT_F32_SOA) {
    float* o = (float*)out + px;
    o[0] = (float)cr;
    o[n] = (float)cg;
    o[2 * n] = (float)cb;
  } else if (out_kind == RTX_OUT_F64_SOA) {
    double* o = (double*)out + px;
    o[0] = cr;
    o[n] = cg;
    o[2 * n] = cb;
  } else {
    unsigned char* o = (unsigned char*)out + 3 * (int64_t)px;
    o[0] = quant_u8(cr);
    o[1] = quant_u8(cg);
    o[2] = quant_u8(cb);
  }
}

constexpr int64_t kIndexLimit = (int64_t)1 << 31;  // pixel and sample-ray indices are 32-bit

bool frame_fits(int width, int height) { return (int64_t)width * height < kIndexLimit; }

unsigned blocks_for(int64_t items) { return (unsigned)((items + kBlock - 1) / kBlock); }

}  // namespace

extern "C" {

int rtx_edge_mask(const double* color_f64, const int32_t* id, const int32_t* hits, const uint8_t* lit, int width,
                  int height, double contrast, uint8_t* mask_out, void* stream) {
  if (!color_f64 || !id || !hits || !lit || !mask_out)
    return rtx_fail(RTX_E_ARG, "rtx_edge_mask: null pointer argument");
  if (width <= 0 || height <= 0 || !frame_fits(width, height))
    return rtx_fail(RTX_E_ARG, "rtx_edge_mask: bad frame geometry (width and height positive, width*height below 2^31)");
  if (!(contrast >= 0.0))
    return rtx_fail(RTX_E_ARG, "rtx_edge_mask: contrast must be >= 0 (+inf: no colour test), not NaN");
  const int64_t tiles = (((int64_t)width + kMaskW - 1) / kMaskW) * (((int64_t)height + kMaskH - 1) / kMaskH);
  if (tiles >= kIndexLimit)
    return rtx_fail(RTX_E_ARG, "rtx_edge_mask: bad frame geometry (too many tiles for one launch)");
  hipLaunchKernelGGL(k_edge_mask, dim3((unsigned)tiles), dim3(kBlock), 0, (hipStream_t)stream, color_f64,
                     (const int*)id, (const int*)hits, lit, width, height, contrast, mask_out);
  return rtx_launched("k_edge_mask");
}

int rtx_sample_dirs(const double* sample_scene, int k, int width, int height, const int32_t* pixels_i32,
                    int n_flagged, double* dirs_out, void* stream) {
  if (!sample_scene || !dirs_out || (!pixels_i32 && n_flagged != 0))
    return rtx_fail(RTX_E_ARG, "rtx_sample_dirs: null pointer argument");
  if (k < 1 || k > 8) return rtx_fail(RTX_E_ARG, "rtx_sample_dirs: samples per pixel side must be in 1..8");
  if (width <= 0 || height <= 0 || n_flagged < 0 || !frame_fits(width, height) ||
      (int64_t)k * width >= kIndexLimit || (int64_t)k * height >= kIndexLimit)
    return rtx_fail(RTX_E_ARG, "rtx_sample_dirs: bad frame geometry or a negative pixel count");
  if ((int64_t)n_flagged * k * k >= kIndexLimit)
    return rtx_fail(RTX_E_ARG, "rtx_sample_dirs: n_flagged*k*k must stay below 2^31 sample rays");
  if (n_flagged == 0) return RTX_OK;
  const int n_rays = n_flagged * k * k;
  hipLaunchKernelGGL(k_sample_dirs, dim3(blocks_for(n_rays)), dim3(kBlock), 0, (hipStream_t)stream, sample_scene, k,
                     width, height, (const int*)pixels_i32, n_rays, dirs_out);
  return rtx_launched("k_sample_dirs");
}

int rtx_resolve_scatter(const double* samples_f64, int k, const int32_t* pixels_i32, int n_flagged, int width,
                        int height, void* out, int out_kind, void* stream) {
  if (!samples_f64 || !out || (!pixels_i32 && n_flagged != 0))
    return rtx_fail(RTX_E_ARG, "rtx_resolve_scatter: null pointer argument");
  if (k < 1 || k > 8) return rtx_fail(RTX_E_ARG, "rtx_resolve_scatter: samples per pixel side must be in 1..8");
  if (width <= 0 || height <= 0 || n_flagged < 0 || !frame_fits(width, height))
    return rtx_fail(RTX_E_ARG, "rtx_resolve_scatter: bad frame geometry or a negative pixel count");
  if (out_kind != RTX_OUT_F32_SOA && out_kind != RTX_OUT_F64_SOA && out_kind != RTX_OUT_U8_HWC)
    return rtx_fail(RTX_E_ARG, "rtx_resolve_scatter: bad out_kind");
  if ((int64_t)n_flagged * k * k >= kIndexLimit)
    return rtx_fail(RTX_E_ARG, "rtx_resolve_scatter: n_flagged*k*k must stay below 2^31 samples per plane");
  if (n_flagged == 0) return RTX_OK;
  hipLaunchKernelGGL(k_resolve_scatter, dim3(blocks_for(n_flagged)), dim3(kBlock), 0, (hipStream_t)stream,
                     samples_f64, k, (const int*)pixels_i32, n_flagged, width, height, out, out_kind);
  return rtx_launched("k_resolve_scatter");
}

}  // extern "C"
