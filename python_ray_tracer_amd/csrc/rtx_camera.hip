// rtx_camera.hip — the ray generator of a perspective camera (domain.PerspectiveCamera):
// a position, a target, an up vector, a vertical field of view and a thin lens, where
// get_ray_directions (base.py:123-141) has a position in front of a screen fixed at z = 0.
//   k_camera_rays   the k x k sample rays of every pixel of one row tile, in the order of a sample
//                   frame's rows (what rtx_resolve_samples reads): directions, and with a lens origins
// A translation unit of its own, like rtx_aov.hip and rtx_adaptive.hip: the render kernels compile from
// untouched text with untouched flags. The rays are traced by rtx_trace_rays / rtx_primary_aovs_rays.
#include "rtx_device.h"
#include "rtx_internal.h"

namespace {

// the camera record (include/rtx_hip.h) as a kernel argument: the host pointer is read during the call
struct CamRec {
  double w[RTX_C_LV + 3];
};

// One lane per ray, consecutive lanes on consecutive ray indices: every store instruction of a wave
// writes 512 contiguous bytes of one plane. Nontemporal stores: the trace reads the rays back once.
// A streaming kernel (24 bytes per ray, 48 with a lens), no LDS, no atomics. K (the samples per pixel
// side) is a template parameter, so that the divisions by k and k*k are by constants; the one
// division by the sample row's length k*width (and the tile's row mapping) happens once per lane.
// LENS: the samples leave through the lens table (at most 128 doubles, read through the cache),
// rotated per pixel by a hash of (column, global row); without it every offset is (0, 0).
// The arithmetic is the contract of include/rtx_hip.h, in its order; iw and ih are the host's
// correctly rounded 1.0 / (k*width) and 1.0 / (k*height).
template <int K, bool LENS>
__global__ __launch_bounds__(kBlock) void k_camera_rays(CamRec cam, const double* __restrict__ lens, unsigned sw,
                                                        int row_block, int n_parts, int part, int part_run,
                                                        double iw, double ih, int64_t n,
                                                        double* __restrict__ origins, double* __restrict__ dirs) {
  const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (t >= n) return;
  const unsigned ti = (unsigned)t;  // n < 2^31 (checked by the host)
  const unsigned srow = ti / sw, ix = ti - srow * sw;  // local sample row, sample column
  const unsigned lr = srow / K, sy = srow - lr * K;
  const unsigned c = ix / K, sx = ix - c * K;
  unsigned gr = lr;
  if (n_parts != 1) {  // (uniform; the row mapping of rtx_render_camera_sched, global_row in rtx_device.h)
    const unsigned own = (unsigned)(row_block * part_run);
    const unsigned cyc = lr / own;
    gr = cyc * (unsigned)(n_parts * row_block) + (unsigned)(part * row_block) + (lr - cyc * own);
  }
  const unsigned iy = K * gr + sy;
  const double u = (double)(2u * ix + 1u) * iw - 1.0;
  const double v = 1.0 - (double)(2u * iy + 1u) * ih;
  double a = 0.0, b = 0.0;
  if (LENS) {
    constexpr unsigned kk = K * K;
    unsigned h = c * 0x9E3779B1u ^ gr * 0x85EBCA77u;
    h ^= h >> 16;
    h *= 0x7FEB352Du;
    h ^= h >> 15;
    h *= 0x846CA68Bu;
    h ^= h >> 16;
    const unsigned j = ((sy * K + sx) + h % kk) % kk;
    a = lens[j];
    b = lens[kk + j];
  }
  const double* w = cam.w;
  const double offx = w[RTX_C_LU + 0] * a + w[RTX_C_LV + 0] * b;
  const double offy = w[RTX_C_LU + 1] * a + w[RTX_C_LV + 1] * b;
  const double offz = w[RTX_C_LU + 2] * a + w[RTX_C_LV + 2] * b;
  if (origins) {
    __builtin_nontemporal_store(w[RTX_C_EYE + 0] + offx, origins + t);
    __builtin_nontemporal_store(w[RTX_C_EYE + 1] + offy, origins + n + t);
    __builtin_nontemporal_store(w[RTX_C_EYE + 2] + offz, origins + 2 * n + t);
  }
  const double dx = ((w[RTX_C_FWD + 0] + w[RTX_C_U + 0] * u) + w[RTX_C_V + 0] * v) - offx;
  const double dy = ((w[RTX_C_FWD + 1] + w[RTX_C_U + 1] * u) + w[RTX_C_V + 1] * v) - offy;
  const double dz = ((w[RTX_C_FWD + 2] + w[RTX_C_U + 2] * u) + w[RTX_C_V + 2] * v) - offz;
  // the reference's norm() (base.py:61-64): correctly rounded square root and division
  const double r = 1.0 / __builtin_sqrt((dx * dx + dy * dy) + dz * dz);
  __builtin_nontemporal_store(dx * r, dirs + t);
  __builtin_nontemporal_store(dy * r, dirs + n + t);
  __builtin_nontemporal_store(dz * r, dirs + 2 * n + t);
}

constexpr int64_t kRayLimit = (int64_t)1 << 31;  // ray indices within a plane are 32-bit

template <int K>
void launch_camera_rays(bool lens_on, dim3 grid, hipStream_t s, const CamRec& cam, const double* lens, unsigned sw,
                        int row_block, int n_parts, int part, int part_run, double iw, double ih, int64_t n,
                        double* origins, double* dirs) {
  if (lens_on) {
    hipLaunchKernelGGL((k_camera_rays<K, true>), grid, dim3(kBlock), 0, s, cam, lens, sw, row_block, n_parts, part,
                       part_run, iw, ih, n, origins, dirs);
  } else {
    hipLaunchKernelGGL((k_camera_rays<K, false>), grid, dim3(kBlock), 0, s, cam, lens, sw, row_block, n_parts, part,
                       part_run, iw, ih, n, origins, dirs);
  }
}

}  // namespace

extern "C" {

int rtx_camera_rays(const double* cam, const double* lens, int k, int width, int height, int row_block, int n_parts,
                    int part, int part_run, int n_local_rows, double* origins_out, double* dirs_out, void* stream) {
  if (!cam || !dirs_out) return rtx_fail(RTX_E_ARG, "rtx_camera_rays: null pointer argument");
  if (k < 1 || k > 8) return rtx_fail(RTX_E_ARG, "rtx_camera_rays: samples per pixel side must be in 1..8");
  if (!tile_geometry_ok(width, height, row_block, n_parts, part, part_run, n_local_rows))
    return rtx_fail(RTX_E_ARG, "rtx_camera_rays: bad frame/tile geometry");
  if ((int64_t)k * width >= kRayLimit || (int64_t)k * height >= kRayLimit)
    return rtx_fail(RTX_E_ARG, "rtx_camera_rays: k*width and k*height must stay below 2^31");
  // (k*width < 2^31 and k <= 8, so the product below cannot overflow 64 bits)
  const int64_t n = (int64_t)k * width * k * n_local_rows;
  if (n >= kRayLimit) return rtx_fail(RTX_E_ARG, "rtx_camera_rays: k*k*width*n_local_rows must stay below 2^31 rays");
  CamRec rec;
  bool has_lens = false;
  for (int i = 0; i < RTX_C_LV + 3; ++i) {
    rec.w[i] = cam[i];
    if (!(cam[i] - cam[i] == 0.0)) return rtx_fail(RTX_E_ARG, "rtx_camera_rays: camera record word %d is not finite", i);
    if (i >= RTX_C_LU && cam[i] != 0.0) has_lens = true;
  }
  if (has_lens && (!lens || !origins_out))
    return rtx_fail(RTX_E_ARG, "rtx_camera_rays: a record with a lens (LU, LV) needs the lens table and origins_out");
  if (n == 0) return RTX_OK;
  const double iw = 1.0 / (double)((int64_t)k * width), ih = 1.0 / (double)((int64_t)k * height);
  const dim3 grid((unsigned)((n + kBlock - 1) / kBlock));
  const unsigned sw = (unsigned)k * (unsigned)width;
  hipStream_t s = (hipStream_t)stream;
#define RTX_CAMERA_K(K)                                                                                              \
  case K:                                                                                                            \
    launch_camera_rays<K>(lens != nullptr, grid, s, rec, lens, sw, row_block, n_parts, part, part_run, iw, ih, n,    \
                          origins_out, dirs_out);                                                                    \
    break;
  switch (k) {
    RTX_CAMERA_K(1)
    RTX_CAMERA_K(2)
    RTX_CAMERA_K(3)
    RTX_CAMERA_K(4)
    RTX_CAMERA_K(5)
    RTX_CAMERA_K(6)
    RTX_CAMERA_K(7)
    RTX_CAMERA_K(8)
  }
#undef RTX_CAMERA_K
  return rtx_launched("k_camera_rays");
}

}  // extern "C"
