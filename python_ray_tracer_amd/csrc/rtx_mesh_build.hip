// rtx_mesh_build.hip — the table of rtx_trace_mesh / rtx_trace_mesh_uv made on the device:
// the triangle rows, the order of the tree's leaves, the node boxes and margins and the UV part, written
// into a skeleton that already holds what depends on (T, max_leaf) and the materials alone. The contract
// is the host's table (python_ray_tracer_amd/meshes.py mesh_table), value for value: every operation here
// is exact or correctly rounded float64 in NumPy's order (no contraction), and the order of the leaves is
// the host's lexsort, realised as two stable radix sorts per level (rocPRIM).
//
// State per triangle t (its number in the group): its segment [seg_s, seg_e) of the leaf order, its
// segment's node and its position. A level cuts every segment longer than the leaf size:
//   k_keys      a cut segment's triangles get the centre along the segment's axis as a sortable word, the
//               others their position;
//   sort 1      (key, t) by key, from the triangles in number order: equal keys stay in number order;
//   k_seg_keys  the segment's start of every sorted triangle;
//   sort 2      (start, t) by start, stable: the segments in place, each in (key, number) order, and a
//               segment that is not cut where it was;
//   k_update    positions, the two halves' ranges and nodes, and the halves' boxes and centre extents
//               reduced into their nodes (a wave whose lanes share a node reduces first).
// A device unit of its own: it shares no device text with the render path (rtx_device.h is not included), so
// every render kernel keeps its machine code.
#include <rocprim/device/device_radix_sort.hpp>

#include "rtx_internal.h"

namespace {

using u64 = unsigned long long;

constexpr int kBlock = 256;
constexpr int kRowBlock = 128;  // k_write: 128 rows staged in 24 KiB of LDS
constexpr uint32_t kNone = RTX_MB_NONE;
constexpr double kMargin = 2e-7;  // meshes.MARGIN

// a double as a word whose unsigned order is the double's order (-0.0 below 0.0; no NaN reaches here)
__device__ __forceinline__ u64 enc(double x) {
  const u64 b = (u64)__double_as_longlong(x);
  return b ^ ((b >> 63) ? ~0ull : 0x8000000000000000ull);
}
__device__ __forceinline__ double dec(u64 k) {
  const u64 b = k ^ ((k >> 63) ? 0x8000000000000000ull : ~0ull);
  return __longlong_as_double((long long)b);
}

struct BuildParams {
  const double* verts;
  const int32_t* faces;
  const int32_t* tri_mesh;
  const double* normals;
  const int32_t* smooth;
  const double* uvs;
  double* table;
  int64_t n_verts;
  int64_t tris_at, nodes_at, uvs_at;  // word offsets (uvs_at 0: no UV part)
  int T, N, M, leaf;
  uint32_t* status;  // [0] the lowest degenerate triangle (kNone: none), [1] 1: an index out of range
  double* centre;    // [T][3]
  double* lo;        // [T][3]
  double* hi;        // [T][3]
  u64* nbox;         // [N][6] lo, hi of the node's boxes, as enc words
  u64* next;         // [N][6] lo, hi of the node's centres
  int32_t *seg_s, *seg_e, *node_of, *pos, *order, *iota, *sorted;
  u64 *key, *key_sorted;
  uint32_t *seg_key, *seg_key_sorted;
};

struct Tri {
  double v0[3], e1[3], e2[3], ng[3];
  int f[3], mesh;
  bool bad;  // the normal cannot be normalised
};

// The row's geometry as triangle_rows computes it.
__device__ __forceinline__ Tri triangle(const BuildParams& p, int t) {
  Tri r;
  bool range = false;
  for (int k = 0; k < 3; ++k) {
    int i = p.faces[3 * (int64_t)t + k];
    if (i < 0 || i >= p.n_verts) i = 0, range = true;
    r.f[k] = i;
  }
  r.mesh = p.tri_mesh[t];
  if (r.mesh < 0 || r.mesh >= p.M) r.mesh = 0, range = true;
  if (range) p.status[1] = 1u;
  const double* a = p.verts + 3 * (int64_t)r.f[0];
  const double* b = p.verts + 3 * (int64_t)r.f[1];
  const double* c = p.verts + 3 * (int64_t)r.f[2];
  for (int k = 0; k < 3; ++k) {
    r.v0[k] = a[k];
    r.e1[k] = b[k] - a[k];
    r.e2[k] = c[k] - a[k];
  }
  const double nx = r.e1[1] * r.e2[2] - r.e1[2] * r.e2[1];
  const double ny = r.e1[2] * r.e2[0] - r.e1[0] * r.e2[2];
  const double nz = r.e1[0] * r.e2[1] - r.e1[1] * r.e2[0];
  const double mag = sqrt((nx * nx + ny * ny) + nz * nz);
  r.ng[0] = nx / mag;
  r.ng[1] = ny / mag;
  r.ng[2] = nz / mag;
  r.bad = !(isfinite(r.ng[0]) && isfinite(r.ng[1]) && isfinite(r.ng[2]));
  return r;
}

// min / max of the lanes' six words into slot[0..2] / slot[3..5]: one atomic per word and wave where every
// lane of the wave takes part with the same slot, one per lane otherwise.
__device__ __forceinline__ void reduce_into(u64* base, int node, bool active, const u64 mn[3], const u64 mx[3]) {
  const int first = __shfl(node, 0);
  const bool uniform = __all(active && node == first);
  if (uniform) {
    u64 a[6] = {mn[0], mn[1], mn[2], mx[0], mx[1], mx[2]};
    for (int off = 32; off >= 1; off >>= 1)
      for (int k = 0; k < 6; ++k) {
        const u64 o = __shfl_xor(a[k], off);
        a[k] = k < 3 ? (o < a[k] ? o : a[k]) : (o > a[k] ? o : a[k]);
      }
    if ((threadIdx.x & 63) == 0) {
      u64* slot = base + 6 * (int64_t)first;
      for (int k = 0; k < 3; ++k) atomicMin(slot + k, a[k]);
      for (int k = 3; k < 6; ++k) atomicMax(slot + k, a[k]);
    }
  } else if (active) {
    u64* slot = base + 6 * (int64_t)node;
    for (int k = 0; k < 3; ++k) atomicMin(slot + k, mn[k]);
    for (int k = 0; k < 3; ++k) atomicMax(slot + 3 + k, mx[k]);
  }
}

// a triangle's box and centre into its node: the box always, the centre where the node will be cut
__device__ __forceinline__ void reduce_triangle(const BuildParams& p, int t, int node, bool active, bool cut) {
  u64 mn[3] = {0, 0, 0}, mx[3] = {0, 0, 0}, c[3] = {0, 0, 0};
  if (active)
    for (int k = 0; k < 3; ++k) {
      mn[k] = enc(p.lo[3 * (int64_t)t + k]);
      mx[k] = enc(p.hi[3 * (int64_t)t + k]);
      c[k] = enc(p.centre[3 * (int64_t)t + k]);
    }
  reduce_into(p.nbox, node, active, mn, mx);
  reduce_into(p.next, node, active && cut, c, c);
}

__global__ __launch_bounds__(kBlock) void k_build_init(BuildParams p) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i < 6 * (int64_t)p.N) {
    const u64 v = i % 6 < 3 ? ~0ull : 0ull;
    p.nbox[i] = v;
    p.next[i] = v;
  }
  if (i == 0) p.status[0] = kNone, p.status[1] = 0u;
}

// boxes and centres of the triangles in number order, the degenerate ones noted, everything in the root
__global__ __launch_bounds__(kBlock) void k_build_rows(BuildParams p) {
  const int t = blockIdx.x * kBlock + threadIdx.x;
  const bool active = t < p.T;
  if (active) {
    const Tri r = triangle(p, t);
    if (r.bad) atomicMin(p.status, (uint32_t)t);
    for (int k = 0; k < 3; ++k) {
      const double a = r.v0[k], b = r.v0[k] + r.e1[k], c = r.v0[k] + r.e2[k];
      const double lo = fmin(fmin(a, b), c), hi = fmax(fmax(a, b), c);
      p.lo[3 * (int64_t)t + k] = lo;
      p.hi[3 * (int64_t)t + k] = hi;
      p.centre[3 * (int64_t)t + k] = (lo + hi) * 0.5;
    }
    p.seg_s[t] = 0;
    p.seg_e[t] = p.T;
    p.node_of[t] = 0;
    p.pos[t] = t;
    p.order[t] = t;
    p.iota[t] = t;
  }
  reduce_triangle(p, t, 0, active, p.leaf > 0 && p.T > p.leaf);
}

__global__ __launch_bounds__(kBlock) void k_build_keys(BuildParams p) {
  const int t = blockIdx.x * kBlock + threadIdx.x;
  if (t >= p.T) return;
  u64 key = (u64)p.pos[t];
  if (p.seg_e[t] - p.seg_s[t] > p.leaf) {
    const u64* e = p.next + 6 * (int64_t)p.node_of[t];
    const double ex = dec(e[3]) - dec(e[0]), ey = dec(e[4]) - dec(e[1]), ez = dec(e[5]) - dec(e[2]);
    int axis = 0;  // the first largest extent, as argmax
    double best = ex;
    if (ey > best) axis = 1, best = ey;
    if (ez > best) axis = 2;
    key = enc(p.centre[3 * (int64_t)t + axis] + 0.0);  // (+ 0.0: -0.0 and 0.0 are one key)
  }
  p.key[t] = key;
}

__global__ __launch_bounds__(kBlock) void k_build_seg_keys(BuildParams p) {
  const int i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= p.T) return;
  int t = p.sorted[i];
  if (t < 0 || t >= p.T) t = 0;
  p.seg_key[i] = (uint32_t)p.seg_s[t];
}

__global__ __launch_bounds__(kBlock) void k_build_update(BuildParams p) {
  const int q = blockIdx.x * kBlock + threadIdx.x;
  bool cut = false, again = false;
  int t = 0, child = 0;
  if (q < p.T) {
    t = p.order[q];
    if (t < 0 || t >= p.T) t = 0;
    p.pos[t] = q;
    int s = p.seg_s[t], e = p.seg_e[t];
    if (e - s > p.leaf) {
      const int mid = s + (e - s + 1) / 2;
      const int left = p.node_of[t] + 1;
      child = left;
      if (q < mid) {
        e = mid;
      } else {
        s = mid;
        child = left < p.N ? (int)p.table[p.nodes_at + (int64_t)left * RTX_NODE_WORDS + RTX_N_SKIP] : p.N;
      }
      cut = child >= 0 && child < p.N;  // (a skeleton of another tree: nothing is written outside the nodes)
      if (!cut) child = 0;
      p.seg_s[t] = s;
      p.seg_e[t] = e;
      p.node_of[t] = child;
      again = e - s > p.leaf;
    }
  }
  reduce_triangle(p, t, child, cut, again);
}

__global__ __launch_bounds__(kBlock) void k_build_nodes(BuildParams p) {
  const int n = blockIdx.x * kBlock + threadIdx.x;
  if (n >= p.N) return;
  double* node = p.table + p.nodes_at + (int64_t)n * RTX_NODE_WORDS;
  double far = 0.0, m[3];
  for (int k = 0; k < 3; ++k) {
    const double lo = dec(p.nbox[6 * (int64_t)n + k]), hi = dec(p.nbox[6 * (int64_t)n + 3 + k]);
    node[RTX_N_LOX + k] = lo;
    node[RTX_N_HIX + k] = hi;
    m[k] = fmax(fabs(lo), fabs(hi));
  }
  far = (m[0] * m[0] + m[1] * m[1]) + m[2] * m[2];
  node[RTX_N_MARGIN] = kMargin * (1.0 + far);
}

// the rows in leaf order: a block's rows are laid out in LDS and written as one contiguous run
__global__ __launch_bounds__(kRowBlock) void k_build_write(BuildParams p) {
  __shared__ double rows[kRowBlock * RTX_TRI_WORDS];
  const int base = blockIdx.x * kRowBlock;
  const int q = base + threadIdx.x;
  if (q < p.T) {
    int t = p.order[q];
    if (t < 0 || t >= p.T) t = 0;
    const Tri r = triangle(p, t);
    double* row = rows + threadIdx.x * RTX_TRI_WORDS;
    for (int k = 0; k < 3; ++k) {
      row[RTX_T_V0 + k] = r.v0[k];
      row[RTX_T_E1 + k] = r.e1[k];
      row[RTX_T_E2 + k] = r.e2[k];
      row[RTX_T_NG + k] = r.ng[k];
    }
    row[RTX_T_MESH] = (double)r.mesh;
    const bool smooth = p.normals && p.smooth && p.smooth[r.mesh] != 0;
    row[RTX_T_SMOOTH] = smooth ? 1.0 : 0.0;
    for (int c = 0; c < 3; ++c)
      for (int k = 0; k < 3; ++k)
        row[RTX_T_N0 + 3 * c + k] = smooth ? p.normals[3 * (int64_t)r.f[c] + k] : 0.0;
    row[RTX_T_NUM] = (double)t;
    if (p.uvs_at) {
      double* uv = p.table + p.uvs_at + (int64_t)q * RTX_UV_WORDS;
      for (int k = 0; k < RTX_UV_WORDS; ++k) uv[k] = p.uvs ? p.uvs[(int64_t)t * RTX_UV_WORDS + k] : 0.0;
    }
  }
  __syncthreads();
  const int n_rows = p.T - base < kRowBlock ? p.T - base : kRowBlock;
  double* out = p.table + p.tris_at + (int64_t)base * RTX_TRI_WORDS;
  for (int i = threadIdx.x; i < n_rows * RTX_TRI_WORDS; i += kRowBlock) out[i] = rows[i];
}

// ---- the host side ----
size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

// the sorts' temporary storage: rocPRIM's own copies of keys and values and its counters, bounded from
// above (rtx_mesh_build asks rocPRIM and refuses a case that would need more)
size_t sort_bytes(int64_t T) { return align256((size_t)T * 32 + ((size_t)1 << 20)); }

// The nodes of the tree over T triangles with leaves of at most `leaf` (0: one leaf), and its levels.
void tree_shape(int64_t T, int64_t leaf, int64_t& nodes, int& levels) {
  nodes = 0, levels = 0;
  // a level's segments have at most two lengths, a and a + 1
  int64_t a = T, na = 1, nb = 0;  // na of length a, nb of length a + 1
  for (;;) {
    nodes += na + nb;
    const bool cut_a = leaf > 0 && a > leaf, cut_b = leaf > 0 && nb > 0 && a + 1 > leaf;
    if (!cut_a && !cut_b) break;
    ++levels;
    // a -> ceil(a/2), floor(a/2); a + 1 -> ceil((a+1)/2), floor((a+1)/2); uncut segments drop out
    const int64_t h = a / 2;  // the new shorter length, where anything of length a or a + 1 is cut
    int64_t nh = 0, nh1 = 0;  // of length h, h + 1
    if (cut_a) (a % 2 ? (nh += na, nh1 += na) : (nh += 2 * na));
    if (cut_b) (a % 2 ? (nh1 += 2 * nb) : (nh += nb, nh1 += nb));
    if (nh == 0) {  // (only a + 1 was cut and a is odd: every half has length h + 1)
      a = h + 1, na = nh1, nb = 0;
    } else {
      a = h, na = nh, nb = nh1;
    }
  }
}

struct Layout {
  size_t status, centre, lo, hi, nbox, next, seg_s, seg_e, node_of, pos, order, iota, sorted, key, key_sorted, seg_key,
      seg_key_sorted, sort, end;
};
Layout layout(int64_t T, int64_t N) {
  Layout l{};
  size_t at = 0;
  auto take = [&](size_t bytes) {
    const size_t here = at;
    at += align256(bytes);
    return here;
  };
  l.status = take(RTX_WS_HDR_BYTES);
  l.centre = take((size_t)T * 24), l.lo = take((size_t)T * 24), l.hi = take((size_t)T * 24);
  l.nbox = take((size_t)N * 48), l.next = take((size_t)N * 48);
  l.seg_s = take((size_t)T * 4), l.seg_e = take((size_t)T * 4), l.node_of = take((size_t)T * 4);
  l.pos = take((size_t)T * 4), l.order = take((size_t)T * 4), l.iota = take((size_t)T * 4), l.sorted = take((size_t)T * 4);
  l.key = take((size_t)T * 8), l.key_sorted = take((size_t)T * 8);
  l.seg_key = take((size_t)T * 4), l.seg_key_sorted = take((size_t)T * 4);
  l.sort = take(sort_bytes(T));
  l.end = at;
  return l;
}

}  // namespace

extern "C" int64_t rtx_mesh_build_nodes(int64_t n_triangles, int max_leaf) {
  if (n_triangles < 1 || n_triangles > RTX_MAX_TRIANGLES || max_leaf < 0) return 0;
  int64_t nodes = 0;
  int levels = 0;
  tree_shape(n_triangles, max_leaf, nodes, levels);
  return nodes;
}

extern "C" size_t rtx_mesh_build_workspace_bytes(int64_t n_triangles, int64_t n_nodes) {
  if (n_triangles < 1 || n_triangles > RTX_MAX_TRIANGLES || n_nodes < 1 || n_nodes > 2 * n_triangles) return 0;
  return layout(n_triangles, n_nodes).end;
}

extern "C" int rtx_mesh_build(const double* vertices, int64_t n_vertices, const int32_t* faces, const int32_t* tri_mesh,
                              int64_t n_triangles, const double* normals, const int32_t* mesh_smooth, const double* uvs,
                              const double* header, double* table, int64_t table_words, int max_leaf, void* workspace,
                              size_t workspace_bytes, void* stream) {
  if (!vertices || !faces || !tri_mesh) return rtx_fail(RTX_E_ARG, "null mesh arrays (vertices, faces, tri_mesh)");
  if (!header || !table) return rtx_fail(RTX_E_ARG, "null skeleton (header, table)");
  if (!workspace) return rtx_fail(RTX_E_ARG, "null workspace pointer");
  if ((normals == nullptr) != (mesh_smooth == nullptr))
    return rtx_fail(RTX_E_ARG, "normals and mesh_smooth are given together or not at all");
  if (n_triangles < 1 || n_triangles > RTX_MAX_TRIANGLES)
    return rtx_fail(RTX_E_ARG, "n_triangles out of range (1..%d)", (int)RTX_MAX_TRIANGLES);
  if (n_vertices < 1 || n_vertices > INT32_MAX) return rtx_fail(RTX_E_ARG, "n_vertices out of range (1..2^31 - 1)");
  if (max_leaf < 0) return rtx_fail(RTX_E_ARG, "max_leaf must be positive, or 0 for one leaf");
  // the header: a mesh table's, of these triangles, its parts within table_words
  const double T = header[RTX_MH_NTRI], M = header[RTX_MH_NMESH], N = header[RTX_MH_NNODES];
  const double ta = header[RTX_MH_TRIS], ma = header[RTX_MH_MATS], na = header[RTX_MH_NODES], w = header[RTX_MH_WORDS];
  const double ua = header[RTX_MH_UVS], xa = header[RTX_MH_TEXELS];
  if (!(header[RTX_MH_MAGIC] == RTX_MESH_MAGIC && T == (double)n_triangles && M >= 1 && M <= T && N >= 1 && N <= 2 * T))
    return rtx_fail(RTX_E_ARG, "the skeleton's header is not that of a mesh table of %lld triangles",
                    (long long)n_triangles);
  if (table_words < RTX_MESH_HDR_WORDS || table_words > INT32_MAX || !(w <= (double)table_words))
    return rtx_fail(RTX_E_ARG, "the skeleton has %lld words, fewer than its header says (or more than 2^31 - 1)",
                    (long long)table_words);
  const bool parts = ta >= RTX_MESH_HDR_WORDS && ta + T * RTX_TRI_WORDS <= w && ma >= RTX_MESH_HDR_WORDS &&
                     ma + M * RTX_MAT_WORDS <= w && na >= RTX_MESH_HDR_WORDS && na + N * RTX_NODE_WORDS <= w &&
                     ta == floor(ta) && na == floor(na);
  const bool uv_part = ua != 0 || xa != 0;
  if (!parts || (uv_part && !(ua >= RTX_MESH_HDR_WORDS && ua == floor(ua) && ua + T * RTX_UV_WORDS <= w)))
    return rtx_fail(RTX_E_ARG, "the skeleton's header: the counts and offsets do not fit its %lld words",
                    (long long)table_words);
  int64_t nodes = 0;
  int levels = 0;
  tree_shape(n_triangles, max_leaf, nodes, levels);
  if ((double)nodes != N)
    return rtx_fail(RTX_E_ARG, "the skeleton has %lld nodes; the tree of %lld triangles with max_leaf %d has %lld",
                    (long long)N, (long long)n_triangles, max_leaf, (long long)nodes);
  const size_t need = rtx_mesh_build_workspace_bytes(n_triangles, nodes);
  if (workspace_bytes < need)
    return rtx_fail(RTX_E_ARG, "workspace too small: %zu < %zu bytes (rtx_mesh_build_workspace_bytes)", workspace_bytes,
                    need);

  const Layout l = layout(n_triangles, nodes);
  uint8_t* ws = (uint8_t*)workspace;
  BuildParams p{};
  p.verts = vertices, p.faces = faces, p.tri_mesh = tri_mesh, p.normals = normals, p.smooth = mesh_smooth, p.uvs = uvs;
  p.table = table;
  p.n_verts = n_vertices;
  p.tris_at = (int64_t)ta, p.nodes_at = (int64_t)na, p.uvs_at = uv_part ? (int64_t)ua : 0;
  p.T = (int)n_triangles, p.N = (int)nodes, p.M = (int)M, p.leaf = max_leaf > 0 ? max_leaf : (int)n_triangles;
  p.status = (uint32_t*)(ws + l.status);
  p.centre = (double*)(ws + l.centre), p.lo = (double*)(ws + l.lo), p.hi = (double*)(ws + l.hi);
  p.nbox = (u64*)(ws + l.nbox), p.next = (u64*)(ws + l.next);
  p.seg_s = (int32_t*)(ws + l.seg_s), p.seg_e = (int32_t*)(ws + l.seg_e), p.node_of = (int32_t*)(ws + l.node_of);
  p.pos = (int32_t*)(ws + l.pos), p.order = (int32_t*)(ws + l.order), p.iota = (int32_t*)(ws + l.iota);
  p.sorted = (int32_t*)(ws + l.sorted);
  p.key = (u64*)(ws + l.key), p.key_sorted = (u64*)(ws + l.key_sorted);
  p.seg_key = (uint32_t*)(ws + l.seg_key), p.seg_key_sorted = (uint32_t*)(ws + l.seg_key_sorted);
  void* sort_ws = ws + l.sort;
  const size_t sort_have = sort_bytes(n_triangles);
  hipStream_t s = (hipStream_t)stream;
  const unsigned size = (unsigned)p.T;
  unsigned seg_bits = 1;
  while (seg_bits < 32 && ((int64_t)1 << seg_bits) < n_triangles) ++seg_bits;

  if (levels > 0) {  // what rocPRIM asks for, against what the workspace sets aside (no launch)
    size_t a = 0, b = 0;
    hipError_t e = rocprim::radix_sort_pairs((void*)nullptr, a, p.key, p.key_sorted, p.iota, p.sorted, size, 0u, 64u, s);
    if (e == hipSuccess)
      e = rocprim::radix_sort_pairs((void*)nullptr, b, p.seg_key, p.seg_key_sorted, p.sorted, p.order, size, 0u, seg_bits, s);
    if (e != hipSuccess) return rtx_fail(RTX_E_LAUNCH, "rocprim::radix_sort_pairs (size): %s", hipGetErrorString(e));
    if (a > sort_have || b > sort_have)
      return rtx_fail(RTX_E_WORKSPACE, "rocPRIM's sort needs %zu bytes, the workspace sets %zu aside", a > b ? a : b,
                      sort_have);
  }

  const dim3 block(kBlock), grid_t((unsigned)((p.T + kBlock - 1) / kBlock));
  const int64_t init = 6 * nodes > 1 ? 6 * nodes : 1;
  hipLaunchKernelGGL(k_build_init, dim3((unsigned)((init + kBlock - 1) / kBlock)), block, 0, s, p);
  hipLaunchKernelGGL(k_build_rows, grid_t, block, 0, s, p);
  if (const int rc = rtx_launched("k_build_rows")) return rc;
  for (int level = 0; level < levels; ++level) {
    hipLaunchKernelGGL(k_build_keys, grid_t, block, 0, s, p);
    size_t bytes = sort_have;
    hipError_t e = rocprim::radix_sort_pairs(sort_ws, bytes, p.key, p.key_sorted, p.iota, p.sorted, size, 0u, 64u, s);
    if (e != hipSuccess) return rtx_fail(RTX_E_LAUNCH, "rocprim::radix_sort_pairs (keys): %s", hipGetErrorString(e));
    hipLaunchKernelGGL(k_build_seg_keys, grid_t, block, 0, s, p);
    bytes = sort_have;
    e = rocprim::radix_sort_pairs(sort_ws, bytes, p.seg_key, p.seg_key_sorted, p.sorted, p.order, size, 0u, seg_bits, s);
    if (e != hipSuccess) return rtx_fail(RTX_E_LAUNCH, "rocprim::radix_sort_pairs (segments): %s", hipGetErrorString(e));
    hipLaunchKernelGGL(k_build_update, grid_t, block, 0, s, p);
    if (const int rc = rtx_launched("k_build_update")) return rc;
  }
  hipLaunchKernelGGL(k_build_nodes, dim3((unsigned)((p.N + kBlock - 1) / kBlock)), block, 0, s, p);
  hipLaunchKernelGGL(k_build_write, dim3((unsigned)((p.T + kRowBlock - 1) / kRowBlock)), dim3(kRowBlock), 0, s, p);
  return rtx_launched("k_build_write");
}
