/*
 * rtx_hip.h — C ABI of the MI355X (gfx950) render-path library  librtx_hip.so
 *
 * This is the drop-in boundary for the reference's NumPy render backend
 * (/root/reference/ray_tracer/infrastructure/numpy/). Every entry point below replaces one
 * reference interface; the Python host layer (python_ray_tracer_amd/infrastructure/hip/) calls
 * them through ctypes with device pointers owned by torch tensors. Signatures are plain C:
 * pointers, sizes and an opaque stream handle (a hipStream_t) — no torch types.
 *
 *   rtx_render_camera   <- NumpyRenderer.get_ray_directions + NumpyRenderer.raytrace_scene at
 *                          level 0 with the camera origin   (base.py:123-141, base.py:91-121,
 *                          and the recursion through shader.py:63-161), fused; also one row tile
 *                          of the frame for the multi-GPU path (application.py:43-52 gains it)
 *   rtx_trace_rays      <- NumpyRenderer.raytrace_scene(ray_origin, dirs, scene) for an arbitrary
 *                          batch of rays                      (base.py:91-121)
 *   rtx_shade_hits      <- NumpyShader.create (the Shader plugin, shader.py:63-112 / application.py:35-40)
 *   rtx_ray_directions  <- NumpyRenderer.get_ray_directions  (base.py:123-141)
 *   rtx_sphere_intersect<- NumpySphere.intersect             (shape.py:28-51)
 *   rtx_quantize_u8     <- NumpyRenderer.save_image's (255*clip(c,0,1)).astype(uint8)
 *                                                             (base.py:143-151)
 *   rtx_resolve_samples <- no counterpart: the box filter of supersampled anti-aliasing
 *                          (HipRenderer(samples=k)); each sample clipped as save_image clips a pixel
 *   rtx_primary_aovs, rtx_primary_aovs_rays
 *                       <- no counterpart: the primary hit's intermediates as render passes — the
 *                          nearest distance and hit shape of raytrace_scene (base.py:97-103), P, the
 *                          normal and is_in_light of NumpyShader.create (shader.py:73-84) and
 *                          Texture.get_color — which the reference computes and discards
 *   rtx_camera_rays     <- generalises get_ray_directions (base.py:123-141): the rays of a camera with
 *                          a target, an up vector, a field of view and a thin lens (PerspectiveCamera)
 *   rtx_edge_mask, rtx_sample_dirs, rtx_resolve_scatter
 *                       <- no counterpart: adaptive anti-aliasing (HipRenderer(samples=k,
 *                          adaptive=True)): which pixels of a plain frame are edges, the k x k sample
 *                          rays of those pixels, and their resolve written back over the frame
 *   rtx_occlusion       <- no counterpart: ambient occlusion and soft shadows of the primary hit (the
 *                          reference's dome light is unshadowed, shader.py:98, its PointLight a point):
 *                          side x side any-hit rays per hit, each the reference's own sphere test
 *   rtx_trace_glass     <- no counterpart (shader.py:143 "TODO: VOIR TRANSMISSION"): raytrace_scene on
 *                          explicit rays through a scene with solid glass spheres, whose transmitted ray
 *                          is one more level of the recursion, added after the iridescence term
 *   rtx_trace_lights    <- no counterpart (main.py "TODO: use multiple lights", domain.py "class
 *                          PointLight:  # TODO: add intensity"): raytrace_scene on explicit rays with
 *                          every point light of a table, each weighted by intensity * colour
 *   rtx_env_sample, rtx_trace_lights_env, rtx_trace_glass_env
 *                       <- no counterpart (raytrace_scene adds nothing on a miss, base.py:100-121): an
 *                          equirectangular environment map that every ray which meets no shape samples
 *   rtx_mesh_build      <- no counterpart: the table of rtx_trace_mesh (rows, tree, boxes) made on the device
 *   rtx_mesh_aovs       <- no counterpart: rtx_primary_aovs' passes for a scene with triangle meshes, with
 *                          the triangle's number, barycentrics and face normal
 *
 * Conventions
 *  - All array pointers are DEVICE pointers (hipMalloc / torch caching allocator), read-only
 *    unless documented as output. Vectors are structure-of-arrays [3][n] float64, exactly the
 *    x/y/z arrays of the reference's NumpyVector3D. A shared origin (the reference passes the
 *    camera position as Python scalars at level 0) is origin_stride == 0 and 3 doubles.
 *  - Work is enqueued asynchronously on `stream` (hipStream_t; NULL = the null stream); the caller
 *    synchronises. Entry points never allocate and never synchronise, so they can be captured into
 *    a HIP graph (tools/graph_ab.py replays captured frames bit-identical to eager ones; the caller
 *    keeps the graph's buffers alive); replays are no faster than eager launches here.
 *  - Return 0 on success, a negative RTX_E_* code otherwise; rtx_last_error() gives a message
 *    (thread-local). The Python layer raises RuntimeError on non-zero, like TORCH_CHECK would.
 *  - Scene blob: float64 array built by the host packer (scene_pack.py), layout below. It holds
 *    everything the reference reads from Scene3D during a render.
 *  - Arithmetic is IEEE float64 with no contraction (built with -ffp-contract=off), in the
 *    reference's operation order; sin (<= 2 ulp) and pow (x^5, x^2.5 by multiplications and a
 *    square root) are the only operations that are not correctly rounded, as NumPy's SIMD sin and
 *    pow (~1 ulp) are not either.
 */
#ifndef RTX_HIP_H
#define RTX_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RTX_ABI_VERSION 3 /* 2: rtx_resolve_samples; 3: rtx_last_launches, RTX_WS_COUNTER_BYTES */
/* (rtx_primary_aovs*, rtx_edge_mask, rtx_sample_dirs and rtx_resolve_scatter were added to version 3:
 * new symbols only, nothing that existed changed; so were rtx_camera_rays, rtx_occlusion,
 * rtx_trace_glass with rtx_glass_workspace_bytes, and rtx_trace_lights with rtx_lights_workspace_bytes,
 * and rtx_env_sample, rtx_trace_lights_env and rtx_trace_glass_env, rtx_trace_mesh and rtx_trace_mesh_uv with
 * rtx_mesh_workspace_bytes, and rtx_mesh_build with rtx_mesh_build_nodes and rtx_mesh_build_workspace_bytes) */

/* ---- scene blob layout (float64 words) ---- */
enum {
  RTX_HDR_WORDS = 64,  /* header */
  RTX_GEOM_WORDS = 8,  /* per sphere, at RTX_HDR_WORDS + s*RTX_GEOM_WORDS            */
  RTX_MAT_WORDS = 24,  /* per sphere, at RTX_HDR_WORDS + S*RTX_GEOM_WORDS + s*MAT    */
  RTX_MAX_DOMES = 8,
  RTX_MAX_SPHERES = 1024
};

/* header words */
enum {
  RTX_H_MAGIC = 0,   /* RTX_MAGIC */
  RTX_H_NSPH = 1,    /* S */
  RTX_H_CAM = 2,     /* camera position x,y,z (also V target on every level, shader.py:76) */
  RTX_H_LIGHT = 5,   /* scene.lights[0].position (shader.py:75) */
  RTX_H_DOMEC = 8,   /* colour of the LAST DomeLight, white if none (shader.py:237-241) */
  RTX_H_NDOME = 11,  /* number of DomeLights */
  RTX_H_DOMEI = 12,  /* their intensities, scene order (RTX_MAX_DOMES words) */
  RTX_H_XSTART = 20, /* np.linspace(-1, 1, W): start, step, stop, (W > 1) endpoint fix */
  RTX_H_XSTEP = 21,
  RTX_H_XSTOP = 22,
  RTX_H_XFIX = 23,
  RTX_H_YSTART = 24, /* np.linspace(1/ar + .25, -1/ar + .25, H) */
  RTX_H_YSTEP = 25,
  RTX_H_YSTOP = 26,
  RTX_H_YFIX = 27,
  RTX_H_VZ = 28,     /* 0 - camera.z (base.py:141) */
  RTX_H_VZ2 = 29,    /* VZ*VZ */
  RTX_H_W = 30,
  RTX_H_H = 31,
  RTX_H_CAMOO = 32,  /* |camera|^2 = camera.dot(camera) (shape.py:35 with the level-0 origin) */
  /* optional culling hierarchy (RTX_H_NNODES == 0: none, every ray tests every sphere) */
  RTX_H_NNODES = 33, /* bounding-sphere tree nodes, depth-first order                        */
  RTX_H_NALWAYS = 34,/* leading entries of the culled geometry list tested by every ray (huge spheres) */
  RTX_H_NODES = 35,  /* word offset of the node array (RTX_NODE_WORDS each)                 */
  RTX_H_CGEO = 36,   /* word offset of the culled geometry list (S records, RTX_GEOM_WORDS)  */
  RTX_H_TAME = 37,   /* 1: every coordinate (centres, camera) and radius below 2^60 in magnitude, so
                        the fast kernel may use the half-b sphere test (rtx_kernels.hip SphTest); 0: the
                        reference expressions everywhere */
  RTX_H_MAT0 = 38,   /* rtx_shade_hits only: word offset of a material record (RTX_MAT_WORDS) that
                        replaces the shape's own at level 0 — NumpyShader.create called on another
                        shape's shader (shader.py:63-112 reads self.* for the hit, and traces the
                        reflections through the unchanged scene, :152); 0 = none */
  RTX_H_SHGRID = 39, /* optional shadow grid (scenes with a culling tree and at most 128 spheres): word
                        offset of its record, 0 = none. Record: lo x,y,z; 1/cell x,y,z; nx, ny, nz;
                        centre x,y,z and grown radius of the small spheres' bounding ball; then per
                        voxel (x fastest) two 64-bit masks stored as the bits of two doubles: bit j of
                        mask k set unless sphere 64k+j provably cannot shadow (shader.py:126-128 in its
                        any-hit form) a shadow ray whose nudged origin lies in the voxel; last, the
                        huge spheres' mask (rays outside the grid that miss the ball) */
  RTX_H_SINRED = 40, /* 1: every material's thin-film phase (shader.py:208, |phase| <= 10 pi |thickness|)
                        lies in the kernel sine's reduction range (|x| <= 2^20), so no lane needs a
                        range check; 0: checked per wave */
  RTX_H_NBEAM = 41,  /* culled scenes: spheres [NBEAM, S) are all huge (the culling tree's always-tested
                        ones, RTX_H_NALWAYS): the level-0 tile candidates and the reflected-ray beams take
                        them as candidates without a test; 0 = no such tail (older blobs) */
  RTX_H_SBOX = 42,   /* culled scenes of at most 128 spheres: word offset of S records {x lo, x hi, y lo,
                        y hi}, each sphere's image-plane box for this camera: a camera ray through (x, y, 0)
                        outside it provably yields FARAWAY for that sphere (bounds may be infinite);
                        0 = none (the level-0 tile candidates then take the frustum-plane test) */
  RTX_H_CAMREL = 43  /* scenes of up to 5 spheres: RTX_H_CAMREL + 1, the word offset of S records of
                        RTX_CAMREL_WORDS words in scene order, {camera.x - cx, camera.y - cy,
                        camera.z - cz, (RTX_G_C0 >= 0.0) ? 1.0 : 0.0}: the float64 subtractions of the
                        level-0 sphere test (shape.py:33-34 with the camera as the origin) done once per
                        (scene, camera). The table fills the header's spare words up to
                        RTX_HDR_WORDS - 1, so the blob is no longer for it and the header is full; only
                        there do the small-scene kernels read it. A larger scene's table follows
                        everything else in the blob (no kernel reads it yet). 0 = none: the kernels
                        subtract per lane */
};
#define RTX_CAMREL_WORDS 4
#define RTX_MAGIC 5527384.0 /* 'RTX1' */
#define RTX_SHGRID_WORDS 13 /* words of the shadow-grid record before its masks */

/* per-sphere geometry words */
enum {
  RTX_G_CX = 0, RTX_G_CY = 1, RTX_G_CZ = 2,
  RTX_G_CC = 3,    /* abs(position) = C.C                 (shape.py:35)  */
  RTX_G_RR = 4,    /* radius*radius                       (shape.py:36)  */
  RTX_G_INVR = 5,  /* 1.0/radius                          (shader.py:74) */
  RTX_G_C0 = 6,    /* c for the camera origin: ((C.C + O.O) - 2*C.O) - r*r, O = camera */
  RTX_G_IDX = 7    /* scene index of the sphere (culled geometry list only)              */
};

/* culling-tree node words. A node bounds all spheres below it with an axis-aligned box; the tree
 * is stored depth-first with a skip link, so a wave traverses it without a stack. A node is
 * entered when any lane's ray segment may meet the box expanded by the rounding margin of the
 * reference formula (conservative test, see rtx_kernels.hip: a skipped sphere is one the reference
 * formula provably reports as FARAWAY or beyond the current nearest distance); leaves list their
 * spheres as a range of the culled geometry list. */
enum {
  RTX_NODE_WORDS = 12,
  RTX_N_LOX = 0, RTX_N_LOY = 1, RTX_N_LOZ = 2,  /* box minimum */
  RTX_N_HIX = 3, RTX_N_HIY = 4, RTX_N_HIZ = 5,  /* box maximum */
  RTX_N_FIRST = 6,  /* leaf: first culled-geometry entry   */
  RTX_N_COUNT = 7,  /* leaf: sphere count (0: inner node)  */
  RTX_N_SKIP = 8,   /* node index after this subtree        */
  RTX_N_MARGIN = 9  /* 2e-7 * (3 (|Cn|+R)^2 + R^2 + 1), Cn/R: the box's bounding sphere (error budget) */
};

/* per-sphere material words (NumpyShader, shader.py:36-54; derived constants computed on the
 * host in Python with the reference's own expressions) */
enum {
  RTX_M_G = 0,       /* specular_gain                                      */
  RTX_M_DG = 1,      /* diffuse_gain                                       */
  RTX_M_TEX = 2,     /* RTX_TEX_CONST / _CHECKER / _IMAGE                  */
  RTX_M_TR = 3, RTX_M_TG = 4, RTX_M_TB = 5, /* Texture colour; IMAGE: texel table word offset in
                                               the blob, width, height (texels: float64 RGB, row-major) */
  RTX_M_A2 = 6,      /* alpha**2, alpha = specular_roughness**2 (:294-296) */
  RTX_M_A2M1 = 7,    /* alpha**2 - 1                                       */
  RTX_M_1MA2 = 8,    /* 1 - alpha**2                                       */
  RTX_M_F0 = 9,      /* ((ior-1)/(ior+1))**2                     (:290)    */
  RTX_M_1MF0 = 10,   /* 1 - F0                                             */
  RTX_M_IG = 11,     /* iridescence_gain                                   */
  RTX_M_TFW = 12,    /* thin_film_weight                                   */
  RTX_M_TFT = 13,    /* thin_film_thickness                                */
  RTX_M_HS = 14,     /* (thin_film_ior - 1.0)/2.0                (:215)    */
  RTX_M_1MHS = 15,   /* 1.0 - hue_shift                                    */
  RTX_M_ROUGH = 16,  /* specular_roughness (informational)                 */
  RTX_M_REFL = 17,   /* reflection_gain (stored, never read: shader.py:45) */
  RTX_M_IOR = 18,
  RTX_M_TFIOR = 19
};

/* texture kinds (RTX_M_TEX) */
#define RTX_TEX_CONST 0.0   /* Texture: constant colour (shader.py:13-19)                         */
#define RTX_TEX_CHECKER 1.0 /* TextureChecker (shader.py:22-32)                                  */
#define RTX_TEX_IMAGE 2.0   /* ImageTexture: per-point texel of NumpyTexturedSphere's mapping (shape.py:66-79) */
#define RTX_MAX_TEXELS (1 << 20) /* per image texture */

/* output kinds */
enum {
  RTX_OUT_F32_SOA = 0, /* float  [3][n]  unclipped colour                     */
  RTX_OUT_F64_SOA = 1, /* double [3][n]  unclipped colour (reference dtype)   */
  RTX_OUT_U8_HWC = 2   /* uint8  [n][3]  (255*clip(c,0,1)) truncated (base.py:147) */
};

#define RTX_UNBOUNDED (-1)       /* max_bounces: no cap, like the reference recursion */
#define RTX_UNBOUNDED_LEVELS 333 /* ~ Python's recursion limit / 3 frames per level */
#define RTX_FAST_MAX_BOUNCES 6   /* bounce caps served entirely by the register-resident kernel; a
                                    larger or no cap runs it for a few levels and defers the
                                    pixels whose chain goes on to the continuation passes and the
                                    depth-first kernel (caps 7-8 that way: 1.1-1.6x faster than
                                    the 7- and 8-level kernels, which spill) */

/* stats buffer (uint64 words, accumulated with atomics; pass NULL to disable) */
enum {
  RTX_S_PIXELS = 0,   /* rays started at level 0               */
  RTX_S_DEFERRED = 1, /* rays handed to the general (tie/deep) kernel */
  RTX_S_TIES = 2,     /* (ray, level) pairs with >1 nearest shape */
  RTX_S_TESTS = 3,    /* ray-sphere tests executed by live lanes (fast kernel; culling skips most) */
  RTX_S_NODES = 4,    /* culling-node (box) tests executed by live lanes (fast kernel)            */
  RTX_S_TESTS1 = 5,   /* ... of them, the sphere tests of reflected rays' nearest-hit searches (levels >= 1) */
  RTX_S_NODES1 = 6,   /* ... and their node tests (the culling tree's box tests where the beam was not used) */
  RTX_S_BEAMW = 7,    /* reflected-ray searches served by the wave's beam candidates (waves x levels) */
  RTX_S_LEVELS = 64,  /* levels recorded                        */
  RTX_S_RAYS = 8,     /* [8 .. 8+64): rays traced per level     */
  RTX_S_HITS = 72,    /* [72 .. 72+64): shaded hits (= shadow rays) per level */
  RTX_S_WTRACE = 136, /* [136 .. 136+64): waves that traced a level (any lane live), fast kernel */
  RTX_S_WSHADE = 200, /* [200 .. 200+64): waves that shaded a level (any lane hit), fast kernel  */
  RTX_S_BOXES = 264,  /* of RTX_S_NODES, the culling tree's box tests (the rest are frustum-plane, shadow-grid
                         and beam work priced as node tests)                                       */
  RTX_S_BEAMT = 265,  /* reflected-ray beam tests: one per live lane and beam pass (a lane's cone test of one
                         sphere; round 6, counted apart from the node tests they used to be priced as) */
  RTX_S_WORDS = 266
};

/* workspace: status words then deferred-ray list then per-worker frame stacks.
 * The workspace must be zero-filled before its first use; every call leaves the counters zeroed
 * again (no per-call memset). RTX_WS_STATUS flags are sticky: the caller reads and clears them. */
enum {
  RTX_WS_COUNT = 0,    /* uint32: deferred rays            */
  RTX_WS_STATUS = 1,   /* uint32: RTX_ST_* flags           */
  RTX_WS_DONE = 2,     /* uint32: finished blocks of the general kernel (reset by the last one) */
  RTX_WS_COUNT2 = 3,   /* uint32: reserved, always zero (not written since the forward fold) */
  RTX_WS_COUNT3 = 4,   /* uint32: rays deferred by the continuation pass (caps above RTX_FAST_MAX_BOUNCES or none) */
  RTX_WS_HDR_BYTES = 256,
  RTX_WS_COUNTER_BYTES = 4352 /* RTX_WS_HDR_BYTES and the persistent launches' tile-fetch counters behind it: the
                                 prefix that is zero after every call, except the sticky status word */
};
/* RTX_ST_BAD_SCENE: the scene blob's magic or sphere count (RTX_H_NSPH) disagrees with the
 * n_spheres argument; nothing was rendered. RTX_ST_UNRENDERED: a render passed RTX_F_NO_GENERAL
 * but deferred rays (a tie, an image-textured hit): those pixels were left unwritten. */
enum { RTX_ST_STACK_OVERFLOW = 1, RTX_ST_LIST_OVERFLOW = 2, RTX_ST_BAD_SCENE = 4, RTX_ST_UNRENDERED = 8 };

enum {
  RTX_OK = 0,
  RTX_E_ARG = -1,     /* bad argument (null pointer, size, kind)  */
  RTX_E_LAUNCH = -2,  /* HIP launch / runtime error               */
  RTX_E_WORKSPACE = -3, /* workspace too small                    */
  RTX_E_COMM = -4      /* RCCL missing, or an RCCL call failed      */
};

/* Library version (RTX_ABI_VERSION) and the layout constants above, for the host to verify:
 * writes up to n ints: {HDR_WORDS, GEOM_WORDS, MAT_WORDS, MAX_DOMES, S_WORDS, WS_HDR_BYTES,
 * FAST_MAX_BOUNCES, UNBOUNDED_LEVELS}; returns RTX_ABI_VERSION. */
int rtx_abi_version(int* layout, int n);
const char* rtx_last_error(void);

/* Bytes of workspace rtx_render_camera / rtx_trace_rays need for n rays at this bounce cap. */
size_t rtx_workspace_bytes(int64_t n_rays, int max_bounces);

/* Fused primary-ray generation + trace for the camera of `scene` (replaces
 * get_ray_directions + raytrace_scene, base.py:91-141). Renders the local rows of one
 * interleaved row tiling of the frame: local row lr is global row
 *   ((lr / row_block) * n_parts + part) * row_block + lr % row_block,
 * n_local_rows of them (1,1,0 with n_local_rows == height: the whole frame). Output holds
 * n = width * n_local_rows pixels in local row-major order, as out_kind says. */
int rtx_render_camera(const double* scene, int n_spheres, int width, int height,
                      int row_block, int n_parts, int part, int n_local_rows,
                      int max_bounces, void* out, int out_kind,
                      void* workspace, size_t workspace_bytes, uint64_t* stats, void* stream);

/* rtx_render_camera with options for callers that render the same frame repeatedly:
 *  - deferred_out (may be NULL): a device-accessible uint32 (device memory, or mapped host memory)
 *    that receives, in stream order, the number of rays the fast kernel deferred in this launch
 *    (ties, longer chains); written by the general kernel, so it is left untouched when that kernel
 *    is skipped;
 *  - flags RTX_F_NO_GENERAL: for a render whose identical earlier launch (same blob content, tile,
 *    cap) deferred no ray, the general kernel is not launched — nor, for an uncapped render, the
 *    continuation pass — (the render is deterministic, so it defers none again). Passing it for a
 *    render that does defer rays leaves those pixels unwritten and raises the sticky
 *    RTX_ST_UNRENDERED flag (the workspace counters stay clean, so later calls are unaffected). */
#define RTX_F_NO_GENERAL 1u
/* RTX_F_IMAGES: the scene has image-textured spheres (RTX_TEX_IMAGE). A capped render then runs the
 * fast kernel's texturing build, which shades those hits itself (the texel lookup compiled in);
 * without the flag they are deferred to k_render_general like ties (same colours either way; the
 * texturing build costs untextured scenes 3-7%, so it is opt-in). Uncapped renders ignore it. */
#define RTX_F_IMAGES 2u
/* RTX_F_RESERVE(n): a persistent launch (>= 32 spheres, one frame) sizes its grid n blocks below what
 * the device holds at once, leaving room for the kernels of a collective running beside it (the
 * row-tiled frame's RCCL gather of the previous frame: the persistent waves would otherwise hold
 * every slot until they finish). n < 4096. */
#define RTX_F_RESERVE_SHIFT 4
#define RTX_F_RESERVE(n) ((((unsigned)(n)) & 0xFFFu) << RTX_F_RESERVE_SHIFT)
int rtx_render_camera_ex(const double* scene, int n_spheres, int width, int height,
                         int row_block, int n_parts, int part, int n_local_rows,
                         int max_bounces, void* out, int out_kind,
                         void* workspace, size_t workspace_bytes, uint64_t* stats, void* stream,
                         unsigned flags, uint32_t* deferred_out);

/* rtx_render_camera_ex with a run of parts and a dispatch order.
 * part_run >= 1: the local rows of parts part .. part + part_run - 1 of the n_parts interleave as one
 * tile (part_run * row_block rows of every cycle of n_parts * row_block rows; local row lr is global
 * row (lr / (part_run row_block)) n_parts row_block + part row_block + lr % (part_run row_block)),
 * so a rank can take a larger or smaller share of the frame than 1 / n_parts.
 * A camera launch of one frame (or row tile) is
 * dispatched in units: scenes of >= 32 spheres run persistent waves fetching kWaveW x kWaveH (8 x 8)
 * wave tiles from counters; smaller scenes one block tile (4 waves) per block, blocks dispatched in
 * grid order. rtx_sched_tiles gives the number of units; unit t is column t % units_x, row
 * t / units_x counted from the bottom of the (local) frame, and the default order is t = 0, 1, 2, ...
 * (bottom-up rows: the ground and the spheres, whose pixels run long bounce chains, first).
 *  - tile_order (may be NULL): a permutation of the units, the order in which they are handed out.
 *    Longest first shortens the launch's drain, where a few long units (long reflection chains)
 *    would otherwise run alone at its end. Output does not depend on the order.
 *  - tile_cost (may be NULL; zero-filled): receives each unit's render time (s_memrealtime ticks,
 *    100 MHz; a block tile: its slowest wave) in this launch, from which a caller derives the order
 *    of the next identical launch. A recording launch runs the kernel build that carries the
 *    counters (slower; the records stay out of the timed build's registers), so record once. */
int rtx_sched_tiles(int width, int n_local_rows, int n_spheres, int64_t* n_tiles);
int rtx_render_camera_sched(const double* scene, int n_spheres, int width, int height,
                            int row_block, int n_parts, int part, int part_run, int n_local_rows,
                            int max_bounces, void* out, int out_kind,
                            void* workspace, size_t workspace_bytes, uint64_t* stats, void* stream,
                            unsigned flags, uint32_t* deferred_out, const uint32_t* tile_order,
                            uint32_t* tile_cost);

/* Animation / batch driver (the reference renders one frame per
 * render_image_pipeline call, application.py:43-52): n_frames whole frames of one size, sphere
 * count and bounce cap in ONE launch. Frame f reads the blob at scenes + f * scene_stride (words;
 * every blob is self-describing, so frames may differ in camera, spheres and lights) and writes
 * its width*height pixels at out + f * (one frame's output bytes for out_kind). Equivalent to
 * n_frames rtx_render_camera calls of whole frames. Workspace: rtx_workspace_bytes(n_frames *
 * width * height, max_bounces). */
int rtx_render_frames(const double* scenes, int64_t scene_stride, int n_frames, int n_spheres,
                      int width, int height, int max_bounces, void* out, int out_kind,
                      void* workspace, size_t workspace_bytes, uint64_t* stats, void* stream);

/* raytrace_scene(ray_origin, normalized_ray_direction, scene) for n rays (base.py:91-121),
 * including all reflection levels up to max_bounces. origins: [3][n] (origin_stride == n) or one
 * shared origin (origin_stride == 0, 3 doubles); dirs: [3][n]. */
int rtx_trace_rays(const double* scene, int n_spheres, const double* origins, int64_t origin_stride,
                   const double* dirs, int64_t n, int max_bounces, void* out, int out_kind,
                   void* workspace, size_t workspace_bytes, uint64_t* stats, void* stream);

/* NumpyShader.create(shape, scene, ray_origin, dirs, distance, ray_tracer) (shader.py:63-112): the
 * colour of n rays that hit sphere `shape` at distances t[n] — P = O + D*t, shadow, diffuse, dome,
 * specular, iridescence, and the reflection recursion through raytrace_scene up to max_bounces
 * (the reflected rays are level 1; -1 = unbounded). The shape is taken as hit whether or not it is
 * the nearest, as create shades what it is handed. A blob whose RTX_H_MAT0 word is set shades the
 * level-0 hits with that material record instead of the shape's own (create on another shape's
 * shader). Same origins/dirs layout as rtx_trace_rays; out_kind colour or u8; workspace
 * rtx_workspace_bytes(n, max_bounces). */
int rtx_shade_hits(const double* scene, int n_spheres, int shape, const double* origins, int64_t origin_stride,
                   const double* dirs, const double* t, int64_t n, int max_bounces, void* out, int out_kind,
                   void* workspace, size_t workspace_bytes, uint64_t* stats, void* stream);

/* get_ray_directions (base.py:123-141) for the same row tiling: dirs_out [3][width*n_local_rows]. */
int rtx_ray_directions(const double* scene, int width, int height, int row_block, int n_parts,
                       int part, int n_local_rows, double* dirs_out, void* stream);

/* NumpySphere.intersect (shape.py:28-51): t_out[i] = distance or 1e39 (FARAWAY).
 * sphere: RTX_GEOM_WORDS doubles (cx, cy, cz, C.C, r*r, ...). */
int rtx_sphere_intersect(const double* sphere, const double* origins, int64_t origin_stride,
                         const double* dirs, int64_t n, double* t_out, void* stream);

/* save_image's quantisation (base.py:143-151): color [3][n] (RTX_OUT_F32_SOA or _F64_SOA) ->
 * out [n][3] uint8 = (uint8)(255 * clip(c, 0, 1)). */
int rtx_quantize_u8(const void* color, int color_kind, int64_t n, uint8_t* out, void* stream);

/* Supersampled anti-aliasing, the resolve (HipRenderer(samples=k); the reference renders one
 * sample per pixel): the box filter of a frame rendered with k x k samples per pixel. The screen is
 * fixed (base.py:130-141), so the render of the same scene and camera position at
 * (k*width) x (k*height) holds exactly the k x k samples of every pixel.
 * samples: n_frames x double [3][(k*n_rows) * (k*width)], each as an RTX_OUT_F64_SOA render of a
 * (k*width)-wide frame with k*n_rows local rows wrote it. out: n_frames x (width x n_rows pixels
 * as out_kind says). Per output pixel (r, c) and channel, in float64 and in exactly this order:
 *   acc = 0.0; for sy in 0..k-1 (top to bottom): for sx in 0..k-1 (left to right):
 *     acc = acc + clip(S[k*r + sy][k*c + sx], 0, 1)
 *   value = acc / (double)(k*k)                       (one correctly rounded division)
 * then RTX_OUT_F64_SOA stores value, RTX_OUT_F32_SOA value rounded once, RTX_OUT_U8_HWC
 * (uint8)(255 * value) truncated. Each sample is clipped before it is averaged, as save_image
 * would have clipped that pixel (one sample of 190 would otherwise whiten the whole pixel), so
 * the colour outputs lie in [0, 1] (an unresolved render's colour is unclipped). A NaN sample
 * counts as 0 where np.clip would keep it; no sample of a valid scene is NaN. k = 1 clips and
 * converts. RTX_E_ARG (before any HIP call) for a null pointer, k outside 1..8, a non-positive
 * size, an unknown out_kind, or k*k*width*n_rows*n_frames >= 2^31. */
int rtx_resolve_samples(const double* samples, int k, int width, int n_rows, int n_frames,
                        void* out, int out_kind, void* stream);

/* Primary-hit render passes (HipRenderer.render_aovs / trace_aovs; the reference returns the
 * finished colour only): the intermediates of the level-0 ray of every pixel, each defined by the
 * reference's own expression and computed in float64 in its operation order, without contraction.
 * With distances[s] = shapes[s].intersect(O, D) (shape.py:28-51) over the S shapes in scene order:
 *   depth    double [n]     nearest = reduce(np.minimum, distances) (base.py:98); a miss is exactly
 *                           1e39 (FARAWAY)
 *   id       int32  [n]     the smallest s with distances[s] == nearest where nearest != FARAWAY
 *                           (base.py:102-103); a miss is -1
 *   hits     int32  [n]     how many shapes have distances[s] == nearest: 0 on a miss, more than 1 on
 *                           a tie (the reference shades and sums every one of them, base.py:119)
 *   position double [3][n]  P = O + D * nearest (shader.py:73)
 *   normal   double [3][n]  N = (P - C) * (1.0 / radius) of shape id (shader.py:74; not renormalised,
 *                           and pointing inwards for a negative radius)
 *   albedo   double [3][n]  shapes[id].shader.diffuse_color.get_color(P): the constant colour
 *                           (shader.py:17-19), the checker cell as 1.0 / 0.0 in all three channels
 *                           (shader.py:30-32), or the image texel of NumpyTexturedSphere's mapping
 *                           (shape.py:66-79; atan2 / asin are not correctly rounded on either side, so
 *                           a point within an ulp of a texel edge may take the neighbour texel)
 *   lit      uint8  [n]     is_in_light (shader.py:75-84, 126-128): with L = norm(lights[0] - P) and
 *                           the nudged origin P + N * 0.0001, light_distances[id] ==
 *                           min(light_distances) over all S shapes; 1 or 0
 * On a miss position, normal and albedo are 0.0 and lit is 0. On a tie the per-hit passes (position,
 * normal, albedo, lit) are those of shape id, the first of the tied shapes in scene order. The passes
 * stop at level 0: no reflected ray is traced.
 * Every output pointer may be NULL: that pass is not requested, costs no store, and a call without
 * lit traces no shadow ray, one without albedo looks up no texel. The RTX_AOV_* bits name the passes
 * for the layers above (rt::primary_aovs's `passes` mask; results in bit order).
 * rtx_primary_aovs: the camera rays of one row tile, the tile geometry and local row order of
 * rtx_render_camera_sched (n = width * n_local_rows). rtx_primary_aovs_rays: n explicit rays in the
 * layout of rtx_trace_rays (origin_stride 0 or n).
 * A blob whose magic or sphere count disagrees with n_spheres is traced as an empty scene (every ray
 * a miss). Needs no workspace; asynchronous on `stream`, never allocates, never synchronises.
 * RTX_E_ARG (before any HIP call) for a null scene or null rays, all seven output pointers null,
 * n_spheres outside 1..RTX_MAX_SPHERES, bad tile geometry, an origin_stride other than 0 or n, or a
 * negative n; zero rays return RTX_OK without a launch. */
enum {
  RTX_AOV_DEPTH = 1, RTX_AOV_ID = 2, RTX_AOV_HITS = 4, RTX_AOV_POSITION = 8, RTX_AOV_NORMAL = 16,
  RTX_AOV_ALBEDO = 32, RTX_AOV_LIT = 64, RTX_AOV_ALL = 127
};
int rtx_primary_aovs(const double* scene, int n_spheres, int width, int height,
                     int row_block, int n_parts, int part, int part_run, int n_local_rows,
                     double* depth, int32_t* id, int32_t* hits, double* position, double* normal,
                     double* albedo, uint8_t* lit, void* stream);
int rtx_primary_aovs_rays(const double* scene, int n_spheres, const double* origins, int64_t origin_stride,
                          const double* dirs, int64_t n,
                          double* depth, int32_t* id, int32_t* hits, double* position, double* normal,
                          double* albedo, uint8_t* lit, void* stream);

/* Adaptive anti-aliasing (HipRenderer(samples=k, adaptive=True); the reference renders
 * one sample per pixel): only the edge pixels of a frame get k x k samples. The contract:
 *  1. Base frame. B is the plain float64 render at width x height (unclipped), cb = clip01(B) with a
 *     NaN sent to 0 as the resolve sends it; id, hits and lit are rtx_primary_aovs' passes of the
 *     same frame.
 *  2. Mask (rtx_edge_mask). Pixel p = (r, c) is flagged if hits[p] > 1, or if some neighbour
 *     q = (r + dr, c + dc) inside the frame, dr, dc in {-1, 0, 1} and not both 0, has id[q] != id[p],
 *     or lit[q] != lit[p], or max over the channels of |cb[ch][q] - cb[ch][p]| > contrast. The colour
 *     comparison is strict and in float64; contrast = +inf turns it off. The criterion is symmetric:
 *     both sides of an edge are flagged. A 1 x 1 frame flags only a tie.
 *  3. Samples (rtx_sample_dirs). The flagged pixels are listed in ascending pixel index. Ray
 *     j*k*k + sy*k + sx of listed pixel j = (r, c) is the direction rtx_ray_directions gives pixel
 *     (row k*r + sy, column k*c + sx) of the sample scene: the same scene and camera position with a
 *     (k*width) x (k*height) camera (endpoint fix of the last column and row included). The rays are
 *     traced by rtx_trace_rays from the shared camera origin, as RTX_OUT_F64_SOA, with the render's
 *     bounce cap; its status word is checked as after any render.
 *  4. Output. A flagged pixel is rtx_resolve_samples' value of its k*k samples: each clipped, added
 *     to 0.0 in ray order (top to bottom, left to right), divided once by k*k. An unflagged pixel is
 *     clip01(B[p]) (rtx_resolve_samples with k = 1 on the base frame, written before
 *     rtx_resolve_scatter overwrites the flagged pixels). RTX_OUT_F32_SOA is that value rounded
 *     once, RTX_OUT_U8_HWC (uint8)(255 * value); every output lies in [0, 1].
 *  Known approximation: the base sample of pixel c sits at linspace(.., width)[c], which is not the
 *  centre of its k x k block of linspace(.., k*width).
 * All three entry points are asynchronous on `stream`, never allocate and never synchronise, and
 * return RTX_E_ARG before any HIP call for a null pointer, a non-positive width or height (or
 * width*height >= 2^31), k outside 1..8, an unknown out_kind, a negative or NaN contrast, a negative
 * n_flagged, or n_flagged*k*k >= 2^31. n_flagged == 0 returns RTX_OK without a launch (pixels_i32 may
 * then be NULL).
 * rtx_edge_mask: color_f64 double [3][width*height] (B), id / hits int32 [width*height], lit uint8
 *   [width*height]; mask_out uint8 [width*height], 1 = flagged.
 * rtx_sample_dirs: sample_scene is the packed sample scene (its camera words are read, nothing else);
 *   pixels_i32 int32 [n_flagged] pixel indices r*width + c; dirs_out double [3][n_flagged*k*k]. An
 *   index outside the frame gives a zero direction.
 * rtx_resolve_scatter: samples_f64 double [3][n_flagged*k*k] in the ray order above; writes pixel
 *   pixels_i32[j] of `out` (a whole width x height frame as out_kind says) for every j and nothing
 *   else. The listed pixels must be distinct; an index outside the frame is skipped. */
int rtx_edge_mask(const double* color_f64, const int32_t* id, const int32_t* hits, const uint8_t* lit,
                  int width, int height, double contrast, uint8_t* mask_out, void* stream);
int rtx_sample_dirs(const double* sample_scene, int k, int width, int height, const int32_t* pixels_i32,
                    int n_flagged, double* dirs_out, void* stream);
int rtx_resolve_scatter(const double* samples_f64, int k, const int32_t* pixels_i32, int n_flagged,
                        int width, int height, void* out, int out_kind, void* stream);

/* A perspective camera's ray generator (HipRenderer with a domain.PerspectiveCamera).
 * It generalises get_ray_directions (base.py:123-141: one shared origin in front of a screen fixed at
 * z = 0, looking along +z) to a camera with a position, a target, an up vector, a vertical field of
 * view and a thin lens. The host (python_ray_tracer_amd/camera.py) reduces the camera to six vectors,
 * the camera record: RTX_CAM_WORDS doubles, vector v at cam[RTX_C_v .. RTX_C_v + 2], the rest zero.
 *   EYE  E  = position
 *   FWD  C  = fwd * F            the centre of the plane in focus (F: the focus distance)
 *   U    U  = right * (hw * F)   half its width   (hw = tan(fov / 2) * width / height)
 *   V    V  = tup * (hh * F)     half its height  (hh = tan(fov / 2))
 *   LU   LU = right * lens_radius,  LV = tup * lens_radius   (all zero: a pinhole)
 * The rays of one row tile (the tile geometry and local row order of rtx_render_camera_sched), k x k
 * samples per pixel, n = k*k*width*n_local_rows of them in the order of a sample frame's rows: the ray
 * of local row lr, column c, sample (sy, sx) has index (k*lr + sy) * (k*width) + k*c + sx, which is
 * the layout rtx_resolve_samples reads. With gr the global row of lr, ix = k*c + sx, iy = k*gr + sy,
 * in float64 without contraction and in exactly this order:
 *   iw = 1.0 / (double)(k*width);  ih = 1.0 / (double)(k*height)
 *   u = (double)(2*ix + 1) * iw - 1.0;  v = 1.0 - (double)(2*iy + 1) * ih
 *   h = (uint32)c * 0x9E3779B1u ^ (uint32)gr * 0x85EBCA77u
 *   h ^= h >> 16;  h *= 0x7FEB352Du;  h ^= h >> 15;  h *= 0x846CA68Bu;  h ^= h >> 16
 *   j = ((sy*k + sx) + h % (k*k)) % (k*k)        a per-pixel rotation of the lens table
 *   (a, b) = lens ? (lens[j], lens[k*k + j]) : (0, 0)
 *   off = LU * a + LV * b                        per component: LU.x * a + LV.x * b
 *   origin = E + off
 *   d = ((C + U * u) + V * v) - off              aims at the point of the focus plane behind (u, v)
 *   dir = d * (1.0 / sqrt((d.x*d.x + d.y*d.y) + d.z*d.z))        the reference's norm(), base.py:61-64
 * cam is a HOST pointer, read during the call (the record travels as a kernel argument). lens:
 * device double [2][k*k], the k*k points of the unit disk the samples of a pixel leave through (x
 * plane, then y plane); NULL takes (0, 0) for every sample. origins_out: device double [3][n], or
 * NULL to store no origins; dirs_out: device double [3][n]. A record with a lens (a non-zero word of
 * LU or LV) needs both lens and origins_out; a pinhole's rays share the origin cam[RTX_C_EYE ..].
 * Asynchronous on `stream`, never allocates, never synchronises. RTX_E_ARG (before any HIP call) for
 * a null cam or dirs_out, a non-finite record word, k outside 1..8, bad tile geometry, k*width or
 * k*height at 2^31 or above, n at 2^31 or above, or a missing lens or origins_out when the record has
 * a lens; zero rays return RTX_OK without a launch. */
enum {
  RTX_CAM_WORDS = 24,
  RTX_C_EYE = 0, RTX_C_FWD = 3, RTX_C_U = 6, RTX_C_V = 9, RTX_C_LU = 12, RTX_C_LV = 15
};
int rtx_camera_rays(const double* cam, const double* lens, int k, int width, int height,
                    int row_block, int n_parts, int part, int part_run, int n_local_rows,
                    double* origins_out, double* dirs_out, void* stream);

/* Occlusion passes (HipRenderer.render_occlusion / trace_occlusion; the reference adds
 * its dome light unshadowed, shader.py:98, and its point light has no size): a bundle of side x side
 * any-hit rays from the primary hit of every ray, computed from the id, position and normal passes
 * rtx_primary_aovs* wrote (so independent of the camera kind and of the tiling). float [n] each:
 *   ao        the share of side x side cosine-distributed hemisphere rays that meet no shape nearer
 *             than max_distance; 1.0 on a miss
 *   soft_lit  the share of side x side points on a disk of radius light_radius around lights[0] that
 *             pass the reference's shadow test from this hit; 0.0 on a miss, as lit is
 * All arithmetic is float64 without contraction in the order written. norm is NumpyVector3D.norm
 * (base.py:61-64), intersect is shape.py:28-51 in the reference expressions; division and square root
 * are correctly rounded.
 * Tables, computed on the host (python_ray_tracer_amd/occlusion.py):
 *   table  double [3][side*side]  hemisphere_table(side): rows 0 and 1 are camera.lens_table(side),
 *                                 the concentric image of the stratum centres; row 2 is
 *                                 sqrt(max(0, 1 - (a*a + b*b)))
 *   rot    double [2][64]         rotation_table(): entry r is (cos phi, sin phi), phi = 2 pi (r + 0.5) / 64
 * Per-hit rotation: r depends on the bits of P = position[:, i] only, not on a pixel index (a row
 * tile, an explicit ray and a perspective camera's pixel give the value of the whole frame). With
 * bx, by, bz the uint64 bit patterns of P:
 *   w = bx ^ rotl64(by, 21) ^ rotl64(bz, 42);  x = (uint32)(w ^ (w >> 32))
 *   x ^= x >> 16;  x *= 0x7feb352d;  x ^= x >> 15;  x *= 0x846ca68b;  x ^= x >> 16
 *   r = x & 63;  (cr, sr) = rot[:, r]
 * Frame around a unit vector n (Duff et al., branch-free; |s + n.z| >= 1, no singular direction):
 *   s = copysign(1.0, n.z);  a = -1.0 / (s + n.z);  b = (n.x * n.y) * a
 *   T = (1.0 + ((s * n.x) * n.x) * a,  s * b,  (-s) * n.x)
 *   B = (b,  s + (n.y * n.y) * a,  -n.y)
 * For a ray i with 0 <= id[i] < S (any other id is a miss and reads nothing of the blob), N =
 * normal[:, i], q = P + N * 0.0001 per component (shader.py:77), h = id[i]:
 *   ao: T, B around N. For sample j with (x, y, z) = table[:, j]:
 *     xr = x * cr - y * sr;  yr = x * sr + y * cr
 *     d = norm((T * xr + B * yr) + N * z)                 per component
 *     occluded iff min_s intersect(s, q, d) < max_distance, over all S shapes including the hit's own
 *     ao = (float)((side*side - occluded) / (double)(side*side))
 *   soft_lit: wv = norm(L - P), L = the blob's RTX_H_LIGHT words; T, B around wv. For sample j with
 *   (a, b) = table[0:2, j]:
 *     ar = a * cr - b * sr;  br = a * sr + b * cr
 *     Lj = L + (T * ar + B * br) * light_radius;  l = norm(Lj - P)
 *     lit iff intersect(h, q, l) == min_s intersect(s, q, l)   (shader.py:126-128, the reference's own
 *                                                               test, which does not stop at the light)
 *     soft_lit = (float)(lit_count / (double)(side*side))
 *   With light_radius = 0 every sample is the reference's shadow ray: soft_lit == lit exactly.
 * A blob whose magic or sphere count disagrees with n_spheres makes every ray a miss, as in
 * rtx_primary_aovs. Either output may be NULL: that pass is then neither computed nor stored.
 * Asynchronous on `stream`; needs no workspace, never allocates, never synchronises. RTX_E_ARG (before
 * any HIP call) for a null scene, id, position, normal, table or rot, both outputs null, n_spheres
 * outside 1..RTX_MAX_SPHERES, side outside 1..8, a negative n, a max_distance outside (0, 1e39] or
 * NaN, or a light_radius that is negative or not finite; n == 0 returns RTX_OK without a launch. */
enum { RTX_OCC_AO = 1, RTX_OCC_SOFT = 2, RTX_OCC_ALL = 3 };
int rtx_occlusion(const double* scene, int n_spheres, const int32_t* id, const double* position,
                  const double* normal, int64_t n, const double* table, int side, const double* rot,
                  double max_distance, double light_radius, float* ao, float* soft_lit, void* stream);

/* Transmission (HipRenderer on a scene with a transmissive sphere; the reference marks
 * the spot, shader.py:143 "TODO: VOIR TRANSMISSION", and stores specular_ior = 1.5 "for glass",
 * shader.py:51): NumpyRenderer.raytrace_scene (base.py:91-121) on n explicit rays, where
 * NumpyShader.create adds one more term after the iridescence (shader.py:110),
 *     color += transmission * transmission_gain        for every hit, lit or not
 * with transmission = raytrace_scene(O', D', scene) one level deeper, traced only where the reflected
 * ray could be (level < max_bounces). `glass` is double [2][n_spheres]: row 0 the transmission_gain
 * of every sphere (finite, >= 0; 0: opaque, the sphere is shaded as before), row 1 its specular_ior
 * (finite, >= 1 where the gain is not 0); it is not part of the scene blob.
 * A glass sphere is solid: a ray that meets it from outside is refracted in, crosses the ball and is
 * refracted out. There are no hits from inside, no internal reflections and no total internal
 * reflection (by the ball's symmetry the exit angle is the entry angle); shapes overlapping the ball
 * are ignored along the passage; a ray that meets the surface from inside (D.n >= 0) gets no
 * transmitted ray. The shadow test is unchanged: a glass ball casts a full shadow.
 * For a hit of sphere (C, r, ior) by the ray (O, D) at distance t, float64 in this order exactly, no
 * contraction, division and square root correctly rounded, norm NumpyVector3D.norm (base.py:61-64),
 * dot products (x*x' + y*y') + z*z' (base.py:34-35), vector expressions per component:
 *     P = O + D*t;  n = (P - C) * (1.0/r)                          (shader.py:73-74)
 *     c = D.n;  transmit only if c < 0
 *     eta = 1.0/ior;  ci = -c;  k = 1.0 - (eta*eta)*(1.0 - ci*ci);  f = eta*ci - sqrt(k)
 *     T = norm(D*eta + n*f)                                         the ray inside the ball
 *     m = P - C;  b = T.m;  E = P - T*(2*b)                         the exit point
 *     u = (E - C) * (1.0/r);  ce = T.u
 *     ke = max(1.0 - (ior*ior)*(1.0 - ce*ce), 0.0);  g = sqrt(ke) - ior*ce
 *     O' = E + u*0.0001;  D' = norm(T*ior + u*g)
 * Which rays exist, what they hit (the nearest shape, ties, base.py:102-119) and is_in_light are the
 * reference's decisions bit for bit. A pixel's colour is the sum over its tree of shaded hits of
 * weight * (the hit's colour with a black reflection), the weight (w*0.5)*g down a reflection
 * (shader.py:106) and w*transmission_gain down a transmission: the terms of the reference's nested
 * sum, reassociated (a few ulp of the colour, as in every render kernel here).
 * One lane per ray; each lane keeps a stack of 4*max_bounces + 4 pending rays in the workspace (a ray
 * tree without ties needs max_bounces + 1). A lane that would need more drops the ray and sets
 * RTX_ST_STACK_OVERFLOW in the workspace's RTX_WS_STATUS word (sticky: the caller reads and clears
 * it). The workspace is RTX_WS_HDR_BYTES of header, zeroed once by the caller, and the stacks of a
 * bounded pool of workers: rtx_glass_workspace_bytes(n, max_bounces) does not grow with n beyond that
 * pool (0 for arguments rtx_trace_glass refuses).
 * out / out_kind as rtx_trace_rays (RTX_OUT_*; uint8 [n][3]). A blob whose magic or sphere count
 * disagrees with n_spheres makes every ray a miss (colour 0). Asynchronous on `stream`, never
 * allocates, never synchronises. RTX_E_ARG (before any HIP call) for a null scene, glass, origins,
 * dirs, out or workspace, n_spheres outside 1..RTX_MAX_SPHERES, max_bounces outside
 * 0..RTX_GLASS_MAX_BOUNCES (the tree has up to 2^(max_bounces+1) rays per pixel: no unbounded form),
 * a bad out_kind, a negative n or an origin_stride other than 0 or n; RTX_E_WORKSPACE for a workspace
 * that is too small; n == 0 returns RTX_OK without a launch. */
enum { RTX_GLASS_MAX_BOUNCES = 8 };
size_t rtx_glass_workspace_bytes(int64_t n_rays, int max_bounces);
int rtx_trace_glass(const double* scene, int n_spheres, const double* glass, const double* origins,
                    int64_t origin_stride, const double* dirs, int64_t n, int max_bounces, void* out,
                    int out_kind, void* workspace, size_t workspace_bytes, void* stream);

/* Several point lights with intensity and colour (HipRenderer on a scene whose lights hold a
 * domain.ColoredPointLight; the reference lights with scene.lights[0] alone, white and
 * of strength 1: main.py "TODO: use multiple lights", domain.py "class PointLight:  # TODO: add
 * intensity"): NumpyRenderer.raytrace_scene (base.py:91-121) on n explicit rays, where
 * NumpyShader.create (shader.py:63-112) sums its light-dependent terms over the rows of `lights`,
 * double [n_lights][6]: row i is (px, py, pz, e_r, e_g, e_b) with e = intensity * colour per channel
 * (finite, >= 0), in scene.lights order; it is not part of the scene blob, whose own light
 * (RTX_H_LIGHT) this entry does not read.
 * For a hit with point P, normal N and nudged point Q (shader.py:73-77), float64 in this order
 * exactly, no contraction, for each light i in table order:
 *     L_i   = norm(pos_i - P)                                              (shader.py:75)
 *     lit_i = the shadow test along L_i from Q (shader.py:126-128) in its any-hit form: no shape is
 *             strictly nearer than the hit shape's own distance
 *     dli_i = max(N.L_i, 0)                                                (shader.py:138)
 *     spec_i = _calculate_physical_specular with L_i (shader.py:246-320), evaluated only where lit_i
 *              and g != 0 (g: specular_gain)
 * and per channel c, with tex the texture's colour, dg the diffuse gain, R the reflected colour one
 * level deeper, dome and irid the reference's dome-light and iridescence terms (unweighted):
 *     diffuse[c] = sum_i (((tex[c]*dli_i)*lit_i)*dg)*e_i[c]
 *     glossy[c]  = sum_i (((spec_i + R[c]*0.5)*g)*lit_i)*e_i[c]
 *     colour[c]  = (((0.004 + diffuse[c]) + dome[c]) + glossy[c]) + irid[c]
 * both sums from 0.0 in table order. The reflected ray is traced only if the level is below
 * max_bounces, g != 0 and some channel of sum_i lit_i*e_i is not 0 (a reflection that is multiplied
 * by zero is not traced). With one light of e = (1, 1, 1) every added factor is a multiplication by
 * 1.0 and the colour is the reference's create exactly. Which rays exist, what they hit (the nearest
 * shape; ties are shaded in scene order, base.py:102-119) and every lit_i are the reference's
 * decisions bit for bit. A pixel's colour is the sum over its ray tree of W[c] * (the hit's colour
 * with R = 0), the weight ((W[c]*0.5)*g) * sum_i lit_i*e_i[c] down a reflection: the terms of the
 * nested sum, reassociated (a few ulp of the colour, as in every render kernel here).
 * The shadow test walks the culling tree where the scene has one; the light-space shadow grid is
 * built for lights[0] only and is not used.
 * One lane per ray; each lane keeps a stack of 2*max_bounces + 2 pending rays (10 words each:
 * origin, direction, RGB weight, level) in the workspace. A hit pushes at most one ray, so a chain
 * needs 1 entry, a tree whose every ray meets two shapes at the nearest distance max_bounces + 1 and
 * one of three shapes 2*max_bounces + 1. A lane that would need more drops the ray and sets
 * RTX_ST_STACK_OVERFLOW in the workspace's RTX_WS_STATUS word (sticky: the caller reads and clears
 * it); nothing is written out of bounds. The workspace is RTX_WS_HDR_BYTES of header, zeroed once by
 * the caller, and the stacks of a bounded pool of workers: rtx_lights_workspace_bytes(n, max_bounces)
 * does not grow with n beyond that pool (0 for arguments rtx_trace_lights refuses).
 * out / out_kind as rtx_trace_rays (RTX_OUT_*; uint8 [n][3]). A blob whose magic or sphere count
 * disagrees with n_spheres makes every ray a miss (colour 0). Asynchronous on `stream`, never
 * allocates, never synchronises. RTX_E_ARG (before any HIP call) for a null scene, lights, origins,
 * dirs, out or workspace, n_spheres outside 1..RTX_MAX_SPHERES, n_lights outside
 * 1..RTX_MAX_POINT_LIGHTS, max_bounces outside 0..RTX_LIGHTS_MAX_BOUNCES, a bad out_kind, a negative
 * n or an origin_stride other than 0 or n; RTX_E_WORKSPACE for a workspace that is too small; n == 0
 * returns RTX_OK without a launch. */
enum { RTX_MAX_POINT_LIGHTS = 8, RTX_LIGHTS_MAX_BOUNCES = 16 };
size_t rtx_lights_workspace_bytes(int64_t n_rays, int max_bounces);
int rtx_trace_lights(const double* scene, int n_spheres, const double* lights, int n_lights,
                     const double* origins, int64_t origin_stride, const double* dirs, int64_t n,
                     int max_bounces, void* out, int out_kind, void* workspace, size_t workspace_bytes,
                     void* stream);

/* An environment map (HipRenderer on a scene whose lights hold a domain.EnvironmentLight; DESIGN.md
 * §16; the reference's raytrace_scene starts from black and adds nothing on a miss, base.py:100-121,
 * and its render settings carry a "background" image that nothing reads): raytrace_scene(O, D) of a
 * ray whose nearest distance is FARAWAY returns env(D) instead of black, at every level: camera rays,
 * reflected rays and rays that leave a glass ball. Nothing else changes: the reflected colour still
 * carries * 0.5 * g * lit (shader.py:106), a ray that is not traced (at the cap, unlit, g == 0) still
 * contributes nothing, and the dome light, the shadows and the passes do not see the environment.
 * The image is `texels`, float [height][width][4] on the device (RGB and a zero word; values above 1
 * are allowed: an HDR sky), 16-byte aligned, at most RTX_ENV_MAX_TEXELS texels, equirectangular: column
 * by longitude about +y, row 0 at the zenith. gain[c] = intensity * colour[c] and turn = rotation / 360
 * (rotation in degrees about +y) are computed by the host in float64. rtx_env_t is read on the host at
 * the call; only `texels` must stay alive until the work has run.
 * env(D), float64 in this order exactly, no contraction, texels t converted from float32 exactly,
 * atan2 and asin the device library's (a few ulp, like NumPy's):
 *     u = 0.5 + atan2(D.z, D.x) / (2 pi) + turn;   u = u - floor(u)
 *     v = 0.5 - asin(min(max(D.y, -1), 1)) / pi
 *     x = u*W - 0.5;  i0 = floor(x);  fx = x - i0;  i1 = (i0 + 1) mod W;  i0 = i0 mod W     (wraps)
 *     y = v*H - 0.5;  j0 = floor(y);  fy = y - j0;  j1 = clamp(j0 + 1, 0, H-1);  j0 = clamp(j0, 0, H-1)
 *     top = t[j0][i0]*(1 - fx) + t[j0][i1]*fx;   bot = t[j1][i0]*(1 - fx) + t[j1][i1]*fx
 *     env[c] = (top*(1 - fy) + bot*fy) * gain[c]
 * (min / max propagate a NaN, as NumPy's do.) If u or v is not finite, env = (0, 0, 0). The lookup is
 * bilinear so that it is continuous in u and v, across the seam and across texel boundaries: the few
 * ulp between the device's atan2 / asin and NumPy's move a colour by about as much, not by a texel.
 * rtx_env_sample: out[c][i] = env(dirs[.][i])[c] for n directions, both double [3][n], one lane per
 * direction: the lookup alone (a background plate; tests).
 * rtx_trace_lights_env / rtx_trace_glass_env: rtx_trace_lights / rtx_trace_glass, arguments, workspace
 * (rtx_lights_workspace_bytes / rtx_glass_workspace_bytes), stacks, status word and errors unchanged,
 * where a popped ray that meets no shape adds W[c] * env(D)[c] to its pixel's sum (W: the forward-folded
 * weight of that ray, per channel in the lights kernel), by the kernel's own kind of sum (multiply and
 * add in the lights kernel, one fused multiply-add in the glass kernel, as their hits). A blob whose
 * magic or sphere count disagrees with n_spheres makes every ray a miss: every ray then returns env(D).
 * RTX_E_ARG (before any HIP call) additionally for a null env or texels, width or height < 1, more than
 * RTX_ENV_MAX_TEXELS texels, a texel pointer that is not 16-byte aligned, a gain or turn that is not
 * finite; rtx_env_sample also for a null dirs or out or a negative n. n == 0 returns RTX_OK without a
 * launch. */
enum { RTX_ENV_MAX_TEXELS = 1 << 23 };
typedef struct rtx_env_t {
  const float* texels; /* device, [height][width][4] */
  int width, height;
  double gain[3];
  double turn;
} rtx_env_t;
int rtx_env_sample(const rtx_env_t* env, const double* dirs, int64_t n, double* out, void* stream);
int rtx_trace_lights_env(const double* scene, int n_spheres, const double* lights, int n_lights,
                         const double* origins, int64_t origin_stride, const double* dirs, int64_t n,
                         int max_bounces, void* out, int out_kind, void* workspace, size_t workspace_bytes,
                         void* stream, const rtx_env_t* env);
int rtx_trace_glass_env(const double* scene, int n_spheres, const double* glass, const double* origins,
                        int64_t origin_stride, const double* dirs, int64_t n, int max_bounces, void* out,
                        int out_kind, void* workspace, size_t workspace_bytes, void* stream,
                        const rtx_env_t* env);

/* Triangle meshes (HipRenderer on a scene whose shapes hold a domain.TriangleMesh; the
 * reference's Shape is an ABC with one subclass, the sphere, domain.py:43-50):
 * NumpyRenderer.raytrace_scene (base.py:91-121) on n explicit rays through the spheres of `scene`
 * (n_spheres may be 0) and the triangles of `mesh`, lit by the rows of `lights` as rtx_trace_lights
 * lights its spheres (the same table, the same sums per hit).
 * The triangle test is Möller–Trumbore, two-sided, float64 in this order exactly, no contraction, with
 * dot(a, b) = (a.x*b.x + a.y*b.y) + a.z*b.z, cross(a, b) = (a.y*b.z - a.z*b.y, a.z*b.x - a.x*b.z,
 * a.x*b.y - a.y*b.x), and the triangle's v0, e1 = v1 - v0, e2 = v2 - v0 computed by the host:
 *     T = O - v0;  P = cross(D, e2);  det = dot(e1, P);  f = 1.0 / det     (one division, correctly
 *     u = f * dot(T, P);  Q = cross(T, e1);  v = f * dot(D, Q);  t = f * dot(e2, Q)          rounded)
 *     hit  <=>  det != 0  and  u >= 0  and  v >= 0  and  u + v <= 1  and  0 < t  and  t < FARAWAY
 * every comparison positive, so a NaN or an infinity from a tiny det is a miss; so are a ray in the
 * triangle's plane (det == 0) and one that starts on it (t == 0).
 * All triangles of a scene form one group, numbered in scene order, then face order (RTX_T_NUM). The
 * group's hit is the triangle at the smallest t, the lowest number among equal t: triangles that
 * share an edge or coincide never shade twice, and two coincident meshes do not add (unlike the
 * reference's rule per Shape, base.py:97-103, which the spheres keep: every sphere at the nearest
 * distance shades). If the group's t equals the spheres' nearest distance it shades too, after the
 * spheres.
 * For a triangle's hit at P = O + D*t (shader.py:73): N_g is the row's unit face normal, negated if
 * dot(N_g, D) > 0 (it opposes the ray); the shading normal N is N_g for a flat row and, for a row with
 * vertex normals, norm(((1 - u) - v)*n0 + u*n1 + v*n2) (u, v of the test above; each component (w*n0 +
 * u*n1) + v*n2), negated if dot(N, N_g) < 0; the nudged point is Q = P + N_g*0.0001 (shader.py:77 with
 * the face normal). Everything else of NumpyShader.create uses N as it uses a sphere's normal
 * (diffuse, specular, iridescence, dome, the reflected direction), V towards the camera, the material
 * the mesh's row; a checker reads P.x and P.z (shader.py:29-32).
 * Shadows, per light, along L from Q, unbounded (the ray does not stop at the light, as in the
 * reference): a sphere's hit is lit unless a sphere or a triangle is strictly nearer than the
 * sphere's own distance t_self (shader.py:126-128 with the triangles taking part); a triangle's hit is
 * lit unless any sphere or triangle, those of its own mesh included, has a hit along L (t_self =
 * FARAWAY).
 * `mesh` is the table of python_ray_tracer_amd.meshes.mesh_table, double [mesh_words]: a header of
 * RTX_MESH_HDR_WORDS words (RTX_MH_*: the magic, the counts of triangles, meshes and nodes, the word
 * offsets of the three parts, the table's length), the triangle rows (RTX_TRI_WORDS each, RTX_T_*) in
 * the tree's leaf order, one material row (RTX_MAT_WORDS, RTX_M_*) per mesh, and the nodes of a
 * bounding-volume tree over the triangles in depth-first order (RTX_NODE_WORDS, RTX_N_*: the box, a
 * leaf's first row and count, the skip link, the margin the box is expanded by). The walk is stackless
 * and wave-uniform: a node is entered when any lane may hit it before its nearest distance so far.
 * A header whose magic, counts or offsets do not fit mesh_words means no triangles; a skip link that
 * does not move forward is stepped over and a leaf's range is clamped to the rows, so no table makes
 * the kernel read outside it or loop.
 * Stacks, workspace (rtx_mesh_workspace_bytes), status word, out / out_kind, asynchrony and errors as
 * rtx_trace_lights, with n_spheres in 0..RTX_MAX_SPHERES, max_bounces in 0..RTX_MESH_MAX_BOUNCES, and
 * RTX_E_ARG also for a null mesh and for mesh_words below RTX_MESH_HDR_WORDS or above 2^31 - 1. */
enum { RTX_MAX_TRIANGLES = 1 << 20, RTX_MESH_MAX_BOUNCES = 16, RTX_MESH_HDR_WORDS = 16, RTX_TRI_WORDS = 24 };
#define RTX_MESH_MAGIC 1296388936.0
enum { RTX_MH_MAGIC = 0, RTX_MH_NTRI, RTX_MH_NMESH, RTX_MH_NNODES, RTX_MH_TRIS, RTX_MH_MATS, RTX_MH_NODES, RTX_MH_WORDS };
enum {
  RTX_T_V0 = 0,      /* 3 words each: v0, e1, e2, the unit face normal */
  RTX_T_E1 = 3,
  RTX_T_E2 = 6,
  RTX_T_NG = 9,
  RTX_T_MESH = 12,   /* the mesh (its material row) */
  RTX_T_SMOOTH = 13, /* 1: the row has vertex normals */
  RTX_T_N0 = 14,     /* 3 words each: the normals at v0, v1, v2 */
  RTX_T_N1 = 17,
  RTX_T_N2 = 20,
  RTX_T_NUM = 23     /* the triangle's number in the group */
};
size_t rtx_mesh_workspace_bytes(int64_t n_rays, int max_bounces);
int rtx_trace_mesh(const double* scene, int n_spheres, const double* mesh, int64_t mesh_words, const double* lights,
                   int n_lights, const double* origins, int64_t origin_stride, const double* dirs, int64_t n,
                   int max_bounces, void* out, int out_kind, void* workspace, size_t workspace_bytes, void* stream);

/* Texture coordinates and image textures on meshes (a TriangleMesh with `uvs` whose texture is an
 * ImageTexture): rtx_trace_mesh_uv is rtx_trace_mesh, arguments and errors alike, on a table
 * with two more parts after the nodes, their word offsets in the header words RTX_MH_UVS and RTX_MH_TEXELS
 * (0 in a table without them, which rtx_trace_mesh renders as before; the host chooses the entry):
 *   the UV part, RTX_UV_WORDS words per triangle row in the rows' leaf order, row k's at uvs + 6k:
 *     s0 t0 s1 t1 s2 t2, the texture coordinates at v0, v1, v2 (zeros for a mesh without any);
 *   the texel part, from RTX_MH_TEXELS to the table's end: one block per distinct image, float64 RGB,
 *     row-major, row 0 the top of the image.
 * The material row of an image-textured mesh is RTX_TEX_IMAGE with RTX_M_TR / TG / TB the block's word
 * offset in the mesh table, the width W and the height H (the sphere record's meaning, the mesh table in
 * the blob's place; W * H <= RTX_MAX_TEXELS). At a triangle's hit, with u, v of the triangle test above,
 * the texture's colour is, per channel c, float64 in this order exactly, no contraction:
 *     w0 = (1 - u) - v
 *     s  = (w0*s0 + u*s1) + v*s2;  t = (w0*t0 + u*t1) + v*t2
 *     x  = s*W - 0.5;  y = (1 - t)*H - 0.5                    (t = 0 is the image's bottom row, as in OBJ)
 *     x0 = floor(x);  fx = x - x0;  y0 = floor(y);  fy = y - y0
 *     i0 = x0 - W*floor(x0 / W);  i1 = (i0 + 1 == W) ? 0 : i0 + 1       (repeat; one correctly rounded
 *     j0 = y0 - H*floor(y0 / H);  j1 = (j0 + 1 == H) ? 0 : j0 + 1        division per axis)
 *     gx = 1 - fx;  gy = 1 - fy
 *     c  = (c[j0][i0]*gx + c[j0][i1]*fx)*gy + (c[j1][i0]*gx + c[j1][i1]*fx)*fy
 * It replaces the constant (tr, tg, tb) of that hit; everything after it is rtx_trace_mesh's text. The
 * host refuses coordinates with |s| or |t| above RTX_MESH_UV_MAX, so x0, y0 and the wrapped indices are
 * exact integers below 2^31. A sphere with an ImageTexture keeps reading the scene blob (image_texel).
 * No table makes the kernel read outside it: UV or texel offsets that do not fit mesh_words, or a
 * material whose block does not lie in the texel part, mean "no image" and the colour is black (the
 * row's TR / TG / TB words are not a colour); a wrapped index outside its axis (coordinates beyond the
 * host's limit) reads index 0. */
enum { RTX_MH_UVS = 8, RTX_MH_TEXELS = 9, RTX_UV_WORDS = 6, RTX_MESH_UV_MAX = 1024 };
int rtx_trace_mesh_uv(const double* scene, int n_spheres, const double* mesh, int64_t mesh_words,
                      const double* lights, int n_lights, const double* origins, int64_t origin_stride,
                      const double* dirs, int64_t n, int max_bounces, void* out, int out_kind, void* workspace,
                      size_t workspace_bytes, void* stream);

/* The mesh table made on the device (HipRenderer.mesh_build = "device"): rtx_mesh_build fills
 * a skeleton of the table of rtx_trace_mesh / rtx_trace_mesh_uv from the meshes' raw arrays. The contract is
 * the host's table: after the call `table` holds, word for word, the float64 values of
 * python_ray_tracer_amd.meshes.mesh_table for the same meshes and max_leaf (only the sign of a zero is
 * free), so the tree, its margins and every frame rendered from it are the host-built table's.
 * Inputs, all on the device: `vertices` double [n_vertices][3], the meshes' vertices one after the other;
 * `faces` int32 [n_triangles][3], indices into `vertices` (each mesh's already offset by its vertex base),
 * the triangles in group order; `tri_mesh` int32 [n_triangles], each triangle's mesh; `normals` double
 * [n_vertices][3] and `mesh_smooth` int32 [n_meshes] (1: the mesh has vertex normals), both null when no
 * mesh is smooth; `uvs` double [n_triangles][RTX_UV_WORDS] per corner, or null (zeros).
 * `table`, double [table_words] on the device, is the skeleton (meshes.device_inputs): the header, the
 * material rows, every node's first, count and skip (they depend on n_triangles and max_leaf alone) and the
 * texel blocks; `header` is a HOST copy of its first RTX_MESH_HDR_WORDS words, read at the call. The call
 * writes the triangle rows in leaf order, the nodes' boxes and margins and, where the header names a UV
 * part, that part. The arithmetic is meshes.triangle_rows' and mesh_table_entry's, float64 without
 * contraction: e1 = v1 - v0, e2 = v2 - v0, N_g = cross(e1, e2) / sqrt((x*x + y*y) + z*z); a triangle's box
 * is min / max of v0, v0 + e1, v0 + e2, its centre (lo + hi) * 0.5; a level sorts every segment longer than
 * max_leaf by its centres along the first largest extent, ties by the triangle's number (-0.0 equals 0.0),
 * and cuts it at s + (len + 1) / 2; a node's margin is 2e-7 * (1 + ((mx*mx + my*my) + mz*mz)), m the larger
 * of |lo| and |hi| per axis. The sorts are rocPRIM's stable device radix sort over the workspace.
 * max_leaf: the most triangles of a leaf, 0 for one leaf. rtx_mesh_build_nodes(n_triangles, max_leaf) is
 * that tree's node count (0 for arguments out of range); rtx_mesh_build_workspace_bytes(n_triangles, n_nodes)
 * the workspace (0 for n_triangles outside 1..RTX_MAX_TRIANGLES or n_nodes outside 1..2 n_triangles). The
 * workspace needs no initialisation. Its first two uint32 words are the build's status, written by the
 * call: word 0 the lowest number of a triangle whose normal cannot be normalised (RTX_MB_NONE: none; the
 * table is then not to be used), word 1 non-zero if a face index or mesh number was out of range (it was
 * read as 0; nothing is read or written out of bounds).
 * Asynchronous on `stream`, never allocates, never synchronises. RTX_E_ARG (before any HIP call) for a null
 * vertices, faces, tri_mesh, header, table or workspace, normals without mesh_smooth or the reverse,
 * n_triangles outside 1..RTX_MAX_TRIANGLES, n_vertices outside 1..2^31 - 1, a negative max_leaf, a header
 * that is not a mesh table's of n_triangles triangles and rtx_mesh_build_nodes nodes or whose parts do not
 * fit it, table_words below the header's word count (a skeleton shorter than its own header says) or above
 * 2^31 - 1, and a workspace smaller than rtx_mesh_build_workspace_bytes; RTX_E_WORKSPACE if rocPRIM asks
 * for more temporary storage than the workspace sets aside. The call is not part of rtx_last_launches'
 * record, which describes k_render_fast launches only. */
#define RTX_MB_NONE 0xFFFFFFFFu
int64_t rtx_mesh_build_nodes(int64_t n_triangles, int max_leaf);
size_t rtx_mesh_build_workspace_bytes(int64_t n_triangles, int64_t n_nodes);
int rtx_mesh_build(const double* vertices, int64_t n_vertices, const int32_t* faces, const int32_t* tri_mesh,
                   int64_t n_triangles, const double* normals, const int32_t* mesh_smooth, const double* uvs,
                   const double* header, double* table, int64_t table_words, int max_leaf, void* workspace,
                   size_t workspace_bytes, void* stream);

/* Primary-hit render passes of a mesh scene (HipRenderer.render_mesh_aovs / trace_mesh_aovs; DESIGN.md §20;
 * rtx_primary_aovs sees spheres alone): intermediates of rtx_trace_mesh's level-0 hit for n explicit rays
 * (the layout of rtx_trace_rays, origin_stride 0 or n) through the spheres of `scene` (n_spheres may be 0)
 * and the triangle group of `mesh`, written out instead of shaded. Everything is float64 in the operation
 * order rtx_trace_mesh fixes above: the sphere test, the triangle test, P = O + D*t, a sphere's normal
 * (P - C) * (1 / radius), a triangle's N_g, interpolated N and their flips.
 * tmin is the spheres' nearest distance (base.py:98), tt the group's hit (smallest t, lowest RTX_T_NUM among
 * equal t); the ray's nearest is min(tmin, tt). The FIRST HIT is the first sphere in scene order at the
 * nearest distance if there is one, else the triangle: the hit rtx_trace_mesh shades first.
 *   depth            double [n]     the nearest distance; exactly FARAWAY (1e39) on a miss
 *   id               int32  [n]     the first hit's shape: shape_ids[s] for sphere s, shape_ids[n_spheres + mesh]
 *                                   for a triangle of mesh `mesh` (RTX_T_MESH); -1 on a miss
 *   hits             int32  [n]     the spheres at the nearest distance, plus 1 if the group's t equals it;
 *                                   0 on a miss
 *   position         double [3][n]  P = O + D * nearest
 *   normal           double [3][n]  the shading normal N of the first hit: the sphere's, or the triangle's (a flat
 *                                   row: N_g flipped to oppose the ray; a row with vertex normals: the normalised
 *                                   interpolation, flipped to N_g's side)
 *   geometric_normal double [3][n]  a triangle's N_g flipped to oppose the ray; a sphere's normal. position +
 *                                   geometric_normal * 0.0001 is the kernel's nudged point Q (shader.py:77)
 *   albedo           double [3][n]  the texture's colour at the first hit: the constant, the checker cell as
 *                                   1.0 / 0.0, a sphere's image texel (the blob's), a UV-mapped mesh's image
 *                                   colour (the lookup of rtx_trace_mesh_uv above; black for a table without a
 *                                   UV part)
 *   lit              uint8  [n]     bit i: row i of `lights` reaches the first hit under rtx_trace_mesh's shadow
 *                                   rule (along L from Q, nothing strictly nearer than a sphere's own distance;
 *                                   t_self = FARAWAY on a triangle). n_lights <= 8 rows fit the byte; with the
 *                                   one-row table it is 0 / 1 as rtx_primary_aovs' lit
 *   triangle         int32  [n]     the first hit's RTX_T_NUM when it is a triangle; -1 on a sphere or a miss
 *   bary             double [2][n]  (u, v) of that triangle's test, computed again from its row (the same bits
 *                                   as the walk's); 0 on a sphere or a miss
 * On a miss every per-hit pass is 0 and triangle is -1. The passes stop at level 0. Every output pointer may
 * be NULL: that pass is neither computed nor stored; without lit there is no shadow walk, without albedo no
 * texel lookup, without any per-hit pass no hit point. The RTX_MESH_AOV_* bits name the passes for the layers
 * above (rt::mesh_aovs's `passes` mask; results in bit order).
 * shape_ids, int32 [n_spheres + the table's RTX_MH_NMESH] on the device or NULL: what id reports, the
 * spheres' first, then the meshes' in table order (HipRenderer passes each shape's index in scene.shapes);
 * NULL is the identity, s and n_spheres + mesh. Read per lane once, at the hit.
 * A blob whose magic or sphere count disagrees with n_spheres means no spheres, a mesh header that does not
 * fit mesh_words no triangles, as in rtx_trace_mesh. Needs no workspace and has no status word; asynchronous
 * on `stream`, never allocates, never synchronises.
 * RTX_E_ARG (before any HIP call) for a null scene, mesh, lights, origins or dirs, all ten output pointers
 * null, n_spheres outside 0..RTX_MAX_SPHERES, mesh_words outside RTX_MESH_HDR_WORDS..2^31 - 1, n_lights
 * outside 1..RTX_MAX_POINT_LIGHTS, a negative n, or an origin_stride other than 0 or n; zero rays return
 * RTX_OK without a launch. */
enum {
  RTX_MESH_AOV_DEPTH = 1, RTX_MESH_AOV_ID = 2, RTX_MESH_AOV_HITS = 4, RTX_MESH_AOV_POSITION = 8,
  RTX_MESH_AOV_NORMAL = 16, RTX_MESH_AOV_GEOMETRIC_NORMAL = 32, RTX_MESH_AOV_ALBEDO = 64, RTX_MESH_AOV_LIT = 128,
  RTX_MESH_AOV_TRIANGLE = 256, RTX_MESH_AOV_BARY = 512, RTX_MESH_AOV_ALL = 1023
};
int rtx_mesh_aovs(const double* scene, int n_spheres, const double* mesh, int64_t mesh_words, const double* lights,
                  int n_lights, const int32_t* shape_ids, const double* origins, int64_t origin_stride,
                  const double* dirs, int64_t n, double* depth, int32_t* id, int32_t* hits, double* position,
                  double* normal, double* geometric_normal, double* albedo, uint8_t* lit, int32_t* triangle,
                  double* bary, void* stream);

/* Frame assembly of the multi-GPU path (render_image_pipeline's row-tile gather, SURVEY.md §8e;
 * the reference renders one process-local frame, application.py:43-52): `tiles` holds n_parts
 * gathered row tiles, part p at tiles + p * part_stride_bytes, each as rtx_render_camera wrote it
 * for (row_block, n_parts, p) with out_kind `kind` (SoA colour: [3][rows_p * width]; u8:
 * [rows_p][width][3]). Writes the whole frame to `out` in the layout of a whole-frame render
 * (SoA [3][height * width] or u8 [height][width][3]). part_stride_bytes must hold part 0's tile
 * (the largest). */
int rtx_assemble_rows(const void* tiles, int64_t part_stride_bytes, int n_parts, int width, int height,
                      int row_block, int kind, void* out, void* stream);
/* rtx_assemble_rows for ranks that render runs of parts (rtx_render_camera_sched part_run): rank 0
 * renders parts [0, root_run), rank i >= 1 parts [root_run + (i - 1) run, root_run + i run) of the
 * root_run + (n_ranks - 1) run interleave; rank i's tile at tiles + i * part_stride_bytes (which
 * must hold the longest run's tile). root_run == run == 1 is rtx_assemble_rows. */
int rtx_assemble_runs(const void* tiles, int64_t part_stride_bytes, int n_ranks, int root_run, int run, int width,
                      int height, int row_block, int kind, void* out, void* stream);

/* ---- the row-tiled multi-GPU frame, one call per frame and rank (csrc/rtx_tiles.hip) ----
 * The north star's "framebuffer row-tiles across the GPUs of one node with an RCCL gather over
 * xGMI": the reference renders one frame in one process (render_image_pipeline,
 * application.py:43-52); python_ray_tracer_amd.distributed.TileGather drives these entry points.
 * Every rank renders its interleaved row tile (as rtx_render_camera_ex with row_block, n_parts =
 * world, part = rank); the root receives every peer's tile with one ncclRecv per peer inside one
 * RCCL group (each peer's link carries its own bytes at once; a ring would be bound by one link)
 * and un-permutes the rows on the device (rtx_assemble_rows). RCCL is the process's own librccl,
 * resolved at run time (rtx_rccl_load): the library has no link-time RCCL dependency. */
#define RTX_TILES_MAX_SLOTS 4
/* dlopen the RCCL library at `path` (NULL: "librccl.so"), reusing it if the process already loaded
 * it (torch's), and resolve the calls used here. Idempotent. */
int rtx_rccl_load(const char* path);
/* ncclGetUniqueId into id_out (128 bytes): the root calls it, the host broadcasts the bytes. */
int rtx_comm_unique_id(void* id_out);
/* ncclCommInitRank over `world` ranks (collective: every rank calls it with the same id); the
 * communicator is bound to the current device. max_ctas > 0: ncclCommInitRankConfig with
 * maxCTAs = max_ctas, capping the blocks its kernels take from a render running beside them. */
int rtx_comm_init(const void* id, int world, int rank, int max_ctas, void** comm_out);
int rtx_comm_destroy(void* comm);
/* rtx_tiles_create flags. RTX_TILES_LOOPBACK: a one-rank plan whose tile still travels through
 * RCCL (sent to and received from itself, then assembled): the gather path on a single GPU.
 * RTX_F_RESERVE(n): every render of a plan that gathers (world > 1 or loopback) passes it, so that
 * frame k's RCCL kernels find free slots beside frame k+1's persistent render. */
#define RTX_TILES_LOOPBACK 1u
/* RTX_TILES_ROWS (uint8 frames): every row block travels on its own, straight into its rows of the
 * root's frame (one ncclSend / ncclRecv per block; the root's own blocks by one strided device
 * copy), so the root never runs the assembly pass (a read and a write of the whole frame in HBM,
 * beside its next render). recv[s] then holds the root's own tile only (part_bytes). */
#define RTX_TILES_ROWS 2u
/* RTX_TILES_TIMED: timing events on the plan's stream around each slot's RCCL group and the root's
 * assembly (plans that gather), read back by rtx_tiles_timing: the measured gather per frame and
 * rank (bench.py's secondary.c4_tiles.gather: bytes per peer and the achieved rate per link). */
#define RTX_TILES_TIMED 4u
/* Shares: rank 0 renders the run of parts [0, root_run) and rank i >= 1 the run [root_run + (i - 1)
 * run, root_run + i run) of the root_run + (world - 1) run interleave (rtx_render_camera_sched
 * part_run). root_run = run = 1 is the even split; a root_run below run leaves the root, which also
 * receives and assembles every frame, a smaller share (then the root must be rank 0). part_bytes must
 * hold the longest run's tile.
 * A plan for frames of width x height in row blocks of row_block, out_kind RTX_OUT_*, `slots`
 * frames in flight (<= RTX_TILES_MAX_SLOTS). Per slot s, caller-owned device buffers kept for the
 * plan's life: a peer's send[s] (part_bytes) and the root's recv[s] (world * part_bytes: part p at
 * p * part_bytes). part_bytes holds the longest run's tile, a multiple of 16. world == 1 needs
 * neither buffers nor a communicator (comm NULL): the single part is the frame (unless
 * RTX_TILES_LOOPBACK: then send and recv as a root and peer would). Creates the plan's own
 * collective stream on the current device. */
int rtx_tiles_create(void* comm, int world, int rank, int root, int width, int height, int row_block, int out_kind,
                     int slots, void* const* send, void* const* recv, int64_t part_bytes, int root_run, int run,
                     unsigned flags, void** plan_out);
/* Frame of slot `slot`: on `stream`, wait until the slot's previous frame has left its buffers, then
 * render this rank's tile (scene, n_spheres, max_bounces, workspace, flags, deferred_out, tile_order,
 * tile_cost as rtx_render_camera_sched); then, on the plan's stream after the render, the RCCL gather to the root
 * and (root) the assembly into `frame` (the root's whole frame, in a whole-frame render's layout;
 * ignored on peers). Asynchronous; never synchronises. */
int rtx_tiles_submit(void* plan, int slot, const double* scene, int n_spheres, int max_bounces, void* workspace,
                     size_t workspace_bytes, unsigned flags, uint32_t* deferred_out, const uint32_t* tile_order,
                     uint32_t* tile_cost, void* frame, void* stream);
/* Make `stream` wait until slot `slot`'s frame is complete (the root's frame is then valid in
 * stream order). */
int rtx_tiles_finish(void* plan, int slot, void* stream);
/* Waits for the plan's stream, then frees its stream and events (not the caller's buffers). */
int rtx_tiles_destroy(void* plan);
/* RTX_TILES_TIMED plans: waits for slot `slot`'s latest frame on the plan's stream, then gives
 * gather_ms, from the moment the plan's stream could start the gather (this rank's tile rendered)
 * to the completion of its RCCL group (a peer: its send delivered; the root: every peer's tile
 * received), and assemble_ms, the root's assembly after it (0 on peers). Synchronising: call it
 * outside a timed region. No replacement in the reference (one process, application.py:43-52). */
int rtx_tiles_timing(void* plan, int slot, float* gather_ms, float* assemble_ms);

/* Test hook: out[0:n] = the library's fast-path sqrt(a), out[n:2n] = the compiler's full sqrt(a),
 * out[2n:3n] = fast-path a/b, out[3n:4n] = full a/b, out[4n:5n] = the renormalisation factor of an
 * already-unit vector with |v|^2 = a (closed form when every lane of the wave has a within 2^-30
 * of 1), out[5n:6n] = 1/sqrt(a) by the full expansions (a == 0: 1). out holds 6n doubles. The
 * render kernels use the fast paths (correctly rounded sequences without operand scaling where it
 * is the identity); tests require each pair to agree bit for bit. */
int rtx_selftest_math(const double* a, const double* b, int64_t n, double* out, void* stream);
/* Test hook: out[i] = the render kernels' sine (the reduction and polynomial for |x| <= 2^20, the path
 * every shade takes when RTX_H_SINRED is set) of x[i], i < n, compiled as the kernels compile it. The
 * sine is a fixed chain of float64 multiplications and fused multiply-adds, so it is determined bit
 * for bit (tests/test_gpu_uniform_terms.py evaluates the chain exactly). */
int rtx_selftest_sin(const double* x, int64_t n, double* out, void* stream);

/* Test hook: the k_render_fast launches of the calling thread's latest render call
 * (rtx_render_camera*, rtx_render_frames, rtx_trace_rays, rtx_shade_hits, rtx_tiles_submit), in
 * launch order, RTX_LAUNCH_WORDS ints each: {B, LDS, DEEP, STATS, TP, IMG, NSPH, WAVES, grid_x,
 * grid_y, grid_z, n_fetch, tile_order != NULL, lds_bytes}: the template arguments of the
 * instantiation that was launched, as its launch site names them, then the launch's grid, the
 * tile-fetch counters in use (0: not a persistent launch), whether it carried a dispatch order, and
 * its dynamic LDS bytes; *general_out (may be NULL) = 1 if k_render_general was launched. Writes at
 * most max_records records; returns how many launches there were (a render call launches at most
 * RTX_LAUNCH_MAX), or RTX_E_ARG for a negative max_records or a null records with max_records > 0.
 * The state is per calling thread and cleared on entry to every render call; 0 launches before
 * the thread's first one. */
#define RTX_LAUNCH_WORDS 14
#define RTX_LAUNCH_MAX 4
int rtx_last_launches(int* records, int max_records, int* general_out);

/* Live timing of the dominant render kernel (used by bench.py for the roofline): after
 * rtx_profile_enable(k), the next k render launches hand a hipEvent pair to the k_render_fast
 * dispatch itself (hipExtLaunchKernelGGL start/stop events: the kernel's own start and end, as
 * rocprofv3's kernel trace sees them). rtx_profile_collect waits for the recorded events and
 * returns the summed kernel time and the launch count, then resets. rtx_profile_enable(0)
 * disables. The profiling state is per calling thread (only that thread's launches are timed);
 * meant for benchmarks, not for graph capture. */
int rtx_profile_enable(int max_launches);
int rtx_profile_collect(double* total_ms, int* n_launches);
/* Time only one render launch in `every` (default 1: all), the every-th, 2*every-th, ... after
 * rtx_profile_enable (not the first: it follows an idle GPU). Timing a launch costs stream time
 * (1080p C2: 24.1 Gpix/s timing every launch against 26.0 timing one in 10); sampling keeps the
 * live kernel timing while leaving the timed region nearly unperturbed. Persists across
 * rtx_profile_enable calls. */
int rtx_profile_sample(int every);

#ifdef __cplusplus
}
#endif
#endif /* RTX_HIP_H */
