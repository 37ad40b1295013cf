/*
 * rrt.h — C ABI of the MI355X-native render hot path that replaces
 *         rs_ray_toy's  renderprocess.rs -> integrator/ -> bvh.rs + shape/ ->
 *         reflection.rs/material/ -> film.rs   (reference @ /root/reference/src).
 *
 * The reference has no FFI of its own (single Rust crate, no extern "C"); the
 * boundary a Rust maintainer would bind is therefore defined here, one entry
 * point per reference call it replaces (file:line cited on each prototype).
 * INTEGRATION.md shows the matching `extern "C"` block and the ctypes stub.
 *
 * Conventions
 *   - plain pointers + sizes, no C++ / torch types;
 *   - every function returns 0 on success or a negative RRT_E* code and never
 *     throws / aborts; rrt_last_error() gives the message for this thread;
 *   - the reference's panics (assert!/unwrap) map to RRT_EPANIC with the same
 *     condition in the message;
 *   - scene data is *host* memory owned by an rrt_scene; device state is owned
 *     by an rrt_handle (one HIP stream per handle, thread-compatible);
 *   - ray / hit / film batches may be host or device memory (`mem` field).
 *
 * All reference arithmetic is f64 (geometry.rs:12-20); the scene description
 * below therefore carries f64, and the device handle picks its compute type
 * (RRT_F32 = product path, RRT_F64 = bit-tight parity mode) at create time.
 */
#ifndef RRT_H
#define RRT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RRT_ABI_VERSION 11

/* ---- error codes ------------------------------------------------------- */
enum {
  RRT_OK = 0,
  RRT_EINVAL = -1,   /* bad argument                                         */
  RRT_EIO = -2,      /* file could not be read / written                     */
  RRT_EPARSE = -3,   /* scene.json / OBJ syntax                              */
  RRT_EPANIC = -4,   /* the reference would panic here (message says where)  */
  RRT_EUNSUP = -5,   /* feature outside SURVEY §8 scope (named in message)   */
  RRT_EDEVICE = -6,  /* HIP error / no GPU / extension not usable            */
  RRT_ENOMEM = -7
};

/* ---- compat flags (SURVEY §8.0 quirk ledger). Default = all reference. --- */
enum {
  RRT_FIX_BVH_LBVH_SLICE = 1u << 0, /* Q26 off: emit_lbvh second child uses slice[split..] */
  RRT_FIX_BVH_SAH        = 1u << 1, /* Q27 off: real 12-bucket SAH in build_upper_sah      */
  RRT_SKIP_MIS_BSDF_RAY  = 1u << 2, /* do not trace estimate_direct's BSDF-sampled ray;
                                       result-invariant because of Q18     */
  /* How the DEVICE evaluates triangle instances (TransformedPrimitive, primitives.rs:115-139; transform.rs:525-537). "Kept": every
   * instance goes through the reference's own per-primitive ray transform (world_to_prim.t(ray), object-space test, t copied
   * back, interaction transformed) - the reference's evaluation order, bit for bit in RRT_F64. "Flattened": rigid instances
   * are moved to world space once at upload (one ray per traversal; exact box / face ties may break differently, DESIGN.md
   * section 4). Defaults: RRT_F64 keeps (parity mode = the reference's order), RRT_F32 flattens (product speed; non-rigid
   * instances are always kept). The two flags override the default of either mode. */
  RRT_INSTANCES_FLATTEN  = 1u << 3,
  RRT_INSTANCES_KEEP     = 1u << 4
};
#define RRT_FIXED_BVH (RRT_FIX_BVH_LBVH_SLICE | RRT_FIX_BVH_SAH)

/* ---- enums mirrored from the reference's scene.json vocabulary ---------- */
enum { RRT_PRIM_TRIANGLE = 0, RRT_PRIM_SPHERE = 1 };
enum { /* material_type, renderprocess.rs:664-871 */
  RRT_MAT_MATTE = 0, RRT_MAT_PLASTIC = 1, RRT_MAT_METAL = 2, RRT_MAT_MIRROR = 3, RRT_MAT_DEBUG = 4,
  RRT_MAT_GLASS = 5, RRT_MAT_TRANSLUCENT = 6   /* material/glass.rs, material/translucent.rs */
};
enum { RRT_LIGHT_POINT = 0, RRT_LIGHT_DIFFUSE = 1, RRT_LIGHT_DISTANT = 2 };  /* renderprocess.rs:991-1031 */
enum { RRT_SAMPLER_HALTON = 0, RRT_SAMPLER_STRATIFIED = 1 };    /* renderprocess.rs:1306-1325 */
enum { RRT_FILTER_BOX = 0, RRT_FILTER_TRIANGLE = 1, RRT_FILTER_GAUSSIAN = 2 };
enum { /* integrator_type, renderprocess.rs:1399-1499 */
  RRT_INT_PATH = 0, RRT_INT_DIRECT = 1, RRT_INT_DEBUG = 2, RRT_INT_AO = 3
};
enum { RRT_STRATEGY_ONE = 0, RRT_STRATEGY_ALL = 1 };
enum { RRT_F32 = 0, RRT_F64 = 1 };
enum { RRT_MEM_HOST = 0, RRT_MEM_DEVICE = 1 };

/* ---- flattened scene description (host memory, read-only to callers) ---- */

/* Transform{m, m_inv}, transform.rs:181-184, row-major 4x4 */
typedef struct rrt_xform { double m[16]; double m_inv[16]; } rrt_xform;

/* Triangle{v,n,uv,mesh}, shape/triangle.rs:63-70 (indices into the pooled arrays) */
typedef struct rrt_tri {
  uint32_t v[3];
  uint32_t n[3];    /* valid iff mesh_has_n  */
  uint32_t uv[3];   /* valid iff mesh_has_uv */
  /* Triangle::new triangle.rs:73-111. 0 = mesh.n (mesh.uv) empty; 1 = array and its index list present;
   * 2 = array present, index list empty (the reference then uses element 0 three times). */
  uint8_t mesh_has_n;
  uint8_t mesh_has_uv;
  uint8_t pad[2];
} rrt_tri;

/* Sphere, shape/sphere.rs:17-26 */
typedef struct rrt_sphere {
  int32_t xform;    /* obj_to_world (index into xforms) */
  double radius, z_min, z_max, theta_min, theta_max, phi_max;
} rrt_sphere;

/* GeometricPrimitive (+ optional TransformedPrimitive), primitives.rs:20-30 */
typedef struct rrt_prim {
  uint8_t type;         /* RRT_PRIM_*                                 */
  uint8_t pad[3];
  uint32_t shape;       /* index into tris / spheres                  */
  int32_t instance;     /* primitive_to_world xform index, -1 = none  */
  uint32_t material;    /* index into materials                       */
} rrt_prim;

/* Texture graph (texture/ module, built by make_textures renderprocess.rs:298-515). Float and rgb textures share one
 * array; a float texture carries its value in all three channels. Children are indices of textures created EARLIER
 * (the reference captures the Arc at creation time, so a later texture of the same name does not rebind them), or -1
 * with the fallback constant in `fallback[]`. ImageTexture: 8-bit non-interlaced PNG files (other formats / depths of
 * the `image` crate are RRT_EUNSUP where a material uses the texture), as the MIPMap of mipmap.rs in `images[]`. */
enum { RRT_TEX_CONSTANT = 0, RRT_TEX_MIX = 1, RRT_TEX_BILERP = 2, RRT_TEX_CHECKER2D = 3, RRT_TEX_CHECKER3D = 4,
       RRT_TEX_SCALE = 5, RRT_TEX_WINDY = 6, RRT_TEX_WRINKLED = 7, RRT_TEX_UV = 8, RRT_TEX_IMAGE = 9 };
enum { RRT_WRAP_REPEAT = 0, RRT_WRAP_BLACK = 1, RRT_WRAP_CLAMP = 2 };   /* ImageWrap mipmap.rs:50-55 */
enum { RRT_MAP_UV = 0, RRT_MAP_SPHERICAL = 1, RRT_MAP_CYLINDRICAL = 2, RRT_MAP_PLANAR = 3, RRT_MAP_IDENTITY3D = 4 };
typedef struct rrt_texture {
  int32_t type;            /* RRT_TEX_*                                                              */
  int32_t mapping;         /* RRT_MAP_* (texture/mod.rs:205-374)                                     */
  int32_t child[3];        /* t1, t2, amount (Mix) -> textures[] index or -1                         */
  int32_t aa_none;         /* Checkerboard2D: aamode == "none" (checkerboard.rs:13-16)               */
  int32_t octaves;         /* Wrinkled                                                               */
  int32_t image;           /* IMAGE: index into rrt_scene_desc.images                                */
  double fallback[3][3];   /* get_text_fallback's ConstantTexture per child (renderprocess.rs:282-296) */
  double v[4][3];          /* CONSTANT: v[0]; BILERP: v00, v01, v10, v11                              */
  double omega;            /* Wrinkled                                                               */
  double map[4];           /* UV: su, sv, du, dv;  PLANAR: ds, dt                                    */
  double vs[3], vt[3];     /* PLANAR                                                                 */
  double world_to_texture[16];   /* SPHERICAL, CYLINDRICAL: inverse(to_world); IDENTITY3D: to_world itself
                                    (renderprocess.rs:368,384,388 pass `to_world` as world_to_texture) */
} rrt_texture;

/* MIPMap (mipmap.rs:70-96) as MIPMap::create (:270-382) leaves it. Each pyramid level is the BlockedArray's own
 * `data` vector (memory.rs:24-98): texel (u, v) lives at
 *     16 * (u_blocks * (v & 3) + (u & 3)) + 4 * (v >> 2) + (u >> 2)
 * - the index expression of memory.rs:76-85, which swaps pbrt's block / offset roles, so texels alias each other and the
 * level holds whatever was written last at each cell. Lookups go through the same expression. */
typedef struct rrt_image_level { uint32_t u_res, v_res, u_blocks, pad; uint64_t offset, n; /* RGB triples in image_texels */ } rrt_image_level;
typedef struct rrt_image {
  int32_t do_trilinear, wrap;   /* RRT_WRAP_* */
  double max_aniso;
  int32_t n_levels, pad;
  rrt_image_level levels[16];
} rrt_image;

/* material parameter slots of rrt_material.tex[] */
enum { RRT_P_KD = 0, RRT_P_KS, RRT_P_KR, RRT_P_ETA, RRT_P_K, RRT_P_SIGMA, RRT_P_ROUGHNESS, RRT_P_UROUGHNESS,
       RRT_P_VROUGHNESS, RRT_P_KT, RRT_P_REFLECT, RRT_P_TRANSMIT, RRT_P_INDEX, RRT_P_COUNT };

/* material parameters, material/{matte,plastic,metal,mirror,debug_material,glass,translucent}.rs: the constant
 * value of each parameter, or (tex[slot] >= 0) the texture that replaces it at every hit */
typedef struct rrt_material {
  int32_t type;         /* RRT_MAT_*                                  */
  int32_t remap_roughness;
  double kd[3], ks[3], kr[3];
  double eta[3], k[3];
  double sigma, roughness, u_roughness, v_roughness;
  double kt[3];         /* glass */
  double reflect[3], transmit[3];   /* translucent */
  double index;         /* glass "eta" (a float texture there; `eta` above is MetalMaterial's spectrum) */
  int32_t tex[RRT_P_COUNT];   /* index into rrt_scene_desc.textures per RRT_P_* slot, -1 = the constant above */
  int32_t bump;               /* "bump_map": float texture displacing the shading geometry (Material::bump, material/mod.rs:22-62), -1 = none */
} rrt_material;

/* PointLight lights/point.rs:13-19, DiffuseAreaLight lights/diffuse.rs:13-22 */
typedef struct rrt_light {
  int32_t type;         /* RRT_LIGHT_*                                */
  int32_t n_samples;
  double spectrum[3];   /* I (point) or Lemit (diffuse)               */
  double p_light[3];    /* always 0,0,0 in the reference (Q17)        */
  int32_t shape_type;   /* RRT_PRIM_* of light_shape (diffuse only)   */
  uint32_t shape;       /* index into spheres / tris                  */
  double area;
  double w_light[3];    /* distant: normalize(light_to_world(from - to)), lights/distant.rs:30 */
  double world_radius;  /* distant: bounding sphere of aggregate.world_bound(), distant.rs:31-33, geometry.rs:1656-1668 */
} rrt_light;

/* LinearBVHNode, bvh.rs:103-109 (f64 bounds as built; device narrows conservatively) */
typedef struct rrt_bvh_node {
  double bounds[6];     /* pmin xyz, pmax xyz                         */
  uint32_t offset;      /* leaf: first prim in prim_order; interior: second child */
  uint32_t n_primitives;
  uint32_t axis;
  uint32_t pad;
} rrt_bvh_node;

/* LensElementInterface after RealisticCamera::new, camera.rs:32-38,80-99 (metres) */
typedef struct rrt_lens_elem { double curvature_radius, thickness, eta, aperture_radius; } rrt_lens_elem;

typedef struct rrt_camera {
  rrt_xform camera_to_world;
  double shutter_open, shutter_close;
  int32_t simple_weighting;
  int32_t n_elems;
  const rrt_lens_elem* elems;
  double exit_pupil_bounds[64][4];   /* Bounds2f pmin.x,pmin.y,pmax.x,pmax.y; camera.rs:121-133 */
  uint8_t exit_pupil_valid[64];      /* only slabs the path can index are computed (Q6): 0 and 63 */
} rrt_camera;

typedef struct rrt_film {
  int32_t xres, yres;
  int32_t crop[4];                   /* cropped_pixel_bounds x0,y0,x1,y1; film.rs:151-160 */
  int32_t sample_bounds[4];          /* get_sample_bounds, film.rs:188-199 */
  double diagonal;                   /* metres */
  double physical_extent[4];         /* get_physical_extent, film.rs:200-208 */
  int32_t filter_type;
  double filter_radius[2];
  double filter_alpha;
  double filter_table[256];          /* film.rs:163-173 (incl. Q4) */
  double scale, max_sample_luminance;
} rrt_film;

typedef struct rrt_sampler {
  int32_t type;
  int32_t sample_at_center;
  uint64_t samples_per_pixel;        /* nsamp; effective = nsamp-1 (Q1) */
  /* Halton, samplers/halton.rs:23-61 */
  int64_t base_scales[2], base_exponents[2];
  uint64_t sample_stride, mult_inverse[2];
  const uint16_t* perms;             /* radical_inverse_permutations, lowdiscrepancy.rs:250-270 (seeded) */
  size_t n_perms;
  uint64_t perm_seed;
  /* Stratified (oracle/host only) */
  int32_t xsamp, ysamp, dimension, jitter;
} rrt_sampler;

typedef struct rrt_integrator {
  int32_t type;
  int32_t max_depth;
  double rr_threshold;
  int32_t light_strategy;
  int32_t cos_sample, n_samples;
} rrt_integrator;

typedef struct rrt_scene_desc {
  uint32_t abi_version, flags;
  /* pooled mesh data (TriangleMesh, triangle.rs:16-28) */
  const double* positions; size_t n_positions;   /* xyz triples */
  const double* normals;   size_t n_normals;
  const double* uvs;       size_t n_uvs;         /* uv pairs */
  const rrt_tri* tris;       size_t n_tris;
  const rrt_sphere* spheres; size_t n_spheres;
  const rrt_xform* xforms;   size_t n_xforms;
  const rrt_prim* prims;     size_t n_prims;     /* aggregate input order, renderprocess.rs:1178-1304 */
  const rrt_material* materials; size_t n_materials;
  const rrt_texture* textures;   size_t n_textures;    /* every declared texture, declaration order */
  const rrt_image* images;       size_t n_images;
  const double* image_texels;    size_t n_image_texels;   /* RGB triples of all pyramid levels */
  const rrt_light* lights;   size_t n_lights;    /* scene.lights; infinite_lights unsupported */
  /* BVHAccel, bvh.rs:116-121 */
  const rrt_bvh_node* bvh_nodes; size_t n_bvh_nodes;
  const uint32_t* prim_order;    size_t n_prim_order;  /* ordered_prims -> index into prims */
  uint32_t max_prims_in_node, bvh_depth;
  double world_bound[6];
  rrt_camera camera;
  rrt_film film;
  rrt_sampler sampler;
  rrt_integrator integrator;
} rrt_scene_desc;

typedef struct rrt_scene rrt_scene;    /* owns every array above */
typedef struct rrt_handle rrt_handle;  /* device state            */

/* ---- batches ------------------------------------------------------------ */
typedef struct rrt_rays {   /* SoA; element type follows the handle's precision */
  int32_t mem;              /* RRT_MEM_*                                          */
  int32_t precision;        /* RRT_F32 / RRT_F64 of the arrays below              */
  const void *ox, *oy, *oz, *dx, *dy, *dz, *tmax;
  /* optional (may be NULL): for a ray spawned on a surface, the triangle it starts on (index as returned in
   * rrt_hits.prim), excluded from the tests; -1 = none. The reference needs no such field because f64 places
   * the self-hit at t ~ 1e-15 < 1e-7 (triangle.rs:200,263); fp32 callers should pass it. */
  const int32_t* skip_prim;
} rrt_rays;

typedef struct rrt_hits {
  int32_t mem, precision;
  void* t;                  /* ray.t_max after traversal (unchanged if miss)      */
  int32_t* prim;            /* index into prim_order (traversal order), -1 = miss */
  void *u, *v;              /* barycentrics of the winning hit                    */
  uint32_t* nodes_visited;  /* optional (may be NULL): per-ray counters, §8(d)    */
  uint32_t* prims_tested;
} rrt_hits;

typedef struct rrt_render_stats {
  uint64_t camera_samples;      /* W*H*(nsamp-1) in range                         */
  uint64_t camera_rays;         /* samples with weight>0: integrator/mod.rs:101   */
  uint64_t closest_queries, any_queries;
  uint64_t nodes_visited, prims_tested;   /* closest + any, when counting is enabled (count_traversal option) */
  double ms_total, ms_raygen, ms_closest, ms_any, ms_shade, ms_film;
  uint64_t closest_launches, any_launches;
  uint64_t closest_nodes, closest_prims;  /* split of nodes_visited / prims_tested per kernel: the roofline's */
  uint64_t any_nodes, any_prims;          /* algorithmic-byte model needs the closest-hit kernel's own counts */
  uint64_t tile_launches;       /* closest-hit launches over camera rays issued with the per-patch sub-trees ("tile_trees" option) */
  uint64_t root_culled;         /* closest_queries answered by the camera kernels: camera rays that miss the root box ("root_cull" option) */
  uint64_t sky_culled;          /* closest_queries answered by the horizon tables: bounce rays the path shading kernel proves to leave the scene ("horizon_cull" option) */
  uint64_t list_launches;       /* any-hit launches served by the shadow candidate lists ("shadow_lists" option) instead of the tree walk */
  double ms_gather;             /* the collective rrt_film_gather / _gather_all enqueued behind a frame in flight (HIP events on the handle's stream around
                                 * the grouped send / recv or the reduce): lets a multi-GPU run separate the ranks' render imbalance (ms_total) from the
                                 * collective (film.rs:248-263 merge_film_tile is what it replaces); 0 when no collective followed the frame */
  double s_horizon_build;       /* host seconds rrt_create spent building this handle's horizon tables (a setup cost, like the BVH build; 0 when another handle
                                 * of the process had built them for the same geometry, or the scene gets none) */
} rrt_render_stats;

/* ---- host side: scene build (stays on the host in the north_star) -------- */

/* deploy_render's loader half: renderprocess.rs:92-105 make_scene + make_integrator
 * (incl. objparser.rs parse_obj, BVHAccel::new bvh.rs:307, RealisticCamera::new camera.rs:66). */
int rrt_scene_load(const char* scene_json_path, uint32_t flags, uint64_t perm_seed, rrt_scene** out);
/* same, JSON text + root dir for relative assets (renderprocess.rs:94-99,114-120) */
int rrt_scene_load_str(const char* json_text, const char* root_dir, uint32_t flags, uint64_t perm_seed,
                       rrt_scene** out);
const rrt_scene_desc* rrt_scene_desc_of(const rrt_scene*);
void rrt_scene_free(rrt_scene*);
/* the reference's non-fatal eprintln! diagnostics raised while loading (unsupported texture types, ...) */
size_t rrt_scene_warning_count(const rrt_scene*);
const char* rrt_scene_warning(const rrt_scene*, size_t i);

/* what a host needs of the film to size its buffers and resolve the image (Film::full_resolution film.rs:137, Film::scale :142) without
 * reading rrt_scene_desc's layout; any pointer may be NULL */
int rrt_scene_film(const rrt_scene*, int32_t* xres, int32_t* yres, double* scale);

/* Film::write_image film.rs:323-366 (Q3 already folded into w) + write_image renderprocess.rs:1501-1530.
 * film_xyzw: W*H*4 host floats/doubles (X,Y,Z sums and filter_weight_sum per pixel). */
int rrt_resolve_rgba8(const void* film_xyzw, int precision, int w, int h, double scale, uint8_t* rgba);
int rrt_write_png(const char* path, const uint8_t* rgba, int w, int h);

/* ---- device side --------------------------------------------------------- */
int rrt_device_count(void);
/* uploads the scene (rigid triangle instances flattened to world space; spheres keep their transforms); the wavefront
 * pools are allocated on first use. RRT_EDEVICE without a HIP device: there is no CPU fallback. */
int rrt_create(int device, const rrt_scene_desc* desc, int precision, rrt_handle** out);
void rrt_destroy(rrt_handle*);
/* non-fatal diagnostics of rrt_create, in the manner of the reference's eprintln! lines (rrt_scene_warning): what this handle's precision
 * mode does not claim for this scene - RRT_F32 with transmissive sphere primitives (sphere.rs:124-259 has no epsilon: the reference's own
 * sphere pixels hang on last-bit coins that fp32 cannot replay; use RRT_F64) - and shortcuts that were switched off */
size_t rrt_warning_count(const rrt_handle*);
const char* rrt_warning(const rrt_handle*, size_t i);
/* raw hipStream_t of the handle (for event timing by the caller) */
void* rrt_stream(rrt_handle*);

/* BVHAccel::intersect bvh.rs:183-236 + Triangle/Sphere::intersect (closest = "last accepted", Q10) */
int rrt_trace_closest(rrt_handle*, const rrt_rays* rays, size_t n, rrt_hits* out);
/* BVHAccel::intersect_p bvh.rs:124-173 + Triangle::intersect_p (Q11) */
int rrt_trace_any(rrt_handle*, const rrt_rays* rays, size_t n, uint8_t* occluded /* mem as rays->mem */);

/* ISampler::get_camerasample samplers/mod.rs:28-34 + RealisticCamera::generate_ray_differential
 * camera.rs:582-628 for sample_num in [s0,s1) of every pixel in [x0,x1)x[y0,y1) (unit test surface).
 * Outputs (host, doubles): per sample 5 sampler dims, ray o(3) d(3), weight. Layout [pixel][sample]. */
int rrt_camera_samples(rrt_handle*, const int32_t rect[4], uint64_t s0, uint64_t s1,
                       double* dims5, double* ray_od6, double* weight);

/* The sampler's unit-test surface, as rrt_camera_samples is the camera's: the values the frame's kernels draw, from the device functions they
 * call (halton_pixel_offset, draw_1d, draw_2d of dmath.hpp). All arrays are the host's; the values are doubles in both precisions, because the
 * sampler produces f64 in both. Stream i is (pixel[i] = y << 16 | x inside the film, sample_num[i] in 0 .. nsamp-1).
 *   index[i]                     the word the kernels carry for the stream (may be NULL): HaltonSampler halton_pixel_offset + sample_num * stride
 *                                (Halton::get_index_for_sample halton.rs:75-105), StratifiedSampler (y * xres + x) << 10 | sample_num
 *   v1[i * count + k]            what get_1d returns with the stream's 1D counter at first + k: HaltonSampler dimension first + k
 *   v2[(i * count + k) * 2 ..]   what get_2d returns with the counter at first + k: HaltonSampler dimensions first + k and first + k + 1,
 *                                StratifiedSampler its 2D counter (which counts apart from the 1D one)
 * The handle's options apply as they do to a frame ("halton_tables"; "cam_tables" belongs to the camera kernels, which this call does not run).
 * Leaves the handle as it was and never sets a device error bit: RRT_EINVAL, before any device work, for NULL arguments (index excepted), n == 0,
 * count == 0, n * count > 2^31 - 1, a pixel outside the film, sample_num >= nsamp, first + count >= 1000 under the HaltonSampler (v2 would read
 * dimension 1000), first + count > 4095 under the StratifiedSampler (a counter of 4095), a frame in flight. RRT_EUNSUP / RRT_EPANIC as
 * rrt_render_rect gives for the scene's sampler. */
int rrt_sampler_values(rrt_handle*, const uint32_t* pixel, const uint32_t* sample_num, size_t n, uint32_t first, uint32_t count,
                       uint64_t* index /* n, may be NULL */, double* v1 /* n x count */, double* v2 /* n x count x 2 */);

/* SamplerIntegrator::si_render integrator/mod.rs:48-139 restricted to pixel rect [x0,y0,x1,y1):
 * all samples of those pixels, Li by the scene's integrator, FilmTile::add_sample + merge_film_tile.
 * film_xyzw: full-frame W*H*4 buffer (handle precision, host or device per film_mem); only pixels the
 * rect's samples touch are written (+=). */
int rrt_render_rect(rrt_handle*, const int32_t rect[4], void* film_xyzw, int film_mem,
                    rrt_render_stats* stats /* may be NULL */);

/* Radiance along caller-supplied rays (no counterpart in the reference, whose only way into an integrator is its RealisticCamera): another
 * camera, light probes and baking, or a look at what each sample of a pixel carried. The caller's rays take the place of the camera kernels;
 * everything behind them - traversal, shading, sampler streams, film - is the frame's own code on the same pool state.
 *
 * rrt_ray_samples: SoA like rrt_rays, element type = the handle's precision, all arrays in `mem`.
 *   d:          taken as given; must be unit length, as the camera's is.
 *   weight:     may be NULL = 1 everywhere. A sample with weight 0 (or below, or NaN) is dead: never traced.
 *   rxo .. ryd: optional ray differentials, all twelve arrays NULL or all set: origin and direction of rx and of ry, ALREADY scaled as
 *               scale_differentials leaves them (integrator/mod.rs:94-96). NULL: rx = ry = the ray itself (zero footprint). Read only when
 *               the scene has textured materials.
 *   pixel, sample_num: the sampler stream of each ray - the state the frame's sample (x, y, sample_num) has after get_camerasample
 *               (samplers/mod.rs:28-34). pixel = y << 16 | x inside the film, sample_num in 1 .. nsamp-1. Used by rrt_radiance only;
 *               rrt_render_rays derives both from the layout.
 *
 * rrt_radiance: rgb4[4 i .. 4 i + 3] = {Li.r, Li.g, Li.b, 0} of ray i (handle precision, in rays->mem, 16-byte aligned there), Li by the
 * scene's integrator - Path, DirectLighting or Debug; AOIntegrator returns 0, as the frame's does (ao.rs:62-64). The sampler starts where the
 * frame's sample (pixel, sample_num) stands after its camera sample: HaltonSampler index halton_pixel_offset + sample_num * stride,
 * StratifiedSampler the (pixel, sample_num) index the camera kernels form, dimension counters past the camera's, bounce 0. The ray is traced
 * as the frame traces a camera ray: t_max = inf, no start triangle. Two rays that name the same (pixel, sample_num) are legal and simply
 * correlated. weight (beyond dead or alive), Film.max_sample_luminance and the pixel filter play no part; a dead ray yields 0. A ray's result
 * depends on its own inputs only - not on its position in the batch, nor on how the batch is cut into pool-sized chunks ("max_paths").
 *
 * rrt_render_rays: what rrt_render_rect does for sample_num in [s0, s1) of the rect's pixels, with the camera kernels replaced by the
 * caller's (ray, weight, p_film) per sample, laid out [pixel][sample] over the rect as rrt_camera_samples lays its outputs out. p_film: 2
 * per sample, handle precision, in rays->mem, raster coordinates (a sample of pixel (x, y) has p_film in [x, x+1) x [y, y+1), as the
 * reference's samplers place it). Everything else is the frame's: FilmTile::add_sample through the film's own filter, weight-0 samples
 * still adding filter weight (Q2), the max_sample_luminance clamp, the tripled weight (Q3), += into the caller's film, the frame
 * statistics - camera_rays counts the weights > 0; what belongs to the camera kernels (tile_launches, root_culled) is 0. Fed the handle's
 * own rrt_camera_samples, it reproduces rrt_render_rect's film.
 *
 * Both leave the handle as it was (a frame rendered before and after is the same frame). Errors, before any device work where the host
 * can see the arguments: RRT_EINVAL for NULL arguments, a precision that is not the handle's, partly set differentials, a rect outside the
 * film, s0 < 1, s1 > nsamp or s0 >= s1, n == 0, a frame in flight, a pixel or sample_num out of range - for device-resident arrays that
 * last check is made on the device before anything is traced, and the call returns RRT_EINVAL with nothing written to rgb4. RRT_EUNSUP /
 * RRT_EPANIC as rrt_render_rect gives for the scene.
 * Not provided: rank / world bands, _begin / _end (frames in flight), and the moments, passes and feature-buffer forms of the frame.
 * Measured (tools/render_rays_time.py, profiles/render_rays_time.json; config 4 at 1024^2, 32 spp, depth 8, fp32, samples and film in device
 * memory, one MI355X): rrt_render_rays on the handle's own camera samples 5.49 ms against rrt_render_rect's 6.42 ms (0.85), the same film bits. */
typedef struct rrt_ray_samples {
  int32_t mem, precision;
  const void *ox, *oy, *oz, *dx, *dy, *dz;
  const void *weight;
  const void *rxo[3], *rxd[3], *ryo[3], *ryd[3];
  const uint32_t *pixel;
  const uint32_t *sample_num;
} rrt_ray_samples;
int rrt_radiance(rrt_handle*, const rrt_ray_samples* rays, size_t n, void* rgb4);
int rrt_render_rays(rrt_handle*, const int32_t rect[4], uint64_t s0, uint64_t s1, const rrt_ray_samples* rays, const void* p_film,
                    void* film_xyzw, int film_mem, rrt_render_stats* stats /* may be NULL */);

/* Irradiance and spherical-harmonic probes at caller-supplied points (no counterpart in the reference): what baking and probes consume - the
 * irradiance at a surface point (a lightmap texel, a vertex, a sensor) or the SH projection of the radiance around a point in space - with
 * the rays made on the device from each draw's own sampler stream and only sums leaving it. rrt_radiance hands out one Li per ray; here the
 * caller ships 6 values per point instead of 6 per draw and gets 4 (or 4 + 27) per point back instead of 4 per draw.
 *
 * rrt_points: SoA, element type = the handle's precision, all arrays in `mem`.
 *   px, py, pz: the points.
 *   nx, ny, nz: RRT_IRR_COSINE: the surface normal, any non-zero finite length. RRT_IRR_SPHERE: the axis of the local frame; all three may
 *               be NULL = the z axis. A point whose normal is zero or not finite is dead: all its draws add nothing.
 *   pixel:      the sampler stream of point i, y << 16 | x inside the film; NULL: x = i % xres, y = (i / xres) % yres. Points may share a
 *               pixel; they are then simply correlated.
 * rrt_irr_params: NULL = {RRT_IRR_COSINE, offset 0}. offset is rounded to the handle's type.
 *
 * Draw j in [s0, s1), 1 <= s0 < s1 <= nsamp, of point i is the ray rrt_radiance would be given with (pixel_i, sample_num = j):
 *   u    = the first two values of that stream, what rrt_camera_samples reports as dims5[0], dims5[1] of sample j of that pixel (the film
 *          sample, which no point has a use for); the integrator continues at the dimensions past the camera's, so nothing is drawn twice
 *   nn   = n / |n|,  (s, t) = coordinate_system(nn) (geometry.rs:1146-1161)
 *   wl   = cosine_sample_hemisphere(u) (sampling.rs:270; a draw with wl.z == 0 is dead)  or  uniform_sample_sphere(u) (sampling.rs:233)
 *   d    = normalize((s wl.x + t wl.y) + nn wl.z),  o = p + nn * offset,  t_max = inf, no start triangle, rx = ry = the ray
 * and adds onto the caller's rows (handle precision, in points->mem; they start from what the buffers hold, draws in ascending j, plain adds):
 *   sums4[4 i ..]         += { L_j.r, L_j.g, L_j.b, y_j^2 },  y = 0.212671 r + 0.715160 g + 0.072169 b
 *   sh27[27 i + 3 k + c]  += L_j.c * Y_k(wl_j)   (RRT_IRR_SPHERE only, may be NULL), the real SH basis of bands 0 .. 2 at the LOCAL direction:
 *     Y_0 = 0.28209479177387814          Y_1 = 0.4886025119029199 y        Y_2 = 0.4886025119029199 z
 *     Y_3 = 0.4886025119029199 x         Y_4 = 1.0925484305920792 x y      Y_5 = 1.0925484305920792 y z
 *     Y_6 = 0.31539156525252005 (3 z^2 - 1)   Y_7 = 1.0925484305920792 x z      Y_8 = 0.5462742152960396 (x^2 - y^2)
 *   With n = NULL the local frame is coordinate_system of the z axis: local (x, y, z) = world (y, -x, z).
 * So calls over [1, a) and [a, b) leave, bit for bit, what one call over [1, b) leaves, and the cut into pool-sized passes ("max_paths")
 * changes no bit either. The caller scales: cosine mode E = pi / N * sums4[0..2], with sums4[3] the variance of its luminance follows;
 * sphere mode coefficients 4 pi / N * sh27. AOIntegrator scenes add zeros, as rrt_radiance returns zeros there.
 *
 * rrt_irradiance_rays: the unit-test surface, as rrt_camera_samples is the camera's: od6[(i * (s1 - s0) + (j - s0)) * 6 ..] = {o, d} of every
 * draw, handle precision, in points->mem; a dead draw writes six zeros. Nothing is traced.
 *
 * Both leave the handle as it was. Errors, the structs checked before the handle and everything the host can see before any device work:
 * RRT_EINVAL for NULL arguments, a precision that is not the handle's, n == 0 or n > 2^31 - 1, a draw range outside [1, nsamp) or empty, a bad
 * mode, a non-finite offset, sh27 given in cosine mode, NULL normals in cosine mode, a frame in flight, a pixel outside the film - for
 * device-resident arrays that last check is made on the device before anything is traced, and nothing is written. RRT_EUNSUP for the
 * StratifiedSampler (its first 2D value is a film sample inside its stratum, not an even cover of [0, 1)^2 by a pixel's draws); RRT_EUNSUP /
 * RRT_EPANIC as rrt_render_rect gives for the scene.
 * Not provided: a start-triangle exclusion per point (the offset is the tool), ray differentials, _begin / _end.
 * Measured (tools/irradiance_time.py, profiles/irradiance_time.json; config 4, Path depth 8, fp32, 31 799 points x 64 cosine draws, everything in
 * device memory, one MI355X): rrt_irradiance 2.71 ms against 4.58 ms for the same draws built in torch, sent through rrt_radiance and reduced in
 * torch (0.59); rrt_radiance alone over those 2.04 M rays 2.63 ms (2.62 on the parent commit's build). k_irr_gen 42 us, k_irr_reduce 49 us. */
enum { RRT_IRR_COSINE = 0, RRT_IRR_SPHERE = 1 };
typedef struct rrt_points {
  int32_t mem, precision;
  const void *px, *py, *pz;
  const void *nx, *ny, *nz;
  const uint32_t *pixel;
} rrt_points;
typedef struct rrt_irr_params { int32_t mode; int32_t pad; double offset; } rrt_irr_params;
int rrt_irradiance(rrt_handle*, const rrt_points* points, size_t n, uint64_t s0, uint64_t s1, const rrt_irr_params* params /* may be NULL */,
                   void* sums4 /* n x 4 */, void* sh27 /* n x 27, RRT_IRR_SPHERE only, may be NULL */);
int rrt_irradiance_rays(rrt_handle*, const rrt_points* points, size_t n, uint64_t s0, uint64_t s1, const rrt_irr_params* params /* may be NULL */,
                        void* od6 /* [point][draw][6] */);

/* Surface records and lightmap sites (no counterpart in the reference): where the surfaces are, and the world-space point, normal, tangent,
 * texture coordinate and reflectance at a place on a primitive - the step before rrt_irradiance. rrt_trace_closest stops at (t, prim, u, v);
 * these calls hand out the interaction the shading kernels rebuild from such a record (prim_order, Q13, kept and flattened instance
 * transforms, get_uvs' defaults and a sphere's root branch are the library's business, not the caller's). The chain atlas -> sites -> records
 * -> rrt_irradiance stays in device memory: px .. pz, nx .. nz of a record set ARE an rrt_points, and a dead record has a zero normal, which
 * rrt_irradiance defines as "adds nothing", so nothing is compacted on the way.
 *
 * rrt_surface: SoA, element type = the handle's precision, all arrays in `mem`. The groups are {px, py, pz}, {nx, ny, nz}, {sx, sy, sz},
 * {tu, tv}, {rho_r, rho_g, rho_b}, {t}, {prim, material}; each is all NULL (not produced, and not computed) or all set. Arrays are overwritten.
 *   p:    the point shading starts its spawned rays from. RRT_F64: o + d t. RRT_F32: the barycentric point on the stored triangle
 *         (p0 + ((p1 - p0) u + (p2 - p0) v), the unevaluated sum p_hi + p_lo of DESIGN.md rounded once), taken through the instance transform
 *         where the handle kept one; a sphere's point is Sphere::intersect's.
 *   n:    rrt_render_aov's n: the geometric normal after the instance transform, normalised, not turned towards anything, before any bump_map.
 *   s:    normalize(GEOMETRIC dpdu) after the instance transform: the s of rrt_render_ao's frame.
 *   uv:   the interaction's uv: the mesh uv or get_uvs' (0,0), (1,0), (1,1), interpolated; a sphere's own parameterisation.
 *   rho:  rrt_render_aov's rho table, textured parameters evaluated at the point with zero differentials.
 *   t:    rays form: what rrt_trace_closest reports (t_max unchanged on a miss); sites form: 0.
 *   prim, material: index into prim_order as rrt_hits.prim / index into materials. A DEAD record (a miss, a site with prim == -1) has
 *         prim = material = -1 and zeros everywhere else (t as above).
 * rrt_surface_rays: the rays are packed and traced exactly as rrt_trace_closest does it (skip_prim and tmax included): t and prim are, bit for
 * bit, what that call returns, and record i is the interaction of hit i. out->mem must equal rays->mem.
 * rrt_surface_at: a site is (prim, b1, b2) with the barycentrics of rrt_hits.u / .v: p = p0 + ((p1 - p0) b1 + (p2 - p0) b2) in the space the
 * handle stores the triangle in, then through the instance transform where the handle kept one; n, s, uv, rho and material as for a hit at those
 * barycentrics. Barycentrics outside the triangle extrapolate its plane. prim == -1 is "no site": a dead record. Refused (RRT_EINVAL): any other
 * index outside [0, n_prim_order), a sphere (its record needs the ray), a non-finite barycentric - host arrays are checked before any device
 * work, device arrays by a checking launch over the whole batch before anything is written. out->mem must equal sites->mem.
 * Both leave the handle as it was (a frame rendered before and after is the same frame). Errors, the structs checked before the handle:
 * RRT_EINVAL for NULL arguments, a bad mem, a partly set group, all groups NULL, a precision that is not the handle's, n == 0 or n > 2^31 - 1, a
 * frame in flight; RRT_EUNSUP / RRT_EPANIC as rrt_render_aov gives for the scene (primitives.rs:66, an ImageTexture lookup out of bounds).
 *
 * rrt_atlas_sites: which triangle, at which barycentrics, each texel of an aw x ah uv atlas shows. Texel (x, y), row-major y * aw + x, has the
 * centre c = ((x + 0.5) / aw, (y + 0.5) / ah). The candidates are the entries `prims` (HOST array, n_list indices as rrt_hits.prim; NULL = every
 * triangle entry of prim_order, ascending). Candidate k has the texture coordinates a, b, c3 of its vertices: its mesh uv, else get_uvs'
 * (0,0), (1,0), (1,1) - the object's own, no transform touches them. In double, in both precision modes, uncontracted, with
 * cross(p, q) = p.x q.y - p.y q.x:
 *   A = cross(b - a, c3 - a) (A == 0 covers nothing),  beta1 = cross(c - a, c3 - a) / A,  beta2 = cross(b - a, c - a) / A,
 *   covered iff beta1 >= 0 && beta2 >= 0 && beta1 + beta2 <= 1 (edges inclusive).
 * The owner of a texel is the covering candidate with the smallest position in the list, so instances that share a chart and duplicated
 * entries (Q26) resolve by the caller's order. site_prim = the owner's index or -1, b1 / b2 = its beta rounded once to the handle's type or 0:
 * the three arrays (aw * ah each, in `mem`) are an rrt_sites. n_covered (host, may be NULL) = the number of owned texels. uv outside [0, 1)^2
 * is not wrapped, and no gutter is made. Errors, before any device work: RRT_EINVAL for a NULL output, aw or ah outside 1 .. 16384, a bad mem,
 * n_list == 0 with a list, a list entry out of range or naming a sphere, a frame in flight.
 * Not provided: a follow-through-mirrors form, sphere sites, ray differentials or filtered rho, atlas dilation, a command-line form.
 * Measured (tools/surface_time.py, profiles/surface_time.json; config 4, fp32, everything in device memory, one MI355X): over 319 652 rays
 * rrt_surface_rays 0.266 ms with all groups against 0.248 ms for rrt_trace_closest (k_surface 6.9 us, at its streaming floor); 1024 x 1024 texels over
 * 100 352 charted triangles: rrt_atlas_sites 0.53 ms, rrt_surface_at 0.068 ms, against 2.08 s + 0.16 s for the same two steps in numpy. */
typedef struct rrt_surface {
  int32_t mem, precision;
  void *px, *py, *pz;
  void *nx, *ny, *nz;
  void *sx, *sy, *sz;
  void *tu, *tv;
  void *rho_r, *rho_g, *rho_b;
  void *t;
  int32_t *prim, *material;
} rrt_surface;
typedef struct rrt_sites { int32_t mem, precision; const int32_t* prim; const void *b1, *b2; } rrt_sites;
int rrt_surface_rays(rrt_handle*, const rrt_rays* rays, size_t n, rrt_surface* out);
int rrt_surface_at(rrt_handle*, const rrt_sites* sites, size_t n, rrt_surface* out);
int rrt_atlas_sites(rrt_handle*, int32_t aw, int32_t ah, const int32_t* prims /* host, may be NULL */, size_t n_list, int mem, int32_t* site_prim /* aw * ah */,
                    void* b1, void* b2 /* aw * ah, handle precision */, uint64_t* n_covered /* host, may be NULL */);

/* Nearest-surface point queries (no counterpart in the reference; none of its quirks applies to a distance, so the call is defined geometrically):
 * per point the nearest site on the scene's triangles and its distance - what a probe grid needs to drop probes against a wall, what baking from one
 * mesh onto another starts from, what a distance field is made of. {prim, b1, b2} of the output ARE an rrt_sites: they go into rrt_surface_at as
 * they are. rrt_points is reused so that a record set or an irradiance point set can be passed as it is: only px, py, pz, mem and precision are read;
 * the normals and `pixel` may be NULL and are ignored. All arrays in `mem` (out->mem must equal points->mem), element type = the handle's precision.
 *   Candidates: the triangle entries of prim_order. Sphere entries are NOT candidates (as for rrt_atlas_sites); a scene with no triangle entry is
 *     RRT_EUNSUP. A candidate's world-space vertices a, b, c are the ones the handle stores (fp32 handles: rounded to float); for a triangle of a
 *     non-rigid instance the handle kept, the stored raw vertices taken through the instance's primitive_to_world (m v + t, row by row,
 *     ((m0 x + m1 y) + m2 z) + m3), in the handle's type.
 *   Closest point of a candidate: the Voronoi-region test (Ericson, Real-Time Collision Detection 5.1.5), all in the handle's type, no operation
 *     contracted to an fma, dot(u, v) = (u.x v.x + u.y v.y) + u.z v.z:
 *       ab = b - a, ac = c - a, ap = p - a, d1 = dot(ab, ap), d2 = dot(ac, ap); bp = p - b, d3 = dot(ab, bp), d4 = dot(ac, bp);
 *       cp = p - c, d5 = dot(ab, cp), d6 = dot(ac, cp); vc = d1 d4 - d3 d2, vb = d5 d2 - d1 d6, va = d3 d6 - d5 d4;
 *       the first rule that holds gives (b1, b2):
 *         d1 <= 0 && d2 <= 0                        (0, 0)
 *         d3 >= 0 && d4 <= d3                       (1, 0)
 *         vc <= 0 && d1 >= 0 && d3 <= 0             (d1 / (d1 - d3), 0)
 *         d6 >= 0 && d5 <= d6                       (0, 1)
 *         vb <= 0 && d2 >= 0 && d6 <= 0             (0, d2 / (d2 - d6))
 *         va <= 0 && d4 - d3 >= 0 && d5 - d6 >= 0   w = (d4 - d3) / ((d4 - d3) + (d5 - d6)), (1 - w, w)
 *         otherwise                                 den = 1 / ((va + vb) + vc), (vb den, vc den)
 *       each of b1, b2 clamped to [0, 1]; q = a + (ab b1 + ac b2); d2 = ((p - q).x^2 + (p - q).y^2) + (p - q).z^2; dist = sqrt(d2).
 *     The result depends on (p, a, b, c) alone. b1 >= 0 and b2 >= 0 exactly; b1 + b2 <= 1 up to one rounding.
 *   Winner: the candidate with the smallest d2; among equal d2 the smallest index into prim_order (a point on a shared edge or vertex is a tie). A
 *     candidate whose d2 is NaN (a degenerate triangle can have one) never wins. The result is therefore that of a scan over all candidates and does
 *     not depend on the tree: a subtree is skipped only where its box's squared distance exceeds the current bound by a margin that covers the
 *     roundings of both distances (csrc/host/nearest.hpp kNearestPadUlps).
 *   Outputs (overwritten): a point is accepted iff dist <= (R)max_dist: prim = the winner's index into prim_order as rrt_hits.prim, b1, b2 its
 *     barycentrics as rrt_hits.u / .v, dist. A point with no accepted candidate, and a point with a non-finite coordinate (dead), gets prim = -1,
 *     b1 = b2 = 0, dist = (R)max_dist. dist may be NULL.
 * Errors, before any device work, the structs checked before the handle: RRT_EINVAL for NULL arguments (dist alone may be NULL), a bad mem, a
 * precision that is not the handle's, n == 0 or n > 2^31 - 1, max_dist NaN or negative (+inf and 0 are legal), a frame in flight. The call leaves
 * the handle as it was (a frame rendered before and after is the same frame).
 * Not provided: sphere candidates, a per-point radius, an excluded primitive, a sign (inside or outside), the k nearest, a _begin / _end form.
 * Measured (tools/nearest_time.py, profiles/nearest_time.json; config 4, fp32, everything in device memory, one MI355X): 1 048 576 atlas points lifted 0.01
 * extent off the surface 1.07 ms (1.0 ns per point) against 0.238 ms for rrt_trace_closest over as many rays; a 128^3 grid over the world bound 8.39 ms
 * (4.0 ns per point) against 0.281 ms. The fp32 default is the generic kernel on the linear tree; the pair-node kernel (option "nearest_pairs") returns the
 * same bits and measured 1.62 ms and 11.78 ms. */
typedef struct rrt_nearest_out {
  int32_t mem, precision;
  int32_t* prim;      /* n: index into prim_order as rrt_hits.prim; -1 = nothing within max_dist */
  void *b1, *b2;      /* n, handle precision: barycentrics as rrt_hits.u / .v  -> {prim, b1, b2} ARE an rrt_sites */
  void *dist;         /* n, handle precision; may be NULL */
} rrt_nearest_out;
int rrt_nearest(rrt_handle*, const rrt_points* points, size_t n, double max_dist, rrt_nearest_out* out);

/* All hits along a ray, in order (no counterpart in the reference, like rrt_nearest; defined geometrically, as a scan over all candidates): per ray the
 * k nearest accepted triangle hits, sorted, and the number of all of them - what thickness and layered baking, transparency and X-ray passes, inside /
 * outside tests and the sign of a distance field are made of. One traversal per ray, against k launches and k root-to-leaf walks of a peel with
 * rrt_trace_closest, which moreover neither terminates cleanly on coplanar faces nor is complete (Q10). Slot-major outputs: plane s of
 * {prim, b1, b2} (n values from [s * n]) IS an rrt_sites and goes into rrt_surface_at as it is. All arrays in `mem` (out->mem must equal rays->mem),
 * element type = the handle's precision R.
 *   Candidates: the triangle entries of prim_order. Sphere entries are NOT candidates (as for rrt_nearest and rrt_atlas_sites); a scene with no
 *     triangle entry is RRT_EUNSUP. A candidate's world-space vertices a, b, c are the ones the handle stores (fp32 handles: rounded to float); for a
 *     triangle of a non-rigid instance the handle kept, the stored raw vertices taken through the instance's primitive_to_world (m v + t, row by row,
 *     ((m0 x + m1 y) + m2 z) + m3), in the handle's type. rays->skip_prim[i], where the array is given and the value is >= 0, removes that one entry (by
 *     index into prim_order) from ray i's candidates.
 *   Acceptance of candidate (a, b, c) for ray (o, d, tmax): all in the handle's type, no operation contracted to an fma, the two divisions IEEE
 *     divisions, dot(u, v) = (u.x v.x + u.y v.y) + u.z v.z, (u x v) = (u.y v.z - u.z v.y, u.z v.x - u.x v.z, u.x v.y - u.y v.x). All three must hold:
 *     (i)   the triangle test, Moller-Trumbore in the operation order of rrt_trace_closest's (Triangle::intersect): E1 = b - a, E2 = c - a, P = d x E2,
 *           det = dot(E1, P), rejected if -1e-7 < det < 1e-7; f = 1 / det; T = o - a; u = f dot(T, P), 0 <= u <= 1; Q = T x E1; v = f dot(d, Q), v >= 0,
 *           u + v <= 1; t = f dot(E2, Q), t >= 1e-7. (No double-float origin: public rays carry none.)
 *     (ii)  t < (R)tmax.
 *     (iii) the ray passes the slab test of the candidate's OWN box, lo = min(a, b, c), hi = max(a, b, c) per axis: inv = 1 / d; per axis
 *           near = (lo - o) * inv, far = (hi - o) * inv, the two swapped where inv < 0; far *= 1 + 2 gamma(3), gamma(3) = 3 eps / (1 - 3 eps),
 *           eps = 2^-24 / 2^-53 (Bounds3::intersect_p); a NaN term is dropped and is never a reason to reject; pass iff max(nears, 0) <= min(fars, tmax).
 *     Rule (iii) makes the result independent of the tree: rounding is monotone, so a node box that contains the own box passes the same test
 *     whenever the own box does (node boxes are rounded outward; for scenes with kept instances they are grown by csrc/host/multihit.hpp
 *     kMultihitPadUlps), and a Moller-Trumbore "hit" at a grazing angle whose point lies nowhere near the triangle is rejected by definition
 *     instead of by accident of the tree. The walk opens every node whose box passes and prunes nothing by t, with or without `count`.
 *   Result (outputs are overwritten): the accepted candidates sorted by (t ascending, index into prim_order ascending). Slots 0 .. min(k, count) - 1
 *     hold them: t, prim = the index as rrt_hits.prim, b1 = u and b2 = v as rrt_hits.u / .v. The remaining slots hold prim = -1, t = (R)tmax,
 *     b1 = b2 = 0. count = the number of ALL accepted candidates, not clipped at k. A ray with a non-finite origin, direction or tmax (+inf is legal),
 *     or with a zero direction, is dead: count = 0 and all slots empty. With k == 0 the slot arrays are ignored and count must be set (the count-only
 *     form, for parity). b1 and b2 may both be NULL.
 *     WARNING for parity users: two triangles that share an edge BOTH report a ray through that edge (and all triangles around a vertex a ray through
 *     that vertex), at equal or nearly equal t, the smaller index first among equal t: such a ray's count is not the number of surface crossings.
 *   Relation to rrt_trace_closest: slot 0 is the NEAREST accepted hit. rrt_trace_closest returns the LAST accepted one in traversal order (Q10: the
 *     reference's triangle test never looks at t_max), its t for a triangle of a kept instance is the object-space one (Q15), it tests spheres, its
 *     fp32 kernels use a fast reciprocal and contract to fma, and it has no rule (iii). Where its hit is a rigid triangle and the nearest one, slot 0
 *     names the same prim; t, u and v agree to rounding, not to the bit.
 * Errors, before any device work, the structs checked before the handle: RRT_EINVAL for NULL arguments or ray arrays, k outside 0 .. RRT_MAX_HITS,
 * k > 0 with a NULL t or prim, exactly one of b1 / b2 set, k == 0 with count == NULL, a bad mem or out->mem != rays->mem, a precision that is not the
 * handle's, n == 0 or n > 2^31 - 1, a frame in flight. The call leaves the handle as it was (a frame rendered before and after is the same frame).
 * Not provided: sphere candidates, more than RRT_MAX_HITS slots, per-slot surface records in the same call (feed plane s to rrt_surface_at), a
 * pair-node fp32 kernel (the walk runs on the linear tree in both precisions), a _begin / _end form.
 * Measured (tools/trace_all_time.py, profiles/trace_all_time.json; config 4, fp32, everything in device memory, one MI355X): 1 048 576 unbounded rays
 * between random points of 1.2 x the world bound, 2.4 hits a ray on average and at most 19: k = 1 2.38 ms, k = 4 2.43 ms, k = 16 3.28 ms, the count-only
 * form 2.31 ms (2.2 - 3.1 ns per ray); a NULL count changes nothing (2.37 / 2.43 / 3.27 ms: nothing is pruned by t). One rrt_trace_closest over the same
 * rays 0.405 ms - it stops at the first hit, on the pair-node tree, where this call walks the whole ray on the linear tree -; a peel of k
 * rrt_trace_closest calls with skip_prim and an advanced origin 0.53 ms at k = 1, 2.14 ms at k = 4, 8.10 ms at k = 16: the single walk overtakes
 * the peel between k = 4 (0.88 x) and k = 16 (2.5 x), and unlike the peel it is complete and terminates on coplanar faces. */
#define RRT_MAX_HITS 16
typedef struct rrt_multi_hits {
  int32_t mem, precision;   /* mem must equal rays->mem; precision the handle's */
  int32_t k, pad;           /* slots per ray, 0 .. RRT_MAX_HITS */
  void* t;                  /* k * n, slot-major: slot s of ray i at [s * n + i] */
  int32_t* prim;            /* k * n, index into prim_order as rrt_hits.prim; -1 = empty slot */
  void *b1, *b2;            /* k * n, as rrt_hits.u / .v; both NULL or both set */
  uint32_t* count;          /* n: ALL accepted candidates of the ray, not clipped at k; may be NULL */
} rrt_multi_hits;
int rrt_trace_all(rrt_handle*, const rrt_rays* rays, size_t n, rrt_multi_hits* out);

/* Mutual visibility of two point sets as a packed bit matrix (no counterpart in the reference; defined geometrically by rrt_trace_all's acceptance
 * rules): can point a_i see point b_j, for n_a x n_b pairs - what form factors, light-visibility and PVS precomputation, sun-hour and sky-view
 * studies (points x directions), soft shadows from a sampled emitter and line-of-sight analysis reduce to. rrt_trace_any is the reference's shadow
 * ray with its quirks (Q9 - Q11) and no geometric occlusion test; rrt_trace_all with k = 0 gives the clean answer (count == 0) but walks the whole
 * ray and makes the caller build and ship n_a x n_b rays of 7 values and reduce as many counts. Here the segments are made on the device from the
 * two sets, a walk stops at the first accepted candidate, and one bit per pair comes back. rrt_points is reused, so a record set, an atlas site
 * set or an irradiance point set passes as it is; `pixel` is ignored. All arrays in a->mem; element type = the handle's precision R.
 *   Everything below is computed in R, no operation contracted to an fma, divisions and square roots IEEE, dot and cross as for rrt_trace_all.
 *   Normals: where a set's nx, ny, nz are given (all three or none), nn = n / sqrt(dot(n, n)) per component. A point whose normal is zero or not
 *     finite (or whose nn is not finite) is dead; so is a point with a non-finite coordinate or a non-finite origin / target below.
 *   Origin: o_i = a_i + nn_a * (R)offset_a where A has normals, otherwise a_i.
 *   RRT_VIS_POINTS: q_j = b_j + nn_b * (R)offset_b where B has normals, otherwise b_j; w = q - o, len = sqrt(dot(w, w)), d = w / len per component,
 *     tmax = len. len == 0: nothing lies between the points, the pair is visible iff no FACING flag is set. len not finite: not visible.
 *   RRT_VIS_DIRECTIONS: B holds directions (sun positions, sky samples): w = b_j, len = sqrt(dot(w, w)), d = w / len, tmax = +inf. A zero or
 *     non-finite direction (or len) is a dead column.
 *   Facing: RRT_VIS_FACING_A requires dot(nn_a, w) > 0, RRT_VIS_FACING_B requires dot(nn_b, w) < 0. A pair that fails is not visible and not traced.
 *   Blocked: a pair is blocked iff some triangle entry of prim_order other than skip_a[i] and skip_b[j] (indices into prim_order as
 *     rrt_rays.skip_prim; -1 or a NULL array = none) is accepted for the ray (o, d, tmax) by rrt_trace_all's rules (i) - (iii) above - the same
 *     functions of csrc/host/multihit.hpp on the same operands. Whether an accepted candidate exists does not depend on the order the candidates
 *     are looked at, so the answer is that of a scan over all entries and independent of the tree; rule (iii) and the grown node boxes of scenes
 *     with kept instances make the walk find what the scan finds, as for rrt_trace_all. No prune margin is involved: the walk opens every node whose
 *     box passes and leaves at the first accepted candidate. Bit for bit, pair (i, j) is visible iff rrt_trace_all reports count == 0 for that ray.
 *   Bit (i, j) = both points live, facing passed, not blocked.
 *   RRT_VIS_MATRIX: pair (i, j) is bit j & 63 of bits[i * words + j / 64], words = (n_b + 63) / 64; the unused high bits of a row's last word are 0.
 *     count[i] (may be NULL) = the number of set bits of row i.
 *   RRT_VIS_PAIRS: requires n_b == n_a; pair (i, i) is bit i & 63 of bits[i / 64], unused bits 0; count must be NULL.
 *   The outputs are overwritten. The result depends neither on how the call is cut into launches (option "max_paths") nor on `mem`.
 * Errors, before any device work, the structs checked before the handle: RRT_EINVAL for NULL a, b, out, bits or coordinate arrays; normals of which
 * only some are given; a bad mem, or a->mem, b->mem, out->mem not all equal; a precision that is not the handle's; n_a == 0, n_b == 0, either above
 * 2^31 - 1, or n_a * n_b > 2^40; a bad mode, b_kind or flag bit; a NaN or infinite offset; a non-zero offset or a FACING flag for a set without
 * normals; in RRT_VIS_DIRECTIONS B normals, offset_b != 0, RRT_VIS_FACING_B or skip_b; in RRT_VIS_PAIRS n_b != n_a or a non-NULL count; a frame in
 * flight. RRT_EUNSUP for a scene with no triangle entry, as rrt_trace_all gives. The call leaves the handle as it was (a frame rendered before and
 * after is the same frame).
 * Not provided: sphere candidates, per-column counts, distances or the blocking primitive (that is rrt_trace_all), a per-pair weight or form-factor
 * kernel, a _begin / _end form.
 * Measured (tools/visibility_time.py, profiles/visibility_time.json; config 4, fp32, everything in device memory, one MI355X):
 * 4 096 x 4 096 atlas sites lifted 1e-3 of the extent (16.8 M pairs, 8.8 % visible), bits and count: 15.1 ms (0.90 ns per pair) against 45.0 ms for
 * the only route the parent commit offers - torch builds the same segments, rrt_trace_all with k = 0 in chunks of 2^22 rays, torch packs
 * count == 0 - (0.34 x); 65 536 sites x 256 directions of the upper hemisphere with RRT_VIS_FACING_A (68.6 % visible): 10.4 ms against 17.5 ms
 * (0.59 x; the route gives pairs that fail the facing test a zero direction, which costs it no walk). Both routes leave the same words and counts,
 * bit for bit. The time is the kernel's: the device time of a call is 99.9 % of its wall time. One rrt_trace_any pass over the same segments,
 * without building or packing anything, takes 7.2 / 5.0 ms - it is the reference's shadow ray on the pair-node tree with the fast reciprocal, and it
 * answers otherwise on 7.3 % / 1.9 % of the pairs (Q9 - Q11). count comes from one atomicAdd per word; a per-row reduction was not measured, nor was
 * refilling idle lanes. bench.py (23.10 / 23.01 / 23.10 ms per frame) is the parent build's (22.85 / 23.31 / 22.98), run alternately. */
enum { RRT_VIS_MATRIX = 0, RRT_VIS_PAIRS = 1 };           /* mode */
enum { RRT_VIS_POINTS = 0, RRT_VIS_DIRECTIONS = 1 };      /* b_kind */
enum { RRT_VIS_FACING_A = 1, RRT_VIS_FACING_B = 2 };      /* flags */
typedef struct rrt_vis_params {
  int32_t mode, b_kind; uint32_t flags; int32_t pad;
  double offset_a, offset_b;          /* rounded to the handle's type R */
  const int32_t *skip_a, *skip_b;     /* may be NULL; n_a / n_b entries of prim_order (as rrt_rays.skip_prim), -1 = none; in a->mem */
} rrt_vis_params;                     /* NULL = {MATRIX, POINTS, 0, 0, 0, NULL, NULL} */
typedef struct rrt_vis_out {
  int32_t mem, pad;
  uint64_t* bits;                     /* MATRIX: n_a * words, words = (n_b + 63) / 64; PAIRS: (n_a + 63) / 64 */
  uint32_t* count;                    /* MATRIX: n_a, visible columns of row i; may be NULL. PAIRS: must be NULL */
} rrt_vis_out;
int rrt_visibility(rrt_handle*, const rrt_points* a, size_t n_a, const rrt_points* b, size_t n_b,
                   const rrt_vis_params* params, rrt_vis_out* out);

/* Multi-GPU film partition: the same, for the rows of the interleaved 16-row tile bands b with
 * b % world == rank (tile height of integrator/mod.rs:55), rendered as one pixel set. Box filter: the ranks' films are
 * disjoint; wider filters: a sample's splat may land in a neighbour's rows of this rank's film. Either way summing
 * the ranks' films (one RCCL reduce) reassembles Film::pixels. */
int rrt_render_bands(rrt_handle*, int rank, int world, void* film_xyzw, int film_mem, rrt_render_stats* stats);

/* Frames in flight (no counterpart in the reference, whose si_render returns with the frame done): _begin enqueues
 * rrt_render_bands on the handle's stream for a DEVICE film and returns; _end waits for that frame and reports what
 * rrt_render_bands would have returned (RRT_EPANIC ...). One frame per handle; a second handle on the same GPU can
 * render the next frame meanwhile, which hides the latency-bound last bounces of one frame behind the camera rays of
 * the next. The film must stay untouched by the caller between the two calls. For the frames of two handles to overlap,
 * both need rrt_set_option("nonblocking_streams", 1): the handle's streams then no longer synchronise with the legacy
 * default stream, so work the caller issued there on the film (a memset ...) must be finished before _begin. */
int rrt_render_bands_begin(rrt_handle*, int rank, int world, void* film_xyzw_device);
int rrt_render_end(rrt_handle*);
/* the same, and the frame's statistics; kernel timings (HIP events on the handle's streams around every launch) are recorded for frames in
 * flight when the option "frame_stats" is 1 */
int rrt_render_end_stats(rrt_handle*, rrt_render_stats* stats);

/* First-hit feature buffers (no counterpart in the reference): what a denoiser or compositor wants beside the film - albedo, normal and
 * depth of the camera rays' first hits, filtered by the film's own pixel filter. The pass runs over exactly the camera samples
 * rrt_render_rect takes for the rect's pixels (same sampler, sample_num 1..nsamp-1, same p_film); rank / world = 0 / 1 takes the whole
 * rect, otherwise the rect's interleaved 16-row bands b % world == rank as rrt_render_bands partitions them; max_samples = 0 takes all
 * samples, k takes sample_num 1..min(k, nsamp-1). Each plane is a full-frame W*H*4 buffer of the handle's precision, added to (+=) like
 * the film, so rects and bands sum to the whole; a wide filter's splats across a rect / band border land in this call's planes.
 *   live sample: camera weight > 0. Dead samples add nothing (unlike the film's filter_weight_sum, which counts them), and no weight
 *                is tripled on the way out.
 *   fw:          the film's filter weight of the sample at the pixel (box filter of radius 0.5: 1 in the sample's own pixel; every
 *                other filter: FilmTile::add_sample's footprint test and 16 x 16 table, film.rs:77-130).
 *   t:           what rrt_trace_closest reports for the camera ray.
 *   n:           the interaction's geometric normal as the reference holds it after Triangle / Sphere::intersect and the instance
 *                transform (primitives.rs:131-136), normalised (a non-rigid instance leaves it un-normalised); not turned towards the
 *                camera, and taken before any bump_map.
 *   rho:         first-hit reflectance from the material's own parameters, textured ones evaluated at the hit with ZERO differentials
 *                (the pixel's samples do the anti-aliasing), clamped to >= 0 where the material clamps: Matte / Plastic / Translucent
 *                Kd, Mirror Kr, Glass (1, 1, 1), Metal ((eta - 1)^2 + k^2) / ((eta + 1)^2 + k^2) per channel, Debug (0, 1, 1).
 * A live sample that misses the scene adds only fw to albedo[3]. The handle is left as it was (a frame rendered before and after is
 * the same frame). Errors: RRT_EINVAL for NULL arguments, all planes NULL, a rect outside the film, bad rank / world, a precision that
 * is not the handle's, or a frame in flight; RRT_EUNSUP / RRT_EPANIC as rrt_render_rect gives for the scene. */
typedef struct rrt_aov {
  int32_t mem;        /* RRT_MEM_* of the planes                                  */
  int32_t precision;  /* must equal the handle's                                  */
  void* albedo;       /* W*H*4: sum fw*rho.r, .g, .b | sum fw   over live samples  */
  void* normal;       /* W*H*4: sum fw*n.x, .y, .z   | sum fw   over hit samples   */
  void* depth;        /* W*H*4: sum fw*t, sum fw*t*t, sum fw over hit samples, 0  */
} rrt_aov;            /* any plane may be NULL (not produced); all NULL = RRT_EINVAL */
int rrt_render_aov(rrt_handle*, const int32_t rect[4], int rank, int world, uint64_t max_samples, rrt_aov* out);

/* Ambient occlusion and bent normals beside the film: what AOIntegrator::li (ao.rs:65-96) means, per camera sample. (The reference's own
 * AO frame is black: ao.rs:74 asks the tile sampler for a 2D array only the throw-away pre_sampler requested, Q30 - and a frame of an AO
 * scene stays black here too. This call is the pass itself, on scenes of every integrator type.) Which samples run is rrt_render_aov's,
 * word for word: the camera samples rrt_render_rect takes for the rect's pixels, rank / world = bands, max_samples, live = camera weight
 * > 0, fw = the film's own filter weight, full-frame W*H*4 planes of the handle's precision in host or device memory, added to (+=), no
 * Q2 and no Q3 tripling, and the handle is left as it was. Per live sample whose camera ray (o, d) hits, with the interaction's fields
 * as they are after the instance transform:
 *   n_g = the geometric normal (not normalised under a non-rigid instance), n = faceforward(n_g, -d), s = normalize(dpdu) with the
 *   GEOMETRIC dpdu (triangle.rs:268-293 / sphere.rs, not shading.dpdu), t = cross(n_g, s) - the un-flipped normal, as ao.rs:76 has it;
 *   draw i = 0 .. n_samples-1: u_i = the i-th get_2d() of the sample's stream after get_camerasample (HaltonSampler: dimensions 5 + 2i
 *   and 6 + 2i of the sample's index); wi_local = cosine_sample_hemisphere(u_i), pdf = |z| / pi (cos_sample != 0) or
 *   uniform_sample_hemisphere(u_i), pdf = 1 / (2 pi) (sampling.rs:245-303); wi = s x + t y + n z; the ray isect.spawn_ray(wi): origin p,
 *   direction d_i = normalize(wi), t_max = inf (Q8), traced as the integrators' spawned rays are (in fp32: start triangle excluded,
 *   double-float origin) and answered by BVHAccel::intersect_p (Q11 included); a free ray adds a_i = dot(wi, n) / (pdf * n_samples).
 *   A draw with pdf == 0 (cosine mode, z == 0) is dropped: ao.rs would form 0 / 0 there.
 *   a = sum a_i in draw order, b = sum a_i * d_i over the free rays. The reference's scale is kept: a fully open point has a = pi in
 *   cosine mode (resolve_ao in Python divides by pi and by the weights).
 * Cost (config 4 at 1024^2, fp32, device planes, max_samples 8, 16 draws, profiles/ao_time.json): 11.3 ms against 2.25 ms for rrt_render_aov over
 * the same samples; 7.6 ms of it are the 16 any-hit launches (21.7 M rays, 2.85 G rays/s), 1.4 ms the 16 launches that make the rays.
 * No distance limit is offered: under Q9 / Q10 t_max prunes boxes and nothing else. Errors, before any device work: RRT_EINVAL for NULL
 * arguments, both planes NULL, n_samples outside 1 .. 256 (5 + 2 n stays below the sampler's 1000 dimensions), a rect outside the film,
 * bad rank / world, a precision that is not the handle's, or a frame in flight; RRT_EUNSUP, the reason named, for the StratifiedSampler
 * (its draws past `dimension` are the [-1, 1) generator of Q25); RRT_EUNSUP / RRT_EPANIC as rrt_render_aov gives for the scene. */
typedef struct rrt_ao_params { int32_t n_samples; int32_t cos_sample; } rrt_ao_params;
void rrt_ao_defaults(const rrt_handle*, rrt_ao_params*);   /* the scene's Integrator.{n_samples, cos_sample} where its type is AO, else 64 / 1 */
typedef struct rrt_ao {
  int32_t mem;        /* RRT_MEM_* of the planes                                                                     */
  int32_t precision;  /* must equal the handle's                                                                     */
  void* ao;           /* W*H*4: sum fw*a, sum fw*a*a, sum fw over hit samples, sum fw over live samples               */
  void* bent;         /* W*H*4: sum fw*b.x, .y, .z, sum fw over hit samples                                           */
} rrt_ao;             /* either plane may be NULL (not produced); both NULL = RRT_EINVAL */
int rrt_render_ao(rrt_handle*, const int32_t rect[4], int rank, int world, uint64_t max_samples,
                  const rrt_ao_params* params /* NULL = rrt_ao_defaults */, rrt_ao* out);

/* Feature buffers through mirrors and glass (no counterpart in the reference): rrt_render_aov's planes with the record of the first
 * non-specular surface along the chain of perfectly specular bounces a camera ray starts - what a denoiser wants on a wall mirror or a
 * window, which first-hit planes show as one flat surface. rect, rank / world, max_samples, the planes' layout, the += semantics, live
 * samples, fw and "the handle is left as it was" are rrt_render_aov's. max_follow = 0..16 is the longest chain followed. Per live sample
 * with camera ray (o, d):
 *   state:   k = 0, throughput thr = (1, 1, 1), path length T = 0.
 *   segment: segment k is traced as rrt_trace_closest would. In fp32 the triangle the segment starts on is excluded, as the frame's spawned
 *            rays exclude it; f64 keeps the reference's behaviour (the origin's own triangle is met at t ~ 1e-15 and refused by t < 1e-7).
 *   miss:    at k = 0 a live miss: it adds only fw to albedo[3]. At k > 0 the sample keeps the record of surface k - 1.
 *   hit:     at t on surface S: T += t; n = the normalised geometric normal, exactly rrt_render_aov's; rho_S from rrt_render_aov's table
 *            (textured parameters with zero differentials). The sample's record becomes {thr * rho_S, n, T}, and it counts as a hit sample
 *            in all three planes from here on, whatever later segments do.
 *   follow:  S is followed iff k < max_follow and one of these rules applies. sn = the shading normal as the reference holds it after
 *            Triangle / Sphere::intersect and the instance transform, before any bump_map; clamp0 = every channel clamped to >= 0.
 *              Mirror: tint = clamp0(Kr), not black; d' = d - 2 (d . sn) sn.
 *              Glass with u_roughness == 0 && v_roughness == 0 at the hit, before any remap (glass.rs:74): eta = "index" at the hit;
 *                refract() of reflection.rs:122-134 with wo = -d, entering = wo . sn > 0, the ratio 1 / eta when entering and eta when
 *                leaving, the normal turned towards wo. If a refracted direction exists and clamp0(Kt) is not black: d' = that direction,
 *                tint = clamp0(Kt). Otherwise d' as for Mirror with tint = clamp0(Kr), if that is not black (total internal reflection).
 *              Rough glass, every other material and a black tint end the chain on S.
 *            On follow: thr *= tint, o' = the hit point exactly (spawn_ray applies no offset, Q8), d' normalised, k += 1.
 * The planes receive the final record as rrt_render_aov's receive theirs: albedo holds the tinted reflectance of the last surface on the
 * chain, depth the path length T and its square. max_follow = 0 adds bit for bit what rrt_render_aov adds, and for every max_follow the
 * three weight channels (albedo[3], normal[3], depth[2]) are bit for bit rrt_render_aov's: the same fw in the same order.
 * A specular *sphere* starts its follow ray under sphere.rs's epsilon-free self-hit test: its chain carries the
 * reference's own coin in f64 and the known bias in fp32.
 * Not provided: a fused form inside rrt_render_frame_aov, an adaptive form, _begin / _end.
 * Errors: rrt_render_aov's, and RRT_EINVAL for max_follow > 16 (before any device work). */
int rrt_render_aov_follow(rrt_handle*, const int32_t rect[4], int rank, int world, uint64_t max_samples, uint32_t max_follow, rrt_aov* out);

/* Denoiser (no counterpart in the reference): an edge-avoiding a-trous wavelet filter over a film, guided by the three planes of rrt_render_aov, with
 * albedo demodulation and a luminance edge-stop scaled by a spatially estimated variance that the iterations carry along (the spatial half of SVGF).
 * film_xyzw and the planes are full-frame W*H*4 sums of the handle's precision, exactly as rrt_render_rect / rrt_render_aov leave them, all in
 * aov->mem (host or device); film_out is a film in the film's own layout (rrt_resolve_rgba8, rrt_film_gather take it as they take a frame) and
 * may be film_xyzw. Rects and bands are summed by the caller first: the filter takes the whole frame.
 *   per pixel p:  w = film[3], data = w > 0, rgb = xyz_to_rgb(film[:3] / w) (spectrum.rs:2075-2090, the matrices of rrt_resolve_rgba8);
 *                 a = albedo[:3] / albedo[3] (0 where albedo[3] == 0); w_hit = depth[2], hit = w_hit > 0, z = depth[0] / w_hit,
 *                 sd = sqrt(max(0, depth[1] / w_hit - z z)); n = normal[:3] / |normal[:3]| (0 where the length is 0);
 *                 d = max(a, 1e-3) per channel when `demodulate`, else 1; c = rgb / d; l = 0.212671 c.r + 0.715160 c.g + 0.072169 c.b.
 *   g(p, q):      0 if hit_p != hit_q, 1 if neither is hit, else max(0, n_p . n_q)^sigma_normal. A tap q is usable inside the frame where data_q.
 *   variance:     over the usable taps of the 7 x 7 window around p, centre included, weights g: v_p = max(0, sum g l_q^2 / sum g - (sum g l_q / sum g)^2)
 *                 (0 where sum g == 0).
 *   iteration i = 0 .. iterations - 1, step s = 2^i:
 *                 gv_p = sum k g v_q / sum k g over the usable taps of the 3 x 3 window at step 1, k = [1,2,1] x [1,2,1] (v_p where the sum is 0);
 *                 the 25 taps q = p + s (dx, dy), dy outer, dx inner, both -2 .. 2 ascending, h = [1/16, 1/4, 3/8, 1/4, 1/16]:
 *                 W = h[dy] h[dx] g(p, q) w_z w_l for usable taps, g = w_z = w_l = 1 at the centre;
 *                 w_z = exp(-|z_p - z_q| / (sigma_depth (max(|dx|, |dy|) s sd_p + 1e-3 z_p))) where both are hit, else 1;
 *                 w_l = exp(-|l_p - l_q| / (sigma_color sqrt(gv_p) + 1e-3 |l_p| + 1e-30)), 1 for sigma_color <= 0;
 *                 c'_p = sum W c_q / sum W, v'_p = sum W^2 v_q / (sum W)^2, l from c'. Pixels without data keep c, v and are never a tap.
 *   finish:       film_out[:3] = rgb_to_xyz(c d) w, film_out[3] = w (copied); a pixel without data is copied through unchanged.
 * No weight carries an absolute radiance scale. The per-pixel steps before and after the iterations run in double in both precision modes.
 * The handle is left as it was; its work buffers are allocated by the first call. Errors: RRT_EINVAL for a NULL aov, a NULL plane, bad mem,
 * iterations outside 1 .. 6, sigma_normal or sigma_depth not > 0, a NULL film, film_out or handle, a precision that is not the handle's, or a
 * frame in flight - each with its own message, the first seven before any device work. */
typedef struct rrt_denoise_params { int32_t iterations; int32_t demodulate; double sigma_color, sigma_normal, sigma_depth; } rrt_denoise_params;
void rrt_denoise_defaults(rrt_denoise_params*);   /* iterations 5, demodulate 1, sigma_color 4, sigma_normal 32, sigma_depth 8 */
int rrt_denoise(rrt_handle*, const void* film_xyzw, const rrt_aov* aov, const rrt_denoise_params* params /* NULL = defaults */, void* film_out);

/* Sample-variance plane beside the film (no counterpart in the reference, whose FilmTile keeps only the sums): the frame of rrt_render_rect
 * (rank / world = 0 / 1) or of the rect's interleaved 16-row bands b % world == rank, partitioned as rrt_render_aov partitions them, and per
 * film pixel the weighted moments of its samples' luminance. film_xyzw is added to (+=) with the very bits, all four channels, that
 * rrt_render_rect / rrt_render_bands would have added, and the statistics hold the same camera_rays, closest_queries, any_queries,
 * root_culled and sky_culled. `moments` is a second full-frame W*H*4 plane of the handle's precision in the same `mem`, also added to (+=):
 *     { S1 = sum fw y,  S2 = sum fw y^2,  S0 = sum fw,  S3 = sum fw^2 }
 * over EVERY sample of the frame whose filter footprint covers the pixel - dead samples (camera weight 0) included with y = 0, because the
 * film's filter_weight_sum counts them (Q2).
 *   fw:  the film's filter weight of the sample at the pixel (box filter of radius 0.5: 1 in the sample's own pixel; every other filter:
 *        FilmTile::add_sample's footprint test and 16 x 16 table, film.rs:77-130, as rrt_render_aov's fw).
 *   y:   (0.212671 L.r + 0.715160 L.g + 0.072169 L.b) w = 0.212671 (L.r w) + 0.715160 (L.g w) + 0.072169 (L.b w) up to rounding, L the
 *        sample's radiance after the film's own NaN / negative / infinity / max_sample_luminance handling (integrator/mod.rs:105-122), w the
 *        camera weight.
 * So S1 is the film's Y channel up to rounding and S0 the film's weight channel / 3 (Q3); for the box filter of radius 0.5 S0 = S3 = the
 * sample count. The plane is a plain sum: rects, bands and ranks add up, a wide filter's splats across a border land in this call's plane as
 * they do in its film, and a pixel's sums do not depend on how the frame was cut into pool passes (samples are added in sample order).
 * A moments frame renders as with the option film_records 0 (per-slot radiance layout), which changes no bit of the film. The handle is left
 * as it was. Errors: RRT_EINVAL, each with its own message, for a NULL handle, rect, film or moments and a bad mem (before any device
 * work), bad rank / world, a rect outside the film, a frame in flight; otherwise what rrt_render_rect gives for the scene. There is no
 * _begin / _end form. */
int rrt_render_moments(rrt_handle*, const int32_t rect[4], int rank, int world, void* film_xyzw, void* moments, int mem,
                       rrt_render_stats* stats /* may be NULL */);

/* The moments frame and its feature buffers from one camera pass (no counterpart in the reference): everything rrt_denoise_moments reads, from
 * one call. film_xyzw and moments are added to (+=) with the very bits rrt_render_moments(h, rect, rank, world, film_xyzw, moments, mem, stats)
 * adds, and the statistics hold the same camera_samples, camera_rays, closest_queries, any_queries, root_culled, sky_culled, tile_launches and
 * list_launches; `moments` may be NULL (the plane is not produced; the film is still the moments frame's). The non-NULL planes of `aov` are
 * added to (+=) with the very bits rrt_render_aov(h, rect, rank, world, aov_max_samples, aov) adds: aov->mem must equal mem, aov->precision the
 * handle's, and aov_max_samples has rrt_render_aov's meaning (0 takes all samples, k takes sample_num 1..min(k, nsamp-1)) - the frame always
 * takes all of its samples. Where the frame's passes begin with a closest-hit launch over the camera rays (the Path integrator; DirectLighting
 * and Debug on scenes without transmissive or textured materials) the first hits are shaded from that launch's queue and no camera ray is traced
 * twice; a camera ray the frame's root cull answered is the miss it is. Every other scene renders the frame and then rrt_render_aov's own
 * pass: the interface is total and the bits are the same. The handle is left as it was. Errors: the union of the two calls', each with its own
 * message - RRT_EINVAL for a NULL handle, rect, film or aov, all planes NULL, a bad mem and aov->mem != mem (all before any device work), bad
 * rank / world, a rect outside the film, a precision that is not the handle's, a frame in flight; otherwise what rrt_render_rect gives for the
 * scene. There is no _begin / _end form and no adaptive form: rrt_render_adaptive keeps its signature and hands out no feature buffers. */
int rrt_render_frame_aov(rrt_handle*, const int32_t rect[4], int rank, int world, void* film_xyzw, void* moments /* may be NULL: plane not produced */,
                         int mem, uint64_t aov_max_samples, rrt_aov* aov, rrt_render_stats* stats /* may be NULL */);

/* rrt_denoise with the variance of the pixels' means taken from the plane of rrt_render_moments (summed over rects / bands by the caller, in
 * aov->mem) where a pixel has one: the same prepare, iterations, finish and argument checks, and RRT_EINVAL for a NULL moments. Only the
 * `variance` step differs. Per pixel p with data, in double in both precision modes:
 *   n_eff = S0^2 / S3 (0 where S3 <= 0);
 *   where n_eff >= 2 and S1 > 0:  rel = max(0, (S2 / S1) (S0 / S1) - 1) (= S2 S0 / S1^2 - 1; no square of a tiny S1),  v_p = l_p^2 rel / (n_eff - 1), l_p the luminance of the stored c record
 *                 (what the spatial estimate reads), the product rounded once to the record type: the variance of the pixel's mean, carried
 *                 to demodulated units by its relative size - no weight carries an absolute radiance scale, and Q3's tripling cancels;
 *   elsewhere:    rrt_denoise's 7 x 7 spatial estimate, unchanged (every sample black, fewer than two effective samples, an empty plane). */
int rrt_denoise_moments(rrt_handle*, const void* film_xyzw, const rrt_aov* aov, const void* moments,
                        const rrt_denoise_params* params /* NULL = defaults */, void* film_out);

/* Error map of a sample-variance plane (no counterpart in the reference). `moments` is a full-frame W*H*4 plane of the handle's precision in `mem`,
 * as rrt_render_moments leaves it; the rect is cut into 8 x 8-pixel tiles anchored at its origin (width and height multiples of 8), numbered
 * row-major within the rect, t = ty * (rw / 8) + tx, and tile_error (in `mem`) receives (rh / 8) * (rw / 8) doubles. Per pixel, in double in both
 * precision modes (resolve_moments of the Python layer):
 *   n_eff = S0^2 / S3 (0 where S3 <= 0);   m = S1 / S0 (0 where S0 <= 0);   v = max(0, S2 / S0 - m^2) / (n_eff - 1) where n_eff >= 2, else 0.
 * Per tile: M = sum m, V = sum v over its 64 pixels, E = sqrt(V / 64) / (M / 64) where M > 0, else 0: the RMS standard error of the pixels' means
 * relative to the tile's mean luminance. No weight carries an absolute radiance scale. The handle is left as it was. Errors: RRT_EINVAL, each with
 * its own message, for a NULL handle, moments, rect or output, a bad mem and a rect that is not whole tiles (all before any device work), a rect
 * outside the film, a frame in flight. */
int rrt_tile_error(rrt_handle*, const void* moments, int mem, const int32_t rect[4], double* tile_error /* in mem */);

/* Adaptive sampling (no counterpart in the reference, which spends nsamp - 1 samples on every pixel): the frame of rrt_render_moments over the rect,
 * except that an 8 x 8 tile (numbered as rrt_tile_error numbers them) stops taking samples once its error E falls below `threshold`.
 *   K = min(max_samples ? max_samples : nsamp - 1, nsamp - 1).
 *   round 0:      sample numbers 1 .. k0, k0 = min(min_samples, K), of every pixel of the rect;
 *   after a round: every tile still active gets rrt_tile_error's E from this call's own running moments (not from what the caller's plane held). A
 *                 tile with E < threshold (strict: threshold 0 stops nothing and gives the uniform frame) stops; an all-black tile has E = 0;
 *   next round:   the next min(batch, K - k) sample numbers of the active tiles only; until no tile is active or k == K.
 * Halton sample k of a pixel does not depend on nsamp and a pixel's sums are added in sample order, so a tile that stopped at k holds in film and
 * moments, bit for bit, what a frame with nsamp = k + 1 holds there. film_xyzw and moments are added to (+=) as rrt_render_moments adds them;
 * tile_samples (in `mem`, may be NULL) receives each tile's final sample count; the statistics hold the sums over the rounds, camera_samples =
 * 64 * sum tile_samples. The handle is left as it was. Errors: as rrt_render_moments, and RRT_EINVAL before any device work for min_samples < 2,
 * batch < 1, a negative or NaN threshold, a rect that is not whole tiles; RRT_EUNSUP, the reason named, for the StratifiedSampler (a prefix of a
 * stratified pixel is not a smaller stratified pixel) and for every pixel filter but the box filter of radius 0.5 (splats across tiles with
 * different counts). There is no rank / world form and no _begin / _end form. */
typedef struct rrt_adaptive_params { uint32_t min_samples, batch, max_samples; double threshold; } rrt_adaptive_params;
void rrt_adaptive_defaults(rrt_adaptive_params*);   /* min_samples 16, batch 16, max_samples 0 (= nsamp - 1), threshold 0.05 */
int rrt_render_adaptive(rrt_handle*, const int32_t rect[4], const rrt_adaptive_params* params /* NULL = defaults */, void* film_xyzw, void* moments,
                        uint32_t* tile_samples /* may be NULL */, int mem, rrt_render_stats* stats /* may be NULL */);

/* Light-group and bounce passes beside the film (no counterpart in the reference, whose PathIntegrator::li returns one sum): the frame of
 * rrt_render_rect (rank / world = 0 / 1) or of the rect's interleaved bands, partitioned as rrt_render_moments partitions them, and per pass a
 * film of the part of every sample's radiance that the pass selects. Path integrator only.
 *   vertex b:  the value of `bounces` in PathIntegrator::li (path.rs:51-226) when uniform_sample_one_light runs: 0 is the camera ray's hit.
 *              Specular vertices count and have no next-event term.
 *   light ln:  the light uniform_sample_one_light picked (integrator/mod.rs:359-401); its group is light_group[ln], or min(ln, 31) for a NULL
 *              light_group.
 *   pass k:    per sample the sum, in vertex order, of the terms beta * Ld / light_pdf that the frame adds to L (estimate_direct's unoccluded
 *              terms; emission is 0, Q18) with bit light_group[ln] set in passes[k].groups and bounce_lo <= b < bounce_hi (bounce_hi <= 0: no
 *              upper end). A term may count for several passes or for none.
 * The pass radiance goes through the film exactly as L does: the NaN / negative / infinity handling of integrator/mod.rs:105-122, the camera
 * weight, the pixel filter, dead samples adding filter weight (Q2), the weight tripled (Q3). So every pass film carries the frame's own weight
 * channel, and rrt_resolve_rgba8, rrt_denoise and rrt_film_gather take a pass film as they take a frame. passes[k].film_xyzw is a full-frame
 * W*H*4 film of the handle's precision in `mem`, added to (+=); rect, rank / world and += are rrt_render_moments'. film_xyzw, when not NULL,
 * is added to with the very bits rrt_render_rect / rrt_render_bands add, and the statistics hold the same camera_samples, camera_rays,
 * closest_queries, any_queries, root_culled and sky_culled: no ray is traced twice, and tile trees, lens cull, root and horizon cull and
 * shadow lists stay on. A pass with groups = ~0u and no bounce limits holds the frame's bits; passes that partition the (group, vertex) pairs
 * sum to the frame up to the rounding of the sums. A passes frame renders as with the option film_records 0 (per-slot radiance layout, as a
 * moments frame), which changes no bit of the film. The handle is left as it was; the radiance planes (16 bytes per pass and pool slot) are
 * allocated by the first call and bound the size of a pool pass.
 * Errors, each with its own message: RRT_EINVAL before any device work for a NULL handle, rect or passes, n_passes outside 1 .. RRT_MAX_PASSES,
 * a NULL pass film, a bad mem, bounce_lo < 0 and a light_group entry >= 32; RRT_EINVAL for a rect outside the film, bad rank / world, a frame in
 * flight; RRT_EUNSUP, the reason named, for every integrator but Path and for a finite Film.max_sample_luminance (its clamp depends on the
 * whole sample's luminance, so the passes would no longer add up); otherwise what rrt_render_rect gives for the scene.
 * Not provided: a _begin / _end form, an adaptive form, moments per pass. */
#define RRT_MAX_PASSES 16
typedef struct rrt_pass {
  uint32_t groups;               /* bit g set: NEE terms of lights in group g count */
  int32_t  bounce_lo, bounce_hi; /* ... at path vertices lo <= b < hi; hi <= 0 means no upper end */
  void*    film_xyzw;            /* full-frame W*H*4, handle precision, added to (+=) */
} rrt_pass;
int rrt_render_passes(rrt_handle*, const int32_t rect[4], int rank, int world,
                      const uint8_t* light_group /* n_lights entries, each < 32; NULL: light i is in group min(i, 31) */,
                      const rrt_pass* passes, int n_passes,
                      void* film_xyzw /* may be NULL */, int mem, rrt_render_stats* stats /* may be NULL */);

/* Relighting from pass films (no counterpart in the reference). films[k] are n full-frame W*H*4 films of the handle's precision in `mem`, as
 * rrt_render_passes leaves them; gains_rgb holds n RGB triples. Per pixel
 *     film_out[:3] = sum_k rgb_to_xyz(gains[k] * xyz_to_rgb(films[k][:3])),
 *     film_out[3]  = films[0][3],
 * rgb_to_xyz the table a film's RGB sums were merged with (spectrum.rs:2084-2090) and xyz_to_rgb its inverse, taken in double. That inverse
 * agrees with the six-digit xyz_to_rgb table of spectrum.rs:2075-2082 (rrt_resolve_rgba8's) to 1.4e-6, which is how far the two tables are from
 * being inverses of each other; with the inverse, unit gains return the sum of the films and gains g the frame of the scene whose lights' spectra
 * are scaled by g, to the rounding of the arithmetic (through the six-digit table: to 5e-7 of the frame's largest value). Computed in double in both precision modes, on the device for both memory kinds (host films are staged). film_out is overwritten, not added
 * to, and may be one of the inputs. The handle is left as it was. Errors: RRT_EINVAL, each with its own message, for a NULL handle, films,
 * films[k], gains_rgb or film_out, n outside 1 .. RRT_MAX_PASSES and a bad mem, all before any device work. */
int rrt_combine_passes(rrt_handle*, const void* const* films, const double* gains_rgb /* n x 3 */, int n, void* film_out, int mem);

/* ID mattes beside the film (no counterpart in the reference): which object each pixel shows - per pixel a table of K (id, coverage) slots, the
 * filtered coverage of the ids its camera samples hit first, ranked (the information a Cryptomatte layer carries), and a weight record to
 * normalise it. The call takes exactly the camera samples rrt_render_aov(h, rect, rank, world, max_samples, ...) takes; live samples, fw and the
 * first hit (what rrt_trace_closest reports for the camera ray) are rrt_render_aov's. ids, coverage and weight are full-frame buffers in `mem`.
 *   id of a hit sample: prim_id[prim_order[hit.prim]] - the caller's value for the primitive that was hit, any uint32_t; with prim_id == NULL,
 *                prims[prim_order[hit.prim]].material + 1.
 *   table rule:  a pixel's table is its K slots in stored order; a slot is empty when its coverage is 0. The call reads the caller's table,
 *                continues it and writes it back (zeroed buffers are an empty table). For every live sample with fw != 0 that covers the pixel, in
 *                arrival order: weight[0] += fw; if it hit something, weight[1] += fw, and then a non-empty slot holding its id takes += fw,
 *                otherwise the first empty slot takes (id, fw), otherwise weight[2] += fw (overflow). Nothing is ever evicted: every coverage
 *                stored by a call on zeroed buffers is its id's complete sum, sum of slots + weight[2] == weight[1] up to rounding (exactly for
 *                the box filter of radius 0.5, whose weights are integers), and a pixel with weight[2] == 0 holds the complete list.
 *   arrival order: box filter of radius 0.5: sample-number order, so the table does not depend on how the frame is cut into pool passes. Every
 *                other filter: the implementation's order - where a pixel meets more than K ids, which K are kept is not specified, only the
 *                identities above are.
 *   on the way out: every pixel's slots are sorted by coverage descending, ties by ascending id; empty slots come last, as (0, 0).
 * Rects and bands of a box-filtered frame touch disjoint pixels, so several calls into one set of buffers give the whole frame's table; a wide
 * filter's splats across a border continue the neighbour's table, which is exact where nothing overflows. Every call reads, ranks and writes
 * the whole W*H*K table whatever the rect (pixels it does not touch are only re-ranked; a host table is staged in and out in full), so a frame
 * cut into n calls pays n times the film's table on top of its samples: prefer few, large calls. The handle is left as it was (a frame
 * rendered before and after is the same frame).
 * Errors, each with its own message: RRT_EINVAL before any device work for a NULL out, ids, coverage, weight, rect or handle, n_slots outside
 * 1 .. RRT_MAX_MATTE_SLOTS and a bad mem; RRT_EINVAL for n_prim_id != n_prims when prim_id is not NULL, a precision that is not the handle's, a
 * rect outside the film, bad rank / world, a frame in flight; otherwise what rrt_render_aov gives for the scene.
 * Not provided: ids through mirrors and glass (a _follow form), a fused form inside rrt_render_frame_aov, _begin / _end, an adaptive form. */
#define RRT_MAX_MATTE_SLOTS 16
typedef struct rrt_mattes {
  int32_t mem;        /* RRT_MEM_* of the three arrays                          */
  int32_t precision;  /* must equal the handle's                                */
  int32_t n_slots;    /* K, 1 .. RRT_MAX_MATTE_SLOTS                            */
  int32_t pad;
  uint32_t* ids;      /* W*H*K  : [pixel][slot]                                 */
  void* coverage;     /* W*H*K  : [pixel][slot], handle precision               */
  void* weight;       /* W*H*4  : sum fw over live samples | over hit samples | overflow | 0 */
} rrt_mattes;
int rrt_render_mattes(rrt_handle*, const int32_t rect[4], int rank, int world, uint64_t max_samples,
                      const uint32_t* prim_id /* n_prim_id entries, indexed like rrt_scene_desc.prims; NULL: material index + 1 */,
                      size_t n_prim_id, rrt_mattes* out);

/* One matte from a table (no counterpart in the reference): alpha[p] = (sum of coverage[p][k] over the slots whose id is in ids[]) / weight[p][0],
 * and 0 where weight[p][0] == 0 - the share of the pixel's live filter weight that the listed ids cover. ids may name absent ids and repeat ids.
 * The arithmetic is in double, rounded once to the handle's precision; it runs on the device for both memory kinds (host arrays are staged).
 * alpha is W*H values of the handle's precision in m->mem, overwritten. On a table without overflow the alphas of a partition of the ids and
 * the miss share 1 - weight[1] / weight[0] sum to 1. The handle is left as it was. Errors, each with its own message: RRT_EINVAL before any
 * device work for a NULL m, ids, coverage, weight, id list, alpha or handle, n_slots outside 1 .. RRT_MAX_MATTE_SLOTS, a bad mem and n_ids
 * outside 1 .. 256; RRT_EINVAL for a precision that is not the handle's or a frame in flight. */
int rrt_matte_extract(rrt_handle*, const rrt_mattes* m, const uint32_t* ids, int n_ids /* 1 .. 256 */, void* alpha /* W*H, handle precision, in m->mem */);

/* ---- multi-GPU film reassembly: RCCL over xGMI, one collective per frame ----
 * The reference has one address space: its rayon tiles merge under a lock (Film::merge_film_tile film.rs:248-263, driven from
 * integrator/mod.rs:64-74,133). Across GPUs every rank renders its bands (rrt_render_bands / _begin) into its own device
 * film and the films meet on `root`. Box filter of radius <= 0.5: the bands are disjoint and only they travel (grouped
 * ncclSend / ncclRecv - a gather: every rank ships 1/world of the film over its direct xGMI link to root); wider filters
 * splat across band borders and the collective is ncclReduce(sum) of the whole film. The call is enqueued on the handle's
 * stream (after the frame it follows) and returns; rrt_render_end() or a stream synchronisation completes it. */

/* rows [y0, y1) of the bands `rank` owns out of `world` (bands b of 16 rows, integrator/mod.rs:55, with b % world == rank).
 * Returns the number of bands and fills up to max_bands {y0, y1} pairs (y0y1 may be NULL); host arithmetic only. */
int rrt_band_rows(int yres, int rank, int world, int32_t* y0y1, int max_bands);

typedef struct rrt_comm rrt_comm;
#define RRT_COMM_ID_BYTES 128
/* one process per GPU: rank 0 draws an id (ncclGetUniqueId) and hands the bytes to the other ranks by any channel it has;
 * every rank then joins (ncclCommInitRank; collective: returns once all `world` ranks have called it) */
int rrt_comm_id(uint8_t id[RRT_COMM_ID_BYTES]);
int rrt_comm_create(const uint8_t id[RRT_COMM_ID_BYTES], int rank, int world, int device, rrt_comm** out);
void rrt_comm_destroy(rrt_comm*);
/* the collective; film_xyzw_device = the W*H*4 device film this rank rendered with (comm rank, comm world) */
int rrt_film_gather(rrt_handle*, rrt_comm*, void* film_xyzw_device, int root);
/* one process that owns all GPUs of the node (the shape of the reference's single binary): handles[i] rendered rank i of
 * n into films_device[i] on its own device; communicators (ncclCommInitAll) are created on first use and kept */
int rrt_film_gather_all(rrt_handle* const* handles, void* const* films_device, int n, int root);

/* Handle options (rrt_set_option). "fp32" = only the RRT_F32 product mode looks at it. Every option marked "invariant" switches a
 * shortcut whose results are identical bit for bit with it on or off (frames, filter weights, query counts); the named test holds that.
 *
 * name                  default   values / meaning                                                              invariant it keeps (test in tests/test_gpu_parity.py)
 * --------------------  --------  ----------------------------------------------------------------------------  ------------------------------------------------------
 * max_paths             2^28      wavefront pool slots (>= 64); clamped to half of the free HBM at creation      frames (fp32: to rounding of the per-pass sums)
 * frame_stats           0         1: frames in flight record kernel timings (rrt_render_end_stats)              -
 * nonblocking_streams   0         1: the handle's streams stop synchronising with the legacy default stream     - (see rrt_render_bands_begin)
 * count_traversal       0         1: exact node / triangle-test counters in rrt_render_stats (generic kernels)  -
 * overlap_shadow        1         0: shadow launches on the main stream instead of a second one                 frames
 * persistent_traversal  3  fp32   0 generic kernels, 1 grid-stride pair-node kernel, 2 persistent-thread kernel, frames: every mode makes the reference's decisions in its
 *                                 3 both by queue size                                                           order (test_trace_modes_agree, sphere / instance tests)
 * pt_split_closest/_any 100000    queue size at which mode 3 switches kernels                                    frames
 * quad_nodes            0  fp32   1: closest-hit rays of the persistent kernel fetch two tree levels at a time   invariant (test_quad_nodes_change_nothing)
 *                                 (128-byte nodes with the four grandchild boxes, visited in the tree's order)
 * tile_order            1         pixels of a pass enumerated in 8 x 8 tiles where the rect is whole tiles      invariant (test_tile_order_of_the_pixels_changes_nothing)
 * tile_trees            1  fp32   camera rays walk per-patch copies of the most visited nodes in LDS;            invariant (test_tile_trees_change_nothing);
 *                                 rrt_render_stats::tile_launches counts those launches                          films above 4096^2 pixels keep the ordinary kernel
 * tt_census             2  fp32   camera samples per pixel of the census that chooses the copied nodes           invariant (same test, two densities)
 * root_cull             1  fp32   path integrator: camera rays that miss the BVH's root box are answered by     invariant (test_root_cull_changes_nothing);
 *                                 the camera kernel (rrt_render_stats::root_culled), never queued                counted in closest_queries
 * shadow_lists          1  fp32   shadow rays towards point / distant / sphere-area lights run down their       invariant (test_shadow_candidate_lists_change_nothing);
 *                                 start triangle's list of candidate leaves (rrt_render_stats::list_launches)    same box and triangle tests
 * sl_grid               32768     workgroup cap of the list kernel                                               frames
 * any_entry             1  fp32   shadow rays that walk the tree start from their triangle's deciding nodes     invariant (test_any_hit_entry_nodes_change_nothing)
 * cam_tables            1  fp32   block tables instead of the digit loops of the camera's Halton dimensions      invariant (test_camera_halton_block_tables_change_nothing)
 * halton_tables         1  fp32   the same for the integrators' first 64 dimensions                             invariant (test_halton_block_tables_change_nothing)
 * raygen_lean           1  fp32   1: dense camera kernels with the lean lens arithmetic; 0: the generic          fp32 camera samples within 1e-3 of the f64 oracle either
 *                                 two-stage kernels in the reference's operation order                           way (test_camera_samples)
 * rg_spb                8  fp32   samples of one 8 x 8 tile per camera workgroup: 1, 2, 4 or 8                   frames
 * aux_margin            1  fp32   skip the auxiliary camera rays (camera.rs:593-620) where the main ray clears   a CALIBRATED HEURISTIC, not a proven bound: 16 x the largest
 *                                 every lens interface by the calibrated margin                                  auxiliary-ray displacement measured at scene load (16 384 host
 *                                                                                                                samples of the scene's own lens); validated bit for bit against
 *                                                                                                                the full traces (test_aux_margins_change_nothing)
 * lens_cull             1  fp32   tiled passes of untextured scenes: camera samples whose (r_film, p_lens) cell   invariant (tests/test_lens_cull.py, tests/test_lens_shapes.py);
 *                                 the host found dead for the scene's lens are dropped before any lens            the table's own promise: tests/test_lens_cull_table.py
 *                                 arithmetic, the survivors packed into whole waves before the first interface
 * horizon_cull          1  fp32   path integrator: a bounce ray whose elevation exceeds everything visible from  invariant (test_horizon_cull_changes_nothing);
 *                                 its start triangle in its azimuth sector (host-built tables) is answered as    counted in closest_queries and sky_culled
 *                                 the miss it is, never queued. The tables are built by rrt_create (host, all
 *                                 cores; ~5 s for 100k triangles, once per geometry and process:
 *                                 rrt_render_stats::s_horizon_build); RRT_HORIZON_TABLES=0 in the environment
 *                                 builds none
 * shade_compact         1         path shading kernel packs the HITS of a chunk of queue entries through LDS       invariant (test_shade_compaction_changes_nothing)
 *                                 before shading them (a miss is shaded with nothing)
 * shade_spec            1  fp32   path shading kernel instantiated for the lobe kinds the scene's materials      same arithmetic per lobe: frames equal to fp32 rounding,
 *                                 can produce; 0: always the general kernel                                      weights and counts identical (test_shading_kernel_specialisation)
 * film_records          1  fp32   path integrator, tile-tree passes, box filter of radius 0.5, untextured:       invariant (tests/test_film_records.py);
 *                                 radiance in per-workgroup record runs read by a run-walking box film;          other passes keep the per-slot layout
 *                                 0: the per-slot layout and k_film_box
 * dn_lds                1         rrt_denoise: 1: the a-trous steps 1 and 2 read their taps from an LDS tile with       invariant (tests/test_denoise.py::test_denoise_lds_changes_nothing)
 *                                 halo (the steps at which that measured faster); 0: direct gathers at every step
 * nearest_pairs         0  fp32   rrt_nearest: 1: the walk on the pair-node tree (LDS treelet and stack; measured     invariant (tests/test_nearest.py::test_invariances, test_tree_shapes)
 *                                 1.4 - 1.5 x slower on config 4); 0: the generic kernel on the linear tree
 */
int rrt_set_option(rrt_handle*, const char* key, double value);

const char* rrt_last_error(void);
const char* rrt_version(void);

#ifdef __cplusplus
}
#endif
#endif /* RRT_H */
