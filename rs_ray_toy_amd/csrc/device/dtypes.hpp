// Device-side data layout (HBM, SoA) for the wavefront path tracer. gfx950 only.
//
// Everything the kernels read is flattened to world space and stored in *traversal order* (ordered_prims
// of bvh.rs:336-357), so a leaf's primitives are contiguous: nodes[i].offset indexes tri arrays directly.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "horizon_build.hpp"   // hz_sector(): shared with the host builder
#include "records.hpp"          // Node, Tri, Material, Light, ... : the plain records, shared with the host scene preparation
namespace rrtd {

template <typename R>
struct SceneDev {
  const Node<R>* nodes;
  const Tri<R>* tris;
  const TriShade<R>* shades;
  const SphereDev<R>* spheres;
  const InstDev<R>* insts;     // non-rigid triangle instances (kInstBase)
  const Material<R>* materials;
  const TexDev<R>* textures;   // texture graph nodes (children before parents)
  const ImageDev<R>* images;
  const R* image_texels;       // RGB triples
  R diff_scale;                // scale_differentials factor 1 / sqrt(samples_per_pixel), integrator/mod.rs:94-96
  const Light<R>* lights;
  const R* light_cdf;          // Distribution1D([1; n]).cdf, n_lights + 1 entries
  uint32_t n_nodes, n_tris, n_lights;
  R light_pick_pdf;            // 1 / (func_int * n)
  uint32_t stack_depth;        // >= bvh depth + 1
  uint32_t flags;
  uint32_t use_shadow_tabs;    // the shading kernel stores Light::shadow_tab with a shadow ray's start triangle (the launch that follows is k_shadow_lists_f32)
  // fp32 path integrator: the camera kernels answer a camera ray that misses the root box themselves (the test lane_ray_begin() makes, on the ray as stored:
  // such a ray is a miss, which the path integrator shades with nothing) instead of sending it through the queue - see camera_ray_meets_root()
  uint32_t root_cull;
  // horizon tables (fp32 path integrator, host/horizon_build.cpp build_horizons()): per triangle 2 x 16 bytes - hemisphere +hz_axis / -hz_axis, 16 azimuth sectors (hz_sector) -
  // holding ceil(254 x sin(max elevation at which anything is visible from any point of the triangle in that sector)) + margin; null = off
  const uint8_t* horizon;
  const float* hz_tau;         // per triangle: the cull applies where min(barycentric) |n.d| > hz_tau (HzTables::tau: the ray's origin is only NEAR its triangle's plane)
  uint32_t hz_axis;
  float root_box[6];
  // camera
  const LensElem<R>* lens;
  int32_t n_lens, simple_weighting;
  R cam_m[12];                 // camera_to_world rows 0..2
  R pupil0[4], pupil63[4];
  R shutter_open, shutter_close;
  // film
  int32_t xres, yres;
  R diagonal, extent[4];
  R max_sample_luminance;
  const R* filter_table;       // 16 x 16 (film.rs:163-173, incl. Q4), only read by the wide-filter film kernel
  R filter_rx, filter_ry;
  R filter_inv_rx, filter_inv_ry;   // 1 / radius (film.rs:43-46), divided on the host: the fp32 build's fast reciprocal is 1 ulp off, and
                               // `distance * inv_radius * 16` sits exactly on table-index boundaries for unjittered strata
  // sampler
  const HaltonDim* hdims;
  uint32_t* err;               // the handle's error word (counters[C_ERROR]): device-side counterparts of the reference's panics
  const uint16_t* perms;
  uint32_t nsamp, sample_at_center;
  uint32_t base_exp0, base_exp1, base_scale0, base_scale1, stride, mult_inv0, mult_inv1;
  uint32_t fast_div;           // all sample indices < 2^26
  // StratifiedSampler (samplers/stratified.rs) with counter-based randomness, see draw_1d() in dmath.hpp
  uint32_t sampler_type;       // RRT_SAMPLER_*
  uint32_t st_nx, st_ny, st_jitter, st_dims, st_seed_lo, st_seed_hi;
  uint32_t cam_db;             // dimension-counter word after the camera sample (Halton: 5; stratified: one 1D, two 2D)
  uint32_t shade_compact;      // k_shade_path packs the hits of a chunk of queue entries before shading them (option "shade_compact")
  uint32_t db_shift;           // a path's queue word = dimension counter(s) | bounce << db_shift: 16 under the HaltonSampler (one counter below 1 000, 65 535 bounces), 24 under the StratifiedSampler (two 12-bit counters, 255 bounces); dmath.hpp db_pack
  // camera lens dimensions 2 and 3 (bases 5 and 7): digit permutation packed 3 bits per digit, and the
  // reference's running product inv_base^k (lowdiscrepancy.rs:204-227) tabulated by the same f64 multiplications
  uint32_t cam_perm[2];
  double cam_invpow[2][16];
  double cam_tail[2];          // inv_base * perm[0] / (1 - inv_base)
  double inv_base_scale1;      // 1 / base_scale1
  double inv3pow[24];          // (1/3)^k by the reference's running product (radical_inverse of dimension 1, lowdiscrepancy.rs:188-202)
  // The digit loops of camera dimensions 1-3 as two table look-ups each (fp32 camera kernel; null = loops): the index is split as
  // hi * B + lo, B = 3^6 / 5^6 / 7^5; cam_lo[w][lo] = the permuted reversal of exactly that many low digits, cam_hi[w][hi] = {permuted
  // reversal of hi's digits, base^(digits of hi), inv_base^(all digits) as the two words of the f64 the loop's table holds} - see halton_cam4()
  const uint32_t* cam_lo[3];
  const uint4* cam_hi[3];
  // the same for the sampler dimensions the integrators draw (dimension < n_hblk; null / 0 = loops)
  const HaltonBlk* hblk;
  const uint32_t* hlo;
  const uint4* hhi;
  uint32_t n_hblk;
  // integrator
  int32_t integrator, max_depth, light_strategy;
  R rr_threshold;
};

// Wavefront pools. One slot = one camera sample of the current pass.
//
// Rays, hits and shadow rays are 16-byte-per-word records stored in QUEUE ORDER (index = position in the queue the
// kernel iterates), not by slot, and so is the path state that changes per bounce (beta, sampler dimension, bounce
// count): every bounce's traversal and shading kernels stream them with coalesced 128-bit loads / stores; the only
// per-slot gather left is the radiance update of an unoccluded shadow ray. (The first version kept rays / hits as 4-byte
// SoA arrays indexed by slot through the queue: 8 + 4 scattered dword accesses per ray, each its own 32/64-B
// request - the PMC write traffic of the closest-hit kernel was 7x its algorithmic bytes.)
// Integers ride in the 4th component as raw bits (never touched by arithmetic).
template <typename R> struct Vec4T;
template <> struct Vec4T<float> { using type = float4; };
template <> struct Vec4T<double> { using type = double4; };

struct alignas(16) QEnt { uint32_t slot, db, index, pad; };   // slot, dimension | bounces << 16, Halton global sample index

template <typename R>
struct Pools {
  using V4 = typename Vec4T<R>::type;
  // rays of q_active (also the public rrt_rays batch): {o.x, o.y, o.z, t_max | packed o_lo}, {d.x, d.y, d.z, skip}
  // skip = triangle (traversal order) a spawned ray starts on, -1 = none (see self_prim())
  // fp32 spawned rays replace t_max (a constant of their queue: inf / 1 - 1e-4) by the packed low word of a double-float
  // origin (pack_lo() / spawn_point() in dkernels.hpp); top bits 11 mark that form (a real t_max is never negative)
  V4 *ray_o, *ray_d;
  V4 *nray_o, *nray_d;   // rays being spawned for q_next (the host swaps them together with the queues)
  V4* hit;               // {t, prim, u, v} for the ray at the same queue position
  V4 *sray_o, *sray_d;   // shadow rays, in shadow-queue order
  V4* sld;               // {Ld.r, Ld.g, Ld.b, slot}: pending contribution of the shadow ray at the same position
  // path state that changes every bounce travels with the queue too (cur / next, swapped with the rays)
  V4 *path, *npath;      // {beta.r, beta.g, beta.b, eta_scale (path.rs:70, 150-162)}
  QEnt *q_active, *q_next;   // {slot, dimension counter (low 16) | bounces (high 16), Halton index, -}
  // per-slot state: only what outlives a path's queue entries
  V4* L;                 // {L.r, L.g, L.b, -}: radiance; touched by unoccluded shadow rays and the film kernel
  R* weight;             // camera ray weight (0 = dead sample: its L is never read)
  V4* samp;              // camera sample {p_film.x, p_film.y, p_lens.x, p_lens.y}: one 128-bit gather per survivor
  uint32_t* hindex;      // Halton index (raygen -> first queue entry)
  uint32_t* pix_off;     // per pixel of the pass, two words: {Halton index of its sample 0, y << 16 | x} (halton_pixel_offset: two 64-bit products and a 64-bit
                         // modulo, the same for all samples of a pixel), filled by k_pixel_offsets before the fp32 sampling kernel
  // camera ray differentials after scale_differentials (scenes with textured materials only, else null):
  // {rx_origin, -}, {rx_direction, -}, {ry_origin, -}, {ry_direction, -} per slot
  V4 *rdx_o, *rdx_d, *rdy_o, *rdy_d;
  uint32_t* counters;    // [0] active, [1] next, [2] shadow, [3] camera rays, [4..] stats
  uint32_t* shadow_count;  // the shadow queue's counter (the path integrator alternates two shadow queues, see render_impl)
  // rrt_render_passes (all null / 0 in every other frame; kept last, so that no other member moves in the kernels' argument blocks)
  uint32_t* smask;         // beside sld, per shadow queue: bit k set = the pending contribution also counts for pass k
  V4* pass_L;              // one radiance plane per pass, each pass_stride slots: plane k of slot s at pass_L[k * pass_stride + s]
  size_t pass_stride;
  // the call's pass table folded per light and per path vertex on the host: the mask of light ln at vertex b is pass_tab[ln] & pass_tab[n_lights + b]
  // (n_lights + max_depth words; bit k of a light's word: its group is in pass k's groups, of a vertex's word: bounce_lo <= b < bounce_hi of pass k)
  const uint32_t* pass_tab;
};

}  // namespace rrtd
