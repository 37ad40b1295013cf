// extern "C" device entry points of include/rrt.h: argument checks, precision dispatch, error mapping.
#include "rrt_impl.hpp"

namespace rrt { void set_last_error(const std::string& msg); void comm_cache_release(int device); }

struct rrt_handle { rrtd::HandleBase* impl; };

namespace {
template <typename F>
int guarded(F&& fn) {
  try { fn(); return RRT_OK; }
  catch (const rrtd::DeviceError& e) { rrt::set_last_error(e.what()); return RRT_EDEVICE; }
  catch (const rrtd::UnsupportedError& e) { rrt::set_last_error(std::string("unsupported: ") + e.what()); return RRT_EUNSUP; }
  catch (const rrtd::PanicError& e) { rrt::set_last_error(std::string("panic: ") + e.what()); return RRT_EPANIC; }
  catch (const std::invalid_argument& e) { rrt::set_last_error(e.what()); return RRT_EINVAL; }
  catch (const std::bad_alloc&) { rrt::set_last_error("out of memory"); return RRT_ENOMEM; }
  catch (const std::exception& e) { rrt::set_last_error(e.what()); return RRT_EINVAL; }
}
}  // namespace

extern "C" {

int rrt_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) { (void)hipGetLastError(); return 0; }
  return n;
}

int rrt_create(int device, const rrt_scene_desc* desc, int precision, rrt_handle** out) {
  if (!desc || !out) { rrt::set_last_error("rrt_create: null argument"); return RRT_EINVAL; }
  *out = nullptr;
  if (precision != RRT_F32 && precision != RRT_F64) { rrt::set_last_error("rrt_create: bad precision"); return RRT_EINVAL; }
  // the desc is checked before anything touches a device (and also where there is none): a caller-filled desc with a bad index or a
  // cyclic BVH must never reach a kernel
  { const int rc = guarded([&]() { rrtd::validate_desc(desc); }); if (rc != RRT_OK) return rc; }
  int n = rrt_device_count();
  if (n <= 0) { rrt::set_last_error("rrt_create: no HIP device visible (this library has no CPU fallback)"); return RRT_EDEVICE; }
  if (device < 0 || device >= n) { rrt::set_last_error("rrt_create: device index out of range"); return RRT_EINVAL; }
  return guarded([&]() {
    rrtd::HandleBase* h = precision == RRT_F32 ? rrtd::make_handle_f32(device, desc) : rrtd::make_handle_f64(device, desc);
    *out = new rrt_handle{h};
  });
}

void rrt_destroy(rrt_handle* h) {
  if (!h) return;
  rrt::comm_cache_release(h->impl->device());   // communicators rrt_film_gather_all cached for this device (rrt_comm.hip)
  delete h->impl;
  delete h;
}

size_t rrt_warning_count(const rrt_handle* h) { return h ? h->impl->warnings.size() : 0; }
const char* rrt_warning(const rrt_handle* h, size_t i) { return (h && i < h->impl->warnings.size()) ? h->impl->warnings[i].c_str() : nullptr; }

void* rrt_stream(rrt_handle* h) { return h ? (void*)h->impl->stream() : nullptr; }

int rrt_trace_closest(rrt_handle* h, const rrt_rays* rays, size_t n, rrt_hits* out) {
  if (!h || !rays || !out) { rrt::set_last_error("rrt_trace_closest: null argument"); return RRT_EINVAL; }
  if (n == 0) return RRT_OK;
  if (n > 0x7fffffffu) { rrt::set_last_error("rrt_trace_closest: batch too large"); return RRT_EINVAL; }
  if (!rays->ox || !rays->oy || !rays->oz || !rays->dx || !rays->dy || !rays->dz || !rays->tmax || !out->t || !out->prim) {
    rrt::set_last_error("rrt_trace_closest: null ray/hit array"); return RRT_EINVAL;
  }
  if (rays->mem != out->mem) { rrt::set_last_error("rrt_trace_closest: rays and hits must live in the same memory kind"); return RRT_EINVAL; }
  return guarded([&]() { h->impl->trace_closest(rays, n, out); });
}

int rrt_trace_any(rrt_handle* h, const rrt_rays* rays, size_t n, uint8_t* occluded) {
  if (!h || !rays || !occluded) { rrt::set_last_error("rrt_trace_any: null argument"); return RRT_EINVAL; }
  if (n == 0) return RRT_OK;
  if (n > 0x7fffffffu) { rrt::set_last_error("rrt_trace_any: batch too large"); return RRT_EINVAL; }
  if (!rays->ox || !rays->oy || !rays->oz || !rays->dx || !rays->dy || !rays->dz || !rays->tmax) {
    rrt::set_last_error("rrt_trace_any: null ray array"); return RRT_EINVAL;
  }
  return guarded([&]() { h->impl->trace_any(rays, n, occluded); });
}

int rrt_camera_samples(rrt_handle* h, const int32_t rect[4], uint64_t s0, uint64_t s1, double* dims5, double* ray_od6, double* weight) {
  if (!h || !rect || !dims5 || !ray_od6 || !weight || s1 < s0) { rrt::set_last_error("rrt_camera_samples: bad argument"); return RRT_EINVAL; }
  return guarded([&]() { h->impl->camera_samples(rect, s0, s1, dims5, ray_od6, weight); });
}

int rrt_sampler_values(rrt_handle* h, const uint32_t* pixel, const uint32_t* sample_num, size_t n, uint32_t first, uint32_t count, uint64_t* index, double* v1, double* v2) {
  auto bad = [&](const char* what) { rrt::set_last_error(std::string("rrt_sampler_values: ") + what); return (int)RRT_EINVAL; };
  if (!pixel || !sample_num || !v1 || !v2) return bad("null argument");
  if (n == 0) return bad("n must be > 0");
  if (n > 0x7fffffffu) return bad("batch too large");
  if (count == 0) return bad("count must be > 0");
  if (!h) return bad("null handle");
  return guarded([&]() { h->impl->sampler_values(pixel, sample_num, n, first, count, index, v1, v2); });
}

int rrt_render_rect(rrt_handle* h, const int32_t rect[4], void* film_xyzw, int film_mem, rrt_render_stats* stats) {
  if (!h || !rect || !film_xyzw) { rrt::set_last_error("rrt_render_rect: null argument"); return RRT_EINVAL; }
  if (film_mem != RRT_MEM_HOST && film_mem != RRT_MEM_DEVICE) { rrt::set_last_error("rrt_render_rect: bad film_mem"); return RRT_EINVAL; }
  return guarded([&]() { h->impl->render_rect(rect, film_xyzw, film_mem, stats); });
}

namespace {
// the caller's own description of its rays, wrong whichever handle it comes with: checked before any device work, each with its own message
int ray_samples_check(const std::string& name, const rrt_ray_samples* r, bool with_stream) {
  auto bad = [&](const char* what) { rrt::set_last_error(name + ": " + what); return (int)RRT_EINVAL; };
  if (!r) return bad("null ray description (rrt_ray_samples)");
  if (r->mem != RRT_MEM_HOST && r->mem != RRT_MEM_DEVICE) return bad("bad mem");
  if (!r->ox || !r->oy || !r->oz || !r->dx || !r->dy || !r->dz) return bad("null ray array");
  int set = 0;
  for (int k = 0; k < 3; k++) set += (r->rxo[k] != nullptr) + (r->rxd[k] != nullptr) + (r->ryo[k] != nullptr) + (r->ryd[k] != nullptr);
  if (set != 0 && set != 12) return bad("ray differentials partly set (all twelve arrays or none)");
  if (with_stream && (!r->pixel || !r->sample_num)) return bad("null pixel or sample_num array");
  return RRT_OK;
}
}  // namespace

int rrt_radiance(rrt_handle* h, const rrt_ray_samples* rays, size_t n, void* rgb4) {
  if (const int rc = ray_samples_check("rrt_radiance", rays, true); rc != RRT_OK) return rc;
  if (!rgb4) { rrt::set_last_error("rrt_radiance: null output"); return RRT_EINVAL; }
  if (n == 0) { rrt::set_last_error("rrt_radiance: n must be > 0"); return RRT_EINVAL; }
  if (n > 0x7fffffffu) { rrt::set_last_error("rrt_radiance: batch too large"); return RRT_EINVAL; }
  if (!h) { rrt::set_last_error("rrt_radiance: null handle"); return RRT_EINVAL; }
  return guarded([&]() { h->impl->radiance(rays, n, rgb4); });
}

namespace {
// rrt_irradiance and rrt_irradiance_rays: the caller's own structs first (wrong whichever handle they come with), everything the host can see
// before any device work, each with its own message; then the handle's checks (precision, a frame in flight, the draw range, the pixels)
int irradiance_entry(const char* fn, rrt_handle* h, const rrt_points* pts, size_t n, uint64_t s0, uint64_t s1, const rrt_irr_params* params, bool rays, void* sums4, void* sh27,
                     void* od6) {
  const std::string name(fn);
  auto bad = [&](const char* what) { rrt::set_last_error(name + ": " + what); return (int)RRT_EINVAL; };
  if (!pts) return bad("null point description (rrt_points)");
  if (pts->mem != RRT_MEM_HOST && pts->mem != RRT_MEM_DEVICE) return bad("bad mem");
  if (!pts->px || !pts->py || !pts->pz) return bad("null point array");
  const int n_normals = (pts->nx != nullptr) + (pts->ny != nullptr) + (pts->nz != nullptr);
  if (n_normals != 0 && n_normals != 3) return bad("normals partly set (all three arrays or none)");
  const int mode = params ? params->mode : (int)RRT_IRR_COSINE;
  const double offset = params ? params->offset : 0.0;
  if (mode != RRT_IRR_COSINE && mode != RRT_IRR_SPHERE) return bad("bad mode (RRT_IRR_COSINE or RRT_IRR_SPHERE)");
  if (!std::isfinite(offset)) return bad("offset must be finite");
  if (mode == RRT_IRR_COSINE && n_normals == 0) return bad("null normals in cosine mode (the hemisphere needs its axis)");
  if (rays) {
    if (!od6) return bad("null output");
  } else {
    if (!sums4) return bad("null output (sums4)");
    if (sh27 && mode != RRT_IRR_SPHERE) return bad("sh27 is a sphere-mode output (mode is RRT_IRR_COSINE)");
  }
  if (n == 0) return bad("n must be > 0");
  if (n > 0x7fffffffu) return bad("batch too large");
  if (s0 < 1 || s0 >= s1) return bad("draw range outside [1, nsamp) or empty");
  if (!h) return bad("null handle");
  return guarded([&]() { h->impl->irradiance(fn, pts, n, s0, s1, mode, offset, sums4, sh27, od6); });
}
}  // namespace

int rrt_irradiance(rrt_handle* h, const rrt_points* pts, size_t n, uint64_t s0, uint64_t s1, const rrt_irr_params* params, void* sums4, void* sh27) {
  return irradiance_entry("rrt_irradiance", h, pts, n, s0, s1, params, false, sums4, sh27, nullptr);
}

int rrt_irradiance_rays(rrt_handle* h, const rrt_points* pts, size_t n, uint64_t s0, uint64_t s1, const rrt_irr_params* params, void* od6) {
  return irradiance_entry("rrt_irradiance_rays", h, pts, n, s0, s1, params, true, nullptr, nullptr, od6);
}

namespace {
// rrt_surface_rays and rrt_surface_at: the caller's own structs first (wrong whichever handle they come with), each with its own message; then the
// handle's checks (precision, a frame in flight, the sites themselves)
int surface_entry(const char* fn, rrt_handle* h, const rrt_rays* rays, const rrt_sites* sites, bool rays_form, size_t n, rrt_surface* out) {
  const std::string name(fn);
  auto bad = [&](const char* what) { rrt::set_last_error(name + ": " + what); return (int)RRT_EINVAL; };
  int in_mem;
  if (rays_form) {
    if (!rays) return bad("null ray description (rrt_rays)");
    if (!rays->ox || !rays->oy || !rays->oz || !rays->dx || !rays->dy || !rays->dz || !rays->tmax) return bad("null ray array");
    in_mem = rays->mem;
  } else {
    if (!sites) return bad("null site description (rrt_sites)");
    if (!sites->prim || !sites->b1 || !sites->b2) return bad("null site array");
    in_mem = sites->mem;
  }
  if (in_mem != RRT_MEM_HOST && in_mem != RRT_MEM_DEVICE) return bad("bad mem");
  if (!out) return bad("null record description (rrt_surface)");
  const int groups[7][2] = {{(out->px != nullptr) + (out->py != nullptr) + (out->pz != nullptr), 3}, {(out->nx != nullptr) + (out->ny != nullptr) + (out->nz != nullptr), 3},
                            {(out->sx != nullptr) + (out->sy != nullptr) + (out->sz != nullptr), 3}, {(out->tu != nullptr) + (out->tv != nullptr), 2},
                            {(out->rho_r != nullptr) + (out->rho_g != nullptr) + (out->rho_b != nullptr), 3}, {out->t != nullptr, 1},
                            {(out->prim != nullptr) + (out->material != nullptr), 2}};
  int set = 0;
  for (const auto& g : groups) {
    if (g[0] != 0 && g[0] != g[1]) return bad("a group of arrays is partly set (p, n, s, uv, rho, t, prim + material: all of a group or none)");
    set += g[0];
  }
  if (set == 0) return bad("no group of arrays asked for (all NULL)");
  if (out->mem != in_mem) return bad(rays_form ? "rays and records must live in the same memory kind" : "sites and records must live in the same memory kind");
  if (n == 0) return bad("n must be > 0");
  if (n > 0x7fffffffu) return bad("batch too large");
  if (!h) return bad("null handle");
  return guarded([&]() { h->impl->surface(fn, rays_form ? rays : nullptr, rays_form ? nullptr : sites, n, out); });
}
}  // namespace

int rrt_surface_rays(rrt_handle* h, const rrt_rays* rays, size_t n, rrt_surface* out) { return surface_entry("rrt_surface_rays", h, rays, nullptr, true, n, out); }
int rrt_surface_at(rrt_handle* h, const rrt_sites* sites, size_t n, rrt_surface* out) { return surface_entry("rrt_surface_at", h, nullptr, sites, false, n, out); }

int rrt_atlas_sites(rrt_handle* h, int32_t aw, int32_t ah, const int32_t* prims, size_t n_list, int mem, int32_t* site_prim, void* b1, void* b2, uint64_t* n_covered) {
  auto bad = [&](const char* what) { rrt::set_last_error(std::string("rrt_atlas_sites: ") + what); return (int)RRT_EINVAL; };
  if (!site_prim || !b1 || !b2) return bad("null output");
  if (aw < 1 || aw > 16384 || ah < 1 || ah > 16384) return bad("atlas size outside 1 .. 16384");
  if (mem != RRT_MEM_HOST && mem != RRT_MEM_DEVICE) return bad("bad mem");
  if (prims && n_list == 0) return bad("an empty candidate list (NULL = every triangle)");
  if (prims && n_list > 0x7fffffffu) return bad("candidate list too large");
  if (!h) return bad("null handle");
  return guarded([&]() { h->impl->atlas_sites(aw, ah, prims, n_list, mem, site_prim, b1, b2, n_covered); });
}

int rrt_nearest(rrt_handle* h, const rrt_points* pts, size_t n, double max_dist, rrt_nearest_out* out) {
  auto bad = [&](const char* what) { rrt::set_last_error(std::string("rrt_nearest: ") + what); return (int)RRT_EINVAL; };
  if (!pts) return bad("null point description (rrt_points)");
  if (!pts->px || !pts->py || !pts->pz) return bad("null point array");
  if (pts->mem != RRT_MEM_HOST && pts->mem != RRT_MEM_DEVICE) return bad("bad mem");
  if (!out) return bad("null output description (rrt_nearest_out)");
  if (!out->prim || !out->b1 || !out->b2) return bad("null output array (dist alone may be NULL)");
  if (out->mem != pts->mem) return bad("points and outputs must live in the same memory kind");
  if (n == 0) return bad("n must be > 0");
  if (n > 0x7fffffffu) return bad("batch too large");
  if (!(max_dist >= 0.0)) return bad("max_dist must be >= 0 (+inf = no limit), not negative or NaN");
  if (!h) return bad("null handle");
  return guarded([&]() { h->impl->nearest(pts, n, max_dist, out); });
}

int rrt_trace_all(rrt_handle* h, const rrt_rays* rays, size_t n, rrt_multi_hits* out) {
  auto bad = [&](const char* what) { rrt::set_last_error(std::string("rrt_trace_all: ") + what); return (int)RRT_EINVAL; };
  if (!rays) return bad("null ray description (rrt_rays)");
  if (!rays->ox || !rays->oy || !rays->oz || !rays->dx || !rays->dy || !rays->dz || !rays->tmax) return bad("null ray array");
  if (rays->mem != RRT_MEM_HOST && rays->mem != RRT_MEM_DEVICE) return bad("bad mem");
  if (!out) return bad("null output description (rrt_multi_hits)");
  if (out->k < 0 || out->k > RRT_MAX_HITS) return bad("k must be 0 .. RRT_MAX_HITS");
  if (out->k > 0 && (!out->t || !out->prim)) return bad("null slot array (t and prim are needed with k > 0)");
  if (out->k > 0 && ((out->b1 == nullptr) != (out->b2 == nullptr))) return bad("b1 and b2 must both be NULL or both be set");
  if (out->k == 0 && !out->count) return bad("k == 0 needs count (the count-only form)");
  if (out->mem != rays->mem) return bad("rays and outputs must live in the same memory kind");
  if (n == 0) return bad("n must be > 0");
  if (n > 0x7fffffffu) return bad("batch too large");
  if (!h) return bad("null handle");
  return guarded([&]() { h->impl->trace_all(rays, n, out); });
}

int rrt_visibility(rrt_handle* h, const rrt_points* a, size_t n_a, const rrt_points* b, size_t n_b, const rrt_vis_params* params, rrt_vis_out* out) {
  auto bad = [&](const char* what) { rrt::set_last_error(std::string("rrt_visibility: ") + what); return (int)RRT_EINVAL; };
  const rrt_vis_params defaults = {RRT_VIS_MATRIX, RRT_VIS_POINTS, 0u, 0, 0.0, 0.0, nullptr, nullptr};
  const rrt_vis_params* p = params ? params : &defaults;
  if (!a) return bad("null point description a (rrt_points)");
  if (!b) return bad("null point description b (rrt_points)");
  if (!out) return bad("null output description (rrt_vis_out)");
  if (!a->px || !a->py || !a->pz) return bad("null coordinate array of a");
  if (!b->px || !b->py || !b->pz) return bad("null coordinate array of b");
  if (!out->bits) return bad("null bits");
  const bool an = a->nx && a->ny && a->nz, bn = b->nx && b->ny && b->nz;
  if (!an && (a->nx || a->ny || a->nz)) return bad("the normals of a must all be NULL or all be set");
  if (!bn && (b->nx || b->ny || b->nz)) return bad("the normals of b must all be NULL or all be set");
  if (a->mem != RRT_MEM_HOST && a->mem != RRT_MEM_DEVICE) return bad("bad mem");
  if (b->mem != a->mem || out->mem != a->mem) return bad("a, b and the outputs must live in the same memory kind (mem)");
  if (a->precision != b->precision) return bad("a and b must have the same precision");
  if (n_a == 0 || n_b == 0) return bad("n_a and n_b must be > 0");
  if (n_a > 0x7fffffffu || n_b > 0x7fffffffu) return bad("n_a or n_b too large (above 2^31 - 1)");
  if ((uint64_t)n_a * (uint64_t)n_b > ((uint64_t)1 << 40)) return bad("n_a * n_b too large (above 2^40)");
  if (p->mode != RRT_VIS_MATRIX && p->mode != RRT_VIS_PAIRS) return bad("bad mode");
  if (p->b_kind != RRT_VIS_POINTS && p->b_kind != RRT_VIS_DIRECTIONS) return bad("bad b_kind");
  if ((p->flags & ~(uint32_t)(RRT_VIS_FACING_A | RRT_VIS_FACING_B)) != 0u) return bad("bad flags");
  if (!(p->offset_a - p->offset_a == 0.0)) return bad("offset_a must be finite");
  if (!(p->offset_b - p->offset_b == 0.0)) return bad("offset_b must be finite");
  if (!an && p->offset_a != 0.0) return bad("offset_a needs the normals of a");
  if (!an && (p->flags & RRT_VIS_FACING_A)) return bad("RRT_VIS_FACING_A needs the normals of a");
  if (p->b_kind == RRT_VIS_DIRECTIONS) {
    if (bn) return bad("RRT_VIS_DIRECTIONS: b is a set of directions and takes no normals");
    if (p->offset_b != 0.0) return bad("RRT_VIS_DIRECTIONS: offset_b must be 0");
    if (p->flags & RRT_VIS_FACING_B) return bad("RRT_VIS_DIRECTIONS: RRT_VIS_FACING_B has no meaning");
    if (p->skip_b) return bad("RRT_VIS_DIRECTIONS: skip_b must be NULL");
  }
  if (!bn && p->offset_b != 0.0) return bad("offset_b needs the normals of b");
  if (!bn && (p->flags & RRT_VIS_FACING_B)) return bad("RRT_VIS_FACING_B needs the normals of b");
  if (p->mode == RRT_VIS_PAIRS) {
    if (n_b != n_a) return bad("RRT_VIS_PAIRS: n_b must equal n_a");
    if (out->count) return bad("RRT_VIS_PAIRS: count must be NULL");
  }
  if (!h) return bad("null handle");
  return guarded([&]() { h->impl->visibility(a, n_a, b, n_b, p, out); });
}

int rrt_render_rays(rrt_handle* h, const int32_t rect[4], uint64_t s0, uint64_t s1, const rrt_ray_samples* rays, const void* p_film, void* film_xyzw, int film_mem,
                    rrt_render_stats* stats) {
  if (const int rc = ray_samples_check("rrt_render_rays", rays, false); rc != RRT_OK) return rc;
  if (!rect) { rrt::set_last_error("rrt_render_rays: null rect"); return RRT_EINVAL; }
  if (!p_film) { rrt::set_last_error("rrt_render_rays: null p_film"); return RRT_EINVAL; }
  if (!film_xyzw) { rrt::set_last_error("rrt_render_rays: null film"); return RRT_EINVAL; }
  if (film_mem != RRT_MEM_HOST && film_mem != RRT_MEM_DEVICE) { rrt::set_last_error("rrt_render_rays: bad film_mem"); return RRT_EINVAL; }
  if (!h) { rrt::set_last_error("rrt_render_rays: null handle"); return RRT_EINVAL; }
  return guarded([&]() { h->impl->render_rays(rect, s0, s1, rays, p_film, film_xyzw, film_mem, stats); });
}

int rrt_render_bands(rrt_handle* h, int rank, int world, void* film_xyzw, int film_mem, rrt_render_stats* stats) {
  if (!h || !film_xyzw) { rrt::set_last_error("rrt_render_bands: null argument"); return RRT_EINVAL; }
  if (film_mem != RRT_MEM_HOST && film_mem != RRT_MEM_DEVICE) { rrt::set_last_error("rrt_render_bands: bad film_mem"); return RRT_EINVAL; }
  return guarded([&]() { h->impl->render_bands(rank, world, film_xyzw, film_mem, stats); });
}

int rrt_render_bands_begin(rrt_handle* h, int rank, int world, void* film_xyzw_device) {
  if (!h || !film_xyzw_device) { rrt::set_last_error("rrt_render_bands_begin: null argument"); return RRT_EINVAL; }
  return guarded([&]() { h->impl->render_bands_begin(rank, world, film_xyzw_device); });
}

int rrt_render_end(rrt_handle* h) {
  if (!h) { rrt::set_last_error("rrt_render_end: null argument"); return RRT_EINVAL; }
  return guarded([&]() { h->impl->render_end(nullptr); });
}

int rrt_render_end_stats(rrt_handle* h, rrt_render_stats* stats) {
  if (!h || !stats) { rrt::set_last_error("rrt_render_end_stats: null argument"); return RRT_EINVAL; }
  return guarded([&]() { h->impl->render_end(stats); });
}

int rrt_render_aov(rrt_handle* h, const int32_t rect[4], int rank, int world, uint64_t max_samples, rrt_aov* out) {
  // the output description is checked first: it is the caller's own struct, wrong whichever handle it comes with
  if (!out) { rrt::set_last_error("rrt_render_aov: null output description (rrt_aov)"); return RRT_EINVAL; }
  if (!out->albedo && !out->normal && !out->depth) { rrt::set_last_error("rrt_render_aov: no plane requested (albedo, normal and depth are all NULL)"); return RRT_EINVAL; }
  if (out->mem != RRT_MEM_HOST && out->mem != RRT_MEM_DEVICE) { rrt::set_last_error("rrt_render_aov: bad mem"); return RRT_EINVAL; }
  if (!h || !rect) { rrt::set_last_error("rrt_render_aov: null handle or rect"); return RRT_EINVAL; }
  return guarded([&]() { h->impl->render_aov(rect, rank, world, max_samples, out); });
}

void rrt_ao_defaults(const rrt_handle* h, rrt_ao_params* p) {
  if (!p) return;
  p->n_samples = 64; p->cos_sample = 1;
  if (h) h->impl->ao_defaults(p);
}

int rrt_render_ao(rrt_handle* h, const int32_t rect[4], int rank, int world, uint64_t max_samples, const rrt_ao_params* params, rrt_ao* out) {
  // everything the host can see, before any device work
  if (!out) { rrt::set_last_error("rrt_render_ao: null output description (rrt_ao)"); return RRT_EINVAL; }
  if (!out->ao && !out->bent) { rrt::set_last_error("rrt_render_ao: no plane requested (ao and bent are both NULL)"); return RRT_EINVAL; }
  if (out->mem != RRT_MEM_HOST && out->mem != RRT_MEM_DEVICE) { rrt::set_last_error("rrt_render_ao: bad mem"); return RRT_EINVAL; }
  if (params && params->n_samples < 1) { rrt::set_last_error("rrt_render_ao: n_samples must be at least 1"); return RRT_EINVAL; }
  if (params && params->n_samples > 256) { rrt::set_last_error("rrt_render_ao: n_samples must be at most 256 (draw i reads sampler dimensions 5 + 2i and 6 + 2i)"); return RRT_EINVAL; }
  if (!h || !rect) { rrt::set_last_error("rrt_render_ao: null handle or rect"); return RRT_EINVAL; }
  return guarded([&]() { h->impl->render_ao(rect, rank, world, max_samples, params, out); });
}

int rrt_render_aov_follow(rrt_handle* h, const int32_t rect[4], int rank, int world, uint64_t max_samples, uint32_t max_follow, rrt_aov* out) {
  // rrt_render_aov's checks in its order, then the chain's own bound: all before any device work
  if (!out) { rrt::set_last_error("rrt_render_aov_follow: null output description (rrt_aov)"); return RRT_EINVAL; }
  if (!out->albedo && !out->normal && !out->depth) { rrt::set_last_error("rrt_render_aov_follow: no plane requested (albedo, normal and depth are all NULL)"); return RRT_EINVAL; }
  if (out->mem != RRT_MEM_HOST && out->mem != RRT_MEM_DEVICE) { rrt::set_last_error("rrt_render_aov_follow: bad mem"); return RRT_EINVAL; }
  if (!rect) { rrt::set_last_error("rrt_render_aov_follow: null rect"); return RRT_EINVAL; }
  if (!h) { rrt::set_last_error("rrt_render_aov_follow: null handle"); return RRT_EINVAL; }
  if (max_follow > 16u) { rrt::set_last_error("rrt_render_aov_follow: max_follow must be 0..16"); return RRT_EINVAL; }
  return guarded([&]() { h->impl->render_aov_follow(rect, rank, world, max_samples, max_follow, out); });
}

void rrt_denoise_defaults(rrt_denoise_params* p) {
  if (!p) return;
  p->iterations = 5; p->demodulate = 1;
  p->sigma_color = 4.0; p->sigma_normal = 32.0; p->sigma_depth = 8.0;
}

namespace {
// rrt_denoise and rrt_denoise_moments: the same checks in the same order under either name; `moments` is looked at only where `with_moments`
int denoise_entry(const char* fn, rrt_handle* h, const void* film_xyzw, const rrt_aov* aov, bool with_moments, const void* moments, const rrt_denoise_params* params, void* film_out) {
  const std::string name(fn);
  auto bad = [&](const char* what) { rrt::set_last_error(name + ": " + what); return (int)RRT_EINVAL; };
  // the caller's own structs first (wrong whichever handle they come with), every pointer before any device work
  if (!aov) return bad("null plane description (rrt_aov)");
  if (!aov->albedo || !aov->normal || !aov->depth) return bad("the filter needs all three planes (albedo, normal or depth is NULL)");
  if (aov->mem != RRT_MEM_HOST && aov->mem != RRT_MEM_DEVICE) return bad("bad mem");
  rrt_denoise_params p;
  rrt_denoise_defaults(&p);
  if (params) p = *params;
  if (p.iterations < 1 || p.iterations > 6) return bad("iterations must be 1 .. 6");
  if (!(p.sigma_normal > 0.0)) return bad("sigma_normal must be > 0");
  if (!(p.sigma_depth > 0.0)) return bad("sigma_depth must be > 0");
  if (!film_xyzw || !film_out) return bad("null film or film_out");
  if (with_moments && !moments) return bad("null moments plane");
  if (!h) return bad("null handle");
  return guarded([&]() { h->impl->denoise(film_xyzw, aov, with_moments ? moments : nullptr, &p, film_out); });
}
}  // namespace

int rrt_denoise(rrt_handle* h, const void* film_xyzw, const rrt_aov* aov, const rrt_denoise_params* params, void* film_out) {
  return denoise_entry("rrt_denoise", h, film_xyzw, aov, false, nullptr, params, film_out);
}

int rrt_denoise_moments(rrt_handle* h, const void* film_xyzw, const rrt_aov* aov, const void* moments, const rrt_denoise_params* params, void* film_out) {
  return denoise_entry("rrt_denoise_moments", h, film_xyzw, aov, true, moments, params, film_out);
}

int rrt_render_moments(rrt_handle* h, const int32_t rect[4], int rank, int world, void* film_xyzw, void* moments, int mem, rrt_render_stats* stats) {
  // every pointer before any device work, each with its own message
  if (!h) { rrt::set_last_error("rrt_render_moments: null handle"); return RRT_EINVAL; }
  if (!rect) { rrt::set_last_error("rrt_render_moments: null rect"); return RRT_EINVAL; }
  if (!film_xyzw) { rrt::set_last_error("rrt_render_moments: null film"); return RRT_EINVAL; }
  if (!moments) { rrt::set_last_error("rrt_render_moments: null moments plane"); return RRT_EINVAL; }
  if (mem != RRT_MEM_HOST && mem != RRT_MEM_DEVICE) { rrt::set_last_error("rrt_render_moments: bad mem"); return RRT_EINVAL; }
  return guarded([&]() { h->impl->render_moments(rect, rank, world, film_xyzw, moments, mem, stats); });
}

int rrt_render_frame_aov(rrt_handle* h, const int32_t rect[4], int rank, int world, void* film_xyzw, void* moments, int mem, uint64_t aov_max_samples, rrt_aov* aov,
                         rrt_render_stats* stats) {
  // every check that needs no device before any device work, each with its own message; the caller's own arguments first (wrong whichever
  // handle they come with), as rrt_render_aov has it; `moments` may be NULL (the plane is not produced)
  if (!rect) { rrt::set_last_error("rrt_render_frame_aov: null rect"); return RRT_EINVAL; }
  if (!film_xyzw) { rrt::set_last_error("rrt_render_frame_aov: null film"); return RRT_EINVAL; }
  if (!aov) { rrt::set_last_error("rrt_render_frame_aov: null plane description (rrt_aov)"); return RRT_EINVAL; }
  if (!aov->albedo && !aov->normal && !aov->depth) { rrt::set_last_error("rrt_render_frame_aov: no plane requested (albedo, normal and depth are all NULL)"); return RRT_EINVAL; }
  if (mem != RRT_MEM_HOST && mem != RRT_MEM_DEVICE) { rrt::set_last_error("rrt_render_frame_aov: bad mem"); return RRT_EINVAL; }
  if (aov->mem != mem) { rrt::set_last_error("rrt_render_frame_aov: the planes must live in the film's memory kind (aov->mem != mem)"); return RRT_EINVAL; }
  if (!h) { rrt::set_last_error("rrt_render_frame_aov: null handle"); return RRT_EINVAL; }
  return guarded([&]() { h->impl->render_frame_aov(rect, rank, world, film_xyzw, moments, mem, aov_max_samples, aov, stats); });
}

void rrt_adaptive_defaults(rrt_adaptive_params* p) {
  if (!p) return;
  p->min_samples = 16; p->batch = 16; p->max_samples = 0;
  p->threshold = 0.05;
}

namespace {
// whole kTileW x kTileH tiles anchored at the rect's origin (host arithmetic: asked before any device work)
bool whole_tiles(const int32_t rect[4]) {
  const int64_t rw = (int64_t)rect[2] - rect[0], rh = (int64_t)rect[3] - rect[1];
  return rw > 0 && rh > 0 && rw % (int64_t)rrtd::kTileW == 0 && rh % (int64_t)rrtd::kTileH == 0;
}
}  // namespace

int rrt_tile_error(rrt_handle* h, const void* moments, int mem, const int32_t rect[4], double* tile_error) {
  // the caller's own arguments first, every one before any device work and each with its own message
  if (!moments) { rrt::set_last_error("rrt_tile_error: null moments plane"); return RRT_EINVAL; }
  if (!rect) { rrt::set_last_error("rrt_tile_error: null rect"); return RRT_EINVAL; }
  if (!tile_error) { rrt::set_last_error("rrt_tile_error: null output"); return RRT_EINVAL; }
  if (mem != RRT_MEM_HOST && mem != RRT_MEM_DEVICE) { rrt::set_last_error("rrt_tile_error: bad mem"); return RRT_EINVAL; }
  if (!whole_tiles(rect)) { rrt::set_last_error("rrt_tile_error: the rect's width and height must be positive multiples of 8 (whole 8 x 8 tiles)"); return RRT_EINVAL; }
  if (!h) { rrt::set_last_error("rrt_tile_error: null handle"); return RRT_EINVAL; }
  return guarded([&]() { h->impl->tile_error(moments, mem, rect, tile_error); });
}

int rrt_render_adaptive(rrt_handle* h, const int32_t rect[4], const rrt_adaptive_params* params, void* film_xyzw, void* moments, uint32_t* tile_samples, int mem,
                        rrt_render_stats* stats) {
  // the caller's own arguments first (wrong whichever handle they come with), every one before any device work and each with its own message
  if (!rect) { rrt::set_last_error("rrt_render_adaptive: null rect"); return RRT_EINVAL; }
  if (!film_xyzw) { rrt::set_last_error("rrt_render_adaptive: null film"); return RRT_EINVAL; }
  if (!moments) { rrt::set_last_error("rrt_render_adaptive: null moments plane"); return RRT_EINVAL; }
  if (mem != RRT_MEM_HOST && mem != RRT_MEM_DEVICE) { rrt::set_last_error("rrt_render_adaptive: bad mem"); return RRT_EINVAL; }
  rrt_adaptive_params p;
  rrt_adaptive_defaults(&p);
  if (params) p = *params;
  if (p.min_samples < 2) { rrt::set_last_error("rrt_render_adaptive: min_samples must be >= 2 (a variance needs two samples)"); return RRT_EINVAL; }
  if (p.batch < 1) { rrt::set_last_error("rrt_render_adaptive: batch must be >= 1"); return RRT_EINVAL; }
  if (!(p.threshold >= 0.0)) { rrt::set_last_error("rrt_render_adaptive: threshold must be >= 0 and not NaN"); return RRT_EINVAL; }
  if (!whole_tiles(rect)) { rrt::set_last_error("rrt_render_adaptive: the rect's width and height must be positive multiples of 8 (whole 8 x 8 tiles)"); return RRT_EINVAL; }
  if (!h) { rrt::set_last_error("rrt_render_adaptive: null handle"); return RRT_EINVAL; }
  return guarded([&]() { h->impl->render_adaptive(rect, &p, film_xyzw, moments, tile_samples, mem, stats); });
}

int rrt_render_passes(rrt_handle* h, const int32_t rect[4], int rank, int world, const uint8_t* light_group, const rrt_pass* passes, int n_passes, void* film_xyzw, int mem,
                      rrt_render_stats* stats) {
  // the caller's own arguments first (wrong whichever handle they come with), each with its own message; the light_group entries, whose number is the
  // handle's, are the first thing the handle checks - also before any device work
  static_assert(RRT_MAX_PASSES == rrtd::kMaxPasses && RRT_MAX_PASSES <= 16, "a pass mask rides in 16 bits of a shadow record's table word");
  if (!rect) { rrt::set_last_error("rrt_render_passes: null rect"); return RRT_EINVAL; }
  if (!passes) { rrt::set_last_error("rrt_render_passes: null passes"); return RRT_EINVAL; }
  if (n_passes < 1 || n_passes > RRT_MAX_PASSES) { rrt::set_last_error("rrt_render_passes: n_passes must be 1 .. 16 (RRT_MAX_PASSES)"); return RRT_EINVAL; }
  for (int k = 0; k < n_passes; k++) {
    if (!passes[k].film_xyzw) { rrt::set_last_error("rrt_render_passes: null pass film (passes[" + std::to_string(k) + "].film_xyzw)"); return RRT_EINVAL; }
    if (passes[k].bounce_lo < 0) { rrt::set_last_error("rrt_render_passes: passes[" + std::to_string(k) + "].bounce_lo must be >= 0"); return RRT_EINVAL; }
  }
  if (mem != RRT_MEM_HOST && mem != RRT_MEM_DEVICE) { rrt::set_last_error("rrt_render_passes: bad mem"); return RRT_EINVAL; }
  if (!h) { rrt::set_last_error("rrt_render_passes: null handle"); return RRT_EINVAL; }
  return guarded([&]() { h->impl->render_passes(rect, rank, world, light_group, passes, n_passes, film_xyzw, mem, stats); });
}

int rrt_combine_passes(rrt_handle* h, const void* const* films, const double* gains_rgb, int n, void* film_out, int mem) {
  if (!films) { rrt::set_last_error("rrt_combine_passes: null films"); return RRT_EINVAL; }
  if (!gains_rgb) { rrt::set_last_error("rrt_combine_passes: null gains"); return RRT_EINVAL; }
  if (!film_out) { rrt::set_last_error("rrt_combine_passes: null output film"); return RRT_EINVAL; }
  if (n < 1 || n > RRT_MAX_PASSES) { rrt::set_last_error("rrt_combine_passes: n must be 1 .. 16 (RRT_MAX_PASSES)"); return RRT_EINVAL; }
  for (int k = 0; k < n; k++) if (!films[k]) { rrt::set_last_error("rrt_combine_passes: null film (films[" + std::to_string(k) + "])"); return RRT_EINVAL; }
  if (mem != RRT_MEM_HOST && mem != RRT_MEM_DEVICE) { rrt::set_last_error("rrt_combine_passes: bad mem"); return RRT_EINVAL; }
  if (!h) { rrt::set_last_error("rrt_combine_passes: null handle"); return RRT_EINVAL; }
  return guarded([&]() { h->impl->combine_passes(films, gains_rgb, n, film_out, mem); });
}

namespace {
// the caller's own table description, wrong whichever handle it comes with: every check before any device work, each with its own message
int mattes_desc_check(const std::string& name, const rrt_mattes* m) {
  auto bad = [&](const char* what) { rrt::set_last_error(name + ": " + what); return (int)RRT_EINVAL; };
  static_assert(RRT_MAX_MATTE_SLOTS == rrtd::kMaxMatteSlots, "the slot tile of the matte kernels is sized for RRT_MAX_MATTE_SLOTS");
  if (!m) return bad("null table description (rrt_mattes)");
  if (!m->ids) return bad("null ids array");
  if (!m->coverage) return bad("null coverage array");
  if (!m->weight) return bad("null weight array");
  if (m->n_slots < 1 || m->n_slots > RRT_MAX_MATTE_SLOTS) return bad("n_slots must be 1 .. 16 (RRT_MAX_MATTE_SLOTS)");
  if (m->mem != RRT_MEM_HOST && m->mem != RRT_MEM_DEVICE) return bad("bad mem");
  return RRT_OK;
}
}  // namespace

int rrt_render_mattes(rrt_handle* h, const int32_t rect[4], int rank, int world, uint64_t max_samples, const uint32_t* prim_id, size_t n_prim_id, rrt_mattes* out) {
  if (const int rc = mattes_desc_check("rrt_render_mattes", out); rc != RRT_OK) return rc;
  if (!rect) { rrt::set_last_error("rrt_render_mattes: null rect"); return RRT_EINVAL; }
  if (!h) { rrt::set_last_error("rrt_render_mattes: null handle"); return RRT_EINVAL; }
  return guarded([&]() { h->impl->render_mattes(rect, rank, world, max_samples, prim_id, n_prim_id, out); });
}

int rrt_matte_extract(rrt_handle* h, const rrt_mattes* m, const uint32_t* ids, int n_ids, void* alpha) {
  if (const int rc = mattes_desc_check("rrt_matte_extract", m); rc != RRT_OK) return rc;
  if (!ids) { rrt::set_last_error("rrt_matte_extract: null id list"); return RRT_EINVAL; }
  if (n_ids < 1 || n_ids > 256) { rrt::set_last_error("rrt_matte_extract: n_ids must be 1 .. 256"); return RRT_EINVAL; }
  if (!alpha) { rrt::set_last_error("rrt_matte_extract: null alpha"); return RRT_EINVAL; }
  if (!h) { rrt::set_last_error("rrt_matte_extract: null handle"); return RRT_EINVAL; }
  return guarded([&]() { h->impl->matte_extract(m, ids, n_ids, alpha); });
}

int rrt_set_option(rrt_handle* h, const char* key, double value) {
  if (!h || !key) { rrt::set_last_error("rrt_set_option: null argument"); return RRT_EINVAL; }
  return guarded([&]() { h->impl->set_option(key, value); });
}

}  // extern "C"
