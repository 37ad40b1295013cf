// Host-side driver of the wavefront kernels for one arithmetic type R: scene upload (the tables come from the plain host code of
// host/scene_prep.hpp; here they go to HBM), pool allocation, the per-pass / per-bounce launch sequence and the public trace entry points.
// One HIP stream per handle; no host synchronisation inside a frame (queue sizes are read on the device).
#pragma once
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <memory>
#include <optional>
#include <stdexcept>
#include <string>
#include <vector>

#include <type_traits>

#include "dfilter.hpp"
#include "dkernels.hpp"
#include "dtraverse_f32.hpp"
#include "errors.hpp"
#include "rrt.h"
#include "scene_prep.hpp"

namespace rrtd {


#define HIP_CHECK(expr)                                                                                   \
  do {                                                                                                    \
    hipError_t _e = (expr);                                                                               \
    if (_e != hipSuccess)                                                                                 \
      throw ::rrtd::DeviceError(std::string("HIP error: ") + hipGetErrorString(_e) + " at " #expr);              \
  } while (0)

struct HandleBase {
  virtual ~HandleBase() {}
  virtual int precision() const = 0;
  virtual hipStream_t stream() const = 0;
  virtual int device() const = 0;
  // film geometry for the multi-GPU reassembly (rrt_comm.hip): resolution, and whether samples splat across pixels (then the
  // ranks' films overlap and the collective is a sum instead of a gather of disjoint bands)
  virtual void film_geometry(int* xres, int* yres, bool* splats) const = 0;
  virtual void trace_closest(const rrt_rays* rays, size_t n, rrt_hits* out) = 0;
  virtual void trace_any(const rrt_rays* rays, size_t n, uint8_t* occluded) = 0;
  virtual void camera_samples(const int32_t rect[4], uint64_t s0, uint64_t s1, double* dims5, double* ray_od6, double* weight) = 0;
  virtual void sampler_values(const uint32_t* pixel, const uint32_t* sample_num, size_t n, uint32_t first, uint32_t count, uint64_t* index /* may be NULL */, double* v1, double* v2) = 0;
  virtual void render_rect(const int32_t rect[4], void* film, int film_mem, rrt_render_stats* stats) = 0;
  virtual void radiance(const rrt_ray_samples* rays, size_t n, void* rgb4) = 0;
  // rrt_irradiance (od6 NULL; sh27 may be NULL) and rrt_irradiance_rays (od6 set, sums4 and sh27 NULL) under the name `who`
  virtual void irradiance(const char* who, const rrt_points* pts, size_t n, uint64_t s0, uint64_t s1, int mode, double offset, void* sums4, void* sh27, void* od6) = 0;
  // rrt_surface_rays (rays set, sites NULL) and rrt_surface_at (sites set, rays NULL) under the name `who`
  virtual void surface(const char* who, const rrt_rays* rays, const rrt_sites* sites, size_t n, const rrt_surface* out) = 0;
  virtual void atlas_sites(int32_t aw, int32_t ah, const int32_t* prims, size_t n_list, int mem, int32_t* site_prim, void* b1, void* b2, uint64_t* n_covered) = 0;
  virtual void nearest(const rrt_points* pts, size_t n, double max_dist, const rrt_nearest_out* out) = 0;
  virtual void trace_all(const rrt_rays* rays, size_t n, const rrt_multi_hits* out) = 0;
  virtual void visibility(const rrt_points* a, size_t n_a, const rrt_points* b, size_t n_b, const rrt_vis_params* prm, const rrt_vis_out* out) = 0;
  virtual void render_rays(const int32_t rect[4], uint64_t s0, uint64_t s1, const rrt_ray_samples* rays, const void* p_film, void* film, int film_mem, rrt_render_stats* stats) = 0;   // p_film in rays->mem
  virtual void render_bands(int rank, int world, void* film, int film_mem, rrt_render_stats* stats) = 0;
  virtual void render_bands_begin(int rank, int world, void* film_device) = 0;
  virtual void render_end(rrt_render_stats* stats) = 0;
  virtual void render_aov(const int32_t rect[4], int rank, int world, uint64_t max_samples, const rrt_aov* out) = 0;
  virtual void render_aov_follow(const int32_t rect[4], int rank, int world, uint64_t max_samples, uint32_t max_follow, const rrt_aov* out) = 0;
  virtual void ao_defaults(rrt_ao_params* p) const = 0;
  virtual void render_ao(const int32_t rect[4], int rank, int world, uint64_t max_samples, const rrt_ao_params* params, const rrt_ao* out) = 0;   // params may be NULL
  virtual void render_moments(const int32_t rect[4], int rank, int world, void* film, void* moments, int mem, rrt_render_stats* stats) = 0;
  virtual void render_frame_aov(const int32_t rect[4], int rank, int world, void* film, void* moments, int mem, uint64_t aov_max_samples, const rrt_aov* aov, rrt_render_stats* stats) = 0;   // moments may be NULL
  virtual void render_adaptive(const int32_t rect[4], const rrt_adaptive_params* ap, void* film, void* moments, uint32_t* tile_samples, int mem, rrt_render_stats* stats) = 0;
  virtual void tile_error(const void* moments, int mem, const int32_t rect[4], double* tile_error) = 0;
  virtual void render_passes(const int32_t rect[4], int rank, int world, const uint8_t* light_group, const rrt_pass* passes, int n_passes, void* film, int mem, rrt_render_stats* stats) = 0;   // film may be NULL
  virtual void combine_passes(const void* const* films, const double* gains_rgb, int n, void* film_out, int mem) = 0;
  virtual void denoise(const void* film, const rrt_aov* aov, const void* moments, const rrt_denoise_params* p, void* film_out) = 0;   // moments may be NULL (rrt_denoise)
  virtual void render_mattes(const int32_t rect[4], int rank, int world, uint64_t max_samples, const uint32_t* prim_id, size_t n_prim_id, const rrt_mattes* out) = 0;   // prim_id may be NULL
  virtual void matte_extract(const rrt_mattes* m, const uint32_t* ids, int n_ids, void* alpha) = 0;
  virtual void set_option(const std::string& key, double v) = 0;
  // rrt_film_gather (rrt_comm.hip): events on the handle's stream around the frame's collective, so that the frame's statistics can tell
  // the collective (rrt_render_stats::ms_gather) from the render (ms_total) - what a multi-GPU scaling run needs to separate imbalance from xGMI time
  virtual void gather_mark(bool begin) = 0;
  std::vector<std::string> warnings;   // rrt_warning(): non-fatal diagnostics of the handle's creation
};

template <typename T>
struct DevBuf {
  T* p = nullptr;
  size_t n = 0;
  void alloc(size_t count) {
    release();
    n = count;
    if (count) HIP_CHECK(hipMalloc((void**)&p, count * sizeof(T)));
  }
  // (H: T itself, or the plain record of the same layout that the host code emits where T is a HIP vector type - HaltonHi for uint4, Float4 for float4)
  template <typename H>
  void upload(const std::vector<H>& h, hipStream_t st) {
    static_assert(sizeof(H) == sizeof(T) && std::is_trivially_copyable<H>::value, "upload: host record and device record differ in size");
    alloc(h.size());
    if (!h.empty()) HIP_CHECK(hipMemcpyAsync(p, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice, st));
  }
  void release() { if (p) { (void)hipFree(p); p = nullptr; } n = 0; }
  ~DevBuf() { release(); }
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
};


// what a frame leaves behind for its statistics: HIP events around every launch (on the stream the launch went to), launch counts
struct FrameRec {
  std::vector<hipEvent_t> all;
  std::vector<std::pair<int, std::pair<hipEvent_t, hipEvent_t>>> evs;   // category, begin, end
  hipEvent_t ev_begin = nullptr, ev_end = nullptr;
  uint64_t n_closest_launch = 0, n_any_launch = 0, n_tile_launch = 0, n_list_launch = 0, camera_samples = 0;
  bool timing = false;
  hipEvent_t make() { hipEvent_t e = nullptr; HIP_CHECK(hipEventCreate(&e)); all.push_back(e); return e; }
  // the frame's own two events, where its timing is wanted: made and the first recorded before the first pass, the second recorded after the last
  void begin(bool want_timing, hipStream_t st) { timing = want_timing; if (timing) { ev_begin = make(); ev_end = make(); HIP_CHECK(hipEventRecord(ev_begin, st)); } }
  void end(hipStream_t st) { if (timing) HIP_CHECK(hipEventRecord(ev_end, st)); }
  ~FrameRec() { for (hipEvent_t e : all) (void)hipEventDestroy(e); }   // on every way out (a panic / HIP error thrown mid-frame included)
  FrameRec() = default;
  FrameRec(const FrameRec&) = delete;
  FrameRec& operator=(const FrameRec&) = delete;
};

// ---- launch dispatch: run-time facts into template arguments. A launcher writes its kernel's launch once, in a generic lambda, and takes the
// flags as arguments: `MIXED()` inside it is a constant. Only what a launcher asks for is instantiated ("Traversal launches").
template <bool B> using Flag = std::integral_constant<bool, B>;
constexpr Flag<true> kYes{};
constexpr Flag<false> kNo{};
template <class F> void with_flag(bool b, F&& f) { if (b) f(kYes); else f(kNo); }
// What an any-hit launch does with a free ray: the frame's L (film), the pending radiance of a rrt_render_passes frame (the kernels' PASSES),
// or the accumulators of a rrt_render_ao round (their AO). No kernel has PASSES and AO together: f(PASSES, AO) sees the three that exist.
enum class AnySink { film, passes, ao };
template <class F> void with_sink(AnySink s, F&& f) {
  if (s == AnySink::ao) f(kNo, kYes);
  else if (s == AnySink::passes) f(kYes, kNo);
  else f(kNo, kNo);
}

template <typename R>
class Handle : public HandleBase {
  // ---- what the entry points below share: the call preamble, the pixels and samples of a call (CallGeom), the film window of a wide filter ------
  // The film kernels in their box form (k_film_box, k_gather_box ...) are the closed form for the default box filter (radius exactly
  // 0.5: every sample lands in its own pixel with weight 1); a smaller radius leaves samples near the pixel borders in no pixel at all, a larger
  // one splats: both take the general (wide) kernels
  bool wide_filter() const {
    const rrt_film& f = desc_.film;
    return f.filter_type != RRT_FILTER_BOX || f.filter_radius[0] != 0.5 || f.filter_radius[1] != 0.5;
  }
  void check_rect(const char* msg, const int32_t rect[4], bool allow_empty = false) const {
    const rrt_film& f = desc_.film;
    const bool inside = rect[0] >= 0 && rect[1] >= 0 && rect[2] <= f.xres && rect[3] <= f.yres;
    const bool ordered = allow_empty ? (rect[0] <= rect[2] && rect[1] <= rect[3]) : (rect[0] < rect[2] && rect[1] < rect[3]);
    if (!inside || !ordered) throw std::invalid_argument(msg);
  }
  void check_no_crop() const {
    const rrt_film& f = desc_.film;
    if (f.crop[0] != 0 || f.crop[1] != 0 || f.crop[2] != f.xres || f.crop[3] != f.yres) throw UnsupportedError("film crop window");
  }
  // the rows of a rect that belong to this rank: those of the interleaved band_h-row bands b with b % n_ranks == rank (partition.py)
  size_t band_rows(const int32_t rect[4], uint32_t band_h, uint32_t n_ranks, uint32_t rank) const {
    const size_t rh = (size_t)(rect[3] - rect[1]);
    if (n_ranks <= 1) return rh;
    size_t rows = 0;
    for (size_t y = 0; y < rh; y++) if ((y / band_h) % n_ranks == rank) rows++;
    return rows;
  }
  // the samples of a pixel a frame takes: numbers 1 .. nsamp-1 (Q1), the first max_samples of them where that is not 0
  uint64_t frame_samples(uint64_t max_samples = 0) const {
    const uint64_t nsamp = desc_.sampler.samples_per_pixel, n = nsamp > 1 ? nsamp - 1 : 0;
    return max_samples != 0 ? std::min(n, max_samples) : n;
  }
  // the film pixels the samples of a rect can touch under a wide filter (FilmWindow): the rect grown by ceil(r + 0.5), clipped to the film
  FilmWindow film_window(const int32_t rect[4]) const {
    const rrt_film& f = desc_.film;
    const int reach_x = (int)std::ceil(f.filter_radius[0] + 0.5), reach_y = (int)std::ceil(f.filter_radius[1] + 0.5);
    const int ex0 = std::max(0, rect[0] - reach_x), ey0 = std::max(0, rect[1] - reach_y);
    const int ex1 = std::min(f.xres, rect[2] + reach_x), ey1 = std::min(f.yres, rect[3] + reach_y);
    return {ex0, ey0, ex1 - ex0, ey1 - ey0, reach_x, reach_y, f.yres};
  }
  // The call preamble, first half: what a call refuses of its arguments before any device work, in the one order every call has it - a frame in
  // flight (idle), a struct of the other precision (prec: the "plane", "table" or "ray" struct the caller filled), rank / world, the rect. A
  // call passes what it checks; each message begins with the call's own name.
  struct Prec { const char* what; int precision; };
  struct Ranks { int rank, world; };
  static constexpr bool kWhenIdle = true, kAnyTime = false;   // (not "kIdle": a member of that name would hide the traversal kernels' word in build_tile_trees)
  void check_args(const std::string& who, bool idle, std::optional<Prec> prec = {}, std::optional<Ranks> ranks = {}, const int32_t* rect = nullptr) const {
    if (idle && pending_) throw std::invalid_argument(who + ": a frame is in flight (rrt_render_bands_begin without rrt_render_end)");
    if (prec && prec->precision != precision()) throw std::invalid_argument(who + ": " + prec->what + " precision must match the handle");
    if (ranks && (ranks->world < 1 || ranks->rank < 0 || ranks->rank >= ranks->world)) throw std::invalid_argument(who + ": bad rank/world");
    if (rect) check_rect((who + ": rect outside the film").c_str(), rect);
  }
  // second half: the device, and what the kernels do not render (film: the call adds to film pixels, which a crop window would cut)
  void device_prologue(bool film = true) {
    HIP_CHECK(hipSetDevice(dev_));
    check_renderable();
    if (film) check_no_crop();
  }
  // The pixels and samples of a call, worked out once when check_args has passed: the rect, this rank's rows of its interleaved band_h-row bands
  // (rh: their number, so rpix counts this rank's pixels), the samples of a pixel, the film window. Every pass of the call is cut from it.
  struct CallGeom { int32_t rect[4]; uint32_t band_h, n_ranks, rank; size_t rw, rh, rpix; uint64_t s_total; FilmWindow win; };
  static constexpr uint32_t kBandH = 16, kNoBands = 1u << 30;
  static uint32_t bands_of(int world) { return world > 1 ? kBandH : kNoBands; }   // every call but rrt_render_bands, which has bands at world 1 too
  CallGeom call_geom(const int32_t rect[4], uint32_t band_h, int rank, int world, uint64_t max_samples = 0) const {
    const size_t rw = (size_t)(rect[2] - rect[0]), rh = band_rows(rect, band_h, (uint32_t)world, (uint32_t)rank);
    return {{rect[0], rect[1], rect[2], rect[3]}, band_h, (uint32_t)world, (uint32_t)rank, rw, rh, rw * rh, frame_samples(max_samples), film_window(rect)};
  }
  // What launch_raygen sets for the pass it last ran for, put back when a first-hit call ends (a frame's tile-tree and film-record state is its
  // own), and the queue halves as the call found them (swapped: the follow levels have swapped them an odd number of times)
  struct RaygenStateGuard {
    Handle* h; bool tt_ok, runs_ok; uint32_t root_cull; float root_box[6]; bool swapped = false;
    explicit RaygenStateGuard(Handle* hh) : h(hh), tt_ok(hh->tt_pass_ok_), runs_ok(hh->film_runs_ok_), root_cull(hh->scene_.root_cull) {
      for (int k = 0; k < 6; k++) root_box[k] = hh->scene_.root_box[k];
    }
    RaygenStateGuard(const RaygenStateGuard&) = delete;
    RaygenStateGuard& operator=(const RaygenStateGuard&) = delete;
    ~RaygenStateGuard() {
      h->tt_pass_ok_ = tt_ok; h->film_runs_ok_ = runs_ok; h->scene_.root_cull = root_cull; for (int k = 0; k < 6; k++) h->scene_.root_box[k] = root_box[k];
      if (swapped) h->swap_queues();
    }
  };

 public:
  Handle(int device, const rrt_scene_desc* d) : dev_(device), desc_(*d) {
    HIP_CHECK(hipSetDevice(dev_));
    try {
      create_streams(hipStreamDefault);
      HIP_CHECK(hipEventCreateWithFlags(&ev_shade_, hipEventDisableTiming));
      for (int k = 0; k < 2; k++) HIP_CHECK(hipEventCreateWithFlags(&ev_shadow_[k], hipEventDisableTiming));
      upload_scene(d);
      HIP_CHECK(hipStreamSynchronize(st_));
    } catch (...) { release_streams(); throw; }   // a refused scene (unsupported / panic) must not leak its streams: the destructor does not run
    // Large pools matter: a launch lasts at least as long as the latency chain of its longest ray, so few big
    // launches beat many small ones (whole 1024^2 x 256 spp frame in one pass: 268 M slots x 280 B = 75 GB in fp32).
    size_t free_b = 0, total_b = 0;
    HIP_CHECK(hipMemGetInfo(&free_b, &total_b));
    const size_t per_slot = (n_vec_records() * 4 + 1) * sizeof(R) + 9 * sizeof(uint32_t);
    max_paths_ = std::max<size_t>(1u << 16, std::min(max_paths_, (free_b / 2) / per_slot));
  }
  ~Handle() override {
    (void)hipSetDevice(dev_);
    release_streams();
  }
  void release_streams() {
    if (st_) (void)hipStreamSynchronize(st_);
    if (st2_) (void)hipStreamSynchronize(st2_);
    if (ev_shade_) (void)hipEventDestroy(ev_shade_);
    for (int k = 0; k < 2; k++) if (ev_shadow_[k]) (void)hipEventDestroy(ev_shadow_[k]);
    for (int k = 0; k < 2; k++) if (ev_gather_[k]) { (void)hipEventDestroy(ev_gather_[k]); ev_gather_[k] = nullptr; }
    if (st2_) (void)hipStreamDestroy(st2_);
    if (st_) (void)hipStreamDestroy(st_);
    ev_shade_ = ev_shadow_[0] = ev_shadow_[1] = nullptr; st_ = st2_ = nullptr;
  }
  int precision() const override { return sizeof(R) == 4 ? RRT_F32 : RRT_F64; }
  hipStream_t stream() const override { return st_; }
  int device() const override { return dev_; }
  void gather_mark(bool begin) override {
    if (!pending_ || !frame_stats_) return;   // only a frame in flight whose statistics are wanted (rrt_render_end_stats) reports it
    HIP_CHECK(hipSetDevice(dev_));
    hipEvent_t& e = ev_gather_[begin ? 0 : 1];
    if (!e) HIP_CHECK(hipEventCreate(&e));
    HIP_CHECK(hipEventRecord(e, st_));
    if (!begin) gather_marked_ = true;
  }
  void film_geometry(int* xres, int* yres, bool* splats) const override {
    const rrt_film& f = desc_.film;
    *xres = f.xres; *yres = f.yres;
    // (not wide_filter(): a box filter narrower than 0.5 takes the wide kernels, but none of its samples reaches a neighbouring pixel)
    *splats = f.filter_type != RRT_FILTER_BOX || f.filter_radius[0] > 0.5 || f.filter_radius[1] > 0.5;
  }

  void set_option(const std::string& key, double v) override {
    if (key == "max_paths") { if (v < 64) throw std::invalid_argument("max_paths must be >= 64"); max_paths_ = (size_t)v; }
    else if (key == "count_traversal") count_traversal_ = v != 0;
    else if (key == "persistent_traversal") { persistent_ = v != 0; if (v >= 1) trav_mode_ = (int)v; }
    else if (key == "raygen_lean") raygen_lean_ = v != 0;   // 0: generic two-stage kernels (the reference's operation order), 1 (default): dense two-stage kernels with the lean lens arithmetic
    else if (key == "tile_order") tile_order_ = v != 0;
    else if (key == "tile_trees") tile_trees_on_ = v != 0;
    else if (key == "quad_nodes") quad_on_ = v != 0;
    else if (key == "shade_compact") scene_.shade_compact = v != 0 ? 1u : 0u;
    else if (key == "horizon_cull") horizon_on_ = v != 0;
    else if (key == "root_cull") root_cull_on_ = v != 0;
    else if (key == "tt_census") { tt_census_spp_ = std::max(1, (int)v); tt_state_ = 0; }
    else if (key == "shadow_lists") shadow_lists_on_ = v != 0;
    else if (key == "sl_grid") sl_grid_cap_ = std::max(1, (int)v);
    else if (key == "rg_spb") {   // the workgroup's 512 threads = 512 / spb pixels x spb samples: spb must divide it evenly, or the last threads would compute the next workgroup's first sample a second time
      if (v != 1 && v != 2 && v != 4 && v != 8) throw std::invalid_argument("rg_spb must be 1, 2, 4 or 8");
      rg_spb_ = (int)v;
    }
    else if (key == "pt_split_closest") pt_split_closest_ = (uint32_t)v;
    else if (key == "pt_split_any") pt_split_any_ = (uint32_t)v;
    else if (key == "overlap_shadow") overlap_shadow_ = v != 0;
    else if (key == "aux_margin") aux_margin_ = v != 0;
    else if (key == "lens_cull") lens_cull_on_ = v != 0;   // 1 (default): the fp32 camera kernel drops the samples of dead lens cells before any lens arithmetic (host/lens_cull.cpp)
    else if (key == "film_records") film_records_on_ = v != 0;   // 1 (default): the path integrator's tile-tree passes keep radiance in per-workgroup record runs, added up by k_film_box_runs
    else if (key == "shade_spec") shade_kinds_ = v != 0 ? shade_kinds_scene_ : kAllKinds;
    else if (key == "frame_stats") frame_stats_ = v != 0;
    else if (key == "nearest_pairs") nn_pairs_on_ = v != 0;   // rrt_nearest in fp32: 0 (default): k_nearest<float> on the linear tree; 1: k_nearest_pairs_f32 on the pair nodes (the same bits, measured slower)
    else if (key == "dn_lds") dn_lds_ = v != 0;   // rrt_denoise: 1 (default): the a-trous steps 1 and 2 read their taps from an LDS tile; 0: direct gathers at every step
    else if (key == "halton_tables") scene_.n_hblk = (v != 0 && hblk_.n) ? (uint32_t)kHaltonTabDims : 0u;
    else if (key == "cam_tables") { for (int w = 0; w < 3; w++) { scene_.cam_lo[w] = (v != 0 && cam_lo_.n) ? cam_lo_.p + cam_lo_off_[w] : nullptr; scene_.cam_hi[w] = (v != 0 && cam_hi_.n) ? cam_hi_.p + cam_hi_off_[w] : nullptr; } }
    else if (key == "any_entry") { any_entry_on_ = v != 0; trav_.any_list = (any_entry_on_ && any_list_.n) ? reinterpret_cast<const uint4*>(any_list_.p) : nullptr; }
    else if (key == "nonblocking_streams") {   // see rrt.h: needed for two handles to overlap their frames
      if (pending_) throw std::invalid_argument("nonblocking_streams: a frame is in flight");
      HIP_CHECK(hipSetDevice(dev_));
      create_streams(v != 0 ? hipStreamNonBlocking : hipStreamDefault);
    }
    else throw std::invalid_argument("unknown option " + key);
  }

  // ---- public trace entry points (rays / hits in caller memory) ---------------------------------------------
  void trace_closest(const rrt_rays* rays, size_t n, rrt_hits* out) override {
    HIP_CHECK(hipSetDevice(dev_));
    if (rays->precision != precision() || out->precision != precision()) throw std::invalid_argument("ray/hit precision must match the handle");
    ensure_pools(n);
    load_rays(rays, n);
    const bool want_counts = out->nodes_visited && out->prims_tested;
    DevBuf<uint32_t> cn, cp;
    if (want_counts) { cn.alloc(n); cp.alloc(n); }
    hipLaunchKernelGGL(k_rotate, dim3(1), dim3(1), 0, st_, counters_.p, 3);
    launch_closest(nullptr, nullptr, (uint32_t)n, want_counts, want_counts ? cn.p : nullptr, want_counts ? cp.p : nullptr, nullptr);
    auto kind = out->mem == RRT_MEM_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
    const uint32_t ug = (uint32_t)((n + kBlock - 1) / kBlock);
    if (out->mem == RRT_MEM_DEVICE) {
      hipLaunchKernelGGL((k_unpack_hits<R>), dim3(ug), dim3(kBlock), 0, st_, pool_, (const Tri<R>*)tris_.p, (R*)out->t, (int32_t*)out->prim, (R*)out->u, (R*)out->v, (uint32_t)n);
    } else {
      DevBuf<R> hr; DevBuf<int32_t> hp;
      hr.alloc(3 * n); hp.alloc(n);
      hipLaunchKernelGGL((k_unpack_hits<R>), dim3(ug), dim3(kBlock), 0, st_, pool_, (const Tri<R>*)tris_.p, hr.p, hp.p, hr.p + n, hr.p + 2 * n, (uint32_t)n);
      HIP_CHECK(hipMemcpyAsync(out->t, hr.p, n * sizeof(R), kind, st_));
      HIP_CHECK(hipMemcpyAsync(out->prim, hp.p, n * sizeof(int32_t), kind, st_));
      if (out->u) HIP_CHECK(hipMemcpyAsync(out->u, hr.p + n, n * sizeof(R), kind, st_));
      if (out->v) HIP_CHECK(hipMemcpyAsync(out->v, hr.p + 2 * n, n * sizeof(R), kind, st_));
      HIP_CHECK(hipStreamSynchronize(st_));   // staging buffers go out of scope
    }
    if (want_counts) {
      HIP_CHECK(hipMemcpyAsync(out->nodes_visited, cn.p, n * sizeof(uint32_t), kind, st_));
      HIP_CHECK(hipMemcpyAsync(out->prims_tested, cp.p, n * sizeof(uint32_t), kind, st_));
    }
    HIP_CHECK(hipStreamSynchronize(st_));
  }
  void trace_any(const rrt_rays* rays, size_t n, uint8_t* occluded) override {
    HIP_CHECK(hipSetDevice(dev_));
    if (rays->precision != precision()) throw std::invalid_argument("ray precision must match the handle");
    ensure_pools(n);
    load_rays(rays, n);
    DevBuf<uint8_t> occ;
    uint8_t* dst = occluded;
    if (rays->mem != RRT_MEM_DEVICE) { occ.alloc(n); dst = occ.p; }
    const uint32_t grid = (uint32_t)((n + kBlock - 1) / kBlock);
    hipLaunchKernelGGL(k_rotate, dim3(1), dim3(1), 0, st_, counters_.p, 3);
    launch_any(grid, st_, /*ao=*/false, (uint32_t)n, dst);
    if (rays->mem != RRT_MEM_DEVICE) HIP_CHECK(hipMemcpyAsync(occluded, occ.p, n, hipMemcpyDeviceToHost, st_));
    HIP_CHECK(hipStreamSynchronize(st_));
  }

  void camera_samples(const int32_t rect[4], uint64_t s0, uint64_t s1, double* dims5, double* ray_od6, double* weight) override {
    device_prologue(/*film=*/false);
    check_rect("camera_samples: rect outside the film", rect, /*allow_empty=*/true);
    if (s1 < s0 || s1 > desc_.sampler.samples_per_pixel) throw std::invalid_argument("camera_samples: sample range outside [0, samples_per_pixel]");
    const size_t npix = (size_t)(rect[2] - rect[0]) * (size_t)(rect[3] - rect[1]), ns = (size_t)(s1 - s0), n = npix * ns;
    if (n == 0) return;
    if (n > max_paths_) throw std::invalid_argument("camera_samples: more samples than pool slots (max_paths)");
    ensure_pools(n);
    DevBuf<double> dd, dr, dw;
    dd.alloc(5 * n); dr.alloc(6 * n); dw.alloc(n);
    PassDesc pd{rect[0], rect[1], rect[2] - rect[0], 0u, (uint32_t)npix, (uint32_t)s0, (uint32_t)ns, 1u << 30, 1u, 0u, 0u};
    hipLaunchKernelGGL(k_rotate, dim3(1), dim3(1), 0, st_, counters_.p, 2);
    const uint32_t g = (uint32_t)((n + kBlock - 1) / kBlock);
    launch_raygen(pd, g, dd.p, 1);
    HIP_CHECK(hipMemsetAsync(dr.p, 0, 6 * n * sizeof(double), st_));
    hipLaunchKernelGGL((k_camera_dump<R>), dim3(g), dim3(kBlock), 0, st_, pool_, pd, dr.p, dw.p);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipMemcpyAsync(dims5, dd.p, 5 * n * sizeof(double), hipMemcpyDeviceToHost, st_));
    HIP_CHECK(hipMemcpyAsync(ray_od6, dr.p, 6 * n * sizeof(double), hipMemcpyDeviceToHost, st_));
    HIP_CHECK(hipMemcpyAsync(weight, dw.p, n * sizeof(double), hipMemcpyDeviceToHost, st_));
    HIP_CHECK(hipStreamSynchronize(st_));
  }

  // rrt_sampler_values: the sampler's unit-test surface (k_sampler_values). Everything is checked on the host first, so the kernel sets no error
  // bit; it touches neither the pools nor the counters, so the handle is left as it was.
  void sampler_values(const uint32_t* pixel, const uint32_t* sample_num, size_t n, uint32_t first, uint32_t count, uint64_t* index, double* v1, double* v2) override {
    const std::string who = "rrt_sampler_values";
    check_args(who, kWhenIdle);
    const rrt_film& f = desc_.film;
    const uint64_t nsamp = desc_.sampler.samples_per_pixel, total = (uint64_t)n * count;
    if (total > 0x7fffffffu) throw std::invalid_argument(who + ": batch too large (n * count)");
    const bool st = desc_.sampler.type == RRT_SAMPLER_STRATIFIED;
    if (!st && (uint64_t)first + count >= 1000u) throw std::invalid_argument(who + ": the range reaches Halton dimension 1000 (v2 reads dimension first + count)");
    if (st && (uint64_t)first + count > (uint64_t)kStMask) throw std::invalid_argument(who + ": the range reaches Stratified counter 4095");
    for (size_t i = 0; i < n; i++) {
      const uint32_t pw = pixel[i];
      if ((int32_t)(pw & 0xffffu) >= f.xres || (int32_t)(pw >> 16) >= f.yres) throw std::invalid_argument(who + ": pixel outside the film (stream " + std::to_string(i) + ")");
      if (sample_num[i] >= nsamp) throw std::invalid_argument(who + ": sample_num outside 0 .. nsamp-1 (stream " + std::to_string(i) + ")");
    }
    device_prologue(/*film=*/false);
    DevBuf<uint32_t> du;
    DevBuf<unsigned long long> di;
    DevBuf<double> dv;
    du.alloc(2 * n); di.alloc(n); dv.alloc(3 * total);
    HIP_CHECK(hipMemcpyAsync(du.p, pixel, n * sizeof(uint32_t), hipMemcpyHostToDevice, st_));
    HIP_CHECK(hipMemcpyAsync(du.p + n, sample_num, n * sizeof(uint32_t), hipMemcpyHostToDevice, st_));
    hipLaunchKernelGGL((k_sampler_values<R>), dim3((uint32_t)((total + kBlock - 1) / kBlock)), dim3(kBlock), 0, st_, scene_, du.p, du.p + n, (uint32_t)n, first, count, di.p, dv.p,
                       dv.p + total);
    HIP_CHECK(hipGetLastError());
    if (index) HIP_CHECK(hipMemcpyAsync(index, di.p, n * sizeof(uint64_t), hipMemcpyDeviceToHost, st_));
    HIP_CHECK(hipMemcpyAsync(v1, dv.p, total * sizeof(double), hipMemcpyDeviceToHost, st_));
    HIP_CHECK(hipMemcpyAsync(v2, dv.p + total, 2 * total * sizeof(double), hipMemcpyDeviceToHost, st_));
    HIP_CHECK(hipStreamSynchronize(st_));
  }

  // ---- radiance along caller-supplied rays: rrt_radiance, rrt_render_rays ------------------------------------------------------------------------
  // k_ingest_rays in place of the camera kernels, then pass_integrate as a frame's pass runs it; what follows is k_radiance_out (rrt_radiance) or the
  // frame's own film part (rrt_render_rays). No camera kernel has run for these passes, so the first closest-hit launch goes the generic queue way:
  // no tile trees, no root cull, no film-record runs (RaysPassState, put back by its RaygenStateGuard). Horizon tables, shadow lists, the two shadow
  // queues and shading compaction depend on geometry only and stay on.
  struct RaysPassState : RaygenStateGuard {
    explicit RaysPassState(Handle* hh) : RaygenStateGuard(hh) { hh->tt_pass_ok_ = false; hh->film_runs_ok_ = false; hh->scene_.root_cull = 0u; }
  };
  // the caller's arrays as the kernel takes them: the pointers themselves for device memory, else copies in `stage` (n elements each)
  struct RayStage { DevBuf<R> r; DevBuf<uint32_t> u; };
  RaySamples<R> ray_samples_device(const rrt_ray_samples* rays, const void* p_film, size_t n, bool with_stream, RayStage& stage) {
    const bool diffs = rays->rxo[0] != nullptr && tex_depth_ > 0;   // read only when the scene has textured materials
    const void* real[20];
    int nr = 0;
    const void* const od[6] = {rays->ox, rays->oy, rays->oz, rays->dx, rays->dy, rays->dz};
    for (int k = 0; k < 6; k++) real[nr++] = od[k];
    real[nr++] = rays->weight;
    for (int k = 0; k < 3; k++) real[nr++] = diffs ? rays->rxo[k] : nullptr;
    for (int k = 0; k < 3; k++) real[nr++] = diffs ? rays->rxd[k] : nullptr;
    for (int k = 0; k < 3; k++) real[nr++] = diffs ? rays->ryo[k] : nullptr;
    for (int k = 0; k < 3; k++) real[nr++] = diffs ? rays->ryd[k] : nullptr;
    const void* pf = p_film;
    const void* words[2] = {with_stream ? rays->pixel : nullptr, with_stream ? rays->sample_num : nullptr};
    if (rays->mem != RRT_MEM_DEVICE) {
      size_t need = p_film ? 2 * n : 0;
      for (int k = 0; k < nr; k++) if (real[k]) need += n;
      stage.r.alloc(need);
      R* dst = stage.r.p;
      for (int k = 0; k < nr; k++) if (real[k]) { HIP_CHECK(hipMemcpyAsync(dst, real[k], n * sizeof(R), hipMemcpyHostToDevice, st_)); real[k] = dst; dst += n; }
      if (p_film) { HIP_CHECK(hipMemcpyAsync(dst, p_film, 2 * n * sizeof(R), hipMemcpyHostToDevice, st_)); pf = dst; }
      if (with_stream) {
        stage.u.alloc(2 * n);
        for (int k = 0; k < 2; k++) { HIP_CHECK(hipMemcpyAsync(stage.u.p + k * n, words[k], n * sizeof(uint32_t), hipMemcpyHostToDevice, st_)); words[k] = stage.u.p + k * n; }
      }
    }
    RaySamples<R> in{};
    for (int k = 0; k < 3; k++) {
      in.o[k] = (const R*)real[k]; in.d[k] = (const R*)real[3 + k];
      in.rxo[k] = (const R*)real[7 + k]; in.rxd[k] = (const R*)real[10 + k]; in.ryo[k] = (const R*)real[13 + k]; in.ryd[k] = (const R*)real[16 + k];
    }
    in.weight = (const R*)real[6];
    in.p_film = (const R*)pf;
    in.pixel = (const uint32_t*)words[0]; in.sample_num = (const uint32_t*)words[1];
    return in;
  }
  void launch_ingest(const PassDesc& pd, RaySamples<R> in, int check_only) {
    // workgroup shape (RaySamples::pb_log2): the next power of two >= min(ns, 32) samples, the rest of the 256 threads pixels
    uint32_t sb = 1;
    while (sb < std::min<uint32_t>(pd.ns, 32u)) sb <<= 1;
    const uint32_t pb = (uint32_t)kBlock / sb;
    in.pb_log2 = 0;
    while ((1u << in.pb_log2) < pb) in.pb_log2++;
    const dim3 g((pd.npix + pb * kIngestTiles - 1) / (pb * kIngestTiles), (pd.ns + sb - 1) / sb);
    const int enqueue = desc_.integrator.type != RRT_INT_AO ? 1 : 0;
    hipLaunchKernelGGL((k_ingest_rays<R>), g, dim3(kBlock), 0, st_, scene_, pool_, pd, in, enqueue, in.p_film != nullptr && wide_filter() ? 1 : 0, check_only);
    if (enqueue && !check_only) hipLaunchKernelGGL(k_ingest_count, dim3(1), dim3(1), 0, st_, counters_.p);
    HIP_CHECK(hipGetLastError());
  }
  bool ingest_refused() {
    uint32_t err = 0;
    HIP_CHECK(hipStreamSynchronize(st_));
    HIP_CHECK(hipMemcpy(&err, counters_.p + C_ERROR, sizeof(err), hipMemcpyDeviceToHost));
    return (err & ERR_INGEST) != 0u;
  }
  void radiance(const rrt_ray_samples* rays, size_t n, void* rgb4) override {
    using V4 = typename Vec4T<R>::type;
    check_args("rrt_radiance", kWhenIdle, Prec{"ray", rays->precision});
    const rrt_film& f = desc_.film;
    const uint64_t nsamp = desc_.sampler.samples_per_pixel;
    const bool host = rays->mem != RRT_MEM_DEVICE;
    if (host) {   // device-resident arrays: the same check by k_ingest_rays, below
      for (size_t i = 0; i < n; i++) {
        const uint32_t pw = rays->pixel[i], sn = rays->sample_num[i];
        if ((int32_t)(pw & 0xffffu) >= f.xres || (int32_t)(pw >> 16) >= f.yres) throw std::invalid_argument("rrt_radiance: pixel outside the film (ray " + std::to_string(i) + ")");
        if (sn < 1 || sn >= nsamp) throw std::invalid_argument("rrt_radiance: sample_num outside 1 .. nsamp-1 (ray " + std::to_string(i) + ")");
      }
    }
    device_prologue(/*film=*/false);
    RaysPassState guard(this);
    HIP_CHECK(hipMemsetAsync(counters_.p, 0, C_COUNT * sizeof(uint32_t), st_));
    if (totals_.n == 0) totals_.alloc(12);
    HIP_CHECK(hipMemsetAsync(totals_.p, 0, 12 * sizeof(unsigned long long), st_));
    const size_t chunk = pool_slots(n);
    ensure_pools(chunk);
    RayStage stage;
    RaySamples<R> in = ray_samples_device(rays, nullptr, n, true, stage);
    const PassDesc whole{0, 0, 1, 0u, (uint32_t)n, 1u, 1u, 1u << 30, 1u, 0u, 0u};
    if (!host) {
      launch_ingest(whole, in, 1);
      if (ingest_refused()) {
        HIP_CHECK(hipMemsetAsync(counters_.p + C_ERROR, 0, sizeof(uint32_t), st_));
        throw std::invalid_argument("rrt_radiance: a pixel outside the film or a sample_num outside 1 .. nsamp-1");
      }
    }
    DevBuf<V4> out_stage;
    if (host) out_stage.alloc(n);
    V4* const out = host ? out_stage.p : (V4*)rgb4;
    FrameRec fr;   // no statistics: no events
    for (size_t base = 0; base < n; base += chunk) {
      PassDesc pd = whole;
      pd.npix = (uint32_t)std::min(chunk, n - base);
      in.base = base;
      hipLaunchKernelGGL(k_rotate, dim3(1), dim3(1), 0, st_, counters_.p, 2);
      launch_ingest(pd, in, 0);
      pass_integrate(pd, 0u, fr);
      hipLaunchKernelGGL((k_radiance_out<R>), dim3((pd.npix + kBlock - 1) / kBlock), dim3(kBlock), 0, st_, pool_, out + base, pd.npix);
      HIP_CHECK(hipGetLastError());
    }
    if (host) HIP_CHECK(hipMemcpyAsync(rgb4, out_stage.p, n * sizeof(V4), hipMemcpyDeviceToHost, st_));
    HIP_CHECK(hipStreamSynchronize(st_));
    HIP_CHECK(hipStreamSynchronize(st2_));
    check_device_errors();
  }
  // ---- irradiance and SH probes at caller-supplied points: rrt_irradiance, rrt_irradiance_rays ---------------------------------------------------
  // radiance() with k_irr_gen in place of k_ingest_rays and k_irr_reduce in place of k_radiance_out: the rays are made on the device and only sums
  // leave it. A pass holds whole draw ranges of as many points as the pools take, or, where one range exceeds the pools, a sub-range of one point's
  // draws; the reducer adds a pass's draws onto the caller's row, so the cut changes no bit.
  void launch_irr_gen(const PassDesc& pd, const IrrPoints<R>& in, int check_only, R* od6) {
    const dim3 g((pd.npix + kBlock - 1) / kBlock, check_only ? 1u : (pd.ns + kIngestTiles - 1) / kIngestTiles);
    const int enqueue = desc_.integrator.type != RRT_INT_AO ? 1 : 0;
    hipLaunchKernelGGL((k_irr_gen<R>), g, dim3(kBlock), 0, st_, scene_, pool_, pd, in, enqueue, check_only, od6);
    if (enqueue && !check_only && !od6) hipLaunchKernelGGL(k_ingest_count, dim3(1), dim3(1), 0, st_, counters_.p);
    HIP_CHECK(hipGetLastError());
  }
  void irradiance(const char* who_c, const rrt_points* pts, size_t n, uint64_t s0, uint64_t s1, int mode, double offset, void* sums4, void* sh27, void* od6_user) override {
    const std::string who(who_c);
    check_args(who, kWhenIdle, Prec{"point", pts->precision});
    const rrt_film& f = desc_.film;
    if (s0 < 1 || s1 > desc_.sampler.samples_per_pixel || s0 >= s1) throw std::invalid_argument(who + ": draw range outside [1, nsamp) or empty");
    // the StratifiedSampler's first 2D value is the film sample of its stratum, not a point of [0, 1)^2 that the draws of a pixel cover evenly
    if (desc_.sampler.type == RRT_SAMPLER_STRATIFIED) throw UnsupportedError(who + " under the StratifiedSampler (a draw's direction is the stream's first 2D value: use the HaltonSampler)");
    const bool host = pts->mem != RRT_MEM_DEVICE;
    if (host && pts->pixel) {   // device-resident arrays: the same check by k_irr_gen, below
      for (size_t i = 0; i < n; i++) {
        const uint32_t pw = pts->pixel[i];
        if ((int32_t)(pw & 0xffffu) >= f.xres || (int32_t)(pw >> 16) >= f.yres) throw std::invalid_argument(who + ": pixel outside the film (point " + std::to_string(i) + ")");
      }
    }
    device_prologue(/*film=*/false);
    RaysPassState guard(this);
    HIP_CHECK(hipMemsetAsync(counters_.p, 0, C_COUNT * sizeof(uint32_t), st_));
    if (totals_.n == 0) totals_.alloc(12);
    HIP_CHECK(hipMemsetAsync(totals_.p, 0, 12 * sizeof(unsigned long long), st_));
    const size_t ns_all = (size_t)(s1 - s0);
    const size_t cap = pool_slots(n * ns_all);
    if (!od6_user) ensure_pools(cap);
    // the caller's arrays as the kernels take them: the pointers themselves for device memory, else copies
    const void* arr[6] = {pts->px, pts->py, pts->pz, pts->nx, pts->ny, pts->nz};
    const int n_arr = pts->nx ? 6 : 3;
    const uint32_t* pixel = pts->pixel;
    DevBuf<R> stage_r, stage_out;
    DevBuf<uint32_t> stage_u;
    if (host) {
      stage_r.alloc((size_t)n_arr * n);
      for (int k = 0; k < n_arr; k++) { HIP_CHECK(hipMemcpyAsync(stage_r.p + (size_t)k * n, arr[k], n * sizeof(R), hipMemcpyHostToDevice, st_)); arr[k] = stage_r.p + (size_t)k * n; }
      if (pixel) { stage_u.alloc(n); HIP_CHECK(hipMemcpyAsync(stage_u.p, pixel, n * sizeof(uint32_t), hipMemcpyHostToDevice, st_)); pixel = stage_u.p; }
    }
    IrrPoints<R> in{};
    for (int k = 0; k < 3; k++) { in.p[k] = (const R*)arr[k]; in.n[k] = n_arr == 6 ? (const R*)arr[3 + k] : nullptr; }
    in.pixel = pixel; in.offset = (R)offset; in.mode = (uint32_t)mode; in.s0 = (uint32_t)s0; in.ns_all = (uint32_t)ns_all;
    const PassDesc whole{0, 0, 1, 0u, (uint32_t)n, (uint32_t)s0, 1u, 1u << 30, 1u, 0u, 0u};
    if (!host && pixel) {
      launch_irr_gen(whole, in, 1, nullptr);
      if (ingest_refused()) {
        HIP_CHECK(hipMemsetAsync(counters_.p + C_ERROR, 0, sizeof(uint32_t), st_));
        throw std::invalid_argument(who + ": a pixel outside the film");
      }
    }
    // outputs: the caller's own rows in device memory, else copies that start from what the caller's rows hold
    const size_t n_sums = od6_user ? 0 : 4 * n, n_sh = sh27 ? 27 * n : 0, n_od6 = od6_user ? 6 * n * ns_all : 0;
    R *d_sums = (R*)sums4, *d_sh = (R*)sh27, *d_od6 = (R*)od6_user;
    if (host) {
      stage_out.alloc(n_sums + n_sh + n_od6);
      d_sums = stage_out.p; d_sh = sh27 ? stage_out.p + n_sums : nullptr; d_od6 = od6_user ? stage_out.p : nullptr;
      if (n_sums) HIP_CHECK(hipMemcpyAsync(d_sums, sums4, n_sums * sizeof(R), hipMemcpyHostToDevice, st_));
      if (n_sh) HIP_CHECK(hipMemcpyAsync(d_sh, sh27, n_sh * sizeof(R), hipMemcpyHostToDevice, st_));
    }
    // draws per pass (the launch grid's second dimension counts kIngestTiles of them), points per pass
    const size_t dpc = std::min<size_t>({ns_all, cap, (size_t)kIngestTiles * 65535u});
    const size_t ppc = std::max<size_t>(1, std::min(n, cap / dpc));
    FrameRec fr;   // no statistics: no events
    for (size_t p0 = 0; p0 < n; p0 += ppc) {
      for (uint64_t sb = s0; sb < s1; sb += dpc) {
        PassDesc pd = whole;
        pd.npix = (uint32_t)std::min(ppc, n - p0);
        pd.s_begin = (uint32_t)sb; pd.ns = (uint32_t)std::min<uint64_t>(dpc, s1 - sb);
        in.base = p0;
        if (od6_user) { launch_irr_gen(pd, in, 0, d_od6); continue; }
        hipLaunchKernelGGL(k_rotate, dim3(1), dim3(1), 0, st_, counters_.p, 2);
        launch_irr_gen(pd, in, 0, nullptr);
        pass_integrate(pd, 0u, fr);
        hipLaunchKernelGGL((k_irr_reduce<R>), dim3((pd.npix + kBlock - 1) / kBlock), dim3(kBlock), 0, st_, scene_, pool_, pd, (uint64_t)p0, d_sums, d_sh);
        HIP_CHECK(hipGetLastError());
      }
    }
    if (host) {
      if (n_sums) HIP_CHECK(hipMemcpyAsync(sums4, d_sums, n_sums * sizeof(R), hipMemcpyDeviceToHost, st_));
      if (n_sh) HIP_CHECK(hipMemcpyAsync(sh27, d_sh, n_sh * sizeof(R), hipMemcpyDeviceToHost, st_));
      if (n_od6) HIP_CHECK(hipMemcpyAsync(od6_user, d_od6, n_od6 * sizeof(R), hipMemcpyDeviceToHost, st_));
    }
    HIP_CHECK(hipStreamSynchronize(st_));
    HIP_CHECK(hipStreamSynchronize(st2_));
    check_device_errors();
  }
  // ---- surface records and lightmap sites: rrt_surface_rays, rrt_surface_at, rrt_atlas_sites ------------------------------------------------------
  // The rays form is trace_closest() with k_surface in place of k_unpack_hits: the same load_rays, k_rotate and launch_closest, so the pool's hit
  // records are the ones rrt_trace_closest unpacks. The sites form launches k_surface alone. Host arrays are staged and copied back per array.
  void surface(const char* who_c, const rrt_rays* rays, const rrt_sites* sites, size_t n, const rrt_surface* out) override {
    const std::string who(who_c);
    check_args(who, kWhenIdle, Prec{"record", out->precision});
    if ((rays ? rays->precision : sites->precision) != precision()) throw std::invalid_argument(who + ": " + (rays ? "ray" : "site") + " precision must match the handle");
    const bool host = out->mem != RRT_MEM_DEVICE;
    if (sites && host) {   // device-resident sites: the same checks by k_sites_check, below
      const R *b1 = (const R*)sites->b1, *b2 = (const R*)sites->b2;
      for (size_t i = 0; i < n; i++) {
        const int32_t pr = sites->prim[i];
        if (pr == -1) continue;
        const std::string at = " (site " + std::to_string(i) + ")";
        if (pr < 0 || (size_t)pr >= surf_sphere_.size()) throw std::invalid_argument(who + ": prim outside [0, n_prim_order)" + at);
        if (surf_sphere_[pr]) throw std::invalid_argument(who + ": prim names a sphere (its record needs the ray: rrt_surface_rays)" + at);
        if (!std::isfinite((double)b1[i]) || !std::isfinite((double)b2[i])) throw std::invalid_argument(who + ": non-finite barycentric" + at);
      }
    }
    device_prologue(/*film=*/false);
    HIP_CHECK(hipMemsetAsync(counters_.p, 0, C_COUNT * sizeof(uint32_t), st_));
    // the caller's arrays as the kernel takes them: the pointers themselves for device memory, else staging
    void* const real[15] = {out->px, out->py, out->pz, out->nx, out->ny, out->nz, out->sx, out->sy, out->sz, out->tu, out->tv, out->rho_r, out->rho_g, out->rho_b, out->t};
    R* dev_r[15];
    int32_t *dev_prim = out->prim, *dev_mat = out->material;
    DevBuf<R> stage_r, stage_in;
    DevBuf<int32_t> stage_i, stage_prim;
    if (host) {
      size_t n_real = 0;
      for (int k = 0; k < 15; k++) n_real += real[k] != nullptr;
      stage_r.alloc(n_real * n);
      R* next = stage_r.p;
      for (int k = 0; k < 15; k++) { dev_r[k] = real[k] ? next : nullptr; if (real[k]) next += n; }
      if (out->prim) { stage_i.alloc(2 * n); dev_prim = stage_i.p; dev_mat = stage_i.p + n; }
    } else {
      for (int k = 0; k < 15; k++) dev_r[k] = (R*)real[k];
    }
    SurfaceOut<R> so{};
    for (int k = 0; k < 3; k++) { so.p[k] = dev_r[k]; so.n[k] = dev_r[3 + k]; so.s[k] = dev_r[6 + k]; so.rho[k] = dev_r[11 + k]; }
    so.uv[0] = dev_r[9]; so.uv[1] = dev_r[10]; so.t = dev_r[14]; so.prim = dev_prim; so.material = dev_mat;
    const dim3 grid((uint32_t)((n + kBlock - 1) / kBlock));
    if (rays) {
      ensure_pools(n);
      load_rays(rays, n);
      hipLaunchKernelGGL(k_rotate, dim3(1), dim3(1), 0, st_, counters_.p, 3);
      launch_closest(nullptr, nullptr, (uint32_t)n, false, nullptr, nullptr, nullptr);
      with_flag(tex_depth_ > 0, [&](auto TEX) { hipLaunchKernelGGL((k_surface<R, TEX(), false>), grid, dim3(kBlock), 0, st_, scene_, pool_, SitesIn<R>{}, so, (uint32_t)n); });
    } else {
      SitesIn<R> in{sites->prim, (const R*)sites->b1, (const R*)sites->b2};
      if (host) {
        stage_in.alloc(2 * n); stage_prim.alloc(n);
        HIP_CHECK(hipMemcpyAsync(stage_prim.p, sites->prim, n * sizeof(int32_t), hipMemcpyHostToDevice, st_));
        HIP_CHECK(hipMemcpyAsync(stage_in.p, sites->b1, n * sizeof(R), hipMemcpyHostToDevice, st_));
        HIP_CHECK(hipMemcpyAsync(stage_in.p + n, sites->b2, n * sizeof(R), hipMemcpyHostToDevice, st_));
        in = SitesIn<R>{stage_prim.p, stage_in.p, stage_in.p + n};
      } else {
        hipLaunchKernelGGL((k_sites_check<R>), grid, dim3(kBlock), 0, st_, scene_, in, (uint32_t)n);
        HIP_CHECK(hipGetLastError());
        uint32_t err = 0;
        HIP_CHECK(hipStreamSynchronize(st_));
        HIP_CHECK(hipMemcpy(&err, counters_.p + C_ERROR, sizeof(err), hipMemcpyDeviceToHost));
        if (err & ERR_SITE) {
          HIP_CHECK(hipMemsetAsync(counters_.p + C_ERROR, 0, sizeof(uint32_t), st_));
          throw std::invalid_argument(who + ": a refused site (a prim outside [0, n_prim_order) other than -1, a sphere, or a non-finite barycentric)");
        }
      }
      with_flag(tex_depth_ > 0, [&](auto TEX) { hipLaunchKernelGGL((k_surface<R, TEX(), true>), grid, dim3(kBlock), 0, st_, scene_, pool_, in, so, (uint32_t)n); });
    }
    HIP_CHECK(hipGetLastError());
    if (host) {
      for (int k = 0; k < 15; k++) if (real[k]) HIP_CHECK(hipMemcpyAsync(real[k], dev_r[k], n * sizeof(R), hipMemcpyDeviceToHost, st_));
      if (out->prim) {
        HIP_CHECK(hipMemcpyAsync(out->prim, dev_prim, n * sizeof(int32_t), hipMemcpyDeviceToHost, st_));
        HIP_CHECK(hipMemcpyAsync(out->material, dev_mat, n * sizeof(int32_t), hipMemcpyDeviceToHost, st_));
      }
    }
    HIP_CHECK(hipStreamSynchronize(st_));
    check_device_errors();
  }
  // k_atlas_owner over the candidate list (the caller's, or every triangle entry of prim_order), k_atlas_emit over the texels
  void atlas_sites(int32_t aw, int32_t ah, const int32_t* prims, size_t n_list, int mem, int32_t* site_prim, void* b1, void* b2, uint64_t* n_covered) override {
    const std::string who("rrt_atlas_sites");
    check_args(who, kWhenIdle);
    std::vector<int32_t> list;
    if (prims) {
      for (size_t i = 0; i < n_list; i++) {
        const int32_t pr = prims[i];
        if (pr < 0 || (size_t)pr >= surf_sphere_.size()) throw std::invalid_argument(who + ": list entry outside [0, n_prim_order) (entry " + std::to_string(i) + ")");
        if (surf_sphere_[pr]) throw std::invalid_argument(who + ": list entry names a sphere (entry " + std::to_string(i) + ")");
      }
      list.assign(prims, prims + n_list);
    } else {
      for (size_t i = 0; i < surf_sphere_.size(); i++) if (!surf_sphere_[i]) list.push_back((int32_t)i);
    }
    HIP_CHECK(hipSetDevice(dev_));
    const size_t nt = (size_t)aw * (size_t)ah;
    const bool host = mem != RRT_MEM_DEVICE;
    DevBuf<uint32_t> owner;
    DevBuf<int32_t> dlist, stage_i;
    DevBuf<unsigned long long> count;
    DevBuf<R> stage_r;
    owner.alloc(nt); count.alloc(1);
    HIP_CHECK(hipMemsetAsync(owner.p, 0xff, nt * sizeof(uint32_t), st_));
    HIP_CHECK(hipMemsetAsync(count.p, 0, sizeof(unsigned long long), st_));
    dlist.upload(list, st_);
    int32_t* d_prim = site_prim;
    R *d_b1 = (R*)b1, *d_b2 = (R*)b2;
    if (host) { stage_i.alloc(nt); stage_r.alloc(2 * nt); d_prim = stage_i.p; d_b1 = stage_r.p; d_b2 = stage_r.p + nt; }
    if (!list.empty()) {
      const size_t blocks = (list.size() * 64 + kBlock - 1) / kBlock;
      hipLaunchKernelGGL((k_atlas_owner<R>), dim3((uint32_t)blocks), dim3(kBlock), 0, st_, scene_, (const int32_t*)dlist.p, (uint32_t)list.size(), (uint32_t)aw, (uint32_t)ah, owner.p);
    }
    hipLaunchKernelGGL((k_atlas_emit<R>), dim3((uint32_t)((nt + kBlock - 1) / kBlock)), dim3(kBlock), 0, st_, scene_, (const int32_t*)dlist.p, (const uint32_t*)owner.p, (uint32_t)aw, (uint32_t)ah,
                       d_prim, d_b1, d_b2, count.p);
    HIP_CHECK(hipGetLastError());
    if (host) {
      HIP_CHECK(hipMemcpyAsync(site_prim, d_prim, nt * sizeof(int32_t), hipMemcpyDeviceToHost, st_));
      HIP_CHECK(hipMemcpyAsync(b1, d_b1, nt * sizeof(R), hipMemcpyDeviceToHost, st_));
      HIP_CHECK(hipMemcpyAsync(b2, d_b2, nt * sizeof(R), hipMemcpyDeviceToHost, st_));
    }
    unsigned long long c = 0;
    if (n_covered) HIP_CHECK(hipMemcpyAsync(&c, count.p, sizeof(c), hipMemcpyDeviceToHost, st_));
    HIP_CHECK(hipStreamSynchronize(st_));   // the work buffers go out of scope
    if (n_covered) *n_covered = (uint64_t)c;
  }
  // ---- nearest-surface point queries: rrt_nearest ------------------------------------------------------------------------------------------------
  // One lane per point, no pool and no queue: the points are cut into passes of at most max_paths (and 2^20) points only to bound the stack arrays,
  // which the handle keeps between calls. k_nearest<R> runs in both precisions; fp32 handles with a pair-node tree run k_nearest_pairs_f32 under option
  // "nearest_pairs" (measured slower: DESIGN.md). A point's result depends on the point alone, so neither the cut nor the kernel changes a bit. Host arrays are staged and copied back per array.
  void nearest(const rrt_points* pts, size_t n, double max_dist, const rrt_nearest_out* out) override {
    const std::string who("rrt_nearest");
    check_args(who, kWhenIdle, Prec{"point", pts->precision});
    if (out->precision != precision()) throw std::invalid_argument(who + ": output precision must match the handle");
    if (!nn_has_tri_) throw UnsupportedError(who + ": the scene has no triangle entry (spheres are not candidates)");
    HIP_CHECK(hipSetDevice(dev_));
    HIP_CHECK(hipMemsetAsync(counters_.p + C_ERROR, 0, sizeof(uint32_t), st_));
    const bool host = pts->mem != RRT_MEM_DEVICE;
    DevBuf<R> stage_in, stage_out;
    DevBuf<int32_t> stage_prim;
    NearestIO<R> io{};
    io.px = (const R*)pts->px; io.py = (const R*)pts->py; io.pz = (const R*)pts->pz;
    io.prim = out->prim; io.b1 = (R*)out->b1; io.b2 = (R*)out->b2; io.dist = (R*)out->dist;
    if (host) {
      stage_in.alloc(3 * n); stage_out.alloc((out->dist ? 3 : 2) * n); stage_prim.alloc(n);
      const void* src[3] = {pts->px, pts->py, pts->pz};
      for (int k = 0; k < 3; k++) HIP_CHECK(hipMemcpyAsync(stage_in.p + (size_t)k * n, src[k], n * sizeof(R), hipMemcpyHostToDevice, st_));
      io.px = stage_in.p; io.py = stage_in.p + n; io.pz = stage_in.p + 2 * n;
      io.prim = stage_prim.p; io.b1 = stage_out.p; io.b2 = stage_out.p + n; io.dist = out->dist ? stage_out.p + 2 * n : nullptr;
    }
    io.max_dist = (R)max_dist; io.delta = nn_delta_; io.prune0 = nn_prune_start<R>(io.max_dist, io.delta);
    const size_t per_pass = std::min<size_t>({n, max_paths_, (size_t)1 << 20});
    const uint32_t depth = scene_.stack_depth;
    bool pairs = false;
    if constexpr (std::is_same<R, float>::value) pairs = pairs_ok_ && nn_pairs_on_;
    const size_t block = pairs ? (size_t)kNnBlock : (size_t)kBlock;
    const size_t stride = (per_pass + block - 1) / block * block;   // threads of a launch
    if (pairs) {
      if (depth > (uint32_t)kNnStackLds && nn_overflow_.n < (size_t)(depth - kNnStackLds) * stride) nn_overflow_.alloc((size_t)(depth - kNnStackLds) * stride);
    } else if (nn_stack_.n < (size_t)depth * stride) nn_stack_.alloc((size_t)depth * stride);
    for (size_t p0 = 0; p0 < n; p0 += per_pass) {
      const uint32_t m = (uint32_t)std::min(per_pass, n - p0);
      const dim3 grid((uint32_t)((m + block - 1) / block));
      if constexpr (std::is_same<R, float>::value) {
        if (pairs) {
          with_flag(mixed_, [&](auto MIXED) {
            hipLaunchKernelGGL((k_nearest_pairs_f32<MIXED()>), grid, dim3(kNnBlock), 0, st_, trav_, io, p0, m, scene_.n_tris, depth, counters_.p + C_ERROR, nn_overflow_.p, (uint32_t)stride);
          });
          continue;
        }
      }
      hipLaunchKernelGGL((k_nearest<R>), grid, dim3(kBlock), 0, st_, scene_.nodes, scene_.n_nodes, scene_.tris, scene_.n_tris, scene_.insts, counters_.p + C_ERROR, io, p0, m,
                         nn_stack_.p, (uint32_t)stride, depth);
    }
    HIP_CHECK(hipGetLastError());
    if (host) {
      HIP_CHECK(hipMemcpyAsync(out->prim, io.prim, n * sizeof(int32_t), hipMemcpyDeviceToHost, st_));
      HIP_CHECK(hipMemcpyAsync(out->b1, io.b1, n * sizeof(R), hipMemcpyDeviceToHost, st_));
      HIP_CHECK(hipMemcpyAsync(out->b2, io.b2, n * sizeof(R), hipMemcpyDeviceToHost, st_));
      if (out->dist) HIP_CHECK(hipMemcpyAsync(out->dist, io.dist, n * sizeof(R), hipMemcpyDeviceToHost, st_));
    }
    HIP_CHECK(hipStreamSynchronize(st_));
    check_device_errors();
  }
  // ---- all hits along a ray, in order: rrt_trace_all ---------------------------------------------------------------------------------------------
  // One lane per ray, no pool and no queue, as nearest(): the rays are cut into passes of at most max_paths (and 2^20) rays only to bound the deep
  // stack array, which the handle keeps between calls (trees deeper than 64 alone use it). A ray's result depends on the ray alone, so the cut
  // changes no bit. The k-buffer is dynamic LDS, k x kBlock x (sizeof(R) + 4) bytes a block: 32 KiB in fp32 and 48 KiB in f64 at k = 16, so three
  // f64 blocks fit the 160 KiB of a CU. Host arrays are staged and copied back per array.
  void trace_all(const rrt_rays* rays, size_t n, const rrt_multi_hits* out) override {
    const std::string who("rrt_trace_all");
    check_args(who, kWhenIdle, Prec{"ray", rays->precision});
    if (out->precision != precision()) throw std::invalid_argument(who + ": output precision must match the handle");
    if (!nn_has_tri_) throw UnsupportedError(who + ": the scene has no triangle entry (spheres are not candidates)");
    HIP_CHECK(hipSetDevice(dev_));
    HIP_CHECK(hipMemsetAsync(counters_.p + C_ERROR, 0, sizeof(uint32_t), st_));
    const bool host = rays->mem != RRT_MEM_DEVICE;
    const size_t k = (size_t)out->k, kn = k * n;
    const bool bary = k > 0 && out->b1 != nullptr;
    DevBuf<R> stage_in, stage_out;
    DevBuf<int32_t> stage_skip, stage_prim;
    DevBuf<uint32_t> stage_count;
    TraceAllIO<R> io{};
    io.ox = (const R*)rays->ox; io.oy = (const R*)rays->oy; io.oz = (const R*)rays->oz; io.dx = (const R*)rays->dx; io.dy = (const R*)rays->dy; io.dz = (const R*)rays->dz;
    io.tmax = (const R*)rays->tmax; io.skip = rays->skip_prim;
    io.t = k ? (R*)out->t : nullptr; io.prim = k ? out->prim : nullptr; io.b1 = bary ? (R*)out->b1 : nullptr; io.b2 = bary ? (R*)out->b2 : nullptr; io.count = out->count;
    io.n = n; io.k = (uint32_t)k; io.delta = mh_delta_;
    if (host) {
      stage_in.alloc(7 * n);
      const void* src[7] = {rays->ox, rays->oy, rays->oz, rays->dx, rays->dy, rays->dz, rays->tmax};
      for (int a = 0; a < 7; a++) HIP_CHECK(hipMemcpyAsync(stage_in.p + (size_t)a * n, src[a], n * sizeof(R), hipMemcpyHostToDevice, st_));
      io.ox = stage_in.p; io.oy = stage_in.p + n; io.oz = stage_in.p + 2 * n; io.dx = stage_in.p + 3 * n; io.dy = stage_in.p + 4 * n; io.dz = stage_in.p + 5 * n; io.tmax = stage_in.p + 6 * n;
      if (rays->skip_prim) { stage_skip.alloc(n); HIP_CHECK(hipMemcpyAsync(stage_skip.p, rays->skip_prim, n * sizeof(int32_t), hipMemcpyHostToDevice, st_)); io.skip = stage_skip.p; }
      if (k) {
        stage_out.alloc((bary ? 3 : 1) * kn); stage_prim.alloc(kn);
        io.t = stage_out.p; io.prim = stage_prim.p;
        if (bary) { io.b1 = stage_out.p + kn; io.b2 = stage_out.p + 2 * kn; }
      }
      if (out->count) { stage_count.alloc(n); io.count = stage_count.p; }
    }
    const size_t per_pass = std::min<size_t>({n, max_paths_, (size_t)1 << 20});
    const uint32_t depth = scene_.stack_depth;
    const size_t stride = (per_pass + kBlock - 1) / kBlock * kBlock;   // threads of a launch
    if (deep_ && mh_stack_.n < (size_t)depth * stride) mh_stack_.alloc((size_t)depth * stride);
    const size_t lds = k * (size_t)kBlock * (sizeof(R) + sizeof(int32_t));
    for (size_t p0 = 0; p0 < n; p0 += per_pass) {
      const uint32_t m = (uint32_t)std::min(per_pass, n - p0);
      const dim3 grid((uint32_t)((m + kBlock - 1) / kBlock));
      with_flag(deep_, [&](auto DEEP) {
        hipLaunchKernelGGL((k_trace_all<R, DEEP()>), grid, dim3(kBlock), lds, st_, scene_.nodes, scene_.n_nodes, scene_.tris, scene_.n_tris, scene_.insts, counters_.p + C_ERROR, io, p0, m,
                           deep_ ? mh_stack_.p : nullptr, (uint32_t)stride, depth);
      });
    }
    HIP_CHECK(hipGetLastError());
    if (host) {
      if (k) {
        HIP_CHECK(hipMemcpyAsync(out->t, io.t, kn * sizeof(R), hipMemcpyDeviceToHost, st_));
        HIP_CHECK(hipMemcpyAsync(out->prim, io.prim, kn * sizeof(int32_t), hipMemcpyDeviceToHost, st_));
        if (bary) {
          HIP_CHECK(hipMemcpyAsync(out->b1, io.b1, kn * sizeof(R), hipMemcpyDeviceToHost, st_));
          HIP_CHECK(hipMemcpyAsync(out->b2, io.b2, kn * sizeof(R), hipMemcpyDeviceToHost, st_));
        }
      }
      if (out->count) HIP_CHECK(hipMemcpyAsync(out->count, io.count, n * sizeof(uint32_t), hipMemcpyDeviceToHost, st_));
    }
    HIP_CHECK(hipStreamSynchronize(st_));
    check_device_errors();
  }
  // ---- mutual visibility of two point sets as a packed bit matrix: rrt_visibility ------------------------------------------------------------------
  // One lane per pair, one wave per output word (k_visibility), no pool and no queue. The words are cut into launches of at most max_paths (and 2^20)
  // threads, whole waves each, only to bound the deep stack array (trace_all's mh_stack_); a pair's bit depends on the pair alone, so the cut changes
  // no bit. The count plane is zeroed here and summed by integer atomics. Host arrays are staged and copied back per array, as trace_all's.
  void visibility(const rrt_points* a, size_t n_a, const rrt_points* b, size_t n_b, const rrt_vis_params* prm, const rrt_vis_out* out) override {
    const std::string who("rrt_visibility");
    check_args(who, kWhenIdle, Prec{"a", a->precision});
    if (b->precision != precision()) throw std::invalid_argument(who + ": b precision must match the handle");
    if (!nn_has_tri_) throw UnsupportedError(who + ": the scene has no triangle entry (spheres are not candidates)");
    HIP_CHECK(hipSetDevice(dev_));
    HIP_CHECK(hipMemsetAsync(counters_.p + C_ERROR, 0, sizeof(uint32_t), st_));
    const bool host = a->mem != RRT_MEM_DEVICE;
    const bool pairs = prm->mode == RRT_VIS_PAIRS;
    const bool an = a->nx != nullptr, bn = b->nx != nullptr;
    const size_t words = (n_b + 63) / 64;
    const size_t n_tasks = pairs ? (n_a + 63) / 64 : n_a * words;   // one wave, one output word each
    VisIO<R> io{};
    io.ax = (const R*)a->px; io.ay = (const R*)a->py; io.az = (const R*)a->pz; io.anx = (const R*)a->nx; io.any = (const R*)a->ny; io.anz = (const R*)a->nz;
    io.bx = (const R*)b->px; io.by = (const R*)b->py; io.bz = (const R*)b->pz; io.bnx = (const R*)b->nx; io.bny = (const R*)b->ny; io.bnz = (const R*)b->nz;
    io.skip_a = prm->skip_a; io.skip_b = prm->skip_b; io.bits = out->bits; io.count = out->count;
    io.n_a = (uint32_t)n_a; io.n_b = (uint32_t)n_b; io.words = (uint32_t)words; io.mode = prm->mode; io.b_kind = prm->b_kind; io.flags = prm->flags;
    io.off_a = (R)prm->offset_a; io.off_b = (R)prm->offset_b; io.delta = mh_delta_;
    DevBuf<R> stage_a, stage_b;
    DevBuf<int32_t> stage_skip_a, stage_skip_b;
    DevBuf<uint64_t> stage_bits;
    DevBuf<uint32_t> stage_count;
    if (host) {
      auto stage = [&](DevBuf<R>& buf, const rrt_points* s, size_t n, bool normals, const R** dst) {
        buf.alloc((normals ? 6 : 3) * n);
        const void* src[6] = {s->px, s->py, s->pz, s->nx, s->ny, s->nz};
        for (int k = 0; k < (normals ? 6 : 3); k++) {
          HIP_CHECK(hipMemcpyAsync(buf.p + (size_t)k * n, src[k], n * sizeof(R), hipMemcpyHostToDevice, st_));
          dst[k] = buf.p + (size_t)k * n;
        }
      };
      const R* pa[6] = {}; const R* pb[6] = {};
      stage(stage_a, a, n_a, an, pa); stage(stage_b, b, n_b, bn, pb);
      io.ax = pa[0]; io.ay = pa[1]; io.az = pa[2]; io.anx = pa[3]; io.any = pa[4]; io.anz = pa[5];
      io.bx = pb[0]; io.by = pb[1]; io.bz = pb[2]; io.bnx = pb[3]; io.bny = pb[4]; io.bnz = pb[5];
      if (prm->skip_a) { stage_skip_a.alloc(n_a); HIP_CHECK(hipMemcpyAsync(stage_skip_a.p, prm->skip_a, n_a * sizeof(int32_t), hipMemcpyHostToDevice, st_)); io.skip_a = stage_skip_a.p; }
      if (prm->skip_b) { stage_skip_b.alloc(n_b); HIP_CHECK(hipMemcpyAsync(stage_skip_b.p, prm->skip_b, n_b * sizeof(int32_t), hipMemcpyHostToDevice, st_)); io.skip_b = stage_skip_b.p; }
      stage_bits.alloc(n_tasks); io.bits = stage_bits.p;
      if (out->count) { stage_count.alloc(n_a); io.count = stage_count.p; }
    }
    if (io.count) HIP_CHECK(hipMemsetAsync(io.count, 0, n_a * sizeof(uint32_t), st_));
    const size_t per_pass = std::min<size_t>({n_tasks, std::max<size_t>(1, max_paths_ / 64), (size_t)1 << 14});   // waves of a launch: at most 2^20 threads
    const uint32_t depth = scene_.stack_depth;
    const size_t stride = (per_pass * 64 + kBlock - 1) / kBlock * kBlock;   // threads of a launch
    if (deep_ && mh_stack_.n < (size_t)depth * stride) mh_stack_.alloc((size_t)depth * stride);
    for (size_t t0 = 0; t0 < n_tasks; t0 += per_pass) {
      const uint32_t m = (uint32_t)std::min(per_pass, n_tasks - t0);
      const dim3 grid((uint32_t)(((size_t)m * 64 + kBlock - 1) / kBlock));
      with_flag(deep_, [&](auto DEEP) {
        hipLaunchKernelGGL((k_visibility<R, DEEP()>), grid, dim3(kBlock), 0, st_, scene_.nodes, scene_.n_nodes, scene_.tris, scene_.n_tris, scene_.insts, counters_.p + C_ERROR, io,
                           (unsigned long long)t0, m, deep_ ? mh_stack_.p : nullptr, (uint32_t)stride, depth);
      });
    }
    HIP_CHECK(hipGetLastError());
    if (host) {
      HIP_CHECK(hipMemcpyAsync(out->bits, io.bits, n_tasks * sizeof(uint64_t), hipMemcpyDeviceToHost, st_));
      if (out->count) HIP_CHECK(hipMemcpyAsync(out->count, io.count, n_a * sizeof(uint32_t), hipMemcpyDeviceToHost, st_));
    }
    HIP_CHECK(hipStreamSynchronize(st_));
    check_device_errors();
  }
  void render_rays(const int32_t rect[4], uint64_t s0, uint64_t s1, const rrt_ray_samples* rays, const void* p_film, void* film_user, int film_mem, rrt_render_stats* stats) override {
    check_args("rrt_render_rays", kWhenIdle, Prec{"ray", rays->precision}, {}, rect);
    if (s0 < 1 || s1 > desc_.sampler.samples_per_pixel || s0 >= s1) throw std::invalid_argument("rrt_render_rays: sample range outside [1, nsamp) or empty");
    device_prologue();
    const CallGeom g = call_geom(rect, kNoBands, 0, 1);
    const size_t ns_all = (size_t)(s1 - s0);
    RaysPassState guard(this);
    frame_setup(false, g.rpix * ns_all, /*tile_trees=*/false);
    RayStage stage;
    RaySamples<R> in = ray_samples_device(rays, p_film, g.rpix * ns_all, false, stage);
    in.s0 = (uint32_t)s0; in.ns_all = (uint32_t)ns_all;
    FrameRec fr;
    fr.camera_samples = (uint64_t)g.rpix * ns_all;
    fr.begin(stats != nullptr, st_);
    for_each_pass(g, s0 - 1, s1 - 1, cap_, [&](const PassDesc& pd) {
      hipLaunchKernelGGL(k_rotate, dim3(1), dim3(1), 0, st_, counters_.p, 2);
      const size_t e = tick(fr, 0);
      launch_ingest(pd, in, 0);
      tock(fr, e);
      pass_integrate(pd, 0u, fr);
      pass_film(pd, nullptr, g, false, 0u, fr);
    });
    fr.end(st_);
    merge_out(film_user, nullptr, film_mem, true);
    HIP_CHECK(hipStreamSynchronize(st2_));
    check_device_errors();
    if (stats) frame_stats(fr, stats);
  }

  // ---- the frame: SamplerIntegrator::si_render (integrator/mod.rs:48-139) over a pixel rect -------------------
  void render_rect(const int32_t rect[4], void* film_user, int film_mem, rrt_render_stats* stats) override {
    check_rect("render rect outside the film", rect);   // (the frame's own refusal: its text is older than the calls' names)
    render_impl(call_geom(rect, kNoBands, 0, 1), film_user, film_mem, stats);
  }
  // rows of the interleaved 16-row bands b with b % world == rank (partition.py), as ONE pixel set
  // the main stream carries the critical path (closest-hit -> shade); shadow rays fill what it leaves idle
  void create_streams(unsigned flags) {
    if (st_) { HIP_CHECK(hipStreamSynchronize(st_)); HIP_CHECK(hipStreamSynchronize(st2_)); (void)hipStreamDestroy(st2_); (void)hipStreamDestroy(st_); st_ = st2_ = nullptr; }
    int lo = 0, hi = 0;
    HIP_CHECK(hipDeviceGetStreamPriorityRange(&lo, &hi));
    HIP_CHECK(hipStreamCreateWithPriority(&st_, flags, hi));
    HIP_CHECK(hipStreamCreateWithPriority(&st2_, flags, lo));
  }
  // frames in flight: enqueue a frame and return; render_end() waits for it and reports its panics. A second handle can
  // render the next frame meanwhile - its camera rays fill the chip while this frame's last, latency-bound bounces drain.
  void render_bands_begin(int rank, int world, void* film_device) override {
    if (pending_) throw std::invalid_argument("render_bands_begin: the previous frame was not ended");
    gather_marked_ = false;
    defer_ = true;
    try { render_bands(rank, world, film_device, RRT_MEM_DEVICE, nullptr); } catch (...) { defer_ = false; throw; }
    defer_ = false;
    pending_ = true;
  }
  void render_end(rrt_render_stats* stats) override {
    if (!pending_) { if (stats) memset(stats, 0, sizeof(*stats)); return; }
    pending_ = false;
    std::unique_ptr<FrameRec> fr = std::move(frame_);
    HIP_CHECK(hipSetDevice(dev_));
    HIP_CHECK(hipStreamSynchronize(st_));
    HIP_CHECK(hipStreamSynchronize(st2_));
    check_device_errors();
    if (stats) { if (fr) frame_stats(*fr, stats); else memset(stats, 0, sizeof(*stats)); }
  }
  void check_device_errors() {
    uint32_t err = 0;
    HIP_CHECK(hipMemcpy(&err, counters_.p + C_ERROR, sizeof(err), hipMemcpyDeviceToHost));
    if (err & ERR_SHADING_NORMAL) throw PanicError("primitives.rs:66 assert!(dot3(&si.ist.n, &si.shading.n) >= 0.0) (vertex normals oppose the winding, Q14)");
    if (err & ERR_NO_LIGHTS) throw PanicError("directlighting.rs:91 unbounded recursion on a miss with an empty light list (Q20)");
    if (err & ERR_ST_DIMS) throw UnsupportedError("StratifiedSampler on the device: a sample drew more than 4095 1D or 2D dimensions (12-bit counters); very deep DirectLighting / Debug trees do");
    if (err & ERR_HALTON_DIMS) throw PanicError("samplers/halton.rs:65 HaltonSampler can only sample 1000 dimensions.");
    if (err & ERR_MIPMAP) throw PanicError("mipmap.rs:217 / memory.rs:84 index out of bounds in an ImageTexture lookup (EWA of the level past the last one: images with fewer than two pyramid levels, or a footprint >= the whole texture)");
    if (err & ERR_NULL_BSDF) throw PanicError("glass.rs:70 / translucent.rs:66 null BSDF (textures evaluate to black): path.rs:103 `bounces -= 1` underflows");
    if (err & ERR_BETA) throw PanicError("path.rs:146 assert!(beta.y() > 0.0 && beta.y().is_finite())");
    if (err & ERR_KIND_SET) throw DeviceError("internal: a material produced a BxDF outside the kind set its shading kernel was selected for (shade_spec())");
    if (err & ERR_NEAREST) throw DeviceError("internal: a rrt_nearest walk passed its step or stack bound (the tree is not the tree its depth and node count describe)");
    if (err & ERR_TRACE_ALL) throw DeviceError("internal: a rrt_trace_all walk passed its step or stack bound (the tree is not the tree its depth and node count describe)");
    if (err & ERR_VISIBILITY) throw DeviceError("internal: a rrt_visibility walk passed its step or stack bound (the tree is not the tree its depth and node count describe)");
  }
  void render_bands(int rank, int world, void* film_user, int film_mem, rrt_render_stats* stats) override {
    check_args("render_bands", kAnyTime, {}, Ranks{rank, world});
    const int32_t full[4] = {0, 0, desc_.film.xres, desc_.film.yres};
    render_impl(call_geom(full, kBandH, rank, world), film_user, film_mem, stats);
  }
  // ---- rrt_render_moments: the frame of render_rect / render_bands, and the sample-variance plane beside it ----------------------------------
  // render_impl in its moments mode: the passes of a frame with film_records off (per-slot layout), k_film_box_moments / k_film_wide_moments in
  // place of the film kernels, a second internal W x H x 4 running-sum buffer merged into the caller's plane by k_aov_merge (a plain +=).
  void render_moments(const int32_t rect[4], int rank, int world, void* film_user, void* moments_user, int mem, rrt_render_stats* stats) override {
    check_args("render_moments", kWhenIdle, {}, Ranks{rank, world}, rect);
    render_impl(call_geom(rect, bands_of(world), rank, world), film_user, mem, stats, moments_user);
  }
  // ---- rrt_render_frame_aov: the moments frame and the feature buffers of rrt_render_aov from one camera pass --------------------------------------------
  // Which scenes take which route. A frame whose passes begin with a queued closest-hit launch over the camera rays - the Path integrator, and
  // DirectLighting / Debug on scenes without transmissive or textured materials (the level loop of run_pass) - is fused: run_pass shades the first
  // hits from the bounce-0 queue (k_aov_shade_frame) and gathers them beside the moments film kernel (the gather skeletons over AovFrameAcc). A frame
  // that runs no such launch - the AO integrator, a Path integrator of depth 0, and DirectLighting / Debug on transmissive or textured scenes
  // (k_direct_tree: one thread per camera sample, no queue) - renders as a moments frame and render_aov's own pass follows it. Both routes add the
  // same bits.
  void render_frame_aov(const int32_t rect[4], int rank, int world, void* film_user, void* moments_user, int mem, uint64_t aov_max_samples, const rrt_aov* aov, rrt_render_stats* stats) override {
    check_args("render_frame_aov", kWhenIdle, Prec{"plane", aov->precision}, Ranks{rank, world}, rect);
    const int integ = desc_.integrator.type;
    const bool queued = (integ == RRT_INT_PATH && desc_.integrator.max_depth > 0) || ((integ == RRT_INT_DIRECT || integ == RRT_INT_DEBUG) && !(has_transmissive_ || tex_depth_ > 0));
    FrameAov fa{aov, queued ? frame_samples(aov_max_samples) : 0};
    render_impl(call_geom(rect, bands_of(world), rank, world), film_user, mem, stats, moments_user, &fa);
    if (!queued) render_aov(rect, rank, world, aov_max_samples, aov);
  }
  // ---- rrt_render_passes: the frame, and beside it the films of its next-event terms split by light group and path vertex --------------------------------
  // render_impl in its passes mode: the passes of a frame with film_records off (per-slot layout, as a moments frame), the PASSES instantiations of
  // k_shade_path, which store a pass mask beside every shadow record (Pools::smask, from the table folded here), add_pending adding an unoccluded record
  // to the radiance plane of every pass in its mask, and the frame's own film kernel run once more per plane into that pass's internal film.
  void render_passes(const int32_t rect[4], int rank, int world, const uint8_t* light_group, const rrt_pass* passes, int n_passes, void* film_user, int mem, rrt_render_stats* stats) override {
    const uint32_t nl = (uint32_t)desc_.n_lights;
    if (light_group) for (uint32_t i = 0; i < nl; i++)
      if (light_group[i] >= 32) throw std::invalid_argument("render_passes: light_group[" + std::to_string(i) + "] = " + std::to_string((int)light_group[i]) + ": a group is 0 .. 31");
    check_args("render_passes", kWhenIdle, {}, Ranks{rank, world}, rect);
    const rrt_film& f = desc_.film;
    if (desc_.integrator.type != RRT_INT_PATH)
      throw UnsupportedError("render_passes: the passes are the Path integrator's next-event terms; DirectLighting, AO and Debug frames have no passes");
    if (!std::isinf(f.max_sample_luminance))
      throw UnsupportedError("render_passes: a finite Film.max_sample_luminance clamps by the whole sample's luminance, so the passes would no longer add up to the frame");
    // the call's table folded per light and per vertex (Pools::pass_tab)
    const int depth = std::max(0, desc_.integrator.max_depth);
    pass_tab_host_.assign((size_t)nl + (size_t)depth, 0u);
    for (int k = 0; k < n_passes; k++) {
      for (uint32_t i = 0; i < nl; i++) {
        const uint32_t g = light_group ? light_group[i] : std::min(i, 31u);
        if ((passes[k].groups >> g) & 1u) pass_tab_host_[i] |= 1u << k;
      }
      for (int b = 0; b < depth; b++)
        if (b >= passes[k].bounce_lo && (passes[k].bounce_hi <= 0 || b < passes[k].bounce_hi)) pass_tab_host_[nl + (size_t)b] |= 1u << k;
    }
    const PassesReq pq{passes, n_passes};
    render_impl(call_geom(rect, bands_of(world), rank, world), film_user, mem, stats, nullptr, nullptr, &pq);
  }
  struct PassesReq { const rrt_pass* passes; int n; };
  // rrt_combine_passes: one kernel over the pixels; films in host memory are staged
  void combine_passes(const void* const* films, const double* gains_rgb, int n, void* film_out, int mem) override {
    HIP_CHECK(hipSetDevice(dev_));
    using V4 = typename Vec4T<R>::type;
    const size_t npix = (size_t)desc_.film.xres * (size_t)desc_.film.yres;
    CombineArgs a{};
    a.n = n;
    combine_to_rgb(a.to_rgb);
    for (int k = 0; k < n; k++) for (int c = 0; c < 3; c++) a.gains[k][c] = gains_rgb[3 * k + c];
    DevBuf<V4> stage;
    R* out = (R*)film_out;
    if (mem == RRT_MEM_DEVICE) for (int k = 0; k < n; k++) a.films[k] = films[k];
    else {
      stage.alloc((size_t)(n + 1) * npix);
      for (int k = 0; k < n; k++) {
        HIP_CHECK(hipMemcpyAsync(stage.p + (size_t)k * npix, films[k], npix * sizeof(V4), hipMemcpyHostToDevice, st_));
        a.films[k] = stage.p + (size_t)k * npix;
      }
      out = (R*)(stage.p + (size_t)n * npix);
    }
    hipLaunchKernelGGL((k_combine_passes<R>), dim3((uint32_t)((npix + kBlock - 1) / kBlock)), dim3(kBlock), 0, st_, a, out, npix);
    HIP_CHECK(hipGetLastError());
    if (mem != RRT_MEM_DEVICE) HIP_CHECK(hipMemcpyAsync(film_out, out, npix * sizeof(V4), hipMemcpyDeviceToHost, st_));
    HIP_CHECK(hipStreamSynchronize(st_));
  }
  // the feature buffers a frame was asked for: the caller's planes, and the leading samples that run_pass shades and gathers (0: none - the frame is
  // only held to its moments mode)
  struct FrameAov { const rrt_aov* out; uint64_t prefix; };
  // moments_user: the caller's sample-variance plane (same memory kind as the film) = the frame's moments mode; NULL = a plain frame, unless `fa` asks
  // for a moments-mode frame whose plane is not handed out
  void render_impl(const CallGeom& g, void* film_user, int film_mem, rrt_render_stats* stats, void* moments_user = nullptr, const FrameAov* fa = nullptr,
                   const PassesReq* pq = nullptr) {
    device_prologue();
    const rrt_film& f = desc_.film;
    if (g.rpix == 0) { if (stats) memset(stats, 0, sizeof(*stats)); return; }   // a rank that owns no band (world > yres / 16): nothing to add to the caller's film

    const bool with_moments = moments_user != nullptr || fa != nullptr;
    // run_pass, rect_passes and frame_setup work for a passes frame while passes_n_ > 0; the pools' passes members are null in every other frame
    struct PassesOff { Handle* h; ~PassesOff() { h->passes_n_ = 0; h->pool_.smask = nullptr; h->pool_.pass_L = nullptr; h->pool_.pass_stride = 0; h->pool_.pass_tab = nullptr; } } passes_off{this};
    passes_n_ = pq ? (uint32_t)pq->n : 0u;
    frame_setup(with_moments, g.rpix * (size_t)std::max<uint64_t>(g.s_total, 1));
    struct AovOff { Handle* h; ~AovOff() { h->aov_prefix_ = 0; } } aov_off{this};   // run_pass shades first hits for this frame only
    aov_prefix_ = fa ? fa->prefix : 0;
    if (aov_prefix_ > 0) {   // (setup, not the pass loop: frame_setup has sized the pools)
      const size_t plane_n = (size_t)f.xres * (size_t)f.yres * 4;
      if (aov_planes_.n != 3 * plane_n) aov_planes_.alloc(3 * plane_n);
      HIP_CHECK(hipMemsetAsync(aov_planes_.p, 0, 3 * plane_n * sizeof(R), st_));
      ensure_aov_recs();
    }
    auto fr = std::make_unique<FrameRec>();
    fr->camera_samples = (uint64_t)g.rpix * g.s_total;
    fr->begin(stats != nullptr || (defer_ && frame_stats_), st_);
    rect_passes(g, 0, g.s_total, with_moments, *fr);
    fr->end(st_);
    // merge into the caller's film (+=)
    const bool wait = !(film_mem == RRT_MEM_DEVICE && defer_) || pq != nullptr;
    if (pq) {   // each pass's internal film into its caller's film, as the frame's own below
      const size_t nfilm = (size_t)f.xres * (size_t)f.yres * 4;
      for (int k = 0; k < pq->n; k++) merge_film(pass_films_.p + (size_t)k * nfilm, pq->passes[k].film_xyzw, film_mem);
    }
    if (film_user || !pq) merge_out(film_user, moments_user, film_mem, wait);
    else HIP_CHECK(hipStreamSynchronize(st_));
    if (!wait) { frame_ = std::move(fr); return; }   // render_end() synchronises, checks the error flags and reads the statistics
    if (aov_prefix_ > 0) aov_merge_out(fa->out);
    check_device_errors();
    if (stats) frame_stats(*fr, stats);
  }
  // internal full-frame film (zeroed; merged into the caller's buffer at the end), the moments buffer beside it in a moments frame, the statistics'
  // totals, and pools for `want` slots or what max_paths allows
  void frame_setup(bool with_moments, size_t want, bool tile_trees = true) {
    const size_t W = (size_t)desc_.film.xres, H = (size_t)desc_.film.yres;
    if (film_.n != W * H * 4) film_.alloc(W * H * 4);
    HIP_CHECK(hipMemsetAsync(film_.p, 0, W * H * 4 * sizeof(R), st_));
    if (with_moments) {
      if (moments_.n != W * H * 4) moments_.alloc(W * H * 4);
      HIP_CHECK(hipMemsetAsync(moments_.p, 0, W * H * 4 * sizeof(R), st_));
    }
    if (totals_.n == 0) totals_.alloc(12);
    HIP_CHECK(hipMemsetAsync(totals_.p, 0, 12 * sizeof(unsigned long long), st_));
    HIP_CHECK(hipMemsetAsync(counters_.p, 0, C_COUNT * sizeof(uint32_t), st_));

    const size_t P = pool_slots(want);
    ensure_pools(P);
    if (passes_n_ > 0) passes_setup(P);
    if constexpr (std::is_same<R, float>::value) {
      if (tile_trees && tt_state_ == 0 && tile_trees_on_) {
        build_tile_trees();
        HIP_CHECK(hipMemsetAsync(counters_.p, 0, C_COUNT * sizeof(uint32_t), st_));   // the census ran the camera kernels
      }
    }
  }
  // the slots a pass of a call that wants `want` of them may hold
  size_t pool_slots(size_t want) {
    size_t P = std::min(max_paths_, std::max<size_t>(want, 64));
    if ((desc_.integrator.type == RRT_INT_DIRECT || desc_.integrator.type == RRT_INT_DEBUG) && (has_transmissive_ || tex_depth_ > 0) && desc_.integrator.max_depth > kTreeMax) {
      // k_direct_tree keeps (max_depth - kTreeMax) overflow frames per slot of a pass: a quarter of the free memory at most
      size_t free_b = 0, total_b = 0;
      HIP_CHECK(hipMemGetInfo(&free_b, &total_b));
      const size_t per_slot = (size_t)(desc_.integrator.max_depth - kTreeMax) * sizeof(TreeFrame<R>);
      P = std::max<size_t>(64, std::min(P, (free_b / 4) / per_slot));
    }
    return P;
  }
  // rrt_render_passes: the passes' internal films (zeroed), the table, one radiance plane per pass and a mask array per shadow queue. The planes come
  // after the pools: a pool pass of such a frame holds at most pass_cap_ slots - what the pools hold, or what half of the memory still free lets the
  // planes hold.
  void passes_setup(size_t want) {
    using V4 = typename Vec4T<R>::type;
    const size_t nfilm = (size_t)desc_.film.xres * (size_t)desc_.film.yres * 4;
    if (pass_films_.n < passes_n_ * nfilm) pass_films_.alloc(passes_n_ * nfilm);
    HIP_CHECK(hipMemsetAsync(pass_films_.p, 0, passes_n_ * nfilm * sizeof(R), st_));
    if (pass_tab_.n < pass_tab_host_.size()) { HIP_CHECK(hipStreamSynchronize(st_)); pass_tab_.alloc(pass_tab_host_.size()); }
    if (!pass_tab_host_.empty()) HIP_CHECK(hipMemcpyAsync(pass_tab_.p, pass_tab_host_.data(), pass_tab_host_.size() * sizeof(uint32_t), hipMemcpyHostToDevice, st_));
    size_t P = std::min(cap_, std::max<size_t>(want, 64));
    if (pass_planes_.n < passes_n_ * P || pass_smask_[0].n < P) {
      HIP_CHECK(hipStreamSynchronize(st_));
      pass_planes_.release(); pass_smask_[0].release(); pass_smask_[1].release();
      size_t free_b = 0, total_b = 0;
      HIP_CHECK(hipMemGetInfo(&free_b, &total_b));
      P = std::max<size_t>(64, std::min(P, (free_b / 2) / (passes_n_ * sizeof(V4) + 2 * sizeof(uint32_t))));
      pass_planes_.alloc(passes_n_ * P);
      pass_smask_[0].alloc(P); pass_smask_[1].alloc(P);
    }
    pass_cap_ = P;
    pool_.pass_L = pass_planes_.p; pool_.pass_stride = P; pool_.pass_tab = pass_tab_.p; pool_.smask = pass_smask_[0].p;
  }
  // the passes of sample numbers 1 + s_lo .. s_hi of a call's pixels: pixel groups and sample chunks from what the pools hold
  void rect_passes(const CallGeom& g, uint64_t s_lo, uint64_t s_hi, bool with_moments, FrameRec& fr) {
    for_each_pass(g, s_lo, s_hi, passes_n_ > 0 ? pass_cap_ : cap_, [&](const PassDesc& pd) { run_pass(pd, nullptr, g, with_moments, fr); });
  }
  // The cutter: sample numbers 1 + s_lo .. s_hi of n_units units of unit_px pixels each (1: the call's pixels; kTileW * kTileH: the tiles of a
  // list) as passes of at most cap slots - unit groups outermost, sample chunks inside. fn(pixel offset, pixels, s_begin, samples) makes the PassDesc.
  template <class F>
  static void cut_passes(size_t n_units, size_t unit_px, uint64_t s_lo, uint64_t s_hi, size_t cap, F&& fn) {
    if (n_units == 0 || s_hi <= s_lo) return;
    const size_t group = std::max<size_t>(1, std::min(n_units, cap / unit_px));          // units per group
    const uint64_t s_chunk = std::max<uint64_t>(1, cap / (group * unit_px));             // samples per pass
    for (size_t u0 = 0; u0 < n_units; u0 += group) {
      const size_t nu = std::min(group, n_units - u0);
      for (uint64_t sb = s_lo; sb < s_hi; sb += s_chunk)
        fn((uint32_t)(u0 * unit_px), (uint32_t)(nu * unit_px), (uint32_t)(1 + sb), (uint32_t)std::min<uint64_t>(s_chunk, s_hi - sb));
    }
  }
  // the passes of a call's own pixel grid, in tile order (PassDesc::tiled) where the rect allows it: whole kTileW x kTileH tiles
  template <class F>
  void for_each_pass(const CallGeom& g, uint64_t s_lo, uint64_t s_hi, size_t cap, F&& fn) {
    const uint32_t tiled = (tile_order_ && g.rw % kTileW == 0 && g.rh % kTileH == 0) ? 1u : 0u;
    cut_passes(g.rpix, 1, s_lo, s_hi, cap, [&](uint32_t p0, uint32_t npix, uint32_t s_begin, uint32_t ns) {
      fn(PassDesc{g.rect[0], g.rect[1], (int32_t)g.rw, p0, npix, s_begin, ns, g.band_h, g.n_ranks, g.rank, tiled});
    });
  }
  // HIP events around a launch of a frame whose statistics are wanted (FrameRec::timing), under the category frame_stats() adds it to
  size_t tick(FrameRec& fr, int cat, hipStream_t stream = nullptr) {
    if (!fr.timing) return (size_t)0;
    const hipEvent_t a = fr.make(), b = fr.make();
    HIP_CHECK(hipEventRecord(a, stream ? stream : st_));
    fr.evs.push_back({cat, {a, b}});
    return fr.evs.size() - 1;
  }
  void tock(FrameRec& fr, size_t id, hipStream_t stream = nullptr) { if (fr.timing) HIP_CHECK(hipEventRecord(fr.evs[id].second.second, stream ? stream : st_)); }
  // one pass: camera kernels, the integrator's launches, the film kernel. list: the tiles of a listed pass (list_pixel; box filter of radius 0.5 and
  // moments only, no tile trees, no film records), NULL for a pass over the rect's own pixel grid. The three parts meet in pool state only (q_active,
  // counters[C_ACTIVE], ray_o / ray_d, path, L, weight, samp, rdx_*): rrt_radiance and rrt_render_rays put k_ingest_rays in place of the first part.
  void run_pass(const PassDesc& pd, const uint32_t* list, const CallGeom& g, bool with_moments, FrameRec& fr) {
    // rrt_render_frame_aov: the leading samples of this pass that the feature buffers take (a pass that begins beyond the prefix: none)
    const uint64_t s_off = (uint64_t)pd.s_begin - 1;
    const uint32_t aov_ns = (!list && aov_prefix_ > s_off) ? (uint32_t)std::min<uint64_t>(pd.ns, aov_prefix_ - s_off) : 0u;
    pass_camera(pd, list, with_moments, fr);
    pass_integrate(pd, aov_ns, fr);
    pass_film(pd, list, g, with_moments, aov_ns, fr);
  }
  // first part: the camera kernels fill the pools
  void pass_camera(const PassDesc& pd, const uint32_t* list, bool with_moments, FrameRec& fr) {
    const size_t nslots = (size_t)pd.npix * pd.ns;
    const uint32_t grid = (uint32_t)((nslots + kBlock - 1) / kBlock);
    hipLaunchKernelGGL(k_rotate, dim3(1), dim3(1), 0, st_, counters_.p, 2);
    const size_t e = tick(fr, 0);
    launch_raygen(pd, grid, nullptr, desc_.integrator.type != RRT_INT_AO ? 1 : 0, true, /*film_records=*/!with_moments && passes_n_ == 0, list);
    // rrt_render_passes: this pool pass's slots of every plane start at 0, as raygen starts L (on the main stream: the shadow stream waits for shading)
    for (uint32_t k = 0; k < passes_n_; k++) HIP_CHECK(hipMemsetAsync(pool_.pass_L + (size_t)k * pool_.pass_stride, 0, nslots * sizeof(typename Vec4T<R>::type), st_));
    tock(fr, e);
  }
  // One closest-hit round of an integrator over the active queue. first: the queue is the one the camera kernels of this pass filled (tile trees
  // where the pass has them; the first hits that rrt_render_frame_aov keeps)
  void closest_step(const PassDesc& pd, uint32_t aov_ns, uint32_t grid, bool first, FrameRec& fr) {
    hipLaunchKernelGGL(k_accumulate_counts, dim3(1), dim3(1), 0, st_, counters_.p, totals_.p);
    const size_t e = tick(fr, 1);
    launch_closest(nullptr, &counters_.p[C_ACTIVE], 0, count_traversal_, nullptr, nullptr, count_traversal_ ? totals_.p : nullptr, grid, first);
    tock(fr, e); fr.n_closest_launch++;
    if (first && tt_pass_ok_ && !count_traversal_ && use_persistent()) fr.n_tile_launch++;
    if (first && aov_ns > 0) launch_aov_shade_frame(pd, aov_ns, grid);
  }
  // the shadow rays of the queue that shading has just filled, on `stream`
  void shadow_step(uint32_t grid, hipStream_t stream, FrameRec& fr) {
    hipLaunchKernelGGL(k_accumulate_shadow, dim3(1), dim3(1), 0, stream, pool_.shadow_count, totals_.p);
    const size_t e = tick(fr, 2, stream);
    launch_any(grid, stream);
    tock(fr, e, stream); fr.n_any_launch++; if (use_shadow_lists()) fr.n_list_launch++;
  }
  // second part: the integrator's launches over the queue the first part left, until every slot's L is final. aov_ns: see run_pass
  void pass_integrate(const PassDesc& pd, uint32_t aov_ns, FrameRec& fr) {
    const int integ = desc_.integrator.type;
    const int max_depth = desc_.integrator.max_depth;
    const size_t nslots = (size_t)pd.npix * pd.ns;
    const uint32_t grid = (uint32_t)((nslots + kBlock - 1) / kBlock);
    const uint32_t sgrid = (uint32_t)((nslots + ShadeBlock<R>::n - 1) / ShadeBlock<R>::n);
    size_t e = 0;
    hipLaunchKernelGGL(k_accumulate_camera, dim3(1), dim3(1), 0, st_, counters_.p, totals_.p, (integ == RRT_INT_PATH && max_depth <= 0) ? 0 : 1);
    if (integ == RRT_INT_PATH) {
      // bounce b: closest -> shade (NEE + BSDF sample + RR) -> shadow rays; paths live while bounces < max_depth
      const bool overlap = two_shadow_queues() && shadow_buf_[1][0] && !count_traversal_ && max_depth > 1;
      auto use_shadow_queue = [&](int k) {
        pool_.sray_o = shadow_buf_[k][0]; pool_.sray_d = shadow_buf_[k][1]; pool_.sld = shadow_buf_[k][2];
        pool_.shadow_count = counters_.p + (k ? C_SHADOW2 : C_SHADOW);
        if (passes_n_ > 0) pool_.smask = pass_smask_[k].p;
      };
      for (int b = 0; b < max_depth; b++) {
        closest_step(pd, aov_ns, grid, b == 0, fr);
        if (overlap) {
          use_shadow_queue(b & 1);
          if (b > 1) HIP_CHECK(hipStreamWaitEvent(st_, ev_shadow_[b & 1], 0));   // shading refills the queue the shadow launch of bounce b - 2 read
        }
        scene_.use_shadow_tabs = use_shadow_lists() ? 1u : 0u;
        scene_.horizon = (horizon_on_ && horizon_.n) ? horizon_.p : nullptr; scene_.hz_tau = horizon_tau_.p; scene_.hz_axis = hz_axis_;   // (counting frames too: the cull is geometry, not a kernel's arithmetic - their node counters then hold the rays that are traced)
        e = tick(fr, 3);
        if (passes_n_ > 0) launch_shade_path<true>(nslots, sgrid); else launch_shade_path<false>(nslots, sgrid);
        tock(fr, e);
        if (scene_.horizon) hipLaunchKernelGGL(k_accumulate_sky, dim3(1), dim3(1), 0, st_, counters_.p, totals_.p);
        if (overlap) {
          HIP_CHECK(hipEventRecord(ev_shade_, st_));
          HIP_CHECK(hipStreamWaitEvent(st2_, ev_shade_, 0));
          shadow_step(grid, st2_, fr);
          hipLaunchKernelGGL(k_rotate, dim3(1), dim3(1), 0, st2_, counters_.p, 6 + (b & 1));   // this shadow queue + the any-hit work counter
          HIP_CHECK(hipEventRecord(ev_shadow_[b & 1], st2_));
          swap_queues();
          hipLaunchKernelGGL(k_rotate, dim3(1), dim3(1), 0, st_, counters_.p, 5);    // active <- next, closest work counter
        } else {
          shadow_step(grid, st_, fr);
          swap_queues();
          hipLaunchKernelGGL(k_rotate, dim3(1), dim3(1), 0, st_, counters_.p, 0);
        }
      }
      if (overlap) {   // the film kernel reads L
        HIP_CHECK(hipStreamWaitEvent(st_, ev_shadow_[(max_depth - 1) & 1], 0));
        use_shadow_queue(0);
      }
    } else if (integ == RRT_INT_DIRECT || integ == RRT_INT_DEBUG) {
      if (has_transmissive_ || tex_depth_ > 0) {   // binary recursion with depth-first sampler dimensions / inherited ray differentials: one thread per camera sample
        e = tick(fr, 3);
        // frames below level kTreeMax of the per-sample recursion live in a strided global array, sized for this pass
        TreeFrame<R>* deep = nullptr;
        if (max_depth > kTreeMax) {
          const size_t need = (size_t)(max_depth - kTreeMax) * nslots;
          if (tree_deep_.n < need) { HIP_CHECK(hipStreamSynchronize(st_)); tree_deep_.alloc(need); }
          deep = tree_deep_.p;
        }
        with_flag(tex_depth_ > 0, [&](auto TEX) { hipLaunchKernelGGL((k_direct_tree<R, TEX()>), dim3(grid), dim3(kBlock), 0, st_, scene_, pool_, totals_.p, deep, (uint32_t)nslots); });
        tock(fr, e);
      } else {
      const bool all = integ == RRT_INT_DEBUG || desc_.integrator.light_strategy == RRT_STRATEGY_ALL;
      // level k handles reference depth k+1; specular recursion while depth + 1 < max_depth
      for (int level = 0; level < std::max(1, max_depth - 1); level++) {
        closest_step(pd, aov_ns, grid, level == 0, fr);
        if (desc_.n_lights > 0) {
          const int nl = all ? (int)desc_.n_lights : 1;
          for (int j = 0; j < nl; j++) {
            hipLaunchKernelGGL(k_rotate, dim3(1), dim3(1), 0, st_, counters_.p, 1);
            scene_.use_shadow_tabs = use_shadow_lists() ? 1u : 0u;
            e = tick(fr, 3);
            hipLaunchKernelGGL((k_shade_nee<R>), dim3(sgrid), dim3(ShadeBlock<R>::n), 0, st_, scene_, pool_, all ? j : -1, j == 0 ? 1 : 0);
            tock(fr, e);
            shadow_step(grid, st_, fr);
          }
        }
        e = tick(fr, 3);
        hipLaunchKernelGGL((k_shade_specular<R>), dim3(sgrid), dim3(ShadeBlock<R>::n), 0, st_, scene_, pool_, (desc_.n_lights == 0 && integ == RRT_INT_DEBUG) ? 1 : 0);
        tock(fr, e);
        swap_queues();
        hipLaunchKernelGGL(k_rotate, dim3(1), dim3(1), 0, st_, counters_.p, 0);
      }
      }
    }
    HIP_CHECK(hipGetLastError());
  }
  // third part: the film kernel reads L, weight and samp by slot
  void pass_film(const PassDesc& pd, const uint32_t* list, const CallGeom& g, bool with_moments, uint32_t aov_ns, FrameRec& fr) {
    const rrt_film& f = desc_.film;
    const bool wide = wide_filter();
    const FilmWindow& win = g.win;
    const size_t npix = pd.npix;
    const uint64_t ns = pd.ns;
    const size_t e = tick(fr, 4);
    // rrt_render_passes: after the frame's own film (k = -1) the same kernel once per pass, with L pointing at the pass's radiance plane, into the
    // pass's internal film
    typename Vec4T<R>::type* const frame_L = pool_.L;
    for (int k = -1; k < (int)passes_n_; k++) {
      R* const film_dst = k < 0 ? film_.p : pass_films_.p + (size_t)k * ((size_t)f.xres * (size_t)f.yres * 4);
      if (k >= 0) pool_.L = pool_.pass_L + (size_t)k * pool_.pass_stride;
      if (!wide && film_runs_ok_) {   // the camera kernels of this pass wrote record runs (launch_raygen); never in a moments frame
        if constexpr (std::is_same<R, float>::value)
          hipLaunchKernelGGL(k_film_box_runs, dim3((uint32_t)((npix / 64 + kFrTiles - 1) / kFrTiles)), dim3(64 * kFrTiles), 0, st_, scene_, pool_, pd, film_dst, film_runs_.p, (uint32_t)(ns / 8));
      }
      else if (!wide) {
        const dim3 fg((uint32_t)((npix + kBlock - 1) / kBlock));
        if (list) hipLaunchKernelGGL((k_film_box_moments<R, true>), fg, dim3(kBlock), 0, st_, scene_, pool_, pd, list, film_dst, moments_.p);
        else if (with_moments) hipLaunchKernelGGL((k_film_box_moments<R, false>), fg, dim3(kBlock), 0, st_, scene_, pool_, pd, list, film_dst, moments_.p);
        else hipLaunchKernelGGL((k_film_box<R>), fg, dim3(kBlock), 0, st_, scene_, pool_, pd, film_dst);
      }
      else {
        const dim3 fg((uint32_t)((win.n() + kBlock - 1) / kBlock));
        if (with_moments) hipLaunchKernelGGL((k_film_wide_moments<R>), fg, dim3(kBlock), 0, st_, scene_, pool_, pd, film_dst, moments_.p, win);
        else hipLaunchKernelGGL((k_film_wide<R>), fg, dim3(kBlock), 0, st_, scene_, pool_, pd, film_dst, win);
      }
    }
    pool_.L = frame_L;
    tock(fr, e);
    if (aov_ns > 0) launch_aov_gather_frame(pd, aov_ns, win);
    HIP_CHECK(hipGetLastError());
  }
  // the path shading kernel the scene's materials select (shade_kinds_); PS: its rrt_render_passes instantiation
  template <bool PS>
  void launch_shade_path(size_t nslots, uint32_t sgrid) {
    if (tex_depth_ > 0) hipLaunchKernelGGL((k_shade_path<R, 4, true, kAllKinds, true, PS>), dim3(std::min((uint32_t)((nslots + 255) / 256), 16384u)), dim3(256), 0, st_, scene_, pool_);
    else if (has_translucent_) hipLaunchKernelGGL((k_shade_path<R, 4, false, kAllKinds, true, PS>), dim3(std::min((uint32_t)((nslots + 255) / 256), 16384u)), dim3(256), 0, st_, scene_, pool_);
    else if (shade_kinds_ == kKindsLambert) {
      constexpr uint32_t kB = (uint32_t)shade_path_block<R, kKindsLambert>();
      const dim3 g(std::min((uint32_t)((nslots + kB - 1) / kB), 16384u));
      if (area_lights_ || shade_kinds_ == kAllKinds) hipLaunchKernelGGL((k_shade_path<R, 2, false, kKindsLambert, true, PS>), g, dim3(kB), 0, st_, scene_, pool_);
      else hipLaunchKernelGGL((k_shade_path<R, 2, false, kKindsLambert, false, PS>), g, dim3(kB), 0, st_, scene_, pool_);
    }
    else if (shade_kinds_ == kKindsGlossy) {
      constexpr uint32_t kB = (uint32_t)shade_path_block<R, kKindsGlossy>();
      hipLaunchKernelGGL((k_shade_path<R, 2, false, kKindsGlossy, true, PS>), dim3(std::min((uint32_t)((nslots + kB - 1) / kB), 16384u)), dim3(kB), 0, st_, scene_, pool_);
    }
    else hipLaunchKernelGGL((k_shade_path<R, 2, false, kAllKinds, true, PS>), dim3(std::min(sgrid, 16384u)), dim3(ShadeBlock<R>::n), 0, st_, scene_, pool_);
  }
  // rrt_render_frame_aov, first half of a pass: the first hits of the queue the bounce-0 closest-hit launch has just answered, under a stamp that no
  // earlier pass has written into the record buffers. It reads the queue and writes its own records: the shadow stream is not involved.
  void launch_aov_shade_frame(const PassDesc& pd, uint32_t aov_ns, uint32_t grid) {
    if (aov_serial_ >= 0x7fffffffu) {   // the stamp's 31 bits are used up: start over on clean flag words
      HIP_CHECK(hipMemsetAsync(aov_rec_a_.p, 0, aov_rec_a_.n * sizeof(typename Vec4T<R>::type), st_));
      aov_serial_ = 0;
    }
    aov_serial_++;
    const uint32_t slot_end = aov_ns * pd.npix;
    const dim3 sg(std::min(grid, 16384u));
    with_flag(tex_depth_ > 0, [&](auto TEX) { hipLaunchKernelGGL((k_aov_shade_frame<R, TEX()>), sg, dim3(kBlock), 0, st_, scene_, pool_, aov_rec_a_.p, aov_rec_b_.p, aov_serial_, slot_end); });
  }
  // second half, beside the moments film kernel: the pass's PassDesc with ns cut to the feature buffers' samples, gathered into the internal planes
  void launch_aov_gather_frame(PassDesc pd, uint32_t aov_ns, const FilmWindow& w) {
    pd.ns = aov_ns;
    launch_gather(AovFrameAcc<R>{aov_acc(), aov_serial_}, pd, w);
  }
  // the accumulator of the first-hit calls (render_aov, render_aov_follow): the internal planes, the records k_aov_shade / k_aov_follow left
  AovAcc<R> aov_acc() const { return {aov_planes_.p, aov_rec_a_.p, aov_rec_b_.p}; }
  // One gather of a pass into a pixel state `acc` describes (dkernels.hpp, the gather skeletons): the box form over the pass's pixels under the
  // default box filter, the wide form over the window's otherwise. lds_bytes: the dynamic LDS the accumulator asks for.
  template <class Acc>
  void launch_gather(const Acc& acc, const PassDesc& pd, const FilmWindow& w, size_t lds_bytes = 0) {
    if (!wide_filter()) hipLaunchKernelGGL((k_gather_box<R, Acc>), dim3((uint32_t)((pd.npix + kBlock - 1) / kBlock)), dim3(kBlock), lds_bytes, st_, scene_, pool_, pd, acc);
    else hipLaunchKernelGGL((k_gather_wide<R, Acc>), dim3((uint32_t)((w.n() + kBlock - 1) / kBlock)), dim3(kBlock), lds_bytes, st_, scene_, pool_, pd, acc, w);
  }
  // the per-slot records of the first-hit shading kernels, sized like the pools; rec_a - the flag words - zeroed when allocated, so that a slot no
  // kernel has written yet carries no pass's stamp (k_aov_shade_frame)
  void ensure_aov_recs() {
    if (aov_rec_a_.n >= cap_) return;
    HIP_CHECK(hipStreamSynchronize(st_));
    aov_rec_a_.alloc(cap_); aov_rec_b_.alloc(cap_);
    HIP_CHECK(hipMemsetAsync(aov_rec_a_.p, 0, cap_ * sizeof(typename Vec4T<R>::type), st_));
  }
  // the internal feature planes added to the caller's non-NULL planes (+=)
  void aov_merge_out(const rrt_aov* out) {
    void* const user[3] = {out->albedo, out->normal, out->depth};
    merge_planes(aov_planes_.p, 3, user, out->mem);
  }
  // n internal W x H x 4 planes, one after the other, each added to the caller's plane of the same number where that is not NULL (+=)
  void merge_planes(const R* planes, int n, void* const* user, int mem) {
    const size_t plane_n = (size_t)desc_.film.xres * (size_t)desc_.film.yres * 4;
    if (mem == RRT_MEM_DEVICE) {
      for (int k = 0; k < n; k++)
        if (user[k]) hipLaunchKernelGGL((k_aov_merge<R>), dim3((uint32_t)((plane_n + kBlock - 1) / kBlock)), dim3(kBlock), 0, st_, planes + k * plane_n, (R*)user[k], plane_n);
      HIP_CHECK(hipGetLastError());
      HIP_CHECK(hipStreamSynchronize(st_));
    } else {
      for (int k = 0; k < n; k++)
        if (user[k]) add_to_host(planes + k * plane_n, (R*)user[k], plane_n);
    }
  }
  // a device plane added to a host array (+=): staged, one synchronisation of the stream
  void add_to_host(const R* dev, R* host, size_t n) {
    std::vector<R> tmp(n);
    HIP_CHECK(hipMemcpyAsync(tmp.data(), dev, n * sizeof(R), hipMemcpyDeviceToHost, st_));
    HIP_CHECK(hipStreamSynchronize(st_));
    for (size_t i = 0; i < n; i++) host[i] += tmp[i];
  }
  // one internal film (RGB sums + weight sum), converted to XYZ, added to a caller's film (+=): enqueued for device memory, done on return for host memory
  void merge_film(const R* src, void* film_user, int film_mem) {
    const size_t npx = (size_t)desc_.film.xres * (size_t)desc_.film.yres, nfilm = npx * 4;
    if (film_mem == RRT_MEM_DEVICE) {
      hipLaunchKernelGGL((k_film_add<R>), dim3((uint32_t)((npx + kBlock - 1) / kBlock)), dim3(kBlock), 0, st_, src, (R*)film_user, npx);
      return;
    }
    if (film_xyz_.n != nfilm) film_xyz_.alloc(nfilm);
    HIP_CHECK(hipMemsetAsync(film_xyz_.p, 0, nfilm * sizeof(R), st_));
    hipLaunchKernelGGL((k_film_add<R>), dim3((uint32_t)((npx + kBlock - 1) / kBlock)), dim3(kBlock), 0, st_, src, film_xyz_.p, npx);
    HIP_CHECK(hipGetLastError());
    add_to_host(film_xyz_.p, (R*)film_user, nfilm);
  }
  // the internal film, converted to XYZ, and the internal moments buffer (where moments_user is given) added to the caller's buffers (+=); wait = 0
  // (device memory only): enqueued, not waited for
  void merge_out(void* film_user, void* moments_user, int film_mem, bool wait) {
    const size_t W = (size_t)desc_.film.xres, H = (size_t)desc_.film.yres;
    const bool with_moments = moments_user != nullptr;
    const size_t nfilm = W * H * 4;
    merge_film(film_.p, film_user, film_mem);
    if (film_mem == RRT_MEM_DEVICE) {
      if (with_moments) hipLaunchKernelGGL((k_aov_merge<R>), dim3((uint32_t)((nfilm + kBlock - 1) / kBlock)), dim3(kBlock), 0, st_, (const R*)moments_.p, (R*)moments_user, nfilm);
      HIP_CHECK(hipGetLastError());
      if (!wait) return;
      HIP_CHECK(hipStreamSynchronize(st_));
    }
    else if (with_moments) add_to_host(moments_.p, (R*)moments_user, nfilm);
  }
  // ---- rrt_render_adaptive: a moments frame that stops sampling the 8 x 8 tiles whose error estimate fell below the threshold ------------------------------
  // Round 0 is the moments frame's own passes over the rect for sample numbers 1 .. k0 (tile trees and all). After each round k_tile_error measures the
  // active tiles from the internal moments buffer and k_tile_select writes the next round's tile list in ascending order and its length, which the host
  // reads (4 bytes: the one synchronisation of a round) to size the listed passes of the next sample numbers. The internal film and moments buffers are
  // zeroed once and run on across the rounds; a pixel's sums are added in sample order whatever the pass, so a tile that stopped at k holds the bits
  // of a k-sample frame.
  void render_adaptive(const int32_t rect[4], const rrt_adaptive_params* ap, void* film_user, void* moments_user, uint32_t* tile_samples_user, int mem, rrt_render_stats* stats) override {
    check_args("render_adaptive", kWhenIdle, {}, {}, rect);
    device_prologue();
    const rrt_film& f = desc_.film;
    if (desc_.sampler.type == RRT_SAMPLER_STRATIFIED)
      throw UnsupportedError("render_adaptive: StratifiedSampler (the first k samples of a stratified pixel are not a k-sample stratified pixel; use the HaltonSampler)");
    if (wide_filter())
      throw UnsupportedError("render_adaptive: pixel filters other than the box filter of radius 0.5 (a wider filter splats across tiles with different sample counts)");
    const CallGeom g = call_geom(rect, kNoBands, 0, 1, ap->max_samples);
    const uint64_t K = g.s_total, k0 = std::min<uint64_t>(ap->min_samples, K);
    const uint32_t tiles_x = (uint32_t)(g.rw / kTileW), n_tiles = tiles_x * (uint32_t)(g.rh / kTileH);
    const auto kind = mem == RRT_MEM_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
    if (ad_samples_.n < n_tiles) { ad_list_[0].alloc(n_tiles); ad_list_[1].alloc(n_tiles); ad_err_.alloc(n_tiles); ad_samples_.alloc(n_tiles); }
    if (ad_count_.n == 0) ad_count_.alloc(1);
    HIP_CHECK(hipMemsetAsync(ad_samples_.p, 0, n_tiles * sizeof(uint32_t), st_));
    frame_setup(true, g.rpix * (size_t)std::max<uint64_t>(K, 1));
    FrameRec fr;
    fr.begin(stats != nullptr, st_);
    rect_passes(g, 0, k0, true, fr);
    fr.camera_samples = (uint64_t)g.rpix * k0;
    const uint32_t* list_in = nullptr;   // (round 0 took every tile)
    uint32_t n_active = n_tiles;
    int cur = 0;
    for (uint64_t k = k0; K > 0;) {
      // (at k == K every tile stops whatever its error: k_tile_select does not read it)
      if (k < K) hipLaunchKernelGGL((k_tile_error<R>), dim3((n_active + kTeBlock / 64u - 1) / (kTeBlock / 64u)), dim3(kTeBlock), 0, st_, (const typename Vec4T<R>::type*)moments_.p, (uint32_t)f.xres, rect[0], rect[1],
                         tiles_x, list_in, n_active, ad_err_.p);
      hipLaunchKernelGGL(k_tile_select, dim3(1), dim3(kSelBlock), 0, st_, list_in, n_active, (const double*)ad_err_.p, ap->threshold, (uint32_t)k, k == K ? 1 : 0, ad_list_[cur].p, ad_count_.p, ad_samples_.p);
      HIP_CHECK(hipGetLastError());
      if (k == K) break;
      uint32_t n_next = 0;
      HIP_CHECK(hipMemcpyAsync(&n_next, ad_count_.p, sizeof(n_next), hipMemcpyDeviceToHost, st_));
      HIP_CHECK(hipStreamSynchronize(st_));
      if (n_next == 0) break;
      if (n_next > n_active) throw DeviceError("internal: k_tile_select kept more tiles than it was given");
      const uint64_t nb = std::min<uint64_t>(ap->batch, K - k);
      // listed passes: the list's tiles as the cutter's units, always in tile order
      cut_passes(n_next, kTileW * kTileH, k, k + nb, cap_, [&](uint32_t p0, uint32_t npix, uint32_t s_begin, uint32_t ns) {
        run_pass(PassDesc{rect[0], rect[1], (int32_t)g.rw, p0, npix, s_begin, ns, g.band_h, g.n_ranks, g.rank, 1u}, ad_list_[cur].p, g, true, fr);
      });
      fr.camera_samples += (uint64_t)n_next * (kTileW * kTileH) * nb;
      k += nb;
      list_in = ad_list_[cur].p; n_active = n_next; cur ^= 1;
    }
    fr.end(st_);
    if (tile_samples_user) HIP_CHECK(hipMemcpyAsync(tile_samples_user, ad_samples_.p, n_tiles * sizeof(uint32_t), kind, st_));
    merge_out(film_user, moments_user, mem, true);
    check_device_errors();
    if (stats) frame_stats(fr, stats);
  }
  // ---- rrt_tile_error: k_tile_error over every tile of the rect, on the caller's plane --------------------------------------------------------------------
  void tile_error(const void* moments, int mem, const int32_t rect[4], double* out) override {
    check_args("tile_error", kWhenIdle, {}, {}, rect);
    const rrt_film& f = desc_.film;
    HIP_CHECK(hipSetDevice(dev_));
    using V4 = typename Vec4T<R>::type;
    const size_t npix = (size_t)f.xres * (size_t)f.yres;
    const uint32_t tiles_x = (uint32_t)(rect[2] - rect[0]) / kTileW, n_tiles = tiles_x * ((uint32_t)(rect[3] - rect[1]) / kTileH);
    const V4* mom = (const V4*)moments;
    if (mem == RRT_MEM_HOST) {
      if (!dn_stage_m_.p || dn_stage_m_.n != npix) dn_stage_m_.alloc(npix);
      HIP_CHECK(hipMemcpyAsync(dn_stage_m_.p, moments, npix * sizeof(V4), hipMemcpyHostToDevice, st_));
      mom = dn_stage_m_.p;
    }
    if (te_out_.n < n_tiles) te_out_.alloc(n_tiles);
    hipLaunchKernelGGL((k_tile_error<R>), dim3((n_tiles + kTeBlock / 64u - 1) / (kTeBlock / 64u)), dim3(kTeBlock), 0, st_, mom, (uint32_t)f.xres, rect[0], rect[1], tiles_x, (const uint32_t*)nullptr, n_tiles, te_out_.p);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipMemcpyAsync(out, te_out_.p, n_tiles * sizeof(double), mem == RRT_MEM_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, st_));
    HIP_CHECK(hipStreamSynchronize(st_));
  }
  // ---- the first-hit calls: rrt_render_aov, rrt_render_aov_follow, rrt_render_mattes ---------------------------------------------------------------
  // Each traces the frame's camera samples once and keeps something of the surface they see instead of radiance. They share first_hit_passes:
  // the passes of a frame (for_each_pass: the same pixel groups and sample chunks from cap_), and per pass the camera kernels, the closest-hit
  // launch over the camera queue (tile trees where a frame has built them, never built here), the call's `shade` - what a slot keeps of its hit,
  // written into the call's per-slot records - and the call's `gather`, the film kernel in gather form over those records. Nothing of the frame's
  // state is kept changed: the internal film, the statistics' totals and the tile-tree state are not touched, and a RaygenStateGuard of the
  // call puts back what launch_raygen sets per pass. The caller sizes the pools and its records before.
  template <class Shade, class Gather>
  void first_hit_passes(const CallGeom& g, Shade&& shade, Gather&& gather) {
    for_each_pass(g, 0, g.s_total, cap_, [&](const PassDesc& pd) {
      const uint32_t grid = (uint32_t)(((size_t)pd.npix * pd.ns + kBlock - 1) / kBlock);
      hipLaunchKernelGGL(k_rotate, dim3(1), dim3(1), 0, st_, counters_.p, 2);
      launch_raygen(pd, grid, nullptr, 1, /*for_render=*/false);   // no root cull, no film records: every survivor is queued, weight[slot] is per slot
      launch_closest(nullptr, &counters_.p[C_ACTIVE], 0, false, nullptr, nullptr, nullptr, grid, /*camera_rays=*/true);
      shade(pd, grid);
      gather(pd);
      HIP_CHECK(hipGetLastError());
    });
  }
  // ---- feature buffers (rrt_render_aov) and feature buffers through mirrors and glass (rrt_render_aov_follow): albedo / normal / depth planes -------
  // One body: rrt_render_aov is rrt_render_aov_follow with max_follow = 0 under its own name. shade: k_aov_shade for the first hits' records, then
  // per level k_aov_follow, the queue rotation and a closest-hit launch over the device-side count of followed entries - no host read-back
  // between levels, launches sized by the pass like the path loop's; with max_follow = 0 the level loop ends before its first launch. gather:
  // the skeletons over AovAcc into the handle's internal planes, which aov_merge_out adds to the caller's. The guard also puts the queue halves back
  // that the levels swap.
  void render_aov(const int32_t rect[4], int rank, int world, uint64_t max_samples, const rrt_aov* out) override {
    aov_passes("render_aov", rect, rank, world, max_samples, 0, out);
  }
  void render_aov_follow(const int32_t rect[4], int rank, int world, uint64_t max_samples, uint32_t max_follow, const rrt_aov* out) override {
    aov_passes("render_aov_follow", rect, rank, world, max_samples, max_follow, out);
  }
  void aov_passes(const std::string& who, const int32_t rect[4], int rank, int world, uint64_t max_samples, uint32_t max_follow, const rrt_aov* out) {
    check_args(who, kWhenIdle, Prec{"plane", out->precision}, Ranks{rank, world}, rect);
    device_prologue();
    const size_t plane_n = (size_t)desc_.film.xres * (size_t)desc_.film.yres * 4;
    const CallGeom g = call_geom(rect, bands_of(world), rank, world, max_samples);
    if (g.rpix == 0 || g.s_total == 0) return;   // nothing to add to the caller's planes
    if (!has_specular_) max_follow = 0;   // no surface of the scene is followed: every chain ends on its first hit, and no level is launched to find that out
    RaygenStateGuard guard(this);

    if (aov_planes_.n != 3 * plane_n) aov_planes_.alloc(3 * plane_n);
    HIP_CHECK(hipMemsetAsync(aov_planes_.p, 0, 3 * plane_n * sizeof(R), st_));
    HIP_CHECK(hipMemsetAsync(counters_.p, 0, C_COUNT * sizeof(uint32_t), st_));
    ensure_pools(std::min(max_paths_, std::max<size_t>(g.rpix * (size_t)g.s_total, 64)));
    ensure_aov_recs();
    first_hit_passes(g,
      [&](const PassDesc&, uint32_t grid) {
        const dim3 sg(std::min(grid, 16384u));
        // level 0's records are k_aov_shade's own (see k_aov_follow)
        with_flag(tex_depth_ > 0, [&](auto TEX) { hipLaunchKernelGGL((k_aov_shade<R, TEX()>), sg, dim3(kBlock), 0, st_, scene_, pool_, aov_rec_a_.p, aov_rec_b_.p); });
        for (uint32_t k = 0; k <= max_follow; k++) {
          const int level0 = k == 0 ? 1 : 0, may_follow = k < max_follow ? 1 : 0;
          if (level0 && !may_follow) break;   // max_follow = 0: the first hits are the planes
          with_flag(tex_depth_ > 0, [&](auto TEX) { hipLaunchKernelGGL((k_aov_follow<R, TEX()>), sg, dim3(kBlock), 0, st_, scene_, pool_, aov_rec_a_.p, aov_rec_b_.p, level0, may_follow); });
          if (!may_follow) break;
          swap_queues(); guard.swapped = !guard.swapped;
          hipLaunchKernelGGL(k_rotate, dim3(1), dim3(1), 0, st_, counters_.p, 0);   // active <- next
          launch_closest(nullptr, &counters_.p[C_ACTIVE], 0, false, nullptr, nullptr, nullptr, grid, /*camera_rays=*/false);
        }
      },
      [&](const PassDesc& pd) { launch_gather(aov_acc(), pd, g.win); });
    aov_merge_out(out);   // into the caller's planes (+=)
    check_device_errors();
  }
  // ---- ambient occlusion and bent normals (rrt_render_ao): first_hit_passes with shade = the draw rounds, gather = the skeletons over AoAcc ----------
  // Round i of a pass handles draw i of every hit of the pass: k_ao_gen pushes one hemisphere ray per hit into the pool's shadow queue (never more
  // entries than the camera queue, so no queue exceeds the pool), the any-hit launch over that queue adds the free rays' records into the per-slot
  // accumulators (Pools::L points at them for the call). A slot occurs once per round and the rounds follow each other on the stream: the sums need
  // no atomics and their order is the draw order, whatever the pool size. The rays' t_max is inf: the AO instantiations of the any-hit kernels
  // (persistent, plain and deep), which also leave the per-triangle any-hit lists alone; shadow candidate lists are per light and are not taken.
  void ao_defaults(rrt_ao_params* p) const override {
    const bool ao = desc_.integrator.type == RRT_INT_AO;
    p->n_samples = ao ? desc_.integrator.n_samples : 64;
    p->cos_sample = ao ? (desc_.integrator.cos_sample ? 1 : 0) : 1;
  }
  void render_ao(const int32_t rect[4], int rank, int world, uint64_t max_samples, const rrt_ao_params* params, const rrt_ao* out) override {
    using V4 = typename Vec4T<R>::type;
    rrt_ao_params prm;
    if (params) prm = *params; else ao_defaults(&prm);
    if (prm.n_samples < 1 || prm.n_samples > 256) throw std::invalid_argument("render_ao: n_samples must be 1..256 (draw i reads sampler dimensions 5 + 2i and 6 + 2i, and the permutation tables end at 1000)");
    check_args("render_ao", kWhenIdle, Prec{"plane", out->precision}, Ranks{rank, world}, rect);
    // the StratifiedSampler's draws past `dimension` are the [-1, 1) generator (Q25): no scene means a hemisphere sample drawn from those
    if (desc_.sampler.type == RRT_SAMPLER_STRATIFIED) throw UnsupportedError("render_ao under the StratifiedSampler (its 2D draws past `dimension` are not in [0, 1))");
    device_prologue();
    const size_t plane_n = (size_t)desc_.film.xres * (size_t)desc_.film.yres * 4;
    const CallGeom g = call_geom(rect, bands_of(world), rank, world, max_samples);
    if (g.rpix == 0 || g.s_total == 0) return;   // nothing to add to the caller's planes
    RaygenStateGuard guard(this);
    // what the rounds borrow of the pool: L (the accumulators' place) and the first shadow queue, put back on every way out
    struct PoolGuard {
      Pools<R>& p; V4 *L, *so, *sd, *sld; uint32_t* sc;
      explicit PoolGuard(Pools<R>& pp) : p(pp), L(pp.L), so(pp.sray_o), sd(pp.sray_d), sld(pp.sld), sc(pp.shadow_count) {}
      ~PoolGuard() { p.L = L; p.sray_o = so; p.sray_d = sd; p.sld = sld; p.shadow_count = sc; }
    };

    if (ao_planes_.n != 2 * plane_n) ao_planes_.alloc(2 * plane_n);
    HIP_CHECK(hipMemsetAsync(ao_planes_.p, 0, 2 * plane_n * sizeof(R), st_));
    HIP_CHECK(hipMemsetAsync(counters_.p, 0, C_COUNT * sizeof(uint32_t), st_));
    ensure_pools(std::min(max_paths_, std::max<size_t>(g.rpix * (size_t)g.s_total, 64)));
    if (ao_acc_.n < cap_) { HIP_CHECK(hipStreamSynchronize(st_)); ao_acc_.alloc(cap_); }
    PoolGuard pool_guard(pool_);
    pool_.L = ao_acc_.p;
    pool_.sray_o = shadow_buf_[0][0]; pool_.sray_d = shadow_buf_[0][1]; pool_.sld = shadow_buf_[0][2];
    pool_.shadow_count = counters_.p + C_SHADOW;
    const uint32_t n_draws = (uint32_t)prm.n_samples;
    const int cos_sample = prm.cos_sample ? 1 : 0;
    first_hit_passes(g,
      [&](const PassDesc&, uint32_t grid) {
        for (uint32_t i = 0; i < n_draws; i++) {
          hipLaunchKernelGGL(k_rotate, dim3(1), dim3(1), 0, st_, counters_.p, 1);   // the shadow queue and the work cursors start at 0
          hipLaunchKernelGGL((k_ao_gen<R>), dim3(grid), dim3(kBlock), 0, st_, scene_, pool_, i, n_draws, cos_sample);
          launch_any(grid, st_, /*ao=*/true);
        }
      },
      [&](const PassDesc& pd) { launch_gather(AoAcc<R>{ao_planes_.p, ao_acc_.p}, pd, g.win); });
    void* const user[2] = {out->ao, out->bent};
    merge_planes(ao_planes_.p, 2, user, out->mem);   // into the caller's planes (+=)
    check_device_errors();
  }
  // ---- ID mattes (rrt_render_mattes): first_hit_passes with shade = k_matte_ids and gather = the skeletons over MatteAcc into a (id, coverage) table --
  // Per call: the ids of the entries of prim_order are built on the host and uploaded (they are the caller's, not the scene's: nothing of the scene
  // preparation knows them), the caller's table is copied into the internal slot-major one (k_matte_load; a host table is staged), the passes insert
  // into it, k_matte_rank sorts it out. Load, rank and the staging of a host table run over the whole W x H x K table whatever the rect - also for
  // a rank without rows or a call without samples, which runs no pass: a frame cut into n calls moves the table n times.
  void render_mattes(const int32_t rect[4], int rank, int world, uint64_t max_samples, const uint32_t* prim_id, size_t n_prim_id, const rrt_mattes* out) override {
    if (prim_id && n_prim_id != desc_.n_prims)
      throw std::invalid_argument("render_mattes: n_prim_id = " + std::to_string(n_prim_id) + ", the scene has " + std::to_string(desc_.n_prims) + " primitives (one id per entry of rrt_scene_desc.prims)");
    check_args("render_mattes", kWhenIdle, Prec{"table", out->precision}, Ranks{rank, world}, rect);
    device_prologue();
    const size_t NP = (size_t)desc_.film.xres * (size_t)desc_.film.yres;
    const uint32_t K = (uint32_t)out->n_slots;
    const CallGeom g = call_geom(rect, bands_of(world), rank, world, max_samples);
    using V4 = typename Vec4T<R>::type;
    RaygenStateGuard guard(this);

    // the id of every entry of prim_order
    const size_t n_ord = matte_order_.size();
    const std::vector<uint32_t>* id_host = &matte_mat_;
    if (prim_id) {
      matte_id_host_.resize(n_ord);
      for (size_t i = 0; i < n_ord; i++) matte_id_host_[i] = prim_id[matte_order_[i]];
      id_host = &matte_id_host_;
    }
    if (matte_id_dev_.n != n_ord) matte_id_dev_.alloc(n_ord);
    if (n_ord) HIP_CHECK(hipMemcpyAsync(matte_id_dev_.p, id_host->data(), n_ord * sizeof(uint32_t), hipMemcpyHostToDevice, st_));
    // the caller's table in
    if (matte_ids_.n != NP * K) { matte_ids_.alloc(NP * K); matte_cov_.alloc(NP * K); }
    if (matte_w_.n != NP) matte_w_.alloc(NP);
    const MatteTab<R> tab{matte_ids_.p, matte_cov_.p, matte_w_.p, K, NP};
    const bool host = out->mem == RRT_MEM_HOST;
    const uint32_t* user_ids = out->ids;
    const R* user_cov = (const R*)out->coverage;
    if (host) {
      if (matte_stage_ids_.n != NP * K) { matte_stage_ids_.alloc(NP * K); matte_stage_cov_.alloc(NP * K); }
      HIP_CHECK(hipMemcpyAsync(matte_stage_ids_.p, out->ids, NP * K * sizeof(uint32_t), hipMemcpyHostToDevice, st_));
      HIP_CHECK(hipMemcpyAsync(matte_stage_cov_.p, out->coverage, NP * K * sizeof(R), hipMemcpyHostToDevice, st_));
      user_ids = matte_stage_ids_.p; user_cov = matte_stage_cov_.p;
    }
    HIP_CHECK(hipMemcpyAsync(matte_w_.p, out->weight, NP * sizeof(V4), host ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice, st_));
    const uint32_t tab_grid = (uint32_t)((NP * K + kBlock - 1) / kBlock), pix_grid = (uint32_t)((NP + kBlock - 1) / kBlock);
    const size_t lds = matte_lds_bytes(K, sizeof(R));
    hipLaunchKernelGGL((k_matte_load<R>), dim3(tab_grid), dim3(kBlock), 0, st_, user_ids, user_cov, tab);
    HIP_CHECK(hipGetLastError());

    HIP_CHECK(hipMemsetAsync(counters_.p, 0, C_COUNT * sizeof(uint32_t), st_));   // also where no pass runs: check_device_errors below reads them
    if (g.rpix > 0 && g.s_total > 0) {
      ensure_pools(std::min(max_paths_, std::max<size_t>(g.rpix * (size_t)g.s_total, 64)));
      if (matte_rec_.n < cap_) { HIP_CHECK(hipStreamSynchronize(st_)); matte_rec_.alloc(cap_); }
      first_hit_passes(g,
        [&](const PassDesc&, uint32_t grid) {
          hipLaunchKernelGGL((k_matte_ids<R>), dim3(std::min(grid, 16384u)), dim3(kBlock), 0, st_, pool_, (const uint32_t*)matte_id_dev_.p, (uint32_t)n_ord, matte_rec_.p);
        },
        [&](const PassDesc& pd) { launch_gather(MatteAcc<R>{tab, matte_rec_.p}, pd, g.win, lds); });
    }
    // ranked, into the caller's table
    hipLaunchKernelGGL((k_matte_rank<R>), dim3(pix_grid), dim3(kBlock), lds, st_, tab, host ? matte_stage_ids_.p : out->ids, host ? matte_stage_cov_.p : (R*)out->coverage);
    HIP_CHECK(hipGetLastError());
    if (host) {
      HIP_CHECK(hipMemcpyAsync(out->ids, matte_stage_ids_.p, NP * K * sizeof(uint32_t), hipMemcpyDeviceToHost, st_));
      HIP_CHECK(hipMemcpyAsync(out->coverage, matte_stage_cov_.p, NP * K * sizeof(R), hipMemcpyDeviceToHost, st_));
    }
    HIP_CHECK(hipMemcpyAsync(out->weight, matte_w_.p, NP * sizeof(V4), host ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice, st_));
    HIP_CHECK(hipStreamSynchronize(st_));
    check_device_errors();
  }
  // rrt_matte_extract: one kernel over the pixels; a table in host memory is staged through the buffers render_mattes stages through
  void matte_extract(const rrt_mattes* m, const uint32_t* ids, int n_ids, void* alpha) override {
    check_args("matte_extract", kWhenIdle, Prec{"table", m->precision});
    HIP_CHECK(hipSetDevice(dev_));
    using V4 = typename Vec4T<R>::type;
    const size_t NP = (size_t)desc_.film.xres * (size_t)desc_.film.yres;
    const uint32_t K = (uint32_t)m->n_slots;
    if (NP == 0) return;
    std::vector<uint32_t> list(ids, ids + n_ids);
    std::sort(list.begin(), list.end());
    list.erase(std::unique(list.begin(), list.end()), list.end());
    if (matte_list_.n < list.size()) matte_list_.alloc(256);
    HIP_CHECK(hipMemcpyAsync(matte_list_.p, list.data(), list.size() * sizeof(uint32_t), hipMemcpyHostToDevice, st_));
    const bool host = m->mem == RRT_MEM_HOST;
    const uint32_t* t_ids = m->ids;
    const R* t_cov = (const R*)m->coverage;
    const V4* t_w = (const V4*)m->weight;
    R* out = (R*)alpha;
    if (host) {
      if (matte_stage_ids_.n != NP * K) { matte_stage_ids_.alloc(NP * K); matte_stage_cov_.alloc(NP * K); }
      if (matte_w_.n != NP) matte_w_.alloc(NP);
      if (matte_alpha_.n != NP) matte_alpha_.alloc(NP);
      HIP_CHECK(hipMemcpyAsync(matte_stage_ids_.p, m->ids, NP * K * sizeof(uint32_t), hipMemcpyHostToDevice, st_));
      HIP_CHECK(hipMemcpyAsync(matte_stage_cov_.p, m->coverage, NP * K * sizeof(R), hipMemcpyHostToDevice, st_));
      HIP_CHECK(hipMemcpyAsync(matte_w_.p, m->weight, NP * sizeof(V4), hipMemcpyHostToDevice, st_));
      t_ids = matte_stage_ids_.p; t_cov = matte_stage_cov_.p; t_w = matte_w_.p; out = matte_alpha_.p;
    }
    hipLaunchKernelGGL((k_matte_extract<R>), dim3((uint32_t)((NP + kBlock - 1) / kBlock)), dim3(kBlock), 0, st_, t_ids, t_cov, t_w, K, (const uint32_t*)matte_list_.p, (int)list.size(), out, NP);
    HIP_CHECK(hipGetLastError());
    if (host) HIP_CHECK(hipMemcpyAsync(alpha, matte_alpha_.p, NP * sizeof(R), hipMemcpyDeviceToHost, st_));
    HIP_CHECK(hipStreamSynchronize(st_));
  }
  // ---- rrt_denoise (device/dfilter.hpp): prepare, initial variance, one a-trous launch per iteration, finish ---------------------------------------------
  // Only the handle's stream and its own work buffers are used: nothing of the frame's state is read or written.
  template <int S>
  void launch_atrous(bool lds, dim3 grid, const typename Vec4T<R>::type* cin, typename Vec4T<R>::type* cout, const DnParams<R>& k) {
    const dim3 block(kDnBX, kDnBY);
    if constexpr (S <= 2) {   // the steps at which the LDS tile measured faster than the gathers (40 against 67 us per launch at 1024^2, fp32)
      if (lds) { hipLaunchKernelGGL((k_dn_atrous_lds<R, S>), grid, block, 0, st_, cin, cout, dn_g_.p, dn_p_.p, k); return; }
    }
    hipLaunchKernelGGL((k_dn_atrous<R, S>), grid, block, 0, st_, cin, cout, dn_g_.p, dn_p_.p, k);
  }
  void denoise(const void* film, const rrt_aov* aov, const void* moments, const rrt_denoise_params* p, void* film_out) override {
    check_args("denoise", kWhenIdle, Prec{"plane", aov->precision});
    HIP_CHECK(hipSetDevice(dev_));
    using V4 = typename Vec4T<R>::type;
    const size_t W = (size_t)desc_.film.xres, H = (size_t)desc_.film.yres, npix = W * H;
    if (npix == 0) return;
    if (!dn_p_.p || dn_p_.n != npix) { dn_c_[0].alloc(npix); dn_c_[1].alloc(npix); dn_g_.alloc(npix); dn_p_.alloc(npix); }   // dn_p_ last: set only when all four exist
    const V4* in[4] = {(const V4*)film, (const V4*)aov->albedo, (const V4*)aov->normal, (const V4*)aov->depth};
    V4* out = (V4*)film_out;
    const bool host = aov->mem == RRT_MEM_HOST;
    if (host) {   // staged: the four inputs, the output over the film's copy
      if (!dn_stage_.p || dn_stage_.n != 4 * npix) dn_stage_.alloc(4 * npix);
      const void* src[4] = {film, aov->albedo, aov->normal, aov->depth};
      for (int j = 0; j < 4; j++) {
        HIP_CHECK(hipMemcpyAsync(dn_stage_.p + j * npix, src[j], npix * sizeof(V4), hipMemcpyHostToDevice, st_));
        in[j] = dn_stage_.p + j * npix;
      }
      out = dn_stage_.p;
    }
    const V4* mom = (const V4*)moments;
    if (moments && host) {
      if (!dn_stage_m_.p || dn_stage_m_.n != npix) dn_stage_m_.alloc(npix);
      HIP_CHECK(hipMemcpyAsync(dn_stage_m_.p, moments, npix * sizeof(V4), hipMemcpyHostToDevice, st_));
      mom = dn_stage_m_.p;
    }
    const DnParams<R> k{(int)W, (int)H, (R)p->sigma_color, (R)p->sigma_normal, (R)p->sigma_depth};
    const uint32_t lin = (uint32_t)((npix + 255) / 256);
    const dim3 grid((uint32_t)((W + kDnBX - 1) / kDnBX), (uint32_t)((H + kDnBY - 1) / kDnBY)), block(kDnBX, kDnBY);
    hipLaunchKernelGGL((k_dn_prepare<R>), dim3(lin), dim3(256), 0, st_, in[0], in[1], in[2], in[3], dn_c_[0].p, dn_g_.p, dn_p_.p, npix, p->demodulate != 0 ? 1 : 0);
    hipLaunchKernelGGL((k_dn_moments<R>), grid, block, 0, st_, (const V4*)dn_c_[0].p, dn_c_[1].p, (const V4*)dn_g_.p, k);
    if (mom) hipLaunchKernelGGL((k_dn_sample_variance<R>), dim3(lin), dim3(256), 0, st_, mom, dn_c_[1].p, npix);   // rrt_denoise_moments
    int cur = 1;
    const bool lds = dn_lds_;
    for (int i = 0; i < p->iterations; i++, cur ^= 1) {
      const V4* cin = dn_c_[cur].p;
      V4* cout = dn_c_[cur ^ 1].p;
      switch (i) {
        case 0: launch_atrous<1>(lds, grid, cin, cout, k); break;
        case 1: launch_atrous<2>(lds, grid, cin, cout, k); break;
        case 2: launch_atrous<4>(lds, grid, cin, cout, k); break;
        case 3: launch_atrous<8>(lds, grid, cin, cout, k); break;
        case 4: launch_atrous<16>(lds, grid, cin, cout, k); break;
        default: launch_atrous<32>(lds, grid, cin, cout, k); break;
      }
    }
    hipLaunchKernelGGL((k_dn_finish<R>), dim3(lin), dim3(256), 0, st_, in[0], (const V4*)dn_c_[cur].p, (const V4*)dn_p_.p, out, npix);
    HIP_CHECK(hipGetLastError());
    if (host) HIP_CHECK(hipMemcpyAsync(film_out, dn_stage_.p, npix * sizeof(V4), hipMemcpyDeviceToHost, st_));
    HIP_CHECK(hipStreamSynchronize(st_));
  }
  void frame_stats(const FrameRec& fr, rrt_render_stats* stats) {
    unsigned long long ht[12];
    HIP_CHECK(hipMemcpy(ht, totals_.p, sizeof(ht), hipMemcpyDeviceToHost));
    memset(stats, 0, sizeof(*stats));
    stats->camera_samples = fr.camera_samples;
    stats->camera_rays = ht[4];
    stats->closest_queries = ht[2];
    stats->any_queries = ht[3];
    stats->nodes_visited = ht[0] + ht[5];
    stats->prims_tested = ht[1] + ht[6];
    stats->closest_nodes = ht[0]; stats->closest_prims = ht[1]; stats->any_nodes = ht[5]; stats->any_prims = ht[6];
    stats->closest_launches = fr.n_closest_launch;
    stats->any_launches = fr.n_any_launch;
    stats->tile_launches = fr.n_tile_launch;
    stats->list_launches = fr.n_list_launch;
    stats->root_culled = ht[7];
    stats->sky_culled = ht[8];
    stats->s_horizon_build = hz_build_s_;
    if (!fr.timing) return;
    float ms = 0;
    HIP_CHECK(hipEventElapsedTime(&ms, fr.ev_begin, fr.ev_end));
    stats->ms_total = ms;
    double cat[5] = {0, 0, 0, 0, 0};
    for (auto& ev : fr.evs) {
      HIP_CHECK(hipEventElapsedTime(&ms, ev.second.first, ev.second.second));
      cat[ev.first] += ms;
    }
    stats->ms_raygen = cat[0]; stats->ms_closest = cat[1]; stats->ms_any = cat[2]; stats->ms_shade = cat[3]; stats->ms_film = cat[4];
    if (gather_marked_) {   // the collective rrt_film_gather enqueued behind this frame (render_end has synchronised the stream)
      HIP_CHECK(hipEventElapsedTime(&ms, ev_gather_[0], ev_gather_[1]));
      stats->ms_gather = ms;
    }
  }

 private:
  int dev_;
  rrt_scene_desc desc_;   // shallow copy: scalar fields only are used after construction
  hipStream_t st_ = nullptr;
  // Path integrator: the shadow rays of bounce k are traced on st2_ beside the closest-hit launch of bounce k + 1 (they only
  // feed L[slot]); both launches end in a latency tail that leaves most of the chip idle, and the tails overlap this way.
  hipStream_t st2_ = nullptr;
  hipEvent_t ev_shade_ = nullptr, ev_shadow_[2] = {nullptr, nullptr};
  hipEvent_t ev_gather_[2] = {nullptr, nullptr};   // gather_mark()
  bool gather_marked_ = false;
  typename Vec4T<R>::type* shadow_buf_[2][3] = {{nullptr, nullptr, nullptr}, {nullptr, nullptr, nullptr}};
  bool overlap_shadow_ = true;
  bool defer_ = false, pending_ = false;   // render_bands_begin / render_end
  bool frame_stats_ = false;               // option "frame_stats": deferred frames record their kernel timings too (rrt_render_end_stats)
  std::unique_ptr<FrameRec> frame_;        // the frame in flight
  SceneDev<R> scene_{};
  Pools<R> pool_{};
  size_t cap_ = 0;
  size_t max_paths_ = (size_t)1 << 28;   // clamped to half of the free HBM at creation (sized for 288 GB parts)
  bool deep_ = false, count_traversal_ = false, persistent_ = true;
  bool pairs_ok_ = false;
  bool mixed_ = false;   // the tree has kSpecialLeaf leaves (spheres, kept instances): the MIXED instantiations of the pair-node kernels
  int n_cus_ = 0;           // compute units of dev_ (resident_grid)
  uint32_t trav_grid_ = 0, pt_grid_ = 0, pt_grid_quad_ = 0;
  int rg_spb_ = 8;          // option "rg_spb": samples per workgroup of the dense camera kernel (the workgroup's 512 threads = 512 / spb pixels x spb samples)
  bool tile_order_ = true;  // option "tile_order": pixels of a pass enumerated tile by tile (PassDesc::tiled)
  bool raygen_lean_ = true;   // option "raygen_lean"
  bool has_transmissive_ = false, has_translucent_ = false;
  bool has_specular_ = false;   // a Mirror or Glass primitive exists (render_aov_follow runs no level beyond the first hits otherwise)
  bool area_lights_ = true;   // some light is a DiffuseAreaLight (else the Lambert shading kernel drops the area-light code)
  uint32_t shade_kinds_scene_ = kAllKinds, shade_kinds_ = kAllKinds;   // lobe-kind set of the scene's materials / of the shading kernel in use (option "shade_spec")
  int trav_mode_ = 3;   // 1 = LDS-treelet grid-stride kernel, 2 = persistent-thread kernel, 3 = by queue size
  uint32_t pt_split_closest_ = 100000u, pt_split_any_ = 100000u;   // re-tuned with the shadow launches overlapped (tools/band_scaling.py)
  DevBuf<uint32_t> pt_overflow_, pt_overflow_any_;
  DevBuf<uint32_t> any_list_;              // TravScene::any_list, 8 words per triangle
  DevBuf<uint32_t> sl_headers_, sl_entries_;   // shadow candidate lists (build_shadow_lists())
  DevBuf<LeafRec> sl_leaves_;
  ShadowLists sl_dev_{};
  int sl_grid_cap_ = 32768;  // option "sl_grid" (measured: 2 048 / 8 192 / 32 768 workgroups: any-hit alone 4.27 / 3.46 / 3.38 ms)
  bool shadow_lists_ok_ = false, shadow_lists_on_ = true;   // built for this scene / option "shadow_lists"
  bool any_entry_on_ = true;
  // tile trees (dtraverse_f32.hpp k_trace_tiles_f32): per 32 x 32-pixel patch of the image, a local copy of the pair nodes its camera rays visit most
  bool tile_trees_on_ = true;              // option "tile_trees"
  bool root_cull_on_ = true;               // option "root_cull": the camera kernels answer camera rays that miss the root box (SceneDev::root_cull)
  int tt_census_spp_ = 2;                  // option "tt_census": camera samples per pixel of the census
  int tt_state_ = 0;                       // 0 = not built yet, 1 = built, -1 = not for this scene
  std::vector<PairNode> pairs_host_;       // the kernels' tree (build_pairs()), fetched back for the census walk
  std::vector<Tri<float>> tris_host_;
  DevBuf<PairNode> tt_pairs_;              // kTtLocalBytes unused bytes, then the whole tree with its interior child words shifted by kTtLocalBytes
  DevBuf<PairNode> tt_trees_;              // [patches + 1][kTtNodes]
  DevBuf<uint2> tt_chunks_;
  DevBuf<float4> tt_tris_;                 // [patches + 1][kTtTris][3] (RRT_TT_TRIS > 0 builds)
  DevBuf<uint32_t> tt_overflow_;
  uint32_t tt_grid_ = 0, tt_mt_x_ = 0, tt_n_trees_ = 0;
  TileTrees tt_pass_{};                    // this pass
  bool tt_pass_ok_ = false;
  DevBuf<uint32_t> pix_off_;
  TravScene trav_{};
  DevBuf<PairNode> pairs_;
  DevBuf<float> horizon_tau_;              // HzTables::tau
  DevBuf<uint8_t> horizon_;                // horizon tables (host/horizon_build.cpp): 32 bytes per triangle; empty = not built for this scene
  uint32_t hz_axis_ = 1u;
  bool horizon_on_ = true;                 // option "horizon_cull"
  double hz_build_s_ = 0.0;                // host seconds this handle spent building the tables when it was created (0: found in the process cache, or none built)
  DevBuf<QuadNode> quads_;                 // two levels per fetch (dtraverse_f32.hpp "quad nodes"); empty = not built for this scene
  bool quad_on_ = false;                   // option "quad_nodes"
  DevBuf<uint32_t> overflow_, overflow_any_;
  DevBuf<Node<R>> nodes_;
  DevBuf<Tri<R>> tris_;
  DevBuf<TriShade<R>> shades_;
  DevBuf<SphereDev<R>> spheres_;
  DevBuf<InstDev<R>> insts_;
  DevBuf<Material<R>> materials_;
  DevBuf<TexDev<R>> textures_;
  DevBuf<ImageDev<R>> images_;
  DevBuf<R> image_texels_;
  int tex_depth_ = 0;          // deepest texture graph some primitive's material evaluates (0 = no textured material in use)
  DevBuf<Light<R>> lights_;
  DevBuf<R> light_cdf_;
  DevBuf<LensElem<R>> lens_;
  DevBuf<float> lens_safe_;   // calibrate_aux_margins(): per interface, the squared radius inside which an auxiliary ray cannot be blocked (fp32 camera kernels)
  bool aux_margin_ = true;
  float aux_delta_ = 0.0f, aux_pupil_ = 0.0f;
  DevBuf<uint32_t> lens_cull_;   // build_lens_cull(): the lens cull table of the fp32 camera kernel (empty: no table)
  float lc_inv_dr_ = 0.0f;
  bool lens_cull_on_ = true;    // option "lens_cull"
  DevBuf<uint2> film_runs_;      // per camera workgroup of a pass with film records: {first record, records} (k_raygen_main_f32, k_film_box_runs)
  bool film_records_on_ = true;  // option "film_records"
  bool film_runs_ok_ = false;    // the pass the camera kernels last ran for writes film records
  DevBuf<R> filter_table_;
  DevBuf<HaltonDim> hdims_;
  static constexpr int kHaltonTabDims = 64;
  DevBuf<HaltonBlk> hblk_;                 // SceneDev::hblk / hlo / hhi
  DevBuf<uint32_t> hlo_;
  DevBuf<uint4> hhi_;
  DevBuf<uint32_t> cam_lo_;                // SceneDev::cam_lo / cam_hi
  DevBuf<uint4> cam_hi_;
  bool cam_tables_on_ = true;
  size_t cam_lo_off_[3] = {0, 0, 0}, cam_hi_off_[3] = {0, 0, 0};
  DevBuf<uint16_t> perms_;
  DevBuf<typename Vec4T<R>::type> vpool_;
  DevBuf<R> rpool_;
  DevBuf<uint32_t> upool_, counters_, deep_stack_;
  DevBuf<TreeFrame<R>> tree_deep_;   // k_direct_tree: frames of recursion levels past kTreeMax, [level][slot of the pass]
  DevBuf<unsigned long long> totals_;
  DevBuf<R> film_;       // per pixel: running RGB contribution sum + filter weight sum of the frame being rendered
  DevBuf<R> film_xyz_;   // the same merged to XYZ, staging for a host film
  DevBuf<R> moments_;    // render_moments: per pixel running {S1, S2, S0, S3} of the frame being rendered (allocated by the first call)
  DevBuf<uint32_t> ad_list_[2], ad_count_, ad_samples_;   // render_adaptive: the tile lists of this round and the next, the next round's length, the tiles' sample counts
  DevBuf<double> ad_err_, te_out_;                        // k_tile_error's output per tile: of render_adaptive's rounds / of tile_error (allocated by the first call)
  DevBuf<R> aov_planes_;   // render_aov: running sums of the albedo, normal and depth planes, W x H x 4 each (allocated by the first call)
  DevBuf<typename Vec4T<R>::type> dn_c_[2], dn_g_, dn_p_, dn_stage_;   // denoise: the record planes C (ping-pong), G, P of dfilter.hpp, and the staging of host-memory calls (allocated by the first call)
  DevBuf<typename Vec4T<R>::type> dn_stage_m_;   // denoise with a moments plane in host memory: its staging
  bool dn_lds_ = true;       // option "dn_lds"
  DevBuf<R> ao_planes_;    // render_ao: running sums of the occlusion and bent-normal planes, W x H x 4 each (allocated by the first call)
  DevBuf<typename Vec4T<R>::type> ao_acc_;   // render_ao: per-slot accumulators {b.xyz, a} of a pass's draws, sized like pool.L (allocated by the first call)
  DevBuf<typename Vec4T<R>::type> aov_rec_a_, aov_rec_b_;   // k_aov_shade's per-slot records {rho.rgb, hit flag}, {n.xyz, t}: sized like pool.L
  // render_passes (all allocated by the first call): the passes' internal films, the folded pass table (Pools::pass_tab) and its host copy, the radiance
  // planes, the mask arrays of the two shadow queues; passes_n_ = the passes of the frame being rendered, 0 outside such a frame
  DevBuf<R> pass_films_;
  DevBuf<uint32_t> pass_tab_, pass_smask_[2];
  std::vector<uint32_t> pass_tab_host_;
  DevBuf<typename Vec4T<R>::type> pass_planes_;
  size_t pass_cap_ = 0;
  uint32_t passes_n_ = 0;
  uint64_t aov_prefix_ = 0;   // render_frame_aov: the leading samples whose first hits run_pass shades and gathers; 0 outside such a frame
  // render_mattes (all allocated by the first call): the internal slot-major table and weight records, k_matte_ids' per-slot records (sized like
  // pool.L), the per-call id of every entry of prim_order, the staging of a host-memory table, matte_extract's sorted id list and staged output
  DevBuf<uint32_t> matte_ids_, matte_id_dev_, matte_stage_ids_, matte_list_;
  DevBuf<R> matte_cov_, matte_stage_cov_, matte_alpha_;
  DevBuf<typename Vec4T<R>::type> matte_w_;
  DevBuf<uint2> matte_rec_;
  std::vector<uint32_t> matte_order_, matte_mat_, matte_id_host_;
  std::vector<uint8_t> surf_sphere_;   // per entry of prim_order: 1 = a sphere
  // rrt_nearest: the absolute part of the prune margin (host/nearest.hpp: kNearestPadUlps x eps x M), whether any entry is a triangle, the stack
  // arrays of the two kernels (kept between calls, grown on demand), the fp32 kernel choice (option "nearest_pairs")
  R nn_delta_ = R(0);
  bool nn_has_tri_ = false, nn_pairs_on_ = false;
  DevBuf<uint32_t> nn_stack_;
  // rrt_trace_all: the pad of the node boxes (host/multihit.hpp: kMultihitPadUlps x eps x M where the scene has a kept instance, else 0) and the deep stack
  R mh_delta_ = R(0);
  DevBuf<uint32_t> mh_stack_;
  DevBuf<uint2> nn_overflow_;
  uint32_t aov_serial_ = 0;   // k_aov_shade_frame's stamp of the pass last shaded: counted up per pass over the handle's life, never 0 in a record

  void check_renderable() {
    if (tex_depth_ > kTexDepth) throw UnsupportedError("texture graphs deeper than " + std::to_string(kTexDepth) + " levels");
    if (tex_depth_ > 0 && (desc_.integrator.type == RRT_INT_DIRECT || desc_.integrator.type == RRT_INT_DEBUG)) {
      // specular children inherit ray differentials (integrator/mod.rs:183-201, 238-292): the per-sample recursion kernel carries them
      if (deep_) throw UnsupportedError("DirectLighting / Debug with textured materials on a BVH deeper than 64");
    }
    if (has_transmissive_ && (desc_.integrator.type == RRT_INT_DIRECT || desc_.integrator.type == RRT_INT_DEBUG)) {
      if (deep_) throw UnsupportedError("DirectLighting / Debug with transmissive materials on a BVH deeper than 64");
    }
    if (desc_.sampler.type == RRT_SAMPLER_STRATIFIED) {
      // index word = pixel << 10 | sample number; 12-bit 1D / 2D dimension counters (<= 3 of each per bounce; deep DirectLighting / Debug trees draw more: checked on the device)
      if (desc_.sampler.samples_per_pixel > 1024 || (uint64_t)desc_.film.xres * (uint64_t)desc_.film.yres > (1ull << 22))
        throw UnsupportedError("StratifiedSampler on the device: at most 1024 samples per pixel and 2^22 pixels");
      if (desc_.sampler.dimension > (int64_t)kStMask || 3 * (int64_t)desc_.integrator.max_depth + 4 > (int64_t)kStMask)
        throw UnsupportedError("StratifiedSampler on the device: dimension counters are 12 bits");
      // under this sampler a path's bounce count rides in the 8 bits the two counters leave of its queue word (dmath.hpp db_pack)
      if (desc_.integrator.max_depth > (int64_t)kDbMaxBounceStratified) throw UnsupportedError("StratifiedSampler on the device: max_depth above 255");
      if (desc_.sampler.xsamp < 1 || desc_.sampler.ysamp < 1) throw PanicError("stratified sampler with zero strata");
      // `dimension` 0: even the film sample is one of the rng.gen_range(-1.0..1.0) draws (samplers/mod.rs:211-226), i.e. it can leave
      // its pixel towards -x / -y; the film kernels assume p_film inside the sample's pixel
      if (desc_.sampler.dimension < 1) throw UnsupportedError("StratifiedSampler with dimension 0 (film samples outside their pixel)");
      return;
    }
    if (desc_.sampler.type != RRT_SAMPLER_HALTON) throw UnsupportedError("unknown sampler type");
    const uint64_t max_index = desc_.sampler.sample_stride * (desc_.sampler.samples_per_pixel + 1);
    if (max_index >= (1ull << 32)) throw UnsupportedError("Halton sample index exceeds 32 bits (nsamp too large for this build)");
  }

  // prepare (host/scene_prep.hpp: plain host code), upload each vector, fill the SceneDev / TravScene pointers and scalars, set the member flags
  void upload_scene(const rrt_scene_desc* d) {
    constexpr bool kF32 = std::is_same<R, float>::value;
#ifdef RRT_SLAB_FMA
    const double slab_pad = kF32 ? (double)kSlabPadUlps : 0.0;   // fp32 boxes padded outward for the FMA slab form (dtraverse_f32.hpp lane_ray_set_inv)
#else
    const double slab_pad = 0.0;
#endif
    FlatScene<R> fs = flatten_scene<R>(d, slab_pad);
    has_transmissive_ = fs.used.has_transmissive; has_translucent_ = fs.used.has_translucent; area_lights_ = fs.used.area_lights;
    has_specular_ = false;   // some primitive's material is a Mirror or a Glass: the only surfaces render_aov_follow can follow
    for (size_t i = 0; i < d->n_prims; i++) {
      const int mt = d->materials[d->prims[i].material].type;
      if (mt == RRT_MAT_MIRROR || mt == RRT_MAT_GLASS) has_specular_ = true;
    }
    // render_mattes: the primitive behind each entry of prim_order and its material index + 1 (the ids of a NULL prim_id), kept on the host
    matte_order_.assign(d->prim_order, d->prim_order + d->n_prim_order);
    matte_mat_.resize(d->n_prim_order);
    for (size_t i = 0; i < d->n_prim_order; i++) matte_mat_[i] = d->prims[d->prim_order[i]].material + 1u;
    // rrt_surface_at, rrt_atlas_sites: which entries of prim_order are spheres (refused as sites and as candidates), kept on the host
    surf_sphere_.resize(fs.tris.size());
    for (size_t i = 0; i < fs.tris.size(); i++) surf_sphere_[i] = fs.tris[i].plane == kSphereMark ? 1 : 0;
    {   // rrt_nearest: M = the largest coordinate a query meets - the root box, and what a kept instance's vertex transform sums up (|m_ij| |v_j| + |t_i|)
      double M = 0.0;
      if (!fs.nodes.empty()) for (int k = 0; k < 3; k++) M = std::max({M, std::fabs((double)fs.nodes[0].bmin[k]), std::fabs((double)fs.nodes[0].bmax[k])});
      nn_has_tri_ = false;
      bool kept = false;
      for (const Tri<R>& t : fs.tris) {
        if (t.plane == kSphereMark) continue;
        nn_has_tri_ = true;
        if ((t.material & kInstFlag) == 0u) continue;
        kept = true;
        const R* m = fs.insts[(t.material >> 16) & 0x7fffu].m;
        for (const R* v : {t.p0, t.p1, t.p2}) for (int i = 0; i < 3; i++)
          M = std::max(M, std::fabs((double)m[4 * i] * (double)v[0]) + std::fabs((double)m[4 * i + 1] * (double)v[1]) + std::fabs((double)m[4 * i + 2] * (double)v[2]) + std::fabs((double)m[4 * i + 3]));
      }
      nn_delta_ = (R)((double)kNearestPadUlps * (double)NnConst<R>::eps * M);
      mh_delta_ = kept ? (R)((double)kMultihitPadUlps * (double)NnConst<R>::eps * M) : R(0);
    }
    shade_kinds_scene_ = fs.used.shade == ShadeClass::Lambert ? kKindsLambert : (fs.used.shade == ShadeClass::Glossy ? kKindsGlossy : kAllKinds);
    shade_kinds_ = shade_kinds_scene_;
    if (!fs.used.warning.empty()) warnings.push_back(fs.used.warning);
    tex_depth_ = fs.tex_depth;
    const uint32_t cam_blocks[3] = {kCamB3, kCamB5, kCamB7};
    const SamplerTables stab = build_sampler_tables(d, kF32, kHaltonTabDims, cam_blocks, cam_tables_on_);

    nodes_.upload(fs.nodes, st_); tris_.upload(fs.tris, st_); spheres_.upload(fs.spheres, st_); insts_.upload(fs.insts, st_);
    if constexpr (kF32) {   // the fp32 traversal kernels' tree: pair nodes, any-hit start lists, quad nodes (dtraverse_f32.hpp)
      pairs_ok_ = false;
      const PairTables pt = build_pairs(fs.nodes, fs.tris, kTreeletNodes);
      mixed_ = pt.mixed; trav_.n_treelet = pt.n_treelet;
      any_list_.upload(pt.any_list, st_);
      if (pt.ok) {
        pairs_.upload(pt.pairs, st_);
        HIP_CHECK(hipStreamSynchronize(st_));
        trav_.any_list = (any_entry_on_ && any_list_.n) ? reinterpret_cast<const uint4*>(any_list_.p) : nullptr;
        trav_.pairs = pairs_.p;
        trav_.tris = reinterpret_cast<const float*>(tris_.p);
        for (int k = 0; k < 6; k++) trav_.root_box[k] = pt.root_box[k];
        trav_.root_id = pt.root_id;
        trav_.spheres = spheres_.p; trav_.insts = insts_.p;
        trav_.n_nodes = pt.n_nodes;
        pairs_ok_ = true;
        quads_.release(); trav_.quads = nullptr; trav_.n_qtreelet = 0;
        if (!mixed_) {
          const QuadTables qt = build_quads(fs.nodes, kQuadTreelet);
          trav_.n_qtreelet = qt.n_qtreelet;
          if (!qt.quads.empty()) {
            quads_.upload(qt.quads, st_);
            HIP_CHECK(hipStreamSynchronize(st_));
            trav_.quads = quads_.p;
          }
        }
      }
    }
    shades_.upload(fs.shades, st_);
    materials_.upload(fs.mats, st_); textures_.upload(fs.texs, st_); images_.upload(fs.imgs, st_); image_texels_.upload(fs.texels, st_);
    { const AuxMargins am = calibrate_aux_margins(d); lens_safe_.upload(am.lim, st_); aux_delta_ = am.delta; aux_pupil_ = am.pupil; }
    if constexpr (kF32) {
      const LensCull lc = build_lens_cull(d);
      if (!lc.bits.empty()) { lens_cull_.upload(lc.bits, st_); lc_inv_dr_ = lc.inv_dr; }
    }
    if constexpr (kF32) {
      // shadow candidate lists (dtraverse_f32.hpp): scenes whose lights are all point / distant lights, triangles in world space only
      shadow_lists_ok_ = false;
      if (pairs_ok_ && !mixed_ && d->n_lights > 0 && d->bvh_depth + 1 <= 64) {
        const auto t_sl0 = std::chrono::steady_clock::now();
        ShadowListsHost sl = build_shadow_lists(fs.nodes, fs.tris, d);
        const double t_sl = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_sl0).count();
        if (sl.n_tables > 0) {
          sl_headers_.upload(sl.headers, st_); sl_entries_.upload(sl.entries, st_); sl_leaves_.upload(sl.leaves, st_);
          HIP_CHECK(hipStreamSynchronize(st_));
          sl_dev_ = ShadowLists{sl_headers_.p, sl_entries_.p, sl_leaves_.p, (uint32_t)fs.tris.size(), sl.n_tables};
          for (size_t i = 0; i < d->n_lights; i++) fs.lights[i].shadow_tab = sl.table_of_light[i];
          shadow_lists_ok_ = true;
          size_t n_with = 0, n_entries = 0;
          for (uint32_t h : sl.headers) if ((h & 0xffu) != 0xffu) { n_with++; n_entries += h & 0xffu; }
          if (getenv("RRT_DEBUG")) fprintf(stderr, "[rrt] shadow lists: %u table(s), %zu of %zu (table, triangle) pairs listed, %.2f candidate leaves on average, built in %.3f s\n", sl.n_tables, n_with, sl.headers.size(), n_with ? (double)n_entries / (double)n_with : 0.0, t_sl);
        }
      }
    }
    if constexpr (kF32) {
      // horizon tables: which bounce rays of the path integrator provably leave the scene (build_horizons())
      horizon_.release(); horizon_tau_.release();
      const char* hz_env = getenv("RRT_HORIZON_TABLES");   // =0: build none (the "horizon_cull" option then has nothing to switch on)
      if (pairs_ok_ && !mixed_ && d->integrator.type == RRT_INT_PATH && d->bvh_depth + 1 <= 64 && fs.tris.size() < (1u << 27) && !(hz_env && atoi(hz_env) == 0)) {
        const auto t_h0 = std::chrono::steady_clock::now();
        std::vector<HzNode> hn(fs.nodes.size());
        std::vector<HzTri> ht(fs.tris.size());
        for (size_t i = 0; i < fs.nodes.size(); i++) { for (int c = 0; c < 3; c++) { hn[i].bmin[c] = fs.nodes[i].bmin[c]; hn[i].bmax[c] = fs.nodes[i].bmax[c]; } hn[i].offset = fs.nodes[i].offset; hn[i].n_prims = fs.nodes[i].meta >> 2; }
        for (size_t i = 0; i < fs.tris.size(); i++) { for (int c = 0; c < 3; c++) { ht[i].p[0][c] = fs.tris[i].p0[c]; ht[i].p[1][c] = fs.tris[i].p1[c]; ht[i].p[2][c] = fs.tris[i].p2[c]; } ht[i].skip = (fs.tris[i].plane == kSphereMark || (fs.tris[i].material & kInstFlag) != 0u) ? 1u : 0u; }
        const char* chk = getenv("RRT_HZ_CHECK");
        bool cached = false;
        const std::shared_ptr<const HzTables> hz = horizons_cached(hn, ht, chk ? atol(chk) : 0, &cached);
        if (hz->check_hits != 0) throw DeviceError("internal: horizon tables are not conservative (" + std::to_string(hz->check_hits) + " of " + std::to_string(hz->checked) + " free rays hit geometry)");
        hz_axis_ = hz->axis;
        horizon_.upload(hz->bytes, st_); horizon_tau_.upload(hz->tau, st_);
        HIP_CHECK(hipStreamSynchronize(st_));
        if (!cached) hz_build_s_ = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_h0).count();
        if (getenv("RRT_DEBUG")) fprintf(stderr, "[rrt] horizon tables: axis %u, %zu triangles, mean open share of the upper sectors %.3f, %s in %.3f s%s\n", hz_axis_, fs.tris.size(), hz->mean_open, cached ? "found" : "built",
                                         std::chrono::duration<double>(std::chrono::steady_clock::now() - t_h0).count(), chk ? (" (self-check: " + std::to_string(hz->checked) + " free rays, " + std::to_string(hz->check_hits) + " hits)").c_str() : "");
      }
    }
    lights_.upload(fs.lights, st_); light_cdf_.upload(fs.light_cdf, st_); lens_.upload(fs.lens, st_); hdims_.upload(stab.hdims, st_); perms_.upload(stab.perms, st_);
    HIP_CHECK(hipStreamSynchronize(st_));  // host vectors go out of scope below

    SceneDev<R>& s = scene_;
    const size_t nl = d->n_lights;
    const double func_int = fs.light_func_int;
    s.nodes = nodes_.p; s.tris = tris_.p; s.shades = shades_.p; s.spheres = spheres_.p; s.insts = insts_.p; s.materials = materials_.p; s.textures = textures_.p; s.images = images_.p; s.image_texels = image_texels_.p; s.lights = lights_.p; s.light_cdf = light_cdf_.p;
    s.n_nodes = (uint32_t)d->n_bvh_nodes; s.n_tris = (uint32_t)d->n_prim_order; s.n_lights = (uint32_t)nl;
    s.light_pick_pdf = (nl && func_int > 0.0) ? (R)(1.0 / (func_int * (double)nl)) : (R)0;
    s.stack_depth = d->bvh_depth + 1;
    deep_ = d->bvh_depth + 1 > 64;
    s.flags = d->flags;
    s.lens = lens_.p; s.n_lens = d->camera.n_elems; s.simple_weighting = d->camera.simple_weighting;
    affine_rows(d->camera.camera_to_world.m, s.cam_m, "camera_to_world");
    for (int k = 0; k < 4; k++) { s.pupil0[k] = (R)d->camera.exit_pupil_bounds[0][k]; s.pupil63[k] = (R)d->camera.exit_pupil_bounds[63][k]; }
    s.shutter_open = (R)d->camera.shutter_open; s.shutter_close = (R)d->camera.shutter_close;
    s.xres = d->film.xres; s.yres = d->film.yres; s.diagonal = (R)d->film.diagonal;
    for (int k = 0; k < 4; k++) s.extent[k] = (R)d->film.physical_extent[k];
    s.max_sample_luminance = std::isinf(d->film.max_sample_luminance) ? Const<R>::inf : (R)d->film.max_sample_luminance;
    s.hdims = hdims_.p; s.perms = perms_.p;
    s.diff_scale = (R)(1.0 / std::sqrt((double)d->sampler.samples_per_pixel));
    s.nsamp = (uint32_t)d->sampler.samples_per_pixel; s.sample_at_center = (uint32_t)d->sampler.sample_at_center;
    s.base_exp0 = (uint32_t)d->sampler.base_exponents[0]; s.base_exp1 = (uint32_t)d->sampler.base_exponents[1];
    s.base_scale0 = (uint32_t)d->sampler.base_scales[0]; s.base_scale1 = (uint32_t)d->sampler.base_scales[1];
    s.stride = (uint32_t)d->sampler.sample_stride; s.mult_inv0 = (uint32_t)d->sampler.mult_inverse[0]; s.mult_inv1 = (uint32_t)d->sampler.mult_inverse[1];
    s.fast_div = (d->sampler.sample_stride * (d->sampler.samples_per_pixel + 1) < (1ull << 26)) ? 1u : 0u;
    s.inv_base_scale1 = 1.0 / (double)std::max<uint32_t>(1u, s.base_scale1);
    for (int k = 0; k < 24; k++) s.inv3pow[k] = stab.inv3pow[k];
    for (int w = 0; w < 2; w++) {   // lens dims 2, 3
      s.cam_perm[w] = stab.cam_perm[w]; s.cam_tail[w] = stab.cam_tail[w];
      for (int k = 0; k < 16; k++) s.cam_invpow[w][k] = stab.cam_invpow[w][k];
    }
    for (int w = 0; w < 3; w++) { s.cam_lo[w] = nullptr; s.cam_hi[w] = nullptr; }
    s.hblk = nullptr; s.hlo = nullptr; s.hhi = nullptr; s.n_hblk = 0;
    if (!stab.blk.empty()) {   // block tables of the dimensions the integrators draw (SceneDev::hblk, halton_dim())
      hblk_.upload(stab.blk, st_); hlo_.upload(stab.lo, st_); hhi_.upload(stab.hi, st_);
      HIP_CHECK(hipStreamSynchronize(st_));
      s.hblk = hblk_.p; s.hlo = hlo_.p; s.hhi = hhi_.p; s.n_hblk = (uint32_t)kHaltonTabDims;
    }
    if (stab.has_cam) {   // block tables of the camera dimensions' digit loops (SceneDev::cam_lo / cam_hi, halton_cam4())
      cam_lo_.upload(stab.cam_lo, st_); cam_hi_.upload(stab.cam_hi, st_);
      HIP_CHECK(hipStreamSynchronize(st_));
      for (int w = 0; w < 3; w++) { cam_lo_off_[w] = stab.cam_lo_off[w]; cam_hi_off_[w] = stab.cam_hi_off[w]; s.cam_lo[w] = cam_lo_.p + cam_lo_off_[w]; s.cam_hi[w] = cam_hi_.p + cam_hi_off_[w]; }
    }
    {
      std::vector<R> ft(256);
      for (int i = 0; i < 256; i++) ft[i] = (R)d->film.filter_table[i];
      filter_table_.upload(ft, st_);
      HIP_CHECK(hipStreamSynchronize(st_));
      s.filter_table = filter_table_.p;
      s.filter_rx = (R)d->film.filter_radius[0]; s.filter_ry = (R)d->film.filter_radius[1];
      s.filter_inv_rx = (R)(1.0 / d->film.filter_radius[0]); s.filter_inv_ry = (R)(1.0 / d->film.filter_radius[1]);
    }
    s.sampler_type = (uint32_t)d->sampler.type;
    s.st_nx = (uint32_t)std::max(1, d->sampler.xsamp); s.st_ny = (uint32_t)std::max(1, d->sampler.ysamp);
    s.st_jitter = d->sampler.jitter ? 1u : 0u; s.st_dims = (uint32_t)std::max(0, d->sampler.dimension);
    s.st_seed_lo = (uint32_t)d->sampler.perm_seed; s.st_seed_hi = (uint32_t)(d->sampler.perm_seed >> 32);
    s.cam_db = d->sampler.type == RRT_SAMPLER_STRATIFIED ? (1u | (2u << kStBits)) : 5u;
    s.db_shift = d->sampler.type == RRT_SAMPLER_STRATIFIED ? kDbShiftStratified : kDbShiftHalton;
    s.shade_compact = 1u;
    s.integrator = d->integrator.type; s.max_depth = d->integrator.max_depth; s.light_strategy = d->integrator.light_strategy;
    s.rr_threshold = (R)d->integrator.rr_threshold;
    counters_.alloc(C_COUNT);
    HIP_CHECK(hipMemsetAsync(counters_.p, 0, C_COUNT * sizeof(uint32_t), st_));
    s.err = counters_.p + C_ERROR;
  }

  // The path integrator alternates two shadow queues, so that shading bounce k + 1 need not wait for the shadow rays of bounce k
  bool two_shadow_queues() const { return overlap_shadow_ && desc_.integrator.type == RRT_INT_PATH && !deep_; }
  // 12 four-word records per slot, +4 camera ray differentials on textured scenes, +3 for the second shadow queue
  size_t n_vec_records() const { return 12 + (tex_depth_ > 0 ? 4 : 0) + (two_shadow_queues() ? 3 : 0); }
  void ensure_pools(size_t n) {
    if (n <= cap_) return;
    HIP_CHECK(hipStreamSynchronize(st_));
    cap_ = n;
    using V4 = typename Vec4T<R>::type;
    const size_t NV = n_vec_records(), NR = 1, NU = 9;   // 4-word records, reals, u32 per slot
    vpool_.alloc(NV * cap_);
    rpool_.alloc(NR * cap_);
    upool_.alloc(NU * cap_);
    Pools<R>& p = pool_;
    V4* v = vpool_.p;
    auto nv = [&]() { V4* x = v; v += cap_; return x; };
    p.ray_o = nv(); p.ray_d = nv(); p.nray_o = nv(); p.nray_d = nv(); p.hit = nv();
    p.sray_o = nv(); p.sray_d = nv(); p.sld = nv(); p.samp = nv(); p.path = nv(); p.npath = nv(); p.L = nv();
    p.rdx_o = p.rdx_d = p.rdy_o = p.rdy_d = nullptr;
    if (tex_depth_ > 0) { p.rdx_o = nv(); p.rdx_d = nv(); p.rdy_o = nv(); p.rdy_d = nv(); }
    R* r = rpool_.p;
    auto nr = [&]() { R* x = r; r += cap_; return x; };
    p.weight = nr();
    uint32_t* u = upool_.p;
    auto nu = [&]() { uint32_t* x = u; u += cap_; return x; };
    p.q_active = (QEnt*)u; u += 4 * cap_; p.q_next = (QEnt*)u; u += 4 * cap_; p.hindex = nu();
    p.counters = counters_.p;
    p.pix_off = pix_off_.p;
    p.shadow_count = counters_.p + C_SHADOW;
    shadow_buf_[0][0] = p.sray_o; shadow_buf_[0][1] = p.sray_d; shadow_buf_[0][2] = p.sld;
    shadow_buf_[1][0] = shadow_buf_[1][1] = shadow_buf_[1][2] = nullptr;
    if (two_shadow_queues()) { shadow_buf_[1][0] = nv(); shadow_buf_[1][1] = nv(); shadow_buf_[1][2] = nv(); }
    if (deep_) deep_stack_.alloc((size_t)scene_.stack_depth * cap_);

  }

  void load_rays(const rrt_rays* rays, size_t n) {
    const uint32_t g = (uint32_t)((n + kBlock - 1) / kBlock);
    if (rays->mem == RRT_MEM_DEVICE) {
      hipLaunchKernelGGL((k_pack_rays<R>), dim3(g), dim3(kBlock), 0, st_, pool_, (const R*)rays->ox, (const R*)rays->oy, (const R*)rays->oz,
                         (const R*)rays->dx, (const R*)rays->dy, (const R*)rays->dz, (const R*)rays->tmax, (const int32_t*)rays->skip_prim, (uint32_t)n, scene_.n_tris);
      return;
    }
    DevBuf<R> sr; DevBuf<int32_t> sk;
    sr.alloc(7 * n);
    const void* src[7] = {rays->ox, rays->oy, rays->oz, rays->dx, rays->dy, rays->dz, rays->tmax};
    for (int k = 0; k < 7; k++) HIP_CHECK(hipMemcpyAsync(sr.p + k * n, src[k], n * sizeof(R), hipMemcpyHostToDevice, st_));
    if (rays->skip_prim) { sk.alloc(n); HIP_CHECK(hipMemcpyAsync(sk.p, rays->skip_prim, n * sizeof(int32_t), hipMemcpyHostToDevice, st_)); }
    hipLaunchKernelGGL((k_pack_rays<R>), dim3(g), dim3(kBlock), 0, st_, pool_, sr.p, sr.p + n, sr.p + 2 * n, sr.p + 3 * n, sr.p + 4 * n, sr.p + 5 * n, sr.p + 6 * n,
                       (const int32_t*)sk.p, (uint32_t)n, scene_.n_tris);
    HIP_CHECK(hipStreamSynchronize(st_));   // staging buffers go out of scope
  }
  // active <- next for the queue and for the rays stored at its positions
  void swap_queues() { std::swap(pool_.q_active, pool_.q_next); std::swap(pool_.ray_o, pool_.nray_o); std::swap(pool_.ray_d, pool_.nray_d); std::swap(pool_.path, pool_.npath); }

  // camera_rays: the queue is the one the camera kernels of this pass filled (tile trees, where the pass has them)
  void launch_closest(const uint32_t* queue, const uint32_t* count, uint32_t n_fixed, bool counting, uint32_t* cn, uint32_t* cp,
                      unsigned long long* totals, uint32_t grid_override = 0, bool camera_rays = false) {
    const uint32_t grid = grid_override ? grid_override : (uint32_t)((n_fixed + kBlock - 1) / kBlock);
    if (!counting && use_persistent()) { launch_persistent(TravJob{false, AnySink::film, queue, count, n_fixed, nullptr, st_}, grid, camera_rays && tt_pass_ok_ && count != nullptr); return; }
    with_flag(deep_, [&](auto DEEP) { with_flag(counting, [&](auto COUNT) {
      hipLaunchKernelGGL((k_closest<R, DEEP(), COUNT()>), dim3(grid), dim3(kBlock), 0, st_, scene_, pool_, queue, count, n_fixed, deep_stack(), deep_stride(), cn, cp, totals);
    }); });
    HIP_CHECK(hipGetLastError());
  }
  // the per-slot stacks of the generic kernels' DEEP instantiations (trees deeper than 64 levels)
  uint32_t* deep_stack() const { return deep_ ? deep_stack_.p : nullptr; }
  uint32_t deep_stride() const { return deep_ ? (uint32_t)cap_ : 0u; }
  // camera ray generation: the dense lean-arithmetic kernels in fp32 (dtraverse_f32.hpp), the generic two-stage kernels (main trace, auxiliary traces; the
  // reference's operation order) in f64 and for what the dense ones do not cover
  // for_render: the queue feeds the integrator (camera rays that miss the root box may be answered here); otherwise every survivor's ray is wanted (rrt_camera_samples)
  // list: the tiles of a listed pass (list_pixel): the same camera kernels behind the list form of k_pixel_offsets, or k_raygen_list; no tile trees
  void launch_raygen(const PassDesc& pd, uint32_t grid, double* dims_out, int enqueue, bool for_render = false, bool film_records = true, const uint32_t* list = nullptr) {
    tt_pass_ok_ = false;
    film_runs_ok_ = false;
    scene_.root_cull = 0u;
    if constexpr (std::is_same<R, float>::value) {
      // a miss is shaded with nothing by the path integrator only (DirectLighting / Debug panic on a miss without lights, Q20), and the root test that
      // is replayed is the pair-node kernels' (lane_ray_begin); counting frames keep every query in the queue
      if (for_render && root_cull_on_ && enqueue && desc_.integrator.type == RRT_INT_PATH && use_persistent() && !count_traversal_ && trav_.n_nodes != 0u) {
        scene_.root_cull = 1u;
        for (int k = 0; k < 6; k++) scene_.root_box[k] = trav_.root_box[k];
      }
    }
    if constexpr (std::is_same<R, float>::value) {
      if (raygen_lean_ && dense_raygen_ok()) {   // everything else takes the generic kernels below, which have no such limits
        const uint32_t total = pd.npix * pd.ns;
        if (pix_off_.n < 2 * (size_t)pd.npix) { HIP_CHECK(hipStreamSynchronize(st_)); pix_off_.alloc(2 * (size_t)pd.npix); }
        pool_.pix_off = pix_off_.p;
        const int write_samp = wide_filter() ? 1 : 0;   // only the wide film kernels read p_film
        if (list) hipLaunchKernelGGL(k_pixel_offsets_list, dim3((pd.npix + kBlock - 1) / kBlock), dim3(kBlock), 0, st_, scene_, pool_, pd, list);
        else hipLaunchKernelGGL(k_pixel_offsets, dim3((pd.npix + kBlock - 1) / kBlock), dim3(kBlock), 0, st_, scene_, pool_, pd);
        // (dead samples: weight 0, Q2 - written by k_raygen_main_f32 itself, one coalesced store per sample)
        {   // dense two-stage version with the lean lens arithmetic
          const float2* safe_r2 = (aux_margin_ && tex_depth_ == 0) ? reinterpret_cast<const float2*>(lens_safe_.p) : nullptr;   // textured scenes keep the auxiliary rays themselves (ray differentials)
          // lens cull table (option lens_cull): tiled passes of untextured scenes
          const uint32_t* cull = (lens_cull_on_ && lens_cull_.n != 0 && tex_depth_ == 0 && pd.tiled) ? lens_cull_.p : nullptr;
          // pixel blocks over grid y and z (a grid dimension holds at most 65 535 blocks; a pass has up to 2^28 / 512 of them)
          // samples / pixels per workgroup: 8 samples of one 8 x 8-pixel tile (PassDesc::tiled) where the pass has that many, else one sample of 512 pixels
          const uint32_t spb = (pd.tiled && pd.ns >= (uint32_t)rg_spb_) ? (uint32_t)std::max(1, std::min(rg_spb_, kRgDense / 64)) : 1u, ppb = kRgDense / spb;
          const uint32_t n_pb = (pd.npix + ppb - 1) / ppb, gz = (n_pb + 65534u) / 65535u, gy = (n_pb + gz - 1) / gz;
          // tile trees: the pass qualifies when it covers the whole pixel grid of its rect in tile order with one 8 x 8 tile x 8 samples per camera workgroup
          if (!list && tt_state_ == 1 && tile_trees_on_ && enqueue && pd.tiled && spb == 8 && ppb == kTileW * kTileH && pd.pix_begin == 0 && pd.npix % ((uint32_t)pd.rw * kTileH) == 0 &&
              pd.ns % spb == 0 && use_persistent() && trav_mode_ == 3 && !count_traversal_) {
            const size_t n_chunks = (size_t)gy * gz * ((pd.ns + spb - 1) / spb);
            if (tt_chunks_.n < n_chunks) { HIP_CHECK(hipStreamSynchronize(st_)); tt_chunks_.alloc(n_chunks); }
            tt_pass_ = TileTrees{reinterpret_cast<const float4*>(tt_trees_.p), tt_tris_.p, tt_chunks_.p, (uint32_t)pd.rw / kTileW, pd.npix / (uint32_t)pd.rw / kTileH, pd.ns / spb, tt_mt_x_, tt_n_trees_, pd};
            tt_pass_ok_ = true;
            // film records (option film_records): the path integrator's radiance in record runs, one per camera workgroup (k_film_box_runs). Only where every
            // reader of the per-slot state is known: the box filter of radius 0.5 (write_samp = 0), untextured (no ray differentials per slot), the frame's
            // own passes (not rrt_camera_samples, which reads weight[slot])
            if (film_records_on_ && film_records && for_render && !dims_out && write_samp == 0 && tex_depth_ == 0 && desc_.integrator.type == RRT_INT_PATH) {
              if (film_runs_.n < n_chunks) { HIP_CHECK(hipStreamSynchronize(st_)); film_runs_.alloc(n_chunks); }
              film_runs_ok_ = true;
            }
          }
          hipLaunchKernelGGL(k_raygen_main_f32, dim3((pd.ns + spb - 1) / spb, gy, gz), dim3(kRgDense), 0, st_, scene_, pool_, pd, write_samp, dims_out, safe_r2, aux_delta_, aux_pupil_, enqueue, spb,
                             tt_pass_ok_ ? tt_chunks_.p : nullptr, cull, lc_inv_dr_, film_runs_ok_ ? film_runs_.p : nullptr);
          if (tt_pass_ok_) hipLaunchKernelGGL(k_tt_snapshot, dim3(1), dim3(1), 0, st_, counters_.p);
          hipLaunchKernelGGL(k_raygen_aux2_f32, dim3((total + kRgDense - 1) / kRgDense), dim3(kRgDense), 0, st_, scene_, pool_, enqueue, film_runs_ok_ ? 1 : 0);
          hipLaunchKernelGGL(k_rotate, dim3(1), dim3(1), 0, st_, counters_.p, 4);   // q_next was only a staging queue
        }
        HIP_CHECK(hipGetLastError());
        return;
      }
    }
    if (list) hipLaunchKernelGGL((k_raygen_list<R>), dim3(grid), dim3(kBlock), 0, st_, scene_, pool_, pd, list);
    else hipLaunchKernelGGL((k_raygen<R>), dim3(grid), dim3(kBlock), 0, st_, scene_, pool_, pd, dims_out);
    hipLaunchKernelGGL((k_raygen_aux<R>), dim3(grid), dim3(kBlock), 0, st_, scene_, pool_, enqueue);
    hipLaunchKernelGGL(k_rotate, dim3(1), dim3(1), 0, st_, counters_.p, 4);   // q_next was only a staging queue
    HIP_CHECK(hipGetLastError());
  }
  // the dense fp32 camera kernels cover Halton scenes with lenses of up to 32 interfaces on films below 65 536 px per side (StratifiedSampler and
  // longer lens tables are the generic kernels'); the tile-tree census asks the same question, so that it and the frame take the same camera kernels
  bool dense_raygen_ok() const { return scene_.n_lens <= 32 && scene_.sampler_type == RRT_SAMPLER_HALTON && scene_.xres < 65536 && scene_.yres < 65536; }
  // fp32 production traversal (dtraverse_f32.hpp): 64 B pair nodes, LDS stack with global overflow
  bool use_persistent() const { return std::is_same<R, float>::value && persistent_ && pairs_ok_; }
  // one traversal launch over a queue: closest-hit, or any-hit with its sink. occluded: rrt_trace_any's answers, else NULL
  struct TravJob { bool any; AnySink sink; const uint32_t *queue, *count; uint32_t n_fixed; uint8_t* occluded; hipStream_t stream; };
  // the workgroups of `kernel` that the chip holds at once: the grid of a persistent launch
  template <class K>
  uint32_t resident_grid(K kernel, int block, int* per_cu_out = nullptr) {
    if (n_cus_ == 0) HIP_CHECK(hipDeviceGetAttribute(&n_cus_, hipDeviceAttributeMultiprocessorCount, dev_));
    int per_cu = 0;
    HIP_CHECK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, block, 0));
    if (per_cu_out) *per_cu_out = per_cu;
    return (uint32_t)(std::max(1, per_cu) * std::max(1, n_cus_));
  }
  // Run once per kernel, at the first launch that needs it: the resident grids of the three traversal kernels and the overflow stacks sized by them
  void size_traversal(bool tiles) {
    if (trav_grid_ == 0) {
      with_flag(mixed_, [&](auto MIXED) { trav_grid_ = resident_grid(k_trace_pairs_f32<false, MIXED()>, kTravBlock); });
      if (scene_.stack_depth > (uint32_t)kStackLds) {   // any-hit launches have their own columns: they may run beside a closest-hit launch
        overflow_.alloc((size_t)(scene_.stack_depth - kStackLds) * (size_t)trav_grid_ * kTravBlock * 2);
        overflow_any_.alloc((size_t)(scene_.stack_depth - kStackLds) * (size_t)trav_grid_ * kTravBlock * 2);
      }
    }
    if (trav_mode_ == 1) return;   // grid-stride only
    if (tiles && tt_grid_ == 0) {
      int per_cu = 0;
      tt_grid_ = resident_grid(k_trace_tiles_f32<false>, kTtBlock, &per_cu);
      if (scene_.stack_depth > (uint32_t)kTtStack) tt_overflow_.alloc((size_t)(scene_.stack_depth - kTtStack) * (size_t)tt_grid_ * kTtBlock * 2);
      if (getenv("RRT_DEBUG")) fprintf(stderr, "[rrt] tile trees: %d workgroup(s) of %d threads per CU, grid %u\n", per_cu, kTtBlock, tt_grid_);
    }
    if (!tiles && pt_grid_ == 0) {
      int per_cu = 0, per_cu_q = 0;
      with_flag(mixed_, [&](auto MIXED) { pt_grid_ = resident_grid(k_trace_pt_f32<false, MIXED()>, kPtBlock, &per_cu); });
      if (quads_.n) {   // the two-levels-per-fetch kernel has its own register count, and pushes up to three entries per two levels
        pt_grid_quad_ = resident_grid(k_trace_pt_f32<false, false, true>, kPtBlock, &per_cu_q);
        if (getenv("RRT_DEBUG")) fprintf(stderr, "[rrt] quad nodes: %zu nodes, %d workgroup(s) per CU (pair-node kernel: %d)\n", quads_.n, per_cu_q, per_cu);
      }
      const uint32_t quad_depth = quads_.n ? 3u * ((scene_.stack_depth + 1u) / 2u) + 3u : 0u;   // deepest stack of a quad walk
      const uint32_t depth_cl = std::max(scene_.stack_depth, quad_depth);
      if (pairs_ok_ && depth_cl > (uint32_t)kPtStack) pt_overflow_.alloc((size_t)(depth_cl - kPtStack) * (size_t)std::max(pt_grid_, pt_grid_quad_) * kPtBlock * 2);
      if (pairs_ok_ && scene_.stack_depth > (uint32_t)kPtStackAny) pt_overflow_any_.alloc((size_t)(scene_.stack_depth - kPtStackAny) * (size_t)pt_grid_ * kPtBlock * 2);
    }
  }
  // the grid-stride kernel: persistent workgroups over the queue, one overflow column per resident thread of the persistent grid
  void launch_pairs(const TravJob& j, uint32_t grid, uint32_t hi_gs) {
    TravScene t = trav_;
    t.overflow = j.any ? overflow_any_.p : overflow_.p;
    t.overflow_stride = trav_grid_ * kTravBlock;
    auto go = [&](auto ANY, auto MIXED, auto PASSES, auto AO) {
      hipLaunchKernelGGL((k_trace_pairs_f32<ANY(), MIXED(), PASSES(), AO()>), dim3(grid), dim3(kTravBlock), 0, j.stream, t, pool_, j.queue, j.count, j.n_fixed, j.occluded, 0u, hi_gs);
    };
    with_flag(mixed_, [&](auto MIXED) {
      if (j.any) with_sink(j.sink, [&](auto PASSES, auto AO) { go(kYes, MIXED, PASSES, AO); });
      else go(kNo, MIXED, kNo, kNo);
    });
  }
  // the persistent-thread kernel; closest-hit launches over all-triangle trees with quad nodes (option quad_nodes) take its QUAD form, which has its own grid
  void launch_pt(const TravJob& j, uint32_t grid, uint32_t lo_pt) {
    const bool quad = !j.any && !mixed_ && quad_on_ && quads_.n && pt_grid_quad_;
    TravScene t = trav_;
    t.overflow = j.any ? pt_overflow_any_.p : pt_overflow_.p;
    t.overflow_stride = (j.any ? pt_grid_ : std::max(pt_grid_, pt_grid_quad_)) * kPtBlock;
    const uint32_t g = std::max(1u, std::min(grid, quad ? pt_grid_quad_ : pt_grid_));
    uint32_t* work = &counters_.p[j.any ? C_WORK8_SHADOW : C_WORK8_CLOSEST];   // 8 cursors, one 128-B line each
    auto go = [&](auto ANY, auto MIXED, auto QUAD, auto PASSES, auto AO) {
      hipLaunchKernelGGL((k_trace_pt_f32<ANY(), MIXED(), QUAD(), PASSES(), AO()>), dim3(g), dim3(kPtBlock), 0, j.stream, t, pool_, j.queue, j.count, j.n_fixed, work, j.occluded, lo_pt, 0xffffffffu);
    };
    if (quad) go(kNo, kNo, kYes, kNo, kNo);
    else with_flag(mixed_, [&](auto MIXED) {
      if (j.any) with_sink(j.sink, [&](auto PASSES, auto AO) { go(kYes, MIXED, kNo, PASSES, AO); });
      else go(kNo, MIXED, kNo, kNo, kNo);
    });
  }
  // camera rays of a pass with chunk records: k_trace_tiles_f32 in the persistent-thread kernel's place
  void launch_tiles(const TravJob& j, uint32_t lo_pt) {
    TravScene t = trav_;
    t.pairs = tt_pairs_.p; t.root_id = 0u;   // slot 0 of every local copy is the root
    t.overflow = tt_overflow_.p;
    t.overflow_stride = tt_grid_ * kTtBlock;
    hipLaunchKernelGGL((k_trace_tiles_f32<false>), dim3(tt_grid_), dim3(kTtBlock), 0, j.stream, t, pool_, j.count, &counters_.p[C_WORK8_CLOSEST], tt_pass_, lo_pt, 0xffffffffu);
  }
  // grid: slots / kBlock thread blocks, as the caller of a generic kernel would ask for. tiles: the queue is a camera queue with chunk records
  void launch_persistent(const TravJob& j, uint32_t grid, bool tiles = false) {
    if constexpr (std::is_same<R, float>::value) {
      size_traversal(tiles);
      // Two kernels, two queue-size regimes (decided on the device from the queue counter): large queues go to the
      // persistent-thread kernel (lane refill keeps the VALUs busy), small ones to the grid-stride kernel (its fixed
      // cost — the latency chain of the longest ray — is lower). trav_mode_: 1 = grid-stride only, 2 = persistent
      // only, 3 = both by regime.
      const uint32_t split = j.any ? pt_split_any_ : pt_split_closest_;
      const uint32_t lo_pt = trav_mode_ == 2 ? 0u : (trav_mode_ == 1 ? 0xffffffffu : split);
      const uint32_t hi_gs = trav_mode_ == 1 ? 0xffffffffu : (trav_mode_ == 2 ? 0u : split);
      // The grid-stride kernel goes FIRST. Both kernels are launched for every queue and the one whose regime it is not returns at once - but
      // even a no-op workgroup needs its LDS to be scheduled, and a no-op launched BEHIND the persistent kernel found the chip held by the
      // other stream's persistent launch (the shadow rays of the previous bounce): rocprofv3 showed the empty k_trace_pairs_f32<false> of bounce
      // 1 waiting 3.5 ms for the any-hit launch of bounce 0 to drain, on the critical path of a frame rendered alone. In front, it is
      // dispatched while the chip is still filling. Its grid is no larger than its regime needs.
      if (trav_mode_ != 2) {
        uint32_t g = std::max(1u, std::min((uint32_t)(((size_t)grid * kBlock + kTravBlock - 1) / kTravBlock), trav_grid_));
        if (trav_mode_ == 3) g = std::max(1u, std::min(g, (split + kTravBlock - 1) / kTravBlock));
        launch_pairs(j, g, hi_gs);
      }
      if (trav_mode_ != 1) { if (tiles) launch_tiles(j, lo_pt); else launch_pt(j, grid, lo_pt); }
      HIP_CHECK(hipGetLastError());
    }
  }
  // Tile trees (dtraverse_f32.hpp, k_trace_tiles_f32): per 32 x 32-pixel patch of the image, a local copy of the kTtNodes pair nodes its camera rays visit
  // most. The census: a few camera samples per pixel through the product's own camera kernels, their rays walked here on the host (plain fp32 slab and
  // Moeller-Trumbore tests, hits accepted like Q10) with a visit counter per pair node and patch. The counts only decide which nodes are copied; what a
  // copy says about a node is the tree's own data, so no result depends on them. A set of most-visited nodes is closed under "parent" (a parent is
  // visited at least as often as its child and has the smaller index, which breaks ties), so every copied node can be reached through copies.
  void build_tile_trees() {
    tt_state_ = -1;
    if constexpr (std::is_same<R, float>::value) {
      // the host copies of the tree are held only while a census needs them: fetched back from the device here, released at the end
      struct HostCopies { std::vector<PairNode>& a; std::vector<Tri<float>>& b; ~HostCopies() { std::vector<PairNode>().swap(a); std::vector<Tri<float>>().swap(b); } } host_copies{pairs_host_, tris_host_};
      if (pairs_host_.empty() && pairs_.n) {
        pairs_host_.resize(pairs_.n); tris_host_.resize(tris_.n);
        HIP_CHECK(hipMemcpy(pairs_host_.data(), pairs_.p, pairs_.n * sizeof(PairNode), hipMemcpyDeviceToHost));
        if (tris_.n) HIP_CHECK(hipMemcpy(tris_host_.data(), tris_.p, tris_.n * sizeof(Tri<float>), hipMemcpyDeviceToHost));
      }
      const size_t n_int = pairs_host_.size();
      if (!use_persistent() || mixed_ || !dense_raygen_ok() || !raygen_lean_ || n_int <= kTtNodes || trav_.root_id != 0u || (uint64_t)n_int * 64u + kTtLocalBytes >= kIdle) return;
      const uint64_t s_total = desc_.sampler.samples_per_pixel > 1 ? desc_.sampler.samples_per_pixel - 1 : 0;
      if (s_total == 0 || cap_ == 0) return;
      const auto t_begin = std::chrono::steady_clock::now();
      const size_t W = (size_t)desc_.film.xres, H = (size_t)desc_.film.yres;
      const uint32_t mt_x = (uint32_t)((W + kTtMacro - 1) / kTtMacro), mt_y = (uint32_t)((H + kTtMacro - 1) / kTtMacro), n_trees = mt_x * mt_y;
      const uint32_t S = (uint32_t)std::min<uint64_t>((uint64_t)tt_census_spp_, s_total);
      // the census renders the image in pixel groups of what the pools hold: with very small pools (option "max_paths") that would be thousands of launches
      // for passes that do not qualify anyway - try again when the pools have grown
      if (cap_ / S < std::min<size_t>(W * H, 65536)) { tt_state_ = 0; return; }
      // Bounded cost: the census copies ~32 B per camera ray to the host and the copies take (patches + 1) x kTtNodes x 64 B on both sides. Films beyond
      // kTtMaxPixels (4096^2: 1 GB of transient host memory, 240 MB of HBM per handle) keep the ordinary kernels instead of a blocking, unbounded first frame.
      constexpr size_t kTtMaxPixels = (size_t)4096 * 4096;
      if (W * H > kTtMaxPixels) { warnings.push_back("tile_trees: film larger than 4096 x 4096 pixels - camera rays keep the ordinary traversal kernel"); return; }
      // ---- camera rays of the census, bucketed by patch
      std::vector<CensusRay> rays;
      std::vector<uint32_t> tree_of;
      {
        const size_t group = std::max<size_t>(1, std::min(W * H, cap_ / S));
        std::vector<QEnt> q; std::vector<float4> ro, rd;
        const bool save_ok = tt_pass_ok_;
        for (size_t g0 = 0; g0 < W * H; g0 += group) {
          const size_t npix = std::min(group, W * H - g0);
          PassDesc pd{0, 0, (int32_t)W, (uint32_t)g0, (uint32_t)npix, 1u, S, 1u << 30, 1u, 0u, 0u};
          HIP_CHECK(hipMemsetAsync(counters_.p, 0, C_COUNT * sizeof(uint32_t), st_));
          launch_raygen(pd, (uint32_t)((npix * S + kBlock - 1) / kBlock), nullptr, 1);
          uint32_t n = 0;
          HIP_CHECK(hipMemcpyAsync(&n, counters_.p + C_ACTIVE, sizeof(n), hipMemcpyDeviceToHost, st_));
          HIP_CHECK(hipStreamSynchronize(st_));
          q.resize(n); ro.resize(n); rd.resize(n);
          if (n) {
            HIP_CHECK(hipMemcpy(q.data(), pool_.q_active, (size_t)n * sizeof(QEnt), hipMemcpyDeviceToHost));
            HIP_CHECK(hipMemcpy(ro.data(), pool_.ray_o, (size_t)n * sizeof(float4), hipMemcpyDeviceToHost));
            HIP_CHECK(hipMemcpy(rd.data(), pool_.ray_d, (size_t)n * sizeof(float4), hipMemcpyDeviceToHost));
          }
          for (uint32_t i = 0; i < n; i++) {
            const size_t lin = g0 + q[i].slot % npix, x = lin % W, y = lin / W;
            rays.push_back(CensusRay{{ro[i].x, ro[i].y, ro[i].z}, {rd[i].x, rd[i].y, rd[i].z}});
            tree_of.push_back((uint32_t)((y / kTtMacro) * mt_x + x / kTtMacro));
          }
        }
        tt_pass_ok_ = save_ok;
      }
      // ---- per patch: walk, count, choose, copy (host/trav_tables.cpp)
      const TileTreeTables tt = rrtd::build_tile_trees(pairs_host_, tris_host_, trav_.root_box, rays, tree_of, n_trees, TileTreeSizes{kTtNodes, kTtTris, kTtLocalBytes});
      if (tt.failed) { warnings.push_back("tile_trees: the census ran out of host memory - camera rays keep the ordinary traversal kernel"); return; }
      tt_pairs_.upload(tt.shifted, st_); tt_trees_.upload(tt.trees, st_);
      if (kTtTris > 0) {
        tt_tris_.upload(tt.packets, st_);
        if (getenv("RRT_DEBUG")) fprintf(stderr, "[rrt] tile trees: triangle packets of %u triangles per patch, share of the census rays' leaf visits they serve: %.3f\n",
                                         kTtTris, tt.sum_tests ? (double)tt.sum_local_tests / (double)tt.sum_tests : 0.0);
      }
      HIP_CHECK(hipStreamSynchronize(st_));
      tt_mt_x_ = mt_x; tt_n_trees_ = n_trees;
      tt_state_ = 1;
      if (getenv("RRT_DEBUG")) fprintf(stderr, "[rrt] tile trees: %u patches of %u x %u pixels, %zu census rays (%u spp), %.1f distinct pair nodes visited per patch with rays (%llu patches), %.1f MB, built in %.3f s\n",
                                       n_trees, kTtMacro, kTtMacro, rays.size(), S, tt.n_with ? (double)tt.sum_nodes / (double)tt.n_with : 0.0, (unsigned long long)tt.n_with,
                                       (double)(tt.trees.size() * sizeof(PairNode)) / 1e6, std::chrono::duration<double>(std::chrono::steady_clock::now() - t_begin).count());
    }
  }
  // (the shading kernels that feed the shadow queue - k_shade_path, k_shade_nee - store the light table with the ray's start triangle)
  bool use_shadow_lists() const { return std::is_same<R, float>::value && shadow_lists_ok_ && shadow_lists_on_ && !count_traversal_ && use_persistent(); }
  // The sink of an any-hit launch, decided here for every kernel family. Precedence: a rrt_render_ao round is AO whatever else is set; then the
  // shadow launch of a passes frame adds to the pending planes (add_pending<R, true>) - not rrt_trace_any's launch, which hands in `occluded`
  // and touches no radiance; everything else is the film's. A closest-hit launch has no sink.
  AnySink any_sink(bool ao, const uint8_t* occluded) const { return ao ? AnySink::ao : (passes_n_ > 0 && !occluded) ? AnySink::passes : AnySink::film; }
  // Every any-hit launch: the pool's shadow queue for an integrator or (ao) a rrt_render_ao round, or rrt_trace_any's n_fixed rays answered into
  // `occluded`. Shadow candidate lists are per light: the integrators' launches only. A counting frame's shadow rays keep the generic kernels;
  // AO rounds and rrt_trace_any count nothing.
  void launch_any(uint32_t grid, hipStream_t stream, bool ao = false, uint32_t n_fixed = 0, uint8_t* occluded = nullptr) {
    const AnySink sink = any_sink(ao, occluded);
    const bool shadow = !ao && !occluded;
    if constexpr (std::is_same<R, float>::value) {
      if (shadow && use_shadow_lists()) {   // (the shading kernel stored the light table with the ray's start triangle: scene_.use_shadow_tabs)
        const uint32_t g = std::max(1u, std::min((uint32_t)(((size_t)grid * kBlock + kSlBlock - 1) / kSlBlock), (uint32_t)sl_grid_cap_));
        with_flag(sink == AnySink::passes, [&](auto PASSES) {
          hipLaunchKernelGGL((k_shadow_lists_f32<PASSES()>), dim3(g), dim3(kSlBlock), 0, stream, trav_, sl_dev_, pool_, pool_.shadow_count);
        });
        HIP_CHECK(hipGetLastError());
        return;
      }
    }
    const uint32_t* count = occluded ? nullptr : pool_.shadow_count;
    if (use_persistent() && !(shadow && count_traversal_)) { launch_persistent(TravJob{true, sink, nullptr, count, n_fixed, occluded, stream}, grid); return; }
    const bool counting = shadow && count_traversal_;
    auto go = [&](auto DEEP, auto COUNT, auto PASSES, auto AO) {
      hipLaunchKernelGGL((k_shadow<R, DEEP(), COUNT(), PASSES(), AO()>), dim3(grid), dim3(kBlock), 0, stream, scene_, pool_, (const uint32_t*)nullptr, count, deep_stack(), deep_stride(),
                         counting ? totals_.p + 5 : nullptr);
    };
    with_flag(deep_, [&](auto DEEP) {
      if (occluded) hipLaunchKernelGGL((k_any_public<R, DEEP()>), dim3(grid), dim3(kBlock), 0, stream, scene_, pool_, n_fixed, occluded, deep_stack(), deep_stride());
      else if (ao) go(DEEP, kNo, kNo, kYes);
      else with_flag(counting, [&](auto COUNT) { with_flag(sink == AnySink::passes, [&](auto PASSES) { go(DEEP, COUNT, PASSES, kNo); }); });
    });
    HIP_CHECK(hipGetLastError());
  }
};

HandleBase* make_handle_f32(int device, const rrt_scene_desc* d);
HandleBase* make_handle_f64(int device, const rrt_scene_desc* d);

}  // namespace rrtd