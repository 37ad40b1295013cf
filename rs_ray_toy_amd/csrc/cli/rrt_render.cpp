// rrt_render <scene.json> <out.png> — the reference's command line (main.rs:55-61 -> deploy_render renderprocess.rs:92-105)
// over the C ABI of include/rrt.h, plain C++ (no HIP, no Python): the caller a Rust host would be, see INTEGRATION.md.
//
//   deploy_render:  make_scene + make_integrator        -> rrt_scene_load (host: loader, OBJ parser, BVH build, camera init)
//                   inte.render(&scene)                 -> rrt_create + rrt_render_bands_begin on every GPU this process owns,
//                                                          rrt_film_gather_all (RCCL; nothing to do on one GPU) to device 0
//                   film.write_image -> write_image     -> rrt_resolve_rgba8 + rrt_write_png
// Diagnostics go to stderr like the reference's eprintln!; its "N rays generated" line (integrator/mod.rs:137) goes to stdout.
// Environment: RRT_GPUS = number of GPUs to partition the film over (default 1), RRT_PRECISION = f32 (default) | f64,
// RRT_FIXED_BVH = 1 builds pbrt's intended tree instead of the reference's (quirks Q26 / Q27),
// RRT_AOV = <prefix> writes the first-hit feature buffers after the frame (rrt_render_aov, on device 0 alone): <prefix>_albedo.png,
// <prefix>_normal.png (n * 0.5 + 0.5) and <prefix>_depth.png (mean depth scaled to its own min .. max),
// RRT_DENOISE = <path.png> writes the denoised frame beside the ordinary one: rrt_render_aov with max_samples 32 on device 0, then rrt_denoise
// (default parameters) over the gathered film,
// RRT_DENOISE_MOMENTS = 1 (any value but "" and "0") beside RRT_DENOISE (one GPU): the frame is rendered by rrt_render_moments - the same film, bit for bit, so the ordinary
// PNG is unchanged - and the denoised frame comes from rrt_denoise_moments under the frame's sample-variance plane. That frame and the planes of
// its first 32 samples come from one call, rrt_render_frame_aov: the same bits as rrt_render_moments followed by rrt_render_aov, one camera pass less.
// RRT_AOV_FOLLOW = <n> (1..16) makes RRT_AOV and RRT_DENOISE take their planes from rrt_render_aov_follow(max_follow = n): the feature buffers of the
// first non-specular surface behind mirrors and smooth glass. With RRT_DENOISE_MOMENTS that is rrt_render_moments followed by that call.
// RRT_AO = <path.png> writes the resolved ambient occlusion as grey after the frame (rrt_render_ao, on device 0 alone): the mean of a / pi over the
// hit samples; RRT_AO_SAMPLES sets n_samples (default: rrt_ao_defaults), RRT_AO_SPP max_samples (default 0: every sample of the frame).
// RRT_PASSES = <prefix> writes light-group and bounce passes after the frame (rrt_render_passes, on device 0 alone): <prefix>_direct.png (path vertex 0),
// <prefix>_indirect.png (vertices >= 1) and <prefix>_light<i>.png for the first 14 lights, each light its own group; Path integrator only.
// RRT_MATTES = <path.png> writes one preview image of the ID mattes after the frame (rrt_render_mattes, on device 0 alone): per pixel the ids' hash
// colours weighted by their coverage shares; RRT_MATTE_BY = material | instance | object (default) chooses the ids, RRT_MATTE_SLOTS (default 6) the
// slots per pixel.
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "rrt.h"

namespace {
int fail(const char* what, int rc) {
  std::fprintf(stderr, "rrt_render: %s failed (%d): %s\n", what, rc, rrt_last_error());
  return rc == RRT_EPANIC ? 101 : 1;   // a Rust panic exits with 101
}

// the sums of rrt_render_aov (rrt_aov in rrt.h) -> three 8-bit images
template <typename R>
int write_aov(rrt_handle* h, int precision, int W, int H, uint32_t follow, const std::string& prefix) {
  const size_t npx = (size_t)W * (size_t)H;
  std::vector<R> alb(4 * npx, R(0)), nrm(4 * npx, R(0)), dep(4 * npx, R(0));
  rrt_aov out{RRT_MEM_HOST, precision, alb.data(), nrm.data(), dep.data()};
  const int32_t rect[4] = {0, 0, W, H};
  int rc = follow > 0 ? rrt_render_aov_follow(h, rect, 0, 1, 0, follow, &out) : rrt_render_aov(h, rect, 0, 1, 0, &out);
  if (rc != RRT_OK) return rc;
  double dmin = INFINITY, dmax = -INFINITY;
  for (size_t i = 0; i < npx; i++)
    if (dep[4 * i + 2] != R(0)) { const double d = (double)dep[4 * i] / (double)dep[4 * i + 2]; dmin = std::min(dmin, d); dmax = std::max(dmax, d); }
  auto q = [](double v) { return (uint8_t)std::min(255.0, std::max(0.0, (v == v ? v : 0.0) * 255.0 + 0.5)); };
  std::vector<uint8_t> img[3];
  for (auto& im : img) im.assign(4 * npx, 255);
  for (size_t i = 0; i < npx; i++) {
    const double w_live = (double)alb[4 * i + 3], w_hit = (double)dep[4 * i + 2];
    const double n[3] = {(double)nrm[4 * i], (double)nrm[4 * i + 1], (double)nrm[4 * i + 2]}, len = std::sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);
    const double grey = (w_hit != 0.0 && dmax > dmin) ? ((double)dep[4 * i] / w_hit - dmin) / (dmax - dmin) : 0.0;
    for (int c = 0; c < 3; c++) {
      img[0][4 * i + c] = q(w_live != 0.0 ? (double)alb[4 * i + c] / w_live : 0.0);
      img[1][4 * i + c] = q((w_hit != 0.0 && len > 0.0) ? n[c] / len * 0.5 + 0.5 : 0.0);
      img[2][4 * i + c] = q(grey);
    }
  }
  const char* names[3] = {"_albedo.png", "_normal.png", "_depth.png"};
  for (int k = 0; k < 3 && rc == RRT_OK; k++) rc = rrt_write_png((prefix + names[k]).c_str(), img[k].data(), W, H);
  return rc;
}

// the occlusion sums of rrt_render_ao (rrt_ao in rrt.h) -> one grey 8-bit image: the mean of a / pi over the hit samples, clipped to [0, 1]
template <typename R>
int write_ao(rrt_handle* h, int precision, int W, int H, uint64_t max_samples, int n_samples, const std::string& path) {
  const size_t npx = (size_t)W * (size_t)H;
  std::vector<R> ao(4 * npx, R(0));
  rrt_ao out{RRT_MEM_HOST, precision, ao.data(), nullptr};
  rrt_ao_params prm;
  rrt_ao_defaults(h, &prm);
  if (n_samples > 0) prm.n_samples = n_samples;
  const int32_t rect[4] = {0, 0, W, H};
  const int rc = rrt_render_ao(h, rect, 0, 1, max_samples, &prm, &out);
  if (rc != RRT_OK) return rc;
  std::vector<uint8_t> img(4 * npx, 255);
  for (size_t i = 0; i < npx; i++) {
    const double w_hit = (double)ao[4 * i + 2];
    const double v = w_hit != 0.0 ? std::min(1.0, std::max(0.0, (double)ao[4 * i] / w_hit / 3.14159265358979323846)) : 0.0;
    for (int c = 0; c < 3; c++) img[4 * i + c] = (uint8_t)std::min(255.0, std::max(0.0, (v == v ? v : 0.0) * 255.0 + 0.5));
  }
  return rrt_write_png(path.c_str(), img.data(), W, H);
}

// the pass films of rrt_render_passes -> 8-bit images: direct, indirect, and one per light for the first 14 lights (RRT_MAX_PASSES - 2)
template <typename R>
int write_passes(rrt_handle* h, int precision, int W, int H, double scale, size_t n_lights, const std::string& prefix) {
  const size_t npx = (size_t)W * (size_t)H;
  const size_t shown = std::min<size_t>(n_lights, RRT_MAX_PASSES - 2);
  if (n_lights > shown) std::fprintf(stderr, "rrt_render: RRT_PASSES writes the passes of the first %zu of the scene's %zu lights\n", shown, n_lights);
  std::vector<std::vector<R>> films(2 + shown, std::vector<R>(4 * npx, R(0)));
  std::vector<std::string> names = {"_direct.png", "_indirect.png"};
  std::vector<rrt_pass> passes = {{~0u, 0, 1, films[0].data()}, {~0u, 1, 0, films[1].data()}};
  std::vector<uint8_t> group(n_lights);
  for (size_t i = 0; i < n_lights; i++) group[i] = (uint8_t)std::min<size_t>(i, 31);   // (lights past the 31st share a group no pass here asks for alone)
  for (size_t i = 0; i < shown; i++) {
    passes.push_back({1u << i, 0, 0, films[2 + i].data()});
    names.push_back("_light" + std::to_string(i) + ".png");
  }
  const int32_t rect[4] = {0, 0, W, H};
  int rc = rrt_render_passes(h, rect, 0, 1, group.data(), passes.data(), (int)passes.size(), nullptr, RRT_MEM_HOST, nullptr);
  std::vector<uint8_t> rgba(4 * npx);
  for (size_t k = 0; k < passes.size() && rc == RRT_OK; k++) {
    rc = rrt_resolve_rgba8(films[k].data(), precision, W, H, scale, rgba.data());
    if (rc == RRT_OK) rc = rrt_write_png((prefix + names[k]).c_str(), rgba.data(), W, H);
  }
  return rc;
}

// one id per primitive, as Scene.prim_ids of the Python layer numbers them: "material" = material + 1, "instance" = instance + 2, "object" = 1 + the
// dense index of the distinct (instance, material) pairs in ascending order. False = an unknown key.
bool matte_prim_ids(const rrt_scene_desc* d, const std::string& by, std::vector<uint32_t>& ids) {
  ids.resize(d->n_prims);
  if (by == "material") { for (size_t i = 0; i < d->n_prims; i++) ids[i] = d->prims[i].material + 1u; return true; }
  if (by == "instance") { for (size_t i = 0; i < d->n_prims; i++) ids[i] = (uint32_t)(d->prims[i].instance + 2); return true; }
  if (by != "object") return false;
  std::vector<std::pair<int64_t, int64_t>> pairs(d->n_prims);
  for (size_t i = 0; i < d->n_prims; i++) pairs[i] = {(int64_t)d->prims[i].instance, (int64_t)d->prims[i].material};
  std::vector<std::pair<int64_t, int64_t>> uniq(pairs);
  std::sort(uniq.begin(), uniq.end());
  uniq.erase(std::unique(uniq.begin(), uniq.end()), uniq.end());
  for (size_t i = 0; i < d->n_prims; i++) ids[i] = 1u + (uint32_t)(std::lower_bound(uniq.begin(), uniq.end(), pairs[i]) - uniq.begin());
  return true;
}

// the table of rrt_render_mattes -> one 8-bit preview: per pixel sum_k colour(id_k) * coverage_k / weight[0], the slots added in stored order;
// colour(id) = the three low bytes of id * 2654435761 (mod 2^32), each / 255 (write_matte_png of the Python layer, operation by operation)
template <typename R>
int write_mattes(rrt_handle* h, int precision, int W, int H, const std::vector<uint32_t>& prim_id, int slots, const char* path) {
  const size_t npx = (size_t)W * (size_t)H, K = (size_t)slots;
  std::vector<uint32_t> ids(npx * K, 0u);
  std::vector<R> cov(npx * K, R(0)), wgt(4 * npx, R(0));
  rrt_mattes m{RRT_MEM_HOST, precision, slots, 0, ids.data(), cov.data(), wgt.data()};
  const int32_t rect[4] = {0, 0, W, H};
  int rc = rrt_render_mattes(h, rect, 0, 1, 0, prim_id.data(), prim_id.size(), &m);
  if (rc != RRT_OK) return rc;
  auto q = [](double v) { return (uint8_t)std::min(255.0, std::max(0.0, (v == v ? v : 0.0) * 255.0 + 0.5)); };
  std::vector<uint8_t> img(4 * npx, 255);
  for (size_t i = 0; i < npx; i++) {
    const double w0 = (double)wgt[4 * i];
    double rgb[3] = {0.0, 0.0, 0.0};
    for (size_t k = 0; k < K; k++) {
      const double share = w0 != 0.0 ? (double)cov[i * K + k] / w0 : 0.0;
      const uint32_t hash = ids[i * K + k] * 2654435761u;
      for (int c = 0; c < 3; c++) {
        const double colour = (double)((hash >> (8 * c)) & 0xffu) / 255.0;
        const double term = colour * share;   // (a statement of its own: a product that is rounded before it is added, as numpy rounds it)
        rgb[c] += term;
      }
    }
    for (int c = 0; c < 3; c++) img[4 * i + c] = q(rgb[c]);
  }
  return rrt_write_png(path, img.data(), W, H);
}

// the gathered film, filtered by rrt_denoise under the planes of at most 32 samples per pixel -> one 8-bit image. planes_dev: the three planes as
// rrt_render_frame_aov left them on device 0, one after the other; NULL = rendered here by rrt_render_aov
template <typename R>
int write_denoised(rrt_handle* h, int precision, int W, int H, double scale, const void* film, const void* moments /* NULL: rrt_denoise */, const void* planes_dev,
                   uint32_t follow, const char* path) {
  const size_t npx = (size_t)W * (size_t)H;
  std::vector<R> alb(4 * npx, R(0)), nrm(4 * npx, R(0)), dep(4 * npx, R(0)), out(4 * npx, R(0));
  rrt_aov aov{RRT_MEM_HOST, precision, alb.data(), nrm.data(), dep.data()};
  const int32_t rect[4] = {0, 0, W, H};
  int rc = RRT_OK;
  if (planes_dev) {
    R* dst[3] = {alb.data(), nrm.data(), dep.data()};
    for (int k = 0; k < 3; k++)
      if (hipMemcpy(dst[k], (const R*)planes_dev + (size_t)k * 4 * npx, 4 * npx * sizeof(R), hipMemcpyDeviceToHost) != hipSuccess) {
        std::fprintf(stderr, "rrt_render: feature plane copy-out failed\n");
        return RRT_EDEVICE;
      }
  } else rc = follow > 0 ? rrt_render_aov_follow(h, rect, 0, 1, 32, follow, &aov) : rrt_render_aov(h, rect, 0, 1, 32, &aov);
  if (rc == RRT_OK) rc = moments ? rrt_denoise_moments(h, film, &aov, moments, nullptr, out.data()) : rrt_denoise(h, film, &aov, nullptr, out.data());
  std::vector<uint8_t> rgba(4 * npx);
  if (rc == RRT_OK) rc = rrt_resolve_rgba8(out.data(), precision, W, H, scale, rgba.data());
  if (rc == RRT_OK) rc = rrt_write_png(path, rgba.data(), W, H);
  return rc;
}
}  // namespace

int main(int argc, char** argv) {
  if (argc != 3) {   // main.rs:56-59 indexes args[1], args[2]: fewer is an index panic there
    std::fprintf(stderr, "usage: %s <scene.json> <out.png>\n", argc > 0 ? argv[0] : "rrt_render");
    return 2;
  }
  const char* env_gpus = std::getenv("RRT_GPUS");
  const char* env_prec = std::getenv("RRT_PRECISION");
  const char* env_fix = std::getenv("RRT_FIXED_BVH");
  const int precision = (env_prec && std::strcmp(env_prec, "f64") == 0) ? RRT_F64 : RRT_F32;
  const uint32_t flags = (env_fix && std::atoi(env_fix) != 0) ? RRT_FIXED_BVH : 0u;
  int n_gpus = env_gpus ? std::atoi(env_gpus) : 1;
  const int visible = rrt_device_count();
  if (visible <= 0) { std::fprintf(stderr, "rrt_render: no HIP device visible (there is no CPU fallback)\n"); return 1; }
  if (n_gpus < 1) n_gpus = 1;
  if (n_gpus > visible) n_gpus = visible;

  rrt_scene* scene = nullptr;
  int rc = rrt_scene_load(argv[1], flags, 0x853C49E6748FEA9Bull, &scene);
  if (rc != RRT_OK) return fail("rrt_scene_load", rc);
  for (size_t i = 0; i < rrt_scene_warning_count(scene); i++) std::fprintf(stderr, "%s\n", rrt_scene_warning(scene, i));
  const rrt_scene_desc* desc = rrt_scene_desc_of(scene);   // handed to rrt_create as it is (RRT_ADAPTIVE reads its sample count)
  int32_t W = 0, H = 0;
  double film_scale = 1.0;
  (void)rrt_scene_film(scene, &W, &H, &film_scale);
  // RRT_ADAPTIVE=<threshold>: rrt_render_adaptive in the frame's place (RRT_ADAPTIVE_MIN, RRT_ADAPTIVE_BATCH: its min_samples and batch); film and
  // moments are consistent per pixel, so RRT_DENOISE / RRT_DENOISE_MOMENTS take them as they take a uniform frame's. Looked at before
  // RRT_DENOISE_MOMENTS: the adaptive frame is rendered on one GPU and has the plane. A value that is not a number is refused, not read as 0
  // (which would quietly give the uniform frame).
  const char* env_ad = std::getenv("RRT_ADAPTIVE");
  const bool adaptive = env_ad && *env_ad;
  rrt_adaptive_params adaptive_params;
  rrt_adaptive_defaults(&adaptive_params);
  if (adaptive) {
    char* end = nullptr;
    adaptive_params.threshold = std::strtod(env_ad, &end);
    bool ok = end != env_ad && *end == '\0';
    const char* env_min = std::getenv("RRT_ADAPTIVE_MIN");
    const char* env_batch = std::getenv("RRT_ADAPTIVE_BATCH");
    if (ok && env_min && *env_min) { const unsigned long v = std::strtoul(env_min, &end, 10); ok = end != env_min && *end == '\0' && v <= 0xfffffffful; adaptive_params.min_samples = (uint32_t)v; }
    if (ok && env_batch && *env_batch) { const unsigned long v = std::strtoul(env_batch, &end, 10); ok = end != env_batch && *end == '\0' && v <= 0xfffffffful; adaptive_params.batch = (uint32_t)v; }
    if (!ok) {
      std::fprintf(stderr, "rrt_render: RRT_ADAPTIVE, RRT_ADAPTIVE_MIN and RRT_ADAPTIVE_BATCH must be numbers (threshold, min_samples, batch)\n");
      rrt_scene_free(scene);
      return 2;
    }
    if (n_gpus > 1) {
      std::fprintf(stderr, "rrt_render: RRT_ADAPTIVE runs on one GPU: device 0 renders the whole frame\n");
      n_gpus = 1;
    }
  }
  const char* env_dn_path = std::getenv("RRT_DENOISE");
  const char* env_dn_mom = std::getenv("RRT_DENOISE_MOMENTS");
  bool with_moments = env_dn_path && *env_dn_path && env_dn_mom && *env_dn_mom && std::strcmp(env_dn_mom, "0") != 0;   // on for any value but "" and "0", as deploy_render reads it
  if (with_moments && n_gpus > 1) {
    std::fprintf(stderr, "rrt_render: RRT_DENOISE_MOMENTS runs on one GPU: the denoised frame keeps the spatial variance estimate\n");
    with_moments = false;
  }
  // RRT_AOV_FOLLOW=<n>: the planes of RRT_AOV / RRT_DENOISE through up to n specular bounces (rrt_render_aov_follow). Not a number: refused, not read as 0
  uint32_t follow = 0;
  if (const char* env_follow = std::getenv("RRT_AOV_FOLLOW"); env_follow && *env_follow) {
    char* end = nullptr;
    const unsigned long v = std::strtoul(env_follow, &end, 10);
    if (end == env_follow || *end != '\0' || v > 0xfffffffful) {
      std::fprintf(stderr, "rrt_render: RRT_AOV_FOLLOW must be a number (max_follow, 0..16)\n");
      rrt_scene_free(scene);
      return 2;
    }
    follow = (uint32_t)v;
  }
  const size_t word = precision == RRT_F32 ? 4 : 8, film_bytes = (size_t)W * (size_t)H * 4 * word;
  // the tiles banner of integrator/mod.rs:59-62
  std::fprintf(stderr, "Rendering %d x %d, %d tile rows of 16 over %d GPU(s)\n", W, H, (H + 15) / 16, n_gpus);

  std::vector<rrt_handle*> handles(n_gpus, nullptr);
  std::vector<void*> films(n_gpus, nullptr);
  void* moments_dev = nullptr;   // the sample-variance plane of device 0 (RRT_DENOISE_MOMENTS)
  void* planes_dev = nullptr;    // albedo, normal and depth planes of device 0, one after the other (rrt_render_frame_aov)
  auto cleanup = [&]() {
    if (moments_dev) { (void)hipSetDevice(0); (void)hipFree(moments_dev); }
    if (planes_dev) { (void)hipSetDevice(0); (void)hipFree(planes_dev); }
    for (int i = 0; i < n_gpus; i++) {
      if (handles[i]) rrt_destroy(handles[i]);
      if (films[i]) { (void)hipSetDevice(i); (void)hipFree(films[i]); }
    }
    rrt_scene_free(scene);
  };
  for (int i = 0; i < n_gpus; i++) {
    rc = rrt_create(i, desc, precision, &handles[i]);
    if (rc != RRT_OK) { const int e = fail("rrt_create", rc); cleanup(); return e; }
    if (i == 0) for (size_t k = 0; k < rrt_warning_count(handles[i]); k++) std::fprintf(stderr, "%s\n", rrt_warning(handles[i], k));
    if (hipSetDevice(i) != hipSuccess || hipMalloc(&films[i], film_bytes) != hipSuccess || hipMemset(films[i], 0, film_bytes) != hipSuccess) {
      std::fprintf(stderr, "rrt_render: cannot allocate the %zu-byte film on device %d\n", film_bytes, i);
      cleanup();
      return 1;
    }
  }
  unsigned long long rays_generated = 0;
  if (with_moments || adaptive) {   // one GPU: the whole frame and its moments plane in one call
    if (hipSetDevice(0) != hipSuccess || hipMalloc(&moments_dev, film_bytes) != hipSuccess || hipMemset(moments_dev, 0, film_bytes) != hipSuccess) {
      std::fprintf(stderr, "rrt_render: cannot allocate the %zu-byte moments plane on device 0\n", film_bytes);
      cleanup();
      return 1;
    }
    const int32_t rect[4] = {0, 0, W, H};
    rrt_render_stats st;
    if (adaptive) {
      rc = rrt_render_adaptive(handles[0], rect, &adaptive_params, films[0], moments_dev, nullptr, RRT_MEM_DEVICE, &st);
      if (rc != RRT_OK) { const int e = fail("rrt_render_adaptive", rc); cleanup(); return e; }
      const unsigned long long spp = desc->sampler.samples_per_pixel > 1 ? (unsigned long long)desc->sampler.samples_per_pixel - 1ull : 0ull;
      std::printf("%llu of %llu camera samples taken (adaptive)\n", (unsigned long long)st.camera_samples, (unsigned long long)W * (unsigned long long)H * spp);
    } else if (follow > 0) {   // the moments frame alone: the followed planes are rendered by write_denoised
      rc = rrt_render_moments(handles[0], rect, 0, 1, films[0], moments_dev, RRT_MEM_DEVICE, &st);
      if (rc != RRT_OK) { const int e = fail("rrt_render_moments", rc); cleanup(); return e; }
    } else {   // the frame, its moments plane and the denoiser's feature planes (at most 32 samples per pixel) from one camera pass
      if (hipMalloc(&planes_dev, 3 * film_bytes) != hipSuccess || hipMemset(planes_dev, 0, 3 * film_bytes) != hipSuccess) {
        std::fprintf(stderr, "rrt_render: cannot allocate the %zu-byte feature planes on device 0\n", 3 * film_bytes);
        cleanup();
        return 1;
      }
      unsigned char* pl = (unsigned char*)planes_dev;
      rrt_aov aov{RRT_MEM_DEVICE, precision, pl, pl + film_bytes, pl + 2 * film_bytes};
      rc = rrt_render_frame_aov(handles[0], rect, 0, 1, films[0], moments_dev, RRT_MEM_DEVICE, 32, &aov, &st);
      if (rc != RRT_OK) { const int e = fail("rrt_render_frame_aov", rc); cleanup(); return e; }
    }
    rays_generated = st.camera_rays;
  } else {
    // every GPU renders its interleaved bands at the same time (the calls only enqueue), then one collective, then wait
    for (int i = 0; i < n_gpus; i++) {
      rc = rrt_render_bands_begin(handles[i], i, n_gpus, films[i]);
      if (rc != RRT_OK) { const int e = fail("rrt_render_bands_begin", rc); cleanup(); return e; }
    }
    rc = rrt_film_gather_all(handles.data(), films.data(), n_gpus, 0);
    if (rc != RRT_OK) { const int e = fail("rrt_film_gather_all", rc); cleanup(); return e; }
    for (int i = n_gpus - 1; i >= 0; i--) {   // rank 0 last: its stream carries the receiving half of the collective
      rrt_render_stats st;
      rc = rrt_render_end_stats(handles[i], &st);
      if (rc != RRT_OK) { const int e = fail("rrt_render_end", rc); cleanup(); return e; }
      rays_generated += st.camera_rays;
    }
  }
  std::printf("%llu rays generated\n", rays_generated);   // integrator/mod.rs:137 (camera samples with weight > 0, over all tiles)
  std::vector<unsigned char> host(film_bytes), rgba((size_t)W * (size_t)H * 4);
  if (hipSetDevice(0) != hipSuccess || hipMemcpy(host.data(), films[0], film_bytes, hipMemcpyDeviceToHost) != hipSuccess) {
    std::fprintf(stderr, "rrt_render: film copy-out failed\n");
    cleanup();
    return 1;
  }
  rc = rrt_resolve_rgba8(host.data(), precision, W, H, film_scale, rgba.data());
  if (rc == RRT_OK) rc = rrt_write_png(argv[2], rgba.data(), W, H);
  if (rc != RRT_OK) { const int e = fail("write_image", rc); cleanup(); return e; }
  if (const char* env_aov = std::getenv("RRT_AOV"); env_aov && *env_aov) {
    if (n_gpus > 1) std::fprintf(stderr, "rrt_render: RRT_AOV runs on one GPU: the feature buffers are rendered on device 0 alone\n");
    rc = precision == RRT_F32 ? write_aov<float>(handles[0], precision, W, H, follow, env_aov) : write_aov<double>(handles[0], precision, W, H, follow, env_aov);
    if (rc != RRT_OK) { const int e = fail("rrt_render_aov", rc); cleanup(); return e; }
  }
  if (const char* env_ao = std::getenv("RRT_AO"); env_ao && *env_ao) {
    if (n_gpus > 1) std::fprintf(stderr, "rrt_render: RRT_AO runs on one GPU: the occlusion plane is rendered on device 0 alone\n");
    const char* env_n = std::getenv("RRT_AO_SAMPLES");
    const char* env_spp = std::getenv("RRT_AO_SPP");
    char *end_n = nullptr, *end_spp = nullptr;
    const long n = (env_n && *env_n) ? std::strtol(env_n, &end_n, 10) : 0, spp = (env_spp && *env_spp) ? std::strtol(env_spp, &end_spp, 10) : 0;
    if ((end_n && *end_n != '\0') || (end_spp && *end_spp != '\0') || n < 0 || n > 256 || spp < 0) {
      std::fprintf(stderr, "rrt_render: RRT_AO_SAMPLES must be a number (n_samples, 1..256), RRT_AO_SPP a number (max_samples)\n");
      cleanup();
      return 2;
    }
    rc = precision == RRT_F32 ? write_ao<float>(handles[0], precision, W, H, (uint64_t)spp, (int)n, env_ao) : write_ao<double>(handles[0], precision, W, H, (uint64_t)spp, (int)n, env_ao);
    if (rc != RRT_OK) { const int e = fail("rrt_render_ao", rc); cleanup(); return e; }
  }
  if (const char* env_ps = std::getenv("RRT_PASSES"); env_ps && *env_ps) {
    if (n_gpus > 1) std::fprintf(stderr, "rrt_render: RRT_PASSES runs on one GPU: the passes are rendered on device 0 alone\n");
    rc = precision == RRT_F32 ? write_passes<float>(handles[0], precision, W, H, film_scale, desc->n_lights, env_ps)
                              : write_passes<double>(handles[0], precision, W, H, film_scale, desc->n_lights, env_ps);
    if (rc != RRT_OK) { const int e = fail("rrt_render_passes", rc); cleanup(); return e; }
  }
  if (const char* env_mt = std::getenv("RRT_MATTES"); env_mt && *env_mt) {
    if (n_gpus > 1) std::fprintf(stderr, "rrt_render: RRT_MATTES runs on one GPU: the ID mattes are rendered on device 0 alone\n");
    const char* env_by = std::getenv("RRT_MATTE_BY");
    const char* env_slots = std::getenv("RRT_MATTE_SLOTS");
    std::vector<uint32_t> prim_id;
    char* end = nullptr;
    const long slots = (env_slots && *env_slots) ? std::strtol(env_slots, &end, 10) : 6;
    if (!matte_prim_ids(desc, (env_by && *env_by) ? env_by : "object", prim_id) || (end && *end != '\0') || slots < 1 || slots > RRT_MAX_MATTE_SLOTS) {
      std::fprintf(stderr, "rrt_render: RRT_MATTE_BY must be material, instance or object, RRT_MATTE_SLOTS a number (1..16)\n");
      cleanup();
      return 2;
    }
    const int k = (int)slots;
    rc = precision == RRT_F32 ? write_mattes<float>(handles[0], precision, W, H, prim_id, k, env_mt) : write_mattes<double>(handles[0], precision, W, H, prim_id, k, env_mt);
    if (rc != RRT_OK) { const int e = fail("rrt_render_mattes", rc); cleanup(); return e; }
  }
  if (const char* env_dn = env_dn_path; env_dn && *env_dn) {
    std::vector<unsigned char> host_moments;
    if (with_moments) {
      host_moments.resize(film_bytes);
      if (hipMemcpy(host_moments.data(), moments_dev, film_bytes, hipMemcpyDeviceToHost) != hipSuccess) {
        std::fprintf(stderr, "rrt_render: moments copy-out failed\n");
        cleanup();
        return 1;
      }
    }
    const void* mom = with_moments ? host_moments.data() : nullptr;
    rc = precision == RRT_F32 ? write_denoised<float>(handles[0], precision, W, H, film_scale, host.data(), mom, planes_dev, follow, env_dn)
                              : write_denoised<double>(handles[0], precision, W, H, film_scale, host.data(), mom, planes_dev, follow, env_dn);
    if (rc != RRT_OK) { const int e = fail(with_moments ? "rrt_denoise_moments" : "rrt_denoise", rc); cleanup(); return e; }
  }
  cleanup();
  return 0;
}
