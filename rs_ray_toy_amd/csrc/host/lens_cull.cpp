// Lens cull table of the fp32 camera kernel (dtraverse_f32.hpp k_raygen_main_f32), built on the host at handle creation.
//
// What it decides. Whether a camera sample gets through the lens depends on (r_film, plx, ply) only: the lens is rotationally symmetric and
// sample_exit_pupil (camera.rs:505-513) rotates the pupil sample (plx, ply) - a lerp of p_lens inside the chosen exit-pupil box (Q6) - to the film
// point's polar angle. In the frame turned by that angle the film point is (r_film, 0, 0) and the rear point (plx, ply, rear_z). 69 % of the
// samples of config 4 die in the lens (Q5); the table lets the kernel drop most of them before any lens arithmetic, so that the workgroup's
// survivors can be packed into whole waves before the first interface instead of after the third.
//
// Domain and cells. r_film in [0, r_max) (r_max: the film extent's farthest corner), p_lens in [0.5, 1.5) per axis (Q5); kLcR x kLcX x kLcY cells,
// one table per exit-pupil box, because the box decides what (plx, ply) a p_lens stands for. Box 0 is used below r_film = diagonal / 2, box 63 at
// and above it; each table is built over the r cells its box can be chosen in (with a tolerance of 1e-4 relative around the switch) and one cell
// more on either side, the others stay alive.
//
// When a cell is dead. The f64 trace below (the reference's operation order, camera.rs:163-211, in the turned frame) runs at every corner of every
// cell, over the domain and one cell beyond it on each side; a cell is lattice-dead when none of its 8 corners gets through. A cell is marked dead
// only when it AND its 26 neighbours are lattice-dead (erosion by one cell). What that one cell of margin covers:
//   - the samples between lattice points: the set of passing samples is bounded by smooth surfaces (aperture circles and element rims seen through
//     smooth refractions, the critical angle), so a passing region that reaches into a dead cell would have to slip between the lattice points of a
//     3 x 3 x 3 block of cells; tests/test_lens_cull_table.py checks every dead cell on a lattice 4x denser than this one with an independent f64 trace,
//     and 4 M uniform random samples per lens against the table (a sliver thinner than a quarter cell), also on lenses of 2, 3, 5 and 64 interfaces;
//   - the kernel's cell index: floor(r_film * inv_dr) and floor((p_lens - 0.5) * 96) in fp32 are off by at most one ulp of the product, far below one
//     cell, so a sample is looked up in its own cell or a neighbour of it, and every neighbour of a dead cell is lattice-dead;
//   - the fp32 lean lens arithmetic (dtraverse_f32.hpp rg_begin_lean / rg_step_lean): it evaluates the trace of a sample displaced by its rounding.
//     The rotation by the polar angle (sin_t, cos_t from rcp(r_film), each within 2 ulp) turns the rear point by < 1e-6 of the pupil extent; the
//     interfaces add ~1e-7 relative each, and the lens does not amplify a displacement of the ray (calibrate_aux_margins() measures c_i = 0.3-0.5
//     per interface for the scene.json lens), so 13 interfaces move the verdict's argument by < 1e-5 of the pupil extent, while a cell is 1 / 96
//     of the box (and 1 / 32 of r_max). The margin exceeds the arithmetic's displacement by about three orders of magnitude.
// (The c_i quoted above are the scene.json lens's. The argument needs only that they are of order 1; on the hand-built prescriptions of tests/lens_shapes.py -
// a strong singlet with total internal reflection inside the rim among them - the table changed no bit either.)
// The GPU side of the promise is tests/test_lens_cull.py and tests/test_lens_shapes.py: frames, weights and counters bit-identical with and without the table.
#include "lens_cull.hpp"

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <exception>
#include <mutex>
#include <thread>

namespace rrtd {
namespace {
struct V { double x, y, z; };
V nrm(V v) { const double l = std::sqrt(v.x * v.x + v.y * v.y + v.z * v.z); return l == 0.0 ? v : V{v.x / l, v.y / l, v.z / l}; }

// trace_lenses_from_film for the film point (rf, 0, 0) and the rear point (plx, ply, rear_z), f64, the reference's operation order; true = through
bool trace_through(const rrt_lens_elem* e, int n, double rf, double plx, double ply) {
  V o{rf, 0.0, 0.0};
  V dir = nrm(V{plx - rf, ply, e[n - 1].thickness});
  dir.z = -dir.z;   // flip_z
  double element_z = 0.0;
  for (int i = n - 1; i >= 0; i--) {
    element_z -= e[i].thickness;
    double t;
    V nn{0, 0, 0};
    const bool is_stop = e[i].curvature_radius == 0.0;
    if (is_stop) {
      if (dir.z >= 0.0) return false;
      t = (element_z - o.z) / dir.z;
    } else {
      const double radius = e[i].curvature_radius, zc = element_z + radius;
      const V oc{o.x, o.y, o.z - zc};
      const double a = dir.x * dir.x + dir.y * dir.y + dir.z * dir.z, b = 2.0 * (dir.x * oc.x + dir.y * oc.y + dir.z * oc.z), c = oc.x * oc.x + oc.y * oc.y + oc.z * oc.z - radius * radius;
      const double disc = b * b - 4.0 * a * c;
      if (disc < 0.0) return false;
      const double root = std::sqrt(disc), q = b < 0.0 ? -0.5 * (b - root) : -0.5 * (b + root);
      const double t0 = q / a, t1 = c / q;
      const bool use_closer = (dir.z > 0.0) ^ (radius < 0.0);
      t = use_closer ? std::fmin(t0, t1) : std::fmax(t0, t1);
      if (t < 0.0) return false;
      nn = nrm(V{oc.x + dir.x * t, oc.y + dir.y * t, oc.z + dir.z * t});
      if (nn.x * -dir.x + nn.y * -dir.y + nn.z * -dir.z < 0.0) nn = V{-nn.x, -nn.y, -nn.z};
    }
    if (!(t >= 0.0)) return false;
    const V ph{o.x + dir.x * t, o.y + dir.y * t, o.z + dir.z * t};
    if (ph.x * ph.x + ph.y * ph.y >= e[i].aperture_radius * e[i].aperture_radius) return false;
    o = ph;
    if (!is_stop) {
      const double eta_t = (i > 0 && e[i - 1].eta != 0.0) ? e[i - 1].eta : 1.0, eta = e[i].eta / eta_t;
      const V wi = nrm(V{-dir.x, -dir.y, -dir.z});
      const double cos_i = nn.x * wi.x + nn.y * wi.y + nn.z * wi.z, sin2_t = eta * eta * std::fmax(0.0, 1.0 - cos_i * cos_i);
      if (sin2_t >= 1.0) return false;
      const double cos_tt = std::sqrt(1.0 - sin2_t), k = eta * cos_i - cos_tt;
      dir = V{-wi.x * eta + nn.x * k, -wi.y * eta + nn.y * k, -wi.z * eta + nn.z * k};
    }
  }
  return true;
}
}  // namespace

LensCull build_lens_cull(const rrt_scene_desc* d) {
  const auto t0 = std::chrono::steady_clock::now();
  LensCull out;
  const int n = d->camera.n_elems;
  const rrt_film& f = d->film;
  double r_max = 0.0;
  for (int cx : {0, 2}) for (int cy : {1, 3}) r_max = std::max(r_max, std::hypot(f.physical_extent[cx], f.physical_extent[cy]));
  r_max *= 1.0 + 1e-6;
  if (n <= 0 || !(r_max > 0.0) || !std::isfinite(r_max) || !(f.diagonal > 0.0)) return out;
  out.r_max = r_max;
  out.inv_dr = (float)(kLcR / r_max);
  const double dr = r_max / kLcR, r_switch = f.diagonal / 2.0;
  // lattice points i = -1 .. N + 1 per axis (cell c spans points c and c + 1; cells -1 and N lie beyond the domain, for the erosion)
  constexpr int PR = kLcR + 3, PX = kLcX + 3, PY = kLcY + 3;
  constexpr int CR = kLcR + 2, CX = kLcX + 2, CY = kLcY + 2;   // cells -1 .. N
  std::vector<uint8_t> lat_dead[2], cell_dead[2];
  int cr_lo[2], cr_hi[2];   // computed cells of each box (inclusive, -1 .. kLcR)
  for (int b = 0; b < 2; b++) {
    // cells the box can be chosen in (r_film / (diagonal / 2) >= 1 picks box 63; a tolerance of 1e-4 around the switch for the fp32 comparison), one more each side
    int lo = kLcR, hi = -1;
    for (int c = 0; c < kLcR; c++) {
      const double a = c * dr, z = (c + 1) * dr;
      const bool used = b == 0 ? a < r_switch * (1.0 + 1e-4) : z > r_switch * (1.0 - 1e-4);
      if (used) { lo = std::min(lo, c); hi = std::max(hi, c); }
    }
    cr_lo[b] = lo - 1; cr_hi[b] = hi + 1;
    lat_dead[b].assign((size_t)PR * PX * PY, 0u);
    cell_dead[b].assign((size_t)CR * CX * CY, 0u);
  }
  // f64 lattice traces, one r plane of one box per work item, up to 16 threads (a GPU process's share of the host)
  struct Item { int b, ir; };
  std::vector<Item> items;
  for (int b = 0; b < 2; b++)
    if (cr_lo[b] <= cr_hi[b])
      for (int ir = cr_lo[b] + 1; ir <= cr_hi[b] + 2; ir++) items.push_back(Item{b, ir});   // point index ir: r = (ir - 1) dr; cells lo .. hi use points lo .. hi + 1
  std::atomic<size_t> next{0};
  std::atomic<uint64_t> traces{0};
  std::exception_ptr failed;
  std::mutex failed_mu;
  auto work = [&]() {
    try {
      for (;;) {
        const size_t k = next.fetch_add(1);
        if (k >= items.size()) break;
        const Item it = items[k];
        const double* pb = d->camera.exit_pupil_bounds[it.b == 0 ? 0 : 63];
        const double rf = (it.ir - 1) * dr;
        uint8_t* plane = &lat_dead[it.b][(size_t)it.ir * PX * PY];
        for (int ix = 0; ix < PX; ix++) {
          const double lx = 0.5 + (double)(ix - 1) / kLcX, plx = pb[0] * (1.0 - lx) + pb[2] * lx;
          for (int iy = 0; iy < PY; iy++) {
            const double ly = 0.5 + (double)(iy - 1) / kLcY, ply = pb[1] * (1.0 - ly) + pb[3] * ly;
            plane[(size_t)ix * PY + iy] = trace_through(d->camera.elems, n, rf, plx, ply) ? 0u : 1u;
          }
        }
        traces += (uint64_t)PX * PY;
      }
    } catch (...) { std::lock_guard<std::mutex> lk(failed_mu); if (!failed) failed = std::current_exception(); }
  };
  {
    const unsigned hw = std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
    std::vector<std::thread> pool;
    for (unsigned t = 1; t < hw && t < items.size(); t++) pool.emplace_back(work);
    work();
    for (auto& th : pool) th.join();
    if (failed) std::rethrow_exception(failed);
  }
  out.traces = traces.load();
  // lattice-dead cells (all 8 corners dead), then the erosion
  auto L = [&](int b, int ir, int ix, int iy) { return lat_dead[b][((size_t)ir * PX + ix) * PY + iy]; };   // point indices (offset by 1)
  auto C = [&](int b, int cr, int cx, int cy) -> uint8_t& { return cell_dead[b][((size_t)(cr + 1) * CX + (cx + 1)) * CY + (cy + 1)]; };   // cell indices -1 .. N
  for (int b = 0; b < 2; b++)
    for (int cr = std::max(-1, cr_lo[b]); cr <= std::min(kLcR, cr_hi[b]); cr++)
      for (int cx = -1; cx <= kLcX; cx++)
        for (int cy = -1; cy <= kLcY; cy++) {
          bool dead = true;
          for (int q = 0; q < 8 && dead; q++) dead = L(b, cr + 1 + (q & 1), cx + 1 + ((q >> 1) & 1), cy + 1 + (q >> 2)) != 0u;
          C(b, cr, cx, cy) = dead ? 1u : 0u;
        }
  out.bits.assign(kLcTableWords, 0u);
  uint64_t n_dead = 0, n_cells = 0;
  for (int b = 0; b < 2; b++)
    for (int cr = std::max(0, cr_lo[b] + 1); cr <= std::min(kLcR - 1, cr_hi[b] - 1); cr++)   // the cells the box can be chosen in
      for (int cy = 0; cy < kLcY; cy++)
        for (int cx = 0; cx < kLcX; cx++) {
          n_cells++;
          bool dead = true;
          for (int q = 0; q < 27 && dead; q++) dead = C(b, cr + q % 3 - 1, cx + (q / 3) % 3 - 1, cy + q / 9 - 1) != 0u;
          if (!dead) continue;
          n_dead++;
          out.bits[(((size_t)b * kLcR + cr) * kLcY + cy) * kLcWords + (size_t)(cx >> 5)] |= 1u << (cx & 31);
        }
  out.dead_share = n_cells ? (double)n_dead / (double)n_cells : 0.0;
  out.seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  return out;
}
}  // namespace rrtd

// Test and timing hook (NOT part of include/rrt.h; tests/test_lens_cull_table.py binds it with ctypes): the table of a scene desc's lens on the CPU alone.
// bits: kLcTableWords words; info: {r_max, inv_dr, dead share, traces, seconds}. Returns 0, or 1 when the lens gets no table (bits untouched).
extern "C" __attribute__((visibility("default"))) int rrt_internal_lens_cull(const rrt_scene_desc* d, uint32_t* bits, double* info) {
  if (!d || !bits || !info) return 2;
  const rrtd::LensCull lc = rrtd::build_lens_cull(d);
  if (lc.bits.empty()) return 1;
  std::copy(lc.bits.begin(), lc.bits.end(), bits);
  info[0] = lc.r_max; info[1] = lc.inv_dr; info[2] = lc.dead_share; info[3] = (double)lc.traces; info[4] = lc.seconds;
  return 0;
}
