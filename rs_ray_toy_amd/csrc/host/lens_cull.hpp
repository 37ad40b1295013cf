// Lens cull table of the fp32 camera kernel: host builder (plain C++, no HIP) - see lens_cull.cpp for the derivation.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#include "rrt.h"

namespace rrtd {
// cells over (r_film, lens sample x, lens sample y): r_film in [0, r_max), p_lens in [0.5, 1.5) (Q5) per axis
constexpr int kLcR = 32, kLcX = 96, kLcY = 96;
constexpr int kLcWords = (kLcX + 31) / 32;   // 32-bit words of one (box, r, y) row; bit x set = dead cell
constexpr size_t kLcTableWords = (size_t)2 * kLcR * kLcY * kLcWords;   // box 0 = exit_pupil_bounds[0], box 1 = exit_pupil_bounds[63] (Q6)

struct LensCull {
  std::vector<uint32_t> bits;   // [2][kLcR][kLcY][kLcWords]; empty: no table (the kernel culls nothing)
  float inv_dr = 0.0f;          // kLcR / r_max: r cell = floor(r_film * inv_dr)
  double r_max = 0.0;
  double dead_share = 0.0;      // dead cells / cells, over the cells the kernel can look up
  uint64_t traces = 0;          // f64 lattice traces run by the builder
  double seconds = 0.0;
};
LensCull build_lens_cull(const rrt_scene_desc* d);
}  // namespace rrtd
