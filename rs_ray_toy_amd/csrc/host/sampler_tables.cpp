// Scene preparation, part 2: the Halton sampler's tables (see scene_prep.hpp). The f64 steps marked volatile replay the reference's running products
// operation by operation.
#include "scene_prep.hpp"

#include <algorithm>
#include <cstring>

namespace rrtd {

SamplerTables build_sampler_tables(const rrt_scene_desc* d, bool block_tables, int n_tab_dims, const uint32_t cam_blocks[3], bool cam_tables) {
  SamplerTables s;
  const uint32_t base_scale1 = (uint32_t)d->sampler.base_scales[1];
  std::vector<HaltonDim>& hd = s.hdims;
  hd.resize(1000);
  {
    int n = 0;
    uint32_t acc = 0;
    for (uint32_t c = 2; n < 1000; c++) {
      bool prime = true;
      for (uint32_t q = 2; q * q <= c; q++) if (c % q == 0) { prime = false; break; }
      if (prime) { hd[n].base = c; hd[n].perm_offset = acc; { uint32_t l = 0; while ((1ull << l) < c) l++; const uint64_t mp = ((1ull << 32) * ((1ull << l) - c)) / c + 1ull; hd[n].magic = (mp & 0xffffffffull) | ((uint64_t)(l - 1) << 32); } hd[n].inv = 1.0 / (double)c; acc += c; n++; }
    }
  }
  std::vector<uint16_t>& perms = s.perms;
  if (d->sampler.type == RRT_SAMPLER_HALTON && d->sampler.perms) perms.assign(d->sampler.perms, d->sampler.perms + d->sampler.n_perms);
  for (auto& h : hd) {   // lowdiscrepancy.rs:225: inv_base * perm[0] / (1 - inv_base), operation by operation
    h.tail = 0.0;
    if (h.perm_offset < perms.size()) {
      volatile double num = h.inv * (double)perms[h.perm_offset];
      volatile double den = 1.0 - h.inv;
      h.tail = num / den;
    }
  }
  { double v = 1.0; const double inv3 = hd[1].inv; for (int k = 0; k < 24; k++) { s.inv3pow[k] = v; v *= inv3; } }
  for (int w = 0; w < 2; w++) {   // lens dims 2, 3: bases hd[2].base = 5, hd[3].base = 7
    const uint32_t base = hd[2 + w].base;
    uint32_t packed = 0;
    const uint16_t* pm = perms.empty() ? nullptr : perms.data() + hd[2 + w].perm_offset;
    for (uint32_t dgt = 0; dgt < base && pm; dgt++) packed |= ((uint32_t)pm[dgt] & 7u) << (3u * dgt);
    s.cam_perm[w] = packed;
    const double inv_base = 1.0 / (double)base;
    double v = 1.0;
    for (int k = 0; k < 16; k++) { s.cam_invpow[w][k] = v; v *= inv_base; }
    s.cam_tail[w] = pm ? inv_base * (double)pm[0] / (1.0 - inv_base) : 0.0;
  }
  if (block_tables) {
    // block tables of the dimensions the integrators draw (SceneDev::hblk, halton_dim()): the first kHaltonTabDims dimensions, block =
    // the largest power of the base below 2^17 (a 0.5 MB table of low blocks at most), one entry per high part up to the largest sample index
    if (d->sampler.type == RRT_SAMPLER_HALTON && !perms.empty()) {
      const uint64_t max_index = std::min<uint64_t>(0xffffffffull, (uint64_t)d->sampler.sample_stride * (uint64_t)std::max<int64_t>(1, d->sampler.samples_per_pixel));
      std::vector<HaltonBlk>& blk = s.blk;
      blk.resize(n_tab_dims);
      std::vector<uint32_t>& lo_all = s.lo;
      std::vector<HaltonHi>& hi_all = s.hi;
      for (uint32_t dim = 0; dim < (uint32_t)n_tab_dims; dim++) {
        HaltonBlk& hb = blk[dim];
        std::memset(&hb, 0, sizeof(hb));
        if (dim < 2) continue;   // dimensions 0 and 1 are the pixel's (halton.rs:107-121)
        const uint32_t b = hd[dim].base;
        if (hd[dim].perm_offset + b > perms.size()) continue;
        const uint16_t* pm = perms.data() + hd[dim].perm_offset;
        uint32_t low_digits = 1; uint64_t block = b;
        while (block * b < (1ull << 17)) { block *= b; low_digits++; }
        if (block >= max_index) continue;
        { uint32_t l = 0; while ((1ull << l) < block) l++; const uint64_t mp = ((1ull << 32) * ((1ull << l) - block)) / block + 1ull; hb.magic = (uint32_t)mp; hb.shift = l - 1; }
        hb.block = (uint32_t)block; hb.lo_off = (uint32_t)lo_all.size(); hb.hi_off = (uint32_t)hi_all.size();
        for (uint32_t lo = 0; lo < hb.block; lo++) {
          uint32_t a = lo, rev = 0;
          for (uint32_t i = 0; i < low_digits; i++) { rev = rev * b + pm[a % b]; a /= b; }
          lo_all.push_back(rev);
        }
        const uint64_t n_hi = max_index / block + 2;
        for (uint64_t hi = 0; hi < n_hi; hi++) {
          uint64_t a = hi, rev = 0, pw = 1; uint32_t k = low_digits;
          while (a != 0) { rev = rev * b + pm[a % b]; a /= b; pw *= b; k++; }
          volatile double ip = 1.0;   // the loop's running product inv_base_n *= inv_base, k times (lowdiscrepancy.rs:204-227)
          for (uint32_t i = 0; i < k; i++) ip = ip * hd[dim].inv;
          const double ipv = ip;
          uint64_t bits; std::memcpy(&bits, &ipv, 8);
          hi_all.push_back(HaltonHi{(uint32_t)rev, (uint32_t)pw, (uint32_t)bits, (uint32_t)(bits >> 32)});
        }
      }
    }
  }
  if (block_tables) {
    // block tables of the camera dimensions' digit loops (SceneDev::cam_lo / cam_hi, halton_cam4()); every sample index is below stride * spp
    const uint64_t max_index = std::min<uint64_t>(0xffffffffull, (uint64_t)d->sampler.sample_stride * (uint64_t)std::max<int64_t>(1, d->sampler.samples_per_pixel));
    if (d->sampler.type == RRT_SAMPLER_HALTON && !perms.empty() && cam_tables) {
      const uint32_t bases[3] = {3u, 5u, 7u}, blocks[3] = {cam_blocks[0], cam_blocks[1], cam_blocks[2]}, low_digits[3] = {6u, 6u, 5u};
      const uint64_t top[3] = {max_index / std::max<uint32_t>(1u, base_scale1), max_index, max_index};   // dimension 1 digests index / 3^e
      std::vector<uint32_t>& lo_all = s.cam_lo;
      std::vector<HaltonHi>& hi_all = s.cam_hi;
      size_t* lo_off = s.cam_lo_off;
      size_t* hi_off = s.cam_hi_off;
      s.has_cam = true;
      for (int w = 0; w < 3; w++) {
        const uint32_t b = bases[w];
        const uint16_t* pm = w == 0 ? nullptr : perms.data() + hd[1 + w].perm_offset;   // dimension 1 is not scrambled (halton.rs:107-128)
        auto perm = [&](uint32_t dgt) { return pm ? (uint32_t)pm[dgt] & 7u : dgt; };
        lo_off[w] = lo_all.size(); hi_off[w] = hi_all.size();
        for (uint32_t lo = 0; lo < blocks[w]; lo++) {
          uint32_t a = lo, rev = 0;
          for (uint32_t i = 0; i < low_digits[w]; i++) { rev = rev * b + perm(a % b); a /= b; }
          lo_all.push_back(rev);
        }
        const uint64_t n_hi = top[w] / blocks[w] + 2;
        for (uint64_t hi = 0; hi < n_hi; hi++) {
          uint64_t a = hi, rev = 0, pw = 1; uint32_t kh = 0;
          while (a != 0) { rev = rev * b + perm((uint32_t)(a % b)); a /= b; pw *= b; kh++; }
          const double ip = w == 0 ? s.inv3pow[std::min<uint32_t>(23u, low_digits[w] + kh)] : s.cam_invpow[w - 1][std::min<uint32_t>(15u, low_digits[w] + kh)];
          uint64_t bits; std::memcpy(&bits, &ip, 8);
          hi_all.push_back(HaltonHi{(uint32_t)rev, (uint32_t)pw, (uint32_t)bits, (uint32_t)(bits >> 32)});
        }
      }
    }
  }
  return s;
}

}  // namespace rrtd
