// The Halton sampler's host tables (host/sampler_tables.cpp) checked on the CPU alone: host objects only, as prep_check.
//
// The kernels divide by multiply-high with the numbers this builder makes (device/dmath.hpp div_base: hd.magic of every base; halton_dim: hb.magic /
// hb.shift of every table block). A magic number that is off by a few units divides wrongly for about one index in 2^32 / error - no table of
// probes finds that (tests/test_sampler_shapes.py finds errors from a few hundred units up). But the quotient floor(a m / 2^k) is monotone in a and
// its error grows with a, so it is exact for every 32-bit a if and only if it is exact at the ends and at the last multiple of the divisor and the
// number before it: those are checked here, with the device's own 32-bit sequence, for all 1000 bases and every block. Then the tables themselves:
// every block's high part covers the largest index of the film, and entries of both parts (every 61st, the first and the last) are the digit
// loop's integers and its running f64 product.
//
//   sampler_tables_check <base_scale0> <base_scale1> <nsamp> ...      (triples; the permutation table is a fixed non-trivial one)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "scene_prep.hpp"

using namespace rrtd;

static int g_bad = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (g_bad++ < 20) { std::printf("FAILED %s: ", #cond); std::printf(__VA_ARGS__); std::printf("\n"); } } } while (0)

static uint32_t umulhi(uint32_t a, uint32_t b) { return (uint32_t)(((uint64_t)a * b) >> 32); }
static uint32_t div_magic(uint32_t a, uint32_t magic, uint32_t shift) { const uint32_t t = umulhi(magic, a); return (t + ((a - t) >> 1)) >> shift; }   // div_base()

static void check_divider(const char* what, uint32_t dim, uint32_t d, uint32_t magic, uint32_t shift) {
  const uint32_t top = 0xffffffffu / d;
  const uint32_t at[] = {0u, 1u, d - 1u, d, d + 1u, 2u * d - 1u, top * d - 1u, top * d, 0xffffffffu, 0x80000000u, 0x7fffffffu};
  for (uint32_t a : at) CHECK(div_magic(a, magic, shift) == a / d, "%s of dimension %u: %u / %u gives %u", what, dim, a, d, div_magic(a, magic, shift));
}

int main(int argc, char** argv) {
  if (argc < 4 || (argc - 1) % 3 != 0) { std::printf("usage: sampler_tables_check <base_scale0> <base_scale1> <nsamp> ...\n"); return 2; }
  std::vector<uint32_t> primes;
  for (uint32_t c = 2; primes.size() < 1000; c++) { bool p = true; for (uint32_t q = 2; q * q <= c; q++) if (c % q == 0) { p = false; break; } if (p) primes.push_back(c); }
  std::vector<uint16_t> perms;
  for (uint32_t c : primes) for (uint32_t k = 0; k < c; k++) perms.push_back((uint16_t)(c == 2 ? 1u - k : (k * 2u + 1u) % c));   // k -> 2 k + 1 (mod c): a permutation, perm[0] = 1
  const uint32_t cam_blocks[3] = {729u, 15625u, 16807u};
  for (int arg = 1; arg + 2 < argc; arg += 3) {
    const uint64_t s0 = std::strtoull(argv[arg], nullptr, 10), s1 = std::strtoull(argv[arg + 1], nullptr, 10), nsamp = std::strtoull(argv[arg + 2], nullptr, 10);
    rrt_scene_desc d;
    std::memset(&d, 0, sizeof d);
    d.sampler.type = RRT_SAMPLER_HALTON; d.sampler.samples_per_pixel = nsamp; d.sampler.base_scales[0] = (int64_t)s0; d.sampler.base_scales[1] = (int64_t)s1;
    d.sampler.sample_stride = s0 * s1; d.sampler.perms = perms.data(); d.sampler.n_perms = perms.size();
    const uint64_t max_index = s0 * s1 * nsamp;
    CHECK(s0 * s1 * (nsamp + 1) < (1ull << 32), "the host refuses this film: stride %llu, nsamp %llu", (unsigned long long)(s0 * s1), (unsigned long long)nsamp);
    const SamplerTables t = build_sampler_tables(&d, true, 64, cam_blocks, true);
    CHECK(t.hdims.size() == 1000, "%zu dimensions", t.hdims.size());
    uint32_t sum = 0;
    for (uint32_t dim = 0; dim < 1000; dim++) {
      const HaltonDim& hd = t.hdims[dim];
      CHECK(hd.base == primes[dim] && hd.perm_offset == sum && hd.inv == 1.0 / (double)primes[dim], "dimension %u: base %u, offset %u", dim, hd.base, hd.perm_offset);
      sum += primes[dim];
      check_divider("hd.magic", dim, hd.base, (uint32_t)hd.magic, (uint32_t)(hd.magic >> 32));
    }
    size_t n_tables = 0;
    for (uint32_t dim = 0; dim < t.blk.size(); dim++) {
      const HaltonBlk& hb = t.blk[dim];
      if (hb.block == 0) continue;
      n_tables++;
      const uint64_t b = primes[dim];
      const uint16_t* pm = perms.data() + t.hdims[dim].perm_offset;
      uint32_t low_digits = 0;
      { uint64_t p = 1; while (p < hb.block) { p *= b; low_digits++; } CHECK(p == hb.block && hb.block * b >= (1ull << 17) && hb.block < max_index, "dimension %u: block %u", dim, hb.block); }
      check_divider("hb.magic / hb.shift", dim, hb.block, hb.magic, hb.shift);
      // the high part reaches the largest index; the next table (or the end) bounds it
      uint64_t end = t.hi.size();
      for (uint32_t next = dim + 1; next < t.blk.size(); next++) if (t.blk[next].block) { end = t.blk[next].hi_off; break; }
      const uint64_t n_hi = end - hb.hi_off;
      CHECK(max_index / hb.block < n_hi && (size_t)hb.lo_off + hb.block <= t.lo.size() && (size_t)hb.hi_off + n_hi <= t.hi.size(), "dimension %u: %llu high entries for index %llu",
            dim, (unsigned long long)n_hi, (unsigned long long)max_index);
      for (uint32_t lo = 0; lo < hb.block; lo = (lo + 61 < hb.block || lo == hb.block - 1) ? lo + 61 : hb.block - 1) {
        uint64_t a = lo, rev = 0;
        for (uint32_t i = 0; i < low_digits; i++) { rev = rev * b + pm[a % b]; a /= b; }
        CHECK(t.lo[hb.lo_off + lo] == rev, "dimension %u: low entry %u", dim, lo);
      }
      for (uint64_t hi = 0; hi < n_hi; hi = (hi + 61 < n_hi || hi == n_hi - 1) ? hi + 61 : n_hi - 1) {
        uint64_t a = hi, rev = 0, pw = 1;
        volatile double ip = 1.0;
        for (uint32_t i = 0; i < low_digits; i++) ip = ip * t.hdims[dim].inv;
        while (a != 0) { rev = rev * b + pm[a % b]; a /= b; pw *= b; ip = ip * t.hdims[dim].inv; }
        const double ipv = ip;
        uint64_t bits; std::memcpy(&bits, &ipv, 8);
        const HaltonHi& e = t.hi[hb.hi_off + hi];
        CHECK(e.rev == rev && e.pw == pw && e.bits_lo == (uint32_t)bits && e.bits_hi == (uint32_t)(bits >> 32), "dimension %u: high entry %llu", dim, (unsigned long long)hi);
      }
    }
    std::printf("stride %llu, nsamp %llu: 1000 dividers, %zu block tables\n", (unsigned long long)(s0 * s1), (unsigned long long)nsamp, n_tables);
  }
  if (g_bad) { std::printf("sampler_tables_check: %d FAILED\n", g_bad); return 1; }
  std::printf("sampler_tables_check: ok\n");
  return 0;
}
