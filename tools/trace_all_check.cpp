// trace_all_check: the rrt_trace_all walk (rs_ray_toy_amd/csrc/host/multihit.hpp multihit_walk - the code the kernel k_trace_all runs) on the CPU alone,
// compared bit for bit - slots and counts - with the scan over all entries the call is defined as (multihit_scan: the same acceptance function).
// usage: trace_all_check [scene.json ...]   - exit status 0 = no difference. Built from the host objects only (make -C rs_ray_toy_amd/csrc trace_all_check);
// it can be built with the host sanitizers as it stands, which proves the stack, buffer and index logic without a device.
// Besides the scenes named on the command line (both precisions, every instance kept or flattened as the handle would have it) it walks two trees it makes
// itself: a root that is a single leaf, and a 96-deep one-sided chain. Every tree is walked with k = 1, 4 and 16 and a stack of exactly the tree's depth:
// a push past it is a failure. `count` is no input of the walk (nothing is pruned by t, so whether the caller asks for it changes no step): the walk's
// count is compared at every k, and the slots of k = 1 and 4 must be prefixes of those of k = 16.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <exception>
#include <limits>
#include <string>
#include <vector>

#include "multihit.hpp"
#include "rrt.h"
#include "scene_prep.hpp"

using namespace rrtd;

namespace {
int g_fail = 0;
std::string g_what;
void fail(const char* msg, size_t at) {
  if (g_fail++ < 20) fprintf(stderr, "trace_all_check: %s: %s (ray %zu)\n", g_what.c_str(), msg, at);
}

struct VecStack {   // bounds-checked: the walk itself refuses a push past stack_cap, this catches a walk that does not
  std::vector<uint32_t> a;
  bool overrun = false;
  void put(uint32_t i, uint32_t v) { if (i < a.size()) a[i] = v; else overrun = true; }
  uint32_t get(uint32_t i) { if (i < a.size()) return a[i]; overrun = true; return 0u; }
};
template <typename R>
struct VecHits {   // bounds-checked against the k of the call, not against kMaxHits
  std::vector<R> ts;
  std::vector<int32_t> ps;
  bool overrun = false;
  explicit VecHits(uint32_t k) : ts(k, R(-1)), ps(k, -7) {}
  R t(uint32_t s) { if (s < ts.size()) return ts[s]; overrun = true; return R(0); }
  int32_t prim(uint32_t s) { if (s < ps.size()) return ps[s]; overrun = true; return 0; }
  void set(uint32_t s, R t, int32_t p) { if (s < ts.size()) { ts[s] = t; ps[s] = p; } else overrun = true; }
};

template <typename R> bool same_bits(R a, R b) { return memcmp(&a, &b, sizeof(R)) == 0; }

template <typename R>
uint32_t tree_depth(const std::vector<Node<R>>& nodes) {
  if (nodes.empty()) return 0;
  uint32_t depth = 0;
  std::vector<std::pair<uint32_t, uint32_t>> todo{{0u, 1u}};
  while (!todo.empty()) {
    const auto [i, lvl] = todo.back(); todo.pop_back();
    depth = std::max(depth, lvl);
    if ((nodes[i].meta >> 2) == 0u) { todo.push_back({i + 1u, lvl + 1u}); todo.push_back({nodes[i].offset, lvl + 1u}); }
  }
  return depth;
}

template <typename R>
void check_tree(const std::vector<Node<R>>& nodes, const std::vector<Tri<R>>& tris, const std::vector<InstDev<R>>& insts, size_t n_random) {
  if (nodes.empty()) return;
  const Node<R>& root = nodes[0];
  double M = 0.0, ext = 0.0;
  bool kept = false;
  for (int k = 0; k < 3; k++) { M = std::max({M, std::fabs((double)root.bmin[k]), std::fabs((double)root.bmax[k])}); ext = std::max(ext, (double)root.bmax[k] - (double)root.bmin[k]); }
  for (const Tri<R>& t : tris) if (t.plane != kSphereMark && (t.material & kInstFlag)) {
    kept = true;
    const R* m = insts[(t.material >> 16) & 0x7fffu].m;
    for (const R* v : {t.p0, t.p1, t.p2}) for (int i = 0; i < 3; i++)
      M = std::max(M, std::fabs((double)m[4 * i] * v[0]) + std::fabs((double)m[4 * i + 1] * v[1]) + std::fabs((double)m[4 * i + 2] * v[2]) + std::fabs((double)m[4 * i + 3]));
  }
  const R delta = kept ? (R)((double)kMultihitPadUlps * (double)NnConst<R>::eps * M) : R(0);
  // rays {o, d, tmax, skip}: between uniform points of 1.5 x the root box; through interior points, edge midpoints and vertices of triangles (ties),
  // from a uniform point; axis-parallel ones (a zero direction component: NaN and infinite slab terms); every second ray with a finite tmax; every
  // fifth through-ray with the aimed-at entry skipped; four dead ones
  struct Ray { R o[3], d[3], tmax; int32_t skip; };
  std::vector<Ray> rays;
  uint64_t st = 0x9E3779B97F4A7C15ull;
  auto rnd = [&]() { st ^= st << 13; st ^= st >> 7; st ^= st << 17; return (double)(st >> 11) * (1.0 / 9007199254740992.0); };
  auto uniform = [&](double* p) {
    for (int k = 0; k < 3; k++) {
      const double c = 0.5 * ((double)root.bmin[k] + (double)root.bmax[k]), h = 0.75 * ((double)root.bmax[k] - (double)root.bmin[k]) + 1e-3;
      p[k] = c + h * (2.0 * rnd() - 1.0);
    }
  };
  auto add = [&](const double* o, const double* to, int32_t skip) {
    Ray r;
    for (int k = 0; k < 3; k++) { r.o[k] = (R)o[k]; r.d[k] = (R)(to[k] - o[k]); }
    r.tmax = (rays.size() & 1u) ? (R)(0.5 + 1.5 * rnd()) : NnConst<R>::inf;   // d is not normalised: the target is at t = 1
    r.skip = skip;
    rays.push_back(r);
  };
  for (size_t i = 0; i < n_random; i++) { double a[3], b[3]; uniform(a); uniform(b); add(a, b, -1); }
  const size_t step = std::max<size_t>(1, tris.size() / 150);
  for (size_t i = 0; i < tris.size(); i += step) {
    R va[3], vb[3], vc[3];
    if (!mh_vertices<R>(tris[i], insts.data(), va, vb, vc)) continue;
    const R* v[3] = {va, vb, vc};
    double o[3], to[3];
    const int32_t skip = (i / step) % 5 == 4 ? (int32_t)i : -1;
    uniform(o); for (int k = 0; k < 3; k++) to[k] = 0.5 * v[0][k] + 0.25 * v[1][k] + 0.25 * v[2][k];
    add(o, to, skip);
    for (int j = 0; j < 3; j++) {
      uniform(o); for (int k = 0; k < 3; k++) to[k] = 0.5 * ((double)v[j][k] + (double)v[(j + 1) % 3][k]);
      add(o, to, -1);
      uniform(o); for (int k = 0; k < 3; k++) to[k] = v[j][k];
      add(o, to, -1);
    }
    // axis-parallel through the first vertex: two direction components are exactly 0
    for (int k = 0; k < 3; k++) { o[k] = v[0][k]; to[k] = v[0][k]; }
    o[i % 3] = (double)root.bmin[i % 3] - 0.25 * ext - 1.0;
    add(o, to, -1);
  }
  {
    double a[3], b[3]; uniform(a); uniform(b);
    add(a, b, -1); rays.back().o[0] = std::numeric_limits<R>::quiet_NaN();
    add(a, b, -1); rays.back().d[1] = NnConst<R>::inf;
    add(a, a, -1);                                                              // zero direction
    add(a, b, -1); rays.back().tmax = std::numeric_limits<R>::quiet_NaN();
  }
  const uint32_t depth = tree_depth(nodes);
  VecStack stack;
  stack.a.resize(depth);
  size_t n_hits = 0, n_over = 0, n_dead = 0;
  uint32_t most = 0;
  const uint32_t ks[3] = {16u, 4u, 1u};
  for (size_t i = 0; i < rays.size(); i++) {
    const Ray& q = rays[i];
    MhRay<R> r;
    const bool live = mh_make_ray<R>(q.o[0], q.o[1], q.o[2], q.d[0], q.d[1], q.d[2], q.tmax, &r);
    if (!live) { n_dead++; continue; }
    VecHits<R> wide(16);
    uint32_t wide_count = 0;
    for (const uint32_t k : ks) {
      VecHits<R> scan(k), walk(k);
      const uint32_t c_scan = multihit_scan<R>(tris.data(), (uint32_t)tris.size(), insts.data(), r, q.skip, scan, k);
      uint32_t c_walk = 0;
      if (!multihit_walk<R>(nodes.data(), (uint32_t)nodes.size(), tris.data(), (uint32_t)tris.size(), insts.data(), r, q.skip, delta, stack, depth, walk, k, &c_walk)) { fail("the walk passed a bound", i); continue; }
      if (stack.overrun) { fail("the walk left its stack", i); stack.overrun = false; }
      if (scan.overrun || walk.overrun) fail("an insert left its buffer", i);
      if (c_scan != c_walk) fail("walk and scan count differently", i);
      const uint32_t held = std::min(c_scan, k);
      for (uint32_t s = 0; s < held; s++) {
        if (scan.ps[s] != walk.ps[s] || !same_bits(scan.ts[s], walk.ts[s])) fail("walk and scan differ in a slot", i);
        if (s > 0 && !(scan.ts[s - 1] < scan.ts[s] || (scan.ts[s - 1] == scan.ts[s] && scan.ps[s - 1] < scan.ps[s]))) fail("slots out of order", i);
        if (q.skip >= 0 && scan.ps[s] == q.skip) fail("the skipped entry was reported", i);
        const MhHit<R> h = mh_rehit<R>(r, tris[scan.ps[s]], insts.data());
        if (!same_bits(h.t, scan.ts[s])) fail("the triangle test run again gives another t", i);
      }
      if (k == 16u) { wide = walk; wide_count = c_walk; n_hits += held; most = std::max(most, c_walk); if (c_walk > 16u) n_over++; }
      else {
        if (c_walk != wide_count) fail("count depends on k", i);
        for (uint32_t s = 0; s < held; s++) if (walk.ps[s] != wide.ps[s] || !same_bits(walk.ts[s], wide.ts[s])) fail("slots of a smaller k are no prefix", i);
      }
    }
  }
  printf("  %s (%s): %zu nodes, depth %u, %zu entries, %zu rays (%zu dead) x k = 16, 4, 1: %zu hits in the slots, at most %u per ray, %zu rays with more than 16\n", g_what.c_str(),
         sizeof(R) == 4 ? "f32" : "f64", nodes.size(), depth, tris.size(), rays.size(), n_dead, n_hits, most, n_over);
  if (n_hits == 0) fail("no ray hit anything", 0);
}

template <typename R>
void check_flat(const rrt_scene_desc* d) {
  const FlatScene<R> fs = flatten_scene<R>(d, 0.0);
  bool any = false;
  for (const Tri<R>& t : fs.tris) any |= t.plane != kSphereMark;
  if (!any) { printf("  %s: no triangle entry (RRT_EUNSUP)\n", g_what.c_str()); return; }
  check_tree<R>(fs.nodes, fs.tris, fs.insts, fs.tris.size() > 20000 ? 100 : 400);
}

void check_scene(const char* path) {
  rrt_scene* sc = nullptr;
  g_what = path;
  if (rrt_scene_load(path, RRT_FIXED_BVH, 0, &sc) != RRT_OK) { fprintf(stderr, "trace_all_check: %s: %s\n", path, rrt_last_error()); g_fail++; return; }
  const rrt_scene_desc* d = rrt_scene_desc_of(sc);
  validate_desc(d);
  check_flat<double>(d);
  check_flat<float>(d);
  rrt_scene_free(sc);
}

// tools/nearest_check.cpp's hand-built shapes, stacked along z as well so that a ray meets several: n leaves of one triangle each, a one-sided chain in pre-order
template <typename R>
void check_hand_built(int n_leaves, const char* name) {
  g_what = name;
  std::vector<Node<R>> nodes;
  std::vector<Tri<R>> tris((size_t)n_leaves);
  for (int i = 0; i < n_leaves; i++) {
    Tri<R>& t = tris[i];
    memset(&t, 0, sizeof(t));
    const R x = (R)0.125 * (R)(i % 4);
    t.p0[0] = x; t.p1[0] = x + (R)4; t.p2[0] = x; t.p2[1] = (R)4; t.p0[2] = t.p1[2] = t.p2[2] = (R)0.25 * (R)i;
    t.shade = 0xffffffffu; t.plane = (uint32_t)i;
  }
  auto leaf = [&](int i) {
    Node<R> n{};
    for (int k = 0; k < 3; k++) { n.bmin[k] = std::fmin(tris[i].p0[k], std::fmin(tris[i].p1[k], tris[i].p2[k])); n.bmax[k] = std::fmax(tris[i].p0[k], std::fmax(tris[i].p1[k], tris[i].p2[k])); }
    n.offset = (uint32_t)i; n.meta = 1u << 2;
    return n;
  };
  for (int i = 0; i + 1 < n_leaves; i++) { Node<R> n{}; n.offset = (uint32_t)(2 * i + 2); n.meta = (uint32_t)(i % 3); nodes.push_back(n); nodes.push_back(leaf(i)); }
  nodes.push_back(leaf(n_leaves - 1));
  for (int i = (int)nodes.size() - 1; i >= 0; i--) if ((nodes[i].meta >> 2) == 0u) {
    const Node<R>&a = nodes[i + 1], &b = nodes[nodes[i].offset];
    for (int k = 0; k < 3; k++) { nodes[i].bmin[k] = std::fmin(a.bmin[k], b.bmin[k]); nodes[i].bmax[k] = std::fmax(a.bmax[k], b.bmax[k]); }
  }
  check_tree<R>(nodes, tris, std::vector<InstDev<R>>(), 400);
}
}  // namespace

int main(int argc, char** argv) {
  try {
    for (int i = 1; i < argc; i++) { printf("%s\n", argv[i]); check_scene(argv[i]); }
    printf("hand-built trees\n");
    check_hand_built<float>(1, "single-leaf root"); check_hand_built<double>(1, "single-leaf root");
    check_hand_built<float>(96, "96-deep chain"); check_hand_built<double>(96, "96-deep chain");
  } catch (const std::exception& e) {
    fprintf(stderr, "trace_all_check: %s: exception: %s\n", g_what.c_str(), e.what());
    return 2;
  }
  if (g_fail) { fprintf(stderr, "trace_all_check: %d check(s) failed\n", g_fail); return 1; }
  printf("trace_all_check: ok\n");
  return 0;
}
