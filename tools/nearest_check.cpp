// nearest_check: the rrt_nearest walk (rs_ray_toy_amd/csrc/host/nearest.hpp nearest_walk - the code the generic kernel k_nearest runs) on the CPU
// alone, compared bit for bit with a scan over all triangles by the same per-triangle function.
// usage: nearest_check [scene.json ...]   - exit status 0 = no difference. Built from the host objects only (make -C rs_ray_toy_amd/csrc nearest_check); it can be
// built with the host sanitizers as it stands, which proves the stack and index logic without a device.
// Besides the scenes named on the command line (both precisions, every instance kept or flattened as the handle would have it) it walks two trees it makes
// itself: a root that is a single leaf, and a 96-deep one-sided chain. Every tree is walked with an unlimited search radius and with two finite ones, and
// with a stack of exactly the tree's depth: a push past it is a failure.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <exception>
#include <limits>
#include <string>
#include <vector>

#include "nearest.hpp"
#include "rrt.h"
#include "scene_prep.hpp"

using namespace rrtd;

namespace {
int g_fail = 0;
std::string g_what;
void fail(const char* msg, size_t at) {
  if (g_fail++ < 20) fprintf(stderr, "nearest_check: %s: %s (point %zu)\n", g_what.c_str(), msg, at);
}

struct VecStack {   // bounds-checked: the walk itself refuses a push past stack_cap, this catches a walk that does not
  std::vector<uint32_t> a;
  bool overrun = false;
  void put(uint32_t i, uint32_t v) { if (i < a.size()) a[i] = v; else overrun = true; }
  uint32_t get(uint32_t i) { if (i < a.size()) return a[i]; overrun = true; return 0u; }
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

// the world-space vertices of entry i as the kernels form them (for the query points only)
template <typename R>
bool world_vertices(const Tri<R>& t, const std::vector<InstDev<R>>& insts, R v[3][3]) {
  if (t.plane == kSphereMark) return false;
  const R* src[3] = {t.p0, t.p1, t.p2};
  for (int j = 0; j < 3; j++) for (int k = 0; k < 3; k++) v[j][k] = src[j][k];
  if (t.material & kInstFlag) {
    const R* m = insts[(t.material >> 16) & 0x7fffu].m;
    for (int j = 0; j < 3; j++) {
      const R x = v[j][0], y = v[j][1], z = v[j][2];
      for (int k = 0; k < 3; k++) v[j][k] = ((m[4 * k] * x + m[4 * k + 1] * y) + m[4 * k + 2] * z) + m[4 * k + 3];
    }
  }
  return true;
}

template <typename R>
void check_tree(const std::vector<Node<R>>& nodes, const std::vector<Tri<R>>& tris, const std::vector<InstDev<R>>& insts, size_t n_random) {
  if (nodes.empty()) return;
  const Node<R>& root = nodes[0];
  double M = 0.0, ext = 0.0;
  for (int k = 0; k < 3; k++) { M = std::max({M, std::fabs((double)root.bmin[k]), std::fabs((double)root.bmax[k])}); ext = std::max(ext, (double)root.bmax[k] - (double)root.bmin[k]); }
  for (const Tri<R>& t : tris) if (t.plane != kSphereMark && (t.material & kInstFlag)) {
    const R* m = insts[(t.material >> 16) & 0x7fffu].m;
    for (const R* v : {t.p0, t.p1, t.p2}) for (int i = 0; i < 3; i++)
      M = std::max(M, std::fabs((double)m[4 * i] * v[0]) + std::fabs((double)m[4 * i + 1] * v[1]) + std::fabs((double)m[4 * i + 2] * v[2]) + std::fabs((double)m[4 * i + 3]));
  }
  const R delta = (R)((double)kNearestPadUlps * (double)NnConst<R>::eps * M);
  // points: uniform in 1.5 x the root box, every triangle's vertices, edge midpoints and centroid (ties) up to a budget, points 100 extents away, a dead one
  std::vector<R> pts;
  uint64_t st = 0x9E3779B97F4A7C15ull;
  auto rnd = [&]() { st ^= st << 13; st ^= st >> 7; st ^= st << 17; return (double)(st >> 11) * (1.0 / 9007199254740992.0); };
  for (size_t i = 0; i < n_random; i++) for (int k = 0; k < 3; k++) {
    const double c = 0.5 * ((double)root.bmin[k] + (double)root.bmax[k]), h = 0.75 * ((double)root.bmax[k] - (double)root.bmin[k]) + 1e-3;
    pts.push_back((R)(c + h * (2.0 * rnd() - 1.0)));
  }
  const size_t step = std::max<size_t>(1, tris.size() / 300);
  for (size_t i = 0; i < tris.size(); i += step) {
    R v[3][3];
    if (!world_vertices(tris[i], insts, v)) continue;
    for (int j = 0; j < 3; j++) {
      for (int k = 0; k < 3; k++) pts.push_back(v[j][k]);
      for (int k = 0; k < 3; k++) pts.push_back((R)0.5 * (v[j][k] + v[(j + 1) % 3][k]));
    }
    for (int k = 0; k < 3; k++) pts.push_back((v[0][k] + v[1][k] + v[2][k]) / (R)3);
  }
  for (int i = 0; i < 8; i++) for (int k = 0; k < 3; k++) pts.push_back((R)((double)root.bmin[k] + ((i >> k) & 1 ? 100.0 : -100.0) * (ext + 1.0)));
  const size_t n_pts = pts.size() / 3;
  const uint32_t depth = tree_depth(nodes);
  VecStack stack;
  stack.a.resize(depth);
  std::vector<R> dists;
  size_t n_accepted = 0;
  for (int pass = 0; pass < 3; pass++) {
    // pass 0: no limit; passes 1, 2: the median and a tenth of the median of pass 0's distances
    R max_dist = NnConst<R>::inf;
    if (pass > 0) { std::vector<R> s(dists); std::sort(s.begin(), s.end()); max_dist = s[s.size() / 2] * (pass == 1 ? (R)1 : (R)0.1); }
    const R prune0 = nn_prune_start<R>(max_dist, delta);
    for (size_t i = 0; i < n_pts; i++) {
      const R px = pts[3 * i], py = pts[3 * i + 1], pz = pts[3 * i + 2];
      NnBest<R> scan = nn_none<R>(), walk;
      for (size_t t = 0; t < tris.size(); t++) nn_consider<R, true>(scan, tris[t], insts.data(), (uint32_t)t, px, py, pz);
      if (!nearest_walk<R>(nodes.data(), (uint32_t)nodes.size(), tris.data(), (uint32_t)tris.size(), insts.data(), px, py, pz, prune0, delta, stack, depth, &walk)) { fail("the walk passed a bound", i); continue; }
      if (stack.overrun) { fail("the walk left its stack", i); stack.overrun = false; }
      const NnOut<R> a = nn_result<R>(scan, max_dist), b = nn_result<R>(walk, max_dist);
      if (a.prim != b.prim || !same_bits(a.b1, b.b1) || !same_bits(a.b2, b.b2) || !same_bits(a.dist, b.dist)) fail("walk and scan differ", i);
      if (pass == 0) { dists.push_back(a.dist); if (a.prim < 0) fail("no candidate won with an unlimited radius", i); }
      else if (a.prim >= 0) n_accepted++;
    }
  }
  printf("  %s (%s): %zu nodes, depth %u, %zu entries, %zu points x 3 radii, %zu accepted under the finite radii\n", g_what.c_str(), sizeof(R) == 4 ? "f32" : "f64", nodes.size(), depth,
         tris.size(), n_pts, n_accepted);
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
  if (rrt_scene_load(path, RRT_FIXED_BVH, 0, &sc) != RRT_OK) { fprintf(stderr, "nearest_check: %s: %s\n", path, rrt_last_error()); g_fail++; return; }
  const rrt_scene_desc* d = rrt_scene_desc_of(sc);
  validate_desc(d);
  check_flat<double>(d);
  check_flat<float>(d);
  rrt_scene_free(sc);
}

// tools/prep_check.cpp's hand-built shapes: n leaves of one triangle each, a one-sided chain in pre-order
template <typename R>
void check_hand_built(int n_leaves, const char* name) {
  g_what = name;
  std::vector<Node<R>> nodes;
  std::vector<Tri<R>> tris((size_t)n_leaves);
  for (int i = 0; i < n_leaves; i++) {
    Tri<R>& t = tris[i];
    memset(&t, 0, sizeof(t));
    const R x = (R)1.5 * (R)i;
    t.p0[0] = x; t.p1[0] = x + (R)1; t.p2[0] = x; t.p2[1] = (R)1; t.p0[2] = t.p1[2] = t.p2[2] = (R)0.25 * (R)(i % 3);
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
    fprintf(stderr, "nearest_check: %s: exception: %s\n", g_what.c_str(), e.what());
    return 2;
  }
  if (g_fail) { fprintf(stderr, "nearest_check: %d check(s) failed\n", g_fail); return 1; }
  printf("nearest_check: ok\n");
  return 0;
}
