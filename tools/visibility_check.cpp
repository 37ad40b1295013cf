// visibility_check: the rrt_visibility walk (rs_ray_toy_amd/csrc/host/visibility.hpp vis_segment + vis_walk - the code the kernel k_visibility runs) on the
// CPU alone, compared pair by pair with the scan over all entries the call is defined as (vis_scan) and with rrt_trace_all's own scan (multihit_scan,
// k = 0: blocked iff its count is not 0).
// usage: visibility_check [scene.json ...]   - exit status 0 = no difference. Built from the host objects only (make -C rs_ray_toy_amd/csrc visibility_check);
// it can be built with the host sanitizers as it stands, which proves the stack and index logic without a device.
// Besides the scenes named on the command line (both precisions, every instance kept or flattened as the handle would have it) it walks two trees it makes
// itself: a root that is a single leaf, and a 96-deep one-sided chain. Every tree is walked with a stack of exactly the tree's depth - a push past it is a
// failure - in every combination of mode (MATRIX, PAIRS), b_kind (POINTS, DIRECTIONS) and flags (none, FACING_A, FACING_B, both) the call accepts, with and
// without skip entries, over point sets that hold surface points with normals, free points, coincident points and dead ones.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <exception>
#include <limits>
#include <string>
#include <vector>

#include "rrt.h"
#include "scene_prep.hpp"
#include "visibility.hpp"

using namespace rrtd;

namespace {
int g_fail = 0;
std::string g_what;
void fail(const char* msg, size_t i, size_t j) {
  if (g_fail++ < 20) fprintf(stderr, "visibility_check: %s: %s (pair %zu, %zu)\n", g_what.c_str(), msg, i, j);
}

struct VecStack {   // bounds-checked: the walk itself refuses a push past stack_cap, this catches a walk that does not
  std::vector<uint32_t> a;
  bool overrun = false;
  void put(uint32_t i, uint32_t v) { if (i < a.size()) a[i] = v; else overrun = true; }
  uint32_t get(uint32_t i) { if (i < a.size()) return a[i]; overrun = true; return 0u; }
};
template <typename R>
struct NoHits {   // multihit_scan at k = 0 never touches its buffer
  bool touched = false;
  R t(uint32_t) { touched = true; return R(0); }
  int32_t prim(uint32_t) { touched = true; return 0; }
  void set(uint32_t, R, int32_t) { touched = true; }
};

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
struct Point { R p[3], n[3]; int32_t skip; };

template <typename R>
void check_tree(const std::vector<Node<R>>& nodes, const std::vector<Tri<R>>& tris, const std::vector<InstDev<R>>& insts, size_t n_a, size_t n_b) {
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
  uint64_t st = 0x9E3779B97F4A7C15ull;
  auto rnd = [&]() { st ^= st << 13; st ^= st >> 7; st ^= st << 17; return (double)(st >> 11) * (1.0 / 9007199254740992.0); };
  std::vector<uint32_t> tri_ids;
  for (uint32_t i = 0; i < tris.size(); i++) if (tris[i].plane != kSphereMark) tri_ids.push_back(i);
  // a set: three quarters surface points (interior barycentrics, the geometric normal - un-normalised, either side -, the own entry as skip), the
  // rest free points of 1.5 x the root box with a random normal; then a coincident pair and the dead ones are planted
  auto make = [&](size_t n) {
    std::vector<Point<R>> s(n);
    for (size_t i = 0; i < n; i++) {
      Point<R>& q = s[i];
      if (i % 4 != 3 && !tri_ids.empty()) {
        const uint32_t id = tri_ids[(size_t)(rnd() * tri_ids.size()) % tri_ids.size()];
        R a[3], b[3], c[3];
        mh_vertices<R>(tris[id], insts.data(), a, b, c);
        double u = 0.05 + 0.85 * rnd(), v = 0.05 + 0.85 * rnd();
        if (u + v > 0.95) { u = 0.95 - u + 0.05; v = 0.95 - v + 0.05; }
        double e1[3], e2[3];
        for (int k = 0; k < 3; k++) { e1[k] = (double)b[k] - a[k]; e2[k] = (double)c[k] - a[k]; q.p[k] = (R)(a[k] + u * e1[k] + v * e2[k]); }
        const double sgn = rnd() < 0.5 ? -1.0 : 1.0;
        q.n[0] = (R)(sgn * (e1[1] * e2[2] - e1[2] * e2[1])); q.n[1] = (R)(sgn * (e1[2] * e2[0] - e1[0] * e2[2])); q.n[2] = (R)(sgn * (e1[0] * e2[1] - e1[1] * e2[0]));
        q.skip = (int32_t)id;
      } else {
        for (int k = 0; k < 3; k++) {
          const double c = 0.5 * ((double)root.bmin[k] + (double)root.bmax[k]), h = 0.75 * ((double)root.bmax[k] - (double)root.bmin[k]) + 1e-3;
          q.p[k] = (R)(c + h * (2.0 * rnd() - 1.0));
          q.n[k] = (R)(2.0 * rnd() - 1.0);
        }
        q.skip = -1;
      }
    }
    return s;
  };
  std::vector<Point<R>> A = make(n_a), B = make(n_b);
  const R nan = std::numeric_limits<R>::quiet_NaN();
  B[1] = A[1];                                             // coincident (with offsets 0)
  if (n_a > 8) { A[5].p[1] = nan; A[6].n[0] = A[6].n[1] = A[6].n[2] = R(0); A[7].n[2] = NnConst<R>::inf; }
  if (n_b > 8) { B[4].p[0] = NnConst<R>::inf; B[6].n[0] = B[6].n[1] = B[6].n[2] = R(0); B[8].p[0] = B[8].p[1] = B[8].p[2] = R(0); /* a zero direction */ }
  const uint32_t depth = tree_depth(nodes);
  VecStack stack;
  stack.a.resize(depth);
  const R offsets[2] = {R(0), (R)(1e-3 * ext)};
  size_t n_pairs = 0, n_traced = 0, n_blocked = 0, n_visible = 0;
  for (int mode = 0; mode < 2; mode++) for (int b_kind = 0; b_kind < 2; b_kind++) for (uint32_t flags = 0; flags < 4; flags++) for (int normals = 0; normals < 2; normals++)
  for (int with_skip = 0; with_skip < 2; with_skip++) {
    // the combinations rrt_visibility refuses: a FACING flag or an offset without normals; in DIRECTIONS B normals, FACING_B and skip_b
    const bool an = normals != 0, bn = normals != 0 && b_kind == kVisPoints;
    if (((flags & kVisFacingA) && !an) || ((flags & kVisFacingB) && !bn)) continue;
    const R off_a = an ? offsets[with_skip ? 0 : 1] : R(0), off_b = bn ? offsets[with_skip ? 0 : 1] : R(0);   // (skipping the own entry is what replaces the offset)
    const size_t rows = mode == kVisPairs ? std::min(n_a, n_b) : n_a;
    for (size_t i = 0; i < rows; i++) {
      const VisEnd<R> ea = vis_end<R>(A[i].p[0], A[i].p[1], A[i].p[2], an, A[i].n[0], A[i].n[1], A[i].n[2], off_a);
      for (size_t j = (mode == kVisPairs ? i : 0); j < (mode == kVisPairs ? i + 1 : n_b); j++) {
        const VisEnd<R> eb = vis_end<R>(B[j].p[0], B[j].p[1], B[j].p[2], bn, B[j].n[0], B[j].n[1], B[j].n[2], off_b);
        const int32_t sa = with_skip ? A[i].skip : -1, sb = with_skip && b_kind == kVisPoints ? B[j].skip : -1;
        MhRay<R> r;
        const VisVerdict v = vis_segment<R>(ea, eb, b_kind, flags, &r);
        n_pairs++;
        if (v == kVisYes) { if (!(b_kind == kVisPoints && flags == 0u)) fail("a pair is visible untraced where a flag or a direction forbids it", i, j); n_visible++; continue; }
        if (v == kVisNo) continue;
        n_traced++;
        if (b_kind == kVisDirections ? r.tmax != NnConst<R>::inf : !(r.tmax > R(0) && nn_finite(r.tmax))) fail("a traced pair's tmax is not what the kind says", i, j);
        bool blocked = false;
        if (!vis_walk<R>(nodes.data(), (uint32_t)nodes.size(), tris.data(), (uint32_t)tris.size(), insts.data(), r, sa, sb, delta, stack, depth, &blocked)) { fail("the walk passed a bound", i, j); continue; }
        if (stack.overrun) { fail("the walk left its stack", i, j); stack.overrun = false; }
        const bool scan = vis_scan<R>(tris.data(), (uint32_t)tris.size(), insts.data(), r, sa, sb);
        if (scan != blocked) fail("walk and scan differ", i, j);
        if (sb < 0 || sb == sa) {   // one skip entry at most: rrt_trace_all's own scan, count-only
          NoHits<R> none;
          const uint32_t c = multihit_scan<R>(tris.data(), (uint32_t)tris.size(), insts.data(), r, sa >= 0 ? sa : sb, none, 0u);
          if ((c != 0u) != scan || none.touched) fail("the scan differs from rrt_trace_all's count", i, j);
        }
        if (blocked) n_blocked++; else n_visible++;
      }
    }
  }
  printf("  %s (%s): %zu nodes, depth %u, %zu entries, %zu x %zu points: %zu pairs over the mode / kind / flag / normal / skip combinations, %zu traced, %zu blocked, %zu visible\n",
         g_what.c_str(), sizeof(R) == 4 ? "f32" : "f64", nodes.size(), depth, tris.size(), n_a, n_b, n_pairs, n_traced, n_blocked, n_visible);
  if (n_blocked == 0) fail("no pair was blocked", 0, 0);
  if (n_visible == 0) fail("no pair was visible", 0, 0);
}

template <typename R>
void check_flat(const rrt_scene_desc* d) {
  const FlatScene<R> fs = flatten_scene<R>(d, 0.0);
  bool any = false;
  for (const Tri<R>& t : fs.tris) any |= t.plane != kSphereMark;
  if (!any) { printf("  %s: no triangle entry (RRT_EUNSUP)\n", g_what.c_str()); return; }
  const bool large = fs.tris.size() > 20000;
  check_tree<R>(fs.nodes, fs.tris, fs.insts, large ? 12 : 24, large ? 20 : 40);
}

void check_scene(const char* path) {
  rrt_scene* sc = nullptr;
  g_what = path;
  if (rrt_scene_load(path, RRT_FIXED_BVH, 0, &sc) != RRT_OK) { fprintf(stderr, "visibility_check: %s: %s\n", path, rrt_last_error()); g_fail++; return; }
  const rrt_scene_desc* d = rrt_scene_desc_of(sc);
  validate_desc(d);
  check_flat<double>(d);
  check_flat<float>(d);
  rrt_scene_free(sc);
}

// tools/trace_all_check.cpp's hand-built shapes: n leaves of one triangle each, stacked along z, a one-sided chain in pre-order
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
  check_tree<R>(nodes, tris, std::vector<InstDev<R>>(), 24, 40);
}
}  // namespace

int main(int argc, char** argv) {
  try {
    for (int i = 1; i < argc; i++) { printf("%s\n", argv[i]); check_scene(argv[i]); }
    printf("hand-built trees\n");
    check_hand_built<float>(1, "single-leaf root"); check_hand_built<double>(1, "single-leaf root");
    check_hand_built<float>(96, "96-deep chain"); check_hand_built<double>(96, "96-deep chain");
  } catch (const std::exception& e) {
    fprintf(stderr, "visibility_check: %s: exception: %s\n", g_what.c_str(), e.what());
    return 2;
  }
  if (g_fail) { fprintf(stderr, "visibility_check: %d check(s) failed\n", g_fail); return 1; }
  printf("visibility_check: ok\n");
  return 0;
}
