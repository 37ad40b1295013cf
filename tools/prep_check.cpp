// prep_check: the scene preparation (rs_ray_toy_amd/csrc/host/scene_prep.hpp) run on the CPU alone, and every index its tables hand to the kernels checked.
// usage: prep_check [scene.json ...]   - exit status 0 = every check holds. Built from the host objects only (make -C rs_ray_toy_amd/csrc prep_check): that it
// links without a HIP library is the proof that preparation is HIP-free; it can be built with the host sanitizers as it stands.
// Besides the scenes named on the command line it checks two trees it makes itself: a root that is a single leaf, and a 96-deep one-sided chain.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <exception>
#include <string>
#include <vector>

#include "rrt.h"
#include "scene_prep.hpp"

using namespace rrtd;

namespace {
// the kernels' constants, as the driver passes them (device/dtraverse_f32.hpp, device/dmath.hpp)
constexpr int kTreelet = 512, kQuadTreeletN = 32, kTabDims = 64;
constexpr uint32_t kTtNodesN = 232u, kCamBlocks[3] = {729u, 15625u, 16807u};

int g_fail = 0;
std::string g_what;
void fail(const char* msg, size_t at = 0) {
  if (g_fail++ < 20) fprintf(stderr, "prep_check: %s: %s (at %zu)\n", g_what.c_str(), msg, at);
}
#define CHECK(cond, msg, at) do { if (!(cond)) { fail(msg, (size_t)(at)); } } while (0)

using Nodes = std::vector<Node<float>>;
using Tris = std::vector<Tri<float>>;
bool is_special(const Tri<float>& t) { return t.plane == kSphereMark || (t.material & kInstFlag) != 0u; }
bool same_box(const float* mn, const float* mx, const Node<float>& n) {
  for (int k = 0; k < 3; k++) if (mn[k] != n.bmin[k] || mx[k] != n.bmax[k]) return false;
  return true;
}
// a leaf word against the linear leaf it stands for; counts its triangles
void check_leaf_word(uint32_t w, const Node<float>& n, const Tris& tris, std::vector<uint32_t>& seen, bool with_special_bit) {
  const uint32_t np = n.meta >> 2;
  CHECK((w & kLeafBit) != 0u, "leaf child without the leaf bit", n.offset);
  CHECK((w & 0x7ffffu) == n.offset && ((w >> 19) & kLeafCountMask) == np, "leaf word names other triangles than the leaf", n.offset);
  bool sp = false;
  for (uint32_t t = n.offset; t < n.offset + np; t++) {
    if (t >= tris.size()) { fail("leaf outside the triangle array", t); return; }
    seen[t]++;
    sp |= is_special(tris[t]);
  }
  if (with_special_bit) CHECK(((w & kSpecialLeaf) != 0u) == sp, "kSpecialLeaf does not match the leaf's primitives", n.offset);
}
void check_seen(const Nodes& nodes, const std::vector<uint32_t>& seen) {
  for (const auto& n : nodes) for (uint32_t t = n.offset, e = n.offset + (n.meta >> 2); (n.meta >> 2) && t < e && t < seen.size(); t++)
    CHECK(seen[t] == 1u, "a leaf triangle is not reached exactly once", t);
}

void check_pairs(const Nodes& nodes, const Tris& tris, const PairTables& pt) {
  const size_t n = pt.pairs.size();
  std::vector<uint32_t> seen(tris.size(), 0u);
  std::vector<uint8_t> visited(n, 0);
  CHECK(pt.n_nodes == nodes.size(), "n_nodes", 0);
  CHECK(same_box(pt.root_box, pt.root_box + 3, nodes[0]), "root box", 0);
  if (nodes[0].meta >> 2) { check_leaf_word(pt.root_id, nodes[0], tris, seen, true); CHECK(n == 0, "pair nodes under a leaf root", n); }
  else {
    CHECK(pt.root_id == 0u && n > 0, "root word", pt.root_id);
    struct S { uint32_t word, lin; };
    std::vector<S> todo;
    if (n > 0) todo.push_back({0u, 0u});
    while (!todo.empty()) {
      const S s = todo.back(); todo.pop_back();
      if (s.word % 64u != 0u || s.word / 64u >= n) { fail("interior child word outside the pair array", s.word); continue; }
      if (visited[s.word / 64u]++) { fail("pair node reached twice", s.word / 64u); continue; }
      const PairNode& p = pt.pairs[s.word / 64u];
      CHECK(p.axis == (nodes[s.lin].meta & 3u), "split axis", s.lin);
      const uint32_t c[2] = {s.lin + 1u, nodes[s.lin].offset}, id[2] = {p.id0, p.id1};
      const float mn[2][3] = {{p.xy0[0], p.xy0[1], p.zz[0]}, {p.xy1[0], p.xy1[1], p.zz[2]}}, mx[2][3] = {{p.xy0[2], p.xy0[3], p.zz[1]}, {p.xy1[2], p.xy1[3], p.zz[3]}};
      for (int k = 0; k < 2; k++) {
        CHECK(same_box(mn[k], mx[k], nodes[c[k]]), "child box differs from the linear node's", c[k]);
        if (nodes[c[k]].meta >> 2) check_leaf_word(id[k], nodes[c[k]], tris, seen, true);
        else if (id[k] & kLeafBit) fail("interior child with a leaf word", c[k]);
        else todo.push_back({id[k], c[k]});
      }
    }
    for (size_t i = 0; i < n; i++) CHECK(visited[i] == 1, "pair node not reachable from the root", i);
    // BFS order of the treelet
    CHECK(pt.n_treelet <= (uint32_t)kTreelet && pt.n_treelet <= n, "treelet larger than its limit", pt.n_treelet);
    std::vector<uint32_t> bfs{0u};
    for (size_t h = 0; h < bfs.size() && bfs.size() < (size_t)pt.n_treelet + 2u; h++) {
      if (bfs[h] >= n) break;
      for (uint32_t id : {pt.pairs[bfs[h]].id0, pt.pairs[bfs[h]].id1}) if (!(id & kLeafBit)) bfs.push_back(id / 64u);
    }
    for (uint32_t i = 0; i < pt.n_treelet && i < bfs.size(); i++) CHECK(bfs[i] == i, "treelet not in BFS order", i);
  }
  check_seen(nodes, seen);
  // any-hit start lists
  if (!pt.any_list.empty()) {
    CHECK(pt.any_list.size() == tris.size() * 8u, "any-hit list size", pt.any_list.size());
    for (size_t t = 0; t < tris.size() && t * 8 + 7 < pt.any_list.size(); t++) {
      const uint32_t* w = &pt.any_list[t * 8];
      if (!seen[t]) continue;
      CHECK(w[7] <= (uint32_t)kAnyList, "any-hit list longer than kAnyList", t);
      if (w[0] & kLeafBit) CHECK((size_t)(w[0] & 0x7ffffu) + ((w[0] >> 19) & kLeafCountMask) <= tris.size(), "any-hit list: leaf word outside the triangles", t);
      else CHECK(w[0] % 64u == 0u && w[0] / 64u < n, "any-hit list: word 0 outside the pair array", t);
      for (uint32_t k = 0; k < w[7] && k < (uint32_t)kAnyList; k++) {
        const uint32_t e = w[1 + k], flag = e & 63u;
        CHECK((flag == kSkip0 || flag == kSkip1) && e / 64u < n && !(e & kLeafBit), "any-hit list: flagged entry outside the pair array", t);
      }
    }
  }
}

void check_quads(const Nodes& nodes, const Tris& tris, const QuadTables& qt) {
  const size_t n = qt.quads.size();
  if (n == 0) return;
  std::vector<uint32_t> seen(tris.size(), 0u);
  std::vector<uint8_t> visited(n, 0);
  struct S { uint32_t word, lin; };
  std::vector<S> todo{{0u, 0u}};
  auto interior = [&](uint32_t i) { return (nodes[i].meta >> 2) == 0u; };
  while (!todo.empty()) {
    const S s = todo.back(); todo.pop_back();
    if (s.word % 128u != 0u || s.word / 128u >= n) { fail("interior child word outside the quad array", s.word); continue; }
    if (visited[s.word / 128u]++) { fail("quad node reached twice", s.word / 128u); continue; }
    const QuadNode& q = qt.quads[s.word / 128u];
    const uint32_t c[2] = {s.lin + 1u, nodes[s.lin].offset};
    uint32_t slot[4] = {0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu};
    for (int k = 0; k < 2; k++) { if (interior(c[k])) { slot[2 * k] = c[k] + 1u; slot[2 * k + 1] = nodes[c[k]].offset; } else slot[2 * k] = c[k]; }
    const uint32_t axes[3] = {nodes[s.lin].meta & 3u, interior(c[0]) ? nodes[c[0]].meta & 3u : 0u, interior(c[1]) ? nodes[c[1]].meta & 3u : 0u};
    for (int k = 0; k < 4; k++) {
      const uint32_t id = k < 3 ? q.id[k] & ~kQuadAxisMask : q.id[k];
      if (k < 3) CHECK(((q.id[k] & kQuadAxisMask) >> kQuadAxisShift) == axes[k], "quad node: split axis", s.lin);
      if (slot[k] == 0xffffffffu) { CHECK(id == (kIdle & ~kQuadAxisMask) && std::isnan(q.mnx[k]) && std::isnan(q.mxx[k]), "quad node: empty slot is not idle", s.lin); continue; }
      const float mn[3] = {q.mnx[k], q.mny[k], q.mnz[k]}, mx[3] = {q.mxx[k], q.mxy[k], q.mxz[k]};
      CHECK(same_box(mn, mx, nodes[slot[k]]), "quad slot box differs from the linear node's", slot[k]);
      if (!interior(slot[k])) check_leaf_word(id, nodes[slot[k]], tris, seen, false);
      else if (id & kLeafBit) fail("interior slot with a leaf word", slot[k]);
      else todo.push_back({id, slot[k]});
    }
  }
  for (size_t i = 0; i < n; i++) CHECK(visited[i] == 1, "quad node not reachable from the root", i);
  check_seen(nodes, seen);
  CHECK(qt.n_qtreelet <= (uint32_t)kQuadTreeletN && qt.n_qtreelet <= n, "quad treelet larger than its limit", qt.n_qtreelet);
  std::vector<uint32_t> bfs{0u};
  for (size_t h = 0; h < bfs.size() && bfs.size() < (size_t)qt.n_qtreelet + 4u; h++) {
    if (bfs[h] >= n) break;
    for (int k = 0; k < 4; k++) { const uint32_t id = k < 3 ? qt.quads[bfs[h]].id[k] & ~kQuadAxisMask : qt.quads[bfs[h]].id[k]; if (!(id & kLeafBit) && id != (kIdle & ~kQuadAxisMask)) bfs.push_back(id / 128u); }
  }
  for (uint32_t i = 0; i < qt.n_qtreelet && i < bfs.size(); i++) CHECK(bfs[i] == i, "quad treelet not in BFS order", i);
}

void check_shadow_lists(const Tris& tris, const ShadowListsHost& sl, size_t n_lights) {
  CHECK(sl.table_of_light.size() == n_lights, "table_of_light size", sl.table_of_light.size());
  for (uint32_t t : sl.table_of_light) CHECK(t <= sl.n_tables, "light names a table that does not exist", t);
  if (sl.n_tables == 0) return;
  CHECK(sl.headers.size() == (size_t)sl.n_tables * tris.size(), "shadow list headers size", sl.headers.size());
  CHECK(sl.entries.size() % 4u == 0u, "shadow list entries not padded to four", sl.entries.size());
  for (size_t i = 0; i < sl.headers.size(); i++) {
    const uint32_t h = sl.headers[i], count = h & 0xffu;
    if (h == 0xffu) continue;
    const size_t first = (size_t)(h >> 8) * 4u;
    if (count > kShadowListMax || first + count > sl.entries.size()) { fail("shadow list header points outside the entries", i); continue; }
    for (uint32_t k = 0; k < count; k++) CHECK(sl.entries[first + k] < sl.leaves.size(), "shadow list entry is no leaf index", i);
  }
  for (size_t i = 0; i < sl.entries.size(); i++) CHECK(sl.entries[i] < sl.leaves.size() || sl.entries[i] == 0xffffffffu, "shadow list entry is neither a leaf index nor padding", i);
  for (size_t i = 0; i < sl.leaves.size(); i++) {
    const uint32_t w = sl.leaves[i].word;
    CHECK((w & kLeafBit) && (size_t)(w & 0x7ffffu) + ((w >> 19) & kLeafCountMask) <= tris.size(), "shadow list leaf record outside the triangles", i);
  }
}

// a few hundred rays through the root box, dealt to four patches; a fifth patch gets none (it takes the copy of the tree's top)
void check_tile_trees(const Tris& tris, const PairTables& pt, uint32_t tt_nodes, uint32_t tt_tris) {
  const size_t n_int = pt.pairs.size();
  const TileTreeSizes sz{tt_nodes, tt_tris, (tt_local_addr(tt_nodes - 1u) + 64u + 63u) & ~63u};
  std::vector<CensusRay> rays;
  std::vector<uint32_t> tree_of;
  uint64_t st = 0x9E3779B97F4A7C15ull;
  auto rnd = [&]() { st ^= st << 13; st ^= st >> 7; st ^= st << 17; return (float)((double)(st >> 11) * (1.0 / 9007199254740992.0)); };
  const float* b = pt.root_box;
  const float ext = std::fmax(std::fmax(b[3] - b[0], b[4] - b[1]), std::fmax(b[5] - b[2], 1e-3f));
  for (int i = 0; i < 400; i++) {
    CensusRay r;
    float to[3];
    for (int k = 0; k < 3; k++) { to[k] = b[k] + (b[3 + k] - b[k]) * rnd(); r.o[k] = 0.5f * (b[k] + b[3 + k]) + (k == i % 3 ? 2.0f : 0.3f * (rnd() - 0.5f)) * ext * (i & 4 ? 1.0f : -1.0f); }
    float l = 0.0f;
    for (int k = 0; k < 3; k++) { r.d[k] = to[k] - r.o[k]; l += r.d[k] * r.d[k]; }
    l = std::sqrt(l);
    for (int k = 0; k < 3; k++) r.d[k] /= l;
    rays.push_back(r); tree_of.push_back((uint32_t)(i % 4));
  }
  const uint32_t n_trees = 5;
  const TileTreeTables tt = build_tile_trees(pt.pairs, tris, pt.root_box, rays, tree_of, n_trees, sz);
  if (tt.failed) { fail("tile trees: out of memory"); return; }
  CHECK(tt.trees.size() == (size_t)(n_trees + 1) * sz.nodes, "tile trees: size of the copies", tt.trees.size());
  CHECK(tt.shifted.size() == sz.local_bytes / sizeof(PairNode) + n_int, "tile trees: size of the shifted tree", tt.shifted.size());
  CHECK(tt.packets.size() == (size_t)(n_trees + 1) * sz.tris * 3u, "tile trees: size of the packets", tt.packets.size());
  CHECK(tt.n_with == 4u, "tile trees: patches with rays", tt.n_with);
  std::vector<uint8_t> is_local(sz.local_bytes, 0);
  for (uint32_t k = 0; k < sz.nodes; k++) is_local[tt_local_addr(k)] = 1;
  auto word_ok = [&](uint32_t w, bool in_copy) {
    if (w & kLeafBit) return !(w & kSpecialLeaf) || (in_copy && sz.tris > 0u && (w & 0x7ffffu) + ((w >> 19) & kLeafCountMask) <= sz.tris);
    if (w < sz.local_bytes) return in_copy && is_local[w] != 0;
    return (w - sz.local_bytes) % 64u == 0u && (w - sz.local_bytes) / 64u < n_int;
  };
  for (size_t i = 0; i < tt.trees.size(); i++) CHECK(word_ok(tt.trees[i].id0, true) && word_ok(tt.trees[i].id1, true), "tile tree copy: child word is neither a local slot nor a node of the whole tree", i);
  for (size_t i = sz.local_bytes / sizeof(PairNode); i < tt.shifted.size(); i++) CHECK(word_ok(tt.shifted[i].id0, false) && word_ok(tt.shifted[i].id1, false), "shifted tree: child word outside the tree", i);
}

// every fp32 traversal table of one tree; d: the desc whose lights the shadow lists are for
void check_tree(const Nodes& nodes, const Tris& tris, const rrt_scene_desc* d) {
  if (nodes.empty()) return;
  const PairTables pt = build_pairs(nodes, tris, kTreelet);
  if (!pt.ok) { printf("  %s: no pair nodes for this tree\n", g_what.c_str()); return; }
  check_pairs(nodes, tris, pt);
  size_t n_quads = 0, n_entries = 0;
  if (!pt.mixed) { const QuadTables qt = build_quads(nodes, kQuadTreeletN); check_quads(nodes, tris, qt); n_quads = qt.quads.size(); }
  if (!pt.mixed && d->n_lights > 0) { const ShadowListsHost sl = build_shadow_lists(nodes, tris, d); check_shadow_lists(tris, sl, d->n_lights); n_entries = sl.entries.size(); }
  bool tiles = false;
  if (!pt.mixed && pt.root_id == 0u && pt.pairs.size() >= 2) {
    const uint32_t tt_nodes = pt.pairs.size() > kTtNodesN ? kTtNodesN : (uint32_t)(pt.pairs.size() / 2);
    check_tile_trees(tris, pt, tt_nodes, 0u);
    check_tile_trees(tris, pt, tt_nodes, 4u);
    tiles = true;
  }
  printf("  %s: %zu nodes, %zu triangles -> %zu pair nodes (treelet %u%s), %zu quad nodes, %zu shadow list entries, tile trees %s\n", g_what.c_str(), nodes.size(), tris.size(),
         pt.pairs.size(), pt.n_treelet, pt.mixed ? ", mixed" : "", n_quads, n_entries, tiles ? "checked" : "not built");
}

template <typename R>
FlatScene<R> check_flatten(const rrt_scene_desc* d, double pad) {
  FlatScene<R> fs = flatten_scene<R>(d, pad);
  CHECK(fs.nodes.size() == d->n_bvh_nodes && fs.tris.size() == d->n_prim_order && fs.mats.size() == d->n_materials && fs.texs.size() == d->n_textures &&
        fs.imgs.size() == d->n_images && fs.lights.size() == d->n_lights && fs.light_cdf.size() == d->n_lights + 1 && fs.lens.size() == (size_t)d->camera.n_elems, "flatten_scene: sizes", 0);
  for (size_t i = 0; i < fs.tris.size(); i++) {
    const Tri<R>& t = fs.tris[i];
    if (t.plane == kSphereMark) CHECK(t.shade < fs.spheres.size(), "sphere index", i);
    else {
      CHECK(t.shade == 0xffffffffu || t.shade < fs.shades.size(), "shade index", i);
      if (t.material & kInstFlag) CHECK(((t.material >> 16) & 0x7fffu) < fs.insts.size(), "instance index", i);
    }
    CHECK((t.material & kInstFlag ? t.material & 0xffffu : t.material) < fs.mats.size(), "material index", i);
  }
  for (size_t i = 0; i < fs.nodes.size(); i++) for (int k = 0; k < 3; k++)
    CHECK((double)fs.nodes[i].bmin[k] <= d->bvh_nodes[i].bounds[k] && (double)fs.nodes[i].bmax[k] >= d->bvh_nodes[i].bounds[3 + k], "node box narrowed inward", i);
  return fs;
}

void check_scene(const char* path) {
  rrt_scene* sc = nullptr;
  g_what = path;
  if (rrt_scene_load(path, RRT_FIXED_BVH, 0, &sc) != RRT_OK) { fail(rrt_last_error()); return; }
  const rrt_scene_desc* d = rrt_scene_desc_of(sc);
  printf("%s\n", path);
  validate_desc(d);
  check_flatten<double>(d, 0.0);
  check_flatten<float>(d, 4.0);   // (the padded boxes of the FMA slab variant)
  const FlatScene<float> fs = check_flatten<float>(d, 0.0);
  for (int f32 = 0; f32 < 2; f32++) {
    const SamplerTables s = build_sampler_tables(d, f32 != 0, kTabDims, kCamBlocks, true);
    CHECK(s.hdims.size() == 1000u, "sampler tables: dimensions", s.hdims.size());
    CHECK(f32 || (s.blk.empty() && !s.has_cam), "sampler tables: block tables in the f64 mode", 0);
    for (const HaltonBlk& b : s.blk) if (b.block) CHECK((size_t)b.lo_off + b.block <= s.lo.size() && b.hi_off < s.hi.size(), "sampler tables: block outside its table", b.lo_off);
    if (s.has_cam) for (int w = 0; w < 3; w++) CHECK(s.cam_lo_off[w] + kCamBlocks[w] <= s.cam_lo.size() && s.cam_hi_off[w] < s.cam_hi.size(), "camera tables: block outside its table", w);
  }
  const AuxMargins am = calibrate_aux_margins(d);
  CHECK(am.lim.size() == 2u * (size_t)d->camera.n_elems, "aux margins: size", am.lim.size());
  check_tree(fs.nodes, fs.tris, d);
  rrt_scene_free(sc);
}

// the smallest shapes that can go wrong; one point light for the shadow lists
void check_hand_built(int n_leaves, const char* name) {
  g_what = name;
  Nodes nodes;
  Tris tris((size_t)n_leaves);
  for (int i = 0; i < n_leaves; i++) {
    Tri<float>& t = tris[i];
    memset(&t, 0, sizeof(t));
    const float x = 1.5f * (float)i;
    t.p0[0] = x; t.p1[0] = x + 1.0f; t.p2[0] = x; t.p2[1] = 1.0f; t.p0[2] = t.p1[2] = t.p2[2] = 0.25f * (float)(i % 3);
    t.shade = 0xffffffffu; t.plane = (uint32_t)i;
  }
  auto leaf = [&](int i) { Node<float> n{}; for (int k = 0; k < 3; k++) { n.bmin[k] = std::fmin(tris[i].p0[k], std::fmin(tris[i].p1[k], tris[i].p2[k])); n.bmax[k] = std::fmax(tris[i].p0[k], std::fmax(tris[i].p1[k], tris[i].p2[k])); } n.offset = (uint32_t)i; n.meta = 1u << 2; return n; };
  // pre-order: interior node 2k has the leaf of triangle k as its first child (2k + 1) and the rest of the chain as its second (2k + 2)
  for (int i = 0; i + 1 < n_leaves; i++) { Node<float> n{}; n.offset = (uint32_t)(2 * i + 2); n.meta = (uint32_t)(i % 3); nodes.push_back(n); nodes.push_back(leaf(i)); }
  nodes.push_back(leaf(n_leaves - 1));
  for (int i = (int)nodes.size() - 1; i >= 0; i--) if ((nodes[i].meta >> 2) == 0u) {
    const Node<float>&a = nodes[i + 1], &b = nodes[nodes[i].offset];
    for (int k = 0; k < 3; k++) { nodes[i].bmin[k] = std::fmin(a.bmin[k], b.bmin[k]); nodes[i].bmax[k] = std::fmax(a.bmax[k], b.bmax[k]); }
  }
  rrt_scene_desc d;
  memset(&d, 0, sizeof(d));
  rrt_light light;
  memset(&light, 0, sizeof(light));
  light.type = RRT_LIGHT_POINT;
  light.p_light[0] = 3.0; light.p_light[1] = 40.0; light.p_light[2] = 25.0;
  d.lights = &light; d.n_lights = 1;
  check_tree(nodes, tris, &d);
}
}  // namespace

int main(int argc, char** argv) {
  try {
    for (int i = 1; i < argc; i++) check_scene(argv[i]);
    printf("hand-built trees\n");
    check_hand_built(1, "single-leaf root");
    check_hand_built(96, "96-deep chain");
  } catch (const std::exception& e) {
    fprintf(stderr, "prep_check: %s: exception: %s\n", g_what.c_str(), e.what());
    return 2;
  }
  if (g_fail) { fprintf(stderr, "prep_check: %d check(s) failed\n", g_fail); return 1; }
  printf("prep_check: ok\n");
  return 0;
}
