// Scene preparation, part 3: the tables of the fp32 traversal kernels - pair nodes with their treelet numbering and any-hit start lists, quad nodes,
// tile trees (see scene_prep.hpp; device/dtraverse_f32.hpp has the kernels that read them).
#include "scene_prep.hpp"

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstring>
#include <queue>
#include <thread>

namespace rrtd {

// re-pack the linear BVH into pair nodes (see dtraverse_f32.hpp)
PairTables build_pairs(const std::vector<Node<float>>& nodes, const std::vector<Tri<float>>& tris, int treelet_nodes) {
  PairTables out;
  {
    const size_t n_tris = tris.size();
    if (nodes.empty() || n_tris >= (1u << 19)) return out;
    // leaves that hold a sphere or a triangle of a kept instance carry kSpecialLeaf in their word (the MIXED kernels' rare path)
    auto special_leaf = [&](uint32_t first, uint32_t n) {
      for (uint32_t t = first; t < first + n && t < n_tris; t++) if (tris[t].plane == kSphereMark || (tris[t].material & kInstFlag) != 0u) return true;
      return false;
    };
    std::vector<uint32_t> compact(nodes.size(), 0xffffffffu);
    uint32_t n_int = 0;
    for (size_t i = 0; i < nodes.size(); i++) {
      const uint32_t np = nodes[i].meta >> 2;
      if (np == 0) compact[i] = n_int++;
      else if (np > kLeafCountMask) return out;
    }
    struct Pair {   // host-side form; packed into the kernels' PairNode below
      float b0min[3], b0max[3], b1min[3], b1max[3];
      uint32_t ref0, ref1;   // interior child: pair index; leaf child: first triangle
      uint32_t meta;         // bits 0-1 split axis, bits 2-13 n_prims of child 0 (0 = interior), bits 14-25 of child 1
    };
    std::vector<Pair> pairs(n_int);
    std::vector<uint32_t> newidx_keep;   // BFS renumbering of the pair nodes
    for (size_t i = 0; i < nodes.size(); i++) {
      if ((nodes[i].meta >> 2) != 0) continue;
      Pair& pn = pairs[compact[i]];
      const size_t c0 = i + 1, c1 = nodes[i].offset;
      const uint32_t n0 = nodes[c0].meta >> 2, n1 = nodes[c1].meta >> 2;
      for (int k = 0; k < 3; k++) { pn.b0min[k] = nodes[c0].bmin[k]; pn.b0max[k] = nodes[c0].bmax[k]; pn.b1min[k] = nodes[c1].bmin[k]; pn.b1max[k] = nodes[c1].bmax[k]; }
      pn.ref0 = n0 ? nodes[c0].offset : compact[c0];
      pn.ref1 = n1 ? nodes[c1].offset : compact[c1];
      pn.meta = (nodes[i].meta & 3u) | (n0 << 2) | (n1 << 14);
    }
    // renumber: the BFS top of the tree first (staged in LDS by the kernels), the rest in pre-order
    if (n_int > 0 && (nodes[0].meta >> 2) == 0) {
      std::vector<uint32_t> order; order.reserve(n_int);
      std::vector<uint8_t> taken(n_int, 0);
      std::vector<uint32_t> frontier{0};
      while (!frontier.empty() && order.size() < (size_t)treelet_nodes) {
        std::vector<uint32_t> next;
        for (uint32_t k : frontier) {
          if (order.size() >= (size_t)treelet_nodes) break;
          order.push_back(k); taken[k] = 1;
          const Pair& pn = pairs[k];
          if (((pn.meta >> 2) & 0xfffu) == 0) next.push_back(pn.ref0);
          if (((pn.meta >> 14) & 0xfffu) == 0) next.push_back(pn.ref1);
        }
        frontier.swap(next);
      }
      out.n_treelet = (uint32_t)order.size();
      for (uint32_t k = 0; k < n_int; k++) if (!taken[k]) order.push_back(k);
      std::vector<uint32_t> newidx(n_int);
      for (uint32_t i = 0; i < n_int; i++) newidx[order[i]] = i;
      newidx_keep = newidx;
      std::vector<Pair> re(n_int);
      for (uint32_t i = 0; i < n_int; i++) {
        Pair pn = pairs[order[i]];
        if (((pn.meta >> 2) & 0xfffu) == 0) pn.ref0 = newidx[pn.ref0];
        if (((pn.meta >> 14) & 0xfffu) == 0) pn.ref1 = newidx[pn.ref1];
        re[i] = pn;
      }
      pairs.swap(re);
    } else out.n_treelet = 0;
    // any-hit start lists (TravScene::any_list): per triangle, the pair nodes between the root and its leaf whose OFF-path child is within
    // reach of a shadow ray (kShadowTmax long, Q9; + 0.02 + 8 ulp of the largest scene coordinate, see `reach` below), top down,
    // at most kAnyList of them; the ordinary walk resumes at the next such node (or at the leaf itself when the list holds them all).
    std::vector<uint32_t>& lists = out.any_list;
    if (n_int > 0 && (nodes[0].meta >> 2) == 0) {
      lists.assign(n_tris * 8, kIdle);
      std::vector<uint32_t> pair_of(nodes.size(), 0xffffffffu);   // linear interior node -> pair node id as the kernels index them
      {
        std::vector<uint32_t> renum(n_int);
        bool renumbered = out.n_treelet > 0;
        for (uint32_t k = 0; k < n_int; k++) renum[k] = k;
        if (renumbered) renum = newidx_keep;
        for (size_t i = 0; i < nodes.size(); i++) if ((nodes[i].meta >> 2) == 0) pair_of[i] = renum[compact[i]];
      }
      auto box_dist2 = [&](const Node<float>& a, const Node<float>& b) {
        double d2 = 0;
        for (int k = 0; k < 3; k++) { const double g = std::max(0.0, std::max((double)a.bmin[k] - (double)b.bmax[k], (double)b.bmin[k] - (double)a.bmax[k])); d2 += g * g; }
        return d2;
      };
      // Reach of a pool shadow ray from its triangle's leaf box: its length kShadowTmax, 0.02 for what the fp32 evaluation adds relative
      // to it (|d| = 1 +- 1e-6, the boxes' outward rounding, the slab test's widening factor g), plus what is ABSOLUTE in world units: the
      // ray's fp32 origin word lies within an ulp of its triangle - hence of the leaf box - and the plane distances are differences of
      // coordinates of the size M = the largest root-box coordinate: 8 ulp(M). At coordinates of 1e5 that is 0.06, not covered by 0.02.
      double coord_max = 0.0;
      for (int k = 0; k < 3; k++) coord_max = std::max(coord_max, std::max(std::fabs((double)nodes[0].bmin[k]), std::fabs((double)nodes[0].bmax[k])));
      const double reach = (double)kShadowTmax + 0.02 + 8.0 * coord_max * 1.1920929e-7;
      const double reach2 = reach * reach;
      // iterative pre-order walk carrying the path of interior nodes from the root to the current node's parent
      struct Step { uint32_t node; uint32_t depth; };
      std::vector<uint32_t> path;
      std::vector<Step> todo{{0u, 0u}};
      while (!todo.empty()) {
        const Step st = todo.back(); todo.pop_back();
        path.resize(st.depth);
        const Node<float>& nd = nodes[st.node];
        const uint32_t np = nd.meta >> 2;
        if (np == 0) {
          path.push_back(st.node);
          todo.push_back({nd.offset, st.depth + 1});
          todo.push_back({st.node + 1, st.depth + 1});
          continue;
        }
        uint32_t words[8];
        for (uint32_t& w : words) w = kIdle;
        uint32_t n_flagged = 0;
        words[0] = kLeafBit | (special_leaf(nd.offset, np) ? kSpecialLeaf : 0u) | (np << 19) | nd.offset;   // every deciding node fits the list: only the leaf itself is left
        for (size_t k = 0; k < path.size(); k++) {
          const uint32_t a = path[k];
          const uint32_t on = (k + 1 < path.size()) ? path[k + 1] : st.node;
          const uint32_t c0 = a + 1, c1 = nodes[a].offset;
          const uint32_t off = on == c0 ? c1 : c0;
          if (box_dist2(nodes[off], nd) > reach2) continue;   // the off-path child cannot be hit from this leaf: the node decides nothing
          if (n_flagged == (uint32_t)kAnyList) { words[0] = pair_of[a] * 64u; break; }   // list full: the ordinary walk takes over here
          words[1 + n_flagged++] = (pair_of[a] * 64u) | (on == c0 ? kSkip0 : kSkip1);
        }
        words[7] = n_flagged;
        for (uint32_t t = 0; t < np; t++) if ((size_t)nd.offset + t < n_tris) for (int w = 0; w < 8; w++) lists[((size_t)nd.offset + t) * 8 + w] = words[w];
      }
    }
    // the kernels' form: plane coordinates paired for the packed slab arithmetic, children as ready-made stack words
    if ((uint64_t)n_int * 64u >= kIdle) return out;
    std::vector<PairNode>& packed = out.pairs;
    packed.resize(n_int);
    auto child_word = [&](uint32_t ref, uint32_t n_prims) {
      if (!n_prims) return ref * 64u;
      const bool sp = special_leaf(ref, n_prims);
      out.mixed |= sp;
      return kLeafBit | (sp ? kSpecialLeaf : 0u) | (n_prims << 19) | ref;
    };
    for (uint32_t i = 0; i < n_int; i++) {
      const Pair& s = pairs[i];
      PairNode& d = packed[i];
      d.xy0[0] = s.b0min[0]; d.xy0[1] = s.b0min[1]; d.xy0[2] = s.b0max[0]; d.xy0[3] = s.b0max[1];
      d.xy1[0] = s.b1min[0]; d.xy1[1] = s.b1min[1]; d.xy1[2] = s.b1max[0]; d.xy1[3] = s.b1max[1];
      d.zz[0] = s.b0min[2]; d.zz[1] = s.b0max[2]; d.zz[2] = s.b1min[2]; d.zz[3] = s.b1max[2];
      d.id0 = child_word(s.ref0, (s.meta >> 2) & 0xfffu);
      d.id1 = child_word(s.ref1, (s.meta >> 14) & 0xfffu);
      d.axis = s.meta & 3u;
      d.pad = 0;
    }
    for (int k = 0; k < 3; k++) { out.root_box[k] = nodes[0].bmin[k]; out.root_box[3 + k] = nodes[0].bmax[k]; }
    out.root_id = (nodes[0].meta >> 2) ? child_word(nodes[0].offset, nodes[0].meta >> 2) : 0u;
    out.n_nodes = (uint32_t)nodes.size();
    out.ok = true;
  }
  return out;
}
// QuadNode array of the two-levels-per-fetch closest-hit kernel (dtraverse_f32.hpp): one node per interior node that a walk from the root in
// steps of two levels can reach; numbered BFS for the top kQuadTreelet (the kernel's LDS treelet), pre-order below
QuadTables build_quads(const std::vector<Node<float>>& nodes, int quad_treelet) {
  QuadTables out;
  {
    if (nodes.empty() || (nodes[0].meta >> 2) != 0) return out;
    for (const auto& nd : nodes) if ((nd.meta >> 2) > kQuadLeafMax) return out;
    auto interior = [&](uint32_t i) { return (nodes[i].meta >> 2) == 0; };
    // slots of N: (child, grandchild) linear indices; a leaf child = one slot holding the child itself
    struct Slots { uint32_t n[4]; };
    auto slots_of = [&](uint32_t N) {
      Slots sl{{0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu}};
      const uint32_t c[2] = {N + 1u, nodes[N].offset};
      for (int k = 0; k < 2; k++) {
        if (interior(c[k])) { sl.n[2 * k] = c[k] + 1u; sl.n[2 * k + 1] = nodes[c[k]].offset; }
        else sl.n[2 * k] = c[k];
      }
      return sl;
    };
    std::vector<uint32_t> qidx(nodes.size(), 0xffffffffu), order;
    {   // BFS for the treelet
      std::vector<uint32_t> frontier{0u};
      while (!frontier.empty() && order.size() < (size_t)quad_treelet) {
        std::vector<uint32_t> next;
        for (uint32_t N : frontier) {
          if (order.size() >= (size_t)quad_treelet) break;
          qidx[N] = (uint32_t)order.size(); order.push_back(N);
          const Slots sl = slots_of(N);
          for (uint32_t g : sl.n) if (g != 0xffffffffu && interior(g)) next.push_back(g);
        }
        frontier.swap(next);
      }
      out.n_qtreelet = (uint32_t)order.size();
      // the rest in pre-order
      std::vector<uint32_t> todo{0u};
      while (!todo.empty()) {
        const uint32_t N = todo.back(); todo.pop_back();
        if (qidx[N] == 0xffffffffu) { qidx[N] = (uint32_t)order.size(); order.push_back(N); }
        const Slots sl = slots_of(N);
        for (int k = 3; k >= 0; k--) if (sl.n[k] != 0xffffffffu && interior(sl.n[k])) todo.push_back(sl.n[k]);
      }
    }
    if ((uint64_t)order.size() * 128u >= (1ull << 28)) { out.n_qtreelet = 0; return out; }
    std::vector<QuadNode>& q = out.quads;
    q.resize(order.size());
    const float nan = std::nanf("");
    for (size_t i = 0; i < order.size(); i++) {
      const uint32_t N = order[i];
      const Slots sl = slots_of(N);
      QuadNode& d = q[i];
      memset(&d, 0, sizeof(d));
      for (int k = 0; k < 4; k++) {
        const uint32_t g = sl.n[k];
        if (g == 0xffffffffu) { d.mnx[k] = d.mny[k] = d.mnz[k] = d.mxx[k] = d.mxy[k] = d.mxz[k] = nan; d.id[k] = kIdle & ~kQuadAxisMask; continue; }
        d.mnx[k] = nodes[g].bmin[0]; d.mny[k] = nodes[g].bmin[1]; d.mnz[k] = nodes[g].bmin[2];
        d.mxx[k] = nodes[g].bmax[0]; d.mxy[k] = nodes[g].bmax[1]; d.mxz[k] = nodes[g].bmax[2];
        const uint32_t np = nodes[g].meta >> 2;
        d.id[k] = np ? (kLeafBit | (np << 19) | nodes[g].offset) : qidx[g] * 128u;
      }
      const uint32_t c0 = N + 1u, c1 = nodes[N].offset;
      d.id[0] |= (nodes[N].meta & 3u) << kQuadAxisShift;
      d.id[1] |= (interior(c0) ? (nodes[c0].meta & 3u) : 0u) << kQuadAxisShift;
      d.id[2] |= (interior(c1) ? (nodes[c1].meta & 3u) : 0u) << kQuadAxisShift;
    }
  }
  return out;
}

// Tile trees (dtraverse_f32.hpp, k_trace_tiles_f32): per 32 x 32-pixel patch of the image, a local copy of the kTtNodes pair nodes its camera rays visit
// most. The census: a few camera samples per pixel through the product's own camera kernels, their rays walked here on the host (plain fp32 slab and
// Moeller-Trumbore tests, hits accepted like Q10) with a visit counter per pair node and patch. The counts only decide which nodes are copied; what a
// copy says about a node is the tree's own data, so no result depends on them. A set of most-visited nodes is closed under "parent" (a parent is
// visited at least as often as its child and has the smaller index, which breaks ties), so every copied node can be reached through copies.
namespace {
inline float uint_as_float(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }
}  // namespace
TileTreeTables build_tile_trees(const std::vector<PairNode>& pairs, const std::vector<Tri<float>>& tris, const float root_box[6], const std::vector<CensusRay>& rays,
                                const std::vector<uint32_t>& tree_of, uint32_t n_trees, TileTreeSizes sz) {
  TileTreeTables res;
  using CRay = CensusRay;
  const uint32_t kTtNodes = sz.nodes, kTtTris = sz.tris, kTtLocalBytes = sz.local_bytes;
  const size_t n_int = pairs.size();
  std::vector<uint32_t> first(n_trees + 1, 0), order(rays.size());
  for (uint32_t t : tree_of) first[t + 1]++;
  for (uint32_t t = 0; t < n_trees; t++) first[t + 1] += first[t];
  { std::vector<uint32_t> at(first.begin(), first.end() - 1); for (uint32_t i = 0; i < (uint32_t)rays.size(); i++) order[at[tree_of[i]]++] = i; }

  // ---- per patch: walk, count, choose, copy
  std::vector<PairNode>& trees = res.trees;
  trees.resize((size_t)(n_trees + 1) * kTtNodes);
  memset(trees.data(), 0, trees.size() * sizeof(PairNode));
  std::vector<Float4>& packets = res.packets;
  packets.assign(kTtTris > 0 ? (size_t)(n_trees + 1) * kTtTris * 3u : 0u, Float4{0.0f, 0.0f, 0.0f, 0.0f});   // RRT_TT_TRIS > 0 builds
  std::atomic<uint64_t> sum_local_tests{0}, sum_tests{0};
  // the triangle packet of one copy: the leaves named by the copy's nodes, most tested first, while they fit; their words rewritten to local indices
  auto pack_tris = [&](PairNode* dst, uint32_t n_nodes, Float4* out, const std::vector<uint32_t>& tcount, uint64_t* served) {
    if (kTtTris == 0) return;
    struct L { uint32_t count, node, which; };
    std::vector<L> leaves;
    for (uint32_t k = 0; k < n_nodes; k++) for (uint32_t w = 0; w < 2; w++) {
      const uint32_t id = w ? dst[k].id1 : dst[k].id0;
      if ((id & kLeafBit) && !(id & kSpecialLeaf)) leaves.push_back(L{tcount.empty() ? 0u : tcount[id & 0x7ffffu], k, w});
    }
    std::stable_sort(leaves.begin(), leaves.end(), [](const L& a, const L& b) { return a.count > b.count; });
    uint32_t used = 0;
    for (const L& l : leaves) {
      uint32_t& id = l.which ? dst[l.node].id1 : dst[l.node].id0;
      const uint32_t first = id & 0x7ffffu, np = (id >> 19) & kLeafCountMask;
      if (used + np > kTtTris) continue;
      for (uint32_t t = 0; t < np; t++) {
        const Tri<float>& tr = tris[first + t];
        out[3u * (used + t)] = Float4{tr.p0[0], tr.p0[1], tr.p0[2], tr.p1[0]};
        out[3u * (used + t) + 1u] = Float4{tr.p1[1], tr.p1[2], tr.p2[0], tr.p2[1]};
        out[3u * (used + t) + 2u] = Float4{tr.p2[2], uint_as_float(first + t), uint_as_float(tr.shade), uint_as_float(tr.plane)};   // material word <- the triangle's own index
      }
      id = kLeafBit | kSpecialLeaf | (np << 19) | used;
      used += np;
      if (served) *served += l.count;
    }
  };
  const uint32_t shift = kTtLocalBytes;   // interior child words of the whole tree start here; below: LDS addresses of a copy's slots
  auto slab = [](const float bmin[3], const float bmax[3], const float o[3], const float inv[3], float* t) {
    float tn = -INFINITY, tf = INFINITY;
    for (int k = 0; k < 3; k++) { const float a = (bmin[k] - o[k]) * inv[k], b = (bmax[k] - o[k]) * inv[k]; tn = std::max(tn, std::min(a, b)); tf = std::min(tf, std::max(a, b)); }
    *t = tn;
    return tn <= tf * 1.0000004f && tf > 0.0f;
  };
  auto copy_into = [&](PairNode* dst, const std::vector<uint32_t>& sel, std::vector<uint32_t>& slot_of) {   // sel ascending; slot_of: all-ones scratch, restored
    for (uint32_t k = 0; k < (uint32_t)sel.size(); k++) slot_of[sel[k]] = k;
    for (uint32_t k = 0; k < (uint32_t)sel.size(); k++) {
      PairNode nd = pairs[sel[k]];
      for (uint32_t* id : {&nd.id0, &nd.id1}) if (!(*id & kLeafBit)) { const uint32_t c = slot_of[*id / 64u]; *id = c != 0xffffffffu ? tt_local_addr(c) : *id + shift; }
      dst[k] = nd;
    }
    for (uint32_t k : sel) slot_of[k] = 0xffffffffu;
  };
  std::vector<uint32_t> top(kTtNodes);
  for (uint32_t k = 0; k < kTtNodes; k++) top[k] = k;
  { std::vector<uint32_t> slot_of(n_int, 0xffffffffu); copy_into(&trees[(size_t)n_trees * kTtNodes], top, slot_of);
    if (kTtTris > 0) pack_tris(&trees[(size_t)n_trees * kTtNodes], kTtNodes, &packets[(size_t)n_trees * kTtTris * 3u], std::vector<uint32_t>(), nullptr); }
  std::atomic<uint32_t> next_tree{0};
  std::atomic<uint64_t> sum_nodes{0}, n_with{0};
  auto worker = [&]() {
    std::vector<uint32_t> counts(n_int, 0), touched, slot_of(n_int, 0xffffffffu), sel;
    std::vector<uint32_t> tcount(kTtTris > 0 ? tris.size() : 0u, 0u), ttouched;   // leaf visits of this patch's census rays, by the leaf's first triangle
    struct E { uint32_t w; float t; };
    std::vector<E> stack;
    for (;;) {
      const uint32_t t = next_tree.fetch_add(1);
      if (t >= n_trees) break;
      touched.clear();
      for (uint32_t ri = first[t]; ri < first[t + 1]; ri++) {
        const CRay& ray = rays[order[ri]];
        float inv[3]; bool neg[3];
        for (int k = 0; k < 3; k++) { inv[k] = 1.0f / ray.d[k]; neg[k] = inv[k] < 0.0f; }
        float tmax = INFINITY, tb;
        if (!slab(root_box, root_box + 3, ray.o, inv, &tb)) continue;
        stack.clear();
        uint32_t cur = 0u;
        for (;;) {
          if (!(cur & kLeafBit)) {
            const uint32_t k = cur / 64u;
            if (counts[k]++ == 0) touched.push_back(k);
            const PairNode& nd = pairs[k];
            const float b0min[3] = {nd.xy0[0], nd.xy0[1], nd.zz[0]}, b0max[3] = {nd.xy0[2], nd.xy0[3], nd.zz[1]};
            const float b1min[3] = {nd.xy1[0], nd.xy1[1], nd.zz[2]}, b1max[3] = {nd.xy1[2], nd.xy1[3], nd.zz[3]};
            float t0, t1;
            const bool h0 = slab(b0min, b0max, ray.o, inv, &t0), h1 = slab(b1min, b1max, ray.o, inv, &t1);
            const bool sf = neg[nd.axis & 3u];
            const uint32_t id_near = sf ? nd.id1 : nd.id0, id_far = sf ? nd.id0 : nd.id1;
            const bool h_near = sf ? h1 : h0, h_far = sf ? h0 : h1;
            const float t_near = sf ? t1 : t0, t_far = sf ? t0 : t1;
            if (h_far) stack.push_back(E{id_far, t_far});
            if (h_near && t_near < tmax) { cur = id_near; continue; }
          } else if (!(cur & kSpecialLeaf)) {
            uint32_t lf = cur & 0x7ffffu, ln = (cur >> 19) & kLeafCountMask;
            if (kTtTris > 0) { if (tcount[lf]++ == 0) ttouched.push_back(lf); }
            for (; ln; lf++, ln--) {
              const Tri<float>& tr = tris[lf];
              const float e1[3] = {tr.p1[0] - tr.p0[0], tr.p1[1] - tr.p0[1], tr.p1[2] - tr.p0[2]}, e2[3] = {tr.p2[0] - tr.p0[0], tr.p2[1] - tr.p0[1], tr.p2[2] - tr.p0[2]};
              const float* d = ray.d;
              const float pv[3] = {d[1] * e2[2] - d[2] * e2[1], d[2] * e2[0] - d[0] * e2[2], d[0] * e2[1] - d[1] * e2[0]};
              const float det = e1[0] * pv[0] + e1[1] * pv[1] + e1[2] * pv[2];
              if (det > -1e-7f && det < 1e-7f) continue;
              const float f = 1.0f / det, tv[3] = {ray.o[0] - tr.p0[0], ray.o[1] - tr.p0[1], ray.o[2] - tr.p0[2]};
              const float u = f * (tv[0] * pv[0] + tv[1] * pv[1] + tv[2] * pv[2]);
              if (u < 0.0f || u > 1.0f) continue;
              const float qv[3] = {tv[1] * e1[2] - tv[2] * e1[1], tv[2] * e1[0] - tv[0] * e1[2], tv[0] * e1[1] - tv[1] * e1[0]};
              const float v = f * (d[0] * qv[0] + d[1] * qv[1] + d[2] * qv[2]);
              if (v < 0.0f || u + v > 1.0f) continue;
              const float tt = f * (e2[0] * qv[0] + e2[1] * qv[1] + e2[2] * qv[2]);
              if (tt >= 1e-7f) tmax = tt;
            }
          }
          bool got = false;
          while (!stack.empty()) { const E e = stack.back(); stack.pop_back(); if (e.t < tmax) { cur = e.w; got = true; break; } }
          if (!got) break;
        }
      }
      PairNode* dst = &trees[(size_t)t * kTtNodes];
      if (touched.empty()) {
        memcpy(dst, &trees[(size_t)n_trees * kTtNodes], kTtNodes * sizeof(PairNode));
        if (kTtTris > 0) memcpy(&packets[(size_t)t * kTtTris * 3u], &packets[(size_t)n_trees * kTtTris * 3u], (size_t)kTtTris * 3u * sizeof(Float4));
        continue;
      }
      std::sort(touched.begin(), touched.end(), [&](uint32_t a, uint32_t b) { return counts[a] != counts[b] ? counts[a] > counts[b] : a < b; });
      sel.assign(touched.begin(), touched.begin() + std::min<size_t>(touched.size(), kTtNodes));
      if (sel.size() < kTtNodes) {   // room left: children of the chosen nodes, the most visited parents' first
        std::priority_queue<std::pair<float, uint32_t>> cand;
        for (uint32_t k : sel) slot_of[k] = 0u;
        auto offer = [&](uint32_t k, float pr) { const PairNode& nd = pairs[k]; for (uint32_t id : {nd.id0, nd.id1}) if (!(id & kLeafBit) && slot_of[id / 64u] == 0xffffffffu) cand.push({pr, id / 64u}); };
        for (uint32_t k : sel) offer(k, 0.5f * (float)counts[k]);
        while (sel.size() < kTtNodes && !cand.empty()) {
          const auto c = cand.top(); cand.pop();
          if (slot_of[c.second] != 0xffffffffu) continue;
          sel.push_back(c.second); slot_of[c.second] = 0u;
          offer(c.second, 0.5f * c.first);
        }
        for (uint32_t k : sel) slot_of[k] = 0xffffffffu;
      }
      std::sort(sel.begin(), sel.end());
      copy_into(dst, sel, slot_of);
      if (kTtTris > 0) {
        uint64_t served = 0, all = 0;
        for (uint32_t lf : ttouched) all += tcount[lf];
        pack_tris(dst, (uint32_t)sel.size(), &packets[(size_t)t * kTtTris * 3u], tcount, &served);
        sum_local_tests += served; sum_tests += all;
        for (uint32_t lf : ttouched) tcount[lf] = 0;
        ttouched.clear();
      }
      sum_nodes += touched.size(); n_with++;
      for (uint32_t k : touched) counts[k] = 0;
    }
  };
  {
    // (an exception escaping a std::thread terminates the process: a worker that runs out of memory leaves the scene without tile trees instead)
    std::atomic<bool> failed{false};
    auto guarded_worker = [&]() { try { worker(); } catch (...) { failed = true; next_tree = n_trees; } };
    const unsigned nt = std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
    std::vector<std::thread> pool;
    for (unsigned k = 0; k < nt; k++) pool.emplace_back(guarded_worker);
    for (auto& th : pool) th.join();
    if (failed) { res.failed = true; return res; }
  }
  const size_t kFront = kTtLocalBytes / sizeof(PairNode);
  std::vector<PairNode>& shifted = res.shifted;
  shifted.resize(kFront + n_int);
  memset(shifted.data(), 0, kFront * sizeof(PairNode));
  for (size_t i = 0; i < n_int; i++) {
    PairNode nd = pairs[i];
    for (uint32_t* id : {&nd.id0, &nd.id1}) if (!(*id & kLeafBit)) *id += shift;
    shifted[kFront + i] = nd;
  }
  res.sum_local_tests = sum_local_tests; res.sum_tests = sum_tests; res.sum_nodes = sum_nodes; res.n_with = n_with;
  return res;
}

}  // namespace rrtd
