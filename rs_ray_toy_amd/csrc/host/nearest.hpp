// Nearest-surface point queries (rrt_nearest, include/rrt.h): the closest point on one triangle, the box distance, the prune bound and the walk over
// the linear tree - plain C++ that hipcc compiles for the device and g++ for the host (tools/nearest_check.cpp runs the same walk on the CPU).
// Nothing here is contracted to an fma (the pragma below in every function that computes; the host build has -ffp-contract=off), so every
// instantiation of nearest_on_triangle - the generic kernel, the pair-node kernel, its rare path - rounds alike.
#pragma once
#include <stdint.h>

#include "records.hpp"

#if defined(__HIP__)
#define RRT_NN_FN __host__ __device__ __forceinline__
#else
#define RRT_NN_FN inline
#endif
#if defined(__clang__)
#define RRT_NN_EXACT _Pragma("clang fp contract(off)")
#else
#define RRT_NN_EXACT
#endif

namespace rrtd {

template <typename R> struct NnConst;
template <> struct NnConst<float> { static constexpr float eps = 5.9604645e-8f; static constexpr float inf = __builtin_huge_valf(); };             // 2^-24
template <> struct NnConst<double> { static constexpr double eps = 1.1102230246251565e-16; static constexpr double inf = __builtin_huge_val(); };   // 2^-53
RRT_NN_FN float nn_sqrt(float x) { return __builtin_sqrtf(x); }
RRT_NN_FN double nn_sqrt(double x) { return __builtin_sqrt(x); }

// The prune margin. A subtree may be skipped only when NO triangle under it can win or tie, i.e. when every computed d2 under it exceeds the best one.
// With u = NnConst<R>::eps and M = the largest coordinate the call meets (the root box, and for kept instances the sums |m_ij| |v_j| + |t_i| of the
// vertex transform: Handle::upload_scene), per axis:
//   the computed closest point q = a + ((b - a) b1 + (c - a) b2): b - a and c - a round by 2 M u each, the two products by 2 M u each and inherit the
//     differences' errors, their sum by 2 M u, the final sum by M u, and b1 + b2 may exceed 1 by one rounding (2 M u of overshoot): 13 M u;
//   a kept instance's vertex m v + t: three products and three sums on operands that were themselves rounded from f64, 6 M u away from the f64 vertex
//     the (outward rounded) box was built around: 6 M u.
// Over three axes the computed point of a triangle lies within sqrt(3) (13 + 6) M u < 33 M u of a point the box contains, so
//   sqrt(d2 computed) >= (sqrt(d2 of the box) - 33 M u) (1 - 3 u),
// the last factor for p - q, the squares and their sum. kNearestPadUlps = 48 leaves a margin over the 33; the relative roundings - of the box
// distance (one subtraction, one square and the sums: 4 u), of the triangle distance (3 u), of the bound itself (sqrt, sum, square: 4 u) - are covered
// by the factor 1 + 16 u. A box is skipped iff  d2_box > (sqrt(best d2) + 48 M u)^2 (1 + 16 u)  - the right side changes only when the best does.
// The comparison is written so that a NaN box distance (no box has one: nn_box_d2 drops NaN terms) or an infinite bound never skips.
constexpr int kNearestPadUlps = 48;
template <typename R>
RRT_NN_FN R nn_prune_bound(R best_d2, R delta) {
  RRT_NN_EXACT
  const R s = nn_sqrt(best_d2) + delta;
  return (s * s) * (R(1) + R(16) * NnConst<R>::eps);
}

// squared distance from p to a box: max(bmin - p, p - bmax, 0) per axis (a NaN term counts as 0: never a reason to skip)
template <typename R>
RRT_NN_FN R nn_box_d2(R mnx, R mny, R mnz, R mxx, R mxy, R mxz, R px, R py, R pz) {
  RRT_NN_EXACT
  const R ax = mnx - px, bx = px - mxx, ay = mny - py, by = py - mxy, az = mnz - pz, bz = pz - mxz;
  R ex = ax > bx ? ax : bx, ey = ay > by ? ay : by, ez = az > bz ? az : bz;
  ex = ex > R(0) ? ex : R(0); ey = ey > R(0) ? ey : R(0); ez = ez > R(0) ? ez : R(0);
  return (ex * ex + ey * ey) + ez * ez;
}

template <typename R>
RRT_NN_FN R nn_dot(R ax, R ay, R az, R bx, R by, R bz) {
  RRT_NN_EXACT
  return (ax * bx + ay * by) + az * bz;
}

// The closest point on triangle (a, b, c) to p by the Voronoi-region test (Ericson, Real-Time Collision Detection 5.1.5), in the operation order
// include/rrt.h writes down. The result depends on (p, a, b, c) alone. A degenerate triangle may give NaN barycentrics and a NaN d2.
template <typename R> struct NnSite { R b1, b2, d2; };
template <typename R>
RRT_NN_FN NnSite<R> nearest_on_triangle(R px, R py, R pz, const R* a, const R* b, const R* c) {
  RRT_NN_EXACT
  const R abx = b[0] - a[0], aby = b[1] - a[1], abz = b[2] - a[2];
  const R acx = c[0] - a[0], acy = c[1] - a[1], acz = c[2] - a[2];
  const R apx = px - a[0], apy = py - a[1], apz = pz - a[2];
  const R d1 = nn_dot(abx, aby, abz, apx, apy, apz), d2 = nn_dot(acx, acy, acz, apx, apy, apz);
  const R bpx = px - b[0], bpy = py - b[1], bpz = pz - b[2];
  const R d3 = nn_dot(abx, aby, abz, bpx, bpy, bpz), d4 = nn_dot(acx, acy, acz, bpx, bpy, bpz);
  const R cpx = px - c[0], cpy = py - c[1], cpz = pz - c[2];
  const R d5 = nn_dot(abx, aby, abz, cpx, cpy, cpz), d6 = nn_dot(acx, acy, acz, cpx, cpy, cpz);
  const R vc = d1 * d4 - d3 * d2, vb = d5 * d2 - d1 * d6, va = d3 * d6 - d5 * d4;
  R b1, b2;
  if (d1 <= R(0) && d2 <= R(0)) { b1 = R(0); b2 = R(0); }                            // vertex a
  else if (d3 >= R(0) && d4 <= d3) { b1 = R(1); b2 = R(0); }                         // vertex b
  else if (vc <= R(0) && d1 >= R(0) && d3 <= R(0)) { b1 = d1 / (d1 - d3); b2 = R(0); }   // edge ab
  else if (d6 >= R(0) && d5 <= d6) { b1 = R(0); b2 = R(1); }                         // vertex c
  else if (vb <= R(0) && d2 >= R(0) && d6 <= R(0)) { b1 = R(0); b2 = d2 / (d2 - d6); }   // edge ac
  else if (va <= R(0) && (d4 - d3) >= R(0) && (d5 - d6) >= R(0)) {                   // edge bc
    const R w = (d4 - d3) / ((d4 - d3) + (d5 - d6));
    b1 = R(1) - w; b2 = w;
  } else {                                                                           // the face
    const R den = R(1) / ((va + vb) + vc);
    b1 = vb * den; b2 = vc * den;
  }
  // b1, b2 >= 0 exactly (a quotient of the device's fast division may come out one ulp below 0 or above 1; NaN passes through)
  if (b1 < R(0)) b1 = R(0);
  if (b2 < R(0)) b2 = R(0);
  if (b1 > R(1)) b1 = R(1);
  if (b2 > R(1)) b2 = R(1);
  const R qx = a[0] + (abx * b1 + acx * b2), qy = a[1] + (aby * b1 + acy * b2), qz = a[2] + (abz * b1 + acz * b2);
  const R ex = px - qx, ey = py - qy, ez = pz - qz;
  NnSite<R> s;
  s.b1 = b1; s.b2 = b2; s.d2 = (ex * ex + ey * ey) + ez * ez;
  return s;
}

// The best candidate so far. prim = kNnNone until one wins. A candidate wins with a smaller d2, or an equal d2 and a smaller index: both
// comparisons are false for a NaN d2, which therefore never wins.
constexpr int32_t kNnNone = 0x7fffffff;
template <typename R> struct NnBest { R d2, b1, b2; int32_t prim; };
template <typename R>
RRT_NN_FN NnBest<R> nn_none() { NnBest<R> b; b.d2 = NnConst<R>::inf; b.b1 = R(0); b.b2 = R(0); b.prim = kNnNone; return b; }

// one entry of the triangle array against p. SPECIAL: the entry may be a sphere (no candidate) or a triangle of a kept instance (raw vertices
// through InstDev::m, in R)
template <typename R, bool SPECIAL>
RRT_NN_FN bool nn_consider(NnBest<R>& best, const Tri<R>& tr, const InstDev<R>* insts, uint32_t idx, R px, R py, R pz) {
  RRT_NN_EXACT
  R a[3], b[3], c[3];
  for (int k = 0; k < 3; k++) { a[k] = tr.p0[k]; b[k] = tr.p1[k]; c[k] = tr.p2[k]; }
  if (SPECIAL) {
    if (tr.plane == kSphereMark) return false;
    if ((tr.material & kInstFlag) != 0u) {
      const R* m = insts[(tr.material >> 16) & 0x7fffu].m;
      R* const v[3] = {a, b, c};
      for (int j = 0; j < 3; j++) {
        const R x = v[j][0], y = v[j][1], z = v[j][2];
        for (int k = 0; k < 3; k++) v[j][k] = ((m[4 * k] * x + m[4 * k + 1] * y) + m[4 * k + 2] * z) + m[4 * k + 3];
      }
    }
  }
  const NnSite<R> s = nearest_on_triangle<R>(px, py, pz, a, b, c);
  if (s.d2 < best.d2 || (s.d2 == best.d2 && (int32_t)idx < best.prim)) {
    best.d2 = s.d2; best.b1 = s.b1; best.b2 = s.b2; best.prim = (int32_t)idx;
    return true;
  }
  return false;
}

// The walk over the linear tree (first child at i + 1, second at Node::offset), one query. Near child first; the far child is pushed if its box is
// within the bound and judged again when popped, against the bound of that moment. Near-first pushes at most one entry per level, so the tree depth
// bounds the stack (stack_cap entries). A node is handled at most once and popped at most once: 2 n_nodes + 2 steps bound the loop. Returns false
// - never spins, never writes past the stack - if either bound is broken (a tree that is none).
// prune0 = the bound to start with: nn_prune_bound of the squared search radius (inf: none).
template <typename R, typename Stack>
RRT_NN_FN bool nearest_walk(const Node<R>* nodes, uint32_t n_nodes, const Tri<R>* tris, uint32_t n_tris, const InstDev<R>* insts, R px, R py, R pz, R prune0, R delta,
                            Stack& st, uint32_t stack_cap, NnBest<R>* out) {
  NnBest<R> best = nn_none<R>();
  *out = best;
  if (n_nodes == 0u) return true;
  R prune = prune0;
  const uint32_t limit = 2u * n_nodes + 2u;
  uint32_t cur = 0u, sp = 0u, steps = 0u;
  Node<R> nd = nodes[0];
  bool have = !(nn_box_d2<R>(nd.bmin[0], nd.bmin[1], nd.bmin[2], nd.bmax[0], nd.bmax[1], nd.bmax[2], px, py, pz) > prune);
  while (true) {
    if (++steps > limit) return false;
    if (have) {
      const uint32_t np = nd.meta >> 2;
      if (np > 0u) {
        if (nd.offset > n_tris || np > n_tris - nd.offset) return false;
        bool better = false;
        for (uint32_t i = 0; i < np; i++) better |= nn_consider<R, true>(best, tris[nd.offset + i], insts, nd.offset + i, px, py, pz);
        if (better) { const R b = nn_prune_bound<R>(best.d2, delta); if (b < prune) prune = b; }
        have = false;
      } else {
        const uint32_t c0 = cur + 1u, c1 = nd.offset;
        if (c0 >= n_nodes || c1 >= n_nodes) return false;
        const Node<R> n0 = nodes[c0], n1 = nodes[c1];
        const R e0 = nn_box_d2<R>(n0.bmin[0], n0.bmin[1], n0.bmin[2], n0.bmax[0], n0.bmax[1], n0.bmax[2], px, py, pz);
        const R e1 = nn_box_d2<R>(n1.bmin[0], n1.bmin[1], n1.bmin[2], n1.bmax[0], n1.bmax[1], n1.bmax[2], px, py, pz);
        const bool second = e1 < e0;
        const R e_near = second ? e1 : e0, e_far = second ? e0 : e1;
        if (!(e_far > prune)) {
          if (sp >= stack_cap) return false;
          st.put(sp++, second ? c0 : c1);
        }
        if (!(e_near > prune)) { cur = second ? c1 : c0; nd = second ? n1 : n0; }
        else have = false;
      }
    }
    if (!have) {
      if (sp == 0u) break;
      cur = st.get(--sp);
      if (cur >= n_nodes) return false;
      nd = nodes[cur];
      have = !(nn_box_d2<R>(nd.bmin[0], nd.bmin[1], nd.bmin[2], nd.bmax[0], nd.bmax[1], nd.bmax[2], px, py, pz) > prune);
    }
  }
  *out = best;
  return true;
}

// what a query reports: accepted iff a candidate won and dist <= max_dist; otherwise prim = -1, b1 = b2 = 0, dist = max_dist
template <typename R> struct NnOut { int32_t prim; R b1, b2, dist; };
template <typename R>
RRT_NN_FN NnOut<R> nn_result(const NnBest<R>& best, R max_dist) {
  NnOut<R> o;
  o.prim = -1; o.b1 = R(0); o.b2 = R(0); o.dist = max_dist;
  if (best.prim != kNnNone) {
    const R dist = nn_sqrt(best.d2);
    if (dist <= max_dist) { o.prim = best.prim; o.b1 = best.b1; o.b2 = best.b2; o.dist = dist; }
  }
  return o;
}
// the bound a call starts from: no candidate farther than max_dist is accepted, so none needs to be found (4 u: the product, and sqrt(d2) <= max_dist
// leaves d2 <= max_dist^2 (1 + 2 u))
template <typename R>
RRT_NN_FN R nn_prune_start(R max_dist, R delta) {
  RRT_NN_EXACT
  return nn_prune_bound<R>((max_dist * max_dist) * (R(1) + R(4) * NnConst<R>::eps), delta);
}
RRT_NN_FN bool nn_finite(float x) { return (x - x) == 0.0f; }
RRT_NN_FN bool nn_finite(double x) { return (x - x) == 0.0; }

}  // namespace rrtd
