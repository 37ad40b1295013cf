// All hits along a ray, in order (rrt_trace_all, include/rrt.h): the triangle test, the slab test, the sorted insert and the walk over the linear
// tree - plain C++ that hipcc compiles for the device and g++ for the host (tools/trace_all_check.cpp runs the same walk on the CPU).
// Nothing here is contracted to an fma (the pragma of nearest.hpp in every function that computes; the host build has -ffp-contract=off), and the two
// divisions (1 / det, 1 / d) are IEEE divisions in every build: the fp32 device code is compiled with the fast reciprocal, so a float quotient is
// taken in double and rounded once more - 53 >= 2 x 24 + 2 bits, which makes the double rounding innocuous for a quotient of two floats.
#pragma once
#include <stdint.h>

#include "nearest.hpp"   // RRT_NN_FN, RRT_NN_EXACT, NnConst, nn_finite
#include "records.hpp"

namespace rrtd {

constexpr int kMaxHits = 16;   // RRT_MAX_HITS

RRT_NN_FN float mh_div(float a, float b) { return (float)((double)a / (double)b); }
RRT_NN_FN double mh_div(double a, double b) { return a / b; }

// 1 + 2 gamma(3), gamma(n) = n eps / (1 - n eps): the factor Bounds3::intersect_p widens a far distance by
template <typename R>
RRT_NN_FN R mh_far_factor() { return R(1) + R(2) * ((R(3) * NnConst<R>::eps) / (R(1) - R(3) * NnConst<R>::eps)); }

// The pad of the node boxes for scenes with kept (non-rigid) instances. A node box is the f64 box of the f64 world vertices, narrowed outward; the
// walk forms a kept instance's vertex m v + t in R: three products and three sums on operands that were themselves rounded from f64, at most 6 M u
// away from the f64 vertex per axis (u = NnConst<R>::eps, M = the largest sum |m_ij| |v_j| + |t_i| and root-box coordinate: Handle::upload_scene, the
// same M as kNearestPadUlps is used with). So the candidate's own box may leave its node's box by 6 M u. The grown bounds lo - delta and hi + delta
// are themselves rounded, by at most M u (|lo|, delta <= M): 7 M u in all, kMultihitPadUlps = 8. With every node box grown by
// delta = 8 u M a node contains the own boxes of the entries under it, and by the monotonicity of rounding ((lo - o) * inv is monotone in lo for a
// fixed o and inv) the node passes mh_slab whenever one of those own boxes does. Rigid entries need no pad - their vertices are the f64 ones rounded
// to nearest, which cannot leave a box rounded outward -, and scenes without kept instances walk with delta = 0 through the same code (x - 0 = x).
constexpr int kMultihitPadUlps = 8;

template <typename R>
struct MhRay {
  R o[3], d[3], inv[3], tmax;
};
// false = a dead ray: a non-finite origin, direction or tmax (+inf is legal) or a zero direction
template <typename R>
RRT_NN_FN bool mh_make_ray(R ox, R oy, R oz, R dx, R dy, R dz, R tmax, MhRay<R>* r) {
  r->o[0] = ox; r->o[1] = oy; r->o[2] = oz; r->d[0] = dx; r->d[1] = dy; r->d[2] = dz; r->tmax = tmax;
  for (int k = 0; k < 3; k++) r->inv[k] = mh_div(R(1), r->d[k]);
  const bool fin = nn_finite(ox) && nn_finite(oy) && nn_finite(oz) && nn_finite(dx) && nn_finite(dy) && nn_finite(dz);
  const bool t_ok = nn_finite(tmax) || tmax == NnConst<R>::inf;
  return fin && t_ok && !(dx == R(0) && dy == R(0) && dz == R(0));
}

// (i) Moller-Trumbore in tri_closest's operation order (device/dkernels.hpp), without a double-float origin; the result depends on (o, d, a, b, c) alone
template <typename R> struct MhHit { R t, u, v; };
template <typename R>
RRT_NN_FN bool mh_triangle(const MhRay<R>& r, const R* a, const R* b, const R* c, MhHit<R>* h) {
  RRT_NN_EXACT
  const R e1x = b[0] - a[0], e1y = b[1] - a[1], e1z = b[2] - a[2];
  const R e2x = c[0] - a[0], e2y = c[1] - a[1], e2z = c[2] - a[2];
  const R px = r.d[1] * e2z - r.d[2] * e2y, py = r.d[2] * e2x - r.d[0] * e2z, pz = r.d[0] * e2y - r.d[1] * e2x;
  const R det = (e1x * px + e1y * py) + e1z * pz;
  if (det > R(-0.0000001) && det < R(0.0000001)) return false;
  const R f = mh_div(R(1), det);
  const R tx = r.o[0] - a[0], ty = r.o[1] - a[1], tz = r.o[2] - a[2];
  const R u = f * ((tx * px + ty * py) + tz * pz);
  if (!(u >= R(0) && u <= R(1))) return false;
  const R qx = ty * e1z - tz * e1y, qy = tz * e1x - tx * e1z, qz = tx * e1y - ty * e1x;
  const R v = f * ((r.d[0] * qx + r.d[1] * qy) + r.d[2] * qz);
  if (!(v >= R(0) && (u + v) <= R(1))) return false;
  const R t = f * ((e2x * qx + e2y * qy) + e2z * qz);
  if (!(t >= R(0.0000001))) return false;
  h->t = t; h->u = u; h->v = v;
  return true;
}

// (iii) the slab test, for a candidate's own box and for the node boxes alike: near and far per axis, far widened, a NaN term dropped
// (every comparison with one is false), pass iff max(nears, 0) <= min(fars, tmax)
template <typename R>
RRT_NN_FN bool mh_slab(const R* lo, const R* hi, const MhRay<R>& r, R delta) {
  RRT_NN_EXACT
  const R g = mh_far_factor<R>();
  R tn = R(0), tf = r.tmax;
  for (int k = 0; k < 3; k++) {
    const R l = lo[k] - delta, h = hi[k] + delta;
    const bool neg = r.inv[k] < R(0);
    const R nr = ((neg ? h : l) - r.o[k]) * r.inv[k];
    const R fr = (((neg ? l : h) - r.o[k]) * r.inv[k]) * g;
    if (nr > tn) tn = nr;
    if (fr < tf) tf = fr;
  }
  return tn <= tf;
}

// The world vertices of entry `tr` as the handle stores them: false for a sphere; a kept instance's raw vertices through InstDev::m, in R
template <typename R>
RRT_NN_FN bool mh_vertices(const Tri<R>& tr, const InstDev<R>* insts, R* a, R* b, R* c) {
  RRT_NN_EXACT
  if (tr.plane == kSphereMark) return false;
  for (int k = 0; k < 3; k++) { a[k] = tr.p0[k]; b[k] = tr.p1[k]; c[k] = tr.p2[k]; }
  if ((tr.material & kInstFlag) != 0u) {
    const R* m = insts[(tr.material >> 16) & 0x7fffu].m;
    R* const v[3] = {a, b, c};
    for (int j = 0; j < 3; j++) {
      const R x = v[j][0], y = v[j][1], z = v[j][2];
      for (int k = 0; k < 3; k++) v[j][k] = ((m[4 * k] * x + m[4 * k + 1] * y) + m[4 * k + 2] * z) + m[4 * k + 3];
    }
  }
  return true;
}

// acceptance of one entry: (i) the triangle test, (ii) t < tmax, (iii) the slab test of its own box (delta = 0: the vertices are the computed ones).
// The three are a conjunction of functions of (ray, a, b, c) alone, so their order is free: (iii) goes first - it needs no division and turns away
// most entries of a leaf.
template <typename R>
RRT_NN_FN bool mh_accept(const MhRay<R>& r, const Tri<R>& tr, const InstDev<R>* insts, MhHit<R>* h) {
  R a[3], b[3], c[3];
  if (!mh_vertices<R>(tr, insts, a, b, c)) return false;
  R lo[3], hi[3];
  for (int k = 0; k < 3; k++) {
    R l = a[k], m = a[k];
    if (b[k] < l) l = b[k];
    if (c[k] < l) l = c[k];
    if (b[k] > m) m = b[k];
    if (c[k] > m) m = c[k];
    lo[k] = l; hi[k] = m;
  }
  if (!mh_slab<R>(lo, hi, r, R(0))) return false;
  if (!mh_triangle<R>(r, a, b, c, h)) return false;
  return h->t < r.tmax;
}

// The sorted insert into a buffer of k slots of which `held` = min(k, accepted so far) are filled, ordered by (t, index) ascending. Buf: t(s), prim(s),
// set(s, t, prim). The k smallest of a set under a strict total order do not depend on the order of arrival. Shifts from the tail.
template <typename R, typename Buf>
RRT_NN_FN void mh_insert(Buf& buf, uint32_t k, uint32_t held, R t, int32_t idx) {
  if (k == 0u) return;
  uint32_t j = held;
  if (held == k) {
    const R tl = buf.t(k - 1u);
    if (!(t < tl || (t == tl && idx < buf.prim(k - 1u)))) return;
    j = k - 1u;
  }
  while (j > 0u) {
    const R tp = buf.t(j - 1u);
    const int32_t pp = buf.prim(j - 1u);
    if (!(t < tp || (t == tp && idx < pp))) break;
    buf.set(j, tp, pp);
    j--;
  }
  buf.set(j, t, idx);
}

// The walk over the linear tree (first child at i + 1, second at Node::offset), one ray: every node whose (grown) box passes the slab test is opened,
// every entry of such a leaf is judged by mh_accept. An interior node fetches and judges both children at once (two loads in flight instead of one
// after the other); first child first, the second pushed only if it passed: at most one entry per level, so the tree depth bounds the stack
// (stack_cap entries); a node is handled at most once: 2 n_nodes + 2 steps bound the loop. Returns false - never spins, never writes past the stack -
// if either bound is broken or a word points outside its array (a tree that is none).
// Nothing is pruned by t: a candidate's computed t and the computed near distance of a box around it are two roundings of nearly the same number where
// the box is flat (an axis-aligned face), so a k-th t between them would drop a hit the scan keeps. The slab test keeps the caller's tmax throughout.
// *count = the number of accepted candidates; the buffer holds the min(k, *count) first of them in (t, index) order.
template <typename R, typename Stack, typename Buf>
RRT_NN_FN bool multihit_walk(const Node<R>* nodes, uint32_t n_nodes, const Tri<R>* tris, uint32_t n_tris, const InstDev<R>* insts, const MhRay<R>& r, int32_t skip, R delta,
                             Stack& st, uint32_t stack_cap, Buf& buf, uint32_t k, uint32_t* count) {
  uint32_t n_acc = 0u;
  *count = 0u;
  if (n_nodes == 0u) return true;
  const uint32_t limit = 2u * n_nodes + 2u;
  uint32_t cur = 0u, sp = 0u, steps = 0u;
  Node<R> nd = nodes[0];
  bool have = mh_slab<R>(nd.bmin, nd.bmax, r, delta);   // nd = nodes[cur], and its box passed
  while (true) {
    if (++steps > limit) return false;
    if (have) {
      const uint32_t np = nd.meta >> 2;
      if (np > 0u) {
        if (nd.offset > n_tris || np > n_tris - nd.offset) return false;
        for (uint32_t i = 0; i < np; i++) {
          const uint32_t idx = nd.offset + i;
          if ((int32_t)idx == skip) continue;
          MhHit<R> h;
          if (!mh_accept<R>(r, tris[idx], insts, &h)) continue;
          mh_insert<R>(buf, k, n_acc < k ? n_acc : k, h.t, (int32_t)idx);
          n_acc++;
        }
        have = false;
      } else {
        const uint32_t c0 = cur + 1u, c1 = nd.offset;
        if (c0 >= n_nodes || c1 >= n_nodes) return false;
        const Node<R> n0 = nodes[c0], n1 = nodes[c1];
        const bool h0 = mh_slab<R>(n0.bmin, n0.bmax, r, delta), h1 = mh_slab<R>(n1.bmin, n1.bmax, r, delta);
        if (h0 && h1) {
          if (sp >= stack_cap) return false;
          st.put(sp++, c1);
        }
        if (h0) { cur = c0; nd = n0; }
        else if (h1) { cur = c1; nd = n1; }
        else have = false;
      }
    }
    if (!have) {
      if (sp == 0u) break;
      cur = st.get(--sp);
      if (cur >= n_nodes) return false;
      nd = nodes[cur];   // (its box passed when it was pushed)
      have = true;
    }
  }
  *count = n_acc;
  return true;
}

// the scan the call is defined as: every entry in index order (tools/trace_all_check.cpp, and a root that is a single leaf walks exactly this)
template <typename R, typename Buf>
RRT_NN_FN uint32_t multihit_scan(const Tri<R>* tris, uint32_t n_tris, const InstDev<R>* insts, const MhRay<R>& r, int32_t skip, Buf& buf, uint32_t k) {
  uint32_t n_acc = 0u;
  for (uint32_t idx = 0; idx < n_tris; idx++) {
    if ((int32_t)idx == skip) continue;
    MhHit<R> h;
    if (!mh_accept<R>(r, tris[idx], insts, &h)) continue;
    mh_insert<R>(buf, k, n_acc < k ? n_acc : k, h.t, (int32_t)idx);
    n_acc++;
  }
  return n_acc;
}

// b1, b2 of a surviving slot: the triangle test again - the same function on the same operands, the same bits
template <typename R>
RRT_NN_FN MhHit<R> mh_rehit(const MhRay<R>& r, const Tri<R>& tr, const InstDev<R>* insts) {
  MhHit<R> h;
  h.t = r.tmax; h.u = R(0); h.v = R(0);
  R a[3], b[3], c[3];
  if (mh_vertices<R>(tr, insts, a, b, c)) mh_triangle<R>(r, a, b, c, &h);
  return h;
}

}  // namespace rrtd
