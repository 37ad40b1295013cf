// Mutual visibility of point sets (rrt_visibility, include/rrt.h): the segment between two points, the walk that stops at the first accepted
// candidate and the scan the call is defined as - plain C++ that hipcc compiles for the device and g++ for the host (tools/visibility_check.cpp runs
// the same walk on the CPU). The candidate tests are multihit.hpp's (mh_make_ray, mh_accept, mh_slab) on the same operands, so a pair is blocked
// exactly where rrt_trace_all would count a hit on the pair's ray. Nothing is contracted to an fma; divisions and square roots are IEEE in every
// build: the fp32 device code is compiled with the fast reciprocal and square root, so a float quotient or root is taken in double and rounded once
// more - 53 >= 2 x 24 + 2 bits, which makes the double rounding innocuous for both.
#pragma once
#include <stdint.h>

#include "multihit.hpp"

namespace rrtd {

enum { kVisMatrix = 0, kVisPairs = 1 };              // RRT_VIS_MATRIX, RRT_VIS_PAIRS
enum { kVisPoints = 0, kVisDirections = 1 };         // RRT_VIS_POINTS, RRT_VIS_DIRECTIONS
enum { kVisFacingA = 1u, kVisFacingB = 2u };         // RRT_VIS_FACING_A, RRT_VIS_FACING_B

RRT_NN_FN float vis_sqrt(float x) { return (float)__builtin_sqrt((double)x); }
RRT_NN_FN double vis_sqrt(double x) { return __builtin_sqrt(x); }

template <typename R>
RRT_NN_FN R vis_dot(const R* u, const R* v) {
  RRT_NN_EXACT
  return (u[0] * v[0] + u[1] * v[1]) + u[2] * v[2];
}

// One end of a segment: the point moved along its unit normal. nn = n / sqrt(dot(n, n)) per component, q = p + nn * offset; without normals
// nn = 0 and q = p. live = false for a non-finite coordinate, a zero or non-finite normal (or one whose nn is not finite) and a q that is not finite.
template <typename R>
struct VisEnd {
  R q[3], nn[3];
  bool live;
};
template <typename R>
RRT_NN_FN VisEnd<R> vis_end(R px, R py, R pz, bool has_n, R nx, R ny, R nz, R offset) {
  RRT_NN_EXACT
  VisEnd<R> e;
  e.q[0] = px; e.q[1] = py; e.q[2] = pz;
  e.nn[0] = e.nn[1] = e.nn[2] = R(0);
  e.live = nn_finite(px) && nn_finite(py) && nn_finite(pz);
  if (has_n) {
    const R n[3] = {nx, ny, nz};
    const R len = vis_sqrt(vis_dot<R>(n, n));
    for (int k = 0; k < 3; k++) e.nn[k] = mh_div(n[k], len);
    e.live = e.live && nn_finite(nx) && nn_finite(ny) && nn_finite(nz) && !(nx == R(0) && ny == R(0) && nz == R(0)) && nn_finite(e.nn[0]) && nn_finite(e.nn[1]) &&
             nn_finite(e.nn[2]);
    for (int k = 0; k < 3; k++) e.q[k] = e.q[k] + e.nn[k] * offset;
    e.live = e.live && nn_finite(e.q[0]) && nn_finite(e.q[1]) && nn_finite(e.q[2]);
  }
  return e;
}

// The pair's verdict before any candidate is looked at
enum VisVerdict { kVisNo = 0 /* not visible, not traced */, kVisYes = 1 /* visible, nothing to trace (coincident points) */, kVisTrace = 2 /* visible iff not blocked: *r */ };

// a: a live end of set A. POINTS: b a live end of set B, w = b.q - a.q, tmax = |w|. DIRECTIONS: w = b.q (the direction as given; b.nn = 0), tmax = +inf,
// a zero or non-finite direction (or |w|) is a dead column. d = w / |w| per component. Facing is judged on w, before the ray is made.
template <typename R>
RRT_NN_FN VisVerdict vis_segment(const VisEnd<R>& a, const VisEnd<R>& b, int b_kind, uint32_t flags, MhRay<R>* r) {
  RRT_NN_EXACT
  if (!a.live || !b.live) return kVisNo;
  R w[3];
  for (int k = 0; k < 3; k++) w[k] = b_kind == kVisDirections ? b.q[k] : b.q[k] - a.q[k];
  const R len = vis_sqrt(vis_dot<R>(w, w));
  if (!nn_finite(len)) return kVisNo;
  if (len == R(0)) return (b_kind == kVisPoints && flags == 0u) ? kVisYes : kVisNo;
  if ((flags & kVisFacingA) != 0u && !(vis_dot<R>(a.nn, w) > R(0))) return kVisNo;
  if ((flags & kVisFacingB) != 0u && !(vis_dot<R>(b.nn, w) < R(0))) return kVisNo;
  const R tmax = b_kind == kVisDirections ? NnConst<R>::inf : len;
  if (!mh_make_ray<R>(a.q[0], a.q[1], a.q[2], mh_div(w[0], len), mh_div(w[1], len), mh_div(w[2], len), tmax, r)) return kVisNo;
  return kVisTrace;
}

// multihit_walk's loop without the buffer: *blocked = some entry other than skip_a and skip_b is accepted, found at the first such entry the walk
// meets - existence does not depend on the order. The same step and stack bounds; false for a tree that is none.
template <typename R, typename Stack>
RRT_NN_FN bool vis_walk(const Node<R>* nodes, uint32_t n_nodes, const Tri<R>* tris, uint32_t n_tris, const InstDev<R>* insts, const MhRay<R>& r, int32_t skip_a, int32_t skip_b,
                        R delta, Stack& st, uint32_t stack_cap, bool* blocked) {
  *blocked = false;
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
          if ((int32_t)idx == skip_a || (int32_t)idx == skip_b) continue;
          MhHit<R> h;
          if (mh_accept<R>(r, tris[idx], insts, &h)) { *blocked = true; return true; }
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
  return true;
}

// the scan the call is defined as: every entry (tools/visibility_check.cpp)
template <typename R>
RRT_NN_FN bool vis_scan(const Tri<R>* tris, uint32_t n_tris, const InstDev<R>* insts, const MhRay<R>& r, int32_t skip_a, int32_t skip_b) {
  for (uint32_t idx = 0; idx < n_tris; idx++) {
    if ((int32_t)idx == skip_a || (int32_t)idx == skip_b) continue;
    MhHit<R> h;
    if (mh_accept<R>(r, tris[idx], insts, &h)) return true;
  }
  return false;
}

}  // namespace rrtd
