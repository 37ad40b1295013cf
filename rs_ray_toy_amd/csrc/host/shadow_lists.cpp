// Scene preparation, part 4: shadow candidate lists of the fp32 any-hit path (see scene_prep.hpp).
#include "scene_prep.hpp"

#include <algorithm>
#include <cmath>
#include <thread>

namespace rrtd {

// ---- shadow candidate lists of the fp32 any-hit path (dtraverse_f32.hpp "Shadow rays towards delta lights by candidate lists") ----------
// One table per distinct delta-light source (point lights by position - the reference puts every one at the world origin, Q17 -, distant lights
// by direction). Per triangle T: the leaves whose box can meet a shadow ray that starts on T and points at the source. Such a ray is
// q + t u(q), q in T, t in [0, kShadowTmax |d|] with |d| = 1 +- 1e-6; u(q) lies within an angle theta of the centroid's direction u_c
// (point light: tan(theta) <= r_T / sqrt(dist^2 - r_T^2); distant light: theta = 0), so the ray stays within delta = L tan(theta) of the prism
// "T swept along u_c by L". A leaf is a candidate when its box, fattened by delta + slack, meets that prism - decided by a separating-axis
// test over the box axes, the prism's face normals and the edge cross products, which can only err towards "meets". The slack covers what
// separates the fp32 evaluation from this geometry: the ray's origin word is the fp32 rounding of a point of T (<= 1 ulp of the coordinates),
// the boxes are rounded outward, the slab test widens the far planes by 1 + 2 gamma(3): 16 ulp of the largest coordinate + 1e-4 in all.
// Triangles closer to a point light than 8 triangle radii, or with more than kShadowListMax candidates, get no list (the kernel walks the tree).
// [r4] Area lights (lights/diffuse.rs:63-88 -> Shape::sample_ref shape/mod.rs:33-48: a point of the light's shape) are sources too: every point the
// light can sample lies in the shape's bounding sphere (centre C, radius r_L), so the direction from q in T to it stays within theta of u_c with
// sin(theta) <= (r_L + r_T) / dist - the same formula with the light's radius added. With theta of 5-10 degrees one prism fattened by L sin(theta)
// would list a swept volume (w + 2 L sin(theta))^2 L for a ray that stays in a CONE: the sweep is cut into kShadowSegments pieces in the ray
// parameter, piece k = T swept from t_k cos(theta) to t_(k+1) and fattened by t_(k+1) sin(theta) only (a point q + t u of the ray lies within
// t sin(theta) of the axis point q + t' u_c, t' in [t cos(theta), t]); the candidates are the leaves that meet any piece - about half as many.
constexpr int kShadowSegments = 6;   // pieces of the sweep towards an area light (build_shadow_lists)
ShadowListsHost build_shadow_lists(const std::vector<Node<float>>& nodes, const std::vector<Tri<float>>& tris, const rrt_scene_desc* d) {
  ShadowListsHost out;
  out.table_of_light.assign(d->n_lights, 0u);
  if (nodes.empty() || tris.empty()) return out;
  struct Src { int type; double v[3]; double radius; };   // radius: bounding sphere of an area light's shape (0 for point / distant lights)
  std::vector<Src> srcs;
  const ShadowListsHost none{{}, {}, {}, 0u, std::vector<uint32_t>(d->n_lights, 0u)};
  for (size_t i = 0; i < d->n_lights; i++) {
    const rrt_light& l = d->lights[i];
    Src s{l.type, {0, 0, 0}, 0.0};
    if (l.type == RRT_LIGHT_POINT) for (int k = 0; k < 3; k++) s.v[k] = (double)(float)l.p_light[k];
    else if (l.type == RRT_LIGHT_DISTANT) for (int k = 0; k < 3; k++) s.v[k] = (double)(float)l.w_light[k];
    else if (l.type == RRT_LIGHT_DIFFUSE && l.shape_type == RRT_PRIM_SPHERE) {
      // Sphere::sample (sphere.rs:265-285): obj_to_world of a point at distance `radius` from the object-space origin; the Frobenius norm of the linear
      // part bounds its stretch (exact for a rigid transform times a uniform scale / sqrt(3) ... conservative for anything else)
      const rrt_sphere& sp = d->spheres[l.shape];
      const double* m = d->xforms[sp.xform].m;
      if (m[12] != 0.0 || m[13] != 0.0 || m[14] != 0.0 || m[15] != 1.0) return none;
      double fro = 0.0, col[3] = {0, 0, 0};
      for (int r0 = 0; r0 < 3; r0++) for (int c0 = 0; c0 < 3; c0++) { fro += m[4 * r0 + c0] * m[4 * r0 + c0]; col[c0] += m[4 * r0 + c0] * m[4 * r0 + c0]; }
      double offd = 0.0;   // columns orthogonal and of one length: a rotation times a uniform scale
      for (int a0 = 0; a0 < 3; a0++) for (int b0 = a0 + 1; b0 < 3; b0++) { double q = 0; for (int r0 = 0; r0 < 3; r0++) q += m[4 * r0 + a0] * m[4 * r0 + b0]; offd = std::max(offd, std::fabs(q)); }
      const bool uniform = offd <= 1e-12 * fro && std::fabs(col[0] - col[1]) <= 1e-12 * fro && std::fabs(col[0] - col[2]) <= 1e-12 * fro;
      const double stretch = uniform ? std::sqrt(col[0]) : std::sqrt(fro);
      for (int k = 0; k < 3; k++) s.v[k] = m[4 * k + 3];
      s.radius = std::fabs(sp.radius) * stretch * (1.0 + 1e-6) + 1e-6 * (std::fabs(s.v[0]) + std::fabs(s.v[1]) + std::fabs(s.v[2]));
      s.type = RRT_LIGHT_DIFFUSE;
    }
    // (a triangle-shaped area light: Triangle::sample takes its "barycentrics" from a point of the unit SPHERE (triangle.rs:393-418, Q19), so the sampled
    // point is sum b_k q_k with |b_k| <= 1 each - anywhere within |q_0| + |q_1| + |q_2| of the world origin, no useful bound: such a scene keeps the tree walk)
    else return none;
    size_t t = 0;
    for (; t < srcs.size(); t++) if (srcs[t].type == s.type && srcs[t].v[0] == s.v[0] && srcs[t].v[1] == s.v[1] && srcs[t].v[2] == s.v[2] && srcs[t].radius == s.radius) break;
    if (t == srcs.size()) srcs.push_back(s);
    if (t >= 15) return none;
    out.table_of_light[i] = (uint32_t)t + 1u;
  }
  if (srcs.empty()) return out;
  // leaves of the tree
  std::vector<uint32_t> leaf_of(nodes.size(), 0xffffffffu);
  for (size_t i = 0; i < nodes.size(); i++) {
    const uint32_t np = nodes[i].meta >> 2;
    if (np == 0) continue;
    leaf_of[i] = (uint32_t)out.leaves.size();
    LeafRec lr{};
    for (int k = 0; k < 3; k++) { lr.bmin[k] = nodes[i].bmin[k]; lr.bmax[k] = nodes[i].bmax[k]; }
    lr.word = kLeafBit | (np << 19) | nodes[i].offset;
    out.leaves.push_back(lr);
  }
  double coord_max = 0.0;
  for (int k = 0; k < 3; k++) coord_max = std::max(coord_max, std::max(std::fabs((double)nodes[0].bmin[k]), std::fabs((double)nodes[0].bmax[k])));
  const double L = (double)kShadowTmax * (1.0 + 1e-5), slack = 16.0 * coord_max * 1.1920929e-7 + 1e-4;
  const size_t nt = tris.size();
  out.n_tables = (uint32_t)srcs.size();
  out.headers.assign(nt * srcs.size(), 0xffu);
  std::vector<std::vector<uint32_t>> lists(nt * srcs.size());
  auto work = [&](size_t t0, size_t t1) {
    std::vector<uint32_t> stack;
    for (size_t ti = t0; ti < t1; ti++) {
      const Tri<float>& T = tris[ti];
      if (T.plane == kSphereMark || (T.material & kInstFlag) != 0u) continue;   // (not a world-space triangle: no list)
      const double P[3][3] = {{T.p0[0], T.p0[1], T.p0[2]}, {T.p1[0], T.p1[1], T.p1[2]}, {T.p2[0], T.p2[1], T.p2[2]}};
      double c[3], rT = 0.0;
      for (int k = 0; k < 3; k++) c[k] = (P[0][k] + P[1][k] + P[2][k]) / 3.0;
      for (int v = 0; v < 3; v++) rT = std::max(rT, std::sqrt((P[v][0] - c[0]) * (P[v][0] - c[0]) + (P[v][1] - c[1]) * (P[v][1] - c[1]) + (P[v][2] - c[2]) * (P[v][2] - c[2])));
      for (size_t si = 0; si < srcs.size(); si++) {
        double u[3], sin_t = 0.0, cos_t = 1.0;
        int n_seg = 1;
        if (srcs[si].type == RRT_LIGHT_POINT || srcs[si].type == RRT_LIGHT_DIFFUSE) {
          double w[3] = {srcs[si].v[0] - c[0], srcs[si].v[1] - c[1], srcs[si].v[2] - c[2]};
          const double dist = std::sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]);
          const double rho = (rT + srcs[si].radius) * 1.01;    // spread of the ray's two end points around the axis c -> C
          if (srcs[si].type == RRT_LIGHT_POINT ? !(dist > 8.0 * rT) : !(dist > 3.0 * rho)) continue;   // light too close: the directions over T spread too far
          if (!(dist > 0.0)) continue;
          for (int k = 0; k < 3; k++) u[k] = w[k] / dist;
          sin_t = rho / dist; cos_t = std::sqrt(std::max(0.0, 1.0 - sin_t * sin_t));
          if (srcs[si].type == RRT_LIGHT_POINT) { sin_t = sin_t / cos_t; cos_t = 0.0; }   // (round 3's single prism over the whole length, fattened by L tan(theta): the lists of point lights stay what they were)
          else n_seg = kShadowSegments;
        } else {
          const double len = std::sqrt(srcs[si].v[0] * srcs[si].v[0] + srcs[si].v[1] * srcs[si].v[1] + srcs[si].v[2] * srcs[si].v[2]);
          if (!(len > 0.0)) continue;
          for (int k = 0; k < 3; k++) u[k] = srcs[si].v[k] / len;
        }
        // the pieces of the sweep: piece g = T swept along u from a_g to b_g, fattened by m_g; prism vertices and the axes of the separating-axis test
        double E[4][3];   // edge directions: the triangle's three edges and the sweep
        for (int k = 0; k < 3; k++) { E[0][k] = P[1][k] - P[0][k]; E[1][k] = P[2][k] - P[1][k]; E[2][k] = P[0][k] - P[2][k]; E[3][k] = u[k]; }
        auto cross = [](const double* a, const double* b, double* o) { o[0] = a[1] * b[2] - a[2] * b[1]; o[1] = a[2] * b[0] - a[0] * b[2]; o[2] = a[0] * b[1] - a[1] * b[0]; };
        double A[16][3];
        int na = 0;
        cross(E[0], E[1], A[na++]);                                   // the triangle's plane
        for (int e = 0; e < 3; e++) cross(E[e], E[3], A[na++]);      // the three side faces
        for (int e = 0; e < 4; e++) for (int ax = 0; ax < 3; ax++) { const double b[3] = {ax == 0 ? 1.0 : 0.0, ax == 1 ? 1.0 : 0.0, ax == 2 ? 1.0 : 0.0}; cross(E[e], b, A[na++]); }
        struct Piece { double V[6][3], lo[3], hi[3], m; };
        Piece pieces[kShadowSegments];
        for (int g = 0; g < n_seg; g++) {
          const double t0 = L * (double)g / (double)n_seg, t1 = L * (double)(g + 1) / (double)n_seg;
          Piece& pc = pieces[g];
          const double a = t0 * cos_t, b = t1;
          pc.m = t1 * sin_t + slack;
          for (int v = 0; v < 3; v++) for (int k = 0; k < 3; k++) { pc.V[v][k] = P[v][k] + a * u[k]; pc.V[3 + v][k] = P[v][k] + b * u[k]; }
          for (int k = 0; k < 3; k++) { pc.lo[k] = pc.hi[k] = pc.V[0][k]; for (int v = 1; v < 6; v++) { pc.lo[k] = std::min(pc.lo[k], pc.V[v][k]); pc.hi[k] = std::max(pc.hi[k], pc.V[v][k]); } }
        }
        auto meets_piece = [&](const Node<float>& nd, const Piece& pc) {
          double bc[3], bh[3];
          for (int k = 0; k < 3; k++) {
            const double b0 = (double)nd.bmin[k] - pc.m, b1 = (double)nd.bmax[k] + pc.m;
            if (b0 > pc.hi[k] || b1 < pc.lo[k]) return false;   // the box axes
            bc[k] = 0.5 * (b0 + b1); bh[k] = 0.5 * (b1 - b0);
          }
          for (int a = 0; a < na; a++) {
            const double* ax = A[a];
            const double l2 = ax[0] * ax[0] + ax[1] * ax[1] + ax[2] * ax[2];
            if (!(l2 > 1e-30)) continue;   // degenerate axis: decides nothing
            double pmin = 1e300, pmax = -1e300;
            for (int v = 0; v < 6; v++) { const double q = pc.V[v][0] * ax[0] + pc.V[v][1] * ax[1] + pc.V[v][2] * ax[2]; pmin = std::min(pmin, q); pmax = std::max(pmax, q); }
            const double cc = bc[0] * ax[0] + bc[1] * ax[1] + bc[2] * ax[2], rr = bh[0] * std::fabs(ax[0]) + bh[1] * std::fabs(ax[1]) + bh[2] * std::fabs(ax[2]);
            if (cc - rr > pmax || cc + rr < pmin) return false;
          }
          return true;
        };
        auto meets = [&](const Node<float>& nd) { for (int g = 0; g < n_seg; g++) if (meets_piece(nd, pieces[g])) return true; return false; };
        std::vector<uint32_t>& list = lists[si * nt + ti];
        bool too_many = false;
        stack.clear(); stack.push_back(0u);
        while (!stack.empty() && !too_many) {
          const uint32_t ni = stack.back(); stack.pop_back();
          const Node<float>& nd = nodes[ni];
          if (!meets(nd)) continue;
          if ((nd.meta >> 2) != 0u) { if (list.size() >= kShadowListMax) too_many = true; else list.push_back(leaf_of[ni]); }
          else { stack.push_back(nd.offset); stack.push_back(ni + 1u); }
        }
        if (too_many) list.clear();
        else {
          // nearest leaves first: an occluded ray (a fifth of them on config 4) then stops early; the verdict does not depend on the order
          auto dist2 = [&](uint32_t leaf) {
            const LeafRec& lr = out.leaves[leaf];
            double d2 = 0.0;
            for (int k = 0; k < 3; k++) { const double g = std::max(0.0, std::max((double)lr.bmin[k] - c[k], c[k] - (double)lr.bmax[k])); d2 += g * g; }
            return d2;
          };
          std::stable_sort(list.begin(), list.end(), [&](uint32_t a, uint32_t b) { return dist2(a) < dist2(b); });
          out.headers[si * nt + ti] = (uint32_t)list.size();   // (offset filled in below)
        }
      }
    }
  };
  {
    const unsigned hw = std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
    std::vector<std::thread> pool;
    const size_t chunk = (nt + hw - 1) / hw;
    for (unsigned t = 0; t < hw; t++) { const size_t a = std::min(nt, t * chunk), b = std::min(nt, a + chunk); if (a < b) pool.emplace_back(work, a, b); }
    for (auto& th : pool) th.join();
  }
  for (size_t i = 0; i < lists.size(); i++) {
    if (out.headers[i] == 0xffu) continue;
    if (out.entries.size() / 4u + 64u >= (1u << 24)) { out.headers[i] = 0xffu; continue; }
    out.headers[i] = ((uint32_t)(out.entries.size() / 4u) << 8) | (uint32_t)lists[i].size();   // (the offset in units of four entries: the kernel reads four ids at a time)
    out.entries.insert(out.entries.end(), lists[i].begin(), lists[i].end());
    while (out.entries.size() % 4u != 0u) out.entries.push_back(0xffffffffu);
  }
  if (out.entries.empty()) out.entries.assign(4, 0xffffffffu);
  return out;
}

}  // namespace rrtd
