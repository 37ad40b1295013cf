// Wavefront kernels (gfx950, wave64): camera ray generation, BVH traversal (closest / any), shading
// (next-event estimation + BSDF sampling + Russian roulette), film accumulation. One thread = one path
// slot; live paths are carried between kernels as index queues compacted with wave ballots and one atomic per block (block_push).
#pragma once
#include "dmath.hpp"
#include "dtexture.hpp"
#include "nearest.hpp"   // rrt_nearest: the per-triangle function and the walk, shared with the host (tools/nearest_check.cpp)
#include "multihit.hpp"  // rrt_trace_all: the triangle test, the slab test, the sorted insert and the walk, shared with the host (tools/trace_all_check.cpp)
#include "visibility.hpp"  // rrt_visibility: the segment, the first-accept walk and the scan, shared with the host (tools/visibility_check.cpp)

namespace rrtd {

constexpr int kBlock = 256;
// device counters, one 128-byte line each (atomics on different queues must not share an L2 line)
enum { C_ACTIVE = 0, C_NEXT = 32, C_SHADOW = 64, C_CAMERA_RAYS = 96, C_ERROR = 128, C_WORK_CLOSEST = 160, C_WORK_SHADOW = 192, C_WORK_AUX = 224, C_SHADOW2 = 256,
       // per-XCD work cursors of the persistent traversal kernels: 8 lines each (one cursor per eighth of the queue)
       C_WORK8_CLOSEST = 288, C_WORK8_SHADOW = 544,
       // queue entries [0, C_TT_DONE) came from the camera workgroups in whole chunks (k_raygen_main_f32's chunk records), the rest from stage B
       C_TT_DONE = 800,
       // camera rays answered by the camera kernels (SceneDev::root_cull): closest-hit queries that never entered a queue
       C_CULLED = 832,
       // bounce rays the path shading kernel proves to leave the scene (SceneDev::horizon): closest-hit queries that never entered a queue
       C_SKY = 864,
       // film records of the pass (k_raygen_main_f32 with film runs: one run per camera workgroup, allocated from this counter)
       C_RECORDS = 896, C_COUNT = 928 };
// shading kernels push to their queues once per block (measured: 256 <= 512 <= 1024 threads by 5 %: smaller blocks retire
// and refill a CU sooner, and one atomic per 256 paths no longer serialises)
template <typename R> struct ShadeBlock { static constexpr int n = 256; };
#ifndef RRT_SHADE_BLOCK
#define RRT_SHADE_BLOCK 256
#endif
template <> struct ShadeBlock<float> { static constexpr int n = RRT_SHADE_BLOCK; };
enum { ERR_SHADING_NORMAL = 1, ERR_BETA = 4, ERR_NULL_BSDF = 8, ERR_MIPMAP = 16, ERR_HALTON_DIMS = 32, ERR_ST_DIMS = 64, ERR_NO_LIGHTS = 128,
       ERR_KIND_SET = 256 /* a material produced a lobe outside the shading kernel's kind set (dmath.hpp): host-side selection error */,
       ERR_INGEST = 512 /* k_ingest_rays: a pixel or sample_num of rrt_ray_samples outside the film / outside 1 .. nsamp-1 */,
       ERR_SITE = 1024 /* k_sites_check: a site of rrt_sites that rrt_surface_at refuses */,
       ERR_NEAREST = 2048 /* k_nearest / k_nearest_pairs_f32: a walk passed its step or stack bound, or met a word outside its arrays (a tree that is none) */,
       ERR_TRACE_ALL = 4096 /* k_trace_all: a walk passed its step or stack bound, or met a word outside its arrays (a tree that is none) */,
       ERR_VISIBILITY = 8192 /* k_visibility: the same, for a rrt_visibility walk */ };
static_assert(ERR_ST_DIMS == kErrStDims, "error bit shared with dmath.hpp");
static_assert(ERR_HALTON_DIMS == kErrHaltonDims, "error bit shared with dmath.hpp");

// ------------------------------------------------------------------------------------------------------------
// BVH traversal: BVHAccel::intersect / intersect_p (bvh.rs:124-236), same node order, same leaf order, every
// accepted triangle overwrites the hit and t_max (Q10), triangle tests ignore t_max, box test uses it.
// ------------------------------------------------------------------------------------------------------------
template <typename R>
struct RayCtx {
  V3<R> o, d, inv;
  V3<R> lo;   // o = o_hi + lo (fp32 spawned rays; zero otherwise)
  int neg[3];
  R tmax;
};

// ---- pool records (dtypes.hpp Pools): 4-word loads / stores and raw-bit integers ------------------------------------
RRT_DEV float bits_to_real(uint32_t u, float) { return __uint_as_float(u); }
RRT_DEV double bits_to_real(uint32_t u, double) { return __longlong_as_double((long long)u); }
RRT_DEV uint32_t real_to_bits(float v) { return __float_as_uint(v); }
RRT_DEV uint32_t real_to_bits(double v) { return (uint32_t)__double_as_longlong(v); }
template <typename R> RRT_DEV typename Vec4T<R>::type mk4(R x, R y, R z, R w) { typename Vec4T<R>::type v; v.x = x; v.y = y; v.z = z; v.w = w; return v; }
template <typename R> RRT_DEV typename Vec4T<R>::type mk4u(R x, R y, R z, uint32_t w) { return mk4<R>(x, y, z, bits_to_real(w, R(0))); }
// Low word of a double-float origin (spawn_point()), 3 x 10 bits: lo_k is at most half an ulp of hi_k, so it is stored
// as round(lo_k / ulp(hi_k) * 1024) + 512 (resolution ulp / 1024 ~ 4e-9 at coordinates of ~35). Top bits 11 tag the word.
RRT_DEV uint32_t pack_lo(V3<float> hi, V3<float> lo) {
  auto q = [](float h, float l) -> uint32_t {
    const uint32_t e = (__float_as_uint(h) >> 23) & 0xffu;
    if (e < 64u || e > 250u) return 512u;
    const float scaled = l * __uint_as_float((287u - e) << 23);   // l * 2^(33 - (e - 127)) = l / ulp(h) * 1024
    const float r = rintf(scaled) + 512.0f;
    return (uint32_t)fminf(fmaxf(r, 0.0f), 1023.0f);
  };
  return 0xC0000000u | (q(hi.x, lo.x) << 20) | (q(hi.y, lo.y) << 10) | q(hi.z, lo.z);
}
RRT_DEV V3<float> unpack_lo(V3<float> hi, uint32_t w) {
  auto u = [](float h, uint32_t q) -> float {
    const uint32_t e = (__float_as_uint(h) >> 23) & 0xffu;
    if (e < 64u || e > 250u) return 0.0f;
    return ((float)(int)q - 512.0f) * __uint_as_float((e - 33u) << 23);
  };
  return V3<float>(u(hi.x, (w >> 20) & 1023u), u(hi.y, (w >> 10) & 1023u), u(hi.z, w & 1023u));
}
template <typename R> RRT_DEV void store_ray(typename Vec4T<R>::type* ro, typename Vec4T<R>::type* rd, uint32_t i, V3<R> o, V3<R> lo, V3<R> d, R tmax, int skip);
template <> RRT_DEV void store_ray<float>(float4* ro, float4* rd, uint32_t i, V3<float> o, V3<float> lo, V3<float> d, float tmax, int skip) {
  const bool has_lo = lo.x != 0.0f || lo.y != 0.0f || lo.z != 0.0f;
  ro[i] = make_float4(o.x, o.y, o.z, has_lo ? __uint_as_float(pack_lo(o, lo)) : tmax);
  rd[i] = make_float4(d.x, d.y, d.z, __uint_as_float((uint32_t)skip));
}
template <> RRT_DEV void store_ray<double>(double4* ro, double4* rd, uint32_t i, V3<double> o, V3<double>, V3<double> d, double tmax, int skip) {
  ro[i] = mk4<double>(o.x, o.y, o.z, tmax);
  rd[i] = mk4u<double>(d.x, d.y, d.z, (uint32_t)skip);
}
// t_max and origin low word of a stored ray; `queue_tmax` = the t_max every spawned ray of this queue has
RRT_DEV void ray_tail(const float4& ro, float queue_tmax, float* tmax, V3<float>* lo) {
  const uint32_t w = __float_as_uint(ro.w);
  if ((w >> 30) == 3u) { *tmax = queue_tmax; *lo = unpack_lo(V3<float>(ro.x, ro.y, ro.z), w); }
  else { *tmax = ro.w; *lo = V3<float>(); }
}
RRT_DEV void ray_tail(const double4& ro, double, double* tmax, V3<double>* lo) { *tmax = ro.w; *lo = V3<double>(); }

// Bounds3::intersect_p geometry.rs:1767-1800 with gamma(3) of the arithmetic type
template <typename R>
RRT_DEV bool box_hit(const Node<R>& nd, const RayCtx<R>& r) {
  const R g = R(1) + R(2) * ((R(3) * Const<R>::machine_eps) / (R(1) - R(3) * Const<R>::machine_eps));
  R t_min = ((r.neg[0] ? nd.bmax[0] : nd.bmin[0]) - r.o.x) * r.inv.x;
  R t_max = ((r.neg[0] ? nd.bmin[0] : nd.bmax[0]) - r.o.x) * r.inv.x;
  R ty_min = ((r.neg[1] ? nd.bmax[1] : nd.bmin[1]) - r.o.y) * r.inv.y;
  R ty_max = ((r.neg[1] ? nd.bmin[1] : nd.bmax[1]) - r.o.y) * r.inv.y;
  t_max *= g;
  ty_max *= g;
  if (t_min > ty_max || ty_min > t_max) return false;
  if (ty_min > t_min) t_min = ty_min;
  if (ty_max < t_max) t_max = ty_max;
  R tz_min = ((r.neg[2] ? nd.bmax[2] : nd.bmin[2]) - r.o.z) * r.inv.z;
  R tz_max = ((r.neg[2] ? nd.bmin[2] : nd.bmax[2]) - r.o.z) * r.inv.z;
  tz_max *= g;
  if (t_min > tz_max || tz_min > t_max) return false;
  if (tz_min > t_min) t_min = tz_min;
  if (tz_max < t_max) t_max = tz_max;
  return (t_min < r.tmax) && (t_max > R(0));
}

// Triangle::intersect shape/triangle.rs:226-266 (Moller-Trumbore, E2 = p2 - p0)
template <typename R>
RRT_DEV bool tri_closest(const Tri<R>& t, const RayCtx<R>& r, R* th, R* uh, R* vh) {
  V3<R> p0(t.p0), p1(t.p1), p2(t.p2);
  V3<R> E1 = p1 - p0, E2 = p2 - p0;
  V3<R> P = cross(r.d, E2);
  R a = dot(E1, P);
  if (a > R(-0.0000001) && a < R(0.0000001)) return false;
  R f = rcp_r(a);
  V3<R> T = r.o - p0;
  if (sizeof(R) == 4) T = T + r.lo;   // double-float origin: o_hi - p0 is exact for nearby vertices
  R u = f * dot(T, P);
  if (u < R(0) || u > R(1)) return false;
  V3<R> Q = cross(T, E1);
  R v = f * dot(r.d, Q);
  if (v < R(0) || (u + v) > R(1)) return false;
  R tt = f * dot(E2, Q);
  if (tt < R(0.0000001)) return false;
  *th = tt; *uh = u; *vh = v;
  return true;
}
// Triangle::intersect_p shape/triangle.rs:167-205 (E2 = p2 - p1: Q11)
template <typename R>
RRT_DEV bool tri_any(const Tri<R>& t, const RayCtx<R>& r) {
  V3<R> p0(t.p0), p1(t.p1), p2(t.p2);
  V3<R> E1 = p1 - p0, E2 = p2 - p1;
  V3<R> P = cross(r.d, E2);
  R a = dot(E1, P);
  if (a > R(-0.0000001) && a < R(0.0000001)) return false;
  R f = rcp_r(a);
  V3<R> T = r.o - p0;
  if (sizeof(R) == 4) T = T + r.lo;   // double-float origin: o_hi - p0 is exact for nearby vertices
  R u = f * dot(T, P);
  if (u < R(0) || u > R(1)) return false;
  V3<R> Q = cross(T, E1);
  R v = f * dot(r.d, Q);
  if (v < R(0) || (u + v) > R(1)) return false;
  R tt = f * dot(E2, Q);
  if (tt < R(0.0000001)) return false;
  return true;
}

template <typename R>
RRT_DEV RayCtx<R> make_ctx(V3<R> o, V3<R> d, R tmax, V3<R> lo = V3<R>()) {
  RayCtx<R> c;
  c.o = o; c.d = d; c.tmax = tmax; c.lo = lo;
  c.inv = V3<R>(R(1) / d.x, R(1) / d.y, R(1) / d.z);
  c.neg[0] = c.inv.x < R(0); c.neg[1] = c.inv.y < R(0); c.neg[2] = c.inv.z < R(0);
  return c;
}

// Stack policies: a private array for trees no deeper than the reference's 64 entries, a strided global
// array for deeper (compat-built) trees the reference itself could not traverse.
struct PrivStack {
  uint32_t a[64];
  RRT_DEV void put(uint32_t i, uint32_t v) { a[i] = v; }
  RRT_DEV uint32_t get(uint32_t i) const { return a[i]; }
};
struct GlobStack {
  uint32_t* base;
  uint32_t stride;
  RRT_DEV void put(uint32_t i, uint32_t v) { base[(size_t)i * stride] = v; }
  RRT_DEV uint32_t get(uint32_t i) const { return base[(size_t)i * stride]; }
};

// Spawned rays start exactly on their triangle (spawn_ray applies no offset, Q8) and the reference relies on
// f64 to see that triangle again at t ~ 1e-15 < 1e-7. In fp32 the same test returns |t| ~ 1e-6, so the fp32
// path excludes the originating triangle instead — equivalent in exact arithmetic, because a ray meets its own
// triangle's plane only at t = 0. The same holds for every triangle *coplanar* with it (the other half of a
// quad, and — for shadow rays — the sheared triangle Triangle::intersect_p really tests, Q11), so the exclusion
// is by plane id. The f64 parity mode keeps the reference behaviour (skip = -1).
template <typename R> RRT_DEV int self_prim(int prim) { return sizeof(R) == 4 ? prim : -1; }
template <typename R> RRT_DEV uint32_t skip_plane_of(const SceneDev<R>& s, int skip) { return skip >= 0 ? s.tris[skip].plane : 0xffffffffu; }

// Sphere::intersect (sphere.rs:124-259) / Sphere::intersect_p (:51-108) behind GeometricPrimitive /
// TransformedPrimitive (primitives.rs:51-68,115-139), replayed transform by transform.
//   * the quadratic is solved with the object-space ray, the first p_hit uses the ray *handed to the sphere* (Q16);
//   * intersect_p tests the clipping planes against p_hit = 0, phi = 0 first (:75-83);
//   * neither compares t with ray.t_max (Q10).
// There is no epsilon in sphere.rs: a ray spawned on a sphere re-tests it with c = |o|^2 - r^2 ~ 1 ulp of either
// sign and re-hits its own sphere at t ~ 0 whenever the stored hit point landed inside, i.e. for about half of the
// spawned rays. The reference's pixels on spheres are that rounding noise. The f64 mode replays it bit for bit; the
// fp32 mode deliberately keeps the same test (no self exclusion, unlike triangles), so it shows the same noise in
// distribution (mean radiance within a few % of the oracle) though not pixel by pixel. (Tried in round 2 and dropped: solving the
// quadric in double from a double-float hit point inside the fp32 mode. The means did not come closer - a point's coin is not one flip
// but a chain over all later bounces at that point, which a 4e-9 origin does not replay - see DESIGN.md section 4.)
template <typename R>
struct SphereSI { V3<R> p, n, wo, sn, sdpdu; };
// the parts of SurfaceInteraction only textured scenes read: uv, geometric dpdu / dpdv (compute_differentials),
// shading dndu / dndv (specular ray differentials, integrator/mod.rs:188-196)
template <typename R>
struct SurfExt { R u, v; V3<R> dpdu, dpdv, sdpdv, sdndu, sdndv; };

// The rays the sphere code works with: the ray handed to the sphere (instance space, Q16) and the object-space ray.
template <typename R>
RRT_DEV void sphere_rays(const SphereDev<R>& S, V3<R> wo_, V3<R> wd_, V3<R>* ro, V3<R>* rd, V3<R>* oo, V3<R>* od) {
  *ro = wo_; *rd = wd_;
  if (S.has_inst) { *ro = aff_pt(S.imi, wo_); *rd = vnormalize(vnormalize(aff_vec(S.imi, wd_))); }   // xf_ray + Ray::new
  *oo = aff_pt(S.mi, *ro); *od = vnormalize(vnormalize(aff_vec(S.mi, *rd)));
}
// Hit decision. *branch = 1 when the accepted hit is the second root after the clipping test (sphere.rs:170-191):
// the hit record keeps it so that the shading kernel rebuilds the surface without deciding anything again.
template <typename R, bool ANY>
RRT_DEV bool sphere_prim_hit(const SphereDev<R>& S, V3<R> wo_, V3<R> wd_, R* t_out, R* branch) {
  V3<R> ro, rd, oo, od;
  sphere_rays(S, wo_, wd_, &ro, &rd, &oo, &od);
  const R a = od.x * od.x + od.y * od.y + od.z * od.z;
  const R b = R(2) * (od.x * oo.x + od.y * oo.y + od.z * oo.z);
  const R c = oo.x * oo.x + oo.y * oo.y + oo.z * oo.z - S.radius * S.radius;
  R t0, t1;
  if (!quadratic(a, b, c, &t0, &t1)) return false;
  const R kMax = R(1999999999.0);   // MAX_DIST misc.rs
  if (t0 > kMax || t1 <= R(0)) return false;
  R th = t0;
  if (t0 <= R(0)) { th = t1; if (th > kMax) return false; }
  V3<R> ph = ANY ? V3<R>() : ro + rd * th;
  R phi = R(0);
  if (!ANY) {
    if (ph.x == R(0) && ph.y == R(0)) ph.x = R(1e-5) * S.radius;
    phi = atan2(ph.y, ph.x);
    if (phi < R(0)) phi += R(2) * R(RRT_PI);
  }
  *branch = R(0);
  if ((S.z_min > -S.radius && ph.z < S.z_min) || (S.z_max < S.radius && ph.z > S.z_max) || (phi > S.phi_max)) {
    if (th == t1) return false;
    if (t1 > kMax) return false;
    th = t1;
    ph = oo + od * th;
    ph = ph * (S.radius / len(ph));
    if (ph.x == R(0) && ph.y == R(0)) ph.x = R(1e-5) * S.radius;
    phi = atan2(ph.y, ph.x);
    if (phi < R(0)) phi += R(2) * R(RRT_PI);
    if ((S.z_min > -S.radius && ph.z < S.z_min) || (S.z_max < S.radius && ph.z > S.z_max) || (phi > S.phi_max)) return false;
    *branch = R(1);
  }
  *t_out = th;
  return true;
}
// SurfaceInteraction of an accepted sphere hit (sphere.rs:192-259) from (t, branch)
template <typename R>
RRT_DEV void sphere_surface(const SphereDev<R>& S, V3<R> wo_, V3<R> wd_, R th, R branch, SphereSI<R>* si, SurfExt<R>* ext = nullptr) {
  V3<R> ro, rd, oo, od;
  sphere_rays(S, wo_, wd_, &ro, &rd, &oo, &od);
  V3<R> ph;
  if (branch == R(0)) ph = ro + rd * th;
  else { ph = oo + od * th; ph = ph * (S.radius / len(ph)); }
  if (ph.x == R(0) && ph.y == R(0)) ph.x = R(1e-5) * S.radius;
  const R theta = acos(clampr(ph.z / S.radius, R(-1), R(1)));
  const R z_radius = sqrt(ph.x * ph.x + ph.y * ph.y);
  const R inv_zr = R(1) / z_radius;
  const R cphi = ph.x * inv_zr, sphi = ph.y * inv_zr;
  const V3<R> dpdu(-S.phi_max * ph.y, S.phi_max * ph.x, R(0));
  const V3<R> dpdv = V3<R>(ph.z * cphi, ph.z * sphi, -S.radius * R(sin(theta))) * (S.theta_max - S.theta_min);
  // SurfaceInteraction::new (interaction.rs:131-181) then obj_to_world.t(&ist) (transform.rs:628-655)
  V3<R> n = vnormalize(cross(dpdu, dpdv));
  si->p = aff_pt(S.m, ph);
  si->wo = aff_vec(S.m, -od);
  si->n = aff_nrm(S.mi, n);
  si->sn = faceforward(nnormalize(aff_nrm(S.mi, n)), si->n);
  si->sdpdu = aff_vec(S.m, dpdu);
  if (ext) {   // sphere.rs:198-242
    R phi = atan2(ph.y, ph.x);
    if (phi < R(0)) phi += R(2) * R(RRT_PI);
    ext->u = phi / S.phi_max;
    ext->v = (theta - S.theta_min) / (S.theta_max - S.theta_min);
    const V3<R> d2pduu = V3<R>(ph.x, ph.y, R(0)) * -S.phi_max * S.phi_max;
    const V3<R> d2pduv = V3<R>(-sphi, cphi, R(0)) * (S.theta_max - S.theta_min) * ph.z * S.phi_max;
    const V3<R> d2pdvv = ph * -(S.theta_max - S.theta_min) * (S.theta_max - S.theta_min);
    const R E = dot(dpdu, dpdu), F = dot(dpdu, dpdv), G = dot(dpdv, dpdv);
    const R e = dot(n, d2pduu), f = dot(n, d2pduv), g = dot(n, d2pdvv);
    const R inv_EFG2 = R(1) / (E * G - F * F);
    const V3<R> dndu = dpdu * ((f * F - e * G) * inv_EFG2) + dpdv * ((e * F - f * E) * inv_EFG2);
    const V3<R> dndv = dpdu * ((g * F - f * G) * inv_EFG2) + dpdv * ((f * F - g * E) * inv_EFG2);
    ext->dpdu = aff_vec(S.m, dpdu); ext->dpdv = aff_vec(S.m, dpdv);
    ext->sdndu = aff_nrm(S.mi, dndu); ext->sdndv = aff_nrm(S.mi, dndv);
    ext->sdpdv = ext->dpdv;
  }
  if (S.has_inst && !S.inst_identity) {   // TransformedPrimitive::intersect primitives.rs:131-136
    si->p = aff_pt(S.im, si->p);
    si->wo = aff_vec(S.im, si->wo);
    const V3<R> n2 = aff_nrm(S.imi, si->n);
    si->sn = faceforward(nnormalize(aff_nrm(S.imi, si->sn)), n2);
    si->n = n2;
    si->sdpdu = aff_vec(S.im, si->sdpdu);
    if (ext) {
      ext->dpdu = aff_vec(S.im, ext->dpdu); ext->dpdv = aff_vec(S.im, ext->dpdv);
      ext->sdndu = aff_nrm(S.imi, ext->sdndu); ext->sdndv = aff_nrm(S.imi, ext->sdndv);
      ext->sdpdv = ext->dpdv;
    }
  }
}

// triangle of a non-rigid instance (dtypes.hpp kInstBase): the ray as TransformedPrimitive hands it to the triangle
template <typename R> RRT_DEV bool is_inst_tri(const Tri<R>& t) { return (t.material & kInstFlag) != 0u; }
template <typename R> RRT_DEV uint32_t inst_of(const Tri<R>& t) { return (t.material >> 16) & 0x7fffu; }
template <typename R>
RRT_DEV RayCtx<R> inst_ray(const InstDev<R>& I, const RayCtx<R>& r) {   // world_to_prim.t(r): xf_ray + Ray::new (direction normalised twice)
  RayCtx<R> o;
  o.o = aff_pt(I.mi, r.o); o.d = vnormalize(vnormalize(aff_vec(I.mi, r.d))); o.lo = V3<R>(); o.tmax = r.tmax;
  return o;
}

template <typename R, typename Stack>
RRT_DEV int traverse_closest(const SceneDev<R>& s, RayCtx<R>& r, Stack& st, int skip, R* hu, R* hv, uint32_t* nn, uint32_t* np) {
  int hit = -1;
  const uint32_t skip_plane = skip_plane_of(s, skip);
  uint32_t to_visit = 0, cur = 0, cn = 0, cp = 0;
  if (s.n_nodes == 0) return -1;
  while (true) {
    const Node<R> nd = s.nodes[cur];
    cn++;
    if (box_hit(nd, r)) {
      const uint32_t nprims = nd.meta >> 2;
      if (nprims > 0) {
        for (uint32_t i = 0; i < nprims; i++) {
          cp++;
          R t, u, v;
          const Tri<R> tr = s.tris[nd.offset + i];
          if (tr.plane == kSphereMark) {
            if (sphere_prim_hit<R, false>(s.spheres[tr.shade], r.o, r.d, &t, &u)) { r.tmax = t; hit = (int)(nd.offset + i); *hu = u; *hv = R(0); }   // u carries the root branch
            continue;
          }
          if (tr.plane == skip_plane) continue;
          if (is_inst_tri(tr)) {   // object-space test, object-space t copied to the world ray (Q15)
            const RayCtx<R> ro = inst_ray(s.insts[inst_of(tr)], r);
            if (tri_closest(tr, ro, &t, &u, &v)) { r.tmax = t; hit = (int)(nd.offset + i); *hu = u; *hv = v; }
            continue;
          }
          if (tri_closest(tr, r, &t, &u, &v)) { r.tmax = t; hit = (int)(nd.offset + i); *hu = u; *hv = v; }
        }
        if (to_visit == 0) break;
        cur = st.get(--to_visit);
      } else {
        if (r.neg[nd.meta & 3]) { st.put(to_visit++, cur + 1); cur = nd.offset; }
        else { st.put(to_visit++, nd.offset); cur = cur + 1; }
      }
    } else {
      if (to_visit == 0) break;
      cur = st.get(--to_visit);
    }
  }
  *nn = cn; *np = cp;
  return hit;
}
template <typename R, typename Stack>
RRT_DEV bool traverse_any(const SceneDev<R>& s, const RayCtx<R>& r, Stack& st, int skip, uint32_t* nn, uint32_t* np) {
  uint32_t to_visit = 0, cur = 0, cn = 0, cp = 0;
  bool found = false;
  const uint32_t skip_plane = skip_plane_of(s, skip);
  if (s.n_nodes == 0) return false;
  while (true) {
    const Node<R> nd = s.nodes[cur];
    cn++;
    if (box_hit(nd, r)) {
      const uint32_t nprims = nd.meta >> 2;
      if (nprims > 0) {
        for (uint32_t i = 0; i < nprims; i++) {
          cp++;
          const Tri<R> tr = s.tris[nd.offset + i];
          if (tr.plane == kSphereMark) {
            R t, br;
            if (sphere_prim_hit<R, true>(s.spheres[tr.shade], r.o, r.d, &t, &br)) { found = true; break; }
            continue;
          }
          if (tr.plane == skip_plane) continue;
          if (is_inst_tri(tr)) {
            if (tri_any(tr, inst_ray(s.insts[inst_of(tr)], r))) { found = true; break; }
            continue;
          }
          if (tri_any(tr, r)) { found = true; break; }
        }
        if (found) break;
        if (to_visit == 0) break;
        cur = st.get(--to_visit);
      } else {
        if (r.neg[nd.meta & 3]) { st.put(to_visit++, cur + 1); cur = nd.offset; }
        else { st.put(to_visit++, nd.offset); cur = cur + 1; }
      }
    } else {
      if (to_visit == 0) break;
      cur = st.get(--to_visit);
    }
  }
  *nn = cn; *np = cp;
  return found;
}

// Closest-hit kernel over the rays of the active queue (records in queue order: `queue` itself is not read);
// `count` is read on device so the host never synchronises between bounces. Optional per-ray counters feed the roofline's byte model.
template <typename R, bool DEEP, bool COUNT>
__global__ void __launch_bounds__(kBlock) k_closest(SceneDev<R> s, Pools<R> p, const uint32_t* queue, const uint32_t* count, uint32_t n_fixed,
                                                     uint32_t* deep_stack, uint32_t deep_stride, uint32_t* nodes_out, uint32_t* prims_out,
                                                     unsigned long long* totals) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t n = count ? *count : n_fixed;
  if (i >= n) return;
  const typename Vec4T<R>::type ro = p.ray_o[i], rd = p.ray_d[i];
  R r_tmax; V3<R> r_lo;
  ray_tail(ro, Const<R>::inf, &r_tmax, &r_lo);
  RayCtx<R> r = make_ctx(V3<R>(ro.x, ro.y, ro.z), V3<R>(rd.x, rd.y, rd.z), r_tmax, r_lo);
  R hu = 0, hv = 0;
  uint32_t nn = 0, np = 0;
  int hit;
  const int skip = (int)real_to_bits(rd.w);
  if (DEEP) { GlobStack st{deep_stack + i, deep_stride}; hit = traverse_closest(s, r, st, skip, &hu, &hv, &nn, &np); }
  else { PrivStack st; hit = traverse_closest(s, r, st, skip, &hu, &hv, &nn, &np); }
  p.hit[i] = mk4<R>(r.tmax, bits_to_real((uint32_t)hit, R(0)), hu, hv);
  if (COUNT) {
    if (nodes_out) { nodes_out[i] = nn; prims_out[i] = np; }
    if (totals) { atomicAdd(&totals[0], (unsigned long long)nn); atomicAdd(&totals[1], (unsigned long long)np); }
  }
}

// unoccluded shadow ray: L += Ld (a path owns at most one shadow ray per launch, so the update needs no atomic)
// PASSES: the any-hit launch belongs to a frame of rrt_render_passes. A template flag of the four any-hit kernels, as k_shade_path's: the
// instantiations every other frame launches are the code they were.
template <typename R, bool PASSES = false> RRT_DEV void add_pending(const Pools<R>& p, uint32_t i) {
  const typename Vec4T<R>::type ld = p.sld[i];
  const uint32_t slot = real_to_bits(ld.w);
  typename Vec4T<R>::type L = p.L[slot];
  L.x += ld.x; L.y += ld.y; L.z += ld.z;
  p.L[slot] = L;
  // rrt_render_passes: the same term into the plane of every pass it counts for. A plane receives a slot's terms in the order L does - one shadow
  // ray per path and launch - so a pass that takes every term holds L's own bits.
  if (PASSES) {
    for (uint32_t m = p.smask[i]; m != 0u; m &= m - 1u) {
      typename Vec4T<R>::type* const q = p.pass_L + (size_t)(__ffs((int)m) - 1) * p.pass_stride + slot;
      typename Vec4T<R>::type a = *q;
      a.x += ld.x; a.y += ld.y; a.z += ld.z;
      *q = a;
    }
  }
}

// rrt_render_ao: an unoccluded hemisphere ray adds its record {a_i * d_i, slot} to the slot's accumulator {b.xyz, a} (Pools::L points at the
// call's accumulators, not at radiance): d_i is unit and a_i >= 0, so |a_i * d_i| is a_i. A slot owns one ray per launch: no atomic.
template <typename R> RRT_DEV void ao_pending(const Pools<R>& p, uint32_t i) {
  const typename Vec4T<R>::type ld = p.sld[i];
  const uint32_t slot = real_to_bits(ld.w);
  typename Vec4T<R>::type b = p.L[slot];
  b.x += ld.x; b.y += ld.y; b.z += ld.z;
  b.w += sqrt(ld.x * ld.x + ld.y * ld.y + ld.z * ld.z);
  p.L[slot] = b;
}

// Any-hit kernel over the shadow queue: VisibilityTester::unoccluded (lights/mod.rs:60-66); unoccluded paths
// add their pending contribution to L (estimate_direct integrator/mod.rs:459-481).
// AO: the queue holds rrt_render_ao's hemisphere rays (t_max = inf, ao_pending): a template flag, as PASSES is.
template <typename R, bool DEEP, bool COUNT, bool PASSES = false, bool AO = false>
__global__ void __launch_bounds__(kBlock) k_shadow(SceneDev<R> s, Pools<R> p, const uint32_t* queue, const uint32_t* count,
                                                    uint32_t* deep_stack, uint32_t deep_stride, unsigned long long* totals) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= *count) return;
  const typename Vec4T<R>::type ro = p.sray_o[i], rd = p.sray_d[i];
  R r_tmax; V3<R> r_lo;
  ray_tail(ro, AO ? Const<R>::inf : R(1) - R(0.0001), &r_tmax, &r_lo);
  RayCtx<R> r = make_ctx(V3<R>(ro.x, ro.y, ro.z), V3<R>(rd.x, rd.y, rd.z), r_tmax, r_lo);
  uint32_t nn = 0, np = 0;
  bool occ;
  const int skip = (int)real_to_bits(rd.w);
  if (DEEP) { GlobStack st{deep_stack + i, deep_stride}; occ = traverse_any(s, r, st, skip, &nn, &np); }
  else { PrivStack st; occ = traverse_any(s, r, st, skip, &nn, &np); }
  if (!occ) { if (AO) ao_pending<R>(p, i); else add_pending<R, PASSES>(p, i); }
  if (COUNT && totals) { atomicAdd(&totals[0], (unsigned long long)nn); atomicAdd(&totals[1], (unsigned long long)np); }
}

// Public batches (rrt_rays / rrt_hits are SoA arrays): pack into / unpack from the pool's records.
template <typename R>
__global__ void __launch_bounds__(kBlock) k_pack_rays(Pools<R> p, const R* ox, const R* oy, const R* oz, const R* dx, const R* dy, const R* dz, const R* tmax,
                                                       const int32_t* skip, uint32_t n, uint32_t n_tris) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  // caller data: an index outside the triangle array means "none" (the kernels index tris[] with it)
  const int32_t sk = (skip && (uint32_t)skip[i] < n_tris) ? skip[i] : -1;
  store_ray<R>(p.ray_o, p.ray_d, i, V3<R>(ox[i], oy[i], oz[i]), V3<R>(), V3<R>(dx[i], dy[i], dz[i]), tmax[i], sk);
}
template <typename R>
__global__ void __launch_bounds__(kBlock) k_unpack_hits(Pools<R> p, const Tri<R>* tris, R* t, int32_t* prim, R* u, R* v, uint32_t n) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const typename Vec4T<R>::type h = p.hit[i];
  const int32_t pr = (int32_t)real_to_bits(h.y);
  t[i] = h.x; prim[i] = pr;
  if (u) u[i] = (pr >= 0 && tris[pr].plane == kSphereMark) ? R(0) : h.z;   // sphere hits keep their root branch there internally
  if (v) v[i] = h.w;
}

// Public any-hit on caller rays (rrt_trace_any): rays live in the closest-ray arrays of the pool.
template <typename R, bool DEEP>
__global__ void __launch_bounds__(kBlock) k_any_public(SceneDev<R> s, Pools<R> p, uint32_t n, uint8_t* occluded, uint32_t* deep_stack, uint32_t deep_stride) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const typename Vec4T<R>::type ro = p.ray_o[i], rd = p.ray_d[i];
  R r_tmax; V3<R> r_lo;
  ray_tail(ro, Const<R>::inf, &r_tmax, &r_lo);
  RayCtx<R> r = make_ctx(V3<R>(ro.x, ro.y, ro.z), V3<R>(rd.x, rd.y, rd.z), r_tmax, r_lo);
  uint32_t nn, np;
  bool occ;
  const int skip = (int)real_to_bits(rd.w);
  if (DEEP) { GlobStack st{deep_stack + i, deep_stride}; occ = traverse_any(s, r, st, skip, &nn, &np); }
  else { PrivStack st; occ = traverse_any(s, r, st, skip, &nn, &np); }
  occluded[i] = occ ? 1 : 0;
}

// ------------------------------------------------------------------------------------------------------------
// Camera ray generation: ISampler::get_camerasample (samplers/mod.rs:28-34) + generate_ray_differential.
// Slot layout of a pass: slot = sample_local * npix + pixel_local, so the film kernel can sum a pixel's samples
// in sample order without atomics.
// ------------------------------------------------------------------------------------------------------------
struct PassDesc {
  int32_t rx0, ry0, rw;        // rect origin / width the pixel group is enumerated in
  uint32_t pix_begin, npix;    // pixel group [pix_begin, pix_begin + npix) in rect-linear order
  uint32_t s_begin, ns;        // sample_num range [s_begin, s_begin + ns)
  // interleaved row bands (multi-GPU film partition): local row r -> y = ry0 + ((r / band_h) * n_ranks + rank) * band_h + r % band_h
  uint32_t band_h, n_ranks, rank;
  // tiled = 1: the (local row, x) grid is enumerated tile by tile (kTileW x kTileH = 64 pixels; a workgroup of the dense camera kernel takes
  // one tile x 8 consecutive samples), row-major inside a tile and over the tiles, instead of row by row - the host sets it when the width is
  // a multiple of kTileW and the number of local rows a multiple of kTileH. Neighbouring queue entries are then neighbours in BOTH image
  // directions: the rays a wave holds cross a compact patch of the scene instead of a strip of an image row. Measured (frame, config 4):
  // rows 36.8 ms; 32 x 16 tiles, one sample per workgroup 35.7; 8 x 8 tiles x 8 samples 35.0 (16 x 8 x 4, 16 x 16 x 2: in between).
  uint32_t tiled;
};
// The film pixels the samples of a rect can touch under a wide filter (Handle::film_window): the rect grown by the filter's reach
// ceil(r + 0.5) and clipped to the film, ew x eh pixels from (ex0, ey0); ymax = the film's height. One kernel argument of every wide kernel.
struct FilmWindow {
  int ex0, ey0, ew, eh, reach_x, reach_y, ymax;
  size_t n() const { return (size_t)ew * (size_t)eh; }   // host only: the launch's thread count
};
#ifndef RRT_TILE_W
#define RRT_TILE_W 8u
#define RRT_TILE_H 8u
#endif
constexpr uint32_t kTileW = RRT_TILE_W, kTileH = RRT_TILE_H;
RRT_DEV void pass_pixel(const PassDesc& pd, uint32_t lin, uint32_t* px, uint32_t* py) {
  uint32_t row = lin / (uint32_t)pd.rw, col = lin % (uint32_t)pd.rw;
  if (pd.tiled) {
    const uint32_t tile = lin / (kTileW * kTileH), within = lin % (kTileW * kTileH), tiles_per_row = (uint32_t)pd.rw / kTileW;
    col = (tile % tiles_per_row) * kTileW + within % kTileW;
    row = (tile / tiles_per_row) * kTileH + within / kTileW;
  }
  *px = (uint32_t)pd.rx0 + col;
  *py = (uint32_t)pd.ry0 + ((row / pd.band_h) * pd.n_ranks + pd.rank) * pd.band_h + row % pd.band_h;
}

// Listed passes (rrt_render_adaptive): the pixel group is a list of kTileW x kTileH tiles of the rect, numbered row-major from the rect's origin
// (tile t = ty * (rw / kTileW) + tx). Pixel `lin` of the pass (pd.pix_begin + pl, as pass_pixel counts) is pixel `lin % 64` of tile list[lin / 64],
// row-major inside the tile - the enumeration of a tiled pass with the tile number looked up instead of counted. The slot layout stays
// sl * npix + pl. A listed pass has no bands (band_h = 2^30, one rank) and pd.tiled = 1.
RRT_DEV void list_pixel(const PassDesc& pd, const uint32_t* list, uint32_t lin, uint32_t* px, uint32_t* py) {
  const uint32_t tile = list[lin / (kTileW * kTileH)], within = lin % (kTileW * kTileH), tiles_per_row = (uint32_t)pd.rw / kTileW;
  *px = (uint32_t)pd.rx0 + (tile % tiles_per_row) * kTileW + within % kTileW;
  *py = (uint32_t)pd.ry0 + (tile / tiles_per_row) * kTileH + within / kTileW;
}

// Stage 1 (every slot): Halton index + dims 0..3, film point, lens sample, and the *main* lens trace
// (generate_ray, camera.rs:534-580). About 70 % of the samples die here (lens samples are drawn in [0.5,1.5)^2,
// Q5); the survivors are compacted into q_next so that stage 2 runs with full lanes. The main ray waits in the
// next-ray arrays *by slot* until stage 2 knows whether the sample lives.
template <typename R>
__global__ void __launch_bounds__(kBlock) k_raygen(SceneDev<R> s, Pools<R> p, PassDesc pd, double* dbg_dims) {
  const uint32_t slot = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t total = pd.npix * pd.ns;
  bool alive = false;
  if (slot < total) {
    const uint32_t pl = slot % pd.npix, sl = slot / pd.npix;
    uint32_t px, py;
    pass_pixel(pd, pd.pix_begin + pl, &px, &py);
    const uint32_t sample_num = pd.s_begin + sl;
    uint32_t index;
    double d0, d1, d2, d3, d4 = 0.0;
    if (s.sampler_type == 1u) {   // StratifiedSampler: get_camerasample = 2D film, 2D lens, 1D time (samplers/mod.rs:28-34)
      index = ((py * (uint32_t)s.xres + px) << 10) | sample_num;
      uint32_t cd = 0;
      st_get_2d(s, index, &cd, &d0, &d1);
      st_get_2d(s, index, &cd, &d2, &d3);
      d4 = st_get_1d(s, index, &cd);
    } else {
      index = halton_pixel_offset(s, px, py) + sample_num * s.stride;
      d0 = halton_dim(s, index, 0); d1 = halton_dim(s, index, 1); d2 = halton_cam_dim(s, index, 0); d3 = halton_cam_dim(s, index, 1);
    }
    // dimension 4 (time) is drawn and unused by a static scene
    const R pfx = (R)px + to_real<R>(d0), pfy = (R)py + to_real<R>(d1);
    const R lx = to_real<R>(d2) + R(0.5), ly = to_real<R>(d3) + R(0.5);  // Q5
    RayT<R> ray;
    const R w = generate_ray(s, pfx, pfy, lx, ly, &ray);
    alive = w != R(0);
    p.hindex[slot] = index;
    p.weight[slot] = alive ? w : R(0);
    p.samp[slot] = mk4<R>(pfx, pfy, lx, ly);
    if (alive) {
      store_ray<R>(p.nray_o, p.nray_d, slot, ray.o, V3<R>(), ray.d, Const<R>::inf, -1);
    }
    if (dbg_dims) {
      double* dd = dbg_dims + 5 * (size_t)(pl * pd.ns + sl);   // [pixel][sample]
      dd[0] = d0; dd[1] = d1; dd[2] = d2; dd[3] = d3; dd[4] = s.sampler_type == 1u ? d4 : halton_dim(s, index, 4);
    }
  }
  __shared__ uint32_t push_lds[kBlock / 64 + 1];
  const uint32_t q = block_push(&p.counters[C_NEXT], alive, push_lds);
  if (alive) p.q_next[q] = QEnt{slot, 0u, 0u, 0u};
}

// unit-test surface of rrt_sampler_values: one thread per (stream, k). The index word is formed as k_raygen forms it, and the values are what
// draw_1d / draw_2d return with the stream's counter at first + k - the very device functions the frame calls (dmath.hpp), no copies. The host has
// checked the pixels, the sample numbers and the counter range (no draw reaches ERR_HALTON_DIMS / ERR_ST_DIMS) and n * count < 2^31.
template <typename R>
__global__ void __launch_bounds__(kBlock) k_sampler_values(SceneDev<R> s, const uint32_t* pixel, const uint32_t* sample_num, uint32_t n, uint32_t first, uint32_t count,
                                                           unsigned long long* index_out, double* v1, double* v2) {
  const uint32_t t = blockIdx.x * kBlock + threadIdx.x;
  if (t >= n * count) return;
  const uint32_t i = t / count, k = t - i * count;
  const uint32_t pw = pixel[i], px = pw & 0xffffu, py = pw >> 16, sn = sample_num[i];
  const bool st = s.sampler_type == 1u;
  const uint32_t index = st ? (((py * (uint32_t)s.xres + px) << 10) | sn) : halton_pixel_offset(s, px, py) + sn * s.stride;
  if (k == 0 && index_out) index_out[i] = index;
  uint32_t d = first + k;                                 // the 1D counter (StratifiedSampler: the low kStBits; HaltonSampler: the dimension)
  v1[t] = draw_1d(s, index, &d);
  d = st ? (first + k) << kStBits : first + k;            // the 2D counter
  double a, b;
  draw_2d(s, index, &d, &a, &b);
  v2[2 * (size_t)t] = a; v2[2 * (size_t)t + 1] = b;
}

// k_raygen over a listed pass (list_pixel): the same statements per slot, HaltonSampler only (rrt_render_adaptive refuses the StratifiedSampler)
// and without the debug dimensions. A kernel of its own, so that the kernel every other pass launches stays the code it is.
template <typename R>
__global__ void __launch_bounds__(kBlock) k_raygen_list(SceneDev<R> s, Pools<R> p, PassDesc pd, const uint32_t* list) {
  const uint32_t slot = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t total = pd.npix * pd.ns;
  bool alive = false;
  if (slot < total) {
    const uint32_t pl = slot % pd.npix, sl = slot / pd.npix;
    uint32_t px, py;
    list_pixel(pd, list, pd.pix_begin + pl, &px, &py);
    const uint32_t sample_num = pd.s_begin + sl;
    const uint32_t index = halton_pixel_offset(s, px, py) + sample_num * s.stride;
    const double d0 = halton_dim(s, index, 0), d1 = halton_dim(s, index, 1), d2 = halton_cam_dim(s, index, 0), d3 = halton_cam_dim(s, index, 1);
    const R pfx = (R)px + to_real<R>(d0), pfy = (R)py + to_real<R>(d1);
    const R lx = to_real<R>(d2) + R(0.5), ly = to_real<R>(d3) + R(0.5);  // Q5
    RayT<R> ray;
    const R w = generate_ray(s, pfx, pfy, lx, ly, &ray);
    alive = w != R(0);
    p.hindex[slot] = index;
    p.weight[slot] = alive ? w : R(0);
    p.samp[slot] = mk4<R>(pfx, pfy, lx, ly);
    if (alive) {
      store_ray<R>(p.nray_o, p.nray_d, slot, ray.o, V3<R>(), ray.d, Const<R>::inf, -1);
    }
  }
  __shared__ uint32_t push_lds[kBlock / 64 + 1];
  const uint32_t q = block_push(&p.counters[C_NEXT], alive, push_lds);
  if (alive) p.q_next[q] = QEnt{slot, 0u, 0u, 0u};
}

// Stage 2 (survivors): the auxiliary rays of generate_ray_differential (camera.rs:582-628) at p_film +- 0.05 px in
// x then y. A sample whose x or y pair both fail gets weight 0; on scenes with textured materials the auxiliary rays
// themselves are kept as the camera ray's differentials (p.rdx_* / p.rdy_*). Living samples
// enter q_active with their ray at the same position. `enqueue` = 0 for AOIntegrator, whose li returns 0 before
// drawing anything (ao.rs:62-64).
template <typename R>
__global__ void __launch_bounds__(kBlock) k_raygen_aux(SceneDev<R> s, Pools<R> p, int enqueue) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t n = p.counters[C_NEXT];
  bool alive = false;
  uint32_t slot = 0;
  if (i < n) {
    slot = p.q_next[i].slot;
    const typename Vec4T<R>::type cs = p.samp[slot];
    const R pfx = cs.x, pfy = cs.y, lx = cs.z, ly = cs.w;
    RayT<R> aux, auy;
    R epsx = R(0.05), epsy = R(0.05);
    R wtx = generate_ray(s, pfx + R(0.05), pfy, lx, ly, &aux);
    if (wtx == R(0)) { epsx = R(-0.05); wtx = generate_ray(s, pfx + R(-0.05), pfy, lx, ly, &aux); }
    R wty = R(0);
    if (wtx != R(0)) {
      wty = generate_ray(s, pfx, pfy + R(0.05), lx, ly, &auy);
      if (wty == R(0)) { epsy = R(-0.05); wty = generate_ray(s, pfx, pfy + R(-0.05), lx, ly, &auy); }
    }
    alive = wtx != R(0) && wty != R(0) && p.weight[slot] > R(0);   // `if ray_weight > 0.0` integrator/mod.rs:100
    if (!(wtx != R(0) && wty != R(0))) p.weight[slot] = R(0);
    if (alive && p.rdx_o) {
      // rx / ry of generate_ray_differential (camera.rs:597-598, 613-614), then scale_differentials (geometry.rs:1883-1888)
      const typename Vec4T<R>::type mo = p.nray_o[slot], md = p.nray_d[slot];
      const V3<R> o(mo.x, mo.y, mo.z), d(md.x, md.y, md.z);
      V3<R> rxo = o + (aux.o - o) / epsx, rxd = d + (aux.d - d) / epsx;
      V3<R> ryo = o + (auy.o - o) / epsy, ryd = d + (auy.d - d) / epsy;
      rxo = o + (rxo - o) * s.diff_scale; ryo = o + (ryo - o) * s.diff_scale;
      rxd = d + (rxd - d) * s.diff_scale; ryd = d + (ryd - d) * s.diff_scale;
      p.rdx_o[slot] = mk4<R>(rxo.x, rxo.y, rxo.z, R(0)); p.rdx_d[slot] = mk4<R>(rxd.x, rxd.y, rxd.z, R(0));
      p.rdy_o[slot] = mk4<R>(ryo.x, ryo.y, ryo.z, R(0)); p.rdy_d[slot] = mk4<R>(ryd.x, ryd.y, ryd.z, R(0));
    }
  }
  __shared__ uint32_t push_lds[kBlock / 64 + 1];
  const bool enq = alive && enqueue;
  const uint32_t q = block_push(&p.counters[C_ACTIVE], enq, push_lds);
  if (enq) {
    p.q_active[q] = QEnt{slot, s.cam_db, p.hindex[slot], 0u};   // camera dimensions consumed, bounce 0
    p.path[q] = mk4<R>(R(1), R(1), R(1), R(1));
    p.ray_o[q] = p.nray_o[slot]; p.ray_d[q] = p.nray_d[slot];
  }
  if (alive) p.L[slot] = mk4<R>(R(0), R(0), R(0), R(0));
  (void)block_push(&p.counters[C_CAMERA_RAYS], alive, push_lds);
}

// debug / unit-test surface of rrt_camera_samples: rays + weights of a pass, [pixel][sample] order (dbg_ray zeroed
// by the host: dead samples report a zero ray)
template <typename R>
__global__ void __launch_bounds__(kBlock) k_camera_dump(Pools<R> p, PassDesc pd, double* dbg_ray, double* dbg_w) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t < pd.npix * pd.ns) {
    const uint32_t pl = t % pd.npix, sl = t / pd.npix;
    dbg_w[pl * pd.ns + sl] = (double)p.weight[t];
  }
  if (t < p.counters[C_ACTIVE]) {
    const uint32_t slot = p.q_active[t].slot;
    const uint32_t pl = slot % pd.npix, sl = slot / pd.npix;
    const typename Vec4T<R>::type ro = p.ray_o[t], rd = p.ray_d[t];
    double* rr = dbg_ray + 6 * (size_t)(pl * pd.ns + sl);
    rr[0] = (double)ro.x; rr[1] = (double)ro.y; rr[2] = (double)ro.z;
    rr[3] = (double)rd.x; rr[4] = (double)rd.y; rr[5] = (double)rd.z;
  }
}

// ------------------------------------------------------------------------------------------------------------
// Caller-supplied rays (rrt_radiance, rrt_render_rays): the second producer of the pool state the integrators consume - k_ingest_rays leaves what
// k_raygen + k_raygen_aux leave for a pass - and, for rrt_radiance, the second consumer of L beside the film kernels.
// ------------------------------------------------------------------------------------------------------------
// rrt_ray_samples on the device (staged there for a host-memory call). p_film set = rrt_render_rays: sample (x, y, sample_num) of the pass lies at
// ((y - ry0) * rw + (x - rx0)) * ns_all + (sample_num - s0) of every array, the [pixel][sample] layout of rrt_camera_samples over the call's rect
// (PassDesc::rx0 / ry0 / rw). p_film null = rrt_radiance: slot i of the pass is ray base + i, its sampler stream named by pixel / sample_num.
template <typename R>
struct RaySamples {
  const R *o[3], *d[3];
  const R* weight;                                // null = 1 everywhere
  const R *rxo[3], *rxd[3], *ryo[3], *ryd[3];     // all null (rx = ry = the ray) or all set
  const R* p_film;
  const uint32_t *pixel, *sample_num;
  uint64_t base;
  uint32_t s0, ns_all;
  // Workgroup shape: 2^pb_log2 pixels x (kBlock >> pb_log2) samples of the pass, pixels on the fast lanes. The caller's arrays run sample-fastest
  // and the slots pixel-fastest, so a wave of one sample x 64 pixels would fetch one element from each of 64 runs ns_all elements apart - every
  // 128-byte line fetched ns_all times over the launch, by workgroups too far apart to meet in a cache. With min(ns, 32) samples in the workgroup
  // (the host picks the shape) its four waves read the same few contiguous runs within the lifetime of one workgroup, and the 8+ neighbouring
  // pixels of a sample still make whole 128-byte lines of the 16-byte per-slot records (samp, L, differentials). rrt_radiance: 256 x 1, a plain
  // coalesced copy.
  uint32_t pb_log2;
};
// One thread per slot of a tile, kIngestTiles tiles per workgroup. check_only: nothing but the range check of pixel / sample_num is done (rrt_radiance on device-resident arrays
// runs it over the whole batch first, so that a refused call has written nothing); the check itself is made in every launch, and a sample that
// fails it is dead - no table of the sampler is ever indexed by an unchecked value. write_samp: as the camera kernels' (launch_raygen).
constexpr uint32_t kIngestTiles = 4;   // pixel tiles per workgroup of k_ingest_rays: one queue reservation for all of them
template <typename R>
__global__ void __launch_bounds__(kBlock) k_ingest_rays(SceneDev<R> s, Pools<R> p, PassDesc pd, RaySamples<R> in, int enqueue, int write_samp, int check_only) {
  const uint32_t pb = 1u << in.pb_log2, sb = (uint32_t)kBlock >> in.pb_log2;
  const uint32_t sl = blockIdx.y * sb + (threadIdx.x >> in.pb_log2);
  __shared__ uint32_t push_lds[kBlock / 64 + 2];
  // The workgroup takes kIngestTiles tiles of pb pixels x sb samples and reserves queue space for their live samples with ONE atomic: every
  // workgroup of the launch adds to the same counter, and those additions are served one after the other (measured at 1024^2 x 32 samples: 131 072
  // reservations made the launch 1.5 ms long whatever it loaded or stored)
  bool alive[kIngestTiles];
  uint32_t slot[kIngestTiles], index[kIngestTiles], rank[kIngestTiles], total = 0;
  V3<R> o[kIngestTiles], d[kIngestTiles];
#pragma unroll
  for (uint32_t k = 0; k < kIngestTiles; k++) {
    const uint32_t pl = (blockIdx.x * kIngestTiles + k) * pb + (threadIdx.x & (pb - 1u));
    alive[k] = false; slot[k] = 0; index[k] = 0;
    if (pl < pd.npix && sl < pd.ns) {
      slot[k] = sl * pd.npix + pl;
      size_t i;
      uint32_t px, py, sample_num;
      R pfx, pfy;
      bool ok = true;
      if (in.p_film) {
        pass_pixel(pd, pd.pix_begin + pl, &px, &py);
        sample_num = pd.s_begin + sl;
        i = ((size_t)(py - (uint32_t)pd.ry0) * (uint32_t)pd.rw + (px - (uint32_t)pd.rx0)) * in.ns_all + (sample_num - in.s0);
        pfx = pfy = R(0);
        if (write_samp) { pfx = in.p_film[2 * i]; pfy = in.p_film[2 * i + 1]; }
      } else {
        i = (size_t)in.base + slot[k];
        const uint32_t pw = in.pixel[i];
        px = pw & 0xffffu; py = pw >> 16; sample_num = in.sample_num[i];
        ok = px < (uint32_t)s.xres && py < (uint32_t)s.yres && sample_num >= 1u && sample_num < s.nsamp;
        if (!ok) atomicOr(s.err, (uint32_t)ERR_INGEST);
        pfx = (R)px + R(0.5); pfy = (R)py + R(0.5);   // no film in rrt_radiance: never written (write_samp = 0)
      }
      if (!check_only) {
        const R w = in.weight ? in.weight[i] : R(1);
        alive[k] = ok && w > R(0);
        p.weight[slot[k]] = alive[k] ? w : R(0);
        if (write_samp) p.samp[slot[k]] = mk4<R>(pfx, pfy, R(0), R(0));   // only the wide film kernels read p_film
        if (alive[k]) {   // (a dead sample's index and radiance record are never read: the queue, film_sample_radiance, k_radiance_out)
          if (s.sampler_type == 1u) index[k] = ((py * (uint32_t)s.xres + px) << 10) | sample_num;   // as k_raygen forms them
          else index[k] = halton_pixel_offset(s, px, py) + sample_num * s.stride;
          p.hindex[slot[k]] = index[k];
          p.L[slot[k]] = mk4<R>(R(0), R(0), R(0), R(0));
          o[k] = V3<R>(in.o[0][i], in.o[1][i], in.o[2][i]); d[k] = V3<R>(in.d[0][i], in.d[1][i], in.d[2][i]);
          if (p.rdx_o) {
            V3<R> rxo = o[k], rxd = d[k], ryo = o[k], ryd = d[k];
            if (in.rxo[0]) {
              rxo = V3<R>(in.rxo[0][i], in.rxo[1][i], in.rxo[2][i]); rxd = V3<R>(in.rxd[0][i], in.rxd[1][i], in.rxd[2][i]);
              ryo = V3<R>(in.ryo[0][i], in.ryo[1][i], in.ryo[2][i]); ryd = V3<R>(in.ryd[0][i], in.ryd[1][i], in.ryd[2][i]);
            }
            p.rdx_o[slot[k]] = mk4<R>(rxo.x, rxo.y, rxo.z, R(0)); p.rdx_d[slot[k]] = mk4<R>(rxd.x, rxd.y, rxd.z, R(0));
            p.rdy_o[slot[k]] = mk4<R>(ryo.x, ryo.y, ryo.z, R(0)); p.rdy_d[slot[k]] = mk4<R>(ryd.x, ryd.y, ryd.z, R(0));
          }
        }
      }
    }
    if (!check_only) {   // (block-uniform) rank among the workgroup's live samples: tiles in turn, block order inside a tile
      uint32_t n_tile;
      rank[k] = total + block_rank(alive[k], push_lds, &n_tile);
      total += n_tile;
    }
  }
  if (check_only) return;
  // camera rays = the weights > 0: where they are enqueued that is the queue's own count, copied by k_ingest_count behind this launch
  uint32_t* const counter = &p.counters[enqueue ? C_ACTIVE : C_CAMERA_RAYS];
  if (threadIdx.x == 0) push_lds[kBlock / 64 + 1] = total ? atomicAdd(counter, total) : 0u;
  __syncthreads();
  const uint32_t first = push_lds[kBlock / 64 + 1];
  if (!enqueue) return;
#pragma unroll
  for (uint32_t k = 0; k < kIngestTiles; k++) {
    if (!alive[k]) continue;
    const uint32_t q = first + rank[k];
    p.q_active[q] = QEnt{slot[k], s.cam_db, index[k], 0u};   // camera dimensions consumed, bounce 0
    p.path[q] = mk4<R>(R(1), R(1), R(1), R(1));
    store_ray<R>(p.ray_o, p.ray_d, q, o[k], V3<R>(), d[k], Const<R>::inf, -1);
  }
}
static __global__ void k_ingest_count(uint32_t* c) { c[C_CAMERA_RAYS] = c[C_ACTIVE]; }

// rrt_radiance: Li of the first n slots as {r, g, b, 0}, one 128-bit (f64: 256-bit) load and store per thread; a dead slot's record is not the
// integrator's to write, so it is answered here
template <typename R>
__global__ void __launch_bounds__(kBlock) k_radiance_out(Pools<R> p, typename Vec4T<R>::type* rgb4, uint32_t n) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  typename Vec4T<R>::type l = mk4<R>(R(0), R(0), R(0), R(0));
  if (p.weight[i] > R(0)) l = p.L[i];
  l.w = R(0);
  rgb4[i] = l;
}

// ------------------------------------------------------------------------------------------------------------
// Irradiance and SH probes at caller-supplied points (rrt_irradiance, rrt_irradiance_rays): the third producer of the pool state the integrators
// consume - k_irr_gen makes the rays of a pass in registers from the points and the draws' own sampler streams - and the third consumer of L,
// k_irr_reduce, which adds a point's draws up on the device.
// ------------------------------------------------------------------------------------------------------------
// rrt_points on the device (staged there for a host-memory call). Pixel pl of a pass is point base + pl, sample sl is draw pd.s_begin + sl.
template <typename R>
struct IrrPoints {
  const R *p[3], *n[3];       // n all null (sphere mode): the z axis
  const uint32_t* pixel;      // null: x = i % xres, y = (i / xres) % yres
  uint64_t base;
  R offset;
  uint32_t mode;              // RRT_IRR_COSINE / RRT_IRR_SPHERE
  uint32_t s0, ns_all;        // the call's first draw and its number of draws: the [point][draw] layout of rrt_irradiance_rays
};
// local direction of a draw from the first two values of its sampler stream (the camera sample's film dimensions, which no point has a use for)
template <typename R>
RRT_DEV V3<R> irr_local_dir(const SceneDev<R>& s, uint32_t mode, uint32_t index) {
  const R u0 = to_real<R>(halton_dim(s, index, 0)), u1 = to_real<R>(halton_dim(s, index, 1));
  return mode == 1u ? uniform_sample_sphere(u0, u1) : cosine_sample_hemisphere(u0, u1);
}
// One thread per point, points on the fast lanes: the point's six values (coalesced loads), its unit normal, frame and Halton offset are worked
// out once and serve kIngestTiles consecutive draws, tile k of the workgroup = draw blockIdx.y * kIngestTiles + k of its 256 points. Slot layout
// and queue reservation are k_ingest_rays' (slot = draw * npix + point; one atomic per workgroup for all its tiles, see there for what per-tile
// atomics cost). od6 set (rrt_irradiance_rays): the rays are written out as [point][draw][6], a dead draw as zeros, and no pool is touched.
// check_only: nothing but the range check of `pixel`, which is made in every launch - a point that fails it is dead.
template <typename R>
__global__ void __launch_bounds__(kBlock) k_irr_gen(SceneDev<R> s, Pools<R> p, PassDesc pd, IrrPoints<R> in, int enqueue, int check_only, R* od6) {
  const uint32_t pl = blockIdx.x * kBlock + threadIdx.x;
  __shared__ uint32_t push_lds[kBlock / 64 + 2];
  bool live = false;
  uint32_t index0 = 0;
  V3<R> org, nn(R(0), R(0), R(1)), sv, tv;
  if (pl < pd.npix) {
    const size_t i = (size_t)in.base + pl;
    uint32_t px, py;
    bool ok = true;
    if (in.pixel) {
      const uint32_t pw = in.pixel[i];
      px = pw & 0xffffu; py = pw >> 16;
      ok = px < (uint32_t)s.xres && py < (uint32_t)s.yres;
      if (!ok) atomicOr(s.err, (uint32_t)ERR_INGEST);
    } else {
      px = (uint32_t)(i % (size_t)s.xres); py = (uint32_t)((i / (size_t)s.xres) % (size_t)s.yres);
    }
    if (!check_only && ok) {
      live = true;
      if (in.n[0]) {   // any non-zero finite length: a length whose square leaves the type's range is brought into it first
        V3<R> nv(in.n[0][i], in.n[1][i], in.n[2][i]);
        live = isfinite(nv.x) && isfinite(nv.y) && isfinite(nv.z);
        R l2 = len2(nv);
        if (live && !(l2 >= R(1e-30) && isfinite(l2))) {
          const R m = rmax(rmax(rabs(nv.x), rabs(nv.y)), rabs(nv.z));
          live = m > R(0);
          nv = nv / m;
        }
        nn = nv / len(nv);
      }
      if (live) {
        coordinate_system(nn, &sv, &tv);
        org = V3<R>(in.p[0][i], in.p[1][i], in.p[2][i]) + nn * in.offset;
        index0 = halton_pixel_offset(s, px, py);
      }
    }
  }
  if (check_only) return;
  bool alive[kIngestTiles];
  uint32_t slot[kIngestTiles], index[kIngestTiles], rank[kIngestTiles], total = 0;
  V3<R> d[kIngestTiles];
#pragma unroll
  for (uint32_t k = 0; k < kIngestTiles; k++) {
    const uint32_t sl = blockIdx.y * kIngestTiles + k;
    alive[k] = false; slot[k] = 0; index[k] = 0;
    if (pl < pd.npix && sl < pd.ns) {
      slot[k] = sl * pd.npix + pl;
      if (live) {
        index[k] = index0 + (pd.s_begin + sl) * s.stride;   // as k_raygen forms it (HaltonSampler: the host refuses the StratifiedSampler)
        const V3<R> wl = irr_local_dir(s, in.mode, index[k]);
        alive[k] = in.mode == 1u || wl.z != R(0);
        d[k] = vnormalize(V3<R>((sv.x * wl.x + tv.x * wl.y) + nn.x * wl.z, (sv.y * wl.x + tv.y * wl.y) + nn.y * wl.z, (sv.z * wl.x + tv.z * wl.y) + nn.z * wl.z));
      }
      if (od6) {
        R* const r6 = od6 + 6 * (((size_t)in.base + pl) * in.ns_all + ((pd.s_begin + sl) - in.s0));
        r6[0] = alive[k] ? org.x : R(0); r6[1] = alive[k] ? org.y : R(0); r6[2] = alive[k] ? org.z : R(0);
        r6[3] = alive[k] ? d[k].x : R(0); r6[4] = alive[k] ? d[k].y : R(0); r6[5] = alive[k] ? d[k].z : R(0);
      } else {
        p.weight[slot[k]] = alive[k] ? R(1) : R(0);
        if (alive[k]) {   // (a dead draw's index and radiance record are never read: the queue, k_irr_reduce)
          p.hindex[slot[k]] = index[k];
          p.L[slot[k]] = mk4<R>(R(0), R(0), R(0), R(0));
          if (p.rdx_o) {   // no differentials: rx = ry = the ray
            p.rdx_o[slot[k]] = mk4<R>(org.x, org.y, org.z, R(0)); p.rdx_d[slot[k]] = mk4<R>(d[k].x, d[k].y, d[k].z, R(0));
            p.rdy_o[slot[k]] = mk4<R>(org.x, org.y, org.z, R(0)); p.rdy_d[slot[k]] = mk4<R>(d[k].x, d[k].y, d[k].z, R(0));
          }
        }
      }
    }
    if (!od6) {   // (block-uniform) rank among the workgroup's live draws: tiles in turn, block order inside a tile
      uint32_t n_tile;
      rank[k] = total + block_rank(alive[k], push_lds, &n_tile);
      total += n_tile;
    }
  }
  if (od6) return;
  uint32_t* const counter = &p.counters[enqueue ? C_ACTIVE : C_CAMERA_RAYS];
  if (threadIdx.x == 0) push_lds[kBlock / 64 + 1] = total ? atomicAdd(counter, total) : 0u;
  __syncthreads();
  const uint32_t first = push_lds[kBlock / 64 + 1];
  if (!enqueue) return;
#pragma unroll
  for (uint32_t k = 0; k < kIngestTiles; k++) {
    if (!alive[k]) continue;
    const uint32_t q = first + rank[k];
    p.q_active[q] = QEnt{slot[k], s.cam_db, index[k], 0u};   // the camera's dimensions count as consumed, bounce 0
    p.path[q] = mk4<R>(R(1), R(1), R(1), R(1));
    store_ray<R>(p.ray_o, p.ray_d, q, org, V3<R>(), d[k], Const<R>::inf, -1);
  }
}

// The nine real spherical harmonics of bands 0 .. 2 at a unit vector, in the order and with the constants rrt.h writes out
template <typename R>
RRT_DEV void sh9(V3<R> w, R y[9]) {
  y[0] = R(0.28209479177387814);
  y[1] = R(0.4886025119029199) * w.y;
  y[2] = R(0.4886025119029199) * w.z;
  y[3] = R(0.4886025119029199) * w.x;
  y[4] = R(1.0925484305920792) * (w.x * w.y);
  y[5] = R(1.0925484305920792) * (w.y * w.z);
  y[6] = R(0.31539156525252005) * (R(3) * (w.z * w.z) - R(1));
  y[7] = R(1.0925484305920792) * (w.x * w.z);
  y[8] = R(0.5462742152960396) * (w.x * w.x - w.y * w.y);
}
// One thread per point of the pass: the caller's row, then the pass's draws of the point in draw order - L[draw * npix + point], one 128-bit
// (f64: 256-bit) load per lane, contiguous across the wave - and the row written back: {sum r, sum g, sum b, sum y^2} with plain adds in the
// handle's type, so a row holds the same bits however the draws were cut into passes and calls. sh27 set (sphere mode): the draw's local
// direction again from its own stream, and 27 more sums held in registers. A dead draw (weight 0) adds nothing.
// ISA (gfx950): no scratch in either precision - the 27 sums and the 9 basis values stay in registers (the loops over them are unrolled): 67 VGPRs
// in fp32, 120 in f64, private segment 0 (k_irr_gen: 60 / 96 VGPRs, no scratch either).
template <typename R>
__global__ void __launch_bounds__(kBlock) k_irr_reduce(SceneDev<R> s, Pools<R> p, PassDesc pd, uint64_t base, R* sums4, R* sh27) {
  const uint32_t pl = blockIdx.x * kBlock + threadIdx.x;
  if (pl >= pd.npix) return;
  R* const row = sums4 + 4 * ((size_t)base + pl);
  R a0 = row[0], a1 = row[1], a2 = row[2], a3 = row[3];
  R sh[27];
  R* const shrow = sh27 ? sh27 + 27 * ((size_t)base + pl) : nullptr;
  if (shrow) {
#pragma unroll
    for (int k = 0; k < 27; k++) sh[k] = shrow[k];
  }
  for (uint32_t sl = 0; sl < pd.ns; sl++) {
    const uint32_t slot = sl * pd.npix + pl;
    if (!(p.weight[slot] > R(0))) continue;
    const typename Vec4T<R>::type l = p.L[slot];
    const R y = Rgb<R>(l.x, l.y, l.z).y();
    a0 += l.x; a1 += l.y; a2 += l.z; a3 += y * y;
    if (shrow) {
      R yk[9];
      sh9(irr_local_dir(s, 1u, p.hindex[slot]), yk);
#pragma unroll
      for (int k = 0; k < 9; k++) { sh[3 * k] += l.x * yk[k]; sh[3 * k + 1] += l.y * yk[k]; sh[3 * k + 2] += l.z * yk[k]; }
    }
  }
  row[0] = a0; row[1] = a1; row[2] = a2; row[3] = a3;
  if (shrow) {
#pragma unroll
    for (int k = 0; k < 27; k++) shrow[k] = sh[k];
  }
}

// ------------------------------------------------------------------------------------------------------------
// Shading
// ------------------------------------------------------------------------------------------------------------
template <typename R>
struct Surf {   // the parts of SurfaceInteraction (interaction.rs:95-181) the in-scope materials read
  V3<R> p, p_lo, n, wo, sn, sdpdu;   // p_lo: see spawn_point()
  uint32_t material;
  bool ok;
};

// Hit point. The reference uses o + d * t in f64 and then relies on its `t < 1e-7` rejection to swallow the ~1e-15
// by which that point misses the surface. In fp32 the same expression misses by ~3e-6 at scene coordinates of ~50,
// more than the threshold: a spawned ray that starts just below the plane of the *adjacent* triangle (origin within
// ~1e-4 of a shared edge) then "hits" it at t ~ 1e-5 - about 1e-4 of all shadow rays on the 100k-triangle config,
// 3-4 % of its pixels off by a whole sample. So the fp32 mode builds the point from the barycentrics on the stored
// (fp32) triangle as an unevaluated sum p_hi + p_lo (TwoSum), and the triangle tests form (o_hi - p0) + o_lo:
// o_hi - p0 is exact for nearby vertices, so the origin lies on its triangle to ~1e-9 and on the right side of every
// neighbour. f64 mode: the reference expression, p_lo = 0.
// SITE (rrt_surface_at): there is no ray; the point is the barycentric one in both precisions, p0 + ((p1 - p0) u + (p2 - p0) v), and in f64 p_lo = 0.
template <typename R, bool SITE = false>
RRT_DEV void spawn_point(V3<R> o, V3<R> d, R t, R u, R v, V3<R> p0, V3<R> p1, V3<R> p2, V3<R>* p, V3<R>* p_lo) {
  if (!SITE) {
#ifdef RRT_SPAWN_OLD
    { *p = o + d * t; *p_lo = V3<R>(); return; }
#endif
    if (sizeof(R) == 8) { *p = o + d * t; *p_lo = V3<R>(); return; }
  }
  const V3<R> w = (p1 - p0) * u + (p2 - p0) * v;
  const V3<R> s = p0 + w;
  if (SITE && sizeof(R) == 8) { *p = s; *p_lo = V3<R>(); return; }
  const V3<R> bb = s - p0;
  *p = s;
  *p_lo = (p0 - (s - bb)) + (w - bb);
}

// Triangle::intersect's SurfaceInteraction (shape/triangle.rs:267-390) rebuilt from (triangle, t, u, v)
// SITE (rrt_surface_at): from (triangle, u, v) alone - o, d and t are not read, wo is not meaningful, and `prim` is a triangle (a sphere's
// interaction needs the ray). Every other statement is the one the hit form runs.
template <typename R, bool SITE = false>
RRT_DEV Surf<R> build_surface(const SceneDev<R>& s, int prim, V3<R> o, V3<R> d, R t, R u, R v, SurfExt<R>* ext = nullptr) {
  Surf<R> si;
  const Tri<R> tr = s.tris[prim];
  if (!SITE && tr.plane == kSphereMark) {   // u = root branch recorded by the traversal (public API reports 0, 0 for spheres)
    SphereSI<R> ss;
    sphere_surface(s.spheres[tr.shade], o, d, t, u, &ss, ext);
    si.ok = true;
    si.p = ss.p; si.p_lo = V3<R>(); si.n = ss.n; si.wo = ss.wo; si.sn = ss.sn; si.sdpdu = ss.sdpdu;
    si.material = tr.material;
    if (!(dot(si.n, si.sn) >= R(0))) si.ok = false;   // primitives.rs:66
    return si;
  }
  const bool inst = is_inst_tri(tr);
  if (!SITE && inst) {   // the triangle works with the ray TransformedPrimitive::intersect handed it (primitives.rs:124-127)
    const InstDev<R>& I = s.insts[inst_of(tr)];
    o = aff_pt(I.mi, o); d = vnormalize(vnormalize(aff_vec(I.mi, d)));
  }
  V3<R> p0(tr.p0), p1(tr.p1), p2(tr.p2);
  R uv[3][2] = {{R(0), R(0)}, {R(1), R(0)}, {R(1), R(1)}};  // get_uvs :113-128
  uint32_t has_n = 0;
  V3<R> vn0, vn1, vn2;
  if (tr.shade != 0xffffffffu) {
    const TriShade<R>& sh = s.shades[tr.shade];
    if (sh.has_uv) for (int k = 0; k < 3; k++) { uv[k][0] = sh.uv[k][0]; uv[k][1] = sh.uv[k][1]; }
    has_n = sh.has_n;
    if (has_n == 1) { vn0 = V3<R>(sh.n[0]); vn1 = V3<R>(sh.n[1]); vn2 = V3<R>(sh.n[2]); }
  }
  R duv02[2] = {uv[0][0] - uv[2][0], uv[0][1] - uv[2][1]}, duv12[2] = {uv[1][0] - uv[2][0], uv[1][1] - uv[2][1]};
  V3<R> dp02 = p0 - p2, dp12 = p1 - p2;
  R determinant = duv02[0] * duv12[1] - duv02[1] * duv12[0];
  bool degenerate_uv = rabs(determinant) < R(1e-8);
  V3<R> dpdu, dpdv;
  if (!degenerate_uv) {
    R i_det = R(1) / determinant;
    dpdu = (dp02 * duv12[1] - dp12 * duv02[1]) * i_det;
    dpdv = (dp02 * -duv12[0] + dp12 * duv02[0]) * i_det;
  }
  if (degenerate_uv || len2(cross(dpdu, dpdv)) == R(0)) {
    V3<R> ng = cross(p2 - p0, p1 - p0);
    coordinate_system(vnormalize(ng), &dpdu, &dpdv);
  }
  spawn_point<R, SITE>(o, d, t, u, v, p0, p1, p2, &si.p, &si.p_lo);
  si.wo = -d;
  si.n = vnormalize(cross(dp02, dp12));
  si.sn = si.n;
  si.sdpdu = dpdu;
  si.material = inst ? (tr.material & 0xffffu) : tr.material;
  si.ok = true;
  if (ext) {
    ext->u = uv[0][0] * (R(1) - u - v) + uv[1][0] * u + uv[2][0] * v;
    ext->v = uv[0][1] * (R(1) - u - v) + uv[1][1] * u + uv[2][1] * v;
    ext->dpdu = dpdu; ext->dpdv = dpdv; ext->sdpdv = dpdv;
    ext->sdndu = ext->sdndv = V3<R>();
    if (has_n == 1) {   // triangle.rs:351-386
      const V3<R> dn1 = vn0 - vn2, dn2 = vn1 - vn2;
      if (degenerate_uv) {
        const V3<R> dn = cross(vn2 - vn0, vn1 - vn0);
        if (len2(dn) != R(0)) coordinate_system(dn, &ext->sdndu, &ext->sdndv);
      } else {
        const R i_det = R(1) / determinant;
        ext->sdndu = (dn1 * duv12[1] - dn2 * duv02[1]) * i_det;
        ext->sdndv = (dn1 * -duv12[0] + dn2 * duv02[0]) * i_det;
      }
    }
  }
  if (has_n == 1) {
    V3<R> ns = vn0 * (R(1) - u - v) + vn1 * u + vn2 * v;
    if (len2(ns) > R(0)) ns = nnormalize(ns); else ns = si.n;
    V3<R> ss = vnormalize(dpdu);
    V3<R> ts = cross(ss, ns);
    if (len2(ts) > R(0)) { ts = vnormalize(ts); ss = cross(ts, ns); }
    else coordinate_system(ns, &ss, &ts);
    // set_shading_geometry(.., orientation_is_authoritative = true) interaction.rs:183-202: the *geometric*
    // normal is flipped towards the interpolated frame and stored as the shading normal (Q14) ...
    V3<R> nn = nnormalize(cross(ss, ts));
    si.sn = faceforward(si.n, nn);
    si.sdpdu = ss;
    if (ext) ext->sdpdv = ts;
    // ... and primitives.rs:66 asserts dot(ist.n, shading.n) >= 0, i.e. panics when vn opposes the winding.
    if (!(dot(si.n, si.sn) >= R(0))) si.ok = false;
  }
  if (inst) {   // `*si = primitive_to_world.t(si)` primitives.rs:131-136 + SurfaceInteraction::t_by transform.rs:628-655
    const InstDev<R>& I = s.insts[inst_of(tr)];
    if (!I.identity) {
      si.p = aff_pt(I.m, si.p + si.p_lo); si.p_lo = V3<R>();
      si.wo = aff_vec(I.m, si.wo);                       // (not re-normalised: its length is the instance's scale along the ray)
      const V3<R> n2 = aff_nrm(I.mi, si.n);              // BaseInteraction::t_by: not re-normalised either
      si.sn = faceforward(nnormalize(aff_nrm(I.mi, si.sn)), n2);
      si.n = n2;
      si.sdpdu = aff_vec(I.m, si.sdpdu);
      if (ext) {
        ext->dpdu = aff_vec(I.m, ext->dpdu); ext->dpdv = aff_vec(I.m, ext->dpdv); ext->sdpdv = aff_vec(I.m, ext->sdpdv);
        ext->sdndu = aff_nrm(I.mi, ext->sdndu); ext->sdndv = aff_nrm(I.mi, ext->sdndv);
      }
    }
  }
  return si;
}

template <typename R, int NL, uint32_t KM>
RRT_DEV bool build_bsdf(const SceneDev<R>& s, const Surf<R>& si, Bsdf<R, NL, KM>* b, bool allow_multiple_lobes = true) {  // Bsdf::new reflection.rs:215-226
  b->ns = si.sn;
  b->ss = vnormalize(si.sdpdu);
  b->ng = si.n;
  b->ts = cross(b->ns, b->ss);
  return build_lobes(s.materials[si.material], b, allow_multiple_lobes);
}
// textured scenes: compute_differentials (interaction.rs:209), then the material's textures at this hit, then the lobes.
// Returns false for a Glass / Translucent whose evaluated colours are all black: the reference leaves `bsdf` None there
// and path.rs:103 underflows `bounces` (constant materials are checked on the host).
template <typename R, int NL, uint32_t KM>
RRT_DEV bool build_bsdf_tex(const SceneDev<R>& s, Surf<R>& si, const SurfExt<R>& ext, const DiffRay<R>& rd, TexCtx<R>* c,
                            Bsdf<R, NL, KM>* b, bool allow_multiple_lobes = true) {
  c->p = si.p; c->u = ext.u; c->v = ext.v;
  c->pd = V3<double>((double)si.p.x + (double)si.p_lo.x, (double)si.p.y + (double)si.p_lo.y, (double)si.p.z + (double)si.p_lo.z);
  compute_differentials(c, si.n, ext.dpdu, ext.dpdv, rd);
  const int bump = s.materials[si.material].bump;
  if (bump >= 0) {   // Material::bump material/mod.rs:22-62: the displacement texture at (u + du, v), (u, v + dv) and (u, v)
    TexCtx<R> ev = *c;
    R du = rabs(c->dudx) * R(0.5) + rabs(c->dudy);   // (as written at :26)
    if (du == R(0)) du = R(0.0005);
    auto step_d = [&](V3<R> dir, R h) { return V3<double>(c->pd.x + (double)dir.x * (double)h, c->pd.y + (double)dir.y * (double)h, c->pd.z + (double)dir.z * (double)h); };
    ev.p = si.p + si.sdpdu * du; ev.pd = step_d(si.sdpdu, du); ev.u = c->u + du; ev.v = c->v;
    const R u_displace = TexEval<R, kTexDepth>::eval(s, bump, ev).r;
    R dv = (rabs(c->dvdx) + rabs(c->dvdy)) * R(0.5);
    if (dv == R(0)) dv = R(0.0005);
    ev.p = si.p + ext.sdpdv * dv; ev.pd = step_d(ext.sdpdv, dv); ev.u = c->u; ev.v = c->v + dv;
    const R v_displace = TexEval<R, kTexDepth>::eval(s, bump, ev).r;
    const R displace = TexEval<R, kTexDepth>::eval(s, bump, *c).r;
    c->err |= ev.err;
    const V3<R> dpdu = si.sdpdu + si.sn * (u_displace - displace) / du + ext.sdndu * displace;
    const V3<R> dpdv = ext.sdpdv + si.sn * (v_displace - displace) / dv + ext.sdndv * displace;
    // set_shading_geometry(.., orientation_is_authoritative = false) interaction.rs:183-202
    si.sn = faceforward(nnormalize(cross(dpdu, dpdv)), si.n);
    si.sdpdu = dpdu;
  }
  b->ns = si.sn;
  b->ss = vnormalize(si.sdpdu);
  b->ng = si.n;
  b->ts = cross(b->ns, b->ss);
  const Material<R> m = resolve_material(s, s.materials[si.material], *c);
  build_lobes(m, b, allow_multiple_lobes);
  if (c->err) return false;
  if (m.type == 5 && rgb_clamp0(Rgb<R>(m.kr)).is_black() && rgb_clamp0(Rgb<R>(m.kt)).is_black()) return false;
  if (m.type == 6 && rgb_clamp0(Rgb<R>(m.reflect)).is_black() && rgb_clamp0(Rgb<R>(m.transmit)).is_black()) return false;
  return true;
}

// Light::sample_li for PointLight (point.rs:55-77) and DiffuseAreaLight (diffuse.rs:63-79) over
// Shape::sample_ref (shape/mod.rs:33-48), Sphere::sample (sphere.rs:265-285), Triangle::sample (triangle.rs:393-418)
template <typename R, bool AREA = true>
RRT_DEV Rgb<R> light_sample_li(const Light<R>& L, V3<R> ref_p, R u0, R u1, V3<R>* wi, R* pdf, V3<R>* p1, V3<R>* n1) {
  if (!AREA && L.type != 0 && L.type != 2) __builtin_unreachable();   // (instantiation for scenes whose lights are all point / distant: the host checks, rrt_impl.hpp)
  if (L.type == 0) {
    V3<R> pl(L.p_light);
    *wi = vnormalize(pl - ref_p);
    *pdf = R(1);
    *p1 = pl; *n1 = V3<R>();
    return Rgb<R>(L.spectrum) / len2(pl - ref_p);
  }
  if (L.type == 2) {   // DistantLight::sample_li distant.rs:67-92
    const V3<R> w(L.w_light);
    *wi = w;
    *pdf = R(1);
    *p1 = ref_p + w * (R(2) * L.world_radius); *n1 = V3<R>();
    return Rgb<R>(L.spectrum);
  }
  V3<R> p, n;
  if (L.shape_type == 1) {
    V3<R> p_obj = uniform_sample_sphere(u0, u1) * L.radius;
    n = nnormalize(aff_nrm(L.mi, p_obj));
    p_obj = p_obj * (L.radius / len(p_obj));
    p = aff_pt(L.m, p_obj);
  } else {
    V3<R> b = uniform_sample_sphere(u0, u1);  // used as barycentrics (Q19)
    V3<R> q0(L.tp[0]), q1(L.tp[1]), q2(L.tp[2]);
    p = q0 * b.x + q1 * b.y + q2 * b.z;
    n = vnormalize(cross(q1 - q0, q2 - q0));
    if (L.tri_has_n) {
      V3<R> ns = V3<R>(L.tn[0]) * b.x + V3<R>(L.tn[1]) * b.y + V3<R>(L.tn[2]) * b.z;
      n = faceforward(n, ns);
    }
  }
  V3<R> w = p - ref_p;
  R wl2 = len2(w), pd;
  if (wl2 == R(0)) pd = R(0);
  else {
    w = vnormalize(w);
    pd = wl2 / absdot(-w, n);
    if (isinf(pd)) pd = R(0);
  }
  *pdf = pd;
  if (pd == R(0) || len2(p - ref_p) == R(0)) { *pdf = R(0); return Rgb<R>(); }
  *wi = vnormalize(p - ref_p);
  *p1 = p; *n1 = n;
  return (dot(n, -*wi) > R(0)) ? Rgb<R>(L.spectrum) : Rgb<R>();  // DiffuseAreaLight::l diffuse.rs:133-141
}

// estimate_direct's light-sampling half (integrator/mod.rs:403-481), handle_media = false, specular = false.
// Returns true and fills the shadow ray + contribution when a visibility test is needed.
// The BSDF-sampling half (:483-556) can only add `li * f * weight / pdf` with li = 0 (no primitive carries an
// area light, Q18; DiffuseAreaLight::le is the trait default 0), so it is not executed: see DESIGN.md.
template <bool AREA = true, typename R, int NL, uint32_t KM>
RRT_DEV bool estimate_direct_light(const Surf<R>& si, const Bsdf<R, NL, KM>& bsdf, const Light<R>& L, R ul0, R ul1, V3<R>* so, V3<R>* sd, Rgb<R>* ld) {
  const uint32_t flags = BXDF_ALL & ~BXDF_SPECULAR;
  V3<R> wi, p1, n1;
  R light_pdf = R(0);
  Rgb<R> li = light_sample_li<R, AREA>(L, si.p, ul0, ul1, &wi, &light_pdf, &p1, &n1);
  if (!(light_pdf > R(0)) || li.is_black()) return false;
  Rgb<R> f = bsdf.f(si.wo, wi, flags) * absdot(wi, si.sn);
  R scattering_pdf = bsdf.pdf(si.wo, wi, flags);
  if (f.is_black()) return false;
  // spawn_ray_to_si interaction.rs:66-77 with p_error = 0 (Q8): origin = p, target = p1, Ray::new normalises d
  // and keeps t_max = 1 - SHADOW_EPSILON (Q9)
  *so = si.p;
  *sd = vnormalize(p1 - si.p);
  if (!AREA || L.type != 1) *ld = f * li / light_pdf;   // delta lights (point, distant): no MIS
  else { R w = power_heuristic1(light_pdf, scattering_pdf); *ld = li * f * w / light_pdf; }
  return true;
}

// Distribution1D::sample_discrete sampling.rs:93-123 on the uniform light distribution
template <typename R>
RRT_DEV uint32_t sample_light_discrete(const SceneDev<R>& s, R u) {
  uint32_t first = 0, len = s.n_lights + 1;
  while (len > 0) {
    uint32_t half = len >> 1, middle = first + half;
    if (s.light_cdf[middle] <= u) { first = middle + 1; len -= half + 1; } else len = half;
  }
  uint32_t off = first - 1;
  if (off > s.n_lights - 1) off = s.n_lights - 1;
  return off;
}

// PathIntegrator::li loop body (path.rs:74-223) for one bounce of every active path.
// occupancy target of the path shading kernel: asking for 4 waves per SIMD lets the register allocator use the full
// 128-VGPR budget of that occupancy (measured: 8.9 ms against 9.9 ms without the hint; 5 or 6 waves spill: 10.6 / 13.2 ms)
#ifndef RRT_SHADE_CHUNK
#define RRT_SHADE_CHUNK 4u   // queue entries per workgroup and trip of the hit compaction, in workgroup sizes (measured: 2 / 4 / 8 - see DESIGN.md)
#endif
#ifndef RRT_SHADE_WAVES
#define RRT_SHADE_WAVES 4
#endif
// The Lambert-only instantiation needs 96 VGPRs unforced; measured (shading alone / frame with two in flight, config 4): 4 waves per SIMD
// 5.87 ms, 5: 5.58 / 37.8, 6: 5.43 / 37.7, 7: 5.35 / 37.6, 8: 5.64; with 512-thread blocks 5: 5.61 / 38.0, 6: 4.92 / 37.4, 7: 5.01 / 37.3; 1024: 6.39.
#ifndef RRT_SHADE_WAVES_LAMBERT
#define RRT_SHADE_WAVES_LAMBERT 6
#endif
#ifndef RRT_SHADE_BLOCK_LAMBERT
#define RRT_SHADE_BLOCK_LAMBERT 512
#endif
#ifndef RRT_SHADE_WAVES_GLOSSY
#define RRT_SHADE_WAVES_GLOSSY RRT_SHADE_WAVES
#endif
#ifndef RRT_SHADE_BLOCK_GLOSSY
#define RRT_SHADE_BLOCK_GLOSSY RRT_SHADE_BLOCK
#endif
template <typename R, uint32_t KM> constexpr int shade_path_block() {
  return sizeof(R) != 4 ? ShadeBlock<R>::n : (KM == kKindsLambert ? RRT_SHADE_BLOCK_LAMBERT : (KM == kKindsGlossy ? RRT_SHADE_BLOCK_GLOSSY : ShadeBlock<R>::n));
}
template <uint32_t KM> constexpr int shade_path_waves() { return KM == kKindsLambert ? RRT_SHADE_WAVES_LAMBERT : (KM == kKindsGlossy ? RRT_SHADE_WAVES_GLOSSY : RRT_SHADE_WAVES); }
// TEX: the scene has materials that evaluate a texture per hit (SurfExt + ray differentials of the camera ray at bounce 0;
// `ray = isect.spawn_ray(wi).into()` drops them afterwards, path.rs:163).
// KM: the lobe kinds the scene's materials can produce (dmath.hpp "Lobe-kind sets"); kAllKinds = the general kernel.
// AREA = false: every light of the scene is a point or distant light (no area-light sampling code, no light sample dimensions drawn).
// PASSES: the launch belongs to a frame of rrt_render_passes - a shadow record's pass mask (Pools::pass_tab) rides in bits 8 .. 23 of sh_tab, which the
// start-triangle word's `<< 24` drops, and is stored beside the record (Pools::smask). A template flag, not a pointer test: the instantiations every
// other frame launches are the code they were, register for register.
template <typename R, int NL, bool TEX = false, uint32_t KM = kAllKinds, bool AREA = true, bool PASSES = false>
__global__ void __launch_bounds__((shade_path_block<R, KM>())) __attribute__((amdgpu_waves_per_eu(TEX ? 1 : shade_path_waves<KM>(), 8))) k_shade_path(SceneDev<R> s, Pools<R> p) {
  __shared__ uint32_t push_lds[shade_path_block<R, KM>() / 64 + 1];
  // [r4] Hit compaction (option "shade_compact"). More than half of a queue's rays MISS on an open scene (config 4: 104 M queued closest-hit rays, ~47 M hits per
  // frame), and the path integrator shades a miss with nothing (Q18) - with one thread per queue entry half of every wave sat idle through the whole kernel. A
  // workgroup now takes kShadeChunk x its size consecutive entries, reads their hit words, packs the indices of the hits into LDS in queue order (block_rank) and
  // shades those with full waves. The next / shadow queues receive the same entries in the same order inside a workgroup's chunk; every sample adds to its own slot:
  // frames are identical bit for bit (tests/test_gpu_parity.py::test_shade_compaction_changes_nothing).
  constexpr uint32_t kShadeChunk = RRT_SHADE_CHUNK;
  __shared__ uint32_t hit_idx[kShadeChunk * shade_path_block<R, KM>()];
  const uint32_t n = p.counters[C_ACTIVE];
  using V4 = typename Vec4T<R>::type;
  const uint32_t chunk = s.shade_compact ? kShadeChunk : 1u;
  // a bounded grid walks the queue (block-uniform trip counts, as block_push needs): the host does not know the queue
  // size, and a grid sized for the whole pass costs 0.2 ms of empty blocks per launch once the queues are short
  for (uint32_t base0 = blockIdx.x * blockDim.x * chunk; base0 < n; base0 += gridDim.x * blockDim.x * chunk) {
  uint32_t n_hits = min(blockDim.x, n - base0);   // (no compaction: the entries themselves)
  if (chunk > 1u) {
    n_hits = 0u;
    for (uint32_t k = 0; k < chunk; k++) {
      const uint32_t e = base0 + k * blockDim.x + threadIdx.x;
      const bool is_hit = e < n && (int)real_to_bits(p.hit[e].y) >= 0;
      uint32_t cnt = 0;
      const uint32_t at = block_rank(is_hit, push_lds, &cnt);
      if (is_hit) hit_idx[n_hits + at] = e;
      n_hits += cnt;
    }
    __syncthreads();
  }
  for (uint32_t base = 0; base < n_hits; base += blockDim.x) {
  const uint32_t i = base + threadIdx.x < n_hits ? (chunk > 1u ? hit_idx[base + threadIdx.x] : base0 + base + threadIdx.x) : n;   // n: no entry for this thread
  bool want_shadow = false, want_next = false, sky = false;
  uint32_t slot = 0;
  int prim = -1;
  V3<R> sh_o, sh_d, nx_o, nx_d, o_lo;   // shadow ray / next ray + path state, stored at their queue positions at the end
  Rgb<R> sh_ld, nx_beta;
  R nx_eta_scale = R(1);
  uint32_t index = 0, nx_db = 0, sh_tab = 0;
  if (i < n) {
    const QEnt qe = p.q_active[i];
    slot = qe.slot;
    const V4 h = p.hit[i];
    prim = (int)real_to_bits(h.y);
    const uint32_t db = qe.db;
    uint32_t dim = db_dim(s, db), bounces = db_bounce(s, db);
    // `if !found_intersection || bounces >= max_depth { break }` (:91); emitted light is 0 (Q18)
    if (prim >= 0 && (int)bounces < s.max_depth) {
      const V4 ro = p.ray_o[i], rd = p.ray_d[i];
      V3<R> o(ro.x, ro.y, ro.z), d(rd.x, rd.y, rd.z);
      SurfExt<R> ext;
      Surf<R> si = build_surface(s, prim, o, d, h.x, h.z, h.w, TEX ? &ext : nullptr);
      if (!si.ok) { atomicOr(&p.counters[C_ERROR], (uint32_t)ERR_SHADING_NORMAL); }
      else {
        Bsdf<R, NL, KM> bsdf;
        if (TEX) {
          DiffRay<R> dr;
          if (bounces == 0) {
            const V4 a = p.rdx_o[slot], b = p.rdx_d[slot], c = p.rdy_o[slot], e = p.rdy_d[slot];
            dr.has = true;
            dr.rxo = V3<R>(a.x, a.y, a.z); dr.rxd = V3<R>(b.x, b.y, b.z); dr.ryo = V3<R>(c.x, c.y, c.z); dr.ryd = V3<R>(e.x, e.y, e.z);
          }
          TexCtx<R> tc;
          if (!build_bsdf_tex(s, si, ext, dr, &tc, &bsdf)) atomicOr(&p.counters[C_ERROR], (uint32_t)(tc.err ? ERR_MIPMAP : ERR_NULL_BSDF));
        } else if (!build_bsdf(s, si, &bsdf)) atomicOr(&p.counters[C_ERROR], (uint32_t)ERR_KIND_SET);
        // a camera ray's path record is {1, 1, 1, 1} whoever produced it: not read (and, by the dense fp32 camera kernels under this integrator, not written)
        const V4 st_b = bounces == 0u ? mk4<R>(R(1), R(1), R(1), R(1)) : p.path[i];
        index = qe.index;
        Rgb<R> beta(st_b.x, st_b.y, st_b.z);
        R eta_scale = st_b.w;
        // uniform_sample_one_light integrator/mod.rs:359-401 with the uniform Distribution1D (path.rs:47-49)
        if (bsdf.num_components(BXDF_ALL & ~BXDF_SPECULAR) > 0 && s.n_lights > 0) {
          // Sampler values nobody reads are not computed, only counted (a radical inverse in a high dimension is ~6 digit
          // steps of f64 / u64 arithmetic, and these three were half of this kernel's draws): with one light the discrete
          // distribution returns light 0 for every u; point and distant lights ignore their 2D sample (point.rs:55-77,
          // distant.rs:67-92).
          double du0 = 0.0, du1 = 0.0;
          uint32_t ln = 0;
          if (s.n_lights == 1u) skip_1d(s, &dim);
          else ln = sample_light_discrete(s, to_real<R>(draw_1d(s, index, &dim)));
          if (!AREA || s.lights[ln].type != 1) skip_2d(s, &dim);
          else draw_2d(s, index, &dim, &du0, &du1);
          R ul0 = to_real<R>(du0), ul1 = to_real<R>(du1);
          skip_2d(s, &dim);  // u_scattering: drawn, only used by the BSDF-sampling half
          V3<R> so, sd;
          Rgb<R> ld;
          if (s.light_pick_pdf != R(0) && estimate_direct_light<AREA>(si, bsdf, s.lights[ln], ul0, ul1, &so, &sd, &ld)) {
            sh_ld = beta * (ld / s.light_pick_pdf);
            sh_o = so; sh_d = sd;
            sh_tab = s.use_shadow_tabs ? s.lights[ln].shadow_tab : 0u;
            if (PASSES) sh_tab |= (p.pass_tab[ln] & p.pass_tab[s.n_lights + bounces]) << 8;   // `bounces` is still this vertex's number (path.rs:51-226)
            want_shadow = true;
          }
        }
        o_lo = si.p_lo;
        // Sample BSDF to get new path direction (:125-148)
        double db0, db1;
        draw_2d(s, index, &dim, &db0, &db1);
        R u0 = to_real<R>(db0), u1 = to_real<R>(db1);
        V3<R> wi;
        R pdf = R(0);
        uint32_t flags = 0;
        // `let wo = -ray.d` (path.rs:126): the WORLD ray's direction, not the interaction's wo - which estimate_direct uses (integrator/mod.rs:441)
        // and which differs from it on a non-rigid instance (transformed back, not re-normalised: primitives.rs:131-136) and by rounding on a sphere
        const V3<R> wo_path = -d;
        Rgb<R> f = bsdf.sample_f(wo_path, &wi, u0, u1, &pdf, BXDF_ALL, &flags);
        if (!(f.is_black() || pdf == R(0))) {
          beta = beta * (f * absdot(wi, si.sn) / pdf);
          if (!(beta.y() > R(0)) || isinf(beta.y()) || beta.y() != beta.y()) atomicOr(&p.counters[C_ERROR], (uint32_t)ERR_BETA);  // path.rs:146-147 asserts
          if ((flags & BXDF_SPECULAR) && (flags & BXDF_TRANSMISSION))   // path.rs:150-162
            eta_scale *= dot(wo_path, si.n) > R(0) ? bsdf.eta * bsdf.eta : R(1) / (bsdf.eta * bsdf.eta);
          V3<R> nd = vnormalize(wi);  // spawn_ray -> Ray::new_od (Q8: no origin offset)
          bool cont = true;
          // Russian roulette (:214-222) on beta * eta_scale
          const R rr_max = (beta * eta_scale).max_component();
          if (rr_max < s.rr_threshold && bounces > 3) {
            R q = rmax(R(1) - rr_max, R(0.05));
            R ur = to_real<R>(draw_1d(s, index, &dim));
            if (ur < q) cont = false;
            else beta = beta / (R(1) - q);
          }
          bounces += 1;
          // the next loop iteration would trace and then break on `bounces >= max_depth` without using the
          // hit (emission is 0): that dead closest-hit query is not issued.
          // Horizon cull (SceneDev::horizon, host/horizon_build.cpp): the next ray starts on triangle `prim`; if its elevation above / below the scene's
          // flattest axis exceeds everything the host found visible from ANY point of that triangle in the ray's azimuth sector, BVHAccel::intersect would
          // return false for it and the path would end at `if !found_intersection { break }` (path.rs:91) - it is counted as the closest-hit query it is, and not traced.
          if (cont && (int)bounces < s.max_depth && s.horizon != nullptr) {
            const float u = s.hz_axis == 0u ? (float)nd.x : (s.hz_axis == 1u ? (float)nd.y : (float)nd.z);
            const float a = s.hz_axis == 0u ? (float)nd.y : (s.hz_axis == 1u ? (float)nd.z : (float)nd.x), b = s.hz_axis == 0u ? (float)nd.z : (s.hz_axis == 1u ? (float)nd.x : (float)nd.y);
            const uint32_t q = s.horizon[(size_t)prim * 32u + (u < 0.0f ? 16u : 0u) + hz_sector(a, b)];
            // (the tables speak for rays that start ON the triangle; the spawn point is within 2^-24 x the scene's size of its plane, and the ray's line then meets the
            // plane inside the triangle - where the tables hold - if the point is this far from the edges for this inclination: HzTables::tau. Both loads are issued
            // before either comparison: one latency, not two in a row)
#ifdef RRT_HZ_NO_GUARD   // measurement variant only
            const float tau = -1.0f;
#else
            const float tau = s.hz_tau[prim];
#endif
            const bool above = fabsf(u) * 254.0f > (float)q;
            const bool inside = fminf(fminf((float)h.z, (float)h.w), 1.0f - (float)h.z - (float)h.w) * fabsf((float)dot(si.n, nd)) > tau;
            if (above && inside) { cont = false; sky = true; }
          }
          if (cont && (int)bounces < s.max_depth) {
            nx_o = si.p; nx_d = nd;
            nx_beta = beta; nx_eta_scale = eta_scale;
            nx_db = db_pack(s, dim, bounces);
            want_next = true;
          }
        }
      }
    }
  }
  const uint32_t qs = block_push(p.shadow_count, want_shadow, push_lds);
  if (want_shadow) {
    store_ray<R>(p.sray_o, p.sray_d, qs, sh_o, o_lo, sh_d, R(1) - R(0.0001), self_prim<R>(prim) | (int)(sh_tab << 24));   // (sh_tab != 0 only in fp32, where prim >= 0 and < 2^19)
    p.sld[qs] = mk4u<R>(sh_ld.r, sh_ld.g, sh_ld.b, slot);
    if (PASSES) p.smask[qs] = sh_tab >> 8;
  }
  const uint32_t qn = block_push(&p.counters[C_NEXT], want_next, push_lds);
  if (want_next) {
    p.q_next[qn] = QEnt{slot, nx_db, index, 0u};
    p.npath[qn] = mk4<R>(nx_beta.r, nx_beta.g, nx_beta.b, nx_eta_scale);
    store_ray<R>(p.nray_o, p.nray_d, qn, nx_o, o_lo, nx_d, Const<R>::inf, self_prim<R>(prim));
  }
  if (s.horizon != nullptr) (void)block_push(&p.counters[C_SKY], sky, push_lds);   // (block-uniform condition)
  }  // the chunk's hits
  __syncthreads();   // hit_idx is rewritten by the next chunk
  }  // queue walk
}

// DirectLighting / Debug integrators (directlighting.rs:72-132, intersect_debug.rs:56-89) as a wavefront chain:
// one NEE launch per light (strategy all) or one (strategy one), then the specular continuation.
// mode: light_j >= 0 -> uniform_sample_all_lights' j-th term; light_j == -1 -> uniform_sample_one_light(None).
template <typename R>
__global__ void __launch_bounds__(ShadeBlock<R>::n) k_shade_nee(SceneDev<R> s, Pools<R> p, int light_j, int first) {
  __shared__ uint32_t push_lds[ShadeBlock<R>::n / 64 + 1];
  using V4 = typename Vec4T<R>::type;
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t n = p.counters[C_ACTIVE];
  if (blockIdx.x * blockDim.x >= n) return;   // whole block past the queue end (the grid is sized for the worst case)
  bool want_shadow = false;
  uint32_t slot = 0, sh_tab = 0;
  int prim = -1;
  V3<R> sh_o, sh_d, o_lo;
  Rgb<R> sh_ld;
  if (i < n) {
    const QEnt qe = p.q_active[i];
    slot = qe.slot;
    const V4 h = p.hit[i];
    prim = (int)real_to_bits(h.y);
    if (prim >= 0) {
      const V4 ro = p.ray_o[i], rd = p.ray_d[i];
      V3<R> o(ro.x, ro.y, ro.z), d(rd.x, rd.y, rd.z);
      Surf<R> si = build_surface(s, prim, o, d, h.x, h.z, h.w);
      if (!si.ok) atomicOr(&p.counters[C_ERROR], (uint32_t)ERR_SHADING_NORMAL);
      else {
        Bsdf<R> bsdf;
        build_bsdf(s, si, &bsdf, false);   // allow_multiple_lobes = false (directlighting.rs:91)
        const uint32_t db = qe.db;
        uint32_t dim = db_dim(s, db);
        const V4 st_b = p.path[i];
        const uint32_t index = qe.index;
        Rgb<R> beta(st_b.x, st_b.y, st_b.z);
        if (first && s.integrator == 2) {  // Debug: l = Spectrum(0.1) on a hit (intersect_debug.rs:66-70)
          V4 l = p.L[slot];
          l.x += beta.r * R(0.1); l.y += beta.g * R(0.1); l.z += beta.b * R(0.1);
          p.L[slot] = l;
        }
        uint32_t ln;
        R pick_pdf = R(1);
        if (light_j >= 0) ln = (uint32_t)light_j;
        else {
          R u_pick = to_real<R>(draw_1d(s, index, &dim));
          R v = u_pick * (R)s.n_lights;
          uint32_t vi = (v != v || v <= R(0)) ? 0u : (uint32_t)v;
          ln = vi < s.n_lights - 1 ? vi : s.n_lights - 1;
          pick_pdf = R(1) / (R)s.n_lights;
        }
        double du0, du1;
        draw_2d(s, index, &dim, &du0, &du1);
        R ul0 = to_real<R>(du0), ul1 = to_real<R>(du1);
        skip_2d(s, &dim);  // u_scattering
        V3<R> so, sd;
        Rgb<R> ld;
        if (estimate_direct_light(si, bsdf, s.lights[ln], ul0, ul1, &so, &sd, &ld)) {
          sh_ld = beta * (ld / pick_pdf);
          sh_o = so; sh_d = sd; o_lo = si.p_lo;
          sh_tab = s.use_shadow_tabs ? s.lights[ln].shadow_tab : 0u;
          want_shadow = true;
        }
        p.q_active[i].db = db_pack(s, dim, db_bounce(s, db));
      }
    }
  }
  const uint32_t qs = block_push(p.shadow_count, want_shadow, push_lds);
  if (want_shadow) {
    store_ray<R>(p.sray_o, p.sray_d, qs, sh_o, o_lo, sh_d, R(1) - R(0.0001), self_prim<R>(prim) | (int)(sh_tab << 24));
    p.sld[qs] = mk4u<R>(sh_ld.r, sh_ld.g, sh_ld.b, slot);
  }
}

// specular_reflect (integrator/mod.rs:150-198) as the chain's continuation; this chain only runs on scenes without
// transmissive or textured materials (those take k_direct_tree), where specular_transmit (:199-301) finds no lobe and
// its 2D draw lands after the recursion returns.
// `depth` of the reference starts at 1; the high half of dim_bounce stores depth - 1.
template <typename R>
__global__ void __launch_bounds__(ShadeBlock<R>::n) k_shade_specular(SceneDev<R> s, Pools<R> p, int grey_only) {
  __shared__ uint32_t push_lds[ShadeBlock<R>::n / 64 + 1];
  using V4 = typename Vec4T<R>::type;
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t n = p.counters[C_ACTIVE];
  if (blockIdx.x * blockDim.x >= n) return;   // whole block past the queue end (the grid is sized for the worst case)
  bool want_next = false;
  uint32_t slot = 0;
  int prim = -1;
  V3<R> nx_o, nx_d, o_lo;
  Rgb<R> nx_beta;
  uint32_t index = 0, nx_db = 0;
  if (i < n) {
    const QEnt qe = p.q_active[i];
    slot = qe.slot;
    const V4 h = p.hit[i];
    prim = (int)real_to_bits(h.y);
    // DirectLightingIntegrator::li on a miss: `for light in &scene.lights { .. return l }` falls through to a call of itself when the
    // list is empty (directlighting.rs:83-99, Q20): unbounded recursion in the reference, a panic here
    if (prim < 0 && s.integrator == 1 && s.n_lights == 0u) atomicOr(&p.counters[C_ERROR], (uint32_t)ERR_NO_LIGHTS);
    if (prim >= 0) {
      const V4 st_b = p.path[i];
      const uint32_t db = qe.db;
      uint32_t dim = db_dim(s, db);
      const uint32_t depth = db_bounce(s, db) + 1;
      Rgb<R> beta(st_b.x, st_b.y, st_b.z);
      index = qe.index;
      if (grey_only) {  // Debug with no lights still adds the 0.1 grey
        V4 l = p.L[slot];
        l.x += beta.r * R(0.1); l.y += beta.g * R(0.1); l.z += beta.b * R(0.1);
        p.L[slot] = l;
      }
      if ((int)(depth + 1) < s.max_depth) {
        const V4 ro = p.ray_o[i], rd = p.ray_d[i];
        V3<R> o(ro.x, ro.y, ro.z), d(rd.x, rd.y, rd.z);
        Surf<R> si = build_surface(s, prim, o, d, h.x, h.z, h.w);
        if (si.ok) {
          Bsdf<R> bsdf;
          build_bsdf(s, si, &bsdf, false);
          double db0, db1;
          draw_2d(s, index, &dim, &db0, &db1);
          R u0 = to_real<R>(db0), u1 = to_real<R>(db1);
          V3<R> wi;
          R pdf = R(0);
          uint32_t st = 0;
          Rgb<R> f = bsdf.sample_f(si.wo, &wi, u0, u1, &pdf, BXDF_SPECULAR | BXDF_REFLECTION, &st);
          if (pdf > R(0) && !f.is_black() && absdot(wi, si.sn) != R(0)) {
            nx_beta = beta * (f * absdot(wi, si.sn) / pdf);
            nx_o = si.p; nx_d = vnormalize(wi); o_lo = si.p_lo;
            nx_db = db_pack(s, dim, depth);
            want_next = true;
          }
        }
      }
    }
  }
  const uint32_t qn = block_push(&p.counters[C_NEXT], want_next, push_lds);
  if (want_next) {
    p.q_next[qn] = QEnt{slot, nx_db, index, 0u};
    p.npath[qn] = mk4<R>(nx_beta.r, nx_beta.g, nx_beta.b, R(1));
    store_ray<R>(p.nray_o, p.nray_d, qn, nx_o, o_lo, nx_d, Const<R>::inf, self_prim<R>(prim));
  }
}

// DirectLighting / Debug with transmissive materials. `l += specular_reflect(..) + specular_transmit(..)`
// (directlighting.rs:126-129, integrator/mod.rs:150-301) makes li() a binary recursion, and the sampler dimensions are
// consumed depth-first: the transmit draw of a vertex comes after everything its reflect subtree drew, which depends on
// what that subtree hit. A breadth-first wavefront cannot know that count, so here one thread walks one camera
// sample's whole tree with an explicit stack (traversal, shading and shadow tests inline; a vertex is re-intersected
// when its reflect subtree returns instead of keeping its interaction on the stack). A correctness path, not a fast one.
// TEX: textured materials; every frame then carries its ray's differentials, which specular children inherit
// (integrator/mod.rs:183-201, 238-292) - the reason textured scenes take this kernel even without transmissive materials.
// The explicit stack holds one frame per level of the recursion (at most max_depth): the first kTreeMax in registers / scratch, deeper
// ones in a strided global array `deep` ([level - kTreeMax][thread of the launch], TreeFrame<R> each; null when max_depth <= kTreeMax).
constexpr int kTreeMax = 16;
template <typename R> struct TreeFrame { V3<R> o, d, lo; Rgb<R> beta; int skip, depth, phase; DiffRay<R> dr; };
template <typename R, bool TEX>
__global__ void __launch_bounds__(kBlock) k_direct_tree(SceneDev<R> s, Pools<R> p, unsigned long long* totals, TreeFrame<R>* deep, uint32_t deep_stride) {
  using V4 = typename Vec4T<R>::type;
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= p.counters[C_ACTIVE]) return;
  uint32_t n_closest = 0, n_any = 0;   // query counts for rrt_stats (totals[2], totals[3])
  const QEnt qe = p.q_active[i];
  const uint32_t index = qe.index;
  uint32_t dim = db_dim(s, qe.db);
  using Frame = TreeFrame<R>;
  Frame st[kTreeMax];
  auto frame = [&](int k) -> Frame& { return k < kTreeMax ? st[k] : deep[(size_t)(k - kTreeMax) * deep_stride + i]; };
  const int sp_max = deep ? s.max_depth : kTreeMax;
  int sp = 0;
  {
    const V4 ro = p.ray_o[i], rd = p.ray_d[i];
    st[0].o = V3<R>(ro.x, ro.y, ro.z); st[0].d = V3<R>(rd.x, rd.y, rd.z); st[0].lo = V3<R>();
    st[0].beta = Rgb<R>(R(1)); st[0].skip = -1; st[0].depth = 1; st[0].phase = 0;   // li(ray, .., depth = 1)
    if (TEX) {
      const V4 a = p.rdx_o[qe.slot], b = p.rdx_d[qe.slot], c = p.rdy_o[qe.slot], e = p.rdy_d[qe.slot];
      st[0].dr.has = true;
      st[0].dr.rxo = V3<R>(a.x, a.y, a.z); st[0].dr.rxd = V3<R>(b.x, b.y, b.z); st[0].dr.ryo = V3<R>(c.x, c.y, c.z); st[0].dr.ryd = V3<R>(e.x, e.y, e.z);
    }
    sp = 1;
  }
  Rgb<R> L;
  const bool all_lights = s.integrator == 2 || s.light_strategy == 1 /* RRT_STRATEGY_ALL */;
  while (sp > 0) {
    Frame& f = frame(sp - 1);
    RayCtx<R> r = make_ctx(f.o, f.d, Const<R>::inf, f.lo);
    R hu = 0, hv = 0;
    uint32_t nn, np;
    int hit;
    { PrivStack stack; hit = traverse_closest(s, r, stack, f.skip, &hu, &hv, &nn, &np); }
    if (f.phase == 0) n_closest++;   // the phase-1 re-intersection is bookkeeping, not a reference query
    if (hit < 0) {   // `for light in lights { l += le; return l }`: le = 0; with no light at all DirectLighting recurses for ever (Q20)
      if (s.integrator == 1 && s.n_lights == 0u) atomicOr(&p.counters[C_ERROR], (uint32_t)ERR_NO_LIGHTS);
      sp--; continue;
    }
    SurfExt<R> ext;
    Surf<R> si = build_surface(s, hit, f.o, f.d, r.tmax, hu, hv, TEX ? &ext : nullptr);
    if (!si.ok) { atomicOr(&p.counters[C_ERROR], (uint32_t)ERR_SHADING_NORMAL); sp--; continue; }
    Bsdf<R, 4> bsdf;
    TexCtx<R> tc;
    const DiffRay<R> fdr = f.dr;   // (a child frame may reuse this frame's stack entry below)
    // allow_multiple_lobes = false (directlighting.rs:91, intersect_debug.rs:71)
    if (TEX) { if (!build_bsdf_tex(s, si, ext, fdr, &tc, &bsdf, false)) atomicOr(&p.counters[C_ERROR], (uint32_t)(tc.err ? ERR_MIPMAP : ERR_NULL_BSDF)); }
    else build_bsdf(s, si, &bsdf, false);
    const Rgb<R> beta = f.beta;
    const int depth = f.depth;
    uint32_t want = 0;   // lobe class of the continuation to try now
    if (f.phase == 0) {
      if (s.integrator == 2) L = L + beta * R(0.1);   // intersect_debug.rs:66-70
      if (s.n_lights > 0) {
        const uint32_t n_iter = all_lights ? s.n_lights : 1u;
        for (uint32_t j = 0; j < n_iter; j++) {
          uint32_t ln = j;
          R pick_pdf = R(1);
          if (!all_lights) {   // uniform_sample_one_light(.., None) integrator/mod.rs:377-386
            const R v = to_real<R>(draw_1d(s, index, &dim)) * (R)s.n_lights;
            const uint32_t vi = (v != v || v <= R(0)) ? 0u : (uint32_t)v;
            ln = vi < s.n_lights - 1 ? vi : s.n_lights - 1;
            pick_pdf = R(1) / (R)s.n_lights;
          }
          double du0, du1;
          draw_2d(s, index, &dim, &du0, &du1);
          skip_2d(s, &dim);   // u_scattering
          V3<R> so, sd;
          Rgb<R> ld;
          if (estimate_direct_light(si, bsdf, s.lights[ln], to_real<R>(du0), to_real<R>(du1), &so, &sd, &ld)) {
            RayCtx<R> sr = make_ctx(so, sd, R(1) - R(0.0001), si.p_lo);
            PrivStack stack;
            n_any++;
            if (!traverse_any(s, sr, stack, self_prim<R>(hit), &nn, &np)) L = L + beta * (ld / pick_pdf);
          }
        }
      }
      if (depth + 1 < s.max_depth) { f.phase = 1; want = BXDF_SPECULAR | BXDF_REFLECTION; }
      else sp--;
    } else {
      want = BXDF_SPECULAR | BXDF_TRANSMISSION;
      sp--;   // this vertex is finished once its transmit child (if any) is pushed
    }
    if (want) {   // specular_reflect / specular_transmit: one 2D draw each, whether or not such a lobe exists
      double db0, db1;
      draw_2d(s, index, &dim, &db0, &db1);
      V3<R> wi;
      R pdf = R(0);
      uint32_t sampled = 0;
      const Rgb<R> fs = bsdf.sample_f(si.wo, &wi, to_real<R>(db0), to_real<R>(db1), &pdf, want, &sampled);
      if (pdf > R(0) && !fs.is_black() && absdot(wi, si.sn) != R(0) && sp < sp_max) {
        Frame& c = frame(sp++);
        c.o = si.p; c.lo = si.p_lo; c.d = vnormalize(wi);
        c.beta = beta * (fs * absdot(wi, si.sn) / pdf);
        c.skip = self_prim<R>(hit); c.depth = depth + 1; c.phase = 0;
        c.dr = DiffRay<R>();
        if (TEX && fdr.has) {
          DiffRay<R> cd;
          cd.has = true;
          cd.rxo = si.p + tc.dpdx; cd.ryo = si.p + tc.dpdy;
          V3<R> ns = si.sn;
          V3<R> dndx = ext.sdndu * tc.dudx + ext.sdndv * tc.dvdx;
          V3<R> dndy = ext.sdndu * tc.dudy + ext.sdndv * tc.dvdy;
          const V3<R> wo = si.wo;
          if (want & BXDF_REFLECTION) {   // integrator/mod.rs:183-201 (the factor is 0.2 there, not pbrt's 2)
            const V3<R> dwodx = -fdr.rxd - wo, dwody = -fdr.ryd - wo;
            const R ddndx = dot(dwodx, ns) + dot(wo, dndx), ddndy = dot(dwody, ns) + dot(wo, dndy);
            cd.rxd = wi - dwodx + (dndx * dot(wo, ns) + ns * ddndx) * R(0.2);
            cd.ryd = wi - dwody + (dndy * dot(wo, ns) + ns * ddndy) * R(0.2);
          } else {                        // :238-292
            R eta = R(1) / bsdf.eta;
            if (dot(wo, ns) < R(0)) { eta = R(1) / eta; ns = -ns; dndx = -dndx; dndy = -dndy; }
            const V3<R> dwodx = -fdr.rxd - wo, dwody = -fdr.ryd - wo;
            const R ddndx = dot(dwodx, ns) + dot(wo, dndx), ddndy = dot(dwody, ns) + dot(wo, dndy);
            const R mu = eta * dot(wo, ns) - absdot(wi, ns);
            const R dmudx = ddndx * (eta - (eta * eta * dot(wo, ns)) / absdot(wi, ns));
            const R dmudy = ddndy * (eta - (eta * eta * dot(wo, ns)) / absdot(wi, ns));
            cd.rxd = wi - dwodx * eta + (dndx * mu + ns * dmudx);
            cd.ryd = wi - dwody * eta + (dndy * mu + ns * dmudy);
          }
          c.dr = cd;
        }
      }
    }
  }
  V4 l = p.L[qe.slot];
  l.x += L.r; l.y += L.g; l.z += L.b;
  p.L[qe.slot] = l;
  if (n_closest) atomicAdd(&totals[2], (unsigned long long)n_closest);
  if (n_any) atomicAdd(&totals[3], (unsigned long long)n_any);
}

// queue rotation between bounces: active <- next, next <- 0, shadow <- 0 (single thread)
static __global__ void k_rotate(uint32_t* c, int what) {
  if (what == 0) { c[C_ACTIVE] = c[C_NEXT]; c[C_NEXT] = 0; c[C_SHADOW] = 0; }
  else if (what == 1) { c[C_SHADOW] = 0; }
  else if (what == 3) { /* only the work counters */ }
  else if (what == 4) { c[C_NEXT] = 0; }
  // 5 / 6: the two halves of `0` when the shadow launch runs on its own stream beside the next closest-hit launch
  else if (what == 5) { c[C_ACTIVE] = c[C_NEXT]; c[C_NEXT] = 0; c[C_WORK_CLOSEST] = 0; c[C_WORK_AUX] = 0; for (int k = 0; k < 8; k++) c[C_WORK8_CLOSEST + 32 * k] = 0; return; }
  else if (what == 6) { c[C_SHADOW] = 0; c[C_WORK_SHADOW] = 0; for (int k = 0; k < 8; k++) c[C_WORK8_SHADOW + 32 * k] = 0; return; }
  else if (what == 7) { c[C_SHADOW2] = 0; c[C_WORK_SHADOW] = 0; for (int k = 0; k < 8; k++) c[C_WORK8_SHADOW + 32 * k] = 0; return; }
  else { c[C_ACTIVE] = 0; c[C_NEXT] = 0; c[C_SHADOW] = 0; c[C_RECORDS] = 0; }
  c[C_WORK_CLOSEST] = 0; c[C_WORK_SHADOW] = 0; c[C_WORK_AUX] = 0;
  for (int k = 0; k < 8; k++) { c[C_WORK8_CLOSEST + 32 * k] = 0; c[C_WORK8_SHADOW + 32 * k] = 0; }
}
static __global__ void k_accumulate_counts(uint32_t* c, unsigned long long* totals) {
  // totals[2] closest queries, totals[3] shadow queries, totals[4] camera rays
  totals[2] += c[C_ACTIVE];
}
static __global__ void k_accumulate_shadow(const uint32_t* shadow_count, unsigned long long* totals) { totals[3] += *shadow_count; }
// bounce rays answered by the horizon tables in the shading launch just finished: queries all the same (totals[8] says how many)
static __global__ void k_accumulate_sky(uint32_t* c, unsigned long long* totals) { totals[2] += c[C_SKY]; totals[8] += c[C_SKY]; c[C_SKY] = 0; }
// queries: 0 where the integrator never issues the camera rays' closest-hit query (Path at max_depth <= 0: it is the dead query at bounces == max_depth),
// so that the rays the root-box test answered are not counted as queries either
static __global__ void k_accumulate_camera(uint32_t* c, unsigned long long* totals, int queries) {
  totals[4] += c[C_CAMERA_RAYS]; c[C_CAMERA_RAYS] = 0;
  if (queries) totals[2] += c[C_CULLED];   // queries all the same: answered by the root-box test in the camera kernel
  totals[7] += c[C_CULLED]; c[C_CULLED] = 0;
}

// ------------------------------------------------------------------------------------------------------------
// Film: FilmTile::add_sample (film.rs:77-130) + merge_film_tile (:248-263, Q3) for the box filter of radius
// <= 0.5: every sample lands in its own pixel, so one thread owns a pixel and sums the pass's samples in sample
// order (deterministic, no atomics). film = per pixel {X, Y, Z sums, filter_weight_sum}.
// ------------------------------------------------------------------------------------------------------------
// L of one sample as the film clamps it: `w` = its weight, `l` = its radiance record (only read for w > 0)
template <typename R>
RRT_DEV Rgb<R> film_sample_radiance(const SceneDev<R>& s, R w, const typename Vec4T<R>::type& l) {
  Rgb<R> L;
  if (w > R(0)) L = Rgb<R>(l.x, l.y, l.z);   // dead samples: L = 0, w = 0 (Q2); their record is never initialised
  // integrator/mod.rs:105-122
  if (L.has_nan()) L = Rgb<R>();
  else if (L.y() < R(-1e-5)) L = Rgb<R>();
  else if (isinf(L.y())) L = Rgb<R>();
  if (L.y() > s.max_sample_luminance) L = L * (s.max_sample_luminance / L.y());
  return L;
}
// One sample of the box filter: `w` = its weight, `l` = its radiance record (only read for w > 0). k_film_box and k_film_box_runs
// both add through this function, so their sums are the same expressions, contracted the same way.
template <typename R>
RRT_DEV void film_box_add(const SceneDev<R>& s, R& cr, R& cg, R& cb, R& wsum, R w, const typename Vec4T<R>::type& l) {
  const Rgb<R> L = film_sample_radiance(s, w, l);
  cr += (L.r * w) * R(1); cg += (L.g * w) * R(1); cb += (L.b * w) * R(1);  // box filter table weight 1
  wsum += R(1);
}

template <typename R>
__global__ void __launch_bounds__(kBlock) k_film_box(SceneDev<R> s, Pools<R> p, PassDesc pd, R* film) {
  const uint32_t pl = blockIdx.x * blockDim.x + threadIdx.x;
  if (pl >= pd.npix) return;
  uint32_t px_, py_;
  pass_pixel(pd, pd.pix_begin + pl, &px_, &py_);
  const uint32_t pix = py_ * (uint32_t)s.xres + px_;
  // The handle's internal film holds the pixel's running contribution sum as RGB + weight (FilmTilePixel film.rs:22-27): the samples of every
  // pool pass are added to it one by one, in sample order, so the sum does not depend on how the samples were cut into passes (a frame and
  // its band partition agree bit for bit also when they need different numbers of passes); k_film_add converts to XYZ once, as
  // merge_film_tile does (film.rs:248-263).
  R* px = film + 4 * (size_t)pix;
  R cr = px[0], cg = px[1], cb = px[2], wsum = px[3];
  constexpr uint32_t kBatch = 8;   // independent loads in flight per thread: a band of a frame has too few pixels to hide the latency otherwise
  auto add = [&](R w, const typename Vec4T<R>::type& l) { film_box_add(s, cr, cg, cb, wsum, w, l); };
  uint32_t sl = 0;
  // few pixels (a band of a frame): latency-bound, batch the loads; many pixels: bandwidth-bound, and seven samples in ten are
  // dead on the 100k-triangle config, so their L records are better left unread
  if (pd.npix < (1u << 18))
  for (; sl + kBatch <= pd.ns; sl += kBatch) {   // samples are added in sample order, as the tile loop does
    R wb[kBatch];
    typename Vec4T<R>::type lb[kBatch];
#pragma unroll
    for (uint32_t k = 0; k < kBatch; k++) { wb[k] = p.weight[(sl + k) * pd.npix + pl]; lb[k] = p.L[(sl + k) * pd.npix + pl]; }
#pragma unroll
    for (uint32_t k = 0; k < kBatch; k++) add(wb[k], lb[k]);
  }
  for (; sl < pd.ns; sl++) {
    const R w = p.weight[sl * pd.npix + pl];
    typename Vec4T<R>::type l = mk4<R>(R(0), R(0), R(0), R(0));
    if (w > R(0)) l = p.L[sl * pd.npix + pl];
    add(w, l);
  }
  px[0] = cr; px[1] = cg; px[2] = cb; px[3] = wsum;
}

// Filters wider than one pixel (TriangleFilter / GaussianFilter / wide BoxFilter, film.rs:77-130 with the 16x16
// table): a sample at p_film touches pixels [ceil(p - 0.5 - r), trunc(p - 0.5 + r)] in x and y. Gather form: one
// thread owns a film pixel and visits the samples of every pixel of this pass within reach, applying exactly the
// reference's footprint test and table lookup - deterministic, no atomics, and contributions that cross a rect /
// band / rank border simply land in that pixel of this handle's film (the multi-GPU reduce is a sum).
RRT_DEV bool pass_pixel_inverse(const PassDesc& pd, int x, int y, uint32_t* pl) {
  if (x < pd.rx0 || x >= pd.rx0 + pd.rw || y < pd.ry0) return false;
  const uint32_t yy = (uint32_t)(y - pd.ry0), band = yy / pd.band_h;
  if (band % pd.n_ranks != pd.rank) return false;
  const uint32_t row = (band / pd.n_ranks) * pd.band_h + yy % pd.band_h, col = (uint32_t)(x - pd.rx0);
  uint64_t lin = (uint64_t)row * (uint32_t)pd.rw + col;
  if (pd.tiled) lin = ((uint64_t)(row / kTileH) * ((uint32_t)pd.rw / kTileW) + col / kTileW) * (kTileW * kTileH) + (row % kTileH) * kTileW + col % kTileW;
  if (lin < pd.pix_begin || lin >= (uint64_t)pd.pix_begin + pd.npix) return false;
  *pl = (uint32_t)(lin - pd.pix_begin);
  return true;
}
// One sample of a wide filter at film pixel (x, y): FilmTile::add_sample's footprint test and table look-up (film.rs:77-130). False = the pixel is
// outside the sample's footprint. k_film_wide and k_gather_wide both weigh through this function, so their weights are the same expressions.
template <typename R>
RRT_DEV bool film_wide_weight(const SceneDev<R>& s, R pfx, R pfy, int x, int y, R* fw) {
  const R dx = pfx - R(0.5), dy = pfy - R(0.5);
  // p0 = ceil(d - r), p1 = trunc(d + r) + 1 (Point2i::from truncates), clipped to the film by the tile bounds
  const R p0x = ceil(dx - s.filter_rx), p0y = ceil(dy - s.filter_ry);
  const R p1x = trunc(dx + s.filter_rx) + R(1), p1y = trunc(dy + s.filter_ry) + R(1);
  if ((R)x < p0x || (R)x >= p1x || (R)y < p0y || (R)y >= p1y) return false;
  const R fy = rabs(((R)y - dy) * s.filter_inv_ry * R(16)), fx = rabs(((R)x - dx) * s.filter_inv_rx * R(16));
  const int ify = (int)rmin(floor(fy), R(15)), ifx = (int)rmin(floor(fx), R(15));
  *fw = s.filter_table[ify * 16 + ifx];
  return true;
}
template <typename R>
__global__ void __launch_bounds__(kBlock) k_film_wide(SceneDev<R> s, Pools<R> p, PassDesc pd, R* film, FilmWindow win) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (uint32_t)win.ew * (uint32_t)win.eh) return;
  const int x = win.ex0 + (int)(t % (uint32_t)win.ew), y = win.ey0 + (int)(t / (uint32_t)win.ew);
  R* px = film + 4 * ((size_t)y * (size_t)s.xres + (size_t)x);
  R cr = px[0], cg = px[1], cb = px[2], wsum = px[3];   // running RGB + weight sums (see k_film_box)
  for (int sy = y - win.reach_y; sy <= y + win.reach_y; sy++) {
    if (sy < 0 || sy >= win.ymax) continue;
    for (int sx = x - win.reach_x; sx <= x + win.reach_x; sx++) {
      uint32_t pl;
      if (sx < 0 || sx >= s.xres || !pass_pixel_inverse(pd, sx, sy, &pl)) continue;
      for (uint32_t sl = 0; sl < pd.ns; sl++) {
        const uint32_t slot = sl * pd.npix + pl;
        const typename Vec4T<R>::type cs = p.samp[slot];
        R fw;
        if (!film_wide_weight(s, cs.x, cs.y, x, y, &fw)) continue;
        const R w = p.weight[slot];
        Rgb<R> L;
        if (w > R(0)) { const typename Vec4T<R>::type l = p.L[slot]; L = Rgb<R>(l.x, l.y, l.z); }
        if (L.has_nan()) L = Rgb<R>();
        else if (L.y() < R(-1e-5)) L = Rgb<R>();
        else if (isinf(L.y())) L = Rgb<R>();
        if (L.y() > s.max_sample_luminance) L = L * (s.max_sample_luminance / L.y());
        cr += (L.r * w) * fw; cg += (L.g * w) * fw; cb += (L.b * w) * fw;
        wsum += fw;
      }
    }
  }
  px[0] = cr; px[1] = cg; px[2] = cb; px[3] = wsum;
}

// ------------------------------------------------------------------------------------------------------------
// The gather skeletons of the first-hit planes (feature buffers, their frame form, ambient occlusion, ID mattes): k_film_box's and
// k_film_wide's loops over the LIVE samples of a pass, around an accumulator that says what a pixel keeps. The contract ("The
// gather contract"):
//  * box: one thread per pixel of the pass (pass_pixel), its samples in sample order, filter weight 1. wide: one thread per film pixel of
//    the window, the pass pixels within reach row by row (pass_pixel_inverse), each one's samples in sample order, weighed by film_wide_weight.
//    This visiting order is what makes a frame and its parts (rects, bands, pool passes) sum to the same bits;
//  * weight[slot] > 0 is tested BEFORE samp[slot] or any record of the slot is read: a dead sample has neither;
//  * Acc is a trivially copyable kernel argument (pointers and small scalars) with a per-thread Pixel: load(s, pix) reads the pixel's running
//    state, add(px, fw, slot) adds one live sample of weight fw from the slot's records, store(s, pix, px) writes the state back. An
//    accumulator touches its own pixel and its own records only, never the pools, and decides nothing about which samples are visited.
// Not under the skeleton, on purpose: k_film_wide_moments counts dead samples into its weight sums and tests the footprint before the
// weight - another visiting rule - and k_film_box / k_film_wide / k_film_box_runs are what a plain frame launches and stay the code they are.
// ------------------------------------------------------------------------------------------------------------
template <typename R, class Acc>
__global__ void __launch_bounds__(kBlock) k_gather_box(SceneDev<R> s, Pools<R> p, PassDesc pd, Acc acc) {
  const uint32_t pl = blockIdx.x * blockDim.x + threadIdx.x;
  if (pl >= pd.npix) return;
  uint32_t px_, py_;
  pass_pixel(pd, pd.pix_begin + pl, &px_, &py_);
  const size_t pix = (size_t)py_ * (size_t)s.xres + px_;
  typename Acc::Pixel px = acc.load(s, pix);
  for (uint32_t sl = 0; sl < pd.ns; sl++) {
    const uint32_t slot = sl * pd.npix + pl;
    if (!(p.weight[slot] > R(0))) continue;   // dead sample
    acc.add(px, R(1), slot);   // box filter table weight 1
  }
  acc.store(s, pix, px);
}
template <typename R, class Acc>
__global__ void __launch_bounds__(kBlock) k_gather_wide(SceneDev<R> s, Pools<R> p, PassDesc pd, Acc acc, FilmWindow win) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (uint32_t)win.ew * (uint32_t)win.eh) return;
  const int x = win.ex0 + (int)(t % (uint32_t)win.ew), y = win.ey0 + (int)(t / (uint32_t)win.ew);
  const size_t pix = (size_t)y * (size_t)s.xres + (size_t)x;
  typename Acc::Pixel px = acc.load(s, pix);
  for (int sy = y - win.reach_y; sy <= y + win.reach_y; sy++) {
    if (sy < 0 || sy >= win.ymax) continue;
    for (int sx = x - win.reach_x; sx <= x + win.reach_x; sx++) {
      uint32_t pl;
      if (sx < 0 || sx >= s.xres || !pass_pixel_inverse(pd, sx, sy, &pl)) continue;
      for (uint32_t sl = 0; sl < pd.ns; sl++) {
        const uint32_t slot = sl * pd.npix + pl;
        if (!(p.weight[slot] > R(0))) continue;
        const typename Vec4T<R>::type cs = p.samp[slot];
        R fw;
        if (!film_wide_weight(s, cs.x, cs.y, x, y, &fw)) continue;
        acc.add(px, fw, slot);
      }
    }
  }
  acc.store(s, pix, px);
}

// Film::merge_film_tile (film.rs:248-263): the pixel's RGB contribution sum -> XYZ (rgb_to_xyz spectrum.rs:2084-2090), added to the
// caller's film; filter_weight_sum is added three times per merged pixel (Q3). `n` = pixels.
template <typename R>
__global__ void k_film_add(const R* src, R* dst, size_t n) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const R cr = src[4 * i], cg = src[4 * i + 1], cb = src[4 * i + 2], wsum = src[4 * i + 3];
  R* px = dst + 4 * i;
  px[0] += R(0.412453) * cr + R(0.357580) * cg + R(0.180423) * cb;
  px[1] += R(0.212671) * cr + R(0.715160) * cg + R(0.072169) * cb;
  px[2] += R(0.019334) * cr + R(0.119193) * cg + R(0.950227) * cb;
  px[3] += wsum; px[3] += wsum; px[3] += wsum;
}

// rrt_combine_passes: out = sum_k rgb_to_xyz(gain_k * xyz_to_rgb(film_k)) per pixel, the weight channel film_0's. One thread per pixel reads all its inputs
// before it writes, so the output may be one of the inputs. The arithmetic is f64 in both precisions (xyz_to_rgb has coefficients of both signs: in fp32
// its cancellation would cost the digits the gain then scales) - a few dozen flops per pixel beside n 16-byte loads.
// xyz_to_rgb here is CombineArgs::to_rgb, the inverse in f64 of the rgb_to_xyz table a film was merged with (k_film_add), not the six-digit table of
// spectrum.rs:2075-2082: the two tables are inverses of each other only to 1.4e-6, and a relit frame is the frame of the scaled lights only as far as the
// way back to RGB undoes the way there (f64: 5.1e-7 of the frame's largest value with the six-digit table, 1e-15 with the inverse).
constexpr int kMaxPasses = 16;   // RRT_MAX_PASSES
struct CombineArgs {
  const void* films[kMaxPasses];
  double gains[kMaxPasses][3];
  double to_rgb[3][3];
  int n;
};
// the inverse of k_film_add's rgb_to_xyz (spectrum.rs:2084-2090) by cofactors, in f64
inline void combine_to_rgb(double inv[3][3]) {
  const double m[3][3] = {{0.412453, 0.357580, 0.180423}, {0.212671, 0.715160, 0.072169}, {0.019334, 0.119193, 0.950227}};
  const double c00 = m[1][1] * m[2][2] - m[1][2] * m[2][1], c01 = m[1][2] * m[2][0] - m[1][0] * m[2][2], c02 = m[1][0] * m[2][1] - m[1][1] * m[2][0];
  const double det = m[0][0] * c00 + m[0][1] * c01 + m[0][2] * c02;
  inv[0][0] = c00 / det; inv[1][0] = c01 / det; inv[2][0] = c02 / det;
  inv[0][1] = (m[0][2] * m[2][1] - m[0][1] * m[2][2]) / det; inv[1][1] = (m[0][0] * m[2][2] - m[0][2] * m[2][0]) / det; inv[2][1] = (m[0][1] * m[2][0] - m[0][0] * m[2][1]) / det;
  inv[0][2] = (m[0][1] * m[1][2] - m[0][2] * m[1][1]) / det; inv[1][2] = (m[0][2] * m[1][0] - m[0][0] * m[1][2]) / det; inv[2][2] = (m[0][0] * m[1][1] - m[0][1] * m[1][0]) / det;
}
template <typename R>
__global__ void __launch_bounds__(kBlock) k_combine_passes(CombineArgs a, R* out, size_t npix) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= npix) return;
  using V4 = typename Vec4T<R>::type;
  double x = 0.0, y = 0.0, z = 0.0;
  R w0 = R(0);
  for (int k = 0; k < a.n; k++) {
    const V4 f = reinterpret_cast<const V4*>(a.films[k])[i];
    if (k == 0) w0 = f.w;
    const double fx = (double)f.x, fy = (double)f.y, fz = (double)f.z;
    // back to RGB (to_rgb), the gain, rgb_to_xyz spectrum.rs:2084-2090
    const double r = (a.to_rgb[0][0] * fx + a.to_rgb[0][1] * fy + a.to_rgb[0][2] * fz) * a.gains[k][0];
    const double g = (a.to_rgb[1][0] * fx + a.to_rgb[1][1] * fy + a.to_rgb[1][2] * fz) * a.gains[k][1];
    const double b = (a.to_rgb[2][0] * fx + a.to_rgb[2][1] * fy + a.to_rgb[2][2] * fz) * a.gains[k][2];
    x += 0.412453 * r + 0.357580 * g + 0.180423 * b;
    y += 0.212671 * r + 0.715160 * g + 0.072169 * b;
    z += 0.019334 * r + 0.119193 * g + 0.950227 * b;
  }
  reinterpret_cast<V4*>(out)[i] = mk4<R>((R)x, (R)y, (R)z, w0);
}

// ------------------------------------------------------------------------------------------------------------
// First-hit feature buffers (rrt_render_aov, include/rrt.h): albedo, normal and depth of the camera rays' first hits, filtered by the
// film's pixel filter. A pass of their own - camera kernels, closest-hit launch, k_aov_shade, the gather over AovAcc - not a branch of
// k_shade_path: the frame's kernels and their register budgets stay what they are.
// ------------------------------------------------------------------------------------------------------------
// rho of the table in rrt.h from the material's own parameters; a textured one is evaluated through `c` (zero differentials)
template <typename R, bool TEX>
RRT_DEV Rgb<R> aov_rho(const SceneDev<R>& s, const Material<R>& m, TexCtx<R>& c) {
  auto par = [&](int slot, const R* k) -> Rgb<R> {
    if (TEX) { if (m.tex[slot] >= 0) return TexEval<R, kTexDepth>::eval(s, m.tex[slot], c); }
    return Rgb<R>(k);
  };
  switch (m.type) {
    case 0: case 1: case 6: return rgb_clamp0(par(0, m.kd));   // Matte, Plastic, Translucent: Kd
    case 3: return rgb_clamp0(par(2, m.kr));                   // Mirror: Kr
    case 5: return Rgb<R>(R(1));                               // Glass
    case 2: {                                                  // Metal: the conductor's reflectance at normal incidence
      const Rgb<R> eta = par(3, m.eta), k = par(4, m.k), one(R(1));
      return ((eta - one) * (eta - one) + k * k) / ((eta + one) * (eta + one) + k * k);
    }
    default: return Rgb<R>(R(0), R(1), R(1));                  // Debug: the sum of its two lobes
  }
}

// One thread per entry of the camera queue, in queue order (slot word, ray, hit record: 128-bit loads). Two 16-byte records per slot:
// rec_a = {rho.rgb, hit flag}, rec_b = {n.xyz, t}. Every live sample of the pass is in the queue (the camera kernels ran without the root
// cull), so rec_a - the flag - is written for every live slot, hit or miss; rec_b only for hits. Slots that never reach the queue (dead
// samples) get no record: the film kernels read records of slots with weight > 0 only.
template <typename R, bool TEX>
__global__ void __launch_bounds__(kBlock) k_aov_shade(SceneDev<R> s, Pools<R> p, typename Vec4T<R>::type* rec_a, typename Vec4T<R>::type* rec_b) {
  using V4 = typename Vec4T<R>::type;
  const uint32_t n = p.counters[C_ACTIVE];
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    const uint32_t slot = p.q_active[i].slot;
    const V4 h = p.hit[i];
    const int prim = (int)real_to_bits(h.y);
    if (prim < 0) { rec_a[slot] = mk4u<R>(R(0), R(0), R(0), 0u); continue; }
    const V4 ro = p.ray_o[i], rd = p.ray_d[i];
    SurfExt<R> ext;
    const Surf<R> si = build_surface(s, prim, V3<R>(ro.x, ro.y, ro.z), V3<R>(rd.x, rd.y, rd.z), h.x, h.z, h.w, TEX ? &ext : nullptr);
    if (!si.ok) atomicOr(&p.counters[C_ERROR], (uint32_t)ERR_SHADING_NORMAL);   // primitives.rs:66, as the frame reports it
    TexCtx<R> tc;
    if (TEX) {   // dpdx = dpdy = 0, dudx .. dvdy = 0 (TexCtx's defaults)
      tc.p = si.p; tc.u = ext.u; tc.v = ext.v;
      tc.pd = V3<double>((double)si.p.x + (double)si.p_lo.x, (double)si.p.y + (double)si.p_lo.y, (double)si.p.z + (double)si.p_lo.z);
    }
    const Rgb<R> rho = aov_rho<R, TEX>(s, s.materials[si.material], tc);
    if (TEX) { if (tc.err) atomicOr(&p.counters[C_ERROR], (uint32_t)ERR_MIPMAP); }
    const V3<R> nn = vnormalize(si.n);
    rec_a[slot] = mk4u<R>(rho.r, rho.g, rho.b, 1u);
    rec_b[slot] = mk4<R>(nn.x, nn.y, nn.z, h.x);
  }
}

// One live sample with filter weight fw into the three running sums of a pixel (rrt_aov in rrt.h): what AovAcc and AovFrameAcc
// add through, under both gather skeletons.
template <typename R>
struct AovPixel { typename Vec4T<R>::type alb, nrm, dep; };
template <typename R>
RRT_DEV void aov_add(AovPixel<R>& px, R fw, const typename Vec4T<R>::type& a, const typename Vec4T<R>::type* rec_b, uint32_t slot) {
  px.alb.w += fw;
  if (real_to_bits(a.w) == 0u) return;   // a live sample that misses the scene
  const typename Vec4T<R>::type b = rec_b[slot];
  px.alb.x += fw * a.x; px.alb.y += fw * a.y; px.alb.z += fw * a.z;
  px.nrm.x += fw * b.x; px.nrm.y += fw * b.y; px.nrm.z += fw * b.z; px.nrm.w += fw;
  px.dep.x += fw * b.w; px.dep.y += (fw * b.w) * b.w; px.dep.z += fw;
}
template <typename R>
RRT_DEV AovPixel<R> aov_load(const R* planes, size_t plane_n, size_t pix) {
  using V4 = typename Vec4T<R>::type;
  AovPixel<R> px;
  px.alb = reinterpret_cast<const V4*>(planes)[pix];
  px.nrm = reinterpret_cast<const V4*>(planes + plane_n)[pix];
  px.dep = reinterpret_cast<const V4*>(planes + 2 * plane_n)[pix];
  return px;
}
template <typename R>
RRT_DEV void aov_store(R* planes, size_t plane_n, size_t pix, const AovPixel<R>& px) {
  using V4 = typename Vec4T<R>::type;
  reinterpret_cast<V4*>(planes)[pix] = px.alb;
  reinterpret_cast<V4*>(planes + plane_n)[pix] = px.nrm;
  reinterpret_cast<V4*>(planes + 2 * plane_n)[pix] = px.dep;
}

// The feature buffers under the gather skeletons (k_gather_box / k_gather_wide): running sums in the handle's three internal W x H x 4 planes
// (`planes`, one after the other), the records k_aov_shade / k_aov_follow left per slot.
template <typename R>
struct AovAcc {
  using V4 = typename Vec4T<R>::type;
  using Pixel = AovPixel<R>;
  R* planes;
  const V4 *rec_a, *rec_b;
  RRT_DEV static size_t plane_n(const SceneDev<R>& s) { return 4 * (size_t)s.xres * (size_t)s.yres; }
  RRT_DEV Pixel load(const SceneDev<R>& s, size_t pix) const { return aov_load(planes, plane_n(s), pix); }
  RRT_DEV void add(Pixel& px, R fw, uint32_t slot) const { aov_add(px, fw, rec_a[slot], rec_b, slot); }
  RRT_DEV void store(const SceneDev<R>& s, size_t pix, const Pixel& px) const { aov_store(planes, plane_n(s), pix, px); }
};

// the caller's plane += the internal one (`n` = W x H x 4 values)
template <typename R>
__global__ void k_aov_merge(const R* src, R* dst, size_t n) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) dst[i] += src[i];
}

// ------------------------------------------------------------------------------------------------------------
// Ambient occlusion and bent normals (rrt_render_ao, include/rrt.h): AOIntegrator::li (ao.rs:65-96) over the first hits of the camera queue.
// ------------------------------------------------------------------------------------------------------------
// uniform_sample_hemisphere sampling.rs:245-256
template <typename R> RRT_DEV V3<R> uniform_sample_hemisphere(R u0, R u1) {
  const R z = u0;
  const R r = sqrt(rmax(R(0), R(1) - z * z));
  const R phi = R(2) * R(RRT_PI) * u1;
  return {r * R(cos(phi)), r * R(sin(phi)), z};
}

// The interaction's GEOMETRIC dpdu after the instance transform. Surf::sdpdu is that vector on spheres and on triangles without vertex normals;
// a triangle with them carries the shading frame's there (triangle.rs:330-349), so its dpdu is formed again, by build_surface's own expressions.
// (Not an output of build_surface: a SurfExt asked for here lives in scratch, and one more optional argument moved the register allocation of
// an existing kernel.)
template <typename R>
RRT_DEV V3<R> ao_dpdu(const SceneDev<R>& s, int prim, const Surf<R>& si) {
  const Tri<R> tr = s.tris[prim];
  if (tr.plane == kSphereMark || tr.shade == 0xffffffffu) return si.sdpdu;
  const TriShade<R>& sh = s.shades[tr.shade];
  if (sh.has_n != 1) return si.sdpdu;
  const V3<R> p0(tr.p0), p1(tr.p1), p2(tr.p2);
  R uv[3][2] = {{R(0), R(0)}, {R(1), R(0)}, {R(1), R(1)}};  // get_uvs :113-128
  if (sh.has_uv) for (int k = 0; k < 3; k++) { uv[k][0] = sh.uv[k][0]; uv[k][1] = sh.uv[k][1]; }
  const R duv02[2] = {uv[0][0] - uv[2][0], uv[0][1] - uv[2][1]}, duv12[2] = {uv[1][0] - uv[2][0], uv[1][1] - uv[2][1]};
  const V3<R> dp02 = p0 - p2, dp12 = p1 - p2;
  const R determinant = duv02[0] * duv12[1] - duv02[1] * duv12[0];
  const bool degenerate_uv = rabs(determinant) < R(1e-8);
  V3<R> dpdu, dpdv;
  if (!degenerate_uv) {
    const R i_det = R(1) / determinant;
    dpdu = (dp02 * duv12[1] - dp12 * duv02[1]) * i_det;
    dpdv = (dp02 * -duv12[0] + dp12 * duv02[0]) * i_det;
  }
  if (degenerate_uv || len2(cross(dpdu, dpdv)) == R(0)) coordinate_system(vnormalize(cross(p2 - p0, p1 - p0)), &dpdu, &dpdv);
  if (is_inst_tri(tr)) {
    const InstDev<R>& I = s.insts[inst_of(tr)];
    if (!I.identity) dpdu = aff_vec(I.m, dpdu);
  }
  return dpdu;
}

// Draw `draw` of every hit of the camera queue: one thread per queue entry, in queue order (slot word, ray and hit record: 128-bit loads), the
// surface rebuilt as k_aov_shade rebuilds it, the frame of ao.rs:74-76 on the GEOMETRIC dpdu, one hemisphere direction from the sample's own
// stream (the draw's 2D value: Halton dimensions 5 + 2 draw, 6 + 2 draw), and the ray pushed into the pool's shadow queue with its record
// {a_i * d_i, slot} - one atomic per block. Misses push nothing; a draw with pdf == 0 (cosine mode, z = 0: ao.rs forms 0 / 0 there) is dropped.
// p.L points at the call's per-slot accumulators {b.xyz, a}: the first draw starts them (hit: 0, miss: a = -1, the gather kernels' flag).
template <typename R>
__global__ void __launch_bounds__(kBlock) k_ao_gen(SceneDev<R> s, Pools<R> p, uint32_t draw, uint32_t n_draws, int cos_sample) {
  __shared__ uint32_t push_lds[kBlock / 64 + 1];
  using V4 = typename Vec4T<R>::type;
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t n = p.counters[C_ACTIVE];
  if (blockIdx.x * blockDim.x >= n) return;   // whole block past the queue end (the grid is sized for the worst case)
  bool want = false;
  uint32_t slot = 0;
  int prim = -1;
  V3<R> sh_o, sh_d, o_lo, rec;
  if (i < n) {
    const QEnt qe = p.q_active[i];
    slot = qe.slot;
    const V4 h = p.hit[i];
    prim = (int)real_to_bits(h.y);
    if (draw == 0u) p.L[slot] = mk4<R>(R(0), R(0), R(0), prim >= 0 ? R(0) : R(-1));
    if (prim >= 0) {
      const V4 ro = p.ray_o[i], rd = p.ray_d[i];
      const V3<R> d(rd.x, rd.y, rd.z);
      const Surf<R> si = build_surface(s, prim, V3<R>(ro.x, ro.y, ro.z), d, h.x, h.z, h.w);
      if (!si.ok) atomicOr(&p.counters[C_ERROR], (uint32_t)ERR_SHADING_NORMAL);   // primitives.rs:66, as the frame reports it
      const V3<R> nf = faceforward(si.n, -d);
      const V3<R> ss = vnormalize(ao_dpdu(s, prim, si));
      const V3<R> ts = cross(si.n, ss);   // the un-flipped normal, as ao.rs:76 has it
      const R u0 = to_real<R>(halton_dim(s, qe.index, 5u + 2u * draw)), u1 = to_real<R>(halton_dim(s, qe.index, 6u + 2u * draw));
      V3<R> wl;
      R pdf;
      if (cos_sample) { wl = cosine_sample_hemisphere(u0, u1); pdf = rabs(wl.z) * R(0.31830988618379067154); }
      else { wl = uniform_sample_hemisphere(u0, u1); pdf = R(1) / (R(2) * R(RRT_PI)); }
      const V3<R> wi((ss.x * wl.x + ts.x * wl.y) + nf.x * wl.z, (ss.y * wl.x + ts.y * wl.y) + nf.y * wl.z, (ss.z * wl.x + ts.z * wl.y) + nf.z * wl.z);
      if (pdf != R(0)) {
        const R a = dot(wi, nf) / (pdf * (R)n_draws);
        sh_d = vnormalize(wi);   // spawn_ray -> Ray::new_od (Q8: no origin offset)
        sh_o = si.p; o_lo = si.p_lo;
        rec = sh_d * a;
        want = true;
      }
    }
  }
  const uint32_t qs = block_push(p.shadow_count, want, push_lds);
  if (want) {
    store_ray<R>(p.sray_o, p.sray_d, qs, sh_o, o_lo, sh_d, Const<R>::inf, self_prim<R>(prim));
    p.sld[qs] = mk4u<R>(rec.x, rec.y, rec.z, slot);
  }
}

// One live sample with filter weight fw into the two running sums of a pixel (rrt_ao in rrt.h); acc = the slot's accumulator {b.xyz, a}, a < 0 = miss
template <typename R>
struct AoPixel { typename Vec4T<R>::type ao, bent; };
template <typename R>
RRT_DEV void ao_add(AoPixel<R>& px, R fw, const typename Vec4T<R>::type& acc) {
  px.ao.w += fw;
  if (acc.w < R(0)) return;   // a live sample that misses the scene
  px.ao.x += fw * acc.w; px.ao.y += (fw * acc.w) * acc.w; px.ao.z += fw;
  px.bent.x += fw * acc.x; px.bent.y += fw * acc.y; px.bent.z += fw * acc.z; px.bent.w += fw;
}

// Under the gather skeletons: running sums in the handle's two internal W x H x 4 planes (`planes`, one after the other), `acc` = the slots' accumulators
template <typename R>
struct AoAcc {
  using V4 = typename Vec4T<R>::type;
  using Pixel = AoPixel<R>;
  R* planes;
  const V4* acc;
  RRT_DEV static size_t plane_n(const SceneDev<R>& s) { return 4 * (size_t)s.xres * (size_t)s.yres; }
  RRT_DEV Pixel load(const SceneDev<R>& s, size_t pix) const {
    return Pixel{reinterpret_cast<const V4*>(planes)[pix], reinterpret_cast<const V4*>(planes + plane_n(s))[pix]};
  }
  RRT_DEV void add(Pixel& px, R fw, uint32_t slot) const { ao_add(px, fw, acc[slot]); }
  RRT_DEV void store(const SceneDev<R>& s, size_t pix, const Pixel& px) const {
    reinterpret_cast<V4*>(planes)[pix] = px.ao;
    reinterpret_cast<V4*>(planes + plane_n(s))[pix] = px.bent;
  }
};

// ------------------------------------------------------------------------------------------------------------
// Frame forms of k_aov_shade and AovAcc (rrt_render_frame_aov, include/rrt.h): the feature buffers from the frame's own bounce-0 queue.
// A frame's camera kernels run with the root cull: a live camera ray that misses the root box has weight[slot] > 0 and never enters the
// queue, so "every live sample is in the queue" does not hold and nothing writes its rec_a - the slot keeps what an earlier pass left.
// Such a sample is a miss. The shading kernel therefore stamps rec_a.w with {serial of the pass << 1 | hit bit}; the serial is non-zero and
// used by no earlier pass that wrote into the handle's record buffers (the host counts it up, and the buffers are zeroed when allocated;
// k_aov_shade's own flag words 0 and 1 carry serial 0), and the gather reads every other stamp as a miss. The shading kernel is one of
// its own, not a template flag on k_aov_shade: the code rrt_render_aov launches stays what it is. The gather is the skeletons' own loops around
// AovFrameAcc, which differs from AovAcc in the rec_a read alone, so the arithmetic per sample is the same expressions, in the same order.
// ------------------------------------------------------------------------------------------------------------
// rec_a as the gather of the frame form takes it: the record of this pass's own stamp, a miss otherwise
template <typename R>
RRT_DEV typename Vec4T<R>::type aov_frame_rec(const typename Vec4T<R>::type* rec_a, uint32_t slot, uint32_t serial) {
  typename Vec4T<R>::type a = rec_a[slot];
  const uint32_t stamp = real_to_bits(a.w);
  // aov_add's flag word: the hit bit of this pass's own record; any other stamp = unwritten in this pass: root-culled, provably a miss
  a.w = bits_to_real((stamp >> 1) == serial ? (stamp & 1u) : 0u, R(0));
  return a;
}

// k_aov_shade over the queue the frame's first closest-hit launch of a pass leaves. slot_end: the slots of the leading samples that the
// feature buffers take (slot = sl * npix + pl, so a prefix of the samples is a prefix of the slots); entries beyond it are skipped.
template <typename R, bool TEX>
__global__ void __launch_bounds__(kBlock) k_aov_shade_frame(SceneDev<R> s, Pools<R> p, typename Vec4T<R>::type* rec_a, typename Vec4T<R>::type* rec_b, uint32_t serial, uint32_t slot_end) {
  using V4 = typename Vec4T<R>::type;
  const uint32_t n = p.counters[C_ACTIVE];
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    const uint32_t slot = p.q_active[i].slot;
    if (slot >= slot_end) continue;
    const V4 h = p.hit[i];
    const int prim = (int)real_to_bits(h.y);
    if (prim < 0) { rec_a[slot] = mk4u<R>(R(0), R(0), R(0), serial << 1); continue; }
    const V4 ro = p.ray_o[i], rd = p.ray_d[i];
    SurfExt<R> ext;
    const Surf<R> si = build_surface(s, prim, V3<R>(ro.x, ro.y, ro.z), V3<R>(rd.x, rd.y, rd.z), h.x, h.z, h.w, TEX ? &ext : nullptr);
    if (!si.ok) atomicOr(&p.counters[C_ERROR], (uint32_t)ERR_SHADING_NORMAL);   // primitives.rs:66, as the frame reports it
    TexCtx<R> tc;
    if (TEX) {   // dpdx = dpdy = 0, dudx .. dvdy = 0 (TexCtx's defaults)
      tc.p = si.p; tc.u = ext.u; tc.v = ext.v;
      tc.pd = V3<double>((double)si.p.x + (double)si.p_lo.x, (double)si.p.y + (double)si.p_lo.y, (double)si.p.z + (double)si.p_lo.z);
    }
    const Rgb<R> rho = aov_rho<R, TEX>(s, s.materials[si.material], tc);
    if (TEX) { if (tc.err) atomicOr(&p.counters[C_ERROR], (uint32_t)ERR_MIPMAP); }
    const V3<R> nn = vnormalize(si.n);
    rec_a[slot] = mk4u<R>(rho.r, rho.g, rho.b, (serial << 1) | 1u);
    rec_b[slot] = mk4<R>(nn.x, nn.y, nn.z, h.x);
  }
}

// AovAcc over the leading pd.ns samples of a frame's pass (the host cuts pd.ns to the feature buffers' prefix): rec_a read through the pass's stamp
template <typename R>
struct AovFrameAcc : AovAcc<R> {
  uint32_t serial;
  RRT_DEV void add(typename AovAcc<R>::Pixel& px, R fw, uint32_t slot) const { aov_add(px, fw, aov_frame_rec<R>(this->rec_a, slot, serial), this->rec_b, slot); }
};

// ------------------------------------------------------------------------------------------------------------
// Feature buffers through mirrors and glass (rrt_render_aov_follow, include/rrt.h): the record of the first non-specular surface along
// the chain of perfectly specular bounces a camera ray starts. A kernel of its own, not a template flag on k_aov_shade: the code
// rrt_render_aov and rrt_render_frame_aov launch stays what it is. The first hits' records are k_aov_shade's own, rho goes through aov_rho and
// the planes through the gather over AovAcc unchanged, so a chain of length 0 leaves rrt_render_aov's bits.
// ------------------------------------------------------------------------------------------------------------
// The continuation of the chain at a hit, by the rules on the prototype: Mirror reflects about the shading normal; smooth Glass refracts
// (reflection.rs:122-134, wo = -d, the normal turned towards wo) and reflects where there is no refracted direction or Kt is black. `m` has
// its textured parameters evaluated at the hit, `kr` = its Kr clamped to >= 0. false: the chain ends on this surface.
template <typename R>
RRT_DEV bool aov_follow_dir(const Material<R>& m, Rgb<R> kr, V3<R> d, V3<R> sn, V3<R>* d_next, Rgb<R>* tint) {
  if (m.type != 3 && m.type != 5) return false;
  if (m.type == 5) {
    if (!(m.u_roughness == R(0) && m.v_roughness == R(0))) return false;   // rough glass (glass.rs:74, before any remap)
    const Rgb<R> kt = rgb_clamp0(Rgb<R>(m.kt));
    const V3<R> wo = -d;
    const bool entering = dot(wo, sn) > R(0);
    V3<R> wt;
    if (!kt.is_black() && refract(wo, faceforward(sn, wo), entering ? R(1) / m.index : m.index, &wt)) {
      *d_next = vnormalize(wt); *tint = kt;
      return true;
    }
  }
  if (kr.is_black()) return false;
  *d_next = vnormalize(d - sn * (R(2) * dot(d, sn)));
  *tint = kr;
  return true;
}

// The chain's own record arithmetic, never contracted: the TEX and non-TEX instantiations form the same bits
template <typename R>
RRT_DEV typename Vec4T<R>::type aov_follow_scale(const typename Vec4T<R>::type& st, Rgb<R> c, R t) {
#pragma clang fp contract(off)
  return mk4<R>(st.x * c.r, st.y * c.g, st.z * c.b, st.w + t);
}
// the material build_surface reports for a hit on `prim`
template <typename R>
RRT_DEV uint32_t aov_hit_material(const SceneDev<R>& s, int prim) {
  const Tri<R>& tr = s.tris[prim];
  return (tr.plane != kSphereMark && is_inst_tri(tr)) ? (tr.material & 0xffffu) : tr.material;
}

// One level of the chain: one thread per entry of the active queue, in queue order (slot word, ray, hit and the entry's {thr.rgb, T}
// record in p.path - the role npath plays for beta: 128-bit loads). A hit writes the slot's record {thr * rho, hit flag}, {n, T + t}, so the
// record of the last surface hit is always in place: a later miss, or a chain that has used up its levels, needs no fix-up.
// level0: the queue is the camera kernels' and k_aov_shade ITSELF has just written its records (rec_a for every entry, hit or miss - a record
// an earlier pass left in a slot is never read): with thr = 1 and T = 0 they are the chain's, and only k_aov_shade's own code leaves
// k_aov_shade's bits - a second copy of its statements inside this kernel is contracted differently by the compiler (the normal plane of a
// chain of length 0 then differs from rrt_render_aov's in its last bit: measured). So level 0 here only decides and spawns, for the hits on
// Mirror / Glass. may_follow: followed entries go to q_next through block_push with their ray (store_ray: the self-triangle exclusion and the
// low word of the origin) and {thr * tint, T + t}. The grid walks the queue with block-uniform trip counts, as block_push needs.
template <typename R, bool TEX>
__global__ void __launch_bounds__(kBlock) k_aov_follow(SceneDev<R> s, Pools<R> p, typename Vec4T<R>::type* rec_a, typename Vec4T<R>::type* rec_b, int level0, int may_follow) {
  using V4 = typename Vec4T<R>::type;
  __shared__ uint32_t push_lds[kBlock / 64 + 1];
  const uint32_t n = p.counters[C_ACTIVE];
  for (uint32_t base = blockIdx.x * blockDim.x; base < n; base += gridDim.x * blockDim.x) {
    const uint32_t i = base + threadIdx.x;
    bool want_next = false;
    uint32_t slot = 0;
    int prim = -1;
    V3<R> nx_o, nx_lo, nx_d;
    V4 nx_rec = mk4<R>(R(0), R(0), R(0), R(0));
    if (i < n) {
      slot = p.q_active[i].slot;
      const V4 h = p.hit[i];
      prim = (int)real_to_bits(h.y);
      bool work = prim >= 0;
      if (work && level0) { const int mt = s.materials[aov_hit_material(s, prim)].type; work = mt == 3 || mt == 5; }
      if (work) {
        const V4 ro = p.ray_o[i], rd = p.ray_d[i];
        const V3<R> d(rd.x, rd.y, rd.z);
        SurfExt<R> ext;
        const Surf<R> si = build_surface(s, prim, V3<R>(ro.x, ro.y, ro.z), d, h.x, h.z, h.w, TEX ? &ext : nullptr);
        if (!si.ok) atomicOr(&p.counters[C_ERROR], (uint32_t)ERR_SHADING_NORMAL);   // primitives.rs:66, as the frame reports it
        TexCtx<R> tc;
        if (TEX) {   // dpdx = dpdy = 0, dudx .. dvdy = 0 (TexCtx's defaults)
          tc.p = si.p; tc.u = ext.u; tc.v = ext.v;
          tc.pd = V3<double>((double)si.p.x + (double)si.p_lo.x, (double)si.p.y + (double)si.p_lo.y, (double)si.p.z + (double)si.p_lo.z);
        }
        const Material<R>& m0 = s.materials[si.material];
        const Rgb<R> rho = aov_rho<R, TEX>(s, m0, tc);
        const V4 st = level0 ? mk4<R>(R(1), R(1), R(1), R(0)) : p.path[i];
        if (!level0) {
          const V3<R> nn = vnormalize(si.n);
          const V4 rec = aov_follow_scale<R>(st, rho, h.x);   // {thr * rho, T + t}
          rec_a[slot] = mk4u<R>(rec.x, rec.y, rec.z, 1u);
          rec_b[slot] = mk4<R>(nn.x, nn.y, nn.z, rec.w);
        }
        if (may_follow && (m0.type == 3 || m0.type == 5)) {
          Rgb<R> tint;
          if (m0.type == 3) want_next = aov_follow_dir(m0, rho, d, si.sn, &nx_d, &tint);   // a Mirror's rho is its clamped Kr at this hit: not evaluated twice
          else if (TEX) {
            const Material<R> m = resolve_material(s, m0, tc);
            want_next = aov_follow_dir(m, rgb_clamp0(Rgb<R>(m.kr)), d, si.sn, &nx_d, &tint);
          }
          else want_next = aov_follow_dir(m0, rgb_clamp0(Rgb<R>(m0.kr)), d, si.sn, &nx_d, &tint);
          if (want_next) {
            nx_o = si.p; nx_lo = si.p_lo;   // spawn_ray applies no offset (Q8)
            nx_rec = aov_follow_scale<R>(st, tint, h.x);   // {thr * tint, T + t}
          }
        }
        if (TEX) { if (tc.err) atomicOr(&p.counters[C_ERROR], (uint32_t)ERR_MIPMAP); }
      }
    }
    const uint32_t qn = block_push(&p.counters[C_NEXT], want_next, push_lds);
    if (want_next) {
      p.q_next[qn] = QEnt{slot, 0u, 0u, 0u};
      p.npath[qn] = nx_rec;
      store_ray<R>(p.nray_o, p.nray_d, qn, nx_o, nx_lo, nx_d, Const<R>::inf, self_prim<R>(prim));
    }
  }
}

// ------------------------------------------------------------------------------------------------------------
// Sample-variance plane beside the film (rrt_render_moments, include/rrt.h): per film pixel {S1 = sum fw y, S2 = sum fw y^2, S0 = sum fw,
// S3 = sum fw^2} over every sample whose footprint covers the pixel, y = the luminance of L w after the film's own clamps. Kernels of their
// own, not a template flag on k_film_box / k_film_wide: the kernels a plain frame launches stay the code they are. The film sums go through
// film_box_add and, for the wide filter, k_film_wide's three accumulation statements after film_sample_radiance. k_film_wide itself keeps its own
// inline copy of those clamp statements on purpose: re-emitting it around the shared function is a risk to the code plain frames launch, and
// tests/test_moments.py::test_film_is_the_plain_frames is what holds the two copies to the same film bits.
// ------------------------------------------------------------------------------------------------------------

// k_film_box with two more running sums per pixel: the same passes, the same sequential sample order in both of its paths, so neither the film
// nor the moments depend on how the frame was cut into passes. S0 = S3 = the sample count, which the film's weight sum already is.
// LISTED: a listed pass (list_pixel over `list`, rrt_render_adaptive) instead of a rect's pixel group (pass_pixel; `list` is not read) - the
// pixel decode is all that differs, so a pixel that a listed pass continues holds what a longer rect pass would have left in it.
template <typename R, bool LISTED>
__global__ void __launch_bounds__(kBlock) k_film_box_moments(SceneDev<R> s, Pools<R> p, PassDesc pd, const uint32_t* list, R* film, R* mom) {
  const uint32_t pl = blockIdx.x * blockDim.x + threadIdx.x;
  if (pl >= pd.npix) return;
  uint32_t px_, py_;
  if constexpr (LISTED) list_pixel(pd, list, pd.pix_begin + pl, &px_, &py_);
  else pass_pixel(pd, pd.pix_begin + pl, &px_, &py_);
  const uint32_t pix = py_ * (uint32_t)s.xres + px_;
  R* px = film + 4 * (size_t)pix;
  R* pm = mom + 4 * (size_t)pix;
  R cr = px[0], cg = px[1], cb = px[2], wsum = px[3];
  R s1 = pm[0], s2 = pm[1];
  constexpr uint32_t kBatch = 8;
  auto add = [&](R w, const typename Vec4T<R>::type& l) {
    film_box_add(s, cr, cg, cb, wsum, w, l);
    const R y = film_sample_radiance(s, w, l).y() * w;
    s1 += y; s2 += y * y;
  };
  uint32_t sl = 0;
  if (pd.npix < (1u << 18))
  for (; sl + kBatch <= pd.ns; sl += kBatch) {
    R wb[kBatch];
    typename Vec4T<R>::type lb[kBatch];
#pragma unroll
    for (uint32_t k = 0; k < kBatch; k++) { wb[k] = p.weight[(sl + k) * pd.npix + pl]; lb[k] = p.L[(sl + k) * pd.npix + pl]; }
#pragma unroll
    for (uint32_t k = 0; k < kBatch; k++) add(wb[k], lb[k]);
  }
  for (; sl < pd.ns; sl++) {
    const R w = p.weight[sl * pd.npix + pl];
    typename Vec4T<R>::type l = mk4<R>(R(0), R(0), R(0), R(0));
    if (w > R(0)) l = p.L[sl * pd.npix + pl];
    add(w, l);
  }
  px[0] = cr; px[1] = cg; px[2] = cb; px[3] = wsum;
  pm[0] = s1; pm[1] = s2; pm[2] = wsum; pm[3] = wsum;
}

// k_film_wide with the four running sums of the pixel
template <typename R>
__global__ void __launch_bounds__(kBlock) k_film_wide_moments(SceneDev<R> s, Pools<R> p, PassDesc pd, R* film, R* mom, FilmWindow win) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (uint32_t)win.ew * (uint32_t)win.eh) return;
  const int x = win.ex0 + (int)(t % (uint32_t)win.ew), y = win.ey0 + (int)(t / (uint32_t)win.ew);
  R* px = film + 4 * ((size_t)y * (size_t)s.xres + (size_t)x);
  R* pm = mom + 4 * ((size_t)y * (size_t)s.xres + (size_t)x);
  R cr = px[0], cg = px[1], cb = px[2], wsum = px[3];
  R s1 = pm[0], s2 = pm[1], s0 = pm[2], s3 = pm[3];
  for (int sy = y - win.reach_y; sy <= y + win.reach_y; sy++) {
    if (sy < 0 || sy >= win.ymax) continue;
    for (int sx = x - win.reach_x; sx <= x + win.reach_x; sx++) {
      uint32_t pl;
      if (sx < 0 || sx >= s.xres || !pass_pixel_inverse(pd, sx, sy, &pl)) continue;
      for (uint32_t sl = 0; sl < pd.ns; sl++) {
        const uint32_t slot = sl * pd.npix + pl;
        const typename Vec4T<R>::type cs = p.samp[slot];
        R fw;
        if (!film_wide_weight(s, cs.x, cs.y, x, y, &fw)) continue;
        const R w = p.weight[slot];
        typename Vec4T<R>::type l = mk4<R>(R(0), R(0), R(0), R(0));
        if (w > R(0)) l = p.L[slot];
        const Rgb<R> L = film_sample_radiance(s, w, l);
        cr += (L.r * w) * fw; cg += (L.g * w) * fw; cb += (L.b * w) * fw;
        wsum += fw;
        const R ly = L.y() * w, fy = fw * ly;
        s1 += fy; s2 += fy * ly; s0 += fw; s3 += fw * fw;
      }
    }
  }
  px[0] = cr; px[1] = cg; px[2] = cb; px[3] = wsum;
  pm[0] = s1; pm[1] = s2; pm[2] = s0; pm[3] = s3;
}

// ------------------------------------------------------------------------------------------------------------
// Error map of a moments plane (rrt_tile_error, include/rrt.h) and the stopping rule of rrt_render_adaptive.
// ------------------------------------------------------------------------------------------------------------
static_assert(kTileW * kTileH == 64u, "k_tile_error: one wave per tile, one lane per pixel");
constexpr uint32_t kTeBlock = 256;   // four tiles per workgroup

// One wave per tile, one lane per pixel: one 128-bit load of the pixel's {S1, S2, S0, S3} (a tile row is kTileW consecutive records), the pixel's
// mean and variance of the mean in double (api.py resolve_moments, statement by statement and never contracted), the two sums over the wave
// by a butterfly of cross-lane shuffles (a fixed order), one store by lane 0. `list` = the tiles to measure (NULL: tiles 0 .. n - 1);
// err is indexed by tile number.
template <typename R>
__global__ void __launch_bounds__(kTeBlock) k_tile_error(const typename Vec4T<R>::type* mom, uint32_t xres, int32_t rx0, int32_t ry0, uint32_t tiles_per_row,
                                                         const uint32_t* list, uint32_t n, double* err) {
#pragma clang fp contract(off)
  const uint32_t i = blockIdx.x * (kTeBlock / 64u) + threadIdx.x / 64u, lane = threadIdx.x % 64u;
  if (i >= n) return;   // (the whole wave)
  const uint32_t tile = list ? list[i] : i;
  const uint32_t x = (uint32_t)rx0 + (tile % tiles_per_row) * kTileW + lane % kTileW, y = (uint32_t)ry0 + (tile / tiles_per_row) * kTileH + lane / kTileW;
  const typename Vec4T<R>::type rec = mom[(size_t)y * (size_t)xres + (size_t)x];
  const double s1 = (double)rec.x, s2 = (double)rec.y, s0 = (double)rec.z, s3 = (double)rec.w;
  const double n_eff = s3 > 0.0 ? s0 * s0 / s3 : 0.0;
  const double m = s0 > 0.0 ? s1 / s0 : 0.0;
  double v = 0.0;
  if (n_eff >= 2.0) v = fmax(0.0, s2 / s0 - m * m) / (n_eff - 1.0);
  double M = m, V = v;
  for (int o = 32; o > 0; o >>= 1) { M += __shfl_xor(M, o, 64); V += __shfl_xor(V, o, 64); }
  if (lane == 0u) err[tile] = M > 0.0 ? sqrt(V / 64.0) / (M / 64.0) : 0.0;
}

// The stopping rule, one workgroup: the tiles of list_in (NULL: 0 .. n - 1), kSelBlock at a time in list order. A tile with err < threshold
// (strict: threshold 0 stops nothing), and every tile when `last`, stops: tile_samples[tile] = k. The others are written to list_out in the
// order they came in - their position is the running count plus a ballot / popcount scan over the workgroup, no atomic append - so an ascending
// list stays ascending and two runs issue the same passes. *count_out = the tiles kept.
constexpr uint32_t kSelBlock = 1024;
static __global__ void __launch_bounds__(kSelBlock) k_tile_select(const uint32_t* list_in, uint32_t n, const double* err, double threshold, uint32_t k, int last,
                                                                  uint32_t* list_out, uint32_t* count_out, uint32_t* tile_samples) {
  __shared__ uint32_t wave_n[kSelBlock / 64u];
  const uint32_t tid = threadIdx.x, lane = tid % 64u, wave = tid / 64u;
  uint32_t base = 0;
  for (uint32_t i0 = 0; i0 < n; i0 += kSelBlock) {
    const uint32_t i = i0 + tid;
    bool keep = false;
    uint32_t tile = 0;
    if (i < n) {
      tile = list_in ? list_in[i] : i;
      keep = !last && !(err[tile] < threshold);
      if (!keep) tile_samples[tile] = k;
    }
    const unsigned long long b = __ballot(keep);
    if (lane == 0u) wave_n[wave] = (uint32_t)__popcll(b);
    __syncthreads();
    uint32_t off = base, tot = 0;
    for (uint32_t w = 0; w < kSelBlock / 64u; w++) { if (w < wave) off += wave_n[w]; tot += wave_n[w]; }
    if (keep) list_out[off + (uint32_t)__popcll(b & ((1ull << lane) - 1ull))] = tile;
    base += tot;
    __syncthreads();
  }
  if (tid == 0u) *count_out = base;
}

// ------------------------------------------------------------------------------------------------------------
// ID mattes (rrt_render_mattes / rrt_matte_extract, include/rrt.h): per pixel a table of K (id, coverage) slots and a weight record. A pass of
// its own beside the k_aov_* family - camera kernels, closest-hit launch, k_matte_ids, the gather over MatteAcc - around an internal table that
// lives across the pool passes of a call: k_matte_load copies the caller's table in before the first pass, k_matte_rank sorts it out after the last.
// The internal table is slot-major (ids[k * npix + pix], cov[k * npix + pix]: a wave's loads of one slot are consecutive); the caller's is
// [pixel][slot]. Nothing is ever evicted: a stored coverage is then the id's complete sum, and the overflow channel says how much is missing.
// ------------------------------------------------------------------------------------------------------------
constexpr uint32_t kMaxMatteSlots = 16;   // RRT_MAX_MATTE_SLOTS
template <typename R>
struct MatteTab {
  uint32_t* ids;                        // [slot][film pixel]
  R* cov;                               // [slot][film pixel]; 0 = the slot is empty
  typename Vec4T<R>::type* weight;      // [film pixel]: sum fw over live samples | over hit samples | overflow | 0
  uint32_t K;
  size_t npix;                          // W x H
};

// One thread per entry of the camera queue, as k_aov_shade reads it, but only the primitive index of the hit record is looked at: no surface, no
// texture. An 8-byte record per slot: {hit flag, id}. Every live sample of the pass is in the queue (no root cull), so every live slot gets a record.
template <typename R>
__global__ void __launch_bounds__(kBlock) k_matte_ids(Pools<R> p, const uint32_t* id_dev, uint32_t n_ids, uint2* rec) {
  const uint32_t n = p.counters[C_ACTIVE];
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    const uint32_t slot = p.q_active[i].slot;
    const int prim = (int)real_to_bits(p.hit[i].y);
    rec[slot] = prim < 0 ? make_uint2(0u, 0u) : make_uint2(1u, (uint32_t)prim < n_ids ? id_dev[prim] : 0u);
  }
}

// A thread's K slots in LDS, slot-major over the workgroup (word k * kBlock + tid: consecutive lanes in consecutive banks): a per-thread array
// indexed by a runtime slot number would live in scratch. K * kBlock ids, then K * kBlock coverages; a thread touches its own column only.
template <typename R>
struct MatteLds { uint32_t* id; R* cov; };
template <typename R>
RRT_DEV MatteLds<R> matte_lds(uint32_t K) {
  extern __shared__ uint32_t matte_smem[];
  return {matte_smem + threadIdx.x, reinterpret_cast<R*>(matte_smem + K * kBlock) + threadIdx.x};
}
inline size_t matte_lds_bytes(uint32_t K, size_t real_bytes) { return (size_t)K * kBlock * (sizeof(uint32_t) + real_bytes); }
template <typename R>
RRT_DEV void matte_lds_load(const MatteTab<R>& tab, const MatteLds<R>& t, size_t pix) {
  for (uint32_t k = 0; k < tab.K; k++) { t.id[k * kBlock] = tab.ids[k * tab.npix + pix]; t.cov[k * kBlock] = tab.cov[k * tab.npix + pix]; }
}
template <typename R>
RRT_DEV void matte_lds_store(const MatteTab<R>& tab, const MatteLds<R>& t, size_t pix) {
  for (uint32_t k = 0; k < tab.K; k++) { tab.ids[k * tab.npix + pix] = t.id[k * kBlock]; tab.cov[k * tab.npix + pix] = t.cov[k * kBlock]; }
}
// The table rule of rrt.h for one live sample with filter weight fw. `last`: the slot the previous hit sample went to, tried first (consecutive
// samples of a pixel mostly share an id); it finds what the search would find, since a table holds an id once.
template <typename R>
RRT_DEV void matte_add(const MatteLds<R>& t, uint32_t K, uint32_t& last, typename Vec4T<R>::type& w, R fw, uint2 rec) {
  if (fw == R(0)) return;
  w.x += fw;
  if (rec.x == 0u) return;   // a live sample that misses the scene
  w.y += fw;
  const uint32_t id = rec.y;
  if (t.id[last * kBlock] == id && t.cov[last * kBlock] != R(0)) { t.cov[last * kBlock] += fw; return; }
  uint32_t found = K, empty = K;
  for (uint32_t k = 0; k < K; k++) {
    if (t.cov[k * kBlock] != R(0)) { if (t.id[k * kBlock] == id) { found = k; break; } }
    else if (empty == K) empty = k;
  }
  if (found < K) { t.cov[found * kBlock] += fw; last = found; }
  else if (empty < K) { t.id[empty * kBlock] = id; t.cov[empty * kBlock] = fw; last = empty; }
  else w.z += fw;   // overflow: K other ids hold the slots
}

// Under the gather skeletons, launched with matte_lds_bytes of dynamic LDS: a pixel's state is its LDS column, its weight record and `last`. The
// skeletons' sample order is the arrival order the table rule of rrt.h speaks of.
template <typename R>
struct MatteAcc {
  struct Pixel { MatteLds<R> t; typename Vec4T<R>::type w; uint32_t last; };
  MatteTab<R> tab;
  const uint2* rec;
  RRT_DEV Pixel load(const SceneDev<R>&, size_t pix) const {
    const MatteLds<R> t = matte_lds<R>(tab.K);
    matte_lds_load(tab, t, pix);
    return Pixel{t, tab.weight[pix], 0u};
  }
  RRT_DEV void add(Pixel& px, R fw, uint32_t slot) const { matte_add(px.t, tab.K, px.last, px.w, fw, rec[slot]); }
  RRT_DEV void store(const SceneDev<R>&, size_t pix, const Pixel& px) const {
    matte_lds_store(tab, px.t, pix);
    tab.weight[pix] = px.w;
  }
};

// the caller's [pixel][slot] table into the internal slot-major one: one thread per (pixel, slot), reads consecutive
template <typename R>
__global__ void __launch_bounds__(kBlock) k_matte_load(const uint32_t* ids, const R* cov, MatteTab<R> tab) {
  const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= tab.npix * tab.K) return;
  const size_t pix = e / tab.K, k = e % tab.K;
  tab.ids[k * tab.npix + pix] = ids[e];
  tab.cov[k * tab.npix + pix] = cov[e];
}

// Rank on the way out: one thread per pixel sorts its K slots (insertion sort in its LDS column, K <= 16) by coverage descending, ties by
// ascending id, empty slots last as (0, 0), and writes them in the caller's [pixel][slot] layout.
template <typename R>
RRT_DEV bool matte_before(uint32_t ia, R ca, uint32_t ib, R cb) {
  if (ca == R(0)) return false;
  if (cb == R(0)) return true;
  return ca > cb || (ca == cb && ia < ib);
}
template <typename R>
__global__ void __launch_bounds__(kBlock) k_matte_rank(MatteTab<R> tab, uint32_t* ids, R* cov) {
  const size_t pix = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (pix >= tab.npix) return;
  const MatteLds<R> t = matte_lds<R>(tab.K);
  matte_lds_load(tab, t, pix);
  for (uint32_t i = 1; i < tab.K; i++) {
    const uint32_t ci = t.id[i * kBlock];
    const R cc = t.cov[i * kBlock];
    uint32_t j = i;
    while (j > 0 && matte_before<R>(ci, cc, t.id[(j - 1) * kBlock], t.cov[(j - 1) * kBlock])) {
      t.id[j * kBlock] = t.id[(j - 1) * kBlock]; t.cov[j * kBlock] = t.cov[(j - 1) * kBlock];
      j--;
    }
    t.id[j * kBlock] = ci; t.cov[j * kBlock] = cc;
  }
  for (uint32_t k = 0; k < tab.K; k++) {
    const R c = t.cov[k * kBlock];
    ids[pix * tab.K + k] = c != R(0) ? t.id[k * kBlock] : 0u;
    cov[pix * tab.K + k] = c;
  }
}

// rrt_matte_extract: one thread per pixel over a table in the caller's layout; `list` is the wanted ids, sorted and without duplicates (binary
// search). The sum and the division are in double, rounded once.
template <typename R>
__global__ void __launch_bounds__(kBlock) k_matte_extract(const uint32_t* ids, const R* cov, const typename Vec4T<R>::type* weight, uint32_t K,
                                                           const uint32_t* list, int n_list, R* alpha, size_t npix) {
  const size_t pix = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (pix >= npix) return;
  const double w0 = (double)weight[pix].x;
  double sum = 0.0;
  for (uint32_t k = 0; k < K; k++) {
    const R c = cov[pix * K + k];
    if (c == R(0)) continue;
    const uint32_t id = ids[pix * K + k];
    int lo = 0, hi = n_list - 1;
    bool in = false;
    while (lo <= hi) {
      const int mid = (lo + hi) >> 1;
      const uint32_t v = list[mid];
      if (v == id) { in = true; break; }
      if (v < id) lo = mid + 1; else hi = mid - 1;
    }
    if (in) sum += (double)c;
  }
  alpha[pix] = w0 != 0.0 ? (R)(sum / w0) : R(0);
}

// ------------------------------------------------------------------------------------------------------------
// Surface records (rrt_surface_rays, rrt_surface_at, include/rrt.h): the interaction k_aov_shade rebuilds, written out per record instead of
// summed into planes. One thread per record; every produced array gets one element per lane, so a wave's store is one contiguous run. A group
// whose pointers are NULL is a wave-uniform branch not taken: neither the tangent nor the texture context nor aov_rho is formed for it.
// ------------------------------------------------------------------------------------------------------------
template <typename R>
struct SurfaceOut { R *p[3], *n[3], *s[3], *uv[2], *rho[3], *t; int32_t *prim, *material; };
template <typename R>
struct SitesIn { const int32_t* prim; const R *b1, *b2; };

// what rrt_surface_at refuses of a site; prim == -1 is "no site"
template <typename R>
RRT_DEV bool site_ok(const SceneDev<R>& s, int32_t prim, R b1, R b2) {
  if (prim == -1) return true;
  if ((uint32_t)prim >= s.n_tris) return false;
  if (s.tris[prim].plane == kSphereMark) return false;
  return !(isinf(b1) || b1 != b1 || isinf(b2) || b2 != b2);
}
// the checking launch over a device-resident batch: nothing is written but the error bit
template <typename R>
__global__ void __launch_bounds__(kBlock) k_sites_check(SceneDev<R> s, SitesIn<R> in, uint32_t n) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  if (!site_ok(s, in.prim[i], in.b1[i], in.b2[i])) atomicOr(s.err, (uint32_t)ERR_SITE);
}

// SITE = false: record i is the hit record at pool position i (rrt_surface_rays: the rays were packed and traced as rrt_trace_closest does it).
// SITE = true: record i is site i; no pool is read.
template <typename R, bool TEX, bool SITE>
__global__ void __launch_bounds__(kBlock) k_surface(SceneDev<R> s, Pools<R> p, SitesIn<R> in, SurfaceOut<R> out, uint32_t n) {
  using V4 = typename Vec4T<R>::type;
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  int prim;
  R t, u, v;
  V3<R> o, d;
  if (SITE) {
    prim = in.prim[i]; t = R(0); u = in.b1[i]; v = in.b2[i];
    if (prim >= 0 && !site_ok(s, prim, u, v)) prim = -1;   // (the host or k_sites_check has refused the batch already: this only keeps the index inside tris[])
  } else {
    const V4 h = p.hit[i];
    prim = (int)real_to_bits(h.y); t = h.x; u = h.z; v = h.w;
    if (prim >= 0) { const V4 ro = p.ray_o[i], rd = p.ray_d[i]; o = V3<R>(ro.x, ro.y, ro.z); d = V3<R>(rd.x, rd.y, rd.z); }
  }
  const bool want_s = out.s[0] != nullptr, want_uv = out.uv[0] != nullptr, want_rho = out.rho[0] != nullptr;
  V3<R> pw, nn, ss;
  R tu = R(0), tv = R(0);
  Rgb<R> rho(R(0));
  int32_t material = -1;
  if (prim >= 0) {
    SurfExt<R> ext;   // (always asked for: a pointer that is NULL on some paths keeps the struct in scratch; its unread members fold away)
    const Surf<R> si = build_surface<R, SITE>(s, prim, o, d, t, u, v, &ext);
    if (!si.ok) atomicOr(s.err, (uint32_t)ERR_SHADING_NORMAL);   // primitives.rs:66, as the frame reports it
    pw = si.p + si.p_lo;
    nn = vnormalize(si.n);
    material = (int32_t)si.material;
    if (want_s) ss = vnormalize(ao_dpdu(s, prim, si));
    if (want_uv) { tu = ext.u; tv = ext.v; }
    if (want_rho) {
      TexCtx<R> tc;
      if (TEX) {   // dpdx = dpdy = 0, dudx .. dvdy = 0 (TexCtx's defaults), as k_aov_shade sets it
        tc.p = si.p; tc.u = ext.u; tc.v = ext.v;
        tc.pd = V3<double>((double)si.p.x + (double)si.p_lo.x, (double)si.p.y + (double)si.p_lo.y, (double)si.p.z + (double)si.p_lo.z);
      }
      rho = aov_rho<R, TEX>(s, s.materials[si.material], tc);
      if (TEX) { if (tc.err) atomicOr(s.err, (uint32_t)ERR_MIPMAP); }
    }
  }
  if (out.p[0]) { out.p[0][i] = pw.x; out.p[1][i] = pw.y; out.p[2][i] = pw.z; }
  if (out.n[0]) { out.n[0][i] = nn.x; out.n[1][i] = nn.y; out.n[2][i] = nn.z; }
  if (want_s) { out.s[0][i] = ss.x; out.s[1][i] = ss.y; out.s[2][i] = ss.z; }
  if (want_uv) { out.uv[0][i] = tu; out.uv[1][i] = tv; }
  if (want_rho) { out.rho[0][i] = rho.r; out.rho[1][i] = rho.g; out.rho[2][i] = rho.b; }
  if (out.t) out.t[i] = t;
  if (out.prim) { out.prim[i] = prim; out.material[i] = material; }
}

// ------------------------------------------------------------------------------------------------------------
// Lightmap sites (rrt_atlas_sites, include/rrt.h): which triangle, at which barycentrics, each texel centre of a uv atlas shows. All arithmetic
// is in double in both precision modes and is never contracted (the pragma below), so both builds and a plain numpy restatement form the
// same bits.
// ------------------------------------------------------------------------------------------------------------
struct AtlasUv { double a[2], b[2], c[2]; };
// the candidate's texture coordinates: its mesh uv, else get_uvs' (0,0), (1,0), (1,1) (triangle.rs:113-128); the object's own, no transform
template <typename R>
RRT_DEV AtlasUv atlas_uv(const SceneDev<R>& s, int prim) {
  AtlasUv t{{0.0, 0.0}, {1.0, 0.0}, {1.0, 1.0}};
  const uint32_t shade = s.tris[prim].shade;
  if (shade != 0xffffffffu) {
    const TriShade<R>& sh = s.shades[shade];
    if (sh.has_uv) {
      t.a[0] = (double)sh.uv[0][0]; t.a[1] = (double)sh.uv[0][1]; t.b[0] = (double)sh.uv[1][0]; t.b[1] = (double)sh.uv[1][1];
      t.c[0] = (double)sh.uv[2][0]; t.c[1] = (double)sh.uv[2][1];
    }
  }
  return t;
}
// beta of the texel centre (x + 0.5) / aw, (y + 0.5) / ah in the candidate; true = covered (edges inclusive). A == 0 covers nothing.
RRT_DEV bool atlas_beta(const AtlasUv& t, uint32_t x, uint32_t y, double aw, double ah, double* b1, double* b2) {
#pragma clang fp contract(off)
  const double cx = ((double)x + 0.5) / aw, cy = ((double)y + 0.5) / ah;
  const double bax = t.b[0] - t.a[0], bay = t.b[1] - t.a[1], cax = t.c[0] - t.a[0], cay = t.c[1] - t.a[1];
  const double A = bax * cay - bay * cax;
  *b1 = 0.0; *b2 = 0.0;
  if (!(A != 0.0)) return false;   // (a NaN area covers nothing either)
  const double px = cx - t.a[0], py = cy - t.a[1];
  const double e1 = (px * cay - py * cax) / A, e2 = (bax * py - bay * px) / A;
  *b1 = e1; *b2 = e2;
  return e1 >= 0.0 && e2 >= 0.0 && e1 + e2 <= 1.0;
}

// One wave per candidate (list position k = wave index): the lanes stride the texels of its uv bounding box, grown by one texel and clipped to
// the atlas - the coverage test itself decides - and take atomicMin of k into owner[], pre-filled with ~0u.
template <typename R>
__global__ void __launch_bounds__(kBlock) k_atlas_owner(SceneDev<R> s, const int32_t* list, uint32_t n_list, uint32_t aw, uint32_t ah, uint32_t* owner) {
  const uint32_t k = (uint32_t)(((size_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6), lane = threadIdx.x & 63u;
  if (k >= n_list) return;
  const AtlasUv t = atlas_uv(s, list[k]);
  const double daw = (double)aw, dah = (double)ah;
  const double u0 = fmin(fmin(t.a[0], t.b[0]), t.c[0]), u1 = fmax(fmax(t.a[0], t.b[0]), t.c[0]);
  const double v0 = fmin(fmin(t.a[1], t.b[1]), t.c[1]), v1 = fmax(fmax(t.a[1], t.b[1]), t.c[1]);
  if (!(u0 <= u1) || !(v0 <= v1) || isinf(u0) || isinf(u1) || isinf(v0) || isinf(v1)) return;   // NaN or infinite coordinates cover nothing
  // texel columns [x0, x1), rows [y0, y1): clamped as doubles before the conversion
  const uint32_t x0 = (uint32_t)fmin(fmax(floor(u0 * daw) - 1.0, 0.0), daw), x1 = (uint32_t)fmin(fmax(ceil(u1 * daw) + 1.0, 0.0), daw);
  const uint32_t y0 = (uint32_t)fmin(fmax(floor(v0 * dah) - 1.0, 0.0), dah), y1 = (uint32_t)fmin(fmax(ceil(v1 * dah) + 1.0, 0.0), dah);
  if (x1 <= x0 || y1 <= y0) return;
  const uint32_t bw = x1 - x0, total = bw * (y1 - y0);   // <= 16384^2 = 2^28
  for (uint32_t idx = lane; idx < total; idx += 64u) {
    const uint32_t x = x0 + idx % bw, y = y0 + idx / bw;   // x < aw, y < ah
    double b1, b2;
    if (atlas_beta(t, x, y, daw, dah, &b1, &b2)) atomicMin(&owner[(size_t)y * aw + x], k);
  }
}

// One thread per texel: beta again for the owner, the three outputs coalesced, the owned texels counted with one atomic per wave.
template <typename R>
__global__ void __launch_bounds__(kBlock) k_atlas_emit(SceneDev<R> s, const int32_t* list, const uint32_t* owner, uint32_t aw, uint32_t ah, int32_t* site_prim, R* b1o, R* b2o,
                                                        unsigned long long* n_covered) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const bool in = i < (size_t)aw * ah;
  bool owned = false;
  if (in) {
    const uint32_t k = owner[i];
    int32_t prim = -1;
    double b1 = 0.0, b2 = 0.0;
    if (k != ~0u) {
      prim = list[k];
      atlas_beta(atlas_uv(s, prim), (uint32_t)(i % aw), (uint32_t)(i / aw), (double)aw, (double)ah, &b1, &b2);
      owned = true;
    }
    site_prim[i] = prim; b1o[i] = (R)b1; b2o[i] = (R)b2;
  }
  const unsigned long long m = __ballot(owned);
  if ((threadIdx.x & 63u) == 0u && m != 0ull) atomicAdd(n_covered, (unsigned long long)__popcll(m));
}

// ------------------------------------------------------------------------------------------------------------
// Nearest-surface point queries (rrt_nearest, include/rrt.h): one lane per point over the linear tree (host/nearest.hpp nearest_walk). The stack
// holds node indices only - a popped node is fetched and its box judged against the bound of that moment - as [entry][thread of the launch] in
// global memory, stack_depth entries per thread, like the generic closest-hit kernel's deep stack. Point base + i of the call is thread i.
// ------------------------------------------------------------------------------------------------------------
template <typename R>
struct NearestIO {
  const R *px, *py, *pz;
  int32_t* prim;
  R *b1, *b2, *dist;       // dist may be null
  R max_dist, prune0, delta;   // prune0 = nn_prune_start(max_dist, delta), delta = kNearestPadUlps x eps x M
};
template <typename R>
RRT_DEV void nearest_store(const NearestIO<R>& io, size_t g, const NnBest<R>& best) {
  const NnOut<R> o = nn_result<R>(best, io.max_dist);
  io.prim[g] = o.prim; io.b1[g] = o.b1; io.b2[g] = o.b2;
  if (io.dist) io.dist[g] = o.dist;
}
template <typename R>
__global__ void __launch_bounds__(kBlock) k_nearest(const Node<R>* nodes, uint32_t n_nodes, const Tri<R>* tris, uint32_t n_tris, const InstDev<R>* insts, uint32_t* err,
                                                     NearestIO<R> io, size_t base, uint32_t n, uint32_t* stack, uint32_t stride, uint32_t stack_cap) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const size_t g = base + i;
  const R px = io.px[g], py = io.py[g], pz = io.pz[g];
  NnBest<R> best = nn_none<R>();
  if (nn_finite(px) && nn_finite(py) && nn_finite(pz)) {   // a point with a non-finite coordinate is dead
    GlobStack st{stack + i, stride};
    if (!nearest_walk<R>(nodes, n_nodes, tris, n_tris, insts, px, py, pz, io.prune0, io.delta, st, stack_cap, &best)) atomicOr(err, (uint32_t)ERR_NEAREST);
  }
  nearest_store<R>(io, g, best);
}

// ------------------------------------------------------------------------------------------------------------
// All hits along a ray, in order (rrt_trace_all, include/rrt.h): one lane per ray over the linear tree (host/multihit.hpp multihit_walk). The stack
// is private for trees up to 64 deep and [entry][thread of the launch] in global memory for deeper ones (DEEP), as k_closest's. The k-buffer holds
// (t, prim) per slot in dynamic LDS, [slot][thread of the block] - k x blockDim x (sizeof(R) + 4) bytes, the t plane first -, so that no
// runtime-indexed private array goes to scratch; b1 and b2 of the surviving slots are recomputed after the walk by the same triangle test. A lane
// touches its own column only: no barrier. Ray base + i of the call is thread i; slot s of ray j is at [s * io.n + j].
// ------------------------------------------------------------------------------------------------------------
template <typename R>
struct TraceAllIO {
  const R *ox, *oy, *oz, *dx, *dy, *dz, *tmax;
  const int32_t* skip;     // may be null
  R* t;
  int32_t* prim;
  R *b1, *b2;              // both null or both set
  uint32_t* count;         // may be null
  size_t n;                // rays of the call: the stride of a slot plane
  uint32_t k;
  R delta;                 // kMultihitPadUlps x eps x M for scenes with kept instances, else 0
};
template <typename R>
struct LdsHits {
  R* ts;
  int32_t* ps;
  uint32_t stride;
  RRT_DEV R t(uint32_t s) const { return ts[s * stride]; }
  RRT_DEV int32_t prim(uint32_t s) const { return ps[s * stride]; }
  RRT_DEV void set(uint32_t s, R t, int32_t p) { ts[s * stride] = t; ps[s * stride] = p; }
};
extern __shared__ double trace_all_lds[];
template <typename R, bool DEEP>
__global__ void __launch_bounds__(kBlock) k_trace_all(const Node<R>* nodes, uint32_t n_nodes, const Tri<R>* tris, uint32_t n_tris, const InstDev<R>* insts, uint32_t* err,
                                                       TraceAllIO<R> io, size_t base, uint32_t n, uint32_t* stack, uint32_t stride, uint32_t stack_cap) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const size_t g = base + i;
  R* const lds_t = reinterpret_cast<R*>(trace_all_lds);
  LdsHits<R> buf{lds_t + threadIdx.x, reinterpret_cast<int32_t*>(lds_t + (size_t)io.k * blockDim.x) + threadIdx.x, blockDim.x};
  MhRay<R> r;
  const bool live = mh_make_ray<R>(io.ox[g], io.oy[g], io.oz[g], io.dx[g], io.dy[g], io.dz[g], io.tmax[g], &r);
  const int32_t skip = io.skip ? io.skip[g] : -1;
  uint32_t count = 0u;
  if (live) {
    bool ok;
    if (DEEP) { GlobStack st{stack + i, stride}; ok = multihit_walk<R>(nodes, n_nodes, tris, n_tris, insts, r, skip, io.delta, st, stack_cap, buf, io.k, &count); }
    else { PrivStack st; ok = multihit_walk<R>(nodes, n_nodes, tris, n_tris, insts, r, skip, io.delta, st, stack_cap < 64u ? stack_cap : 64u, buf, io.k, &count); }
    if (!ok) { atomicOr(err, (uint32_t)ERR_TRACE_ALL); count = 0u; }
  }
  if (io.count) io.count[g] = count;
  const uint32_t held = count < io.k ? count : io.k;
  for (uint32_t s = 0; s < io.k; s++) {
    const size_t at = (size_t)s * io.n + g;
    if (s < held) {
      const int32_t p = buf.prim(s);
      io.t[at] = buf.t(s); io.prim[at] = p;
      if (io.b1) { const MhHit<R> h = mh_rehit<R>(r, tris[p], insts); io.b1[at] = h.u; io.b2[at] = h.v; }
    } else {
      io.t[at] = io.tmax[g]; io.prim[at] = -1;
      if (io.b1) { io.b1[at] = R(0); io.b2[at] = R(0); }
    }
  }
}

// ------------------------------------------------------------------------------------------------------------
// Mutual visibility of two point sets as a packed bit matrix (rrt_visibility, include/rrt.h): one lane per pair over the linear tree
// (host/visibility.hpp vis_segment, vis_walk). A wavefront is one output word: task w of the call is word w % words of row w / words in MATRIX mode -
// 64 consecutive columns of ONE row, so the row's point, normal and skip entry are wave-uniform loads (readfirstlane puts the row index into an SGPR)
// and the column loads are coalesced - and rows 64 w .. 64 w + 63 in PAIRS mode. The 64 verdicts are collected with one __ballot and lane 0 stores
// the word with an ordinary 64-bit store; lanes past the last column (row) vote 0, which is the zero padding. count[row] += popcount(word) by one
// integer atomicAdd per word into a plane the driver zeroed: integer sums are order-free. The stack is k_trace_all's: private up to 64 deep,
// [entry][thread of the launch] in global memory beyond (DEEP). A launch holds whole waves only (n_tasks x 64 threads), so the early return below
// retires whole waves and every lane of a live wave reaches the ballot.
// ------------------------------------------------------------------------------------------------------------
template <typename R>
struct VisIO {
  const R *ax, *ay, *az, *anx, *any, *anz;   // normals: all null or all set
  const R *bx, *by, *bz, *bnx, *bny, *bnz;
  const int32_t *skip_a, *skip_b;            // may be null
  uint64_t* bits;
  uint32_t* count;                           // may be null (MATRIX); null in PAIRS
  uint32_t n_a, n_b, words;                  // words per row (MATRIX)
  int32_t mode, b_kind;
  uint32_t flags;
  R off_a, off_b, delta;
};
template <typename R, bool DEEP>
__global__ void __launch_bounds__(kBlock) k_visibility(const Node<R>* nodes, uint32_t n_nodes, const Tri<R>* tris, uint32_t n_tris, const InstDev<R>* insts, uint32_t* err, VisIO<R> io,
                                                        unsigned long long task0, uint32_t n_tasks, uint32_t* stack, uint32_t stride, uint32_t stack_cap) {
  const uint32_t th = blockIdx.x * blockDim.x + threadIdx.x;   // thread of the launch
  if ((th >> 6) >= n_tasks) return;                             // (whole waves)
  const unsigned long long w = task0 + (th >> 6);
  const uint32_t lane = th & 63u;
  uint32_t i, j;
  bool in_range;
  if (io.mode == kVisMatrix) {
    i = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(w / io.words));
    j = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(w % io.words)) * 64u + lane;
    in_range = j < io.n_b;
  } else {
    i = j = (uint32_t)w * 64u + lane;
    in_range = i < io.n_a;
  }
  bool visible = false;
  if (in_range) {
    const bool an = io.anx != nullptr, bn = io.bnx != nullptr;
    const VisEnd<R> a = vis_end<R>(io.ax[i], io.ay[i], io.az[i], an, an ? io.anx[i] : R(0), an ? io.any[i] : R(0), an ? io.anz[i] : R(0), io.off_a);
    const VisEnd<R> b = vis_end<R>(io.bx[j], io.by[j], io.bz[j], bn, bn ? io.bnx[j] : R(0), bn ? io.bny[j] : R(0), bn ? io.bnz[j] : R(0), io.off_b);
    MhRay<R> r;
    const VisVerdict v = vis_segment<R>(a, b, io.b_kind, io.flags, &r);
    visible = v == kVisYes;
    if (v == kVisTrace) {
      const int32_t sa = io.skip_a ? io.skip_a[i] : -1, sb = io.skip_b ? io.skip_b[j] : -1;
      bool ok, blocked = true;
      if (DEEP) { GlobStack st{stack + th, stride}; ok = vis_walk<R>(nodes, n_nodes, tris, n_tris, insts, r, sa, sb, io.delta, st, stack_cap, &blocked); }
      else { PrivStack st; ok = vis_walk<R>(nodes, n_nodes, tris, n_tris, insts, r, sa, sb, io.delta, st, stack_cap < 64u ? stack_cap : 64u, &blocked); }
      if (!ok) { atomicOr(err, (uint32_t)ERR_VISIBILITY); blocked = true; }
      visible = !blocked;
    }
  }
  const unsigned long long word = __ballot(visible);
  if (lane == 0u) {
    io.bits[w] = word;
    if (io.count) atomicAdd(io.count + i, (uint32_t)__popcll(word));
  }
}

}  // namespace rrtd
