// rrt_denoise (include/rrt.h): edge-avoiding a-trous wavelet filter over the film, guided by the planes of rrt_render_aov. The definition is on the
// prototype; tests/denoise_reference.py restates it in numpy. One thread per pixel, 32 x 8 workgroups (one wave = two 32-pixel rows), three planes
// of 128-bit records per pixel:
//   C = {c.r, c.g, c.b, v}   demodulated colour and the variance of its luminance, ping-ponged by the iterations; v = -1: a pixel without data
//   G = {n.x, n.y, n.z, z}   unit normal and mean depth of the first hits; z = -1: no hit (a hit always has t > 0)
//   P = {d.r, d.g, d.b, sd}  demodulation divisor and depth spread, read by the centre pixel only
// so a tap costs two 16-byte loads. k_dn_prepare and k_dn_finish run in double in both precision modes (once per pixel: the sum t^2 cancellation
// and the divisions by the weights are then the reference's); k_dn_moments and k_dn_atrous run in the handle's type.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dtypes.hpp"

namespace rrtd {

constexpr int kDnBX = 32, kDnBY = 8;      // workgroup = 32 x 8 pixels
constexpr int kDnMomentsHalo = 3;         // 7 x 7 window of the initial variance

template <typename R>
struct DnParams {
  int W, H;
  R sigma_color, sigma_normal, sigma_depth;
};

#define RRT_DN_DEV __device__ __forceinline__

template <typename V4, typename R> RRT_DN_DEV V4 dn_mk4(R x, R y, R z, R w) { V4 v; v.x = x; v.y = y; v.z = z; v.w = w; return v; }
// The tap arithmetic is shared by two kernels (direct gathers, LDS tile) whose results must be the same bits. Left to the compiler, the fp32 unit
// fuses a * b + c in one instantiation and not in the other (measured: last-bit differences between the two forms), so the shared functions pin
// contraction off and spell their fused multiply-adds out.
RRT_DN_DEV float dn_fma(float a, float b, float c) { return __builtin_fmaf(a, b, c); }
RRT_DN_DEV double dn_fma(double a, double b, double c) { return __builtin_fma(a, b, c); }
template <typename R> RRT_DN_DEV R dn_lum(R r, R g, R b) {
#pragma clang fp contract(off)
  return dn_fma(R(0.072169), b, dn_fma(R(0.715160), g, R(0.212671) * r));
}
RRT_DN_DEV float dn_exp(float x) { return expf(x); }
RRT_DN_DEV double dn_exp(double x) { return exp(x); }
RRT_DN_DEV float dn_log(float x) { return logf(x); }
RRT_DN_DEV double dn_log(double x) { return log(x); }
RRT_DN_DEV float dn_sqrt(float x) { return sqrtf(x); }
RRT_DN_DEV double dn_sqrt(double x) { return sqrt(x); }

// log of the surface weight g(p, q) between two HIT pixels: sigma_normal * log(max(0, n_p . n_q)); -inf (g = 0 exactly) for normals at 90 degrees
// or more. The a-trous taps add the depth and luminance exponents to it and take one exp.
template <typename R, typename V4>
RRT_DN_DEV R dn_log_g(const V4& gp, const V4& gq, R sigma_normal) {
#pragma clang fp contract(off)
  const R d = fmax(R(0), dn_fma(gp.z, gq.z, dn_fma(gp.y, gq.y, gp.x * gq.x)));
  return sigma_normal * dn_log(d);
}
// g(p, q): 0 where one is hit and the other is not, 1 where neither is
template <typename R, typename V4>
RRT_DN_DEV R dn_g(const V4& gp, const V4& gq, R sigma_normal) {
  const bool hp = gp.w > R(0), hq = gq.w > R(0);
  if (hp != hq) return R(0);
  if (!hp) return R(1);
  return dn_exp(dn_log_g<R>(gp, gq, sigma_normal));
}

// ---- prepare: the sums of the film and the planes -> records (double arithmetic in both modes) -------------------------------------------------------
template <typename R>
__global__ void __launch_bounds__(256) k_dn_prepare(const typename Vec4T<R>::type* __restrict__ film, const typename Vec4T<R>::type* __restrict__ alb,
                                                    const typename Vec4T<R>::type* __restrict__ nrm, const typename Vec4T<R>::type* __restrict__ dep,
                                                    typename Vec4T<R>::type* __restrict__ C, typename Vec4T<R>::type* __restrict__ G,
                                                    typename Vec4T<R>::type* __restrict__ P, size_t npix, int demodulate) {
  using V4 = typename Vec4T<R>::type;
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= npix) return;
  const V4 f = film[i], a4 = alb[i], n4 = nrm[i], d4 = dep[i];
  const double w = (double)f.w;
  const bool data = w > 0.0;
  double c[3] = {0.0, 0.0, 0.0}, d[3] = {1.0, 1.0, 1.0};
  const double w_live = (double)a4.w;
  if (demodulate) {
    const double a[3] = {(double)a4.x, (double)a4.y, (double)a4.z};
    for (int k = 0; k < 3; k++) d[k] = fmax(w_live != 0.0 ? a[k] / w_live : 0.0, 1e-3);
  }
  if (data) {
    const double X = (double)f.x / w, Y = (double)f.y / w, Z = (double)f.z / w;
    const double rgb[3] = {3.240479 * X - 1.537150 * Y - 0.498535 * Z, -0.969256 * X + 1.875991 * Y + 0.041556 * Z, 0.055648 * X - 0.204043 * Y + 1.057311 * Z};
    for (int k = 0; k < 3; k++) c[k] = rgb[k] / d[k];
  }
  const double w_hit = (double)d4.z;
  const bool hit = w_hit > 0.0;
  double n[3] = {0.0, 0.0, 0.0}, z = -1.0, sd = 0.0;
  if (hit) {
    z = (double)d4.x / w_hit;
    sd = sqrt(fmax(0.0, (double)d4.y / w_hit - z * z));
    const double nx = (double)n4.x, ny = (double)n4.y, nz = (double)n4.z, len = sqrt(nx * nx + ny * ny + nz * nz);
    if (len > 0.0) { n[0] = nx / len; n[1] = ny / len; n[2] = nz / len; }
  }
  C[i] = dn_mk4<V4, R>((R)c[0], (R)c[1], (R)c[2], data ? R(0) : R(-1));
  G[i] = dn_mk4<V4, R>((R)n[0], (R)n[1], (R)n[2], (R)z);
  P[i] = dn_mk4<V4, R>((R)d[0], (R)d[1], (R)d[2], (R)sd);
}

// ---- finish: records -> film sums (double arithmetic in both modes); `out` may be `film` ------------------------------------------------------------
template <typename R>
__global__ void __launch_bounds__(256) k_dn_finish(const typename Vec4T<R>::type* film, const typename Vec4T<R>::type* __restrict__ C,
                                                   const typename Vec4T<R>::type* __restrict__ P, typename Vec4T<R>::type* out, size_t npix) {
  using V4 = typename Vec4T<R>::type;
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= npix) return;
  const V4 f = film[i];
  const V4 c = C[i];
  if (!(c.w >= R(0))) { out[i] = f; return; }   // no data: copied through
  const V4 p = P[i];
  const double w = (double)f.w;
  const double r = (double)c.x * (double)p.x, g = (double)c.y * (double)p.y, b = (double)c.z * (double)p.z;
  const double X = 0.412453 * r + 0.357580 * g + 0.180423 * b, Y = 0.212671 * r + 0.715160 * g + 0.072169 * b, Z = 0.019334 * r + 0.119193 * g + 0.950227 * b;
  out[i] = dn_mk4<V4, R>((R)(X * w), (R)(Y * w), (R)(Z * w), f.w);
}

// ---- initial variance: weighted luminance moments of the 7 x 7 window, from an LDS tile with a 3-pixel halo ------------------------------------------
// The moments are taken of l_q - l_p: the variance is the same number, without the cancellation of sum l^2 / n - mean^2 at the size of l^2.
template <typename R>
__global__ void __launch_bounds__(kDnBX* kDnBY) k_dn_moments(const typename Vec4T<R>::type* __restrict__ Cin, typename Vec4T<R>::type* __restrict__ Cout,
                                                             const typename Vec4T<R>::type* __restrict__ G, DnParams<R> k) {
  using V4 = typename Vec4T<R>::type;
  constexpr int HALO = kDnMomentsHalo, TW = kDnBX + 2 * HALO, TH = kDnBY + 2 * HALO;
  __shared__ V4 tg[TW * TH];
  __shared__ R tl[TW * TH];       // luminance; usable flag in tu
  __shared__ uint8_t tu[TW * TH];
  const int tid = threadIdx.y * kDnBX + threadIdx.x;
  const int x0 = blockIdx.x * kDnBX - HALO, y0 = blockIdx.y * kDnBY - HALO;
  for (int t = tid; t < TW * TH; t += kDnBX * kDnBY) {
    const int tx = t % TW, ty = t / TW, gx = x0 + tx, gy = y0 + ty;
    V4 g = dn_mk4<V4, R>(R(0), R(0), R(0), R(-1));
    R l = R(0);
    uint8_t u = 0;
    if (gx >= 0 && gx < k.W && gy >= 0 && gy < k.H) {
      const size_t q = (size_t)gy * (size_t)k.W + (size_t)gx;
      const V4 c = Cin[q];
      if (c.w >= R(0)) { u = 1; l = dn_lum<R>(c.x, c.y, c.z); g = G[q]; }
    }
    tg[t] = g; tl[t] = l; tu[t] = u;
  }
  __syncthreads();
  const int x = blockIdx.x * kDnBX + threadIdx.x, y = blockIdx.y * kDnBY + threadIdx.y;
  if (x >= k.W || y >= k.H) return;
  const size_t i = (size_t)y * (size_t)k.W + (size_t)x;
  V4 cp = Cin[i];
  const int ct = (threadIdx.y + HALO) * TW + threadIdx.x + HALO;
  if (!tu[ct]) { Cout[i] = cp; return; }
  const V4 gp = tg[ct];
  const R lp = tl[ct];
  R sg = R(0), s1 = R(0), s2 = R(0);
  for (int dy = -HALO; dy <= HALO; dy++)
    for (int dx = -HALO; dx <= HALO; dx++) {
      const int t = ct + dy * TW + dx;
      if (!tu[t]) continue;
      const R g = dn_g<R>(gp, tg[t], k.sigma_normal), dl = tl[t] - lp;
      sg += g; s1 = dn_fma(g, dl, s1); s2 = dn_fma(g * dl, dl, s2);
    }
  R v = R(0);
  if (sg > R(0)) { const R m = s1 / sg; v = fmax(R(0), s2 / sg - m * m); }
  cp.w = v;
  Cout[i] = cp;
}

// ---- rrt_denoise_moments: the variance of the pixel's mean from the plane of rrt_render_moments, where the pixel has one ----------------------------
// Runs after k_dn_moments over the same C records: v is replaced where n_eff >= 2 and S1 > 0, the spatial estimate stays everywhere else. One
// thread per pixel, double arithmetic in both modes, one rounding to the record type. `M` = {S1, S2, S0, S3} per pixel.
template <typename R>
__global__ void __launch_bounds__(256) k_dn_sample_variance(const typename Vec4T<R>::type* __restrict__ M, typename Vec4T<R>::type* __restrict__ C, size_t npix) {
  using V4 = typename Vec4T<R>::type;
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= npix) return;
  const V4 c = C[i];
  if (!(c.w >= R(0))) return;   // no data
  const V4 m = M[i];
  const double s1 = (double)m.x, s2 = (double)m.y, s0 = (double)m.z, s3 = (double)m.w;
  const double n_eff = s3 > 0.0 ? s0 * s0 / s3 : 0.0;
  if (!(n_eff >= 2.0) || !(s1 > 0.0)) return;
  const double l = 0.212671 * (double)c.x + 0.715160 * (double)c.y + 0.072169 * (double)c.z;
  const double rel = fmax(0.0, (s2 / s1) * (s0 / s1) - 1.0);   // = S2 S0 / S1^2 - 1, without the square of a tiny S1 underflowing
  C[i].w = (R)(l * l * rel / (n_eff - 1.0));
}

// ---- one a-trous iteration ---------------------------------------------------------------------------------------------------------------------------
// dn_prefilter_tap / dn_tap hold the arithmetic of a tap; the two fetch forms (direct gathers, LDS tile) call them with the same records in the
// same order, so their results are the same bits.
template <typename R, typename V4>
RRT_DN_DEV void dn_prefilter_tap(const V4& gp, const V4& cq, const V4& gq, R kw, R sigma_normal, R& sk, R& sv) {
#pragma clang fp contract(off)
  const R kg = kw * dn_g<R>(gp, gq, sigma_normal);
  sk += kg; sv = dn_fma(kg, cq.w, sv);
}

template <typename R>
struct DnCentre {   // what the 25 taps need of the centre pixel
  R l, inv_l;       // luminance, 1 / (sigma_color sqrt(gv) + 1e-3 |l| + 1e-30) (0: sigma_color <= 0)
  R z, sd, z_floor; // depth, spread, 1e-3 z
  bool hit;
};

template <typename R, typename V4>
RRT_DN_DEV void dn_tap(const DnCentre<R>& p, const V4& gp, const V4& cq, const V4& gq, R hh, R reach, const DnParams<R>& k, R& sw, R& sr, R& sg, R& sb, R& sv) {
#pragma clang fp contract(off)
  const bool hq = gq.w > R(0);
  if (hq != p.hit) return;                                   // g = 0
  R e = -fabs(p.l - dn_lum<R>(cq.x, cq.y, cq.z)) * p.inv_l;   // log w_l
  if (p.hit) {
    e += dn_log_g<R>(gp, gq, k.sigma_normal);                                     // log g
    e -= fabs(p.z - gq.w) / (k.sigma_depth * dn_fma(reach, p.sd, p.z_floor));     // log w_z
  }
  const R w = hh * dn_exp(e);
  sw += w; sr = dn_fma(w, cq.x, sr); sg = dn_fma(w, cq.y, sg); sb = dn_fma(w, cq.z, sb); sv = dn_fma(w * w, cq.w, sv);
}

RRT_DN_DEV constexpr float dn_b3(int d) { return d == 0 ? 0.375f : (d == 1 || d == -1) ? 0.25f : 0.0625f; }

// fetch1(ox, oy, cq, gq): the records of pixel p + (ox, oy), |ox|, |oy| <= 1; fetch(dx, dy, cq, gq): those of p + S (dx, dy). Both return false
// where that pixel is outside the frame or has no data.
template <typename R, int S, typename F1, typename F>
RRT_DN_DEV typename Vec4T<R>::type dn_filter_pixel(const typename Vec4T<R>::type& cp, const typename Vec4T<R>::type& gp, R sd, const DnParams<R>& k, F1&& fetch1, F&& fetch) {
#pragma clang fp contract(off)
  using V4 = typename Vec4T<R>::type;
  // the variance, prefiltered over the 3 x 3 neighbourhood at step 1
  R sk = R(0), skv = R(0);
#pragma unroll
  for (int dy = -1; dy <= 1; dy++)
#pragma unroll
    for (int dx = -1; dx <= 1; dx++) {
      V4 cq, gq;
      if (!fetch1(dx, dy, cq, gq)) continue;
      dn_prefilter_tap<R>(gp, cq, gq, R((2 - (dy < 0 ? -dy : dy)) * (2 - (dx < 0 ? -dx : dx))), k.sigma_normal, sk, skv);
    }
  const R gv = sk > R(0) ? skv / sk : cp.w;
  DnCentre<R> p;
  p.l = dn_lum<R>(cp.x, cp.y, cp.z);
  p.inv_l = k.sigma_color > R(0) ? R(1) / (dn_fma(k.sigma_color, dn_sqrt(fmax(gv, R(0))), R(1e-3) * fabs(p.l)) + R(1e-30)) : R(0);
  p.hit = gp.w > R(0);
  p.z = gp.w; p.sd = sd; p.z_floor = R(1e-3) * gp.w;
  R sw = R(0), sr = R(0), sg = R(0), sb = R(0), sv = R(0);
#pragma unroll
  for (int dy = -2; dy <= 2; dy++)
#pragma unroll
    for (int dx = -2; dx <= 2; dx++) {
      const R hh = R(dn_b3(dy)) * R(dn_b3(dx));
      if (dx == 0 && dy == 0) { sw += hh; sr = dn_fma(hh, cp.x, sr); sg = dn_fma(hh, cp.y, sg); sb = dn_fma(hh, cp.z, sb); sv = dn_fma(hh * hh, cp.w, sv); continue; }
      V4 cq, gq;
      if (!fetch(dx, dy, cq, gq)) continue;
      const int m = (dx < 0 ? -dx : dx) > (dy < 0 ? -dy : dy) ? (dx < 0 ? -dx : dx) : (dy < 0 ? -dy : dy);
      dn_tap<R>(p, gp, cq, gq, hh, R(m * S), k, sw, sr, sg, sb, sv);
    }
  const R inv = R(1) / sw;
  return dn_mk4<V4, R>(sr * inv, sg * inv, sb * inv, sv * inv * inv);
}

// (a) direct gathers: every tap is two 16-byte loads through the vector L1 / L2
template <typename R, int S>
__global__ void __launch_bounds__(kDnBX* kDnBY) k_dn_atrous(const typename Vec4T<R>::type* __restrict__ Cin, typename Vec4T<R>::type* __restrict__ Cout,
                                                            const typename Vec4T<R>::type* __restrict__ G, const typename Vec4T<R>::type* __restrict__ P, DnParams<R> k) {
  using V4 = typename Vec4T<R>::type;
  const int x = blockIdx.x * kDnBX + threadIdx.x, y = blockIdx.y * kDnBY + threadIdx.y;
  if (x >= k.W || y >= k.H) return;
  const size_t i = (size_t)y * (size_t)k.W + (size_t)x;
  const V4 cp = Cin[i];
  if (!(cp.w >= R(0))) { Cout[i] = cp; return; }
  const V4 gp = G[i];
  auto fetch = [&](int ox, int oy, V4& cq, V4& gq) -> bool {
    const int qx = x + ox, qy = y + oy;
    if (qx < 0 || qx >= k.W || qy < 0 || qy >= k.H) return false;
    const size_t q = (size_t)qy * (size_t)k.W + (size_t)qx;
    cq = Cin[q];
    if (!(cq.w >= R(0))) return false;
    gq = G[q];
    return true;
  };
  auto fetch_s = [&](int dx, int dy, V4& cq, V4& gq) -> bool { return fetch(S * dx, S * dy, cq, gq); };
  Cout[i] = dn_filter_pixel<R, S>(cp, gp, P[i].w, k, fetch, fetch_s);
}

// (b) LDS tile of the workgroup's pixels and a halo of 2 S on the pixel grid: (32 + 4 S) x (8 + 4 S) records of C and of G. Rows are contiguous
// 16-byte records, so the 32 lanes of a row read 512 consecutive bytes whatever the tap's column offset; the wave's second row starts (32 + 4 S) x 16
// bytes further on.
template <typename R, int S>
__global__ void __launch_bounds__(kDnBX* kDnBY) k_dn_atrous_lds(const typename Vec4T<R>::type* __restrict__ Cin, typename Vec4T<R>::type* __restrict__ Cout,
                                                                const typename Vec4T<R>::type* __restrict__ G, const typename Vec4T<R>::type* __restrict__ P, DnParams<R> k) {
  using V4 = typename Vec4T<R>::type;
  constexpr int HALO = 2 * S, TW = kDnBX + 2 * HALO, TH = kDnBY + 2 * HALO;
  static_assert((size_t)TW * TH * 2 * sizeof(V4) <= 64 * 1024, "tile exceeds a workgroup's LDS");
  __shared__ V4 tc[TW * TH];
  __shared__ V4 tg[TW * TH];
  const int tid = threadIdx.y * kDnBX + threadIdx.x;
  const int x0 = blockIdx.x * kDnBX - HALO, y0 = blockIdx.y * kDnBY - HALO;
  for (int t = tid; t < TW * TH; t += kDnBX * kDnBY) {
    const int tx = t % TW, ty = t / TW, gx = x0 + tx, gy = y0 + ty;
    V4 c = dn_mk4<V4, R>(R(0), R(0), R(0), R(-1)), g = c;      // outside the frame = no data
    if (gx >= 0 && gx < k.W && gy >= 0 && gy < k.H) {
      const size_t q = (size_t)gy * (size_t)k.W + (size_t)gx;
      c = Cin[q];
      if (c.w >= R(0)) g = G[q];
    }
    tc[t] = c; tg[t] = g;
  }
  __syncthreads();
  const int x = blockIdx.x * kDnBX + threadIdx.x, y = blockIdx.y * kDnBY + threadIdx.y;
  if (x >= k.W || y >= k.H) return;
  const size_t i = (size_t)y * (size_t)k.W + (size_t)x;
  const int ct = (threadIdx.y + HALO) * TW + threadIdx.x + HALO;
  const V4 cp = tc[ct];
  if (!(cp.w >= R(0))) { Cout[i] = cp; return; }
  const V4 gp = tg[ct];
  auto fetch = [&](int ox, int oy, V4& cq, V4& gq) -> bool {
    const int t = ct + oy * TW + ox;      // |ox|, |oy| <= 2 S: inside the tile
    cq = tc[t];
    if (!(cq.w >= R(0))) return false;
    gq = tg[t];
    return true;
  };
  auto fetch_s = [&](int dx, int dy, V4& cq, V4& gq) -> bool { return fetch(S * dx, S * dy, cq, gq); };
  Cout[i] = dn_filter_pixel<R, S>(cp, gp, P[i].w, k, fetch, fetch_s);
}

// A third form was measured and not kept: a workgroup taking 32 x 8 pixels of ONE sub-lattice ((x mod S, y mod S) fixed), on which the step-S taps are
// a step-1 5 x 5 with a 2-point halo (36 x 12 records at any S). Its tile loads and stores are strided by S records and the step-1 variance prefilter
// is not in the tile; at 1024^2 in fp32 it took 201 / 470 / 415 / 372 us at S = 4 / 8 / 16 / 32 against 66 / 67 / 81 / 109 us of the direct gathers,
// whose taps are whole 512-byte rows.

}  // namespace rrtd
