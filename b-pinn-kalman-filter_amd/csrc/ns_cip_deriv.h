// Derivative pieces of one CIP site, shared by the adjoint (ns_step_vjp.hip) and the
// tangent-linear model (ns_step_jvp.hip) of the Navier-Stokes step: the weights
// d out / d (gathered value), the local derivatives d out / d (X, Y), the site loop and its
// grid.  One copy of the formulas, so a site takes the same weights in both directions.  On
// top of ns_common.h (Geo, clampx, sgn, CipVals / cip_gather, the argument checks), which the
// forward shares.
//
// Plain float32 with FMA contraction; none of the forward's exact-division machinery.
#pragma once
#include <algorithm>

#include "ns_common.h"

namespace {

struct VjpConst {
  float dt, dx, r1, r2, r3;  // 1/dx, 1/dx^2, 1/dx^3
  __device__ VjpConst(float dt_, float dx_) : dt(dt_), dx(dx_) {
    r1 = 1.0f / dx;
    r2 = r1 * r1;
    r3 = r2 * r1;
  }
};

// One thread per site, x fastest: blockIdx.y walks the planes and blockIdx.x the sites of a
// plane, so no thread pays a 64-bit division to find its plane.  Closes with one brace.
#define NS_VJP_SITES(planes)                                                      \
  for (int64_t b = blockIdx.y; b < (planes); b += gridDim.y)                      \
    for (int s = blockIdx.x * blockDim.x + threadIdx.x; s < (int)g.hw;            \
         s += gridDim.x * blockDim.x)

// grid of NS_VJP_SITES: x over the sites of a plane, y over the planes
inline dim3 grid_for(int64_t planes, const Geo& g) {
  return dim3((unsigned)std::min<int64_t>(bpk::ceil_div(g.hw, 256), 1 << 20),
              (unsigned)std::min<int64_t>(planes, 65535));
}

// d out / d (gathered value) of one CIP site, from the site's velocity alone: one weight per
// gathered value
using CipW = CipVals;

// out = a X^3 + c X^2 Y + e X^2 + g X Y + fx_c X + b Y^3 + d X Y^2 + f Y^2 + fy_c Y + f_c
// with (ns_step.hip cip_site_fast; 1/s = s for s = +-1)
//   a = (sx (fx_xm + fx_c) dx + 2 tmp2) sx / dx^3     b = (sy (fy_ym + fy_c) dx + 2 tmp3) sy / dx^3
//   c = (-tmp1 - sx (fx_ym - fx_c) dx) sy / dx^3      d = (-tmp1 - sy (fy_xm - fy_c) dx) sx / dx^3
//   e = (3 tmp2 + sx (fx_xm + 2 fx_c) dx) / dx^2      f = (3 tmp3 + sy (fy_ym + 2 fy_c) dx) / dx^2
//   g = (-(fy_xm - fy_c) + c dx^2) sx / dx
//   tmp1 = f_c - f_ym - f_xm + f_xy,  tmp2 = f_xm - f_c,  tmp3 = f_ym - f_c
__device__ inline CipW cip_weights(float u, float v, int sxi, int syi, const VjpConst& k) {
  const float sx = (float)sxi, sy = (float)syi;
  const float X = -u * k.dt, Y = -v * k.dt;
  const float XY = X * Y;
  const float wg = XY;                                  // d out / d g
  const float wa = X * X * X * sx * k.r3;               // cotangent of a's numerator
  const float wb = Y * Y * Y * sy * k.r3;
  const float wc = (X * XY + wg * k.dx * sx) * sy * k.r3;  // c feeds g as well
  const float wd = XY * Y * sx * k.r3;
  const float we = X * X * k.r2;
  const float wf = Y * Y * k.r2;
  const float t1 = -(wc + wd);
  const float t2 = 2.0f * wa + 3.0f * we;
  const float t3 = 2.0f * wb + 3.0f * wf;
  const float gs = wg * sx * k.r1;
  const float sxd = sx * k.dx, syd = sy * k.dx;
  CipW w;
  w.f_c = 1.0f + t1 - t2 - t3;
  w.f_xm = t2 - t1;
  w.f_ym = t3 - t1;
  w.f_xy = t1;
  w.fx_xm = sxd * (wa + we);
  w.fx_c = sxd * (wa + wc + 2.0f * we) + X;
  w.fx_ym = -sxd * wc;
  w.fy_ym = syd * (wb + wf);
  w.fy_c = syd * (wb + wd + 2.0f * wf) + Y + gs;
  w.fy_xm = -syd * wd - gs;
  return w;
}

// sum_role W_role q_role in a fixed order: the site's value for q = its gathered values, its
// tangent for q = the gathered tangents
__device__ inline float cip_dot(const CipW& w, const CipVals& q) {
  float r = w.f_c * q.f_c;
  r += w.f_xm * q.f_xm;
  r += w.f_ym * q.f_ym;
  r += w.f_xy * q.f_xy;
  r += w.fx_c * q.fx_c;
  r += w.fx_xm * q.fx_xm;
  r += w.fx_ym * q.fx_ym;
  r += w.fy_c * q.fy_c;
  r += w.fy_xm * q.fy_xm;
  r += w.fy_ym * q.fy_ym;
  return r;
}

// (d out / dX, d out / dY) of one CIP site from its ten gathered values
__device__ inline void cip_dxy_vals(const CipVals& q, float u, float v, int sxi, int syi,
                                    const VjpConst& k, float* dX, float* dY) {
  const float sx = (float)sxi, sy = (float)syi;
  const float f_c = q.f_c, f_xm = q.f_xm, f_ym = q.f_ym, f_xy = q.f_xy;
  const float fx_c = q.fx_c, fx_xm = q.fx_xm, fx_ym = q.fx_ym;
  const float fy_c = q.fy_c, fy_xm = q.fy_xm, fy_ym = q.fy_ym;
  const float tmp1 = f_c - f_ym - f_xm + f_xy;
  const float tmp2 = f_xm - f_c, tmp3 = f_ym - f_c;
  const float a = (sx * (fx_xm + fx_c) * k.dx + 2.0f * tmp2) * sx * k.r3;
  const float b = (sy * (fy_ym + fy_c) * k.dx + 2.0f * tmp3) * sy * k.r3;
  const float cc = (-tmp1 - sx * (fx_ym - fx_c) * k.dx) * sy * k.r3;
  const float d = (-tmp1 - sy * (fy_xm - fy_c) * k.dx) * sx * k.r3;
  const float e = (3.0f * tmp2 + sx * (fx_xm + 2.0f * fx_c) * k.dx) * k.r2;
  const float ff = (3.0f * tmp3 + sy * (fy_ym + 2.0f * fy_c) * k.dx) * k.r2;
  const float gg = (-(fy_xm - fy_c) + cc * k.dx * k.dx) * sx * k.r1;
  const float X = -u * k.dt, Y = -v * k.dt;
  *dX = (3.0f * a * X + 2.0f * cc * Y + 2.0f * e) * X + (gg + d * Y) * Y + fx_c;
  *dY = (3.0f * b * Y + 2.0f * d * X + 2.0f * ff) * Y + (gg + cc * X) * X + fy_c;
}

__device__ inline void cip_dxy(const float* __restrict__ f, const float* __restrict__ fx,
                               const float* __restrict__ fy, int x, int y, float u, float v,
                               const Geo& g, const VjpConst& k, float* dX, float* dY) {
  const int sxi = sgn(u), syi = sgn(v);
  const int xm = clampx(x - sxi, g.nx), ym = clampx(y - syi, g.ny);
  cip_dxy_vals(cip_gather(f, fx, fy, x, y, xm, ym, g), u, v, sxi, syi, k, dX, dY);
}

}  // namespace
