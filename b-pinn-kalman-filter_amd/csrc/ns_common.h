// Pieces of the Navier-Stokes step shared by the forward (ns_step.hip), its adjoint
// (ns_step_vjp.hip) and its tangent-linear model (ns_step_jvp.hip): the plane geometry, the
// mirror clamp, the sign, the ten gathered values of a CIP site, the mirrored neighbours of
// the pressure update, the argument checks of every bpk_ns_* entry and the velocity stage's
// base recomputation.  One copy, so a site takes the same branch in all three.
//
// Integer logic, structs and pure loads only: ns_step.hip turns FMA contraction off after its
// includes (its bit-exactness against the C oracle rests on that), and code in a header is
// compiled with contraction on, so no floating-point arithmetic the forward uses lives here.
#pragma once
#include <climits>

#include "bpk_common.h"

namespace {

struct Geo {
  int nx, ny;
  int64_t hw;
};

__device__ inline int clampx(int x, int n) { return x < 0 ? -x : (x > n - 1 ? 2 * n - 2 - x : x); }

__device__ inline int sgn(float v) { return v < 0.0f ? -1 : (v > 0.0f ? 1 : 0); }

// the ten gathered values of one CIP site (op/ns_step_kernel.cu:115-158)
struct CipVals {
  float f_c, f_xm, f_ym, f_xy;  // f(x,y) f(xm,y) f(x,ym) f(xm,ym)
  float fx_c, fx_xm, fx_ym;     // fx(x,y) fx(xm,y) fx(x,ym)
  float fy_c, fy_xm, fy_ym;     // fy(x,y) fy(xm,y) fy(x,ym)
};

// the ten values of site (x, y) with upwind indices (xm, ym) from a field and its stored
// stencil gradient
__device__ inline CipVals cip_gather(const float* __restrict__ f, const float* __restrict__ fx,
                                     const float* __restrict__ fy, int x, int y, int xm, int ym,
                                     const Geo& g) {
  const int64_t c = (int64_t)y * g.nx + x, cxm = (int64_t)y * g.nx + xm,
                cym = (int64_t)ym * g.nx + x, cxy = (int64_t)ym * g.nx + xm;
  CipVals q;
  q.f_c = f[c], q.f_xm = f[cxm], q.f_ym = f[cym], q.f_xy = f[cxy];
  q.fx_c = fx[c], q.fx_xm = fx[cxm], q.fx_ym = fx[cym];
  q.fy_c = fy[c], q.fy_xm = fy[cxm], q.fy_ym = fy[cym];
  return q;
}

// The mirrored neighbours xu, xd, yu, yd of site (x, y) that the pressure update reads
// (op/ns_step_kernel.cu:205-234) and their in-plane indices ixu, ixd, iyu, iyd, declared in the
// caller's scope.  A macro (like NS_VJP_SITES) so that the statements reach every kernel as
// written: behind a function call the compiler folds the mirror before it inlines, and the
// fused forward and tangent kernels come out with other instructions and register counts.
#define NS_PRES_NEIGHBOURS(x, y, g)                                                  \
  const int xu = clampx((x) + 1, (g).nx), xd = clampx((x) - 1, (g).nx);              \
  const int yu = clampx((y) + 1, (g).ny), yd = clampx((y) - 1, (g).ny);              \
  const int64_t ixu = (int64_t)(y) * (g).nx + xu, ixd = (int64_t)(y) * (g).nx + xd,  \
                iyu = (int64_t)yu * (g).nx + (x), iyd = (int64_t)yd * (g).nx + (x)

// Every bpk_ns_* entry, before it touches a pointer or the device.  A site's in-plane index is
// an int in every kernel, hence the bound on nx * ny.  family: "ns_step", "ns_step vjp", ...
#define NS_GEO_CHECK(family, B, nx, ny)                                                       \
  do {                                                                                        \
    BPK_REQUIRE((B) >= 0 && (nx) >= 2 && (ny) >= 2, family ": need B >= 0 and planes >= 2x2 "  \
                                                           "(got B=%d nx=%d ny=%d)",          \
                (B), (nx), (ny));                                                             \
    BPK_REQUIRE((int64_t)(nx) * (ny) <= INT_MAX, family ": planes of at most 2^31 - 1 sites "  \
                                                        "(got nx=%d ny=%d)",                  \
                (nx), (ny));                                                                  \
  } while (0)

#define NS_HIP_OK(expr, what)                                                \
  do {                                                                       \
    hipError_t e_ = (expr);                                                  \
    if (e_ != hipSuccess) {                                                  \
      bpk::set_error("%s: %s", what, hipGetErrorString(e_));                 \
      return BPK_ERR_LAUNCH;                                                 \
    }                                                                        \
  } while (0)

// Base recomputation of the velocity stage into the first 4 * B planes of ws: (px, py) =
// grad p (B planes each), then vel_n = vel - dt (px, py) (2B planes, returned in *vel_n).
// The forward's own kernels, so update_velocity, the tangent and the adjoint see the same
// bits, hence the same signs, as the fused forward.
inline int velocity_stage_base(const float* vel, const float* pres, float* ws, float** vel_n,
                               int B, const Geo& g, float dt, float dx, void* stream) {
  const int64_t P = (int64_t)B * g.hw;
  float *px = ws, *py = ws + P;
  *vel_n = ws + 2 * P;
  int rc = bpk_ns_gradient_f32(pres, g.hw, px, py, B, g.nx, g.ny, dx, stream);
  if (rc) return rc;
  return bpk_ns_vel_update_f32(vel, px, py, *vel_n, B, g.nx, g.ny, dt, stream);
}

}  // namespace
