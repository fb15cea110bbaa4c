// Tangent-linear model (Jacobian-vector products) of the Navier-Stokes step
// (csrc/ns_step.hip) for gfx950; the forward-mode counterpart of ns_step_vjp.hip.
//
// One step with compat = 0, plane convention f[y * nx + x]:
//   (px, py) = grad p;  un = u - dt px;  vn = v - dt py
//   u1 = CIP(un; un, vn);  v1 = CIP(vn; un, vn)
//   p1 = PRES(p, u1, v1);  d1 = CIP(d; u1, v1)
// Given tangents (t_d, t_(u,v), t_p) at a base state these kernels produce the tangents of
// (d1, (u1, v1), p1).  The derivative is piecewise like the function: sgn(u), sgn(v) and the
// upwind indices xm, ym are constants taken from the base state.
//
// A CIP site is linear in its ten gathered values with the weights cip_weights(u, v, sx, sy)
// and depends on the site's own velocity through X = -u dt, Y = -v dt (cip_dxy), so
//   t_out = sum_role W_role t_gathered_role + dX (-dt t_u) + dY (-dt t_v)
// where the gathered tangents are t_f and the stencil gradient of t_f at the base's upwind
// indices.  Every output site is a pure gather over its own upwind neighbourhood: no atomics,
// no scatter, a fixed summation order (cip_dot, then the dX and the dY term), the same bits
// on every run.  Where the advected field is the advecting velocity itself (the velocity
// stage) both terms carry t_un, t_vn.
//
// Launch structure, after the forward's own:
//  * the velocity stage is an unfused sequence over a workspace (as update_velocity and
//    velocity_stage_vjp): un, vn are recomputed with the forward's own kernels (k_gradient of
//    p, k_vel_update), so a site takes the same branch in the forward, the tangent and the
//    adjoint; t_un / t_vn = t_(u,v) - dt grad t_p (k_veln_jvp); then k_cip_jvp<2, inline>
//    takes the stencil gradients of un, vn, t_un, t_vn inline from those planes (storing
//    them first cost two more launches over 2B planes and 8B planes of workspace, and
//    measured slower);
//  * the pressure and the density tangent share one launch (k_pres_dens_jvp) that takes
//    grad d and grad t_d inline, as k_fused_pres_dens does;
//  * the stand-alone density op keeps the forward's unfused form (stencil gradients of d and
//    t_d from the forward's k_gradient in the workspace, k_cip_jvp<1, stored>).
// A full step is 5 launches.
//
// Plain float32 with FMA contraction; none of the forward's exact-division machinery.
// A velocity component exactly 0 makes the forward non-finite (a reference property); the
// tangent there is unspecified, but sgn = 0 gives xm = x, so every index stays in bounds.
//
// ns_common.h (shared with the forward): Geo, clampx, sgn, CipVals, cip_gather,
// NS_PRES_NEIGHBOURS, NS_GEO_CHECK, NS_HIP_OK, velocity_stage_base.  ns_cip_deriv.h (shared with
// the adjoint): VjpConst, NS_VJP_SITES, grid_for, cip_weights, cip_dot, cip_dxy_vals.
#include "ns_cip_deriv.h"

namespace {

// The stencil of diff_x / diff_y along one axis: central in the interior, one-sided at the two
// borders, loaded at clamped addresses.
__device__ inline float diff1d(const float* f, int64_t stride, int i, int n, float r1) {
  const int lo = max(i - 1, 0), hi = min(i + 1, n - 1);
  const float coef = (i == 0 || i == n - 1) ? r1 : 0.5f * r1;
  return (f[(int64_t)hi * stride] - f[(int64_t)lo * stride]) * coef;
}

// the ten values of a CIP site with the stencil gradient taken inline from the field
__device__ inline CipVals cip_gather_inline(const float* __restrict__ f, int x, int y, int xm,
                                            int ym, const Geo& g, float r1) {
  const float* ry = f + (int64_t)y * g.nx;    // row y
  const float* rym = f + (int64_t)ym * g.nx;  // row ym
  CipVals q;
  q.f_c = ry[x], q.f_xm = ry[xm], q.f_ym = rym[x], q.f_xy = rym[xm];
  q.fx_c = diff1d(ry, 1, x, g.nx, r1);
  q.fx_xm = diff1d(ry, 1, xm, g.nx, r1);
  q.fx_ym = diff1d(rym, 1, x, g.nx, r1);
  q.fy_c = diff1d(f + x, g.nx, y, g.ny, r1);
  q.fy_xm = diff1d(f + xm, g.nx, y, g.ny, r1);
  q.fy_ym = diff1d(f + x, g.nx, ym, g.ny, r1);
  return q;
}

// NF fields advected by the same velocity (planes 2b, 2b + 1 of `vel`).  Field j of sample b:
// f[j] + b * fstride, the tangent tf[j] (NULL = zero tangent), the output out[j] + b * ostride.
// tvel (2B planes, optional): tangent of the advecting velocity.  STORED: the stencil
// gradients are read from fx[j] / fy[j] and tfx[j] / tfy[j] (plane stride dstride); otherwise
// they are taken inline from f[j] and tf[j] and those four are not read.
template <int NF>
struct CipJvpArgs {
  const float* f[NF];
  const float* fx[NF];
  const float* fy[NF];
  const float* tf[NF];
  const float* tfx[NF];
  const float* tfy[NF];
  float* out[NF];
  int64_t fstride, dstride, ostride;
  const float* vel;
  const float* tvel;
};

template <int NF, bool STORED>
__global__ __launch_bounds__(256) void k_cip_jvp(CipJvpArgs<NF> a, int B, Geo g, float dt,
                                                 float dx) {
  const VjpConst k(dt, dx);
  auto gather = [&](const float* f, const float* fx, const float* fy, int64_t b, int x, int y,
                    int xm, int ym) {
    if constexpr (STORED)
      return cip_gather(f + b * a.fstride, fx + b * a.dstride, fy + b * a.dstride, x, y, xm, ym,
                        g);
    else
      return cip_gather_inline(f + b * a.fstride, x, y, xm, ym, g, k.r1);
  };
  NS_VJP_SITES(B) {
    const int y = s / g.nx, x = s - y * g.nx;
    const float u = a.vel[(2 * b) * g.hw + s];
    const float v = a.vel[(2 * b + 1) * g.hw + s];
    const int sx = sgn(u), sy = sgn(v);
    const int xm = clampx(x - sx, g.nx), ym = clampx(y - sy, g.ny);
    float mtu = 0.f, mtv = 0.f;  // tangents of X, Y
    if (a.tvel) {
      mtu = -dt * a.tvel[(2 * b) * g.hw + s];
      mtv = -dt * a.tvel[(2 * b + 1) * g.hw + s];
    }
    const CipW w = cip_weights(u, v, sx, sy, k);
#pragma unroll
    for (int j = 0; j < NF; ++j) {
      float r = 0.f;
      if (a.tf[j]) r = cip_dot(w, gather(a.tf[j], a.tfx[j], a.tfy[j], b, x, y, xm, ym));
      if (a.tvel) {
        float dX, dY;
        cip_dxy_vals(gather(a.f[j], a.fx[j], a.fy[j], b, x, y, xm, ym), u, v, sx, sy, k, &dX,
                     &dY);
        r += dX * mtu;
        r += dY * mtv;
      }
      a.out[j][b * a.ostride + s] = r;
    }
  }
}

// t_un = t_u - dt d/dx t_p, t_vn = t_v - dt d/dy t_p over B samples (2B output planes);
// tvel, tpres optional (NULL = zero).
__global__ __launch_bounds__(256) void k_veln_jvp(const float* __restrict__ tvel,
                                                  const float* __restrict__ tpres,
                                                  float* __restrict__ tveln, int B, Geo g,
                                                  float dt, float dx) {
  const float r1 = 1.0f / dx;
  NS_VJP_SITES(B) {
    const int y = s / g.nx, x = s - y * g.nx;
    float tu = 0.f, tv = 0.f;
    if (tvel) {
      tu = tvel[(2 * b) * g.hw + s];
      tv = tvel[(2 * b + 1) * g.hw + s];
    }
    if (tpres) {
      const float* tp = tpres + b * g.hw;
      tu -= dt * diff1d(tp + (int64_t)y * g.nx, 1, x, g.nx, r1);
      tv -= dt * diff1d(tp + x, g.nx, y, g.ny, r1);
    }
    tveln[(2 * b) * g.hw + s] = tu;
    tveln[(2 * b + 1) * g.hw + s] = tv;
  }
}

// Tangents of p1 = PRES(p, u1, v1) and d1 = CIP(d; u1, v1) in one launch.  vel1: the base
// (u1, v1); tvel1, tpres, tdens: tangents, each optional (NULL = zero).  t_p1 / t_d1: outputs,
// each optional (dens may be NULL when t_d1 is).
//   t_p1 = avg4(t_p) + (2 sxx t_sxx + 2 syy t_syy + syx t_sxy + sxy t_syx) / 8
//          - dx (t_sxx + t_syy) / (8 dt),   the t_s the mirrored differences of (t_u1, t_v1)
__global__ __launch_bounds__(256) void k_pres_dens_jvp(const float* __restrict__ dens,
                                                       const float* __restrict__ vel1,
                                                       const float* __restrict__ tdens,
                                                       const float* __restrict__ tvel1,
                                                       const float* __restrict__ tpres,
                                                       float* __restrict__ t_d1,
                                                       float* __restrict__ t_p1, int B, Geo g,
                                                       float dt, float dx) {
  const VjpConst k(dt, dx);
  const float kk = dx / (8.0f * dt);
  NS_VJP_SITES(B) {
    const int y = s / g.nx, x = s - y * g.nx;
    const float* u = vel1 + (2 * b) * g.hw;
    const float* v = vel1 + (2 * b + 1) * g.hw;
    const float* tu = tvel1 ? tvel1 + (2 * b) * g.hw : nullptr;
    const float* tv = tvel1 ? tvel1 + (2 * b + 1) * g.hw : nullptr;
    if (t_p1) {
      NS_PRES_NEIGHBOURS(x, y, g);
      float r = 0.f;
      if (tpres) {
        const float* tp = tpres + b * g.hw;
        r = 0.25f * (tp[ixd] + tp[ixu] + tp[iyd] + tp[iyu]);
      }
      if (tvel1) {
        const float sxx = u[ixu] - u[ixd], sxy = v[ixu] - v[ixd];
        const float syx = u[iyu] - u[iyd], syy = v[iyu] - v[iyd];
        const float tsxx = tu[ixu] - tu[ixd], tsxy = tv[ixu] - tv[ixd];
        const float tsyx = tu[iyu] - tu[iyd], tsyy = tv[iyu] - tv[iyd];
        float q = 2.0f * sxx * tsxx;
        q += 2.0f * syy * tsyy;
        q += syx * tsxy;
        q += sxy * tsyx;
        r += 0.125f * q;
        r -= kk * (tsxx + tsyy);
      }
      t_p1[b * g.hw + s] = r;
    }
    if (t_d1) {
      const float uc = u[s], vc = v[s];
      const int sx = sgn(uc), sy = sgn(vc);
      const int xm = clampx(x - sx, g.nx), ym = clampx(y - sy, g.ny);
      float r = 0.f;
      if (tdens)
        r = cip_dot(cip_weights(uc, vc, sx, sy, k),
                    cip_gather_inline(tdens + b * g.hw, x, y, xm, ym, g, k.r1));
      if (tvel1) {
        float dX, dY;
        cip_dxy_vals(cip_gather_inline(dens + b * g.hw, x, y, xm, ym, g, k.r1), uc, vc, sx, sy,
                     k, &dX, &dY);
        r += dX * (-dt * tu[s]);
        r += dY * (-dt * tv[s]);
      }
      t_d1[b * g.hw + s] = r;
    }
  }
}

int launch_pres_dens_jvp(const float* dens, const float* vel1, const float* tdens,
                         const float* tvel1, const float* tpres, float* t_d1, float* t_p1, int B,
                         const Geo& g, float dt, float dx, hipStream_t st, const char* what) {
  hipLaunchKernelGGL(k_pres_dens_jvp, grid_for(B, g), dim3(256), 0, st, dens, vel1, tdens, tvel1,
                     tpres, t_d1, t_p1, B, g, dt, dx);
  BPK_LAUNCH_CHECK(what);
  return BPK_OK;
}

// Tangent of the velocity stage: t_out (2B planes) from t_vel and t_pres (each optional, at
// least one).  ws: 6 * B planes.
int velocity_stage_jvp(const float* vel, const float* pres, const float* t_vel,
                       const float* t_pres, float* t_out, float* ws, int B, const Geo& g,
                       float dt, float dx, void* stream) {
  const int64_t hw = g.hw, P = (int64_t)B * hw;
  hipStream_t st = bpk::as_stream(stream);
  float* vel_n;                // first 4B planes: velocity_stage_base
  float* tvel_n = ws + 4 * P;  // 2B planes: tangent of vel_n
  int rc = velocity_stage_base(vel, pres, ws, &vel_n, B, g, dt, dx, stream);
  if (rc) return rc;
  hipLaunchKernelGGL(k_veln_jvp, grid_for(B, g), dim3(256), 0, st, t_vel, t_pres, tvel_n, B, g,
                     dt, dx);
  BPK_LAUNCH_CHECK("ns_update_velocity_jvp(vel_n)");
  CipJvpArgs<2> a;
  for (int j = 0; j < 2; ++j) {
    a.f[j] = vel_n + j * hw;
    a.tf[j] = tvel_n + j * hw;
    a.fx[j] = a.fy[j] = a.tfx[j] = a.tfy[j] = nullptr;  // inline
    a.out[j] = t_out + j * hw;
  }
  a.fstride = a.dstride = a.ostride = 2 * hw;
  a.vel = vel_n;
  a.tvel = tvel_n;
  hipLaunchKernelGGL((k_cip_jvp<2, false>), grid_for(B, g), dim3(256), 0, st, a, B, g, dt, dx);
  BPK_LAUNCH_CHECK("ns_update_velocity_jvp(cip)");
  return BPK_OK;
}

}  // namespace

extern "C" int64_t bpk_ns_jvp_workspace_bytes(int op, int B, int nx, int ny) {
  const int64_t plane = (int64_t)nx * ny * (int64_t)sizeof(float);
  if (B <= 0 || nx <= 0 || ny <= 0) return 0;
  switch (op) {
    case 0: return 4 * B * plane;   // density: fx, fy, t_fx, t_fy
    case 1: return 6 * B * plane;   // velocity stage: px, py, vel_n, t_vel_n
    case 3: return 6 * B * plane;   // full step: the velocity stage's
    default: return 0;              // pressure: none
  }
}

extern "C" int bpk_ns_update_density_jvp_f32(const float* dens, const float* vel,
                                             const float* t_dens, const float* t_vel,
                                             float* t_out, void* workspace, int B, int nx, int ny,
                                             float dt, float dx, void* stream) {
  NS_GEO_CHECK("ns_step jvp", B, nx, ny);
  if (B == 0) return BPK_OK;
  BPK_REQUIRE(dens && vel && t_out, "ns_update_density_jvp: dens, vel and t_out required");
  BPK_REQUIRE(t_dens || t_vel, "ns_update_density_jvp: no tangent given");
  BPK_REQUIRE(workspace, "ns_update_density_jvp: workspace required");
  const Geo g{nx, ny, (int64_t)nx * ny};
  const int64_t P = (int64_t)B * g.hw;
  float* ws = static_cast<float*>(workspace);
  float *fx = ws, *fy = ws + P, *tfx = ws + 2 * P, *tfy = ws + 3 * P;
  int rc;
  if (t_vel) {  // the base's gradient enters through d out / d (X, Y) only
    rc = bpk_ns_gradient_f32(dens, g.hw, fx, fy, B, nx, ny, dx, stream);
    if (rc) return rc;
  }
  if (t_dens) {
    rc = bpk_ns_gradient_f32(t_dens, g.hw, tfx, tfy, B, nx, ny, dx, stream);
    if (rc) return rc;
  }
  CipJvpArgs<1> a;
  a.f[0] = dens;
  a.fx[0] = fx;
  a.fy[0] = fy;
  a.tf[0] = t_dens;
  a.tfx[0] = tfx;
  a.tfy[0] = tfy;
  a.out[0] = t_out;
  a.fstride = a.dstride = a.ostride = g.hw;
  a.vel = vel;
  a.tvel = t_vel;
  hipLaunchKernelGGL((k_cip_jvp<1, true>), grid_for(B, g), dim3(256), 0, bpk::as_stream(stream),
                     a, B, g, dt, dx);
  BPK_LAUNCH_CHECK("ns_update_density_jvp");
  return BPK_OK;
}

extern "C" int bpk_ns_update_velocity_jvp_f32(const float* vel, const float* pres,
                                              const float* t_vel, const float* t_pres,
                                              float* t_out, void* workspace, int B, int nx,
                                              int ny, float dt, float dx, void* stream) {
  NS_GEO_CHECK("ns_step jvp", B, nx, ny);
  if (B == 0) return BPK_OK;
  BPK_REQUIRE(vel && pres && t_out, "ns_update_velocity_jvp: vel, pres and t_out required");
  BPK_REQUIRE(t_vel || t_pres, "ns_update_velocity_jvp: no tangent given");
  BPK_REQUIRE(workspace, "ns_update_velocity_jvp: workspace required");
  const Geo g{nx, ny, (int64_t)nx * ny};
  return velocity_stage_jvp(vel, pres, t_vel, t_pres, t_out, static_cast<float*>(workspace), B, g,
                            dt, dx, stream);
}

extern "C" int bpk_ns_update_pressure_jvp_f32(const float* vel, const float* t_pres,
                                              const float* t_vel, float* t_out, int B, int nx,
                                              int ny, float dt, float dx, void* stream) {
  NS_GEO_CHECK("ns_step jvp", B, nx, ny);
  if (B == 0) return BPK_OK;
  BPK_REQUIRE(vel && t_out, "ns_update_pressure_jvp: vel and t_out required");
  BPK_REQUIRE(t_pres || t_vel, "ns_update_pressure_jvp: no tangent given");
  const Geo g{nx, ny, (int64_t)nx * ny};
  return launch_pres_dens_jvp(nullptr, vel, nullptr, t_vel, t_pres, nullptr, t_out, B, g, dt, dx,
                              bpk::as_stream(stream), "ns_update_pressure_jvp");
}

extern "C" int bpk_ns_full_step_jvp_f32(const float* dens, const float* vel, const float* pres,
                                        const float* vel1, const float* t_dens,
                                        const float* t_vel, const float* t_pres, float* t_dens1,
                                        float* t_vel1, float* t_pres1, void* workspace, int B,
                                        int nx, int ny, float dt, float dx, void* stream) {
  NS_GEO_CHECK("ns_step jvp", B, nx, ny);
  if (B == 0) return BPK_OK;
  BPK_REQUIRE(dens && vel && pres && vel1, "ns_full_step_jvp: dens, vel, pres and vel1 required");
  BPK_REQUIRE(t_dens || t_vel || t_pres, "ns_full_step_jvp: no tangent given");
  BPK_REQUIRE(t_dens1 && t_vel1 && t_pres1,
              "ns_full_step_jvp: t_dens1, t_vel1 and t_pres1 required");
  BPK_REQUIRE(workspace, "ns_full_step_jvp: workspace required");
  const Geo g{nx, ny, (int64_t)nx * ny};
  const int64_t P = (int64_t)B * g.hw;
  hipStream_t st = bpk::as_stream(stream);
  // (u1, v1) depend on (u, v) and p only: with the density tangent alone their tangent is 0
  const bool moves = t_vel || t_pres;
  if (moves) {
    int rc = velocity_stage_jvp(vel, pres, t_vel, t_pres, t_vel1, static_cast<float*>(workspace),
                                B, g, dt, dx, stream);
    if (rc) return rc;
  } else {
    NS_HIP_OK(hipMemsetAsync(t_vel1, 0, 2 * P * sizeof(float), st), "ns_full_step_jvp");
  }
  return launch_pres_dens_jvp(dens, vel1, t_dens, moves ? t_vel1 : nullptr, t_pres, t_dens1,
                              t_pres1, B, g, dt, dx, st, "ns_full_step_jvp(pressure+density)");
}
