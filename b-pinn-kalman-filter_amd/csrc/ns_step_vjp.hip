// Vector-Jacobian products of the Navier-Stokes step (csrc/ns_step.hip) for gfx950.
//
// One step with compat = 0, plane convention f[y * nx + x]:
//   (px, py) = grad p;  un = u - dt px;  vn = v - dt py
//   u1 = CIP(un; un, vn);  v1 = CIP(vn; un, vn)
//   p1 = PRES(p, u1, v1);  d1 = CIP(d; u1, v1)
// Given cotangents of (d1, (u1, v1), p1) these kernels produce the gradients of
// (d, (u, v), p).  The derivative is piecewise like the function: sgn(u), sgn(v) and the
// upwind indices xm, ym are constants.
//
// A CIP site is linear in its ten gathered values (CipVals of ns_common.h) with weights that
// are polynomials in X = -u dt, Y = -v dt, dx and the two signs of the site's own velocity.
// The adjoint with respect to f, fx, fy is therefore a gather: site s walks its 3x3
// neighbourhood, recomputes each neighbour t's signs, mirrored xm / ym and weights from t's
// velocity alone and adds g_out[t] * W_role(t) for every role (c, xm, ym, xmym) in which t
// read s.  The clamp is a mirror (x = 0 with sgn = +1 reads x = 1), so |xm - x| = 1 for
// n >= 2 and the 3x3 window is exact at the borders.  No atomics, no scatter, a fixed
// summation order: the same bits on every run.  The field's total gradient is
// g_f + grad^T (g_fx, g_fy), the second term through the adjoint stencil (k_grad_vjp).
//
// Plain float32 with FMA contraction; none of the forward's exact-division machinery.
// A velocity component exactly 0 makes the forward non-finite (a reference property); the
// backward there is unspecified, but sgn = 0 gives xm = x, so every index stays in bounds.
//
// ns_common.h (shared with the forward): Geo, clampx, sgn, CipVals, cip_gather, NS_GEO_CHECK,
// NS_HIP_OK, velocity_stage_base.  ns_cip_deriv.h (shared with the tangent): VjpConst,
// NS_VJP_SITES, grid_for, cip_weights, cip_dxy.
#include "ns_cip_deriv.h"

namespace {

// NF fields advected by the same velocity (planes 2b, 2b + 1 of `vel`).  Field j of sample b:
// f[j] + b * fstride, its stencil gradient fx[j] / fy[j] and the outputs gf[j] / gfx[j] /
// gfy[j] at plane stride ostride, the cotangent gout[j] at plane stride gstride.
// gf / gfx / gfy (all or none): the gather adjoint.  gvel_out (2B planes, optional):
// gvel_in (optional) + the local -dt g_out d out/d(X, Y) terms of all NF fields.
template <int NF>
struct CipVjpArgs {
  const float* f[NF];
  const float* fx[NF];
  const float* fy[NF];
  const float* gout[NF];
  float* gf[NF];
  float* gfx[NF];
  float* gfy[NF];
  int64_t fstride, dstride, gstride, ostride;
  const float* vel;
  const float* gvel_in;
  float* gvel_out;
};

template <int NF>
__global__ __launch_bounds__(256) void k_cip_vjp(CipVjpArgs<NF> a, int B, Geo g, float dt,
                                                 float dx) {
  const VjpConst k(dt, dx);
  NS_VJP_SITES(B) {
    const int y = s / g.nx, x = s - y * g.nx;
    const float* u = a.vel + (2 * b) * g.hw;
    const float* v = a.vel + (2 * b + 1) * g.hw;
    if (a.gf[0]) {
      float af[NF], afx[NF], afy[NF];
#pragma unroll
      for (int j = 0; j < NF; ++j) af[j] = afx[j] = afy[j] = 0.f;
      // the nine neighbours' velocities and cotangents first (clamped addresses, so every
      // load is in bounds and all of them are in flight together), then the arithmetic
      float ut[9], vt[9], go[NF][9];
#pragma unroll
      for (int n = 0; n < 9; ++n) {
        const int ty = min(max(y + n / 3 - 1, 0), g.ny - 1);
        const int tx = min(max(x + n % 3 - 1, 0), g.nx - 1);
        const int64_t t = (int64_t)ty * g.nx + tx;
        ut[n] = u[t];
        vt[n] = v[t];
#pragma unroll
        for (int j = 0; j < NF; ++j) go[j][n] = a.gout[j][b * a.gstride + t];
      }
#pragma unroll
      for (int n = 0; n < 9; ++n) {
        const int ty = y + n / 3 - 1, tx = x + n % 3 - 1;
        if (ty < 0 || ty >= g.ny || tx < 0 || tx >= g.nx) continue;
        const int sx = sgn(ut[n]), sy = sgn(vt[n]);
        const bool cx = tx == x, cy = ty == y;
        const bool mx = clampx(tx - sx, g.nx) == x, my = clampx(ty - sy, g.ny) == y;
        if (!((cx || mx) && (cy || my))) continue;  // t read nothing at s
        const CipW w = cip_weights(ut[n], vt[n], sx, sy, k);
        float wf = 0.f, wfx = 0.f, wfy = 0.f;
        if (cx && cy) wf += w.f_c, wfx += w.fx_c, wfy += w.fy_c;
        if (mx && cy) wf += w.f_xm, wfx += w.fx_xm, wfy += w.fy_xm;
        if (cx && my) wf += w.f_ym, wfx += w.fx_ym, wfy += w.fy_ym;
        if (mx && my) wf += w.f_xy;
#pragma unroll
        for (int j = 0; j < NF; ++j) {
          af[j] += go[j][n] * wf;
          afx[j] += go[j][n] * wfx;
          afy[j] += go[j][n] * wfy;
        }
      }
#pragma unroll
      for (int j = 0; j < NF; ++j) {
        a.gf[j][b * a.ostride + s] = af[j];
        a.gfx[j][b * a.ostride + s] = afx[j];
        a.gfy[j][b * a.ostride + s] = afy[j];
      }
    }
    if (a.gvel_out) {
      const float uc = u[s], vc = v[s];
      float gu = 0.f, gv = 0.f;
      if (a.gvel_in) {
        gu = a.gvel_in[(2 * b) * g.hw + s];
        gv = a.gvel_in[(2 * b + 1) * g.hw + s];
      }
#pragma unroll
      for (int j = 0; j < NF; ++j) {
        float dX, dY;
        cip_dxy(a.f[j] + b * a.fstride, a.fx[j] + b * a.dstride, a.fy[j] + b * a.dstride, x, y,
                uc, vc, g, k, &dX, &dY);
        const float go = a.gout[j][b * a.gstride + s] * dt;
        gu -= go * dX;
        gv -= go * dY;
      }
      a.gvel_out[(2 * b) * g.hw + s] = gu;
      a.gvel_out[(2 * b + 1) * g.hw + s] = gv;
    }
  }
}

// Gather adjoint of pres_site (ns_step.hip): p1[t] = 0.25 (p[xd] + p[xu] + p[yd] + p[yu])
//   + (sxx^2 + syy^2 + syx sxy) / 8 - dx (sxx + syy) / (8 dt),   sxx = u[xu] - u[xd],
//   sxy = v[xu] - v[xd], syx = u[yu] - u[yd], syy = v[yu] - v[yd] with mirrored indices.
// Site s is read by its row neighbours (through xu / xd) and column neighbours (yu / yd); at a
// border xu == xd, so p counts twice and the velocity difference vanishes.
__global__ __launch_bounds__(256) void k_pres_vjp(const float* __restrict__ vel,
                                                  const float* __restrict__ gout,
                                                  float* __restrict__ gpres,
                                                  const float* __restrict__ gvel_in,
                                                  float* __restrict__ gvel_out, int B, Geo g,
                                                  float dt, float dx) {
  const float kk = dx / (8.0f * dt);
  NS_VJP_SITES(B) {
    const int y = s / g.nx, x = s - y * g.nx;
    const float* u = vel + (2 * b) * g.hw;
    const float* v = vel + (2 * b + 1) * g.hw;
    const float* go = gout + b * g.hw;
    float gp = 0.f, gu = 0.f, gv = 0.f;
    const int yu = clampx(y + 1, g.ny), yd = clampx(y - 1, g.ny);
    const int xu = clampx(x + 1, g.nx), xd = clampx(x - 1, g.nx);
    for (int tx = x - 1; tx <= x + 1; tx += 2) {  // row neighbours t = (tx, y)
      if (tx < 0 || tx >= g.nx) continue;
      const int txu = clampx(tx + 1, g.nx), txd = clampx(tx - 1, g.nx);
      const float G = go[(int64_t)y * g.nx + tx];
      gp += (float)((txu == x) + (txd == x)) * G;
      const int cu = (txu == x) - (txd == x);
      if (gvel_out && cu) {
        const float sxx = u[(int64_t)y * g.nx + txu] - u[(int64_t)y * g.nx + txd];
        const float syx = u[(int64_t)yu * g.nx + tx] - u[(int64_t)yd * g.nx + tx];
        gu += (float)cu * G * (0.25f * sxx - kk);
        gv += (float)cu * G * 0.125f * syx;
      }
    }
    for (int ty = y - 1; ty <= y + 1; ty += 2) {  // column neighbours t = (x, ty)
      if (ty < 0 || ty >= g.ny) continue;
      const int tyu = clampx(ty + 1, g.ny), tyd = clampx(ty - 1, g.ny);
      const float G = go[(int64_t)ty * g.nx + x];
      gp += (float)((tyu == y) + (tyd == y)) * G;
      const int cv = (tyu == y) - (tyd == y);
      if (gvel_out && cv) {
        const float syy = v[(int64_t)tyu * g.nx + x] - v[(int64_t)tyd * g.nx + x];
        const float sxy = v[(int64_t)ty * g.nx + xu] - v[(int64_t)ty * g.nx + xd];
        gv += (float)cv * G * (0.25f * syy - kk);
        gu += (float)cv * G * 0.125f * sxy;
      }
    }
    if (gpres) gpres[b * g.hw + s] = 0.25f * gp;
    if (gvel_out) {
      if (gvel_in) {
        gu += gvel_in[(2 * b) * g.hw + s];
        gv += gvel_in[(2 * b + 1) * g.hw + s];
      }
      gvel_out[(2 * b) * g.hw + s] = gu;
      gvel_out[(2 * b + 1) * g.hw + s] = gv;
    }
  }
}

// (D^T g)[x] for the 1-D difference stencil D of diff_x / diff_y: row j of D reads x = j +- 1
// with +-1/(2dx) in the interior and x = j, j +- 1 with +-1/dx at the two borders (one-sided
// differences).  The three rows that can read x are loaded unconditionally at clamped
// addresses (a zero coefficient where the row does not exist), so the loads do not wait for
// one another.
__device__ inline float adj1d(const float* g, int64_t stride, int x, int n, float r1) {
  const float gm = g[(int64_t)max(x - 1, 0) * stride];
  const float gc = g[(int64_t)x * stride];
  const float gp = g[(int64_t)min(x + 1, n - 1) * stride];
  const float cm = x >= 1 ? (x == 1 ? r1 : 0.5f * r1) : 0.f;          // row x - 1 (row 0: +1/dx)
  const float cc = x == 0 ? -r1 : (x == n - 1 ? r1 : 0.f);            // row x (borders only)
  const float cp = x <= n - 2 ? (x == n - 2 ? -r1 : -0.5f * r1) : 0.f;  // row x + 1 (row n-1: -1/dx)
  return cm * gm + cc * gc + cp * gp;
}

// out[k] = a[k] + c[k] + scale (Dx^T gx[k] + Dy^T gy[k]) over P planes; a, c optional; every
// operand has its own plane stride.  out may alias a or c (each site reads its own element).
// Not k_gradient_adjoint of ns_step.hip: contraction on here, so the two round differently.
__global__ __launch_bounds__(256) void k_grad_vjp(const float* gx, int64_t gxs, const float* gy,
                                                  int64_t gys, const float* a, int64_t as,
                                                  const float* c, int64_t cs, float* out,
                                                  int64_t os, int P, Geo g, float dx,
                                                  float scale) {
  const float r1 = 1.0f / dx;
  NS_VJP_SITES(P) {
    const int y = s / g.nx, x = s - y * g.nx;
    const float* rx = gx + b * gxs + (int64_t)y * g.nx;  // row y of gx, stride 1 in x
    const float* cy = gy + b * gys + x;                   // column x of gy, stride nx in y
    float r = scale * (adj1d(rx, 1, x, g.nx, r1) + adj1d(cy, g.nx, y, g.ny, r1));
    if (a) r += a[b * as + s];
    if (c) r += c[b * cs + s];
    out[b * os + s] = r;
  }
}

int launch_grad_vjp(const float* gx, int64_t gxs, const float* gy, int64_t gys, const float* a,
                    int64_t as, const float* c, int64_t cs, float* out, int64_t os, int P,
                    const Geo& g, float dx, float scale, hipStream_t st) {
  hipLaunchKernelGGL(k_grad_vjp, grid_for(P, g), dim3(256), 0, st, gx, gxs, gy, gys, a,
                     as, c, cs, out, os, P, g, dx, scale);
  BPK_LAUNCH_CHECK("ns_gradient_vjp");
  return BPK_OK;
}

// Backward of the velocity stage: given G = cotangent of (u1, v1) (2B planes), writes
// g_vel (2B planes) and g_pres = gp_base (optional, may alias g_pres) - dt grad^T g_vel.
// ws: 16 * B planes.
int velocity_stage_vjp(const float* vel, const float* pres, const float* G, float* g_vel,
                       float* g_pres, const float* gp_base, float* ws, int B, const Geo& g,
                       float dt, float dx, void* stream) {
  const int64_t hw = g.hw, P = (int64_t)B * hw;
  hipStream_t st = bpk::as_stream(stream);
  float* vel_n;                // first 4B planes: velocity_stage_base
  float* dfx = ws + 4 * P;     // 2B planes: d/dx of plane k of vel_n
  float* dfy = ws + 6 * P;
  float* H = ws + 8 * P;       // 2B planes: local terms
  float* gf = ws + 10 * P;     // 2B planes each
  float* gfx = ws + 12 * P;
  float* gfy = ws + 14 * P;
  // un, vn and their stencil gradients, with the forward's own kernels
  int rc = velocity_stage_base(vel, pres, ws, &vel_n, B, g, dt, dx, stream);
  if (rc) return rc;
  rc = bpk_ns_gradient_f32(vel_n, hw, dfx, dfy, 2 * B, g.nx, g.ny, dx, stream);
  if (rc) return rc;
  CipVjpArgs<2> a;
  for (int j = 0; j < 2; ++j) {
    a.f[j] = vel_n + j * hw;
    a.fx[j] = dfx + j * hw;
    a.fy[j] = dfy + j * hw;
    a.gout[j] = G + j * hw;
    a.gf[j] = gf + j * hw;
    a.gfx[j] = gfx + j * hw;
    a.gfy[j] = gfy + j * hw;
  }
  a.fstride = a.dstride = a.gstride = a.ostride = 2 * hw;
  a.vel = vel_n;
  a.gvel_in = nullptr;
  a.gvel_out = H;
  hipLaunchKernelGGL(k_cip_vjp<2>, grid_for(B, g), dim3(256), 0, st, a, B, g, dt, dx);
  BPK_LAUNCH_CHECK("ns_update_velocity_vjp(cip)");
  // g_un = g_f + local + grad^T (g_fx, g_fy) per plane; g_u = g_un, g_v = g_vn
  rc = launch_grad_vjp(gfx, hw, gfy, hw, gf, hw, H, hw, g_vel, hw, 2 * B, g, dx, 1.0f, st);
  if (rc) return rc;
  if (g_pres)  // un = u - dt px: g_p -= dt grad^T (g_un, g_vn)
    rc = launch_grad_vjp(g_vel, 2 * hw, g_vel + hw, 2 * hw, gp_base, hw, nullptr, 0, g_pres, hw,
                         B, g, dx, -dt, st);
  return rc;
}

}  // namespace

extern "C" int64_t bpk_ns_vjp_workspace_bytes(int op, int B, int nx, int ny) {
  const int64_t plane = (int64_t)nx * ny * (int64_t)sizeof(float);
  if (B <= 0 || nx <= 0 || ny <= 0) return 0;
  switch (op) {
    case 0: return 5 * B * plane;   // density: fx, fy, g_f, g_fx, g_fy
    case 1: return 16 * B * plane;  // velocity stage
    case 3: return 18 * B * plane;  // full step: velocity stage + cotangent of (u1, v1)
    default: return 0;              // pressure: none
  }
}

extern "C" int bpk_ns_gradient_vjp_f32(const float* gx, const float* gy, const float* base,
                                       float* out, int B, int nx, int ny, float dx, float scale,
                                       void* stream) {
  NS_GEO_CHECK("ns_step vjp", B, nx, ny);
  if (B == 0) return BPK_OK;
  BPK_REQUIRE(gx && gy && out, "ns_gradient_vjp: gx, gy and out required");
  const Geo g{nx, ny, (int64_t)nx * ny};
  return launch_grad_vjp(gx, g.hw, gy, g.hw, base, g.hw, nullptr, 0, out, g.hw, B, g, dx, scale,
                         bpk::as_stream(stream));
}

extern "C" int bpk_ns_cip_vjp_f32(const float* f, int64_t f_plane_stride, const float* fx,
                                  const float* fy, const float* vel, const float* g_out,
                                  float* g_f, float* g_fx, float* g_fy, const float* g_vel_in,
                                  float* g_vel, int B, int nx, int ny, float dt, float dx,
                                  void* stream) {
  NS_GEO_CHECK("ns_step vjp", B, nx, ny);
  if (B == 0) return BPK_OK;
  BPK_REQUIRE(vel && g_out, "ns_cip_vjp: vel and g_out required");
  BPK_REQUIRE((g_f && g_fx && g_fy) || (!g_f && !g_fx && !g_fy),
              "ns_cip_vjp: g_f, g_fx, g_fy go together");
  BPK_REQUIRE(!g_vel || (f && fx && fy), "ns_cip_vjp: g_vel needs f, fx, fy");
  const Geo g{nx, ny, (int64_t)nx * ny};
  CipVjpArgs<1> a;
  a.f[0] = f;
  a.fx[0] = fx;
  a.fy[0] = fy;
  a.gout[0] = g_out;
  a.gf[0] = g_f;
  a.gfx[0] = g_fx;
  a.gfy[0] = g_fy;
  a.fstride = f_plane_stride;
  a.dstride = a.gstride = a.ostride = g.hw;
  a.vel = vel;
  a.gvel_in = g_vel_in;
  a.gvel_out = g_vel;
  hipLaunchKernelGGL(k_cip_vjp<1>, grid_for(B, g), dim3(256), 0, bpk::as_stream(stream),
                     a, B, g, dt, dx);
  BPK_LAUNCH_CHECK("ns_cip_vjp");
  return BPK_OK;
}

extern "C" int bpk_ns_update_pressure_vjp_f32(const float* vel, const float* g_out, float* g_pres,
                                              const float* g_vel_in, float* g_vel, int B, int nx,
                                              int ny, float dt, float dx, void* stream) {
  NS_GEO_CHECK("ns_step vjp", B, nx, ny);
  if (B == 0) return BPK_OK;
  BPK_REQUIRE(vel && g_out, "ns_update_pressure_vjp: vel and g_out required");
  BPK_REQUIRE(g_pres || g_vel, "ns_update_pressure_vjp: no gradient requested");
  const Geo g{nx, ny, (int64_t)nx * ny};
  hipLaunchKernelGGL(k_pres_vjp, grid_for(B, g), dim3(256), 0, bpk::as_stream(stream),
                     vel, g_out, g_pres, g_vel_in, g_vel, B, g, dt, dx);
  BPK_LAUNCH_CHECK("ns_update_pressure_vjp");
  return BPK_OK;
}

extern "C" int bpk_ns_update_density_vjp_f32(const float* dens, const float* vel,
                                             const float* g_out, float* g_dens,
                                             const float* g_vel_in, float* g_vel,
                                             void* workspace, int B, int nx, int ny, float dt,
                                             float dx, void* stream) {
  NS_GEO_CHECK("ns_step vjp", B, nx, ny);
  if (B == 0) return BPK_OK;
  BPK_REQUIRE(dens && vel && g_out, "ns_update_density_vjp: dens, vel and g_out required");
  BPK_REQUIRE(g_dens || g_vel, "ns_update_density_vjp: no gradient requested");
  BPK_REQUIRE(workspace, "ns_update_density_vjp: workspace required");
  const Geo g{nx, ny, (int64_t)nx * ny};
  const int64_t P = (int64_t)B * g.hw;
  float* ws = static_cast<float*>(workspace);
  float *fx = ws, *fy = ws + P;
  float* gf = g_dens ? ws + 2 * P : nullptr;
  float* gfx = g_dens ? ws + 3 * P : nullptr;
  float* gfy = g_dens ? ws + 4 * P : nullptr;
  int rc = bpk_ns_gradient_f32(dens, g.hw, fx, fy, B, nx, ny, dx, stream);
  if (rc) return rc;
  rc = bpk_ns_cip_vjp_f32(dens, g.hw, fx, fy, vel, g_out, gf, gfx, gfy, g_vel_in, g_vel, B, nx, ny,
                          dt, dx, stream);
  if (rc || !g_dens) return rc;
  return launch_grad_vjp(gfx, g.hw, gfy, g.hw, gf, g.hw, nullptr, 0, g_dens, g.hw, B, g, dx, 1.0f,
                         bpk::as_stream(stream));
}

extern "C" int bpk_ns_update_velocity_vjp_f32(const float* vel, const float* pres,
                                              const float* g_out, float* g_vel, float* g_pres,
                                              void* workspace, int B, int nx, int ny, float dt,
                                              float dx, void* stream) {
  NS_GEO_CHECK("ns_step vjp", B, nx, ny);
  if (B == 0) return BPK_OK;
  BPK_REQUIRE(vel && pres && g_out && g_vel,
              "ns_update_velocity_vjp: vel, pres, g_out and g_vel required");
  BPK_REQUIRE(workspace, "ns_update_velocity_vjp: workspace required");
  const Geo g{nx, ny, (int64_t)nx * ny};
  return velocity_stage_vjp(vel, pres, g_out, g_vel, g_pres, nullptr,
                            static_cast<float*>(workspace), B, g, dt, dx, stream);
}

extern "C" int bpk_ns_full_step_vjp_f32(const float* dens, const float* vel, const float* pres,
                                        const float* vel1, const float* g_dens1,
                                        const float* g_vel1, const float* g_pres1, float* g_dens,
                                        float* g_vel, float* g_pres, void* workspace, int B,
                                        int nx, int ny, float dt, float dx, void* stream) {
  NS_GEO_CHECK("ns_step vjp", B, nx, ny);
  if (B == 0) return BPK_OK;
  BPK_REQUIRE(dens && vel && pres && vel1, "ns_full_step_vjp: dens, vel, pres and vel1 required");
  BPK_REQUIRE(g_dens1 || g_vel1 || g_pres1, "ns_full_step_vjp: no cotangent given");
  BPK_REQUIRE(g_vel && g_pres, "ns_full_step_vjp: g_vel and g_pres required");
  BPK_REQUIRE(workspace, "ns_full_step_vjp: workspace required");
  const Geo g{nx, ny, (int64_t)nx * ny};
  const int64_t P = (int64_t)B * g.hw;
  hipStream_t st = bpk::as_stream(stream);
  float* ws = static_cast<float*>(workspace);
  float* G1 = ws + 16 * P;  // total cotangent of (u1, v1), 2B planes
  int rc;
  // p1 = PRES(p, u1, v1): g_pres <- 0.25 gather, G1 <- g_vel1 + velocity terms
  if (g_pres1) {
    rc = bpk_ns_update_pressure_vjp_f32(vel1, g_pres1, g_pres, g_vel1, G1, B, nx, ny, dt, dx,
                                        stream);
    if (rc) return rc;
  } else {
    NS_HIP_OK(hipMemsetAsync(g_pres, 0, P * sizeof(float), st), "ns_full_step_vjp");
    if (g_vel1)
      NS_HIP_OK(hipMemcpyAsync(G1, g_vel1, 2 * P * sizeof(float), hipMemcpyDeviceToDevice, st),
                "ns_full_step_vjp");
    else
      NS_HIP_OK(hipMemsetAsync(G1, 0, 2 * P * sizeof(float), st), "ns_full_step_vjp");
  }
  // d1 = CIP(d; u1, v1): g_dens, G1 += local terms (its scratch is reused by the next stage)
  if (g_dens1) {
    rc = bpk_ns_update_density_vjp_f32(dens, vel1, g_dens1, g_dens, G1, G1, ws, B, nx, ny, dt, dx,
                                       stream);
    if (rc) return rc;
  } else if (g_dens) {
    NS_HIP_OK(hipMemsetAsync(g_dens, 0, P * sizeof(float), st), "ns_full_step_vjp");
  }
  return velocity_stage_vjp(vel, pres, G1, g_vel, g_pres, g_pres, ws, B, g, dt, dx, stream);
}
