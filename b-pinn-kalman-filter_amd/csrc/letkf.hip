// Local ensemble transform Kalman filter analysis (Hunt, Kostelich & Szunyogh 2007), float32
// (include/bpk.h, section "letkf"), in two entries that share one kernel body: the identity
// observation of the state (bpk_letkf_analysis_f32: the observation-space perturbations dY are
// the state's own dX), and observations on a grid of their own behind any operator
// (bpk_letkf_analysis_obs_f32: the caller passes the members in observation space, yens
// [B, m, Cy, Hy, Wy], and observation (i, j) sits at state grid point (stride i + offset,
// stride j + offset)).  Two launches for the identity, three with yens:
//
//   k_letkf_prep  member mean xbar [B, C, H, W] and the perturbations dX = ens - xbar written
//                 member-innermost, dxt [B, H, W, C, MP] (MP = m padded to 8 / 16 / 32 / 64, the
//                 pad members hold 0), into the workspace.  Reads are coalesced on x; the
//                 analysis kernel then reads one window entry of all members as one contiguous
//                 run of MP floats, and the C entries of a site are adjacent.  Run a second
//                 time on yens for ybar and dyt [B, Hy, Wy, Cy, MP].
//   k_letkf<MP, OBS>
//                 one 64-thread block (one wave) per 64 / MP grid points: lane = (g, r), group g
//                 works on grid point blockIdx * G + g, r is the member.
//                   1. A = (m-1)/inflation I + sum_j rho_j dY_j dY_j^T and g = sum_j rho_j dY_j
//                      (obs_j - ybar_j): lane r keeps row r of A in MP registers; the other
//                      members' dY_j come from a double-buffered LDS row (one barrier per
//                      entry, 16-byte reads).  The window is walked in the fixed order
//                      (dy, dx, c) over the whole (2R+1)^2 Cy box with wave-uniform bounds;
//                      clipped, tapered-out and unobserved entries are predicated off, and an
//                      entry no lane of the wave needs is skipped as a whole.  Whether a window
//                      position carries an observation ((y - offset) % stride == 0) and which
//                      one are running per-lane counters, one division before the loops, and
//                      rows and positions between the observations are skipped whole where the
//                      wave agrees.  The identity instantiation (OBS = false) has none of this:
//                      it indexes the state's grid directly, (y0 + dy, x0 + dx).
//                      (dY_r dY_k) rho is rounded in that order, so A is symmetric bit for bit,
//                      and with yens == ens, stride 1 the two entries give the same bits.
//                   2. Two-sided cyclic Jacobi on A and Q (= I at the start) in LDS tiles of row
//                      stride MP + 1 (as the [64][65] tiles of ukf.hip: row and column walks are
//                      both conflict free).  A sweep is MP - 1 rounds of the round-robin
//                      tournament, MP / 2 disjoint pairs each: lanes r < MP / 2 compute the
//                      rotations, every lane applies all of them to row r of A and of Q
//                      (A J, Q J), then to column r of A (J^T A), where the pivot pair is set to
//                      exact zeros.  A pair with |a_pq| <= u sqrt(a_pp a_qq) is left alone, and a
//                      round in which no pair of the wave rotates is not applied at all; the
//                      loop ends after the first sweep without a rotation anywhere in the wave
//                      (further sweeps over a converged group rotate nothing, so a grid point's
//                      result does not depend on its wave neighbours), or at the sweep cap.
//                   3. wbar = Q L^-1 Q^T g by a column and a row walk; lane i keeps
//                      sqrt(m-1) Q[i][:] L^-1/2 in registers and forms column i of the symmetric
//                      root Wa against broadcast rows of Q; the C channels of the centre site
//                      are updated from the centre perturbations held in LDS.
//                 Pad members (r >= m) carry dX = 0: their rows of A are (m-1)/inflation on the
//                 diagonal and exact zeros elsewhere, every rotation that touches them is
//                 skipped, and they decouple exactly.
//
// LDS per block: 2 G MP (MP + 1) floats for A and Q (33 280 B at MP = 64, 16 896 B at 32) plus
// 4 KB of vectors: four blocks per CU at MP = 64.  No atomics, every reduction has a fixed
// order, all loop bounds are wave-uniform: a second run gives the same bits.
#include "bpk_common.h"

#include <cfloat>
#include <cmath>

// (dX_r dX_k) rho must round the product first (symmetry of A); every fused multiply-add
// below is an explicit fmaf
#pragma clang fp contract(off)

namespace {

constexpr int kWave = 64;
constexpr int kSweepCap = 16;
constexpr int kMaxC = 8;
constexpr int kMaxR = 8;
constexpr int kMaxM = 64;
constexpr float kU = 5.9604645e-8f;  // 2^-24, the unit roundoff

int padded_members(int m) { return m <= 8 ? 8 : m <= 16 ? 16 : m <= 32 ? 32 : 64; }

__global__ __launch_bounds__(256) void k_letkf_prep(const float* __restrict__ ens,
                                                    float* __restrict__ xbar,
                                                    float* __restrict__ dxt, int64_t total, int m,
                                                    int C, int64_t HW, int MP) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;  // (b, c, site)
  if (t >= total) return;
  const int64_t s = t % HW, bc = t / HW;
  const int c = (int)(bc % C);
  const int64_t b = bc / C;
  const float* e = ens + ((b * m) * C + c) * HW + s;
  const int64_t ms = (int64_t)C * HW;  // member stride
  float sum = 0.f;
  for (int k = 0; k < m; ++k) sum += e[k * ms];
  const float mean = sum / (float)m;
  xbar[t] = mean;
  float* d = dxt + ((b * HW + s) * C + c) * MP;
  for (int k = 0; k < m; ++k) d[k] = e[k * ms] - mean;
  for (int k = m; k < MP; ++k) d[k] = 0.f;
}

// pair i (0 <= i < n / 2) of round t (0 <= t < n - 1) of the round-robin tournament of n
// players (n even): player n - 1 stays, the others rotate; p < q
template <int N>
__device__ __forceinline__ void rr_pair(int t, int i, int& p, int& q) {
  constexpr int n1 = N - 1;
  int a = t + i, b = t - i;
  if (a >= n1) a -= n1;
  if (b < 0) b += n1;
  if (i == 0) a = n1;
  p = a < b ? a : b;
  q = a < b ? b : a;
}

// observation grid: observation (i, j) of [Cy, Hy, Wy] sits at state point (stride i + offset,
// stride j + offset); ybar / dyt are the prep kernel's output for the observation-space members
struct ObsGrid {
  const float* ybar;
  const float* dyt;
  int Cy, Hy, Wy, stride, offset;
};

// floor(a / s) for s >= 1
__device__ __forceinline__ int floor_div(int a, int s) { return a >= 0 ? a / s : -((s - 1 - a) / s); }

// OBS = false: the identity observation (dY = dX on the state's grid); og is not read, and
// that path pays nothing for the observation grid's indexing
template <int MP, bool OBS>
__global__ __launch_bounds__(kWave) void k_letkf(
    const float* __restrict__ xbar, const float* __restrict__ dxt, const float* __restrict__ obs,
    const float* __restrict__ prec, const float* __restrict__ taper, float* __restrict__ ens_out,
    int* __restrict__ status, int64_t N, int m, int C, int H, int W, int R, float a0,
    float sqrt_m1, float sqrt_infl, const ObsGrid og) {
  constexpr int G = kWave / MP, LD = MP + 1, HP = MP / 2;
  __shared__ float As[G * MP * LD];
  __shared__ float Qs[G * MP * LD];
  __shared__ __align__(16) float rowbuf[2][kWave];
  __shared__ float rc[kWave / 2], rs[kWave / 2];
  __shared__ float cen[kMaxC][kWave];
  __shared__ float gv[kWave], zv[kWave], wb[kWave], dl[kWave];

  const int lane = threadIdx.x, g = lane / MP, r = lane % MP;
  const int64_t pt = (int64_t)blockIdx.x * G + g;
  const bool active = pt < N;
  const int64_t HW = (int64_t)H * W;
  const int64_t b = active ? pt / HW : 0;
  const int site = active ? (int)(pt % HW) : 0;
  const int y0 = site / W, x0 = site % W;
  float* Ag = As + g * MP * LD;
  float* Qg = Qs + g * MP * LD;

  // ---- 1. A and g over the window --------------------------------------------------------
  float acc[MP];
#pragma unroll
  for (int k = 0; k < MP; ++k) acc[k] = 0.f;
  float gacc = 0.f;
  const int win = 2 * R + 1;
  // the identity observes the state's own grid: dY is dX, every window position carries an
  // observation, and stride, offset and the counters below are unused (dead code)
  const float* __restrict__ ybar = OBS ? og.ybar : xbar;
  const float* __restrict__ dyt = OBS ? og.dyt : dxt;
  const int Cy = OBS ? og.Cy : C, Hy = OBS ? og.Hy : H, Wy = OBS ? og.Wy : W;
  const int stride = OBS ? og.stride : 1, offset = OBS ? og.offset : 0;
  const int64_t HWy = (int64_t)Hy * Wy;
  // window position y0 + dy = stride * iy + offset + ry, 0 <= ry < stride, kept while dy runs
  // (likewise x): it carries observation row iy where ry == 0 and 0 <= iy < Hy, which lies
  // inside the state's domain because stride (Hy - 1) + offset <= H - 1
  const int iy_first = floor_div(y0 - R - offset, stride);
  const int ix_first = floor_div(x0 - R - offset, stride);
  const int ry_first = y0 - R - offset - iy_first * stride;
  const int rx_first = x0 - R - offset - ix_first * stride;
  int e = 0;
  int iy = iy_first, ry = ry_first;
  for (int dy = -R; dy <= R; ++dy, ++ry) {
    bool hit_y = active;
    if constexpr (OBS) {
      if (ry == stride) {
        ry = 0;
        ++iy;
      }
      hit_y = active && ry == 0 && iy >= 0 && iy < Hy;
      if (!__any(hit_y)) continue;  // wave-uniform: a row between the observations' rows
    }
    int ix = ix_first, rx = rx_first;
    for (int dx = -R; dx <= R; ++dx, ++rx) {
      if constexpr (OBS) {
        if (rx == stride) {
          rx = 0;
          ++ix;
        }
      }
      const float tp = taper[(dy + R) * win + dx + R];
      if (tp == 0.f) continue;  // wave-uniform
      int y, x;  // the entry's row and column on the observation grid
      bool inwin;
      if constexpr (OBS) {
        y = iy, x = ix;
        inwin = hit_y && rx == 0 && ix >= 0 && ix < Wy;
        if (!__any(inwin)) continue;  // wave-uniform: no observation sits here
      } else {
        y = y0 + dy, x = x0 + dx;
        inwin = active && y >= 0 && y < H && x >= 0 && x < W;
      }
      for (int c = 0; c < Cy; ++c) {
        float rho = 0.f, dv = 0.f, innov = 0.f;
        if (inwin) {
          const int64_t idx = ((b * Cy + c) * Hy + y) * Wy + x;
          rho = tp * prec[idx];
          if (rho != 0.f) {
            dv = dyt[((b * HWy + (int64_t)y * Wy + x) * Cy + c) * MP + r];
            innov = obs[idx] - ybar[idx];
          }
        }
        if (!__any(rho != 0.f)) continue;  // wave-uniform: nobody observes this entry
        float* rb = rowbuf[e & 1];
        ++e;
        rb[lane] = dv;
        __syncthreads();
        const float4* r4 = reinterpret_cast<const float4*>(rb + g * MP);
#pragma unroll
        for (int k4 = 0; k4 < MP / 4; ++k4) {
          const float4 v = r4[k4];
          acc[4 * k4 + 0] = fmaf(dv * v.x, rho, acc[4 * k4 + 0]);
          acc[4 * k4 + 1] = fmaf(dv * v.y, rho, acc[4 * k4 + 1]);
          acc[4 * k4 + 2] = fmaf(dv * v.z, rho, acc[4 * k4 + 2]);
          acc[4 * k4 + 3] = fmaf(dv * v.w, rho, acc[4 * k4 + 3]);
        }
        gacc = fmaf(rho * dv, innov, gacc);
      }
    }
  }
#pragma unroll
  for (int k = 0; k < MP; ++k) {
    Ag[r * LD + k] = k == r ? acc[k] + a0 : acc[k];
    Qg[r * LD + k] = k == r ? 1.f : 0.f;
  }
  gv[lane] = gacc;
  for (int c = 0; c < C; ++c) cen[c][lane] = active ? dxt[(pt * C + c) * MP + r] : 0.f;
  __syncthreads();

  // ---- 2. cyclic Jacobi: A -> diag(lambda), Q -> eigenvectors ------------------------------
  unsigned long long rotated = 0;
  int sweep = 0;
  for (; sweep < kSweepCap; ++sweep) {
    bool rot = false;
    for (int t = 0; t < MP - 1; ++t) {
      bool rot_t = false;
      if (r < HP) {
        int p, q;
        rr_pair<MP>(t, r, p, q);
        const float app = Ag[p * LD + p], aqq = Ag[q * LD + q], apq = Ag[q * LD + p];
        float cs = 1.f, sn = 0.f;
        if (!(fabsf(apq) <= kU * sqrtf(fabsf(app * aqq)))) {  // also taken by NaN
          const float theta = (aqq - app) / (2.f * apq);
          const float at = fabsf(theta);
          // sqrt(theta^2 + 1) == |theta| in float32 long before theta^2 overflows
          const float tt = copysignf(at > 1e9f ? 0.5f / at : 1.f / (at + sqrtf(fmaf(at, at, 1.f))),
                                     theta);
          cs = 1.f / sqrtf(fmaf(tt, tt, 1.f));
          sn = tt * cs;
          rot_t = sn != 0.f;
        }
        rc[g * HP + r] = cs;
        rs[g * HP + r] = sn;
      }
      // wave-uniform: a round without a rotation anywhere in the wave changes nothing (its
      // rotations are identities, c = 1 and s = 0 exactly), so it is not applied
      if (!__any(rot_t)) continue;
      rot = rot || rot_t;
      __syncthreads();
      // A J and Q J: lane r owns row r
      for (int i = 0; i < HP; ++i) {
        int p, q;
        rr_pair<MP>(t, i, p, q);
        const float cs = rc[g * HP + i], sn = rs[g * HP + i];
        const float ap = Ag[r * LD + p], aq = Ag[r * LD + q];
        const float qp = Qg[r * LD + p], qq = Qg[r * LD + q];
        Ag[r * LD + p] = fmaf(cs, ap, -sn * aq);
        Ag[r * LD + q] = fmaf(sn, ap, cs * aq);
        Qg[r * LD + p] = fmaf(cs, qp, -sn * qq);
        Qg[r * LD + q] = fmaf(sn, qp, cs * qq);
      }
      __syncthreads();
      // J^T A: lane r owns column r; the pivot entries become exact zeros
      for (int i = 0; i < HP; ++i) {
        int p, q;
        rr_pair<MP>(t, i, p, q);
        const float cs = rc[g * HP + i], sn = rs[g * HP + i];
        const float ap = Ag[p * LD + r], aq = Ag[q * LD + r];
        float np_ = fmaf(cs, ap, -sn * aq);
        float nq_ = fmaf(sn, ap, cs * aq);
        if (sn != 0.f) {
          if (r == q) np_ = 0.f;
          if (r == p) nq_ = 0.f;
        }
        Ag[p * LD + r] = np_;
        Ag[q * LD + r] = nq_;
      }
      __syncthreads();
    }
    rotated = __ballot(rot);
    if (rotated == 0) break;
  }
  const unsigned long long gmask = (MP == kWave ? ~0ull : ((1ull << (MP % kWave)) - 1ull))
                                   << (g * MP);
  const bool capped = sweep == kSweepCap && (rotated & gmask) != 0;

  // ---- 3. wbar = Q L^-1 Q^T g,  Wa = sqrt(m-1) Q L^-1/2 Q^T,  the centre site ---------------
  const float lam = Ag[r * LD + r];
  float z = 0.f;
  for (int k = 0; k < MP; ++k) z = fmaf(Qg[k * LD + r], gv[g * MP + k], z);
  zv[lane] = z / lam;
  dl[lane] = sqrt_m1 / sqrtf(lam);
  __syncthreads();
  float w = 0.f;
  for (int l = 0; l < MP; ++l) w = fmaf(Qg[r * LD + l], zv[g * MP + l], w);
  wb[lane] = w;
  float qs[MP];
#pragma unroll
  for (int l = 0; l < MP; ++l) qs[l] = Qg[r * LD + l] * dl[g * MP + l];
  __syncthreads();
  float out[kMaxC];
#pragma unroll
  for (int c = 0; c < kMaxC; ++c) out[c] = 0.f;
  for (int k = 0; k < m; ++k) {
    float wa = 0.f;
#pragma unroll
    for (int l = 0; l < MP; ++l) wa = fmaf(Qg[k * LD + l], qs[l], wa);
    const float tki = wb[g * MP + k] + wa;
#pragma unroll
    for (int c = 0; c < kMaxC; ++c)
      if (c < C) out[c] = fmaf(cen[c][g * MP + k], tki, out[c]);
  }

  const bool mine = active && r < m;
  float mean[kMaxC];
  bool bad = false;
#pragma unroll
  for (int c = 0; c < kMaxC; ++c) {
    mean[c] = 0.f;
    if (c < C && mine) {
      mean[c] = xbar[(b * C + c) * HW + site];
      out[c] += mean[c];
      bad = bad || !(fabsf(out[c]) <= FLT_MAX);
    }
  }
  const bool flagged = capped || (__ballot(bad) & gmask) != 0;
  if (mine) {
#pragma unroll
    for (int c = 0; c < kMaxC; ++c)
      if (c < C)
        ens_out[((b * m + r) * C + c) * HW + site] =
            flagged ? fmaf(sqrt_infl, cen[c][lane], mean[c]) : out[c];
    if (r == 0) status[pt] = flagged ? 1 : 0;
  }
}

// og == nullptr: the identity observation
template <int MP>
void launch(const float* xbar, const float* dxt, const ObsGrid* og, const float* obs,
            const float* prec, const float* taper, float* ens_out, int* status, int64_t N, int m,
            int C, int H, int W, int R, float inflation, hipStream_t stream) {
  constexpr int G = kWave / MP;
  const dim3 grid((unsigned)((N + G - 1) / G));
  const float a0 = (float)(m - 1) / inflation, sqrt_m1 = sqrtf((float)(m - 1));
  if (og == nullptr)
    hipLaunchKernelGGL((k_letkf<MP, false>), grid, dim3(kWave), 0, stream, xbar, dxt, obs, prec,
                       taper, ens_out, status, N, m, C, H, W, R, a0, sqrt_m1, sqrtf(inflation),
                       ObsGrid{});
  else
    hipLaunchKernelGGL((k_letkf<MP, true>), grid, dim3(kWave), 0, stream, xbar, dxt, obs, prec,
                       taper, ens_out, status, N, m, C, H, W, R, a0, sqrt_m1, sqrtf(inflation),
                       *og);
}

void launch_padded(int MP, const float* xbar, const float* dxt, const ObsGrid* og,
                   const float* obs, const float* prec, const float* taper, float* ens_out,
                   int* status, int64_t N, int m, int C, int H, int W, int R, float inflation,
                   hipStream_t s) {
  switch (MP) {
    case 8: launch<8>(xbar, dxt, og, obs, prec, taper, ens_out, status, N, m, C, H, W, R, inflation, s); break;
    case 16: launch<16>(xbar, dxt, og, obs, prec, taper, ens_out, status, N, m, C, H, W, R, inflation, s); break;
    case 32: launch<32>(xbar, dxt, og, obs, prec, taper, ens_out, status, N, m, C, H, W, R, inflation, s); break;
    default: launch<64>(xbar, dxt, og, obs, prec, taper, ens_out, status, N, m, C, H, W, R, inflation, s); break;
  }
}

void launch_prep(const float* ens, float* mean, float* pert, int64_t B, int m, int C, int64_t HW,
                 int MP, hipStream_t s) {
  const int64_t total = B * HW * C;
  hipLaunchKernelGGL(k_letkf_prep, dim3((unsigned)bpk::ceil_div(total, 256)), dim3(256), 0, s, ens,
                     mean, pert, total, m, C, HW, MP);
}

bool geometry_ok(int64_t B, int m, int C, int H, int W) {
  return B >= 0 && m >= 2 && m <= kMaxM && C >= 1 && C <= kMaxC && H >= 1 && W >= 1 &&
         (B == 0 || (int64_t)H * W < (1ll << 31) / B);
}

}  // namespace

extern "C" int64_t bpk_letkf_workspace_bytes(int64_t B, int m, int C, int H, int W) {
  if (!geometry_ok(B, m, C, H, W)) return -1;
  return B * C * H * W * (int64_t)(1 + padded_members(m)) * (int64_t)sizeof(float);
}

extern "C" int bpk_letkf_analysis_f32(const float* ens, const float* obs, const float* prec,
                                      const float* taper, float* ens_out, int* status,
                                      void* workspace, int64_t B, int m, int C, int H, int W, int R,
                                      float inflation, void* stream) {
  BPK_REQUIRE(m >= 2 && m <= kMaxM, "letkf_analysis: m = %d out of range [2, %d]", m, kMaxM);
  BPK_REQUIRE(C >= 1 && C <= kMaxC, "letkf_analysis: C = %d out of range [1, %d]", C, kMaxC);
  BPK_REQUIRE(R >= 0 && R <= kMaxR, "letkf_analysis: R = %d out of range [0, %d]", R, kMaxR);
  BPK_REQUIRE(H >= 1, "letkf_analysis: H = %d must be >= 1", H);
  BPK_REQUIRE(W >= 1, "letkf_analysis: W = %d must be >= 1", W);
  BPK_REQUIRE(inflation > 0.f && inflation <= FLT_MAX,
              "letkf_analysis: inflation = %g must be positive and finite", (double)inflation);
  BPK_REQUIRE(geometry_ok(B, m, C, H, W), "letkf_analysis: B = %lld out of range (B H W < 2^31)",
              (long long)B);
  BPK_REQUIRE(ens_out == nullptr || ens_out != ens,
              "letkf_analysis: ens_out must not alias ens (neighbours read the background)");
  if (B == 0) return BPK_OK;
  BPK_REQUIRE(ens != nullptr, "letkf_analysis: ens is NULL");
  BPK_REQUIRE(obs != nullptr, "letkf_analysis: obs is NULL");
  BPK_REQUIRE(prec != nullptr, "letkf_analysis: prec is NULL");
  BPK_REQUIRE(taper != nullptr, "letkf_analysis: taper is NULL");
  BPK_REQUIRE(ens_out != nullptr, "letkf_analysis: ens_out is NULL");
  BPK_REQUIRE(status != nullptr, "letkf_analysis: status is NULL");
  BPK_REQUIRE(workspace != nullptr, "letkf_analysis: workspace is NULL");

  const int MP = padded_members(m);
  const int64_t HW = (int64_t)H * W, N = B * HW, total = N * C;
  float* xbar = static_cast<float*>(workspace);
  float* dxt = xbar + total;
  hipStream_t s = bpk::as_stream(stream);
  launch_prep(ens, xbar, dxt, B, m, C, HW, MP, s);
  BPK_LAUNCH_CHECK("letkf_analysis (prep)");
  launch_padded(MP, xbar, dxt, nullptr, obs, prec, taper, ens_out, status, N, m, C, H, W, R,
                inflation, s);
  BPK_LAUNCH_CHECK("letkf_analysis");
  return BPK_OK;
}

extern "C" int64_t bpk_letkf_obs_workspace_bytes(int64_t B, int m, int C, int H, int W, int Cy,
                                                 int Hy, int Wy) {
  if (!geometry_ok(B, m, C, H, W) || !geometry_ok(B, m, Cy, Hy, Wy)) return -1;
  return (B * C * H * W + B * Cy * Hy * Wy) * (int64_t)(1 + padded_members(m)) *
         (int64_t)sizeof(float);
}

extern "C" int bpk_letkf_analysis_obs_f32(const float* ens, const float* yens, const float* obs,
                                          const float* prec, const float* taper, float* ens_out,
                                          int* status, void* workspace, int64_t B, int m, int C,
                                          int H, int W, int Cy, int Hy, int Wy, int stride,
                                          int offset, int R, float inflation, void* stream) {
  BPK_REQUIRE(m >= 2 && m <= kMaxM, "letkf_analysis_obs: m = %d out of range [2, %d]", m, kMaxM);
  BPK_REQUIRE(C >= 1 && C <= kMaxC, "letkf_analysis_obs: C = %d out of range [1, %d]", C, kMaxC);
  BPK_REQUIRE(Cy >= 1 && Cy <= kMaxC, "letkf_analysis_obs: Cy = %d out of range [1, %d]", Cy,
              kMaxC);
  BPK_REQUIRE(R >= 0 && R <= kMaxR, "letkf_analysis_obs: R = %d out of range [0, %d]", R, kMaxR);
  BPK_REQUIRE(H >= 1, "letkf_analysis_obs: H = %d must be >= 1", H);
  BPK_REQUIRE(W >= 1, "letkf_analysis_obs: W = %d must be >= 1", W);
  BPK_REQUIRE(Hy >= 1, "letkf_analysis_obs: Hy = %d must be >= 1", Hy);
  BPK_REQUIRE(Wy >= 1, "letkf_analysis_obs: Wy = %d must be >= 1", Wy);
  BPK_REQUIRE(stride >= 1, "letkf_analysis_obs: stride = %d must be >= 1", stride);
  BPK_REQUIRE(offset >= 0 && offset < stride,
              "letkf_analysis_obs: offset = %d out of range [0, stride = %d)", offset, stride);
  BPK_REQUIRE((int64_t)stride * (Hy - 1) + offset <= (int64_t)H - 1,
              "letkf_analysis_obs: Hy = %d does not fit: stride * (Hy - 1) + offset = %lld > "
              "H - 1 = %d",
              Hy, (long long)((int64_t)stride * (Hy - 1) + offset), H - 1);
  BPK_REQUIRE((int64_t)stride * (Wy - 1) + offset <= (int64_t)W - 1,
              "letkf_analysis_obs: Wy = %d does not fit: stride * (Wy - 1) + offset = %lld > "
              "W - 1 = %d",
              Wy, (long long)((int64_t)stride * (Wy - 1) + offset), W - 1);
  BPK_REQUIRE(inflation > 0.f && inflation <= FLT_MAX,
              "letkf_analysis_obs: inflation = %g must be positive and finite", (double)inflation);
  BPK_REQUIRE(geometry_ok(B, m, C, H, W) && geometry_ok(B, m, Cy, Hy, Wy),
              "letkf_analysis_obs: B = %lld out of range (B H W and B Hy Wy < 2^31)",
              (long long)B);
  BPK_REQUIRE(ens_out == nullptr || ens_out != ens,
              "letkf_analysis_obs: ens_out must not alias ens (neighbours read the background)");
  BPK_REQUIRE(ens_out == nullptr || ens_out != yens,
              "letkf_analysis_obs: ens_out must not alias yens (neighbours read it)");
  if (B == 0) return BPK_OK;
  BPK_REQUIRE(ens != nullptr, "letkf_analysis_obs: ens is NULL");
  BPK_REQUIRE(yens != nullptr, "letkf_analysis_obs: yens is NULL");
  BPK_REQUIRE(obs != nullptr, "letkf_analysis_obs: obs is NULL");
  BPK_REQUIRE(prec != nullptr, "letkf_analysis_obs: prec is NULL");
  BPK_REQUIRE(taper != nullptr, "letkf_analysis_obs: taper is NULL");
  BPK_REQUIRE(ens_out != nullptr, "letkf_analysis_obs: ens_out is NULL");
  BPK_REQUIRE(status != nullptr, "letkf_analysis_obs: status is NULL");
  BPK_REQUIRE(workspace != nullptr, "letkf_analysis_obs: workspace is NULL");

  const int MP = padded_members(m);
  const int64_t HW = (int64_t)H * W, N = B * HW, HWy = (int64_t)Hy * Wy;
  float* xbar = static_cast<float*>(workspace);
  float* dxt = xbar + N * C;
  float* ybar = dxt + N * C * MP;
  float* dyt = ybar + B * HWy * Cy;
  hipStream_t s = bpk::as_stream(stream);
  launch_prep(ens, xbar, dxt, B, m, C, HW, MP, s);
  BPK_LAUNCH_CHECK("letkf_analysis_obs (prep of ens)");
  launch_prep(yens, ybar, dyt, B, m, Cy, HWy, MP, s);
  BPK_LAUNCH_CHECK("letkf_analysis_obs (prep of yens)");
  const ObsGrid og{ybar, dyt, Cy, Hy, Wy, stride, offset};
  launch_padded(MP, xbar, dxt, &og, obs, prec, taper, ens_out, status, N, m, C, H, W, R, inflation,
                s);
  BPK_LAUNCH_CHECK("letkf_analysis_obs");
  return BPK_OK;
}
