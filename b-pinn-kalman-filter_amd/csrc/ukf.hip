// Square-root unscented Kalman filter (Van der Merwe & Wan 2001, Merwe scaled sigma points),
// batched over N independent filters of state dimension n <= 64 and observation dimension
// <= 64, float32 (include/bpk.h, section "ukf").  One 256-thread block per filter
// (k_innovation: one 64-thread block per filter, described at the kernel):
//
//   k_sigma   S staged in LDS (stride 65), 2n+1 point rows written coalesced on n.
//   k_root    the (2n + d) x d matrix [sqrt(wi) D_1..D_2n ; R^T] lives in LDS (192 x 65 floats
//             = 48.75 KB at n = d = 64); Householder QR in place, d reflections, all four waves
//             (wave w owns rows k + w, k + w + 4, ...; lane = column); then wave 0 takes one row
//             of S = R^T per lane into registers for the sign fix and the point-0 rank-1
//             up/downdate.
//   k_update  P_xz by an LDS-tiled fma loop (chunks of 32 sigma points, 4 x 4 outputs per
//             thread), then wave 0 alone, lane = row: U = P_xz S_z^-T by forward substitution,
//             y = S_z^-1 (z - zhat), m+ = m- + U y (= m- + K (z - zhat), K = U S_z^-1), and the
//             obs-dim rank-1 downdates of S- by the columns of U (= K S_z) with the row of S in
//             64 registers and S_kk / x_k broadcast by v_readlane: no barrier and no LDS access
//             inside the n x obs-dim chain.
//   k_smooth  one backward (Rauch-Tung-Striebel) step: C = sum_s wc_s (X_s - m)(Y_s - m-)^T by
//             the same tiled loop, then wave 0 does U = C S-^-T, y and m^s exactly as the update
//             does (S_z := S-, z := m^s_+) while wave 1 solves S- B = S^s_+ (lane = column) in
//             the tile the chunks left free; W = U B by all four waves (4 x 4 outputs per
//             thread) overwrites S-; S is staged through the B tile and wave 0 runs n rank-1
//             updates by W's columns, then n downdates by U's, on its 64-register row.  Three
//             tiles, 49 920 B, as the update.
//
// LDS tiles are [64][65]: a column walk (lane = row, fixed column) and a row walk (lane =
// column) both touch 32 distinct banks per half wave (65 mod 32 = 1).
//
// Point rows are ordered (g, s, r): filter i = g * (N / groups) + r has its sigma point s at row
// (g * (2n + 1) + s) * (N / groups) + r.
//
// Loss of positive definiteness in a downdate (S_kk^2 - x_k^2 <= 0, or NaN) is a numerical
// condition, not an error: S_kk := eps_f32 |S_kk|, the rest of that vector is dropped (so
// nothing can grow without bound), and the filter's status is set to 1.  All loops have trip
// counts fixed by (n, d); no atomics; every reduction has a fixed order.
#include "bpk_common.h"

#include <cfloat>
#include <cmath>

// no implicit FMA contraction: the sigma points must round like torch's separate gamma * S and
// m +- (.) float32 ops (bit-exact test); every fused multiply-add below is an explicit fmaf
#pragma clang fp contract(off)

namespace {

constexpr int kMaxDim = 64;
constexpr int kLd = 65;  // LDS row stride of a 64-wide tile
constexpr int kThreads = 256;
constexpr int kWaves = 4;

struct Rows {  // (g, s, r) row addressing of one filter
  int64_t base, stride;
  __device__ Rows(int64_t filter, int64_t N, int groups, int n) {
    const int64_t ng = N / groups, g = filter / ng, r = filter % ng;
    base = g * (2 * n + 1) * ng + r;
    stride = ng;
  }
  __device__ int64_t row(int s) const { return base + s * stride; }
};

__device__ __forceinline__ float lane_bcast(float v, int k) {
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), k));
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// Rank-1 update (SIGN = +1) / downdate (SIGN = -1) of a lower Cholesky factor held one row per
// lane (row[k] = S[lane][k]; lanes >= n and the upper triangle hold zeros and stay zero) by the
// vector x (one element per lane).  One wave, no memory access.
template <int SIGN>
__device__ __forceinline__ void chol_rank1(float (&row)[kMaxDim], float x, int n, int lane,
                                           int& flag) {
#pragma unroll
  for (int k = 0; k < kMaxDim; ++k) {
    if (k < n) {  // wave-uniform
      const float skk = lane_bcast(row[k], k);
      const float xk = lane_bcast(x, k);
      const float r2 = fmaf((float)SIGN * xk, xk, skk * skk);
      if (SIGN < 0 && !(r2 > 0.f)) {  // wave-uniform: not positive definite (or NaN)
        flag = 1;
        if (lane == k) row[k] = FLT_EPSILON * fabsf(skk);
        x = 0.f;
      } else {
        const float r = sqrtf(r2);
        const float rinv = 1.f / r, sinv = 1.f / skk;
        // (S + sign s x) / c = (S S_kk + sign x_k x) / r;  c x - s S' = (r x - x_k S') / S_kk
        const float snew = fmaf((float)SIGN * xk, x, row[k] * skk) * rinv;
        if (lane > k) {
          row[k] = snew;
          x = fmaf(r, x, -xk * snew) * sinv;
        } else if (lane == k) {
          row[k] = r;
        }
      }
    }
  }
}

// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void k_sigma(const float* __restrict__ mean,
                                                    const float* __restrict__ S,
                                                    float* __restrict__ out, int64_t N, int n,
                                                    float gamma, int groups) {
  __shared__ float St[kMaxDim * kLd];
  const int64_t f = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const float* Sf = S + f * n * n;
  for (int idx = tid; idx < n * n; idx += kThreads) St[(idx / n) * kLd + idx % n] = Sf[idx];
  __syncthreads();
  if (lane >= n) return;
  const Rows rows(f, N, groups, n);
  const float m = mean[f * n + lane];
  for (int s = w; s < 2 * n + 1; s += kWaves) {
    float v = m;  // two roundings, as m + gamma * S evaluated op by op
    if (s >= 1 && s <= n) v = m + gamma * St[lane * kLd + s - 1];
    if (s > n) v = m - gamma * St[lane * kLd + s - 1 - n];
    out[rows.row(s) * n + lane] = v;
  }
}

// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void k_root(const float* __restrict__ pts,
                                                   const float* __restrict__ noise,
                                                   float* __restrict__ mean_out,
                                                   float* __restrict__ tril_out,
                                                   int* __restrict__ status, int64_t N, int n,
                                                   int d, float wm0, float wc0, float wi,
                                                   int groups) {
  __shared__ float A[3 * kMaxDim * kLd];  // rows 0..2n-1: deviations, 2n..2n+d-1: R^T
  __shared__ float part[kWaves * kMaxDim];
  __shared__ float red[kWaves];
  const int64_t f = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const Rows rows(f, N, groups, n);
  const int ns = 2 * n, M = ns + d;

  for (int t = w; t < ns; t += kWaves)
    A[t * kLd + lane] = lane < d ? pts[rows.row(t + 1) * d + lane] : 0.f;
  const float y0 = lane < d ? pts[rows.row(0) * d + lane] : 0.f;
  {  // R^T below the deviations: lane = column k of the factor, lower triangle only
    const float* Rf = noise + f * d * d;
    for (int j = w; j < d; j += kWaves)
      if (lane < d) A[(ns + lane) * kLd + j] = lane <= j ? Rf[j * d + lane] : 0.f;
  }
  __syncthreads();

  // weighted mean: four partial sums per column, fixed order
  float acc = 0.f;
  for (int t = w; t < ns; t += kWaves) acc += A[t * kLd + lane];
  part[w * kMaxDim + lane] = acc;
  __syncthreads();
  const float ybar =
      fmaf(wm0, y0, wi * ((part[lane] + part[kMaxDim + lane]) +
                          (part[2 * kMaxDim + lane] + part[3 * kMaxDim + lane])));
  const float swi = sqrtf(wi);
  for (int t = w; t < ns; t += kWaves) A[t * kLd + lane] = swi * (A[t * kLd + lane] - ybar);
  const float x0 = lane < d ? sqrtf(fabsf(wc0)) * (y0 - ybar) : 0.f;
  if (w == 0 && lane < d) mean_out[f * d + lane] = ybar;
  __syncthreads();

  // Householder QR, R only: after step k row k of A holds R[k][k..d-1]
  for (int k = 0; k < d; ++k) {
    const int i0 = k + tid;
    const float cv = i0 < M ? A[i0 * kLd + k] : 0.f;
    const float ws = wave_sum(cv * cv);
    if (lane == 0) red[w] = ws;
    const float akk = A[k * kLd + k];
    __syncthreads();
    const float sigma = (red[0] + red[1]) + (red[2] + red[3]);
    const float nrm = sqrtf(sigma);
    const float alpha = akk >= 0.f ? -nrm : nrm;
    const float vk = akk - alpha;
    const float beta = sigma > 0.f ? 1.f / (nrm * (nrm + fabsf(akk))) : 0.f;
    const bool col = lane > k && lane < d;
    float dot = 0.f;
    if (col) {
      for (int i = k + w; i < M; i += kWaves) {
        const float vi = i == k ? vk : A[i * kLd + k];
        dot = fmaf(vi, A[i * kLd + lane], dot);
      }
    }
    part[w * kMaxDim + lane] = dot;
    __syncthreads();
    if (col) {
      const float wj = beta * ((part[lane] + part[kMaxDim + lane]) +
                               (part[2 * kMaxDim + lane] + part[3 * kMaxDim + lane]));
      for (int i = k + w; i < M; i += kWaves) {
        const float vi = i == k ? vk : A[i * kLd + k];
        A[i * kLd + lane] = fmaf(-vi, wj, A[i * kLd + lane]);
      }
    }
    if (w == 0 && lane == k) A[k * kLd + k] = alpha;
    __syncthreads();
  }

  // wave 0: S = R^T with a positive diagonal, one row per lane, then the point-0 term
  float* St = A + kMaxDim * kLd;  // rows 64..127 of A: output staging, disjoint from R
  if (w == 0) {
    float row[kMaxDim];
#pragma unroll
    for (int k = 0; k < kMaxDim; ++k) {
      row[k] = 0.f;
      if (k < d) {
        const float sg = A[k * kLd + k] < 0.f ? -1.f : 1.f;
        if (lane < d && k <= lane) row[k] = sg * A[k * kLd + lane];
      }
    }
    int flag = 0;
    if (wc0 > 0.f) chol_rank1<1>(row, x0, d, lane, flag);
    if (wc0 < 0.f) chol_rank1<-1>(row, x0, d, lane, flag);
#pragma unroll
    for (int k = 0; k < kMaxDim; ++k) St[lane * kLd + k] = row[k];
    if (lane == 0) status[f] = flag;
  }
  __syncthreads();
  float* So = tril_out + f * d * d;
  for (int idx = tid; idx < d * d; idx += kThreads) So[idx] = St[(idx / d) * kLd + idx % d];
}

// ---------------------------------------------------------------------------------------
constexpr int kChunk = 32;  // sigma points per cross-covariance tile

// Shared by k_update and k_smooth, all 256 threads: P[i][j] = sum_s wc_s (X_s - mx)[i]
// (Z_s - mz)[j] (P_xz of the update with Z = the measured points, C of the smoother with Z = the
// propagated points), contraction in chunks of kChunk points staged in T (2 x 32 x 64 floats);
// thread -> i = ti + 16 a, j = tj + 16 b.  mx / mz: this lane's element of the two means (0 past
// the dimension).  Rows and columns past (n, dz) come out 0.  The caller synchronises before it
// reads P or reuses T.
__device__ __forceinline__ void cross_cov(float* T, float* P, const float* __restrict__ xp,
                                          const float* __restrict__ zp, float mx, float mz,
                                          const Rows& rows, int n, int dz, float wc0, float wi,
                                          int tid) {
  const int lane = tid & 63, w = tid >> 6;
  const int ns1 = 2 * n + 1;
  float* Xc = T;
  float* Zc = T + kChunk * kMaxDim;
  const int ti = tid >> 4, tj = tid & 15;
  float acc[4][4] = {};
  for (int s0 = 0; s0 < ns1; s0 += kChunk) {
    __syncthreads();
    for (int t = w; t < kChunk; t += kWaves) {
      const int s = s0 + t;
      float xv = 0.f, zv = 0.f;
      if (s < ns1) {
        const int64_t r = rows.row(s);
        const float wgt = s == 0 ? wc0 : wi;
        if (lane < n) xv = wgt * (xp[r * n + lane] - mx);
        if (lane < dz) zv = zp[r * dz + lane] - mz;
      }
      Xc[t * kMaxDim + lane] = xv;
      Zc[t * kMaxDim + lane] = zv;
    }
    __syncthreads();
#pragma unroll 4
    for (int t = 0; t < kChunk; ++t) {
      float xa[4], zb[4];
#pragma unroll
      for (int a = 0; a < 4; ++a) xa[a] = Xc[t * kMaxDim + ti + 16 * a];
#pragma unroll
      for (int b = 0; b < 4; ++b) zb[b] = Zc[t * kMaxDim + tj + 16 * b];
#pragma unroll
      for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) acc[a][b] = fmaf(xa[a], zb[b], acc[a][b]);
    }
  }
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) P[(ti + 16 * a) * kLd + tj + 16 * b] = acc[a][b];
}

// Shared by k_update and k_smooth, wave 0 alone, lane = row: P := U = P Zt^-T in place by forward
// substitution (rows are independent), y = Zt^-1 v (v = this lane's element of the innovation,
// 0 past dz), and the return value mx + (U y)[lane].
__device__ __forceinline__ float gain_mean(float* P, const float* Zt, float v, float mx, int dz,
                                           int lane) {
  for (int j = 0; j < dz; ++j) {
    float a = P[lane * kLd + j];
    for (int c = 0; c < j; ++c) a = fmaf(-P[lane * kLd + c], Zt[j * kLd + c], a);
    P[lane * kLd + j] = a / Zt[j * kLd + j];
  }
  // Zt y = v; lane c ends up holding y_c
  for (int c = 0; c < dz; ++c) {
    const float yc = __shfl(v, c) / Zt[c * kLd + c];
    if (lane > c) v = fmaf(-yc, Zt[lane * kLd + c], v);
    if (lane == c) v = yc;
  }
  float mnew = mx;
  for (int c = 0; c < dz; ++c) mnew = fmaf(P[lane * kLd + c], __shfl(v, c), mnew);
  return mnew;
}

// Zt := the lower triangle of the d x d factor F, exact zeros everywhere else in the tile.
__device__ __forceinline__ void stage_tril(float* Zt, const float* __restrict__ F, int d,
                                           int tid) {
  for (int idx = tid; idx < kMaxDim * kLd; idx += kThreads) Zt[idx] = 0.f;
  __syncthreads();
  for (int idx = tid; idx < d * d; idx += kThreads) {
    const int j = idx / d, c = idx % d;
    if (c <= j) Zt[j * kLd + c] = F[idx];
  }
}

__global__ __launch_bounds__(kThreads) void k_update(
    const float* __restrict__ mean, const float* __restrict__ S, const float* __restrict__ xp,
    const float* __restrict__ zp, const float* __restrict__ zmean, const float* __restrict__ Sz,
    const float* __restrict__ obs, float* __restrict__ mean_out, float* __restrict__ tril_out,
    int* __restrict__ status, int64_t N, int n, int dz, float wc0, float wi, int groups) {
  __shared__ float T[kMaxDim * kLd];   // P_xz tiles (2 x 32 x 64), later S- / S+ staging
  __shared__ float P[kMaxDim * kLd];   // P_xz, then U = P_xz S_z^-T in place
  __shared__ float Zt[kMaxDim * kLd];  // S_z
  const int64_t f = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const Rows rows(f, N, groups, n);

  stage_tril(Zt, Sz + f * dz * dz, dz, tid);
  const float mx = lane < n ? mean[f * n + lane] : 0.f;
  const float mz = lane < dz ? zmean[f * dz + lane] : 0.f;
  cross_cov(T, P, xp, zp, mx, mz, rows, n, dz, wc0, wi, tid);
  __syncthreads();  // tiles consumed: T becomes the staging tile of S-
  {
    const float* Sf = S + f * n * n;
    for (int idx = tid; idx < n * n; idx += kThreads) T[(idx / n) * kLd + idx % n] = Sf[idx];
  }
  __syncthreads();

  if (w == 0) {
    const float mnew = gain_mean(P, Zt, lane < dz ? obs[f * dz + lane] - mz : 0.f, mx, dz, lane);
    if (lane < n) mean_out[f * n + lane] = mnew;

    float row[kMaxDim];
#pragma unroll
    for (int k = 0; k < kMaxDim; ++k)
      row[k] = (lane < n && k <= lane && k < n) ? T[lane * kLd + k] : 0.f;
    int flag = 0;
    for (int c = 0; c < dz; ++c) {
      const float x = lane < n ? P[lane * kLd + c] : 0.f;
      chol_rank1<-1>(row, x, n, lane, flag);
    }
#pragma unroll
    for (int k = 0; k < kMaxDim; ++k) T[lane * kLd + k] = row[k];
    if (lane == 0) status[f] = flag;
  }
  __syncthreads();
  float* So = tril_out + f * n * n;
  for (int idx = tid; idx < n * n; idx += kThreads) So[idx] = T[(idx / n) * kLd + idx % n];
}

// ---------------------------------------------------------------------------------------
// One backward (Rauch-Tung-Striebel) step of the unscented smoother, see include/bpk.h.
__global__ __launch_bounds__(kThreads) void k_smooth(
    const float* __restrict__ mean, const float* __restrict__ S, const float* __restrict__ xp,
    const float* __restrict__ yp, const float* __restrict__ pmean, const float* __restrict__ Sp,
    const float* __restrict__ nmean, const float* __restrict__ Sn, float* __restrict__ mean_out,
    float* __restrict__ tril_out, int* __restrict__ status, int64_t N, int n, float wc0, float wi,
    int groups) {
  __shared__ float T[kMaxDim * kLd];   // C tiles, then S^s_+ -> B = S-^-1 S^s_+, then S / S^s
  __shared__ float P[kMaxDim * kLd];   // C, then U = C S-^-T in place
  __shared__ float Zt[kMaxDim * kLd];  // S- (the prediction's factor), then W = U B
  const int64_t f = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const Rows rows(f, N, groups, n);

  stage_tril(Zt, Sp + f * n * n, n, tid);
  const float mx = lane < n ? mean[f * n + lane] : 0.f;
  const float mp = lane < n ? pmean[f * n + lane] : 0.f;
  cross_cov(T, P, xp, yp, mx, mp, rows, n, n, wc0, wi, tid);
  __syncthreads();  // tiles consumed: T becomes S^s_+ (zeros outside its lower triangle)
  stage_tril(T, Sn + f * n * n, n, tid);
  __syncthreads();

  if (w == 0) {  // U, y and the smoothed mean, as the update does with S_z := S-, z := m^s_+
    const float mnew = gain_mean(P, Zt, lane < n ? nmean[f * n + lane] - mp : 0.f, mx, n, lane);
    if (lane < n) mean_out[f * n + lane] = mnew;
  } else if (w == 1) {
    // S- B = S^s_+ in place, lane = column: B[j][c] for j >= c (the zeros above the diagonal of
    // S^s_+ make the terms c' < c exact no-ops, so every lane runs the same trip counts)
    for (int j = 0; j < n; ++j) {
      float a = T[j * kLd + lane];
      for (int c = 0; c < j; ++c) a = fmaf(-Zt[j * kLd + c], T[c * kLd + lane], a);
      if (lane <= j) T[j * kLd + lane] = a / Zt[j * kLd + j];
    }
  }
  __syncthreads();
  {  // W = U B by all four waves into the tile of S- (read for the last time above)
    const int ti = tid >> 4, tj = tid & 15;
    float acc[4][4] = {};
#pragma unroll 4
    for (int k = 0; k < n; ++k) {
      float ua[4], bb[4];
#pragma unroll
      for (int a = 0; a < 4; ++a) ua[a] = P[(ti + 16 * a) * kLd + k];
#pragma unroll
      for (int b = 0; b < 4; ++b) bb[b] = T[k * kLd + tj + 16 * b];
#pragma unroll
      for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) acc[a][b] = fmaf(ua[a], bb[b], acc[a][b]);
    }
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int b = 0; b < 4; ++b) Zt[(ti + 16 * a) * kLd + tj + 16 * b] = acc[a][b];
  }
  __syncthreads();  // B consumed: T becomes the staging tile of S
  {
    const float* Sf = S + f * n * n;
    for (int idx = tid; idx < n * n; idx += kThreads) T[(idx / n) * kLd + idx % n] = Sf[idx];
  }
  __syncthreads();

  if (w == 0) {
    float row[kMaxDim];
#pragma unroll
    for (int k = 0; k < kMaxDim; ++k)
      row[k] = (lane < n && k <= lane && k < n) ? T[lane * kLd + k] : 0.f;
    int flag = 0;
    // updates first: every intermediate then dominates P^s (downdates first would pass through
    // the nearly singular P - C P-^-1 C^T when Q is small)
    for (int c = 0; c < n; ++c) {
      const float x = lane < n ? Zt[lane * kLd + c] : 0.f;
      chol_rank1<1>(row, x, n, lane, flag);
    }
    for (int c = 0; c < n; ++c) {
      const float x = lane < n ? P[lane * kLd + c] : 0.f;
      chol_rank1<-1>(row, x, n, lane, flag);
    }
#pragma unroll
    for (int k = 0; k < kMaxDim; ++k) T[lane * kLd + k] = row[k];
    if (lane == 0) status[f] = flag;
  }
  __syncthreads();
  float* So = tril_out + f * n * n;
  for (int idx = tid; idx < n * n; idx += kThreads) So[idx] = T[(idx / n) * kLd + idx % n];
}

// ---------------------------------------------------------------------------------------
// Innovation statistics of one filter per 64-thread block (one wave, lane = row), see
// include/bpk.h.  The lower triangle of S_z is staged in one [64][65] tile (16.6 KB, so nine
// blocks fit a CU's LDS and the 2304 filters of the shipped case are all resident at once); the
// global read is coalesced, 16 bytes per lane when VEC4.  The substitution is gain_mean's second
// loop, operation for operation (same divisor read, same fmaf), so e is the vector the update
// applied, bit for bit.  The two sums are wave butterflies: a fixed order.
constexpr int kInnovThreads = 64;

template <bool VEC4>
__global__ __launch_bounds__(kInnovThreads) void k_innovation(
    const float* __restrict__ zmean, const float* __restrict__ Sz, const float* __restrict__ obs,
    float* __restrict__ white, float* __restrict__ nis, float* __restrict__ loglik,
    int* __restrict__ status, int dz) {
  __shared__ float Zt[kMaxDim * kLd];
  const int64_t f = blockIdx.x;
  const int lane = threadIdx.x;
  const float* F = Sz + f * dz * dz;
  if (VEC4) {  // dz % 4 == 0 and a 16-byte aligned base: a quad never leaves its row
    const int q = dz >> 2;
    for (int idx = lane; idx < dz * q; idx += kInnovThreads) {
      const int j = idx / q, c = (idx % q) * 4;
      if (c <= j) {
        const float4 t = *reinterpret_cast<const float4*>(F + j * dz + c);
        float* z = Zt + j * kLd + c;
        z[0] = t.x;
        z[1] = t.y;
        z[2] = t.z;
        z[3] = t.w;
      }
    }
  } else {
    for (int idx = lane; idx < dz * dz; idx += kInnovThreads) {
      const int j = idx / dz, c = idx % dz;
      if (c <= j) Zt[j * kLd + c] = F[idx];
    }
  }
  __syncthreads();

  const bool in = lane < dz;
  const float d = in ? Zt[lane * kLd + lane] : 1.f;
  const float qnan = __int_as_float(0x7fc00000);
  if (__any(!(d > 0.f) || !(d <= FLT_MAX))) {  // wave-uniform: no factor of a covariance
    if (white != nullptr && in) white[f * dz + lane] = qnan;
    if (lane == 0) {
      nis[f] = qnan;
      loglik[f] = qnan;
      status[f] = 1;
    }
    return;
  }
  float v = in ? obs[f * dz + lane] - zmean[f * dz + lane] : 0.f;
  // Zt e = v; lane c ends up holding e_c
  for (int c = 0; c < dz; ++c) {
    const float yc = __shfl(v, c) / Zt[c * kLd + c];
    if (in && lane > c) v = fmaf(-yc, Zt[lane * kLd + c], v);
    if (lane == c) v = yc;
  }
  if (white != nullptr && in) white[f * dz + lane] = v;
  const float q2 = wave_sum(v * v);  // lanes >= dz hold 0
  const float sl = wave_sum(in ? logf(d) : 0.f);
  if (lane == 0) {
    nis[f] = q2;
    // the three terms are combined in double and rounded once
    loglik[f] = (float)(-0.5 * ((double)q2 + 2.0 * (double)sl + dz * 1.8378770664093453));
    status[f] = 0;
  }
}

#define UKF_GEO_CHECK(what, dimname, dim)                                                      \
  BPK_REQUIRE(N >= 0 && N < (1ll << 31), "%s: N = %lld out of range", what, (long long)N);      \
  BPK_REQUIRE(n >= 1 && n <= kMaxDim, "%s: n = %d out of range [1, %d]", what, n, kMaxDim);     \
  BPK_REQUIRE(dim >= 1 && dim <= kMaxDim, "%s: %s = %d out of range [1, %d]", what, dimname,    \
              dim, kMaxDim);                                                                    \
  BPK_REQUIRE(groups >= 1 && N % groups == 0, "%s: groups = %d does not divide N = %lld", what, \
              groups, (long long)N)

#define UKF_PTR(what, p) BPK_REQUIRE(p != nullptr, "%s: %s is NULL", what, #p)

}  // namespace

extern "C" int bpk_ukf_sigma_points_f32(const float* mean, const float* scale_tril,
                                        float* points, int64_t N, int n, float gamma, int groups,
                                        void* stream) {
  UKF_GEO_CHECK("ukf_sigma_points", "n", n);
  UKF_PTR("ukf_sigma_points", mean);
  UKF_PTR("ukf_sigma_points", scale_tril);
  UKF_PTR("ukf_sigma_points", points);
  if (N == 0) return BPK_OK;
  hipLaunchKernelGGL(k_sigma, dim3((unsigned)N), dim3(kThreads), 0, bpk::as_stream(stream), mean,
                     scale_tril, points, N, n, gamma, groups);
  BPK_LAUNCH_CHECK("ukf_sigma_points");
  return BPK_OK;
}

extern "C" int bpk_ukf_root_f32(const float* points, const float* noise_tril, float* mean,
                                float* scale_tril, int* status, int64_t N, int n, int d,
                                float wm0, float wc0, float wi, int groups, void* stream) {
  UKF_GEO_CHECK("ukf_root", "d", d);
  BPK_REQUIRE(wi > 0.f, "ukf_root: wi = %g must be positive", (double)wi);
  UKF_PTR("ukf_root", points);
  UKF_PTR("ukf_root", noise_tril);
  UKF_PTR("ukf_root", mean);
  UKF_PTR("ukf_root", scale_tril);
  UKF_PTR("ukf_root", status);
  if (N == 0) return BPK_OK;
  hipLaunchKernelGGL(k_root, dim3((unsigned)N), dim3(kThreads), 0, bpk::as_stream(stream), points,
                     noise_tril, mean, scale_tril, status, N, n, d, wm0, wc0, wi, groups);
  BPK_LAUNCH_CHECK("ukf_root");
  return BPK_OK;
}

extern "C" int bpk_ukf_update_f32(const float* mean, const float* scale_tril,
                                  const float* x_points, const float* z_points,
                                  const float* z_mean, const float* z_tril, const float* obs,
                                  float* mean_out, float* scale_tril_out, int* status, int64_t N,
                                  int n, int dz, float wc0, float wi, int groups, void* stream) {
  UKF_GEO_CHECK("ukf_update", "dz", dz);
  UKF_PTR("ukf_update", mean);
  UKF_PTR("ukf_update", scale_tril);
  UKF_PTR("ukf_update", x_points);
  UKF_PTR("ukf_update", z_points);
  UKF_PTR("ukf_update", z_mean);
  UKF_PTR("ukf_update", z_tril);
  UKF_PTR("ukf_update", obs);
  UKF_PTR("ukf_update", mean_out);
  UKF_PTR("ukf_update", scale_tril_out);
  UKF_PTR("ukf_update", status);
  if (N == 0) return BPK_OK;
  hipLaunchKernelGGL(k_update, dim3((unsigned)N), dim3(kThreads), 0, bpk::as_stream(stream), mean,
                     scale_tril, x_points, z_points, z_mean, z_tril, obs, mean_out,
                     scale_tril_out, status, N, n, dz, wc0, wi, groups);
  BPK_LAUNCH_CHECK("ukf_update");
  return BPK_OK;
}

extern "C" int bpk_ukf_smooth_f32(const float* mean, const float* scale_tril,
                                  const float* x_points, const float* y_points,
                                  const float* pred_mean, const float* pred_tril,
                                  const float* next_mean, const float* next_tril,
                                  float* mean_out, float* scale_tril_out, int* status, int64_t N,
                                  int n, float wc0, float wi, int groups, void* stream) {
  UKF_GEO_CHECK("ukf_smooth", "n", n);
  UKF_PTR("ukf_smooth", mean);
  UKF_PTR("ukf_smooth", scale_tril);
  UKF_PTR("ukf_smooth", x_points);
  UKF_PTR("ukf_smooth", y_points);
  UKF_PTR("ukf_smooth", pred_mean);
  UKF_PTR("ukf_smooth", pred_tril);
  UKF_PTR("ukf_smooth", next_mean);
  UKF_PTR("ukf_smooth", next_tril);
  UKF_PTR("ukf_smooth", mean_out);
  UKF_PTR("ukf_smooth", scale_tril_out);
  UKF_PTR("ukf_smooth", status);
  if (N == 0) return BPK_OK;
  hipLaunchKernelGGL(k_smooth, dim3((unsigned)N), dim3(kThreads), 0, bpk::as_stream(stream), mean,
                     scale_tril, x_points, y_points, pred_mean, pred_tril, next_mean, next_tril,
                     mean_out, scale_tril_out, status, N, n, wc0, wi, groups);
  BPK_LAUNCH_CHECK("ukf_smooth");
  return BPK_OK;
}

extern "C" int bpk_ukf_innovation_f32(const float* z_mean, const float* z_tril, const float* obs,
                                      float* white, float* nis, float* loglik, int* status,
                                      int64_t N, int dz, void* stream) {
  BPK_REQUIRE(N >= 0 && N < (1ll << 31), "ukf_innovation: N = %lld out of range", (long long)N);
  BPK_REQUIRE(dz >= 1 && dz <= kMaxDim, "ukf_innovation: dz = %d out of range [1, %d]", dz,
              kMaxDim);
  UKF_PTR("ukf_innovation", z_mean);
  UKF_PTR("ukf_innovation", z_tril);
  UKF_PTR("ukf_innovation", obs);
  UKF_PTR("ukf_innovation", nis);
  UKF_PTR("ukf_innovation", loglik);
  UKF_PTR("ukf_innovation", status);
  if (N == 0) return BPK_OK;
  const bool vec4 = dz % 4 == 0 && reinterpret_cast<uintptr_t>(z_tril) % 16 == 0;
  hipLaunchKernelGGL(vec4 ? k_innovation<true> : k_innovation<false>, dim3((unsigned)N),
                     dim3(kInnovThreads), 0, bpk::as_stream(stream), z_mean, z_tril, obs, white,
                     nis, loglik, status, dz);
  BPK_LAUNCH_CHECK("ukf_innovation");
  return BPK_OK;
}
