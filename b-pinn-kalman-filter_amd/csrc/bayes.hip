// Bayesian (mean-field Gaussian, reparameterized) weights of one network in one launch.
//
// The reference gets its Bayesian conv layers from bayesian_torch (dnn_to_bnn,
// pinn_kalman/pinn.py:116-148): every layer call computes sigma = log1p(exp(rho)),
// w = mu + sigma * eps and kl_div(mu, sigma, prior_mu, prior_sigma).mean() for its kernel and
// its bias, and get_kl_loss sums those means over the layers -- ~8 small launches per tensor,
// ~260 tensors per PINN.  Here mu and rho of a whole network are two flat float32 vectors of
// P elements, a device table of S segments (one per kernel / bias) says which prior and which
// mean each element belongs to, and
//
//   forward : W[e]  = mu[e] + softplus(rho[e]) * eps[e]
//             KL    = sum_s (1 / n_s) sum_{e in s} [ log(sp_s / sigma) + (sigma^2 +
//                     (mu - mp_s)^2) / (2 sp_s^2) - 1/2 ]
//   backward: gmu   = gW + gKL (mu - mp_s) / (sp_s^2 n_s)
//             grho  = (gW eps + gKL (sigma / sp_s^2 - 1 / sigma) / n_s) sigmoid(rho)
//
// eps[e] is the Philox4x32-10 / Box-Muller normal of philox.h at (seed, step, draw 0, global
// element e) -- the bits bpk_philox_normal_f32(out, 1, P, 0, seed, &step, 0) writes at e.  It
// is never stored: the backward draws it again.  One thread owns one Philox block, i.e. the 4
// consecutive flat elements 4 q .. 4 q + 3 (one float4 of every operand); segments start at
// arbitrary offsets, so a thread walks the table while it walks its 4 elements.
//
// KL: the per-element term is evaluated in float64 (sigma spans e^-100 .. 30 and
// log(sp / sigma) would carry the whole float32 error of the sum), summed per thread in
// element order, per block in a fixed shuffle / LDS tree into `ws`, and a one-block second
// launch adds the block partials in index order: no atomics, so the value is bitwise the same
// from run to run (the grid is a function of P alone).
#include "bpk_common.h"
#include "philox.h"

namespace {

constexpr int kThreads = 256;
constexpr int kMaxBlocks = 1024;
constexpr int kTab = 4;  // doubles per segment: offset, numel, prior_mu, prior_sigma

inline int64_t blocks_of(int64_t P) {
  const int64_t nb = bpk::ceil_div(bpk::ceil_div(P, 4), kThreads);
  return nb < kMaxBlocks ? nb : kMaxBlocks;
}

// largest s with offset[s] <= e (offsets ascend from 0; s stays in [0, S))
__device__ inline int find_segment(const double* tab, int S, int64_t e) {
  int lo = 0, hi = S - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if ((int64_t)tab[(int64_t)mid * kTab] <= e) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

struct Load4 {
  float v[4];
};

template <bool VEC>
__device__ inline Load4 load4(const float* p, int64_t e0, int cnt) {
  Load4 r;
  if (VEC && cnt == 4) {
    const float4 t = *reinterpret_cast<const float4*>(p + e0);
    r.v[0] = t.x, r.v[1] = t.y, r.v[2] = t.z, r.v[3] = t.w;
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) r.v[j] = j < cnt ? p[e0 + j] : 0.0f;
  }
  return r;
}

template <bool VEC>
__device__ inline void store4(float* p, int64_t e0, int cnt, const float v[4]) {
  if (VEC && cnt == 4) {
    *reinterpret_cast<float4*>(p + e0) = make_float4(v[0], v[1], v[2], v[3]);
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (j < cnt) p[e0 + j] = v[j];
  }
}

// sum of `v` over the block in a fixed order; valid in thread 0
__device__ inline double block_sum(double v) {
  __shared__ double part[kThreads / 64];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
  __syncthreads();
  double s = 0.0;
  if (threadIdx.x == 0) {
#pragma unroll
    for (int w = 0; w < kThreads / 64; ++w) s += part[w];
  }
  return s;
}

template <bool VEC>
__global__ __launch_bounds__(kThreads) void k_bayes_fwd(
    const float* __restrict__ mu, const float* __restrict__ rho, const double* __restrict__ tab,
    int S, int64_t P, uint64_t seed, int step, float* __restrict__ W, double* __restrict__ ws) {
  const int64_t nq = (P + 3) >> 2;
  double acc = 0.0;
  for (int64_t q = (int64_t)blockIdx.x * kThreads + threadIdx.x; q < nq;
       q += (int64_t)gridDim.x * kThreads) {
    const int64_t e0 = q << 2;
    const int cnt = P - e0 < 4 ? (int)(P - e0) : 4;
    const Load4 m = load4<VEC>(mu, e0, cnt), r = load4<VEC>(rho, e0, cnt);
    float z[4], w[4];
    bpk::normal4((uint64_t)q, step, 0, seed, z);
    int s = find_segment(tab, S, e0);
    int cur = -1;
    double pm = 0.0, log_sp = 0.0, inv2 = 0.0, invn = 0.0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (j < cnt) {
        while (s + 1 < S && e0 + j >= (int64_t)tab[(int64_t)(s + 1) * kTab]) ++s;
        if (s != cur) {
          const double* t = tab + (int64_t)s * kTab;
          pm = t[2];
          const double sp = t[3];
          log_sp = log(sp);
          inv2 = 0.5 / (sp * sp);
          invn = 1.0 / t[1];
          cur = s;
        }
        const double rd = (double)r.v[j];
        // softplus, stable at both ends: no overflow of exp, no cancellation in log1p
        const double sg = rd > 0.0 ? rd + log1p(exp(-rd)) : log1p(exp(rd));
        const double d = (double)m.v[j] - pm;
        acc += ((log_sp - log(sg)) + (sg * sg + d * d) * inv2 - 0.5) * invn;
        w[j] = m.v[j] + (float)sg * z[j];
      } else {
        w[j] = 0.0f;
      }
    }
    store4<VEC>(W, e0, cnt, w);
  }
  const double total = block_sum(acc);
  if (threadIdx.x == 0) ws[blockIdx.x] = total;
}

// second stage: the block partials added in index order (strided per thread, then the tree)
__global__ __launch_bounds__(kThreads) void k_bayes_kl(const double* __restrict__ ws, int nb,
                                                        float* __restrict__ kl) {
  double acc = 0.0;
  for (int i = threadIdx.x; i < nb; i += kThreads) acc += ws[i];
  const double total = block_sum(acc);
  if (threadIdx.x == 0) *kl = (float)total;
}

template <bool VEC>
__global__ __launch_bounds__(kThreads) void k_bayes_bwd(
    const float* __restrict__ mu, const float* __restrict__ rho, const double* __restrict__ tab,
    int S, int64_t P, uint64_t seed, int step, const float* __restrict__ gW,
    const float* __restrict__ gkl, float* __restrict__ gmu, float* __restrict__ grho) {
  const int64_t nq = (P + 3) >> 2;
  const float gk = gkl ? *gkl : 0.0f;
  for (int64_t q = (int64_t)blockIdx.x * kThreads + threadIdx.x; q < nq;
       q += (int64_t)gridDim.x * kThreads) {
    const int64_t e0 = q << 2;
    const int cnt = P - e0 < 4 ? (int)(P - e0) : 4;
    const Load4 m = load4<VEC>(mu, e0, cnt), r = load4<VEC>(rho, e0, cnt);
    Load4 g;
    if (gW) {
      g = load4<VEC>(gW, e0, cnt);
    } else {
      g.v[0] = g.v[1] = g.v[2] = g.v[3] = 0.0f;
    }
    float z[4], om[4], orh[4];
    bpk::normal4((uint64_t)q, step, 0, seed, z);
    int s = find_segment(tab, S, e0);
    int cur = -1;
    float pm = 0.0f, inv_s2 = 0.0f, c = 0.0f;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (j < cnt) {
        while (s + 1 < S && e0 + j >= (int64_t)tab[(int64_t)(s + 1) * kTab]) ++s;
        if (s != cur) {
          const double* t = tab + (int64_t)s * kTab;
          pm = (float)t[2];
          const float sp = (float)t[3];
          inv_s2 = 1.0f / (sp * sp);
          c = gk / (float)t[1];
          cur = s;
        }
        // sigma = softplus(rho), sig = sigmoid(rho), ratio = sig / sigma (-> 1 as rho -> -inf,
        // where sigma itself underflows: never formed as 1 / sigma)
        const float rr = r.v[j];
        float sg, sig, ratio;
        if (rr > 0.0f) {
          const float t = expf(-rr);
          sig = 1.0f / (1.0f + t);
          sg = rr + log1pf(t);
          ratio = sig / sg;
        } else {
          const float t = expf(rr);
          sig = t / (1.0f + t);
          if (rr < -17.0f) {  // log1p(t) == t and 1 / (1 + t) == 1 in float32
            sg = t;
            ratio = 1.0f;
          } else {
            sg = log1pf(t);
            ratio = sig / sg;
          }
        }
        om[j] = g.v[j] + c * (m.v[j] - pm) * inv_s2;
        orh[j] = g.v[j] * z[j] * sig + c * (sg * sig * inv_s2 - ratio);
      } else {
        om[j] = orh[j] = 0.0f;
      }
    }
    store4<VEC>(gmu, e0, cnt, om);
    store4<VEC>(grho, e0, cnt, orh);
  }
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

}  // namespace

extern "C" int64_t bpk_bayes_workspace_bytes(int64_t P) {
  if (P < 1) return 0;
  return blocks_of(P) * (int64_t)sizeof(double);
}

extern "C" int bpk_bayes_sample_kl_f32(const float* mu, const float* rho, const double* table,
                                       int S, int64_t P, uint64_t seed, int step, float* W,
                                       float* kl, void* ws, void* stream) {
  BPK_REQUIRE(P >= 1, "bayes_sample_kl: P = %lld elements (need >= 1)", (long long)P);
  BPK_REQUIRE(S >= 1 && (int64_t)S <= P, "bayes_sample_kl: S = %d segments for P = %lld", S,
              (long long)P);
  BPK_REQUIRE(mu && rho && table && W && kl && ws, "bayes_sample_kl: null pointer");
  const int nb = (int)blocks_of(P);
  double* part = static_cast<double*>(ws);
  if (aligned16(mu) && aligned16(rho) && aligned16(W))
    hipLaunchKernelGGL(k_bayes_fwd<true>, dim3(nb), dim3(kThreads), 0, bpk::as_stream(stream), mu,
                       rho, table, S, P, seed, step, W, part);
  else
    hipLaunchKernelGGL(k_bayes_fwd<false>, dim3(nb), dim3(kThreads), 0, bpk::as_stream(stream),
                       mu, rho, table, S, P, seed, step, W, part);
  BPK_LAUNCH_CHECK("bayes_sample_kl");
  hipLaunchKernelGGL(k_bayes_kl, dim3(1), dim3(kThreads), 0, bpk::as_stream(stream), part, nb, kl);
  BPK_LAUNCH_CHECK("bayes_sample_kl (second stage)");
  return BPK_OK;
}

extern "C" int bpk_bayes_sample_kl_bwd_f32(const float* mu, const float* rho, const double* table,
                                           int S, int64_t P, uint64_t seed, int step,
                                           const float* gW, const float* gkl, float* gmu,
                                           float* grho, void* stream) {
  BPK_REQUIRE(P >= 1, "bayes_sample_kl_bwd: P = %lld elements (need >= 1)", (long long)P);
  BPK_REQUIRE(S >= 1 && (int64_t)S <= P, "bayes_sample_kl_bwd: S = %d segments for P = %lld", S,
              (long long)P);
  BPK_REQUIRE(mu && rho && table && gmu && grho, "bayes_sample_kl_bwd: null pointer");
  const int nb = (int)blocks_of(P);
  if (aligned16(mu) && aligned16(rho) && aligned16(gmu) && aligned16(grho) &&
      (!gW || aligned16(gW)))
    hipLaunchKernelGGL(k_bayes_bwd<true>, dim3(nb), dim3(kThreads), 0, bpk::as_stream(stream), mu,
                       rho, table, S, P, seed, step, gW, gkl, gmu, grho);
  else
    hipLaunchKernelGGL(k_bayes_bwd<false>, dim3(nb), dim3(kThreads), 0, bpk::as_stream(stream),
                       mu, rho, table, S, P, seed, step, gW, gkl, gmu, grho);
  BPK_LAUNCH_CHECK("bayes_sample_kl_bwd");
  return BPK_OK;
}
