// Score-SDE Predictor-Corrector update kernels + counter-based Gaussian noise.
//
// Restates the per-step arithmetic of sampling.py (EulerMaruyamaPredictor
// :176-187, ReverseDiffusionPredictor :190-200, AncestralSamplingPredictor
// :203-239, LangevinCorrector :253-282, AnnealedLangevinDynamics :285-319) and
// of the reverse SDE (sde_lib.py:81-119) as fused elementwise kernels.  Each
// kernel keeps the reference's float32 operation order (FMA contraction off),
// so with the same model output and noise it is bit-identical to the torch-CPU
// restatement in oracle/score_sde_ref.py.
//
// Per-step scalars come from a device table built once on the host (float32,
// reference algorithm) and the step index from a device counter, so one PC step
// is a fixed launch sequence that a hipGraph can capture and replay N times.
//
// Noise: Philox4x32-10 keyed by `seed`; counter = (q_lo, q_hi, step, draw) with
// q = global_element / 4, global_element = (sample_offset + b) * D + e; 4 normals
// per counter via Box-Muller.  Identical values for any batch sharding.
//
// Conditional sampling (controllable_generation.py:44-52 inpainting, :136-144
// colorization): the data-consistency projection the reference applies after
// every predictor and corrector half-step is folded into the update kernels'
// single store of x_out / x_mean (template parameter COND), and exists stand-alone
// (k_project) for the half-steps whose update is None.  Its scalars (mean
// coefficient, std of sde.marginal_prob) come from a second table `mtab`
// [n_steps, mtab_bdim, 2] indexed by the same step counter.
//
// Draw ids (4th Philox counter word): 0 = predictor update, 1 + j = corrector
// update j, BPK_DATA_DRAW (0x100) + d = the data noise of the projection that
// follows the update with draw id d.  The data draw uses the same global element
// index as the update draw; colorization consumes only channel 0's elements.
#include "bpk_common.h"
#include "philox.h"

#include <algorithm>

#pragma clang fp contract(off)

namespace {

using bpk::normal4;

__device__ inline float noise_at(const float* noise, int64_t i, int64_t ge, int step, int draw,
                                 uint64_t seed) {
  if (noise) return noise[i];
  float z[4];
  normal4((uint64_t)ge >> 2, step, draw, seed, z);
  return z[ge & 3];
}

__device__ inline float score_of(float m, float sdiv, int score_mode) {
  return score_mode == 0 ? (-m) / sdiv : m;
}

// every kernel handles 4 consecutive elements of one sample per thread so the
// Philox block is computed once per 4 outputs when D % 4 == 0
struct Idx {
  int64_t b, e;
};

__global__ __launch_bounds__(256) void k_philox(float* out, int B, int64_t D, int64_t sample_offset,
                                                uint64_t seed, const int* step_ptr, int draw) {
  const int step = step_ptr ? *step_ptr : 0;
  const int64_t total = (int64_t)B * D;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t b = i / D;
    const int64_t ge = (sample_offset + b) * D + (i - b * D);
    out[i] = noise_at(nullptr, i, ge, step, draw, seed);
  }
}

// coef index helpers
#define C_SDIV 0
#define C_DRIFT 1
#define C_DIFF 2
#define C_DT 3
#define C_SQRT_MDT 4
#define C_ALPHA 5
#define C_AUX 6

// coefficient row of local sample b at `step`: table [n_steps, coef_bdim, STRIDE]
__device__ inline const float* coef_row(const float* coef, int coef_bdim, int step, int64_t b) {
  return coef + ((int64_t)step * coef_bdim + (coef_bdim == 1 ? 0 : b)) * BPK_COEF_STRIDE;
}

// ---- data-consistency projection of the conditional samplers
struct CondArgs {
  const float* data;    // inpaint: known image [B, D]; colorize: gray image [B, 3, HW]
  const float* mask;    // inpaint: float32 0/1 [B, D], 1 = known; colorize: not read
  const float* mtab;    // [n_steps, mtab_bdim, 2]: (mean coefficient, std) of marginal_prob
  const float* noise2;  // explicit data draw [B, D], or NULL for the Philox stream
  int mtab_bdim;
  int64_t HW;           // colorize: pixels per channel, D == 3 * HW
  float M[9], invM[9];  // colorize: decouple / couple matrices, row major [i][j]
};

__device__ inline const float* mtab_row(const CondArgs& c, int step, int64_t b) {
  return c.mtab + ((int64_t)step * c.mtab_bdim + (c.mtab_bdim == 1 ? 0 : b)) * 2;
}

// controllable_generation.py:48-51.  x_mean is built from the projected x, not from the
// update's x_mean (the reference's own expression).
__device__ inline void project_inpaint(float xn, float data, float mask, float mc, float sd,
                                       float z2, float& xo, float& xmo) {
  const float md_mean = mc * data;
  const float md = md_mean + z2 * sd;
  const float keep = 1.0f - mask;
  xo = xn * keep + md * mask;
  xmo = xo * keep + md_mean * mask;
}

// out_j = sum_i in_i * M[i][j]  (einsum 'bihw,ij->bjhw')
__device__ inline void mat3(const float in[3], const float* M, float out[3]) {
#pragma unroll
  for (int j = 0; j < 3; ++j) out[j] = in[0] * M[j] + in[1] * M[3 + j] + in[2] * M[6 + j];
}

// controllable_generation.py:140-143 with mask = (1, 0, 0) over the channels: channel 0 of
// the decoupled image is replaced, channels 1 and 2 are kept.
__device__ inline void project_colorize(const float xn[3], const float gray[3], const CondArgs& c,
                                        float mc, float sd, float z2, float xo[3], float xmo[3]) {
  float u[3], g[3], v[3];
  mat3(xn, c.M, u);
  mat3(gray, c.M, g);
  const float md_mean = mc * g[0];
  const float md = md_mean + z2 * sd;
  u[0] = u[0] * 0.0f + md * 1.0f;
  mat3(u, c.invM, xo);
  mat3(xo, c.M, v);
  v[0] = v[0] * 0.0f + md_mean * 1.0f;
  mat3(v, c.invM, xmo);
}

// One thread per element (none / inpaint) or per pixel over the 3 channels (colorize):
// `update(i, ge, b, xm, xn)` is the half-step's arithmetic for one element, the projection
// is applied to its xn before the only store of x_out / x_mean.
template <int COND, typename Update>
__device__ inline void update_project_store(float* x_out, float* __restrict__ x_mean, int B,
                                            int64_t D, int64_t sample_offset, int step,
                                            uint64_t seed, int draw, const CondArgs& c,
                                            Update update) {
  if constexpr (COND != BPK_COND_COLORIZE) {
    const int64_t total = (int64_t)B * D;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total;
         i += (int64_t)gridDim.x * blockDim.x) {
      const int64_t b = i / D;
      const int64_t ge = (sample_offset + b) * D + (i - b * D);
      float xm, xn;
      update(i, ge, b, xm, xn);
      if constexpr (COND == BPK_COND_INPAINT) {
        const float* mt = mtab_row(c, step, b);
        const float z2 = noise_at(c.noise2, i, ge, step, BPK_DATA_DRAW + draw, seed);
        project_inpaint(xn, c.data[i], c.mask[i], mt[0], mt[1], z2, xn, xm);
      }
      if (x_mean) x_mean[i] = xm;
      x_out[i] = xn;
    }
  } else {
    const int64_t pixels = (int64_t)B * c.HW;
    for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < pixels;
         p += (int64_t)gridDim.x * blockDim.x) {
      const int64_t b = p / c.HW;
      const int64_t i0 = b * D + (p - b * c.HW);
      const int64_t ge0 = (sample_offset + b) * D + (p - b * c.HW);
      float xn[3], gray[3], xo[3], xmo[3], unused;
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) {
        update(i0 + ch * c.HW, ge0 + ch * c.HW, b, unused, xn[ch]);
        gray[ch] = c.data[i0 + ch * c.HW];
      }
      const float* mt = mtab_row(c, step, b);
      const float z2 = noise_at(c.noise2, i0, ge0, step, BPK_DATA_DRAW + draw, seed);
      project_colorize(xn, gray, c, mt[0], mt[1], z2, xo, xmo);
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) {
        if (x_mean) x_mean[i0 + ch * c.HW] = xmo[ch];
        x_out[i0 + ch * c.HW] = xo[ch];
      }
    }
  }
}

template <int COND>
__global__ __launch_bounds__(256) void k_predictor(int kind, const float* x,
                                                   const float* __restrict__ m,
                                                   const float* __restrict__ noise,
                                                   float* x_out, float* __restrict__ x_mean,
                                                   int B, int64_t D, int64_t sample_offset,
                                                   const float* __restrict__ coef, int coef_bdim,
                                                   const int* __restrict__ step_ptr,
                                                   int score_mode, int drift_mul_x,
                                                   uint64_t seed, int draw, CondArgs c) {
  const int step = *step_ptr;
  update_project_store<COND>(
      x_out, x_mean, B, D, sample_offset, step, seed, draw, c,
      [=](int64_t i, int64_t ge, int64_t b, float& xm, float& xn) {
        const float* cf = coef_row(coef, coef_bdim, step, b);
        const float sdiv = cf[C_SDIV];
        const float xv = x[i];
        const float score = score_of(m[i], sdiv, score_mode);
        const float z = noise_at(noise, i, ge, step, draw, seed);
        if (kind == BPK_PRED_EULER_MARUYAMA) {
          // drift, diffusion = sde(x,t); drift = drift - diffusion**2 * score * 1.
          // x_mean = x + drift*dt; x = x_mean + (diffusion*sqrt(-dt)) * z
          const float diff = cf[C_DIFF];
          float drift = drift_mul_x ? cf[C_DRIFT] * xv : cf[C_DRIFT];
          const float diff2 = diff * diff;
          drift = drift - diff2 * score * 1.0f;
          xm = xv + drift * cf[C_DT];
          xn = xm + (diff * cf[C_SQRT_MDT]) * z;
        } else if (kind == BPK_PRED_REVERSE_DIFFUSION) {
          // VP: f = sqrt(alpha)*x - x ; VE: f = 0.  G = coef[DIFF]
          // rev_f = f - G**2 * score * 1. ; x_mean = x - rev_f ; x = x_mean + G*z
          const float G = cf[C_DIFF];
          const float f = drift_mul_x ? cf[C_DRIFT] * xv - xv : 0.0f;
          const float G2 = G * G;
          const float rev_f = f - G2 * score * 1.0f;
          xm = xv - rev_f;
          xn = xm + G * z;
        } else if (kind == BPK_PRED_ANCESTRAL_VP) {
          // x_mean = (x + beta*score) / sqrt(1-beta) ; x = x_mean + sqrt(beta)*noise
          xm = (xv + cf[C_DRIFT] * score) / cf[C_DIFF];
          xn = xm + cf[C_SQRT_MDT] * z;
        } else {  // ANCESTRAL_VE
          // x_mean = x + score*(sigma^2 - adj^2) ; x = x_mean + std*noise
          xm = xv + score * cf[C_DRIFT];
          xn = xm + cf[C_DIFF] * z;
        }
      });
}

// the half-steps whose update is None: (x, x) projected with fresh data noise
template <int COND>
__global__ __launch_bounds__(256) void k_project(const float* x, float* x_out,
                                                 float* __restrict__ x_mean, int B, int64_t D,
                                                 int64_t sample_offset,
                                                 const int* __restrict__ step_ptr, uint64_t seed,
                                                 int draw, CondArgs c) {
  const int step = *step_ptr;
  update_project_store<COND>(x_out, x_mean, B, D, sample_offset, step, seed, draw, c,
                             [=](int64_t i, int64_t, int64_t, float& xm, float& xn) {
                               xm = xn = x[i];
                             });
}

// ---- Langevin corrector
constexpr int kLgvThreads = 256;
constexpr int64_t kLgvChunk = 256 * 16;  // elements per (sample, chunk) workgroup

__global__ __launch_bounds__(kLgvThreads) void k_lgv_partial(
    const float* __restrict__ m, const float* __restrict__ noise, float* __restrict__ part,
    int64_t D, int chunks, int64_t sample_offset, const float* __restrict__ coef, int coef_bdim,
    const int* __restrict__ step_ptr, int score_mode, uint64_t seed, int draw) {
  __shared__ float sg[kLgvThreads / 64], sn[kLgvThreads / 64];
  const int step = *step_ptr;
  const int chunk = blockIdx.x;
  const int64_t b = blockIdx.y;
  const float sdiv = coef_row(coef, coef_bdim, step, b)[C_SDIV];
  const int64_t e0 = chunk * kLgvChunk;
  const int64_t e1 = std::min<int64_t>(D, e0 + kLgvChunk);
  float ag = 0.f, an = 0.f;
  for (int64_t e = e0 + threadIdx.x; e < e1; e += kLgvThreads) {
    const int64_t i = b * D + e;
    const float g = score_of(m[i], sdiv, score_mode);
    const float z = noise_at(noise, i, (sample_offset + b) * D + e, step, draw, seed);
    ag += g * g;
    an += z * z;
  }
  for (int off = 32; off > 0; off >>= 1) {
    ag += __shfl_xor(ag, off, 64);
    an += __shfl_xor(an, off, 64);
  }
  if ((threadIdx.x & 63) == 0) {
    sg[threadIdx.x >> 6] = ag;
    sn[threadIdx.x >> 6] = an;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    float tg = 0.f, tn = 0.f;
    for (int w = 0; w < kLgvThreads / 64; ++w) {
      tg += sg[w];
      tn += sn[w];
    }
    part[(b * chunks + chunk) * 2] = tg;
    part[(b * chunks + chunk) * 2 + 1] = tn;
  }
}

__global__ __launch_bounds__(256) void k_lgv_reduce(const float* __restrict__ part,
                                                    float* __restrict__ red, int B, int chunks) {
  __shared__ float sg[256], sn[256];
  float tg = 0.f, tn = 0.f;
  for (int b = threadIdx.x; b < B; b += 256) {
    float g = 0.f, n = 0.f;
    for (int c = 0; c < chunks; ++c) {
      g += part[((int64_t)b * chunks + c) * 2];
      n += part[((int64_t)b * chunks + c) * 2 + 1];
    }
    tg += sqrtf(g);
    tn += sqrtf(n);
  }
  sg[threadIdx.x] = tg;
  sn[threadIdx.x] = tn;
  __syncthreads();
  if (threadIdx.x == 0) {
    float a = 0.f, c = 0.f;
    for (int i = 0; i < 256; ++i) {
      a += sg[i];
      c += sn[i];
    }
    red[0] = a;
    red[1] = c;
  }
}

template <int COND>
__global__ __launch_bounds__(256) void k_lgv_update(
    int mode, const float* x, const float* __restrict__ m, const float* __restrict__ noise,
    const float* __restrict__ red, float* x_out, float* __restrict__ x_mean, int B, int64_t D,
    int B_global, int64_t sample_offset, const float* __restrict__ coef, int coef_bdim,
    const int* __restrict__ step_ptr, int score_mode, float snr, uint64_t seed, int draw,
    CondArgs c) {
  const int step = *step_ptr;
  float grad_norm = 0.f, noise_norm = 0.f;
  if (mode == 0) {
    grad_norm = red[0] / (float)B_global;
    noise_norm = red[1] / (float)B_global;
  }
  update_project_store<COND>(
      x_out, x_mean, B, D, sample_offset, step, seed, draw, c,
      [=](int64_t i, int64_t ge, int64_t b, float& xm, float& xn) {
        const float* cf = coef_row(coef, coef_bdim, step, b);
        const float alpha = cf[C_ALPHA];
        float step_size;
        if (mode == 0) {
          // (snr * noise_norm / grad_norm) ** 2 * 2 * alpha
          const float r = snr * noise_norm / grad_norm;
          step_size = r * r * 2.0f * alpha;
        } else {
          // (snr * std) ** 2 * 2 * alpha
          const float r = snr * cf[C_AUX];
          step_size = r * r * 2.0f * alpha;
        }
        const float nscale = sqrtf(step_size * 2.0f);
        const float g = score_of(m[i], cf[C_SDIV], score_mode);
        const float z = noise_at(noise, i, ge, step, draw, seed);
        xm = x[i] + step_size * g;
        xn = xm + nscale * z;
      });
}

__global__ void k_step_inc(int* step_ptr) { step_ptr[0] += 1; }

__global__ void k_fill(float* labels, int B, const float* table, const int* step_ptr) {
  const float v = table[*step_ptr];
  for (int b = threadIdx.x; b < B; b += blockDim.x) labels[b] = v;
}

unsigned blocks_for(int64_t total) {
  return (unsigned)std::max<int64_t>(1, std::min<int64_t>(bpk::ceil_div(total, 256), 256 * 32));
}

}  // namespace

extern "C" int bpk_philox_normal_f32(float* out, int B, int64_t D, int64_t sample_offset,
                                     uint64_t seed, const int* step_ptr, int draw, void* stream) {
  BPK_REQUIRE(B >= 0 && D >= 0, "philox_normal: bad shape");
  if ((int64_t)B * D == 0) return BPK_OK;
  hipLaunchKernelGGL(k_philox, dim3(blocks_for((int64_t)B * D)), dim3(256), 0,
                     bpk::as_stream(stream), out, B, D, sample_offset, seed, step_ptr, draw);
  BPK_LAUNCH_CHECK("philox_normal");
  return BPK_OK;
}

namespace {

// validates the projection's arguments and packs them; `mats` is HOST memory (18 floats:
// M then invM, row major), read here and passed to the kernel by value
int make_cond(const char* what, int cond, const float* data, const float* mask, const float* mtab,
              int mtab_bdim, const float* noise2, const float* mats, int B, int C, int64_t D,
              CondArgs* out) {
  CondArgs c{};
  BPK_REQUIRE(cond >= BPK_COND_NONE && cond <= BPK_COND_COLORIZE, "%s: unknown condition %d",
              what, cond);
  if (cond != BPK_COND_NONE) {
    BPK_REQUIRE(data && mtab, "%s: data and marginal table required", what);
    BPK_REQUIRE(mtab_bdim == 1 || mtab_bdim == B, "%s: marginal table batch dim %d must be 1 or %d",
                what, mtab_bdim, B);
    c.data = data;
    c.mtab = mtab;
    c.noise2 = noise2;
    c.mtab_bdim = mtab_bdim;
  }
  if (cond == BPK_COND_INPAINT) {
    BPK_REQUIRE(mask, "%s: inpainting needs a mask", what);
    c.mask = mask;
  }
  if (cond == BPK_COND_COLORIZE) {
    BPK_REQUIRE(C == 3, "%s: colorization needs 3 channels, got %d", what, C);
    BPK_REQUIRE(D % 3 == 0, "%s: D = %lld is not 3 * H * W", what, (long long)D);
    BPK_REQUIRE(mats, "%s: colorization needs the decouple / couple matrices", what);
    c.HW = D / 3;
    for (int k = 0; k < 9; ++k) {
      c.M[k] = mats[k];
      c.invM[k] = mats[9 + k];
    }
  }
  *out = c;
  return BPK_OK;
}

// threads of a launch: one per element, or per pixel for colorize
int64_t cond_threads(int cond, int B, int64_t D) {
  return cond == BPK_COND_COLORIZE ? (int64_t)B * (D / 3) : (int64_t)B * D;
}

#define BPK_COND_DISPATCH(cond, KERNEL, ...)                                         \
  do {                                                                               \
    if ((cond) == BPK_COND_NONE)                                                     \
      hipLaunchKernelGGL(KERNEL<BPK_COND_NONE>, __VA_ARGS__);                        \
    else if ((cond) == BPK_COND_INPAINT)                                             \
      hipLaunchKernelGGL(KERNEL<BPK_COND_INPAINT>, __VA_ARGS__);                     \
    else                                                                             \
      hipLaunchKernelGGL(KERNEL<BPK_COND_COLORIZE>, __VA_ARGS__);                    \
  } while (0)

int launch_predictor(const char* what, int cond, const CondArgs& c, int kind, const float* x,
                     const float* model_out, const float* noise, float* x_out, float* x_mean,
                     int B, int64_t D, int64_t sample_offset, const float* coef, int coef_bdim,
                     const int* step_ptr, int score_mode, int drift_mul_x, uint64_t seed, int draw,
                     void* stream) {
  BPK_REQUIRE(kind >= 0 && kind <= 3, "%s: unknown kind %d", what, kind);
  BPK_REQUIRE(score_mode == 0 || score_mode == 1, "%s: bad score_mode", what);
  BPK_REQUIRE(coef && step_ptr, "%s: coef table and step counter required", what);
  BPK_REQUIRE(B >= 0 && D >= 0, "%s: bad shape", what);
  if ((int64_t)B * D == 0) return BPK_OK;
  BPK_COND_DISPATCH(cond, k_predictor, dim3(blocks_for(cond_threads(cond, B, D))), dim3(256), 0,
                    bpk::as_stream(stream), kind, x, model_out, noise, x_out, x_mean, B, D,
                    sample_offset, coef, coef_bdim, step_ptr, score_mode, drift_mul_x, seed, draw,
                    c);
  BPK_LAUNCH_CHECK(what);
  return BPK_OK;
}

int launch_lgv_update(const char* what, int cond, const CondArgs& c, int mode, const float* x,
                      const float* model_out, const float* noise, const float* red, float* x_out,
                      float* x_mean, int B, int64_t D, int B_global, int64_t sample_offset,
                      const float* coef, int coef_bdim, const int* step_ptr, int score_mode,
                      float snr, uint64_t seed, int draw, void* stream) {
  BPK_REQUIRE(mode == 0 || mode == 1, "%s: mode must be 0 or 1", what);
  BPK_REQUIRE(coef && step_ptr && (mode == 1 || red), "%s: missing inputs", what);
  BPK_REQUIRE(B >= 0 && D >= 0 && B_global > 0, "%s: bad shape", what);
  if ((int64_t)B * D == 0) return BPK_OK;
  BPK_COND_DISPATCH(cond, k_lgv_update, dim3(blocks_for(cond_threads(cond, B, D))), dim3(256), 0,
                    bpk::as_stream(stream), mode, x, model_out, noise, red, x_out, x_mean, B, D,
                    B_global, sample_offset, coef, coef_bdim, step_ptr, score_mode, snr, seed,
                    draw, c);
  BPK_LAUNCH_CHECK(what);
  return BPK_OK;
}

}  // namespace

extern "C" int bpk_pc_predictor_f32(int kind, const float* x, const float* model_out,
                                    const float* noise, float* x_out, float* x_mean, int B,
                                    int64_t D, int64_t sample_offset, const float* coef,
                                    int coef_bdim, const int* step_ptr, int score_mode,
                                    int drift_mul_x, uint64_t seed, int draw, void* stream) {
  return launch_predictor("pc_predictor", BPK_COND_NONE, CondArgs{}, kind, x, model_out, noise,
                          x_out, x_mean, B, D, sample_offset, coef, coef_bdim, step_ptr,
                          score_mode, drift_mul_x, seed, draw, stream);
}

extern "C" int bpk_pc_predictor_cond_f32(int cond, int kind, const float* x,
                                         const float* model_out, const float* noise,
                                         const float* noise2, float* x_out, float* x_mean,
                                         const float* data, const float* mask, const float* mtab,
                                         int mtab_bdim, const float* mats, int B, int C, int64_t D,
                                         int64_t sample_offset, const float* coef, int coef_bdim,
                                         const int* step_ptr, int score_mode, int drift_mul_x,
                                         uint64_t seed, int draw, void* stream) {
  CondArgs c;
  if (int rc = make_cond("pc_predictor_cond", cond, data, mask, mtab, mtab_bdim, noise2, mats, B,
                         C, D, &c))
    return rc;
  return launch_predictor("pc_predictor_cond", cond, c, kind, x, model_out, noise, x_out, x_mean,
                          B, D, sample_offset, coef, coef_bdim, step_ptr, score_mode, drift_mul_x,
                          seed, draw, stream);
}

extern "C" int bpk_pc_project_f32(int cond, const float* x, const float* noise2, float* x_out,
                                  float* x_mean, const float* data, const float* mask,
                                  const float* mtab, int mtab_bdim, const float* mats, int B,
                                  int C, int64_t D, int64_t sample_offset, const int* step_ptr,
                                  uint64_t seed, int draw, void* stream) {
  BPK_REQUIRE(cond == BPK_COND_INPAINT || cond == BPK_COND_COLORIZE,
              "pc_project: condition must be inpaint or colorize, got %d", cond);
  CondArgs c;
  if (int rc = make_cond("pc_project", cond, data, mask, mtab, mtab_bdim, noise2, mats, B, C, D,
                         &c))
    return rc;
  BPK_REQUIRE(x && x_out && step_ptr, "pc_project: x, x_out and step counter required");
  BPK_REQUIRE(B >= 0 && D >= 0, "pc_project: bad shape");
  if ((int64_t)B * D == 0) return BPK_OK;
  const dim3 grid(blocks_for(cond_threads(cond, B, D)));
  if (cond == BPK_COND_INPAINT)
    hipLaunchKernelGGL(k_project<BPK_COND_INPAINT>, grid, dim3(256), 0, bpk::as_stream(stream), x,
                       x_out, x_mean, B, D, sample_offset, step_ptr, seed, draw, c);
  else
    hipLaunchKernelGGL(k_project<BPK_COND_COLORIZE>, grid, dim3(256), 0, bpk::as_stream(stream), x,
                       x_out, x_mean, B, D, sample_offset, step_ptr, seed, draw, c);
  BPK_LAUNCH_CHECK("pc_project");
  return BPK_OK;
}

extern "C" int64_t bpk_langevin_workspace_bytes(int B, int64_t D) {
  if (B <= 0 || D <= 0) return 0;
  return (int64_t)B * bpk::ceil_div(D, kLgvChunk) * 2 * (int64_t)sizeof(float);
}

extern "C" int bpk_langevin_partial_f32(const float* model_out, const float* noise,
                                        void* workspace, int B, int64_t D, int64_t sample_offset,
                                        const float* coef, int coef_bdim, const int* step_ptr,
                                        int score_mode, uint64_t seed, int draw, void* stream) {
  BPK_REQUIRE(workspace && coef && step_ptr, "langevin_partial: workspace/coef/step required");
  BPK_REQUIRE(B > 0 && D > 0 && B <= 65535, "langevin_partial: bad shape");
  const int chunks = (int)bpk::ceil_div(D, kLgvChunk);
  hipLaunchKernelGGL(k_lgv_partial, dim3(chunks, B), dim3(kLgvThreads), 0, bpk::as_stream(stream),
                     model_out, noise, static_cast<float*>(workspace), D, chunks, sample_offset,
                     coef, coef_bdim, step_ptr, score_mode, seed, draw);
  BPK_LAUNCH_CHECK("langevin_partial");
  return BPK_OK;
}

extern "C" int bpk_langevin_reduce_f32(void* workspace, float* red, int B, int64_t D,
                                       void* stream) {
  BPK_REQUIRE(workspace && red, "langevin_reduce: workspace/red required");
  BPK_REQUIRE(B > 0 && D > 0, "langevin_reduce: bad shape");
  const int chunks = (int)bpk::ceil_div(D, kLgvChunk);
  hipLaunchKernelGGL(k_lgv_reduce, dim3(1), dim3(256), 0, bpk::as_stream(stream),
                     static_cast<const float*>(workspace), red, B, chunks);
  BPK_LAUNCH_CHECK("langevin_reduce");
  return BPK_OK;
}

extern "C" int bpk_langevin_update_f32(int mode, const float* x, const float* model_out,
                                       const float* noise, const float* red, float* x_out,
                                       float* x_mean, int B, int64_t D, int B_global,
                                       int64_t sample_offset, const float* coef, int coef_bdim,
                                       const int* step_ptr, int score_mode, float snr,
                                       uint64_t seed, int draw, void* stream) {
  return launch_lgv_update("langevin_update", BPK_COND_NONE, CondArgs{}, mode, x, model_out, noise,
                           red, x_out, x_mean, B, D, B_global, sample_offset, coef, coef_bdim,
                           step_ptr, score_mode, snr, seed, draw, stream);
}

extern "C" int bpk_langevin_update_cond_f32(int cond, int mode, const float* x,
                                            const float* model_out, const float* noise,
                                            const float* noise2, const float* red, float* x_out,
                                            float* x_mean, const float* data, const float* mask,
                                            const float* mtab, int mtab_bdim, const float* mats,
                                            int B, int C, int64_t D, int B_global,
                                            int64_t sample_offset, const float* coef,
                                            int coef_bdim, const int* step_ptr, int score_mode,
                                            float snr, uint64_t seed, int draw, void* stream) {
  CondArgs c;
  if (int rc = make_cond("langevin_update_cond", cond, data, mask, mtab, mtab_bdim, noise2, mats,
                         B, C, D, &c))
    return rc;
  return launch_lgv_update("langevin_update_cond", cond, c, mode, x, model_out, noise, red, x_out,
                           x_mean, B, D, B_global, sample_offset, coef, coef_bdim, step_ptr,
                           score_mode, snr, seed, draw, stream);
}

extern "C" int bpk_step_increment(int* step_ptr, void* stream) {
  BPK_REQUIRE(step_ptr, "step_increment: null counter");
  hipLaunchKernelGGL(k_step_inc, dim3(1), dim3(1), 0, bpk::as_stream(stream), step_ptr);
  BPK_LAUNCH_CHECK("step_increment");
  return BPK_OK;
}

extern "C" int bpk_fill_step_scalar_f32(float* labels, int B, const float* table,
                                        const int* step_ptr, void* stream) {
  BPK_REQUIRE(labels && table && step_ptr && B >= 0, "fill_step_scalar: bad args");
  if (B == 0) return BPK_OK;
  hipLaunchKernelGGL(k_fill, dim3(1), dim3(256), 0, bpk::as_stream(stream), labels, B, table,
                     step_ptr);
  BPK_LAUNCH_CHECK("fill_step_scalar");
  return BPK_OK;
}
