// 3x3 / stride 1 / pad 1 fp32 convolution as fused Winograd F(2x2, 3x3) on the
// f32-input MFMA (v_mfma_f32_16x16x4_f32) for gfx950.
//
// The score networks' convolutions (models/layerspp.py, layers.py: every 3x3 conv of
// NCSN++ / DDPM++) are ~99 % of their FLOPs.  Winograd F(2,3) computes a 2x2 output
// tile from a 4x4 input tile with 16 multiplies per (cin, cout) instead of 36:
//     Y = A^T [ sum_cin (G g G^T) .* (B^T d B) ] A
// so for each of the 16 transform positions the contraction over cin is a GEMM
//     M_pos[tile, cout] = sum_cin V_pos[tile, cin] * U_pos[cin, cout]
// which runs on MFMA with exact f32 products (a k-ordered fma chain).
//
// Every form works on one 8 x 16-pixel region of one image per workgroup, a wave owning 16
// output channels: the input patch (10 x 18 per cin) goes to LDS, is transformed to V in LDS,
// and the waves run the MFMAs against U operands prefetched from global memory; the output
// transform is lane-local and stores straight from registers.  A GroupNorm+SiLU prologue
// (PRE) needs the per-channel table in LDS: at most kPreMaxCin input channels.  The forms,
// and when the host (wino_ex, wino_splitk, k16_launch) picks each:
//   * wino_f23_pipe_kernel -- 8-cin chunks, software-pipelined, 4 waves x 64 couts, or 8
//     waves x 128 couts for a prologue conv without a residual tail whose padded Cout is a
//     multiple of 128: the shapes the 16-cin forms do not take (Cin or C1 % 16 != 0, padded
//     Cout % 128 != 0);
//   * wino_f23_k16_kernel (k16_item) -- 16-cin chunks, 8 waves x 128 couts, persistent over
//     the items: padded Cout % 128 == 0 and Cin, C1 % 16 == 0 with an F(2x2) filter (every
//     backward-data conv, bpk_conv3x3_wino_up2_f32); its PAIR instantiation puts two
//     8-pixel-wide images side by side in a region (W == 8, CIFAR-10's 8 x 8 level);
//   * wino_f24_k16_kernel (k16_item24, wino_f24.h) -- the same item as F(2x4, 3x3): 24
//     points per 2 x 4 tile, 0.75 of the MFMAs; callers that hold a U24 filter ask for it
//     (bpk_conv3x3_wino_f24_*: the forward convs of the samplers);
//   * wino_splitk_reduce_kernel -- epilogue of a 16-cin launch split over the input
//     channels (wino_splits: launches that would leave most CUs idle).
// The filter transforms U = G g G^T (16 or 24 x cin x cout) are separate, tiny kernels;
// callers cache U while the weights do not change (sampling).
#include "bpk_common.h"
#include "wino_f24.h"

#include <algorithm>
#include <cstdlib>
#include <type_traits>

namespace {

using f4 = __attribute__((ext_vector_type(4))) float;

constexpr int kTR = 4, kTC = 8;          // tiles per region (rows, cols)
constexpr int kM = kTR * kTC;            // 32 tiles
constexpr int kPR = 2 * kTR + 2;         // 10 patch rows
constexpr int kPC = 2 * kTC + 2;         // 18 patch cols
// LDS row pitch of the input patch: 24 floats.  The V transform reads each 4 x 4 input tile
// as 8 ds_read_b64 at dword offsets 24 (2 ty + i) + 2 tx: per 32-lane group (one cin, 32
// tiles) the four tile rows land on dword banks {0-15, 48-63, 32-47, 16-31} (48 ty mod 64)
// -- all 64 banks once, conflict-free (a pitch of 19 with 16 ds_read_b32 was 2-way)
constexpr int kPCp = 24;
constexpr int kCK = 8;                   // cin per chunk
constexpr int kOutRows = 2 * kTR, kOutCols = 2 * kTC;  // 8 x 16 pixels

// U[cin][cout][pos] = (G g G^T)[pos] with G = [[1,0,0],[.5,.5,.5],[.5,-.5,.5],[0,0,1]]
// (the 16 positions of one (cin, cout) pair are contiguous: one lane of the GEMM loads
// its B operands for all positions with four 16-B loads)
// Cout not a multiple of 64: U is laid out for CoutP = Cout rounded up to 64 couts, the
// extra couts zero (the conv computes them and never stores them).
__device__ inline void wino_filter_range(const float* __restrict__ w, float* __restrict__ U,
                                         int Cin, int Cout, int CoutP, int ft, int64_t first,
                                         int64_t stride) {
  const int64_t total = (int64_t)Cin * CoutP;
  for (int64_t i = first; i < total; i += stride) {
    const int co = (int)(i % CoutP);
    const int ci = (int)(i / CoutP);
    if (co >= Cout) {
      f4* u = reinterpret_cast<f4*>(U + ((int64_t)ci * CoutP + co) * 16);
#pragma unroll
      for (int r = 0; r < 4; ++r) u[r] = f4{0.f, 0.f, 0.f, 0.f};
      continue;
    }
    // ft: the filter is flip_t(w) for w [Cin, Cout, 3, 3] (backward-data of the conv with
    // w): element (co, ci, r, s) = w[ci][co][2 - r][2 - s], read in place
    const float* g = ft ? w + ((int64_t)ci * Cout + co) * 9 : w + ((int64_t)co * Cin + ci) * 9;
    auto gv = [&](int k) { return ft ? g[8 - k] : g[k]; };
    float t[4][3];  // G g
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float g0 = gv(c), g1 = gv(3 + c), g2 = gv(6 + c);
      t[0][c] = g0;
      t[1][c] = 0.5f * (g0 + g1 + g2);
      t[2][c] = 0.5f * (g0 - g1 + g2);
      t[3][c] = g2;
    }
    float* u = U + ((int64_t)ci * CoutP + co) * 16;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float a0 = t[r][0], a1 = t[r][1], a2 = t[r][2];
      u[4 * r + 0] = a0;
      u[4 * r + 1] = 0.5f * (a0 + a1 + a2);
      u[4 * r + 2] = 0.5f * (a0 - a1 + a2);
      u[4 * r + 3] = a2;
    }
  }
}

__global__ __launch_bounds__(256) void wino_filter_kernel(const float* __restrict__ w,
                                                          float* __restrict__ U, int Cin,
                                                          int Cout, int CoutP, int ft) {
  wino_filter_range(w, U, Cin, Cout, CoutP, ft, (int64_t)blockIdx.x * blockDim.x + threadIdx.x,
                    (int64_t)gridDim.x * blockDim.x);
}

// many filters in one launch (op.conv.FilterBatch: every 3x3 conv weight of a model, forward
// and flipped, refreshed once per training step instead of one launch per conv call): job j =
// jobs[6 j .. 6 j + 5] = (w, U, Cin, Cout, CoutP, ft), blockIdx.y = j
__global__ __launch_bounds__(256) void wino_filter_batch_kernel(const int64_t* __restrict__ jobs) {
  const int64_t* jb = jobs + 6 * (int64_t)blockIdx.y;
  wino_filter_range(reinterpret_cast<const float*>(jb[0]), reinterpret_cast<float*>(jb[1]),
                    (int)jb[2], (int)jb[3], (int)jb[4], (int)jb[5],
                    (int64_t)blockIdx.x * blockDim.x + threadIdx.x,
                    (int64_t)gridDim.x * blockDim.x);
}

// U24 = G2 g G4^T of the F(2x4,3x3) form (wino_f24.h: computed in double, rounded once; point
// order 6 s + j of wino24_slot_row), 24 floats per (cin, cout) laid out per 16-cout group, same
// CoutP padding rule and ft meaning as wino_filter_range
__global__ __launch_bounds__(256) void wino_filter24_kernel(const float* __restrict__ w,
                                                            float* __restrict__ U, int Cin,
                                                            int Cout, int CoutP, int ft) {
  const int64_t total = (int64_t)Cin * CoutP;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += (int64_t)gridDim.x * blockDim.x) {
    const int co = (int)(i % CoutP);
    const int ci = (int)(i / CoutP);
    float u[24];
    if (co >= Cout) {
#pragma unroll
      for (int p = 0; p < 24; ++p) u[p] = 0.f;
    } else {
      const float* g = ft ? w + ((int64_t)ci * Cout + co) * 9 : w + ((int64_t)co * Cin + ci) * 9;
      float gg[9];
#pragma unroll
      for (int k = 0; k < 9; ++k) gg[k] = ft ? g[8 - k] : g[k];
      wino24_filter(gg, u);
    }
    // [cin][cout / 16][q][cout % 16][4]: the 16 couts of a wave's B fragment q are 256
    // contiguous bytes, so one buffer_load_b128 of the conv kernel reads 4 whole segments
    f4* dst = reinterpret_cast<f4*>(U) + ((int64_t)ci * (CoutP / 16) + co / 16) * 96 + co % 16;
#pragma unroll
    for (int q = 0; q < 6; ++q)
      dst[16 * q] = f4{u[4 * q], u[4 * q + 1], u[4 * q + 2], u[4 * q + 3]};
  }
}

struct WinoGeo {
  int N, Cin, Cout, H, W;
  int regions_x, regions_y, cout_blocks;
  float div;  // fused residual: y = (skip + (conv + bias)) / div when skip != nullptr
  int C1;     // input channels [0, C1) from x, [C1, Cin) from x2 (pipelined kernel only)
  int CoutS;  // couts stored (y, skip, stats channel count); Cout = CoutS rounded up to 64
  int up;     // 16-cin kernel only: 1 = x is [N, Cin, H/2, W/2], convolved as its nearest x2
              // upsample (the ddpm net's Upsample + Conv_0, reference layers.py:576-590)
  int ksplit; // 16-cin kernel only: > 1 = split-K over the input channels; workgroup s of a tile
              // contracts chunks [s, s + 1) * nch / ksplit and writes its raw partial output to
              // y + s * N * CoutS * H * W (no bias / tail / statistics: wino_splitk_reduce_kernel)
  int pair;   // 16-cin kernel only: 1 = W == 8, a region is two 8 x 8 images side by side
              // (images 2p, 2p + 1; regions_x = 1, N even, one source, no statistics)
};

constexpr int kVS = 20;                  // LDS stride of one (cin, tile) V record (16 + pad)
constexpr int kPreMaxCin = 1024;        // GroupNorm affine table in LDS

// PRE: the conv input is act(GroupNorm(x + b)) given as x and its per-(n, cin) affine form
// pre[n][cin] = (s, t) (bpk_group_norm_affine_f32): the patch load applies silu(x s + t)
// (zero padding stays zero), so the normalized tensor is never written to HBM.
// fast exp / reciprocal: a few ulp, far inside the network tolerance (1e-4)

__device__ inline float silu_f(float z) { return z * __builtin_amdgcn_rcpf(1.f + __expf(-z)); }

// q = a / d, r = a % d for a block index: a shift when d is a power of two (every NCSN++ /
// DDPM++ shape), else a 32-bit unsigned division -- the 64-bit forms were ~600 scalar
// instructions of the workgroup prologue
__device__ inline unsigned udivmod(unsigned a, unsigned d, unsigned& r) {
  if ((d & (d - 1)) == 0) {
    r = a & (d - 1);
    return a >> __builtin_ctz(d);
  }
  const unsigned q = a / d;
  r = a - q * d;
  return q;
}

// a / b correctly rounded (== IEEE division, bit for bit) from r = 1 / b (correctly rounded,
// computed once): q = a r, then one Markstein correction with the exact residual a - b q.
// 3 VALU instead of the ~10 of a full-range division (the residual tail divides by sqrt 2).
__device__ inline float div_rn(float a, float b, float r) {
  const float q = a * r;
  return fmaf(fmaf(-q, b, a), r, q);
}

template <int CTRL>
__device__ inline float dpp_f(float v) {
  return __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), CTRL, 0xF, 0xF, false));
}

// Chan merge of two equal-count partials (count c each); symmetric in its arguments, so both
// partners of a butterfly get the same bits
__device__ inline void merge_stats(float& m, float& m2, float mo, float m2o, float c) {
  const float d = mo - m;
  m2 = (m2 + m2o) + d * d * (0.5f * c);
  m = 0.5f * (m + mo);
}

// 4 x 4 transpose inside a DPP quad: lane t (= lane & 3) gives a[r] and gets a[s] = the a[t] of
// the quad's lane s.  Two butterfly steps (lanes xor 1 on the pairs (0, 1), (2, 3), then lanes
// xor 2 on (0, 2), (1, 3)): values are moved, never combined.
template <int CTRL>
__device__ inline void quad_swap(float& lo, float& hi, bool upper) {
  const float plo = dpp_f<CTRL>(lo), phi = dpp_f<CTRL>(hi);
  lo = upper ? phi : lo;
  hi = upper ? hi : plo;
}
__device__ inline void quad_transpose(float (&a)[4], int t) {
  quad_swap<0xB1>(a[0], a[1], t & 1);
  quad_swap<0xB1>(a[2], a[3], t & 1);
  quad_swap<0x4E>(a[0], a[2], t & 2);
  quad_swap<0x4E>(a[1], a[3], t & 2);
}

// Per-workgroup phase timestamps (diagnostic build only, -DWINO_TIMING; tools/wino_timing.py):
// wall clock (100 MHz) at entry, once the prologue's loads have landed, after the first patch
// stores, at the start of the chunk loop, after it and after the epilogue (wave 0's view), the
// shader clock at entry and exit (s_memtime, for the clock rate), and the XCC / SE / CU.
#ifdef WINO_TIMING
constexpr unsigned kTsMax = 1u << 17;
__device__ long long g_wino_ts[kTsMax][8];
__device__ unsigned g_wino_cu[kTsMax];
// WINO_TS_AT(rec, slot): the record index is the item where a workgroup walks several
// (k16_item24); WINO_TS(slot) keeps one record per workgroup.
#define WINO_TS_AT(rec, slot)                                                      \
  do {                                                                             \
    if (threadIdx.x == 0 && (rec) < kTsMax) {                                      \
      g_wino_ts[rec][slot] = wall_clock64();                                       \
      if (slot == 0) g_wino_cu[rec] = __smid();                                    \
      if (slot == 0 || slot == 5)                                                  \
        g_wino_ts[rec][6 + slot / 5] = (long long)__builtin_amdgcn_s_memtime();    \
    }                                                                              \
  } while (0)
#else
#define WINO_TS_AT(rec, slot) \
  do {                        \
  } while (0)
#endif
#define WINO_TS(slot) WINO_TS_AT(blockIdx.x, slot)

// Software-pipelined 8-cin form (32 tiles, 16 couts per wave).  A serial schedule runs
// store-patch | barrier | transform | barrier | MFMAs per chunk, so a wave's MFMA pipe idles
// through the transform phase.  Here the work of three chunks overlaps inside each wave:
// while the MFMAs of chunk k read V(k) from one LDS buffer, the same wave transforms
// patch(k+1) (already in LDS) into the other V buffer, stores patch(k+2) (in registers)
// into the free patch buffer and issues the global loads of patch(k+3) and of U(k+1) --
// one barrier per chunk.  The VALU / LDS work (~70
// instructions per chunk) fills MFMA issue gaps (64 MFMAs of 32 cycles per chunk per wave).
// WG = waves per workgroup: 4 (64 couts, two workgroups per CU) or 8 (128 couts, one
// workgroup per CU): the eight waves share one patch / V stream, so the GroupNorm+SiLU
// patch stores take 4 channels per thread instead of 8 (half the SiLU work per SIMD per MFMA
// of the two-workgroup form).
// TAIL (nch = Cin / 8 even and >= 4): the last three chunks are peeled so they skip the side
// work of chunks that do not exist (patch loads / stores, the V transform and the filter
// prefetch past the last chunk, and the last barrier) instead of redoing the last chunk's.
template <bool PRE, int WG = 4, bool TAIL = false>
__global__ __launch_bounds__(64 * WG, WG == 8 ? 1 : 2) void wino_f23_pipe_kernel(
    const float* __restrict__ x, const float* __restrict__ U, const float* __restrict__ bias,
    const float* __restrict__ skip, const float2* __restrict__ pre, float* __restrict__ y,
    float2* __restrict__ stats, WinoGeo g, int xcd_remap, const float* __restrict__ x2) {
  constexpr int kWN = 16;  // couts per wave
  constexpr int kPatch = kCK * kPR * kPCp;
  __shared__ __attribute__((aligned(16))) float s_patch_raw[2][kPatch];     // 2 x 7.5 KB
  constexpr int kVBuf = kCK * kM * kVS;                                      // 20.5 KB
  __shared__ __attribute__((aligned(16))) float s_v[2][kVBuf];              // V double buffer
  __shared__ float2 s_ss[PRE ? kPreMaxCin : 1];  // PRE: (s, t) of every input channel

  WINO_TS(0);
  const int tid = threadIdx.x;
  const int wave = tid >> 6, lane = tid & 63;
  // grid < 2^31 blocks (host check): 32-bit block arithmetic
  const unsigned nblk = gridDim.x;
  unsigned b = blockIdx.x;
  if (xcd_remap) b = (b & 7u) * (nblk >> 3) + (b >> 3);
  unsigned cb, rx, ry;
  unsigned r = udivmod(b, (unsigned)g.cout_blocks, cb);
  r = udivmod(r, (unsigned)g.regions_x, rx);
  const int n = (int)udivmod(r, (unsigned)g.regions_y, ry);
  const int oy0 = (int)ry * kOutRows, ox0 = (int)rx * kOutCols;
  const int cout_w = (int)cb * (WG * kWN) + wave * kWN;
  // 8 waves: waves 0-3 stage channels 0-3 of a chunk and transform V, waves 4-7 stage
  // channels 4-7 (wave-uniform, in SGPRs).  Every wave transforms (waves w and w + 4 write the
  // same V records, identical values): a wave-uniform branch around the transform, or waves
  // with split roles, made the compiler spill
  constexpr int kCT = kCK * 4 / WG;  // channels staged per thread
  const int phc = WG == 8 ? __builtin_amdgcn_readfirstlane(tid >> 8) : 0;

  // accumulators: the first chunk's k-step 0 MFMAs take an inline-constant zero C operand
  // (no 128 register clears in the prologue)
  f4 acc[16][2];

  const int64_t plane = (int64_t)g.H * g.W;
  const int C2 = g.Cin - g.C1;
  const float* xn = x + (int64_t)n * g.C1 * plane;
  const float2* pre_n = PRE ? pre + (int64_t)n * g.Cin : nullptr;
  const int kq = lane >> 4, jj = lane & 15;
  const int nch = g.Cin / kCK;

  // Global loads go through buffer descriptors (base in SGPRs, 32-bit per-lane offsets,
  // the chunk offset in soffset): no 64-bit address registers next to the accumulators.
  // Two sources (the up path's [h, skip] without their concatenation): channels [0, C1)
  // from x, [C1, Cin) from x2; a chunk never straddles (C1 % 8 == 0).
  const __amdgpu_buffer_rsrc_t xrs = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<float*>(xn), 0, (int)(g.C1 * plane * 4), 0x00020000);
  const __amdgpu_buffer_rsrc_t xrs2 = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<float*>(C2 > 0 ? x2 + (int64_t)n * C2 * plane : xn), 0,
      (int)((C2 > 0 ? C2 : g.C1) * plane * 4), 0x00020000);
  const __amdgpu_buffer_rsrc_t urs = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<float*>(U), 0, (int)((int64_t)g.Cin * g.Cout * 64), 0x00020000);

  // patch loads, position-major: thread t < 180 owns patch position (py, px) = (t / 18,
  // t % 18) for all 8 channels of a chunk (one in-plane offset, one LDS slot, one
  // in-image bit per thread; the channel stride goes into soffset / the LDS immediate).
  // Threads >= 180 duplicate thread 0 (same loads, same values to the same LDS words), so
  // every lane runs the same branch-free code.
  constexpr int kPos = kPR * kPC;  // 180
  int poff, pdst;
  bool pin;
  {
    const int t8 = tid & 255;
    const int t = t8 < kPos ? t8 : 0;
    const int py = t / kPC, px = t - py * kPC;
    const int iy = oy0 - 1 + py, ix = ox0 - 1 + px;
    pin = iy >= 0 && iy < g.H && ix >= 0 && ix < g.W;
    const int cy = min(max(iy, 0), g.H - 1), cx = min(max(ix, 0), g.W - 1);
    poff = (cy * g.W + cx) * 4;
    pdst = py * kPCp + px + phc * kCT * (kPR * kPCp);
  }
  float pv[kCT];
  auto load_patch = [&](int k) {
    const int cc = min(k, nch - 1) * kCK;
    const bool second = cc >= g.C1;
    const int soff = ((second ? cc - g.C1 : cc) + phc * kCT) * (int)plane * 4;
#pragma unroll
    for (int c = 0; c < kCT; ++c)
      pv[c] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(
          second ? xrs2 : xrs, poff, soff + c * (int)plane * 4, 0));
  };
  auto store_patch_from = [&](const float* src, float* sp, int k) {
    const int c0 = min(k, nch - 1) * kCK + phc * kCT;
#pragma unroll
    for (int c = 0; c < kCT; ++c) {
      float v = src[c];
      if (PRE) {
        const float2 st = s_ss[c0 + c];
        v = silu_f(v * st.x + st.y);
      }
      sp[pdst + c * (kPR * kPCp)] = pin ? v : 0.f;
    }
  };
  auto store_patch = [&](float* sp, int k) { store_patch_from(pv, sp, k); };
  // B operands of one k-step half: uo[ks][q] = U[c0 + 4ks + kq][cout_w + jj][4q..]
  f4 uo[2][4];
  const int uoff = ((kq * g.Cout + cout_w + jj) * 16) * 4;
  auto load_u = [&](int ks, int k) {
    const int soff = ((min(k, nch - 1) * kCK + 4 * ks) * g.Cout) * 64;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      using u4 = __attribute__((ext_vector_type(4))) unsigned;
      const u4 w = __builtin_amdgcn_raw_buffer_load_b128(urs, uoff + q * 16, soff, 0);
      uo[ks][q] = __builtin_bit_cast(f4, w);
    }
  };
  // V = B^T d B of one (cin, tile) per thread
  const int tc = (tid & 255) >> 5, tm = tid & 31;
  const int tty = tm / kTC, ttx = tm - tty * kTC;
  float d[4][4];
  auto read_d = [&](const float* sp) {
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; j += 2) {
        const float2 v2 =
            *reinterpret_cast<const float2*>(&sp[(tc * kPR + 2 * tty + i) * kPCp + 2 * ttx + j]);
        d[i][j] = v2.x;
        d[i][j + 1] = v2.y;
      }
  };
  auto write_v = [&](float* sv) {
    float t[4][4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      t[0][j] = d[0][j] - d[2][j];
      t[1][j] = d[1][j] + d[2][j];
      t[2][j] = d[2][j] - d[1][j];
      t[3][j] = d[1][j] - d[3][j];
    }
    f4* dst = reinterpret_cast<f4*>(&sv[(tc * kM + tm) * kVS]);
#pragma unroll
    for (int i = 0; i < 4; ++i)
      dst[i] = f4{t[i][0] - t[i][2], t[i][1] + t[i][2], t[i][2] - t[i][1], t[i][1] - t[i][3]};
  };

  // prologue: V(0) in s_v[0], patch(1) in s_patch[1], patch(2) and U(0) in flight.  The
  // global loads of patches 0-2, U(0) and the GroupNorm table are all issued before the
  // first wait, so a workgroup pays one memory latency here, not four.
  float pv0[kCT], pv1[kCT];
  load_patch(0);
#pragma unroll
  for (int c = 0; c < kCT; ++c) pv0[c] = pv[c];
  load_patch(1);
#pragma unroll
  for (int c = 0; c < kCT; ++c) pv1[c] = pv[c];
  load_patch(2);
  load_u(0, 0);
  load_u(1, 0);
  if (PRE) {
    for (int c = tid; c < g.Cin; c += 64 * WG) s_ss[c] = pre_n[c];
    __syncthreads();
  }
  WINO_TS(1);
  store_patch_from(pv0, s_patch_raw[0], 0);
  store_patch_from(pv1, s_patch_raw[1], 1);
  __syncthreads();
  WINO_TS(2);
  read_d(s_patch_raw[0]);
  write_v(s_v[0]);
  __syncthreads();

  // A operands a[q] = V[pos 4q..4q+3] of (ks, mb) = this lane's tile row of one LDS record;
  // each a[q] / uo[ks][q] register is refilled (next group's A, next chunk's U) right
  // after the last MFMA that reads it, so A needs 16 registers and U 32, and every load
  // has most of a group (>= 12 MFMAs) to land
  f4 a[4];
  auto a_src = [&](const float* sv, int grp) {  // grp = 2 ks + mb
    const int ks = grp >> 1, mb = grp & 1;
    return reinterpret_cast<const f4*>(&sv[((4 * ks + kq) * kM + mb * 16 + jj) * kVS]);
  };
  {
    const f4* src = a_src(s_v[0], 0);
#pragma unroll
    for (int q = 0; q < 4; ++q) a[q] = src[q];
  }
  // TM: 0 = full side work, 1 = no patch load (chunk nch - 3), 2 = no patch load / store
  // (nch - 2), 3 = the last chunk: no side work, no filter prefetch, no barrier
  auto step = [&](int k, auto sb_c, auto first_c, auto tm_c) __attribute__((always_inline)) {
    constexpr int SB = decltype(sb_c)::value;
    constexpr bool FIRST = decltype(first_c)::value;
    constexpr int TM = decltype(tm_c)::value;
    const float* sv = s_v[SB];
#pragma unroll
    for (int grp = 0; grp < 4; ++grp) {
      const int ks = grp >> 1, mb = grp & 1;
      // side work of the next chunks, spread over the four MFMA groups and fenced off from
      // the MFMAs (free / interleaved schedules measured slower, round 2)
      __builtin_amdgcn_sched_barrier(0);
      if (TM < 3 && grp == 0) read_d(s_patch_raw[SB ^ 1]);  // patch(k+1)
      if (TM < 3 && grp == 1) write_v(s_v[SB ^ 1]);         // V(k+1)
      if (TM < 2 && grp == 2) store_patch(s_patch_raw[SB], k + 2);  // patch(k+2)
      if (TM < 1 && grp == 3) load_patch(k + 3);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int q = 0; q < 4; ++q) {
#pragma unroll
        for (int pp = 0; pp < 4; ++pp)
          acc[4 * q + pp][mb] = __builtin_amdgcn_mfma_f32_16x16x4f32(
              a[q][pp], uo[ks][q][pp],
              (FIRST && ks == 0) ? f4{0.f, 0.f, 0.f, 0.f} : acc[4 * q + pp][mb], 0, 0, 0);
        // refill: A of the next group (the next chunk's group 0 comes after the barrier)
        if (grp < 3) a[q] = a_src(sv, grp + 1)[q];
        if (TM < 3 && mb == 1) {
          const int soff = ((min(k + 1, nch - 1) * kCK + 4 * ks) * g.Cout) * 64;
          using u4 = __attribute__((ext_vector_type(4))) unsigned;
          const u4 w = __builtin_amdgcn_raw_buffer_load_b128(urs, uoff + q * 16, soff, 0);
          uo[ks][q] = __builtin_bit_cast(f4, w);
        }
      }
    }
    if constexpr (TM < 3) {
      __syncthreads();
      const f4* src = a_src(s_v[SB ^ 1], 0);
#pragma unroll
      for (int q = 0; q < 4; ++q) a[q] = src[q];
    }
  };
  using C0 = std::integral_constant<int, 0>;
  using C1 = std::integral_constant<int, 1>;
  using F = std::false_type;
  WINO_TS(3);
  using T0 = std::integral_constant<int, 0>;
  auto run = [&]() __attribute__((always_inline)) {
    step(0, C0{}, std::true_type{}, T0{});
    int k = 1;
    if constexpr (TAIL) {  // nch even, >= 4: chunks nch - 3, nch - 2, nch - 1 have SB 1, 0, 1
      for (; k + 1 <= nch - 4; k += 2) {
        step(k, C1{}, F{}, T0{});
        step(k + 1, C0{}, F{}, T0{});
      }
      step(k, C1{}, F{}, std::integral_constant<int, 1>{});
      step(k + 1, C0{}, F{}, std::integral_constant<int, 2>{});
      step(k + 2, C1{}, F{}, std::integral_constant<int, 3>{});
    } else {
      for (; k + 1 < nch; k += 2) {
        step(k, C1{}, F{}, T0{});
        step(k + 1, C0{}, F{}, T0{});
      }
      if (k < nch) step(k, C1{}, F{}, T0{});
    }
  };
  // (one call site per instantiation: a second, dead one stopped the inliner and put the
  // accumulators in scratch)
  run();
  WINO_TS(4);

  // output transform straight from registers to global memory (no LDS staging, no
  // barrier).  Per M-block a lane holds tiles m = 16 mb + 4 kq + rg, rg = 0..3: tile row
  // 2 mb + kq / 2, tile cols 4 (kq & 1) + rg -- 2 output rows x 8 pixels of channel
  // cout_w + jj, stored as two 16-B strips per row (lanes kq, kq ^ 1 cover a whole
  // 64-B row).  GroupNorm partial statistics: a running Chan merge over the lane's 32
  // values, then the 4 lanes jj + 16 kq (equal counts, symmetric butterfly: same bits).
  const float rdiv = 1.f / g.div;
  // (a one-trip loop: written as `if (cout_w < g.CoutS)` the compiler orders the address
  // arithmetic of the statistics store differently; unmeasured, so the loop stays)
  for (int once = 0; once < 1; ++once) {
    if (cout_w >= g.CoutS) continue;  // padded couts (wave-uniform: CoutS % 16 == 0)
    const int co = cout_w + jj;
    const float bv = bias ? bias[co] : 0.f;
    const int64_t obase = ((int64_t)n * g.CoutS + co) * plane;
    float lm = 0.f, lm2 = 0.f;
#pragma unroll
    for (int mb = 0; mb < 2; ++mb) {
      const int oy = oy0 + 2 * (2 * mb + (kq >> 1));
      const int ox = ox0 + 8 * (kq & 1);
#pragma unroll
      for (int h = 0; h < 2; ++h) {
#pragma unroll
        for (int e = 0; e < 2; ++e) {
          f4 v;
#pragma unroll
          for (int u = 0; u < 2; ++u) {
            const int rg = 2 * e + u;
            float t[4];  // row h of A^T M, A^T = [[1,1,1,0],[0,1,-1,-1]]
#pragma unroll
            for (int j = 0; j < 4; ++j)
              t[j] = h == 0 ? acc[j][mb][rg] + acc[4 + j][mb][rg] + acc[8 + j][mb][rg]
                            : acc[4 + j][mb][rg] - acc[8 + j][mb][rg] - acc[12 + j][mb][rg];
            v[2 * u] = t[0] + t[1] + t[2] + bv;
            v[2 * u + 1] = t[1] - t[2] - t[3] + bv;
          }
          const int64_t o = obase + (int64_t)(oy + h) * g.W + ox + 4 * e;
          if (skip) {  // residual block tail, bit-identical to bpk_residual_rescale_f32
            const f4 sk = *reinterpret_cast<const f4*>(&skip[o]);
#pragma unroll
            for (int c = 0; c < 4; ++c) v[c] = div_rn(sk[c] + v[c], g.div, rdiv);
          }
          *reinterpret_cast<f4*>(&y[o]) = v;
          if (stats) {  // strip s = 4 mb + 2 h + e joins the s strips (4 s values) before it
            const float sm = ((v[0] + v[1]) + (v[2] + v[3])) * 0.25f;
            float sm2 = 0.f;
#pragma unroll
            for (int c = 0; c < 4; ++c) sm2 = fmaf(v[c] - sm, v[c] - sm, sm2);
            constexpr float kW[8] = {1.f, 1.f / 2, 1.f / 3, 1.f / 4, 1.f / 5, 1.f / 6, 1.f / 7, 1.f / 8};
            const int st = 4 * mb + 2 * h + e;
            const float d = sm - lm;
            lm = lm + d * kW[st];
            lm2 = (lm2 + sm2) + d * d * (4.f * st * kW[st]);
          }
        }
      }
    }
    if (stats) {
      merge_stats(lm, lm2, __shfl_xor(lm, 16, 64), __shfl_xor(lm2, 16, 64), 32.f);
      merge_stats(lm, lm2, __shfl_xor(lm, 32, 64), __shfl_xor(lm2, 32, 64), 64.f);
      if (kq == 0) {
        const int R = g.regions_x * g.regions_y;
        const int region = (oy0 / kOutRows) * g.regions_x + ox0 / kOutCols;
        stats[((int64_t)n * g.CoutS + co) * R + region] = make_float2(lm, lm2);
      }
    }
  }
  WINO_TS(5);
}

// 16-cin chunk form of the 8-wave pipelined kernel (one workgroup per CU, 8 waves x 16 couts =
// 128 couts, 32 tiles).  With 8-cin chunks the 8 waves transform the 256 (cin, tile) records of
// a chunk twice (waves w and w + 4 write identical V records: a wave-uniform branch around the
// transform made the compiler spill) and meet at a barrier every 64 MFMAs per wave.  Here a
// chunk is 16 input channels: the 512 threads own one (cin, tile) record each (no duplicate
// transform), every thread stages 8 channels of the patch (as the 4-wave form), and each wave
// issues 128 MFMAs per barrier; the side work of a chunk spreads over 8 MFMA groups.  The B
// operands (U) keep two k-step slots in registers: the slot a group has just finished is
// refilled with the k-step two ahead (next chunk's for the last two), one group pair before use.
// LDS: 2 x 15 KB patches + 2 x 40 KB V + the GroupNorm table (8 KB) = 118 KB.
// PAIR (images 8 pixels wide: CIFAR-10's 8 x 8 level): the 8 x 16-pixel region holds the same
// 8 rows of two images side by side -- tile columns 0-3 of image 2p, 4-7 of image 2p + 1 --
// and the patch is 10 x 20 (each image with its own one-pixel halo: columns 0-9 and 10-19), so
// the 3x3 convs of 8 x 8 feature maps run at the full 32-tile region instead of on the
// implicit GEMM.
template <bool PRE, bool PAIR>
__device__ __forceinline__ void k16_item(
    unsigned b, const float* __restrict__ x, const float* __restrict__ U,
    const float* __restrict__ bias, const float* __restrict__ skip,
    const float2* __restrict__ pre, float* __restrict__ y, float2* __restrict__ stats,
    const WinoGeo& g, const float* __restrict__ x2) {
  constexpr int CK = 16;
  constexpr int kPatch = CK * kPR * kPCp;
  __shared__ __attribute__((aligned(16))) float s_patch_raw[2][kPatch];
  constexpr int kVBuf = CK * kM * kVS;
  __shared__ __attribute__((aligned(16))) float s_v[2][kVBuf];
  __shared__ float2 s_ss[PRE ? kPreMaxCin : 1];

  WINO_TS(0);
  const int tid = threadIdx.x;
  const int wave = tid >> 6, lane = tid & 63;
  unsigned cb, rx, ry;
  unsigned r = udivmod(b, (unsigned)g.cout_blocks, cb);
  r = udivmod(r, (unsigned)g.regions_x, rx);
  r = udivmod(r, (unsigned)g.regions_y, ry);
  unsigned nn;
  // split-K slice (0 unless ksplit > 1); PAIR: nn = the image pair, n its first image
  const int ks_idx = (int)udivmod(r, (unsigned)(PAIR ? g.N >> 1 : g.N), nn);
  const int n = PAIR ? (int)nn * 2 : (int)nn;
  const int oy0 = (int)ry * kOutRows, ox0 = (int)rx * kOutCols;
  const int cout_w = (int)cb * 128 + wave * 16;
  const int ph = __builtin_amdgcn_readfirstlane(tid >> 8);  // channels 8 ph .. 8 ph + 7

  f4 acc[16][2];
  const int64_t plane = (int64_t)g.H * g.W;
  const int up = g.up;  // nearest x2 input: the patch reads x[iy >> 1][ix >> 1] of an H/2 x W/2 plane
  const int64_t xplane = plane >> (2 * up);
  const int C2 = g.Cin - g.C1;
  const float* xn = x + (int64_t)n * g.C1 * xplane;
  const float2* pre_n = PRE ? pre + (int64_t)n * g.Cin : nullptr;
  const int kq = lane >> 4, jj = lane & 15;
  const int nch = g.Cin / CK / max(g.ksplit, 1);  // chunks of this workgroup
  const int kb = ks_idx * nch;                    // its first chunk

  const __amdgpu_buffer_rsrc_t xrs = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<float*>(xn), 0, (int)(g.C1 * xplane * 4) << (PAIR ? 1 : 0), 0x00020000);
  const __amdgpu_buffer_rsrc_t xrs2 = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<float*>(C2 > 0 ? x2 + (int64_t)n * C2 * plane : xn), 0,
      (int)((C2 > 0 ? C2 : g.C1) * plane * 4), 0x00020000);
  const __amdgpu_buffer_rsrc_t urs = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<float*>(U), 0, (int)((int64_t)g.Cin * g.Cout * 64), 0x00020000);

  // 180 patch positions (PAIR: 200); threads beyond them in a half duplicate position 0
  constexpr int kCols = PAIR ? 2 * (kOutCols / 2 + 2) : kPC;
  constexpr int kPos = kPR * kCols;
  static_assert(kCols <= kPCp && kPos <= 256, "patch layout");
  int poff, pdst;
  bool pin;
  {
    const int t8 = tid & 255;
    const int t = t8 < kPos ? t8 : 0;
    const int py = t / kCols, px = t - py * kCols;
    const int img = PAIR && px >= kCols / 2;        // PAIR: second image of the region
    const int iy = oy0 - 1 + py, ix = ox0 - 1 + px - img * (kCols / 2);
    pin = iy >= 0 && iy < g.H && ix >= 0 && ix < g.W;
    const int cy = min(max(iy, 0), g.H - 1), cx = min(max(ix, 0), g.W - 1);
    poff = ((cy >> up) * (g.W >> up) + (cx >> up)) * 4 + img * (int)(g.C1 * xplane * 4);
    pdst = py * kPCp + px + ph * 8 * (kPR * kPCp);
  }
  float pv[8];
  auto load_patch_part = [&](float* dst, int k, int c0, int cn) {
    const int cc = (kb + min(k, nch - 1)) * CK;
    const bool second = cc >= g.C1;
    const int soff = ((second ? cc - g.C1 : cc) + ph * 8) * (int)xplane * 4;
#pragma unroll
    for (int c = c0; c < c0 + cn; ++c)
      dst[c] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(
          second ? xrs2 : xrs, poff, soff + c * (int)xplane * 4, 0));
  };
  // PAIR: the second image's GroupNorm table follows the first's in LDS
  const int ssoff = PAIR ? ((tid & 255) < kPos && ((tid & 255) % kCols) >= kCols / 2) * g.Cin : 0;
  auto store_patch_part = [&](const float* src, float* sp, int k, int c0, int cn) {
    const int cb0 = (kb + min(k, nch - 1)) * CK + ph * 8;
#pragma unroll
    for (int c = c0; c < c0 + cn; ++c) {
      float v = src[c];
      if (PRE) {
        const float2 st = s_ss[ssoff + cb0 + c];
        v = silu_f(v * st.x + st.y);
      }
      sp[pdst + c * (kPR * kPCp)] = pin ? v : 0.f;
    }
  };
  // B operands: uo[ks & 1][q] = U[c0 + 4 ks + kq][cout_w + jj][4q..4q + 3]
  f4 uo[2][4];
  const int uoff = ((kq * g.Cout + cout_w + jj) * 16) * 4;
  auto u_soff = [&](int k, int ks) {
    return (((kb + min(k, nch - 1)) * CK + 4 * ks) * g.Cout) * 64;
  };
  auto load_u = [&](int slot, int k, int ks) {
    const int soff = u_soff(k, ks);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      using u4 = __attribute__((ext_vector_type(4))) unsigned;
      const u4 w = __builtin_amdgcn_raw_buffer_load_b128(urs, uoff + q * 16, soff, 0);
      uo[slot][q] = __builtin_bit_cast(f4, w);
    }
  };
  // V = B^T d B of one (cin, tile) per thread (512 records = 16 cin x 32 tiles)
  const int tc = tid >> 5, tm = tid & 31;
  const int tty = tm / kTC, ttx = tm - tty * kTC;
  const int tcol = 2 * ttx + (PAIR ? 2 * (ttx >= kTC / 2) : 0);  // PAIR: past the first halo
  float d[4][4];
  auto read_d = [&](const float* sp) {
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; j += 2) {
        const float2 v2 =
            *reinterpret_cast<const float2*>(&sp[(tc * kPR + 2 * tty + i) * kPCp + tcol + j]);
        d[i][j] = v2.x;
        d[i][j + 1] = v2.y;
      }
  };
  auto write_v = [&](float* sv) {
    float t[4][4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      t[0][j] = d[0][j] - d[2][j];
      t[1][j] = d[1][j] + d[2][j];
      t[2][j] = d[2][j] - d[1][j];
      t[3][j] = d[1][j] - d[3][j];
    }
    f4* dst = reinterpret_cast<f4*>(&sv[(tc * kM + tm) * kVS]);
#pragma unroll
    for (int i = 0; i < 4; ++i)
      dst[i] = f4{t[i][0] - t[i][2], t[i][1] + t[i][2], t[i][2] - t[i][1], t[i][1] - t[i][3]};
  };

  // prologue: V(0) in s_v[0], patch(1) in s_patch[1], patch(2) and U(0) in flight
  {
    float pv0[8], pv1[8];
    load_patch_part(pv0, 0, 0, 8);
    load_patch_part(pv1, 1, 0, 8);
    load_patch_part(pv, 2, 0, 8);
    load_u(0, 0, 0);
    load_u(1, 0, 1);
    if (PRE) {
      for (int c = tid; c < (g.Cin << (PAIR ? 1 : 0)); c += 512) s_ss[c] = pre_n[c];
      __syncthreads();
    }
    WINO_TS(1);
    store_patch_part(pv0, s_patch_raw[0], 0, 0, 8);
    store_patch_part(pv1, s_patch_raw[1], 1, 0, 8);
  }
  __syncthreads();
  WINO_TS(2);
  read_d(s_patch_raw[0]);
  write_v(s_v[0]);
  __syncthreads();

  f4 a[4];
  auto a_src = [&](const float* sv, int grp) {  // grp = 2 ks + mb
    const int ks = grp >> 1, mb = grp & 1;
    return reinterpret_cast<const f4*>(&sv[((4 * ks + kq) * kM + mb * 16 + jj) * kVS]);
  };
  {
    const f4* src = a_src(s_v[0], 0);
#pragma unroll
    for (int q = 0; q < 4; ++q) a[q] = src[q];
  }
  auto step = [&](int k, auto sb_c, auto first_c) __attribute__((always_inline)) {
    constexpr int SB = decltype(sb_c)::value;
    constexpr bool FIRST = decltype(first_c)::value;
    const float* sv = s_v[SB];
#pragma unroll
    for (int grp = 0; grp < 8; ++grp) {
      const int ks = grp >> 1, mb = grp & 1;
      __builtin_amdgcn_sched_barrier(0);
      if (grp == 0) read_d(s_patch_raw[SB ^ 1]);                        // patch(k+1)
      if (grp == 1) write_v(s_v[SB ^ 1]);                               // V(k+1)
      if (grp == 2) store_patch_part(pv, s_patch_raw[SB], k + 2, 0, 4);  // patch(k+2)
      if (grp == 3) store_patch_part(pv, s_patch_raw[SB], k + 2, 4, 4);
      if (grp == 4) load_patch_part(pv, k + 3, 0, 4);
      if (grp == 5) load_patch_part(pv, k + 3, 4, 4);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int q = 0; q < 4; ++q) {
#pragma unroll
        for (int pp = 0; pp < 4; ++pp)
          acc[4 * q + pp][mb] = __builtin_amdgcn_mfma_f32_16x16x4f32(
              a[q][pp], uo[ks & 1][q][pp],
              (FIRST && ks == 0) ? f4{0.f, 0.f, 0.f, 0.f} : acc[4 * q + pp][mb], 0, 0, 0);
        if (grp < 7) a[q] = a_src(sv, grp + 1)[q];
        if (mb == 1) {  // k-step ks + 2 of this chunk, or ks - 2 of the next
          const int soff = ks < 2 ? u_soff(k, ks + 2) : u_soff(k + 1, ks - 2);
          using u4 = __attribute__((ext_vector_type(4))) unsigned;
          const u4 w = __builtin_amdgcn_raw_buffer_load_b128(urs, uoff + q * 16, soff, 0);
          uo[ks & 1][q] = __builtin_bit_cast(f4, w);
        }
      }
    }
    __syncthreads();
    const f4* src = a_src(s_v[SB ^ 1], 0);
#pragma unroll
    for (int q = 0; q < 4; ++q) a[q] = src[q];
  };
  using C0 = std::integral_constant<int, 0>;
  using C1 = std::integral_constant<int, 1>;
  WINO_TS(3);
  step(0, C0{}, std::true_type{});
  int k = 1;
  for (; k + 1 < nch; k += 2) {
    step(k, C1{}, std::false_type{});
    step(k + 1, C0{}, std::false_type{});
  }
  if (k < nch) step(k, C1{}, std::false_type{});
  WINO_TS(4);

  // output transform straight from registers (as wino_f23_pipe_kernel).  PAIR: a
  // lane's tile columns 4 (kq & 1) + rg all lie in image n + (kq & 1), at x 0..7
  const float rdiv = 1.f / g.div;
  if (cout_w < g.CoutS) {
    const int co = cout_w + jj;
    const float bv = bias ? bias[co] : 0.f;
    const int oimg = PAIR ? n + (kq & 1) : n;
    const int oxl = PAIR ? 0 : ox0 + 8 * (kq & 1);
    const int64_t obase = ((int64_t)(ks_idx * g.N + oimg) * g.CoutS + co) * plane;
    float lm = 0.f, lm2 = 0.f;
    // residual tail: all eight skip vectors of this lane requested before the first is used
    // (one exposed memory latency; loaded per store, the compiler waited for each in turn)
    f4 skv[2][2][2];
    if (skip) {
#pragma unroll
      for (int mb = 0; mb < 2; ++mb)
#pragma unroll
        for (int h = 0; h < 2; ++h)
#pragma unroll
          for (int e = 0; e < 2; ++e)
            skv[mb][h][e] = *reinterpret_cast<const f4*>(
                &skip[obase + (int64_t)(oy0 + 2 * (2 * mb + (kq >> 1)) + h) * g.W + oxl + 4 * e]);
    }
#pragma unroll
    for (int mb = 0; mb < 2; ++mb) {
      const int oy = oy0 + 2 * (2 * mb + (kq >> 1));
      const int ox = oxl;
#pragma unroll
      for (int h = 0; h < 2; ++h) {
#pragma unroll
        for (int e = 0; e < 2; ++e) {
          f4 v;
#pragma unroll
          for (int u = 0; u < 2; ++u) {
            const int rg = 2 * e + u;
            float t[4];
#pragma unroll
            for (int j = 0; j < 4; ++j)
              t[j] = h == 0 ? acc[j][mb][rg] + acc[4 + j][mb][rg] + acc[8 + j][mb][rg]
                            : acc[4 + j][mb][rg] - acc[8 + j][mb][rg] - acc[12 + j][mb][rg];
            v[2 * u] = t[0] + t[1] + t[2] + bv;
            v[2 * u + 1] = t[1] - t[2] - t[3] + bv;
          }
          const int64_t o = obase + (int64_t)(oy + h) * g.W + ox + 4 * e;
          if (skip) {
            const f4 sk = skv[mb][h][e];
#pragma unroll
            for (int c = 0; c < 4; ++c) v[c] = div_rn(sk[c] + v[c], g.div, rdiv);
          }
          *reinterpret_cast<f4*>(&y[o]) = v;
          if (!PAIR && stats) {
            const float sm = ((v[0] + v[1]) + (v[2] + v[3])) * 0.25f;
            float sm2 = 0.f;
#pragma unroll
            for (int c = 0; c < 4; ++c) sm2 = fmaf(v[c] - sm, v[c] - sm, sm2);
            constexpr float kW[8] = {1.f, 1.f / 2, 1.f / 3, 1.f / 4, 1.f / 5, 1.f / 6, 1.f / 7, 1.f / 8};
            const int st = 4 * mb + 2 * h + e;
            const float dd = sm - lm;
            lm = lm + dd * kW[st];
            lm2 = (lm2 + sm2) + dd * dd * (4.f * st * kW[st]);
          }
        }
      }
    }
    if (!PAIR && stats) {
      merge_stats(lm, lm2, __shfl_xor(lm, 16, 64), __shfl_xor(lm2, 16, 64), 32.f);
      merge_stats(lm, lm2, __shfl_xor(lm, 32, 64), __shfl_xor(lm2, 32, 64), 64.f);
      if (kq == 0) {
        const int R = g.regions_x * g.regions_y;
        const int region = (oy0 / kOutRows) * g.regions_x + ox0 / kOutCols;
        stats[((int64_t)n * g.CoutS + co) * R + region] = make_float2(lm, lm2);
      }
    }
  }
  WINO_TS(5);
}

// Persistent form (round 6): gridDim.x workgroups (one per CU, k16_launch) walk the items, so the
// dispatcher's workgroup turnaround (~1 us between one workgroup's exit and the next one's start
// on a CU, the round-4 timeline) is paid once per CU instead of once per item.  With xcd_remap
// the workgroups sharing an XCD (w, w + 8, ...: blocks are dealt round-robin over the 8 XCDs)
// walk one contiguous eighth of the items together, in order -- the order the dispatcher gave
// the one-workgroup-per-item launch: the cout blocks of a region and the neighbouring regions
// (their patch halos) are processed close in time on one XCD's L2.  Items do not overlap inside
// a workgroup (the register-staged overlap spilled); the barrier between
// items keeps the next prologue's LDS stores behind every wave's last reads of the previous one.
template <bool PRE, bool PAIR = false>
__global__ __launch_bounds__(512, 1) void wino_f23_k16_kernel(
    const float* __restrict__ x, const float* __restrict__ U, const float* __restrict__ bias,
    const float* __restrict__ skip, const float2* __restrict__ pre, float* __restrict__ y,
    float2* __restrict__ stats, WinoGeo g, int xcd_remap, const float* __restrict__ x2,
    unsigned items) {
  const unsigned G = gridDim.x, w = blockIdx.x;
  unsigned first = w, stride = G, end = items;
  if (xcd_remap) {  // G % 8 == 0: XCD label w % 8 owns items [start, start + count)
    const unsigned xc = w & 7u, q = items >> 3, r = items & 7u;
    const unsigned start = xc * q + min(xc, r);
    first = start + (w >> 3);
    stride = G >> 3;
    end = start + q + (xc < r ? 1u : 0u);
  }
  for (unsigned b = first; b < end; b += stride) {
    if (b != first) __syncthreads();
    k16_item<PRE, PAIR>(b, x, U, bias, skip, pre, y, stats, g, x2);
  }
}

// F(2x4,3x3) form of the 16-cin item (wino_f24.h): the same workgroup, region (8 x 16 pixels),
// 10 x 18 patch, GroupNorm+SiLU prologue, two-source switch, `up` addressing and split-K slicing
// as k16_item, but the region is 4 x 4 tiles of 2 rows x 4 columns -- 16 tiles, ONE M block of
// the 16x16x4 MFMA -- with 24 transform-domain points per tile: 24 points x 4 k-steps = 96 MFMAs
// per wave and chunk instead of 128 for the same pixels x cin x couts.
//   * V records: 16 cin x 16 tiles of 24 floats at a 28-float stride (28 i mod 64 over the 16
//     lanes of a ds_read_b128 group covers the 64 banks once): 2 x 28 KB.  Each thread owns half
//     a record: wave w transforms half h = w & 1 (slots 2 h, 2 h + 1: the F(2,3) row pass of
//     patch rows h .. h + 2, then the F(4,3) pass along both rows) of channels 4 kq + (w >> 1),
//     so a read group's two kq values sit 960 dwords apart (= 0 mod 64 banks).
//   * accumulators: acc[24] f4 = 96 registers.  The filter fragment is the MFMA's A operand and
//     the V fragment its B operand (both are held as index lane & 15, k = lane >> 4), so D is
//     [cout][tile]: lane (kq, jj) holds the 24 points of tile jj = 4 tty + ttx for the couts
//     cout_w + 4 kq + r, r = 0..3 -- after the output transform one f4 strip per (r, h).  The
//     four lanes of a quad (ttx) then write the 64 contiguous bytes of one region row: a wave's
//     store or skip load is 16 segments of 64 B (4 couts x 4 tile rows), not 64 pieces of 16 B
//     (measurements: profiles/wino_epilogue/).  The statistics keep the merge order of k16_item.
//   * U operands: uo[2][6] f4, one f4 per 4 MFMAs, refilled two k-steps ahead right after use;
//     U24 is laid out per 16-cout group and fragment so that a wave's load is 4 x 256 B.
// LDS: 2 x 15 KB patches + 2 x 28 KB V + the GroupNorm table (8 KB) = 94 KB.
// The item boundary (prologue, last steps) is kept short; none of this changes an operand or
// the order of an accumulation (measurements: profiles/r09_wino_boundary/):
//   * the prologue issues the GroupNorm table load first, then patch(0), then the rest, so the
//     first patch store waits for those two only (loads return in issue order); patch(1) is
//     activated after V(0) is written;
//   * the table in LDS is reloaded only when the image changes (Item24Carry::tab_n);
//   * TAILK, which the host picks for even chunk counts (every conv of the nets): steps
//     nch-3 .. nch-1 are peeled (TL 1..3) without the loads, patch stores, transform and filter
//     refills of chunks that do not exist; odd counts keep the full-step schedule;
//   * TAILK: the filter refills of the last step's k-steps 2 and 3 fetch k-steps 0 and 1 of
//     this slice's first chunk again, and the prologue of the workgroup's next item loads no
//     filter when that item has the same cout block and split-K slice (a scalar test, once per
//     item: Item24Carry::u_ready).
constexpr int kM24 = 16;   // tiles per region
constexpr int kVS24 = 28;  // LDS stride of one (cin, tile) V record (24 + pad)

// What one workgroup carries from item to item of its walk: the image whose table is in LDS
// and, when `u_ready`, the first two filter k-steps of the coming item in `uo`.
struct Item24Carry {
  f4 uo[2][6];
  int tab_n;
  bool u_ready;
};

// Timing diagnostic only (wrong results; tools/build_wino_timing.sh NAME
// -DWINO_F24_NO_SIDE_WORK=7): the chunk loop without its side work -- bit 0 the data transform
// (read_d, write_v), bit 1 the patch stores with the SiLU, bit 2 the patch loads.  Every MFMA,
// filter refill, V operand read, barrier, address and bound stays as it is, so the loop time of
// such a build is the floor that any placement of that work can reach
// (profiles/wino_interleave/README.md, section 2).
#ifndef WINO_F24_NO_SIDE_WORK
#define WINO_F24_NO_SIDE_WORK 0
#endif

template <bool PRE, bool TAILK>
__device__ __forceinline__ void k16_item24(
    unsigned b, unsigned nb, const float* __restrict__ x, const float* __restrict__ U,
    const float* __restrict__ bias, const float* __restrict__ skip,
    const float2* __restrict__ pre, float* __restrict__ y, float2* __restrict__ stats,
    const WinoGeo& g, const float* __restrict__ x2, Item24Carry& carry) {
  constexpr int kOob = (int)0x80000000u;  // buffer offset past every tensor: the load returns 0
                                          // and fetches nothing
  constexpr int CK = 16;
  constexpr int kPatch = CK * kPR * kPCp;
  __shared__ __attribute__((aligned(16))) float s_patch_raw[2][kPatch];
  constexpr int kVBuf = CK * kM24 * kVS24;
  __shared__ __attribute__((aligned(16))) float s_v[2][kVBuf];
  __shared__ float2 s_ss[PRE ? kPreMaxCin : 1];

  const int tid = threadIdx.x;
  const int wave = tid >> 6, lane = tid & 63;
  unsigned cb, rx, ry;
  unsigned r = udivmod(b, (unsigned)g.cout_blocks, cb);
  r = udivmod(r, (unsigned)g.regions_x, rx);
  r = udivmod(r, (unsigned)g.regions_y, ry);
  unsigned nn;
  const int ks_idx = (int)udivmod(r, (unsigned)g.N, nn);  // split-K slice (0 unless ksplit > 1)
  const int n = (int)nn;
  const int oy0 = (int)ry * kOutRows, ox0 = (int)rx * kOutCols;
  const int cout_w = (int)cb * 128 + wave * 16;
  const int ph = __builtin_amdgcn_readfirstlane(tid >> 8);  // channels 8 ph .. 8 ph + 7
  WINO_TS_AT(b, 0);
  // does the workgroup's next item (nb, ~0u = none) read the same filter slice as this one?
  bool u_next = false;
  if (TAILK && nb != ~0u) {
    unsigned cb2, t2;
    unsigned r2 = udivmod(nb, (unsigned)g.cout_blocks, cb2);
    r2 = udivmod(r2, (unsigned)g.regions_x, t2);
    r2 = udivmod(r2, (unsigned)g.regions_y, t2);
    u_next = cb2 == cb && (int)udivmod(r2, (unsigned)g.N, t2) == ks_idx;
  }

  f4 acc[24];
  const int64_t plane = (int64_t)g.H * g.W;
  const int up = g.up;
  const int64_t xplane = plane >> (2 * up);
  const int C2 = g.Cin - g.C1;
  const float* xn = x + (int64_t)n * g.C1 * xplane;
  const float2* pre_n = PRE ? pre + (int64_t)n * g.Cin : nullptr;
  const int kq = lane >> 4, jj = lane & 15;
  const int nch = g.Cin / CK / max(g.ksplit, 1);  // chunks of this workgroup
  const int kb = ks_idx * nch;                    // its first chunk

  const __amdgpu_buffer_rsrc_t xrs = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<float*>(xn), 0, (int)(g.C1 * xplane * 4), 0x00020000);
  const __amdgpu_buffer_rsrc_t xrs2 = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<float*>(C2 > 0 ? x2 + (int64_t)n * C2 * plane : xn), 0,
      (int)((C2 > 0 ? C2 : g.C1) * plane * 4), 0x00020000);
  const __amdgpu_buffer_rsrc_t urs = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<float*>(U), 0, (int)((int64_t)g.Cin * g.Cout * 96), 0x00020000);

  // 180 patch positions; threads beyond them in a half duplicate position 0 (as k16_item)
  constexpr int kPos = kPR * kPC;
  int poff, pdst;
  bool pin;
  {
    const int t8 = tid & 255;
    const int t = t8 < kPos ? t8 : 0;
    const int py = t / kPC, px = t - py * kPC;
    const int iy = oy0 - 1 + py, ix = ox0 - 1 + px;
    pin = iy >= 0 && iy < g.H && ix >= 0 && ix < g.W;
    const int cy = min(max(iy, 0), g.H - 1), cx = min(max(ix, 0), g.W - 1);
    poff = ((cy >> up) * (g.W >> up) + (cx >> up)) * 4;
    pdst = py * kPCp + px + ph * 8 * (kPR * kPCp);
  }
  float pv[8];
  // guard (the prologue of the TAILK form): a chunk past the last is requested out of range, which
  // fetches nothing and keeps the number of loads in flight the same for every nch
  auto load_patch_part = [&](float* dst, int k, int c0, int cn, bool guard = false) {
    const int cc = (kb + min(k, nch - 1)) * CK;
    const bool second = cc >= g.C1;
    const int soff = ((second ? cc - g.C1 : cc) + ph * 8) * (int)xplane * 4;
    const int po = (guard && k >= nch) ? kOob : poff;
#pragma unroll
    for (int c = c0; c < c0 + cn; ++c)
      dst[c] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(
          second ? xrs2 : xrs, po, soff + c * (int)xplane * 4, 0));
  };
  auto store_patch_part = [&](const float* src, float* sp, int k, int c0, int cn) {
    const int cb0 = (kb + min(k, nch - 1)) * CK + ph * 8;
#pragma unroll
    for (int c = c0; c < c0 + cn; ++c) {
      float v = src[c];
      if (PRE) {
        const float2 st = s_ss[cb0 + c];
        v = silu_f(v * st.x + st.y);
      }
      sp[pdst + c * (kPR * kPCp)] = pin ? v : 0.f;
    }
  };
  // filter operands (the MFMA's A, rows of D = couts): uo[ks & 1][q] = points 4q..4q + 3 of U24
  // (cin c0 + 4 ks + kq, cout cout_w + jj),
  // at [cin][cout_w / 16][q][jj] (wino_filter24_kernel): 256 contiguous bytes per kq
  f4(&uo)[2][6] = carry.uo;
  const int uoff = ((kq * g.Cout + cout_w) * 24 + jj * 4) * 4;
  // (wave-uniform by construction; said so, or the tail steps wrap every refill in an exec loop)
  auto u_soff = [&](int k, int ks) {
    return __builtin_amdgcn_readfirstlane((kb + min(k, nch - 1)) * 4 + ks) * (g.Cout * 384);
  };
  const int u_soff0[2] = {u_soff(0, 0), u_soff(0, 1)};
  auto load_u = [&](int slot, int k, int ks) {
    const int soff = u_soff(k, ks);
#pragma unroll
    for (int q = 0; q < 6; ++q)
      uo[slot][q] = __builtin_bit_cast(
          f4, __builtin_amdgcn_raw_buffer_load_b128(urs, uoff + q * 256, soff, 0));
  };
  // V = B2^T d B4: half th of the record (channel tc, tile jj) per thread
  const int th = __builtin_amdgcn_readfirstlane(wave & 1);
  const int tc = 4 * kq + (wave >> 1);
  const int tty = jj >> 2, ttx = jj & 3;
  float d[3][6];
  auto read_d = [&](const float* sp) {
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      const float* row = &sp[(tc * kPR + 2 * tty + th + i) * kPCp + 4 * ttx];
      const f4 v4 = *reinterpret_cast<const f4*>(row);
      const float2 v2 = *reinterpret_cast<const float2*>(row + 4);
      d[i][0] = v4[0];
      d[i][1] = v4[1];
      d[i][2] = v4[2];
      d[i][3] = v4[3];
      d[i][4] = v2.x;
      d[i][5] = v2.y;
    }
  };
  auto write_v = [&](float* sv) {
    float rx_[6], ry_[6], vx[6], vy[6];
#pragma unroll
    for (int j = 0; j < 6; ++j) wino24_data_rows(d[0][j], d[1][j], d[2][j], th, rx_[j], ry_[j]);
    wino24_data_cols(rx_, vx);
    wino24_data_cols(ry_, vy);
    f4* dst = reinterpret_cast<f4*>(&sv[(tc * kM24 + jj) * kVS24 + 12 * th]);
    dst[0] = f4{vx[0], vx[1], vx[2], vx[3]};
    dst[1] = f4{vx[4], vx[5], vy[0], vy[1]};
    dst[2] = f4{vy[2], vy[3], vy[4], vy[5]};
  };

  // prologue: V(0) in s_v[0], patch(1) in s_patch[1], patch(2) and U(0) in flight
  const bool tab_load = PRE && carry.tab_n != n;
  const bool u_have = TAILK && carry.u_ready;  // uo[0], uo[1] came with the previous item
  carry.tab_n = n;
  carry.u_ready = u_next;
  {
    // loads return in issue order: the table and patch(0), which the first stores need, go
    // first and the filter (98 KB per workgroup) last
    float pv0[8], pv1[8];
    float2 tv[kPreMaxCin / 512];
    if (tab_load) {
#pragma unroll
      for (int i = 0; i < kPreMaxCin / 512; ++i) tv[i] = pre_n[min(tid + 512 * i, g.Cin - 1)];
    }
    __builtin_amdgcn_sched_barrier(0);
    load_patch_part(pv0, 0, 0, 8);
    __builtin_amdgcn_sched_barrier(0);
    load_patch_part(pv1, 1, 0, 8, TAILK);
    load_patch_part(pv, 2, 0, 8, TAILK);
    // the filter only where the previous item did not fetch it: in place, under a branch, so
    // that no copy of uo (a wait for every load) is needed where the two cases join; the wait
    // for patch(0) below is exact for the common case, the one without these loads
    if (!u_have) {
      load_u(0, 0, 0);
      load_u(1, 0, 1);
    }
    __builtin_amdgcn_sched_barrier(0);
    if (tab_load) {
#pragma unroll
      for (int i = 0; i < kPreMaxCin / 512; ++i)
        if (tid + 512 * i < g.Cin) s_ss[tid + 512 * i] = tv[i];
      __syncthreads();
    }
    store_patch_part(pv0, s_patch_raw[0], 0, 0, 8);
    __syncthreads();
    read_d(s_patch_raw[0]);
    write_v(s_v[0]);
    if (!TAILK || nch > 1) store_patch_part(pv1, s_patch_raw[1], 1, 0, 8);  // for step 0
  }
  __syncthreads();
  WINO_TS_AT(b, 1);

  // V operands (the MFMA's B, columns of D = tiles): points 4q..4q + 3 of the record (cin
  // 4 ks + kq, tile jj), in a ring of four
  // registers quads over the chunk's 24 (ks, q) fragments: fragment i sits in a[i & 3] and is
  // replaced by fragment i + 4 right after its MFMAs (12 MFMAs before that one is used)
  f4 a[4];
  auto a_src = [&](const float* sv, int ks) {
    return reinterpret_cast<const f4*>(&sv[((4 * ks + kq) * kM24 + jj) * kVS24]);
  };
  {
    const f4* src = a_src(s_v[0], 0);
#pragma unroll
    for (int q = 0; q < 4; ++q) a[q] = src[q];
  }
  // TL (TAILK): 0 = a full step; 1 / 2 / 3 = step nch - 3 / nch - 2 / nch - 1, which has
  // no patch(k+3) to load / nor a patch(k+2) to store / nor any chunk k + 1
  auto step = [&](int k, auto sb_c, auto first_c, auto tail_c) __attribute__((always_inline)) {
    constexpr int SB = decltype(sb_c)::value;
    constexpr bool FIRST = decltype(first_c)::value;
    constexpr int TL = decltype(tail_c)::value;
    const float* sv = s_v[SB];
#pragma unroll
    for (int grp = 0; grp < 8; ++grp) {  // 12 MFMAs each: k-step grp / 2, points 12 (grp & 1) ..
      const int ks = grp >> 1, hf = grp & 1;
      // side work of the next chunks, fenced off from the MFMAs.  (Issued among the MFMAs --
      // one MFMA, then four or five vector instructions, by sched_group_barrier -- the loop
      // measured 3 % slower in this one-workgroup form too.  Its time is the MFMAs' cycles plus
      // the side work's issue cycles of both waves of a SIMD wherever that work stands:
      // profiles/wino_interleave/README.md, sections 2 and 3)
      __builtin_amdgcn_sched_barrier(0);
      constexpr int kOff = WINO_F24_NO_SIDE_WORK;
      if (grp == 0 && TL < 3 && !(kOff & 1)) read_d(s_patch_raw[SB ^ 1]);  // patch(k+1)
      if (grp == 1 && TL < 3 && !(kOff & 1)) write_v(s_v[SB ^ 1]);         // V(k+1)
      if (grp == 2 && TL < 2 && !(kOff & 2))
        store_patch_part(pv, s_patch_raw[SB], k + 2, 0, 4);  // patch(k+2)
      if (grp == 3 && TL < 2 && !(kOff & 2)) store_patch_part(pv, s_patch_raw[SB], k + 2, 4, 4);
      if (grp == 4 && TL < 1 && !(kOff & 4)) load_patch_part(pv, k + 3, 0, 4);
      if (grp == 5 && TL < 1 && !(kOff & 4)) load_patch_part(pv, k + 3, 4, 4);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int qq = 0; qq < 3; ++qq) {
        const int q = 3 * hf + qq;
        const int fi = 6 * ks + q;  // fragment index in the chunk
#pragma unroll
        for (int pp = 0; pp < 4; ++pp)
          acc[4 * q + pp] = __builtin_amdgcn_mfma_f32_16x16x4f32(
              uo[ks & 1][q][pp], a[fi & 3][pp],
              (FIRST && ks == 0) ? f4{0.f, 0.f, 0.f, 0.f} : acc[4 * q + pp], 0, 0, 0);
        if (fi + 4 < 24) a[fi & 3] = a_src(sv, (fi + 4) / 6)[(fi + 4) % 6];
        // k-step ks + 2 of this chunk, or ks - 2 of the next; after the last chunk (UNEXT) of
        // this slice's first chunk again, which is what the workgroup's next item starts with
        // when u_next (otherwise 98 KB read for nothing, once or twice per workgroup and launch)
        if (ks < 2 || TL < 3 || TAILK) {
          const int soff = ks < 2 ? u_soff(k, ks + 2)
                                  : (TL < 3 ? u_soff(k + 1, ks - 2) : u_soff0[ks - 2]);
          uo[ks & 1][q] = __builtin_bit_cast(
              f4, __builtin_amdgcn_raw_buffer_load_b128(urs, uoff + q * 256, soff, 0));
        }
      }
    }
    if (TL < 3) {  // after the last step comes the barrier between items, or nothing
      __syncthreads();
      const f4* src = a_src(s_v[SB ^ 1], 0);
#pragma unroll
      for (int q = 0; q < 4; ++q) a[q] = src[q];
    }
  };
  using C0 = std::integral_constant<int, 0>;
  using C1 = std::integral_constant<int, 1>;
  using T2 = std::integral_constant<int, 2>;
  using T3 = std::integral_constant<int, 3>;
  using Fi = std::true_type;
  using No = std::false_type;
  WINO_TS_AT(b, 2);
  if (!TAILK) {
    step(0, C0{}, Fi{}, C0{});
    int k = 1;
    for (; k + 1 < nch; k += 2) {
      step(k, C1{}, No{}, C0{});
      step(k + 1, C0{}, No{}, C0{});
    }
    if (k < nch) step(k, C1{}, No{}, C0{});
  } else {
    // TAILK: nch is even, so the last chunk sits in buffer 1 and the tail steps are one copy
    // of code on the one path out of the loop.  (With a copy per parity, or per small nch, the
    // compiler spilled the accumulators where the accumulating paths join; odd chunk counts
    // run the kernel's TAILK = false form.)  Full steps 0 .. nch - 4, then TAIL 1, 2, 3;
    // nch = 2 enters at TAIL 2 from zeroed accumulators, the same sums as FIRST's zero operand.
    if (nch >= 4) {
      step(0, C0{}, Fi{}, C0{});
      int k = 1;
      for (; k + 3 < nch; k += 2) {
        step(k, C1{}, No{}, C0{});
        step(k + 1, C0{}, No{}, C0{});
      }
    } else {
#pragma unroll
      for (int i = 0; i < 24; ++i) acc[i] = f4{0.f, 0.f, 0.f, 0.f};
    }
    // (a branch of its own: inside the block above this step cost the PRE form 24 B of scratch)
    if (nch >= 4) step(nch - 3, C1{}, No{}, C1{});
    step(nch - 2, C0{}, No{}, T2{});
    step(nch - 1, C1{}, No{}, T3{});
  }
  WINO_TS_AT(b, 3);

  // output transform straight from registers: lane (kq, jj = 4 tty + ttx) holds tile (tty, ttx)
  // of couts co0 .. co0 + 3 (register r): per (r, h) one f4 strip of output row oy0 + 2 tty + h,
  // so the four lanes of a quad write 64 contiguous bytes and a wave's store is 16 such segments
  const float rdiv = 1.f / g.div;
  if (cout_w < g.CoutS) {
    const int co0 = cout_w + 4 * kq;
    f4 bv = f4{0.f, 0.f, 0.f, 0.f};
    if (bias) bv = f4{bias[co0], bias[co0 + 1], bias[co0 + 2], bias[co0 + 3]};
    const int64_t obase = ((int64_t)(ks_idx * g.N + n) * g.CoutS + co0) * plane +
                          (int64_t)(oy0 + 2 * tty) * g.W + ox0 + 4 * ttx;
    float sm[2][4], sm2[2][4];  // strip (mean, M2) of (h, cout r)
    // residual tail: all eight skip vectors of this lane requested before the first is used
    f4 skv[4][2];
    if (skip) {
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int h = 0; h < 2; ++h)
#ifdef WINO_F24_EPI_ONE_STORE
          skv[r][h] = f4{0.f, 0.f, 0.f, 0.f};
#else
          skv[r][h] = *reinterpret_cast<const f4*>(&skip[obase + r * plane + (int64_t)h * g.W]);
#endif
    }
#ifdef WINO_F24_EPI_ONE_STORE
    // timing diagnostic only (wrong results; tools/build_wino_timing.sh NAME -D...=1): the eight
    // strips summed into one store per lane and no skip loads -- what is left of epilogue + gap
    // then is not the stores' or the loads' (profiles/wino_epilogue/README.md, section 1)
    f4 vsum = f4{0.f, 0.f, 0.f, 0.f};
#endif
#pragma unroll
    for (int r = 0; r < 4; ++r) {
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        float t[6], yv[4];
#pragma unroll
        for (int j = 0; j < 6; ++j)
          t[j] = wino24_out_rows(acc[j][r], acc[6 + j][r], acc[12 + j][r], acc[18 + j][r], h);
        wino24_out_cols(t, yv);
        f4 v = f4{yv[0] + bv[r], yv[1] + bv[r], yv[2] + bv[r], yv[3] + bv[r]};
        if (skip) {
          const f4 sk = skv[r][h];
#pragma unroll
          for (int c = 0; c < 4; ++c) v[c] = div_rn(sk[c] + v[c], g.div, rdiv);
        }
#ifdef WINO_F24_EPI_ONE_STORE
        vsum += v;
#else
        *reinterpret_cast<f4*>(&y[obase + r * plane + (int64_t)h * g.W]) = v;
#endif
        if (stats) {
          const float m = ((v[0] + v[1]) + (v[2] + v[3])) * 0.25f;
          float q = 0.f;
#pragma unroll
          for (int c = 0; c < 4; ++c) q = fmaf(v[c] - m, v[c] - m, q);
          sm[h][r] = m, sm2[h][r] = q;
        }
      }
    }
#ifdef WINO_F24_EPI_ONE_STORE
    *reinterpret_cast<f4*>(&y[obase]) = vsum;
#endif
    WINO_TS_AT(b, 4);
    if (stats) {
      // The eight strips of one cout and tile row sit in the quad's four lanes (ttx) x two h.
      // A 4 x 4 exchange inside the quad gives lane ttx the strips of cout co0 + ttx (sm[h][s]:
      // the strip of lane s), which it chains in the order st = 4 h + s (strip st joins the
      // 4 st values before it) -- the merge order of k16_item, so the records keep their bits.
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        quad_transpose(sm[h], ttx);
        quad_transpose(sm2[h], ttx);
      }
      constexpr float kW[8] = {1.f, 1.f / 2, 1.f / 3, 1.f / 4, 1.f / 5, 1.f / 6, 1.f / 7, 1.f / 8};
      float lm = 0.f, lm2 = 0.f;
#pragma unroll
      for (int st = 0; st < 8; ++st) {
        const float dd = sm[st >> 2][st & 3] - lm;
        lm = lm + dd * kW[st];
        lm2 = (lm2 + sm2[st >> 2][st & 3]) + dd * dd * (4.f * st * kW[st]);
      }
      // tile rows (0, 1), (2, 3), then the halves
      merge_stats(lm, lm2, __shfl_xor(lm, 4, 64), __shfl_xor(lm2, 4, 64), 32.f);
      merge_stats(lm, lm2, __shfl_xor(lm, 8, 64), __shfl_xor(lm2, 8, 64), 64.f);
      if (tty == 0) {
        const int R = g.regions_x * g.regions_y;
        const int region = (oy0 / kOutRows) * g.regions_x + ox0 / kOutCols;
        stats[((int64_t)n * g.CoutS + co0 + ttx) * R + region] = make_float2(lm, lm2);
      }
    }
  }
  WINO_TS_AT(b, 5);
}

// the persistent walk of wino_f23_k16_kernel over F(2x4,3x3) items
// TAILK: the chunk count per workgroup is even (k16_item24's peeled tail steps)
template <bool PRE, bool TAILK>
__global__ __launch_bounds__(512, 1) void wino_f24_k16_kernel(
    const float* __restrict__ x, const float* __restrict__ U, const float* __restrict__ bias,
    const float* __restrict__ skip, const float2* __restrict__ pre, float* __restrict__ y,
    float2* __restrict__ stats, WinoGeo g, int xcd_remap, const float* __restrict__ x2,
    unsigned items) {
  const unsigned G = gridDim.x, w = blockIdx.x;
  unsigned first = w, stride = G, end = items;
  if (xcd_remap) {  // G % 8 == 0: XCD label w % 8 owns items [start, start + count)
    const unsigned xc = w & 7u, q = items >> 3, r = items & 7u;
    const unsigned start = xc * q + min(xc, r);
    first = start + (w >> 3);
    stride = G >> 3;
    end = start + q + (xc < r ? 1u : 0u);
  }
  Item24Carry carry;
  carry.tab_n = -1;
  carry.u_ready = false;
  for (unsigned b = first; b < end; b += stride) {
    if (b != first) __syncthreads();
    const unsigned nb = b + stride < end ? b + stride : ~0u;
    k16_item24<PRE, TAILK>(b, nb, x, U, bias, skip, pre, y, stats, g, x2, carry);
  }
}

// Split-K epilogue: y = sum_s part[s] + bias, or (skip + that) / div, and the GroupNorm partial
// statistics of the stored values, as the 16-cin kernel's own epilogue (the partial slabs are
// summed in a fixed order: deterministic).  One workgroup = 8 channels x one 8 x 16 region of
// one image; a half-wave holds one channel's 128 values (8 rows x 4 float4), reduced over its
// 32 lanes by a butterfly of equal-count merges that gives every lane the same bits.
__global__ __launch_bounds__(256) void wino_splitk_reduce_kernel(
    const float* __restrict__ part, int S, const float* __restrict__ bias,
    const float* __restrict__ skip, float* __restrict__ y, float2* __restrict__ stats,
    WinoGeo g) {
  const int lane = threadIdx.x & 63;
  const int q = threadIdx.x;
  unsigned b = blockIdx.x, reg, cg;
  const unsigned R = (unsigned)(g.regions_x * g.regions_y);
  unsigned r = udivmod(b, R, reg);
  int n = (int)udivmod(r, (unsigned)(g.CoutS / 8), cg);
  const int co = (int)cg * 8 + (q >> 5);
  const int rem = q & 31;
  const int row = rem >> 2;
  int c4 = rem & 3;
  if (g.pair) {  // region = image pair n: columns 0-7 of image 2n, 8-15 of image 2n + 1
    n = 2 * n + (c4 >> 1);
    c4 &= 1;
  }
  const int oy0 = (int)(reg / g.regions_x) * kOutRows, ox0 = (int)(reg % g.regions_x) * kOutCols;
  const int64_t plane = (int64_t)g.H * g.W;
  const int64_t slab = (int64_t)g.N * g.CoutS * plane;
  const int64_t o = ((int64_t)n * g.CoutS + co) * plane + (int64_t)(oy0 + row) * g.W + ox0 + 4 * c4;
  f4 v = *reinterpret_cast<const f4*>(&part[o]);
  for (int s = 1; s < S; ++s) v += *reinterpret_cast<const f4*>(&part[s * slab + o]);
  const float bv = bias ? bias[co] : 0.f;
  v += f4{bv, bv, bv, bv};
  if (skip) {
    const f4 sk = *reinterpret_cast<const f4*>(&skip[o]);
    const float rdiv = 1.f / g.div;
#pragma unroll
    for (int c = 0; c < 4; ++c) v[c] = div_rn(sk[c] + v[c], g.div, rdiv);
  }
  *reinterpret_cast<f4*>(&y[o]) = v;
  if (!stats || g.pair) return;
  float mm = ((v[0] + v[1]) + (v[2] + v[3])) * 0.25f;
  float qq = 0.f;
#pragma unroll
  for (int e = 0; e < 4; ++e) qq = fmaf(v[e] - mm, v[e] - mm, qq);
  merge_stats(mm, qq, dpp_f<0xB1>(mm), dpp_f<0xB1>(qq), 4.f);
  merge_stats(mm, qq, dpp_f<0x4E>(mm), dpp_f<0x4E>(qq), 8.f);
  merge_stats(mm, qq, dpp_f<0x141>(mm), dpp_f<0x141>(qq), 16.f);
  merge_stats(mm, qq, dpp_f<0x140>(mm), dpp_f<0x140>(qq), 32.f);
  merge_stats(mm, qq, __shfl_xor(mm, 16, 64), __shfl_xor(qq, 16, 64), 64.f);
  if ((lane & 31) == 0) stats[((int64_t)n * g.CoutS + co) * R + reg] = make_float2(mm, qq);
}

}  // namespace

static int cout_padded(int Cout) { return (Cout + 63) / 64 * 64; }

static int cu_count() {
  static const int cus = [] {
    int dev = 0, n = 0;
    (void)hipGetDevice(&dev);
    (void)hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev);
    return n > 0 ? n : 256;
  }();
  return cus;
}

// ---- filter transforms: U (16 floats per (cin, cout)) and U24 (24, k16_item24) ----------------

extern "C" int64_t bpk_conv3x3_wino_filter_bytes(int Cin, int Cout) {
  return (int64_t)16 * Cin * cout_padded(Cout) * (int64_t)sizeof(float);
}

extern "C" int64_t bpk_conv3x3_wino_filter24_bytes(int Cin, int Cout) {
  return (int64_t)24 * Cin * cout_padded(Cout) * (int64_t)sizeof(float);
}

using FilterKernel = void (*)(const float*, float*, int, int, int, int);

static int wino_filter(FilterKernel kern, const float* weight, float* U, int Cin, int Cout,
                       int ft, void* stream) {
  BPK_REQUIRE(Cin > 0 && Cout > 0, "conv3x3_wino_filter: bad channels %d -> %d", Cin, Cout);
  const int64_t total = (int64_t)Cin * cout_padded(Cout);
  hipLaunchKernelGGL(kern, dim3((unsigned)std::min<int64_t>(bpk::ceil_div(total, 256), 4096)),
                     dim3(256), 0, bpk::as_stream(stream), weight, U, Cin, Cout,
                     cout_padded(Cout), ft);
  BPK_LAUNCH_CHECK("conv3x3_wino_filter");
  return BPK_OK;
}

extern "C" int bpk_conv3x3_wino_filter_f32(const float* weight, float* U, int Cin, int Cout,
                                           void* stream) {
  return wino_filter(wino_filter_kernel, weight, U, Cin, Cout, 0, stream);
}

extern "C" int bpk_conv3x3_wino_filter_ft_f32(const float* weight, float* U, int Cin, int Cout,
                                              void* stream) {
  return wino_filter(wino_filter_kernel, weight, U, Cin, Cout, 1, stream);
}

extern "C" int bpk_conv3x3_wino_filter24_f32(const float* weight, float* U, int Cin, int Cout,
                                             void* stream) {
  return wino_filter(wino_filter24_kernel, weight, U, Cin, Cout, 0, stream);
}

extern "C" int bpk_conv3x3_wino_filter24_ft_f32(const float* weight, float* U, int Cin, int Cout,
                                                void* stream) {
  return wino_filter(wino_filter24_kernel, weight, U, Cin, Cout, 1, stream);
}

extern "C" int bpk_conv3x3_wino_filter_batch_f32(const int64_t* jobs, int n, int max_elems,
                                                 void* stream) {
  BPK_REQUIRE(n >= 0 && n < 65536 && max_elems >= 0, "conv3x3_wino_filter_batch: bad job count");
  if (n == 0 || max_elems == 0) return BPK_OK;
  BPK_REQUIRE(jobs != nullptr, "conv3x3_wino_filter_batch: jobs is NULL");
  const dim3 grid((unsigned)std::min<int64_t>(bpk::ceil_div(max_elems, 256), 64), (unsigned)n);
  hipLaunchKernelGGL(wino_filter_batch_kernel, grid, dim3(256), 0, bpk::as_stream(stream), jobs);
  BPK_LAUNCH_CHECK("conv3x3_wino_filter_batch");
  return BPK_OK;
}

// ---- shapes ------------------------------------------------------------------------------------

extern "C" int bpk_conv3x3_wino_supported(int N, int Cin, int Cout, int H, int W) {
  // Cout % 64 != 0 (multiples of 16): padded to 64 couts, software-pipelined kernel
  return N > 0 && Cin > 0 && Cin % kCK == 0 && Cout % 16 == 0 && H % kOutRows == 0 &&
         W % kOutCols == 0;
}

// channel counts the 16-cin items take: 16-cin chunks that do not straddle the two sources,
// 128-cout blocks
static bool k16_channels_ok(int Cin, int C1, int Cout) {
  return Cin % 16 == 0 && C1 % 16 == 0 && cout_padded(Cout) % 128 == 0;
}

// The PAIR form of the 16-cin kernel (8-pixel-wide images, two per region): one source, no
// GroupNorm statistics, N even; a GroupNorm prologue needs both images' tables in LDS.
static bool wino_pair_ok(int N, int Cin, int Cout, int H, int W) {
  return N > 0 && N % 2 == 0 && W == 8 && H > 0 && H % kOutRows == 0 && Cout % 16 == 0 &&
         k16_channels_ok(Cin, Cin, Cout);
}

extern "C" int bpk_conv3x3_wino_pair_supported(int N, int Cin, int Cout, int H, int W) {
  return wino_pair_ok(N, Cin, Cout, H, W);
}

extern "C" int bpk_conv3x3_wino_up2_supported(int N, int Cin, int Cout, int H, int W) {
  return bpk_conv3x3_wino_supported(N, Cin, Cout, H, W) && k16_channels_ok(Cin, Cin, Cout);
}

extern "C" int bpk_conv3x3_wino_f24_supported(int N, int Cin, int C1, int Cout, int H, int W) {
  return N > 0 && Cin > 0 && Cin <= kPreMaxCin && C1 > 0 && C1 <= Cin && Cout > 0 &&
         Cout % 16 == 0 && k16_channels_ok(Cin, C1, Cout) && H > 0 && H % kOutRows == 0 && W > 0 &&
         W % kOutCols == 0;
}

// ---- launches ----------------------------------------------------------------------------------

// the operands of one conv call, as the C ABI passes them (x2, pre, bias, skip, stats may be null)
struct WinoArgs {
  const float *x, *x2, *pre, *U, *bias, *skip;
  float *y, *stats;
  void* stream;
};

// Geometry of a 16-cin launch: up = 1 reads x at half resolution (WinoGeo::up), S = split-K
// slices, pair = 1 the PAIR form.  One item = one region x one 128-cout block x one slice.
static WinoGeo k16_geo(int N, int Cin, int C1, int Cout, int H, int W, float div, int up, int S,
                       int pair) {
  const int CoutP = cout_padded(Cout);
  WinoGeo g{};
  g.N = N, g.Cin = Cin, g.C1 = C1, g.Cout = CoutP, g.CoutS = Cout, g.H = H, g.W = W;
  g.regions_x = pair ? 1 : W / kOutCols;
  g.regions_y = H / kOutRows;
  g.cout_blocks = CoutP / 128;
  g.div = div, g.up = up, g.ksplit = S, g.pair = pair;
  return g;
}

static int64_t k16_items(const WinoGeo& g) {
  return (int64_t)(g.pair ? g.N / 2 : g.N) * g.regions_x * g.regions_y * g.cout_blocks * g.ksplit;
}

using K16Kernel = void (*)(const float*, const float*, const float*, const float*, const float2*,
                           float*, float2*, WinoGeo, int, const float*, unsigned);

// One launch of a 16-cin kernel over the items of g (the callers have checked the shape): a
// persistent grid of one workgroup per CU, at most one per item, XCD-ordered when the grid is a
// multiple of 8.  f24: a.U is a U24 filter (k16_item24), else F(2x2) (k16_item).  With
// g.ksplit > 1 every slice writes its raw partial slab to a.y: no bias, tail or statistics.
static int k16_launch(bool f24, const WinoGeo& g, const WinoArgs& a) {
  const int64_t items = k16_items(g);
  BPK_REQUIRE(items < (1LL << 31), "conv3x3_wino: grid too large");
  // [f24][pre][F(2x2): PAIR; F(2x4): TAILK = an even number of chunks per workgroup]
  static const K16Kernel kKern[2][2][2] = {
      {{wino_f23_k16_kernel<false, false>, wino_f23_k16_kernel<false, true>},
       {wino_f23_k16_kernel<true, false>, wino_f23_k16_kernel<true, true>}},
      {{wino_f24_k16_kernel<false, false>, wino_f24_k16_kernel<false, true>},
       {wino_f24_k16_kernel<true, false>, wino_f24_k16_kernel<true, true>}}};
  const bool even = (g.Cin / 16 / g.ksplit) % 2 == 0;
  const unsigned grid = (unsigned)std::min<int64_t>(items, cu_count());
  const bool raw = g.ksplit > 1;
  hipLaunchKernelGGL(kKern[f24][a.pre != nullptr][f24 ? even : g.pair != 0], dim3(grid), dim3(512),
                     0, bpk::as_stream(a.stream), a.x, a.U, raw ? nullptr : a.bias,
                     raw ? nullptr : a.skip, reinterpret_cast<const float2*>(a.pre), a.y,
                     raw ? nullptr : reinterpret_cast<float2*>(a.stats), g, grid % 8 == 0 ? 1 : 0,
                     a.x2, (unsigned)items);
  BPK_LAUNCH_CHECK(f24 ? "conv3x3_wino_f24" : "conv3x3_wino_k16");
  return BPK_OK;
}

static int wino_f24_check(int N, int Cin, int C1, int Cout, int H, int W) {
  BPK_REQUIRE(bpk_conv3x3_wino_f24_supported(N, Cin, C1, Cout, H, W),
              "conv3x3_wino_f24: unsupported shape N=%d Cin=%d (C1=%d) Cout=%d H=%d W=%d (need "
              "Cin, C1 %% 16, Cout %% 128, H %% 8, W %% 16 == 0, Cin <= %d)", N, Cin, C1, Cout, H,
              W, kPreMaxCin);
  return BPK_OK;
}

static int wino_pair_check(const WinoArgs& a, int N, int Cin, int Cout, int H, int W) {
  BPK_REQUIRE(!a.x2 && !a.stats, "conv3x3_wino pair form (W == 8): one source, no statistics");
  BPK_REQUIRE(wino_pair_ok(N, Cin, Cout, H, W),
              "conv3x3_wino pair form: unsupported shape N=%d Cin=%d Cout=%d H=%d W=%d (need "
              "W == 8, N even, H %% 8, Cin %% 16, Cout %% 128 == 0)", N, Cin, Cout, H, W);
  BPK_REQUIRE(!a.pre || 2 * Cin <= kPreMaxCin, "conv3x3_wino pair form: GroupNorm prologue over "
              "%d > %d channels", Cin, kPreMaxCin / 2);
  return BPK_OK;
}

using PipeKernel = void (*)(const float*, const float*, const float*, const float*, const float2*,
                            float*, float2*, WinoGeo, int, const float*);

// F(2x2) conv of one launch: the form by shape (the map at the top of the file)
static int wino_ex(const WinoArgs& a, int C1, float div, int N, int Cin, int Cout, int H, int W) {
  if (!a.x2) C1 = Cin;
  if (W == 8) {
    const int rc = wino_pair_check(a, N, Cin, Cout, H, W);
    return rc != BPK_OK ? rc : k16_launch(false, k16_geo(N, Cin, Cin, Cout, H, W, div, 0, 1, 1), a);
  }
  BPK_REQUIRE(C1 > 0 && C1 <= Cin && C1 % kCK == 0,
              "conv3x3_wino: bad channel split C1=%d of Cin=%d", C1, Cin);
  BPK_REQUIRE(bpk_conv3x3_wino_supported(N, Cin, Cout, H, W),
              "conv3x3_wino: unsupported shape N=%d Cin=%d Cout=%d H=%d W=%d (need Cin %% 8, "
              "Cout %% 16, H %% 8, W %% 16 == 0)", N, Cin, Cout, H, W);
  BPK_REQUIRE(!a.pre || Cin <= kPreMaxCin,
              "conv3x3_wino: GroupNorm prologue over %d > %d input channels (the table in LDS): "
              "apply it to the input first", Cin, kPreMaxCin);
  if (k16_channels_ok(Cin, C1, Cout))
    return k16_launch(false, k16_geo(N, Cin, C1, Cout, H, W, div, 0, 1, 0), a);
  const int CoutP = cout_padded(Cout);
  const bool wg8 = a.pre && !a.skip && CoutP % 128 == 0;
  WinoGeo g{};
  g.N = N, g.Cin = Cin, g.C1 = C1, g.Cout = CoutP, g.CoutS = Cout, g.H = H, g.W = W;
  g.regions_x = W / kOutCols, g.regions_y = H / kOutRows, g.cout_blocks = CoutP / (wg8 ? 128 : 64);
  g.div = div;
  const int64_t blocks = (int64_t)N * g.regions_x * g.regions_y * g.cout_blocks;
  BPK_REQUIRE(blocks < (1LL << 31), "conv3x3_wino: grid too large");
  // peeled tail chunks (GroupNorm-prologue form only: the plain form spills with them)
  const int nch = Cin / kCK;
  const bool tail = a.pre && nch % 2 == 0 && nch >= 4;
  // [pre][8 waves][tail]; tail and wg8 imply pre, so the row without it has one kernel that runs
  static const PipeKernel kPipe[2][2][2] = {
      {{wino_f23_pipe_kernel<false, 4, false>, wino_f23_pipe_kernel<false, 4, false>},
       {wino_f23_pipe_kernel<false, 8, false>, wino_f23_pipe_kernel<false, 8, false>}},
      {{wino_f23_pipe_kernel<true, 4, false>, wino_f23_pipe_kernel<true, 4, true>},
       {wino_f23_pipe_kernel<true, 8, false>, wino_f23_pipe_kernel<true, 8, true>}}};
  hipLaunchKernelGGL(kPipe[a.pre != nullptr][wg8][tail], dim3((unsigned)blocks),
                     dim3(wg8 ? 512 : 256), 0, bpk::as_stream(a.stream), a.x, a.U, a.bias, a.skip,
                     reinterpret_cast<const float2*>(a.pre), a.y,
                     reinterpret_cast<float2*>(a.stats), g, blocks % 8 == 0 ? 1 : 0, a.x2);
  BPK_LAUNCH_CHECK("conv3x3_wino_pipe");
  return BPK_OK;
}

extern "C" int bpk_conv3x3_wino_ex_f32(const float* x, const float* x2, int C1, const float* pre,
                                       const float* U, const float* bias, const float* skip,
                                       float div, float* y, float* stats, int N, int Cin,
                                       int Cout, int H, int W, void* stream) {
  return wino_ex({x, x2, pre, U, bias, skip, y, stats, stream}, C1, div, N, Cin, Cout, H, W);
}

extern "C" int bpk_conv3x3_wino_pre_f32(const float* x, const float* pre, const float* U,
                                        const float* bias, const float* skip, float div, float* y,
                                        int N, int Cin, int Cout, int H, int W, void* stream) {
  return wino_ex({x, nullptr, pre, U, bias, skip, y, nullptr, stream}, Cin, div, N, Cin, Cout, H,
                 W);
}

extern "C" int bpk_conv3x3_wino_residual_f32(const float* x, const float* U, const float* bias,
                                             const float* skip, float div, float* y, int N,
                                             int Cin, int Cout, int H, int W, void* stream) {
  return bpk_conv3x3_wino_pre_f32(x, nullptr, U, bias, skip, div, y, N, Cin, Cout, H, W, stream);
}

extern "C" int bpk_conv3x3_wino_f32(const float* x, const float* U, const float* bias, float* y,
                                    int N, int Cin, int Cout, int H, int W, void* stream) {
  return bpk_conv3x3_wino_pre_f32(x, nullptr, U, bias, nullptr, 1.0f, y, N, Cin, Cout, H, W,
                                  stream);
}

// y = conv3x3(nearest_x2(x)) + bias for x [N, Cin, H/2, W/2], y [N, Cout, H, W]: the 16-cin
// kernel reads the half-resolution input inside its patch load, so the upsampled tensor is
// never written (reference layers.py:576-590, Upsample(with_conv=True)).
extern "C" int bpk_conv3x3_wino_up2_f32(const float* x, const float* U, const float* bias,
                                        float* y, int N, int Cin, int Cout, int H, int W,
                                        void* stream) {
  BPK_REQUIRE(bpk_conv3x3_wino_up2_supported(N, Cin, Cout, H, W),
              "conv3x3_wino_up2: unsupported shape N=%d Cin=%d Cout=%d H=%d W=%d (need Cin %% 16, "
              "Cout %% 128, H %% 8, W %% 16 == 0)", N, Cin, Cout, H, W);
  return k16_launch(false, k16_geo(N, Cin, Cin, Cout, H, W, 1.0f, 1, 1, 0),
                    {x, nullptr, nullptr, U, bias, nullptr, y, nullptr, stream});
}

// bpk_conv3x3_wino_up2_f32 with a U24 filter
extern "C" int bpk_conv3x3_wino_f24_up2_f32(const float* x, const float* U, const float* bias,
                                            float* y, int N, int Cin, int Cout, int H, int W,
                                            void* stream) {
  const int rc = wino_f24_check(N, Cin, Cin, Cout, H, W);
  if (rc != BPK_OK) return rc;
  return k16_launch(true, k16_geo(N, Cin, Cin, Cout, H, W, 1.0f, 1, 1, 0),
                    {x, nullptr, nullptr, U, bias, nullptr, y, nullptr, stream});
}

// Split-K for 16-cin launches that leave most CUs idle (the 32^2 / 16^2 levels at the small
// per-GPU batches of a batch-sharded run: B = 8 -> 128 / 32 workgroups on 256 CUs): the input
// channels are split into S slices (S a power of two, at least 2 chunks per slice), so that
// items x S is at most one workgroup per CU, then a reduce kernel applies the epilogue.
static int wino_splits(int N, int Cin, int C1, int Cout, int H, int W) {
  const bool pair = W == 8 && C1 == Cin && wino_pair_ok(N, Cin, Cout, H, W);
  if (!pair && !(bpk_conv3x3_wino_supported(N, Cin, Cout, H, W) && k16_channels_ok(Cin, C1, Cout)))
    return 1;
  const int64_t items = k16_items(k16_geo(N, Cin, C1, Cout, H, W, 1.0f, 0, 1, pair));
  const int nch = Cin / 16;
  int S = 1;
  while (items * S * 2 <= cu_count() && nch % (2 * S) == 0 && nch / (2 * S) >= 2) S *= 2;
  return S;
}

extern "C" int64_t bpk_conv3x3_wino_splitk_bytes(int N, int Cin, int C1, int Cout, int H, int W) {
  const int S = wino_splits(N, Cin, C1, Cout, H, W);
  return S > 1 ? (int64_t)S * N * Cout * H * W * (int64_t)sizeof(float) : 0;
}

// split rule -> launch -> reduce; S == 1 is the plain launch.  The partial slabs are in the
// output domain, so both filter forms share the workspace size and the reduce kernel.
static int wino_splitk(bool f24, const WinoArgs& a, int C1, float div, float* workspace, int N,
                       int Cin, int Cout, int H, int W) {
  if (!a.x2) C1 = Cin;
  if (f24) {
    const int rc = wino_f24_check(N, Cin, C1, Cout, H, W);
    if (rc != BPK_OK) return rc;
  }
  const int S = wino_splits(N, Cin, C1, Cout, H, W);
  if (S <= 1)
    return f24 ? k16_launch(true, k16_geo(N, Cin, C1, Cout, H, W, div, 0, 1, 0), a)
               : wino_ex(a, C1, div, N, Cin, Cout, H, W);
  BPK_REQUIRE(workspace != nullptr, "conv3x3_wino_splitk: workspace is NULL");
  const bool pair = W == 8;  // S > 1: wino_splits has checked the shape of either form
  if (pair) {
    const int rc = wino_pair_check(a, N, Cin, Cout, H, W);
    if (rc != BPK_OK) return rc;
  }
  const WinoGeo g = k16_geo(N, Cin, C1, Cout, H, W, div, 0, S, pair);
  WinoArgs part = a;
  part.y = workspace;
  const int rc = k16_launch(f24, g, part);
  if (rc != BPK_OK) return rc;
  const int64_t rblocks = (int64_t)(pair ? N / 2 : N) * (Cout / 8) * g.regions_x * g.regions_y;
  BPK_REQUIRE(Cout % 8 == 0 && rblocks < (1LL << 31), "conv3x3_wino_splitk: reduce grid");
  hipLaunchKernelGGL(wino_splitk_reduce_kernel, dim3((unsigned)rblocks), dim3(256), 0,
                     bpk::as_stream(a.stream), workspace, S, a.bias, a.skip, a.y,
                     reinterpret_cast<float2*>(a.stats), g);
  BPK_LAUNCH_CHECK("conv3x3_wino_splitk_reduce");
  return BPK_OK;
}

extern "C" int bpk_conv3x3_wino_splitk_f32(const float* x, const float* x2, int C1,
                                           const float* pre, const float* U, const float* bias,
                                           const float* skip, float div, float* y, float* stats,
                                           float* workspace, int N, int Cin, int Cout, int H,
                                           int W, void* stream) {
  return wino_splitk(false, {x, x2, pre, U, bias, skip, y, stats, stream}, C1, div, workspace, N,
                     Cin, Cout, H, W);
}

// bpk_conv3x3_wino_splitk_f32 with a U24 filter (bpk_conv3x3_wino_filter24_f32)
extern "C" int bpk_conv3x3_wino_f24_splitk_f32(const float* x, const float* x2, int C1,
                                               const float* pre, const float* U,
                                               const float* bias, const float* skip, float div,
                                               float* y, float* stats, float* workspace, int N,
                                               int Cin, int Cout, int H, int W, void* stream) {
  return wino_splitk(true, {x, x2, pre, U, bias, skip, y, stats, stream}, C1, div, workspace, N,
                     Cin, Cout, H, W);
}

#ifdef WINO_TIMING
extern "C" int bpk_wino_timing_read(long long* ts, unsigned* cu, int n) {
  if (n > (int)kTsMax) n = (int)kTsMax;
  if (hipMemcpyFromSymbol(ts, HIP_SYMBOL(g_wino_ts), sizeof(long long) * 8 * n) != hipSuccess) return -1;
  if (hipMemcpyFromSymbol(cu, HIP_SYMBOL(g_wino_cu), sizeof(unsigned) * n) != hipSuccess) return -1;
  return n;
}
#endif
