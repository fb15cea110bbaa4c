// Separable blur + decimation measurement operator A = D G Sym and its adjoint, gfx950.
//
// Per plane x [H, W], odd tap count K, p = K / 2, stride s, o = (s - 1) / 2:
//   xs        = half-sample symmetric extension of x by p  (d c b a | a b c d | d c b a)
//   (G x)[r,c] = sum_{k,l} g[k] g[l] xs[r + p - k, c + p - l]      ('same' convolution)
//   y[i, j]   = (G x)[s i + o, s j + o],  Ho = ceil((H - o) / s), Wo likewise.
// i.e. scipy.signal.convolve2d(x, outer(g, g), boundary='symm', mode='same')[o::s, o::s].
//
// Forward: one block per BLUR_TH x BLUR_TW tile of the blurred image (= the output tile at
// s = 1).  The input tile with its halo is loaded through the symmetric index map into LDS,
// the column pass runs at the decimated rows only, the row pass at the decimated columns,
// and the result is staged in LDS for the store: one launch, the intermediate never
// reaches HBM.
//
// Adjoint A^T = Sym^T G^T D^T in gather form: one block per BLUR_TH x BLUR_TW tile of the
// input-side gradient, one thread per pixel m.  Per axis the thread sums over the at most
// three pre-images of m under the symmetric map -- m, -1 - m (m < p), 2 n - 1 - m
// (m >= n - p) -- the taps times the zero-upsampled y; y is held in LDS in compact
// (decimated) form and the tap loop steps by s, so the inserted zeros are never touched.
// No atomics; the summation order is fixed, so two runs agree bit for bit.
//
// Rows move as 16-byte vectors wherever a whole vector lies inside the row and the plane
// is 16-byte aligned: the LDS column origin of every tile is rounded down to a vector
// boundary of the global row, so global and LDS addresses are aligned together.
// Taps arrive by value in the kernel arguments (<= 33 values).
#include "bpk_common.h"

namespace {

// Mirrored by op/blur.py (TILE_H, TILE_W, MAX_TAPS).
constexpr int BLUR_TH = 16;                                // tile rows
constexpr int BLUR_TW = 64;                                // tile columns
constexpr int BLUR_KMAX = 33;                              // most taps
constexpr int BLUR_PMAX = BLUR_KMAX / 2;                   // widest halo
constexpr int BLUR_LH = BLUR_TH + 2 * BLUR_PMAX;           // LDS tile rows
constexpr int BLUR_LW = BLUR_TW + 2 * BLUR_PMAX + 4;       // LDS row stride (+ alignment slack)
constexpr int BLUR_THREADS = 256;
// static LDS: (BLUR_LH + BLUR_TH) * BLUR_LW elements = 25.6 KB (f32) / 51.2 KB (f64)
static_assert((BLUR_LH + BLUR_TH) * BLUR_LW * sizeof(double) + BLUR_KMAX * sizeof(double) <=
                  64 * 1024, "blur: static LDS over 64 KB");
static_assert(BLUR_THREADS == 4 * 64 && BLUR_THREADS == 16 * BLUR_TH && BLUR_TH == 16 &&
                  BLUR_TW == 64 && BLUR_LW % 4 == 0, "blur: thread / vector layout");

template <typename T>
struct Taps {
  T g[BLUR_KMAX];
};

template <typename T>
struct VecOf;
template <>
struct VecOf<float> {
  using type = float4;
  static constexpr int N = 4;
};
template <>
struct VecOf<double> {
  using type = double2;
  static constexpr int N = 2;
};

struct BlurGeo {
  int H, W;      // input side (x, and the adjoint's result)
  int Ho, Wo;    // output side (y)
  int K, p, s, o;
  int tiles_h, tiles_w;
};

__device__ inline int cdiv(int a, int b) { return -bpk::floordiv(-a, b); }
__device__ inline int floor_to(int a, int v) { return bpk::floordiv(a, v) * v; }
__device__ inline int ceil_to(int a, int v) { return cdiv(a, v) * v; }

// Source index of coordinate a on an axis of n samples, -1 where the value is zero.
// SYMM: [-p, n + p) folds back by the half-sample symmetric map (p <= n: one fold).
template <bool SYMM>
__device__ inline int src_index(int a, int n, int p) {
  if (SYMM) {
    if (a < -p || a >= n + p) return -1;
    return a < 0 ? -1 - a : (a >= n ? 2 * n - 1 - a : a);
  }
  return (a < 0 || a >= n) ? -1 : a;
}

// lds[r * BLUR_LW + c] = src(row_lo + r, col_lo + c) for r < nrows, c < ncols.
// col_lo and ncols are multiples of the vector length.
template <typename T, bool SYMM>
__device__ inline void load_tile(T* lds, const T* __restrict__ src, int SH, int SW, int row_lo,
                                 int nrows, int col_lo, int ncols, int p, bool vec_ok) {
  using V = typename VecOf<T>::type;
  constexpr int VN = VecOf<T>::N;
  constexpr int NCH = BLUR_LW / VN;
  const int nch = ncols / VN;
  for (int idx = threadIdx.x; idx < nrows * NCH; idx += BLUR_THREADS) {
    const int r = idx / NCH, ch = idx - r * NCH;
    if (ch >= nch) continue;
    T* dst = lds + r * BLUR_LW + ch * VN;
    const int c = col_lo + ch * VN;
    const int sr = src_index<SYMM>(row_lo + r, SH, p);
    if (sr < 0) {
#pragma unroll
      for (int j = 0; j < VN; ++j) dst[j] = T(0);
      continue;
    }
    const T* row = src + (int64_t)sr * SW;
    if (vec_ok && c >= 0 && c + VN <= SW) {
      *reinterpret_cast<V*>(dst) = *reinterpret_cast<const V*>(row + c);
    } else {
#pragma unroll
      for (int j = 0; j < VN; ++j) {
        const int sc = src_index<SYMM>(c + j, SW, p);
        dst[j] = sc < 0 ? T(0) : row[sc];
      }
    }
  }
}

// dst(row0 + r, c) = lds[r * BLUR_LW + (c - col_base)] for r < nrows, col_lo <= c < col_hi.
// col_base is a multiple of the vector length, col_base <= col_lo.
template <typename T>
__device__ inline void store_tile(const T* lds, T* __restrict__ dst, int DW, int row0, int nrows,
                                  int col_lo, int col_hi, int col_base, bool vec_ok) {
  using V = typename VecOf<T>::type;
  constexpr int VN = VecOf<T>::N;
  constexpr int NCH = BLUR_LW / VN;
  const int nch = cdiv(col_hi - col_base, VN);
  for (int idx = threadIdx.x; idx < nrows * NCH; idx += BLUR_THREADS) {
    const int r = idx / NCH, ch = idx - r * NCH;
    if (ch >= nch) continue;
    const T* s = lds + r * BLUR_LW + ch * VN;
    const int c = col_base + ch * VN;
    T* row = dst + (int64_t)(row0 + r) * DW;
    if (vec_ok && c >= col_lo && c + VN <= col_hi) {
      *reinterpret_cast<V*>(row + c) = *reinterpret_cast<const V*>(s);
    } else {
#pragma unroll
      for (int j = 0; j < VN; ++j)
        if (c + j >= col_lo && c + j < col_hi) row[c + j] = s[j];
    }
  }
}

struct Tile {
  int64_t plane;
  int r0, r1, c0, c1;  // rows [r0, r1), columns [c0, c1) of the H x W side
};

__device__ inline Tile tile_of_block(const BlurGeo& g) {
  const int64_t b = blockIdx.x;
  const int tw = (int)(b % g.tiles_w);
  const int64_t q = b / g.tiles_w;
  const int th = (int)(q % g.tiles_h);
  Tile t;
  t.plane = q / g.tiles_h;
  t.r0 = th * BLUR_TH;
  t.c0 = tw * BLUR_TW;
  t.r1 = min(t.r0 + BLUR_TH, g.H);
  t.c1 = min(t.c0 + BLUR_TW, g.W);
  return t;
}

template <typename T>
__global__ __launch_bounds__(BLUR_THREADS) void k_blur2d_fwd(const T* __restrict__ x,
                                                             T* __restrict__ y, BlurGeo g,
                                                             Taps<T> taps, bool vec_in,
                                                             bool vec_out) {
  constexpr int VN = VecOf<T>::N;
  __shared__ __align__(16) T s_in[BLUR_LH * BLUR_LW];
  __shared__ __align__(16) T s_mid[BLUR_TH * BLUR_LW];
  const Tile t = tile_of_block(g);
  // outputs whose sample point s i + o lies in this tile
  const int i_lo = max(0, cdiv(t.r0 - g.o, g.s)), i_hi = max(0, cdiv(t.r1 - g.o, g.s));
  const int j_lo = max(0, cdiv(t.c0 - g.o, g.s)), j_hi = max(0, cdiv(t.c1 - g.o, g.s));
  const int ni = i_hi - i_lo, nj = j_hi - j_lo;
  if (ni <= 0 || nj <= 0) return;  // block-uniform
  const int row_lo = g.s * i_lo + g.o - g.p;
  const int nrows = g.s * (ni - 1) + g.K;
  const int col_lo = floor_to(g.s * j_lo + g.o - g.p, VN);
  const int ncols = ceil_to(g.s * (j_hi - 1) + g.o + g.p + 1 - col_lo, VN);
  load_tile<T, true>(s_in, x + t.plane * g.H * g.W, g.H, g.W, row_lo, nrows, col_lo, ncols, g.p,
                     vec_in);
  __syncthreads();
  // A thread keeps the sums of rows ly, ly + 4, ly + 8, ly + 12 (and of two columns in the
  // column pass) side by side, so each tap feeds independent LDS reads instead of one
  // dependent chain per output.  Rows / columns past the tile read a clamped (valid)
  // address and are not written.
  const int lx = threadIdx.x & 63, ly = threadIdx.x >> 6;
  // column pass at the decimated rows: s_mid[li][c] = sum_k g[k] s_in[s li + 2p - k][c]
  {
    const int lc0 = min(lx, ncols - 1), lc1 = min(lx + 64, ncols - 1);
    const T* top[4];
    T acc[4][2];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      top[q] = s_in + (g.s * min(ly + 4 * q, ni - 1) + 2 * g.p) * BLUR_LW;
      acc[q][0] = taps.g[0] * top[q][lc0];
      acc[q][1] = taps.g[0] * top[q][lc1];
    }
    for (int k = 1; k < g.K; ++k) {
      const T gk = taps.g[k];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        acc[q][0] = __builtin_fma(gk, top[q][lc0 - k * BLUR_LW], acc[q][0]);
        acc[q][1] = __builtin_fma(gk, top[q][lc1 - k * BLUR_LW], acc[q][1]);
      }
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int li = ly + 4 * q;
      if (li < ni && lx < ncols) s_mid[li * BLUR_LW + lx] = acc[q][0];
      if (li < ni && lx + 64 < ncols) s_mid[li * BLUR_LW + lx + 64] = acc[q][1];
    }
  }
  __syncthreads();
  // row pass at the decimated columns, staged in s_in for the store
  const int jbase = floor_to(j_lo, VN);
  {
    const int right = g.s * (j_lo + min(lx, nj - 1)) + g.o + g.p - col_lo;
    const T* mid[4];
    T acc[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      mid[q] = s_mid + min(ly + 4 * q, ni - 1) * BLUR_LW + right;
      acc[q] = taps.g[0] * mid[q][0];
    }
    for (int k = 1; k < g.K; ++k) {
      const T gk = taps.g[k];
#pragma unroll
      for (int q = 0; q < 4; ++q) acc[q] = __builtin_fma(gk, mid[q][-k], acc[q]);
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int li = ly + 4 * q;
      if (li < ni && lx < nj) s_in[li * BLUR_LW + (j_lo + lx - jbase)] = acc[q];
    }
  }
  __syncthreads();
  store_tile<T>(s_in, y + t.plane * g.Ho * g.Wo, g.Wo, i_lo, ni, j_lo, j_hi, jbase, vec_out);
}

// One axis of the adjoint at pixel m of n, for R sums that share m (acc[r] starts at 0):
// acc[r] = the sum over the pre-images e of m of sum_k g[k] u_r[e - p + k], u_r the
// zero-upsampled y (u_r[s i + o] = val(r, i)).  Only the taps that meet a sample are
// visited: at most ceil(K / s) per pre-image, in a loop of block-uniform length whose
// spare trips add nothing.  lo_edge / hi_edge (block-uniform): some pixel of the tile has
// the pre-image -1 - m / 2 n - 1 - m.
template <int R, typename T, typename F>
__device__ inline void adjoint_axis(T (&acc)[R], int m, int n, bool lo_edge, bool hi_edge,
                                    const BlurGeo& g, const T* taps, F val) {
  const int trips = (g.K + g.s - 1) / g.s;
#pragma unroll
  for (int r = 0; r < R; ++r) acc[r] = T(0);
  for (int q = 0; q < 3; ++q) {
    if ((q == 1 && !lo_edge) || (q == 2 && !hi_edge)) continue;
    const bool on = q == 0 || (q == 1 ? m < g.p : m >= n - g.p);
    const int e = q == 0 ? m : (q == 1 ? -1 - m : 2 * n - 1 - m);
    const int a0 = e - g.p;                                       // u index at k = 0
    const int first = g.o + cdiv(max(a0, g.o) - g.o, g.s) * g.s;  // first sample >= a0
    int k = on ? first - a0 : g.K, a = first, i = (first - g.o) / g.s;
    for (int t = 0; t < trips; ++t, k += g.s, a += g.s, ++i) {
      const bool v = k < g.K && a < n;
      const T gk = v ? taps[k] : T(0);
#pragma unroll
      for (int r = 0; r < R; ++r) acc[r] = __builtin_fma(gk, v ? val(r, i) : T(0), acc[r]);
    }
  }
}

template <typename T>
__global__ __launch_bounds__(BLUR_THREADS) void k_blur2d_adj(const T* __restrict__ y,
                                                             T* __restrict__ gx, BlurGeo g,
                                                             Taps<T> taps, bool vec_in,
                                                             bool vec_out) {
  constexpr int VN = VecOf<T>::N;
  __shared__ __align__(16) T s_y[BLUR_LH * BLUR_LW];
  __shared__ __align__(16) T s_t[BLUR_TH * BLUR_LW];
  __shared__ T s_g[BLUR_KMAX];
  const Tile t = tile_of_block(g);
  if (threadIdx.x < BLUR_KMAX) s_g[threadIdx.x] = taps.g[threadIdx.x];
  // samples of y within p of the tile (the reflected pre-images stay inside that range)
  const int i_lo = max(0, cdiv(t.r0 - g.p - g.o, g.s));
  const int i_hi = min(g.Ho, bpk::floordiv(t.r1 - 1 + g.p - g.o, g.s) + 1);
  const int j_lo = max(0, cdiv(t.c0 - g.p - g.o, g.s));
  const int j_hi = min(g.Wo, bpk::floordiv(t.c1 - 1 + g.p - g.o, g.s) + 1);
  const int ni = max(i_hi - i_lo, 0);
  const int jbase = floor_to(j_lo, VN);
  const int ncols = max(ceil_to(j_hi - jbase, VN), 0);
  load_tile<T, false>(s_y, y + t.plane * g.Ho * g.Wo, g.Ho, g.Wo, i_lo, ni, jbase, ncols, 0,
                      vec_in);
  __syncthreads();
  const int nr = t.r1 - t.r0, nc = t.c1 - t.c0;
  // rows: thread (row, cg) of 16 x 16 sums its row at the columns cg, cg + 16, ... of s_y
  {
    constexpr int R = (BLUR_LW + 15) / 16;
    const int lr = threadIdx.x >> 4, cg = threadIdx.x & 15;
    if (lr < nr) {
      T acc[R];
      adjoint_axis<R>(acc, t.r0 + lr, g.H, t.r0 < g.p, t.r1 > g.H - g.p, g, s_g, [&](int r, int i) {
        return s_y[(i - i_lo) * BLUR_LW + min(cg + 16 * r, BLUR_LW - 1)];
      });
#pragma unroll
      for (int r = 0; r < R; ++r)
        if (cg + 16 * r < ncols) s_t[lr * BLUR_LW + cg + 16 * r] = acc[r];
    }
  }
  __syncthreads();
  // columns: thread (lx, ly) sums column lx of the rows ly, ly + 4, ly + 8, ly + 12 of s_t
  {
    const int lx = threadIdx.x & 63, ly = threadIdx.x >> 6;
    if (lx < nc) {
      T acc[4];
      adjoint_axis<4>(acc, t.c0 + lx, g.W, t.c0 < g.p, t.c1 > g.W - g.p, g, s_g, [&](int r, int j) {
        return s_t[min(ly + 4 * r, nr - 1) * BLUR_LW + (j - jbase)];
      });
#pragma unroll
      for (int r = 0; r < 4; ++r)
        if (ly + 4 * r < nr) s_y[(ly + 4 * r) * BLUR_LW + lx] = acc[r];
    }
  }
  __syncthreads();
  store_tile<T>(s_y, gx + t.plane * g.H * g.W, g.W, t.r0, nr, t.c0, t.c1, t.c0, vec_out);
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

template <typename T>
int blur_launch(const char* what, bool adjoint, const T* in, T* out, int64_t planes, int H, int W,
                const double* taps, int K, int stride, void* stream) {
  BPK_REQUIRE(planes >= 0 && H >= 1 && W >= 1 && H <= (1 << 29) && W <= (1 << 29),
              "%s: planes >= 0 and 1 <= H, W <= 2^29 required", what);
  BPK_REQUIRE(K >= 1 && K <= BLUR_KMAX && (K & 1), "%s: tap count must be odd, 1 <= K <= %d (got %d)",
              what, BLUR_KMAX, K);
  BPK_REQUIRE(K / 2 <= (H < W ? H : W), "%s: halo K / 2 = %d exceeds min(H, W) = %d", what, K / 2,
              H < W ? H : W);
  BPK_REQUIRE(stride >= 1, "%s: stride >= 1 required (got %d)", what, stride);
  const int o = (stride - 1) / 2;
  BPK_REQUIRE(o < (H < W ? H : W), "%s: stride %d leaves no sample in a %d x %d plane", what,
              stride, H, W);
  BPK_REQUIRE(taps != nullptr, "%s: taps is NULL", what);
  if (planes == 0) return BPK_OK;
  BPK_REQUIRE(in != nullptr && out != nullptr, "%s: NULL tensor", what);
  BlurGeo g;
  g.H = H;
  g.W = W;
  g.Ho = (int)bpk::ceil_div(H - o, stride);
  g.Wo = (int)bpk::ceil_div(W - o, stride);
  g.K = K;
  g.p = K / 2;
  g.s = stride;
  g.o = o;
  g.tiles_h = (int)bpk::ceil_div(H, BLUR_TH);
  g.tiles_w = (int)bpk::ceil_div(W, BLUR_TW);
  const int64_t blocks = planes * g.tiles_h * g.tiles_w;
  if (blocks > 0x7fffffffLL) {
    bpk::set_error("%s: %lld tiles exceed the grid limit", what, (long long)blocks);
    return BPK_ERR_UNSUPPORTED;
  }
  Taps<T> tp;
  for (int k = 0; k < BLUR_KMAX; ++k) tp.g[k] = k < K ? (T)taps[k] : T(0);
  constexpr int VN = VecOf<T>::N;
  const bool vx = aligned16(adjoint ? (const void*)out : (const void*)in) && W % VN == 0;
  const bool vy = aligned16(adjoint ? (const void*)in : (const void*)out) && g.Wo % VN == 0;
  if (adjoint)
    hipLaunchKernelGGL(k_blur2d_adj<T>, dim3((unsigned)blocks), dim3(BLUR_THREADS), 0,
                       bpk::as_stream(stream), in, out, g, tp, vy, vx);
  else
    hipLaunchKernelGGL(k_blur2d_fwd<T>, dim3((unsigned)blocks), dim3(BLUR_THREADS), 0,
                       bpk::as_stream(stream), in, out, g, tp, vx, vy);
  BPK_LAUNCH_CHECK(what);
  return BPK_OK;
}

}  // namespace

extern "C" int bpk_blur2d_f32(const float* x, float* out, int64_t planes, int H, int W,
                              const double* taps, int K, int stride, void* stream) {
  return blur_launch<float>("blur2d", false, x, out, planes, H, W, taps, K, stride, stream);
}
extern "C" int bpk_blur2d_f64(const double* x, double* out, int64_t planes, int H, int W,
                              const double* taps, int K, int stride, void* stream) {
  return blur_launch<double>("blur2d", false, x, out, planes, H, W, taps, K, stride, stream);
}
extern "C" int bpk_blur2d_adjoint_f32(const float* y, float* out, int64_t planes, int H, int W,
                                      const double* taps, int K, int stride, void* stream) {
  return blur_launch<float>("blur2d_adjoint", true, y, out, planes, H, W, taps, K, stride,
                            stream);
}
extern "C" int bpk_blur2d_adjoint_f64(const double* y, double* out, int64_t planes, int H, int W,
                                      const double* taps, int K, int stride, void* stream) {
  return blur_launch<double>("blur2d_adjoint", true, y, out, planes, H, W, taps, K, stride,
                             stream);
}
