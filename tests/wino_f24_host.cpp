// Host check of the Winograd F(2x4, 3x3) arithmetic of csrc/wino_f24.h (built and run by
// tests/test_wino_f24_host.py).  Convolves one image (3x3, stride 1, zero pad 1) the way the HIP
// kernel does -- filter transform in double rounded once, data / output transforms in fp32, the
// contraction over cin as one fp32 fmaf chain per transform-domain point -- and prints the
// largest difference from its own double-precision direct convolution.
//   wino_f24_host exact             small integers, weights scaled by 15: the algebra is exact
//   wino_f24_host error Cin Cout H W   silu(randn) inputs, randn / (3 sqrt(Cin)) weights
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "wino_f24.h"

static double run(int Cin, int Cout, int H, int W, const std::vector<float>& x,
                  const std::vector<float>& w, double* max_ref) {
  const int TY = H / 2, TX = W / 4, T = TY * TX;
  auto at = [&](int c, int yy, int xx) -> float {
    return (yy < 0 || yy >= H || xx < 0 || xx >= W) ? 0.f : x[((size_t)c * H + yy) * W + xx];
  };
  std::vector<float> V((size_t)Cin * T * 24), U((size_t)Cin * Cout * 24);
  for (int c = 0; c < Cin; ++c)
    for (int t = 0; t < T; ++t) {
      const int y0 = 2 * (t / TX) - 1, x0 = 4 * (t % TX) - 1;
      float* v = &V[((size_t)c * T + t) * 24];
      for (int h = 0; h < 2; ++h) {
        float rx[6], ry[6];
        for (int j = 0; j < 6; ++j)
          wino24_data_rows(at(c, y0 + h, x0 + j), at(c, y0 + h + 1, x0 + j),
                           at(c, y0 + h + 2, x0 + j), h, rx[j], ry[j]);
        wino24_data_cols(rx, v + 12 * h);
        wino24_data_cols(ry, v + 12 * h + 6);
      }
    }
  for (int c = 0; c < Cin; ++c)
    for (int o = 0; o < Cout; ++o)
      wino24_filter(&w[((size_t)o * Cin + c) * 9], &U[((size_t)c * Cout + o) * 24]);
  double worst = 0.0, mref = 0.0;
  for (int o = 0; o < Cout; ++o)
    for (int t = 0; t < T; ++t) {
      float m[24];
      for (int p = 0; p < 24; ++p) m[p] = 0.f;
      for (int c = 0; c < Cin; ++c) {  // the MFMA's k-ordered fma chain
        const float* v = &V[((size_t)c * T + t) * 24];
        const float* u = &U[((size_t)c * Cout + o) * 24];
        for (int p = 0; p < 24; ++p) m[p] = fmaf(v[p], u[p], m[p]);
      }
      for (int h = 0; h < 2; ++h) {
        float tt[6], y[4];
        for (int j = 0; j < 6; ++j)
          tt[j] = wino24_out_rows(m[j], m[6 + j], m[12 + j], m[18 + j], h);
        wino24_out_cols(tt, y);
        for (int e = 0; e < 4; ++e) {
          const int oy = 2 * (t / TX) + h, ox = 4 * (t % TX) + e;
          double ref = 0.0;
          for (int c = 0; c < Cin; ++c)
            for (int r = 0; r < 3; ++r)
              for (int s = 0; s < 3; ++s)
                ref += (double)at(c, oy - 1 + r, ox - 1 + s) *
                       (double)w[((size_t)o * Cin + c) * 9 + 3 * r + s];
          worst = std::fmax(worst, std::fabs((double)y[e] - ref));
          mref = std::fmax(mref, std::fabs(ref));
        }
      }
    }
  *max_ref = mref;
  return worst;
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  std::mt19937_64 rng(1234);
  if (!std::strcmp(argv[1], "exact")) {
    const int Cin = 5, Cout = 3, H = 6, W = 12;
    std::vector<float> x((size_t)Cin * H * W), w((size_t)Cout * Cin * 9);
    std::uniform_int_distribution<int> d(-4, 4);
    for (auto& v : x) v = (float)d(rng);
    for (auto& v : w) v = 15.f * (float)d(rng);
    double mref;
    const double e = run(Cin, Cout, H, W, x, w, &mref);
    std::printf("max_abs_diff %.9g max_ref %.9g\n", e, mref);
    return 0;
  }
  if (!std::strcmp(argv[1], "error") && argc == 6) {
    const int Cin = std::atoi(argv[2]), Cout = std::atoi(argv[3]), H = std::atoi(argv[4]),
              W = std::atoi(argv[5]);
    if (Cin <= 0 || Cout <= 0 || H <= 0 || W <= 0 || H % 2 || W % 4) return 2;
    std::vector<float> x((size_t)Cin * H * W), w((size_t)Cout * Cin * 9);
    std::normal_distribution<double> n(0.0, 1.0);
    for (auto& v : x) {
      const double z = n(rng);
      v = (float)(z / (1.0 + std::exp(-z)));
    }
    for (auto& v : w) v = (float)(n(rng) / (3.0 * std::sqrt((double)Cin)));
    double mref;
    const double e = run(Cin, Cout, H, W, x, w, &mref);
    std::printf("max_abs_diff %.9g max_ref %.9g rel %.9g\n", e, mref, e / mref);
    return 0;
  }
  return 2;
}
