// Winograd F(2x4, 3x3): F(2,3) down the rows, F(4,3) along the row (points 0, 1, -1, 1/2, -2,
// inf), 24 transform-domain products per 2 x 4 output tile instead of the 32 of two F(2x2) tiles.
//     V = B2^T d B4  (4 x 6, d the 4 x 6 input tile)      U = G2 g G4^T  (4 x 6)
//     Y = A2^T [sum_cin U .* V] A4                         (2 rows x 4 columns)
// The one definition of the three transforms: the conv kernel, the filter kernel
// (csrc/conv_winograd.hip) and the host test program (tests/test_wino_f24_host.py) include it.
// Every B^T / A^T entry is an exact binary fraction; every multiply below sits in an explicit
// fmaf (or is by a power of two), so host and device round alike whatever the compiler's
// contraction setting.
#pragma once

#include <math.h>

#if defined(__HIPCC__)
#define WINO24_HD __host__ __device__ inline
#else
#define WINO24_HD inline
#endif

// Point order of a V record, a U24 entry and the accumulators: index 6 s + j = row position
// wino24_slot_row(s), column position j.  Slots (0, 1) come from patch rows 0-2 and slots (2, 3)
// from rows 1-3 of the tile, and with rows 3 and 2 swapped both halves compute
// (first - third, second +- ...) from their three rows (wino24_data_rows).
WINO24_HD int wino24_slot_row(int s) { return s < 2 ? s : 5 - s; }

// F(2,3) data transform down the rows, half h of a tile: r0, r1, r2 = tile rows h, h + 1, h + 2.
// x = slot 2 h (row position 0 or 3), y = slot 2 h + 1 (row position 1 or 2).
//   B2^T = [1 0 -1 0; 0 1 1 0; 0 -1 1 0; 0 1 0 -1]
WINO24_HD void wino24_data_rows(float r0, float r1, float r2, int h, float& x, float& y) {
  x = r0 - r2;
  y = r1 + (h ? -r0 : r2);
}

// F(4,3) data transform along one row: v = B4^T r,
//   B4^T = [1 -3/2 -2 3/2 1 0; 0 -1 1/2 5/2 1 0; 0 1 -5/2 1/2 1 0; 0 -2 -1 2 1 0;
//           0 1/2 -1 -1/2 1 0; 0 1 -3/2 -2 3/2 1]
WINO24_HD void wino24_data_cols(const float r[6], float v[6]) {
  const float d31 = r[3] - r[1], d42 = r[4] - r[2];
  v[0] = fmaf(-2.f, r[2], fmaf(1.5f, d31, r[0] + r[4]));
  v[1] = fmaf(2.5f, r[3], fmaf(0.5f, r[2], r[4] - r[1]));
  v[2] = fmaf(0.5f, r[3], fmaf(-2.5f, r[2], r[4] + r[1]));
  v[3] = fmaf(2.f, d31, d42);
  v[4] = fmaf(-0.5f, d31, d42);
  v[5] = fmaf(-2.f, r[3], fmaf(1.5f, d42, r[1] + r[5]));
}

// Filter transform in double, rounded once: u[6 s + j] = (G2 g G4^T)[wino24_slot_row(s)][j] for
// g[3 r + c] (row-major 3 x 3).  G2 = [1 0 0; 1/2 1/2 1/2; 1/2 -1/2 1/2; 0 0 1],
//   G4 = [1 0 0; 1/3 1/3 1/3; -1/3 1/3 -1/3; -16/15 -8/15 -4/15; 1/15 -2/15 4/15; 0 0 1]
WINO24_HD void wino24_filter(const float g[9], float u[24]) {
  double t[4][3];  // G2 g
  for (int c = 0; c < 3; ++c) {
    const double g0 = g[c], g1 = g[3 + c], g2 = g[6 + c];
    t[0][c] = g0;
    t[1][c] = 0.5 * (g0 + g1 + g2);
    t[2][c] = 0.5 * (g0 - g1 + g2);
    t[3][c] = g2;
  }
  for (int s = 0; s < 4; ++s) {
    const double* a = t[wino24_slot_row(s)];
    u[6 * s + 0] = (float)a[0];
    u[6 * s + 1] = (float)((a[0] + a[1] + a[2]) / 3.0);
    u[6 * s + 2] = (float)((a[1] - a[0] - a[2]) / 3.0);
    u[6 * s + 3] = (float)(-(16.0 * a[0] + 8.0 * a[1] + 4.0 * a[2]) / 15.0);
    u[6 * s + 4] = (float)((a[0] - 2.0 * a[1] + 4.0 * a[2]) / 15.0);
    u[6 * s + 5] = (float)a[2];
  }
}

// Output transform down the rows: output row h of A2^T m for the four slots of one column
// position (A2^T = [1 1 1 0; 0 1 -1 -1] over row positions; slots 2, 3 = row positions 3, 2).
WINO24_HD float wino24_out_rows(float m0, float m1, float m2, float m3, int h) {
  return h == 0 ? (m0 + m1) + m3 : (m1 - m3) - m2;
}

// Output transform along the row: y = A4^T t,
//   A4^T = [1 1 1 1 1 0; 0 1 -1 1/2 -2 0; 0 1 1 1/4 4 0; 0 1 -1 1/8 -8 1]
WINO24_HD void wino24_out_cols(const float t[6], float y[4]) {
  const float s12 = t[1] + t[2], d12 = t[1] - t[2];
  y[0] = (t[0] + s12) + (t[3] + t[4]);
  y[1] = fmaf(-2.f, t[4], fmaf(0.5f, t[3], d12));
  y[2] = fmaf(4.f, t[4], fmaf(0.25f, t[3], s12));
  y[3] = fmaf(-8.f, t[4], fmaf(0.125f, t[3], d12)) + t[5];
}
