// Affine cell geometry of the element kernels: J^-1 and |det J| from the SoA vertex coordinates of a cell, and the
// physical gradient of a reference gradient.  Shared by assembly.hip, assembly3d.hip and functionals.hip -- every
// kernel that inlines these gets the same bits.
#pragma once
#include "nsfem_internal.hpp"

namespace nsfem {

struct CellGeo {
  double ji00, ji01, ji10, ji11;   // J^{-1}
  double adet;
};

__device__ __forceinline__ CellGeo load_geo(const double* __restrict__ vx, int nc, int c) {
  // (products fuse with the sums of their own statement only: every kernel that inlines this gets the same bits)
#pragma clang fp contract(on)
  const double x0 = vx[c], y0 = vx[(size_t)nc + c];
  const double x1 = vx[(size_t)2 * nc + c], y1 = vx[(size_t)3 * nc + c];
  const double x2 = vx[(size_t)4 * nc + c], y2 = vx[(size_t)5 * nc + c];
  const double j00 = x1 - x0, j01 = x2 - x0, j10 = y1 - y0, j11 = y2 - y0;
  const double det = j00 * j11 - j01 * j10;
  const double id = 1.0 / det;
  CellGeo g;
  g.ji00 = j11 * id;
  g.ji01 = -j01 * id;
  g.ji10 = -j10 * id;
  g.ji11 = j00 * id;
  g.adet = fabs(det);
  return g;
}

// physical gradient of a reference gradient (dr0, dr1): g_a = sum_b Jinv[b][a] dr_b
__device__ __forceinline__ void phys(const CellGeo& g, double dr0, double dr1, double& gx,
                                     double& gy) {
#pragma clang fp contract(on)
  gx = g.ji00 * dr0 + g.ji10 * dr1;
  gy = g.ji01 * dr0 + g.ji11 * dr1;
}

struct CellGeo3 {
  double ji[3][3];   // J^{-1}[b][a] = d xi_b / d x_a
  double adet;
};

__device__ __forceinline__ CellGeo3 load_geo3(const double* __restrict__ vx, int nc, int c) {
  double x[4][3];
#pragma unroll
  for (int v = 0; v < 4; ++v)
#pragma unroll
    for (int d = 0; d < 3; ++d) x[v][d] = vx[(size_t)(3 * v + d) * nc + c];
  double J[3][3];   // J[a][b] = x_{b+1}[a] - x_0[a]
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int b = 0; b < 3; ++b) J[a][b] = x[b + 1][a] - x[0][a];
  const double c00 = J[1][1] * J[2][2] - J[1][2] * J[2][1];
  const double c01 = J[1][2] * J[2][0] - J[1][0] * J[2][2];
  const double c02 = J[1][0] * J[2][1] - J[1][1] * J[2][0];
  const double det = J[0][0] * c00 + J[0][1] * c01 + J[0][2] * c02;
  const double id = 1.0 / det;
  CellGeo3 g;
  g.ji[0][0] = c00 * id;
  g.ji[0][1] = (J[0][2] * J[2][1] - J[0][1] * J[2][2]) * id;
  g.ji[0][2] = (J[0][1] * J[1][2] - J[0][2] * J[1][1]) * id;
  g.ji[1][0] = c01 * id;
  g.ji[1][1] = (J[0][0] * J[2][2] - J[0][2] * J[2][0]) * id;
  g.ji[1][2] = (J[0][2] * J[1][0] - J[0][0] * J[1][2]) * id;
  g.ji[2][0] = c02 * id;
  g.ji[2][1] = (J[0][1] * J[2][0] - J[0][0] * J[2][1]) * id;
  g.ji[2][2] = (J[0][0] * J[1][1] - J[0][1] * J[1][0]) * id;
  g.adet = fabs(det);
  return g;
}

// physical gradient of a reference gradient dr: out_a = sum_b Jinv[b][a] dr_b
__device__ __forceinline__ void phys3(const CellGeo3& g, const double* dr, double* out) {
#pragma unroll
  for (int a = 0; a < 3; ++a) out[a] = g.ji[0][a] * dr[0] + g.ji[1][a] * dr[1] + g.ji[2][a] * dr[2];
}

// Variable-viscosity laws (nsfem_set_viscosity_law): the ONE copy of nu_x(gamma, Delta_K) the element kernels of both
// dimensions and their cell-mean variants inline.  gamma = sqrt(2 S:S) >= 0, delta2 = Delta_K^2, p = params[0..2].
//   LAW 1 Smagorinsky  (C_s Delta_K)^2 gamma                          p0 = C_s
//   LAW 2 Carreau      a [ (1 + (lambda gamma)^2)^((n - 1)/2) - 1 ]   p0 = a, p1 = lambda, p2 = n
template <int LAW>
__device__ __forceinline__ double visc_law_nu(double gamma, double delta2, double p0, double p1, double p2) {
  if constexpr (LAW == 1) {
    return (p0 * p0 * delta2) * gamma;
  } else {
    const double lg = p1 * gamma;
    return p0 * (pow(1.0 + lg * lg, 0.5 * (p2 - 1.0)) - 1.0);
  }
}

}  // namespace nsfem
