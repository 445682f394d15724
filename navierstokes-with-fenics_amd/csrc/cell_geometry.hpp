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
//   LAW 8 dynamic Smagorinsky  (c_K Delta_K^2) gamma                  p0 = c_K, the cell's C_s^2 (dynamic_cell_constant)
template <int LAW>
__device__ __forceinline__ double visc_law_nu(double gamma, double delta2, double p0, double p1, double p2) {
  static_assert(LAW == 1 || LAW == 2 || LAW == 8, "shear-rate laws are 1 (Smagorinsky), 2 (Carreau) and 8 (dynamic)");
  if constexpr (LAW == 1) {
    return (p0 * p0 * delta2) * gamma;
  } else if constexpr (LAW == 8) {
    return (p0 * delta2) * gamma;
  } else {
    const double lg = p1 * gamma;
    return p0 * (pow(1.0 + lg * lg, 0.5 * (p2 - 1.0)) - 1.0);
  }
}

// Laws of the velocity-gradient tensor G[a][b] = d_b u_a (laws 4 and 5 of nsfem_set_viscosity_law): the ONE copy as
// above.  A DIM = 2 field is the 3D field that does not depend on z: G has a zero third row and column, which the
// DIM = 2 instantiations never form.
//   LAW 4 WALE    (C_w Delta_K)^2 B^(3/2) / (A^(5/2) + B^(5/4))   p0 = C_w
//                 A = S:S, S = sym G;  B = Sd:Sd, Sd = sym(G G) - tr(G G)/3 I_3, summed entry by entry (in 2D with
//                 Sd_33 = -tr(G G)/3); 0 where the denominator is not > 0.  Powers by products and sqrt
//   LAW 5 Vreman  c Delta_K^2 sqrt(B_beta / G:G)                  p0 = c
//                 B_beta = the sum of the squares of the 2x2 minors of G (nine in 3D, det G in 2D), >= 0 by
//                 construction; 0 where G:G is not > 0
template <int LAW, int DIM>
__device__ __forceinline__ double visc_law_nu_grad(const double (&G)[DIM][DIM], double delta2, double p0) {
  static_assert(LAW == 4 || LAW == 5, "gradient-tensor laws are 4 (WALE) and 5 (Vreman)");
  if constexpr (LAW == 4) {
    double A = 0.0, trh = 0.0;
    double H[DIM][DIM];                  // H = G G
#pragma unroll
    for (int a = 0; a < DIM; ++a)
#pragma unroll
      for (int b = 0; b < DIM; ++b) {
        const double s = 0.5 * (G[a][b] + G[b][a]);
        A += s * s;
        double h = 0.0;
#pragma unroll
        for (int k = 0; k < DIM; ++k) h += G[a][k] * G[k][b];
        H[a][b] = h;
      }
#pragma unroll
    for (int a = 0; a < DIM; ++a) trh += H[a][a];
    const double t3 = trh / 3.0;
    double B = DIM == 2 ? t3 * t3 : 0.0;
#pragma unroll
    for (int a = 0; a < DIM; ++a)
#pragma unroll
      for (int b = 0; b < DIM; ++b) {
        const double sd = 0.5 * (H[a][b] + H[b][a]) - (a == b ? t3 : 0.0);
        B += sd * sd;
      }
    const double den = A * A * sqrt(A) + B * sqrt(sqrt(B));
    return den > 0.0 ? (p0 * p0 * delta2) * (B * sqrt(B) / den) : 0.0;
  } else {
    double gg = 0.0, bb = 0.0;
#pragma unroll
    for (int a = 0; a < DIM; ++a)
#pragma unroll
      for (int b = 0; b < DIM; ++b) gg += G[a][b] * G[a][b];
#pragma unroll
    for (int a = 0; a < DIM; ++a)
#pragma unroll
      for (int a2 = a + 1; a2 < DIM; ++a2)
#pragma unroll
        for (int b = 0; b < DIM; ++b)
#pragma unroll
          for (int b2 = b + 1; b2 < DIM; ++b2) {
            const double mnr = G[a][b] * G[a2][b2] - G[a][b2] * G[a2][b];
            bb += mnr * mnr;
          }
    return gg > 0.0 ? (p0 * delta2) * sqrt(bb / gg) : 0.0;
  }
}

// Law 8: c_K = the mean over the DIM + 1 vertices of cell c of the vertex field C_s^2 (k_dyn_reduce), summed in local
// vertex order -- the ONE copy the element and facet kernels inline.  p1 SoA [DIM + 1][nc].
template <int DIM>
__device__ __forceinline__ double dynamic_cell_constant(const int32_t* __restrict__ p1, const double* __restrict__ cs2v,
                                                        int nc, int c) {
  double s = cs2v[p1[c]];
#pragma unroll
  for (int v = 1; v <= DIM; ++v) s += cs2v[p1[(size_t)v * nc + c]];
  return s / (double)(DIM + 1);
}

// nu_x of any law at a point: laws 1, 2 and 8 from the shear rate alone (nothing of G is touched in their
// instantiations), laws 4 and 5 from the tensor
template <int LAW, int DIM>
__device__ __forceinline__ double visc_law_at(const double (&G)[DIM][DIM], double gamma, double delta2, double p0,
                                              double p1, double p2) {
  if constexpr (LAW == 4 || LAW == 5) return visc_law_nu_grad<LAW, DIM>(G, delta2, p0);
  else return visc_law_nu<LAW>(gamma, delta2, p0, p1, p2);
}

}  // namespace nsfem
