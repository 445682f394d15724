// Immersed bodies (nsfem_set_bodies, include/nsfem.h): the ONE copy of the signed distances, the mask and the
// "largest chi wins" rule that the penalisation element kernels of both dimensions (k_penal_cell, assembly.hip;
// k3_penal_cell, assembly3d.hip) and the force kernel (k_penal_forces, bodies.hip) inline -- and, for heated bodies, the
// scalar convection kernels with PENAL != 0 (k_scalar_conv_cell / k3_scalar_conv_cell) and k_body_heat.  The body table
// is a kernel argument: its entries are read with wave-uniform indices, i.e. as scalar loads.
#pragma once
#include "nsfem_internal.hpp"

namespace nsfem {

// signed distance of body s at x, negative inside:  kind 1 ball |x - c| - r,  kind 2 axis-aligned box
// |max(q, 0)| + min(max_a q_a, 0) with q = |x - c| - h,  kind 3 half-space (x - c) . n
template <int DIM>
__device__ __forceinline__ double body_distance(const BodyTable& t, int s, const double* x) {
  double r[DIM];
#pragma unroll
  for (int a = 0; a < DIM; ++a) r[a] = x[a] - t.centre[s][a];
  const int kind = t.kind[s];
  if (kind == 1) {
    double rr = 0.0;
#pragma unroll
    for (int a = 0; a < DIM; ++a) rr += r[a] * r[a];
    return sqrt(rr) - t.size[s][0];
  }
  if (kind == 2) {
    double out2 = 0.0, qmax = -1.0e300;
#pragma unroll
    for (int a = 0; a < DIM; ++a) {
      const double q = fabs(r[a]) - t.size[s][a];
      const double qp = fmax(q, 0.0);
      out2 += qp * qp;
      qmax = fmax(qmax, q);
    }
    return sqrt(out2) + fmin(qmax, 0.0);
  }
  double d = 0.0;
#pragma unroll
  for (int a = 0; a < DIM; ++a) d += r[a] * t.size[s][a];
  return d;
}

// the mask: sharp 1 where d <= 0; smoothed over |d| < eps by 0.5 (1 - d/eps - sin(pi d/eps)/pi)
template <bool SMOOTH>
__device__ __forceinline__ double body_chi(double d, double eps) {
  if constexpr (!SMOOTH) {
    return d <= 0.0 ? 1.0 : 0.0;
  } else {
    if (d <= -eps) return 1.0;
    if (d >= eps) return 0.0;
    const double z = d / eps;
    return 0.5 * (1.0 - z - sin(M_PI * z) / M_PI);
  }
}

// the body that counts at x: the largest chi, the lowest index on ties.  Returns chi (0: no body), the index in win
template <int DIM, bool SMOOTH>
__device__ __forceinline__ double body_winner(const BodyTable& t, const double* x, int& win) {
  double best = 0.0;
  win = 0;
  for (int s = 0; s < t.n; ++s) {
    const double chi = body_chi<SMOOTH>(body_distance<DIM>(t, s, x), t.eps);
    if (chi > best) {
      best = chi;
      win = s;
    }
  }
  return best;
}

// rigid velocity of body s at x:  U + W x (x - c);  2D: U + w (-(y - c_y), x - c_x) with w = angular[2]
template <int DIM>
__device__ __forceinline__ void body_velocity(const BodyTable& t, int s, const double* x, double* us) {
  double r[DIM];
#pragma unroll
  for (int a = 0; a < DIM; ++a) r[a] = x[a] - t.centre[s][a];
  if constexpr (DIM == 2) {
    const double w = t.angular[s][2];
    us[0] = t.velocity[s][0] - w * r[1];
    us[1] = t.velocity[s][1] + w * r[0];
  } else {
    const double* W = t.angular[s];
    us[0] = t.velocity[s][0] + (W[1] * r[2] - W[2] * r[1]);
    us[1] = t.velocity[s][1] + (W[2] * r[0] - W[0] * r[2]);
    us[2] = t.velocity[s][2] + (W[0] * r[1] - W[1] * r[0]);
  }
}

// Centroid x_c of a cell with vertices xv[DIM + 1][DIM] and R = max_v |x_v - x_c|: every point of the cell lies
// within R of x_c
template <int DIM>
__device__ __forceinline__ double cell_ball(const double (*xv)[DIM], double* xc) {
#pragma unroll
  for (int a = 0; a < DIM; ++a) {
    double sum = 0.0;
#pragma unroll
    for (int v = 0; v <= DIM; ++v) sum += xv[v][a];
    xc[a] = sum / (DIM + 1);
  }
  double r2 = 0.0;
#pragma unroll
  for (int v = 0; v <= DIM; ++v) {
    double rr = 0.0;
#pragma unroll
    for (int a = 0; a < DIM; ++a) rr += (xv[v][a] - xc[a]) * (xv[v][a] - xc[a]);
    r2 = fmax(r2, rr);
  }
  return sqrt(r2);
}

// Can the support of body s not reach the cell?  Signed distances are 1-Lipschitz, so d_s(x_c) - R >= eps means
// chi_s = 0 on the whole cell (the quadrature points are interior: rounding in R or d cannot flip a point that
// counts).  k_penal_forces: the row of a body skips every other cell.
template <int DIM>
__device__ __forceinline__ bool body_misses_cell(const BodyTable& t, int s, const double (*xv)[DIM]) {
  double xc[DIM];
  const double reach = cell_ball<DIM>(xv, xc) + t.eps;
  return body_distance<DIM>(t, s, xc) >= reach;
}

}  // namespace nsfem
