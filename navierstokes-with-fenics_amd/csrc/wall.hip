// Wall quantities of the discrete solution on a resident, group-sorted set of facets: measure, pressure force,
// viscous force (with the viscosity law of nsfem_set_viscosity_law when asked for), mass flux, integral of the
// transported scalar, conductive heat flux and the torque of the traction about a point.
//
// The facet side of the device post-processing next to functionals.hip (cells), derived.hip (cells / nodes) and
// points.hip (points); nsfem_boundary_force (boundary.hip) stays as the one-shot call.  Two launches per call:
//   k_wall_facets<DIM, LAW>  one thread per facet, NW = 9 (2D) / 13 (3D) integrals per facet into a row of its own
//   k_wall_reduce<NW>        one workgroup per group of facets, the rows of a group summed in a fixed order
// Plain vector stores, no atomics: the same state gives the same bytes, and the sums of a group do not depend on
// which other groups exist.  Both kernels read the state and write only the context's wall buffers.
//
// Facet rules as in k_boundary_force: the 2-point Gauss rule on an edge, the 3 edge midpoints on a face.  grad u, p
// and grad T are linear on an affine facet, u.n and T quadratic, (x - x0) x t quadratic: the rules are exact for
// every integrand when LAW = 0.  With a law, nu_x (of gamma and Delta_K for laws 1 and 2, of the gradient tensor for
// laws 4 and 5, of gamma with the cell's dynamic constant c_K for law 8: cell_geometry.hpp) is evaluated at the points of the rule and the rule is part of the
// definition (as the degree-5 rule is for nsfem_viscosity_cells).
#include "cell_geometry.hpp"

namespace nsfem {

// P2 basis values and physical gradients at the barycentric point lam[] (UFC order: vertices, then the edges
// e(12), e(02), e(01) / e(23), e(13), e(12), e(03), e(02), e(01)); gl[v][d] = d lambda_v / d x_d
template <int DIM>
__device__ __forceinline__ void wall_p2_at(const double* lam, const double (*gl)[3], double* phi, double (*dphi)[3]) {
  constexpr int NV = DIM + 1;
  constexpr int NE = DIM == 2 ? 3 : 6;
  const int ea2[3] = {1, 0, 0}, eb2[3] = {2, 2, 1};
  const int ea3[6] = {2, 1, 1, 0, 0, 0}, eb3[6] = {3, 3, 2, 3, 2, 1};
#pragma unroll
  for (int v = 0; v < NV; ++v) {
    phi[v] = lam[v] * (2.0 * lam[v] - 1.0);
#pragma unroll
    for (int d = 0; d < DIM; ++d) dphi[v][d] = (4.0 * lam[v] - 1.0) * gl[v][d];
  }
#pragma unroll
  for (int e = 0; e < NE; ++e) {
    const int a = DIM == 2 ? ea2[e] : ea3[e], b = DIM == 2 ? eb2[e] : eb3[e];
    phi[NV + e] = 4.0 * lam[a] * lam[b];
#pragma unroll
    for (int d = 0; d < DIM; ++d) dphi[NV + e][d] = 4.0 * (lam[a] * gl[b][d] + lam[b] * gl[a][d]);
  }
}

// Row of facet f (resident order), NW = 2 DIM + 4 + (DIM == 2 ? 1 : 3) doubles:
//   [0]                       |f|
//   [1 .. DIM]                int -p n
//   [1 + DIM .. 2 DIM]        int [ nu (G + sym G^T) + nu_x (G + G^T) ] n        G_ab = d_b u_a
//   [1 + 2 DIM]               int u.n
//   [2 + 2 DIM]               int T                  (+0.0 without a scalar)
//   [3 + 2 DIM]               int -kappa grad T . n  (+0.0 without a scalar); with LAW = 1, 4, 5 and ipr = 1 / Pr_t != 0
//                             (subgrid heat flux, nsfem_set_scalar_sgs): int -(kappa + nu_x ipr) grad T . n; with
//                             LAW = 8 and cthv != null (nsfem_set_scalar_sgs_dynamic): int -(kappa + c_K Delta_K^2
//                             gamma) grad T . n, c_K the cell mean of the vertex field C_theta
//   [4 + 2 DIM ..]            int (x - x0) x t, t the sum of the two traction integrands (2D: the z component)
// n = the unit normal pointing out of the facet's cell.
template <int DIM, int LAW>
__global__ __launch_bounds__(256) void k_wall_facets(int nf, int nc, const int32_t* __restrict__ fcell,
                                                     const int32_t* __restrict__ flocal,
                                                     const double* __restrict__ vx, const int32_t* __restrict__ p2,
                                                     const int32_t* __restrict__ p1, const double* __restrict__ u,
                                                     const double* __restrict__ p, const double* __restrict__ T,
                                                     double nu, double sym, double kappa, double ox, double oy,
                                                     double oz, double lp0, double lp1, double lp2, double ipr,
                                                     double* __restrict__ out, const double* __restrict__ cs2v,
                                                     const double* __restrict__ cthv) {
  constexpr int NV = DIM + 1, N2 = DIM == 2 ? 6 : 10, NQ = DIM == 2 ? 2 : 3;
  constexpr int NT = DIM == 2 ? 1 : 3, NW = 2 * DIM + 4 + NT;
  const int f = blockIdx.x * blockDim.x + threadIdx.x;
  if (f >= nf) return;
  const int c = fcell[f], opp = flocal[f];
  double x[NV][3];
#pragma unroll
  for (int v = 0; v < NV; ++v) {
    x[v][2] = 0.0;
#pragma unroll
    for (int d = 0; d < DIM; ++d) x[v][d] = vx[(size_t)(DIM * v + d) * nc + c];
  }
  // gradients of the barycentric coordinates: rows of J^-1 (J = [x1-x0, .., xd-x0]) for lambda_1..d,
  // lambda_0 = 1 - sum;  vol = |T| d!
  double gl[NV][3];
  double vol;
  if (DIM == 2) {
    const double a00 = x[1][0] - x[0][0], a01 = x[2][0] - x[0][0];
    const double a10 = x[1][1] - x[0][1], a11 = x[2][1] - x[0][1];
    const double det = a00 * a11 - a01 * a10, id = 1.0 / det;
    gl[1][0] = a11 * id;  gl[1][1] = -a01 * id;
    gl[2][0] = -a10 * id; gl[2][1] = a00 * id;
    gl[0][0] = -gl[1][0] - gl[2][0];
    gl[0][1] = -gl[1][1] - gl[2][1];
    vol = fabs(det);
  } else {
    double a[3][3];   // columns = edge vectors
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      a[d][0] = x[1][d] - x[0][d];
      a[d][1] = x[2][d] - x[0][d];
      a[d][2] = x[3][d] - x[0][d];
    }
    const double c00 = a[1][1] * a[2][2] - a[1][2] * a[2][1];
    const double c01 = a[1][2] * a[2][0] - a[1][0] * a[2][2];
    const double c02 = a[1][0] * a[2][1] - a[1][1] * a[2][0];
    const double det = a[0][0] * c00 + a[0][1] * c01 + a[0][2] * c02, id = 1.0 / det;
    gl[1][0] = c00 * id;
    gl[1][1] = (a[0][2] * a[2][1] - a[0][1] * a[2][2]) * id;
    gl[1][2] = (a[0][1] * a[1][2] - a[0][2] * a[1][1]) * id;
    gl[2][0] = c01 * id;
    gl[2][1] = (a[0][0] * a[2][2] - a[0][2] * a[2][0]) * id;
    gl[2][2] = (a[0][2] * a[1][0] - a[0][0] * a[1][2]) * id;
    gl[3][0] = c02 * id;
    gl[3][1] = (a[0][1] * a[2][0] - a[0][0] * a[2][1]) * id;
    gl[3][2] = (a[0][0] * a[1][1] - a[0][1] * a[1][0]) * id;
#pragma unroll
    for (int d = 0; d < 3; ++d) gl[0][d] = -gl[1][d] - gl[2][d] - gl[3][d];
    vol = fabs(det);
  }
  // outward unit normal of the facet opposite vertex `opp` and its measure: grad lambda_opp points inward,
  // |f| = |grad lambda_opp| vol / (d-1)!
  double gn = 0.0, nrm[3] = {0.0, 0.0, 0.0};
#pragma unroll
  for (int v = 0; v < NV; ++v)
    if (v == opp) {
#pragma unroll
      for (int d = 0; d < DIM; ++d) nrm[d] = -gl[v][d];
    }
#pragma unroll
  for (int d = 0; d < DIM; ++d) gn += nrm[d] * nrm[d];
  gn = sqrt(gn);
#pragma unroll
  for (int d = 0; d < DIM; ++d) nrm[d] /= gn;
  const double area = gn * vol / (DIM == 2 ? 1.0 : 2.0);
  // Delta_K^2 of the viscosity laws (k_visc_var_cell / k3_visc_var_cell)
  double delta2 = 0.0;
  if constexpr (LAW != 0) {
    if (DIM == 2) delta2 = 0.5 * vol;
    else {
      const double delta = cbrt(vol / 6.0);
      delta2 = delta * delta;
    }
  }
  // LAW 8 (dynamic Smagorinsky): c_K of the facet's cell from the vertex field in the place of the constant
  if constexpr (LAW == 8) lp0 = dynamic_cell_constant<DIM>(p1, cs2v, nc, c);
  // ... and, with the dynamic subgrid heat flux on, c_K Delta_K^2 of the eddy diffusivity from the second vertex field
  double ckd2 = 0.0;
  if constexpr (LAW == 8) {
    if (cthv) ckd2 = dynamic_cell_constant<DIM>(p1, cthv, nc, c) * delta2;
  }
  // nodal data
  const bool have_T = T != nullptr;
  double un[N2][3], pn[NV], Tn[N2];
#pragma unroll
  for (int k = 0; k < N2; ++k) {
    const size_t node = (size_t)p2[(size_t)k * nc + c];
#pragma unroll
    for (int d = 0; d < DIM; ++d) un[k][d] = u[node * DIM + d];
    Tn[k] = have_T ? T[node] : 0.0;
  }
#pragma unroll
  for (int v = 0; v < NV; ++v) pn[v] = p[p1[(size_t)v * nc + c]];
  const double org[3] = {ox, oy, oz};
  const double g2 = 0.21132486540518713;              // (1 - 1/sqrt(3)) / 2
  double fp[3] = {0.0, 0.0, 0.0}, fv[3] = {0.0, 0.0, 0.0}, tq[3] = {0.0, 0.0, 0.0};
  double flux = 0.0, sT = 0.0, heat = 0.0;
  const double w = area / NQ;
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    double fl[3];                                       // barycentric point inside the facet
    if (DIM == 2) {
      fl[0] = q == 0 ? g2 : 1.0 - g2;
      fl[1] = 1.0 - fl[0];
      fl[2] = 0.0;
    } else {
      fl[0] = q == 0 ? 0.0 : 0.5;
      fl[1] = q == 1 ? 0.0 : 0.5;
      fl[2] = q == 2 ? 0.0 : 0.5;
    }
    double lam[NV];
    int t = 0;
#pragma unroll
    for (int v = 0; v < NV; ++v) {
      if (v == opp) lam[v] = 0.0;
      else { lam[v] = t == 0 ? fl[0] : (t == 1 ? fl[1] : fl[2]); ++t; }
    }
    double phi[N2], dphi[N2][3];
    wall_p2_at<DIM>(lam, gl, phi, dphi);
    double uq[3] = {0.0, 0.0, 0.0}, G[3][3] = {{0.0}}, gT[3] = {0.0, 0.0, 0.0}, pq = 0.0, Tq = 0.0;
    double r[3] = {0.0, 0.0, 0.0};
#pragma unroll
    for (int k = 0; k < N2; ++k) {
#pragma unroll
      for (int a = 0; a < DIM; ++a) {
        uq[a] += phi[k] * un[k][a];
#pragma unroll
        for (int b = 0; b < DIM; ++b) G[a][b] += un[k][a] * dphi[k][b];      // d_b u_a
      }
      Tq += phi[k] * Tn[k];
#pragma unroll
      for (int b = 0; b < DIM; ++b) gT[b] += Tn[k] * dphi[k][b];
    }
#pragma unroll
    for (int v = 0; v < NV; ++v) {
      pq += lam[v] * pn[v];
#pragma unroll
      for (int d = 0; d < DIM; ++d) r[d] += lam[v] * x[v][d];
    }
#pragma unroll
    for (int d = 0; d < DIM; ++d) r[d] -= org[d];
    double nux = 0.0, kapx = 0.0;
    if constexpr (LAW != 0) {
      double ss = 0.0;                                  // sum_ab (G_ab + G_ba)^2
#pragma unroll
      for (int a = 0; a < DIM; ++a)
#pragma unroll
        for (int b = 0; b < DIM; ++b) {
          const double s = G[a][b] + G[b][a];
          ss += s * s;
        }
      if constexpr (LAW == 4 || LAW == 5) {
        double Gd[DIM][DIM];                            // the DIM x DIM block the tensor laws take
#pragma unroll
        for (int a = 0; a < DIM; ++a)
#pragma unroll
          for (int b = 0; b < DIM; ++b) Gd[a][b] = G[a][b];
        nux = visc_law_nu_grad<LAW, DIM>(Gd, delta2, lp0);
      } else {
        nux = visc_law_nu<LAW>(sqrt(0.5 * ss), delta2, lp0, lp1, lp2);
        if constexpr (LAW == 8) kapx = ckd2 * sqrt(0.5 * ss);
      }
    }
    double tr[3] = {0.0, 0.0, 0.0};                     // traction at the point
    double hq = 0.0;
#pragma unroll
    for (int a = 0; a < DIM; ++a) {
      const double tp = -pq * nrm[a];
      double tv = 0.0;
#pragma unroll
      for (int b = 0; b < DIM; ++b) {
        tv += nu * (G[a][b] + sym * G[b][a]) * nrm[b];
        if constexpr (LAW != 0) tv += nux * (G[a][b] + G[b][a]) * nrm[b];
      }
      fp[a] += w * tp;
      fv[a] += w * tv;
      tr[a] = tp + tv;
      flux += w * uq[a] * nrm[a];
      hq += gT[a] * nrm[a];
    }
    sT += w * Tq;
    if ((LAW == 1 || LAW == 4 || LAW == 5) && ipr != 0.0) heat += w * (-(kappa + nux * ipr) * hq);
    else if (LAW == 8 && cthv != nullptr) heat += w * (-(kappa + kapx) * hq);
    else heat += w * (-kappa * hq);
    if (DIM == 2) {
      tq[0] += w * (r[0] * tr[1] - r[1] * tr[0]);
    } else {
      tq[0] += w * (r[1] * tr[2] - r[2] * tr[1]);
      tq[1] += w * (r[2] * tr[0] - r[0] * tr[2]);
      tq[2] += w * (r[0] * tr[1] - r[1] * tr[0]);
    }
  }
  double* o = out + (size_t)f * NW;
  o[0] = area;
#pragma unroll
  for (int a = 0; a < DIM; ++a) {
    o[1 + a] = fp[a];
    o[1 + DIM + a] = fv[a];
  }
  o[1 + 2 * DIM] = flux;
  o[2 + 2 * DIM] = have_T ? sT : 0.0;
  o[3 + 2 * DIM] = have_T ? heat : 0.0;
#pragma unroll
  for (int a = 0; a < NT; ++a) o[4 + 2 * DIM + a] = tq[a];
}

// out[g][0 .. NW) = the sum of the rows goff[g] <= f < goff[g + 1].  One workgroup of 256 threads per group: thread t
// adds the rows t, t + 256, ... of the group in ascending order from +0.0, the 256 partials are folded by a
// xor-shuffle tree within each wave and the four wave sums are added in wave order through LDS.  The order depends on
// the group's own facets only; an empty group gives +0.0.
template <int NW>
__global__ __launch_bounds__(256) void k_wall_reduce(const int32_t* __restrict__ goff,
                                                     const double* __restrict__ rows, double* __restrict__ out) {
  __shared__ double sh[4][NW];
  const int g = blockIdx.x, t = threadIdx.x;
  const int begin = goff[g], end = goff[g + 1];
  double acc[NW];
#pragma unroll
  for (int k = 0; k < NW; ++k) acc[k] = 0.0;
  for (int f = begin + t; f < end; f += 256) {
    const double* r = rows + (size_t)f * NW;
#pragma unroll
    for (int k = 0; k < NW; ++k) acc[k] += r[k];
  }
#pragma unroll
  for (int k = 0; k < NW; ++k)
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) acc[k] += __shfl_xor(acc[k], off, 64);
  if ((t & 63) == 0) {
#pragma unroll
    for (int k = 0; k < NW; ++k) sh[t >> 6][k] = acc[k];
  }
  __syncthreads();
  if (t < NW) out[(size_t)g * NW + t] = ((sh[0][t] + sh[1][t]) + sh[2][t]) + sh[3][t];
}

void launch_wall_facets(hipStream_t s, const MeshDev& m, int nf, const int32_t* fcell, const int32_t* flocal,
                        const double* u, const double* p, const double* T, const WallParams& w, double* rows) {
  if (nf <= 0) return;
  NSFEM_REQUIRE(is_viscosity_law(w.law), "wall quantities: unknown viscosity law");
  NSFEM_REQUIRE((w.law == 8) == (w.cs2v != nullptr), "wall quantities: the vertex constants go with law 8 and only with it");
  NSFEM_REQUIRE(w.law == 8 || w.cthv == nullptr, "wall quantities: the vertex field C_theta goes with law 8 only");
  with_int<3, 2>(m.dim, [&](auto dc) {
    with_viscosity_law(w.law, [&](auto lc) {
      hipLaunchKernelGGL((k_wall_facets<decltype(dc)::value, decltype(lc)::value>), dim3((nf + 255) / 256), dim3(256), 0,
                         s, nf, m.n_cells, fcell, flocal, m.vx.p, m.p2.p, m.p1.p, u, p, T, w.nu, w.sym, w.kappa,
                         w.origin[0], w.origin[1], w.origin[2], w.law_p[0], w.law_p[1], w.law_p[2], w.inv_prt, rows,
                         w.cs2v, w.cthv);
    });
  });
  NSFEM_HIP(hipGetLastError());
}

void launch_wall_reduce(hipStream_t s, int dim, int n_groups, const int32_t* goff, const double* rows, double* out) {
  if (n_groups <= 0) return;
  if (dim == 2) hipLaunchKernelGGL((k_wall_reduce<9>), dim3(n_groups), dim3(256), 0, s, goff, rows, out);
  else hipLaunchKernelGGL((k_wall_reduce<13>), dim3(n_groups), dim3(256), 0, s, goff, rows, out);
  NSFEM_HIP(hipGetLastError());
}

}  // namespace nsfem
