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
#include "element_front.hpp"

namespace nsfem {

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
  FacetFront<DIM> F;
  if constexpr (DIM == 2) facet_front(vx, nc, c, opp, F);
  else { NSFEM_FACET_FRONT_3D(vx, nc, c, opp, F) }
  const double(&x)[NV][3] = F.x;
  const double(&gl)[NV][3] = F.gl;
  const double(&nrm)[3] = F.nrm;
  const double vol = F.vol, area = F.area;
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
  gather_p2_vector<DIM, DIM>(p2, nc, c, u, un);
  if (have_T) gather_p2_scalar<DIM>(p2, nc, c, T, Tn);
  else {
#pragma unroll
    for (int k = 0; k < N2; ++k) Tn[k] = 0.0;
  }
  gather_p1<DIM>(p1, nc, c, p, nullptr, pn);
  const double org[3] = {ox, oy, oz};
  double fp[3] = {0.0, 0.0, 0.0}, fv[3] = {0.0, 0.0, 0.0}, tq[3] = {0.0, 0.0, 0.0};
  double flux = 0.0, sT = 0.0, heat = 0.0;
  const double w = area / NQ;
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    double lam[NV];
    if constexpr (DIM == 2) facet_rule_point(q, opp, lam);
    else { NSFEM_FACET_RULE_POINT_3D(q, opp, lam) }
    double phi[N2], dphi[N2][3];
    p2_at<DIM>(lam, gl, phi, dphi);
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
  __shared__ double sh[4 * NW];
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
  block_sum_fixed<NW>(acc, sh);
  store_block_partials<NW>(sh, out, (size_t)g * NW, 1, 0);
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
