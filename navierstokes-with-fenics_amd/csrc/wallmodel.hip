// Wall-stress models in the IMEX step (nsfem_set_wall_model): the third explicit term W(u) next to V(u) and B(u).
//
// A modelled facet f of cell K keeps u.n = 0 only (a component-wise Dirichlet row); its tangential stress comes from a
// law of the wall sampled inside the flow.  Per point q of the facet rule the host fixed a sample cell, the barycentric
// coordinates lambda_s of the sample point in it and the wall distance y (wall_models.py); then
//   U = u(x_s) - u_w,  u_par = U - (U.n) n,  Re_y = y |u_par| / nu,  r = y+^2 / Re_y  (r(0) = 1)
//   W(u)_(i,a) = sum_f sum_q  w_q (nu r / y) u_par,a  phi_i(x_q)
// so the term never divides by |u_par|.  The rule is part of the definition: 3-point Gauss-Legendre on an edge, the
// symmetric 6-point rule of degree 4 on a face (phi_i u_par r is no polynomial; the 2-point and midpoint rules of
// wall.hip are exact for degree 3 / 2 only, and the midpoint rule gives the vertex nodes no load).
//
// Two launches per evaluation, plain vector stores into rows owned by the thread, no atomics -- the same state gives
// the same bytes:
//   k_wm_facets<DIM, LAW>  one thread per modelled facet: the facet vector [NF2][DIM] of its 3 / 6 P2 nodes and one
//                          diagnostics row  |f|, int tau_w [DIM], int u_tau, int y+, max y+
//   k_wm_gather            one thread per node on a modelled facet: v = the node's (facet, local) entries summed in
//                          ascending facet order from +0.0, then per component  n += v,  rhs -= b0 v  (two roundings,
//                          no contraction: the rule of k_visc_gather)
// Laws (template parameter, as the viscosity laws): 1 Werner-Wengle, pointwise and closed; 2 Reichardt, solved by a
// FIXED number of Newton steps from the law-1 value -- the same count in every lane, no data-dependent exit.
#include "element_front.hpp"

namespace nsfem {

// Newton steps of law 2: the smallest count at which the host restatement's |g| / Re_y is <= 1e-15 over 4001
// log-spaced Re_y in [1e-6, 1e8] (4: 5.4e-3, 2.5e-6, 5.2e-13, 4.8e-16 after steps 1 .. 4), plus one
constexpr int kWallNewtonSteps = 5;

// y+ of Werner-Wengle: sqrt(Re_y) in the sublayer, (Re_y / A)^(1 / (1 + B)) above the switch A^(2 / (1 - B));
// e = 1 / (1 + B) and the switch come from the host
__device__ __forceinline__ double wm_werner_wengle(double re, double A, double e, double re_switch) {
  return re <= re_switch ? sqrt(re) : pow(re / A, e);
}

// u+(y+) of Reichardt and its derivative.  log1p / expm1: the plain forms lose four digits at small y+
__device__ __forceinline__ void wm_reichardt(double yp, double kappa, double C, double& up, double& dup) {
  const double e11 = exp(-yp / 11.0), e3 = exp(-yp / 3.0);
  up = log1p(kappa * yp) / kappa + C * (-expm1(-yp / 11.0) - (yp / 11.0) * e3);
  dup = 1.0 / (1.0 + kappa * yp) + C * (e11 / 11.0 - e3 / 11.0 + (yp / 33.0) * e3);
}

// y+ of the law at Re_y > 0.  (p0, p1): law 1 unused, law 2 (kappa, C); (s0, s1, s2): the Werner-Wengle triple
// (A, 1 / (1 + B), switch) -- the law's own for law 1, that of the default constants as the start value of law 2
template <int LAW>
__device__ __forceinline__ double wm_yplus(double re, double p0, double p1, double s0, double s1, double s2) {
  double yp = wm_werner_wengle(re, s0, s1, s2);
  if constexpr (LAW == 2) {
#pragma unroll 1
    for (int it = 0; it < kWallNewtonSteps; ++it) {
      double up, dup;
      wm_reichardt(yp, p0, p1, up, dup);
      const double g = yp * up - re, dg = up + yp * dup;
      yp = fmax(yp - g / dg, 0.25 * yp);         // (every step floored at a quarter of the iterate)
    }
  }
  return yp;
}

// point q of the facet rule in the facet's own barycentric coordinates and its weight (the weights sum to 1):
// edge: 3-point Gauss-Legendre; face: the symmetric 6-point rule of degree 4, points (1 - 2a, a, a) and permutations
template <int DIM>
__device__ __forceinline__ double wm_rule_point(int q, double (&fl)[3]) {
  if constexpr (DIM == 2) {
    const double g = 0.3872983346207417;                // sqrt(3 / 5) / 2
    fl[0] = q == 0 ? 0.5 + g : (q == 1 ? 0.5 : 0.5 - g);
    fl[1] = q == 0 ? 0.5 - g : (q == 1 ? 0.5 : 0.5 + g);
    fl[2] = 0.0;
    return q == 1 ? 0.4444444444444444 : 0.2777777777777778;
  } else {
    const double a = q < 3 ? 0.44594849091596483 : 0.09157621350977073;
    const double b = q < 3 ? 0.10810301816807033 : 0.8168475729804585;
    const int k = q < 3 ? q : q - 3;
    fl[0] = k == 0 ? b : a;
    fl[1] = k == 1 ? b : a;
    fl[2] = k == 2 ? b : a;
    return q < 3 ? 0.22338158967801144 : 0.10995174365532187;
  }
}

// local P2 node k of a cell lies on the facet opposite vertex opp
template <int DIM>
__device__ __forceinline__ bool wm_on_facet(int k, int opp) {
  constexpr int NV = DIM + 1;
  if (k < NV) return k != opp;
  return edge_end<DIM>(k - NV, 0) != opp && edge_end<DIM>(k - NV, 1) != opp;
}

// scell [nf][NQ], slam [nf][NQ][DIM + 1], sy [nf][NQ], uw [nf][DIM] or null; fvec [nf][NF2][DIM] (the facet's nodes:
// its vertices ascending, then its edge nodes ascending, in the local numbering of the cell), rows [nf][DIM + 4].
// weight scales the facet vector only.  The per-facet arrays are read with a stride of a row per lane: a facet set is
// a boundary, thousands of rows at most, and every row is read once.
template <int DIM, int LAW>
__global__ __launch_bounds__(256) void k_wm_facets(int nf, int nc, const int32_t* __restrict__ fcell,
                                                   const int32_t* __restrict__ flocal,
                                                   const int32_t* __restrict__ scell, const double* __restrict__ slam,
                                                   const double* __restrict__ sy, const double* __restrict__ uw,
                                                   const double* __restrict__ vx, const int32_t* __restrict__ p2,
                                                   const double* __restrict__ u, double nu, double weight, double p0,
                                                   double p1, double s0, double s1, double s2,
                                                   double* __restrict__ fvec, double* __restrict__ rows) {
  constexpr int NV = DIM + 1, N2 = DIM == 2 ? 6 : 10, NQ = DIM == 2 ? 3 : 6, NF2 = DIM == 2 ? 3 : 6;
  const int f = blockIdx.x * blockDim.x + threadIdx.x;
  if (f >= nf) return;
  const int c = fcell[f], opp = flocal[f];
  FacetFront<DIM> F;
  if constexpr (DIM == 2) facet_front(vx, nc, c, opp, F);
  else { NSFEM_FACET_FRONT_3D(vx, nc, c, opp, F) }
  double wall[DIM];
#pragma unroll
  for (int a = 0; a < DIM; ++a) wall[a] = uw ? uw[(size_t)f * DIM + a] : 0.0;
  double acc[N2][DIM], tau[DIM];
#pragma unroll
  for (int k = 0; k < N2; ++k)
#pragma unroll
    for (int a = 0; a < DIM; ++a) acc[k][a] = 0.0;
#pragma unroll
  for (int a = 0; a < DIM; ++a) tau[a] = 0.0;
  double sut = 0.0, syp = 0.0, ypmax = 0.0;
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    // the sample: u at lambda_s of the sample cell
    const size_t fq = (size_t)f * NQ + q;
    const int sc = scell[fq];
    const double y = sy[fq];
    double ls[NV], phis[N2], un[N2][DIM];
#pragma unroll
    for (int v = 0; v < NV; ++v) ls[v] = slam[fq * NV + v];
    p2_at<DIM>(ls, phis);
    gather_p2_vector<DIM, DIM>(p2, nc, sc, u, un);
    double U[DIM], un_dot = 0.0;
#pragma unroll
    for (int a = 0; a < DIM; ++a) {
      double s = 0.0;
#pragma unroll
      for (int k = 0; k < N2; ++k) s += phis[k] * un[k][a];
      U[a] = s - wall[a];
      un_dot += U[a] * F.nrm[a];
    }
    double upar[DIM], m2 = 0.0;
#pragma unroll
    for (int a = 0; a < DIM; ++a) {
      upar[a] = U[a] - un_dot * F.nrm[a];
      m2 += upar[a] * upar[a];
    }
    // the law: Re_y = 0 gives y+ = 0, r = 1
    const double re = y * sqrt(m2) / nu;
    const bool pos = re > 0.0;
    const double rs = pos ? re : 1.0;
    double yp = wm_yplus<LAW>(rs, p0, p1, s0, s1, s2);
    const double r = pos ? yp * yp / rs : 1.0;
    yp = pos ? yp : 0.0;
    // the point of the rule in the cell and the facet's basis functions there (those of the other nodes vanish)
    double fl[3], lam[NV], phi[N2];
    const double wq = wm_rule_point<DIM>(q, fl) * F.area;
    int t = 0;
#pragma unroll
    for (int v = 0; v < NV; ++v) {
      if (v == opp) lam[v] = 0.0;
      else { lam[v] = t == 0 ? fl[0] : (t == 1 ? fl[1] : fl[2]); ++t; }
    }
    p2_at<DIM>(lam, phi);
    const double coef = wq * (nu * r / y);
#pragma unroll
    for (int a = 0; a < DIM; ++a) {
      const double ta = coef * upar[a];
      tau[a] += ta;
#pragma unroll
      for (int k = 0; k < N2; ++k) acc[k][a] += ta * phi[k];
    }
    sut += wq * (nu * yp / y);
    syp += wq * yp;
    ypmax = fmax(ypmax, yp);
  }
  // the facet's nodes in their order: a running position, every store to the facet's own row
  double* o = fvec + (size_t)f * NF2 * DIM;
  int t = 0;
#pragma unroll
  for (int k = 0; k < N2; ++k) {
    if (wm_on_facet<DIM>(k, opp)) {
#pragma unroll
      for (int a = 0; a < DIM; ++a) o[t * DIM + a] = weight * acc[k][a];
      ++t;
    }
  }
  double* row = rows + (size_t)f * (DIM + 4);
  row[0] = F.area;
#pragma unroll
  for (int a = 0; a < DIM; ++a) row[1 + a] = tau[a];
  row[1 + DIM] = sut;
  row[2 + DIM] = syp;
  row[3 + DIM] = ypmax;
}

// One thread per node on a modelled facet.  nodes [n_nodes]: the P2 node; nptr [n_nodes + 1], entry: the node's rows
// of fvec (facet * NF2 + local), ascending.  rhs null: the plain sum (the hook, and N2 formed afresh)
__global__ __launch_bounds__(256) void k_wm_gather(int n_nodes, int dim, const int32_t* __restrict__ nodes,
                                                   const int32_t* __restrict__ nptr, const int32_t* __restrict__ entry,
                                                   const double* __restrict__ fvec, double b0, double* __restrict__ n1,
                                                   double* __restrict__ rhs) {
#pragma clang fp contract(off)
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_nodes) return;
  const size_t node = (size_t)nodes[i];
  const int begin = nptr[i], end = nptr[i + 1];
  for (int a = 0; a < dim; ++a) {
    double v = 0.0;
    for (int k = begin; k < end; ++k) v += fvec[(size_t)entry[k] * dim + a];
    const size_t t = node * dim + a;
    n1[t] += v;
    if (rhs) rhs[t] -= b0 * v;
  }
}

void launch_wall_model_facets(hipStream_t s, const MeshDev& m, const WallModelDev& w, const double* u, double nu,
                              double weight) {
  if (w.n_facets <= 0) return;
  NSFEM_REQUIRE(w.law == 1 || w.law == 2, "wall model: no law set");
  with_int<3, 2>(m.dim, [&](auto dc) {
    with_int<1, 2>(w.law, [&](auto lc) {
      hipLaunchKernelGGL((k_wm_facets<decltype(dc)::value, decltype(lc)::value>), dim3((w.n_facets + 255) / 256),
                         dim3(256), 0, s, w.n_facets, m.n_cells, w.fcell.p, w.flocal.p, w.scell.p, w.slam.p, w.sy.p,
                         w.have_uw ? w.uw.p : nullptr, m.vx.p, m.p2.p, u, nu, weight, w.p[0], w.p[1], w.start[0],
                         w.start[1], w.start[2], w.fvec.p, w.rows.p);
    });
  });
  NSFEM_HIP(hipGetLastError());
}

void launch_wall_model_gather(hipStream_t s, const MeshDev& m, const WallModelDev& w, double b0, double* n1,
                              double* rhs) {
  if (w.n_nodes <= 0) return;
  hipLaunchKernelGGL(k_wm_gather, dim3((w.n_nodes + 255) / 256), dim3(256), 0, s, w.n_nodes, m.dim, w.nodes.p,
                     w.nptr.p, w.entry.p, w.fvec.p, b0, n1, rhs);
  NSFEM_HIP(hipGetLastError());
}

}  // namespace nsfem
