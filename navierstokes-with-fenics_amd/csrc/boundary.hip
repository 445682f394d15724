// Boundary functionals of the discrete solution: surface force (drag / lift), mass flux and
// measure of a set of boundary facets.
//
// Replaces the dolfin.assemble(... * ds(subdomain_id)) calls of the reference's post-processing
// hooks -- demo/dfg_benchmark.py:44-66 (traction = -p n + 1/Re sym(grad u) n integrated over the
// cylinder), demo/gravity_driven_flow.py:66-70 (total mass flux dot(n, u) ds) -- with one thread
// per boundary facet: the adjacent cell's geometry, the 6 / 10 nodal velocities and the 3 / 4
// nodal pressures are gathered once, the integrand is evaluated at the points of a facet rule
// that is exact for it (grad u and p are linear on an affine facet, u.n is quadratic):
// 2D: 2-point Gauss rule on the edge, 3D: the 3 edge midpoints of the face.  Per-facet results
// are stored and summed by the caller in facet order (deterministic, no atomics).
#include "element_front.hpp"

namespace nsfem {

// out[f][0..DIM-1] = int_f ( -p n + nu (grad u + sym grad u^T) n ) dS
// out[f][DIM] = int_f u.n dS ; out[f][DIM+1] = |f|
template <int DIM>
__global__ __launch_bounds__(256) void k_boundary_force(int nf, int nc,
                                                        const int32_t* __restrict__ fcell,
                                                        const int32_t* __restrict__ flocal,
                                                        const double* __restrict__ vx,
                                                        const int32_t* __restrict__ p2,
                                                        const int32_t* __restrict__ p1,
                                                        const double* __restrict__ u,
                                                        const double* __restrict__ p, double nu,
                                                        double sym, double* __restrict__ out) {
  constexpr int NV = DIM + 1, N2 = DIM == 2 ? 6 : 10, NQ = DIM == 2 ? 2 : 3;
  const int f = blockIdx.x * blockDim.x + threadIdx.x;
  if (f >= nf) return;
  const int c = fcell[f], opp = flocal[f];
  FacetFront<DIM> F;
  if constexpr (DIM == 2) facet_front(vx, nc, c, opp, F);
  else { NSFEM_FACET_FRONT_3D(vx, nc, c, opp, F) }
  const double(&gl)[NV][3] = F.gl;
  const double(&nrm)[3] = F.nrm;
  const double area = F.area;
  // nodal data
  double un[N2][3], pn[NV];
  gather_p2_vector<DIM, DIM>(p2, nc, c, u, un);
  gather_p1<DIM>(p1, nc, c, p, nullptr, pn);
  double force[3] = {0.0, 0.0, 0.0}, flux = 0.0;
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    double lam[NV];
    if constexpr (DIM == 2) facet_rule_point(q, opp, lam);
    else { NSFEM_FACET_RULE_POINT_3D(q, opp, lam) }
    double phi[N2], dphi[N2][3];
    p2_at<DIM>(lam, gl, phi, dphi);
    double uq[3] = {0.0, 0.0, 0.0}, G[3][3] = {{0.0}}, pq = 0.0;
#pragma unroll
    for (int k = 0; k < N2; ++k)
#pragma unroll
      for (int a = 0; a < DIM; ++a) {
        uq[a] += phi[k] * un[k][a];
#pragma unroll
        for (int b = 0; b < DIM; ++b) G[a][b] += un[k][a] * dphi[k][b];      // d_b u_a
      }
#pragma unroll
    for (int v = 0; v < NV; ++v) pq += lam[v] * pn[v];
    const double w = area / NQ;
#pragma unroll
    for (int a = 0; a < DIM; ++a) {
      double s = -pq * nrm[a];
#pragma unroll
      for (int b = 0; b < DIM; ++b) s += nu * (G[a][b] + sym * G[b][a]) * nrm[b];
      force[a] += w * s;
      flux += w * uq[a] * nrm[a];
    }
  }
  double* o = out + (size_t)f * (DIM + 2);
#pragma unroll
  for (int a = 0; a < DIM; ++a) o[a] = force[a];
  o[DIM] = flux;
  o[DIM + 1] = area;
}

void launch_boundary_force(hipStream_t s, const MeshDev& m, int nf, const int32_t* fcell,
                           const int32_t* flocal, const double* u, const double* p, double nu,
                           double sym, double* out) {
  if (nf <= 0) return;
  const int grid = (nf + 255) / 256;
  if (m.dim == 2)
    hipLaunchKernelGGL((k_boundary_force<2>), dim3(grid), dim3(256), 0, s, nf, m.n_cells, fcell, flocal,
                       m.vx.p, m.p2.p, m.p1.p, u, p, nu, sym, out);
  else
    hipLaunchKernelGGL((k_boundary_force<3>), dim3(grid), dim3(256), 0, s, nf, m.n_cells, fcell, flocal,
                       m.vx.p, m.p2.p, m.p1.p, u, p, nu, sym, out);
  NSFEM_HIP(hipGetLastError());
}

}  // namespace nsfem
