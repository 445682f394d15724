// Volume functionals of the discrete solution: measure, |u|^2, |grad u|^2, |curl u|^2, (div u)^2, momentum,
// int p, |p|^2 and |grad p|^2 over a set of cells -- of the state itself or of its difference to a reference
// field (error norms).
//
// Replaces the dolfin.assemble(... * dx) / dolfin.errornorm calls a driver makes after a step (kinetic energy and
// enstrophy of the Taylor-Green runs, |div u| after a projection, convergence_test/taylor_green_vortex.py:118-119)
// -- the volume counterpart of boundary.hip, with the shape of k_cfl: one thread per cell (grid-stride), SoA cell
// data read coalesced, the 6 / 10 nodal velocities and 3 / 4 nodal pressures gathered once, the integrands
// evaluated at the points of the degree-5 rules of the assembly kernels (7 points on triangles, 15-point Keast rule
// on tetrahedra).  Every integrand has degree <= 4 on an affine cell: the sums are the integrals up to rounding.
//
// Reduction without atomics: a thread accumulates its cells in ascending order, a wave folds its 64 lanes with a fixed
// xor-shuffle tree, the 4 waves of a workgroup are added in wave order and stored as one partial per quantity;
// k_fold_partials folds the kVolParts partials of a quantity in a fixed order as well.  Same state, same bytes.
// The P1 gather, the degree-5 tables and both levels of the reduction come from element_front.hpp; the gather of the
// nodal velocities stays here (through the shared helper the compiler fuses the products of |u|^2 the other way round).
#include "cell_geometry.hpp"
#include "element_front.hpp"

namespace nsfem {

NSFEM_FRONT_TABLES(c_fq, c_fq3)
void upload_functional_tables(int dim) { upload_front_tables(dim); }

// parts[j][block]: quantity j of NSFEM_N_FUNCTIONALS (include/nsfem.h) over the cells of the block's threads.
// ur / pr != null: the fields are u - ur / p - pr (formed at the nodes while loading); flags != null: cells with
// flag 0 contribute nothing.
template <int DIM>
__global__ __launch_bounds__(256) void k_vol_functionals(int nc, const double* __restrict__ vx,
                                                         const int32_t* __restrict__ p2,
                                                         const int32_t* __restrict__ p1,
                                                         const double* __restrict__ u,
                                                         const double* __restrict__ p,
                                                         const double* __restrict__ ur,
                                                         const double* __restrict__ pr,
                                                         const uint8_t* __restrict__ flags,
                                                         double* __restrict__ parts) {
  constexpr int N2 = DIM == 2 ? 6 : 10, N1 = DIM + 1, NQ = DIM == 2 ? 7 : 15;
  constexpr int NF = NSFEM_N_FUNCTIONALS;
  __shared__ double sh[4 * NF];
  double acc[NF];
#pragma unroll
  for (int j = 0; j < NF; ++j) acc[j] = 0.0;
  for (int c = blockIdx.x * blockDim.x + threadIdx.x; c < nc; c += gridDim.x * blockDim.x) {
    if (flags && flags[c] == 0) continue;
    double uu[N2][DIM], pp[N1];
#pragma unroll
    for (int k = 0; k < N2; ++k) {
      const size_t node = (size_t)p2[(size_t)k * nc + c];
      if (DIM == 2) {
        double2 v = reinterpret_cast<const double2*>(u)[node];
        if (ur) {
          const double2 r = reinterpret_cast<const double2*>(ur)[node];
          v.x -= r.x;
          v.y -= r.y;
        }
        uu[k][0] = v.x;
        uu[k][1] = v.y;
      } else {
#pragma unroll
        for (int a = 0; a < DIM; ++a) uu[k][a] = u[DIM * node + a];
        if (ur) {
#pragma unroll
          for (int a = 0; a < DIM; ++a) uu[k][a] -= ur[DIM * node + a];
        }
      }
    }
    gather_p1<DIM>(p1, nc, c, p, pr, pp);
    // grad p is constant on the cell: sum_i p_i grad lambda_i, reference gradients (-1, .., -1), e_1, .., e_DIM
    double gp2, adet;
    if constexpr (DIM == 2) {
      const CellGeo g = load_geo(vx, nc, c);
      adet = g.adet;
      double gpx, gpy;
      phys(g, pp[1] - pp[0], pp[2] - pp[0], gpx, gpy);
      gp2 = gpx * gpx + gpy * gpy;
      for (int q = 0; q < NQ; ++q) {
        double uq0 = 0.0, uq1 = 0.0, g00 = 0.0, g01 = 0.0, g10 = 0.0, g11 = 0.0;
#pragma unroll
        for (int k = 0; k < N2; ++k) {
          double gx, gy;
          phys(g, c_fq.dphi2[q][k][0], c_fq.dphi2[q][k][1], gx, gy);
          const double ph = c_fq.phi2[q][k];
          uq0 += ph * uu[k][0];
          uq1 += ph * uu[k][1];
          g00 += gx * uu[k][0];   // d_x u_x
          g01 += gy * uu[k][0];   // d_y u_x
          g10 += gx * uu[k][1];   // d_x u_y
          g11 += gy * uu[k][1];   // d_y u_y
        }
        const double pq = c_fq.phi1[q][0] * pp[0] + c_fq.phi1[q][1] * pp[1] + c_fq.phi1[q][2] * pp[2];
        const double w = c_fq.w[q] * adet;
        const double div = g00 + g11, curl = g10 - g01;
        acc[0] += w;
        acc[1] += w * (uq0 * uq0 + uq1 * uq1);
        acc[2] += w * (g00 * g00 + g01 * g01 + g10 * g10 + g11 * g11);
        acc[3] += w * (curl * curl);
        acc[4] += w * (div * div);
        acc[5] += w * uq0;
        acc[6] += w * uq1;
        acc[8] += w * pq;
        acc[9] += w * (pq * pq);
        acc[10] += w * gp2;
      }
    } else {
      const CellGeo3 g = load_geo3(vx, nc, c);
      adet = g.adet;
      const double dpr[3] = {pp[1] - pp[0], pp[2] - pp[0], pp[3] - pp[0]};
      double gp[3];
      phys3(g, dpr, gp);
      gp2 = gp[0] * gp[0] + gp[1] * gp[1] + gp[2] * gp[2];
      for (int q = 0; q < NQ; ++q) {
        double uq[3] = {0.0, 0.0, 0.0};
        double G[3][3];   // G[a][b] = d_b u_a
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
          for (int b = 0; b < 3; ++b) G[a][b] = 0.0;
#pragma unroll
        for (int k = 0; k < N2; ++k) {
          // (a scheduling fence per half of the nodes: all 40 table entries of a point fetched at once do not fit
          // the scalar registers)
          if (k == 5) asm volatile("" ::: "memory");
          double gk[3];
          phys3(g, c_fq3.dphi2[q][k], gk);
          const double ph = c_fq3.phi2[q][k];
#pragma unroll
          for (int a = 0; a < 3; ++a) {
            uq[a] += ph * uu[k][a];
#pragma unroll
            for (int b = 0; b < 3; ++b) G[a][b] += gk[b] * uu[k][a];
          }
        }
        const double pq = c_fq3.phi1[q][0] * pp[0] + c_fq3.phi1[q][1] * pp[1] + c_fq3.phi1[q][2] * pp[2] +
                          c_fq3.phi1[q][3] * pp[3];
        const double w = c_fq3.w[q] * adet;
        const double div = G[0][0] + G[1][1] + G[2][2];
        const double cx = G[2][1] - G[1][2], cy = G[0][2] - G[2][0], cz = G[1][0] - G[0][1];
        double gg = 0.0;
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
          for (int b = 0; b < 3; ++b) gg += G[a][b] * G[a][b];
        acc[0] += w;
        acc[1] += w * (uq[0] * uq[0] + uq[1] * uq[1] + uq[2] * uq[2]);
        acc[2] += w * gg;
        acc[3] += w * (cx * cx + cy * cy + cz * cz);
        acc[4] += w * (div * div);
        acc[5] += w * uq[0];
        acc[6] += w * uq[1];
        acc[7] += w * uq[2];
        acc[8] += w * pq;
        acc[9] += w * (pq * pq);
        acc[10] += w * gp2;
      }
    }
  }
  block_sum_fixed<NF>(acc, sh);
  store_block_partials<NF>(sh, parts, 0, gridDim.x, blockIdx.x);
}

// out[b] = sum of the n_parts partials parts[b][.] of number b: one wave per number, lane l adds its n_parts / 64
// consecutive partials in index order, then the xor-shuffle tree (a fixed order).  The second level of every two-launch
// reduction of the post-processing
__global__ __launch_bounds__(64) void k_fold_partials(int n_parts, const double* __restrict__ parts,
                                                      double* __restrict__ out) {
  const int per = n_parts / 64;
  const double* src = parts + (size_t)blockIdx.x * n_parts + (size_t)threadIdx.x * per;
  double v = 0.0;
  for (int i = 0; i < per; ++i) v += src[i];
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
  if (threadIdx.x == 0) out[blockIdx.x] = v;
}

void launch_fold_partials(hipStream_t s, int n_numbers, int n_parts, const double* parts, double* out) {
  hipLaunchKernelGGL(k_fold_partials, dim3(n_numbers), dim3(64), 0, s, n_parts, parts, out);
  NSFEM_HIP(hipGetLastError());
}

void launch_vol_functionals(hipStream_t s, const MeshDev& m, const double* u, const double* p, const double* ur,
                            const double* pr, const uint8_t* flags, double* parts, double* out) {
  static_assert(kVolParts % 64 == 0, "k_fold_partials gives every lane the same number of partials");
  if (m.dim == 3)
    hipLaunchKernelGGL(k_vol_functionals<3>, dim3(kVolParts), dim3(256), 0, s, m.n_cells, m.vx.p, m.p2.p, m.p1.p, u,
                       p, ur, pr, flags, parts);
  else
    hipLaunchKernelGGL(k_vol_functionals<2>, dim3(kVolParts), dim3(256), 0, s, m.n_cells, m.vx.p, m.p2.p, m.p1.p, u,
                       p, ur, pr, flags, parts);
  NSFEM_HIP(hipGetLastError());
  launch_fold_partials(s, NSFEM_N_FUNCTIONALS, kVolParts, parts, out);
}

}  // namespace nsfem
