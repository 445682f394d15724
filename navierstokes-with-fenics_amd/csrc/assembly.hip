// Element integration kernels for P2/P1 Taylor-Hood triangles on gfx950.
//
// Replaces the FFC/uflacs generated tabulate_tensor kernels + dolfin::Assembler
// cell loops that the reference triggers at source/ns_ipcs_solver.py:126-141,
// 160-169,183-193 and source/ns_bdf_solver.py:68-94.
//
// Layout choices (MI355X):
//   * one thread per (cell, test function i): consecutive lanes = consecutive
//     cells, so every per-cell array (vertex coords, dof maps, slot maps) is stored
//     SoA [k][n_cells] and read fully coalesced (512 B per wave-instruction);
//   * reference basis tables live in __constant__ memory: the quadrature index is
//     wave-uniform, so they arrive through the scalar cache (s_load) and occupy no
//     VGPRs / LDS;
//   * element tensors stay in registers (<= 24 fp64 accumulators per thread);
//   * no atomics: every element tensor is written with plain stores to an element
//     buffer indexed by (cell, i, j); a second kernel sums, for every CSR slot / dof,
//     the entries listed in a precomputed inverted index in a fixed order.  Results
//     are bitwise reproducible and each CSR value is written exactly once.
//
// All integrands are polynomials of degree <= 5 on affine cells, so the 7-point
// degree-5 rule reproduces FEniCS' integrals to round-off.
#include "nsfem_internal.hpp"
#include "cell_geometry.hpp"
#include "bodies.hpp"

namespace nsfem {

__constant__ QuadTables c_q;

void upload_quad_tables(const QuadTables& t) {
  NSFEM_HIP(hipMemcpyToSymbol(HIP_SYMBOL(c_q), &t, sizeof(QuadTables)));
}

// ------------------------------------------------------------------ scalar P2
__global__ __launch_bounds__(256) void k_p2_scalar(int nc, const double* __restrict__ vx,
                                                   const int32_t* __restrict__ slot,
                                                   double* __restrict__ mass,
                                                   double* __restrict__ stiff) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (int64_t)nc * 6) return;
  const int i = (int)(t / nc), c = (int)(t % nc);
  const CellGeo g = load_geo(vx, nc, c);
  double m[6], k[6];
#pragma unroll
  for (int j = 0; j < 6; ++j) m[j] = k[j] = 0.0;
  for (int q = 0; q < 7; ++q) {
    const double w = c_q.w[q] * g.adet;
    double gix, giy;
    phys(g, c_q.dphi2[q][i][0], c_q.dphi2[q][i][1], gix, giy);
    const double pi = c_q.phi2[q][i] * w;
#pragma unroll
    for (int j = 0; j < 6; ++j) {
      double gjx, gjy;
      phys(g, c_q.dphi2[q][j][0], c_q.dphi2[q][j][1], gjx, gjy);
      m[j] += pi * c_q.phi2[q][j];
      k[j] += w * (gix * gjx + giy * gjy);
    }
  }
#pragma unroll
  for (int j = 0; j < 6; ++j) {
    const size_t s = ((size_t)c * 6 + i) * 6 + j;     // element-buffer index (cell, i, j)
    mass[s] = m[j];
    stiff[s] = k[j];
  }
}

// ------------------------------------------------------------------ scalar P1
__global__ __launch_bounds__(256) void k_p1_scalar(int nc, const double* __restrict__ vx,
                                                   const int32_t* __restrict__ slot,
                                                   double* __restrict__ stiff,
                                                   double* __restrict__ mass) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (int64_t)nc * 3) return;
  const int i = (int)(t / nc), c = (int)(t % nc);
  const CellGeo g = load_geo(vx, nc, c);
  const double dl[3][2] = {{-1.0, -1.0}, {1.0, 0.0}, {0.0, 1.0}};
  double gix, giy;
  phys(g, dl[i][0], dl[i][1], gix, giy);
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    double gjx, gjy;
    phys(g, dl[j][0], dl[j][1], gjx, gjy);
    double m = 0.0;
    for (int q = 0; q < 7; ++q) m += c_q.w[q] * c_q.phi1[q][i] * c_q.phi1[q][j];
    const size_t s = ((size_t)c * 3 + i) * 3 + j;
    stiff[s] = 0.5 * g.adet * (gix * gjx + giy * gjy);
    mass[s] = m * g.adet;
  }
}

// --------------------------------------------------- divergence (P1 rows, 1x2)
__global__ __launch_bounds__(256) void k_div(int nc, const double* __restrict__ vx,
                                             const int32_t* __restrict__ slot12,
                                             double* __restrict__ div) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (int64_t)nc * 3) return;
  const int i = (int)(t / nc), c = (int)(t % nc);
  const CellGeo g = load_geo(vx, nc, c);
  double dx[6], dy[6];
#pragma unroll
  for (int j = 0; j < 6; ++j) dx[j] = dy[j] = 0.0;
  for (int q = 0; q < 7; ++q) {
    const double wp = c_q.w[q] * g.adet * c_q.phi1[q][i];
#pragma unroll
    for (int j = 0; j < 6; ++j) {
      double gjx, gjy;
      phys(g, c_q.dphi2[q][j][0], c_q.dphi2[q][j][1], gjx, gjy);
      dx[j] += wp * gjx;
      dy[j] += wp * gjy;
    }
  }
#pragma unroll
  for (int j = 0; j < 6; ++j) {
    const size_t s = ((size_t)c * 3 + i) * 6 + j;
    div[2 * s] = dx[j];
    div[2 * s + 1] = dy[j];
  }
}

// --------------------------- gradient / transposed divergence (P2 rows, 2x1)
__global__ __launch_bounds__(256) void k_grad(int nc, const double* __restrict__ vx,
                                              const int32_t* __restrict__ slot21,
                                              double* __restrict__ grad,
                                              double* __restrict__ divT) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (int64_t)nc * 6) return;
  const int i = (int)(t / nc), c = (int)(t % nc);
  const CellGeo g = load_geo(vx, nc, c);
  const double dl[3][2] = {{-1.0, -1.0}, {1.0, 0.0}, {0.0, 1.0}};
  double gr[3][2], dt[3][2];
#pragma unroll
  for (int j = 0; j < 3; ++j) gr[j][0] = gr[j][1] = dt[j][0] = dt[j][1] = 0.0;
  for (int q = 0; q < 7; ++q) {
    const double w = c_q.w[q] * g.adet;
    const double pi = c_q.phi2[q][i] * w;
    double gix, giy;
    phys(g, c_q.dphi2[q][i][0], c_q.dphi2[q][i][1], gix, giy);
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      double gjx, gjy;
      phys(g, dl[j][0], dl[j][1], gjx, gjy);
      gr[j][0] += pi * gjx;                       // int phi_i d_x psi_j
      gr[j][1] += pi * gjy;
      dt[j][0] += w * gix * c_q.phi1[q][j];       // int d_x phi_i psi_j
      dt[j][1] += w * giy * c_q.phi1[q][j];
    }
  }
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const size_t s = ((size_t)c * 6 + i) * 3 + j;
    grad[2 * s] = gr[j][0];
    grad[2 * s + 1] = gr[j][1];
    divT[2 * s] = dt[j][0];
    divT[2 * s + 1] = dt[j][1];
  }
}

// ----------- traction-form extra block  E[(i,a),(j,b)] = int d_b phi_i d_a phi_j
__global__ __launch_bounds__(256) void k_visc_extra(int nc, const double* __restrict__ vx,
                                                    const int32_t* __restrict__ slot,
                                                    double* __restrict__ E) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (int64_t)nc * 6) return;
  const int i = (int)(t / nc), c = (int)(t % nc);
  const CellGeo g = load_geo(vx, nc, c);
  double acc[6][4];
#pragma unroll
  for (int j = 0; j < 6; ++j) acc[j][0] = acc[j][1] = acc[j][2] = acc[j][3] = 0.0;
  for (int q = 0; q < 7; ++q) {
    const double w = c_q.w[q] * g.adet;
    double gi[2];
    phys(g, c_q.dphi2[q][i][0], c_q.dphi2[q][i][1], gi[0], gi[1]);
#pragma unroll
    for (int j = 0; j < 6; ++j) {
      double gj[2];
      phys(g, c_q.dphi2[q][j][0], c_q.dphi2[q][j][1], gj[0], gj[1]);
#pragma unroll
      for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) acc[j][a * 2 + b] += w * gi[b] * gj[a];
    }
  }
#pragma unroll
  for (int j = 0; j < 6; ++j) {
    const size_t s = ((size_t)c * 6 + i) * 6 + j;
#pragma unroll
    for (int e = 0; e < 4; ++e) E[4 * s + e] = acc[j][e];
  }
}

// ----------------------------------------------------- J = L (x) I_2 + cvE * E
__global__ __launch_bounds__(256) void k_jac_init(int nnz, const double* __restrict__ L,
                                                  const double* __restrict__ E, double cvE,
                                                  double* __restrict__ J) {
  for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < nnz;
       k += (int64_t)gridDim.x * blockDim.x) {
    const double l = L[k];
    double2 r0 = make_double2(l, 0.0), r1 = make_double2(0.0, l);
    if (E) {
      const double2 e0 = reinterpret_cast<const double2*>(E)[2 * k];
      const double2 e1 = reinterpret_cast<const double2*>(E)[2 * k + 1];
      r0.x += cvE * e0.x; r0.y += cvE * e0.y;
      r1.x += cvE * e1.x; r1.y += cvE * e1.y;
    }
    reinterpret_cast<double2*>(J)[2 * k] = r0;
    reinterpret_cast<double2*>(J)[2 * k + 1] = r1;
  }
}

// ---- convection blocks of the Newton (or Picard) matrix for the four weak forms of
// source/ns_solver_base.py:370-390 (Gateaux derivatives) / :478-499 (Picard linearisations).
// FORM: 0 standard, 1 rotational, 2 divergence, 3 skew-symmetric.  With u, G = grad u,
// div, curl at the quadrature point, test (phi_i, a), trial (phi_j, b):
//   standard    phi_i [ (u.g_j) d_ab + phi_j G_ab ]                 (Picard: first term)
//   divergence  standard + 1/2 phi_i [ g_j,b u_a + div phi_j d_ab ] (Picard: 1st + 4th term)
//   skew        1/2 standard - 1/2 [ g_i,b phi_j u_a + (u.g_i) phi_j d_ab ]
//   rotational  phi_i e_a [ dcurl_j,b u_(1-a) + curl phi_j d_(b,1-a) ],  e = (-1, +1)
template <int FORM, bool PICARD>
__global__ __launch_bounds__(256) void k_conv_jac(int nc, const double* __restrict__ vx,
                                                  const int32_t* __restrict__ p2,
                                                  const double* __restrict__ u, double cc,
                                                  double* __restrict__ ebuf) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (int64_t)nc * 6) return;
  const int i = (int)(t / nc), c = (int)(t % nc);
  const CellGeo g = load_geo(vx, nc, c);
  double ux[6], uy[6];
#pragma unroll
  for (int k = 0; k < 6; ++k) {
    const int node = p2[(size_t)k * nc + c];
    const double2 v = reinterpret_cast<const double2*>(u)[node];
    ux[k] = v.x;
    uy[k] = v.y;
  }
  double acc[6][4];
#pragma unroll
  for (int j = 0; j < 6; ++j) acc[j][0] = acc[j][1] = acc[j][2] = acc[j][3] = 0.0;
  for (int q = 0; q < 7; ++q) {
    double gx[6], gy[6];
    double uqx = 0.0, uqy = 0.0, g00 = 0.0, g01 = 0.0, g10 = 0.0, g11 = 0.0;
    double gix = 0.0, giy = 0.0;
#pragma unroll
    for (int k = 0; k < 6; ++k) {
      phys(g, c_q.dphi2[q][k][0], c_q.dphi2[q][k][1], gx[k], gy[k]);
      const double ph = c_q.phi2[q][k];
      uqx += ph * ux[k];
      uqy += ph * uy[k];
      g00 += gx[k] * ux[k];   // d_x u_x
      g01 += gy[k] * ux[k];   // d_y u_x
      g10 += gx[k] * uy[k];   // d_x u_y
      g11 += gy[k] * uy[k];   // d_y u_y
      if (k == i) { gix = gx[k]; giy = gy[k]; }
    }
    const double w = c_q.w[q] * g.adet * cc;
    const double wpi = w * c_q.phi2[q][i];
    const double div = g00 + g11, curl = g10 - g01;
    const double udgi = uqx * gix + uqy * giy;
#pragma unroll
    for (int j = 0; j < 6; ++j) {
      const double udg = uqx * gx[j] + uqy * gy[j];
      const double pj = c_q.phi2[q][j];
      if (FORM == 0) {
        acc[j][0] += wpi * (udg + (PICARD ? 0.0 : pj * g00));
        acc[j][3] += wpi * (udg + (PICARD ? 0.0 : pj * g11));
        if (!PICARD) {
          acc[j][1] += wpi * (pj * g01);
          acc[j][2] += wpi * (pj * g10);
        }
      } else if (FORM == 2) {
        const double hd = 0.5 * div * pj;
        acc[j][0] += wpi * (udg + hd + (PICARD ? 0.0 : pj * g00 + 0.5 * gx[j] * uqx));
        acc[j][3] += wpi * (udg + hd + (PICARD ? 0.0 : pj * g11 + 0.5 * gy[j] * uqy));
        if (!PICARD) {
          acc[j][1] += wpi * (pj * g01 + 0.5 * gy[j] * uqx);
          acc[j][2] += wpi * (pj * g10 + 0.5 * gx[j] * uqy);
        }
      } else if (FORM == 3) {
        const double sk = 0.5 * (wpi * udg - w * udgi * pj);
        acc[j][0] += sk;
        acc[j][3] += sk;
        if (!PICARD) {
          const double hw = 0.5 * w * pj;
          acc[j][0] += 0.5 * wpi * pj * g00 - hw * gix * uqx;
          acc[j][1] += 0.5 * wpi * pj * g01 - hw * giy * uqx;
          acc[j][2] += 0.5 * wpi * pj * g10 - hw * gix * uqy;
          acc[j][3] += 0.5 * wpi * pj * g11 - hw * giy * uqy;
        }
      } else {   // rotational: rows a = 0 (e = -1, u_1) and a = 1 (e = +1, u_0)
        const double cj = curl * pj;
        acc[j][1] += wpi * (-cj);          // a = 0, b = 1 = 1 - a
        acc[j][2] += wpi * (cj);           // a = 1, b = 0
        if (!PICARD) {
          // dcurl_j,0 = -d_y phi_j ; dcurl_j,1 = d_x phi_j
          acc[j][0] += wpi * (gy[j] * uqy);
          acc[j][1] += wpi * (-gx[j] * uqy);
          acc[j][2] += wpi * (-gy[j] * uqx);
          acc[j][3] += wpi * (gx[j] * uqx);
        }
      }
    }
  }
  // plain stores of the 6 blocks of row i: ebuf[cell][i][j][4]
  double2* out = reinterpret_cast<double2*>(ebuf) + ((size_t)c * 36 + (size_t)i * 6) * 2;
#pragma unroll
  for (int j = 0; j < 6; ++j) {
    out[2 * j] = make_double2(acc[j][0], acc[j][1]);
    out[2 * j + 1] = make_double2(acc[j][2], acc[j][3]);
  }
}

// J[s] = L[s] (x) I_2 + cvE * E[s] + sum of the element blocks scattered to slot s, summed
// in ascending (cell, i, j) order: deterministic, every value written exactly once
__global__ __launch_bounds__(256) void k_jac_gather(int nnz, const int32_t* __restrict__ cptr,
                                                    const int32_t* __restrict__ cidx,
                                                    const double* __restrict__ ebuf,
                                                    const double* __restrict__ L,
                                                    const double* __restrict__ E, double cvE,
                                                    double* __restrict__ J) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= nnz) return;
  const double l = L[s];
  double2 r0 = make_double2(l, 0.0), r1 = make_double2(0.0, l);
  if (E) {
    const double2 e0 = reinterpret_cast<const double2*>(E)[2 * (size_t)s];
    const double2 e1 = reinterpret_cast<const double2*>(E)[2 * (size_t)s + 1];
    r0.x += cvE * e0.x; r0.y += cvE * e0.y;
    r1.x += cvE * e1.x; r1.y += cvE * e1.y;
  }
  for (int k = cptr[s]; k < cptr[s + 1]; ++k) {
    const double2* src = reinterpret_cast<const double2*>(ebuf) + 2 * (size_t)cidx[k];
    const double2 a = src[0], b = src[1];
    r0.x += a.x; r0.y += a.y;
    r1.x += b.x; r1.y += b.y;
  }
  reinterpret_cast<double2*>(J)[2 * (size_t)s] = r0;
  reinterpret_cast<double2*>(J)[2 * (size_t)s + 1] = r1;
}

// ---- CFL diagnostic (reference source/ns_problem.py:554-587): cell-local L2 projection onto
// DG2 of  degree |u| k / h  (degree = 2, h = dolfin CellDiameter = circumdiameter) with the
// degree-4 rule, then the max-norm of the coefficients.  One thread per cell, one partial max
// per block.
__global__ __launch_bounds__(256) void k_cfl(int nc, const double* __restrict__ vx,
                                             const int32_t* __restrict__ p2,
                                             const double* __restrict__ u, double scale,
                                             double* __restrict__ parts) {
  __shared__ double sh[4];
  double best = 0.0;
  for (int c = blockIdx.x * blockDim.x + threadIdx.x; c < nc; c += gridDim.x * blockDim.x) {
    const double x0 = vx[c], y0 = vx[(size_t)nc + c];
    const double x1 = vx[(size_t)2 * nc + c], y1 = vx[(size_t)3 * nc + c];
    const double x2 = vx[(size_t)4 * nc + c], y2 = vx[(size_t)5 * nc + c];
    const double la = sqrt((x1 - x2) * (x1 - x2) + (y1 - y2) * (y1 - y2));
    const double lb = sqrt((x0 - x2) * (x0 - x2) + (y0 - y2) * (y0 - y2));
    const double lc = sqrt((x0 - x1) * (x0 - x1) + (y0 - y1) * (y0 - y1));
    const double area2 = fabs((x1 - x0) * (y2 - y0) - (x2 - x0) * (y1 - y0));
    const double h = la * lb * lc / area2;                  // 2 R = abc / (2 A)
    double ux[6], uy[6], f[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) {
      const double2 v = reinterpret_cast<const double2*>(u)[p2[(size_t)k * nc + c]];
      ux[k] = v.x;
      uy[k] = v.y;
    }
#pragma unroll
    for (int q = 0; q < 6; ++q) {
      double a = 0.0, b = 0.0;
#pragma unroll
      for (int k = 0; k < 6; ++k) {
        a += c_q.cfl_phi[q][k] * ux[k];
        b += c_q.cfl_phi[q][k] * uy[k];
      }
      f[q] = scale * sqrt(a * a + b * b) / h;
    }
#pragma unroll
    for (int i = 0; i < 6; ++i) {
      double ci = 0.0;
#pragma unroll
      for (int q = 0; q < 6; ++q) ci += c_q.cfl_inv[i][q] * f[q];
      best = fmax(best, fabs(ci));
    }
  }
  for (int off = 32; off > 0; off >>= 1) best = fmax(best, __shfl_xor(best, off));
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = best;
  __syncthreads();
  if (threadIdx.x == 0) parts[blockIdx.x] = fmax(fmax(sh[0], sh[1]), fmax(sh[2], sh[3]));
}

// nodal values of e_z x x = (-y, x) at the P2 nodes (vertices and edge midpoints of the affine
// cells; every cell sharing a node writes the same value)
__global__ __launch_bounds__(256) void k_rot_field(int nc, const double* __restrict__ vx,
                                                   const int32_t* __restrict__ p2,
                                                   double* __restrict__ out) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= nc) return;
  double x[3], y[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    x[k] = vx[(size_t)(2 * k) * nc + c];
    y[k] = vx[(size_t)(2 * k + 1) * nc + c];
  }
  const int pr[3][2] = {{1, 2}, {0, 2}, {0, 1}};
#pragma unroll
  for (int k = 0; k < 6; ++k) {
    const double xn = k < 3 ? x[k] : 0.5 * (x[pr[k - 3][0]] + x[pr[k - 3][1]]);
    const double yn = k < 3 ? y[k] : 0.5 * (y[pr[k - 3][0]] + y[pr[k - 3][1]]);
    reinterpret_cast<double2*>(out)[p2[(size_t)k * nc + c]] = make_double2(-yn, xn);
  }
}
void launch_rot_field(hipStream_t s, const MeshDev& m, double* out) {
  hipLaunchKernelGGL(k_rot_field, dim3((m.n_cells + 255) / 256), dim3(256), 0, s, m.n_cells, m.vx.p,
                     m.p2.p, out);
  NSFEM_HIP(hipGetLastError());
}

void launch_cfl(hipStream_t s, const MeshDev& m, const double* u, double scale, double* parts,
                int n_parts) {
  hipLaunchKernelGGL(k_cfl, dim3(n_parts), dim3(256), 0, s, m.n_cells, m.vx.p, m.p2.p, u, scale,
                     parts);
  NSFEM_HIP(hipGetLastError());
}

// ---- convection residual / linearised action, one thread per CELL (the 2D counterpart of
// k3_conv_cell): u (and the direction v) at the 6 nodes in registers, u_q and grad u_q formed once
// per quadrature point for all 6 test functions.
//   LIN = 0  r_(i,a) = int c(u)_a phi_i ;  LIN = 1  Newton matrix times v ;  LIN = 2  Picard matrix
//   times v.  FORM as in k_conv_jac (0 standard, 1 rotational, 2 divergence, 3 skew-symmetric).
// element vector of one cell: u (and the direction w) at the 6 nodes in registers; shared by the one-thread-per-cell
// kernel below and the lattice kernel k_jac_lattice (same arithmetic, bit for bit)
// G supplies the physical gradients of the basis, G::grad(q, k, gx, gy), and the quadrature weight times |det J|,
// G::wdet(q): from the cell's geometry (CellGrad: phys() on the spot) or from tables of a uniform lattice (TabGrad,
// filled by phys() once per cell type: the same bits)
struct CellGrad {
  const CellGeo& g;
  __device__ __forceinline__ void grad(int q, int k, double& gx, double& gy) const {
    phys(g, c_q.dphi2[q][k][0], c_q.dphi2[q][k][1], gx, gy);
  }
  __device__ __forceinline__ double wdet(int q) const { return c_q.w[q] * g.adet; }
};
// ROT (residual mode only): the explicit Coriolis vector of the IMEX step joins the element vector, gam = 2 c_cor omega:
//   r_(i,.) += wdet(q) phi_i gam (e_z x u_q),   e_z x u = (-u_y, u_x)
// weighted by the quadrature weight alone, not by cc.  phi_i phi_j has degree 4 and the rule is exact to degree 5: the
// node sums are M (gam e_z x u) to rounding.
template <int FORM, int LIN, bool ROT, class G>
__device__ __forceinline__ void conv_cell_eval_g(const G& gr, const double* ux, const double* uy,
                                                 const double* wx, const double* wy, double cc,
                                                 double* rx, double* ry, double gam = 0.0) {
  // contraction inside statements only (not across them, which depends on the surrounding kernel): the two kernels
  // that inline this function produce the same element vectors bit for bit
#pragma clang fp contract(on)
  static_assert(!ROT || LIN == 0, "the rotation term belongs to the residual mode");
#pragma unroll
  for (int i = 0; i < 6; ++i) rx[i] = ry[i] = 0.0;
  for (int q = 0; q < 7; ++q) {
    double gx[6], gy[6];
    double uqx = 0.0, uqy = 0.0, g00 = 0.0, g01 = 0.0, g10 = 0.0, g11 = 0.0;
    double vqx = 0.0, vqy = 0.0, h00 = 0.0, h01 = 0.0, h10 = 0.0, h11 = 0.0;
#pragma unroll
    for (int k = 0; k < 6; ++k) {
      gr.grad(q, k, gx[k], gy[k]);
      const double ph = c_q.phi2[q][k];
      uqx += ph * ux[k];
      uqy += ph * uy[k];
      g00 += gx[k] * ux[k];
      g01 += gy[k] * ux[k];
      g10 += gx[k] * uy[k];
      g11 += gy[k] * uy[k];
      if (LIN) {
        vqx += ph * wx[k];
        vqy += ph * wy[k];
        h00 += gx[k] * wx[k];
        h01 += gy[k] * wx[k];
        h10 += gx[k] * wy[k];
        h11 += gy[k] * wy[k];
      }
    }
    const double w = gr.wdet(q) * cc;   // (c_q.w[q] * adet) * cc
    double fx, fy;                       // coefficient of phi_i
    if (LIN == 0) {
      const double ax = g00 * uqx + g01 * uqy, ay = g10 * uqx + g11 * uqy;       // (grad u) u
      if (FORM == 1) {
        const double curl = g10 - g01;
        fx = -curl * uqy;
        fy = curl * uqx;
      } else {
        fx = ax;
        fy = ay;
        if (FORM == 2) {
          const double hd = 0.5 * (g00 + g11);
          fx += hd * uqx;
          fy += hd * uqy;
        }
      }
    } else {
      const double gvu_x = h00 * uqx + h01 * uqy, gvu_y = h10 * uqx + h11 * uqy;   // (grad v) u
      const double guv_x = g00 * vqx + g01 * vqy, guv_y = g10 * vqx + g11 * vqy;   // (grad u) v
      if (FORM == 1) {
        const double cu = g10 - g01, cv = h10 - h01;
        fx = -cu * vqy;
        fy = cu * vqx;
        if (LIN == 1) {
          fx += -cv * uqy;
          fy += cv * uqx;
        }
      } else {
        fx = gvu_x + (LIN == 1 ? guv_x : 0.0);
        fy = gvu_y + (LIN == 1 ? guv_y : 0.0);
        if (FORM == 2) {
          const double hdu = 0.5 * (g00 + g11);
          fx += hdu * vqx;
          fy += hdu * vqy;
          if (LIN == 1) {
            const double hdv = 0.5 * (h00 + h11);
            fx += hdv * uqx;
            fy += hdv * uqy;
          }
        }
      }
    }
    if (FORM == 3) { fx *= 0.5; fy *= 0.5; }
#pragma unroll
    for (int i = 0; i < 6; ++i) {
      const double wpi = w * c_q.phi2[q][i];
      rx[i] += wpi * fx;
      ry[i] += wpi * fy;
      if (FORM == 3) {
        const double ugi = uqx * gx[i] + uqy * gy[i];
        if (LIN == 0) {
          rx[i] -= 0.5 * w * ugi * uqx;
          ry[i] -= 0.5 * w * ugi * uqy;
        } else {
          const double vgi = vqx * gx[i] + vqy * gy[i];
          rx[i] -= 0.5 * w * (ugi * vqx + (LIN == 1 ? vgi * uqx : 0.0));
          ry[i] -= 0.5 * w * (ugi * vqy + (LIN == 1 ? vgi * uqy : 0.0));
        }
      }
    }
    if (ROT) {
      // (statements of their own: the contraction rule above keeps the two inlining kernels bit-equal)
      const double wr = gr.wdet(q);
      const double cx = -gam * uqy;
      const double cy = gam * uqx;
#pragma unroll
      for (int i = 0; i < 6; ++i) {
        const double rpi = wr * c_q.phi2[q][i];
        rx[i] += rpi * cx;
        ry[i] += rpi * cy;
      }
    }
  }
}
template <int FORM, int LIN, bool ROT = false>
__device__ __forceinline__ void conv_cell_eval(const CellGeo& g, const double* ux, const double* uy,
                                               const double* wx, const double* wy, double cc,
                                               double* rx, double* ry, double gam = 0.0) {
  conv_cell_eval_g<FORM, LIN, ROT>(CellGrad{g}, ux, uy, wx, wy, cc, rx, ry, gam);
}

template <int FORM, int LIN, bool ROT = false>
__global__ __launch_bounds__(256) void k_conv_cell(int nc, const double* __restrict__ vx,
                                                   const int32_t* __restrict__ p2,
                                                   const double* __restrict__ u,
                                                   const double* __restrict__ v, double cc,
                                                   const int32_t* __restrict__ ndst,
                                                   double* __restrict__ rbuf, double gam) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= nc) return;
  const CellGeo g = load_geo(vx, nc, c);
  double ux[6], uy[6], wx[LIN ? 6 : 1], wy[LIN ? 6 : 1];
#pragma unroll
  for (int k = 0; k < 6; ++k) {
    const int node = p2[(size_t)k * nc + c];
    const double2 a = reinterpret_cast<const double2*>(u)[node];
    ux[k] = a.x;
    uy[k] = a.y;
    if (LIN) {
      const double2 b = reinterpret_cast<const double2*>(v)[node];
      wx[k] = b.x;
      wy[k] = b.y;
    }
  }
  double rx[6], ry[6];
  conv_cell_eval<FORM, LIN, ROT>(g, ux, uy, wx, wy, cc, rx, ry, gam);
  // node-sorted element buffer: entry (c, i) lands inside the contiguous run of its node
  double2* out = reinterpret_cast<double2*>(rbuf);
#pragma unroll
  for (int i = 0; i < 6; ++i) out[ndst[(size_t)i * nc + c]] = make_double2(rx[i], ry[i]);
}

// b[(node, a)] += sum of the element vectors of the cells around the node: the contiguous run
// nptr[n] .. nptr[n + 1] of the node-sorted buffer, summed in ascending (cell) order
__global__ __launch_bounds__(256) void k_res_gather(int n_nodes, const int32_t* __restrict__ nptr,
                                                    const double* __restrict__ rbuf,
                                                    const uint8_t* __restrict__ skip,
                                                    double* __restrict__ b) {
  const int n = blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= n_nodes) return;
  bool sx = false, sy = false;          // flagged entries (Dirichlet / ghost rows) stay untouched
  if (skip) {
    sx = skip[2 * (size_t)n] != 0;
    sy = skip[2 * (size_t)n + 1] != 0;
    if (sx && sy) return;
  }
  const double2* __restrict__ rb = reinterpret_cast<const double2*>(rbuf);
  double2 acc = reinterpret_cast<double2*>(b)[n];
  int k = nptr[n];
  const int e = nptr[n + 1];
  for (; k + 4 <= e; k += 4) {          // four independent loads in flight per lane
    const double2 v0 = rb[k], v1 = rb[k + 1], v2 = rb[k + 2], v3 = rb[k + 3];
    acc.x += v0.x; acc.y += v0.y;
    acc.x += v1.x; acc.y += v1.y;
    acc.x += v2.x; acc.y += v2.y;
    acc.x += v3.x; acc.y += v3.y;
  }
  for (; k < e; ++k) {
    const double2 v = rb[k];
    acc.x += v.x;
    acc.y += v.y;
  }
  if (sx) acc.x = reinterpret_cast<double2*>(b)[n].x;
  if (sy) acc.y = reinterpret_cast<double2*>(b)[n].y;
  reinterpret_cast<double2*>(b)[n] = acc;
}

// vals[slot][bs] = sum over the slot's sources of ebuf[source][bs]  (fixed order)
__global__ __launch_bounds__(256) void k_gather_vals(int nnz, int bs,
                                                     const int32_t* __restrict__ cptr,
                                                     const int32_t* __restrict__ cidx,
                                                     const double* __restrict__ ebuf,
                                                     double* __restrict__ vals) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (int64_t)nnz * bs) return;
  const int s = (int)(t / bs), e = (int)(t % bs);
  double acc = 0.0;
  for (int k = cptr[s]; k < cptr[s + 1]; ++k) acc += ebuf[(size_t)cidx[k] * bs + e];
  vals[t] = acc;
}

// ------------------------------------------------------------- launch wrappers
static inline int grid_for(int64_t n) { return (int)((n + kBlock - 1) / kBlock); }

void gather_vals(hipStream_t s, const Pattern& p, int bs, const double* ebuf, double* vals) {
  NSFEM_REQUIRE(p.cptr.p && p.cidx.p, "pattern has no inverted index");
  hipLaunchKernelGGL(k_gather_vals, dim3(grid_for((int64_t)p.nnz * bs)), dim3(kBlock), 0, s,
                     p.nnz, bs, p.cptr.p, p.cidx.p, ebuf, vals);
  NSFEM_HIP(hipGetLastError());
}

void launch_assemble_p2_scalar(hipStream_t s, const MeshDev& m, const Pattern& p22, double* mass,
                               double* stiff) {
  if (m.dim == 3) return assemble_p2_scalar_3d(s, m, p22, mass, stiff);
  DevBuf<double> tmp;
  tmp.alloc((size_t)m.n_cells * 72);
  double* t0 = tmp.p;
  double* t1 = tmp.p + (size_t)m.n_cells * 36;
  hipLaunchKernelGGL(k_p2_scalar, dim3(grid_for((int64_t)m.n_cells * 6)), dim3(kBlock), 0, s,
                     m.n_cells, m.vx.p, p22.slot.p, t0, t1);
  gather_vals(s, p22, 1, t0, mass);
  gather_vals(s, p22, 1, t1, stiff);
  NSFEM_HIP(hipStreamSynchronize(s));
}
void launch_assemble_p1_scalar(hipStream_t s, const MeshDev& m, const Pattern& p11, double* stiff,
                               double* mass) {
  if (m.dim == 3) return assemble_p1_scalar_3d(s, m, p11, stiff, mass);
  DevBuf<double> tmp;
  tmp.alloc((size_t)m.n_cells * 18);
  double* t0 = tmp.p;
  double* t1 = tmp.p + (size_t)m.n_cells * 9;
  hipLaunchKernelGGL(k_p1_scalar, dim3(grid_for((int64_t)m.n_cells * 3)), dim3(kBlock), 0, s,
                     m.n_cells, m.vx.p, p11.slot.p, t0, t1);
  gather_vals(s, p11, 1, t0, stiff);
  gather_vals(s, p11, 1, t1, mass);
  NSFEM_HIP(hipStreamSynchronize(s));
}
void launch_assemble_div_grad(hipStream_t s, const MeshDev& m, const Pattern& p12,
                              const Pattern& p21, double* div, double* grad, double* divT) {
  if (m.dim == 3) return assemble_div_grad_3d(s, m, p12, p21, div, grad, divT);
  DevBuf<double> tmp;
  tmp.alloc((size_t)m.n_cells * 36 * 3);
  double* t0 = tmp.p;
  double* t1 = tmp.p + (size_t)m.n_cells * 36;
  double* t2 = tmp.p + (size_t)m.n_cells * 72;
  hipLaunchKernelGGL(k_div, dim3(grid_for((int64_t)m.n_cells * 3)), dim3(kBlock), 0, s, m.n_cells,
                     m.vx.p, p12.slot.p, t0);
  hipLaunchKernelGGL(k_grad, dim3(grid_for((int64_t)m.n_cells * 6)), dim3(kBlock), 0, s, m.n_cells,
                     m.vx.p, p21.slot.p, t1, t2);
  gather_vals(s, p12, 2, t0, div);
  gather_vals(s, p21, 2, t1, grad);
  gather_vals(s, p21, 2, t2, divT);
  NSFEM_HIP(hipStreamSynchronize(s));
}
void launch_assemble_viscous_extra(hipStream_t s, const MeshDev& m, const Pattern& p22,
                                   double* extra) {
  if (m.dim == 3) return assemble_viscous_extra_3d(s, m, p22, extra);
  DevBuf<double> tmp;
  tmp.alloc((size_t)m.n_cells * 144);
  hipLaunchKernelGGL(k_visc_extra, dim3(grid_for((int64_t)m.n_cells * 6)), dim3(kBlock), 0, s,
                     m.n_cells, m.vx.p, p22.slot.p, tmp.p);
  gather_vals(s, p22, 4, tmp.p, extra);
  NSFEM_HIP(hipStreamSynchronize(s));
}
void launch_jacobian_init(hipStream_t s, int dim, int nnz, const double* L, const double* E, double cvE,
                          double* J) {
  if (dim == 3) return jacobian_init_3d(s, nnz, L, E, cvE, J);
  int grid = grid_for(nnz);
  if (grid > 4096) grid = 4096;
  hipLaunchKernelGGL(k_jac_init, dim3(grid), dim3(kBlock), 0, s, nnz, L, E, cvE, J);
  NSFEM_HIP(hipGetLastError());
}
void launch_convection_jacobian(hipStream_t s, const MeshDev& m, const Pattern& p22,
                                const double* u, double cc, const double* L, const double* E,
                                double cvE, double* J, int form, bool picard) {
  if (m.dim == 3) return convection_jacobian_3d(s, m, p22, u, cc, L, E, cvE, J, form, picard);
  const dim3 grid(grid_for((int64_t)m.n_cells * 6)), block(kBlock);
#define NSFEM_CJ(F, P) \
  hipLaunchKernelGGL((k_conv_jac<F, P>), grid, block, 0, s, m.n_cells, m.vx.p, m.p2.p, u, cc, m.ebuf.p)
  switch (form * 2 + (picard ? 1 : 0)) {
    case 0: NSFEM_CJ(0, false); break;
    case 1: NSFEM_CJ(0, true); break;
    case 2: NSFEM_CJ(1, false); break;
    case 3: NSFEM_CJ(1, true); break;
    case 4: NSFEM_CJ(2, false); break;
    case 5: NSFEM_CJ(2, true); break;
    case 6: NSFEM_CJ(3, false); break;
    case 7: NSFEM_CJ(3, true); break;
    default: throw Error(NSFEM_ERR_ARG, "unknown convective form");
  }
#undef NSFEM_CJ
  hipLaunchKernelGGL(k_jac_gather, dim3(grid_for(p22.nnz)), dim3(kBlock), 0, s, p22.nnz,
                     p22.cptr.p, p22.cidx.p, m.ebuf.p, L, E, cvE, J);
  NSFEM_HIP(hipGetLastError());
}
template <int LIN, bool ROT = false>
static void launch_conv_cell(hipStream_t s, const MeshDev& m, const double* u, const double* v,
                             double cc, int form, double gam = 0.0) {
  const dim3 grid(grid_for(m.n_cells)), block(kBlock);
#define NSFEM_CC(F) \
  hipLaunchKernelGGL((k_conv_cell<F, LIN, ROT>), grid, block, 0, s, m.n_cells, m.vx.p, m.p2.p, u, v, cc, m.ndst.p, \
                     m.rbuf.p, gam)
  switch (form) {
    case 0: NSFEM_CC(0); break;
    case 1: NSFEM_CC(1); break;
    case 2: NSFEM_CC(2); break;
    case 3: NSFEM_CC(3); break;
    default: throw Error(NSFEM_ERR_ARG, "unknown convective form");
  }
#undef NSFEM_CC
  NSFEM_HIP(hipGetLastError());
}

void launch_convection_residual(hipStream_t s, const MeshDev& m, const double* u, double cc,
                                double* b, int form, const double* gam) {
  if (m.dim == 3) return convection_residual_3d(s, m, u, cc, b, form, gam);
  if (gam && gam[0] != 0.0) launch_conv_cell<0, true>(s, m, u, nullptr, cc, form, gam[0]);
  else launch_conv_cell<0>(s, m, u, nullptr, cc, form);
  hipLaunchKernelGGL(k_res_gather, dim3(grid_for(m.n_p2)), dim3(kBlock), 0, s, m.n_p2, m.nptr.p,
                     m.rbuf.p, (const uint8_t*)nullptr, b);
  NSFEM_HIP(hipGetLastError());
}

// y += c_c [d conv(u)/du] v (Newton) or its Picard linearisation: matrix-free action of the
// convection blocks of the velocity Jacobian
void launch_convection_action(hipStream_t s, const MeshDev& m, const double* u, const double* v,
                              double cc, double* y, int form, bool picard, const uint8_t* skipmask) {
  if (m.dim == 3) return convection_action_3d(s, m, u, v, cc, y, form, picard, skipmask);
  if (picard) launch_conv_cell<2>(s, m, u, v, cc, form);
  else launch_conv_cell<1>(s, m, u, v, cc, form);
  hipLaunchKernelGGL(k_res_gather, dim3(grid_for(m.n_p2)), dim3(kBlock), 0, s, m.n_p2, m.nptr.p,
                     m.rbuf.p, skipmask, y);
  NSFEM_HIP(hipGetLastError());
}

void launch_convection_cells(hipStream_t s, const MeshDev& m, const double* u, const double* v, double cc,
                             int form, bool picard) {
  NSFEM_REQUIRE(m.dim == 2, "launch_convection_cells: triangles only");
  if (picard) launch_conv_cell<2>(s, m, u, v, cc, form);
  else launch_conv_cell<1>(s, m, u, v, cc, form);
}

// ---------------------------------------------------------------- scalar transport (nsfem_step_scalar_imex)
// Convection of a P2 scalar T by the P2 velocity u, one thread per CELL: u and T at the 6 nodes in registers, u_q and
// grad T_q formed once per quadrature point and shared by the 6 test functions.
//   FORM 0 (standard)        r_i = wgt int (u . grad T) phi_i
//   FORM 1 (skew-symmetric)  r_i = wgt/2 int [ (u . grad T) phi_i - (u . grad phi_i) T ]      (= 1/2 (C - C^T) T)
// The element vector goes node-sorted into the first 6 n_cells doubles of m.rbuf (ndst, as k_conv_cell);
// k_scalar_gather sums the run of every node in ascending cell order: no atomics, the same state gives the same bytes.
// PENAL 1 (sharp masks) / 2 (smoothed): heated bodies (nsfem_set_body_temperatures) -- the same launch adds
//   wgt/eta_T sum_q w_q |det J| chi(x_q) theta_win (T(x_q) - T_win) phi_i(x_q)
// x_q the affine image of the reference point, chi and the winner from body_winner (bodies.hpp) as in k_penal_cell;
// x_q, the winner, chi and T_q are formed once per quadrature point, points with chi = 0 or a passive winner add
// nothing.  PENAL 0 takes no table at all and is the code of every run without temperatures.
// SGS 1, 4, 5 (the subgrid law: Smagorinsky, WALE, Vreman): subgrid heat flux (nsfem_set_scalar_sgs) -- the same
// launch adds
//   wgt sum_q w_q |det J| kappa_x grad T_q . grad phi_i(x_q),   kappa_x = nu_x / Pr_t   (SGS 1: (C_s Delta_K)^2 gamma / Pr_t)
// with g_ab = d_b u_a summed from the gradients the point forms anyway, gamma and Delta_K^2 = |det J| / 2 as in
// k_visc_var_cell and the law of cell_geometry.hpp (visc_law_nu<1> of gamma, visc_law_nu_grad<4 | 5, 2> of g).  SGS 0
// takes nothing and is the code of every run without the setting.
// SGS 8 (dynamic diffusivity, nsfem_set_scalar_sgs_dynamic): kappa_x = (c_K Delta_K^2) gamma, the arithmetic of SGS 1
// with c_K -- the mean of the vertex field C_theta over the cell's vertices, dynamic_cell_constant -- in the place of
// C_s^2 and no 1 / Pr_t; c_K Delta_K^2 is formed once before the quadrature loop.
template <int FORM, int PENAL, int SGS = 0>
__global__ __launch_bounds__(256) void k_scalar_conv_cell(int nc, const double* __restrict__ vx,
                                                          const int32_t* __restrict__ p2,
                                                          const double* __restrict__ u,
                                                          const double* __restrict__ T, double wgt,
                                                          const ScalarPenalArgs<PENAL> pa,
                                                          const ScalarSgsKernelArgs<SGS> sg,
                                                          const int32_t* __restrict__ ndst,
                                                          double* __restrict__ rbuf) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= nc) return;
  const CellGeo g = load_geo(vx, nc, c);
  double ux[6], uy[6], t[6];
#pragma unroll
  for (int k = 0; k < 6; ++k) {
    const int node = p2[(size_t)k * nc + c];
    const double2 a = reinterpret_cast<const double2*>(u)[node];
    ux[k] = a.x;
    uy[k] = a.y;
    t[k] = T[node];
  }
  // (reach: can the support of any body touch the cell?  body_misses_cell, bodies.hpp -- most cells skip the winner)
  double xv[3][2];
  bool reach = false;
  if constexpr (PENAL != 0) {
#pragma unroll
    for (int v = 0; v < 3; ++v) {
      xv[v][0] = vx[(size_t)(2 * v) * nc + c];
      xv[v][1] = vx[(size_t)(2 * v + 1) * nc + c];
    }
    for (int s = 0; s < pa.bt.n; ++s) reach = reach || !body_misses_cell<2>(pa.bt, s, xv);
  }
  double ckd2 = 0.0;                     // c_K Delta_K^2 (SGS 8)
  if constexpr (SGS == 8) ckd2 = dynamic_cell_constant<2>(sg.vtx, sg.cthv, nc, c) * (0.5 * g.adet);
  double r[6];
#pragma unroll
  for (int i = 0; i < 6; ++i) r[i] = 0.0;
  for (int q = 0; q < 7; ++q) {
    double gx[6], gy[6];
    double uqx = 0.0, uqy = 0.0, tq = 0.0, dtx = 0.0, dty = 0.0;
    double g00 = 0.0, g01 = 0.0, g10 = 0.0, g11 = 0.0;     // g_ab = d_b u_a (SGS)
#pragma unroll
    for (int k = 0; k < 6; ++k) {
      phys(g, c_q.dphi2[q][k][0], c_q.dphi2[q][k][1], gx[k], gy[k]);
      const double ph = c_q.phi2[q][k];
      uqx += ph * ux[k];
      uqy += ph * uy[k];
      dtx += gx[k] * t[k];
      dty += gy[k] * t[k];
      if (FORM == 1 || PENAL != 0) tq += ph * t[k];
      if constexpr (SGS != 0) {
        g00 += gx[k] * ux[k];
        g01 += gy[k] * ux[k];
        g10 += gx[k] * uy[k];
        g11 += gy[k] * uy[k];
      }
    }
    const double w = c_q.w[q] * g.adet * wgt;
    const double adv = uqx * dtx + uqy * dty;           // u . grad T
#pragma unroll
    for (int i = 0; i < 6; ++i) {
      if (FORM == 0) {
        r[i] += w * c_q.phi2[q][i] * adv;
      } else {
        const double ugi = uqx * gx[i] + uqy * gy[i];   // u . grad phi_i
        r[i] += 0.5 * w * (c_q.phi2[q][i] * adv - ugi * tq);
      }
    }
    if constexpr (SGS != 0) {
      const double s00 = 2.0 * g00, s01 = g01 + g10, s11 = 2.0 * g11;      // g + g^T
      double wk;
      if constexpr (SGS == 8) {
        // (the sum under the root written out as the fused sequence the SGS = 1 instantiations compile to with the
        // present compiler -- left to itself the compiler contracts it in another order in this instantiation and the
        // last bit of gamma differs.  With every group at the clip this instantiation then gives the bytes of SGS = 1
        // with C_s^2 = ctheta_max, Pr_t = 1, which tests/test_gpu_dynamic_scalar.py pins; a compiler that contracts
        // the expression of the other branch differently needs this line written to match)
        const double gamma = sqrt(0.5 * fma(s11, s11, fma(2.0, s01 * s01, s00 * s00)));
        wk = w * (ckd2 * gamma);
      } else {
        const double gamma = sqrt(0.5 * (s00 * s00 + 2.0 * (s01 * s01) + s11 * s11));
        double nux;
        if constexpr (SGS == 1) {
          nux = visc_law_nu<1>(gamma, 0.5 * g.adet, sg.c0, 0.0, 0.0);
        } else {
          const double G[2][2] = {{g00, g01}, {g10, g11}};
          nux = visc_law_nu_grad<SGS, 2>(G, 0.5 * g.adet, sg.c0);
        }
        wk = w * (nux * sg.inv_prt);
      }
#pragma unroll
      for (int i = 0; i < 6; ++i) r[i] += wk * (dtx * gx[i] + dty * gy[i]);
    }
    if constexpr (PENAL != 0) {
      if (!reach) continue;
      double x[2];
#pragma unroll
      for (int a = 0; a < 2; ++a)
        x[a] = c_q.phi1[q][0] * xv[0][a] + c_q.phi1[q][1] * xv[1][a] + c_q.phi1[q][2] * xv[2][a];
      int win;
      const double chi = body_winner<2, PENAL == 2>(pa.bt, x, win);
      if (!(chi > 0.0) || pa.th.flag[win] == 0) continue;
      const double h = w * pa.th.inv_eta * chi * (tq - pa.th.temperature[win]);
#pragma unroll
      for (int i = 0; i < 6; ++i) r[i] += h * c_q.phi2[q][i];
    }
  }
#pragma unroll
  for (int i = 0; i < 6; ++i) rbuf[ndst[(size_t)i * nc + c]] = r[i];
}

// out[n] = sum of the node's run nptr[n] .. nptr[n + 1] of the node-sorted scalar element vectors (ascending cells)
__global__ __launch_bounds__(256) void k_scalar_gather(int n_nodes, const int32_t* __restrict__ nptr,
                                                       const double* __restrict__ rbuf, double* __restrict__ out) {
  const int n = blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= n_nodes) return;
  double acc = 0.0;
  int k = nptr[n];
  const int e = nptr[n + 1];
  for (; k + 4 <= e; k += 4) {          // four independent loads in flight per lane
    const double v0 = rbuf[k], v1 = rbuf[k + 1], v2 = rbuf[k + 2], v3 = rbuf[k + 3];
    acc += v0;
    acc += v1;
    acc += v2;
    acc += v3;
  }
  for (; k < e; ++k) acc += rbuf[k];
  out[n] = acc;
}

// f_eff[n dim + c] = f[n dim + c] + T[n] b[c]   (f null: no body force set, f_eff = T b)
__global__ __launch_bounds__(256) void k_buoyancy_force(int64_t n_nodes, int dim, const double* __restrict__ f,
                                                        const double* __restrict__ T, double b0, double b1, double b2,
                                                        double* __restrict__ out) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n_nodes * dim) return;
  const int c = (int)(t % dim);
  const double b = c == 0 ? b0 : (c == 1 ? b1 : b2);
  const double tb = T[t / dim] * b;
  out[t] = f ? f[t] + tb : tb;
}

void launch_scalar_convection(hipStream_t s, const MeshDev& m, const double* u, const double* T, double weight,
                              int form, const ScalarBodies* hb, double* out, ScalarSgsArgs sgs) {
  NSFEM_REQUIRE(form == 0 || form == 1, "scalar convection: form must be 0 (standard) or 1 (skew-symmetric)");
  NSFEM_REQUIRE(!hb || (hb->bt.n > 0 && hb->th.n == hb->bt.n), "heated bodies: no temperatures set for the bodies");
  const int penal = !hb ? 0 : (hb->bt.eps > 0.0 ? 2 : 1);
  NSFEM_REQUIRE((sgs.law == 8) == (sgs.cthv != nullptr),
                "scalar convection: the vertex constants go with the dynamic diffusivity and only with it");
  if (m.dim == 3) {
    scalar_convection_cells_3d(s, m, u, T, weight, form, penal, hb, sgs);
  } else {
    const dim3 grid(grid_for(m.n_cells)), block(kBlock);
    with_scalar_kernel(form, penal, sgs.law, [&](auto fc, auto pc, auto lc) {
      constexpr int F = decltype(fc)::value, P = decltype(pc)::value, L = decltype(lc)::value;
      hipLaunchKernelGGL((k_scalar_conv_cell<F, P, L>), grid, block, 0, s, m.n_cells, m.vx.p, m.p2.p, u, T, weight,
                         scalar_penal_args<P>(hb), scalar_sgs_kernel_args<L>(sgs, m.p1.p), m.ndst.p, m.rbuf.p);
    });
  }
  hipLaunchKernelGGL(k_scalar_gather, dim3(grid_for(m.n_p2)), dim3(kBlock), 0, s, m.n_p2, m.nptr.p, m.rbuf.p, out);
  NSFEM_HIP(hipGetLastError());
}

void launch_buoyancy_force(hipStream_t s, const MeshDev& m, const double* f, const double* T, const double b[3],
                           double* out) {
  const int64_t n = (int64_t)m.n_p2 * m.dim;
  hipLaunchKernelGGL(k_buoyancy_force, dim3(grid_for(n)), dim3(kBlock), 0, s, (int64_t)m.n_p2, m.dim, f, T, b[0], b[1],
                     m.dim == 3 ? b[2] : 0.0, out);
  NSFEM_HIP(hipGetLastError());
}

// ---------------------------------------------------------------- variable viscosity (nsfem_set_viscosity_law)
// Explicit remainder of a strain-rate dependent viscosity, one thread per CELL, 7-point rule (part of the definition:
// the integrand is no polynomial):
//   r_(i,a) = wgt sum_q w_q |det J| nu_x(gamma_q, Delta_K) sum_b (g_ab + g_ba)_q d_b phi_i,   g_ab = d_b u_a,
//   gamma = sqrt(1/2 sum_ab (g_ab + g_ba)^2),   Delta_K^2 = |det J| / 2
// LAW 1, 2: nu_x of gamma (visc_law_nu); LAW 4, 5 (WALE, Vreman): nu_x of the tensor g itself (visc_law_nu_grad<LAW, 2>:
// the 2D field as the z-independent 3D one), cell_geometry.hpp.  LAW 8 (dynamic Smagorinsky): the arithmetic of law 1
// with c_K, the mean of the vertex field cs2v over the cell's vertices (through p1), in the place of C_s^2; the other
// instantiations never touch vtx (the P1 connectivity) / cs2v.
// u at the 6 nodes in registers; the physical gradients, g, gamma and nu_x of a quadrature point are formed once and
// shared by the 6 test functions.  The element vector goes node-sorted into m.rbuf (ndst, as k_conv_cell); k_visc_gather
// sums the run of every node in ascending cell order: no atomics, the same state gives the same bytes.
// MEAN: no element vector; rbuf[c] = sum_q w_q nu_x(gamma_q) / sum_q w_q, the cell mean of nu_x (output).
template <int LAW, bool MEAN>
__global__ __launch_bounds__(256) void k_visc_var_cell(int nc, const double* __restrict__ vx,
                                                       const int32_t* __restrict__ p2,
                                                       const double* __restrict__ u, double wgt, double p0, double p1,
                                                       double pp2, const int32_t* __restrict__ ndst,
                                                       double* __restrict__ rbuf, const int32_t* __restrict__ vtx,
                                                       const double* __restrict__ cs2v) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= nc) return;
  const CellGeo g = load_geo(vx, nc, c);
  const double delta2 = 0.5 * g.adet;
  if constexpr (LAW == 8) p0 = dynamic_cell_constant<2>(vtx, cs2v, nc, c);      // c_K in the place of C_s
  double ux[6], uy[6];
#pragma unroll
  for (int k = 0; k < 6; ++k) {
    const int node = p2[(size_t)k * nc + c];
    const double2 a = reinterpret_cast<const double2*>(u)[node];
    ux[k] = a.x;
    uy[k] = a.y;
  }
  double rx[6], ry[6];
#pragma unroll
  for (int i = 0; i < 6; ++i) rx[i] = ry[i] = 0.0;
  double mean = 0.0, wsum = 0.0;
  for (int q = 0; q < 7; ++q) {
    double gx[6], gy[6];
    double g00 = 0.0, g01 = 0.0, g10 = 0.0, g11 = 0.0;     // g_ab = d_b u_a
#pragma unroll
    for (int k = 0; k < 6; ++k) {
      phys(g, c_q.dphi2[q][k][0], c_q.dphi2[q][k][1], gx[k], gy[k]);
      g00 += gx[k] * ux[k];
      g01 += gy[k] * ux[k];
      g10 += gx[k] * uy[k];
      g11 += gy[k] * uy[k];
    }
    const double s00 = 2.0 * g00, s01 = g01 + g10, s11 = 2.0 * g11;      // g + g^T
    const double gamma = sqrt(0.5 * (s00 * s00 + 2.0 * (s01 * s01) + s11 * s11));
    double nu;
    if constexpr (LAW == 4 || LAW == 5) {
      const double G[2][2] = {{g00, g01}, {g10, g11}};
      nu = visc_law_nu_grad<LAW, 2>(G, delta2, p0);
    } else {
      nu = visc_law_nu<LAW>(gamma, delta2, p0, p1, pp2);
    }
    if (MEAN) {
      mean += c_q.w[q] * nu;
      wsum += c_q.w[q];
    } else {
      const double w = c_q.w[q] * g.adet * wgt * nu;
#pragma unroll
      for (int i = 0; i < 6; ++i) {
        rx[i] += w * (s00 * gx[i] + s01 * gy[i]);
        ry[i] += w * (s01 * gx[i] + s11 * gy[i]);
      }
    }
  }
  if (MEAN) {
    rbuf[c] = mean / wsum;
  } else {
    double2* out = reinterpret_cast<double2*>(rbuf);
#pragma unroll
    for (int i = 0; i < 6; ++i) out[ndst[(size_t)i * nc + c]] = make_double2(rx[i], ry[i]);
  }
}

// v = sum of the run nptr[n] .. nptr[n + 1] of the node-sorted element vectors (dim components per entry, ascending
// cell order, as k_res_gather), one thread per (node, component); in the same launch  n1 += v  and  rhs -= b0 v
// (rhs null: the plain sum, nsfem_viscosity_residual and the stored vector of the old level)
__global__ __launch_bounds__(256) void k_visc_gather(int64_t n_entries, int dim, const int32_t* __restrict__ nptr,
                                                     const double* __restrict__ rbuf, double b0,
                                                     double* __restrict__ n1, double* __restrict__ rhs) {
#pragma clang fp contract(off)
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n_entries) return;
  const int n = (int)(t / dim), a = (int)(t % dim);
  double v = 0.0;
  int k = nptr[n];
  const int e = nptr[n + 1];
  for (; k + 4 <= e; k += 4) {          // four independent loads in flight per lane
    const double v0 = rbuf[(size_t)k * dim + a], v1 = rbuf[(size_t)(k + 1) * dim + a];
    const double v2 = rbuf[(size_t)(k + 2) * dim + a], v3 = rbuf[(size_t)(k + 3) * dim + a];
    v += v0;
    v += v1;
    v += v2;
    v += v3;
  }
  for (; k < e; ++k) v += rbuf[(size_t)k * dim + a];
  n1[t] += v;
  if (rhs) rhs[t] -= b0 * v;
}

void launch_viscosity_cells(hipStream_t s, const MeshDev& m, const double* u, double weight, int law,
                            const double p[4], bool mean, const double* cs2v) {
  NSFEM_REQUIRE(law != 0 && is_viscosity_law(law), "variable viscosity: no law set");
  NSFEM_REQUIRE((law == 8) == (cs2v != nullptr), "variable viscosity: the vertex constants go with law 8 and only with it");
  if (m.dim == 3) return viscosity_cells_3d(s, m, u, weight, law, p, mean, cs2v);
  with_variable_law(law, mean, [&](auto lc, auto mc) {
    hipLaunchKernelGGL((k_visc_var_cell<decltype(lc)::value, decltype(mc)::value != 0>), dim3(grid_for(m.n_cells)),
                       dim3(kBlock), 0, s, m.n_cells, m.vx.p, m.p2.p, u, weight, p[0], p[1], p[2], m.ndst.p, m.rbuf.p,
                       m.p1.p, cs2v);
  });
  NSFEM_HIP(hipGetLastError());
}

// ---------------------------------------------------------------- the Germano-Lilly procedure: C_s^2 (law 8) and C_theta
// Three launches on a velocity level u, or on a level pair (u, T) for the dynamic subgrid heat flux kappa_x = c_K
// Delta_K^2 gamma (nsfem_set_scalar_sgs_dynamic) -- launch_dynamic_constant; plain stores, no atomics, the same state
// gives the same bytes:
//   k_dyn_moments<DIM>         one thread per CELL: m_K[f] = |K| sum_q w_q f(x_q) / sum_q w_q by the degree-5 rule for
//   k_dyn_scalar_moments<DIM>  u:       f = u_a | u_a u_b | S_ab | gamma S_ab (a <= b; NS = DIM (DIM + 1) / 2 pairs)
//                              (u, T):  f = T | T u_a | u_a | d_a T | gamma d_a T | S_ab
//                              the gamma rows scaled by Delta_K^2 at the store, then |K| and |K| Delta_K^2: SoA
//                              [dynamic_moment_rows][n_cells].  G_ab = d_b u_a and grad T are formed from the
//                              differences u_k - u_0, T_k - T_0 (the basis gradients sum to zero): a constant field
//                              has G = 0 exactly, not a rounding residue.  The set on (u, T) repeats u_a, S_ab and
//                              the volumes of the set on u on purpose: the buffer of law 8 may hold another level when
//                              the scalar step runs.
//   k_dyn_vertex<DIM>          one thread per VERTEX: the patch sums of the moments through the vertex-to-cell CSR in
//   k_dyn_scalar_vertex<DIM>   ascending cell order (patch_mean), the test-filtered fields, the Germano identity;
//                              writes W_v, LM_v, MM_v, on (u, T) W_v, PR_v = P . R, RR_v = R . R with P_a = hat(T u_a)
//                              - hat T hat u_a, R_a = hat(Delta^2 gamma d_a T) - alpha^2 Delta_v^2 hat gamma hat(d_a T)
//                              ([n_p1][3])
//   k_dyn_reduce               one workgroup per averaging GROUP over the group-sorted vertex list (the scheme of
//                              k_wall_reduce): num_g, den_g, the clipped constant ([n_groups][3]) and the constant at
//                              the vertices of the group
// Register layout of the moment kernels as k_visc_var_cell: the fields at the cell nodes in registers, the physical
// gradients of a quadrature point formed once.
//
// DynFront: what both moment kernels of triangles need of a cell and of a quadrature point -- the nodal values, u_q
// (and T_q), 2 S and gamma (and grad T), the weight sum; WITH_T = false carries nothing of T.  (Tetrahedra: DynFront3,
// assembly3d.hip -- another geometry type and another grouping of the sum under gamma.)
template <bool WITH_T>
struct DynFront {
  CellGeo g;
  double vol, delta2;                        // |K| and Delta_K^2 = |K|^(2 / dim)
  double ux[6], uy[6], t[WITH_T ? 6 : 1];
  double wsum = 0.0;
  double w, uqx, uqy, tq, dtx, dty, S[3], gamma;          // of the point: w_q, u, T, grad T, S (00 01 11), gamma
  __device__ __forceinline__ DynFront(const double* __restrict__ vx, int nc, int c, const int32_t* __restrict__ p2,
                                      const double* __restrict__ u, const double* __restrict__ T)
      : g(load_geo(vx, nc, c)) {
    vol = delta2 = 0.5 * g.adet;
#pragma unroll
    for (int k = 0; k < 6; ++k) {
      const int node = p2[(size_t)k * nc + c];
      const double2 a = reinterpret_cast<const double2*>(u)[node];
      ux[k] = a.x;
      uy[k] = a.y;
      if constexpr (WITH_T) t[k] = T[node];
    }
  }
  __device__ __forceinline__ void point(int q) {
    uqx = uqy = tq = 0.0;
#pragma unroll
    for (int k = 0; k < 6; ++k) {
      uqx += c_q.phi2[q][k] * ux[k];
      uqy += c_q.phi2[q][k] * uy[k];
      if constexpr (WITH_T) tq += c_q.phi2[q][k] * t[k];
    }
    double g00 = 0.0, g01 = 0.0, g10 = 0.0, g11 = 0.0;     // g_ab = d_b u_a
    dtx = dty = 0.0;
#pragma unroll
    for (int k = 1; k < 6; ++k) {
      double gx, gy;
      phys(g, c_q.dphi2[q][k][0], c_q.dphi2[q][k][1], gx, gy);
      const double dx = ux[k] - ux[0], dy = uy[k] - uy[0];
      g00 += gx * dx;
      g01 += gy * dx;
      g10 += gx * dy;
      g11 += gy * dy;
      if constexpr (WITH_T) {
        const double dt = t[k] - t[0];
        dtx += gx * dt;
        dty += gy * dt;
      }
    }
    const double s00 = 2.0 * g00, s01 = g01 + g10, s11 = 2.0 * g11;      // g + g^T = 2 S
    // gamma^2 = (s00^2 + 2 s01^2 + s11^2) / 2.  Written once per kernel, the first sum was contracted differently in
    // the two: the product s00^2 fused on u, the product 2 s01^2 fused on (u, T).  Each keeps its rounding, written out
    const double s01s = s01 * s01;
    const double in = WITH_T ? fma(2.0, s01s, s00 * s00) : fma(s00, s00, 2.0 * s01s);
    gamma = sqrt(0.5 * fma(s11, s11, in));
    S[0] = 0.5 * s00;
    S[1] = 0.5 * s01;
    S[2] = 0.5 * s11;
    w = c_q.w[q];
    wsum += w;
  }
  __device__ __forceinline__ double scale() const { return vol / wsum; }
};

template <int DIM>
__global__ void k_dyn_moments(int nc, const double* __restrict__ vx, const int32_t* __restrict__ p2,
                              const double* __restrict__ u, double* __restrict__ mom);     // <3>: assembly3d.hip

template <>
__global__ __launch_bounds__(256) void k_dyn_moments<2>(int nc, const double* __restrict__ vx,
                                                        const int32_t* __restrict__ p2,
                                                        const double* __restrict__ u, double* __restrict__ mom) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= nc) return;
  DynFront<false> p(vx, nc, c, p2, u, nullptr);
  double mu[2] = {0.0, 0.0}, muu[3] = {0.0, 0.0, 0.0}, ms[3] = {0.0, 0.0, 0.0}, mg[3] = {0.0, 0.0, 0.0};
  for (int q = 0; q < 7; ++q) {
    p.point(q);
    mu[0] += p.w * p.uqx;
    mu[1] += p.w * p.uqy;
    muu[0] += p.w * (p.uqx * p.uqx);
    muu[1] += p.w * (p.uqx * p.uqy);
    muu[2] += p.w * (p.uqy * p.uqy);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      ms[k] += p.w * p.S[k];
      mg[k] += p.w * (p.gamma * p.S[k]);
    }
  }
  const double f = p.scale();
  double* o = mom + c;
  o[0] = f * mu[0];
  o[(size_t)nc] = f * mu[1];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    o[(size_t)(2 + k) * nc] = f * muu[k];
    o[(size_t)(5 + k) * nc] = f * ms[k];
    o[(size_t)(8 + k) * nc] = (f * p.delta2) * mg[k];
  }
  o[(size_t)11 * nc] = p.vol;
  o[(size_t)12 * nc] = p.vol * p.delta2;
}

// The patch of a vertex v: a[i] = the sum of row i of mom over the cells of v in ascending order (the vertex-to-cell
// CSR), then divided by W = a[NM - 2], the patch volume -- the test-filtered fields.  false: a vertex of no cell, no
// patch (a is not divided; the caller writes no contribution).  No contraction, as in the kernels that call it (their
// pragma does not reach in here).
template <int NM>
__device__ __forceinline__ bool patch_mean(int v, int nc, const int32_t* __restrict__ vptr,
                                           const int32_t* __restrict__ vcell, const double* __restrict__ mom,
                                           double (&a)[NM], double& W) {
#pragma clang fp contract(off)
#pragma unroll
  for (int i = 0; i < NM; ++i) a[i] = 0.0;
  const int e = vptr[v + 1];
  for (int k = vptr[v]; k < e; ++k) {
    const double* m = mom + vcell[k];
#pragma unroll
    for (int i = 0; i < NM; ++i) a[i] += m[(size_t)i * nc];
  }
  W = a[NM - 2];
  if (!(W > 0.0)) return false;
#pragma unroll
  for (int i = 0; i < NM; ++i) a[i] /= W;
  return true;
}

// the filtered shear rate hat gamma = sqrt(2 hat S : hat S) from the NS rows s of hat S (pairs a <= b in row order:
// the contraction counts the off-diagonal pairs twice)
template <int DIM>
__device__ __forceinline__ double patch_shear_rate(const double* s) {
#pragma clang fp contract(off)
  double ss = 0.0;
  int i = 0;
#pragma unroll
  for (int r = 0; r < DIM; ++r)
#pragma unroll
    for (int c = r; c < DIM; ++c, ++i) ss += (r == c ? 1.0 : 2.0) * (s[i] * s[i]);
  return sqrt(2.0 * ss);
}

// vert[v] = {W_v, LM_v, MM_v}.  Pairs (a <= b) in row order: 00 01 11 | 00 01 02 11 12 22; full contractions count the
// off-diagonal pairs twice.  alpha2 = alpha^2, the squared ratio of the test filter width to the grid filter width.
template <int DIM>
__global__ __launch_bounds__(256) void k_dyn_vertex(int nv, int nc, const int32_t* __restrict__ vptr,
                                                    const int32_t* __restrict__ vcell,
                                                    const double* __restrict__ mom, double alpha2,
                                                    double* __restrict__ vert) {
#pragma clang fp contract(off)
  constexpr int NS = DIM * (DIM + 1) / 2, NM = dynamic_moment_rows(DIM, false);
  const int v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= nv) return;
  double a[NM], W;
  double* o = vert + (size_t)v * 3;
  if (!patch_mean(v, nc, vptr, vcell, mom, a, W)) {      // (a vertex of no cell: no contribution)
    o[0] = o[1] = o[2] = 0.0;
    return;
  }
  // the test-filtered fields: hat u = a[0 ..), hat(u u) = a[UU ..), hat S = a[SS ..), hat(Delta^2 gamma S) = a[GS ..)
  constexpr int UU = DIM, SS = DIM + NS, GS = DIM + 2 * NS;
  const double d2 = a[NM - 1];
  double trl = 0.0;
  double L[NS];
  {
    int i = 0;
#pragma unroll
    for (int r = 0; r < DIM; ++r)
#pragma unroll
      for (int c = r; c < DIM; ++c, ++i) {
        L[i] = a[UU + i] - a[r] * a[c];
        if (r == c) trl += L[i];
      }
  }
  const double coef = (alpha2 * d2) * patch_shear_rate<DIM>(a + SS), tr = trl / (double)DIM;
  double lm = 0.0, mm = 0.0;
  {
    int i = 0;
#pragma unroll
    for (int r = 0; r < DIM; ++r)
#pragma unroll
      for (int c = r; c < DIM; ++c, ++i) {
        const double M = 2.0 * (a[GS + i] - coef * a[SS + i]);
        const double ld = r == c ? L[i] - tr : L[i];
        const double mult = r == c ? 1.0 : 2.0;
        lm += mult * (ld * M);
        mm += mult * (M * M);
      }
  }
  o[0] = W;
  o[1] = lm;
  o[2] = mm;
}

// sums[g] = {num_g, den_g, cs2_g}, num_g = sum W_v LM_v, den_g = sum W_v MM_v over gvert[goff[g] .. goff[g + 1]): thread t
// adds the entries t, t + 256, ... in ascending order from +0.0, the partials are folded by the xor-shuffle tree within
// each wave and the four wave sums added in wave order through LDS (k_wall_reduce).  cs2_g = min(max(num / den, 0),
// cs2_max) where den > 0, else 0 (an empty group, a field at rest); every vertex of the group receives it.
__global__ __launch_bounds__(256) void k_dyn_reduce(const int32_t* __restrict__ goff, const int32_t* __restrict__ gvert,
                                                    const double* __restrict__ vert, double cs2_max,
                                                    double* __restrict__ sums, double* __restrict__ cs2v) {
#pragma clang fp contract(off)
  __shared__ double sh[4][2];
  __shared__ double result;
  const int g = blockIdx.x, t = threadIdx.x;
  const int begin = goff[g], end = goff[g + 1];
  double num = 0.0, den = 0.0;
  for (int i = begin + t; i < end; i += 256) {
    const double* r = vert + (size_t)gvert[i] * 3;
    num += r[0] * r[1];
    den += r[0] * r[2];
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    num += __shfl_xor(num, off, 64);
    den += __shfl_xor(den, off, 64);
  }
  if ((t & 63) == 0) {
    sh[t >> 6][0] = num;
    sh[t >> 6][1] = den;
  }
  __syncthreads();
  if (t == 0) {
    const double n = ((sh[0][0] + sh[1][0]) + sh[2][0]) + sh[3][0];
    const double d = ((sh[0][1] + sh[1][1]) + sh[2][1]) + sh[3][1];
    const double cs2 = d > 0.0 ? fmin(fmax(n / d, 0.0), cs2_max) : 0.0;
    sums[(size_t)g * 3] = n;
    sums[(size_t)g * 3 + 1] = d;
    sums[(size_t)g * 3 + 2] = cs2;
    result = cs2;
  }
  __syncthreads();
  const double cs2 = result;
  for (int i = begin + t; i < end; i += 256) cs2v[gvert[i]] = cs2;
}

// Lagrangian averaging (nsfem_set_dynamic_averaging mode 1; Meneveau, Lund & Cabot 1996) in the place of k_dyn_reduce:
// one thread per VERTEX, plain stores, no atomics, no LDS.  The definition is that of include/nsfem.h, rule by rule:
//   1. d = -k u_v, u_v at the P2 node of v in the first cell of its patch
//   2. per patch cell (ascending) the barycentric coordinates of x_v + d RELATIVE to v -- lambda_j = grad(lambda_j) . d
//      for j != i, lambda_i = 1 - their sum --, m_c their minimum; c* the first cell of the largest m_c; m_c* < 0: the
//      point left the patch, the coordinates are clamped at 0 and divided by their sum
//   3. I_up = sum_j lambda_j I[p1[c*][j]]
//   4. eps = k / (k + T), T = theta Delta_v / (I_LM_up I_MM_up)^(1/8) where the product is > 0, else eps = 1;
//      I_MM' = eps MM_v + (1 - eps) I_MM_up, I_LM' = max(eps LM_v + (1 - eps) I_LM_up, cs2_floor I_MM')
//   5. cs2_v = min(max(I_LM' / I_MM', 0), cs2_max) where I_MM' > 0, else 0
//   6. Iold null (no state yet): I_MM = MM_v, I_LM = cs2_init MM_v, cs2_v by 5; the upstream pair is that state
// Iold and Inew [n_p1][2] = I_LM, I_MM are two buffers: neighbours' old values are read.  mom2: the last two moment
// rows (|K|, |K| Delta_K^2), [2][n_cells].  up [n_p1][2] may be null.  A vertex of no cell: zeros.  The local index of
// v in a cell is found by comparison and every array is indexed with compile-time constants (no scratch).
template <int DIM>
struct LagrangeGeo;
template <>
struct LagrangeGeo<2> {
  // grad[j][a] = d lambda_j / d x_a: lambda_1 = xi_0, lambda_2 = xi_1, lambda_0 = 1 - xi_0 - xi_1
  static __device__ __forceinline__ void gradients(const double* __restrict__ vx, int nc, int c, double (&g)[3][2]) {
#pragma clang fp contract(off)
    const CellGeo geo = load_geo(vx, nc, c);
    g[1][0] = geo.ji00;
    g[1][1] = geo.ji01;
    g[2][0] = geo.ji10;
    g[2][1] = geo.ji11;
    g[0][0] = -(geo.ji00 + geo.ji10);
    g[0][1] = -(geo.ji01 + geo.ji11);
  }
};
template <>
struct LagrangeGeo<3> {
  static __device__ __forceinline__ void gradients(const double* __restrict__ vx, int nc, int c, double (&g)[4][3]) {
#pragma clang fp contract(off)
    const CellGeo3 geo = load_geo3(vx, nc, c);
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      g[1][a] = geo.ji[0][a];
      g[2][a] = geo.ji[1][a];
      g[3][a] = geo.ji[2][a];
      g[0][a] = -((geo.ji[0][a] + geo.ji[1][a]) + geo.ji[2][a]);
    }
  }
};

template <int DIM>
__global__ __launch_bounds__(256) void k_dyn_lagrange(int nv, int nc, const int32_t* __restrict__ vptr,
                                                      const int32_t* __restrict__ vcell,
                                                      const int32_t* __restrict__ p1, const int32_t* __restrict__ p2,
                                                      const double* __restrict__ vx, const double* __restrict__ u,
                                                      const double* __restrict__ mom2, const double* __restrict__ vert,
                                                      const double* __restrict__ Iold, double k, double theta,
                                                      double cs2_init, double cs2_floor, double cs2_max,
                                                      double* __restrict__ Inew, double* __restrict__ cs2v,
                                                      double* __restrict__ up) {
#pragma clang fp contract(off)
  constexpr int NL = DIM + 1;
  const int v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= nv) return;
  const int begin = vptr[v], end = vptr[v + 1];
  double W = 0.0, D = 0.0;
  for (int e = begin; e < end; ++e) {
    const int c = vcell[e];
    W += mom2[c];
    D += mom2[(size_t)nc + c];
  }
  double ilm = 0.0, imm = 0.0, ulm = 0.0, umm = 0.0;
  if (W > 0.0) {
    const double lm = vert[(size_t)v * 3 + 1], mm = vert[(size_t)v * 3 + 2];
    if (!Iold) {
      imm = mm;
      ilm = cs2_init * mm;
      ulm = ilm;
      umm = imm;
    } else {
      const double delta2 = D / W;
      // 1. the displacement
      double d[DIM];
      {
        const int c0 = vcell[begin];
        int node = p2[c0];
#pragma unroll
        for (int j = 1; j < NL; ++j)
          if (p1[(size_t)j * nc + c0] == v) node = p2[(size_t)j * nc + c0];
#pragma unroll
        for (int a = 0; a < DIM; ++a) d[a] = -(k * u[(size_t)node * DIM + a]);
      }
      // 2. the upstream cell
      double best = -INFINITY, lam[NL];
      int vb[NL];
#pragma unroll
      for (int j = 0; j < NL; ++j) {
        lam[j] = 0.0;
        vb[j] = v;
      }
      for (int e = begin; e < end; ++e) {
        const int c = vcell[e];
        double g[NL][DIM];
        LagrangeGeo<DIM>::gradients(vx, nc, c, g);
        int vc[NL];
        double l[NL], s = 0.0;
#pragma unroll
        for (int j = 0; j < NL; ++j) {
          vc[j] = p1[(size_t)j * nc + c];
          double t = 0.0;
#pragma unroll
          for (int a = 0; a < DIM; ++a) t += g[j][a] * d[a];
          l[j] = vc[j] == v ? 0.0 : t;           // (its own entry adds +0.0 to the sum, which changes no bit of it)
          s += l[j];
        }
        const double own = 1.0 - s;
        double m = INFINITY;
#pragma unroll
        for (int j = 0; j < NL; ++j) {
          if (vc[j] == v) l[j] = own;
          m = fmin(m, l[j]);
        }
        if (m > best) {
          best = m;
#pragma unroll
          for (int j = 0; j < NL; ++j) {
            lam[j] = l[j];
            vb[j] = vc[j];
          }
        }
      }
      if (best < 0.0) {
        double s = 0.0;
#pragma unroll
        for (int j = 0; j < NL; ++j) {
          lam[j] = fmax(lam[j], 0.0);
          s += lam[j];
        }
#pragma unroll
        for (int j = 0; j < NL; ++j) lam[j] /= s;
      }
      // 3. the upstream value
#pragma unroll
      for (int j = 0; j < NL; ++j) {
        const double2 I = reinterpret_cast<const double2*>(Iold)[vb[j]];
        ulm += lam[j] * I.x;
        umm += lam[j] * I.y;
      }
      // 4. the relaxation
      const double prod = ulm * umm;
      double eps = 1.0;
      if (prod > 0.0) {
        const double T = (theta * sqrt(delta2)) / sqrt(sqrt(sqrt(prod)));
        eps = k / (k + T);
      }
      const double keep = 1.0 - eps;
      imm = eps * mm + keep * umm;
      ilm = fmax(eps * lm + keep * ulm, cs2_floor * imm);
    }
  }
  // 5. the constant
  const double cs2 = imm > 0.0 ? fmin(fmax(ilm / imm, 0.0), cs2_max) : 0.0;
  reinterpret_cast<double2*>(Inew)[v] = make_double2(ilm, imm);
  cs2v[v] = cs2;
  if (up) reinterpret_cast<double2*>(up)[v] = make_double2(ulm, umm);
}

template <int DIM>
__global__ void k_dyn_scalar_moments(int nc, const double* __restrict__ vx, const int32_t* __restrict__ p2,
                                     const double* __restrict__ u, const double* __restrict__ T,
                                     double* __restrict__ mom);                             // <3>: assembly3d.hip

template <>
__global__ __launch_bounds__(256) void k_dyn_scalar_moments<2>(int nc, const double* __restrict__ vx,
                                                               const int32_t* __restrict__ p2,
                                                               const double* __restrict__ u,
                                                               const double* __restrict__ T,
                                                               double* __restrict__ mom) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= nc) return;
  DynFront<true> p(vx, nc, c, p2, u, T);
  double mt = 0.0, mtu[2] = {0.0, 0.0}, mu[2] = {0.0, 0.0}, md[2] = {0.0, 0.0}, mgd[2] = {0.0, 0.0};
  double ms[3] = {0.0, 0.0, 0.0};
  for (int q = 0; q < 7; ++q) {
    p.point(q);
    mt += p.w * p.tq;
    mtu[0] += p.w * (p.tq * p.uqx);
    mtu[1] += p.w * (p.tq * p.uqy);
    mu[0] += p.w * p.uqx;
    mu[1] += p.w * p.uqy;
    md[0] += p.w * p.dtx;
    md[1] += p.w * p.dty;
    mgd[0] += p.w * (p.gamma * p.dtx);
    mgd[1] += p.w * (p.gamma * p.dty);
#pragma unroll
    for (int k = 0; k < 3; ++k) ms[k] += p.w * p.S[k];
  }
  const double f = p.scale();
  double* o = mom + c;
  o[0] = f * mt;
#pragma unroll
  for (int a = 0; a < 2; ++a) {
    o[(size_t)(1 + a) * nc] = f * mtu[a];
    o[(size_t)(3 + a) * nc] = f * mu[a];
    o[(size_t)(5 + a) * nc] = f * md[a];
    o[(size_t)(7 + a) * nc] = (f * p.delta2) * mgd[a];
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) o[(size_t)(9 + k) * nc] = f * ms[k];
  o[(size_t)12 * nc] = p.vol;
  o[(size_t)13 * nc] = p.vol * p.delta2;
}

// vert[v] = {W_v, PR_v, RR_v}.  Rows of the moments: T | T u_a | u_a | d_a T | Delta^2 gamma d_a T | S_ab (a <= b in row
// order; the contraction S : S counts the off-diagonal pairs twice) | |K| | |K| Delta^2.  alpha2 = alpha^2
template <int DIM>
__global__ __launch_bounds__(256) void k_dyn_scalar_vertex(int nv, int nc, const int32_t* __restrict__ vptr,
                                                           const int32_t* __restrict__ vcell,
                                                           const double* __restrict__ mom, double alpha2,
                                                           double* __restrict__ vert) {
#pragma clang fp contract(off)
  constexpr int NM = dynamic_moment_rows(DIM, true);
  const int v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= nv) return;
  double a[NM], W;
  double* o = vert + (size_t)v * 3;
  if (!patch_mean(v, nc, vptr, vcell, mom, a, W)) {      // (a vertex of no cell: no contribution)
    o[0] = o[1] = o[2] = 0.0;
    return;
  }
  constexpr int TU = 1, UU = 1 + DIM, DT = 1 + 2 * DIM, GD = 1 + 3 * DIM, SS = 1 + 4 * DIM;
  const double d2 = a[NM - 1];
  const double coef = (alpha2 * d2) * patch_shear_rate<DIM>(a + SS);
  double pr = 0.0, rr = 0.0;
#pragma unroll
  for (int r = 0; r < DIM; ++r) {
    const double P = a[TU + r] - a[0] * a[UU + r];
    const double R = a[GD + r] - coef * a[DT + r];
    pr += P * R;
    rr += R * R;
  }
  o[0] = W;
  o[1] = pr;
  o[2] = rr;
}

// T null: C_s^2 on u (k_dyn_moments, k_dyn_vertex); else C_theta on (u, T) (the k_dyn_scalar_ pair)
// lag given (mode 1 of nsfem_set_dynamic_averaging, T null): k_dyn_lagrange in the place of k_dyn_reduce; with
// lag->vertex_only the third launch is left out (the vertex rows alone, for the output hook)
void launch_dynamic_constant(hipStream_t s, const MeshDev& m, const double* u, const double* T, double alpha,
                             double clip, const DynamicDev& d, const DynamicLagrangeDev* lag) {
  NSFEM_REQUIRE(d.n_groups >= 1 && d.vptr && d.vcell && d.goff && d.gvert && d.mom && d.vert && d.sums && d.cs2v,
                T ? "dynamic subgrid heat flux: buffers not allocated" : "dynamic Smagorinsky: buffers not allocated");
  NSFEM_REQUIRE(!lag || (!T && (lag->vertex_only || (lag->Inew && lag->Inew != lag->Iold))),
                "dynamic Smagorinsky: Lagrangian averaging needs two state buffers and no scalar");
  const dim3 cells(grid_for(m.n_cells)), verts(grid_for(m.n_p1)), block(kBlock);
  if (m.dim == 3) dynamic_moments_3d(s, m, u, T, d.mom);
  else if (T) hipLaunchKernelGGL((k_dyn_scalar_moments<2>), cells, block, 0, s, m.n_cells, m.vx.p, m.p2.p, u, T, d.mom);
  else hipLaunchKernelGGL((k_dyn_moments<2>), cells, block, 0, s, m.n_cells, m.vx.p, m.p2.p, u, d.mom);
  with_int<3, 2>(m.dim, [&](auto dc) {
    constexpr int DIM = decltype(dc)::value;
    const auto vertex = T ? k_dyn_scalar_vertex<DIM> : k_dyn_vertex<DIM>;
    hipLaunchKernelGGL(vertex, verts, block, 0, s, m.n_p1, m.n_cells, d.vptr, d.vcell, d.mom, alpha * alpha, d.vert);
  });
  if (!lag) {
    hipLaunchKernelGGL(k_dyn_reduce, dim3(d.n_groups), dim3(256), 0, s, d.goff, d.gvert, d.vert, clip, d.sums, d.cs2v);
  } else if (!lag->vertex_only) {
    with_int<3, 2>(m.dim, [&](auto dc) {
      constexpr int DIM = decltype(dc)::value;
      const double* mom2 = d.mom + (size_t)(dynamic_moment_rows(DIM, false) - 2) * m.n_cells;
      hipLaunchKernelGGL(k_dyn_lagrange<DIM>, verts, dim3(256), 0, s, m.n_p1, m.n_cells, d.vptr, d.vcell, m.p1.p, m.p2.p,
                         m.vx.p, u, mom2, d.vert, lag->Iold, lag->k, lag->theta, lag->cs2_init, lag->cs2_floor, clip,
                         lag->Inew, d.cs2v, lag->up);
    });
  }
  NSFEM_HIP(hipGetLastError());
}

void launch_viscosity_gather(hipStream_t s, const MeshDev& m, double b0, double* n1, double* rhs) {
  const int64_t n = (int64_t)m.n_p2 * m.dim;
  hipLaunchKernelGGL(k_visc_gather, dim3(grid_for(n)), dim3(kBlock), 0, s, n, m.dim, m.nptr.p, m.rbuf.p, b0, n1, rhs);
  NSFEM_HIP(hipGetLastError());
}

// ---------------------------------------------------------------- immersed bodies (nsfem_set_bodies)
// Brinkman volume penalisation, one thread per CELL, 7-point rule (part of the definition: the integrand is no
// polynomial):
//   r_(i,a) = scale sum_q w_q |det J| chi(x_q) (u(x_q) - u_s(x_q))_a phi_i(x_q),   scale = weight / eta,
// x_q the affine image of the reference point (the P1 basis values are its barycentric coordinates), chi and u_s those
// of the body with the largest chi at x_q (bodies.hpp).  u at the 6 nodes in registers; x_q, the winning body, chi and
// u - u_s of a quadrature point are formed once and shared by the 6 test functions.  The element vector goes
// node-sorted into m.rbuf (ndst, as k_visc_var_cell); k_visc_gather sums the node runs: no atomics, no LDS, the same
// state gives the same bytes.  Quadrature points with chi = 0 are skipped: a cell no body reaches stores zeros.
// SMOOTH false: every mask is sharp and no sin is called.  MEAN: rbuf[c] = sum_q w_q chi(x_q) / sum_q w_q instead.
template <bool SMOOTH, bool MEAN>
__global__ __launch_bounds__(256) void k_penal_cell(int nc, const double* __restrict__ vx,
                                                    const int32_t* __restrict__ p2,
                                                    const double* __restrict__ u, double scale, const BodyTable bt,
                                                    const int32_t* __restrict__ ndst, double* __restrict__ rbuf) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= nc) return;
  double xv[3][2];
#pragma unroll
  for (int v = 0; v < 3; ++v) {
    xv[v][0] = vx[(size_t)(2 * v) * nc + c];
    xv[v][1] = vx[(size_t)(2 * v + 1) * nc + c];
  }
  const CellGeo g = load_geo(vx, nc, c);
  double ux[6], uy[6];
  if (!MEAN) {
#pragma unroll
    for (int k = 0; k < 6; ++k) {
      const int node = p2[(size_t)k * nc + c];
      const double2 a = reinterpret_cast<const double2*>(u)[node];
      ux[k] = a.x;
      uy[k] = a.y;
    }
  }
  double rx[6], ry[6];
#pragma unroll
  for (int i = 0; i < 6; ++i) rx[i] = ry[i] = 0.0;
  double mean = 0.0, wsum = 0.0;
  for (int q = 0; q < 7; ++q) {
    double x[2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
      x[a] = c_q.phi1[q][0] * xv[0][a] + c_q.phi1[q][1] * xv[1][a] + c_q.phi1[q][2] * xv[2][a];
    int win;
    const double chi = body_winner<2, SMOOTH>(bt, x, win);
    if (MEAN) {
      mean += c_q.w[q] * chi;
      wsum += c_q.w[q];
      continue;
    }
    if (!(chi > 0.0)) continue;
    double us[2], uqx = 0.0, uqy = 0.0;
    body_velocity<2>(bt, win, x, us);
#pragma unroll
    for (int k = 0; k < 6; ++k) {
      uqx += c_q.phi2[q][k] * ux[k];
      uqy += c_q.phi2[q][k] * uy[k];
    }
    const double w = c_q.w[q] * g.adet * scale * chi;
    const double fx = w * (uqx - us[0]), fy = w * (uqy - us[1]);
#pragma unroll
    for (int i = 0; i < 6; ++i) {
      rx[i] += fx * c_q.phi2[q][i];
      ry[i] += fy * c_q.phi2[q][i];
    }
  }
  if (MEAN) {
    rbuf[c] = mean / wsum;
  } else {
    double2* out = reinterpret_cast<double2*>(rbuf);
#pragma unroll
    for (int i = 0; i < 6; ++i) out[ndst[(size_t)i * nc + c]] = make_double2(rx[i], ry[i]);
  }
}

void launch_penalty_cells(hipStream_t s, const MeshDev& m, const double* u, double weight, const BodyTable& bt,
                          bool mean) {
  NSFEM_REQUIRE(bt.n > 0, "immersed bodies: no body set");
  if (m.dim == 3) return penalty_cells_3d(s, m, u, weight, bt, mean);
  const dim3 grid(grid_for(m.n_cells)), block(kBlock);
  const double scale = weight * bt.inv_eta;
#define NSFEM_PC(S, M) \
  hipLaunchKernelGGL((k_penal_cell<S, M>), grid, block, 0, s, m.n_cells, m.vx.p, m.p2.p, u, scale, bt, m.ndst.p, m.rbuf.p)
  if (bt.eps > 0.0) { if (mean) NSFEM_PC(true, true); else NSFEM_PC(true, false); }
  else { if (mean) NSFEM_PC(false, true); else NSFEM_PC(false, false); }
#undef NSFEM_PC
  NSFEM_HIP(hipGetLastError());
}

// ---------------------------------------------------------------- IMEX right-hand side
// rhs = -(t + (b0 n1 + b1 n2)): the last operation of the right-hand side of nsfem_step_imex, shared by the generic
// path (k_imex_combine) and the lattice kernel (k_jac_lattice<FORM, 3>).  No contraction: both callers must round
// the same way whatever surrounds the call
__device__ __forceinline__ double imex_rhs_value(double t, double n1, double n2, double b0, double b1, bool have_n2) {
#pragma clang fp contract(off)
  const double old = have_n2 ? b1 * n2 : 0.0;
  const double e = fma(b0, n1, old);
  return -(t + e);
}
// u* - dx of the Newton update: the expression of the vector launch it replaces, k_axpby(1, u, -1, dx) =
// a x + b y (contracted or not, the products with 1 and -1 are exact: one rounding, that of the difference)
__device__ __forceinline__ double newton_update_value(double u, double dx) { return 1.0 * u + (-1.0 * dx); }
__global__ __launch_bounds__(256) void k_imex_combine(int64_t n, const double* __restrict__ t,
                                                      const double* __restrict__ n1, const double* __restrict__ n2,
                                                      double b0, double b1, double* __restrict__ rhs) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  rhs[i] = imex_rhs_value(t[i], n1[i], n2 ? n2[i] : 0.0, b0, b1, n2 != nullptr);
}
void launch_imex_combine(hipStream_t s, int64_t n, const double* t, const double* n1, const double* n2, double b0,
                         double b1, double* rhs) {
  hipLaunchKernelGGL(k_imex_combine, dim3(grid_for(n)), dim3(kBlock), 0, s, n, t, n1, n2, b0, b1, rhs);
  NSFEM_HIP(hipGetLastError());
}

// ---------------------------------------------------------------- lattice Jacobian action
// y = L x + c_c [d conv(u)/du] x  (identity on the rows flagged in the mask) in ONE launch on 2D lattice meshes
// (rectangle_mesh numbering: cell 2 (sy nx + sx) + t, P2 node j W + i): the pair of launches it replaces --
// k_conv_cell (element vectors -> node-sorted buffer in HBM) and the dictionary product that sums the buffer --
// moves 96 B per cell out and in again, and the element kernel's scattered 16-byte stores and dependent index
// loads keep it at a third of its VALU bound.  Here a workgroup owns the nodes of 31 x 7 squares:
//   phase 0  u and x on the 65 x 17 nodes the 32 x 8 squares around them touch are staged in LDS (row-contiguous
//            global reads), together with the operator's stencil dictionary;
//   phase 1  one thread per owned node: acc = (L x)(node) from the LDS copy of x -- the dictionary entry's
//            products in entry order, exactly the sum of k_spmv_dict;
//   phase 2  one thread per cell (512 cells, the one-square ring around the owned nodes is recomputed by the
//            neighbouring workgroups): node values from LDS, conv_cell_eval in registers -- no index loads, the
//            node positions of a cell are a template of its type;
//   phase 3  six rounds: in round r every cell adds its element vector entry to the node it is the r-th
//            adjacent cell of (ascending cell number: at most one writer per node and round, and the node sums
//            come out in the order of the node-sorted buffer, bit for bit);
//   phase 4  y written once (coalesced 16-byte stores).
// Algorithmic bytes per launch: u, x read, y written (48 B per node), 48 B per cell of vertex coordinates, one
// byte per node of dictionary ids and two of masks.
// tile shapes: SX x SY squares per workgroup (powers of two; one cell per thread, 2 SX SY threads), of which the
// workgroup owns the nodes of (SX - 1) x (SY - 1)
// Variants (V): 0 the kernel above (NSFEM_JL_KERNEL=0, for A/B runs); 1 one cell type per wave (wave w holds the
// cells of type w & 1: the type, its node template and rank template are wave-uniform) and phase 3 as a gather --
// every cell stores its element vector to LDS once (over the dead staging buffers), and after ONE barrier the thread
// of each owned node adds its <= 6 contributions in ascending cell order onto L x (+ g) kept in registers: the same
// additions in the same order as the six rounds, bit for bit; 2 as 1 with the physical gradients and weights of the
// two cell types read from tables (uniform lattices: phys() once per type in k_grad_tables, the same bits)
// LIN = 3 (variant 2 only: uniform lattices): the right-hand side of the IMEX diffusion step.  u = u1 AND ix.u2 are staged (the layout of
// the Jacobian action: two staged vectors; the second value table of 8 B per dictionary entry fits under the element
// vectors' overlay, the workgroup's LDS does not grow); phase 1 forms (L1 u1)(node) and (L2 u2)(node) from the two
// value tables of the shared dictionary and adds them and g; phase 2 is the residual's element kernel on u1; the
// gather sums the node's element vectors from +0.0 on -- c_c conv(u1), stored to ix.n1 -- and writes
// imex_rhs_value(...) with the stored ix.n2: the generic sequence of nsfem_step_imex, bit for bit.
// LIN = 4: LIN 3 on the strip of a partitioned mesh (the rank's own lattice: own cell rows + the ghost row).  The row
// mask is read as in the Jacobian action; on the rows of ghost nodes (mask value 2) the partial sums are dropped and
// BOTH outputs are written as +0.0 -- the right-hand side and the stored c_c conv(u1) (no owned row ever reads the
// latter: n2 is read row-wise).  Owned rows: the arithmetic and summation order of LIN 3, untouched.
// LIN = 5, 6: LIN 3, 4 with the rotation flag of conv_cell_eval_g set -- the stored vector is c_c conv(u1) + M (gam e_z x
// u1), gam = ix.gam = 2 c_cor omega(t^n) (the rotating frame of the IMEX step).  Instantiations of their own: modes 0 - 4
// compile as without them.
struct TabGrad {
  const double* __restrict__ t;   // [7][6][2] gradients, then [7] weights of one cell type (wave-uniform address)
  __device__ __forceinline__ void grad(int q, int k, double& gx, double& gy) const {
    gx = t[(q * 6 + k) * 2];
    gy = t[(q * 6 + k) * 2 + 1];
  }
  __device__ __forceinline__ double wdet(int q) const { return t[84 + q]; }
};

struct JacLatArgs {
  int nx, ny, W, H, nc;
  int ntx, ntiles;
  int tbase, tsplit, tskip;   // tile = tbase + (t < tsplit ? t : t + tskip), t < ntiles: the whole lattice, or the tile
                              // rows away from / next to the ghost lines of a partitioned strip (two launches around
                              // the halo exchange)
  int lmax, lp, n_st;   // lp: table row stride (lmax rounded up to 4, zero padded)
  int dbg;              // knock-out build only (NSFEM_KNOCKOUTS): 1 no element kernel, 2 no L product, 4 no node sums
  double cc;
  // node sums by gather (variants 1, 2): per parity class (i & 1) + 2 (j & 1) of a node, its six contributions in
  // ascending cell order as element-vector offsets from the node's square ((j >> 1) SX + (i >> 1)) plus 2 SX, 16 bits
  // each (two per int; classes with fewer than six cells point the rest at the plane of -0.0).  Indexed by constants
  // only (selected per lane with v_cndmask)
  int gl[4][3];
  // per cell type t and local node k, packed 6 x 5 bits (k-th field): the node's lattice offset from the square's corner
  // node as dj * 3 + di, and the cell's rank among the cells around that node (ascending cell number).  Plain
  // integers on purpose: an array indexed by the lane's cell type turns into VECTOR loads from the kernel-argument
  // segment (38 per wave, ~14 us of the launch).
  int noff0, noff1, rank0, rank1;
};

template <int FORM, int LIN, int SX, int SY, int V>
__global__ __launch_bounds__(2 * SX * SY) __attribute__((amdgpu_waves_per_eu(4, 4)))
void k_jac_lattice(JacLatArgs a, const double* __restrict__ vx, const double* __restrict__ u,
                   const double* __restrict__ x, const uint8_t* __restrict__ sid8,
                   const uint8_t* __restrict__ mask, const int32_t* __restrict__ slen,
                   const int32_t* __restrict__ spack, const double* __restrict__ sval,
                   const double* __restrict__ gadd, double* __restrict__ y, const double* __restrict__ ugeo,
                   ImexLatArgs ix) {
  // LIN = 0: the momentum residual  y = L u + g + c_c conv(u)  (x is not read, no mask: the Dirichlet rows are
  // set by the caller afterwards); g joins the node's sum after the L product and before the element vectors,
  // the order of the launches it replaces (product, axpby, k_conv_cell, k_res_gather).
  // ugeo: V 0, 1 the two types' geometry [2][5] (uniform lattices; null: load_geo per cell), V 2 the gradient tables
  // LIN = 7, 8 (variants 1, 2): LIN 0 with the frame of the Newton iteration (see launch_residual_frame_lattice)
  constexpr bool ROWS = LIN == 7 || LIN == 8;                       // Dirichlet rows u - g_D and the tile's sum of squares
  constexpr bool UPD = LIN == 8;                                    // u = u_old - x staged, and stored to ix.unew
  constexpr int BL = ROWS ? 0 : LIN;                                // the mode underneath
  constexpr bool IMX = BL >= 3;
  constexpr bool GH = BL == 4 || BL == 6;                           // ghost rows of a strip -> 0
  constexpr bool ROT = BL >= 5;                                     // Coriolis term in the element vector
  constexpr bool RES = BL == 0 || IMX;
  constexpr bool TWO = BL != 0;                                     // a second staged vector (x, or u2)
  constexpr int CLIN = IMX ? 0 : BL;                                // mode of the element kernel
  static_assert(!ROWS || V != 0, "the Newton frame is built for the gather variants only");
  static_assert(!IMX || V == 2, "the right-hand-side mode is built for the table variant only");
  extern __shared__ __attribute__((aligned(16))) double sh_jl[];
  constexpr int NT = 2 * SX * SY;                                   // threads
  constexpr int kJlNW = 2 * SX + 1, kJlNH = 2 * SY + 1;             // staged node lines
  constexpr int kJlOX = 2 * (SX - 1), kJlOY = 2 * (SY - 1);         // owned node lines
  constexpr int LOGSX = SX == 32 ? 5 : SX == 16 ? 4 : 3;
  static_assert((1 << LOGSX) == SX, "SX: 8, 16 or 32");
  constexpr int NN = kJlNW * kJlNH;
  // (V 1, 2: sa first, the element vectors of phase 3 then overlay su, sx and the tables: NN + 12 SX SY double2)
  double2* __restrict__ su = reinterpret_cast<double2*>(sh_jl) + (V ? NN : 0);
  double2* __restrict__ sx = TWO ? su + NN : su;
  double2* __restrict__ sa = V ? reinterpret_cast<double2*>(sh_jl) : sx + NN;
  double* __restrict__ tv = reinterpret_cast<double*>((V ? sx : sa) + NN);   // [n_st * lp]
  double* __restrict__ tv2 = tv + a.n_st * a.lp;                             // (LIN 3: the values of L2)
  int* __restrict__ to = reinterpret_cast<int*>(tv + (IMX ? 2 : 1) * a.n_st * a.lp);
  int* __restrict__ tl = to + a.n_st * a.lp;
  // XCD x (workgroups b = x mod 8) walks a contiguous range of tiles: neighbouring tiles share their halo in L2
  const int per = (a.ntiles + 7) >> 3;
  const int tlin = (int)(blockIdx.x & 7) * per + (int)(blockIdx.x >> 3);
  if (tlin >= a.ntiles || NSFEM_KO(a.dbg & 256)) return;
  const int tile = a.tbase + (tlin < a.tsplit ? tlin : tlin + a.tskip);
  const int ty = tile / a.ntx, tx = tile - ty * a.ntx;
  const int i0 = tx * kJlOX - 2, j0 = ty * kJlOY - 2;               // lattice position of the LDS tile's corner
  const int tid = threadIdx.x;
  const double2* __restrict__ u2 = reinterpret_cast<const double2*>(u);
  const double2* __restrict__ x2 = reinterpret_cast<const double2*>(IMX ? ix.u2 : x);
  // ---- phase 0: every global load of the workgroup is requested before the first one is waited for
  constexpr int NLD = (NN + NT - 1) / NT;
  double2 uv[NLD], xv[NLD];
#pragma unroll
  for (int r = 0; r < NLD; ++r) {
    const int t = tid + r * NT;
    const int lj = t / kJlNW, li = t - lj * kJlNW;
    const int gi = i0 + li, gj = j0 + lj;
    uv[r] = make_double2(0.0, 0.0);
    xv[r] = uv[r];
    if (t < NN && gi >= 0 && gi < a.W && gj >= 0 && gj < a.H && !NSFEM_KO(a.dbg & 8)) {
      const size_t g = (size_t)gj * a.W + gi;
      uv[r] = u2[g];
      if (TWO || UPD) xv[r] = x2[g];
    }
    if constexpr (UPD) {
      // the Newton update u_old - dx, entry by entry as the launch it replaces forms it (outside the lattice: 0 - 0)
      uv[r].x = newton_update_value(uv[r].x, xv[r].x);
      uv[r].y = newton_update_value(uv[r].y, xv[r].y);
    }
  }
  // (this thread's cell, its two owned nodes)
  static_assert(NT % 128 == 0 && SX <= 64, "whole waves per cell type");
  int ct, sxl, syl;
  if constexpr (V == 0) {
    ct = tid & 1; sxl = (tid >> 1) & (SX - 1); syl = tid >> (1 + LOGSX);
  } else {
    // wave w: cells of type w & 1 in the 64 / SX square rows from (w >> 1) 64 / SX on (readfirstlane: an SGPR)
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    ct = wv & 1; sxl = tid & (SX - 1); syl = ((wv >> 1) << (6 - LOGSX)) | ((tid & 63) >> LOGSX);
  }
  const int sqx = (i0 >> 1) + sxl, sqy = (j0 >> 1) + syl;          // (i0, j0 even; >> is an arithmetic shift)
  const bool cell = sqx >= 0 && sqx < a.nx && sqy >= 0 && sqy < a.ny;
  CellGeo geo;
  if constexpr (V == 2) {
  } else if (ugeo) {
    // uniform lattice: the two cell types' geometry through the scalar cache (wave-uniform addresses), picked per lane
    const double g0[5] = {ugeo[0], ugeo[1], ugeo[2], ugeo[3], ugeo[4]};
    const double g1[5] = {ugeo[5], ugeo[6], ugeo[7], ugeo[8], ugeo[9]};
    geo.ji00 = cell ? (ct ? g1[0] : g0[0]) : 1.0;
    geo.ji01 = cell ? (ct ? g1[1] : g0[1]) : 1.0;
    geo.ji10 = cell ? (ct ? g1[2] : g0[2]) : 1.0;
    geo.ji11 = cell ? (ct ? g1[3] : g0[3]) : 1.0;
    geo.adet = cell ? (ct ? g1[4] : g0[4]) : 1.0;
  } else if (cell && !NSFEM_KO(a.dbg & 16)) geo = load_geo(vx, a.nc, 2 * (sqy * a.nx + sqx) + ct);
  else geo.ji00 = geo.ji01 = geo.ji10 = geo.ji11 = geo.adet = 1.0;
  constexpr int OWN = kJlOX * kJlOY, NOWN = (OWN + NT - 1) / NT;
  int obase[NOWN], oent[NOWN], omask[NOWN];
  size_t onode[NOWN];
  double2 og[RES ? NOWN : 1];
  double2 on2[IMX ? NOWN : 1];
  double2 ogd[ROWS ? NOWN : 1];
#pragma unroll
  for (int r = 0; r < NOWN; ++r) {
    const int o = tid + r * NT;
    const int oj = o / kJlOX, oi = o - oj * kJlOX;
    const int gi = i0 + 2 + oi, gj = j0 + 2 + oj;
    obase[r] = -1;
    oent[r] = 0;
    omask[r] = 0;
    onode[r] = 0;
    if (o < OWN && gi < a.W && gj < a.H) {
      obase[r] = (oj + 2) * kJlNW + oi + 2;
      onode[r] = (size_t)gj * a.W + gi;
      oent[r] = sid8[onode[r]];
      if (RES) og[r] = reinterpret_cast<const double2*>(gadd)[onode[r]];
      if (IMX) on2[r] = ix.n2 ? reinterpret_cast<const double2*>(ix.n2)[onode[r]] : make_double2(0.0, 0.0);
      if (!RES || GH || ROWS) omask[r] = reinterpret_cast<const uint16_t*>(mask)[onode[r]];
      if constexpr (ROWS) {
        // Dirichlet values: fetched by the lanes of flagged components only (the dense vector of nsfem_set_dirichlet)
        ogd[r] = make_double2(0.0, 0.0);
        if (omask[r] & 0x00ff) ogd[r].x = ix.gd[2 * onode[r]];
        if (omask[r] & 0xff00) ogd[r].y = ix.gd[2 * onode[r] + 1];
      }
    }
  }
  for (int t = tid; t < a.n_st * a.lp; t += NT) {
    const int e = t / a.lp, k = t - e * a.lp;
    const bool in = k < a.lmax;
    tv[t] = in ? sval[e * a.lmax + k] : 0.0;
    if (IMX) tv2[t] = in ? ix.sval2[e * a.lmax + k] : 0.0;
    const int pk = in ? spack[e * a.lmax + k] : (8 * 32 + 8);
    to[t] = ((pk >> 5) - 8) * kJlNW + ((pk & 31) - 8);
  }
  if (tid < a.n_st) tl[tid] = slen[tid];
  if NSFEM_KO(a.dbg & 512) return;
#pragma unroll
  for (int r = 0; r < NLD; ++r) {
    const int t = tid + r * NT;
    if (t < NN) {
      su[t] = uv[r];
      if (TWO) sx[t] = xv[r];
    }
  }
  __syncthreads();
  if NSFEM_KO(a.dbg & 128) return;
  // ---- phase 1: (L x) on the owned nodes; four entries of the row in flight (rows are zero padded to 4).
  // (Measured and rejected: advancing the rows of the thread's two nodes together with the next trip's table
  // entries prefetched -- 51.1 instead of 48.3 us per launch at n = 512.)
#pragma unroll
  for (int r = 0; r < NOWN; ++r) {
    if (obase[r] < 0) continue;
    const int base = obase[r];
    const int L = NSFEM_KO(a.dbg & 2) ? 0 : tl[oent[r]];
    const int* __restrict__ op = to + oent[r] * a.lp;
    const double* __restrict__ vp = tv + oent[r] * a.lp;
    const double2* __restrict__ s1 = IMX ? su : sx;
    double ax = 0.0, ay = 0.0;
    for (int k = 0; k < L; k += 4) {
      const int4 o4 = *reinterpret_cast<const int4*>(op + k);
      const double2 va = *reinterpret_cast<const double2*>(vp + k), vb = *reinterpret_cast<const double2*>(vp + k + 2);
      const double2 x0 = s1[base + o4.x], x1 = s1[base + o4.y], x2_ = s1[base + o4.z], x3 = s1[base + o4.w];
      ax = fma(va.x, x0.x, ax); ay = fma(va.x, x0.y, ay);
      ax = fma(va.y, x1.x, ax); ay = fma(va.y, x1.y, ay);
      ax = fma(vb.x, x2_.x, ax); ay = fma(vb.x, x2_.y, ay);
      ax = fma(vb.y, x3.x, ax); ay = fma(vb.y, x3.y, ay);
    }
    if constexpr (IMX) {
      // (L2 u2)(node): the same row of the shared dictionary with L2's values, then L1 u1 + L2 u2 (the generic
      // path's axpby with weights 1, 1)
      const double* __restrict__ vq = tv2 + oent[r] * a.lp;
      double bx = 0.0, by = 0.0;
      for (int k = 0; k < L; k += 4) {
        const int4 o4 = *reinterpret_cast<const int4*>(op + k);
        const double2 va = *reinterpret_cast<const double2*>(vq + k), vb = *reinterpret_cast<const double2*>(vq + k + 2);
        const double2 x0 = sx[base + o4.x], x1 = sx[base + o4.y], x2_ = sx[base + o4.z], x3 = sx[base + o4.w];
        bx = fma(va.x, x0.x, bx); by = fma(va.x, x0.y, by);
        bx = fma(va.y, x1.x, bx); by = fma(va.y, x1.y, by);
        bx = fma(vb.x, x2_.x, bx); by = fma(vb.x, x2_.y, by);
        bx = fma(vb.y, x3.x, bx); by = fma(vb.y, x3.y, by);
      }
      ax += bx; ay += by;
    }
    if (RES) { ax += og[r].x; ay += og[r].y; }
    if constexpr (ROWS) {
      // the node's new u* while su is staged: written out (never in place: the neighbouring tiles read the old halo),
      // and on a flagged component the row's value u - g_D takes the place of the partial sum (the gather skips it)
      const double2 uo = su[base];
      if (UPD) reinterpret_cast<double2*>(ix.unew)[onode[r]] = uo;
      if (omask[r] & 0x00ff) ax = uo.x - ogd[r].x;
      if (omask[r] & 0xff00) ay = uo.y - ogd[r].y;
    }
    if (V != 0 && !RES) {
      // V 1, 2: the identity row's value now, while sx is staged (flag 1: identity row; flag 2: ghost row of a
      // partitioned strip -> 0); the node sum does not enter it
      const double2 xo = sx[base];
      if (omask[r] & 0x00ff) ax = (omask[r] & 0x0002) ? 0.0 : xo.x;
      if (omask[r] & 0xff00) ay = (omask[r] & 0x0200) ? 0.0 : xo.y;
    }
    sa[base] = make_double2(ax, ay);
  }
  // ---- phase 2: the element vector of this thread's cell
  int nl[6];
  double rx[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, ry[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  const int corner = 2 * syl * kJlNW + 2 * sxl;
  const int pno = a.noff0 ^ ((a.noff0 ^ a.noff1) & -ct), prk = a.rank0 ^ ((a.rank0 ^ a.rank1) & -ct);
#pragma unroll
  for (int k = 0; k < 6; ++k) {
    const int f = (pno >> (5 * k)) & 31;          // dj * 3 + di
    const int dj = (f * 11) >> 5;                 // f / 3 for f < 9
    nl[k] = corner + dj * kJlNW + (f - 3 * dj);
  }
  if (cell && !NSFEM_KO(a.dbg & 64)) {
    double ux[6], uy[6], wx[RES ? 1 : 6], wy[RES ? 1 : 6];
#pragma unroll
    for (int k = 0; k < 6; ++k) {
      const double2 p = su[nl[k]];
      ux[k] = p.x; uy[k] = p.y;
      if (!RES) {
        const double2 q = sx[nl[k]];
        wx[k] = q.x; wy[k] = q.y;
      }
    }
    if NSFEM_KO(a.dbg & 1) {
#pragma unroll
      for (int k = 0; k < 6; ++k) { rx[k] = ux[k]; ry[k] = uy[k]; }
    } else {
      if constexpr (V == 2)
        conv_cell_eval_g<FORM, CLIN, ROT>(TabGrad{ugeo + kGradTab * ct}, ux, uy, wx, wy, a.cc, rx, ry, ROT ? ix.gam : 0.0);
      else conv_cell_eval<FORM, CLIN>(geo, ux, uy, wx, wy, a.cc, rx, ry);
    }
  }
  __syncthreads();
  double2* __restrict__ y2 = reinterpret_cast<double2*>(y);
  if constexpr (V != 0) {
    // ---- phase 3 (gather): element vectors over the staging buffers, [t][k][SY][SX] (a wave stores contiguous runs),
    // then a 13th plane of -0.0.  Squares outside the lattice store -0.0 as well: x + (-0.0) is x bit for bit (+0.0
    // included), so every node adds six entries without a test and the sums keep the bits of the six rounds
    constexpr int NSQ = SX * SY;
    double2* __restrict__ se = reinterpret_cast<double2*>(sh_jl) + NN;
    const double2 nz = make_double2(-0.0, -0.0);
#pragma unroll
    for (int k = 0; k < 6; ++k) se[(ct * 6 + k) * NSQ + syl * SX + sxl] = cell ? make_double2(rx[k], ry[k]) : nz;
    for (int t = tid; t < NSQ; t += NT) se[12 * NSQ + t] = nz;
    __syncthreads();
    double ssq = 0.0;                                              // (ROWS) squares of what this thread stores
#pragma unroll
    for (int r = 0; r < NOWN; ++r) {
      if (obase[r] < 0) continue;
      const int o = tid + r * NT;
      const int oj = o / kJlOX, oi = o - oj * kJlOX;
      const int li = oi + 2, lj = oj + 2;                          // LDS tile position (i0, j0 even: same parity)
      int pe[3];
#pragma unroll
      for (int h = 0; h < 3; ++h) pe[h] = (lj & 1) ? ((li & 1) ? a.gl[3][h] : a.gl[2][h]) : ((li & 1) ? a.gl[1][h] : a.gl[0][h]);
      const double2* __restrict__ sq = se + ((lj >> 1) * SX + (li >> 1) - 2 * SX);
      const double2 a0 = sa[obase[r]];
      double vx_ = IMX ? 0.0 : a0.x, vy_ = IMX ? 0.0 : a0.y;
#pragma unroll
      for (int e = 0; e < 6; ++e) {
        if NSFEM_KO(a.dbg & 4) break;
        const double2 v = sq[(pe[e >> 1] >> (16 * (e & 1))) & 0xffff];
        vx_ += v.x;
        vy_ += v.y;
      }
      double2 v = make_double2(vx_, vy_);
      if constexpr (IMX) {
        if constexpr (GH) {
          if (omask[r] & 0x0002) v = make_double2(0.0, 0.0);        // (ghost node: both components carry the flag)
        }
        reinterpret_cast<double2*>(ix.n1)[onode[r]] = v;
        const bool have = ix.n2 != nullptr;
        v.x = imex_rhs_value(a0.x, vx_, on2[r].x, ix.b0, ix.b1, have);
        v.y = imex_rhs_value(a0.y, vy_, on2[r].y, ix.b0, ix.b1, have);
        if constexpr (GH) {
          if (omask[r] & 0x0002) v = make_double2(0.0, 0.0);
        }
      }
      if (!RES || ROWS) {
        if (omask[r] & 0x00ff) v.x = a0.x;
        if (omask[r] & 0xff00) v.y = a0.y;
      }
      if (!NSFEM_KO(a.dbg & 32) || v.x == 1.2345) y2[onode[r]] = v;
      if constexpr (ROWS) {
        const double qx = v.x, qy = v.y;
        ssq = fma(qx, qx, ssq);
        ssq = fma(qy, qy, ssq);
      }
    }
    if constexpr (ROWS) {
      // the tile's sum of squares in a fixed order: lanes of a wave (shuffle tree), then the waves in ascending order.
      // The wave sums go to the first entries of sa: the halo lines of the tile, which no phase reads or writes
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) ssq += __shfl_down(ssq, off, 64);
      if ((tid & 63) == 0) sh_jl[tid >> 6] = ssq;
      __syncthreads();
      if (tid == 0) {
        double t = sh_jl[0];
#pragma unroll
        for (int w = 1; w < NT / 64; ++w) t += sh_jl[w];
        ix.tparts[tlin] = t;
      }
    }
    return;
  }
  // ---- phase 3: node sums in ascending cell order
#pragma unroll
  for (int r = 0; r < 6; ++r) {
#pragma unroll
    for (int k = 0; k < 6; ++k) {
      const int rk = (prk >> (5 * k)) & 31;
      if (cell && rk == r && !NSFEM_KO(a.dbg & 4)) {
        double2 v = sa[nl[k]];
        v.x += rx[k];
        v.y += ry[k];
        sa[nl[k]] = v;
      }
    }
    __syncthreads();
  }
  // ---- phase 4
#pragma unroll
  for (int r = 0; r < NOWN; ++r) {
    if (obase[r] < 0) continue;
    double2 v = sa[obase[r]];
    if (!RES) {
      const double2 xo = sx[obase[r]];
      // (flag 1: identity row; flag 2: ghost row of a partitioned strip -> 0, as the SpMV kernels write it)
      if (omask[r] & 0x00ff) v.x = (omask[r] & 0x0002) ? 0.0 : xo.x;
      if (omask[r] & 0xff00) v.y = (omask[r] & 0x0200) ? 0.0 : xo.y;
    }
    if (!NSFEM_KO(a.dbg & 32) || v.x == 1.2345) y2[onode[r]] = v;
  }
}

bool build_cell_lattice(const int32_t* p2map, int nc, int W, int H, CellLattice& cl) {
  cl.ok = false;
  cl.geo_uniform = false;
  cl.nx = cl.ny = cl.W = cl.H = 0;
  cl.tried = true;
  if (W < 7 || H < 7 || !(W & 1) || !(H & 1)) return false;
  const int nx = (W - 1) / 2, ny = (H - 1) / 2;
  if ((int64_t)2 * nx * ny != nc) return false;
  // the template of the two cell types: node positions relative to the square's corner node
  for (int t = 0; t < 2; ++t)
    for (int k = 0; k < 6; ++k) {
      const int node = p2map[(size_t)t * 6 + k];
      const int j = node / W, i = node - j * W;
      if (i > 2 || j > 2) return false;
      cl.di[t][k] = i;
      cl.dj[t][k] = j;
    }
  for (int sy = 0; sy < ny; ++sy)
    for (int sx = 0; sx < nx; ++sx)
      for (int t = 0; t < 2; ++t) {
        const size_t c = 2 * ((size_t)sy * nx + sx) + t;
        for (int k = 0; k < 6; ++k)
          if (p2map[c * 6 + k] != (2 * sy + cl.dj[t][k]) * W + 2 * sx + cl.di[t][k]) return false;
      }
  // rank of (t, k) among the cells around its node, taken at the interior square (1, 1)
  for (int t = 0; t < 2; ++t)
    for (int k = 0; k < 6; ++k) {
      const size_t c = 2 * ((size_t)1 * nx + 1) + t;
      const int node = p2map[c * 6 + k];
      int before = 0;
      for (int sy = 0; sy < 3; ++sy)
        for (int sx = 0; sx < 3; ++sx)
          for (int t2 = 0; t2 < 2; ++t2) {
            const size_t c2 = 2 * ((size_t)sy * nx + sx) + t2;
            if (c2 >= c) continue;
            for (int k2 = 0; k2 < 6; ++k2) before += p2map[c2 * 6 + k2] == node;
          }
      if (before > 5) return false;
      cl.rank[t][k] = before;
    }
  cl.nx = nx; cl.ny = ny; cl.W = W; cl.H = H;
  cl.ok = true;
  return true;
}

// is the geometry of every cell that of the first cell of its type, bit for bit?  (load_geo itself: what the kernels
// would compute.)  flag[0] != 0: not uniform; ref[2][5]: the two types' geometry
__global__ __launch_bounds__(256) void k_geo_uniform(int nc, const double* __restrict__ vx, double* __restrict__ ref,
                                                     int* __restrict__ flag) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= nc) return;
  const CellGeo g = load_geo(vx, nc, c), r = load_geo(vx, nc, c & 1);
  const bool same = g.ji00 == r.ji00 && g.ji01 == r.ji01 && g.ji10 == r.ji10 && g.ji11 == r.ji11 && g.adet == r.adet;
  if (!same) flag[0] = 1;
  if (c < 2) {
    double* o = ref + 5 * c;
    o[0] = g.ji00; o[1] = g.ji01; o[2] = g.ji10; o[3] = g.ji11; o[4] = g.adet;
  }
}
// the physical gradients and weights of the two cell types of a uniform lattice: phys() and the weight product of
// conv_cell_eval on the geometry k_geo_uniform took from the cells themselves (same function, same bits).  One thread
// per (type, q, k)
__global__ __launch_bounds__(128) void k_grad_tables(const double* __restrict__ ugeo, double* __restrict__ tab) {
  const int t = threadIdx.x;
  if (t >= 2 * 7 * 6) return;
  const int ty = t / 42, q = (t / 6) % 7, k = t % 6;
  const double* r = ugeo + 5 * ty;
  CellGeo g;
  g.ji00 = r[0]; g.ji01 = r[1]; g.ji10 = r[2]; g.ji11 = r[3]; g.adet = r[4];
  const CellGrad cg{g};
  double* o = tab + kGradTab * ty;
  cg.grad(q, k, o[(q * 6 + k) * 2], o[(q * 6 + k) * 2 + 1]);
  if (k == 0) o[84 + q] = cg.wdet(q);
}
// test hook: count the cells whose per-cell phys() gradients or weights differ from the tables in any bit
__global__ __launch_bounds__(256) void k_grad_tables_check(int nc, const double* __restrict__ vx,
                                                           const double* __restrict__ tab, int* __restrict__ bad) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= nc) return;
  const CellGeo g = load_geo(vx, nc, c);
  const CellGrad cg{g};
  const double* o = tab + kGradTab * (c & 1);
  bool same = true;
  for (int q = 0; q < 7; ++q) {
    for (int k = 0; k < 6; ++k) {
      double gx, gy;
      cg.grad(q, k, gx, gy);
      same = same && __double_as_longlong(gx) == __double_as_longlong(o[(q * 6 + k) * 2]) &&
             __double_as_longlong(gy) == __double_as_longlong(o[(q * 6 + k) * 2 + 1]);
    }
    same = same && __double_as_longlong(cg.wdet(q)) == __double_as_longlong(o[84 + q]);
  }
  if (!same) atomicAdd(bad, 1);
}
void check_uniform_geometry(hipStream_t s, MeshDev& m) {
  CellLattice& cl = m.cl;
  cl.geo_uniform = false;
  if (!cl.ok || m.dim != 2 || m.n_cells < 2) return;
  cl.ugeo.alloc(10);
  DevBuf<int> flag;
  flag.alloc(1);
  flag.zero(s);
  hipLaunchKernelGGL(k_geo_uniform, dim3((m.n_cells + 255) / 256), dim3(256), 0, s, m.n_cells, (const double*)m.vx.p,
                     cl.ugeo.p, flag.p);
  NSFEM_HIP(hipGetLastError());
  int h = 1;
  NSFEM_HIP(hipMemcpyAsync(&h, flag.p, sizeof(int), hipMemcpyDeviceToHost, s));
  NSFEM_HIP(hipStreamSynchronize(s));
  cl.geo_uniform = h == 0;
  if (cl.geo_uniform) {
    cl.gtab.alloc(2 * kGradTab);
    cl.gtab.zero(s);
    hipLaunchKernelGGL(k_grad_tables, dim3(1), dim3(128), 0, s, (const double*)cl.ugeo.p, cl.gtab.p);
    NSFEM_HIP(hipGetLastError());
  }
}
int64_t check_gradient_tables(hipStream_t s, const MeshDev& m) {
  const CellLattice& cl = m.cl;
  if (!cl.geo_uniform || !cl.gtab.p) return -1;
  DevBuf<int> bad;
  bad.alloc(1);
  bad.zero(s);
  hipLaunchKernelGGL(k_grad_tables_check, dim3((m.n_cells + 255) / 256), dim3(256), 0, s, m.n_cells,
                     (const double*)m.vx.p, (const double*)cl.gtab.p, bad.p);
  NSFEM_HIP(hipGetLastError());
  int h = -1;
  NSFEM_HIP(hipMemcpyAsync(&h, bad.p, sizeof(int), hipMemcpyDeviceToHost, s));
  NSFEM_HIP(hipStreamSynchronize(s));
  return h;
}

static bool g_jac_lattice_on = true;
static int g_jac_lattice_dbg = 0;
// tile shape: 32 x 8 squares (512 threads).  Measured at n = 512 (us per launch of the
// Newton action): 32 x 8: 48.3, 16 x 8: 50.4, 16 x 16: 50.5, 8 x 8: 55.5, 32 x 16 (1024 threads, one workgroup per CU):
// 62.7 -- the launch is bound by the latency chain of
// a wave (loads, barriers, LDS phases) at 4 waves per SIMD, not by the shape of the tile
constexpr int kJlSx = 32, kJlSy = 8;
static bool g_jac_uniform_geo = true;                 // NSFEM_JL_UNIFORM_GEO=0: always load the cell coordinates
static bool g_jac_gather = true;                      // NSFEM_JL_KERNEL=0: the round-4 kernel (variant 0), for A/B runs
void refresh_assembly_switches() {
  const char* e = std::getenv("NSFEM_JAC_LATTICE");
  g_jac_lattice_on = e ? std::atoi(e) != 0 : true;
  e = std::getenv("NSFEM_JL_UNIFORM_GEO");
  g_jac_uniform_geo = e ? std::atoi(e) != 0 : true;
  e = std::getenv("NSFEM_JL_KERNEL");
  g_jac_gather = e ? std::atoi(e) != 0 : true;
#if NSFEM_KNOCKOUTS
  e = std::getenv("NSFEM_JL_DBG");
  g_jac_lattice_dbg = e ? std::atoi(e) : 0;
#endif
}
static size_t jac_lattice_lds(const StencilDict& d, bool imex = false) {
  const size_t lp = (size_t)((d.lmax + 3) & ~3);
  const int sx = kJlSx, sy = kJlSy;
  const size_t nn = (size_t)(2 * sx + 1) * (2 * sy + 1);
  const size_t staged = 3 * nn * sizeof(double2) + (size_t)d.n_stencils * lp * (imex ? 20 : 12) + (size_t)d.n_stencils * 4 + 16;
  // variants 1, 2: sa, then the element vectors of the gather over su, sx and the tables
  return g_jac_gather ? std::max(staged, (nn + (size_t)13 * sx * sy) * sizeof(double2)) : staged;
}

bool jacobian_lattice_available(const MeshDev& m, const BlockMat& L) {
  const CellLattice& cl = m.cl;
  if (!g_jac_lattice_on || !cl.ok || m.dim != 2 || !L.dict_ready || !L.dict) return false;
  const StencilDict& d = *L.dict;
  return d.lat_w == cl.W && d.lat_h == cl.H && d.lat_r <= 2 && !d.rect && L.br == 1 && L.bc == 1 &&
         d.n_stencils <= 64 && jac_lattice_lds(d) <= (size_t)96 * 1024;
}
int jacobian_lattice_variant(const MeshDev& m) {
  if (!g_jac_gather) return 0;
  return g_jac_uniform_geo && m.cl.geo_uniform && m.cl.gtab.p ? 2 : 1;
}
int64_t jacobian_lattice_bytes(const MeshDev& m) {
  // (uniform lattices: the cell geometry comes from 10 scalar loads, no coordinate stream)
  return (int64_t)m.n_p2 * (3 * 16 + 1 + 2) + ((g_jac_uniform_geo && m.cl.geo_uniform) ? 0 : (int64_t)m.n_cells * 48);
}

// lin: 0 residual (x, mask unused; gadd = g), 1 Newton action, 2 Picard action, 3 IMEX right-hand side (ix; L = L1),
// 4 the same on a partitioned strip (mask: ghost rows -> 0), 5 / 6: 3 / 4 with the Coriolis term (ix.gam), 7 / 8: the
// residual with its Dirichlet rows and sum of squares (ix.gd, ix.tparts), 8 at u - x with the difference stored (ix.unew)
// phase 0: every tile; 1: the tile rows that read no lattice line below `safe_lo` or from `safe_hi` on (the interior of
// a partitioned strip, launched under the halo exchange); 2: the other tile rows.  jacobian_lattice_split tells
// whether phases 1 / 2 exist for the given ghost lines
static bool lattice_tile_rows(const CellLattice& cl, int gh_lo, int gh_hi, int& nty, int& r0, int& r1) {
  const int oy = 2 * (kJlSy - 1);
  nty = (cl.H + oy - 1) / oy;
  // tile row ty reads the lattice lines ty * oy - 2 ... (ty + 1) * oy
  r0 = 0;
  while (r0 < nty && r0 * oy - 2 < gh_lo) ++r0;
  r1 = nty;
  while (r1 > r0 && r1 * oy >= cl.H - gh_hi) --r1;
  return r1 > r0 && (r0 > 0 || r1 < nty);
}
bool jacobian_lattice_split(const MeshDev& m, int gh_lo, int gh_hi) {
  int nty, r0, r1;
  return m.cl.ok && lattice_tile_rows(m.cl, gh_lo, gh_hi, nty, r0, r1);
}
static bool launch_lattice_cells(hipStream_t s, const MeshDev& m, const BlockMat& L, const double* u,
                                 const double* x, double cc, int form, int lin, const uint8_t* mask,
                                 const double* gadd, double* y, int phase = 0, int gh_lo = 0, int gh_hi = 0,
                                 const ImexLatArgs* imex = nullptr) {
  const CellLattice& cl = m.cl;
  if (!jacobian_lattice_available(m, L)) return false;
  const ImexLatArgs ix = imex ? *imex : ImexLatArgs();
  const StencilDict& d = *L.dict;
  JacLatArgs a;
  a.nx = cl.nx; a.ny = cl.ny; a.W = cl.W; a.H = cl.H; a.nc = m.n_cells;
  const int sx = kJlSx, sy = kJlSy;
  const int ox = 2 * (sx - 1), oy = 2 * (sy - 1);
  a.ntx = (cl.W + ox - 1) / ox;
  a.ntiles = a.ntx * ((cl.H + oy - 1) / oy);
  a.tbase = 0; a.tsplit = a.ntiles; a.tskip = 0;
  if (phase != 0) {
    int nty, r0, r1;
    if (!lattice_tile_rows(cl, gh_lo, gh_hi, nty, r0, r1)) return false;
    if (phase == 1) {
      a.tbase = r0 * a.ntx;
      a.ntiles = (r1 - r0) * a.ntx;
      a.tsplit = a.ntiles;
    } else {
      a.ntiles = (r0 + nty - r1) * a.ntx;
      a.tsplit = r0 * a.ntx;
      a.tskip = (r1 - r0) * a.ntx;
    }
    if (a.ntiles == 0) return true;
  }
  a.lmax = d.lmax; a.lp = (d.lmax + 3) & ~3; a.n_st = d.n_stencils;
  a.dbg = g_jac_lattice_dbg;
  a.cc = cc;
  int pk[2][2] = {{0, 0}, {0, 0}};
  for (int t = 0; t < 2; ++t)
    for (int k = 0; k < 6; ++k) {
      pk[0][t] |= (cl.dj[t][k] * 3 + cl.di[t][k]) << (5 * k);
      pk[1][t] |= cl.rank[t][k] << (5 * k);
    }
  a.noff0 = pk[0][0]; a.noff1 = pk[0][1]; a.rank0 = pk[1][0]; a.rank1 = pk[1][1];
  // gather lists per node parity class: the (t, k) of that class in rank order, as offsets into the element vectors
  // [t][k][sy][sx] from the node's square: (j - dj) >> 1 = (j >> 1) - (dj >> 1) when j and dj have one parity
  for (int c = 0; c < 4; ++c) {
    int ent[6] = {-1, -1, -1, -1, -1, -1};
    for (int t = 0; t < 2; ++t)
      for (int k = 0; k < 6; ++k)
        if ((cl.di[t][k] & 1) == (c & 1) && (cl.dj[t][k] & 1) == (c >> 1)) {
          NSFEM_REQUIRE(ent[cl.rank[t][k]] < 0, "k_jac_lattice: two cells of one rank around a node");
          ent[cl.rank[t][k]] = (6 * t + k) * sx * sy - (cl.dj[t][k] >> 1) * sx - (cl.di[t][k] >> 1);
        }
    int n = 0, packed[6];
    for (int r = 0; r < 6; ++r)
      if (ent[r] >= 0) packed[n++] = ent[r] + 2 * sx;
    for (; n < 6; ++n) packed[n] = 12 * sx * sy + 2 * sx;     // the plane of -0.0
    for (int h = 0; h < 3; ++h) a.gl[c][h] = packed[2 * h] | (packed[2 * h + 1] << 16);
  }
  const int var = jacobian_lattice_variant(m);
  const bool imx = lin >= 3 && lin <= 6;
  if (imx && var != 2) return false;                // (the right-hand-side mode: uniform lattices, gradient tables)
  if (lin >= 7 && var == 0) return false;           // (the Newton frame: the gather variants)
  const size_t lds = jac_lattice_lds(d, imx);
  const int grid = ((a.ntiles + 7) / 8) * 8;
#define NSFEM_JL_V(F, LIN, SX, SY, V)                                                                       \
  do {                                                                                                      \
    static bool attr = false;                                                                               \
    if (!attr) {                                                                                            \
      NSFEM_HIP(hipFuncSetAttribute((const void*)k_jac_lattice<F, LIN, SX, SY, V>,                          \
                                    hipFuncAttributeMaxDynamicSharedMemorySize, 96 * 1024));                \
      attr = true;                                                                                          \
    }                                                                                                       \
    hipLaunchKernelGGL((k_jac_lattice<F, LIN, SX, SY, V>), dim3(grid), dim3(2 * SX * SY), lds, s, a, m.vx.p, u, \
                       x, d.sid8.p, mask, d.len.p, d.pack.p, L.dict_vals.p, gadd, y,                        \
                       (const double*)(V == 2 ? cl.gtab.p                                                   \
                                              : g_jac_uniform_geo && cl.geo_uniform ? cl.ugeo.p : nullptr), ix); \
  } while (0)
#define NSFEM_JL_T(F, LIN, SX, SY)                                                                          \
  do {                                                                                                      \
    if (var == 2) NSFEM_JL_V(F, LIN, SX, SY, 2);                                                            \
    else if (var == 1) NSFEM_JL_V(F, LIN, SX, SY, 1);                                                       \
    else NSFEM_JL_V(F, LIN, SX, SY, 0);                                                                     \
  } while (0)
#define NSFEM_JL(F, LIN) NSFEM_JL_T(F, LIN, kJlSx, kJlSy)
  if (lds > 96 * 1024) return false;
#define NSFEM_JL_F(LIN)                                                                                     \
  switch (form) {                                                                                           \
    case 0: NSFEM_JL(0, LIN); break;                                                                        \
    case 1: NSFEM_JL(1, LIN); break;                                                                        \
    case 2: NSFEM_JL(2, LIN); break;                                                                        \
    case 3: NSFEM_JL(3, LIN); break;                                                                        \
    default: throw Error(NSFEM_ERR_ARG, "unknown convective form");                                         \
  }
  if (lin == 0) { NSFEM_JL_F(0) } else if (lin == 2) { NSFEM_JL_F(2) } else if (lin == 1) { NSFEM_JL_F(1) }
#undef NSFEM_JL_T
#define NSFEM_JL_T(F, LIN, SX, SY) NSFEM_JL_V(F, LIN, SX, SY, 2)
  if (lin == 3) { NSFEM_JL_F(3) } else if (lin == 4) { NSFEM_JL_F(4) }
  else if (lin == 5) { NSFEM_JL_F(5) } else if (lin == 6) { NSFEM_JL_F(6) }
#undef NSFEM_JL_T
#define NSFEM_JL_T(F, LIN, SX, SY)                                                                          \
  do {                                                                                                      \
    if (var == 2) NSFEM_JL_V(F, LIN, SX, SY, 2);                                                            \
    else NSFEM_JL_V(F, LIN, SX, SY, 1);                                                                     \
  } while (0)
  if (lin == 7) { NSFEM_JL_F(7) } else if (lin == 8) { NSFEM_JL_F(8) }
#undef NSFEM_JL_F
#undef NSFEM_JL_T
#undef NSFEM_JL_V
#undef NSFEM_JL
  NSFEM_HIP(hipGetLastError());
  return true;
}

bool launch_jacobian_lattice(hipStream_t s, const MeshDev& m, const BlockMat& L, const double* u,
                             const double* x, double cc, int form, bool picard, const uint8_t* mask,
                             double* y, int phase, int gh_lo, int gh_hi) {
  if (!mask) return false;
  return launch_lattice_cells(s, m, L, u, x, cc, form, picard ? 2 : 1, mask, nullptr, y, phase, gh_lo, gh_hi);
}
// y = L u + g + c_c conv(u): the momentum residual before its Dirichlet rows are set.  Only on dictionaries that
// equal the assembled matrix bit for bit (the residual decides the convergence of the Newton iteration)
bool launch_residual_lattice(hipStream_t s, const MeshDev& m, const BlockMat& L, const double* u, const double* g,
                             double cc, int form, double* y) {
  if (!L.dict || !L.dict->exact || !g) return false;
  return launch_lattice_cells(s, m, L, u, u, cc, form, 0, nullptr, g, y);
}

// The residual launch with the frame of the Newton iteration around it (k_jac_lattice<FORM, 7 / 8>, variants 1, 2):
//   dx set    the pending update first: u_new = u - dx formed while staging, stored to `unew` by the thread of each
//             owned node (a second buffer: the neighbouring tiles still read the old halo), the residual taken at u_new;
//   rows      on the components flagged in `mask` the row's value u_new - g_D (`gdense`: the Dirichlet values as a dense
//             velocity vector) is stored in place of the node sum: what k_bc_residual_norm writes afterwards;
//   norm      every workgroup leaves the sum of the squares of what it stored in tparts[0 .. lattice_tile_count): one
//             entry per tile, written by every launch, summed by launch-order-independent code (host_sum_run).
// y and every entry of u_new carry the bits of the launches replaced; the sum of squares is ordered differently
int lattice_tile_count(const MeshDev& m) {
  const CellLattice& cl = m.cl;
  if (!cl.ok) return 0;
  const int ox = 2 * (kJlSx - 1), oy = 2 * (kJlSy - 1);
  return ((cl.W + ox - 1) / ox) * ((cl.H + oy - 1) / oy);
}
bool residual_frame_lattice_available(const MeshDev& m, const BlockMat& L) {
  return L.dict && L.dict->exact && jacobian_lattice_available(m, L) && jacobian_lattice_variant(m) != 0;
}
bool launch_residual_frame_lattice(hipStream_t s, const MeshDev& m, const BlockMat& L, const double* u, const double* dx,
                                   double* unew, const double* g, double cc, int form, const uint8_t* mask,
                                   const double* gdense, double* y, double* tparts) {
  if (!residual_frame_lattice_available(m, L) || !g || !mask || !gdense || !tparts || (dx && !unew)) return false;
  ImexLatArgs ix;
  ix.gd = gdense;
  ix.unew = unew;
  ix.tparts = tparts;
  return launch_lattice_cells(s, m, L, u, dx ? dx : u, cc, form, dx ? 8 : 7, mask, g, y, 0, 0, 0, &ix);
}

// rhs = -((L1 u1 + L2 u2 + g) + (b0 n1 + b1 n2)) with n1 = c_c conv(u1) stored: the right-hand side of the IMEX
// diffusion step before its Dirichlet rows are set.  Only on dictionaries that equal the assembled matrices bit for bit
// ghostmask (partitioned strips): the row mask whose value 2 flags the ghost rows -- both outputs are 0 there; phase,
// gh_lo, gh_hi: the tile-row split of launch_jacobian_lattice
bool imex_rhs_lattice_available(const MeshDev& m, const BlockMat& L1, const BlockMat& L2) {
  if (!L1.dict || !L1.dict->exact || L2.dict != L1.dict || !L1.dict_ready || !L2.dict_ready) return false;
  return jacobian_lattice_available(m, L1) && jacobian_lattice_variant(m) == 2 &&
         jac_lattice_lds(*L1.dict, true) <= (size_t)96 * 1024;
}
bool launch_imex_rhs_lattice(hipStream_t s, const MeshDev& m, const BlockMat& L1, const BlockMat& L2, const double* u1,
                             const double* u2, const double* g, double cc, int form, double b0, double b1,
                             const double* n2, double* n1, double* rhs, const uint8_t* ghostmask, int phase, int gh_lo,
                             int gh_hi, double gam) {
  if (!L1.dict || !L1.dict->exact || L2.dict != L1.dict || !L1.dict_ready || !L2.dict_ready || !g || !n1) return false;
  ImexLatArgs ix;
  ix.u2 = u2;
  ix.sval2 = L2.dict_vals.p;
  ix.n2 = n2;
  ix.n1 = n1;
  ix.b0 = b0;
  ix.b1 = b1;
  ix.gam = gam;
  // (gam == 0: the non-rotating instantiations, whatever was asked for)
  return launch_lattice_cells(s, m, L1, u1, u1, cc, form, (ghostmask ? 4 : 3) + (gam != 0.0 ? 2 : 0), ghostmask, g, rhs,
                              phase, gh_lo, gh_hi, &ix);
}

}  // namespace nsfem
