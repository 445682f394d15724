// Immersed bodies (nsfem_set_bodies): volume, force and torque of every body from the penalisation term itself,
//   vol_s = int chi_s,   F_s = (1/eta) int chi_s (u - u_s),   T_s = (1/eta) int chi_s (x - c_s) x (u - u_s),
// with the rule, the points x_q, the masks and the "largest chi wins" rule of the element kernels k_penal_cell /
// k3_penal_cell (bodies.hpp): a point counts for its winning body only, so sum_s F_(s,a) = sum_i B(u)_(i,a).
//
// Shape of k_vol_functionals (functionals.hip): one thread per cell, grid-stride; row blockIdx.y of the grid integrates
// body blockIdx.y and skips every cell its support cannot reach, so the accumulators are the 4 / 7 numbers of one body
// and stay in registers.  Reduction without atomics: a thread adds its cells in ascending order, a wave folds its
// lanes with a fixed xor-shuffle tree, the 4 waves of a workgroup are added in wave order, k_fold_partials folds the
// kBodyParts partials of a number in a fixed order.  Same state, same bytes.
#include "cell_geometry.hpp"
#include "bodies.hpp"
#include "element_front.hpp"

namespace nsfem {

NSFEM_FRONT_TABLES(c_bq, c_bq3)
void upload_body_tables(int dim) { upload_front_tables(dim); }

// parts[(s NQ + j) kBodyParts + block]: number j of body s over the cells of the block's threads;
// j = 0 volume, 1 .. DIM force, then the torque about c_s (2D: z component; 3D: 3 components)
template <int DIM, bool SMOOTH>
__global__ __launch_bounds__(256) void k_penal_forces(int nc, const double* __restrict__ vx,
                                                      const int32_t* __restrict__ p2,
                                                      const double* __restrict__ u, const BodyTable bt,
                                                      double* __restrict__ parts) {
  constexpr int N2 = DIM == 2 ? 6 : 10, NQ = DIM == 2 ? 7 : 15, NO = DIM == 2 ? 4 : 7;
  __shared__ double sh[4 * NO];
  const int s = blockIdx.y;
  double acc[NO];
#pragma unroll
  for (int j = 0; j < NO; ++j) acc[j] = 0.0;
  for (int c = blockIdx.x * blockDim.x + threadIdx.x; c < nc; c += gridDim.x * blockDim.x) {
    double xv[DIM + 1][DIM];
#pragma unroll
    for (int v = 0; v <= DIM; ++v)
#pragma unroll
      for (int d = 0; d < DIM; ++d) xv[v][d] = vx[(size_t)(DIM * v + d) * nc + c];
    if (body_misses_cell<DIM>(bt, s, xv)) continue;
    double adet;
    if constexpr (DIM == 2) adet = load_geo(vx, nc, c).adet;
    else adet = load_geo3(vx, nc, c).adet;
    double uu[N2][DIM];
    gather_p2_vector<DIM, DIM>(p2, nc, c, u, uu);
    for (int q = 0; q < NQ; ++q) {
      double x[DIM];
#pragma unroll
      for (int a = 0; a < DIM; ++a) {
        double xa = 0.0;
#pragma unroll
        for (int v = 0; v <= DIM; ++v) xa += (DIM == 2 ? c_bq.phi1[q][v] : c_bq3.phi1[q][v]) * xv[v][a];
        x[a] = xa;
      }
      int win;
      const double chi = body_winner<DIM, SMOOTH>(bt, x, win);
      if (!(chi > 0.0) || win != s) continue;
      double us[DIM], f[DIM], r[DIM];
      body_velocity<DIM>(bt, s, x, us);
      const double w = (DIM == 2 ? c_bq.w[q] : c_bq3.w[q]) * adet * chi;
#pragma unroll
      for (int a = 0; a < DIM; ++a) {
        double uq = 0.0;
#pragma unroll
        for (int k = 0; k < N2; ++k) uq += (DIM == 2 ? c_bq.phi2[q][k] : c_bq3.phi2[q][k]) * uu[k][a];
        f[a] = w * bt.inv_eta * (uq - us[a]);
        r[a] = x[a] - bt.centre[s][a];
        acc[1 + a] += f[a];
      }
      acc[0] += w;
      if constexpr (DIM == 2) {
        acc[3] += r[0] * f[1] - r[1] * f[0];
      } else {
        acc[4] += r[1] * f[2] - r[2] * f[1];
        acc[5] += r[2] * f[0] - r[0] * f[2];
        acc[6] += r[0] * f[1] - r[1] * f[0];
      }
    }
  }
  block_sum_fixed<NO>(acc, sh);
  store_block_partials<NO>(sh, parts, (size_t)s * NO, gridDim.x, blockIdx.x);
}

// Heated bodies (nsfem_set_body_temperatures): per body the volume int chi_s, the heat rate
// Q_s = (1/eta_T) int chi_s theta_s (T - T_s) the body takes from the fluid (0 for a passive body) and int chi_s T,
// with the rule, the points and the winner of k_scalar_conv_cell<FORM, PENAL> / k3_scalar_conv_cell: a point counts
// for its winning body only, so sum_s Q_s = sum_i H(T)_i.  Shape and reduction of k_penal_forces.
// parts[(s 3 + j) kBodyParts + block]
template <int DIM, bool SMOOTH>
__global__ __launch_bounds__(256) void k_body_heat(int nc, const double* __restrict__ vx,
                                                   const int32_t* __restrict__ p2, const double* __restrict__ T,
                                                   const BodyTable bt, const ThermalTable th,
                                                   double* __restrict__ parts) {
  constexpr int N2 = DIM == 2 ? 6 : 10, NQ = DIM == 2 ? 7 : 15, NO = 3;
  __shared__ double sh[4 * NO];
  const int s = blockIdx.y;
  const double scale = th.flag[s] != 0 ? th.inv_eta : 0.0, ts = th.temperature[s];
  double acc[NO] = {0.0, 0.0, 0.0};
  for (int c = blockIdx.x * blockDim.x + threadIdx.x; c < nc; c += gridDim.x * blockDim.x) {
    double xv[DIM + 1][DIM];
#pragma unroll
    for (int v = 0; v <= DIM; ++v)
#pragma unroll
      for (int d = 0; d < DIM; ++d) xv[v][d] = vx[(size_t)(DIM * v + d) * nc + c];
    if (body_misses_cell<DIM>(bt, s, xv)) continue;
    double adet;
    if constexpr (DIM == 2) adet = load_geo(vx, nc, c).adet;
    else adet = load_geo3(vx, nc, c).adet;
    double t[N2];
    gather_p2_scalar<DIM>(p2, nc, c, T, t);
    for (int q = 0; q < NQ; ++q) {
      double x[DIM];
#pragma unroll
      for (int a = 0; a < DIM; ++a) {
        double xa = 0.0;
#pragma unroll
        for (int v = 0; v <= DIM; ++v) xa += (DIM == 2 ? c_bq.phi1[q][v] : c_bq3.phi1[q][v]) * xv[v][a];
        x[a] = xa;
      }
      int win;
      const double chi = body_winner<DIM, SMOOTH>(bt, x, win);
      if (!(chi > 0.0) || win != s) continue;
      double tq = 0.0;
#pragma unroll
      for (int k = 0; k < N2; ++k) tq += (DIM == 2 ? c_bq.phi2[q][k] : c_bq3.phi2[q][k]) * t[k];
      const double w = (DIM == 2 ? c_bq.w[q] : c_bq3.w[q]) * adet * chi;
      acc[0] += w;
      acc[1] += w * scale * (tq - ts);
      acc[2] += w * tq;
    }
  }
  block_sum_fixed<NO>(acc, sh);
  store_block_partials<NO>(sh, parts, (size_t)s * NO, gridDim.x, blockIdx.x);
}

void launch_penalty_forces(hipStream_t s, const MeshDev& m, const double* u, const BodyTable& bt, double* parts,
                           double* out) {
  static_assert(kBodyParts % 64 == 0, "k_fold_partials gives every lane the same number of partials");
  NSFEM_REQUIRE(bt.n > 0, "immersed bodies: no body set");
  const dim3 grid(kBodyParts, bt.n), block(256);
  const bool smooth = bt.eps > 0.0;
  if (m.dim == 3) {
    if (smooth) hipLaunchKernelGGL((k_penal_forces<3, true>), grid, block, 0, s, m.n_cells, m.vx.p, m.p2.p, u, bt, parts);
    else hipLaunchKernelGGL((k_penal_forces<3, false>), grid, block, 0, s, m.n_cells, m.vx.p, m.p2.p, u, bt, parts);
  } else {
    if (smooth) hipLaunchKernelGGL((k_penal_forces<2, true>), grid, block, 0, s, m.n_cells, m.vx.p, m.p2.p, u, bt, parts);
    else hipLaunchKernelGGL((k_penal_forces<2, false>), grid, block, 0, s, m.n_cells, m.vx.p, m.p2.p, u, bt, parts);
  }
  NSFEM_HIP(hipGetLastError());
  launch_fold_partials(s, bt.n * body_numbers(m.dim), kBodyParts, parts, out);
}

void launch_body_heat(hipStream_t s, const MeshDev& m, const double* T, const BodyTable& bt, const ThermalTable& th,
                      double* parts, double* out) {
  NSFEM_REQUIRE(bt.n > 0 && th.n == bt.n, "heated bodies: no temperatures set for the bodies");
  const dim3 grid(kBodyParts, bt.n), block(256);
  const bool smooth = bt.eps > 0.0;
  if (m.dim == 3) {
    if (smooth) hipLaunchKernelGGL((k_body_heat<3, true>), grid, block, 0, s, m.n_cells, m.vx.p, m.p2.p, T, bt, th, parts);
    else hipLaunchKernelGGL((k_body_heat<3, false>), grid, block, 0, s, m.n_cells, m.vx.p, m.p2.p, T, bt, th, parts);
  } else {
    if (smooth) hipLaunchKernelGGL((k_body_heat<2, true>), grid, block, 0, s, m.n_cells, m.vx.p, m.p2.p, T, bt, th, parts);
    else hipLaunchKernelGGL((k_body_heat<2, false>), grid, block, 0, s, m.n_cells, m.vx.p, m.p2.p, T, bt, th, parts);
  }
  NSFEM_HIP(hipGetLastError());
  launch_fold_partials(s, bt.n * 3, kBodyParts, parts, out);
}

}  // namespace nsfem
