// Gradient-derived fields of the discrete solution: vorticity, divergence, shear rate, Q-criterion, the velocity
// gradient itself, pressure gradient and the gradient of the transported scalar -- per cell (means), per cell vertex
// (DG1 data) or recovered at the P2 nodes -- from ONE element-kernel launch for every quantity of a mask.
//
// Replaces the get_state copy and the numpy einsums of ProblemBase._cell_gradients / _compute_vorticity /
// _compute_pressure_gradient (which stay, as the host yardstick), and adds the quantities a viewer contours in the
// Taylor-Green, channel and LES runs.  The shape of k_vol_functionals: one thread per cell (grid-stride), SoA cell data
// read coalesced, the 6 / 10 nodal velocities, 3 / 4 nodal pressures and 6 / 10 nodal scalar values gathered once,
// geometry from load_geo / load_geo3.
//
// G_ab = d_b u_a of a P2 velocity is LINEAR on an affine cell: the kernel forms it at the dim + 1 vertices (the
// reference gradients of the P2 basis at a vertex are the constants 3, -1, 4, 0 times grad lambda: no table, no
// load), and every other point of the cell is a barycentric combination of those -- an edge midpoint 1/2 (G_a + G_b),
// a point of the degree-5 rule sum_v lambda_v(q) G_v with the lambda_v(q) of the rule's own phi1 table.  That keeps
// the live state of the 3D velocity-gradient path at 4 x 9 doubles once the 30 nodal values are consumed.
//
// NODE centring without atomics: the element kernel stores |K| q (and |K|) node-sorted through m.ndst into planes of a
// buffer of the context's own (one plane per component: the stores of a wave are as coalesced as the node-sorted
// order allows), k_derived_gather sums each run m.nptr[n] .. m.nptr[n + 1] in ascending cell order and divides.  Same
// state, same bytes.  m.rbuf, m.ebuf and the state slots are never written.
#include "cell_geometry.hpp"
#include "element_front.hpp"

namespace nsfem {

// weights and barycentric coordinates of the degree-5 rules (7 / 15 points): copies of w and phi1 of the tables the
// assembly kernels use, filled by the same fill_quad_tables / fill_quad_tables_3d.  A __constant__ symbol belongs to the
// device, not to a context: BOTH halves are filled by every upload (nsfem_create), so contexts of either dimension
// that live side by side always find their rule
struct DerivedTables {
  double w2[7], l2[7][3];
  double w3[15], l3[15][4];
};
__constant__ DerivedTables c_dq;

void upload_derived_tables() {
  DerivedTables d;
  QuadTables t;
  fill_quad_tables(t);
  for (int q = 0; q < 7; ++q) {
    d.w2[q] = t.w[q];
    for (int i = 0; i < 3; ++i) d.l2[q][i] = t.phi1[q][i];
  }
  QuadTables3 t3;
  fill_quad_tables_3d(t3);
  for (int q = 0; q < 15; ++q) {
    d.w3[q] = t3.w[q];
    for (int i = 0; i < 4; ++i) d.l3[q][i] = t3.phi1[q][i];
  }
  NSFEM_HIP(hipMemcpyToSymbol(HIP_SYMBOL(c_dq), &d, sizeof(DerivedTables)));
}

// ---- reference gradients of the P2 basis at vertex v, as compile-time constants (the loops over v, k, b are fully
// unrolled: a zero entry costs nothing)
// d lambda_i / d xi_b
__host__ __device__ constexpr double dlam(int i, int b) { return i == 0 ? -1.0 : (i - 1 == b ? 1.0 : 0.0); }
// d phi_k / d xi_b at vertex v: vertex functions (4 lambda_k - 1) grad lambda_k, edge functions
// 4 (lambda_a grad lambda_b + lambda_b grad lambda_a), a and b the ends of the edge (edge_end, element_front.hpp)
template <int DIM>
__host__ __device__ constexpr double dphi2_at_vertex(int v, int k, int b) {
  if (k <= DIM) return (k == v ? 3.0 : -1.0) * dlam(k, b);
  const int ea = edge_end<DIM>(k - DIM - 1, 0), eb = edge_end<DIM>(k - DIM - 1, 1);
  return 4.0 * ((ea == v ? 1.0 : 0.0) * dlam(eb, b) + (eb == v ? 1.0 : 0.0) * dlam(ea, b));
}

// physical gradient of a reference gradient, both dimensions
__device__ __forceinline__ void phys_grad(const CellGeo& g, const double (&dr)[2], double (&out)[2]) {
  phys(g, dr[0], dr[1], out[0], out[1]);
}
__device__ __forceinline__ void phys_grad(const CellGeo3& g, const double (&dr)[3], double (&out)[3]) {
  phys3(g, dr, out);
}

// out[v][b] = d_b f at vertex v of the P2 function with the nodal values f[k]
template <int DIM, class Geo>
__device__ __forceinline__ void p2_vertex_gradients(const Geo& g, const double (&f)[DIM == 2 ? 6 : 10],
                                                    double (&out)[DIM + 1][DIM]) {
  constexpr int N2 = DIM == 2 ? 6 : 10;
#pragma unroll
  for (int v = 0; v <= DIM; ++v) {
    double dr[DIM];
#pragma unroll
    for (int b = 0; b < DIM; ++b) {
      double t = 0.0;
#pragma unroll
      for (int k = 0; k < N2; ++k) {
        const double d = dphi2_at_vertex<DIM>(v, k, b);
        if (d != 0.0) t += d * f[k];
      }
      dr[b] = t;
    }
    phys_grad(g, dr, out[v]);
  }
}

// gamma = sqrt(2 S:S), S = (G + G^T) / 2 -- with s = G + G^T: sqrt(1/2 sum_ab s_ab^2), as k_visc_var_cell
template <int DIM>
__device__ __forceinline__ double shear_rate(const double (&G)[DIM][DIM]) {
  double t = 0.0;
#pragma unroll
  for (int a = 0; a < DIM; ++a) {
    const double d = 2.0 * G[a][a];
    t += d * d;
#pragma unroll
    for (int b = a + 1; b < DIM; ++b) {
      const double s = G[a][b] + G[b][a];
      t += 2.0 * (s * s);
    }
  }
  return sqrt(0.5 * t);
}

// Q = (|W|^2 - |S|^2) / 2 = -1/2 G_ab G_ba
template <int DIM>
__device__ __forceinline__ double q_criterion(const double (&G)[DIM][DIM]) {
  double t = 0.0;
#pragma unroll
  for (int a = 0; a < DIM; ++a)
#pragma unroll
    for (int b = 0; b < DIM; ++b) t += G[a][b] * G[b][a];
  return -0.5 * t;
}

// the requested quantities of one point, ascending id order: st(column, wgt * value)
template <int DIM, class Store>
__device__ __forceinline__ void derived_emit(unsigned mask, const double (&G)[DIM][DIM], double gamma, double q,
                                             const double (&gp)[DIM], const double (&gT)[DIM], double wgt,
                                             Store&& st) {
  int col = 0;
  if (mask & (1u << NSFEM_DERIVED_VORTICITY)) {
    if constexpr (DIM == 2) {
      st(col++, wgt * (G[1][0] - G[0][1]));
    } else {
      st(col++, wgt * (G[2][1] - G[1][2]));
      st(col++, wgt * (G[0][2] - G[2][0]));
      st(col++, wgt * (G[1][0] - G[0][1]));
    }
  }
  if (mask & (1u << NSFEM_DERIVED_DIVERGENCE)) {
    double t = G[0][0];
#pragma unroll
    for (int a = 1; a < DIM; ++a) t += G[a][a];
    st(col++, wgt * t);
  }
  if (mask & (1u << NSFEM_DERIVED_SHEAR_RATE)) st(col++, wgt * gamma);
  if (mask & (1u << NSFEM_DERIVED_Q_CRITERION)) st(col++, wgt * q);
  if (mask & (1u << NSFEM_DERIVED_VELOCITY_GRADIENT)) {
#pragma unroll
    for (int a = 0; a < DIM; ++a)
#pragma unroll
      for (int b = 0; b < DIM; ++b) st(col++, wgt * G[a][b]);
  }
  if (mask & (1u << NSFEM_DERIVED_PRESSURE_GRADIENT)) {
#pragma unroll
    for (int a = 0; a < DIM; ++a) st(col++, wgt * gp[a]);
  }
  if (mask & (1u << NSFEM_DERIVED_SCALAR_GRADIENT)) {
#pragma unroll
    for (int a = 0; a < DIM; ++a) st(col++, wgt * gT[a]);
  }
}

// CENTER = NSFEM_DERIVED_CELL:   out [nc][ncomp], the cell means by the degree-5 rule
//          NSFEM_DERIVED_VERTEX: out [nc][DIM + 1][ncomp]
//          NSFEM_DERIVED_NODE:   out = ncomp + 1 planes of N2 * nc doubles, plane j at out + j * N2 * nc: |K| q_j of
//                                (cell, local node i) at position ndst[i][cell] of plane j, |K| in plane ncomp
// p / T are read only when the mask asks for their gradient.
template <int DIM, int CENTER>
__global__ __launch_bounds__(256) void k_derived_cell(int nc, const double* __restrict__ vx,
                                                      const int32_t* __restrict__ p2,
                                                      const int32_t* __restrict__ p1,
                                                      const double* __restrict__ u,
                                                      const double* __restrict__ p,
                                                      const double* __restrict__ T, unsigned mask, int ncomp,
                                                      const int32_t* __restrict__ ndst, double* __restrict__ out) {
  constexpr int N2 = DIM == 2 ? 6 : 10, N1 = DIM + 1, NQ = DIM == 2 ? 7 : 15;
  const bool want_p = (mask & (1u << NSFEM_DERIVED_PRESSURE_GRADIENT)) != 0;
  const bool want_T = (mask & (1u << NSFEM_DERIVED_SCALAR_GRADIENT)) != 0;
  for (int c = blockIdx.x * blockDim.x + threadIdx.x; c < nc; c += gridDim.x * blockDim.x) {
    typename std::conditional<DIM == 2, CellGeo, CellGeo3>::type g;
    if constexpr (DIM == 2) g = load_geo(vx, nc, c);
    else g = load_geo3(vx, nc, c);
    // ---- vertex gradients: Gv[v][a][b] = d_b u_a, gTv[v][b] = d_b T, gp[b] = d_b p (constant)
    double Gv[N1][DIM][DIM], gTv[N1][DIM], gp[DIM];
    {
      size_t node[N2];
#pragma unroll
      for (int k = 0; k < N2; ++k) node[k] = (size_t)p2[(size_t)k * nc + c];
#pragma unroll
      for (int a = 0; a < DIM; ++a) {
        double f[N2], ga[N1][DIM];
#pragma unroll
        for (int k = 0; k < N2; ++k) f[k] = u[DIM * node[k] + a];
        p2_vertex_gradients<DIM>(g, f, ga);
#pragma unroll
        for (int v = 0; v < N1; ++v)
#pragma unroll
          for (int b = 0; b < DIM; ++b) Gv[v][a][b] = ga[v][b];
      }
      if (want_T) {
        double f[N2];
#pragma unroll
        for (int k = 0; k < N2; ++k) f[k] = T[node[k]];
        p2_vertex_gradients<DIM>(g, f, gTv);
      } else {
#pragma unroll
        for (int v = 0; v < N1; ++v)
#pragma unroll
          for (int b = 0; b < DIM; ++b) gTv[v][b] = 0.0;
      }
    }
    if (want_p) {
      // sum_i p_i grad lambda_i, reference gradients (-1, .., -1), e_1, .., e_DIM
      const double p0 = p[(size_t)p1[c]];
      double dr[DIM];
#pragma unroll
      for (int b = 0; b < DIM; ++b) dr[b] = p[(size_t)p1[(size_t)(b + 1) * nc + c]] - p0;
      phys_grad(g, dr, gp);
    } else {
#pragma unroll
      for (int b = 0; b < DIM; ++b) gp[b] = 0.0;
    }

    if constexpr (CENTER == NSFEM_DERIVED_CELL) {
      // means by the rule: G, grad T (linear: exact), Q (quadratic: exact), gamma (the rule is its definition)
      double mG[DIM][DIM], mT[DIM], mq = 0.0, mgam = 0.0, wsum = 0.0;
#pragma unroll
      for (int a = 0; a < DIM; ++a) {
        mT[a] = 0.0;
#pragma unroll
        for (int b = 0; b < DIM; ++b) mG[a][b] = 0.0;
      }
      // (not unrolled: the tables of all points at once do not fit the scalar registers)
#pragma unroll 1
      for (int q = 0; q < NQ; ++q) {
        double lam[N1];
#pragma unroll
        for (int v = 0; v < N1; ++v) lam[v] = DIM == 2 ? c_dq.l2[q][v < 3 ? v : 0] : c_dq.l3[q][v];
        const double w = DIM == 2 ? c_dq.w2[q] : c_dq.w3[q];
        double G[DIM][DIM];
#pragma unroll
        for (int a = 0; a < DIM; ++a)
#pragma unroll
          for (int b = 0; b < DIM; ++b) {
            double t = lam[0] * Gv[0][a][b];
#pragma unroll
            for (int v = 1; v < N1; ++v) t += lam[v] * Gv[v][a][b];
            G[a][b] = t;
            mG[a][b] += w * t;
          }
#pragma unroll
        for (int b = 0; b < DIM; ++b) {
          double t = lam[0] * gTv[0][b];
#pragma unroll
          for (int v = 1; v < N1; ++v) t += lam[v] * gTv[v][b];
          mT[b] += w * t;
        }
        mq += w * q_criterion<DIM>(G);
        mgam += w * shear_rate<DIM>(G);
        wsum += w;
      }
      const double inv = 1.0 / wsum;
#pragma unroll
      for (int a = 0; a < DIM; ++a) {
        mT[a] *= inv;
#pragma unroll
        for (int b = 0; b < DIM; ++b) mG[a][b] *= inv;
      }
      double* o = out + (size_t)c * ncomp;
      derived_emit<DIM>(mask, mG, mgam * inv, mq * inv, gp, mT, 1.0, [&](int col, double v) { o[col] = v; });
    } else if constexpr (CENTER == NSFEM_DERIVED_VERTEX) {
#pragma unroll
      for (int v = 0; v < N1; ++v) {
        double* o = out + ((size_t)c * N1 + v) * ncomp;
        derived_emit<DIM>(mask, Gv[v], shear_rate<DIM>(Gv[v]), q_criterion<DIM>(Gv[v]), gp, gTv[v], 1.0,
                          [&](int col, double val) { o[col] = val; });
      }
    } else {
      const size_t plane = (size_t)N2 * nc;
      const double vol = DIM == 2 ? 0.5 * g.adet : g.adet / 6.0;   // |K|
#pragma unroll
      for (int i = 0; i < N2; ++i) {
        double* o = out + (size_t)ndst[(size_t)i * nc + c];
        o[(size_t)ncomp * plane] = vol;
        if (i < N1) {
          const int v = i < N1 ? i : 0;
          derived_emit<DIM>(mask, Gv[v], shear_rate<DIM>(Gv[v]), q_criterion<DIM>(Gv[v]), gp, gTv[v], vol,
                            [&](int col, double val) { o[(size_t)col * plane] = val; });
        } else {
          // edge midpoint: 1/2 (value at one end + value at the other)
          const int e = i >= N1 ? i - N1 : 0;
          const int ea = edge_end<DIM>(e, 0), eb = edge_end<DIM>(e, 1);
          double G[DIM][DIM], gT[DIM];
#pragma unroll
          for (int a = 0; a < DIM; ++a) {
            gT[a] = 0.5 * (gTv[ea][a] + gTv[eb][a]);
#pragma unroll
            for (int b = 0; b < DIM; ++b) G[a][b] = 0.5 * (Gv[ea][a][b] + Gv[eb][a][b]);
          }
          derived_emit<DIM>(mask, G, shear_rate<DIM>(G), q_criterion<DIM>(G), gp, gT, vol,
                            [&](int col, double val) { o[(size_t)col * plane] = val; });
        }
      }
    }
  }
}

// out[n][j] = (sum of plane j over the run nptr[n] .. nptr[n + 1]) / (sum of the |K| plane over the same run), both in
// ascending cell order; thread t works on component t / n_nodes of node t % n_nodes (neighbouring lanes read
// neighbouring runs of one plane)
__global__ __launch_bounds__(256) void k_derived_gather(int64_t n_nodes, int ncomp, const int32_t* __restrict__ nptr,
                                                        const double* __restrict__ planes, size_t plane,
                                                        double* __restrict__ out) {
#pragma clang fp contract(off)
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < n_nodes * ncomp;
       t += (int64_t)gridDim.x * blockDim.x) {
    const int j = (int)(t / n_nodes);
    const int64_t n = t % n_nodes;
    const double* q = planes + (size_t)j * plane;
    const double* wk = planes + (size_t)ncomp * plane;
    double s = 0.0, w = 0.0;
    const int e = nptr[n + 1];
    for (int k = nptr[n]; k < e; ++k) {
      s += q[k];
      w += wk[k];
    }
    out[(size_t)n * ncomp + j] = s / w;
  }
}

int64_t derived_work_doubles(const MeshDev& m, int center, int ncomp) {
  const int64_t n2 = m.dim == 2 ? 6 : 10;
  switch (center) {
    case NSFEM_DERIVED_CELL: return (int64_t)m.n_cells * ncomp;
    case NSFEM_DERIVED_VERTEX: return (int64_t)m.n_cells * (m.dim + 1) * ncomp;
    default: return (int64_t)m.n_p2 * ncomp + (int64_t)(ncomp + 1) * n2 * m.n_cells;
  }
}

const double* launch_derived_fields(hipStream_t s, const MeshDev& m, const double* u, const double* p, const double* T,
                                    unsigned mask, int center, int ncomp, double* work) {
  const int grid = (int)std::min<int64_t>(((int64_t)m.n_cells + 255) / 256, 4096);
  // NODE: the result first, the element planes behind it
  double* cell_out = center == NSFEM_DERIVED_NODE ? work + (size_t)m.n_p2 * ncomp : work;
#define NSFEM_DERIVED(D, C)                                                                                       \
  hipLaunchKernelGGL((k_derived_cell<D, C>), dim3(grid), dim3(256), 0, s, m.n_cells, m.vx.p, m.p2.p, m.p1.p, u, p, T, \
                     mask, ncomp, m.ndst.p, cell_out)
  if (m.dim == 3) {
    if (center == NSFEM_DERIVED_CELL) NSFEM_DERIVED(3, NSFEM_DERIVED_CELL);
    else if (center == NSFEM_DERIVED_VERTEX) NSFEM_DERIVED(3, NSFEM_DERIVED_VERTEX);
    else NSFEM_DERIVED(3, NSFEM_DERIVED_NODE);
  } else {
    if (center == NSFEM_DERIVED_CELL) NSFEM_DERIVED(2, NSFEM_DERIVED_CELL);
    else if (center == NSFEM_DERIVED_VERTEX) NSFEM_DERIVED(2, NSFEM_DERIVED_VERTEX);
    else NSFEM_DERIVED(2, NSFEM_DERIVED_NODE);
  }
#undef NSFEM_DERIVED
  NSFEM_HIP(hipGetLastError());
  if (center == NSFEM_DERIVED_NODE) {
    const int64_t n = (int64_t)m.n_p2 * ncomp;
    const int ggrid = (int)std::min<int64_t>((n + 255) / 256, 8192);
    hipLaunchKernelGGL(k_derived_gather, dim3(ggrid), dim3(256), 0, s, (int64_t)m.n_p2, ncomp, m.nptr.p, cell_out,
                       (size_t)(m.dim == 2 ? 6 : 10) * m.n_cells, work);
    NSFEM_HIP(hipGetLastError());
  }
  return work;
}

}  // namespace nsfem
