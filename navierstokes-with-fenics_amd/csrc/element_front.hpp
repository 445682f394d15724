// The front of a device-side diagnostic: what every post-processing kernel does before its own integrand and after
// its own accumulation, written once.  boundary.hip, wall.hip, functionals.hip, bodies.hip, points.hip, statistics.hip
// and derived.hip start from here, and so does the next diagnostic:
//
//   edge_end<DIM>                 the UFC edge order of the P2 edge nodes -- the only place it is written
//   p2_at<DIM>                    P2 values (and physical gradients) at a barycentric point
//   FacetFront<DIM>, facet_front  vertex coordinates, gradients of the barycentric coordinates, |T| d!, the outward unit
//                                 normal and the measure of a facet of a cell; facet_rule_point: the points of its rule
//                                 (functions in 2D, macros expanded in the kernel in 3D)
//   gather_p2_vector / gather_p2_scalar / gather_p1
//                                 the nodal values of a cell through the dof maps
//   block_sum_fixed<N>            the workgroup sum in a fixed order, block_total / store_block_partials / block_sum_all
//                                 what a kernel does with it (the second level is k_fold_partials, functionals.hip)
//   NSFEM_FRONT_TABLES            this translation unit's __constant__ copy of the degree-5 rules and its uploader
//
// "Same state, same bytes" rests on these orders: the lanes of a wave by the xor-shuffle tree 32, 16, .., 1, the four
// waves of a workgroup as ((s0 + s1) + s2) + s3, the partials of a number lane-consecutive in index order.
#pragma once
#include "nsfem_internal.hpp"

namespace nsfem {

// ---------------------------------------------------------------------------------------------- P2 local numbering
// the two vertices of edge node e (local node DIM + 1 + e): UFC order as fem_mesh.Mesh, fill_quad_tables and
// fill_quad_tables_3d -- triangle e(12), e(02), e(01); tetrahedron e(23), e(13), e(12), e(03), e(02), e(01)
template <int DIM>
__host__ __device__ constexpr int edge_end(int e, int which) {
  if (DIM == 2) {
    constexpr int pr[3][2] = {{1, 2}, {0, 2}, {0, 1}};
    return pr[e][which];
  } else {
    constexpr int pr[6][2] = {{2, 3}, {1, 3}, {1, 2}, {0, 3}, {0, 2}, {0, 1}};
    return pr[e][which];
  }
}

// P2 basis values at the barycentric point lam[]: vertices, then the edge nodes
template <int DIM>
__device__ __forceinline__ void p2_at(const double* lam, double* phi) {
  constexpr int NV = DIM + 1, NE = DIM == 2 ? 3 : 6;
#pragma unroll
  for (int v = 0; v < NV; ++v) phi[v] = lam[v] * (2.0 * lam[v] - 1.0);
#pragma unroll
  for (int e = 0; e < NE; ++e) phi[NV + e] = 4.0 * lam[edge_end<DIM>(e, 0)] * lam[edge_end<DIM>(e, 1)];
}

// ... and the physical gradients, gl[v][d] = d lambda_v / d x_d
template <int DIM>
__device__ __forceinline__ void p2_at(const double* lam, const double (*gl)[3], double* phi, double (*dphi)[3]) {
  constexpr int NV = DIM + 1, NE = DIM == 2 ? 3 : 6;
#pragma unroll
  for (int v = 0; v < NV; ++v) {
    phi[v] = lam[v] * (2.0 * lam[v] - 1.0);
#pragma unroll
    for (int d = 0; d < DIM; ++d) dphi[v][d] = (4.0 * lam[v] - 1.0) * gl[v][d];
  }
#pragma unroll
  for (int e = 0; e < NE; ++e) {
    const int a = edge_end<DIM>(e, 0), b = edge_end<DIM>(e, 1);
    phi[NV + e] = 4.0 * lam[a] * lam[b];
#pragma unroll
    for (int d = 0; d < DIM; ++d) dphi[NV + e][d] = 4.0 * (lam[a] * gl[b][d] + lam[b] * gl[a][d]);
  }
}

// ------------------------------------------------------------------------------------------------------ facet front
// the facet opposite vertex `opp` of cell c: filled by facet_front in 2D, by NSFEM_FACET_FRONT_3D (below) in 3D
template <int DIM>
struct FacetFront {
  double x[DIM + 1][3];    // vertex coordinates (x[v][DIM ..] not written)
  double gl[DIM + 1][3];   // gradients of the barycentric coordinates
  double vol;              // |T| d!
  double nrm[3];           // outward unit normal
  double area;             // |f|
};

__device__ __forceinline__ void facet_front(const double* __restrict__ vx, int nc, int c, int opp, FacetFront<2>& F) {
  double(&x)[3][3] = F.x;
  double(&gl)[3][3] = F.gl;
#pragma unroll
  for (int v = 0; v < 3; ++v)
#pragma unroll
    for (int d = 0; d < 2; ++d) x[v][d] = vx[(size_t)(2 * v + d) * nc + c];
  // rows of J^-1 (J = [x1-x0, x2-x0]) for lambda_1, lambda_2; lambda_0 = 1 - sum
  const double a00 = x[1][0] - x[0][0], a01 = x[2][0] - x[0][0];
  const double a10 = x[1][1] - x[0][1], a11 = x[2][1] - x[0][1];
  const double det = a00 * a11 - a01 * a10, id = 1.0 / det;
  gl[1][0] = a11 * id;  gl[1][1] = -a01 * id;
  gl[2][0] = -a10 * id; gl[2][1] = a00 * id;
  gl[0][0] = -gl[1][0] - gl[2][0];
  gl[0][1] = -gl[1][1] - gl[2][1];
  F.vol = fabs(det);
  // grad lambda_opp points inward, |f| = |grad lambda_opp| * d * |T| = |grad lambda_opp| vol / (d-1)!
  double gn = 0.0;
#pragma unroll
  for (int d = 0; d < 3; ++d) F.nrm[d] = 0.0;
#pragma unroll
  for (int v = 0; v < 3; ++v)
    if (v == opp) {
#pragma unroll
      for (int d = 0; d < 2; ++d) F.nrm[d] = -gl[v][d];
    }
#pragma unroll
  for (int d = 0; d < 2; ++d) gn += F.nrm[d] * F.nrm[d];
  gn = sqrt(gn);
#pragma unroll
  for (int d = 0; d < 2; ++d) F.nrm[d] /= gn;
  F.area = gn * F.vol / 1.0;
}

// point q of the 2-point Gauss rule on the edge opposite `opp` (equal weights |f| / 2) in the barycentric coordinates
// of the cell: those of the edge's own vertices, lam[opp] = 0.  (3D: the 3 edge midpoints of the face, in the kernels.)
__device__ __forceinline__ void facet_rule_point(int q, int opp, double (&lam)[3]) {
  const double g2 = 0.21132486540518713;              // (1 - 1/sqrt(3)) / 2
  double fl[3];                                       // barycentric point inside the facet
  fl[0] = q == 0 ? g2 : 1.0 - g2;
  fl[1] = 1.0 - fl[0];
  fl[2] = 0.0;
  int t = 0;
#pragma unroll
  for (int v = 0; v <= 2; ++v) {
    if (v == opp) lam[v] = 0.0;
    else { lam[v] = t == 0 ? fl[0] : (t == 1 ? fl[1] : fl[2]); ++t; }
  }
}

// The same steps for a tetrahedron (the 3 edge midpoints of the face as the rule), as MACROS for k_boundary_force<3> and
// k_wall_facets<3, *>: expanded in the kernel they compile to the parent's arithmetic; as functions the compiler folds
// the rule's constants another way and the kernels lose the parent's count of multiplications (the byte rule).  NV, DIM
// are the kernel's constants.
#define NSFEM_FACET_FRONT_3D(vx, nc, c, opp, F) \
_Pragma("unroll") \
    for (int v = 0; v < NV; ++v) \
_Pragma("unroll") \
      for (int d = 0; d < DIM; ++d) F.x[v][d] = vx[(size_t)(DIM * v + d) * nc + c]; \
    double a[3][3]; \
_Pragma("unroll") \
    for (int d = 0; d < 3; ++d) { \
      a[d][0] = F.x[1][d] - F.x[0][d]; \
      a[d][1] = F.x[2][d] - F.x[0][d]; \
      a[d][2] = F.x[3][d] - F.x[0][d]; \
    } \
    const double c00 = a[1][1] * a[2][2] - a[1][2] * a[2][1]; \
    const double c01 = a[1][2] * a[2][0] - a[1][0] * a[2][2]; \
    const double c02 = a[1][0] * a[2][1] - a[1][1] * a[2][0]; \
    const double det = a[0][0] * c00 + a[0][1] * c01 + a[0][2] * c02, id = 1.0 / det; \
    F.gl[1][0] = c00 * id; \
    F.gl[1][1] = (a[0][2] * a[2][1] - a[0][1] * a[2][2]) * id; \
    F.gl[1][2] = (a[0][1] * a[1][2] - a[0][2] * a[1][1]) * id; \
    F.gl[2][0] = c01 * id; \
    F.gl[2][1] = (a[0][0] * a[2][2] - a[0][2] * a[2][0]) * id; \
    F.gl[2][2] = (a[0][2] * a[1][0] - a[0][0] * a[1][2]) * id; \
    F.gl[3][0] = c02 * id; \
    F.gl[3][1] = (a[0][1] * a[2][0] - a[0][0] * a[2][1]) * id; \
    F.gl[3][2] = (a[0][0] * a[1][1] - a[0][1] * a[1][0]) * id; \
_Pragma("unroll") \
    for (int d = 0; d < 3; ++d) F.gl[0][d] = -F.gl[1][d] - F.gl[2][d] - F.gl[3][d]; \
    F.vol = fabs(det); \
    double gn = 0.0, nrm3[3] = {0.0, 0.0, 0.0}; \
_Pragma("unroll") \
    for (int v = 0; v < NV; ++v) \
      if (v == opp) { \
_Pragma("unroll") \
        for (int d = 0; d < DIM; ++d) nrm3[d] = -F.gl[v][d]; \
      } \
_Pragma("unroll") \
    for (int d = 0; d < DIM; ++d) gn += nrm3[d] * nrm3[d]; \
    gn = sqrt(gn); \
_Pragma("unroll") \
    for (int d = 0; d < DIM; ++d) F.nrm[d] = nrm3[d] / gn; \
    F.area = gn * F.vol / 2.0;

#define NSFEM_FACET_RULE_POINT_3D(q, opp, lam) \
      double fl[3]; \
      fl[0] = q == 0 ? 0.0 : 0.5; \
      fl[1] = q == 1 ? 0.0 : 0.5; \
      fl[2] = q == 2 ? 0.0 : 0.5; \
      int t = 0; \
_Pragma("unroll") \
      for (int v = 0; v < NV; ++v) { \
        if (v == opp) lam[v] = 0.0; \
        else { lam[v] = t == 0 ? fl[0] : (t == 1 ? fl[1] : fl[2]); ++t; } \
      }

// ---------------------------------------------------------------------------------------------------- nodal gathers
// v[a] = u[node][a] of a node-interleaved field with NC components; PAIR (NC = 2): one 16-byte load
template <int NC, bool PAIR>
__device__ __forceinline__ void load_node(const double* __restrict__ u, size_t node, double (&v)[NC]) {
  if constexpr (PAIR && NC == 2) {
    const double2 t = reinterpret_cast<const double2*>(u)[node];
    v[0] = t.x;
    v[1] = t.y;
  } else {
#pragma unroll
    for (int a = 0; a < NC; ++a) v[a] = u[NC * node + a];
  }
}
// out[k][a] = u[node_k][a] at the 6 / 10 P2 nodes of cell c.  (k_vol_functionals keeps a gather of its own, the pair
// load with the reference field subtracted at the nodes: through this helper the compiler fuses the products under
// its |u|^2 the other way round, and the sum moves by an ulp.)
template <int DIM, int NC, int LD>
__device__ __forceinline__ void gather_p2_vector(const int32_t* __restrict__ p2, int nc, int c,
                                                 const double* __restrict__ u, double (&out)[DIM == 2 ? 6 : 10][LD]) {
#pragma unroll
  for (int k = 0; k < (DIM == 2 ? 6 : 10); ++k) {
    double v[NC];
    load_node<NC, false>(u, (size_t)p2[(size_t)k * nc + c], v);
#pragma unroll
    for (int a = 0; a < NC; ++a) out[k][a] = v[a];
  }
}

// out[k] = T[node_k] at the 6 / 10 P2 nodes of cell c
template <int DIM>
__device__ __forceinline__ void gather_p2_scalar(const int32_t* __restrict__ p2, int nc, int c,
                                                 const double* __restrict__ T, double (&out)[DIM == 2 ? 6 : 10]) {
#pragma unroll
  for (int k = 0; k < (DIM == 2 ? 6 : 10); ++k) out[k] = T[(size_t)p2[(size_t)k * nc + c]];
}

// out[i] = p[node_i] (- pr[node_i] with pr != null) at the 3 / 4 vertices of cell c
template <int DIM>
__device__ __forceinline__ void gather_p1(const int32_t* __restrict__ p1, int nc, int c, const double* __restrict__ p,
                                          const double* __restrict__ pr, double (&out)[DIM + 1]) {
#pragma unroll
  for (int i = 0; i <= DIM; ++i) {
    const size_t node = (size_t)p1[(size_t)i * nc + c];
    out[i] = p[node];
    if (pr) out[i] -= pr[node];
  }
}

// ------------------------------------------------------------------------------------- fixed-order workgroup sums
// Workgroups of 256 threads (4 waves).  After the call sh[w * N + j] holds the sum of v[j] over wave w (sh: 4 N
// values), folded by the xor-shuffle tree; the barrier has been passed.  (All trees first, then the stores under one
// branch: the N chains of shuffles are independent and overlap; a store between them would serialise them.)
template <int N, class T>
__device__ __forceinline__ void block_sum_fixed(const T (&v)[N], T* sh) {
  T t[N];
#pragma unroll
  for (int j = 0; j < N; ++j) {
    t[j] = v[j];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) t[j] += __shfl_xor(t[j], off);
  }
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int j = 0; j < N; ++j) sh[(threadIdx.x >> 6) * N + j] = t[j];
  }
  __syncthreads();
}
// sum j of the workgroup: the four wave sums in wave order
template <int N, class T>
__device__ __forceinline__ T block_total(const T* sh, unsigned j) {
  return ((sh[0 * N + j] + sh[1 * N + j]) + sh[2 * N + j]) + sh[3 * N + j];
}
// thread j < N stores sum j of this workgroup to dst[(row0 + j) * n_cols + col]
template <int N, class T>
__device__ __forceinline__ void store_block_partials(const T* sh, T* __restrict__ dst, size_t row0, unsigned n_cols,
                                                     unsigned col) {
  if (threadIdx.x < N) dst[(row0 + threadIdx.x) * n_cols + col] = block_total<N>(sh, threadIdx.x);
}
// the totals in every thread, and sh free for the next use
template <int N, class T>
__device__ __forceinline__ void block_sum_all(T (&v)[N], T* sh) {
  block_sum_fixed<N>(v, sh);
#pragma unroll
  for (int j = 0; j < N; ++j) v[j] = block_total<N>(sh, j);
  __syncthreads();
}

// --------------------------------------------------------------------------------------------------- front tables
// A __constant__ symbol is private to its translation unit: a file that integrates with the degree-5 rules of the
// assembly kernels gets its own copy and the uploader of it with NSFEM_FRONT_TABLES(name, name3) in namespace nsfem,
// filled by the same fill_quad_tables / fill_quad_tables_3d.  Run-time values: the compiler must not fold the tables'
// zeros into the sums.  The symbols keep external linkage under a name per file: the compiler addresses an internal
// (static) one differently, and k_vol_functionals<3> then needs 169 VGPRs for 166 and loses a wave of occupancy.
#define NSFEM_FRONT_TABLES(Q2, Q3)                                                \
  __constant__ QuadTables Q2;                                                     \
  __constant__ QuadTables3 Q3;                                                    \
  static void upload_front_tables(int dim) {                                      \
    QuadTables t;                                                                 \
    fill_quad_tables(t);                                                          \
    NSFEM_HIP(hipMemcpyToSymbol(HIP_SYMBOL(Q2), &t, sizeof(QuadTables)));         \
    if (dim == 3) {                                                               \
      QuadTables3 t3;                                                             \
      fill_quad_tables_3d(t3);                                                    \
      NSFEM_HIP(hipMemcpyToSymbol(HIP_SYMBOL(Q3), &t3, sizeof(QuadTables3)));     \
    }                                                                             \
  }

}  // namespace nsfem
