// Fast diagonalisation on 3D box lattices (poisson_fd.factors_3d builds the factors on the host).  On a box_mesh
// (six Kuhn tetrahedra per cube) the tensor sum of the 1D stiffness and lumped mass matrices of the three directions,
//
//     T = K_z (x) W_y (x) W_x + W_z (x) K_y (x) W_x + W_z (x) W_y (x) K_x ,
//
// is the P1 stiffness matrix A itself when every box edge between two non-periodic faces touches a Dirichlet face and
// the lines are uniform (triple-periodic, periodic in x and y with z walls, Dirichlet everywhere); otherwise it is a
// spectrally equivalent preconditioner (eigenvalues of (A, T) in [0.798, 1.334], independent of the size).  With the
// generalised eigenvectors V_x, V_y, V_z of the three directions and R = r as an N_z x N_y x N_x array,
//
//     z = T^+ r = (R x_1 V_x x_2 V_y x_3 V_z .* inv) x_1 V_x^T x_2 V_y^T x_3 V_z^T ,
//
// six mode products.  The x products (N_z N_y x N_x times N_x x N_x) and the z products (N_z x N_z times
// N_z x N_y N_x) are plain row-major GEMMs: they run in the 2D solver's k_fd_gemm (fastdiag.hip, launch_fd_gemm), the
// z product of the forward pass with inv fused into its epilogue.  The y products are N_z independent
// (N_y x N_y)(N_y x N_x) products, one per z-plane: k_fd_gemm_batched below, the same MFMA tile (v_mfma_f64_16x16x4_f64,
// 32 x 32 block per 4 waves, k-blocks of 96 staged through LDS, the next two blocks' loads in flight) with the plane
// in blockIdx.z.
#include "nsfem_internal.hpp"

namespace nsfem {

typedef double fd3_acc4 __attribute__((ext_vector_type(4)));

constexpr int kFb3M = 32, kFb3N = 32, kFb3K = 96, kFb3Ld = kFb3K + 2, kFb3Q = kFb3M * kFb3K / 256;

// C_b[M x N] = op(A)[M x K] * B_b[K x N] for b = blockIdx.z: B_b = B + b * strideB (row-major, leading dimension
// ldb), C_b = C + b * strideC (leading dimension ldc), A shared by all planes; TA: A(m, k) = A[k * lda + m].  LDS
// layout and pipeline as k_fd_gemm: As[m][k], Bs[n][k] with lines of 98 doubles; every thread holds the loads of two
// k-blocks (register double buffer) while the 24 MFMAs of the current block run.
template <bool TA>
__global__ __launch_bounds__(256) void k_fd_gemm_batched(int M, int N, int K, const double* __restrict__ A, int lda,
                                                         const double* __restrict__ B, int ldb, int64_t strideB,
                                                         double* __restrict__ C, int ldc, int64_t strideC) {
  __shared__ double As[kFb3M * kFb3Ld];
  __shared__ double Bs[kFb3N * kFb3Ld];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int m0 = blockIdx.y * kFb3M, n0 = blockIdx.x * kFb3N;
  const int wm = (wave >> 1) * 16, wn = (wave & 1) * 16;
  B += (int64_t)blockIdx.z * strideB;
  C += (int64_t)blockIdx.z * strideC;
  // element e = tid + 256 q of a 32 x 96 block along the operand's contiguous direction: A row-major (contiguous
  // along k): k = e % 96, m = e / 96; A transposed and B (contiguous along m / n): line = e % 32, k = e / 32
  double ra0[kFb3Q], rb0[kFb3Q], ra1[kFb3Q], rb1[kFb3Q];
  auto load_block = [&](int k0, double (&ra)[kFb3Q], double (&rb)[kFb3Q]) {
#pragma unroll
    for (int q = 0; q < kFb3Q; ++q) {
      const int e = tid + 256 * q;
      {
        const int m = TA ? (e & 31) : (e / kFb3K), k = TA ? (e >> 5) : (e % kFb3K);
        const int gm = m0 + m, gk = k0 + k;
        ra[q] = (gm < M && gk < K) ? (TA ? A[(size_t)gk * lda + gm] : A[(size_t)gm * lda + gk]) : 0.0;
      }
      {
        const int n = e & 31, k = e >> 5;
        const int gn = n0 + n, gk = k0 + k;
        rb[q] = (gn < N && gk < K) ? B[(size_t)gk * ldb + gn] : 0.0;
      }
    }
  };
  auto store_block = [&](const double (&ra)[kFb3Q], const double (&rb)[kFb3Q]) {
#pragma unroll
    for (int q = 0; q < kFb3Q; ++q) {
      const int e = tid + 256 * q;
      const int ma = TA ? (e & 31) : (e / kFb3K), ka = TA ? (e >> 5) : (e % kFb3K);
      As[ma * kFb3Ld + ka] = ra[q];
      Bs[(e & 31) * kFb3Ld + (e >> 5)] = rb[q];
    }
  };
  fd3_acc4 acc = {0.0, 0.0, 0.0, 0.0}, acc2 = {0.0, 0.0, 0.0, 0.0};
  auto block_products = [&](const double* __restrict__ ap, const double* __restrict__ bp) {
    double af[kFb3K / 4], bf[kFb3K / 4];
#pragma unroll
    for (int i = 0; i < kFb3K / 4; ++i) {
      af[i] = ap[4 * i];
      bf[i] = bp[4 * i];
    }
#pragma unroll
    for (int i = 0; i < kFb3K / 4; i += 2) {
      acc = __builtin_amdgcn_mfma_f64_16x16x4f64(af[i], bf[i], acc, 0, 0, 0);
      acc2 = __builtin_amdgcn_mfma_f64_16x16x4f64(af[i + 1], bf[i + 1], acc2, 0, 0, 0);
    }
  };
  const double* __restrict__ ap = As + (wm + (lane & 15)) * kFb3Ld + (lane >> 4);
  const double* __restrict__ bp = Bs + (wn + (lane & 15)) * kFb3Ld + (lane >> 4);
  load_block(0, ra0, rb0);
  if (kFb3K < K) load_block(kFb3K, ra1, rb1);
  for (int k0 = 0; k0 < K; k0 += 2 * kFb3K) {
    __syncthreads();
    store_block(ra0, rb0);
    __syncthreads();
    if (k0 + 2 * kFb3K < K) load_block(k0 + 2 * kFb3K, ra0, rb0);
    block_products(ap, bp);
    if (k0 + kFb3K >= K) break;
    __syncthreads();
    store_block(ra1, rb1);
    __syncthreads();
    if (k0 + 3 * kFb3K < K) load_block(k0 + 3 * kFb3K, ra1, rb1);
    block_products(ap, bp);
  }
  acc += acc2;
  // C/D layout of v_mfma_f64_16x16x4_f64: col = lane & 15, row = (lane >> 4) + 4 * reg
  const int col = n0 + wn + (lane & 15);
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int row = m0 + wm + (lane >> 4) + 4 * r;
    if (row < M && col < N) C[(size_t)row * ldc + col] = acc[r];
  }
}

// the y products: plane k of the N_z x N_y x N_x array, C_k = op(V_y) B_k
template <bool TA>
static void fd_gemm_planes(hipStream_t s, int Nx, int Ny, int Nz, const double* Vy, const double* B, double* C) {
  const int64_t plane = (int64_t)Ny * Nx;
  const dim3 grid((Nx + kFb3N - 1) / kFb3N, (Ny + kFb3M - 1) / kFb3M, Nz), block(256);
  hipLaunchKernelGGL((k_fd_gemm_batched<TA>), grid, block, 0, s, Ny, Nx, Ny, Vy, Ny, B, Nx, plane, C, Nx, plane);
  NSFEM_HIP(hipGetLastError());
}

void FastDiag3::set(hipStream_t s, int Nx_, int Ny_, int Nz_, const double* vx, const double* vy, const double* vz,
                    const double* inv_, bool exact_) {
  NSFEM_REQUIRE(Nx_ >= 2 && Ny_ >= 2 && Nz_ >= 2 && Nz_ <= 65535 && vx && vy && vz && inv_,
                "fast diagonalisation (3D): bad factors");
  NSFEM_REQUIRE((int64_t)Nz_ * Ny_ < INT32_MAX && (int64_t)Ny_ * Nx_ < INT32_MAX,
                "fast diagonalisation (3D): lattice too large");
  Nx = Nx_;
  Ny = Ny_;
  Nz = Nz_;
  exact = exact_;
  first = n_loc = own0 = n_own = 0;
  comm = nullptr;
  tz.release();
  const size_t n = (size_t)Nx * Ny * Nz;
  Vx.upload(vx, (size_t)Nx * Nx, s);
  Vy.upload(vy, (size_t)Ny * Ny, s);
  Vz.upload(vz, (size_t)Nz * Nz, s);
  inv.upload(inv_, n, s);
  // (buffers of an unchanged size are kept, as upload() keeps those of the factors: a CG iteration body captured into
  // a graph holds their addresses -- the setters bump the context's graph epoch as well)
  if (t1.n != n) t1.alloc(n);
  if (t2.n != n) t2.alloc(n);
  NSFEM_HIP(hipStreamSynchronize(s));
}

// Partitioned slabs (rank r holds the lattice planes (first + i) mod N_z, i < n_loc, ghost planes included, and owns the
// run own0 ... own0 + n_own - 1 of them; every node is owned by one rank): the contraction over z is a sum over the
// ranks, the other two directions stay inside the planes,
//
//     T     = sum_ranks V_z[owned planes, :]^T (R_own x_1 V_x x_2 V_y)  .* inv      one all-reduce of N_z N_y N_x doubles
//     Z_loc = (V_z[local planes, :] T) x_2 V_y^T x_1 V_x^T                           every local plane, ghosts included
//
// -- the strip design of FastDiag::apply_strip one dimension up.  Only owned planes enter the contraction (the ghost
// planes of r are never read), so inv goes into that product's epilogue: an elementwise scale commutes with the sum.
void FastDiag3::set_planes(hipStream_t s, Comm* comm_, int Nx_, int Ny_, int Nz_, int first_, int n_loc_, int own0_,
                           int n_own_, const double* vx, const double* vy, const double* vz, const double* inv_,
                           bool exact_) {
  NSFEM_REQUIRE(comm_ && Nx_ >= 2 && Ny_ >= 2 && Nz_ >= 2 && vx && vy && vz && inv_, "fast diagonalisation (3D): bad factors");
  NSFEM_REQUIRE(first_ >= 0 && first_ < Nz_ && n_loc_ >= 1 && n_loc_ <= 65535 && own0_ >= 0 && n_own_ >= 1 &&
                    own0_ + n_own_ <= n_loc_ && n_own_ <= Nz_,
                "fast diagonalisation (3D): bad local planes");
  NSFEM_REQUIRE((int64_t)Nz_ * Ny_ < INT32_MAX && (int64_t)n_loc_ * Ny_ < INT32_MAX && (int64_t)Ny_ * Nx_ < INT32_MAX,
                "fast diagonalisation (3D): lattice too large");
  Nx = Nx_;
  Ny = Ny_;
  Nz = Nz_;
  exact = exact_;
  first = first_;
  n_loc = n_loc_;
  own0 = own0_;
  n_own = n_own_;
  comm = comm_;
  const size_t pl = (size_t)Nx * Ny;
  // rows (first + i) mod N_z of the row-major N_z x N_z matrix V_z (periodic slabs wrap around)
  std::vector<double> rows((size_t)n_loc * Nz);
  for (int i = 0; i < n_loc; ++i) {
    const double* src = vz + (size_t)((first + i) % Nz) * Nz;
    std::copy(src, src + Nz, rows.begin() + (size_t)i * Nz);
  }
  Vx.upload(vx, (size_t)Nx * Nx, s);
  Vy.upload(vy, (size_t)Ny * Ny, s);
  Vz.upload(rows.data(), rows.size(), s);
  inv.upload(inv_, pl * Nz, s);
  if (t1.n != pl * n_loc) t1.alloc(pl * n_loc);
  if (t2.n != pl * n_loc) t2.alloc(pl * n_loc);
  if (tz.n != pl * Nz) tz.alloc(pl * Nz);
  NSFEM_HIP(hipStreamSynchronize(s));      // (rows is a pageable host vector)
}

void FastDiag3::release() {
  Nx = Ny = Nz = 0;
  first = n_loc = own0 = n_own = 0;
  comm = nullptr;
  exact = false;
  for (DevBuf<double>* b : {&Vx, &Vy, &Vz, &inv, &t1, &t2, &tz}) b->release();
}

// slabs: r on the local planes in (its ghost planes ignored), z on EVERY local plane out -- a collective
void FastDiag3::apply_slab(hipStream_t s, const double* r, double* z) {
  NSFEM_REQUIRE(ready() && slab() && comm, "fast diagonalisation (3D): slab factors / communicator not set");
  const int pl = Ny * Nx;
  const double* r_own = r + (size_t)own0 * pl;
  launch_fd_gemm(s, false, false, n_own * Ny, Nx, Nx, r_own, Nx, Vx.p, Nx, t1.p, Nx, nullptr);    // x: owned planes
  fd_gemm_planes<true>(s, Nx, Ny, n_own, Vy.p, t1.p, t2.p);                                        // y: V_y^T per plane
  launch_fd_gemm(s, true, false, Nz, pl, n_own, Vz.p + (size_t)own0 * Nz, Nz, t2.p, pl, tz.p, pl,  // z: partial sum
                 inv.p);                                                                            //    .* inv
  comm->allreduce_sum(s, tz.p, (int64_t)Nz * pl);
  launch_fd_gemm(s, false, false, n_loc, pl, Nz, Vz.p, Nz, tz.p, pl, t1.p, pl, nullptr);            // z: local planes
  fd_gemm_planes<false>(s, Nx, Ny, n_loc, Vy.p, t1.p, t2.p);                                       // y: V_y per plane
  launch_fd_gemm(s, false, true, n_loc * Ny, Nx, Nx, t2.p, Nx, Vx.p, Nx, z, Nx, nullptr);          // x: ... V_x^T
  ++applications;
}

// z = T^+ r: six launches, r and z untouched until the first / last one
void FastDiag3::apply(hipStream_t s, const double* r, double* z) {
  if (slab()) return apply_slab(s, r, z);      // (CG preconditioned by the slab T^+: op.prec)
  NSFEM_REQUIRE(ready(), "fast diagonalisation (3D): factors not set");
  const int pl = Ny * Nx, rows = Nz * Ny;
  launch_fd_gemm(s, false, false, rows, Nx, Nx, r, Nx, Vx.p, Nx, t1.p, Nx, nullptr);        // x:  R x_1 V_x
  fd_gemm_planes<true>(s, Nx, Ny, Nz, Vy.p, t1.p, t2.p);                                     // y:  V_y^T per plane
  launch_fd_gemm(s, true, false, Nz, pl, Nz, Vz.p, Nz, t2.p, pl, t1.p, pl, inv.p);           // z:  V_z^T ... .* inv
  launch_fd_gemm(s, false, false, Nz, pl, Nz, Vz.p, Nz, t1.p, pl, t2.p, pl, nullptr);        // z:  V_z
  fd_gemm_planes<false>(s, Nx, Ny, Nz, Vy.p, t2.p, t1.p);                                    // y:  V_y per plane
  launch_fd_gemm(s, false, true, rows, Nx, Nx, t1.p, Nx, Vx.p, Nx, z, Nx, nullptr);          // x:  ... V_x^T
  ++applications;
}

}  // namespace nsfem
