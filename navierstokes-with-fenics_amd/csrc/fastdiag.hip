// Fast diagonalisation of the pressure Poisson operator on tensor-product lattices (poisson_fd.py builds the
// factors on the host).  The reference solves the projection step with a sparse LU every step
// (source/ns_ipcs_solver.py:160-171); on the right-diagonal triangulation of a rectangle the P1 stiffness matrix is the
// tensor sum  A = K_y (x) W_x + W_y (x) K_x  of 1D stiffness and lumped mass matrices, so with the generalised
// eigenvectors V_x, V_y of the two directions
//
//     z = A^+ r = V_y ( (V_y^T R V_x) .* inv ) V_x^T ,      R = r as an H x W array,  inv_ji = 1 / (lam_y,j + lam_x,i)
//
// -- four dense products with (n + 1)-sized matrices, the one GEMM-shaped operation of the hot path.  They run on the
// matrix cores: v_mfma_f64_16x16x4_f64, one 16 x 16 accumulator tile per wavefront, operands staged through LDS
// (rows padded to 48 doubles: the four k-lines a wave reads land on disjoint halves of the 64 banks), the next
// k-block's global loads in flight under the current block's MFMAs.  (On the MI355X the fp64 matrix rate equals the
// vector rate; what the matrix instruction buys here is 16 x fewer issued instructions and 8 x fewer LDS reads per
// FMA than a register-tiled VALU kernel: these 513-sized products are latency bound, not flop bound.)
//
// 3D box lattices (poisson_fd.factors_3d; box_mesh: six Kuhn tetrahedra per cube): the tensor sum of the 1D stiffness
// and lumped mass matrices of the three directions,
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
// N_z x N_y N_x) are plain row-major GEMMs (k_fd_gemm, the z product of the forward pass with inv fused into its
// epilogue); the y products are N_z independent (N_y x N_y)(N_y x N_x) products, one per z-plane: k_fd_gemm_batched,
// the same tile with the plane in blockIdx.z.
#include "nsfem_internal.hpp"

namespace nsfem {

typedef double fd_acc4 __attribute__((ext_vector_type(4)));

constexpr int kFdBM = 32, kFdBN = 32, kFdBK = 96, kFdLd = kFdBK + 2, kFdNQ = kFdBM * kFdBK / 256;

// The tile body of both kernels: one 32 x 32 block of
// C[M x N] = op(A)[M x K] * op(B)[K x N] (.* scale[M x N]); row-major storage.  TA: A(m, k) = A[k * lda + m];
// TB: B(k, n) = B[n * ldb + k].  256 threads = 4 waves, wave w owns the 16 x 16 tile (w >> 1, w & 1) of a 32 x 32
// block of C.  The products are latency bound (K = 513: six k-blocks of 96, every one a global round trip): a thread
// keeps the 2 x 12 loads of the NEXT TWO blocks in flight (register double buffer) under the 24 MFMAs of a block.
// LDS: As[m][k], Bs[n][k] with lines of 98 doubles -- the fragment reads (16 lines x 4 consecutive k per wave) and the
// stores along k are conflict free.
template <bool TA, bool TB>
__device__ __forceinline__ void fd_gemm_tile(int M, int N, int K, const double* __restrict__ A, int lda,
                                             const double* __restrict__ B, int ldb, double* __restrict__ C, int ldc,
                                             const double* __restrict__ scale) {
  __shared__ double As[kFdBM * kFdLd];      // As[m][k]
  __shared__ double Bs[kFdBN * kFdLd];      // Bs[n][k]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int m0 = blockIdx.y * kFdBM, n0 = blockIdx.x * kFdBN;
  const int wm = (wave >> 1) * 16, wn = (wave & 1) * 16;
  // element e = tid + 256 q of a 32 x 96 block, walked along the operand's contiguous direction:
  //   contiguous along k (A row-major, B transposed): k = e % 96, line = e / 96
  //   contiguous along m / n (A transposed, B row-major): line = e % 32, k = e / 32
  double ra0[kFdNQ], rb0[kFdNQ], ra1[kFdNQ], rb1[kFdNQ];      // two k-blocks in flight (register double buffer)
  auto load_block = [&](int k0, double (&ra)[kFdNQ], double (&rb)[kFdNQ]) {
#pragma unroll
    for (int q = 0; q < kFdNQ; ++q) {
      const int e = tid + 256 * q;
      {
        const int m = TA ? (e & 31) : (e / kFdBK), k = TA ? (e >> 5) : (e % kFdBK);
        const int gm = m0 + m, gk = k0 + k;
        ra[q] = (gm < M && gk < K) ? (TA ? A[(size_t)gk * lda + gm] : A[(size_t)gm * lda + gk]) : 0.0;
      }
      {
        const int n = TB ? (e / kFdBK) : (e & 31), k = TB ? (e % kFdBK) : (e >> 5);
        const int gn = n0 + n, gk = k0 + k;
        rb[q] = (gn < N && gk < K) ? (TB ? B[(size_t)gn * ldb + gk] : B[(size_t)gk * ldb + gn]) : 0.0;
      }
    }
  };
  auto store_block = [&](const double (&ra)[kFdNQ], const double (&rb)[kFdNQ]) {
#pragma unroll
    for (int q = 0; q < kFdNQ; ++q) {
      const int e = tid + 256 * q;
      const int ma = TA ? (e & 31) : (e / kFdBK), ka = TA ? (e >> 5) : (e % kFdBK);
      As[ma * kFdLd + ka] = ra[q];
      const int nb = TB ? (e / kFdBK) : (e & 31), kb = TB ? (e % kFdBK) : (e >> 5);
      Bs[nb * kFdLd + kb] = rb[q];
    }
  };
  // (two accumulator chains and the block's 2 x 24 fragments read before its first MFMA: one chain waits for every
  // product and, just in time, for its LDS read)
  fd_acc4 acc = {0.0, 0.0, 0.0, 0.0}, acc2 = {0.0, 0.0, 0.0, 0.0};
  auto block_products = [&](const double* __restrict__ ap, const double* __restrict__ bp) {
    double af[kFdBK / 4], bf[kFdBK / 4];
#pragma unroll
    for (int i = 0; i < kFdBK / 4; ++i) {
      af[i] = ap[4 * i];
      bf[i] = bp[4 * i];
    }
#pragma unroll
    for (int i = 0; i < kFdBK / 4; i += 2) {
      acc = __builtin_amdgcn_mfma_f64_16x16x4f64(af[i], bf[i], acc, 0, 0, 0);
      acc2 = __builtin_amdgcn_mfma_f64_16x16x4f64(af[i + 1], bf[i + 1], acc2, 0, 0, 0);
    }
  };
  const double* __restrict__ ap = As + (wm + (lane & 15)) * kFdLd + (lane >> 4);       // A[m = lane & 15][k = lane >> 4]
  const double* __restrict__ bp = Bs + (wn + (lane & 15)) * kFdLd + (lane >> 4);       // B[k = lane >> 4][n = lane & 15]
  load_block(0, ra0, rb0);
  if (kFdBK < K) load_block(kFdBK, ra1, rb1);
  for (int k0 = 0; k0 < K; k0 += 2 * kFdBK) {
    __syncthreads();                         // (the previous block's fragments have been read)
    store_block(ra0, rb0);
    __syncthreads();
    if (k0 + 2 * kFdBK < K) load_block(k0 + 2 * kFdBK, ra0, rb0);
    block_products(ap, bp);
    if (k0 + kFdBK >= K) break;
    __syncthreads();
    store_block(ra1, rb1);
    __syncthreads();
    if (k0 + 3 * kFdBK < K) load_block(k0 + 3 * kFdBK, ra1, rb1);
    block_products(ap, bp);
  }
  acc += acc2;
  // C/D layout of v_mfma_f64_16x16x4_f64: col = lane & 15, row = (lane >> 4) + 4 * reg
  const int col = n0 + wn + (lane & 15);
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int row = m0 + wm + (lane >> 4) + 4 * r;
    if (row < M && col < N) {
      double v = acc[r];
      if (scale) v *= scale[(size_t)row * N + col];
      C[(size_t)row * ldc + col] = v;
    }
  }
}

template <bool TA, bool TB>
__global__ __launch_bounds__(256) void k_fd_gemm(int M, int N, int K, const double* __restrict__ A, int lda,
                                                 const double* __restrict__ B, int ldb, double* __restrict__ C, int ldc,
                                                 const double* __restrict__ scale) {
  fd_gemm_tile<TA, TB>(M, N, K, A, lda, B, ldb, C, ldc, scale);
}

// C_b = op(A) * B_b for b = blockIdx.z: B_b = B + b * strideB, C_b = C + b * strideC (both row-major), A shared by all
// planes
template <bool TA>
__global__ __launch_bounds__(256) void k_fd_gemm_batched(int M, int N, int K, const double* __restrict__ A, int lda,
                                                         const double* __restrict__ B, int ldb, int64_t strideB,
                                                         double* __restrict__ C, int ldc, int64_t strideC) {
  fd_gemm_tile<TA, false>(M, N, K, A, lda, B + (int64_t)blockIdx.z * strideB, ldb, C + (int64_t)blockIdx.z * strideC,
                          ldc, nullptr);
}

template <bool TA, bool TB>
static void fd_gemm(hipStream_t s, int M, int N, int K, const double* A, int lda, const double* B, int ldb, double* C,
                    int ldc, const double* scale) {
  const dim3 grid((N + kFdBN - 1) / kFdBN, (M + kFdBM - 1) / kFdBM), block(256);
  hipLaunchKernelGGL((k_fd_gemm<TA, TB>), grid, block, 0, s, M, N, K, A, lda, B, ldb, C, ldc, scale);
  NSFEM_HIP(hipGetLastError());
}

// the y products of the 3D solve: plane k of the N_z x N_y x N_x array, C_k = op(V_y) B_k
template <bool TA>
static void fd_gemm_planes(hipStream_t s, int Nx, int Ny, int Nz, const double* Vy, const double* B, double* C) {
  const int64_t plane = (int64_t)Ny * Nx;
  const dim3 grid((Nx + kFdBN - 1) / kFdBN, (Ny + kFdBM - 1) / kFdBM, Nz), block(256);
  hipLaunchKernelGGL((k_fd_gemm_batched<TA>), grid, block, 0, s, Ny, Nx, Ny, Vy, Ny, B, Nx, plane, C, Nx, plane);
  NSFEM_HIP(hipGetLastError());
}

// (work buffers of an unchanged size are kept, as upload() keeps those of the factors: a CG iteration body captured
// into a graph holds the addresses of the 3D ones -- the setters bump the context's graph epoch as well)
static void fd_keep_or_alloc(DevBuf<double>& b, size_t n) {
  if (b.n != n) b.alloc(n);
}

// ---- 2D --------------------------------------------------------------------------------------------------------------
void FastDiag::set(hipStream_t s, int W_, int H_, const double* vx, const double* vy, const double* inv_) {
  NSFEM_REQUIRE(W_ >= 2 && H_ >= 2 && vx && vy && inv_, "fast diagonalisation: bad factors");
  W = W_;
  H = H_;
  j0 = h_loc = 0;
  Vx.upload(vx, (size_t)W * W, s);
  Vy.upload(vy, (size_t)H * H, s);
  inv.upload(inv_, (size_t)H * W, s);
  fd_keep_or_alloc(t1, (size_t)H * W);
  fd_keep_or_alloc(t2, (size_t)H * W);
  NSFEM_HIP(hipStreamSynchronize(s));
}

// Strips of a partitioned mesh (rank r holds the lattice lines j0 ... j0 + h_loc - 1, ghost lines included; every
// node is OWNED by one rank and r vanishes on the ghost rows): the contraction over y is a sum over the ranks,
//
//     T2 = sum_ranks V_y[lines of the rank, :]^T (R_loc V_x)          one all-reduce of H x W doubles
//     Z_loc = (V_y[lines of the rank, :] (T2 .* inv)) V_x^T           every local line, ghost lines included
//
// -- the whole projection solve of an N-rank run costs ONE collective (the multigrid-CG solve it replaces: ~10 halo
// exchanges + 2 small all-reduces per iteration), the four products shrink to 1 / N of their size, and the result
// comes with valid ghost rows (no exchange afterwards).
void FastDiag::set_rows(hipStream_t s, int W_, int H_, int j0_, int h_loc_, const double* vx, const double* vy,
                        const double* inv_) {
  NSFEM_REQUIRE(W_ >= 2 && H_ >= 2 && vx && vy && inv_ && j0_ >= 0 && h_loc_ >= 1 && j0_ + h_loc_ <= H_,
                "fast diagonalisation: bad factors / lines");
  W = W_;
  H = H_;
  j0 = j0_;
  h_loc = h_loc_;
  Vx.upload(vx, (size_t)W * W, s);
  Vy.upload(vy + (size_t)j0 * H, (size_t)h_loc * H, s);          // rows j0 ... of the row-major H x H matrix
  inv.upload(inv_, (size_t)H * W, s);
  fd_keep_or_alloc(t1, (size_t)h_loc * W);
  fd_keep_or_alloc(t2, (size_t)H * W);
  NSFEM_HIP(hipStreamSynchronize(s));
}

__global__ __launch_bounds__(256) void k_fd_scale(int64_t n, const double* __restrict__ a, double* __restrict__ x) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) x[i] *= a[i];
}

void FastDiag::apply_strip(hipStream_t s, const double* r, double* z) {
  NSFEM_REQUIRE(ready() && partitioned() && *comm, "fast diagonalisation: strip factors / communicator not set");
  fd_gemm<false, false>(s, h_loc, W, W, r, W, Vx.p, W, t1.p, W, nullptr);          // T1 = R_loc V_x
  fd_gemm<true, false>(s, H, W, h_loc, Vy.p, H, t1.p, W, t2.p, W, nullptr);         // T2 = V_y[loc, :]^T T1  (partial)
  (*comm)->allreduce_sum(s, t2.p, (int64_t)H * W);
  const int64_t n = (int64_t)H * W;
  hipLaunchKernelGGL(k_fd_scale, dim3((unsigned)std::min<int64_t>((n + 255) / 256, 2048)), dim3(256), 0, s, n,
                     (const double*)inv.p, t2.p);
  NSFEM_HIP(hipGetLastError());
  fd_gemm<false, false>(s, h_loc, W, H, Vy.p, H, t2.p, W, t1.p, W, nullptr);        // U = V_y[loc, :] (T2 .* inv)
  fd_gemm<false, true>(s, h_loc, W, W, t1.p, W, Vx.p, W, z, W, nullptr);            // Z_loc = U V_x^T
  ++applications;
}

// z = V_y ((V_y^T (R V_x)) .* inv) V_x^T
void FastDiag::apply(hipStream_t s, const double* r, double* z) {
  if (partitioned()) return apply_strip(s, r, z);
  NSFEM_REQUIRE(ready(), "fast diagonalisation: factors not set (or set for a strip)");
  fd_gemm<false, false>(s, H, W, W, r, W, Vx.p, W, t1.p, W, nullptr);            // T1 = R V_x
  fd_gemm<true, false>(s, H, W, H, Vy.p, H, t1.p, W, t2.p, W, inv.p);            // T2 = (V_y^T T1) .* inv
  fd_gemm<false, true>(s, H, W, W, t2.p, W, Vx.p, W, t1.p, W, nullptr);          // T1 = T2 V_x^T
  fd_gemm<false, false>(s, H, W, H, Vy.p, H, t1.p, W, z, W, nullptr);            // Z  = V_y T1
  ++applications;
}

void FastDiag::release() {
  W = H = j0 = h_loc = 0;
  for (DevBuf<double>* b : {&Vx, &Vy, &inv, &t1, &t2}) b->release();
}

// ---- 3D --------------------------------------------------------------------------------------------------------------
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
  tz.release();
  const size_t n = (size_t)Nx * Ny * Nz;
  Vx.upload(vx, (size_t)Nx * Nx, s);
  Vy.upload(vy, (size_t)Ny * Ny, s);
  Vz.upload(vz, (size_t)Nz * Nz, s);
  inv.upload(inv_, n, s);
  fd_keep_or_alloc(t1, n);
  fd_keep_or_alloc(t2, n);
  NSFEM_HIP(hipStreamSynchronize(s));
}

// Partitioned slabs (rank r holds the lattice planes (first + i) mod N_z, i < n_loc, ghost planes included, and owns the
// run own0 ... own0 + n_own - 1 of them; every node is owned by one rank): the contraction over z is a sum over the
// ranks, the other two directions stay inside the planes,
//
//     T     = sum_ranks V_z[owned planes, :]^T (R_own x_1 V_x x_2 V_y)  .* inv      one all-reduce of N_z N_y N_x doubles
//     Z_loc = (V_z[local planes, :] T) x_2 V_y^T x_1 V_x^T                           every local plane, ghosts included
//
// -- the strip design one dimension up.  Only owned planes enter the contraction (the ghost planes of r are never
// read), so inv goes into that product's epilogue: an elementwise scale commutes with the sum.
void FastDiag3::set_planes(hipStream_t s, int Nx_, int Ny_, int Nz_, int first_, int n_loc_, int own0_, int n_own_,
                           const double* vx, const double* vy, const double* vz, const double* inv_, bool exact_) {
  NSFEM_REQUIRE(*comm && Nx_ >= 2 && Ny_ >= 2 && Nz_ >= 2 && vx && vy && vz && inv_, "fast diagonalisation (3D): bad factors");
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
  fd_keep_or_alloc(t1, pl * n_loc);
  fd_keep_or_alloc(t2, pl * n_loc);
  fd_keep_or_alloc(tz, pl * Nz);
  NSFEM_HIP(hipStreamSynchronize(s));      // (rows is a pageable host vector)
}

void FastDiag3::release() {
  Nx = Ny = Nz = 0;
  first = n_loc = own0 = n_own = 0;
  exact = false;
  for (DevBuf<double>* b : {&Vx, &Vy, &Vz, &inv, &t1, &t2, &tz}) b->release();
}

void FastDiag3::apply_slab(hipStream_t s, const double* r, double* z) {
  NSFEM_REQUIRE(ready() && partitioned() && *comm, "fast diagonalisation (3D): slab factors / communicator not set");
  const int pl = Ny * Nx;
  const double* r_own = r + (size_t)own0 * pl;
  fd_gemm<false, false>(s, n_own * Ny, Nx, Nx, r_own, Nx, Vx.p, Nx, t1.p, Nx, nullptr);           // x: owned planes
  fd_gemm_planes<true>(s, Nx, Ny, n_own, Vy.p, t1.p, t2.p);                                        // y: V_y^T per plane
  fd_gemm<true, false>(s, Nz, pl, n_own, Vz.p + (size_t)own0 * Nz, Nz, t2.p, pl, tz.p, pl, inv.p); // z: partial sum .* inv
  (*comm)->allreduce_sum(s, tz.p, (int64_t)Nz * pl);
  fd_gemm<false, false>(s, n_loc, pl, Nz, Vz.p, Nz, tz.p, pl, t1.p, pl, nullptr);                  // z: local planes
  fd_gemm_planes<false>(s, Nx, Ny, n_loc, Vy.p, t1.p, t2.p);                                       // y: V_y per plane
  fd_gemm<false, true>(s, n_loc * Ny, Nx, Nx, t2.p, Nx, Vx.p, Nx, z, Nx, nullptr);                 // x: ... V_x^T
  ++applications;
}

// z = T^+ r: six launches, r and z untouched until the first / last one
void FastDiag3::apply(hipStream_t s, const double* r, double* z) {
  if (partitioned()) return apply_slab(s, r, z);      // (also CG preconditioned by the slab T^+: op.prec)
  NSFEM_REQUIRE(ready(), "fast diagonalisation (3D): factors not set");
  const int pl = Ny * Nx, rows = Nz * Ny;
  fd_gemm<false, false>(s, rows, Nx, Nx, r, Nx, Vx.p, Nx, t1.p, Nx, nullptr);        // x:  R x_1 V_x
  fd_gemm_planes<true>(s, Nx, Ny, Nz, Vy.p, t1.p, t2.p);                              // y:  V_y^T per plane
  fd_gemm<true, false>(s, Nz, pl, Nz, Vz.p, Nz, t2.p, pl, t1.p, pl, inv.p);           // z:  V_z^T ... .* inv
  fd_gemm<false, false>(s, Nz, pl, Nz, Vz.p, Nz, t1.p, pl, t2.p, pl, nullptr);        // z:  V_z
  fd_gemm_planes<false>(s, Nx, Ny, Nz, Vy.p, t2.p, t1.p);                             // y:  V_y per plane
  fd_gemm<false, true>(s, rows, Nx, Nx, t1.p, Nx, Vx.p, Nx, z, Nx, nullptr);          // x:  ... V_x^T
  ++applications;
}

// ---- separable transform (energy spectra: spectrum.hip) -----------------------------------------------------------------
// the forward products of FastDiag3::apply with matrices stored row = basis function: the same three kernels, nothing
// of the solvers changes
double* fd_transform_axes(hipStream_t s, int n0, int n1, int n2, const double* Fx, const double* Fy, const double* Fz,
                          double* a, double* b, int64_t* launches) {
  NSFEM_REQUIRE(n0 >= 1 && n1 >= 1 && n2 >= 1 && n2 <= 65535 && (int64_t)n2 * n1 < INT32_MAX &&
                    (int64_t)n1 * n0 < INT32_MAX && ((int64_t)n2 * n1 + kFdBM - 1) / kFdBM <= 65535 &&
                    (n1 + kFdBM - 1) / kFdBM <= 65535,
                "separable transform: lattice too large");
  double *src = a, *dst = b;
  if (Fx) {
    fd_gemm<false, true>(s, n2 * n1, n0, n0, src, n0, Fx, n0, dst, n0, nullptr);      // x:  ... F_x^T
    std::swap(src, dst);
    ++*launches;
  }
  if (Fy) {
    fd_gemm_planes<false>(s, n0, n1, n2, Fy, src, dst);                               // y:  F_y per plane
    std::swap(src, dst);
    ++*launches;
  }
  if (Fz) {
    fd_gemm<false, false>(s, n2, n1 * n0, n2, Fz, n2, src, n1 * n0, dst, n1 * n0, nullptr);   // z:  F_z
    std::swap(src, dst);
    ++*launches;
  }
  return src;
}

}  // namespace nsfem
