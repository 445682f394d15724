// Energy spectra on box lattices: a separable linear transform of a nodal field on its lattice followed by binned sums
// of squares (nsfem_spectrum_* of include/nsfem.h; the host side, energy_spectrum.py, decides what a bin means).
//
// The nodes of a P2 (P1) field on a box mesh occupy every point of the half-spacing (vertex) lattice exactly once, so
// the nodal values ARE a regular sample and a wavenumber spectrum needs no interpolation: k_spec_pack gathers one
// component into lattice order, fd_transform_axes (fastdiag.hip) applies the dense matrices of the transformed axes on
// the matrix cores, and the two kernels below sum the squared coefficients per bin.  With the real orthonormal Fourier
// basis no complex arithmetic is needed: the squares of the cos and sin coefficients of wavenumber k add up to
// N (|u^_k|^2 + |u^_-k|^2), and the host puts both rows into the bin of |k|.
//
// Replaces get_state + numpy.fft.fftn + a Python binning loop per sample.  No atomics: every sum has a fixed order, the
// same state gives the same bytes.  The state is read only; the work arrays belong to the plan.
#include "nsfem_internal.hpp"

namespace nsfem {

// the writes along `point` are coalesced; the reads are a gather (parity numbering: the nodes are not in lattice order)
__global__ __launch_bounds__(256) void k_spec_pack(int64_t n_points, const int32_t* __restrict__ node_of_point,
                                                   const double* __restrict__ state, int ncomp, int c,
                                                   double* __restrict__ w) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_points; i += (int64_t)gridDim.x * blockDim.x)
    w[i] = state[(size_t)node_of_point[i] * ncomp + c];
}

// one workgroup per chunk of at most kSpecChunk entries of the bin CSR: thread t adds the squares of the entries
// t, t + 256, ... of its chunk in ascending order from +0.0, then a fixed tree over the 256 thread sums in LDS
__global__ __launch_bounds__(256) void k_spec_bin(const double* __restrict__ w, int32_t n_chunks,
                                                  const int32_t* __restrict__ chunk_ptr,
                                                  const int32_t* __restrict__ bin_points, double* __restrict__ parts) {
#pragma clang fp contract(off)
  __shared__ double red[256];
  const int t = threadIdx.x;
  for (int32_t k = blockIdx.x; k < n_chunks; k += gridDim.x) {
    const int32_t b = chunk_ptr[k], e = chunk_ptr[k + 1];
    double s = 0.0;
    for (int32_t i = b + t; i < e; i += 256) {
      const double v = w[bin_points[i]];
      s += v * v;
    }
    red[t] = s;
    __syncthreads();
#pragma unroll
    for (int h = 128; h >= 1; h >>= 1) {
      if (t < h) red[t] += red[t + h];
      __syncthreads();
    }
    if (t == 0) parts[k] = red[0];
    __syncthreads();      // (red is written again by the next chunk of this workgroup)
  }
}

// one thread per bin: its chunk partials in ascending order
__global__ __launch_bounds__(256) void k_spec_bin_sum(int32_t n_bins, const int32_t* __restrict__ bin_chunk_ptr,
                                                      const double* __restrict__ parts, int ncomp, int c,
                                                      double* __restrict__ out) {
  for (int32_t b = blockIdx.x * blockDim.x + threadIdx.x; b < n_bins; b += gridDim.x * blockDim.x) {
    double s = 0.0;
    const int32_t e = bin_chunk_ptr[b + 1];
    for (int32_t k = bin_chunk_ptr[b]; k < e; ++k) s += parts[k];
    out[(size_t)b * ncomp + c] = s;
  }
}

void launch_spec_pack(hipStream_t s, int64_t n_points, const int32_t* node_of_point, const double* state, int ncomp,
                      int c, double* w) {
  const int grid = (int)std::min<int64_t>((n_points + 255) / 256, 8192);
  hipLaunchKernelGGL(k_spec_pack, dim3(grid), dim3(256), 0, s, n_points, node_of_point, state, ncomp, c, w);
  NSFEM_HIP(hipGetLastError());
}

void launch_spec_bin(hipStream_t s, const double* w, int32_t n_chunks, const int32_t* chunk_ptr,
                     const int32_t* bin_points, double* parts, int32_t n_bins, const int32_t* bin_chunk_ptr, int ncomp,
                     int c, double* out) {
  if (n_chunks > 0) {
    const int grid = std::min<int32_t>(n_chunks, 65536);
    hipLaunchKernelGGL(k_spec_bin, dim3(grid), dim3(256), 0, s, w, n_chunks, chunk_ptr, bin_points, parts);
    NSFEM_HIP(hipGetLastError());
  }
  const int grid = std::min<int32_t>((n_bins + 255) / 256, 8192);
  hipLaunchKernelGGL(k_spec_bin_sum, dim3(grid), dim3(256), 0, s, n_bins, bin_chunk_ptr, parts, ncomp, c, out);
  NSFEM_HIP(hipGetLastError());
}

}  // namespace nsfem
