// Internal declarations of libnsfem_hip.so (not part of the C ABI).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <cmath>
#include <string>
#include <type_traits>
#include <vector>
#include <stdexcept>
#include <functional>
#include <map>
#include <memory>
#include "../../include/nsfem.h"

// Knock-out switches of the measurement experiments (NSFEM_LATTICE_DBG, NSFEM_JL_DBG, NSFEM_SPMV_DEBUG: parts of the
// dominant kernels switched off, WRONG results): compiled in only with -DNSFEM_KNOCKOUTS=1 (scripts/build_knockouts.sh);
// in the product build NSFEM_KO(..) is the constant 0 and the environment variables are never read.
#ifndef NSFEM_KNOCKOUTS
#define NSFEM_KNOCKOUTS 0
#endif
#if NSFEM_KNOCKOUTS
#define NSFEM_KO(expr) (expr)
#else
#define NSFEM_KO(expr) (0)
#endif

namespace nsfem {

struct Error : std::runtime_error {
  int code;
  Error(int c, const std::string& m) : std::runtime_error(m), code(c) {}
};

#define NSFEM_HIP(expr)                                                              \
  do {                                                                               \
    hipError_t e_ = (expr);                                                          \
    if (e_ != hipSuccess)                                                            \
      throw ::nsfem::Error(NSFEM_ERR_HIP, std::string(#expr) + ": " +                \
                                              hipGetErrorString(e_));                \
  } while (0)

#define NSFEM_REQUIRE(cond, msg)                                                     \
  do {                                                                               \
    if (!(cond)) throw ::nsfem::Error(NSFEM_ERR_ARG, std::string(msg));              \
  } while (0)

// number of partial sums every reduction kernel emits (= its grid size); the
// consumer kernels re-reduce them in a fixed order => bitwise reproducible dots.
constexpr int kParts = 512;
constexpr int kPartSlots = 14;   // partial-sum slots of the Krylov work space (slots 10, 11: drivers; 12, 13: start sums |r0|^2, |b|^2)
constexpr int kBlock = 256;

template <class T>
struct DevBuf {
  T* p = nullptr;
  size_t n = 0;
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  DevBuf(DevBuf&& o) noexcept : p(o.p), n(o.n) { o.p = nullptr; o.n = 0; }
  ~DevBuf() { release(); }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    n = 0;
  }
  void alloc(size_t count) {
    release();
    n = count;
    // (+64 bytes of slack: the SpMV kernels read 16-byte aligned quads that may end past the last
    // entry of a column / value array)
    if (count) NSFEM_HIP(hipMalloc(&p, count * sizeof(T) + 64));
  }
  void upload(const T* host, size_t count, hipStream_t s) {
    if (count != n) alloc(count);
    if (count) NSFEM_HIP(hipMemcpyAsync(p, host, count * sizeof(T), hipMemcpyHostToDevice, s));
  }
  void upload(const std::vector<T>& v, hipStream_t s) {
    upload(v.data(), v.size(), s);
    NSFEM_HIP(hipStreamSynchronize(s));   // host vector may die after the call
  }
  void zero(hipStream_t s) {
    if (n) NSFEM_HIP(hipMemsetAsync(p, 0, n * sizeof(T), s));
  }
};

// ---- host-built sparsity pattern (CSR over block rows/cols) + slot map ---------
struct HostPattern {
  int n_rows = 0, n_cols = 0, nr = 0, nc = 0;   // nr/nc: local rows/cols per cell
  std::vector<int32_t> rowptr, col, diag;       // diag only for square patterns
  std::vector<int32_t> slot;                    // SoA: [nr*nc][n_cells]
  std::vector<int32_t> cptr, cidx;              // inverted index of the slot map (want_contrib)
};
int host_threads();                             // threads of the host set-up loops (NSFEM_HOST_THREADS)
void build_pattern(int n_rows, int n_cols, int n_cells, const int32_t* rowmap, int nr,
                   const int32_t* colmap, int nc, bool want_diag, HostPattern& out, bool want_contrib = false);

struct Pattern {
  int n_rows = 0, n_cols = 0, nnz = 0, nr = 0, nc = 0;
  DevBuf<int32_t> rowptr, col, diag, slot;
  DevBuf<int32_t> cptr, cidx;             // per slot: sources (cell * nr*nc + i * nc + j)
  DevBuf<int32_t> rblk1;                  // chunks of the CSR-stream SpMV: row-start table [n_rblk + 1]
  int n_rblk = 0;
  std::vector<int32_t> h_rblk;            // host copy (interior / halo-adjacent split)
  // partitioned meshes: the row blocks [int_b0, int_b1) reference no ghost column -- they can run
  // while the halo exchange of the input vector is still in flight (mark_interior_blocks)
  int int_b0 = 0, int_b1 = 0;
  // SELL-64 layout (sliced ELLPACK, slices of 64 rows = one wavefront, entries of a slice stored
  // column-major: lane r of a wave walks row r) for patterns whose consecutive rows have (nearly)
  // equal length -- structured numberings that group the P2 nodes by lattice-parity class.  The
  // k-th entries of 64 consecutive rows then sit at consecutive column ids: the x gather of a wave
  // is one contiguous run instead of ~50 scattered cache lines.  Built by build_sell when the
  // padding stays below a few per cent; n_slices = 0 otherwise (CSR-stream kernel).
  DevBuf<int32_t> sell_ptr;               // [n_slices + 1] entry offsets (multiples of 64)
  DevBuf<int32_t> sell_col;               // column ids, padding entries point at the row itself
  DevBuf<int32_t> sell_src;               // CSR slot of every entry, -1 = padding
  int n_slices = 0;
  int64_t sell_len = 0;
  int sell_w0 = 0, sell_w1 = 0;           // interior workgroups (4 slices each), see int_b0/int_b1
  int wg_w0 = 0, wg_w1 = 0;   // longest run of 256-row groups without a ghost column (dictionary kernel)
  // contiguous workgroup ranges of the 8 XCDs, balanced by (padded) nonzeros: the parity-class
  // numberings group rows of very different length (3D vertex rows 65, edge rows 14-32 entries),
  // an equal-count split would leave one XCD with 2-3 times the work of the others
  int sell_xcd[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  std::vector<int32_t> h_rowptr, h_col;   // kept for export
};
void build_rowblocks(Pattern& p, hipStream_t s);
// the same pattern, slot map and inverted index built on the device (pattern_device.hip); d_rowmap / d_colmap: SoA
// device copies of the cell dof maps [nr][n_cells] / [nc][n_cells]
void build_pattern_device(hipStream_t s, int n_rows, int n_cols, int n_cells, const int32_t* d_rowmap, int nr,
                          const int32_t* d_colmap, int nc, bool want_diag, Pattern& out);
// node-sorted layout of the element vectors (MeshDev::nptr, ndst) from the SoA device dof map [nl][n_cells]
void build_node_index_device(hipStream_t s, int n_nodes, int n_cells, int nl, const int32_t* d_map, DevBuf<int32_t>& nptr,
                             DevBuf<int32_t>& ndst);
void build_sell(Pattern& p, hipStream_t s);
// longest run of row blocks none of whose columns is flagged in `ghost_cols` ([n_cols] flags)
void mark_interior_blocks(Pattern& p, const std::vector<uint8_t>& ghost_cols);
void build_inverse_index(int n_targets, int64_t n_sources,
                         const std::function<int32_t(int64_t)>& target_of,
                         std::vector<int32_t>& ptr, std::vector<int32_t>& idx);

// block matrix on a pattern; vals[nnz][BR][BC] row-major blocks
// Stencil dictionary of a scalar matrix family on one pattern (structured meshes): rows whose
// (column offsets, values) agree to 2^-40 (of the largest entry) share one dictionary entry, so a product reads ONE
// 4-byte id per row instead of 12 bytes per nonzero -- on the lattice meshes of the benchmark
// configurations a P2 operator has a few dozen (2D) to a few thousand (3D, slab-blocked parity
// numbering) distinct rows.  Built once per pattern from the constant matrices it will combine
// (mass and stiffness: any a M + b K has the same dictionary); the value table of a matrix is a
// gather from the CSR values of the representative rows (dict_update, device only).  The
// compressed copy differs from the CSR matrix by the dedupe tolerance: unless `exact` it is used by
// multigrid SMOOTHING and Newton-Jacobian products only, never by a residual or a linear operator
// whose solution is returned.
struct StencilDict {
  int n_rows = 0, n_stencils = 0, lmax = 0;
  bool exact = false;      // every row equals its representative BITWISE (meshes with a binary spacing): the
                           // dictionary copy is the matrix itself and every product may use it
  int bsz = 1;             // doubles per entry (block matrices: br * bc)
  bool rect = false;       // offsets are relative to the row's FIRST column (rectangular P2 x P1 blocks:
                           // the two numberings differ), kept per row in cbase; square: relative to the row
  int max_local = 0;       // most entries any workgroup uses (sizes the LDS copy)
  DevBuf<int32_t> cbase;   // [n_rows] (rect only)
  DevBuf<int32_t> sid;     // [n_rows] dictionary entry of every row
  DevBuf<uint8_t> lid;     // [n_rows] its position in the list of the row's workgroup (256 rows)
  DevBuf<int32_t> wg_ptr, wg_list;   // per workgroup: the entries it uses (<= 32)
  DevBuf<int32_t> len;     // [n_stencils]
  DevBuf<int32_t> off;     // [n_stencils * lmax] column - row
  DevBuf<int32_t> src;     // [n_stencils * lmax] CSR position in the representative row (-1: padding)
  DevBuf<int32_t> dpos;    // [n_stencils] position of the diagonal entry inside the stencil (-1: none); the
                           // smoother kernels take 1 / diagonal from the table instead of streaming a dinv vector
  // 2D lattice structure (lexicographic numbering, row = j * lat_w + i): every offset is dj * lat_w + di
  // with |di|, |dj| <= lat_r and every row's entries stay inside the lat_w x lat_h box.  Set (lat_w > 0)
  // only for square scalar operators with <= 64 stencils: the multi-step lattice smoother
  // (k_cheb_lattice) keeps a tile of x in LDS and needs (dj, di) to address it.
  int lat_w = 0, lat_h = 0, lat_r = 0;
  DevBuf<int32_t> pack;    // [n_stencils * lmax] (dj + 8) * 32 + (di + 8)
  DevBuf<uint8_t> sid8;    // [n_rows] dictionary entry of every row as one byte
  std::vector<int32_t> h_pack, h_len;     // host copies (offset tables of the lattice kernel's LDS layouts)
  struct LatticeOffsets {
    int ewh = 0, ehh = 0;
    DevBuf<int32_t> buf;   // [n_stencils][4 classes][lmax]
  };
  mutable std::vector<LatticeOffsets> loff_cache;   // one table per tile shape in use (built on first use)
  mutable DevBuf<uint8_t> sidm_scratch;             // entry | mask bytes for callers that bring none (test hook, timing)
  // entries with the canonical interior stencil shape of a parity class (launch_cheb_lattice: compile-time LDS
  // offsets): shape 0 = not looked at yet, -1 = none, 1 = P2 right-diagonal lattice, 2 = P1 7-point
  mutable int fixed_shape = 0;
  mutable unsigned long long fixed_mask[4] = {0, 0, 0, 0};
};
// false: the rows do not repeat (unstructured mesh) -- no dictionary
void ensure_fixed_masks(const StencilDict& d);   // fills d.fixed_shape / fixed_mask (entries of canonical interior shape)
bool build_stencil_dict(hipStream_t s, const Pattern& p, const double* dev_a, const double* dev_b,
                        StencilDict& d, int bsz = 1, bool rect = false);

struct BlockMat {
  const Pattern* pat = nullptr;
  int br = 1, bc = 1;
  DevBuf<double> vals;
  const StencilDict* dict = nullptr;      // set: sell_update() also refreshes dict_vals
  DevBuf<double> dict_vals;               // [n_stencils * lmax]
  DevBuf<double> dict_dinv;               // [n_stencils] 1 / diagonal (scalar square operators)
  DevBuf<double> lat_vals;                // [n_stencils * lp] zero-padded rows for the lattice kernel
  bool dict_ready = false;
  // copy of the values in the pattern's SELL-64 order (scalar matrices on patterns that have one);
  // refreshed by sell_update() after every change of `vals` -- the SpMV kernels use it only while
  // sell_ready is set
  DevBuf<double> sell_vals;
  bool sell_ready = false;
  void init(const Pattern* p, int br_, int bc_, hipStream_t s) {
    pat = p; br = br_; bc = bc_;
    vals.alloc((size_t)p->nnz * br * bc);
    vals.zero(s);
    sell_ready = false;
  }
  void sell_update(hipStream_t s);        // linalg.hip
};

// reference-element tables (7-point degree-5 rule)
struct QuadTables {
  double w[7];
  double phi2[7][6];
  double dphi2[7][6][2];
  double phi1[7][3];
  // dphi1 is constant: (-1,-1), (1,0), (0,1)
  // CFL diagnostic: P2 basis at the 6 points of the degree-4 Strang-Fix rule and its inverse
  // (the local L2 projection onto P2 with that rule is interpolation at its points)
  double cfl_phi[6][6];
  double cfl_inv[6][6];
};
void fill_quad_tables(QuadTables& t);
void upload_quad_tables(const QuadTables& t);
struct MeshDev;
void launch_cfl(hipStream_t s, const MeshDev& m, const double* u, double scale, double* parts,
                int n_parts);

// SpMV row-mask modes
enum MaskMode { MASK_NONE = 0, MASK_IDENTITY = 1, MASK_ZERO = 2 };
// SpMV epilogues (described at the kernels, linalg.hip)
enum Epi { EPI_STORE = 0, EPI_RESID = 1, EPI_ACCUM = 2, EPI_CHEB = 3, EPI_RESID_SUM = 4 };
// The kernel family a product with A runs on.  spmv_path is the ONE statement of the rule ("Which kernel
// family a product runs on"): the dispatcher switches on it, the fused launches state their preconditions through it
// and the test hook reports it.
// phase, dict_ok: as for launch_spmv below; second_output: EPI_STORE with the fused first smoothing step (y2)
enum class SpmvPath { DictBlock, DictScalar, Sell, Stream, LaneGroup };
SpmvPath spmv_path(const BlockMat& A, int nv, int epi, int phase, bool dict_ok, bool second_output);

// -------------------------- kernel launch wrappers ------------------------------
// y = A x.  nv = number of interleaved right-hand sides the scalar blocks act on
// (scalar P2 matrices applied to both velocity components use br=bc=1, nv=2).
// ghost: treatment of rows flagged 2 (ghost rows of a partitioned mesh): 0 output 0, 2 computed
// phase (partitioned meshes, halo exchange overlapped with the product): 0 all rows, 1 only the
// row blocks that touch no ghost column (Pattern::int_b0..int_b1), 2 the remaining row blocks
// dict_ok: the product may run on the matrix's stencil-dictionary copy (equal to the CSR values to
// 2^-40 of the largest entry): Newton-Jacobian products and smoothing steps only
void launch_spmv(hipStream_t s, const BlockMat& A, int nv, const double* x, double* y,
                 const uint8_t* rowmask, int maskmode, int ghost = 0, int phase = 0, int dict_ok = 0);
bool launch_spmv_with_gather(hipStream_t s, const BlockMat& A, int nv, const double* x, double* y,
                             const uint8_t* rowmask, int maskmode, const int32_t* gptr, const double* gbuf);
void launch_spmv_cheb_first(hipStream_t s, const BlockMat& A, int nv, const double* x, double* y,
                            const uint8_t* rowmask, const double* dinv, double c2, double* d,
                            double* x1);
// y = b - A x  (same arguments + b)
void launch_residual(hipStream_t s, const BlockMat& A, int nv, const double* x,
                     const double* b, double* y, const uint8_t* rowmask, int maskmode, int phase = 0);

// y += A x (masked rows -> 0);  Chebyshev/Jacobi smoother step
//   d = c1 d + c2 dinv (b - A x) ; xout = x + d   (masked rows -> 0)
void launch_spmv_accumulate(hipStream_t s, const BlockMat& A, int nv, const double* x, double* y,
                            const uint8_t* rowmask, int ghost = 0 /* 2: ghost rows accumulate too */);
// y = scale * A x ;  y += scale * A x on rows not flagged in skipmask (flagged rows untouched)
void launch_spmv_scaled(hipStream_t s, const BlockMat& A, int nv, double scale, const double* x,
                        double* y, int dict_ok = 0);
void launch_spmv_axpy(hipStream_t s, const BlockMat& A, int nv, double scale, const double* x,
                      double* y, const uint8_t* skipmask, int dict_ok = 0);
void launch_cheb_step(hipStream_t s, const BlockMat& A, int nv, const double* x, const double* b,
                      const double* dinv, double* d, double c1, double c2, double* xout,
                      const uint8_t* rowmask, int ghost = 0 /* 1: ghost rows keep x */, int phase = 0,
                      int ident = 0 /* 1: rows flagged 1 take xout = b (identity rows) */);

// Fused launches of the step frame (NSFEM_STEP_FUSED, linalg.hip); each reproduces the launches it replaces bit for bit
// q = r - A z and psum = base + z (scalar dictionary kernel, no mask); false: no exact dictionary copy, nothing launched
bool launch_residual_sum(hipStream_t s, const BlockMat& A, const double* z, const double* r, double* q,
                         const double* base, double* psum);
// M (scalar P2 x P2, two interleaved components) and B (2 x 1 blocks, P2 rows) both run on exact dictionaries today
bool spmv_pair_available(const BlockMat& M, const BlockMat& B);
void launch_spmv_pair_accum(hipStream_t s, const BlockMat& M, const BlockMat& B, const double* x, double c2,
                            const double* z, double* y);                          // y = M x + c2 B z
void launch_spmv_pair_correction(hipStream_t s, const BlockMat& M, const BlockMat& B, const double* x, double a,
                                 const double* z, const double* z2, const uint8_t* mask, double* rhs, double* r0);
bool newton_fused_enabled();            // NSFEM_NEWTON_FUSED (and not NSFEM_GRAPHS) as last read by refresh_env_switches
bool step_fused_enabled();              // NSFEM_STEP_FUSED as last read by refresh_env_switches

// multi-step lattice smoother (2D lexicographic lattices with a stencil dictionary; linalg.hip)
void refresh_env_switches();            // NSFEM_LATTICE, NSFEM_LATTICE_TRANSFERS (re-read by nsfem_create)
void refresh_assembly_switches();       // NSFEM_JAC_LATTICE
bool lattice_transfers_enabled();
bool lattice_smoother_available(const BlockMat& A, int nv);
int lattice_smoother_max_steps(const BlockMat& A, bool from_zero, bool with_resid);
// test hook only: forced launch choices in, the geometry of the launch out
struct LatticeLaunchOverride {
  int tile_lines = 0;       // 0: the launcher's choice; 16, 24, 32, 48: forced (refused when the halo does not fit)
  int fixed = -1;           // -1: the launcher's choice (on); 0 / 1: compile-time-offset stages off / on
  int generic = 0;          // 1: the runtime-flag kernel even where the launch kind has a specialised instantiation
  int used_tile_lines = 0, tx = 0, ty = 0, tiles = 0, fixed_shape = 0;   // out
  int kind = 0;             // out: the launch kind that ran (lattice_launch_kind; 0: the runtime-flag kernel)
};
// launch kind of k_cheb_lattice for these operands: LK_FIXED (64) | operand flags (x_in 1, xc 2, rf 4, d_in 8, d_out 16,
// r_out 32) where a specialised instantiation exists, else 0
int lattice_launch_kind(bool x_in, bool xc, bool rf, bool d_in, bool d_out, bool r_out, bool ghost);
// do the lattice's vectors (w x h nodes, nv components; with rf also the finer lattice's) fit 32-bit byte offsets?
bool lattice_offsets_fit(int64_t w, int64_t h, int nv, bool rf);
void launch_cheb_lattice(hipStream_t s, const BlockMat& A, int nv, const double* x_in, const double* b,
                         const double* d_in, double* x_out, double* d_out, double* r_out,
                         const uint8_t* mask, int steps, const double* c1, const double* c2, int ident,
                         const uint8_t* sidm = nullptr, const double* xc = nullptr, const double* rf = nullptr,
                         double* b_out = nullptr, int gh_lo = 0, int gh_hi = 0, int gh_zero = 0,
                         LatticeLaunchOverride* ovr = nullptr);
// out[row] = dictionary entry | (mask of component c) << (6 + c): one byte per row for the lattice kernel
void launch_lattice_sidm(hipStream_t s, const BlockMat& A, int nv, const uint8_t* mask, uint8_t* out);
// out = R rf on a lattice hierarchy (rows flagged in the coarse mask: 0); false = shapes do not nest, nothing launched
bool launch_restrict_lattice(hipStream_t s, int nv, int Wc, int Hc, int Wf, int Hf, const double* rf,
                             const uint8_t* mask, double* out);
// two levels of a restriction chain in one launch: b1 = R1 rf, b2 = R2 b1
bool launch_restrict_lattice2(hipStream_t s, int nv, int W2, int H2, int W1, int H1, int Wf, int Hf,
                              const double* rf, const uint8_t* mask1, const uint8_t* mask2, double* b1, double* b2);

int64_t lattice_launch_bytes(const BlockMat& A, int nv, bool from_zero, bool d_in, bool d_out, bool r_out);

// element kernels
// 2D lattice meshes in rectangle_mesh numbering (cell 2 (sy nx + sx) + t, P2 node j W + i): the node positions of
// a cell are a template of its type -- verified cell by cell on the host (build_cell_lattice), used by k_jac_lattice
struct CellLattice {
  bool ok = false, tried = false;
  int nx = 0, ny = 0, W = 0, H = 0;
  int di[2][6] = {{0}}, dj[2][6] = {{0}};   // lattice offset of local node k of cell type t from the square's corner
  int rank[2][6] = {{0}};                   // position of the cell among the cells around that node (ascending)
  // uniform lattices (every cell of a type has the geometry of the first one BIT FOR BIT -- checked on the device
  // with the kernels' own load_geo): {J^-1, |det|} of the two cell types; the one-launch kernel then takes the
  // geometry from 10 scalar loads instead of six strided coordinate loads per cell (48 B per cell of the launch)
  bool geo_uniform = false;
  DevBuf<double> ugeo;                      // [2][5]
  // and, from them, the physical basis gradients and weights of both types (phys() once per type, the same bits as
  // per cell): [type][kGradTab] = gx, gy [7][6][2], then c_q.w[q] |det| [7]
  DevBuf<double> gtab;
};
constexpr int kGradTab = 96;              // doubles per cell type (84 gradients + 7 weights, padded)
bool build_cell_lattice(const int32_t* p2map /* [cell][6] */, int nc, int W, int H, CellLattice& cl);
struct MeshDev;
void check_uniform_geometry(hipStream_t s, MeshDev& m);   // fills m.cl.geo_uniform / ugeo / gtab (after build_cell_lattice)
// cells whose phys() gradients or weights differ from m.cl.gtab (-1: no tables); test hook
int64_t check_gradient_tables(hipStream_t s, const MeshDev& m);
// k_jac_lattice variant the next launch takes: 0 the round-4 kernel (NSFEM_JL_KERNEL=0), 1 one cell type per wave and
// node sums by gather, 2 the same with gradient tables (uniform lattices)
int jacobian_lattice_variant(const MeshDev& m);

struct MeshDev {
  int dim = 2;              // 2: triangles (6 + 3 nodes per cell), 3: tetrahedra (10 + 4)
  int n_cells = 0, n_p2 = 0, n_p1 = 0, n_vertices = 0;
  DevBuf<double> vx;        // SoA vertex coords per cell: [6][n_cells] (x0,y0,x1,y1,x2,y2)
  DevBuf<int32_t> p2;       // SoA [6][n_cells]
  DevBuf<int32_t> p1;       // SoA [3][n_cells]
  // vector assembly without atomics: the element vectors are stored NODE-SORTED -- entry (cell, i)
  // goes to position ndst[i][cell] (SoA [6 | 10][n_cells]) of rbuf, the contributions of node n are
  // the contiguous run nptr[n] .. nptr[n + 1] (ascending cell order: deterministic sums, and the
  // gather kernel streams the buffer instead of chasing 16 / 24-byte pieces through it)
  DevBuf<int32_t> nptr, ndst;
  DevBuf<double> ebuf;      // element Jacobian blocks [cell][6][6][4] (plain stores)
  DevBuf<double> rbuf;      // element residual [cell][6][2]
  CellLattice cl;
};
void launch_assemble_p2_scalar(hipStream_t s, const MeshDev& m, const Pattern& p22,
                               double* mass, double* stiff);
// tetrahedral meshes (assembly3d.hip); the launch_* wrappers dispatch on MeshDev::dim
struct QuadTables3 {          // 15-point degree-5 Keast rule, P2 (10 nodes) / P1 (4 nodes) tables
  double w[15];
  double phi2[15][10];
  double dphi2[15][10][3];
  double phi1[15][4];
};
void fill_quad_tables_3d(QuadTables3& t);
void upload_quad_tables_3d();
void launch_cfl_3d(hipStream_t s, const MeshDev& m, const double* u, double scale, double* parts,
                   int n_parts);
// extreme eigenvalues of diag(M_e)^{-1} M_e for the P2 element mass matrix (Wathen: they bound
// the spectrum of the Jacobi-scaled assembled mass matrix on any affine mesh)
void p2_mass_jacobi_bounds(int dim, double& lmin, double& lmax);
// max_i K_ii / M_ii of two scalar matrices on the same pattern (stored diagonals)
double diag_ratio_max(hipStream_t s, const Pattern& pat, const double* M, const double* K, double* parts);
void assemble_p2_scalar_3d(hipStream_t s, const MeshDev& m, const Pattern& p22, double* mass,
                           double* stiff);
void assemble_p1_scalar_3d(hipStream_t s, const MeshDev& m, const Pattern& p11, double* stiff,
                           double* mass);
void assemble_div_grad_3d(hipStream_t s, const MeshDev& m, const Pattern& p12, const Pattern& p21,
                          double* div, double* grad, double* divT);
void jacobian_init_3d(hipStream_t s, int nnz, const double* L, const double* E, double cvE,
                      double* J);
void assemble_viscous_extra_3d(hipStream_t s, const MeshDev& m, const Pattern& p22, double* extra);
void convection_jacobian_3d(hipStream_t s, const MeshDev& m, const Pattern& p22, const double* u,
                            double cc, const double* L, const double* E, double cvE, double* J,
                            int form, bool picard);
void convection_residual_3d(hipStream_t s, const MeshDev& m, const double* u, double cc, double* b,
                            int form, const double* gam = nullptr);
void convection_action_3d(hipStream_t s, const MeshDev& m, const double* u, const double* v,
                          double cc, double* y, int form, bool picard, const uint8_t* skipmask = nullptr);
void launch_assemble_p1_scalar(hipStream_t s, const MeshDev& m, const Pattern& p11,
                               double* stiff, double* mass);
void launch_assemble_div_grad(hipStream_t s, const MeshDev& m, const Pattern& p12,
                              const Pattern& p21, double* div, double* grad, double* divT);
void launch_assemble_viscous_extra(hipStream_t s, const MeshDev& m, const Pattern& p22,
                                   double* extra);
// J(2x2 blocks) = L (scalar) (x) I_2 [+ cv_extra * E]  then  += cc * conv'(u)
void launch_jacobian_init(hipStream_t s, int dim, int nnz, const double* L, const double* E,
                          double cvE, double* J);
// J = L (x) I_2 + cvE * E + cc * conv'(u): element blocks are stored, then gathered per slot
void launch_convection_jacobian(hipStream_t s, const MeshDev& m, const Pattern& p22,
                                const double* u, double cc, const double* L, const double* E,
                                double cvE, double* J, int form, bool picard);
// skipmask != nullptr: vector entries with a nonzero flag are left untouched by the node gather
void launch_convection_action(hipStream_t s, const MeshDev& m, const double* u, const double* v,
                              double cc, double* y, int form, bool picard,
                              const uint8_t* skipmask = nullptr);
// only the element kernel of the action: the element vectors land node-sorted in m.rbuf (runs m.nptr); the
// caller sums them per node (launch_spmv_with_gather)
bool launch_residual_lattice(hipStream_t s, const MeshDev& m, const BlockMat& L, const double* u, const double* g,
                             double cc, int form, double* y);   // y = L u + g + c_c conv(u) (exact dictionaries)
// y = L x + c_c [d conv(u)/du] x, identity on the rows flagged in mask: ONE launch on 2D lattice meshes (m.cl.ok and a
// lattice stencil dictionary of L); false = not available, nothing launched
bool jacobian_lattice_available(const MeshDev& m, const BlockMat& L);
int64_t jacobian_lattice_bytes(const MeshDev& m);   // u, x read, y written, ids + masks, vertex coordinates
bool launch_jacobian_lattice(hipStream_t s, const MeshDev& m, const BlockMat& L, const double* u, const double* x,
                             double cc, int form, bool picard, const uint8_t* mask, double* y, int phase = 0,
                             int gh_lo = 0, int gh_hi = 0);
// IMEX right-hand side (nsfem_step_imex): with t = (L1 u1 + L2 u2) + g and n1 = 0 + c_c conv(u1) (the node sums of
// launch_convection_residual on a zeroed vector)
//   rhs = -(t + (b0 n1 + b1 n2))      (imex_rhs_value; n2 is not read when have_n2 is false)
// and n1 is stored.  launch_imex_rhs_lattice: ONE launch of k_jac_lattice<FORM, 3> on 2D lattice meshes whose
// dictionary equals the assembled matrices bit for bit (false = not available, nothing launched); it reproduces the
// generic sequence -- launch_spmv (L1, L2), launch_axpby twice, launch_convection_residual, launch_imex_combine --
// bit for bit.  L1, L2 share L's pattern and dictionary.  ghostmask set (the strip of a partitioned mesh, after the
// ghost lines of u1 and u2 were exchanged): k_jac_lattice<FORM, 4>, rows of ghost nodes get rhs = 0 and n1 = 0.
// gam != 0 (rotating frame, nsfem_set_imex_rotation): k_jac_lattice<FORM, 5 / 6>, n1 = c_c conv(u1) + M (gam e_z x u1)
// from the same element kernel -- as launch_convection_residual with gam forms it.
struct ImexLatArgs {
  const double* u2 = nullptr;      // velocity at t_(n-1)
  const double* sval2 = nullptr;   // dictionary values of L2
  const double* n2 = nullptr;      // c_c conv(u2) (null: not read)
  double* n1 = nullptr;            // c_c conv(u1), written
  double b0 = 1.0, b1 = 0.0;
  double gam = 0.0;                // 2 c_cor omega(t^n): read by the rotating modes (LIN 5, 6) only
  // the frame of the Newton iteration (LIN 7, 8; launch_residual_frame_lattice): read by those modes only
  const double* gd = nullptr;      // Dirichlet values as a dense velocity vector
  double* unew = nullptr;          // LIN 8: u - x, written
  double* tparts = nullptr;        // one sum of squares per tile, written
};
// The momentum residual with its Dirichlet rows, the sum of its squares per tile and, with dx set, the Newton update
// u - dx (stored to unew) in ONE launch; false = not available, nothing launched.  Comment at the definition
int lattice_tile_count(const MeshDev& m);
bool residual_frame_lattice_available(const MeshDev& m, const BlockMat& L);
bool launch_residual_frame_lattice(hipStream_t s, const MeshDev& m, const BlockMat& L, const double* u, const double* dx,
                                   double* unew, const double* g, double cc, int form, const uint8_t* mask,
                                   const double* gdense, double* y, double* tparts);
bool launch_imex_rhs_lattice(hipStream_t s, const MeshDev& m, const BlockMat& L1, const BlockMat& L2, const double* u1,
                             const double* u2, const double* g, double cc, int form, double b0, double b1,
                             const double* n2, double* n1, double* rhs, const uint8_t* ghostmask = nullptr,
                             int phase = 0, int gh_lo = 0, int gh_hi = 0, double gam = 0.0);
// every precondition of launch_imex_rhs_lattice that depends on the mesh and the operators (the ranks of a partitioned
// run agree on the path once, from this)
bool imex_rhs_lattice_available(const MeshDev& m, const BlockMat& L1, const BlockMat& L2);
void launch_imex_combine(hipStream_t s, int64_t n, const double* t, const double* n1, const double* n2, double b0,
                         double b1, double* rhs);
// partitioned strips: can the launch be cut into tile rows that read no ghost line (phase 1, under the halo
// exchange) and the rest (phase 2)?
bool jacobian_lattice_split(const MeshDev& m, int gh_lo, int gh_hi);
// are the ghost nodes of a W x H lattice whole lines at its bottom (lo of them) and top (hi)?
bool ghost_lattice_lines(const std::vector<uint8_t>& ghost, int W, int H, int& lo, int& hi);
void launch_convection_cells(hipStream_t s, const MeshDev& m, const double* u, const double* v, double cc,
                             int form, bool picard);
// gam (null: none): 2 c_cor Omega, 1 double in 2D and 3 in 3D -- the element kernel adds M (gam x u) to the node sums
// (the explicit Coriolis vector of the IMEX step; weighted by the quadrature weights alone, so it survives cc = 0)
void launch_convection_residual(hipStream_t s, const MeshDev& m, const double* u, double cc,
                                double* b, int form, const double* gam = nullptr);
// scalar transport (nsfem_step_scalar_imex): out = weight * C(u) T for the P2 scalar T on the velocity nodes, form 0
// standard C_ij = int (u . grad phi_j) phi_i, 1 skew-symmetric 1/2 (C - C^T) -- element kernel (k_scalar_conv_cell /
// k3_scalar_conv_cell, node-sorted element vectors in m.rbuf) plus the per-node sums in ascending cell order.
// Subgrid heat flux (nsfem_set_scalar_sgs): the launchers take ScalarSgsArgs by value.  law 1, 4 or 5 (Smagorinsky,
// WALE, Vreman): the same launch adds D(u, T), the eddy diffusivity kappa_x = nu_x inv_prt of that law with its
// constant c0 (C_s, C_w, c) under the gradients (the SGS = law instantiations), out = weight (C(u) T + D(u, T));
// law 0: the term is off, the SGS = 0 kernels, which take nothing.  law 8 (nsfem_set_scalar_sgs_dynamic): kappa_x =
// c_K Delta_K^2 gamma with c_K from cthv, the vertex field C_theta of launch_dynamic_constant on the same level
// pair (u, T); no Pr_t, c0 and inv_prt are not read
struct ScalarSgsArgs {
  double c0 = 0.0, inv_prt = 0.0;
  int32_t law = 0;
  int32_t pad_ = 0;
  const double* cthv = nullptr;
};
// ... and what the kernels take: the two numbers with SGS = 1, 4, 5, the P1 connectivity and the vertex field with
// SGS = 8, nothing at all with SGS = 0
template <int SGS>
struct ScalarSgsKernelArgs {
  double c0, inv_prt;
};
template <>
struct ScalarSgsKernelArgs<0> {};
template <>
struct ScalarSgsKernelArgs<8> {
  const int32_t* vtx;
  const double* cthv;
};
// variable viscosity (nsfem_set_viscosity_law; law 1 Smagorinsky, 2 Carreau, 4 WALE, 5 Vreman, p = params): the element kernel
// k_visc_var_cell / k3_visc_var_cell on the velocity u, element vectors weight * V_K(u) node-sorted into m.rbuf --
// mean: the cell means of nu_x into the first n_cells doubles of m.rbuf instead
// law 8 (dynamic Smagorinsky): cs2v = the vertex field C_s^2 of launch_dynamic_constant on the same u; null for every
// other law
void launch_viscosity_cells(hipStream_t s, const MeshDev& m, const double* u, double weight, int law,
                            const double p[4], bool mean, const double* cs2v = nullptr);
void viscosity_cells_3d(hipStream_t s, const MeshDev& m, const double* u, double weight, int law, const double p[4],
                        bool mean, const double* cs2v);
// The device side of the Germano-Lilly procedure (assembly.hip / assembly3d.hip): three launches, cell moments, vertex
// patches, group sums with the clip.  Two uses:
//   T null   dynamic Smagorinsky (law 8) on the velocity u -- k_dyn_moments, k_dyn_vertex, k_dyn_reduce; vert rows W,
//            LM, MM; sums rows num, den, cs2; cs2v = C_s^2 at the vertices, what launch_viscosity_cells and
//            launch_wall_facets read with law 8; clip = cs2_max
//   T given  dynamic subgrid heat flux (nsfem_set_scalar_sgs_dynamic), the Germano identity of the scalar flux on the
//            level pair (u, T) -- k_dyn_scalar_moments, k_dyn_scalar_vertex, k_dyn_reduce; vert rows W, PR, RR; sums
//            rows num, den, ctheta; cs2v = C_theta at the vertices; clip = ctheta_max
// vptr, vcell: the vertex-to-cell CSR (ascending cells); goff [n_groups + 1], gvert [n_p1]: the group-sorted vertex
// list -- shared by the two uses; mom [dynamic_moment_rows][n_cells], vert [n_p1][3], sums [n_groups][3], cs2v [n_p1]:
// each use has its own
struct DynamicDev {
  int n_groups = 0;
  const int32_t *vptr = nullptr, *vcell = nullptr, *goff = nullptr, *gvert = nullptr;
  double *mom = nullptr, *vert = nullptr, *sums = nullptr, *cs2v = nullptr;
};
// Lagrangian averaging (nsfem_set_dynamic_averaging mode 1): k_dyn_lagrange<DIM> in the place of k_dyn_reduce -- one
// application of rules 1 to 5 of include/nsfem.h to the state Iold [n_p1][2] = I_LM, I_MM of the level before (null:
// the initialisation rule), step size k; writes Inew (another buffer), the vertex field d.cs2v and, where up is not
// null, the upstream pair [n_p1][2].  vertex_only: the first two launches alone (the vertex rows for the output hook)
struct DynamicLagrangeDev {
  const double* Iold = nullptr;
  double k = 0.0, theta = 1.5, cs2_init = 0.0256, cs2_floor = 1e-12;
  double *Inew = nullptr, *up = nullptr;
  bool vertex_only = false;
};
void launch_dynamic_constant(hipStream_t s, const MeshDev& m, const double* u, const double* T, double alpha,
                             double clip, const DynamicDev& d, const DynamicLagrangeDev* lag = nullptr);
void dynamic_moments_3d(hipStream_t s, const MeshDev& m, const double* u, const double* T, double* mom);
// rows of mom: DIM + 3 NS + 2 on u (13 | 23), 1 + 4 DIM + NS + 2 on (u, T) (14 | 21), NS = DIM (DIM + 1) / 2
constexpr int dynamic_moment_rows(int dim, bool with_T) {
  const int ns = dim * (dim + 1) / 2;
  return (with_T ? 1 + 4 * dim + ns : dim + 3 * ns) + 2;
}
// k_visc_gather: v = per-node sums of m.rbuf in ascending cell order; n1 += v, rhs -= b0 v (rhs may be null)
void launch_viscosity_gather(hipStream_t s, const MeshDev& m, double b0, double* n1, double* rhs);
// immersed bodies (nsfem_set_bodies): the table the penalisation kernels take as a kernel ARGUMENT (1.6 kB; entries
// are read with wave-uniform indices).  size: kind 1 {r}, kind 2 half widths, kind 3 the unit normal; 2D reads
// angular[2].  eps the smoothing half width (0: every mask sharp), inv_eta = 1 / eta
struct BodyTable {
  int32_t n = 0;
  int32_t kind[NSFEM_MAX_BODIES] = {};
  int32_t pad_ = 0;                  // (no padding bytes: the table is compared with memcmp)
  double centre[NSFEM_MAX_BODIES][3] = {}, size[NSFEM_MAX_BODIES][3] = {};
  double velocity[NSFEM_MAX_BODIES][3] = {}, angular[NSFEM_MAX_BODIES][3] = {};
  double eps = 0.0, inv_eta = 0.0;
};
// heated bodies (nsfem_set_body_temperatures): flag theta_s in {0, 1} and temperature T_s per body of the table,
// inv_eta = 1 / eta_T.  A kernel argument beside the BodyTable, read with the same wave-uniform indices.  Rows of
// passive bodies hold temperature 0, so that what is compared (memcmp; store_thermal, api.hip) is what the kernels
// can see
struct ThermalTable {
  int32_t n = 0;
  int32_t flag[NSFEM_MAX_BODIES] = {};
  int32_t pad_ = 0;                  // (no padding bytes)
  double temperature[NSFEM_MAX_BODIES] = {};
  double inv_eta = 0.0;
};
// what the scalar convection kernels take when they add H(T): nothing at all without it (PENAL 0)
template <int PENAL>
struct ScalarPenalArgs {
  BodyTable bt;
  ThermalTable th;
};
template <>
struct ScalarPenalArgs<0> {};
// the pose that belongs to the level of T and the thermal table: what a launch with heated bodies takes
struct ScalarBodies {
  const BodyTable& bt;
  const ThermalTable& th;
};
// f(std::integral_constant<int, V>) for the V that equals v; the LAST V stands for every other value
template <int V0, int... Vs, class F>
inline void with_int(int v, F&& f) {
  if constexpr (sizeof...(Vs) == 0) f(std::integral_constant<int, V0>{});
  else if (v == V0) f(std::integral_constant<int, V0>{});
  else with_int<Vs...>(v, f);
}
// The viscosity laws (nsfem_set_viscosity_law), written ONCE: 0 constant, 1 Smagorinsky, 2 Carreau, 4 WALE, 5 Vreman,
// 8 dynamic Smagorinsky.  with_int lets its last value stand for every other one, so a caller asks is_viscosity_law
// first
template <class F>
inline void with_viscosity_law(int law, F&& f) {
  with_int<0, 1, 2, 4, 5, 8>(law, f);
}
inline bool is_viscosity_law(int law) {
  bool is = false;
  with_viscosity_law(law, [&](auto lc) { is = law == decltype(lc)::value; });
  return is;
}
// ... and the subgrid laws among them that take a fixed Pr_t as the partner of the subgrid heat flux
inline bool is_subgrid_law(int law) { return law == 1 || law == 4 || law == 5; }
// f(LAW, MEAN) for the element kernels of a variable viscosity, k_visc_var_cell / k3_visc_var_cell <LAW, MEAN>: every
// law but 0, which has no such kernel
template <class F>
inline void with_variable_law(int law, bool mean, F&& f) {
  with_viscosity_law(law, [&](auto lc) {
    if constexpr (decltype(lc)::value != 0) with_int<1, 0>(mean, [&](auto mc) { f(lc, mc); });
  });
}
// The ONE place that turns the run-time (form, PENAL, law) of a scalar element launch into template arguments:
// f(FORM, PENAL, SGS) gets three integral constants, so each translation unit holds one launch of k_scalar_conv_cell
// <FORM, PENAL, SGS> / k3_scalar_conv_cell -- 2 forms x 3 PENAL x 5 SGS (the subgrid laws 1, 4, 5, the dynamic
// diffusivity 8; 0 for all else)
template <class F>
inline void with_scalar_kernel(int form, int penal, int law, F&& f) {
  with_int<0, 1>(form, [&](auto fc) {
    with_int<0, 1, 2>(penal, [&](auto pc) { with_int<1, 4, 5, 8, 0>(law, [&](auto lc) { f(fc, pc, lc); }); });
  });
}
// (PENAL 0 and SGS 0 are the code of every run without temperatures / without the term: their kernels take nothing)
template <int PENAL>
inline ScalarPenalArgs<PENAL> scalar_penal_args(const ScalarBodies* hb) {
  if constexpr (PENAL == 0) return {};
  else return {hb->bt, hb->th};
}
template <int SGS>
inline ScalarSgsKernelArgs<SGS> scalar_sgs_kernel_args(const ScalarSgsArgs& a, const int32_t* p1) {
  if constexpr (SGS == 0) return {};
  else if constexpr (SGS == 8) return {p1, a.cthv};
  else return {a.c0, a.inv_prt};
}
// out = weight (C(u) T + D(u, T) + H(T)): the fused element kernel k_scalar_conv_cell<FORM, PENAL, SGS> /
// k3_scalar_conv_cell plus k_scalar_gather.  hb null: no heated bodies, PENAL 0; else PENAL 1 (sharp masks, bt.eps = 0)
// or 2 (smoothed), bt the pose that belongs to the level of T
void launch_scalar_convection(hipStream_t s, const MeshDev& m, const double* u, const double* T, double weight,
                              int form, const ScalarBodies* hb, double* out, ScalarSgsArgs sgs = ScalarSgsArgs{});
void scalar_convection_cells_3d(hipStream_t s, const MeshDev& m, const double* u, const double* T, double weight,
                                int form, int penal, const ScalarBodies* hb, ScalarSgsArgs sgs);
// k_body_heat + k_fold_partials (bodies.hip): out[s][3] = {int chi_s, Q_s, int chi_s T} in device memory, parts
// [n 3 kBodyParts] work space
void launch_body_heat(hipStream_t s, const MeshDev& m, const double* T, const BodyTable& bt, const ThermalTable& th,
                      double* parts, double* out);
// numbers per body of nsfem_body_forces: volume, dim force components, 1 (2D) or 3 torque components
inline int body_numbers(int dim) { return dim == 2 ? 4 : 7; }
constexpr int kBodyParts = 256;
// k_penal_cell / k3_penal_cell on the velocity u: element vectors (weight / eta) B_K(u) node-sorted into m.rbuf, to be
// summed by launch_viscosity_gather -- mean: the cell means of chi into the first n_cells doubles of m.rbuf instead
void launch_penalty_cells(hipStream_t s, const MeshDev& m, const double* u, double weight, const BodyTable& bt,
                          bool mean);
void penalty_cells_3d(hipStream_t s, const MeshDev& m, const double* u, double weight, const BodyTable& bt, bool mean);
// k_penal_forces + k_fold_partials (bodies.hip): out[s][body_numbers] in device memory, parts
// [n body_numbers kBodyParts] work space
void upload_body_tables(int dim);
void launch_penalty_forces(hipStream_t s, const MeshDev& m, const double* u, const BodyTable& bt, double* parts,
                           double* out);
// out[n dim + c] = f[n dim + c] + T[n] b[c] on the P2 nodes (f null: out = T b)
void launch_buoyancy_force(hipStream_t s, const MeshDev& m, const double* f, const double* T, const double b[3],
                           double* out);
// per-facet surface force / flux / measure (boundary.hip): out[nf][dim + 2]
void launch_boundary_force(hipStream_t s, const MeshDev& m, int nf, const int32_t* fcell,
                           const int32_t* flocal, const double* u, const double* p, double nu,
                           double sym, double* out);
// volume functionals (functionals.hip): the NSFEM_N_FUNCTIONALS integrals of include/nsfem.h over the cells whose
// flag is nonzero (flags null: all cells), of (u, p) or, with ur / pr set, of (u - ur, p - pr).  parts:
// [NSFEM_N_FUNCTIONALS][kVolParts] work space, out: [NSFEM_N_FUNCTIONALS], both in device memory
constexpr int kVolParts = 1024;
void upload_functional_tables(int dim);
// k_fold_partials (functionals.hip): out[b] = the sum of parts[b][0 .. n_parts) in a fixed order, n_parts a multiple of 64
void launch_fold_partials(hipStream_t s, int n_numbers, int n_parts, const double* parts, double* out);
void launch_vol_functionals(hipStream_t s, const MeshDev& m, const double* u, const double* p, const double* ur,
                            const double* pr, const uint8_t* flags, double* parts, double* out);

// ---- point location, point evaluation and tracer particles (points.hip).  The uniform grid of bins over the mesh
// (host: point_locator.build_bins): bin of a point = floor((x - origin) * inv_h) per direction, x fastest; the
// candidates of bin b are bin_cells[bin_ptr[b] .. bin_ptr[b + 1]), ascending cell ids.
struct PointLocatorDev {
  double origin[3] = {0.0, 0.0, 0.0}, inv_h[3] = {0.0, 0.0, 0.0};
  int32_t nbins[3] = {1, 1, 1};
  const int32_t* bin_ptr = nullptr;
  const int32_t* bin_cells = nullptr;
};
// cells[i] = lowest-id candidate cell containing x[i] (all barycentric coordinates >= -1e-12), -1: outside
void launch_locate_points(hipStream_t s, const MeshDev& m, const PointLocatorDev& L, int64_t n, const double* x,
                          int32_t* cells);
// kind 0: velocity f [dim n_p2] -> out [n][dim]; 1: P1 field f [n_p1]; 2: P2 scalar f [n_p2] -> out [n]; NaN where the
// cell is not one of the mesh
void launch_eval_points(hipStream_t s, const MeshDev& m, int kind, const double* f, int64_t n, const double* x,
                        const int32_t* cells, double* out);
// status[i] = cells[i] < 0; counts [2][workgroups of 256 particles]: (left, 0) per workgroup
void launch_tracer_init(hipStream_t s, int64_t n, const int32_t* cells, uint8_t* status, int32_t* counts);
// RK4 over n_sub substeps of dt / n_sub in (1 - theta) ua + theta ub (ub null: frozen ua); counts: (left, bin-search
// fallbacks) per workgroup
void launch_advect_tracers(hipStream_t s, const MeshDev& m, const PointLocatorDev& L, const double* ua,
                           const double* ub, double dt, int n_sub, int64_t n, double* x, int32_t* cells,
                           uint8_t* status, int32_t* counts);

// ---- running flow statistics (statistics.hip).  Accumulators of one field: n_q arrays of `stride` doubles each
// (stride = the node count rounded up to even: every array starts 16-byte aligned), array q at acc + q * stride, in
// the column order of nsfem_stats_profiles -- `dim` variables u with SCALAR = false: m_u[dim], C_uu[dim (dim + 1) / 2];
// SCALAR = true appends m_T, C_TT, C_uT[dim].  The P1 accumulators (m_p, C_pp) are the case dim = 1 without a scalar.
inline int stats_columns(int dim, bool scalar) { return dim + dim * (dim + 1) / 2 + (scalar ? 2 + dim : 0); }
struct StatsUpdate {
  int64_t n2 = 0, n1 = 0;          // P2 / P1 nodes (n1 = 0: no pressure)
  size_t stride2 = 0, stride1 = 0;
  const double* u = nullptr;       // [n2][dim]
  const double* T = nullptr;       // [n2], scalar only
  const double* p = nullptr;       // [n1]
  double* acc2 = nullptr;
  double* acc1 = nullptr;
  double a = 1.0, b = 0.0;         // w / (W + w), w W / (W + w)
  int first = 1;                   // W == 0: the means take the sample's bytes
  int blocks2 = 0;                 // workgroups [0, blocks2) work on the P2 nodes, the rest on the P1 nodes
};
// ONE launch: weighted Welford / Chan update of all accumulators
void launch_stats_update(hipStream_t s, int dim, bool scalar, StatsUpdate a);
// pooled mean and covariance over groups of nodes (CSR), out [n_groups][stats_columns(dim, scalar)]; dim = 1: P1
void launch_stats_profile(hipStream_t s, int dim, bool scalar, const double* acc, size_t stride, double inv_w,
                          int32_t n_groups, const int32_t* group_ptr, const int32_t* nodes, const double* weights,
                          double* out);
// out[node * nc + c] = scale * acc[(col + c) * stride + node]; nc = 0: out[node] = scale * sum of the `dim` arrays
// col_trace[0 .. dim) (turbulent kinetic energy)
void launch_stats_gather(hipStream_t s, int64_t n, const double* acc, size_t stride, int col, int nc, double scale,
                         int dim, const int col_trace[3], double* out);
// ---- gradient-derived fields (derived.hip): the quantities NSFEM_DERIVED_* of include/nsfem.h at the centring
// NSFEM_DERIVED_CELL / VERTEX / NODE.  Components of a quantity (-1: no such quantity):
inline int derived_components(int dim, int quantity) {
  switch (quantity) {
    case NSFEM_DERIVED_VORTICITY: return dim == 2 ? 1 : 3;
    case NSFEM_DERIVED_DIVERGENCE: case NSFEM_DERIVED_SHEAR_RATE: case NSFEM_DERIVED_Q_CRITERION: return 1;
    case NSFEM_DERIVED_VELOCITY_GRADIENT: return dim * dim;
    case NSFEM_DERIVED_PRESSURE_GRADIENT: case NSFEM_DERIVED_SCALAR_GRADIENT: return dim;
    default: return -1;
  }
}
void upload_derived_tables();   // the rules of both dimensions (nsfem_create)
// doubles of work space a call needs: the result in its host layout ([entities][ncomp]) and, for NODE, the ncomp + 1
// node-sorted element planes behind it
int64_t derived_work_doubles(const MeshDev& m, int center, int ncomp);
// ONE element launch (plus ONE gather launch for NODE); returns where the result lies in `work`.  p / T may be null
// when the mask does not ask for their gradients
const double* launch_derived_fields(hipStream_t s, const MeshDev& m, const double* u, const double* p, const double* T,
                                    unsigned mask, int center, int ncomp, double* work);
// ---- energy spectra (spectrum.hip): a nodal field packed onto its lattice, and the binned sums of squares of its
// transformed values.  The axis passes between the two are fd_transform_axes (fastdiag.hip).
constexpr int kSpecChunk = 2048;   // entries of the bin CSR one workgroup reduces; a chunk never straddles a bin
// w[point] = state[node_of_point[point] * ncomp + c]
void launch_spec_pack(hipStream_t s, int64_t n_points, const int32_t* node_of_point, const double* state, int ncomp,
                      int c, double* w);
// parts[k] = sum of w[bin_points[e]]^2 over the entries chunk_ptr[k] .. chunk_ptr[k + 1] (fixed tree), then
// out[b * ncomp + c] = parts[bin_chunk_ptr[b]] + ... in ascending order (+0.0 for a bin without entries)
void launch_spec_bin(hipStream_t s, const double* w, int32_t n_chunks, const int32_t* chunk_ptr,
                     const int32_t* bin_points, double* parts, int32_t n_bins, const int32_t* bin_chunk_ptr, int ncomp,
                     int c, double* out);
// ---- wall quantities (wall.hip): NW = wall_components(dim) integrals per facet of a resident, group-sorted facet set
// (k_wall_facets<DIM, LAW>) and their sums per group in a fixed order (k_wall_reduce<NW>); the row layout is in
// include/nsfem.h (nsfem_wall_compute)
inline int wall_components(int dim) { return dim == 2 ? 9 : 13; }
struct WallParams {
  double nu = 0.0, sym = 0.0, kappa = 0.0, origin[3] = {0.0, 0.0, 0.0};
  int law = 0;                               // 0: constant viscosity; 1, 2, 4, 5, 8: + nu_x of visc_law_at<law>
  double law_p[3] = {0.0, 0.0, 0.0};
  const double* cs2v = nullptr;              // law 8: the vertex field C_s^2 (launch_dynamic_constant), else null
  const double* cthv = nullptr;              // law 8 and != null: the heat row uses kappa + c_K Delta_K^2 gamma, c_K from
                                             // this vertex field C_theta (launch_dynamic_constant on (u, T))
  double inv_prt = 0.0;                      // law 1, 4, 5 and != 0: the heat row uses kappa + nu_x inv_prt (subgrid heat flux)
};
// ONE launch: rows[f][NW] of the nf facets (fcell, flocal: device lists); T may be null (no scalar: +0.0 entries)
void launch_wall_facets(hipStream_t s, const MeshDev& m, int nf, const int32_t* fcell, const int32_t* flocal,
                        const double* u, const double* p, const double* T, const WallParams& w, double* rows);
// ONE launch: out[g][NW] = sum of the rows goff[g] <= f < goff[g + 1], one workgroup per group
void launch_wall_reduce(hipStream_t s, int dim, int n_groups, const int32_t* goff, const double* rows, double* out);
// ---- wall-stress models (wallmodel.hip, nsfem_set_wall_model): the resident facet set of the explicit term W(u), its
// samples, the node CSR of the gather and the two buffers the launches write.  NQ = 3 / 6 points per facet, NF2 = 3 / 6
// P2 nodes per facet.  law 0: the term is off (the buffers stay for the next call that needs them)
inline int wall_model_points(int dim) { return dim == 2 ? 3 : 6; }
inline int wall_model_facet_nodes(int dim) { return dim == 2 ? 3 : 6; }
inline int wall_model_row(int dim) { return dim + 4; }
struct WallModelDev {
  int law = 0;                                // 1 Werner-Wengle (p = A, B), 2 Reichardt (p = kappa, C)
  double p[4] = {0.0, 0.0, 0.0, 0.0};
  double start[3] = {0.0, 0.0, 0.0};          // the Werner-Wengle triple A, 1 / (1 + B), A^(2 / (1 - B)) the kernel takes
  int32_t n_facets = 0, n_nodes = 0;
  bool have_uw = false;
  DevBuf<int32_t> fcell, flocal, scell;       // [nf], [nf], [nf][NQ]
  DevBuf<double> slam, sy, uw;                // [nf][NQ][dim + 1], [nf][NQ], [nf][dim]
  DevBuf<int32_t> nodes, nptr, entry;         // the nodes on modelled facets, their runs, rows of fvec (facet NF2 + local)
  DevBuf<double> fvec, rows;                  // [nf][NF2][dim], [nf][dim + 4]
};
// ONE launch: w.fvec = weight times the facet vectors of W(u), w.rows = the diagnostics rows
void launch_wall_model_facets(hipStream_t s, const MeshDev& m, const WallModelDev& w, const double* u, double nu,
                              double weight);
// ONE launch: v = the node sums of w.fvec in ascending facet order;  n1 += v,  rhs -= b0 v  (rhs null: the plain sum)
void launch_wall_model_gather(hipStream_t s, const MeshDev& m, const WallModelDev& w, double b0, double* n1,
                              double* rhs);
// diag extraction: d[(i,a)] = 1 / A_ii[a][a]  (mask rows -> 1)
void launch_inv_diag(hipStream_t s, const BlockMat& A, int nv, const uint8_t* rowmask,
                     double* dinv);

// vector kernels (n = number of doubles)
void launch_rot90(hipStream_t s, int64_t n_nodes, double g, const double* u, double* out);
void launch_jac_add_skew(hipStream_t s, int64_t nnz, double g, const double* M, double* J);
void launch_rot_field(hipStream_t s, const MeshDev& m, double* out);
void launch_coord_field_3d(hipStream_t s, const MeshDev& m, double* out);
void launch_cross3(hipStream_t s, int64_t n_nodes, const double g[3], const double* u, double* out);
void launch_jac_add_skew3(hipStream_t s, int64_t nnz, const double g[3], const double* M, double* J);
void launch_axpby(hipStream_t s, int64_t n, double a, const double* x, double b, const double* y,
                  double* z);                                     // z = a x + b y
void launch_lincomb3(hipStream_t s, int64_t n, double a, const double* x, double b,
                     const double* y, double c, const double* z, double* out);
void launch_scale_combine(hipStream_t s, int nnz, double a, const double* A, double b,
                          const double* B, double* C);            // C = a A + b B (values)
void launch_dot(hipStream_t s, int64_t n, const double* x, const double* y, double* parts);
void launch_sum_sub_mean(hipStream_t s, int64_t n, double* x, double* parts);
void launch_correction_setup(hipStream_t s, int64_t n, double a, double* rhs, const double* t, const uint8_t* mask,
                             double* r0, double* parts_r, double* parts_b);
// x -= mean(x), then x . x of the shifted vector into `parts_dot`, the subtraction and the dot in one launch
void launch_sum_sub_mean_dot(hipStream_t s, int64_t n, double* x, double* parts, double* parts_dot);
// u0 = ustar + e ; partial sums of rn . rn, r0 . r0, rhs . rhs (the partitions of k_dot / k_correction_setup)
void launch_correction_finish(hipStream_t s, int64_t n, const double* ustar, const double* e, double* u0,
                              const double* rn, const double* r0, const double* rhs, double* parts_n, double* parts_r,
                              double* parts_b);
// the same together with |b|^2 (512 partial sums) in one launch; rows with mask != 0 must be exactly the nbc dofs
void launch_bc_residual_norm(hipStream_t s, int64_t n, double* b, const uint8_t* mask, int nbc, const int32_t* dofs,
                             const double* g, const double* x, double* parts);
void launch_set_bc_residual(hipStream_t s, int nbc, const int32_t* dofs, const double* g,
                            const double* x, double* b);          // b[d] = x[d] - g[d]
void launch_set_values(hipStream_t s, int nbc, const int32_t* dofs, const double* g, double* x);
void launch_fill_mask(hipStream_t s, int nbc, const int32_t* dofs, uint8_t* mask);
void launch_mask_zero(hipStream_t s, int64_t n, const uint8_t* mask, double* x);
void launch_add_scalar(hipStream_t s, int64_t n, double a, double* x);

// Krylov scratch + drivers
struct LinOp;
// identity of one captured Krylov iteration body (all baked kernel arguments)
struct GraphKey {
  const void *op, *prec, *x, *dinv;
  int64_t n;
  int parity;
  uint64_t epoch;
  const void* b = nullptr;          // right-hand side, where the body reads or writes it (BiCGStab: zero-start bodies)
  bool operator==(const GraphKey& o) const {
    return op == o.op && prec == o.prec && x == o.x && dinv == o.dinv && n == o.n &&
           parity == o.parity && epoch == o.epoch && b == o.b;
  }
};
struct KrylovWork {
  int64_t n = 0;
  DevBuf<double> r, rhat, p, v, s, t, phat, shat, z, q;
  DevBuf<double> parts;     // [kPartSlots][kParts]
  DevBuf<double> scal;      // device scalars
  double* h_parts = nullptr;   // pinned host [kPartSlots][kParts]
  // reduced sums for the host (convergence checks): a one-workgroup kernel re-reduces the partial sums of up to four
  // slots in the order the device kernels use (sum_parts) and stores them, then a sequence number, into coherent
  // pinned host memory; the host spins on the number.  Replaces hipMemcpyAsync + hipStreamSynchronize: on the
  // MI355X the copy path leaves the GPU idle ~20 us before and ~25 us after the copy (rocprofv3 trace, round 4)
  struct HostResult { double v[4]; uint64_t seq; };
  HostResult* h_res = nullptr;
  uint64_t seq_no = 0;
  // captured HIP graphs of the iteration bodies
  std::vector<std::pair<GraphKey, hipGraphExec_t>> graphs;
  std::vector<GraphKey> seen;   // bodies that ran eagerly once (lazy table builds synchronise): captured at their second run
  uint64_t epoch = 0;
  // replay is worth its capture only while the baked arguments stay put: contexts whose operators change every few
  // iterations (variable time steps) fall back to eager launches (graphs_off); profiling windows that record HIP
  // events inside the bodies suspend it
  uint64_t touch = 0;           // bumped by every solver that uses the work vectors (who may rely on what another left in them)
  double last_target = 0.0;     // absolute residual target of the last solve (max(atol, rtol |b|)): the drivers' iteration predictor
  bool graphs_off = false, graphs_suspended = false;
  int64_t replays_in_epoch = 0;
  int short_epochs = 0;
  bool graphs_enabled(const LinOp& op) const;
  void replay(hipStream_t s, const GraphKey& key, const std::function<void()>& body);
  void clear_graphs();
  void ensure(int64_t n_);
  ~KrylovWork();
};

// general preconditioner z = M^{-1} r (multigrid); nullptr in LinOp => Jacobi (dinv)
struct Precond {
  virtual ~Precond() {}
  virtual void apply(hipStream_t s, const double* r, double* z) = 0;
};

// ---- partitioned meshes: halo ranges (node units) and the communicator interface ---------
// general halo of an unstructured partition: per neighbouring rank the nodes this rank sends
// (owned here, ghost there) and receives (ghost here), both in the order of the global node ids
struct HaloLists {
  std::vector<int32_t> nbr;
  std::vector<int64_t> send_ptr, recv_ptr;       // [nbr.size() + 1]
  DevBuf<int32_t> send_idx, recv_idx;
  int64_t n_send() const { return send_ptr.empty() ? 0 : send_ptr.back(); }
  int64_t n_recv() const { return recv_ptr.empty() ? 0 : recv_ptr.back(); }
  int find(int rank) const {
    for (size_t k = 0; k < nbr.size(); ++k)
      if (nbr[k] == rank) return (int)k;
    return -1;
  }
};
// strips / slabs: two neighbours, contiguous ranges (no packing); `lists` set: index lists instead
struct HaloRange {
  int64_t send_up_off = 0, send_up_cnt = 0, recv_above_off = 0, recv_above_cnt = 0;
  int64_t send_down_off = 0, send_down_cnt = 0, recv_below_off = 0, recv_below_cnt = 0;
  const HaloLists* lists = nullptr;
};
struct Comm {
  int rank = 0, size = 1;
  bool periodic = false;     // the partition closes periodically: neighbours wrap around
  int up() const { return rank + 1 < size ? rank + 1 : (periodic ? 0 : -1); }
  int down() const { return rank > 0 ? rank - 1 : (periodic ? size - 1 : -1); }
  virtual ~Comm() {}
  // in-place sum over the ranks of `count` doubles in device memory, ordered on stream s
  virtual void allreduce_sum(hipStream_t s, double* dev, int64_t count) = 0;
  virtual void allreduce_max(hipStream_t s, double* dev, int64_t count) = 0;
  // fill the ghost ranges of `vec` (width entries per node) from the neighbouring ranks
  virtual void exchange(hipStream_t s, const HaloRange& h, double* vec, int width) = 0;
  // the reverse of `exchange`: the values this rank holds in its ghost ranges are ADDED to the
  // owners' entries (their send ranges) -- products with operators that are stored as rank-local
  // additive parts (A = sum_r A_r), where every rank computes partial sums for its ghost rows
  virtual void exchange_add(hipStream_t s, const HaloRange& h, double* vec, int width) = 0;
  // ---- overlap of the exchange with the interior rows of the product that consumes `vec`:
  // exchange_begin orders the exchange after everything queued on `s` so far and runs it on the
  // communicator's own stream; exchange_end makes `s` wait for its completion.  Between the two
  // calls the caller launches (on `s`) only work that neither reads the ghost ranges nor writes
  // the send ranges of `vec`.
  bool overlap = false;
  hipStream_t cs = nullptr;
  hipEvent_t ev_in = nullptr, ev_done = nullptr;
  int64_t n_overlapped = 0;
  void exchange_begin(hipStream_t s, const HaloRange& h, double* vec, int width) {
    if (!cs) {
      NSFEM_HIP(hipStreamCreateWithFlags(&cs, hipStreamNonBlocking));
      NSFEM_HIP(hipEventCreateWithFlags(&ev_in, hipEventDisableTiming));
      NSFEM_HIP(hipEventCreateWithFlags(&ev_done, hipEventDisableTiming));
    }
    NSFEM_HIP(hipEventRecord(ev_in, s));
    NSFEM_HIP(hipStreamWaitEvent(cs, ev_in, 0));
    exchange(cs, h, vec, width);
    NSFEM_HIP(hipEventRecord(ev_done, cs));
    ++n_overlapped;
  }
  void exchange_end(hipStream_t s) { NSFEM_HIP(hipStreamWaitEvent(s, ev_done, 0)); }
  void release_streams() {
    if (cs) { (void)hipStreamSynchronize(cs); (void)hipStreamDestroy(cs); cs = nullptr; }
    if (ev_in) { (void)hipEventDestroy(ev_in); ev_in = nullptr; }
    if (ev_done) { (void)hipEventDestroy(ev_done); ev_done = nullptr; }
  }
  // traffic counters (calls / payload bytes this rank sends), read through nsfem_comm_stats
  int64_t n_allreduce = 0, n_exchange = 0, bytes_allreduce = 0, bytes_exchange = 0;
  // NSFEM_COMM_HIST=1: calls by (kind, payload bytes) since the last reset, printed by nsfem_comm_stats --
  // the payload size identifies the level / vector a message belongs to
  std::map<std::pair<int, int64_t>, int64_t> hist;
  void tally(int kind, int64_t bytes) {
    static const bool on = std::getenv("NSFEM_COMM_HIST") != nullptr;
    if (on) ++hist[{kind, bytes}];
  }
  void count_allreduce(int64_t count) { ++n_allreduce; bytes_allreduce += 8 * count; tally(0, 8 * count); }
  void count_exchange_add(const HaloRange& h, int width) {
    ++n_exchange;
    const int64_t before = bytes_exchange;
    if (h.lists) bytes_exchange += 8 * (int64_t)width * h.lists->n_recv();
    else bytes_exchange += 8 * (int64_t)width * ((up() >= 0 ? h.recv_above_cnt : 0) + (down() >= 0 ? h.recv_below_cnt : 0));
    tally(2, bytes_exchange - before);
  }
  void count_exchange(const HaloRange& h, int width) {
    ++n_exchange;
    const int64_t before = bytes_exchange;
    if (h.lists) bytes_exchange += 8 * (int64_t)width * h.lists->n_send();
    else bytes_exchange += 8 * (int64_t)width * ((up() >= 0 ? h.send_up_cnt : 0) + (down() >= 0 ? h.send_down_cnt : 0));
    tally(1, bytes_exchange - before);
  }
};
void launch_zero_ghost(hipStream_t s, int64_t n, const uint8_t* mask, double* x);  // x[mask==2]=0
// packed halo exchange of two vectors (width entries per node each): a, b -> buf[node][2 width] on the nodes this rank
// sends, and buf -> a, b on its ghost nodes.  One message of width 2 * width instead of two
void launch_halo_pack2(hipStream_t s, int64_t n_nodes, const HaloRange& h, int width, const double* a, const double* b,
                       double* buf);
void launch_halo_unpack2(hipStream_t s, int64_t n_nodes, const HaloRange& h, int width, const double* buf, double* a,
                         double* b);

// product with a halo-dependent input: exchange, then launch(0) -- or, when the communicator
// overlaps and the pattern has interior row blocks, exchange on the communicator's stream under
// launch(1) (interior blocks), then launch(2) (halo-adjacent blocks) after the event wait
template <class F>
inline void product_with_halo(Comm* comm, const HaloRange* halo, int width, hipStream_t s,
                              const double* v, const Pattern* pat, F&& launch) {
  if (!comm || !halo) { launch(0); return; }
  double* vec = const_cast<double*>(v);
  if (!comm->overlap || !pat || pat->n_rblk == 0 || pat->int_b1 <= pat->int_b0) {
    comm->exchange(s, *halo, vec, width);
    launch(0);
    return;
  }
  comm->exchange_begin(s, *halo, vec, width);
  launch(1);
  comm->exchange_end(s);
  launch(2);
}

// abstract operator (block systems): y = A x on vectors of length n
struct Operator {
  int64_t n = 0;
  virtual ~Operator() {}
  virtual void apply(hipStream_t s, const double* x, double* y) = 0;
};

struct LinOp {
  Operator* custom = nullptr;       // overrides A / nv / rowmask when set (BiCGStab only)
  const BlockMat* A = nullptr;
  int nv = 1;
  const uint8_t* rowmask = nullptr;
  int maskmode = MASK_NONE;
  const double* dinv = nullptr;     // Jacobi
  Precond* prec = nullptr;          // overrides dinv when set
  // partitioned meshes (all null / 0 in serial runs)
  Comm* comm = nullptr;
  const HaloRange* halo = nullptr;
  int halo_width = 1;               // vector entries per node
  const uint8_t* ghostmask = nullptr;
  int64_t n_global = 0;             // global length (mean projection)
  uint64_t graph_epoch = 0;         // bumped whenever baked kernel arguments may have changed
  bool x_zero = false;              // the caller's start vector is all zeros: the start residual is b itself
                                    // (BiCGStab skips the operator application that would compute b - A 0)
  double known_bnorm = -1.0;        // >= 0: |b|_2 (all ranks), already on the host -- with x_zero it is the start
                                    // residual too and the solve begins without a device -> host round trip
  bool b_scratch = false;           // the solver may overwrite b (the caller recomputes it before reading it again):
                                    // a zero-start BiCGStab solve then keeps its shadow residual IN b, without a copy
};

// ---- multigrid ------------------------------------------------------------------
// P (rows = finer level, cols = coarser level) and R = P^T as scalar CSR operators
struct Transfer {
  Pattern patP, patR;
  BlockMat P, R;
  std::vector<int32_t> h_inj;   // coarse node -> coinciding finer-level node
  std::vector<double> h_val;    // host copy of P's values (lattice check)
  int lattice = -1;             // P is the lattice interpolation of a (2 Wc - 1)-wide fine lattice: -1 unknown, 0 no, 1 yes
  bool is_lattice(int wf, int hf);
  // kind: 1 nested, 2 non-nested interpolation, 0 decide from the values (nsfem_mg_level_desc::transfer_kind)
  void build(hipStream_t s, int n_fine, int n_coarse, const int32_t* rowptr, const int32_t* col,
             const double* val, int kind = 0);
};

struct MGLevel {
  const BlockMat* A = nullptr;   // scalar operator of this level
  int n = 0;                     // scalar unknowns
  const uint8_t* mask = nullptr; // [n * nv]; level 0 uses the context's mask
  DevBuf<uint8_t> own_mask;
  DevBuf<double> dinv, xa, xb, x, b, r, d;
  DevBuf<double> xc, d2;         // lattice smoother: out-of-place iterate of a cycle leg, second direction buffer
  DevBuf<uint8_t> sidm;          // lattice smoother: dictionary entry | mask bits, one byte per row
  const void* sidm_for = nullptr; // (dictionary, mask) pair the byte array was built for
  const void* sidm_mask = nullptr;
  double lmax = 2.0;
  double ratio = 0.0;            // > 0: Chebyshev interval [lmax / ratio, lmax] of THIS level (truncated solve)
  const BlockMat* P = nullptr;   // transfer to / from the next coarser level
  const BlockMat* R = nullptr;
  Transfer* transfer = nullptr;  // the object P and R belong to (lattice check), when known
  const std::vector<int32_t>* h_inj = nullptr;
  // partitioned meshes
  const std::vector<uint8_t>* h_ghost = nullptr;   // per node: nonzero = ghost
  int ghost_lo = -2, ghost_hi = -2;                // ghost lattice lines at the bottom / top of a strip (-2: not looked
                                                   // at yet, -1: the ghost nodes are not whole lines)
  HaloRange halo;
  bool has_halo = false;
  // partitioned meshes, operators without an element-local form (the algebraic Schur Laplacian
  // D diag(M)^-1 D^T): A holds this rank's ADDITIVE part -- the sum over the ranks of the parts,
  // ghost rows included, is the operator.  Products: fill the ghosts of x, multiply every local
  // row, add the ghost rows at their owners (Comm::exchange_add).
  bool additive = false;
  DevBuf<double> t;              // additive levels: the product before the smoother update
};


struct Multigrid : Precond {
  int nv = 1;
  std::vector<MGLevel> lv;
  int degree = 2;                // Chebyshev steps per pre/post smoothing
  int pre_degree = -1;           // >= 0: pre-smoothing steps differ from `degree` (non-symmetric cycle)
  double eig_ratio = 4.0;        // smoothing interval [lmax / ratio, lmax]
  int coarse_dense_max = 1200;
  int coarse_steps = 30;
  bool dense_coarse = true, ready = false;
  DevBuf<double> coarse_inv, parts;
  // partitioned meshes: communicator + replicated global coarsest problem
  Comm* comm = nullptr;          // set only when the context is partitioned (or forced)
  bool comm_active() const { return comm != nullptr; }
  const BlockMat* globA = nullptr;
  int n_glob = 0;
  int64_t glob_off = 0;
  // unstructured partitions: global id of every local coarsest node instead of offset + i
  const int32_t* glob_idx = nullptr;
  const std::vector<int32_t>* h_glob_idx = nullptr;
  size_t glob_of(size_t i) const {
    return h_glob_idx ? (size_t)(*h_glob_idx)[i] : ((size_t)glob_off + i) % (size_t)n_glob;
  }
  bool glob_wrap = false;        // periodic partitions: the local coarsest level wraps around the global numbering
  DevBuf<double> gb, gx;
  // when the global coarsest mesh is too large for a dense solve it carries its own REPLICATED
  // hierarchy: a serial multigrid (no communicator) every rank runs redundantly on the
  // all-reduced right-hand side -- the small levels cost no halo exchanges at all
  Multigrid* tail = nullptr;     // not owned
  // in-situ timing of the finest-level smoothing launches (bench.py's roofline figure): one
  // HIP-event pair per launch while enabled
  bool prof = false;
  std::vector<hipEvent_t> prof_ev;
  size_t prof_n = 0;
  bool prof_open = false;        // an event pair is open inside the current smooth() call
  int64_t prof_launches = 0;     // launches covered by the recorded pairs
  int64_t lattice_launches = 0;  // launches of the multi-step lattice kernel by this hierarchy (nsfem_mg_info)
  int64_t prof_steps = 0;        // smoothing steps covered (the lattice kernel runs several per launch)
  int64_t prof_bytes = 0;        // algorithmic bytes of the covered launches (lattice kernel: per launch shape)
  bool own_mask0 = false;        // level 0 keeps its own mask buffer (tails)
  bool smoother_only = false;    // the last level is smoothed (coarse_steps), never solved globally
  // preconditioner of a Newton matrix with dolfin-style Dirichlet rows: the result carries z = r on
  // the rows flagged 1 of level 0 -- written by the epilogue of the last finest-level smoothing step
  // instead of a separate copy kernel
  bool identity_rows = false;
  // partitioned meshes, relaxed mode: a smoothing sequence exchanges the ghost values ONCE (at
  // its first step that reads them) and keeps them frozen afterwards -- Chebyshev iteration on
  // the rank-local operator (block-Jacobi across ranks) around the true residual, still a
  // symmetric preconditioner; prolongations compute the ghost rows themselves.  Default (false):
  // one exchange per SpMV, the partitioned cycle IS the serial one.
  bool relaxed_halo = false;
  // truncated cycle (mass-dominated operators): only the first `active` levels are used and the
  // last of them is SOLVED by `trunc_steps` Chebyshev steps over its whole spectrum
  // [trunc_lmin, lmax] -- no coarser level, no dense / global coarse solve, no all-reduce
  size_t active = 0;             // 0: all levels
  double trunc_lmin = 0.0, trunc_tol = 0.1;
  int trunc_steps = 0;
  bool truncated() const { return active > 0 && active < lv.size(); }
  void refresh_global_coarse(hipStream_t s, const std::vector<uint8_t>& cur, bool singular);
  void halo_fill(hipStream_t s, const MGLevel& L, const double* v);
  void apply_additive(hipStream_t s, MGLevel& L, const double* x, double* t);
  void smooth_additive(hipStream_t s, MGLevel& L, const double* b, const double* x_in, double* x_out,
                       int steps, bool first_done);
  void setup_work(hipStream_t s);
  void refresh(hipStream_t s, const std::vector<uint8_t>& mask0, bool singular);
  void apply(hipStream_t s, const double* r, double* z) override;
  // result in x (level 0: always) or in a buffer of the level: the returned pointer says where
  const double* vcycle(hipStream_t s, size_t l, const double* b, double* x, bool first_done = false);
  // multi-step lattice kernel (2D lexicographic lattices, serial levels): `steps` Chebyshev steps out of
  // place, optionally the residual of the result as well
  bool lattice_ok(const MGLevel& L) const;
  // partitioned level in relaxed halo mode whose ghost nodes are whole lattice lines: smoothing sequences run in
  // the multi-step lattice kernel with the ghost lines frozen (transfers stay explicit products)
  bool lattice_ok_relaxed(MGLevel& L);
  bool chain_child_forms_b(size_t l);
  size_t restricted_to = 0;      // level whose b the two-level restriction kernel has already formed in this leg
  // xc: the start vector is [x_in +] P xc (prolongation fused into the staging); rf: b = R rf is computed by the
  // first launch and stored to `b` (restriction fused)
  void smooth_lattice(hipStream_t s, MGLevel& L, const double* b, const double* x_in, double* x_out,
                      int steps, bool ident_last, double* r_out, const double* xc = nullptr,
                      const double* rf = nullptr);
  bool transfer_lattice(size_t l);      // levels l, l + 1: lattice operators and a lattice interpolation between them
  const double* vcycle_lattice(hipStream_t s, size_t l, const double* b, double* x, const double* rf);
  void smooth(hipStream_t s, MGLevel& L, const double* b, const double* x_in, double* x_out,
              int steps, bool ghosts_valid = false, bool ident_last = false, bool first_done = false);
  // restriction to level l + 1 fused with the first smoothing step there (when that level starts
  // from zero): returns true when L[l+1].xa / .d already hold step 0
  bool restrict_to(hipStream_t s, size_t l, const double* src);
  bool starts_from_zero(size_t l) const;
  void cheb_coeffs(const MGLevel& L, int k, double rho_prev, double& c1, double& c2,
                   double& rho) const;
};

// Fast diagonalisation of the pressure Poisson operator on tensor-product lattices (fastdiag.hip, poisson_fd.py): what
// the callers need of either solver object.  apply(s, r, z) is z = A^+ r on one rank and a COLLECTIVE (one all-reduce
// of the transformed global lattice array between the forward and the backward products) when the factors are
// partitioned.  Contracts of the partitioned forms: strips sum over every local row, so r must carry ZERO ghost rows
// (reads_ghosts()); slabs contract the owned planes only and never read the ghost planes of r; both return z on EVERY
// local row / plane, ghosts included (no halo exchange afterwards).
struct FastDiagBase : Precond {
  Comm* const* comm;             // the owner's communicator slot, read at every partitioned apply (no copy to patch)
  bool exact = true;             // the tensor sum is the stiffness matrix itself (2D: always); else it preconditions CG
  int64_t applications = 0;      // apply() calls issued by the host (a CG iteration replayed from a graph: not counted)
  int64_t solves = 0;            // projection solves that ran with these factors
  explicit FastDiagBase(Comm* const* comm_) : comm(comm_) {}
  virtual bool ready() const = 0;
  virtual bool partitioned() const = 0;            // strip or slab factors
  virtual bool reads_ghosts() const { return false; }
  // the factors fit a pressure space of n_local dofs on this rank, n_global in all: partitioned exactly when the
  // context is, this rank's lines / planes n_local nodes, and then the GLOBAL lattice n_global nodes
  virtual bool fits(int64_t n_local, int64_t n_global, bool distributed) const = 0;
  virtual void release() = 0;    // frees the factors and work buffers (ready() false); the counters stay
};

// 2D: z = A^+ r by four dense products on the matrix cores
struct FastDiag : FastDiagBase {
  using FastDiagBase::FastDiagBase;
  int W = 0, H = 0;
  // partitioned strips: this rank holds the lattice lines j0 ... j0 + h_loc - 1 (ghost lines included) of the GLOBAL
  // W x H lattice; Vy then keeps those rows of V_y only.  h_loc == 0: the whole lattice (one rank)
  int j0 = 0, h_loc = 0;
  DevBuf<double> Vx, Vy, inv, t1, t2;
  bool ready() const override { return W > 0 && Vx.p && Vy.p && inv.p; }
  bool partitioned() const override { return h_loc > 0; }
  bool reads_ghosts() const override { return partitioned(); }
  bool fits(int64_t n_local, int64_t n_global, bool distributed) const override {
    return ready() && distributed == partitioned() && (int64_t)W * (partitioned() ? h_loc : H) == n_local &&
           (!distributed || (int64_t)W * H == n_global);
  }
  void set(hipStream_t s, int W_, int H_, const double* vx, const double* vy, const double* inv_);
  void set_rows(hipStream_t s, int W_, int H_, int j0_, int h_loc_, const double* vx, const double* vy,
                const double* inv_);
  void release() override;
  void apply(hipStream_t s, const double* r, double* z) override;      // strip factors: apply_strip

 private:
  void apply_strip(hipStream_t s, const double* r, double* z);
};

// 3D box lattices (poisson_fd.factors_3d): z = T^+ r, T the tensor sum of the 1D stiffness / lumped mass matrices, by
// six mode products of the N_z x N_y x N_x array on the matrix cores.  exact: T is the P1 stiffness matrix itself (the
// projection step is one pass plus the residual check); otherwise T^+ preconditions CG.
struct FastDiag3 : FastDiagBase {
  using FastDiagBase::FastDiagBase;
  int Nx = 0, Ny = 0, Nz = 0;    // the GLOBAL lattice
  // partitioned slabs: this rank holds the n_loc lattice planes (first + i) mod Nz (ghost planes included) and owns
  // the run own0 ... own0 + n_own - 1 of them; Vz then keeps the rows of V_z of its local planes.  n_loc == 0: the
  // whole lattice (one rank)
  int first = 0, n_loc = 0, own0 = 0, n_own = 0;
  DevBuf<double> Vx, Vy, Vz, inv, t1, t2, tz;
  bool ready() const override { return Nx > 0 && Vx.p && Vy.p && Vz.p && inv.p; }
  bool partitioned() const override { return n_loc > 0; }
  bool fits(int64_t n_local, int64_t n_global, bool distributed) const override {
    return ready() && distributed == partitioned() && (int64_t)Nx * Ny * (partitioned() ? n_loc : Nz) == n_local &&
           (!distributed || (int64_t)Nx * Ny * Nz == n_global);
  }
  void set(hipStream_t s, int Nx_, int Ny_, int Nz_, const double* vx, const double* vy, const double* vz,
           const double* inv_, bool exact_);
  // vz: the GLOBAL Nz x Nz matrix (its rows of the local planes are gathered here)
  void set_planes(hipStream_t s, int Nx_, int Ny_, int Nz_, int first_, int n_loc_, int own0_, int n_own_,
                  const double* vx, const double* vy, const double* vz, const double* inv_, bool exact_);
  void release() override;
  void apply(hipStream_t s, const double* r, double* z) override;      // slab factors: apply_slab

 private:
  void apply_slab(hipStream_t s, const double* r, double* z);
};
// Separable transform of an [n2][n1][n0] array (x fastest) through the tile body of the solvers above: along every
// axis a with a matrix, out[.., k, ..] = sum_i F_a[k][i] in[.., i, ..] (row-major [n_a][n_a], row = basis function); a
// null matrix skips its pass.  x is one plain GEMM over [n2 n1] x n0, y the batched plane product, z one plain GEMM over
// n2 x [n1 n0]; the passes alternate between a (the input) and b.  Returns the array that holds the result (a when
// nothing was transformed) and adds the launches it made to *launches.
double* fd_transform_axes(hipStream_t s, int n0, int n1, int n2, const double* Fx, const double* Fy, const double* Fz,
                          double* a, double* b, int64_t* launches);
// x -= sum(parts) / count on n entries (k_sum fills the slot: launch_sum)
void launch_sum(hipStream_t s, int64_t n, const double* x, double* parts);
void launch_gather_diag(hipStream_t s, int n, const int32_t* diag, const double* vals, double* out);   // out[i] = vals[diag[i]]
void launch_sub_mean(hipStream_t s, int64_t n, int64_t count, const double* parts, double* x);

// z[dofs] = r[dofs]
void launch_copy_at(hipStream_t s, int n, const int32_t* dofs, const double* r, double* z);
// mask[i] = 2 where ghost[i] != 0
void launch_overlay_ghost(hipStream_t s, int64_t n, const uint8_t* ghost, uint8_t* mask);
// communicators (comm.hip)
Comm* make_local_comm(void* group, int rank);
Comm* make_rccl_comm(const char* id128, int rank, int size);
Comm* make_shm_comm(const char* name, int rank, int size, int64_t slot_bytes);

// Jacobi-preconditioned BiCGStab; x holds the initial guess on entry
int bicgstab(hipStream_t s, KrylovWork& w, const LinOp& op, const double* b, double* x,
             const nsfem_krylov_opts& o, nsfem_solve_info& info);
// Jacobi-preconditioned CG (rowmask in MASK_ZERO mode => symmetric elimination);
// project_mean: remove the mean of residuals (singular Neumann problem)
int pcg(hipStream_t s, KrylovWork& w, const LinOp& op, const double* b, double* x,
        const nsfem_krylov_opts& o, nsfem_solve_info& info, bool project_mean);

double host_sum_parts(hipStream_t s, KrylovWork& w, int which);   // sync + sum
double host_sum_run(hipStream_t s, KrylovWork& w, const double* run, int n);   // sum of n device entries, fixed order
void host_sum_parts2(hipStream_t s, KrylovWork& w, int a, int b, double& ra, double& rb);   // two slots, one round trip
void host_sum_parts3(hipStream_t s, KrylovWork& w, int a, int b, int c, double& ra, double& rb, double& rc);

}  // namespace nsfem

// the context
struct nsfem_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  std::string err;
  nsfem::MeshDev mesh;
  nsfem::Pattern p22, p11, p12, p21;
  nsfem::BlockMat M2, K2, Ap, Mp, Dv, Gr, DT, L, J, E;   // constant + per-step operators
  bool have_E = false;
  int traction_form = 0;
  double coef[6] = {1.0, 1.0, 1.0, NAN, NAN, NAN};
  double alpha[3] = {1.0, -1.0, 0.0};
  // rotating frame: angular velocity and its time derivative (2D: scalars about e_z, rot_field =
  // nodal (-y, x); 3D: vectors, rot_field = nodal coordinates x)
  double omega = 0.0, omega_dot = 0.0;
  double omega3[3] = {0.0, 0.0, 0.0}, omega_dot3[3] = {0.0, 0.0, 0.0};
  nsfem::DevBuf<double> rot_field, rot_tmp;
  double k = 1.0;
  bool L_dirty = true;
  // IMEX pressure correction (nsfem_set_imex / nsfem_step_imex): gamma0 scales the stiffness part of L; L1, L2 are
  // the operators of the old levels in the right-hand side, (alpha_i/k) M + gamma_i c_v K
  bool imex_active = false;
  double imex_beta[2] = {1.0, 0.0}, imex_gamma[3] = {1.0, 0.0, 0.0};
  nsfem::BlockMat L1, L2;
  bool imex_ops_dirty = true;
  bool conv_n2_valid = false, conv_n1_fresh = false;   // N2 holds c_c N(u2) / N1 was written since the last advance
  // Key of the stored explicit vectors N1, N2 (the vector itself: imex_explicit_add, api.hip): everything but the level
  // that they were formed with -- convective form, c_c, visc.epoch, bodies.epoch and the 2 c_cor Omega of their level
  // (compared bit for bit), and wm.epoch.  A step forms N(u2) again iff the key of its N2 is not the key the settings give now.
  // vouched: the caller wrote the slot (nsfem_set_state).  The two sides differ here, on purpose: a
  // vouched NSFEM_CONV_N2 is used whatever the other components say; a vouched NSFEM_TCONV_2 (Scalar::Key below)
  // stands for every FORM only -- its epochs are those of the vouching call and are honoured afterwards
  struct ImexKey {
    int form = -1;
    double cc = 0.0;
    int64_t visc = 0, body = 0, wall = 0;
    double gam[3] = {0.0, 0.0, 0.0};
    bool vouched = false;
    static ImexKey of(const nsfem_ctx& c, const double gam[3]);       // (api.hip: what the settings give now)
    bool serves(const ImexKey& now) const {
      return vouched || (form == now.form && cc == now.cc && visc == now.visc && body == now.body &&
                         wall == now.wall && std::memcmp(gam, now.gam, sizeof(gam)) == 0);
    }
  } conv_key;
  // partitioned meshes: the ghost entries of the slot are bit copies of the owners' values (exchanged by an IMEX
  // right-hand side and not written since) -- kept next to the flags above, nsfem_advance rotates them with the slots
  bool u1_ghost_fresh = false, u2_ghost_fresh = false;
  nsfem::DevBuf<double> imex_pack;                     // [n_p2][2 dim]: u1 and u2 in one halo message
  int imex_lattice_agreed = -1;                        // the ranks' common answer to "one-launch right-hand side?" (-1: not asked)
  // rotating frame in the IMEX calls (nsfem_set_imex_rotation): treatment 0 refuse, 1 Coriolis term extrapolated with
  // the convective term.  w[0], w[1]: the angular velocity at t^n, t^(n-1) where `given` (else the value of
  // nsfem_set_angular_velocity)
  struct ImexRotation {
    int treatment = 0;
    bool given[2] = {false, false};
    double w[2][3] = {{0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}};
    int64_t rhs = 0, recomputed = 0;
  } imex_rot;
  // variable viscosity (nsfem_set_viscosity_law): law 0 none, 1 Smagorinsky, 2 Carreau, 4 WALE, 5 Vreman.  With a law the stored
  // vectors N1, N2 are c_c conv(u) + V(u); `epoch` counts the changes of law or parameters (a component of conv_key)
  struct Viscosity {
    int law = 0;
    double p[4] = {0.0, 0.0, 0.0, 0.0};
    int64_t epoch = 0, launches = 0, recomputed = 0;
  } visc;
  // What one use of the Germano-Lilly procedure (launch_dynamic_constant) owns: the buffers of its three launches,
  // `field` the constant at the vertices, the host copy of `sums` and the counters.  Two uses: dyn.buf (law 8, C_s^2 on
  // u) and sc.dynflux.buf (C_theta on (u, T)); each has buffers of its own because each may hold another level
  struct DynamicBuffers {
    bool allocated = false;
    nsfem::DevBuf<double> mom, vert, sums, field;
    std::vector<double> h_sums;
    int64_t runs = 0, launches = 0;
  };
  // dynamic Smagorinsky (law 8; p = {alpha, cs2_max}): what both uses of the procedure share -- the vertex-to-cell
  // CSR and the averaging groups (nsfem_set_dynamic_groups; global: one group of all vertices) -- and the buffers of
  // law 8, allocated when law 8 is first set and kept.  The constant is a function of the level it is evaluated on --
  // it is formed before every law-8 element launch and is no stored state; a change of the groups is a change of the
  // law (visc.epoch)
  struct Dynamic {
    bool global = true;
    int n_groups = 1;
    std::vector<int32_t> h_group;                   // [n_p1], what nsfem_set_dynamic_groups took (empty: global)
    nsfem::DevBuf<int32_t> vptr, vcell, goff, gvert;
    DynamicBuffers buf;
    // Lagrangian averaging (nsfem_set_dynamic_averaging mode 1): the constant is STATE that lives with the velocity
    // slots.  I = (I_LM, I_MM) of level n-1 (have_state); Inew and cs2_cur of level n, formed once by nsfem_step_imex
    // (cur_valid) and rotated by nsfem_advance (I <- Inew, cs2_prev <- cs2_cur, have_prev); buf.field is the scratch
    // of the runs that write no state (an N(u2) without cs2_prev, nsfem_imex_rhs, the hooks), work [n_p1][4] that of
    // nsfem_dynamic_lagrangian_advance.  Allocated by the first call of the setter with mode 1 and kept; a context
    // that never makes that call allocates nothing
    struct Lagrangian {
      int mode = 0;
      double theta = 1.5, cs2_init = 0.0256, cs2_floor = 1e-12;
      bool have_state = false, cur_valid = false, have_prev = false;
      nsfem::DevBuf<double> I, Inew, cs2_cur, cs2_prev, work;
    } lag;
  } dyn;
  // immersed bodies (nsfem_set_bodies): with bodies the stored vectors carry B(u) as well.  `cur` is the pose of t^n,
  // `prev` that of t^(n-1) (nsfem_move_bodies shifts cur to prev; without a move they are equal): a stored N(u2) was
  // formed with prev and one that has to be recomputed is formed with it again.  `epoch` counts the changes of the set,
  // eta or the smoothing (a component of conv_key)
  struct Bodies {
    nsfem::BodyTable cur, prev;
    int64_t epoch = 0, launches = 0, recomputed = 0;
    nsfem::DevBuf<double> work;     // partials and results of nsfem_body_forces
    // heated bodies (nsfem_set_body_temperatures): with a thermal body the stored scalar vectors carry H(T) as
    // well.  have_thermal: temperatures are set (n_thermal of them with flag 1); thermal_epoch counts the changes of
    // what the step's kernels see: the table with a thermal body, nothing without one
    nsfem::ThermalTable thermal;
    bool have_thermal = false;
    int n_thermal = 0;
    int64_t thermal_epoch = 0, fused_launches = 0, thermal_recomputed = 0;
    nsfem::DevBuf<double> heat_work;   // partials and results of nsfem_body_heat
  } bodies;
  // wall-stress model (nsfem_set_wall_model): with a model the stored vectors carry W(u) as well, added third.  `epoch`
  // counts the changes of the law, its parameters or the facet set (a component of conv_key); the host copies of what
  // the last call took (h_int, h_dbl) tell a change from the same data again
  struct WallModel {
    nsfem::WallModelDev dev;
    int64_t epoch = 0, launches = 0, recomputed = 0;
    std::vector<int32_t> h_int;
    std::vector<double> h_dbl;
  } wm;
  // CG needs a symmetric preconditioner: while IMEX steps run, the velocity cycle is V(d, d) instead of the
  // non-symmetric V(0, d + 1) the BiCGStab solves use (nsfem_set_bdf switches back)
  bool mg_v_symmetric = false;
  int mg_v_pre_saved = 0, mg_v_degree_saved = 0;
  int imex_last_path = 0;
  int64_t imex_lattice_rhs = 0, imex_generic_rhs = 0, imex_matrix_builds = 0;
  // IMEX scalar transport (nsfem_set_scalar / nsfem_step_scalar_imex): a P2 scalar on the velocity nodes, slots
  // NSFEM_T0 .. NSFEM_TCONV_2 (allocated on first use).  A = alpha0/k M + gamma0 kappa K on p22, rebuilt only when one
  // of the three numbers it was built from changes.  The stored convection vectors carry the weight (beta0 of their
  // step) they were evaluated with: the next step scales by beta1 / weight.
  struct Scalar {
    bool configured = false, buoyant = false, have_source = false;
    double kappa = 0.0, b[3] = {0.0, 0.0, 0.0};
    int form = 0;
    nsfem::BlockMat A;
    double built_a = NAN, built_g0 = NAN, built_kappa = NAN;
    nsfem::DevBuf<double> rhs, tmp, dinv, f_eff, bc_vals;
    nsfem::DevBuf<int32_t> bc_dofs;
    nsfem::DevBuf<uint8_t> mask;
    std::vector<int32_t> h_bc;
    int nbc = 0;
    bool conv1_fresh = false, conv2_valid = false;   // TCONV_1 written since the last advance / TCONV_2 usable
    double conv1_weight = 0.0, conv2_weight = 0.0;
    // subgrid heat flux (nsfem_set_scalar_sgs): prandtl_t > 0 switches D(u, T) on, the stored vectors carry it then.
    // sgs_epoch counts the changes of prandtl_t
    double prandtl_t = 0.0;
    int64_t sgs_epoch = 0, sgs_launches = 0, sgs_recomputed = 0;
    // dynamic subgrid heat flux (nsfem_set_scalar_sgs_dynamic): kappa_x = c_K Delta_K^2 gamma with C_theta from the
    // Germano identity of the scalar flux on the level pair of the launch -- formed before every SGS = 8 element
    // launch, no stored state.  A change of the switch or of ctheta_max counts in sgs_epoch; alpha and the groups are
    // the law's (visc.epoch).  The buffers are allocated by the first run and kept; the vertex-to-cell CSR and the
    // group list are those of `dyn`
    struct DynamicFlux {
      bool on = false;
      double ctheta_max = 0.0;
      DynamicBuffers buf;
    } dynflux;
    // Key of the stored vectors TCONV_1, TCONV_2: the form, bodies.thermal_epoch, bodies.epoch (compared only while a
    // body is thermal), sgs_epoch and visc.epoch (compared only while the subgrid term is on) they were formed with.
    // The three answers are kept apart: a stale heat key and a stale subgrid key are counted each on its own.
    // vouched (nsfem_set_state wrote NSFEM_TCONV_2): any form serves; the epochs are those of that call (ImexKey above)
    struct Key {
      int form = -1;
      int64_t thermal = 0, body = 0, sgs = 0, visc = 0;
      bool vouched = false;
      static Key of(const nsfem_ctx& c) {
        Key k;
        k.form = c.sc.form;
        k.thermal = c.bodies.thermal_epoch;
        k.body = c.bodies.epoch;
        k.sgs = c.sc.sgs_epoch;
        k.visc = c.visc.epoch;
        return k;
      }
      bool same_form(const Key& now) const { return vouched || form == now.form; }
      bool same_heat(const Key& now, bool heated) const { return thermal == now.thermal && (!heated || body == now.body); }
      bool same_sgs(const Key& now, bool sgs_on) const { return sgs == now.sgs && (!sgs_on || visc == now.visc); }
    } conv_key;
    int64_t matrix_builds = 0, conv_launches = 0, conv_reuses = 0;
    int dict_used = 0;
    bool dinv_dirty = true;                          // 1 / diagonal belongs to an older matrix or Dirichlet set
  } sc;
  nsfem::DevBuf<double> state[NSFEM_N_SLOTS];
  bool have_body_force = false, have_traction = false;
  // Dirichlet data
  int nbc_v = 0, nbc_p = 0;
  nsfem::DevBuf<int32_t> bc_v_dofs, bc_p_dofs;
  nsfem::DevBuf<double> bc_v_vals, bc_p_vals;
  nsfem::DevBuf<uint8_t> mask_v, mask_p;
  // per-system work vectors
  nsfem::DevBuf<double> rhs_v, rhs_p, dx_v, gconst, tmp_v, tmp_p, dinv_v, dinv_p, dinv_m;
  bool dinv_p_ready = false, dinv_m_ready = false;
  int64_t mass_dinv_epoch = 0, mass_dinv_copied_epoch = -1;   // dinv_m recomputed / copied into the mass smoother
  nsfem::KrylovWork kw;
  int assembled_system = -1;
  double area = 0.0;
  uint64_t graph_epoch = 1; // captured iteration graphs are valid within one epoch
  int conv_form = 0;        // 0 standard, 1 rotational, 2 divergence, 3 skew-symmetric
  bool picard = false;      // Picard instead of Newton linearisation of the convection
  // ---- multigrid hierarchy (optional; nsfem_mg_add_level / nsfem_mg_finalize)
  struct P1Level {
    int n = 0;
    nsfem::MeshDev mesh;
    nsfem::Pattern pat;
    nsfem::BlockMat K, M, Lc;
    nsfem::StencilDict dict;                   // lattice levels: rows of K, M and every combination of them
    nsfem::Transfer to_finer;
    std::vector<uint8_t> h_ghost;              // per node (partitioned meshes)
    nsfem::HaloRange halo;
    bool has_halo = false;
  };
  // ---- partitioned meshes (nsfem_set_partition + nsfem_comm_attach_*)
  nsfem::Comm* comm = nullptr;                 // owned
  nsfem::HaloRange halo_p2, halo_p1;
  std::vector<uint8_t> h_ghost_p2, h_ghost_p1; // per node: nonzero = ghost
  int p2_gh_lo = -2, p2_gh_hi = -2;            // ghost lattice lines of the P2 lattice of a strip (-2: not looked at, -1: none such)
  nsfem::DevBuf<uint8_t> ghost_v, ghost_p;     // per vector entry: 0 / 2
  int64_t n_p2_global = 0, n_p1_global = 0;
  P1Level* global_coarse = nullptr;            // replicated global coarsest mesh (owned)
  std::vector<P1Level*> global_tail;           // its coarser levels, finest first (owned)
  nsfem::Multigrid mg_p_tail, mg_v_tail;       // replicated hierarchies below global_coarse
  nsfem::Multigrid mg_mv;                      // one level: Chebyshev solver of the velocity mass matrix
  double mass_kappa = 0.0;
  double mg_trunc_ratio = 4.0;                 // > 0: truncate the velocity cycle where nu K_ii <= ratio * alpha M_ii
  double mg_trunc_tol = 0.1;
  int64_t glob_off = 0;
  std::vector<int32_t> h_glob_idx;             // unstructured partitions: local coarsest node -> global id
  nsfem::DevBuf<int32_t> glob_idx;
  std::vector<nsfem::HaloLists*> halo_lists;   // owned (nsfem_set_halo_lists)
  bool partition_periodic = false;
  bool overlap = false;                        // halo exchanges under the interior rows (nsfem_set_overlap)
  double area_global = 0.0;                    // measure of the whole (partitioned) domain, lazily all-reduced
  // NSFEM_FORCE_COMM=1 routes a single-rank run through the communicator as well (lets a
  // one-GPU box exercise the RCCL all-reduce calls)
  bool distributed() const {
    static const bool force = std::getenv("NSFEM_FORCE_COMM") != nullptr;
    return comm && (comm->size > 1 || force);
  }
  std::vector<int32_t> h_p2map, h_p1map;       // host copies of the fine dof maps
  std::vector<P1Level*> coarse;                // owned
  nsfem::Transfer t_p2p1;                      // P2 (fine mesh) <- P1 (fine mesh)
  nsfem::BlockMat Lc0;                         // alpha0/k M_p + c_v A_p on the fine P1 space
  nsfem::Multigrid mg_p, mg_v;
  bool cor_start_ready = false;                // correction_assemble produced the mass solve's start residual and sums
  uint64_t cor_start_touch = 0;                //   ... and nobody has used the Krylov work vectors since (kw.touch)
  // fused step frame (NSFEM_STEP_FUSED at creation).  cor_finish_pending: correction_assemble left U0 unwritten and
  // the sums of slots 12, 13 unformed -- k_correction_finish after the first Chebyshev sequence supplies them
  bool step_fused = true;
  bool cor_finish_pending = false;
  // launches so far: pair kernel begin step / correction, k_correction_finish, fused projection epilogue
  int64_t step_frame_launches[4] = {0, 0, 0, 0};
  // frame of the Newton iteration of nsfem_step_ipcs in the residual launch (NSFEM_NEWTON_FUSED at creation; see
  // launch_residual_frame_lattice).  newton_update_pending: the solve left u* -= dx to the residual launch that follows;
  // that launch writes the new u* to ustar_alt and the two buffers are exchanged behind state[NSFEM_USTAR]
  bool newton_fused = true;
  bool newton_update_pending = false;
  nsfem::DevBuf<double> bc_v_dense;            // the velocity Dirichlet values as a dense vector (0 elsewhere)
  nsfem::DevBuf<double> ustar_alt;             // second u* buffer
  nsfem::DevBuf<double> tile_parts;            // one sum of squares per tile of the residual launch
  int64_t newton_frame_launches[2] = {0, 0};   // residual launches with the frame, those among them with the update
  nsfem::FastDiag fd_p{&comm};                 // direct projection-step solver on tensor-product lattices
  nsfem::FastDiag3 fd3_p{&comm};               // the same on 3D box lattices (direct or CG preconditioner)
  // the factors precond = 3 uses: the 3D ones if set, else the 2D ones, else none (a setter releases the other object)
  nsfem::FastDiagBase* fast_diag() {
    if (fd3_p.ready()) return &fd3_p;
    return fd_p.ready() ? &fd_p : nullptr;
  }
  // the projection step can take the pass-and-check driver (poisson_direct_step): exact factors, partitioned exactly
  // when the context is
  bool fast_diag_direct() {
    nsfem::FastDiagBase* fd = fast_diag();
    return fd && fd->exact && distributed() == fd->partitioned();
  }
  bool fd_p_singular = false;
  bool mg_built = false, mg_p_dirty = true, mg_v_dirty = true;
  std::vector<int32_t> h_bc_v, h_bc_p;         // host copies of the Dirichlet dof sets
  struct MomentumPrec : nsfem::Precond {
    nsfem_ctx* c = nullptr;
    void apply(hipStream_t s, const double* r, double* z) override;
  } mom_prec;
  // host-supplied CSR operators (algebraic Schur Laplacian per multigrid level)
  struct CsrOp {
    nsfem::Pattern pat;
    nsfem::BlockMat mat;
    nsfem::StencilDict dict;                   // lattice meshes: smoothing steps run on the dictionary copy
  };
  std::vector<CsrOp*> schur_ops;               // owned
  nsfem::StencilDict dict22;                   // rows of the scalar P2 operators (ensure_L)
  bool dict22_tried = false;
  nsfem::StencilDict dict11;                   // rows of the scalar P1 operators of the fine mesh
  bool dict11_tried = false;
  nsfem::StencilDict dict21, dict12, dict21g;  // divergence-transpose / divergence / gradient blocks
  bool dictD_tried = false;
  int bc_p_any = -1;                           // partitioned: pressure Dirichlet dofs on any rank (-1 unknown)
  bool schur_additive = false;                 // operators of nsfem_mg_set_schur_operator are rank parts
  int schur_singular = -1;                     // -1: geometric hierarchy (singular iff no Dirichlet set)
  // monolithic BDF system: mixed operator, block preconditioner and their data
  nsfem::Multigrid mg_s, mg_m;                 // Schur Laplacian V-cycle, pressure-mass smoother
  bool mg_s_dirty = true;
  std::vector<int32_t> h_bc_s;
  nsfem::DevBuf<uint8_t> mask_s;
  nsfem::DevBuf<double> rhs_m, dx_m;
  // matrix-free velocity Jacobian (tetrahedral meshes): y = L x + c_c [d conv(u)/du] x with
  // identity rows on Dirichlet dofs and zero ghost rows; u = state[vel_slot]
  struct MomentumMF : nsfem::Operator {
    nsfem_ctx* c = nullptr;
    int vel_slot = 3;               // NSFEM_USTAR
    void apply(hipStream_t s, const double* x, double* y) override;
  } mom_mf;
  nsfem::DevBuf<uint8_t> mask_m;     // ghost flags of the pressure mass smoother (partitioned)
  double prec_shift = 0.0;          // mass shift of the velocity / Schur preconditioners
  nsfem::BlockMat Lprec;            // (alpha0/k + shift) M + c_v K when shift != 0
  // iteration predictor of a recurring solve (see hinted / next_hint in api.hip): the count the same solve needed
  // in the previous step, how many solves in a row needed exactly that count, and the number of solves so far
  struct SolveHint { int its = 0, same = 0; int64_t count = 0; };
  SolveHint hint_mom[4], hint_poi, hint_cor, hint_sc;
  // in-situ timing of the matrix-free convection action (k_conv_cell + k_res_gather): one HIP-event
  // pair per application while enabled (nsfem_profile_convection; bench.py's assembly roofline)
  struct Probe {
    bool on = false;
    std::vector<hipEvent_t> ev;
    size_t n = 0;
    ~Probe() { for (hipEvent_t e : ev) (void)hipEventDestroy(e); }
  } conv_probe;
  // nsfem_volume_functionals: partial sums + results, resident reference fields and cell flags (with the host copy
  // the next call's flags are compared against), and on partitioned meshes the copies of the two slots whose ghost
  // entries are exchanged (the state itself is not written)
  nsfem::DevBuf<double> vf_parts, vf_ref_u, vf_ref_p, vf_u, vf_p;
  nsfem::DevBuf<uint8_t> vf_flags;
  std::vector<uint8_t> vf_flags_host;
  // point location / evaluation / tracers (points.hip): the bins of nsfem_set_point_locator, grow-only work buffers of
  // nsfem_locate_points / nsfem_eval_points, and the particle cloud of nsfem_tracers_*
  struct Points {
    bool have_locator = false;
    nsfem::PointLocatorDev loc;
    nsfem::DevBuf<int32_t> bin_ptr, bin_cells;
    nsfem::DevBuf<double> x, out;
    nsfem::DevBuf<int32_t> cells;
    int64_t n_tracers = -1;                     // -1: nsfem_tracers_set has not been called
    nsfem::DevBuf<double> tx;                   // [n][dim]
    nsfem::DevBuf<int32_t> tcell, tcounts;      // [n]; [workgroups][2]: (left, bin-search fallbacks of the last call)
    nsfem::DevBuf<uint8_t> tstatus;             // [n] 0 moving, 1 left
    int64_t advect_calls = 0;
  } pts;
  // running flow statistics (statistics.hip, nsfem_stats_*): nothing is allocated before nsfem_stats_enable
  struct Stats {
    uint32_t flags = 0;                         // 0: not enabled
    double W = 0.0;                             // accumulated weight, the same for every node
    int64_t samples = 0, launches = 0;
    size_t stride2 = 0, stride1 = 0;
    nsfem::DevBuf<double> acc2, acc1, out;      // P2 / P1 accumulators; grow-only read-out buffer
    struct Groups {
      int32_t n = -1;                           // -1: nsfem_stats_set_groups has not been called
      nsfem::DevBuf<int32_t> ptr, nodes;
      nsfem::DevBuf<double> weights;
    } groups[2];
  } stats;
  // nsfem_derived_fields (derived.hip): the grow-only work buffer of its own (result + node-sorted element planes;
  // never m.rbuf / m.ebuf) and the counters of nsfem_derived_info
  struct Derived {
    nsfem::DevBuf<double> work;
    int64_t cell_launches = 0, gather_launches = 0, calls = 0;
  } derived;
  // nsfem_spectrum_set / nsfem_spectrum_compute (spectrum.hip): the one transform-and-bin plan of the context -- the
  // matrices of the transformed axes, the node of every lattice point, the bin CSR cut into chunks, two work arrays of
  // one component each, the chunk partials and the result -- and the counters of nsfem_spectrum_info.  All of it is
  // allocated by nsfem_spectrum_set; nsfem_spectrum_compute allocates nothing
  struct Spectrum {
    bool have_plan = false;
    int32_t n[3] = {0, 0, 0}, n_bins = 0, n_chunks = 0, max_node = -1;
    nsfem::DevBuf<double> F[3], w0, w1, parts, out;
    nsfem::DevBuf<int32_t> node_of_point, bin_points, chunk_ptr, bin_chunk_ptr;
    int64_t transform_launches = 0, bin_launches = 0, calls = 0;
    int64_t bytes() const {
      size_t d = w0.n + w1.n + parts.n + out.n, i = node_of_point.n + bin_points.n + chunk_ptr.n + bin_chunk_ptr.n;
      for (const auto& f : F) d += f.n;
      return (int64_t)(d * sizeof(double) + i * sizeof(int32_t));
    }
    void release() {
      have_plan = false;
      n[0] = n[1] = n[2] = n_bins = n_chunks = 0;
      max_node = -1;
      for (nsfem::DevBuf<double>* b : {&F[0], &F[1], &F[2], &w0, &w1, &parts, &out}) b->release();
      for (nsfem::DevBuf<int32_t>* b : {&node_of_point, &bin_points, &chunk_ptr, &bin_chunk_ptr}) b->release();
    }
  } spectrum;
  // nsfem_wall_set_facets / nsfem_wall_compute (wall.hip): the resident facet set, sorted by group (stable), its
  // group offsets, the permutation back to the caller's order (host only), the buffers of the rows and of the group sums -- all the
  // context's own, sized by nsfem_wall_set_facets -- and the counters of nsfem_wall_info
  struct Wall {
    bool have_set = false;
    int32_t n_facets = 0, n_groups = 0;
    nsfem::DevBuf<int32_t> fcell, flocal, goff;
    nsfem::DevBuf<double> rows, sums;
    std::vector<int32_t> h_perm;             // h_perm[k] = input index of the k-th resident facet
    std::vector<double> h_rows;              // staging of the rows for the un-permuted copy
    int64_t computes = 0, uploads = 0;
  } wall;
  int64_t jac_lattice_launches = 0;   // applications of the matrix-free Jacobian through k_jac_lattice
  bool mf_active = false;           // the running step driver applies the Jacobian matrix-free
  bool mono_mf = false;             // nsfem_assemble(NSFEM_SYS_MONOLITHIC): the solve that follows runs matrix-free
  double mono_rnorm = -1.0;         // ... and |rhs_m| as that assembly evaluated it
  int pressure_history = 0;         // IPCS: pressure levels shifted since the state was last set (0..2)
  struct MixedOp : nsfem::Operator {
    nsfem_ctx* c = nullptr;
    void apply(hipStream_t s, const double* x, double* y) override;
  } mixed_op;
  struct BlockPrec : nsfem::Precond {
    nsfem_ctx* c = nullptr;
    void apply(hipStream_t s, const double* r, double* z) override;
  } block_prec;
  ~nsfem_ctx() {
    if (comm) comm->release_streams();
    for (P1Level* p : coarse) delete p;
    for (nsfem::HaloLists* h : halo_lists) delete h;
    for (CsrOp* p : schur_ops) delete p;
    for (P1Level* p : global_tail) delete p;
    delete global_coarse;
    delete comm;
  }
};
