/*
 * nsfem.h -- C ABI of libnsfem_hip.so: MI355X (gfx950) implementation of the
 * per-time-step Taylor-Hood (P2/P1) assembly + sparse solve that the reference
 * (LKM-code-base/NavierStokes-with-Fenics) delegates to FEniCS/PETSc.
 *
 * Nothing like this interface exists in the reference (it is pure Python on top
 * of dolfin).  Every entry point names the reference call it replaces; the
 * Python binding a maintainer would add is shown in INTEGRATION.md.
 *
 * Conventions
 *   - plain C types only; every function returns int (0 = ok, <0 = nsfem_status),
 *     no C++ exception crosses the boundary; nsfem_last_error() gives the text.
 *   - the caller owns every host buffer it passes (read during the call only);
 *     the library owns all device memory; nothing returned outlives
 *     nsfem_destroy().
 *   - one context per process x device, one HIP stream per context; calls on a
 *     context are not re-entrant (the reference is single threaded).
 *   - all floating point data is fp64, all indices int32.
 *   - dim = 2 (triangles) or 3 (tetrahedra); velocity vectors are node-interleaved:
 *     index = dim * p2_node + component; "mixed" vectors are
 *     [velocity (dim * n_p2) | pressure (n_p1)].
 */
#ifndef NSFEM_H
#define NSFEM_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct nsfem_ctx nsfem_ctx;

enum nsfem_status {
  NSFEM_OK = 0,
  NSFEM_ERR_ARG = -1,         /* bad argument / wrong call order            */
  NSFEM_ERR_HIP = -2,         /* HIP runtime error (no device, OOM, ...)     */
  NSFEM_ERR_BREAKDOWN = -3,   /* Krylov breakdown (rho / omega = 0, NaN)     */
  NSFEM_ERR_NOT_CONVERGED = -4, /* Newton / Krylov hit its iteration limit   */
  NSFEM_ERR_COMM = -5         /* RCCL error                                  */
};

/* Mesh + dof maps: what dolfin.Mesh / FunctionSpace(mesh, P2^d x P1) hold in the
 * reference (source/ns_solver_base.py:501-524).  Affine simplices: triangles (dim = 2) or
 * tetrahedra (dim = 3); local P2 order = vertices, then the edge midpoints in UFC edge order
 * (triangle: e(v1v2), e(v0v2), e(v0v1); tetrahedron: e(v2v3), e(v1v3), e(v1v2), e(v0v3), e(v0v2),
 * e(v0v1)). */
typedef struct {
  int32_t dim;               /* 2 or 3                                        */
  int32_t n_cells;
  int32_t n_vertices;
  int32_t n_p2;              /* scalar P2 nodes                               */
  int32_t n_p1;              /* P1 nodes                                      */
  const double* coords;      /* [n_vertices * dim]                            */
  const int32_t* cells;      /* [n_cells * (dim + 1)] vertex ids              */
  const int32_t* p2_dofmap;  /* [n_cells * 6 | 10]                            */
  const int32_t* p1_dofmap;  /* [n_cells * (dim + 1)]                         */
} nsfem_mesh_desc;

/* state slots (device-resident vectors) */
enum nsfem_slot {
  NSFEM_U0 = 0,      /* velocity at t_{n+1}   (IPCS _velocities[0]) [dim*n_p2] */
  NSFEM_U1 = 1,      /* velocity at t_n                                       */
  NSFEM_U2 = 2,      /* velocity at t_{n-1}                                   */
  NSFEM_USTAR = 3,   /* IPCS _intermediate_velocity                           */
  NSFEM_P = 4,       /* pressure                                    [n_p1]    */
  NSFEM_P_OLD = 5,   /* IPCS _old_pressure / BDF pressure at t_n              */
  NSFEM_BODY_FORCE = 6, /* nodal P2 interpolant of f             [dim*n_p2]   */
  NSFEM_TRACTION = 7,   /* assembled boundary traction vector    [dim*n_p2]   */
  NSFEM_P2_OLD = 8,  /* BDF: pressure at t_{n-1} (keeps _solutions[2] whole)  */
  NSFEM_CONV_N1 = 9, /* IMEX: c_c N(u^n), written by nsfem_step_imex    [dim*n_p2] */
  NSFEM_CONV_N2 = 10, /* IMEX: c_c N(u^(n-1)); nsfem_advance moves N1 here       */
  /* scalar transport (nsfem_set_scalar): a P2 scalar on the velocity nodes, [n_p2] each, allocated on first use */
  NSFEM_T0 = 11,       /* scalar at t_{n+1}, written by nsfem_step_scalar_imex                  */
  NSFEM_T1 = 12,       /* scalar at t_n                                                          */
  NSFEM_T2 = 13,       /* scalar at t_{n-1}                                                      */
  NSFEM_T_SOURCE = 14, /* nodal P2 interpolant of the source q (optional)                        */
  NSFEM_TCONV_1 = 15,  /* beta0 C(u^n) T^n, written by nsfem_step_scalar_imex                    */
  NSFEM_TCONV_2 = 16,  /* the vector of the step before; nsfem_advance moves TCONV_1 here.  Set by hand it is
                          read as the unweighted C(u^(n-1)) T^(n-1)                              */
  NSFEM_N_SLOTS = 17
};

/* fields for Dirichlet sets */
enum nsfem_field {
  NSFEM_VELOCITY = 0,
  NSFEM_PRESSURE = 1,
  NSFEM_PRESSURE_PRECOND = 2,  /* Dirichlet set of the pressure Laplacian used inside the
                                  Schur-complement preconditioner of the monolithic scheme
                                  (P1 nodes on open boundaries + true pressure conditions) */
  NSFEM_SCALAR = 3             /* transported P2 scalar (nsfem_step_scalar_imex): dofs index the P2 nodes */
};

/* operators that can be exported / applied (parity tests, _assemble_system) */
enum nsfem_operator {
  NSFEM_OP_MASS_P2 = 0,      /* scalar P2 mass               n_p2 x n_p2      */
  NSFEM_OP_STIFF_P2 = 1,     /* scalar P2 stiffness                           */
  NSFEM_OP_STIFF_P1 = 2,     /* (grad p, grad q)  ns_ipcs_solver.py:160       */
  NSFEM_OP_MASS_P1 = 3,
  NSFEM_OP_DIV = 4,          /* (div u, q)       n_p1 x dim n_p2              */
  NSFEM_OP_GRAD = 5,         /* (grad p, w)      dim n_p2 x n_p1              */
  NSFEM_OP_DIVT = 6,         /* (p, div w)       dim n_p2 x n_p1              */
  NSFEM_OP_MOMENTUM_JAC = 7, /* IPCS/BDF velocity block of the Newton matrix  */
  NSFEM_OP_VISCOUS_EXTRA = 8, /* traction-form extra block (grad u^T : grad v) */
  NSFEM_OP_MOMENTUM_JAC_MF = 9, /* nsfem_operator_apply only: matrix-free velocity Jacobian */
  NSFEM_OP_MOMENTUM_SMOOTHER = 10, /* nsfem_time_spmv only: finest-level Chebyshev step of the
                                     velocity multigrid (scalar P2 operator, fused epilogue) */
  NSFEM_OP_CONVECTION_ACTION = 11 /* nsfem_time_spmv only: matrix-free convection action
                                     (element kernel + node gather), cache-cold            */
};

enum nsfem_system {
  NSFEM_SYS_MOMENTUM = 0,    /* IPCS diffusion step  ns_ipcs_solver.py:106-147 */
  NSFEM_SYS_POISSON = 1,     /* projection step      ns_ipcs_solver.py:149-171 */
  NSFEM_SYS_CORRECTION = 2,  /* velocity correction  ns_ipcs_solver.py:173-196 */
  NSFEM_SYS_MONOLITHIC = 3   /* BDF mixed system     ns_bdf_solver.py:36-100   */
};

typedef struct {
  double rtol;          /* relative residual (to |b|) tolerance                */
  double atol;          /* absolute residual tolerance                         */
  int32_t max_iter;
  int32_t precond;      /* 0 = Jacobi, 1 = multigrid (where available), 2 = (velocity mass
                           solve only) Chebyshev iteration with a-priori element bounds:
                           no dot products, no all-reduce inside the iteration;
                           3 = (projection step only) direct solve by fast diagonalisation on
                           tensor-product lattices, see nsfem_poisson_set_fast_diag            */
  int32_t check_every;  /* host convergence check interval (>=1)               */
  int32_t first_check;  /* iterations before the first host convergence check (every check is a
                           device -> host round trip; the step drivers set it from the iteration
                           count the same solve needed in the previous step)     */
} nsfem_krylov_opts;

typedef struct {
  int32_t iterations;
  int32_t converged;
  double residual;      /* final |r|_2                                          */
  double residual0;     /* initial |r|_2                                        */
} nsfem_solve_info;

typedef struct {
  double newton_atol;   /* reference: tol (1e-10)   ns_ipcs_solver.py:144       */
  double newton_rtol;   /* reference: 10 * tol                                  */
  int32_t newton_max_iter; /* reference: 50                                     */
  int32_t convective_form; /* 0 standard, 1 rotational, 2 divergence, 3 skew-symmetric */
  nsfem_krylov_opts momentum;   /* BiCGStab */
  nsfem_krylov_opts poisson;    /* CG       */
  nsfem_krylov_opts correction; /* CG       */
  int32_t picard;               /* monolithic step: Picard instead of Newton matrix
                                   (StationarySolverBase, ns_solver_base.py:930-934)        */
  int32_t allow_nonconvergence; /* monolithic step: return instead of failing when the
                                   iteration limit is hit (error_on_nonconvergence=False)   */
  double newton_forcing;        /* 0: every Newton linear solve to the Krylov tolerances given
                                   (direct-solver accuracy, parity runs).  eta > 0: inexact
                                   Newton -- linear residual reduced by eta, at most down to a
                                   tenth of the nonlinear target; the Newton loop still stops on
                                   the reference's criterion (throughput runs)              */
  int32_t matrix_free;          /* velocity Jacobian inside the step drivers: 0 auto (= matrix-
                                   free: L x + linearised convection by an element kernel),
                                   1 assembled block CSR, 2 matrix-free                      */
  int32_t pressure_extrapolation; /* IPCS projection step: start the CG iteration from the linear
                                   extrapolation 2 p_n - p_(n-1) instead of p_n (the reference's direct
                                   solve has no initial guess; the converged pressure is the same, the
                                   iteration starts closer to it).  0 = off (default)               */
} nsfem_step_opts;

#define NSFEM_MAX_NEWTON 64
typedef struct {
  int32_t newton_iterations;
  int32_t krylov_iterations_momentum;   /* summed over Newton iterations        */
  int32_t krylov_iterations_poisson;
  int32_t krylov_iterations_correction;
  double newton_residuals[NSFEM_MAX_NEWTON]; /* |b| after 0,1,.. updates        */
  int32_t converged;
  int32_t reserved;
} nsfem_step_info;

/* ---- life cycle: replaces FunctionSpace/Function construction
 * (source/ns_solver_base.py:501-524,1018-1025; ns_ipcs_solver.py:66-82) ------ */
int nsfem_create(const nsfem_mesh_desc* mesh, int device, nsfem_ctx** out);
void nsfem_destroy(nsfem_ctx* ctx);
const char* nsfem_last_error(const nsfem_ctx* ctx);   /* ctx may be NULL: last create error */
int nsfem_version(void);

/* ---- coefficients: replaces set_equation_coefficients (ns_solver_base.py:829-855)
 * c = {convective, pressure, viscous, body_force, coriolis, euler}; NaN = None */
int nsfem_set_coeffs(nsfem_ctx* ctx, const double c[6]);
/* replaces _update_time_stepping_coefficients (ns_ipcs_solver.py:210-227) */
int nsfem_set_bdf(nsfem_ctx* ctx, const double alpha[3], double k);
/* coefficients of the IMEX pressure-correction step (imex_time_stepping.py: alpha, beta, gamma) and the step size k.
 * The system matrix alpha0/k M + gamma0 c_v K and the velocity multigrid hierarchy are rebuilt only when alpha0/k or
 * gamma0 changed.  nsfem_set_bdf switches back to the fully implicit schemes (gamma = (1, 0, 0)). */
int nsfem_set_imex(nsfem_ctx* ctx, const double alpha[3], const double beta[2], const double gamma[3], double k);
/* replaces DirichletBC lists (ns_solver_base.py:546-660); re-callable each step
 * (time dependent values, _set_time ns_solver_base.py:1033-1104).  dofs index the
 * velocity (interleaved) or pressure vector (NSFEM_SCALAR: the P2 nodes); later entries win on duplicates. */
int nsfem_set_dirichlet(nsfem_ctx* ctx, int field, int32_t n, const int32_t* dofs,
                        const double* vals);
/* convective term form (ns_solver_base.py:370-390): 0 standard, 1 rotational, 2 divergence,
 * 3 skew-symmetric; picard != 0 selects the Picard linearisation (:478-499) for the matrices
 * assembled through nsfem_assemble (the fused step drivers take the form from their options) */
int nsfem_set_convective_form(nsfem_ctx* ctx, int form, int picard);
/* viscous term form: 0 reduced, 1 traction (ns_solver_base.py:662-673) */
int nsfem_set_viscous_form(nsfem_ctx* ctx, int traction_form);

/* ---- state transfer: Function.vector() get/set ------------------------------ */
int nsfem_set_state(nsfem_ctx* ctx, int slot, const double* host, int64_t n);
int nsfem_get_state(nsfem_ctx* ctx, int slot, double* host, int64_t n);
int64_t nsfem_state_size(const nsfem_ctx* ctx, int slot);
void* nsfem_state_devptr(nsfem_ctx* ctx, int slot);   /* device pointer (plumbing) */

/* ---- the explicit assembly seam (_assemble_system) ------------
 * Assembles matrix and right-hand side / residual of one system from the current
 * state; replaces the implicit dolfin assemble() inside *VariationalSolver.solve().
 * NSFEM_SYS_MONOLITHIC (single contexts, multigrid hierarchy attached): the Newton residual of nsfem_step_bdf about
 * U0 / P in a mixed vector of nvel + npre entries (nsfem_get_rhs, nsfem_residual_norm), the Jacobian and the block
 * preconditioner's hierarchies; flags bit 0: a new time step, bit 1: the Jacobian is applied matrix-free.
 * nsfem_solve then runs the step's block-preconditioned BiCGStab from zero with the caller's options and subtracts
 * the solution from U0 and P: one Newton iteration of nsfem_step_bdf. */
int nsfem_assemble(nsfem_ctx* ctx, int system, uint32_t flags);
/* 2-norm of the assembled residual / rhs (Dirichlet rows: x_i - g_i for Newton) */
int nsfem_residual_norm(nsfem_ctx* ctx, int system, double* out);
int nsfem_get_rhs(nsfem_ctx* ctx, int system, double* host, int64_t n);
/* Krylov solve of the assembled system; replaces PETSc LU */
int nsfem_solve(nsfem_ctx* ctx, int system, const nsfem_krylov_opts* opts,
                nsfem_solve_info* info);

/* ---- operator introspection for parity tests -------------------------------- */
int nsfem_operator_shape(nsfem_ctx* ctx, int op, int64_t* n_rows, int64_t* n_cols,
                         int64_t* nnz_scalar);
/* scalar CSR copy (blocks expanded); arrays sized from nsfem_operator_shape */
int nsfem_operator_export(nsfem_ctx* ctx, int op, int32_t* rowptr, int32_t* col, double* val);
/* diagonal of a square scalar operator (n_rows doubles) without exporting the matrix */
int nsfem_operator_diagonal(nsfem_ctx* ctx, int op, double* out);
/* y = op * x on the device through the production SpMV kernel (host in/out) */
int nsfem_operator_apply(nsfem_ctx* ctx, int op, const double* x, double* y);
/* Test hook (parity tests): ONE product / residual / Chebyshev-Jacobi smoothing sequence of the scalar
 * lattice operator  a M + b K  (space 0: P2 mass / stiffness of the fine mesh on nv interleaved
 * components; space 1: P1 mass / stiffness) through a CHOSEN kernel family, on host data -- so that every
 * SpMV kernel family and every epilogue can be pinned to the oracle's matrices directly.
 *   family   0 library default, 1 CSR (stream / lane-group), 2 SELL-64, 3 stencil dictionary (one step per
 *            launch), 4 multi-step lattice kernel (all steps in one launch; epilogue 3 only)
 *   epilogue 0  y = A x   1  y = b - A x   3  `steps` steps  d = c1[k] d + c2[k] D^-1 (b - A x), x += d
 *   maskmode 0 none, 1 identity rows, 2 zero rows (flags in `mask`, one per vector entry; flag 2 = ghost)
 * Outputs: y (result / last iterate), d_out, r_out (b - A y when with_residual), and which family ran.
 * Family 4 only -- the launches the multigrid cycles make (W x H: the operator's lattice):
 *   xc          host [((W + 1) / 2) ((H + 1) / 2) nv] or NULL: fused prolongation, start = [x +] P xc (x may be
 *               NULL: start = P xc alone; rows flagged in the mask start at 0)
 *   rf          host [(2 W - 1) (2 H - 1) nv] or NULL: fused restriction, b = R rf (flagged rows 0); b is not read
 *   b_formed    host [n * nv] or NULL: the right-hand side the launch stored (with rf)
 *   gh_lo, gh_hi, gh_zero   frozen ghost lines of a partitioned strip (flag every component of their rows)
 *   tile_lines  0 the launcher's choice; 16, 24, 32 or 48 forced (refused when the halo does not fit)
 *   fixed       -1 default (on), 0 compile-time-offset stages off, 1 on
 *   lattice_*   out: the geometry of the launch and its fixed_shape
 * d_out NULL (family 4): the launch stores no direction. */

typedef struct {
  int32_t space, nv, family, epilogue, steps, maskmode, ghost, ident, from_zero, with_residual, dict_ok;
  int32_t used_family;        /* out */
  int32_t dict_entries, dict_exact, lattice_w;   /* out: dictionary of the pattern (0: none) */
  int32_t lattice_kind;       /* out (family 4): launch kind that ran, 64 | operand flags, 0: runtime-flag kernel */
  double a, b_coef;
  double c1[8], c2[8];
  const double *x, *b, *d;    /* host [n * nv]; b, d may be NULL */
  const uint8_t* mask;        /* host [n * nv] or NULL */
  double *y, *d_out, *r_out;  /* host [n * nv]; d_out, r_out may be NULL */
  const double *xc, *rf;
  double* b_formed;
  int32_t gh_lo, gh_hi, gh_zero, tile_lines, fixed;
  int32_t lattice_tile_lines, lattice_tx, lattice_ty, lattice_tiles, lattice_fixed_shape;   /* out */
} nsfem_kernel_test;
int nsfem_kernel_apply(nsfem_ctx* ctx, nsfem_kernel_test* t);
/* Test hook: the standalone restrictions of a lattice hierarchy on host data.  levels = 1: b1 = R rf through
 * k_restrict_lattice, coarse lattice w x h, fine (2 w - 1) x (2 h - 1), rows flagged in mask1 get 0.  levels = 2:
 * b1 = R rf, b2 = R b1 through k_restrict_lattice2, coarsest lattice w x h (mask2), middle (2 w - 1) x (2 h - 1)
 * (b1, mask1), fine (4 w - 3) x (4 h - 3).  nv = 1 or 2 interleaved components; masks may be NULL. */
int nsfem_lattice_restrict(nsfem_ctx* ctx, int nv, int levels, int w, int h, const double* rf, const uint8_t* mask1,
                           const uint8_t* mask2, double* b1, double* b2);

/* ---- multigrid hierarchy (optional).  Coarse P1 levels are added finest-first; each
 * carries its mesh and the prolongation P (CSR, rows = nodes of the previous finer P1
 * level, n_fine of them; cols = nodes of this level).  Spaces must be nested (every
 * coarse node coincides with a finer node: a row of P with the single entry 1).  The
 * library integrates the coarse operators on the device, adds the P2 <- P1 transfer of
 * the fine mesh itself and builds two V-cycle preconditioners: pressure Poisson and
 * alpha0/k M + c_v K.  Selected per solve with nsfem_krylov_opts.precond = 1. */
/* contiguous halo ranges of a strip (2D) / slab (3D) partition, in node units (offset, count) */
typedef struct {
  int64_t send_up_off, send_up_cnt, recv_above_off, recv_above_cnt;
  int64_t send_down_off, send_down_cnt, recv_below_off, recv_below_cnt;
} nsfem_halo;
typedef struct {
  int32_t n_vertices, n_cells;
  const double* coords;      /* [n_vertices * dim]     */
  const int32_t* cells;      /* [n_cells * (dim + 1)]  */
  int32_t n_fine;
  const int32_t* p_rowptr;   /* [n_fine + 1]     */
  const int32_t* p_col;
  const double* p_val;
  const uint8_t* ghost;      /* one flag per P1 dof of the level ([n_vertices], or [n_dofs] with a
                                dofmap): nonzero = ghost; NULL on unpartitioned meshes */
  nsfem_halo halo;           /* used when ghost != NULL */
  /* constrained (periodic) spaces: the P1 dof of every cell vertex, [n_cells * (dim + 1)], with
   * n_dofs < n_vertices distinct ids (slaves share their master's dof); the geometry still comes
   * from coords[cells].  NULL / 0: dof = vertex id.  P then has n_dofs columns. */
  const int32_t* dofmap;
  int32_t n_dofs;
  int32_t transfer_kind;     /* how Dirichlet / ghost flags travel down this transfer: 1 = nested levels (a coarse node
                                takes the flag of the finer node it coincides with: the row of P with the single entry
                                1), 2 = non-nested interpolation (the finer node its hat function weighs most, weight
                                >= 1/2), 0 = decide from the values of P (every entry 1 or 1/2 -> nested) */
} nsfem_mg_level_desc;
typedef struct {
  int32_t smoother_degree;   /* Chebyshev steps per pre/post smoothing (default 2) */
  int32_t coarse_dense_max;  /* dense coarse solve up to this many unknowns (1200)  */
  double eig_ratio;          /* smoothing interval [lmax/ratio, lmax] (default 4)   */
} nsfem_mg_opts;
int nsfem_mg_add_level(nsfem_ctx* ctx, const nsfem_mg_level_desc* level);
/* monolithic scheme: algebraic pressure Laplacian  D_f diag(M_v)^{-1} D_f^T  (and its Galerkin
 * coarsenings) for level `level` of the Schur-complement hierarchy; scalar CSR with a stored
 * diagonal, n = number of P1 nodes of that level (level 0 = fine mesh); singular != 0 when no
 * boundary is open (constants in the kernel: the coarse solve uses the pseudo-inverse) */
int nsfem_mg_set_schur_operator(nsfem_ctx* ctx, int level, int32_t n, const int32_t* rowptr,
                                const int32_t* col, const double* val, int singular);
/* partitioned meshes (additive != 0, call before nsfem_mg_set_schur_operator): the operators are
 * the rank's ADDITIVE parts  D_r W_r D_r^T  (W_r = 1 / M_v,jj on the velocity dofs the rank owns,
 * 0 on ghosts and Dirichlet dofs), ghost rows included, and their Galerkin coarsenings with the
 * rank-local prolongations: their sum over the ranks is the operator.  Products run as forward
 * halo exchange -> local product -> reverse (add) exchange; the global coarsest matrix is the
 * all-reduced dense sum of the coarsest parts (the partition must not carry a replicated tail).
 * `singular` must be the same on every rank (nsfem_comm_allreduce). */
int nsfem_mg_set_schur_mode(nsfem_ctx* ctx, int additive);
/* sum (op = 0) / max (op = 1) over the ranks of `count` (<= 1024) host doubles, in place;
 * single contexts: a no-op */
int nsfem_comm_allreduce(nsfem_ctx* ctx, double* values, int count, int op);
/* partitioned hierarchies: the GLOBAL coarsest mesh (solved redundantly on every rank);
 * offset = global id of this rank's local coarsest node 0 */
int nsfem_mg_set_global_coarse(nsfem_ctx* ctx, int32_t n_vertices, int32_t n_cells,
                               const double* coords, const int32_t* cells, int64_t offset);
/* coarser levels of a REPLICATED hierarchy below the global coarsest mesh (finest first): when
 * that mesh is too large for a dense solve every rank runs the remaining V-cycle redundantly on
 * the all-reduced right-hand side, so the small levels cost no halo exchange */
int nsfem_mg_add_global_level(nsfem_ctx* ctx, const nsfem_mg_level_desc* level);
/* nsfem_mg_set_global_coarse for constrained (periodic) spaces: dofmap [n_cells * (dim + 1)] with
 * n_dofs distinct P1 dofs; on periodic partitions the local coarsest level may wrap around the end
 * of the global numbering (offset + local size > n_dofs) */
int nsfem_mg_set_global_coarse_constrained(nsfem_ctx* ctx, int32_t n_vertices, int32_t n_cells,
                                           const double* coords, const int32_t* cells,
                                           const int32_t* dofmap, int32_t n_dofs, int64_t offset);
int nsfem_mg_finalize(nsfem_ctx* ctx, const nsfem_mg_opts* opts /* may be NULL */);
/* truncated velocity cycle for mass-dominated operators (small time steps): the first P1 level
 * on which  c_v K_ii <= max_ratio * (alpha0/k) M_ii  for every node is solved by Chebyshev
 * iteration to the relative accuracy coarse_tol (a-priori spectral bounds), and the levels below
 * it -- including the dense / global coarse solve and its all-reduce -- leave the cycle.
 * Defaults: max_ratio = 4, coarse_tol = 0.1; max_ratio = 0 disables the truncation.  Re-evaluated whenever the step size or the
 * coefficients change. */
int nsfem_mg_set_truncation(nsfem_ctx* ctx, double max_ratio, double coarse_tol);
/* partitioned meshes: relaxed = 0 (default) exchanges the ghost values before every SpMV of the
 * multigrid preconditioners, so the partitioned cycle IS the serial one; relaxed = 1 exchanges
 * once per smoothing sequence and smooths with frozen ghost values in between (Chebyshev on the
 * rank-local operator around the true residual: block-Jacobi across ranks, still a symmetric
 * preconditioner) -- about a third fewer halo exchanges per step, iteration counts may differ
 * slightly from the serial run.  Krylov operators, residuals and the mass solve stay exact. */
int nsfem_mg_set_halo_mode(nsfem_ctx* ctx, int relaxed);
/* partitioned meshes: enable != 0 runs the halo exchange of every Krylov operator application and
 * smoothing step on the communicator's own HIP stream, concurrently with the row blocks of the
 * product that reference no ghost column; the halo-adjacent row blocks follow after an event wait
 * (SURVEY.md section 8e "overlapped with interior-row SpMV").  Results are bitwise those of the
 * non-overlapped run.  Default: off. */
int nsfem_set_overlap(nsfem_ctx* ctx, int enable);
/* number of overlapped halo exchanges since the last reset */
int nsfem_comm_overlapped(nsfem_ctx* ctx, int64_t* out, int reset);

/* ---- multi-GPU: one process per GPU, each owning a strip of the mesh (new; the reference
 * is serial).  The context is created on the LOCAL mesh (own cell rows + one ghost row);
 * nsfem_set_partition marks the ghost nodes and the contiguous halo ranges; a communicator is
 * attached either over RCCL (production) or in-process (several contexts on one device, one
 * host thread per rank: single-GPU testing of the partitioned algorithm). */
typedef struct {
  int32_t rank, size;
  const uint8_t* p2_ghost;   /* [n_p2] nonzero = ghost (owned by a neighbour) */
  const uint8_t* p1_ghost;   /* [n_p1] */
  nsfem_halo p2_halo, p1_halo;
  int64_t n_p2_global, n_p1_global;
  int32_t periodic;          /* nonzero: the strips / slabs close periodically -- rank size-1 is
                                the lower neighbour of rank 0, halo exchanges wrap around */
} nsfem_partition_desc;
int nsfem_set_partition(nsfem_ctx* ctx, const nsfem_partition_desc* part);
/* Unstructured partitions (recursive coordinate bisection, partition.GraphPartition): a rank has
 * any number of neighbours and its ghost / send nodes are index lists.  For neighbour k (rank
 * neighbour[k]) this rank sends the nodes send_idx[send_ptr[k] .. send_ptr[k+1]) -- owned here,
 * ghost there -- and receives into recv_idx[recv_ptr[k] .. recv_ptr[k+1]); both sides order a
 * pair's list by global node id, so the k-th value sent is the k-th value received.
 * target 0: P2 nodes, 1: P1 nodes of the context (call nsfem_set_partition first, with zeroed
 * nsfem_halo ranges), 2 + l: P1 nodes of multigrid level l (after its nsfem_mg_add_level, ghost
 * flags given there).  Before nsfem_mg_finalize. */
typedef struct {
  int32_t n_neighbours;
  const int32_t* neighbour;  /* [n_neighbours] */
  const int64_t* send_ptr;   /* [n_neighbours + 1] */
  const int32_t* send_idx;
  const int64_t* recv_ptr;   /* [n_neighbours + 1] */
  const int32_t* recv_idx;
} nsfem_halo_lists;
int nsfem_set_halo_lists(nsfem_ctx* ctx, int target, const nsfem_halo_lists* lists);
/* unstructured partitions: global id (in the mesh of nsfem_mg_set_global_coarse, offset 0) of every
 * node of the local coarsest level */
int nsfem_mg_set_global_index(nsfem_ctx* ctx, int32_t n_local, const int32_t* local_to_global);
int nsfem_comm_unique_id(char* id128 /* 128 bytes out */);
int nsfem_comm_attach_rccl(nsfem_ctx* ctx, const char* id128, int rank, int size);
int nsfem_comm_local_create(int size, void** group);
void nsfem_comm_local_destroy(void* group);
int nsfem_comm_attach_local(nsfem_ctx* ctx, void* group, int rank);
/* one PROCESS per rank on ranks that SHARE a device (RCCL refuses two ranks on one GPU): host-staged
 * through the POSIX shared-memory segment `name` ("/..."; rank 0 creates it, slot_bytes per rank,
 * <= 0: 64 MiB).  Functional rehearsal of the process-per-rank launch on a one-GPU box, not a
 * performance transport.  Collective over the ranks (returns when all have attached). */
int nsfem_comm_attach_shm(nsfem_ctx* ctx, const char* name, int rank, int size, int64_t slot_bytes);
/* communication of this rank since the last reset: out = {all-reduce calls, all-reduce payload
 * bytes, halo exchanges, halo bytes sent}; zeros without a communicator */
int nsfem_comm_stats(nsfem_ctx* ctx, int64_t out[4], int reset);

/* ---- fused per-step drivers: replace _solve_time_step
 * (ns_ipcs_solver.py:198-208, ns_bdf_solver.py:102-106) ------------------------ */
int nsfem_default_step_opts(nsfem_step_opts* opts);
int nsfem_step_ipcs(nsfem_ctx* ctx, const nsfem_step_opts* opts, nsfem_step_info* info);
int nsfem_step_bdf(nsfem_ctx* ctx, const nsfem_step_opts* opts, nsfem_step_info* info);
/* One IMEX pressure-correction step (coefficients: nsfem_set_imex).  Diffusion step: ONE CG solve of
 *   (alpha0/k M + gamma0 c_v K) u* = -[ M (alpha1 u1 + alpha2 u2)/k + c_v K (gamma1 u1 + gamma2 u2)
 *                                       + c_c (beta0 N(u1) + beta1 N(u2)) - c_p D^T p_old - c_b M f + traction ]
 * with Dirichlet rows u*_i = g_i (opts->momentum: precond 0 Jacobi, 1 the velocity V-cycle; traction-form viscosity:
 * K is the traction-form stiffness); projection and velocity correction as nsfem_step_ipcs.  c_c N(u1) is kept in
 * NSFEM_CONV_N1, nsfem_advance moves it to NSFEM_CONV_N2 where the next step reads it as c_c N(u2) (recomputed only
 * after NSFEM_U2 / NSFEM_CONV_N2 were set by hand or the convective form / coefficient changed).
 * info->newton_iterations = 0, krylov_iterations_momentum = the CG count.  Rotating frames: NSFEM_ERR_ARG unless
 * nsfem_set_imex_rotation(1) was called.  3D meshes, inexact dictionaries, traction-form viscosity: the generic right-hand-side path. */
int nsfem_step_imex(nsfem_ctx* ctx, const nsfem_step_opts* opts, nsfem_step_info* info);
/* How the right-hand side of the last nsfem_step_imex was formed: out[0] = 1 generic path (products, element kernel,
 * node gather, vector updates), 2 one launch of k_jac_lattice's right-hand-side mode (2D lattice meshes whose stencil
 * dictionaries equal the assembled matrices bit for bit), 0 no step yet; out[1] = one-launch right-hand sides so far,
 * out[2] = generic ones, out[3] = rebuilds of the system matrix.
 * nsfem_imex_rhs (test hook): forms the right-hand side for the current state and coefficients WITHOUT the Dirichlet
 * rows and without touching NSFEM_CONV_N1 / N2: path 1 generic, 2 one-launch (NSFEM_ERR_ARG where it does not apply);
 * rhs and conv_n1 (c_c N(u1), may be null) are host arrays of dim * n_p2 doubles. */
int nsfem_imex_info(nsfem_ctx* ctx, int64_t out[4]);
int nsfem_imex_rhs(nsfem_ctx* ctx, int path, int convective_form, double* rhs, double* conv_n1);
/* Rotating frames in the IMEX calls (nsfem_step_imex, nsfem_imex_rhs, nsfem_step_scalar_imex): opt-in.
 * treatment 0: rotating frames are refused by the IMEX calls (default, as before).
 * treatment 1: Coriolis term extrapolated with the convective term, Euler term in the step-constant vector: the stored
 *   explicit vector is N(u) = c_c conv(u) + V(u) + R(u), R(u) = M (2 c_cor Omega x u) (2D: 2 c_cor omega M (-u_y, u_x)),
 *   formed by the convection element kernel itself (no launch, no pass over memory and no halo exchange of its own;
 *   on uniform 2D lattices inside the one-launch right-hand side), and c_e M (dOmega/dt x x) with the dOmega/dt last
 *   given to nsfem_set_angular_velocity joins g.  Matrix, CG solve, projection and correction are unchanged.
 * omega_n / omega_nm1: angular velocity at t^n / t^(n-1) (1 double in 2D, 3 in 3D);
 * NULL = the value of nsfem_set_angular_velocity (steady frame).  The stored N(u2) is reused only if the 2 c_cor Omega
 * it was formed with equals the one now given for t^(n-1) bit for bit.  With zero rotation the non-rotating kernels
 * run: every output is that of a context that never made the call. */
int nsfem_set_imex_rotation(nsfem_ctx* ctx, int treatment, const double* omega_n, const double* omega_nm1);
int nsfem_imex_rotation_info(nsfem_ctx* ctx, int64_t out[4]);
/* out[0] treatment; out[1] right-hand sides formed with rotation folded in;
   out[2] recomputations of the stored N(u2); out[3] 0 */
/* ---- IMEX transport of a P2 scalar T on the velocity nodes with Boussinesq buoyancy (new; the reference's gravity
 * driven cases prescribe their body force).  diffusivity kappa >= 0; buoyancy: dim entries b (NULL = 0); convective
 * form 0 standard C_ij = int (u . grad phi_j) phi_i, 1 skew-symmetric 1/2 (C - C^T).  With a nonzero b,
 * nsfem_step_imex uses the body force  f_eff = f + T^{n+1} b  (T^{n+1} = NSFEM_T0; formed in a work buffer,
 * NSFEM_BODY_FORCE is never written; body_force_term must be set) exactly where it uses f.  With b = 0 it launches what
 * it launches without a scalar.  NSFEM_ERR_ARG on contexts with a communicator. */
int nsfem_set_scalar(nsfem_ctx* ctx, double diffusivity, const double* buoyancy /* dim, NULL = 0 */,
                     int convective_form);
/* One transport step with alpha, beta, gamma, k of nsfem_set_imex, T1 = NSFEM_T1, T2 = NSFEM_T2, u1 = NSFEM_U1,
 * u2 = NSFEM_U2, q = NSFEM_T_SOURCE (when set):
 *   (alpha0/k M + gamma0 kappa K) T0 = -[ M (alpha1 T1 + alpha2 T2)/k + kappa K (gamma1 T1 + gamma2 T2)
 *                                         + beta0 C(u1) T1 + beta1 C(u2) T2 ] + M q
 * with Dirichlet rows T_i = g_i (field NSFEM_SCALAR; symmetric elimination), solved by Jacobi-preconditioned CG
 * (opts NULL: rtol 1e-12, 20000 iterations).  Call it BEFORE nsfem_step_imex of the same time step: it needs the known
 * levels only, and the flow step reads T0.  beta0 C(u1) T1 is kept in NSFEM_TCONV_1; nsfem_advance(ctx, 0) rotates
 * T2 <- T1 <- T0 and moves it to NSFEM_TCONV_2, where the next step reads it as beta1 C(u2) T2 (scaled by beta1 over
 * the beta0 it was evaluated with; recomputed only after a level or a stored vector was set by hand or the form
 * changed).  The system matrix is rebuilt only when alpha0/k, gamma0 or kappa change.
 * NSFEM_ERR_ARG: no nsfem_set_scalar / nsfem_set_imex, contexts with a communicator, rotating frames. */
int nsfem_step_scalar_imex(nsfem_ctx* ctx, const nsfem_krylov_opts* opts /* may be NULL */,
                           nsfem_solve_info* info /* may be NULL */);
/* Test hook: out_host [n_p2] = weight * C(u) T in the given form (0 / 1) for u = velocity_slot and T = scalar_slot (one
 * of NSFEM_T0 .. NSFEM_T_SOURCE) -- the element kernel plus the per-node sums, no Dirichlet rows; no stored state is
 * touched.  Two calls on the same state return the same bytes. */
int nsfem_scalar_convection(nsfem_ctx* ctx, int velocity_slot, int scalar_slot, int form, double weight,
                            double* out_host);
/* out = {rebuilds of the system matrix, convection launches of the steps, stored-convection reuses, 1 when the products
 * of the last solve ran on the stencil-dictionary copy of the matrix (dictionaries equal to the matrix bit for bit:
 * binary lattice spacings), else 0 (CSR)} */
int nsfem_scalar_info(nsfem_ctx* ctx, int64_t out[4]);
/* ---- subgrid heat flux: eddy diffusivity of a subgrid law in the scalar step (new).  With law 1 (Smagorinsky, C_s),
 * 4 (WALE, C_w) or 5 (Vreman, c) of nsfem_set_viscosity_law, g_ab = d_b u_a, gamma and Delta_K as there, and a
 * turbulent Prandtl number Pr_t > 0:
 *   kappa_x = nu_x / Pr_t          (law 1: kappa_x(gamma, Delta_K) = (C_s Delta_K)^2 gamma / Pr_t)
 *   D(u, T)_i = sum_K sum_q w_q |det J_K| kappa_x(gamma_q, Delta_K) grad T_q . grad phi_i(x_q)
 * by the 7-point (triangles) / 15-point (tetrahedra) rule of the scalar convection kernels; the rule is part of the
 * definition.  kappa K stays in the implicit matrix (no rebuild, the one CG solve); D joins the extrapolated vector,
 * formed inside the convection launch (k_scalar_conv_cell<FORM, PENAL, law>): NSFEM_TCONV_1 = beta0 [C(u1) T1 +
 * D(u1, T1) (+ H)], likewise NSFEM_TCONV_2.  The explicit treatment is stable for every k only while kappa_x <
 * kappa / 3 (SBDF2); otherwise k is bounded by about Delta^2 / kappa_x.
 * prandtl_t = 0 switches the term off (nsfem_step_scalar_imex then launches what it launches without this call), a
 * finite value > 0 switches it on; the same value again changes nothing.  The stored NSFEM_TCONV_2 counts as stale
 * after a change of Pr_t and, while the term is on, of the law or its parameters; it is then formed again with the
 * level's own data.  NSFEM_ERR_ARG: any other value, contexts with a communicator.
 * With the term on, nsfem_step_scalar_imex and nsfem_scalar_explicit refuse (NSFEM_ERR_ARG, state untouched) unless the
 * viscosity law is 1, 4 or 5: law 0 and Carreau are errors, not molecular runs.  nsfem_wall_compute with use_law and
 * one of these laws forms its conductive heat row with kappa + nu_x / Pr_t; with the term off that row keeps its bytes. */
int nsfem_set_scalar_sgs(nsfem_ctx* ctx, double prandtl_t);
/* Test hook: out_host [n_p2] = what ONE launch of the step forms for a level, weight [C(u) T + D(u, T) (+ H(T))] -- D
 * while the term is on, H while a body is thermal (pose of t^(n-1) for scalar_slot NSFEM_T2, of t^n otherwise).  It
 * goes into a Krylov work vector: no slot is written.  With the term off and no thermal body it returns the bytes of
 * nsfem_scalar_convection, which keeps returning C(u) T alone. */
int nsfem_scalar_explicit(nsfem_ctx* ctx, int velocity_slot, int scalar_slot, int form, double weight,
                          double* out_host);
/* out = {1 while the term is on else 0, launches of the SGS != 0 kernels, stored vectors formed again because Pr_t or
 * (with the term on) the law changed, 0} */
int nsfem_scalar_sgs_info(nsfem_ctx* ctx, int64_t out[4]);
/* ---- dynamic subgrid heat flux: the Germano-Lilly eddy diffusivity of the scalar (Moin et al. 1991, Lilly 1992), the
 * partner of viscosity law 8.  kappa_x = c_K Delta_K^2 gamma -- no Pr_t, and C_s^2 is not read -- with the constant
 * C_theta computed on the device from the pair (velocity level, scalar level) the explicit scalar term is evaluated on.
 * With |K| = |det J_K| / dim!, Delta_K^2, gamma = sqrt(2 S:S), the degree-5 rule (7 / 15 points), p1 the P1
 * connectivity, alpha the filter ratio of law 8 and the averaging groups of nsfem_set_dynamic_groups:
 *   1. cell moments m_K[f] = |K| sum_q w_q f(x_q) / sum_q w_q of f = T, T u_a, u_a, d_a T, Delta_K^2 gamma d_a T, S_ab
 *      (a <= b), then |K| and |K| Delta_K^2: 14 doubles per cell in 2D, 21 in 3D.  grad T and G_ab = d_b u_a from the
 *      differences T_k - T_0, u_k - u_0 of the nodal values: a constant T or u gives an exact 0.0.  The set repeats u_a,
 *      S_ab and the volumes of law 8 on purpose (the velocity moments of law 8 may belong to another level)
 *   2. test filter at a vertex v over its cells, ascending: W_v = sum |K|, hat f_v = (sum m_K[f]) / W_v, Delta_v^2 =
 *      (sum |K| Delta_K^2) / W_v, hat gamma_v = sqrt(2 hat S : hat S)
 *   3. P_a = hat(T u_a) - hat T hat u_a, R_a = hat(Delta^2 gamma d_a T) - alpha^2 Delta_v^2 hat gamma hat(d_a T),
 *      PR_v = P . R, RR_v = R . R   (the modelled flux is -C_theta Delta^2 gamma grad T, so P = C_theta R: the sign
 *      convention of law 8's L = C M)
 *   4. per group g: num_g = sum W_v PR_v, den_g = sum W_v RR_v in the fixed order of law 8 from +0.0, ctheta_g =
 *      min(max(num_g / den_g, 0), ctheta_max) where den_g > 0, else 0
 *   5. c_K = the mean over the vertices of K of ctheta_g(v); D(u, T) is that of nsfem_set_scalar_sgs with this kappa_x
 * Three launches (k_dyn_scalar_moments, k_dyn_scalar_vertex, k_dyn_reduce) before every element launch of the term, on
 * that launch's level pair: the constant is a pure function of the pair, NSFEM_TCONV_2 keeps the constant of its own
 * level and a new constant invalidates nothing.  A change of the switch, of ctheta_max, of alpha or of the groups
 * invalidates the stored scalar vector.  enable = 0 switches the term off (ctheta_max is not read); the same setting
 * again changes nothing.  NSFEM_ERR_ARG: enable not 0 or 1, ctheta_max not finite or not > 0, contexts with a
 * communicator, a fixed Pr_t that is on (nsfem_set_scalar_sgs with Pr_t > 0 is likewise refused while this switch is
 * on).  With the switch on, nsfem_step_scalar_imex and nsfem_scalar_explicit refuse (NSFEM_ERR_ARG, state untouched)
 * unless the viscosity law is 8.  nsfem_wall_compute with use_law, law 8, a scalar slot and the switch on forms its
 * conductive row with kappa + c_K Delta_K^2 gamma, the procedure run on the call's velocity and scalar slots; with the
 * switch off that row keeps its bytes.  A context that never calls this allocates and launches nothing new. */
int nsfem_set_scalar_sgs_dynamic(nsfem_ctx* ctx, int enable, double ctheta_max);
/* Output and test hook: runs the procedure on (velocity_slot, scalar_slot).  ctheta_groups [n_groups]; sums
 * [n_groups][2] = num_g, den_g or NULL; vertices [n_p1][3] = W_v, PR_v, RR_v or NULL.  No stored state is touched; two
 * calls on the same state return the same bytes.  NSFEM_ERR_ARG: the switch off, law 8 not set, other slots, contexts
 * with a communicator. */
int nsfem_scalar_dynamic_constant(nsfem_ctx* ctx, int velocity_slot, int scalar_slot, double* ctheta_groups,
                                  double* sums, double* vertices);
/* out [n_cells] = the cell means of kappa_x = c_K Delta_K^2 gamma by the rule of nsfem_viscosity_cells, the constant
 * formed on (velocity_slot, scalar_slot).  Refusals as nsfem_scalar_dynamic_constant. */
int nsfem_scalar_diffusivity_cells(nsfem_ctx* ctx, int velocity_slot, int scalar_slot, double* out);
/* out = {1 while the switch is on else 0, runs of the procedure so far, launches of its three kernels, bytes of its
 * device buffers (0 before the first run)}.  nsfem_scalar_sgs_info keeps its entries: its launch counter counts the
 * element launches of the term, dynamic or not. */
int nsfem_scalar_dynamic_info(nsfem_ctx* ctx, int64_t out[4]);
/* ---- variable viscosity in the IMEX step (new; the reference knows one constant viscosity).  nu = c_v + nu_x(gamma,
 * Delta_K) with gamma = sqrt(2 S:S) = sqrt(1/2 sum_ab (g_ab + g_ba)^2), g_ab = d_b u_a, and Delta_K = |K|^(1/dim),
 * |K| = |det J_K| / dim!.  The constant part c_v K stays in the implicit matrix; the remainder
 *   V(u)_(i,a) = sum_K sum_q w_q |det J_K| nu_x(gamma_q, Delta_K) sum_b (g_ab + g_ba)_q d_b phi_i
 * (7-point Radon rule on triangles, 15-point Keast rule on tetrahedra: the integrand is no polynomial, the rule is part
 * of the definition; always the symmetric form, whatever nsfem_set_viscous_form says) is explicit: nsfem_step_imex then
 * stores and extrapolates N(u) = c_c conv(u) + V(u).  nu_x is used as given (not multiplied by c_v); V has the sign of
 * c_v K u.
 *   law 0  none: nsfem_step_imex launches exactly what it launches without this call (params may be NULL)
 *   law 1  Smagorinsky  nu_x = (C_s Delta_K)^2 gamma                         params = {C_s >= 0}
 *   law 2  Carreau      nu_x = a [ (1 + (lambda gamma)^2)^((n-1)/2) - 1 ]    params = {a finite, lambda >= 0, n > 0};
 *          c_v is the zero-shear viscosity, a = c_v - nu_inf
 *   law 4  WALE (Nicoud & Ducros 1999)                                       params = {C_w finite and >= 0}
 *          S = 1/2 (G + G^T), H = G G (matrix square), Sd = 1/2 (H + H^T) - (tr H / 3) I_3, A = S:S, B = Sd:Sd summed
 *          entry by entry (never as sym(H):sym(H) - tr^2/3, which cancels):
 *          nu_x = (C_w Delta_K)^2 B sqrt(B) / (A^2 sqrt(A) + B sqrt(sqrt(B))), 0 wherever the denominator is not > 0.
 *          The fractional powers are products and sqrt, not pow.  Zero in pure shear, O(y^3) at a wall
 *   law 5  Vreman (2004)                                                     params = {c finite and >= 0}, c ~ 2.5 C_s^2
 *          B_beta = the sum of the squares of all 2x2 minors of G (nine in 3D; one, det G, in 2D) -- by Cauchy-Binet
 *          the second invariant of alpha^T alpha of the paper, non-negative by construction, no clamp, no cancellation:
 *          nu_x = c Delta_K^2 sqrt(B_beta / G:G), 0 where G:G is not > 0.  Zero in pure shear, O(y) at a wall
 * Laws 4 and 5 take the whole tensor G_ab = g_ab = d_b u_a, not gamma alone.  A 2D field counts as the 3D field that
 * does not depend on z: G is the 3x3 tensor with a zero third row and column (so Sd_33 = -tr H / 3 is kept in B).
 * V(u), the cell means, the stored vectors and the explicit treatment are those of laws 1 and 2 with this nu_x.  There
 * is no law 3: ids 3, 6, 7 and 9 and above are unknown.
 *   law 8  dynamic Smagorinsky (Germano et al. 1991, Lilly 1992)              params = {alpha finite and > 1,
 *          nu_x = c_K Delta_K^2 gamma with C_s^2 computed on the device       cs2_max finite and > 0}
 *          from the velocity level the term is evaluated on.  With |K| = |det J_K| / dim! and the degree-5 rule:
 *          1. cell moments m_K[f] = |K| sum_q w_q f(x_q) / sum_q w_q of f = u_a, u_a u_b, S_ab, Delta_K^2 gamma S_ab
 *             (a <= b; G_ab from the differences u_k - u_0 of the nodal values, so a constant field has G = 0 exactly)
 *          2. test filter at a vertex v over its patch of cells, ascending: W_v = sum |K|, hat f_v = (sum m_K[f]) / W_v,
 *             Delta_v^2 = (sum |K| Delta_K^2) / W_v, hat gamma_v = sqrt(2 hat S : hat S)
 *          3. L = hat(u u) - hat u hat u, Ld its deviator, M = 2 (hat(Delta^2 gamma S) - alpha^2 Delta_v^2 hat gamma
 *             hat S), LM_v = Ld : M, MM_v = M : M
 *          4. per averaging group g of vertices (nsfem_set_dynamic_groups; default: all vertices): num_g = sum W_v LM_v,
 *             den_g = sum W_v MM_v in a fixed order, cs2_g = min(max(num_g / den_g, 0), cs2_max) where den_g > 0, else 0
 *          5. c_K = the mean over the vertices of K of cs2_g(v)
 *          alpha is the ratio of the test to the grid filter width (usually 2), cs2_max the clip (0.09 = 0.3^2).  Three
 *          launches (k_dyn_moments, k_dyn_vertex, k_dyn_reduce) before every element launch of this law, on that
 *          launch's velocity level: N(u^(n-1)) keeps the constant of its own level, and a new constant invalidates
 *          nothing.  Setting law 8 resets the groups to the global one.  The subgrid heat flux that goes with this
 *          law is the dynamic one (nsfem_set_scalar_sgs_dynamic); a fixed Pr_t is refused at the step as for law 0
 *          (nsfem_set_scalar_sgs).
 * A change of law or parameters invalidates the stored vectors.  NSFEM_ERR_ARG: unknown law, parameters outside these
 * ranges or not finite, a law other than 0 on contexts with a communicator; nsfem_step_ipcs and nsfem_step_bdf refuse
 * to run while a law other than 0 is set. */
int nsfem_set_viscosity_law(nsfem_ctx* ctx, int law, const double params[4]);
/* Test hook: out_host [dim n_p2] = weight * V(u) for u = velocity_slot (NSFEM_U0, U1, U2 or USTAR) -- the element kernel
 * plus the per-node sums, no Dirichlet rows; no stored state is touched.  Two calls on the same state return the same
 * bytes.  NSFEM_ERR_ARG: no law set, other slots, contexts with a communicator. */
int nsfem_viscosity_residual(nsfem_ctx* ctx, int velocity_slot, double weight, double* out_host);
/* Output: out_host [n_cells] = sum_q w_q nu_x(gamma_q) / sum_q w_q, the cell mean of nu_x for u = velocity_slot */
int nsfem_viscosity_cells(nsfem_ctx* ctx, int velocity_slot, double* out_host);
/* out = {current law, element-kernel launches so far (steps, hook and cell means), stored vectors N(u2) that had to be
 * recomputed with a law set, 0} */
int nsfem_viscosity_info(nsfem_ctx* ctx, int64_t out[4]);
/* Averaging groups of law 8: group_of_vertex [n_p1] with ids in [0, n_groups), n_groups >= 1; vertex ids are P1 dof
 * ids.  Empty groups are allowed (cs2 = 0).  Other groups invalidate the stored vectors; the same groups again change
 * nothing.  NSFEM_ERR_ARG: law 8 not set, n_groups < 1, an id out of range. */
int nsfem_set_dynamic_groups(nsfem_ctx* ctx, int n_groups, const int32_t* group_of_vertex);
/* Output and test hook: runs the procedure of law 8 on u = velocity_slot.  cs2_groups [n_groups]; sums [n_groups][2] =
 * num_g, den_g or NULL; vertices [n_p1][3] = W_v, LM_v, MM_v or NULL.  No stored state is touched; two calls on the same
 * state return the same bytes.  NSFEM_ERR_ARG: law 8 not set, other slots, contexts with a communicator. */
int nsfem_dynamic_constant(nsfem_ctx* ctx, int velocity_slot, double* cs2_groups, double* sums, double* vertices);
/* out = {n_groups (0 before law 8 was ever set), runs of the procedure so far, launches of its three kernels, bytes of
 * its device buffers}.  nsfem_viscosity_info keeps counting the element launches alone. */
int nsfem_dynamic_info(nsfem_ctx* ctx, int64_t out[4]);
/* ---- Lagrangian averaging of law 8 (Meneveau, Lund & Cabot, JFM 319, 1996): LM and MM are averaged along fluid path
 * lines with an exponential memory instead of over groups -- no homogeneous direction is needed.  mode 0: the groups
 * (nsfem_set_dynamic_groups; as before).  mode 1: params = {theta > 0 (1.5), cs2_init >= 0 (0.0256), cs2_floor >= 0
 * (1e-12), 0}.  alpha and cs2_max stay those of law 8.  With k the step size of nsfem_set_imex, vert[v] = {W_v, LM_v,
 * MM_v} of step 3 of law 8 on the level u = u^n, Delta_v^2 = (sum_K |K| Delta_K^2) / W_v over the patch in ascending
 * cell order, p1 / p2 the connectivities and I = (I_LM, I_MM) the state at the vertices of the level before -- all
 * arithmetic without contraction, sums from +0.0 in the order written:
 *   1. displacement   u_v = the velocity at the P2 node p2[c0][i], c0 the first cell of the patch of v and i the local
 *                     index with p1[c0][i] == v;  d = -k u_v
 *   2. upstream cell  barycentric coordinates RELATIVE to v (d = 0 gives exactly lambda_i = 1, the others 0.0): for
 *                     every patch cell c in ascending order, i the local index of v in c: lambda_j = grad(lambda_j) . d
 *                     for j != i, lambda_i = 1 - sum_{j != i} lambda_j (j ascending), m_c = min_j lambda_j.  c* = the
 *                     first cell with the largest m_c.  m_c* < 0 (the point left the patch: CFL > 1, an inflow
 *                     boundary): lambda_j <- max(lambda_j, 0), each divided by their sum.  "The first cell with the
 *                     largest m_c" compares rounded numbers.  Inside the patch a tie is harmless (P1 interpolation
 *                     is continuous across faces).  Outside it is not: the clamped values of tied cells differ, and
 *                     on structured meshes ties are exact by construction -- at an inflow vertex of a box the faces
 *                     of several cells lie in the boundary plane and give the same limiting coordinate, and in 3D the
 *                     far faces of two cells of a Kuhn patch lie in one coordinate plane.  Which of the tied cells
 *                     is taken there depends on the rounding of m_c, and an implementation that rounds otherwise
 *                     (another compiler, a host restatement) may take another one: the result is reproducible for
 *                     one build, the same state gives the same bytes, but it is defined only up to that choice
 *   3. upstream value I_up = sum_j lambda_j I[p1[c*][j]], j ascending, both components
 *   4. relaxation     prod = I_LM_up I_MM_up;  prod > 0: T = theta sqrt(Delta_v^2) / sqrt(sqrt(sqrt(prod))),
 *                     eps = k / (k + T); else eps = 1.  I_MM' = eps MM_v + (1 - eps) I_MM_up,
 *                     I_LM' = max(eps LM_v + (1 - eps) I_LM_up, cs2_floor I_MM').  A vertex of no cell: I' = 0
 *   5. constant       cs2_v = min(max(I_LM' / I_MM', 0), cs2_max) where I_MM' > 0, else 0; c_K and nu_x as in law 8
 *   6. initialisation where no state exists it is formed from the first level evaluated: I_MM = MM_v, I_LM =
 *                     cs2_init MM_v, cs2_v by rule 5
 * Three launches as before (k_dyn_moments, k_dyn_vertex, k_dyn_lagrange in the place of k_dyn_reduce).
 * Time levels: the constant is STATE that lives with the velocity slots.  The context keeps I of level n-1, I' and
 * cs2_cur of level n (valid once formed) and cs2_prev of level n-1.  nsfem_step_imex forms level n once, when it forms
 * N(u1); a second call without nsfem_advance reuses cs2_cur and launches nothing of the procedure.  nsfem_advance
 * rotates (I <- I', cs2_prev <- cs2_cur) and clears the valid flag; without a formed level it drops cs2_prev and keeps
 * I.  nsfem_set_state on NSFEM_U1 clears the valid flag as well (the level changed under its constant).  A stored
 * N(u2) keeps the constant it was formed with; one that has to be formed again (a key that does not serve; always in
 * nsfem_imex_rhs) reads cs2_prev, and without a cs2_prev the initialisation rule is applied to u2 and no state is
 * written.  nsfem_imex_rhs reads cs2_cur where it exists, else applies the rules to the stored I into scratch: it
 * never moves the state.  The hooks -- nsfem_viscosity_residual, nsfem_viscosity_cells, nsfem_wall_compute with
 * use_law, nsfem_dynamic_constant -- read the stored field of the slot's level and never advance or recompute:
 * cs2_prev for NSFEM_U2; for the other slots cs2_cur where formed, else the newest field there is (cs2_prev); a level
 * without any field gets the initialisation rule on the slot's velocity, in scratch.  In mode 1 nsfem_dynamic_constant
 * returns that vertex field in cs2_groups [n_p1], takes sums == NULL only, and vertices are the rows W, LM, MM of the
 * slot's velocity (two launches).
 * A change of mode, theta, cs2_init or cs2_floor resets the state and invalidates the stored vectors; so does setting
 * law 8 (which returns to mode 0 with the global group) and nsfem_set_dynamic_groups (which returns to mode 0).  A
 * change of k alone resets nothing.  NSFEM_ERR_ARG: law 8 not set, unknown mode, parameters out of range or not finite,
 * contexts with a communicator, mode 1 while nsfem_set_scalar_sgs_dynamic is on (which refuses likewise while mode 1 is
 * set: a Lagrangian C_theta is not supported).  A context that never calls this allocates and launches what it did. */
int nsfem_set_dynamic_averaging(nsfem_ctx* ctx, int mode, const double params[4] /* mode 0: may be NULL */);
/* The state for restart files: state [n_p1][4] = I_LM, I_MM, cs2 of level n, cs2 of level n-1; direction 0 get, 1 set.
 * get: a column that does not exist is NaN in every row (I before the first advance, cs2 of level n-1 likewise); the
 * third column is cs2_cur where formed, else a copy of the fourth.  set: columns 0, 1 and 3 count -- each is taken where
 * no entry is NaN and absent where every entry is NaN (I_MM and cs2 >= 0, all finite) --, column 2 is NOT read: level n
 * is formed by the next step.  With the velocity slots and NSFEM_CONV_N2 restored, a run continued in a fresh context
 * forms bit for bit the explicit vectors and the state of the uninterrupted one; u and p are bit for bit the same only
 * if the Krylov solves stop at the same iterations -- they postpone their first convergence check by the iteration count
 * of the solve before, a memory that is no part of any state and that a fresh context does not have.  first_check of
 * nsfem_krylov_opts at or above those counts takes that memory out.  NSFEM_ERR_ARG: mode 1 not set, a column NaN in part, values out of range. */
int nsfem_dynamic_lagrangian_state(nsfem_ctx* ctx, int direction, double* state);
/* Output and test hook: ONE application of rules 1 to 5 to the STORED I (rule 6 while there is none; the upstream
 * pair is then that state) on u = velocity_slot with step size k > 0: out_state [n_p1][2] = I', out_upstream [n_p1][2]
 * = I_up or NULL, out_cs2 [n_p1].  No stored state is touched; two calls on the same state return the same bytes. */
int nsfem_dynamic_lagrangian_advance(nsfem_ctx* ctx, int velocity_slot, double k, double* out_state,
                                     double* out_upstream, double* out_cs2);
/* out = {1 while mode 1 is in force (law 8 set) else 0, 1 while I exists, 1 while level n is formed, 1 while cs2_prev
 * exists}.  nsfem_dynamic_info counts k_dyn_lagrange among its launches and the state among its bytes. */
int nsfem_dynamic_lagrangian_info(nsfem_ctx* ctx, int64_t out[4]);
/* ---- immersed bodies in the IMEX step: Brinkman volume penalisation (new; the reference has body-fitted meshes only).
 * The momentum equation gains (chi / eta) (u - u_s), chi the indicator of the solid, u_s its rigid velocity.  Up to
 * NSFEM_MAX_BODIES bodies, each a primitive with a signed distance d(x), negative inside:
 *   kind 1  ball (disc in 2D)   d = |x - c| - r                                  size = {r > 0}
 *   kind 2  axis-aligned box    d = |max(q, 0)| + min(max_a q_a, 0),  q = |x - c| - h componentwise
 *                                                                               size = half widths h_a > 0
 *   kind 3  half-space          d = (x - c) . n                                  size = unit normal n, | |n| - 1 | <= 1e-12
 * Mask: smoothing eps = 0: chi = 1 where d <= 0, else 0;  eps > 0: chi = 1 for d <= -eps, 0 for d >= eps and
 * 0.5 (1 - d/eps - sin(pi d/eps)/pi) between.  Body velocity u_s(x) = U + W x (x - c); 2D: U + w (-(y - c_y), x - c_x)
 * with w = angular[2].  Where bodies overlap the one with the largest chi counts, the lowest index on ties.
 *   B(u)_(i,a) = (1/eta) sum_K sum_q w_q |det J_K| chi(x_q) (u(x_q) - u_s(x_q))_a phi_i(x_q)
 * with the 7-point Radon rule on triangles and the 15-point Keast rule on tetrahedra (the rules of the viscosity
 * laws: the integrand is no polynomial, the rule is part of the definition), x_q the affine image of the reference
 * point.  eta > 0 is used as given, multiplied by no equation coefficient; B has the sign of c_c conv(u).
 * nsfem_step_imex then stores and extrapolates N(u) = c_c conv(u) + V(u) + R(u) + B(u); the matrices, the CG solve
 * and the one-launch right-hand side stay as they are.  The term is explicit, so k / eta is bounded by the scheme
 * (4/3 SBDF2, 1 CNAB and mCNAB, 0 CNLF for uniform steps); nothing here checks that. */
#define NSFEM_MAX_BODIES 16
typedef struct {
  int32_t kind;
  double centre[3], size[3], velocity[3], angular[3];
} nsfem_body;
/* n = 0 removes the bodies: nothing is launched after that (bodies may be NULL).  A change of the set, eta or the
 * smoothing invalidates the stored vectors; the same set again does not.  NSFEM_ERR_ARG: contexts with a
 * communicator (n > 0), n > NSFEM_MAX_BODIES, unknown kinds, sizes <= 0 or not finite (kind 3: no unit normal), centres
 * or velocities not finite, eta <= 0, smoothing < 0; nsfem_step_ipcs and nsfem_step_bdf refuse to run while bodies
 * are set.  Bodies are not wrapped at periodic sides (see the tracer particles below): no image at the opposite side. */
int nsfem_set_bodies(nsfem_ctx* ctx, int32_t n, const nsfem_body* bodies, double eta, double smoothing);
/* Pose and velocity at t^n of the bodies set: centre, velocity, angular (kind 3: the normal in size as well; other
 * sizes are kept as set).  Call it once per step, before nsfem_step_imex: the pose it replaces becomes that of
 * t^(n-1), which the stored N(u2) was formed with -- that vector is kept, and one that has to be recomputed is formed
 * with that pose again.  NSFEM_ERR_ARG: another count or kind than set. */
int nsfem_move_bodies(nsfem_ctx* ctx, int32_t n, const nsfem_body* bodies);
/* Test hook: out_host [dim n_p2] = weight * B(u) for u = velocity_slot (NSFEM_U0, U1, U2 or USTAR) with the pose of
 * t^n -- the element kernel plus the per-node sums, no Dirichlet rows; no stored state is touched.  Two calls on the
 * same state return the same bytes.  NSFEM_ERR_ARG: no body set, other slots. */
int nsfem_body_residual(nsfem_ctx* ctx, int velocity_slot, double weight, double* out_host);
/* Output: out_host [n_cells] = sum_q w_q chi(x_q) / sum_q w_q, the cell mean of the winning chi */
int nsfem_body_mask_cells(nsfem_ctx* ctx, double* out_host);
/* out [n][1 + dim + ntorque] (ntorque 1 in 2D, 3 in 3D), per body s: the volume int chi_s, the force
 * F_s = (1/eta) int chi_s (u - u_s) the body takes from the fluid, and its torque about c_s; each quadrature point
 * counts for its winning body only, so sum_s F_(s,a) = sum_i B(u)_(i,a).  Bitwise reproducible. */
int nsfem_body_forces(nsfem_ctx* ctx, int velocity_slot, double* out);
/* out = {bodies, element-kernel launches so far (steps, hook and cell means), stored vectors N(u2) that had to be
 * recomputed with bodies set, 0} */
int nsfem_body_info(nsfem_ctx* ctx, int64_t out[4]);

/* ---- wall-stress models in the IMEX step: wall-modelled LES (new; the reference resolves every wall).
 * A modelled boundary facet f of cell K keeps u.n = 0 only (a component-wise Dirichlet row set by the caller); its
 * tangential stress comes from a law of the wall sampled inside the flow.  n = the unit normal out of K.  Rule
 * (x_q, w_q): 3-point Gauss-Legendre on an edge, the symmetric 6-point rule of degree 4 on a face (part of the
 * definition).  Per quadrature point the caller fixes a sample cell, the barycentric coordinates lambda_s of the sample
 * point x_s in it and a wall distance y > 0:
 *   U = u(x_s) - u_w,  u_par = U - (U.n) n,  Re_y = y |u_par| / nu,  r(Re_y) = y+^2 / Re_y, r(0) = 1
 *   W(u)_(i,a) = sum_f sum_q w_q (nu r / y) u_par,a phi_i(x_q)
 * nu = the viscous_term coefficient.  W has the sign of c_c conv(u): nsfem_step_imex stores and extrapolates
 * N(u) = c_c conv(u) + V(u) + B(u) + W(u), W added third; matrices, the CG solve and the one-launch right-hand side
 * stay as they are.
 *   law 1  Werner-Wengle   params = {A, B}: y+ = sqrt(Re_y) for Re_y <= A^(2/(1-B)), else (Re_y / A)^(1/(1+B))
 *   law 2  Reichardt       params = {kappa, C}: u+ = log1p(kappa y+)/kappa + C (-expm1(-y+/11) - (y+/11) exp(-y+/3)),
 *                          y+ u+(y+) = Re_y solved by 5 Newton steps from the law-1 value (A = 8.3, B = 1/7), each step
 *                          floored at a quarter of the iterate; the count is the same at every point
 * facet_cell, facet_local [n_facets] (local = index of the vertex opposite the facet), sample_cell [n_facets][NQ],
 * sample_lambda [n_facets][NQ][dim + 1], sample_y [n_facets][NQ] with NQ = 3 (2D) / 6 (3D) in the order of the rule,
 * wall_velocity [n_facets][dim] or NULL (u_w = 0).  law = 0 or n_facets = 0 switches the term off (the other arguments
 * may be NULL): nothing is launched after that.  A change of the law, its parameters or any array invalidates the
 * stored vectors; the same data again does not.  NSFEM_ERR_ARG: contexts with a communicator, unknown laws, parameters
 * out of range, cells or local indices out of range, y <= 0, non-finite entries; nsfem_step_ipcs and nsfem_step_bdf
 * refuse to run while a model is set.  nu is always a number: nsfem_set_coeffs refuses a viscous coefficient of None. */
int nsfem_set_wall_model(nsfem_ctx* ctx, int law, const double params[4], int32_t n_facets, const int32_t* facet_cell,
                         const int32_t* facet_local, const int32_t* sample_cell, const double* sample_lambda,
                         const double* sample_y, const double* wall_velocity);
/* Test hook: out_host [dim n_p2] = weight * W(u) for u = velocity_slot (NSFEM_U0, U1, U2 or USTAR) -- the facet kernel
 * plus the per-node sums, no Dirichlet rows; no stored state is touched.  Two calls on the same state return the same
 * bytes.  NSFEM_ERR_ARG: no model set, other slots. */
int nsfem_wall_model_residual(nsfem_ctx* ctx, int velocity_slot, double weight, double* out_host);
/* out [n_facets][dim + 4] in input order, per facet: |f|, int tau_w [dim] with tau_w = (nu r / y) u_par, int u_tau with
 * u_tau = nu y+ / y, int y+, max y+ over the facet's quadrature points */
int nsfem_wall_model_facets(nsfem_ctx* ctx, int velocity_slot, double* out);
/* out = {modelled facets, facet-kernel launches so far (steps and hooks), stored vectors N(u2) that had to be
 * recomputed with a model set, the law} */
int nsfem_wall_model_info(nsfem_ctx* ctx, int64_t out[4]);

/* ---- heated immersed bodies: scalar penalisation in the convection kernel of nsfem_step_scalar_imex (new).
 * Each body s of the set given to nsfem_set_bodies gets a thermal flag theta_s in {0, 1} and a temperature T_s; one
 * eta_T > 0 holds for the set.  The scalar equation gains (chi theta / eta_T)(T - T_s), as the vector
 *   H(T)_i = (1/eta_T) sum_K sum_q w_q |det J_K| chi(x_q) theta_win (T(x_q) - T_win) phi_i(x_q)
 * with the rules of B(u) (7-point Radon on triangles, 15-point Keast on tetrahedra), x_q the affine image of the
 * reference point, chi and the winning body as for B(u) (largest chi, lowest index on ties).  A point whose winner has
 * theta = 0 adds nothing: that body stays thermally passive, as every body is without this call.  eta_T is used as
 * given and nothing here checks k / eta_T; H has the sign of C(u) T.
 * The term is explicit and rides with the convection, in ONE element launch: NSFEM_TCONV_1 = beta0 (C(u1) T1 + H^n(T1))
 * with the pose of t^n; a NSFEM_TCONV_2 that has to be formed afresh uses the pose of t^(n-1), as N(u2) does.
 * nsfem_move_bodies invalidates nothing.  The stored scalar vectors count as stale after a change of the flags, the
 * temperatures of thermal bodies or eta_T, and -- while a body is thermal -- of the body set or the smoothing; the
 * same data again is no change.  With no temperatures, or all flags 0, nsfem_step_scalar_imex launches exactly what
 * it launches without this call.
 * n must equal the number of bodies set; n = 0 removes the temperatures (the arrays may be NULL).  A later
 * nsfem_set_bodies with ANOTHER count drops them; one with the same count keeps them, body by index.
 * NSFEM_ERR_ARG: another n, a flag other than 0 / 1, a temperature that is not finite, eta_T <= 0 or not finite, no
 * bodies set. */
int nsfem_set_body_temperatures(nsfem_ctx* ctx, int32_t n, const int32_t* thermal, const double* temperature,
                                double eta_T);
/* test hook: out_host [n_p2] = weight (C(u) T + H(T)) from the fused element launch plus the node sums, u and T the
 * given slots, form 0 standard / 1 skew-symmetric, pose 0 the bodies at t^n, 1 at t^(n-1).  No stored state is
 * touched; two calls return the same bytes.  nsfem_scalar_convection keeps returning the convection alone.
 * NSFEM_ERR_ARG: no bodies or no temperatures set, other slots, form or pose. */
int nsfem_body_scalar_residual(nsfem_ctx* ctx, int velocity_slot, int scalar_slot, int form, double weight,
                               int pose /* 0: t^n, 1: t^(n-1) */, double* out_host /* [n_p2] */);
/* out [n_bodies][3], per body s (pose of t^n): the volume int chi_s, the heat rate
 * Q_s = (1/eta_T) int chi_s theta_s (T - T_s) the body takes from the fluid (0 for passive bodies) and int chi_s T,
 * whose ratio to the volume is the mean temperature inside.  Each quadrature point counts for its winning body only,
 * so sum_s Q_s = sum_i H(T)_i.  Bitwise reproducible.  NSFEM_ERR_ARG: no bodies or no temperatures set, scalar_slot
 * not a scalar slot. */
int nsfem_body_heat(nsfem_ctx* ctx, int scalar_slot, double* out /* [n_bodies][3] */);
/* out = {thermal bodies (flag 1), fused element launches so far (steps and hook), stored scalar vectors recomputed
 * because of a change of the thermal data or the body set, 0} */
int nsfem_body_heat_info(nsfem_ctx* ctx, int64_t out[4]);
/* replaces _advance_solution (ns_solver_base.py:1012-1016, ns_ipcs_solver.py:35-43); scheme 0 with a scalar
 * configured: also T2 <- T1 <- T0 and the stored scalar convection */
int nsfem_advance(nsfem_ctx* ctx, int scheme /* 0 ipcs, 1 bdf */);
/* L2 projection solve  M x = b  (no Dirichlet rows) on the velocity (field 0, both
 * components, b/x node-interleaved) or pressure (field 1) space; replaces the
 * mass-matrix LU inside dlfn.project (ns_solver_base.py:1151,1168).  b = int f phi_i
 * is supplied by the caller. */
int nsfem_mass_solve(nsfem_ctx* ctx, int field, const double* b, double* x,
                     const nsfem_krylov_opts* opts, nsfem_solve_info* info);
/* mean-pressure shift (ns_solver_base.py:1190-1203): p -= (int p / |Omega| - target) */
/* post-processing: (grad phi, grad psi) = rhs on the P1 space, phi = 0 on `dofs` (velocity
 * potential, reference source/ns_problem.py:105-176); pure Neumann data are mean-projected */
int nsfem_poisson_solve(nsfem_ctx* ctx, const double* rhs, int64_t n_dirichlet, const int32_t* dofs,
                        double* x, const nsfem_krylov_opts* opts, nsfem_solve_info* info);
int nsfem_shift_mean_pressure(nsfem_ctx* ctx, double target, double* mean_before);
/* stationary / very large time steps at high cell Peclet numbers: the multigrid V-cycle of the
 * velocity block and the Schur-complement approximation are built for (J + shift M) instead of J
 * ("time-step preconditioner", shift = 1/tau with |u| tau / h = O(1)).  Changes only the
 * preconditioner, never the equations.  shift = 0 (default): off. */
int nsfem_set_preconditioner_shift(nsfem_ctx* ctx, double shift);
/* rotating frame of reference (2D): adds  2 c_coriolis omega (e_z x u, w)  to the momentum
 * residual/Jacobian and  c_euler omega_dot (e_z x x, w)  to its right-hand side
 * (reference source/ns_solver_base.py:173-211); call again when omega changes in time */
int nsfem_set_angular_velocity(nsfem_ctx* ctx, double omega, double omega_dot);
/* 3D meshes: angular velocity VECTOR and its time derivative, cross(Omega, u) / cross(dOmega/dt, x)
 * (ns_solver_base.py:186-190, 207-209) */
int nsfem_set_angular_velocity_3d(nsfem_ctx* ctx, const double omega[3], const double omega_dot[3]);
/* CFL diagnostic of velocity slot `slot` for the step size k: max-norm of the cell-local P2
 * projection of  2 |u| k / h_circumdiameter  (reference source/ns_problem.py:554-587) */
int nsfem_cfl_number(nsfem_ctx* ctx, int slot, double step_size, double* cfl);

/* ---- boundary functionals of the solution: replaces dolfin.assemble(... * ds(subdomain_id)) in the
 * reference's post-processing hooks (demo/dfg_benchmark.py:44-66: drag / lift from the traction
 * -p n + 1/Re sym(grad u) n on the cylinder; demo/gravity_driven_flow.py:66-70: total mass flux).
 * facet_cell[k] = cell adjacent to boundary facet k, facet_local[k] = local index of the vertex
 * opposite to it in that cell (UFC local facet number).  out [dim + 2]:
 *   out[0..dim-1] = int ( -p n + nu (grad u + sym grad u^T) n ) dS   (n = outward unit normal)
 *   out[dim]      = int u . n dS ,   out[dim + 1] = int dS
 * One thread per facet, exact facet quadrature, per-facet values summed in facet order. */
int nsfem_boundary_force(nsfem_ctx* ctx, int velocity_slot, int pressure_slot, int32_t n_facets,
                         const int32_t* facet_cell, const int32_t* facet_local, double nu,
                         double sym, double* out);

/* ---- volume functionals of the solution: replaces dolfin.assemble(... * dx) / dolfin.norm / dolfin.errornorm of a
 * driver's post-processing (kinetic energy and enstrophy of the Taylor-Green runs, |div u| after a projection step,
 * convergence_test/taylor_green_vortex.py:118-119).  With (v, q) = (u, p) of the two slots, or (u - ref_velocity,
 * p - ref_pressure) where a reference field is given (host vectors in the layout of the slots, the difference is
 * formed node by node on the device), out holds the integrals over the cells whose flag is nonzero (NULL: all cells):
 *   out[0] = int 1              out[1] = int v.v            out[2] = int grad v : grad v
 *   out[3] = int |curl v|^2     (2D: scalar curl)           out[4] = int (div v)^2
 *   out[5..7] = int v_x, v_y, v_z   (out[7] = +0.0 in 2D)
 *   out[8] = int q              out[9] = int q^2            out[10] = int |grad q|^2
 * Degree-5 quadrature (7 points / 15-point Keast rule): exact up to rounding on affine cells.  One thread per cell,
 * no atomics, every partial sum folded in a fixed order: two calls on the same state return the same bytes.  The call
 * writes no state slot.  The reference fields and the flags are kept in buffers of the context; the flags are
 * uploaded again only when their CONTENTS differ from the resident copy.
 * Contexts with a communicator: the ghost entries are taken from their owners (halo exchange of copies of the two
 * slots), then ONE all-reduce (sum) of the 11 values follows; every rank calls, and the flags must select each
 * global cell on exactly one rank (partition.py: owned_cell_flags()).
 * NSFEM_ERR_ARG: velocity_slot / pressure_slot not a velocity / pressure slot. */
#define NSFEM_N_FUNCTIONALS 11
int nsfem_volume_functionals(nsfem_ctx* ctx, int velocity_slot, int pressure_slot,
                             const double* ref_velocity /* host, dim*n_p2, or NULL */,
                             const double* ref_pressure /* host, n_p1, or NULL */,
                             const uint8_t* cell_flags  /* host, n_cells, or NULL = all cells */,
                             double out[NSFEM_N_FUNCTIONALS]);

/* ---- point location, point evaluation and passive tracer particles (csrc/points.hip): replaces the point
 * evaluation u(x), p(x) of a dolfin.Function in a driver's post-processing (probe time series, centre-line profiles)
 * and adds particle tracking (new).  One context without a communicator; NSFEM_ERR_ARG on contexts with one (a point
 * can lie in another rank's cells).
 *
 * nsfem_set_point_locator uploads, once, a uniform grid of bins over the mesh (host: point_locator.build_bins):
 * bin of a point = floor((x_d - origin[d]) * inv_h[d]) per direction (x fastest, nbins[d] bins), candidates of bin b =
 * bin_cells[bin_ptr[b] .. bin_ptr[b + 1]) in ascending cell id; all lists are checked against the mesh.
 * nsfem_locate_points: cells[i] = the FIRST candidate of the bin of x[i] whose dim + 1 barycentric coordinates are all
 * >= -1e-12, -1 for a point outside the mesh (a hole, outside the grid of bins, NaN).
 * nsfem_eval_points: value at x[i] of the field in `slot` -- NSFEM_U0/U1/U2/USTAR: velocity, out [n][dim];
 * NSFEM_P/P_OLD/P2_OLD: pressure, out [n]; NSFEM_T0/T1/T2 (after nsfem_set_scalar): P2 scalar, out [n]; any other slot
 * is refused.  cells NULL: the points are located first; a cell of -1 gives NaN.  n = 0 launches nothing.
 * One thread per point, plain loads and stores: two calls on the same input return the same bytes; no state slot is
 * written. */
int nsfem_set_point_locator(nsfem_ctx* ctx, const double* origin, const double* inv_h, const int32_t* nbins,
                            const int32_t* bin_ptr, const int32_t* bin_cells);
int nsfem_locate_points(nsfem_ctx* ctx, int64_t n, const double* x /* [n][dim] */, int32_t* cells);
int nsfem_eval_points(nsfem_ctx* ctx, int slot, int64_t n, const double* x, const int32_t* cells /* NULL: locate */,
                      double* out);
/* Tracer particles, kept in the context: positions [n][dim], a cell that contains each, status (0 moving, 1 left).
 * nsfem_tracers_set locates the points (outside the mesh: status 1) and replaces the cloud.
 * nsfem_tracers_advect: classical RK4 over n_sub equal substeps of dt / n_sub in the velocity blended linearly in
 * time, u(x, theta) = (1 - theta) U[slot_begin] + theta U[slot_end], theta from 0 to 1 over the whole dt (equal slots:
 * frozen field).  Every stage point and the end point of a substep are located, the last known cell first and the
 * bins only when the point is not in it.  A particle one of whose points lies outside the mesh gets status 1, keeps
 * the position it had at the start of that substep and is never moved again.  Periodic sides are not wrapped.
 * Neither are immersed bodies (nsfem_set_bodies, heated or not): their masks are evaluated at the coordinates of the
 * cells, so a body cut by a periodic side has no image at the opposite side -- give the image as a body of its own.
 * NSFEM_ERR_ARG: n_sub < 1, dt not finite, slots that are no velocity slots, no nsfem_tracers_set.
 * nsfem_tracers_info: out = {particles, particles with status 1, advect calls since nsfem_tracers_set, bin-search
 * fallbacks of the last advect call}. */
int nsfem_tracers_set(nsfem_ctx* ctx, int64_t n, const double* x);
int nsfem_tracers_advect(nsfem_ctx* ctx, int slot_begin, int slot_end, double dt, int n_sub);
int nsfem_tracers_get(nsfem_ctx* ctx, double* x, int32_t* cells, uint8_t* status);   /* any may be NULL */
int nsfem_tracers_info(nsfem_ctx* ctx, int64_t out[4]);

/* ---- running flow statistics (csrc/statistics.hip): time averages of the device-resident solution without a copy per
 * step -- mean velocity, Reynolds stresses <u_i' u_j'>, turbulent kinetic energy, mean and variance of the pressure and
 * of the transported scalar, the turbulent flux <u' T'>, and their profiles over groups of nodes.  New; a reference
 * driver would keep numpy sums of get_state copies.
 *
 * Per node the context keeps, in fp64 and one array per quantity, the weighted mean m and the weighted central second
 * moment C of the samples so far (P2 nodes: m_u[dim], C_uu[dim (dim + 1) / 2] in the order xx, xy, yy / xx, xy, xz, yy,
 * yz, zz, and with NSFEM_STATS_SCALAR m_T, C_TT, C_uT[dim]; P1 nodes with NSFEM_STATS_PRESSURE: m_p, C_pp) and on the
 * host the accumulated weight W.  nsfem_stats_sample(.., w) is ONE launch (weighted Welford / Chan update):
 *   d_i = x_i - m_i;   m_i += w / (W + w) d_i;   C_ij += w W / (W + w) d_i d_j   (d taken before the mean moves)
 * The first sample gives m == x bit for bit and C == 0; a field that never changes keeps C == 0 exactly.  Elementwise,
 * no atomics: the same samples give the same bytes.  No state slot is written.
 *
 * nsfem_stats_enable allocates and zeroes the accumulators for `flags` (NSFEM_STATS_VELOCITY is mandatory, the scalar
 * needs nsfem_set_scalar); calling it again starts over; flags = 0 frees everything, the groups included.
 * nsfem_stats_get: one quantity at every node, covariances divided by W; vectors and tensors node-interleaved
 * (MEAN_U, FLUX_UT: [n_p2][dim]; COV_U: [n_p2][dim (dim + 1) / 2]; TKE = trace(C_uu) / (2 W), MEAN_T, VAR_T: [n_p2];
 * MEAN_P, VAR_P: [n_p1]); n = the number of doubles.
 * nsfem_stats_set_groups: groups of nodes of one field (0: P2 nodes, 1: P1 nodes) as a CSR -- nodes and weights of
 * group g at [group_ptr[g], group_ptr[g + 1]); every group has an entry, every weight is finite and > 0, a node may
 * appear in any number of groups.  nsfem_stats_profiles reduces the node statistics over each group, with
 * A = sum_n a_n, to the pooled mean and covariance (within-node plus between-node part)
 *   m_g = sum_n a_n m_n / A      C_g = sum_n a_n (C_n / W) / A + sum_n a_n (m_n - m_g)(m_n - m_g)^T / A
 * out [n_groups][n_q], the columns in the order of the accumulators above: P2 n_q = dim + dim (dim + 1) / 2 (m_u, C_uu)
 * and with the scalar 2 + dim more (m_T, C_TT, C_uT); P1 n_q = 2 (m_p, C_pp).  One workgroup per group, every sum in a
 * fixed order, no atomics.
 * nsfem_stats_info: out = {samples, flags, bytes of the accumulators, update launches}; nsfem_stats_weight: W.
 * NSFEM_ERR_ARG (the accumulators keep their bytes): weight not finite or <= 0, a slot of the wrong kind, the scalar
 * without nsfem_set_scalar, a quantity that is not enabled, get / profiles before the first sample or with the wrong n,
 * group lists with an index out of range, contexts on a partitioned mesh (profiles would need a merge across ranks). */
enum nsfem_stats_flags { NSFEM_STATS_VELOCITY = 1, NSFEM_STATS_PRESSURE = 2, NSFEM_STATS_SCALAR = 4 };
enum nsfem_stats_quantity {
  NSFEM_STATS_MEAN_U = 0, NSFEM_STATS_COV_U = 1, NSFEM_STATS_TKE = 2, NSFEM_STATS_MEAN_P = 3, NSFEM_STATS_VAR_P = 4,
  NSFEM_STATS_MEAN_T = 5, NSFEM_STATS_VAR_T = 6, NSFEM_STATS_FLUX_UT = 7
};
int nsfem_stats_enable(nsfem_ctx* ctx, uint32_t flags);
int nsfem_stats_sample(nsfem_ctx* ctx, int velocity_slot, int pressure_slot /* -1: none */,
                       int scalar_slot /* -1: none */, double weight);
int nsfem_stats_get(nsfem_ctx* ctx, int quantity, double* host, int64_t n);
int nsfem_stats_set_groups(nsfem_ctx* ctx, int field /* 0 P2, 1 P1 */, int32_t n_groups, const int32_t* group_ptr,
                           const int32_t* nodes, const double* weights);
int nsfem_stats_profiles(nsfem_ctx* ctx, int field, double* out /* [n_groups][n_q] */, int64_t n);
int nsfem_stats_info(nsfem_ctx* ctx, int64_t out[4]);
int nsfem_stats_weight(nsfem_ctx* ctx, double* W);

/* ---- gradient-derived fields of the current solution (csrc/derived.hip): vorticity, divergence, shear rate,
 * Q-criterion, velocity gradient, pressure gradient and the gradient of the transported scalar, from ONE element-kernel
 * launch whatever the mask -- replaces the get_state copy plus numpy einsums of ProblemBase._compute_vorticity /
 * _compute_pressure_gradient / _cell_gradients (which stay as the host yardstick) and adds what they do not have.
 *
 * With G_ab = d_b u_a at a point of a cell (linear on the cell for the P2 velocity):
 *   NSFEM_DERIVED_VORTICITY          1 (2D) / 3 (3D)  2D: G_10 - G_01;  3D: (G_21 - G_12, G_02 - G_20, G_10 - G_01)
 *   NSFEM_DERIVED_DIVERGENCE         1                tr G
 *   NSFEM_DERIVED_SHEAR_RATE         1                gamma = sqrt(2 S:S), S = (G + G^T) / 2 (the gamma of the
 *                                                     viscosity laws, nsfem_set_viscosity_law)
 *   NSFEM_DERIVED_Q_CRITERION        1                Q = (|W|_F^2 - |S|_F^2) / 2 = -1/2 G_ab G_ba, W = (G - G^T) / 2
 *   NSFEM_DERIVED_VELOCITY_GRADIENT  dim^2            G_ab, row-major in (a, b)
 *   NSFEM_DERIVED_PRESSURE_GRADIENT  dim              constant on a cell
 *   NSFEM_DERIVED_SCALAR_GRADIENT    dim              gradient of the P2 scalar of nsfem_set_scalar
 * Centres:
 *   NSFEM_DERIVED_CELL    [n_cells][ncomp]           cell means (1/|K|) int_K q by the degree-5 rule (7 / 15 points) of
 *                                                    nsfem_viscosity_cells: exact up to rounding except SHEAR_RATE,
 *                                                    for which the rule is part of the definition
 *   NSFEM_DERIVED_VERTEX  [n_cells][dim + 1][ncomp]  q at every vertex of every cell (DG1 data; exact representation
 *                                                    of the quantities linear in G)
 *   NSFEM_DERIVED_NODE    [n_p2][ncomp]              volume-weighted recovery at the P2 nodes,
 *                                                    sum_{K contains n} |K| q(G_K(x_n)) / sum_{K contains n} |K|
 *                                                    with G_K(x_n) the cell's own gradient at the node's position in K
 *                                                    (a vertex or an edge midpoint); nonlinear quantities are formed
 *                                                    before averaging, the pressure gradient averages the cell
 *                                                    constants; identified nodes of a periodic mesh sum over all
 *                                                    their cells
 * out_host is [entities][total components], the requested quantities in ascending id order within a row; out_len =
 * the number of doubles (checked).  quantity_mask = the OR of 1 << NSFEM_DERIVED_<quantity>.  pressure_slot /
 * scalar_slot may be -1 when the mask does not need them.
 * NODE: the element kernel stores |K| q and |K| node-sorted (the index of the assembly kernels) into a buffer of the
 * context's own -- allocated at the first call, grown when a call needs more, never the buffers of the step --, one
 * second launch sums the run of every node in ascending cell order and divides.  No atomics: the same state gives the
 * same bytes, and a quantity has the same bytes whatever else is in the mask.  No state slot is written.
 * nsfem_derived_components: components of one quantity on this context's mesh.
 * nsfem_derived_info: out = {element launches, gather launches, calls, bytes of the private buffer}.
 * NSFEM_ERR_ARG, with a message and nothing launched: an unknown quantity bit or centre, an empty mask, a slot of the
 * wrong kind, SCALAR_GRADIENT without nsfem_set_scalar, a wrong out_len, a context with a communicator.  Partitioned
 * meshes are out of scope on purpose: the recovery at a node on a partition boundary needs the cells of other
 * ranks. */
enum nsfem_derived_quantity {
  NSFEM_DERIVED_VORTICITY = 0, NSFEM_DERIVED_DIVERGENCE = 1, NSFEM_DERIVED_SHEAR_RATE = 2,
  NSFEM_DERIVED_Q_CRITERION = 3, NSFEM_DERIVED_VELOCITY_GRADIENT = 4, NSFEM_DERIVED_PRESSURE_GRADIENT = 5,
  NSFEM_DERIVED_SCALAR_GRADIENT = 6
};
#define NSFEM_N_DERIVED 7
enum nsfem_derived_center { NSFEM_DERIVED_CELL = 0, NSFEM_DERIVED_VERTEX = 1, NSFEM_DERIVED_NODE = 2 };
int nsfem_derived_components(nsfem_ctx* ctx, int quantity, int* ncomp);
int nsfem_derived_fields(nsfem_ctx* ctx, int velocity_slot, int pressure_slot, int scalar_slot,
                         unsigned quantity_mask, int center, double* out_host, int64_t out_len);
int nsfem_derived_info(nsfem_ctx* ctx, int64_t out[4]);

/* ---- energy spectra on box lattices (csrc/spectrum.hip, the axis passes through the tile body of csrc/fastdiag.hip):
 * a separable linear transform of a nodal field on its lattice followed by binned sums of squares -- the wavenumber
 * spectrum E(k) of a periodic box, the one-dimensional spectra E(k_x; y) of a channel.  Replaces get_state plus
 * numpy.fft.fftn plus a Python binning loop per sample; new, the reference has no spectra.
 *
 * On a box mesh the P2 nodes (vertices and edge midpoints) occupy every point of the half-spacing lattice exactly once,
 * the P1 nodes every point of the vertex lattice: the nodal values are a regular sample, n_a = 2 cells_a (P1: cells_a)
 * points along a periodic axis and one more along a walled one.  The device part is generic; what a bin means (a
 * shell, a (y, |k_x|) pair) is decided on the host (energy_spectrum.py).
 *
 * nsfem_spectrum_set: the plan of this context (one per context; setting again replaces it, n[0] = 0 frees it).  n: the
 * lattice points per axis, x fastest, n[2] = 1 in 2D.  Fx, Fy, Fz: row-major [n_a][n_a], row = basis function; NULL:
 * the axis is not transformed.  node_of_point [n0 n1 n2]: the node that carries each lattice point.  The bins are a CSR
 * of lattice points: bin b holds bin_points[bin_ptr[b] .. bin_ptr[b + 1]); bins may overlap, leave points out or be
 * empty.  Validated on the host before anything is uploaded -- every node_of_point inside the P2 node count (the
 * largest one is kept: nsfem_spectrum_compute refuses a slot whose field has fewer nodes), every bin point inside the
 * lattice, bin_ptr starting at 0 and not decreasing, the matrices finite -- so no kernel can index out of range.  The
 * plan owns two work arrays of n0 n1 n2 doubles (components are processed one after the other), the chunk partials
 * and the result; nothing else is allocated later.
 *
 * nsfem_spectrum_compute: out [n_bins][ncomp] = sum over the points of the bin of c^2, c the transformed values of
 * one component, RAW (normalisation is the host's business).  slot: any slot of nodal values -- NSFEM_U0 .. NSFEM_USTAR
 * and NSFEM_BODY_FORCE give ncomp = dim (node-interleaved), NSFEM_T0 .. NSFEM_T_SOURCE and the pressure slots 1.  Per
 * component: k_spec_pack (w[point] = state[node_of_point[point] ncomp + c], coalesced writes, gathered reads), one
 * launch per transformed axis (x: a plain GEMM over [n2 n1] x n0, y: the batched plane product, z: a plain GEMM over
 * n2 x [n1 n0]), k_spec_bin (one workgroup of 256 threads per chunk of at most 2048 CSR entries, chunks never straddle
 * a bin: thread t adds the squares of the entries t, t + 256, ... in ascending order, then a fixed tree in LDS) and
 * k_spec_bin_sum (one thread per bin adds its chunk partials in ascending order; +0.0 for an empty bin).  No atomics:
 * the same state gives the same bytes, whatever ran in between.  No state slot and no buffer of the step is written.
 *
 * With the real orthonormal Fourier basis of n points (row 0 constant, then cos / sin pairs scaled sqrt(2 / n), then
 * the alternating row when n is even) the squares of the cos and sin coefficients of wavenumber k add up to
 * n (|u^_k|^2 + |u^_-k|^2), u^ the normalised DFT; in d dimensions the sum over the 2^d cos / sin products is the
 * energy of all sign combinations of (k_x, k_y, k_z).  No complex arithmetic is needed.
 *
 * nsfem_spectrum_info: out = {transform launches, bin launches, calls, bytes of the plan}.
 * NSFEM_ERR_ARG, with a message, nothing launched and the plan and counters unchanged: a context with a communicator
 * (partitioned meshes are out of scope, as for the statistics and the derived fields), a non-positive n, a failed
 * validation, a slot of no nodal kind or without storage, a wrong out_len, compute or info before set. */
int nsfem_spectrum_set(nsfem_ctx* ctx, const int32_t n[3], const double* Fx, const double* Fy, const double* Fz,
                       const int32_t* node_of_point, int32_t n_bins, const int32_t* bin_ptr,
                       const int32_t* bin_points);
int nsfem_spectrum_compute(nsfem_ctx* ctx, int slot, double* out /* [n_bins][ncomp] */, int64_t out_len);
int nsfem_spectrum_info(nsfem_ctx* ctx, int64_t out[4]);

/* ---- wall quantities (csrc/wall.hip): everything evaluated on a set of facets -- measure, pressure force, viscous
 * force, mass flux, mean temperature, conductive heat flux, torque -- per facet and summed per group of facets, from a
 * facet set that stays resident on the device.  The facet side of the device post-processing; nsfem_boundary_force
 * stays as the one-shot call (one summed traction of one list, lists uploaded at every call).
 *
 * nsfem_wall_set_facets: n_facets facets, facet f = the facet of cell facet_cell[f] opposite its local vertex
 * facet_local[f], in group facet_group[f] (NULL: all in group 0) of n_groups >= 1 groups.  Every cell, local index and
 * group id is validated on the host, the facets are sorted by group (stable), and the lists and the group offsets are
 * uploaded ONCE (the permutation back to the input order stays on the host, where facet rows are un-permuted); an
 * earlier set is replaced.  n_facets = 0 is valid.  Facets need not lie on the
 * boundary: an interior facet gives the one-sided trace from facet_cell.
 *
 * nsfem_wall_compute: with n = the unit normal pointing out of facet_cell, G_ab = d_b u_a, gamma = sqrt(2 S:S) and
 * Delta_K of nsfem_set_viscosity_law, a row of NW = 9 (2D) / 13 (3D) doubles per facet, in this order:
 *   1          |f|
 *   dim        int -p n
 *   dim        int [ nu (G + sym G^T) + nu_x(gamma, Delta_K) (G + G^T) ] n     nu_x = 0 unless opts->use_law != 0 and a
 *                                                                             law is set
 *   1          int u.n
 *   1          int T                                                           +0.0 with scalar_slot = -1
 *   1          int -kappa grad T . n   (conductive heat LEAVING the fluid)     +0.0 with scalar_slot = -1
 *   1 / 3      int (x - x0) x t, t the sum of the two traction integrands, x0 = opts->origin (2D: the z component)
 * Facet rules: 2-point Gauss on edges, the 3 edge midpoints on faces -- exact for every integrand without a law; with
 * a law the rule is part of the definition (as for nsfem_viscosity_cells).  out_groups [n_groups][NW]: the sums of
 * the rows of every group; out_facets NULL or [n_facets][NW]: the rows in the INPUT order of nsfem_wall_set_facets.
 * ONE launch of k_wall_facets<DIM, LAW> (one thread per facet) and ONE of k_wall_reduce<NW> (one workgroup of 256
 * threads per group: thread t adds the rows t, t + 256, ... of its group in ascending resident order from +0.0, then
 * a xor-shuffle tree within every wave, then the four wave sums in order), one copy of n_groups * NW doubles, one more
 * of the rows only when out_facets is given.  No atomics: the same state gives the same bytes and the sums of a group
 * do not depend on which other groups exist; an empty group gives +0.0.  No allocation after nsfem_wall_set_facets,
 * no state slot and no buffer of the step written.
 * nsfem_wall_components: NW of this context's mesh.
 * nsfem_wall_info: out = {facets, groups, compute calls, facet-set uploads}.
 * NSFEM_ERR_ARG, with a message, nothing launched and the counters unchanged: no facet set; null opts or out_groups;
 * slots of the wrong kind; a scalar slot without nsfem_set_scalar or one that was never set or stepped (no storage yet:
 * nothing is allocated here); non-finite nu, sym, kappa or origin; a cell, local
 * index or group out of range; n_groups < 1; a context with a communicator (partitioned meshes keep
 * nsfem_boundary_force: out of scope here on purpose). */
typedef struct {
  double nu, sym, kappa, origin[3];
  int use_law;
} nsfem_wall_opts;
int nsfem_wall_set_facets(nsfem_ctx* ctx, int32_t n_facets, const int32_t* facet_cell, const int32_t* facet_local,
                          const int32_t* facet_group /* NULL: all 0 */, int32_t n_groups);
int nsfem_wall_compute(nsfem_ctx* ctx, int velocity_slot, int pressure_slot, int scalar_slot /* -1: none */,
                       const nsfem_wall_opts* opts, double* out_groups /* [n_groups][NW] */,
                       double* out_facets /* NULL or [n_facets][NW], INPUT order */);
int nsfem_wall_components(nsfem_ctx* ctx, int* nw);
int nsfem_wall_info(nsfem_ctx* ctx, int64_t out[4]);

/* ---- measurement hooks (bench.py): time `reps` launches of the dominant SpMV
 * with HIP events on the context's stream; ms per launch returned ------------- */
/* in-situ HIP-event timing of the finest-level smoothing launches of the velocity multigrid
 * (the dominant kernel of a time step), one event pair around each run of consecutive launches
 * of a smoothing sequence: enable != 0 starts sampling, enable == 0 stops and
 * reports average launch duration [ms], number of launches and algorithmic bytes per launch */
int nsfem_profile_smoother(nsfem_ctx* ctx, int enable, double* avg_ms, int64_t* launches,
                           int64_t* algorithmic_bytes);
/* detail of the window nsfem_profile_smoother just closed: out = {launches, smoothing steps they
 * ran (the multi-step lattice kernel runs up to 4 per launch), algorithmic bytes they moved in total,
 * 1 when the lattice kernel ran them} */
int nsfem_profile_smoother_detail(nsfem_ctx* ctx, int64_t out[4]);
int nsfem_time_spmv(nsfem_ctx* ctx, int op, int reps, double* ms_per_launch,
                    int64_t* algorithmic_bytes);
/* which finest-level smoothing kernel of the velocity multigrid runs: out = {kind (0 CSR-stream,
 * 1 SELL-64, 2 stencil dictionary), dictionary entries, longest row (negative: the dictionary
 * reproduces the matrix bit for bit and every product uses it), algorithmic bytes a CSR
 * stream of the same operator moves per smoothing launch}.  The stencil dictionary (lattice
 * meshes: rows with equal column offsets and values to 2^-40 of the largest entry share one entry;
 * a launch reads one byte per row instead of 12 bytes per nonzero) is used by smoothing steps and
 * Newton-Jacobian products only -- never by a residual or a linear operator whose solution is
 * returned; NSFEM_DICT=0 disables it. */
int nsfem_smoother_info(nsfem_ctx* ctx, int64_t out[4]);
/* Test hook: z = M^-1 r, one cycle of a multigrid preconditioner on host vectors (which: 0 = pressure Poisson
   hierarchy, 1 = velocity hierarchy); nsfem_mg_info: out = {reserved (always 0), reserved (always 0), levels in use,
   reserved (always 0)}; which = 2 / 3: the multi-step lattice kernel on the Poisson / velocity hierarchy: out =
   {levels whose smoothing sequences run in it (partitioned strips: relaxed halo mode only), its launches so far,
   levels in use, ghost lattice lines of the finest level as bottom * 256 + top}.  New functionality (the reference has no preconditioner: sparse LU,
   source/ns_ipcs_solver.py:171,205). */
int nsfem_mg_apply(nsfem_ctx* ctx, int which, const double* r, double* z);   /* which = 2: fast diagonalisation */
/* which = 3 / 4 (single contexts): the two pressure hierarchies of the monolithic block preconditioner, refreshed as
   nsfem_step_bdf refreshes them -- 3 the Schur hierarchy (Dirichlet set NSFEM_PRESSURE_PRECOND; geometric or
   nsfem_mg_set_schur_operator levels), 4 the pressure mass smoother (four Chebyshev-Jacobi steps).  nsfem_mg_info:
   which = 4 / 5 the record of which = 0 / 1 for these two, which = 6 / 7 the record of which = 2 / 3.
   Test hook nsfem_monolithic_apply (single contexts), host vectors of nvel + npre entries: what = 0: y = the mixed
   operator [[J, -c_p D^T], [-c_p D, 0]] of nsfem_step_bdf's linear solve applied to x, linearised about U0 with the
   context's convective form and Picard flag, identity rows on Dirichlet dofs; what = 1: y = the block-triangular
   Cahouet-Chabard preconditioner applied to x.  matrix_free != 0: the velocity Jacobian is applied matrix-free.
   Prepares what that linear solve prepares; writes no state slot. */
int nsfem_monolithic_apply(nsfem_ctx* ctx, int what, int matrix_free, const double* x, double* y);
/* Direct solver of the projection step on tensor-product lattices (replaces the sparse LU of
   source/ns_ipcs_solver.py:160-171 where it applies): Vx [W x W], Vy [H x H] generalised eigenvectors of the 1D
   stiffness / lumped-mass pairs of the two directions (row-major, V^T W V = I, zero rows on Dirichlet sides),
   inv [H x W] = 1 / (lambda_y,j + lambda_x,i) (0: singular mode, Dirichlet slots).  The P1 space must be the W x H
   lattice in lexicographic numbering.  nsfem_krylov_opts.precond = 3 of the projection step then runs
   x += A^+ (b - A x) (four dense products on the matrix cores) and checks the residual.  Host side:
   poisson_fd.factors(). */
int nsfem_poisson_set_fast_diag(nsfem_ctx* ctx, int32_t W, int32_t H, const double* Vx, const double* Vy,
                                const double* inv);
/* The same on a partitioned strip (nsfem_set_partition): the factors of the GLOBAL W x H lattice; the context's P1
   space is the lattice lines first_line ... first_line + n_p1 / W - 1, ghost lines included.  The projection step of
   nsfem_step_ipcs (precond = 3, no pressure Dirichlet dofs) then costs ONE all-reduce of W x H doubles instead of the
   halo exchanges and dot-product reductions of a multigrid-CG solve, and returns the pressure with valid ghost rows. */
int nsfem_poisson_set_fast_diag_rows(nsfem_ctx* ctx, int32_t W, int32_t H, int32_t first_line, const double* Vx,
                                     const double* Vy, const double* inv);
/* The same on 3D box lattices (fem_mesh.box_mesh, six Kuhn tetrahedra per cube, any line spacing, periodic directions
   allowed): Vx [Nx x Nx], Vy [Ny x Ny], Vz [Nz x Nz] the generalised eigenvectors of the three directions (row-major),
   inv [Nz x Ny x Nx] = 1 / (lambda_z,k + lambda_y,j + lambda_x,i).  The P1 space must be the Nz x Ny x Nx lattice in
   lexicographic numbering (x fastest).  T, the tensor sum of the 1D stiffness / lumped-mass pairs, is the P1 stiffness
   matrix itself when exact != 0 (uniform lines, every box edge between two non-periodic faces next to a Dirichlet
   face): precond = 3 then solves the projection step directly (one pass plus the residual check); with exact == 0 it
   runs CG preconditioned by T^+ (mesh-independent iteration counts).  Six dense mode products on the matrix cores
   (csrc/fastdiag.hip).  Refused on partitioned contexts.  Replaces 2D factors set before, and vice versa.  Host side:
   poisson_fd.factors_3d(). */
int nsfem_poisson_set_fast_diag_3d(nsfem_ctx* ctx, int32_t Nx, int32_t Ny, int32_t Nz, const double* Vx,
                                   const double* Vy, const double* Vz, const double* inv, int32_t exact);
/* The same on partitioned slabs (nsfem_set_partition with a communicator): the factors of the GLOBAL Nz x Ny x Nx
   lattice; local P1 plane i is global plane (first_plane + i) mod Nz (ghost planes included; periodic partitions
   only may wrap around), and the owned dofs (the P1 ghost flags) are one contiguous run of whole planes.  precond = 3
   of the projection step (no pressure Dirichlet dofs) then costs ONE all-reduce of Nz x Ny x Nx doubles -- a direct
   solve for exact factors, CG preconditioned by T^+ otherwise -- and returns the pressure with valid ghost planes.
   NSFEM_ERR_ARG: no partition / communicator, n_p1 not a multiple of Nx Ny, Nx Ny Nz != the global P1 count, owned
   dofs not a run of whole planes, wrapping planes on a non-periodic partition.  Replaces other factors. */
int nsfem_poisson_set_fast_diag_3d_planes(nsfem_ctx* ctx, int32_t Nx, int32_t Ny, int32_t Nz, int32_t first_plane,
                                          const double* Vx, const double* Vy, const double* Vz, const double* inv,
                                          int32_t exact);
/* out = {Nx, Ny, Nz, exact, applications of T^+ issued by the host (CG iterations replayed from a captured graph apply
   it without the host), projection solves that ran with the 3D factors}; zeros when none are set.
   nsfem_mg_apply(which = 2) applies z = T^+ r when 3D factors are set (slab factors: a collective). */
int nsfem_poisson_fast_diag_3d_info(nsfem_ctx* ctx, int64_t out[6]);
int nsfem_mg_info(nsfem_ctx* ctx, int which, int64_t out[4]);
/* in-situ HIP-event timing of the matrix-free convection action of the velocity Jacobian inside
 * the Newton-Krylov solves (element kernel k_conv_cell / k3_conv_cell + node gather = the
 * per-iteration "assembly" of the fused step drivers; replaces the dolfin assemble(J) call of
 * ns_ipcs_solver.py:136-147 / ns_bdf_solver.py:88-100): enable != 0 starts sampling, enable == 0
 * stops and reports the average duration [ms] of one application, the number of applications and
 * the algorithmic bytes of one application (SURVEY.md section 8d formula).  One GPU, triangles, lattice
 * mesh: the per-node sums run inside the L-product launch, the event pair then brackets the element
 * kernel alone -- flagged by a NEGATIVE byte count (minus the element kernel's own bytes).  Lattice meshes in
 * rectangle_mesh numbering (nsfem_jacobian_info path 2): the pair brackets k_jac_lattice, i.e. the WHOLE Jacobian
 * action  L x + c_c [d conv(u)/du] x  in one launch; the byte count is nsfem_jacobian_info's out[2] */
int nsfem_profile_convection(nsfem_ctx* ctx, int enable, double* avg_ms, int64_t* applications,
                             int64_t* algorithmic_bytes);
/* How the matrix-free action of the velocity Jacobian (NSFEM_OP_MOMENTUM_JAC_MF; the operator of the Newton-Krylov
 * solves in nsfem_step_ipcs / nsfem_step_bdf, replacing the assembled J of ns_ipcs_solver.py:136-147) runs on this
 * context: out[0] = 0  L product, element kernel, node gather (three launches: partitioned meshes, tetrahedra,
 * unstructured meshes); 1  element kernel, then the dictionary product of L sums its node-sorted element vectors;
 * 2  k_jac_lattice -- one launch (2D lattice meshes in rectangle_mesh numbering on one GPU, gradient-form viscosity,
 * no rotating frame; NSFEM_JAC_LATTICE=0 disables it).  out[1] = applications through k_jac_lattice so far,
 * out[2] = its algorithmic bytes per application (u, x read, y written: 48 B per P2 node; 3 B per node of
 * dictionary ids and masks; 48 B per cell of vertex coordinates), out[3] = the k_jac_lattice variant (0 the
 * round-4 kernel, NSFEM_JL_KERNEL=0; 1 one cell type per wave and node sums by gather; 2 the same with the physical
 * gradients of a uniform lattice from tables). */
int nsfem_jacobian_info(nsfem_ctx* ctx, int64_t out[4]);
/* Launches so far of the fused step frame of the pressure-correction steps (NSFEM_STEP_FUSED, default on, read when
 * the context is created; 0 keeps one launch per vector pass): out[0] = k_spmv_dict_pair in the begin step
 * (M x + c D^T p_old), out[1] = k_spmv_dict_pair in the correction assembly, out[2] = k_correction_finish,
 * out[3] = projection checks whose launch also stored p = p_old + z.  Each stays 0 where its path does not apply
 * (partitioned contexts, no exact stencil dictionaries, 3D, optional right-hand-side terms, other solvers). */
int nsfem_step_frame_info(nsfem_ctx* ctx, int64_t out[4]);
/* Residual launches so far of nsfem_step_ipcs that carried the frame of its Newton iteration (NSFEM_NEWTON_FUSED,
 * default on, read when the context is created; 0 keeps the update u* -= dx, the Dirichlet rows of the residual and
 * its norm as launches of their own): out[0] = launches of k_jac_lattice that also set the Dirichlet rows and left
 * the sum of squares per tile, out[1] = those among them that first applied the pending update.  Both stay 0 where
 * the path does not apply (partitioned contexts, no exact stencil dictionary, 3D, NSFEM_JAC_LATTICE=0, NSFEM_GRAPHS=1,
 * every caller but nsfem_step_ipcs).  The update is written to a second buffer that then takes the place of the
 * NSFEM_USTAR slot: a pointer from nsfem_state_devptr(NSFEM_USTAR) is good until the next step call only. */
int nsfem_newton_frame_info(nsfem_ctx* ctx, int64_t out[2]);
/* Test hook: *bad_cells = the number of cells whose basis gradients and weights, evaluated per cell as the element
 * kernels do, differ in any bit from the tables k_jac_lattice reads on a uniform lattice; -1 when there are none. */
int nsfem_jacobian_table_check(nsfem_ctx* ctx, int64_t* bad_cells);
/* extreme eigenvalues of diag(M_e)^-1 M_e of the P2 element mass matrix (host arithmetic only) */
int nsfem_p2_mass_bounds(int dim, double* lmin, double* lmax);
int nsfem_synchronize(nsfem_ctx* ctx);

#ifdef __cplusplus
}
#endif
#endif /* NSFEM_H */
