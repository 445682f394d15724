// C ABI of libnsfem_hip.so (declared in include/nsfem.h) and the per-step drivers.
//
// Step drivers restate, on device-resident state, what the reference does in
//   IPCSSolver._solve_time_step            source/ns_ipcs_solver.py:198-208
//   (diffusion Newton / projection / correction forms :106-196)
//   InstationarySolverBase._advance_solution   source/ns_solver_base.py:1012-1016
//   IPCSSolver._advance_solution               source/ns_ipcs_solver.py:35-43
// with dolfin's NewtonSolver control (residual criterion, relaxation 1; parameters
// from source/ns_ipcs_solver.py:143-147) and Krylov solves instead of sparse LU.
#include "nsfem_internal.hpp"
#include <thread>
#include <chrono>
#include <algorithm>

using namespace nsfem;

static std::string g_create_error;

#define API_BEGIN try {
#define API_END(ctx)                                  \
  }                                                   \
  catch (const nsfem::Error& e) {                     \
    if (ctx) (ctx)->err = e.what();                   \
    else g_create_error = e.what();                   \
    return e.code;                                    \
  }                                                   \
  catch (const std::exception& e) {                   \
    if (ctx) (ctx)->err = e.what();                   \
    else g_create_error = e.what();                   \
    return NSFEM_ERR_ARG;                             \
  }                                                   \
  return NSFEM_OK;

static inline int64_t nvel(const nsfem_ctx* c) { return (int64_t)c->mesh.dim * c->mesh.n_p2; }
static inline int64_t npre(const nsfem_ctx* c) { return (int64_t)c->mesh.n_p1; }

static int64_t slot_size(const nsfem_ctx* c, int slot) {
  switch (slot) {
    case NSFEM_U0: case NSFEM_U1: case NSFEM_U2: case NSFEM_USTAR:
    case NSFEM_BODY_FORCE: case NSFEM_TRACTION: case NSFEM_CONV_N1: case NSFEM_CONV_N2:
      return nvel(c);
    case NSFEM_P: case NSFEM_P_OLD: case NSFEM_P2_OLD:
      return npre(c);
    case NSFEM_T0: case NSFEM_T1: case NSFEM_T2: case NSFEM_T_SOURCE: case NSFEM_TCONV_1: case NSFEM_TCONV_2:
      return (int64_t)c->mesh.n_p2;
    default:
      return -1;
  }
}

// the slots of the transported scalar are allocated (zeroed) when something first touches them
static inline bool scalar_slot(int slot) { return slot >= NSFEM_T0 && slot <= NSFEM_TCONV_2; }
static void ensure_scalar_slot(nsfem_ctx* c, int slot) {
  if (!scalar_slot(slot) || c->state[slot].p) return;
  c->state[slot].alloc((size_t)c->mesh.n_p2);
  c->state[slot].zero(c->stream);
}

// The classes of slots an entry point asks for -- the strict ones by name, the loose ones "any slot of this size" --
// and the one check of them.  The message is `prefix` (the feature, "" for none) and the text of the class.
enum class SlotClass {
  VelocityLevel,   // U0, U1, U2, USTAR
  PressureSlot,    // P, P_OLD, P2_OLD
  ScalarLevel,     // T0, T1, T2
  ScalarSlot,      // T0 .. T_SOURCE
  VelocitySized,   // dim * n_p2 doubles
  PressureSized,   // n_p1 doubles
  ScalarSized      // n_p2 doubles
};
static void require_slot(int slot, SlotClass cls, const char* prefix = "") {      // the classes by name
  bool ok = false;
  const char* what = "";
  switch (cls) {
    case SlotClass::VelocityLevel:
      ok = slot == NSFEM_U0 || slot == NSFEM_U1 || slot == NSFEM_U2 || slot == NSFEM_USTAR;
      what = "velocity_slot is not a velocity slot";
      break;
    case SlotClass::PressureSlot:
      ok = slot == NSFEM_P || slot == NSFEM_P_OLD || slot == NSFEM_P2_OLD;
      what = "pressure_slot is not a pressure slot";
      break;
    case SlotClass::ScalarLevel:
      ok = slot == NSFEM_T0 || slot == NSFEM_T1 || slot == NSFEM_T2;
      what = "scalar_slot is not a level of the transported scalar";
      break;
    case SlotClass::ScalarSlot:
      ok = slot >= NSFEM_T0 && slot <= NSFEM_T_SOURCE;
      what = "scalar_slot is not a scalar slot";
      break;
    default: throw Error(NSFEM_ERR_ARG, "a slot class by size needs the context");
  }
  NSFEM_REQUIRE(ok, std::string(prefix) + what);
}
static void require_slot(const nsfem_ctx* c, int slot, SlotClass cls, const char* prefix = "") {   // ... and by size
  int64_t n = 0;
  const char* what = "";
  switch (cls) {
    case SlotClass::VelocitySized: n = nvel(c); what = "not a velocity slot"; break;
    case SlotClass::PressureSized: n = npre(c); what = "not a pressure slot"; break;
    case SlotClass::ScalarSized: n = (int64_t)c->mesh.n_p2; what = "not a scalar slot"; break;
    default: return require_slot(slot, cls, prefix);
  }
  NSFEM_REQUIRE(slot >= 0 && slot < NSFEM_N_SLOTS && slot_size(c, slot) == n, std::string(prefix) + what);
}
// what the test hooks of the explicit terms check about their arguments
static void require_velocity_slot(int slot) { require_slot(slot, SlotClass::VelocityLevel); }
static void require_scalar_slot(int slot) { require_slot(slot, SlotClass::ScalarSlot); }
static void require_scalar_form(int form) {
  NSFEM_REQUIRE(form == 0 || form == 1, "scalar transport: convective form must be 0 (standard) or 1 (skew-symmetric)");
}
static void require_finite_weight(double weight) { NSFEM_REQUIRE(std::isfinite(weight), "bad weight"); }

// ... and how they return a vector: fill(out) runs on a work vector of the Krylov solvers (no slot and none of the
// step's buffers is written), n doubles of it go to the host
template <class Fill>
static void hook_to_host(nsfem_ctx* c, int64_t n, double* out_host, Fill&& fill) {
  c->kw.ensure(nvel(c));
  ++c->kw.touch;
  double* out = c->kw.q.p;
  fill(out);
  NSFEM_HIP(hipMemcpyAsync(out_host, out, sizeof(double) * n, hipMemcpyDeviceToHost, c->stream));
  NSFEM_HIP(hipStreamSynchronize(c->stream));
}

static HaloRange to_halo(const nsfem_halo& h) {
  HaloRange r;
  r.send_up_off = h.send_up_off; r.send_up_cnt = h.send_up_cnt;
  r.recv_above_off = h.recv_above_off; r.recv_above_cnt = h.recv_above_cnt;
  r.send_down_off = h.send_down_off; r.send_down_cnt = h.send_down_cnt;
  r.recv_below_off = h.recv_below_off; r.recv_below_cnt = h.recv_below_cnt;
  return r;
}

static void upload_pattern(hipStream_t s, HostPattern& h, Pattern& d, bool want_contrib = false) {
  d.n_rows = h.n_rows;
  d.n_cols = h.n_cols;
  d.nr = h.nr;
  d.nc = h.nc;
  d.nnz = (int)h.col.size();
  d.rowptr.upload(h.rowptr, s);
  d.col.upload(h.col, s);
  if (!h.diag.empty()) d.diag.upload(h.diag, s);
  d.slot.upload(h.slot, s);
  if (want_contrib) {
    if (h.cptr.empty()) {          // (patterns built without the index: serial fallback)
      const int64_t nc = (int64_t)h.slot.size() / (h.nr * h.nc), loc = h.nr * h.nc;
      build_inverse_index(d.nnz, nc * loc,
                          [&](int64_t src) { return h.slot[(size_t)(src % loc) * nc + src / loc]; },
                          h.cptr, h.cidx);
    }
    d.cptr.upload(h.cptr, s);
    d.cidx.upload(h.cidx, s);
    std::vector<int32_t>().swap(h.cptr);
    std::vector<int32_t>().swap(h.cidx);
  }
  d.h_rowptr.swap(h.rowptr);
  d.h_col.swap(h.col);
  build_rowblocks(d, s);
  std::vector<int32_t>().swap(h.slot);
}

extern "C" int nsfem_version(void) { return 2; }

extern "C" const char* nsfem_last_error(const nsfem_ctx* ctx) {
  return ctx ? ctx->err.c_str() : g_create_error.c_str();
}

extern "C" int nsfem_create(const nsfem_mesh_desc* m, int device, nsfem_ctx** out) {
  nsfem_ctx* ctx = nullptr;
  nsfem_ctx* fresh = nullptr;
  API_BEGIN
  NSFEM_REQUIRE(m && out, "null argument");
  refresh_env_switches();
  refresh_assembly_switches();
  *out = nullptr;
  NSFEM_REQUIRE(m->dim == 2 || m->dim == 3, "dim must be 2 (triangles) or 3 (tetrahedra)");
  NSFEM_REQUIRE(m->n_cells > 0 && m->n_vertices > 0 && m->n_p2 > 0 && m->n_p1 > 0, "empty mesh");
  NSFEM_REQUIRE(m->coords && m->cells && m->p2_dofmap && m->p1_dofmap, "null mesh array");
  int ndev = 0;
  NSFEM_HIP(hipGetDeviceCount(&ndev));
  if (device < 0 || device >= ndev) throw Error(NSFEM_ERR_HIP, "no such HIP device");
  NSFEM_HIP(hipSetDevice(device));
  fresh = new nsfem_ctx();
  fresh->device = device;
  fresh->step_fused = step_fused_enabled();
  fresh->newton_fused = newton_fused_enabled();
  NSFEM_HIP(hipStreamCreate(&fresh->stream));
  hipStream_t s = fresh->stream;
  const int nc = m->n_cells;
  // NSFEM_DEBUG_SETUP=1: wall-clock of the phases of this function on stderr
  const bool dbg_setup = std::getenv("NSFEM_DEBUG_SETUP") != nullptr;
  auto t_setup = std::chrono::steady_clock::now();
  auto lap = [&](const char* what) {
    if (!dbg_setup) return;
    (void)hipStreamSynchronize(s);
    const auto now = std::chrono::steady_clock::now();
    std::fprintf(stderr, "[nsfem_create] %-28s %.3f s\n", what, std::chrono::duration<double>(now - t_setup).count());
    t_setup = now;
  };
  // ---- mesh arrays, SoA
  const int dim = m->dim;
  NSFEM_REQUIRE(dim == 2 || dim == 3, "dim must be 2 (triangles) or 3 (tetrahedra)");
  const int nl1 = dim + 1, nl2 = dim == 2 ? 6 : 10;
  {
    std::vector<double> vx((size_t)nl1 * dim * nc);
    std::vector<int32_t> p2((size_t)nl2 * nc), p1((size_t)nl1 * nc);
    // (cell ranges on host threads; the cell volumes are summed afterwards in cell order: the same total on any
    // number of threads)
    std::vector<double> vol((size_t)nc);
    std::vector<int> bad((size_t)std::max(1, host_threads()), 0);
    auto fill_cells = [&](int c0, int c1, int tix) {
    for (int c = c0; c < c1; ++c) {
      double x[4][3] = {{0}};
      for (int v = 0; v < nl1; ++v) {
        const int vid = m->cells[(size_t)c * nl1 + v];
        if (vid < 0 || vid >= m->n_vertices) { bad[tix] = 1; return; }
        for (int d = 0; d < dim; ++d) {
          x[v][d] = m->coords[(size_t)vid * dim + d];
          vx[(size_t)(dim * v + d) * nc + c] = x[v][d];
        }
      }
      double det;
      if (dim == 2) {
        det = (x[1][0] - x[0][0]) * (x[2][1] - x[0][1]) - (x[2][0] - x[0][0]) * (x[1][1] - x[0][1]);
        vol[c] = 0.5 * std::fabs(det);
      } else {
        double a[3], b[3], e[3];
        for (int d = 0; d < 3; ++d) { a[d] = x[1][d] - x[0][d]; b[d] = x[2][d] - x[0][d]; e[d] = x[3][d] - x[0][d]; }
        det = a[0] * (b[1] * e[2] - b[2] * e[1]) - a[1] * (b[0] * e[2] - b[2] * e[0]) +
              a[2] * (b[0] * e[1] - b[1] * e[0]);
        vol[c] = std::fabs(det) / 6.0;
      }
      if (det == 0.0) { bad[tix] = 2; return; }
      for (int k = 0; k < nl2; ++k) p2[(size_t)k * nc + c] = m->p2_dofmap[(size_t)c * nl2 + k];
      for (int k = 0; k < nl1; ++k) p1[(size_t)k * nc + c] = m->p1_dofmap[(size_t)c * nl1 + k];
    }
    };
    {
      const int nt = (int)std::max<int64_t>(1, std::min<int64_t>(host_threads(), nc / 65536));
      std::vector<std::thread> th;
      for (int t = 1; t < nt; ++t)
        th.emplace_back(fill_cells, (int)((int64_t)nc * t / nt), (int)((int64_t)nc * (t + 1) / nt), t);
      fill_cells(0, (int)((int64_t)nc / nt), 0);
      for (auto& x : th) x.join();
      for (int t = 0; t < nt; ++t) {
        NSFEM_REQUIRE(bad[t] != 1, "cell vertex id out of range");
        NSFEM_REQUIRE(bad[t] != 2, "degenerate cell");
      }
    }
    double area = 0.0;
    for (int c = 0; c < nc; ++c) area += vol[c];
    fresh->area = area;
    fresh->h_p2map.assign(m->p2_dofmap, m->p2_dofmap + (size_t)nl2 * nc);
    fresh->h_p1map.assign(m->p1_dofmap, m->p1_dofmap + (size_t)nl1 * nc);
    fresh->mom_prec.c = fresh;
    fresh->mesh.dim = dim;
    fresh->mesh.n_cells = nc;
    fresh->mesh.n_p2 = m->n_p2;
    fresh->mesh.n_p1 = m->n_p1;
    fresh->mesh.n_vertices = m->n_vertices;
    fresh->mesh.vx.upload(vx, s);
    fresh->mesh.p2.upload(p2, s);
    fresh->mesh.p1.upload(p1, s);
  }
  lap("mesh arrays");
  // ---- sparsity patterns + slot maps (host), then device copies
  // (round 4: built on the device by one radix sort per pattern, pattern_device.hip; NSFEM_PATTERN_HOST=1 keeps the
  // threaded host construction of pattern.cpp -- the two produce the same arrays)
  const bool pattern_on_host = std::getenv("NSFEM_PATTERN_HOST") != nullptr;
  if (!pattern_on_host) {
    for (int64_t q = 0; q < (int64_t)nc * nl2; ++q)
      NSFEM_REQUIRE(m->p2_dofmap[q] >= 0 && m->p2_dofmap[q] < m->n_p2, "dof map entry out of range (P2)");
    for (int64_t q = 0; q < (int64_t)nc * nl1; ++q)
      NSFEM_REQUIRE(m->p1_dofmap[q] >= 0 && m->p1_dofmap[q] < m->n_p1, "dof map entry out of range (P1)");
  }
  {
    HostPattern h;
    if (pattern_on_host) {
      build_pattern(m->n_p2, m->n_p2, nc, m->p2_dofmap, nl2, m->p2_dofmap, nl2, true, h, true);
      lap("pattern p22 (host)");
      upload_pattern(s, h, fresh->p22, true);
      lap("pattern p22 upload");
    } else {
      build_pattern_device(s, m->n_p2, m->n_p2, nc, fresh->mesh.p2.p, nl2, fresh->mesh.p2.p, nl2, true, fresh->p22);
      lap("pattern p22 (device)");
    }
    if (pattern_on_host) {
      std::vector<int32_t> ptr, idx;
      build_inverse_index(m->n_p2, (int64_t)nc * nl2,
                          [&](int64_t src) { return m->p2_dofmap[src]; }, ptr, idx);
      fresh->mesh.nptr.upload(ptr, s);
      std::vector<int32_t> dst(idx.size());
      for (size_t pos = 0; pos < idx.size(); ++pos) {
        const int64_t src = idx[pos];
        dst[(size_t)(src % nl2) * nc + (size_t)(src / nl2)] = (int32_t)pos;
      }
      fresh->mesh.ndst.upload(dst, s);
    } else {
      build_node_index_device(s, m->n_p2, nc, nl2, fresh->mesh.p2.p, fresh->mesh.nptr, fresh->mesh.ndst);
    }
    fresh->mesh.ebuf.alloc((size_t)nc * nl2 * nl2 * dim * dim);
    fresh->mesh.rbuf.alloc((size_t)nc * nl2 * dim);
    lap("node-sorted index + buffers");
    if (pattern_on_host) {
      build_pattern(m->n_p1, m->n_p1, nc, m->p1_dofmap, nl1, m->p1_dofmap, nl1, true, h, true);
      upload_pattern(s, h, fresh->p11, true);
      lap("pattern p11");
      build_pattern(m->n_p1, m->n_p2, nc, m->p1_dofmap, nl1, m->p2_dofmap, nl2, false, h, true);
      upload_pattern(s, h, fresh->p12, true);
      lap("pattern p12");
      build_pattern(m->n_p2, m->n_p1, nc, m->p2_dofmap, nl2, m->p1_dofmap, nl1, false, h, true);
      upload_pattern(s, h, fresh->p21, true);
      lap("pattern p21");
    } else {
      build_pattern_device(s, m->n_p1, m->n_p1, nc, fresh->mesh.p1.p, nl1, fresh->mesh.p1.p, nl1, true, fresh->p11);
      lap("pattern p11");
      build_pattern_device(s, m->n_p1, m->n_p2, nc, fresh->mesh.p1.p, nl1, fresh->mesh.p2.p, nl2, false, fresh->p12);
      lap("pattern p12");
      build_pattern_device(s, m->n_p2, m->n_p1, nc, fresh->mesh.p2.p, nl2, fresh->mesh.p1.p, nl1, false, fresh->p21);
      lap("pattern p21");
    }
  }
  // ---- constant operators, integrated on the device
  QuadTables qt;
  fill_quad_tables(qt);
  upload_quad_tables(qt);
  if (dim == 3) upload_quad_tables_3d();
  upload_functional_tables(dim);
  upload_body_tables(dim);
  upload_derived_tables();
  fresh->M2.init(&fresh->p22, 1, 1, s);
  fresh->K2.init(&fresh->p22, 1, 1, s);
  fresh->L.init(&fresh->p22, 1, 1, s);
  fresh->J.init(&fresh->p22, dim, dim, s);
  fresh->Ap.init(&fresh->p11, 1, 1, s);
  fresh->Mp.init(&fresh->p11, 1, 1, s);
  fresh->Dv.init(&fresh->p12, 1, dim, s);
  fresh->Gr.init(&fresh->p21, dim, 1, s);
  fresh->DT.init(&fresh->p21, dim, 1, s);
  launch_assemble_p2_scalar(s, fresh->mesh, fresh->p22, fresh->M2.vals.p, fresh->K2.vals.p);
  launch_assemble_p1_scalar(s, fresh->mesh, fresh->p11, fresh->Ap.vals.p, fresh->Mp.vals.p);
  launch_assemble_div_grad(s, fresh->mesh, fresh->p12, fresh->p21, fresh->Dv.vals.p,
                           fresh->Gr.vals.p, fresh->DT.vals.p);
  lap("operator assembly (device)");
  for (BlockMat* A : {&fresh->M2, &fresh->K2, &fresh->Ap, &fresh->Mp}) A->sell_update(s);
  lap("SELL / dictionary copies");
  // ---- state + work vectors
  for (int i = 0; i < NSFEM_N_SLOTS; ++i) {
    if (scalar_slot(i)) continue;
    fresh->state[i].alloc((size_t)slot_size(fresh, i));
    fresh->state[i].zero(s);
  }
  const size_t nv = (size_t)nvel(fresh), np = (size_t)npre(fresh);
  for (DevBuf<double>* b : {&fresh->rhs_v, &fresh->dx_v, &fresh->gconst, &fresh->tmp_v,
                            &fresh->dinv_v, &fresh->dinv_m}) {
    b->alloc(nv);
    b->zero(s);
  }
  for (DevBuf<double>* b : {&fresh->rhs_p, &fresh->tmp_p, &fresh->dinv_p}) {
    b->alloc(np);
    b->zero(s);
  }
  fresh->mask_v.alloc(nv);
  fresh->mask_v.zero(s);
  fresh->mask_p.alloc(np);
  fresh->mask_p.zero(s);
  fresh->kw.ensure((int64_t)std::max(nv, np));
  NSFEM_HIP(hipStreamSynchronize(s));
  lap("state + work vectors");
  *out = fresh;
  fresh = nullptr;
  }
  catch (const nsfem::Error& e) {
    g_create_error = e.what();
    delete fresh;
    return e.code;
  }
  catch (const std::exception& e) {
    g_create_error = e.what();
    delete fresh;
    return NSFEM_ERR_ARG;
  }
  (void)ctx;
  return NSFEM_OK;
}

extern "C" void nsfem_destroy(nsfem_ctx* ctx) {
  if (!ctx) return;
  (void)hipSetDevice(ctx->device);
  if (ctx->stream) {
    (void)hipStreamSynchronize(ctx->stream);
    (void)hipStreamDestroy(ctx->stream);
  }
  delete ctx;
}

// element bounds of the Jacobi-scaled P2 mass matrix (host only; exposed for the CPU tests)
extern "C" int nsfem_p2_mass_bounds(int dim, double* lmin, double* lmax) {
  if ((dim != 2 && dim != 3) || !lmin || !lmax) return NSFEM_ERR_ARG;
  p2_mass_jacobi_bounds(dim, *lmin, *lmax);
  return NSFEM_OK;
}

extern "C" int nsfem_synchronize(nsfem_ctx* ctx) {
  API_BEGIN
  NSFEM_REQUIRE(ctx, "null context");
  NSFEM_HIP(hipStreamSynchronize(ctx->stream));
  API_END(ctx)
}

extern "C" int nsfem_set_coeffs(nsfem_ctx* ctx, const double c[6]) {
  API_BEGIN
  NSFEM_REQUIRE(ctx && c, "null argument");
  NSFEM_REQUIRE(std::isfinite(c[1]) && std::isfinite(c[2]), "pressure and viscous coefficients are required");
  for (int i = 0; i < 6; ++i) ctx->coef[i] = c[i];
  ctx->L_dirty = true;
  ctx->imex_ops_dirty = true;
  ctx->imex_lattice_agreed = -1;
  ctx->graph_epoch++;                  // (coefficients are baked into captured kernel arguments)
  API_END(ctx)
}

// the velocity V-cycle as a symmetric operator (CG, IMEX diffusion step) or as nsfem_mg_finalize set it up
// (non-symmetric, BiCGStab); the hierarchy's smoother data and fused launches are planned again at the next refresh
static void set_velocity_cycle_symmetric(nsfem_ctx* c, bool symmetric) {
  if (!c->mg_built || c->mg_v_symmetric == symmetric) return;
  Multigrid& mg = c->mg_v;
  if (symmetric) {
    c->mg_v_pre_saved = mg.pre_degree;
    c->mg_v_degree_saved = mg.degree;
    if (mg.pre_degree >= 0) {
      mg.degree = std::max(1, mg.pre_degree == 0 ? mg.degree - 1 : mg.degree);
      mg.pre_degree = -1;
    }
  } else {
    mg.pre_degree = c->mg_v_pre_saved;
    mg.degree = c->mg_v_degree_saved;
  }
  // (partitioned hierarchies: the replicated levels below the global coarse mesh run the same cycle)
  if (mg.tail) {
    mg.tail->degree = mg.degree;
    mg.tail->pre_degree = mg.pre_degree;
  }
  c->mg_v_symmetric = symmetric;
  c->mg_v_dirty = true;
}

extern "C" int nsfem_set_bdf(nsfem_ctx* ctx, const double alpha[3], double k) {
  API_BEGIN
  NSFEM_REQUIRE(ctx && alpha, "null argument");
  // alpha = (0, 0, 0) selects the stationary equations (monolithic step only)
  NSFEM_REQUIRE(k > 0.0 && std::isfinite(k) && std::isfinite(alpha[0]), "bad BDF coefficients");
  if (alpha[0] != ctx->alpha[0] || k != ctx->k) ctx->L_dirty = true;
  if (alpha[0] != ctx->alpha[0] || alpha[1] != ctx->alpha[1] || alpha[2] != ctx->alpha[2] || k != ctx->k) ctx->graph_epoch++;
  if (ctx->imex_active) {              // back to the fully implicit schemes: L = alpha0/k M + c_v K
    ctx->imex_active = false;
    ctx->L_dirty = true;
    ctx->graph_epoch++;
    set_velocity_cycle_symmetric(ctx, false);
  }
  for (int i = 0; i < 3; ++i) ctx->alpha[i] = alpha[i];
  ctx->k = k;
  API_END(ctx)
}

extern "C" int nsfem_set_imex(nsfem_ctx* ctx, const double alpha[3], const double beta[2], const double gamma[3],
                              double k) {
  API_BEGIN
  NSFEM_REQUIRE(ctx && alpha && beta && gamma, "null argument");
  bool finite = k > 0.0 && std::isfinite(k) && std::isfinite(beta[0]) && std::isfinite(beta[1]);
  for (int i = 0; i < 3; ++i) finite = finite && std::isfinite(alpha[i]) && std::isfinite(gamma[i]);
  NSFEM_REQUIRE(finite, "bad IMEX coefficients");
  // (the system matrix must be symmetric positive definite: CG solves the diffusion step)
  NSFEM_REQUIRE(alpha[0] > 0.0 && gamma[0] >= 0.0, "IMEX scheme needs alpha0 > 0 and gamma0 >= 0");
  const bool was = ctx->imex_active;
  // the system matrix alpha0/k M + gamma0 c_v K (and the hierarchy built on it) depends on these two numbers only
  if (!was || alpha[0] / k != ctx->alpha[0] / ctx->k || gamma[0] != ctx->imex_gamma[0]) ctx->L_dirty = true;
  bool changed = !was || k != ctx->k || beta[0] != ctx->imex_beta[0] || beta[1] != ctx->imex_beta[1];
  bool ops = !was || alpha[1] / k != ctx->alpha[1] / ctx->k || alpha[2] / k != ctx->alpha[2] / ctx->k;
  for (int i = 0; i < 3; ++i) {
    changed = changed || alpha[i] != ctx->alpha[i] || gamma[i] != ctx->imex_gamma[i];
    if (i > 0) ops = ops || gamma[i] != ctx->imex_gamma[i];
  }
  if (ops) ctx->imex_ops_dirty = true;
  if (changed) ctx->graph_epoch++;
  for (int i = 0; i < 3; ++i) { ctx->alpha[i] = alpha[i]; ctx->imex_gamma[i] = gamma[i]; }
  ctx->imex_beta[0] = beta[0];
  ctx->imex_beta[1] = beta[1];
  ctx->k = k;
  ctx->imex_active = true;
  API_END(ctx)
}

extern "C" int nsfem_set_convective_form(nsfem_ctx* ctx, int form, int picard) {
  API_BEGIN
  NSFEM_REQUIRE(ctx, "null context");
  NSFEM_REQUIRE(form >= 0 && form <= 3, "unknown convective form");
  if (ctx->conv_form != form || ctx->picard != (picard != 0)) ctx->graph_epoch++;
  ctx->conv_form = form;
  ctx->picard = picard != 0;
  API_END(ctx)
}

extern "C" int nsfem_set_viscous_form(nsfem_ctx* ctx, int traction_form) {
  API_BEGIN
  NSFEM_REQUIRE(ctx, "null context");
  ctx->traction_form = traction_form ? 1 : 0;
  ctx->imex_lattice_agreed = -1;
  ctx->graph_epoch++;
  if (ctx->traction_form && !ctx->have_E) {
    ctx->E.init(&ctx->p22, ctx->mesh.dim, ctx->mesh.dim, ctx->stream);
    launch_assemble_viscous_extra(ctx->stream, ctx->mesh, ctx->p22, ctx->E.vals.p);
    ctx->have_E = true;
  }
  API_END(ctx)
}

extern "C" int nsfem_set_dirichlet(nsfem_ctx* ctx, int field, int32_t n, const int32_t* dofs,
                                   const double* vals) {
  API_BEGIN
  NSFEM_REQUIRE(ctx, "null context");
  NSFEM_REQUIRE(field == NSFEM_VELOCITY || field == NSFEM_PRESSURE ||
                    field == NSFEM_PRESSURE_PRECOND || field == NSFEM_SCALAR, "bad field");
  NSFEM_REQUIRE(n >= 0 && (n == 0 || dofs), "bad Dirichlet arrays");
  if (field == NSFEM_SCALAR) {
    // transported scalar: dofs are P2 nodes; later entries win on duplicates, as below
    NSFEM_REQUIRE(n == 0 || vals, "bad Dirichlet arrays");
    const int64_t size = ctx->mesh.n_p2;
    std::vector<int32_t> last((size_t)size, -1), d;
    std::vector<double> v;
    for (int32_t i = 0; i < n; ++i) {
      NSFEM_REQUIRE(dofs[i] >= 0 && dofs[i] < size, "Dirichlet dof out of range");
      last[dofs[i]] = i;
    }
    for (int64_t k = 0; k < size; ++k)
      if (last[k] >= 0) {
        d.push_back((int32_t)k);
        v.push_back(vals[last[k]]);
      }
    nsfem_ctx::Scalar& sc = ctx->sc;
    hipStream_t s = ctx->stream;
    sc.bc_dofs.upload(d, s);
    sc.bc_vals.upload(v, s);
    if (!sc.mask.p) sc.mask.alloc((size_t)size);
    sc.mask.zero(s);
    launch_fill_mask(s, (int)d.size(), sc.bc_dofs.p, sc.mask.p);
    if (sc.h_bc != d) {                     // (re-allocated dof arrays are baked into captured iteration graphs)
      ctx->graph_epoch++;
      sc.dinv_dirty = true;
    }
    sc.nbc = (int)d.size();
    sc.h_bc.swap(d);
    NSFEM_HIP(hipStreamSynchronize(s));
    return NSFEM_OK;
  }
  if (field == NSFEM_PRESSURE_PRECOND) {
    // Dirichlet set of the pressure Laplacian inside the Schur-complement preconditioner of
    // the monolithic scheme (open boundaries + true pressure conditions); values unused
    std::vector<int32_t> d(dofs, dofs + n);
    std::sort(d.begin(), d.end());
    d.erase(std::unique(d.begin(), d.end()), d.end());
    for (int32_t k : d) NSFEM_REQUIRE(k >= 0 && k < npre(ctx), "Dirichlet dof out of range");
    if (d != ctx->h_bc_s || !ctx->mask_s.p) {
      DevBuf<int32_t> dd;
      dd.upload(d, ctx->stream);
      if (!ctx->mask_s.p) ctx->mask_s.alloc((size_t)npre(ctx));
      ctx->mask_s.zero(ctx->stream);
      launch_fill_mask(ctx->stream, (int)d.size(), dd.p, ctx->mask_s.p);
      NSFEM_HIP(hipStreamSynchronize(ctx->stream));
      ctx->h_bc_s.swap(d);
      ctx->mg_s_dirty = true;
    }
    return NSFEM_OK;
  }
  NSFEM_REQUIRE(n == 0 || vals, "bad Dirichlet arrays");
  const int64_t size = field == NSFEM_VELOCITY ? nvel(ctx) : npre(ctx);
  // later entries win on duplicates (list order of dolfin bc.apply): dedupe on host
  std::vector<int32_t> d;
  std::vector<double> v;
  {
    std::vector<int32_t> last((size_t)size, -1);
    for (int32_t i = 0; i < n; ++i) {
      NSFEM_REQUIRE(dofs[i] >= 0 && dofs[i] < size, "Dirichlet dof out of range");
      last[dofs[i]] = i;
    }
    for (int64_t k = 0; k < size; ++k)
      if (last[k] >= 0) {
        d.push_back((int32_t)k);
        v.push_back(vals[last[k]]);
      }
  }
  hipStream_t s = ctx->stream;
  DevBuf<int32_t>& dd = field == NSFEM_VELOCITY ? ctx->bc_v_dofs : ctx->bc_p_dofs;
  DevBuf<double>& dv = field == NSFEM_VELOCITY ? ctx->bc_v_vals : ctx->bc_p_vals;
  DevBuf<uint8_t>& mask = field == NSFEM_VELOCITY ? ctx->mask_v : ctx->mask_p;
  dd.upload(d, s);
  dv.upload(v, s);
  mask.zero(s);
  launch_fill_mask(s, (int)d.size(), dd.p, mask.p);
  launch_overlay_ghost(s, size, field == NSFEM_VELOCITY ? ctx->ghost_v.p : ctx->ghost_p.p, mask.p);
  std::vector<int32_t>& prev = field == NSFEM_VELOCITY ? ctx->h_bc_v : ctx->h_bc_p;
  const bool changed = prev != d;
  if (changed) ctx->graph_epoch++;  // the device dof arrays were re-allocated (values-only
                                    // updates keep the pointers: captured graphs stay valid)
  if (field == NSFEM_VELOCITY) {
    // the values as a dense vector for the residual launch that sets its own Dirichlet rows (one rank, 2D), refreshed
    // with every call
    if (ctx->newton_fused && ctx->mesh.dim == 2 && !ctx->ghost_v.p) {
      if (!ctx->bc_v_dense.p) ctx->bc_v_dense.alloc((size_t)size);
      ctx->bc_v_dense.zero(s);
      launch_set_values(s, (int)d.size(), dd.p, dv.p, ctx->bc_v_dense.p);
    }
    ctx->nbc_v = (int)d.size();
    ctx->imex_lattice_agreed = -1;
    if (changed) {
      ctx->dinv_m_ready = false;
      ctx->mg_v_dirty = true;
      for (nsfem::MGLevel& L : ctx->mg_mv.lv) L.sidm_for = nullptr;   // (the mass smoother shares mask_v)
    }
  } else {
    ctx->nbc_p = (int)d.size();
    ctx->bc_p_any = -1;            // partitioned meshes: agreed on by all ranks at the next solve
    if (changed) { ctx->dinv_p_ready = false; ctx->mg_p_dirty = true; }
  }
  prev.swap(d);
  NSFEM_HIP(hipStreamSynchronize(s));
  API_END(ctx)
}

extern "C" int64_t nsfem_state_size(const nsfem_ctx* ctx, int slot) {
  if (!ctx || slot < 0 || slot >= NSFEM_N_SLOTS) return -1;
  return slot_size(ctx, slot);
}

extern "C" void* nsfem_state_devptr(nsfem_ctx* ctx, int slot) {
  if (!ctx || slot < 0 || slot >= NSFEM_N_SLOTS) return nullptr;
  if (scalar_slot(slot) && !ctx->state[slot].p) {
    try { ensure_scalar_slot(ctx, slot); } catch (const std::exception&) { return nullptr; }
  }
  return ctx->state[slot].p;
}

extern "C" int nsfem_set_state(nsfem_ctx* ctx, int slot, const double* host, int64_t n) {
  API_BEGIN
  NSFEM_REQUIRE(ctx && host, "null argument");
  NSFEM_REQUIRE(slot >= 0 && slot < NSFEM_N_SLOTS && n == slot_size(ctx, slot), "bad slot / size");
  ensure_scalar_slot(ctx, slot);
  NSFEM_HIP(hipMemcpyAsync(ctx->state[slot].p, host, sizeof(double) * n, hipMemcpyHostToDevice,
                           ctx->stream));
  NSFEM_HIP(hipStreamSynchronize(ctx->stream));
  if (slot == NSFEM_BODY_FORCE) ctx->have_body_force = true;
  if (slot == NSFEM_TRACTION) ctx->have_traction = true;
  if (slot == NSFEM_P || slot == NSFEM_P_OLD || slot == NSFEM_P2_OLD) ctx->pressure_history = 0;
  // IMEX: the stored convection vectors follow the velocity levels they were evaluated at
  if (slot == NSFEM_U1 || slot == NSFEM_CONV_N1) ctx->conv_n1_fresh = false;
  if (slot == NSFEM_U2) ctx->conv_n2_valid = false;
  // (Lagrangian averaging: a constant of level n formed on another u1 is not that of this one; cs2_prev stays -- an
  // N(u2) that is formed again reads it)
  if (slot == NSFEM_U1) ctx->dyn.lag.cur_valid = false;
  // ... and on partitioned meshes the ghost entries of a slot written from the host are whatever the caller put there
  if (slot == NSFEM_U1) ctx->u1_ghost_fresh = false;
  if (slot == NSFEM_U2) ctx->u2_ghost_fresh = false;
  if (slot == NSFEM_CONV_N2) { ctx->conv_n2_valid = true; ctx->conv_key.vouched = true; }   // (the caller vouches for it)
  // scalar transport: the stored convection vectors follow the levels (velocity and scalar) they were evaluated at
  if (slot == NSFEM_U1 || slot == NSFEM_T1 || slot == NSFEM_TCONV_1) ctx->sc.conv1_fresh = false;
  if (slot == NSFEM_U2 || slot == NSFEM_T2) ctx->sc.conv2_valid = false;
  if (slot == NSFEM_TCONV_2) {
    ctx->sc.conv2_valid = true; ctx->sc.conv2_weight = 1.0;
    ctx->sc.conv_key = nsfem_ctx::Scalar::Key::of(*ctx);
    ctx->sc.conv_key.vouched = true;
  }
  if (slot == NSFEM_T_SOURCE) ctx->sc.have_source = true;
  API_END(ctx)
}

extern "C" int nsfem_get_state(nsfem_ctx* ctx, int slot, double* host, int64_t n) {
  API_BEGIN
  NSFEM_REQUIRE(ctx && host, "null argument");
  NSFEM_REQUIRE(slot >= 0 && slot < NSFEM_N_SLOTS && n == slot_size(ctx, slot), "bad slot / size");
  ensure_scalar_slot(ctx, slot);
  NSFEM_HIP(hipMemcpyAsync(host, ctx->state[slot].p, sizeof(double) * n, hipMemcpyDeviceToHost,
                           ctx->stream));
  NSFEM_HIP(hipStreamSynchronize(ctx->stream));
  API_END(ctx)
}

// ------------------------------------------------------------------ internals
// Mass-dominated velocity operators (small time steps): on a level where the stiffness part of
// the diagonal is at most `mg_trunc_ratio` times the mass part, a = ap M + b K is spectrally close
// to the (well conditioned) mass matrix, lambda_min(D^-1 a) >= lambda_min(D_M^-1 M) / (1 + r) with
// r = max_i b K_ii / (ap M_ii) and lambda_min(D_M^-1 M) = 1/2 for P1 elements (element bound) --
// a few Chebyshev steps SOLVE that level, and every coarser level, the dense coarse solve and (on
// partitioned meshes) the global coarse all-reduce drop out of the cycle.
static void select_velocity_cycle_depth(nsfem_ctx* c, double ap, double b) {
  Multigrid& mg = c->mg_v;
  mg.active = 0;
  if (!(c->mg_trunc_ratio > 0.0) || !(ap > 0.0) || mg.lv.size() < 3) return;
  hipStream_t s = c->stream;
  c->kw.ensure(nvel(c));
  double* parts = c->kw.parts.p;
  // level 1 = P1 on the fine mesh, level l + 2 = coarse[l]
  for (size_t l = 1; l + 1 < mg.lv.size(); ++l) {
    double r;
    if (l == 1) r = diag_ratio_max(s, c->p11, c->Mp.vals.p, c->Ap.vals.p, parts);
    else if (l - 2 < c->coarse.size())
      r = diag_ratio_max(s, c->coarse[l - 2]->pat, c->coarse[l - 2]->M.vals.p, c->coarse[l - 2]->K.vals.p, parts);
    else break;
    r *= b / ap;
    if (c->distributed()) {           // every rank must run the same cycle
      NSFEM_HIP(hipMemcpyAsync(parts, &r, sizeof(double), hipMemcpyHostToDevice, s));
      c->comm->allreduce_max(s, parts, 1);
      NSFEM_HIP(hipMemcpyAsync(&r, parts, sizeof(double), hipMemcpyDeviceToHost, s));
      NSFEM_HIP(hipStreamSynchronize(s));
    }
    if (r <= c->mg_trunc_ratio) {
      mg.active = l + 1;
      mg.trunc_lmin = 0.5 / (1.0 + r);
      mg.trunc_tol = c->mg_trunc_tol;
      return;
    }
  }
}

// stencil dictionary of the scalar P2 operators (lattice meshes only): shared by every a M + b K; used by the
// smoothing steps of the velocity multigrid (and, where it equals the matrices bit for bit, by every product)
static void ensure_dict22(nsfem_ctx* c) {
  if (c->dict22_tried) return;
  c->dict22_tried = true;
  if (build_stencil_dict(c->stream, c->p22, c->M2.vals.p, c->K2.vals.p, c->dict22)) {
    c->L.dict = &c->dict22;
    c->Lprec.dict = &c->dict22;
    if (c->dict22.exact) {       // the Chebyshev / CG mass solves may use it too
      c->M2.dict = &c->dict22;
      c->M2.sell_update(c->stream);
    }
  }
}

static void ensure_L(nsfem_ctx* c) {
  if (!c->L_dirty) return;
  // L = alpha0/k M + c_viscous K   (scalar P2; acts on all velocity components)
  // (IMEX pressure correction: alpha0/k M + gamma0 c_v K, the system matrix of its diffusion step)
  const double a = c->alpha[0] / c->k, b = c->imex_active ? c->imex_gamma[0] * c->coef[2] : c->coef[2];
  if (c->imex_active) ++c->imex_matrix_builds;
  launch_scale_combine(c->stream, c->p22.nnz, a, c->M2.vals.p, b, c->K2.vals.p, c->L.vals.p);
  ensure_dict22(c);
  c->L.sell_update(c->stream);
  // preconditioner version: (alpha0/k + shift) M + c_viscous K -- the multigrid hierarchy of the
  // velocity block is built on it.  shift = 0 (all transient problems): the operator itself.
  // shift = 1/tau > 0 (stationary problems at high cell Peclet numbers): the V-cycle then
  // approximates (J + M/tau)^{-1}, the "time-step preconditioner" -- convection-dominated modes
  // are clustered at 1, only the slow diffusive modes are left to the Krylov method.
  const double ap = a + c->prec_shift;
  if (c->prec_shift != 0.0) {
    if (!c->Lprec.vals.p) c->Lprec.init(&c->p22, 1, 1, c->stream);
    launch_scale_combine(c->stream, c->p22.nnz, ap, c->M2.vals.p, b, c->K2.vals.p, c->Lprec.vals.p);
    c->Lprec.sell_update(c->stream);
  }
  if (c->mg_built) {
    c->mg_v.lv[0].A = c->prec_shift != 0.0 ? &c->Lprec : &c->L;
    launch_scale_combine(c->stream, c->p11.nnz, ap, c->Mp.vals.p, b, c->Ap.vals.p, c->Lc0.vals.p);
    if (!c->dict11_tried) {        // the fine P1 level of both hierarchies (smoothing steps)
      c->dict11_tried = true;
      if (build_stencil_dict(c->stream, c->p11, c->Mp.vals.p, c->Ap.vals.p, c->dict11)) {
        c->Lc0.dict = &c->dict11;
        c->Ap.dict = &c->dict11;
        c->Ap.sell_update(c->stream);
        c->Mp.dict = &c->dict11;
        c->Mp.sell_update(c->stream);
      }
    }
    c->Lc0.sell_update(c->stream);
    for (nsfem_ctx::P1Level* lv : c->coarse) {
      launch_scale_combine(c->stream, lv->pat.nnz, ap, lv->M.vals.p, b, lv->K.vals.p, lv->Lc.vals.p);
      lv->Lc.sell_update(c->stream);
    }
    if (c->global_coarse) {
      nsfem_ctx::P1Level* g = c->global_coarse;
      launch_scale_combine(c->stream, g->pat.nnz, ap, g->M.vals.p, b, g->K.vals.p, g->Lc.vals.p);
      g->Lc.sell_update(c->stream);
      for (nsfem_ctx::P1Level* t : c->global_tail) {
        launch_scale_combine(c->stream, t->pat.nnz, ap, t->M.vals.p, b, t->K.vals.p, t->Lc.vals.p);
        t->Lc.sell_update(c->stream);
      }
    }
    select_velocity_cycle_depth(c, ap, b);
    c->mg_v_dirty = true;
  }
  c->L_dirty = false;
}

// (re)build masks / smoother data / coarse inverse of a hierarchy when its inputs changed
static void mg_refresh_schur(nsfem_ctx* c) {
  auto ghost_flags = [&](std::vector<uint8_t>& m) {
    for (size_t i = 0; i < c->h_ghost_p1.size(); ++i)
      if (c->h_ghost_p1[i]) m[i] = 2;
  };
  if (c->mg_s_dirty) {
    c->graph_epoch++;
    std::vector<uint8_t> m((size_t)npre(c), 0);
    for (int32_t d : c->h_bc_s) m[d] = 1;
    ghost_flags(m);
    const bool singular = c->schur_singular >= 0 ? c->schur_singular != 0
                                                 : (c->distributed() ? true : c->h_bc_s.empty());
    c->mg_s.refresh(c->stream, m, singular);
    c->mg_s_dirty = false;
  }
  if (!c->mg_m.ready) {
    std::vector<uint8_t> m((size_t)npre(c), 0);
    ghost_flags(m);
    if (c->distributed()) {       // level 0 of the mass smoother needs its own device mask
      if (!c->mask_m.p) c->mask_m.alloc((size_t)npre(c));
      c->mask_m.upload(m, c->stream);
      c->mg_m.lv[0].mask = c->mask_m.p;
    }
    c->mg_m.refresh(c->stream, m, false);
  }
}

static void mg_refresh(nsfem_ctx* c, bool momentum) {
  if (momentum) {
    ensure_L(c);
    if (!c->mg_v_dirty) return;
    c->graph_epoch++;
    std::vector<uint8_t> m((size_t)nvel(c), 0);
    for (int32_t d : c->h_bc_v) m[d] = 1;
    const size_t dim = (size_t)c->mesh.dim;
    for (size_t i = 0; i < c->h_ghost_p2.size(); ++i)
      if (c->h_ghost_p2[i])
        for (size_t a = 0; a < dim; ++a) m[dim * i + a] = 2;
    c->mg_v.refresh(c->stream, m, false);
    c->mg_v_dirty = false;
  } else {
    if (!c->mg_p_dirty) return;
    c->graph_epoch++;
    std::vector<uint8_t> m((size_t)npre(c), 0);
    for (int32_t d : c->h_bc_p) m[d] = 1;
    for (size_t i = 0; i < c->h_ghost_p1.size(); ++i)
      if (c->h_ghost_p1[i]) m[i] = 2;
    // partitioned: whether the problem is singular is decided on the all-reduced mask
    c->mg_p.refresh(c->stream, m, c->distributed() ? true : c->h_bc_p.empty());
    c->mg_p_dirty = false;
  }
}

void nsfem_ctx::MomentumPrec::apply(hipStream_t s, const double* r, double* z) {
  // Newton rows of Dirichlet dofs are identity rows: the preconditioner must be too -- the last
  // finest-level smoothing step of the cycle writes z = r on them (Multigrid::identity_rows)
  c->mg_v.apply(s, r, z);
}

constexpr int P10 = 10;      // partial-sum slots 10, 11 of the Krylov work space belong to the drivers
static double cc_of(const nsfem_ctx* c) { return std::isfinite(c->coef[0]) ? c->coef[0] : 0.0; }
// Coriolis factor 2 c_cor omega (source/ns_solver_base.py:173-191): a scalar about e_z in 2D, the
// vector 2 c_cor Omega in 3D (coriolis_gamma3)
static bool coriolis_active(const nsfem_ctx* c) {
  if (c->mesh.dim == 2) return c->omega != 0.0;
  return c->omega3[0] != 0.0 || c->omega3[1] != 0.0 || c->omega3[2] != 0.0;
}
// Euler acceleration c_e (d Omega/dt) x x: is an angular acceleration set?
static bool euler_active(const nsfem_ctx* c) {
  if (c->mesh.dim == 2) return c->omega_dot != 0.0;
  return c->omega_dot3[0] != 0.0 || c->omega_dot3[1] != 0.0 || c->omega_dot3[2] != 0.0;
}
static double coriolis_gamma(const nsfem_ctx* c) {
  if (!coriolis_active(c)) return 0.0;
  if (!std::isfinite(c->coef[4])) throw Error(NSFEM_ERR_ARG, "angular velocity set but coriolis_term coefficient is None");
  return 2.0 * c->coef[4] * (c->mesh.dim == 2 ? c->omega : 1.0);
}
// y += (2 c_cor Omega x u, w): the mass matrix applied to the rotated field
static void coriolis_apply(nsfem_ctx* c, double g, const double* u, double* y,
                           const uint8_t* skipmask = nullptr) {
  hipStream_t s = c->stream;
  if (!c->rot_tmp.p) c->rot_tmp.alloc((size_t)nvel(c));
  if (c->mesh.dim == 2) {
    launch_rot90(s, c->mesh.n_p2, g, u, c->rot_tmp.p);
  } else {
    const double gv[3] = {g * c->omega3[0], g * c->omega3[1], g * c->omega3[2]};
    launch_cross3(s, c->mesh.n_p2, gv, u, c->rot_tmp.p);
  }
  launch_spmv_axpy(s, c->M2, c->mesh.dim, 1.0, c->rot_tmp.p, y, skipmask);
}

// lattice meshes: dictionary copies of the rectangular divergence / gradient blocks (the monolithic operator uses
// them in every Krylov iteration; the pressure-correction scheme once per step each -- there only dictionaries that
// equal the assembled blocks bit for bit serve, see spmv_dispatch)
static void ensure_div_dicts(nsfem_ctx* ctx) {
  if (ctx->dictD_tried) return;
  ctx->dictD_tried = true;
  hipStream_t s = ctx->stream;
  const int dim = ctx->mesh.dim;
  if (build_stencil_dict(s, ctx->p21, ctx->DT.vals.p, nullptr, ctx->dict21, dim, true)) {
    ctx->DT.dict = &ctx->dict21;
    ctx->DT.sell_update(s);
  }
  if (build_stencil_dict(s, ctx->p12, ctx->Dv.vals.p, nullptr, ctx->dict12, dim, true)) {
    ctx->Dv.dict = &ctx->dict12;
    ctx->Dv.sell_update(s);
  }
  if (build_stencil_dict(s, ctx->p21, ctx->Gr.vals.p, nullptr, ctx->dict21g, dim, true)) {
    ctx->Gr.dict = &ctx->dict21g;
    ctx->Gr.sell_update(s);
  }
}

// v += c_e (d Omega/dt) x x, nodal: the Euler acceleration before the mass product (ns_solver_base.py:193-211)
static void euler_add(nsfem_ctx* c, double* v) {
  hipStream_t s = c->stream;
  const int64_t nv = nvel(c);
  NSFEM_REQUIRE(std::isfinite(c->coef[5]), "angular acceleration set but euler_term coefficient is None");
  if (!c->rot_field.p) {
    c->rot_field.alloc((size_t)nv);
    if (c->mesh.dim == 2) launch_rot_field(s, c->mesh, c->rot_field.p);       // e_z x x
    else launch_coord_field_3d(s, c->mesh, c->rot_field.p);                    // x
  }
  if (c->mesh.dim == 2) {
    launch_axpby(s, nv, 1.0, v, c->coef[5] * c->omega_dot, c->rot_field.p, v);
  } else {
    if (!c->rot_tmp.p) c->rot_tmp.alloc((size_t)nv);
    const double a[3] = {c->coef[5] * c->omega_dot3[0], c->coef[5] * c->omega_dot3[1],
                         c->coef[5] * c->omega_dot3[2]};
    launch_cross3(s, c->mesh.n_p2, a, c->rot_field.p, c->rot_tmp.p);
    launch_axpby(s, nv, 1.0, v, 1.0, c->rot_tmp.p, v);
  }
}

// time-step constant part of the momentum residual:
//   g = M (a1 u1 + a2 u2) / k - c_p (p_old, div w) - c_b M f + traction
static void momentum_begin_step(nsfem_ctx* c, bool with_old_pressure = true) {
  hipStream_t s = c->stream;
  const int64_t nv = nvel(c);
  ensure_L(c);
  ensure_div_dicts(c);
  const double a1 = c->alpha[1] / c->k, a2 = c->alpha[2] / c->k;
  if (c->have_body_force) {
    NSFEM_REQUIRE(std::isfinite(c->coef[3]), "body force set but body_force_term coefficient is None");
    launch_lincomb3(s, nv, a1, c->state[NSFEM_U1].p, a2, c->state[NSFEM_U2].p, -c->coef[3],
                    c->state[NSFEM_BODY_FORCE].p, c->tmp_v.p);
  } else {
    launch_axpby(s, nv, a1, c->state[NSFEM_U1].p, a2, c->state[NSFEM_U2].p, c->tmp_v.p);
  }
  if (euler_active(c)) euler_add(c, c->tmp_v.p);
  // fused step frame (one rank, 2D, exact dictionaries of both operators, none of the optional terms): the product
  // with M and the accumulated D^T p_old in ONE launch, gconst written once
  if (c->step_fused && with_old_pressure && !c->distributed() && c->mesh.dim == 2 && !c->have_body_force &&
      !c->have_traction && !euler_active(c) && spmv_pair_available(c->M2, c->DT)) {
    launch_spmv_pair_accum(s, c->M2, c->DT, c->tmp_v.p, -c->coef[1], c->state[NSFEM_P_OLD].p, c->gconst.p);
    ++c->step_frame_launches[0];
    return;
  }
  launch_spmv(s, c->M2, c->mesh.dim, c->tmp_v.p, c->gconst.p, nullptr, MASK_NONE);
  if (with_old_pressure)   // IPCS: - c_p (p_old, div w); the monolithic scheme keeps p unknown
    launch_spmv_axpy(s, c->DT, 1, -c->coef[1], c->state[NSFEM_P_OLD].p, c->gconst.p, nullptr);
  if (c->have_traction)
    launch_axpby(s, nv, 1.0, c->gconst.p, 1.0, c->state[NSFEM_TRACTION].p, c->gconst.p);
}

// b = L u* [+ c_v E u*] + g + c_c conv(u*) ;  Dirichlet rows: u*_i - g_i ;  returns |b|
// |x|_2 over owned entries (ghost entries are zeroed first), all-reduced over the ranks
static double global_norm(nsfem_ctx* c, int64_t n, double* x, const uint8_t* ghostmask) {
  hipStream_t s = c->stream;
  if (ghostmask) launch_zero_ghost(s, n, ghostmask, x);
  double* parts = c->kw.parts.p + (size_t)10 * kParts;
  launch_dot(s, n, x, x, parts);
  if (c->distributed()) c->comm->allreduce_sum(s, parts, kParts);
  return std::sqrt(host_sum_parts(s, c->kw, 10));
}

static void fill_linop(nsfem_ctx* c, LinOp& op, bool velocity) {
  op.graph_epoch = c->graph_epoch;
  if (!c->distributed()) return;
  op.comm = c->comm;
  op.halo = velocity ? &c->halo_p2 : &c->halo_p1;
  op.halo_width = velocity ? c->mesh.dim : 1;
  op.ghostmask = velocity ? c->mask_v.p : c->mask_p.p;
  op.n_global = velocity ? 2 * c->n_p2_global : c->n_p1_global;
}

static int jacobian_path(nsfem_ctx* c, bool explicit_rotation = false);
static void momentum_residual_raw(nsfem_ctx* c, const double* u, double* out) {
  hipStream_t s = c->stream;
  const int64_t nv = nvel(c);
  // lattice meshes (same conditions as the one-launch Jacobian action): product, + g, element kernel and node sums
  // in one launch of k_jac_lattice<FORM, 0>
  if (jacobian_path(c) == 2 &&
      launch_residual_lattice(s, c->mesh, c->L, u, c->gconst.p, cc_of(c), c->conv_form, out)) {
    ++c->jac_lattice_launches;
    return;
  }
  launch_spmv(s, c->L, c->mesh.dim, u, out, nullptr, MASK_NONE);
  launch_axpby(s, nv, 1.0, out, 1.0, c->gconst.p, out);
  if (c->traction_form) launch_spmv_axpy(s, c->E, 1, c->coef[2], u, out, nullptr);
  const double cc = cc_of(c);
  if (cc != 0.0) launch_convection_residual(s, c->mesh, u, cc, out, c->conv_form);
  const double g = coriolis_gamma(c);
  if (g != 0.0) coriolis_apply(c, g, u, out);
}

// The frame of the Newton iteration inside the residual launch (k_jac_lattice<FORM, 7 / 8>): one rank, the one-launch
// lattice path on a dictionary that equals the matrix, a velocity mask, the switch on
static bool newton_frame_available(nsfem_ctx* c) {
  return c->newton_fused && !c->distributed() && c->mask_v.p && !c->ghost_v.p && c->bc_v_dense.p &&
         jacobian_path(c) == 2 && residual_frame_lattice_available(c->mesh, c->L);
}
// frame: the caller is the Newton loop of nsfem_step_ipcs -- Dirichlet rows and the sum of squares come out of the
// residual launch, and so does a pending update u* -= dx (momentum_solve_update left it)
static double momentum_residual(nsfem_ctx* c, bool frame = false) {
  hipStream_t s = c->stream;
  const int64_t nv = nvel(c);
  if (frame && newton_frame_available(c)) {
    const bool upd = c->newton_update_pending;
    const int ntiles = lattice_tile_count(c->mesh);
    if (!c->tile_parts.p) c->tile_parts.alloc((size_t)ntiles);
    if (upd && !c->ustar_alt.p) c->ustar_alt.alloc((size_t)nv);
    if (launch_residual_frame_lattice(s, c->mesh, c->L, c->state[NSFEM_USTAR].p, upd ? c->dx_v.p : nullptr,
                                      upd ? c->ustar_alt.p : nullptr, c->gconst.p, cc_of(c), c->conv_form, c->mask_v.p,
                                      c->bc_v_dense.p, c->rhs_v.p, c->tile_parts.p)) {
      ++c->jac_lattice_launches;
      ++c->newton_frame_launches[0];
      if (upd) {
        std::swap(c->state[NSFEM_USTAR].p, c->ustar_alt.p);
        c->newton_update_pending = false;
        ++c->newton_frame_launches[1];
      }
      return std::sqrt(host_sum_run(s, c->kw, c->tile_parts.p, ntiles));
    }
  }
  if (c->newton_update_pending) {              // (the launch was refused after all: the update as a launch of its own)
    launch_axpby(s, nv, 1.0, c->state[NSFEM_USTAR].p, -1.0, c->dx_v.p, c->state[NSFEM_USTAR].p);
    c->newton_update_pending = false;
  }
  double* u = c->state[NSFEM_USTAR].p;
  momentum_residual_raw(c, u, c->rhs_v.p);
  if (!c->distributed() && c->mask_v.p) {      // Dirichlet rows and the norm in one launch (mask != 0 <=> bc dof)
    double* parts = c->kw.parts.p + (size_t)10 * kParts;
    launch_bc_residual_norm(s, nv, c->rhs_v.p, c->mask_v.p, c->nbc_v, c->bc_v_dofs.p, c->bc_v_vals.p, u, parts);
    return std::sqrt(host_sum_parts(s, c->kw, 10));
  }
  launch_set_bc_residual(s, c->nbc_v, c->bc_v_dofs.p, c->bc_v_vals.p, u, c->rhs_v.p);
  return global_norm(c, nv, c->rhs_v.p, c->ghost_v.p ? c->mask_v.p : nullptr);
}

static void momentum_jacobian(nsfem_ctx* c, int vel_slot = NSFEM_USTAR) {
  hipStream_t s = c->stream;
  const double* E = c->traction_form ? c->E.vals.p : nullptr;
  const double cc = cc_of(c);
  if (cc != 0.0)
    launch_convection_jacobian(s, c->mesh, c->p22, c->state[vel_slot].p, cc, c->L.vals.p, E,
                               c->coef[2], c->J.vals.p, c->conv_form, c->picard);
  else
    launch_jacobian_init(s, c->mesh.dim, c->p22.nnz, c->L.vals.p, E, c->coef[2], c->J.vals.p);
  const double g = coriolis_gamma(c);
  if (g != 0.0) {
    if (c->mesh.dim == 2) {
      launch_jac_add_skew(s, c->p22.nnz, g, c->M2.vals.p, c->J.vals.p);
    } else {
      const double gv[3] = {g * c->omega3[0], g * c->omega3[1], g * c->omega3[2]};
      launch_jac_add_skew3(s, c->p22.nnz, gv, c->M2.vals.p, c->J.vals.p);
    }
  }
  launch_inv_diag(s, c->J, 1, c->mask_v.p, c->dinv_v.p);
}

// how the matrix-free Jacobian action runs: 0 = L product, element kernel, node gather; 1 = element kernel, then
// the L product sums its node-sorted vectors (one GPU, triangles, stencil dictionary); 2 = k_jac_lattice, everything
// in one launch (lattice mesh in rectangle_mesh numbering, gradient-form viscosity, no rotating frame)
// Partitioned strips (round 4): the local mesh of a rank is a lattice of its own (own cell rows + the ghost row), so
// path 2 runs there as well -- after ONE halo exchange of the input; rows of ghost nodes come out as zeros (mask
// value 2).  Path 1 stays single-context (its node-sorted buffer has no interior / halo split).
// explicit_rotation (the IMEX right-hand side): a rotating frame does not enter the operator, the lattice path stays
static int jacobian_path(nsfem_ctx* c, bool explicit_rotation) {
  if (c->mesh.dim != 2 || cc_of(c) == 0.0 || !c->L.dict_ready) return 0;
  if (!c->mesh.cl.tried && c->L.dict && c->L.dict->lat_w > 0) {
    build_cell_lattice(c->h_p2map.data(), c->mesh.n_cells, c->L.dict->lat_w, c->L.dict->lat_h, c->mesh.cl);
    check_uniform_geometry(c->stream, c->mesh);
  }
  if (!c->traction_form && (explicit_rotation || coriolis_gamma(c) == 0.0) && c->mask_v.p &&
      jacobian_lattice_available(c->mesh, c->L))
    return 2;
  return c->distributed() ? 0 : 1;
}

// ghost lattice lines of the P2 lattice of a strip (looked at once; -1: the ghost nodes are not whole lines)
static void strip_ghost_lines(nsfem_ctx* c) {
  if (c->p2_gh_lo != -2) return;
  int lo, hi;
  const bool lines = c->L.dict && ghost_lattice_lines(c->h_ghost_p2, c->L.dict->lat_w, c->L.dict->lat_h, lo, hi);
  c->p2_gh_lo = lines ? lo : -1;
  c->p2_gh_hi = lines ? hi : -1;
}

void nsfem_ctx::MomentumMF::apply(hipStream_t s, const double* x, double* y) {
  const int64_t nv = nvel(c);
  const int dim = c->mesh.dim;
  // (partitioned: the halo exchange of x runs under the interior rows of the L product; the
  // element kernel of the convection action below reads the ghost nodes and comes after it)
  // identity rows on the Dirichlet dofs and zero ghost rows come out of the L product itself
  // (row mask, MASK_IDENTITY); every later contribution leaves the flagged rows untouched
  (void)nv;
  const double cc = cc_of(c);
  // one GPU, triangles, lattice mesh: the element kernel of the convection action first, then ONE launch of the
  // dictionary kernel forms L x AND sums the node-sorted element vectors (no separate node gather, y is written
  // once instead of written, read and written again)
  const int path = (dim == 2 && cc != 0.0 && c->L.dict_ready) ? jacobian_path(c) : 0;
  if (path != 0) {
    nsfem_ctx::Probe& pr = c->conv_probe;
    const bool timed = pr.on && pr.n + 2 <= pr.ev.size();
    // lattice meshes: element kernel, node sums and L product in one launch (k_jac_lattice)
    if (path == 2) {
      // strips: the ghost lines of the input first -- under the tile rows that read none of them when the overlap
      // mode is on and the strip is high enough; the kernel writes zeros to the ghost rows
      if (c->distributed()) {
        strip_ghost_lines(c);
        if (c->comm->overlap && c->p2_gh_lo >= 0 && jacobian_lattice_split(c->mesh, c->p2_gh_lo, c->p2_gh_hi)) {
          c->comm->exchange_begin(s, c->halo_p2, const_cast<double*>(x), dim);
          bool ok = launch_jacobian_lattice(s, c->mesh, c->L, c->state[vel_slot].p, x, cc, c->conv_form, c->picard,
                                            c->mask_v.p, y, 1, c->p2_gh_lo, c->p2_gh_hi);
          c->comm->exchange_end(s);
          ok = ok && launch_jacobian_lattice(s, c->mesh, c->L, c->state[vel_slot].p, x, cc, c->conv_form, c->picard,
                                             c->mask_v.p, y, 2, c->p2_gh_lo, c->p2_gh_hi);
          NSFEM_REQUIRE(ok, "one-launch Jacobian action: tile-row split failed");
          ++c->jac_lattice_launches;
          return;
        }
        c->comm->exchange(s, c->halo_p2, const_cast<double*>(x), dim);
      }
      if (timed) NSFEM_HIP(hipEventRecord(pr.ev[pr.n], s));
      if (launch_jacobian_lattice(s, c->mesh, c->L, c->state[vel_slot].p, x, cc, c->conv_form, c->picard,
                                  c->mask_v.p, y)) {
        ++c->jac_lattice_launches;
        if (timed) {
          NSFEM_HIP(hipEventRecord(pr.ev[pr.n + 1], s));
          pr.n += 2;
        }
        return;
      }
    }
    if (!c->distributed()) {
      if (timed) NSFEM_HIP(hipEventRecord(pr.ev[pr.n], s));
      launch_convection_cells(s, c->mesh, c->state[vel_slot].p, x, cc, c->conv_form, c->picard);
      if (timed) {
        NSFEM_HIP(hipEventRecord(pr.ev[pr.n + 1], s));
        pr.n += 2;
      }
      if (launch_spmv_with_gather(s, c->L, dim, x, y, c->mask_v.p, MASK_IDENTITY, c->mesh.nptr.p, c->mesh.rbuf.p)) {
        if (c->traction_form) launch_spmv_axpy(s, c->E, 1, c->coef[2], x, y, c->mask_v.p);
        const double g = coriolis_gamma(c);
        if (g != 0.0) coriolis_apply(c, g, x, y, c->mask_v.p);
        return;
      }
      // (no dictionary kernel: product, then the gather below re-runs the cheap element kernel)
    }
  }
  product_with_halo(c->distributed() ? c->comm : nullptr, &c->halo_p2, dim, s, x, c->L.pat,
                    [&](int phase) { launch_spmv(s, c->L, dim, x, y, c->mask_v.p, MASK_IDENTITY, 0, phase, 1); });
  if (c->traction_form) launch_spmv_axpy(s, c->E, 1, c->coef[2], x, y, c->mask_v.p);
  if (cc != 0.0) {
    nsfem_ctx::Probe& pr = c->conv_probe;
    const bool timed = pr.on && pr.n + 2 <= pr.ev.size();
    if (timed) NSFEM_HIP(hipEventRecord(pr.ev[pr.n], s));
    launch_convection_action(s, c->mesh, c->state[vel_slot].p, x, cc, y, c->conv_form, c->picard,
                             c->mask_v.p);
    if (timed) {
      NSFEM_HIP(hipEventRecord(pr.ev[pr.n + 1], s));
      pr.n += 2;
    }
  }
  const double g = coriolis_gamma(c);
  if (g != 0.0) coriolis_apply(c, g, x, y, c->mask_v.p);
}

// 0 = auto = matrix-free: inside the fused step drivers the velocity Jacobian is applied as
// L x + c_c [d conv(u)/du] x by an element kernel (one thread per cell) instead of being
// assembled.  Measured: tetrahedra, n = 48: step 55 -> 29 ms (assembling the 3x3-block matrix cost
// more than the handful of products an inexact Newton step needs); triangles, n = 512:
// 9.3 -> 8.6 ms with inexact Newton, equal (16 ms) with rtol 1e-12 + exact Newton.
// 1 = always assemble (block CSR), 2 = always matrix-free.
static bool use_matrix_free(const nsfem_ctx* c, const nsfem_step_opts* o) {
  (void)c;
  return o->matrix_free != 1;
}

// J dx = b ; u* -= dx
// known_rhs_norm >= 0: |rhs_v|_2 as the caller has just evaluated it (the Newton residual norm): the solve starts
// without reading its start-up sums back
// rhs_dead: the caller recomputes rhs_v before anything reads it again (the Newton loops: momentum_residual follows);
// the solver may then use it as scratch.  Not so behind nsfem_solve: nsfem_get_rhs / nsfem_residual_norm may follow.
// defer_update: u* -= dx is left to the residual launch the caller runs next (momentum_residual with the frame)
static int momentum_solve_update(nsfem_ctx* c, const nsfem_krylov_opts& o, nsfem_solve_info& info,
                                 double known_rhs_norm = -1.0, bool rhs_dead = false, bool defer_update = false) {
  hipStream_t s = c->stream;
  LinOp op;
  op.A = &c->J;
  op.nv = 1;
  op.rowmask = c->mask_v.p;
  op.maskmode = MASK_IDENTITY;
  op.dinv = c->dinv_v.p;
  fill_linop(c, op, true);
  if (c->mf_active) {               // matrix-free Jacobian (the step driver skipped the assembly)
    c->mom_mf.c = c;
    c->mom_mf.n = nvel(c);
    c->mom_mf.vel_slot = NSFEM_USTAR;
    op.custom = &c->mom_mf;
    if (o.precond != 1) launch_inv_diag(s, c->L, c->mesh.dim, c->mask_v.p, c->dinv_v.p);
  }
  if (o.precond == 1) {
    NSFEM_REQUIRE(c->mg_built, "multigrid requested but no hierarchy was set (nsfem_mg_finalize)");
    mg_refresh(c, true);
    op.prec = &c->mom_prec;
  }
  op.graph_epoch = c->graph_epoch;
  op.x_zero = true;                 // (dx_v is not read: the first update of the solve writes it)
  op.known_bnorm = known_rhs_norm;
  op.b_scratch = rhs_dead;
  int rc = bicgstab(s, c->kw, op, c->rhs_v.p, c->dx_v.p, o, info);
  if (rc != NSFEM_OK) return rc;
  if (defer_update) {
    c->newton_update_pending = true;
    return NSFEM_OK;
  }
  double* u = c->state[NSFEM_USTAR].p;
  launch_axpby(s, nvel(c), 1.0, u, -1.0, c->dx_v.p, u);
  return NSFEM_OK;
}

// rhs = A_p p_old - alpha0/k D u* ; start vector p = p_old with Dirichlet values
static void poisson_assemble(nsfem_ctx* c, bool extrapolate = false) {
  hipStream_t s = c->stream;
  const int64_t np = npre(c);
  launch_spmv(s, c->Ap, 1, c->state[NSFEM_P_OLD].p, c->rhs_p.p, nullptr, MASK_NONE);
  launch_spmv(s, c->Dv, 1, c->state[NSFEM_USTAR].p, c->tmp_p.p, nullptr, MASK_NONE);
  launch_axpby(s, np, 1.0, c->rhs_p.p, -c->alpha[0] / c->k, c->tmp_p.p, c->rhs_p.p);
  if (c->ghost_p.p) launch_zero_ghost(s, np, c->mask_p.p, c->rhs_p.p);
  if (extrapolate && c->pressure_history >= 2)       // start vector 2 p_n - p_(n-1)
    launch_axpby(s, np, 2.0, c->state[NSFEM_P_OLD].p, -1.0, c->state[NSFEM_P2_OLD].p, c->state[NSFEM_P].p);
  else
    NSFEM_HIP(hipMemcpyAsync(c->state[NSFEM_P].p, c->state[NSFEM_P_OLD].p, sizeof(double) * np,
                             hipMemcpyDeviceToDevice, s));
  launch_set_values(s, c->nbc_p, c->bc_p_dofs.p, c->bc_p_vals.p, c->state[NSFEM_P].p);
  if (!c->dinv_p_ready) {
    launch_inv_diag(s, c->Ap, 1, c->mask_p.p, c->dinv_p.p);
    c->dinv_p_ready = true;
  }
}

// is the pressure pinned by a Dirichlet value ANYWHERE?  On partitioned meshes a rank may hold
// none of the outlet nodes (unstructured partitions): all ranks must take the same branch in the
// solver (mean projection of the singular problem = an all-reduce), so the flag is all-reduced
// once after every nsfem_set_dirichlet(PRESSURE) -- which every rank calls, if only with n = 0.
static bool pressure_pinned_anywhere(nsfem_ctx* c) {
  if (!c->distributed()) return c->nbc_p > 0;
  if (c->bc_p_any < 0) {
    hipStream_t s = c->stream;
    c->kw.ensure(nvel(c));
    double* parts = c->kw.parts.p;
    double v = c->nbc_p > 0 ? 1.0 : 0.0;
    NSFEM_HIP(hipMemcpyAsync(parts, &v, sizeof(double), hipMemcpyHostToDevice, s));
    c->comm->allreduce_max(s, parts, 1);
    NSFEM_HIP(hipMemcpyAsync(&v, parts, sizeof(double), hipMemcpyDeviceToHost, s));
    NSFEM_HIP(hipStreamSynchronize(s));
    c->bc_p_any = v > 0.5 ? 1 : 0;
  }
  return c->bc_p_any > 0;
}

// Projection step by fast diagonalisation (precond = 3; tensor-product lattices, Dirichlet conditions on whole sides):
// x += A^+ (b - A x), then the residual is checked -- the direct solve is exact up to round-off, so ONE pass and one
// device -> host round trip; further passes (iterative refinement) only if the check fails.
static int poisson_solve_fast_diag(nsfem_ctx* c, const nsfem_krylov_opts& o, nsfem_solve_info& info) {
  hipStream_t s = c->stream;
  const int64_t np = npre(c);
  // (one-rank factors of the whole pressure space; 3D box lattices: exact factors only -- inexact ones precondition
  // CG, poisson_solve)
  FastDiagBase* fd = c->fast_diag();
  NSFEM_REQUIRE(fd && fd->exact && fd->fits(np, np, false),
                "fast diagonalisation requested but no factors were set (nsfem_poisson_set_fast_diag)");
  ++fd->solves;
  NSFEM_REQUIRE(!c->distributed(), "fast diagonalisation: one rank only");
  KrylovWork& w = c->kw;
  w.ensure(std::max<int64_t>(np, nvel(c)));
  ++w.touch;
  double* parts = w.parts.p;
  double* x = c->state[NSFEM_P].p;
  const double* rhs = c->rhs_p.p;
  if (!pressure_pinned_anywhere(c)) {
    // singular (all-Neumann) operator: make the right-hand side compatible, as the CG path does
    NSFEM_HIP(hipMemcpyAsync(w.t.p, rhs, sizeof(double) * np, hipMemcpyDeviceToDevice, s));
    launch_sum_sub_mean(s, np, w.t.p, parts + 10 * kParts);
    rhs = w.t.p;
  }
  constexpr int PR = 10, PB0 = 13;
  launch_dot(s, np, rhs, rhs, parts + PB0 * kParts);
  info.iterations = 0;
  info.converged = 0;
  double bnorm = 0.0, target = 0.0;
  launch_residual(s, c->Ap, 1, x, rhs, w.r.p, c->mask_p.p, MASK_ZERO);
  for (int pass = 0; pass < std::max(1, std::min(o.max_iter, 8)); ++pass) {
    fd->apply(s, w.r.p, w.z.p);
    launch_axpby(s, np, 1.0, x, 1.0, w.z.p, x);
    ++info.iterations;
    // the residual of the corrected iterate (the next pass's right-hand side)
    launch_residual(s, c->Ap, 1, x, rhs, w.r.p, c->mask_p.p, MASK_ZERO);
    launch_dot(s, np, w.r.p, w.r.p, parts + PR * kParts);
    double rr, bb;
    host_sum_parts2(s, w, PR, PB0, rr, bb);
    bnorm = std::sqrt(bb);
    target = std::max(o.atol, o.rtol * (bnorm > 0.0 ? bnorm : 1.0));
    w.last_target = target;
    if (!std::isfinite(rr)) return NSFEM_ERR_BREAKDOWN;
    info.residual = std::sqrt(rr);
    if (pass == 0) info.residual0 = info.residual;
    if (info.residual <= target) { info.converged = 1; break; }
  }
  return info.converged ? NSFEM_OK : NSFEM_ERR_NOT_CONVERGED;
}

// The whole projection step of the fused driver by fast diagonalisation, for the pure Neumann problem (no pressure
// Dirichlet dofs, one rank): with the start vector p_old the residual of  A p = A p_old - (alpha0 / k) D u*  is
// -(alpha0 / k) D u*  itself -- no product with A to form a right-hand side, none for a start residual:
//   r = -(alpha0 / k) D u* - mean ;  z = A^+ r ;  p = p_old + z ;  check |r - A z| <= max(atol, rtol |r|)
// (the same p as the assembled system gives, up to the constant and round-off; |r| <= |rhs| makes the check the
// stricter one).  Further passes refine (never needed so far: the direct solve leaves ~1e-14 |r|).
static int poisson_direct_step(nsfem_ctx* c, const nsfem_krylov_opts& o, nsfem_solve_info& info) {
  hipStream_t s = c->stream;
  const int64_t np = npre(c);
  KrylovWork& w = c->kw;
  w.ensure(std::max<int64_t>(np, nvel(c)));
  ++w.touch;
  double* parts = w.parts.p;
  constexpr int PR = 10, PB0 = 13;
  // Partitioned strips / slabs: the same solve with ONE collective (FastDiagBase::apply on partitioned factors).
  // u* carries valid ghost values (every Krylov solve fills the ghosts of its solution), so D u* is complete on the
  // owned rows; ghost rows are zeroed (every node counts once in the sums over the ranks); z comes back on every local
  // row, ghost lines / planes included, so p = p_old + z needs no halo exchange and the check r - A z none either.
  const bool dist = c->distributed();
  const uint8_t* gm = dist ? c->mask_p.p : nullptr;                            // (flag 2 on ghost rows)
  FastDiagBase& fd = *c->fast_diag();           // (the caller checked fast_diag_direct())
  NSFEM_REQUIRE(!dist || (fd.partitioned() && gm),
                "fast diagonalisation on a partitioned mesh: strip or slab factors not set");
  ++fd.solves;
  launch_spmv_scaled(s, c->Dv, 1, -c->alpha[0] / c->k, c->state[NSFEM_USTAR].p, w.r.p);
  if (dist) {
    launch_zero_ghost(s, np, gm, w.r.p);
    launch_sum(s, np, w.r.p, parts + PR * kParts);
    c->comm->allreduce_sum(s, parts + PR * kParts, kParts);
    launch_sub_mean(s, np, c->n_p1_global, parts + PR * kParts, w.r.p);
    launch_zero_ghost(s, np, gm, w.r.p);
  } else if (c->step_fused) {
    launch_sum_sub_mean_dot(s, np, w.r.p, parts + PR * kParts, parts + PB0 * kParts);   // (|r|^2 with the subtraction)
  } else {
    launch_sum_sub_mean(s, np, w.r.p, parts + PR * kParts);
  }
  if (dist || !c->step_fused) launch_dot(s, np, w.r.p, w.r.p, parts + PB0 * kParts);
  const double* base = c->state[NSFEM_P_OLD].p;
  // (local names for the two work vectors: refinement alternates them without permuting the KrylovWork buffers,
  // whose pointers the captured graphs of the other solvers hold)
  double* r = w.r.p;
  double* q = w.q.p;
  info.iterations = 0;
  info.converged = 0;
  for (int pass = 0; pass < std::max(1, std::min(o.max_iter, 8)); ++pass) {
    fd.apply(s, r, w.z.p);                                                     // (partitioned factors: a collective)
    // fused step frame, first pass on one rank: p = p_old + z is stored by the check's launch q = r - A z
    if (c->step_fused && !dist && pass == 0 &&
        launch_residual_sum(s, c->Ap, w.z.p, r, q, base, c->state[NSFEM_P].p)) {
      ++c->step_frame_launches[3];
    } else {
      launch_axpby(s, np, 1.0, base, 1.0, w.z.p, c->state[NSFEM_P].p);        // p = p_old + z (later passes: p += z)
      launch_residual(s, c->Ap, 1, w.z.p, r, q, gm, gm ? MASK_ZERO : MASK_NONE);    // q = r - A z
    }
    base = c->state[NSFEM_P].p;
    ++info.iterations;
    launch_dot(s, np, q, q, parts + PR * kParts);
    // (slots 10 ... 13 in the first pass, |r|^2 included; afterwards slot PB0 already holds the global sum)
    if (dist) c->comm->allreduce_sum(s, parts + PR * kParts, (pass == 0 ? PB0 - PR + 1 : 1) * kParts);
    double qq, rr;
    host_sum_parts2(s, w, PR, PB0, qq, rr);
    if (!std::isfinite(qq)) return NSFEM_ERR_BREAKDOWN;
    const double rnorm = std::sqrt(rr);
    const double target = std::max(o.atol, o.rtol * (rnorm > 0.0 ? rnorm : 1.0));
    w.last_target = target;
    info.residual = std::sqrt(qq);
    if (pass == 0) info.residual0 = rnorm;
    if (info.residual <= target) { info.converged = 1; break; }
    std::swap(r, q);                                                           // refine: the residual is the next right-hand side
  }
  return info.converged ? NSFEM_OK : NSFEM_ERR_NOT_CONVERGED;
}

static int poisson_solve(nsfem_ctx* c, const nsfem_krylov_opts& o, nsfem_solve_info& info) {
  // (3D box lattices with inexact factors: CG preconditioned by T^+ below)
  FastDiagBase* fd = c->fast_diag();
  const bool box_pcg = o.precond == 3 && fd && !fd->exact;
  if (o.precond == 3 && !box_pcg) return poisson_solve_fast_diag(c, o, info);
  LinOp op;
  op.A = &c->Ap;
  op.nv = 1;
  op.rowmask = c->mask_p.p;
  op.maskmode = MASK_ZERO;
  op.dinv = c->dinv_p.p;
  fill_linop(c, op, false);
  if (o.precond == 1) {
    NSFEM_REQUIRE(c->mg_built, "multigrid requested but no hierarchy was set (nsfem_mg_finalize)");
    mg_refresh(c, false);
    op.prec = &c->mg_p;
  }
  if (box_pcg) {
    // (slab factors: T^+ is a collective with valid ghost planes in z; the CG iteration itself exchanges halos)
    NSFEM_REQUIRE(fd->fits(npre(c), c->n_p1_global, c->distributed()),
                  "fast diagonalisation (3D): factors do not fit the pressure space");
    op.prec = fd;
    ++fd->solves;
  }
  op.graph_epoch = c->graph_epoch;
  return pcg(c->stream, c->kw, op, c->rhs_p.p, c->state[NSFEM_P].p, o, info, !pressure_pinned_anywhere(c));
}

// rhs = M u* - k/alpha0 G (p - p_old) ; start vector u0 = u* with Dirichlet values
// with_start_residual (fused step, one rank, Chebyshev mass solve): the start residual of the solve and the two sums
// its convergence check needs come out of the same pass as the right-hand side (k_correction_setup): r0 in kw.r,
// |r0|^2 and |rhs|^2 in the partial-sum slots 12, 13
// defer_finish (correction_step: the Chebyshev solve has a predicted step count and runs the lattice kernel): the fused
// step frame -- ONE pair launch forms rhs and r0 without writing p - p_old or G (p - p_old); U0 and the two sums are
// left to k_correction_finish after the solve's first sequence (cor_finish_pending)
static void correction_assemble(nsfem_ctx* c, bool with_start_residual = false, bool defer_finish = false) {
  hipStream_t s = c->stream;
  const int64_t nv = nvel(c), np = npre(c);
  c->cor_finish_pending = false;
  if (defer_finish && with_start_residual && c->step_fused && !c->distributed() && c->mask_v.p && !c->ghost_v.p &&
      c->mesh.dim == 2 && c->dinv_m_ready && (ensure_div_dicts(c), spmv_pair_available(c->M2, c->Gr))) {
    c->kw.ensure(nv);
    launch_spmv_pair_correction(s, c->M2, c->Gr, c->state[NSFEM_USTAR].p, -c->k / c->alpha[0], c->state[NSFEM_P].p,
                                c->state[NSFEM_P_OLD].p, c->mask_v.p, c->rhs_v.p, c->kw.r.p);
    ++c->step_frame_launches[1];
    c->cor_start_ready = true;
    c->cor_start_touch = ++c->kw.touch;
    c->cor_finish_pending = true;
    return;
  }
  launch_spmv(s, c->M2, c->mesh.dim, c->state[NSFEM_USTAR].p, c->rhs_v.p, nullptr, MASK_NONE);
  launch_axpby(s, np, 1.0, c->state[NSFEM_P].p, -1.0, c->state[NSFEM_P_OLD].p, c->tmp_p.p);
  launch_spmv(s, c->Gr, 1, c->tmp_p.p, c->tmp_v.p, nullptr, MASK_NONE);
  c->cor_start_ready = false;
  if (with_start_residual && !c->distributed() && c->mask_v.p) {
    c->kw.ensure(nv);
    launch_correction_setup(s, nv, -c->k / c->alpha[0], c->rhs_v.p, c->tmp_v.p, c->mask_v.p, c->kw.r.p,
                            c->kw.parts.p + 12 * kParts, c->kw.parts.p + 13 * kParts);
    c->cor_start_ready = true;
    c->cor_start_touch = ++c->kw.touch;
  } else {
    launch_axpby(s, nv, 1.0, c->rhs_v.p, -c->k / c->alpha[0], c->tmp_v.p, c->rhs_v.p);
  }
  if (c->ghost_v.p) launch_zero_ghost(s, nv, c->mask_v.p, c->rhs_v.p);
  NSFEM_HIP(hipMemcpyAsync(c->state[NSFEM_U0].p, c->state[NSFEM_USTAR].p, sizeof(double) * nv,
                           hipMemcpyDeviceToDevice, s));
  launch_set_values(s, c->nbc_v, c->bc_v_dofs.p, c->bc_v_vals.p, c->state[NSFEM_U0].p);
  if (!c->dinv_m_ready) {
    ++c->mass_dinv_epoch;
    launch_inv_diag(s, c->M2, c->mesh.dim, c->mask_v.p, c->dinv_m.p);
    c->dinv_m_ready = true;
  }
}

// Chebyshev iteration on the Jacobi-scaled velocity mass matrix with A-PRIORI spectral bounds
// (Wathen's element bounds, p2_mass_jacobi_bounds): no dot products, every iteration is ONE
// launch of the fused smoother kernel, and on partitioned meshes no all-reduce at all inside
// the iteration.  Solves the correction equation  M e = b - M x0  (e vanishes on the Dirichlet
// dofs), then x0 += e; the residual norm is checked after the predicted number of steps.
static int correction_solve_chebyshev(nsfem_ctx* c, const nsfem_krylov_opts& o, nsfem_solve_info& info) {
  hipStream_t s = c->stream;
  const int64_t nv = nvel(c);
  Multigrid& mg = c->mg_mv;
  if (mg.lv.empty()) {
    double lmin, lmax;
    p2_mass_jacobi_bounds(c->mesh.dim, lmin, lmax);
    mg.nv = c->mesh.dim;
    mg.coarse_dense_max = 0;
    mg.smoother_only = true;
    mg.lv.resize(1);
    mg.lv[0].A = &c->M2;
    mg.lv[0].n = c->mesh.n_p2;
    mg.lv[0].mask = c->mask_v.p;
    if (c->distributed()) {
      mg.comm = c->comm;
      mg.lv[0].halo = c->halo_p2;
      mg.lv[0].has_halo = true;
    }
    mg.setup_work(s);
    c->mass_dinv_copied_epoch = -1;            // (fresh work vectors)
    // interval [0.98 lmin, 1.02 lmax] in the parametrisation of Multigrid::cheb_coeffs
    c->mass_kappa = (1.02 * lmax) / (0.98 * lmin);
    mg.eig_ratio = c->mass_kappa;
    mg.lv[0].lmax = 1.02 * lmax / 1.05;
  }
  MGLevel& L = mg.lv[0];
  if (c->mass_dinv_copied_epoch != c->mass_dinv_epoch) {       // (once per change of the Dirichlet set, not per solve)
    NSFEM_HIP(hipMemcpyAsync(L.dinv.p, c->dinv_m.p, sizeof(double) * nv, hipMemcpyDeviceToDevice, s));
    c->mass_dinv_copied_epoch = c->mass_dinv_epoch;
  }
  KrylovWork& w = c->kw;
  w.ensure(nv);
  double* x = c->state[NSFEM_U0].p;
  double* parts = w.parts.p;
  auto residual_norm = [&](double* r, int slot = P10) {
    if (c->distributed()) c->comm->exchange(s, c->halo_p2, x, c->mesh.dim);
    launch_residual(s, c->M2, c->mesh.dim, x, c->rhs_v.p, r, c->mask_v.p, MASK_ZERO);
    launch_dot(s, nv, r, r, parts + slot * kParts);
  };
  // The a-priori step count is a worst-case bound; the same solve one time step ago tells what was actually needed
  // (first_check = its count, reduced by next_hint's linear-convergence estimate when it overshot): the first
  // sequence runs that many steps, the bound takes over if the residual check then fails.  With such a prediction
  // (one rank) the start-up sums |r0|^2, |b|^2 are not read back before the sequence: they wait in their own slots
  // and come with the residual check after it -- one device -> host round trip per solve instead of two.
  int k_hint = o.first_check >= 1 ? o.first_check : 0;
  // (correction_assemble left r0 in w.r and the sums in slots 12, 13 -- and no other solver has run since)
  const bool start_ready = c->cor_start_ready && c->cor_start_touch == w.touch;
  c->cor_start_ready = false;
  ++w.touch;
  const bool deferred = (k_hint > 0 || start_ready) && !c->distributed();
  constexpr int PR0 = 12, PB0 = 13;
  // fused step frame: correction_assemble left U0 and the sums of slots 12, 13 to the launch after the first sequence
  bool finish = c->cor_finish_pending;
  c->cor_finish_pending = false;
  if (finish && !(start_ready && k_hint > 0 && o.max_iter > 0 && !c->distributed() && mg.lattice_ok(L))) {
    // (not the sequence the assembly counted on: supply them now, the way the unfused assembly does)
    finish = false;
    NSFEM_HIP(hipMemcpyAsync(x, c->state[NSFEM_USTAR].p, sizeof(double) * nv, hipMemcpyDeviceToDevice, s));
    launch_set_values(s, c->nbc_v, c->bc_v_dofs.p, c->bc_v_vals.p, x);
    launch_dot(s, nv, w.r.p, w.r.p, parts + PR0 * kParts);
    launch_dot(s, nv, c->rhs_v.p, c->rhs_v.p, parts + PB0 * kParts);
  }
  if (!start_ready) {
    residual_norm(w.r.p, deferred ? PR0 : P10);
    launch_dot(s, nv, c->rhs_v.p, c->rhs_v.p, parts + (deferred ? PB0 : P10 + 1) * kParts);
  }
  if (c->distributed()) c->comm->allreduce_sum(s, parts + P10 * kParts, 2 * kParts);
  double rr0 = 0.0, bb0 = 0.0, r0 = 0.0, bnorm = 0.0, target = 0.0;
  if (!deferred) {
    host_sum_parts2(s, w, P10, P10 + 1, rr0, bb0);
    r0 = std::sqrt(rr0);
    bnorm = std::sqrt(bb0);
    target = std::max(o.atol, o.rtol * (bnorm > 0.0 ? bnorm : 1.0));
    w.last_target = target;
  }
  info.residual0 = info.residual = r0;
  info.iterations = 0;
  info.converged = deferred ? false : r0 <= target;
  const double sk = std::sqrt(c->mass_kappa);
  const double rate = std::log((sk + 1.0) / (sk - 1.0));
  double res = r0;
  bool first_pass = true;
  while (!info.converged && info.iterations < o.max_iter) {
    // steps needed for the error bound 2 sqrt(kappa) ((sqrt(kappa)-1)/(sqrt(kappa)+1))^k <= target / res
    int k = (deferred && first_pass && k_hint > 0) ? k_hint : 0;
    if (k == 0 && deferred && first_pass) {
      // no prediction yet (first step): the start sums are read now after all
      double rr_, bb_;
      host_sum_parts2(s, w, PR0, PB0, rr_, bb_);
      r0 = res = std::sqrt(rr_);
      bnorm = std::sqrt(bb_);
      target = std::max(o.atol, o.rtol * (bnorm > 0.0 ? bnorm : 1.0));
      w.last_target = target;
      info.residual0 = info.residual = r0;
      if (r0 <= target) { info.converged = 1; break; }
    }
    if (k == 0) k = (int)std::ceil(std::log(2.0 * sk * res / target) / rate);
    if (k_hint > 0) k = std::min(k, k_hint);
    k_hint = 0;
    k = std::max(1, std::min(k, o.max_iter - info.iterations));
    if (!c->distributed() && mg.lattice_ok(L)) {
      // lattice kernel: the residual of the correction equation r - M e (= rhs - M (x + e)) rides along in the last
      // launch of the sequence -- no separate product with M for the check
      mg.smooth_lattice(s, L, w.r.p, nullptr, w.q.p, k, false, w.t.p);
      if (finish && first_pass) {
        // U0 = u* + e, |r|^2 and the two start sums in one launch (r0 now lies in the buffer renamed w.t)
        info.iterations += k;
        std::swap(w.r.p, w.t.p);
        launch_correction_finish(s, nv, c->state[NSFEM_USTAR].p, w.q.p, x, w.r.p, w.t.p, c->rhs_v.p,
                                 parts + P10 * kParts, parts + PR0 * kParts, parts + PB0 * kParts);
        launch_set_values(s, c->nbc_v, c->bc_v_dofs.p, c->bc_v_vals.p, x);
        ++c->step_frame_launches[2];
      } else {
        launch_axpby(s, nv, 1.0, x, 1.0, w.q.p, x);
        info.iterations += k;
        std::swap(w.r.p, w.t.p);
        launch_dot(s, nv, w.r.p, w.r.p, parts + P10 * kParts);
      }
    } else {
      mg.smooth(s, L, w.r.p, nullptr, w.q.p, k);                       // e ~ M^{-1} r
      launch_axpby(s, nv, 1.0, x, 1.0, w.q.p, x);                      // x += e (e = 0 on Dirichlet dofs)
      info.iterations += k;
      residual_norm(w.r.p);
    }
    if (c->distributed()) c->comm->allreduce_sum(s, parts + P10 * kParts, kParts);
    if (deferred && first_pass) {
      double rr;
      host_sum_parts3(s, w, P10, PR0, PB0, rr, rr0, bb0);
      r0 = std::sqrt(rr0);
      bnorm = std::sqrt(bb0);
      target = std::max(o.atol, o.rtol * (bnorm > 0.0 ? bnorm : 1.0));
      w.last_target = target;
      info.residual0 = r0;
      res = std::sqrt(rr);
    } else {
      res = std::sqrt(host_sum_parts(s, w, P10));
    }
    first_pass = false;
    if (!std::isfinite(res)) return NSFEM_ERR_BREAKDOWN;
    info.residual = res;
    info.converged = res <= target;
  }
  return info.converged ? NSFEM_OK : NSFEM_ERR_NOT_CONVERGED;
}

static int correction_solve(nsfem_ctx* c, const nsfem_krylov_opts& o, nsfem_solve_info& info) {
  if (o.precond == 2) return correction_solve_chebyshev(c, o, info);
  LinOp op;
  op.A = &c->M2;
  op.nv = c->mesh.dim;
  op.rowmask = c->mask_v.p;
  op.maskmode = MASK_ZERO;
  op.dinv = c->dinv_m.p;
  fill_linop(c, op, true);
  return pcg(c->stream, c->kw, op, c->rhs_v.p, c->state[NSFEM_U0].p, o, info, false);
}

// ------------------------------------------------------- assembly seam + solve
static void monolithic_assemble(nsfem_ctx* ctx, uint32_t flags);
static int monolithic_solve(nsfem_ctx* ctx, const nsfem_krylov_opts& o, nsfem_solve_info& inf);

extern "C" int nsfem_assemble(nsfem_ctx* ctx, int system, uint32_t flags) {
  API_BEGIN
  NSFEM_REQUIRE(ctx, "null context");
  switch (system) {
    case NSFEM_SYS_MOMENTUM:
      if (flags & 1u) momentum_begin_step(ctx);
      (void)momentum_residual(ctx);
      momentum_jacobian(ctx);
      break;
    case NSFEM_SYS_POISSON:
      poisson_assemble(ctx);
      break;
    case NSFEM_SYS_CORRECTION:
      correction_assemble(ctx, true);      // (the same pass as the fused driver: its Chebyshev solve may start from it)
      break;
    case NSFEM_SYS_MONOLITHIC:
      monolithic_assemble(ctx, flags);
      break;
    default:
      throw Error(NSFEM_ERR_ARG, "nsfem_assemble: system not available");
  }
  ctx->assembled_system = system;
  NSFEM_HIP(hipStreamSynchronize(ctx->stream));
  API_END(ctx)
}

extern "C" int nsfem_residual_norm(nsfem_ctx* ctx, int system, double* out) {
  API_BEGIN
  NSFEM_REQUIRE(ctx && out, "null argument");
  NSFEM_REQUIRE(system == ctx->assembled_system, "system not assembled");
  const bool vel = (system != NSFEM_SYS_POISSON), mixed = (system == NSFEM_SYS_MONOLITHIC);
  const double* b = mixed ? ctx->rhs_m.p : vel ? ctx->rhs_v.p : ctx->rhs_p.p;
  const int64_t n = mixed ? nvel(ctx) + npre(ctx) : vel ? nvel(ctx) : npre(ctx);
  *out = global_norm(ctx, n, const_cast<double*>(b), nullptr);
  API_END(ctx)
}

extern "C" int nsfem_get_rhs(nsfem_ctx* ctx, int system, double* host, int64_t n) {
  API_BEGIN
  NSFEM_REQUIRE(ctx && host, "null argument");
  const bool vel = (system != NSFEM_SYS_POISSON), mixed = (system == NSFEM_SYS_MONOLITHIC);
  NSFEM_REQUIRE(n == (mixed ? nvel(ctx) + npre(ctx) : vel ? nvel(ctx) : npre(ctx)), "bad size");
  NSFEM_REQUIRE(!mixed || ctx->rhs_m.p, "system not assembled");
  NSFEM_HIP(hipMemcpyAsync(host, mixed ? ctx->rhs_m.p : vel ? ctx->rhs_v.p : ctx->rhs_p.p, sizeof(double) * n,
                           hipMemcpyDeviceToHost, ctx->stream));
  NSFEM_HIP(hipStreamSynchronize(ctx->stream));
  API_END(ctx)
}

// Every host convergence check of a Krylov solve is a device -> host round trip during which the
// GPU runs dry.  The same solve of the previous time step is an excellent predictor of the
// iteration count: the first check is postponed to one iteration before that count.
// Round 4: a check costs ~15 - 20 us of idle GPU, an iteration too many costs the iteration.  While the count is
// steady (the last two solves needed exactly the prediction) the first check sits AT the predicted count -- one round
// trip per solve --, otherwise and at every 8th solve (the probe that notices a falling count) one iteration before
// it.  exact: the prediction itself (the Chebyshev mass solve runs exactly that many steps before its only check).
static nsfem_krylov_opts hinted(nsfem_krylov_opts k, const nsfem_ctx::SolveHint& h, bool exact = false) {
  const bool steady = h.same >= 2 && (h.count & 7) != 7;
  k.first_check = std::max(k.first_check, (exact || steady) ? h.its : h.its - 1);
  return k;
}
// The predictor for the next solve: the iteration count of this one, reduced when the postponed
// first check found the residual far below the target (linear-convergence estimate of the count
// that would have sufficed) -- otherwise a single long solve would keep all later ones long.
static int next_hint(const nsfem_solve_info& si, const nsfem_krylov_opts& k, double target) {
  (void)k;
  if (!si.converged) return 0;                     // a failed solve predicts nothing
  if (si.iterations <= 1 || !(si.residual > 0.0) || !(si.residual0 > si.residual)) return si.iterations;
  // (target: the solve's own absolute target max(atol, rtol |b|) -- with a good start vector |r0| << |b|)
  if (!(si.residual < target) || !(si.residual0 > target)) return si.iterations;
  const double need = si.iterations * std::log(si.residual0 / target) / std::log(si.residual0 / si.residual);
  return std::max(1, std::min(si.iterations, (int)std::ceil(need)));
}
static void note_solve(nsfem_ctx::SolveHint& h, const nsfem_solve_info& si, const nsfem_krylov_opts& k, double target) {
  const int next = next_hint(si, k, target);
  h.same = (si.converged && next == h.its && si.iterations == h.its) ? h.same + 1 : 0;
  h.its = next;
  ++h.count;
}
// Krylov tolerances of one Newton linear solve.  newton_forcing = 0: the caller's tolerances
// (a direct solver's accuracy, as the reference's LU).  newton_forcing = eta > 0 (inexact
// Newton): reduce the linear residual by eta, but never below a tenth of what the nonlinear
// criterion itself asks for -- the Newton loop still terminates on the reference's criterion,
// evaluated on the true nonlinear residual.
static nsfem_krylov_opts forced_opts(const nsfem_step_opts* o, const nsfem_krylov_opts& base, double r0) {
  nsfem_krylov_opts k = base;
  if (o->newton_forcing > 0.0) {
    k.rtol = std::max(k.rtol, o->newton_forcing);
    k.atol = std::max(k.atol, 0.1 * std::max(o->newton_atol, o->newton_rtol * r0));
  }
  return k;
}

extern "C" int nsfem_solve(nsfem_ctx* ctx, int system, const nsfem_krylov_opts* opts,
                           nsfem_solve_info* info) {
  nsfem_solve_info local;
  API_BEGIN
  NSFEM_REQUIRE(ctx && opts, "null argument");
  NSFEM_REQUIRE(system == ctx->assembled_system, "system not assembled");
  nsfem_solve_info& inf = info ? *info : local;
  int rc = NSFEM_OK;
  switch (system) {
    case NSFEM_SYS_MOMENTUM: rc = momentum_solve_update(ctx, *opts, inf); break;
    case NSFEM_SYS_POISSON: rc = poisson_solve(ctx, *opts, inf); break;
    case NSFEM_SYS_CORRECTION:
      // (the Chebyshev mass solve takes its step count from the previous solve: the same predictor as in the fused
      // step drivers, so that the explicit seam and the fused step stay bit for bit equal)
      rc = correction_solve(ctx, hinted(*opts, ctx->hint_cor, opts->precond == 2), inf);
      note_solve(ctx->hint_cor, inf, *opts, ctx->kw.last_target);
      break;
    case NSFEM_SYS_MONOLITHIC: rc = monolithic_solve(ctx, *opts, inf); break;
    default: throw Error(NSFEM_ERR_ARG, "nsfem_solve: system not available");
  }
  if (rc == NSFEM_ERR_BREAKDOWN) throw Error(rc, "Krylov breakdown");
  if (rc == NSFEM_ERR_NOT_CONVERGED) throw Error(rc, "Krylov solver did not converge");
  API_END(ctx)
}

// mesh arrays, pattern and the P1 stiffness / mass matrices of one coarse level (same space
// dimension as the fine mesh)
static void fill_p1_level(nsfem_ctx* ctx, nsfem_ctx::P1Level* lv, int n_vertices, int nc,
                          const double* coords, const int32_t* cells,
                          const int32_t* dofmap = nullptr, int n_dofs = 0) {
  hipStream_t s = ctx->stream;
  const int dim = ctx->mesh.dim, nl1 = dim + 1;
  // numbering of the P1 space: vertex ids, or (periodic levels) the given cell dof map -- the
  // geometry always comes from the vertex coordinates of the cells
  const int32_t* dm = dofmap ? dofmap : cells;
  const int n = dofmap ? n_dofs : n_vertices;
  NSFEM_REQUIRE(n > 0 && n <= n_vertices, "bad number of coarse dofs");
  lv->n = n;
  std::vector<double> vx((size_t)nl1 * dim * nc);
  std::vector<int32_t> p1((size_t)nl1 * nc);
  for (int c = 0; c < nc; ++c)
    for (int v = 0; v < nl1; ++v) {
      const int vid = cells[(size_t)c * nl1 + v];
      NSFEM_REQUIRE(vid >= 0 && vid < n_vertices, "coarse cell vertex id out of range");
      const int dof = dm[(size_t)c * nl1 + v];
      NSFEM_REQUIRE(dof >= 0 && dof < n, "coarse cell dof id out of range");
      p1[(size_t)v * nc + c] = dof;
      for (int k = 0; k < dim; ++k) vx[(size_t)(dim * v + k) * nc + c] = coords[(size_t)vid * dim + k];
    }
  lv->mesh.dim = dim;
  lv->mesh.n_cells = nc;
  lv->mesh.n_p1 = n;
  lv->mesh.n_vertices = n_vertices;
  lv->mesh.vx.upload(vx, s);
  lv->mesh.p1.upload(p1, s);
  HostPattern h;
  build_pattern(n, n, nc, dm, nl1, dm, nl1, true, h);
  upload_pattern(s, h, lv->pat, true);
  lv->K.init(&lv->pat, 1, 1, s);
  lv->M.init(&lv->pat, 1, 1, s);
  lv->Lc.init(&lv->pat, 1, 1, s);
  launch_assemble_p1_scalar(s, lv->mesh, lv->pat, lv->K.vals.p, lv->M.vals.p);
  // lattice levels: stencil dictionary of the level's operators (smoothing steps of both hierarchies;
  // the multi-step lattice kernel needs it)
  if (build_stencil_dict(s, lv->pat, lv->M.vals.p, lv->K.vals.p, lv->dict))
    lv->K.dict = lv->M.dict = lv->Lc.dict = &lv->dict;
  lv->K.sell_update(s);
  lv->M.sell_update(s);
}

extern "C" int nsfem_mg_add_level(nsfem_ctx* ctx, const nsfem_mg_level_desc* d) {
  API_BEGIN
  NSFEM_REQUIRE(ctx && d, "null argument");
  NSFEM_REQUIRE(!ctx->mg_built, "hierarchy already finalized");
  NSFEM_REQUIRE(d->n_vertices > 0 && d->n_cells > 0 && d->coords && d->cells && d->p_rowptr &&
                    d->p_col && d->p_val, "bad level description");
  const int n_fine = ctx->coarse.empty() ? ctx->mesh.n_p1 : ctx->coarse.back()->n;
  NSFEM_REQUIRE(d->n_fine == n_fine, "prolongation rows must match the previous level");
  hipStream_t s = ctx->stream;
  nsfem_ctx::P1Level* lv = new nsfem_ctx::P1Level();
  ctx->coarse.push_back(lv);
  fill_p1_level(ctx, lv, d->n_vertices, d->n_cells, d->coords, d->cells, d->dofmap, d->n_dofs);
  NSFEM_REQUIRE(d->transfer_kind >= 0 && d->transfer_kind <= 2, "transfer_kind: 0 (from the values), 1 nested, 2 interpolation");
  lv->to_finer.build(s, n_fine, lv->n, d->p_rowptr, d->p_col, d->p_val, d->transfer_kind);
  if (d->ghost) {                       // one flag per dof of the level (= per vertex without a dof map)
    lv->h_ghost.assign(d->ghost, d->ghost + lv->n);
    lv->halo = to_halo(d->halo);
    lv->has_halo = true;
    mark_interior_blocks(lv->pat, lv->h_ghost);
  }
  NSFEM_HIP(hipStreamSynchronize(s));
  API_END(ctx)
}

// Algebraic pressure Laplacian of the Schur-complement preconditioner, level by level (level 0 =
// fine P1 space): A_L = D_f diag(M_v)^{-1} D_f^T and its Galerkin coarsenings, computed by the
// host at set-up.  Replaces the geometric stiffness matrices in the mg_s hierarchy: the algebraic
// form carries the correct behaviour on open (natural-outflow) boundaries, where a strongly
// imposed Dirichlet condition leaves one badly preconditioned mode per outflow node.
extern "C" int nsfem_mg_set_schur_operator(nsfem_ctx* ctx, int level, int32_t n,
                                           const int32_t* rowptr, const int32_t* col,
                                           const double* val, int singular) {
  API_BEGIN
  NSFEM_REQUIRE(ctx && rowptr && col && val, "null argument");
  ctx->schur_singular = singular ? 1 : 0;
  NSFEM_REQUIRE(ctx->mg_built, "build the hierarchy first (nsfem_mg_finalize)");
  NSFEM_REQUIRE(level >= 0 && level < (int)ctx->mg_s.lv.size(), "no such level");
  NSFEM_REQUIRE(n == ctx->mg_s.lv[level].n, "operator size does not match the level");
  hipStream_t s = ctx->stream;
  if (ctx->schur_ops.size() < ctx->mg_s.lv.size()) ctx->schur_ops.resize(ctx->mg_s.lv.size());
  nsfem_ctx::CsrOp*& op = ctx->schur_ops[level];
  delete op;
  op = new nsfem_ctx::CsrOp();
  Pattern& p = op->pat;
  p.n_rows = p.n_cols = n;
  p.nnz = rowptr[n];
  p.h_rowptr.assign(rowptr, rowptr + n + 1);
  p.h_col.assign(col, col + p.nnz);
  std::vector<int32_t> diag((size_t)n, -1);
  for (int r = 0; r < n; ++r)
    for (int k = rowptr[r]; k < rowptr[r + 1]; ++k) {
      NSFEM_REQUIRE(col[k] >= 0 && col[k] < n, "column out of range");
      if (col[k] == r) diag[r] = k;
    }
  for (int r = 0; r < n; ++r) NSFEM_REQUIRE(diag[r] >= 0, "operator without a stored diagonal");
  p.rowptr.upload(p.h_rowptr, s);
  p.col.upload(p.h_col, s);
  p.diag.upload(diag, s);
  build_rowblocks(p, s);
  op->mat.pat = &p;
  op->mat.br = op->mat.bc = 1;
  op->mat.vals.upload(val, (size_t)p.nnz, s);
  NSFEM_HIP(hipStreamSynchronize(s));
  if (build_stencil_dict(s, p, op->mat.vals.p, nullptr, op->dict)) op->mat.dict = &op->dict;
  op->mat.sell_update(s);
  NSFEM_HIP(hipStreamSynchronize(s));
  ctx->mg_s.lv[level].A = &op->mat;
  ctx->mg_s.lv[level].additive = ctx->schur_additive;
  ctx->mg_s_dirty = true;
  API_END(ctx)
}

// Partitioned meshes: the operators handed to nsfem_mg_set_schur_operator AFTER this call are the
// rank's additive parts A_r = D_r W_r D_r^T (W_r: 1 / M_v,jj on the velocity dofs this rank owns,
// 0 elsewhere), ghost rows included; the hierarchy applies them with a forward halo exchange of
// the input and a reverse (add) exchange of the ghost rows of the product.
extern "C" int nsfem_mg_set_schur_mode(nsfem_ctx* ctx, int additive) {
  API_BEGIN
  NSFEM_REQUIRE(ctx, "null argument");
  ctx->schur_additive = additive != 0;
  API_END(ctx)
}

// max (op = 1) or sum (op = 0) over the ranks of `count` host doubles (set-up-time agreement on
// flags and bounds; single contexts: a no-op)
extern "C" int nsfem_comm_allreduce(nsfem_ctx* ctx, double* values, int count, int op) {
  API_BEGIN
  NSFEM_REQUIRE(ctx && values && count > 0 && count <= 1024, "bad argument");
  if (ctx->distributed()) {
    hipStream_t s = ctx->stream;
    DevBuf<double> tmp;
    tmp.upload(values, (size_t)count, s);
    if (op) ctx->comm->allreduce_max(s, tmp.p, count);
    else ctx->comm->allreduce_sum(s, tmp.p, count);
    NSFEM_HIP(hipMemcpyAsync(values, tmp.p, sizeof(double) * count, hipMemcpyDeviceToHost, s));
    NSFEM_HIP(hipStreamSynchronize(s));
  }
  API_END(ctx)
}

// replicated global coarsest mesh of a partitioned hierarchy; `offset` = global id of this
// rank's local coarsest node 0
extern "C" int nsfem_mg_set_global_coarse(nsfem_ctx* ctx, int32_t n_vertices, int32_t n_cells,
                                          const double* coords, const int32_t* cells,
                                          int64_t offset) {
  API_BEGIN
  NSFEM_REQUIRE(ctx && coords && cells && n_vertices > 0 && n_cells > 0, "bad argument");
  NSFEM_REQUIRE(!ctx->mg_built, "hierarchy already finalized");
  hipStream_t s = ctx->stream;
  delete ctx->global_coarse;
  nsfem_ctx::P1Level* lv = ctx->global_coarse = new nsfem_ctx::P1Level();
  fill_p1_level(ctx, lv, n_vertices, n_cells, coords, cells);
  ctx->glob_off = offset;
  NSFEM_HIP(hipStreamSynchronize(s));
  API_END(ctx)
}

// a coarser level of the REPLICATED global hierarchy below the mesh of nsfem_mg_set_global_coarse
// (finest first; prolongation rows = nodes of the previous global level)
extern "C" int nsfem_mg_add_global_level(nsfem_ctx* ctx, const nsfem_mg_level_desc* d) {
  API_BEGIN
  NSFEM_REQUIRE(ctx && d, "null argument");
  NSFEM_REQUIRE(!ctx->mg_built, "hierarchy already finalized");
  NSFEM_REQUIRE(ctx->global_coarse, "set the global coarsest mesh first (nsfem_mg_set_global_coarse)");
  NSFEM_REQUIRE(d->n_vertices > 0 && d->n_cells > 0 && d->coords && d->cells && d->p_rowptr &&
                    d->p_col && d->p_val, "bad level description");
  const int n_fine = ctx->global_tail.empty() ? ctx->global_coarse->n : ctx->global_tail.back()->n;
  NSFEM_REQUIRE(d->n_fine == n_fine, "prolongation rows must match the previous global level");
  hipStream_t s = ctx->stream;
  nsfem_ctx::P1Level* lv = new nsfem_ctx::P1Level();
  ctx->global_tail.push_back(lv);
  fill_p1_level(ctx, lv, d->n_vertices, d->n_cells, d->coords, d->cells, d->dofmap, d->n_dofs);
  lv->to_finer.build(s, n_fine, lv->n, d->p_rowptr, d->p_col, d->p_val, d->transfer_kind);
  NSFEM_HIP(hipStreamSynchronize(s));
  API_END(ctx)
}

extern "C" int nsfem_mg_set_global_coarse_constrained(nsfem_ctx* ctx, int32_t n_vertices, int32_t n_cells,
                                                      const double* coords, const int32_t* cells,
                                                      const int32_t* dofmap, int32_t n_dofs,
                                                      int64_t offset) {
  API_BEGIN
  NSFEM_REQUIRE(ctx && coords && cells && dofmap && n_vertices > 0 && n_cells > 0 && n_dofs > 0, "bad argument");
  NSFEM_REQUIRE(!ctx->mg_built, "hierarchy already finalized");
  NSFEM_REQUIRE(!ctx->global_coarse, "global coarsest mesh already set");
  NSFEM_REQUIRE(offset >= 0 && offset < n_dofs, "offset outside the global coarsest space");
  nsfem_ctx::P1Level* lv = ctx->global_coarse = new nsfem_ctx::P1Level();
  fill_p1_level(ctx, lv, n_vertices, n_cells, coords, cells, dofmap, n_dofs);
  ctx->glob_off = offset;
  NSFEM_HIP(hipStreamSynchronize(ctx->stream));
  API_END(ctx)
}

// unstructured partitions: the local coarsest level maps into the global coarsest mesh through
// an index list instead of an offset
extern "C" int nsfem_mg_set_global_index(nsfem_ctx* ctx, int32_t n_local, const int32_t* local_to_global) {
  API_BEGIN
  NSFEM_REQUIRE(ctx && local_to_global && n_local > 0, "bad argument");
  NSFEM_REQUIRE(!ctx->mg_built, "hierarchy already finalized");
  NSFEM_REQUIRE(ctx->global_coarse, "set the global coarsest mesh first (nsfem_mg_set_global_coarse)");
  for (int i = 0; i < n_local; ++i)
    NSFEM_REQUIRE(local_to_global[i] >= 0 && local_to_global[i] < ctx->global_coarse->n, "global id out of range");
  ctx->h_glob_idx.assign(local_to_global, local_to_global + n_local);
  ctx->glob_idx.upload(ctx->h_glob_idx, ctx->stream);
  NSFEM_HIP(hipStreamSynchronize(ctx->stream));
  API_END(ctx)
}

// halo of an unstructured partition as index lists; target 0: P2 nodes, 1: P1 nodes of the
// context (after nsfem_set_partition), 2 + l: P1 nodes of multigrid level l (after its
// nsfem_mg_add_level); before nsfem_mg_finalize
extern "C" int nsfem_set_halo_lists(nsfem_ctx* ctx, int target, const nsfem_halo_lists* d) {
  API_BEGIN
  NSFEM_REQUIRE(ctx && d && d->n_neighbours >= 0, "bad argument");
  NSFEM_REQUIRE(!ctx->mg_built, "set the halo lists before nsfem_mg_finalize");
  int64_t n_nodes = 0;
  HaloRange* h = nullptr;
  if (target == 0) { h = &ctx->halo_p2; n_nodes = ctx->mesh.n_p2; }
  else if (target == 1) { h = &ctx->halo_p1; n_nodes = ctx->mesh.n_p1; }
  else {
    NSFEM_REQUIRE(target >= 2 && target - 2 < (int)ctx->coarse.size(), "no such multigrid level");
    h = &ctx->coarse[target - 2]->halo;
    n_nodes = ctx->coarse[target - 2]->n;
    ctx->coarse[target - 2]->has_halo = true;
  }
  HaloLists* L = new HaloLists();
  ctx->halo_lists.push_back(L);
  const int nn = d->n_neighbours;
  NSFEM_REQUIRE(nn == 0 || (d->neighbour && d->send_ptr && d->recv_ptr), "null list");
  L->nbr.assign(d->neighbour, d->neighbour + nn);
  L->send_ptr.assign(1, 0);
  L->recv_ptr.assign(1, 0);
  if (nn > 0) {
    L->send_ptr.assign(d->send_ptr, d->send_ptr + nn + 1);
    L->recv_ptr.assign(d->recv_ptr, d->recv_ptr + nn + 1);
  }
  NSFEM_REQUIRE(L->send_ptr[0] == 0 && L->recv_ptr[0] == 0, "list pointers start at 0");
  for (int k = 0; k < nn; ++k) {
    NSFEM_REQUIRE(L->nbr[k] >= 0 && L->send_ptr[k + 1] >= L->send_ptr[k] && L->recv_ptr[k + 1] >= L->recv_ptr[k],
                  "malformed halo lists");
  }
  for (int64_t i = 0; i < L->n_send(); ++i)
    NSFEM_REQUIRE(d->send_idx[i] >= 0 && d->send_idx[i] < n_nodes, "send index out of range");
  for (int64_t i = 0; i < L->n_recv(); ++i)
    NSFEM_REQUIRE(d->recv_idx[i] >= 0 && d->recv_idx[i] < n_nodes, "receive index out of range");
  if (L->n_send() > 0) L->send_idx.upload(d->send_idx, (size_t)L->n_send(), ctx->stream);
  if (L->n_recv() > 0) L->recv_idx.upload(d->recv_idx, (size_t)L->n_recv(), ctx->stream);
  NSFEM_HIP(hipStreamSynchronize(ctx->stream));
  *h = HaloRange();
  h->lists = L;
  ctx->mg_mv.lv.clear();
  API_END(ctx)
}

extern "C" int nsfem_set_partition(nsfem_ctx* ctx, const nsfem_partition_desc* d) {
  API_BEGIN
  NSFEM_REQUIRE(ctx && d && d->p2_ghost && d->p1_ghost, "null argument");
  NSFEM_REQUIRE(!ctx->mg_built, "set the partition before building the multigrid hierarchy");
  hipStream_t s = ctx->stream;
  const int n2 = ctx->mesh.n_p2, n1 = ctx->mesh.n_p1;
  ctx->h_ghost_p2.assign(d->p2_ghost, d->p2_ghost + n2);
  ctx->h_ghost_p1.assign(d->p1_ghost, d->p1_ghost + n1);
  std::vector<uint8_t> gv((size_t)ctx->mesh.dim * n2), gp((size_t)n1);
  for (int i = 0; i < n2; ++i)
    for (int a = 0; a < ctx->mesh.dim; ++a) gv[(size_t)ctx->mesh.dim * i + a] = d->p2_ghost[i] ? 2 : 0;
  for (int i = 0; i < n1; ++i) gp[i] = d->p1_ghost[i] ? 2 : 0;
  // (a single-rank "partition" has no ghosts: keep the ghost arrays unallocated, so that none of
  // the ghost-zeroing launches run)
  bool any_ghost = false;
  for (uint8_t g : gv) any_ghost |= g != 0;
  for (uint8_t g : gp) any_ghost |= g != 0;
  if (any_ghost) {
    ctx->ghost_v.upload(gv, s);
    ctx->ghost_p.upload(gp, s);
  }
  ctx->halo_p2 = to_halo(d->p2_halo);
  mark_interior_blocks(ctx->p22, ctx->h_ghost_p2);   // row blocks that can run under the halo exchange
  mark_interior_blocks(ctx->p11, ctx->h_ghost_p1);
  ctx->mg_mv.lv.clear();            // rebuilt with the halo on the next Chebyshev mass solve
  ctx->halo_p1 = to_halo(d->p1_halo);
  ctx->n_p2_global = d->n_p2_global;
  ctx->n_p1_global = d->n_p1_global;
  ctx->partition_periodic = d->periodic != 0;
  if (ctx->comm) ctx->comm->periodic = ctx->partition_periodic;
  // masks carry the ghost flag from now on
  launch_overlay_ghost(s, nvel(ctx), ctx->ghost_v.p, ctx->mask_v.p);
  launch_overlay_ghost(s, n1, ctx->ghost_p.p, ctx->mask_p.p);
  ctx->dinv_m_ready = ctx->dinv_p_ready = false;
  NSFEM_HIP(hipStreamSynchronize(s));
  API_END(ctx)
}

// A context's communicator is replaced: the old one goes before the new one is made (a rank holds one slot of its
// group / segment), the new one takes the context's settings.  (Nobody keeps a copy of ctx->comm across an attach:
// the fast-diagonalisation objects hold the address of the member.)
static void drop_comm(nsfem_ctx* ctx) {
  delete ctx->comm;
  ctx->comm = nullptr;
}
static void adopt_comm(nsfem_ctx* ctx, Comm* comm) {
  ctx->comm = comm;
  comm->periodic = ctx->partition_periodic;
  comm->overlap = ctx->overlap;
}

extern "C" int nsfem_comm_attach_local(nsfem_ctx* ctx, void* group, int rank) {
  API_BEGIN
  NSFEM_REQUIRE(ctx && group, "null argument");
  drop_comm(ctx);
  adopt_comm(ctx, make_local_comm(group, rank));
  API_END(ctx)
}

extern "C" int nsfem_comm_attach_rccl(nsfem_ctx* ctx, const char* id128, int rank, int size) {
  API_BEGIN
  NSFEM_REQUIRE(ctx && id128, "null argument");
  NSFEM_HIP(hipSetDevice(ctx->device));
  drop_comm(ctx);
  adopt_comm(ctx, make_rccl_comm(id128, rank, size));
  API_END(ctx)
}

extern "C" int nsfem_comm_attach_shm(nsfem_ctx* ctx, const char* name, int rank, int size, int64_t slot_bytes) {
  API_BEGIN
  NSFEM_REQUIRE(ctx && name, "null argument");
  NSFEM_HIP(hipSetDevice(ctx->device));
  drop_comm(ctx);
  adopt_comm(ctx, make_shm_comm(name, rank, size, slot_bytes));
  API_END(ctx)
}

// partitioned meshes: communicator, halo ranges and ghost flags of every level, and the
// replicated global coarsest operator.  `first_p1` = index of the fine P1 level in mg.lv.
static void wire_partition(nsfem_ctx* ctx, Multigrid& mg, size_t first_p1, bool momentum) {
  if (!ctx->distributed()) return;
  NSFEM_REQUIRE(ctx->global_coarse, "partitioned multigrid needs nsfem_mg_set_global_coarse");
  mg.comm = ctx->comm;
  if (first_p1 == 1) {
    mg.lv[0].halo = ctx->halo_p2;
    mg.lv[0].has_halo = true;
    mg.lv[0].h_ghost = &ctx->h_ghost_p2;
  }
  mg.lv[first_p1].halo = ctx->halo_p1;
  mg.lv[first_p1].has_halo = true;
  mg.lv[first_p1].h_ghost = &ctx->h_ghost_p1;
  for (size_t l = 0; l < ctx->coarse.size(); ++l) {
    nsfem_ctx::P1Level* c = ctx->coarse[l];
    NSFEM_REQUIRE(c->has_halo, "coarse level without partition data");
    mg.lv[first_p1 + 1 + l].halo = c->halo;
    mg.lv[first_p1 + 1 + l].has_halo = true;
    mg.lv[first_p1 + 1 + l].h_ghost = &c->h_ghost;
  }
  mg.globA = momentum ? &ctx->global_coarse->Lc : &ctx->global_coarse->K;
  mg.n_glob = ctx->global_coarse->n;
  mg.glob_off = ctx->glob_off;
  if (!ctx->h_glob_idx.empty()) {
    NSFEM_REQUIRE((int)ctx->h_glob_idx.size() == mg.lv.back().n, "global index list does not match the coarsest level");
    mg.glob_idx = ctx->glob_idx.p;
    mg.h_glob_idx = &ctx->h_glob_idx;
  }
  if (!ctx->global_tail.empty()) {          // replicated hierarchy below the global coarse mesh
    Multigrid& t = momentum ? ctx->mg_v_tail : ctx->mg_p_tail;
    t.nv = mg.nv; t.degree = mg.degree; t.pre_degree = mg.pre_degree; t.eig_ratio = mg.eig_ratio;
    t.coarse_dense_max = mg.coarse_dense_max;
    t.comm = nullptr;
    t.own_mask0 = true;
    t.lv.clear();
    t.lv.resize(1 + ctx->global_tail.size());
    t.lv[0].A = mg.globA; t.lv[0].n = mg.n_glob;
    for (size_t l = 0; l < ctx->global_tail.size(); ++l) {
      nsfem_ctx::P1Level* c = ctx->global_tail[l];
      t.lv[l].P = &c->to_finer.P; t.lv[l].R = &c->to_finer.R; t.lv[l].h_inj = &c->to_finer.h_inj;
      t.lv[l].transfer = &c->to_finer;
      t.lv[l + 1].A = momentum ? &c->Lc : &c->K; t.lv[l + 1].n = c->n;
    }
    t.setup_work(ctx->stream);
    mg.tail = &t;
  }
  mg.glob_wrap = ctx->partition_periodic;
  NSFEM_REQUIRE(mg.glob_idx || (mg.glob_off >= 0 && (mg.glob_wrap || mg.glob_off + mg.lv.back().n <= mg.n_glob)),
                "local coarsest level does not fit into the global coarsest mesh");
}

extern "C" int nsfem_mg_finalize(nsfem_ctx* ctx, const nsfem_mg_opts* o) {
  API_BEGIN
  NSFEM_REQUIRE(ctx, "null context");
  NSFEM_REQUIRE(!ctx->mg_built, "hierarchy already finalized");
  hipStream_t s = ctx->stream;
  // P2 <- P1 on the fine mesh: identity at vertices, average at edge midpoints
  {
    const int n2 = ctx->mesh.n_p2, nc = ctx->mesh.n_cells;
    std::vector<int32_t> a((size_t)n2, -1), b((size_t)n2, -1);
    const int dim = ctx->mesh.dim, nl1 = dim + 1, nl2 = dim == 2 ? 6 : 10;
    const int ends2[3][2] = {{1, 2}, {0, 2}, {0, 1}};                               // UFC edges
    const int ends3[6][2] = {{2, 3}, {1, 3}, {1, 2}, {0, 3}, {0, 2}, {0, 1}};
    for (int c = 0; c < nc; ++c) {
      const int32_t* p2 = &ctx->h_p2map[(size_t)c * nl2];
      const int32_t* p1 = &ctx->h_p1map[(size_t)c * nl1];
      for (int v = 0; v < nl1; ++v) { a[p2[v]] = p1[v]; b[p2[v]] = -1; }
      for (int e = 0; e < nl2 - nl1; ++e) {
        const int e0 = dim == 2 ? ends2[e][0] : ends3[e][0], e1 = dim == 2 ? ends2[e][1] : ends3[e][1];
        a[p2[nl1 + e]] = std::min(p1[e0], p1[e1]);
        b[p2[nl1 + e]] = std::max(p1[e0], p1[e1]);
      }
    }
    std::vector<int32_t> rp((size_t)n2 + 1, 0), col;
    std::vector<double> val;
    for (int i = 0; i < n2; ++i) {
      NSFEM_REQUIRE(a[i] >= 0, "P2 node not referenced by any cell");
      if (b[i] < 0 || b[i] == a[i]) { col.push_back(a[i]); val.push_back(1.0); }
      else { col.push_back(a[i]); val.push_back(0.5); col.push_back(b[i]); val.push_back(0.5); }
      rp[i + 1] = (int32_t)col.size();
    }
    ctx->t_p2p1.build(s, n2, ctx->mesh.n_p1, rp.data(), col.data(), val.data(), 1 /* nested: P1 in P2 */);
  }
  ctx->Lc0.init(&ctx->p11, 1, 1, s);
  const int degree = (o && o->smoother_degree > 0) ? o->smoother_degree : 2;
  const double ratio = (o && o->eig_ratio > 1.0) ? o->eig_ratio : 4.0;
  const int dense_max = (o && o->coarse_dense_max > 0) ? o->coarse_dense_max : 1200;
  // pressure Poisson hierarchy: P1 fine -> coarse P1 levels
  {
    Multigrid& mg = ctx->mg_p;
    mg.nv = 1; mg.degree = degree; mg.eig_ratio = ratio; mg.coarse_dense_max = dense_max;
    mg.lv.clear();
    mg.lv.resize(1 + ctx->coarse.size());
    mg.lv[0].A = &ctx->Ap; mg.lv[0].n = ctx->mesh.n_p1; mg.lv[0].mask = ctx->mask_p.p;
    for (size_t l = 0; l < ctx->coarse.size(); ++l) {
      nsfem_ctx::P1Level* c = ctx->coarse[l];
      mg.lv[l].P = &c->to_finer.P; mg.lv[l].R = &c->to_finer.R; mg.lv[l].h_inj = &c->to_finer.h_inj;
      mg.lv[l].transfer = &c->to_finer;
      mg.lv[l + 1].A = &c->K; mg.lv[l + 1].n = c->n;
    }
    wire_partition(ctx, mg, 0, false);
    mg.setup_work(s);
  }
  // momentum hierarchy: P2 fine -> P1 fine -> coarse P1 levels, operator a M + b K
  {
    Multigrid& mg = ctx->mg_v;
    mg.nv = ctx->mesh.dim; mg.degree = degree; mg.eig_ratio = ratio; mg.coarse_dense_max = dense_max;
    // non-symmetric cycle V(0, degree+1): BiCGStab does not need a symmetric preconditioner, and
    // without pre-smoothing the fine residual is the input itself (two fine SpMVs fewer per
    // cycle; measured 6 % faster steps than V(2,2) at equal iteration counts)
    mg.pre_degree = 0;
    mg.degree = degree + 1;
    ctx->mg_v_symmetric = false;
    mg.identity_rows = true;     // z = r on Dirichlet rows, written by the last smoothing step
    mg.lv.clear();
    mg.lv.resize(2 + ctx->coarse.size());
    mg.lv[0].A = &ctx->L; mg.lv[0].n = ctx->mesh.n_p2; mg.lv[0].mask = ctx->mask_v.p;
    mg.lv[0].P = &ctx->t_p2p1.P; mg.lv[0].R = &ctx->t_p2p1.R; mg.lv[0].h_inj = &ctx->t_p2p1.h_inj;
    mg.lv[0].transfer = &ctx->t_p2p1;
    mg.lv[1].A = &ctx->Lc0; mg.lv[1].n = ctx->mesh.n_p1;
    for (size_t l = 0; l < ctx->coarse.size(); ++l) {
      nsfem_ctx::P1Level* c = ctx->coarse[l];
      mg.lv[l + 1].P = &c->to_finer.P; mg.lv[l + 1].R = &c->to_finer.R;
      mg.lv[l + 1].h_inj = &c->to_finer.h_inj;
      mg.lv[l + 1].transfer = &c->to_finer;
      mg.lv[l + 2].A = &c->Lc; mg.lv[l + 2].n = c->n;
    }
    wire_partition(ctx, mg, 1, true);
    mg.setup_work(s);
  }
  // Schur-complement pressure Laplacian (own Dirichlet set) and pressure mass smoother
  {
    if (!ctx->mask_s.p) { ctx->mask_s.alloc((size_t)npre(ctx)); ctx->mask_s.zero(s); }
    Multigrid& mg = ctx->mg_s;
    mg.nv = 1; mg.degree = degree; mg.eig_ratio = ratio; mg.coarse_dense_max = dense_max;
    mg.lv.clear();
    mg.lv.resize(1 + ctx->coarse.size());
    mg.lv[0].A = &ctx->Ap; mg.lv[0].n = ctx->mesh.n_p1; mg.lv[0].mask = ctx->mask_s.p;
    for (size_t l = 0; l < ctx->coarse.size(); ++l) {
      nsfem_ctx::P1Level* c = ctx->coarse[l];
      mg.lv[l].P = &c->to_finer.P; mg.lv[l].R = &c->to_finer.R; mg.lv[l].h_inj = &c->to_finer.h_inj;
      mg.lv[l].transfer = &c->to_finer;
      mg.lv[l + 1].A = &c->K; mg.lv[l + 1].n = c->n;
    }
    wire_partition(ctx, mg, 0, false);
    mg.setup_work(s);
    Multigrid& mm = ctx->mg_m;          // 4 Chebyshev-Jacobi steps on the P1 mass matrix
    mm.nv = 1; mm.coarse_dense_max = 0; mm.coarse_steps = 4; mm.eig_ratio = 8.0;
    mm.lv.clear();
    mm.lv.resize(1);
    mm.lv[0].A = &ctx->Mp; mm.lv[0].n = ctx->mesh.n_p1; mm.lv[0].mask = nullptr;
    mm.smoother_only = true;
    if (ctx->distributed()) {           // partitioned: halo exchange before every smoothing SpMV
      mm.comm = ctx->comm;
      mm.lv[0].halo = ctx->halo_p1;
      mm.lv[0].has_halo = true;
      mm.lv[0].h_ghost = &ctx->h_ghost_p1;
    }
    mm.setup_work(s);
  }
  ctx->mg_built = true;
  ctx->mg_p_dirty = ctx->mg_v_dirty = ctx->mg_s_dirty = true;
  ctx->L_dirty = true;       // (re)compute the coarse momentum operators
  NSFEM_HIP(hipStreamSynchronize(s));
  API_END(ctx)
}

// communication counters of this rank since the last reset: {all-reduce calls, all-reduce payload
// bytes, halo exchanges, halo bytes sent}
extern "C" int nsfem_comm_stats(nsfem_ctx* ctx, int64_t out[4], int reset) {
  API_BEGIN
  NSFEM_REQUIRE(ctx && out, "null argument");
  out[0] = out[1] = out[2] = out[3] = 0;
  if (ctx->comm) {
    out[0] = ctx->comm->n_allreduce; out[1] = ctx->comm->bytes_allreduce;
    out[2] = ctx->comm->n_exchange; out[3] = ctx->comm->bytes_exchange;
    if (!ctx->comm->hist.empty() && ctx->comm->rank == 0 && !reset) {
      static const char* kind[3] = {"all-reduce", "exchange", "reverse-add"};
      for (auto& e : ctx->comm->hist)
        std::fprintf(stderr, "[comm hist rank 0] %-11s %9lld B x %lld\n", kind[e.first.first], (long long)e.first.second,
                     (long long)e.second);
    }
    if (reset) {
      ctx->comm->n_allreduce = ctx->comm->bytes_allreduce = ctx->comm->n_exchange = ctx->comm->bytes_exchange = 0;
      ctx->comm->hist.clear();
    }
  }
  API_END(ctx)
}

// number of halo exchanges since the last reset that ran on the communicator's stream under the
// interior rows of the product consuming them (nsfem_set_overlap)
extern "C" int nsfem_comm_overlapped(nsfem_ctx* ctx, int64_t* out, int reset) {
  API_BEGIN
  NSFEM_REQUIRE(ctx && out, "null argument");
  *out = ctx->comm ? ctx->comm->n_overlapped : 0;
  if (reset && ctx->comm) ctx->comm->n_overlapped = 0;
  API_END(ctx)
}

// partitioned meshes: run the halo exchanges of the Krylov operators and of the smoothing steps on
// the communicator's own stream, concurrently with the row blocks that reference no ghost column
extern "C" int nsfem_set_overlap(nsfem_ctx* ctx, int enable) {
  API_BEGIN
  NSFEM_REQUIRE(ctx, "null context");
  if (ctx->comm) ctx->comm->overlap = enable != 0;
  ctx->overlap = enable != 0;
  ctx->graph_epoch++;
  API_END(ctx)
}

extern "C" int nsfem_mg_set_halo_mode(nsfem_ctx* ctx, int relaxed) {
  API_BEGIN
  NSFEM_REQUIRE(ctx, "null context");
  // (tried in round 3 and removed: a "local" mode without any exchange inside the velocity cycle -- smoothing,
  // residuals and transfers on the rank-local operator, ranks coupled through the global coarse problem only --
  // cut the exchanges of a strong-scaling step from 187 to 133 but tripled the BiCGStab count (5.2 -> 19.5 on 8
  // ranks, 960^2) and stalled the Poisson CG altogether: dropped interface contributions in the restriction)
  for (Multigrid* mg : {&ctx->mg_v, &ctx->mg_p, &ctx->mg_s, &ctx->mg_m}) mg->relaxed_halo = relaxed != 0;
  ctx->graph_epoch++;
  API_END(ctx)
}

extern "C" int nsfem_mg_set_truncation(nsfem_ctx* ctx, double max_ratio, double coarse_tol) {
  API_BEGIN
  NSFEM_REQUIRE(ctx, "null context");
  NSFEM_REQUIRE(max_ratio >= 0.0 && coarse_tol > 0.0 && coarse_tol < 1.0, "truncation parameters out of range");
  ctx->mg_trunc_ratio = max_ratio;
  ctx->mg_trunc_tol = coarse_tol;
  ctx->L_dirty = true;
  ctx->graph_epoch++;
  API_END(ctx)
}

extern "C" int nsfem_default_step_opts(nsfem_step_opts* o) {
  if (!o) return NSFEM_ERR_ARG;
  std::memset(o, 0, sizeof(*o));
  o->newton_atol = 1e-10;
  o->newton_rtol = 1e-9;
  o->newton_max_iter = 50;
  o->convective_form = 0;
  nsfem_krylov_opts k;
  k.rtol = 1e-12;
  k.atol = 1e-14;
  k.max_iter = 20000;
  k.precond = 0;
  k.check_every = 1;
  k.first_check = 0;
  o->momentum = k;
  o->poisson = k;
  o->correction = k;
  return NSFEM_OK;
}


// ---------------------------------------------------------------- parts the step calls share
// What every step call does first: the checks on its options, the graph epoch (captured Krylov bodies bake in the
// convective form and the Picard flag) and the cleared record of the step -- the caller's, or `local`
static nsfem_step_info& step_begin(nsfem_ctx* ctx, const nsfem_step_opts* opts, nsfem_step_info* info,
                                   nsfem_step_info& local, bool newton, bool picard) {
  NSFEM_REQUIRE(ctx && opts, "null argument");
  NSFEM_REQUIRE(opts->convective_form >= 0 && opts->convective_form <= 3, "unknown convective form");
  NSFEM_REQUIRE(!newton || (opts->newton_max_iter > 0 && opts->newton_max_iter < NSFEM_MAX_NEWTON),
                "newton_max_iter out of range");
  if (ctx->conv_form != opts->convective_form || ctx->picard != picard) ctx->graph_epoch++;
  ctx->conv_form = opts->convective_form;
  ctx->picard = picard;
  nsfem_step_info& inf = info ? *info : local;
  std::memset(&inf, 0, sizeof(inf));
  return inf;
}

// Newton iteration of the diffusion step and of the monolithic step (dolfin NewtonSolver: residual criterion,
// relaxation 1).  residual() evaluates the residual at the iterate and returns its norm; solve_update(r, k, si) solves
// the linearised system with the Krylov options k (r: the norm just evaluated), updates the iterate and returns the
// solver's status.  `where` names the step in the error messages.
template <class Residual, class SolveUpdate>
static void newton_solve(nsfem_ctx* ctx, const nsfem_step_opts* opts, nsfem_step_info& inf, const char* where,
                         bool allow_nonconvergence, Residual residual, SolveUpdate solve_update) {
  double r = residual();
  const double r0 = r;
  inf.newton_residuals[0] = r;
  int it = 0;
  bool converged = r < opts->newton_atol;
  ctx->mf_active = use_matrix_free(ctx, opts);
  while (!converged && it < opts->newton_max_iter) {
    nsfem_solve_info si;
    nsfem_ctx::SolveHint& hint = ctx->hint_mom[std::min(it, 3)];
    const nsfem_krylov_opts ko = forced_opts(opts, opts->momentum, r0);
    const int rc = solve_update(r, hinted(ko, hint), si);
    note_solve(hint, si, ko, ctx->kw.last_target);
    inf.krylov_iterations_momentum += si.iterations;
    if (rc == NSFEM_ERR_BREAKDOWN) throw Error(rc, std::string("BiCGStab breakdown in the ") + where);
    if (rc == NSFEM_ERR_NOT_CONVERGED) throw Error(rc, std::string("BiCGStab did not converge in the ") + where);
    ++it;
    r = residual();
    inf.newton_residuals[it] = r;
    if (!std::isfinite(r)) throw Error(NSFEM_ERR_BREAKDOWN, "Newton residual is not finite");
    converged = (r / r0 < opts->newton_rtol) || (r < opts->newton_atol);
  }
  inf.newton_iterations = it;
  inf.converged = converged ? 1 : 0;
  ctx->mf_active = false;
  ctx->picard = false;
  if (!converged && !allow_nonconvergence) throw Error(NSFEM_ERR_NOT_CONVERGED, "Newton solver did not converge");
}

// Projection step of the pressure-correction schemes (nsfem_step_ipcs, nsfem_step_imex)
static void projection_step(nsfem_ctx* ctx, const nsfem_step_opts* opts, nsfem_step_info& inf) {
  nsfem_solve_info si;
  int rc;
  // (every rank must take the same branch: the pressure Dirichlet set is judged globally)
  const bool fd = opts->poisson.precond == 3;
  NSFEM_REQUIRE(!fd || !ctx->distributed() || !pressure_pinned_anywhere(ctx),
                "fast diagonalisation on a partitioned mesh solves the pure Neumann projection step only "
                "(pressure Dirichlet nodes are set): use another Poisson preconditioner");
  // (3D box lattices: the pass-plus-check driver for exact factors; inexact ones assemble and run CG with T^+)
  if (fd && !pressure_pinned_anywhere(ctx) && ctx->fast_diag_direct()) {
    rc = poisson_direct_step(ctx, opts->poisson, si);
  } else {
    poisson_assemble(ctx, opts->pressure_extrapolation != 0);
    rc = poisson_solve(ctx, hinted(opts->poisson, ctx->hint_poi), si);
  }
  note_solve(ctx->hint_poi, si, opts->poisson, ctx->kw.last_target);
  inf.krylov_iterations_poisson = si.iterations;
  if (rc != NSFEM_OK) throw Error(rc, "CG failed in the projection step");
}

// Velocity correction step of the pressure-correction schemes
static void correction_step(nsfem_ctx* ctx, const nsfem_step_opts* opts, nsfem_step_info& inf) {
  const bool cheb = opts->correction.precond == 2;
  const nsfem_krylov_opts ko = hinted(opts->correction, ctx->hint_cor, cheb);
  // (the fused frame needs the solve to run a predicted number of steps in the lattice kernel before its only check;
  // the first steps, which read the start sums before the sequence, keep the present launches)
  const bool defer = cheb && ko.first_check >= 1 && ko.max_iter > 0 && !ctx->mg_mv.lv.empty() &&
                     ctx->mg_mv.lattice_ok(ctx->mg_mv.lv[0]);
  correction_assemble(ctx, cheb, defer);
  nsfem_solve_info si;
  int rc = correction_solve(ctx, ko, si);
  note_solve(ctx->hint_cor, si, opts->correction, ctx->kw.last_target);
  inf.krylov_iterations_correction = si.iterations;
  if (rc != NSFEM_OK) throw Error(rc, "CG failed in the velocity correction step");
}

extern "C" int nsfem_step_ipcs(nsfem_ctx* ctx, const nsfem_step_opts* opts, nsfem_step_info* info) {
  nsfem_step_info local;
  API_BEGIN
  nsfem_step_info& inf = step_begin(ctx, opts, info, local, true, false);
  NSFEM_REQUIRE(ctx->alpha[0] != 0.0, "the pressure-correction scheme needs alpha0 != 0");
  NSFEM_REQUIRE(ctx->visc.law == 0, "variable viscosity: only nsfem_step_imex takes a viscosity law (set law 0 first)");
  NSFEM_REQUIRE(ctx->bodies.cur.n == 0, "immersed bodies: only nsfem_step_imex takes bodies (remove them with n = 0 first)");
  NSFEM_REQUIRE(ctx->wm.dev.law == 0, "wall model: only nsfem_step_imex takes a wall model (switch it off with law 0 first)");
  NSFEM_REQUIRE(!ctx->imex_active, "IMEX coefficients are set (nsfem_set_imex): call nsfem_set_bdf or nsfem_step_imex");
  // ---- diffusion step: Newton
  momentum_begin_step(ctx);
  // (the residual evaluation that follows every solve applies the update the solve left pending)
  newton_solve(ctx, opts, inf, "diffusion step", false, [&] { return momentum_residual(ctx, true); },
               [&](double r, const nsfem_krylov_opts& k, nsfem_solve_info& si) {
                 if (!ctx->mf_active) momentum_jacobian(ctx);
                 return momentum_solve_update(ctx, k, si, r, true, newton_frame_available(ctx));
               });
  projection_step(ctx, opts, inf);
  correction_step(ctx, opts, inf);
  ctx->assembled_system = -1;
  API_END(ctx)
}


// ---------------------------------------------------------------- IMEX pressure correction
// the operators of the old levels in the right-hand side: L_i = alpha_i/k M + gamma_i c_v K, i = 1, 2 (built as
// ensure_L builds L; they share its pattern and stencil dictionary)
static void imex_build_ops(nsfem_ctx* c);
static void imex_agree_on_lattice(nsfem_ctx* c);
static void ensure_imex_ops(nsfem_ctx* c) {
  ensure_L(c);
  hipStream_t s = c->stream;
  if (!c->L1.vals.p) {
    c->L1.init(&c->p22, 1, 1, s);
    c->L2.init(&c->p22, 1, 1, s);
    c->imex_ops_dirty = true;
    c->imex_lattice_agreed = -1;
  }
  if (c->L1.dict != c->L.dict) {
    c->L1.dict = c->L2.dict = c->L.dict;
    c->imex_ops_dirty = true;
    c->imex_lattice_agreed = -1;
  }
  if (c->imex_ops_dirty) imex_build_ops(c);
  imex_agree_on_lattice(c);
}
static void imex_build_ops(nsfem_ctx* c) {
  hipStream_t s = c->stream;
  const double cv = c->coef[2];
  launch_scale_combine(s, c->p22.nnz, c->alpha[1] / c->k, c->M2.vals.p, c->imex_gamma[1] * cv, c->K2.vals.p, c->L1.vals.p);
  launch_scale_combine(s, c->p22.nnz, c->alpha[2] / c->k, c->M2.vals.p, c->imex_gamma[2] * cv, c->K2.vals.p, c->L2.vals.p);
  c->L1.sell_update(s);
  c->L2.sell_update(s);
  c->imex_ops_dirty = false;
}

// step-constant part of the right-hand side:  g = - c_p D^T p_old + M (- c_b f + c_e dOmega/dt x x) + traction
// (momentum_begin_step's signs; the Euler term only with nsfem_set_imex_rotation(1), from the value last given to
// nsfem_set_angular_velocity -- the convention of the body-force slot)
static void imex_begin_step(nsfem_ctx* c) {
  hipStream_t s = c->stream;
  const int64_t nv = nvel(c);
  ensure_div_dicts(c);
  // Boussinesq buoyancy (nsfem_set_scalar with b != 0): f_eff = f + T^{n+1} b in a work buffer takes the place of f
  const double* f = c->have_body_force ? c->state[NSFEM_BODY_FORCE].p : nullptr;
  if (c->sc.configured && c->sc.buoyant) {
    NSFEM_REQUIRE(std::isfinite(c->coef[3]), "buoyancy set but body_force_term coefficient is None");
    ensure_scalar_slot(c, NSFEM_T0);
    if (!c->sc.f_eff.p) c->sc.f_eff.alloc((size_t)nv);
    launch_buoyancy_force(s, c->mesh, f, c->state[NSFEM_T0].p, c->sc.b, c->sc.f_eff.p);
    f = c->sc.f_eff.p;
  }
  const bool euler = euler_active(c);
  if (f || euler) {
    if (f) {
      NSFEM_REQUIRE(std::isfinite(c->coef[3]), "body force set but body_force_term coefficient is None");
      launch_axpby(s, nv, -c->coef[3], f, 0.0, f, c->tmp_v.p);
    } else {
      c->tmp_v.zero(s);
    }
    if (euler) euler_add(c, c->tmp_v.p);
    launch_spmv(s, c->M2, c->mesh.dim, c->tmp_v.p, c->gconst.p, nullptr, MASK_NONE);
  } else {
    c->gconst.zero(s);
  }
  launch_spmv_axpy(s, c->DT, 1, -c->coef[1], c->state[NSFEM_P_OLD].p, c->gconst.p, nullptr);
  if (c->have_traction)
    launch_axpby(s, nv, 1.0, c->gconst.p, 1.0, c->state[NSFEM_TRACTION].p, c->gconst.p);
}

// does the one-launch right-hand side apply?  (uniform lattices only: graded ones keep the generic path.)  On a
// partitioned mesh the answer must be the same on every rank -- the two paths are different collective sequences when
// the overlap mode is on, and nsfem_imex_rhs(path 2) must fail everywhere or nowhere --, so the ranks' own answers
// are reduced ONCE (minimum), when the operators are built or something the answer depends on was set, and kept
static bool imex_lattice_local(nsfem_ctx* c) {
  return jacobian_path(c, true) == 2 && imex_rhs_lattice_available(c->mesh, c->L1, c->L2);
}
static void imex_agree_on_lattice(nsfem_ctx* c) {
  if (!c->distributed() || c->imex_lattice_agreed >= 0) return;
  hipStream_t s = c->stream;
  c->kw.ensure(nvel(c));
  double* parts = c->kw.parts.p + (size_t)P10 * kParts;
  double no = imex_lattice_local(c) ? 0.0 : 1.0;
  NSFEM_HIP(hipMemcpyAsync(parts, &no, sizeof(double), hipMemcpyHostToDevice, s));
  c->comm->allreduce_max(s, parts, 1);
  NSFEM_HIP(hipMemcpyAsync(&no, parts, sizeof(double), hipMemcpyDeviceToHost, s));
  NSFEM_HIP(hipStreamSynchronize(s));
  c->imex_lattice_agreed = no == 0.0 ? 1 : 0;
}
static bool imex_lattice_ok(nsfem_ctx* c) {
  return c->distributed() ? c->imex_lattice_agreed == 1 : imex_lattice_local(c);
}

// partitioned meshes: the right-hand side reads the ghost entries of u1 and u2.  After a step they are copies of the
// owners' values to round-off only, so u1 is exchanged before every right-hand side.  u2 is the u1 of the step before
// (nsfem_advance rotates the pointers): its ghosts are the bit copies that exchange left, unless the slot was written
// since (nsfem_set_state, the first step) -- then both levels travel in ONE message of 2 dim values per node, before
// anything reads them.  true: u1 has travelled
static bool imex_exchange_stale_levels(nsfem_ctx* c) {
  if (!c->distributed() || c->u2_ghost_fresh) return false;
  hipStream_t s = c->stream;
  const int dim = c->mesh.dim;
  const int64_t n = c->mesh.n_p2;
  if (!c->imex_pack.p) c->imex_pack.alloc((size_t)(2 * nvel(c)));
  double *u1 = c->state[NSFEM_U1].p, *u2 = c->state[NSFEM_U2].p;
  launch_halo_pack2(s, n, c->halo_p2, dim, u1, u2, c->imex_pack.p);
  c->comm->exchange(s, c->halo_p2, c->imex_pack.p, 2 * dim);
  launch_halo_unpack2(s, n, c->halo_p2, dim, c->imex_pack.p, u1, u2);
  c->u1_ghost_fresh = c->u2_ghost_fresh = true;
  return true;
}

// rhs = -[ L1 u1 + L2 u2 (+ c_v E (g1 u1 + g2 u2)) + g + (b0 n1 + b1 n2) ],  n1 = c_c conv(u1) -> `n1`;
// n2 (null: not read, b1 = 0) = c_c conv(u2).  path: 0 the one-launch kernel where it applies, 1 generic, 2 one-launch
// or error.  The generic sequence below DEFINES the summation order; k_jac_lattice<FORM, 3> reproduces it.
// Partitioned meshes: ONE halo exchange (u1; `u1_travelled`: imex_exchange_stale_levels has sent it with u2), rows of
// ghost nodes come out as zeros in rhs and n1 on both paths, the arithmetic on owned rows is the single context's.
// gam (null: no rotation): 2 c_cor Omega(t^n); the element kernel of either path adds M (gam x u1) to n1 -- no launch
// and no exchange of its own.
static int imex_rhs(nsfem_ctx* c, int path, const double* n2, double* n1, double* rhs, bool u1_travelled = false,
                    const double* gam = nullptr) {
  hipStream_t s = c->stream;
  const int64_t nv = nvel(c);
  const double cc = cc_of(c);
  double* u1 = c->state[NSFEM_U1].p;
  const double* u2 = c->state[NSFEM_U2].p;
  const double b0 = c->imex_beta[0], b1 = c->imex_beta[1];
  const int dim = c->mesh.dim;
  const bool dist = c->distributed();
  bool need_u1 = dist && !u1_travelled;
  if (path != 1 && imex_lattice_ok(c)) {
    const uint8_t* gm = dist ? c->mask_v.p : nullptr;
    auto launch = [&](int phase) {
      return launch_imex_rhs_lattice(s, c->mesh, c->L1, c->L2, u1, u2, c->gconst.p, cc, c->conv_form, b0, b1, n2, n1,
                                     rhs, gm, phase, c->p2_gh_lo, c->p2_gh_hi, gam ? gam[0] : 0.0);
    };
    if (need_u1) {
      // the tile rows that read no ghost line run under the exchange when the overlap mode is on and the strip is
      // high enough (as the Jacobian action, MomentumMF::apply)
      strip_ghost_lines(c);
      need_u1 = false;
      c->u1_ghost_fresh = true;
      if (c->comm->overlap && c->p2_gh_lo >= 0 && jacobian_lattice_split(c->mesh, c->p2_gh_lo, c->p2_gh_hi)) {
        c->comm->exchange_begin(s, c->halo_p2, u1, dim);
        bool ok = launch(1);
        c->comm->exchange_end(s);
        ok = ok && launch(2);
        NSFEM_REQUIRE(ok, "one-launch IMEX right-hand side: tile-row split failed");
        return 2;
      }
      c->comm->exchange(s, c->halo_p2, u1, dim);
    }
    if (launch(0)) return 2;
    // (the ranks agreed on this path: falling back here would leave them in different collective sequences)
    NSFEM_REQUIRE(!dist, "one-launch IMEX right-hand side: launch failed on a rank of a partitioned mesh");
  }
  NSFEM_REQUIRE(path != 2, "one-launch IMEX right-hand side: not available on this mesh / these settings");
  if (need_u1) {
    product_with_halo(c->comm, &c->halo_p2, dim, s, u1, c->L1.pat,
                      [&](int phase) { launch_spmv(s, c->L1, dim, u1, rhs, nullptr, MASK_NONE, 0, phase); });
    c->u1_ghost_fresh = true;
  } else {
    launch_spmv(s, c->L1, dim, u1, rhs, nullptr, MASK_NONE);
  }
  launch_spmv(s, c->L2, dim, u2, c->tmp_v.p, nullptr, MASK_NONE);
  launch_axpby(s, nv, 1.0, rhs, 1.0, c->tmp_v.p, rhs);
  if (c->traction_form) {
    launch_spmv_axpy(s, c->E, 1, c->imex_gamma[1] * c->coef[2], u1, rhs, nullptr);
    launch_spmv_axpy(s, c->E, 1, c->imex_gamma[2] * c->coef[2], u2, rhs, nullptr);
  }
  launch_axpby(s, nv, 1.0, rhs, 1.0, c->gconst.p, rhs);
  NSFEM_HIP(hipMemsetAsync(n1, 0, sizeof(double) * nv, s));
  if (cc != 0.0 || gam) launch_convection_residual(s, c->mesh, u1, cc, n1, c->conv_form, gam);
  launch_imex_combine(s, nv, rhs, n1, n2, b0, b1, rhs);
  if (dist && c->ghost_v.p) {
    launch_zero_ghost(s, nv, c->mask_v.p, rhs);
    launch_zero_ghost(s, nv, c->mask_v.p, n1);
  }
  return 1;
}

// ---- dynamic Smagorinsky (law 8): host side of the Germano-Lilly procedure (kernels: assembly.hip)
// group-sorted vertex list of the averaging groups: gvert ascending within a group, goff the offsets.  group null: one
// group of all vertices
static void dynamic_upload_groups(nsfem_ctx* c, int n_groups, const int32_t* group) {
  nsfem_ctx::Dynamic& D = c->dyn;
  const int nv = c->mesh.n_p1;
  std::vector<int32_t> goff((size_t)n_groups + 1, 0), gvert((size_t)nv);
  for (int v = 0; v < nv; ++v) ++goff[(size_t)(group ? group[v] : 0) + 1];
  for (int g = 0; g < n_groups; ++g) goff[(size_t)g + 1] += goff[g];
  std::vector<int32_t> fill(goff.begin(), goff.end() - 1);
  for (int v = 0; v < nv; ++v) gvert[(size_t)fill[group ? group[v] : 0]++] = v;
  D.goff.upload(goff, c->stream);
  D.gvert.upload(gvert, c->stream);
  if (D.buf.sums.n != (size_t)n_groups * 3) D.buf.sums.alloc((size_t)n_groups * 3);
  D.n_groups = n_groups;
  D.global = group == nullptr;
  if (group) D.h_group.assign(group, group + nv);
  else D.h_group.clear();
}

// mom, vert and the vertex field of one use of the procedure, once; sums follows the group count
static void dynamic_alloc(nsfem_ctx* c, nsfem_ctx::DynamicBuffers& B, bool with_T) {
  const MeshDev& m = c->mesh;
  if (!B.allocated) {
    B.mom.alloc((size_t)dynamic_moment_rows(m.dim, with_T) * m.n_cells);
    B.vert.alloc((size_t)m.n_p1 * 3);
    B.field.alloc((size_t)m.n_p1);
    B.allocated = true;
  }
  if (B.sums.n != (size_t)c->dyn.n_groups * 3) B.sums.alloc((size_t)c->dyn.n_groups * 3);
}

// the buffers of law 8 and the vertex-to-cell CSR (from the P1 connectivity: vertex ids are P1 dof ids), once
static void dynamic_ensure(nsfem_ctx* c) {
  nsfem_ctx::Dynamic& D = c->dyn;
  if (D.buf.allocated) return;
  const MeshDev& m = c->mesh;
  const int nl1 = m.dim + 1, nv = m.n_p1, nc = m.n_cells;
  NSFEM_REQUIRE(c->h_p1map.size() == (size_t)nl1 * nc, "dynamic Smagorinsky: no host copy of the P1 connectivity");
  std::vector<int32_t> vptr((size_t)nv + 1, 0), vcell((size_t)nl1 * nc);
  for (size_t i = 0; i < c->h_p1map.size(); ++i) {
    NSFEM_REQUIRE(c->h_p1map[i] >= 0 && c->h_p1map[i] < nv, "dynamic Smagorinsky: P1 connectivity out of range");
    ++vptr[(size_t)c->h_p1map[i] + 1];
  }
  for (int v = 0; v < nv; ++v) vptr[(size_t)v + 1] += vptr[v];
  std::vector<int32_t> fill(vptr.begin(), vptr.end() - 1);
  for (int k = 0; k < nc; ++k)                               // ascending cells: every run comes out sorted
    for (int i = 0; i < nl1; ++i) vcell[(size_t)fill[c->h_p1map[(size_t)k * nl1 + i]]++] = k;
  D.vptr.upload(vptr, c->stream);
  D.vcell.upload(vcell, c->stream);
  dynamic_alloc(c, D.buf, false);
}

// The three launches of the Germano-Lilly procedure; returns the vertex field that the element / facet launch on the
// SAME level reads.
//   T null   law 8: C_s^2 on the level u.  Every other law: null, nothing launched
//   T given  the dynamic subgrid heat flux (nsfem_set_scalar_sgs_dynamic): C_theta on the level pair (u, T).  Its
//            buffers are allocated by the first run (a context that never switches the term on allocates nothing);
//            the vertex-to-cell CSR and the group list are those of law 8
static const double* dynamic_run(nsfem_ctx* c, const double* u, const double* T = nullptr) {
  if (!T && c->visc.law != 8) return nullptr;
  const nsfem_ctx::Dynamic& D = c->dyn;
  NSFEM_REQUIRE(c->visc.law == 8 && D.buf.allocated,
                T ? "dynamic subgrid heat flux: law 8 is not set (nsfem_set_viscosity_law)"
                  : "dynamic Smagorinsky: buffers not allocated");
  nsfem_ctx::DynamicBuffers& B = T ? c->sc.dynflux.buf : c->dyn.buf;
  dynamic_alloc(c, B, T != nullptr);
  const DynamicDev d{D.n_groups, D.vptr.p, D.vcell.p, D.goff.p, D.gvert.p, B.mom.p, B.vert.p, B.sums.p, B.field.p};
  launch_dynamic_constant(c->stream, c->mesh, u, T, c->visc.p[0], T ? c->sc.dynflux.ctheta_max : c->visc.p[1], d);
  ++B.runs;
  B.launches += 3;
  return B.field.p;
}

// ---- Lagrangian averaging of law 8 (nsfem_set_dynamic_averaging mode 1): the constant is state of the time levels
static bool lagrangian_on(const nsfem_ctx* c) { return c->visc.law == 8 && c->dyn.lag.mode == 1; }

static void lagrangian_reset(nsfem_ctx* c) {
  nsfem_ctx::Dynamic::Lagrangian& L = c->dyn.lag;
  L.have_state = L.cur_valid = L.have_prev = false;
}

// One run in mode 1 on the velocity u: k_dyn_moments, k_dyn_vertex, k_dyn_lagrange -- rules 1 to 5 applied to the
// stored I with step size k, or the initialisation rule (init, and always while no state exists).  Writes Inew
// [n_p1][2], cs2 [n_p1] and, where not null, up [n_p1][2]; what of these is stored state is the caller's business.
// vertex_only: the first two launches alone (the vertex rows in dyn.buf.vert)
static void lagrangian_run(nsfem_ctx* c, const double* u, double k, bool init, double* Inew, double* cs2, double* up,
                           bool vertex_only = false) {
  nsfem_ctx::Dynamic& D = c->dyn;
  nsfem_ctx::DynamicBuffers& B = D.buf;
  NSFEM_REQUIRE(lagrangian_on(c) && B.allocated && D.lag.I.p, "dynamic Smagorinsky: Lagrangian averaging is not set");
  dynamic_alloc(c, B, false);
  const DynamicDev d{D.n_groups, D.vptr.p, D.vcell.p, D.goff.p, D.gvert.p, B.mom.p, B.vert.p, B.sums.p, cs2};
  DynamicLagrangeDev l;
  l.Iold = !init && D.lag.have_state ? D.lag.I.p : nullptr;
  l.k = k;
  l.theta = D.lag.theta;
  l.cs2_init = D.lag.cs2_init;
  l.cs2_floor = D.lag.cs2_floor;
  l.Inew = Inew;
  l.up = up;
  l.vertex_only = vertex_only;
  launch_dynamic_constant(c->stream, c->mesh, u, nullptr, c->visc.p[0], c->visc.p[1], d, &l);
  if (!vertex_only) ++B.runs;
  B.launches += vertex_only ? 2 : 3;
}

// The vertex field an explicit vector of mode 1 is formed with.  Level n (u1): cs2_cur, formed ONCE per level by
// nsfem_step_imex (commit) and kept until nsfem_advance; nsfem_imex_rhs (no commit) reads it where it exists and else
// applies the rules to the stored I into scratch.  Level n-1 (u2): cs2_prev; without one the initialisation rule on u2
// into scratch.  Only the committing run writes state
static const double* lagrangian_level_field(nsfem_ctx* c, const double* u, bool level_n, bool commit) {
  nsfem_ctx::Dynamic::Lagrangian& L = c->dyn.lag;
  if (level_n) {
    if (L.cur_valid) return L.cs2_cur.p;
    if (commit) {
      lagrangian_run(c, u, c->k, false, L.Inew.p, L.cs2_cur.p, nullptr);
      L.cur_valid = true;
      return L.cs2_cur.p;
    }
    lagrangian_run(c, u, c->k, false, L.work.p, c->dyn.buf.field.p, nullptr);
    return c->dyn.buf.field.p;
  }
  if (L.have_prev) return L.cs2_prev.p;
  lagrangian_run(c, u, c->k, true, L.work.p, c->dyn.buf.field.p, nullptr);
  return c->dyn.buf.field.p;
}

// The vertex field the hooks read for a velocity slot (nsfem_viscosity_residual, nsfem_viscosity_cells,
// nsfem_wall_compute with use_law, nsfem_dynamic_constant).  Mode 0: the procedure on the slot.  Mode 1: the STORED
// field of the slot's level, never advanced and never formed again -- NSFEM_U2: cs2_prev; the other slots: cs2_cur
// where formed, else the newest field there is (cs2_prev); where the level has no field at all, the initialisation
// rule on the slot into scratch, no state written
static const double* dynamic_slot_field(nsfem_ctx* c, int velocity_slot) {
  const double* u = c->state[velocity_slot].p;
  if (!lagrangian_on(c)) return dynamic_run(c, u);
  nsfem_ctx::Dynamic::Lagrangian& L = c->dyn.lag;
  if (velocity_slot != NSFEM_U2 && L.cur_valid) return L.cs2_cur.p;
  if (L.have_prev) return L.cs2_prev.p;
  lagrangian_run(c, u, c->k, true, L.work.p, c->dyn.buf.field.p, nullptr);
  return c->dyn.buf.field.p;
}

// The explicit vector of a level, stated ONCE:  N(u) = c_c conv(u) (+ M (gam x u)) + V(u) + B(u) + W(u).  The convective part
// (with the Coriolis vector of the level) is in `n` already -- imex_rhs for u1, imex_form_n2 for u2; this adds the rest,
// V (nsfem_set_viscosity_law) first, B (nsfem_set_bodies) second and W (nsfem_set_wall_model) third, each only when
// switched on: with law 0 / without bodies / without a wall model nothing is launched.  Each term is TWO launches, after imex_rhs (which runs unchanged on either path) and
// BEFORE the Dirichlet rows are set: the element kernel on u (weight 1, element vectors node-sorted in mesh.rbuf) and
// k_visc_gather, which forms v = the per-node sums from zero in ascending cell order and then, per entry,
// n <- n + v,  rhs <- rhs - b0 v  (two roundings, no contraction).  So with a law and bodies the order is viscosity
// cells, gather, penalisation cells, gather, and the summation order is
//   rhs = [ [ -(t + (b0 c_c conv(u1) + b1 N2)) ] - b0 V(u1) ] - b0 B(u1),   the inner bracket as imex_rhs leaves it.
// level_n: u is the level n (u1; the bodies' pose `cur`), else n-1 (u2; `prev`).  N2 is read as stored (it already
// holds V(u2) + B(u2)); where it is formed afresh the terms are added the same way with b0 = 0 and rhs = null.
// commit (nsfem_step_imex on u1 alone): with Lagrangian averaging the run that forms the constant of level n keeps it
static void imex_explicit_add(nsfem_ctx* c, const double* u, bool level_n, bool commit, double b0, double* n,
                              double* rhs) {
  if (c->visc.law != 0) {
    // (law 8: the constant of THIS level, three launches -- with Lagrangian averaging the level's stored field, formed
    // once; else null)
    const double* cs2v = lagrangian_on(c) ? lagrangian_level_field(c, u, level_n, commit) : dynamic_run(c, u);
    launch_viscosity_cells(c->stream, c->mesh, u, 1.0, c->visc.law, c->visc.p, false, cs2v);
    launch_viscosity_gather(c->stream, c->mesh, b0, n, rhs);
    ++c->visc.launches;
  }
  if (c->bodies.cur.n != 0) {
    launch_penalty_cells(c->stream, c->mesh, u, 1.0, level_n ? c->bodies.cur : c->bodies.prev, false);
    launch_viscosity_gather(c->stream, c->mesh, b0, n, rhs);
    ++c->bodies.launches;
  }
  // W (nsfem_set_wall_model) third, the same two-roundings rule: the facet kernel, then its gather over the nodes on
  // modelled facets
  if (c->wm.dev.law != 0) {
    launch_wall_model_facets(c->stream, c->mesh, c->wm.dev, u, c->coef[2], 1.0);
    launch_wall_model_gather(c->stream, c->mesh, c->wm.dev, b0, n, rhs);
    ++c->wm.launches;
  }
}

// n2 <- N(u2) from scratch (nsfem_step_imex where the stored N2 does not serve; nsfem_imex_rhs always).  gam2: the
// 2 c_cor Omega(t^(n-1)), null without rotation at that level
static void imex_form_n2(nsfem_ctx* c, const double* gam2, double* n2) {
  const double cc = cc_of(c);
  NSFEM_HIP(hipMemsetAsync(n2, 0, sizeof(double) * nvel(c), c->stream));
  if (cc != 0.0 || gam2) launch_convection_residual(c->stream, c->mesh, c->state[NSFEM_U2].p, cc, n2, c->conv_form, gam2);
  imex_explicit_add(c, c->state[NSFEM_U2].p, false, false, 0.0, n2, nullptr);
}

nsfem_ctx::ImexKey nsfem_ctx::ImexKey::of(const nsfem_ctx& c, const double gam[3]) {
  ImexKey k;
  k.form = c.conv_form;
  k.cc = cc_of(&c);
  k.visc = c.visc.epoch;
  k.body = c.bodies.epoch;
  k.wall = c.wm.epoch;
  std::memcpy(k.gam, gam, sizeof(k.gam));
  return k;
}

static void imex_require_supported(nsfem_ctx* c) {
  NSFEM_REQUIRE(c->imex_active, "nsfem_set_imex has not been called");
  NSFEM_REQUIRE(c->bodies.cur.n == 0 || !c->comm,
                "immersed bodies: contexts with a communicator (partitioned meshes) are not supported");
  NSFEM_REQUIRE(c->visc.law == 0 || !c->comm,
                "variable viscosity: contexts with a communicator (partitioned meshes) are not supported");
  NSFEM_REQUIRE(c->wm.dev.law == 0 || !c->comm,
                "wall model: contexts with a communicator (partitioned meshes) are not supported");
  NSFEM_REQUIRE(c->imex_rot.treatment == 1 || (!coriolis_active(c) && !euler_active(c)),
                "IMEX pressure correction: rotating frames (Coriolis / Euler terms) are not supported");
}

// 2 c_cor Omega at the old level `lev` (0: t^n, 1: t^(n-1)) -> gam[3] (2D: gam[0]); false: no rotation at that level,
// the non-rotating kernels run
static bool imex_rotation_gamma(const nsfem_ctx* c, int lev, double gam[3]) {
  gam[0] = gam[1] = gam[2] = 0.0;
  if (c->imex_rot.treatment != 1) return false;
  const int nc = c->mesh.dim == 2 ? 1 : 3;
  double w[3] = {0.0, 0.0, 0.0};
  for (int a = 0; a < nc; ++a)
    w[a] = c->imex_rot.given[lev] ? c->imex_rot.w[lev][a] : (c->mesh.dim == 2 ? c->omega : c->omega3[a]);
  if (w[0] == 0.0 && w[1] == 0.0 && w[2] == 0.0) return false;      // (gam stays +0.0: the stored vector's key)
  NSFEM_REQUIRE(std::isfinite(c->coef[4]), "angular velocity set but coriolis_term coefficient is None");
  for (int a = 0; a < nc; ++a) gam[a] = 2.0 * c->coef[4] * w[a];
  if (gam[0] != 0.0 || gam[1] != 0.0 || gam[2] != 0.0) return true;
  gam[0] = gam[1] = gam[2] = 0.0;
  return false;
}

extern "C" int nsfem_step_imex(nsfem_ctx* ctx, const nsfem_step_opts* opts, nsfem_step_info* info) {
  nsfem_step_info local;
  API_BEGIN
  nsfem_step_info& inf = step_begin(ctx, opts, info, local, false, false);
  NSFEM_REQUIRE(opts->momentum.precond == 0 || opts->momentum.precond == 1,
                "IMEX diffusion step: momentum.precond must be 0 (Jacobi) or 1 (multigrid)");
  imex_require_supported(ctx);
  hipStream_t s = ctx->stream;
  const int64_t nv = nvel(ctx);
  // ---- diffusion step: one linear solve
  ensure_imex_ops(ctx);
  imex_begin_step(ctx);
  const bool u1_travelled = imex_exchange_stale_levels(ctx);
  double gam1[3], gam2[3];
  const bool rot1 = imex_rotation_gamma(ctx, 0, gam1), rot2 = imex_rotation_gamma(ctx, 1, gam2);
  const double* n2 = nullptr;
  if (ctx->imex_beta[1] != 0.0) {
    // c_c N(u2): what the previous step stored, unless the level or a component of its key changed under it (the
    // key it must have now is that of the 2 c_cor Omega(t^(n-1)) of this step)
    if (!(ctx->conv_n2_valid && ctx->conv_key.serves(nsfem_ctx::ImexKey::of(*ctx, gam2)))) {
      imex_form_n2(ctx, rot2 ? gam2 : nullptr, ctx->state[NSFEM_CONV_N2].p);
      if (ctx->imex_rot.treatment == 1 && ctx->conv_n2_valid) ++ctx->imex_rot.recomputed;
      if (ctx->visc.law != 0) ++ctx->visc.recomputed;
      if (ctx->bodies.cur.n != 0) ++ctx->bodies.recomputed;
      if (ctx->wm.dev.law != 0) ++ctx->wm.recomputed;
      if (ctx->distributed() && ctx->ghost_v.p) launch_zero_ghost(s, nv, ctx->mask_v.p, ctx->state[NSFEM_CONV_N2].p);
      ctx->conv_n2_valid = true;
    }
    n2 = ctx->state[NSFEM_CONV_N2].p;
  }
  ctx->imex_last_path = imex_rhs(ctx, 0, n2, ctx->state[NSFEM_CONV_N1].p, ctx->rhs_v.p, u1_travelled,
                                 rot1 ? gam1 : nullptr);
  ++(ctx->imex_last_path == 2 ? ctx->imex_lattice_rhs : ctx->imex_generic_rhs);
  if (rot1) ++ctx->imex_rot.rhs;
  imex_explicit_add(ctx, ctx->state[NSFEM_U1].p, true, true, ctx->imex_beta[0], ctx->state[NSFEM_CONV_N1].p,
                    ctx->rhs_v.p);
  ctx->conv_n1_fresh = true;
  ctx->conv_key = nsfem_ctx::ImexKey::of(*ctx, gam1);       // (the next step's N2: formed with Omega(t^n))
  {
    // Dirichlet rows u*_i = g_i; start vector u1 with the Dirichlet values
    double* x = ctx->state[NSFEM_USTAR].p;
    launch_set_values(s, ctx->nbc_v, ctx->bc_v_dofs.p, ctx->bc_v_vals.p, ctx->rhs_v.p);
    // (partitioned: Dirichlet dofs on ghost nodes belong to their owners -- ghost rows stay out of the dot products;
    // the ghost entries of the start vector are those of u1, exchanged for the right-hand side)
    if (ctx->distributed() && ctx->ghost_v.p) launch_zero_ghost(s, nv, ctx->mask_v.p, ctx->rhs_v.p);
    NSFEM_HIP(hipMemcpyAsync(x, ctx->state[NSFEM_U1].p, sizeof(double) * nv, hipMemcpyDeviceToDevice, s));
    launch_set_values(s, ctx->nbc_v, ctx->bc_v_dofs.p, ctx->bc_v_vals.p, x);
    LinOp op;
    if (ctx->traction_form) {       // block matrix  (alpha0/k M + gamma0 c_v K) I + gamma0 c_v E
      const double cvE = ctx->imex_gamma[0] * ctx->coef[2];
      launch_jacobian_init(s, ctx->mesh.dim, ctx->p22.nnz, ctx->L.vals.p, ctx->E.vals.p, cvE, ctx->J.vals.p);
      op.A = &ctx->J;
      op.nv = 1;
    } else {
      op.A = &ctx->L;
      op.nv = ctx->mesh.dim;
    }
    op.rowmask = ctx->mask_v.p;
    op.maskmode = MASK_ZERO;
    op.dinv = ctx->dinv_v.p;
    fill_linop(ctx, op, true);
    if (opts->momentum.precond == 1) {
      NSFEM_REQUIRE(ctx->mg_built, "multigrid requested but no hierarchy was set (nsfem_mg_finalize)");
      set_velocity_cycle_symmetric(ctx, true);
      mg_refresh(ctx, true);
      op.prec = &ctx->mom_prec;
    } else {
      launch_inv_diag(s, *op.A, op.nv, ctx->mask_v.p, ctx->dinv_v.p);
    }
    op.graph_epoch = ctx->graph_epoch;
    nsfem_solve_info si;
    nsfem_ctx::SolveHint& hint = ctx->hint_mom[0];
    int rc = pcg(s, ctx->kw, op, ctx->rhs_v.p, x, hinted(opts->momentum, hint), si, false);
    note_solve(hint, si, opts->momentum, ctx->kw.last_target);
    inf.krylov_iterations_momentum = si.iterations;
    if (rc != NSFEM_OK) throw Error(rc, "CG failed in the IMEX diffusion step");
    inf.newton_iterations = 0;
    inf.converged = 1;
  }
  projection_step(ctx, opts, inf);
  correction_step(ctx, opts, inf);
  ctx->assembled_system = -1;
  API_END(ctx)
}

extern "C" int nsfem_imex_info(nsfem_ctx* ctx, int64_t out[4]) {
  API_BEGIN
  NSFEM_REQUIRE(ctx && out, "null argument");
  out[0] = ctx->imex_last_path;
  out[1] = ctx->imex_lattice_rhs;
  out[2] = ctx->imex_generic_rhs;
  out[3] = ctx->imex_matrix_builds;
  API_END(ctx)
}

extern "C" int nsfem_imex_rhs(nsfem_ctx* ctx, int path, int convective_form, double* rhs, double* conv_n1) {
  API_BEGIN
  NSFEM_REQUIRE(ctx && rhs, "null argument");
  NSFEM_REQUIRE(path == 1 || path == 2, "path: 1 generic, 2 one-launch");
  NSFEM_REQUIRE(convective_form >= 0 && convective_form <= 3, "unknown convective form");
  imex_require_supported(ctx);
  if (ctx->conv_form != convective_form || ctx->picard) ctx->graph_epoch++;
  ctx->conv_form = convective_form;
  ctx->picard = false;
  hipStream_t s = ctx->stream;
  const int64_t nv = nvel(ctx);
  ensure_imex_ops(ctx);
  imex_begin_step(ctx);
  // (work vectors of the Krylov solvers: nothing of the step's own state is touched; c_c N(u2) is evaluated afresh)
  ctx->kw.ensure(nv);
  ++ctx->kw.touch;
  double *n1 = ctx->kw.p.p, *n2 = nullptr, *out = ctx->kw.q.p;
  // (every rank fails here or none: the path was agreed on when the operators were built)
  NSFEM_REQUIRE(path != 2 || imex_lattice_ok(ctx),
                "one-launch IMEX right-hand side: not available on this mesh / these settings");
  const bool u1_travelled = imex_exchange_stale_levels(ctx);
  double gam1[3], gam2[3];
  const bool rot1 = imex_rotation_gamma(ctx, 0, gam1), rot2 = imex_rotation_gamma(ctx, 1, gam2);
  if (ctx->imex_beta[1] != 0.0) {
    n2 = ctx->kw.z.p;
    imex_form_n2(ctx, rot2 ? gam2 : nullptr, n2);
  }
  imex_rhs(ctx, path, n2, n1, out, u1_travelled, rot1 ? gam1 : nullptr);
  if (rot1) ++ctx->imex_rot.rhs;
  imex_explicit_add(ctx, ctx->state[NSFEM_U1].p, true, false, ctx->imex_beta[0], n1, out);
  NSFEM_HIP(hipMemcpyAsync(rhs, out, sizeof(double) * nv, hipMemcpyDeviceToHost, s));
  if (conv_n1) NSFEM_HIP(hipMemcpyAsync(conv_n1, n1, sizeof(double) * nv, hipMemcpyDeviceToHost, s));
  NSFEM_HIP(hipStreamSynchronize(s));
  API_END(ctx)
}

// rotating frame in the IMEX calls: opt-in (the default refuses, imex_require_supported)
extern "C" int nsfem_set_imex_rotation(nsfem_ctx* ctx, int treatment, const double* omega_n, const double* omega_nm1) {
  API_BEGIN
  NSFEM_REQUIRE(ctx, "null context");
  NSFEM_REQUIRE(treatment == 0 || treatment == 1, "IMEX rotation: treatment 0 (refuse) or 1 (explicit Coriolis term)");
  nsfem_ctx::ImexRotation& r = ctx->imex_rot;
  const int nc = ctx->mesh.dim == 2 ? 1 : 3;
  const double* w[2] = {omega_n, omega_nm1};
  for (int lev = 0; lev < 2; ++lev)
    for (int a = 0; a < nc && w[lev]; ++a)
      NSFEM_REQUIRE(std::isfinite(w[lev][a]), "non-finite angular velocity");
  r.treatment = treatment;
  for (int lev = 0; lev < 2; ++lev) {
    r.given[lev] = treatment == 1 && w[lev] != nullptr;
    for (int a = 0; a < 3; ++a) r.w[lev][a] = r.given[lev] && a < nc ? w[lev][a] : 0.0;
  }
  API_END(ctx)
}

extern "C" int nsfem_imex_rotation_info(nsfem_ctx* ctx, int64_t out[4]) {
  API_BEGIN
  NSFEM_REQUIRE(ctx && out, "null argument");
  out[0] = ctx->imex_rot.treatment;
  out[1] = ctx->imex_rot.rhs;
  out[2] = ctx->imex_rot.recomputed;
  out[3] = 0;
  API_END(ctx)
}

// ---------------------------------------------------------------- variable viscosity
extern "C" int nsfem_set_viscosity_law(nsfem_ctx* ctx, int law, const double params[4]) {
  API_BEGIN
  NSFEM_REQUIRE(ctx, "null context");
  NSFEM_REQUIRE(is_viscosity_law(law),
                "variable viscosity: unknown law (0 none, 1 Smagorinsky, 2 Carreau, 4 WALE, 5 Vreman, 8 dynamic Smagorinsky)");
  NSFEM_REQUIRE(law == 0 || !ctx->comm,
                "variable viscosity: contexts with a communicator (partitioned meshes) are not supported");
  NSFEM_REQUIRE(law == 0 || params, "variable viscosity: the law needs its parameters");
  double p[4] = {0.0, 0.0, 0.0, 0.0};
  if (law == 1) {
    NSFEM_REQUIRE(std::isfinite(params[0]) && params[0] >= 0.0, "Smagorinsky: C_s must be finite and >= 0");
    p[0] = params[0];
  } else if (law == 2) {
    NSFEM_REQUIRE(std::isfinite(params[0]), "Carreau: a = c_v - nu_inf must be finite");
    NSFEM_REQUIRE(std::isfinite(params[1]) && params[1] >= 0.0, "Carreau: lambda must be finite and >= 0");
    NSFEM_REQUIRE(std::isfinite(params[2]) && params[2] > 0.0, "Carreau: n must be finite and > 0");
    p[0] = params[0];
    p[1] = params[1];
    p[2] = params[2];
  } else if (law == 4) {
    NSFEM_REQUIRE(std::isfinite(params[0]) && params[0] >= 0.0, "WALE: C_w must be finite and >= 0");
    p[0] = params[0];
  } else if (law == 5) {
    NSFEM_REQUIRE(std::isfinite(params[0]) && params[0] >= 0.0, "Vreman: c must be finite and >= 0");
    p[0] = params[0];
  } else if (law == 8) {
    NSFEM_REQUIRE(std::isfinite(params[0]) && params[0] > 1.0, "dynamic Smagorinsky: alpha must be finite and > 1");
    NSFEM_REQUIRE(std::isfinite(params[1]) && params[1] > 0.0, "dynamic Smagorinsky: cs2_max must be finite and > 0");
    p[0] = params[0];
    p[1] = params[1];
  }
  nsfem_ctx::Viscosity& v = ctx->visc;
  if (law == 8) {
    // buffers on the first call, kept afterwards; the groups go back to global (other groups were another law)
    dynamic_ensure(ctx);
    if (!ctx->dyn.global || !ctx->dyn.goff.p) {
      if (!ctx->dyn.global) ++v.epoch;
      dynamic_upload_groups(ctx, 1, nullptr);
    }
    // (... and the averaging back to the groups: the Lagrangian state belonged to the law as it was set before)
    if (ctx->dyn.lag.mode != 0) {
      ctx->dyn.lag.mode = 0;
      lagrangian_reset(ctx);
      ++v.epoch;
    }
  }
  // (the stored explicit vectors belong to the law and parameters they were evaluated with; the law enters no
  // captured Krylov body -- its launches precede the solve --, so graph_epoch stays)
  if (law != v.law || std::memcmp(p, v.p, sizeof(p)) != 0) ++v.epoch;
  v.law = law;
  std::memcpy(v.p, p, sizeof(p));
  API_END(ctx)
}

static void viscosity_require(nsfem_ctx* ctx, int velocity_slot) {
  NSFEM_REQUIRE(!ctx->comm, "variable viscosity: contexts with a communicator (partitioned meshes) are not supported");
  NSFEM_REQUIRE(ctx->visc.law != 0, "variable viscosity: no law set (nsfem_set_viscosity_law)");
  require_velocity_slot(velocity_slot);
}

extern "C" int nsfem_viscosity_residual(nsfem_ctx* ctx, int velocity_slot, double weight, double* out_host) {
  API_BEGIN
  NSFEM_REQUIRE(ctx && out_host, "null argument");
  viscosity_require(ctx, velocity_slot);
  require_finite_weight(weight);
  hipStream_t s = ctx->stream;
  const int64_t nv = nvel(ctx);
  hook_to_host(ctx, nv, out_host, [&](double* out) {
    NSFEM_HIP(hipMemsetAsync(out, 0, sizeof(double) * nv, s));
    const double* cs2v = dynamic_slot_field(ctx, velocity_slot);
    launch_viscosity_cells(s, ctx->mesh, ctx->state[velocity_slot].p, weight, ctx->visc.law, ctx->visc.p, false, cs2v);
    launch_viscosity_gather(s, ctx->mesh, 0.0, out, nullptr);
    ++ctx->visc.launches;
  });
  API_END(ctx)
}

extern "C" int nsfem_viscosity_cells(nsfem_ctx* ctx, int velocity_slot, double* out_host) {
  API_BEGIN
  NSFEM_REQUIRE(ctx && out_host, "null argument");
  viscosity_require(ctx, velocity_slot);
  hipStream_t s = ctx->stream;
  // (the cell means land in the element buffer, which every user fills before it reads)
  const double* cs2v = dynamic_slot_field(ctx, velocity_slot);
  launch_viscosity_cells(s, ctx->mesh, ctx->state[velocity_slot].p, 1.0, ctx->visc.law, ctx->visc.p, true, cs2v);
  ++ctx->visc.launches;
  NSFEM_HIP(hipMemcpyAsync(out_host, ctx->mesh.rbuf.p, sizeof(double) * ctx->mesh.n_cells, hipMemcpyDeviceToHost, s));
  NSFEM_HIP(hipStreamSynchronize(s));
  API_END(ctx)
}

extern "C" int nsfem_viscosity_info(nsfem_ctx* ctx, int64_t out[4]) {
  API_BEGIN
  NSFEM_REQUIRE(ctx && out, "null argument");
  out[0] = ctx->visc.law;
  out[1] = ctx->visc.launches;
  out[2] = ctx->visc.recomputed;
  out[3] = 0;
  API_END(ctx)
}

// ---- dynamic Smagorinsky: averaging groups, the constant as output / test hook, counters
extern "C" int nsfem_set_dynamic_groups(nsfem_ctx* ctx, int n_groups, const int32_t* group_of_vertex) {
  API_BEGIN
  NSFEM_REQUIRE(ctx && group_of_vertex, "null argument");
  NSFEM_REQUIRE(ctx->visc.law == 8, "dynamic Smagorinsky: groups without law 8 (nsfem_set_viscosity_law)");
  NSFEM_REQUIRE(n_groups >= 1, "dynamic Smagorinsky: n_groups must be >= 1");
  const int nv = ctx->mesh.n_p1;
  for (int v = 0; v < nv; ++v)
    NSFEM_REQUIRE(group_of_vertex[v] >= 0 && group_of_vertex[v] < n_groups,
                  "dynamic Smagorinsky: group id out of range");
  nsfem_ctx::Dynamic& D = ctx->dyn;
  if (D.lag.mode != 0) {             // (groups are mode 0 of nsfem_set_dynamic_averaging)
    D.lag.mode = 0;
    lagrangian_reset(ctx);
    ++ctx->visc.epoch;
  }
  const bool same = !D.global && D.n_groups == n_groups &&
                    std::memcmp(D.h_group.data(), group_of_vertex, sizeof(int32_t) * (size_t)nv) == 0;
  if (!same) {
    dynamic_upload_groups(ctx, n_groups, group_of_vertex);
    ++ctx->visc.epoch;               // (the stored explicit vectors belong to the groups they were evaluated with)
  }
  API_END(ctx)
}

// what a run has left, to the host: the constant of every group, sums [n_groups][2] = num, den (may be null) and the
// vertex rows [n_p1][3] (may be null)
static void dynamic_read_back(nsfem_ctx* c, nsfem_ctx::DynamicBuffers& B, double* groups, double* sums,
                              double* vertices) {
  hipStream_t s = c->stream;
  const int ng = c->dyn.n_groups;
  B.h_sums.resize((size_t)ng * 3);
  NSFEM_HIP(hipMemcpyAsync(B.h_sums.data(), B.sums.p, sizeof(double) * B.h_sums.size(), hipMemcpyDeviceToHost, s));
  if (vertices)
    NSFEM_HIP(hipMemcpyAsync(vertices, B.vert.p, sizeof(double) * (size_t)c->mesh.n_p1 * 3, hipMemcpyDeviceToHost, s));
  NSFEM_HIP(hipStreamSynchronize(s));
  for (int g = 0; g < ng; ++g) {
    groups[g] = B.h_sums[(size_t)g * 3 + 2];
    if (sums) {
      sums[(size_t)g * 2] = B.h_sums[(size_t)g * 3];
      sums[(size_t)g * 2 + 1] = B.h_sums[(size_t)g * 3 + 1];
    }
  }
}

// (bytes of the buffers of one use, for the info calls)
static int64_t dynamic_bytes(const nsfem_ctx::DynamicBuffers& B) {
  return (int64_t)(sizeof(double) * (B.mom.n + B.vert.n + B.sums.n + B.field.n));
}

extern "C" int nsfem_dynamic_constant(nsfem_ctx* ctx, int velocity_slot, double* cs2_groups, double* sums,
                                      double* vertices) {
  API_BEGIN
  NSFEM_REQUIRE(ctx && cs2_groups, "null argument");
  NSFEM_REQUIRE(!ctx->comm, "variable viscosity: contexts with a communicator (partitioned meshes) are not supported");
  NSFEM_REQUIRE(ctx->visc.law == 8, "dynamic Smagorinsky: law 8 is not set (nsfem_set_viscosity_law)");
  require_velocity_slot(velocity_slot);
  if (lagrangian_on(ctx)) {
    // the stored vertex field of the slot's level, [n_p1]; the vertex rows are those of the slot's velocity (two
    // launches); there are no group sums
    NSFEM_REQUIRE(!sums, "dynamic Smagorinsky: Lagrangian averaging has no group sums (sums must be NULL)");
    hipStream_t s = ctx->stream;
    const size_t nv = (size_t)ctx->mesh.n_p1;
    const double* field = dynamic_slot_field(ctx, velocity_slot);
    NSFEM_HIP(hipMemcpyAsync(cs2_groups, field, sizeof(double) * nv, hipMemcpyDeviceToHost, s));
    if (vertices) {
      lagrangian_run(ctx, ctx->state[velocity_slot].p, ctx->k, true, nullptr, ctx->dyn.buf.field.p, nullptr, true);
      NSFEM_HIP(hipMemcpyAsync(vertices, ctx->dyn.buf.vert.p, sizeof(double) * nv * 3, hipMemcpyDeviceToHost, s));
    }
    NSFEM_HIP(hipStreamSynchronize(s));
    return NSFEM_OK;
  }
  dynamic_run(ctx, ctx->state[velocity_slot].p);
  dynamic_read_back(ctx, ctx->dyn.buf, cs2_groups, sums, vertices);
  API_END(ctx)
}

// ---- Lagrangian averaging: the setter, the state for restart files, one application as output / test hook
extern "C" int nsfem_set_dynamic_averaging(nsfem_ctx* ctx, int mode, const double params[4]) {
  API_BEGIN
  NSFEM_REQUIRE(ctx, "null context");
  NSFEM_REQUIRE(!ctx->comm, "variable viscosity: contexts with a communicator (partitioned meshes) are not supported");
  NSFEM_REQUIRE(ctx->visc.law == 8, "dynamic Smagorinsky: averaging without law 8 (nsfem_set_viscosity_law)");
  NSFEM_REQUIRE(mode == 0 || mode == 1, "dynamic Smagorinsky: unknown averaging mode (0 groups, 1 Lagrangian)");
  nsfem_ctx::Dynamic::Lagrangian& L = ctx->dyn.lag;
  if (mode == 0) {
    if (L.mode != 0) {
      L.mode = 0;
      lagrangian_reset(ctx);
      ++ctx->visc.epoch;
    }
    return NSFEM_OK;
  }
  NSFEM_REQUIRE(params, "dynamic Smagorinsky: Lagrangian averaging needs its parameters");
  NSFEM_REQUIRE(std::isfinite(params[0]) && params[0] > 0.0, "Lagrangian averaging: theta must be finite and > 0");
  NSFEM_REQUIRE(std::isfinite(params[1]) && params[1] >= 0.0, "Lagrangian averaging: cs2_init must be finite and >= 0");
  NSFEM_REQUIRE(std::isfinite(params[2]) && params[2] >= 0.0, "Lagrangian averaging: cs2_floor must be finite and >= 0");
  NSFEM_REQUIRE(!ctx->sc.dynflux.on,
                "Lagrangian averaging: the dynamic subgrid heat flux is on (nsfem_set_scalar_sgs_dynamic); a Lagrangian "
                "C_theta is not supported");
  const size_t nv = (size_t)ctx->mesh.n_p1;
  if (!L.I.p) {
    L.I.alloc(nv * 2);
    L.Inew.alloc(nv * 2);
    L.cs2_cur.alloc(nv);
    L.cs2_prev.alloc(nv);
    L.work.alloc(nv * 4);
  }
  if (L.mode != 1 || L.theta != params[0] || L.cs2_init != params[1] || L.cs2_floor != params[2]) {
    lagrangian_reset(ctx);
    ++ctx->visc.epoch;
  }
  L.mode = 1;
  L.theta = params[0];
  L.cs2_init = params[1];
  L.cs2_floor = params[2];
  API_END(ctx)
}

static void lagrangian_require(nsfem_ctx* ctx) {
  NSFEM_REQUIRE(!ctx->comm, "variable viscosity: contexts with a communicator (partitioned meshes) are not supported");
  NSFEM_REQUIRE(lagrangian_on(ctx),
                "dynamic Smagorinsky: Lagrangian averaging is not set (nsfem_set_viscosity_law 8, "
                "nsfem_set_dynamic_averaging 1)");
}

extern "C" int nsfem_dynamic_lagrangian_state(nsfem_ctx* ctx, int direction, double* state) {
  API_BEGIN
  NSFEM_REQUIRE(ctx && state, "null argument");
  lagrangian_require(ctx);
  NSFEM_REQUIRE(direction == 0 || direction == 1, "Lagrangian state: direction 0 (get) or 1 (set)");
  nsfem_ctx::Dynamic::Lagrangian& L = ctx->dyn.lag;
  hipStream_t s = ctx->stream;
  const size_t nv = (size_t)ctx->mesh.n_p1;
  std::vector<double> I(nv * 2), cur(nv), prev(nv);
  if (direction == 0) {
    const double* level_n = L.cur_valid ? L.cs2_cur.p : L.have_prev ? L.cs2_prev.p : nullptr;
    if (L.have_state) NSFEM_HIP(hipMemcpyAsync(I.data(), L.I.p, sizeof(double) * nv * 2, hipMemcpyDeviceToHost, s));
    if (level_n) NSFEM_HIP(hipMemcpyAsync(cur.data(), level_n, sizeof(double) * nv, hipMemcpyDeviceToHost, s));
    if (L.have_prev) NSFEM_HIP(hipMemcpyAsync(prev.data(), L.cs2_prev.p, sizeof(double) * nv, hipMemcpyDeviceToHost, s));
    NSFEM_HIP(hipStreamSynchronize(s));
    for (size_t v = 0; v < nv; ++v) {               // (NaN: the column does not exist)
      state[v * 4] = L.have_state ? I[v * 2] : NAN;
      state[v * 4 + 1] = L.have_state ? I[v * 2 + 1] : NAN;
      state[v * 4 + 2] = level_n ? cur[v] : NAN;
      state[v * 4 + 3] = L.have_prev ? prev[v] : NAN;
    }
    return NSFEM_OK;
  }
  // set: columns 0, 1 (the state of level n-1) and 3 (cs2_prev) count, each taken where none of its entries is NaN and
  // absent where all are; column 2 is not read -- level n is formed by the next step
  size_t nan_I = 0, nan_prev = 0;
  for (size_t v = 0; v < nv; ++v) {
    nan_I += (std::isnan(state[v * 4]) ? 1 : 0) + (std::isnan(state[v * 4 + 1]) ? 1 : 0);
    nan_prev += std::isnan(state[v * 4 + 3]) ? 1 : 0;
  }
  NSFEM_REQUIRE((nan_I == 0 || nan_I == 2 * nv) && (nan_prev == 0 || nan_prev == nv),
                "Lagrangian state: a column is either given for every vertex or NaN for every vertex");
  for (size_t v = 0; v < nv; ++v) {
    if (nan_I == 0)
      NSFEM_REQUIRE(std::isfinite(state[v * 4]) && std::isfinite(state[v * 4 + 1]) && state[v * 4 + 1] >= 0.0,
                    "Lagrangian state: I_LM must be finite and I_MM finite and >= 0");
    if (nan_prev == 0)
      NSFEM_REQUIRE(std::isfinite(state[v * 4 + 3]) && state[v * 4 + 3] >= 0.0,
                    "Lagrangian state: cs2 must be finite and >= 0");
    I[v * 2] = state[v * 4];
    I[v * 2 + 1] = state[v * 4 + 1];
    prev[v] = state[v * 4 + 3];
  }
  if (nan_I == 0) NSFEM_HIP(hipMemcpyAsync(L.I.p, I.data(), sizeof(double) * nv * 2, hipMemcpyHostToDevice, s));
  if (nan_prev == 0) NSFEM_HIP(hipMemcpyAsync(L.cs2_prev.p, prev.data(), sizeof(double) * nv, hipMemcpyHostToDevice, s));
  NSFEM_HIP(hipStreamSynchronize(s));
  L.have_state = nan_I == 0;
  L.have_prev = nan_prev == 0;
  L.cur_valid = false;
  API_END(ctx)
}

extern "C" int nsfem_dynamic_lagrangian_advance(nsfem_ctx* ctx, int velocity_slot, double k, double* out_state,
                                                double* out_upstream, double* out_cs2) {
  API_BEGIN
  NSFEM_REQUIRE(ctx && out_state && out_cs2, "null argument");
  lagrangian_require(ctx);
  require_velocity_slot(velocity_slot);
  NSFEM_REQUIRE(std::isfinite(k) && k > 0.0, "Lagrangian averaging: the step size must be finite and > 0");
  nsfem_ctx::Dynamic::Lagrangian& L = ctx->dyn.lag;
  hipStream_t s = ctx->stream;
  const size_t nv = (size_t)ctx->mesh.n_p1;
  // (scratch only: work = I' | I_up, buf.field = cs2; the stored I is read, nothing stored is written)
  lagrangian_run(ctx, ctx->state[velocity_slot].p, k, false, L.work.p, ctx->dyn.buf.field.p, L.work.p + nv * 2);
  NSFEM_HIP(hipMemcpyAsync(out_state, L.work.p, sizeof(double) * nv * 2, hipMemcpyDeviceToHost, s));
  if (out_upstream)
    NSFEM_HIP(hipMemcpyAsync(out_upstream, L.work.p + nv * 2, sizeof(double) * nv * 2, hipMemcpyDeviceToHost, s));
  NSFEM_HIP(hipMemcpyAsync(out_cs2, ctx->dyn.buf.field.p, sizeof(double) * nv, hipMemcpyDeviceToHost, s));
  NSFEM_HIP(hipStreamSynchronize(s));
  API_END(ctx)
}

extern "C" int nsfem_dynamic_lagrangian_info(nsfem_ctx* ctx, int64_t out[4]) {
  API_BEGIN
  NSFEM_REQUIRE(ctx && out, "null argument");
  const nsfem_ctx::Dynamic::Lagrangian& L = ctx->dyn.lag;
  out[0] = lagrangian_on(ctx) ? 1 : 0;
  out[1] = L.have_state ? 1 : 0;
  out[2] = L.cur_valid ? 1 : 0;
  out[3] = L.have_prev ? 1 : 0;
  API_END(ctx)
}

extern "C" int nsfem_dynamic_info(nsfem_ctx* ctx, int64_t out[4]) {
  API_BEGIN
  NSFEM_REQUIRE(ctx && out, "null argument");
  const nsfem_ctx::Dynamic& D = ctx->dyn;
  out[0] = D.buf.allocated ? D.n_groups : 0;
  out[1] = D.buf.runs;
  out[2] = D.buf.launches;
  out[3] = (int64_t)(sizeof(int32_t) * (D.vptr.n + D.vcell.n + D.goff.n + D.gvert.n)) + dynamic_bytes(D.buf) +
           (int64_t)(sizeof(double) * (D.lag.I.n + D.lag.Inew.n + D.lag.cs2_cur.n + D.lag.cs2_prev.n + D.lag.work.n));
  API_END(ctx)
}

// ---------------------------------------------------------------- immersed bodies
// nsfem_body -> row s of the table.  move: the kind is the one set and the sizes of kinds 1 and 2 stay as set (the
// normal of a half-space is part of its pose and is taken)
static void body_to_table(const nsfem_body& b, int dim, BodyTable& t, int s, bool move) {
  const int kind = move ? t.kind[s] : b.kind;
  for (int a = 0; a < 3; ++a) {
    const bool in = a < dim;
    NSFEM_REQUIRE(std::isfinite(b.centre[a]) || !in, "immersed bodies: centre not finite");
    NSFEM_REQUIRE(std::isfinite(b.velocity[a]) || !in, "immersed bodies: velocity not finite");
    NSFEM_REQUIRE(std::isfinite(b.angular[a]) || (dim == 2 && a != 2), "immersed bodies: angular velocity not finite");
    t.centre[s][a] = in ? b.centre[a] : 0.0;
    t.velocity[s][a] = in ? b.velocity[a] : 0.0;
    t.angular[s][a] = (dim == 3 || a == 2) ? b.angular[a] : 0.0;
  }
  if (move && kind != 3) return;
  double size[3] = {0.0, 0.0, 0.0};
  if (kind == 1) {
    NSFEM_REQUIRE(std::isfinite(b.size[0]) && b.size[0] > 0.0, "immersed bodies: size (radius) must be finite and > 0");
    size[0] = b.size[0];
  } else if (kind == 2) {
    for (int a = 0; a < dim; ++a) {
      NSFEM_REQUIRE(std::isfinite(b.size[a]) && b.size[a] > 0.0,
                    "immersed bodies: size (half widths) must be finite and > 0");
      size[a] = b.size[a];
    }
  } else {
    double nn = 0.0;
    for (int a = 0; a < dim; ++a) {
      NSFEM_REQUIRE(std::isfinite(b.size[a]), "immersed bodies: size (normal) not finite");
      size[a] = b.size[a];
      nn += size[a] * size[a];
    }
    NSFEM_REQUIRE(std::fabs(std::sqrt(nn) - 1.0) <= 1e-12, "immersed bodies: size of a half-space must be a unit normal");
  }
  for (int a = 0; a < 3; ++a) t.size[s][a] = size[a];
}

// Heated bodies: t becomes the table (have: temperatures are set).  The epoch counts the changes of what the scalar
// step's kernels see -- the table where a flag is 1, nothing where none is --, so the same data again, or passive
// bodies coming and going, leave the stored scalar vectors valid
static void store_thermal(nsfem_ctx::Bodies& b, const ThermalTable& t, bool have) {
  int n_thermal = 0;
  for (int s = 0; s < t.n; ++s) n_thermal += t.flag[s];
  const ThermalTable none;
  const ThermalTable& seen_new = n_thermal > 0 ? t : none;
  const ThermalTable& seen_old = b.n_thermal > 0 ? b.thermal : none;
  if (std::memcmp(&seen_new, &seen_old, sizeof(ThermalTable)) != 0) ++b.thermal_epoch;
  std::memcpy(&b.thermal, &t, sizeof(ThermalTable));
  b.have_thermal = have;
  b.n_thermal = n_thermal;
}

extern "C" int nsfem_set_bodies(nsfem_ctx* ctx, int32_t n, const nsfem_body* bodies, double eta, double smoothing) {
  API_BEGIN
  NSFEM_REQUIRE(ctx, "null context");
  NSFEM_REQUIRE(n >= 0 && n <= NSFEM_MAX_BODIES, "immersed bodies: n must be 0 .. NSFEM_MAX_BODIES (16)");
  BodyTable t;
  if (n > 0) {
    NSFEM_REQUIRE(!ctx->comm, "immersed bodies: contexts with a communicator (partitioned meshes) are not supported");
    NSFEM_REQUIRE(bodies, "immersed bodies: null body array");
    NSFEM_REQUIRE(std::isfinite(eta) && eta > 0.0, "immersed bodies: eta must be finite and > 0");
    NSFEM_REQUIRE(std::isfinite(smoothing) && smoothing >= 0.0, "immersed bodies: smoothing must be finite and >= 0");
    t.n = n;
    for (int s = 0; s < n; ++s) {
      NSFEM_REQUIRE(bodies[s].kind >= 1 && bodies[s].kind <= 3,
                    "immersed bodies: unknown kind (1 ball, 2 box, 3 half-space)");
      t.kind[s] = bodies[s].kind;
      body_to_table(bodies[s], ctx->mesh.dim, t, s, false);
    }
    t.eps = smoothing;
    t.inv_eta = 1.0 / eta;
  }
  nsfem_ctx::Bodies& b = ctx->bodies;
  // (the stored explicit vectors belong to the set they were evaluated with; the bodies enter no captured Krylov
  // body -- their launches precede the solve --, so graph_epoch stays)
  if (std::memcmp(&t, &b.cur, sizeof(BodyTable)) != 0 || std::memcmp(&t, &b.prev, sizeof(BodyTable)) != 0) ++b.epoch;
  std::memcpy(&b.cur, &t, sizeof(BodyTable));
  std::memcpy(&b.prev, &t, sizeof(BodyTable));
  // (temperatures belong to the bodies by index: another count drops them)
  if (b.have_thermal && b.thermal.n != n) store_thermal(b, ThermalTable(), false);
  API_END(ctx)
}

extern "C" int nsfem_move_bodies(nsfem_ctx* ctx, int32_t n, const nsfem_body* bodies) {
  API_BEGIN
  NSFEM_REQUIRE(ctx && bodies, "null argument");
  nsfem_ctx::Bodies& b = ctx->bodies;
  NSFEM_REQUIRE(b.cur.n > 0, "immersed bodies: no body set (nsfem_set_bodies)");
  NSFEM_REQUIRE(n == b.cur.n, "immersed bodies: nsfem_move_bodies with another count than set");
  BodyTable t;
  std::memcpy(&t, &b.cur, sizeof(BodyTable));
  for (int s = 0; s < n; ++s) {
    NSFEM_REQUIRE(bodies[s].kind == t.kind[s], "immersed bodies: nsfem_move_bodies with another kind than set");
    body_to_table(bodies[s], ctx->mesh.dim, t, s, true);
  }
  std::memcpy(&b.prev, &b.cur, sizeof(BodyTable));
  std::memcpy(&b.cur, &t, sizeof(BodyTable));
  API_END(ctx)
}

// The work buffer of a two-launch reduction (a kernel that stores n_parts partials per number, then k_fold_partials):
// the n_out * n_parts partials, the n_out results behind them.  (Re)allocated when the size asked for changes.
struct PartialsWork {
  double* parts;
  double* res;
  size_t n_out;
  PartialsWork(DevBuf<double>& buf, size_t n_out_, int n_parts) : n_out(n_out_) {
    const size_t n_work = n_out * (size_t)(n_parts + 1);
    if (buf.n != n_work) buf.alloc(n_work);
    parts = buf.p;
    res = parts + n_out * (size_t)n_parts;
  }
  // the results to the host: one copy, one synchronise
  void read_back(hipStream_t s, double* out) const {
    NSFEM_HIP(hipMemcpyAsync(out, res, sizeof(double) * n_out, hipMemcpyDeviceToHost, s));
    NSFEM_HIP(hipStreamSynchronize(s));
  }
};

static void bodies_require(nsfem_ctx* ctx, int velocity_slot) {
  NSFEM_REQUIRE(!ctx->comm, "immersed bodies: contexts with a communicator (partitioned meshes) are not supported");
  NSFEM_REQUIRE(ctx->bodies.cur.n != 0, "immersed bodies: no body set (nsfem_set_bodies)");
  require_velocity_slot(velocity_slot);
}

extern "C" int nsfem_body_residual(nsfem_ctx* ctx, int velocity_slot, double weight, double* out_host) {
  API_BEGIN
  NSFEM_REQUIRE(ctx && out_host, "null argument");
  bodies_require(ctx, velocity_slot);
  require_finite_weight(weight);
  hipStream_t s = ctx->stream;
  const int64_t nv = nvel(ctx);
  hook_to_host(ctx, nv, out_host, [&](double* out) {
    NSFEM_HIP(hipMemsetAsync(out, 0, sizeof(double) * nv, s));
    launch_penalty_cells(s, ctx->mesh, ctx->state[velocity_slot].p, weight, ctx->bodies.cur, false);
    launch_viscosity_gather(s, ctx->mesh, 0.0, out, nullptr);
    ++ctx->bodies.launches;
  });
  API_END(ctx)
}

extern "C" int nsfem_body_mask_cells(nsfem_ctx* ctx, double* out_host) {
  API_BEGIN
  NSFEM_REQUIRE(ctx && out_host, "null argument");
  bodies_require(ctx, NSFEM_U0);
  hipStream_t s = ctx->stream;
  // (the cell means land in the element buffer, which every user fills before it reads; MEAN reads no velocity)
  launch_penalty_cells(s, ctx->mesh, ctx->state[NSFEM_U0].p, 1.0, ctx->bodies.cur, true);
  ++ctx->bodies.launches;
  NSFEM_HIP(hipMemcpyAsync(out_host, ctx->mesh.rbuf.p, sizeof(double) * ctx->mesh.n_cells, hipMemcpyDeviceToHost, s));
  NSFEM_HIP(hipStreamSynchronize(s));
  API_END(ctx)
}

extern "C" int nsfem_body_forces(nsfem_ctx* ctx, int velocity_slot, double* out) {
  API_BEGIN
  NSFEM_REQUIRE(ctx && out, "null argument");
  bodies_require(ctx, velocity_slot);
  hipStream_t s = ctx->stream;
  const PartialsWork w(ctx->bodies.work, (size_t)ctx->bodies.cur.n * body_numbers(ctx->mesh.dim), kBodyParts);
  launch_penalty_forces(s, ctx->mesh, ctx->state[velocity_slot].p, ctx->bodies.cur, w.parts, w.res);
  w.read_back(s, out);
  API_END(ctx)
}

extern "C" int nsfem_body_info(nsfem_ctx* ctx, int64_t out[4]) {
  API_BEGIN
  NSFEM_REQUIRE(ctx && out, "null argument");
  out[0] = ctx->bodies.cur.n;
  out[1] = ctx->bodies.launches;
  out[2] = ctx->bodies.recomputed;
  out[3] = 0;
  API_END(ctx)
}

// ---------------------------------------------------------------- wall-stress models
// validates everything on the host first, then replaces the resident set.  The node CSR of the gather is built here,
// from the host copy of the P2 dof map: the nodes on modelled facets ascending, per node its (facet, local) entries in
// ascending facet order.  Switching off (law 0 or no facet) keeps the buffers
extern "C" int nsfem_set_wall_model(nsfem_ctx* ctx, int law, const double params[4], int32_t n_facets,
                                    const int32_t* facet_cell, const int32_t* facet_local, const int32_t* sample_cell,
                                    const double* sample_lambda, const double* sample_y, const double* wall_velocity) {
  API_BEGIN
  NSFEM_REQUIRE(ctx, "null context");
  NSFEM_REQUIRE(law == 0 || law == 1 || law == 2, "wall model: unknown law (0 none, 1 Werner-Wengle, 2 Reichardt)");
  NSFEM_REQUIRE(n_facets >= 0, "wall model: n_facets < 0");
  nsfem_ctx::WallModel& W = ctx->wm;
  WallModelDev& d = W.dev;
  if (law == 0 || n_facets == 0) {
    if (d.law != 0) ++W.epoch;
    d.law = 0;
    d.n_facets = d.n_nodes = 0;
    W.h_int.clear();
    W.h_dbl.clear();
  } else {
    NSFEM_REQUIRE(!ctx->comm, "wall model: contexts with a communicator (partitioned meshes) are not supported");
    NSFEM_REQUIRE(params, "wall model: the law needs its parameters");
    NSFEM_REQUIRE(facet_cell && facet_local && sample_cell && sample_lambda && sample_y, "null argument");
    double p[4] = {0.0, 0.0, 0.0, 0.0}, start[3] = {8.3, 1.0 / (1.0 + 1.0 / 7.0), std::pow(8.3, 2.0 / (1.0 - 1.0 / 7.0))};
    if (law == 1) {
      NSFEM_REQUIRE(std::isfinite(params[0]) && params[0] > 0.0, "Werner-Wengle: A must be finite and > 0");
      NSFEM_REQUIRE(std::isfinite(params[1]) && params[1] > 0.0 && params[1] < 1.0,
                    "Werner-Wengle: B must be finite and in (0, 1)");
      start[0] = params[0];
      start[1] = 1.0 / (1.0 + params[1]);
      start[2] = std::pow(params[0], 2.0 / (1.0 - params[1]));
    } else {
      NSFEM_REQUIRE(std::isfinite(params[0]) && params[0] > 0.0, "Reichardt: kappa must be finite and > 0");
      NSFEM_REQUIRE(std::isfinite(params[1]) && params[1] >= 0.0, "Reichardt: C must be finite and >= 0");
    }
    p[0] = params[0];
    p[1] = params[1];
    const int dim = ctx->mesh.dim, nv = dim + 1, nq = wall_model_points(dim), nf2 = wall_model_facet_nodes(dim);
    const int nl2 = dim == 2 ? 6 : 10;
    const size_t nf = (size_t)n_facets;
    for (size_t f = 0; f < nf; ++f) {
      NSFEM_REQUIRE(facet_cell[f] >= 0 && facet_cell[f] < ctx->mesh.n_cells, "wall model: facet cell out of range");
      NSFEM_REQUIRE(facet_local[f] >= 0 && facet_local[f] <= dim, "wall model: local facet index out of range");
      for (int q = 0; q < nq; ++q) {
        const size_t fq = f * nq + q;
        NSFEM_REQUIRE(sample_cell[fq] >= 0 && sample_cell[fq] < ctx->mesh.n_cells, "wall model: sample cell out of range");
        NSFEM_REQUIRE(std::isfinite(sample_y[fq]) && sample_y[fq] > 0.0, "wall model: wall distance must be finite and > 0");
        for (int v = 0; v < nv; ++v)
          NSFEM_REQUIRE(std::isfinite(sample_lambda[fq * nv + v]), "wall model: non-finite sample coordinate");
      }
      for (int a = 0; a < dim && wall_velocity; ++a)
        NSFEM_REQUIRE(std::isfinite(wall_velocity[f * dim + a]), "wall model: non-finite wall velocity");
    }
    // what the call took, in one integer and one double vector: the same data again changes nothing
    std::vector<int32_t> h_int;
    std::vector<double> h_dbl;
    h_int.push_back(law);
    h_int.push_back(wall_velocity ? 1 : 0);
    h_int.insert(h_int.end(), facet_cell, facet_cell + nf);
    h_int.insert(h_int.end(), facet_local, facet_local + nf);
    h_int.insert(h_int.end(), sample_cell, sample_cell + nf * nq);
    h_dbl.insert(h_dbl.end(), p, p + 4);
    h_dbl.insert(h_dbl.end(), sample_lambda, sample_lambda + nf * nq * nv);
    h_dbl.insert(h_dbl.end(), sample_y, sample_y + nf * nq);
    if (wall_velocity) h_dbl.insert(h_dbl.end(), wall_velocity, wall_velocity + nf * dim);
    const bool same = d.law != 0 && h_int == W.h_int && h_dbl.size() == W.h_dbl.size() &&
                      std::memcmp(h_dbl.data(), W.h_dbl.data(), sizeof(double) * h_dbl.size()) == 0;
    if (!same) {
      // the node CSR: (node, facet NF2 + local) pairs sorted by node, then by facet
      std::vector<std::pair<int32_t, int32_t>> pairs;
      pairs.reserve(nf * nf2);
      const int ends2[3][2] = {{1, 2}, {0, 2}, {0, 1}};                               // UFC edges
      const int ends3[6][2] = {{2, 3}, {1, 3}, {1, 2}, {0, 3}, {0, 2}, {0, 1}};
      for (size_t f = 0; f < nf; ++f) {
        const int32_t* p2 = &ctx->h_p2map[(size_t)facet_cell[f] * nl2];
        const int opp = facet_local[f];
        int t = 0;
        for (int k = 0; k < nl2; ++k) {
          bool on = k != opp;
          if (k >= nv) {
            const int* e = dim == 2 ? ends2[k - nv] : ends3[k - nv];
            on = e[0] != opp && e[1] != opp;
          }
          if (on) pairs.emplace_back(p2[k], (int32_t)(f * nf2 + t++));
        }
      }
      std::sort(pairs.begin(), pairs.end());
      std::vector<int32_t> nodes, nptr, entry;
      for (size_t i = 0; i < pairs.size(); ++i) {
        if (i == 0 || pairs[i].first != pairs[i - 1].first) {
          nodes.push_back(pairs[i].first);
          nptr.push_back((int32_t)i);
        }
        entry.push_back(pairs[i].second);
      }
      nptr.push_back((int32_t)pairs.size());
      hipStream_t s = ctx->stream;
      d.law = 0;                                  // (off until everything is resident)
      d.fcell.upload(facet_cell, nf, s);
      d.flocal.upload(facet_local, nf, s);
      d.scell.upload(sample_cell, nf * nq, s);
      d.slam.upload(sample_lambda, nf * nq * nv, s);
      d.sy.upload(sample_y, nf * nq, s);
      if (wall_velocity) d.uw.upload(wall_velocity, nf * dim, s);
      d.nodes.upload(nodes.data(), nodes.size(), s);
      d.nptr.upload(nptr.data(), nptr.size(), s);
      d.entry.upload(entry.data(), entry.size(), s);
      NSFEM_HIP(hipStreamSynchronize(s));         // the host vectors die with the call
      if (d.fvec.n != nf * nf2 * dim) d.fvec.alloc(nf * nf2 * dim);
      if (d.rows.n != nf * wall_model_row(dim)) d.rows.alloc(nf * wall_model_row(dim));
      d.have_uw = wall_velocity != nullptr;
      d.n_facets = n_facets;
      d.n_nodes = (int32_t)nodes.size();
      std::memcpy(d.p, p, sizeof(p));
      std::memcpy(d.start, start, sizeof(start));
      d.law = law;
      W.h_int.swap(h_int);
      W.h_dbl.swap(h_dbl);
      // (the stored explicit vectors belong to the model they were evaluated with; the model enters no captured
      // Krylov body -- its launches precede the solve --, so graph_epoch stays)
      ++W.epoch;
    }
  }
  API_END(ctx)
}

static void wall_model_require(nsfem_ctx* ctx, int velocity_slot) {
  NSFEM_REQUIRE(!ctx->comm, "wall model: contexts with a communicator (partitioned meshes) are not supported");
  NSFEM_REQUIRE(ctx->wm.dev.law != 0, "wall model: no model set (nsfem_set_wall_model)");
  // (nu = coef[2] is always a number: nsfem_set_coeffs refuses a viscous coefficient of None)
  require_velocity_slot(velocity_slot);
}

extern "C" int nsfem_wall_model_residual(nsfem_ctx* ctx, int velocity_slot, double weight, double* out_host) {
  API_BEGIN
  NSFEM_REQUIRE(ctx && out_host, "null argument");
  wall_model_require(ctx, velocity_slot);
  require_finite_weight(weight);
  hipStream_t s = ctx->stream;
  const int64_t nv = nvel(ctx);
  hook_to_host(ctx, nv, out_host, [&](double* out) {
    NSFEM_HIP(hipMemsetAsync(out, 0, sizeof(double) * nv, s));
    launch_wall_model_facets(s, ctx->mesh, ctx->wm.dev, ctx->state[velocity_slot].p, ctx->coef[2], weight);
    launch_wall_model_gather(s, ctx->mesh, ctx->wm.dev, 0.0, out, nullptr);
    ++ctx->wm.launches;
  });
  API_END(ctx)
}

extern "C" int nsfem_wall_model_facets(nsfem_ctx* ctx, int velocity_slot, double* out) {
  API_BEGIN
  NSFEM_REQUIRE(ctx && out, "null argument");
  wall_model_require(ctx, velocity_slot);
  hipStream_t s = ctx->stream;
  const WallModelDev& d = ctx->wm.dev;
  // (the facet vectors land in the model's own buffer, which every user fills before it reads; the resident order is
  // the input order)
  launch_wall_model_facets(s, ctx->mesh, d, ctx->state[velocity_slot].p, ctx->coef[2], 1.0);
  ++ctx->wm.launches;
  NSFEM_HIP(hipMemcpyAsync(out, d.rows.p, sizeof(double) * (size_t)d.n_facets * wall_model_row(ctx->mesh.dim),
                           hipMemcpyDeviceToHost, s));
  NSFEM_HIP(hipStreamSynchronize(s));
  API_END(ctx)
}

extern "C" int nsfem_wall_model_info(nsfem_ctx* ctx, int64_t out[4]) {
  API_BEGIN
  NSFEM_REQUIRE(ctx && out, "null argument");
  out[0] = ctx->wm.dev.law != 0 ? ctx->wm.dev.n_facets : 0;
  out[1] = ctx->wm.launches;
  out[2] = ctx->wm.recomputed;
  out[3] = ctx->wm.dev.law;
  API_END(ctx)
}

// ---------------------------------------------------------------- heated bodies
extern "C" int nsfem_set_body_temperatures(nsfem_ctx* ctx, int32_t n, const int32_t* thermal, const double* temperature,
                                           double eta_T) {
  API_BEGIN
  NSFEM_REQUIRE(ctx, "null context");
  nsfem_ctx::Bodies& b = ctx->bodies;
  ThermalTable t;
  if (n != 0) {
    NSFEM_REQUIRE(b.cur.n > 0, "heated bodies: no body set (nsfem_set_bodies)");
    NSFEM_REQUIRE(n == b.cur.n, "heated bodies: nsfem_set_body_temperatures with another count than bodies set");
    NSFEM_REQUIRE(thermal && temperature, "heated bodies: null flag or temperature array");
    NSFEM_REQUIRE(std::isfinite(eta_T) && eta_T > 0.0, "heated bodies: eta_T must be finite and > 0");
    t.n = n;
    for (int s = 0; s < n; ++s) {
      NSFEM_REQUIRE(thermal[s] == 0 || thermal[s] == 1, "heated bodies: flag must be 0 (passive) or 1 (thermal)");
      NSFEM_REQUIRE(std::isfinite(temperature[s]), "heated bodies: temperature not finite");
      t.flag[s] = thermal[s];
      t.temperature[s] = thermal[s] ? temperature[s] : 0.0;      // (a passive body's temperature is read nowhere)
    }
    t.inv_eta = 1.0 / eta_T;
  }
  store_thermal(b, t, n != 0);
  API_END(ctx)
}

static void heated_require(nsfem_ctx* ctx, int scalar_slot) {
  NSFEM_REQUIRE(!ctx->comm, "immersed bodies: contexts with a communicator (partitioned meshes) are not supported");
  NSFEM_REQUIRE(ctx->bodies.cur.n != 0, "immersed bodies: no body set (nsfem_set_bodies)");
  NSFEM_REQUIRE(ctx->bodies.have_thermal, "heated bodies: no temperatures set (nsfem_set_body_temperatures)");
  require_scalar_slot(scalar_slot);
}

// The scalar explicit vector of a level in ONE element launch (plus k_scalar_gather):
//   out = weight [ C(u) T  + D(u, T)  + H(T) ]
// D (subgrid heat flux, nsfem_set_scalar_sgs / nsfem_set_scalar_sgs_dynamic) with sgs.law != 0: the SGS = law kernels
// (8: the dynamic diffusivity, whose constant is formed here on the pair (u, T) first); H (heated bodies,
// nsfem_set_body_temperatures with at least one flag 1) with a pose: that of the level -- cur for T1, prev for a T2
// vector formed afresh -- and the fused PENAL kernels.  pose null and sgs.law 0: the launches of old.
// in_step: the launch is one of nsfem_step_scalar_imex and counts as a convection launch (the hooks' never did)
static void scalar_explicit_launch(nsfem_ctx* c, const double* u, const double* T, double weight, int form,
                                   const BodyTable* pose, double* out, const ScalarSgsArgs& sgs_in, bool in_step) {
  const ScalarBodies hb{pose ? *pose : c->bodies.cur, c->bodies.thermal};
  ScalarSgsArgs sgs = sgs_in;
  // (dynamic diffusivity: C_theta of THIS level pair, three launches before the element launch)
  if (sgs.law == 8) sgs.cthv = dynamic_run(c, u, T);
  launch_scalar_convection(c->stream, c->mesh, u, T, weight, form, pose ? &hb : nullptr, out, sgs);
  if (pose) ++c->bodies.fused_launches;
  if (in_step) ++c->sc.conv_launches;
  if (sgs.law != 0) ++c->sc.sgs_launches;
}

extern "C" int nsfem_body_scalar_residual(nsfem_ctx* ctx, int velocity_slot, int scalar_slot, int form, double weight,
                                          int pose, double* out_host) {
  API_BEGIN
  NSFEM_REQUIRE(ctx && out_host, "null argument");
  heated_require(ctx, scalar_slot);
  require_velocity_slot(velocity_slot);
  require_scalar_form(form);
  NSFEM_REQUIRE(pose == 0 || pose == 1, "heated bodies: pose must be 0 (t^n) or 1 (t^(n-1))");
  require_finite_weight(weight);
  ensure_scalar_slot(ctx, scalar_slot);
  hook_to_host(ctx, ctx->mesh.n_p2, out_host, [&](double* out) {
    scalar_explicit_launch(ctx, ctx->state[velocity_slot].p, ctx->state[scalar_slot].p, weight, form,
                           pose == 0 ? &ctx->bodies.cur : &ctx->bodies.prev, out, ScalarSgsArgs{}, false);
  });
  API_END(ctx)
}

extern "C" int nsfem_body_heat(nsfem_ctx* ctx, int scalar_slot, double* out) {
  API_BEGIN
  NSFEM_REQUIRE(ctx && out, "null argument");
  heated_require(ctx, scalar_slot);
  hipStream_t s = ctx->stream;
  ensure_scalar_slot(ctx, scalar_slot);
  const PartialsWork w(ctx->bodies.heat_work, (size_t)ctx->bodies.cur.n * 3, kBodyParts);
  launch_body_heat(s, ctx->mesh, ctx->state[scalar_slot].p, ctx->bodies.cur, ctx->bodies.thermal, w.parts, w.res);
  w.read_back(s, out);
  API_END(ctx)
}

extern "C" int nsfem_body_heat_info(nsfem_ctx* ctx, int64_t out[4]) {
  API_BEGIN
  NSFEM_REQUIRE(ctx && out, "null argument");
  out[0] = ctx->bodies.n_thermal;
  out[1] = ctx->bodies.fused_launches;
  out[2] = ctx->bodies.thermal_recomputed;
  out[3] = 0;
  API_END(ctx)
}

// ---------------------------------------------------------------- IMEX scalar transport
extern "C" int nsfem_set_scalar(nsfem_ctx* ctx, double diffusivity, const double* buoyancy, int convective_form) {
  API_BEGIN
  NSFEM_REQUIRE(ctx, "null context");
  NSFEM_REQUIRE(!ctx->comm, "scalar transport: contexts with a communicator (partitioned meshes) are not supported");
  NSFEM_REQUIRE(std::isfinite(diffusivity) && diffusivity >= 0.0, "scalar transport: diffusivity must be finite and >= 0");
  NSFEM_REQUIRE(convective_form == 0 || convective_form == 1,
                "scalar transport: convective form must be 0 (standard) or 1 (skew-symmetric)");
  nsfem_ctx::Scalar& sc = ctx->sc;
  bool buoyant = false;
  for (int d = 0; d < 3; ++d) {
    const double b = buoyancy && d < ctx->mesh.dim ? buoyancy[d] : 0.0;
    NSFEM_REQUIRE(std::isfinite(b), "scalar transport: buoyancy vector must be finite");
    sc.b[d] = b;
    buoyant = buoyant || b != 0.0;
  }
  sc.buoyant = buoyant;
  sc.kappa = diffusivity;
  sc.form = convective_form;
  sc.configured = true;
  API_END(ctx)
}

// Subgrid heat flux: kappa_x = nu_x / Pr_t of the subgrid law (1 Smagorinsky, 4 WALE, 5 Vreman) under the gradients of
// the scalar, explicit, inside the convection launch (k_scalar_conv_cell<FORM, PENAL, law>).  kappa K stays in the
// matrix: no rebuild, no new solve
extern "C" int nsfem_set_scalar_sgs(nsfem_ctx* ctx, double prandtl_t) {
  API_BEGIN
  NSFEM_REQUIRE(ctx, "null context");
  NSFEM_REQUIRE(!ctx->comm, "scalar transport: contexts with a communicator (partitioned meshes) are not supported");
  NSFEM_REQUIRE(std::isfinite(prandtl_t) && prandtl_t >= 0.0,
                "subgrid heat flux: Pr_t must be 0 (off) or finite and > 0");
  nsfem_ctx::Scalar& sc = ctx->sc;
  NSFEM_REQUIRE(prandtl_t == 0.0 || !sc.dynflux.on,
                "subgrid heat flux: a fixed Pr_t while the dynamic diffusivity is on (nsfem_set_scalar_sgs_dynamic)");
  // (the stored vectors belong to the Pr_t they were evaluated with; the term enters no captured Krylov body)
  if (prandtl_t != sc.prandtl_t) ++sc.sgs_epoch;
  sc.prandtl_t = prandtl_t == 0.0 ? 0.0 : prandtl_t;
  API_END(ctx)
}

// Dynamic subgrid heat flux: kappa_x = c_K Delta_K^2 gamma with C_theta from the Germano identity of the scalar flux
// (dynamic_run on the pair), no Pr_t.  The stored scalar vector belongs to the switch and the clip it was formed with
extern "C" int nsfem_set_scalar_sgs_dynamic(nsfem_ctx* ctx, int enable, double ctheta_max) {
  API_BEGIN
  NSFEM_REQUIRE(ctx, "null context");
  NSFEM_REQUIRE(!ctx->comm, "scalar transport: contexts with a communicator (partitioned meshes) are not supported");
  NSFEM_REQUIRE(enable == 0 || enable == 1, "dynamic subgrid heat flux: enable must be 0 or 1");
  nsfem_ctx::Scalar& sc = ctx->sc;
  if (enable) {
    NSFEM_REQUIRE(std::isfinite(ctheta_max) && ctheta_max > 0.0,
                  "dynamic subgrid heat flux: ctheta_max must be finite and > 0");
    NSFEM_REQUIRE(sc.prandtl_t == 0.0,
                  "dynamic subgrid heat flux: a fixed Pr_t is on (nsfem_set_scalar_sgs); switch it off first");
    NSFEM_REQUIRE(!lagrangian_on(ctx),
                  "dynamic subgrid heat flux: Lagrangian averaging is on (nsfem_set_dynamic_averaging); a Lagrangian "
                  "C_theta is not supported");
  }
  nsfem_ctx::Scalar::DynamicFlux& F = sc.dynflux;
  const bool on = enable != 0;
  const double cmax = on ? ctheta_max : 0.0;
  if (on != F.on || cmax != F.ctheta_max) ++sc.sgs_epoch;
  F.on = on;
  F.ctheta_max = cmax;
  API_END(ctx)
}

// what the convection launches take: the law, its constant (C_s, C_w, c) and 1 / Pr_t while the term is on; law 8
// alone with the dynamic diffusivity (its vertex field is formed by scalar_explicit_launch); nothing otherwise
static ScalarSgsArgs scalar_sgs_args(const nsfem_ctx* c) {
  ScalarSgsArgs a;
  if (c->sc.dynflux.on) {
    a.law = 8;
    return a;
  }
  if (c->sc.prandtl_t > 0.0) {
    a.c0 = c->visc.p[0];
    a.inv_prt = 1.0 / c->sc.prandtl_t;
    a.law = c->visc.law;
  }
  return a;
}

static void scalar_sgs_require_law(const nsfem_ctx* c) {
  const int law = c->visc.law;
  NSFEM_REQUIRE(c->sc.prandtl_t == 0.0 || is_subgrid_law(law),
                "subgrid heat flux: Pr_t is set but the viscosity law is not 1 (Smagorinsky), 4 (WALE) or 5 (Vreman) "
                "(nsfem_set_viscosity_law)");
  NSFEM_REQUIRE(!c->sc.dynflux.on || law == 8,
                "dynamic subgrid heat flux: the switch is on but the viscosity law is not 8 (dynamic Smagorinsky) "
                "(nsfem_set_viscosity_law)");
}

// A = alpha0/k M + gamma0 kappa K, rebuilt only when one of the three numbers changed
static void ensure_scalar_matrix(nsfem_ctx* c) {
  nsfem_ctx::Scalar& sc = c->sc;
  hipStream_t s = c->stream;
  const double a = c->alpha[0] / c->k, g0 = c->imex_gamma[0];
  if (!sc.A.vals.p) sc.A.init(&c->p22, 1, 1, s);
  ensure_dict22(c);
  const StencilDict* dict = c->dict22.n_stencils > 0 ? &c->dict22 : nullptr;
  const bool rebuild = !(a == sc.built_a && g0 == sc.built_g0 && sc.kappa == sc.built_kappa) || sc.A.dict != dict;
  if (!rebuild) return;
  sc.A.dict = dict;
  launch_scale_combine(s, c->p22.nnz, a, c->M2.vals.p, g0 * sc.kappa, c->K2.vals.p, sc.A.vals.p);
  sc.A.sell_update(s);
  sc.built_a = a;
  sc.built_g0 = g0;
  sc.built_kappa = sc.kappa;
  ++sc.matrix_builds;
  sc.dinv_dirty = true;
}

static void scalar_require_supported(nsfem_ctx* c) {
  NSFEM_REQUIRE(c->sc.configured, "nsfem_set_scalar has not been called");
  NSFEM_REQUIRE(!c->comm, "scalar transport: contexts with a communicator (partitioned meshes) are not supported");
  imex_require_supported(c);
}

extern "C" int nsfem_step_scalar_imex(nsfem_ctx* ctx, const nsfem_krylov_opts* opts, nsfem_solve_info* info) {
  nsfem_solve_info local;
  API_BEGIN
  NSFEM_REQUIRE(ctx, "null context");
  scalar_require_supported(ctx);
  scalar_sgs_require_law(ctx);
  nsfem_ctx::Scalar& sc = ctx->sc;
  hipStream_t s = ctx->stream;
  const int64_t n = ctx->mesh.n_p2;
  for (int slot : {NSFEM_T0, NSFEM_T1, NSFEM_T2, NSFEM_TCONV_1, NSFEM_TCONV_2}) ensure_scalar_slot(ctx, slot);
  if (!sc.rhs.p) {
    sc.dinv_dirty = true;
    sc.rhs.alloc((size_t)n);
    sc.tmp.alloc((size_t)n);
    sc.dinv.alloc((size_t)n);
  }
  if (!sc.mask.p) {
    sc.mask.alloc((size_t)n);
    sc.mask.zero(s);
  }
  ensure_scalar_matrix(ctx);
  const double k = ctx->k, *al = ctx->alpha, *ga = ctx->imex_gamma;
  const double b0 = ctx->imex_beta[0], b1 = ctx->imex_beta[1];
  double *T1 = ctx->state[NSFEM_T1].p, *T2 = ctx->state[NSFEM_T2].p;
  double *rhs = sc.rhs.p, *tmp = sc.tmp.p;
  // rhs = M ((alpha1 T1 + alpha2 T2)/k - q) + kappa K (gamma1 T1 + gamma2 T2)
  if (sc.have_source) launch_lincomb3(s, n, al[1] / k, T1, al[2] / k, T2, -1.0, ctx->state[NSFEM_T_SOURCE].p, tmp);
  else launch_axpby(s, n, al[1] / k, T1, al[2] / k, T2, tmp);
  launch_spmv(s, ctx->M2, 1, tmp, rhs, nullptr, MASK_NONE);
  if (sc.kappa != 0.0 && (ga[1] != 0.0 || ga[2] != 0.0)) {
    launch_axpby(s, n, ga[1], T1, ga[2], T2, tmp);
    launch_spmv_axpy(s, ctx->K2, 1, sc.kappa, tmp, rhs, nullptr);
  }
  // beta1 C(u2) T2: the vector the previous step stored (beta0' C(u1) T1 then), unless a level, a stored vector or
  // a component of its key changed under it: the form; with heated bodies the thermal table or, while a body is
  // thermal, the body set; with the subgrid heat flux Pr_t or, while the term is on, the viscosity law or its
  // parameters.  What the launches form: scalar_explicit_launch
  nsfem_ctx::Bodies& bd = ctx->bodies;
  const bool heated = bd.n_thermal > 0 && bd.cur.n > 0;
  const ScalarSgsArgs sgs = scalar_sgs_args(ctx);
  const nsfem_ctx::Scalar::Key now = nsfem_ctx::Scalar::Key::of(*ctx);
  double f2 = 0.0;
  if (b1 != 0.0) {
    const bool usable = sc.conv2_valid && sc.conv2_weight != 0.0 && sc.conv_key.same_form(now);
    const bool same_heat = sc.conv_key.same_heat(now, heated), same_sgs = sc.conv_key.same_sgs(now, sgs.law != 0);
    if (usable && same_heat && same_sgs) {
      ++sc.conv_reuses;
    } else {
      if (usable && !same_heat) ++bd.thermal_recomputed;
      if (usable && !same_sgs) ++sc.sgs_recomputed;
      scalar_explicit_launch(ctx, ctx->state[NSFEM_U2].p, T2, 1.0, sc.form, heated ? &bd.prev : nullptr,
                             ctx->state[NSFEM_TCONV_2].p, sgs, true);
      sc.conv2_weight = 1.0;
      sc.conv2_valid = true;
    }
    f2 = b1 / sc.conv2_weight;
  }
  // beta0 C(u1) T1: beta0 rides in the kernel's weight, the node sums are the stored copy
  scalar_explicit_launch(ctx, ctx->state[NSFEM_U1].p, T1, b0, sc.form, heated ? &bd.cur : nullptr,
                         ctx->state[NSFEM_TCONV_1].p, sgs, true);
  sc.conv1_fresh = true;
  sc.conv1_weight = b0;
  sc.conv_key = now;
  if (b1 != 0.0) launch_lincomb3(s, n, -1.0, rhs, -1.0, ctx->state[NSFEM_TCONV_1].p, -f2, ctx->state[NSFEM_TCONV_2].p, rhs);
  else launch_axpby(s, n, -1.0, rhs, -1.0, ctx->state[NSFEM_TCONV_1].p, rhs);
  // Dirichlet rows T_i = g_i; start vector T1 with the Dirichlet values (as the IMEX diffusion step)
  double* x = ctx->state[NSFEM_T0].p;
  launch_set_values(s, sc.nbc, sc.bc_dofs.p, sc.bc_vals.p, rhs);
  NSFEM_HIP(hipMemcpyAsync(x, T1, sizeof(double) * n, hipMemcpyDeviceToDevice, s));
  launch_set_values(s, sc.nbc, sc.bc_dofs.p, sc.bc_vals.p, x);
  LinOp op;
  op.A = &sc.A;
  op.nv = 1;
  op.rowmask = sc.mask.p;
  op.maskmode = MASK_ZERO;
  op.dinv = sc.dinv.p;
  op.graph_epoch = ctx->graph_epoch;
  if (sc.dinv_dirty) {              // (the matrix and the mask change only on a rebuild / a new Dirichlet set)
    launch_inv_diag(s, sc.A, 1, sc.mask.p, sc.dinv.p);
    sc.dinv_dirty = false;
  }
  sc.dict_used = sc.A.dict_ready && sc.A.dict->exact ? 1 : 0;
  nsfem_krylov_opts ko;
  if (opts) ko = *opts;
  else { ko.rtol = 1e-12; ko.atol = 0.0; ko.max_iter = 20000; ko.precond = 0; ko.check_every = 1; ko.first_check = 0; }
  NSFEM_REQUIRE(ko.precond == 0, "scalar transport: precond must be 0 (Jacobi)");
  nsfem_solve_info& si = info ? *info : local;
  ctx->kw.ensure(nvel(ctx));
  int rc = pcg(s, ctx->kw, op, rhs, x, hinted(ko, ctx->hint_sc), si, false);
  note_solve(ctx->hint_sc, si, ko, ctx->kw.last_target);
  if (rc != NSFEM_OK) throw Error(rc, "CG failed in the scalar transport step");
  API_END(ctx)
}

// The two test hooks of the scalar element launch: scalar_explicit_launch on a work vector.  all_terms false: C(u) T
// alone, no bodies and no subgrid term; true: what ONE launch of the step forms for a level, weight [C(u) T + D(u, T)
// (+ H(T))] -- D while the subgrid heat flux is on, H while a body is thermal (pose: prev for the level T2, cur
// otherwise, as the step takes them)
static void scalar_hook(nsfem_ctx* ctx, int velocity_slot, int scalar_slot, int form, double weight, bool all_terms,
                        double* out_host) {
  NSFEM_REQUIRE(ctx && out_host, "null argument");
  NSFEM_REQUIRE(!ctx->comm, "scalar transport: contexts with a communicator (partitioned meshes) are not supported");
  require_velocity_slot(velocity_slot);
  require_scalar_slot(scalar_slot);
  require_scalar_form(form);
  require_finite_weight(weight);
  if (all_terms) scalar_sgs_require_law(ctx);
  ensure_scalar_slot(ctx, scalar_slot);
  nsfem_ctx::Bodies& bd = ctx->bodies;
  const BodyTable* pose = scalar_slot == NSFEM_T2 ? &bd.prev : &bd.cur;
  if (!all_terms || bd.n_thermal == 0 || bd.cur.n == 0) pose = nullptr;
  hook_to_host(ctx, ctx->mesh.n_p2, out_host, [&](double* out) {
    scalar_explicit_launch(ctx, ctx->state[velocity_slot].p, ctx->state[scalar_slot].p, weight, form, pose, out,
                           all_terms ? scalar_sgs_args(ctx) : ScalarSgsArgs{}, false);
  });
}

extern "C" int nsfem_scalar_convection(nsfem_ctx* ctx, int velocity_slot, int scalar_slot, int form, double weight,
                                       double* out_host) {
  API_BEGIN
  scalar_hook(ctx, velocity_slot, scalar_slot, form, weight, false, out_host);
  API_END(ctx)
}

extern "C" int nsfem_scalar_explicit(nsfem_ctx* ctx, int velocity_slot, int scalar_slot, int form, double weight,
                                     double* out_host) {
  API_BEGIN
  scalar_hook(ctx, velocity_slot, scalar_slot, form, weight, true, out_host);
  API_END(ctx)
}

extern "C" int nsfem_scalar_sgs_info(nsfem_ctx* ctx, int64_t out[4]) {
  API_BEGIN
  NSFEM_REQUIRE(ctx && out, "null argument");
  out[0] = ctx->sc.prandtl_t > 0.0 ? 1 : 0;
  out[1] = ctx->sc.sgs_launches;
  out[2] = ctx->sc.sgs_recomputed;
  out[3] = 0;
  API_END(ctx)
}

// ---- dynamic subgrid heat flux: the constant as output / test hook, the cell means of kappa_x, counters
static void scalar_dynamic_require(nsfem_ctx* ctx, int velocity_slot, int scalar_slot) {
  NSFEM_REQUIRE(!ctx->comm, "scalar transport: contexts with a communicator (partitioned meshes) are not supported");
  NSFEM_REQUIRE(ctx->sc.dynflux.on, "dynamic subgrid heat flux: the switch is off (nsfem_set_scalar_sgs_dynamic)");
  scalar_sgs_require_law(ctx);
  require_velocity_slot(velocity_slot);
  require_scalar_slot(scalar_slot);
  ensure_scalar_slot(ctx, scalar_slot);
}

extern "C" int nsfem_scalar_dynamic_constant(nsfem_ctx* ctx, int velocity_slot, int scalar_slot, double* ctheta_groups,
                                             double* sums, double* vertices) {
  API_BEGIN
  NSFEM_REQUIRE(ctx && ctheta_groups, "null argument");
  scalar_dynamic_require(ctx, velocity_slot, scalar_slot);
  dynamic_run(ctx, ctx->state[velocity_slot].p, ctx->state[scalar_slot].p);
  dynamic_read_back(ctx, ctx->sc.dynflux.buf, ctheta_groups, sums, vertices);
  API_END(ctx)
}

extern "C" int nsfem_scalar_diffusivity_cells(nsfem_ctx* ctx, int velocity_slot, int scalar_slot, double* out_host) {
  API_BEGIN
  NSFEM_REQUIRE(ctx && out_host, "null argument");
  scalar_dynamic_require(ctx, velocity_slot, scalar_slot);
  hipStream_t s = ctx->stream;
  const double* u = ctx->state[velocity_slot].p;
  // (the law-8 MEAN instantiation of the viscosity kernel with C_theta in the place of C_s^2; the cell means land in
  // the element buffer, which every user fills before it reads)
  const double* cthv = dynamic_run(ctx, u, ctx->state[scalar_slot].p);
  launch_viscosity_cells(s, ctx->mesh, u, 1.0, 8, ctx->visc.p, true, cthv);
  NSFEM_HIP(hipMemcpyAsync(out_host, ctx->mesh.rbuf.p, sizeof(double) * ctx->mesh.n_cells, hipMemcpyDeviceToHost, s));
  NSFEM_HIP(hipStreamSynchronize(s));
  API_END(ctx)
}

extern "C" int nsfem_scalar_dynamic_info(nsfem_ctx* ctx, int64_t out[4]) {
  API_BEGIN
  NSFEM_REQUIRE(ctx && out, "null argument");
  const nsfem_ctx::Scalar::DynamicFlux& F = ctx->sc.dynflux;
  out[0] = F.on ? 1 : 0;
  out[1] = F.buf.runs;
  out[2] = F.buf.launches;
  out[3] = dynamic_bytes(F.buf);
  API_END(ctx)
}

extern "C" int nsfem_scalar_info(nsfem_ctx* ctx, int64_t out[4]) {
  API_BEGIN
  NSFEM_REQUIRE(ctx && out, "null argument");
  out[0] = ctx->sc.matrix_builds;
  out[1] = ctx->sc.conv_launches;
  out[2] = ctx->sc.conv_reuses;
  out[3] = ctx->sc.dict_used;
  API_END(ctx)
}

// ---------------------------------------------------------------- monolithic BDF
// mixed operator  [[J, -c_p D^T], [-c_p D, 0]]  with identity rows on Dirichlet dofs
void nsfem_ctx::MixedOp::apply(hipStream_t s, const double* x, double* y) {
  const int64_t nv = nvel(c), np = npre(c);
  const double cp = c->coef[1];
  const bool dist = c->distributed();
  if (dist) {       // ghost entries of the input (in place: the Krylov vectors keep consistent ghosts)
    if (!c->mf_active) c->comm->exchange(s, c->halo_p2, const_cast<double*>(x), c->mesh.dim);
    c->comm->exchange(s, c->halo_p1, const_cast<double*>(x) + nv, 1);
  }
  if (c->mf_active) c->mom_mf.apply(s, x, y);          // (exchanges the velocity part itself)
  else launch_spmv(s, c->J, 1, x, y, c->mask_v.p, MASK_IDENTITY);
  launch_spmv_axpy(s, c->DT, 1, -cp, x + nv, y, c->mask_v.p, 1);       // (Jacobian product: dictionary copies allowed)
  launch_spmv_scaled(s, c->Dv, 1, -cp, x, y + nv, 1);
  launch_copy_at(s, c->nbc_p, c->bc_p_dofs.p, x + nv, y + nv);
  if (c->ghost_p.p) launch_zero_ghost(s, np, c->mask_p.p, y + nv);
}

// upper block-triangular preconditioner with the Cahouet-Chabard Schur approximation
//   z_p = -(1/c_p^2) (c_v M_p^{-1} + alpha0/k A_p^{+}) r_p ;  z_u = F^{-1} (r_u + c_p D^T z_p)
// F^{-1}, A_p^{+}: one multigrid V-cycle each;  M_p^{-1}: 4 Chebyshev-Jacobi steps
void nsfem_ctx::BlockPrec::apply(hipStream_t s, const double* r, double* z) {
  const int64_t nv = nvel(c), np = npre(c);
  const double cp = c->coef[1], cv = c->coef[2], a = c->alpha[0] / c->k + c->prec_shift;
  const double* rp = r + nv;
  double* zp = z + nv;
  c->mg_s.apply(s, rp, c->tmp_p.p);
  c->mg_m.apply(s, rp, c->rhs_p.p);
  launch_axpby(s, np, -a / (cp * cp), c->tmp_p.p, -cv / (cp * cp), c->rhs_p.p, zp);
  launch_copy_at(s, c->nbc_p, c->bc_p_dofs.p, rp, zp);
  if (c->distributed()) c->comm->exchange(s, c->halo_p1, zp, 1);
  NSFEM_HIP(hipMemcpyAsync(c->tmp_v.p, r, sizeof(double) * nv, hipMemcpyDeviceToDevice, s));
  launch_spmv_axpy(s, c->DT, 1, cp, zp, c->tmp_v.p, c->mask_v.p, 1);   // (preconditioner)
  if (c->ghost_p.p) launch_zero_ghost(s, np, c->mask_p.p, zp);      // keep ghost entries out of the dots
  c->mg_v.apply(s, c->tmp_v.p, z);        // (identity rows on the Dirichlet dofs: Multigrid::identity_rows)
}

// F_u = L u + g + c_c conv(u) - c_p D^T p ; F_p = -c_p D u ; Dirichlet rows x_i - g_i
static double bdf_residual(nsfem_ctx* c) {
  hipStream_t s = c->stream;
  const int64_t nv = nvel(c), np = npre(c);
  double* u = c->state[NSFEM_U0].p;
  double* p = c->state[NSFEM_P].p;
  double* b = c->rhs_m.p;
  momentum_residual_raw(c, u, b);
  launch_spmv_axpy(s, c->DT, 1, -c->coef[1], p, b, nullptr);
  launch_set_bc_residual(s, c->nbc_v, c->bc_v_dofs.p, c->bc_v_vals.p, u, b);
  launch_spmv_scaled(s, c->Dv, 1, -c->coef[1], u, b + nv);
  launch_set_bc_residual(s, c->nbc_p, c->bc_p_dofs.p, c->bc_p_vals.p, p, b + nv);
  if (c->ghost_v.p) {            // owners compute: ghost rows are zero (also for the norm)
    launch_zero_ghost(s, nv, c->mask_v.p, b);
    launch_zero_ghost(s, np, c->mask_p.p, b + nv);
  }
  return global_norm(c, nv + np, b, nullptr);
}

// What every entry to the mixed system does first (nsfem_step_bdf, the explicit seam with NSFEM_SYS_MONOLITHIC, the
// test hook nsfem_monolithic_apply): the checks, the mixed vectors, the operator objects, the dictionary copies of D / D^T
static void monolithic_setup(nsfem_ctx* ctx) {
  NSFEM_REQUIRE(ctx->visc.law == 0, "variable viscosity: only nsfem_step_imex takes a viscosity law (set law 0 first)");
  NSFEM_REQUIRE(ctx->bodies.cur.n == 0, "immersed bodies: only nsfem_step_imex takes bodies (remove them with n = 0 first)");
  NSFEM_REQUIRE(ctx->wm.dev.law == 0, "wall model: only nsfem_step_imex takes a wall model (switch it off with law 0 first)");
  NSFEM_REQUIRE(!ctx->distributed() || ctx->schur_singular < 0 || ctx->schur_additive,
                "partitioned meshes take the algebraic Schur Laplacian as additive rank parts "
                "(nsfem_mg_set_schur_mode)");
  NSFEM_REQUIRE(ctx->mg_built, "the monolithic step needs the multigrid hierarchy "
                               "(block preconditioner): call nsfem_mg_finalize");
  const int64_t nv = nvel(ctx), np = npre(ctx);
  if (!ctx->rhs_m.p) {
    ctx->rhs_m.alloc((size_t)(nv + np));
    ctx->dx_m.alloc((size_t)(nv + np));
  }
  ctx->mixed_op.c = ctx;
  ctx->mixed_op.n = nv + np;
  ctx->block_prec.c = ctx;
  ctx->mom_mf.c = ctx;
  ctx->mom_mf.n = nv;
  ctx->mom_mf.vel_slot = NSFEM_U0;
  ensure_div_dicts(ctx);
}

// What the linear solve of one Newton iteration prepares: the Jacobian about U0 (unless it is applied matrix-free) and
// the three hierarchies of the block preconditioner
static void monolithic_linearise(nsfem_ctx* ctx) {
  if (!ctx->mf_active) momentum_jacobian(ctx, NSFEM_U0);
  mg_refresh(ctx, true);
  mg_refresh_schur(ctx);
}

// MixedOp dx = rhs_m by block-preconditioned BiCGStab from zero; u -= dx, p -= dx.  r: |rhs_m| as bdf_residual has just
// returned it; rhs_dead: the caller recomputes rhs_m before anything reads it again (the Newton loop; not so behind
// nsfem_solve, where nsfem_get_rhs / nsfem_residual_norm may follow)
static int monolithic_solve_update(nsfem_ctx* ctx, double r, bool rhs_dead, const nsfem_krylov_opts& k,
                                   nsfem_solve_info& si) {
  hipStream_t s = ctx->stream;
  const int64_t nv = nvel(ctx), np = npre(ctx);
  LinOp op;
  op.custom = &ctx->mixed_op;
  op.prec = &ctx->block_prec;
  if (ctx->distributed()) op.comm = ctx->comm;        // all-reduce of the partial dot products
  op.graph_epoch = ctx->graph_epoch;
  op.x_zero = true;               // (dx_m is not read: the first update of the solve writes it)
  op.known_bnorm = r;             // |rhs_m| = the Newton residual norm just evaluated (bdf_residual)
  op.b_scratch = rhs_dead;        // (bdf_residual rewrites rhs_m before anything reads it)
  const int rc = bicgstab(s, ctx->kw, op, ctx->rhs_m.p, ctx->dx_m.p, k, si);
  if (rc != NSFEM_OK) return rc;  // (a failed solve leaves the iterate: the caller may resume from it)
  double* u = ctx->state[NSFEM_U0].p;
  double* p = ctx->state[NSFEM_P].p;
  launch_axpby(s, nv, 1.0, u, -1.0, ctx->dx_m.p, u);
  launch_axpby(s, np, 1.0, p, -1.0, ctx->dx_m.p + nv, p);
  return rc;
}

extern "C" int nsfem_step_bdf(nsfem_ctx* ctx, const nsfem_step_opts* opts, nsfem_step_info* info) {
  nsfem_step_info local;
  API_BEGIN
  nsfem_step_info& inf = step_begin(ctx, opts, info, local, true, opts && opts->picard != 0);
  monolithic_setup(ctx);
  momentum_begin_step(ctx, false);
  newton_solve(ctx, opts, inf, "monolithic step", opts->allow_nonconvergence != 0, [&] { return bdf_residual(ctx); },
               [&](double r, const nsfem_krylov_opts& k, nsfem_solve_info& si) {
                 monolithic_linearise(ctx);
                 return monolithic_solve_update(ctx, r, true, k, si);
               });
  ctx->assembled_system = -1;
  API_END(ctx)
}

// The explicit seam for the mixed system (nsfem_assemble / nsfem_solve with NSFEM_SYS_MONOLITHIC; single contexts).
// flags: bit 0 -- a new time step (the step-constant vector g is formed first); bit 1 -- the velocity Jacobian is
// applied matrix-free by the solve that follows, as the step does with nsfem_step_opts.matrix_free != 1
static void monolithic_assemble(nsfem_ctx* ctx, uint32_t flags) {
  NSFEM_REQUIRE(!ctx->distributed(), "the explicit seam of the monolithic system takes single contexts only "
                                     "(this context has a communicator)");
  monolithic_setup(ctx);
  if (flags & 1u) momentum_begin_step(ctx, false);
  ctx->mono_rnorm = bdf_residual(ctx);
  ctx->mono_mf = (flags & 2u) != 0;
  ctx->mf_active = ctx->mono_mf;
  monolithic_linearise(ctx);
  ctx->mf_active = false;
}

static int monolithic_solve(nsfem_ctx* ctx, const nsfem_krylov_opts& o, nsfem_solve_info& inf) {
  ctx->mf_active = ctx->mono_mf;
  int rc;
  try {
    rc = monolithic_solve_update(ctx, ctx->mono_rnorm, false, o, inf);
  } catch (...) {
    ctx->mf_active = false;
    throw;
  }
  ctx->mf_active = false;
  return rc;
}

// Test hook: the two composite objects of the monolithic linear solve on host vectors of nvel + npre entries, prepared
// as the linear solve of nsfem_step_bdf prepares them (and nothing else; no state slot is written, and what = 0
// writes no right-hand side either -- the preconditioner uses rhs_p as scratch, as it does inside the step).  what = 0: y = MixedOp x, linearised about U0 with the convective form and Picard flag the context holds
// (nsfem_set_convective_form); what = 1: y = BlockPrec x.  matrix_free != 0: the velocity Jacobian is applied
// matrix-free, as in a step with nsfem_step_opts.matrix_free != 1.  Single contexts only.
extern "C" int nsfem_monolithic_apply(nsfem_ctx* ctx, int what, int matrix_free, const double* x, double* y) {
  API_BEGIN
  NSFEM_REQUIRE(ctx && x && y && (what == 0 || what == 1), "bad argument");
  NSFEM_REQUIRE(!ctx->distributed(), "nsfem_monolithic_apply takes single contexts only (this context has a "
                                     "communicator)");
  hipStream_t s = ctx->stream;
  monolithic_setup(ctx);
  momentum_begin_step(ctx, false);
  ctx->mf_active = matrix_free != 0;
  try {
    monolithic_linearise(ctx);
    const int64_t n = nvel(ctx) + npre(ctx);
    DevBuf<double> dx, dy;
    dx.upload(x, (size_t)n, s);
    dy.alloc((size_t)n);
    dy.zero(s);
    if (what == 0) ctx->mixed_op.apply(s, dx.p, dy.p);
    else ctx->block_prec.apply(s, dx.p, dy.p);
    NSFEM_HIP(hipMemcpyAsync(y, dy.p, sizeof(double) * n, hipMemcpyDeviceToHost, s));
    NSFEM_HIP(hipStreamSynchronize(s));
  } catch (...) {
    ctx->mf_active = false;
    throw;
  }
  ctx->mf_active = false;
  API_END(ctx)
}

// the explicit vector a step stored (slot `one`) becomes the next step's old one (slot `two`); without a fresh vector
// the old one is no longer that of the level before
static void rotate_stored_vector(nsfem_ctx* ctx, int one, int two, bool& fresh1, bool& valid2) {
  if (fresh1) std::swap(ctx->state[two].p, ctx->state[one].p);
  valid2 = fresh1;
  fresh1 = false;
}

extern "C" int nsfem_advance(nsfem_ctx* ctx, int scheme) {
  API_BEGIN
  NSFEM_REQUIRE(ctx, "null context");
  hipStream_t s = ctx->stream;
  // u2 <- u1 (pointer swap), u1 <- u0 (copy; u0 keeps its value as in the reference)
  std::swap(ctx->state[NSFEM_U2].p, ctx->state[NSFEM_U1].p);
  NSFEM_HIP(hipMemcpyAsync(ctx->state[NSFEM_U1].p, ctx->state[NSFEM_U0].p,
                           sizeof(double) * nvel(ctx), hipMemcpyDeviceToDevice, s));
  // (partitioned IMEX steps: the ghost entries travel with the rotation; those of u0 are copies to round-off only)
  ctx->u2_ghost_fresh = ctx->u1_ghost_fresh;
  ctx->u1_ghost_fresh = false;
  // (p_(n-1) is kept for the optional extrapolated start vector of the projection step)
  std::swap(ctx->state[NSFEM_P2_OLD].p, ctx->state[NSFEM_P_OLD].p);
  NSFEM_HIP(hipMemcpyAsync(ctx->state[NSFEM_P_OLD].p, ctx->state[NSFEM_P].p,
                           sizeof(double) * npre(ctx), hipMemcpyDeviceToDevice, s));
  if (scheme == 0 && ctx->pressure_history < 2) ctx->pressure_history++;
  // IMEX: c_c N(u1) of the step becomes c_c N(u2) of the next one
  rotate_stored_vector(ctx, NSFEM_CONV_N1, NSFEM_CONV_N2, ctx->conv_n1_fresh, ctx->conv_n2_valid);
  // Lagrangian averaging of law 8: I <- I', cs2_prev <- cs2_cur (pointer swaps).  Without a formed level n the old
  // cs2_prev is no longer that of level n-1; I stays (the memory along the path lines misses that step)
  if (lagrangian_on(ctx)) {
    nsfem_ctx::Dynamic::Lagrangian& L = ctx->dyn.lag;
    if (L.cur_valid) {
      std::swap(L.I.p, L.Inew.p);
      std::swap(L.cs2_prev.p, L.cs2_cur.p);
      L.have_state = true;
    }
    L.have_prev = L.cur_valid;
    L.cur_valid = false;
  }
  // scalar transport: T2 <- T1 (pointer swap), T1 <- T0 (copy), and the stored convection as above
  if (scheme == 0 && ctx->sc.configured) {
    nsfem_ctx::Scalar& sc = ctx->sc;
    for (int slot : {NSFEM_T0, NSFEM_T1, NSFEM_T2, NSFEM_TCONV_1, NSFEM_TCONV_2}) ensure_scalar_slot(ctx, slot);
    std::swap(ctx->state[NSFEM_T2].p, ctx->state[NSFEM_T1].p);
    NSFEM_HIP(hipMemcpyAsync(ctx->state[NSFEM_T1].p, ctx->state[NSFEM_T0].p, sizeof(double) * ctx->mesh.n_p2,
                             hipMemcpyDeviceToDevice, s));
    sc.conv2_weight = sc.conv1_weight;
    rotate_stored_vector(ctx, NSFEM_TCONV_1, NSFEM_TCONV_2, sc.conv1_fresh, sc.conv2_valid);
  }
  // (no synchronisation: everything that reads the state is ordered on the context's stream, nsfem_get_state and
  // nsfem_synchronize wait for it -- a host wait here left the GPU idle ~20 us in every time step)
  API_END(ctx)
}

// Post-processing Poisson solve on the P1 space:  (grad phi, grad psi) = rhs  with phi = 0 on the
// given dofs (velocity potential of source/ns_problem.py:105-176); Jacobi-CG, the singular pure
// Neumann case is handled by mean projection.  Not on the per-step path.
extern "C" int nsfem_poisson_solve(nsfem_ctx* ctx, const double* rhs, int64_t n_dirichlet,
                                   const int32_t* dofs, double* x, const nsfem_krylov_opts* opts,
                                   nsfem_solve_info* info) {
  nsfem_solve_info local;
  API_BEGIN
  NSFEM_REQUIRE(ctx && rhs && x && opts && (n_dirichlet == 0 || dofs), "null argument");
  NSFEM_REQUIRE(!ctx->distributed(), "post-processing solves are single-context");
  nsfem_solve_info& inf = info ? *info : local;
  hipStream_t s = ctx->stream;
  const int64_t n = npre(ctx);
  std::vector<uint8_t> hm((size_t)n, 0);
  std::vector<double> hb(rhs, rhs + n);
  for (int64_t i = 0; i < n_dirichlet; ++i) {
    NSFEM_REQUIRE(dofs[i] >= 0 && dofs[i] < n, "Dirichlet dof out of range");
    hm[dofs[i]] = 1;
    hb[dofs[i]] = 0.0;
  }
  DevBuf<uint8_t> mask;
  DevBuf<double> db, dx, dinv;
  mask.upload(hm, s);
  db.upload(hb, s);
  dx.alloc((size_t)n);
  dx.zero(s);
  dinv.alloc((size_t)n);
  LinOp op;
  op.A = &ctx->Ap;
  op.nv = 1;
  op.rowmask = mask.p;
  op.maskmode = MASK_ZERO;
  launch_inv_diag(s, ctx->Ap, 1, mask.p, dinv.p);
  op.dinv = dinv.p;
  op.n_global = n;
  int rc = pcg(s, ctx->kw, op, db.p, dx.p, *opts, inf, n_dirichlet == 0);
  if (rc != NSFEM_OK) throw Error(rc, "CG failed in the post-processing Poisson solve");
  NSFEM_HIP(hipMemcpyAsync(x, dx.p, sizeof(double) * n, hipMemcpyDeviceToHost, s));
  NSFEM_HIP(hipStreamSynchronize(s));
  API_END(ctx)
}

extern "C" int nsfem_mass_solve(nsfem_ctx* ctx, int field, const double* b, double* x,
                                const nsfem_krylov_opts* opts, nsfem_solve_info* info) {
  nsfem_solve_info local;
  API_BEGIN
  NSFEM_REQUIRE(ctx && b && x && opts, "null argument");
  NSFEM_REQUIRE(field == NSFEM_VELOCITY || field == NSFEM_PRESSURE, "bad field");
  nsfem_solve_info& inf = info ? *info : local;
  hipStream_t s = ctx->stream;
  const bool vel = field == NSFEM_VELOCITY;
  const int64_t n = vel ? nvel(ctx) : npre(ctx);
  DevBuf<double> db, dx, dinv;
  db.alloc((size_t)n);
  dx.alloc((size_t)n);
  dinv.alloc((size_t)n);
  NSFEM_HIP(hipMemcpyAsync(db.p, b, sizeof(double) * n, hipMemcpyHostToDevice, s));
  dx.zero(s);
  LinOp op;
  op.A = vel ? &ctx->M2 : &ctx->Mp;
  op.nv = vel ? ctx->mesh.dim : 1;
  launch_inv_diag(s, *op.A, op.nv, nullptr, dinv.p);
  op.dinv = dinv.p;
  int rc = pcg(s, ctx->kw, op, db.p, dx.p, *opts, inf, false);
  if (rc != NSFEM_OK) throw Error(rc, "CG failed in the mass (projection) solve");
  NSFEM_HIP(hipMemcpyAsync(x, dx.p, sizeof(double) * n, hipMemcpyDeviceToHost, s));
  NSFEM_HIP(hipStreamSynchronize(s));
  API_END(ctx)
}

extern "C" int nsfem_shift_mean_pressure(nsfem_ctx* ctx, double target, double* mean_before) {
  API_BEGIN
  NSFEM_REQUIRE(ctx, "null context");
  hipStream_t s = ctx->stream;
  const int64_t np = npre(ctx);
  // int p dx = 1^T M_p p ; partitioned meshes: owned rows only (ghost rows are the neighbours'),
  // all-reduced, divided by the GLOBAL measure of the domain
  ctx->kw.ensure(nvel(ctx));
  double* parts = ctx->kw.parts.p + 5 * kParts;
  const bool dist = ctx->distributed();
  double area = ctx->area;
  launch_axpby(s, np, 0.0, ctx->tmp_p.p, 0.0, nullptr, ctx->rhs_p.p);
  launch_add_scalar(s, np, 1.0, ctx->rhs_p.p);                     // rhs_p = 1
  if (dist) {
    if (!(ctx->area_global > 0.0)) {
      launch_spmv(s, ctx->Mp, 1, ctx->rhs_p.p, ctx->tmp_p.p, nullptr, MASK_NONE);
      if (ctx->ghost_p.p) launch_zero_ghost(s, np, ctx->mask_p.p, ctx->tmp_p.p);
      launch_dot(s, np, ctx->tmp_p.p, ctx->rhs_p.p, parts);
      ctx->comm->allreduce_sum(s, parts, kParts);
      ctx->area_global = host_sum_parts(s, ctx->kw, 5);
    }
    area = ctx->area_global;
    ctx->comm->exchange(s, ctx->halo_p1, ctx->state[NSFEM_P].p, 1);
  }
  launch_spmv(s, ctx->Mp, 1, ctx->state[NSFEM_P].p, ctx->tmp_p.p, nullptr, MASK_NONE);
  if (dist && ctx->ghost_p.p) launch_zero_ghost(s, np, ctx->mask_p.p, ctx->tmp_p.p);
  launch_dot(s, np, ctx->tmp_p.p, ctx->rhs_p.p, parts);
  if (dist) ctx->comm->allreduce_sum(s, parts, kParts);
  const double mean = host_sum_parts(s, ctx->kw, 5) / area;
  if (mean_before) *mean_before = mean;
  launch_add_scalar(s, np, -(mean - target), ctx->state[NSFEM_P].p);
  NSFEM_HIP(hipStreamSynchronize(s));
  API_END(ctx)
}

// mass shift 1/tau of the velocity-block / Schur-complement preconditioners (see ensure_L); only
// the preconditioner changes, never the discrete equations
extern "C" int nsfem_set_preconditioner_shift(nsfem_ctx* ctx, double shift) {
  API_BEGIN
  NSFEM_REQUIRE(ctx, "null context");
  NSFEM_REQUIRE(shift >= 0.0 && std::isfinite(shift), "the preconditioner shift must be >= 0");
  if (shift != ctx->prec_shift) { ctx->L_dirty = true; ctx->graph_epoch++; }
  ctx->prec_shift = shift;
  API_END(ctx)
}

// rotating frame (2D): angular velocity omega and its time derivative at the new time level
extern "C" int nsfem_set_angular_velocity(nsfem_ctx* ctx, double omega, double omega_dot) {
  API_BEGIN
  NSFEM_REQUIRE(ctx, "null context");
  NSFEM_REQUIRE(ctx->mesh.dim == 2, "scalar angular velocity: 2D meshes (use nsfem_set_angular_velocity_3d)");
  NSFEM_REQUIRE(std::isfinite(omega) && std::isfinite(omega_dot), "non-finite angular velocity");
  if (ctx->omega != omega || ctx->omega_dot != omega_dot) ctx->graph_epoch++;
  ctx->omega = omega;
  ctx->omega_dot = omega_dot;
  API_END(ctx)
}

// rotating frame (3D): angular velocity vector and its time derivative
extern "C" int nsfem_set_angular_velocity_3d(nsfem_ctx* ctx, const double omega[3], const double omega_dot[3]) {
  API_BEGIN
  NSFEM_REQUIRE(ctx && omega && omega_dot, "null argument");
  NSFEM_REQUIRE(ctx->mesh.dim == 3, "vector angular velocity: 3D meshes only");
  for (int a = 0; a < 3; ++a) {
    NSFEM_REQUIRE(std::isfinite(omega[a]) && std::isfinite(omega_dot[a]), "non-finite angular velocity");
    if (ctx->omega3[a] != omega[a] || ctx->omega_dot3[a] != omega_dot[a]) ctx->graph_epoch++;
    ctx->omega3[a] = omega[a];
    ctx->omega_dot3[a] = omega_dot[a];
  }
  API_END(ctx)
}

// max over cells of the DG2-projected local CFL number  2 |u| k / h  (reference
// source/ns_problem.py:554-587) of velocity slot `slot`; one kernel + a 256-value read-back
extern "C" int nsfem_cfl_number(nsfem_ctx* ctx, int slot, double step_size, double* cfl) {
  API_BEGIN
  NSFEM_REQUIRE(ctx && cfl, "null argument");
  require_slot(ctx, slot, SlotClass::VelocitySized);
  hipStream_t s = ctx->stream;
  const int n_parts = 256;
  ctx->kw.ensure(nvel(ctx));
  double* parts = ctx->kw.parts.p + 5 * kParts;
  if (ctx->mesh.dim == 3) launch_cfl_3d(s, ctx->mesh, ctx->state[slot].p, 2.0 * step_size, parts, n_parts);
  else launch_cfl(s, ctx->mesh, ctx->state[slot].p, 2.0 * step_size, parts, n_parts);
  if (ctx->distributed()) ctx->comm->allreduce_max(s, parts, n_parts);
  double h[256];
  NSFEM_HIP(hipMemcpyAsync(h, parts, sizeof(h), hipMemcpyDeviceToHost, s));
  NSFEM_HIP(hipStreamSynchronize(s));
  double m = 0.0;
  for (double v : h) m = std::max(m, v);
  *cfl = m;
  API_END(ctx)
}

// Surface force, mass flux and measure of a set of boundary facets (csrc/boundary.hip): one thread
// per facet, per-facet values summed here in facet order.
extern "C" int nsfem_boundary_force(nsfem_ctx* ctx, int velocity_slot, int pressure_slot,
                                    int32_t n_facets, const int32_t* facet_cell,
                                    const int32_t* facet_local, double nu, double sym, double* out) {
  API_BEGIN
  NSFEM_REQUIRE(ctx && out && (n_facets == 0 || (facet_cell && facet_local)), "null argument");
  require_slot(ctx, velocity_slot, SlotClass::VelocitySized);
  require_slot(ctx, pressure_slot, SlotClass::PressureSized);
  const int dim = ctx->mesh.dim, w = dim + 2;
  for (int k = 0; k < w; ++k) out[k] = 0.0;
  if (n_facets == 0) return NSFEM_OK;
  for (int32_t f = 0; f < n_facets; ++f) {
    NSFEM_REQUIRE(facet_cell[f] >= 0 && facet_cell[f] < ctx->mesh.n_cells, "facet cell out of range");
    NSFEM_REQUIRE(facet_local[f] >= 0 && facet_local[f] <= dim, "local facet index out of range");
  }
  hipStream_t s = ctx->stream;
  DevBuf<int32_t> dc, dl;
  DevBuf<double> dout;
  dc.upload(facet_cell, (size_t)n_facets, s);
  dl.upload(facet_local, (size_t)n_facets, s);
  dout.alloc((size_t)n_facets * w);
  launch_boundary_force(s, ctx->mesh, n_facets, dc.p, dl.p, ctx->state[velocity_slot].p,
                        ctx->state[pressure_slot].p, nu, sym, dout.p);
  std::vector<double> h((size_t)n_facets * w);
  NSFEM_HIP(hipMemcpyAsync(h.data(), dout.p, sizeof(double) * h.size(), hipMemcpyDeviceToHost, s));
  NSFEM_HIP(hipStreamSynchronize(s));
  for (int32_t f = 0; f < n_facets; ++f)
    for (int k = 0; k < w; ++k) out[k] += h[(size_t)f * w + k];
  API_END(ctx)
}

// Volume integrals of the discrete solution or of its difference to a reference field (csrc/functionals.hip): one
// thread per cell, one partial per workgroup and quantity, folded on the device in a fixed order.  Reads the two
// slots, writes no state.
extern "C" int nsfem_volume_functionals(nsfem_ctx* ctx, int velocity_slot, int pressure_slot,
                                        const double* ref_velocity, const double* ref_pressure,
                                        const uint8_t* cell_flags, double out[NSFEM_N_FUNCTIONALS]) {
  API_BEGIN
  NSFEM_REQUIRE(ctx && out, "null argument");
  require_slot(ctx, velocity_slot, SlotClass::VelocitySized);
  require_slot(ctx, pressure_slot, SlotClass::PressureSized);
  hipStream_t s = ctx->stream;
  const int dim = ctx->mesh.dim;
  const size_t nc = (size_t)ctx->mesh.n_cells;
  const PartialsWork w(ctx->vf_parts, NSFEM_N_FUNCTIONALS, kVolParts);
  const double *ur = nullptr, *pr = nullptr;
  if (ref_velocity) {
    ctx->vf_ref_u.upload(ref_velocity, (size_t)nvel(ctx), s);
    ur = ctx->vf_ref_u.p;
  }
  if (ref_pressure) {
    ctx->vf_ref_p.upload(ref_pressure, (size_t)npre(ctx), s);
    pr = ctx->vf_ref_p.p;
  }
  const uint8_t* flags = nullptr;
  if (cell_flags) {
    // the resident copy is replaced only when the CONTENTS differ (the same pointer may hold new flags)
    if (ctx->vf_flags.n != nc || ctx->vf_flags_host.size() != nc ||
        std::memcmp(ctx->vf_flags_host.data(), cell_flags, nc) != 0) {
      ctx->vf_flags_host.assign(cell_flags, cell_flags + nc);
      ctx->vf_flags.upload(ctx->vf_flags_host, s);
    }
    flags = ctx->vf_flags.p;
  }
  const double* u = ctx->state[velocity_slot].p;
  const double* p = ctx->state[pressure_slot].p;
  const bool dist = ctx->distributed();
  if (dist) {   // ghost nodes take their owners' values -- in copies, the slots keep their bytes
    if (ctx->vf_u.n != (size_t)nvel(ctx)) ctx->vf_u.alloc((size_t)nvel(ctx));
    if (ctx->vf_p.n != (size_t)npre(ctx)) ctx->vf_p.alloc((size_t)npre(ctx));
    NSFEM_HIP(hipMemcpyAsync(ctx->vf_u.p, u, sizeof(double) * nvel(ctx), hipMemcpyDeviceToDevice, s));
    NSFEM_HIP(hipMemcpyAsync(ctx->vf_p.p, p, sizeof(double) * npre(ctx), hipMemcpyDeviceToDevice, s));
    ctx->comm->exchange(s, ctx->halo_p2, ctx->vf_u.p, dim);
    ctx->comm->exchange(s, ctx->halo_p1, ctx->vf_p.p, 1);
    u = ctx->vf_u.p;
    p = ctx->vf_p.p;
  }
  launch_vol_functionals(s, ctx->mesh, u, p, ur, pr, flags, w.parts, w.res);
  if (dist) ctx->comm->allreduce_sum(s, w.res, NSFEM_N_FUNCTIONALS);
  w.read_back(s, out);
  API_END(ctx)
}

// ------------------------------------------------- point location, point evaluation, tracer particles (points.hip)
static void points_require_supported(nsfem_ctx* c, bool need_locator = true) {
  NSFEM_REQUIRE(!c->comm, "point evaluation / tracers: contexts with a communicator (partitioned meshes) are not "
                          "supported -- a point can lie in another rank's cells");
  if (need_locator) NSFEM_REQUIRE(c->pts.have_locator, "nsfem_set_point_locator has not been called");
}

// field kind of a state slot for point evaluation: 0 velocity, 1 pressure, 2 P2 scalar; anything else is refused
static int point_field_kind(nsfem_ctx* c, int slot) {
  switch (slot) {
    case NSFEM_U0: case NSFEM_U1: case NSFEM_U2: case NSFEM_USTAR: return 0;
    case NSFEM_P: case NSFEM_P_OLD: case NSFEM_P2_OLD: return 1;
    case NSFEM_T0: case NSFEM_T1: case NSFEM_T2:
      NSFEM_REQUIRE(c->sc.configured, "temperature slot without nsfem_set_scalar");
      ensure_scalar_slot(c, slot);
      return 2;
    default: throw Error(NSFEM_ERR_ARG, "not a state slot (velocity, pressure or transported scalar level)");
  }
}

template <class T>
static void grow(DevBuf<T>& b, size_t count) {
  if (b.n < count) b.alloc(count);
}

extern "C" int nsfem_set_point_locator(nsfem_ctx* ctx, const double* origin, const double* inv_h,
                                       const int32_t* nbins, const int32_t* bin_ptr, const int32_t* bin_cells) {
  API_BEGIN
  NSFEM_REQUIRE(ctx && origin && inv_h && nbins && bin_ptr, "null argument");
  points_require_supported(ctx, false);
  const int dim = ctx->mesh.dim;
  int64_t nb = 1;
  for (int d = 0; d < dim; ++d) {
    NSFEM_REQUIRE(std::isfinite(origin[d]) && std::isfinite(inv_h[d]) && inv_h[d] > 0.0, "point locator: bad grid");
    NSFEM_REQUIRE(nbins[d] >= 1, "point locator: nbins must be >= 1");
    nb *= nbins[d];
    NSFEM_REQUIRE(nb < ((int64_t)1 << 31) - 1, "point locator: too many bins");
  }
  // the kernels index the mesh with these lists: every entry is checked here, once
  NSFEM_REQUIRE(bin_ptr[0] == 0, "point locator: bin_ptr[0] != 0");
  for (int64_t b = 0; b < nb; ++b) NSFEM_REQUIRE(bin_ptr[b + 1] >= bin_ptr[b], "point locator: bin_ptr decreases");
  const int64_t len = bin_ptr[nb];
  NSFEM_REQUIRE(len == 0 || bin_cells, "null argument");
  for (int64_t k = 0; k < len; ++k)
    NSFEM_REQUIRE(bin_cells[k] >= 0 && bin_cells[k] < ctx->mesh.n_cells, "point locator: cell id out of range");
  nsfem_ctx::Points& P = ctx->pts;
  hipStream_t s = ctx->stream;
  P.have_locator = false;
  P.bin_ptr.upload(bin_ptr, (size_t)nb + 1, s);
  P.bin_cells.upload(bin_cells, (size_t)len, s);
  NSFEM_HIP(hipStreamSynchronize(s));
  P.loc = PointLocatorDev();
  for (int d = 0; d < dim; ++d) {
    P.loc.origin[d] = origin[d];
    P.loc.inv_h[d] = inv_h[d];
    P.loc.nbins[d] = nbins[d];
  }
  P.loc.bin_ptr = P.bin_ptr.p;
  P.loc.bin_cells = P.bin_cells.p;
  P.have_locator = true;
  API_END(ctx)
}

extern "C" int nsfem_locate_points(nsfem_ctx* ctx, int64_t n, const double* x, int32_t* cells) {
  API_BEGIN
  NSFEM_REQUIRE(ctx, "null context");
  points_require_supported(ctx);
  NSFEM_REQUIRE(n >= 0 && (n == 0 || (x && cells)), "n < 0 or null argument");
  if (n == 0) return NSFEM_OK;
  nsfem_ctx::Points& P = ctx->pts;
  hipStream_t s = ctx->stream;
  const size_t dim = (size_t)ctx->mesh.dim;
  grow(P.x, (size_t)n * dim);
  grow(P.cells, (size_t)n);
  NSFEM_HIP(hipMemcpyAsync(P.x.p, x, sizeof(double) * n * dim, hipMemcpyHostToDevice, s));
  launch_locate_points(s, ctx->mesh, P.loc, n, P.x.p, P.cells.p);
  NSFEM_HIP(hipMemcpyAsync(cells, P.cells.p, sizeof(int32_t) * n, hipMemcpyDeviceToHost, s));
  NSFEM_HIP(hipStreamSynchronize(s));
  API_END(ctx)
}

extern "C" int nsfem_eval_points(nsfem_ctx* ctx, int slot, int64_t n, const double* x, const int32_t* cells,
                                 double* out) {
  API_BEGIN
  NSFEM_REQUIRE(ctx, "null context");
  points_require_supported(ctx);
  const int kind = point_field_kind(ctx, slot);
  NSFEM_REQUIRE(n >= 0 && (n == 0 || (x && out)), "n < 0 or null argument");
  if (n == 0) return NSFEM_OK;
  nsfem_ctx::Points& P = ctx->pts;
  hipStream_t s = ctx->stream;
  const size_t dim = (size_t)ctx->mesh.dim, nv = kind == 0 ? dim : 1;
  grow(P.x, (size_t)n * dim);
  grow(P.cells, (size_t)n);
  grow(P.out, (size_t)n * dim);
  NSFEM_HIP(hipMemcpyAsync(P.x.p, x, sizeof(double) * n * dim, hipMemcpyHostToDevice, s));
  if (cells) NSFEM_HIP(hipMemcpyAsync(P.cells.p, cells, sizeof(int32_t) * n, hipMemcpyHostToDevice, s));
  else launch_locate_points(s, ctx->mesh, P.loc, n, P.x.p, P.cells.p);
  launch_eval_points(s, ctx->mesh, kind, ctx->state[slot].p, n, P.x.p, P.cells.p, P.out.p);
  NSFEM_HIP(hipMemcpyAsync(out, P.out.p, sizeof(double) * n * nv, hipMemcpyDeviceToHost, s));
  NSFEM_HIP(hipStreamSynchronize(s));
  API_END(ctx)
}

extern "C" int nsfem_tracers_set(nsfem_ctx* ctx, int64_t n, const double* x) {
  API_BEGIN
  NSFEM_REQUIRE(ctx, "null context");
  points_require_supported(ctx);
  NSFEM_REQUIRE(n >= 0 && (n == 0 || x), "n < 0 or null argument");
  nsfem_ctx::Points& P = ctx->pts;
  hipStream_t s = ctx->stream;
  const size_t dim = (size_t)ctx->mesh.dim, blocks = (size_t)((n + 255) / 256);
  grow(P.tx, (size_t)n * dim);
  grow(P.tcell, (size_t)n);
  grow(P.tstatus, (size_t)n);
  grow(P.tcounts, 2 * blocks);
  if (n > 0) NSFEM_HIP(hipMemcpyAsync(P.tx.p, x, sizeof(double) * n * dim, hipMemcpyHostToDevice, s));
  launch_locate_points(s, ctx->mesh, P.loc, n, P.tx.p, P.tcell.p);
  launch_tracer_init(s, n, P.tcell.p, P.tstatus.p, P.tcounts.p);
  NSFEM_HIP(hipStreamSynchronize(s));
  P.n_tracers = n;
  P.advect_calls = 0;
  API_END(ctx)
}

extern "C" int nsfem_tracers_advect(nsfem_ctx* ctx, int slot_begin, int slot_end, double dt, int n_sub) {
  API_BEGIN
  NSFEM_REQUIRE(ctx, "null context");
  points_require_supported(ctx);
  nsfem_ctx::Points& P = ctx->pts;
  NSFEM_REQUIRE(P.n_tracers >= 0, "nsfem_tracers_set has not been called");
  NSFEM_REQUIRE(point_field_kind(ctx, slot_begin) == 0 && point_field_kind(ctx, slot_end) == 0,
                "tracers move in a velocity slot");
  NSFEM_REQUIRE(n_sub >= 1, "n_sub < 1");
  NSFEM_REQUIRE(std::isfinite(dt), "dt is not finite");
  const double* ua = ctx->state[slot_begin].p;
  const double* ub = slot_end == slot_begin ? nullptr : ctx->state[slot_end].p;
  launch_advect_tracers(ctx->stream, ctx->mesh, P.loc, ua, ub, dt, n_sub, P.n_tracers, P.tx.p, P.tcell.p, P.tstatus.p,
                        P.tcounts.p);
  ++P.advect_calls;
  API_END(ctx)
}

extern "C" int nsfem_tracers_get(nsfem_ctx* ctx, double* x, int32_t* cells, uint8_t* status) {
  API_BEGIN
  NSFEM_REQUIRE(ctx, "null context");
  points_require_supported(ctx, false);
  nsfem_ctx::Points& P = ctx->pts;
  NSFEM_REQUIRE(P.n_tracers >= 0, "nsfem_tracers_set has not been called");
  hipStream_t s = ctx->stream;
  const size_t n = (size_t)P.n_tracers, dim = (size_t)ctx->mesh.dim;
  if (n && x) NSFEM_HIP(hipMemcpyAsync(x, P.tx.p, sizeof(double) * n * dim, hipMemcpyDeviceToHost, s));
  if (n && cells) NSFEM_HIP(hipMemcpyAsync(cells, P.tcell.p, sizeof(int32_t) * n, hipMemcpyDeviceToHost, s));
  if (n && status) NSFEM_HIP(hipMemcpyAsync(status, P.tstatus.p, n, hipMemcpyDeviceToHost, s));
  NSFEM_HIP(hipStreamSynchronize(s));
  API_END(ctx)
}

extern "C" int nsfem_tracers_info(nsfem_ctx* ctx, int64_t out[4]) {
  API_BEGIN
  NSFEM_REQUIRE(ctx && out, "null argument");
  nsfem_ctx::Points& P = ctx->pts;
  out[0] = out[1] = out[2] = out[3] = 0;
  if (P.n_tracers < 0) return NSFEM_OK;
  const size_t blocks = (size_t)((P.n_tracers + 255) / 256);
  std::vector<int32_t> h(2 * blocks);
  if (blocks) {
    NSFEM_HIP(hipMemcpyAsync(h.data(), P.tcounts.p, sizeof(int32_t) * h.size(), hipMemcpyDeviceToHost, ctx->stream));
    NSFEM_HIP(hipStreamSynchronize(ctx->stream));
  }
  out[0] = P.n_tracers;
  for (size_t b = 0; b < blocks; ++b) {
    out[1] += h[2 * b];
    out[3] += h[2 * b + 1];
  }
  out[2] = P.advect_calls;
  API_END(ctx)
}

// ------------------------------------------------------------------ running flow statistics (statistics.hip)
// every check of a call comes before its first launch: a refused call leaves the accumulators as they were
static void stats_require_supported(nsfem_ctx* c) {
  NSFEM_REQUIRE(!c->distributed(), "flow statistics: partitioned contexts are not supported -- the profiles need a "
                                   "merge of the group sums across ranks");
}

static void stats_require_enabled(nsfem_ctx* c) {
  stats_require_supported(c);
  NSFEM_REQUIRE(c->stats.flags != 0, "flow statistics: nsfem_stats_enable has not been called");
}

extern "C" int nsfem_stats_enable(nsfem_ctx* ctx, uint32_t flags) {
  API_BEGIN
  NSFEM_REQUIRE(ctx, "null context");
  stats_require_supported(ctx);
  nsfem_ctx::Stats& S = ctx->stats;
  if (flags == 0) {
    S.acc2.release();
    S.acc1.release();
    S.out.release();
    for (nsfem_ctx::Stats::Groups& g : S.groups) {
      g.n = -1;
      g.ptr.release();
      g.nodes.release();
      g.weights.release();
    }
    S.flags = 0;
    S.W = 0.0;
    S.samples = S.launches = 0;
    return NSFEM_OK;
  }
  NSFEM_REQUIRE((flags & ~7u) == 0, "flow statistics: unknown flag");
  NSFEM_REQUIRE(flags & NSFEM_STATS_VELOCITY, "flow statistics: NSFEM_STATS_VELOCITY is mandatory");
  const bool scalar = (flags & NSFEM_STATS_SCALAR) != 0;
  NSFEM_REQUIRE(!scalar || ctx->sc.configured, "flow statistics: scalar requested, but nsfem_set_scalar has not been "
                                               "called");
  hipStream_t s = ctx->stream;
  const size_t stride2 = ((size_t)ctx->mesh.n_p2 + 1) & ~(size_t)1, stride1 = ((size_t)ctx->mesh.n_p1 + 1) & ~(size_t)1;
  const size_t len2 = (size_t)stats_columns(ctx->mesh.dim, scalar) * stride2;
  const size_t len1 = flags & NSFEM_STATS_PRESSURE ? 2 * stride1 : 0;
  if (S.acc2.n != len2) S.acc2.alloc(len2);
  if (S.acc1.n != len1) S.acc1.alloc(len1);
  S.acc2.zero(s);
  S.acc1.zero(s);
  NSFEM_HIP(hipStreamSynchronize(s));
  S.stride2 = stride2;
  S.stride1 = stride1;
  S.flags = flags;
  S.W = 0.0;
  S.samples = S.launches = 0;
  API_END(ctx)
}

extern "C" int nsfem_stats_sample(nsfem_ctx* ctx, int velocity_slot, int pressure_slot, int scalar_slot,
                                  double weight) {
  API_BEGIN
  NSFEM_REQUIRE(ctx, "null context");
  stats_require_enabled(ctx);
  nsfem_ctx::Stats& S = ctx->stats;
  NSFEM_REQUIRE(std::isfinite(weight) && weight > 0.0, "flow statistics: the weight of a sample must be finite and > 0");
  require_slot(ctx, velocity_slot, SlotClass::VelocitySized, "flow statistics: ");
  const bool pressure = (S.flags & NSFEM_STATS_PRESSURE) != 0, scalar = (S.flags & NSFEM_STATS_SCALAR) != 0;
  if (pressure) require_slot(ctx, pressure_slot, SlotClass::PressureSized, "flow statistics: ");
  else NSFEM_REQUIRE(pressure_slot == -1, "flow statistics: pressure slot given, but NSFEM_STATS_PRESSURE is not enabled");
  if (scalar) {
    NSFEM_REQUIRE(ctx->sc.configured, "flow statistics: scalar requested, but nsfem_set_scalar has not been called");
    require_slot(ctx, scalar_slot, SlotClass::ScalarSized, "flow statistics: ");
    ensure_scalar_slot(ctx, scalar_slot);
  } else {
    NSFEM_REQUIRE(scalar_slot == -1, "flow statistics: scalar slot given, but NSFEM_STATS_SCALAR is not enabled");
  }
  StatsUpdate a;
  a.n2 = ctx->mesh.n_p2;
  a.stride2 = S.stride2;
  a.u = ctx->state[velocity_slot].p;
  a.T = scalar ? ctx->state[scalar_slot].p : nullptr;
  a.acc2 = S.acc2.p;
  if (pressure) {
    a.n1 = ctx->mesh.n_p1;
    a.stride1 = S.stride1;
    a.p = ctx->state[pressure_slot].p;
    a.acc1 = S.acc1.p;
  }
  const double W1 = S.W + weight;
  a.a = weight / W1;
  a.b = weight * S.W / W1;
  a.first = S.W == 0.0;
  launch_stats_update(ctx->stream, ctx->mesh.dim, scalar, a);
  S.W = W1;
  ++S.samples;
  ++S.launches;
  API_END(ctx)
}

extern "C" int nsfem_stats_get(nsfem_ctx* ctx, int quantity, double* host, int64_t n) {
  API_BEGIN
  NSFEM_REQUIRE(ctx && host, "null argument");
  stats_require_enabled(ctx);
  nsfem_ctx::Stats& S = ctx->stats;
  NSFEM_REQUIRE(S.samples > 0, "flow statistics: no sample has been taken");
  const int dim = ctx->mesh.dim, ncov = dim * (dim + 1) / 2;
  const bool p1 = quantity == NSFEM_STATS_MEAN_P || quantity == NSFEM_STATS_VAR_P;
  int col = 0, nc = 1;                      // first column, columns (0: trace of C_uu)
  bool moment = true;                       // divided by W
  const int tr[3] = {dim, dim == 2 ? dim + 2 : dim + 3, dim + 5};
  switch (quantity) {
    case NSFEM_STATS_MEAN_U: col = 0; nc = dim; moment = false; break;
    case NSFEM_STATS_COV_U: col = dim; nc = ncov; break;
    case NSFEM_STATS_TKE: nc = 0; break;
    case NSFEM_STATS_MEAN_P: col = 0; moment = false; break;
    case NSFEM_STATS_VAR_P: col = 1; break;
    case NSFEM_STATS_MEAN_T: col = dim + ncov; moment = false; break;
    case NSFEM_STATS_VAR_T: col = dim + ncov + 1; break;
    case NSFEM_STATS_FLUX_UT: col = dim + ncov + 2; nc = dim; break;
    default: throw Error(NSFEM_ERR_ARG, "flow statistics: unknown quantity");
  }
  if (p1) NSFEM_REQUIRE(S.flags & NSFEM_STATS_PRESSURE, "flow statistics: NSFEM_STATS_PRESSURE is not enabled");
  if (quantity >= NSFEM_STATS_MEAN_T) NSFEM_REQUIRE(S.flags & NSFEM_STATS_SCALAR, "flow statistics: NSFEM_STATS_SCALAR is not enabled");
  const int64_t nodes = p1 ? ctx->mesh.n_p1 : ctx->mesh.n_p2, len = nodes * (nc ? nc : 1);
  NSFEM_REQUIRE(n == len, "flow statistics: wrong size of the output");
  hipStream_t s = ctx->stream;
  grow(S.out, (size_t)len);
  const double scale = moment ? (nc ? 1.0 : 0.5) / S.W : 1.0;
  launch_stats_gather(s, nodes, p1 ? S.acc1.p : S.acc2.p, p1 ? S.stride1 : S.stride2, col, nc, scale, dim, tr, S.out.p);
  NSFEM_HIP(hipMemcpyAsync(host, S.out.p, sizeof(double) * len, hipMemcpyDeviceToHost, s));
  NSFEM_HIP(hipStreamSynchronize(s));
  API_END(ctx)
}

extern "C" int nsfem_stats_set_groups(nsfem_ctx* ctx, int field, int32_t n_groups, const int32_t* group_ptr,
                                      const int32_t* nodes, const double* weights) {
  API_BEGIN
  NSFEM_REQUIRE(ctx && group_ptr && nodes && weights, "null argument");
  stats_require_enabled(ctx);
  NSFEM_REQUIRE(field == 0 || field == 1, "flow statistics: field must be 0 (P2 nodes) or 1 (P1 nodes)");
  NSFEM_REQUIRE(n_groups >= 1, "flow statistics: n_groups < 1");
  // the profile kernel indexes the accumulators with these lists: every entry is checked here, before the upload
  const int32_t n_nodes = field == 0 ? ctx->mesh.n_p2 : ctx->mesh.n_p1;
  NSFEM_REQUIRE(group_ptr[0] == 0, "flow statistics: group_ptr[0] != 0");
  for (int32_t g = 0; g < n_groups; ++g)
    NSFEM_REQUIRE(group_ptr[g + 1] > group_ptr[g], "flow statistics: group_ptr must increase (no empty group)");
  const int32_t len = group_ptr[n_groups];
  for (int32_t k = 0; k < len; ++k) {
    NSFEM_REQUIRE(nodes[k] >= 0 && nodes[k] < n_nodes, "flow statistics: group node index out of range");
    NSFEM_REQUIRE(std::isfinite(weights[k]) && weights[k] > 0.0, "flow statistics: group weights must be finite and > 0");
  }
  nsfem_ctx::Stats::Groups& G = ctx->stats.groups[field];
  hipStream_t s = ctx->stream;
  G.n = -1;
  G.ptr.upload(group_ptr, (size_t)n_groups + 1, s);
  G.nodes.upload(nodes, (size_t)len, s);
  G.weights.upload(weights, (size_t)len, s);
  NSFEM_HIP(hipStreamSynchronize(s));
  G.n = n_groups;
  API_END(ctx)
}

extern "C" int nsfem_stats_profiles(nsfem_ctx* ctx, int field, double* out, int64_t n) {
  API_BEGIN
  NSFEM_REQUIRE(ctx && out, "null argument");
  stats_require_enabled(ctx);
  nsfem_ctx::Stats& S = ctx->stats;
  NSFEM_REQUIRE(field == 0 || field == 1, "flow statistics: field must be 0 (P2 nodes) or 1 (P1 nodes)");
  NSFEM_REQUIRE(field == 0 || (S.flags & NSFEM_STATS_PRESSURE), "flow statistics: NSFEM_STATS_PRESSURE is not enabled");
  NSFEM_REQUIRE(S.samples > 0, "flow statistics: no sample has been taken");
  const nsfem_ctx::Stats::Groups& G = S.groups[field];
  NSFEM_REQUIRE(G.n >= 1, "flow statistics: nsfem_stats_set_groups has not been called for this field");
  const bool scalar = field == 0 && (S.flags & NSFEM_STATS_SCALAR);
  const int dim = field == 0 ? ctx->mesh.dim : 1;
  const int64_t len = (int64_t)G.n * stats_columns(dim, scalar);
  NSFEM_REQUIRE(n == len, "flow statistics: wrong size of the output");
  hipStream_t s = ctx->stream;
  grow(S.out, (size_t)len);
  launch_stats_profile(s, dim, scalar, field == 0 ? S.acc2.p : S.acc1.p, field == 0 ? S.stride2 : S.stride1, 1.0 / S.W,
                       G.n, G.ptr.p, G.nodes.p, G.weights.p, S.out.p);
  NSFEM_HIP(hipMemcpyAsync(out, S.out.p, sizeof(double) * len, hipMemcpyDeviceToHost, s));
  NSFEM_HIP(hipStreamSynchronize(s));
  API_END(ctx)
}

extern "C" int nsfem_stats_info(nsfem_ctx* ctx, int64_t out[4]) {
  API_BEGIN
  NSFEM_REQUIRE(ctx && out, "null argument");
  const nsfem_ctx::Stats& S = ctx->stats;
  out[0] = S.samples;
  out[1] = S.flags;
  out[2] = (int64_t)(sizeof(double) * (S.acc2.n + S.acc1.n));
  out[3] = S.launches;
  API_END(ctx)
}

extern "C" int nsfem_stats_weight(nsfem_ctx* ctx, double* W) {
  API_BEGIN
  NSFEM_REQUIRE(ctx && W, "null argument");
  *W = ctx->stats.W;
  API_END(ctx)
}

// ------------------------------------------------------------------ gradient-derived fields (derived.hip)
static void derived_require_supported(nsfem_ctx* c) {
  NSFEM_REQUIRE(!c->comm, "derived fields: contexts with a communicator (partitioned meshes) are not supported -- the "
                          "recovery at a node on a partition boundary needs the cells of other ranks");
}

extern "C" int nsfem_derived_components(nsfem_ctx* ctx, int quantity, int* ncomp) {
  API_BEGIN
  NSFEM_REQUIRE(ctx && ncomp, "null argument");
  const int n = derived_components(ctx->mesh.dim, quantity);
  NSFEM_REQUIRE(n > 0, "derived fields: unknown quantity");
  *ncomp = n;
  API_END(ctx)
}

// every check comes before the first launch; reads the slots, writes the context's own work buffer only
extern "C" int nsfem_derived_fields(nsfem_ctx* ctx, int velocity_slot, int pressure_slot, int scalar_slot,
                                    unsigned quantity_mask, int center, double* out_host, int64_t out_len) {
  API_BEGIN
  NSFEM_REQUIRE(ctx && out_host, "null argument");
  derived_require_supported(ctx);
  NSFEM_REQUIRE(quantity_mask != 0, "derived fields: empty quantity mask");
  NSFEM_REQUIRE((quantity_mask >> NSFEM_N_DERIVED) == 0, "derived fields: unknown quantity bit");
  NSFEM_REQUIRE(center == NSFEM_DERIVED_CELL || center == NSFEM_DERIVED_VERTEX || center == NSFEM_DERIVED_NODE,
                "derived fields: unknown centre");
  require_slot(ctx, velocity_slot, SlotClass::VelocityLevel, "derived fields: ");
  const bool want_p = (quantity_mask & (1u << NSFEM_DERIVED_PRESSURE_GRADIENT)) != 0;
  const bool want_T = (quantity_mask & (1u << NSFEM_DERIVED_SCALAR_GRADIENT)) != 0;
  if (want_p || pressure_slot != -1) require_slot(ctx, pressure_slot, SlotClass::PressureSlot, "derived fields: ");
  if (want_T) NSFEM_REQUIRE(ctx->sc.configured, "derived fields: SCALAR_GRADIENT without nsfem_set_scalar");
  if (want_T || scalar_slot != -1) require_slot(ctx, scalar_slot, SlotClass::ScalarLevel, "derived fields: ");
  const MeshDev& m = ctx->mesh;
  int ncomp = 0;
  for (int q = 0; q < NSFEM_N_DERIVED; ++q)
    if (quantity_mask & (1u << q)) ncomp += derived_components(m.dim, q);
  const int64_t entities = center == NSFEM_DERIVED_CELL ? (int64_t)m.n_cells
                           : center == NSFEM_DERIVED_VERTEX ? (int64_t)m.n_cells * (m.dim + 1) : (int64_t)m.n_p2;
  NSFEM_REQUIRE(out_len == entities * ncomp, "derived fields: wrong size of the output");
  if (want_T) ensure_scalar_slot(ctx, scalar_slot);
  nsfem_ctx::Derived& D = ctx->derived;
  hipStream_t s = ctx->stream;
  grow(D.work, (size_t)derived_work_doubles(m, center, ncomp));
  const double* res = launch_derived_fields(s, m, ctx->state[velocity_slot].p, want_p ? ctx->state[pressure_slot].p : nullptr,
                                            want_T ? ctx->state[scalar_slot].p : nullptr, quantity_mask, center, ncomp,
                                            D.work.p);
  ++D.cell_launches;
  if (center == NSFEM_DERIVED_NODE) ++D.gather_launches;
  ++D.calls;
  NSFEM_HIP(hipMemcpyAsync(out_host, res, sizeof(double) * (size_t)out_len, hipMemcpyDeviceToHost, s));
  NSFEM_HIP(hipStreamSynchronize(s));
  API_END(ctx)
}

extern "C" int nsfem_derived_info(nsfem_ctx* ctx, int64_t out[4]) {
  API_BEGIN
  NSFEM_REQUIRE(ctx && out, "null argument");
  out[0] = ctx->derived.cell_launches;
  out[1] = ctx->derived.gather_launches;
  out[2] = ctx->derived.calls;
  out[3] = (int64_t)(ctx->derived.work.n * sizeof(double));
  API_END(ctx)
}

// ------------------------------------------------------------------ energy spectra (spectrum.hip, fd_transform_axes)
static void spectrum_require_supported(nsfem_ctx* c) {
  NSFEM_REQUIRE(!c->comm, "energy spectrum: contexts with a communicator (partitioned meshes) are not supported -- "
                          "the lattice of a rank is a strip or slab of the box");
}

// components and nodes of a nodal slot (0 components: no nodal slot)
static int spectrum_slot_kind(const nsfem_ctx* c, int slot, int64_t* nodes) {
  switch (slot) {
    case NSFEM_U0: case NSFEM_U1: case NSFEM_U2: case NSFEM_USTAR: case NSFEM_BODY_FORCE:
      *nodes = c->mesh.n_p2;
      return c->mesh.dim;
    case NSFEM_T0: case NSFEM_T1: case NSFEM_T2: case NSFEM_T_SOURCE:
      *nodes = c->mesh.n_p2;
      return 1;
    case NSFEM_P: case NSFEM_P_OLD: case NSFEM_P2_OLD:
      *nodes = c->mesh.n_p1;
      return 1;
    default:      // assembled vectors (traction, stored convection terms) are no nodal values
      return 0;
  }
}

// everything is validated on the host before the first upload: no kernel of the plan can index out of range
extern "C" int nsfem_spectrum_set(nsfem_ctx* ctx, const int32_t n[3], const double* Fx, const double* Fy,
                                  const double* Fz, const int32_t* node_of_point, int32_t n_bins,
                                  const int32_t* bin_ptr, const int32_t* bin_points) {
  API_BEGIN
  NSFEM_REQUIRE(ctx && n, "null argument");
  spectrum_require_supported(ctx);
  nsfem_ctx::Spectrum& S = ctx->spectrum;
  if (n[0] == 0) {      // frees the plan; the counters stay
    NSFEM_HIP(hipStreamSynchronize(ctx->stream));
    S.release();
    return NSFEM_OK;
  }
  NSFEM_REQUIRE(n[0] >= 1 && n[1] >= 1 && n[2] >= 1, "energy spectrum: non-positive lattice size");
  NSFEM_REQUIRE(node_of_point && bin_ptr, "null argument");
  NSFEM_REQUIRE(n_bins >= 1, "energy spectrum: n_bins < 1");
  const int64_t np = (int64_t)n[0] * n[1] * n[2];
  NSFEM_REQUIRE(np < INT32_MAX && n[2] <= 65535 && ((int64_t)n[2] * n[1] + 31) / 32 <= 65535,
                "energy spectrum: lattice too large");
  // a P1 field has fewer nodes than a P2 field: the largest index decides at nsfem_spectrum_compute which slots the
  // plan fits; none that no field has passes here
  int32_t max_node = -1;
  for (int64_t i = 0; i < np; ++i) {
    NSFEM_REQUIRE(node_of_point[i] >= 0 && node_of_point[i] < ctx->mesh.n_p2,
                  "energy spectrum: node_of_point out of range");
    max_node = std::max(max_node, node_of_point[i]);
  }
  NSFEM_REQUIRE(bin_ptr[0] == 0, "energy spectrum: bin_ptr[0] != 0");
  for (int32_t b = 0; b < n_bins; ++b)
    NSFEM_REQUIRE(bin_ptr[b + 1] >= bin_ptr[b], "energy spectrum: bin_ptr must not decrease");
  const int32_t len = bin_ptr[n_bins];
  NSFEM_REQUIRE(len == 0 || bin_points, "null argument");
  for (int32_t k = 0; k < len; ++k)
    NSFEM_REQUIRE(bin_points[k] >= 0 && bin_points[k] < np, "energy spectrum: bin point out of range");
  const double* F[3] = {Fx, Fy, Fz};
  for (int a = 0; a < 3; ++a)
    if (F[a])
      for (int64_t i = 0; i < (int64_t)n[a] * n[a]; ++i)
        NSFEM_REQUIRE(std::isfinite(F[a][i]), "energy spectrum: transform matrix is not finite");
  // chunks of at most kSpecChunk entries that never straddle a bin
  std::vector<int32_t> chunk_ptr{0}, bin_chunk_ptr((size_t)n_bins + 1, 0);
  for (int32_t b = 0; b < n_bins; ++b) {
    for (int32_t k = bin_ptr[b]; k < bin_ptr[b + 1]; k += kSpecChunk)
      chunk_ptr.push_back(std::min(k + kSpecChunk, bin_ptr[b + 1]));
    bin_chunk_ptr[b + 1] = (int32_t)chunk_ptr.size() - 1;
  }
  hipStream_t s = ctx->stream;
  NSFEM_HIP(hipStreamSynchronize(s));
  S.release();
  for (int a = 0; a < 3; ++a)
    if (F[a]) S.F[a].upload(F[a], (size_t)n[a] * n[a], s);
  S.node_of_point.upload(node_of_point, (size_t)np, s);
  S.bin_points.upload(bin_points, (size_t)len, s);
  S.chunk_ptr.upload(chunk_ptr.data(), chunk_ptr.size(), s);
  S.bin_chunk_ptr.upload(bin_chunk_ptr.data(), bin_chunk_ptr.size(), s);
  S.w0.alloc((size_t)np);
  S.w1.alloc((size_t)np);
  S.parts.alloc(std::max<size_t>(chunk_ptr.size() - 1, 1));
  S.out.alloc((size_t)n_bins * 3);
  NSFEM_HIP(hipStreamSynchronize(s));      // (the chunk lists are host vectors of this call)
  for (int a = 0; a < 3; ++a) S.n[a] = n[a];
  S.n_bins = n_bins;
  S.n_chunks = (int32_t)chunk_ptr.size() - 1;
  S.max_node = max_node;
  S.have_plan = true;
  API_END(ctx)
}

// per component: pack, the axis passes, the two bin launches; one copy of the result.  Reads the slot, writes the
// plan's own arrays only
extern "C" int nsfem_spectrum_compute(nsfem_ctx* ctx, int slot, double* out, int64_t out_len) {
  API_BEGIN
  NSFEM_REQUIRE(ctx && out, "null argument");
  spectrum_require_supported(ctx);
  nsfem_ctx::Spectrum& S = ctx->spectrum;
  NSFEM_REQUIRE(S.have_plan, "energy spectrum: nsfem_spectrum_set has not been called");
  int64_t nodes = 0;
  const int ncomp = spectrum_slot_kind(ctx, slot, &nodes);
  NSFEM_REQUIRE(ncomp > 0, "energy spectrum: the slot holds no nodal field");
  NSFEM_REQUIRE(ctx->state[slot].p && (int64_t)ctx->state[slot].n == nodes * ncomp,
                "energy spectrum: the slot has no storage yet (a scalar slot that was never set or stepped)");
  NSFEM_REQUIRE((int64_t)S.max_node < nodes, "energy spectrum: the plan names nodes the field of this slot does not have");
  NSFEM_REQUIRE(out_len == (int64_t)S.n_bins * ncomp, "energy spectrum: wrong size of the output");
  hipStream_t s = ctx->stream;
  const int64_t np = (int64_t)S.n[0] * S.n[1] * S.n[2];
  for (int c = 0; c < ncomp; ++c) {
    launch_spec_pack(s, np, S.node_of_point.p, ctx->state[slot].p, ncomp, c, S.w0.p);
    const double* w = fd_transform_axes(s, S.n[0], S.n[1], S.n[2], S.F[0].p, S.F[1].p, S.F[2].p, S.w0.p, S.w1.p,
                                        &S.transform_launches);
    launch_spec_bin(s, w, S.n_chunks, S.chunk_ptr.p, S.bin_points.p, S.parts.p, S.n_bins, S.bin_chunk_ptr.p, ncomp, c,
                    S.out.p);
    S.bin_launches += S.n_chunks > 0 ? 2 : 1;
  }
  ++S.calls;
  NSFEM_HIP(hipMemcpyAsync(out, S.out.p, sizeof(double) * (size_t)out_len, hipMemcpyDeviceToHost, s));
  NSFEM_HIP(hipStreamSynchronize(s));
  API_END(ctx)
}

extern "C" int nsfem_spectrum_info(nsfem_ctx* ctx, int64_t out[4]) {
  API_BEGIN
  NSFEM_REQUIRE(ctx && out, "null argument");
  NSFEM_REQUIRE(ctx->spectrum.have_plan, "energy spectrum: nsfem_spectrum_set has not been called");
  out[0] = ctx->spectrum.transform_launches;
  out[1] = ctx->spectrum.bin_launches;
  out[2] = ctx->spectrum.calls;
  out[3] = ctx->spectrum.bytes();
  API_END(ctx)
}

// ------------------------------------------------------------------ wall quantities (wall.hip)
static void wall_require_supported(nsfem_ctx* c) {
  NSFEM_REQUIRE(!c->comm, "wall quantities: contexts with a communicator (partitioned meshes) are not supported -- "
                          "use nsfem_boundary_force there");
}

// validates everything on the host first, then replaces the resident set: lists sorted by group (stable), group
// offsets, and the buffers nsfem_wall_compute writes -- the only allocations of the wall calls; the permutation back to
// the caller's order stays on the host, where the rows are un-permuted
extern "C" int nsfem_wall_set_facets(nsfem_ctx* ctx, int32_t n_facets, const int32_t* facet_cell,
                                     const int32_t* facet_local, const int32_t* facet_group, int32_t n_groups) {
  API_BEGIN
  NSFEM_REQUIRE(ctx, "null argument");
  wall_require_supported(ctx);
  NSFEM_REQUIRE(n_facets >= 0, "wall quantities: n_facets < 0");
  NSFEM_REQUIRE(n_groups >= 1, "wall quantities: n_groups < 1");
  NSFEM_REQUIRE(n_facets == 0 || (facet_cell && facet_local), "null argument");
  const int dim = ctx->mesh.dim, nw = wall_components(dim);
  for (int32_t f = 0; f < n_facets; ++f) {
    NSFEM_REQUIRE(facet_cell[f] >= 0 && facet_cell[f] < ctx->mesh.n_cells, "wall quantities: facet cell out of range");
    NSFEM_REQUIRE(facet_local[f] >= 0 && facet_local[f] <= dim, "wall quantities: local facet index out of range");
    if (facet_group)
      NSFEM_REQUIRE(facet_group[f] >= 0 && facet_group[f] < n_groups, "wall quantities: facet group out of range");
  }
  // counting sort by group: stable, goff[g] .. goff[g + 1] = the resident facets of group g
  std::vector<int32_t> goff((size_t)n_groups + 1, 0), perm((size_t)n_facets), cell((size_t)n_facets),
      local((size_t)n_facets);
  for (int32_t f = 0; f < n_facets; ++f) ++goff[(size_t)(facet_group ? facet_group[f] : 0) + 1];
  for (int32_t g = 0; g < n_groups; ++g) goff[(size_t)g + 1] += goff[g];
  {
    std::vector<int32_t> next(goff.begin(), goff.end() - 1);
    for (int32_t f = 0; f < n_facets; ++f) perm[(size_t)next[facet_group ? facet_group[f] : 0]++] = f;
  }
  for (int32_t k = 0; k < n_facets; ++k) {
    cell[k] = facet_cell[perm[k]];
    local[k] = facet_local[perm[k]];
  }
  nsfem_ctx::Wall& W = ctx->wall;
  hipStream_t s = ctx->stream;
  W.have_set = false;
  W.fcell.upload(cell.data(), cell.size(), s);
  W.flocal.upload(local.data(), local.size(), s);
  W.goff.upload(goff.data(), goff.size(), s);
  NSFEM_HIP(hipStreamSynchronize(s));   // the host vectors die with the call
  if (W.rows.n != (size_t)n_facets * nw) W.rows.alloc((size_t)n_facets * nw);
  if (W.sums.n != (size_t)n_groups * nw) W.sums.alloc((size_t)n_groups * nw);
  W.h_perm.swap(perm);
  W.h_rows.assign((size_t)n_facets * nw, 0.0);
  W.n_facets = n_facets;
  W.n_groups = n_groups;
  W.have_set = true;
  ++W.uploads;
  API_END(ctx)
}

// every check comes before the first launch; reads the slots, writes the context's wall buffers only
extern "C" int nsfem_wall_compute(nsfem_ctx* ctx, int velocity_slot, int pressure_slot, int scalar_slot,
                                  const nsfem_wall_opts* opts, double* out_groups, double* out_facets) {
  API_BEGIN
  NSFEM_REQUIRE(ctx, "null argument");
  wall_require_supported(ctx);
  NSFEM_REQUIRE(opts && out_groups, "wall quantities: null opts or out_groups");
  nsfem_ctx::Wall& W = ctx->wall;
  NSFEM_REQUIRE(W.have_set, "wall quantities: no facet set (nsfem_wall_set_facets)");
  require_slot(ctx, velocity_slot, SlotClass::VelocityLevel, "wall quantities: ");
  require_slot(ctx, pressure_slot, SlotClass::PressureSlot, "wall quantities: ");
  if (scalar_slot != -1) {
    require_slot(ctx, scalar_slot, SlotClass::ScalarLevel, "wall quantities: ");
    NSFEM_REQUIRE(ctx->sc.configured, "wall quantities: a scalar slot without nsfem_set_scalar");
    // (a level that was never set or stepped has no storage: allocating it here would write state)
    NSFEM_REQUIRE(ctx->state[scalar_slot].p, "wall quantities: the scalar slot holds no data yet");
  }
  NSFEM_REQUIRE(std::isfinite(opts->nu) && std::isfinite(opts->sym) && std::isfinite(opts->kappa) &&
                    std::isfinite(opts->origin[0]) && std::isfinite(opts->origin[1]) && std::isfinite(opts->origin[2]),
                "wall quantities: non-finite nu, sym, kappa or origin");
  const MeshDev& m = ctx->mesh;
  const int nw = wall_components(m.dim);
  WallParams wp;
  wp.nu = opts->nu;
  wp.sym = opts->sym;
  wp.kappa = opts->kappa;
  for (int d = 0; d < 3; ++d) wp.origin[d] = opts->origin[d];
  wp.law = opts->use_law != 0 ? ctx->visc.law : 0;
  for (int k = 0; k < 3; ++k) wp.law_p[k] = ctx->visc.p[k];
  // subgrid heat flux: the conductive row carries kappa + nu_x / Pr_t where the traction carries nu_x (the subgrid
  // laws 1, 4 and 5 only)
  const bool subgrid = is_subgrid_law(wp.law);
  wp.inv_prt = subgrid && scalar_slot != -1 && ctx->sc.prandtl_t > 0.0 ? 1.0 / ctx->sc.prandtl_t : 0.0;
  hipStream_t s = ctx->stream;
  // (law 8: nu_x of a facet's cell takes the constant of the velocity level the rows are formed on)
  if (wp.law == 8) wp.cs2v = dynamic_slot_field(ctx, velocity_slot);
  // (... and, with the dynamic subgrid heat flux on, the conductive row carries kappa + c_K Delta_K^2 gamma with C_theta
  // of the call's level pair)
  if (wp.law == 8 && scalar_slot != -1 && ctx->sc.dynflux.on)
    wp.cthv = dynamic_run(ctx, ctx->state[velocity_slot].p, ctx->state[scalar_slot].p);
  launch_wall_facets(s, m, W.n_facets, W.fcell.p, W.flocal.p, ctx->state[velocity_slot].p, ctx->state[pressure_slot].p,
                     scalar_slot != -1 ? ctx->state[scalar_slot].p : nullptr, wp, W.rows.p);
  launch_wall_reduce(s, m.dim, W.n_groups, W.goff.p, W.rows.p, W.sums.p);
  ++W.computes;
  NSFEM_HIP(hipMemcpyAsync(out_groups, W.sums.p, sizeof(double) * (size_t)W.n_groups * nw, hipMemcpyDeviceToHost, s));
  if (out_facets && W.n_facets > 0)
    NSFEM_HIP(hipMemcpyAsync(W.h_rows.data(), W.rows.p, sizeof(double) * W.h_rows.size(), hipMemcpyDeviceToHost, s));
  NSFEM_HIP(hipStreamSynchronize(s));
  if (out_facets)
    for (int32_t k = 0; k < W.n_facets; ++k)
      std::memcpy(out_facets + (size_t)W.h_perm[k] * nw, W.h_rows.data() + (size_t)k * nw, sizeof(double) * nw);
  API_END(ctx)
}

extern "C" int nsfem_wall_components(nsfem_ctx* ctx, int* nw) {
  API_BEGIN
  NSFEM_REQUIRE(ctx && nw, "null argument");
  *nw = wall_components(ctx->mesh.dim);
  API_END(ctx)
}

extern "C" int nsfem_wall_info(nsfem_ctx* ctx, int64_t out[4]) {
  API_BEGIN
  NSFEM_REQUIRE(ctx && out, "null argument");
  out[0] = ctx->wall.have_set ? ctx->wall.n_facets : 0;
  out[1] = ctx->wall.have_set ? ctx->wall.n_groups : 0;
  out[2] = ctx->wall.computes;
  out[3] = ctx->wall.uploads;
  API_END(ctx)
}

// ----------------------------------------------------------- operator access
static const BlockMat* get_op(nsfem_ctx* c, int op, int* nv_apply) {
  *nv_apply = 1;
  switch (op) {
    case NSFEM_OP_MASS_P2: return &c->M2;
    case NSFEM_OP_STIFF_P2: return &c->K2;
    case NSFEM_OP_STIFF_P1: return &c->Ap;
    case NSFEM_OP_MASS_P1: return &c->Mp;
    case NSFEM_OP_DIV: return &c->Dv;
    case NSFEM_OP_GRAD: return &c->Gr;
    case NSFEM_OP_DIVT: return &c->DT;
    case NSFEM_OP_MOMENTUM_JAC: return &c->J;
    case NSFEM_OP_VISCOUS_EXTRA:
      NSFEM_REQUIRE(c->have_E, "traction-form block not assembled (nsfem_set_viscous_form)");
      return &c->E;
    default: throw Error(NSFEM_ERR_ARG, "unknown operator id");
  }
}

extern "C" int nsfem_operator_shape(nsfem_ctx* ctx, int op, int64_t* n_rows, int64_t* n_cols,
                                    int64_t* nnz_scalar) {
  API_BEGIN
  NSFEM_REQUIRE(ctx, "null context");
  int nv;
  const BlockMat* A = get_op(ctx, op, &nv);
  if (n_rows) *n_rows = (int64_t)A->pat->n_rows * A->br;
  if (n_cols) *n_cols = (int64_t)A->pat->n_cols * A->bc;
  if (nnz_scalar) *nnz_scalar = (int64_t)A->pat->nnz * A->br * A->bc;
  API_END(ctx)
}

extern "C" int nsfem_operator_export(nsfem_ctx* ctx, int op, int32_t* rowptr, int32_t* col,
                                     double* val) {
  API_BEGIN
  NSFEM_REQUIRE(ctx && rowptr && col && val, "null argument");
  int nv;
  const BlockMat* A = get_op(ctx, op, &nv);
  const Pattern& p = *A->pat;
  const int br = A->br, bc = A->bc;
  std::vector<double> v((size_t)p.nnz * br * bc);
  NSFEM_HIP(hipMemcpyAsync(v.data(), A->vals.p, sizeof(double) * v.size(), hipMemcpyDeviceToHost,
                           ctx->stream));
  NSFEM_HIP(hipStreamSynchronize(ctx->stream));
  int64_t pos = 0;
  for (int R = 0; R < p.n_rows; ++R)
    for (int r = 0; r < br; ++r) {
      rowptr[(size_t)R * br + r] = (int32_t)pos;
      for (int k = p.h_rowptr[R]; k < p.h_rowptr[R + 1]; ++k)
        for (int cc = 0; cc < bc; ++cc) {
          col[pos] = p.h_col[k] * bc + cc;
          val[pos] = v[(size_t)k * br * bc + r * bc + cc];
          ++pos;
        }
    }
  rowptr[(size_t)p.n_rows * br] = (int32_t)pos;
  API_END(ctx)
}

// diagonal of a square scalar operator (one value per block row: 1 x 1 blocks) without exporting the matrix -- the
// algebraic Schur Laplacian needs diag(M_v) of a 1.3e8-entry mass matrix
extern "C" int nsfem_operator_diagonal(nsfem_ctx* ctx, int op, double* out) {
  API_BEGIN
  NSFEM_REQUIRE(ctx && out, "null argument");
  int nv;
  const BlockMat* A = get_op(ctx, op, &nv);
  const Pattern& p = *A->pat;
  NSFEM_REQUIRE(A->br == 1 && A->bc == 1 && p.n_rows == p.n_cols && p.diag.p, "diagonal: square scalar operators only");
  DevBuf<double> d;
  d.alloc((size_t)p.n_rows);
  launch_gather_diag(ctx->stream, p.n_rows, p.diag.p, A->vals.p, d.p);
  NSFEM_HIP(hipMemcpyAsync(out, d.p, sizeof(double) * (size_t)p.n_rows, hipMemcpyDeviceToHost, ctx->stream));
  NSFEM_HIP(hipStreamSynchronize(ctx->stream));
  API_END(ctx)
}

extern "C" int nsfem_operator_apply(nsfem_ctx* ctx, int op, const double* x, double* y) {
  API_BEGIN
  NSFEM_REQUIRE(ctx && x && y, "null argument");
  if (op == NSFEM_OP_MOMENTUM_JAC_MF) {      // matrix-free Jacobian at u = USTAR (parity tests)
    hipStream_t s = ctx->stream;
    const size_t n = (size_t)nvel(ctx);
    DevBuf<double> dx, dy;
    dx.alloc(n);
    dy.alloc(n);
    ensure_L(ctx);
    NSFEM_HIP(hipMemcpyAsync(dx.p, x, sizeof(double) * n, hipMemcpyHostToDevice, s));
    ctx->mom_mf.c = ctx;
    ctx->mom_mf.n = (int64_t)n;
    ctx->mom_mf.vel_slot = NSFEM_USTAR;
    ctx->mom_mf.apply(s, dx.p, dy.p);
    NSFEM_HIP(hipMemcpyAsync(y, dy.p, sizeof(double) * n, hipMemcpyDeviceToHost, s));
    NSFEM_HIP(hipStreamSynchronize(s));
    return NSFEM_OK;
  }
  int nv;
  const BlockMat* A = get_op(ctx, op, &nv);
  const Pattern& p = *A->pat;
  const size_t nx = (size_t)p.n_cols * A->bc, ny = (size_t)p.n_rows * A->br;
  DevBuf<double> dx, dy;
  dx.alloc(nx);
  dy.alloc(ny);
  hipStream_t s = ctx->stream;
  NSFEM_HIP(hipMemcpyAsync(dx.p, x, sizeof(double) * nx, hipMemcpyHostToDevice, s));
  launch_spmv(s, *A, 1, dx.p, dy.p, nullptr, MASK_NONE);
  NSFEM_HIP(hipMemcpyAsync(y, dy.p, sizeof(double) * ny, hipMemcpyDeviceToHost, s));
  NSFEM_HIP(hipStreamSynchronize(s));
  API_END(ctx)
}

// Test hook: one product / residual / Chebyshev smoothing sequence of a scalar lattice operator
// a M + b K (P2 or P1 space of the fine mesh) through a CHOSEN kernel family, on host data.  Lets the
// parity tests pin every SpMV kernel family and every epilogue to the oracle's matrices directly.
extern "C" int nsfem_kernel_apply(nsfem_ctx* ctx, nsfem_kernel_test* t) {
  API_BEGIN
  NSFEM_REQUIRE(ctx && t && (t->x || (t->family == 4 && t->epilogue == 3 && (t->xc || t->from_zero))) && t->y,
                "null argument");
  NSFEM_REQUIRE(t->nv >= 1 && t->nv <= 3 && t->steps >= 0 && t->steps <= 8, "bad kernel test description");
  NSFEM_REQUIRE(t->family == 4 || !(t->xc || t->rf || t->gh_lo || t->gh_hi || t->tile_lines),
                "fused transfers, ghost lines and launch overrides are lattice kernel (family 4) inputs");
  hipStream_t s = ctx->stream;
  const bool p2 = t->space == 0;
  const Pattern& pat = p2 ? ctx->p22 : ctx->p11;
  const BlockMat& Mm = p2 ? ctx->M2 : ctx->Mp;
  const BlockMat& Kk = p2 ? ctx->K2 : ctx->Ap;
  StencilDict& dict = p2 ? ctx->dict22 : ctx->dict11;
  bool& tried = p2 ? ctx->dict22_tried : ctx->dict11_tried;
  bool have_dict = dict.n_stencils > 0;
  if (!tried) {
    tried = true;
    have_dict = build_stencil_dict(s, pat, Mm.vals.p, Kk.vals.p, dict);
  }
  BlockMat T;
  T.init(&pat, 1, 1, s);
  launch_scale_combine(s, pat.nnz, t->a, Mm.vals.p, t->b_coef, Kk.vals.p, T.vals.p);
  if (have_dict) T.dict = &dict;
  T.sell_update(s);
  const int nv = t->nv;
  const size_t n = (size_t)pat.n_rows * nv;
  DevBuf<double> x, b, d, d2, y, y2, r, dinv;
  DevBuf<uint8_t> mask;
  if (t->x) x.upload(t->x, n, s);
  y.alloc(n); y.zero(s);
  y2.alloc(n); y2.zero(s);
  r.alloc(n); r.zero(s);
  b.alloc(n); b.zero(s);
  d.alloc(n); d.zero(s);
  d2.alloc(n); d2.zero(s);
  if (t->b) NSFEM_HIP(hipMemcpyAsync(b.p, t->b, sizeof(double) * n, hipMemcpyHostToDevice, s));
  if (t->d) NSFEM_HIP(hipMemcpyAsync(d.p, t->d, sizeof(double) * n, hipMemcpyHostToDevice, s));
  if (t->mask) mask.upload(t->mask, n, s);
  const uint8_t* mk = t->mask ? mask.p : nullptr;
  int family = t->family;
  if (family == 1) { T.dict_ready = false; T.sell_ready = false; }
  else if (family == 2) { T.dict_ready = false; NSFEM_REQUIRE(T.sell_ready, "no SELL-64 layout for this pattern"); }
  else if (family == 3) { NSFEM_REQUIRE(T.dict_ready, "no stencil dictionary for this pattern"); T.sell_ready = false; }
  else if (family == 4) { NSFEM_REQUIRE(lattice_smoother_available(T, nv), "no lattice structure for this pattern"); }
  // used_family: the dispatcher's own decision for the launch below (whole operator, one output) as a family number
  auto family_of = [](SpmvPath path) {
    return path == SpmvPath::DictBlock || path == SpmvPath::DictScalar ? 3 : (path == SpmvPath::Sell ? 2 : 1);
  };
  const double* result = y.p;
  if (t->epilogue == 0) {
    t->used_family = family_of(spmv_path(T, nv, EPI_STORE, 0, t->dict_ok != 0, false));
    launch_spmv(s, T, nv, x.p, y.p, mk, mk ? t->maskmode : MASK_NONE, t->ghost, 0, t->dict_ok);
  } else if (t->epilogue == 1) {
    NSFEM_REQUIRE(t->b, "residual needs b");
    t->used_family = family_of(spmv_path(T, nv, EPI_RESID, 0, false, false));
    launch_residual(s, T, nv, x.p, b.p, y.p, mk, mk ? t->maskmode : MASK_NONE);
  } else {
    NSFEM_REQUIRE((t->b || (family == 4 && t->rf)) && t->steps >= 1, "smoothing needs b and steps >= 1");
    if (family == 4) {
      t->used_family = 4;
      NSFEM_REQUIRE(!(t->from_zero && t->xc), "lattice kernel: a zero start takes no coarse correction");
      const bool fz = t->from_zero != 0;
      NSFEM_REQUIRE(t->steps <= lattice_smoother_max_steps(T, fz, t->with_residual != 0),
                    "too many steps for one launch of the lattice kernel");
      // fused transfers: the coarse (even-even sublattice) and the finer lattice of this level
      const StencilDict& D = *T.dict;
      const size_t nc = (size_t)((D.lat_w + 1) / 2) * ((D.lat_h + 1) / 2) * nv;
      const size_t nf = (size_t)(2 * D.lat_w - 1) * (2 * D.lat_h - 1) * nv;
      DevBuf<double> xc, rf, bo;
      if (t->xc) xc.upload(t->xc, nc, s);
      if (t->rf) {
        rf.upload(t->rf, nf, s);
        bo.alloc(n);
        bo.zero(s);
      }
      LatticeLaunchOverride ov;
      ov.tile_lines = t->tile_lines;
      ov.fixed = t->fixed;
      // (no d_out on the host: the launch stores no direction either -- the launch kinds without d_out)
      launch_cheb_lattice(s, T, nv, (fz || !t->x) ? nullptr : x.p, b.p, (t->d && !fz) ? d.p : nullptr, y.p,
                          t->d_out ? d2.p : nullptr, t->with_residual ? r.p : nullptr, mk, t->steps, t->c1, t->c2,
                          t->ident, nullptr,
                          t->xc ? xc.p : nullptr, t->rf ? rf.p : nullptr, t->rf ? bo.p : nullptr, t->gh_lo, t->gh_hi,
                          t->gh_zero, &ov);
      if (t->d_out) NSFEM_HIP(hipMemcpyAsync(d.p, d2.p, sizeof(double) * n, hipMemcpyDeviceToDevice, s));
      if (t->rf && t->b_formed) NSFEM_HIP(hipMemcpyAsync(t->b_formed, bo.p, sizeof(double) * n, hipMemcpyDeviceToHost, s));
      NSFEM_HIP(hipStreamSynchronize(s));      // (before the transfer buffers go out of scope)
      t->lattice_tile_lines = ov.used_tile_lines;
      t->lattice_tx = ov.tx;
      t->lattice_ty = ov.ty;
      t->lattice_tiles = ov.tiles;
      t->lattice_fixed_shape = ov.fixed_shape;
      t->lattice_kind = ov.kind;
    } else {
      t->used_family = family_of(spmv_path(T, nv, EPI_CHEB, 0, true, false));
      dinv.alloc(n);
      launch_inv_diag(s, T, nv, mk, dinv.p);
      const double* cur = x.p;
      if (t->from_zero) { x.zero(s); d.zero(s); }
      for (int k = 0; k < t->steps; ++k) {
        double* out = cur == y.p ? y2.p : y.p;
        launch_cheb_step(s, T, nv, cur, b.p, dinv.p, d.p, t->c1[k], t->c2[k], out, mk, t->ghost, 0,
                         t->ident && k == t->steps - 1 ? 1 : 0);
        cur = out;
      }
      result = cur;
      if (t->with_residual) launch_residual(s, T, nv, cur, b.p, r.p, mk, MASK_ZERO);
    }
  }
  NSFEM_HIP(hipMemcpyAsync(t->y, result, sizeof(double) * n, hipMemcpyDeviceToHost, s));
  if (t->d_out) NSFEM_HIP(hipMemcpyAsync(t->d_out, d.p, sizeof(double) * n, hipMemcpyDeviceToHost, s));
  if (t->r_out) NSFEM_HIP(hipMemcpyAsync(t->r_out, r.p, sizeof(double) * n, hipMemcpyDeviceToHost, s));
  NSFEM_HIP(hipStreamSynchronize(s));
  t->dict_entries = have_dict ? dict.n_stencils : 0;
  t->dict_exact = have_dict && dict.exact ? 1 : 0;
  t->lattice_w = have_dict ? dict.lat_w : 0;
  API_END(ctx)
}

// Test hook: the standalone restrictions of a lattice hierarchy (k_restrict_lattice, k_restrict_lattice2) on host data
extern "C" int nsfem_lattice_restrict(nsfem_ctx* ctx, int nv, int levels, int w, int h, const double* rf,
                                      const uint8_t* mask1, const uint8_t* mask2, double* b1, double* b2) {
  API_BEGIN
  NSFEM_REQUIRE(ctx && rf && b1 && (levels == 1 || (levels == 2 && b2)), "null argument");
  NSFEM_REQUIRE(nv >= 1 && nv <= 2 && w >= 1 && h >= 1, "bad restriction description");
  hipStream_t s = ctx->stream;
  const int w1 = levels == 1 ? w : 2 * w - 1, h1 = levels == 1 ? h : 2 * h - 1;
  const int wf = 2 * w1 - 1, hf = 2 * h1 - 1;
  const size_t n1 = (size_t)w1 * h1 * nv, n2 = (size_t)w * h * nv, nf = (size_t)wf * hf * nv;
  DevBuf<double> f, o1, o2;
  DevBuf<uint8_t> m1, m2;
  f.upload(rf, nf, s);
  o1.alloc(n1);
  o1.zero(s);
  if (mask1) m1.upload(mask1, n1, s);
  if (levels == 1) {
    NSFEM_REQUIRE(launch_restrict_lattice(s, nv, w1, h1, wf, hf, f.p, mask1 ? m1.p : nullptr, o1.p),
                  "restriction: lattices do not nest");
  } else {
    o2.alloc(n2);
    o2.zero(s);
    if (mask2) m2.upload(mask2, n2, s);
    NSFEM_REQUIRE(launch_restrict_lattice2(s, nv, w, h, w1, h1, wf, hf, f.p, mask1 ? m1.p : nullptr,
                                           mask2 ? m2.p : nullptr, o1.p, o2.p),
                  "restriction: lattices do not nest");
    NSFEM_HIP(hipMemcpyAsync(b2, o2.p, sizeof(double) * n2, hipMemcpyDeviceToHost, s));
  }
  NSFEM_HIP(hipMemcpyAsync(b1, o1.p, sizeof(double) * n1, hipMemcpyDeviceToHost, s));
  NSFEM_HIP(hipStreamSynchronize(s));
  API_END(ctx)
}

// The shared tail of the four setters: the factors set last are the ones precond = 3 uses, so the other object is
// released.  Captured CG bodies hold the addresses of 3D factors and work buffers (FastDiag3 as op.prec): the graph
// epoch moves whenever 3D factors are installed or released (not for a plain 2D re-set: nothing captures those).
static void fast_diag_installed(nsfem_ctx* ctx, bool box) {
  if (box || ctx->fd3_p.ready()) ctx->graph_epoch++;
  if (box) ctx->fd_p.release();
  else ctx->fd3_p.release();
}

// Factors of the fast diagonalisation of the pressure Poisson operator (poisson_fd.factors): the P1 space must be
// the W x H lattice in lexicographic numbering, the pressure Dirichlet set a union of whole sides (or empty).
// Krylov option precond = 3 of the projection step then solves it directly (four dense products on the matrix cores).
extern "C" int nsfem_poisson_set_fast_diag(nsfem_ctx* ctx, int32_t W, int32_t H, const double* Vx, const double* Vy,
                                           const double* inv) {
  API_BEGIN
  NSFEM_REQUIRE(ctx && Vx && Vy && inv, "null argument");
  NSFEM_REQUIRE((int64_t)W * H == npre(ctx), "fast diagonalisation: W x H must be the number of pressure dofs");
  NSFEM_REQUIRE(!ctx->distributed(), "partitioned context: nsfem_poisson_set_fast_diag_rows");
  ctx->fd_p.set(ctx->stream, W, H, Vx, Vy, inv);
  fast_diag_installed(ctx, false);
  API_END(ctx)
}

// Factors of a 3D box lattice (poisson_fd.factors_3d): the P1 space must be the Nz x Ny x Nx lattice in lexicographic
// numbering (x fastest), the pressure Dirichlet set a union of whole faces (or empty).  exact != 0: T is the stiffness
// matrix itself and precond = 3 solves directly; exact == 0: precond = 3 runs CG preconditioned by T^+.
extern "C" int nsfem_poisson_set_fast_diag_3d(nsfem_ctx* ctx, int32_t Nx, int32_t Ny, int32_t Nz, const double* Vx,
                                              const double* Vy, const double* Vz, const double* inv, int32_t exact) {
  API_BEGIN
  NSFEM_REQUIRE(ctx && Vx && Vy && Vz && inv, "null argument");
  NSFEM_REQUIRE(!ctx->distributed(), "fast diagonalisation (3D): partitioned contexts are not supported");
  NSFEM_REQUIRE(Nx >= 2 && Ny >= 2 && Nz >= 2 && (int64_t)Nx * Ny * Nz == npre(ctx),
                "fast diagonalisation (3D): Nx x Ny x Nz must be the number of pressure dofs");
  ctx->fd3_p.set(ctx->stream, Nx, Ny, Nz, Vx, Vy, Vz, inv, exact != 0);
  fast_diag_installed(ctx, true);
  API_END(ctx)
}

// out = {Nx, Ny, Nz, exact, host-issued applications of T^+, projection solves with the factors}; zeros when none
extern "C" int nsfem_poisson_fast_diag_3d_info(nsfem_ctx* ctx, int64_t out[6]) {
  API_BEGIN
  NSFEM_REQUIRE(ctx && out, "null argument");
  const nsfem::FastDiag3& f = ctx->fd3_p;
  const bool on = f.ready();
  out[0] = on ? f.Nx : 0;
  out[1] = on ? f.Ny : 0;
  out[2] = on ? f.Nz : 0;
  out[3] = on && f.exact ? 1 : 0;
  out[4] = f.applications;
  out[5] = f.solves;
  API_END(ctx)
}

// Partitioned strips: the factors of the GLOBAL W x H lattice; this rank's P1 space is the lattice lines
// first_line ... first_line + n_p1 / W - 1 (ghost lines included).  The fused step driver then solves the projection
// step with one all-reduce of H x W doubles (FastDiag::apply on strip factors).
extern "C" int nsfem_poisson_set_fast_diag_rows(nsfem_ctx* ctx, int32_t W, int32_t H, int32_t first_line,
                                                const double* Vx, const double* Vy, const double* inv) {
  API_BEGIN
  NSFEM_REQUIRE(ctx && Vx && Vy && inv && W >= 2, "null argument");
  NSFEM_REQUIRE(ctx->distributed(), "strip factors need a partitioned context (nsfem_set_partition)");
  const int64_t np = npre(ctx);
  NSFEM_REQUIRE(np % W == 0 && first_line >= 0 && first_line + np / W <= H,
                "fast diagonalisation: the local pressure space is not a run of whole lattice lines");
  NSFEM_REQUIRE((int64_t)W * H == ctx->n_p1_global, "fast diagonalisation: W x H must be the global number of pressure dofs");
  ctx->fd_p.set_rows(ctx->stream, W, H, first_line, (int)(np / W), Vx, Vy, inv);
  fast_diag_installed(ctx, false);
  API_END(ctx)
}

// Partitioned slabs of a 3D box lattice: the factors of the GLOBAL Nz x Ny x Nx lattice; this rank's P1 space is the
// lattice planes (first_plane + i) mod Nz, i < n_p1 / (Nx Ny) (ghost planes included), and the planes it owns (the P1
// ghost flags of nsfem_set_partition) are one contiguous run.  precond = 3 then solves the projection step with one
// all-reduce of Nz x Ny x Nx doubles (FastDiag3::apply on slab factors): directly for exact factors, as the
// preconditioner of CG otherwise.
extern "C" int nsfem_poisson_set_fast_diag_3d_planes(nsfem_ctx* ctx, int32_t Nx, int32_t Ny, int32_t Nz,
                                                     int32_t first_plane, const double* Vx, const double* Vy,
                                                     const double* Vz, const double* inv, int32_t exact) {
  API_BEGIN
  NSFEM_REQUIRE(ctx && Vx && Vy && Vz && inv, "null argument");
  NSFEM_REQUIRE(ctx->distributed(), "slab factors need a partitioned context with a communicator "
                                    "(nsfem_set_partition, nsfem_comm_attach_*)");
  NSFEM_REQUIRE(Nx >= 2 && Ny >= 2 && Nz >= 2, "fast diagonalisation (3D): bad dims");
  const int64_t np = npre(ctx), pl = (int64_t)Nx * Ny;
  NSFEM_REQUIRE(np % pl == 0, "fast diagonalisation (3D): the local pressure space is not a run of whole lattice planes");
  NSFEM_REQUIRE(pl * Nz == ctx->n_p1_global,
                "fast diagonalisation (3D): Nx x Ny x Nz must be the global number of pressure dofs");
  const int64_t n_loc = np / pl;
  NSFEM_REQUIRE(first_plane >= 0 && first_plane < Nz && n_loc <= 65535,
                "fast diagonalisation (3D): first plane out of range / too many local planes");
  NSFEM_REQUIRE(ctx->partition_periodic || first_plane + n_loc <= Nz,
                "fast diagonalisation (3D): the local planes wrap around on a partition that is not periodic");
  // the owned planes: every plane wholly owned or wholly ghost, the owned ones one contiguous run
  const std::vector<uint8_t>& g = ctx->h_ghost_p1;
  NSFEM_REQUIRE((int64_t)g.size() == np, "fast diagonalisation (3D): no P1 ghost flags (nsfem_set_partition)");
  int64_t own0 = -1, own_end = -1;
  bool run = true;
  for (int64_t i = 0; i < n_loc && run; ++i) {
    const uint8_t* q = g.data() + i * pl;
    const bool owned = q[0] == 0;
    for (int64_t j = 1; j < pl && run; ++j) run = (q[j] == 0) == owned;
    if (!owned) continue;
    if (own0 < 0) own0 = i;
    else if (own_end != i) run = false;
    own_end = i + 1;
  }
  NSFEM_REQUIRE(run && own0 >= 0,
                "fast diagonalisation (3D): the owned pressure dofs are not one contiguous run of whole lattice planes");
  ctx->fd3_p.set_planes(ctx->stream, Nx, Ny, Nz, first_plane, (int)n_loc, (int)own0, (int)(own_end - own0), Vx, Vy, Vz,
                        inv, exact != 0);
  fast_diag_installed(ctx, true);
  API_END(ctx)
}

// Test hook: one application z = M^-1 r of a multigrid preconditioner on host vectors -- which = 0 pressure Poisson
// hierarchy (mg_p), 1 velocity hierarchy (mg_v, the identity rows of the Newton preconditioner included), 2 the
// fast-diagonalisation solve z = A^+ r of the active factors (FastDiagBase::apply; on strip and slab factors a
// collective), 3 the Schur hierarchy (mg_s: its own Dirichlet set NSFEM_PRESSURE_PRECOND, geometric or algebraic
// level operators), 4 the pressure mass smoother (mg_m) -- the last two after the refreshes nsfem_step_bdf makes, on
// single contexts only.  Lets the parity tests compare kernel families cycle by cycle.
extern "C" int nsfem_mg_apply(nsfem_ctx* ctx, int which, const double* r, double* z) {
  API_BEGIN
  NSFEM_REQUIRE(ctx && r && z && which >= 0 && which <= 4, "bad argument");
  hipStream_t s = ctx->stream;
  if (which >= 3) {                    // the two hierarchies of the block preconditioner's pressure part
    NSFEM_REQUIRE(!ctx->distributed(), "nsfem_mg_apply(3 | 4) takes single contexts only (this context has a "
                                       "communicator)");
    NSFEM_REQUIRE(ctx->mg_built, "no multigrid hierarchy (nsfem_mg_finalize)");
    ensure_L(ctx);                     // (builds the dictionaries of the fine P1 operators as well)
    mg_refresh_schur(ctx);
    const int64_t n = npre(ctx);
    DevBuf<double> dr, dz;
    dr.upload(r, (size_t)n, s);
    dz.alloc((size_t)n);
    dz.zero(s);
    (which == 3 ? ctx->mg_s : ctx->mg_m).apply(s, dr.p, dz.p);
    NSFEM_HIP(hipMemcpyAsync(z, dz.p, sizeof(double) * n, hipMemcpyDeviceToHost, s));
    NSFEM_HIP(hipStreamSynchronize(s));
    return NSFEM_OK;
  }
  if (which == 2) {                    // the fast-diagonalisation Poisson solve z = A^+ r
    const int64_t n = npre(ctx);
    DevBuf<double> dr, dz;
    dr.upload(r, (size_t)n, s);
    dz.alloc((size_t)n);
    nsfem::FastDiagBase* fd = ctx->fast_diag();
    NSFEM_REQUIRE(fd, "fast diagonalisation: factors not set (or set for a strip)");
    if (fd->reads_ghosts()) {          // strips (a collective: every rank calls it): ghost rows zeroed, as the step does
      NSFEM_REQUIRE(ctx->distributed(), "strip factors need a partitioned context");
      launch_zero_ghost(s, n, ctx->mask_p.p, dr.p);
    }
    fd->apply(s, dr.p, dz.p);          // (slab factors: a collective as well, ghost planes of r ignored)
    NSFEM_HIP(hipMemcpyAsync(z, dz.p, sizeof(double) * n, hipMemcpyDeviceToHost, s));
    NSFEM_HIP(hipStreamSynchronize(s));
    return NSFEM_OK;
  }
  NSFEM_REQUIRE(ctx->mg_built, "no multigrid hierarchy (nsfem_mg_finalize)");
  ensure_L(ctx);                       // (builds the dictionaries of the fine P1 operators as well)
  if (which == 0) ctx->mg_p_dirty = true;   // (refreshed before the dictionaries of the fine P1 operators existed)
  mg_refresh(ctx, which == 1);
  const int64_t n = which == 1 ? nvel(ctx) : npre(ctx);
  DevBuf<double> dr, dz;
  dr.upload(r, (size_t)n, s);
  dz.alloc((size_t)n);
  dz.zero(s);
  (which == 1 ? ctx->mg_v : ctx->mg_p).apply(s, dr.p, dz.p);
  NSFEM_HIP(hipMemcpyAsync(z, dz.p, sizeof(double) * n, hipMemcpyDeviceToHost, s));
  NSFEM_HIP(hipStreamSynchronize(s));
  API_END(ctx)
}

// How a multigrid cycle runs: which = 0 / 1: out = {0, 0, levels in use, 0} (the two zero fields are reserved);
// which = 2 / 3: the multi-step lattice kernel on the hierarchy; which = 4 / 5 and 6 / 7: the same two records for the
// Schur hierarchy mg_s / the mass smoother mg_m (single contexts)
extern "C" int nsfem_mg_info(nsfem_ctx* ctx, int which, int64_t out[4]) {
  API_BEGIN
  NSFEM_REQUIRE(ctx && out && which >= 0 && which <= 7, "bad argument");
  NSFEM_REQUIRE(which < 4 || !ctx->distributed(), "nsfem_mg_info(4 .. 7) takes single contexts only (this context "
                                                  "has a communicator)");
  NSFEM_REQUIRE(ctx->mg_built, "no multigrid hierarchy (nsfem_mg_finalize)");
  ensure_L(ctx);
  if (which >= 4) mg_refresh_schur(ctx);
  else mg_refresh(ctx, (which & 1) == 1);
  Multigrid& mg = which >= 4 ? ((which & 1) ? ctx->mg_m : ctx->mg_s) : ((which & 1) ? ctx->mg_v : ctx->mg_p);
  if (which & 2) {                     // the multi-step lattice kernel on this hierarchy (strips: relaxed halo mode)
    const size_t n_used = mg.truncated() ? mg.active : mg.lv.size();
    int64_t levels = 0;
    for (size_t l = 0; l < n_used; ++l) levels += (mg.lattice_ok(mg.lv[l]) || mg.lattice_ok_relaxed(mg.lv[l])) ? 1 : 0;
    out[0] = levels;
    out[1] = mg.lattice_launches;
    out[2] = (int64_t)n_used;
    out[3] = mg.lv[0].ghost_lo >= 0 ? mg.lv[0].ghost_lo * 256 + mg.lv[0].ghost_hi : 0;
    return NSFEM_OK;
  }
  out[0] = 0;
  out[1] = 0;
  out[2] = (int64_t)(mg.truncated() ? mg.active : mg.lv.size());
  out[3] = 0;
  API_END(ctx)
}

// In-situ timing of the dominant kernel: while enabled, every finest-level Chebyshev smoothing
// launch of the velocity multigrid (k_spmv_stream<1,1,dim,EPI_CHEB>) is bracketed by a HIP-event
// pair on the context's stream.  enable != 0: start (discarding earlier samples); enable == 0:
// stop and return the average launch duration, the number of launches and the algorithmic bytes
// per launch.
// algorithmic bytes of one Chebyshev smoothing launch with operator A on nv interleaved vectors.
// Vectors: x, b, dinv, d read; d, x_out written (8 bytes each) + 1 mask byte per entry.  Matrix: a
// CSR stream (12 bytes per nonzero + row pointers) or -- stencil-dictionary copy -- one byte per
// row + the dictionary once.
static int64_t smoother_launch_bytes(const BlockMat& A, int nv, bool csr_equivalent) {
  const Pattern& p = *A.pat;
  const int64_t n = (int64_t)p.n_rows * nv;
  if (A.dict_ready && !csr_equivalent)     // (no dinv stream: 1 / diagonal comes from the dictionary)
    return (int64_t)p.n_rows + (int64_t)A.dict->n_stencils * (A.dict->lmax * 12 + 4) + n * (5 * 8 + 1);
  return (int64_t)p.nnz * 12 + (int64_t)(p.n_rows + 1) * 4 + n * (6 * 8 + 1);
}

extern "C" int nsfem_profile_smoother(nsfem_ctx* ctx, int enable, double* avg_ms, int64_t* launches,
                                      int64_t* algorithmic_bytes) {
  API_BEGIN
  NSFEM_REQUIRE(ctx, "null context");
  NSFEM_REQUIRE(ctx->mg_built, "no multigrid hierarchy (nsfem_mg_finalize)");
  Multigrid& mg = ctx->mg_v;
  if (enable) {
    if (mg.prof_ev.empty()) {
      mg.prof_ev.resize(8192);
      for (hipEvent_t& e : mg.prof_ev) NSFEM_HIP(hipEventCreate(&e));
    }
    mg.prof_n = 0;
    mg.prof_launches = 0;
    mg.prof_steps = 0;
    mg.prof_bytes = 0;
    mg.prof = true;
    ctx->kw.graphs_suspended = true;     // (HIP events are recorded inside the iteration bodies)
    ctx->kw.clear_graphs();
    return NSFEM_OK;
  }
  mg.prof = false;
  ctx->kw.graphs_suspended = ctx->conv_probe.on;
  NSFEM_HIP(hipStreamSynchronize(ctx->stream));
  double total = 0.0;
  for (size_t i = 0; i + 1 < mg.prof_n; i += 2) {
    float t = 0.f;
    NSFEM_HIP(hipEventElapsedTime(&t, mg.prof_ev[i], mg.prof_ev[i + 1]));
    total += t;
  }
  const int64_t n_launch = mg.prof_launches;
  if (avg_ms) *avg_ms = n_launch ? total / (double)n_launch : 0.0;
  if (launches) *launches = n_launch;
  // (lattice kernel: launches of different shapes -- with / without the carried direction -- were
  // timed; the average over exactly those launches)
  if (algorithmic_bytes)
    *algorithmic_bytes = (mg.prof_bytes > 0 && n_launch > 0) ? mg.prof_bytes / n_launch
                                                             : smoother_launch_bytes(*mg.lv[0].A, mg.nv, false);
  API_END(ctx)
}

// detail of the last nsfem_profile_smoother window: out = {launches, smoothing steps they ran,
// algorithmic bytes they moved in total, 1 when the multi-step lattice kernel ran them}
extern "C" int nsfem_profile_smoother_detail(nsfem_ctx* ctx, int64_t out[4]) {
  API_BEGIN
  NSFEM_REQUIRE(ctx && out, "null argument");
  const Multigrid& mg = ctx->mg_v;
  out[0] = mg.prof_launches;
  out[1] = mg.prof_steps;
  out[2] = mg.prof_bytes > 0 ? mg.prof_bytes
                             : (mg.lv.empty() ? 0 : mg.prof_launches * smoother_launch_bytes(*mg.lv[0].A, mg.nv, false));
  out[3] = mg.prof_bytes > 0 ? 1 : 0;
  API_END(ctx)
}

// which finest-level smoothing kernel of the velocity multigrid runs, and what a CSR stream of the
// same operator would move: out = {kind (0 CSR-stream, 1 SELL-64, 2 stencil dictionary, 3 stencil
// dictionary inside the multi-step lattice kernel),
// dictionary entries, longest row, CSR-equivalent algorithmic bytes of one smoothing launch}
extern "C" int nsfem_smoother_info(nsfem_ctx* ctx, int64_t out[4]) {
  API_BEGIN
  NSFEM_REQUIRE(ctx && out, "null argument");
  NSFEM_REQUIRE(ctx->mg_built, "no multigrid hierarchy (nsfem_mg_finalize)");
  ensure_L(ctx);
  const Multigrid& mg = ctx->mg_v;
  const BlockMat& A = *mg.lv[0].A;
  Multigrid& mgw = ctx->mg_v;
  out[0] = A.dict_ready ? ((mg.lattice_ok(mg.lv[0]) || mgw.lattice_ok_relaxed(mgw.lv[0])) ? 3 : 2) : (A.sell_ready ? 1 : 0);
  out[1] = A.dict_ready ? A.dict->n_stencils : 0;
  out[2] = A.dict_ready ? (A.dict->exact ? -A.dict->lmax : A.dict->lmax) : 0;
  out[3] = smoother_launch_bytes(A, mg.nv, true);
  API_END(ctx)
}

// launches so far of the fused step frame (NSFEM_STEP_FUSED): out = {pair kernel in the begin step, pair kernel in the
// correction assembly, k_correction_finish, fused projection epilogue}
extern "C" int nsfem_step_frame_info(nsfem_ctx* ctx, int64_t out[4]) {
  API_BEGIN
  NSFEM_REQUIRE(ctx && out, "null argument");
  for (int i = 0; i < 4; ++i) out[i] = ctx->step_frame_launches[i];
  API_END(ctx)
}

// residual launches so far that carried the frame of the Newton iteration (NSFEM_NEWTON_FUSED): out = {launches with
// the Dirichlet rows and the sum of squares, those among them that also applied the update u* -= dx}
extern "C" int nsfem_newton_frame_info(nsfem_ctx* ctx, int64_t out[2]) {
  API_BEGIN
  NSFEM_REQUIRE(ctx && out, "null argument");
  for (int i = 0; i < 2; ++i) out[i] = ctx->newton_frame_launches[i];
  API_END(ctx)
}

extern "C" int nsfem_jacobian_info(nsfem_ctx* ctx, int64_t out[4]) {
  API_BEGIN
  NSFEM_REQUIRE(ctx && out, "null argument");
  ensure_L(ctx);
  out[0] = jacobian_path(ctx);
  out[1] = ctx->jac_lattice_launches;
  out[2] = jacobian_lattice_bytes(ctx->mesh);
  out[3] = jacobian_path(ctx) == 2 ? jacobian_lattice_variant(ctx->mesh) : -1;
  API_END(ctx)
}

extern "C" int nsfem_jacobian_table_check(nsfem_ctx* ctx, int64_t* bad_cells) {
  API_BEGIN
  NSFEM_REQUIRE(ctx && bad_cells, "null argument");
  ensure_L(ctx);
  (void)jacobian_path(ctx);                          // (builds the cell lattice and the tables on first use)
  *bad_cells = check_gradient_tables(ctx->stream, ctx->mesh);
  API_END(ctx)
}

// Algorithmic bytes of one matrix-free convection action  y += c_c [d conv(u)/du] x  (SURVEY.md
// section 8d, "assembly of a vector"): per cell the vertex coordinates, the P2 dof ids and the
// nodal values of u and x gathered through them; the output vector read-modify-written once.
static int64_t convection_action_bytes(const nsfem_ctx* c) {
  const int64_t dim = c->mesh.dim, nl1 = dim + 1, nl2 = dim == 2 ? 6 : 10;
  return (int64_t)c->mesh.n_cells * (nl1 * dim * 8 + nl2 * 4 + 2 * nl2 * dim * 8) +
         (int64_t)c->mesh.n_p2 * dim * 16;
}
// one GPU, triangles, lattice mesh: the per-node sums run inside the L-product launch (MomentumMF::apply); the
// probe then brackets the element kernel alone, whose bytes are the per-cell part plus the element vectors it
// stores (dim * nl2 doubles per cell, summed by the other launch)
static bool convection_gather_fused(const nsfem_ctx* c) {
  return !c->distributed() && c->mesh.dim == 2 && c->L.dict_ready;
}
static int64_t convection_cells_bytes(const nsfem_ctx* c) {
  const int64_t dim = c->mesh.dim, nl1 = dim + 1, nl2 = dim == 2 ? 6 : 10;
  return (int64_t)c->mesh.n_cells * (nl1 * dim * 8 + nl2 * 4 + 2 * nl2 * dim * 8 + nl2 * dim * 8);
}

// In-situ timing of the matrix-free convection action inside the Newton-Krylov solves (one HIP-event
// pair around every k_conv_cell<FORM,LIN> + k_res_gather pair on the context's stream).
extern "C" int nsfem_profile_convection(nsfem_ctx* ctx, int enable, double* avg_ms,
                                        int64_t* applications, int64_t* algorithmic_bytes) {
  API_BEGIN
  NSFEM_REQUIRE(ctx, "null context");
  nsfem_ctx::Probe& pr = ctx->conv_probe;
  if (enable) {
    if (pr.ev.empty()) {
      pr.ev.resize(4096);
      for (hipEvent_t& e : pr.ev) NSFEM_HIP(hipEventCreate(&e));
    }
    pr.n = 0;
    pr.on = true;
    ctx->kw.graphs_suspended = true;     // (HIP events are recorded inside the iteration bodies)
    ctx->kw.clear_graphs();
    return NSFEM_OK;
  }
  pr.on = false;
  ctx->kw.graphs_suspended = ctx->mg_v.prof;
  NSFEM_HIP(hipStreamSynchronize(ctx->stream));
  double total = 0.0;
  for (size_t i = 0; i + 1 < pr.n; i += 2) {
    float t = 0.f;
    NSFEM_HIP(hipEventElapsedTime(&t, pr.ev[i], pr.ev[i + 1]));
    total += t;
  }
  const int64_t n = (int64_t)(pr.n / 2);
  if (avg_ms) *avg_ms = n ? total / (double)n : 0.0;
  if (applications) *applications = n;
  if (algorithmic_bytes)
    *algorithmic_bytes = jacobian_path(ctx) == 2 ? jacobian_lattice_bytes(ctx->mesh)
                         : convection_gather_fused(ctx) ? -convection_cells_bytes(ctx) : convection_action_bytes(ctx);
  API_END(ctx)
}

// milliseconds of `reps` rounds (flush, step) on s between two events, after 3 rounds of warm-up
template <class Flush, class Step>
static double time_rounds(hipStream_t s, int reps, Flush&& flush, Step&& step) {
  hipEvent_t e0, e1;
  NSFEM_HIP(hipEventCreate(&e0));
  NSFEM_HIP(hipEventCreate(&e1));
  for (int i = 0; i < 3; ++i) { flush(); step(); }
  NSFEM_HIP(hipEventRecord(e0, s));
  for (int i = 0; i < reps; ++i) { flush(); step(); }
  NSFEM_HIP(hipEventRecord(e1, s));
  NSFEM_HIP(hipEventSynchronize(e1));
  float t = 0.f;
  NSFEM_HIP(hipEventElapsedTime(&t, e0, e1));
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
  return (double)t;
}

extern "C" int nsfem_time_spmv(nsfem_ctx* ctx, int op, int reps, double* ms_per_launch,
                               int64_t* algorithmic_bytes) {
  API_BEGIN
  NSFEM_REQUIRE(ctx && reps != 0 && ms_per_launch, "bad argument");
  auto nothing = [] {};
  // reps < 0 (smoother only): |reps| back-to-back launches without the cache-flushing launches in
  // between (the operands stay in the 256 MiB Infinity Cache when they fit)
  const bool warm = reps < 0;
  if (warm) reps = -reps;
  if (op == NSFEM_OP_CONVECTION_ACTION) {
    // matrix-free convection action at u = U1 in the direction x = U0, each repetition preceded by
    // a cache-flushing product with the block Jacobian array (timed separately and subtracted)
    hipStream_t s = ctx->stream;
    const double cc = cc_of(ctx) != 0.0 ? cc_of(ctx) : 1.0;
    DevBuf<double> fx, fy, y;
    fx.alloc((size_t)nvel(ctx));
    fy.alloc((size_t)nvel(ctx));
    y.alloc((size_t)nvel(ctx));
    fx.zero(s);
    y.zero(s);
    auto flush = [&] { launch_spmv(s, ctx->J, 1, fx.p, fy.p, nullptr, MASK_NONE); };
    auto step = [&] {
      launch_convection_action(s, ctx->mesh, ctx->state[NSFEM_U1].p, ctx->state[NSFEM_U0].p, cc, y.p,
                               ctx->conv_form, false);
    };
    const double t_both = time_rounds(s, reps, flush, step), t_flush = time_rounds(s, reps, flush, nothing);
    *ms_per_launch = (t_both - t_flush) / reps;
    if (algorithmic_bytes) *algorithmic_bytes = convection_action_bytes(ctx);
    return NSFEM_OK;
  }
  if (op == NSFEM_OP_MOMENTUM_SMOOTHER) {
    // one Chebyshev-Jacobi smoothing step of the velocity multigrid on its finest level: the
    // scalar P2 operator L applied to the interleaved components with the fused epilogue
    // d = c1 d + c2 dinv (b - L x), y = x + d  (k_spmv_stream<1,1,dim,EPI_CHEB>)
    NSFEM_REQUIRE(ctx->mg_built, "no multigrid hierarchy (nsfem_mg_finalize)");
    mg_refresh(ctx, true);
    hipStream_t s = ctx->stream;
    Multigrid& mg = ctx->mg_v;
    MGLevel& L0 = mg.lv[0];
    const Pattern& p = *L0.A->pat;
    const int nv = mg.nv;
    const bool lattice = mg.lattice_ok(L0);
    const int lat_steps = mg.degree >= 1 && mg.degree <= 3 ? mg.degree : 3;
    auto step = [&] {
      if (lattice) {       // the post-smoothing launch of the cycle: `degree` steps from a given iterate
        const double c1[4] = {0.0, 0.3, 0.3, 0.3}, c2[4] = {0.7, 0.7, 0.7, 0.7};
        launch_cheb_lattice(s, *L0.A, nv, L0.xa.p, L0.r.p, nullptr, L0.xb.p, nullptr, nullptr, L0.mask,
                            lat_steps, c1, c2, 0, L0.sidm_for == (const void*)L0.A->dict ? L0.sidm.p : nullptr);
      } else {
        launch_cheb_step(s, *L0.A, nv, L0.xa.p, L0.r.p, L0.dinv.p, L0.d.p, 0.3, 0.7, L0.xb.p, L0.mask);
      }
    };
    // In the solver this launch follows other kernels that have streamed hundreds of MB; the
    // operator (145 MB at n = 512) would otherwise sit in the 256 MB Infinity Cache between
    // back-to-back repetitions.  Timed: `reps` pairs (flush, step) minus `reps` flushes, the
    // flush being a product with the 2x2-block Jacobian array (0.47 GB streamed, larger than the
    // cache, so its own time does not depend on what ran before).
    DevBuf<double> fx, fy;
    fx.alloc((size_t)nvel(ctx));
    fy.alloc((size_t)nvel(ctx));
    fx.zero(s);
    auto flush = [&] { launch_spmv(s, ctx->J, 1, fx.p, fy.p, nullptr, MASK_NONE); };
    double ms;
    if (warm) {
      ms = time_rounds(s, reps, nothing, step);
    } else {
      const double t_both = time_rounds(s, reps, flush, step), t_flush = time_rounds(s, reps, flush, nothing);
      ms = t_both - t_flush;
    }
    *ms_per_launch = (double)ms / reps;
    (void)p;
    if (algorithmic_bytes)
      *algorithmic_bytes = lattice ? lattice_launch_bytes(*L0.A, nv, false, false, false, false)
                                   : smoother_launch_bytes(*L0.A, nv, false);
    return NSFEM_OK;
  }
  int nv;
  const BlockMat* A = get_op(ctx, op, &nv);
  const Pattern& p = *A->pat;
  // scalar P2 operators act on all velocity components in the solver
  const int nvv = (op == NSFEM_OP_MASS_P2 || op == NSFEM_OP_STIFF_P2) ? ctx->mesh.dim : 1;
  const size_t nx = (size_t)p.n_cols * A->bc * nvv, ny = (size_t)p.n_rows * A->br * nvv;
  DevBuf<double> dx, dy;
  dx.alloc(nx);
  dy.alloc(ny);
  hipStream_t s = ctx->stream;
  std::vector<double> hx(nx);
  for (size_t i = 0; i < nx; ++i) hx[i] = std::sin((double)i);
  NSFEM_HIP(hipMemcpyAsync(dx.p, hx.data(), sizeof(double) * nx, hipMemcpyHostToDevice, s));
  const double ms = time_rounds(s, reps, nothing, [&] { launch_spmv(s, *A, nvv, dx.p, dy.p, nullptr, MASK_NONE); });
  *ms_per_launch = ms / reps;
  if (algorithmic_bytes)
    *algorithmic_bytes = (int64_t)p.nnz * (8 * A->br * A->bc + 4) + (int64_t)(p.n_rows + 1) * 4 +
                         (int64_t)(nx + ny) * 8;
  API_END(ctx)
}
