// Geometric multigrid on gfx950 (K8-K13 of SURVEY 2.1; a15-a18 of SURVEY 8).
// Replaces the PETSc PCMG wiring of
//   src/08_algebra.../03_solvers_with_preconditioner/LinearEquationSolverPetsc.cpp:185-353 (MGInit/MGSetLevel/MGSolve)
// with the cycle the reference states itself in LinearImplicitSystem::MGStep (LinearImplicitSystem.cpp:1397-1562):
//   pre-smooth -> residual -> restrict (R = PP^T, LinearImplicitSystem.cpp:379-382) -> recurse -> prolong+add -> post-smooth.
// PETSc behaviours restated: multiplicative V-cycle, smoother = KSPRICHARDSON(scale omega) + PCJACOBI
// with a FIXED iteration count and zero initial guess on the way down (first sweep needs no SpMV), level 0 = exact solve
// (PREONLY + LU, LinearEquationSolverPetsc.hpp:131-134), outer KSP = PREONLY / RICHARDSON(0.99999) / left-preconditioned
// GMRES(restart) with classical Gram-Schmidt and Knoll initial guess (:294-335) / PCG.
//
// MI355X design: every smoother sweep is ONE fused CSR-stream SpMV (matrix read once, x_new = x + omega*dinv*(b - A x));
// restriction uses the explicit transpose (built once) so it is a plain coalesced SpMV; the exact solve of level 0 is
// fh_coarse.hip's (a dense GEMV with the inverse factored once per assembly, or its block / sparse forms); the whole cycle (~25 short launches, launch-bound on the coarse
// levels) is captured in a hipGraph and replayed.
#include "fh_coarse.h"
#include "fh_krylov.h"
#include "fh_patch.h"
#include "fh_spmv.h"
#include "fh_trisolve.h"
#include <algorithm>
#include <memory>
#include <cmath>

struct MgLevel {
  fh_mat_t A = nullptr, P = nullptr, R = nullptr;
  bool R_given = false;      // restriction handed in by the caller; otherwise R = the cached explicit transpose of P, refreshed at every setup
  uint64_t A_uid = 0;        // the matrix the colourings below were built for (pattern caches: dropped when another matrix is installed)
  int n = 0, smoother = 0, npre = 2, npost = 2;
  double omega = 2.0 / 3.0;
  double *dinv = nullptr, *x = nullptr, *x2 = nullptr, *b = nullptr, *r = nullptr;
  // multicolour Gauss-Seidel (SOR) smoother: rows grouped by colour of the matrix graph
  int ncolors = 0;
  std::vector<int> color_ptr;
  int* d_color_rows = nullptr;
  // natural-order sweeps (FH_SMOOTH_SOR, FH_SMOOTH_ILU0): level schedules of the matrix graph, ILU(0) factors
  fh_tri_t tri = nullptr;
  // block Schwarz smoothers (FH_SMOOTH_VANKA, FH_SMOOTH_ASM): dof patches, their colours and dense inverses (fh_patch.hip); null until patches are set
  PatchSmoother* patch = nullptr;
  // distributed level: operator = owned rows over [owned | ghost] columns; halo refreshes the ghosts
  fh_halo_t halo = nullptr;
  bool replicated_below = false;
  int ncols = 0;
  int buf_n = -1;            // size the work vectors were allocated for (kept across preparations)
  double* buf_base = nullptr;   // dinv, x, x2, b, r: one allocation
  // FH_SMOOTH_LU: B = A^-1 by the sparse exact solve (fh_direct.hip); coordinates of the level's unknowns let it cut at coordinate layers
  fh_direct_t direct = nullptr;
  uint64_t direct_uid = 0;
  std::vector<double> xyz;
  int xyz_dim = 0;
  // level solver: 0 = Richardson(omega) around the sweep preconditioner, 1 = GMRES (fixed iteration count, left-preconditioned)
  int solver = 0, gm_restart = 30;
  LevelGmres gm;             // workspace of the GMRES level solver (fh_krylov.hip)
};

struct fh_mg_s {
  fh_ctx_t ctx = nullptr;
  int nlevels = 0;
  std::vector<MgLevel> lv;
  CoarseSolve* coarse = nullptr;      // the exact solve of level 0 and all its state (fh_coarse.hip)
  int cycle_type = 0;                 // FH_CYCLE_*: PCMGSetType
  bool capturable = true;             // no distributed level: the cycle is replayed from a captured graph
  bool setup_done = false;
  hipGraph_t graph = nullptr;
  hipGraphExec_t gexec = nullptr;
  uint64_t graph_sig = 0;     // what the captured cycle was recorded for (every pointer, size and option a launch of the cycle carries)
  KrylovWork krylov;          // workspace of the outer solvers (fh_krylov.hip)
  int64_t cycle_bytes = 0;
};

// ------------------------------------------------------------------------------------------------
// small kernels
// ------------------------------------------------------------------------------------------------
// sweep 1 from a zero guess; on a distributed level the interface entries go straight into the send buffer of the exchange that
// follows (the pack kernel fused into the sweep: nsend > 0)
__global__ __launch_bounds__(256) void k_first_sweep(double* __restrict__ x, const double* __restrict__ b, const double* __restrict__ dinv,
                                                     double omega, int n, const int* __restrict__ send_idx, double* __restrict__ sendbuf, int nsend) {
  for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) x[i] = omega * dinv[i] * b[i];
  for (int k = blockIdx.x * 256 + threadIdx.x; k < nsend; k += gridDim.x * 256) {
    const int i = send_idx[k];
    sendbuf[k] = omega * dinv[i] * b[i];
  }
}

// one colour of a Gauss-Seidel sweep on A z = r: z_i = dinv_i (r_i - sum_{j != i} a_ij z_j) for the rows of the colour
// (rows of one colour are mutually uncoupled, so the in-place update is race-free); 16 lanes per row
__global__ __launch_bounds__(256) void k_gs_color(const int* __restrict__ rows, int nrows, const int* __restrict__ rowptr, const int* __restrict__ col,
                                                  const double* __restrict__ val, const double* __restrict__ dinv, const double* __restrict__ r,
                                                  double* z) {
  const int rr = (blockIdx.x * 256 + threadIdx.x) >> 4;
  const int gl = threadIdx.x & 15;
  const bool live = rr < nrows;
  const int i = live ? rows[rr] : 0;
  double acc = 0.0;
  if (live)
    for (int k = rowptr[i] + gl; k < rowptr[i + 1]; k += 16) {
      const int j = col[k];
      if (j != i) acc += val[k] * z[j];
    }
#pragma unroll
  for (int off = 8; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
  if (live && gl == 0) z[i] = dinv[i] * (r[i] - acc);
}

static inline int halo_spmv(fh_halo_t h, fh_mat_t A, double* x, int n_own, double* y, int mode, const double* b, const double* dinv, double omega,
                            bool prepacked = false) {
  return fh_dev_halo_spmv(h, A, x, n_own, y, mode, b, dinv, omega, prepacked);
}

// ------------------------------------------------------------------------------------------------
// API
// ------------------------------------------------------------------------------------------------
static void free_level_colors(MgLevel& L);
extern "C" int fh_mg_create(fh_ctx_t ctx, int nlevels, fh_mg_t* out) {
  FH_REQUIRE(ctx && out && nlevels >= 1, "fh_mg_create: bad arguments");
  fh_mg_t mg = new fh_mg_s();
  mg->ctx = ctx;
  mg->nlevels = nlevels;
  mg->lv.resize(nlevels);
  mg->coarse = fh_coarse_create(ctx);
  *out = mg;
  return 0;
}

extern "C" int fh_mg_set_level(fh_mg_t mg, int level, fh_mat_t A, fh_mat_t P, fh_mat_t R, int smoother, double omega, int npre, int npost) {
  FH_REQUIRE(mg && A, "fh_mg_set_level: null argument");
  FH_REQUIRE(level >= 0 && level < mg->nlevels, "fh_mg_set_level: level %d out of range", level);
  FH_REQUIRE(A->m <= A->n, "fh_mg_set_level: operator must be square (or owned rows x local columns on a distributed level)");
  FH_REQUIRE(level == 0 || P != nullptr, "fh_mg_set_level: level %d needs an interpolation matrix", level);
  FH_REQUIRE(!P || P->m == A->m, "fh_mg_set_level: interpolation has %d rows, operator has %d", P ? P->m : 0, A->m);
  FH_REQUIRE(smoother >= FH_SMOOTH_JACOBI && smoother <= FH_SMOOTH_ASM,
             "fh_mg_set_level: unknown smoother %d (0 = Richardson+Jacobi, 1 = Richardson+multicolour SOR, 2 = block Schwarz / Vanka, "
             "3 = Richardson+SOR in natural order, 4 = Richardson+ILU(0), 5 = no preconditioner, 6 = exact solve, 7 = PCASM basic / multiplicative with ILU(0) blocks)", smoother);
  FH_REQUIRE(npre >= 0 && npost >= 0, "fh_mg_set_level: negative sweep count");
  MgLevel& L = mg->lv[level];
  if (L.A_uid != A->uid) {   // another matrix (also one that landed on the address of a destroyed one): its graph may differ
    free_level_colors(L);
    fh_patch_drop_setup(L.patch);
    fh_tri_destroy(L.tri);
    L.tri = nullptr;
    L.A_uid = A->uid;
  }
  L.A = A;
  L.P = P;
  L.R = R;
  L.R_given = R != nullptr;
  L.n = A->m;
  L.ncols = A->n;
  L.smoother = smoother;
  L.omega = omega;
  L.npre = npre;
  L.npost = npost;
  mg->setup_done = false;
  return 0;
}

static int capture_cycle(fh_mg_t mg);
extern "C" int fh_mg_set_cycle_type(fh_mg_t mg, int type) {
  FH_REQUIRE(mg, "fh_mg_set_cycle_type: null argument");
  FH_REQUIRE(type >= FH_CYCLE_MULTIPLICATIVE && type <= FH_CYCLE_KASKADE, "fh_mg_set_cycle_type: unknown type %d (0 multiplicative, 1 full, 2 additive, 3 kaskade)", type);
  const bool changed = mg->cycle_type != type;
  mg->cycle_type = type;
  if (changed && mg->setup_done) FH_TRY(capture_cycle(mg));      // the captured launch sequence is the old type's
  return 0;
}

extern "C" int fh_mg_set_level_solver(fh_mg_t mg, int level, int solver, int restart) {
  FH_REQUIRE(mg && level >= 0 && level < mg->nlevels, "fh_mg_set_level_solver: bad level %d", level);
  FH_REQUIRE(solver == FH_LEVEL_RICHARDSON || solver == FH_LEVEL_GMRES, "fh_mg_set_level_solver: unknown level solver %d", solver);
  FH_REQUIRE(restart >= 1, "fh_mg_set_level_solver: restart must be positive");
  mg->lv[level].solver = solver;
  mg->lv[level].gm_restart = restart;
  mg->setup_done = false;
  return 0;
}

extern "C" int fh_mg_set_level_distributed(fh_mg_t mg, int level, fh_halo_t halo, int replicated_below) {
  FH_REQUIRE(mg && level >= 0 && level < mg->nlevels, "fh_mg_set_level_distributed: bad level");
  mg->lv[level].halo = halo;
  mg->lv[level].replicated_below = replicated_below != 0;
  mg->setup_done = false;
  return 0;
}

static void free_level_buffers(MgLevel& L) {
  if (L.buf_base) hipFree(L.buf_base);         // the five work vectors of the level are one allocation (one fill per preparation)
  L.buf_base = nullptr;
  for (double** p : {&L.dinv, &L.x, &L.x2, &L.b, &L.r}) *p = nullptr;
  L.gm.release();
  L.buf_n = -1;
}

// everything a launch of the captured cycle carries: a repeated preparation of the same hierarchy (MGsolve prepares before every
// solve, LinearImplicitSystem.cpp:347-383) finds the same pointers, sizes and options and replays the graph it already has
static uint64_t cycle_signature(fh_mg_t mg) {
  uint64_t h = 1469598103934665603ull;
  auto mix = [&](uint64_t v) {
    for (int k = 0; k < 8; k++) {
      h ^= (v >> (8 * k)) & 0xff;
      h *= 1099511628211ull;
    }
  };
  auto mixp = [&](const void* p) { mix((uint64_t)(uintptr_t)p); };
  auto mixm = [&](fh_mat_t M) {
    mixp(M);
    if (M) {
      mix(M->uid);
      mixp(M->d_val);
      std::vector<uint64_t> sw;
      fh_spmv_signature(M, sw);
      for (uint64_t w : sw) mix(w);
    }
  };
  mix((uint64_t)mg->nlevels);
  mix((uint64_t)mg->cycle_type);
  mix((uint64_t)mg->ctx->opt_gen);
  std::vector<uint64_t> cw;
  fh_coarse_signature(mg->coarse, cw);
  for (int l = 0; l < mg->nlevels; l++) fh_patch_signature(mg->lv[l].patch, cw);
  for (uint64_t w : cw) mix(w);
  for (int l = 0; l < mg->nlevels; l++) {
    MgLevel& L = mg->lv[l];
    mixm(L.A);
    mixm(L.P);
    mixm(L.R);
    mix((uint64_t)L.smoother);
    mix((uint64_t)L.npre);
    mix((uint64_t)L.npost);
    uint64_t ob;
    memcpy(&ob, &L.omega, 8);
    mix(ob);
    mix((uint64_t)L.n);
    mix((uint64_t)L.ncols);
    for (double* p : {L.dinv, L.x, L.x2, L.b, L.r}) mixp(p);
    mixp(L.direct);
    mix(fh_direct_generation(L.direct));
    mixp(L.tri);
    mixp(L.d_color_rows);
    mix((uint64_t)L.ncolors);
    mixp(L.halo);
    mix((uint64_t)L.solver);
    mix((uint64_t)L.gm_restart);
    mixp(L.gm.basis);
  }
  return h ? h : 1;
}

static void free_level_colors(MgLevel& L) {
  if (L.d_color_rows) hipFree(L.d_color_rows);
  L.d_color_rows = nullptr;
  L.ncolors = 0;
}

extern "C" int fh_mg_set_level_patches(fh_mg_t mg, int level, int npatch, const int* ptr, const int* dofs) {
  FH_REQUIRE(mg && level >= 0 && level < mg->nlevels && npatch > 0 && ptr && dofs, "fh_mg_set_level_patches: bad arguments");
  FH_TRY(fh_patch_set(&mg->lv[level].patch, npatch, ptr, dofs));
  mg->setup_done = false;
  return 0;
}

extern "C" int fh_mg_set_level_patches_exact(fh_mg_t mg, int level, int nfirst) {
  FH_REQUIRE(mg && level >= 0 && level < mg->nlevels, "fh_mg_set_level_patches_exact: bad arguments");
  FH_TRY(fh_patch_set_exact(mg->lv[level].patch, nfirst));
  mg->setup_done = false;
  return 0;
}

static int run_cycle(fh_mg_t mg);

// greedy colouring of the matrix graph (host, integer setup work): coupled rows get different colours.  "Coupled" is symmetric: row i
// reading x_j keeps j out of i's colour whether or not row j reads x_i (an unsymmetric pattern -- a convection term, a one-sided
// constraint -- would otherwise let i and j share a colour, and row i would race with row j's update)
static int color_rows(MgLevel& L) {
  fh_mat_t A = L.A;
  const int m = A->m;
  std::vector<int> tptr(m + 1, 0);
  for (int i = 0; i < m; i++)
    for (int k = A->h_rowptr[i]; k < A->h_rowptr[i + 1]; k++) {
      const int j = fh_hcol(A)[k];
      if (j < m && j != i) tptr[j + 1]++;
    }
  for (int i = 0; i < m; i++) tptr[i + 1] += tptr[i];
  std::vector<int> trow(tptr[m]), tpos(tptr.begin(), tptr.end() - 1);
  for (int i = 0; i < m; i++)
    for (int k = A->h_rowptr[i]; k < A->h_rowptr[i + 1]; k++) {
      const int j = fh_hcol(A)[k];
      if (j < m && j != i) trow[tpos[j]++] = i;      // row i reads column j
    }
  std::vector<int> color(m, -1), mark;
  int nc = 0;
  for (int i = 0; i < m; i++) {
    mark.assign(nc + 1, 0);
    for (int k = A->h_rowptr[i]; k < A->h_rowptr[i + 1]; k++) {
      const int j = fh_hcol(A)[k];
      if (j < m && j != i && color[j] >= 0) mark[color[j]] = 1;
    }
    for (int k = tptr[i]; k < tptr[i + 1]; k++)
      if (color[trow[k]] >= 0) mark[color[trow[k]]] = 1;
    int c = 0;
    while (c < nc && mark[c]) c++;
    color[i] = c;
    nc = std::max(nc, c + 1);
  }
  L.color_ptr.assign(nc + 1, 0);
  for (int i = 0; i < m; i++) L.color_ptr[color[i] + 1]++;
  for (int c = 0; c < nc; c++) L.color_ptr[c + 1] += L.color_ptr[c];
  std::vector<int> rows(m), pos(L.color_ptr.begin(), L.color_ptr.end() - 1);
  for (int i = 0; i < m; i++) rows[pos[color[i]]++] = i;
  FH_CHECK_HIP(hipMalloc(&L.d_color_rows, std::max(m, 1) * sizeof(int)));
  FH_CHECK_HIP(hipMemcpy(L.d_color_rows, rows.data(), (size_t)m * sizeof(int), hipMemcpyHostToDevice));
  L.ncolors = nc;
  return 0;
}

// (re)capture of the cycle: un-captured warm-up run, then one cycle recorded on the internal buffers and kept for replay
static int capture_cycle(fh_mg_t mg) {
  fh_ctx_t c = mg->ctx;
  if (mg->gexec) {
    hipGraphExecDestroy(mg->gexec);
    mg->gexec = nullptr;
  }
  if (mg->graph) {
    hipGraphDestroy(mg->graph);
    mg->graph = nullptr;
  }
  mg->graph_sig = 0;
  FH_TRY(run_cycle(mg));   // un-captured warm-up: builds lazily created row blocks, validates the launches
  FH_CHECK_HIP(hipStreamSynchronize(c->stream));
  FH_TRACE("capture_cycle: warm-up cycle done");
  // distributed cycles are NOT captured: stream capture of the grouped ncclSend/ncclRecv (forked communication stream) was tried on
  // this stack (RCCL 2.26.6 of the PyTorch wheel, one-rank self exchange) and segfaults inside the library at capture time; the
  // launches of a distributed cycle are issued one by one
  if (c->use_graph && mg->capturable) {
    FH_CHECK_HIP(hipStreamBeginCapture(c->stream, hipStreamCaptureModeThreadLocal));
    int rc = run_cycle(mg);
    hipError_t e = hipStreamEndCapture(c->stream, &mg->graph);
    if (rc) return rc;
    FH_CHECK_HIP(e);
    FH_CHECK_HIP(hipGraphInstantiate(&mg->gexec, mg->graph, nullptr, nullptr, 0));
    mg->graph_sig = cycle_signature(mg);      // after the warm-up: lazily built row blocks exist now
  }
  return 0;
}

extern "C" int fh_mg_setup(fh_mg_t mg) {
  FH_GUARD_BEGIN
  fh_ctx_t c = mg->ctx;
  for (int l = 0; l < mg->nlevels; l++) FH_REQUIRE(mg->lv[l].A, "fh_mg_setup: level %d has not been set", l);
  bool distributed = false;
  for (int l = 0; l < mg->nlevels; l++) {
    MgLevel& L = mg->lv[l];
    distributed |= (L.halo != nullptr);
    FH_REQUIRE(L.halo || L.A->m == L.A->n, "fh_mg_setup: level %d is not square and has no halo", l);
    FH_REQUIRE(!L.halo || L.R || l == 0, "fh_mg_setup: distributed level %d needs an explicit restriction matrix", l);
  }
  for (int l = 1; l < mg->nlevels; l++)
    FH_REQUIRE(mg->lv[l].P->n == mg->lv[l - 1].ncols, "fh_mg_setup: interpolation of level %d has %d columns, level %d has %d local entries", l,
               mg->lv[l].P->n, l - 1, mg->lv[l - 1].ncols);
  mg->cycle_bytes = 0;
  for (int l = 0; l < mg->nlevels; l++) {
    MgLevel& L = mg->lv[l];
    const size_t nb = ((size_t)L.ncols + 2) * sizeof(double);
    const size_t nbd = ((size_t)L.ncols + 2 + 1) & ~(size_t)1;      // doubles per vector, even: every vector stays 16-byte aligned
    if (L.buf_n != L.ncols) {      // a repeated preparation keeps its work vectors (and with them the captured cycle)
      free_level_buffers(L);
      FH_CHECK_HIP(hipMalloc(&L.buf_base, 5 * nbd * sizeof(double)));
      int slot = 0;
      for (double** p : {&L.dinv, &L.x, &L.x2, &L.b, &L.r}) *p = L.buf_base + (size_t)(slot++) * nbd;
      L.buf_n = L.ncols;
    }
    if (c->debug_poison) {
      for (double** p : {&L.dinv, &L.x, &L.x2, &L.b, &L.r}) {
        if (p != &L.dinv) FH_CHECK_HIP(hipMemsetAsync(*p, 0xFF, nb, c->stream));
        else hipLaunchKernelGGL(k_fill_value, dim3(sgrid(c, L.ncols + 2)), dim3(256), 0, c->stream, *p, 0.0, L.ncols + 2);
      }
    } else {      // zeroed by ONE fill kernel: the runtime's memset reaches 0.6 TB/s (five vectors of the finest level: 0.14 ms), five launches cost 20 us per level
      FH_REQUIRE(5 * nbd < ((size_t)1 << 31), "fh_mg_setup: level %d is too large for the 32-bit fill", l);
      hipLaunchKernelGGL(k_fill_value, dim3(sgrid(c, (int)std::min<size_t>(5 * nbd, (size_t)1 << 30))), dim3(256), 0, c->stream, L.buf_base, 0.0, (int)(5 * nbd));
    }
    FH_TRY(fh_dev_get_diag(L.A, L.dinv, 1));
    if (l > 0 && L.smoother == FH_SMOOTH_IDENTITY)      // PCNONE: B = I, the Jacobi kernels with a unit "inverse diagonal"
      hipLaunchKernelGGL(k_fill_value, dim3(sgrid(c, L.n)), dim3(256), 0, c->stream, L.dinv, 1.0, L.n);
    if (l > 0 && L.solver == FH_LEVEL_GMRES) FH_TRY(L.gm.reserve(std::max(1, std::min(std::max(L.npre, L.npost), L.gm_restart)), L.ncols, L.n, c));
    else L.gm.release();
    if (L.smoother == FH_SMOOTH_GS_COLOR && l > 0 && L.ncolors == 0) FH_TRY(color_rows(L));
    if ((L.smoother == FH_SMOOTH_SOR || L.smoother == FH_SMOOTH_ILU0) && l > 0) {
      if (!L.tri) FH_TRY(fh_tri_create(L.A, &L.tri));                       // level schedules: once per pattern
      if (L.smoother == FH_SMOOTH_ILU0) FH_TRY(fh_tri_ilu_factor(L.tri, L.A));   // numeric factorisation: every setup
    }
    if (L.smoother == FH_SMOOTH_LU && l > 0) {
      FH_REQUIRE(!L.halo, "fh_mg_setup: level %d: the exact solve as level preconditioner serves undistributed levels", l);
      if (!L.direct || L.direct_uid != L.A->uid) {
        if (L.direct) fh_direct_destroy(L.direct);
        L.direct = nullptr;
        const bool have_xyz = L.xyz_dim >= 1 && (int)L.xyz.size() == L.n * L.xyz_dim;
        FH_TRY(fh_direct_create(c, L.A, have_xyz ? L.xyz_dim : 0, have_xyz ? L.xyz.data() : nullptr, 0, &L.direct));
        L.direct_uid = L.A->uid;
      }
      FH_TRY(fh_direct_factor(L.direct));
    }
    if ((L.smoother == FH_SMOOTH_VANKA || L.smoother == FH_SMOOTH_ASM) && l > 0) {
      FH_REQUIRE(fh_patch_count(L.patch) > 0 && !L.halo, "fh_mg_setup: level %d uses the block smoother but has no patches (fh_mg_set_level_patches)", l);
      FH_TRY(fh_patch_setup(L.patch, c, L.A, L.smoother == FH_SMOOTH_ASM ? 1 : 0));
    }
    if (l > 0) {
      if (!L.R_given) {
        // restriction = transpose of the interpolation (LinearImplicitSystem.cpp:379-382): P's cached explicit transpose, whose
        // values are re-gathered here whenever P was edited since (zero_rows / zero_cols / new values clear its validity flag)
        FH_TRY(fh_mat_refresh_transpose(L.P));
        L.R = L.P->At;
      }
      FH_REQUIRE(L.R->m == mg->lv[l - 1].n && (L.R->n == L.n || L.R->n == L.ncols), "fh_mg_setup: restriction of level %d has the wrong shape", l);
      const int64_t bA = fh_spmv_algorithmic_bytes(L.A), n8 = 8ll * L.n;
      // algorithmic bytes of the cycle on this level (SURVEY 8d model, zero-guess first sweep needs no SpMV):
      if (L.npre > 0) mg->cycle_bytes += 3 * n8 + (int64_t)(L.npre - 1) * (bA + 2 * n8);
      mg->cycle_bytes += bA + n8;                                            // residual
      mg->cycle_bytes += fh_spmv_algorithmic_bytes(L.R) + fh_spmv_algorithmic_bytes(L.P) + n8;   // restrict, prolong+add
      mg->cycle_bytes += (int64_t)L.npost * (bA + 2 * n8);
    }
  }
  FH_TRACE("fh_mg_setup: levels set up");
  FH_TRY(fh_coarse_factor(mg->coarse, mg->lv[0].A));
  FH_TRACE("fh_mg_setup: coarse level factored");
  mg->cycle_bytes += 8ll * mg->lv[0].n * mg->lv[0].n + 16ll * mg->lv[0].n;
  mg->setup_done = true;
  mg->capturable = !distributed;
  const uint64_t sig = cycle_signature(mg);
  if (mg->gexec && mg->graph_sig == sig && c->use_graph && mg->capturable && c->mg_reuse_graph) return 0;   // same launches: the graph stays
  FH_TRY(capture_cycle(mg));
  return 0;
  FH_GUARD_END("fh_mg_setup")
}

// z = B r: forward then backward Gauss-Seidel from a zero guess over the colours of the matrix graph
static int gs_color_apply(fh_mg_t mg, MgLevel& L, const double* r, double* z) {
  fh_ctx_t c = mg->ctx;
  FH_CHECK_HIP(hipMemsetAsync(z, 0, (size_t)L.ncols * sizeof(double), c->stream));
  for (int pass = 0; pass < 2; pass++)
    for (int k = 0; k < L.ncolors; k++) {
      const int col = pass == 0 ? k : L.ncolors - 1 - k;
      const int nr = L.color_ptr[col + 1] - L.color_ptr[col];
      if (nr == 0) continue;
      hipLaunchKernelGGL(k_gs_color, dim3(fh_div_up((int64_t)nr * 16, 256)), dim3(256), 0, c->stream, L.d_color_rows + L.color_ptr[col], nr,
                         L.A->d_rowptr, L.A->d_col, L.A->d_val, L.dinv, r, z);
    }
  FH_CHECK_HIP(hipGetLastError());
  return 0;
}

__global__ __launch_bounds__(256) void k_scale_by(double* __restrict__ z, const double* __restrict__ r, const double* __restrict__ dinv, int n) {
  for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) z[i] = dinv[i] * r[i];
}

// z = B r with the level's sweep preconditioner: forward then backward Gauss-Seidel from a zero guess (PCSOR's local symmetric sweep,
// PetscPreconditioner.cpp:219-222) over the colours (FH_SMOOTH_GS_COLOR) or in the natural row order as PETSc runs it (FH_SMOOTH_SOR, level-scheduled,
// fh_trisolve.hip), the ILU(0) solve (FH_SMOOTH_ILU0, PetscPreconditioner.cpp:91-115), A^-1 r (FH_SMOOTH_LU), one block sweep from zero, else the
// diagonal.  rwork: a vector that is neither r nor z, the residual inside the unfused block sweep (unused by every other smoother)
static int level_precond(fh_mg_t mg, MgLevel& L, const double* r, double* z, double* rwork) {
  fh_ctx_t c = mg->ctx;
  switch (L.smoother) {
    case FH_SMOOTH_SOR: return fh_tri_ssor_apply(L.tri, L.A, L.dinv, r, z);
    case FH_SMOOTH_ILU0: return fh_tri_ilu_apply(L.tri, L.A, r, z);
    case FH_SMOOTH_LU: return fh_direct_solve_ptr(L.direct, r, z);
    case FH_SMOOTH_GS_COLOR: return gs_color_apply(mg, L, r, z);
    case FH_SMOOTH_VANKA:
    case FH_SMOOTH_ASM:           // PCApply_ASM: the blocks in order on the residual of r with the corrections so far, from zero
      FH_CHECK_HIP(hipMemsetAsync(z, 0, (size_t)L.ncols * sizeof(double), c->stream));
      return fh_patch_apply(L.patch, c, L.A, z, r, rwork, 1.0, 1);
    default:
      hipLaunchKernelGGL(k_scale_by, dim3(sgrid(c, L.n)), dim3(256), 0, c->stream, z, r, L.dinv, L.n);
      return 0;
  }
}

// Richardson(scale omega) around the sweep preconditioner: x <- x + omega * B (b - A x), z = B r in x2.  The work vector of the block sweep is
// dinv here (x2 is taken, and FH_SMOOTH_ASM, the one block smoother that comes this way, does not read the inverse diagonal)
static int gs_sweeps(fh_mg_t mg, MgLevel& L, int nsweeps, bool zero_guess) {
  fh_ctx_t c = mg->ctx;
  for (int s = 0; s < nsweeps; s++) {
    const bool first = zero_guess && s == 0;
    if (first) {
      FH_CHECK_HIP(hipMemcpyAsync(L.r, L.b, (size_t)L.n * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
    } else {
      FH_TRY(halo_spmv(L.halo, L.A, L.x, L.n, L.r, 2, L.b, nullptr, 0.0));
    }
    FH_TRY(level_precond(mg, L, L.r, L.x2, L.dinv));
    hipLaunchKernelGGL(k_axpby2, dim3(sgrid(c, L.n)), dim3(256), 0, c->stream, L.x, L.x2, L.omega, first ? 0.0 : 1.0, L.n);
  }
  FH_CHECK_HIP(hipGetLastError());
  return 0;
}

// the level as a Krylov solver sees it: operator with ghost refresh, sum over the ranks, sweep preconditioner
static KrylovOps level_ops(fh_mg_t mg, MgLevel& L) {
  KrylovOps op;
  op.ctx = mg->ctx;
  op.n = L.n;
  op.ncols = L.ncols;
  op.spmv = [&L](double* x, double* y, int mode, const double* b) { return halo_spmv(L.halo, L.A, x, L.n, y, mode, b, nullptr, 0.0); };
  op.allreduce = [&L](double* d, int count) { return L.halo ? fh_halo_allreduce_ptr(L.halo, d, count) : 0; };
  op.precond = [mg, &L](const double* in, double* out) { return level_precond(mg, L, in, out, L.x2); };
  return op;
}


// one multiplicative V-cycle on the internal buffers: input lv[top].b, output lv[top].x
// distributed levels: ghosts of the operand are refreshed before every operator application (MPIAIJ MatMult semantics)
// npre / npost iterations of a level's smoother on L.x for the right-hand side L.b; zero_guess: L.x is taken as zero (sweep 1 of the
// Richardson/Jacobi smoother is then the diagonal scaling PETSc's Richardson does from a zero guess).  *packed: the send buffer of the level's
// exchange already holds the interface entries of L.x (the first sweep writes them).
static int smooth_level(fh_mg_t mg, MgLevel& L, int nits, bool zero_guess, bool* packed) {
  fh_ctx_t c = mg->ctx;
  *packed = false;
  if (nits == 0) {
    if (zero_guess) FH_CHECK_HIP(hipMemsetAsync(L.x, 0, (size_t)L.ncols * sizeof(double), c->stream));
    return 0;
  }
  if (L.solver == FH_LEVEL_GMRES) return fh_gmres_smooth(L.gm, level_ops(mg, L), L.x, L.b, L.r, nits, zero_guess);
  if (L.smoother == FH_SMOOTH_VANKA) {
    if (zero_guess) FH_CHECK_HIP(hipMemsetAsync(L.x, 0, (size_t)L.ncols * sizeof(double), c->stream));
    return fh_patch_apply(L.patch, c, L.A, L.x, L.b, L.r, L.omega, nits);
  }
  if (L.smoother == FH_SMOOTH_GS_COLOR || L.smoother == FH_SMOOTH_SOR || L.smoother == FH_SMOOTH_ILU0 || L.smoother == FH_SMOOTH_LU ||
      L.smoother == FH_SMOOTH_ASM)
    return gs_sweeps(mg, L, nits, zero_guess);
  int s = 0;
  if (zero_guess) {
    // sweep 1 from a zero guess: x = omega D^-1 b ; the others: fused Jacobi SpMV, ping-pong x <-> x2
    const int* sidx = nullptr;
    double* sbuf = nullptr;
    int nsend = 0;
    if (L.halo) fh_halo_send_plan(L.halo, &sidx, &sbuf, &nsend);
    hipLaunchKernelGGL(k_first_sweep, dim3(sgrid(c, L.n)), dim3(256), 0, c->stream, L.x, L.b, L.dinv, L.omega, L.n, sidx, sbuf, nsend);
    *packed = L.halo != nullptr;             // the exchange of this x needs no pack launch
    s = 1;
  }
  for (; s < nits; s++) {
    FH_TRY(halo_spmv(L.halo, L.A, L.x, L.n, L.x2, 3, L.b, L.dinv, L.omega, *packed));
    *packed = false;
    std::swap(L.x, L.x2);
  }
  return 0;
}


// the exact solve of level 0: x = A_0^-1 b
static int coarse_solve(fh_mg_t mg) {
  MgLevel& L0 = mg->lv[0];
  return fh_coarse_solve(mg->coarse, L0.b, L0.x, L0.r, L0.dinv);
}

// b_{l-1} = R v on level l (v = the level's residual, or its right-hand side): the restriction reads ghost entries, except into a replicated
// level (owned part, then all-reduce)
static int restrict_into(fh_mg_t mg, int l, double* v) {
  MgLevel& L = mg->lv[l];
  FH_TRY(halo_spmv(L.replicated_below ? nullptr : L.halo, L.R, v, L.n, mg->lv[l - 1].b, 0, nullptr, nullptr, 0.0));
  if (L.halo && L.replicated_below) FH_TRY(fh_halo_allreduce_ptr(L.halo, mg->lv[l - 1].b, mg->lv[l - 1].n));
  return 0;
}

// PCMGMCycle_Private from level `from` down (PC_MG_MULTIPLICATIVE with one cycle per level): x_from starts at zero (zero_guess) or holds a guess
static int mcycle(fh_mg_t mg, int from, bool zero_guess) {
  if (from == 0) return coarse_solve(mg);
  for (int l = from; l >= 1; l--) {
    MgLevel& L = mg->lv[l];
    bool packed = false;
    FH_TRY(smooth_level(mg, L, L.npre, zero_guess || l < from, &packed));
    FH_TRY(halo_spmv(L.halo, L.A, L.x, L.n, L.r, 2, L.b, nullptr, 0.0, packed));     // r = b - A x (ghosts of x refreshed)
    FH_TRY(restrict_into(mg, l, L.r));
  }
  FH_TRY(coarse_solve(mg));
  for (int l = 1; l <= from; l++) {
    MgLevel& L = mg->lv[l];
    MgLevel& Lc = mg->lv[l - 1];
    FH_TRY(halo_spmv(Lc.halo, L.P, Lc.x, Lc.n, L.x, 1, nullptr, nullptr, 0.0));      // x += P x_{l-1} (reads ghost coarse values)
    bool packed = false;
    FH_TRY(smooth_level(mg, L, L.npost, false, &packed));
  }
  return 0;
}

// one application of the multigrid preconditioner to lv[top].b -> lv[top].x, PCMG's four forms (PCMGSetType, LinearEquationSolverPetsc.cpp:199-214;
// PETSc mg.c / fmg.c: PCMGMCycle_Private, PCMGACycle_Private, PCMGFCycle_Private, PCMGKCycle_Private)
static int run_cycle(fh_mg_t mg) {
  const int top = mg->nlevels - 1;
  if (mg->cycle_type == FH_CYCLE_MULTIPLICATIVE) {
    FH_TRY(mcycle(mg, top, true));
    FH_CHECK_HIP(hipGetLastError());
    return 0;
  }
  // the other three restrict the RIGHT-HAND SIDE through all levels first
  for (int l = top; l >= 1; l--) FH_TRY(restrict_into(mg, l, mg->lv[l].b));
  if (mg->cycle_type == FH_CYCLE_ADDITIVE) {
    // every level solves for itself from zero with its down smoother, the corrections are interpolated upwards and added
    for (int l = top; l >= 1; l--) {
      bool packed = false;
      FH_TRY(smooth_level(mg, mg->lv[l], mg->lv[l].npre, true, &packed));
    }
    FH_TRY(coarse_solve(mg));
    for (int l = 1; l <= top; l++) FH_TRY(halo_spmv(mg->lv[l - 1].halo, mg->lv[l].P, mg->lv[l - 1].x, mg->lv[l - 1].n, mg->lv[l].x, 1, nullptr, nullptr, 0.0));
  } else if (mg->cycle_type == FH_CYCLE_FULL) {
    // coarsest solve, then per level: interpolate the solution as the guess and run one multiplicative cycle from there
    FH_TRY(coarse_solve(mg));
    for (int l = 1; l <= top; l++) {
      FH_TRY(halo_spmv(mg->lv[l - 1].halo, mg->lv[l].P, mg->lv[l - 1].x, mg->lv[l - 1].n, mg->lv[l].x, 0, nullptr, nullptr, 0.0));   // x_l = P x_{l-1}
      FH_TRY(mcycle(mg, l, false));
    }
  } else {   // FH_CYCLE_KASKADE: coarsest solve, then interpolate and smooth (down smoother) on the way up, no coarse-grid correction
    FH_TRY(coarse_solve(mg));
    for (int l = 1; l <= top; l++) {
      FH_TRY(halo_spmv(mg->lv[l - 1].halo, mg->lv[l].P, mg->lv[l - 1].x, mg->lv[l - 1].n, mg->lv[l].x, 0, nullptr, nullptr, 0.0));
      bool packed = false;
      FH_TRY(smooth_level(mg, mg->lv[l], mg->lv[l].npre, false, &packed));
    }
  }
  FH_CHECK_HIP(hipGetLastError());
  return 0;
}

// x_out = M^-1 b_in with raw device pointers
// b_in may BE the cycle's own right-hand-side buffer (lv[top].b: a caller inside this file wrote it there) and x_out may be null (the result stays
// in lv[top].x, read there by the caller before the next cycle): the Krylov loops save the two vector copies per application that way
static int apply_cycle(fh_mg_t mg, const double* b_in, double* x_out) {
  fh_ctx_t c = mg->ctx;
  const int top = mg->nlevels - 1;
  MgLevel& L = mg->lv[top];
  if (b_in != L.b) FH_CHECK_HIP(hipMemcpyAsync(L.b, b_in, (size_t)L.n * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
  if (mg->gexec) {
    // the graph bakes in the x / x2 roles of the capture run, and that run left L.x (host side) pointing at the buffer it ended in;
    // run_cycle is never called un-captured while the graph exists, so the copy below reads the buffer the replay writes
    FH_CHECK_HIP(hipGraphLaunch(mg->gexec, c->stream));
  } else {
    FH_TRY(run_cycle(mg));
  }
  if (x_out && x_out != L.x) FH_CHECK_HIP(hipMemcpyAsync(x_out, L.x, (size_t)L.n * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
  return 0;
}

static int not_recording(fh_ctx_t c, const char* who) {
  hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
  FH_CHECK_HIP(hipStreamIsCapturing(c->stream, &st));
  FH_REQUIRE(st == hipStreamCaptureStatusNone, "%s: not inside fh_graph_begin / fh_graph_end (the cycle replays its own graph)", who);
  return 0;
}

extern "C" int fh_mg_vcycle(fh_mg_t mg, fh_vec_t b, fh_vec_t x) {
  FH_REQUIRE(mg && mg->setup_done, "fh_mg_vcycle: fh_mg_setup has not been called");
  FH_TRY(not_recording(mg->ctx, "fh_mg_vcycle"));
  const int n = mg->lv[mg->nlevels - 1].n;
  FH_REQUIRE(b->n_local >= n && x->n_local >= n, "fh_mg_vcycle: vectors too short");
  return apply_cycle(mg, b->d, x->d);
}

extern "C" int64_t fh_mg_cycle_algorithmic_bytes(fh_mg_t mg) { return mg->cycle_bytes; }

// coordinates of the unknowns of level 0 (any dimension 1..3): lets the exact coarse solve dissect its dense problem (option coarse_nd);
// without them it inverts one dense matrix
extern "C" int fh_mg_set_coarse_coords(fh_mg_t mg, int dim, int n, const double* coords) {
  FH_REQUIRE(mg && dim >= 1 && dim <= 3 && n >= 0 && (coords || n == 0), "fh_mg_set_coarse_coords: bad arguments");
  fh_coarse_set_coords(mg->coarse, dim, n, coords);
  return 0;
}

// what the last fh_mg_setup made of the coarsest level: unknowns in the dense problem, interior blocks of the dissection (0: one dense
// inverse), separator size, largest block
// coordinates of the unknowns of a level >= 1 whose preconditioner is the exact solve (FH_SMOOTH_LU): optional, as fh_mg_set_coarse_coords for level 0
extern "C" int fh_mg_set_level_coords(fh_mg_t mg, int level, int dim, int n, const double* coords) {
  FH_REQUIRE(mg && level >= 0 && level < mg->nlevels && dim >= 1 && dim <= 3 && n >= 0 && (coords || n == 0), "fh_mg_set_level_coords: bad arguments");
  if (level == 0) return fh_mg_set_coarse_coords(mg, dim, n, coords);
  MgLevel& L = mg->lv[level];
  L.xyz.assign(coords, coords + (size_t)n * dim);
  L.xyz_dim = dim;
  if (L.direct) {            // the tree was cut with other (or no) coordinates
    fh_direct_destroy(L.direct);
    L.direct = nullptr;
  }
  return 0;
}

extern "C" int fh_mg_coarse_info(fh_mg_t mg, int* n_dense, int* nd_blocks, int* nd_separator, int* nd_largest_block) {
  FH_REQUIRE(mg && mg->setup_done, "fh_mg_coarse_info: fh_mg_setup has not been called");
  fh_coarse_info(mg->coarse, n_dense, nd_blocks, nd_separator, nd_largest_block);
  return 0;
}

extern "C" int fh_mg_sweep_info(fh_mg_t mg, int level, int* forward, int* backward, int* ilu, double* ilu_shift) {
  FH_REQUIRE(mg && mg->setup_done, "fh_mg_sweep_info: fh_mg_setup has not been called");
  FH_REQUIRE(level >= 0 && level < mg->nlevels && mg->lv[level].tri, "fh_mg_sweep_info: level %d has no natural-order sweep (FH_SMOOTH_SOR, FH_SMOOTH_ILU0)", level);
  fh_tri_info(mg->lv[level].tri, forward, backward, ilu, ilu_shift);
  return 0;
}

extern "C" int fh_mg_destroy(fh_mg_t mg) {
  if (!mg) return 0;
  hipStreamSynchronize(mg->ctx->stream);
  if (mg->gexec) hipGraphExecDestroy(mg->gexec);
  if (mg->graph) hipGraphDestroy(mg->graph);
  for (auto& L : mg->lv) {
    free_level_buffers(L);
    free_level_colors(L);
    fh_patch_destroy(L.patch);
    L.patch = nullptr;
    fh_tri_destroy(L.tri);
    L.tri = nullptr;
    if (L.direct) fh_direct_destroy(L.direct);
    L.direct = nullptr;
  }
  fh_coarse_destroy(mg->coarse);
  mg->krylov.release();
  delete mg;
  return 0;
}

// ------------------------------------------------------------------------------------------------
// outer solvers (fh_krylov.hip): PREONLY / RICHARDSON(0.99999) / PCG / GMRES(restart) / flexible GMRES(restart) around the cycle
// ------------------------------------------------------------------------------------------------
extern "C" int fh_mg_solve(fh_mg_t mg, fh_vec_t bv, fh_vec_t xv, int outer, double rtol, double atol, double dtol, int maxit, int restart,
                           int* iterations, double* final_residual) {
  FH_REQUIRE(mg && mg->setup_done, "fh_mg_solve: fh_mg_setup has not been called");
  fh_ctx_t c = mg->ctx;
  MgLevel& top = mg->lv[mg->nlevels - 1];
  fh_mat_t A = top.A;
  fh_halo_t HL = top.halo;
  // the finest level as the solvers see it: the distributed forms of the global operations (MatMult with ghost refresh, VecDot with all-reduce),
  // and the cycle as the preconditioner, reading lv[top].b in place and leaving its result in lv[top].x
  KrylovOps op;
  op.ctx = c;
  op.n = A->m;               // owned rows
  op.ncols = top.ncols;      // owned + ghosts on a distributed level
  FH_REQUIRE(bv->n_local >= op.n && xv->n_local + xv->nghost >= op.ncols, "fh_mg_solve: vectors too short");
  FH_REQUIRE(outer >= 0 && outer <= 4, "fh_mg_solve: unknown outer solver %d", outer);
  op.spmv = [=](double* x, double* y, int mode, const double* b) { return halo_spmv(HL, A, x, A->m, y, mode, b, nullptr, 0.0); };
  op.allreduce = [=](double* d, int count) { return HL ? fh_halo_allreduce_ptr(HL, d, count) : 0; };
  op.allreduce_host = [=](double* vals, int count) { return HL ? fh_halo_allreduce_sum(HL, vals, count) : 0; };
  op.precond = [=](const double* in, double* out) { return apply_cycle(mg, in, out); };
  op.precond_result = [&top]() { return top.x; };
  op.precond_input = top.b;
  double *b = bv->d, *x = xv->d;
  int its = 0, rc = 0;
  double rn = 0.0;
  switch (outer) {
    case FH_OUTER_PREONLY: rc = fh_krylov_preonly(op, b, x, &its); break;
    case FH_OUTER_RICHARDSON: rc = fh_krylov_richardson(op, mg->krylov, b, x, rtol, atol, dtol, maxit, &its, &rn); break;
    case FH_OUTER_CG: rc = fh_krylov_cg(op, mg->krylov, b, x, rtol, atol, dtol, maxit, &its, &rn); break;
    case FH_OUTER_FGMRES: rc = fh_krylov_gmres_host(op, mg->krylov, true, b, x, rtol, atol, dtol, maxit, restart, &its, &rn); break;
    default:      // FH_OUTER_GMRES: device-resident unless option gmres_device is 0
      rc = c->gmres_device ? fh_krylov_gmres_device(op, mg->krylov, b, x, rtol, atol, dtol, maxit, restart, &its, &rn)
                           : fh_krylov_gmres_host(op, mg->krylov, false, b, x, rtol, atol, dtol, maxit, restart, &its, &rn);
  }
  if (rc) return rc;
  FH_CHECK_HIP(hipStreamSynchronize(c->stream));
  if (iterations) *iterations = its;
  if (final_residual) *final_residual = rn;
  return 0;
}
