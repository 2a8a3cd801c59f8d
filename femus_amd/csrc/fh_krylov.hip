// Krylov solvers on gfx950: the outer solvers of fh_mg_solve (KSPPREONLY / KSPRICHARDSON / KSPCG / KSPGMRES / KSPFGMRES around the multigrid cycle,
// LinearEquationSolverPetsc.cpp:294-335, 506-507) and GMRES as the solver of a level (:238-250, 501-502).  They see the operator and the cycle through
// KrylovOps (fh_krylov.h), never through the multigrid object; their workspaces are KrylovWork and LevelGmres.  The small dense algebra of GMRES --
// one Hessenberg column through the Givens rotations, the back substitution -- is fh_hessenberg.h, shared by the device kernel and the host loop.
#include "fh_krylov.h"
#include "fh_hessenberg.h"
#include <cmath>

// ------------------------------------------------------------------------------------------------
// kernels
// ------------------------------------------------------------------------------------------------
// V^T w for nvec basis vectors (GMRES classical Gram-Schmidt): partials[j*nb + block]
__global__ __launch_bounds__(256) void k_multidot(const double* const* __restrict__ V, const double* __restrict__ w, int nvec, int n,
                                                  double* __restrict__ part) {
  __shared__ double sm[4];
  for (int j = 0; j < nvec; j++) {
    const double* v = V[j];
    double acc = 0.0;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) acc += v[i] * w[i];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
    if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) part[(size_t)j * gridDim.x + blockIdx.x] = sm[0] + sm[1] + sm[2] + sm[3];
    __syncthreads();
  }
}

__global__ __launch_bounds__(256) void k_multidot_final(double* __restrict__ part, int nvec, int nb) {
  __shared__ double sm[4];
  const int j = blockIdx.x;
  double acc = 0.0;
  for (int i = threadIdx.x; i < nb; i += 256) acc += part[(size_t)j * nb + i];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
  if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) part[(size_t)nvec * nb + j] = sm[0] + sm[1] + sm[2] + sm[3];
}

// w -= sum_j h[j] V_j   (h on the device, right behind the partials)
__global__ __launch_bounds__(256) void k_multiaxpy(double* __restrict__ w, const double* const* __restrict__ V, const double* __restrict__ h,
                                                   double sign, int nvec, int n) {
  for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
    double acc = w[i];
    for (int j = 0; j < nvec; j++) acc += sign * h[j] * V[j][i];
    w[i] = acc;
  }
}

__global__ __launch_bounds__(256) void k_axpby2(double* y, const double* x, double a, double b, int n) {   // x may alias y
  // BLAS semantics: with b == 0 the old y is NOT referenced (it may be uninitialised memory: 0 * NaN = NaN)
  for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) y[i] = (b == 0.0) ? a * x[i] : a * x[i] + b * y[i];
}

// ---- device-resident GMRES (the default outer solver): the Hessenberg column, the Givens rotations, the residual estimate and the convergence test live in
// a small state block on the device; the host reads {done, rn} back ONCE per iteration (one synchronisation instead of two, no arithmetic on the host) ----
// state layout (doubles): [0] reference norm beta0  [1] rtol  [2] atol  [3] dtol  [4] rn  [5] scale of the next basis vector (1 / h_{k+1,k}, or 1 / beta)
//                         [6] iterations done  [7] done flag  [8] maxit  [9] kused  [10] last norm  [11] restart   [16 ..] g, cs, sn, y, H (row-major, restart columns)
constexpr int GM_HDR = 16;
__host__ __device__ __forceinline__ double* gm_g(double* S) { return S + GM_HDR; }
__host__ __device__ __forceinline__ double* gm_cs(double* S, int m) { return S + GM_HDR + (m + 1); }
__host__ __device__ __forceinline__ double* gm_sn(double* S, int m) { return S + GM_HDR + (m + 1) + m; }
__host__ __device__ __forceinline__ double* gm_y(double* S, int m) { return S + GM_HDR + (m + 1) + 2 * m; }
__host__ __device__ __forceinline__ double* gm_H(double* S, int m) { return S + GM_HDR + (m + 1) + 3 * m; }
static size_t gm_state_doubles(int m) { return (size_t)GM_HDR + (m + 1) + 3 * (size_t)m + (size_t)(m + 1) * m; }

// squared norm, partial sums per block
__global__ __launch_bounds__(256) void k_sqnorm_part(const double* __restrict__ w, int n, double* __restrict__ part) {
  __shared__ double sm[4];
  double acc = 0.0;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) acc += w[i] * w[i];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
  if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) part[blockIdx.x] = sm[0] + sm[1] + sm[2] + sm[3];
}
__global__ __launch_bounds__(256) void k_sum_part(const double* __restrict__ part, int nb, double* __restrict__ out) {
  __shared__ double sm[4];
  double acc = 0.0;
  for (int i = threadIdx.x; i < nb; i += 256) acc += part[i];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
  if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) out[0] = sm[0] + sm[1] + sm[2] + sm[3];
}
// y = s[0] * x (s on the device)
__global__ __launch_bounds__(256) void k_scale_dev(double* __restrict__ y, const double* __restrict__ x, const double* __restrict__ s, int n) {
  const double a = s[0];
  for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) y[i] = a * x[i];
}
// Knoll guess done: beta0 = ||M^-1 b|| (sq = its square, summed over the ranks)
__global__ void k_gm_begin(double* __restrict__ S, const double* __restrict__ sq, double rtol, double atol, double dtol, int maxit, int restart) {
  S[0] = sqrt(sq[0]);
  S[1] = rtol; S[2] = atol; S[3] = dtol;
  S[4] = 0.0; S[5] = 0.0; S[6] = 0.0; S[7] = 0.0;
  S[8] = (double)maxit; S[9] = 0.0; S[10] = 0.0; S[11] = (double)restart;
}
// start of a restart cycle: beta = ||v0|| (sq = its square); converged / diverged / out of iterations -> done, otherwise g = beta e_0 and the scale 1 / beta
__global__ void k_gm_restart(double* __restrict__ S, const double* __restrict__ sq) {
  const int m = (int)S[11];
  const double beta = sqrt(sq[0]);
  S[4] = beta;
  S[10] = beta;
  S[9] = 0.0;
  double* g = gm_g(S);
  for (int i = 0; i <= m; i++) g[i] = 0.0;
  g[0] = beta;
  const bool stop = beta <= fmax(S[1] * S[0], S[2]) || S[6] >= S[8] || beta > S[3] * S[0];
  S[7] = stop ? 1.0 : 0.0;
  S[5] = (stop || beta == 0.0) ? 0.0 : 1.0 / beta;
}
// iteration k: h[0..k] = V^T w (before the orthogonalisation), wsq = ||w||^2 after it -> column k of the Hessenberg matrix, rotations, residual estimate,
// convergence test; at the end of a restart cycle (converged or k == restart - 1) the back substitution y = H^-1 g as well.  The same two functions
// (fh_hessenberg.h) as the host-driven loop below.
__global__ void k_gm_step(double* __restrict__ S, const double* __restrict__ h, const double* __restrict__ wsq, int k) {
  const int m = (int)S[11];
  double* g = gm_g(S);
  double* cs = gm_cs(S, m);
  double* sn = gm_sn(S, m);
  double* y = gm_y(S, m);
  double* H = gm_H(S, m);
  const double wn = sqrt(wsq[0]);
  for (int j = 0; j <= k; j++) H[(size_t)j * m + k] = h[j];
  H[(size_t)(k + 1) * m + k] = wn;
  S[10] = wn;
  S[5] = wn != 0.0 ? 1.0 / wn : 0.0;
  const bool done = fh_gmres_hessenberg_step(H, m, k, wn, g, cs, sn, S, S + 6, S + 8, S + 4);      // S[0 .. 3] = reference norm, rtol, atol, dtol
  const int kused = k + 1;
  S[9] = (double)kused;
  S[7] = done ? 1.0 : 0.0;
  if (done || k == m - 1) fh_gmres_back_substitute(H, m, kused, g, y);
}

// v <- v / sqrt(s2[0]), the norm goes to *hout (a zero norm -- lucky breakdown -- gives the zero vector and a zero entry)
__global__ __launch_bounds__(256) void k_gm_normalize(double* __restrict__ v, const double* __restrict__ s2, double* __restrict__ hout, int n) {
  const double nrm = sqrt(fmax(s2[0], 0.0));
  const double inv = nrm > 0.0 ? 1.0 / nrm : 0.0;
  if (blockIdx.x == 0 && threadIdx.x == 0) *hout = nrm;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) v[i] *= inv;
}
__global__ void k_gm_copy(double* __restrict__ dst, const double* __restrict__ src, int k) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < k) dst[i] = src[i];
}
// least-squares solution of min || beta e1 - H y ||, H (m + 1) x m stored by columns of length ld (Givens rotations, one thread)
__global__ void k_gm_solve(double* __restrict__ H, int ld, int m, const double* __restrict__ beta, double* __restrict__ g, double* __restrict__ y) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  for (int i = 0; i <= m; i++) g[i] = 0.0;
  g[0] = *beta;
  for (int k = 0; k < m; k++) {
    double* hk = H + (size_t)k * ld;
    // (rotations 0 .. k-1 have been applied to this column as they were formed: see below)
    const double a = hk[k], b2 = hk[k + 1];
    const double d = hypot(a, b2);
    const double cs = d > 0.0 ? a / d : 1.0, sn = d > 0.0 ? b2 / d : 0.0;
    hk[k] = d;
    hk[k + 1] = 0.0;
    const double t = cs * g[k] + sn * g[k + 1];
    g[k + 1] = -sn * g[k] + cs * g[k + 1];
    g[k] = t;
    for (int j = k + 1; j < m; j++) {          // the same rotation on the later columns
      double* hj = H + (size_t)j * ld;
      const double u = cs * hj[k] + sn * hj[k + 1];
      hj[k + 1] = -sn * hj[k] + cs * hj[k + 1];
      hj[k] = u;
    }
  }
  for (int k = m - 1; k >= 0; k--) {
    double acc = g[k];
    for (int j = k + 1; j < m; j++) acc -= H[(size_t)j * ld + k] * y[j];
    const double d = H[(size_t)k * ld + k];
    y[k] = d != 0.0 ? acc / d : 0.0;
  }
}

// ------------------------------------------------------------------------------------------------
// workspaces
// ------------------------------------------------------------------------------------------------
int KrylovWork::reserve(fh_ctx_t c, int nvec, int n, int ntable, int restart, bool need_device_state) {
  if ((int)kv.size() < nvec || kv_n != n) {
    for (double* p : kv) hipFree(p);
    kv.assign(nvec, nullptr);
    for (int i = 0; i < nvec; i++) {
      FH_CHECK_HIP(hipMalloc(&kv[i], ((size_t)n + 2) * sizeof(double)));
      // zero: ghost tails are read by the SpMV before any write.  debug_poison fills with NaN bit patterns instead, so that a test
      // can show that nothing ELSE of a work vector is read before it is written (tests/test_gpu_multigrid.py)
      FH_CHECK_HIP(hipMemsetAsync(kv[i], c->debug_poison ? 0xFF : 0, ((size_t)n + 2) * sizeof(double), c->stream));
    }
    kv_n = n;
  }
  if (ntable > 0) {      // basis pointers on the device: owned by the workspace (an early error return of a solver must not leak them)
    if (d_V_n < ntable) {
      if (d_V) FH_CHECK_HIP(hipFree(d_V));
      d_V = nullptr;
      d_V_n = 0;
      FH_CHECK_HIP(hipMalloc(&d_V, (size_t)ntable * sizeof(double*)));
      d_V_n = ntable;
    }
    FH_CHECK_HIP(hipMemcpyAsync(d_V, kv.data(), (size_t)ntable * sizeof(double*), hipMemcpyHostToDevice, c->stream));
  }
  if (need_device_state) {
    if (gm_cap < gm_state_doubles(restart)) {
      if (d_gm) FH_CHECK_HIP(hipFree(d_gm));
      d_gm = nullptr;
      gm_cap = 0;
      FH_CHECK_HIP(hipMalloc(&d_gm, gm_state_doubles(restart) * sizeof(double)));
      gm_cap = gm_state_doubles(restart);
    }
    if (!h_gm) FH_CHECK_HIP(hipHostMalloc(&h_gm, GM_HDR * sizeof(double)));
  }
  return 0;
}

void KrylovWork::release() {
  for (double* p : kv) hipFree(p);
  if (d_V) hipFree(d_V);
  if (d_gm) hipFree(d_gm);
  if (h_gm) hipHostFree(h_gm);
  *this = KrylovWork();
}

int LevelGmres::reserve(int m_new, int ncols, int n, fh_ctx_t c) {
  const size_t vs = (size_t)ncols + 2;
  if (m != m_new || !basis) {
    release();
    m = m_new;
    nb = sgrid(c, n);
    auto allocate = [&]() -> int {
      FH_CHECK_HIP(hipMalloc(&basis, (size_t)(m + 1) * vs * sizeof(double)));
      FH_CHECK_HIP(hipMalloc(&d_V, (size_t)(m + 1) * sizeof(double*)));
      FH_CHECK_HIP(hipMalloc(&small, small_doubles() * sizeof(double)));
      std::vector<double*> tab(m + 1);
      for (int j = 0; j <= m; j++) tab[j] = basis + (size_t)j * vs;
      FH_CHECK_HIP(hipMemcpy(d_V, tab.data(), tab.size() * sizeof(double*), hipMemcpyHostToDevice));
      return 0;
    };
    const int rc = allocate();
    if (rc) {
      release();
      return rc;
    }
  }
  FH_CHECK_HIP(hipMemsetAsync(basis, 0, (size_t)(m + 1) * vs * sizeof(double), c->stream));
  return 0;
}

void LevelGmres::release() {
  if (basis) hipFree(basis);
  if (d_V) hipFree(d_V);
  if (small) hipFree(small);
  *this = LevelGmres();
}

// ------------------------------------------------------------------------------------------------
// shared pieces
// ------------------------------------------------------------------------------------------------
static int dev_dot(fh_ctx_t c, const double* x, const double* y, int n, double* out) {
  fh_vec_s vx, vy;
  vx.ctx = vy.ctx = c;
  vx.n_local = vy.n_local = n;
  vx.d = const_cast<double*>(x);
  vy.d = const_cast<double*>(y);
  return fh_vec_dot(&vx, &vy, out);
}

static int dev_axpby(fh_ctx_t c, double* y, const double* x, double a, double b, int n) {
  hipLaunchKernelGGL(k_axpby2, dim3(sgrid(c, n)), dim3(256), 0, c->stream, y, x, a, b, n);
  FH_CHECK_HIP(hipGetLastError());
  return 0;
}

// *out = u . w over all ranks, on the host (VecDot)
static int dot(const KrylovOps& op, const double* u, const double* w, double* out) {
  FH_TRY(dev_dot(op.ctx, u, w, op.n, out));
  return op.allreduce_host(out, 1);
}

// V[0 .. nvec)^T w -> part[nvec * nb ...], summed over the ranks; the vectors come from a device pointer table, part holds (nvec + 1) * nb + nvec doubles
static int multidot(const KrylovOps& op, const double* const* d_V, const double* w, int nvec, int nb, double* part) {
  hipLaunchKernelGGL(k_multidot, dim3(nb), dim3(256), 0, op.ctx->stream, d_V, w, nvec, op.n, part);
  hipLaunchKernelGGL(k_multidot_final, dim3(nvec), dim3(256), 0, op.ctx->stream, part, nvec, nb);
  return op.allreduce(part + (size_t)nvec * nb, nvec);
}

// the projection of an Arnoldi step, classical Gram-Schmidt without refinement (PETSc's default): h = V[0 .. nvec)^T w in one pass, w -= V h.
// *h = the nvec projections on the device: behind the partial sums, or in `keep` when the caller names a place to keep them (the level solver's
// Hessenberg column)
static int arnoldi_project(const KrylovOps& op, const double* const* d_V, double* w, int nvec, int nb, double* part, double* keep, double** h) {
  FH_TRY(multidot(op, d_V, w, nvec, nb, part));
  *h = part + (size_t)nvec * nb;
  if (keep) {
    hipLaunchKernelGGL(k_gm_copy, dim3(fh_div_up(nvec, 64)), dim3(64), 0, op.ctx->stream, keep, *h, nvec);
    *h = keep;
  }
  hipLaunchKernelGGL(k_multiaxpy, dim3(nb), dim3(256), 0, op.ctx->stream, w, d_V, *h, -1.0, nvec, op.n);
  return 0;
}

// ------------------------------------------------------------------------------------------------
// GMRES as the level solver (FH_LEVEL_GMRES): what `SetSolverFineGrids(GMRES)` -- the reference's default `_levelSolverType`, and
// what 003_NavierStokes sets -- makes of a level (LinearEquationSolverPetsc.cpp:238-250, 501-502): exactly npre / npost iterations
// (PCMG skips the convergence test of its smoothers), left-preconditioned by the level's sweep preconditioner B (Jacobi, SOR,
// ILU(0), colour sweep, one multiplicative pass over the patches), classical Gram-Schmidt, restart _restart.  Minimises
// ||B (b - A x)||_2 over x0 + K_m(BA, B r0).  Everything stays on the device and on the stream -- dot products into device
// scalars, the (m + 1) x m least-squares problem in one single-thread kernel -- so the cycle remains one captured graph.
// ------------------------------------------------------------------------------------------------
int fh_gmres_smooth(LevelGmres& W, const KrylovOps& op, double* x, const double* b, double* r, int nits, bool zero_guess) {
  fh_ctx_t c = op.ctx;
  const int n = op.n, nb = W.nb, ld = W.m + 1;
  double *part = W.part(), *Hm = W.H(), *g = W.g(), *y = W.y(), *beta = W.beta();
  const double* const* d_V = W.d_V;
  auto V = [&](int j) { return W.vec(j, op.ncols); };
  int done = 0;
  while (done < nits) {
    const int m = std::min(W.m, nits - done);
    const bool zg = zero_guess && done == 0;
    if (zg) FH_TRY(op.precond(b, V(0)));
    else {
      FH_TRY(op.spmv(x, r, 2, b));
      FH_TRY(op.precond(r, V(0)));
    }
    // beta = ||V0||, V0 <- V0 / beta : the dot kernel takes its vectors from the pointer table, so V0 . V0 = table entry 0 against V0
    FH_TRY(multidot(op, d_V, V(0), 1, nb, part));
    hipLaunchKernelGGL(k_gm_normalize, dim3(sgrid(c, n)), dim3(256), 0, c->stream, V(0), part + (size_t)nb, beta, n);
    FH_CHECK_HIP(hipMemsetAsync(Hm, 0, (size_t)W.m * ld * sizeof(double), c->stream));
    for (int j = 0; j < m; j++) {
      FH_TRY(op.spmv(V(j), r, 0, nullptr));
      FH_TRY(op.precond(r, V(j + 1)));
      double* h;
      FH_TRY(arnoldi_project(op, d_V, V(j + 1), j + 1, nb, part, Hm + (size_t)j * ld, &h));
      FH_TRY(multidot(op, d_V + j + 1, V(j + 1), 1, nb, part));      // ||w||: table entry j + 1 is w itself
      hipLaunchKernelGGL(k_gm_normalize, dim3(sgrid(c, n)), dim3(256), 0, c->stream, V(j + 1), part + (size_t)nb, Hm + (size_t)j * ld + j + 1, n);
    }
    hipLaunchKernelGGL(k_gm_solve, dim3(1), dim3(1), 0, c->stream, Hm, ld, m, beta, g, y);
    if (zg) FH_CHECK_HIP(hipMemsetAsync(x, 0, (size_t)op.ncols * sizeof(double), c->stream));
    hipLaunchKernelGGL(k_multiaxpy, dim3(nb), dim3(256), 0, c->stream, x, d_V, y, 1.0, m, n);
    done += m;
  }
  FH_CHECK_HIP(hipGetLastError());
  return 0;
}

// ------------------------------------------------------------------------------------------------
// outer solvers
// ------------------------------------------------------------------------------------------------
// exactly one cycle per MGSolve (LinearEquationSolverPetsc.cpp:310-313)
int fh_krylov_preonly(const KrylovOps& op, double* b, double* x, int* its) {
  FH_TRY(op.precond(b, x));
  *its = 1;
  return 0;
}

// x <- x + 0.99999 M^-1 (b - A x), x0 = 0.  The scale of the OUTER Richardson is fixed by the reference itself: MGInit sets
// _richardsonScaleFactor = .99999 around SetSolver(_ksp) and restores the user's value afterwards (:190-193), so
// SetRichardsonScaleFactor only ever reaches the level smoothers (omega of fh_mg_set_level)
int fh_krylov_richardson(const KrylovOps& op, KrylovWork& W, double* b, double* x, double rtol, double atol, double dtol, int maxit, int* its_out,
                         double* rn_out) {
  fh_ctx_t c = op.ctx;
  const int n = op.n;
  FH_TRY(W.reserve(c, 2, op.ncols));
  double *r = W.kv[0], *z = W.kv[1];
  int its = 0;
  double rn = 0.0;
  FH_CHECK_HIP(hipMemsetAsync(x, 0, (size_t)n * sizeof(double), c->stream));
  double bn;
  FH_TRY(dot(op, b, b, &bn));
  bn = sqrt(bn);
  for (;;) {
    FH_TRY(op.spmv(x, r, 2, b));
    FH_TRY(dot(op, r, r, &rn));
    rn = sqrt(rn);
    if (rn <= std::max(rtol * bn, atol) || its >= maxit || rn > dtol * bn) break;
    FH_TRY(op.precond(r, z));
    FH_TRY(dev_axpby(c, x, z, 0.99999, 1.0, n));
    its++;
  }
  *its_out = its;
  *rn_out = rn;
  return 0;
}

int fh_krylov_cg(const KrylovOps& op, KrylovWork& W, double* b, double* x, double rtol, double atol, double dtol, int maxit, int* its_out,
                 double* rn_out) {
  fh_ctx_t c = op.ctx;
  const int n = op.n;
  FH_TRY(W.reserve(c, 4, op.ncols));
  double *r = W.kv[0], *z = W.kv[1], *p = W.kv[2], *Ap = W.kv[3];
  int its = 0;
  FH_CHECK_HIP(hipMemsetAsync(x, 0, (size_t)n * sizeof(double), c->stream));
  FH_CHECK_HIP(hipMemcpyAsync(r, b, (size_t)n * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
  double bn, rn, rz, rz_new, pAp;
  FH_TRY(dot(op, b, b, &bn));
  bn = sqrt(bn);
  rn = bn;
  FH_TRY(op.precond(r, z));
  FH_CHECK_HIP(hipMemcpyAsync(p, z, (size_t)n * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
  FH_TRY(dot(op, r, z, &rz));
  while (rn > std::max(rtol * bn, atol) && its < maxit && rn <= dtol * bn) {
    FH_TRY(op.spmv(p, Ap, 0, nullptr));
    FH_TRY(dot(op, p, Ap, &pAp));
    const double alpha = rz / pAp;
    FH_TRY(dev_axpby(c, x, p, alpha, 1.0, n));
    FH_TRY(dev_axpby(c, r, Ap, -alpha, 1.0, n));
    FH_TRY(dot(op, r, r, &rn));
    rn = sqrt(rn);
    its++;
    FH_TRY(op.precond(r, z));
    FH_TRY(dot(op, r, z, &rz_new));
    FH_TRY(dev_axpby(c, p, z, 1.0, rz_new / rz, n));
    rz = rz_new;
  }
  *its_out = its;
  *rn_out = rn;
  return 0;
}

// GMRES(restart) driven from the host, classical Gram-Schmidt, Knoll guess x0 = M^-1 b (LinearEquationSolverPetsc.cpp:294-335): two synchronisations
// per iteration, the small dense algebra on the host (fh_hessenberg.h).  Two forms of one loop:
//   left-preconditioned (KSPGMRES with option gmres_device 0; same arithmetic in the same order as the device-resident form below):
//     w = M^-1 (A v_k), reference norm ||M^-1 b||, a restart cycle starts from v0 = M^-1 (b - A x), x += V y;
//   flexible (KSPFGMRES, :506-507): RIGHT preconditioning with the vectors z_k = M^-1 v_k kept, so the cycle may be a different operator at every
//     application (GMRES level solvers): w = A z_k, convergence on the TRUE residual norm against ||b|| (KSPConvergedDefault with a non-zero guess),
//     a restart cycle starts from v0 = b - A x, x += Z y.
int fh_krylov_gmres_host(const KrylovOps& op, KrylovWork& W, bool flexible, double* b, double* x, double rtol, double atol, double dtol, int maxit,
                         int restart, int* its_out, double* rn_out) {
  FH_REQUIRE(restart >= 1 && restart <= 200, "fh_mg_solve: restart %d out of range", restart);
  fh_ctx_t c = op.ctx;
  const int n = op.n;
  // flexible: v_0 .. v_restart, z_0 .. z_{restart-1} and w; otherwise v_0 .. v_restart (A v lands in the preconditioner's own input buffer t, and
  // w is wherever the preconditioner leaves its result)
  FH_TRY(W.reserve(c, flexible ? 2 * restart + 2 : restart + 3, op.ncols, flexible ? 2 * restart + 1 : restart + 1));
  double** V = W.kv.data();
  double** Z = V + restart + 1;
  double* t = op.precond_input;
  const double* const* d_V = W.d_V;
  const double* const* d_update = flexible ? W.d_V + restart + 1 : W.d_V;      // the vectors that update x
  const int nb = sgrid(c, n);
  FH_TRY(fh_reserve_reduction(c, (size_t)(restart + 2) * (nb + 1) + 64));
  auto residual_vector = [&]() -> int {                     // v0 of a restart cycle, not yet normalised
    if (flexible) return op.spmv(x, V[0], 2, b);            // v0 = b - A x
    FH_TRY(op.spmv(x, t, 2, b));                            // t = b - A x
    return op.precond(t, V[0]);                             // v0 = M^-1 t
  };
  auto next_direction = [&](int k, double** w) -> int {
    if (flexible) {
      *w = W.kv[2 * restart + 1];
      FH_TRY(op.precond(V[k], Z[k]));                       // z_k = M^-1 v_k
      return op.spmv(Z[k], *w, 0, nullptr);                 // w = A z_k
    }
    FH_TRY(op.spmv(V[k], t, 0, nullptr));
    FH_TRY(op.precond(t, nullptr));
    *w = op.precond_result();
    return 0;
  };
  std::vector<double> H((size_t)(restart + 1) * restart, 0.0), g(restart + 1), cs(restart), sn(restart), y(restart);
  int its = 0;
  double rn = 0.0;
  FH_TRY(op.precond(b, x));                                 // Knoll
  double ref;
  FH_TRY(dot(op, flexible ? b : x, flexible ? b : x, &ref));
  ref = sqrt(ref);
  const double tol[4] = {ref, rtol, atol, dtol};
  bool done = false;
  while (!done) {
    FH_TRY(residual_vector());
    double beta;
    FH_TRY(dot(op, V[0], V[0], &beta));
    beta = sqrt(beta);
    rn = beta;
    if (beta <= std::max(rtol * ref, atol) || its >= maxit || beta > dtol * ref) break;
    FH_TRY(dev_axpby(c, V[0], V[0], 0.0, 1.0 / beta, n));
    std::fill(g.begin(), g.end(), 0.0);
    g[0] = beta;
    int kused = 0;
    for (int k = 0; k < restart && !done; k++) {
      double *w, *h;
      FH_TRY(next_direction(k, &w));
      // h = V^T w (one pass), w -= V h, h_{k+1,k} = ||w||
      FH_TRY(arnoldi_project(op, d_V, w, k + 1, nb, c->d_red, nullptr, &h));
      FH_CHECK_HIP(hipMemcpyAsync(c->h_red, h, (k + 1) * sizeof(double), hipMemcpyDeviceToHost, c->stream));
      FH_CHECK_HIP(hipStreamSynchronize(c->stream));
      for (int j = 0; j <= k; j++) H[(size_t)j * restart + k] = c->h_red[j];
      double wn;
      FH_TRY(dot(op, w, w, &wn));
      wn = sqrt(wn);
      H[(size_t)(k + 1) * restart + k] = wn;
      // happy breakdown (w = 0: the Krylov space is invariant): the next basis vector is never used, but it must not stay
      // uninitialised / stale either
      if (wn != 0.0) FH_TRY(dev_axpby(c, V[k + 1], w, 1.0 / wn, 0.0, n));
      else FH_CHECK_HIP(hipMemsetAsync(V[k + 1], 0, (size_t)n * sizeof(double), c->stream));
      done = fh_gmres_hessenberg_step(H.data(), restart, k, wn, g.data(), cs.data(), sn.data(), tol, &its, &maxit, &rn);
      kused = k + 1;
    }
    fh_gmres_back_substitute(H.data(), restart, kused, g.data(), y.data());
    // x += V y (flexible: Z y)
    FH_CHECK_HIP(hipMemcpyAsync(c->d_red, y.data(), kused * sizeof(double), hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(k_multiaxpy, dim3(nb), dim3(256), 0, c->stream, x, d_update, c->d_red, 1.0, kused, n);
    FH_CHECK_HIP(hipStreamSynchronize(c->stream));
  }
  *its_out = its;
  *rn_out = rn;
  return 0;
}

// left-preconditioned GMRES(restart), classical Gram-Schmidt, Knoll guess x0 = M^-1 b (LinearEquationSolverPetsc.cpp:294-335), device-resident: the
// Hessenberg matrix, the rotations, the residual estimate and the convergence test stay on the device (k_gm_*); per iteration the host enqueues
// [A v, cycle, V^T w, w -= V h, ||w||^2, k_gm_step, v_{k+1} = w / h_{k+1,k}] and reads {done, rn, iterations} back once.  Same arithmetic in the same
// order as the host-driven form above (option gmres_device 0), which it replaces as the default.
int fh_krylov_gmres_device(const KrylovOps& op, KrylovWork& W, double* b, double* x, double rtol, double atol, double dtol, int maxit, int restart,
                           int* its_out, double* rn_out) {
  FH_REQUIRE(restart >= 1 && restart <= 200, "fh_mg_solve: restart %d out of range", restart);
  fh_ctx_t c = op.ctx;
  const int n = op.n;
  const int nb = sgrid(c, n);
  FH_TRY(W.reserve(c, restart + 3, op.ncols, restart + 1, restart, true));
  FH_TRY(fh_reserve_reduction(c, (size_t)(restart + 2) * (nb + 1) + nb + 64));
  double** V = W.kv.data();
  double* t = op.precond_input;
  const double* const* d_V = W.d_V;
  double* S = W.d_gm;
  // scratch inside the reduction buffer: partial sums [0, (restart + 1) * nb), the projections h behind them, then the partials of ||w||^2 and its sum
  double* sqp = c->d_red + (size_t)(restart + 2) * (nb + 1);
  double* sq1 = sqp + nb;
  auto sqnorm = [&](const double* v) -> int {          // sq1[0] = ||v||^2 over all ranks
    hipLaunchKernelGGL(k_sqnorm_part, dim3(nb), dim3(256), 0, c->stream, v, n, sqp);
    hipLaunchKernelGGL(k_sum_part, dim3(1), dim3(256), 0, c->stream, sqp, nb, sq1);
    return op.allreduce(sq1, 1);
  };
  auto readback = [&]() -> int {
    FH_CHECK_HIP(hipMemcpyAsync(W.h_gm, S, GM_HDR * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    FH_CHECK_HIP(hipStreamSynchronize(c->stream));
    return 0;
  };
  int its = 0;
  double rn = 0.0;
  // Knoll: x0 = M^-1 b ; reference norm = ||M^-1 b||
  FH_TRY(op.precond(b, x));
  FH_TRY(sqnorm(x));
  hipLaunchKernelGGL(k_gm_begin, dim3(1), dim3(1), 0, c->stream, S, sq1, rtol, atol, dtol, maxit, restart);
  bool done = false;
  while (!done) {
    FH_TRY(op.spmv(x, t, 2, b));                             // t = b - A x
    FH_TRY(op.precond(t, V[0]));                             // v0 = M^-1 t
    FH_TRY(sqnorm(V[0]));
    hipLaunchKernelGGL(k_gm_restart, dim3(1), dim3(1), 0, c->stream, S, sq1);
    hipLaunchKernelGGL(k_scale_dev, dim3(nb), dim3(256), 0, c->stream, V[0], V[0], S + 5, n);
    FH_CHECK_HIP(hipGetLastError());
    FH_TRY(readback());
    rn = W.h_gm[4];
    if (W.h_gm[7] != 0.0) break;
    int kused = 0;
    for (int k = 0; k < restart && !done; k++) {
      FH_TRY(op.spmv(V[k], t, 0, nullptr));
      FH_TRY(op.precond(t, nullptr));
      double* w = op.precond_result();
      // h = V^T w (one pass), w -= V h, h_{k+1,k} = ||w||
      double* h;
      FH_TRY(arnoldi_project(op, d_V, w, k + 1, nb, c->d_red, nullptr, &h));
      FH_TRY(sqnorm(w));
      hipLaunchKernelGGL(k_gm_step, dim3(1), dim3(1), 0, c->stream, S, h, sq1, k);
      // v_{k+1} = w / h_{k+1,k} (zero on a happy breakdown: the scale is 0 then); never used when the test above said stop
      hipLaunchKernelGGL(k_scale_dev, dim3(nb), dim3(256), 0, c->stream, V[k + 1], w, S + 5, n);
      FH_CHECK_HIP(hipGetLastError());
      FH_TRY(readback());
      its = (int)W.h_gm[6];
      rn = W.h_gm[4];
      kused = k + 1;
      done = W.h_gm[7] != 0.0;
    }
    // x += V y (y from the back substitution inside the last k_gm_step)
    hipLaunchKernelGGL(k_multiaxpy, dim3(nb), dim3(256), 0, c->stream, x, d_V, gm_y(S, restart), 1.0, kused, n);
    FH_CHECK_HIP(hipGetLastError());
  }
  *its_out = its;
  *rn_out = rn;
  return 0;
}
