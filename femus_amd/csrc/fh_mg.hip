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
#include "fh_trisolve.h"
#include <algorithm>
#include <memory>
#include <cmath>

int fh_dev_get_diag(fh_mat_t A, double* d, int invert);
int fh_halo_update_ptr(fh_halo_t h, double* vd, int n_owned);
int fh_halo_end_ptr(fh_halo_t h);
int fh_halo_allreduce_ptr(fh_halo_t h, double* d, int n);
int fh_direct_solve_ptr(fh_direct_t d, const double* b, double* x);
uint64_t fh_direct_generation(fh_direct_t d);      // changes whenever the object re-analysed its operator (new device buffers, new launch shapes)

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
  // block Schwarz (Vanka) smoother: dof patches, their colours and dense inverses
  int npatch = 0, vanka_ncolors = 0, max_patch = 0;
  int npatch_exact = 0;       // FH_SMOOTH_ASM: the first npatch_exact blocks get the EXACT sub-solve (MLU_PRECOND on the solid / porous blocks, LinearEquationSolverPetscAsm.cpp:298-307)
  std::vector<int> h_pptr, h_pdofs, vcolor_ptr;
  std::vector<int64_t> h_poff;
  int *d_pptr = nullptr, *d_pdofs = nullptr, *d_porder = nullptr, *d_pflag = nullptr, *d_pcptr = nullptr;
  int4* d_pdesc = nullptr;    // per patch dof: {row, first entry, end of the row, 0} -- one load instead of the chain dof -> row pointer (k_vanka_color_fused)
  unsigned* d_pbar = nullptr;      // arrival / exit counters of the persistent sweep
  int vanka_maxcolor = 0;          // patches of the largest colour
  int pbar_len = 0;
  int64_t* d_poff = nullptr;
  double* d_pinv = nullptr;
  // FH_SMOOTH_ASM (PCASM as the reference configures it): scratch of the block ILU(0) products and the pattern masks of the blocks; order_kind
  // says how d_porder / d_pcptr were made (0: greedy colours, 1: dependency levels of the blocks in their index order)
  double* d_pscr = nullptr;
  unsigned char* d_pmask = nullptr;
  int order_kind = -1;
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

// ------------------------------------------------------------------------------------------------
// block Schwarz (Vanka) smoother for saddle-point systems: x_p += omega A_pp^-1 (b - A x)_p for every patch p, patches of one
// colour concurrently (patches of a colour neither share a dof nor read one another's dofs, so the order inside a colour is
// irrelevant), colours in sequence = multiplicative Schwarz.  GPU form of the element-block ASM smoother the reference
// selects with FEMuS_ASM (petsc_asm/LinearEquationSolverPetscAsm.cpp:91-345).
// ------------------------------------------------------------------------------------------------
// dense copy of A restricted to the patch, stored TRANSPOSED (column-major) so that the apply kernel reads it coalesced
__global__ __launch_bounds__(256) void k_patch_extract(const int* __restrict__ pptr, const int* __restrict__ pdofs, const int64_t* __restrict__ poff,
                                                       const int* __restrict__ rowptr, const int* __restrict__ col, const double* __restrict__ val,
                                                       double* __restrict__ M) {
  const int p = blockIdx.x;
  const int* d = pdofs + pptr[p];
  const int np = pptr[p + 1] - pptr[p];
  double* Mp = M + poff[p];
  for (int t = threadIdx.x; t < np * np; t += 256) {
    const int a = t / np, b = t % np;    // entry (row a, col b) of the patch matrix
    const int r = d[a], c = d[b];
    int lo = rowptr[r], hi = rowptr[r + 1] - 1;
    double v = 0.0;
    while (lo <= hi) {
      const int mid = lo + ((hi - lo) >> 1);   // (lo + hi) overflows beyond 2^30 non-zeros
      const int cc = col[mid];
      if (cc == c) {
        v = val[mid];
        break;
      }
      if (cc < c) lo = mid + 1; else hi = mid - 1;
    }
    Mp[(size_t)a * np + b] = v;
  }
}

// in-place inverse by Gauss-Jordan with partial (row) pivoting, one workgroup per patch, row-major in global memory (the
// patch matrix is L2-resident); on exit the matrix is transposed in place for the apply kernel.  flag[p] = 1: singular.
__global__ __launch_bounds__(256) void k_patch_invert(const int* __restrict__ pptr, const int64_t* __restrict__ poff, double* __restrict__ M,
                                                      int* __restrict__ flag, int skip_upto) {
  __shared__ int piv[512];
  __shared__ double red_v[256];
  __shared__ int red_i[256];
  __shared__ double colk[512];
  const int p = blockIdx.x, tid = threadIdx.x;
  const int n = pptr[p + 1] - pptr[p];
  if (n <= skip_upto) return;                   // inverted by k_patch_invert_lds
  double* A = M + poff[p];
  bool singular = false;
  for (int k = 0; k < n; k++) {
    // pivot search: largest |A[i][k]|, i >= k, smallest index on ties
    double best = -1.0;
    int bi = k;
    for (int i = k + tid; i < n; i += 256) {
      const double v = fabs(A[(size_t)i * n + k]);
      if (v > best) {
        best = v;
        bi = i;
      }
    }
    red_v[tid] = best;
    red_i[tid] = bi;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
      if (tid < s) {
        const double v2 = red_v[tid + s];
        const int i2 = red_i[tid + s];
        if (v2 > red_v[tid] || (v2 == red_v[tid] && i2 < red_i[tid])) {
          red_v[tid] = v2;
          red_i[tid] = i2;
        }
      }
      __syncthreads();
    }
    const int pr = red_i[0];
    const double pmax = red_v[0];
    __syncthreads();
    if (tid == 0) piv[k] = pr;
    if (!(pmax > 0.0)) {
      singular = true;
      break;
    }
    if (pr != k)
      for (int j = tid; j < n; j += 256) {
        const double t = A[(size_t)k * n + j];
        A[(size_t)k * n + j] = A[(size_t)pr * n + j];
        A[(size_t)pr * n + j] = t;
      }
    __syncthreads();
    const double pv = 1.0 / A[(size_t)k * n + k];
    for (int i = tid; i < n; i += 256) colk[i] = A[(size_t)i * n + k];
    __syncthreads();
    for (int j = tid; j < n; j += 256) A[(size_t)k * n + j] = (j == k) ? pv : A[(size_t)k * n + j] * pv;
    __syncthreads();
    for (int t = tid; t < n * n; t += 256) {
      const int i = t / n, j = t % n;
      if (i == k) continue;
      const double f = colk[i];
      const double akj = A[(size_t)k * n + j];
      A[t] = (j == k) ? -f * akj : A[t] - f * akj;
    }
    __syncthreads();
  }
  if (singular) {
    if (tid == 0) flag[p] = 1;
    return;
  }
  // undo the row interchanges as column interchanges, last first
  for (int k = n - 1; k >= 0; k--) {
    const int pr = piv[k];
    if (pr != k)
      for (int i = tid; i < n; i += 256) {
        const double t = A[(size_t)i * n + k];
        A[(size_t)i * n + k] = A[(size_t)i * n + pr];
        A[(size_t)i * n + pr] = t;
      }
    __syncthreads();
  }
  // transpose in place
  for (int t = tid; t < n * n; t += 256) {
    const int i = t / n, j = t % n;
    if (i < j) {
      const double a = A[(size_t)i * n + j];
      A[(size_t)i * n + j] = A[(size_t)j * n + i];
      A[(size_t)j * n + i] = a;
    }
  }
}

// the same inversion for patches of at most PLDS_MAX dofs, whole matrix in LDS, ONE wave per patch (no workgroup barriers; the same
// pivot rule -- largest |a_ik|, smallest row on ties -- and the same arithmetic per entry as k_patch_invert, so both give the same bits)
constexpr int PLDS_MAX = 96;
__device__ __forceinline__ void wave_sync_lds() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
__global__ __launch_bounds__(64) void k_patch_invert_lds(const int* __restrict__ pptr, const int64_t* __restrict__ poff, double* __restrict__ M,
                                                         int* __restrict__ flag, int nmax) {
  extern __shared__ double pl_smem[];
  const int p = blockIdx.x, lane = threadIdx.x;
  const int n = pptr[p + 1] - pptr[p];
  if (n > PLDS_MAX) return;                      // left to k_patch_invert
  const int ld = n | 1;
  double* As = pl_smem;                          // [n][ld]
  double* colk = pl_smem + nmax * (nmax | 1);    // nmax: the largest patch this launch inverts (sizes the LDS of every workgroup)
  int* piv = reinterpret_cast<int*>(colk + nmax);
  double* A = M + poff[p];
  for (int t = lane; t < n * n; t += 64) As[(t / n) * ld + t % n] = A[t];
  wave_sync_lds();
  for (int k = 0; k < n; k++) {
    double best = -1.0, bval = 0.0;
    int bi = k;
    for (int i = k + lane; i < n; i += 64) {
      const double v = As[i * ld + k];
      if (fabs(v) > best) {
        best = fabs(v);
        bval = v;
        bi = i;
      }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const double v2 = __shfl_xor(best, off, 64), w2 = __shfl_xor(bval, off, 64);
      const int i2 = __shfl_xor(bi, off, 64);
      if (v2 > best || (v2 == best && i2 < bi)) {
        best = v2;
        bval = w2;
        bi = i2;
      }
    }
    const int pr = bi;
    if (!(best > 0.0)) {
      if (lane == 0) flag[p] = 1;
      return;
    }
    if (lane == 0) piv[k] = pr;
    const double pv = 1.0 / bval;
    // column k of the other rows (after the interchange), then the interchange and the scaled pivot row, every lane its own columns
    for (int i = lane; i < n; i += 64) colk[i] = (i == pr) ? As[k * ld + k] : As[i * ld + k];
    wave_sync_lds();
    for (int j = lane; j < n; j += 64) {
      const double akj = As[pr * ld + j];
      if (pr != k) As[pr * ld + j] = As[k * ld + j];
      As[k * ld + j] = (j == k) ? pv : akj * pv;
    }
    wave_sync_lds();
    for (int j = lane; j < n; j += 64) {
      const double akj = As[k * ld + j];
      for (int i0 = 0; i0 < n; i0 += 8) {          // eight rows at a time: all loads issued before the first store
        double a[8], f[8];
#pragma unroll
        for (int u = 0; u < 8; u++) {
          const int i = min(i0 + u, n - 1);
          a[u] = As[i * ld + j];
          f[u] = colk[i];
        }
#pragma unroll
        for (int u = 0; u < 8; u++) {
          const int i = i0 + u;
          if (i < n && i != k) As[i * ld + j] = (j == k) ? -f[u] * akj : a[u] - f[u] * akj;
        }
      }
    }
    wave_sync_lds();
  }
  // undo the row interchanges as column interchanges, last first
  for (int k = n - 1; k >= 0; k--) {
    const int pr = piv[k];
    if (pr != k)
      for (int i = lane; i < n; i += 64) {
        const double t = As[i * ld + k];
        As[i * ld + k] = As[i * ld + pr];
        As[i * ld + pr] = t;
      }
    wave_sync_lds();
  }
  // transposed back to global memory
  for (int t = lane; t < n * n; t += 64) A[t] = As[(t % n) * ld + t / n];
}

// one colour of the sweep; one workgroup of 64 per patch.  r = b - A x of the whole level is formed once per colour by the
// fused SpMV (patches of a colour do not read each other's dofs, so it is the exact residual for every patch of the colour);
// the patch gathers its rows of r, applies the dense inverse and updates x
__global__ __launch_bounds__(64) void k_vanka_color(const int* __restrict__ order, int npat, const int* __restrict__ pptr, const int* __restrict__ pdofs,
                                                    const int64_t* __restrict__ poff, const double* __restrict__ Minv, const double* __restrict__ r,
                                                    double* x, double omega) {
  extern __shared__ double rp[];
  if ((int)blockIdx.x >= npat) return;
  const int p = order[blockIdx.x], lane = threadIdx.x;
  const int* d = pdofs + pptr[p];
  const int np = pptr[p + 1] - pptr[p];
  for (int a = lane; a < np; a += 64) rp[a] = r[d[a]];
  __syncthreads();
  const double* Mi = Minv + poff[p];     // transposed inverse: Mi[b * np + a] = inv[a][b]
  for (int a = lane; a < np; a += 64) {
    double s = 0.0;
    for (int c = 0; c < np; c++) s += Mi[(size_t)c * np + a] * rp[c];
    x[d[a]] += omega * s;
  }
}

// The same colour in ONE launch (round 5, default: option vanka_fused 1): every patch forms the residual of ITS OWN rows (4 lanes per row, 16 rows at a
// time) instead of reading a residual of the whole level that a separate SpMV launch has just made -- exact for the colour, because its patches do not
// read each other's dofs.  Half the launches of a sweep (the cycles of config 4 are launch-latency bound: ~380 launches of 4-9 us) and none of the
// residual rows nobody reads.  One workgroup of four waves per patch: 8 lanes per row, the dense inverse applied a quarter of the columns per wave.
__global__ __launch_bounds__(256) void k_patch_desc(int n, const int* __restrict__ pdofs, const int* __restrict__ rowptr, int4* __restrict__ desc) {
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k >= n) return;
  const int r = pdofs[k];
  desc[k] = make_int4(r, rowptr[r], rowptr[r + 1], 0);
}
__global__ __launch_bounds__(256) void k_vanka_color_fused(const int* __restrict__ order, int npat, const int* __restrict__ pptr, const int4* __restrict__ pdesc,
                                                           const int64_t* __restrict__ poff, const double* __restrict__ Minv, const int* __restrict__ col,
                                                           const double* __restrict__ val, const double* __restrict__ b, double* x, double omega, int max_patch) {
  extern __shared__ double vf_smem[];
  double* rp = vf_smem;                          // [max_patch] residual of the patch rows
  double* part = vf_smem + max_patch;            // [4][max_patch] partial products of the four waves
  if ((int)blockIdx.x >= npat) return;
  const int p = order[blockIdx.x], tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, sub = tid & 7, rl = tid >> 3;
  const int p0 = pptr[p], np = pptr[p + 1] - p0;
  const int4* d = pdesc + p0;
  const double* Mi = Minv + poff[p];             // transposed inverse: Mi[c * np + a] = inv[a][c]
  const int c0 = (np * wave) >> 2, c1 = (np * (wave + 1)) >> 2;          // this wave's quarter of the columns
  // the step is a chain of dependent memory round trips (cycles of config 4: 192 colour steps of 15-25 us): what does not depend on x goes out first --
  // this thread's entries of the inverse (patches of <= 64 dofs: at most sixteen), the row descriptors ({row, first, end} in one load)
  constexpr int MR = 16;
  double mreg[MR];
  const bool small = np <= 64;
  if (small) {
#pragma unroll
    for (int q = 0; q < MR; q++) mreg[q] = (lane < np && c0 + q < c1) ? Mi[(size_t)(c0 + q) * np + lane] : 0.0;
  }
  for (int a0 = 0; a0 < np; a0 += 32) {          // 32 rows at a time, 8 lanes per row (one wave per patch and 4 lanes per row was latency bound: 184 instead
    const int a = a0 + rl;                       //  of 120 ms per linear solve of config 4)
    double acc = 0.0, bb = 0.0;
    if (a < np) {
      const int4 q = d[a];
      bb = b[q.x];
      for (int kk = q.y + sub; kk < q.z; kk += 8) acc += val[kk] * x[col[kk]];
    }
    acc += __shfl_xor(acc, 1, 64);
    acc += __shfl_xor(acc, 2, 64);
    acc += __shfl_xor(acc, 4, 64);
    if (a < np && sub == 0) rp[a] = bb - acc;
  }
  __syncthreads();
  if (small) {
    double s = 0.0;
#pragma unroll
    for (int q = 0; q < MR; q++) s += mreg[q] * rp[min(c0 + q, np - 1)];          // (entries beyond c1 are zero)
    if (lane < np) part[wave * max_patch + lane] = s;
  } else {
    for (int a = lane; a < np; a += 64) {
      double s = 0.0;
      for (int c = c0; c < c1; c++) s += Mi[(size_t)c * np + a] * rp[c];
      part[wave * max_patch + a] = s;
    }
  }
  __syncthreads();
  for (int a = tid; a < np; a += 256) x[d[a].x] += omega * (((part[a] + part[max_patch + a]) + part[2 * max_patch + a]) + part[3 * max_patch + a]);
}

// ALL colours of ALL sweeps in one launch (fh_set_option(vanka_persistent, 1 | 2); off by default): a grid of resident one-wave workgroups walks
// the colours together, a device-wide barrier between two colours instead of a launch boundary.  Every patch forms the residual
// of its own rows (4 lanes per row, shuffle reduction), exact for the colour because its patches do not read each other's dofs;
// pass A of a step (patch dofs, row extents: independent of x) is issued BEFORE the barrier wait, so that after the barrier only
// the x-dependent part is on the critical path.  The grid is sized by the host to fit the device many times over (one wave and
// <= 4 KB of LDS per workgroup), which is what makes the spin barrier safe.  bar[0]: arrivals (monotone), bar[1]: exits; the
// last workgroup to leave zeroes both, so the next launch finds them clean.
// Barrier of the resident grid.  MODE 1: one arrival counter (bar[0], monotone over the launch; bar[1] counts exits and the last
// workgroup out zeroes both).  MODE 2: one flag per workgroup (plain stores, no read-modify-write on a shared address), workgroup 0
// polls them 64 at a time and publishes the step in bar[0]; at the end every workgroup clears its flag, workgroup 0 then bar[0].
__device__ __forceinline__ void wave_lds_sync() {      // LDS written by one lane, read by another lane of the same wave
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

template <int MODE>
__device__ __forceinline__ void vanka_grid_barrier(unsigned* bar, unsigned step) {
  __threadfence();                                   // release: this workgroup's x updates reach the other XCDs' view
  __syncthreads();
  if (MODE == 1) {
    if (threadIdx.x == 0) {
      __hip_atomic_fetch_add(bar, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      const unsigned target = step * gridDim.x;
      while (__hip_atomic_load(bar, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < target) __builtin_amdgcn_s_sleep(1);
    }
  } else {
    unsigned* flags = bar + 2;
    if (threadIdx.x == 0) __hip_atomic_store(flags + blockIdx.x, step, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (blockIdx.x == 0) {
      if (threadIdx.x < 64) {
        for (unsigned w = threadIdx.x; w < gridDim.x; w += 64)
          while (__hip_atomic_load(flags + w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != step) __builtin_amdgcn_s_sleep(1);
      }
      __syncthreads();
      if (threadIdx.x == 0) __hip_atomic_store(bar, step, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    } else if (threadIdx.x == 0) {
      while (__hip_atomic_load(bar, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != step) __builtin_amdgcn_s_sleep(1);
    }
  }
  __syncthreads();
  __threadfence();                                   // acquire: drop stale lines of x before the next colour reads it
}

template <int MODE>
__global__ __launch_bounds__(256) void k_vanka_persistent(const int* __restrict__ order, const int* __restrict__ cptr, int ncolors, int nsweeps,
                                                          const int* __restrict__ pptr, const int* __restrict__ pdofs,
                                                          const int64_t* __restrict__ poff, const double* __restrict__ Minv,
                                                          const int* __restrict__ rowptr, const int* __restrict__ col, const double* __restrict__ val,
                                                          const double* __restrict__ b, double* x, double omega, unsigned* bar, int max_patch) {
  extern __shared__ double rp_all[];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, sub = lane & 3, rl = lane >> 2;
  double* rp = rp_all + (size_t)wave * max_patch;     // one patch per wave
  const int nsteps = nsweeps * ncolors;
  for (int st = 0; st < nsteps; st++) {
    const int k = st % ncolors;
    const int c0 = cptr[k], npat = cptr[k + 1] - c0;
    if (st > 0) vanka_grid_barrier<MODE>(bar, (unsigned)st);
    for (int q = blockIdx.x * 4 + wave; q < npat; q += gridDim.x * 4) {
      const int p = order[c0 + q];
      const int* d = pdofs + pptr[p];
      const int np = pptr[p + 1] - pptr[p];
      for (int a0 = 0; a0 < np; a0 += 16) {            // 16 rows at a time, 4 lanes per row
        const int a = a0 + rl;
        double acc = 0.0;
        int row = 0;
        if (a < np) {
          row = d[a];
          const int ke = rowptr[row + 1];
          for (int kk = rowptr[row] + sub; kk < ke; kk += 4) acc += val[kk] * x[col[kk]];
        }
        acc += __shfl_xor(acc, 1, 64);
        acc += __shfl_xor(acc, 2, 64);
        if (a < np && sub == 0) rp[a] = b[row] - acc;
      }
      wave_lds_sync();
      const double* Mi = Minv + poff[p];               // transposed inverse: Mi[c * np + a] = inv[a][c]
      for (int a = lane; a < np; a += 64) {
        double s = 0.0;
        for (int c = 0; c < np; c++) s += Mi[(size_t)c * np + a] * rp[c];
        x[d[a]] += omega * s;
      }
      wave_lds_sync();
    }
  }
  // leave with clean counters for the next launch
  if (MODE == 1) {
    __syncthreads();
    if (threadIdx.x == 0) {
      const unsigned left = __hip_atomic_fetch_add(bar + 1, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
      if (left == gridDim.x - 1) {
        __hip_atomic_store(bar, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(bar + 1, 0u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
      }
    }
  } else if (nsteps > 1) {
    vanka_grid_barrier<MODE>(bar, (unsigned)nsteps);  // everybody has read the last published step ...
    vanka_grid_barrier<MODE>(bar, 0u);                // ... and the flags and the step go back to zero
  }
}


static inline int halo_spmv(fh_halo_t h, fh_mat_t A, double* x, int n_own, double* y, int mode, const double* b, const double* dinv, double omega,
                            bool prepacked = false) {
  return fh_dev_halo_spmv(h, A, x, n_own, y, mode, b, dinv, omega, prepacked);
}

// ------------------------------------------------------------------------------------------------
// API
// ------------------------------------------------------------------------------------------------
static void free_level_colors(MgLevel& L);
static void free_level_patch_setup(MgLevel& L);
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
    free_level_patch_setup(L);
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
      mixp(M->d_blkinfo);
      mixp(M->d_rowblk);
      mix((uint64_t)M->nblk);
      mix((uint64_t)M->tile);
      mix((uint64_t)M->lx_tile);
    }
  };
  mix((uint64_t)mg->nlevels);
  mix((uint64_t)mg->cycle_type);
  mix((uint64_t)mg->ctx->opt_gen);
  std::vector<uint64_t> cw;
  fh_coarse_signature(mg->coarse, cw);
  for (uint64_t w : cw) mix(w);
  for (int l = 0; l < mg->nlevels; l++) {
    MgLevel& L = mg->lv[l];
    mixm(L.A);
    mixm(L.P);
    mixm(L.R);
    mix((uint64_t)L.smoother);
    mix((uint64_t)L.npatch_exact);
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
    mixp(L.d_pinv);
    mixp(L.d_porder);
    mix((uint64_t)L.vanka_ncolors);
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

// device side of the patch smoother (colouring by the matrix graph, inverses): rebuilt by the next setup; the patch lists stay
static void free_level_patch_setup(MgLevel& L) {
  for (void** q : {(void**)&L.d_pptr, (void**)&L.d_pdofs, (void**)&L.d_porder, (void**)&L.d_pflag, (void**)&L.d_poff, (void**)&L.d_pinv, (void**)&L.d_pcptr,
                   (void**)&L.d_pbar, (void**)&L.d_pscr, (void**)&L.d_pmask, (void**)&L.d_pdesc})
    if (*q) {
      hipFree(*q);
      *q = nullptr;
    }
  L.vanka_ncolors = 0;
}

static void free_level_patches(MgLevel& L) {
  free_level_patch_setup(L);
  L.npatch = 0;
}

extern "C" int fh_mg_set_level_patches(fh_mg_t mg, int level, int npatch, const int* ptr, const int* dofs) {
  FH_REQUIRE(mg && level >= 0 && level < mg->nlevels && npatch > 0 && ptr && dofs, "fh_mg_set_level_patches: bad arguments");
  MgLevel& L = mg->lv[level];
  free_level_patches(L);
  L.npatch = npatch;
  L.h_pptr.assign(ptr, ptr + npatch + 1);
  L.h_pdofs.assign(dofs, dofs + ptr[npatch]);
  L.h_poff.assign(npatch + 1, 0);
  L.max_patch = 0;
  for (int p = 0; p < npatch; p++) {
    const int np = ptr[p + 1] - ptr[p];
    FH_REQUIRE(np > 0 && np <= 512, "fh_mg_set_level_patches: patch %d has %d dofs (1..512 supported)", p, np);
    L.max_patch = std::max(L.max_patch, np);
    L.h_poff[p + 1] = L.h_poff[p] + (int64_t)np * np;
  }
  L.npatch_exact = 0;
  mg->setup_done = false;
  return 0;
}

extern "C" int fh_mg_set_level_patches_exact(fh_mg_t mg, int level, int nfirst) {
  FH_REQUIRE(mg && level >= 0 && level < mg->nlevels, "fh_mg_set_level_patches_exact: bad arguments");
  MgLevel& L = mg->lv[level];
  FH_REQUIRE(nfirst >= 0 && nfirst <= L.npatch, "fh_mg_set_level_patches_exact: %d of %d blocks", nfirst, L.npatch);
  L.npatch_exact = nfirst;
  mg->setup_done = false;
  return 0;
}

// greedy colouring in patch order; two patches conflict when a dof of one appears in the matrix rows of the other
// sequential = false: greedy colours (patches of a colour neither share nor read each other's dofs; colours in any order -- the Vanka smoother).
// sequential = true (FH_SMOOTH_ASM): the blocks keep their INDEX ORDER, as PCASM's multiplicative composition visits them: block p gets the
// dependency level 1 + max level of the earlier blocks it conflicts with, so a level holds blocks whose order among themselves does not matter and
// the levels, run one after the other, give exactly the sequential sweep (level scheduling, as for the natural-order SOR / ILU sweeps)
static int color_patches(MgLevel& L, bool sequential) {
  const int n = L.A->m, np = L.npatch;
  const std::vector<int>&rp = L.A->h_rowptr, &cl = fh_hcol(L.A);
  for (int d : L.h_pdofs) FH_REQUIRE(d >= 0 && d < n, "Vanka smoother: patch dof %d out of range", d);
  std::vector<int> optr(n + 1, 0), rptr(n + 1, 0);
  std::vector<std::vector<int>> reads(np);
  std::vector<int> mark(n, -1);
  for (int p = 0; p < np; p++) {
    for (int q = L.h_pptr[p]; q < L.h_pptr[p + 1]; q++) {
      const int r = L.h_pdofs[q];
      optr[r + 1]++;
      for (int k = rp[r]; k < rp[r + 1]; k++)
        if (mark[cl[k]] != p) {
          mark[cl[k]] = p;
          reads[p].push_back(cl[k]);
        }
    }
    for (int c : reads[p]) rptr[c + 1]++;
  }
  for (int i = 0; i < n; i++) {
    optr[i + 1] += optr[i];
    rptr[i + 1] += rptr[i];
  }
  std::vector<int> owner(optr[n]), reader(rptr[n]), oc(optr.begin(), optr.end() - 1), rc(rptr.begin(), rptr.end() - 1);
  for (int p = 0; p < np; p++) {
    for (int q = L.h_pptr[p]; q < L.h_pptr[p + 1]; q++) owner[oc[L.h_pdofs[q]]++] = p;
    for (int c : reads[p]) reader[rc[c]++] = p;
  }
  std::vector<int> color(np, -1), used;
  int ncol = 0;
  for (int p = 0; p < np; p++) {
    used.assign(ncol + 1, 0);
    for (int c : reads[p])
      for (int k = optr[c]; k < optr[c + 1]; k++)
        if (color[owner[k]] >= 0) used[color[owner[k]]] = 1;
    for (int q = L.h_pptr[p]; q < L.h_pptr[p + 1]; q++) {
      const int d = L.h_pdofs[q];
      for (int k = rptr[d]; k < rptr[d + 1]; k++)
        if (color[reader[k]] >= 0) used[color[reader[k]]] = 1;
    }
    int c = 0;
    if (sequential) {
      for (int k = 0; k < ncol; k++)
        if (used[k]) c = k + 1;
    } else
      while (used[c]) c++;
    color[p] = c;
    ncol = std::max(ncol, c + 1);
  }
  L.vanka_ncolors = ncol;
  L.vcolor_ptr.assign(ncol + 1, 0);
  for (int p = 0; p < np; p++) L.vcolor_ptr[color[p] + 1]++;
  for (int c = 0; c < ncol; c++) L.vcolor_ptr[c + 1] += L.vcolor_ptr[c];
  std::vector<int> order(np), pos(L.vcolor_ptr.begin(), L.vcolor_ptr.end() - 1);
  for (int p = 0; p < np; p++) order[pos[color[p]]++] = p;
  auto up = [&](void** d, const void* h, size_t bytes) -> int {
    FH_CHECK_HIP(hipMalloc(d, bytes ? bytes : 8));
    if (bytes) FH_CHECK_HIP(hipMemcpy(*d, h, bytes, hipMemcpyHostToDevice));
    return 0;
  };
  FH_TRY(up((void**)&L.d_pptr, L.h_pptr.data(), L.h_pptr.size() * sizeof(int)));
  FH_TRY(up((void**)&L.d_pdofs, L.h_pdofs.data(), L.h_pdofs.size() * sizeof(int)));
  FH_CHECK_HIP(hipMalloc(&L.d_pdesc, std::max<size_t>(L.h_pdofs.size(), 1) * sizeof(int4)));
  hipLaunchKernelGGL(k_patch_desc, dim3(fh_div_up((int64_t)L.h_pdofs.size(), 256)), dim3(256), 0, L.A->ctx->stream, (int)L.h_pdofs.size(), L.d_pdofs, L.A->d_rowptr, L.d_pdesc);
  FH_CHECK_HIP(hipGetLastError());
  FH_TRY(up((void**)&L.d_poff, L.h_poff.data(), L.h_poff.size() * sizeof(int64_t)));
  FH_TRY(up((void**)&L.d_porder, order.data(), order.size() * sizeof(int)));
  FH_TRY(up((void**)&L.d_pcptr, L.vcolor_ptr.data(), L.vcolor_ptr.size() * sizeof(int)));
  L.pbar_len = 2 + 1024;
  FH_CHECK_HIP(hipMalloc(&L.d_pbar, L.pbar_len * sizeof(unsigned)));
  FH_CHECK_HIP(hipMemset(L.d_pbar, 0, L.pbar_len * sizeof(unsigned)));
  L.vanka_maxcolor = 0;
  for (int c = 0; c < ncol; c++) L.vanka_maxcolor = std::max(L.vanka_maxcolor, L.vcolor_ptr[c + 1] - L.vcolor_ptr[c]);
  FH_CHECK_HIP(hipMalloc(&L.d_pflag, (size_t)np * sizeof(int)));
  FH_CHECK_HIP(hipMalloc(&L.d_pinv, (size_t)L.h_poff[np] * sizeof(double)));
  if (sequential) {
    FH_CHECK_HIP(hipMalloc(&L.d_pscr, (size_t)L.h_poff[np] * sizeof(double)));
    FH_CHECK_HIP(hipMalloc(&L.d_pmask, (size_t)L.h_poff[np]));
  }
  L.order_kind = sequential ? 1 : 0;
  return 0;
}

// FH_SMOOTH_ASM: the sub-solve of a block is ONE application of ILU(0) of the block matrix in its natural (ascending dof) order with
// PCFactorSetZeroPivot(1e-16) and MAT_SHIFT_NONZERO (LinearEquationSolverPetscAsm.cpp:278-335): the block matrix A_pp in M is replaced by the
// product L~ U~ of its incomplete factors (restarted on A_pp + shift I, shift = 100 eps then doubled, when a pivot fails
// |u_kk| > 1e-16 sum_{j>k} |u_kj|), which the patch inversion then turns into the dense operator (L~ U~)^-1 the sweep applies.  One workgroup
// per block on global memory (setup); O: scratch of the same layout, mask: which entries of the block lie in the pattern of A.
__global__ __launch_bounds__(256) void k_patch_ilu0(const int* __restrict__ pptr, const int* __restrict__ pdofs, const int64_t* __restrict__ poff,
                                                    const int* __restrict__ rowptr, const int* __restrict__ col, double* __restrict__ M, double* __restrict__ O,
                                                    unsigned char* __restrict__ mask, int* __restrict__ flag, int first) {
  __shared__ double s_shift, s_piv;
  __shared__ int s_fail;
  const int p = blockIdx.x + first, tid = threadIdx.x;
  const int* d = pdofs + pptr[p];
  const int np = pptr[p + 1] - pptr[p];
  double* Mp = M + poff[p];
  double* Op = O + poff[p];
  unsigned char* mk = mask + poff[p];
  for (int t = tid; t < np * np; t += 256) {
    const int r = d[t / np], c = d[t % np];
    int lo = rowptr[r], hi = rowptr[r + 1] - 1, found = 0;
    while (lo <= hi) {
      const int mid = lo + ((hi - lo) >> 1);
      const int cc = col[mid];
      if (cc == c) { found = 1; break; }
      if (cc < c) lo = mid + 1; else hi = mid - 1;
    }
    mk[t] = (unsigned char)found;
    Op[t] = Mp[t];
  }
  if (tid == 0) s_shift = 0.0;
  __syncthreads();
  for (int attempt = 0; attempt < 64; attempt++) {
    const double shift = s_shift;
    for (int t = tid; t < np * np; t += 256) Mp[t] = Op[t] + ((t / np == t % np) ? shift : 0.0);
    if (tid == 0) s_fail = 0;
    __syncthreads();
    for (int k = 0; k < np; k++) {
      if (tid == 0) {
        const double piv = Mp[(size_t)k * np + k];
        double rs = 0.0;
        for (int j = k + 1; j < np; j++)
          if (mk[(size_t)k * np + j]) rs += fabs(Mp[(size_t)k * np + j]);
        if (!(fabs(piv) > 1e-16 * rs)) s_fail = 1;
        s_piv = piv;
      }
      __syncthreads();
      if (s_fail) break;
      const double piv = s_piv;
      for (int i = k + 1 + tid; i < np; i += 256)
        if (mk[(size_t)i * np + k]) Mp[(size_t)i * np + k] /= piv;
      __syncthreads();
      const int w = np - k - 1;
      for (int t = tid; t < w * w; t += 256) {
        const int i = k + 1 + t / w, j = k + 1 + t % w;
        if (mk[(size_t)i * np + k] && mk[(size_t)k * np + j] && mk[(size_t)i * np + j]) Mp[(size_t)i * np + j] -= Mp[(size_t)i * np + k] * Mp[(size_t)k * np + j];
      }
      __syncthreads();
    }
    if (!s_fail) break;
    __syncthreads();
    if (tid == 0) s_shift = shift == 0.0 ? 100.0 * 2.220446049250313e-16 : 2.0 * shift;
    __syncthreads();
  }
  if (s_fail) {
    if (tid == 0) flag[p] = 2;
    return;
  }
  // M <- L~ U~ (entries outside the pattern of the factors are zero, so the dense product needs no masks)
  for (int t = tid; t < np * np; t += 256) {
    const int i = t / np, j = t % np, kmax = i < j ? i : j;
    double a = 0.0;
    for (int k = 0; k <= kmax; k++) a += (k == i ? 1.0 : Mp[(size_t)i * np + k]) * Mp[(size_t)k * np + j];
    Op[t] = a;
  }
  __syncthreads();
  for (int t = tid; t < np * np; t += 256) Mp[t] = Op[t];
}

// numeric part of the smoother setup (every fh_mg_setup, i.e. every Newton iteration): extract and invert the patch matrices
static int factor_patches(fh_mg_t mg, MgLevel& L) {
  fh_ctx_t c = mg->ctx;
  FH_CHECK_HIP(hipMemsetAsync(L.d_pflag, 0, (size_t)L.npatch * sizeof(int), c->stream));
  hipLaunchKernelGGL(k_patch_extract, dim3(L.npatch), dim3(256), 0, c->stream, L.d_pptr, L.d_pdofs, L.d_poff, L.A->d_rowptr, L.A->d_col, L.A->d_val,
                     L.d_pinv);
  // (blocks below npatch_exact keep A_pp: their sub-solve is the exact one, the reference's MLU_PRECOND on the solid / porous blocks)
  if (L.smoother == FH_SMOOTH_ASM && L.npatch > L.npatch_exact)
    hipLaunchKernelGGL(k_patch_ilu0, dim3(L.npatch - L.npatch_exact), dim3(256), 0, c->stream, L.d_pptr, L.d_pdofs, L.d_poff, L.A->d_rowptr, L.A->d_col, L.d_pinv, L.d_pscr,
                       L.d_pmask, L.d_pflag, L.npatch_exact);
  // patches of at most PLDS_MAX dofs: one wave each with the matrix in LDS; the others (and everything with patch_invert_lds = 0): the
  // workgroup kernel on the matrix in global memory
  int nsmall = 0;
  for (int p = 0; p < L.npatch; p++) nsmall += (L.h_pptr[p + 1] - L.h_pptr[p] <= PLDS_MAX) ? 1 : 0;
  if (c->patch_invert_lds && nsmall > 0) {
    constexpr size_t lds_max = ((size_t)PLDS_MAX * (PLDS_MAX | 1) + PLDS_MAX) * sizeof(double) + PLDS_MAX * sizeof(int);
    static bool attr_set[64] = {};
    if (!attr_set[c->device & 63]) {
      FH_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_patch_invert_lds), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_max));
      attr_set[c->device & 63] = true;
    }
    int nmax = 1;                                   // the LDS a launch asks for follows the largest small patch of this level
    for (int p = 0; p < L.npatch; p++) {
      const int np = L.h_pptr[p + 1] - L.h_pptr[p];
      if (np <= PLDS_MAX) nmax = std::max(nmax, np);
    }
    const size_t lds = ((size_t)nmax * (nmax | 1) + nmax) * sizeof(double) + nmax * sizeof(int);
    hipLaunchKernelGGL(k_patch_invert_lds, dim3(L.npatch), dim3(64), lds, c->stream, L.d_pptr, L.d_poff, L.d_pinv, L.d_pflag, nmax);
  }
  if (!c->patch_invert_lds || nsmall < L.npatch)
    hipLaunchKernelGGL(k_patch_invert, dim3(L.npatch), dim3(256), 0, c->stream, L.d_pptr, L.d_poff, L.d_pinv, L.d_pflag,
                       c->patch_invert_lds ? PLDS_MAX : 0);
  FH_CHECK_HIP(hipGetLastError());
  std::vector<int> flag(L.npatch);
  FH_CHECK_HIP(hipMemcpyAsync(flag.data(), L.d_pflag, flag.size() * sizeof(int), hipMemcpyDeviceToHost, c->stream));
  FH_CHECK_HIP(hipStreamSynchronize(c->stream));
  for (int p = 0; p < L.npatch; p++)
    FH_REQUIRE(flag[p] == 0, flag[p] == 2 ? "ASM smoother: ILU(0) of block %d found no usable pivots within 64 shifts" : "Vanka smoother: the matrix of patch %d is singular", p);
  return 0;
}

// multiplicative Schwarz sweeps over the colours of the patches on A x = b (x updated in place; rwork: a residual vector)
static int vanka_apply(fh_mg_t mg, MgLevel& L, double* x, const double* b, double* rwork, double omega, int nsweeps) {
  fh_ctx_t c = mg->ctx;
  if (c->vanka_persistent && nsweeps > 0 && L.vanka_ncolors > 0) {
    // four waves and 4 * max_patch * 8 <= 16 KB of LDS per workgroup, at most one workgroup per CU: the whole grid is resident
    const int grid = std::max(1, std::min(fh_div_up(L.vanka_maxcolor, 4), c->num_cu));
    FH_REQUIRE(grid <= L.pbar_len - 2, "Vanka smoother: barrier buffer too small");
    const size_t lds = (size_t)4 * L.max_patch * sizeof(double);
    if (c->vanka_persistent == 1)
      hipLaunchKernelGGL(k_vanka_persistent<1>, dim3(grid), dim3(256), lds, c->stream, L.d_porder, L.d_pcptr, L.vanka_ncolors, nsweeps, L.d_pptr, L.d_pdofs,
                         L.d_poff, L.d_pinv, L.A->d_rowptr, L.A->d_col, L.A->d_val, b, x, omega, L.d_pbar, L.max_patch);
    else
      hipLaunchKernelGGL(k_vanka_persistent<2>, dim3(grid), dim3(256), lds, c->stream, L.d_porder, L.d_pcptr, L.vanka_ncolors, nsweeps, L.d_pptr, L.d_pdofs,
                         L.d_poff, L.d_pinv, L.A->d_rowptr, L.A->d_col, L.A->d_val, b, x, omega, L.d_pbar, L.max_patch);
    FH_CHECK_HIP(hipGetLastError());
    return 0;
  }
  for (int s = 0; s < nsweeps; s++)
    for (int k = 0; k < L.vanka_ncolors; k++) {
      const int np = L.vcolor_ptr[k + 1] - L.vcolor_ptr[k];
      if (np == 0) continue;
      if (c->vanka_fused) {
        hipLaunchKernelGGL(k_vanka_color_fused, dim3(np), dim3(256), (size_t)5 * L.max_patch * sizeof(double), c->stream, L.d_porder + L.vcolor_ptr[k], np, L.d_pptr,
                           L.d_pdesc, L.d_poff, L.d_pinv, L.A->d_col, L.A->d_val, b, x, omega, L.max_patch);
        continue;
      }
      FH_TRY(fh_dev_spmv(L.A, x, rwork, 2, b, nullptr, 0.0));                       // r = b - A x
      hipLaunchKernelGGL(k_vanka_color, dim3(np), dim3(64), (size_t)L.max_patch * sizeof(double), c->stream, L.d_porder + L.vcolor_ptr[k], np,
                         L.d_pptr, L.d_pdofs, L.d_poff, L.d_pinv, rwork, x, omega);
    }
  FH_CHECK_HIP(hipGetLastError());
  return 0;
}
static int vanka_sweeps(fh_mg_t mg, MgLevel& L, int nsweeps) { return vanka_apply(mg, L, L.x, L.b, L.r, L.omega, nsweeps); }


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
      FH_REQUIRE(L.npatch > 0 && !L.halo, "fh_mg_setup: level %d uses the block smoother but has no patches (fh_mg_set_level_patches)", l);
      const int kind = L.smoother == FH_SMOOTH_ASM ? 1 : 0;
      if (L.d_pinv && L.order_kind != kind) free_level_patch_setup(L);
      if (!L.d_pinv) FH_TRY(color_patches(L, kind == 1));
      FH_TRY(factor_patches(mg, L));
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

// Richardson(scale omega) + a sweep preconditioner: x <- x + omega * B (b - A x).  B = forward then backward Gauss-Seidel from a
// zero guess (PCSOR's local symmetric sweep, PetscPreconditioner.cpp:219-222) over the colours (FH_SMOOTH_GS_COLOR) or in the natural
// row order as PETSc runs it (FH_SMOOTH_SOR), or the ILU(0) solve (FH_SMOOTH_ILU0, PetscPreconditioner.cpp:91-115)
static int gs_sweeps(fh_mg_t mg, MgLevel& L, int nsweeps, bool zero_guess) {
  fh_ctx_t c = mg->ctx;
  for (int s = 0; s < nsweeps; s++) {
    const bool first = zero_guess && s == 0;
    if (first) {
      FH_CHECK_HIP(hipMemcpyAsync(L.r, L.b, (size_t)L.n * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
    } else {
      FH_TRY(halo_spmv(L.halo, L.A, L.x, L.n, L.r, 2, L.b, nullptr, 0.0));
    }
    double* z = L.x2;
    if (L.smoother == FH_SMOOTH_ASM) {
      // Richardson around PCASM: z = B r from zero (x2), the residual of the block sweep goes through dinv (unused by this smoother)
      FH_CHECK_HIP(hipMemsetAsync(z, 0, (size_t)L.ncols * sizeof(double), c->stream));
      FH_TRY(vanka_apply(mg, L, z, L.r, L.dinv, 1.0, 1));
      hipLaunchKernelGGL(k_axpby2, dim3(sgrid(c, L.n)), dim3(256), 0, c->stream, L.x, z, L.omega, first ? 0.0 : 1.0, L.n);
      continue;
    }
    if (L.smoother == FH_SMOOTH_SOR || L.smoother == FH_SMOOTH_ILU0 || L.smoother == FH_SMOOTH_LU) {
      // z = B r in the natural row order, as the reference's PCSOR / PCILU apply it (level-scheduled, fh_trisolve.hip); PCLU: z = A^-1 r
      if (L.smoother == FH_SMOOTH_SOR) FH_TRY(fh_tri_ssor_apply(L.tri, L.A, L.dinv, L.r, z));
      else if (L.smoother == FH_SMOOTH_LU) FH_TRY(fh_direct_solve_ptr(L.direct, L.r, z));
      else FH_TRY(fh_tri_ilu_apply(L.tri, L.A, L.r, z));
      hipLaunchKernelGGL(k_axpby2, dim3(sgrid(c, L.n)), dim3(256), 0, c->stream, L.x, z, L.omega, first ? 0.0 : 1.0, L.n);
      continue;
    }
    FH_TRY(gs_color_apply(mg, L, L.r, z));
    hipLaunchKernelGGL(k_axpby2, dim3(sgrid(c, L.n)), dim3(256), 0, c->stream, L.x, z, L.omega, first ? 0.0 : 1.0, L.n);
  }
  FH_CHECK_HIP(hipGetLastError());
  return 0;
}

__global__ __launch_bounds__(256) void k_scale_by(double* __restrict__ z, const double* __restrict__ r, const double* __restrict__ dinv, int n) {
  for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) z[i] = dinv[i] * r[i];
}

static int gs_color_apply(fh_mg_t mg, MgLevel& L, const double* r, double* z);

// z = B r with the level's sweep preconditioner
static int level_precond(fh_mg_t mg, MgLevel& L, const double* r, double* z) {
  fh_ctx_t c = mg->ctx;
  switch (L.smoother) {
    case FH_SMOOTH_SOR: return fh_tri_ssor_apply(L.tri, L.A, L.dinv, r, z);
    case FH_SMOOTH_ILU0: return fh_tri_ilu_apply(L.tri, L.A, r, z);
    case FH_SMOOTH_LU: return fh_direct_solve_ptr(L.direct, r, z);
    case FH_SMOOTH_GS_COLOR: return gs_color_apply(mg, L, r, z);
    case FH_SMOOTH_VANKA:
    case FH_SMOOTH_ASM:           // PCApply_ASM: the blocks in order on the residual of r with the corrections so far, from zero
      FH_CHECK_HIP(hipMemsetAsync(z, 0, (size_t)L.ncols * sizeof(double), c->stream));
      return vanka_apply(mg, L, z, r, L.x2, 1.0, 1);
    default:
      hipLaunchKernelGGL(k_scale_by, dim3(sgrid(c, L.n)), dim3(256), 0, c->stream, z, r, L.dinv, L.n);
      return 0;
  }
}

// the level as a Krylov solver sees it: operator with ghost refresh, sum over the ranks, sweep preconditioner
static KrylovOps level_ops(fh_mg_t mg, MgLevel& L) {
  KrylovOps op;
  op.ctx = mg->ctx;
  op.n = L.n;
  op.ncols = L.ncols;
  op.spmv = [&L](double* x, double* y, int mode, const double* b) { return halo_spmv(L.halo, L.A, x, L.n, y, mode, b, nullptr, 0.0); };
  op.allreduce = [&L](double* d, int count) { return L.halo ? fh_halo_allreduce_ptr(L.halo, d, count) : 0; };
  op.precond = [mg, &L](const double* in, double* out) { return level_precond(mg, L, in, out); };
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
    return vanka_sweeps(mg, L, nits);
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

extern "C" int fh_mg_destroy(fh_mg_t mg) {
  if (!mg) return 0;
  hipStreamSynchronize(mg->ctx->stream);
  if (mg->gexec) hipGraphExecDestroy(mg->gexec);
  if (mg->graph) hipGraphDestroy(mg->graph);
  for (auto& L : mg->lv) {
    free_level_buffers(L);
    free_level_colors(L);
    free_level_patches(L);
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
