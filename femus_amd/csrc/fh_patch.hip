// The block Schwarz smoothers of a multigrid level on gfx950, FH_SMOOTH_VANKA and FH_SMOOTH_ASM.  The multigrid (fh_mg.hip) sees the functions
// of fh_patch.h and nothing of the state.
//
// block Schwarz (Vanka) smoother for saddle-point systems: x_p += omega A_pp^-1 (b - A x)_p for every patch p, patches of one
// colour concurrently (patches of a colour neither share a dof nor read one another's dofs, so the order inside a colour is
// irrelevant), colours in sequence = multiplicative Schwarz.  GPU form of the element-block ASM smoother the reference
// selects with FEMuS_ASM (petsc_asm/LinearEquationSolverPetscAsm.cpp:91-345).
//
// FH_SMOOTH_ASM (PCASM as the reference configures it, LinearEquationSolverPetscAsm.cpp:278-335): the blocks keep their INDEX ORDER, as PCASM's
// multiplicative composition visits them (dependency levels in place of colours), the sub-solve of a block is one application of ILU(0) of the
// block matrix, and the first npatch_exact blocks get the EXACT sub-solve (MLU_PRECOND on the solid / porous blocks, :298-307).  Both smoothers
// share every kernel of the sweep: the block operator, whichever it is, is a dense inverse made at setup.
#include "fh_patch.h"
#include <algorithm>

// ------------------------------------------------------------------------------------------------
// kernels
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

// ------------------------------------------------------------------------------------------------
// state
// ------------------------------------------------------------------------------------------------
struct PatchSmoother {
  // the patch lists: set by fh_patch_set, independent of the matrix
  int npatch = 0, max_patch = 0;
  int npatch_exact = 0;       // FH_SMOOTH_ASM: the first npatch_exact blocks get the EXACT sub-solve (MLU_PRECOND on the solid / porous blocks, LinearEquationSolverPetscAsm.cpp:298-307)
  std::vector<int> h_pptr, h_pdofs;
  std::vector<int64_t> h_poff;
  // the setup: made for one matrix pattern by color_patches (d_pinv != nullptr: it exists), dropped by drop_setup
  int vanka_ncolors = 0;
  std::vector<int> vcolor_ptr;
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
};

void fh_patch_drop_setup(PatchSmoother* ps) {
  if (!ps) return;
  PatchSmoother& S = *ps;
  for (void** q : {(void**)&S.d_pptr, (void**)&S.d_pdofs, (void**)&S.d_porder, (void**)&S.d_pflag, (void**)&S.d_poff, (void**)&S.d_pinv, (void**)&S.d_pcptr,
                   (void**)&S.d_pbar, (void**)&S.d_pscr, (void**)&S.d_pmask, (void**)&S.d_pdesc})
    if (*q) {
      hipFree(*q);
      *q = nullptr;
    }
  S.vanka_ncolors = 0;
}

void fh_patch_destroy(PatchSmoother* ps) {
  fh_patch_drop_setup(ps);
  delete ps;
}

int fh_patch_count(const PatchSmoother* ps) { return ps ? ps->npatch : 0; }

int fh_patch_set(PatchSmoother** ps, int npatch, const int* ptr, const int* dofs) {
  // checked on a copy: a list that is refused leaves the patches of the level as they were
  for (int p = 0; p < npatch; p++) {
    const int np = ptr[p + 1] - ptr[p];
    FH_REQUIRE(np > 0 && np <= 512, "fh_mg_set_level_patches: patch %d has %d dofs (1..512 supported)", p, np);
  }
  // every patch in ASCENDING dof order, whatever order the caller gave it in: the order PCASM's index sets have (the reference sorts every block before
  // ISCreateGeneral, LinearEquationSolverPetscAsm.cpp:253-254) and the one ILU(0) of a block is defined in; the Vanka sweep does not depend on it beyond
  // rounding.  A dof listed twice would give x[d] two writers in one patch and two equal rows in its matrix
  std::vector<int> sorted(dofs + ptr[0], dofs + ptr[npatch]);
  for (int p = 0; p < npatch; p++) {
    auto b = sorted.begin() + (ptr[p] - ptr[0]), e = sorted.begin() + (ptr[p + 1] - ptr[0]);
    std::sort(b, e);
    auto dup = std::adjacent_find(b, e);
    FH_REQUIRE(dup == e, "fh_mg_set_level_patches: patch %d lists dof %d twice", p, dup == e ? 0 : *dup);
  }
  if (!*ps) *ps = new PatchSmoother();
  PatchSmoother& S = **ps;
  fh_patch_drop_setup(&S);
  S.npatch = npatch;
  S.h_pptr.resize(npatch + 1);
  for (int p = 0; p <= npatch; p++) S.h_pptr[p] = ptr[p] - ptr[0];
  S.h_pdofs.swap(sorted);
  S.h_poff.assign(npatch + 1, 0);
  S.max_patch = 0;
  for (int p = 0; p < npatch; p++) {
    const int np = S.h_pptr[p + 1] - S.h_pptr[p];
    S.max_patch = std::max(S.max_patch, np);
    S.h_poff[p + 1] = S.h_poff[p] + (int64_t)np * np;
  }
  S.npatch_exact = 0;
  return 0;
}

int fh_patch_set_exact(PatchSmoother* ps, int nfirst) {
  FH_REQUIRE(nfirst >= 0 && nfirst <= fh_patch_count(ps), "fh_mg_set_level_patches_exact: %d of %d blocks", nfirst, fh_patch_count(ps));
  if (ps) ps->npatch_exact = nfirst;
  return 0;
}

void fh_patch_signature(const PatchSmoother* ps, std::vector<uint64_t>& w) {
  w.push_back(ps ? (uint64_t)ps->npatch_exact : 0);
  w.push_back((uint64_t)(uintptr_t)(ps ? ps->d_pinv : nullptr));
  w.push_back((uint64_t)(uintptr_t)(ps ? ps->d_porder : nullptr));
  w.push_back(ps ? (uint64_t)ps->vanka_ncolors : 0);
}

// ------------------------------------------------------------------------------------------------
// setup
// ------------------------------------------------------------------------------------------------
// greedy colouring in patch order; two patches conflict when a dof of one appears in the matrix rows of the other
// sequential = false: greedy colours (patches of a colour neither share nor read each other's dofs; colours in any order -- the Vanka smoother).
// sequential = true (FH_SMOOTH_ASM): the blocks keep their INDEX ORDER, as PCASM's multiplicative composition visits them: block p gets the
// dependency level 1 + max level of the earlier blocks it conflicts with, so a level holds blocks whose order among themselves does not matter and
// the levels, run one after the other, give exactly the sequential sweep (level scheduling, as for the natural-order SOR / ILU sweeps)
static int color_patches(PatchSmoother& S, fh_mat_t A, bool sequential) {
  const int n = A->m, np = S.npatch;
  const std::vector<int>&rp = A->h_rowptr, &cl = fh_hcol(A);
  for (int d : S.h_pdofs) FH_REQUIRE(d >= 0 && d < n, "Vanka smoother: patch dof %d out of range", d);
  std::vector<int> optr(n + 1, 0), rptr(n + 1, 0);
  std::vector<std::vector<int>> reads(np);
  std::vector<int> mark(n, -1);
  for (int p = 0; p < np; p++) {
    for (int q = S.h_pptr[p]; q < S.h_pptr[p + 1]; q++) {
      const int r = S.h_pdofs[q];
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
    for (int q = S.h_pptr[p]; q < S.h_pptr[p + 1]; q++) owner[oc[S.h_pdofs[q]]++] = p;
    for (int c : reads[p]) reader[rc[c]++] = p;
  }
  std::vector<int> color(np, -1), used;
  int ncol = 0;
  for (int p = 0; p < np; p++) {
    used.assign(ncol + 1, 0);
    for (int c : reads[p])
      for (int k = optr[c]; k < optr[c + 1]; k++)
        if (color[owner[k]] >= 0) used[color[owner[k]]] = 1;
    for (int q = S.h_pptr[p]; q < S.h_pptr[p + 1]; q++) {
      const int d = S.h_pdofs[q];
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
  S.vanka_ncolors = ncol;
  S.vcolor_ptr.assign(ncol + 1, 0);
  for (int p = 0; p < np; p++) S.vcolor_ptr[color[p] + 1]++;
  for (int c = 0; c < ncol; c++) S.vcolor_ptr[c + 1] += S.vcolor_ptr[c];
  std::vector<int> order(np), pos(S.vcolor_ptr.begin(), S.vcolor_ptr.end() - 1);
  for (int p = 0; p < np; p++) order[pos[color[p]]++] = p;
  auto up = [&](void** d, const void* h, size_t bytes) -> int {
    FH_CHECK_HIP(hipMalloc(d, bytes ? bytes : 8));
    if (bytes) FH_CHECK_HIP(hipMemcpy(*d, h, bytes, hipMemcpyHostToDevice));
    return 0;
  };
  FH_TRY(up((void**)&S.d_pptr, S.h_pptr.data(), S.h_pptr.size() * sizeof(int)));
  FH_TRY(up((void**)&S.d_pdofs, S.h_pdofs.data(), S.h_pdofs.size() * sizeof(int)));
  FH_CHECK_HIP(hipMalloc(&S.d_pdesc, std::max<size_t>(S.h_pdofs.size(), 1) * sizeof(int4)));
  hipLaunchKernelGGL(k_patch_desc, dim3(fh_div_up((int64_t)S.h_pdofs.size(), 256)), dim3(256), 0, A->ctx->stream, (int)S.h_pdofs.size(), S.d_pdofs, A->d_rowptr, S.d_pdesc);
  FH_CHECK_HIP(hipGetLastError());
  FH_TRY(up((void**)&S.d_poff, S.h_poff.data(), S.h_poff.size() * sizeof(int64_t)));
  FH_TRY(up((void**)&S.d_porder, order.data(), order.size() * sizeof(int)));
  FH_TRY(up((void**)&S.d_pcptr, S.vcolor_ptr.data(), S.vcolor_ptr.size() * sizeof(int)));
  S.pbar_len = 2 + 1024;
  FH_CHECK_HIP(hipMalloc(&S.d_pbar, S.pbar_len * sizeof(unsigned)));
  FH_CHECK_HIP(hipMemset(S.d_pbar, 0, S.pbar_len * sizeof(unsigned)));
  S.vanka_maxcolor = 0;
  for (int c = 0; c < ncol; c++) S.vanka_maxcolor = std::max(S.vanka_maxcolor, S.vcolor_ptr[c + 1] - S.vcolor_ptr[c]);
  FH_CHECK_HIP(hipMalloc(&S.d_pflag, (size_t)np * sizeof(int)));
  FH_CHECK_HIP(hipMalloc(&S.d_pinv, (size_t)S.h_poff[np] * sizeof(double)));
  if (sequential) {
    FH_CHECK_HIP(hipMalloc(&S.d_pscr, (size_t)S.h_poff[np] * sizeof(double)));
    FH_CHECK_HIP(hipMalloc(&S.d_pmask, (size_t)S.h_poff[np]));
  }
  S.order_kind = sequential ? 1 : 0;
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
static int factor_patches(PatchSmoother& S, fh_ctx_t c, fh_mat_t A, int kind) {
  FH_CHECK_HIP(hipMemsetAsync(S.d_pflag, 0, (size_t)S.npatch * sizeof(int), c->stream));
  hipLaunchKernelGGL(k_patch_extract, dim3(S.npatch), dim3(256), 0, c->stream, S.d_pptr, S.d_pdofs, S.d_poff, A->d_rowptr, A->d_col, A->d_val,
                     S.d_pinv);
  // (blocks below npatch_exact keep A_pp: their sub-solve is the exact one, the reference's MLU_PRECOND on the solid / porous blocks)
  if (kind == 1 && S.npatch > S.npatch_exact)
    hipLaunchKernelGGL(k_patch_ilu0, dim3(S.npatch - S.npatch_exact), dim3(256), 0, c->stream, S.d_pptr, S.d_pdofs, S.d_poff, A->d_rowptr, A->d_col, S.d_pinv, S.d_pscr,
                       S.d_pmask, S.d_pflag, S.npatch_exact);
  // patches of at most PLDS_MAX dofs: one wave each with the matrix in LDS; the others (and everything with patch_invert_lds = 0): the
  // workgroup kernel on the matrix in global memory
  int nsmall = 0;
  for (int p = 0; p < S.npatch; p++) nsmall += (S.h_pptr[p + 1] - S.h_pptr[p] <= PLDS_MAX) ? 1 : 0;
  if (c->patch_invert_lds && nsmall > 0) {
    constexpr size_t lds_max = ((size_t)PLDS_MAX * (PLDS_MAX | 1) + PLDS_MAX) * sizeof(double) + PLDS_MAX * sizeof(int);
    static bool attr_set[64] = {};
    if (!attr_set[c->device & 63]) {
      FH_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_patch_invert_lds), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_max));
      attr_set[c->device & 63] = true;
    }
    int nmax = 1;                                   // the LDS a launch asks for follows the largest small patch of this level
    for (int p = 0; p < S.npatch; p++) {
      const int np = S.h_pptr[p + 1] - S.h_pptr[p];
      if (np <= PLDS_MAX) nmax = std::max(nmax, np);
    }
    const size_t lds = ((size_t)nmax * (nmax | 1) + nmax) * sizeof(double) + nmax * sizeof(int);
    hipLaunchKernelGGL(k_patch_invert_lds, dim3(S.npatch), dim3(64), lds, c->stream, S.d_pptr, S.d_poff, S.d_pinv, S.d_pflag, nmax);
  }
  if (!c->patch_invert_lds || nsmall < S.npatch)
    hipLaunchKernelGGL(k_patch_invert, dim3(S.npatch), dim3(256), 0, c->stream, S.d_pptr, S.d_poff, S.d_pinv, S.d_pflag,
                       c->patch_invert_lds ? PLDS_MAX : 0);
  FH_CHECK_HIP(hipGetLastError());
  std::vector<int> flag(S.npatch);
  FH_CHECK_HIP(hipMemcpyAsync(flag.data(), S.d_pflag, flag.size() * sizeof(int), hipMemcpyDeviceToHost, c->stream));
  FH_CHECK_HIP(hipStreamSynchronize(c->stream));
  for (int p = 0; p < S.npatch; p++)
    FH_REQUIRE(flag[p] == 0, flag[p] == 2 ? "ASM smoother: ILU(0) of block %d found no usable pivots within 64 shifts" : "Vanka smoother: the matrix of patch %d is singular", p);
  return 0;
}

int fh_patch_setup(PatchSmoother* ps, fh_ctx_t ctx, fh_mat_t A, int kind) {
  FH_REQUIRE(ps && ps->npatch > 0 && ctx && A, "fh_patch_setup: no patches");
  PatchSmoother& S = *ps;
  if (S.d_pinv && S.order_kind != kind) fh_patch_drop_setup(ps);
  if (!S.d_pinv) FH_TRY(color_patches(S, A, kind == 1));
  return factor_patches(S, ctx, A, kind);
}

// ------------------------------------------------------------------------------------------------
// sweep
// ------------------------------------------------------------------------------------------------
int fh_patch_apply(PatchSmoother* ps, fh_ctx_t c, fh_mat_t A, double* x, const double* b, double* rwork, double omega, int nsweeps) {
  FH_REQUIRE(ps && ps->d_pinv, "fh_patch_apply: fh_patch_setup has not been called");
  PatchSmoother& S = *ps;
  if (c->vanka_persistent && nsweeps > 0 && S.vanka_ncolors > 0) {
    // four waves and 4 * max_patch * 8 <= 16 KB of LDS per workgroup, at most one workgroup per CU: the whole grid is resident
    const int grid = std::max(1, std::min(fh_div_up(S.vanka_maxcolor, 4), c->num_cu));
    FH_REQUIRE(grid <= S.pbar_len - 2, "Vanka smoother: barrier buffer too small");
    const size_t lds = (size_t)4 * S.max_patch * sizeof(double);
    if (c->vanka_persistent == 1)
      hipLaunchKernelGGL(k_vanka_persistent<1>, dim3(grid), dim3(256), lds, c->stream, S.d_porder, S.d_pcptr, S.vanka_ncolors, nsweeps, S.d_pptr, S.d_pdofs,
                         S.d_poff, S.d_pinv, A->d_rowptr, A->d_col, A->d_val, b, x, omega, S.d_pbar, S.max_patch);
    else
      hipLaunchKernelGGL(k_vanka_persistent<2>, dim3(grid), dim3(256), lds, c->stream, S.d_porder, S.d_pcptr, S.vanka_ncolors, nsweeps, S.d_pptr, S.d_pdofs,
                         S.d_poff, S.d_pinv, A->d_rowptr, A->d_col, A->d_val, b, x, omega, S.d_pbar, S.max_patch);
    FH_CHECK_HIP(hipGetLastError());
    return 0;
  }
  for (int s = 0; s < nsweeps; s++)
    for (int k = 0; k < S.vanka_ncolors; k++) {
      const int np = S.vcolor_ptr[k + 1] - S.vcolor_ptr[k];
      if (np == 0) continue;
      if (c->vanka_fused) {
        hipLaunchKernelGGL(k_vanka_color_fused, dim3(np), dim3(256), (size_t)5 * S.max_patch * sizeof(double), c->stream, S.d_porder + S.vcolor_ptr[k], np, S.d_pptr,
                           S.d_pdesc, S.d_poff, S.d_pinv, A->d_col, A->d_val, b, x, omega, S.max_patch);
        continue;
      }
      FH_TRY(fh_dev_spmv(A, x, rwork, 2, b, nullptr, 0.0));                       // r = b - A x
      hipLaunchKernelGGL(k_vanka_color, dim3(np), dim3(64), (size_t)S.max_patch * sizeof(double), c->stream, S.d_porder + S.vcolor_ptr[k], np,
                         S.d_pptr, S.d_pdofs, S.d_poff, S.d_pinv, rwork, x, omega);
    }
  FH_CHECK_HIP(hipGetLastError());
  return 0;
}
