// The exact solve of the coarsest multigrid level on gfx950: x = A_0^-1 b (the reference's PREONLY + LU on level 0, LinearEquationSolverPetsc.hpp:131-134).
// Unknowns coupled to nothing are solved by their diagonal; the others by the sparse exact solve (fh_direct.hip), by the block form of their
// nested dissection (block inverses + separator Schur complement) or by one dense inverse that a GEMV applies in the cycle.  The multigrid
// (fh_mg.hip) sees the functions of fh_coarse.h and nothing of the state.
#include "fh_coarse.h"
#include <algorithm>
#include <memory>
#include <cmath>

// y = Ainv b, one wave per row, 16-byte loads
__global__ __launch_bounds__(256) void k_dense_gemv(const double* __restrict__ M, const double* __restrict__ b, double* __restrict__ y, int n) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= n) return;
  const double* m = M + (size_t)row * n;
  double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;          // four loads of the row in flight per lane
  int k = lane;
  for (; k + 192 < n; k += 256) {
    a0 += m[k] * b[k];
    a1 += m[k + 64] * b[k + 64];
    a2 += m[k + 128] * b[k + 128];
    a3 += m[k + 192] * b[k + 192];
  }
  for (; k < n; k += 64) a0 += m[k] * b[k];
  double acc = (a0 + a1) + (a2 + a3);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
  if (lane == 0) y[row] = acc;
}

__global__ __launch_bounds__(256) void k_csr_to_dense(const int* __restrict__ rowptr, const int* __restrict__ col, const double* __restrict__ val,
                                                      double* __restrict__ D, int n) {
  const int row = blockIdx.x;
  for (int k = rowptr[row] + threadIdx.x; k < rowptr[row + 1]; k += 256) D[(size_t)row * n + col[k]] = val[k];
}

// ------------------------------------------------------------------------------------------------
// dense inverse of the coarsest operator: BLOCKED in-place Gauss-Jordan without pivoting (the operator is SPD on the free
// dofs and the identity on Dirichlet rows).  Per pivot block of NB columns: save the column panel, invert the NB x NB pivot
// in LDS, form the new row panel D^-1 A[k,:], rank-NB update of all other rows as a tiled FP64 GEMM (64x64 tiles, 4x4
// register blocks, operands staged in LDS), and the pivot-column panel -C D^-1.  2 n^3 flops in n/NB steps of 5 launches
// instead of 3 n launches of rank-1 updates.
// ------------------------------------------------------------------------------------------------
constexpr int GJ_NB = 32;   // pivot block (64 measured slower twice, also with the MFMA update: pivot-block inversion 34 -> 192 us, row panel 38 -> 144 us per step)
constexpr int GJ_KS = 32;   // K slice of the update staged in LDS at a time

// in-place inverse of the NB x NB block M (LDS, row stride NB + 1; rows / columns >= nb are identity padding) by Gauss-Jordan with
// PARTIAL PIVOTING, all 256 threads of the workgroup.  The inverse of a block does not depend on how it is computed, so the
// callers (general and symmetric sweeps) are unchanged; what pivoting buys is a stable inverse of blocks that are not positive
// definite -- saddle-point operators carry zero diagonal entries (the reference factors level 0 with a pivoted LU,
// LinearEquationSolverPetsc.hpp:131-134).  A pivot column without any entry above 1e-300 raises *flag (singular block).
__device__ __forceinline__ void gj_invert_block(double (*M)[GJ_NB + 1], double* colk, int* piv, int nb, int tid, int* flag) {
  for (int k = 0; k < nb; k++) {
    if (tid < 64) {            // wave 0: largest |M[i][k]|, i in [k, nb), smallest index on ties
      double v = (tid >= k && tid < nb) ? fabs(M[tid][k]) : -1.0;
      int idx = tid;
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) {
        const double v2 = __shfl_xor(v, off, 64);
        const int i2 = __shfl_xor(idx, off, 64);
        if (v2 > v || (v2 == v && i2 < idx)) {
          v = v2;
          idx = i2;
        }
      }
      if (tid == 0) {
        piv[k] = idx;
        if (!(v > 1e-300)) atomicOr(flag, 1);
      }
    }
    __syncthreads();
    const int pr = piv[k];
    if (pr != k && tid < GJ_NB) {
      const double t = M[k][tid];
      M[k][tid] = M[pr][tid];
      M[pr][tid] = t;
    }
    __syncthreads();
    if (tid < GJ_NB) colk[tid] = M[tid][k];
    __syncthreads();
    const double p = 1.0 / colk[k];
#pragma unroll
    for (int idx = tid; idx < GJ_NB * GJ_NB; idx += 256) {
      const int i = idx / GJ_NB, j = idx % GJ_NB;
      if (i != k) {
        const double f = colk[i] * p;
        M[i][j] = (j == k) ? -f : M[i][j] - f * M[k][j];
      }
    }
    __syncthreads();
    if (tid < GJ_NB) M[k][tid] = (tid == k) ? p : M[k][tid] * p;
    __syncthreads();
  }
  for (int k = nb - 1; k >= 0; k--) {      // the row interchanges come back as column interchanges, last first
    const int pr = piv[k];
    if (pr != k && tid < GJ_NB) {
      const double t = M[tid][k];
      M[tid][k] = M[tid][pr];
      M[tid][pr] = t;
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(256) void k_check_finite(const double* __restrict__ D, size_t n, int* __restrict__ flag) {
  bool bad = false;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) bad |= !isfinite(D[i]);
  if (__any(bad) && (threadIdx.x & 63) == 0) atomicOr(flag, 2);
}

__global__ __launch_bounds__(256) void k_gjb_save_panel(const double* __restrict__ D, double* __restrict__ Cp, double* __restrict__ CpT, int n, int kb, int nb) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= n * nb) return;
  const int i = idx / nb, t = idx % nb;
  const double v = D[(size_t)i * n + kb + t];
  Cp[(size_t)i * GJ_NB + t] = v;
  CpT[(size_t)t * n + i] = v;
}

// one workgroup; a single-wave version (no workgroup barriers) was measured 3x slower: 16 LDS read-modify-writes per lane and step
// instead of 4.  Index arithmetic on the compile-time block size (the run-time nb only guards).
__global__ __launch_bounds__(256) void k_gjb_pivot(const double* __restrict__ D, double* __restrict__ Dinv, int n, int kb, int nb, int* __restrict__ flag) {
  __shared__ double M[GJ_NB][GJ_NB + 1];
  __shared__ double colk[GJ_NB];
  __shared__ int piv[GJ_NB];
  const int tid = threadIdx.x;
  for (int idx = tid; idx < GJ_NB * GJ_NB; idx += 256) {
    const int i = idx / GJ_NB, j = idx % GJ_NB;
    M[i][j] = (i < nb && j < nb) ? D[(size_t)(kb + i) * n + kb + j] : (i == j ? 1.0 : 0.0);   // identity padding: inert
  }
  __syncthreads();
  gj_invert_block(M, colk, piv, nb, tid, flag);
  for (int idx = tid; idx < nb * nb; idx += 256) Dinv[(idx / nb) * GJ_NB + idx % nb] = M[idx / nb][idx % nb];
}

// rows of the pivot block: A[kb+s, j] <- sum_t Dinv[s,t] * A_old[kb+t, j] (j outside the pivot columns), Dinv inside
__global__ __launch_bounds__(64) void k_gjb_row_panel(double* __restrict__ D, const double* __restrict__ Dinv, const double* __restrict__ Cp,
                                                      int n, int kb, int nb) {
  __shared__ double Ds[GJ_NB][GJ_NB + 1];
  const int tid = threadIdx.x;
  for (int idx = tid; idx < GJ_NB * GJ_NB; idx += 64) {
    const int a = idx / GJ_NB, b = idx % GJ_NB;
    Ds[a][b] = (a < nb && b < nb) ? Dinv[a * GJ_NB + b] : 0.0;
  }
  __syncthreads();
  const int j = blockIdx.x * 64 + tid;
  if (j >= n) return;
  if (j >= kb && j < kb + nb) {
    for (int s2 = 0; s2 < nb; s2++) D[(size_t)(kb + s2) * n + j] = Ds[s2][j - kb];
    return;
  }
  double old[GJ_NB];        // compile-time trip counts: with the run-time bound nb the array lived in scratch memory
#pragma unroll
  for (int t = 0; t < GJ_NB; t++) old[t] = (t < nb) ? D[(size_t)(kb + t) * n + j] : 0.0;
  for (int s2 = 0; s2 < nb; s2++) {
    double acc = 0.0;
#pragma unroll
    for (int t = 0; t < GJ_NB; t++) acc += Ds[s2][t] * old[t];
    D[(size_t)(kb + s2) * n + j] = acc;
  }
}

// all other rows, columns outside the pivot block: A[i,j] -= sum_t Cp[i,t] * R[t,j]   (R = the new row panel)
__global__ __launch_bounds__(256) void k_gjb_update(double* __restrict__ D, const double* __restrict__ Cp, int n, int kb, int nb) {
  __shared__ double Cs[64][GJ_KS + 1];
  __shared__ double Rs[GJ_KS][64 + 2];
  const int tid = threadIdx.x;
  const int ti = blockIdx.y * 64, tj = blockIdx.x * 64;
  const int ty = tid >> 4, tx = tid & 15;
  double acc[4][4];
#pragma unroll
  for (int a = 0; a < 4; a++)
#pragma unroll
    for (int b2 = 0; b2 < 4; b2++) acc[a][b2] = 0.0;
  for (int t0 = 0; t0 < nb; t0 += GJ_KS) {
    for (int idx = tid; idx < 64 * GJ_KS; idx += 256) {
      const int r = idx / GJ_KS, t = t0 + idx % GJ_KS;
      const int i = ti + r;
      Cs[r][idx % GJ_KS] = (i < n && t < nb) ? Cp[(size_t)i * GJ_NB + t] : 0.0;
    }
    for (int idx = tid; idx < GJ_KS * 64; idx += 256) {
      const int t = t0 + idx / 64, c = idx % 64;
      const int j = tj + c;
      Rs[idx / 64][c] = (j < n && t < nb) ? D[(size_t)(kb + t) * n + j] : 0.0;
    }
    __syncthreads();
#pragma unroll 8
    for (int t = 0; t < GJ_KS; t++) {
      double cv[4], rv[4];
#pragma unroll
      for (int a = 0; a < 4; a++) cv[a] = Cs[ty * 4 + a][t];
#pragma unroll
      for (int b2 = 0; b2 < 4; b2++) rv[b2] = Rs[t][tx * 4 + b2];
#pragma unroll
      for (int a = 0; a < 4; a++)
#pragma unroll
        for (int b2 = 0; b2 < 4; b2++) acc[a][b2] += cv[a] * rv[b2];
    }
    __syncthreads();
  }
#pragma unroll
  for (int a = 0; a < 4; a++) {
    const int i = ti + ty * 4 + a;
    if (i >= n || (i >= kb && i < kb + nb)) continue;
#pragma unroll
    for (int b2 = 0; b2 < 4; b2++) {
      const int j = tj + tx * 4 + b2;
      if (j >= n || (j >= kb && j < kb + nb)) continue;
      D[(size_t)i * n + j] -= acc[a][b2];
    }
  }
}

// the same update on the FP64 matrix cores (v_mfma_f64_16x16x4): 64 x 64 output tile per workgroup, 32 x 32 per wave as 2 x 2
// MFMA tiles, K slices of 32 staged in LDS k-major (row stride 80 doubles = 16 mod 32: conflict-free fragment reads; A fragment:
// lane = 16 k + i, B fragment: lane = 16 k + j, C: col = lane & 15, row = (lane >> 4) + 4 reg).  CpT = the saved column panel
// transposed (t-major), so that both operands load coalesced.
typedef double gj_d4 __attribute__((ext_vector_type(4)));
__global__ __launch_bounds__(256) void k_gjb_update_mfma(double* __restrict__ D, const double* __restrict__ CpT, int n, int kb, int nb) {
  constexpr int LD = 80;
  __shared__ double Cs[GJ_KS][LD], Rs[GJ_KS][LD];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int ti = blockIdx.y * 64, tj = blockIdx.x * 64;
  const int wi = (wave >> 1) * 32, wj = (wave & 1) * 32;
  const int kk = lane >> 4, li = lane & 15;
  // the tile of D this workgroup updates is read FIRST (its HBM latency then overlaps the operand staging and the MFMAs) and
  // serves as the accumulator: D - Cp R = D + (-Cp) R, the sign goes onto the A operand
  gj_d4 acc[2][2];
  bool live[2][4][2];
#pragma unroll
  for (int a = 0; a < 2; a++)
#pragma unroll
    for (int r = 0; r < 4; r++) {
      const int i = ti + wi + a * 16 + kk + 4 * r;
#pragma unroll
      for (int b = 0; b < 2; b++) {
        const int j = tj + wj + b * 16 + li;
        live[a][r][b] = i < n && j < n && !(i >= kb && i < kb + nb) && !(j >= kb && j < kb + nb);
        acc[a][b][r] = live[a][r][b] ? D[(size_t)i * n + j] : 0.0;
      }
    }
  for (int t0 = 0; t0 < nb; t0 += GJ_KS) {
    for (int idx = tid; idx < GJ_KS * 64; idx += 256) {
      const int k = idx >> 6, c = idx & 63, t = t0 + k;
      Cs[k][c] = (ti + c < n && t < nb) ? -CpT[(size_t)t * n + ti + c] : 0.0;
      Rs[k][c] = (tj + c < n && t < nb) ? D[(size_t)(kb + t) * n + tj + c] : 0.0;
    }
    __syncthreads();
#pragma unroll
    for (int k0 = 0; k0 < GJ_KS; k0 += 4) {
      const double a0 = Cs[k0 + kk][wi + li], a1 = Cs[k0 + kk][wi + 16 + li];
      const double b0 = Rs[k0 + kk][wj + li], b1 = Rs[k0 + kk][wj + 16 + li];
      acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc[0][0], 0, 0, 0);
      acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, acc[0][1], 0, 0, 0);
      acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, acc[1][0], 0, 0, 0);
      acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc[1][1], 0, 0, 0);
    }
    __syncthreads();
  }
#pragma unroll
  for (int a = 0; a < 2; a++)
#pragma unroll
    for (int r = 0; r < 4; r++) {
      const int i = ti + wi + a * 16 + kk + 4 * r;
#pragma unroll
      for (int b = 0; b < 2; b++) {
        const int j = tj + wj + b * 16 + li;
        if (live[a][r][b]) D[(size_t)i * n + j] = acc[a][b][r];
      }
    }
}

// ------------------------------------------------------------------------------------------------
// SYMMETRIC coarse operators (Poisson, AMR: checked entry by entry before use): the sweep operator on pivot blocks,
//   A_kk <- -A_kk^-1,   A_ko <- A_kk^-1 A_ko (and its transpose),   A_oo <- A_oo - A_ok A_kk^-1 A_ko,
// keeps the working matrix symmetric through all steps and ends in -A^-1, so only the UPPER block triangle is updated: half the
// flops and half the HBM traffic of the general Gauss-Jordan above.  PT = the old pivot rows for ALL columns (taken from the
// rows right of the pivot block and from the columns above it), RT = the new row panel, both k-major for the MFMA fragments.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_csr_symmetry(const int* __restrict__ rowptr, const int* __restrict__ col, const double* __restrict__ val, int n,
                                                      double tol, int* __restrict__ flag) {
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;     // one wave per row
  if (i >= n) return;
  double dmax = 0.0;
  for (int k = rowptr[i] + lane; k < rowptr[i + 1]; k += 64) dmax = fmax(dmax, fabs(val[k]));
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) dmax = fmax(dmax, __shfl_xor(dmax, off, 64));
  for (int k = rowptr[i] + lane; k < rowptr[i + 1]; k += 64) {
    const int j = col[k];
    if (j == i) continue;
    int lo = rowptr[j], hi = rowptr[j + 1] - 1;
    double vt = 0.0;
    while (lo <= hi) {
      const int mid = lo + ((hi - lo) >> 1);   // (lo + hi) overflows beyond 2^30 non-zeros
      if (col[mid] == i) { vt = val[mid]; break; }
      if (col[mid] < i) lo = mid + 1; else hi = mid - 1;
    }
    if (fabs(val[k] - vt) > tol * dmax) atomicOr(flag, 1);
  }
}

__global__ __launch_bounds__(256) void k_gjs_gather_panel(const double* __restrict__ D, double* __restrict__ PT, int n, int kb, int nb) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= n * GJ_NB) return;
  const int j = idx / GJ_NB, t = idx % GJ_NB;            // t fastest: for j < kb the 32 entries D[j][kb..] are contiguous
  if (t >= nb) return;
  double v;
  if (j < kb) v = D[(size_t)j * n + kb + t];             // column above the pivot block (upper triangle)
  else if (j < kb + nb) v = D[(size_t)(kb + min(t, j - kb)) * n + kb + max(t, j - kb)];
  else v = D[(size_t)(kb + t) * n + j];                  // row right of the pivot block
  PT[(size_t)t * n + j] = v;
}

__global__ __launch_bounds__(256) void k_gjs_pivot(const double* __restrict__ PT, double* __restrict__ Dinv, int n, int kb, int nb, int* __restrict__ flag) {
  __shared__ double M[GJ_NB][GJ_NB + 1];
  __shared__ double colk[GJ_NB];
  __shared__ int piv[GJ_NB];
  const int tid = threadIdx.x;
  for (int idx = tid; idx < GJ_NB * GJ_NB; idx += 256) {
    const int i = idx / GJ_NB, j = idx % GJ_NB;
    M[i][j] = (i < nb && j < nb) ? PT[(size_t)i * n + kb + j] : (i == j ? 1.0 : 0.0);
  }
  __syncthreads();
  gj_invert_block(M, colk, piv, nb, tid, flag);
  for (int idx = tid; idx < nb * nb; idx += 256) Dinv[(idx / nb) * GJ_NB + idx % nb] = M[idx / nb][idx % nb];
}

// new row panel R = Dinv * PT for the columns outside the pivot block -> RT, the matrix row (j right of the block), the matrix
// column (j above it: the transpose); -Dinv into the pivot block
__global__ __launch_bounds__(256) void k_gjs_row_panel(double* __restrict__ D, const double* __restrict__ Dinv, const double* __restrict__ PT,
                                                       double* __restrict__ RT, int n, int kb, int nb) {
  // 64 columns x 4 groups of 8 output rows per workgroup (one wave per group): 4x the waves of a column-per-thread layout
  __shared__ double Ds[GJ_NB][GJ_NB + 1];
  const int tid = threadIdx.x, tx = tid & 63, ty = tid >> 6;
  for (int idx = tid; idx < GJ_NB * GJ_NB; idx += 256) {
    const int a = idx / GJ_NB, b = idx % GJ_NB;
    Ds[a][b] = (a < nb && b < nb) ? Dinv[a * GJ_NB + b] : 0.0;
  }
  __syncthreads();
  const int j = blockIdx.x * 64 + tx;
  if (j >= n) return;
  const int s_lo = ty * (GJ_NB / 4), s_hi = min(nb, s_lo + GJ_NB / 4);
  if (j >= kb && j < kb + nb) {
    for (int s2 = s_lo; s2 < s_hi; s2++) {
      D[(size_t)(kb + s2) * n + j] = -Ds[s2][j - kb];
      RT[(size_t)s2 * n + j] = 0.0;
    }
    return;
  }
  double old[GJ_NB];
#pragma unroll
  for (int t = 0; t < GJ_NB; t++) old[t] = (t < nb) ? PT[(size_t)t * n + j] : 0.0;
  for (int s2 = s_lo; s2 < s_hi; s2++) {
    double acc = 0.0;
#pragma unroll
    for (int t = 0; t < GJ_NB; t++) acc += Ds[s2][t] * old[t];
    RT[(size_t)s2 * n + j] = acc;
    if (j > kb) D[(size_t)(kb + s2) * n + j] = acc;
    else D[(size_t)j * n + kb + s2] = acc;
  }
}

// upper block triangle: A[i][j] -= sum_t PT[t][i] * RT[t][j]   (i, j outside the pivot block)
// Look-ahead: the workgroup that owns the diagonal tile with the NEXT pivot block inverts that block right after its update
// (the tile order is rotated so that it is scheduled first), which takes the sequential 32-step inversion (23 us) off the
// critical path of every step but the first.
__global__ __launch_bounds__(256) void k_gjs_update_mfma(double* __restrict__ D, const double* __restrict__ PT, const double* __restrict__ RT, int n,
                                                         int kb, int nb, double* __restrict__ Dinv_next, int kb_next, int nb_next, int* __restrict__ flag) {
  const int nt = gridDim.x, t_next = (kb_next < n) ? kb_next / 64 : 0;
  const int by = (blockIdx.y + t_next) % nt, bx = (blockIdx.x + t_next) % nt;
  if (by > bx) return;                                    // lower block triangle: not maintained
  constexpr int LD = 80;
  __shared__ double Cs[GJ_KS][LD], Rs[GJ_KS][LD];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int ti = by * 64, tj = bx * 64;
  const int wi = (wave >> 1) * 32, wj = (wave & 1) * 32;
  const int kk = lane >> 4, li = lane & 15;
  gj_d4 acc[2][2];
  bool live[2][4][2];
#pragma unroll
  for (int a = 0; a < 2; a++)
#pragma unroll
    for (int r = 0; r < 4; r++) {
      const int i = ti + wi + a * 16 + kk + 4 * r;
#pragma unroll
      for (int b = 0; b < 2; b++) {
        const int j = tj + wj + b * 16 + li;
        live[a][r][b] = i < n && j < n && !(i >= kb && i < kb + nb) && !(j >= kb && j < kb + nb);
        acc[a][b][r] = live[a][r][b] ? D[(size_t)i * n + j] : 0.0;
      }
    }
  for (int t0 = 0; t0 < nb; t0 += GJ_KS) {
    for (int idx = tid; idx < GJ_KS * 64; idx += 256) {
      const int k = idx >> 6, c = idx & 63, t = t0 + k;
      Cs[k][c] = (ti + c < n && t < nb) ? -PT[(size_t)t * n + ti + c] : 0.0;
      Rs[k][c] = (tj + c < n && t < nb) ? RT[(size_t)t * n + tj + c] : 0.0;
    }
    __syncthreads();
#pragma unroll
    for (int k0 = 0; k0 < GJ_KS; k0 += 4) {
      const double a0 = Cs[k0 + kk][wi + li], a1 = Cs[k0 + kk][wi + 16 + li];
      const double b0 = Rs[k0 + kk][wj + li], b1 = Rs[k0 + kk][wj + 16 + li];
      acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc[0][0], 0, 0, 0);
      acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, acc[0][1], 0, 0, 0);
      acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, acc[1][0], 0, 0, 0);
      acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc[1][1], 0, 0, 0);
    }
    __syncthreads();
  }
#pragma unroll
  for (int a = 0; a < 2; a++)
#pragma unroll
    for (int r = 0; r < 4; r++) {
      const int i = ti + wi + a * 16 + kk + 4 * r;
#pragma unroll
      for (int b = 0; b < 2; b++) {
        const int j = tj + wj + b * 16 + li;
        if (live[a][r][b]) D[(size_t)i * n + j] = acc[a][b][r];
      }
    }
  if (!(kb_next < n && by == bx && by == t_next)) return;
  // ---- this workgroup holds the updated next pivot block in its accumulators: invert it (same elimination as k_gjs_pivot) ----
  double (*M)[GJ_NB + 1] = reinterpret_cast<double (*)[GJ_NB + 1]>(&Cs[0][0]);     // 32 x 33 doubles inside Cs (32 x 80)
  double* colk = &Rs[0][0];
  __syncthreads();
  for (int idx = tid; idx < GJ_NB * GJ_NB; idx += 256) M[idx / GJ_NB][idx % GJ_NB] = (idx / GJ_NB == idx % GJ_NB) ? 1.0 : 0.0;   // identity padding
  __syncthreads();
  const int o = kb_next - ti;                              // offset of the block inside the tile (0 or 32)
#pragma unroll
  for (int a = 0; a < 2; a++)
#pragma unroll
    for (int r = 0; r < 4; r++) {
      const int il = wi + a * 16 + kk + 4 * r - o;
#pragma unroll
      for (int b = 0; b < 2; b++) {
        const int jl = wj + b * 16 + li - o;
        if (il >= 0 && il < nb_next && jl >= 0 && jl < nb_next) M[il][jl] = acc[a][b][r];
      }
    }
  __syncthreads();
  gj_invert_block(M, colk, reinterpret_cast<int*>(&Rs[1][0]), nb_next, tid, flag);
  for (int idx = tid; idx < nb_next * nb_next; idx += 256) Dinv_next[(idx / nb_next) * GJ_NB + idx % nb_next] = M[idx / nb_next][idx % nb_next];
}

// the upper triangle holds -A^-1: negate and mirror (64 x 64 tiles through LDS, both directions coalesced)
__global__ __launch_bounds__(256) void k_gjs_finish(double* __restrict__ D, int n) {
  if (blockIdx.y > blockIdx.x) return;
  __shared__ double Ts[64][65];
  const int ti = blockIdx.y * 64, tj = blockIdx.x * 64;
  for (int idx = threadIdx.x; idx < 64 * 64; idx += 256) {
    const int r = idx >> 6, c = idx & 63, i = ti + r, j = tj + c;
    double v = 0.0;
    if (i < n && j < n) {
      v = (i <= j) ? -D[(size_t)i * n + j] : 0.0;
      if (i <= j) D[(size_t)i * n + j] = v;
    }
    Ts[r][c] = v;
  }
  __syncthreads();
  for (int idx = threadIdx.x; idx < 64 * 64; idx += 256) {
    const int r = idx >> 6, c = idx & 63;              // writes D[tj + r][ti + c] = Ts[c][r]
    const int i = tj + r, j = ti + c;
    if (i < n && j < n && j < i) D[(size_t)i * n + j] = Ts[c][r];
  }
}

// ------------------------------------------------------------------------------------------------
// Symmetric sweep with pivot blocks of 128 (default for symmetric operators; option gj_block): the same three updates as above,
//   A_kk <- -A_kk^-1,  A_ko <- A_kk^-1 A_ko,  A_oo <- A_oo - A_ok A_kk^-1 A_ko     (upper block triangle, ends in -A^-1)
// in n / 128 steps of TWO launches.  With rank-32 updates every step streamed the whole upper triangle (97 MB at n = 4913) for
// 0.8 GFLOP -- 154 steps of ~69 us; a rank-128 update does 3.1 GFLOP per pass over the same bytes, i.e. it is bound by the FP64
// matrix cores and not by HBM, and there are 39 of them.
//   k_inv_panel   one workgroup per 32 columns: gathers the pivot rows PT (from the upper triangle: a row right of the block, a
//                 column above it), R = A_kk^-1 PT on the matrix cores (A_kk^-1 comes from the look-ahead below), writes PT, RT, the
//                 row panel of D and -A_kk^-1 into the pivot block
//   k_inv_update  128 x 128 tiles of the upper block triangle, K = 128 staged through LDS in double-buffered chunks of 16 (one
//                 barrier per chunk), 4 waves x (4 x 4) v_mfma_f64_16x16x4 tiles; tiles of the pivot block column copy the column
//                 panel out of RT (transposed through LDS); the workgroup that owns the NEXT pivot block inverts it right after its
//                 update (tile order rotated so that it is scheduled first): the sequential inversion stays off the critical path
//   inversion of a 128 x 128 block: every thread keeps an 8 x 8 sub-block in registers, pivot row and column go through a
//                 double-buffered LDS line (one barrier per pivot), WITHOUT pivoting; a pivot below 1e-10 of the block's largest
//                 diagonal entry raises flag bit 2 and the host repeats the whole factorisation with the pivoted 32-wide sweep.
// ------------------------------------------------------------------------------------------------
constexpr int IB = 128;          // pivot block and tile
constexpr int IKC = 16;          // k rows staged per chunk
constexpr int ILD = 144;         // LDS row stride in doubles: 2 * ILD mod 64 = 32, the two k rows a half-wave reads hit disjoint banks
constexpr int IPN = 32;          // columns per workgroup of the panel kernel
constexpr int IPLD = 48;         // its B stride: 2 * 48 mod 64 = 32

// In-register inverse of the symmetric block src (nb x nb, upper entries valid, row stride ld, read past the L1: the caller may just
// have written it) -> dst (row-major 128 x 128, rows / columns >= nb identity) and dstT (its transpose).  256 threads, thread
// (ty, tx) owns rows ty*8.., columns tx*8...  lines: 2 x 2 x 128 doubles of LDS.
__device__ __forceinline__ void inv128_block(const double* src, size_t ld, int nb, double* __restrict__ dst, double* __restrict__ dstT, double* lines,
                                            unsigned long long* dmax_bits, int* flag) {
  const int tid = threadIdx.x, ty = tid >> 4, tx = tid & 15;
  double M[8][8];
  double dloc = 0.0;
#pragma unroll
  for (int r = 0; r < 8; r++)
#pragma unroll
    for (int c = 0; c < 8; c++) {
      const int i = ty * 8 + r, j = tx * 8 + c;
      double v = (i == j) ? 1.0 : 0.0;
      if (i < nb && j < nb) v = __hip_atomic_load(src + (size_t)min(i, j) * ld + max(i, j), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      M[r][c] = v;
      if (i == j) dloc = fmax(dloc, fabs(v));
    }
  if (tid == 0) *dmax_bits = 0ull;
  __syncthreads();
  if (ty == tx) atomicMax(dmax_bits, (unsigned long long)__double_as_longlong(dloc));      // non-negative doubles order like their bits
  __syncthreads();
  const double tiny = 1e-10 * __longlong_as_double((long long)*dmax_bits);
  bool bad = false;
#pragma unroll 1
  for (int k8 = 0; k8 < 16; k8++) {
    if (k8 * 8 >= nb) break;
#pragma unroll
    for (int kk = 0; kk < 8; kk++) {
      const int k = k8 * 8 + kk;
      double* rowb = lines + (kk & 1) * 256;       // k and kk have the same parity
      double* colb = rowb + 128;
      if (ty == k8) {
#pragma unroll
        for (int c = 0; c < 8; c++) rowb[tx * 8 + c] = M[kk][c];
      }
      if (tx == k8) {
#pragma unroll
        for (int r = 0; r < 8; r++) colb[ty * 8 + r] = M[r][kk];
      }
      __syncthreads();
      const double piv = rowb[k];
      bad |= !(fabs(piv) > tiny);
      const double p = 1.0 / piv;
      double rk[8], f[8];
#pragma unroll
      for (int c = 0; c < 8; c++) rk[c] = rowb[tx * 8 + c];
#pragma unroll
      for (int r = 0; r < 8; r++) f[r] = colb[ty * 8 + r] * p;
#pragma unroll
      for (int r = 0; r < 8; r++)
#pragma unroll
        for (int c = 0; c < 8; c++) M[r][c] -= f[r] * rk[c];
      if (tx == k8) {                               // column k of the other rows
#pragma unroll
        for (int r = 0; r < 8; r++) M[r][kk] = -f[r];
      }
      if (ty == k8) {                               // row k
#pragma unroll
        for (int c = 0; c < 8; c++) M[kk][c] = rk[c] * p;
        if (tx == k8) M[kk][kk] = p;
      }
    }
  }
  if (bad) atomicOr(flag, 4);
#pragma unroll
  for (int r = 0; r < 8; r++)
#pragma unroll
    for (int c = 0; c < 8; c++) {
      dst[(ty * 8 + r) * IB + tx * 8 + c] = M[r][c];
      dstT[(tx * 8 + c) * IB + ty * 8 + r] = M[r][c];
    }
}

__global__ __launch_bounds__(256) void k_inv_first(const double* __restrict__ D, int n, int nb, double* __restrict__ Dinv, int* __restrict__ flag) {
  __shared__ double lines[512];
  __shared__ unsigned long long dmax_bits;
  inv128_block(D, (size_t)n, nb, Dinv, Dinv + IB * IB, lines, &dmax_bits, flag);
}

// Dinv: [0, IB*IB) the inverse of the pivot block (row-major), [IB*IB, 2 IB*IB) its transpose
__device__ __forceinline__ void inv_panel_body(double* __restrict__ D, const double* __restrict__ Dinv, double* __restrict__ PT, double* __restrict__ RT,
                                               int n, int kb, int nb, int bxi) {
  __shared__ double As[IKC][ILD];
  __shared__ double Bs[IB][IPLD];              // the whole gathered panel of this workgroup: 128 x 32 (+ padding)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int tj = bxi * IPN;
  const bool inside = tj >= kb && tj < kb + IB, left = tj < kb;
  // ---- gather PT[t][tj + jj], t < nb: a column above the block (contiguous in t), the symmetric pivot block, or a row right of it ----
  if (left) {
    for (int idx = tid; idx < IB * IPN; idx += 256) {
      const int jj = idx >> 7, t = idx & 127, j = tj + jj;
      Bs[t][jj] = (t < nb && j < n) ? D[(size_t)j * n + kb + t] : 0.0;
    }
  } else {
    for (int idx = tid; idx < IB * IPN; idx += 256) {
      const int t = idx >> 5, jj = idx & 31, j = tj + jj;
      double v = 0.0;
      if (t < nb && j < n) v = inside ? D[(size_t)(kb + min(t, j - kb)) * n + kb + max(t, j - kb)] : D[(size_t)(kb + t) * n + j];
      Bs[t][jj] = v;
    }
  }
  __syncthreads();
  for (int idx = tid; idx < IB * IPN; idx += 256) {
    const int t = idx >> 5, jj = idx & 31;
    if (tj + jj < n) PT[(size_t)t * n + tj + jj] = Bs[t][jj];
  }
  if (inside) {               // the pivot block takes -A_kk^-1 (upper part); its columns of RT are never read
    for (int idx = tid; idx < IB * IPN; idx += 256) {
      const int s2 = idx >> 5, jj = idx & 31, j = tj + jj;
      if (s2 < nb && j < kb + nb && kb + s2 <= j) D[(size_t)(kb + s2) * n + j] = -Dinv[s2 * IB + (j - kb)];
    }
    return;
  }
  // ---- R = Dinv * PT: wave w the rows 32 w .. 32 w + 31, all 32 columns; A[k][i] = Dinv^T[k][i] streamed through LDS ----
  const int kk = lane >> 4, li = lane & 15, wi = wave * 32;
  gj_d4 acc[2][2];
#pragma unroll
  for (int a = 0; a < 2; a++)
#pragma unroll
    for (int b = 0; b < 2; b++) acc[a][b] = gj_d4{0.0, 0.0, 0.0, 0.0};
  const double* DinvT = Dinv + IB * IB;
  const int nchunk = (nb + IKC - 1) / IKC;
  for (int ch = 0; ch < nchunk; ch++) {
    __syncthreads();
    {
      const int kr = tid >> 4, c8 = (tid & 15) * 8;
      const double* src = DinvT + (size_t)(ch * IKC + kr) * IB + c8;
#pragma unroll
      for (int q = 0; q < 8; q += 2) *reinterpret_cast<double2*>(&As[kr][c8 + q]) = *reinterpret_cast<const double2*>(src + q);
    }
    __syncthreads();
#pragma unroll
    for (int k0 = 0; k0 < IKC; k0 += 4) {
      const double a0 = As[k0 + kk][wi + li], a1 = As[k0 + kk][wi + 16 + li];
      const double b0 = Bs[ch * IKC + k0 + kk][li], b1 = Bs[ch * IKC + k0 + kk][16 + li];
      acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc[0][0], 0, 0, 0);
      acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, acc[0][1], 0, 0, 0);
      acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, acc[1][0], 0, 0, 0);
      acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc[1][1], 0, 0, 0);
    }
  }
#pragma unroll
  for (int a = 0; a < 2; a++)
#pragma unroll
    for (int r = 0; r < 4; r++) {
      const int s2 = wi + a * 16 + kk + 4 * r;
#pragma unroll
      for (int b = 0; b < 2; b++) {
        const int j = tj + b * 16 + li;
        if (j < n) {
          const double v = (s2 < nb) ? acc[a][b][r] : 0.0;
          RT[(size_t)s2 * n + j] = v;
          if (!left && s2 < nb) D[(size_t)(kb + s2) * n + j] = v;
        }
      }
    }
}

// one dense matrix per launch (k_inv_panel / k_inv_update) or several beside each other (k_inv_panel_b / k_inv_update_b: blockIdx.z names the
// matrix, the grid is sized for the largest; the dissected coarse solve inverts its interior blocks this way)
// (InvDesc: fh_internal.h)

__global__ __launch_bounds__(256) void k_inv_panel(double* __restrict__ D, const double* __restrict__ Dinv, double* __restrict__ PT, double* __restrict__ RT,
                                                   int n, int kb, int nb) {
  inv_panel_body(D, Dinv, PT, RT, n, kb, nb, blockIdx.x);
}

__global__ __launch_bounds__(256) void k_inv_panel_b(const InvDesc* __restrict__ desc, int kb, int odd) {
  const InvDesc q = desc[blockIdx.z];
  if (kb >= q.n || (int)blockIdx.x * IPN >= q.n) return;
  inv_panel_body(q.D, odd ? q.Dv1 : q.Dv0, q.PT, q.RT, q.n, kb, min(IB, q.n - kb), blockIdx.x);
}

__device__ __forceinline__ void inv_update_body(double* __restrict__ D, const double* __restrict__ PT, const double* __restrict__ RT, int n, int kb,
                                                int nb, double* __restrict__ Dinv_next, int* __restrict__ flag, int nt, int bxi, int byi) {
  extern __shared__ __attribute__((aligned(16))) double iu_smem[];
  const int kblk = kb / IB, kb_next = kb + IB;
  const int t_next = (kb_next < n) ? kblk + 1 : 0;
  const int by = (byi + t_next) % nt, bx = (bxi + t_next) % nt;
  if (by > bx) return;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int ti = by * IB, tj = bx * IB;
  if (by == kblk) return;                                  // pivot block and row panel: written by k_inv_panel
  if (bx == kblk) {                                         // column panel above the pivot block: D[ti + i][kb + s] = RT[s][ti + i]
    double (*Ts)[65] = reinterpret_cast<double (*)[65]>(iu_smem);
    for (int h = 0; h < 4; h++) {                           // four 64 x 64 quarters through LDS, both directions coalesced
      const int s0 = (h >> 1) * 64, i0 = (h & 1) * 64;
      __syncthreads();
      for (int idx = tid; idx < 64 * 64; idx += 256) {
        const int s2 = s0 + (idx >> 6), i = ti + i0 + (idx & 63);
        Ts[idx >> 6][idx & 63] = (s2 < nb && i < n) ? RT[(size_t)s2 * n + i] : 0.0;
      }
      __syncthreads();
      for (int idx = tid; idx < 64 * 64; idx += 256) {
        const int i = ti + i0 + (idx >> 6), s2 = s0 + (idx & 63);
        if (s2 < nb && i < n) D[(size_t)i * n + kb + s2] = Ts[idx & 63][idx >> 6];
      }
    }
    return;
  }
  double* As = iu_smem;                       // [2][IKC][ILD]
  double* Bs = iu_smem + 2 * IKC * ILD;       // [2][IKC][ILD]
  const int kk = lane >> 4, li = lane & 15;
  const int wi = (wave >> 1) * 64, wj = (wave & 1) * 64;
  gj_d4 acc[4][4];
#pragma unroll
  for (int a = 0; a < 4; a++)
#pragma unroll
    for (int r = 0; r < 4; r++) {
      const int i = ti + wi + a * 16 + kk + 4 * r;
#pragma unroll
      for (int b = 0; b < 4; b++) {
        const int j = tj + wj + b * 16 + li;
        acc[a][b][r] = (i < n && j < n) ? D[(size_t)i * n + j] : 0.0;
      }
    }
  // staging: thread -> k row tid >> 4, eight columns (tid & 15) * 8 of A (= -PT) and of B (= RT)
  const int skr = tid >> 4, sc8 = (tid & 15) * 8;
  double2 ra[4], rb[4];
  auto gload = [&](int ch) {
    const int t = ch * IKC + skr;
    const double* pa = PT + (size_t)t * n + ti + sc8;
    const double* pb = RT + (size_t)t * n + tj + sc8;
#pragma unroll
    for (int q = 0; q < 4; q++) {
      const int ca = ti + sc8 + 2 * q, cb = tj + sc8 + 2 * q;
      double2 va = make_double2(0.0, 0.0), vb = make_double2(0.0, 0.0);
      if (t < nb) {
        if (ca + 1 < n) { va.x = pa[2 * q]; va.y = pa[2 * q + 1]; } else if (ca < n) va.x = pa[2 * q];
        if (cb + 1 < n) { vb.x = pb[2 * q]; vb.y = pb[2 * q + 1]; } else if (cb < n) vb.x = pb[2 * q];
      }
      ra[q] = make_double2(-va.x, -va.y);
      rb[q] = vb;
    }
  };
  auto lstore = [&](int buf) {
    double* da = As + (buf * IKC + skr) * ILD + sc8;
    double* db = Bs + (buf * IKC + skr) * ILD + sc8;
#pragma unroll
    for (int q = 0; q < 4; q++) {
      *reinterpret_cast<double2*>(da + 2 * q) = ra[q];
      *reinterpret_cast<double2*>(db + 2 * q) = rb[q];
    }
  };
  const int nchunk = (nb + IKC - 1) / IKC;
  gload(0);
  lstore(0);
  __syncthreads();
  for (int ch = 0; ch < nchunk; ch++) {
    const int buf = ch & 1;
    if (ch + 1 < nchunk) gload(ch + 1);
    const double* A0 = As + buf * IKC * ILD + wi + li;
    const double* B0 = Bs + buf * IKC * ILD + wj + li;
#pragma unroll
    for (int k0 = 0; k0 < IKC; k0 += 4) {
      double av[4], bv[4];
#pragma unroll
      for (int x = 0; x < 4; x++) {
        av[x] = A0[(k0 + kk) * ILD + x * 16];
        bv[x] = B0[(k0 + kk) * ILD + x * 16];
      }
#pragma unroll
      for (int a = 0; a < 4; a++)
#pragma unroll
        for (int b = 0; b < 4; b++) acc[a][b] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[a], bv[b], acc[a][b], 0, 0, 0);
    }
    if (ch + 1 < nchunk) lstore(buf ^ 1);
    __syncthreads();
  }
#pragma unroll
  for (int a = 0; a < 4; a++)
#pragma unroll
    for (int r = 0; r < 4; r++) {
      const int i = ti + wi + a * 16 + kk + 4 * r;
#pragma unroll
      for (int b = 0; b < 4; b++) {
        const int j = tj + wj + b * 16 + li;
        if (i < n && j < n) D[(size_t)i * n + j] = acc[a][b][r];
      }
    }
  if (!(kb_next < n && by == bx && by == t_next)) return;
  // ---- this workgroup has just written the next pivot block: invert it (off the critical path of the sweep) ----
  __threadfence();
  __syncthreads();
  unsigned long long* dmax_bits = reinterpret_cast<unsigned long long*>(iu_smem + 512);
  inv128_block(D + (size_t)kb_next * n + kb_next, (size_t)n, min(IB, n - kb_next), Dinv_next, Dinv_next + IB * IB, iu_smem, dmax_bits, flag);
}

__global__ __launch_bounds__(256) void k_inv_update(double* __restrict__ D, const double* __restrict__ PT, const double* __restrict__ RT, int n, int kb,
                                                    int nb, double* __restrict__ Dinv_next, int* __restrict__ flag) {
  inv_update_body(D, PT, RT, n, kb, nb, Dinv_next, flag, gridDim.x, blockIdx.x, blockIdx.y);
}

__global__ __launch_bounds__(256) void k_inv_update_b(const InvDesc* __restrict__ desc, int kb, int odd) {
  const InvDesc q = desc[blockIdx.z];
  const int nt = (q.n + IB - 1) / IB;
  if (kb >= q.n || (int)blockIdx.x >= nt || (int)blockIdx.y >= nt) return;
  inv_update_body(q.D, q.PT, q.RT, q.n, kb, min(IB, q.n - kb), odd ? q.Dv0 : q.Dv1, q.flg + 1, nt, blockIdx.x, blockIdx.y);
}

__global__ __launch_bounds__(256) void k_inv_first_b(const InvDesc* __restrict__ desc) {
  __shared__ double lines[512];
  __shared__ unsigned long long dmax_bits;
  const InvDesc q = desc[blockIdx.x];
  inv128_block(q.D, (size_t)q.n, min(IB, q.n), q.Dv0, q.Dv0 + IB * IB, lines, &dmax_bits, q.flg + 1);
}

// the upper triangle holds -A^-1: negate and mirror -- k_gjs_finish for several matrices (blockIdx.z)
__global__ __launch_bounds__(256) void k_gjs_finish_b(const InvDesc* __restrict__ desc) {
  const InvDesc q = desc[blockIdx.z];
  const int n = q.n, nt = (n + 63) / 64;
  if (blockIdx.y > blockIdx.x || (int)blockIdx.x >= nt) return;
  double* D = q.D;
  __shared__ double Ts[64][65];
  const int ti = blockIdx.y * 64, tj = blockIdx.x * 64;
  for (int idx = threadIdx.x; idx < 64 * 64; idx += 256) {
    const int r = idx >> 6, c = idx & 63, i = ti + r, j = tj + c;
    double v = 0.0;
    if (i < n && j < n) {
      v = (i <= j) ? -D[(size_t)i * n + j] : 0.0;
      if (i <= j) D[(size_t)i * n + j] = v;
    }
    Ts[r][c] = v;
  }
  __syncthreads();
  for (int idx = threadIdx.x; idx < 64 * 64; idx += 256) {
    const int r = idx >> 6, c = idx & 63;
    const int i = tj + r, j = ti + c;
    if (i < n && j < n && j < i) D[(size_t)i * n + j] = Ts[c][r];
  }
}

// pivot columns of all other rows: A[i, kb+t] <- - sum_s Cp[i,s] * Dinv[s,t]
__global__ __launch_bounds__(256) void k_gjb_col_panel(double* __restrict__ D, const double* __restrict__ Dinv, const double* __restrict__ Cp,
                                                       int n, int kb, int nb) {
  __shared__ double Ds[GJ_NB][GJ_NB + 1];
  const int tid = threadIdx.x;
  for (int idx = tid; idx < nb * nb; idx += 256) Ds[idx / nb][idx % nb] = Dinv[(idx / nb) * GJ_NB + idx % nb];
  __syncthreads();
  const int idx = blockIdx.x * 256 + tid;
  if (idx >= n * nb) return;
  const int i = idx / nb, t = idx % nb;
  if (i >= kb && i < kb + nb) return;
  double acc = 0.0;
  for (int s2 = 0; s2 < nb; s2++) acc += Cp[(size_t)i * GJ_NB + s2] * Ds[s2][t];
  D[(size_t)i * n + kb + t] = -acc;
}

// row i is decoupled when it has a non-zero diagonal and no other non-zero entry, and no other row has a non-zero in column i; one wave per row
__global__ __launch_bounds__(256) void k_coarse_coupling(const int* __restrict__ rowptr, const int* __restrict__ col, const double* __restrict__ val, int n,
                                                         int* __restrict__ rowhit, int* __restrict__ colhit) {
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (i >= n) return;
  int hit = 0, diag = 0;
  for (int k = rowptr[i] + lane; k < rowptr[i + 1]; k += 64) {
    const int j = col[k];
    const bool nz = val[k] != 0.0;
    if (j == i) diag |= nz ? 1 : 0;
    else if (nz && j < n) {
      hit = 1;
      colhit[j] = 1;          // benign race: every writer stores 1
    }
  }
  hit = __any(hit);
  diag = __any(diag);
  if (lane == 0) rowhit[i] = hit | (diag ? 0 : 2);
}

__global__ __launch_bounds__(256) void k_csr_to_dense_sub(const int* __restrict__ rowptr, const int* __restrict__ col, const double* __restrict__ val,
                                                          double* __restrict__ D, int na, const int* __restrict__ act, const int* __restrict__ pos) {
  const int i = blockIdx.x, row = act[i];
  for (int k = rowptr[row] + threadIdx.x; k < rowptr[row + 1]; k += 256) {
    const int j = pos[col[k]];
    if (j >= 0) D[(size_t)i * na + j] = val[k];
  }
}

// coarse solve with decoupled unknowns, two launches: bc = b[act[0 .. na)] (k_gather_act), then blocks [0, ceil(na / 4)): y[act[i]] = sum_k M[i][k] bc[k],
// one wave per row; the blocks behind them: y[j] = dinv[j] b[j] for the n - na others (act[na ...])
__global__ __launch_bounds__(256) void k_gather_act(const double* __restrict__ b, const int* __restrict__ act, int na, double* __restrict__ bc) {
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k < na) bc[k] = b[act[k]];
}

__global__ __launch_bounds__(256) void k_dense_gemv_sub(const double* __restrict__ M, const double* __restrict__ bc, const double* __restrict__ b,
                                                        double* __restrict__ y, int na, int n, const int* __restrict__ act, const double* __restrict__ dinv) {
  const int nbr = (na + 3) >> 2;
  if ((int)blockIdx.x >= nbr) {
    const int t = ((int)blockIdx.x - nbr) * 256 + threadIdx.x + na;
    if (t < n) {
      const int j = act[t];
      y[j] = dinv[j] * b[j];
    }
    return;
  }
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= na) return;
  const double* m = M + (size_t)row * na;
  double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;          // four loads of the row in flight per lane
  int k = lane;
  for (; k + 192 < na; k += 256) {
    a0 += m[k] * bc[k];
    a1 += m[k + 64] * bc[k + 64];
    a2 += m[k + 128] * bc[k + 128];
    a3 += m[k + 192] * bc[k + 192];
  }
  for (; k < na; k += 64) a0 += m[k] * bc[k];
  double acc = (a0 + a1) + (a2 + a3);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
  if (lane == 0) y[act[row]] = acc;
}

__global__ __launch_bounds__(256) void k_fill_value(double* __restrict__ v, double a, int n) {
  for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) v[i] = a;
}

// ------------------------------------------------------------------------------------------------
// Nested dissection of the dense coarse problem (option coarse_nd = k interior blocks, default 4; needs fh_mg_set_coarse_coords).
// What bounds the dense inverse is its SERIAL pivot chain: n pivots of ~0.7 us whatever the matrix size.  With the coupled unknowns
// ordered [I_0 | ... | I_{k-1} | S] -- S a vertex separator, no entry between two interior blocks --
//     A = [A_II A_IS; A_SI A_SS],  A_II block diagonal,   Sc = A_SS - A_SI A_II^-1 A_IS,   W = A_II^-1 A_IS
// the k block inverses run BESIDE each other (one stream each, chains of n / k pivots), then Sc^-1 (|S| pivots), and the cycle solves
//     t = b_S - W^T b_I,   x_S = Sc^-1 t,   x_I = A_II^-1 b_I - W x_S                    (three launches, exact like the full inverse)
// over 39 instead of 91 MB (bench hierarchy: 4 blocks of 735, separator 435).  Symmetric operators only (W^T = A_SI A_II^-1); an
// unusable pivot in any block falls back to the full inverse with its own fall-backs.
// The separator comes from the coordinates (host, once per pattern, fh_dissect.cpp): the set is halved across the principal axis of its coordinates at
// a layer boundary next to the median, and the side with fewer unknowns coupled to the other side gives them up as separator.
// ------------------------------------------------------------------------------------------------
constexpr int ND_ROW = 512;      // entries of a separator row staged in LDS

__global__ __launch_bounds__(256) void k_csr_to_dense_blk(const int* __restrict__ rowptr, const int* __restrict__ col, const double* __restrict__ val,
                                                          double* __restrict__ D, int off, int nb, const int* __restrict__ act, const int* __restrict__ pos) {
  const int i = blockIdx.x, row = act[off + i];
  for (int k = rowptr[row] + threadIdx.x; k < rowptr[row + 1]; k += 256) {
    const int j = pos[col[k]] - off;
    if (j >= 0 && j < nb) D[(size_t)i * nb + j] = val[k];
  }
}

// W[p][c] = sum over the entries (j, v) of separator row c inside interior block i of v * Binv_i[pos(j)][p]   (A_IS = A_SI^T, Binv symmetric);
// grid (separator unknowns, blocks).  Written as W (interior x separator) and as its transpose.
__device__ __forceinline__ void nd_w_body(const int* __restrict__ rowptr, const int* __restrict__ col, const double* __restrict__ val,
                                          const int* __restrict__ act, const int* __restrict__ pos, const double* __restrict__ Binv, int off, int nb,
                                          int nI, int ns, double* __restrict__ W, double* __restrict__ WT, int* __restrict__ flag) {
  __shared__ int ej[ND_ROW];
  __shared__ double ev[ND_ROW];
  __shared__ int ne;
  const int c = blockIdx.x, row = act[nI + c];
  if (threadIdx.x == 0) {        // the entries of the row inside the block, in the order of the row (the sums below do not depend on lane timing)
    int m = 0;
    for (int k = rowptr[row]; k < rowptr[row + 1]; k++) {
      const int j = pos[col[k]] - off;
      if (j >= 0 && j < nb && val[k] != 0.0) {
        if (m < ND_ROW) {
          ej[m] = j;
          ev[m] = val[k];
        }
        m++;
      }
    }
    if (m > ND_ROW) atomicOr(flag, 8);          // a row with more entries than the staging holds: the caller falls back to the full inverse
    ne = min(m, ND_ROW);
  }
  __syncthreads();
  const int m = ne;
  for (int p = threadIdx.x; p < nb; p += 256) {
    double acc = 0.0;
    for (int e = 0; e < m; e++) acc += ev[e] * Binv[(size_t)ej[e] * nb + p];
    W[(size_t)(off + p) * ns + c] = acc;
    WT[(size_t)c * nI + off + p] = acc;
  }
}

__global__ __launch_bounds__(256) void k_nd_w(const int* __restrict__ rowptr, const int* __restrict__ col, const double* __restrict__ val,
                                              const int* __restrict__ act, const int* __restrict__ pos, const double* __restrict__ Binv, int off, int nb,
                                              int nI, int ns, double* __restrict__ W, double* __restrict__ WT, int* __restrict__ flag) {
  nd_w_body(rowptr, col, val, act, pos, Binv, off, nb, nI, ns, W, WT, flag);
}

// all interior blocks in one launch: grid (separator unknowns, blocks)
__global__ __launch_bounds__(256) void k_nd_w_b(const int* __restrict__ rowptr, const int* __restrict__ col, const double* __restrict__ val,
                                                const int* __restrict__ act, const int* __restrict__ pos, const InvDesc* __restrict__ desc, int nI, int ns,
                                                double* __restrict__ W, double* __restrict__ WT, int* __restrict__ flag) {
  const InvDesc q = desc[blockIdx.y];
  nd_w_body(rowptr, col, val, act, pos, q.D, q.off, q.n, nI, ns, W, WT, flag);
}

// Sc[c1][c2] = A_SS[c1][c2] - sum over the interior entries (j, v) of separator row c1 of v * W[pos(j)][c2]
__global__ __launch_bounds__(256) void k_nd_schur(const int* __restrict__ rowptr, const int* __restrict__ col, const double* __restrict__ val,
                                                  const int* __restrict__ act, const int* __restrict__ pos, const double* __restrict__ W, int nI, int ns,
                                                  double* __restrict__ S, int* __restrict__ flag) {
  __shared__ int ej[ND_ROW];
  __shared__ double ev[ND_ROW];
  __shared__ int ne;
  const int c1 = blockIdx.x, row = act[nI + c1];
  if (threadIdx.x == 0) {
    int m = 0;
    for (int k = rowptr[row]; k < rowptr[row + 1]; k++) {
      const int j = pos[col[k]];
      if (j >= 0 && j < nI && val[k] != 0.0) {
        if (m < ND_ROW) {
          ej[m] = j;
          ev[m] = val[k];
        }
        m++;
      }
    }
    if (m > ND_ROW) atomicOr(flag, 8);
    ne = min(m, ND_ROW);
  }
  __syncthreads();
  const int m = ne;
  for (int c2 = threadIdx.x; c2 < ns; c2 += 256) {
    double acc = 0.0;
    for (int e = 0; e < m; e++) acc += ev[e] * W[(size_t)ej[e] * ns + c2];
    S[(size_t)c1 * ns + c2] -= acc;
  }
}

// the three launches of the block solve (bc = b gathered at the coupled unknowns): one wave per row
__device__ __forceinline__ double nd_wave_dot(const double* __restrict__ m, const double* __restrict__ v, int n, int lane) {
  double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
  int k = lane;
  for (; k + 192 < n; k += 256) {
    a0 += m[k] * v[k];
    a1 += m[k + 64] * v[k + 64];
    a2 += m[k + 128] * v[k + 128];
    a3 += m[k + 192] * v[k + 192];
  }
  for (; k < n; k += 64) a0 += m[k] * v[k];
  double acc = (a0 + a1) + (a2 + a3);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
  return acc;
}

__global__ __launch_bounds__(256) void k_nd_t(const double* __restrict__ WT, const double* __restrict__ bc, int nI, int ns, double* __restrict__ t) {
  const int c = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (c >= ns) return;
  const double acc = nd_wave_dot(WT + (size_t)c * nI, bc, nI, lane);
  if (lane == 0) t[c] = bc[nI + c] - acc;
}

__global__ __launch_bounds__(256) void k_nd_xs(const double* __restrict__ Sinv, const double* __restrict__ t, int ns, int nI, const int* __restrict__ act,
                                               double* __restrict__ xs, double* __restrict__ y) {
  const int c = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (c >= ns) return;
  const double acc = nd_wave_dot(Sinv + (size_t)c * ns, t, ns, lane);
  if (lane == 0) {
    xs[c] = acc;
    y[act[nI + c]] = acc;
  }
}

__global__ __launch_bounds__(256) void k_nd_xi(const double* __restrict__ base, const int64_t* __restrict__ rowoff, const int* __restrict__ rowinfo,
                                               const double* __restrict__ W, const double* __restrict__ bc, const double* __restrict__ xs,
                                               const double* __restrict__ b, double* __restrict__ y, int nI, int ns, int na, int n,
                                               const int* __restrict__ act, const double* __restrict__ dinv) {
  const int nbr = (nI + 3) >> 2;
  if ((int)blockIdx.x >= nbr) {              // the unknowns coupled to nothing: their diagonal
    const int t = ((int)blockIdx.x - nbr) * 256 + threadIdx.x + na;
    if (t < n) {
      const int j = act[t];
      y[j] = dinv[j] * b[j];
    }
    return;
  }
  const int p = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (p >= nI) return;
  const int off = rowinfo[2 * p], nb = rowinfo[2 * p + 1];
  const double a = nd_wave_dot(base + rowoff[p], bc + off, nb, lane);
  const double w = nd_wave_dot(W + (size_t)p * ns, xs, ns, lane);
  if (lane == 0) y[act[p]] = a - w;
}

// ------------------------------------------------------------------------------------------------
// state and host side
// ------------------------------------------------------------------------------------------------
struct CoarseSolve {
  fh_ctx_t ctx = nullptr;
  int n0 = 0;                 // unknowns of level 0 at the last factorisation
  double* d_ainv = nullptr;   // dense inverse of the coupled part of the operator, row-major na x na
  double* d_gjwork = nullptr; // panels of the blocked inversion, kept with d_ainv across preparations
  double* d_gjwork2 = nullptr;   // second pivot-inverse buffer (inside d_gjwork)
  int ainv_n = -1;
  // unknowns of the coarsest level that are coupled to nothing (Dirichlet rows after SetPenalty, whose columns the Galerkin product has
  // emptied too) are solved by their diagonal; the dense inverse holds the na remaining ones.  d_act: their indices, then the others
  int na = -1;
  int* d_act = nullptr;
  int* d_hit = nullptr;       // row / column coupling marks of the last test
  int hit_n = 0;
  // nested dissection of the coupled unknowns (coarse_nd): [interior block 0 | ... | interior block k-1 | separator], see nd_factor
  std::vector<double> xyz;            // coordinates of the unknowns of level 0 (fh_coarse_set_coords), [n0 * dim]
  int dim = 0;
  std::vector<int> h_act_raw;         // the coupled / uncoupled lists before the dissection reordered the coupled part
  int nd_key = -1, coords_version = 0;
  fh_direct_t direct0 = nullptr;      // sparse exact solve of level 0 (more coupled unknowns than the dense inverse holds, or option coarse_direct)
  uint64_t direct0_uid = 0;
  bool direct0_active = false;
  uint64_t nd_A_uid = 0;              // the level-0 matrix the dissection was computed on (another pattern may not be separated by the cached separator)
  bool nd_tables_valid = false;
  std::vector<int> nd_off;            // offsets of the blocks inside the coupled unknowns, nd_off[k] = first separator unknown, nd_off[k + 1] = na
  bool nd_active = false;             // the last factorisation produced the block form (the cycle solves with it)
  double* d_nd = nullptr;             // block inverses, separator inverse, W, W^T, work space
  size_t nd_cap = 0;
  double *d_nd_sinv = nullptr, *d_nd_w = nullptr, *d_nd_wt = nullptr, *d_nd_t = nullptr, *d_nd_xs = nullptr;
  std::vector<double*> nd_dinv;       // per block
  int64_t* d_nd_rowoff = nullptr;     // per interior unknown: where its row of the block inverse starts (doubles from d_nd)
  int* d_nd_rowinfo = nullptr;        // per interior unknown: block offset, block size
  InvDesc* d_nd_desc = nullptr;       // per interior block: matrix, size, work space of its inversion, for the batched launches
  int nd_rows_cap = 0;
  std::vector<hipStream_t> nd_streams;
  std::vector<hipEvent_t> nd_events;
};

CoarseSolve* fh_coarse_create(fh_ctx_t ctx) {
  CoarseSolve* cs = new CoarseSolve();
  cs->ctx = ctx;
  return cs;
}

void fh_coarse_destroy(CoarseSolve* cs) {
  if (!cs) return;
  if (cs->direct0) fh_direct_destroy(cs->direct0);
  for (void* p : std::initializer_list<void*>{cs->d_ainv, cs->d_act, cs->d_hit, cs->d_gjwork, cs->d_nd, cs->d_nd_rowoff, cs->d_nd_rowinfo, cs->d_nd_desc})
    if (p) hipFree(p);
  for (hipStream_t st : cs->nd_streams) hipStreamDestroy(st);
  for (hipEvent_t ev : cs->nd_events) hipEventDestroy(ev);
  delete cs;
}

void fh_coarse_set_coords(CoarseSolve* cs, int dim, int n, const double* coords) {
  cs->xyz.assign(coords, coords + (size_t)n * dim);
  cs->dim = dim;
  cs->coords_version++;
}

void fh_coarse_info(const CoarseSolve* cs, int* n_dense, int* nd_blocks, int* nd_separator, int* nd_largest_block) {
  const int k = (cs->nd_active && !cs->direct0_active) ? (int)cs->nd_off.size() - 2 : 0;
  if (n_dense) *n_dense = cs->na;
  if (nd_blocks) *nd_blocks = cs->direct0_active ? -1 : k;      // -1: no dense inverse at all, the sparse exact solve serves level 0
  if (nd_separator) *nd_separator = k ? cs->na - cs->nd_off[k] : 0;
  int big = 0;
  for (int i = 0; i < k; i++) big = std::max(big, cs->nd_off[i + 1] - cs->nd_off[i]);
  if (nd_largest_block) *nd_largest_block = big;
}

void fh_coarse_signature(const CoarseSolve* cs, std::vector<uint64_t>& w) {
  auto ptr = [&](const void* p) { w.push_back((uint64_t)(uintptr_t)p); };
  ptr(cs->d_ainv);
  ptr(cs->d_nd);
  w.push_back((uint64_t)(cs->nd_active ? cs->nd_off.size() : 0));
  if (cs->nd_active)
    for (int o : cs->nd_off) w.push_back((uint64_t)o);          // another dissection of the same size keeps no captured pointer
  w.push_back((uint64_t)cs->na);
  w.push_back((uint64_t)cs->direct0_active);
  ptr(cs->direct0);
  w.push_back(fh_direct_generation(cs->direct0));     // a re-analysed sparse solve frees and reallocates every buffer the captured launches refer to
  ptr(cs->d_act);
}

// the unpivoted symmetric sweep with pivot blocks of 128 on ONE dense matrix (n x n, leading dimension n) on a given stream;
// work: 2 n IB + 4 IB IB doubles; flag[1] collects bit 2 when a pivot block has no usable diagonal pivot
static size_t inv128_work_doubles(int n) { return (size_t)2 * n * IB + (size_t)4 * IB * IB; }

static int invert_sym128(fh_ctx_t c, hipStream_t st, double* D, int n, double* work, int* flg) {
  double* PT = work;
  double* RT = PT + (size_t)n * IB;
  double* Dv[2] = {RT + (size_t)n * IB, RT + (size_t)n * IB + 2 * IB * IB};
  const int ntb = fh_div_up(n, IB), nt = fh_div_up(n, 64);
  constexpr size_t upd_lds = (size_t)4 * IKC * ILD * sizeof(double);
  static bool attr_set[64] = {};
  if (!attr_set[c->device & 63]) {
    FH_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_inv_update), hipFuncAttributeMaxDynamicSharedMemorySize, (int)upd_lds));
    attr_set[c->device & 63] = true;
  }
  hipLaunchKernelGGL(k_inv_first, dim3(1), dim3(256), 0, st, D, n, std::min(IB, n), Dv[0], flg + 1);
  for (int kb = 0, step = 0; kb < n; kb += IB, step++) {
    const int nb = std::min(IB, n - kb);
    hipLaunchKernelGGL(k_inv_panel, dim3(fh_div_up(n, IPN)), dim3(256), 0, st, D, Dv[step & 1], PT, RT, n, kb, nb);
    hipLaunchKernelGGL(k_inv_update, dim3(ntb, ntb), dim3(256), upd_lds, st, D, PT, RT, n, kb, nb, Dv[(step + 1) & 1], flg + 1);
  }
  hipLaunchKernelGGL(k_gjs_finish, dim3(nt, nt), dim3(256), 0, st, D, n);
  FH_CHECK_HIP(hipGetLastError());
  return 0;
}

// the batched form, also for fh_direct.hip (see fh_coarse.h)
size_t fh_inv_work_doubles(int n) { return inv128_work_doubles(n); }
int fh_inv_sym_batched(fh_ctx_t c, const InvDesc* desc, int k, int nmax) {
  if (k <= 0 || nmax <= 0) return 0;
  constexpr size_t upd_lds = (size_t)4 * IKC * ILD * sizeof(double);
  static bool attr_set[64] = {};
  if (!attr_set[c->device & 63]) {
    FH_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_inv_update_b), hipFuncAttributeMaxDynamicSharedMemorySize, (int)upd_lds));
    attr_set[c->device & 63] = true;
  }
  const int ntb = fh_div_up(nmax, IB), nt64 = fh_div_up(nmax, 64);
  for (int z0 = 0; z0 < k; z0 += 32768) {          // gridDim.z <= 65535
    const int kz = std::min(k - z0, 32768);
    hipLaunchKernelGGL(k_inv_first_b, dim3(kz), dim3(256), 0, c->stream, desc + z0);
    for (int kb = 0, step = 0; kb < nmax; kb += IB, step++) {
      hipLaunchKernelGGL(k_inv_panel_b, dim3(fh_div_up(nmax, IPN), 1, kz), dim3(256), 0, c->stream, desc + z0, kb, step & 1);
      hipLaunchKernelGGL(k_inv_update_b, dim3(ntb, ntb, kz), dim3(256), upd_lds, c->stream, desc + z0, kb, step & 1);
    }
    hipLaunchKernelGGL(k_gjs_finish_b, dim3(nt64, nt64, kz), dim3(256), 0, c->stream, desc + z0);
  }
  FH_CHECK_HIP(hipGetLastError());
  return 0;
}

// layout of the buffer of the block form: block inverses | separator inverse | W | W^T | t | xs | work of the blocks | work of the separator | flags
struct NdLayout {
  std::vector<size_t> boff, woff;   // per block (and the separator behind them): its inverse, the work space of its inversion
  size_t o_sinv, n_mat, o_w, o_wt, n_result, o_t, o_xs, o_flags, tot;
};

static NdLayout nd_layout(const std::vector<int>& nd_off, int k, int nI, int ns) {
  NdLayout y;
  size_t tot = 0;
  auto take = [&](size_t n) { const size_t o = tot; tot += n; return o; };
  auto nb = [&](int i) { return (size_t)(nd_off[i + 1] - nd_off[i]); };
  y.boff.assign(k + 1, 0);
  for (int i = 0; i < k; i++) y.boff[i] = take(nb(i) * nb(i));
  y.boff[k] = tot;
  y.o_sinv = take((size_t)ns * ns);
  y.n_mat = tot;                 // everything that is zeroed before the operator is copied in
  y.o_w = take((size_t)nI * ns);
  y.o_wt = take((size_t)nI * ns);
  y.n_result = tot;              // ... checked for Inf / NaN at the end
  y.o_t = take((size_t)ns + 8);
  y.o_xs = take((size_t)ns + 8);
  y.woff.assign(k + 1, 0);
  for (int i = 0; i < k; i++) y.woff[i] = take(inv128_work_doubles((int)nb(i)));
  y.woff[k] = take(inv128_work_doubles(std::max(ns, 1)));
  y.o_flags = take((size_t)(k + 2) + 8);               // two ints per matrix
  y.tot = tot;
  return y;
}

// the tables the block solve reads per interior unknown and the descriptors of the batched block inverses (once per dissection and buffer)
static int nd_upload_tables(CoarseSolve* cs, const NdLayout& y, int k, int nI, int* flags) {
  double* base = cs->d_nd;
  if (cs->nd_rows_cap < nI) {
    if (cs->d_nd_rowoff) FH_CHECK_HIP(hipFree(cs->d_nd_rowoff));
    if (cs->d_nd_rowinfo) FH_CHECK_HIP(hipFree(cs->d_nd_rowinfo));
    cs->d_nd_rowoff = nullptr;
    cs->d_nd_rowinfo = nullptr;
    cs->nd_rows_cap = 0;
    FH_CHECK_HIP(hipMalloc(&cs->d_nd_rowoff, (size_t)std::max(nI, 1) * sizeof(int64_t)));
    FH_CHECK_HIP(hipMalloc(&cs->d_nd_rowinfo, (size_t)2 * std::max(nI, 1) * sizeof(int)));
    cs->nd_rows_cap = nI;
  }
  std::vector<int64_t> ro(nI);
  std::vector<int> ri((size_t)2 * nI);
  for (int i = 0; i < k; i++) {
    const int off = cs->nd_off[i], nb = cs->nd_off[i + 1] - off;
    for (int p = 0; p < nb; p++) {
      ro[off + p] = (int64_t)(y.boff[i] + (size_t)p * nb);
      ri[2 * (off + p)] = off;
      ri[2 * (off + p) + 1] = nb;
    }
  }
  FH_CHECK_HIP(hipMemcpy(cs->d_nd_rowoff, ro.data(), ro.size() * sizeof(int64_t), hipMemcpyHostToDevice));
  FH_CHECK_HIP(hipMemcpy(cs->d_nd_rowinfo, ri.data(), ri.size() * sizeof(int), hipMemcpyHostToDevice));
  std::vector<InvDesc> hd(k);
  for (int i = 0; i < k; i++) {
    const int nb = cs->nd_off[i + 1] - cs->nd_off[i];
    double* w = base + y.woff[i];
    hd[i] = InvDesc{cs->nd_dinv[i], nb, w, w + (size_t)nb * IB, w + (size_t)2 * nb * IB, w + (size_t)2 * nb * IB + 2 * IB * IB, flags + 2 * i, cs->nd_off[i]};
  }
  if (cs->d_nd_desc) FH_CHECK_HIP(hipFree(cs->d_nd_desc));
  cs->d_nd_desc = nullptr;
  FH_CHECK_HIP(hipMalloc(&cs->d_nd_desc, hd.size() * sizeof(InvDesc)));
  FH_CHECK_HIP(hipMemcpy(cs->d_nd_desc, hd.data(), hd.size() * sizeof(InvDesc), hipMemcpyHostToDevice));
  cs->nd_tables_valid = true;
  return 0;
}

// block form of the coarse solve (see the note above the k_nd_* kernels).  Returns 0 with cs->nd_active set, or 0 with it cleared when a block
// could not be inverted without pivoting (the caller goes on with the full inverse); non-zero: an error of the runtime
static int nd_factor(CoarseSolve* cs, fh_mat_t A, int n, int nfull) {
  fh_ctx_t c = cs->ctx;
  cs->nd_active = false;
  const int k = (int)cs->nd_off.size() - 2;
  if (k < 2) return 0;
  const int nI = cs->nd_off[k], ns = n - nI;
  const NdLayout y = nd_layout(cs->nd_off, k, nI, ns);
  if (y.n_mat >= (size_t)2147483647) return 0;      // beyond the fill kernel's 32-bit length: the caller goes on with the other paths (sparse exact solve)
  if (cs->nd_cap < y.tot) {
    if (cs->d_nd) FH_CHECK_HIP(hipFree(cs->d_nd));
    cs->d_nd = nullptr;
    cs->nd_cap = 0;
    FH_CHECK_HIP(hipMalloc(&cs->d_nd, y.tot * sizeof(double)));
    cs->nd_cap = y.tot;
    cs->nd_tables_valid = false;
  }
  double* base = cs->d_nd;
  cs->nd_dinv.assign(k, nullptr);
  for (int i = 0; i < k; i++) cs->nd_dinv[i] = base + y.boff[i];
  cs->d_nd_sinv = base + y.o_sinv;
  cs->d_nd_w = base + y.o_w;
  cs->d_nd_wt = base + y.o_wt;
  cs->d_nd_t = base + y.o_t;
  cs->d_nd_xs = base + y.o_xs;
  int* flags = reinterpret_cast<int*>(base + y.o_flags);        // [2 i], [2 i + 1] per matrix; the last pair: W / Schur staging overflow
  if (!cs->nd_tables_valid) FH_TRY(nd_upload_tables(cs, y, k, nI, flags));
  while ((int)cs->nd_streams.size() < k) {
    hipStream_t st;
    FH_CHECK_HIP(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    cs->nd_streams.push_back(st);
  }
  while ((int)cs->nd_events.size() < k + 1) {
    hipEvent_t ev;
    FH_CHECK_HIP(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    cs->nd_events.push_back(ev);
  }
  const int* act = cs->d_act;
  const int* pos = cs->d_act + nfull;
  hipLaunchKernelGGL(k_fill_value, dim3(c->num_cu * 4), dim3(256), 0, c->stream, base, 0.0, (int)y.n_mat);
  FH_CHECK_HIP(hipMemsetAsync(flags, 0, (size_t)(2 * (k + 2)) * sizeof(int), c->stream));
  for (int i = 0; i < k; i++) {
    const int off = cs->nd_off[i], nb = cs->nd_off[i + 1] - off;
    hipLaunchKernelGGL(k_csr_to_dense_blk, dim3(nb), dim3(256), 0, c->stream, A->d_rowptr, A->d_col, A->d_val, cs->nd_dinv[i], off, nb, act, pos);
  }
  if (ns > 0) hipLaunchKernelGGL(k_csr_to_dense_blk, dim3(ns), dim3(256), 0, c->stream, A->d_rowptr, A->d_col, A->d_val, cs->d_nd_sinv, nI, ns, act, pos);
  FH_CHECK_HIP(hipGetLastError());
  // the block inverses beside each other: ONE launch per step for all of them (blockIdx.z = block; default), or one stream per block
  // (coarse_nd_streams = 1; beside each other only where the runtime gives the streams distinct hardware queues)
  if (c->coarse_nd_streams == 0) {
    int nmax = 0;
    for (int i = 0; i < k; i++) nmax = std::max(nmax, cs->nd_off[i + 1] - cs->nd_off[i]);
    FH_TRY(fh_inv_sym_batched(c, cs->d_nd_desc, k, nmax));
    if (ns > 0)
      hipLaunchKernelGGL(k_nd_w_b, dim3(ns, k), dim3(256), 0, c->stream, A->d_rowptr, A->d_col, A->d_val, act, pos, cs->d_nd_desc, nI, ns, cs->d_nd_w, cs->d_nd_wt,
                         flags + 2 * (k + 1));
    FH_CHECK_HIP(hipGetLastError());
  } else {
    FH_CHECK_HIP(hipEventRecord(cs->nd_events[k], c->stream));
    for (int i = 0; i < k; i++) {
      const int nb = cs->nd_off[i + 1] - cs->nd_off[i];
      hipStream_t sti = c->coarse_nd_streams == 2 ? c->stream : cs->nd_streams[i];      // 2: one block after the other on the compute stream (measurements)
      FH_CHECK_HIP(hipStreamWaitEvent(sti, cs->nd_events[k], 0));
      FH_TRY(invert_sym128(c, sti, cs->nd_dinv[i], nb, base + y.woff[i], flags + 2 * i));
      if (ns > 0)          // W of this block on its own stream as well: it needs nothing but the block inverse
        hipLaunchKernelGGL(k_nd_w, dim3(ns), dim3(256), 0, sti, A->d_rowptr, A->d_col, A->d_val, act, pos, cs->nd_dinv[i], cs->nd_off[i], nb, nI, ns, cs->d_nd_w,
                           cs->d_nd_wt, flags + 2 * (k + 1));
      FH_CHECK_HIP(hipEventRecord(cs->nd_events[i], sti));
      FH_CHECK_HIP(hipStreamWaitEvent(c->stream, cs->nd_events[i], 0));
    }
  }
  if (ns > 0) {
    hipLaunchKernelGGL(k_nd_schur, dim3(ns), dim3(256), 0, c->stream, A->d_rowptr, A->d_col, A->d_val, act, pos, cs->d_nd_w, nI, ns, cs->d_nd_sinv,
                       flags + 2 * (k + 1));
    FH_CHECK_HIP(hipGetLastError());
    FH_TRY(invert_sym128(c, c->stream, cs->d_nd_sinv, ns, base + y.woff[k], flags + 2 * k));
  }
  hipLaunchKernelGGL(k_check_finite, dim3(std::min(fh_div_up((int64_t)y.n_result, 256), c->num_cu * 8)), dim3(256), 0, c->stream, base, y.n_result,
                     flags + 2 * (k + 1) + 1);
  FH_CHECK_HIP(hipGetLastError());
  std::vector<int> hf((size_t)2 * (k + 2), 0);
  FH_CHECK_HIP(hipMemcpyAsync(hf.data(), flags, hf.size() * sizeof(int), hipMemcpyDeviceToHost, c->stream));
  FH_CHECK_HIP(hipStreamSynchronize(c->stream));
  bool ok = true;
  for (int v : hf) ok = ok && v == 0;
  cs->nd_active = ok;          // anything else: the full inverse with its own fall-backs and error messages decides
  return 0;
}

// step 2 of the factorisation: nested dissection of the coupled unknowns act[0 .. n) (host, once per pattern; coupling graph from the pattern of the
// operator).  Leaves cs->nd_off empty, or fills it and reorders act[0 .. n) into [blocks | separator]
static int coarse_order(CoarseSolve* cs, fh_mat_t A, int n, std::vector<int>& act) {
  fh_ctx_t c = cs->ctx;
  const int nfull = A->m, dim = cs->dim;
  if (!(c->coarse_nd >= 2 && n >= c->coarse_nd_min && dim >= 1 && (int)cs->xyz.size() == nfull * dim)) return 0;
  std::vector<int> rp(nfull + 1), posn(nfull, -1);
  FH_CHECK_HIP(hipMemcpy(rp.data(), A->d_rowptr, rp.size() * sizeof(int), hipMemcpyDeviceToHost));
  std::vector<int> cl(rp[nfull]);
  FH_CHECK_HIP(hipMemcpy(cl.data(), A->d_col, cl.size() * sizeof(int), hipMemcpyDeviceToHost));
  for (int i = 0; i < n; i++) posn[act[i]] = i;
  std::vector<int> sp(n + 1, 0), sc;             // the pattern among the coupled unknowns, in their positions
  for (int i = 0; i < n; i++) {
    for (int k = rp[act[i]]; k < rp[act[i] + 1]; k++)
      if (cl[k] < nfull && posn[cl[k]] >= 0) sc.push_back(posn[cl[k]]);
    sp[i + 1] = (int)sc.size();
  }
  std::vector<double> xyz((size_t)n * dim);
  for (int i = 0; i < n; i++)
    for (int d = 0; d < dim; d++) xyz[(size_t)i * dim + d] = cs->xyz[(size_t)act[i] * dim + d];
  std::vector<int> order(n), off((size_t)c->coarse_nd + 2);
  int noff = 0;
  FH_TRY(fh_coarse_dissection(n, sp.data(), sc.data(), dim, xyz.data(), c->coarse_nd, order.data(), off.data(), &noff));
  if (noff - 2 < 2) return 0;                    // nothing was cut: one dense inverse
  cs->nd_off.assign(off.begin(), off.begin() + noff);
  std::vector<int> act2(act);
  for (int i = 0; i < n; i++) act2[i] = act[order[i]];
  act.swap(act2);
  return 0;
}

// step 1: unknowns coupled to nothing leave the dense problem (exact: the operator is block diagonal with respect to them).  *n: the coupled ones;
// *sym: the operator passed (1) / failed (0) the symmetry test, taken in the same host round trip.  d_act and the dissection are kept while the
// coupled set, the matrix, the coordinates and coarse_nd are the same
static int coarse_reduce(CoarseSolve* cs, fh_mat_t A, int* n, int* sym) {
  fh_ctx_t c = cs->ctx;
  const int nfull = A->m;
  if (cs->hit_n < nfull) {           // kept across preparations (an allocation and its release cost more than the test itself)
    if (cs->d_hit) FH_CHECK_HIP(hipFree(cs->d_hit));
    cs->d_hit = nullptr;
    cs->hit_n = 0;
    FH_CHECK_HIP(hipMalloc(&cs->d_hit, ((size_t)2 * nfull + 2) * sizeof(int)));
    cs->hit_n = nfull;
  }
  int* d_hit = cs->d_hit;
  FH_CHECK_HIP(hipMemsetAsync(d_hit, 0, ((size_t)2 * nfull + 2) * sizeof(int), c->stream));
  hipLaunchKernelGGL(k_coarse_coupling, dim3(fh_div_up(nfull, 4)), dim3(256), 0, c->stream, A->d_rowptr, A->d_col, A->d_val, nfull, d_hit, d_hit + nfull);
  // the symmetry test in the same host round trip (entry by entry on the sparse form, 1e-12 of the row's largest entry; flag behind the marks)
  hipLaunchKernelGGL(k_csr_symmetry, dim3(fh_div_up(nfull, 4)), dim3(256), 0, c->stream, A->d_rowptr, A->d_col, A->d_val, nfull, 1e-12, d_hit + 2 * nfull);
  FH_CHECK_HIP(hipGetLastError());
  std::vector<int> hit((size_t)2 * nfull + 2);
  FH_CHECK_HIP(hipMemcpyAsync(hit.data(), d_hit, hit.size() * sizeof(int), hipMemcpyDeviceToHost, c->stream));
  FH_CHECK_HIP(hipStreamSynchronize(c->stream));
  *sym = hit[(size_t)2 * nfull] == 0 ? 1 : 0;
  std::vector<int> act, rest;
  for (int i = 0; i < nfull; i++) (hit[i] == 0 && hit[nfull + i] == 0 ? rest : act).push_back(i);
  *n = (int)act.size();
  act.insert(act.end(), rest.begin(), rest.end());
  const int nd_key = c->coarse_nd * 1024 + (cs->coords_version & 1023);
  if (act == cs->h_act_raw && cs->d_act && nd_key == cs->nd_key && cs->nd_A_uid == A->uid) return 0;
  cs->nd_A_uid = A->uid;
  if (cs->d_act) FH_CHECK_HIP(hipFree(cs->d_act));
  cs->d_act = nullptr;
  cs->h_act_raw = act;
  cs->nd_key = nd_key;
  cs->nd_off.clear();
  cs->nd_tables_valid = false;
  FH_TRY(coarse_order(cs, A, *n, act));
  std::vector<int> both(act);
  both.resize((size_t)2 * nfull, -1);                  // [nfull, 2 nfull): position of an unknown in the dense problem, -1 = not in it
  for (int i = 0; i < *n; i++) both[nfull + act[i]] = i;
  FH_CHECK_HIP(hipMalloc(&cs->d_act, both.size() * sizeof(int)));
  FH_CHECK_HIP(hipMemcpy(cs->d_act, both.data(), both.size() * sizeof(int), hipMemcpyHostToDevice));
  return 0;
}

// step 3: more coupled unknowns than the dense inverse is meant for (or asked for): the sparse exact solve -- symmetric operators on its unpivoted
// fronts, unsymmetric / indefinite ones on pivoted fronts; only a singular operator is refused and goes on to the dense path and its own limits
static int coarse_try_direct(CoarseSolve* cs, fh_mat_t A, int n) {
  fh_ctx_t c = cs->ctx;
  cs->direct0_active = false;
  if (!(c->coarse_direct == 2 || (c->coarse_direct == 1 && n > c->coarse_direct_min))) return 0;
  if (!cs->direct0 || cs->direct0_uid != A->uid) {
    if (cs->direct0) fh_direct_destroy(cs->direct0);
    cs->direct0 = nullptr;
    const bool have_xyz = cs->dim >= 1 && (int)cs->xyz.size() == A->m * cs->dim;
    FH_TRY(fh_direct_create(c, A, have_xyz ? cs->dim : 0, have_xyz ? cs->xyz.data() : nullptr, 0, &cs->direct0));
    cs->direct0_uid = A->uid;
  }
  if (fh_direct_factor(cs->direct0) == 0) cs->direct0_active = true;
  else FH_TRACE("coarse_factor: the sparse exact solve refused the operator (%s); dense path", fh_last_error());
  return 0;
}

// the dense inverse of step 5: buffers, flag word and the operator as a dense matrix
struct DenseInv {
  CoarseSolve* cs;
  fh_mat_t A;
  int n, nfull;
  // flags behind everything else in the work buffer: [0] unsymmetric, [1] bit 0: singular pivot block, bit 1: non-finite inverse, bit 2: the
  // unpivoted 128-wide sweep met a pivot it cannot use
  int* d_flag;
};

// the coupled part of the operator into the zeroed d_ainv
static void dense_load(const DenseInv& q) {
  fh_ctx_t c = q.cs->ctx;
  const int n = q.n;
  hipLaunchKernelGGL(k_fill_value, dim3(c->num_cu * 8), dim3(256), 0, c->stream, q.cs->d_ainv, 0.0, n * n);      // (the runtime's memset runs at 0.6 TB/s)
  if (n == q.nfull) hipLaunchKernelGGL(k_csr_to_dense, dim3(n), dim3(256), 0, c->stream, q.A->d_rowptr, q.A->d_col, q.A->d_val, q.cs->d_ainv, n);
  else hipLaunchKernelGGL(k_csr_to_dense_sub, dim3(n), dim3(256), 0, c->stream, q.A->d_rowptr, q.A->d_col, q.A->d_val, q.cs->d_ainv, n, q.cs->d_act,
                          q.cs->d_act + q.nfull);
}

// the factorisation must end in a usable inverse: a pivot block without a usable pivot, or Inf / NaN anywhere in the result, is an
// error of fh_mg_setup, not a silent part of every later cycle
static int dense_finish(const DenseInv& q) {
  fh_ctx_t c = q.cs->ctx;
  const int n = q.n;
  int h[2] = {0, 0};
  hipLaunchKernelGGL(k_check_finite, dim3(std::min(fh_div_up((int64_t)n * n, 256), c->num_cu * 8)), dim3(256), 0, c->stream, q.cs->d_ainv, (size_t)n * n,
                     q.d_flag + 1);
  FH_CHECK_HIP(hipGetLastError());
  FH_CHECK_HIP(hipMemcpyAsync(h, q.d_flag, 2 * sizeof(int), hipMemcpyDeviceToHost, c->stream));
  FH_CHECK_HIP(hipStreamSynchronize(c->stream));
  FH_REQUIRE(!(h[1] & 1), "fh_mg_setup: the coarsest operator (%d unknowns) is singular to working precision (no pivot in a %d x %d block)", n, GJ_NB, GJ_NB);
  FH_REQUIRE(!(h[1] & 2), "fh_mg_setup: the inverse of the coarsest operator (%d unknowns) contains Inf / NaN", n);
  return 0;
}

// symmetric operator, pivot blocks of 32 with partial pivoting inside a block: four launches per step (the first: five)
static int dense_sweep_sym32(const DenseInv& q) {
  CoarseSolve* cs = q.cs;
  fh_ctx_t c = cs->ctx;
  const int n = q.n, nt = fh_div_up(n, 64);
  double *PT = cs->d_gjwork, *RT = PT + (size_t)n * GJ_NB;
  double* Dinv2[2] = {PT + (size_t)2 * n * GJ_NB, cs->d_gjwork2};          // pivot inverse of this step / of the next one (look-ahead)
  for (int kb = 0, step = 0; kb < n; kb += GJ_NB, step++) {
    const int nb = std::min(GJ_NB, n - kb);
    const int kb_next = kb + GJ_NB, nb_next = std::max(0, std::min(GJ_NB, n - kb_next));
    hipLaunchKernelGGL(k_gjs_gather_panel, dim3(fh_div_up((int64_t)n * GJ_NB, 256)), dim3(256), 0, c->stream, cs->d_ainv, PT, n, kb, nb);
    if (step == 0) hipLaunchKernelGGL(k_gjs_pivot, dim3(1), dim3(256), 0, c->stream, PT, Dinv2[0], n, kb, nb, q.d_flag + 1);
    hipLaunchKernelGGL(k_gjs_row_panel, dim3(fh_div_up(n, 64)), dim3(256), 0, c->stream, cs->d_ainv, Dinv2[step & 1], PT, RT, n, kb, nb);
    hipLaunchKernelGGL(k_gjs_update_mfma, dim3(nt, nt), dim3(256), 0, c->stream, cs->d_ainv, PT, RT, n, kb, nb, Dinv2[(step + 1) & 1], kb_next, nb_next,
                       q.d_flag + 1);
  }
  hipLaunchKernelGGL(k_gjs_finish, dim3(nt, nt), dim3(256), 0, c->stream, cs->d_ainv, n);
  FH_CHECK_HIP(hipGetLastError());
  return dense_finish(q);
}

// any operator: blocked Gauss-Jordan, five launches per pivot block of 32
static int dense_sweep_general(const DenseInv& q) {
  CoarseSolve* cs = q.cs;
  fh_ctx_t c = cs->ctx;
  const int n = q.n, nt = fh_div_up(n, 64);
  double* Cp = cs->d_gjwork;   // column panel (n x NB), its transpose / the row panel, pivot inverse (NB x NB)
  double* CpT = Cp + (size_t)n * GJ_NB;
  double* Dinv = Cp + (size_t)2 * n * GJ_NB;
  for (int kb = 0; kb < n; kb += GJ_NB) {
    const int nb = std::min(GJ_NB, n - kb);
    hipLaunchKernelGGL(k_gjb_save_panel, dim3(fh_div_up((int64_t)n * nb, 256)), dim3(256), 0, c->stream, cs->d_ainv, Cp, CpT, n, kb, nb);
    hipLaunchKernelGGL(k_gjb_pivot, dim3(1), dim3(256), 0, c->stream, cs->d_ainv, Dinv, n, kb, nb, q.d_flag + 1);
    hipLaunchKernelGGL(k_gjb_row_panel, dim3(fh_div_up(n, 64)), dim3(64), 0, c->stream, cs->d_ainv, Dinv, Cp, n, kb, nb);
    if (c->gj_mfma) hipLaunchKernelGGL(k_gjb_update_mfma, dim3(nt, nt), dim3(256), 0, c->stream, cs->d_ainv, CpT, n, kb, nb);
    else hipLaunchKernelGGL(k_gjb_update, dim3(nt, nt), dim3(256), 0, c->stream, cs->d_ainv, Cp, n, kb, nb);
    hipLaunchKernelGGL(k_gjb_col_panel, dim3(fh_div_up((int64_t)n * nb, 256)), dim3(256), 0, c->stream, cs->d_ainv, Dinv, Cp, n, kb, nb);
  }
  FH_CHECK_HIP(hipGetLastError());
  return dense_finish(q);
}

// step 5: one dense inverse of the coupled part.  sym: the verdict of the symmetry test of this preparation, -1 when it has not run yet
static int coarse_dense_inverse(CoarseSolve* cs, fh_mat_t A, int n, int sym) {
  fh_ctx_t c = cs->ctx;
  const int nfull = A->m;
  FH_REQUIRE(n <= 16384, "coarse level has %d coupled unknowns: the dense direct solve supports at most 16384 (the sparse exact solve, option coarse_direct, serves operators of any size: %s)", n,
             c->coarse_direct ? "it refused this operator as singular" : "it is switched off");
  if (cs->ainv_n != n) {      // a repeated preparation of the same hierarchy keeps its buffers (the 193 MB allocation cost 5-10 ms)
    if (cs->d_ainv) FH_CHECK_HIP(hipFree(cs->d_ainv));
    if (cs->d_gjwork) FH_CHECK_HIP(hipFree(cs->d_gjwork));
    cs->d_ainv = nullptr;
    cs->d_gjwork = nullptr;
    FH_CHECK_HIP(hipMalloc(&cs->d_ainv, (size_t)n * n * sizeof(double)));
    // panels PT, RT of the widest sweep (2 x n x 128), then the pivot inverses: 2 x (block + transpose) of 128 x 128, flags
    FH_CHECK_HIP(hipMalloc(&cs->d_gjwork, (inv128_work_doubles(n) + 8) * sizeof(double)));
    cs->d_gjwork2 = cs->d_gjwork + (size_t)2 * n * GJ_NB + GJ_NB * GJ_NB + 8;
    cs->ainv_n = n;
  }
  const DenseInv q{cs, A, n, nfull, reinterpret_cast<int*>(cs->d_gjwork + inv128_work_doubles(n))};
  dense_load(q);
  FH_CHECK_HIP(hipMemsetAsync(q.d_flag, 0, 2 * sizeof(int), c->stream));
  if (c->gj_symmetric && sym < 0) {          // no coupling pass took the test along (coarse_reduce off)
    int h_flag = 0;
    hipLaunchKernelGGL(k_csr_symmetry, dim3(fh_div_up(nfull, 4)), dim3(256), 0, c->stream, A->d_rowptr, A->d_col, A->d_val, nfull, 1e-12, q.d_flag);
    FH_CHECK_HIP(hipMemcpyAsync(&h_flag, q.d_flag, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    FH_CHECK_HIP(hipStreamSynchronize(c->stream));
    sym = h_flag == 0 ? 1 : 0;
  }
  if (!c->gj_symmetric || sym != 1) return dense_sweep_general(q);
  if (c->gj_block >= IB) {
    // pivot blocks of 128, two launches per step (see k_inv_update)
    FH_TRY(invert_sym128(c, c->stream, cs->d_ainv, n, cs->d_gjwork, q.d_flag));
    int hf[2] = {0, 0};
    FH_CHECK_HIP(hipMemcpyAsync(hf, q.d_flag, 2 * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    FH_CHECK_HIP(hipStreamSynchronize(c->stream));
    if (!(hf[1] & 4)) return dense_finish(q);
    // a pivot block without a usable diagonal pivot (the operator is symmetric but not definite): start again with the pivoted sweep
    FH_CHECK_HIP(hipMemsetAsync(q.d_flag, 0, 2 * sizeof(int), c->stream));
    dense_load(q);
  }
  return dense_sweep_sym32(q);
}

// Prepares the exact solve of level 0 in five steps; the first route that accepts the operator serves the cycle:
//   1. reduce to the coupled unknowns   2. order them (dissection, inside step 1: only when the coupled set or its inputs changed)
//   3. sparse exact solve   4. block form of the dissected dense problem   5. one dense inverse
int fh_coarse_factor(CoarseSolve* cs, fh_mat_t A) {
  fh_ctx_t c = cs->ctx;
  const int nfull = A->m;
  int n = nfull;
  int sym = -1;                  // 1 / 0: the operator passed / failed the symmetry test of this preparation
  cs->n0 = nfull;
  cs->nd_active = false;
  if (!c->coarse_reduce) cs->nd_off.clear();
  if (c->coarse_reduce && nfull > 0) FH_TRY(coarse_reduce(cs, A, &n, &sym));
  cs->na = n;
  if (n == 0) return 0;
  FH_TRY(coarse_try_direct(cs, A, n));
  if (cs->direct0_active) return 0;
  // block form: needs a symmetric operator
  if (!cs->nd_off.empty() && c->gj_symmetric && c->gj_block >= IB && sym == 1) {
    FH_TRY(nd_factor(cs, A, n, nfull));
    if (cs->nd_active) return 0;
  }
  return coarse_dense_inverse(cs, A, n, sym);
}

// the exact solve of level 0: x = A_0^-1 b
int fh_coarse_solve(CoarseSolve* cs, const double* b, double* x, double* r, const double* dinv) {
  fh_ctx_t c = cs->ctx;
  const int n0 = cs->n0, na = cs->na;
  if (cs->direct0_active) return fh_direct_solve_ptr(cs->direct0, b, x);
  if (cs->nd_active) {
    const int k = (int)cs->nd_off.size() - 2, nI = cs->nd_off[k], ns = na - nI;
    hipLaunchKernelGGL(k_gather_act, dim3(fh_div_up(std::max(na, 1), 256)), dim3(256), 0, c->stream, b, cs->d_act, na, r);
    if (ns > 0) {
      hipLaunchKernelGGL(k_nd_t, dim3(fh_div_up(ns, 4)), dim3(256), 0, c->stream, cs->d_nd_wt, r, nI, ns, cs->d_nd_t);
      hipLaunchKernelGGL(k_nd_xs, dim3(fh_div_up(ns, 4)), dim3(256), 0, c->stream, cs->d_nd_sinv, cs->d_nd_t, ns, nI, cs->d_act, cs->d_nd_xs, x);
    }
    hipLaunchKernelGGL(k_nd_xi, dim3(fh_div_up(nI, 4) + fh_div_up(n0 - na, 256)), dim3(256), 0, c->stream, cs->d_nd, cs->d_nd_rowoff, cs->d_nd_rowinfo,
                       cs->d_nd_w, r, cs->d_nd_xs, b, x, nI, ns, na, n0, cs->d_act, dinv);
  } else if (na == n0)
    hipLaunchKernelGGL(k_dense_gemv, dim3(fh_div_up(n0, 4)), dim3(256), 0, c->stream, cs->d_ainv, b, x, n0);
  else {
    hipLaunchKernelGGL(k_gather_act, dim3(fh_div_up(std::max(na, 1), 256)), dim3(256), 0, c->stream, b, cs->d_act, na, r);
    hipLaunchKernelGGL(k_dense_gemv_sub, dim3(fh_div_up(na, 4) + fh_div_up(n0 - na, 256)), dim3(256), 0, c->stream, cs->d_ainv, r, b, x, na, n0, cs->d_act,
                       dinv);
  }
  FH_CHECK_HIP(hipGetLastError());
  return 0;
}
