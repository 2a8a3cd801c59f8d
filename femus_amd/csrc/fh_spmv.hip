// The SpMV family (K7, K8, K9, K10 of SURVEY 2.1) for gfx950 and the layout data it keeps per matrix.
// Replaces MatMult / MatMultAdd / MatMultTranspose (src/03_algebra/01_matrices/PetscMatrix.cpp, src/03_algebra/00_vectors/PetscVector.cpp:182-247).
//
// SpMV design ("CSR-stream", HBM-bound): rows are grouped at setup into row blocks of <= TILE non-zeros.
// One 256-thread workgroup per block streams its contiguous slice of (val, col) with fully coalesced
// 16 B + 8 B loads per lane, multiplies by the gathered x entries (L1/L2/Infinity-Cache hits: x is
// 17 MB on the 64^3 level) and parks the products in LDS; a wave-level segmented reduction (G lanes per
// row, shuffles) then produces the rows.  The epilogue fuses residual / Jacobi-sweep forms, so a smoother
// sweep moves the matrix exactly once.  Blocks are renumbered so that consecutive row blocks (which share
// x lines) run on the same XCD and hit the same 4 MiB L2.
#include "fh_spmv.h"
#include <algorithm>

// ------------------------------------------------------------------------------------------------
// the plan: everything the kernels read beyond the CSR arrays of the matrix (lifetime and invalidation: fh_spmv.h)
// ------------------------------------------------------------------------------------------------
struct SpmvPlan {
  // CSR-stream row blocks
  int tile = 0;
  int tile_kernel = 0;                 // the spmv_kernel the blocks were cut for (it sets the row cap)
  int nblk = 0;
  int* d_rowblk = nullptr;
  std::vector<int> h_rowblk;
  // tile-local column compaction (spmv_kernel 3): unique columns per row block + 16-bit local indices
  int* d_uptr = nullptr;
  int* d_ucols = nullptr;
  unsigned short* d_lcol = nullptr;
  int* d_tile_s = nullptr;             // first non-zero of every row block (persistent pipelined kernel)
  int* d_blkinfo = nullptr;            // 8 ints per row block: r0, r1, s, e, u0, nu (one descriptor load instead of a pointer chain)
  int lx_tile = 0;                     // the tile the local columns were built for (0: none, or stale)
  int64_t nu_total = 0;                // sum over the row blocks of their distinct columns (entries of d_ucols)
  // interior / interface split of the row blocks for operators over [owned | ghost] columns (fh_dev_spmv_part):
  // descriptors permuted so that blocks without a ghost column come first
  int split_nown = -1;                 // number of owned columns the split was built for (-1: none)
  int split_tile = 0;
  int nblk_int = 0;
  int* d_blkinfo_split = nullptr;
};

void fh_spmv_free(SpmvPlan* S) {
  if (!S) return;
  for (void* p : {(void*)S->d_rowblk, (void*)S->d_uptr, (void*)S->d_ucols, (void*)S->d_lcol, (void*)S->d_tile_s, (void*)S->d_blkinfo, (void*)S->d_blkinfo_split})
    if (p) hipFree(p);
  delete S;
}

void fh_spmv_signature(fh_mat_t A, std::vector<uint64_t>& w) {
  const SpmvPlan* S = A->spmv;
  w.push_back((uint64_t)(uintptr_t)(S ? S->d_blkinfo : nullptr));
  w.push_back((uint64_t)(uintptr_t)(S ? S->d_rowblk : nullptr));
  w.push_back(S ? (uint64_t)S->nblk : 0);
  w.push_back(S ? (uint64_t)S->tile : 0);
  w.push_back(S ? (uint64_t)S->lx_tile : 0);
}

extern "C" int64_t fh_spmv_algorithmic_bytes(fh_mat_t A) {
  return 12ll * A->nnz + 4ll * (A->m + 1) + 8ll * A->n + 8ll * A->m;
}

// row blocks: greedy, <= tile non-zeros and <= 512 rows per block; a row longer than the tile is alone
int fh_spmv_build_rowblocks(fh_mat_t A) {
  const int tile = A->ctx->spmv_tile;
  FH_REQUIRE(tile == 256 || tile == 512 || tile == 1024 || tile == 2048 || tile == 4096, "spmv_tile must be 256..4096, power of two (got %d)", tile);
  if (!A->spmv) A->spmv = new SpmvPlan();
  SpmvPlan* const S = A->spmv;
  const int maxrows = (A->ctx->spmv_kernel == 2) ? 128 : (A->ctx->spmv_kernel == 4) ? 255 : 512;
  std::vector<int> blk;
  blk.push_back(0);
  int acc = 0, rows = 0;
  for (int i = 0; i < A->m; i++) {
    int len = A->h_rowptr[i + 1] - A->h_rowptr[i];
    if (rows > 0 && (acc + len > tile || rows >= maxrows)) {
      blk.push_back(i);
      acc = 0;
      rows = 0;
    }
    acc += len;
    rows++;
  }
  blk.push_back(A->m);
  if (A->m == 0) blk.assign(1, 0);
  S->nblk = (int)blk.size() - 1;
  S->tile = tile;
  S->tile_kernel = A->ctx->spmv_kernel;
  S->h_rowblk = blk;
  S->lx_tile = 0;   // local-column data (if any) no longer matches the row blocks
  S->split_nown = -1;
  if (S->d_rowblk) FH_CHECK_HIP(hipFree(S->d_rowblk));
  FH_CHECK_HIP(hipMalloc(&S->d_rowblk, blk.size() * sizeof(int)));
  FH_CHECK_HIP(hipMemcpy(S->d_rowblk, blk.data(), blk.size() * sizeof(int), hipMemcpyHostToDevice));
  return 0;
}

// ------------------------------------------------------------------------------------------------
// SpMV kernels
// ------------------------------------------------------------------------------------------------
// epilogue: MODE 0: y = s ; 1: y += s ; 2: y = b - s ; 3: y = x + omega*dinv*(b - s)
template <int MODE>
__device__ __forceinline__ void spmv_store(double s, int r, const double* __restrict__ x, double* __restrict__ y,
                                           const double* __restrict__ b, const double* __restrict__ dinv, double omega) {
  if (MODE == 0) y[r] = s;
  else if (MODE == 1) y[r] += s;
  else if (MODE == 2) y[r] = b[r] - s;
  else y[r] = x[r] + omega * dinv[r] * (b[r] - s);
}

template <int TILE, int MODE>
__global__ __launch_bounds__(256) void k_spmv_stream(const int* __restrict__ rowptr, const int* __restrict__ col,
                                                     const double* __restrict__ val, const int* __restrict__ rowblk, int nblk, int q,
                                                     const double* __restrict__ x, double* __restrict__ y,
                                                     const double* __restrict__ b, const double* __restrict__ dinv, double omega) {
  __shared__ double prod[TILE + 2];
  // XCD-aware logical block id: physical block p runs on XCD p%8; give each XCD a contiguous range of row blocks
  int blk = (q > 0) ? (int)(blockIdx.x & 7) * q + (int)(blockIdx.x >> 3) : (int)blockIdx.x;
  if (blk >= nblk) return;
  const int tid = threadIdx.x;
  const int r0 = rowblk[blk], r1 = rowblk[blk + 1];
  const int s = rowptr[r0], e = rowptr[r1];
  if (r1 - r0 == 1 && e - s > TILE) {
    // one long row: CSR-vector over the whole workgroup
    double acc = 0.0;
    for (int k = s + tid; k < e; k += 256) acc += val[k] * x[col[k]];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
    if ((tid & 63) == 0) prod[tid >> 6] = acc;
    __syncthreads();
    if (tid == 0) spmv_store<MODE>(prod[0] + prod[1] + prod[2] + prod[3], r0, x, y, b, dinv, omega);
    return;
  }
  // ---- stream phase: aligned (16 B val, 8 B col) pairs --------------------------------------------
  const int s2 = s & ~1;
  constexpr int ITER = TILE / 512 + 1;
  double2 v[ITER];
  int2 c[ITER];
#pragma unroll
  for (int k = 0; k < ITER; k++) {
    int i = s2 + 2 * tid + k * 512;
    if (i < e) {
      v[k] = *reinterpret_cast<const double2*>(val + i);
      c[k] = *reinterpret_cast<const int2*>(col + i);
    }
  }
#pragma unroll
  for (int k = 0; k < ITER; k++) {
    int i = s2 + 2 * tid + k * 512;
    if (i < e) {
      double p0 = v[k].x * x[c[k].x];
      if (i >= s) prod[i - s] = p0;
      if (i + 1 < e) prod[i + 1 - s] = v[k].y * x[c[k].y];
    }
  }
  __syncthreads();
  // ---- segmented reduction: G lanes per row ---------------------------------------------------------
  const int nrows = r1 - r0;
  int G = (nrows <= 16) ? 16 : (nrows <= 32) ? 8 : (nrows <= 64) ? 4 : (nrows <= 128) ? 2 : 1;
  const int gl = tid & (G - 1);
  const int rows_per_pass = 256 / G;
  const int npass = (nrows + rows_per_pass - 1) / rows_per_pass;   // uniform trip count: every lane joins the shuffles
  for (int p = 0; p < npass; p++) {
    const int rr = p * rows_per_pass + tid / G;
    const bool live = rr < nrows;
    const int r = r0 + (live ? rr : 0);
    double acc = 0.0;
    if (live) {
      const int a = rowptr[r] - s, z = rowptr[r + 1] - s;
      for (int k = a + gl; k < z; k += G) acc += prod[k];
    }
    for (int off = G >> 1; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
    if (live && gl == 0) spmv_store<MODE>(acc, r, x, y, b, dinv, omega);
  }
}

// ------------------------------------------------------------------------------------------------
// tile-local column compaction: for every row block the sorted list of distinct columns (ucols) and, per non-zero,
// the 16-bit index into that list.  The SpMV then gathers each needed x entry ONCE per tile into LDS (sorted, hence
// mostly coalesced) and the 135M per-non-zero gathers become LDS reads; the column stream shrinks from 4 to 2 bytes.
// Integer setup work on host threads, done lazily at the first product with the matrix.
// ------------------------------------------------------------------------------------------------
// On the DEVICE since round 4 (the host version, 16 threads, took 0.39 s for the 135 M non-zeros of the bench's fine level -- half of the
// first preparation): one workgroup per row block sorts the block's columns in LDS (bitonic, <= 4096 keys), marks the first of every run,
// scans the marks and writes the distinct columns to a scratch slab and the 16-bit local index of every non-zero; the host only scans the
// 67 k per-block counts.  Same lists, same indices as the host loop gave.
template <int TILE>
__global__ __launch_bounds__(256) void k_localcols(const int* __restrict__ blk, const int* __restrict__ rowptr, const int* __restrict__ col, int tile,
                                                   int* __restrict__ uscratch, int* __restrict__ ucount, unsigned short* __restrict__ lcol) {
  __shared__ int key[TILE];
  __shared__ int uniq[TILE];
  __shared__ int wsum[4];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int s = rowptr[blk[b]], e = rowptr[blk[b + 1]], n = e - s;
  if (n > tile) {                       // single long row: handled by the global-column path
    if (tid == 0) ucount[b] = 0;
    return;
  }
  int np = 64;
  while (np < n) np <<= 1;
  for (int k = tid; k < np; k += 256) key[k] = k < n ? col[s + k] : 0x7fffffff;
  __syncthreads();
  for (int size = 2; size <= np; size <<= 1)
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      for (int t = tid; t < (np >> 1); t += 256) {
        const int lo = ((t / stride) * (stride << 1)) + (t % stride), hi = lo + stride;
        const bool up = ((lo & size) == 0);
        const int a = key[lo], c = key[hi];
        if ((a > c) == up) {
          key[lo] = c;
          key[hi] = a;
        }
      }
      __syncthreads();
    }
  // distinct keys: exclusive scan of the "first of its run" marks, 256 threads x (np / 256) consecutive entries
  const int per = np >> 8 ? np >> 8 : 1, k0 = tid * per;
  int mine = 0;
  for (int k = k0; k < k0 + per && k < n; k++) mine += (k == 0 || key[k] != key[k - 1]) ? 1 : 0;
  int incl = mine;
  const int lane = tid & 63, wave = tid >> 6;
  for (int d = 1; d < 64; d <<= 1) {
    const int v = __shfl_up(incl, d, 64);
    if (lane >= d) incl += v;
  }
  if (lane == 63) wsum[wave] = incl;
  __syncthreads();
  int base = incl - mine;
  for (int w = 0; w < wave; w++) base += wsum[w];
  const int total = wsum[0] + wsum[1] + wsum[2] + wsum[3];
  for (int k = k0; k < k0 + per && k < n; k++)
    if (k == 0 || key[k] != key[k - 1]) uniq[base++] = key[k];
  __syncthreads();
  for (int k = tid; k < total; k += 256) uscratch[(size_t)b * tile + k] = uniq[k];
  if (tid == 0) ucount[b] = total;
  for (int k = tid; k < n; k += 256) {
    const int c = col[s + k];
    int lo = 0, hi = total - 1;
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (uniq[mid] < c) lo = mid + 1; else hi = mid;
    }
    lcol[s + k] = (unsigned short)lo;
  }
}
__global__ __launch_bounds__(256) void k_localcols_compact(const int* __restrict__ uscratch, const int* __restrict__ uptr, int tile, int* __restrict__ ucols) {
  const int b = blockIdx.x;
  const int o = uptr[b], n = uptr[b + 1] - o;
  for (int k = threadIdx.x; k < n; k += 256) ucols[o + k] = uscratch[(size_t)b * tile + k];
}

static int fh_mat_build_localcols(fh_mat_t A) {
  SpmvPlan* const S = A->spmv;
  const int nblk = S->nblk;
  const std::vector<int>& blk = S->h_rowblk;
  fh_ctx_t c = A->ctx;
  std::vector<int> uptr(nblk + 1, 0);
  if (S->d_uptr) FH_CHECK_HIP(hipFree(S->d_uptr));
  if (S->d_ucols) FH_CHECK_HIP(hipFree(S->d_ucols));
  if (S->d_lcol) FH_CHECK_HIP(hipFree(S->d_lcol));
  S->d_uptr = nullptr;
  S->d_ucols = nullptr;
  S->d_lcol = nullptr;
  FH_CHECK_HIP(hipMalloc(&S->d_lcol, ((size_t)A->nnz + 2) * sizeof(unsigned short)));
  FH_CHECK_HIP(hipMemsetAsync(S->d_lcol, 0, ((size_t)A->nnz + 2) * sizeof(unsigned short), c->stream));
  {
    int *d_scratch = nullptr, *d_count = nullptr;
    FH_CHECK_HIP(hipMalloc(&d_scratch, std::max<size_t>((size_t)nblk * S->tile, 1) * sizeof(int)));
    FH_CHECK_HIP(hipMalloc(&d_count, (size_t)(nblk + 1) * sizeof(int)));
    if (nblk) {
      hipLaunchKernelGGL(k_localcols<4096>, dim3(nblk), dim3(256), 0, c->stream, S->d_rowblk, A->d_rowptr, A->d_col, S->tile, d_scratch, d_count, S->d_lcol);
      FH_CHECK_HIP(hipGetLastError());
      FH_CHECK_HIP(hipMemcpyAsync(uptr.data() + 1, d_count, (size_t)nblk * sizeof(int), hipMemcpyDeviceToHost, c->stream));
      FH_CHECK_HIP(hipStreamSynchronize(c->stream));
    }
    for (int b = 0; b < nblk; b++) uptr[b + 1] += uptr[b];
    S->nu_total = uptr[nblk];
    FH_CHECK_HIP(hipMalloc(&S->d_uptr, uptr.size() * sizeof(int)));
    FH_CHECK_HIP(hipMalloc(&S->d_ucols, ((size_t)uptr[nblk] + 1) * sizeof(int)));
    FH_CHECK_HIP(hipMemcpyAsync(S->d_uptr, uptr.data(), uptr.size() * sizeof(int), hipMemcpyHostToDevice, c->stream));
    if (nblk) {
      hipLaunchKernelGGL(k_localcols_compact, dim3(nblk), dim3(256), 0, c->stream, d_scratch, S->d_uptr, S->tile, S->d_ucols);
      FH_CHECK_HIP(hipGetLastError());
    }
    FH_CHECK_HIP(hipStreamSynchronize(c->stream));
    hipFree(d_scratch);
    hipFree(d_count);
  }
  {
    std::vector<int> ts(nblk + 1);
    for (int b = 0; b <= nblk; b++) ts[b] = A->h_rowptr[blk[b]];
    if (S->d_tile_s) FH_CHECK_HIP(hipFree(S->d_tile_s));
    FH_CHECK_HIP(hipMalloc(&S->d_tile_s, ts.size() * sizeof(int)));
    FH_CHECK_HIP(hipMemcpy(S->d_tile_s, ts.data(), ts.size() * sizeof(int), hipMemcpyHostToDevice));
  }
  {
    // one 32-byte descriptor per row block {first row, end row, first nnz, end nnz, first unique column, #unique columns}: the
    // kernel starts from ONE scalar load instead of the chain rowblk -> rowptr (and uptr), i.e. one memory round trip less
    // before the matrix stream can be issued
    std::vector<int> info((size_t)nblk * 8 + 8, 0);
    for (int b = 0; b < nblk; b++) {
      int* d = &info[(size_t)b * 8];
      d[0] = blk[b];
      d[1] = blk[b + 1];
      d[2] = A->h_rowptr[blk[b]];
      d[3] = A->h_rowptr[blk[b + 1]];
      d[4] = uptr[b];
      d[5] = uptr[b + 1] - uptr[b];
    }
    if (S->d_blkinfo) FH_CHECK_HIP(hipFree(S->d_blkinfo));
    FH_CHECK_HIP(hipMalloc(&S->d_blkinfo, info.size() * sizeof(int)));
    FH_CHECK_HIP(hipMemcpy(S->d_blkinfo, info.data(), info.size() * sizeof(int), hipMemcpyHostToDevice));
  }
  S->lx_tile = S->tile;
  S->split_nown = -1;
  FH_TRACE("fh_mat_build_localcols: %d x %d, %d non-zeros, %d row blocks", A->m, A->n, A->nnz, nblk);
  return 0;
}

// SHARE: the x tile and the products use the SAME LDS buffer (one more barrier) -> half the LDS per tile, so twice the
// matrix bytes are in flight per CU at the same residency
template <int TILE, int MODE, bool SHARE, int NT>
__global__ __launch_bounds__(NT) void k_spmv_lx(const int* __restrict__ rowptr, const int* __restrict__ col, const unsigned short* __restrict__ lcol,
                                                 const double* __restrict__ val, const int* __restrict__ blkinfo,
                                                 const int* __restrict__ ucols, int nblk, int q, int chunk, const double* __restrict__ x,
                                                 double* __restrict__ y, const double* __restrict__ b, const double* __restrict__ dinv, double omega) {
  __shared__ double prod[TILE + 2];
  __shared__ double xs_own[SHARE ? 1 : TILE];
  double* xs = SHARE ? prod : xs_own;
  __shared__ int rps[512 + 4];   // a row block holds at most 512 rows (fh_spmv_build_rowblocks)
  // XCD-aware order (workgroup p runs on XCD p % 8).  q > 0: XCD k walks the row blocks in chunks of `chunk` consecutive blocks
  // (neighbouring blocks share x lines -> L2 reuse), the chunks of the 8 XCDs interleaved so that the device as a whole still
  // advances through the matrix front to back; chunk == q is the fully contiguous split
  int blk = (int)blockIdx.x;
  if (q > 0) {
    const int xcd = (int)(blockIdx.x & 7), pos = (int)(blockIdx.x >> 3);
    blk = ((pos / chunk) * 8 + xcd) * chunk + pos % chunk;
  }
  if (blk >= nblk) return;
  const int tid = threadIdx.x;
  const int4 d0 = *reinterpret_cast<const int4*>(blkinfo + (size_t)blk * 8);
  const int2 d1 = *reinterpret_cast<const int2*>(blkinfo + (size_t)blk * 8 + 4);
  const int r0 = d0.x, r1 = d0.y, s = d0.z, e = d0.w;
  if (r1 - r0 == 1 && e - s > TILE) {
    double acc = 0.0;
    for (int k = s + tid; k < e; k += NT) acc += val[k] * x[col[k]];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
    if ((tid & 63) == 0) prod[tid >> 6] = acc;
    __syncthreads();
    if (tid == 0) {
      double tot = 0.0;
      for (int w = 0; w < NT / 64; w++) tot += prod[w];
      spmv_store<MODE>(tot, r0, x, y, b, dinv, omega);
    }
    return;
  }
  // row pointers of the tile: issued now, parked in LDS before the first barrier (no dependent global load in the reduction)
  const int nrows = r1 - r0;
  // epilogue operands of the row this lane will finish (first reduction pass): fetched now, with the stream, instead of as a
  // last dependent round trip after the reduction
  const int G = (nrows <= 16) ? 16 : (nrows <= 32) ? 8 : (nrows <= 64) ? 4 : (nrows <= 128) ? 2 : 1;
  double eb = 0.0, ed = 0.0, ex = 0.0;
  if (MODE >= 1) {
    const int rr0 = tid / G;
    if (rr0 < nrows) {
      if (MODE == 1) eb = y[r0 + rr0];
      if (MODE >= 2) eb = b[r0 + rr0];
      if (MODE == 3) {
        ed = dinv[r0 + rr0];
        ex = x[r0 + rr0];
      }
    }
  }
  int rp0 = 0, rp1 = 0, rp2 = 0;
  if (tid <= nrows) rp0 = rowptr[r0 + tid];
  int rp3 = 0, rp4 = 0;
  if (tid + NT <= nrows) rp1 = rowptr[r0 + tid + NT];
  if (tid + 2 * NT <= nrows) rp2 = rowptr[r0 + tid + 2 * NT];
  if (tid + 3 * NT <= nrows) rp3 = rowptr[r0 + tid + 3 * NT];
  if (tid + 4 * NT <= nrows) rp4 = rowptr[r0 + tid + 4 * NT];
  // ---- matrix stream first (longest latency): 16 B of values + 4 B of local columns per lane and step ----
  const int s2 = s & ~1;
  constexpr int ITER = TILE / (2 * NT) + 1;
  double2 v[ITER];
  ushort2 lc[ITER];
#pragma unroll
  for (int k = 0; k < ITER; k++) {
    const int i = s2 + 2 * tid + k * (2 * NT);
    if (i < e) {
      v[k] = *reinterpret_cast<const double2*>(val + i);
      lc[k] = *reinterpret_cast<const ushort2*>(lcol + i);
    }
  }
  // ---- x entries of this tile -> LDS (sorted distinct columns: neighbouring lanes share cache lines) ----
  const int u0 = d1.x, nu = d1.y;
  for (int j = tid; j < nu; j += NT) xs[j] = x[ucols[u0 + j]];
  if (tid <= nrows) rps[tid] = rp0;
  if (tid + NT <= nrows) rps[tid + NT] = rp1;
  if (tid + 2 * NT <= nrows) rps[tid + 2 * NT] = rp2;
  if (tid + 3 * NT <= nrows) rps[tid + 3 * NT] = rp3;
  if (tid + 4 * NT <= nrows) rps[tid + 4 * NT] = rp4;
  __syncthreads();
  if (SHARE) {
    double p0[ITER], p1[ITER];
#pragma unroll
    for (int k = 0; k < ITER; k++) {
      const int i = s2 + 2 * tid + k * (2 * NT);
      p0[k] = p1[k] = 0.0;
      if (i < e) {
        p0[k] = v[k].x * xs[lc[k].x];
        p1[k] = v[k].y * xs[lc[k].y];
      }
    }
    __syncthreads();                      // every lane has read its x values: the buffer may now hold the products
#pragma unroll
    for (int k = 0; k < ITER; k++) {
      const int i = s2 + 2 * tid + k * (2 * NT);
      if (i < e) {
        if (i >= s) prod[i - s] = p0[k];
        if (i + 1 < e) prod[i + 1 - s] = p1[k];
      }
    }
  } else {
#pragma unroll
    for (int k = 0; k < ITER; k++) {
      const int i = s2 + 2 * tid + k * (2 * NT);
      if (i < e) {
        if (i >= s) prod[i - s] = v[k].x * xs[lc[k].x];
        if (i + 1 < e) prod[i + 1 - s] = v[k].y * xs[lc[k].y];
      }
    }
  }
  __syncthreads();
  const int gl = tid & (G - 1);
  const int rows_per_pass = NT / G;
  const int npass = (nrows + rows_per_pass - 1) / rows_per_pass;
  for (int p = 0; p < npass; p++) {
    const int rr = p * rows_per_pass + tid / G;
    const bool live = rr < nrows;
    const int r = r0 + (live ? rr : 0);
    double acc = 0.0;
    if (live) {
      const int a = rps[rr] - s, z = rps[rr + 1] - s;
      for (int k = a + gl; k < z; k += G) acc += prod[k];
    }
    for (int off = G >> 1; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
    if (live && gl == 0) {
      if (p == 0 && MODE >= 1) {
        if (MODE == 1) y[r] = eb + acc;
        else if (MODE == 2) y[r] = eb - acc;
        else y[r] = ex + omega * ed * (eb - acc);
      } else {
        spmv_store<MODE>(acc, r, x, y, b, dinv, omega);
      }
    }
  }
}

// the epilogue is a template argument of every kernel: LAUNCH(MODE, ...) with the run-time mode as its first argument
#define FH_BY_MODE(mode, LAUNCH, ...)              \
  switch (mode) {                                  \
    case 0: LAUNCH(0, ##__VA_ARGS__); break;       \
    case 1: LAUNCH(1, ##__VA_ARGS__); break;       \
    case 2: LAUNCH(2, ##__VA_ARGS__); break;       \
    default: LAUNCH(3, ##__VA_ARGS__); break;      \
  }

template <int TILE, int NT>
static void launch_lx(fh_mat_t A, int mode, const double* x, double* y, const double* b, const double* dinv, double omega,
                      const int* blkinfo = nullptr, int nblk = -1) {
  fh_ctx_t c = A->ctx;
  const SpmvPlan* const S = A->spmv;
  if (!blkinfo) {          // all row blocks in matrix order; otherwise a sub-list of descriptors (interior / interface split)
    blkinfo = S->d_blkinfo;
    nblk = S->nblk;
  }
  if (nblk <= 0) return;
  int q = 0, grid = nblk, chunk = 1;
  if (c->spmv_xcd_remap && nblk >= 64) {
    // spmv_xcd_remap: 1 = contiguous eighth per XCD, n > 1 = chunks of n consecutive row blocks per XCD, interleaved
    chunk = (c->spmv_xcd_remap == 1) ? (nblk + 7) / 8 : c->spmv_xcd_remap;
    const int per_round = 8 * chunk;
    q = ((nblk + per_round - 1) / per_round) * chunk;     // positions per XCD
    grid = 8 * q;
  }
#define FH_LAUNCH(MODE, SH) \
  hipLaunchKernelGGL((k_spmv_lx<TILE, MODE, SH, NT>), dim3(grid), dim3(NT), 0, c->stream, A->d_rowptr, A->d_col, S->d_lcol, A->d_val, \
                     blkinfo, S->d_ucols, nblk, q, chunk, x, y, b, dinv, omega)
  if (c->spmv_share) {
    FH_BY_MODE(mode, FH_LAUNCH, true)
  } else {
    FH_BY_MODE(mode, FH_LAUNCH, false)
  }
#undef FH_LAUNCH
}

// interior / interface split for an operator over [owned | ghost] columns (PETSc keeps the two column ranges of an MPIAIJ matrix
// as two matrices so that MatMult can multiply the local part while the scatter is in flight, PetscVector.cpp:203-214 ->
// MatMult; here the row BLOCKS are classified): the 32-byte block descriptors are copied in a permuted order, blocks whose
// rows read no column >= n_own first.  The kernel is unchanged -- every descriptor is self-contained.
static int build_split(fh_mat_t A, int n_own) {
  SpmvPlan* const S = A->spmv;
  const int nblk = S->nblk;
  const std::vector<int>& blk = S->h_rowblk;
  std::vector<int> info((size_t)nblk * 8 + 8, 0);
  FH_CHECK_HIP(hipMemcpy(info.data(), S->d_blkinfo, (size_t)nblk * 8 * sizeof(int), hipMemcpyDeviceToHost));
  std::vector<int> order;
  order.reserve(nblk);
  std::vector<char> ghost(nblk, 0);
  for (int b = 0; b < nblk; b++)
    for (int r = blk[b]; r < blk[b + 1] && !ghost[b]; r++)     // columns are sorted inside a row: its last one is its largest
      if (A->h_rowptr[r + 1] > A->h_rowptr[r] && fh_hcol(A)[A->h_rowptr[r + 1] - 1] >= n_own) ghost[b] = 1;
  for (int b = 0; b < nblk; b++)
    if (!ghost[b]) order.push_back(b);
  const int n_int = (int)order.size();
  for (int b = 0; b < nblk; b++)
    if (ghost[b]) order.push_back(b);
  std::vector<int> perm((size_t)nblk * 8 + 8, 0);
  for (int k = 0; k < nblk; k++) memcpy(&perm[(size_t)k * 8], &info[(size_t)order[k] * 8], 8 * sizeof(int));
  if (S->d_blkinfo_split) FH_CHECK_HIP(hipFree(S->d_blkinfo_split));
  S->d_blkinfo_split = nullptr;
  FH_CHECK_HIP(hipMalloc(&S->d_blkinfo_split, perm.size() * sizeof(int)));
  FH_CHECK_HIP(hipMemcpy(S->d_blkinfo_split, perm.data(), perm.size() * sizeof(int), hipMemcpyHostToDevice));
  S->nblk_int = n_int;
  S->split_nown = n_own;
  S->split_tile = S->tile;
  return 0;
}

// THE statement of "the plan is current": brings the layers up to `need` in line with the options in force and rebuilds only what is stale.
// Row blocks serve when they were cut for the tile in force under spmv_kernel ka or kb (the row cap differs: 128 / 255 / 512 rows for kernel
// 2 / 4 / the others).  k_spmv_lx takes the blocks of kernels 3 and 4 alike; the wave kernel (2), the persistent form (4) and the plain stream
// (0) take only their own.  Block boundaries decide the order of a row's partial sums, so a rebuild that today's rule does not ask for changes bits.
enum { SPMV_ROWBLOCKS, SPMV_LOCALCOLS, SPMV_SPLIT };
static int plan_current(fh_mat_t A, int need, int ka, int kb, int n_own = 0) {
  if (!A->spmv || A->spmv->tile != A->ctx->spmv_tile || (A->spmv->tile_kernel != ka && A->spmv->tile_kernel != kb)) FH_TRY(fh_spmv_build_rowblocks(A));
  SpmvPlan* const S = A->spmv;
  if (need >= SPMV_LOCALCOLS && S->lx_tile != S->tile) FH_TRY(fh_mat_build_localcols(A));
  if (need >= SPMV_SPLIT && (S->split_nown != n_own || S->split_tile != S->tile || !S->d_blkinfo_split)) FH_TRY(build_split(A, n_own));
  return 0;
}

// ------------------------------------------------------------------------------------------------
// persistent, software-pipelined form of k_spmv_lx: every workgroup walks a contiguous range of row blocks and keeps
// TWO tiles of matrix data in flight (the loads of tile t+1 and the column list of tile t+2 are issued before tile t is
// reduced), so the HBM stream does not drain while a tile waits for its x gather, its barriers and its row reduction.
// LDS is double-buffered by tile parity: two barriers per tile.
// ------------------------------------------------------------------------------------------------
template <int TILE, int MODE>
__global__ __launch_bounds__(256) void k_spmv_lxp(const int* __restrict__ rowptr, const unsigned short* __restrict__ lcol,
                                                  const double* __restrict__ val, const int* __restrict__ rowblk, const int* __restrict__ tile_s,
                                                  const int* __restrict__ uptr, const int* __restrict__ ucols, int nblk, int tpb, int q,
                                                  const double* __restrict__ x, double* __restrict__ y, const double* __restrict__ b,
                                                  const double* __restrict__ dinv, double omega) {
  constexpr int ITER = TILE / 512 + 1;
  constexpr int NX = TILE / 256;
  __shared__ double prod[2][TILE + 2];
  __shared__ double xs[2][TILE];
  __shared__ int rps[2][260];
  const int tid = threadIdx.x;
  const int chunk = (q > 0) ? (int)(blockIdx.x & 7) * q + (int)(blockIdx.x >> 3) : (int)blockIdx.x;
  const int first = chunk * tpb;
  const int last = min(first + tpb, nblk);
  if (first >= last) return;

  // registers of the tile being loaded ("N") and of the tile after it (column list only, "NN")
  double2 vN[ITER];
  ushort2 lN[ITER];
  double xN[NX];
  int rpN = 0, ucNN[NX];
  int sN, eN, r0N, r1N, nuN;

  auto load_ucols = [&](int t, int (&uc)[NX]) {
    const int u0 = uptr[t], nu = uptr[t + 1] - u0;
#pragma unroll
    for (int k = 0; k < NX; k++) {
      const int j = tid + k * 256;
      uc[k] = (j < nu) ? ucols[u0 + j] : -1;
    }
  };
  auto issue_tile = [&](int t, const int (&uc)[NX]) {
    sN = tile_s[t];
    eN = tile_s[t + 1];
    r0N = rowblk[t];
    r1N = rowblk[t + 1];
    nuN = uptr[t + 1] - uptr[t];
    const int s2 = sN & ~1;
#pragma unroll
    for (int k = 0; k < ITER; k++) {
      const int i = s2 + 2 * tid + k * 512;
      if (i < eN) {
        vN[k] = *reinterpret_cast<const double2*>(val + i);
        lN[k] = *reinterpret_cast<const ushort2*>(lcol + i);
      }
    }
#pragma unroll
    for (int k = 0; k < NX; k++) xN[k] = (uc[k] >= 0) ? x[uc[k]] : 0.0;
    rpN = (tid <= r1N - r0N) ? rowptr[r0N + tid] : 0;
  };

  {
    int uc0[NX];
    load_ucols(first, uc0);
    issue_tile(first, uc0);
    if (first + 1 < last) load_ucols(first + 1, ucNN);
  }
  for (int t = first; t < last; t++) {
    // ---- current tile := the one in flight; start the next one ----
    double2 vC[ITER];
    ushort2 lC[ITER];
    double xC[NX];
#pragma unroll
    for (int k = 0; k < ITER; k++) { vC[k] = vN[k]; lC[k] = lN[k]; }
#pragma unroll
    for (int k = 0; k < NX; k++) xC[k] = xN[k];
    const int rpC = rpN, s = sN, e = eN, r0 = r0N, r1 = r1N, nu = nuN;
    if (t + 1 < last) {
      int ucT[NX];
#pragma unroll
      for (int k = 0; k < NX; k++) ucT[k] = ucNN[k];
      if (t + 2 < last) load_ucols(t + 2, ucNN);
      issue_tile(t + 1, ucT);
    }
    // ---- process tile t ----
    const int par = t & 1;
    const int nrows = r1 - r0;
#pragma unroll
    for (int k = 0; k < NX; k++) {
      const int j = tid + k * 256;
      if (j < nu) xs[par][j] = xC[k];
    }
    if (tid <= nrows) rps[par][tid] = rpC;
    __syncthreads();
    const int s2 = s & ~1;
#pragma unroll
    for (int k = 0; k < ITER; k++) {
      const int i = s2 + 2 * tid + k * 512;
      if (i < e) {
        if (i >= s) prod[par][i - s] = vC[k].x * xs[par][lC[k].x];
        if (i + 1 < e) prod[par][i + 1 - s] = vC[k].y * xs[par][lC[k].y];
      }
    }
    __syncthreads();
    const int G = (nrows <= 16) ? 16 : (nrows <= 32) ? 8 : (nrows <= 64) ? 4 : (nrows <= 128) ? 2 : 1;
    const int gl = tid & (G - 1);
    const int rr = tid / G;                       // nrows <= 255 and 256/G >= nrows for every G above: one pass
    const bool live = rr < nrows;
    double acc = 0.0;
    if (live) {
      const int a = rps[par][rr] - s, z = rps[par][rr + 1] - s;
      for (int k = a + gl; k < z; k += G) acc += prod[par][k];
    }
    for (int off = G >> 1; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
    if (live && gl == 0) spmv_store<MODE>(acc, r0 + rr, x, y, b, dinv, omega);
  }
}

template <int TILE>
static void launch_lxp(fh_mat_t A, int mode, const double* x, double* y, const double* b, const double* dinv, double omega) {
  fh_ctx_t c = A->ctx;
  const SpmvPlan* const S = A->spmv;
  const int target_blocks = c->num_cu * 5;
  int tpb = std::max(1, (S->nblk + target_blocks - 1) / target_blocks);
  int nchunks = (S->nblk + tpb - 1) / tpb;
  int q = 0, grid = nchunks;
  if (c->spmv_xcd_remap && nchunks >= 64) {
    q = (nchunks + 7) / 8;
    grid = 8 * q;
  }
#define FH_LAUNCH(MODE) \
  hipLaunchKernelGGL((k_spmv_lxp<TILE, MODE>), dim3(grid), dim3(256), 0, c->stream, A->d_rowptr, S->d_lcol, A->d_val, S->d_rowblk, S->d_tile_s, \
                     S->d_uptr, S->d_ucols, S->nblk, tpb, q, x, y, b, dinv, omega)
  FH_BY_MODE(mode, FH_LAUNCH)
#undef FH_LAUNCH
}

// wave-granular CSR-stream: every wave owns one row block of <= WT non-zeros and runs on its own (no workgroup
// barrier), so slow gathers of one tile do not hold back its neighbours; NT=1 streams (val, col) with non-temporal
// loads so the once-read matrix does not evict x from L2.
template <int WT, int MODE, int NT>
__global__ __launch_bounds__(256) void k_spmv_wave(const int* __restrict__ rowptr, const int* __restrict__ col,
                                                   const double* __restrict__ val, const int* __restrict__ rowblk, int nblk, int q,
                                                   const double* __restrict__ x, double* __restrict__ y,
                                                   const double* __restrict__ b, const double* __restrict__ dinv, double omega) {
  __shared__ double prod_all[4][WT + 2];
  __shared__ int rp_all[4][132];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int pb = blockIdx.x * 4 + wave;     // physical wave-tile id
  // XCD-aware: workgroup p runs on XCD p%8; keep consecutive row blocks on one XCD
  int blk = pb;
  if (q > 0) {
    const int wg = blockIdx.x;
    blk = ((wg & 7) * q + (wg >> 3)) * 4 + wave;
  }
  if (blk >= nblk) return;
  double* prod = prod_all[wave];
  int* rp = rp_all[wave];
  const int r0 = rowblk[blk], r1 = rowblk[blk + 1];
  const int nrows = r1 - r0;
  // row pointers of the tile -> LDS (also gives s, e)
  for (int k = lane; k <= nrows; k += 64) rp[k] = rowptr[r0 + k];
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  const int s = rp[0], e = rp[nrows];
  if (nrows == 1 && e - s > WT) {
    double acc = 0.0;
    for (int k = s + lane; k < e; k += 64) acc += val[k] * x[col[k]];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
    if (lane == 0) spmv_store<MODE>(acc, r0, x, y, b, dinv, omega);
    return;
  }
  const int s2 = s & ~1;
  constexpr int ITER = WT / 128 + 1;
  double2 v[ITER];
  int2 c[ITER];
#pragma unroll
  for (int k = 0; k < ITER; k++) {
    const int i = s2 + 2 * lane + k * 128;
    if (i < e) {
      if (NT) {
        typedef double d2v __attribute__((ext_vector_type(2)));
        typedef int i2v __attribute__((ext_vector_type(2)));
        const d2v vv = __builtin_nontemporal_load(reinterpret_cast<const d2v*>(val + i));
        const i2v cc = __builtin_nontemporal_load(reinterpret_cast<const i2v*>(col + i));
        v[k] = make_double2(vv.x, vv.y);
        c[k] = make_int2(cc.x, cc.y);
      } else {
        v[k] = *reinterpret_cast<const double2*>(val + i);
        c[k] = *reinterpret_cast<const int2*>(col + i);
      }
    }
  }
#pragma unroll
  for (int k = 0; k < ITER; k++) {
    const int i = s2 + 2 * lane + k * 128;
    if (i < e) {
      const double p0 = v[k].x * x[c[k].x];
      if (i >= s) prod[i - s] = p0;
      if (i + 1 < e) prod[i + 1 - s] = v[k].y * x[c[k].y];
    }
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  const int G = (nrows <= 4) ? 16 : (nrows <= 8) ? 8 : (nrows <= 16) ? 4 : (nrows <= 32) ? 2 : 1;
  const int gl = lane & (G - 1);
  const int rows_per_pass = 64 / G;
  const int npass = (nrows + rows_per_pass - 1) / rows_per_pass;
  for (int p = 0; p < npass; p++) {
    const int rr = p * rows_per_pass + lane / G;
    const bool live = rr < nrows;
    double acc = 0.0;
    if (live) {
      const int a = rp[rr] - s, z = rp[rr + 1] - s;
      for (int k = a + gl; k < z; k += G) acc += prod[k];
    }
    for (int off = G >> 1; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
    if (live && gl == 0) spmv_store<MODE>(acc, r0 + rr, x, y, b, dinv, omega);
  }
}

// classic CSR-vector: LANES lanes per row (kept for A/B measurements and very small matrices)
template <int LANES, int MODE>
__global__ __launch_bounds__(256) void k_spmv_vector(const int* __restrict__ rowptr, const int* __restrict__ col,
                                                     const double* __restrict__ val, int m, const double* __restrict__ x,
                                                     double* __restrict__ y, const double* __restrict__ b,
                                                     const double* __restrict__ dinv, double omega) {
  const int r = (blockIdx.x * 256 + threadIdx.x) / LANES;
  const int gl = threadIdx.x & (LANES - 1);
  const bool live = r < m;
  double acc = 0.0;
  if (live) {
    const int s = rowptr[r], e = rowptr[r + 1];
    for (int k = s + gl; k < e; k += LANES) acc += val[k] * x[col[k]];
  }
#pragma unroll
  for (int off = LANES >> 1; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
  if (live && gl == 0) spmv_store<MODE>(acc, r, x, y, b, dinv, omega);
}

template <int TILE>
static void launch_stream(fh_mat_t A, int mode, const double* x, double* y, const double* b, const double* dinv, double omega) {
  fh_ctx_t c = A->ctx;
  const SpmvPlan* const S = A->spmv;
  int q = 0, grid = S->nblk;
  if (c->spmv_xcd_remap && S->nblk >= 64) {
    q = (S->nblk + 7) / 8;
    grid = 8 * q;
  }
#define FH_LAUNCH(MODE) \
  hipLaunchKernelGGL((k_spmv_stream<TILE, MODE>), dim3(grid), dim3(256), 0, c->stream, A->d_rowptr, A->d_col, A->d_val, \
                     S->d_rowblk, S->nblk, q, x, y, b, dinv, omega)
  FH_BY_MODE(mode, FH_LAUNCH)
#undef FH_LAUNCH
}

int fh_dev_spmv(fh_mat_t A, const double* x, double* y, int mode, const double* b, const double* dinv, double omega) {
  fh_ctx_t c = A->ctx;
  if (A->m == 0) return 0;
  FH_REQUIRE(mode >= 0 && mode <= 3, "fh_spmv: unknown mode %d", mode);
  FH_REQUIRE(x != y, "fh_spmv: x and y must not alias");
  if (c->spmv_kernel == 1) {
    const int grid = fh_div_up((int64_t)A->m * 16, 256);
#define FH_LAUNCHV(MODE) \
  hipLaunchKernelGGL((k_spmv_vector<16, MODE>), dim3(grid), dim3(256), 0, c->stream, A->d_rowptr, A->d_col, A->d_val, A->m, x, y, b, dinv, omega)
    FH_BY_MODE(mode, FH_LAUNCHV)
#undef FH_LAUNCHV
  } else if (c->spmv_kernel == 2) {
    FH_TRY(plan_current(A, SPMV_ROWBLOCKS, 2, 2));
    const SpmvPlan* const S = A->spmv;
    const int nwg = fh_div_up(S->nblk, 4);
    int q = 0, grid = nwg;
    if (c->spmv_xcd_remap && nwg >= 64) {
      q = (nwg + 7) / 8;
      grid = 8 * q;
    }
    const int nt = c->spmv_nt;
#define FH_LW(MODE, WT, NT) \
  hipLaunchKernelGGL((k_spmv_wave<WT, MODE, NT>), dim3(grid), dim3(256), 0, c->stream, A->d_rowptr, A->d_col, A->d_val, S->d_rowblk, \
                     S->nblk, q, x, y, b, dinv, omega)
    FH_REQUIRE(S->tile <= 1024, "spmv_kernel 2 needs spmv_tile <= 1024");
    if (S->tile == 256) { if (nt) { FH_BY_MODE(mode, FH_LW, 256, 1) } else { FH_BY_MODE(mode, FH_LW, 256, 0) } }
    else if (S->tile == 512) { if (nt) { FH_BY_MODE(mode, FH_LW, 512, 1) } else { FH_BY_MODE(mode, FH_LW, 512, 0) } }
    else { if (nt) { FH_BY_MODE(mode, FH_LW, 1024, 1) } else { FH_BY_MODE(mode, FH_LW, 1024, 0) } }
#undef FH_LW
  } else if (c->spmv_kernel == 4 && A->max_row <= c->spmv_tile) {
    FH_REQUIRE(c->spmv_tile == 1024 || c->spmv_tile == 2048, "spmv_kernel 4 needs spmv_tile 1024 or 2048");
    FH_TRY(plan_current(A, SPMV_LOCALCOLS, 4, 4));
    if (c->spmv_tile == 1024) launch_lxp<1024>(A, mode, x, y, b, dinv, omega);
    else launch_lxp<2048>(A, mode, x, y, b, dinv, omega);
  } else if (c->spmv_kernel == 3 || c->spmv_kernel == 4) {
    FH_REQUIRE(c->spmv_tile == 1024 || c->spmv_tile == 2048 || c->spmv_tile == 4096, "spmv_kernel 3 needs spmv_tile 1024, 2048 or 4096");
    FH_TRY(plan_current(A, SPMV_LOCALCOLS, 3, 4));
    const int tile = c->spmv_tile;       // the tile of the plan, now
    if (c->spmv_threads == 128) {
      if (tile == 1024) launch_lx<1024, 128>(A, mode, x, y, b, dinv, omega);
      else if (tile == 2048) launch_lx<2048, 128>(A, mode, x, y, b, dinv, omega);
      else launch_lx<4096, 128>(A, mode, x, y, b, dinv, omega);
    } else {
      if (tile == 1024) launch_lx<1024, 256>(A, mode, x, y, b, dinv, omega);
      else if (tile == 2048) launch_lx<2048, 256>(A, mode, x, y, b, dinv, omega);
      else launch_lx<4096, 256>(A, mode, x, y, b, dinv, omega);
    }
  } else {
    FH_TRY(plan_current(A, SPMV_ROWBLOCKS, 0, 0));
    const int tile = c->spmv_tile;       // the tile of the plan, now
    FH_REQUIRE(tile >= 1024, "spmv_kernel 0 needs spmv_tile >= 1024");
    if (tile == 1024) launch_stream<1024>(A, mode, x, y, b, dinv, omega);
    else if (tile == 2048) launch_stream<2048>(A, mode, x, y, b, dinv, omega);
    else launch_stream<4096>(A, mode, x, y, b, dinv, omega);
  }
  FH_CHECK_HIP(hipGetLastError());
  return 0;
}

int fh_dev_spmv_part(fh_mat_t A, int n_own, int part, const double* x, double* y, int mode, const double* b, const double* dinv, double omega) {
  fh_ctx_t c = A->ctx;
  if (A->m == 0) return 0;
  FH_REQUIRE(mode >= 0 && mode <= 3, "fh_spmv: unknown mode %d", mode);
  FH_REQUIRE(x != y, "fh_spmv: x and y must not alias");
  FH_REQUIRE(part == 0 || part == 1, "fh_dev_spmv_part: part %d", part);
  const bool lx = (c->spmv_kernel == 3 || (c->spmv_kernel == 4 && A->max_row > c->spmv_tile)) && c->spmv_threads == 256 &&
                  (c->spmv_tile == 1024 || c->spmv_tile == 2048 || c->spmv_tile == 4096);
  if (!lx) return part == 0 ? 0 : fh_dev_spmv(A, x, y, mode, b, dinv, omega);     // other kernels: no split, everything after the exchange
  FH_TRY(plan_current(A, SPMV_SPLIT, 3, 4, n_own));
  const SpmvPlan* const S = A->spmv;
  const int* info = S->d_blkinfo_split + (part == 0 ? 0 : (size_t)S->nblk_int * 8);
  const int nb = part == 0 ? S->nblk_int : S->nblk - S->nblk_int;
  if (S->tile == 1024) launch_lx<1024, 256>(A, mode, x, y, b, dinv, omega, info, nb);
  else if (S->tile == 2048) launch_lx<2048, 256>(A, mode, x, y, b, dinv, omega, info, nb);
  else launch_lx<4096, 256>(A, mode, x, y, b, dinv, omega, info, nb);
  FH_CHECK_HIP(hipGetLastError());
  return 0;
}

/* interior / interface block counts of the split used on distributed levels (diagnostics, tests) */
extern "C" int fh_mat_split_info(fh_mat_t A, int n_own_cols, int* nblk_interior, int* nblk_interface) {
  FH_REQUIRE(A, "fh_mat_split_info: null argument");
  FH_TRY(plan_current(A, SPMV_SPLIT, 3, 4, n_own_cols));
  const SpmvPlan* const S = A->spmv;
  if (nblk_interior) *nblk_interior = S->nblk_int;
  if (nblk_interface) *nblk_interface = S->nblk - S->nblk_int;
  return 0;
}

extern "C" int fh_spmv(fh_mat_t A, fh_vec_t x, fh_vec_t y, int mode, fh_vec_t b, fh_vec_t dinv, double omega) {
  FH_REQUIRE(A && x && y, "fh_spmv: null argument");
  FH_REQUIRE(x->n_local + x->nghost >= A->n, "fh_spmv: x has %d entries, matrix has %d columns", x->n_local + x->nghost, A->n);
  FH_REQUIRE(y->n_local >= A->m, "fh_spmv: y has %d entries, matrix has %d rows", y->n_local, A->m);
  FH_REQUIRE(mode < 2 || (b && b->n_local >= A->m), "fh_spmv: mode %d needs b", mode);
  // Jacobi sweep: x_new[i] = x[i] + omega dinv[i] (b[i] - (A x)[i]) for the rows of A; on a distributed level A holds the owned
  // rows over [owned | ghost] columns (m <= n) and row i sits at column i
  FH_REQUIRE(mode < 3 || (dinv && dinv->n_local >= A->m && A->m <= A->n),
             "fh_spmv: mode 3 needs dinv and a square matrix (or owned rows over [owned | ghost] columns)");
  return fh_dev_spmv(A, x->d, y->d, mode, b ? b->d : nullptr, dinv ? dinv->d : nullptr, omega);
}

extern "C" int fh_spmv_transpose(fh_mat_t A, fh_vec_t x, fh_vec_t y) {
  FH_REQUIRE(x->n_local >= A->m && y->n_local >= A->n, "fh_spmv_transpose: size mismatch");
  FH_TRY(fh_mat_refresh_transpose(A));
  return fh_dev_spmv(A->At, x->d, y->d, 0, nullptr, nullptr, 0.0);
}

// Bytes the LDS-staged kernel (spmv_kernel 3) really touches per product, from the sizes of its arrays: the value stream (8 nnz), the 16-bit
// local columns (2 nnz), the distinct-column lists (4 per entry of ucols), the 32-byte block descriptors, the row pointers of the block's
// rows, y (and b, D^-1, x_row for the fused forms) -- and x: `lo` counts every entry of x once (all tiles that share a column find it in the
// L2), `hi` counts every tile's gather as a miss.  The algorithmic figure (12 B per non-zero) sits between the two for FE matrices.
extern "C" int fh_spmv_expected_bytes(fh_mat_t A, int mode, int64_t* lo, int64_t* hi) {
  FH_REQUIRE(A && lo && hi && mode >= 0 && mode <= 3, "fh_spmv_expected_bytes: bad arguments");
  FH_TRY(plan_current(A, SPMV_LOCALCOLS, 3, 4));
  const SpmvPlan* const S = A->spmv;
  const int64_t fixed = 10ll * A->nnz + 4ll * S->nu_total + 32ll * S->nblk + 4ll * ((int64_t)A->m + S->nblk) + 8ll * A->m +
                        (mode == 1 || mode == 2 ? 8ll * A->m : mode == 3 ? 24ll * A->m : 0);
  *lo = fixed + 8ll * A->n;
  *hi = fixed + 8ll * S->nu_total;
  return 0;
}
