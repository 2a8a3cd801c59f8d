// Device CSR matrices for gfx950: creation, patterns from elements, row and column operations, transpose, block systems, norms.
// Replaces PetscMatrix / MatZeroRows (src/03_algebra/01_matrices/PetscMatrix.cpp).  The products with a matrix are fh_spmv.hip's.
#include "fh_spmv.h"
#include <atomic>
#include <mutex>
#include <unordered_map>
#include <algorithm>
#include <cmath>
#include <thread>

// ------------------------------------------------------------------------------------------------
// creation / destruction
// ------------------------------------------------------------------------------------------------
// the live matrices by uid: whoever remembers a matrix beyond the call that named it (the macro rows of a fused assembly) keeps the uid and asks here
// (both live in one object that is made at the first use and never destroyed: a matrix may be destroyed from a finaliser that runs after the library's
//  static destructors)
struct LiveMats {
  std::mutex mutex;
  std::unordered_map<uint64_t, fh_mat_t> map;
};
static LiveMats& live_mats() {
  static LiveMats* const l = new LiveMats();
  return *l;
}
// the one place a matrix object is made: a uid of its own, and an entry among the live matrices until fh_mat_destroy
static fh_mat_t mat_new(fh_ctx_t c) {
  static std::atomic<uint64_t> next_uid{1};
  fh_mat_t A = new fh_mat_s();
  A->uid = next_uid++;
  A->ctx = c;
  LiveMats& L = live_mats();
  std::lock_guard<std::mutex> g(L.mutex);
  L.map[A->uid] = A;
  return A;
}
fh_mat_t fh_mat_alive(uint64_t uid) {
  LiveMats& L = live_mats();
  std::lock_guard<std::mutex> g(L.mutex);
  auto it = L.map.find(uid);
  return it == L.map.end() ? nullptr : it->second;
}

extern "C" int fh_mat_create_csr(fh_ctx_t c, int m, int n, const int* rowptr, const int* col, const double* val, fh_mat_t* out) {
  FH_GUARD_BEGIN
  FH_REQUIRE(c && out && rowptr, "fh_mat_create_csr: null argument");
  FH_REQUIRE(m >= 0 && n >= 0 && rowptr[0] == 0, "fh_mat_create_csr: bad sizes");
  const int nnz = rowptr[m];
  FH_REQUIRE(nnz == 0 || col != nullptr, "fh_mat_create_csr: null column array");
  fh_mat_t A = mat_new(c);
  A->m = m;
  A->n = n;
  A->nnz = nnz;
  A->h_rowptr.assign(rowptr, rowptr + m + 1);
  A->h_col.assign(col, col + nnz);
  int maxrow = 0;
  for (int i = 0; i < m; i++) {
    FH_REQUIRE(rowptr[i + 1] >= rowptr[i], "fh_mat_create_csr: rowptr not monotone at row %d", i);
    maxrow = std::max(maxrow, rowptr[i + 1] - rowptr[i]);
    for (int k = rowptr[i]; k < rowptr[i + 1]; k++) {
      FH_REQUIRE(col[k] >= 0 && col[k] < n, "fh_mat_create_csr: column %d out of range in row %d", col[k], i);
      FH_REQUIRE(k == rowptr[i] || col[k] > col[k - 1], "fh_mat_create_csr: columns of row %d not strictly sorted", i);
    }
  }
  A->max_row = maxrow;
  // +2 padding: the streaming kernel reads (val,col) in aligned pairs and may touch one element past the end
  FH_CHECK_HIP(hipMalloc(&A->d_rowptr, ((size_t)m + 1) * sizeof(int)));
  FH_CHECK_HIP(hipMalloc(&A->d_col, ((size_t)nnz + 2) * sizeof(int)));
  FH_CHECK_HIP(hipMalloc(&A->d_val, ((size_t)nnz + 2) * sizeof(double)));
  FH_CHECK_HIP(hipMemsetAsync(A->d_col, 0, ((size_t)nnz + 2) * sizeof(int), c->stream));
  FH_CHECK_HIP(hipMemsetAsync(A->d_val, 0, ((size_t)nnz + 2) * sizeof(double), c->stream));
  FH_CHECK_HIP(hipMemcpyAsync(A->d_rowptr, rowptr, ((size_t)m + 1) * sizeof(int), hipMemcpyHostToDevice, c->stream));
  if (nnz) FH_CHECK_HIP(hipMemcpyAsync(A->d_col, col, (size_t)nnz * sizeof(int), hipMemcpyHostToDevice, c->stream));
  if (val && nnz) FH_CHECK_HIP(hipMemcpyAsync(A->d_val, val, (size_t)nnz * sizeof(double), hipMemcpyHostToDevice, c->stream));
  FH_CHECK_HIP(hipStreamSynchronize(c->stream));
  FH_TRY(fh_spmv_build_rowblocks(A));
  *out = A;
  return 0;
  FH_GUARD_END("fh_mat_create_csr")
}

int fh_mat_fetch_host_cols(fh_mat_t A) {
  A->h_col.resize((size_t)A->nnz);
  if (A->nnz) {
    FH_CHECK_HIP(hipMemcpyAsync(A->h_col.data(), A->d_col, (size_t)A->nnz * sizeof(int), hipMemcpyDeviceToHost, A->ctx->stream));
    FH_CHECK_HIP(hipStreamSynchronize(A->ctx->stream));
  }
  return 0;
}

// A matrix whose pattern is produced ON THE DEVICE: row pointers (scanned on the host) are given, the column array is allocated and left to
// the caller's kernels; values start at zero.  The host column copy is fetched only if host code asks for it (fh_hcol).  The caller
// finishes with fh_spmv_build_rowblocks once the columns are written.
int fh_mat_alloc_device_pattern(fh_ctx_t c, int m, int n, std::vector<int>&& rp, fh_mat_t* out) {
  fh_mat_t A = mat_new(c);
  A->m = m;
  A->n = n;
  A->h_rowptr = std::move(rp);
  A->nnz = A->h_rowptr[m];
  A->built_on = 1;
  int maxrow = 0;
  for (int r = 0; r < m; r++) maxrow = std::max(maxrow, A->h_rowptr[r + 1] - A->h_rowptr[r]);
  A->max_row = maxrow;
  *out = A;
  FH_CHECK_HIP(hipMalloc(&A->d_rowptr, ((size_t)m + 1) * sizeof(int)));
  FH_CHECK_HIP(hipMalloc(&A->d_col, ((size_t)A->nnz + 2) * sizeof(int)));
  FH_CHECK_HIP(hipMalloc(&A->d_val, ((size_t)A->nnz + 2) * sizeof(double)));
  FH_CHECK_HIP(hipMemsetAsync(A->d_col + A->nnz, 0, 2 * sizeof(int), c->stream));
  FH_CHECK_HIP(hipMemsetAsync(A->d_val, 0, ((size_t)A->nnz + 2) * sizeof(double), c->stream));
  FH_CHECK_HIP(hipMemcpyAsync(A->d_rowptr, A->h_rowptr.data(), ((size_t)m + 1) * sizeof(int), hipMemcpyHostToDevice, c->stream));
  return 0;
}

// ------------------------------------------------------------------------------------------------------------------
// Finite-element pattern on the DEVICE (round 4; LinearEquation::GetSparsityPatternSize + SparseMatrix::init, LinearEquation.cpp:407-548): row r
// holds the dofs of all elements around dof r.  node -> element lists by a counting pass, then one wave per row: the <= 1024 candidate
// columns into LDS, bitonic sort, distinct keys -> length (first launch) / columns (second launch).  The host only scans the row lengths;
// the column array never visits it unless host code asks (fh_hcol).  Same pattern as fh_pattern_from_elements (sorted, unique).
// ------------------------------------------------------------------------------------------------------------------
constexpr int PE_CAP = 1024;
// pad: an entry of -1 (the padding of a table whose rows have several widths) is skipped, not refused
__global__ __launch_bounds__(256) void k_pe_count(size_t n, const int* __restrict__ elem_dof, int m, int ncols, int pad, int* __restrict__ cnt, int* __restrict__ err) {
  const size_t k = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (k >= n) return;
  const int d = elem_dof[k];
  if (d == -1 && pad) return;
  if (d < 0 || d >= ncols) { atomicExch(err, 1); return; }
  if (d < m) atomicAdd(&cnt[d], 1);
}
// div = nloc: the list of a dof names the elements that hold it; div = 1: the entries of the table (element * nloc + local node)
__global__ __launch_bounds__(256) void k_pe_fill(size_t n, int div, const int* __restrict__ elem_dof, int m, int* __restrict__ cur, int* __restrict__ adj) {
  const size_t k = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (k >= n) return;
  const int d = elem_dof[k];
  if (d >= 0 && d < m) adj[atomicAdd(&cur[d], 1)] = (int)(k / div);
}

fh_dof_lists::~fh_dof_lists() {
  for (int* p : {d_ptr, d_adj, d_cur, d_err})
    if (p) hipFree(p);
}

// the counting pass: dof -> the elements (or table entries) that hold it, for the dofs < m.  The order inside a list depends on the race between the threads.
int fh_dof_lists_build(fh_ctx_t c, const char* who, size_t ne, int div, const int* d_ed, int m, int ncols, bool padded, fh_dof_lists* L) {
  FH_CHECK_HIP(hipMalloc(&L->d_cur, ((size_t)m + 2) * sizeof(int)));
  FH_CHECK_HIP(hipMalloc(&L->d_err, sizeof(int)));
  FH_CHECK_HIP(hipMemsetAsync(L->d_cur, 0, ((size_t)m + 2) * sizeof(int), c->stream));
  FH_CHECK_HIP(hipMemsetAsync(L->d_err, 0, sizeof(int), c->stream));
  const unsigned gb = (unsigned)((ne + 255) / 256);
  if (ne) hipLaunchKernelGGL(k_pe_count, dim3(gb), dim3(256), 0, c->stream, ne, d_ed, m, ncols, padded ? 1 : 0, L->d_cur, L->d_err);
  L->ptr.assign((size_t)m + 1, 0);
  if (m) FH_CHECK_HIP(hipMemcpyAsync(L->ptr.data() + 1, L->d_cur, (size_t)m * sizeof(int), hipMemcpyDeviceToHost, c->stream));
  int err = 0;
  FH_CHECK_HIP(hipMemcpyAsync(&err, L->d_err, sizeof(int), hipMemcpyDeviceToHost, c->stream));
  FH_CHECK_HIP(hipStreamSynchronize(c->stream));
  FH_REQUIRE(!err, "%s: a dof of an element is out of range", who);
  int64_t tot = 0;
  for (int r = 0; r < m; r++) {
    tot += L->ptr[r + 1];
    L->ptr[r + 1] = (int)tot;
  }
  FH_REQUIRE(tot < 2147483647ll, "%s: adjacency overflows int32", who);
  FH_CHECK_HIP(hipMalloc(&L->d_ptr, ((size_t)m + 1) * sizeof(int)));
  FH_CHECK_HIP(hipMalloc(&L->d_adj, std::max<size_t>((size_t)tot, 1) * sizeof(int)));
  FH_CHECK_HIP(hipMemcpyAsync(L->d_ptr, L->ptr.data(), ((size_t)m + 1) * sizeof(int), hipMemcpyHostToDevice, c->stream));
  FH_CHECK_HIP(hipMemcpyAsync(L->d_cur, L->ptr.data(), (size_t)m * sizeof(int), hipMemcpyHostToDevice, c->stream));        // cursors
  if (ne) hipLaunchKernelGGL(k_pe_fill, dim3(gb), dim3(256), 0, c->stream, ne, div, d_ed, m, L->d_cur, L->d_adj);
  return 0;
}
template <bool FILL>
__global__ __launch_bounds__(256) void k_pe_rows(int m, const int* __restrict__ aptr, const int* __restrict__ adj, const int* __restrict__ elem_dof, int nloc,
                                                 const int* __restrict__ rowptr, int* __restrict__ rowlen, int* __restrict__ col, int* __restrict__ err) {
  __shared__ int keys[4][PE_CAP];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int r = blockIdx.x * 4 + wave;
  if (r >= m) return;
  int* key = keys[wave];
  const int a0 = aptr[r], na = aptr[r + 1] - a0, n = na * nloc;
  if (n > PE_CAP) {
    if (lane == 0) atomicExch(err, 2);
    return;
  }
  int np = 64;
  while (np < n) np <<= 1;
  for (int k = lane; k < np; k += 64) key[k] = k < n ? elem_dof[(size_t)adj[a0 + k / nloc] * nloc + k % nloc] : 0x7fffffff;
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  for (int size = 2; size <= np; size <<= 1)
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      for (int t = lane; t < (np >> 1); t += 64) {
        const int lo = ((t / stride) * (stride << 1)) + (t % stride), hi = lo + stride;
        const bool up = ((lo & size) == 0);
        const int a = key[lo], c = key[hi];
        if ((a > c) == up) {
          key[lo] = c;
          key[hi] = a;
        }
      }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
  const int per = np >> 6, k0 = lane * per;
  int mine = 0;
  for (int k = k0; k < k0 + per && k < n; k++) mine += (k == 0 || key[k] != key[k - 1]) ? 1 : 0;
  int incl = mine;
  for (int d = 1; d < 64; d <<= 1) {
    const int v = __shfl_up(incl, d, 64);
    if (lane >= d) incl += v;
  }
  const int total = __shfl(incl, 63, 64);
  if (!FILL) {
    if (lane == 0) rowlen[r] = total;
    return;
  }
  int o = rowptr[r] + incl - mine;
  for (int k = k0; k < k0 + per && k < n; k++)
    if (k == 0 || key[k] != key[k - 1]) col[o++] = key[k];
}

// elem_dof: host array [nel * nloc], or null when dev_elem_dof -- the same array already in device memory (not owned) -- is given
int mat_create_from_elements_impl(fh_ctx_t c, int nel, int nloc, const int* elem_dof, const int* dev_elem_dof, int m, int n, fh_mat_t* out) {
  FH_GUARD_BEGIN
  FH_REQUIRE(c && out && nel >= 0 && nloc > 0 && m >= 0 && n >= m && (elem_dof || dev_elem_dof || nel == 0), "fh_mat_create_from_elements: bad arguments");
  const size_t ne = (size_t)nel * nloc;
  int *d_ed = nullptr, *d_ed_own = nullptr, *d_len = nullptr;
  auto cleanup = [&]() {
    for (int* p : {d_ed_own, d_len})
      if (p) hipFree(p);
  };
  std::vector<int> fetched;        // host copy of a device-only table, made only if the host builder has to serve a row
  if (dev_elem_dof) {
    d_ed = const_cast<int*>(dev_elem_dof);
  } else {
    FH_CHECK_HIP(hipMalloc(&d_ed_own, std::max<size_t>(ne, 1) * sizeof(int)));
    d_ed = d_ed_own;
  }
  FH_CHECK_HIP(hipMalloc(&d_len, ((size_t)m + 1) * sizeof(int)));
  if (ne && !dev_elem_dof) FH_CHECK_HIP(hipMemcpyAsync(d_ed, elem_dof, ne * sizeof(int), hipMemcpyHostToDevice, c->stream));
  fh_dof_lists L;                  // freed on return; every path below synchronises the stream first
  if (int rc = fh_dof_lists_build(c, "fh_mat_create_from_elements", ne, nloc, d_ed, m, n, false, &L)) {
    hipStreamSynchronize(c->stream);
    cleanup();
    return rc;
  }
  int* const d_aptr = L.d_ptr;
  int* const d_adj = L.d_adj;
  int* const d_err = L.d_err;
  int err = 0;
  if (m) hipLaunchKernelGGL(k_pe_rows<false>, dim3(fh_div_up(m, 4)), dim3(256), 0, c->stream, m, d_aptr, d_adj, d_ed, nloc, (const int*)nullptr, d_len, (int*)nullptr, d_err);
  std::vector<int> rp((size_t)m + 1, 0);
  if (m) FH_CHECK_HIP(hipMemcpyAsync(rp.data() + 1, d_len, (size_t)m * sizeof(int), hipMemcpyDeviceToHost, c->stream));
  FH_CHECK_HIP(hipMemcpyAsync(&err, d_err, sizeof(int), hipMemcpyDeviceToHost, c->stream));
  FH_CHECK_HIP(hipStreamSynchronize(c->stream));
  if (err) {               // a node with more than PE_CAP candidate columns: the host builder serves it
    if (!elem_dof) {
      fetched.resize(ne);
      FH_CHECK_HIP(hipMemcpy(fetched.data(), d_ed, ne * sizeof(int), hipMemcpyDeviceToHost));
      elem_dof = fetched.data();
    }
    cleanup();
    std::vector<int> hrp((size_t)n + 1), hcol;
    FH_TRY(fh_pattern_from_elements(nel, nloc, elem_dof, n, hrp.data(), nullptr));
    hcol.resize((size_t)hrp[n]);
    FH_TRY(fh_pattern_from_elements(nel, nloc, elem_dof, n, hrp.data(), hcol.data()));
    FH_TRY(fh_mat_create_csr(c, m, n, hrp.data(), hcol.data(), nullptr, out));
    (*out)->built_on = 2;
    return 0;
  }
  int64_t tot = 0;
  for (int r = 0; r < m; r++) {
    tot += rp[r + 1];
    rp[r + 1] = (int)tot;
  }
  if (tot >= 2147483647ll) {
    cleanup();
    fh_set_error("fh_mat_create_from_elements: nnz overflows int32");
    return 2;
  }
  fh_mat_t A = nullptr;
  if (fh_mat_alloc_device_pattern(c, m, n, std::move(rp), &A)) {
    cleanup();
    fh_mat_destroy(A);
    return 2;
  }
  if (m) hipLaunchKernelGGL(k_pe_rows<true>, dim3(fh_div_up(m, 4)), dim3(256), 0, c->stream, m, d_aptr, d_adj, d_ed, nloc, A->d_rowptr, (int*)nullptr, A->d_col, d_err);
  FH_CHECK_HIP(hipGetLastError());
  FH_CHECK_HIP(hipStreamSynchronize(c->stream));
  cleanup();
  FH_TRY(fh_spmv_build_rowblocks(A));
  *out = A;
  return 0;
  FH_GUARD_END("fh_mat_create_from_elements")
}

extern "C" int fh_mat_create_from_elements(fh_ctx_t c, int nel, int nloc, const int* elem_dof, int m, int n, fh_mat_t* out) {
  FH_REQUIRE(elem_dof || nel == 0, "fh_mat_create_from_elements: bad arguments");
  return mat_create_from_elements_impl(c, nel, nloc, elem_dof, nullptr, m, n, out);
}

int fh_mesh_host_arrays(fh_mesh_t m, int* dim, int* geom, int* nel, int* nnode, int* nloc, int* n_linear, const int** elem_dof, const double** coords);

extern "C" int fh_mat_create_from_mesh(fh_ctx_t c, fh_mesh_t mesh, int fe, fh_mat_t* out) {
  FH_REQUIRE(c && mesh && out && fe >= 0 && fe <= 3, "fh_mat_create_from_mesh: bad arguments (fe: 0 linear, 1 serendipity, 2 biquadratic, 3 piecewise constant)");
  int dim, geom, nel, nnode, nloc, nlin;
  const int* ed;
  const double* xy;
  FH_TRY(fh_mesh_host_arrays(mesh, &dim, &geom, &nel, &nnode, &nloc, &nlin, &ed, &xy));
  if (fe == 3) {       // element-owned dofs: every element couples with itself only
    std::vector<int> iota(nel);
    for (int e = 0; e < nel; e++) iota[e] = e;
    return mat_create_from_elements_impl(c, nel, 1, iota.data(), nullptr, nel, nel, out);
  }
  fh_mesh_dev* dev = nullptr;
  FH_TRY(fh_mesh_device(c, mesh, &dev));
  if (fe == 2) return mat_create_from_elements_impl(c, nel, nloc, nullptr, dev->d_elem_dof, nnode, nnode, out);
  // linear / serendipity: the family's nodes are the first 2^dim (4 / 8) resp. vertex + edge (8 / 20) local nodes of every element -- a strided copy of the
  // table -- and own the leading node ids (Mesh::GetSolutionDof, Mesh.cpp:1026-1050)
  int own[3] = {0, 0, 0};
  FH_TRY(fh_mesh_info(mesh, nullptr, nullptr, nullptr, nullptr, own, nullptr));
  const int nv = fe == 0 ? 1 << dim : (dim == 3 ? 20 : 8);
  if (fe == 1) nlin = own[1];
  int* d_lin = nullptr;
  FH_CHECK_HIP(hipMalloc(&d_lin, std::max<size_t>((size_t)nel * nv, 1) * sizeof(int)));
  hipError_t e = nel ? hipMemcpy2DAsync(d_lin, nv * sizeof(int), dev->d_elem_dof, nloc * sizeof(int), nv * sizeof(int), nel, hipMemcpyDeviceToDevice, c->stream) : hipSuccess;
  int rc = e == hipSuccess ? mat_create_from_elements_impl(c, nel, nv, nullptr, d_lin, nlin, nlin, out) : 1;
  if (e != hipSuccess) fh_set_error("fh_mat_create_from_mesh: %s", hipGetErrorString(e));
  hipStreamSynchronize(c->stream);
  hipFree(d_lin);
  return rc;
}

extern "C" int fh_mat_destroy(fh_mat_t A) {
  if (!A) return 0;
  {
    LiveMats& L = live_mats();
    std::lock_guard<std::mutex> g(L.mutex);
    L.map.erase(A->uid);
  }
  hipStreamSynchronize(A->ctx->stream);
  fh_stage_free(A->stage);
  if (A->plan && A->plan_destroy) A->plan_destroy(A->plan);
  if (A->At) fh_mat_destroy(A->At);
  if (A->d_tperm) hipFree(A->d_tperm);
  if (A->d_rowptr) hipFree(A->d_rowptr);
  if (A->d_col) hipFree(A->d_col);
  if (A->d_val) hipFree(A->d_val);
  fh_spmv_free(A->spmv);
  if (A->d_diagpos) hipFree(A->d_diagpos);
  delete A;
  return 0;
}

extern "C" int fh_mat_size(fh_mat_t A, int* m, int* n, int* nnz) {
  if (m) *m = A->m;
  if (n) *n = A->n;
  if (nnz) *nnz = A->nnz;
  return 0;
}

extern "C" int fh_mat_built_on(fh_mat_t A, int* how) {
  FH_REQUIRE(A && how, "fh_mat_built_on: null argument");
  *how = A->built_on;
  return 0;
}

extern "C" int fh_mat_dev_ptrs(fh_mat_t A, const int** rowptr, const int** col, const double** val) {
  FH_REQUIRE(A, "fh_mat_dev_ptrs: null matrix");
  if (rowptr) *rowptr = A->d_rowptr;
  if (col) *col = A->d_col;
  if (val) *val = A->d_val;
  return 0;
}

extern "C" int fh_mat_zero(fh_mat_t A) {
  FH_REQUIRE(A, "fh_mat_zero: null matrix");
  FH_CHECK_HIP(hipMemsetAsync(A->d_val, 0, (size_t)A->nnz * sizeof(double), A->ctx->stream));
  fh_mat_values_written(A);
  return 0;
}

extern "C" int fh_mat_set_values_csr(fh_mat_t A, const double* val) {
  FH_REQUIRE(A && (val || A->nnz == 0), "fh_mat_set_values_csr: null argument");
  fh_mat_values_written(A);
  FH_CHECK_HIP(hipMemcpyAsync(A->d_val, val, (size_t)A->nnz * sizeof(double), hipMemcpyHostToDevice, A->ctx->stream));
  FH_CHECK_HIP(hipStreamSynchronize(A->ctx->stream));
  return 0;
}

extern "C" int fh_mat_get_values_csr(fh_mat_t A, double* val) {
  FH_CHECK_HIP(hipMemcpyAsync(val, A->d_val, (size_t)A->nnz * sizeof(double), hipMemcpyDeviceToHost, A->ctx->stream));
  FH_CHECK_HIP(hipStreamSynchronize(A->ctx->stream));
  return 0;
}

extern "C" int fh_mat_get_pattern(fh_mat_t A, int* rowptr, int* col) {
  if (rowptr) memcpy(rowptr, A->h_rowptr.data(), ((size_t)A->m + 1) * sizeof(int));
  if (col) memcpy(col, fh_hcol(A).data(), (size_t)A->nnz * sizeof(int));
  return 0;
}

// ------------------------------------------------------------------------------------------------
// per-element crossings of the reference interface (slow path; the batched assembler is the fast one)
// ------------------------------------------------------------------------------------------------
static int host_find(const fh_mat_t A, int row, int c) {
  const int* b = fh_hcol(A).data() + A->h_rowptr[row];
  const int* e = fh_hcol(A).data() + A->h_rowptr[row + 1];
  const int* p = std::lower_bound(b, e, c);
  if (p == e || *p != c) return -1;
  return (int)(p - fh_hcol(A).data());
}

__global__ void k_apply_entries(double* __restrict__ val, const int* __restrict__ pos, const double* __restrict__ v, int n, int add) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n && pos[i] >= 0) {
    if (add) atomicAdd(&val[pos[i]], v[i]);
    else val[pos[i]] = v[i];
  }
}

static int apply_entries(fh_mat_t A, const std::vector<int>& pos, const double* vals, int add) {
  fh_ctx_t c = A->ctx;
  int n = (int)pos.size();
  if (!n) return 0;
  int* d_pos = nullptr;
  double* d_v = nullptr;
  FH_CHECK_HIP(hipMalloc(&d_pos, n * sizeof(int)));
  FH_CHECK_HIP(hipMalloc(&d_v, n * sizeof(double)));
  FH_CHECK_HIP(hipMemcpyAsync(d_pos, pos.data(), n * sizeof(int), hipMemcpyHostToDevice, c->stream));
  FH_CHECK_HIP(hipMemcpyAsync(d_v, vals, n * sizeof(double), hipMemcpyHostToDevice, c->stream));
  hipLaunchKernelGGL(k_apply_entries, dim3(fh_div_up(n, 256)), dim3(256), 0, c->stream, A->d_val, d_pos, d_v, n, add);
  FH_CHECK_HIP(hipGetLastError());
  FH_CHECK_HIP(hipStreamSynchronize(c->stream));
  hipFree(d_pos);
  hipFree(d_v);
  fh_mat_values_written(A);
  return 0;
}

// immediate form of the staged add (fh_stage.hip): the block is on the device when the call returns
extern "C" int fh_mat_add_block(fh_mat_t A, int nrow, const int* rows, int ncol, const int* cols, const double* vals) {
  FH_TRY(fh_mat_stage_block(A, nrow, rows, ncol, cols, vals));
  return fh_mat_flush(A);
}

extern "C" int fh_mat_insert_row(fh_mat_t A, int row, int ncols, const int* cols, const double* vals) {
  FH_REQUIRE(A, "fh_mat_insert_row: null matrix");
  FH_REQUIRE(row >= 0 && row < A->m, "fh_mat_insert_row: row %d out of range", row);
  std::vector<int> pos(ncols);
  for (int j = 0; j < ncols; j++) {
    pos[j] = host_find(A, row, cols[j]);
    FH_REQUIRE(pos[j] >= 0, "fh_mat_insert_row: entry (%d,%d) is outside the pattern", row, cols[j]);
  }
  return apply_entries(A, pos, vals, 0);
}

extern "C" int fh_mat_get_row(fh_mat_t A, int row, int* ncols, int* cols, double* vals) {
  FH_REQUIRE(row >= 0 && row < A->m, "fh_mat_get_row: row %d out of range", row);
  int s = A->h_rowptr[row], e = A->h_rowptr[row + 1];
  if (ncols) *ncols = e - s;
  if (cols) memcpy(cols, fh_hcol(A).data() + s, (size_t)(e - s) * sizeof(int));
  if (vals && e > s) {
    FH_CHECK_HIP(hipMemcpyAsync(vals, A->d_val + s, (size_t)(e - s) * sizeof(double), hipMemcpyDeviceToHost, A->ctx->stream));
    FH_CHECK_HIP(hipStreamSynchronize(A->ctx->stream));
  }
  return 0;
}

// ------------------------------------------------------------------------------------------------
// K5: Dirichlet rows / columns
// ------------------------------------------------------------------------------------------------
// two rows per wave (32 lanes each: a Q2 row has 27 ... 125 entries), four waves per workgroup
__global__ __launch_bounds__(256) void k_zero_rows(const int* __restrict__ rowptr, const int* __restrict__ col, double* __restrict__ val,
                                                   const int* __restrict__ rows, int nrows, double diag) {
  const int r = blockIdx.x * 8 + (threadIdx.x >> 5), lane = threadIdx.x & 31;
  if (r >= nrows) return;
  const int row = rows[r];
  const int e = rowptr[row + 1];
  for (int k = rowptr[row] + lane; k < e; k += 32) val[k] = (col[k] == row) ? diag : 0.0;
}

__global__ __launch_bounds__(256) void k_mask_set(unsigned char* __restrict__ mask, const int* __restrict__ idx, int n) {
  int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) mask[idx[i]] = 1;
}

__global__ __launch_bounds__(256) void k_zero_cols(const int* __restrict__ col, double* __restrict__ val, const unsigned char* __restrict__ mask, int nnz) {
  for (int k = blockIdx.x * 256 + threadIdx.x; k < nnz; k += gridDim.x * 256)
    if (mask[col[k]]) val[k] = 0.0;
}

extern "C" int fh_mat_zero_rows(fh_mat_t A, int n, const int* rows, double diag) {
  if (n <= 0) return 0;
  fh_ctx_t c = A->ctx;
  for (int i = 0; i < n; i++) FH_REQUIRE(rows[i] >= 0 && rows[i] < A->m, "fh_mat_zero_rows: row %d out of range", rows[i]);
  int* d_rows = nullptr;
  FH_CHECK_HIP(hipMalloc(&d_rows, n * sizeof(int)));
  FH_CHECK_HIP(hipMemcpyAsync(d_rows, rows, n * sizeof(int), hipMemcpyHostToDevice, c->stream));
  hipLaunchKernelGGL(k_zero_rows, dim3(fh_div_up(n, 8)), dim3(256), 0, c->stream, A->d_rowptr, A->d_col, A->d_val, d_rows, n, diag);
  FH_CHECK_HIP(hipGetLastError());
  FH_CHECK_HIP(hipStreamSynchronize(c->stream));
  hipFree(d_rows);
  fh_mat_rows_replaced(A);
  return 0;
}

// ---- device-resident index list: the result of BuildBdcIndex (LinearEquationSolverPetsc.cpp:53-90) is built once per level
// (_bdcIndexIsInitialized) and reused by SetPenalty / ZerosBoundaryResiduals at every assembly; kept on the device, these two
// calls need no host traffic and no synchronisation
struct fh_index_s {
  fh_ctx_t ctx = nullptr;
  int n = 0, max_index = -1;
  bool has_negative = false;     // -1 entries are allowed for gather maps ("no source": the target gets 0)
  int* d = nullptr;
};

extern "C" int fh_index_create(fh_ctx_t ctx, int n, const int* idx, fh_index_t* out) {
  FH_REQUIRE(ctx && out && n >= 0 && (n == 0 || idx), "fh_index_create: bad arguments");
  fh_index_s* x = new fh_index_s();
  x->ctx = ctx;
  x->n = n;
  for (int i = 0; i < n; i++) {
    FH_REQUIRE(idx[i] >= -1, "fh_index_create: index %d (only -1 is allowed as 'none')", idx[i]);
    if (idx[i] < 0) x->has_negative = true;
    x->max_index = std::max(x->max_index, idx[i]);
  }
  FH_CHECK_HIP(hipMalloc(&x->d, std::max(n, 1) * sizeof(int)));
  if (n) FH_CHECK_HIP(hipMemcpy(x->d, idx, (size_t)n * sizeof(int), hipMemcpyHostToDevice));
  *out = x;
  return 0;
}

extern "C" int fh_index_destroy(fh_index_t x) {
  if (!x) return 0;
  hipStreamSynchronize(x->ctx->stream);
  hipFree(x->d);
  delete x;
  return 0;
}

extern "C" int fh_mat_zero_rows_index(fh_mat_t A, fh_index_t rows, double diag) {
  FH_REQUIRE(A && rows, "fh_mat_zero_rows_index: null argument");
  FH_REQUIRE(!rows->has_negative, "fh_mat_zero_rows_index: the list holds 'none' entries");
  FH_REQUIRE(rows->max_index < A->m, "fh_mat_zero_rows_index: row %d out of range", rows->max_index);
  if (rows->n == 0) return 0;
  hipLaunchKernelGGL(k_zero_rows, dim3(fh_div_up(rows->n, 8)), dim3(256), 0, A->ctx->stream, A->d_rowptr, A->d_col, A->d_val, rows->d, rows->n, diag);
  FH_CHECK_HIP(hipGetLastError());
  fh_mat_rows_replaced(A);
  return 0;
}

__global__ __launch_bounds__(256) void k_set_index(double* __restrict__ v, const int* __restrict__ idx, int n, double value) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) v[idx[i]] = value;
}

extern "C" int fh_vec_set_index(fh_vec_t v, fh_index_t idx, double value) {
  FH_REQUIRE(v && idx, "fh_vec_set_index: null argument");
  FH_REQUIRE(!idx->has_negative, "fh_vec_set_index: the list holds 'none' entries");
  FH_REQUIRE(idx->max_index < v->n_local, "fh_vec_set_index: index %d is not an owned entry", idx->max_index);
  if (idx->n == 0) return 0;
  hipLaunchKernelGGL(k_set_index, dim3(fh_div_up(idx->n, 256)), dim3(256), 0, v->ctx->stream, v->d, idx->d, idx->n, value);
  FH_CHECK_HIP(hipGetLastError());
  return 0;
}

// gathers along a device-resident map: dst[k] = (map[k] >= 0) ? src[map[k]] : 0.  Used to take the owned rows of an operator that
// was assembled / projected on a rank's extended box (adaptive levels on several ranks) without host traffic.
__global__ __launch_bounds__(256) void k_gather_map(double* __restrict__ dst, const double* __restrict__ src, const int* __restrict__ map, int n) {
  for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
    const int j = map[i];
    dst[i] = (j >= 0) ? src[j] : 0.0;
  }
}

extern "C" int fh_mat_gather_values(fh_mat_t dst, fh_mat_t src, fh_index_t map) {
  FH_REQUIRE(dst && src && map, "fh_mat_gather_values: null argument");
  FH_REQUIRE(map->n == dst->nnz && map->max_index < src->nnz, "fh_mat_gather_values: map has %d entries (target nnz %d), largest source %d (source nnz %d)",
             map->n, dst->nnz, map->max_index, src->nnz);
  if (dst->nnz == 0) return 0;
  const int nb = std::min(fh_div_up(dst->nnz, 256), dst->ctx->num_cu * 16);
  hipLaunchKernelGGL(k_gather_map, dim3(nb), dim3(256), 0, dst->ctx->stream, dst->d_val, src->d_val, map->d, dst->nnz);
  FH_CHECK_HIP(hipGetLastError());
  fh_mat_values_written(dst);
  return 0;
}

// ---- owned-row operators of a domain-decomposed level, built on the device from the operator of the rank's extended box ----------
// The reference's multi-rank matrices hold the rows a rank owns over [owned | ghost] columns (MPIAIJ behind PetscMatrix::init,
// PetscMatrix.cpp:162-203; ghost lists LinearEquation.cpp:239-280).  Here the rank's complete local operator already lives on the
// device; these entry points cut the owned rows out of it: integer pattern work on the host copies of the pattern, values by a
// device gather along a map that is kept, so that every re-preparation (new values, same pattern) is one kernel per operator.

// mask[c] = 1 for every column that one of the listed rows touches (the halo a set of owned rows reads)
extern "C" int fh_mat_col_mask(fh_mat_t A, int nrows, const int* rows, unsigned char* mask /* [A->n], or-ed into */) {
  FH_REQUIRE(A && mask && nrows >= 0 && (nrows == 0 || rows), "fh_mat_col_mask: bad arguments");
  for (int i = 0; i < nrows; i++) {
    const int r = rows[i];
    FH_REQUIRE(r >= 0 && r < A->m, "fh_mat_col_mask: row %d out of range", r);
    for (int k = A->h_rowptr[r]; k < A->h_rowptr[r + 1]; k++) mask[fh_hcol(A)[k]] = 1;
  }
  return 0;
}

// rowmask[r] = 1 for every row with an entry in a masked column (the rows a transposed operator restricted to those columns reads)
extern "C" int fh_mat_row_mask(fh_mat_t A, const unsigned char* colmask /* [A->n] */, unsigned char* rowmask /* [A->m], or-ed into */) {
  FH_REQUIRE(A && colmask && rowmask, "fh_mat_row_mask: null argument");
  for (int r = 0; r < A->m; r++) {
    if (rowmask[r]) continue;
    for (int k = A->h_rowptr[r]; k < A->h_rowptr[r + 1]; k++)
      if (colmask[fh_hcol(A)[k]]) {
        rowmask[r] = 1;
        break;
      }
  }
  return 0;
}

// map[k] for every non-zero k = (r, c) of dst: position of (src_row[r], src_col[c]) in src, or -1 when src has no such entry
// (NULL row / column lists = identity).  Feeds fh_mat_gather_values.
extern "C" int fh_mat_value_map(fh_mat_t dst, fh_mat_t src, const int* src_row, const int* src_col, fh_index_t* out) {
  FH_GUARD_BEGIN
  FH_REQUIRE(dst && src && out, "fh_mat_value_map: null argument");
  std::vector<int> map((size_t)dst->nnz, -1);
  for (int r = 0; r < dst->m; r++) {
    const int sr = src_row ? src_row[r] : r;
    if (sr < 0) continue;
    FH_REQUIRE(sr < src->m, "fh_mat_value_map: source row %d out of range", sr);
    const int* b = fh_hcol(src).data() + src->h_rowptr[sr];
    const int* e = fh_hcol(src).data() + src->h_rowptr[sr + 1];
    for (int k = dst->h_rowptr[r]; k < dst->h_rowptr[r + 1]; k++) {
      const int sc = src_col ? src_col[fh_hcol(dst)[k]] : fh_hcol(dst)[k];
      if (sc < 0) continue;
      const int* q = std::lower_bound(b, e, sc);
      if (q != e && *q == sc) map[k] = (int)(q - fh_hcol(src).data());
    }
  }
  return fh_index_create(dst->ctx, dst->nnz, map.data(), out);
  FH_GUARD_END("fh_mat_value_map")
}

// dst = the listed rows of src (in list order) with columns renumbered by newcol[src->n] (entries whose new column is < 0 are
// dropped -- they must hold zeros, which fh_mat_restrict_check verifies on the device); *map as in fh_mat_value_map, values gathered
extern "C" int fh_mat_restrict(fh_mat_t src, int nrows, const int* rows, const int* newcol, int ncols_new, fh_mat_t* out, fh_index_t* map_out) {
  FH_GUARD_BEGIN
  FH_REQUIRE(src && out && map_out && newcol && nrows >= 0 && (nrows == 0 || rows) && ncols_new >= 0, "fh_mat_restrict: bad arguments");
  std::vector<int> rp(nrows + 1, 0);
  for (int i = 0; i < nrows; i++) {
    const int r = rows[i];
    FH_REQUIRE(r >= 0 && r < src->m, "fh_mat_restrict: row %d out of range", r);
    int cnt = 0;
    for (int k = src->h_rowptr[r]; k < src->h_rowptr[r + 1]; k++) {
      const int c = newcol[fh_hcol(src)[k]];
      FH_REQUIRE(c < ncols_new, "fh_mat_restrict: new column %d out of range (%d columns)", c, ncols_new);
      cnt += c >= 0;
    }
    rp[i + 1] = rp[i] + cnt;
  }
  std::vector<int> col((size_t)rp[nrows]), map((size_t)rp[nrows]);
  std::vector<std::pair<int, int>> buf;
  for (int i = 0; i < nrows; i++) {
    const int r = rows[i];
    buf.clear();
    for (int k = src->h_rowptr[r]; k < src->h_rowptr[r + 1]; k++) {
      const int c = newcol[fh_hcol(src)[k]];
      if (c >= 0) buf.emplace_back(c, k);
    }
    std::sort(buf.begin(), buf.end());
    for (size_t t = 0; t < buf.size(); t++) {
      FH_REQUIRE(t == 0 || buf[t].first != buf[t - 1].first, "fh_mat_restrict: two columns of row %d map to the same new column", r);
      col[rp[i] + t] = buf[t].first;
      map[rp[i] + t] = buf[t].second;
    }
  }
  fh_mat_t D = nullptr;
  FH_TRY(fh_mat_create_csr(src->ctx, nrows, ncols_new, rp.data(), col.data(), nullptr, &D));
  fh_index_t M = nullptr;
  int rc = fh_index_create(src->ctx, (int)map.size(), map.data(), &M);
  if (rc) {
    fh_mat_destroy(D);
    return rc;
  }
  rc = fh_mat_gather_values(D, src, M);
  if (rc) {
    fh_mat_destroy(D);
    fh_index_destroy(M);
    return rc;
  }
  *out = D;
  *map_out = M;
  return 0;
  FH_GUARD_END("fh_mat_restrict")
}

// largest |value| among the entries of the listed rows of src that fh_mat_restrict drops (new column < 0): must be 0 for the owned
// rows of a level operator -- an owned row reads nothing outside its halo
__global__ __launch_bounds__(256) void k_dropped_max(const int* __restrict__ rowptr, const int* __restrict__ col, const double* __restrict__ val,
                                                     const int* __restrict__ rows, int nrows, const int* __restrict__ newcol, double* __restrict__ out) {
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  double mx = 0.0;
  if (i < nrows) {
    const int r = rows[i];
    for (int k = rowptr[r] + lane; k < rowptr[r + 1]; k += 64)
      if (newcol[col[k]] < 0) mx = fmax(mx, fabs(val[k]));
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) mx = fmax(mx, __shfl_xor(mx, off, 64));
  if (lane == 0 && mx > 0.0) atomicMax(reinterpret_cast<unsigned long long*>(out), (unsigned long long)__double_as_longlong(mx));   // positive doubles order like integers
}

extern "C" int fh_mat_restrict_check(fh_mat_t src, int nrows, const int* rows, const int* newcol, double* max_dropped) {
  FH_REQUIRE(src && newcol && max_dropped && nrows >= 0 && (nrows == 0 || rows), "fh_mat_restrict_check: bad arguments");
  *max_dropped = 0.0;
  for (int i = 0; i < nrows; i++) FH_REQUIRE(rows[i] >= 0 && rows[i] < src->m, "fh_mat_restrict_check: row %d out of range", rows[i]);
  if (nrows == 0) return 0;
  fh_ctx_t c = src->ctx;
  int *d_rows = nullptr, *d_new = nullptr;
  double* d_out = nullptr;
  FH_CHECK_HIP(hipMalloc(&d_rows, (size_t)nrows * sizeof(int)));
  FH_CHECK_HIP(hipMalloc(&d_new, (size_t)std::max(src->n, 1) * sizeof(int)));
  FH_CHECK_HIP(hipMalloc(&d_out, sizeof(double)));
  FH_CHECK_HIP(hipMemcpyAsync(d_rows, rows, (size_t)nrows * sizeof(int), hipMemcpyHostToDevice, c->stream));
  FH_CHECK_HIP(hipMemcpyAsync(d_new, newcol, (size_t)src->n * sizeof(int), hipMemcpyHostToDevice, c->stream));
  FH_CHECK_HIP(hipMemsetAsync(d_out, 0, sizeof(double), c->stream));
  hipLaunchKernelGGL(k_dropped_max, dim3(fh_div_up(nrows, 4)), dim3(256), 0, c->stream, src->d_rowptr, src->d_col, src->d_val, d_rows, nrows, d_new, d_out);
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) e = hipMemcpyAsync(max_dropped, d_out, sizeof(double), hipMemcpyDeviceToHost, c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  hipFree(d_rows);
  hipFree(d_new);
  hipFree(d_out);
  FH_CHECK_HIP(e);
  return 0;
}

extern "C" int fh_vec_gather(fh_vec_t dst, fh_vec_t src, fh_index_t map) {
  FH_REQUIRE(dst && src && map, "fh_vec_gather: null argument");
  FH_REQUIRE(map->n <= dst->n_local + dst->nghost && map->max_index < src->n_local + src->nghost, "fh_vec_gather: map does not fit the vectors");
  if (map->n == 0) return 0;
  const int nb = std::min(fh_div_up(map->n, 256), dst->ctx->num_cu * 16);
  hipLaunchKernelGGL(k_gather_map, dim3(nb), dim3(256), 0, dst->ctx->stream, dst->d, src->d, map->d, map->n);
  FH_CHECK_HIP(hipGetLastError());
  return 0;
}

extern "C" int fh_mat_zero_cols(fh_mat_t A, int n, const int* cols) {
  FH_REQUIRE(A, "fh_mat_zero_cols: null matrix");
  if (n <= 0 || A->nnz == 0) return 0;
  fh_ctx_t c = A->ctx;
  for (int i = 0; i < n; i++) FH_REQUIRE(cols[i] >= 0 && cols[i] < A->n, "fh_mat_zero_cols: column %d out of range", cols[i]);
  int* d_idx = nullptr;
  unsigned char* d_mask = nullptr;
  FH_CHECK_HIP(hipMalloc(&d_idx, n * sizeof(int)));
  FH_CHECK_HIP(hipMalloc(&d_mask, (size_t)A->n));
  FH_CHECK_HIP(hipMemsetAsync(d_mask, 0, (size_t)A->n, c->stream));
  FH_CHECK_HIP(hipMemcpyAsync(d_idx, cols, n * sizeof(int), hipMemcpyHostToDevice, c->stream));
  hipLaunchKernelGGL(k_mask_set, dim3(fh_div_up(n, 256)), dim3(256), 0, c->stream, d_mask, d_idx, n);
  int nb = std::min(fh_div_up(A->nnz, 256), c->num_cu * 8);
  hipLaunchKernelGGL(k_zero_cols, dim3(nb), dim3(256), 0, c->stream, A->d_col, A->d_val, d_mask, A->nnz);
  FH_CHECK_HIP(hipGetLastError());
  FH_CHECK_HIP(hipStreamSynchronize(c->stream));
  hipFree(d_idx);
  hipFree(d_mask);
  fh_mat_values_written(A);
  return 0;
}

// position of the diagonal entry of every row (-1: none), once per matrix: the pattern of a matrix never changes after its creation
__global__ __launch_bounds__(256) void k_diag_pos(const int* __restrict__ rowptr, const int* __restrict__ col, int* __restrict__ pos, int m) {
  int r = blockIdx.x * 256 + threadIdx.x;
  if (r >= m) return;
  int lo = rowptr[r], hi = rowptr[r + 1] - 1, p = -1;
  while (lo <= hi) {  // sorted columns
    int mid = lo + ((hi - lo) >> 1);   // (lo + hi) overflows beyond 2^30 non-zeros
    int cc = col[mid];
    if (cc == r) { p = mid; break; }
    if (cc < r) lo = mid + 1; else hi = mid - 1;
  }
  pos[r] = p;
}

__global__ __launch_bounds__(256) void k_get_diag(const int* __restrict__ pos, const double* __restrict__ val, double* __restrict__ d, int m, int invert) {
  int r = blockIdx.x * 256 + threadIdx.x;
  if (r >= m) return;
  const int p = pos[r];
  double v = p >= 0 ? val[p] : 0.0;
  if (invert) v = (v == 0.0) ? 1.0 : 1.0 / v;   // PCJACOBI: zero diagonal -> 1
  d[r] = v;
}

// the first `count` <= m rows
static int dev_get_diag(fh_mat_t A, double* d, int count, int invert) {
  if (count == 0) return 0;
  if (!A->d_diagpos) {
    FH_CHECK_HIP(hipMalloc(&A->d_diagpos, (size_t)A->m * sizeof(int)));
    hipLaunchKernelGGL(k_diag_pos, dim3(fh_div_up(A->m, 256)), dim3(256), 0, A->ctx->stream, A->d_rowptr, A->d_col, A->d_diagpos, A->m);
  }
  hipLaunchKernelGGL(k_get_diag, dim3(fh_div_up(count, 256)), dim3(256), 0, A->ctx->stream, A->d_diagpos, A->d_val, d, count, invert);
  FH_CHECK_HIP(hipGetLastError());
  return 0;
}

int fh_dev_get_diag(fh_mat_t A, double* d, int invert) { return dev_get_diag(A, d, A->m, invert); }

// the min(m, n) entries a rectangular matrix has a diagonal for: a tall matrix (a prolongator) writes nothing for its rows from n on
extern "C" int fh_mat_get_diagonal(fh_mat_t A, fh_vec_t d) {
  FH_REQUIRE(A && d, "fh_mat_get_diagonal: null argument");
  const int count = std::min(A->m, A->n);
  FH_REQUIRE(d->n_local >= count, "fh_mat_get_diagonal: vector too short");
  return dev_get_diag(A, d->d, count, 0);
}

// ------------------------------------------------------------------------------------------------
// transpose: symbolic part on the host (integer setup work), values gathered on the device
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_gather_perm(double* __restrict__ dst, const double* __restrict__ src, const int* __restrict__ perm, int n) {
  for (int k = blockIdx.x * 256 + threadIdx.x; k < n; k += gridDim.x * 256) dst[k] = src[perm[k]];
}

static int build_transpose_host(fh_mat_t A, fh_mat_t* out, int** d_perm_out) {
  const int m = A->m, n = A->n, nnz = A->nnz;
  std::vector<int> trp(n + 1, 0), tcol(nnz), perm(nnz);
  for (int k = 0; k < nnz; k++) trp[fh_hcol(A)[k] + 1]++;
  for (int j = 0; j < n; j++) trp[j + 1] += trp[j];
  std::vector<int> cur(trp.begin(), trp.end() - 1);
  for (int i = 0; i < m; i++)
    for (int k = A->h_rowptr[i]; k < A->h_rowptr[i + 1]; k++) {
      int p = cur[fh_hcol(A)[k]]++;
      tcol[p] = i;   // rows visited in increasing order => sorted columns in the transpose
      perm[p] = k;
    }
  fh_mat_t At = nullptr;
  FH_TRY(fh_mat_create_csr(A->ctx, n, m, trp.data(), tcol.data(), nullptr, &At));
  At->built_on = 2;
  int* d_perm = nullptr;
  FH_CHECK_HIP(hipMalloc(&d_perm, std::max(nnz, 1) * sizeof(int)));
  if (nnz) FH_CHECK_HIP(hipMemcpy(d_perm, perm.data(), nnz * sizeof(int), hipMemcpyHostToDevice));
  *out = At;
  *d_perm_out = d_perm;
  FH_TRACE("build_transpose: %d x %d, %d non-zeros", m, n, nnz);
  return 0;
}

// the same on the DEVICE (round 4): column counts by a counting pass, the host scans them, entries dropped into their transposed row through an
// atomic cursor and every transposed row (<= TR_CAP entries) sorted by its column (= the source row) in LDS, the position in the source riding
// along -- identical pattern and permutation as the host loop (which visits the rows in ascending order); longer rows: the host loop.
constexpr int TR_CAP = 1024;
__global__ __launch_bounds__(256) void k_tr_count(int nnz, const int* __restrict__ col, int* __restrict__ cnt) {
  for (int k = blockIdx.x * 256 + threadIdx.x; k < nnz; k += gridDim.x * 256) atomicAdd(&cnt[col[k]], 1);
}
__global__ __launch_bounds__(256) void k_tr_fill(int m, const int* __restrict__ rowptr, const int* __restrict__ col, int* __restrict__ cur, int* __restrict__ tcol,
                                                 int* __restrict__ perm) {
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (i >= m) return;
  for (int k = rowptr[i] + lane; k < rowptr[i + 1]; k += 64) {
    const int p = atomicAdd(&cur[col[k]], 1);
    tcol[p] = i;
    perm[p] = k;
  }
}
__global__ __launch_bounds__(256) void k_tr_sort(int n, const int* __restrict__ trp, int* __restrict__ tcol, int* __restrict__ perm) {
  __shared__ int keys[4][TR_CAP], pay[4][TR_CAP];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int j = blockIdx.x * 4 + wave;
  if (j >= n) return;
  const int s = trp[j], len = trp[j + 1] - s;
  if (len <= 1) return;
  int *key = keys[wave], *val = pay[wave];
  int np = 64;
  while (np < len) np <<= 1;
  for (int k = lane; k < np; k += 64) {
    key[k] = k < len ? tcol[s + k] : 0x7fffffff;
    val[k] = k < len ? perm[s + k] : 0;
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  for (int size = 2; size <= np; size <<= 1)
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      for (int t = lane; t < (np >> 1); t += 64) {
        const int lo = ((t / stride) * (stride << 1)) + (t % stride), hi = lo + stride;
        const bool up = ((lo & size) == 0);
        const int a = key[lo], c = key[hi];
        if ((a > c) == up) {
          key[lo] = c;
          key[hi] = a;
          const int v = val[lo];
          val[lo] = val[hi];
          val[hi] = v;
        }
      }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
  for (int k = lane; k < len; k += 64) {
    tcol[s + k] = key[k];
    perm[s + k] = val[k];
  }
}

static int build_transpose(fh_mat_t A, fh_mat_t* out, int** d_perm_out) {
  const int m = A->m, n = A->n, nnz = A->nnz;
  fh_ctx_t c = A->ctx;
  if (nnz == 0) return build_transpose_host(A, out, d_perm_out);
  int* d_cnt = nullptr;
  FH_CHECK_HIP(hipMalloc(&d_cnt, ((size_t)n + 1) * sizeof(int)));
  FH_CHECK_HIP(hipMemsetAsync(d_cnt, 0, ((size_t)n + 1) * sizeof(int), c->stream));
  hipLaunchKernelGGL(k_tr_count, dim3(std::min(fh_div_up(nnz, 256), c->num_cu * 16)), dim3(256), 0, c->stream, nnz, A->d_col, d_cnt);
  std::vector<int> trp((size_t)n + 1, 0);
  FH_CHECK_HIP(hipMemcpyAsync(trp.data() + 1, d_cnt, (size_t)n * sizeof(int), hipMemcpyDeviceToHost, c->stream));
  FH_CHECK_HIP(hipStreamSynchronize(c->stream));
  int maxrow = 0;
  for (int j = 0; j < n; j++) {
    maxrow = std::max(maxrow, trp[j + 1]);
    trp[j + 1] += trp[j];
  }
  if (maxrow > TR_CAP) {
    hipFree(d_cnt);
    return build_transpose_host(A, out, d_perm_out);
  }
  fh_mat_t At = mat_new(c);
  At->m = n;
  At->n = m;
  At->nnz = nnz;
  At->max_row = maxrow;
  At->built_on = 1;
  At->h_rowptr = trp;
  int* d_perm = nullptr;
  FH_CHECK_HIP(hipMalloc(&At->d_rowptr, ((size_t)n + 1) * sizeof(int)));
  FH_CHECK_HIP(hipMalloc(&At->d_col, ((size_t)nnz + 2) * sizeof(int)));
  FH_CHECK_HIP(hipMalloc(&At->d_val, ((size_t)nnz + 2) * sizeof(double)));
  FH_CHECK_HIP(hipMalloc(&d_perm, (size_t)nnz * sizeof(int)));
  FH_CHECK_HIP(hipMemsetAsync(At->d_col + nnz, 0, 2 * sizeof(int), c->stream));
  FH_CHECK_HIP(hipMemsetAsync(At->d_val, 0, ((size_t)nnz + 2) * sizeof(double), c->stream));
  FH_CHECK_HIP(hipMemcpyAsync(At->d_rowptr, trp.data(), ((size_t)n + 1) * sizeof(int), hipMemcpyHostToDevice, c->stream));
  FH_CHECK_HIP(hipMemcpyAsync(d_cnt, trp.data(), (size_t)n * sizeof(int), hipMemcpyHostToDevice, c->stream));          // cursors
  hipLaunchKernelGGL(k_tr_fill, dim3(fh_div_up(m, 4)), dim3(256), 0, c->stream, m, A->d_rowptr, A->d_col, d_cnt, At->d_col, d_perm);
  hipLaunchKernelGGL(k_tr_sort, dim3(fh_div_up(n, 4)), dim3(256), 0, c->stream, n, At->d_rowptr, At->d_col, d_perm);
  FH_CHECK_HIP(hipGetLastError());
  FH_CHECK_HIP(hipStreamSynchronize(c->stream));
  hipFree(d_cnt);
  FH_TRY(fh_spmv_build_rowblocks(At));
  *out = At;
  *d_perm_out = d_perm;
  FH_TRACE("build_transpose (device): %d x %d, %d non-zeros", m, n, nnz);
  return 0;
}

static int gather_transpose_values(fh_mat_t A, fh_mat_t At, const int* d_perm) {
  if (A->nnz == 0) return 0;
  int nb = std::min(fh_div_up(A->nnz, 256), A->ctx->num_cu * 8);
  hipLaunchKernelGGL(k_gather_perm, dim3(nb), dim3(256), 0, A->ctx->stream, At->d_val, A->d_val, d_perm, A->nnz);
  FH_CHECK_HIP(hipGetLastError());
  return 0;
}

extern "C" int fh_mat_transpose(fh_mat_t A, fh_mat_t* out) {
  int* d_perm = nullptr;
  FH_TRY(build_transpose(A, out, &d_perm));
  FH_TRY(gather_transpose_values(A, *out, d_perm));
  FH_CHECK_HIP(hipStreamSynchronize(A->ctx->stream));
  hipFree(d_perm);
  return 0;
}

int fh_mat_refresh_transpose(fh_mat_t A) {
  if (!A->At) FH_TRY(build_transpose(A, &A->At, &A->d_tperm));
  if (!A->at_valid) {
    FH_TRY(gather_transpose_values(A, A->At, A->d_tperm));
    A->at_valid = true;
  }
  return 0;
}

// ------------------------------------------------------------------------------------------------
// Block matrices of m stacked variables of one family (unknown (k, i) = k rows + i), made by kernels from the resident CSR arrays; the row table alone is
// scanned on the host, from the host copy every matrix keeps.  Columns ascend in every row.
//   block_system(S, m)   = kron(ones(m, m), S), values zero: row (k, i) starts at k m nnz + m rowptr[i], block l of it at l len(i) further
//   block_diagonal(P, m) = kron(I_m, P) with P's values: row (k, i) is P's row i, its columns shifted by k cols
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_block_system_cols(int rows, int m, int ncols, long long nnz, const int* __restrict__ rowptr, const int* __restrict__ col,
                                                           int* __restrict__ out) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;      // (k, i, l)
  if (idx >= (long long)rows * m * m) return;
  const int l = (int)(idx % m), i = (int)((idx / m) % rows), k = (int)(idx / ((long long)m * rows));
  const int rs = rowptr[i], n = rowptr[i + 1] - rs;
  int* o = out + (long long)k * m * nnz + (long long)m * rs + (long long)l * n;
  for (int t = 0; t < n; t++) o[t] = l * ncols + col[rs + t];
}

__global__ __launch_bounds__(256) void k_block_diagonal_fill(int m, int ncols, long long nnz, const int* __restrict__ col, const double* __restrict__ val,
                                                             int* __restrict__ ocol, double* __restrict__ oval) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;      // (k, entry)
  if (idx >= nnz * m) return;
  const int k = (int)(idx / nnz);
  const long long e = idx - (long long)k * nnz;
  ocol[idx] = k * ncols + col[e];
  oval[idx] = val[e];
}

static int block_matrix(const char* who, fh_mat_t A, int m, bool diagonal, fh_mat_t* out) {
  FH_GUARD_BEGIN
  FH_REQUIRE(A && out, "%s: null argument", who);
  FH_REQUIRE(m >= 1 && m <= 4, "%s: %d variables, 1 .. 4 are served", who, m);
  FH_REQUIRE((int)A->h_rowptr.size() == A->m + 1, "%s: the matrix has no host row table", who);
  const int rows = A->m, f = diagonal ? 1 : m;
  const long long nnz = A->nnz, total = nnz * m * f;
  FH_REQUIRE(total < 2147483647ll && (long long)rows * m < 2147483647ll && (long long)A->n * m < 2147483647ll, "%s: the block matrix overflows int32", who);
  *out = nullptr;
  std::vector<int> rp((size_t)rows * m + 1);
  for (int k = 0; k < m; k++)
    for (int i = 0; i < rows; i++) rp[(size_t)k * rows + i] = (int)(k * f * nnz + (long long)f * A->h_rowptr[i]);
  rp[(size_t)rows * m] = (int)total;
  fh_ctx_t c = A->ctx;
  fh_mat_t B = nullptr;
  if (fh_mat_alloc_device_pattern(c, rows * m, A->n * m, std::move(rp), &B)) {
    fh_mat_destroy(B);
    return 2;
  }
  if (diagonal) {
    if (total) hipLaunchKernelGGL(k_block_diagonal_fill, dim3(fh_div_up(total, 256)), dim3(256), 0, c->stream, m, A->n, nnz, A->d_col, A->d_val, B->d_col, B->d_val);
  } else {
    if (rows) hipLaunchKernelGGL(k_block_system_cols, dim3(fh_div_up((long long)rows * m * m, 256)), dim3(256), 0, c->stream, rows, m, A->n, nnz, A->d_rowptr, A->d_col, B->d_col);
  }
  if (hipGetLastError() != hipSuccess || hipStreamSynchronize(c->stream) != hipSuccess || fh_spmv_build_rowblocks(B)) {
    fh_mat_destroy(B);
    fh_set_error("%s: the fill kernel failed", who);
    return 1;
  }
  *out = B;
  return 0;
  FH_GUARD_END(who)
}

extern "C" int fh_mat_block_system(fh_mat_t S, int m, fh_mat_t* out) { return block_matrix("fh_mat_block_system", S, m, false, out); }
extern "C" int fh_mat_block_diagonal(fh_mat_t P, int m, fh_mat_t* out) { return block_matrix("fh_mat_block_diagonal", P, m, true, out); }

// ------------------------------------------------------------------------------------------------
// Block matrices of m stacked variables of different sizes n_0 .. n_{m-1} (unknown (k, i) = off_k + i, off_k = n_0 + .. + n_{k-1}):
//   block_system_families(S, n) : block (k, l) is S[:n_k, :n_l], values zero.  The columns of a row of S ascend, so the columns < n_l of row i are its first
//                                 cnt_l(i) entries: row (k, i) holds cnt_0(i) + .. + cnt_{m-1}(i) entries, block l after the blocks before it
//   block_diagonal_of(P_0 ..)   : blkdiag of rectangular matrices with their values
// The counts are taken by a kernel (a binary search per row and size); they come to the host, where the row table is scanned, and go back as the row table.
// ------------------------------------------------------------------------------------------------
struct BlockSizes {
  int m, n[4], off[5];
};

__device__ __forceinline__ int prefix_count(const int* __restrict__ c, int len, int bound) {   // columns < bound among the ascending c[0 .. len)
  int lo = 0, hi = len;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (c[mid] < bound) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

__global__ __launch_bounds__(256) void k_prefix_counts(int rows, BlockSizes bs, const int* __restrict__ rowptr, const int* __restrict__ col, int* __restrict__ out) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;      // (l, i)
  if (idx >= (long long)rows * bs.m) return;
  const int l = (int)(idx / rows), i = (int)(idx - (long long)l * rows);
  const int rs = rowptr[i];
  out[idx] = prefix_count(col + rs, rowptr[i + 1] - rs, bs.n[l]);
}

__global__ __launch_bounds__(256) void k_block_families_cols(int nrows, BlockSizes bs, const int* __restrict__ rowptr, const int* __restrict__ col,
                                                             const int* __restrict__ orp, int* __restrict__ out) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;      // (system row, l)
  if (idx >= (long long)nrows * bs.m) return;
  const int R = (int)(idx / bs.m), l = (int)(idx - (long long)R * bs.m);
  int k = 0;
  while (k + 1 < bs.m && R >= bs.off[k + 1]) k++;
  const int i = R - bs.off[k];
  const int rs = rowptr[i], len = rowptr[i + 1] - rs;
  int at = orp[R], cnt = 0, nl = 0, ol = 0;
#pragma unroll
  for (int q = 0; q < 4; q++)                                            // the blocks before l, then l's own count
    if (q <= l) {
      at += cnt;
      nl = bs.n[q], ol = bs.off[q];
      cnt = prefix_count(col + rs, len, nl);
    }
  const int room = orp[R + 1] - at;                                      // the row table was scanned from the same counts: never less than cnt
  for (int t = 0; t < cnt && t < room; t++) out[at + t] = ol + col[rs + t];
}

__global__ __launch_bounds__(256) void k_block_diagonal_of_fill(long long nnz, int coloff, const int* __restrict__ col, const double* __restrict__ val,
                                                                int* __restrict__ ocol, double* __restrict__ oval) {
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= nnz) return;
  ocol[e] = coloff + col[e];
  oval[e] = val[e];
}

int fh_mat_prefix_counts(const char* who, fh_mat_t S, int cnt, const int* n, std::vector<int>& out) {
  BlockSizes bs{};
  bs.m = cnt;
  for (int l = 0; l < cnt; l++) bs.n[l] = n[l];
  const size_t total = (size_t)S->m * cnt;
  out.assign(total, 0);
  if (!total) return 0;
  int* d = nullptr;
  FH_REQUIRE(hipMalloc(&d, total * sizeof(int)) == hipSuccess, "%s: out of device memory", who);
  hipStream_t st = S->ctx->stream;
  hipLaunchKernelGGL(k_prefix_counts, dim3(fh_div_up((long long)total, 256)), dim3(256), 0, st, S->m, bs, S->d_rowptr, S->d_col, d);
  const bool ok = hipGetLastError() == hipSuccess && hipMemcpyAsync(out.data(), d, total * sizeof(int), hipMemcpyDeviceToHost, st) == hipSuccess &&
                  hipStreamSynchronize(st) == hipSuccess;
  hipFree(d);
  FH_REQUIRE(ok, "%s: the counting kernel failed", who);
  return 0;
}

extern "C" int fh_mat_block_system_families(fh_mat_t S, int m, const int* n, fh_mat_t* out) {
  FH_GUARD_BEGIN
  const char* who = "fh_mat_block_system_families";
  FH_REQUIRE(S && out && n, "%s: null argument", who);
  FH_REQUIRE(m >= 1 && m <= 4, "%s: %d variables, 1 .. 4 are served", who, m);
  FH_REQUIRE((int)S->h_rowptr.size() == S->m + 1, "%s: the matrix has no host row table", who);
  BlockSizes bs{};
  bs.m = m;
  for (int k = 0; k < m; k++) {
    FH_REQUIRE(n[k] >= 1 && n[k] <= S->m, "%s: variable %d has %d unknowns, 1 .. %d are served by this matrix", who, k, n[k], S->m);
    bs.n[k] = n[k];
    bs.off[k + 1] = bs.off[k] + n[k];
  }
  *out = nullptr;
  const int rows = S->m, N = bs.off[m];
  std::vector<int> cnt;
  FH_TRY(fh_mat_prefix_counts(who, S, m, n, cnt));
  std::vector<int> rp((size_t)N + 1);
  long long total = 0;
  for (int k = 0; k < m; k++)
    for (int i = 0; i < n[k]; i++) {
      rp[(size_t)bs.off[k] + i] = (int)total;
      for (int l = 0; l < m; l++) total += cnt[(size_t)l * rows + i];
      FH_REQUIRE(total < 2147483647ll, "%s: the block matrix overflows int32", who);
    }
  rp[N] = (int)total;
  fh_ctx_t c = S->ctx;
  fh_mat_t B = nullptr;
  if (fh_mat_alloc_device_pattern(c, N, N, std::move(rp), &B)) {
    fh_mat_destroy(B);
    return 2;
  }
  hipLaunchKernelGGL(k_block_families_cols, dim3(fh_div_up((long long)N * m, 256)), dim3(256), 0, c->stream, N, bs, S->d_rowptr, S->d_col, B->d_rowptr, B->d_col);
  if (hipGetLastError() != hipSuccess || hipStreamSynchronize(c->stream) != hipSuccess || fh_spmv_build_rowblocks(B)) {
    fh_mat_destroy(B);
    fh_set_error("%s: the fill kernel failed", who);
    return 1;
  }
  *out = B;
  return 0;
  FH_GUARD_END("fh_mat_block_system_families")
}

extern "C" int fh_mat_block_diagonal_of(int m, const fh_mat_t* P, fh_mat_t* out) {
  FH_GUARD_BEGIN
  const char* who = "fh_mat_block_diagonal_of";
  FH_REQUIRE(P && out, "%s: null argument", who);
  FH_REQUIRE(m >= 1 && m <= 4, "%s: %d variables, 1 .. 4 are served", who, m);
  long long rows = 0, cols = 0, total = 0;
  for (int k = 0; k < m; k++) {
    FH_REQUIRE(P[k], "%s: matrix %d is null", who, k);
    FH_REQUIRE(P[k]->ctx == P[0]->ctx, "%s: matrix %d lives on another context", who, k);
    FH_REQUIRE((int)P[k]->h_rowptr.size() == P[k]->m + 1, "%s: matrix %d has no host row table", who, k);
    rows += P[k]->m, cols += P[k]->n, total += P[k]->nnz;
  }
  FH_REQUIRE(total < 2147483647ll && rows < 2147483647ll && cols < 2147483647ll, "%s: the block matrix overflows int32", who);
  *out = nullptr;
  std::vector<int> rp((size_t)rows + 1);
  {
    size_t r = 0;
    long long base = 0;
    for (int k = 0; k < m; k++) {
      for (int i = 0; i < P[k]->m; i++) rp[r++] = (int)(base + P[k]->h_rowptr[i]);
      base += P[k]->nnz;
    }
    rp[r] = (int)base;
  }
  fh_ctx_t c = P[0]->ctx;
  fh_mat_t B = nullptr;
  if (fh_mat_alloc_device_pattern(c, (int)rows, (int)cols, std::move(rp), &B)) {
    fh_mat_destroy(B);
    return 2;
  }
  long long base = 0;
  int coloff = 0;
  for (int k = 0; k < m; k++) {
    const long long nnz = P[k]->nnz;
    if (nnz)
      hipLaunchKernelGGL(k_block_diagonal_of_fill, dim3(fh_div_up(nnz, 256)), dim3(256), 0, c->stream, nnz, coloff, P[k]->d_col, P[k]->d_val, B->d_col + base,
                         B->d_val + base);
    base += nnz, coloff += P[k]->n;
  }
  if (hipGetLastError() != hipSuccess || hipStreamSynchronize(c->stream) != hipSuccess || fh_spmv_build_rowblocks(B)) {
    fh_mat_destroy(B);
    fh_set_error("%s: the fill kernel failed", who);
    return 1;
  }
  *out = B;
  return 0;
  FH_GUARD_END("fh_mat_block_diagonal_of")
}

// ------------------------------------------------------------------------------------------------
// norms (l1 = max column sum, linfty = max row sum) -- setup/diagnostic only: via the host
// ------------------------------------------------------------------------------------------------
extern "C" int fh_mat_norm(fh_mat_t A, int kind, double* out) {
  std::vector<double> v(A->nnz);
  if (A->nnz) FH_TRY(fh_mat_get_values_csr(A, v.data()));
  double best = 0.0;
  if (kind == 0) {
    for (int i = 0; i < A->m; i++) {
      double s = 0.0;
      for (int k = A->h_rowptr[i]; k < A->h_rowptr[i + 1]; k++) s += fabs(v[k]);
      best = std::max(best, s);
    }
  } else if (kind == 1) {
    std::vector<double> cs(A->n, 0.0);
    for (int k = 0; k < A->nnz; k++) cs[fh_hcol(A)[k]] += fabs(v[k]);
    for (double s : cs) best = std::max(best, s);
  } else {
    fh_set_error("fh_mat_norm: unknown kind %d", kind);
    return 2;
  }
  *out = best;
  return 0;
}
