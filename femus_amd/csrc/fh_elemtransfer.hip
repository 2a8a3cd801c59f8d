// The transfers and the boundary lists of a device-resident ELEMENT mesh (fh_elemmesh.hip), built where the mesh lives: what
// femus_amd/app_poisson.py: _prolongator_from_children and the face loop of run_elements do on the host, integer for integer and bit for bit
// (tests/test_gpu_element_transfer.py).
//
// fh_elem_mesh_prolongator -- PP of a level from the element prolongators (ElemType.cpp:439-532).  For every shape s, child j, fine local node n < nc(s, fe),
// coarse local function k < nc(s, fe) with EP_s[j][n][k] != 0 and coarse element e of shape s, the value EP_s[j][n][k] is INSERTED at row ed_f[nch e + j][n],
// column ed_c[e][k]; insertions are ordered by (shape, j, n, k, e) and the last one of an entry stays.  Shapes go in the order of their NAMES sorted as strings,
// the order in which run_elements passes its groups: hex < quad < tet < tri < wedge, that is the shape codes 0, 1, 4, 3, 5.
//   1. fine dof -> the entries (fine element, local node) that hold it: the counting pass of fh_mat_create_from_elements (fh_dof_lists_build).  The order
//      inside a list depends on the race; nothing below does.
//   2. one wave per fine row, twice (lengths, then columns and values; the host scans the lengths in between as for every device-built pattern).  An entry
//      (f, n) of the row gives the candidates k = 0 .. nc - 1 with a non-zero weight: column ed_c[e][k] and the 64-bit ORDER KEY
//      (rank of the shape, j, n, k, e), which no two candidates share; e = father[f], j = child[f], after a uniform refinement f / nch and f % nch.  The wave packs the candidates into LDS, sorts them by
//      (column, key) -- a bitonic network, columns alone in the first pass -- and the last candidate of every run of equal columns is the entry: the
//      insertion that came last.  Its value is read off its key (the weight EP_s[j][n][k]); no value is ever added, compared or touched by an atomic.
//   3. a row whose entries hold more than `elem_transfer_lds_rows` candidate slots (27 per entry; 1024 at most) does not fit the wave's LDS: the host, which
//      has the list lengths anyway, gives each such row a piece of global scratch, and one workgroup per row writes the candidates there, marks the one with
//      the largest key of its column by comparing all pairs, and places it at the number of marked candidates with a smaller column.  Same rule, same bits.
// A FLAGGED fine level (fh_elem_mesh_refine_flagged) is read through its links: fine element f is child j = child[f] of e = father[f], or its unchanged copy
// (j = -1).  An entry (f, n) of a copy gives the single candidate k = n with the value 1.0 exactly, column ed_c[e][n] (LinearImplicitSystem.cpp:761-811); the
// copies' insertions come after those of every child of every shape, ordered (shape, n, e), so a node a copy shares with a refined neighbour keeps the 1.0
// (app_poisson.py: _prolongator_from_links).  The high word of the order key, from the top: copy (1 bit), rank of the shape (3), j (4), n (5), k (5).
// The weights of the shapes present (family fe, |.| < 1e-14 already zero: fhfe::elem_prolongator) go up once per call.
//
// fh_elem_mesh_boundary_dofs -- one thread per (element, face, face node) marks the dof when the face's flag is one of the caller's; an exclusive scan of the
// marks and a compaction give the ascending list.
#include "fh_elemmesh.h"
#include "fh_fe.h"
#include "fh_spmv.h"

namespace {
constexpr int ET_CAP = 1024;                    // candidates one wave sorts in LDS
constexpr int ET_NOCOL = 0x7fffffff;            // sorts behind every column
constexpr int ET_FN = 9;                        // nodes of the widest face
typedef unsigned long long et_key;

struct EtTab {
  int nc[EM_G], ep[EM_G];         // dofs per element of the family, first double of the shape's [nch][nc][nc] weights
  int rank[EM_G], shape[EM_G];    // shape code -> place of its name among the sorted names, and back
};
struct EtArgs {
  EtTab T;
  const double* EP;
  const int *aptr, *adj;          // fine dof -> entries f * 27 + n
  const int *geom_f, *ed_c, *father, *child;    // of the fine elements
  int m, ncols;
  int* err;
};
struct EtFaces {
  signed char n[EM_G][EM_F];      // face nodes of the family (0: no such face)
  signed char node[EM_G][EM_F][ET_FN];
};

// candidate k of entry `entry` (= f * 27 + n): false when the weight is zero or the shape has no such function
__device__ __forceinline__ bool et_candidate(const EtArgs& A, int entry, int k, int& col, et_key& key) {
  const int f = entry / EM_W, n = entry % EM_W;
  const int g = A.geom_f[f], nc = A.T.nc[g];
  if (k >= nc || n >= nc) return false;
  const int e = A.father[f], j = A.child[f];
  if (j < 0 ? k != n : A.EP[A.T.ep[g] + (j * nc + n) * nc + k] == 0.0) return false;
  col = A.ed_c[(size_t)e * EM_W + k];
  if (col < 0 || col >= A.ncols) {              // not a mesh whose families own the leading ids: refused after the pass
    atomicExch(A.err, 1);
    return false;
  }
  key = ((et_key)(((((j < 0 ? 8 : 0) + A.T.rank[g]) * 16 + (j < 0 ? 0 : j)) * 32 + n) * 32 + k) << 32) | (unsigned)e;
  return true;
}
__device__ __forceinline__ double et_value(const EtArgs& A, et_key key) {
  const int c = (int)(key >> 32), k = c & 31, n = (c >> 5) & 31, j = (c >> 10) & 15, g = A.T.shape[(c >> 14) & 7];
  if (c >> 17) return 1.0;        // a copy
  return A.EP[A.T.ep[g] + (j * A.T.nc[g] + n) * A.T.nc[g] + k];
}

__device__ __forceinline__ void et_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// one wave per fine row; FILL = false: the row's length, true: its columns and values
template <bool FILL>
__global__ __launch_bounds__(256) void k_et_rows(EtArgs A, int cap, const int* __restrict__ rowptr, int* __restrict__ rowlen, int* __restrict__ col,
                                                 double* __restrict__ val) {
  __shared__ int s_col[4][ET_CAP];
  __shared__ et_key s_key[FILL ? 4 : 1][FILL ? ET_CAP : 1];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int r = blockIdx.x * 4 + wave;
  if (r >= A.m) return;
  const int a0 = A.aptr[r], npad = (A.aptr[r + 1] - a0) * EM_W;
  if (npad > cap) return;                       // the workgroup path's (cap <= ET_CAP)
  int* cc = s_col[wave];
  et_key* kk = s_key[FILL ? wave : 0];
  int n = 0;
  for (int t0 = 0; t0 < npad; t0 += 64) {       // packed: most weights are zero
    const int t = t0 + lane;
    int c = 0;
    et_key key = 0;
    const bool ok = t < npad && et_candidate(A, A.adj[a0 + t / EM_W], t % EM_W, c, key);
    const unsigned long long mask = __ballot(ok);
    if (ok) {
      const int p = n + __popcll(mask & ((1ull << lane) - 1ull));
      cc[p] = c;
      if (FILL) kk[p] = key;
    }
    n += __popcll(mask);
  }
  int np = 64;
  while (np < n) np <<= 1;
  for (int k = n + lane; k < np; k += 64) {
    cc[k] = ET_NOCOL;
    if (FILL) kk[k] = 0;
  }
  et_wave_sync();
  for (int size = 2; size <= np; size <<= 1)
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      for (int t = lane; t < (np >> 1); t += 64) {
        const int lo = ((t / stride) * (stride << 1)) + (t % stride), hi = lo + stride;
        const bool up = ((lo & size) == 0);
        const int a = cc[lo], c = cc[hi];
        if (FILL) {
          const et_key ka = kk[lo], kc = kk[hi];
          if ((a > c || (a == c && ka > kc)) == up) {
            cc[lo] = c; cc[hi] = a;
            kk[lo] = kc; kk[hi] = ka;
          }
        } else if ((a > c) == up) {
          cc[lo] = c; cc[hi] = a;
        }
      }
      et_wave_sync();
    }
  // the last candidate of a run of equal columns carries the run's largest key
  const int per = np >> 6, k0 = lane * per;
  int mine = 0;
  for (int k = k0; k < k0 + per && k < n; k++) mine += (k == n - 1 || cc[k + 1] != cc[k]) ? 1 : 0;
  int incl = mine;
  for (int d = 1; d < 64; d <<= 1) {
    const int v = __shfl_up(incl, d, 64);
    if (lane >= d) incl += v;
  }
  if (!FILL) {
    if (lane == 63) rowlen[r] = incl;
    return;
  }
  int o = rowptr[r] + incl - mine;
  for (int k = k0; k < k0 + per && k < n; k++)
    if (k == n - 1 || cc[k + 1] != cc[k]) {
      col[o] = cc[k];
      val[o++] = et_value(A, kk[k]);
    }
}

// one workgroup per row that does not fit the wave's LDS; piece [off[b], off[b + 1]) of the scratch holds its 27 slots per entry
__global__ __launch_bounds__(256) void k_et_slow_count(EtArgs A, const int* __restrict__ rows, const int* __restrict__ off, int* __restrict__ gcol,
                                                       et_key* __restrict__ gkey, int* __restrict__ gwin, int* __restrict__ rowlen) {
  __shared__ int part[256];
  const int r = rows[blockIdx.x], o = off[blockIdx.x], npad = off[blockIdx.x + 1] - o, a0 = A.aptr[r];
  for (int t = threadIdx.x; t < npad; t += 256) {
    int c = 0;
    et_key key = 0;
    const bool ok = et_candidate(A, A.adj[a0 + t / EM_W], t % EM_W, c, key);
    gcol[o + t] = ok ? c : ET_NOCOL;
    gkey[o + t] = ok ? key : 0;
  }
  __syncthreads();
  int mine = 0;
  for (int t = threadIdx.x; t < npad; t += 256) {
    const int c = gcol[o + t];
    int win = c != ET_NOCOL;
    if (win) {
      const et_key key = gkey[o + t];
      for (int u = 0; u < npad; u++)
        if (gcol[o + u] == c && gkey[o + u] > key) {
          win = 0;
          break;
        }
    }
    gwin[o + t] = win;
    mine += win;
  }
  part[threadIdx.x] = mine;
  __syncthreads();
  if (threadIdx.x == 0) {
    int s = 0;
    for (int k = 0; k < 256; k++) s += part[k];
    rowlen[r] = s;
  }
}
__global__ __launch_bounds__(256) void k_et_slow_fill(EtArgs A, const int* __restrict__ rows, const int* __restrict__ off, const int* __restrict__ gcol,
                                                      const et_key* __restrict__ gkey, const int* __restrict__ gwin, const int* __restrict__ rowptr,
                                                      int* __restrict__ col, double* __restrict__ val) {
  const int r = rows[blockIdx.x], o = off[blockIdx.x], npad = off[blockIdx.x + 1] - o;
  for (int t = threadIdx.x; t < npad; t += 256) {
    if (!gwin[o + t]) continue;
    const int c = gcol[o + t];
    int pos = 0;
    for (int u = 0; u < npad; u++) pos += (gwin[o + u] && gcol[o + u] < c) ? 1 : 0;
    col[rowptr[r] + pos] = c;
    val[rowptr[r] + pos] = et_value(A, gkey[o + t]);
  }
}

__global__ __launch_bounds__(256) void k_et_mark(EtFaces F, int nel, const int* __restrict__ geom, const int* __restrict__ ed, const int* __restrict__ ff, int nflags,
                                                 const int* __restrict__ flags, int own, int* __restrict__ mark) {
  const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= (size_t)nel * EM_F * ET_FN) return;
  const int e = (int)(t / (EM_F * ET_FN)), f = (int)(t / ET_FN) % EM_F, i = (int)(t % ET_FN);
  const int g = geom[e];
  if (i >= F.n[g][f]) return;
  const int flag = ff[(size_t)e * EM_F + f];
  bool hit = false;
  for (int q = 0; q < nflags; q++) hit = hit || flags[q] == flag;
  if (!hit) return;
  const int d = ed[(size_t)e * EM_W + F.node[g][f][i]];
  if (d >= 0 && d < own) mark[d] = 1;           // every writer writes the same word
}
__global__ __launch_bounds__(256) void k_et_compact(int n, const int* __restrict__ pos, int* __restrict__ out) {
  const int d = blockIdx.x * 256 + threadIdx.x;
  if (d < n && pos[d + 1] != pos[d]) out[pos[d]] = d;
}

// work buffers: freed with the object, after the stream has been synchronised; 0xFF bytes under debug_poison (every entry is written before it is read)
struct EtScratch {
  fh_ctx_t ctx;
  const char* who;
  std::vector<void*> p;
  EtScratch(fh_ctx_t c, const char* w) : ctx(c), who(w) {}
  ~EtScratch() {
    for (void* q : p)
      if (q) hipFree(q);
  }
  template <class T>
  int get(T** out, size_t n) {
    void* q = nullptr;
    const size_t bytes = std::max<size_t>(n, 2) * sizeof(T);
    if (hipMalloc(&q, bytes) != hipSuccess) {
      fh_set_error("%s: out of device memory", who);
      return 2;
    }
    p.push_back(q);
    *out = (T*)q;
    if (ctx->debug_poison) FH_CHECK_HIP(hipMemsetAsync(q, 0xFF, bytes, ctx->stream));
    return 0;
  }
};

constexpr int ET_RANK[EM_G] = {0, 1, -1, 3, 2, 4};    // hex, quad, (line), tri, tet, wedge among "hex" < "quad" < "tet" < "tri" < "wedge"
bool et_shape(int g) { return g >= 0 && g < EM_G && ET_RANK[g] >= 0; }
}   // namespace

extern "C" int fh_elem_mesh_prolongator(fh_elem_mesh_t C, fh_elem_mesh_t F, int fe, fh_mat_t* out) {
  FH_GUARD_BEGIN
  const char* who = "fh_elem_mesh_prolongator";
  FH_REQUIRE(C && F && out, "%s: null argument", who);
  FH_REQUIRE(fe >= 0 && fe <= 2, "%s: fe must be 0 (linear), 1 (serendipity) or 2 (biquadratic), not %d", who, fe);
  FH_REQUIRE(C->ctx == F->ctx, "%s: the two meshes live on different contexts", who);
  FH_REQUIRE(C->dim == F->dim, "%s: a %d-dimensional coarse and a %d-dimensional fine mesh", who, C->dim, F->dim);
  FH_REQUIRE(F->level == C->level + 1, "%s: the fine mesh is of level %d, the coarse one of level %d: not its refinement", who, F->level, C->level);
  const int nch = C->dim == 3 ? 8 : 4;
  fh_ctx_t ctx = C->ctx;
  hipStream_t st = ctx->stream;
  {   // the links of the fine elements against the coarse mesh: four copies, no launch
    std::vector<int> gc((size_t)C->nel), gf((size_t)F->nel), fa((size_t)F->nel), ch((size_t)F->nel);
    if (C->nel) FH_CHECK_HIP(hipMemcpyAsync(gc.data(), C->d_geom, gc.size() * sizeof(int), hipMemcpyDeviceToHost, st));
    if (F->nel) {
      FH_CHECK_HIP(hipMemcpyAsync(gf.data(), F->d_geom, gf.size() * sizeof(int), hipMemcpyDeviceToHost, st));
      FH_CHECK_HIP(hipMemcpyAsync(fa.data(), F->d_father, fa.size() * sizeof(int), hipMemcpyDeviceToHost, st));
      FH_CHECK_HIP(hipMemcpyAsync(ch.data(), F->d_child, ch.size() * sizeof(int), hipMemcpyDeviceToHost, st));
    }
    FH_CHECK_HIP(hipStreamSynchronize(st));
    for (int e = 0; e < C->nel; e++) FH_REQUIRE(et_shape(gc[e]), "%s: coarse element %d has shape code %d", who, e, gc[e]);
    std::vector<unsigned> seen((size_t)C->nel, 0);           // per coarse element: bit j = child j met, bit nch = its copy met
    for (int f = 0; f < F->nel; f++) {
      FH_REQUIRE(fa[f] >= 0 && fa[f] < C->nel && ch[f] >= -1 && ch[f] < nch,
                 "%s: fine element %d is child %d of element %d, the coarse mesh has %d elements: not its refinement", who, f, ch[f], fa[f], C->nel);
      const unsigned bit = 1u << (ch[f] < 0 ? nch : ch[f]);
      FH_REQUIRE(!(seen[fa[f]] & bit), "%s: coarse element %d has two fine elements that are its child %d: not its refinement", who, fa[f], ch[f]);
      seen[fa[f]] |= bit;
    }
    int64_t nsplit = 0, fine_of[EM_G] = {0, 0, 0, 0, 0, 0};
    for (int e = 0; e < C->nel; e++) {
      const bool split = seen[e] != (1u << nch);
      FH_REQUIRE(seen[e], "%s: coarse element %d has neither children nor a copy among the fine elements: not its refinement", who, e);
      FH_REQUIRE(!split || seen[e] == (1u << nch) - 1u, "%s: coarse element %d has a copy and children, or not all of its %d children: not its refinement", who, e,
                 nch);
      nsplit += split;
      fine_of[gc[e]] += split ? nch : 1;
    }
    FH_REQUIRE((int64_t)F->nel == (int64_t)C->nel + (nch - 1) * nsplit,
               "%s: %d fine elements are not the %d children of each of %lld coarse elements and the copies of the other %lld", who, F->nel, nch, (long long)nsplit,
               (long long)(C->nel - nsplit));
    for (int g = 0; g < EM_G; g++)
      FH_REQUIRE(F->count[g] == fine_of[g], "%s: %lld fine elements of shape code %d are not the children of and copies of %lld coarse ones, which give %lld",
                 who, (long long)F->count[g], g, (long long)C->count[g], (long long)fine_of[g]);
    for (int f = 0; f < F->nel; f++)
      FH_REQUIRE(gf[f] == gc[fa[f]], "%s: fine element %d has shape code %d, its father %d shape code %d: not its refinement", who, f, gf[f], fa[f], gc[fa[f]]);
  }
  const int m = F->own[fe], ncols = C->own[fe];
  FH_REQUIRE(m >= 0 && m <= F->nnode && ncols >= 0 && ncols <= C->nnode, "%s: the family owns %d of %d fine and %d of %d coarse nodes", who, m, F->nnode, ncols,
             C->nnode);
  int cap = std::min(std::max(ctx->elem_transfer_lds_rows, 0), ET_CAP);

  EtArgs A;
  memset(&A, 0, sizeof(A));
  std::vector<double> EP, one;
  for (int g = 0; g < EM_G; g++) {
    A.T.rank[g] = et_shape(g) ? ET_RANK[g] : 0;
    if (et_shape(g)) A.T.shape[ET_RANK[g]] = g;
    if (!et_shape(g) || !C->count[g]) continue;
    A.T.nc[g] = fhfe::ndofs_of(g, fe);
    A.T.ep[g] = (int)EP.size();
    fhfe::elem_prolongator(g, fe, one);
    FH_REQUIRE(one.size() == (size_t)nch * A.T.nc[g] * A.T.nc[g] && A.T.nc[g] <= EM_W, "%s: unexpected sizes of the element prolongator (shape %d)", who, g);
    EP.insert(EP.end(), one.begin(), one.end());
  }

  fh_dof_lists L;                 // freed on return: every path below has synchronised the stream by then
  EtScratch B(ctx, who);
  if (int rc = fh_dof_lists_build(ctx, who, (size_t)F->nel * EM_W, 1, F->d_ed, m, F->nnode, true, &L)) {
    hipStreamSynchronize(st);
    return rc;
  }
  // rows for the workgroup path, each with its piece of the scratch
  std::vector<int> srow, soff(1, 0);
  int64_t stot = 0;
  for (int r = 0; r < m; r++) {
    const int64_t npad = (int64_t)(L.ptr[r + 1] - L.ptr[r]) * EM_W;
    if (npad <= cap) continue;
    stot += npad;
    if (stot >= 2147483647ll) break;
    srow.push_back(r);
    soff.push_back((int)stot);
  }
  const int ns = (int)srow.size();
  double* d_EP;
  int *d_len, *d_srow, *d_soff, *d_gcol, *d_gwin;
  et_key* d_gkey;
  int rc = stot >= 2147483647ll ? 2 : 0;
  if (rc) fh_set_error("%s: the rows beyond the LDS capacity hold more than 2^31 candidate slots", who);
  rc = rc || B.get(&d_EP, EP.size()) || B.get(&d_len, (size_t)m + 1) || B.get(&d_srow, (size_t)ns) || B.get(&d_soff, (size_t)ns + 1) ||
       B.get(&d_gcol, (size_t)stot) || B.get(&d_gwin, (size_t)stot) || B.get(&d_gkey, (size_t)stot);
  if (rc) {
    hipStreamSynchronize(st);
    return 2;
  }
  auto fail = [&](int code) {     // nothing is freed under a running kernel
    hipStreamSynchronize(st);
    return code;
  };
  hipError_t he = hipSuccess;
  if (!EP.empty()) he = hipMemcpyAsync(d_EP, EP.data(), EP.size() * sizeof(double), hipMemcpyHostToDevice, st);
  if (he == hipSuccess && ns) he = hipMemcpyAsync(d_srow, srow.data(), (size_t)ns * sizeof(int), hipMemcpyHostToDevice, st);
  if (he == hipSuccess) he = hipMemcpyAsync(d_soff, soff.data(), ((size_t)ns + 1) * sizeof(int), hipMemcpyHostToDevice, st);
  if (he != hipSuccess) {
    fh_set_error("%s: %s", who, hipGetErrorString(he));
    return fail(1);
  }
  A.EP = d_EP; A.aptr = L.d_ptr; A.adj = L.d_adj; A.geom_f = F->d_geom; A.ed_c = C->d_ed; A.father = F->d_father; A.child = F->d_child; A.m = m; A.ncols = ncols; A.err = L.d_err;
  if (m) hipLaunchKernelGGL(k_et_rows<false>, dim3(fh_div_up(m, 4)), dim3(256), 0, st, A, cap, (const int*)nullptr, d_len, (int*)nullptr, (double*)nullptr);
  if (ns) hipLaunchKernelGGL(k_et_slow_count, dim3(ns), dim3(256), 0, st, A, d_srow, d_soff, d_gcol, d_gkey, d_gwin, d_len);
  std::vector<int> rp((size_t)m + 1, 0);
  int err = 0;
  he = hipGetLastError();
  if (he == hipSuccess && m) he = hipMemcpyAsync(rp.data() + 1, d_len, (size_t)m * sizeof(int), hipMemcpyDeviceToHost, st);
  if (he == hipSuccess) he = hipMemcpyAsync(&err, L.d_err, sizeof(int), hipMemcpyDeviceToHost, st);
  if (he == hipSuccess) he = hipStreamSynchronize(st);
  if (he != hipSuccess) {
    fh_set_error("%s: %s", who, hipGetErrorString(he));
    return fail(1);
  }
  FH_REQUIRE(!err, "%s: a coarse element holds a dof outside the %d the family owns on the coarse mesh", who, ncols);
  int64_t tot = 0;
  for (int r = 0; r < m; r++) {
    tot += rp[r + 1];
    rp[r + 1] = (int)tot;
  }
  FH_REQUIRE(tot < 2147483647ll, "%s: nnz overflows int32", who);
  fh_mat_t P = nullptr;
  if (fh_mat_alloc_device_pattern(ctx, m, ncols, std::move(rp), &P)) {
    hipStreamSynchronize(st);
    if (P) fh_mat_destroy(P);
    return 2;
  }
  if (m) hipLaunchKernelGGL(k_et_rows<true>, dim3(fh_div_up(m, 4)), dim3(256), 0, st, A, cap, P->d_rowptr, (int*)nullptr, P->d_col, P->d_val);
  if (ns) hipLaunchKernelGGL(k_et_slow_fill, dim3(ns), dim3(256), 0, st, A, d_srow, d_soff, d_gcol, d_gkey, d_gwin, P->d_rowptr, P->d_col, P->d_val);
  he = hipGetLastError();
  if (he == hipSuccess) he = hipStreamSynchronize(st);
  if (he == hipSuccess && fh_spmv_build_rowblocks(P)) {
    fh_mat_destroy(P);
    return fail(2);
  }
  if (he != hipSuccess) {
    fh_set_error("%s: %s", who, hipGetErrorString(he));
    fh_mat_destroy(P);
    return fail(1);
  }
  fh_mat_values_written(P);
  *out = P;
  return 0;
  FH_GUARD_END("fh_elem_mesh_prolongator")
}

extern "C" int fh_elem_mesh_boundary_dofs(fh_elem_mesh_t M, int fe, int nflags, const int* flags, int* ndofs, int* dofs) {
  FH_GUARD_BEGIN
  const char* who = "fh_elem_mesh_boundary_dofs";
  FH_REQUIRE(M && ndofs, "%s: null argument", who);
  FH_REQUIRE(fe >= 0 && fe <= 2, "%s: fe must be 0 (linear), 1 (serendipity) or 2 (biquadratic), not %d", who, fe);
  FH_REQUIRE(nflags >= 0 && (flags || nflags == 0), "%s: %d flags and no list of them", who, nflags);
  const int own = M->own[fe];
  FH_REQUIRE(own >= 0 && own <= M->nnode, "%s: the family owns %d of %d nodes", who, own, M->nnode);
  const int given = *ndofs;
  FH_REQUIRE(!dofs || given >= 0, "%s: ndofs is %d (call with dofs = NULL first)", who, given);
  if (!nflags || !M->nel || !own) {
    FH_REQUIRE(!dofs || given == 0, "%s: ndofs is %d, the list has 0 entries (call with dofs = NULL first)", who, given);
    *ndofs = 0;
    return 0;
  }
  EtFaces FT;
  memset(&FT, 0, sizeof(FT));
  for (int g = 0; g < EM_G; g++) {
    if (!et_shape(g)) continue;
    for (int f = 0; f < fhfe::nfaces_of(g); f++) {
      int tmp[ET_FN];
      const int n = fhfe::face_nodes(g, fe, f, tmp);
      FH_REQUIRE(n >= 0 && n <= ET_FN && f < EM_F, "%s: unexpected face tables (shape %d)", who, g);
      FT.n[g][f] = (signed char)n;
      for (int k = 0; k < n; k++) FT.node[g][f][k] = (signed char)tmp[k];
    }
  }
  fh_ctx_t ctx = M->ctx;
  hipStream_t st = ctx->stream;
  EtScratch B(ctx, who);
  int *d_flags, *d_mark, *d_bsum, *d_out;
  if (B.get(&d_flags, (size_t)nflags) || B.get(&d_mark, (size_t)own + 1) || B.get(&d_bsum, (size_t)own / FH_SCAN_BLOCK + 2) ||
      B.get(&d_out, (size_t)(dofs ? given : 0))) {
    hipStreamSynchronize(st);
    return 2;
  }
  int total = 0, rc = 0;
  hipError_t he = hipMemcpyAsync(d_flags, flags, (size_t)nflags * sizeof(int), hipMemcpyHostToDevice, st);
  if (he == hipSuccess) he = hipMemsetAsync(d_mark, 0, ((size_t)own + 1) * sizeof(int), st);
  if (he == hipSuccess) {
    const size_t nthr = (size_t)M->nel * EM_F * ET_FN;
    hipLaunchKernelGGL(k_et_mark, dim3((unsigned)((nthr + 255) / 256)), dim3(256), 0, st, FT, M->nel, M->d_geom, M->d_ed, M->d_ff, nflags, d_flags, own, d_mark);
    he = hipGetLastError();
  }
  if (he == hipSuccess) rc = fh_device_exclusive_scan(st, d_mark, d_mark, own, d_bsum);
  if (he == hipSuccess && !rc) he = hipMemcpyAsync(&total, d_mark + own, sizeof(int), hipMemcpyDeviceToHost, st);
  if (he == hipSuccess && !rc) he = hipStreamSynchronize(st);
  if (he == hipSuccess && !rc && dofs && total == given && total) {
    hipLaunchKernelGGL(k_et_compact, dim3(fh_div_up(own, 256)), dim3(256), 0, st, own, d_mark, d_out);
    he = hipGetLastError();
    if (he == hipSuccess) he = hipMemcpyAsync(dofs, d_out, (size_t)total * sizeof(int), hipMemcpyDeviceToHost, st);
  }
  const hipError_t hs = hipStreamSynchronize(st);       // the scratch is freed on return
  if (he == hipSuccess) he = hs;
  if (he != hipSuccess) {
    fh_set_error("%s: %s", who, hipGetErrorString(he));
    return 1;
  }
  if (rc) return rc;
  FH_REQUIRE(!dofs || total == given, "%s: ndofs is %d, the list has %d entries (call with dofs = NULL first)", who, given, total);
  *ndofs = total;
  return 0;
  FH_GUARD_END("fh_elem_mesh_boundary_dofs")
}
