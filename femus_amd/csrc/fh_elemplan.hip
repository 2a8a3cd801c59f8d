// What stands between "the level is resident" and "the first assembly", built where the element mesh lives (fh_elemmesh.hip): the pattern of a family, the plan
// of the generic assembler and the boundary lists -- what app_poisson.py: _pattern_from_elements, fh_generic_assembler_create and the face loop of run_elements
// make from the downloaded arrays, integer for integer (tests/test_gpu_element_plan.py).  No kernel here lets a value or a position depend on which thread
// came first: atomics only take a minimum or a maximum, lists are ordered by rank counting, compactions go count / scan / write.
//
// fh_elem_mesh_matrix -- one thread per (element, column) writes the compact table [nel][width]: the element's first nc(shape, fe) dofs, then its first dof again
// up to the widest shape of the mesh (a repeated dof adds no entry).  The builder of fh_mat_create_from_elements takes the table where it is.
//
// fh_generic_assembler_create_from_mesh -- the object of fh_generic_assembler_create (fh_generic.h):
//   1. the first element of every shape (atomicMin) orders the shapes; six integers come back
//   2. per shape a flag per element, an exclusive scan: the element's slot = its rank among the elements of its shape
//   3. one thread per (element, local node) writes the ONE compact table T of all shapes, shape after shape: T[row_base[k] + slot nc_k + n], so that an index into
//      T is the id of an element row and d_ed[k] = T + row_base[k]; and slot -> element
//   4. dof -> the indices of T that hold it (fh_dof_lists_build; the order inside a list depends on the race), then one thread per list entry counts the entries
//      of its list with a smaller (element, row id) and writes itself at that rank: ascending ELEMENT order, the order of the host's fill -- not ascending id
//      order where shapes interleave
//   5. coordinates: a copy of d_x (the assembler outlives the mesh); tables, work buffers and positions as on the host path (gp_plan_work)
//
// fh_elem_mesh_boundary_faces -- a mark per (element, face), an exclusive scan, one thread per marked face writes its row: ascending (element, face).
// fh_elem_mesh_boundary_owners -- one thread per (element, face, face node) of a listed face takes atomicMax(6 element + face) on the node's dof: the LAST listed
// face that holds it, as the dictionary of run_elements' loop keeps it; scan and compaction of the dofs that got one, with the winner's flag and the coordinates.
#include "fh_elemmesh.h"
#include "fh_generic.h"
#include "fh_fe.h"
#include <climits>

namespace {
constexpr int EP_FN = 9;                        // nodes of the widest face

struct EpShapes {
  int nc[EM_G];                   // dofs per element of the family by shape code (0: no such shape in the mesh)
  int idx[EM_G];                  // shape code -> index of the shape in the plan (-1: none)
  int row_base[3], ncs[3], nslot[3], elem_base[3];         // by shape index; row_base INT_MAX where there is no such shape
};
struct EpFaces {
  signed char nf[EM_G];           // faces of the shape
  signed char n[EM_G][EM_F];      // face nodes of the family
  signed char node[EM_G][EM_F][EP_FN];
};

bool ep_shape(int g) { return g >= 0 && g < EM_G && g != 2; }

// work buffers of one entry point, freed on return; 0xFF bytes under debug_poison (every entry is written before it is read)
struct EpScratch : EmScratch {
  fh_ctx_t ctx;
  EpScratch(fh_ctx_t c, const char* w) : EmScratch(w), ctx(c) {}
  template <class T>
  int get(T** out, size_t n) {
    if (int rc = EmScratch::get(out, n)) return rc;
    if (ctx->debug_poison) FH_CHECK_HIP(hipMemsetAsync(*out, 0xFF, std::max<size_t>(n, 2) * sizeof(T), ctx->stream));
    return 0;
  }
};

__global__ __launch_bounds__(256) void k_ep_table(int nel, int width, EpShapes S, const int* __restrict__ geom, const int* __restrict__ ed, int* __restrict__ out) {
  const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= (size_t)nel * width) return;
  const int e = (int)(t / width), n = (int)(t % width);
  const int g = geom[e];
  const int nc = g >= 0 && g < EM_G ? S.nc[g] : 0;
  out[t] = ed[(size_t)e * EM_W + (n < nc ? n : 0)];
}

__global__ __launch_bounds__(256) void k_ep_first(int nel, const int* __restrict__ geom, int* __restrict__ first) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= nel) return;
  const int g = geom[e];
  if (g < 0 || g >= EM_G) return;
  if (first[g] > e) atomicMin(&first[g], e);     // a stale read can only show a larger value: the minimum is taken all the same
}

// flag[k * (nel + 1) + e] = element e is of shape k
__global__ __launch_bounds__(256) void k_ep_flags(int nel, int ns, EpShapes S, const int* __restrict__ geom, int* __restrict__ flag) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= nel) return;
  const int g = geom[e];
  const int k = g >= 0 && g < EM_G ? S.idx[g] : -1;
  for (int q = 0; q < ns; q++) flag[(size_t)q * (nel + 1) + e] = q == k ? 1 : 0;
}

// slot[k * (nel + 1) + e]: the scanned flags
__global__ __launch_bounds__(256) void k_ep_compact(int nel, EpShapes S, const int* __restrict__ geom, const int* __restrict__ ed, const int* __restrict__ slot,
                                                    int* __restrict__ T, int* __restrict__ slot_elem, int* __restrict__ err) {
  const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= (size_t)nel * EM_W) return;
  const int e = (int)(t / EM_W), n = (int)(t % EM_W);
  const int g = geom[e];
  const int k = g >= 0 && g < EM_G ? S.idx[g] : -1;
  if (k < 0) {
    atomicExch(err, 1);
    return;
  }
  const int s = slot[(size_t)k * (nel + 1) + e], nc = S.ncs[k];
  if (s < 0 || s >= S.nslot[k]) {               // the shape counts of the mesh are not those of its elements
    atomicExch(err, 1);
    return;
  }
  if (n == 0) slot_elem[S.elem_base[k] + s] = e;
  if (n < nc) T[S.row_base[k] + s * nc + n] = ed[t];
}

__device__ __forceinline__ int ep_elem_of_row(const EpShapes& S, const int* __restrict__ slot_elem, int r) {
  const int k = r >= S.row_base[2] ? 2 : r >= S.row_base[1] ? 1 : 0;
  return slot_elem[S.elem_base[k] + (r - S.row_base[k]) / S.ncs[k]];
}
// one thread per list entry: its rank in its list by (element, row id)
__global__ __launch_bounds__(256) void k_ep_order(int nadj, EpShapes S, const int* __restrict__ T, const int* __restrict__ slot_elem, const int* __restrict__ ptr,
                                                  const int* __restrict__ in, int* __restrict__ out) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= nadj) return;
  const int r = in[p], d = T[r];
  const int a0 = ptr[d], a1 = ptr[d + 1];
  const int e = ep_elem_of_row(S, slot_elem, r);
  int rank = 0;
  for (int a = a0; a < a1; a++) {
    const int q = in[a], eq = ep_elem_of_row(S, slot_elem, q);
    rank += (eq < e || (eq == e && q < r)) ? 1 : 0;
  }
  out[a0 + rank] = r;
}

__device__ __forceinline__ bool ep_hit(int flag, int nflags, const int* __restrict__ flags) {
  bool hit = false;
  for (int q = 0; q < nflags; q++) hit = hit || flags[q] == flag;
  return hit;
}
__global__ __launch_bounds__(256) void k_ep_face_mark(int nel, EpFaces F, const int* __restrict__ geom, const int* __restrict__ ff, int nflags,
                                                      const int* __restrict__ flags, int* __restrict__ mark) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= nel * EM_F) return;
  const int e = t / EM_F, f = t % EM_F, g = geom[e];
  mark[t] = g >= 0 && g < EM_G && f < F.nf[g] && ep_hit(ff[t], nflags, flags) ? 1 : 0;
}
// pos: the scanned marks
__global__ __launch_bounds__(256) void k_ep_face_fill(int nel, EpFaces F, const int* __restrict__ geom, const int* __restrict__ ed, const int* __restrict__ pos, int cap,
                                                      int* __restrict__ elem, int* __restrict__ face, int* __restrict__ nodes, int* __restrict__ nn) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= nel * EM_F) return;
  const int o = pos[t];
  if (pos[t + 1] == o || o < 0 || o >= cap) return;
  const int e = t / EM_F, f = t % EM_F, g = geom[e], n = F.n[g][f];
  elem[o] = e;
  face[o] = f;
  nn[o] = n;
  for (int i = 0; i < EP_FN; i++) nodes[(size_t)o * EP_FN + i] = i < n ? ed[(size_t)e * EM_W + F.node[g][f][i]] : -1;
}

__global__ __launch_bounds__(256) void k_ep_owner_mark(int nel, EpFaces F, const int* __restrict__ geom, const int* __restrict__ ed, const int* __restrict__ ff,
                                                       int nflags, const int* __restrict__ flags, int own, int* __restrict__ win) {
  const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= (size_t)nel * EM_F * EP_FN) return;
  const int ef = (int)(t / EP_FN), i = (int)(t % EP_FN), e = ef / EM_F, f = ef % EM_F;
  const int g = geom[e];
  if (g < 0 || g >= EM_G || f >= F.nf[g] || i >= F.n[g][f]) return;
  if (!ep_hit(ff[ef], nflags, flags)) return;
  const int d = ed[(size_t)e * EM_W + F.node[g][f][i]];
  if (d >= 0 && d < own) atomicMax(&win[d], ef);
}
__global__ __launch_bounds__(256) void k_ep_owner_flag(int own, const int* __restrict__ win, int* __restrict__ mark) {
  const int d = blockIdx.x * 256 + threadIdx.x;
  if (d < own) mark[d] = win[d] >= 0 ? 1 : 0;
}
__global__ __launch_bounds__(256) void k_ep_owner_fill(int own, int dim, const int* __restrict__ pos, int cap, const int* __restrict__ win, const int* __restrict__ ff,
                                                       const double* __restrict__ x, int* __restrict__ dofs, int* __restrict__ oflag, double* __restrict__ coords) {
  const int d = blockIdx.x * 256 + threadIdx.x;
  if (d >= own) return;
  const int o = pos[d];
  if (pos[d + 1] == o || o < 0 || o >= cap) return;
  dofs[o] = d;
  oflag[o] = ff[win[d]];
  for (int c = 0; c < dim; c++) coords[(size_t)o * dim + c] = x[(size_t)d * dim + c];
}

int ep_face_tables(const char* who, int fe, EpFaces& FT) {
  memset(&FT, 0, sizeof(FT));
  for (int g = 0; g < EM_G; g++) {
    if (!ep_shape(g)) continue;
    const int nf = fhfe::nfaces_of(g);
    FH_REQUIRE(nf >= 0 && nf <= EM_F, "%s: unexpected face tables (shape %d)", who, g);
    FT.nf[g] = (signed char)nf;
    for (int f = 0; f < nf; f++) {
      int tmp[EP_FN];
      const int n = fhfe::face_nodes(g, fe, f, tmp);
      FH_REQUIRE(n >= 0 && n <= EP_FN, "%s: unexpected face tables (shape %d)", who, g);
      FT.n[g][f] = (signed char)n;
      for (int k = 0; k < n; k++) {
        FH_REQUIRE(tmp[k] >= 0 && tmp[k] < EM_W, "%s: unexpected face tables (shape %d)", who, g);
        FT.node[g][f][k] = (signed char)tmp[k];
      }
    }
  }
  return 0;
}

// the argument checks the two boundary calls share
int ep_boundary_args(const char* who, fh_elem_mesh_t M, int fe, int nflags, const int* flags, const int* count) {
  FH_REQUIRE(M && count, "%s: null argument", who);
  FH_REQUIRE(fe >= 0 && fe <= 2, "%s: fe must be 0 (linear), 1 (serendipity) or 2 (biquadratic), not %d", who, fe);
  FH_REQUIRE(nflags >= 0 && (flags || nflags == 0), "%s: %d flags and no list of them", who, nflags);
  FH_REQUIRE(M->own[fe] >= 0 && M->own[fe] <= M->nnode, "%s: the family owns %d of %d nodes", who, M->own[fe], M->nnode);
  FH_REQUIRE((int64_t)M->nel * EM_F < 2147483647ll, "%s: too many elements", who);
  return 0;
}
}   // namespace

extern "C" int fh_elem_mesh_matrix(fh_elem_mesh_t M, int fe, fh_mat_t* K) {
  FH_GUARD_BEGIN
  const char* who = "fh_elem_mesh_matrix";
  FH_REQUIRE(M && K, "%s: null argument", who);
  FH_REQUIRE(fe >= 0 && fe <= 2, "%s: fe must be 0 (linear), 1 (serendipity) or 2 (biquadratic), not %d", who, fe);
  const int own = M->own[fe];
  FH_REQUIRE(own >= 0 && own <= M->nnode, "%s: the family owns %d of %d nodes", who, own, M->nnode);
  EpShapes S;
  memset(&S, 0, sizeof(S));
  int width = 1;
  for (int g = 0; g < EM_G; g++) {
    if (!M->count[g]) continue;
    FH_REQUIRE(ep_shape(g), "%s: the mesh holds elements of shape code %d", who, g);
    S.nc[g] = fhfe::ndofs_of(g, fe);
    FH_REQUIRE(S.nc[g] >= 1 && S.nc[g] <= EM_W, "%s: the family has %d dofs on shape %d", who, S.nc[g], g);
    width = std::max(width, S.nc[g]);
  }
  fh_ctx_t ctx = M->ctx;
  if (!M->nel) return mat_create_from_elements_impl(ctx, 0, 1, nullptr, nullptr, own, own, K);
  EpScratch B(ctx, who);
  int* d_tab;
  const size_t ne = (size_t)M->nel * width;
  if (B.get(&d_tab, ne)) {
    hipStreamSynchronize(ctx->stream);
    return 2;
  }
  hipLaunchKernelGGL(k_ep_table, dim3((unsigned)((ne + 255) / 256)), dim3(256), 0, ctx->stream, M->nel, width, S, M->d_geom, M->d_ed, d_tab);
  int rc = 0;
  if (hipGetLastError() != hipSuccess) {
    fh_set_error("%s: launch failed", who);
    rc = 1;
  }
  if (!rc) rc = mat_create_from_elements_impl(ctx, M->nel, width, nullptr, d_tab, own, own, K);
  hipStreamSynchronize(ctx->stream);             // the table is freed on return
  return rc;
  FH_GUARD_END("fh_elem_mesh_matrix")
}

extern "C" int fh_generic_assembler_create_from_mesh(fh_elem_mesh_t M, int fe, int order, fh_mat_t KK, fh_generic_assembler_t* out) {
  FH_GUARD_BEGIN
  const char* who = "fh_generic_assembler_create_from_mesh";
  FH_REQUIRE(M && KK && out, "%s: null argument", who);
  *out = nullptr;
  // ---- every check first: nothing is allocated on the device before the last of them ----
  FH_REQUIRE(fe >= 0 && fe <= 2, "%s: fe must be 0 (linear), 1 (serendipity) or 2 (biquadratic), not %d", who, fe);
  FH_REQUIRE(M->ctx == KK->ctx, "%s: the mesh and the matrix live on different contexts", who);
  const int nel = M->nel, nnode = M->nnode, ndof = M->own[fe];
  FH_REQUIRE(nel >= 1 && nnode >= 1 && ndof >= 1 && ndof <= nnode, "%s: an empty mesh (%d elements, %d nodes, %d of them the family's)", who, nel, nnode, ndof);
  FH_REQUIRE(KK->m == ndof && KK->n == ndof && (int)KK->h_rowptr.size() == ndof + 1,
             "%s: the matrix has %d rows and %d columns; it must be square of the %d dofs the family owns, with a host row table", who, KK->m, KK->n, ndof);
  FH_REQUIRE((int64_t)nel * EM_W < 2147483647ll, "%s: too many elements", who);
  GenMesh m;                      // shapes by code until the device has told the order of their first elements
  int64_t total = 0;
  for (int g = 0; g < EM_G; g++) {
    if (!M->count[g]) continue;
    FH_REQUIRE(ep_shape(g) && M->count[g] > 0, "%s: %lld elements of shape code %d", who, (long long)M->count[g], g);
    FH_REQUIRE(m.ns < 3, "%s: more than three shapes in one mesh", who);
    m.shapes[m.ns] = g;
    m.nslot[m.ns++] = (int)M->count[g];
    total += M->count[g];
  }
  FH_REQUIRE(total == nel, "%s: the shape counts of the mesh give %lld elements, it has %d", who, (long long)total, nel);
  FH_TRY(gen_shape_tables(who, fe, order, EM_W, m));
  FH_REQUIRE(m.dim == M->dim, "%s: %d-dimensional shapes in a %d-dimensional mesh", who, m.dim, M->dim);
  {                               // the checks of the host side do not depend on the order of the shapes
    fh_generic_assembler_t probe = nullptr;
    FH_TRY(gp_plan_host(who, M->ctx, m, nel, nnode, KK, &probe));
    delete probe;
  }

  // ---- device side ----
  fh_ctx_t ctx = M->ctx;
  hipStream_t st = ctx->stream;
  EpScratch B(ctx, who);
  auto fail = [&](int code) {     // nothing is freed under a running kernel
    hipStreamSynchronize(st);
    return code;
  };
  int *d_first, *d_err;
  if (B.get(&d_first, EM_G) || B.get(&d_err, 1)) return fail(2);
  int first[EM_G];
  hipError_t he = hipMemsetAsync(d_first, 0x7F, EM_G * sizeof(int), st);
  if (he == hipSuccess) he = hipMemsetAsync(d_err, 0, 2 * sizeof(int), st);
  if (he == hipSuccess) {
    hipLaunchKernelGGL(k_ep_first, dim3(fh_div_up(nel, 256)), dim3(256), 0, st, nel, M->d_geom, d_first);
    he = hipGetLastError();
  }
  if (he == hipSuccess) he = hipMemcpyAsync(first, d_first, sizeof(first), hipMemcpyDeviceToHost, st);
  if (he == hipSuccess) he = hipStreamSynchronize(st);
  if (he != hipSuccess) {
    fh_set_error("%s: %s", who, hipGetErrorString(he));
    return fail(1);
  }
  for (int k = 0; k < m.ns; k++)
    if (first[m.shapes[k]] < 0 || first[m.shapes[k]] >= nel) {
      fh_set_error("%s: the mesh counts %d elements of shape code %d and holds none", who, m.nslot[k], m.shapes[k]);
      return fail(2);
    }
  for (int a = 0; a < m.ns; a++)                 // at most three: the order of the first elements
    for (int b = a + 1; b < m.ns; b++)
      if (first[m.shapes[b]] < first[m.shapes[a]]) {
        std::swap(m.shapes[a], m.shapes[b]);
        std::swap(m.nc[a], m.nc[b]);
        std::swap(m.nslot[a], m.nslot[b]);
        m.w[a].swap(m.w[b]);
        m.phi[a].swap(m.phi[b]);
        m.dphi[a].swap(m.dphi[b]);
      }
  fh_generic_assembler_t as = nullptr;
  if (int rc = gp_plan_host(who, ctx, m, nel, nnode, KK, &as)) return fail(rc);
  EpShapes S;
  memset(&S, 0, sizeof(S));
  for (int g = 0; g < EM_G; g++) S.idx[g] = -1;
  for (int k = 0, eb = 0; k < 3; k++) {
    S.row_base[k] = as->rows.row_base[k];
    S.ncs[k] = k < m.ns ? m.nc[k] : 1;
    S.nslot[k] = k < m.ns ? m.nslot[k] : 0;
    S.elem_base[k] = eb;
    if (k < m.ns) {
      S.idx[m.shapes[k]] = k;
      S.nc[m.shapes[k]] = m.nc[k];
      eb += m.nslot[k];
    }
  }
  const int ns = m.ns;
  const int nrows = (int)as->nrows;
  int *d_slot, *d_bsum, *d_slot_elem;
  if (B.get(&d_slot, (size_t)ns * ((size_t)nel + 1)) || B.get(&d_bsum, (size_t)nel / FH_SCAN_BLOCK + 2) || B.get(&d_slot_elem, (size_t)nel)) {
    gp_free(as);
    return fail(2);
  }
  int* d_T = (int*)gp_alloc(as, (size_t)nrows * sizeof(int));
  as->d_coords = (double*)gp_alloc(as, (size_t)nnode * as->dim * sizeof(double));
  as->d_adj_ptr = (int*)gp_alloc(as, ((size_t)ndof + 1) * sizeof(int));
  if (!d_T || !as->d_coords || !as->d_adj_ptr) {
    gp_free(as);
    fh_set_error("%s: out of device memory", who);
    return fail(2);
  }
  for (int k = 0; k < ns; k++) as->d_ed[k] = d_T + as->rows.row_base[k];
  hipLaunchKernelGGL(k_ep_flags, dim3(fh_div_up(nel, 256)), dim3(256), 0, st, nel, ns, S, M->d_geom, d_slot);
  int rc = 0;
  for (int k = 0; k < ns && !rc; k++) rc = fh_device_exclusive_scan(st, d_slot + (size_t)k * (nel + 1), d_slot + (size_t)k * (nel + 1), nel, d_bsum);
  if (!rc) {
    const size_t nthr = (size_t)nel * EM_W;
    hipLaunchKernelGGL(k_ep_compact, dim3((unsigned)((nthr + 255) / 256)), dim3(256), 0, st, nel, S, M->d_geom, M->d_ed, d_slot, d_T, d_slot_elem, d_err);
    he = hipMemcpyAsync(as->d_coords, M->d_x, (size_t)nnode * as->dim * sizeof(double), hipMemcpyDeviceToDevice, st);
    if (he == hipSuccess) he = hipGetLastError();
    if (he != hipSuccess) {
      fh_set_error("%s: %s", who, hipGetErrorString(he));
      rc = 1;
    }
  }
  fh_dof_lists L;                 // freed on return: every path below has synchronised the stream by then
  if (!rc) rc = fh_dof_lists_build(ctx, who, (size_t)nrows, 1, d_T, ndof, ndof, false, &L);
  int err = 0;
  if (!rc) {                      // the build has synchronised the stream: the slots are written
    he = hipMemcpy(&err, d_err, sizeof(int), hipMemcpyDeviceToHost);
    if (he != hipSuccess) {
      fh_set_error("%s: %s", who, hipGetErrorString(he));
      rc = 1;
    } else if (err) {
      fh_set_error("%s: the shapes of the elements are not the %d the mesh counts", who, ns);
      rc = 2;
    }
  }
  if (rc) {
    gp_free(as);
    return fail(rc);
  }
  const int nadj = L.ptr[ndof];
  as->nadj = nadj;
  as->d_adj = (int*)gp_alloc(as, (size_t)nadj * sizeof(int));
  if (!as->d_adj) {
    gp_free(as);
    fh_set_error("%s: out of device memory", who);
    return fail(2);
  }
  he = hipMemcpyAsync(as->d_adj_ptr, L.d_ptr, ((size_t)ndof + 1) * sizeof(int), hipMemcpyDeviceToDevice, st);
  if (he == hipSuccess && nadj) {
    hipLaunchKernelGGL(k_ep_order, dim3(fh_div_up(nadj, 256)), dim3(256), 0, st, nadj, S, d_T, d_slot_elem, L.d_ptr, L.d_adj, as->d_adj);
    he = hipGetLastError();
  }
  if (he != hipSuccess) {
    fh_set_error("%s: %s", who, hipGetErrorString(he));
    gp_free(as);
    return fail(1);
  }
  unsigned long long miss = 0;
  if (int rw = gp_plan_work(who, as, m, KK, &miss)) return fail(rw);      // the object is gone
  if (miss != ~0ull) {            // the one path that fetches the slot -> element table
    const int k = (int)(miss >> 56);
    const long long idx = (long long)(miss & ((1ull << 56) - 1));
    const int nc = m.nc[k], j = (int)(idx % nc), i = (int)((idx / nc) % nc);
    const long long s = idx / ((long long)nc * nc);
    int e = -1, di = -1, dj = -1;
    if (k < ns && s < m.nslot[k]) {
      hipMemcpy(&e, d_slot_elem + S.elem_base[k] + s, sizeof(int), hipMemcpyDeviceToHost);
      hipMemcpy(&di, as->d_ed[k] + s * nc + i, sizeof(int), hipMemcpyDeviceToHost);
      hipMemcpy(&dj, as->d_ed[k] + s * nc + j, sizeof(int), hipMemcpyDeviceToHost);
    }
    gp_free(as);
    fh_set_error("%s: element %d: the pair (%d, %d) = dofs (%d, %d) is not in the pattern of the matrix", who, e, i, j, di, dj);
    return 2;
  }
  *out = as;
  return 0;
  FH_GUARD_END("fh_generic_assembler_create_from_mesh")
}

extern "C" int fh_elem_mesh_boundary_faces(fh_elem_mesh_t M, int fe, int nflags, const int* flags, int* nfaces, int* elem, int* face, int* nodes, int* nn) {
  FH_GUARD_BEGIN
  const char* who = "fh_elem_mesh_boundary_faces";
  FH_TRY(ep_boundary_args(who, M, fe, nflags, flags, nfaces));
  const bool fill = elem || face || nodes || nn;
  FH_REQUIRE(!fill || (elem && face && nodes && nn), "%s: all four arrays, or none of them (the call for the count)", who);
  const int given = *nfaces;
  FH_REQUIRE(!fill || given >= 0, "%s: nfaces is %d (call with the arrays NULL first)", who, given);
  if (!nflags || !M->nel) {
    FH_REQUIRE(!fill || given == 0, "%s: nfaces is %d, the list has 0 entries (call with the arrays NULL first)", who, given);
    *nfaces = 0;
    return 0;
  }
  EpFaces FT;
  FH_TRY(ep_face_tables(who, fe, FT));
  fh_ctx_t ctx = M->ctx;
  hipStream_t st = ctx->stream;
  const int nt = M->nel * EM_F, cap = fill ? given : 0;
  EpScratch B(ctx, who);
  int *d_flags, *d_mark, *d_bsum, *d_elem, *d_face, *d_nodes, *d_nn;
  if (B.get(&d_flags, (size_t)nflags) || B.get(&d_mark, (size_t)nt + 1) || B.get(&d_bsum, (size_t)nt / FH_SCAN_BLOCK + 2) || B.get(&d_elem, (size_t)cap) ||
      B.get(&d_face, (size_t)cap) || B.get(&d_nodes, (size_t)cap * EP_FN) || B.get(&d_nn, (size_t)cap)) {
    hipStreamSynchronize(st);
    return 2;
  }
  int total = 0, rc = 0;
  hipError_t he = hipMemcpyAsync(d_flags, flags, (size_t)nflags * sizeof(int), hipMemcpyHostToDevice, st);
  if (he == hipSuccess) {
    hipLaunchKernelGGL(k_ep_face_mark, dim3(fh_div_up(nt, 256)), dim3(256), 0, st, M->nel, FT, M->d_geom, M->d_ff, nflags, d_flags, d_mark);
    he = hipGetLastError();
  }
  if (he == hipSuccess) rc = fh_device_exclusive_scan(st, d_mark, d_mark, nt, d_bsum);
  if (he == hipSuccess && !rc) he = hipMemcpyAsync(&total, d_mark + nt, sizeof(int), hipMemcpyDeviceToHost, st);
  if (he == hipSuccess && !rc) he = hipStreamSynchronize(st);
  if (he == hipSuccess && !rc && fill && total == given && total) {
    hipLaunchKernelGGL(k_ep_face_fill, dim3(fh_div_up(nt, 256)), dim3(256), 0, st, M->nel, FT, M->d_geom, M->d_ed, d_mark, cap, d_elem, d_face, d_nodes, d_nn);
    he = hipGetLastError();
    if (he == hipSuccess) he = hipMemcpyAsync(elem, d_elem, (size_t)total * sizeof(int), hipMemcpyDeviceToHost, st);
    if (he == hipSuccess) he = hipMemcpyAsync(face, d_face, (size_t)total * sizeof(int), hipMemcpyDeviceToHost, st);
    if (he == hipSuccess) he = hipMemcpyAsync(nodes, d_nodes, (size_t)total * EP_FN * sizeof(int), hipMemcpyDeviceToHost, st);
    if (he == hipSuccess) he = hipMemcpyAsync(nn, d_nn, (size_t)total * sizeof(int), hipMemcpyDeviceToHost, st);
  }
  const hipError_t hs = hipStreamSynchronize(st);       // the scratch is freed on return
  if (he == hipSuccess) he = hs;
  if (he != hipSuccess) {
    fh_set_error("%s: %s", who, hipGetErrorString(he));
    return 1;
  }
  if (rc) return rc;
  FH_REQUIRE(!fill || total == given, "%s: nfaces is %d, the list has %d entries (call with the arrays NULL first)", who, given, total);
  *nfaces = total;
  return 0;
  FH_GUARD_END("fh_elem_mesh_boundary_faces")
}

extern "C" int fh_elem_mesh_boundary_owners(fh_elem_mesh_t M, int fe, int nflags, const int* flags, int* ndofs, int* dofs, int* owner_flag, double* coords) {
  FH_GUARD_BEGIN
  const char* who = "fh_elem_mesh_boundary_owners";
  FH_TRY(ep_boundary_args(who, M, fe, nflags, flags, ndofs));
  const bool fill = dofs || owner_flag || coords;
  FH_REQUIRE(!fill || (dofs && owner_flag && coords), "%s: all three arrays, or none of them (the call for the count)", who);
  const int given = *ndofs, own = M->own[fe], dim = M->dim;
  FH_REQUIRE(!fill || given >= 0, "%s: ndofs is %d (call with the arrays NULL first)", who, given);
  if (!nflags || !M->nel || !own) {
    FH_REQUIRE(!fill || given == 0, "%s: ndofs is %d, the list has 0 entries (call with the arrays NULL first)", who, given);
    *ndofs = 0;
    return 0;
  }
  EpFaces FT;
  FH_TRY(ep_face_tables(who, fe, FT));
  fh_ctx_t ctx = M->ctx;
  hipStream_t st = ctx->stream;
  const int cap = fill ? given : 0;
  EpScratch B(ctx, who);
  int *d_flags, *d_win, *d_mark, *d_bsum, *d_dofs, *d_oflag;
  double* d_xy;
  if (B.get(&d_flags, (size_t)nflags) || B.get(&d_win, (size_t)own) || B.get(&d_mark, (size_t)own + 1) || B.get(&d_bsum, (size_t)own / FH_SCAN_BLOCK + 2) ||
      B.get(&d_dofs, (size_t)cap) || B.get(&d_oflag, (size_t)cap) || B.get(&d_xy, (size_t)cap * dim)) {
    hipStreamSynchronize(st);
    return 2;
  }
  int total = 0, rc = 0;
  hipError_t he = hipMemcpyAsync(d_flags, flags, (size_t)nflags * sizeof(int), hipMemcpyHostToDevice, st);
  if (he == hipSuccess) he = hipMemsetAsync(d_win, 0xFF, (size_t)own * sizeof(int), st);       // -1: no face yet
  if (he == hipSuccess) {
    const size_t nthr = (size_t)M->nel * EM_F * EP_FN;
    hipLaunchKernelGGL(k_ep_owner_mark, dim3((unsigned)((nthr + 255) / 256)), dim3(256), 0, st, M->nel, FT, M->d_geom, M->d_ed, M->d_ff, nflags, d_flags, own, d_win);
    hipLaunchKernelGGL(k_ep_owner_flag, dim3(fh_div_up(own, 256)), dim3(256), 0, st, own, d_win, d_mark);
    he = hipGetLastError();
  }
  if (he == hipSuccess) rc = fh_device_exclusive_scan(st, d_mark, d_mark, own, d_bsum);
  if (he == hipSuccess && !rc) he = hipMemcpyAsync(&total, d_mark + own, sizeof(int), hipMemcpyDeviceToHost, st);
  if (he == hipSuccess && !rc) he = hipStreamSynchronize(st);
  if (he == hipSuccess && !rc && fill && total == given && total) {
    hipLaunchKernelGGL(k_ep_owner_fill, dim3(fh_div_up(own, 256)), dim3(256), 0, st, own, dim, d_mark, cap, d_win, M->d_ff, M->d_x, d_dofs, d_oflag, d_xy);
    he = hipGetLastError();
    if (he == hipSuccess) he = hipMemcpyAsync(dofs, d_dofs, (size_t)total * sizeof(int), hipMemcpyDeviceToHost, st);
    if (he == hipSuccess) he = hipMemcpyAsync(owner_flag, d_oflag, (size_t)total * sizeof(int), hipMemcpyDeviceToHost, st);
    if (he == hipSuccess) he = hipMemcpyAsync(coords, d_xy, (size_t)total * dim * sizeof(double), hipMemcpyDeviceToHost, st);
  }
  const hipError_t hs = hipStreamSynchronize(st);       // the scratch is freed on return
  if (he == hipSuccess) he = hs;
  if (he != hipSuccess) {
    fh_set_error("%s: %s", who, hipGetErrorString(he));
    return 1;
  }
  if (rc) return rc;
  FH_REQUIRE(!fill || total == given, "%s: ndofs is %d, the list has %d entries (call with the arrays NULL first)", who, given, total);
  *ndofs = total;
  return 0;
  FH_GUARD_END("fh_elem_mesh_boundary_owners")
}
