// The generic (dim, nc, ng) Poisson assembly: every element family fh_fe has tables for, on any mesh whose element table the caller gives (nloc nodes per element
// in the family's local order; dof id = node id, the classes numbered one after the other as every FEMuS mesh is) -- triangles, tetrahedra, prisms, mixed shapes:
//   K_ij += grad phi_i . grad phi_j w,   RES_i += (scale f phi_i - grad phi_i . grad u) w        (applications/001_Poisson/main.cpp:430-470 with V = 0)
// with elem_type::Jacobian (Jac[a][b] = sum_n dphi_n/dxi_a x_n[b], grad phi_n = Jac^-1 dphi_n, w = det w_g), the rows summed in ascending element order: the
// grouping of the reference's add_matrix_blocked / add_vector_blocked, no atomics.  Two drivers share ONE element body, gen_element_pass:
//
// One-shot calls (fh_assemble_poisson_rows / fh_assemble_poisson_mixed, at the end of this file) prepare everything on every call -- the dof -> element adjacency
// on the host, uploads, a dozen allocations, a linear search of every (i, j) in its CSR row -- and run one wave per element (k_poisson_pairs_generic) and one
// thread per row (k_poisson_rows_generic).  They are the independent yardstick of the resident object: their own launch geometry, search and row pass.
//
// Resident plan (fh_generic_assembler_*): all of that is made ONCE and kept on the device; an assembly then only enqueues kernels.  Per shape k of the mesh (at
// most three of one dimension, in the order of their first element):
//   d_ed[k]     [nslot_k][nc_k]  the dofs of the shape's elements, slot = rank of the element among the elements of its shape (ascending element order)
//   Kb / Pos    element row (slot, i) of shape k starts at kb_base[k] + (slot nc_k + i) nc_k: its nc_k values, and beside them the CSR position of every
//               one, found at create by a binary search of the (sorted) row on the device; a pair the pattern does not hold fails create
//   Fb / adj    the element row's residual entry at row_base[k] + slot nc_k + i = the row's id; adj lists the ids of a dof in ascending ELEMENT order
// The plan has two builders: fh_generic_assembler_create here, from host arrays, and fh_generic_assembler_create_from_mesh (fh_elemplan.hip), from a resident
// element mesh; the object and the steps they share (gen_shape_tables, gp_plan_host, gp_plan_work) are declared in fh_generic.h.
//
// Element pass of the plan, one launch per shape (uniform waves on mixed meshes): workgroups of 256 threads, L = 64 / 32 / 16 lanes per element (1 / 2 / 4
// elements per wave) from the shape's nc (nc + 1) / 2 pairs; dynamic LDS sized by the shape's nc and Gauss chunk, w / phi / dphi staged once per workgroup where
// they fit.  Its values are bitwise the one-shot call's because both kernels inline the same body: Gauss points ascending, nodes ascending inside a point, K_ji
// the bits of K_ij.  What the two pass differently -- lanes per element, the node stride of the LDS arrays, the length of the Gauss chunk -- moves addresses and
// barriers, not one operation: the accumulators run through all points in ascending order whatever the chunk is.
//
// Row pass of the plan: lpr lanes per row (a group never leaves its wave), the row's sums in LDS: element rows in ascending element order, the lanes of the group
// split one element row's entries (distinct positions), LDS operations of one wave complete in order -- so every entry sees its additions in ascending element
// order, starting from 0.0 as the one-shot row thread does.  No search, no atomics, no read-modify-write of global memory.
//
// fh_quasilinear.hip, fh_transient.hip and fh_system.hip put three more element bodies on the same plan (unsymmetric Jacobians from run-time coefficient
// programs).  They share the row pass, the program buffer and the call checks below (gp_launch_rows, gp_upload_program, gp_check_call), the plan step of a body
// (gp_plan_body: Gauss chunk, table staging, LDS; gp_dispatch: its <L, TL> kernel), and most of them with this body the phases of fh_elembody.h: the kernel's
// prologue, (A) and (B).
#include "fh_elembody.h"
#include "fh_fe.h"
#include "fh_expr_device.h"
#include <algorithm>
#include <climits>

namespace {
constexpr int GEN_GC = 32;                    // Gauss points per chunk of the one-shot kernel

// doubles of LDS one element needs at node stride ns and chunk gc: X[ns][3], U[ns], JI[gc][9], WG[gc], FS[gc], GU[gc][3], G[gc][ns][3]
constexpr size_t gp_elem_doubles(int ns, int gc) { return (size_t)ns * 4 + (size_t)gc * 14 + (size_t)gc * ns * 3; }
constexpr int gp_pairs_per_lane(int L) { return L == 64 ? (GEN_NC * (GEN_NC + 1) / 2 + 63) / 64 : 2; }     // 378 pairs on 64 lanes: six; at most 2 L pairs where L < 64
inline int gp_lanes_per_element(int nc, int pack) {
  const int npair = nc * (nc + 1) / 2;
  if (!pack) return 64;
  return npair <= 32 ? 16 : npair <= 64 ? 32 : 64;     // two pairs per lane at most where elements share a wave
}
}  // namespace

// THE element body: L lanes form the matrix and the residual entries of one element whose dofs are dof_row[0 .. nc), in `lds` (gp_elem_doubles(ns, gcm) doubles).
// The Gauss points are taken gcm at a time through LDS: (A) lane = Gauss point: Jacobian, its inverse, weight, source value; (B) lanes over (Gauss point, node):
// the node's gradient; (C) lane = Gauss point: grad u; (D) lanes over the pairs i <= j of the element matrix (K_ji = K_ij bit for bit: the products commute) and
// over the residual entries.  Every sum is taken nodes ascending inside a Gauss point, Gauss points ascending.  On return pair k of this lane is (pi[k], pj[k])
// (-1: none) with the sum acc[k], and F is residual entry `lane` (lane < nc).  Every thread of the workgroup calls this, with the same ng and gcm: the barriers
// are workgroup barriers; a sub-group without an element passes active = false and touches nothing.
template <int L, int NPL>
__device__ __forceinline__ void gen_element_pass(bool active, int lane, int nc, int ng, int gcm, int ns, int dim, const double* w, const double* phi, const double* dphi,
                                                 const int* dof_row, const double* coords, const double* sol, double scale, const int* prog, int nprog,
                                                 const double* pconst, double* lds, int (&pi_out)[NPL], int (&pj_out)[NPL], double (&acc_out)[NPL], double& F_out) {
  double* X = lds;                                   // [ns][3]
  double* U = X + ns * 3;                            // [ns]
  double* JI = U + ns;                               // [gcm][9]
  double* WG = JI + gcm * 9;                         // [gcm] det w
  double* FS = WG + gcm;                             // [gcm] scale f(x_g)
  double* GU = FS + gcm;                             // [gcm][3]
  double* G = GU + gcm * 3;                          // [gcm][ns][3]
  if (active && lane < nc) {
    const int dof = dof_row[lane];
    for (int d = 0; d < 3; d++) X[lane * 3 + d] = d < dim ? coords[(size_t)dof * dim + d] : 0.0;
    U[lane] = sol ? sol[dof] : 0.0;
  }
  const int npair = nc * (nc + 1) / 2;
  // the lane's pairs and sums live in arrays of this function and are handed out at the end: written through the caller's references the pair arrays
  // end up in scratch memory (this body is optimised before it is inlined, and its two-way store to pi / pj cannot be split into registers afterwards)
  int pi[NPL], pj[NPL];
  double acc[NPL];
#pragma unroll
  for (int k = 0; k < NPL; k++) {
    int p = lane + L * k, i = 0;
    if (active && p < npair) {
      while (p >= nc - i) {
        p -= nc - i;
        i++;
      }
      pi[k] = i;
      pj[k] = i + p;
    } else {
      pi[k] = pj[k] = -1;
    }
    acc[k] = 0.0;
  }
  double F = 0.0;
  __syncthreads();
  for (int g0 = 0; g0 < ng; g0 += gcm) {
    const int gc = min(gcm, ng - g0);
    if (active)
      for (int l = lane; l < gc; l += L) {             // (A)
        const int g = g0 + l;
        double xq[4] = {0, 0, 0, 0};                      // x_g and t = 0 for the source program
        eb_point_geometry(X, dphi + (size_t)g * nc * dim, phi + (size_t)g * nc, w + g, nc, dim, JI + l * 9, WG + l, xq);
        FS[l] = prog ? scale * fh_expr_device_eval(prog, nprog, pconst, xq) : 0.0;
      }
    __syncthreads();
    if (active) eb_chunk_gradients<L, false>(lane, g0, gc, nc, ns, dim, dphi, JI, 9, G);     // (B)
    __syncthreads();
    if (active)
      for (int l = lane; l < gc; l += L) {             // (C)
        double gu[3] = {0, 0, 0};
        for (int n = 0; n < nc; n++)
          for (int q = 0; q < dim; q++) gu[q] += G[(l * ns + n) * 3 + q] * U[n];
        for (int q = 0; q < 3; q++) GU[l * 3 + q] = gu[q];
      }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < NPL; k++)                      // (D)
      if (pi[k] >= 0) {
        double a = acc[k];
        for (int l = 0; l < gc; l++) {
          const double *gi = G + (l * ns + pi[k]) * 3, *gj = G + (l * ns + pj[k]) * 3;
          double sacc = 0.0;
          for (int q = 0; q < dim; q++) sacc += gi[q] * gj[q];
          a += sacc * WG[l];
        }
        acc[k] = a;
      }
    if (active && lane < nc)
      for (int l = 0; l < gc; l++) {
        const double* gi = G + (l * ns + lane) * 3;
        double lap = 0.0;
        for (int q = 0; q < dim; q++) lap += gi[q] * GU[l * 3 + q];
        F += (FS[l] * phi[(size_t)(g0 + l) * nc + lane] - lap) * WG[l];
      }
    __syncthreads();
  }
#pragma unroll
  for (int k = 0; k < NPL; k++) pi_out[k] = pi[k], pj_out[k] = pj[k], acc_out[k] = acc[k];
  F_out = F;
}

// Element pass of the plan.  L lanes per element, 256 / L elements per workgroup; TL: the shape's tables in LDS.  Element rows compact: row i of slot s at
// Kb[(s nc + i) nc], its residual entry at Fb[s nc + i].
template <int L, bool TL>
__global__ __launch_bounds__(GP_THREADS) void k_gen_pairs(int nslot, int nc, int ng, int gcm, int dim, const double* __restrict__ gw, const double* __restrict__ gphi,
                                                          const double* __restrict__ gdphi, const int* __restrict__ ed, const double* __restrict__ coords,
                                                          const double* __restrict__ sol, double scale, const int* __restrict__ prog, int nprog,
                                                          const double* __restrict__ pconst, double* __restrict__ Kb, double* __restrict__ Fb) {
  extern __shared__ __attribute__((aligned(16))) double gen_smem[];
  constexpr int NPL = gp_pairs_per_lane(L);
  const EbGroup g = eb_prologue<L, TL>(gen_smem, nslot, nc, ng, dim, nc * 4 + gcm * 14 + gcm * nc * 3, gw, gphi, gdphi);
  int pi[NPL], pj[NPL];
  double acc[NPL], F;
  gen_element_pass<L, NPL>(g.active, g.lane, nc, ng, gcm, nc, dim, g.w, g.phi, g.dphi, ed + (size_t)g.slot * nc, coords, sol, scale, prog, nprog, pconst, g.lds, pi,
                           pj, acc, F);
  if (!g.active) return;
  double* out = Kb + (size_t)g.slot * nc * nc;
#pragma unroll
  for (int k = 0; k < NPL; k++)
    if (pi[k] >= 0) {
      out[(size_t)pi[k] * nc + pj[k]] = acc[k];
      if (pi[k] != pj[k]) out[(size_t)pj[k] * nc + pi[k]] = acc[k];
    }
  if (g.lane < nc) Fb[(size_t)g.slot * nc + g.lane] = F;
}

// create: the CSR position of every entry of every element row of one shape, by binary search in the sorted row; the smallest entry the pattern misses -> *miss
__global__ __launch_bounds__(256) void k_gen_positions(long long nent, int nc, const int* __restrict__ ed, const int* __restrict__ rowptr, const int* __restrict__ col,
                                                       int* __restrict__ Pos, unsigned long long* __restrict__ miss, unsigned long long tag) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= nent) return;
  const long long row = idx / nc;                // slot * nc + i
  const int j = (int)(idx - row * nc);
  const long long slot = row / nc;
  const int r = ed[row], c = ed[slot * nc + j];
  int lo = rowptr[r], hi = rowptr[r + 1] - 1, at = -1;
  while (lo <= hi) {
    const int mid = lo + (hi - lo) / 2, v = col[mid];
    if (v == c) {
      at = mid;
      break;
    }
    if (v < c) lo = mid + 1;
    else hi = mid - 1;
  }
  Pos[idx] = at;
  if (at < 0) atomicMin(miss, tag | (unsigned long long)idx);
}

// Row pass: lpr lanes (a power of two <= 64) per row, the row's sums in LDS (maxrow doubles per group).
__global__ __launch_bounds__(GP_THREADS) void k_gen_rows(int ndof, int lpr, int maxrow, GenRowShapes sh, const int* __restrict__ adj_ptr, const int* __restrict__ adj,
                                                         const double* __restrict__ Kb, const int* __restrict__ Pos, const double* __restrict__ Fb,
                                                         const int* __restrict__ rowptr, double* __restrict__ val, double* __restrict__ res) {
  extern __shared__ __attribute__((aligned(16))) double gen_racc[];
  const int grp = threadIdx.x / lpr, t = threadIdx.x % lpr;
  const int r = blockIdx.x * (GP_THREADS / lpr) + grp;
  if (r >= ndof) return;                         // no workgroup barrier below
  double* acc = gen_racc + (size_t)grp * maxrow;
  const int rs = rowptr[r], n = rowptr[r + 1] - rs;
  for (int k = t; k < n; k += lpr) acc[k] = 0.0;
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
  double racc = 0.0;
  for (int a = adj_ptr[r], ae = adj_ptr[r + 1]; a < ae; a++) {
    const int erow = adj[a];
    const int k = erow >= sh.row_base[2] ? 2 : erow >= sh.row_base[1] ? 1 : 0;
    const int nc = sh.nc[k];
    const long long off = sh.kb_base[k] + (long long)(erow - sh.row_base[k]) * nc;
    if (t == 0) racc += Fb[erow];
    for (int j = t; j < nc; j += lpr) acc[Pos[off + j] - rs] += Kb[off + j];
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
  }
  for (int k = t; k < n; k += lpr) val[rs + k] = acc[k];
  if (t == 0) res[r] = racc;
}

int gen_shape_tables(const char* who, int fe, int order, int nloc, GenMesh& m) {
  FH_REQUIRE(order >= 0 && order <= 4, "%s: unsupported Gauss rule", who);       // fhfe::shape_tables sizes its arrays by the rule before it checks it
  m.dim = fhfe::dim_of(m.shapes[0]);
  for (int k = 0; k < m.ns; k++) {
    FH_REQUIRE(fhfe::dim_of(m.shapes[k]) == m.dim, "%s: the shapes of one mesh have one dimension (shapes %d and %d)", who, m.shapes[0], m.shapes[k]);
    m.nc[k] = fhfe::ndofs_of(m.shapes[k], fe);
    FH_REQUIRE(m.nc[k] >= 1 && m.nc[k] <= GEN_NC && nloc >= m.nc[k], "%s: %d nodes per element given, the family has %d", who, nloc, m.nc[k]);
    FH_REQUIRE(fhfe::shape_tables(m.shapes[k], fe, order, m.w[k], m.phi[k], m.dphi[k]) == 0, "%s: unsupported Gauss rule", who);
    m.ncmax = std::max(m.ncmax, m.nc[k]);
  }
  return 0;
}

// elem_geom[nel] names the shape of every element (nullptr: every element is `geom`); the dofs of an element are the first nc of its nloc
static int gen_mesh(const char* who, int fe, int order, int nel, int nloc, const int* elem_geom, int geom, const int* elem_dof, int nnode, int ndof, GenMesh& m) {
  m.eshape.assign(nel, 0);
  if (elem_geom) {
    for (int e = 0; e < nel; e++) {
      int k = 0;
      while (k < m.ns && m.shapes[k] != elem_geom[e]) k++;
      if (k == m.ns) {
        FH_REQUIRE(m.ns < 3, "%s: more than three shapes in one mesh (element %d)", who, e);
        FH_REQUIRE(elem_geom[e] >= 0 && elem_geom[e] <= 5, "%s: element %d: shape %d", who, e, elem_geom[e]);
        m.shapes[m.ns++] = elem_geom[e];
      }
      m.eshape[e] = (unsigned char)k;
    }
  } else {
    FH_REQUIRE(geom >= 0 && geom <= 5, "%s: geom must be 0 (hex), 1 (quad), 2 (line), 3 (triangle), 4 (tetrahedron) or 5 (prism)", who);
    m.shapes[m.ns++] = geom;
  }
  FH_TRY(gen_shape_tables(who, fe, order, nloc, m));
  m.adj_ptr.assign((size_t)ndof + 1, 0);
  for (int e = 0; e < nel; e++) {
    const int k = m.eshape[e];
    m.nslot[k]++;
    for (int n = 0; n < m.nc[k]; n++) {
      const int d = elem_dof[(size_t)e * nloc + n];
      FH_REQUIRE(d >= 0 && d < ndof && d < nnode, "%s: element %d, node %d: dof %d outside the system (the classes are numbered one after the other)", who, e, n, d);
      m.adj_ptr[d + 1]++;
    }
  }
  for (int d = 0; d < ndof; d++) m.adj_ptr[d + 1] += m.adj_ptr[d];
  return 0;
}

void* gp_alloc(fh_generic_assembler_t as, size_t bytes) {
  void* d = nullptr;
  bytes = std::max<size_t>(bytes, 8);
  if (hipMalloc(&d, bytes) != hipSuccess) return nullptr;
  as->dv.push_back(d);
  as->device_bytes += (int64_t)bytes;
  as->device_allocations++;
  return d;
}

void gp_free(fh_generic_assembler_t as) {
  if (!as) return;
  if (as->ctx) hipStreamSynchronize(as->ctx->stream);     // no copy or kernel of this object in flight
  for (void* q : as->dv) hipFree(q);
  if (as->d_prog) hipFree(as->d_prog);
  if (as->h_prog) hipHostFree(as->h_prog);
  if (as->prog_ev) hipEventDestroy(as->prog_ev);
  delete as;
}

static void gp_launch_pairs(fh_generic_assembler_t as, int k, const double* sol, double scale, const int* prog, int nprog, const double* pconst) {
  const GenBodyPlan& P = as->poisson;
  gp_dispatch(P, k, [&](auto lanes, auto staged) {
    constexpr int L = decltype(lanes)::value;
    hipLaunchKernelGGL((k_gen_pairs<L, decltype(staged)::value>), dim3(fh_div_up(as->nslot[k], GP_THREADS / L)), dim3(GP_THREADS), P.lds[k], as->ctx->stream,
                       as->nslot[k], as->nc[k], as->ng[k], P.gcm[k], as->dim, as->d_w[k], as->d_phi[k], as->d_dphi[k], as->d_ed[k], as->d_coords, sol, scale, prog, nprog,
                       pconst, as->d_Kb + as->rows.kb_base[k], as->d_Fb + as->rows.row_base[k]);
  });
}

void gp_read_plan(fh_generic_assembler_t as, const GenBodyPlan& plan, int gauss_chunk[3], int lanes[3]) {
  for (int k = 0; k < 3; k++) {
    gauss_chunk[k] = k < as->ns ? plan.gcm[k] : 0;
    if (lanes) lanes[k] = k < as->ns ? plan.lanes[k] : 0;
  }
}

int gp_plan_host(const char* who, fh_ctx_t ctx, const GenMesh& m, int nel, int nnode, fh_mat_t KK, fh_generic_assembler_t* out) {
  const int ndof = KK->m;
  const int ns = m.ns, dim = m.dim, ncmax = m.ncmax;
  const int *ncs = m.nc, *nslot = m.nslot;
  int64_t nrows = 0, nent = 0;
  for (int k = 0; k < ns; k++) {
    nrows += (int64_t)nslot[k] * ncs[k];
    nent += (int64_t)nslot[k] * ncs[k] * ncs[k];
  }
  FH_REQUIRE(nrows < 2147483647ll && nent < (1ll << 40), "%s: too many elements", who);
  int maxrow = 1;
  for (int r = 0; r < ndof; r++) maxrow = std::max(maxrow, KK->h_rowptr[r + 1] - KK->h_rowptr[r]);
  int lpr = ncmax <= 6 ? 4 : ncmax <= 10 ? 8 : 16;
  while (lpr < 64 && (size_t)(GP_THREADS / lpr) * maxrow * sizeof(double) > GP_LDS_BUDGET) lpr *= 2;
  FH_REQUIRE((size_t)(GP_THREADS / lpr) * maxrow * sizeof(double) <= GP_LDS_BUDGET, "%s: a row of %d entries is longer than the row pass holds (%d)", who,
             maxrow, (int)(GP_LDS_BUDGET / sizeof(double) / (GP_THREADS / 64)));

  // ---- host side of the plan ----
  fh_generic_assembler_t as = new fh_generic_assembler_s();
  as->ctx = ctx;
  as->mat_uid = KK->uid;
  as->mat_nnz = KK->nnz;
  as->ndof = ndof, as->nnode = nnode, as->dim = dim, as->ns = ns, as->nel = nel;
  as->lpr = lpr, as->maxrow = maxrow;
  as->row_lds = (size_t)(GP_THREADS / lpr) * maxrow * sizeof(double);
  for (int k = 0; k < 3; k++) {
    as->rows.row_base[k] = INT_MAX;
    as->rows.nc[k] = 0;
    as->rows.kb_base[k] = 0;
  }
  {
    int rb = 0;
    long long kb = 0;
    for (int k = 0; k < ns; k++) {
      as->shapes[k] = m.shapes[k];
      as->nc[k] = ncs[k], as->ng[k] = (int)m.w[k].size(), as->nslot[k] = nslot[k];
      as->rows.row_base[k] = rb, as->rows.nc[k] = ncs[k], as->rows.kb_base[k] = kb;
      rb += nslot[k] * ncs[k];
      kb += (long long)nslot[k] * ncs[k] * ncs[k];
    }
  }
  int lanes[3] = {64, 64, 64};
  for (int k = 0; k < ns; k++) lanes[k] = gp_lanes_per_element(ncs[k], ctx->generic_pack);
  if (const int rc = gp_plan_body(who, as, lanes, gp_elem_doubles, false, false, "", "", as->poisson)) {
    delete as;
    return rc;
  }
  as->nrows = nrows, as->nent = nent;
  // what one assembly cannot avoid moving: element tables, coordinates and state in; values and residual out
  as->algorithmic_bytes = nrows * 4 + (int64_t)nnode * dim * 8 + (int64_t)ndof * 8 + (int64_t)KK->nnz * 8 + (int64_t)ndof * 8;
  *out = as;
  return 0;
}

int gp_plan_work(const char* who, fh_generic_assembler_t as, const GenMesh& m, fh_mat_t KK, unsigned long long* miss) {
  hipStream_t st = as->ctx->stream;
  const int64_t nent = as->nent, nrows = as->nrows;
  bool bad = false;
  auto up = [&](const void* h, size_t bytes) -> void* {
    void* d = bad ? nullptr : gp_alloc(as, bytes);
    if (!d) {
      bad = true;
      return nullptr;
    }
    if (h && bytes && hipMemcpyAsync(d, h, bytes, hipMemcpyHostToDevice, st) != hipSuccess) bad = true;
    return d;
  };
  for (int k = 0; k < as->ns; k++) {
    as->d_w[k] = (double*)up(m.w[k].data(), m.w[k].size() * sizeof(double));
    as->d_phi[k] = (double*)up(m.phi[k].data(), m.phi[k].size() * sizeof(double));
    as->d_dphi[k] = (double*)up(m.dphi[k].data(), m.dphi[k].size() * sizeof(double));
  }
  as->d_Kb = (double*)up(nullptr, (size_t)nent * sizeof(double));
  as->d_Fb = (double*)up(nullptr, (size_t)nrows * sizeof(double));
  as->d_Pos = (int*)up(nullptr, (size_t)nent * sizeof(int));
  as->d_miss = (unsigned long long*)up(nullptr, sizeof(unsigned long long));
  if (!bad) {
    if (hipMalloc((void**)&as->d_prog, GP_PROG_BYTES) == hipSuccess) {
      as->prog_cap = GP_PROG_BYTES;
      as->device_bytes += (int64_t)GP_PROG_BYTES;
      as->device_allocations++;
    } else {
      bad = true;
    }
  }
  if (!bad && (hipHostMalloc((void**)&as->h_prog, GP_PROG_BYTES) != hipSuccess || hipEventCreateWithFlags(&as->prog_ev, hipEventDisableTiming) != hipSuccess)) bad = true;
  if (bad) {
    hipGetLastError();
    gp_free(as);
    fh_set_error("%s: out of device memory (%.2f GB of element rows and positions)", who, (double)nent * 12 / 1e9);
    return 2;
  }
  if (as->ctx->debug_poison) {   // tests: the row pass must read nothing the element pass has not written
    hipMemsetAsync(as->d_Kb, 0xFF, (size_t)nent * sizeof(double), st);
    hipMemsetAsync(as->d_Fb, 0xFF, (size_t)nrows * sizeof(double), st);
  }
  hipMemsetAsync(as->d_miss, 0xFF, sizeof(unsigned long long), st);
  for (int k = 0; k < as->ns; k++) {
    const long long ne = (long long)as->nslot[k] * as->nc[k] * as->nc[k];
    hipLaunchKernelGGL(k_gen_positions, dim3(fh_div_up(ne, 256)), dim3(256), 0, st, ne, as->nc[k], as->d_ed[k], KK->d_rowptr, KK->d_col, as->d_Pos + as->rows.kb_base[k],
                       as->d_miss, (unsigned long long)k << 56);
  }
  *miss = 0;
  if (hipMemcpyAsync(miss, as->d_miss, sizeof(*miss), hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess || hipGetLastError() != hipSuccess) {
    gp_free(as);
    fh_set_error("%s: the position kernel failed", who);
    return 1;
  }
  return 0;
}

extern "C" int fh_generic_assembler_create(fh_ctx_t ctx, int fe, int order, int nel, int nloc, const int* elem_geom, int geom, const int* elem_dof, int nnode,
                                           const double* coords, fh_mat_t KK, fh_generic_assembler_t* out) {
  FH_GUARD_BEGIN
  const char* who = "fh_generic_assembler_create";
  FH_REQUIRE(ctx && elem_dof && coords && KK && out && nel >= 1 && nnode >= 1 && nloc >= 1, "fh_generic_assembler_create: null or empty argument");
  FH_REQUIRE(fe == fhfe::FE_LINEAR || fe == fhfe::FE_SERENDIPITY || fe == fhfe::FE_BIQUADRATIC, "fh_generic_assembler_create: fe must be 0, 1 or 2");
  *out = nullptr;
  // ---- every check first: nothing is allocated on the device before the last of them ----
  const int ndof = KK->m;
  FH_REQUIRE(KK->n == ndof && (int)KK->h_rowptr.size() == ndof + 1, "fh_generic_assembler_create: the matrix is not square with a host row table");
  GenMesh m;
  FH_TRY(gen_mesh(who, fe, order, nel, nloc, elem_geom, geom, elem_dof, nnode, ndof, m));
  const int ns = m.ns, dim = m.dim;
  const int *ncs = m.nc, *nslot = m.nslot;
  fh_generic_assembler_t as = nullptr;
  FH_TRY(gp_plan_host(who, ctx, m, nel, nnode, KK, &as));
  // slot of every element inside its shape, the compact dof tables, the adjacency (ids of element rows, ascending element order per dof)
  std::vector<int> ed[3], slot_elem[3];
  for (int k = 0; k < ns; k++) {
    ed[k].reserve((size_t)nslot[k] * ncs[k]);
    slot_elem[k].reserve(nslot[k]);
  }
  std::vector<int> adj(m.adj_ptr[ndof]), fill(m.adj_ptr.begin(), m.adj_ptr.end() - 1);
  for (int e = 0; e < nel; e++) {
    const int k = m.eshape[e], s = (int)slot_elem[k].size();
    slot_elem[k].push_back(e);
    for (int n = 0; n < ncs[k]; n++) {
      const int d = elem_dof[(size_t)e * nloc + n];
      ed[k].push_back(d);
      adj[fill[d]++] = as->rows.row_base[k] + s * ncs[k] + n;
    }
  }

  // ---- device side: every buffer the object will ever need but a longer source program ----
  hipStream_t st = ctx->stream;
  bool bad = false;
  auto up = [&](const void* h, size_t bytes) -> void* {
    void* d = bad ? nullptr : gp_alloc(as, bytes);
    if (!d) {
      bad = true;
      return nullptr;
    }
    if (h && bytes && hipMemcpyAsync(d, h, bytes, hipMemcpyHostToDevice, st) != hipSuccess) bad = true;
    return d;
  };
  as->d_adj_ptr = (int*)up(m.adj_ptr.data(), m.adj_ptr.size() * sizeof(int));
  as->d_adj = (int*)up(adj.data(), adj.size() * sizeof(int));
  as->d_coords = (double*)up(coords, (size_t)nnode * dim * sizeof(double));
  for (int k = 0; k < ns; k++) as->d_ed[k] = (int*)up(ed[k].data(), ed[k].size() * sizeof(int));
  as->nadj = (int64_t)adj.size();
  if (bad) {
    const int64_t nent = as->nent;
    hipGetLastError();
    gp_free(as);
    fh_set_error("fh_generic_assembler_create: out of device memory (%.2f GB of element rows and positions)", (double)nent * 12 / 1e9);
    return 2;
  }
  unsigned long long miss = 0;
  FH_TRY(gp_plan_work(who, as, m, KK, &miss));
  if (miss != ~0ull) {
    const int k = (int)(miss >> 56);
    const long long idx = (long long)(miss & ((1ull << 56) - 1));
    const int nc = ncs[k], j = (int)(idx % nc), i = (int)((idx / nc) % nc);
    const long long s = idx / ((long long)nc * nc);
    const int e = slot_elem[k][s];
    gp_free(as);
    fh_set_error("fh_generic_assembler_create: element %d: the pair (%d, %d) = dofs (%d, %d) is not in the pattern of the matrix", e, i, j, ed[k][s * nc + i], ed[k][s * nc + j]);
    return 2;
  }
  *out = as;
  return 0;
  FH_GUARD_END("fh_generic_assembler_create")
}

extern "C" int fh_generic_assembler_shapes(fh_generic_assembler_t as, int shapes[3]) {
  FH_REQUIRE(as && shapes, "fh_generic_assembler_shapes: null argument");
  for (int k = 0; k < 3; k++) shapes[k] = k < as->ns ? as->shapes[k] : -1;
  return 0;
}

extern "C" int fh_generic_assembler_plan_sizes(fh_generic_assembler_t as, int* ndof, int64_t* nadj, int64_t* nent) {
  FH_REQUIRE(as, "fh_generic_assembler_plan_sizes: null argument");
  if (ndof) *ndof = as->ndof;
  if (nadj) *nadj = as->nadj;
  if (nent) *nent = as->nent;
  return 0;
}

extern "C" int fh_generic_assembler_get_plan(fh_generic_assembler_t as, int* adj_ptr, int* adj, int* pos) {
  FH_REQUIRE(as, "fh_generic_assembler_get_plan: null argument");
  hipStream_t st = as->ctx->stream;
  if (adj_ptr) FH_CHECK_HIP(hipMemcpyAsync(adj_ptr, as->d_adj_ptr, ((size_t)as->ndof + 1) * sizeof(int), hipMemcpyDeviceToHost, st));
  if (adj && as->nadj) FH_CHECK_HIP(hipMemcpyAsync(adj, as->d_adj, (size_t)as->nadj * sizeof(int), hipMemcpyDeviceToHost, st));
  if (pos && as->nent) FH_CHECK_HIP(hipMemcpyAsync(pos, as->d_Pos, (size_t)as->nent * sizeof(int), hipMemcpyDeviceToHost, st));
  FH_CHECK_HIP(hipStreamSynchronize(st));
  return 0;
}

extern "C" int fh_generic_assembler_set_coords(fh_generic_assembler_t as, int nnode, const double* coords) {
  FH_REQUIRE(as && coords, "fh_generic_assembler_set_coords: null argument");
  FH_REQUIRE(nnode == as->nnode, "fh_generic_assembler_set_coords: %d nodes given, the object was created on %d", nnode, as->nnode);
  FH_CHECK_HIP(hipMemcpyAsync(as->d_coords, coords, (size_t)nnode * as->dim * sizeof(double), hipMemcpyHostToDevice, as->ctx->stream));
  FH_CHECK_HIP(hipStreamSynchronize(as->ctx->stream));     // the caller's array is free again
  return 0;
}

int gp_upload_program(const char* who, fh_generic_assembler_t as, std::vector<int>& code, std::vector<double>& consts) {
  if (consts.empty()) consts.resize(1, 0.0);
  if (as->have_prog && code == as->code && consts == as->consts) return 0;
  const size_t bytes = consts.size() * sizeof(double) + code.size() * sizeof(int);
  hipStream_t st = as->ctx->stream;
  if (bytes > as->prog_cap) {          // a longer program than any before: the one place an assembly allocates (and waits for the kernels that read the old buffer)
    const size_t cap = std::max(bytes, 2 * as->prog_cap);
    char *d = nullptr, *h = nullptr;
    FH_CHECK_HIP(hipStreamSynchronize(st));
    FH_CHECK_HIP(hipMalloc((void**)&d, cap));
    if (hipHostMalloc((void**)&h, cap) != hipSuccess) {
      hipFree(d);
      fh_set_error("%s: out of pinned host memory", who);
      return 2;
    }
    hipFree(as->d_prog);
    hipHostFree(as->h_prog);
    as->device_bytes += (int64_t)cap - (int64_t)as->prog_cap;
    as->device_allocations++;
    as->d_prog = d, as->h_prog = h, as->prog_cap = cap;
    as->prog_copied = false;
  }
  if (as->prog_copied) FH_CHECK_HIP(hipEventSynchronize(as->prog_ev));     // the staging area is read by the last upload only
  memcpy(as->h_prog, consts.data(), consts.size() * sizeof(double));
  memcpy(as->h_prog + consts.size() * sizeof(double), code.data(), code.size() * sizeof(int));
  as->have_prog = false;
  FH_CHECK_HIP(hipMemcpyAsync(as->d_prog, as->h_prog, bytes, hipMemcpyHostToDevice, st));
  FH_CHECK_HIP(hipEventRecord(as->prog_ev, st));
  as->prog_copied = true;
  as->code.swap(code);
  as->consts.swap(consts);
  as->have_prog = true;
  return 0;
}

// the source program into the object's buffer, when it is not the one already there
static int gp_stage_program(fh_generic_assembler_t as, fh_expr_t source) {
  std::vector<int> code;
  std::vector<double> consts;
  FH_TRY(fh_expr_fetch(source, "fh_generic_assembler_assemble: the source expression", 4, code, consts));
  return gp_upload_program("fh_generic_assembler_assemble", as, code, consts);
}

int gp_check_call(const char* who, fh_generic_assembler_t as, fh_vec_t sol, fh_mat_t KK, fh_vec_t RES) {
  FH_REQUIRE(as && RES, "%s: null argument", who);
  FH_REQUIRE(fh_mat_alive(as->mat_uid) != nullptr, "%s: the matrix this object was created on has been destroyed", who);
  FH_REQUIRE(KK != nullptr, "%s: null matrix", who);
  FH_REQUIRE(KK->uid == as->mat_uid && KK->nnz == as->mat_nnz, "%s: not the matrix this object was created on (uid %llu, %d non-zeros; created on uid %llu, %d)", who,
             (unsigned long long)KK->uid, KK->nnz, (unsigned long long)as->mat_uid, as->mat_nnz);
  FH_REQUIRE(RES->n_local >= as->ndof && (!sol || sol->n_local >= as->ndof), "%s: size mismatch", who);
  return 0;
}

void gp_launch_rows(fh_generic_assembler_t as, fh_mat_t KK, fh_vec_t RES) {
  hipLaunchKernelGGL(k_gen_rows, dim3(fh_div_up(as->ndof, GP_THREADS / as->lpr)), dim3(GP_THREADS), as->row_lds, as->ctx->stream, as->ndof, as->lpr, as->maxrow, as->rows,
                     as->d_adj_ptr, as->d_adj, as->d_Kb, as->d_Pos, as->d_Fb, KK->d_rowptr, KK->d_val, RES->d);
}

extern "C" int fh_generic_assembler_assemble(fh_generic_assembler_t as, fh_vec_t sol, fh_expr_t source, double scale, fh_mat_t KK, fh_vec_t RES) {
  FH_GUARD_BEGIN
  FH_TRY(gp_check_call("fh_generic_assembler_assemble", as, sol, KK, RES));
  const int* d_code = nullptr;
  const double* d_k = nullptr;
  int ncode = 0;
  if (source) {
    FH_TRY(gp_stage_program(as, source));
    d_k = (const double*)as->d_prog;
    d_code = (const int*)(as->d_prog + as->consts.size() * sizeof(double));
    ncode = (int)as->code.size();
  }
  for (int k = 0; k < as->ns; k++)
    if (as->nslot[k]) gp_launch_pairs(as, k, sol ? sol->d : nullptr, scale, d_code, ncode, d_k);
  gp_launch_rows(as, KK, RES);
  const bool ok = hipGetLastError() == hipSuccess;
  fh_mat_values_written(KK);
  FH_REQUIRE(ok, "fh_generic_assembler_assemble: launch failed");
  return 0;
  FH_GUARD_END("fh_generic_assembler_assemble")
}

extern "C" int fh_generic_assembler_info(fh_generic_assembler_t as, int elems_per_workgroup[3], int64_t* device_bytes, int64_t* algorithmic_bytes,
                                         int64_t* device_allocations) {
  FH_REQUIRE(as, "fh_generic_assembler_info: null argument");
  if (elems_per_workgroup)
    for (int k = 0; k < 3; k++) elems_per_workgroup[k] = k < as->ns ? GP_THREADS / as->poisson.lanes[k] : 0;
  if (device_bytes) *device_bytes = as->device_bytes;
  if (algorithmic_bytes) *algorithmic_bytes = as->algorithmic_bytes;
  if (device_allocations) *device_allocations = as->device_allocations;
  return 0;
}

extern "C" int fh_generic_assembler_destroy(fh_generic_assembler_t as) {
  gp_free(as);
  return 0;
}

// ------------------------------------------------------------------------------------------------------------------
// The one-shot calls.  Two passes: one WAVE per element forms the element matrix with gen_element_pass (node stride GEN_NC, Gauss chunk GEN_GC, static LDS)
// into a buffer, with the place of every entry in the matrix beside it; one thread per ROW then adds the rows of its node's elements in ascending element order
// (first version: the row thread formed them itself -- 80 ms per call on 54 k TET15 elements, host preparation included; 53 760 TET15 elements: 26 + 8.5 ms ->
// 4.7 + 0.8 ms, profiles/r06_shipped_inputs_kernel_summary.md).  Repeated assemblies -- the application's linear iterations -- go through the resident object.
// ------------------------------------------------------------------------------------------------------------------
struct GenTab {              // the tables of one element shape: a mesh of mixed shapes (hexahedra, tetrahedra, prisms; quadrilaterals, triangles) names one per element
  int nc, ng;
  const double *w, *phi, *dphi;
};
struct GenTabs {
  GenTab t[3];
};
// Row i of the element matrix goes to Kb[(e * ncmax + i) * ncmax + j], its residual entry to Fb[e * ncmax + i].
__global__ __launch_bounds__(64) void k_poisson_pairs_generic(int nel, int ncmax, int dim, GenTabs tabs, const unsigned char* __restrict__ etab, int nloc,
                                                              const int* __restrict__ elem_dof, const double* __restrict__ coords, const double* __restrict__ sol,
                                                              double scale, const int* __restrict__ prog, int nprog, const double* __restrict__ pconst,
                                                              const int* __restrict__ rowptr, const int* __restrict__ col, double* __restrict__ Kb,
                                                              int* __restrict__ Pos, double* __restrict__ Fb) {
  __shared__ double S[gp_elem_doubles(GEN_NC, GEN_GC)];
  __shared__ int DOF[GEN_NC];
  const int e = blockIdx.x, lane = threadIdx.x;
  const GenTab& T = tabs.t[etab ? etab[e] : 0];
  const int nc = T.nc;
  const int* dof_row = elem_dof + (size_t)e * nloc;
  if (lane < nc) DOF[lane] = dof_row[lane];
  constexpr int NPL = gp_pairs_per_lane(64);
  int pi[NPL], pj[NPL];
  double acc[NPL], F;
  gen_element_pass<64, NPL>(true, lane, nc, T.ng, GEN_GC, GEN_NC, dim, T.w, T.phi, T.dphi, dof_row, coords, sol, scale, prog, nprog, pconst, S, pi, pj, acc, F);
  // the entry's place in the matrix beside its value (-1: the pattern does not hold it), so that the row pass adds without searching
  double* out = Kb + (size_t)e * ncmax * ncmax;
  int* pos = Pos + (size_t)e * ncmax * ncmax;
  auto place = [&](int i, int j) {
    const int r = DOF[i], c = DOF[j];
    int at = -1;
    for (int k = rowptr[r], re = rowptr[r + 1]; k < re; k++)
      if (col[k] == c) {
        at = k;
        break;
      }
    return at;
  };
#pragma unroll
  for (int k = 0; k < NPL; k++)
    if (pi[k] >= 0) {
      out[(size_t)pi[k] * ncmax + pj[k]] = acc[k];
      pos[(size_t)pi[k] * ncmax + pj[k]] = place(pi[k], pj[k]);
      if (pi[k] != pj[k]) {
        out[(size_t)pj[k] * ncmax + pi[k]] = acc[k];
        pos[(size_t)pj[k] * ncmax + pi[k]] = place(pj[k], pi[k]);
      }
    }
  if (lane < nc) Fb[(size_t)e * ncmax + lane] = F;
}

// Second pass: one thread per row, its (element, local row) pairs in ascending element order -- the order of the reference's element loop --, every entry added
// at the place the first pass found for it.
__global__ __launch_bounds__(64) void k_poisson_rows_generic(int ndof, int ncmax, GenTabs tabs, const unsigned char* __restrict__ etab,
                                                             const int* __restrict__ adj_ptr, const int* __restrict__ adj, const double* __restrict__ Kb,
                                                             const int* __restrict__ Pos, const double* __restrict__ Fb, const int* __restrict__ rowptr,
                                                             double* __restrict__ val, double* __restrict__ res) {
  const int r = blockIdx.x * 64 + threadIdx.x;
  if (r >= ndof) return;
  const int rs = rowptr[r], re = rowptr[r + 1];
  for (int k = rs; k < re; k++) val[k] = 0.0;
  double racc = 0.0;
  for (int a = adj_ptr[r]; a < adj_ptr[r + 1]; a++) {
    const int e = adj[a] / GEN_NC, i = adj[a] % GEN_NC;
    const int nc = tabs.t[etab ? etab[e] : 0].nc;
    const size_t pr = (size_t)e * ncmax + i;
    racc += Fb[pr];
    const double* B = Kb + pr * ncmax;
    const int* at = Pos + pr * ncmax;
    for (int j = 0; j < nc; j++)
      if (at[j] >= 0) val[at[j]] += B[j];
  }
  res[r] = racc;
}

// elem_geom as gen_mesh takes it.  Every check comes before the first allocation on the device.
static int poisson_rows_impl(const char* who, fh_ctx_t ctx, const int* elem_geom, int geom, int fe, int order, int nel, int nloc, const int* elem_dof, int nnode,
                             const double* coords, fh_vec_t sol, fh_expr_t source, double scale, fh_mat_t KK, fh_vec_t RES) {
  FH_REQUIRE(ctx && elem_dof && coords && KK && RES && nel >= 1 && nnode >= 1, "%s: null or empty argument", who);
  FH_REQUIRE(fe == fhfe::FE_LINEAR || fe == fhfe::FE_SERENDIPITY || fe == fhfe::FE_BIQUADRATIC, "%s: fe must be 0, 1 or 2", who);
  const int ndof = KK->m;
  FH_REQUIRE(KK->n == ndof && RES->n_local >= ndof && (!sol || sol->n_local >= ndof), "%s: size mismatch", who);
  FH_REQUIRE((int64_t)nel * GEN_NC < 2147483647ll, "%s: too many elements", who);
  GenMesh m;
  FH_TRY(gen_mesh(who, fe, order, nel, nloc, elem_geom, geom, elem_dof, nnode, ndof, m));
  const int ncmax = m.ncmax;
  std::vector<int> adj(m.adj_ptr[ndof]), fill(m.adj_ptr.begin(), m.adj_ptr.end() - 1);
  for (int e = 0; e < nel; e++)                         // ascending element order per dof; rows padded to GEN_NC
    for (int n = 0; n < m.nc[m.eshape[e]]; n++) adj[fill[elem_dof[(size_t)e * nloc + n]]++] = e * GEN_NC + n;
  std::vector<int> code;
  std::vector<double> consts;
  if (source) {
    char subject[96];
    snprintf(subject, sizeof subject, "%s: the source expression", who);
    FH_TRY(fh_expr_fetch(source, subject, 4, code, consts));
    if (consts.empty()) consts.resize(1);
  }
  hipStream_t st = ctx->stream;
  std::vector<void*> dv;
  bool oom = false;
  auto up = [&](const void* h, size_t bytes) -> void* {
    void* d = nullptr;
    if (hipMalloc(&d, std::max<size_t>(bytes, 8)) != hipSuccess) {
      oom = true;
      return nullptr;
    }
    dv.push_back(d);
    if (bytes && h) hipMemcpyAsync(d, h, bytes, hipMemcpyHostToDevice, st);
    return d;
  };
  int* d_ptr = (int*)up(m.adj_ptr.data(), m.adj_ptr.size() * sizeof(int));
  int* d_adj = (int*)up(adj.data(), adj.size() * sizeof(int));
  int* d_ed = (int*)up(elem_dof, (size_t)nel * nloc * sizeof(int));
  double* d_x = (double*)up(coords, (size_t)nnode * m.dim * sizeof(double));
  GenTabs tabs;
  for (int k = 0; k < 3; k++) tabs.t[k] = GenTab{0, 0, nullptr, nullptr, nullptr};
  for (int k = 0; k < m.ns; k++)
    tabs.t[k] = GenTab{m.nc[k], (int)m.w[k].size(), (const double*)up(m.w[k].data(), m.w[k].size() * sizeof(double)),
                       (const double*)up(m.phi[k].data(), m.phi[k].size() * sizeof(double)), (const double*)up(m.dphi[k].data(), m.dphi[k].size() * sizeof(double))};
  unsigned char* d_etab = elem_geom ? (unsigned char*)up(m.eshape.data(), m.eshape.size()) : nullptr;
  int* d_code = source ? (int*)up(code.data(), code.size() * sizeof(int)) : nullptr;
  double* d_k = source ? (double*)up(consts.data(), consts.size() * sizeof(double)) : nullptr;
  double* d_Kb = (double*)up(nullptr, (size_t)nel * ncmax * ncmax * sizeof(double));      // element rows between the two passes
  double* d_Fb = (double*)up(nullptr, (size_t)nel * ncmax * sizeof(double));
  int* d_Pos = (int*)up(nullptr, (size_t)nel * ncmax * ncmax * sizeof(int));
  int rc = 0;
  if (oom) {
    fh_set_error("%s: out of device memory", who);
    rc = 2;
  } else {
    hipLaunchKernelGGL(k_poisson_pairs_generic, dim3(nel), dim3(64), 0, st, nel, ncmax, m.dim, tabs, d_etab, nloc, d_ed, d_x,
                       sol ? sol->d : nullptr, scale, d_code, (int)code.size(), d_k, KK->d_rowptr, KK->d_col, d_Kb, d_Pos, d_Fb);
    hipLaunchKernelGGL(k_poisson_rows_generic, dim3(fh_div_up(ndof, 64)), dim3(64), 0, st, ndof, ncmax, tabs, d_etab, d_ptr, d_adj, d_Kb, d_Pos, d_Fb, KK->d_rowptr,
                       KK->d_val, RES->d);
    if (hipGetLastError() != hipSuccess) {
      fh_set_error("%s: launch failed", who);
      rc = 2;
    }
    fh_mat_values_written(KK);
  }
  hipStreamSynchronize(st);
  for (void* q : dv) hipFree(q);
  return rc;
}

extern "C" int fh_assemble_poisson_rows(fh_ctx_t ctx, int geom, int fe, int order, int nel, int nloc, const int* elem_dof, int nnode, const double* coords,
                                        fh_vec_t sol, fh_expr_t source, double scale, fh_mat_t KK, fh_vec_t RES) {
  FH_GUARD_BEGIN
  return poisson_rows_impl("fh_assemble_poisson_rows", ctx, nullptr, geom, fe, order, nel, nloc, elem_dof, nnode, coords, sol, source, scale, KK, RES);
  FH_GUARD_END("fh_assemble_poisson_rows")
}

// The same on a mesh of MIXED shapes (cube_all_shapes*.neu of applications/001_Poisson: hexahedra, tetrahedra and prisms in one file): elem_geom[nel] names the
// shape of every element (at most three different ones, of one dimension); rows of elem_dof padded to nloc.  The entries of a row are summed in ascending element
// order whatever the shapes, as the reference's element loop does.
extern "C" int fh_assemble_poisson_mixed(fh_ctx_t ctx, int fe, int order, int nel, int nloc, const int* elem_geom, const int* elem_dof, int nnode, const double* coords,
                                         fh_vec_t sol, fh_expr_t source, double scale, fh_mat_t KK, fh_vec_t RES) {
  FH_GUARD_BEGIN
  FH_REQUIRE(elem_geom, "fh_assemble_poisson_mixed: null or empty argument");
  return poisson_rows_impl("fh_assemble_poisson_mixed", ctx, elem_geom, 0, fe, order, nel, nloc, elem_dof, nnode, coords, sol, source, scale, KK, RES);
  FH_GUARD_END("fh_assemble_poisson_mixed")
}
