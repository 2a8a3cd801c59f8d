// Hanging-node constraints of a device-resident element mesh of any mix of the five shapes: the search of fh_elemconstraints.cpp (Mesh::GetAMRRestrictionAndAMRSolidMark,
// Mesh.cpp:1354-1830) with the interface faces, the candidate search and the inverse maps on the device; the entries it finds are downloaded and resolved into
// rows by the code every search shares (fh_amr_resolve).
//   1. interface faces: every (element, face) inserts the key of its vertices into an open-addressing table of the refinement's kind (an edge: two ids; a
//      triangle: the slot of the edge of its two smallest vertices and the third; a quadrilateral: its smallest vertex and the one diagonal to it) and counts
//      itself there; a second pass marks the faces with flag -1 whose key was counted once, ORs the family's nodes of those faces into a mask per element and
//      the element's level into a word per node.
//   2. per level: the interface elements in element order and the duplicate-free, ascending list of the interface nodes with their coordinates (flag, scan, compact).
//   3. for every pair of levels Lc < Lf, in that order: one wave per coarse interface element streams the finer level's node list through LDS tiles a workgroup of
//      four waves shares and keeps the nodes inside its padded box and hull sphere that are no dofs of its own: count, scan, fill (a ballot orders a tile's hits).
//      Then one wave per element again, a lane per candidate: the Newton inverse of the biquadratic map from the nearest node's reference point, the inside test,
//      the family's functions there (fh_fe_basis.h: the host's code, compiled for the device); count of the weights kept, scan, and a last pass writes the entries.
//      Their order -- (pair of levels, coarse element, node id, local node) -- is that of the host search whatever the threads do: no value is ever combined by an
//      atomic, and a later write of a (master, hanging) pair wins by its place in that order.  Bitwise repeatable.
// Slot numbers of the tables depend on the race; nothing that leaves the kernels does.
#include "fh_elemmesh.h"
#include "fh_elemconstraints.h"
#include "fh_fe.h"
#include <chrono>

namespace {
constexpr int EC_TILE = 256;      // nodes of one LDS tile, one per thread of the workgroup
struct EcFamily {                 // per shape code, for one family: its nodes on every face as a mask of local nodes, and its width
  unsigned face[EM_G][EM_F];
  int nc[EM_G];
};
double ec_ms(std::chrono::steady_clock::time_point a) { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - a).count(); }
}   // namespace

// ---- 1. interface faces -----------------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_ec_face_count(const EmTab* __restrict__ T, int nel, const int* __restrict__ geom, const int* __restrict__ ed, EmHash E, EmHash TR,
                                                       EmHash Q, int* __restrict__ fslot, int* __restrict__ cnt) {
  const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= (size_t)nel * EM_F) return;
  const int e = (int)(t / EM_F), f = (int)(t % EM_F), g = geom[e];
  if (f >= T->nf[g]) {
    fslot[t] = -1;
    return;
  }
  const int* fd = ed + (size_t)e * EM_W;
  const int nvf = T->nvf[g][f];
  int slot;
  if (nvf == 2) {
    int a = fd[T->face_v[g][f][0]], b = fd[T->face_v[g][f][1]];
    if (a > b) { const int c = a; a = b; b = c; }
    slot = E.id0 + em_insert(E.keys, E.mask, E.shift, em_pair(a, b));
  } else if (nvf == 3) {
    int a = fd[T->face_v[g][f][0]], b = fd[T->face_v[g][f][1]], c = fd[T->face_v[g][f][2]], s;
    if (a > b) { s = a; a = b; b = s; }
    if (b > c) { s = b; b = c; c = s; }
    if (a > b) { s = a; a = b; b = s; }
    const int se = em_insert(E.keys, E.mask, E.shift, em_pair(a, b));
    slot = TR.id0 + em_insert(TR.keys, TR.mask, TR.shift, em_pair(se, c));
  } else {
    int v[4], km = 0;
    for (int k = 0; k < 4; k++) v[k] = fd[T->face_v[g][f][k]];
    for (int k = 1; k < 4; k++)
      if (v[k] < v[km]) km = k;
    slot = Q.id0 + em_insert(Q.keys, Q.mask, Q.shift, em_pair(v[km], v[T->face_diag[g][f][km]]));
  }
  fslot[t] = slot;
  atomicAdd(&cnt[slot], 1);
}

// one thread per element: the mask of its interface local nodes; its level into the word of each of them; *any: an interface face exists
__global__ __launch_bounds__(256) void k_ec_mark(const EmTab* __restrict__ T, EcFamily K, int nel, const int* __restrict__ geom, const int* __restrict__ ed,
                                                 const int* __restrict__ ff, const int* __restrict__ lev, const int* __restrict__ fslot, const int* __restrict__ cnt,
                                                 unsigned* __restrict__ emask, unsigned* __restrict__ nodebits, int* __restrict__ any) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= nel) return;
  const int g = geom[e];
  unsigned m = 0;
  bool iface = false;
  for (int f = 0; f < T->nf[g]; f++) {
    const int s = fslot[(size_t)e * EM_F + f];
    if (s >= 0 && ff[(size_t)e * EM_F + f] == -1 && cnt[s] == 1) {
      m |= K.face[g][f];
      iface = true;
    }
  }
  emask[e] = m;
  if (iface) *any = 1;            // (every writer stores the same 1)
  const unsigned bit = 1u << lev[e];
  for (int n = 0; n < T->nl[g]; n++)
    if ((m >> n) & 1u) atomicOr(&nodebits[ed[(size_t)e * EM_W + n]], bit);
}

// ---- 2. the lists of one level ------------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_ec_level_flags(int nel, int nnode, int L, const unsigned* __restrict__ emask, const int* __restrict__ lev,
                                                        const unsigned* __restrict__ nodebits, int* __restrict__ eflag, int* __restrict__ nflag) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < nel) eflag[i] = (emask[i] != 0 && lev[i] == L) ? 1 : 0;
  if (i < nnode) nflag[i] = (int)((nodebits[i] >> L) & 1u);
}
__global__ __launch_bounds__(256) void k_ec_compact(int nel, int nnode, int dim, const int* __restrict__ epos, const int* __restrict__ npos, const double* __restrict__ x,
                                                    int nie, int* __restrict__ ielist, int nn, int* __restrict__ nid, double* __restrict__ nx) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < nel) {
    const int p = epos[i];
    if (epos[i + 1] != p && p < nie) ielist[p] = i;
  }
  if (i < nnode) {
    const int p = npos[i];
    if (npos[i + 1] != p && p < nn) {
      nid[p] = i;
      for (int d = 0; d < dim; d++) nx[(size_t)p * dim + d] = x[(size_t)i * dim + d];
    }
  }
}

// ---- 3. the search of one pair of levels ----------------------------------------------------------------------------------------------------------------------------
// a wave per coarse interface element q, four to a workgroup; the node list of the finer level in tiles of EC_TILE through LDS.  !FILL: ccount[q] = its
// candidates; FILL: they are written from coff[q] on, in list order (ascending node id)
template <bool FILL>
__global__ __launch_bounds__(256) void k_ec_candidates(const EmTab* __restrict__ T, EcFamily K, int dim, int nie, const int* __restrict__ ielist, const int* __restrict__ geom,
                                                       const int* __restrict__ ed, const double* __restrict__ x, int nn, const int* __restrict__ nid,
                                                       const double* __restrict__ nx, int* __restrict__ ccount, const int* __restrict__ coff, int ncand,
                                                       int* __restrict__ cand_node, int* __restrict__ cand_q) {
  __shared__ double s_x[EC_TILE * 3];
  __shared__ int s_id[EC_TILE];
  __shared__ double s_xv[4][EM_W * 3];
  __shared__ int s_ed[4][EM_W];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, q = blockIdx.x * 4 + wave;
  const bool active = q < nie;
  int nl = 0, nc = 0;
  if (active) {
    const int e = ielist[q], g = geom[e];
    nl = T->nl[g];
    nc = K.nc[g];
    if (lane < nl) {
      const int id = ed[(size_t)e * EM_W + lane];
      s_ed[wave][lane] = id;
      for (int d = 0; d < dim; d++) s_xv[wave][lane * dim + d] = x[(size_t)id * dim + d];
    }
  }
  __syncthreads();
  double box[6] = {0, 0, 0, 0, 0, 0}, xc[3] = {0, 0, 0}, r2 = 0.0;
  if (active) fh_amr_hull(dim, nl, s_xv[wave], box, xc, &r2);
  const int base = (FILL && active) ? coff[q] : 0;
  int cnt = 0;
  for (int t0 = 0; t0 < nn; t0 += EC_TILE) {
    __syncthreads();              // the tile before has been read by every wave
    const int i = t0 + (int)threadIdx.x;
    if (i < nn) {
      s_id[threadIdx.x] = nid[i];
      for (int d = 0; d < dim; d++) s_x[threadIdx.x * dim + d] = nx[(size_t)i * dim + d];
    }
    __syncthreads();
    if (!active) continue;
    for (int r = 0; r < EC_TILE / 64; r++) {
      const int k = r * 64 + lane;
      bool hit = false;
      int id = -1;
      if (t0 + k < nn) {
        hit = fh_amr_in_hull(dim, box, xc, r2, &s_x[k * dim]);
        id = s_id[k];
        if (hit)
          for (int j = 0; j < nc; j++) hit = hit && s_ed[wave][j] != id;
      }
      const unsigned long long m = __ballot(hit);
      if (FILL && hit) {
        const int pos = base + cnt + __popcll(m & ((1ull << lane) - 1ull));
        if (pos < ncand) {
          cand_node[pos] = id;
          cand_q[pos] = q;
        }
      }
      cnt += __popcll(m);
    }
  }
  if (!FILL && active && lane == 0) ccount[q] = cnt;
}

// a wave per coarse interface element, a lane per candidate: cphi[c][n] = the family's function of interface local node n at the candidate's reference point
// where it is kept (|v| >= 1e-10), 0.0 anywhere else; tcnt[c] = how many are kept (0: outside the element, or the map did not invert)
__global__ __launch_bounds__(256) void k_ec_newton(const EmTab* __restrict__ T, int dim, int fe, int nie, const int* __restrict__ ielist, const int* __restrict__ geom,
                                                   const int* __restrict__ ed, const double* __restrict__ x, const unsigned* __restrict__ emask,
                                                   const int* __restrict__ coff, int ncand, const int* __restrict__ cand_node, double* __restrict__ cphi,
                                                   int* __restrict__ tcnt) {
  __shared__ double s_xv[4][EM_W * 3];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, q = blockIdx.x * 4 + wave;
  const bool active = q < nie;
  int g = 0, nl = 0, e = 0;
  if (active) {
    e = ielist[q];
    g = geom[e];
    nl = T->nl[g];
    if (lane < nl) {
      const int id = ed[(size_t)e * EM_W + lane];
      for (int d = 0; d < dim; d++) s_xv[wave][lane * dim + d] = x[(size_t)id * dim + d];
    }
  }
  __syncthreads();
  if (!active) return;
  const unsigned mask = emask[e];
  const int c1 = min(coff[q + 1], ncand);
  for (int c = coff[q] + lane; c < c1; c += 64) {
    const int id = cand_node[c];
    double xp[3] = {0, 0, 0}, xi[3] = {0, 0, 0}, phi[EM_W];
    for (int d = 0; d < dim; d++) xp[d] = x[(size_t)id * dim + d];
    fh_amr_closest_node(g, dim, nl, s_xv[wave], xp, xi);
    const bool ok = fh_amr_inverse_map(g, dim, nl, s_xv[wave], xp, xi) && fh_amr_inside(g, xi, 1e-4);
    for (int n = 0; n < EM_W; n++) phi[n] = 0.0;
    if (ok) fhfe::hd::eval_basis(g, fe, xi, phi, nullptr);
    int kept = 0;
    for (int n = 0; n < EM_W; n++) {
      const bool keep = ok && ((mask >> n) & 1u) && !(fabs(phi[n]) < 1.0e-10);
      cphi[(size_t)c * EM_W + n] = keep ? phi[n] : 0.0;
      kept += keep ? 1 : 0;
    }
    tcnt[c] = kept;
  }
}

// one thread per candidate: its entries (master, hanging, value) from toff[c] on, in local-node order
__global__ __launch_bounds__(256) void k_ec_emit(int ncand, const int* __restrict__ ielist, const int* __restrict__ ed, const int* __restrict__ cand_node,
                                                 const int* __restrict__ cand_q, const double* __restrict__ cphi, const int* __restrict__ toff, int ntrip,
                                                 int* __restrict__ tm, int* __restrict__ th, double* __restrict__ tv) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= ncand) return;
  int off = toff[c];
  const int end = min(toff[c + 1], ntrip);
  const int e = ielist[cand_q[c]], id = cand_node[c];
  for (int n = 0; n < EM_W && off < end; n++) {
    const double v = cphi[(size_t)c * EM_W + n];
    if (v != 0.0) {
      tm[off] = ed[(size_t)e * EM_W + n];
      th[off] = id;
      tv[off] = v;
      off++;
    }
  }
}

// ---- host side --------------------------------------------------------------------------------------------------------------------------------------------------------
static int ec_family(int fe, EcFamily& K) {
  memset(&K, 0, sizeof(K));
  for (int g = 0; g < EM_G; g++) {
    if (g == fhfe::GEOM_LINE) continue;
    K.nc[g] = fhfe::ndofs_of(g, fe);
    for (int f = 0; f < fhfe::nfaces_of(g); f++) {
      int fn[9];
      const int n = fhfe::face_nodes(g, fe, f, fn);
      for (int k = 0; k < n; k++)
        if (fn[k] >= 0 && fn[k] < K.nc[g]) K.face[g][f] |= 1u << fn[k];
    }
  }
  return 0;
}

// the entries of the search in the order of fh_elem_amr_search_host; *unmarked: the mesh has interface faces (asked for by a mesh whose levels nobody gave)
static int ec_search_device(fh_elem_mesh_t M, int fe, bool only_probe, bool* has_iface, std::vector<AmrTriple>& writes, double* ms_download) {
  const char* who = "fh_elem_mesh_amr_constraints";
  fh_ctx_t ctx = M->ctx;
  hipStream_t st = ctx->stream;
  const int dim = M->dim, nel = M->nel, nnode = M->nnode, maxlev = M->level;
  writes.clear();
  *has_iface = false;
  if (!nel) return 0;
  FH_REQUIRE(maxlev < 31, "%s: %d levels in one mesh: at most 31 are served", who, maxlev + 1);
  FH_REQUIRE((int64_t)nel * EM_W < ((int64_t)1 << 31), "%s: %d elements do not fit 32-bit offsets", who, nel);
  EcFamily K;
  ec_family(fe, K);
  // the tables: every key fits with load <= 1/2 even if no face were shared
  int64_t nE = 0, nT = 0, nQ = 0;
  for (int g = 0; g < EM_G; g++) {
    if (!M->count[g]) continue;
    for (int f = 0; f < fhfe::nfaces_of(g); f++) {
      int fv[9];
      const int nvf = fhfe::face_nodes(g, fhfe::FE_LINEAR, f, fv);
      (nvf == 2 ? nE : nvf == 3 ? nT : nQ) += M->count[g];
    }
  }
  nE += nT;                       // a triangle looks up the edge of its two smallest vertices
  auto log2cap = [](int64_t nkeys) {
    int l = 6;
    while (((int64_t)1 << l) < 2 * nkeys) l++;
    return l;
  };
  const int lE = log2cap(nE), lT = log2cap(nT), lQ = log2cap(nQ);
  const size_t capE = (size_t)1 << lE, capT = (size_t)1 << lT, capQ = (size_t)1 << lQ, ncnt = capE + capT + capQ;
  FH_REQUIRE(ncnt < ((size_t)1 << 31), "%s: the face tables of %d elements do not fit 32-bit slots", who, nel);
  EmScratch B(who);
  unsigned long long *d_kE, *d_kT, *d_kQ;
  int *d_cnt, *d_fslot, *d_any, *d_eflag, *d_nflag, *d_bsum;
  unsigned *d_emask, *d_bits;
  const size_t nmax = (size_t)std::max(nel, nnode);
  if (B.get(&d_kE, capE) || B.get(&d_kT, capT) || B.get(&d_kQ, capQ) || B.get(&d_cnt, ncnt) || B.get(&d_fslot, (size_t)nel * EM_F) || B.get(&d_any, 2) ||
      B.get(&d_emask, (size_t)nel) || B.get(&d_bits, (size_t)nnode) || B.get(&d_eflag, (size_t)nel + 1) || B.get(&d_nflag, (size_t)nnode + 1) ||
      B.get(&d_bsum, nmax / FH_SCAN_BLOCK + 2))
    return 2;
  const bool poison = ctx->debug_poison != 0;
  if (poison) {                   // every entry is written before it is read
    FH_CHECK_HIP(hipMemsetAsync(d_fslot, 0xFF, (size_t)nel * EM_F * sizeof(int), st));
    FH_CHECK_HIP(hipMemsetAsync(d_emask, 0xFF, (size_t)nel * sizeof(unsigned), st));
    FH_CHECK_HIP(hipMemsetAsync(d_eflag, 0xFF, ((size_t)nel + 1) * sizeof(int), st));
    FH_CHECK_HIP(hipMemsetAsync(d_nflag, 0xFF, ((size_t)nnode + 1) * sizeof(int), st));
  }
  FH_CHECK_HIP(hipMemsetAsync(d_kE, 0xFF, capE * sizeof(unsigned long long), st));
  FH_CHECK_HIP(hipMemsetAsync(d_kT, 0xFF, capT * sizeof(unsigned long long), st));
  FH_CHECK_HIP(hipMemsetAsync(d_kQ, 0xFF, capQ * sizeof(unsigned long long), st));
  FH_CHECK_HIP(hipMemsetAsync(d_cnt, 0, ncnt * sizeof(int), st));
  FH_CHECK_HIP(hipMemsetAsync(d_bits, 0, std::max<size_t>(nnode, 2) * sizeof(unsigned), st));
  FH_CHECK_HIP(hipMemsetAsync(d_any, 0, 2 * sizeof(int), st));
  const EmTab* dT = M->tab->d_tab;
  EmHash hE{d_kE, (unsigned)(capE - 1), 64 - lE, 0}, hT{d_kT, (unsigned)(capT - 1), 64 - lT, (int)capE}, hQ{d_kQ, (unsigned)(capQ - 1), 64 - lQ, (int)(capE + capT)};
  hipLaunchKernelGGL(k_ec_face_count, dim3((unsigned)(((size_t)nel * EM_F + 255) / 256)), dim3(256), 0, st, dT, nel, M->d_geom, M->d_ed, hE, hT, hQ, d_fslot, d_cnt);
  hipLaunchKernelGGL(k_ec_mark, dim3(fh_div_up(nel, 256)), dim3(256), 0, st, dT, K, nel, M->d_geom, M->d_ed, M->d_ff, M->d_lev, d_fslot, d_cnt, d_emask, d_bits, d_any);
  FH_CHECK_HIP(hipGetLastError());
  int any = 0;
  FH_CHECK_HIP(hipMemcpyAsync(&any, d_any, sizeof(int), hipMemcpyDeviceToHost, st));
  FH_CHECK_HIP(hipStreamSynchronize(st));
  *has_iface = any != 0;
  if (!any || only_probe) return 0;
  // the lists of every level
  struct Level {
    int nie = 0, nn = 0;
    int *ielist = nullptr, *nid = nullptr;
    double* nx = nullptr;
  };
  std::vector<Level> lv(maxlev + 1);
  const int gmax = fh_div_up((int64_t)nmax, 256);
  int most_ie = 0;
  for (int L = 0; L <= maxlev; L++) {
    hipLaunchKernelGGL(k_ec_level_flags, dim3(gmax), dim3(256), 0, st, nel, nnode, L, d_emask, M->d_lev, d_bits, d_eflag, d_nflag);
    FH_CHECK_HIP(hipGetLastError());
    FH_TRY(fh_device_exclusive_scan(st, d_eflag, d_eflag, nel, d_bsum));
    FH_TRY(fh_device_exclusive_scan(st, d_nflag, d_nflag, nnode, d_bsum));
    FH_CHECK_HIP(hipMemcpyAsync(&lv[L].nie, d_eflag + nel, sizeof(int), hipMemcpyDeviceToHost, st));
    FH_CHECK_HIP(hipMemcpyAsync(&lv[L].nn, d_nflag + nnode, sizeof(int), hipMemcpyDeviceToHost, st));
    FH_CHECK_HIP(hipStreamSynchronize(st));
    FH_REQUIRE(lv[L].nie >= 0 && lv[L].nie <= nel && lv[L].nn >= 0 && lv[L].nn <= nnode, "%s: level %d: %d interface elements and %d interface nodes of %d and %d", who, L,
               lv[L].nie, lv[L].nn, nel, nnode);
    if (!lv[L].nie) continue;
    if (B.get(&lv[L].ielist, (size_t)lv[L].nie) || B.get(&lv[L].nid, (size_t)lv[L].nn) || B.get(&lv[L].nx, (size_t)lv[L].nn * dim)) return 2;
    if (poison) {
      FH_CHECK_HIP(hipMemsetAsync(lv[L].ielist, 0xFF, std::max<size_t>(lv[L].nie, 2) * sizeof(int), st));
      FH_CHECK_HIP(hipMemsetAsync(lv[L].nid, 0xFF, std::max<size_t>(lv[L].nn, 2) * sizeof(int), st));
      FH_CHECK_HIP(hipMemsetAsync(lv[L].nx, 0xFF, std::max<size_t>((size_t)lv[L].nn * dim, 2) * sizeof(double), st));
    }
    hipLaunchKernelGGL(k_ec_compact, dim3(gmax), dim3(256), 0, st, nel, nnode, dim, d_eflag, d_nflag, M->d_x, lv[L].nie, lv[L].ielist, lv[L].nn, lv[L].nid, lv[L].nx);
    FH_CHECK_HIP(hipGetLastError());
    most_ie = std::max(most_ie, lv[L].nie);
  }
  int *d_ccount, *d_coff;
  if (B.get(&d_ccount, (size_t)most_ie + 1) || B.get(&d_coff, (size_t)most_ie + 1)) return 2;
  std::vector<int> hm, hh;
  std::vector<double> hv;
  for (int Lc = 0; Lc <= maxlev; Lc++) {
    if (!lv[Lc].nie) continue;
    for (int Lf = Lc + 1; Lf <= maxlev; Lf++) {
      if (!lv[Lf].nie || !lv[Lf].nn) continue;
      const Level &C = lv[Lc], &Fn = lv[Lf];
      const int gq = fh_div_up(C.nie, 4);
      if (poison) FH_CHECK_HIP(hipMemsetAsync(d_ccount, 0xFF, ((size_t)C.nie + 1) * sizeof(int), st));
      hipLaunchKernelGGL(k_ec_candidates<false>, dim3(gq), dim3(256), 0, st, dT, K, dim, C.nie, C.ielist, M->d_geom, M->d_ed, M->d_x, Fn.nn, Fn.nid, Fn.nx, d_ccount, nullptr, 0,
                         nullptr, nullptr);
      FH_CHECK_HIP(hipGetLastError());
      FH_TRY(fh_device_exclusive_scan(st, d_ccount, d_coff, C.nie, d_bsum));
      int ncand = 0;
      FH_CHECK_HIP(hipMemcpyAsync(&ncand, d_coff + C.nie, sizeof(int), hipMemcpyDeviceToHost, st));
      FH_CHECK_HIP(hipStreamSynchronize(st));
      FH_REQUIRE(ncand >= 0 && (int64_t)ncand * EM_W < ((int64_t)1 << 31), "%s: levels %d / %d: %d candidate nodes do not fit 32-bit offsets", who, Lc, Lf, ncand);
      if (!ncand) continue;
      EmScratch P(who);           // of this pair
      int *d_cnode, *d_cq, *d_tcnt, *d_tm, *d_th, *d_pbsum;
      double *d_cphi, *d_tv;
      if (P.get(&d_pbsum, (size_t)ncand / FH_SCAN_BLOCK + 2) || P.get(&d_cnode, (size_t)ncand) || P.get(&d_cq, (size_t)ncand) || P.get(&d_tcnt, (size_t)ncand + 1) || P.get(&d_cphi, (size_t)ncand * EM_W)) return 2;
      if (poison) {
        FH_CHECK_HIP(hipMemsetAsync(d_cnode, 0xFF, std::max<size_t>(ncand, 2) * sizeof(int), st));
        FH_CHECK_HIP(hipMemsetAsync(d_cq, 0xFF, std::max<size_t>(ncand, 2) * sizeof(int), st));
        FH_CHECK_HIP(hipMemsetAsync(d_tcnt, 0xFF, ((size_t)ncand + 1) * sizeof(int), st));
        FH_CHECK_HIP(hipMemsetAsync(d_cphi, 0xFF, (size_t)ncand * EM_W * sizeof(double), st));
      }
      hipLaunchKernelGGL(k_ec_candidates<true>, dim3(gq), dim3(256), 0, st, dT, K, dim, C.nie, C.ielist, M->d_geom, M->d_ed, M->d_x, Fn.nn, Fn.nid, Fn.nx, nullptr, d_coff, ncand,
                         d_cnode, d_cq);
      hipLaunchKernelGGL(k_ec_newton, dim3(gq), dim3(256), 0, st, dT, dim, fe, C.nie, C.ielist, M->d_geom, M->d_ed, M->d_x, d_emask, d_coff, ncand, d_cnode, d_cphi, d_tcnt);
      FH_CHECK_HIP(hipGetLastError());
      FH_TRY(fh_device_exclusive_scan(st, d_tcnt, d_tcnt, ncand, d_pbsum));
      int ntrip = 0;
      FH_CHECK_HIP(hipMemcpyAsync(&ntrip, d_tcnt + ncand, sizeof(int), hipMemcpyDeviceToHost, st));
      FH_CHECK_HIP(hipStreamSynchronize(st));
      FH_REQUIRE(ntrip >= 0 && (int64_t)ntrip <= (int64_t)ncand * EM_W, "%s: levels %d / %d: %d entries of %d candidates", who, Lc, Lf, ntrip, ncand);
      if (!ntrip) continue;
      if (P.get(&d_tm, (size_t)ntrip) || P.get(&d_th, (size_t)ntrip) || P.get(&d_tv, (size_t)ntrip)) return 2;
      if (poison) {
        FH_CHECK_HIP(hipMemsetAsync(d_tm, 0xFF, std::max<size_t>(ntrip, 2) * sizeof(int), st));
        FH_CHECK_HIP(hipMemsetAsync(d_th, 0xFF, std::max<size_t>(ntrip, 2) * sizeof(int), st));
        FH_CHECK_HIP(hipMemsetAsync(d_tv, 0xFF, std::max<size_t>(ntrip, 2) * sizeof(double), st));
      }
      hipLaunchKernelGGL(k_ec_emit, dim3(fh_div_up(ncand, 256)), dim3(256), 0, st, ncand, C.ielist, M->d_ed, d_cnode, d_cq, d_cphi, d_tcnt, ntrip, d_tm, d_th, d_tv);
      FH_CHECK_HIP(hipGetLastError());
      FH_CHECK_HIP(hipStreamSynchronize(st));
      const auto t0 = std::chrono::steady_clock::now();
      hm.resize(ntrip);
      hh.resize(ntrip);
      hv.resize(ntrip);
      FH_CHECK_HIP(hipMemcpyAsync(hm.data(), d_tm, (size_t)ntrip * sizeof(int), hipMemcpyDeviceToHost, st));
      FH_CHECK_HIP(hipMemcpyAsync(hh.data(), d_th, (size_t)ntrip * sizeof(int), hipMemcpyDeviceToHost, st));
      FH_CHECK_HIP(hipMemcpyAsync(hv.data(), d_tv, (size_t)ntrip * sizeof(double), hipMemcpyDeviceToHost, st));
      FH_CHECK_HIP(hipStreamSynchronize(st));
      for (int k = 0; k < ntrip; k++) {
        FH_REQUIRE(hm[k] >= 0 && hm[k] < nnode && hh[k] >= 0 && hh[k] < nnode, "%s: levels %d / %d: entry %d names the dofs %d and %d of %d", who, Lc, Lf, k, hm[k], hh[k], nnode);
        writes.push_back({hm[k], hh[k], Lc, hv[k]});
      }
      *ms_download += ec_ms(t0);
    }
  }
  return 0;
}

static int ec_download(fh_elem_mesh_t M, std::vector<int>& geom, std::vector<int>& ed, std::vector<double>& x, std::vector<int>& ff, std::vector<int>& lev) {
  geom.resize(M->nel);
  ed.resize((size_t)M->nel * EM_W);
  ff.resize((size_t)M->nel * EM_F);
  lev.resize(M->nel);
  x.resize((size_t)M->nnode * M->dim);
  FH_TRY(fh_elem_mesh_get(M, geom.data(), ed.data(), x.data(), ff.data()));
  FH_TRY(fh_elem_mesh_elem_levels(M, lev.data(), nullptr, nullptr, nullptr));
  return 0;
}

static int ec_rows(fh_elem_mesh_t M, int fe, int mode, AmrRows& R) {
  const char* who = "fh_elem_mesh_amr_constraints";
  FH_REQUIRE(M, "%s: null mesh", who);
  FH_REQUIRE(fe >= 0 && fe <= 2, "%s: fe must be 0 (linear), 1 (serendipity) or 2 (biquadratic), not %d", who, fe);
  FH_REQUIRE(mode == 0 || mode == 1, "%s: mode must be 0 (as the reference computes it) or 1 (coarsest level, rows sum to one), not %d", who, mode);
  const int key = fe * 4 + mode * 2 + (M->ctx->elem_constraints_host ? 1 : 0);
  if (M->amr_pending && M->amr_pending_key == key) {          // the sizing call of the two-call protocol left them
    R = *M->amr_pending;
    M->amr_pending.reset();
    return 0;
  }
  M->amr_pending.reset();
  R = AmrRows();
  R.ptr.push_back(0);
  for (double& t : M->amr_ms) t = 0.0;
  bool has_iface = false;
  std::vector<AmrTriple> writes;
  if (M->homogeneous) {
    // a mesh out of a refinement knows that it is homogeneous; one from host arrays whose levels nobody set only says so: an interface face shows that it is not
    if (!M->levels_unset) return 0;
    FH_TRY(ec_search_device(M, fe, true, &has_iface, writes, &M->amr_ms[1]));
    FH_REQUIRE(!has_iface, "%s: the mesh has faces with no neighbour and no boundary flag -- it was created non-homogeneous -- but the levels of its elements were "
               "never set (fh_elem_mesh_set_levels)", who);
    return 0;
  }
  const auto t0 = std::chrono::steady_clock::now();
  if (M->ctx->elem_constraints_host) {
    std::vector<int> geom, ed, ff, lev;
    std::vector<double> x;
    FH_TRY(ec_download(M, geom, ed, x, ff, lev));
    M->amr_ms[1] = ec_ms(t0);
    FH_TRY(fh_elem_amr_search_host(M->dim, M->nel, M->nnode, geom.data(), ed.data(), x.data(), ff.data(), lev.data(), fe, writes));
  } else {
    FH_TRY(ec_search_device(M, fe, false, &has_iface, writes, &M->amr_ms[1]));
  }
  M->amr_ms[0] = ec_ms(t0) - M->amr_ms[1];
  const auto t1 = std::chrono::steady_clock::now();
  fh_amr_resolve(writes, M->nnode, mode, R);
  M->amr_ms[2] = ec_ms(t1);
  return 0;
}

extern "C" int fh_elem_mesh_amr_constraints(fh_elem_mesh_t M, int fe, int mode, int* n_hanging, int* nnz, int* hanging, int* ptr, int* master, double* weight) {
  FH_GUARD_BEGIN
  FH_REQUIRE(M && n_hanging && nnz, "fh_elem_mesh_amr_constraints: null argument");
  AmrRows R;
  FH_TRY(ec_rows(M, fe, mode, R));
  if (hanging) {
    FH_REQUIRE(*n_hanging >= (int)R.hang.size() && *nnz >= (int)R.master.size(), "fh_elem_mesh_amr_constraints: capacity too small");
    fh_copy_out(hanging, R.hang);
    if (ptr) fh_copy_out(ptr, R.ptr);
    if (master) fh_copy_out(master, R.master);
    if (weight) fh_copy_out(weight, R.w);
  } else {                        // the filling call takes the rows from here instead of searching again
    M->amr_pending = std::make_shared<AmrRows>(R);
    M->amr_pending_key = fe * 4 + mode * 2 + (M->ctx->elem_constraints_host ? 1 : 0);
  }
  *n_hanging = (int)R.hang.size();
  *nnz = (int)R.master.size();
  return 0;
  FH_GUARD_END("fh_elem_mesh_amr_constraints")
}

extern "C" int fh_elem_mesh_amr_timings(fh_elem_mesh_t M, double ms[3]) {
  FH_REQUIRE(M && ms, "fh_elem_mesh_amr_timings: null argument");
  for (int k = 0; k < 3; k++) ms[k] = M->amr_ms[k];
  return 0;
}

// P_amr (n x n) as fh_build_amr_prolongator builds it: identity rows for regular dofs; a hanging dof's row holds its master weights and an explicit zero on the diagonal
extern "C" int fh_elem_mesh_amr_prolongator(fh_elem_mesh_t M, int fe, int mode, fh_mat_t* out) {
  FH_GUARD_BEGIN
  FH_REQUIRE(M && out, "fh_elem_mesh_amr_prolongator: null argument");
  AmrRows R;
  FH_TRY(ec_rows(M, fe, mode, R));
  const int n = M->own[fe];
  std::vector<int> rowptr, col;
  std::vector<double> val;
  FH_REQUIRE(fh_amr_prolongator_csr(R, n, rowptr, col, val), "fh_elem_mesh_amr_prolongator: a hanging dof beyond the family's %d dofs", n);
  return fh_mat_create_csr(M->ctx, n, n, rowptr.data(), col.data(), val.data(), out);
  FH_GUARD_END("fh_elem_mesh_amr_prolongator")
}
