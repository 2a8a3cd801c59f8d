// Flags of a resident element mesh from the solution: Solution::FlagAMRRegionBasedOnErroNormAdaptive (Solution.cpp:843-1101) for one variable, any mix of the
// five shapes, and its statement on plain host arrays (fh_elem_error_flag_host).  The rule is in include/femus_hip.h; the element body -- one Gauss point, the
// sums over the points, the comparisons -- is fh_elemerror_body.h, compiled for both sides.
//
// The walk of the reference and why its order does not matter.  It visits the refinable elements in ascending order with a mark 0 / 1 / 2 per element.  A strong
// element i (S_i: err_i > eps2 vol_i) is flagged, marks its later refinable vertex-neighbours 2 and flags the earlier ones that were left at 0 and are weak
// (W_j: err_j > neighbor_threshold eps2 vol_j).  An element that arrives with mark 2 is flagged when it is weak.  So an element that is not strong ends flagged
// exactly when it is weak and has a strong refinable neighbour: an EARLIER such neighbour left the 2 it is tested with, a LATER one tests it itself; and nothing
// else flags it.  Hence flag_i = S_i or (W_i and some refinable vertex-neighbour j != i has S_j), and errTestTrue2 -- added when an element is left at 0, taken
// back when a later neighbour flags it -- is the sum of err_i over the refinable elements that end unflagged.
//
// Device path, five launches and two copies, nothing per element on the host:
//   1. k_ee_elements   L = 16 / 32 / 64 lanes per element (16 / 8 / 4 elements per workgroup of 256) from the largest Gauss rule among the mesh's shapes, elements
//                      in table order whatever their shape (a sub-group reads its own shape's tables; waves are uniform on single-shape meshes).  The
//                      coordinates and the two value vectors of the element's dofs are staged in LDS, lane = Gauss point (ee_point) leaves the point's terms in
//                      LDS, lane 0 adds them in ascending order (ee_element_sums): err_i, vol_i and the element's share of solNorm2.
//   2. k_ee_reduce     the sums, fixed shape: chunks of 1024 consecutive entries, 256 strided running sums per chunk and a binary tree in LDS, the partials
//                      in chunk order through the same kernel until one is left (ee_fixed_sum is the same shape on the host).  No floating-point atomics.
//   3. k_ee_strong     a strong element stores 1 into a byte per vertex (the first n_vertices entries of its row); plain stores of the same value, a benign race
//   4. k_ee_flags      every refinable element: S_i, or W_i and a marked vertex (an element that is not strong sees only marks of others); the flags go to
//                      d_flags of the mesh, the terms of volumeTestFalse and errTestTrue2 to the work arrays, the count by one integer atomic per wave
//   5. k_ee_reduce     the last two sums
// The new threshold and the convergence test are evaluated on the host in double.
#include "fh_elemerror.h"
#include <cmath>

using namespace fherr;

// ---- shared with fh_elemnorm.hip (fh_elemerror.h) ----
namespace fherr {
bool ee_shape(int g) { return g == fhfe::GEOM_HEX || g == fhfe::GEOM_QUAD || g == fhfe::GEOM_TRI || g == fhfe::GEOM_TET || g == fhfe::GEOM_WEDGE; }

int ee_tables(const char* who, int dim, int fe, int order, const bool present[EM_G], EeHostTabs& H) {
  memset(&H.t, 0, sizeof(H.t));
  FH_REQUIRE(order >= 0 && order <= 4, "%s: unsupported Gauss rule %d", who, order);
  for (int g = 0; g < EM_G; g++) {
    if (!present[g]) continue;
    FH_REQUIRE(ee_shape(g) && fhfe::dim_of(g) == dim, "%s: shape code %d in a %d-dimensional mesh", who, g, dim);
    std::vector<double> w, phi, dphi;
    FH_REQUIRE(fhfe::shape_tables(g, fe, order, w, phi, dphi) == 0 && !w.empty() && (int)w.size() <= EE_MAXG, "%s: unsupported Gauss rule %d", who, order);
    const int nc = fhfe::ndofs_of(g, fe), ng = (int)w.size();
    FH_REQUIRE(nc >= 1 && nc <= EM_W && phi.size() == (size_t)ng * nc && dphi.size() == (size_t)ng * nc * dim, "%s: unexpected table sizes (shape %d)", who, g);
    H.t.nc[g] = nc;
    H.t.ng[g] = ng;
    H.t.ow[g] = (int)H.buf.size();
    H.buf.insert(H.buf.end(), w.begin(), w.end());
    H.t.ophi[g] = (int)H.buf.size();
    H.buf.insert(H.buf.end(), phi.begin(), phi.end());
    H.t.odphi[g] = (int)H.buf.size();
    H.buf.insert(H.buf.end(), dphi.begin(), dphi.end());
    H.ncmax = std::max(H.ncmax, nc);
    H.ngmax = std::max(H.ngmax, ng);
  }
  return 0;
}

double ee_fixed_sum(std::vector<double> a) {
#pragma clang fp contract(off)
  if (a.empty()) return 0.0;
  do {
    const size_t n = a.size(), nch = (n + EE_RC - 1) / EE_RC;
    std::vector<double> out(nch);
    for (size_t c = 0; c < nch; c++) {
      const size_t base = c * EE_RC, cnt = std::min<size_t>(EE_RC, n - base);
      double s[EE_RB];
      for (int t = 0; t < EE_RB; t++) {
        double v = 0.0;
        for (size_t i = t; i < cnt; i += EE_RB) v += a[base + i];
        s[t] = v;
      }
      for (int off = EE_RB / 2; off > 0; off >>= 1)
        for (int t = 0; t < off; t++) s[t] += s[t + off];
      out[c] = s[0];
    }
    a.swap(out);
  } while (a.size() > 1);
  return a[0];
}
}  // namespace fherr

namespace {
int ee_check_options(const char* who, int fe, int norm, double threshold, double neighbor_threshold) {
  FH_REQUIRE(fe >= 0 && fe <= 2, "%s: fe must be 0 (linear), 1 (serendipity) or 2 (biquadratic), not %d", who, fe);
  FH_REQUIRE(norm == 0 || norm == 1, "%s: norm must be 0 (L2) or 1 (H1), not %d", who, norm);
  FH_REQUIRE(std::isfinite(threshold) && threshold >= 0.0, "%s: the threshold must be finite and not negative, not %g", who, threshold);
  FH_REQUIRE(std::isfinite(neighbor_threshold) && neighbor_threshold >= 0.0, "%s: the neighbour threshold must be finite and not negative, not %g", who,
             neighbor_threshold);
  return 0;
}

// what follows the sums, on the host in double: the new threshold in the reference's expression (Solution.cpp:1083), 1 when nothing is flagged
void ee_finish(int dim, double threshold, const double sums[5], long long nflagged, double* new_threshold, int* converged) {
#pragma clang fp contract(off)
  const double solNorm2 = sums[0], volume = sums[1], volumeRefined = sums[2], volumeTestFalse = sums[3], errTestTrue2 = sums[4];
  if (new_threshold)
    *new_threshold = volumeTestFalse != 0 ? sqrt(threshold * threshold * volumeRefined / volumeTestFalse - errTestTrue2 / solNorm2 * volume / volumeTestFalse) : 1.;
  if (converged) *converged = nflagged * (1LL << dim) <= 1 ? 1 : 0;
}

template <int L>
__global__ __launch_bounds__(256) void k_ee_elements(int nel, int dim, int level, int norm, double sc, EeTabs tb, int ncmax, int ngmax, const double* __restrict__ tab,
                                                     const int* __restrict__ geom, const int* __restrict__ ed, const double* __restrict__ x,
                                                     const int* __restrict__ lev, const double* __restrict__ S, const double* __restrict__ E,
                                                     double* __restrict__ T /* [3][nel]: solNorm2 share, volume, refinable volume */, double* __restrict__ err) {
  extern __shared__ __attribute__((aligned(16))) double ee_smem[];
  constexpr int EPG = 256 / L;
  const int sub = threadIdx.x / L, lane = threadIdx.x % L;
  const int e = blockIdx.x * EPG + sub;
  const int nt = ee_nterms(dim, norm), st = 2 * nt + 1;
  double* X = ee_smem + (size_t)sub * (ncmax * 5 + ngmax * st);       // [ncmax][3]
  double* Sv = X + ncmax * 3;                                         // [ncmax]
  double* Ev = Sv + ncmax;                                            // [ncmax]
  double* TT = Ev + ncmax;                                            // [ngmax][st]
  const bool active = e < nel;                   // tail sub-groups keep the barriers and touch nothing
  int g = 0, nc = 0, ng = 0;
  if (active) {
    g = geom[e];
    nc = tb.nc[g];
    ng = tb.ng[g];
    for (int n = lane; n < nc; n += L) {
      const int dof = ed[(size_t)e * EM_W + n];
      for (int d = 0; d < 3; d++) X[n * 3 + d] = d < dim ? x[(size_t)dof * dim + d] : 0.0;
      Sv[n] = S ? S[dof] : 0.0;
      Ev[n] = E[dof];
    }
  }
  __syncthreads();
  if (active)
    for (int ig = lane; ig < ng; ig += L)
      ee_point(dim, nc, tab[tb.ow[g] + ig], tab + tb.ophi[g] + (size_t)ig * nc, tab + tb.odphi[g] + (size_t)ig * nc * dim, X, S ? Sv : nullptr, Ev, norm, sc, TT + ig * st);
  __syncthreads();
  if (active && lane == 0) {
    double r[3];
    ee_element_sums(ng, nt, TT, r);
    const bool refinable = lev[e] == level;
    T[e] = r[0];
    T[(size_t)nel + e] = r[1];
    T[(size_t)2 * nel + e] = refinable ? r[1] : 0.0;
    err[e] = refinable ? r[2] : 0.0;
  }
}

// out[k * out_stride + chunk] = the sum of chunk `chunk` of array k (blockIdx.y) of n entries
__global__ __launch_bounds__(EE_RB) void k_ee_reduce(size_t n, const double* __restrict__ in, size_t in_stride, double* __restrict__ out, size_t out_stride) {
#pragma clang fp contract(off)
  __shared__ double s[EE_RB];
  const int t = threadIdx.x;
  const size_t base = (size_t)blockIdx.x * EE_RC, cnt = min((size_t)EE_RC, n - base);
  const double* a = in + (size_t)blockIdx.y * in_stride + base;
  double v = 0.0;
  for (size_t i = t; i < cnt; i += EE_RB) v += a[i];
  s[t] = v;
  __syncthreads();
  for (int off = EE_RB / 2; off > 0; off >>= 1) {
    if (t < off) s[t] += s[t + off];
    __syncthreads();
  }
  if (t == 0) out[(size_t)blockIdx.y * out_stride + blockIdx.x] = s[0];
}

__global__ __launch_bounds__(256) void k_ee_strong(int nel, int level, double threshold, const int* __restrict__ lev, const int* __restrict__ geom,
                                                   const int* __restrict__ ed, const double* __restrict__ err, const double* __restrict__ vol,
                                                   const double* __restrict__ sums, unsigned char* __restrict__ vmark) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= nel || lev[e] != level) return;
  if (!ee_strong(err[e], vol[e], ee_eps2(threshold, sums[0], sums[1]))) return;
  const int nv = fhfe::hd::nvert_of(geom[e]);
  for (int v = 0; v < nv; v++) vmark[ed[(size_t)e * EM_W + v]] = 1;
}

__global__ __launch_bounds__(256) void k_ee_flags(int nel, int level, double threshold, double neighbor_threshold, const int* __restrict__ lev,
                                                  const int* __restrict__ geom, const int* __restrict__ ed, const double* __restrict__ err,
                                                  const double* __restrict__ vol, const double* __restrict__ sums, const unsigned char* __restrict__ vmark,
                                                  unsigned char* __restrict__ flags, double* __restrict__ vtf, double* __restrict__ ett,
                                                  unsigned long long* __restrict__ count) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  bool f = false;
  if (e < nel) {
    const bool refinable = lev[e] == level;
    double er = 0.0, vo = 0.0;
    if (refinable) {
      er = err[e];
      vo = vol[e];
      const double eps2 = ee_eps2(threshold, sums[0], sums[1]);
      f = ee_strong(er, vo, eps2);
      if (!f && ee_weak(er, vo, eps2, neighbor_threshold)) {
        const int nv = fhfe::hd::nvert_of(geom[e]);
        for (int v = 0; v < nv; v++) f = f || vmark[ed[(size_t)e * EM_W + v]] != 0;
      }
    }
    flags[e] = f ? 1 : 0;
    vtf[e] = f ? vo : 0.0;
    ett[e] = (refinable && !f) ? er : 0.0;
  }
  const unsigned long long b = __ballot(f);
  if ((threadIdx.x & 63) == 0 && b) atomicAdd(count, (unsigned long long)__popcll(b));
}

}  // namespace

// nk arrays of n entries at d_in (stride n) -> d_out[0 .. nk); p0 / p1 hold nk * ceil(n / EE_RC) doubles each
void fherr::ee_reduce(hipStream_t st, size_t n, int nk, const double* d_in, double* p0, double* p1, double* d_out) {
  const double* in = d_in;
  size_t stride = n;
  double* p[2] = {p0, p1};
  int w = 0;
  do {
    const size_t nch = (n + EE_RC - 1) / EE_RC;
    double* out = nch == 1 ? d_out : p[w];
    const size_t ostride = nch == 1 ? 1 : nch;
    hipLaunchKernelGGL(k_ee_reduce, dim3((unsigned)nch, nk), dim3(EE_RB), 0, st, n, in, stride, out, ostride);
    in = out;
    stride = ostride;
    n = nch;
    w ^= 1;
  } while (n > 1);
}

namespace {
struct EeWork {
  double *d_tab = nullptr, *d_T = nullptr, *d_err = nullptr, *d_p0 = nullptr, *d_p1 = nullptr, *d_sums = nullptr;
  unsigned char* d_vmark = nullptr;
  unsigned long long* d_count = nullptr;
};

// everything the two device entry points check before they allocate
int ee_check_mesh_call(const char* who, fh_elem_mesh_t m, int fe, int order, int norm, fh_vec_t sol, fh_vec_t eps, EeHostTabs& H) {
  FH_TRY(ee_check_options(who, fe, norm, 0.0, 0.0));
  for (fh_vec_t v : {sol, eps}) {
    if (!v) continue;
    FH_REQUIRE(v->ctx == m->ctx, "%s: a vector of another context than the mesh's", who);
    FH_REQUIRE(v->n_global == m->own[fe] && v->n_local == m->own[fe], "%s: a vector of %d entries, the family has %d dofs on this mesh", who, v->n_global, m->own[fe]);
  }
  bool present[EM_G];
  for (int g = 0; g < EM_G; g++) present[g] = m->count[g] > 0;
  FH_TRY(ee_tables(who, m->dim, fe, order, present, H));
  return 0;
}

// launch 1 (and its buffers): S may be null
int ee_run_elements(const char* who, fh_elem_mesh_t m, int fe, int norm, const EeHostTabs& H, const double* S, const double* E, EmScratch& B, EeWork& W) {
  fh_ctx_t ctx = m->ctx;
  hipStream_t st = ctx->stream;
  const size_t nel = (size_t)m->nel, nch = (nel + EE_RC - 1) / EE_RC;
  if (B.get(&W.d_tab, H.buf.size()) || B.get(&W.d_T, 5 * nel) || B.get(&W.d_err, nel) || B.get(&W.d_p0, 3 * nch) || B.get(&W.d_p1, 3 * nch) || B.get(&W.d_sums, (size_t)8) ||
      B.get(&W.d_vmark, (size_t)m->nnode + 8) || B.get(&W.d_count, (size_t)2))
    return 2;
  if (ctx->debug_poison) {        // every entry is written before it is read
    FH_CHECK_HIP(hipMemsetAsync(W.d_T, 0xFF, std::max<size_t>(5 * nel, 2) * sizeof(double), st));
    FH_CHECK_HIP(hipMemsetAsync(W.d_err, 0xFF, std::max<size_t>(nel, 2) * sizeof(double), st));
    FH_CHECK_HIP(hipMemsetAsync(W.d_p0, 0xFF, std::max<size_t>(3 * nch, 2) * sizeof(double), st));
    FH_CHECK_HIP(hipMemsetAsync(W.d_p1, 0xFF, std::max<size_t>(3 * nch, 2) * sizeof(double), st));
    FH_CHECK_HIP(hipMemsetAsync(W.d_sums, 0xFF, 8 * sizeof(double), st));
  }
  FH_CHECK_HIP(hipMemsetAsync(W.d_vmark, 0, (size_t)m->nnode + 8, st));       // the marks and the count start at zero: they are state, not work space
  FH_CHECK_HIP(hipMemsetAsync(W.d_count, 0, 2 * sizeof(unsigned long long), st));
  FH_CHECK_HIP(hipMemcpyAsync(W.d_tab, H.buf.data(), H.buf.size() * sizeof(double), hipMemcpyHostToDevice, st));
  const int L = H.ngmax <= 16 ? 16 : H.ngmax <= 32 ? 32 : 64, epg = 256 / L;
  const int nt = ee_nterms(m->dim, norm);
  const size_t lds = (size_t)epg * (H.ncmax * 5 + H.ngmax * (2 * nt + 1)) * sizeof(double);
  FH_REQUIRE(lds <= 64 * 1024, "%s: %zu bytes of LDS per workgroup", who, lds);
  const double sc = ee_scale2(fe, norm);
  const dim3 grid(fh_div_up(m->nel, epg)), block(256);
#define EE_LAUNCH(LL)                                                                                                                                              \
  hipLaunchKernelGGL(k_ee_elements<LL>, grid, block, lds, st, m->nel, m->dim, m->level, norm, sc, H.t, H.ncmax, H.ngmax, W.d_tab, m->d_geom, m->d_ed, m->d_x, m->d_lev, S, \
                     E, W.d_T, W.d_err)
  if (L == 16) EE_LAUNCH(16);
  else if (L == 32) EE_LAUNCH(32);
  else EE_LAUNCH(64);
#undef EE_LAUNCH
  FH_CHECK_HIP(hipGetLastError());
  return 0;
}
}  // namespace

extern "C" int fh_elem_mesh_error_flag(fh_elem_mesh_t m, int fe, int gauss_order, fh_vec_t sol, fh_vec_t eps, int norm, double threshold, double neighbor_threshold,
                                       unsigned char* flags, double sums[5], double* new_threshold, long long* nflagged, int* converged) {
  FH_GUARD_BEGIN
  const char* who = "fh_elem_mesh_error_flag";
  FH_REQUIRE(m && sol && eps, "%s: null argument", who);
  FH_TRY(ee_check_options(who, fe, norm, threshold, neighbor_threshold));
  EeHostTabs H;
  FH_TRY(ee_check_mesh_call(who, m, fe, gauss_order, norm, sol, eps, H));
  hipStream_t st = m->ctx->stream;
  const size_t nel = (size_t)m->nel, nbytes = std::max<size_t>(nel, 8);
  double hs[5] = {0, 0, 0, 0, 0};
  unsigned long long count = 0;
  if (!m->d_flags) FH_CHECK_HIP(hipMalloc((void**)&m->d_flags, nbytes));
  auto drop = [&]() {             // flags of a pass that failed are no flags: refine("resident") refuses
    hipFree(m->d_flags);
    m->d_flags = nullptr;
  };
  if (nel) {
    EmScratch B(who);
    EeWork W;
    auto run = [&]() -> int {
      if (m->ctx->debug_poison) FH_CHECK_HIP(hipMemsetAsync(m->d_flags, 0xFF, nbytes, st));      // every entry is written before it is read
      FH_TRY(ee_run_elements(who, m, fe, norm, H, sol->d, eps->d, B, W));
      ee_reduce(st, nel, 3, W.d_T, W.d_p0, W.d_p1, W.d_sums);
      const dim3 grid(fh_div_up(m->nel, 256)), block(256);
      hipLaunchKernelGGL(k_ee_strong, grid, block, 0, st, m->nel, m->level, threshold, m->d_lev, m->d_geom, m->d_ed, W.d_err, W.d_T + nel, W.d_sums, W.d_vmark);
      hipLaunchKernelGGL(k_ee_flags, grid, block, 0, st, m->nel, m->level, threshold, neighbor_threshold, m->d_lev, m->d_geom, m->d_ed, W.d_err, W.d_T + nel, W.d_sums,
                         W.d_vmark, m->d_flags, W.d_T + 3 * nel, W.d_T + 4 * nel, W.d_count);
      ee_reduce(st, nel, 2, W.d_T + 3 * nel, W.d_p0, W.d_p1, W.d_sums + 3);
      FH_CHECK_HIP(hipGetLastError());
      FH_CHECK_HIP(hipMemcpyAsync(hs, W.d_sums, 5 * sizeof(double), hipMemcpyDeviceToHost, st));
      FH_CHECK_HIP(hipMemcpyAsync(&count, W.d_count, sizeof(count), hipMemcpyDeviceToHost, st));
      if (flags) FH_CHECK_HIP(hipMemcpyAsync(flags, m->d_flags, nel, hipMemcpyDeviceToHost, st));
      return 0;
    };
    const int rc = run();
    const hipError_t he = hipStreamSynchronize(st);     // the work buffers are freed on return
    if (rc || he != hipSuccess) drop();
    if (rc) return rc;
    FH_CHECK_HIP(he);
  }
  if (sums)
    for (int k = 0; k < 5; k++) sums[k] = hs[k];
  if (nflagged) *nflagged = (long long)count;
  ee_finish(m->dim, threshold, hs, (long long)count, new_threshold, converged);
  return 0;
  FH_GUARD_END("fh_elem_mesh_error_flag")
}

extern "C" int fh_elem_mesh_error_indicators(fh_elem_mesh_t m, int fe, int gauss_order, fh_vec_t eps, int norm, double* err2, double* vol) {
  FH_GUARD_BEGIN
  const char* who = "fh_elem_mesh_error_indicators";
  FH_REQUIRE(m && eps, "%s: null argument", who);
  EeHostTabs H;
  FH_TRY(ee_check_mesh_call(who, m, fe, gauss_order, norm, nullptr, eps, H));
  if (!m->nel) return 0;
  hipStream_t st = m->ctx->stream;
  const size_t nel = (size_t)m->nel;
  EmScratch B(who);
  EeWork W;
  auto run = [&]() -> int {
    FH_TRY(ee_run_elements(who, m, fe, norm, H, nullptr, eps->d, B, W));
    if (err2) FH_CHECK_HIP(hipMemcpyAsync(err2, W.d_err, nel * sizeof(double), hipMemcpyDeviceToHost, st));
    if (vol) FH_CHECK_HIP(hipMemcpyAsync(vol, W.d_T + 2 * nel, nel * sizeof(double), hipMemcpyDeviceToHost, st));
    return 0;
  };
  const int rc = run();
  const hipError_t he = hipStreamSynchronize(st);       // the work buffers are freed on return
  if (rc) return rc;
  FH_CHECK_HIP(he);
  return 0;
  FH_GUARD_END("fh_elem_mesh_error_indicators")
}

extern "C" int fh_elem_error_flag_host(int dim, int nel, const int* elem_geom, const int* elem_dof, const int* lev, int level, int nnode, const double* coords, int fe,
                                       int gauss_order, const double* sol, const double* eps, int norm, double threshold, double neighbor_threshold,
                                       unsigned char* flags, double* err2, double* vol, double sums[5], double* new_threshold, long long* nflagged, int* converged) {
  FH_GUARD_BEGIN
  const char* who = "fh_elem_error_flag_host";
  FH_REQUIRE(nel >= 0 && nnode >= 0, "%s: negative size", who);
  FH_REQUIRE(dim == 2 || dim == 3, "%s: dim must be 2 or 3, not %d", who, dim);
  FH_TRY(ee_check_options(who, fe, norm, threshold, neighbor_threshold));
  FH_REQUIRE(nel == 0 || (elem_geom && elem_dof && lev && coords && sol && eps), "%s: null argument", who);
  bool present[EM_G] = {false, false, false, false, false, false};
  for (int e = 0; e < nel; e++) {
    const int g = elem_geom[e];
    FH_REQUIRE(g >= 0 && g < EM_G && ee_shape(g) && fhfe::dim_of(g) == dim, "%s: element %d has shape code %d in a %d-dimensional mesh", who, e, g, dim);
    present[g] = true;
    for (int k = 0; k < fhfe::nloc_of(g); k++)
      FH_REQUIRE(elem_dof[(size_t)e * EM_W + k] >= 0 && elem_dof[(size_t)e * EM_W + k] < nnode, "%s: element %d, local node %d: id %d outside [0, %d)", who, e, k,
                 elem_dof[(size_t)e * EM_W + k], nnode);
  }
  EeHostTabs H;
  FH_TRY(ee_tables(who, dim, fe, gauss_order, present, H));
  const int nt = ee_nterms(dim, norm);
  const double sc = ee_scale2(fe, norm);
  std::vector<double> T((size_t)5 * nel, 0.0), er((size_t)nel, 0.0);
  std::vector<double> TT((size_t)EE_MAXG * EE_MAXT);
  for (int e = 0; e < nel; e++) {
    const int g = elem_geom[e], nc = H.t.nc[g], ng = H.t.ng[g];
    const int* ed = elem_dof + (size_t)e * EM_W;
    double X[EM_W * 3], Sv[EM_W], Ev[EM_W], r[3];
    for (int n = 0; n < nc; n++) {
      for (int d = 0; d < 3; d++) X[n * 3 + d] = d < dim ? coords[(size_t)ed[n] * dim + d] : 0.0;
      Sv[n] = sol[ed[n]];
      Ev[n] = eps[ed[n]];
    }
    for (int ig = 0; ig < ng; ig++)
      ee_point(dim, nc, H.buf[H.t.ow[g] + ig], &H.buf[H.t.ophi[g] + (size_t)ig * nc], &H.buf[H.t.odphi[g] + (size_t)ig * nc * dim], X, Sv, Ev, norm, sc,
               &TT[(size_t)ig * (2 * nt + 1)]);
    ee_element_sums(ng, nt, TT.data(), r);
    const bool refinable = lev[e] == level;
    T[e] = r[0];
    T[(size_t)nel + e] = r[1];
    T[(size_t)2 * nel + e] = refinable ? r[1] : 0.0;
    er[e] = refinable ? r[2] : 0.0;
  }
  auto arr = [&](int k) { return std::vector<double>(T.begin() + (size_t)k * nel, T.begin() + (size_t)(k + 1) * nel); };
  double hs[5] = {0, 0, 0, 0, 0};
  for (int k = 0; k < 3; k++) hs[k] = ee_fixed_sum(arr(k));
  const double eps2 = nel ? ee_eps2(threshold, hs[0], hs[1]) : 0.0;
  std::vector<unsigned char> vmark((size_t)nnode, 0), fl((size_t)nel, 0);
  for (int e = 0; e < nel; e++)
    if (lev[e] == level && ee_strong(er[e], T[(size_t)nel + e], eps2))
      for (int v = 0; v < fhfe::nvert_of(elem_geom[e]); v++) vmark[elem_dof[(size_t)e * EM_W + v]] = 1;
  long long count = 0;
  for (int e = 0; e < nel; e++) {
    const bool refinable = lev[e] == level;
    bool f = false;
    const double vo = T[(size_t)nel + e];
    if (refinable) {
      f = ee_strong(er[e], vo, eps2);
      if (!f && ee_weak(er[e], vo, eps2, neighbor_threshold))
        for (int v = 0; v < fhfe::nvert_of(elem_geom[e]); v++) f = f || vmark[elem_dof[(size_t)e * EM_W + v]] != 0;
    }
    fl[e] = f ? 1 : 0;
    count += f ? 1 : 0;
    T[(size_t)3 * nel + e] = f ? vo : 0.0;
    T[(size_t)4 * nel + e] = (refinable && !f) ? er[e] : 0.0;
  }
  for (int k = 3; k < 5; k++) hs[k] = ee_fixed_sum(arr(k));
  if (flags) fh_copy_out(flags, fl);
  if (err2) fh_copy_out(err2, er);
  if (vol)
    for (int e = 0; e < nel; e++) vol[e] = T[(size_t)2 * nel + e];
  if (sums)
    for (int k = 0; k < 5; k++) sums[k] = hs[k];
  if (nflagged) *nflagged = count;
  ee_finish(dim, threshold, hs, count, new_threshold, converged);
  return 0;
  FH_GUARD_END("fh_elem_error_flag_host")
}
