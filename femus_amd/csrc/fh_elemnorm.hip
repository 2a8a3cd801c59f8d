// Error norms of a resident element mesh's solution against a known one: GetErrorNorm_L2_H1_with_analytical_sol (FE_convergence.hpp:1279-1415) and its variants
// (:1457-, :480-935) for one variable, any mix of the five shapes, homogeneous or not -- every element counts: the copies and children of a flagged level cover
// the domain once -- and its statement on plain host arrays (fh_elem_error_norms_host).  The rule is in include/femus_hip.h; the element body is
// fh_elemnorm_body.h, compiled for both sides; tables, the fixed-shape sums and their host form are those of the flags (fh_elemerror.h).
//
// Device path, the element kernel and the reduction, nothing per element on the host:
//   1. k_en_elements   the layout of k_ee_elements: L = 16 / 32 / 64 lanes per element from the largest Gauss rule among the mesh's shapes, elements in table order,
//                      a sub-group reads its own shape's tables.  Lane n < nc stages the coordinates and sol of dof n in LDS and with them U_n: other_n (mode
//                      vector) or the exact program at the dof it has just read (mode dofs).  After the barrier lane = Gauss point (en_point) leaves 1 + dim
//                      terms in LDS -- the weight is a factor of each and is not kept on its own --, after another lane 0 adds them in ascending order
//                      (en_element_sums): l2_i and h1_i.  Tail sub-groups keep the barriers and touch nothing.  Mode vector runs an instantiation without the
//                      evaluator (no scratch); the other carries it and with it the scratch of its operand stack, as every kernel that runs programs does.
//   2. k_ee_reduce     the two sums in the fixed shape of the flags (ee_reduce; ee_fixed_sum on the host).  No floating-point atomics.
// The square roots are taken on the host.
#include "fh_elemerror.h"
#include "fh_elemnorm_body.h"
#include <cmath>

using namespace fherr;

namespace {
struct EnHostProgs {              // the 1 + dim programs back to back, as fh_faces.hip uploads its fluxes
  std::vector<int> code, cptr{0}, kptr{0};
  std::vector<double> consts;
  EnProgs view() const { return EnProgs{code.data(), cptr.data(), consts.data(), kptr.data()}; }
};

// fe, mode and which of exact / gradient / other the mode wants; fetches the programs (refusing one over more than x, y, z, t)
int en_check_options(const char* who, int dim, int fe, int mode, fh_expr_t exact, const fh_expr_t* gradient, bool other, EnHostProgs& P) {
  FH_REQUIRE(fe >= 0 && fe <= 2, "%s: fe must be 0 (linear), 1 (serendipity) or 2 (biquadratic), not %d", who, fe);
  FH_REQUIRE(mode >= EN_QP && mode <= EN_VECTOR, "%s: mode must be 0 (qp), 1 (dofs) or 2 (vector), not %d", who, mode);
  static const char* const names[3] = {"0 (qp)", "1 (dofs)", "2 (vector)"};
  if (mode == EN_VECTOR) {
    FH_REQUIRE(other, "%s: mode %s needs other", who, names[mode]);
    FH_REQUIRE(!exact, "%s: exact is not allowed in mode %s", who, names[mode]);
  } else {
    FH_REQUIRE(exact, "%s: mode %s needs exact", who, names[mode]);
    FH_REQUIRE(!other, "%s: other is not allowed in mode %s", who, names[mode]);
  }
  if (mode == EN_QP) {
    FH_REQUIRE(gradient, "%s: mode %s needs gradient", who, names[mode]);
    for (int j = 0; j < dim; j++) FH_REQUIRE(gradient[j], "%s: mode %s needs gradient[%d]", who, names[mode], j);
  } else {
    FH_REQUIRE(!gradient, "%s: gradient is not allowed in mode %s", who, names[mode]);
  }
  const int nprog = mode == EN_QP ? 1 + dim : mode == EN_DOFS ? 1 : 0;
  for (int k = 0; k < nprog; k++) {
    char what[96];
    if (k == 0) snprintf(what, sizeof what, "%s: exact", who);
    else snprintf(what, sizeof what, "%s: gradient[%d]", who, k - 1);
    std::vector<int> code;
    std::vector<double> consts;
    FH_TRY(fh_expr_fetch(k == 0 ? exact : gradient[k - 1], what, 4, code, consts));
    P.code.insert(P.code.end(), code.begin(), code.end());
    P.consts.insert(P.consts.end(), consts.begin(), consts.end());
    P.cptr.push_back((int)P.code.size());
    P.kptr.push_back((int)P.consts.size());
  }
  return 0;
}

// PROGS: the kernel of modes qp and dofs, which runs programs; without it (mode vector) no evaluator is compiled in and the kernel uses no scratch
template <int L, bool PROGS>
__global__ __launch_bounds__(256) void k_en_elements(int nel, int dim, int mode, EeTabs tb, int ncmax, int ngmax, const double* __restrict__ tab,
                                                     const int* __restrict__ geom, const int* __restrict__ ed, const double* __restrict__ x,
                                                     const double* __restrict__ S, const double* __restrict__ O, EnProgs pr,
                                                     double* __restrict__ T /* [2][nel]: l2_i, h1_i */) {
  extern __shared__ __attribute__((aligned(16))) double en_smem[];
  constexpr int EPG = 256 / L;
  const int sub = threadIdx.x / L, lane = threadIdx.x % L;
  const int e = blockIdx.x * EPG + sub;
  const int st = 1 + dim;
  double* X = en_smem + (size_t)sub * (ncmax * 5 + ngmax * st);       // [ncmax][3]
  double* Sv = X + ncmax * 3;                                         // [ncmax]
  double* Uv = Sv + ncmax;                                            // [ncmax]
  double* TT = Uv + ncmax;                                            // [ngmax][st]
  const bool active = e < nel;                   // tail sub-groups keep the barriers and touch nothing
  int g = 0, nc = 0, ng = 0;
  if (active) {
    g = geom[e];
    nc = tb.nc[g];
    ng = tb.ng[g];
    for (int n = lane; n < nc; n += L) {
      const int dof = ed[(size_t)e * EM_W + n];
      double xn[3];
      for (int d = 0; d < 3; d++) xn[d] = X[n * 3 + d] = d < dim ? x[(size_t)dof * dim + d] : 0.0;
      Sv[n] = S[dof];
      if (!PROGS) Uv[n] = O[dof];
      else if (mode == EN_DOFS) Uv[n] = en_nodal(pr, xn);
    }
  }
  __syncthreads();
  if (active)
    for (int ig = lane; ig < ng; ig += L)
      en_point<PROGS>(dim, nc, tab[tb.ow[g] + ig], tab + tb.ophi[g] + (size_t)ig * nc, tab + tb.odphi[g] + (size_t)ig * nc * dim, X, Sv,
                      PROGS && mode == EN_QP ? nullptr : Uv, pr, TT + ig * st);
  __syncthreads();
  if (active && lane == 0) {
    double r[2];
    en_element_sums(ng, dim, TT, r);
    T[e] = r[0];
    T[(size_t)nel + e] = r[1];
  }
}

// a vector of the call: the mesh's context and the family's size
int en_check_vec(const char* who, const char* name, fh_elem_mesh_t m, int fe, fh_vec_t v) {
  FH_REQUIRE(v->ctx == m->ctx, "%s: %s is a vector of another context than the mesh's", who, name);
  FH_REQUIRE(v->n_global == m->own[fe] && v->n_local == m->own[fe], "%s: %s has %d entries, the family has %d dofs on this mesh", who, name, v->n_global, m->own[fe]);
  return 0;
}
}  // namespace

extern "C" int fh_elem_mesh_error_norms(fh_elem_mesh_t m, int fe, int gauss_order, fh_vec_t sol, int mode, fh_expr_t exact, const fh_expr_t* gradient, fh_vec_t other,
                                        double norms[2], double* elem_l2, double* elem_h1) {
  FH_GUARD_BEGIN
  const char* who = "fh_elem_mesh_error_norms";
  FH_REQUIRE(m, "%s: mesh is null", who);
  FH_REQUIRE(sol, "%s: sol is null", who);
  FH_REQUIRE(norms, "%s: norms is null", who);
  EnHostProgs P;
  FH_TRY(en_check_options(who, m->dim, fe, mode, exact, gradient, other != nullptr, P));
  FH_TRY(en_check_vec(who, "sol", m, fe, sol));
  if (other) FH_TRY(en_check_vec(who, "other", m, fe, other));
  bool present[EM_G];
  for (int g = 0; g < EM_G; g++) present[g] = m->count[g] > 0;
  EeHostTabs H;
  FH_TRY(ee_tables(who, m->dim, fe, gauss_order, present, H));
  norms[0] = norms[1] = 0.0;
  if (!m->nel) return 0;
  const int L = H.ngmax <= 16 ? 16 : H.ngmax <= 32 ? 32 : 64, epg = 256 / L;
  const size_t lds = (size_t)epg * (H.ncmax * 5 + H.ngmax * (1 + m->dim)) * sizeof(double);
  FH_REQUIRE(lds <= 40 * 1024, "%s: %zu bytes of LDS per workgroup", who, lds);
  fh_ctx_t ctx = m->ctx;
  hipStream_t st = ctx->stream;
  const size_t nel = (size_t)m->nel, nch = (nel + EE_RC - 1) / EE_RC;
  double hs[2] = {0.0, 0.0};
  EmScratch B(who);
  double *d_tab = nullptr, *d_T = nullptr, *d_p0 = nullptr, *d_p1 = nullptr, *d_sums = nullptr, *d_consts = nullptr;
  int *d_code = nullptr, *d_cptr = nullptr, *d_kptr = nullptr;
  auto run = [&]() -> int {
    if (B.get(&d_tab, H.buf.size()) || B.get(&d_T, 2 * nel) || B.get(&d_p0, 2 * nch) || B.get(&d_p1, 2 * nch) || B.get(&d_sums, (size_t)2) ||
        B.get(&d_code, P.code.size()) || B.get(&d_cptr, P.cptr.size()) || B.get(&d_consts, P.consts.size()) || B.get(&d_kptr, P.kptr.size()))
      return 2;
    if (ctx->debug_poison) {      // every entry is written before it is read
      FH_CHECK_HIP(hipMemsetAsync(d_T, 0xFF, std::max<size_t>(2 * nel, 2) * sizeof(double), st));
      FH_CHECK_HIP(hipMemsetAsync(d_p0, 0xFF, std::max<size_t>(2 * nch, 2) * sizeof(double), st));
      FH_CHECK_HIP(hipMemsetAsync(d_p1, 0xFF, std::max<size_t>(2 * nch, 2) * sizeof(double), st));
      FH_CHECK_HIP(hipMemsetAsync(d_sums, 0xFF, 2 * sizeof(double), st));
    }
    FH_CHECK_HIP(hipMemcpyAsync(d_tab, H.buf.data(), H.buf.size() * sizeof(double), hipMemcpyHostToDevice, st));
    FH_CHECK_HIP(hipMemcpyAsync(d_cptr, P.cptr.data(), P.cptr.size() * sizeof(int), hipMemcpyHostToDevice, st));
    FH_CHECK_HIP(hipMemcpyAsync(d_kptr, P.kptr.data(), P.kptr.size() * sizeof(int), hipMemcpyHostToDevice, st));
    if (!P.code.empty()) FH_CHECK_HIP(hipMemcpyAsync(d_code, P.code.data(), P.code.size() * sizeof(int), hipMemcpyHostToDevice, st));
    if (!P.consts.empty()) FH_CHECK_HIP(hipMemcpyAsync(d_consts, P.consts.data(), P.consts.size() * sizeof(double), hipMemcpyHostToDevice, st));
    const EnProgs pr{d_code, d_cptr, d_consts, d_kptr};
    const dim3 grid(fh_div_up(m->nel, epg)), block(256);
#define EN_LAUNCH(LL, PP)                                                                                                                                        \
  hipLaunchKernelGGL((k_en_elements<LL, PP>), grid, block, lds, st, m->nel, m->dim, mode, H.t, H.ncmax, H.ngmax, d_tab, m->d_geom, m->d_ed, m->d_x, sol->d,      \
                     other ? other->d : nullptr, pr, d_T)
    if (mode == EN_VECTOR) {
      if (L == 16) EN_LAUNCH(16, false);
      else if (L == 32) EN_LAUNCH(32, false);
      else EN_LAUNCH(64, false);
    } else {
      if (L == 16) EN_LAUNCH(16, true);
      else if (L == 32) EN_LAUNCH(32, true);
      else EN_LAUNCH(64, true);
    }
#undef EN_LAUNCH
    FH_CHECK_HIP(hipGetLastError());
    ee_reduce(st, nel, 2, d_T, d_p0, d_p1, d_sums);
    FH_CHECK_HIP(hipGetLastError());
    FH_CHECK_HIP(hipMemcpyAsync(hs, d_sums, 2 * sizeof(double), hipMemcpyDeviceToHost, st));
    if (elem_l2) FH_CHECK_HIP(hipMemcpyAsync(elem_l2, d_T, nel * sizeof(double), hipMemcpyDeviceToHost, st));
    if (elem_h1) FH_CHECK_HIP(hipMemcpyAsync(elem_h1, d_T + nel, nel * sizeof(double), hipMemcpyDeviceToHost, st));
    return 0;
  };
  const int rc = run();
  const hipError_t he = hipStreamSynchronize(st);         // the work buffers are freed on return
  if (rc) return rc;
  FH_CHECK_HIP(he);
  norms[0] = sqrt(hs[0]);
  norms[1] = sqrt(hs[1]);
  return 0;
  FH_GUARD_END("fh_elem_mesh_error_norms")
}

extern "C" int fh_elem_error_norms_host(int dim, int nel, const int* elem_geom, const int* elem_dof, int nnode, const double* coords, int fe, int gauss_order,
                                        const double* sol, int mode, fh_expr_t exact, const fh_expr_t* gradient, const double* other, double norms[2],
                                        double* elem_l2, double* elem_h1) {
  FH_GUARD_BEGIN
  const char* who = "fh_elem_error_norms_host";
  FH_REQUIRE(nel >= 0 && nnode >= 0, "%s: negative size", who);
  FH_REQUIRE(dim == 2 || dim == 3, "%s: dim must be 2 or 3, not %d", who, dim);
  FH_REQUIRE(sol, "%s: sol is null", who);
  FH_REQUIRE(norms, "%s: norms is null", who);
  EnHostProgs P;
  FH_TRY(en_check_options(who, dim, fe, mode, exact, gradient, other != nullptr, P));
  FH_REQUIRE(nel == 0 || (elem_geom && elem_dof && coords), "%s: null argument", who);
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
  const EnProgs pr = P.view();
  const int st = 1 + dim;
  std::vector<double> l2((size_t)nel, 0.0), h1((size_t)nel, 0.0), TT((size_t)EE_MAXG * EN_MAXT);
  for (int e = 0; e < nel; e++) {
    const int g = elem_geom[e], nc = H.t.nc[g], ng = H.t.ng[g];
    const int* ed = elem_dof + (size_t)e * EM_W;
    double X[EM_W * 3], Sv[EM_W], Uv[EM_W], r[2];
    for (int n = 0; n < nc; n++) {
      for (int d = 0; d < 3; d++) X[n * 3 + d] = d < dim ? coords[(size_t)ed[n] * dim + d] : 0.0;
      Sv[n] = sol[ed[n]];
      Uv[n] = mode == EN_VECTOR ? other[ed[n]] : mode == EN_DOFS ? en_nodal(pr, X + n * 3) : 0.0;
    }
    for (int ig = 0; ig < ng; ig++)
      en_point(dim, nc, H.buf[H.t.ow[g] + ig], &H.buf[H.t.ophi[g] + (size_t)ig * nc], &H.buf[H.t.odphi[g] + (size_t)ig * nc * dim], X, Sv,
               mode == EN_QP ? nullptr : Uv, pr, &TT[(size_t)ig * st]);
    en_element_sums(ng, dim, TT.data(), r);
    l2[e] = r[0];
    h1[e] = r[1];
  }
  if (elem_l2) fh_copy_out(elem_l2, l2);
  if (elem_h1) fh_copy_out(elem_h1, h1);
  norms[0] = sqrt(nel ? ee_fixed_sum(l2) : 0.0);
  norms[1] = sqrt(nel ? ee_fixed_sum(h1) : 0.0);
  return 0;
  FH_GUARD_END("fh_elem_error_norms_host")
}
