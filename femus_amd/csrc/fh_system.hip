// A coupled system of m = 1 .. 4 variables of one family on the resident plan of the generic assembly (fh_generic.hip): equation k is
//   - sum_l div(A_kl grad u_l) + c_k = f_k,     A_kl = A_kl(x, U),  c_k = c_k(x, U, grad U),
// the Jacobian and residual of one Newton step of a NonLinearImplicitSystem with several variables stacked in one matrix (applications/000_tutorial/ex04, ex05):
//   RES_(k,i)      = sum_g [ f_k phi_i - sum_l A_kl (grad phi_i . grad u_l) - c_k phi_i ] w
//   KK_(k,i),(l,j) = sum_g [ A_kl (grad phi_i . grad phi_j) + (grad phi_i . W_kl) phi_j + phi_i ( C_kl phi_j + D_kl . grad phi_j ) ] w
//   W_kl = sum_p (dA_kp/du_l) grad u_p,   C_kl = dc_k/du_l,   D_kl = dc_k/d(grad u_l)
// Unknown (k, i) has the number k ndof + i (KKoffset order on one process).  The programs are over x, y, z, u0 .. u{m-1}, u0x, u0y, u0z, u1x, ...: u_k is
// variable 3 + k, d_d u_k variable 3 + m + 3 k + d.  A missing A_kk is 1, every other missing program is 0 and its term is left out (a uniform branch).
//
// The plan is the scalar object's, untouched: element tables, Pos, adj.  The matrix is Mat.block_system(S, m) of the object's own pattern S: row (k, i) starts
// at k m nnz_S + m rowptr_S[i], the entry for column (l, j) sits l len_S(i) + (Pos - rowptr_S[i]) further, so there is no second Pos.  New here:
//   work buffers  Kb of m^2 and Fb of m times the scalar size, block-major (block b = k m + l of an element entry at b nent + its scalar place), made at the
//                 first call with a given m (m = 1: the scalar buffers), counted in info(), freed with the object, 0xFF bytes under debug_poison
//   element pass  k_sys_elements: L lanes per element (the scalar body's width times 1 / 2 / 4 for m = 1 / 2 / 3 and 4, at most 64).  LDS of an element:
//                   X[nc][3] U[m][nc] | PV[gc][13 + 6 m + 8 m^2] | G[gc][nc][3]
//                 one PV block per Gauss point: JI[9] WG | state[3 + 4 m] | f[m] c[m] A[m^2] C[m^2] W[m^2][3] D[m^2][3].  Phases of a chunk, a barrier between:
//                   (A)  of fh_elembody.h: the inverse and det w head the point's PV block, x_g goes into the state
//                   (B)  lanes over (point, node): G_n = Jac^-1 dphi_n.  This and the kernel's prologue are the texts of eb_chunk_gradients and
//                        eb_prologue, kept in this file on purpose: as helpers they give these kernels another schedule and cost time
//                        (profiles/elembody_share_isa.md); a change to them there is made here too
//                   (C1) lanes over (point, variable): u_k, grad u_k into the state (nodes ascending)
//                   (C2) lanes over (point, task): the directory's tasks.  A simple task runs one program and stores its value; a W task runs the at most m
//                        programs dA_kp/du_l, p ascending, and stores W_kl.  The state is read from LDS
//                   (D)  for every block (k, l): lanes over the nc^2 entries with the scalar body's NPL accumulators; W_kl and D_kl are in LDS, so
//                        grad phi_i . W_kl and D_kl . grad phi_j are three multiply-adds inline and there are no per-(point, node) arrays.  A block's sum is
//                        carried across chunks in Kb (first chunk stores, later ones load, add, store: the same lane holds the same entry, points ascend), the
//                        residual of (k, i) likewise in Fb.  One summation order whatever the chunk, no atomics, the same bits from every call
//   row pass      k_sys_rows: lpr lanes per system row, m maxrow doubles of LDS per group, the scalar Pos / adj / rowptr_S
//   programs      all constants, then all code, then the directory (16 ints per task) in the object's program buffer: the directory is part of the code array
//                 gp_upload_program compares, so no other path's upload can leave a stale one behind
#include "fh_elembody.h"
#include "fh_expr_device.h"
#include "fh_system.h"
#include <algorithm>
#include <cstdio>

namespace {
constexpr int SY_MAXM = 4;
constexpr int SY_DIR = 16;                   // ints of a task: dest, kind (0: one program, 1: W_kl), -, -, then (code, ncode, kons) of up to four programs
struct SysMasks {
  unsigned A, W, C, D, f, c;                 // bit k m + l (f, c: bit k): the term is there
};
constexpr int sy_point_doubles(int m) { return 13 + 6 * m + 8 * m * m; }
constexpr size_t sy_elem_doubles(int m, int nc, int gc) { return (size_t)nc * (3 + m) + (size_t)gc * sy_point_doubles(m) + (size_t)gc * nc * 3; }
}  // namespace

// The element body.  Every thread of the workgroup calls this with the same m, ng, gcm, masks and ntask (workgroup barriers, uniform branches); a sub-group
// without an element passes active = false and touches nothing.  Kout + b kstride: block b of the element's nc x nc rows; Fout + k fstride: residual of variable k
template <int L, int NPL>
__device__ __forceinline__ void system_element_pass(bool active, int lane, int m, int nc, int ng, int gcm, int dim, const double* w, const double* phi,
                                                    const double* dphi, const int* dof_row, const double* coords, const double* sol, int ndof, const SysMasks& mk,
                                                    const int* dir, int ntask, const int* pcode, const double* pconst, double* lds, double* Kout, long long kstride,
                                                    double* Fout, long long fstride) {
  const int m2 = m * m, PS = sy_point_doubles(m);
  const int oST = 10, oF = 13 + 4 * m, oC = oF + m, oA = oC + m, oCu = oA + m2, oW = oCu + m2, oD = oW + 3 * m2;
  double* X = lds;                                   // [nc][3]
  double* U = X + nc * 3;                            // [m][nc]
  double* PV = U + m * nc;                           // [gcm][PS]
  double* G = PV + gcm * PS;                         // [gcm][nc][3]
  if (active && lane < nc) {
    const int dof = dof_row[lane];
    for (int d = 0; d < 3; d++) X[lane * 3 + d] = d < dim ? coords[(size_t)dof * dim + d] : 0.0;
    for (int k = 0; k < m; k++) U[k * nc + lane] = sol ? sol[(size_t)k * ndof + dof] : 0.0;
  }
  int ei[NPL], ej[NPL];
#pragma unroll
  for (int k = 0; k < NPL; k++) {
    const int e = lane + L * k;
    if (active && e < nc * nc) {
      ei[k] = e / nc;
      ej[k] = e - ei[k] * nc;
    } else {
      ei[k] = ej[k] = -1;
    }
  }
  __syncthreads();
  for (int g0 = 0; g0 < ng; g0 += gcm) {
    const int gc = min(gcm, ng - g0);
    const bool first = g0 == 0;
    if (active)
      for (int l = lane; l < gc; l += L) {             // (A)
        const int g = g0 + l;
        double* P = PV + l * PS;
        double xq[3] = {0, 0, 0};
        eb_point_geometry(X, dphi + (size_t)g * nc * dim, phi + (size_t)g * nc, w + g, nc, dim, P, P + 9, xq);
        for (int q = 0; q < 3; q++) P[oST + q] = xq[q];
      }
    __syncthreads();
    if (active)
      for (int t = lane; t < gc * nc; t += L) {        // (B)
        const int l = t / nc, n = t - l * nc;
        const double* dp = dphi + ((size_t)(g0 + l) * nc + n) * dim;
        const double* JI = PV + l * PS;
        for (int q = 0; q < 3; q++) {
          double sacc = 0.0;
          if (q < dim)
            for (int p = 0; p < dim; p++) sacc += JI[q * 3 + p] * dp[p];
          G[(l * nc + n) * 3 + q] = sacc;
        }
      }
    __syncthreads();
    if (active)
      for (int t = lane; t < gc * m; t += L) {         // (C1)
        const int l = t / m, k = t - l * m;
        double u = 0.0, gu[3] = {0, 0, 0};
        for (int n = 0; n < nc; n++) {
          const double un = U[k * nc + n];
          u += phi[(size_t)(g0 + l) * nc + n] * un;
          for (int q = 0; q < dim; q++) gu[q] += G[(l * nc + n) * 3 + q] * un;
        }
        double* st = PV + l * PS + oST;
        st[3 + k] = u;
        for (int q = 0; q < 3; q++) st[3 + m + 3 * k + q] = gu[q];
      }
    __syncthreads();
    if (active)
      for (int t = lane; t < gc * ntask; t += L) {     // (C2)
        const int l = t / ntask;
        const int* e = dir + (t - l * ntask) * SY_DIR;
        double* P = PV + l * PS;
        const double* st = P + oST;
        const bool isW = e[1] != 0;
        const int np = isW ? m : 1;                    // one call site of the evaluator for both kinds of task
        double v = 0.0, wv[3] = {0, 0, 0};
#pragma unroll 1
        for (int p = 0; p < np; p++)
          if (e[5 + 3 * p] >= 0) {
            v = fh_expr_device_eval(pcode + e[4 + 3 * p], e[5 + 3 * p], pconst + e[6 + 3 * p], st);
            if (isW)
              for (int q = 0; q < 3; q++) wv[q] += v * st[3 + m + 3 * p + q];
          }
        if (isW)
          for (int q = 0; q < 3; q++) P[e[0] + q] = wv[q];
        else
          P[e[0]] = v;
      }
    __syncthreads();
#pragma unroll 1
    for (int b = 0; b < m2; b++) {                     // (D)
      const bool hasA = (mk.A >> b) & 1, hasW = (mk.W >> b) & 1, hasC = (mk.C >> b) & 1, hasD = (mk.D >> b) & 1;
      double* Kb = Kout + (long long)b * kstride;
#pragma unroll
      for (int k = 0; k < NPL; k++)
        if (ei[k] >= 0) {
          const int i = ei[k], j = ej[k];
          double a = first ? 0.0 : Kb[lane + L * k];
          for (int l = 0; l < gc; l++) {
            const double* P = PV + l * PS;
            const double *gi = G + (l * nc + i) * 3, *gj = G + (l * nc + j) * 3;
            double val = 0.0;
            if (hasA) {
              double dot = 0.0;
              for (int q = 0; q < dim; q++) dot += gi[q] * gj[q];
              val = P[oA + b] * dot;
            }
            if (hasW) {
              double s = 0.0;
              for (int q = 0; q < dim; q++) s += gi[q] * P[oW + 3 * b + q];
              val += s * phi[(size_t)(g0 + l) * nc + j];
            }
            if (hasC || hasD) {
              double tt = hasC ? P[oCu + b] * phi[(size_t)(g0 + l) * nc + j] : 0.0;
              if (hasD)
                for (int q = 0; q < dim; q++) tt += P[oD + 3 * b + q] * gj[q];
              val += phi[(size_t)(g0 + l) * nc + i] * tt;
            }
            a += val * P[9];
          }
          Kb[lane + L * k] = a;
        }
    }
    if (active)
      for (int t = lane; t < m * nc; t += L) {         // the residual of (k, i)
        const int k = t / nc, i = t - k * nc;
        double F = first ? 0.0 : Fout[(long long)k * fstride + i];
        for (int l = 0; l < gc; l++) {
          const double* P = PV + l * PS;
          const double* gi = G + (l * nc + i) * 3;
          const double ph = phi[(size_t)(g0 + l) * nc + i];
          double r = (mk.f >> k) & 1 ? P[oF + k] * ph : 0.0;
          for (int v = 0; v < m; v++)
            if ((mk.A >> (k * m + v)) & 1) {
              double S = 0.0;
              for (int q = 0; q < dim; q++) S += gi[q] * P[oST + 3 + m + 3 * v + q];
              r -= P[oA + k * m + v] * S;
            }
          if ((mk.c >> k) & 1) r -= P[oC + k] * ph;
          F += r * P[9];
        }
        Fout[(long long)k * fstride + i] = F;
      }
    __syncthreads();
  }
}

// Element pass of the plan for a system.  L lanes per element, 256 / L elements per workgroup; TL: the shape's tables in LDS.  Block b of slot s at
// Kb[b kstride + s nc nc], the residual of variable k at Fb[k fstride + s nc]
template <int L, bool TL>
__global__ __launch_bounds__(GP_THREADS) void k_sys_elements(int nslot, int m, int nc, int ng, int gcm, int dim, const double* __restrict__ gw,
                                                             const double* __restrict__ gphi, const double* __restrict__ gdphi, const int* __restrict__ ed,
                                                             const double* __restrict__ coords, const double* __restrict__ sol, int ndof, SysMasks mk,
                                                             const int* __restrict__ dir, int ntask, const int* __restrict__ pcode,
                                                             const double* __restrict__ pconst, double* Kb, long long kstride, double* Fb, long long fstride) {
  extern __shared__ __attribute__((aligned(16))) double sys_smem[];
  constexpr int EPG = GP_THREADS / L;
  constexpr int NPL = gp_entries_per_lane(L);
  const int ntab = TL ? ng + ng * nc + ng * nc * dim : 0;
  const int per = (int)sy_elem_doubles(m, nc, gcm);
  const int sub = threadIdx.x / L, lane = threadIdx.x % L;
  const int slot = blockIdx.x * EPG + sub;
  const bool active = slot < nslot;              // tail sub-groups keep the barriers and touch nothing
  const double *w, *phi, *dphi;
  if (TL) {
    double* tw = sys_smem;
    double* tphi = tw + ng;
    double* tdphi = tphi + ng * nc;
    for (int t = threadIdx.x; t < ng; t += GP_THREADS) tw[t] = gw[t];
    for (int t = threadIdx.x; t < ng * nc; t += GP_THREADS) tphi[t] = gphi[t];
    for (int t = threadIdx.x; t < ng * nc * dim; t += GP_THREADS) tdphi[t] = gdphi[t];
    w = tw, phi = tphi, dphi = tdphi;
  } else {
    w = gw, phi = gphi, dphi = gdphi;
  }
  const int s = active ? slot : 0;               // an inactive sub-group forms no address beyond the buffers
  system_element_pass<L, NPL>(active, lane, m, nc, ng, gcm, dim, w, phi, dphi, ed + (size_t)s * nc, coords, sol, ndof, mk, dir, ntask, pcode, pconst,
                              sys_smem + ntab + (size_t)sub * per, Kb + (size_t)s * nc * nc, kstride, Fb + (size_t)s * nc, fstride);
}

// Row pass into block_system(S, m): lpr lanes (a power of two <= 64) per system row (k, i), the row's m len_S(i) sums in LDS (m maxrow doubles per group).
__global__ __launch_bounds__(GP_THREADS) void k_sys_rows(int ndof, int m, int lpr, int maxrow, GenRowShapes sh, const int* __restrict__ adj_ptr,
                                                         const int* __restrict__ adj, const double* __restrict__ Kb, long long kstride, const int* __restrict__ Pos,
                                                         const double* __restrict__ Fb, long long fstride, const int* __restrict__ rowptr, long long nnz,
                                                         double* __restrict__ val, double* __restrict__ res) {
  extern __shared__ __attribute__((aligned(16))) double sys_racc[];
  const int grp = threadIdx.x / lpr, t = threadIdx.x % lpr;
  const int R = blockIdx.x * (GP_THREADS / lpr) + grp;
  if (R >= m * ndof) return;                     // no workgroup barrier below
  const int k = R / ndof, r = R - k * ndof;
  double* acc = sys_racc + (size_t)grp * m * maxrow;
  const int rs = rowptr[r], n = rowptr[r + 1] - rs;
  for (int q = t; q < m * n; q += lpr) acc[q] = 0.0;
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
  double racc = 0.0;
  for (int a = adj_ptr[r], ae = adj_ptr[r + 1]; a < ae; a++) {
    const int erow = adj[a];
    const int s = erow >= sh.row_base[2] ? 2 : erow >= sh.row_base[1] ? 1 : 0;
    const int nc = sh.nc[s];
    const long long off = sh.kb_base[s] + (long long)(erow - sh.row_base[s]) * nc;
    if (t == 0) racc += Fb[(long long)k * fstride + erow];
    for (int q = t; q < m * nc; q += lpr) {
      const int l = q / nc, j = q - l * nc;
      acc[l * n + Pos[off + j] - rs] += Kb[(long long)(k * m + l) * kstride + off + j];
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
  }
  double* out = val + (long long)k * m * nnz + (long long)m * rs;
  for (int q = t; q < m * n; q += lpr) out[q] = acc[q];
  if (t == 0) res[R] = racc;
}

namespace {
struct SysCall {
  int m, ntask;
  SysMasks mk;
  const int *dir, *pcode;
  const double *pconst, *sol;
  double *Kb, *Fb;
};
}  // namespace

static void sy_launch(fh_generic_assembler_t as, int k, const SysCall& c) {
  const GenBodyPlan& P = as->sys[c.m];
  gp_dispatch(P, k, [&](auto lanes, auto staged) {
    constexpr int L = decltype(lanes)::value;
    hipLaunchKernelGGL((k_sys_elements<L, decltype(staged)::value>), dim3(fh_div_up(as->nslot[k], GP_THREADS / L)), dim3(GP_THREADS), P.lds[k], as->ctx->stream,
                       as->nslot[k], c.m, as->nc[k], as->ng[k], P.gcm[k], as->dim, as->d_w[k], as->d_phi[k], as->d_dphi[k], as->d_ed[k], as->d_coords, c.sol, as->ndof, c.mk,
                       c.dir, c.ntask, c.pcode, c.pconst, c.Kb + as->rows.kb_base[k], (long long)as->nent, c.Fb + as->rows.row_base[k], (long long)as->nrows);
  });
}

// The row pass's lanes and the work buffers of m variables, for assemble_system and assemble_system_transient alike (fh_system.h): made once per m, by
// whichever of the two comes first
int sy_work_buffers(const char* who, fh_generic_assembler_t as, int m) {
  if (as->sys_lpr[m] && as->d_sysK[m] && as->d_sysF[m]) return 0;
  int lpr = as->lpr;
  while (lpr < 64 && (size_t)(GP_THREADS / lpr) * m * as->maxrow * sizeof(double) > GP_LDS_BUDGET) lpr *= 2;
  FH_REQUIRE((size_t)(GP_THREADS / lpr) * m * as->maxrow * sizeof(double) <= GP_LDS_BUDGET, "%s: %d rows of %d entries are longer than the row pass holds", who, m,
             as->maxrow);
  if (m > 1) {
    const size_t kb = (size_t)m * m * as->nent * sizeof(double), fb = (size_t)m * as->nrows * sizeof(double);
    if (!as->d_sysK[m]) as->d_sysK[m] = (double*)gp_alloc(as, kb);
    if (as->d_sysK[m] && !as->d_sysF[m]) as->d_sysF[m] = (double*)gp_alloc(as, fb);
    if (!as->d_sysK[m] || !as->d_sysF[m]) {
      hipGetLastError();
      fh_set_error("%s: out of device memory (%.2f GB of element rows of %d variables)", who, (double)kb / 1e9, m);
      return 2;
    }
    if (as->ctx->debug_poison) {   // tests: the row pass must read nothing the element pass has not written
      hipMemsetAsync(as->d_sysK[m], 0xFF, kb, as->ctx->stream);
      hipMemsetAsync(as->d_sysF[m], 0xFF, fb, as->ctx->stream);
    }
  } else {
    as->d_sysK[1] = as->d_Kb, as->d_sysF[1] = as->d_Fb;
  }
  as->sys_lpr[m] = lpr;
  as->sys_row_lds[m] = (size_t)(GP_THREADS / lpr) * m * as->maxrow * sizeof(double);
  return 0;
}

// first assemble_system with this m: lanes (the scalar body's times 1 / 2 / 4, at most 64), Gauss chunk, table staging and LDS per shape, then the row pass and
// the work buffers -- every refusal before the buffers are allocated; the plan is kept only when all of it succeeds
static int sy_plan(const char* who, fh_generic_assembler_t as, int m) {
  int lanes[3] = {64, 64, 64};
  for (int k = 0; k < as->ns; k++) lanes[k] = std::min(64, as->poisson.lanes[k] * (m == 1 ? 1 : m == 2 ? 2 : 4));
  char body[64];
  snprintf(body, sizeof body, " with the element body of %d variables", m);
  GenBodyPlan plan;
  FH_TRY(gp_plan_body(who, as, lanes, [m](int nc, int gc) { return sy_elem_doubles(m, nc, gc); }, false, true, "a block", body, plan));
  FH_TRY(sy_work_buffers(who, as, m));
  as->sys[m] = plan;
  return 0;
}

// every refusal a form can earn on this object, then all constants, all code and the directory of its tasks
static int sy_gather(const char* who, fh_generic_assembler_t as, const fh_system_form_t* form, SysMasks& mk, int& ntask, std::vector<int>& code,
                     std::vector<int>& dir, std::vector<double>& consts) {
  const int m = form->m, dim = as->dim, m2 = m * m, max_vars = 3 + 4 * m;
  for (int k = 0; k < m; k++)
    for (int l = 0; l < m; l++)
      for (int d = dim; d < 3; d++) FH_REQUIRE(!form->c_g[k][l][d], "%s: c_g[%d][%d][%d] given on a mesh of dimension %d", who, k, l, d, dim);
  const int oF = 13 + 4 * m, oC = oF + m, oA = oC + m, oCu = oA + m2, oW = oCu + m2, oD = oW + 3 * m2;
  std::vector<int> c1;
  std::vector<double> k1;
  code.clear(), dir.clear(), consts.clear();
  mk = SysMasks{0, 0, 0, 0, 0, 0};
  char name[48];
  int ref[3];
  auto fetch = [&](fh_expr_t e) -> int {             // (code, ncode, kons) of one program into ref
    int nv = 0;
    FH_TRY(fh_expr_nvars(e, &nv));
    FH_REQUIRE(nv <= max_vars, "%s: the program %s has %d variables, at most %d (x, y, z, u0 .. u%d and their gradients) are served", who, name, nv, max_vars, m - 1);
    FH_TRY(fh_expr_fetch(e, name, max_vars, c1, k1));
    ref[0] = (int)code.size(), ref[1] = (int)c1.size(), ref[2] = (int)consts.size();
    code.insert(code.end(), c1.begin(), c1.end());
    consts.insert(consts.end(), k1.begin(), k1.end());
    return 0;
  };
  auto constant = [&](double v) {                     // a one-word program: the constant v
    ref[0] = (int)code.size(), ref[1] = 1, ref[2] = (int)consts.size();
    code.push_back(FHX_CONST);
    consts.push_back(v);
  };
  auto task = [&](int dest, int kind) {
    const size_t at = dir.size();
    dir.resize(at + SY_DIR, 0);
    dir[at] = dest, dir[at + 1] = kind;
    for (int p = 0; p < 4; p++) dir[at + 5 + 3 * p] = -1;
    return at;
  };
  auto simple = [&](int dest) {
    const size_t at = task(dest, 0);
    for (int q = 0; q < 3; q++) dir[at + 4 + q] = ref[q];
  };
  for (int k = 0; k < m; k++) {
    if (form->f[k]) {
      snprintf(name, sizeof name, "f[%d]", k);
      FH_TRY(fetch(form->f[k]));
      simple(oF + k);
      mk.f |= 1u << k;
    }
    if (form->c[k]) {
      snprintf(name, sizeof name, "c[%d]", k);
      FH_TRY(fetch(form->c[k]));
      simple(oC + k);
      mk.c |= 1u << k;
    }
    for (int l = 0; l < m; l++) {
      const int b = k * m + l;
      if (form->A[k][l] || k == l) {
        snprintf(name, sizeof name, "A[%d][%d]", k, l);
        if (form->A[k][l]) FH_TRY(fetch(form->A[k][l]));
        else constant(1.0);
        simple(oA + b);
        mk.A |= 1u << b;
      }
      if (form->c_u[k][l]) {
        snprintf(name, sizeof name, "c_u[%d][%d]", k, l);
        FH_TRY(fetch(form->c_u[k][l]));
        simple(oCu + b);
        mk.C |= 1u << b;
      }
      bool anyD = false, anyW = false;
      for (int d = 0; d < dim; d++) anyD = anyD || form->c_g[k][l][d];
      for (int p = 0; p < m; p++) anyW = anyW || form->A_u[k][p][l];
      if (anyD) {
        for (int d = 0; d < 3; d++) {                 // all three: phase (D) reads the first dim, the rest is never NaN from a poisoned start
          snprintf(name, sizeof name, "c_g[%d][%d][%d]", k, l, d);
          if (d < dim && form->c_g[k][l][d]) FH_TRY(fetch(form->c_g[k][l][d]));
          else constant(0.0);
          simple(oD + 3 * b + d);
        }
        mk.D |= 1u << b;
      }
      if (anyW) {
        const size_t at = task(oW + 3 * b, 1);
        for (int p = 0; p < m; p++)
          if (form->A_u[k][p][l]) {
            snprintf(name, sizeof name, "A_u[%d][%d][%d]", k, p, l);
            FH_TRY(fetch(form->A_u[k][p][l]));
            for (int q = 0; q < 3; q++) dir[at + 4 + 3 * p + q] = ref[q];
          }
        mk.W |= 1u << b;
      }
    }
  }
  ntask = (int)(dir.size() / SY_DIR);
  return 0;
}

extern "C" int fh_generic_assembler_assemble_system(fh_generic_assembler_t as, fh_vec_t sol, const fh_system_form_t* form, fh_mat_t KK, fh_vec_t RES) {
  FH_GUARD_BEGIN
  const char* who = "fh_generic_assembler_assemble_system";
  // ---- every refusal first: nothing is enqueued before the last of them ----
  FH_REQUIRE(as && RES, "%s: null argument", who);
  FH_REQUIRE(form, "%s: null form", who);
  const int m = form->m;
  FH_REQUIRE(m >= 1 && m <= SY_MAXM, "%s: %d variables, 1 .. %d are served", who, m, SY_MAXM);
  fh_mat_t S = fh_mat_alive(as->mat_uid);
  FH_REQUIRE(S != nullptr, "%s: the matrix this object was created on has been destroyed", who);
  FH_REQUIRE(KK != nullptr, "%s: null matrix", who);
  FH_REQUIRE(KK->m == m * as->ndof && KK->n == m * as->ndof && (long long)KK->nnz == (long long)m * m * as->mat_nnz,
             "%s: not the block system of %d variables on the matrix this object was created on (%d x %d, %d non-zeros; %d x %d, %lld are expected)", who, m, KK->m,
             KK->n, KK->nnz, m * as->ndof, m * as->ndof, (long long)m * m * as->mat_nnz);
  FH_REQUIRE(RES->n_local >= m * as->ndof && (!sol || sol->n_local >= m * as->ndof), "%s: size mismatch", who);
  SysCall c;
  std::vector<int> code, dir;
  std::vector<double> consts;
  FH_TRY(sy_gather(who, as, form, c.mk, c.ntask, code, dir, consts));
  if (!as->sys[m].ready) FH_TRY(sy_plan(who, as, m));
  const size_t ncode = code.size();
  code.insert(code.end(), dir.begin(), dir.end());       // the directory travels, and is compared, as part of the code array
  FH_TRY(gp_upload_program(who, as, code, consts));
  c.m = m;
  c.pconst = (const double*)as->d_prog;
  c.pcode = (const int*)(as->d_prog + as->consts.size() * sizeof(double));
  c.dir = c.pcode + ncode;
  c.sol = sol ? sol->d : nullptr;
  c.Kb = as->d_sysK[m], c.Fb = as->d_sysF[m];
  for (int k = 0; k < as->ns; k++)
    if (as->nslot[k]) sy_launch(as, k, c);
  const int lpr = as->sys_lpr[m];
  hipLaunchKernelGGL(k_sys_rows, dim3(fh_div_up((int64_t)m * as->ndof, GP_THREADS / lpr)), dim3(GP_THREADS), as->sys_row_lds[m], as->ctx->stream, as->ndof, m, lpr,
                     as->maxrow, as->rows, as->d_adj_ptr, as->d_adj, c.Kb, (long long)as->nent, as->d_Pos, c.Fb, (long long)as->nrows, S->d_rowptr,
                     (long long)as->mat_nnz, KK->d_val, RES->d);
  const bool ok = hipGetLastError() == hipSuccess;
  fh_mat_values_written(KK);
  FH_REQUIRE(ok, "%s: launch failed", who);
  return 0;
  FH_GUARD_END("fh_generic_assembler_assemble_system")
}

extern "C" int fh_generic_assembler_system_chunks(fh_generic_assembler_t as, int m, int gauss_chunk[3], int lanes[3]) {
  FH_REQUIRE(as && gauss_chunk && lanes && m >= 1 && m <= SY_MAXM, "fh_generic_assembler_system_chunks: null argument, or a number of variables outside 1 .. 4");
  gp_read_plan(as, as->sys[m], gauss_chunk, lanes);
  return 0;
}
