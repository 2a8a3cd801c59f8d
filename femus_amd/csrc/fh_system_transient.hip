// One Newton iteration of one theta-step of a coupled system of m = 1 .. 4 variables of one family on the resident plan of the generic assembly
// (fh_generic.hip): equation k is
//   sum_l M_kl d_t u_l - sum_l div(A_kl grad u_l) + c_k = f_k,     M a constant m x m matrix,  A_kl = A_kl(x, U, t),  c_k = c_k(x, U, grad U, t),
// a TransientNonlinearImplicitSystem with several variables stacked in one matrix (src/08_equations/01_time_dependent/TransientSystem.cpp:62-113 is written for
// any number of variables).  With S and J the residual and the Jacobian of fh_system.hip, scaled by dt as fh_transient.hip scales its step:
//   RES_(k,i)      = - sum_g w sum_l M_kl (u_l - uo_l) phi_i  +  dt th_k S_(k,i)(U, time)  +  dt (1 - th_k) S_(k,i)(Uo, time - dt)
//   KK_(k,i),(l,j) = sum_g w M_kl phi_i phi_j  +  dt th_k J_(k,i),(l,j)(U, time)
// th_k = theta for an equation whose row of M has a non-zero entry, and 1 for an ALGEBRAIC equation (row k of M entirely zero): a constraint holds at the new
// time, a theta-mix of it at two times would let it drift.  The Jacobian is the exact one, with the factor th_k.  The programs are those of fh_system_form_t over
// one variable more, the time as the last: x, y, z, u0 .., u0x, u0y, u0z, u1x, .., t (variable 3 + 4 m).  time, dt, theta, M and the th_k are kernel arguments
// and never part of the program buffer: a step with a new time uploads nothing.  Where no th_k is below 1 nothing is evaluated at the old state, where none is
// above 0 nothing at the new one and KK = kron(M, mass matrix): uniform branches, as for the missing terms.
//
// The plan, the work buffers Kb / Fb of m^2 / m times the scalar size and the row pass k_sys_rows are the system body's (fh_system.h: the buffers are made by
// whichever of the two is called first with that m).  The element body is system_element_pass with the old state beside the new one, on the same L lanes per
// element, with a Gauss chunk, table staging and LDS of its own (the object's systr[m] plan).  LDS of an element:
//   X[nc][3] U[m][nc] Uo[m][nc] MM[16] SN[4] SO[4] | PV[gc][18 + 13 m + 9 m^2] | G[gc][nc][3]
// (MM = M, SN = dt th_k, SO = dt (1 - th_k): read by run-time indices, so they are taken out of the kernel arguments once).  One PV block per Gauss point:
//   JI[9] WG | state[4 + 4 m] | f[m] c[m] A[m^2] C[m^2] W[m^2][3] D[m^2][3] | old state[4 + 4 m] | UD[m] = u - uo | fo[m] co[m] Ao[m^2]
// Phases of a chunk, a barrier between:
//   (A)  eb_point_geometry: the inverse and det w head the point's block, x_g goes into both states, time and time - dt behind them
//   (B)  lanes over (point, node): G_n = Jac^-1 dphi_n
//   (C1) lanes over (point, variable): u_k, grad u_k, uo_k, grad uo_k (nodes ascending) into the states, u_k - uo_k into UD
//   (C2) lanes over (point, task): the directory's tasks.  A task names its equation and the state it reads; one of an equation with th_k == 0 at the new
//        state, or with th_k == 1 at the old one, is skipped and its place never read.  Every value is stored times dt th_k (old: dt (1 - th_k)), once per
//        point, so that (D) and the residual lanes add the mass term and nothing else
//   (D)  for every block (k, l): lanes over the nc^2 entries, acc += (M_kl phi_i phi_j + the system body's terms) WG; the sum is carried across chunks in Kb as
//        there.  The residual of (k, i): F += (-(sum_l M_kl UD_l) phi_i + new part + old part) WG, carried in Fb
// Every sum has one order whatever the chunk, there is no atomic, a repeated call gives the same bits.  Every entry of Kb and Fb of an active element is
// written; tail sub-groups keep the barriers and touch nothing.
#include "fh_elembody.h"
#include "fh_expr_device.h"
#include "fh_system.h"
#include <algorithm>
#include <cmath>
#include <cstdio>

namespace {
constexpr int ST_MAXM = 4;
constexpr int ST_DIR = 16;                   // ints of a task: dest, kind (0: one program, 1: W_kl), state (0: new, 1: old), equation, then (code, ncode, kons) x 4
constexpr int ST_STEP = 24;                  // MM[16] SN[4] SO[4]
struct SysTrMasks {
  unsigned A, W, C, D, f, c;                 // bit k m + l (f, c: bit k): the term is there and its equation has th_k > 0
  unsigned Ao, fo, co;                       // the same at the old state: the term is there and its equation has th_k < 1
  unsigned newEq, oldEq;                     // bit k: th_k > 0, th_k < 1
};
struct SysTrStep {
  double M[16], sn[4], so[4];                // M row-major with stride m, dt th_k, dt (1 - th_k)
  double time, time_old;
};
constexpr int st_point_doubles(int m) { return 18 + 13 * m + 9 * m * m; }
constexpr size_t st_elem_doubles(int m, int nc, int gc) {
  return (size_t)nc * (3 + 2 * m) + ST_STEP + (size_t)gc * st_point_doubles(m) + (size_t)gc * nc * 3;
}
}  // namespace

// The element body.  Every thread of the workgroup calls this with the same m, ng, gcm, masks, step and ntask (workgroup barriers, uniform branches); a
// sub-group without an element passes active = false and touches nothing.  Kout + b kstride: block b of the element's nc x nc rows; Fout + k fstride: residual
// of variable k
template <int L, int NPL>
__device__ __forceinline__ void system_transient_element_pass(bool active, int lane, int m, int nc, int ng, int gcm, int dim, const double* w, const double* phi,
                                                              const double* dphi, const int* dof_row, const double* coords, const double* sol,
                                                              const double* sol_old, int ndof, const SysTrMasks& mk, const SysTrStep& sp, const int* dir, int ntask,
                                                              const int* pcode, const double* pconst, double* lds, double* Kout, long long kstride, double* Fout,
                                                              long long fstride) {
  const int m2 = m * m, PS = st_point_doubles(m), NST = 4 + 4 * m;
  const int oST = 10, oF = oST + NST, oC = oF + m, oA = oC + m, oCu = oA + m2, oW = oCu + m2, oD = oW + 3 * m2;
  const int oSO = oD + 3 * m2, oUD = oSO + NST, oFo = oUD + m, oCo = oFo + m, oAo = oCo + m;
  double* X = lds;                                   // [nc][3]
  double* U = X + nc * 3;                            // [m][nc]
  double* Uo = U + m * nc;                           // [m][nc]
  double* MM = Uo + m * nc;                          // [16]
  double* SN = MM + 16;                              // [4]
  double* SO = SN + 4;                               // [4]
  double* PV = SO + 4;                               // [gcm][PS]
  double* G = PV + gcm * PS;                         // [gcm][nc][3]
  if (active && lane < nc) {
    const int dof = dof_row[lane];
    for (int d = 0; d < 3; d++) X[lane * 3 + d] = d < dim ? coords[(size_t)dof * dim + d] : 0.0;
    for (int k = 0; k < m; k++) {
      U[k * nc + lane] = sol ? sol[(size_t)k * ndof + dof] : 0.0;
      Uo[k * nc + lane] = sol_old[(size_t)k * ndof + dof];
    }
  }
  if (active && lane == 0) {
#pragma unroll
    for (int t = 0; t < 16; t++) MM[t] = sp.M[t];
#pragma unroll
    for (int t = 0; t < 4; t++) SN[t] = sp.sn[t], SO[t] = sp.so[t];
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
        for (int q = 0; q < 3; q++) P[oST + q] = xq[q], P[oSO + q] = xq[q];
        P[oST + NST - 1] = sp.time;
        P[oSO + NST - 1] = sp.time_old;
      }
    __syncthreads();
    if (active) eb_chunk_gradients<L, true>(lane, g0, gc, nc, nc, dim, dphi, PV, PS, G);      // (B)
    __syncthreads();
    if (active)
      for (int t = lane; t < gc * m; t += L) {         // (C1)
        const int l = t / m, k = t - l * m;
        double u = 0.0, uo = 0.0, gu[3] = {0, 0, 0}, go[3] = {0, 0, 0};
        for (int n = 0; n < nc; n++) {
          const double un = U[k * nc + n], on = Uo[k * nc + n], ph = phi[(size_t)(g0 + l) * nc + n];
          u += ph * un;
          uo += ph * on;
          for (int q = 0; q < dim; q++) {
            gu[q] += G[(l * nc + n) * 3 + q] * un;
            go[q] += G[(l * nc + n) * 3 + q] * on;
          }
        }
        double* P = PV + l * PS;
        P[oST + 3 + k] = u;
        P[oSO + 3 + k] = uo;
        P[oUD + k] = u - uo;
        for (int q = 0; q < 3; q++) P[oST + 3 + m + 3 * k + q] = gu[q], P[oSO + 3 + m + 3 * k + q] = go[q];
      }
    __syncthreads();
    if (active)
      for (int t = lane; t < gc * ntask; t += L) {     // (C2)
        const int l = t / ntask;
        const int* e = dir + (t - l * ntask) * ST_DIR;
        const bool old = e[2] != 0;
        if (!(((old ? mk.oldEq : mk.newEq) >> e[3]) & 1)) continue;      // no lane waits at a barrier inside this loop
        double* P = PV + l * PS;
        const double* st = P + (old ? oSO : oST);
        const double sc = old ? SO[e[3]] : SN[e[3]];
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
          for (int q = 0; q < 3; q++) P[e[0] + q] = sc * wv[q];
        else
          P[e[0]] = sc * v;
      }
    __syncthreads();
#pragma unroll 1
    for (int b = 0; b < m2; b++) {                     // (D)
      const bool hasA = (mk.A >> b) & 1, hasW = (mk.W >> b) & 1, hasC = (mk.C >> b) & 1, hasD = (mk.D >> b) & 1;
      double* Kb = Kout + (long long)b * kstride;
      const double Mb = active ? MM[b] : 0.0;
#pragma unroll
      for (int k = 0; k < NPL; k++)
        if (ei[k] >= 0) {
          const int i = ei[k], j = ej[k];
          double a = first ? 0.0 : Kb[lane + L * k];
          for (int l = 0; l < gc; l++) {
            const double* P = PV + l * PS;
            const double *gi = G + (l * nc + i) * 3, *gj = G + (l * nc + j) * 3;
            const double pi = phi[(size_t)(g0 + l) * nc + i], pj = phi[(size_t)(g0 + l) * nc + j];
            double val = 0.0;
            if (hasA) {
              double dot = 0.0;
              for (int q = 0; q < dim; q++) dot += gi[q] * gj[q];
              val = P[oA + b] * dot;
            }
            if (hasW) {
              double s = 0.0;
              for (int q = 0; q < dim; q++) s += gi[q] * P[oW + 3 * b + q];
              val += s * pj;
            }
            if (hasC || hasD) {
              double tt = hasC ? P[oCu + b] * pj : 0.0;
              if (hasD)
                for (int q = 0; q < dim; q++) tt += P[oD + 3 * b + q] * gj[q];
              val += pi * tt;
            }
            a += (Mb * (pi * pj) + val) * P[9];
          }
          Kb[lane + L * k] = a;
        }
    }
    if (active)
      for (int t = lane; t < m * nc; t += L) {         // the residual of (k, i)
        const int k = t / nc, i = t - k * nc;
        const bool isNew = (mk.newEq >> k) & 1, isOld = (mk.oldEq >> k) & 1;
        double F = first ? 0.0 : Fout[(long long)k * fstride + i];
        for (int l = 0; l < gc; l++) {
          const double* P = PV + l * PS;
          const double* gi = G + (l * nc + i) * 3;
          const double ph = phi[(size_t)(g0 + l) * nc + i];
          double mu = 0.0;
          for (int v = 0; v < m; v++) mu += MM[k * m + v] * P[oUD + v];
          double val = -mu * ph;
          if (isNew) {
            double r = (mk.f >> k) & 1 ? P[oF + k] * ph : 0.0;
            for (int v = 0; v < m; v++)
              if ((mk.A >> (k * m + v)) & 1) {
                double S = 0.0;
                for (int q = 0; q < dim; q++) S += gi[q] * P[oST + 3 + m + 3 * v + q];
                r -= P[oA + k * m + v] * S;
              }
            if ((mk.c >> k) & 1) r -= P[oC + k] * ph;
            val += r;
          }
          if (isOld) {
            double r = (mk.fo >> k) & 1 ? P[oFo + k] * ph : 0.0;
            for (int v = 0; v < m; v++)
              if ((mk.Ao >> (k * m + v)) & 1) {
                double S = 0.0;
                for (int q = 0; q < dim; q++) S += gi[q] * P[oSO + 3 + m + 3 * v + q];
                r -= P[oAo + k * m + v] * S;
              }
            if ((mk.co >> k) & 1) r -= P[oCo + k] * ph;
            val += r;
          }
          F += val * P[9];
        }
        Fout[(long long)k * fstride + i] = F;
      }
    __syncthreads();
  }
}

// Element pass of the plan for one theta-step of a system.  L lanes per element, 256 / L elements per workgroup; TL: the shape's tables in LDS.  Block b of
// slot s at Kb[b kstride + s nc nc], the residual of variable k at Fb[k fstride + s nc]
template <int L, bool TL>
__global__ __launch_bounds__(GP_THREADS) void k_sys_transient(int nslot, int m, int nc, int ng, int gcm, int dim, const double* __restrict__ gw,
                                                              const double* __restrict__ gphi, const double* __restrict__ gdphi, const int* __restrict__ ed,
                                                              const double* __restrict__ coords, const double* __restrict__ sol,
                                                              const double* __restrict__ sol_old, int ndof, SysTrMasks mk, SysTrStep sp,
                                                              const int* __restrict__ dir, int ntask, const int* __restrict__ pcode,
                                                              const double* __restrict__ pconst, double* Kb, long long kstride, double* Fb, long long fstride) {
  extern __shared__ __attribute__((aligned(16))) double systr_smem[];
  const EbGroup g = eb_prologue<L, TL>(systr_smem, nslot, nc, ng, dim, (int)st_elem_doubles(m, nc, gcm), gw, gphi, gdphi);
  system_transient_element_pass<L, gp_entries_per_lane(L)>(g.active, g.lane, m, nc, ng, gcm, dim, g.w, g.phi, g.dphi, ed + (size_t)g.slot * nc, coords, sol, sol_old,
                                                           ndof, mk, sp, dir, ntask, pcode, pconst, g.lds, Kb + (size_t)g.slot * nc * nc, kstride,
                                                           Fb + (size_t)g.slot * nc, fstride);
}

namespace {
struct SysTrCall {
  int m, ntask;
  SysTrMasks mk;
  SysTrStep sp;
  const int *dir, *pcode;
  const double *pconst, *sol, *sol_old;
  double *Kb, *Fb;
};
}  // namespace

static void st_launch(fh_generic_assembler_t as, int k, const SysTrCall& c) {
  const GenBodyPlan& P = as->systr[c.m];
  gp_dispatch(P, k, [&](auto lanes, auto staged) {
    constexpr int L = decltype(lanes)::value;
    hipLaunchKernelGGL((k_sys_transient<L, decltype(staged)::value>), dim3(fh_div_up(as->nslot[k], GP_THREADS / L)), dim3(GP_THREADS), P.lds[k], as->ctx->stream,
                       as->nslot[k], c.m, as->nc[k], as->ng[k], P.gcm[k], as->dim, as->d_w[k], as->d_phi[k], as->d_dphi[k], as->d_ed[k], as->d_coords, c.sol, c.sol_old,
                       as->ndof, c.mk, c.sp, c.dir, c.ntask, c.pcode, c.pconst, c.Kb + as->rows.kb_base[k], (long long)as->nent, c.Fb + as->rows.row_base[k],
                       (long long)as->nrows);
  });
}

// first assemble_system_transient with this m: the system body's lanes, this body's Gauss chunk, table staging and LDS per shape, then the row pass and the work
// buffers the two bodies share -- every refusal before anything is allocated; the plan is kept only when all of it succeeds
static int st_plan(const char* who, fh_generic_assembler_t as, int m) {
  int lanes[3] = {64, 64, 64};
  for (int k = 0; k < as->ns; k++) lanes[k] = std::min(64, as->poisson.lanes[k] * (m == 1 ? 1 : m == 2 ? 2 : 4));
  char body[80];
  snprintf(body, sizeof body, " with the transient element body of %d variables", m);
  GenBodyPlan plan;
  FH_TRY(gp_plan_body(who, as, lanes, [m](int nc, int gc) { return st_elem_doubles(m, nc, gc); }, false, true, "a block", body, plan));
  FH_TRY(sy_work_buffers(who, as, m));
  as->systr[m] = plan;
  return 0;
}

// every refusal a form can earn on this object, then all constants, all code and the directory of its tasks: those of assemble_system at the new state, and
// f_k, c_k and A_kl once more at the old one (the same programs: no code is stored twice).  The masks say which terms are there; the caller takes out the
// equations its th_k leave out
static int st_gather(const char* who, fh_generic_assembler_t as, const fh_system_form_t* form, SysTrMasks& mk, int& ntask, std::vector<int>& code,
                     std::vector<int>& dir, std::vector<double>& consts) {
  const int m = form->m, dim = as->dim, m2 = m * m, max_vars = 4 + 4 * m, NST = 4 + 4 * m;
  for (int k = 0; k < m; k++)
    for (int l = 0; l < m; l++)
      for (int d = dim; d < 3; d++) FH_REQUIRE(!form->c_g[k][l][d], "%s: c_g[%d][%d][%d] given on a mesh of dimension %d", who, k, l, d, dim);
  const int oF = 10 + NST, oC = oF + m, oA = oC + m, oCu = oA + m2, oW = oCu + m2, oD = oW + 3 * m2;
  const int oSO = oD + 3 * m2, oUD = oSO + NST, oFo = oUD + m, oCo = oFo + m, oAo = oCo + m;
  std::vector<int> c1;
  std::vector<double> k1;
  code.clear(), dir.clear(), consts.clear();
  mk = SysTrMasks{0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  char name[48];
  int ref[3];
  auto fetch = [&](fh_expr_t e) -> int {             // (code, ncode, kons) of one program into ref
    int nv = 0;
    FH_TRY(fh_expr_nvars(e, &nv));
    FH_REQUIRE(nv <= max_vars, "%s: the program %s has %d variables, at most %d (x, y, z, u0 .. u%d, their gradients and t) are served", who, name, nv, max_vars,
               m - 1);
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
  auto task = [&](int dest, int kind, int old, int eq) {
    const size_t at = dir.size();
    dir.resize(at + ST_DIR, 0);
    dir[at] = dest, dir[at + 1] = kind, dir[at + 2] = old, dir[at + 3] = eq;
    for (int p = 0; p < 4; p++) dir[at + 5 + 3 * p] = -1;
    return at;
  };
  auto simple = [&](int dest, int old, int eq) {
    const size_t at = task(dest, 0, old, eq);
    for (int q = 0; q < 3; q++) dir[at + 4 + q] = ref[q];
  };
  for (int k = 0; k < m; k++) {
    if (form->f[k]) {
      snprintf(name, sizeof name, "f[%d]", k);
      FH_TRY(fetch(form->f[k]));
      simple(oF + k, 0, k);
      simple(oFo + k, 1, k);
      mk.f |= 1u << k;
    }
    if (form->c[k]) {
      snprintf(name, sizeof name, "c[%d]", k);
      FH_TRY(fetch(form->c[k]));
      simple(oC + k, 0, k);
      simple(oCo + k, 1, k);
      mk.c |= 1u << k;
    }
    for (int l = 0; l < m; l++) {
      const int b = k * m + l;
      if (form->A[k][l] || k == l) {
        snprintf(name, sizeof name, "A[%d][%d]", k, l);
        if (form->A[k][l]) FH_TRY(fetch(form->A[k][l]));
        else constant(1.0);
        simple(oA + b, 0, k);
        simple(oAo + b, 1, k);
        mk.A |= 1u << b;
      }
      if (form->c_u[k][l]) {
        snprintf(name, sizeof name, "c_u[%d][%d]", k, l);
        FH_TRY(fetch(form->c_u[k][l]));
        simple(oCu + b, 0, k);
        mk.C |= 1u << b;
      }
      bool anyD = false, anyW = false;
      for (int d = 0; d < dim; d++) anyD = anyD || form->c_g[k][l][d];
      for (int p = 0; p < m; p++) anyW = anyW || form->A_u[k][p][l];
      if (anyD) {
        for (int d = 0; d < 3; d++) {                 // all three: phase (D) reads the first dim
          snprintf(name, sizeof name, "c_g[%d][%d][%d]", k, l, d);
          if (d < dim && form->c_g[k][l][d]) FH_TRY(fetch(form->c_g[k][l][d]));
          else constant(0.0);
          simple(oD + 3 * b + d, 0, k);
        }
        mk.D |= 1u << b;
      }
      if (anyW) {
        const size_t at = task(oW + 3 * b, 1, 0, k);
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
  ntask = (int)(dir.size() / ST_DIR);
  return 0;
}

extern "C" int fh_generic_assembler_assemble_system_transient(fh_generic_assembler_t as, fh_vec_t sol, fh_vec_t sol_old, const fh_system_form_t* form,
                                                              const double* mass, double time, double dt, double theta, fh_mat_t KK, fh_vec_t RES) {
  FH_GUARD_BEGIN
  const char* who = "fh_generic_assembler_assemble_system_transient";
  // ---- every refusal first: nothing is enqueued before the last of them ----
  FH_REQUIRE(as && RES, "%s: null argument", who);
  FH_REQUIRE(form, "%s: null form", who);
  const int m = form->m;
  FH_REQUIRE(m >= 1 && m <= ST_MAXM, "%s: %d variables, 1 .. %d are served", who, m, ST_MAXM);
  fh_mat_t S = fh_mat_alive(as->mat_uid);
  FH_REQUIRE(S != nullptr, "%s: the matrix this object was created on has been destroyed", who);
  FH_REQUIRE(KK != nullptr, "%s: null matrix", who);
  FH_REQUIRE(KK->m == m * as->ndof && KK->n == m * as->ndof && (long long)KK->nnz == (long long)m * m * as->mat_nnz,
             "%s: not the block system of %d variables on the matrix this object was created on (%d x %d, %d non-zeros; %d x %d, %lld are expected)", who, m, KK->m,
             KK->n, KK->nnz, m * as->ndof, m * as->ndof, (long long)m * m * as->mat_nnz);
  FH_REQUIRE(RES->n_local >= m * as->ndof && (!sol || sol->n_local >= m * as->ndof), "%s: size mismatch", who);
  FH_REQUIRE(sol_old, "%s: null sol_old", who);
  FH_REQUIRE(sol_old->n_local >= m * as->ndof, "%s: sol_old has %d entries, %d variables on this object have %d", who, sol_old->n_local, m, m * as->ndof);
  FH_REQUIRE(!sol || sol_old->n_local == sol->n_local, "%s: sol_old has %d entries, sol has %d", who, sol_old->n_local, sol ? sol->n_local : 0);
  FH_REQUIRE(std::isfinite(time) && std::isfinite(dt) && std::isfinite(theta), "%s: time, dt and theta must be finite", who);
  FH_REQUIRE(dt > 0.0, "%s: dt = %g is not positive", who, dt);
  FH_REQUIRE(theta >= 0.0 && theta <= 1.0, "%s: theta = %g is outside [0, 1]", who, theta);
  SysTrCall c;
  for (int t = 0; t < 16; t++) c.sp.M[t] = 0.0;
  for (int k = 0; k < m; k++)
    for (int l = 0; l < m; l++) {
      const double v = mass ? mass[k * 4 + l] : (k == l ? 1.0 : 0.0);
      FH_REQUIRE(std::isfinite(v), "%s: mass[%d][%d] is not finite", who, k, l);
      c.sp.M[k * m + l] = v;
    }
  std::vector<int> code, dir;
  std::vector<double> consts;
  FH_TRY(st_gather(who, as, form, c.mk, c.ntask, code, dir, consts));
  if (!as->systr[m].ready) FH_TRY(st_plan(who, as, m));
  const size_t ncode = code.size();
  code.insert(code.end(), dir.begin(), dir.end());       // the directory travels, and is compared, as part of the code array
  FH_TRY(gp_upload_program(who, as, code, consts));
  // th_k: theta, or 1 for an algebraic equation; the terms of an equation that is left out at a state leave the masks
  const unsigned row = (1u << m) - 1;
  for (int k = 0; k < 4; k++) c.sp.sn[k] = c.sp.so[k] = 0.0;
  for (int k = 0; k < m; k++) {
    bool algebraic = true;
    for (int l = 0; l < m; l++) algebraic = algebraic && c.sp.M[k * m + l] == 0.0;
    const double th = algebraic ? 1.0 : theta;
    c.sp.sn[k] = dt * th, c.sp.so[k] = dt * (1.0 - th);
    if (th != 0.0) c.mk.newEq |= 1u << k;
    if (th != 1.0) c.mk.oldEq |= 1u << k;
  }
  unsigned rowsNew = 0, rowsOld = 0;
  for (int k = 0; k < m; k++) {
    if ((c.mk.newEq >> k) & 1) rowsNew |= row << (k * m);
    if ((c.mk.oldEq >> k) & 1) rowsOld |= row << (k * m);
  }
  c.mk.Ao = c.mk.A & rowsOld, c.mk.fo = c.mk.f & c.mk.oldEq, c.mk.co = c.mk.c & c.mk.oldEq;
  c.mk.A &= rowsNew, c.mk.W &= rowsNew, c.mk.C &= rowsNew, c.mk.D &= rowsNew, c.mk.f &= c.mk.newEq, c.mk.c &= c.mk.newEq;
  c.sp.time = time, c.sp.time_old = time - dt;
  c.m = m;
  c.pconst = (const double*)as->d_prog;
  c.pcode = (const int*)(as->d_prog + as->consts.size() * sizeof(double));
  c.dir = c.pcode + ncode;
  c.sol = sol ? sol->d : nullptr, c.sol_old = sol_old->d;
  c.Kb = as->d_sysK[m], c.Fb = as->d_sysF[m];
  for (int k = 0; k < as->ns; k++)
    if (as->nslot[k]) st_launch(as, k, c);
  const int lpr = as->sys_lpr[m];
  hipLaunchKernelGGL(k_sys_rows, dim3(fh_div_up((int64_t)m * as->ndof, GP_THREADS / lpr)), dim3(GP_THREADS), as->sys_row_lds[m], as->ctx->stream, as->ndof, m, lpr,
                     as->maxrow, as->rows, as->d_adj_ptr, as->d_adj, c.Kb, (long long)as->nent, as->d_Pos, c.Fb, (long long)as->nrows, S->d_rowptr,
                     (long long)as->mat_nnz, KK->d_val, RES->d);
  const bool ok = hipGetLastError() == hipSuccess;
  fh_mat_values_written(KK);
  FH_REQUIRE(ok, "%s: launch failed", who);
  return 0;
  FH_GUARD_END("fh_generic_assembler_assemble_system_transient")
}

extern "C" int fh_generic_assembler_system_transient_chunks(fh_generic_assembler_t as, int m, int gauss_chunk[3], int lanes[3]) {
  FH_REQUIRE(as && gauss_chunk && lanes && m >= 1 && m <= ST_MAXM,
             "fh_generic_assembler_system_transient_chunks: null argument, or a number of variables outside 1 .. 4");
  gp_read_plan(as, as->systr[m], gauss_chunk, lanes);
  return 0;
}
