// One Newton iteration of one theta-step of  u_t - div(a grad u) + c = f  on the resident plan of the generic assembly (fh_generic.hip): the callback of
// TransientSystem<NonLinearImplicitSystem> (src/08_equations/01_time_dependent/TransientSystem.cpp:62-113) as applications/000_tutorial/ex20_time_dependent
// writes it (AssembleMatrixRes, main.cpp:348-593), scaled by dt as there, with the old state uo read beside u at every Gauss point:
//   RES_i = sum_g w [ -(u - uo) phi_i + dt theta (f phi_i - a grad phi_i . grad u - c phi_i)|new + dt (1 - theta) (f phi_i - a grad phi_i . grad uo - c phi_i)|old ]
//   KK_ij = sum_g w [ phi_i phi_j + dt theta ( a grad phi_i . grad phi_j + a_u phi_j grad phi_i . grad u + phi_i (c_u phi_j + c_g . grad phi_j) ) ]
// The form is fh_quasilinear.hip's; its programs may be over eight variables (x, y, z, u, ux, uy, uz, t).  |new: f, a, c at (x, u, grad u, t = time), |old: the
// same three programs at (x, uo, grad uo, t = time - dt); the derivative programs at the new state only.  `time` is the time at the END of the step
// (TransientSystem::SetUpForSolve advances _time before the assembly).  The Jacobian is the exact one, with the factor theta: ex20 (main.cpp:571) leaves theta
// out of its Jacobian, which is an inexact Newton and is not reproduced here.  time, dt and theta are kernel arguments and never part of the program buffer: a
// step with a new time uploads nothing.  With theta == 1 nothing is evaluated at the old state (a uniform branch, as for the missing terms): the old state
// enters through the mass term alone, and a program that is NaN at uo does not matter.  With theta == 0 the same holds for the new state: its eight programs
// are not run, and KK is the mass matrix.
// sol_old holds at least the object's dofs, as sol and RES must; where sol is given it has exactly sol's local size (two states of one system); with sol NULL
// (= 0) there is no second vector to hold it against, and any sol_old that covers the dofs is taken.
//
// Plan, Kb / Pos / Fb / adj, row pass, program buffer and launch widths are the form body's; the element body is new and larger per element, so it has a Gauss
// chunk, table staging and LDS of its own (the object's `transient` plan, made at the first assemble_transient within GP_LDS_BUDGET):
//   X[nc][3] U[nc] Uo[nc] | JI[gc][9] WG[gc] FS[gc] GU[gc][3] PT[gc][7] UD[gc] GO[gc][3] PO[gc][3] | G[gc][nc][3] ST[gc][nc][2]    = nc 5 + gc 28 + gc nc 5 doubles
// (the form body's nc 4 + gc 21 + gc nc 5; UD = u - uo, GO = grad uo, PO = (f, a, c)|old of a point).  Phases of one chunk, a workgroup barrier between; (B)
// and (C') are those of fh_elembody.h, as the kernel's prologue is:
//   (A)  lane = Gauss point: Jacobian, inverse, det w, x_g -- the text of eb_point_geometry, kept in this body on purpose: as a helper it costs these kernels
//        registers and time (profiles/elembody_share_isa.md); a change to it there is made here too.  x_g is kept in the point's c_g slots until (C) has
//        read it: the same lane
//   (C)  lane = Gauss point: u_g, uo_g, grad u_g (nodes ascending), the eight programs at the new state; unless theta == 1 also grad uo_g and f, a, c at the old one;
//        every value is stored times dt theta (old: dt (1 - theta)), once per point, so that (D) and the residual lanes add the mass term and nothing else
//   (D)  lanes over the nc^2 entries: acc += (phi_i phi_j + a (G_i . G_j) + a_u S_i phi_j + phi_i T_j) WG, points ascending (a, a_u, T scaled);
//        lanes < nc: F += (-UD phi_i + (f phi_i - a S_i - c phi_i) + (fo phi_i - ao So_i - co phi_i)) WG with So_i = G_i . grad uo_g (all nine scaled)
// Every sum has one order, whatever the chunk: a repeated call gives the same bits, and there is no atomic anywhere.  Every entry of Kb and Fb of an active
// element is written; tail sub-groups keep the barriers and touch nothing.
#include "fh_quasilinear.h"
#include "fh_elembody.h"
#include "fh_expr_device.h"
#include <algorithm>
#include <cmath>

namespace {
constexpr int TR_VARS = 8;                   // x, y, z, u, ux, uy, uz, t
constexpr size_t tr_elem_doubles(int ns, int gc) { return (size_t)ns * 5 + (size_t)gc * (21 + QF_PT) + (size_t)gc * ns * 5; }
}  // namespace

// The element body.  Every thread of the workgroup calls this with the same ng, gcm and theta (workgroup barriers, uniform branches); a sub-group without an
// element passes active = false and touches nothing.  Kout: the element's nc x nc rows, Fout its nc residual entries.
template <int L, int NPL>
__device__ __forceinline__ void transient_element_pass(bool active, int lane, int nc, int ng, int gcm, int dim, const double* w, const double* phi, const double* dphi,
                                                       const int* dof_row, const double* coords, const double* sol, const double* sol_old, double time, double dt,
                                                       double theta, const GenFormDir& dir, const int* pcode, const double* pconst, double* lds, double* Kout,
                                                       double* Fout) {
  const int ns = nc;
  double* X = lds;                                   // [ns][3]
  double* U = X + ns * 3;                            // [ns]
  double* Uo = U + ns;                               // [ns]
  double* JI = Uo + ns;                              // [gcm][9]
  double* WG = JI + gcm * 9;                         // [gcm] det w
  double* FS = WG + gcm;                             // [gcm] f (as PT and PO: times dt theta, PO times dt (1 - theta))
  double* GU = FS + gcm;                             // [gcm][3] grad u
  double* PT = GU + gcm * 3;                         // [gcm][7] a, a_u, c, c_u, c_g
  double* UD = PT + gcm * QF_PT;                     // [gcm] u - uo
  double* GO = UD + gcm;                             // [gcm][3] grad uo
  double* PO = GO + gcm * 3;                         // [gcm][3] f, a, c at the old state
  double* G = PO + gcm * 3;                          // [gcm][ns][3]
  double* ST = G + gcm * ns * 3;                     // [gcm][ns][2] S, T
  if (active && lane < nc) {
    const int dof = dof_row[lane];
    for (int d = 0; d < 3; d++) X[lane * 3 + d] = d < dim ? coords[(size_t)dof * dim + d] : 0.0;
    U[lane] = sol ? sol[dof] : 0.0;
    Uo[lane] = sol_old[dof];
  }
  const bool useOld = theta != 1.0;                  // uniform: with theta == 1 the old state is in the mass term alone,
  const bool useNew = theta != 0.0;                  // with theta == 0 the new one
  const bool useS = dir.ncode[QF_AU] >= 0;           // uniform: a term whose programs are all missing is left out, not multiplied by 0
  const bool useT = dir.ncode[QF_CU] >= 0 || dir.ncode[QF_CG] >= 0 || dir.ncode[QF_CG + 1] >= 0 || dir.ncode[QF_CG + 2] >= 0;
  const double sn = dt * theta, so = dt * (1.0 - theta);
  int ei[NPL], ej[NPL];
  double acc[NPL], F = 0.0;
#pragma unroll
  for (int k = 0; k < NPL; k++) {
    const int e = lane + L * k;
    if (active && e < nc * nc) {
      ei[k] = e / nc;
      ej[k] = e - ei[k] * nc;
    } else {
      ei[k] = ej[k] = -1;
    }
    acc[k] = 0.0;
  }
  __syncthreads();
  for (int g0 = 0; g0 < ng; g0 += gcm) {
    const int gc = min(gcm, ng - g0);
    if (active)
      for (int l = lane; l < gc; l += L) {             // (A)
        const int g = g0 + l;
        const double* dp = dphi + (size_t)g * nc * dim;
        double J[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}}, Ji[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}}, det;
        for (int n = 0; n < nc; n++)
          for (int p = 0; p < dim; p++)
            for (int q = 0; q < dim; q++) J[p][q] += dp[n * dim + p] * X[n * 3 + q];
        if (dim == 1) {
          det = J[0][0];
          Ji[0][0] = 1 / det;
        } else if (dim == 2) {
          det = J[0][0] * J[1][1] - J[0][1] * J[1][0];
          Ji[0][0] = J[1][1] / det;
          Ji[0][1] = -J[0][1] / det;
          Ji[1][0] = -J[1][0] / det;
          Ji[1][1] = J[0][0] / det;
        } else {
          det = J[0][0] * (J[1][1] * J[2][2] - J[1][2] * J[2][1]) + J[0][1] * (J[1][2] * J[2][0] - J[1][0] * J[2][2]) + J[0][2] * (J[1][0] * J[2][1] - J[1][1] * J[2][0]);
          Ji[0][0] = (-J[1][2] * J[2][1] + J[1][1] * J[2][2]) / det;
          Ji[0][1] = (J[0][2] * J[2][1] - J[0][1] * J[2][2]) / det;
          Ji[0][2] = (-J[0][2] * J[1][1] + J[0][1] * J[1][2]) / det;
          Ji[1][0] = (J[1][2] * J[2][0] - J[1][0] * J[2][2]) / det;
          Ji[1][1] = (-J[0][2] * J[2][0] + J[0][0] * J[2][2]) / det;
          Ji[1][2] = (J[0][2] * J[1][0] - J[0][0] * J[1][2]) / det;
          Ji[2][0] = (-J[1][1] * J[2][0] + J[1][0] * J[2][1]) / det;
          Ji[2][1] = (J[0][1] * J[2][0] - J[0][0] * J[2][1]) / det;
          Ji[2][2] = (-J[0][1] * J[1][0] + J[0][0] * J[1][1]) / det;
        }
        for (int q = 0; q < 3; q++)
          for (int p = 0; p < 3; p++) JI[l * 9 + q * 3 + p] = Ji[q][p];
        WG[l] = det * w[g];
        double xq[3] = {0, 0, 0};
        for (int n = 0; n < nc; n++) {
          const double ph = phi[(size_t)g * nc + n];
          for (int q = 0; q < dim; q++) xq[q] += X[n * 3 + q] * ph;
        }
        for (int q = 0; q < 3; q++) PT[l * QF_PT + 4 + q] = xq[q];
      }
    __syncthreads();
    if (active) eb_chunk_gradients<L, true>(lane, g0, gc, nc, ns, dim, dphi, JI, 9, G);      // (B)
    __syncthreads();
    if (active)
      for (int l = lane; l < gc; l += L) {             // (C)
        double ug = 0.0, og = 0.0, gu[3] = {0, 0, 0}, go[3] = {0, 0, 0};       // in registers: the programs' variable vector is indexed at run time
        for (int n = 0; n < nc; n++) {
          const double un = U[n], on = Uo[n], ph = phi[(size_t)(g0 + l) * nc + n];
          ug += ph * un;
          og += ph * on;
#pragma unroll
          for (int q = 0; q < 3; q++)
            if (q < dim) {
              gu[q] += G[(l * ns + n) * 3 + q] * un;
              if (useOld) go[q] += G[(l * ns + n) * 3 + q] * on;
            }
        }
        double v[TR_VARS] = {PT[l * QF_PT + 4], PT[l * QF_PT + 5], PT[l * QF_PT + 6], ug, gu[0], gu[1], gu[2], time};
        for (int q = 0; q < 3; q++) GU[l * 3 + q] = gu[q], GO[l * 3 + q] = go[q];
        UD[l] = ug - og;
#pragma unroll 1
        for (int p = 0; p < QF_NPROG + 3; p++) {       // the eight at the new state, then f, a, c at the old one: one variable vector, rewritten between the two
          const bool old = p >= QF_NPROG;
          if (p == QF_NPROG) {
            if (!useOld) break;
            v[3] = og, v[4] = go[0], v[5] = go[1], v[6] = go[2], v[7] = time - dt;
          }
          const int q = old ? (p == QF_NPROG ? QF_F : p == QF_NPROG + 1 ? QF_A : QF_C) : p;
          double val = 0.0;                              // theta == 0: the new state is in the mass term alone, none of its programs runs
          if (old || useNew)
            val = (old ? so : sn) * (dir.ncode[q] >= 0 ? fh_expr_device_eval(pcode + dir.code[q], dir.ncode[q], pconst + dir.kons[q], v) : q == QF_A ? 1.0 : 0.0);
          if (old) PO[l * 3 + p - QF_NPROG] = val;
          else if (p == QF_F) FS[l] = val;
          else PT[l * QF_PT + p - 1] = val;
        }
      }
    __syncthreads();
    if (active && (useS || useT)) eb_chunk_st<L>(lane, g0, gc, nc, dim, phi, G, GU, PT, ST);     // (C')
    if (useS || useT) __syncthreads();
#pragma unroll
    for (int k = 0; k < NPL; k++)                      // (D)
      if (ei[k] >= 0) {
        double a = acc[k];
        const int i = ei[k], j = ej[k];
        for (int l = 0; l < gc; l++) {
          const double *gi = G + (l * ns + i) * 3, *gj = G + (l * ns + j) * 3;
          const double pi = phi[(size_t)(g0 + l) * nc + i], pj = phi[(size_t)(g0 + l) * nc + j];
          double dot = 0.0;
          for (int q = 0; q < dim; q++) dot += gi[q] * gj[q];
          double val = PT[l * QF_PT] * dot;
          if (useS) val += PT[l * QF_PT + 1] * ST[(l * ns + i) * 2] * pj;
          if (useT) val += pi * ST[(l * ns + j) * 2 + 1];
          a += (pi * pj + val) * WG[l];
        }
        acc[k] = a;
      }
    if (active && lane < nc)
      for (int l = 0; l < gc; l++) {
        const double* gi = G + (l * ns + lane) * 3;
        const double ph = phi[(size_t)(g0 + l) * nc + lane];
        double S = 0.0;
        for (int q = 0; q < dim; q++) S += gi[q] * GU[l * 3 + q];
        double val = -UD[l] * ph + (FS[l] * ph - PT[l * QF_PT] * S - PT[l * QF_PT + 2] * ph);
        if (useOld) {
          double So = 0.0;
          for (int q = 0; q < dim; q++) So += gi[q] * GO[l * 3 + q];
          val += PO[l * 3] * ph - PO[l * 3 + 1] * So - PO[l * 3 + 2] * ph;
        }
        F += val * WG[l];
      }
    __syncthreads();
  }
  if (!active) return;
#pragma unroll
  for (int k = 0; k < NPL; k++)
    if (ei[k] >= 0) Kout[lane + L * k] = acc[k];
  if (lane < nc) Fout[lane] = F;
}

// Element pass of the plan for one theta-step.  L lanes per element, 256 / L elements per workgroup; TL: the shape's tables in LDS.  Output as k_gen_form
// leaves it: row i of slot s at Kb[(s nc + i) nc], its residual entry at Fb[s nc + i].
template <int L, bool TL>
__global__ __launch_bounds__(GP_THREADS) void k_gen_transient(int nslot, int nc, int ng, int gcm, int dim, const double* __restrict__ gw, const double* __restrict__ gphi,
                                                              const double* __restrict__ gdphi, const int* __restrict__ ed, const double* __restrict__ coords,
                                                              const double* __restrict__ sol, const double* __restrict__ sol_old, double time, double dt, double theta,
                                                              GenFormDir dir, const int* __restrict__ pcode, const double* __restrict__ pconst,
                                                              double* __restrict__ Kb, double* __restrict__ Fb) {
  extern __shared__ __attribute__((aligned(16))) double transient_smem[];
  const EbGroup g = eb_prologue<L, TL>(transient_smem, nslot, nc, ng, dim, (int)tr_elem_doubles(nc, gcm), gw, gphi, gdphi);
  transient_element_pass<L, gp_entries_per_lane(L)>(g.active, g.lane, nc, ng, gcm, dim, g.w, g.phi, g.dphi, ed + (size_t)g.slot * nc, coords, sol, sol_old, time, dt,
                                                    theta, dir, pcode, pconst, g.lds, Kb + (size_t)g.slot * nc * nc, Fb + (size_t)g.slot * nc);
}

namespace {
struct TrCall {
  const double *sol, *sol_old;
  double time, dt, theta;
  GenFormDir dir;
  const int* pcode;
  const double* pconst;
};
}  // namespace

static void tr_launch(fh_generic_assembler_t as, int k, const TrCall& c) {
  const GenBodyPlan& P = as->transient;
  gp_dispatch(P, k, [&](auto lanes, auto staged) {
    constexpr int L = decltype(lanes)::value;
    hipLaunchKernelGGL((k_gen_transient<L, decltype(staged)::value>), dim3(fh_div_up(as->nslot[k], GP_THREADS / L)), dim3(GP_THREADS), P.lds[k], as->ctx->stream,
                       as->nslot[k], as->nc[k], as->ng[k], P.gcm[k], as->dim, as->d_w[k], as->d_phi[k], as->d_dphi[k], as->d_ed[k], as->d_coords, c.sol, c.sol_old, c.time,
                       c.dt, c.theta, c.dir, c.pcode, c.pconst, as->d_Kb + as->rows.kb_base[k], as->d_Fb + as->rows.row_base[k]);
  });
}

extern "C" int fh_generic_assembler_assemble_transient(fh_generic_assembler_t as, fh_vec_t sol, fh_vec_t sol_old, const fh_quasilinear_form_t* form, double time,
                                                       double dt, double theta, fh_mat_t KK, fh_vec_t RES) {
  FH_GUARD_BEGIN
  const char* who = "fh_generic_assembler_assemble_transient";
  // ---- every refusal first: nothing is enqueued before the last of them ----
  FH_TRY(gp_check_call(who, as, sol, KK, RES));
  FH_REQUIRE(form, "fh_generic_assembler_assemble_transient: null form");
  FH_REQUIRE(sol_old, "fh_generic_assembler_assemble_transient: null sol_old");
  FH_REQUIRE(sol_old->n_local >= as->ndof, "fh_generic_assembler_assemble_transient: sol_old has %d entries, the object has %d dofs", sol_old->n_local, as->ndof);
  FH_REQUIRE(!sol || sol_old->n_local == sol->n_local, "fh_generic_assembler_assemble_transient: sol_old has %d entries, sol has %d", sol_old->n_local,
             sol ? sol->n_local : 0);
  FH_REQUIRE(std::isfinite(time) && std::isfinite(dt) && std::isfinite(theta), "fh_generic_assembler_assemble_transient: time, dt and theta must be finite");
  FH_REQUIRE(dt > 0.0, "fh_generic_assembler_assemble_transient: dt = %g is not positive", dt);
  FH_REQUIRE(theta >= 0.0 && theta <= 1.0, "fh_generic_assembler_assemble_transient: theta = %g is outside [0, 1]", theta);
  TrCall c;
  std::vector<int> code;
  std::vector<double> consts;
  FH_TRY(qf_gather_programs(who, as, form, TR_VARS, "x, y, z, u, ux, uy, uz, t", c.dir, code, consts));
  // the first call: this body's plan on the Poisson body's lanes, with the evened chunk rule (ng = 16 at a limit of 14 goes as 8 + 8, not 14 + 2)
  if (!as->transient.ready)
    FH_TRY(gp_plan_body(who, as, as->poisson.lanes, tr_elem_doubles, true, true, "an element", " with the transient element body", as->transient));
  FH_TRY(gp_upload_program(who, as, code, consts));
  c.sol = sol ? sol->d : nullptr, c.sol_old = sol_old->d, c.time = time, c.dt = dt, c.theta = theta;
  c.pconst = (const double*)as->d_prog;
  c.pcode = (const int*)(as->d_prog + as->consts.size() * sizeof(double));
  for (int k = 0; k < as->ns; k++)
    if (as->nslot[k]) tr_launch(as, k, c);
  gp_launch_rows(as, KK, RES);
  const bool ok = hipGetLastError() == hipSuccess;
  fh_mat_values_written(KK);
  FH_REQUIRE(ok, "fh_generic_assembler_assemble_transient: launch failed");
  return 0;
  FH_GUARD_END("fh_generic_assembler_assemble_transient")
}

extern "C" int fh_generic_assembler_transient_chunks(fh_generic_assembler_t as, int gauss_chunk[3]) {
  FH_REQUIRE(as && gauss_chunk, "fh_generic_assembler_transient_chunks: null argument");
  gp_read_plan(as, as->transient, gauss_chunk, nullptr);
  return 0;
}
