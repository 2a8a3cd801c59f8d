// A quasilinear scalar equation on the resident plan of the generic assembly (fh_generic.hip): -div(a grad u) + c = f with a = a(x, u), c = c(x, u, grad u),
// the Jacobian and residual of one Newton step of NonLinearImplicitSystem (applications/000_tutorial/ex03_poisson_plus_nonlin_advection/main.cpp:419-446,
// ex03b_div_grad_nonlinear_diffusivity/main.cpp:423-455):
//   RES_i = sum_g [ f phi_i - a (grad phi_i . grad u) - c phi_i ] w
//   KK_ij = sum_g [ a (grad phi_i . grad phi_j) + a_u phi_j (grad phi_i . grad u) + phi_i ( c_u phi_j + c_g . grad phi_j ) ] w
// f, a, a_u, c, c_u, c_g[0 .. dim) are run-time programs over (x, y, z, u, ux, uy, uz) at the Gauss point; a missing one is a = 1, everything else 0.
//
// The plan is the Poisson object's, untouched: the same element tables, Kb / Pos / Fb / adj and the same row pass (k_gen_rows adds full nc x nc element rows
// already).  What is new is the element body: the Poisson body stores the pairs i <= j and mirrors them, this one forms every (i, j) -- the advection and
// the a_u term are not symmetric.  Launch geometry per shape as there (L = 64 / 32 / 16 lanes per element, 256-thread workgroups, tables staged where they
// fit); the Gauss points go through LDS in chunks of a plan of its own (the object's `form`), made at the first assemble_form within GP_LDS_BUDGET because an
// element needs more here:
//   X[nc][3] U[nc] | JI[gc][9] WG[gc] FS[gc] GU[gc][3] PT[gc][7] | G[gc][nc][3] ST[gc][nc][2]      = nc 4 + gc 21 + gc nc 5 doubles
// (the Poisson body's nc 4 + gc 14 + gc nc 3, and gc 7 + gc nc 2 more).  Phases of one chunk, a workgroup barrier between them; (A) and (C') are those of
// fh_elembody.h, as the kernel's prologue is:
//   (A)  x_g is kept in the point's c_g slots until (C) has read it: the same lane
//   (B)  lanes over (point, node): G_n = Jac^-1 dphi_n -- the text of eb_chunk_gradients, kept in this body on purpose: as a helper it gives these kernels
//        another schedule (profiles/elembody_share_isa.md); a change to it there is made here too
//   (C)  lane = Gauss point: u_g = sum phi_n U_n, grad u_g = sum G_n U_n (nodes ascending), then the programs at (x_g, u_g, grad u_g):
//        FS = f, PT = (a, a_u, c, c_u, c_g[3])
//   (D)  lanes over the nc^2 entries e = i nc + j (at most 12 per lane at L = 64 for HEX27's 729, at most 4 where elements share a wave: nc <= 10 there):
//        acc += (a (G_i . G_j) + a_u S_i phi_j + phi_i T_j) WG, points ascending; lanes < nc: F += (f phi_i - a S_i - c phi_i) WG
// Every sum has one order, whatever the chunk: a repeated call gives the same bits, and there is no atomic anywhere.  Every entry of Kb and Fb of an active
// element is written (12 L >= 729, 4 L >= nc^2 is checked on the host), so the row pass reads nothing stale or poisoned.
//
// The programs sit back to back in the object's program buffer -- all constants, then all code, the layout of the Poisson path's single program, so the two
// paths share the buffer and its cache: it is uploaded only when its content differs from the last call's, whichever path made that.  The directory (where
// each program starts, how long it is) is 96 bytes of kernel argument.
#include "fh_quasilinear.h"
#include "fh_elembody.h"
#include "fh_expr_device.h"
#include <algorithm>

namespace {
constexpr int QF_VARS = 7;                   // x, y, z, u, ux, uy, uz
constexpr size_t qf_elem_doubles(int ns, int gc) { return (size_t)ns * 4 + (size_t)gc * (14 + QF_PT) + (size_t)gc * ns * 5; }
}  // namespace

// The element body.  Every thread of the workgroup calls this with the same ng and gcm (workgroup barriers); a sub-group without an element passes
// active = false and touches nothing.  Kout: the element's nc x nc rows, Fout its nc residual entries.
template <int L, int NPL>
__device__ __forceinline__ void form_element_pass(bool active, int lane, int nc, int ng, int gcm, int dim, const double* w, const double* phi, const double* dphi,
                                                  const int* dof_row, const double* coords, const double* sol, const GenFormDir& dir, const int* pcode,
                                                  const double* pconst, double* lds, double* Kout, double* Fout) {
  const int ns = nc;
  double* X = lds;                                   // [ns][3]
  double* U = X + ns * 3;                            // [ns]
  double* JI = U + ns;                               // [gcm][9]
  double* WG = JI + gcm * 9;                         // [gcm] det w
  double* FS = WG + gcm;                             // [gcm] f
  double* GU = FS + gcm;                             // [gcm][3] grad u
  double* PT = GU + gcm * 3;                         // [gcm][7] a, a_u, c, c_u, c_g
  double* G = PT + gcm * QF_PT;                      // [gcm][ns][3]
  double* ST = G + gcm * ns * 3;                     // [gcm][ns][2] S, T
  if (active && lane < nc) {
    const int dof = dof_row[lane];
    for (int d = 0; d < 3; d++) X[lane * 3 + d] = d < dim ? coords[(size_t)dof * dim + d] : 0.0;
    U[lane] = sol ? sol[dof] : 0.0;
  }
  const bool useS = dir.ncode[QF_AU] >= 0;           // uniform: a term whose programs are all missing is left out, not multiplied by 0
  const bool useT = dir.ncode[QF_CU] >= 0 || dir.ncode[QF_CG] >= 0 || dir.ncode[QF_CG + 1] >= 0 || dir.ncode[QF_CG + 2] >= 0;
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
        double xq[3] = {0, 0, 0};
        eb_point_geometry(X, dphi + (size_t)g * nc * dim, phi + (size_t)g * nc, w + g, nc, dim, JI + l * 9, WG + l, xq);
        for (int q = 0; q < 3; q++) PT[l * QF_PT + 4 + q] = xq[q];
      }
    __syncthreads();
    if (active)
      for (int t = lane; t < gc * nc; t += L) {        // (B)
        const int l = t / nc, n = t - l * nc;
        const double* dp = dphi + ((size_t)(g0 + l) * nc + n) * dim;
        for (int q = 0; q < 3; q++) {
          double sacc = 0.0;
          if (q < dim)
            for (int p = 0; p < dim; p++) sacc += JI[l * 9 + q * 3 + p] * dp[p];
          G[(l * ns + n) * 3 + q] = sacc;
        }
      }
    __syncthreads();
    if (active)
      for (int l = lane; l < gc; l += L) {             // (C)
        double v[QF_VARS] = {PT[l * QF_PT + 4], PT[l * QF_PT + 5], PT[l * QF_PT + 6], 0, 0, 0, 0};
        for (int n = 0; n < nc; n++) {
          const double un = U[n];
          v[3] += phi[(size_t)(g0 + l) * nc + n] * un;
          for (int q = 0; q < dim; q++) v[4 + q] += G[(l * ns + n) * 3 + q] * un;
        }
        for (int q = 0; q < 3; q++) GU[l * 3 + q] = v[4 + q];
#pragma unroll 1
        for (int p = 0; p < QF_NPROG; p++) {
          const double val = dir.ncode[p] >= 0 ? fh_expr_device_eval(pcode + dir.code[p], dir.ncode[p], pconst + dir.kons[p], v) : p == QF_A ? 1.0 : 0.0;
          if (p == QF_F) FS[l] = val;
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
          double dot = 0.0;
          for (int q = 0; q < dim; q++) dot += gi[q] * gj[q];
          double val = PT[l * QF_PT] * dot;
          if (useS) val += PT[l * QF_PT + 1] * ST[(l * ns + i) * 2] * phi[(size_t)(g0 + l) * nc + j];
          if (useT) val += phi[(size_t)(g0 + l) * nc + i] * ST[(l * ns + j) * 2 + 1];
          a += val * WG[l];
        }
        acc[k] = a;
      }
    if (active && lane < nc)
      for (int l = 0; l < gc; l++) {
        const double* gi = G + (l * ns + lane) * 3;
        double S = 0.0;
        for (int q = 0; q < dim; q++) S += gi[q] * GU[l * 3 + q];
        const double ph = phi[(size_t)(g0 + l) * nc + lane];
        F += (FS[l] * ph - PT[l * QF_PT] * S - PT[l * QF_PT + 2] * ph) * WG[l];
      }
    __syncthreads();
  }
  if (!active) return;
#pragma unroll
  for (int k = 0; k < NPL; k++)
    if (ei[k] >= 0) Kout[lane + L * k] = acc[k];
  if (lane < nc) Fout[lane] = F;
}

// Element pass of the plan for a form.  L lanes per element, 256 / L elements per workgroup; TL: the shape's tables in LDS.  Output as k_gen_pairs leaves it:
// row i of slot s at Kb[(s nc + i) nc], its residual entry at Fb[s nc + i].
template <int L, bool TL>
__global__ __launch_bounds__(GP_THREADS) void k_gen_form(int nslot, int nc, int ng, int gcm, int dim, const double* __restrict__ gw, const double* __restrict__ gphi,
                                                         const double* __restrict__ gdphi, const int* __restrict__ ed, const double* __restrict__ coords,
                                                         const double* __restrict__ sol, GenFormDir dir, const int* __restrict__ pcode,
                                                         const double* __restrict__ pconst, double* __restrict__ Kb, double* __restrict__ Fb) {
  extern __shared__ __attribute__((aligned(16))) double form_smem[];
  const EbGroup g = eb_prologue<L, TL>(form_smem, nslot, nc, ng, dim, (int)qf_elem_doubles(nc, gcm), gw, gphi, gdphi);
  form_element_pass<L, gp_entries_per_lane(L)>(g.active, g.lane, nc, ng, gcm, dim, g.w, g.phi, g.dphi, ed + (size_t)g.slot * nc, coords, sol, dir, pcode, pconst, g.lds,
                                               Kb + (size_t)g.slot * nc * nc, Fb + (size_t)g.slot * nc);
}

static void qf_launch(fh_generic_assembler_t as, int k, const double* sol, const GenFormDir& dir, const int* pcode, const double* pconst) {
  const GenBodyPlan& P = as->form;
  gp_dispatch(P, k, [&](auto lanes, auto staged) {
    constexpr int L = decltype(lanes)::value;
    hipLaunchKernelGGL((k_gen_form<L, decltype(staged)::value>), dim3(fh_div_up(as->nslot[k], GP_THREADS / L)), dim3(GP_THREADS), P.lds[k], as->ctx->stream,
                       as->nslot[k], as->nc[k], as->ng[k], P.gcm[k], as->dim, as->d_w[k], as->d_phi[k], as->d_dphi[k], as->d_ed[k], as->d_coords, sol, dir, pcode, pconst,
                       as->d_Kb + as->rows.kb_base[k], as->d_Fb + as->rows.row_base[k]);
  });
}

int qf_gather_programs(const char* who, fh_generic_assembler_t as, const fh_quasilinear_form_t* form, int max_vars, const char* vars, GenFormDir& dir,
                       std::vector<int>& code, std::vector<double>& consts) {
  static const char* const names[QF_NPROG] = {"f", "a", "a_u", "c", "c_u", "c_g[0]", "c_g[1]", "c_g[2]"};
  const fh_expr_t progs[QF_NPROG] = {form->f, form->a, form->a_u, form->c, form->c_u, form->c_g[0], form->c_g[1], form->c_g[2]};
  for (int d = as->dim; d < 3; d++) FH_REQUIRE(!progs[QF_CG + d], "%s: c_g[%d] given on a mesh of dimension %d", who, d, as->dim);
  std::vector<int> c1;
  std::vector<double> k1;
  code.clear();
  consts.clear();
  for (int p = 0; p < QF_NPROG; p++) {
    dir.code[p] = dir.kons[p] = 0;
    dir.ncode[p] = -1;
    if (!progs[p]) continue;
    int nv = 0;
    FH_TRY(fh_expr_nvars(progs[p], &nv));
    FH_REQUIRE(nv <= max_vars, "%s: the program %s has %d variables, at most %d (%s) are served", who, names[p], nv, max_vars, vars);
    FH_TRY(fh_expr_fetch(progs[p], names[p], max_vars, c1, k1));
    dir.code[p] = (int)code.size(), dir.ncode[p] = (int)c1.size(), dir.kons[p] = (int)consts.size();
    code.insert(code.end(), c1.begin(), c1.end());
    consts.insert(consts.end(), k1.begin(), k1.end());
  }
  return 0;
}

extern "C" int fh_generic_assembler_assemble_form(fh_generic_assembler_t as, fh_vec_t sol, const fh_quasilinear_form_t* form, fh_mat_t KK, fh_vec_t RES) {
  FH_GUARD_BEGIN
  const char* who = "fh_generic_assembler_assemble_form";
  FH_TRY(gp_check_call(who, as, sol, KK, RES));
  FH_REQUIRE(form, "fh_generic_assembler_assemble_form: null form");
  // ---- every refusal first: nothing is enqueued before the last of them ----
  GenFormDir dir;
  std::vector<int> code;
  std::vector<double> consts;
  FH_TRY(qf_gather_programs(who, as, form, QF_VARS, "x, y, z, u, ux, uy, uz", dir, code, consts));
  // the first call: the Gauss chunk, table staging and LDS of the larger element body per shape, on the Poisson body's lanes
  if (!as->form.ready) FH_TRY(gp_plan_body(who, as, as->poisson.lanes, qf_elem_doubles, false, true, "an element", " with the quasilinear element body", as->form));
  FH_TRY(gp_upload_program(who, as, code, consts));
  const double* d_k = (const double*)as->d_prog;
  const int* d_code = (const int*)(as->d_prog + as->consts.size() * sizeof(double));
  for (int k = 0; k < as->ns; k++)
    if (as->nslot[k]) qf_launch(as, k, sol ? sol->d : nullptr, dir, d_code, d_k);
  gp_launch_rows(as, KK, RES);
  const bool ok = hipGetLastError() == hipSuccess;
  fh_mat_values_written(KK);
  FH_REQUIRE(ok, "fh_generic_assembler_assemble_form: launch failed");
  return 0;
  FH_GUARD_END("fh_generic_assembler_assemble_form")
}

extern "C" int fh_generic_assembler_form_chunks(fh_generic_assembler_t as, int gauss_chunk[3]) {
  FH_REQUIRE(as && gauss_chunk, "fh_generic_assembler_form_chunks: null argument");
  gp_read_plan(as, as->form, gauss_chunk, nullptr);
  return 0;
}
