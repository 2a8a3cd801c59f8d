// The element body of the error norms against a known solution (GetErrorNorm_L2_H1_with_analytical_sol and its variants, FE_convergence.hpp:1279-1415,
// :1457-, :480-935) as code that both the host statement (fh_elem_error_norms_host) and the kernel of fh_elemnorm.hip compile: one Gauss point and the sums of
// an element over its points.  Weight, phi and grad phi are those of the flags' body (ee_jacobian_t, ee_gradphi_t of fh_elemerror_body.h); contraction is off
// inside every function for the reason given there.  The expression evaluator (fh_expr_device.h) applies one operation per statement, so nothing in it can be
// contracted either: a program of + - * /, sqrt and the exact operations gives the same bits on both sides, one with sin, cos, exp and their like differs by the
// ulps of the two math libraries.
#pragma once
#include "fh_elemerror_body.h"
#include "fh_expr_device.h"

namespace fherr {
constexpr int EN_QP = 0, EN_DOFS = 1, EN_VECTOR = 2;      // what u_h is compared with: exact values at the Gauss points, the exact function's nodal interpolant,
                                                          // a second discrete function
constexpr int EN_MAXT = 4;            // doubles one Gauss point leaves: the L2 term, then dim terms of the H1 semi-norm

// the 1 + dim programs (exact, then its gradient's components) back to back: program k is code[cptr[k] .. cptr[k + 1]) over consts + kptr[k]
struct EnProgs {
  const int* code;
  const int* cptr;
  const double* consts;
  const int* kptr;
};
FH_HD inline double en_eval(const EnProgs& pr, int k, const double* xyzt) {
  return fh_expr_device_eval(pr.code + pr.cptr[k], pr.cptr[k + 1] - pr.cptr[k], pr.consts + pr.kptr[k], xyzt);
}
// exact at a node: the point (x, 0 beyond dim, t = 0) as the generic assembler passes it to the source; Xn = X + n * 3, zero beyond dim
FH_HD inline double en_nodal(const EnProgs& pr, const double* Xn) {
  const double xyzt[4] = {Xn[0], Xn[1], Xn[2], 0.0};
  return en_eval(pr, 0, xyzt);
}

// One Gauss point: u_h = sum phi_i sol_i, g_h[j] = sum phi_x[i,j] sol_i, nodes ascending; U non-null (modes dofs and vector): u and g[j] the same sums over U;
// U null (mode qp): x_g[j] = sum x_i[j] phi_i (:1381) and u, g[j] the programs at (x_g, t = 0).  out[0] = (u_h - u)(u_h - u) w, out[1 + j] = (g_h[j] - g[j])
// (g_h[j] - g[j]) w.  X[n * 3 + b], phi[n], dphi[n * dim + a] of this point.  The sums are en_sums_t (the dimension a compile-time number inside, as in
// ee_point_t); the programs run in en_point, in a loop that is not unrolled: the one place of the point's body where the evaluator is instantiated.
struct EnSums {
  double weight, h[4], c[4], xg[4];     // h = {u_h, g_h[j]}, c = {u, g[j]} (U non-null), xg = {x_g[j], 0 ..., t = 0} (U null)
};
template <int dim>
FH_HD inline void en_sums_t(int nc, double wg, const double* phi, const double* dphi, const double* X, const double* S, const double* U, EnSums& s) {
#pragma clang fp contract(off)
  double Ji[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
  s.weight = ee_jacobian_t<dim>(nc, wg, dphi, X, Ji);
  double uh = 0., u = 0., gh[3] = {0., 0., 0.}, g[3] = {0., 0., 0.}, xg[3] = {0., 0., 0.};
  for (int n = 0; n < nc; n++) {
    uh += phi[n] * S[n];
    if (U) u += phi[n] * U[n];
    for (int a = 0; a < dim; a++) {
      const double gp = ee_gradphi_t<dim>(dphi + n * dim, Ji, a);
      gh[a] += gp * S[n];
      if (U) g[a] += gp * U[n];
      else xg[a] += X[n * 3 + a] * phi[n];
    }
  }
  s.h[0] = uh;
  s.c[0] = u;
  for (int a = 0; a < 3; a++) {
    s.h[1 + a] = gh[a];
    s.c[1 + a] = g[a];
    s.xg[a] = xg[a];
  }
  s.xg[3] = 0.;
}

// PROGS false: U is never null and no evaluator is instantiated (the kernel of mode vector)
template <bool PROGS = true>
FH_HD inline void en_point(int dim, int nc, double wg, const double* phi, const double* dphi, const double* X, const double* S, const double* U, const EnProgs& pr,
                           double* out) {
#pragma clang fp contract(off)
  EnSums s;
  if (dim == 2) en_sums_t<2>(nc, wg, phi, dphi, X, S, U, s);
  else en_sums_t<3>(nc, wg, phi, dphi, X, S, U, s);
  const double h[4] = {s.h[0], s.h[1], s.h[2], s.h[3]}, c[4] = {s.c[0], s.c[1], s.c[2], s.c[3]};
#pragma nounroll
  for (int k = 0; k <= dim; k++) {
    const double hk = k == 0 ? h[0] : k == 1 ? h[1] : k == 2 ? h[2] : h[3];
    const double ck = (!PROGS || U) ? (k == 0 ? c[0] : k == 1 ? c[1] : k == 2 ? c[2] : c[3]) : en_eval(pr, k, s.xg);
    out[k] = (hk - ck) * (hk - ck) * s.weight;
  }
}

// The element's sums over its points, ascending, every term added on its own as the reference's += do.  T[ig * (1 + dim) + ...]; res = {l2_i, h1_i}
FH_HD inline void en_element_sums(int ng, int dim, const double* T, double res[2]) {
#pragma clang fp contract(off)
  double l2 = 0., h1 = 0.;
  for (int ig = 0; ig < ng; ig++) {
    const double* t = T + ig * (1 + dim);
    for (int k = 0; k < dim; k++) h1 += t[1 + k];
    l2 += t[0];
  }
  res[0] = l2;
  res[1] = h1;
}
}  // namespace fherr
