// The element body of the error-norm flags (Solution::FlagAMRRegionBasedOnErroNormAdaptive, Solution.cpp:843-1101) as code that both the host statement
// (fh_elem_error_flag_host) and the kernels of fh_elemerror.hip compile: one Gauss point, the sums of an element over its points, the comparisons, and the
// shape of the global sums.  Contraction is switched off inside every function: the translation units are built with -ffp-contract=on, under which the host
// compiler (no fused multiply-add in its baseline instruction set) and the device compiler would round the same text differently; with it off every product
// and every sum is rounded on its own on both sides, and the two give the same bits.
#pragma once
#include "fh_fe_basis.h"

namespace fherr {
constexpr int EE_MAXG = 125;          // most Gauss points of a rule served (HEX27, ninth order)
constexpr int EE_MAXT = 9;            // doubles one Gauss point leaves: the weight, then 1 + dim terms of the solution's norm and as many of the error's
constexpr int EE_RB = 256;            // the global sums: chunks of EE_RC consecutive entries, EE_RB strided running sums in a chunk, then a binary tree
constexpr int EE_RC = 1024;

// the reference's literals (Solution.cpp:846)
FH_HD inline double ee_scale2(int fe, int norm) {
  return fe == 0 ? (norm ? 1. : 0.111111) : (norm ? 0.111111 : 0.0204081632653);
}
FH_HD inline int ee_nterms(int dim, int norm) { return norm ? 1 + dim : 1; }

// elem_type::Jacobian over the family's first nc nodes (Jac[a][b] += dphi_n/dxi_a x_n[b], nodes ascending; the inverse and the determinant in the reference's
// terms): fills JacI and returns the point's weight.  X[n * 3 + b], dphi[n * dim + a] of this point.  Shared by the flags' body below and the norms' body
// (fh_elemnorm_body.h).
template <int dim>
FH_HD inline double ee_jacobian_t(int nc, double wg, const double* dphi, const double* X, double Ji[3][3]) {
#pragma clang fp contract(off)
  double J[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}}, det;
  for (int n = 0; n < nc; n++)
    for (int a = 0; a < dim; a++)
      for (int b = 0; b < dim; b++) J[a][b] += dphi[n * dim + a] * X[n * 3 + b];
  if (dim == 2) {
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
  return det * wg;
}

// grad phi_n [a] = sum_b dphi_n/dxi_b JacI[a][b], from the left; dphi_n = the node's dim reference derivatives
template <int dim>
FH_HD inline double ee_gradphi_t(const double* dphi_n, const double Ji[3][3], int a) {
#pragma clang fp contract(off)
  double g = dphi_n[0] * Ji[a][0];
  for (int b = 1; b < dim; b++) g = g + dphi_n[b] * Ji[a][b];
  return g;
}

// One Gauss point: weight and gradients as above, then solig / solGradig and errig / errGradig (nodes ascending) and the terms as the reference writes them:
// v v w, g_j g_j w and scale v v w, scale g_j g_j w.  X[n * 3 + b], phi[n], dphi[n * dim + a] of this point.
// out[0] = weight, out[1 .. nt] the solution's terms (S null: zeros), out[1 + nt .. 2 nt] the error's.
template <int dim>
FH_HD inline void ee_point_t(int nc, double wg, const double* phi, const double* dphi, const double* X, const double* S, const double* E, int norm, double sc,
                           double* out) {
#pragma clang fp contract(off)
  double Ji[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
  const double weight = ee_jacobian_t<dim>(nc, wg, dphi, X, Ji);
  double sv = 0., ev = 0., sg[3] = {0., 0., 0.}, eg[3] = {0., 0., 0.};
  for (int n = 0; n < nc; n++) {
    if (S) sv += phi[n] * S[n];
    ev += phi[n] * E[n];
    if (norm)
      for (int a = 0; a < dim; a++) {
        const double g = ee_gradphi_t<dim>(dphi + n * dim, Ji, a);
        if (S) sg[a] += S[n] * g;
        eg[a] += E[n] * g;
      }
  }
  const int nt = ee_nterms(dim, norm);
  out[0] = weight;
  out[1] = sv * sv * weight;
  out[1 + nt] = sc * ev * ev * weight;
  if (norm)
    for (int a = 0; a < dim; a++) {
      out[2 + a] = sg[a] * sg[a] * weight;
      out[2 + nt + a] = sc * eg[a] * eg[a] * weight;
    }
}

// (the dimension is a compile-time number inside: J, its inverse and the gradients stay in registers)
FH_HD inline void ee_point(int dim, int nc, double wg, const double* phi, const double* dphi, const double* X, const double* S, const double* E, int norm, double sc,
                           double* out) {
  if (dim == 2) ee_point_t<2>(nc, wg, phi, dphi, X, S, E, norm, sc, out);
  else ee_point_t<3>(nc, wg, phi, dphi, X, S, E, norm, sc, out);
}

// The element's sums over its points, ascending, every term added on its own as the reference's += do.  T[ig * (2 nt + 1) + ...]; res = {solNorm2 share, volume, err}
FH_HD inline void ee_element_sums(int ng, int nt, const double* T, double res[3]) {
#pragma clang fp contract(off)
  double sn = 0., vol = 0., err = 0.;
  const int st = 2 * nt + 1;
  for (int ig = 0; ig < ng; ig++) {
    const double* t = T + ig * st;
    for (int k = 0; k < nt; k++) sn += t[1 + k];
    for (int k = 0; k < nt; k++) err += t[1 + nt + k];
    vol += t[0];
  }
  res[0] = sn;
  res[1] = vol;
  res[2] = err;
}

FH_HD inline double ee_eps2(double threshold, double solNorm2, double volume) {
#pragma clang fp contract(off)
  return threshold * threshold * solNorm2 / volume;
}
FH_HD inline bool ee_strong(double err, double vol, double eps2) {
#pragma clang fp contract(off)
  return err > eps2 * vol;
}
FH_HD inline bool ee_weak(double err, double vol, double eps2, double neighbor_threshold) {
#pragma clang fp contract(off)
  return err > neighbor_threshold * eps2 * vol;
}
}  // namespace fherr
