// What the five element bodies on the resident plan of the generic assembly share on the device: gen_element_pass (fh_generic.hip), form_element_pass
// (fh_quasilinear.hip), transient_element_pass (fh_transient.hip), system_element_pass (fh_system.hip) and system_transient_element_pass
// (fh_system_transient.hip, which calls the prologue, (A) and (B)).  Every body takes the Gauss points of an element
// through LDS a chunk at a time, L lanes per element, with a workgroup barrier between the phases; the phases they have in common are here, inlined into
// each, so that a change to one of them is made once:
//   eb_prologue          the kernel's first lines: sub-group, lane, slot, active, the tables (staged in LDS under TL) and the sub-group's LDS
//   (A)  eb_point_geometry    lane = Gauss point: Jacobian (Jac[a][b] = sum_n dphi_n/dxi_a x_n[b]), its inverse, det w, x_g; nodes ascending
//   (B)  eb_chunk_gradients   lanes over (point, node): G_n = Jac^-1 dphi_n
//   (C') eb_chunk_st          lanes over (point, node): S_n = G_n . grad u_g, T_n = c_u phi_n + c_g . G_n (the form and the transient body)
// The barriers stay in the bodies, where the phases can be read in their order.  Not every body calls every helper: a helper is optimised on its own before it
// is inlined, and where that gave a kernel another register allocation or schedule than the same text in the body, and the kernel lost time by it, the body
// keeps the text (the transient body (A), the form body (B), the system body its prologue and (B); kernel by kernel in profiles/elembody_share_isa.md).  A
// change to a phase is then made here and in those bodies.  The error-norm bodies (ee_jacobian_t, fh_elemerror_body.h) repeat the
// cofactors of (A) and stay apart on purpose: they are compiled under fp contract(off), bit for bit with a host compile, and these translation units
// contract -- one text for both would change the rounding on one side.
#pragma once
#include "fh_generic.h"

constexpr int QF_PT = 7;                     // a, a_u, c, c_u, c_g[3] of a Gauss point in the form and the transient body

struct EbGroup {
  int sub, lane, slot;             // sub-group of the workgroup, lane of the sub-group, the element's slot (0 where there is none)
  bool active;                     // the sub-group has an element; a tail sub-group keeps the barriers and touches nothing
  const double *w, *phi, *dphi;    // the shape's tables: in LDS under TL, else the global ones
  double* lds;                     // the sub-group's `per` doubles
};

// Every thread of the workgroup calls this (the staged tables are read after the body's first barrier).  A tail sub-group gets slot 0: no address is
// formed past the buffers, read or not.
template <int L, bool TL>
__device__ __forceinline__ EbGroup eb_prologue(double* smem, int nslot, int nc, int ng, int dim, int per, const double* gw, const double* gphi, const double* gdphi) {
  EbGroup g;
  const int ntab = TL ? ng + ng * nc + ng * nc * dim : 0;
  g.sub = threadIdx.x / L, g.lane = threadIdx.x % L;
  const int slot = blockIdx.x * (GP_THREADS / L) + g.sub;
  g.active = slot < nslot;
  g.slot = g.active ? slot : 0;
  if (TL) {
    double* tw = smem;
    double* tphi = tw + ng;
    double* tdphi = tphi + ng * nc;
    for (int t = threadIdx.x; t < ng; t += GP_THREADS) tw[t] = gw[t];
    for (int t = threadIdx.x; t < ng * nc; t += GP_THREADS) tphi[t] = gphi[t];
    for (int t = threadIdx.x; t < ng * nc * dim; t += GP_THREADS) tdphi[t] = gdphi[t];
    g.w = tw, g.phi = tphi, g.dphi = tdphi;
  } else {
    g.w = gw, g.phi = gphi, g.dphi = gdphi;
  }
  g.lds = smem + ntab + (size_t)g.sub * per;
  return g;
}

// The lane's entry table (ei[k], ej[k] of e = lane + L k) stays in the bodies: as a helper it either goes to scratch memory or turns the branch around the
// division into selects (profiles/elembody_share_isa.md).

// (A) for one Gauss point.  X[nc][3]: the nodes; dp[nc][dim], ph[nc]: the point's rows of dphi and phi; wg: the address of its weight (read here, after the
// inverse is stored, not by the caller before the Jacobian loop).  JI[9] gets the inverse (zeros beyond dim), *detw the determinant times the weight, and x_g is
// added to xg[0 .. dim), which the caller has cleared: each goes where the body keeps it.
__device__ __forceinline__ void eb_point_geometry(const double* X, const double* dp, const double* ph, const double* wg, int nc, int dim, double* JI, double* detw, double* xg) {
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
    for (int p = 0; p < 3; p++) JI[q * 3 + p] = Ji[q][p];
  *detw = det * *wg;
  for (int n = 0; n < nc; n++) {
    const double pn = ph[n];
    for (int q = 0; q < dim; q++) xg[q] += X[n * 3 + q] * pn;
  }
}

// (B) for the chunk of gc points that starts at g0.  The inverse of point l is at JI + l jis; G[gc][ns][3].  ALL3: all three components are written, zeros
// beyond dim (the bodies whose later phases read three); otherwise the first dim only (the Poisson body).
template <int L, bool ALL3>
__device__ __forceinline__ void eb_chunk_gradients(int lane, int g0, int gc, int nc, int ns, int dim, const double* dphi, const double* JI, int jis, double* G) {
  for (int t = lane; t < gc * nc; t += L) {
    const int l = t / nc, n = t - l * nc;
    const double* dp = dphi + ((size_t)(g0 + l) * nc + n) * dim;
    for (int q = 0; q < (ALL3 ? 3 : dim); q++) {
      double sacc = 0.0;
      if (q < dim)
        for (int p = 0; p < dim; p++) sacc += JI[l * jis + q * 3 + p] * dp[p];
      G[(l * ns + n) * 3 + q] = sacc;
    }
  }
}

// (C') for the same chunk: GU[gc][3] is grad u_g, PT[gc][QF_PT] the point's (a, a_u, c, c_u, c_g[3]); ST[gc][nc][2] gets S and T
template <int L>
__device__ __forceinline__ void eb_chunk_st(int lane, int g0, int gc, int nc, int dim, const double* phi, const double* G, const double* GU, const double* PT, double* ST) {
  for (int t = lane; t < gc * nc; t += L) {
    const int l = t / nc, n = t - l * nc;
    const double* gn = G + (l * nc + n) * 3;
    double S = 0.0;
    for (int q = 0; q < dim; q++) S += gn[q] * GU[l * 3 + q];
    double T = PT[l * QF_PT + 3] * phi[(size_t)(g0 + l) * nc + n];
    for (int q = 0; q < dim; q++) T += PT[l * QF_PT + 4 + q] * gn[q];
    ST[(l * nc + n) * 2] = S;
    ST[(l * nc + n) * 2 + 1] = T;
  }
}
