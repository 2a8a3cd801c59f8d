// Hanging-node constraints (Mesh::GetAMRRestrictionAndAMRSolidMark, Mesh.cpp:1352-1830): what the searches of a box mesh (fh_mesh.cpp), of the arrays of an
// element mesh of any shape (fh_elemconstraints.cpp) and of a resident one (fh_elemconstraints.hip) share -- the raw entries a search writes, and their
// resolution into rows.
#pragma once
#include <vector>
#include "fh_fe_basis.h"

struct AmrRows {
  std::vector<int> hang;                 // sorted hanging dofs
  std::vector<int> ptr;                  // CSR over hang
  std::vector<int> master;
  std::vector<double> w;
};

// one write restriction[master][hanging] = v of the search, found by a coarse interface element of level Lc.  The searches hand them over in the order of the
// reference's loops -- (coarse level, fine level), coarse interface element, hanging node, local node -- in which a later write of a (master, hanging) pair
// replaces an earlier one
struct AmrTriple {
  int master, hanging, Lc;
  double v;
};

// mode 0: the reference's second half as written (Mesh.cpp:1711-1801), a genealogy walk from every real master; a node on the interfaces with two coarser levels
//         keeps its direct entry and loses the path through the intermediate hanging node: its row does not sum to one -- the reference's result.
// mode 1: a node is described by the coarsest level that finds it (the entries of the others are dropped), masters that hang themselves are expanded; rows sum to one.
// `ndof` bounds the dofs named.  Rows ascending in the hanging dof, masters ascending within a row; an expanded row may hold an exact 0.0.
void fh_amr_resolve(const std::vector<AmrTriple>& writes, int ndof, int mode, AmrRows& out);

// the CSR arrays of P_amr (n x n) from the rows: fh_build_amr_prolongator and fh_elem_mesh_amr_prolongator; false when a hanging dof is >= n
bool fh_amr_prolongator_csr(const AmrRows& R, int n, std::vector<int>& rowptr, std::vector<int>& col, std::vector<double>& val);

// the search on host arrays (the entry point fh_elem_amr_constraints_host, and the A/B partner of the device search): elem_dof[nel * 27], face_flag[nel * 6]
int fh_elem_amr_search_host(int dim, int nel, int nnode, const int* elem_geom, const int* elem_dof, const double* coords, const int* face_flag, const int* lev, int fe,
                            std::vector<AmrTriple>& writes);

// ---- what the host search and the kernel run alike ---------------------------------------------------------------------------------------------------------
// GetClosestPointInReferenceElement (PolynomialBases.cpp:1933-): the reference point of the element's node nearest to xp (the first of equal distances)
FH_HD inline void fh_amr_closest_node(int geom, int dim, int nl, const double* xv /* [nl * dim] */, const double* xp, double* xi) {
  int jmin = 0;
  double d2min = 1.0e100;
  for (int j = 0; j < nl; j++) {
    double d2 = 0.0;
    for (int d = 0; d < dim; d++) d2 += (xv[j * dim + d] - xp[d]) * (xv[j * dim + d] - xp[d]);
    if (d2 < d2min) {
      d2min = d2;
      jmin = j;
    }
  }
  fhfe::hd::node_ref(geom, jmin, xi);
}

// Newton inverse of the biquadratic map from the xi handed in; false when a Jacobian is singular (the point is dropped).  Stops below 1e-14 * scale or after 30 steps.
FH_HD inline bool fh_amr_inverse_map(int geom, int dim, int nl, const double* xv /* [nl * dim] */, const double* xp, double* xi) {
  double phi[27], dphi[81];
  double scale = 1.0;
  for (int k = 0; k < nl * dim; k++) scale = fmax(scale, fabs(xv[k]) + 1.0);
  for (int it = 0; it < 30; it++) {
    fhfe::hd::eval_basis(geom, fhfe::FE_BIQUADRATIC, xi, phi, dphi);
    double r[3] = {0, 0, 0}, J[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};   // J[b][a] = d x_b / d xi_a
    for (int j = 0; j < nl; j++)
      for (int b = 0; b < dim; b++) {
        r[b] += phi[j] * xv[j * dim + b];
        for (int a = 0; a < dim; a++) J[b][a] += dphi[j * dim + a] * xv[j * dim + b];
      }
    for (int b = 0; b < dim; b++) r[b] -= xp[b];
    double dx[3] = {0, 0, 0};
    if (dim == 2) {
      const double det = J[0][0] * J[1][1] - J[0][1] * J[1][0];
      if (det == 0.0) return false;
      dx[0] = (J[1][1] * r[0] - J[0][1] * r[1]) / det;
      dx[1] = (-J[1][0] * r[0] + J[0][0] * r[1]) / det;
    } else {
      const double c00 = J[1][1] * J[2][2] - J[1][2] * J[2][1], c01 = J[1][2] * J[2][0] - J[1][0] * J[2][2],
                   c02 = J[1][0] * J[2][1] - J[1][1] * J[2][0];
      const double det = J[0][0] * c00 + J[0][1] * c01 + J[0][2] * c02;
      if (det == 0.0) return false;
      const double inv[3][3] = {
          {c00 / det, (J[0][2] * J[2][1] - J[0][1] * J[2][2]) / det, (J[0][1] * J[1][2] - J[0][2] * J[1][1]) / det},
          {c01 / det, (J[0][0] * J[2][2] - J[0][2] * J[2][0]) / det, (J[0][2] * J[1][0] - J[0][0] * J[1][2]) / det},
          {c02 / det, (J[0][1] * J[2][0] - J[0][0] * J[2][1]) / det, (J[0][0] * J[1][1] - J[0][1] * J[1][0]) / det}};
      for (int a = 0; a < 3; a++) dx[a] = inv[a][0] * r[0] + inv[a][1] * r[1] + inv[a][2] * r[2];
    }
    double mx = 0.0;
    for (int a = 0; a < dim; a++) {
      xi[a] -= dx[a];
      mx = fmax(mx, fabs(dx[a]));
    }
    if (mx < 1e-14 * scale) return true;
  }
  return true;
}

// CheckIfPointIsInsideReferenceDomain{Hex, Tet, Wedge, Quad, Tri} (PolynomialBases.cpp:1484-1526)
FH_HD inline bool fh_amr_inside(int geom, const double* xi, double eps) {
  using namespace fhfe;
  const double th = 1. + eps;
  if (geom == GEOM_HEX) return fabs(xi[0]) < th && fabs(xi[1]) < th && fabs(xi[2]) < th;
  if (geom == GEOM_QUAD) return fabs(xi[0]) < th && fabs(xi[1]) < th;
  if (geom == GEOM_TRI) return xi[0] > -eps && xi[1] > -eps && xi[0] + xi[1] < th;
  if (geom == GEOM_TET) return xi[0] > -eps && xi[1] > -eps && xi[2] > -eps && xi[0] + xi[1] + xi[2] < th;
  if (geom == GEOM_WEDGE) return xi[0] > -eps && xi[1] > -eps && xi[0] + xi[1] < th && fabs(xi[2]) < th;
  return false;
}

// GetBoundingBox and GetConvexHullSphere with the tolerance 0.01 of Mesh.cpp:1509-1513: box[2 * d] = lo, box[2 * d + 1] = hi, then the centre and r^2
FH_HD inline void fh_amr_hull(int dim, int nl, const double* xv, double* box /* [6] */, double* xc /* [3] */, double* r2) {
  for (int d = 0; d < dim; d++) {
    double lo = xv[d], hi = xv[d], s = 0.0;
    for (int i = 0; i < nl; i++) {
      const double c = xv[i * dim + d];
      lo = fmin(lo, c);
      hi = fmax(hi, c);
      s += c;
    }
    const double pad = 0.01 * (hi - lo);
    box[2 * d] = lo - pad;
    box[2 * d + 1] = hi + pad;
    xc[d] = s / nl;
  }
  double m = 0.0;
  for (int i = 0; i < nl; i++) {
    double d2 = 0.0;
    for (int d = 0; d < dim; d++) d2 += (xv[i * dim + d] - xc[d]) * (xv[i * dim + d] - xc[d]);
    m = fmax(m, d2);
  }
  const double r = 1.01 * sqrt(m);
  *r2 = r * r;
}
FH_HD inline bool fh_amr_in_hull(int dim, const double* box, const double* xc, double r2, const double* xp) {
  double d2 = 0.0;
  bool in = true;
  for (int d = 0; d < dim; d++) {
    d2 += (xp[d] - xc[d]) * (xp[d] - xc[d]);
    in = in && xp[d] >= box[2 * d] && xp[d] <= box[2 * d + 1];
  }
  return in && !(d2 > r2);
}
