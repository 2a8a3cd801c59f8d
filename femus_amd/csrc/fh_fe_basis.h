// The reference elements' tables and basis functions as code that both the host and a kernel can run: fh_fe.cpp serves its tables from them, the hanging-node
// search of an element mesh (fh_elemconstraints.hip) evaluates them at the points its inverse map finds.  One statement of every polynomial: the host tables
// keep their bits, a kernel may contract products and sums differently (a few ulp).
#pragma once
#include <hip/hip_runtime.h>
#include <cmath>
#include "fh_fe.h"
#define FH_HD __host__ __device__

namespace fhfe {
namespace hd {

// local node coordinates of the FEMuS HEX27 / QUAD9 ordering: 8 vertices, 12 edge mid-points (bottom ring,
// top ring, vertical), 4 side-face centres (y-, x+, y+, x-), bottom, top, centre.
static constexpr signed char XC_HEX[27][3] = {
    {-1, -1, -1}, {1, -1, -1}, {1, 1, -1}, {-1, 1, -1}, {-1, -1, 1}, {1, -1, 1}, {1, 1, 1}, {-1, 1, 1},
    {0, -1, -1},  {1, 0, -1},  {0, 1, -1}, {-1, 0, -1}, {0, -1, 1},  {1, 0, 1},  {0, 1, 1}, {-1, 0, 1},
    {-1, -1, 0},  {1, -1, 0},  {1, 1, 0},  {-1, 1, 0},  {0, -1, 0},  {1, 0, 0},  {0, 1, 0}, {-1, 0, 0},
    {0, 0, -1},   {0, 0, 1},   {0, 0, 0}};
static constexpr signed char XC_QUAD[9][2] = {{-1, -1}, {1, -1}, {1, 1}, {-1, 1}, {0, -1}, {1, 0}, {0, 1}, {-1, 0}, {0, 0}};
// EDGE3 (1d/Edge.cpp:22-30): the two end points, then the middle
static constexpr signed char XC_LINE[3][1] = {{-1}, {1}, {0}};
// TRI7 (2d/Triangle.cpp:27-37): vertices, edge middles, centre; TRI_IND = the (i, j) selectors of the basis polynomials (0, 1, 2 along an edge, 7 the bubble);
// children (Triangle.cpp:48-53): three at the vertices, the fourth the middle triangle {4, 5, 3}; faces (:55-59)
static constexpr double XC_TRI[7][2] = {{0, 0}, {1, 0}, {0, 1}, {0.5, 0}, {0.5, 0.5}, {0, 0.5}, {1. / 3., 1. / 3.}};
static constexpr int TRI_IND[7][2] = {{0, 0}, {2, 0}, {0, 2}, {1, 0}, {1, 1}, {0, 1}, {7, 7}};
static constexpr int TRI_F2C[4][3] = {{0, 3, 5}, {3, 1, 4}, {5, 4, 2}, {4, 5, 3}};
static constexpr int TRI_FACE[3][3] = {{0, 1, 3}, {1, 2, 4}, {2, 0, 5}};
// TET15 (3d/Tetrahedron.cpp:24-100): vertices, edge middles, the four face centres, the centre; selectors of the P1 / P2 terms; the eight
// children (four at the vertices, four out of the inner octahedron); faces = (three vertices, three middles)
static constexpr double XC_TET[15][3] = {{0, 0, 0}, {1, 0, 0}, {0, 1, 0}, {0, 0, 1}, {0.5, 0, 0}, {0.5, 0.5, 0}, {0, 0.5, 0}, {0., 0, 0.5}, {0.5, 0., 0.5}, {0, 0.5, 0.5},
                                     {1. / 3., 1. / 3., 0.}, {1. / 3., 0., 1. / 3.}, {1. / 3., 1. / 3., 1. / 3.}, {0., 1. / 3., 1. / 3.}, {0.25, 0.25, 0.25}};
static constexpr int TET_IND[10][3] = {{0, 0, 0}, {2, 0, 0}, {0, 2, 0}, {0, 0, 2}, {1, 0, 0}, {1, 1, 0}, {0, 1, 0}, {0, 0, 1}, {1, 0, 1}, {0, 1, 1}};
static constexpr int TET_F2C[8][4] = {{0, 4, 6, 7}, {4, 1, 5, 8}, {6, 5, 2, 9}, {7, 8, 9, 3}, {5, 6, 4, 7}, {8, 7, 5, 4}, {7, 9, 8, 5}, {9, 5, 7, 6}};
static constexpr int TET_FACE[4][7] = {{0, 2, 1, 6, 5, 4, 10}, {0, 1, 3, 4, 8, 7, 11}, {1, 2, 3, 5, 9, 8, 12}, {2, 0, 3, 6, 7, 9, 13}};
// WEDGE21 (3d/Wedge.cpp:23-140) = TRI7 x EDGE3: six vertices, nine edge middles (bottom ring, top ring, vertical), three quadrilateral-face centres, the two
// triangle-face centres, the centre; selectors (triangle pair, line index); eight children (four per layer); faces 0 .. 2 quadrilaterals (QUAD9 order), 3 .. 4 triangles (TRI7)
static constexpr double XC_WDG[21][3] = {{0, 0, -1}, {1, 0, -1}, {0, 1, -1}, {0, 0, 1}, {1, 0, 1}, {0, 1, 1}, {0.5, 0, -1}, {0.5, 0.5, -1}, {0, 0.5, -1}, {0.5, 0, 1}, {0.5, 0.5, 1},
                                     {0, 0.5, 1}, {0, 0, 0}, {1, 0, 0}, {0, 1, 0}, {0.5, 0, 0}, {0.5, 0.5, 0}, {0, 0.5, 0}, {1. / 3., 1. / 3., -1}, {1. / 3., 1. / 3., 1}, {1. / 3., 1. / 3., 0}};
static constexpr int WDG_IND[21][3] = {{0, 0, 0}, {2, 0, 0}, {0, 2, 0}, {0, 0, 2}, {2, 0, 2}, {0, 2, 2}, {1, 0, 0}, {1, 1, 0}, {0, 1, 0}, {1, 0, 2}, {1, 1, 2}, {0, 1, 2}, {0, 0, 1}, {2, 0, 1},
                                   {0, 2, 1}, {1, 0, 1}, {1, 1, 1}, {0, 1, 1}, {7, 7, 0}, {7, 7, 2}, {7, 7, 1}};
static constexpr int WDG_F2C[8][6] = {{0, 6, 8, 12, 15, 17}, {6, 1, 7, 15, 13, 16}, {8, 7, 2, 17, 16, 14}, {7, 8, 6, 16, 17, 15}, {12, 15, 17, 3, 9, 11}, {15, 13, 16, 9, 4, 10},
                                  {17, 16, 14, 11, 10, 5}, {16, 17, 15, 10, 11, 9}};
static constexpr int WDG_FACE[5][9] = {{0, 1, 4, 3, 6, 13, 9, 12, 15}, {1, 2, 5, 4, 7, 14, 10, 13, 16}, {2, 0, 3, 5, 8, 12, 11, 14, 17}, {0, 2, 1, 8, 7, 6, 18, -1, -1}, {3, 4, 5, 9, 10, 11, 19, -1, -1}};
FH_HD inline int dim_of(int geom) { return (geom == GEOM_HEX || geom == GEOM_TET || geom == GEOM_WEDGE) ? 3 : (geom == GEOM_QUAD || geom == GEOM_TRI) ? 2 : 1; }
FH_HD inline int nloc_of(int geom) { return geom == GEOM_HEX ? 27 : geom == GEOM_QUAD ? 9 : geom == GEOM_TRI ? 7 : geom == GEOM_TET ? 15 : geom == GEOM_WEDGE ? 21 : 3; }
FH_HD inline int nvert_of(int geom) { return geom == GEOM_HEX ? 8 : (geom == GEOM_QUAD || geom == GEOM_TET) ? 4 : geom == GEOM_TRI ? 3 : geom == GEOM_WEDGE ? 6 : 2; }
FH_HD inline int nedge_end_of(int geom) { return geom == GEOM_HEX ? 20 : geom == GEOM_QUAD ? 8 : geom == GEOM_TRI ? 6 : geom == GEOM_TET ? 10 : geom == GEOM_WEDGE ? 15 : 2; }
FH_HD inline int nfaces_of(int geom) { return geom == GEOM_HEX ? 6 : (geom == GEOM_QUAD || geom == GEOM_TET) ? 4 : geom == GEOM_TRI ? 3 : geom == GEOM_WEDGE ? 5 : 2; }
// (on the line the "quadratic" family IS the three-node one: NVE[5] = {2, 3, 3, 1, 2}, GeomElTypeEnum)
FH_HD inline int ndofs_of(int geom, int fe) {
  return fe == FE_LINEAR ? nvert_of(geom) : fe == FE_SERENDIPITY ? (geom == GEOM_LINE ? 3 : nedge_end_of(geom)) : fe == FE_CONSTANT ? 1 : nloc_of(geom);
}

FH_HD inline int xc(int geom, int node, int d) { return geom == GEOM_HEX ? XC_HEX[node][d] : geom == GEOM_QUAD ? XC_QUAD[node][d] : XC_LINE[node][d]; }
FH_HD inline void node_ref(int geom, int node, double* pt) {
  for (int k = 0; k < dim_of(geom); k++) pt[k] = geom == GEOM_TRI ? XC_TRI[node][k] : geom == GEOM_TET ? XC_TET[node][k] : geom == GEOM_WEDGE ? XC_WDG[node][k] : (double)xc(geom, node, k);
}
// ---- 1-D Lagrange polynomials, same expressions as Edge.hpp:72-104 ------------------------------------
FH_HD inline double lagL(double x, int i) { return (!i) * 0.5 * (1. - x) + !(i - 2) * 0.5 * (1. + x); }
FH_HD inline double dlagL(double, int i) { return (!i) * (-0.5) + !(i - 2) * 0.5; }
FH_HD inline double lagB(double x, int i) { return !i * 0.5 * x * (x - 1.) + !(i - 1) * (1. - x) * (1. + x) + !(i - 2) * 0.5 * x * (1. + x); }
FH_HD inline double dlagB(double x, int i) { return !i * (x - 0.5) + !(i - 1) * (-2. * x) + !(i - 2) * (x + 0.5); }

FH_HD inline double d2lagB(int i) { return !i * 1.0 + !(i - 1) * (-2.0) + !(i - 2) * 1.0; }
// "quadratic" 1-D factors of the serendipity families (Edge.hpp:81-91): linear at the end nodes, the bubble at the middle one
FH_HD inline double lagQ(double x, int i) { return !i * (0.5) * (1. - x) + !(i - 1) * (1. - x) * (1. + x) + !(i - 2) * (0.5) * (1. + x); }
FH_HD inline double dlagQ(double x, int i) { return (!i) * (-0.5) + !(i - 1) * (-2. * x) + !(i - 2) * (0.5); }
FH_HD inline double d2lagQ(int i) { return !(i - 1) * (-2.); }

// Triangle families (2d/Triangle.hpp:69-181): P1, P2 and P2 enriched with the cubic bubble (TRI7), selected by the (i, j) pair of the node as the 1-D factors
// above are by their index; the terms in the reference's order (the tables are compared bit for bit with the ones its compiled classes give).
// out: phi, d/dx, d/dy, d2/dx2, d2/dy2, d2/dxdy
FH_HD inline void tri_node(int fe, int i, int j, double x, double y, double out[6]) {
  for (int k = 0; k < 6; k++) out[k] = 0.0;
  if (fe == FE_LINEAR) {
    out[0] = (!i * !j) * (1. - x - y) + !(i - 2) * x + !(j - 2) * y;
    out[1] = -(!i * !j) + !(i - 2);
    out[2] = -(!i * !j) + !(j - 2);
  } else if (fe == FE_SERENDIPITY) {
    out[0] = !i * (!j * (1. - x - y) * (1. - 2. * x - 2. * y) + !(j - 1) * 4. * y * (1. - x - y) + !(j - 2) * (-y + 2. * y * y)) +
             !(i - 1) * (!j * 4. * x * (1. - x - y) + !(j - 1) * 4. * x * y) + !(i - 2) * (!j * (-x + 2. * x * x));
    out[1] = !i * (!j * (-3. + 4. * x + 4. * y) + !(j - 1) * y * (-4.)) + !(i - 1) * (!j * 4. * (1. - 2. * x - y) + !(j - 1) * y * (4.)) + !(i - 2) * (!j * (-1 + 4. * x));
    out[2] = !j * (!i * (-3. + 4. * y + 4. * x) + !(i - 1) * x * (-4.)) + !(j - 1) * (!i * 4. * (1. - 2. * y - x) + !(i - 1) * x * (4.)) + !(j - 2) * (!i * (-1 + 4. * y));
    out[3] = !j * ((!i) * 4. + !(i - 1) * (-8.) + !(i - 2) * 4.);
    out[4] = !i * ((!j) * 4. + !(j - 1) * (-8.) + !(j - 2) * 4.);
    out[5] = ((!i) * (!j) + !(i - 1) * !(j - 1)) * 4. + (!(i - 1) * (!j) + (!i) * !(j - 1)) * (-4.);
  } else {
    const double b3 = 3. * x * y * (1 - x - y), bx = y - 2. * x * y - y * y, by = x - x * x - 2. * x * y, bxy = 1 - 2. * x - 2. * y;      // (the products associate as in the reference's inline terms)
    out[0] = !i * (!j * ((1. - x - y) * (1. - 2. * x - 2. * y) + b3) + !(j - 1) * 4. * (y * (1. - x - y) - b3) + !(j - 2) * (-y + 2. * y * y + b3)) +
             !(i - 1) * (!j * 4. * (x * (1. - x - y) - b3) + !(j - 1) * 4. * (x * y - b3)) + !(i - 2) * (!j * (-x + 2. * x * x + b3)) +
             !(i - 7) * (!(j - 7) * 27. * x * y * (1 - x - y));
    out[1] = !i * (!j * (-3. + 4. * x + 4. * y + 3. * bx) + !(j - 1) * 4. * (-y - 3. * bx) + !(j - 2) * 3. * bx) +
             !(i - 1) * (!j * 4. * (1. - 2. * x - y - 3. * bx) + !(j - 1) * 4. * (y - 3. * bx)) + !(i - 2) * (!j * (-1 + 4. * x + 3. * bx)) + !(i - 7) * (!(j - 7) * 27. * bx);
    out[2] = !j * (!i * (-3. + 4. * y + 4. * x + 3. * by) + !(i - 1) * 4. * (-x - 3. * by) + !(i - 2) * 3. * by) +
             !(j - 1) * (!i * 4. * (1. - 2. * y - x - 3. * by) + !(i - 1) * 4. * (x - 3. * by)) + !(j - 2) * (!i * (-1 + 4. * y + 3. * by)) + !(j - 7) * (!(i - 7) * 27. * by);
    out[3] = !i * (!j * (4. - 6. * y) + !(j - 1) * 4. * (6. * y) + !(j - 2) * (-6. * y)) + !(i - 1) * (!j * 4. * (-2. + 6. * y) + !(j - 1) * 4. * (6. * y)) +
             !(i - 2) * (!j * (4. - 6. * y)) + !(i - 7) * (!(j - 7) * (-54. * y));
    out[4] = !j * (!i * (4. - 6. * x) + !(i - 1) * 4. * (6. * x) + !(i - 2) * (-6. * x)) + !(j - 1) * (!i * 4. * (-2. + 6. * x) + !(i - 1) * 4. * (6. * x)) +
             !(j - 2) * (!i * (4. - 6. * x)) + !(j - 7) * (!(i - 7) * (-54. * x));
    out[5] = !j * (!i * (4. + 3. * bxy) + !(i - 1) * 4. * (-1. - 3. * bxy) + !(i - 2) * 3. * bxy) +
             !(j - 1) * (!i * 4. * (-1. - 3. * bxy) + !(i - 1) * 4. * (1. - 3. * bxy)) + !(j - 2) * (!i * (3. * bxy)) + !(j - 7) * (!(i - 7) * 27. * bxy);
  }
}

// Tetrahedron families (3d/Tetrahedron.cpp: TetLinear, TetQuadratic), selected by the (i, j, k) triple of the node; the terms in the reference's order.
// out: phi, d/dx, d/dy, d/dz, then xx, yy, zz, xy, yz, zx (the second derivatives of P2 are the constants 4, -8, -4 of its barycentric products)
FH_HD inline void tet_node(int fe, int i, int j, int k, double x, double y, double z, double out[10]) {
  for (int q = 0; q < 10; q++) out[q] = 0.0;
  if (fe == FE_LINEAR) {
    out[0] = (!i * !j * !k) * (1. - x - y - z) + !(i - 2) * x + !(j - 2) * y + !(k - 2) * z;
    out[1] = -(!i * !j * !k) + !(i - 2);
    out[2] = -(!i * !j * !k) + !(j - 2);
    out[3] = -(!i * !j * !k) + !(k - 2);
    return;
  }
  const double t = 1. - (x + y + z);
  out[0] = !i * (!j * (!k * t * (2. * t - 1.) + !(k - 1) * 4. * z * t + !(k - 2) * (-z + 2. * z * z)) + !(j - 1) * (!k * 4. * y * t + !(k - 1) * 4. * y * z) +
                 !(j - 2) * (!k * (-y + 2. * y * y))) +
           !(i - 1) * (!j * (!k * 4. * x * t + !(k - 1) * 4. * x * z) + !(j - 1) * (!k * 4. * x * y)) + !(i - 2) * (!j * (!k * (-x + 2. * x * x)));
  out[1] = !i * (!j * (!k * (-4. * t + 1.) + !(k - 1) * (-4.) * z) + !(j - 1) * (!k * (-4.) * y)) +
           !(i - 1) * (!j * (!k * 4. * (t - x) + !(k - 1) * 4. * z) + !(j - 1) * (!k * 4. * y)) + !(i - 2) * (!j * (!k * (-1. + 4. * x)));
  out[2] = !i * (!j * (!k * (-4. * t + 1.) + !(k - 1) * (-4.) * z) + !(j - 1) * (!k * 4. * (t - y) + !(k - 1) * 4. * z) + !(j - 2) * (!k * (-1. + 4. * y))) +
           !(i - 1) * (!j * (!k * (-4.) * x) + !(j - 1) * (!k * 4. * x));
  out[3] = !i * (!j * (!k * (-4. * t + 1.) + !(k - 1) * 4. * (t - z) + !(k - 2) * (-1 + 4. * z)) + !(j - 1) * (!k * (-4.) * y + !(k - 1) * 4. * y)) +
           !(i - 1) * (!j * (!k * (-4.) * x + !(k - 1) * 4. * x));
  // Hessian of P2: node (i, j, k) -> barycentric pair; phi = L_a (2 L_a - 1) at a vertex, 4 L_a L_b on an edge; L_0 = t has gradient (-1, -1, -1), L_m the unit vector e_m
  int a = -1, b = -1;                                   // barycentric indices 0 (t), 1 (x), 2 (y), 3 (z) of the node's one or two factors
  const int idx[3] = {i, j, k};
  for (int m = 0; m < 3; m++)
    if (idx[m] == 2) a = b = m + 1;
  if (a < 0) {
    for (int m = 0; m < 3; m++)
      if (idx[m] == 1) (a < 0 ? a : b) = m + 1;
    if (a < 0) a = b = 0;                               // (0, 0, 0): the vertex at the origin
    else if (b < 0) b = 0;                              // one index 1: the edge towards the origin
  }
  auto g = [](int L, int d) { return L == 0 ? -1.0 : (L == d + 1 ? 1.0 : 0.0); };
  const int pr[6][2] = {{0, 0}, {1, 1}, {2, 2}, {0, 1}, {1, 2}, {2, 0}};
  for (int q = 0; q < 6; q++) {
    const int p = pr[q][0], r = pr[q][1];
    out[4 + q] = (a == b) ? 4.0 * g(a, p) * g(a, r) : 4.0 * (g(a, p) * g(b, r) + g(b, p) * g(a, r));
  }
}

// TetBiquadratic (3d/Tetrahedron.cpp:325-600) in hierarchical form: with the barycentric coordinates L0 = 1 - x - y - z, L1 = x, L2 = y, L3 = z, the face monomials
// m_f = L_a L_b L_c and q = L0 L1 L2 L3, the reference's polynomials are
//   vertex v: L_v (2 L_v - 1) + 3 sum_{f contains v} m_f - 4 q      edge (a, b): 4 L_a L_b - 12 sum_{f contains a and b} m_f + 32 q
//   face f:   27 m_f - 108 q                                          centre:      256 q
// (the same functions, summed in another order than the reference's expanded terms: the tables agree to rounding, 1e-14, not bit for bit)
FH_HD inline void tet15(double x, double y, double z, double P[15], double D[15][3]) {
  const double L[4] = {1. - x - y - z, x, y, z};
  const double G[4][3] = {{-1, -1, -1}, {1, 0, 0}, {0, 1, 0}, {0, 0, 1}};
  constexpr int EV[6][2] = {{0, 1}, {1, 2}, {2, 0}, {0, 3}, {1, 3}, {2, 3}};            // local nodes 4 .. 9
  constexpr int FV[4][3] = {{0, 2, 1}, {0, 1, 3}, {1, 2, 3}, {2, 0, 3}};                // local nodes 10 .. 13 (faceDofs)
  double m[4], dm[4][3], q = L[0] * L[1] * L[2] * L[3], dq[3];
  for (int d = 0; d < 3; d++) dq[d] = G[0][d] * L[1] * L[2] * L[3] + L[0] * G[1][d] * L[2] * L[3] + L[0] * L[1] * G[2][d] * L[3] + L[0] * L[1] * L[2] * G[3][d];
  for (int f = 0; f < 4; f++) {
    const int a = FV[f][0], b = FV[f][1], c = FV[f][2];
    m[f] = L[a] * L[b] * L[c];
    for (int d = 0; d < 3; d++) dm[f][d] = G[a][d] * L[b] * L[c] + L[a] * G[b][d] * L[c] + L[a] * L[b] * G[c][d];
  }
  auto on_face = [&](int f, int v) { return FV[f][0] == v || FV[f][1] == v || FV[f][2] == v; };
  for (int v = 0; v < 4; v++) {
    P[v] = L[v] * (2. * L[v] - 1.) - 4. * q;
    for (int d = 0; d < 3; d++) D[v][d] = (4. * L[v] - 1.) * G[v][d] - 4. * dq[d];
    for (int f = 0; f < 4; f++)
      if (on_face(f, v)) {
        P[v] += 3. * m[f];
        for (int d = 0; d < 3; d++) D[v][d] += 3. * dm[f][d];
      }
  }
  for (int e = 0; e < 6; e++) {
    const int a = EV[e][0], b = EV[e][1];
    P[4 + e] = 4. * L[a] * L[b] + 32. * q;
    for (int d = 0; d < 3; d++) D[4 + e][d] = 4. * (G[a][d] * L[b] + L[a] * G[b][d]) + 32. * dq[d];
    for (int f = 0; f < 4; f++)
      if (on_face(f, a) && on_face(f, b)) {
        P[4 + e] -= 12. * m[f];
        for (int d = 0; d < 3; d++) D[4 + e][d] -= 12. * dm[f][d];
      }
  }
  for (int f = 0; f < 4; f++) {
    P[10 + f] = 27. * m[f] - 108. * q;
    for (int d = 0; d < 3; d++) D[10 + f][d] = 27. * dm[f][d] - 108. * dq[d];
  }
  P[14] = 256. * q;
  for (int d = 0; d < 3; d++) D[14][d] = 256. * dq[d];
}

// Prism families (3d/Wedge.cpp): linear and biquadratic = the triangle's function times the line's (WedgeLinear, WedgeBiquadratic); the 15-node "quadratic" one
// (WedgeQuadratic) in the reference's terms.  out: phi, d/dx, d/dy, d/dz, then xx, yy, zz, xy, yz, zx (the second derivatives of the 15-node family are not
// served: its tables are refused)
FH_HD inline void wedge_node(int fe, int i, int j, int k, double x, double y, double z, double out[10]) {
  for (int q = 0; q < 10; q++) out[q] = 0.0;
  if (fe != FE_SERENDIPITY) {
    double t[6];
    tri_node(fe, i, j, x, y, t);
    const double l = fe == FE_LINEAR ? lagL(z, k) : lagB(z, k), dl = fe == FE_LINEAR ? dlagL(z, k) : dlagB(z, k), d2l = fe == FE_LINEAR ? 0.0 : d2lagB(k);
    out[0] = t[0] * l;
    out[1] = t[1] * l;
    out[2] = t[2] * l;
    out[3] = t[0] * dl;
    out[4] = t[3] * l;
    out[5] = t[4] * l;
    out[6] = t[0] * d2l;
    out[7] = t[5] * l;
    out[8] = t[2] * dl;
    out[9] = t[1] * dl;
    return;
  }
  const double t = 1. - (x + y);
  out[0] = !i * (!j * (!k * t * (-2. + 2. * t - z) * (1. - z) * 0.5 + !(k - 1) * t * (1. - z * z) + !(k - 2) * t * (-2. + 2. * t + z) * (1. + z) * 0.5) +
                 !(j - 1) * (!k * 2. * y * t * (1. - z) + !(k - 2) * 2. * y * t * (1. + z)) +
                 !(j - 2) * (!k * y * (-2. + 2. * y - z) * (1. - z) * 0.5 + !(k - 1) * y * (1. - z * z) + !(k - 2) * y * (-2. + 2. * y + z) * (1. + z) * 0.5)) +
           !(i - 1) * (!j * (!k * 2. * x * t * (1. - z) + !(k - 2) * 2. * x * t * (1. + z)) + !(j - 1) * (!k * 2. * x * y * (1. - z) + !(k - 2) * 2. * x * y * (1. + z))) +
           !(i - 2) * ((!k * x * (-2. + 2. * x - z) * (1. - z) * 0.5 + !(k - 1) * x * (1. - z * z) + !(k - 2) * x * (-2. + 2. * x + z) * (1. + z) * 0.5));
  out[1] = !i * (!j * (!k * (1. - 2. * t + 0.5 * z) * (1. - z) + !(k - 1) * (z * z - 1.) + !(k - 2) * (1. - 2. * t - 0.5 * z) * (1. + z)) +
                 !(j - 1) * (!k * (-2.) * y * (1. - z) + !(k - 2) * (-2.) * y * (1. + z))) +
           !(i - 1) * (!j * (!k * 2. * (1. - z) * (1. - 2. * x - y) + !(k - 2) * 2. * (1. + z) * (1. - 2. * x - y)) + !(j - 1) * (!k * 2. * y * (1. - z) + !(k - 2) * 2. * y * (1. + z))) +
           !(i - 2) * ((!k * (-1. + 2. * x - 0.5 * z) * (1. - z) + !(k - 1) * (1. - z * z) + !(k - 2) * (-1. + 2. * x + 0.5 * z) * (1. + z)));
  out[2] = !i * (!j * (!k * (1. - 2. * t + 0.5 * z) * (1. - z) + !(k - 1) * (z * z - 1.) + !(k - 2) * (1. - 2. * t - 0.5 * z) * (1. + z)) +
                 !(j - 1) * (!k * 2. * (1 - z) * (1. - x - 2. * y) + !(k - 2) * 2. * (1 + z) * (1. - x - 2. * y)) +
                 !(j - 2) * (!k * (-1. + 2. * y - 0.5 * z) * (1. - z) + !(k - 1) * (1. - z * z) + !(k - 2) * (-1. + 2. * y + 0.5 * z) * (1. + z))) +
           !(i - 1) * (!j * (!k * (-2.) * x * (1. - z) + !(k - 2) * (-2.) * x * (1. + z)) + !(j - 1) * (!k * 2. * x * (1. - z) + !(k - 2) * 2. * x * (1. + z)));
  out[3] = !i * (!j * (!k * t * (0.5 - t + z) + !(k - 1) * (-2.) * t * z + !(k - 2) * t * (-0.5 + t + z)) + !(j - 1) * (!k * (-2.) * y * t + !(k - 2) * 2. * y * t) +
                 !(j - 2) * (!k * y * (0.5 - y + z) + !(k - 1) * (-2.) * y * z + !(k - 2) * y * (-0.5 + y + z))) +
           !(i - 1) * (!j * (!k * (-2.) * x * t + !(k - 2) * 2. * x * t) + !(j - 1) * (!k * (-2.) * x * y + !(k - 2) * 2. * x * y)) +
           !(i - 2) * ((!k * x * (0.5 - x + z) + !(k - 1) * (-2.) * x * z + !(k - 2) * x * (-0.5 + x + z)));
}

// Serendipity bases, the expressions of QuadQuadratic / HexQuadratic term by term and in their order (the tables are compared bit for bit with the ones the
// reference's compiled classes give): a vertex function is the product of the three (two) linear factors times (-2 + ix x + jx y + kx z) ((-1 + ...) in 2-D),
// an edge function the plain product.  out: phi, d/dx, d/dy, d/dz, then xx, yy, zz, xy, yz, zx (2-D: phi, dx, dy, -, xx, yy, -, xy)
FH_HD inline void serendipity_node(int geom, int j, const double* x, double out[10]) {
  const int d = dim_of(geom);
  int I[3] = {1, 1, 1};
  for (int k = 0; k < d; k++) I[k] = xc(geom, j, k) + 1;
  for (int k = 0; k < 10; k++) out[k] = 0.0;
  if (d == 2) {
    const double ix = I[0] - 1., jx = I[1] - 1.;
    const double l0 = lagQ(x[0], I[0]), l1 = lagQ(x[1], I[1]), d0 = dlagQ(x[0], I[0]), d1 = dlagQ(x[1], I[1]), s0 = d2lagQ(I[0]), s1 = d2lagQ(I[1]);
    if (fabs(ix * jx) == 0) {
      out[0] = l0 * l1;
      out[1] = d0 * l1;
      out[2] = l0 * d1;
      out[4] = s0 * l1;
      out[5] = l0 * s1;
      out[7] = d0 * d1;
    } else {
      const double s = -1. + ix * x[0] + jx * x[1];
      out[0] = s * l0 * l1;
      out[1] = l1 * (ix * l0 + s * d0);
      out[2] = l0 * (jx * l1 + s * d1);
      out[4] = l1 * (2. * ix * d0 + s * s0);
      out[5] = l0 * (2. * jx * d1 + s * s1);
      out[7] = ix * l0 * d1 + jx * l1 * d0 + s * d0 * d1;
    }
    return;
  }
  const double ix = I[0] - 1., jx = I[1] - 1., kx = I[2] - 1.;
  const double l0 = lagQ(x[0], I[0]), l1 = lagQ(x[1], I[1]), l2 = lagQ(x[2], I[2]);
  const double d0 = dlagQ(x[0], I[0]), d1 = dlagQ(x[1], I[1]), d2 = dlagQ(x[2], I[2]);
  const double s0 = d2lagQ(I[0]), s1 = d2lagQ(I[1]), s2 = d2lagQ(I[2]);
  if (fabs(ix * jx * kx) == 0) {
    out[0] = l0 * l1 * l2;
    out[1] = d0 * l1 * l2;
    out[2] = l0 * d1 * l2;
    out[3] = l0 * l1 * d2;
    out[4] = s0 * l1 * l2;
    out[5] = l0 * s1 * l2;
    out[6] = l0 * l1 * s2;
    out[7] = d0 * d1 * l2;
    out[8] = l0 * d1 * d2;
    out[9] = d0 * l1 * d2;
  } else {
    const double s = -2. + ix * x[0] + jx * x[1] + kx * x[2];
    out[0] = s * l0 * l1 * l2;
    out[1] = l1 * l2 * (ix * l0 + s * d0);
    out[2] = l0 * l2 * (jx * l1 + s * d1);
    out[3] = l0 * l1 * (kx * l2 + s * d2);
    out[4] = l1 * l2 * (2. * ix * d0 + s * s0);
    out[5] = l2 * l0 * (2. * jx * d1 + s * s1);
    out[6] = l0 * l1 * (2. * kx * d2 + s * s2);
    out[7] = l2 * (ix * l0 * d1 + jx * l1 * d0 + s * d0 * d1);
    out[8] = l0 * (jx * l1 * d2 + kx * l2 * d1 + s * d1 * d2);
    out[9] = l1 * (kx * l2 * d0 + ix * l0 * d2 + s * d2 * d0);
  }
}
FH_HD inline void eval_basis(int geom, int fe, const double* pt, double* phi, double* dphi /* [nc*dim] node-major */) {
  const int d = dim_of(geom), nc = ndofs_of(geom, fe);
  if (geom == GEOM_WEDGE && fe != FE_CONSTANT) {
    for (int j = 0; j < nc; j++) {
      double v[10];
      wedge_node(fe, WDG_IND[j][0], WDG_IND[j][1], WDG_IND[j][2], pt[0], pt[1], pt[2], v);
      if (phi) phi[j] = v[0];
      if (dphi)
        for (int q = 0; q < 3; q++) dphi[j * 3 + q] = v[1 + q];
    }
    return;
  }
  if (geom == GEOM_TET && fe == FE_BIQUADRATIC) {
    double P[15], D[15][3];
    tet15(pt[0], pt[1], pt[2], P, D);
    for (int j = 0; j < 15; j++) {
      if (phi) phi[j] = P[j];
      if (dphi)
        for (int q = 0; q < 3; q++) dphi[j * 3 + q] = D[j][q];
    }
    return;
  }
  if (geom == GEOM_TET && fe != FE_CONSTANT) {
    for (int j = 0; j < nc; j++) {
      double v[10];
      tet_node(fe, TET_IND[j][0], TET_IND[j][1], TET_IND[j][2], pt[0], pt[1], pt[2], v);
      if (phi) phi[j] = v[0];
      if (dphi)
        for (int q = 0; q < 3; q++) dphi[j * 3 + q] = v[1 + q];
    }
    return;
  }
  if (geom == GEOM_TRI && fe != FE_CONSTANT) {
    for (int j = 0; j < nc; j++) {
      double v[6];
      tri_node(fe, TRI_IND[j][0], TRI_IND[j][1], pt[0], pt[1], v);
      if (phi) phi[j] = v[0];
      if (dphi) {
        dphi[j * 2 + 0] = v[1];
        dphi[j * 2 + 1] = v[2];
      }
    }
    return;
  }
  if (fe == FE_CONSTANT) {        // quad0 / hex0: the constant one
    if (phi) phi[0] = 1.;
    if (dphi)
      for (int k = 0; k < d; k++) dphi[k] = 0.;
    return;
  }
  if (fe == FE_SERENDIPITY && d > 1) {
    for (int j = 0; j < nc; j++) {
      double v[10];
      serendipity_node(geom, j, pt, v);
      if (phi) phi[j] = v[0];
      if (dphi)
        for (int k = 0; k < d; k++) dphi[j * d + k] = v[1 + k];
    }
    return;
  }
  for (int j = 0; j < nc; j++) {
    double l[3], dl[3];
    for (int k = 0; k < d; k++) {
      const int I = xc(geom, j, k) + 1;
      l[k] = (fe == FE_LINEAR) ? lagL(pt[k], I) : lagB(pt[k], I);
      dl[k] = (fe == FE_LINEAR) ? dlagL(pt[k], I) : dlagB(pt[k], I);
    }
    if (d == 1) {
      if (phi) phi[j] = l[0];
      if (dphi) dphi[j] = dl[0];
    } else if (d == 2) {
      if (phi) phi[j] = l[0] * l[1];
      if (dphi) {
        dphi[j * 2 + 0] = dl[0] * l[1];
        dphi[j * 2 + 1] = l[0] * dl[1];
      }
    } else {
      if (phi) phi[j] = l[0] * l[1] * l[2];
      if (dphi) {
        dphi[j * 3 + 0] = dl[0] * l[1] * l[2];
        dphi[j * 3 + 1] = l[0] * dl[1] * l[2];
        dphi[j * 3 + 2] = l[0] * l[1] * dl[2];
      }
    }
  }
}
}  // namespace hd
}  // namespace fhfe
