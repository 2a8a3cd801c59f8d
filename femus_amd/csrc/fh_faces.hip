// What the applications integrate outside the element loop of an assembler, each a one-shot call with its own uploads:
//   fh_fe_jacobian       elem_type::Jacobian for every (element, Gauss point) of a mesh, Hessians optional (k_fe_jacobian)
//   fh_fe_face_normals   the unit normals elem_type::JacobianSur returns, on the host
//   fh_assemble_neumann_faces / _expr, fh_assemble_pressure_faces   boundary-face integrals into a residual vector (k_neumann), the flux a number per
//                        face or a parsed expression evaluated at the face Gauss points
#include "fh_internal.h"
#include "fh_fe.h"
#include "fh_expr_device.h"
#include <algorithm>

// ------------------------------------------------------------------------------------------------------------------
// a4 in full: elem_type::Jacobian (ElemType.hpp:1183-1248 2-D, :1438-1537 3-D) for every (element, Gauss point) of a mesh, with the optional
// Hessians `nablaphi` (:1509-1534, :1232-1244): one thread per (element, Gauss point), the reference's accumulation order and bracketing.
// The Hessian formula is the reference's: JacI^T (reference Hessian) JacI, i.e. without the second derivatives of the map (exact on affine elements).
// ------------------------------------------------------------------------------------------------------------------
template <int DIM>
__global__ __launch_bounds__(128) void k_fe_jacobian(int nel, int ng, int nc, int nloc, const int* __restrict__ ed, const double* __restrict__ coords,
                                                     const double* __restrict__ w, const double* __restrict__ dphi, const double* __restrict__ d2phi,
                                                     double* __restrict__ weight, double* __restrict__ gradphi, double* __restrict__ nablaphi) {
  constexpr int NH = DIM == 2 ? 3 : 6;
  const size_t t = (size_t)blockIdx.x * 128 + threadIdx.x;
  if (t >= (size_t)nel * ng) return;
  const int e = (int)(t / ng), g = (int)(t % ng);
  const int* en = ed + (size_t)e * nloc;
  const double* dp = dphi + (size_t)g * nc * DIM;
  double J[DIM][DIM], I[DIM][DIM];
  for (int a = 0; a < DIM; a++)
    for (int b = 0; b < DIM; b++) J[a][b] = 0.0;
  for (int n = 0; n < nc; n++) {
    const double* x = coords + (size_t)en[n] * DIM;
    for (int a = 0; a < DIM; a++)
      for (int b = 0; b < DIM; b++) J[a][b] += dp[n * DIM + a] * x[b];
  }
  double det;
  if (DIM == 2) {
    det = J[0][0] * J[1][1] - J[0][1] * J[1][0];
    I[0][0] = J[1][1] / det;
    I[0][1] = -J[0][1] / det;
    I[1][0] = -J[1][0] / det;
    I[1][1] = J[0][0] / det;
  } else {
    det = J[0][0] * (J[1][1] * J[2][2] - J[1][2] * J[2][1]) + J[0][1] * (J[1][2] * J[2][0] - J[1][0] * J[2][2]) + J[0][2] * (J[1][0] * J[2][1] - J[1][1] * J[2][0]);
    I[0][0] = (-J[1][2] * J[2][1] + J[1][1] * J[2][2]) / det;
    I[0][1] = (J[0][2] * J[2][1] - J[0][1] * J[2][2]) / det;
    I[0][2] = (-J[0][2] * J[1][1] + J[0][1] * J[1][2]) / det;
    I[1][0] = (J[1][2] * J[2][0] - J[1][0] * J[2][2]) / det;
    I[1][1] = (-J[0][2] * J[2][0] + J[0][0] * J[2][2]) / det;
    I[1][2] = (J[0][2] * J[1][0] - J[0][0] * J[1][2]) / det;
    I[2][0] = (-J[1][1] * J[2][0] + J[1][0] * J[2][1]) / det;
    I[2][1] = (J[0][1] * J[2][0] - J[0][0] * J[2][1]) / det;
    I[2][2] = (-J[0][1] * J[1][0] + J[0][0] * J[1][1]) / det;
  }
  if (weight) weight[t] = det * w[g];
  for (int n = 0; n < nc; n++) {
    if (gradphi)
      for (int a = 0; a < DIM; a++) {
        double sum = dp[n * DIM + 0] * I[a][0];
        for (int b = 1; b < DIM; b++) sum += dp[n * DIM + b] * I[a][b];
        gradphi[(t * nc + n) * DIM + a] = sum;
      }
    if (nablaphi) {
      const double* h = d2phi + ((size_t)g * nc + n) * NH;
      double H[DIM][DIM];      // reference Hessian, symmetric
      if (DIM == 2) {
        H[0][0] = h[0]; H[1][1] = h[1]; H[0][1] = H[1][0] = h[2];
      } else {
        H[0][0] = h[0]; H[1][1] = h[1]; H[2][2] = h[2];
        H[0][1] = H[1][0] = h[3]; H[1][2] = H[2][1] = h[4]; H[0][2] = H[2][0] = h[5];
      }
      auto entry = [&](int a, int b) {
        double out = 0.0;
        for (int r = 0; r < DIM; r++) {
          double row = H[r][0] * I[a][0];
          for (int c2 = 1; c2 < DIM; c2++) row += H[r][c2] * I[a][c2];
          out += row * I[b][r];
        }
        return out;
      };
      double* o = nablaphi + (t * nc + n) * NH;
      if (DIM == 2) {
        o[0] = entry(0, 0); o[1] = entry(1, 1); o[2] = entry(0, 1);
      } else {
        o[0] = entry(0, 0); o[1] = entry(1, 1); o[2] = entry(2, 2);
        o[3] = entry(0, 1); o[4] = entry(1, 2); o[5] = entry(2, 0);
      }
    }
  }
}

extern "C" int fh_fe_tables_d2(int geom, int fe, int order, double* d2phi);

extern "C" int fh_fe_jacobian(fh_ctx_t ctx, int geom, int fe, int order, int nel, int nloc, const int* elem_dof, int nnode, const double* coords,
                              double* weight, double* gradphi, double* nablaphi) {
  FH_GUARD_BEGIN
  FH_REQUIRE(ctx && (nel == 0 || (elem_dof && coords)), "fh_fe_jacobian: null argument");
  FH_REQUIRE(geom == 0 || geom == 1, "fh_fe_jacobian: geom must be 0 (hex) or 1 (quad)");
  FH_REQUIRE(fe == 0 || fe == 1 || fe == 2, "fh_fe_jacobian: fe must be 0 (linear), 1 (serendipity) or 2 (biquadratic)");
  FH_REQUIRE(nloc == fhfe::nloc_of(geom), "fh_fe_jacobian: nloc %d does not match the geometry (%d)", nloc, fhfe::nloc_of(geom));
  if (nel == 0) return 0;
  const int dim = fhfe::dim_of(geom), nc = fhfe::ndofs_of(geom, fe), nh = dim == 2 ? 3 : 6;
  std::vector<double> w, phi, dphi;
  FH_REQUIRE(fhfe::shape_tables(geom, fe, order, w, phi, dphi) == 0, "fh_fe_jacobian: unsupported Gauss rule %d", order);
  const int ng = (int)w.size();
  for (size_t k = 0; k < (size_t)nel * nloc; k++) FH_REQUIRE(elem_dof[k] >= 0 && elem_dof[k] < nnode, "fh_fe_jacobian: node id %d out of range", elem_dof[k]);
  std::vector<double> d2((size_t)ng * nc * nh, 0.0);
  if (nablaphi) {
    std::vector<double> tab((size_t)nh * ng * nc);
    FH_TRY(fh_fe_tables_d2(geom, fe, order, tab.data()));
    for (int k = 0; k < nh; k++)
      for (int g = 0; g < ng; g++)
        for (int n = 0; n < nc; n++) d2[((size_t)g * nc + n) * nh + k] = tab[((size_t)k * ng + g) * nc + n];
  }
  struct Bufs {
    std::vector<void*> p;
    ~Bufs() { for (void* q : p) if (q) hipFree(q); }
  } B;
  auto dev = [&](void** d, const void* h, size_t bytes) -> int {
    FH_CHECK_HIP(hipMalloc(d, bytes ? bytes : 8));
    B.p.push_back(*d);
    if (h && bytes) FH_CHECK_HIP(hipMemcpyAsync(*d, h, bytes, hipMemcpyHostToDevice, ctx->stream));
    return 0;
  };
  const size_t npt = (size_t)nel * ng;
  int* d_ed;
  double *d_xy, *d_w, *d_dphi, *d_d2, *d_wt = nullptr, *d_g = nullptr, *d_n = nullptr;
  FH_TRY(dev((void**)&d_ed, elem_dof, (size_t)nel * nloc * sizeof(int)));
  FH_TRY(dev((void**)&d_xy, coords, (size_t)nnode * dim * sizeof(double)));
  FH_TRY(dev((void**)&d_w, w.data(), w.size() * sizeof(double)));
  FH_TRY(dev((void**)&d_dphi, dphi.data(), dphi.size() * sizeof(double)));
  FH_TRY(dev((void**)&d_d2, d2.data(), d2.size() * sizeof(double)));
  if (weight) FH_TRY(dev((void**)&d_wt, nullptr, npt * sizeof(double)));
  if (gradphi) FH_TRY(dev((void**)&d_g, nullptr, npt * nc * dim * sizeof(double)));
  if (nablaphi) FH_TRY(dev((void**)&d_n, nullptr, npt * nc * nh * sizeof(double)));
  const dim3 grid((unsigned)((npt + 127) / 128)), block(128);
  if (dim == 3) hipLaunchKernelGGL(k_fe_jacobian<3>, grid, block, 0, ctx->stream, nel, ng, nc, nloc, d_ed, d_xy, d_w, d_dphi, d_d2, d_wt, d_g, d_n);
  else hipLaunchKernelGGL(k_fe_jacobian<2>, grid, block, 0, ctx->stream, nel, ng, nc, nloc, d_ed, d_xy, d_w, d_dphi, d_d2, d_wt, d_g, d_n);
  FH_CHECK_HIP(hipGetLastError());
  if (weight) FH_CHECK_HIP(hipMemcpyAsync(weight, d_wt, npt * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  if (gradphi) FH_CHECK_HIP(hipMemcpyAsync(gradphi, d_g, npt * nc * dim * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  if (nablaphi) FH_CHECK_HIP(hipMemcpyAsync(nablaphi, d_n, npt * nc * nh * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  FH_CHECK_HIP(hipStreamSynchronize(ctx->stream));
  return 0;
  FH_GUARD_END("fh_fe_jacobian")
}

// ------------------------------------------------------------------------------------------------------------------
// Neumann boundary faces (a5: elem_type::JacobianSur).  One thread per boundary node: it owns the node's (face, local i)
// pairs (ascending face order) and integrates phi_i * tau over each face with the face element's quadrature.
// ------------------------------------------------------------------------------------------------------------------
// NORMAL: the vector form  res[off[k] + node] += scale * int_face phi_i tau n_k ds  for the DIM components (open-boundary pressure term of the
// Navier-Stokes residual, 03_navier_stokes.hpp:185-290, normal = the one JacobianSur returns at each face Gauss point)
template <int DIM, bool NORMAL>
__global__ __launch_bounds__(128) void k_neumann(const int* __restrict__ node_ptr, const int* __restrict__ node_id, const int* __restrict__ pairs,
                                                 int nbn, const int* __restrict__ face_nodes, int nfn, const double* __restrict__ tau,
                                                 const double* __restrict__ coords, const double* __restrict__ w, const double* __restrict__ phi,
                                                 const double* __restrict__ dphi, int ng, double* __restrict__ res,
                                                 const int* __restrict__ face_expr, const int* __restrict__ prog, const int* __restrict__ prog_ptr,
                                                 const double* __restrict__ pconst, const int* __restrict__ const_ptr, int off0, int off1, int off2, double scale) {
  const int t = blockIdx.x * 128 + threadIdx.x;
  if (t >= nbn) return;
  double total = 0.0, totn[3] = {0.0, 0.0, 0.0};
  for (int p = node_ptr[t]; p < node_ptr[t + 1]; p++) {
    const int f = pairs[p] >> 4, i = pairs[p] & 15;
    const int* fn = face_nodes + (size_t)f * nfn;
    double acc = 0.0, accn[3] = {0.0, 0.0, 0.0};
    for (int g = 0; g < ng; g++) {
      double weight, nrm[3] = {0.0, 0.0, 0.0};
      if (DIM == 3) {   // quad face in 3-D: tangents, normal = t1 x t2, det = |normal|  (ElemType.hpp:1330-1380)
        double J[3][2] = {{0, 0}, {0, 0}, {0, 0}};
        for (int n = 0; n < nfn; n++) {
          const double dx = dphi[((size_t)g * nfn + n) * 2 + 0], dy = dphi[((size_t)g * nfn + n) * 2 + 1];
          const double* x = coords + (size_t)fn[n] * 3;
          for (int d = 0; d < 3; d++) {
            J[d][0] += dx * x[d];
            J[d][1] += dy * x[d];
          }
        }
        const double nx = J[1][0] * J[2][1] - J[1][1] * J[2][0];
        const double ny = J[0][1] * J[2][0] - J[2][1] * J[0][0];
        const double nz = J[0][0] * J[1][1] - J[0][1] * J[1][0];
        const double inv = 1.0 / sqrt(nx * nx + ny * ny + nz * nz);
        const double n0 = nx * inv, n1 = ny * inv, n2 = nz * inv;
        const double det = J[0][0] * (J[1][1] * n2 - n1 * J[2][1]) + J[0][1] * (n1 * J[2][0] - J[1][0] * n2) + n0 * (J[1][0] * J[2][1] - J[1][1] * J[2][0]);
        weight = det * w[g];
        nrm[0] = n0; nrm[1] = n1; nrm[2] = n2;
      } else {          // edge in 2-D (ElemType.hpp:1089-1138)
        double j0 = 0.0, j1 = 0.0;
        for (int n = 0; n < nfn; n++) {
          const double dx = dphi[(size_t)g * nfn + n];
          const double* x = coords + (size_t)fn[n] * 2;
          j0 += dx * x[0];
          j1 += dx * x[1];
        }
        const double modn = sqrt(j0 * j0 + j1 * j1);
        const double n0 = j1 / modn, n1 = -j0 / modn;
        const double det = j0 * (-n1) - (-n0) * j1;
        weight = det * w[g];
        nrm[0] = n0; nrm[1] = n1;
      }
      double tv;
      if (face_expr) {       // the flux is a parsed function of the Gauss point: (*bdcfunc)(&xyzt[0]), 001_Poisson/main.cpp:524-534
        double xg[4] = {0.0, 0.0, 0.0, 0.0};
        for (int n = 0; n < nfn; n++) {
          const double ph = phi[(size_t)g * nfn + n];
          const double* x = coords + (size_t)fn[n] * DIM;
          for (int d = 0; d < DIM; d++) xg[d] += x[d] * ph;
        }
        const int ex = face_expr[f];
        tv = fh_expr_device_eval(prog + prog_ptr[ex], prog_ptr[ex + 1] - prog_ptr[ex], pconst + const_ptr[ex], xg);
      } else {
        tv = tau[f];
      }
      if (NORMAL) {
#pragma unroll
        for (int k = 0; k < DIM; k++) accn[k] += phi[(size_t)g * nfn + i] * tv * nrm[k] * weight;
      } else {
        acc += phi[(size_t)g * nfn + i] * tv * weight;
      }
    }
    total += acc;
#pragma unroll
    for (int k = 0; k < DIM; k++) totn[k] += accn[k];
  }
  if (NORMAL) {
    const int off[3] = {off0, off1, off2};
#pragma unroll
    for (int k = 0; k < DIM; k++) res[off[k] + node_id[t]] += scale * totn[k];
  } else {
    res[node_id[t]] += total;
  }
}

// tables of the face element of `geom` (quad: the 2-D tables; line: 1-D Lagrange at the 1-D Gauss points): weights, phi[g][n], dphi[g][n][dim-1]
static int face_element_tables(int geom, int fe, int order, int* nfn_out, std::vector<double>& w, std::vector<double>& phi, std::vector<double>& dphi) {
  // geom >= 100: the FACE element itself is named (100 + its geometry: 101 quadrilateral, 103 triangle, 102 line) -- prisms have faces of two kinds
  const int fgeom = geom >= 100 ? geom - 100 : (geom == fhfe::GEOM_HEX) ? fhfe::GEOM_QUAD : (geom == fhfe::GEOM_TET) ? fhfe::GEOM_TRI : fhfe::GEOM_LINE;
  int tmp[9];
  const int nfn = geom >= 100 ? fhfe::ndofs_of(fgeom, fe) : fhfe::face_nodes(geom, fe, 0, tmp);
  *nfn_out = nfn;
  if (fgeom == fhfe::GEOM_TRI) {        // the faces of a tetrahedron: TRI3 / TRI6 with the triangle's rule of the same order
    FH_REQUIRE(fhfe::shape_tables(fhfe::GEOM_TRI, fe, order, w, phi, dphi) == 0, "fh_assemble_neumann_faces: unsupported Gauss rule");
  } else if (fgeom == fhfe::GEOM_QUAD) {
    FH_REQUIRE(fhfe::shape_tables(fhfe::GEOM_QUAD, fe, order, w, phi, dphi) == 0, "fh_assemble_neumann_faces: unsupported Gauss rule");
  } else {
    const int ng1 = order + 1;
    w.resize(ng1);
    std::vector<double> x1(ng1);
    FH_REQUIRE(fhfe::gauss_table(fhfe::GEOM_LINE, order, w.data(), x1.data()) == 0, "fh_assemble_neumann_faces: unsupported Gauss rule");
    phi.resize((size_t)ng1 * nfn);
    dphi.resize((size_t)ng1 * nfn);
    for (int g = 0; g < ng1; g++) {
      const double x = x1[g];
      if (fe == 0) {   // LineLinear: nodes -1, +1 (Edge.hpp:72-78)
        phi[g * 2 + 0] = 0.5 * (1. - x);  phi[g * 2 + 1] = 0.5 * (1. + x);
        dphi[g * 2 + 0] = -0.5;           dphi[g * 2 + 1] = 0.5;
      } else {         // LineBiquadratic: nodes -1, +1, 0 (Edge.hpp:94-100)
        phi[g * 3 + 0] = 0.5 * x * (x - 1.);  phi[g * 3 + 1] = 0.5 * x * (1. + x);  phi[g * 3 + 2] = (1. - x) * (1. + x);
        dphi[g * 3 + 0] = x - 0.5;            dphi[g * 3 + 1] = x + 0.5;            dphi[g * 3 + 2] = -2. * x;
      }
    }
  }
  return 0;
}

// unit normals of boundary faces at one face Gauss point, as elem_type::JacobianSur returns them (host; the applications read them to decide what a
// face contributes, e.g. 03_navier_stokes.hpp:264-275 picks the normal velocity component from the normal at Gauss point 0)
extern "C" int fh_fe_face_normals(int geom, int fe, int order, int gauss_point, int nfaces, const int* face_nodes, int nnode, const double* coords,
                                  double* normals /* [nfaces*dim] */) {
  FH_GUARD_BEGIN
  FH_REQUIRE(geom == 0 || geom == 1, "fh_fe_face_normals: geom must be 0 (hex) or 1 (quad)");
  FH_REQUIRE(fe == 0 || fe == 1 || fe == 2, "fh_fe_face_normals: fe must be 0, 1 or 2");
  FH_REQUIRE(nfaces == 0 || (face_nodes && coords && normals), "fh_fe_face_normals: null argument");
  const int dim = fhfe::dim_of(geom);
  int nfn = 0;
  std::vector<double> w, phi, dphi;
  FH_TRY(face_element_tables(geom, fe, order, &nfn, w, phi, dphi));
  const int g = gauss_point;
  FH_REQUIRE(g >= 0 && g < (int)w.size(), "fh_fe_face_normals: Gauss point %d of %d", g, (int)w.size());
  for (int f = 0; f < nfaces; f++) {
    const int* fn = face_nodes + (size_t)f * nfn;
    for (int n = 0; n < nfn; n++) FH_REQUIRE(fn[n] >= 0 && fn[n] < nnode, "fh_fe_face_normals: node id out of range");
    if (dim == 3) {
      double J[3][2] = {{0, 0}, {0, 0}, {0, 0}};
      for (int n = 0; n < nfn; n++) {
        const double dx = dphi[((size_t)g * nfn + n) * 2 + 0], dy = dphi[((size_t)g * nfn + n) * 2 + 1];
        const double* x = coords + (size_t)fn[n] * 3;
        for (int d = 0; d < 3; d++) {
          J[d][0] += dx * x[d];
          J[d][1] += dy * x[d];
        }
      }
      const double nx = J[1][0] * J[2][1] - J[1][1] * J[2][0];
      const double ny = J[0][1] * J[2][0] - J[2][1] * J[0][0];
      const double nz = J[0][0] * J[1][1] - J[0][1] * J[1][0];
      const double inv = 1.0 / sqrt(nx * nx + ny * ny + nz * nz);
      normals[(size_t)f * 3 + 0] = nx * inv;
      normals[(size_t)f * 3 + 1] = ny * inv;
      normals[(size_t)f * 3 + 2] = nz * inv;
    } else {
      double j0 = 0.0, j1 = 0.0;
      for (int n = 0; n < nfn; n++) {
        const double dx = dphi[(size_t)g * nfn + n];
        const double* x = coords + (size_t)fn[n] * 2;
        j0 += dx * x[0];
        j1 += dx * x[1];
      }
      const double modn = sqrt(j0 * j0 + j1 * j1);
      normals[(size_t)f * 2 + 0] = j1 / modn;
      normals[(size_t)f * 2 + 1] = -j0 / modn;
    }
  }
  return 0;
  FH_GUARD_END("fh_fe_face_normals")
}

static int neumann_faces(fh_ctx_t ctx, int geom, int fe, int order, int nfaces, const int* face_nodes, const double* tau, const int* face_expr, int nexpr,
                         const fh_expr_t* exprs, int nnode, const double* coords, fh_vec_t res, const int* comp_offset = nullptr, double scale = 1.0) {
  FH_REQUIRE(ctx && res && (nfaces == 0 || (face_nodes && (tau || face_expr) && coords)), "fh_assemble_neumann_faces: null argument");
  FH_REQUIRE(geom == 0 || geom == 1 || geom == 3 || geom == 4 || geom == 101 || geom == 102 || geom == 103,
             "fh_assemble_neumann_faces: geom must be 0 (hex), 1 (quad), 3 (triangle), 4 (tetrahedron), or 100 + the face element's own geometry (101 / 102 / 103)");
  FH_REQUIRE(fe == 0 || fe == 1 || fe == 2, "fh_assemble_neumann_faces: fe must be 0, 1 or 2");
  if (nfaces == 0) return 0;
  const int dim = geom >= 100 ? fhfe::dim_of(geom - 100) + 1 : fhfe::dim_of(geom);
  int nfn = 0;
  std::vector<double> w, phi, dphi;
  FH_TRY(face_element_tables(geom, fe, order, &nfn, w, phi, dphi));
  const int ng = (int)w.size();
  // node -> (face, i) pairs, ascending face order
  std::vector<int> cnt(nnode + 1, 0);
  for (size_t k = 0; k < (size_t)nfaces * nfn; k++) {
    FH_REQUIRE(face_nodes[k] >= 0 && face_nodes[k] < nnode, "fh_assemble_neumann_faces: node id out of range");
    cnt[face_nodes[k] + 1]++;
  }
  std::vector<int> node_id, node_ptr(1, 0), pairs;
  for (int n = 0; n < nnode; n++) cnt[n + 1] += cnt[n];
  std::vector<int> cur(cnt.begin(), cnt.end() - 1), flat(cnt[nnode]);
  FH_REQUIRE(nfaces < (1 << 27), "fh_assemble_neumann_faces: too many faces");
  for (int f = 0; f < nfaces; f++)
    for (int i = 0; i < nfn; i++) flat[cur[face_nodes[(size_t)f * nfn + i]]++] = (f << 4) | i;
  for (int n = 0; n < nnode; n++)
    if (cnt[n + 1] > cnt[n]) {
      node_id.push_back(n);
      pairs.insert(pairs.end(), flat.begin() + cnt[n], flat.begin() + cnt[n + 1]);
      node_ptr.push_back((int)pairs.size());
    }
  const int nbn = (int)node_id.size();
  FH_REQUIRE(res->n_local + res->nghost > node_id.back() + (comp_offset ? *std::max_element(comp_offset, comp_offset + dim) : 0),
             "fh_assemble_neumann_faces: vector too short");
  // parsed fluxes: the programs of all expressions back to back
  std::vector<int> h_prog, h_prog_ptr(1, 0), h_const_ptr(1, 0);
  std::vector<double> h_const;
  if (face_expr) {
    FH_REQUIRE(nexpr >= 1 && exprs, "fh_assemble_neumann_faces_expr: no expressions");
    for (int f = 0; f < nfaces; f++) FH_REQUIRE(face_expr[f] >= 0 && face_expr[f] < nexpr, "fh_assemble_neumann_faces_expr: face %d names expression %d of %d", f, face_expr[f], nexpr);
    for (int k = 0; k < nexpr; k++) {
      FH_REQUIRE(exprs[k], "fh_assemble_neumann_faces_expr: null expression");
      char who[64];
      snprintf(who, sizeof who, "fh_assemble_neumann_faces_expr: expression %d", k);
      std::vector<int> code;
      std::vector<double> consts;
      FH_TRY(fh_expr_fetch(exprs[k], who, 4, code, consts));
      h_prog.insert(h_prog.end(), code.begin(), code.end());
      h_const.insert(h_const.end(), consts.begin(), consts.end());
      h_prog_ptr.push_back((int)h_prog.size());
      h_const_ptr.push_back((int)h_const.size());
    }
  }
  void* dv[13] = {nullptr};
  auto up = [&](int slot, const void* h, size_t bytes) -> int {
    FH_CHECK_HIP(hipMalloc(&dv[slot], bytes ? bytes : 8));
    FH_CHECK_HIP(hipMemcpyAsync(dv[slot], h, bytes, hipMemcpyHostToDevice, ctx->stream));
    return 0;
  };
  FH_TRY(up(0, node_ptr.data(), node_ptr.size() * sizeof(int)));
  FH_TRY(up(1, node_id.data(), node_id.size() * sizeof(int)));
  FH_TRY(up(2, pairs.data(), pairs.size() * sizeof(int)));
  FH_TRY(up(3, face_nodes, (size_t)nfaces * nfn * sizeof(int)));
  if (tau) FH_TRY(up(4, tau, (size_t)nfaces * sizeof(double)));
  if (face_expr) {
    FH_TRY(up(8, face_expr, (size_t)nfaces * sizeof(int)));
    FH_TRY(up(9, h_prog.data(), h_prog.size() * sizeof(int)));
    FH_TRY(up(10, h_prog_ptr.data(), h_prog_ptr.size() * sizeof(int)));
    FH_TRY(up(11, h_const.data(), h_const.size() * sizeof(double)));
    FH_TRY(up(12, h_const_ptr.data(), h_const_ptr.size() * sizeof(int)));
  }
  FH_TRY(up(5, coords, (size_t)nnode * dim * sizeof(double)));
  FH_TRY(up(6, w.data(), w.size() * sizeof(double)));
  std::vector<double> tab(phi);
  tab.insert(tab.end(), dphi.begin(), dphi.end());
  FH_TRY(up(7, tab.data(), tab.size() * sizeof(double)));
  const double* d_phi = (const double*)dv[7];
  const double* d_dphi = d_phi + phi.size();
  const dim3 grid(fh_div_up(nbn, 128)), block(128);
  const int o0 = comp_offset ? comp_offset[0] : 0, o1 = comp_offset ? comp_offset[1] : 0, o2 = (comp_offset && dim == 3) ? comp_offset[2] : 0;
#define FH_NEUMANN_LAUNCH(D, N)                                                                                                                   \
  hipLaunchKernelGGL((k_neumann<D, N>), grid, block, 0, ctx->stream, (const int*)dv[0], (const int*)dv[1], (const int*)dv[2], nbn, (const int*)dv[3], \
                     nfn, (const double*)dv[4], (const double*)dv[5], (const double*)dv[6], d_phi, d_dphi, ng, res->d, (const int*)dv[8],          \
                     (const int*)dv[9], (const int*)dv[10], (const double*)dv[11], (const int*)dv[12], o0, o1, o2, scale)
  if (dim == 3 && comp_offset) FH_NEUMANN_LAUNCH(3, true);
  else if (dim == 3) FH_NEUMANN_LAUNCH(3, false);
  else if (comp_offset) FH_NEUMANN_LAUNCH(2, true);
  else FH_NEUMANN_LAUNCH(2, false);
#undef FH_NEUMANN_LAUNCH
  FH_CHECK_HIP(hipGetLastError());
  FH_CHECK_HIP(hipStreamSynchronize(ctx->stream));
  for (void* q : dv)
    if (q) hipFree(q);
  return 0;
}

extern "C" int fh_assemble_neumann_faces(fh_ctx_t ctx, int geom, int fe, int order, int nfaces, const int* face_nodes, const double* tau, int nnode,
                                         const double* coords, fh_vec_t res) {
  FH_REQUIRE(nfaces == 0 || tau, "fh_assemble_neumann_faces: null argument");
  return neumann_faces(ctx, geom, fe, order, nfaces, face_nodes, tau, nullptr, 0, nullptr, nnode, coords, res);
}

// Open-boundary pressure term of the steady Navier-Stokes residual (03_navier_stokes.hpp:185-290): on the listed boundary faces (those whose
// normal velocity component is not Dirichlet -- the application's bdc callback decides, :236-262) aResV[k][node_i] += phi_i tau n_k weight with the
// prescribed pressure tau (a number per face, or expression face_expr[f] at the face Gauss point) and the JacobianSur normal; the residual
// vector takes scale * that (scale = -1: RES = -aRes, :425).  comp_offset[k]: where component k of the velocity starts in res.
extern "C" int fh_assemble_pressure_faces(fh_ctx_t ctx, int geom, int order, int nfaces, const int* face_nodes, const double* tau, const int* face_expr,
                                          int nexpr, const fh_expr_t* exprs, int nnode, const double* coords, const int* comp_offset, double scale,
                                          fh_vec_t res) {
  FH_REQUIRE(comp_offset, "fh_assemble_pressure_faces: null component offsets");
  FH_REQUIRE(nfaces == 0 || tau || face_expr, "fh_assemble_pressure_faces: neither a pressure per face nor expressions");
  return neumann_faces(ctx, geom, 2, order, nfaces, face_nodes, face_expr ? nullptr : tau, face_expr, nexpr, exprs, nnode, coords, res, comp_offset, scale);
}

// the flux as a parsed function of the Gauss point (x, y, z, t = 0), as the parsed-boundary-condition branch of the 001_Poisson callback
// evaluates it (`(*bdcfunc)(&xyzt[0])` inside the Gauss loop, applications/001_Poisson/main.cpp:495-553): face_expr[f] names one of `nexpr` expressions
extern "C" int fh_assemble_neumann_faces_expr(fh_ctx_t ctx, int geom, int fe, int order, int nfaces, const int* face_nodes, const int* face_expr, int nexpr,
                                              const fh_expr_t* exprs, int nnode, const double* coords, fh_vec_t res) {
  FH_REQUIRE(nfaces == 0 || face_expr, "fh_assemble_neumann_faces_expr: null argument");
  return neumann_faces(ctx, geom, fe, order, nfaces, face_nodes, nullptr, face_expr, nexpr, exprs, nnode, coords, res);
}
