// The small dense algebra of GMRES, once for the device (k_gm_step) and for the host-driven loops (fh_krylov.hip): one column of the Hessenberg matrix
// through the Givens rotations, and the back substitution behind it.  Plain pointers and no other header than <cmath>: a stand-alone host program
// (tests/test_krylov_host.py) includes this file as it is.  Each side keeps its own hypot and its own code generation.
#pragma once
#include <cmath>
#include <cstddef>

// inlined before anything else is optimised: the kernel comes out as if the statements stood in its body
#if defined(__HIPCC__)
#define FH_HOST_DEVICE __host__ __device__ __attribute__((always_inline))
#else
#define FH_HOST_DEVICE __attribute__((always_inline))
#endif

// Iteration k of a restart cycle.  H: (m + 1) x m, row-major with m columns; the caller has stored column k: H[0 .. k][k] = V^T w before the
// orthogonalisation, H[k + 1][k] = wn = ||w|| after it.  Applies the rotations 0 .. k-1 to the column, forms rotation k (cs, sn: m entries each), updates
// the reduced right-hand side g (m + 1) and *rn, the residual estimate; counts the iteration in *its.  tol = {reference norm, rtol, atol, dtol}.  Returns
// whether the solver is done: converged, out of iterations (*its >= *maxit), happy breakdown (wn == 0) or diverged -- or column k vanished entirely
// (H[k][k] becomes 1, so that the back substitution stays finite: g[k] stays, y[k] = g[k]).  Count: int on the host, double in the state block of the device.
template <class Count>
FH_HOST_DEVICE inline bool fh_gmres_hessenberg_step(double* H, int m, int k, double wn, double* g, double* cs, double* sn,
                                                    const double* tol, Count* its, const Count* maxit, double* rn) {
  for (int j = 0; j < k; j++) {
    const double a = H[(size_t)j * m + k], bb = H[(size_t)(j + 1) * m + k];
    H[(size_t)j * m + k] = cs[j] * a + sn[j] * bb;
    H[(size_t)(j + 1) * m + k] = -sn[j] * a + cs[j] * bb;
  }
  const double a = H[(size_t)k * m + k], bb = H[(size_t)(k + 1) * m + k];
  const double d = hypot(a, bb);
  bool done = false;
  if (d == 0.0) {          // column k of the Hessenberg matrix vanished entirely: nothing to rotate, nothing more to gain
    cs[k] = 1.0;
    sn[k] = 0.0;
    H[(size_t)k * m + k] = 1.0;
    g[k + 1] = 0.0;
    *its += (Count)1;
    *rn = 0.0;
    done = true;
  } else {
    cs[k] = a / d;
    sn[k] = bb / d;
    H[(size_t)k * m + k] = d;
    H[(size_t)(k + 1) * m + k] = 0.0;
    g[k + 1] = -sn[k] * g[k];
    g[k] = cs[k] * g[k];
    *its += (Count)1;
    const double r = fabs(g[k + 1]);
    *rn = r;
    done = r <= fmax(tol[1] * tol[0], tol[2]) || *its >= *maxit || wn == 0.0 || r > tol[3] * tol[0];      // dtol: KSP_DIVERGED_DTOL at every iteration
  }
  return done;
}

// y[0 .. kused) = H^-1 g for the upper triangle the rotations left in the first kused columns
FH_HOST_DEVICE inline void fh_gmres_back_substitute(const double* H, int m, int kused, const double* g, double* y) {
  for (int i = kused - 1; i >= 0; i--) {
    double s2 = g[i];
    for (int j = i + 1; j < kused; j++) s2 -= H[(size_t)i * m + j] * y[j];
    y[i] = s2 / H[(size_t)i * m + i];
  }
}
