// Stand-alone driver of the shared GMRES recurrence (femus_amd/csrc/fh_hessenberg.h) for tests/test_krylov_host.py: no device, no library.
// stdin:  m maxit beta rtol atol dtol, then the (m + 1) x m upper-Hessenberg matrix row by row.
// stdout: "rn <k> <estimate>" after every column, "done <k>" at the step that reports done (or "done -1"), "kused <n>", "y <values>".
// The columns go in one at a time, as the host-driven loop of fh_krylov.hip feeds them.
#include "fh_hessenberg.h"
#include <cstdio>
#include <vector>

int main() {
  int m = 0, maxit = 0;
  double beta = 0.0, rtol = 0.0, atol = 0.0, dtol = 0.0;
  if (scanf("%d %d %lf %lf %lf %lf", &m, &maxit, &beta, &rtol, &atol, &dtol) != 6 || m < 1) return 2;
  std::vector<double> A((size_t)(m + 1) * m);
  for (double& a : A)
    if (scanf("%lf", &a) != 1) return 2;
  std::vector<double> H((size_t)(m + 1) * m, 0.0), g(m + 1, 0.0), cs(m), sn(m), y(m);
  const double tol[4] = {beta, rtol, atol, dtol};
  g[0] = beta;
  int its = 0, kused = 0, done_at = -1;
  double rn = beta;
  for (int k = 0; k < m && done_at < 0; k++) {
    for (int j = 0; j <= k + 1; j++) H[(size_t)j * m + k] = A[(size_t)j * m + k];
    const double wn = A[(size_t)(k + 1) * m + k];
    if (fh_gmres_hessenberg_step(H.data(), m, k, wn, g.data(), cs.data(), sn.data(), tol, &its, &maxit, &rn)) done_at = k;
    kused = k + 1;
    printf("rn %d %.17g\n", k, rn);
  }
  fh_gmres_back_substitute(H.data(), m, kused, g.data(), y.data());
  printf("done %d\nkused %d\ny", done_at, kused);
  for (int i = 0; i < kused; i++) printf(" %.17g", y[i]);
  printf("\n");
  return 0;
}
