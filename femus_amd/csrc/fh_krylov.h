// The Krylov solvers (fh_krylov.hip): the outer solvers of fh_mg_solve and GMRES as a level solver, and what the multigrid (fh_mg.hip) sees of them.
#pragma once
#include "fh_internal.h"
#include <functional>

// what a solver sees of the operator and its preconditioner: the multigrid fills this in, for the finest level (outer solvers) or for one level
// of the cycle (level solver)
struct KrylovOps {
  fh_ctx_t ctx = nullptr;
  int n = 0, ncols = 0;                 // owned rows; owned + ghost entries of a vector on a distributed level
  // y = A x (mode 0) or y = b - A x (mode 2), the ghosts of x refreshed first (MatMult of a distributed matrix)
  std::function<int(double* x, double* y, int mode, const double* b)> spmv;
  // sum over the ranks of count doubles in device memory, on the stream; of count doubles on the host (VecDot); both do nothing without a halo
  std::function<int(double* d, int count)> allreduce;
  std::function<int(double* vals, int count)> allreduce_host;
  // out = M^-1 in.  A null out leaves the result where precond_result() says AFTER the call (an un-captured cycle alternates between its two
  // buffers); an `in` equal to precond_input is read in place -- the outer GMRES writes A v there and saves two vector copies per iteration
  std::function<int(const double* in, double* out)> precond;
  std::function<double*()> precond_result;
  double* precond_input = nullptr;
};

// workspace of the outer solvers, kept between solves (grow only)
struct KrylovWork {
  std::vector<double*> kv;    // work vectors of kv_n + 2 doubles
  int kv_n = 0;
  double** d_V = nullptr;     // device copy of the first d_V_n pointers of kv (the GMRES bases)
  int d_V_n = 0;
  double* d_gm = nullptr;     // state block of the device-resident GMRES; h_gm = pinned mirror of its header
  double* h_gm = nullptr;
  size_t gm_cap = 0;
  // nvec vectors for n entries (zeroed, or NaN patterns under debug_poison), the first ntable of their pointers on the device, and -- with
  // need_device_state -- the state block of GMRES(restart)
  int reserve(fh_ctx_t c, int nvec, int n, int ntable = 0, int restart = 0, bool need_device_state = false);
  void release();
};

// workspace of GMRES as the solver of one level: m = iterations of one restart cycle
struct LevelGmres {
  int m = 0, nb = 0;          // nb: workgroups of the dot-product launches
  double* basis = nullptr;    // m + 1 basis vectors of ncols + 2 entries
  double** d_V = nullptr;     // their device pointer table
  double* small = nullptr;    // the small arrays below, one allocation
  int reserve(int m_new, int ncols, int n, fh_ctx_t c);    // (re)allocates when m changes, zeroes the basis on the stream at every call
  void release();
  double* vec(int j, int ncols) const { return basis + (size_t)j * ((size_t)ncols + 2); }
  // layout of `small`
  double* part() const { return small; }                                      // (m + 2) * nb partial sums, m + 2 reduced ones behind them
  double* H() const { return part() + (size_t)(m + 2) * nb + m + 2; }         // Hessenberg matrix: m columns of length m + 1
  double* g() const { return H() + (size_t)m * (m + 1); }                     // reduced right-hand side, m + 1
  double* y() const { return g() + (m + 1); }                                 // solution of the least-squares problem, m
  double* beta() const { return y() + m; }                                    // norm of the first basis vector
  size_t small_doubles() const { return (size_t)(beta() - part()) + 2; }
};

// the outer solvers of fh_mg_solve: x = the solution, *its / *rn = iterations and last residual norm; all leave work on the stream
int fh_krylov_preonly(const KrylovOps& op, double* b, double* x, int* its);
int fh_krylov_richardson(const KrylovOps& op, KrylovWork& W, double* b, double* x, double rtol, double atol, double dtol, int maxit, int* its, double* rn);
int fh_krylov_cg(const KrylovOps& op, KrylovWork& W, double* b, double* x, double rtol, double atol, double dtol, int maxit, int* its, double* rn);
// GMRES(restart) driven from the host: left-preconditioned, or flexible (right-preconditioned, the vectors M^-1 v_k kept)
int fh_krylov_gmres_host(const KrylovOps& op, KrylovWork& W, bool flexible, double* b, double* x, double rtol, double atol, double dtol, int maxit,
                         int restart, int* its, double* rn);
// left-preconditioned GMRES(restart) with its recurrences on the device (option gmres_device, the default)
int fh_krylov_gmres_device(const KrylovOps& op, KrylovWork& W, double* b, double* x, double rtol, double atol, double dtol, int maxit, int restart,
                           int* its, double* rn);
// nits iterations of left-preconditioned GMRES on A x = b as the solver of a level, everything on the stream (part of the captured cycle);
// r: scratch of n entries, zero_guess: x is taken as zero
int fh_gmres_smooth(LevelGmres& W, const KrylovOps& op, double* x, const double* b, double* r, int nits, bool zero_guess);

// y = a x + b y, x may alias y (defined in fh_krylov.hip; the sweep smoothers of fh_mg.hip launch it too)
__global__ __launch_bounds__(256) void k_axpby2(double* y, const double* x, double a, double b, int n);
