// The exact solve of the coarsest multigrid level (fh_coarse.hip): what the multigrid (fh_mg.hip) and the sparse exact solve (fh_direct.hip) see of it.
#pragma once
#include "fh_internal.h"

// all state of the exact solve of level 0: the coupled unknowns, their dissection, the dense inverse or its block form, the sparse exact solve
struct CoarseSolve;
CoarseSolve* fh_coarse_create(fh_ctx_t ctx);
void fh_coarse_destroy(CoarseSolve* cs);       // every buffer, stream and event, and the sparse exact solve; the caller has synchronised the compute stream
// coordinates of the unknowns of level 0 ([n * dim]): without them the dense problem is not dissected
void fh_coarse_set_coords(CoarseSolve* cs, int dim, int n, const double* coords);
// prepares x = A0^-1 b for the values A0 holds now: sparse exact solve, block form of the dissected dense problem or one dense inverse
int fh_coarse_factor(CoarseSolve* cs, fh_mat_t A0);
// x = A0^-1 b on the context's compute stream; scratch: A0->m doubles, dinv: the inverse diagonal of A0 (unknowns coupled to nothing)
int fh_coarse_solve(CoarseSolve* cs, const double* b, double* x, double* scratch, const double* dinv);
// what the last fh_coarse_factor made of the level (fh_mg_coarse_info); any pointer may be null
void fh_coarse_info(const CoarseSolve* cs, int* n_dense, int* nd_blocks, int* nd_separator, int* nd_largest_block);
// appends every pointer and size a launch of fh_coarse_solve carries (the signature of the captured cycle)
void fh_coarse_signature(const CoarseSolve* cs, std::vector<uint64_t>& words);

// descriptor of one dense symmetric matrix of the batched 128-block inverse (k_inv_*_b; fh_inv_sym_batched)
struct InvDesc {
  double* D;             // n x n, leading dimension n; replaced by its inverse
  int n;
  double *PT, *RT, *Dv0, *Dv1;   // work: panels 2 x (n x 128), pivot-block inverses 2 x 2 x 128 x 128 (fh_inv_work_doubles(n) doubles from PT)
  int* flg;              // two ints; flg[1] != 0: a pivot block had no usable diagonal pivot
  int off;               // first unknown of the block in the dissected ordering (k_nd_w)
};
size_t fh_inv_work_doubles(int n);
// k dense symmetric matrices (descriptors on the device) inverted beside each other on the compute stream, nmax = the largest order; work per
// matrix: fh_inv_work_doubles(n), two flag ints per matrix (flag[1] != 0: no usable pivot)
int fh_inv_sym_batched(fh_ctx_t c, const InvDesc* d_desc, int k, int nmax);

// v[0 .. n) = a, grid-stride (defined in fh_coarse.hip)
__global__ __launch_bounds__(256) void k_fill_value(double* __restrict__ v, double a, int n);
