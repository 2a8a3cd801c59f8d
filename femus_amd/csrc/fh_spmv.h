// The sparse matrix-vector product family (fh_spmv.hip): what the matrix (fh_mat.hip), the builders of matrices and the multigrid (fh_mg.hip) see of it.
// The products themselves, fh_dev_spmv and fh_dev_spmv_part, are declared in fh_internal.h with the other helpers that cross translation units.
#pragma once
#include "fh_internal.h"

// all layout data of the product kernels for one matrix (fh_mat_s::spmv); null until fh_spmv_build_rowblocks.  Three layers, each derived from the
// one before, and what invalidates them:
//   row blocks (tile, kernel they were cut for, count, boundaries)         <- the pattern, options spmv_tile / spmv_kernel
//   local columns, first non-zero per block (d_tile_s), block descriptors  <- the row blocks
//   interior / interface split of the descriptors                          <- the descriptors, n_own
// A product checks the layers it needs against the options in force and rebuilds the stale ones (one rule, plan_current in fh_spmv.hip); rebuilding a
// layer marks the ones below it stale.  Matrix VALUES are not part of the plan: the kernels stream A->d_val.
struct SpmvPlan;
// cuts the rows of A into blocks for the context's spmv_tile and spmv_kernel (creates the plan at the first call).  Every builder of a matrix calls
// it once the pattern is complete -- eagerly: it allocates and copies synchronously, which must not fall into a graph capture
int fh_spmv_build_rowblocks(fh_mat_t A);
// appends what a product with A carries beyond A's own arrays (the signature of the captured cycle); a matrix without a plan: fixed words
void fh_spmv_signature(fh_mat_t A, std::vector<uint64_t>& words);
void fh_spmv_free(SpmvPlan* plan);
