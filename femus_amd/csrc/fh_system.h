// What the two system bodies on the resident plan of the generic assembly share: the stationary one (fh_system.hip) and its theta-step
// (fh_system_transient.hip).  Both leave block b = k m + l of an element entry at Kb[b nent + its scalar place] and the residual of variable k at
// Fb[k nrows + its scalar row], in the same work buffers, and both hand them to the same row pass.
#pragma once
#include "fh_generic.h"

// Row pass into block_system(S, m) (fh_system.hip): lpr lanes (a power of two <= 64) per system row (k, i), m maxrow doubles of dynamic LDS per group
__global__ __launch_bounds__(GP_THREADS) void k_sys_rows(int ndof, int m, int lpr, int maxrow, GenRowShapes sh, const int* __restrict__ adj_ptr, const int* __restrict__ adj,
                           const double* __restrict__ Kb, long long kstride, const int* __restrict__ Pos, const double* __restrict__ Fb, long long fstride,
                           const int* __restrict__ rowptr, long long nnz, double* __restrict__ val, double* __restrict__ res);

// The lanes and LDS of the row pass (sys_lpr, sys_row_lds) and the work buffers d_sysK / d_sysF of m variables (m = 1: the scalar ones), made by whichever of
// the two bodies is called first with that m and found by the other: a system and its theta-step hold them once.  Refusals: a row that is longer than the row
// pass holds, then device memory; 0xFF bytes under debug_poison
int sy_work_buffers(const char* who, fh_generic_assembler_t as, int m);
