// The block Schwarz smoothers of a multigrid level, FH_SMOOTH_VANKA and FH_SMOOTH_ASM (fh_patch.hip): what the multigrid (fh_mg.hip) sees of them.
#pragma once
#include "fh_internal.h"

// all state of the block smoother of one level: the dof patches, their colours (or dependency levels), the dense block inverses and the work
// buffers of the sweep.  Lifetime: the patch lists live from fh_patch_set to the next fh_patch_set; everything derived from the matrix pattern
// (colours, device copies, inverses) lives from fh_patch_setup to fh_patch_drop_setup, fh_patch_set or a fh_patch_setup of the other kind
struct PatchSmoother;
// the patches of the level (ptr: npatch + 1 offsets into dofs); creates *ps on first use, drops the setup, no block gets the exact sub-solve.
// The ORDER of the dofs inside a patch does not matter: every patch is kept sorted ascending (the order of PCASM's index sets, in which ILU(0) of a
// block is taken).  Refused, leaving the patches of the level as they were: a patch that is empty or has more than 512 dofs, a dof listed twice
// in one patch.  (A dof outside the matrix and a singular patch matrix are refused by fh_patch_setup, which is the first to see the matrix.)
int fh_patch_set(PatchSmoother** ps, int npatch, const int* ptr, const int* dofs);
// FH_SMOOTH_ASM: the first nfirst blocks get the exact sub-solve instead of ILU(0)
int fh_patch_set_exact(PatchSmoother* ps, int nfirst);
int fh_patch_count(const PatchSmoother* ps);          // 0 for a null object
// drops the device side (another matrix arrived: its graph may differ); the patch lists stay and the next fh_patch_setup rebuilds the rest
void fh_patch_drop_setup(PatchSmoother* ps);
// kind 0 (Vanka): greedy colours; kind 1 (PCASM): dependency levels of the blocks in their index order, ILU(0) blocks.  Colours once per
// pattern and kind; extracts and inverts the blocks for the values A holds now (every call)
int fh_patch_setup(PatchSmoother* ps, fh_ctx_t ctx, fh_mat_t A, int kind);
// nsweeps multiplicative Schwarz sweeps over the colours on A x = b, x updated in place; rwork: a vector of A->m doubles that is neither x nor
// b (the residual of the unfused sweep, option vanka_fused 0)
int fh_patch_apply(PatchSmoother* ps, fh_ctx_t ctx, fh_mat_t A, double* x, const double* b, double* rwork, double omega, int nsweeps);
// appends what a launch of fh_patch_apply carries beyond its arguments (the signature of the captured cycle); null object: fixed words
void fh_patch_signature(const PatchSmoother* ps, std::vector<uint64_t>& words);
void fh_patch_destroy(PatchSmoother* ps);
