// The tensor-product Poisson assembler as its two users see it: the assembly (fh_assemble.hip), which builds and fills it, and the element-wise
// Galerkin product (fh_galerkin.hip), which consumes what an assembly leaves behind.  Nothing else belongs here: the parameter blocks, layouts and
// macros of the assembly kernels stay in fh_assemble.hip.
#pragma once
#include "fh_internal.h"

struct SfTab { double L[3][4], D[3][4]; };   // l_a(x_k), l'_a(x_k): 1-D quadratic Lagrange basis (nodes -1, 0, +1) at the four abscissae

// what the element-wise Galerkin product (fh_assembler_galerkin) keeps on the COARSE assembler of a pair of levels: children, child interpolation
// tables, Dirichlet masks
struct GalerkinState {
  int* d_child = nullptr;
  uint64_t key = 0;              // hash of (children, fine / coarse Dirichlet nodes) the tables below were made from
  bool children_in_order = false;          // child j of coarse element E is fine element 8 * (its cluster) + j
  unsigned char *d_cnt = nullptr, *d_row = nullptr, *d_fb = nullptr, *d_cb = nullptr;
  unsigned* d_fmask = nullptr;         // [nel * 8] Dirichlet bits of the children's nodes, then [nel] of the coarse element's (k_galerkin_macro)
  double *d_val = nullptr, *d_res = nullptr, *d_dense = nullptr;
  void release();                // frees all of it (fh_galerkin.hip)
};

struct fh_assembler_s {
  fh_ctx_t ctx = nullptr;
  int geom = 0, fe = 0, order = 0, dim = 3, nc = 27, ng = 64, nloc = 27;
  int nel = 0, nnode = 0, ndof = 0;
  int ncolors = 0;
  std::vector<int> color_ptr;    // host
  int* d_color_elems = nullptr;  // elements grouped by colour
  int* d_elem_dof = nullptr;     // [nel*nloc]
  double* d_coords = nullptr;    // [nnode*dim]
  double* d_w = nullptr;         // [ng]
  double* d_phi = nullptr;       // [ng*nc]
  double* d_dphi = nullptr;      // [ng*nc*dim]
  int* d_emap = nullptr;         // [nel*nc*ncp] CSR slot of (i,j), ncp = nc rounded up to 4
  int* d_iota = nullptr;         // identity element list (for the uncoloured element-matrix entry point)
  int ncp = 28;
  // two-pass ("row gather") assembly: element matrices -> Kbuf, then every CSR row sums its <= 8 element rows in element order
  int* d_adj_ptr = nullptr;      // [m+1]
  int* d_adj_ei = nullptr;       // (element << 5) | local row, ascending element order
  unsigned char* d_rowmap = nullptr;   // [nadj*nc] slot of (element row, j) inside the CSR row
  int* d_slot = nullptr;         // [nel*nc] adjacency slot of (element, local row), -1 when the row is not in the matrix
  double* d_Kbuf = nullptr;      // [nadj*kstride] element rows in row-gather order
  size_t kbuf_bytes = 0;
  int nadj = 0;                  // element rows in d_Kbuf; row nadj is the spare one
  GalerkinState gal;             // element-wise Galerkin product from the next finer level
  int kstride = 27;              // doubles per element row in d_Kbuf (nc, or 32 for HEX27/Q2: whole 64-byte lines per row)
  double* d_Fbuf = nullptr;      // [nadj]
  bool two_pass = false;
  // fused cluster assembly (k_cluster_q2hex_sf + k_rows_partial): groups of 8 consecutive elements with one common local topology
  // (the children of one coarse element: 125 macro nodes).  Plan = tables of the template + per-cluster destinations and maps.
  bool fused = false;            // plan built and verified
  bool kbuf_valid = false;       // the element-row buffer holds the matrices of the last assembly (the fused path does not write it)
  bool rows_used_since = false;  // the element-wise Galerkin product asked for the element rows since the last assembly: the next assembly keeps them (two-pass)
  int last_path = 0;             // 1: the last assembly ran the fused path, 2: two-pass
  int cl_ncl = 0, cl_nm = 0, cl_ns = 0, cl_nprow = 0;
  int cl_sup_shift = 0;          // log2 of the clusters per super-cluster whose inner rows are carried in the CSR array (0: none)
  int cl_walk_shift = 0;         // log2 of the consecutive clusters a workgroup of the cluster kernel serves one after the other (= cl_sup_shift; measurements: assemble_carry 100 + k walks 2^k clusters with nothing carried)
  size_t cl_ncarried = 0;        // CSR entries of carried rows
  size_t cl_npart = 0;           // entries of the partial-row buffer (without the sink)
  unsigned* d_cl_sinfo = nullptr;
  void *d_cl_dtab = nullptr, *d_cl_fblk = nullptr, *d_cl_oblk = nullptr;      // descriptor tables of the template (see ClParams)
  int *d_cl_vdst = nullptr, *d_cl_fdst = nullptr;      // [ncl][128]: >= 0 CSR offset / row of a complete row, bit 31: offset into the partial-row buffer
  unsigned long long* d_cl_vdst64 = nullptr;           // ... as addresses, for the value array cl_val_base
  double* cl_val_base = nullptr;
  unsigned char *d_cl_map = nullptr, *d_cl_pmap = nullptr;
  unsigned short* d_cl_gtab = nullptr;      // [8][27 * 27] template entry that child j OWNS at (local row, local column), 0xffff = another child's (fh_assembler_galerkin from the macro rows)
  bool cl_all_rows = false;                 // every row of every cluster lies in the matrix (no ghost rows, no sink): the macro rows can be read back
  bool macro_valid = false;                 // the matrix cl_val_base and the partial-row buffer hold the macro rows of the last assembly
  uint64_t macro_uid = 0;                   // the matrix of that assembly (fh_mat_s::uid, not its address: it may be destroyed, and a later one may get the address)
  uint64_t macro_val_gen = 0;               // ... as long as nobody but SetPenalty has written the matrix since (fh_mat_s::val_gen)
  double* d_Pbuf = nullptr;
  // geometry cache of the fused assembly (option assemble_geom_cache): what phase A computes from this assembler's node coordinates alone, [nel][7][64]:
  // rows 0 .. 5 D_q, row 6 det * w, lane = Gauss point in the cluster kernel's order.  Made at the first fused assembly with a constant source.
  double* d_geo = nullptr;
  int geo_state = 0;                        // 0: not made yet, 1: made, -1: the allocation failed (phase A stays in the kernel)
  int* d_cl_prow = nullptr;                 // rows of the second pass
  unsigned* d_cl_pstart = nullptr;          // [nprow + 1] their segments of the partial-row buffer
  // arguments of the last assembly (the element-wise Galerkin product re-creates the element rows from them when the fused path ran)
  int last_source_kind = 0;
  double last_params[2] = {1.0, 0.0};
  // optional fast path for AFFINE HEX27/Q2 elements (option assemble_affine): K_e = sum_ab det*B_ab * M_ab with the nine reference
  // matrices M_ab = sum_g w_g d_a phi_i d_b phi_j, B = J^-1 J^-T; curved elements keep the quadrature kernel
  int *d_aff_elems = nullptr, *d_gen_elems = nullptr;
  int n_aff = 0, n_gen = 0;
  double *d_Mab = nullptr, *d_mphi = nullptr;
  // matrix-core element kernel (k_elem_q2hex_mfma): reference gradients T[q][c][n] (q-stride 85, c-stride 28, zero padded) and
  // shape values Phi[q][n] (stride 33)
  double *d_mfT = nullptr, *d_mfPhi = nullptr;
  double* d_mfSFc = nullptr;     // sum-factorised map Jacobian: per-lane 1-D shape values [18][64] (null: tables are not tensor products)
  int* d_mfSFi = nullptr;        // ... and per-lane LDS offsets [7][64]
  // sum-factorised element kernel (k_elem_q2hex_sf): 1-D basis values (uniform operands) and the per-lane tables
  SfTab sf_tab;
  double* d_sfLc = nullptr;      // [SF_NLC][64]
  int* d_sfLi = nullptr;         // [SF_NLI][64]
  // source term given as a compiled expression (fh_expr): device copy of the program of the expression last used
  int* d_prog = nullptr;
  double* d_prog_consts = nullptr;
  int nprog = 0;
  std::vector<int> h_prog;
  std::vector<double> h_prog_consts;
};

// the cluster-plan constants the product's k_galerkin_macro reads the plan with (the rest of the plan's layout: fh_assemble.hip)
constexpr int CL_NE = 8;                         // elements per cluster = waves per workgroup
constexpr int CL_T = CL_NE * 64;                 // threads
constexpr int CL_SPT = 10;                       // slots (macro entries) per thread
constexpr int CL_NM_MAX = 128;                   // macro nodes (125), padded

// barrier of ONE wave on its own LDS slab (the element kernels and the product's one-wave-per-element kernels)
__device__ __forceinline__ void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// phase stamps of the instrumented builds of the cluster kernel and of k_galerkin_macro (asm_debug bit 7): shader clock at the phase boundaries, summed
// per wave in scalar registers
struct SfStamps {
  unsigned long long prev, acc[16];
};
template <bool INS>
__device__ __forceinline__ void sf_stamp(SfStamps& st, const int k) {
  if (INS) {
    const unsigned long long t = __builtin_amdgcn_s_memtime();
    st.acc[k] += t - st.prev;
    st.prev = t;
  }
}

// ---- the seam between an assembly and the product: defined in fh_assemble.hip beside assemble_poisson_core, which establishes what they report ----
// the row pass: every CSR row of A sums its element rows of the element-row buffer, res the entries of the element vectors
int fh_assembler_row_pass(fh_assembler_t as, fh_mat_t A, double* res);
// makes sure the element-row buffer holds the element matrices of the last assembly (re-created from its arguments when the fused path ran), and has the
// next assembly keep them
int fh_assembler_need_element_rows(fh_assembler_t as);
// the element-row buffer was filled from outside and gathered into the assembler's matrix: it is valid, macro rows an earlier fused assembly left there are not
void fh_assembler_rows_replaced(fh_assembler_t as);
// the macro rows of the last fused assembly, if they can still be read back: all of them lie in the matrix of that assembly and its partial-row buffer, that
// matrix is alive, has the value array the plan addresses and nobody but the Dirichlet-row replacement has written it since.  ok = false otherwise.
struct MacroRows {
  bool ok = false;
  int nm = 0, ncl = 0;                               // macro nodes of the template, clusters
  const unsigned* sinfo = nullptr;                   // (row, position, template offset) of every slot
  const uint4* map = nullptr;                        // the plan word of every thread and cluster
  const unsigned long long* vdst64 = nullptr;        // [ncl][128] addresses of the macro rows
  const unsigned short* gtab = nullptr;              // [8][27 * 27] template entry that child j owns
};
MacroRows fh_assembler_macro_rows(fh_assembler_t as);
