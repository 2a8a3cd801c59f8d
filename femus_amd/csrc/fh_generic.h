// The resident plan of the generic Poisson assembly (fh_generic.hip): what its second builder, the one that reads a device-resident element mesh
// (fh_elemplan.hip), sees of it.  Both builders make the same object; assemble, set_coords, info and destroy do not know which one did.
#pragma once
#include "fh_internal.h"

constexpr int GP_THREADS = 256;
constexpr size_t GP_LDS_BUDGET = 64 * 1024;   // per workgroup: two workgroups and more per CU (160 KB of LDS), and no opt-in to large dynamic LDS needed
constexpr size_t GP_PROG_BYTES = 4096;        // first size of the source program's buffer
constexpr int GEN_NC = 27;                    // most nodes of an element (HEX27); the node stride of the one-shot kernel

struct GenRowShapes {
  int row_base[3];        // first element-row id of the shape (INT_MAX: no such shape)
  int nc[3];
  long long kb_base[3];   // where its element rows start in Kb / Pos
};

// What every driver makes of a mesh before anything touches the device: the shapes in the order of their first element, the tables and checks of each, and how
// many element rows every dof has.  Filled by gen_mesh (host arrays) or from the shape counts of a resident mesh; refusals begin with the entry point (`who`).
struct GenMesh {
  int ns = 0, dim = 0, ncmax = 0;
  int shapes[3] = {0, 0, 0}, nc[3] = {0, 0, 0}, nslot[3] = {0, 0, 0};     // nslot: elements of the shape
  std::vector<unsigned char> eshape;                                      // [nel] the element's index into shapes
  std::vector<double> w[3], phi[3], dphi[3];
  std::vector<int> adj_ptr;                                               // [ndof + 1] the element rows of dof d are adj_ptr[d] .. adj_ptr[d + 1]
};

struct fh_generic_assembler_s {
  fh_ctx_t ctx = nullptr;
  uint64_t mat_uid = 0;          // the matrix of create: its uid and non-zero count, never its address
  int mat_nnz = 0;
  int ndof = 0, nnode = 0, dim = 0, ns = 0, nel = 0;
  int shapes[3] = {-1, -1, -1};  // shape codes in the order of their first elements
  int nc[3] = {0, 0, 0}, ng[3] = {0, 0, 0}, lanes[3] = {0, 0, 0}, gcm[3] = {0, 0, 0}, nslot[3] = {0, 0, 0};
  bool tl[3] = {false, false, false};
  size_t lds[3] = {0, 0, 0};
  GenRowShapes rows;
  int* d_ed[3] = {nullptr, nullptr, nullptr};
  double *d_w[3] = {nullptr, nullptr, nullptr}, *d_phi[3] = {nullptr, nullptr, nullptr}, *d_dphi[3] = {nullptr, nullptr, nullptr};
  double* d_coords = nullptr;
  int *d_adj_ptr = nullptr, *d_adj = nullptr, *d_Pos = nullptr;
  double *d_Kb = nullptr, *d_Fb = nullptr;
  unsigned long long* d_miss = nullptr;
  int lpr = 1, maxrow = 1;
  size_t row_lds = 0;
  int64_t nadj = 0, nrows = 0, nent = 0;      // entries of adj, element rows, entries of Kb / Pos
  // the source program (assemble_form: all its programs back to back): consts (doubles) then code (ints) in one buffer, staged through pinned memory; uploaded
  // only when it differs from the last one
  char* d_prog = nullptr;
  char* h_prog = nullptr;
  size_t prog_cap = 0;
  hipEvent_t prog_ev = nullptr;
  bool prog_copied = false;
  std::vector<int> code;
  std::vector<double> consts;
  bool have_prog = false;
  // the quasilinear element body (fh_quasilinear.hip): its Gauss chunk, table staging and LDS per shape, chosen at the first assemble_form
  bool form_ready = false;
  int form_gcm[3] = {0, 0, 0};
  bool form_tl[3] = {false, false, false};
  size_t form_lds[3] = {0, 0, 0};
  // the transient element body (fh_transient.hip): the same three of its own, chosen at the first assemble_transient
  bool tr_ready = false;
  int tr_gcm[3] = {0, 0, 0};
  bool tr_tl[3] = {false, false, false};
  size_t tr_lds[3] = {0, 0, 0};
  // the system element body (fh_system.hip), per number of variables m = 1 .. 4: lanes per element, Gauss chunk, table staging and LDS per shape, the lanes and
  // LDS of the block row pass, and the work buffers of m^2 / m times the scalar size (m = 1: the scalar ones), all made at the first assemble_system with that m
  bool sys_ready[5] = {false, false, false, false, false};
  int sys_lanes[5][3] = {}, sys_gcm[5][3] = {};
  bool sys_tl[5][3] = {};
  size_t sys_lds[5][3] = {};
  int sys_lpr[5] = {0, 0, 0, 0, 0};
  size_t sys_row_lds[5] = {0, 0, 0, 0, 0};
  double *d_sysK[5] = {nullptr, nullptr, nullptr, nullptr, nullptr}, *d_sysF[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
  int64_t device_bytes = 0, algorithmic_bytes = 0, device_allocations = 0;
  std::vector<void*> dv;         // every device allocation but d_prog
};

// ---- the steps both builders share (fh_generic.hip) ----
// the shapes m.shapes[0 .. ns) of one dimension: dofs per element of the family and the tables of the Gauss rule; nloc: nodes per row of the caller's table
int gen_shape_tables(const char* who, int fe, int order, int nloc, GenMesh& m);
// every check that needs the matrix and the shapes only, and the host side of the object (no device allocation): sizes, the lanes of the row pass, the launch
// geometry and LDS of every shape.  m.nslot is final
int gp_plan_host(const char* who, fh_ctx_t ctx, const GenMesh& m, int nel, int nnode, fh_mat_t KK, fh_generic_assembler_t* out);
// after d_ed, d_adj_ptr, d_adj and d_coords are there (or their uploads enqueued): the tables, the work buffers (0xFF bytes under debug_poison), the program
// buffer, and the CSR position of every element entry.  *miss = ~0: done; otherwise the smallest entry the pattern does not hold, (shape index << 56) | index
// into the shape's positions, and the object is still alive for the caller's message.  On a failure the object is freed.
int gp_plan_work(const char* who, fh_generic_assembler_t as, const GenMesh& m, fh_mat_t KK, unsigned long long* miss);
// consts then code into the object's program buffer, when they are not what is already there (`who`: the entry point, for the refusals).  A set of several
// programs goes through here laid back to back in both arrays, its directory with the caller: the buffer of a single program is the set of one
int gp_upload_program(const char* who, fh_generic_assembler_t as, std::vector<int>& code, std::vector<double>& consts);
// the checks assemble and assemble_form make of their matrix and vectors
int gp_check_call(const char* who, fh_generic_assembler_t as, fh_vec_t sol, fh_mat_t KK, fh_vec_t RES);
// the row pass: Kb / Fb into KK's values and RES
void gp_launch_rows(fh_generic_assembler_t as, fh_mat_t KK, fh_vec_t RES);
void* gp_alloc(fh_generic_assembler_t as, size_t bytes);
void gp_free(fh_generic_assembler_t as);
