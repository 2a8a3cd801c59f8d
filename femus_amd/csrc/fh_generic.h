// The resident plan of the generic Poisson assembly (fh_generic.hip): what its second builder, the one that reads a device-resident element mesh
// (fh_elemplan.hip), sees of it.  Both builders make the same object; assemble, set_coords, info and destroy do not know which one did.
#pragma once
#include "fh_internal.h"
#include <algorithm>

constexpr int GP_THREADS = 256;
constexpr size_t GP_LDS_BUDGET = 64 * 1024;   // per workgroup: two workgroups and more per CU (160 KB of LDS), and no opt-in to large dynamic LDS needed
constexpr size_t GP_PROG_BYTES = 4096;        // first size of the source program's buffer
constexpr int GEN_NC = 27;                    // most nodes of an element (HEX27); the node stride of the one-shot kernel
// entries of the nc x nc element matrix a lane holds in the bodies that form every (i, j): 729 of HEX27 on 64 lanes, at most 4 L where elements share a wave
constexpr int gp_entries_per_lane(int L) { return L == 64 ? (GEN_NC * GEN_NC + 63) / 64 : 4; }

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

// The launch geometry of one element body on the shapes of one object: lanes per element, Gauss points per chunk, whether the shape's tables are staged in
// LDS beside the chunk, and the dynamic LDS of a workgroup.  Filled by gp_plan_body, all shapes or none
struct GenBodyPlan {
  bool ready = false;
  int lanes[3] = {0, 0, 0}, gcm[3] = {0, 0, 0};
  bool tl[3] = {false, false, false};
  size_t lds[3] = {0, 0, 0};
};

struct fh_generic_assembler_s {
  fh_ctx_t ctx = nullptr;
  uint64_t mat_uid = 0;          // the matrix of create: its uid and non-zero count, never its address
  int mat_nnz = 0;
  int ndof = 0, nnode = 0, dim = 0, ns = 0, nel = 0;
  int shapes[3] = {-1, -1, -1};  // shape codes in the order of their first elements
  int nc[3] = {0, 0, 0}, ng[3] = {0, 0, 0}, nslot[3] = {0, 0, 0};
  // one plan per element body: the Poisson body's at create, the others at the first call that needs them -- the quasilinear (fh_quasilinear.hip) and the
  // transient body (fh_transient.hip) on the Poisson body's lanes, the system body (fh_system.hip) and its theta-step (fh_system_transient.hip) per number of
  // variables m = 1 .. 4 on lanes of their own
  GenBodyPlan poisson, form, transient, sys[5], systr[5];
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
  // the system bodies' block row pass and work buffers, per m: lanes per row and LDS, Kb / Fb of m^2 / m times the scalar size (m = 1: the scalar ones), made
  // with sys[m] or systr[m], whichever comes first (sy_work_buffers, fh_system.h)
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
// The plan of one element body: per shape the lanes given, the largest Gauss chunk <= 32 with which the 256 / lanes elements of a workgroup, at
// elem_doubles(nc, gc) doubles of LDS each, fit GP_LDS_BUDGET -- halved until it fits, or with `evened` stepped down by one and then evened out over the chunks
// it makes (ng = 16 at a limit of 14 goes as 8 + 8, not 14 + 2) -- and the tables staged where they still fit beside it.  Refusals, per shape in this order:
// under every_entry (the bodies that form every (i, j); the Poisson body forms pairs) the gp_entries_per_lane(L) entries of each of the L lanes do not cover
// the nc^2 entries of `entries_of` ("an element", "a block");
// the shape does not fit at one point per chunk (`body` ends that message: "" or " with the ... element body").  plan is written only when every shape fits
template <class Doubles>
int gp_plan_body(const char* who, fh_generic_assembler_t as, const int lanes[3], Doubles elem_doubles, bool evened, bool every_entry, const char* entries_of,
                 const char* body, GenBodyPlan& plan) {
  GenBodyPlan P;
  for (int k = 0; k < as->ns; k++) {
    const int L = lanes[k], epg = GP_THREADS / L, nc = as->nc[k], ng = as->ng[k];
    FH_REQUIRE(!every_entry || gp_entries_per_lane(L) * L >= nc * nc, "%s: shape %d: %d entries of %s on %d lanes", who, as->shapes[k], nc * nc, entries_of, L);
    const auto bytes = [&](int gc) { return epg * elem_doubles(nc, gc) * sizeof(double); };
    int gc = std::min(ng, 32);
    while (gc > 1 && bytes(gc) > GP_LDS_BUDGET) gc = evened ? gc - 1 : (gc + 1) / 2;
    FH_REQUIRE(bytes(gc) <= GP_LDS_BUDGET, "%s: shape %d does not fit the LDS of a workgroup%s", who, as->shapes[k], body);
    if (evened) {
      const int nchunk = (ng + gc - 1) / gc;
      gc = (ng + nchunk - 1) / nchunk;
    }
    const size_t tab = ((size_t)ng * (1 + nc + nc * as->dim)) * sizeof(double);
    P.lanes[k] = L, P.gcm[k] = gc;
    P.tl[k] = bytes(gc) + tab <= GP_LDS_BUDGET;
    P.lds[k] = bytes(gc) + (P.tl[k] ? tab : 0);
  }
  P.ready = true;
  plan = P;
  return 0;
}
// what the *_chunks exports report of a plan: 0 for a shape the mesh does not have, and for every shape before the plan is made
void gp_read_plan(fh_generic_assembler_t as, const GenBodyPlan& plan, int gauss_chunk[3], int lanes[3]);
// the <L, TL> kernel of shape k's plan: f(std::integral_constant<int, L>, std::bool_constant<TL>) is called with the plan's two
template <class F>
void gp_dispatch(const GenBodyPlan& plan, int k, F&& f) {
  using std::integral_constant;
  const bool tl = plan.tl[k];
  switch (plan.lanes[k]) {
    case 16: tl ? f(integral_constant<int, 16>(), std::true_type()) : f(integral_constant<int, 16>(), std::false_type()); break;
    case 32: tl ? f(integral_constant<int, 32>(), std::true_type()) : f(integral_constant<int, 32>(), std::false_type()); break;
    default: tl ? f(integral_constant<int, 64>(), std::true_type()) : f(integral_constant<int, 64>(), std::false_type()); break;
  }
}
// the checks assemble and assemble_form make of their matrix and vectors
int gp_check_call(const char* who, fh_generic_assembler_t as, fh_vec_t sol, fh_mat_t KK, fh_vec_t RES);
// the row pass: Kb / Fb into KK's values and RES
void gp_launch_rows(fh_generic_assembler_t as, fh_mat_t KK, fh_vec_t RES);
void* gp_alloc(fh_generic_assembler_t as, size_t bytes);
void gp_free(fh_generic_assembler_t as);
