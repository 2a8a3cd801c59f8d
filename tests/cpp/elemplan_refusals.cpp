// The host-only parts of fh_elemplan.hip -- argument checks and sizing, everything before the first device allocation -- as a stand-alone program for a
// sanitizer run on a machine without a GPU.  The meshes and matrices are host structs filled by hand (no fh_init, no device memory): every call below must come
// back with its refusal, or, for the last ones, get through the sizing and stop at the first device allocation.
//   make -C femus_amd/csrc OUT=$DIR CXXFLAGS="-O1 -g -std=c++17 -fPIC --offload-arch=gfx950 -ffp-contract=on -Xarch_host -fsanitize=address,undefined"
//   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined -fsanitize=address,undefined -Ifemus_amd/csrc \
//         -x hip tests/cpp/elemplan_refusals.cpp -L$DIR -lfemus_hip -Wl,-rpath,$DIR -o $DIR/elemplan_refusals && $DIR/elemplan_refusals
#include <cstdio>
#include <cstring>
#include "fh_elemmesh.h"

static int fails = 0;
static void refused(int rc, const char* words, int line) {
  const char* msg = fh_last_error();
  if (rc == 0 || !msg || !strstr(msg, words)) {
    printf("FAIL line %d: rc %d, message \"%s\", expected \"%s\"\n", line, rc, msg ? msg : "", words);
    fails++;
  }
}
#define REFUSED(call, words) refused((call), (words), __LINE__)

int main() {
  fh_ctx_s ctx, other;
  fh_elem_mesh_s tets;            // 5 tetrahedra, the counts alone: no call below may reach a device pointer
  tets.ctx = &ctx, tets.dim = 3, tets.nel = 5, tets.nnode = 60, tets.level = 0;
  tets.own[0] = 8, tets.own[1] = 30, tets.own[2] = 60;
  tets.count[4] = 5;
  fh_mat_s K;
  K.ctx = &ctx, K.m = K.n = 60, K.nnz = 60;
  K.h_rowptr.resize(61);
  for (int r = 0; r <= 60; r++) K.h_rowptr[r] = r;
  fh_mat_t M = nullptr;
  fh_generic_assembler_t as = nullptr;
  const char* fe_words = "fe must be 0 (linear), 1 (serendipity) or 2 (biquadratic)";

  REFUSED(fh_elem_mesh_matrix(nullptr, 2, &M), "null argument");
  REFUSED(fh_elem_mesh_matrix(&tets, 3, &M), fe_words);
  REFUSED(fh_generic_assembler_create_from_mesh(nullptr, 2, 3, &K, &as), "null argument");
  REFUSED(fh_generic_assembler_create_from_mesh(&tets, -1, 3, &K, &as), fe_words);
  REFUSED(fh_generic_assembler_create_from_mesh(&tets, 1, 3, &K, &as), "it must be square of the 30 dofs the family owns");
  K.ctx = &other;
  REFUSED(fh_generic_assembler_create_from_mesh(&tets, 2, 3, &K, &as), "different contexts");
  K.ctx = &ctx;
  REFUSED(fh_generic_assembler_create_from_mesh(&tets, 2, 99, &K, &as), "unsupported Gauss rule");
  {
    fh_elem_mesh_s m = tets;      // (a copy shares nothing: every device pointer is null)
    m.count[4] = 4;
    REFUSED(fh_generic_assembler_create_from_mesh(&m, 2, 3, &K, &as), "the shape counts of the mesh give 4 elements, it has 5");
    m.count[4] = 2, m.count[0] = m.count[5] = m.count[1] = 1;
    REFUSED(fh_generic_assembler_create_from_mesh(&m, 2, 3, &K, &as), "more than three shapes");
    m.count[0] = 0, m.count[4] = 3;
    REFUSED(fh_generic_assembler_create_from_mesh(&m, 2, 3, &K, &as), "the shapes of one mesh have one dimension");
    m.count[1] = m.count[5] = 0, m.count[2] = 2;
    REFUSED(fh_generic_assembler_create_from_mesh(&m, 2, 3, &K, &as), "of shape code 2");
    m = tets;
    m.nel = 0, m.count[4] = 0;
    REFUSED(fh_generic_assembler_create_from_mesh(&m, 2, 3, &K, &as), "an empty mesh");
  }
  {                               // a row longer than the row pass holds: the sizing itself
    fh_mat_s wide = K;
    wide.h_rowptr[60] = 100000;
    wide.nnz = 100000;
    REFUSED(fh_generic_assembler_create_from_mesh(&tets, 2, 3, &wide, &as), "is longer than the row pass holds");
  }

  int n = 0, flags[2] = {-2, -3}, buf[16];
  double xy[16];
  REFUSED(fh_elem_mesh_boundary_faces(&tets, 4, 2, flags, &n, nullptr, nullptr, nullptr, nullptr), fe_words);
  REFUSED(fh_elem_mesh_boundary_faces(&tets, 2, 2, nullptr, &n, nullptr, nullptr, nullptr, nullptr), "2 flags and no list of them");
  REFUSED(fh_elem_mesh_boundary_faces(&tets, 2, 2, flags, nullptr, nullptr, nullptr, nullptr, nullptr), "null argument");
  REFUSED(fh_elem_mesh_boundary_faces(&tets, 2, 2, flags, &n, buf, nullptr, buf, buf), "all four arrays, or none of them");
  REFUSED(fh_elem_mesh_boundary_owners(&tets, 2, 2, flags, &n, buf, nullptr, xy), "all three arrays, or none of them");
  REFUSED(fh_elem_mesh_boundary_owners(&tets, 2, -1, flags, &n, nullptr, nullptr, nullptr), "-1 flags");
  n = 3;                          // no flags: the empty list, and a caller that expects three entries is told
  REFUSED(fh_elem_mesh_boundary_owners(&tets, 2, 0, nullptr, &n, buf, buf, xy), "the list has 0 entries");
  REFUSED(fh_elem_mesh_boundary_faces(&tets, 2, 0, nullptr, &n, buf, buf, buf, buf), "the list has 0 entries");
  n = 7;
  if (fh_elem_mesh_boundary_faces(&tets, 2, 0, nullptr, &n, nullptr, nullptr, nullptr, nullptr) != 0 || n != 0) {
    printf("FAIL: no flags must give no faces\n");
    fails++;
  }

  // good arguments: through every check and the sizing, up to the first device allocation, which a machine without a GPU refuses.  Only there: with a
  // device the call would go on to read the mesh, and this one has no arrays
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) {
    const int rc = fh_generic_assembler_create_from_mesh(&tets, 2, 3, &K, &as);
    printf("good arguments: rc %d (%s)\n", rc, fh_last_error());
    if (rc == 0) {
      printf("FAIL: a plan without a device\n");
      fails++;
    }
  } else {
    printf("a device is present: the call with good arguments is left out\n");
  }
  printf(fails ? "%d FAILED\n" : "all refusals as stated\n", fails);
  return fails ? 1 : 0;
}
