// The device-resident element mesh (fh_elemmesh.hip): what the builders of its transfers and boundary lists (fh_elemtransfer.hip) and of its hanging-node
// constraints (fh_elemconstraints.hip) see of it.
#pragma once
#include "fh_internal.h"
#include <memory>

constexpr int EM_W = 27, EM_F = 6, EM_G = 6;      // widths of the padded element and face rows; shape codes 0 .. 5 (2 = line: not a mesh shape here)

struct EmTab {                    // per shape code; lives in device memory
  int nv[EM_G], ne[EM_G], nl[EM_G], nf[EM_G], ep[EM_G];     // ends of the vertex / edge-node / all classes, faces, first double of the shape's prolongator
  signed char f2c[EM_G][8][8];            // [child][child vertex] -> father's local node
  signed char edge_v[EM_G][12][2];        // the two vertices of edge node nv + m
  signed char face_of[EM_G][EM_W];        // local node -> the face it is the last node of (-1: none)
  signed char nvf[EM_G][EM_F];            // vertices per face
  signed char face_v[EM_G][EM_F][4];
  signed char face_diag[EM_G][EM_F][4];   // quadrilateral faces: position of the vertex diagonal to vertex k
  signed char cff[EM_G][8][EM_F];         // [child][child face] -> father's face whose flag it inherits (-1: none)
};
struct EmDevTables {
  EmTab* d_tab = nullptr;
  double* d_EP = nullptr;
  ~EmDevTables() {
    if (d_tab) hipFree(d_tab);
    if (d_EP) hipFree(d_EP);
  }
};

struct fh_elem_mesh_s {
  fh_ctx_t ctx = nullptr;
  int dim = 0, nel = 0, nnode = 0, own[3] = {0, 0, 0}, level = 0;
  int64_t count[EM_G] = {0, 0, 0, 0, 0, 0};      // elements per shape: sizes every allocation of a refinement without asking the device
  int* d_geom = nullptr;          // [nel]
  int* d_ed = nullptr;            // [nel * 27], -1 beyond the shape's width
  double* d_x = nullptr;          // [nnode * dim]
  int* d_ff = nullptr;            // [nel * 6], -1 beyond the shape's faces
  int* d_lev = nullptr;           // [nel] level of every element (a copy of a flagged refinement keeps its own)
  int* d_father = nullptr;        // [nel] element of the mesh this one was refined from (-1: a mesh built from host arrays)
  int* d_child = nullptr;         // [nel] which child of its father (-1: its unchanged copy, or no father)
  unsigned char* d_flags = nullptr;               // [nel] what fh_elem_mesh_flag left (null until then)
  bool homogeneous = true;        // every element is of the mesh's level
  std::shared_ptr<EmDevTables> tab;               // shared along a chain of refinements
  bool levels_unset = false;      // built from host arrays and fh_elem_mesh_set_levels never called: "homogeneous" is then only what nobody contradicted
  std::shared_ptr<struct AmrRows> amr_pending;    // rows the sizing call of fh_elem_mesh_amr_constraints found, for the filling call that follows it (then dropped)
  int amr_pending_key = -1;
  double amr_ms[3] = {0.0, 0.0, 0.0};             // the last search: search (kernels, or the host search), download, resolution
  ~fh_elem_mesh_s() {
    for (void* q : {(void*)d_geom, (void*)d_ed, (void*)d_x, (void*)d_ff, (void*)d_lev, (void*)d_father, (void*)d_child, (void*)d_flags})
      if (q) hipFree(q);
  }
};

// ---- the open-addressing tables of edge and face keys (the refinement's; the interface faces of fh_elemconstraints.hip are counted in tables of the same kind) ----
constexpr unsigned long long EM_EMPTY = ~0ull;
// plain read, then CAS, then the returned value: a stale plain read can only show "empty", and the CAS corrects it (fh_meshdev.hip: rf_insert)
__device__ __forceinline__ int em_insert(unsigned long long* keys, unsigned mask, int shift, unsigned long long key) {
  unsigned s = (unsigned)((key * 0x9E3779B97F4A7C15ull) >> shift) & mask;
  for (;;) {
    unsigned long long old = keys[s];
    if (old == key) return (int)s;
    if (old == EM_EMPTY) {
      old = atomicCAS(&keys[s], EM_EMPTY, key);
      if (old == EM_EMPTY || old == key) return (int)s;
    }
    s = (s + 1) & mask;
  }
}
__device__ __forceinline__ unsigned long long em_pair(int a, int b) { return ((unsigned long long)(unsigned)a << 32) | (unsigned)b; }

struct EmHash {
  unsigned long long* keys;
  unsigned mask;
  int shift, id0;                 // id0: the first provisional id of the family
};


// device work buffers of one entry point, freed on return
struct EmScratch {
  const char* who;                // the entry point, for the message
  std::vector<void*> p;
  explicit EmScratch(const char* w) : who(w) {}
  ~EmScratch() {
    for (void* q : p)
      if (q) hipFree(q);
  }
  template <class T>
  int get(T** out, size_t n) {
    void* q = nullptr;
    if (hipMalloc(&q, std::max<size_t>(n, 2) * sizeof(T)) != hipSuccess) {
      fh_set_error("%s: out of device memory", who);
      return 2;
    }
    p.push_back(q);
    *out = (T*)q;
    return 0;
  }
};
