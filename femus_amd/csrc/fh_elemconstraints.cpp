// Hanging-node constraints of an element mesh of any mix of the five shapes, on the host: the search of Mesh::GetAMRRestrictionAndAMRSolidMark (Mesh.cpp:1354-1830)
// over plain arrays, and the resolution of what a search wrote into rows -- the part the box meshes (fh_mesh.cpp) and the resident element meshes
// (fh_elemconstraints.hip) share.
//
// The search.  A face is an interface face when its flag is -1 and no other element holds all of its vertices.  An element with such a face is an interface
// element of its level; its interface local nodes are the nodes of those faces that the family holds.  For every pair of levels Lc < Lf, in that order, and every
// coarse interface element in element order: the finer level's interface nodes inside the element's 1 % padded bounding box and hull sphere, not dofs of the
// element, are mapped back by Newton from the nearest node's reference point; those that land inside the reference domain (eps 1e-4) hang on the element, with the
// values of the family's functions of the interface local nodes there (|v| >= 1e-10) as weights.
#include "fh_internal.h"
#include "fh_elemconstraints.h"
#include <array>
#include <cmath>
#include <functional>
#include <map>
#include <thread>
#include <unordered_map>

using namespace fhfe;

// ---- the resolution --------------------------------------------------------------------------------------------------------------------------------------------
void fh_amr_resolve(const std::vector<AmrTriple>& writes, int ndof, int mode, AmrRows& out) {
  out = AmrRows();
  out.ptr.push_back(0);
  std::vector<int> owner_level(mode == 1 ? ndof : 0, -1);
  std::unordered_map<int, std::vector<std::pair<int, double>>> raw;
  std::map<int, std::map<int, double>> rest;       // reference mode: master -> {son: value}, ordered like the reference's std::map
  for (const AmrTriple& t : writes) {
    const int ldof = t.hanging, jd = t.master;
    if (mode == 1) {              // which level describes a node: the first (coarsest) that finds it
      if (owner_level[ldof] < 0) owner_level[ldof] = t.Lc;
      if (owner_level[ldof] != t.Lc) continue;
    }
    if (mode == 0) {              // the reference's map restriction[master][son] with its diagonal marks (Mesh.cpp:1560-1567)
      auto& mrow = rest[jd];
      if (mrow.find(jd) == mrow.end()) mrow[jd] = 1.;
      mrow[ldof] = t.v;
      rest[ldof][ldof] = 10.;
      continue;
    }
    auto& row = raw[ldof];
    bool found = false;
    for (auto& e : row)
      if (e.first == jd) {
        e.second = t.v;
        found = true;
      }
    if (!found) row.emplace_back(jd, t.v);
  }
  if (mode == 0) {
    // second half of the reference function as written (Mesh.cpp:1711-1801): for every real master (diagonal mark < 5) a depth-first
    // walk through sons, grandsons, ...: restriction[master][son] += value * heredity(father); a son already present in the
    // genealogy lists of the levels above the one being filled is skipped ("alreadyFound").  For a node on the interfaces with two
    // coarser levels this keeps the direct entry and drops the path through the intermediate hanging node, so its row does not sum to
    // one -- that is the reference's result, reproduced here.
    const std::map<int, std::map<int, double>>& copy = rest;     // (read only from here on)
    std::map<int, std::vector<std::pair<int, double>>> hrow;        // hanging dof -> (master, weight)
    for (auto& kv : copy)
      if (kv.second.at(kv.first) > 5.) hrow[kv.first];
    std::vector<std::vector<int>> genealogy;
    std::vector<std::vector<double>> heredity;
    std::vector<size_t> index;
    for (auto& kv : copy) {
      const int inode = kv.first;
      if (!(kv.second.at(inode) < 5.)) continue;
      std::map<int, double> acc;
      genealogy.assign(1, std::vector<int>(1, inode));
      heredity.assign(1, std::vector<double>(1, 1.));
      index.assign(1, 0);
      size_t level = 1;
      while (level > 0) {
        const int father = genealogy[level - 1][index[level - 1]];
        const double hf = heredity[level - 1][index[level - 1]];
        genealogy.resize(level + 1);
        heredity.resize(level + 1);
        index.resize(level + 1);
        genealogy[level].clear();
        heredity[level].clear();
        index[level] = 0;
        for (auto& e : copy.at(father)) {
          const int son = e.first;
          bool found = false;
          for (size_t kl = 0; kl < level && !found; kl++)
            for (int g : genealogy[kl])
              if (g == son) {
                found = true;
                break;
              }
          if (found) continue;
          genealogy[level].push_back(son);
          heredity[level].push_back(e.second * hf);
          acc[son] += e.second * hf;
        }
        if (!genealogy[level].empty()) {
          level++;
        } else {
          bool test = true;
          while (test && level > 0) {
            index[level - 1]++;
            test = false;
            if (index[level - 1] == genealogy[level - 1].size()) {
              level--;
              test = true;
            }
          }
        }
      }
      for (auto& e : acc) hrow[e.first].emplace_back(inode, e.second);
    }
    for (auto& kv : hrow) {
      out.hang.push_back(kv.first);
      std::sort(kv.second.begin(), kv.second.end());
      for (auto& e : kv.second) {
        out.master.push_back(e.first);
        out.w.push_back(e.second);
      }
      out.ptr.push_back((int)out.master.size());
    }
    return;
  }
  // resolve masters that hang themselves (depth-first, masters in increasing dof order)
  std::unordered_map<int, std::vector<std::pair<int, double>>> res;
  std::function<const std::vector<std::pair<int, double>>&(int, int)> expand = [&](int l, int depth) -> const std::vector<std::pair<int, double>>& {
    auto it = res.find(l);
    if (it != res.end()) return it->second;
    std::vector<std::pair<int, double>> row = raw[l];
    std::sort(row.begin(), row.end());
    std::vector<std::pair<int, double>> acc;
    auto add = [&](int j, double w) {
      for (auto& e : acc)
        if (e.first == j) {
          e.second += w;
          return;
        }
      acc.emplace_back(j, w);
    };
    for (auto& e : row) {
      if (raw.count(e.first) && depth < 16) {
        const auto sub = expand(e.first, depth + 1);   // copy: the map may rehash below
        for (auto& s : sub) add(s.first, e.second * s.second);
      } else {
        add(e.first, e.second);
      }
    }
    std::sort(acc.begin(), acc.end());
    return res.emplace(l, std::move(acc)).first->second;
  };
  std::vector<int> hang;
  for (auto& kv : raw) hang.push_back(kv.first);
  std::sort(hang.begin(), hang.end());
  for (int l : hang) {
    const auto& row = expand(l, 0);
    out.hang.push_back(l);
    for (auto& e : row) {
      out.master.push_back(e.first);
      out.w.push_back(e.second);
    }
    out.ptr.push_back((int)out.master.size());
  }
}

// P_amr (n x n): identity rows for regular dofs; a hanging dof's row holds its master weights and an explicit zero on the diagonal (the reference inserts
// restriction[son][son] = 0, which keeps (son, son) in the pattern of P^T K P so that SetPenalty can put its 1 there).  false: a hanging dof >= n
bool fh_amr_prolongator_csr(const AmrRows& R, int n, std::vector<int>& rowptr, std::vector<int>& col, std::vector<double>& val) {
  rowptr.assign(n + 1, 0);
  col.clear();
  val.clear();
  size_t h = 0;
  std::vector<std::pair<int, double>> row;
  for (int i = 0; i < n; i++) {
    if (h < R.hang.size() && R.hang[h] == i) {
      row.clear();
      row.emplace_back(i, 0.0);
      for (int k = R.ptr[h]; k < R.ptr[h + 1]; k++) row.emplace_back(R.master[k], R.w[k]);
      std::sort(row.begin(), row.end());
      for (auto& e : row) {
        col.push_back(e.first);
        val.push_back(e.second);
      }
      h++;
    } else {
      col.push_back(i);
      val.push_back(1.0);
    }
    rowptr[i + 1] = (int)col.size();
  }
  return h == R.hang.size();
}

// ---- the search on host arrays ---------------------------------------------------------------------------------------------------------------------------------
namespace {
constexpr int W = 27, F = 6;
struct IfaceElem {
  int iel;
  std::vector<int> loc;           // interface-face local nodes (sorted, of the family)
};
}   // namespace

int fh_elem_amr_search_host(int dim, int nel, int nnode, const int* elem_geom, const int* elem_dof, const double* coords, const int* face_flag, const int* lev, int fe,
                            std::vector<AmrTriple>& writes) {
  writes.clear();
  // interface faces: the sorted vertices of every face, seen exactly once, and no boundary flag
  struct Key {
    std::array<int, 4> v;
    int slot;
  };
  std::vector<Key> keys;
  keys.reserve((size_t)nel * F);
  int maxlev = 0;
  for (int e = 0; e < nel; e++) {
    const int g = elem_geom[e];
    FH_REQUIRE(g >= 0 && g <= GEOM_WEDGE && g != GEOM_LINE && dim_of(g) == dim, "fh_elem_amr_constraints_host: element %d has shape code %d in a %d-dimensional mesh", e, g, dim);
    FH_REQUIRE(lev[e] >= 0, "fh_elem_amr_constraints_host: element %d has level %d", e, lev[e]);
    maxlev = std::max(maxlev, lev[e]);
    for (int k = 0; k < nloc_of(g); k++)
      FH_REQUIRE(elem_dof[(size_t)e * W + k] >= 0 && elem_dof[(size_t)e * W + k] < nnode, "fh_elem_amr_constraints_host: element %d, local node %d: id %d outside [0, %d)", e, k,
                 elem_dof[(size_t)e * W + k], nnode);
    for (int f = 0; f < nfaces_of(g); f++) {
      int fv[9];
      const int nfv = face_nodes(g, FE_LINEAR, f, fv);
      Key k{{-1, -1, -1, -1}, e * F + f};
      for (int q = 0; q < nfv; q++) k.v[q] = elem_dof[(size_t)e * W + fv[q]];
      std::sort(k.v.begin(), k.v.end());
      keys.push_back(k);
    }
  }
  std::sort(keys.begin(), keys.end(), [](const Key& a, const Key& b) { return a.v < b.v || (a.v == b.v && a.slot < b.slot); });
  std::vector<char> alone((size_t)nel * F, 0);
  for (size_t i = 0; i < keys.size();) {
    size_t j = i + 1;
    while (j < keys.size() && keys[j].v == keys[i].v) j++;
    if (j == i + 1) alone[keys[i].slot] = 1;
    i = j;
  }
  std::vector<std::vector<IfaceElem>> inter(maxlev + 1);
  for (int e = 0; e < nel; e++) {
    const int g = elem_geom[e], nc = ndofs_of(g, fe);
    std::vector<int> loc;
    for (int f = 0; f < nfaces_of(g); f++)
      if (face_flag[(size_t)e * F + f] == -1 && alone[(size_t)e * F + f]) {
        int fn[9];
        const int n = face_nodes(g, fe, f, fn);
        for (int q = 0; q < n; q++)
          if (fn[q] < nc) loc.push_back(fn[q]);
      }
    if (loc.empty()) continue;
    std::sort(loc.begin(), loc.end());
    loc.erase(std::unique(loc.begin(), loc.end()), loc.end());
    inter[lev[e]].push_back({e, std::move(loc)});
  }
  for (int Lc = 0; Lc <= maxlev; Lc++) {
    if (inter[Lc].empty()) continue;
    for (int Lf = Lc + 1; Lf <= maxlev; Lf++) {
      if (inter[Lf].empty()) continue;
      // the finer level's interface nodes, each once, ascending; a second order by x serves the box queries
      std::vector<int> ids;
      for (auto& ie : inter[Lf])
        for (int n : ie.loc) ids.push_back(elem_dof[(size_t)ie.iel * W + n]);
      std::sort(ids.begin(), ids.end());
      ids.erase(std::unique(ids.begin(), ids.end()), ids.end());
      std::vector<int> byx(ids);
      std::sort(byx.begin(), byx.end(), [&](int a, int b) {
        const double xa = coords[(size_t)a * dim], xb = coords[(size_t)b * dim];
        return xa < xb || (xa == xb && a < b);
      });
      std::vector<double> xs(byx.size());
      for (size_t k = 0; k < byx.size(); k++) xs[k] = coords[(size_t)byx[k] * dim];
      const auto& cel = inter[Lc];
      std::vector<std::vector<AmrTriple>> found(cel.size());
      auto search = [&](size_t q0, size_t q1) {
        std::vector<int> cand;
        for (size_t q = q0; q < q1; q++) {
          const IfaceElem& ie = cel[q];
          const int* ed = &elem_dof[(size_t)ie.iel * W];
          const int g = elem_geom[ie.iel], nl = nloc_of(g), nc = ndofs_of(g, fe);
          double xv[81], box[6], xc[3], r2;
          for (int i = 0; i < nl; i++)
            for (int d = 0; d < dim; d++) xv[i * dim + d] = coords[(size_t)ed[i] * dim + d];
          fh_amr_hull(dim, nl, xv, box, xc, &r2);
          cand.clear();
          const size_t k0 = std::lower_bound(xs.begin(), xs.end(), box[0]) - xs.begin();
          for (size_t k = k0; k < byx.size() && xs[k] <= box[1]; k++)
            if (fh_amr_in_hull(dim, box, xc, r2, &coords[(size_t)byx[k] * dim])) cand.push_back(byx[k]);
          std::sort(cand.begin(), cand.end());
          for (int ldof : cand) {
            bool mine = false;
            for (int i = 0; i < nc; i++) mine = mine || ed[i] == ldof;
            if (mine) continue;
            const double* xp = &coords[(size_t)ldof * dim];
            double xi[3] = {0, 0, 0}, phi[27];
            fh_amr_closest_node(g, dim, nl, xv, xp, xi);
            if (!fh_amr_inverse_map(g, dim, nl, xv, xp, xi)) continue;
            if (!fh_amr_inside(g, xi, 1e-4)) continue;
            hd::eval_basis(g, fe, xi, phi, nullptr);
            for (int n : ie.loc)
              if (!(std::fabs(phi[n]) < 1.0e-10)) found[q].push_back({ed[n], ldof, Lc, phi[n]});
          }
        }
      };
      const int nth = cel.size() >= 256 ? (int)std::max(1u, std::min(16u, std::thread::hardware_concurrency())) : 1;
      if (nth == 1) {
        search(0, cel.size());
      } else {
        std::vector<std::thread> th;
        for (int t = 0; t < nth; t++) th.emplace_back(search, cel.size() * t / nth, cel.size() * (t + 1) / nth);
        for (auto& x : th) x.join();
      }
      for (auto& v : found) writes.insert(writes.end(), v.begin(), v.end());
    }
  }
  return 0;
}

extern "C" int fh_elem_amr_constraints_host(int dim, int nel, int nnode, const int* elem_geom, const int* elem_dof, const double* coords, const int* face_flag,
                                            const int* lev, int fe, int mode, int* n_hanging, int* nnz, int* hanging, int* ptr, int* master, double* weight) {
  FH_GUARD_BEGIN
  const char* who = "fh_elem_amr_constraints_host";
  FH_REQUIRE(n_hanging && nnz && nel >= 0 && nnode >= 0, "%s: null or negative argument", who);
  FH_REQUIRE(dim == 2 || dim == 3, "%s: dim must be 2 or 3, not %d", who, dim);
  FH_REQUIRE(fe >= 0 && fe <= 2, "%s: fe must be 0 (linear), 1 (serendipity) or 2 (biquadratic), not %d", who, fe);
  FH_REQUIRE(mode == 0 || mode == 1, "%s: mode must be 0 (as the reference computes it) or 1 (coarsest level, rows sum to one), not %d", who, mode);
  FH_REQUIRE(nel == 0 || (elem_geom && elem_dof && coords && face_flag && lev), "%s: null mesh arrays", who);
  std::vector<AmrTriple> writes;
  FH_TRY(fh_elem_amr_search_host(dim, nel, nnode, elem_geom, elem_dof, coords, face_flag, lev, fe, writes));
  AmrRows R;
  fh_amr_resolve(writes, nnode, mode, R);
  if (hanging) {
    FH_REQUIRE(*n_hanging >= (int)R.hang.size() && *nnz >= (int)R.master.size(), "%s: capacity too small", who);
    fh_copy_out(hanging, R.hang);
    if (ptr) fh_copy_out(ptr, R.ptr);
    if (master) fh_copy_out(master, R.master);
    if (weight) fh_copy_out(weight, R.w);
  }
  *n_hanging = (int)R.hang.size();
  *nnz = (int)R.master.size();
  return 0;
  FH_GUARD_END("fh_elem_amr_constraints_host")
}
