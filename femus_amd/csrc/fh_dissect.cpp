// Nested-dissection ordering of the coupled unknowns of the coarsest level (host, once per pattern; the block form of the exact coarse solve in
// fh_coarse.hip is built on it).  The separator comes from the coordinates: the set is halved across the principal axis of its coordinates at a
// layer boundary next to the median, and the side with fewer unknowns coupled to the other side gives them up as separator.
#include "fh_internal.h"
#include <cmath>

namespace {
struct NdGraph {
  std::vector<int> ptr, adj;        // coupling graph over the coupled unknowns (positions 0 .. n), both directions
};

static void nd_split(const NdGraph& G, const double* xyz, int dim, const std::vector<int>& set, int depth, std::vector<std::vector<int> >& blocks,
                     std::vector<int>& sep, std::vector<int>& side /* scratch, size n, zero */) {
  if (depth == 0 || set.size() < 64) {
    blocks.push_back(set);
    return;
  }
  // principal axis of the set
  double mean[3] = {0, 0, 0};
  for (int u : set)
    for (int d = 0; d < dim; d++) mean[d] += xyz[(size_t)u * dim + d];
  for (int d = 0; d < dim; d++) mean[d] /= (double)set.size();
  double C[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
  for (int u : set) {
    double x[3] = {0, 0, 0};
    for (int d = 0; d < dim; d++) x[d] = xyz[(size_t)u * dim + d] - mean[d];
    for (int i = 0; i < dim; i++)
      for (int j = 0; j < dim; j++) C[i][j] += x[i] * x[j];
  }
  double v[3] = {0, 0, 0};
  int dmax = 0;
  for (int d = 1; d < dim; d++)
    if (C[d][d] > C[dmax][dmax] * (1.0 + 1e-9)) dmax = d;
  v[dmax] = 1.0;
  for (int it = 0; it < 60; it++) {
    double u[3] = {0, 0, 0}, nrm = 0.0;
    for (int i = 0; i < dim; i++)
      for (int j = 0; j < dim; j++) u[i] += C[i][j] * v[j];
    for (int i = 0; i < dim; i++) nrm += u[i] * u[i];
    nrm = sqrt(nrm);
    if (!(nrm > 0.0)) break;
    for (int i = 0; i < dim; i++) v[i] = u[i] / nrm;
  }
  std::vector<std::pair<double, int> > key(set.size());
  double span = 0.0;
  for (size_t k = 0; k < set.size(); k++) {
    double t = 0.0;
    for (int d = 0; d < dim; d++) t += v[d] * (xyz[(size_t)set[k] * dim + d] - mean[d]);
    key[k] = std::make_pair(t, set[k]);
    span = std::max(span, fabs(t));
  }
  const double q = span > 0.0 ? span * 1e-9 : 1.0;
  for (auto& kv : key) kv.first = std::floor(kv.first / q + 0.5);        // layers across the axis: equal keys
  std::sort(key.begin(), key.end());
  // candidate cuts: the layer boundaries next to the median on both sides
  const size_t half = set.size() / 2;
  size_t c_lo = half, c_hi = half;
  while (c_lo > 0 && key[c_lo - 1].first == key[c_lo].first) c_lo--;
  while (c_hi < set.size() && c_hi > 0 && key[c_hi - 1].first == key[c_hi].first) c_hi++;
  size_t best_cut = 0, best_cnt = (size_t)-1;
  int best_side = 0;
  for (size_t cut : {c_lo, c_hi}) {
    if (cut == 0 || cut >= set.size()) continue;
    for (size_t k = 0; k < set.size(); k++) side[key[k].second] = k < cut ? 1 : 2;
    size_t cntA = 0, cntB = 0;
    for (size_t k = 0; k < set.size(); k++) {
      const int u = key[k].second, mine = side[u];
      bool touches = false;
      for (int e = G.ptr[u]; e < G.ptr[u + 1] && !touches; e++) touches = side[G.adj[e]] == 3 - mine;
      if (touches) (mine == 1 ? cntA : cntB)++;
    }
    for (int which = 1; which <= 2; which++) {
      const size_t cnt = which == 1 ? cntA : cntB;
      const size_t rest = (which == 1 ? cut : set.size() - cut) - cnt;         // a side must keep unknowns
      if (rest == 0) continue;
      if (cnt < best_cnt) {
        best_cnt = cnt;
        best_cut = cut;
        best_side = which;
      }
    }
    for (size_t k = 0; k < set.size(); k++) side[key[k].second] = 0;
  }
  if (best_side == 0) {            // no usable cut (one layer): the set stays one block
    blocks.push_back(set);
    return;
  }
  for (size_t k = 0; k < set.size(); k++) side[key[k].second] = k < best_cut ? 1 : 2;
  std::vector<int> A, B;
  for (size_t k = 0; k < set.size(); k++) {
    const int u = key[k].second, mine = side[u];
    bool touches = false;
    if (mine == best_side)
      for (int e = G.ptr[u]; e < G.ptr[u + 1] && !touches; e++) touches = side[G.adj[e]] == 3 - mine;
    if (touches) sep.push_back(u);
    else (mine == 1 ? A : B).push_back(u);
  }
  for (size_t k = 0; k < set.size(); k++) side[key[k].second] = 0;
  std::sort(A.begin(), A.end());
  std::sort(B.begin(), B.end());
  nd_split(G, xyz, dim, A, depth - 1, blocks, sep, side);
  nd_split(G, xyz, dim, B, depth - 1, blocks, sep, side);
}
}  // namespace

// the ordering [interior block 0 | ... | interior block k-1 | separator] of the n unknowns of a CSR pattern (coupling in either direction counts,
// columns outside [0, n) are ignored): order[n], offsets[0 .. k + 1] (offsets[k] = first separator unknown, offsets[k + 1] = n), *n_offsets = k + 2;
// k <= max(coarse_nd, 1).  One block and the identity order when nothing is cut (coarse_nd < 2, fewer than 64 unknowns, a single layer)
extern "C" int fh_coarse_dissection(int n, const int* rowptr, const int* col, int dim, const double* coords, int coarse_nd, int* order, int* offsets,
                                    int* n_offsets) {
  FH_GUARD_BEGIN
  FH_REQUIRE(n >= 0 && rowptr && dim >= 1 && dim <= 3 && (n == 0 || (col && coords && order)) && offsets && n_offsets,
             "fh_coarse_dissection: bad arguments");
  std::vector<std::pair<int, int> > ed;
  for (int i = 0; i < n; i++)
    for (int k = rowptr[i]; k < rowptr[i + 1]; k++) {
      const int j = col[k];
      if (j >= 0 && j < n && j != i) {
        ed.emplace_back(i, j);
        ed.emplace_back(j, i);
      }
    }
  std::sort(ed.begin(), ed.end());
  ed.erase(std::unique(ed.begin(), ed.end()), ed.end());
  NdGraph G;
  G.ptr.assign(n + 1, 0);
  for (auto& e : ed) G.ptr[e.first + 1]++;
  for (int i = 0; i < n; i++) G.ptr[i + 1] += G.ptr[i];
  G.adj.resize(ed.size());
  for (size_t k = 0; k < ed.size(); k++) G.adj[k] = ed[k].second;
  int depth = 0;
  while (depth < 30 && (1 << (depth + 1)) <= coarse_nd) depth++;
  std::vector<int> all(n), side(n, 0), sep;
  for (int i = 0; i < n; i++) all[i] = i;
  std::vector<std::vector<int> > blocks;
  nd_split(G, coords, dim, all, depth, blocks, sep, side);
  std::sort(sep.begin(), sep.end());
  int at = 0, no = 0;
  for (auto& b : blocks) {
    offsets[no++] = at;
    for (int u : b) order[at++] = u;
  }
  offsets[no++] = at;          // first separator unknown
  for (int u : sep) order[at++] = u;
  offsets[no++] = at;          // = n
  *n_offsets = no;
  FH_REQUIRE(at == n, "coarse_factor: the dissection lost unknowns (%d of %d)", at, n);
  return 0;
  FH_GUARD_END("fh_coarse_dissection")
}
