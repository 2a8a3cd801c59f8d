// What the element-norm passes over a resident element mesh share: the flags from the last correction (fh_elemerror.hip, which defines all of this) and the
// error norms against a known solution (fh_elemnorm.hip).
#pragma once
#include "fh_elemmesh.h"
#include "fh_elemerror_body.h"

namespace fherr {
struct EeTabs {                   // per shape code: dofs of the family, Gauss points, where w / phi / dphi start in the table buffer (doubles)
  int nc[EM_G], ng[EM_G], ow[EM_G], ophi[EM_G], odphi[EM_G];
};
struct EeHostTabs {
  EeTabs t;
  std::vector<double> buf;
  int ncmax = 0, ngmax = 0;
};
bool ee_shape(int g);
// the tables of every shape with present[g] != 0: the ones the generic assembler uploads (fhfe::shape_tables)
int ee_tables(const char* who, int dim, int fe, int order, const bool present[EM_G], EeHostTabs& H);
// the shape of k_ee_reduce on the host
double ee_fixed_sum(std::vector<double> a);
// nk arrays of n entries at d_in (stride n) -> d_out[0 .. nk); p0 / p1 hold nk * ceil(n / EE_RC) doubles each
void ee_reduce(hipStream_t st, size_t n, int nk, const double* d_in, double* p0, double* p1, double* d_out);
}  // namespace fherr
