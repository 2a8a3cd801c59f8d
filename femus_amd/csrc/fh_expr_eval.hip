// fh_expr_eval_device: the device compilation of fh_expr_device_eval seen one value per point (fh_expr_eval_many is the host compilation of the same
// function).  The assembly kernels only ever show a program's values inside a quadrature sum; this entry point is how a caller -- the test suite first --
// checks what the device math library makes of every operator and function of the grammar, non-finite values included.
#include "fh_internal.h"
#include "fh_expr_device.h"
#include <climits>

// one thread per point; x[npts * nvars] row by row
__global__ void k_expr_eval_points(const int* __restrict__ code, int ncode, const double* __restrict__ consts, const double* __restrict__ x, int nvars,
                                   int npts, double* __restrict__ values) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= npts) return;
  values[i] = fh_expr_device_eval(code, ncode, consts, x + (size_t)i * nvars);
}

extern "C" int fh_expr_eval_device(fh_ctx_t ctx, fh_expr_t e, int npts, const double* x, double* values) {
  FH_REQUIRE(ctx && e && npts >= 0, "fh_expr_eval_device: null argument");
  if (npts == 0) return 0;
  int nv = 0;
  FH_TRY(fh_expr_nvars(e, &nv));
  FH_REQUIRE(values && (x || nv == 0), "fh_expr_eval_device: null argument");
  FH_REQUIRE((int64_t)npts * std::max(nv, 1) < ((int64_t)1 << 31), "fh_expr_eval_device: %d points of %d variables: more than 2^31 numbers", npts, nv);
  FH_GUARD_BEGIN
  std::vector<int> code;
  std::vector<double> consts;
  FH_TRY(fh_expr_fetch(e, "fh_expr_eval_device: the expression", INT_MAX, code, consts));     // a point has as many entries as the expression has variables
  if (consts.empty()) consts.resize(1, 0.0);
  const int nc = (int)code.size();
  const size_t bx = (size_t)npts * nv * sizeof(double), bv = (size_t)npts * sizeof(double);
  void* dv[4] = {nullptr, nullptr, nullptr, nullptr};
  auto run = [&]() -> int {
    FH_CHECK_HIP(hipMalloc(&dv[0], code.size() * sizeof(int)));
    FH_CHECK_HIP(hipMalloc(&dv[1], consts.size() * sizeof(double)));
    FH_CHECK_HIP(hipMalloc(&dv[2], std::max<size_t>(bx, 8)));
    FH_CHECK_HIP(hipMalloc(&dv[3], bv));
    FH_CHECK_HIP(hipMemcpyAsync(dv[0], code.data(), code.size() * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
    FH_CHECK_HIP(hipMemcpyAsync(dv[1], consts.data(), consts.size() * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    if (bx) FH_CHECK_HIP(hipMemcpyAsync(dv[2], x, bx, hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(k_expr_eval_points, dim3(fh_div_up(npts, 128)), dim3(128), 0, ctx->stream, (const int*)dv[0], nc, (const double*)dv[1],
                       (const double*)dv[2], nv, npts, (double*)dv[3]);
    FH_CHECK_HIP(hipGetLastError());
    FH_CHECK_HIP(hipMemcpyAsync(values, dv[3], bv, hipMemcpyDeviceToHost, ctx->stream));
    FH_CHECK_HIP(hipStreamSynchronize(ctx->stream));
    return 0;
  };
  const int rc = run();
  for (void* q : dv)
    if (q) hipFree(q);
  return rc;
  FH_GUARD_END("fh_expr_eval_device")
}
