// dd_api_linear.cpp -- the C ABI of include/swin/ddepth_linear.h: argument checks and the launches; the kernels are in dd_linear.hip.
#include "../../include/ddepth.h"
#include "../../include/swin/ddepth_linear.h"
#include "dd_linear.h"
#include "dd_status.h"

#include <cstdint>

namespace {

thread_local ddstatus::LastError g_linear_err;

int mode_of(int precision) { return precision == DD_PREC_FP32 ? 0 : precision == DD_PREC_BF16 ? 1 : precision == DD_PREC_F16 ? 2 : -1; }
bool width_ok(int v) { return v >= 32 && v <= 8192 && v % 32 == 0; }

// the checks that pack and forward share: DD_OK, or the status recorded in g_linear_err
int check_shape(int K, int N, int precision) {
  if (mode_of(precision) < 0) return g_linear_err.fail(DD_ERR_UNSUPPORTED, "precision %d: DD_PREC_FP32, DD_PREC_BF16 or DD_PREC_F16", precision);
  if (!width_ok(K) || !width_ok(N))
    return g_linear_err.fail(DD_ERR_UNSUPPORTED, "K = %d, N = %d: multiples of 32 in 32 .. 8192 only", K, N);
  return DD_OK;
}

}  // namespace

extern "C" {

const char* dd_linear_last_error(void) { return g_linear_err.text.c_str(); }

int dd_linear_supported(int K, int N, int act, int precision) {
  return width_ok(K) && width_ok(N) && (act == 0 || act == 1) && mode_of(precision) >= 0;
}

int dd_linear_packed_bytes(int K, int N, int precision, int64_t* bytes) {
  if (!bytes) return g_linear_err.fail(DD_ERR_INVALID_ARG, "null pointer");
  if (const int rc = check_shape(K, N, precision)) return rc;
  *bytes = (int64_t)N * K * ddlinear::operand_bytes(mode_of(precision));
  return DD_OK;
}

int dd_linear_pack(const float* w, void* wp, int K, int N, int precision, void* stream) {
  if (!w || !wp) return g_linear_err.fail(DD_ERR_INVALID_ARG, "null pointer");
  if (const int rc = check_shape(K, N, precision)) return rc;
  if ((const void*)w == wp) return g_linear_err.fail(DD_ERR_INVALID_ARG, "wp may not alias w");
  if ((((uintptr_t)w | (uintptr_t)wp) & 15) != 0) return g_linear_err.fail(DD_ERR_INVALID_ARG, "w and wp must be 16-byte aligned");
  DD_STATUS_HIP(g_linear_err, ddlinear::launch_linear_pack(w, wp, K, N, mode_of(precision), (hipStream_t)stream));
  return DD_OK;
}

int dd_linear_forward(const float* x, const void* wp, const float* bias, const float* addend, float* y, long long M, int K, int N, int act,
                      int precision, void* stream) {
  if (!x || !wp || !y) return g_linear_err.fail(DD_ERR_INVALID_ARG, "null pointer");
  if (M < 1) return g_linear_err.fail(DD_ERR_INVALID_ARG, "M must be positive (got %lld)", M);
  if (const int rc = check_shape(K, N, precision)) return rc;
  if (act != 0 && act != 1) return g_linear_err.fail(DD_ERR_UNSUPPORTED, "act %d: 0 (none) or 1 (GELU, erf form)", act);
  if ((const void*)y == (const void*)x || (const void*)y == wp || (bias && y == bias) || (addend && y == addend))
    return g_linear_err.fail(DD_ERR_INVALID_ARG, "y may not alias an input");
  if ((((uintptr_t)x | (uintptr_t)wp | (uintptr_t)addend | (uintptr_t)y) & 15) != 0)
    return g_linear_err.fail(DD_ERR_INVALID_ARG, "x, wp, addend and y must be 16-byte aligned");
  if (((uintptr_t)bias & 3) != 0) return g_linear_err.fail(DD_ERR_INVALID_ARG, "bias must be 4-byte aligned");
  // one workgroup per tile on a one-dimensional grid
  const int bm = ddlinear::tile_rows(M, N, mode_of(precision));
  const long long tiles = ((M + bm - 1) / bm) * ((N + ddlinear::kTileN - 1) / ddlinear::kTileN);
  if (M > ((long long)1 << 40) || tiles > 0x7fffffffLL)
    return g_linear_err.fail(DD_ERR_INVALID_ARG, "M = %lld: %lld tiles, at most 2^31 - 1 per call", M, tiles);
  DD_STATUS_HIP(g_linear_err, ddlinear::launch_linear(x, wp, bias, addend, y, M, K, N, act, mode_of(precision), (hipStream_t)stream));
  return DD_OK;
}

}  // extern "C"
