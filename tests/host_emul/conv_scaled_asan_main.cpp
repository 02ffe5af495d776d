// conv_scaled_asan_main.cpp -- stand-alone driver of tests/test_conv_scaled_asan.py: the three functions of include/ddepth_conv_scaled.h on the host
// emulation, built with -fsanitize=address together with csrc/dd_conv.hip, csrc/dd_api_conv.cpp and ddepth_host.cpp.  Every tensor, the workspace
// and the 16-byte scale buffer are heap blocks of EXACTLY the size the API asks for, so a kernel that reads or writes one byte beyond any of them
// ends the process with a sanitizer report.  Exit status 0: every call returned DD_OK, the scale is the power of two the rule gives for the
// data, and every output is finite.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../include/ddepth.h"
#include "../../include/ddepth_conv.h"
#include "../../include/ddepth_conv_scaled.h"

// The emulation keeps its work-item stacks for the life of the process (hip_runtime.h: run_grid), which the leak check at exit would report;
// this program is about addresses, not leaks.  Everything it allocates itself is freed.
extern "C" const char* __asan_default_options() { return "detect_leaks=0"; }

namespace {

struct Shape {
  const char* name;
  int op, B, Cin, Cout, H, W;
};

// R1, T1, P1 of tests/conv_ragged_cases.py
const Shape kShapes[] = {{"R1", DD_CONV_3X3, 1, 72, 72, 5, 35}, {"T1", DD_CONV_DECONV2X2, 1, 72, 72, 3, 5}, {"P1", DD_CONV_1X1, 2, 72, 72, 5, 27}};

const int kPrecisions[] = {DD_PREC_BF16, DD_PREC_F16, DD_PREC_F16X3};

// values k / 64 with |k| <= 128, times `mul`
float* tensor(size_t n, uint32_t seed, bool fill, float mul) {
  float* p = static_cast<float*>(malloc(n * sizeof(float)));      // exactly n floats: the sanitizer's red zone starts behind the last one
  if (!p) exit(3);
  for (size_t i = 0; i < n; ++i) {
    seed = seed * 1664525u + 1013904223u;
    p[i] = fill ? mul * (float)((int)(seed >> 24) - 128) / 64.0f : NAN;
  }
  return p;
}

bool finite(const float* p, size_t n) {
  for (size_t i = 0; i < n; ++i)
    if (!std::isfinite(p[i])) return false;
  return true;
}

int run(const Shape& s, int precision) {
  const int taps = s.op == DD_CONV_3X3 ? 9 : s.op == DD_CONV_DECONV2X2 ? 4 : 1, up = s.op == DD_CONV_DECONV2X2 ? 2 : 1;
  const size_t nx = (size_t)s.B * s.Cin * s.H * s.W, nw = (size_t)taps * s.Cin * s.Cout, ny = (size_t)s.B * s.Cout * s.H * up * s.W * up;
  int64_t bytes = 0;
  if (dd_convx_workspace_bytes(s.op, s.B, s.Cin, s.Cout, s.H, s.W, precision, &bytes) != DD_OK) {
    fprintf(stderr, "%s: workspace query: %s\n", s.name, dd_conv_last_error());
    return 1;
  }
  const float tiny = 0x1p-20f;      // a training step's magnitude: |grad_y| <= 2 * 2^-20, so amax lies in [2^-20, 2^-19] and s is 2^34 or 2^33
  float *x = tensor(nx, 1, true, 1.0f), *w = tensor(nw, 2, true, 1.0f), *gy = tensor(ny, 3, true, tiny);
  float *gx = tensor(nx, 0, false, 0.0f), *gw = tensor(nw, 0, false, 0.0f);
  float* scale = tensor(4, 0, false, 0.0f);                      // exactly 16 bytes
  void* ws = nullptr;
  if (posix_memalign(&ws, 16, (size_t)bytes) != 0) exit(3);      // exactly `bytes`, 16-byte aligned
  int bad = 0;
  if (dd_conv_grad_scale(gy, (int64_t)ny, precision, scale, nullptr) != DD_OK) {
    fprintf(stderr, "%s precision %d dd_conv_grad_scale: %s\n", s.name, precision, dd_conv_last_error());
    bad = 1;
  }
  const bool pair_ok = precision == DD_PREC_BF16 ? (scale[0] == 1.0f && scale[1] == 1.0f)
                                                 : ((scale[0] == 0x1p34f || scale[0] == 0x1p33f) && scale[0] * scale[1] == 1.0f);
  if (!bad && !pair_ok) {
    fprintf(stderr, "%s precision %d: scale = {%g, %g}\n", s.name, precision, scale[0], scale[1]);
    bad = 1;
  }
  for (int dir = 1; dir < 3 && !bad; ++dir) {
    memset(ws, 0xFF, (size_t)bytes);      // arbitrary contents on entry: NaN patterns in every operand type
    const int rc = dir == 1 ? dd_convx_backward_data_scaled(s.op, gy, w, gx, ws, scale, s.B, s.Cin, s.Cout, s.H, s.W, precision, nullptr)
                            : dd_convx_backward_weight_scaled(s.op, x, gy, gw, ws, scale, s.B, s.Cin, s.Cout, s.H, s.W, precision, nullptr);
    if (rc != DD_OK) {
      fprintf(stderr, "%s precision %d direction %d: %s\n", s.name, precision, dir, dd_conv_last_error());
      bad = 1;
    }
  }
  if (!bad && !(finite(gx, nx) && finite(gw, nw))) {
    fprintf(stderr, "%s precision %d: an output is not finite\n", s.name, precision);
    bad = 1;
  }
  free(ws);
  free(x); free(w); free(gy); free(gx); free(gw); free(scale);
  return bad;
}

}  // namespace

int main() {
  int bad = 0;
  for (const Shape& s : kShapes)
    for (int precision : kPrecisions) {
      const int rc = run(s, precision);
      printf("%s precision %d: %s\n", s.name, precision, rc ? "FAILED" : "ok");
      bad |= rc;
    }
  return bad;
}
