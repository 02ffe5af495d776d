// conv_stats_asan_main.cpp -- stand-alone driver of tests/test_conv_stats_asan.py: the statistics-emitting forward of include/ddepth_conv_stats.h on
// the host emulation, built with -fsanitize=address,undefined together with csrc/dd_conv.hip, csrc/dd_api_conv.cpp and ddepth_host.cpp.  Every
// tensor, the bias, sums and the workspace are heap blocks of EXACTLY the size the API asks for, so a kernel that reads the bias for a row >= N,
// writes a partial for such a row or for a tile that does not exist, stores y outside its plane, or touches one byte beyond the packed weight
// image or the partials ends the process with a sanitizer report.
// Exit status 0: every call returned DD_OK, every output is finite and sums[2 Cout] is the element count.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../include/ddepth.h"
#include "../../include/ddepth_conv.h"
#include "../../include/ddepth_conv_stats.h"

// The emulation keeps its work-item stacks for the life of the process (hip_runtime.h: run_grid), which the leak check at exit would report;
// this program is about addresses, not leaks.  Everything it allocates itself is freed.
extern "C" const char* __asan_default_options() { return "detect_leaks=0"; }

namespace {

struct Shape {
  const char* name;
  int stride, B, Cin, Cout, H, W;
};

// S3, R1, R5 (stride 1) and Z4, Z5, Z6 (stride 2) of tests/conv_stats_cases.py
const Shape kShapes[] = {{"S3", 1, 1, 64, 64, 3, 5}, {"R1", 1, 1, 72, 72, 5, 35}, {"R5", 1, 1, 8, 24, 3, 5},
                         {"Z4", 2, 1, 8, 8, 1, 2},   {"Z5", 2, 2, 3, 64, 10, 37}, {"Z6", 2, 1, 72, 216, 7, 12}};

const int kPrecisions[] = {DD_PREC_BF16, DD_PREC_F16X3};

float* tensor(size_t n, uint32_t seed, bool fill) {
  float* p = static_cast<float*>(malloc(n * sizeof(float)));      // exactly n floats: the sanitizer's red zone starts behind the last one
  if (!p) exit(3);
  for (size_t i = 0; i < n; ++i) {
    seed = seed * 1664525u + 1013904223u;
    p[i] = fill ? (float)((int)(seed >> 24) - 128) / 64.0f : NAN;
  }
  return p;
}

int run(const Shape& s, int precision, bool with_bias) {
  const int Ho = s.stride == 2 ? (s.H - 1) / 2 + 1 : s.H, Wo = s.stride == 2 ? (s.W - 1) / 2 + 1 : s.W;
  const size_t nx = (size_t)s.B * s.Cin * s.H * s.W, nw = (size_t)9 * s.Cin * s.Cout, ny = (size_t)s.B * s.Cout * Ho * Wo, nc = (size_t)s.Cout;
  int64_t bytes = 0;
  if (dd_conv3x3_stats_workspace_bytes(s.stride, s.B, s.Cin, s.Cout, s.H, s.W, precision, &bytes) != DD_OK) {
    fprintf(stderr, "%s: workspace query: %s\n", s.name, dd_conv_last_error());
    return 1;
  }
  float *x = tensor(nx, 1, true), *w = tensor(nw, 2, true), *bias = tensor(nc, 3, true), *y = tensor(ny, 0, false);
  double* sums = static_cast<double*>(malloc((2 * nc + 1) * sizeof(double)));      // exactly [2 Cout + 1]
  if (!sums) exit(3);
  for (size_t i = 0; i < 2 * nc + 1; ++i) sums[i] = NAN;
  void* ws = nullptr;
  if (getenv("CONV_STATS_ASAN_SHORT")) bytes -= 16;              // self-check of the harness: a workspace 16 bytes short must be reported
  if (posix_memalign(&ws, 16, (size_t)bytes) != 0) exit(3);      // exactly `bytes`, 16-byte aligned
  memset(ws, 0xFF, (size_t)bytes);                               // arbitrary contents on entry: NaN patterns in every operand type
  int bad = 0;
  const int rc = dd_conv3x3_stats_forward(x, w, with_bias ? bias : nullptr, y, sums, ws, s.stride, s.B, s.Cin, s.Cout, s.H, s.W, precision, nullptr);
  if (rc != DD_OK) {
    fprintf(stderr, "%s precision %d: %s\n", s.name, precision, dd_conv_last_error());
    bad = 1;
  }
  for (size_t i = 0; !bad && i < ny; ++i) bad = !std::isfinite(y[i]);
  for (size_t i = 0; !bad && i < 2 * nc + 1; ++i) bad = !std::isfinite(sums[i]);
  if (!bad && sums[2 * nc] != (double)s.B * Ho * Wo) bad = 1;
  if (bad && rc == DD_OK) fprintf(stderr, "%s precision %d: an output is not finite, or the count is wrong\n", s.name, precision);
  free(ws);
  free(x); free(w); free(bias); free(y); free(sums);
  return bad;
}

}  // namespace

int main() {
  int bad = 0;
  for (const Shape& s : kShapes)
    for (int precision : kPrecisions)
      for (int bias = 0; bias < 2; ++bias) {
        const int rc = run(s, precision, bias != 0);
        printf("%s precision %d bias %d: %s\n", s.name, precision, bias, rc ? "FAILED" : "ok");
        bad |= rc;
      }
  return bad;
}
