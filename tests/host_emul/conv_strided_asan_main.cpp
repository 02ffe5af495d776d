// conv_strided_asan_main.cpp -- stand-alone driver of tests/test_conv_strided_asan.py: the 3x3 stride-2 operator of include/ddepth_conv_strided.h on
// the host emulation, built with -fsanitize=address together with csrc/dd_conv.hip, csrc/dd_api_conv.cpp and ddepth_host.cpp.  Every tensor and the
// workspace are heap blocks of EXACTLY the size the API asks for, so a kernel that reads (or writes) one byte beyond the packed weight image, the
// partial sums or a tensor -- the patch row Ho of an even H, the RGB image's 16-channel K step -- ends the process with a sanitizer report.
// Exit status 0: every call returned DD_OK and every output is finite.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../include/ddepth.h"
#include "../../include/ddepth_conv.h"
#include "../../include/ddepth_conv_strided.h"

// The emulation keeps its work-item stacks for the life of the process (hip_runtime.h: run_grid), which the leak check at exit would report;
// this program is about addresses, not leaks.  Everything it allocates itself is freed.
extern "C" const char* __asan_default_options() { return "detect_leaks=0"; }

namespace {

struct Shape {
  const char* name;
  int B, Cin, Cout, H, W;
};

// Z3 .. Z6 of tests/conv_strided_cases.py
const Shape kShapes[] = {{"Z3", 1, 64, 64, 3, 5}, {"Z4", 1, 8, 8, 1, 2}, {"Z5", 2, 3, 64, 10, 37}, {"Z6", 1, 72, 216, 7, 12}};

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

bool finite(const float* p, size_t n) {
  for (size_t i = 0; i < n; ++i)
    if (!std::isfinite(p[i])) return false;
  return true;
}

int run(const Shape& s, int precision, bool bias) {
  const int Ho = (s.H - 1) / 2 + 1, Wo = (s.W - 1) / 2 + 1;
  const size_t nx = (size_t)s.B * s.Cin * s.H * s.W, nw = (size_t)9 * s.Cin * s.Cout, ny = (size_t)s.B * s.Cout * Ho * Wo, nb = (size_t)s.Cout;
  int64_t bytes = 0;
  if (dd_conv3x3s2_workspace_bytes(s.B, s.Cin, s.Cout, s.H, s.W, precision, &bytes) != DD_OK) {
    fprintf(stderr, "%s: workspace query: %s\n", s.name, dd_conv_last_error());
    return 1;
  }
  float *x = tensor(nx, 1, true), *w = tensor(nw, 2, true), *gy = tensor(ny, 3, true), *b = tensor(nb, 4, true);
  float *y = tensor(ny, 0, false), *gx = tensor(nx, 0, false), *gw = tensor(nw, 0, false), *gb = tensor(nb, 0, false);
  const float scale[4] = {1024.0f, 1.0f / 1024.0f, 0.0f, 0.0f};      // any power of two: the f16x3 run with a bias takes the scaled twins
  const float* sc = bias && precision == DD_PREC_F16X3 ? scale : nullptr;
  void* ws = nullptr;
  if (getenv("CONV_STRIDED_ASAN_SHORT")) bytes -= 16;            // self-check of the harness: a workspace 16 bytes short must be reported
  if (posix_memalign(&ws, 16, (size_t)bytes) != 0) exit(3);      // exactly `bytes`, 16-byte aligned
  int bad = 0;
  for (int dir = 0; dir < 3 && !bad; ++dir) {
    memset(ws, 0xFF, (size_t)bytes);      // arbitrary contents on entry: NaN patterns in every operand type
    int rc;
    if (dir == 0) rc = dd_conv3x3s2_forward(x, w, bias ? b : nullptr, y, ws, s.B, s.Cin, s.Cout, s.H, s.W, precision, nullptr);
    else if (dir == 1) rc = dd_conv3x3s2_backward_data(gy, w, gx, ws, sc, s.B, s.Cin, s.Cout, s.H, s.W, precision, nullptr);
    else rc = dd_conv3x3s2_backward_weight(x, gy, gw, bias ? gb : nullptr, ws, sc, s.B, s.Cin, s.Cout, s.H, s.W, precision, nullptr);
    if (rc != DD_OK) {
      fprintf(stderr, "%s precision %d direction %d: %s\n", s.name, precision, dir, dd_conv_last_error());
      bad = 1;
    }
  }
  if (!bad && !(finite(y, ny) && finite(gx, nx) && finite(gw, nw) && (!bias || finite(gb, nb)))) {
    fprintf(stderr, "%s precision %d: an output is not finite\n", s.name, precision);
    bad = 1;
  }
  free(ws);
  free(x); free(w); free(gy); free(b); free(y); free(gx); free(gw); free(gb);
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
