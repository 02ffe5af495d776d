// swin_backward_asan_main.cpp -- stand-alone driver of tests/test_swin_backward_asan.py: dd_window_attention_backward
// (include/train/ddepth_swin_backward.h) on the host emulation, built with -fsanitize=address,undefined together with csrc/dd_swin_bwd.hip,
// csrc/dd_api_swin_bwd.cpp, the forward's two units and ddepth_host.cpp.  Every tensor and the workspace are heap blocks of EXACTLY their size
// (the workspace: what dd_window_attention_backward_workspace_bytes answers), so a load for a padded position that goes to qkv or grad_out, a
// slot >= 49 that is read or stored, a partial written beyond the workspace or a store outside the image ends the process with a sanitizer
// report.  The shapes are the ragged (2, 10, 17, 3) and the sub-window (1, 4, 5, 1) ones of tests/swin_cases.py, with and without a shift and a
// qkv_pad, at every precision.  Exit status 0: every call returned DD_OK and every output is finite.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>

#include "../../include/ddepth.h"
#include "../../include/ddepth_swin.h"
#include "../../include/train/ddepth_swin_backward.h"

// The emulation keeps its work-item stacks for the life of the process (hip_runtime.h: run_grid), which the leak check at exit would report;
// this program is about addresses, not leaks.  Everything it allocates itself is freed.
extern "C" const char* __asan_default_options() { return "detect_leaks=0"; }

namespace {

struct Shape {
  const char* name;
  int B, H, W, heads;
};

const Shape kShapes[] = {{"ragged", 2, 10, 17, 3}, {"sub", 1, 4, 5, 1}};
const int kPrecisions[] = {DD_PREC_FP32, DD_PREC_BF16, DD_PREC_F16};

float* tensor(size_t n, uint32_t seed, bool fill) {
  void* raw = nullptr;
  if (posix_memalign(&raw, 16, n * sizeof(float)) != 0) exit(3);      // exactly n floats: the sanitizer's red zone starts behind the last one
  float* p = static_cast<float*>(raw);
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

int run(const Shape& s, int precision, int shift, bool with_pad) {
  const size_t C = (size_t)32 * s.heads, tokens = (size_t)s.B * s.H * s.W, nb = (size_t)s.heads * 49 * 49;
  size_t ng = tokens * C;
  if (getenv("SWIN_BWD_ASAN_SHORT")) ng -= 4;      // self-check of the harness: a grad_out 16 bytes short must be reported (the last token's row is read)
  int64_t ws_bytes = 0;
  if (dd_window_attention_backward_workspace_bytes(s.B, s.H, s.W, (int)C, s.heads, 7, precision, &ws_bytes) != DD_OK || ws_bytes <= 0) {
    fprintf(stderr, "%s precision %d: workspace query: %s\n", s.name, precision, dd_swin_last_error());
    return 1;
  }
  float *qkv = tensor(tokens * 3 * C, 1, true), *pad = tensor(3 * C, 2, true), *bias = tensor(nb, 3, true), *gout = tensor(ng, 4, true);
  float *gq = tensor(tokens * 3 * C, 0, false), *gp = tensor(3 * C, 0, false), *gb = tensor(nb, 0, false);
  float* ws = tensor((size_t)ws_bytes / sizeof(float), 0, false);
  float scale[4] = {4096.0f, 1.0f / 4096.0f, 0.0f, 0.0f};
  int bad = 0;
  const int rc = dd_window_attention_backward(qkv, with_pad ? pad : nullptr, bias, gout, gq, gp, gb, ws, with_pad ? scale : nullptr, s.B, s.H, s.W,
                                              (int)C, s.heads, 7, shift, precision, nullptr);
  if (rc != DD_OK) {
    fprintf(stderr, "%s precision %d: %s\n", s.name, precision, dd_swin_last_error());
    bad = 1;
  }
  if (!bad && !(finite(gq, tokens * 3 * C) && finite(gp, 3 * C) && finite(gb, nb))) {
    fprintf(stderr, "%s precision %d: an output is not finite (an element was not stored)\n", s.name, precision);
    bad = 1;
  }
  free(qkv); free(pad); free(bias); free(gout); free(gq); free(gp); free(gb); free(ws);
  return bad;
}

}  // namespace

int main() {
  int bad = 0;
  for (const Shape& s : kShapes)
    for (int precision : kPrecisions)
      for (int shift = 0; shift <= 3; shift += 3)
        for (int pad = 0; pad < 2; ++pad) {
          const int rc = run(s, precision, shift, pad != 0);
          printf("%s precision %d shift %d pad %d: %s\n", s.name, precision, shift, pad, rc ? "FAILED" : "ok");
          bad |= rc;
        }
  return bad;
}
