// swin_asan_main.cpp -- stand-alone driver of tests/test_swin_asan.py: dd_window_attention_forward (include/ddepth_swin.h) on the host emulation,
// built with -fsanitize=address,undefined together with csrc/dd_swin.hip, csrc/dd_api_swin.cpp and ddepth_host.cpp.  qkv, qkv_pad, rel_bias and
// out are heap blocks of EXACTLY their size, so a load for a padded position that goes to qkv instead of qkv_pad, a slot >= 49 that is read
// or stored, a bias read beyond [heads, 49, 49] or a store outside the image ends the process with a sanitizer report.  The shapes are the
// ragged (2, 10, 17, 3) and the sub-window (1, 4, 5, 1) ones of tests/swin_cases.py, with and without a shift and a qkv_pad, at every precision.
// Exit status 0: every call returned DD_OK and every output is finite.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>

#include "../../include/ddepth.h"
#include "../../include/ddepth_swin.h"

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

int run(const Shape& s, int precision, int shift, bool with_pad) {
  const size_t C = (size_t)32 * s.heads, tokens = (size_t)s.B * s.H * s.W;
  size_t nq = tokens * 3 * C;
  if (getenv("SWIN_ASAN_SHORT")) nq -= 4;      // self-check of the harness: a qkv 16 bytes short must be reported (the last token's v is read)
  float *qkv = tensor(nq, 1, true), *pad = tensor(3 * C, 2, true), *bias = tensor((size_t)s.heads * 49 * 49, 3, true), *out = tensor(tokens * C, 0, false);
  int bad = 0;
  const int rc = dd_window_attention_forward(qkv, with_pad ? pad : nullptr, bias, out, s.B, s.H, s.W, (int)C, s.heads, 7, shift, precision, nullptr);
  if (rc != DD_OK) {
    fprintf(stderr, "%s precision %d: %s\n", s.name, precision, dd_swin_last_error());
    bad = 1;
  }
  for (size_t i = 0; !bad && i < tokens * C; ++i) bad = !std::isfinite(out[i]);
  if (bad && rc == DD_OK) fprintf(stderr, "%s precision %d: an output is not finite (a token was not stored)\n", s.name, precision);
  free(qkv); free(pad); free(bias); free(out);
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
