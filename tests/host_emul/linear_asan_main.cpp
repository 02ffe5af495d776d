// linear_asan_main.cpp -- stand-alone driver of tests/test_linear_asan.py: dd_linear_pack and dd_linear_forward (include/swin/ddepth_linear.h) on the
// host emulation, built with -fsanitize=address,undefined together with csrc/dd_linear.hip, csrc/dd_api_linear.cpp and ddepth_host.cpp.  x, w,
// the packed image, bias, addend and y are heap blocks of EXACTLY their size, so a staged row >= M or column >= N that is read from memory, a
// bias read beyond N or a store outside [M, N] ends the process with a sanitizer report.  The shapes are "one" (1, 32, 32), "ragged"
// (340, 96, 288) and the tile edge "tile+1" (65, 64, 128) of tests/linear_cases.py, at every precision, with bias, addend and GELU.
// Exit status 0: every call returned DD_OK and every output is finite.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>

#include "../../include/ddepth.h"
#include "../../include/swin/ddepth_linear.h"

// The emulation keeps its work-item stacks for the life of the process (hip_runtime.h: run_grid), which the leak check at exit would report;
// this program is about addresses, not leaks.  Everything it allocates itself is freed.
extern "C" const char* __asan_default_options() { return "detect_leaks=0"; }

namespace {

struct Shape {
  const char* name;
  int M, K, N;
};

const Shape kShapes[] = {{"one", 1, 32, 32}, {"ragged", 340, 96, 288}, {"tile+1", 65, 64, 128}};
const int kPrecisions[] = {DD_PREC_FP32, DD_PREC_BF16, DD_PREC_F16};

void* block(size_t bytes) {
  void* raw = nullptr;
  if (posix_memalign(&raw, 16, bytes) != 0) exit(3);      // exactly `bytes`: the sanitizer's red zone starts behind the last one
  return raw;
}

float* tensor(size_t n, uint32_t seed, bool fill) {
  float* p = static_cast<float*>(block(n * sizeof(float)));
  for (size_t i = 0; i < n; ++i) {
    seed = seed * 1664525u + 1013904223u;
    p[i] = fill ? (float)((int)(seed >> 24) - 128) / 64.0f : NAN;
  }
  return p;
}

int run(const Shape& s, int precision) {
  const size_t M = s.M, K = s.K, N = s.N;
  size_t nx = M * K;
  if (getenv("LINEAR_ASAN_SHORT")) nx -= 4;      // self-check of the harness: an x 16 bytes short must be reported (the last row's last piece is read)
  float *x = tensor(nx, 1, true), *w = tensor(N * K, 2, true), *bias = tensor(N, 3, true), *addend = tensor(M * N, 4, true), *y = tensor(M * N, 0, false);
  int64_t bytes = 0;
  int bad = dd_linear_packed_bytes(s.K, s.N, precision, &bytes) != DD_OK;
  void* wp = block(bad ? 16 : (size_t)bytes);
  int rc = bad ? DD_ERR_INVALID_ARG : dd_linear_pack(w, wp, s.K, s.N, precision, nullptr);
  if (rc == DD_OK) rc = dd_linear_forward(x, wp, bias, addend, y, s.M, s.K, s.N, 1, precision, nullptr);
  if (rc != DD_OK) {
    fprintf(stderr, "%s precision %d: %s\n", s.name, precision, dd_linear_last_error());
    bad = 1;
  }
  for (size_t i = 0; !bad && i < M * N; ++i) bad = !std::isfinite(y[i]);
  if (bad && rc == DD_OK) fprintf(stderr, "%s precision %d: an output is not finite (an element was not stored)\n", s.name, precision);
  free(x); free(w); free(bias); free(addend); free(y); free(wp);
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
