// nlspn_asan_main.cpp -- stand-alone driver of tests/test_nlspn_asan.py: dd_nlspn_propagate, dd_nlspn_offset_affinity and
// dd_nlspn_guided_offset_affinity (include/ddepth_dcn.h) on the host emulation, built with -fsanitize=address,undefined together with
// csrc/dd_dcn.hip and ddepth_host.cpp.  Every tensor is a heap block of EXACTLY its size, so a window fill, a clamped pair load, an operand
// load of a lane past the right edge or a confidence sample that leaves its plane ends the process with a sanitizer report -- also where
// the neighbouring bytes belong to another tensor of the same call, which sentinels around an output cannot see.  The shapes are the edge
// shapes of tests/nlspn_cases.py (one pixel, one row, one column, a last tile one column and one row wide, exactly one tile); propagation
// runs at every k_f with the default kernel and with DD_NLSPN_KERNEL = g1, g4p and l8pq, offsets 6 N(0, 1), preserve_input, three iterations.
// Exit status 0: every call returned DD_OK and every output is finite.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>

#include "../../include/ddepth.h"
#include "../../include/ddepth_dcn.h"

// The emulation keeps its work-item stacks for the life of the process (hip_runtime.h: run_grid), which the leak check at exit would report;
// this program is about addresses, not leaks.  Everything it allocates itself is freed.
extern "C" const char* __asan_default_options() { return "detect_leaks=0"; }

namespace {

struct Shape {
  int B, H, W;
};

const Shape kShapes[] = {{1, 1, 1}, {1, 1, 2}, {1, 3, 1}, {1, 17, 65}, {2, 16, 64}};
const int kKf[] = {3, 5, 7};
const char* const kKernels[] = {nullptr, "g1", "g4p", "l8pq"};
const int kIters = 3;

std::mt19937 g_rng(20240607u);

enum Law { kNormal, kUniform, kSparse, kNaN };

float* tensor(size_t n, Law law, float scale) {
  void* raw = nullptr;
  if (posix_memalign(&raw, 16, n * sizeof(float)) != 0) exit(3);      // exactly n floats: the sanitizer's red zone starts behind the last one
  float* p = static_cast<float*>(raw);
  std::normal_distribution<float> nd(0.f, 1.f);
  std::uniform_real_distribution<float> ud(0.f, 1.f);
  for (size_t i = 0; i < n; ++i) {
    switch (law) {
      case kNormal: p[i] = scale * nd(g_rng); break;
      case kUniform: p[i] = scale * ud(g_rng); break;
      case kSparse: p[i] = ud(g_rng) < 0.05f ? 1.f + scale * ud(g_rng) : 0.f; break;
      default: p[i] = NAN;
    }
  }
  return p;
}

int all_finite(const float* p, size_t n, const char* what) {
  for (size_t i = 0; i < n; ++i)
    if (!std::isfinite(p[i])) {
      fprintf(stderr, "%s: element %zu is not finite (it was not stored)\n", what, i);
      return 1;
    }
  return 0;
}

int fail(const char* what, int rc) {
  fprintf(stderr, "%s returned %d: %s\n", what, rc, dd_dcn_last_error());
  return 1;
}

int run_propagate(const Shape& s, int k_f, const char* kernel) {
  const size_t n = (size_t)s.B * s.H * s.W, K = (size_t)k_f * k_f;
  size_t n_feat = n;
  if (getenv("NLSPN_ASAN_SHORT") && n > 4) n_feat -= 4;      // self-check of the harness: a feat_init 16 bytes short must be reported
  float *feat = tensor(n_feat, kUniform, 10.f), *offset = tensor(2 * K * n, kNormal, 6.f), *aff = tensor(K * n, kNormal, 0.1f);
  float *fix = tensor(n, kSparse, 19.f), *w = tensor(K, kNormal, 1.f), *b = tensor(1, kUniform, 1.f), *feats = tensor(kIters * n, kNaN, 0.f);
  int64_t bytes = 0;
  int bad = 0;
  int rc = dd_nlspn_workspace_bytes(s.B, s.H, s.W, 1, &bytes);
  if (rc != DD_OK || bytes != (int64_t)(2 * n * sizeof(float))) bad = fail("dd_nlspn_workspace_bytes", rc);
  float* ws = tensor(2 * n, kNaN, 0.f);
  if (kernel) setenv("DD_NLSPN_KERNEL", kernel, 1);
  else unsetenv("DD_NLSPN_KERNEL");
  if (!bad) {
    rc = dd_nlspn_propagate(feat, offset, aff, fix, w, b, feats, ws, s.B, s.H, s.W, k_f, kIters, 1, nullptr);
    if (rc != DD_OK) bad = fail("dd_nlspn_propagate", rc);
  }
  unsetenv("DD_NLSPN_KERNEL");
  if (!bad) bad = all_finite(feats, kIters * n, "feat_list") | all_finite(ws, 2 * n, "workspace");
  free(feat); free(offset); free(aff); free(fix); free(w); free(b); free(feats); free(ws);
  return bad;
}

int run_affinity(const Shape& s, int k_f) {
  const size_t n = (size_t)s.B * s.H * s.W, K = (size_t)k_f * k_f, num = K - 1;
  float *raw = tensor(3 * num * n, kNormal, 6.f), *conf = tensor(n, kUniform, 1.f), *gamma = tensor(1, kUniform, 0.f);
  float *w_conf = tensor(1, kUniform, 0.f), *b_conf = tensor(1, kUniform, 0.f);
  gamma[0] = 0.5f * (float)num; w_conf[0] = 0.7f; b_conf[0] = 0.25f;
  float *offset = tensor(2 * K * n, kNaN, 0.f), *aff = tensor(K * n, kNaN, 0.f);
  int bad = 0;
  const int rc = dd_nlspn_offset_affinity(raw, conf, gamma, w_conf, b_conf, offset, aff, s.B, s.H, s.W, k_f, DD_AFF_TGASS, 1, k_f == 5, nullptr);
  if (rc != DD_OK) bad = fail("dd_nlspn_offset_affinity", rc);
  if (!bad) bad = all_finite(offset, 2 * K * n, "offset") | all_finite(aff, K * n, "aff");
  free(raw); free(conf); free(gamma); free(w_conf); free(b_conf); free(offset); free(aff);
  return bad;
}

int run_guided(const Shape& s) {
  const size_t n = (size_t)s.B * s.H * s.W;
  float *guide = tensor(8 * n, kNormal, 1.f), *cw = tensor(24 * 8 * 9, kNormal, 0.7f), *cb = tensor(24, kNormal, 0.1f), *conf = tensor(n, kUniform, 1.f);
  float *gamma = tensor(1, kUniform, 0.f), *w_conf = tensor(1, kUniform, 0.f), *b_conf = tensor(1, kUniform, 0.f);
  gamma[0] = 4.f; w_conf[0] = 0.7f; b_conf[0] = 0.25f;      // conv weights of deviation 0.7: offsets of deviation 6
  float *offset = tensor(18 * n, kNaN, 0.f), *aff = tensor(9 * n, kNaN, 0.f);
  int bad = 0;
  const int rc = dd_nlspn_guided_offset_affinity(guide, cw, cb, conf, gamma, w_conf, b_conf, offset, aff, s.B, 8, s.H, s.W, 3, 3, DD_AFF_TGASS, 1, 1, nullptr);
  if (rc != DD_OK) bad = fail("dd_nlspn_guided_offset_affinity", rc);
  if (!bad) bad = all_finite(offset, 18 * n, "offset") | all_finite(aff, 9 * n, "aff");
  free(guide); free(cw); free(cb); free(conf); free(gamma); free(w_conf); free(b_conf); free(offset); free(aff);
  return bad;
}

}  // namespace

int main() {
  int bad = 0;
  for (const Shape& s : kShapes) {
    for (int k_f : kKf) {
      for (const char* kernel : kKernels) {
        const int rc = run_propagate(s, k_f, kernel);
        printf("propagate %dx%dx%d k_f %d kernel %s: %s\n", s.B, s.H, s.W, k_f, kernel ? kernel : "default", rc ? "FAILED" : "ok");
        bad |= rc;
      }
      const int rc = run_affinity(s, k_f);
      printf("affinity %dx%dx%d k_f %d: %s\n", s.B, s.H, s.W, k_f, rc ? "FAILED" : "ok");
      bad |= rc;
    }
    const int rc = run_guided(s);
    printf("guided %dx%dx%d: %s\n", s.B, s.H, s.W, rc ? "FAILED" : "ok");
    bad |= rc;
  }
  return bad;
}
