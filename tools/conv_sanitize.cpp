// conv_sanitize.cpp -- a stand-alone AddressSanitizer / UBSan run of the twelve entry points of include/ddepth_conv.h on the CPU: the two
// translation units are compiled for the host on top of tests/host_emul (the kernels execute work-item by work-item), every tensor and the
// workspace is an exact-size heap block, so a read or write one element outside any of them stops the program.  Shapes S1, S3, S4 and D2 of
// tests/conv_cases.py and the pointwise shapes P1, P3 and P5 of tests/conv_pw_cases.py on integer data in {-1, 0, 1}; the small shapes (S3, D2,
// P3, P5) are also compared with a direct evaluation, which must be equal.
//
// Build and run from the repository root (no GPU, nothing loaded into python):
//   /opt/rocm/lib/llvm/bin/clang++ -std=c++17 -O1 -g -mf16c -DDD_HOST_EMULATION -Wno-psabi -Wno-unused-value -fsanitize=address,undefined \
//       -fno-sanitize-recover=undefined -I tests/host_emul -I diffusiondepth_amd/csrc -x c++ diffusiondepth_amd/csrc/dd_conv.hip \
//       diffusiondepth_amd/csrc/dd_api_conv.cpp tests/host_emul/ddepth_host.cpp tools/conv_sanitize.cpp -o build/conv_sanitize
//   ASAN_OPTIONS=detect_stack_use_after_return=0:detect_leaks=0 build/conv_sanitize      # one line per shape and precision, then "CONV-SANITIZE-OK"
// (the emulation switches between work-item stacks of its own, which the stack-use-after-return mode's fake stacks cannot follow, and keeps
// those 256 stacks for the life of the process, which the leak check at exit would report; every block of THIS program is freed).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../include/ddepth.h"
#include "../include/ddepth_conv.h"

namespace {

struct Shape {
  const char* name;
  int op, B, Cin, Cout, H, W;
  bool compare;
};

uint32_t g_state = 12345u;
float next_value() {      // -1, 0 or 1
  g_state = g_state * 1664525u + 1013904223u;
  return (float)((int)((g_state >> 16) % 3u) - 1);
}

float* block(size_t n, bool fill) {      // an exact-size heap block
  float* p = (float*)malloc(n * sizeof(float));
  if (!p) abort();
  for (size_t i = 0; i < n; ++i) p[i] = fill ? next_value() : -777.0f;
  return p;
}

int fail(const char* what) {
  fprintf(stderr, "%s: %s\n", what, dd_conv_last_error());
  return 1;
}

// direct evaluation (exact on this data): y, grad_x, grad_w
void direct(const Shape& s, const float* x, const float* w, const float* gy, std::vector<float>& y, std::vector<float>& gx, std::vector<float>& gw) {
  const int k = s.op == DD_CONV_3X3 ? 3 : s.op == DD_CONV_1X1 ? 1 : 2, st = s.op == DD_CONV_DECONV2X2 ? 2 : 1, pad = s.op == DD_CONV_3X3 ? 1 : 0;
  const int Ho = s.H * st, Wo = s.W * st;
  for (int b = 0; b < s.B; ++b)
    for (int ci = 0; ci < s.Cin; ++ci)
      for (int co = 0; co < s.Cout; ++co)
        for (int ky = 0; ky < k; ++ky)
          for (int kx = 0; kx < k; ++kx) {
            const size_t wi = s.op != DD_CONV_DECONV2X2 ? (((size_t)co * s.Cin + ci) * k + ky) * k + kx : (((size_t)ci * s.Cout + co) * 2 + ky) * 2 + kx;
            for (int iy = 0; iy < s.H; ++iy)
              for (int ix = 0; ix < s.W; ++ix) {
                // 3x3 (1x1: pad 0): output (iy', ix') reads input (iy' + ky - pad, ix' + kx - pad); transpose: input (iy, ix) writes output (2 iy + ky, 2 ix + kx)
                const int oy = s.op != DD_CONV_DECONV2X2 ? iy - ky + pad : 2 * iy + ky, ox = s.op != DD_CONV_DECONV2X2 ? ix - kx + pad : 2 * ix + kx;
                if (oy < 0 || oy >= Ho || ox < 0 || ox >= Wo) continue;
                const size_t xi = (((size_t)b * s.Cin + ci) * s.H + iy) * s.W + ix, yi = (((size_t)b * s.Cout + co) * Ho + oy) * Wo + ox;
                y[yi] += x[xi] * w[wi];
                gx[xi] += gy[yi] * w[wi];
                gw[wi] += x[xi] * gy[yi];
              }
          }
}

int run(const Shape& s, int precision) {
  const int st = s.op == DD_CONV_DECONV2X2 ? 2 : 1, taps = s.op == DD_CONV_3X3 ? 9 : s.op == DD_CONV_1X1 ? 1 : 4;
  const size_t nx = (size_t)s.B * s.Cin * s.H * s.W, ny = (size_t)s.B * s.Cout * s.H * st * s.W * st, nw = (size_t)s.Cin * s.Cout * taps;
  int64_t bytes = 0;
  if (dd_conv_workspace_bytes(s.op, s.B, s.Cin, s.Cout, s.H, s.W, precision, &bytes)) return fail("dd_conv_workspace_bytes");
  float *x = block(nx, true), *w = block(nw, true), *gy = block(ny, true), *y = block(ny, false), *gx = block(nx, false), *gw = block(nw, false);
  void* ws = malloc((size_t)bytes);
  int rc;
  if (s.op == DD_CONV_3X3) {
    rc = dd_conv3x3_forward(x, w, y, ws, s.B, s.Cin, s.Cout, s.H, s.W, precision, nullptr);
    if (!rc) rc = dd_conv3x3_backward_data(gy, w, gx, ws, s.B, s.Cin, s.Cout, s.H, s.W, precision, nullptr);
    if (!rc) rc = dd_conv3x3_backward_weight(x, gy, gw, ws, s.B, s.Cin, s.Cout, s.H, s.W, precision, nullptr);
  } else if (s.op == DD_CONV_1X1) {
    rc = dd_conv1x1_forward(x, w, y, ws, s.B, s.Cin, s.Cout, s.H, s.W, precision, nullptr);
    if (!rc) rc = dd_conv1x1_backward_data(gy, w, gx, ws, s.B, s.Cin, s.Cout, s.H, s.W, precision, nullptr);
    if (!rc) rc = dd_conv1x1_backward_weight(x, gy, gw, ws, s.B, s.Cin, s.Cout, s.H, s.W, precision, nullptr);
  } else {
    rc = dd_deconv2x2_forward(x, w, y, ws, s.B, s.Cin, s.Cout, s.H, s.W, precision, nullptr);
    if (!rc) rc = dd_deconv2x2_backward_data(gy, w, gx, ws, s.B, s.Cin, s.Cout, s.H, s.W, precision, nullptr);
    if (!rc) rc = dd_deconv2x2_backward_weight(x, gy, gw, ws, s.B, s.Cin, s.Cout, s.H, s.W, precision, nullptr);
  }
  if (rc) return fail(s.name);
  size_t wrong = 0;
  if (s.compare) {
    std::vector<float> ry(ny, 0.0f), rgx(nx, 0.0f), rgw(nw, 0.0f);
    direct(s, x, w, gy, ry, rgx, rgw);
    for (size_t i = 0; i < ny; ++i) wrong += y[i] != ry[i];
    for (size_t i = 0; i < nx; ++i) wrong += gx[i] != rgx[i];
    for (size_t i = 0; i < nw; ++i) wrong += gw[i] != rgw[i];
  }
  printf("%s precision %d: three calls done, workspace %lld bytes%s, %zu values differ\n", s.name, precision, (long long)bytes,
         s.compare ? ", compared with the direct evaluation" : "", wrong);
  fflush(stdout);
  free(x); free(w); free(gy); free(y); free(gx); free(gw); free(ws);
  return wrong ? 1 : 0;
}

}  // namespace

int main() {
  const Shape shapes[] = {{"S1", DD_CONV_3X3, 2, 64, 256, 9, 35, false}, {"S3", DD_CONV_3X3, 1, 64, 64, 3, 5, true},
                          {"S4", DD_CONV_3X3, 3, 64, 256, 40, 70, false}, {"D2", DD_CONV_DECONV2X2, 1, 64, 128, 11, 19, true},
                          {"P1", DD_CONV_1X1, 2, 64, 192, 9, 35, false},  {"P3", DD_CONV_1X1, 1, 64, 64, 1, 3, true},
                          {"P5", DD_CONV_1X1, 2, 128, 64, 4, 32, true}};
  for (const Shape& s : shapes) {
    if (run(s, DD_PREC_BF16)) return 1;
    if (s.B * s.H * s.W < 4000 && run(s, DD_PREC_F16X3)) return 1;      // (S4 in one precision: its point is the many splits)
  }
  if (dd_conv3x3_forward(nullptr, nullptr, nullptr, nullptr, 1, 216, 64, 2, 2, DD_PREC_BF16, nullptr) != DD_ERR_UNSUPPORTED) return 1;
  if (dd_conv1x1_forward(nullptr, nullptr, nullptr, nullptr, 1, 216, 64, 2, 2, DD_PREC_BF16, nullptr) != DD_ERR_UNSUPPORTED) return 1;
  printf("CONV-SANITIZE-OK\n");
  return 0;
}
