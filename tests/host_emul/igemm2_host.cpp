// tests/host_emul/igemm2_host.cpp -- TEST INFRASTRUCTURE: a small C interface (ctypes, tests/test_igemm2_host_emulation.py) to the launchers of the
// production convolution kernels (diffusiondepth_amd/csrc/dd_igemm2.hip) inside the host-emulated library (ddepth_host.cpp).  The
// kernels have hundreds of green GPU parity tests; what the GPU cannot show is that they are free of RACES that the hardware's timing happens
// not to trigger: here a wave runs ahead as far as the workgroup barriers allow, and an LDS-DMA lands either at issue or as late as the
// s_waitcnt arithmetic permits (dd_gcn.h) -- the results must not depend on any of it.
#include "dd_api_internal.h"

extern "C" {

// cin, cout, cout_pad, ck, tg, nt, th, ks, planes, stack of (layer, element kind): the packed-weight geometry the host side packs with (all zero: no
// kernel runs the pair)
void emu_geom2(int layer, int ek, int* out10) {
  const dd::PackGeom g = dd::conv_pack_geom2(layer, ek);
  out10[0] = g.cin; out10[1] = g.cout; out10[2] = g.cout_pad; out10[3] = g.ck; out10[4] = g.tg; out10[5] = g.nt; out10[6] = g.th; out10[7] = g.ks;
  out10[8] = g.planes; out10[9] = g.stack;
}

int emu_conv2(int layer, int ek, const void* in, const void* wpack, const float* bias, void* out, double* stats_out, const double* stats_in,
              const float* gn_gamma, const float* gn_beta, const void* cond, const float* emb, const long long* tvec, int t_base, int t_bstride,
              const float* y4, float* xout, const float* c1c2, int step, int B, int h, int w, const float* cadd, const float* etab,
              const void* addend) {
  dd::ConvParams p{};
  p.in = in; p.wpack = wpack; p.bias = bias; p.out = out; p.stats_out = stats_out; p.stats_in = stats_in; p.gn_gamma = gn_gamma;
  p.gn_beta = gn_beta; p.cond = cond; p.emb = emb; p.tvec = tvec; p.t_base = t_base; p.t_bstride = t_bstride; p.y4 = y4; p.xout = xout;
  p.c1c2 = c1c2; p.step = step; p.B = B; p.h = h; p.w = w; p.cadd = cadd; p.etab = etab; p.addend = addend;
  const dd::PackGeom g = dd::conv_pack_geom2(layer, ek);
  if (g.th == 0) return (int)hipErrorInvalidValue;      // (the launcher would answer the same)
  p.tiles_x = (w + 31) / 32;
  p.tiles_y = (h + g.th - 1) / g.th;
  return dd::launch_conv_igemm2(layer, ek, p, nullptr);
}

// fp32 W[cout][cin][ks][ks] (transposed: the tensor whose data-gradient convolution is packed) into the swizzled weight image of (layer, element
// kind) by the library's pack kernel; dst holds pack_weights_bytes of that pair
int emu_pack(int layer, int ek, const float* src, void* dst, int transposed) {
  const dd::PackGeom g = dd::conv_pack_geom2(layer, ek);
  if (g.cout == 0) return (int)hipErrorInvalidValue;
  return (int)dd::launch_pack_weights(src, dst, g, ek, true, transposed != 0, nullptr);
}

// The library's own way to a weight image (ddapi::pack_images: every group of dd_commit_weights and the hoisted Swin form go through it) for a
// tensor of `numel` elements: the status code of the call; on success the image of slot `slot` is copied to `out` (out_bytes = its size, else -1)
int emu_pack_images(dd_handle_t h, const float* w, long long numel, int layer, int slot, void* out, long long out_bytes) {
  DevBuf images[NUM_WIMG];
  const int rc = pack_images(h, w, numel, layer, &slot, 1, images, false, nullptr);
  if (rc != DD_OK) return rc;
  if ((long long)images[slot].bytes != out_bytes) return -1;
  std::memcpy(out, images[slot].p, (size_t)out_bytes);
  return DD_OK;
}

}  // extern "C"
