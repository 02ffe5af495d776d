// dd_api_weights.cpp -- parameter intake and packing (see dd_api_internal.h for the split of the C ABI).
#include "dd_api_internal.h"

namespace ddapi {


// 0 = denoiser (model.*), 1 = latent codec (depth_transform.*), 2 = condition FPN (conv_lateral.* / conv_up.*),
// 3 = HAHI neck in front of the FPN (hahineck.*; Swin-L pyramid only)
int weight_group(const std::string& name) {
  if (name.compare(0, 6, "model.") == 0) return 0;
  if (name.compare(0, 16, "depth_transform.") == 0) return 1;
  if (name.compare(0, 9, "hahineck.") == 0) return 3;
  return 2;
}

std::vector<WeightSpec> required_weights(int variant, int pyr) {
  std::vector<WeightSpec> v = {
      {"model.noise_embedding.0.weight", 64 * 16 * 9}, {"model.noise_embedding.0.bias", 64},
      {"model.noise_embedding.1.weight", 64}, {"model.noise_embedding.1.bias", 64},
      {"model.noise_embedding.3.weight", 256 * 64 * 9}, {"model.noise_embedding.3.bias", 256},
      {"model.noise_embedding.4.weight", 256}, {"model.noise_embedding.4.bias", 256},
      {"model.time_embedding.weight", (int64_t)EMB_ROWS * COND_C},
      {"model.pred.0.weight", 64 * 256 * 9}, {"model.pred.0.bias", 64},
      {"model.pred.1.weight", 64}, {"model.pred.1.bias", 64},
      {"model.pred.3.weight", 16 * 64 * 9}, {"model.pred.3.bias", 16},
      {"model.pred.4.weight", 16}, {"model.pred.4.bias", 16},
      {"depth_transform.conv_transform.0.0.weight", 16 * 9},
      {"depth_transform.conv_transform.0.1.weight", 16}, {"depth_transform.conv_transform.0.1.bias", 16},
      {"depth_transform.conv_transform.0.1.running_mean", 16}, {"depth_transform.conv_transform.0.1.running_var", 16},
      {"depth_transform.conv_transform.1.0.weight", 16 * 16 * 9},
      {"depth_transform.conv_transform.1.1.weight", 16}, {"depth_transform.conv_transform.1.1.bias", 16},
      {"depth_transform.conv_transform.1.1.running_mean", 16}, {"depth_transform.conv_transform.1.1.running_var", 16},
      {"depth_transform.conv_inv_transform.0.weight", 16 * 16 * 16}, {"depth_transform.conv_inv_transform.0.bias", 16},
      {"depth_transform.conv_inv_transform.1.weight", 16}, {"depth_transform.conv_inv_transform.1.bias", 16},
      {"depth_transform.conv_inv_transform.1.running_mean", 16}, {"depth_transform.conv_inv_transform.1.running_var", 16},
      {"depth_transform.conv_inv_transform.3.0.weight", 16 * 9}, {"depth_transform.conv_inv_transform.3.0.bias", 1},
  };
  if (variant == DD_VARIANT_SWIN) {
    v.push_back({"model.upsample_fuse.convA.conv.weight", 256 * 256 * 9});
    v.push_back({"model.upsample_fuse.convA.conv.bias", 256});
    v.push_back({"model.upsample_fuse.convB.conv.weight", 256 * 256 * 9});
    v.push_back({"model.upsample_fuse.convB.conv.bias", 256});
  }
  {
    // condition aggregation FPN of the Res / Swin heads (reference ...res.py:56-84): conv_lateral[i] = Conv3x3(bias=False)+BN+ReLU,
    // conv_up[j] = ConvTranspose2d(k2,s2,bias=False)+BN+ReLU
    const char* bn[4] = {"weight", "bias", "running_mean", "running_var"};
    for (int i = 0; i < FPN_LEVELS; ++i) {
      const std::string pre = "conv_lateral." + std::to_string(i);
      v.push_back({pre + ".0.weight", (int64_t)COND_C * fpn_cin(variant, pyr)[i] * 9});
      for (const char* b : bn) v.push_back({pre + ".1." + b, COND_C});
    }
    for (int j = 0; j < FPN_LEVELS - 1; ++j) {
      const std::string pre = "conv_up." + std::to_string(j);
      v.push_back({pre + ".0.weight", (int64_t)COND_C * COND_C * 4});
      for (const char* b : bn) v.push_back({pre + ".1." + b, COND_C});
    }
  }
  if (variant == DD_VARIANT_SWIN) {
    // HAHI neck (optional 4th group): ConvModule = bias-free conv + BatchNorm + ReLU
    const char* bn[4] = {"weight", "bias", "running_mean", "running_var"};
    for (const NeckConv& c : neck_convs(pyr)) {
      v.push_back({c.name + ".conv.weight", (int64_t)c.cout * c.cin * c.ks * c.ks});
      for (const char* b : bn) v.push_back({c.name + ".bn." + b, c.cout});
    }
  }
  return v;
}

}  // namespace ddapi

extern "C" {

int dd_set_weight(dd_handle_t h, const char* name, const float* data, int64_t numel) {
  if (!h) return DD_ERR_INVALID_ARG;
  if (!name || !data || numel <= 0) return h->fail(DD_ERR_INVALID_ARG, "dd_set_weight: null name/data or non-positive numel");
  if (h->variant == DD_VARIANT_SWIN) {
    // the Swin-L and the MPViT-small heads share this variant's denoiser; which pyramid the FPN has shows in the lateral weights
    const std::string nm(name);
    for (int i = 0; i < FPN_LEVELS; ++i)
      if (nm == "conv_lateral." + std::to_string(i) + ".0.weight") {
        const int pyr = numel == (int64_t)COND_C * FPN_CIN_MPVIT[i] * 9 ? PYR_MPVIT : PYR_DEFAULT;
        if (pyr != h->fpn_pyramid) {
          for (int j = 0; j < FPN_LEVELS; ++j) h->host_w.erase("conv_lateral." + std::to_string(j) + ".0.weight");   // other pyramid's
          for (const NeckConv& c : neck_convs(h->fpn_pyramid)) h->host_w.erase(c.name + ".conv.weight");
          h->fpn_pyramid = pyr;
          h->fpn_committed = false;
          h->neck_committed = false;
        }
      }
    // ... or in the neck's first lateral convolution, whichever arrives first (the heads register the neck in front of the FPN)
    if (nm == "hahineck.lateral_convs.0.conv.weight") {
      const int pyr = numel == (int64_t)NECK_C_MPVIT[0] * NECK_C_MPVIT[0] ? PYR_MPVIT : PYR_DEFAULT;
      if (pyr != h->fpn_pyramid) {
        for (int j = 0; j < FPN_LEVELS; ++j) h->host_w.erase("conv_lateral." + std::to_string(j) + ".0.weight");
        for (const NeckConv& c : neck_convs(h->fpn_pyramid)) h->host_w.erase(c.name + ".conv.weight");
        h->fpn_pyramid = pyr;
        h->fpn_committed = false;
        h->neck_committed = false;
      }
    }
  }
  for (const auto& ws : required_weights(h->variant, h->fpn_pyramid)) {
    if (ws.name == name) {
      if (ws.numel != numel)
        return h->fail(DD_ERR_INVALID_ARG, std::string("dd_set_weight: ") + name + " expects " + std::to_string(ws.numel) +
                                               " elements, got " + std::to_string(numel));
      h->host_w[name].assign(data, data + numel);
      h->dev_newer.erase(name);
      h->weights_serial++;
      const int grp = weight_group(name);
      if (grp == 0) h->committed = false; else if (grp == 1) h->codec_committed = false; else if (grp == 3) h->neck_committed = false; else h->fpn_committed = false;
      return DD_OK;
    }
  }
  return h->fail(DD_ERR_INVALID_ARG, std::string("dd_set_weight: unknown parameter name '") + name + "'");
}

int dd_set_weight_device(dd_handle_t h, const char* name, const float* data, int64_t numel, void* stream) {
  if (!h) return DD_ERR_INVALID_ARG;
  if (!name || !data || numel <= 0) return h->fail(DD_ERR_INVALID_ARG, "dd_set_weight_device: null name/data or non-positive numel");
  if (weight_group(name) != 0)
    return h->fail(DD_ERR_UNSUPPORTED, std::string("dd_set_weight_device: '") + name + "' is not a denoiser parameter (model.*): the codec and "
                                       "FPN groups are folded on the host, use dd_set_weight");
  for (const auto& ws : required_weights(h->variant, h->fpn_pyramid)) {
    if (ws.name != name) continue;
    if (ws.numel != numel)
      return h->fail(DD_ERR_INVALID_ARG, std::string("dd_set_weight_device: ") + name + " expects " + std::to_string(ws.numel) +
                                             " elements, got " + std::to_string(numel));
    DD_HIP(hipSetDevice(h->device));
    std::unique_ptr<DevBuf>& b = h->dev_w[name];
    if (!b) b.reset(new DevBuf());
    if (b->bytes != (size_t)numel * 4) DD_HIP(b->alloc((size_t)numel * 4));
    DD_HIP(hipMemcpyAsync(b->p, data, (size_t)numel * 4, hipMemcpyDeviceToDevice, reinterpret_cast<hipStream_t>(stream)));
    h->dev_newer.insert(name);
    h->committed = false;
    h->weights_serial++;
    return DD_OK;
  }
  return h->fail(DD_ERR_INVALID_ARG, std::string("dd_set_weight_device: unknown parameter name '") + name + "'");
}
}  // extern "C"
namespace ddapi {

// The packed-image geometry of kernel (kid, ek).  A pair no kernel runs (conv_pack_geom2's all-zero answer: a mistyped id, a kind the form does
// not exist in) fails the call here -- it must not travel on as a zero-sized image.
int pack_geom(dd_handle_t h, int kid, int ek, PackGeom* g) {
  *g = conv_pack_geom2(kid, ek);
  if (g->cout == 0) return h->fail(DD_ERR_INVALID_ARG, "no fused convolution kernel, hence no packed weight image, for kernel id " + std::to_string(kid) + " in element kind " + std::to_string(ek));
  return DD_OK;
}

// `dst` holds at least `bytes` (a buffer that is large enough keeps its address: graphs hold it); with `src`, it is filled from that host array
// on stream `s` -- asynchronously: the array stays untouched until the stream has been synchronised (dd_commit_weights does, once, at its end)
int device_buf(dd_handle_t h, DevBuf& dst, size_t bytes, const void* src, hipStream_t s) {
  if (dst.bytes < bytes || !dst.p) DD_HIP(dst.alloc(bytes));
  if (src) DD_HIP(hipMemcpyAsync(dst.p, src, bytes, hipMemcpyHostToDevice, s));
  return DD_OK;
}

// One device fp32 tensor W[cout][cin][ks][ks] of `numel` elements into the weight images of kernel `kid`: image slot slots[i] (element kind
// wimg_kind) into images[slots[i]], by pack_weights_kernel (dd_misc.hip) -- the one place that knows the layout
//   [n_tile][cin_chunk][tap_group][tap_in_group][n (NT)][k (CK)], zero beyond cout, 16-byte pieces swizzled for the LDS-DMA,
// the 16-bit roundings, the split-f16 pair and conv4's stacked lo halves.  transposed: the images of the data-gradient convolution of W.
// The kernel indexes the tensor by the geometry of (kid, kind): a tensor of another size fails the call before anything is read.
int pack_images(dd_handle_t h, const float* w, int64_t numel, int kid, const int* slots, int n_slots, DevBuf* images, bool transposed, hipStream_t s) {
  for (int i = 0; i < n_slots; ++i) {
    const int ek = wimg_kind(slots[i]);
    PackGeom g;
    DD_TRY(pack_geom(h, kid, ek, &g));
    if (numel != (int64_t)g.cout * g.cin * g.ks * g.ks)
      return h->fail(DD_ERR_INVALID_ARG, "weight image of kernel id " + std::to_string(kid) + " in element kind " + std::to_string(ek) + " packs " +
                                             std::to_string((int64_t)g.cout * g.cin * g.ks * g.ks) + " weights, the tensor has " + std::to_string(numel));
    DD_TRY(device_buf(h, images[slots[i]], pack_weights_bytes(g, ek)));
    DD_HIP(launch_pack_weights(w, images[slots[i]].p, g, ek, true, transposed, s));
  }
  return DD_OK;
}

namespace {

// eval-mode BatchNorm `pre` (.weight / .bias / .running_mean / .running_var) of C channels as y = x * scale + shift.  The scale stays in double:
// it multiplies the convolution's weights in double (FPN, neck); the codec rounds it to float first.
void bn_fold(dd_handle_t h, const std::string& pre, int C, std::vector<double>& scale, std::vector<float>& shift) {
  const auto &g = h->host_w[pre + ".weight"], &b = h->host_w[pre + ".bias"], &m = h->host_w[pre + ".running_mean"], &v = h->host_w[pre + ".running_var"];
  scale.resize(C); shift.resize(C);
  for (int c = 0; c < C; ++c) {
    scale[c] = (double)g[c] / std::sqrt((double)v[c] + (double)BN_EPS);
    shift[c] = (float)((double)b[c] - (double)m[c] * scale[c]);
  }
}

// What one dd_commit_weights call shares between its groups: the stream, the host arrays its asynchronous uploads read (alive until the call
// has synchronised the stream) and, per packed group, the device word that collects max |w| of the tensors that were packed.
struct Commit {
  dd_handle_t h;
  hipStream_t s;
  std::list<std::vector<float>> held;
  enum { FIT_MODEL, FIT_FPN, FIT_NECK, N_FIT };
};

// `v` into `dst` on the call's stream; the call keeps the array until it has synchronised
int upload_held(Commit& c, DevBuf& dst, std::vector<float>&& v) {
  c.held.push_back(std::move(v));
  return device_buf(c.h, dst, c.held.back().size() * 4, c.held.back().data(), c.s);
}

// A folded (BatchNorm-scaled, channel-padded) fp32 tensor: through the handle's staging buffer into the images fp32 / bf16 / f16 / split f16 of
// kernel `kid`, its magnitude into the group's max-|w| word.  Stream order keeps the next tensor's upload behind this one's pack kernels.
int pack_folded(Commit& c, std::vector<float>&& w, int kid, DevBuf* images, int fit) {
  dd_handle_t h = c.h;
  const int64_t numel = (int64_t)w.size();
  DD_TRY(upload_held(c, h->stage, std::move(w)));
  DD_HIP(launch_max_abs(h->stage.as<float>(), numel, h->wmax.as<unsigned>() + fit, c.s));
  return pack_images(h, h->stage.as<float>(), numel, kid, kImageSlots, 4, images, false, c.s);
}

// One convolution of the denoiser from its fp32 device tensor into every layout the forward / backward kernels read
int pack_conv_layer(Commit& c, ConvLayer& L, const float* w, int fwd_layer, int dgrad_layer, bool with_naive) {
  dd_handle_t h = c.h;
  const int64_t numel = (int64_t)L.cout * L.cin * 9;
  int fwd[NUM_WIMG], n_fwd = 0;
  for (int wi = 0; wi < NUM_WIMG; ++wi)
    if (wimg_has(wi, fwd_layer)) fwd[n_fwd++] = wi;
  DD_TRY(pack_images(h, w, numel, fwd_layer, fwd, n_fwd, L.wpack2, false, c.s));
  DD_TRY(pack_images(h, w, numel, dgrad_layer, kImageSlots, NUM_EK, L.wpackT, true, c.s));      // (the split / refined f16 modes are forward only)
  DD_HIP(launch_max_abs(w, numel, h->wmax.as<unsigned>() + Commit::FIT_MODEL, c.s));
  DD_TRY(device_buf(h, L.w_oihw, (size_t)numel * 4));        // fp32 OIHW: the naive path, the E[t] tables, the hoisted Swin form's composition
  DD_HIP(hipMemcpyAsync(L.w_oihw.p, w, (size_t)numel * 4, hipMemcpyDeviceToDevice, c.s));
  if (with_naive) {
    DD_TRY(device_buf(h, L.wT_oihw, (size_t)numel * 4));
    DD_HIP(launch_transpose_flip(w, L.wT_oihw.as<float>(), L.cout, L.cin, 9, c.s));
  }
  return DD_OK;
}

// ---- denoiser (model.*): the newest value of every parameter, whichever call delivered it, as an fp32 device tensor; from there the pack kernels ----
int commit_model(Commit& c) {
  dd_handle_t h = c.h;
  hipStream_t s = c.s;
  for (const auto& ws : required_weights(h->variant, h->fpn_pyramid)) {
    if (weight_group(ws.name) != 0 || h->dev_newer.count(ws.name)) continue;
    std::unique_ptr<DevBuf>& b = h->dev_w[ws.name];
    if (!b) b.reset(new DevBuf());
    if (b->bytes != (size_t)ws.numel * 4) DD_HIP(b->alloc((size_t)ws.numel * 4));
    DD_HIP(hipMemcpyAsync(b->p, h->host_w[ws.name].data(), (size_t)ws.numel * 4, hipMemcpyHostToDevice, s));     // (host_w outlives the call)
    h->dev_newer.insert(ws.name);
  }
  auto D = [&](const std::string& n) { return h->dev_w[n]->as<float>(); };
  auto copy_small = [&](DevBuf& dst, const std::string& n, size_t pad_elems) -> int {
    const DevBuf& src = *h->dev_w[n];
    const size_t bytes = std::max(src.bytes, pad_elems * 4);
    DD_TRY(device_buf(h, dst, bytes));
    if (bytes > src.bytes) DD_HIP(hipMemsetAsync(dst.p, 0, bytes, s));
    DD_HIP(hipMemcpyAsync(dst.p, src.p, src.bytes, hipMemcpyDeviceToDevice, s));
    return DD_OK;
  };
  for (int l = 0; l < 4; ++l) {
    ConvLayer& L = h->L[l];
    L.cin = kCins[l]; L.cout = kCouts[l];
    DD_TRY(pack_conv_layer(c, L, D(std::string(kConvNames[l]) + ".weight"), kid_denoiser(l), kid_dgrad(l), true));
    DD_TRY(copy_small(L.bias, std::string(kConvNames[l]) + ".bias", 32));
    DD_TRY(copy_small(L.gamma, std::string(kGnNames[l]) + ".weight", 0));
    DD_TRY(copy_small(L.beta, std::string(kGnNames[l]) + ".bias", 0));
  }
  if (h->variant == DD_VARIANT_SWIN) {
    const char* names[2] = {"model.upsample_fuse.convA.conv", "model.upsample_fuse.convB.conv"};
    ConvLayer* Ls[2] = {&h->LA, &h->LB};
    for (int i = 0; i < 2; ++i) {
      ConvLayer& L = *Ls[i];
      L.cin = COND_C; L.cout = COND_C;
      // backward: the data gradient of a 256 -> 256 convolution = the convB kernel (raw input, no norm) on W^T flipped
      DD_TRY(pack_conv_layer(c, L, D(std::string(names[i]) + ".weight"), kid_swin_fuse(i), KID_SWIN_CONVB, false));
      DD_TRY(copy_small(L.bias, std::string(names[i]) + ".bias", 0));
    }
  }
  DD_TRY(copy_small(h->emb, "model.time_embedding.weight", 0));
  if (h->etab.bytes == 0) {
    DD_HIP(h->etab.alloc((size_t)EMB_ROWS * 10 * HID_C * 4));
    DD_HIP(h->zero_bias.alloc(COND_C * 4));
    DD_HIP(hipMemsetAsync(h->zero_bias.p, 0, COND_C * 4, s));
  }
  DD_HIP(launch_etab(h->L[2].w_oihw.as<float>(), h->emb.as<float>(), h->etab.as<float>(), s));
  return DD_OK;
}

// ---- condition FPN: eval-mode BatchNorm folded into the (bias-free) convolutions on the host, packed for the fused kernels on the device ----
int commit_fpn(Commit& c) {
  dd_handle_t h = c.h;
  const int* cin = fpn_cin(h->variant, h->fpn_pyramid);
  const int* cin_pad = fpn_cin_pad(h->variant, h->fpn_pyramid);      // zero weights for the padding channels
  std::vector<double> sc; std::vector<float> sh;
  for (int i = 0; i < FPN_LEVELS; ++i) {
    const std::string pre = "conv_lateral." + std::to_string(i);
    bn_fold(h, pre + ".1", COND_C, sc, sh);
    const std::vector<float>& w0 = h->host_w[pre + ".0.weight"];    // [256][cin][3][3]
    const size_t per = (size_t)cin[i] * 9, per_pad = (size_t)cin_pad[i] * 9;
    std::vector<float> w((size_t)COND_C * per_pad, 0.f);
    for (int co = 0; co < COND_C; ++co)
      for (size_t k = 0; k < per; ++k) w[co * per_pad + k] = (float)((double)w0[co * per + k] * sc[co]);
    DD_TRY(pack_folded(c, std::move(w), kid_fpn_lateral(pyramid_of(h->variant, h->fpn_pyramid), i), h->fpn_lat_w[i], Commit::FIT_FPN));
    DD_TRY(upload_held(c, h->fpn_lat_b[i], std::move(sh)));
  }
  for (int j = 0; j < FPN_LEVELS - 1; ++j) {
    const std::string pre = "conv_up." + std::to_string(j);
    bn_fold(h, pre + ".1", COND_C, sc, sh);
    const std::vector<float>& wt = h->host_w[pre + ".0.weight"];     // ConvTranspose2d weight [cin][cout][2][2]
    // as a 1x1 convolution with 4 x 256 outputs: row (dy*2+dx)*256 + co, column ci
    std::vector<float> w((size_t)4 * COND_C * COND_C), b4((size_t)4 * COND_C);
    for (int par = 0; par < 4; ++par)
      for (int co = 0; co < COND_C; ++co) {
        b4[par * COND_C + co] = sh[co];
        for (int ci = 0; ci < COND_C; ++ci)
          w[((size_t)par * COND_C + co) * COND_C + ci] = (float)((double)wt[((size_t)ci * COND_C + co) * 4 + par] * sc[co]);
      }
    DD_TRY(pack_folded(c, std::move(w), KID_FPN_UP, h->fpn_up_w[j], Commit::FIT_FPN));
    DD_TRY(upload_held(c, h->fpn_up_b[j], std::move(b4)));
  }
  return DD_OK;
}

// ---- HAHI neck: eval-mode BatchNorm folded into the bias-free convolutions (scale into the weights, shift = bias) ----
// The kernels' channel counts can exceed the reference's (MPViT level 1: 216 carried as 224): the folded weights are laid into
// [cout_k][cin_k] with zeros in the padding; a fusion convolution reads the concatenation [lateral (Ck) | projection (512)] (level 0:
// [projection | lateral]), so its reference input channel ci >= C of the lateral part's successor moves up by Ck - C.
int commit_neck(Commit& c) {
  dd_handle_t h = c.h;
  std::vector<double> sc; std::vector<float> sh;
  for (const NeckConv& nc : neck_convs(h->fpn_pyramid)) {
    bn_fold(h, nc.name + ".bn", nc.cout, sc, sh);
    const std::vector<float>& w0 = h->host_w[nc.name + ".conv.weight"];
    PackGeom pg;
    DD_TRY(pack_geom(h, nc.layer, EK_F32, &pg));
    const int kk = nc.ks * nc.ks, cin_k = pg.cin, cout_k = pg.cout;
    std::vector<float> w((size_t)cout_k * cin_k * kk, 0.f);
    sh.resize((size_t)pg.cout_pad, 0.f);
    for (int co = 0; co < nc.cout; ++co)
      for (int ci = 0; ci < nc.cin; ++ci) {
        int cik = ci;
        if (nc.kind == NECK_FUSION && nc.level > 0 && ci >= nc.C) cik = ci - nc.C + nc.Ck;          // [lateral | projection]: the projection part starts at Ck
        for (int k = 0; k < kk; ++k)
          w[((size_t)co * cin_k + cik) * kk + k] = (float)((double)w0[((size_t)co * nc.cin + ci) * kk + k] * sc[co]);
      }
    const int slot = 4 * nc.kind + nc.level;
    DD_TRY(pack_folded(c, std::move(w), nc.layer, h->neck_w[slot], Commit::FIT_NECK));
    DD_TRY(upload_held(c, h->neck_b[slot], std::move(sh)));
  }
  return DD_OK;
}

// ---- codec: eval-mode BatchNorm folded into the convolutions (reference depth_transform.py:15-26), all in one allocation ----
int commit_codec(Commit& c) {
  dd_handle_t h = c.h;
  auto W = [&](const char* n) -> const std::vector<float>& { return h->host_w[n]; };
  std::vector<float> blob;
  auto push = [&](const std::vector<float>& v) { size_t off = blob.size(); blob.insert(blob.end(), v.begin(), v.end());
                                                 while (blob.size() % 4) blob.push_back(0.f); return off; };
  std::vector<double> scd; std::vector<float> sc, sh;
  auto fold = [&](const char* pre) { bn_fold(h, pre, 16, scd, sh); sc.assign(16, 0.f); for (int ch = 0; ch < 16; ++ch) sc[ch] = (float)scd[ch]; };      // the codec scales in float
  fold("depth_transform.conv_transform.0.1");
  std::vector<float> e0 = W("depth_transform.conv_transform.0.0.weight");
  for (int ch = 0; ch < 16; ++ch) for (int k = 0; k < 9; ++k) e0[ch * 9 + k] *= sc[ch];
  const size_t o_e0 = push(e0), o_eb0 = push(sh);
  fold("depth_transform.conv_transform.1.1");
  std::vector<float> e1 = W("depth_transform.conv_transform.1.0.weight");
  for (int co = 0; co < 16; ++co) for (int k = 0; k < 16 * 9; ++k) e1[co * 144 + k] *= sc[co];
  const size_t o_e1 = push(e1), o_eb1 = push(sh);
  std::vector<float> e1t(2304);          // the same weights tap-major [tap][ci][co] for enc1_kernel
  for (int co = 0; co < 16; ++co) for (int ci = 0; ci < 16; ++ci) for (int k = 0; k < 9; ++k) e1t[(k * 16 + ci) * 16 + co] = e1[(co * 16 + ci) * 9 + k];
  const size_t o_e1t = push(e1t);
  fold("depth_transform.conv_inv_transform.1");
  std::vector<float> d0 = W("depth_transform.conv_inv_transform.0.weight");       // (in, out, 4, 4)
  for (int ci = 0; ci < 16; ++ci) for (int co = 0; co < 16; ++co) for (int k = 0; k < 16; ++k) d0[(ci * 16 + co) * 16 + k] *= sc[co];
  std::vector<float> db0(16);
  { const auto& cb = W("depth_transform.conv_inv_transform.0.bias"); for (int ch = 0; ch < 16; ++ch) db0[ch] = cb[ch] * sc[ch] + sh[ch]; }
  const size_t o_d0 = push(d0), o_db0 = push(db0);
  // the same weights tap-major [ky][kx][ci][co] for the fused decoder kernel (a wave reads one (tap, ci) row of 16 couts uniformly)
  std::vector<float> d0t(4096);
  for (int ci = 0; ci < 16; ++ci) for (int co = 0; co < 16; ++co) for (int k = 0; k < 16; ++k) d0t[(k * 16 + ci) * 16 + co] = d0[(ci * 16 + co) * 16 + k];
  const size_t o_d0t = push(d0t);
  const size_t o_d1 = push(W("depth_transform.conv_inv_transform.3.0.weight"));
  DD_TRY(upload_held(c, h->codec_buf, std::move(blob)));
  const float* base = h->codec_buf.as<float>();
  h->codec.enc_w0 = base + o_e0; h->codec.enc_b0 = base + o_eb0;
  h->codec.enc_w1 = base + o_e1; h->codec.enc_b1 = base + o_eb1; h->codec.enc_w1t = base + o_e1t;
  h->codec.dec_w0 = base + o_d0; h->codec.dec_b0 = base + o_db0; h->codec.dec_w0t = base + o_d0t;
  h->codec.dec_w1 = base + o_d1;
  h->codec.dec_b1 = W("depth_transform.conv_inv_transform.3.0.bias")[0];
  return DD_OK;
}

}  // namespace
}  // namespace ddapi

extern "C" {

int dd_commit_weights(dd_handle_t h, void* stream) {
  if (!h) return DD_ERR_INVALID_ARG;
  DD_HIP(hipSetDevice(h->device));
  // independent groups: "model." (denoiser), "depth_transform." (codec), "conv_lateral." / "conv_up." (condition FPN) and "hahineck." (neck).
  // A group is packed when all of its keys are present; a partially provided group is an error; at least one must be complete.
  int have[4] = {0, 0, 0, 0}, need[4] = {0, 0, 0, 0};
  std::string first_missing[4];
  for (const auto& ws : required_weights(h->variant, h->fpn_pyramid)) {
    const int grp = weight_group(ws.name);
    need[grp]++;
    if (h->host_w.count(ws.name) || h->dev_newer.count(ws.name)) have[grp]++;
    else if (first_missing[grp].empty()) first_missing[grp] = ws.name;
  }
  for (int grp = 0; grp < 4; ++grp)
    if (have[grp] != 0 && have[grp] != need[grp])
      return h->fail(DD_ERR_STATE, "dd_commit_weights: missing parameter '" + first_missing[grp] + "'");
  if (have[0] == 0 && have[1] == 0 && have[2] == 0 && have[3] == 0) return h->fail(DD_ERR_STATE, "dd_commit_weights: no parameters were set");
  // only the groups that changed since their last commit (dd_set_weight / dd_set_weight_device clear the group's flag)
  const bool do_model = have[0] == need[0] && !h->committed, do_codec = have[1] == need[1] && !h->codec_committed;
  const bool do_fpn = need[2] > 0 && have[2] == need[2] && !h->fpn_committed, do_neck = need[3] > 0 && have[3] == need[3] && !h->neck_committed;
  if (!do_model && !do_codec && !do_fpn && !do_neck) return DD_OK;
  // graphs bake weight pointers; buffers are reused when sizes match, so existing graphs stay valid,
  // but make sure nothing is in flight while we overwrite them.
  DD_HIP(hipDeviceSynchronize());
  Commit c{h, reinterpret_cast<hipStream_t>(stream), {}};
  if (!h->wmax.p) DD_HIP(h->wmax.alloc(Commit::N_FIT * sizeof(unsigned)));
  DD_HIP(hipMemsetAsync(h->wmax.p, 0, Commit::N_FIT * sizeof(unsigned), c.s));
  int rc = DD_OK;
  if (rc == DD_OK && do_model) rc = commit_model(c);
  if (rc == DD_OK && do_fpn) rc = commit_fpn(c);
  if (rc == DD_OK && do_neck) rc = commit_neck(c);
  if (rc == DD_OK && do_codec) rc = commit_codec(c);
  // one read-back and one synchronisation for the whole call: the images are in place when it returns, whatever stream runs next, and the
  // host arrays the uploads read (c.held) may go -- also when a group failed half way
  unsigned wbits[Commit::N_FIT] = {0, 0, 0};
  hipError_t e = hipMemcpyAsync(wbits, h->wmax.p, sizeof(wbits), hipMemcpyDeviceToHost, c.s);
  const hipError_t e_sync = hipStreamSynchronize(c.s);
  h->stage.release();
  if (rc != DD_OK) return rc;
  if (e == hipSuccess) e = e_sync;
  if (e != hipSuccess) return h->fail(DD_ERR_HIP, std::string("dd_commit_weights: ") + hipGetErrorString(e));
  // do the packed tensors fit the split-f16 images?  |w| x SPLIT_WSCALE must stay inside f16 (|w| < 234; a NaN does not fit).  The denoiser's split
  // modes (DD_PREC_F16X3 / DD_PREC_F16R) refuse to run on parameters that do not (check_split); the pyramid then keeps the fp32-operand kernels.
  // conv4's stacked image asks less (|w| inside f16).
  auto fits = [&](int grp) { float m; std::memcpy(&m, &wbits[grp], 4); return m * SPLIT_WSCALE < 60000.f; };
  if (do_model) { h->split_ok = fits(Commit::FIT_MODEL); h->committed = true; }
  if (do_fpn) { h->fpn_split_ok = fits(Commit::FIT_FPN); h->fpn_committed = true; }
  if (do_neck) { h->neck_split_ok = fits(Commit::FIT_NECK); h->neck_committed = true; }
  if (do_codec) h->codec_committed = true;
  return DD_OK;
}
}  // extern "C"
