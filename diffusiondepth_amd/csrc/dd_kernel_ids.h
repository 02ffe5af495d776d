// dd_kernel_ids.h -- the kernel ids ("kernel layer ids") of the fused convolutions (dd_igemm2.hip): every id's name, what it computes,
// the classifiers the tiling (Cfg2, dd_igemm2_cfg.h) and the host (dd_api_*.cpp) derive its shape from, and the ONE rule that says which
// instantiation Cfg2<kind, id> runs a requested (id, kind) -- launch_conv_igemm2 and conv_pack_geom2 are generated from the list and that rule.
// The NUMBERS are public and fixed: callers pass them to dd_get_layer_ms / option "phase_prof_layer" (include/ddepth.h), the tests' harness passes
// them, and they appear in the mangled kernel names (conv_igemm2_kernel<Cfg2<kind, id>>: ...Cfg2ILi5ELi49EE...) that the tools and the kernel-stats
// files under profiles/ quote.  A new kernel form takes a free number, a line in DD_KERNEL_IDS and, if a mode treats it specially, a line in kid_route.
#pragma once
#include "dd_kernels.h"

namespace dd {

// ---- the denoiser -----------------------------------------------------------------------------------------------------------------
// 1..4: conv1..conv4 of the Res denoiser.  Swin/MPViT variant (reference ...swin_addHAHI.py:321-382):
//   5 = upsample_fuse.convA 256->256 (prologue relu(gn2(y2)) + up(cond) + E[t]), 6 = upsample_fuse.convB 256->256
//   (raw input, no norm / activation in between: ConvModule(norm_cfg=None, act_cfg=None)), 7 = pred.0 256->64 on a raw input
// Res denoiser with the condition term hoisted (optional): 8 = conv3 applied ONCE per image to the raw condition map (fp32
//   out, no bias / statistics), 9 = conv3 on relu(gn2(y2)) only, epilogue adds layer 8's output and the E[t] tap sums
constexpr int KID_CONV1 = 1, KID_CONV2 = 2, KID_CONV3 = 3, KID_CONV4 = 4;
constexpr int KID_SWIN_CONVA = 5, KID_SWIN_CONVB = 6, KID_SWIN_PRED = 7;
constexpr int KID_CONV3C = 8, KID_CONV3H = 9;
// ---- condition aggregation (FPN of the Res head, reference ...res.py:56-84,108-118; eval-mode BN folded into weights / bias) ---------------
//   10..13 = conv_lateral[0..3]: Conv3x3 (64|128|256|512 -> 256) + BN + ReLU, then "+ top-down term" (optional addend)
//   14     = conv_up[j]: ConvTranspose2d(256->256, k2, s2) + BN + ReLU written as a 1x1 conv with 4 x 256 output
//            "channels" (one block per output parity (dy,dx)) whose epilogue scatters to pixel (2y+dy, 2x+dx)
//   15..18 = the same lateral convs for the Swin-L pyramid (192|384|768|1536 -> 256; reference ...res_swin_add.py:31,57-84)
//   24..26 = lateral convs of the MPViT-small pyramid (reference ...res_mpvit_HAHI.py:32: 128 | 216 | 288 | 288 -> 256; 216 is carried
//            as 224 = 7 blocks of 32 with zero channels / zero weights; levels 2 and 3 share layer 26)
enum Pyramid : int { PYRAMID_RES = 0, PYRAMID_SWIN = 1, PYRAMID_MPVIT = 2 };
constexpr int FPN_LEVELS = 4;
constexpr int KID_FPN_LAT_RES = 10, KID_FPN_UP = 14, KID_FPN_LAT_SWIN = 15, KID_FPN_LAT_MPVIT = 24;
// ---- backward: 20..23 = data gradients of conv4, conv3, conv2, conv1 -- the same implicit GEMM with
//   W'[ci][co][ky][kx] = W[co][ci][2-ky][2-kx] on the raw GroupNorm-backward result: 16->64, 64->256, 256->64, 64->16
constexpr int KID_DGRAD4 = 20, KID_DGRAD3 = 21, KID_DGRAD2 = 22, KID_DGRAD1 = 23;
// ---- HAHI neck of the Swin-L heads with the attention off (reference src/model/necks/hahi.py:60-97,170-173,196-197,226-272; eval-mode BN
// folded): per pyramid level i (C_i = 192 << i, embedding 512), id = base + 4 * kind + level:
//   30 + i = lateral_convs[i]: 1x1 C_i -> C_i        34 + i = conv_proj / trans_proj[i-1]: 1x1 C_i -> 512
//   38 + i = conv_fusion / trans_fusion[i-1]: 3x3 (C_i + 512) -> C_i on the channel concatenation
// all + ReLU, raw inputs.  The concatenation is free in the channel-blocked layout: the two 1x1 convs write their couts at a channel
// offset of ONE buffer (ConvParams::out_coff / out_cstride), the projection reads the lateral result from it (in_coff / in_cstride).
//   54..65 = the same twelve convolutions for the MPViT-small pyramid (reference ...res_mpvit_HAHI.py:32,51-53: 128 | 216 | 288 | 288,
//   embedding 512): 216 is carried as 224 channels (zero channels / zero weights, as in dd_condition), couts round up to whole 64-cout
//   workgroup tiles (224 -> 256, 288 -> 320: the padding couts are computed on zero weights and never stored)
constexpr int KID_NECK_SWIN = 30, KID_NECK_MPVIT = 54;
constexpr int NECK_CONVS = 12, NECK_EMBED_C = 512;
enum NeckKind : int { NECK_LATERAL = 0, NECK_PROJ = 1, NECK_FUSION = 2 };
// ---- special tile / hoisted forms of the layers above (46..53) ------------------------------------------------------------------------
// Kernel ids of the BIG-TILE forms of the hoisted conv3 pair: layer 8 (conv3(cond), once per image) and layer 9 (conv3 in
// the loop) on 16x32-pixel tiles -- four waves of 128 pixels x 64 couts each, 0.75 instead of 1.0 LDS fragment reads per MFMA, half the
// weight stream per pixel -- chosen per launch when there are more 8x32 tiles than resident workgroup slots (the two must agree: layer 8
// leaves its result in the accumulator-fragment order of layer 9's tiles).  Same packed weights as layers 8 / 9.
constexpr int BIG_CONV3C = 48, BIG_CONV3H = 49;
// layer 9 on its 8x32 tiles with ONE patch buffer (dd_igemm2_cfg.h, ONEBUF): the next chunk's patch goes into the buffer the MFMAs just read, behind a
// second workgroup barrier per stage; 52 KB of LDS = three workgroups per CU.  Same tiles, packed weights and accumulator-fragment order as layer 9.
constexpr int ONE_CONV3H = 46;
// layer 8 (the once-per-image conv3(cond)) reading the caller's NCHW fp32 condition tensor DIRECTLY: a staging item's eight channels are eight
// 4-byte loads from eight channel planes (consecutive lanes = consecutive pixels of one plane: whole 128-byte segments) instead of two 16-byte
// loads from the channel-blocked copy -- the copy (438 MB read + 438 MB written per four KITTI maps: 189 us of a 7.5-ms step in the refined f16
// mode) is not made at all.  Split-f16 kernel only (the refined mode's hoisted plans with an explicit condition tensor); same tiles, packed
// weights, arithmetic and output order as layer 8 in that kind -- bit-identical results.
constexpr int CONV3C_NCHW = 47;
// Swin / MPViT denoiser, forward-only plans: upsample_fuse (convA, convB: no norm, no activation) and pred.0 are ONE linear map of
// s = up(feat) + E[t] + NE(x_t) (reference ...swin_addHAHI.py:321-333,378-380), so
//   pred.0(convB(convA(s))) = W3*WB*WA*NE(x_t)  +  [W3*(WB*(WA*up(feat) + a) + b)]  +  W3*WB*WA*(E[t] on every pixel)  + b3
// with every convolution zero-padding its own input as the reference's does.  The bracket is computed ONCE per image (layer 6 kernel on
// convA's and convB's weights, then layer 8: accumulator-fragment order, as the Res variant's hoisted conv3(cond)); the E[t] term is constant
// over the image except within three pixels of its border: a table per loop step with one row per border class (swin_ttab, dd_misc.hip).
//   SWIN_CONVA_H = convA on relu(gn2(y2)) alone (layer 5 without the condition / embedding addends, no bias)
//   SWIN_PRED_H  = pred.0 (layer 7) whose accumulators start at the hoisted term and whose epilogue adds the table rows
constexpr int SWIN_CONVA_H = 50, SWIN_PRED_H = 52;
//   SWIN_PRED5_H = pred.0 and convB as ONE 5x5 convolution 256 -> 64 on convA's result (W5[u] = sum over e + d = u of W3[e] . WB[d], built per
//   parameter generation by swin_compose, dd_misc.hip): 0.82 instead of 1.47 MFLOP per pixel and step and no convB result in HBM.  The 5x5
//   form also sums, at the pixels ON the image border, the terms W3[e] . convB(.)(q + e) for taps e that leave the image -- which the
//   reference's pred.0 zero-pads away; they are computed per step from the border rows / columns of convA's result (swin_bcorr: ring
//   buffer ConvParams::bcorr) and subtracted in the epilogue.  Accumulator start values and E[t] rows as SWIN_PRED_H.
constexpr int SWIN_PRED5_H = 53;
// the same on 16x32-pixel tiles (the tiling of BIG_CONV3C / BIG_CONV3H: half the weight stream per pixel, 40 MFMAs per stage, 0.75 LDS reads per
// MFMA), picked with the same rule (plan_big_tiles, dd_api_plans.cpp); its accumulator start values come from BIG_CONV3C
constexpr int SWIN_PRED5B_H = 51;

// ---- the list: every id that has a kernel, once -----------------------------------------------------------------------------------------
#define DD_KERNEL_IDS(X)                                                                                                                  \
  X(KID_CONV1) X(KID_CONV2) X(KID_CONV3) X(KID_CONV4) X(KID_SWIN_CONVA) X(KID_SWIN_CONVB) X(KID_SWIN_PRED) X(KID_CONV3C) X(KID_CONV3H)    \
  X(KID_FPN_LAT_RES + 0) X(KID_FPN_LAT_RES + 1) X(KID_FPN_LAT_RES + 2) X(KID_FPN_LAT_RES + 3) X(KID_FPN_UP)                               \
  X(KID_FPN_LAT_SWIN + 0) X(KID_FPN_LAT_SWIN + 1) X(KID_FPN_LAT_SWIN + 2) X(KID_FPN_LAT_SWIN + 3)                                         \
  X(KID_DGRAD4) X(KID_DGRAD3) X(KID_DGRAD2) X(KID_DGRAD1) X(KID_FPN_LAT_MPVIT + 0) X(KID_FPN_LAT_MPVIT + 1) X(KID_FPN_LAT_MPVIT + 2)      \
  X(KID_NECK_SWIN + 0) X(KID_NECK_SWIN + 1) X(KID_NECK_SWIN + 2) X(KID_NECK_SWIN + 3) X(KID_NECK_SWIN + 4) X(KID_NECK_SWIN + 5)           \
  X(KID_NECK_SWIN + 6) X(KID_NECK_SWIN + 7) X(KID_NECK_SWIN + 8) X(KID_NECK_SWIN + 9) X(KID_NECK_SWIN + 10) X(KID_NECK_SWIN + 11)         \
  X(ONE_CONV3H) X(CONV3C_NCHW) X(BIG_CONV3C) X(BIG_CONV3H) X(SWIN_CONVA_H) X(SWIN_PRED5B_H) X(SWIN_PRED_H) X(SWIN_PRED5_H)                \
  X(KID_NECK_MPVIT + 0) X(KID_NECK_MPVIT + 1) X(KID_NECK_MPVIT + 2) X(KID_NECK_MPVIT + 3) X(KID_NECK_MPVIT + 4) X(KID_NECK_MPVIT + 5)     \
  X(KID_NECK_MPVIT + 6) X(KID_NECK_MPVIT + 7) X(KID_NECK_MPVIT + 8) X(KID_NECK_MPVIT + 9) X(KID_NECK_MPVIT + 10) X(KID_NECK_MPVIT + 11)
constexpr int KID_LAST = KID_NECK_MPVIT + NECK_CONVS - 1;      // the largest id

// ---- constructors (host side) --------------------------------------------------------------------------------------------------------------
constexpr int kid_denoiser(int l) { return KID_CONV1 + l; }                  // l = 0..3: conv1..conv4
constexpr int kid_dgrad(int l) { return KID_DGRAD1 - l; }                    // data gradient of conv(l + 1)
constexpr int kid_swin_fuse(int i) { return KID_SWIN_CONVA + i; }            // 0 = convA, 1 = convB
constexpr int kid_fpn_lateral(int pyramid, int level) {
  return pyramid == PYRAMID_MPVIT ? KID_FPN_LAT_MPVIT + (level < 2 ? level : 2) : (pyramid == PYRAMID_SWIN ? KID_FPN_LAT_SWIN : KID_FPN_LAT_RES) + level;
}
constexpr int kid_neck_base(int pyramid) { return pyramid == PYRAMID_MPVIT ? KID_NECK_MPVIT : KID_NECK_SWIN; }
constexpr int kid_neck(int pyramid, int kind, int level) { return kid_neck_base(pyramid) + 4 * kind + level; }

// ---- classifiers (Cfg2 and the host) ----------------------------------------------------------------------------------------------------
// the layer whose arithmetic a special form runs ("base layer"; Cfg2::LAYER): itself for the plain ids
constexpr int kid_base(int id) {
  return (id == BIG_CONV3C || id == CONV3C_NCHW) ? KID_CONV3C : (id == BIG_CONV3H || id == ONE_CONV3H) ? KID_CONV3H : id == SWIN_CONVA_H ? KID_SWIN_CONVA
         : (id == SWIN_PRED_H || id == SWIN_PRED5_H || id == SWIN_PRED5B_H) ? KID_SWIN_PRED : id;
}
constexpr bool kid_is_big(int id) { return id == BIG_CONV3C || id == BIG_CONV3H || id == SWIN_PRED5B_H; }      // 16x32-pixel tiles (2-byte kinds only)
constexpr bool kid_in(int id, int first, int n) { return id >= first && id < first + n; }
constexpr bool kid_is_neck_mpvit(int id) { return kid_in(id, KID_NECK_MPVIT, NECK_CONVS); }
constexpr bool kid_is_neck(int id) { return kid_in(id, KID_NECK_SWIN, NECK_CONVS) || kid_is_neck_mpvit(id); }
constexpr int kid_neck_level(int id) { return kid_is_neck(id) ? (id - kid_neck_base(kid_is_neck_mpvit(id) ? PYRAMID_MPVIT : PYRAMID_SWIN)) % 4 : 0; }
constexpr int kid_neck_kind(int id) { return kid_is_neck(id) ? (id - kid_neck_base(kid_is_neck_mpvit(id) ? PYRAMID_MPVIT : PYRAMID_SWIN)) / 4 : -1; }
// channels the kernels carry per pyramid level (MPViT-small's 216 as 224)
constexpr int pyramid_c(int pyramid, int level) {
  return pyramid == PYRAMID_MPVIT ? (level == 0 ? 128 : level == 1 ? 224 : 288) : pyramid == PYRAMID_SWIN ? (192 << level) : (64 << level);
}
constexpr int kid_neck_c(int id) { return pyramid_c(kid_is_neck_mpvit(id) ? PYRAMID_MPVIT : PYRAMID_SWIN, kid_neck_level(id)); }
constexpr bool kid_is_fpn_lateral(int id) { return kid_in(id, KID_FPN_LAT_RES, FPN_LEVELS) || kid_in(id, KID_FPN_LAT_SWIN, FPN_LEVELS) || kid_in(id, KID_FPN_LAT_MPVIT, 3); }
constexpr int kid_fpn_lateral_cin(int id) {
  return kid_in(id, KID_FPN_LAT_MPVIT, 3) ? pyramid_c(PYRAMID_MPVIT, id - KID_FPN_LAT_MPVIT)
         : kid_in(id, KID_FPN_LAT_SWIN, FPN_LEVELS) ? pyramid_c(PYRAMID_SWIN, id - KID_FPN_LAT_SWIN) : pyramid_c(PYRAMID_RES, id - KID_FPN_LAT_RES);
}
constexpr bool kid_is_dgrad(int id) { return kid_in(id, KID_DGRAD4, 4); }
// the forward layers (denoiser, condition FPN, HAHI neck): what the split-f16 kind is instantiated for
constexpr bool kid_is_forward(int id) { return kid_in(id, KID_CONV1, 9) || kid_is_fpn_lateral(id) || id == KID_FPN_UP || kid_is_neck(id); }
constexpr int kid_cin(int id) {      // id = a base layer
  return kid_is_neck(id) ? (kid_neck_kind(id) == NECK_FUSION ? kid_neck_c(id) + NECK_EMBED_C : kid_neck_c(id)) : kid_is_fpn_lateral(id) ? kid_fpn_lateral_cin(id)
         : (id == KID_CONV1 || id == KID_DGRAD4) ? LATENT_C : (id == KID_CONV2 || id == KID_CONV4 || id == KID_DGRAD3 || id == KID_DGRAD1) ? HID_C : COND_C;
}
constexpr int kid_cout(int id) {
  return kid_is_neck(id) ? (kid_neck_kind(id) == NECK_PROJ ? NECK_EMBED_C : kid_neck_c(id)) : id == KID_FPN_UP ? 4 * COND_C
         : (id == KID_CONV4 || id == KID_DGRAD1) ? LATENT_C
         : (id == KID_CONV1 || id == KID_CONV3 || id == KID_SWIN_PRED || id == KID_CONV3C || id == KID_CONV3H || id == KID_DGRAD4 || id == KID_DGRAD2) ? HID_C : COND_C;
}
constexpr bool kid_listed(int id) {
#define DD_KID_EQ(K) || id == (K)
  return false DD_KERNEL_IDS(DD_KID_EQ);
#undef DD_KID_EQ
}

// ---- the routing rule --------------------------------------------------------------------------------------------------------------------
// Which instantiation Cfg2<ek, id> runs a requested (id, kind); id == 0: no kernel does, and launching / packing for the pair is an error.
struct KidRoute { int ek, id; };
constexpr KidRoute KID_NO_ROUTE{0, 0};
constexpr KidRoute kid_route(int id, int ek) {
  if (!kid_listed(id)) return KID_NO_ROUTE;
  switch (ek) {
    case EK_F32: case EK_BF16: case EK_F16:      // plain kinds: every id but the NCHW reader; 16x32 tiles in the 2-byte kinds only; the one-buffer conv3 where a mode runs it (f16)
      if (id == CONV3C_NCHW || (kid_is_big(id) && ek == EK_F32)) return KID_NO_ROUTE;
      if (id == ONE_CONV3H && ek != EK_F16) return KidRoute{ek, KID_CONV3H};
      return KidRoute{ek, id};
    case EK_BF16M:      // bf16 operands, f16 storage: the layers that change kind between storage and operands have their own instantiations, the thin / once-per-
                        // image layers run as f16 kernels, everything else (Swin convB, inner FPN layers, data gradients) as bf16 kernels
      if (id == KID_CONV2 || id == KID_CONV3 || id == KID_SWIN_CONVA || id == KID_SWIN_PRED || id == KID_CONV3H || id == BIG_CONV3H || id == ONE_CONV3H ||
          id == SWIN_CONVA_H || id == SWIN_PRED_H || id == SWIN_PRED5_H || id == SWIN_PRED5B_H ||
          id == kid_fpn_lateral(PYRAMID_RES, 0) || id == kid_fpn_lateral(PYRAMID_SWIN, 0) || id == kid_fpn_lateral(PYRAMID_MPVIT, 0))
        return KidRoute{EK_BF16M, id};
      return kid_route(id, (id == KID_CONV1 || id == KID_CONV4 || id == KID_CONV3C || id == BIG_CONV3C) ? EK_F16 : EK_BF16);
    case EK_F16S:       // split f16: the forward layers (the hoisted Swin plans always run the 5x5 form) and the NCHW reader
      if (id == ONE_CONV3H) return KidRoute{EK_F16S, KID_CONV3H};
      if (kid_is_forward(id) || id == CONV3C_NCHW || id == SWIN_CONVA_H || id == SWIN_PRED5_H) return KidRoute{EK_F16S, id};
      return KID_NO_ROUTE;
    case EK_F16R:       // refined f16: conv1 and the hoisted conv3 / Swin 5x5 forms have their own instantiations; everything else is the f16 mode's kernel
                        // (the split-f16 layer 8 and the stacked conv4 are launched by the host under their own kinds / launchers)
      if (id == KID_CONV1 || id == KID_CONV3H || id == BIG_CONV3H || id == ONE_CONV3H || id == SWIN_PRED5_H || id == SWIN_PRED5B_H) return KidRoute{EK_F16R, id};
      return kid_route(id, EK_F16);
    default: return KID_NO_ROUTE;
  }
}
// The Cfg2 whose tiling describes the PACKED WEIGHT IMAGE of a routed pair: forms that share an image answer with the layer that owns it, the
// 2-byte kinds share one geometry, EK_F16R packs conv1 as the split image and everything else as f16 (conv4 stacked: conv_pack_geom2).
constexpr KidRoute kid_image(int id, int ek) {
  if (kid_route(id, ek).id == 0) return KID_NO_ROUTE;
  const int img = (id == ONE_CONV3H || id == SWIN_CONVA_H || id == SWIN_PRED_H || id == CONV3C_NCHW) ? kid_base(id) : id;
  return KidRoute{ek == EK_F16R ? (id == KID_CONV1 ? (int)EK_F16S : (int)EK_F16) : ek == EK_BF16M ? (int)EK_BF16 : ek, img};
}

}  // namespace dd
