// dd_igemm2_cfg.h -- per-layer tiling constants of the fused convolution kernels (dd_igemm2.hip).
// Variants that were measured slower on MI355X and removed in round 2 (profiles/history/r01_run30_power_and_variants.md,
// profiles/history/r02_run1_ddimloss_and_winograd.md): wave-specialised staging waves, a 16x32 / 8-wave / 9-taps-per-stage conv3 tile with
// and without ping-pong halves, persistent conv1 / conv4 workgroups, in-loop interleaving of the prologue, Winograd F(2x2,3x3).
// Round 3 (profiles/history/r03_run2_variants.md): the next stage's weight DMA issued between the tap groups of the MFMA block, conv1 at eight
// waves per SIMD, eight-wave "latency variants" of conv2 / conv3, a persistent conv3.
#pragma once
#include "dd_elem.h"
#include "dd_kernel_ids.h"

// ConvParams::ablate (timing experiments: skip parts of the kernel) is honoured only in builds with -DDD_ABLATE=1;
// the default build folds every check away so the main loop is straight-line code.
#ifndef DD_FRAG_DEPTH
#define DD_FRAG_DEPTH 2
#endif
#ifndef DD_RAW_DEPTH
#define DD_RAW_DEPTH 2
#endif
#ifndef DD_ABLATE
#define DD_ABLATE 0
#endif
// tiling of the conv3-shaped layers (256 -> 64: layers 3, 7, 8, 9) in the 2-byte kinds:
//   0 = 8x32 pixels, 32-channel chunks, 3 taps per stage (24 MFMAs per wave between barriers)
//   1 = 8x32 pixels, 16-channel chunks, 9 taps per stage (36 MFMAs per wave between barriers)
//   2 = 16x32 pixels, 4 waves x (128 pixels x 64 couts), 16-channel chunks, 9 taps per stage (72 MFMAs between barriers, 0.75 LDS reads per MFMA)
// Round 3: tiling 2 is ALSO instantiated beside the default as the kernel ids BIG_CONV3C / BIG_CONV3H (layers 8 / 9) and picked per launch when
// the tiles do not fit the chip at once -- under the two concurrent lanes it is worth +1.8 % at B=4 and +4 % at B=8 (profiles/history/r03_run2_variants.md).
#ifndef DD_C3
#define DD_C3 1
#endif
// conv2 (64 -> 256, two 128-cout splits): 1 = ONE workgroup per tile walks both cout splits over the same staged input patch (one
// prologue -- partial sums, table, patch fetch, normalisation -- per tile instead of two; the second split's weight stream follows
// the first's without a gap); 0 = one workgroup per (tile, split)
#ifndef DD_C3_2_RD1
#define DD_C3_2_RD1 1      // 16x32 conv3 tiles: raw patch one chunk ahead only (registers: two workgroups per CU need <= 128 VGPRs beside the accumulators)
#endif
// Swin fuse convs (256 -> 256, layers 5 / 6) in the 2-byte kinds: 0 = 32-channel chunks, one tap per stage (16 MFMAs per wave between
// barriers); 1 [default since round 2: convB -4.6 %, convA -5 % with the two options below] = 16-channel chunks, three taps per stage
// (24 MFMAs between barriers, 46 KB of LDS)
#ifndef DD_SWIN_TG3
#define DD_SWIN_TG3 1
#endif
// s_setprio level of a wave while it is inside a stage's MFMA block (0 = off)
#ifndef DD_SETPRIO
#define DD_SETPRIO 0
#endif
#ifndef DD_SWIN_FD2
#define DD_SWIN_FD2 1      // convA with DD_SWIN_TG3: two-deep fragment registers (the 32-channel-chunk prologue left no room for them)
#endif
#ifndef DD_SWIN_RD2
#define DD_SWIN_RD2 1      // convB with DD_SWIN_TG3: raw patch two chunks ahead
#endif
#ifndef DD_CONV2_DUAL
#define DD_CONV2_DUAL 1
#endif
// 1 = kernels take the timestep from ConvParams::t_known when the host knew it (0: always through the tvec load; A/B switch)
#ifndef DD_T_KNOWN
#define DD_T_KNOWN 1
#endif
// hoisted condition term conv3(cond) (layer 8 -> layer 9) in the 2-byte modes: 1 = stored as f16 quads (8 bytes per lane and register quad:
// 128 instead of 256 bytes per pixel and step in conv3's prologue; it is added to accumulators whose result is stored as f16 anyway),
// 0 = fp32.  The fp32 and split-f16 modes always keep fp32.
#ifndef DD_CADD_F16
#define DD_CADD_F16 1      // measured (round 3, one box): conv3 155 -> 138 us at KITTI B=4, 46.5 -> 44.9 at B=1; loop 7.30 -> 7.03 ms
#endif
// conv4 (64 -> 16) in the 2-byte kinds: 1 = 16-channel chunks, nine taps per stage (four chunks, double-buffered 11-KB patches, 40 KB of LDS:
// three to four workgroups per CU instead of two, the next chunk's loads fly under the current chunk's MFMAs); 0 = one 64-channel patch
#ifndef DD_C4_CK16
#define DD_C4_CK16 1       // measured (round 3): conv4 36.7 -> 34.3 us at KITTI B=4, neutral at B=1
#endif
// per-workgroup phase timestamps (ConvParams::prof); compiled in by tools/phase_prof.py only
#ifndef DD_PHASE_PROF
#define DD_PHASE_PROF 0
#endif

namespace dd {

template <int EKM_, int LAYER_ID_> struct Cfg2 {
  // kernel ids BIG_CONV3C / BIG_CONV3H (dd_kernel_ids.h) = layers 8 / 9 on 16x32-pixel tiles
  static constexpr bool BIG = kid_is_big(LAYER_ID_);
  // kernel ids SWIN_CONVA_H / SWIN_PRED_H (dd_kernel_ids.h) = layers 5 / 7 of the Swin denoiser with the step-invariant terms hoisted
  // SWIN_PRED5_H = pred.0 o convB as one 5x5 convolution (layer 7's tiling with five taps per stage)
  static constexpr bool PRED5 = LAYER_ID_ == SWIN_PRED5_H || LAYER_ID_ == SWIN_PRED5B_H;
  static constexpr bool HOIST_A = LAYER_ID_ == SWIN_CONVA_H, ADD_T = LAYER_ID_ == SWIN_PRED_H || PRED5;
  static constexpr bool IN_NCHW = LAYER_ID_ == CONV3C_NCHW;     // layer 8 on the caller's NCHW fp32 tensor (dd_kernel_ids.h)
  static constexpr int LAYER_ = kid_base(LAYER_ID_);
  // EKM_ = element kind or the mode EK_BF16M (dd_kernels.h).  In that mode only the layers that CHANGE kind between storage and operands
  // are instantiated here -- conv2 / conv3 / hoisted conv3 / Swin convA (f16 in, bf16 operands), the producers of f16 tensors in front
  // of them (conv2, conv3, Swin pred.0, the level-0 lateral conv of the condition FPN); the launcher sends every other layer to its
  // plain f16 (conv1, conv4, once-per-image conv3(cond)) or bf16 (Swin convB, inner FPN layers, data gradients) instantiation.
  static constexpr bool MX = EKM_ == EK_BF16M;
  // EKM_ == EK_F16S (split f16, DD_PREC_F16X3; dd_kernels.h): tensors in HBM are fp32 (the fp32 mode's layouts), the LDS patch and the
  // packed weights carry TWO f16 planes (hi, lo) and every (weight, pixel) fragment pair costs three MFMAs.  Instantiated for the
  // denoiser's layers 1..9 and (round 4) the once-per-image layers in front of them -- the condition FPN 10..18 / 24..26 and the HAHI neck
  // 30..41 / 54..65, which the split / refined f16 modes used to run on the fp32-operand kernels (a fifth of this rate); one tiling for all
  // of them: 16-channel chunks, 3 taps per stage (conv1: 9, the 1x1 layers: 1), 64-cout workgroup tiles.
  // EKM_ == EK_F16R (refined f16, DD_PREC_F16R; dd_kernels.h): instantiated for the layers whose kernel differs from the f16 mode's only --
  // conv1 (its weights as an f16 pair against a single-plane patch, y1 stored f16) and the producer of y3 -- the hoisted conv3 of the Res denoiser
  // (layer 9 and its tile forms) / the 5x5 form pred.0 o convB of the Swin denoiser: f16 operands and input, the hoisted term read as block-scaled
  // int16, y3 written as int16 with a per-pixel scale; every other layer of the mode runs its EK_F16 (conv2, Swin convA', conv4 via dd_thin.hip)
  // or EK_F16S (the once-per-image chain) form.
  static constexpr bool RF = EKM_ == EK_F16R;
  static_assert(!RF || LAYER_ == KID_CONV1 || LAYER_ == KID_CONV3H || PRED5, "EK_F16R is instantiated for conv1 and the hoisted conv3 / Swin 5x5 forms only");
  static constexpr bool SPLIT = EKM_ == EK_F16S || (RF && LAYER_ == KID_CONV1);
  static_assert(!IN_NCHW || EKM_ == EK_F16S, "the NCHW-reading layer 8 is a split-f16 kernel");
  static constexpr bool WONLY = RF && LAYER_ == KID_CONV1;             // split weights against a single-plane patch: W.P = Whi.P + Wlo.P
  static constexpr int NPL = SPLIT ? 2 : 1;                    // operand planes of a packed weight stage
  static constexpr int NPLP = (SPLIT && !WONLY) ? 2 : 1;       // operand planes of the LDS patch
  static constexpr bool Q15 = RF && (LAYER_ == KID_CONV3H || PRED5);    // hoisted term read as scaled int16 quads, y3 written as int16 with a per-pixel scale
  static constexpr int EK = MX ? (int)EK_BF16 : (SPLIT || RF) ? (int)EK_F16 : EKM_;          // MFMA operand kind = kind of the LDS patch and of the packed weights
  static constexpr int LAYER = LAYER_;
  static constexpr int IN_K = SPLIT ? (int)EK_F32 : (MX && (LAYER_ == KID_CONV2 || LAYER_ == KID_CONV3 || LAYER_ == KID_SWIN_CONVA || LAYER_ == KID_CONV3H)) ? (int)EK_F16 : EK;      // stored input (and condition map)
  static constexpr int OUT_K = RF ? (int)EK_F16 : SPLIT ? (int)EK_F32 : (MX && (LAYER_ == KID_CONV2 || LAYER_ == KID_CONV3 || LAYER_ == KID_SWIN_PRED || LAYER_ == KID_CONV3H || LAYER_ == KID_FPN_LAT_RES || LAYER_ == KID_FPN_LAT_SWIN || LAYER_ == KID_FPN_LAT_MPVIT)) ? (int)EK_F16 : EK;
  static_assert(!MX || IN_K != EK || OUT_K != EK, "EK_BF16M is instantiated only for the layers that change kind");
  static_assert(!SPLIT || kid_is_forward(LAYER_),
                "EK_F16S is instantiated for the forward layers only (denoiser, condition FPN, HAHI neck)");
  static_assert(!SPLIT || LAYER_ID_ != SWIN_PRED_H, "split f16: the hoisted Swin plans always run the 5x5 form");
  static constexpr int ESZ = ElemSize<EK>::V;
  // what every layer computes: dd_kernel_ids.h
  static constexpr bool IS_NECK = kid_is_neck(LAYER);
  static constexpr int NECK_KIND = kid_neck_kind(LAYER);      // NECK_LATERAL, NECK_PROJ, NECK_FUSION
  static constexpr bool IS_LAT = kid_is_fpn_lateral(LAYER);
  static constexpr bool IS_UP = (LAYER == KID_FPN_UP);
  static constexpr bool IS_C1 = LAYER == KID_CONV1, IS_C2 = LAYER == KID_CONV2, IS_C4 = LAYER == KID_CONV4, IS_C3H = LAYER == KID_CONV3H;      // shorthands for the rules below
  static constexpr bool IS_D4 = LAYER == KID_DGRAD4, IS_D3 = LAYER == KID_DGRAD3, IS_D2 = LAYER == KID_DGRAD2, IS_D1 = LAYER == KID_DGRAD1;
  static constexpr bool IS_CONVA = LAYER == KID_SWIN_CONVA, IS_CONVB = LAYER == KID_SWIN_CONVB;
  static constexpr int KS = PRED5 ? 5 : (IS_UP || (IS_NECK && NECK_KIND != NECK_FUSION)) ? 1 : 3;      // kernel size
  static constexpr int HALO = KS / 2;
  static constexpr int NTAPS = KS * KS;
  static constexpr int CIN = kid_cin(LAYER), COUT = kid_cout(LAYER);
  static constexpr bool RELU_OUT = IS_LAT || IS_UP || IS_NECK;   // epilogue: relu(acc + bias)
  static constexpr bool SCATTER = IS_UP;                         // epilogue: cout block -> output parity of a 2x upsampled tensor
  static constexpr int COUT_PAD = (COUT < 32) ? 32 : IS_NECK ? ((COUT + 63) / 64) * 64 : COUT;
  static constexpr bool C3SHAPE = (LAYER == KID_CONV3 || LAYER == KID_SWIN_PRED || LAYER == KID_CONV3C || IS_C3H);
  static constexpr int C3 = (C3SHAPE && ESZ == 2 && !SPLIT) ? (BIG ? 2 : DD_C3) : 0;
  static_assert(!BIG || (ESZ == 2 && !SPLIT), "big-tile forms: 2-byte kinds only");
  static constexpr bool SWIN3 = DD_SWIN_TG3 && (IS_CONVA || IS_CONVB) && ESZ == 2 && !SPLIT;
  static constexpr bool C4K16 = DD_C4_CK16 && IS_C4 && ESZ == 2 && !SPLIT;
  static constexpr int CK = (SPLIT || C4K16) ? 16 : (IS_C1 || IS_D4) ? 16 : (IS_C2 || IS_C4 || IS_D3 || IS_D1) ? (128 / ESZ) : (C3 != 0 || SWIN3) ? 16 : (64 / ESZ);
  static constexpr int TG = PRED5 ? 5 : SPLIT ? (IS_C1 ? 9 : KS == 1 ? 1 : 3) : (IS_C1 || IS_D4 || C3 != 0 || C4K16) ? 9 : (IS_D2 || IS_D1) ? 3
                          : SWIN3 ? 3 : (IS_C2 || IS_CONVA || IS_CONVB || IS_D3 || IS_LAT || IS_UP || IS_NECK) ? 1 : 3;
  static constexpr int NT = (IS_NECK || (SPLIT && COUT >= 64)) ? 64 : (COUT >= COND_C) ? 128 : COUT_PAD;
  static constexpr int SPW = (IS_C2 && ESZ == 2 && DD_CONV2_DUAL && !SPLIT) ? 2 : 1;      // cout splits one workgroup walks (over one staged patch)
  static constexpr bool STATS = IS_C1 || IS_C2 || LAYER == KID_CONV3 || IS_C4 || LAYER == KID_SWIN_PRED || IS_C3H;   // a GroupNorm follows this convolution
  static constexpr bool ADD_C = IS_C3H;                         // epilogue adds the hoisted condition / embedding terms
  static constexpr bool ADD_ACC = ADD_C || ADD_T;              // accumulators start at the hoisted per-image term (ConvParams::cadd)
  static constexpr bool CADD16 = DD_CADD_F16 && ESZ == 2 && !SPLIT && !RF && (LAYER == KID_CONV3C || IS_C3H || ADD_T);   // the hoisted term travels as f16
  // conv1 / conv4 are latency-bound (18 MFMAs per 32-pixel block): 8 waves of one block each shorten every wave's
  // dependent chain (measured: 4x32 tiles with 4 waves were no faster for conv1 and slower for conv4 - more halo and
  // weight traffic); conv2 / conv3 and the Swin convs keep 4 waves x 2 blocks (fewer LDS reads per MFMA)
  static constexpr int TH = (C3 == 2) ? 16 : 8, TW = 32;
  static constexpr int WAVES = (IS_C1 || IS_C4 || IS_D4 || IS_D1) ? 8 : 4;
  static constexpr int THREADS = WAVES * 64;
  static constexpr int WM = (TH * TW) / (32 * WAVES);
  static constexpr int WN = NT / 32;
  static constexpr int PRO = (HOIST_A || IS_C2 || IS_C4 || IS_C3H) ? PRO_GN : IS_C1 ? PRO_X : (LAYER == KID_CONV3 || IS_CONVA) ? PRO_GN_ADD : PRO_RAW;
  static constexpr int IN_ESZ = (IS_C1 || SPLIT) ? 4 : ESZ;
  static constexpr int OUT_ESZ = RF ? 2 : (IS_C4 || LAYER == KID_CONV3C || IS_D1 || SPLIT) ? 4 : ESZ;
  static constexpr int PH = TH + 2 * HALO, PW = TW + 2 * HALO;
  static constexpr int ROWB = CK * ESZ;                  // 32 / 64 / 128 bytes
  static constexpr int PPP = ROWB / 16;
  static constexpr int LOG2_PPP = (PPP == 2) ? 1 : (PPP == 4) ? 2 : 3;
  static constexpr int RPB = 256 / ROWB;                 // rows per 256-B LDS bank row
  static constexpr int EPP = 16 / ESZ;
  static constexpr int NKQ = PPP / 2;                    // MFMA k-steps per tap (16 B from each half-wave)
  static constexpr int NCHUNK = CIN / CK;
  static constexpr int NTG = NTAPS / TG;
  static constexpr int NSTAGE = NCHUNK * NTG;
  // kernel id ONE_CONV3H: the hoisted conv3 on 8x32 tiles with ONE patch buffer -- the next chunk's patch is written into the buffer the MFMAs just
  // read, behind a second workgroup barrier per stage, instead of into a twin buffer under the running stage.  63 -> 52 KB of LDS = THREE
  // workgroups per CU (12 waves, three per SIMD; the kernel needs 160 VGPRs) where the two-buffer form has two: a wave spends ~20 % of a stage in
  // its MFMA block and the rest waiting for memory, the weight DMA or a barrier -- it lacks co-resident waves, not issue slots.  Measured
  // (round 4, profiles/history/r04_call3_*): conv3 at KITTI B=4 on one stream 140 -> 132 us (bf16), 147 -> 137 (f16r); neutral under two lanes and at B=1
  static constexpr bool ONEBUF = LAYER_ID_ == ONE_CONV3H;
  static_assert(!ONEBUF || (C3 == 1 && NCHUNK > 1), "one-buffer form: the 8x32 tiling of the 2-byte kinds");
  static constexpr int NPB = (NCHUNK > 1 && !ONEBUF) ? 2 : 1;       // patch buffers
  static constexpr int PATCH_PLANE = PH * PW * ROWB;      // one operand plane of a patch buffer (split f16: hi plane, then lo plane)
  static constexpr int PATCH_BYTES = NPLP * PATCH_PLANE;
  static constexpr int W_PLANE = TG * NT * ROWB;          // one operand plane of a weight stage
  static constexpr int W_BYTES = NPL * W_PLANE;
  static constexpr int NWB = (NSTAGE > 1) ? 2 : 1;       // weight ring slots
  static constexpr int W_OFF = NPB * PATCH_BYTES;        // LDS byte offset of the weight ring
  static constexpr int CTAB = (PRO == PRO_RAW) ? 0 : IS_C1 ? LATENT_C : CIN;   // channels of the prologue GroupNorm table
  static constexpr int SCR_FLOATS = 2 * 8 * 8;                               // cross-wave scratch of the statistics epilogue: 8 doubles per wave
  static constexpr int NTABS = (PRO == PRO_GN_ADD) ? 3 : 2;                   // a, b (and the embedding row e) of the prologue GroupNorm
  static constexpr int TAB_FLOATS = NTABS * CTAB + NT * SPW + (ADD_C ? 10 * HID_C : 0) + SCR_FLOATS;   // GroupNorm table, bias, E[t] tap sums, scratch
  static constexpr int SMEM_BYTES = NPB * PATCH_BYTES + NWB * W_BYTES + TAB_FLOATS * 4;
  static constexpr int ITEMS = PH * PW * PPP;
  static constexpr int NIT = (ITEMS + THREADS - 1) / THREADS;      // staging items per thread
  static constexpr int NLD = EPP * IN_ESZ / 16;
  static constexpr int PIXSTRIDE = (CIN >= ACT_CB) ? ACT_CB : CIN; // elements between pixels of one channel block
  // two-deep fragment registers in the MFMA loop (next group's ds_reads issued between this group's MFMAs); the Swin convA
  // prologue (GroupNorm + upsampled condition + embedding on 256 channels, 128 couts per wave) has no registers to spare
  // raw-patch register slots: layers whose prologue reads ONE tensor (no aux term) and has several channel chunks fetch two
  // chunks ahead -- measured on MI355X the global-load latency under load (4-5 us) exceeds one chunk of MFMA work
  static constexpr int RAW_DEPTH = (DD_RAW_DEPTH == 2 && !SPLIT && (IS_C3H || LAYER == KID_SWIN_PRED || IS_D2 || ((IS_CONVB || HOIST_A) && SWIN3 && DD_SWIN_RD2)) && !(C3 == 2 && DD_C3_2_RD1)) ? 2 : 1;
  static constexpr int FRAG_DEPTH = (IS_CONVA && !SPLIT && !(SWIN3 && DD_SWIN_FD2)) ? 1 : DD_FRAG_DEPTH;
  // registers: two workgroups per CU for conv2 / conv3 (8 waves = 2 per SIMD, <= 256 VGPR+AGPR);
  // conv1 / conv4 want >= 2 eight-wave workgroups per CU (<= 128 registers)
  static constexpr int MIN_WAVES_PER_SIMD = (WAVES == 8) ? ((SMEM_BYTES <= 80 * 1024) ? 4 : 2) : (ONEBUF && SMEM_BYTES <= 160 * 1024 / 3) ? 3 : ((SMEM_BYTES <= 80 * 1024) ? 2 : 1);   // 80 KiB = half the CU's LDS
  static_assert(CIN % CK == 0 && NTAPS % TG == 0 && COUT_PAD % NT == 0, "tiling");
  static_assert(PATCH_BYTES % 16 == 0 && W_BYTES % 1024 == 0, "LDS carve / DMA granularity");
  static_assert(WAVES <= 8 && (COUT_PAD / NT) % SPW == 0 && (SPW == 1 || NCHUNK == 1), "scratch size; splits per workgroup");
  static_assert(ROWB == 32 || ROWB == 64 || ROWB == 128, "swizzle derivation");
  static_assert(TW == 32, "one 32-pixel MFMA block == one tile row (column-only swizzle, lane == column)");
  static_assert(THREADS % PPP == 0 && NIT <= 32, "per-thread piece index is constant; masks fit 32 bits");
  static_assert(TG == 1 || TG == 3 || TG == 9 || (TG == 5 && KS == 5), "tap decomposition");
};

// LDS swizzle: 16-B piece j of a row is stored at j ^ swz(k), k = the row's COLUMN index in the patch
// (weights: the cout row index).  Any 16 lanes with distinct k mod 16 then hit 16 distinct 16-B slots of
// the 256-B bank row, whatever the (wave-uniform) patch row is, because PW*ROWB is a multiple of 128 B.
template <int RPB, int PPP> __device__ __forceinline__ int swz16(int k) { return ((k / RPB) & (PPP - 1)) << 4; }

}  // namespace dd
