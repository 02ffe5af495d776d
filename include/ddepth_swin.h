/*
 * ddepth_swin.h -- the shifted-window multi-head self-attention of the Swin backbone (reference src/model/backbone/swin.py, ShiftWindowMSA), forward
 * only, as ONE kernel between the module's `qkv` and `proj` Linears (same shared library as ddepth.h; kernel in diffusiondepth_amd/csrc/dd_swin.hip).
 * Opt-in: nothing in the other headers changes.
 *
 * What it replaces: pad -> roll -> mask build -> window partition -> reshape / permute -> scale -> Q K^T -> + relative-position bias -> + mask ->
 * softmax -> . V -> transpose / reshape -> window reverse -> roll -> crop.  All of it is addressing here:
 *     qkv      fp32 [B, H, W, 3 C], IMAGE-TOKEN layout: what the `qkv` Linear writes for the un-padded, un-rolled, un-partitioned tokens;
 *              channel order [3][heads][32]
 *     qkv_pad  3 C floats, or NULL for zeros: the qkv vector of a padded token.  The reference pads H and W up to multiples of the window AFTER
 *              norm1 and BEFORE qkv, so a padded token's q, k and v are the Linear's bias.  Padded tokens ARE attended to as keys (the
 *              reference does not mask them); they are never stored.
 *     rel_bias fp32 [heads, 49, 49], dense: relative_position_bias_table[relative_position_index], permuted to [head][query][key]
 *     out      fp32 [B, H, W, C], channel head * 32 + d: what `proj` reads
 *     shift    0 <= shift < window: the cyclic roll by -shift on the padded frame.  With shift > 0 the three row bands and three column bands
 *              [0, Hp - 7), [Hp - 7, Hp - shift), [Hp - shift, Hp) are labelled on the rolled padded frame, and a (query, key) pair of one
 *              window with different labels gets an additive -100.0 (NOT -inf), as in the reference.
 *     out[token] = softmax_keys(q * 32^-0.5 . k^T + rel_bias + mask) . v     per window and head, the row maximum subtracted before exp
 * Accumulation and softmax are fp32 at every precision; `precision` chooses the MFMA operand type only: DD_PREC_FP32 (the parity mode),
 * DD_PREC_BF16 or DD_PREC_F16, which round q * scale, k, the probabilities and v once each.
 *
 * Supported: C == 32 * heads, window == 7, those three precisions.  Anything else is DD_ERR_UNSUPPORTED, answered before anything is launched.
 *
 * Conventions: DEVICE pointers, contiguous fp32, qkv / qkv_pad 16-byte aligned; asynchronous on `stream`; no workspace, no atomics, no host
 * synchronisation, allocation or host read of device memory (the call can be captured in a graph); two calls give the same bits; `out` may not
 * alias an input; DD_OK or a dd_status code (ddepth.h) with the message in dd_swin_last_error().
 *
 * Not here: the backward, other windows and head dimensions, the split-f16 mode.
 */
#ifndef DDEPTH_SWIN_H_
#define DDEPTH_SWIN_H_

#ifdef __cplusplus
extern "C" {
#endif

/* The message of the last failed call of this header on the calling thread. */
const char* dd_swin_last_error(void);

/* 1 where (C, heads, window, precision) runs in this library, else 0.  No side effects. */
int dd_window_attention_supported(int C, int heads, int window, int precision);

int dd_window_attention_forward(const float* qkv, const float* qkv_pad, const float* rel_bias, float* out, int B, int H, int W, int C,
                                int heads, int window, int shift, int precision, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DDEPTH_SWIN_H_ */
