/* libfbl -- an exponential moving average (EMA) of the trainable weights, kept INSIDE the Adam launch over parameter groups
 * (MI355X, gfx950), and the exchange of two fp32 buffers that puts the average in the parameters' place for evaluation.  Same
 * library, same conventions as fbl.h: extern "C", plain device pointers + sizes, `stream` a hipStream_t passed as void*, every
 * function only enqueues work (no allocation / copy / sync inside), returns 0, a positive hipError_t or a negative FBL_ERR_*
 * code.  Bound from Python by frozenbilm_amd/lib.py EMA_SIGNATURES, derived from this header.
 *
 * The segment table, the hyper-parameter records and FBL_ADAM_MAX_GROUPS / FBL_ADAM_GROUP_FLOATS are those of fbl_groups.h.
 */
#ifndef FBL_EMA_H
#define FBL_EMA_H
#include "fbl_groups.h"
#ifdef __cplusplus
extern "C" {
#endif

/* fbl_adam_flat_groups on p / g / m / v fp32 [n] -- its arguments, its table, its argument rules, and for every element of
 * every segment the bits it gives p, m and v (the same arithmetic, instruction for instruction) -- and, while the updated
 * parameter is in a register, one step of the average ema fp32 [n]:
 *     d = p_new - ema[i]   (rounded to fp32);   ema[i] = fma(ema_w, d, ema[i]).
 * The lerp form is deliberate: where ema[i] == p_new the average keeps its bits.  With ema_w = 1 - decay this is
 * ema <- decay * ema + (1 - decay) * p_new up to the two roundings.  Words outside the segments are neither read into a result
 * nor written, in ema as in the other four buffers; a malformed table or a segment whose group lies outside [0, n_groups)
 * touches nothing.  One launch.
 * NULL p / g / m / v / ema / segs / hyper, n_groups outside 1 .. FBL_ADAM_MAX_GROUPS or ema_w outside (0, 1]: FBL_ERR_ARG;
 * n % 8 != 0 or a pointer that is not 16-byte aligned: FBL_ERR_ALIGN; then n <= 0: 0, nothing launched. */
int fbl_adam_flat_groups_ema(float* p, const float* g, float* m, float* v, float* ema, int64_t n, const int64_t* segs,
                             int n_groups, const float* hyper, int step, const float* sumsq, float max_norm, float grad_scale,
                             float ema_w, void* stream);

/* a <-> b, fp32 [n], in place: the words move as bits (NaN payloads and signed zeros included), so swapping twice is the
 * identity.  The buffers must not overlap.  One launch.
 * NULL a / b or a == b: FBL_ERR_ARG; n % 8 != 0 or a pointer that is not 16-byte aligned: FBL_ERR_ALIGN; then n <= 0: 0. */
int fbl_swap_f32(float* a, float* b, int64_t n, void* stream);

#ifdef __cplusplus
}
#endif
#endif
