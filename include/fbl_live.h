/* libfbl -- clip norm and Adam over a LIVE SET of the flat trainable buffer (MI355X, gfx950): partial fine-tuning, where
 * the parameters whose requires_grad the caller switched off must neither be read into the norm nor be moved.  Same library,
 * same conventions as fbl.h: extern "C", plain device pointers + sizes, `stream` a hipStream_t passed as void*, every
 * function only enqueues work (no allocation / copy / sync inside), returns 0, a positive hipError_t or a negative
 * FBL_ERR_* code.  Bound from Python by frozenbilm_amd/lib.py LIVE_SIGNATURES, derived from this header.
 *
 * The live set is a table in DEVICE memory, int64:
 *     ranges[0] = nr                 number of ranges, 0 <= nr <= 1024 (more are ignored)
 *     ranges[1] = n_live             live elements = sum of the range lengths
 *     ranges[2 + 2r] = begin_r       first element of range r
 *     ranges[3 + 2r] = cum_r         live elements in front of range r (cum_0 = 0)
 * Ranges are sorted, disjoint, and begin and end on multiples of 8 elements (the flat layout pads every parameter to 8
 * floats).  No host copy of the table is taken: the launch arguments depend on n alone, so a captured launch follows the
 * table it was given.  An access that the table would place outside [0, n) is skipped.
 */
#ifndef FBL_LIVE_H
#define FBL_LIVE_H
#include "fbl.h"
#ifdef __cplusplus
extern "C" {
#endif

/* out_sumsq[0] += sum of x[i]^2 over the live elements of x fp32 [n].  Elements outside the ranges are not read into the
 * result (a NaN there stays there).  ws: fbl_sumsq_ws_floats() floats.  Two launches, ordered fold: identical calls give
 * identical bits, and one range [0, n) gives the bits of fbl_sumsq(x, n, ..).  n % 8 == 0, x 16-byte aligned. */
int fbl_sumsq_live(const float* x, int64_t n, const int64_t* ranges, float* out_sumsq, float* ws, void* stream);

/* fbl_adam_flat on the live elements of p / g / m / v fp32 [n]: the same arithmetic in the same order with the same clip
 * factor from the device norm `sumsq` (NULL or max_norm <= 0: no clip).  Words outside the ranges are neither read into a
 * result nor written.  One launch; one range [0, n) gives the bits of fbl_adam_flat.  n % 8 == 0, pointers 16-byte aligned. */
int fbl_adam_flat_live(float* p, const float* g, float* m, float* v, int64_t n, const int64_t* ranges, float lr, float beta1,
                       float beta2, float eps, float weight_decay, int step, const float* sumsq, float max_norm,
                       float grad_scale, void* stream);

#ifdef __cplusplus
}
#endif
#endif
