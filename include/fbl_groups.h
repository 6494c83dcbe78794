/* libfbl -- Adam over PARAMETER GROUPS of the flat trainable buffer (MI355X, gfx950): every group with its own learning rate,
 * betas, epsilon and weight decay, coupled (L2, folded into the gradient) or decoupled (AdamW), in ONE launch over the live
 * set.  Same library, same conventions as fbl.h: extern "C", plain device pointers + sizes, `stream` a hipStream_t passed as
 * void*, every function only enqueues work (no allocation / copy / sync inside), returns 0, a positive hipError_t or a
 * negative FBL_ERR_* code.  Bound from Python by frozenbilm_amd/lib.py GROUP_SIGNATURES, derived from this header.
 *
 * The segments are a table in DEVICE memory, int64, in the spirit of the live table of fbl_live.h:
 *     segs[0] = ns                   number of segments, 0 <= ns <= 1024 (more are ignored)
 *     segs[1] = n_live               live elements = sum of the segment lengths
 *     segs[2 + 3s] = begin_s         first element of segment s
 *     segs[3 + 3s] = cum_s           live elements in front of segment s (cum_0 = 0)
 *     segs[4 + 3s] = group_s         the parameter group of segment s
 * A segment is a maximal run of the flat buffer that is live and belongs to one group.  Segments are sorted, disjoint, and
 * begin and end on multiples of 8 elements.  No host copy of the table is taken: the launch arguments depend on n alone, so a
 * captured launch follows the table it was given.  An access that the table would place outside [0, n) is skipped, and so is
 * a segment whose group_s lies outside [0, n_groups): a malformed table touches nothing.
 *
 * The hyper-parameters are a HOST array of n_groups records of FBL_ADAM_GROUP_FLOATS floats,
 *     {lr, beta1, beta2, eps, weight_decay, decoupled (0 or 1)},
 * copied into the launch's argument block during the call together with the bias corrections of `step`
 * (1 - beta^step, per group): still no allocation and no copy to the device.
 */
#ifndef FBL_GROUPS_H
#define FBL_GROUPS_H
#include "fbl.h"
#ifdef __cplusplus
extern "C" {
#endif

#define FBL_ADAM_MAX_GROUPS 64
#define FBL_ADAM_GROUP_FLOATS 6

/* One Adam step on the segments of p / g / m / v fp32 [n], each with the hyper-parameters of its group.
 *   coupled group (decoupled == 0): fbl_adam_flat's arithmetic in the same order -- with the same hyper-parameters the bits
 *     of fbl_adam_flat / fbl_adam_flat_live;
 *   decoupled group: p <- p * (1 - lr * weight_decay), then the Adam update with no decay term in the gradient
 *     (torch.optim.AdamW).
 * The clip factor comes from the ONE device norm `sumsq` over all live elements of all groups (fbl_sumsq / fbl_sumsq_live;
 * NULL or max_norm <= 0: no clip).  Words outside the segments are neither read into a result nor written.  One launch.
 * NULL p / g / m / v / segs / hyper or n_groups outside 1 .. FBL_ADAM_MAX_GROUPS: FBL_ERR_ARG; n % 8 != 0 or a pointer that is
 * not 16-byte aligned: FBL_ERR_ALIGN; then n <= 0: 0, nothing launched. */
int fbl_adam_flat_groups(float* p, const float* g, float* m, float* v, int64_t n, const int64_t* segs, int n_groups,
                         const float* hyper, int step, const float* sumsq, float max_norm, float grad_scale, void* stream);

#ifdef __cplusplus
}
#endif
#endif
