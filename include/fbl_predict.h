/* libfbl -- what the model PREDICTS on a set of rows (MI355X, gfx950): top-k ids and log-probabilities, the rank of the label
 * and the per-row negative log-likelihood, from the fp32 logits of those rows, without any [R, V] result leaving the device.
 * Same library, same conventions as fbl.h: extern "C", plain device pointers + sizes, `stream` a hipStream_t passed as
 * void*, every function only enqueues work (no allocation / copy / sync inside), returns 0, a positive hipError_t or a
 * negative FBL_ERR_* code.  Bound from Python by frozenbilm_amd/lib.py PREDICT_SIGNATURES, derived from this header.
 *
 * The ORDER of a row's columns is total: descending by value; equal values (+0 and -0 are equal) ascending by column; -inf is
 * an ordinary, smallest value; a NaN orders below -inf (NaNs among themselves ascending by column).
 */
#ifndef FBL_PREDICT_H
#define FBL_PREDICT_H
#include "fbl.h"
#ifdef __cplusplus
extern "C" {
#endif

#define FBL_PREDICT_MAX_K 16
#define FBL_PREDICT_CHUNK 8192 /* columns one workgroup of the first launch reads (a constant: results do not depend on R) */

/* Bytes of workspace fbl_row_predict needs for R rows of V columns and k slots (the per-chunk candidates); 0 for R <= 0,
 * negative FBL_ERR_* for a bad V / k. */
int64_t fbl_row_predict_ws_bytes(int R, int V, int k);

/* logits fp32 [R, ldv]: columns 0 .. V-1 are valid, columns V .. ldv-1 may hold anything (they are loaded, never used).
 * Per row r:
 *   topk_ids int32 [R, k], topk_logprob fp32 [R, k]: the first k columns in the order above and logit - lse; for k > V the
 *   trailing slots hold id -1 and logprob -inf;
 *   lse = row_lse[r] when row_lse (fp32 [R], e.g. what fbl_ce_fwd wrote) is given, else log(sum_j exp(x_j)) of the same pass;
 *   with labels (int64 [R], every entry in [0, V)): label_rank int32 [R] = #{j : x_j > x_l} + #{j < l : x_j == x_l}
 *   (comparisons with a NaN are false) and row_nll fp32 [R] = lse - x_l; without labels both must be NULL.
 * Two launches: R x (chunks of FBL_PREDICT_CHUNK columns) workgroups read every logit once with 16-byte loads and leave k
 * candidates, a partial (max, sum exp) and a partial rank per chunk in ws; one wave per row merges the chunks in their
 * order.  No atomics: identical calls give identical bits.  ws: fbl_row_predict_ws_bytes(R, V, k) bytes, 8-byte aligned.
 * 1 <= k <= FBL_PREDICT_MAX_K, V >= 1, ldv >= V and ldv % 4 == 0, logits 16-byte aligned.  R = 0: nothing is launched. */
int fbl_row_predict(const float* logits, int64_t ldv, int R, int V, int k, const int64_t* labels, const float* row_lse,
                    int32_t* topk_ids, float* topk_logprob, int32_t* label_rank, float* row_nll, void* ws, int64_t ws_bytes,
                    void* stream);

#ifdef __cplusplus
}
#endif
#endif
