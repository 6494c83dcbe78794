/* libfbl -- disentangled self-attention on SELECTED QUERY ROWS (MI355X, gfx950): the attention of the enhanced mask decoder
 * when only a few token rows reach the prediction head.  Same library, same conventions as fbl.h: extern "C", plain device
 * pointers + sizes, `stream` a hipStream_t passed as void*, every function only enqueues work (no allocation / copy / sync
 * inside), returns 0, a positive hipError_t or a negative FBL_ERR_* code.  Dropout seeds as in fbl.h ("Dropout seeds").
 * Bound from Python by frozenbilm_amd/lib.py QROWS_SIGNATURES, derived from this header.
 */
#ifndef FBL_QROWS_H
#define FBL_QROWS_H
#include "fbl.h"
#ifdef __cplusplus
extern "C" {
#endif

/* fbl_disent_attn_fwd whose query rows are a gathered subset, while keys and values are all rows of the sample:
 *   q bf16 [R, ldq]: the COMPACT query rows, grouped by sample -- sample b owns the rows [rseg[b], rseg[b+1]) (rseg int32
 *   [B+1], rseg[0] = 0, rseg[B] = R, non-decreasing); rpos int32 [R]: the position of the row inside its sample, in [0, S)
 *   (any order, duplicates allowed);
 *   k / v bf16: every key row of the layout -- row b*S + s, or packed through row0 int32 [B+1] as in fbl_disent_attn_fwd;
 *   pk / pq bf16 [span2, ldp] (span2 <= 512), relidx int16 [2S-1] (non-decreasing), mask int32 [B,S] (not necessarily a
 *   prefix), klen int32 [B] (required): last valid position + 1.
 *   For compact row r of sample b at position i = rpos[r]:
 *     score[j] = scale*(Q_r.K_j + Q_r.PK[idx(i-j)] + K_j.PQ[idx(i-j)]),  masked by mask[b,i]*mask[b,j], softmax, dropout,
 *     ctx[r] = P.V  -> ctx bf16 [R, ldo];  lse fp32 [nh, R] (+inf for a row without a valid pair, whose ctx is exactly 0).
 *   Attention-probability dropout is keyed as in fbl_disent_attn_fwd -- (seed, b*nh + h, 2x2 block of query POSITION and key
 *   position, Sp = the padded length of the full-grid call, a multiple of 64): a selected row draws exactly the mask the
 *   full-grid kernel draws for it.
 *   head_dim 64, 1 <= S <= 512; strides multiples of 8, pointers 16-byte aligned.  R = 0: nothing is launched.
 * ref: model/deberta.py:717-947 restricted to query rows; :1382-1412 (the enhanced mask decoder, whose two passes take
 *      their keys and values from the same hidden states). */
int fbl_disent_attn_fwd_qrows(const void* q, int64_t ldq, const int32_t* rseg, const int32_t* rpos, int R, const void* k,
                              int64_t ldk, const void* v, int64_t ldv, const void* pk, const void* pq, int64_t ldp,
                              const int16_t* relidx, const int32_t* mask, const int32_t* klen, const int32_t* row0,
                              float scale, float p_drop, uint64_t seed, const uint64_t* seed_dev, void* ctx, int64_t ldo,
                              float* lse, int B, int S, int Sp, int nh, int span2, void* stream);

/* Bytes of workspace fbl_disent_attn_bwd_qrows needs (dropout(P) and dS of the selected rows, bf16 [nh, R, Sp] each, and
 * eight bytes per row). */
int64_t fbl_disent_attn_bwd_qrows_ws_bytes(int R, int Sp, int nh);

/* Backward of fbl_disent_attn_fwd_qrows (same q .. seed_dev; P is recomputed from the forward's lse, the dropout decisions
 * are regenerated).  dO bf16 [R, lddo], O = the forward's ctx.  Outputs, all fully written (callers hand in uninitialised
 * memory; nothing is accumulated):
 *   dQ bf16 [R, lddq] compact (a masked query row: exactly 0);
 *   dK, dV bf16 for EVERY key row of the layout (strides lddk / lddv): masked keys, keys at or beyond klen and all rows of a
 *   sample without a selected row are exactly 0;
 *   dPK, dPQ fp32 [nh, rcnt, 64]: the gradients of table rows rmin .. rmin + rcnt - 1, summed over samples and rows in a
 *   fixed order -- the layout fbl_attn_pos_grad writes per execution.  Both NULL: the table pass is not launched (rmin, rcnt
 *   are then not read).
 * Three launches (selected rows: dQ, and dropout(P), dS into ws; keys: dK, dV; table rows: dPK, dPQ); no atomics: identical
 * calls give identical bits.
 * R = 0: NOTHING IS LAUNCHED AND NOTHING IS WRITTEN -- dK, dV, dPK and dPQ keep whatever the caller handed in; a caller that
 * adds them into something must skip that for R = 0 (the engine does: no decoder work, the gradient of hs[-2] starts from zero).
 * ref: autograd of model/deberta.py:717-947, XSoftmax.backward :134-138, XDropout.backward :185-190. */
int fbl_disent_attn_bwd_qrows(const void* q, int64_t ldq, const int32_t* rseg, const int32_t* rpos, int R, const void* k,
                              int64_t ldk, const void* v, int64_t ldv, const void* pk, const void* pq, int64_t ldp,
                              const int16_t* relidx, const int32_t* mask, const int32_t* klen, const int32_t* row0,
                              const void* dO, int64_t lddo, const void* O, int64_t ldo, const float* lse, float scale,
                              float p_drop, uint64_t seed, const uint64_t* seed_dev, void* dQ, int64_t lddq, void* dK,
                              int64_t lddk, void* dV, int64_t lddv, float* dPK, float* dPQ, int rmin, int rcnt, void* ws,
                              int64_t ws_bytes, int B, int S, int Sp, int nh, int span2, void* stream);

#ifdef __cplusplus
}
#endif
#endif
