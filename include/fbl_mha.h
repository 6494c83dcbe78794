/* libfbl -- fused multi-head attention of the BERT variant (MI355X, gfx950).  Same library, same conventions as fbl.h:
 * extern "C", plain device pointers + sizes, `stream` a hipStream_t passed as void*, every function only enqueues work
 * (graph-capturable, no allocation / copy / sync inside), returns 0, a positive hipError_t or a negative FBL_ERR_* code.
 * Dropout seeds as in fbl.h ("Dropout seeds").  Bound from Python by frozenbilm_amd/lib.py MHA_SIGNATURES, derived from this header.
 */
#ifndef FBL_MHA_H
#define FBL_MHA_H
#include "fbl.h"
#ifdef __cplusplus
extern "C" {
#endif

/* Plain scaled-dot-product attention with an additive key mask, head_dim 64, S <= 512, any number of heads:
 *   score[i,j] = scale * Q_i.K_j + (mask[b,j] != 0 ? 0 : -10000)   (fp32),   ctx = dropout(softmax_j(score)) . V
 *   Every query row is computed, padded ones included (the mask is on keys only).  A sample without any valid key
 *   softmaxes over all of its keys, as the reference does.
 *   q/k/v: bf16 rows b*S+s, head h at column h*64, row strides ldq/ldk/ldv (multiples of 8: e.g. 3H inside a fused QKV
 *   buffer); mask int32 [B,S]; klen int32 [B] (optional): last valid key + 1 -- key tiles at or beyond it are skipped
 *   (exp underflows to exactly 0 there; klen[b] = 0 means "no valid key": all keys are visited); border int32 [B]
 *   (optional): the order in which the samples are dispatched (longest first), results do not depend on it.
 *   Attention-probability dropout p_drop in [0, 1): the counter hash of attn_common.h (two keys per (seed, b*nh + h), one
 *   32-bit hash per 2x2 block of (query, key) pairs, Sp = S rounded up to 64), as fbl_disent_attn_fwd draws it.
 *   out ctx bf16 [B*S, ldo] (head h at column h*64); lse fp32 [B,nh,S] (natural-log log-sum-exp of the row's scores).
 * ref: model/bert.py:138-191 (BertSelfAttention.forward, dropout of the probabilities :176),
 *      :640-642 (get_extended_attention_mask: (1 - mask) * -10000). */
int fbl_mha_fwd(const void* q, int64_t ldq, const void* k, int64_t ldk, const void* v, int64_t ldv, const int32_t* mask,
                const int32_t* klen, const int32_t* border, float scale, float p_drop, uint64_t seed, const uint64_t* seed_dev,
                void* ctx, int64_t ldo, float* lse, int B, int S, int nh, void* stream);

/* Backward of fbl_mha_fwd: dQ, dK, dV (bf16 rows like q/k/v, strides lddq/lddk/lddv, every row < S written).
 *   Inputs as in the forward (same mask / klen / p_drop / seed / seed_dev: the dropout decisions are regenerated), plus
 *   dO bf16 rows (stride lddo), the forward's lse and Dv fp32 [B,nh,S] = rowdot(dO, ctx) from fbl_attn_rowdot.
 *   Two launches: a key-major pass (dK, dV kept in registers over the query tiles) and a query-major pass (dQ over the key
 *   tiles); both recompute P from lse.  No atomics: the result is the same bit for bit on every run.
 * ref: autograd of model/bert.py:138-191 (softmax, dropout, the two matrix products). */
int fbl_mha_bwd(const void* q, int64_t ldq, const void* k, int64_t ldk, const void* v, int64_t ldv, const void* dO,
                int64_t lddo, const int32_t* mask, const int32_t* klen, const int32_t* border, const float* lse,
                const float* Dv, float scale, float p_drop, uint64_t seed, const uint64_t* seed_dev, void* dQ, int64_t lddq,
                void* dK, int64_t lddk, void* dV, int64_t lddv, int B, int S, int nh, void* stream);

/* fbl_mha_fwd / fbl_mha_bwd on PACKED ROWS: the activation rows of a ragged batch without its trailing padding.
 *   row0 int32 [B+1] (required): sample b owns the rows [row0[b], row0[b+1]) of q / k / v / ctx / dO / O / dQ / dK / dV -- its
 *   positions 0 .. plen[b]-1, plen[b] = row0[b+1] - row0[b] <= S.  klen is required, and plen[b] >= klen[b].  mask, lse and
 *   Dv keep their padded [B,S] / [B,nh,S] indexing.  Rows a sample does not have are neither read nor written: loads clamp
 *   to the sample's last row, keys j >= plen[b] get a -inf bias, query and key tiles wholly beyond plen[b] do nothing, and
 *   lse / Dv are written at positions < plen[b] only.
 *   A sample with klen[b] == 0 has no valid key and softmaxes over all S keys (as the reference does): the caller must give
 *   such a sample plen[b] = S.  (Given less, it softmaxes over the keys it has.)
 *   The rows that exist get exactly the values of the padded call on the same data, bit for bit: keys in [klen, plen) carry
 *   the -10000 bias in both layouts, keys in [plen, S) underflow to exactly 0 there and are exactly 0 here, and the key-tile
 *   order is the same.  For dK / dV this holds when dO is zero at the padded call's rows in [plen, S) -- rows nothing reads
 *   receive exactly that gradient -- because such a query row then adds exact zeros (D = 0, dS = 0, dO^T.P = 0).
 *   Dropout is keyed by (b*nh + h, query position, key position) with Sp from S: the decisions of the padded call.
 *   fbl_mha_bwd_rows takes the forward's output O (= ctx, stride ldo, a multiple of 8) instead of Dv as an input and writes
 *   Dv fp32 [B,nh,S] = rowdot(dO, O) itself for the rows that exist (the arithmetic of fbl_attn_rowdot) in a first
 *   launch, then runs the key-major and the query-major pass: three launches, enqueue-only. */
int fbl_mha_fwd_rows(const void* q, int64_t ldq, const void* k, int64_t ldk, const void* v, int64_t ldv, const int32_t* mask,
                     const int32_t* klen, const int32_t* border, const int32_t* row0, float scale, float p_drop, uint64_t seed,
                     const uint64_t* seed_dev, void* ctx, int64_t ldo, float* lse, int B, int S, int nh, void* stream);

int fbl_mha_bwd_rows(const void* q, int64_t ldq, const void* k, int64_t ldk, const void* v, int64_t ldv, const void* dO,
                     int64_t lddo, const void* O, int64_t ldo, const int32_t* mask, const int32_t* klen, const int32_t* border,
                     const int32_t* row0, const float* lse, float* Dv, float scale, float p_drop, uint64_t seed,
                     const uint64_t* seed_dev, void* dQ, int64_t lddq, void* dK, int64_t lddk, void* dV, int64_t lddv, int B, int S,
                     int nh, void* stream);

#ifdef __cplusplus
}
#endif
#endif
