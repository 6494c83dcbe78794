/* libfbl -- prompt tuning: trainable soft-prompt rows between the video slots and the text (MI355X, gfx950).  The embedding
 * rows of a sample are [video slots T | prompt slots P | text L], S = T + P + L; the prompt is ONE fp32 [P, H] parameter shared
 * by every sample.  Two row kernels: the forward assembles the rows in front of the embedding LayerNorm, the backward sums the
 * gradient of the prompt slots over the batch.  Same library, same conventions as fbl.h: extern "C", plain device pointers +
 * sizes, `stream` a hipStream_t passed as void*, the function only enqueues work (no allocation / copy / sync inside), returns
 * 0, a positive hipError_t or a negative FBL_ERR_* code.  Bound from Python by frozenbilm_amd/lib.py PROMPT_SIGNATURES, derived
 * from this header.
 */
#ifndef FBL_PROMPT_H
#define FBL_PROMPT_H
#include "fbl.h"
#ifdef __cplusplus
extern "C" {
#endif

#define FBL_PROMPT_MAX 128

/* out_t fp32 [B, S, H] (contiguous), fp32 row copies in 16-byte pieces, one workgroup per row:
 *     out[b, s] = vproj[b, s]              s < T                 vproj fp32 [B, T, H]
 *     out[b, s] = prompt[s - T]            T <= s < T + P        prompt fp32 [P, H]
 *     out[b, s] = E[ids[b, s - T - P]]     T + P <= s            ids int64 [B, L], E fp32 [V, H]
 * ids may be NULL: the text rows are then left untouched (the caller copies its own embeddings there) and E is not read.
 * vproj may be NULL when T == 0.
 * H not a positive multiple of 4: FBL_ERR_SHAPE.  P outside 1 .. FBL_PROMPT_MAX, a NULL prompt or out_t, a NULL E next to ids,
 * a negative B / T / L: FBL_ERR_ARG.  More than 2^31 - 1 rows: FBL_ERR_SHAPE.  prompt, out_t, E or vproj not 16-byte aligned,
 * ids not 8-byte aligned: FBL_ERR_ALIGN.  T > 0 with a NULL vproj: FBL_ERR_ARG.  Checked in this order, before any launch.  An
 * empty grid (B == 0): 0, nothing launched. */
int fbl_embed_assemble(const int64_t* ids, const float* E, const float* vproj, const float* prompt, int B, int T, int P, int L,
                       int H, float* out_t, void* stream);

/* g[p, c] += sum_b dt[r(b) + T + p, c]     g fp32 [P, H] (contiguous), dt fp32 [rows, H] (contiguous)
 * dt holds the gradient of the embedding rows in front of the embedding LayerNorm; r(b) = row0[b] (int32 [B]: the first
 * activation row of sample b on packed rows) or, with row0 == NULL, b * S (the padded grid).  The sum is formed as plain fp32
 * adds in ascending b starting from the value already in g: no atomics, no tree -- identical calls give identical bits, and a
 * host loop `acc = g; for b: acc += dt[r(b) + T + p]` reproduces them.  One thread owns 4 consecutive columns of one prompt
 * row (16-byte accesses).
 * H not a positive multiple of 4: FBL_ERR_SHAPE.  P outside 1 .. FBL_PROMPT_MAX, a NULL dt or g, a negative B / T:
 * FBL_ERR_ARG.  row0 == NULL and S < T + P: FBL_ERR_SHAPE.  dt or g not 16-byte aligned, row0 not 4-byte aligned:
 * FBL_ERR_ALIGN.  Checked in this order, before any launch.  B == 0: 0, nothing launched (g keeps its value). */
int fbl_prompt_grad(const float* dt, const int32_t* row0, int B, int S, int T, int P, int H, float* g, void* stream);

#ifdef __cplusplus
}
#endif
#endif
