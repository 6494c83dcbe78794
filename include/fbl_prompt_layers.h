/* libfbl -- deep prompt tuning: trainable prompt rows at the input of encoder layers 1 .. D-1 (MI355X, gfx950).  The rows of a
 * sample are [video slots T | prompt slots P | text L] (include/fbl_prompt.h); layer i >= 1 with a prompt of its own reads its
 * fp32 [P, H] parameter in the prompt slots of its input instead of what the layer below left there.  Two row kernels over
 * B.P.H elements: the forward overwrites the slots' rows of a materialised hidden stream (fp32 and / or its bf16 operand copy),
 * the backward sums the slots' rows of the stream's gradient over the batch and clears them, so that nothing upstream of the
 * overwrite receives a gradient from them.  Same library, same conventions as fbl.h and fbl_prompt.h: extern "C", plain device
 * pointers + sizes, `stream` a hipStream_t passed as void*, the function only enqueues work (no allocation / copy / sync
 * inside), returns 0, a positive hipError_t or a negative FBL_ERR_* code.  r(b) = row0[b] (int32 [B]: the first activation row
 * of sample b on packed or compact rows) or, with row0 == NULL, b * S (the padded grid).  The caller guarantees that the rows
 * r(b) + T .. r(b) + T + P - 1 of every sample lie inside the buffers (on the padded grid: S >= T + P, checked here).  Bound
 * from Python by frozenbilm_amd/lib.py PROMPT_LAYERS_SIGNATURES, derived from this header.
 */
#ifndef FBL_PROMPT_LAYERS_H
#define FBL_PROMPT_LAYERS_H
#include "fbl_prompt.h"
#ifdef __cplusplus
extern "C" {
#endif

/* out_f32[r(b) + T + p, :] = prompt[p, :]            the fp32 bits, copied in 16-byte pieces
 * out_bf16[r(b) + T + p, :] = bf16(prompt[p, :])     round to nearest even, stored in 8-byte pieces
 * for every sample b and prompt row p; prompt fp32 [P, H], out_f32 fp32 [rows, H], out_bf16 bf16 [rows, H] (all contiguous).
 * Either output may be NULL (not both).  No other row is touched.  One workgroup per (b, p).
 * H not a positive multiple of 4: FBL_ERR_SHAPE.  P outside 1 .. FBL_PROMPT_MAX, a NULL prompt, both outputs NULL, a negative
 * B / T: FBL_ERR_ARG.  row0 == NULL and S < T + P, or more than 2^31 - 1 (b, p) pairs: FBL_ERR_SHAPE.  prompt or out_f32 not
 * 16-byte aligned, out_bf16 not 8-byte aligned, row0 not 4-byte aligned: FBL_ERR_ALIGN.  Checked in this order, before any
 * launch.  B == 0: 0, nothing launched. */
int fbl_prompt_rows_write(const float* prompt, const int32_t* row0, int B, int S, int T, int P, int H, float* out_f32,
                          void* out_bf16, void* stream);

/* g[p, c] += sum_b dx[r(b) + T + p, c], then dx[r(b) + T + p, :] = 0 for every b      g fp32 [P, H], dx fp32 [rows, H]
 * dx holds the gradient of a hidden stream whose prompt slots fbl_prompt_rows_write overwrote.  The sum is formed as plain fp32
 * adds in ascending b starting from the value already in g: no atomics, no tree -- identical calls give identical bits, and a
 * host loop `acc = g; for b: acc += dx[r(b) + T + p]` reproduces them.  One thread owns 4 consecutive columns of one prompt row
 * (16-byte accesses) and, after its sum, stores zeros to the pieces it read: no other row of dx is touched.  g may be NULL (a
 * frozen prompt): nothing is summed, the slots' rows are cleared all the same.
 * H not a positive multiple of 4: FBL_ERR_SHAPE.  P outside 1 .. FBL_PROMPT_MAX, a NULL dx, a negative B / T: FBL_ERR_ARG.
 * row0 == NULL and S < T + P: FBL_ERR_SHAPE.  dx or g not 16-byte aligned, row0 not 4-byte aligned: FBL_ERR_ALIGN.  Checked in
 * this order, before any launch.  B == 0: 0, nothing launched (g and dx keep their values). */
int fbl_prompt_rows_grad(float* dx, const int32_t* row0, int B, int S, int T, int P, int H, float* g, void* stream);

#ifdef __cplusplus
}
#endif
#endif
