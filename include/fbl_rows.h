/* libfbl -- a compact row layout for the backward pass (MI355X, gfx950).  The forward of a ragged batch runs on the padded
 * [B, S] grid (N_pad = B*S rows); the gradient of every padding row is exactly zero, so the backward may run its row-wise
 * kernels on the Np rows that exist.  Three maps describe the layout: sel int32 [Np] (padded row of each compact row,
 * ascending), inv int32 [N_pad] (compact row of each padded row, -1 where it has none) and the row0 [B+1] of fbl.h for the
 * attention kernels.  Same library, same conventions as fbl.h: extern "C", plain device pointers + sizes, `stream` a hipStream_t
 * passed as void*, the function only enqueues work (no allocation / copy / sync inside), returns 0, a positive hipError_t or a
 * negative FBL_ERR_* code.  Bound from Python by frozenbilm_amd/lib.py ROWS_SIGNATURES, derived from this header.
 */
#ifndef FBL_ROWS_H
#define FBL_ROWS_H
#include "fbl.h"
#ifdef __cplusplus
extern "C" {
#endif

#define FBL_GATHER_MAX_TENSORS 8

/* fbl_ln_bwd of fbl.h with the gradient on compact rows.  The kernel walks the N_pad PADDED rows with the grid, the row -> block
 * assignment, the workspace and the fold of fbl_ln_bwd, so dgamma / dbeta / dysum receive the bits fbl_ln_bwd gives for the padded
 * dout whose rows without a compact row are zero (such a row adds +-0 to partial sums that start at +0).  For a padded row r
 * with c = inv[r] >= 0: dout is read at row c, t / stats / rowmask at row r, the dropout mask is keyed by r (as in the forward);
 * out_dt (fp32 [Np, H], may be NULL) and out_dy_bf16 (bf16, row stride ld_dy_bf16 elements, 0 = H, may be NULL) are written at
 * row c, out_dy_pad_bf16 (bf16 [N_pad, H] contiguous, required) at row r.  For inv[r] < 0 nothing is loaded and row r of
 * out_dy_pad_bf16 is set to zero.  inv must map onto distinct rows inside the compact buffers.
 * H % 64 != 0, H > 2048 or H/64 not in {1, 2, 4, 8, 12, 16, 24, 32} (as fbl_ln_bwd): FBL_ERR_SHAPE.  A NULL dout, inv, t, stats, gamma, ws
 * or out_dy_pad_bf16: FBL_ERR_ARG.  ld_dy_bf16 < H or not a multiple of 8: FBL_ERR_ALIGN.  N_pad <= 0: 0, nothing launched. */
int fbl_ln_bwd_rows(const float* dout, const int32_t* inv, const int32_t* rowmask, const float* t, const float* stats,
                    const float* gamma, float p_drop, uint64_t seed, const uint64_t* seed_dev, float* out_dt, void* out_dy_bf16,
                    int64_t ld_dy_bf16, void* out_dy_pad_bf16, float* dgamma, float* dbeta, float* dysum, float* ws, int N_pad,
                    int H, void* stream);

/* One launch copies the rows sel[0 .. Np) of n row-major tensors into compact buffers:
 *     dst[i][c, :] = src[i][sel[c], :]      row_bytes[i] bytes per row, src row stride src_ld[i] bytes, dst row stride dst_ld[i]
 * src / dst / row_bytes / src_ld / dst_ld are HOST arrays of n entries.  A tensor whose pointers, strides and row_bytes are all
 * multiples of 16 is copied in 16-byte pieces, any other in 4-byte pieces; no LDS.  One workgroup per compact row.
 * n outside 1 .. FBL_GATHER_MAX_TENSORS, a NULL table, pointer or sel, a stride smaller than its row: FBL_ERR_ARG.  row_bytes,
 * a stride or a pointer not a multiple of 4: FBL_ERR_ALIGN.  Np <= 0: 0, nothing launched.  The rows sel names must exist in
 * every source (not checked). */
int fbl_gather_rows_multi(int n, const void* const* src, void* const* dst, const int64_t* row_bytes, const int64_t* src_ld,
                          const int64_t* dst_ld, const int32_t* sel, int Np, void* stream);

/* dst[r, 0 .. cols) = inv[r] >= 0 ? src[inv[r], 0 .. cols) : 0      for the N_pad rows of dst; bf16, row strides in elements.
 * cols, ld_src, ld_dst not multiples of 8 or a pointer not 16-byte aligned: FBL_ERR_ALIGN.  A NULL pointer or a stride
 * smaller than cols: FBL_ERR_ARG.  N_pad <= 0 or cols == 0: 0, nothing launched. */
int fbl_scatter_rows_zero_bf16(const void* src, int64_t ld_src, const int32_t* inv, int N_pad, int cols, void* dst, int64_t ld_dst,
                               void* stream);

#ifdef __cplusplus
}
#endif
#endif
