/* libfbl -- low-rank updates (LoRA) of frozen projections, MERGED into the packed bf16 operands (MI355X, gfx950):
 *     W' = W + s . B . A          W fp32 [O, I], A fp32 [r, I], B fp32 [O, r], s a scalar
 * computed in fp32 and rounded once to bf16, for every site of a table in ONE launch.  Same library, same conventions as
 * fbl.h: extern "C", plain device pointers + sizes, `stream` a hipStream_t passed as void*, the function only enqueues work
 * (no allocation / copy / sync inside), returns 0, a positive hipError_t or a negative FBL_ERR_* code.  Bound from Python by
 * frozenbilm_amd/lib.py LORA_SIGNATURES, derived from this header.
 *
 * A site is a record of FBL_LORA_SITE_WORDS int64 words:
 *     [0]  W      const float*, row-major, leading dimension [1] ldw   (elements)
 *     [2]  A      const float*, [r, I] contiguous
 *     [3]  B      const float*, [O, r] contiguous
 *     [4]  dst    bf16*  [O, I] row-major, leading dimension [5] ld_dst          (a row slice of a packed [sum O, I] weight)
 *     [6]  dstT   bf16*  [I, O] row-major, leading dimension [7] ld_dstT         (a column slice of its transposed copy)
 *     [8]  dst32  float* [O, I] row-major, leading dimension [9] ld_dst32, or 0: no fp32 result.  dst32 may be W itself
 *                 (the merge W <- W + s.B.A: every element is read and written by the same thread)
 *     [10] O   [11] I   [12] r   [13] the bits of the float s in the low 32 bits   [14], [15] reserved (0)
 * The table exists twice with the same contents: `sites_host` is validated during the call, `sites_dev` (device memory) is
 * what the kernel reads -- its launch arguments do not depend on the contents, so a captured launch follows the table.
 */
#ifndef FBL_LORA_H
#define FBL_LORA_H
#include "fbl.h"
#ifdef __cplusplus
extern "C" {
#endif

#define FBL_LORA_MAX_RANK 64
#define FBL_LORA_SITE_WORDS 16
#define FBL_LORA_MAX_SITES 4096

/* Per element: acc = sum_k B[o,k] * A[k,i] by fused multiply-adds in ascending k starting from +0, then
 * v = fma(s, acc, W[o,i]) (fp32); dst[o,i] = dstT[i,o] = bf16(v) rounded to nearest even -- the two layouts hold identical
 * bits -- and dst32[o,i] = v.  s = 0 or an all-zero row of B gives exactly bf16(W).  A workgroup owns one 64 x 64 tile; the
 * transposed tile goes through LDS, so both destinations are written in 16-byte pieces.  No atomics: identical calls give
 * identical bits.
 * n_sites = 0: 0, nothing launched.  n_sites outside 0 .. FBL_LORA_MAX_SITES, a NULL table, a NULL W / A / B / dst / dstT or
 * r outside 1 .. FBL_LORA_MAX_RANK: FBL_ERR_ARG.  O or I not a positive multiple of 64, or a leading dimension smaller than
 * its row: FBL_ERR_SHAPE.  ldw or ld_dst32 not a multiple of 4, ld_dst or ld_dstT not a multiple of 8, or W / A / dst / dstT /
 * dst32 not 16-byte aligned (B: 4-byte): FBL_ERR_ALIGN.  Checked in this order per site, before any launch. */
int fbl_lora_compose(const int64_t* sites_host, const int64_t* sites_dev, int n_sites, void* stream);

#ifdef __cplusplus
}
#endif
#endif
