// LoRA merged into the packed operands: W' = W + s . B . A for every site of a device table in one launch
// (include/fbl_lora.h).  W fp32 [O, I], A fp32 [r, I], B fp32 [O, r], r <= 64: 2 r flops per element against 4 bytes read and
// 4 (+ 4) written -- memory-bound, no matrix cores.  A workgroup owns one 64 x 64 tile of one site: the r x 64 slice of A
// and the 64 x r slice of B are staged in LDS (16 KiB each at r = 64), a thread forms 2 x 8 consecutive elements of a row
// (fp32 fused multiply-adds in ascending k), rounds them once to bf16 and stores them with one 16-byte store into the
// row-major destination; the same bf16 values are written transposed into LDS and leave as 16-byte stores along the rows
// of the transposed destination -- both destinations are written coalesced and hold identical bits.
#include "fbl_common.h"
#include "../../include/fbl_lora.h"

namespace {

constexpr int LT = 64;        // tile edge
constexpr int LDT = LT + 8;   // bf16 row stride of the transposed tile in LDS (144 bytes: rows stay 16-byte aligned)
constexpr int SW = FBL_LORA_SITE_WORDS;

__global__ __launch_bounds__(256) void lora_compose_kernel(const int64_t* sites) {
  const int64_t* st = sites + (long)blockIdx.y * SW;
  const int O = (int)st[10], I = (int)st[11], r = (int)st[12];
  const int tiles_i = I / LT;
  const int n_tiles = (O / LT) * tiles_i;
  if ((int)blockIdx.x >= n_tiles) return;  // (the grid's x extent is the largest site's tile count)
  const float* W = (const float*)st[0];
  const long ldw = st[1];
  const float* A = (const float*)st[2];
  const float* B = (const float*)st[3];
  bf16* dst = (bf16*)st[4];
  const long ld_dst = st[5];
  bf16* dstT = (bf16*)st[6];
  const long ld_dstT = st[7];
  float* dst32 = (float*)st[8];
  const long ld32 = st[9];
  const float s = __uint_as_float((uint32_t)st[13]);
  const int o0 = ((int)blockIdx.x / tiles_i) * LT, i0 = ((int)blockIdx.x % tiles_i) * LT;

  __shared__ __attribute__((aligned(16))) float sA[FBL_LORA_MAX_RANK * LT];  // [k][64 columns of this tile]
  __shared__ float sB[LT * FBL_LORA_MAX_RANK];                                // [64 rows of this tile][r], packed
  __shared__ __attribute__((aligned(16))) bf16 sT[LT * LDT];                  // [i][o]: the tile, transposed
  const int tid = threadIdx.x;
  for (int idx = tid; idx < r * (LT / 4); idx += 256) {
    const int k = idx / (LT / 4), c4 = idx % (LT / 4);
    *(f32x4*)&sA[k * LT + c4 * 4] = *(const f32x4*)(A + (long)k * I + i0 + c4 * 4);
  }
  for (int idx = tid; idx < LT * r; idx += 256) sB[idx] = B[(long)o0 * r + idx];  // rows o0 .. o0+63 of B are contiguous
  __syncthreads();

  const int cg = tid & 7, row = tid >> 3;  // 8 threads x 8 columns per row, 32 rows per pass
#pragma unroll
  for (int p = 0; p < 2; ++p) {
    const int o = row + 32 * p;
    float acc[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] = 0.f;
    for (int k = 0; k < r; ++k) {
      const float b = sB[o * r + k];
      const f32x4 a0 = *(const f32x4*)&sA[k * LT + cg * 8], a1 = *(const f32x4*)&sA[k * LT + cg * 8 + 4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        acc[j] = __builtin_fmaf(b, a0[j], acc[j]);
        acc[4 + j] = __builtin_fmaf(b, a1[j], acc[4 + j]);
      }
    }
    const float* wp = W + (long)(o0 + o) * ldw + i0 + cg * 8;
    const f32x4 w0 = *(const f32x4*)wp, w1 = *(const f32x4*)(wp + 4);
    f32x4 v0, v1;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      v0[j] = __builtin_fmaf(s, acc[j], w0[j]);
      v1[j] = __builtin_fmaf(s, acc[4 + j], w1[j]);
    }
    bf16x8 vb;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      vb[j] = f2bf(v0[j]);
      vb[4 + j] = f2bf(v1[j]);
    }
    *(bf16x8*)(dst + (long)(o0 + o) * ld_dst + i0 + cg * 8) = vb;
    if (dst32) {
      float* dp = dst32 + (long)(o0 + o) * ld32 + i0 + cg * 8;
      *(f32x4*)dp = v0;
      *(f32x4*)(dp + 4) = v1;
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) sT[(cg * 8 + j) * LDT + o] = vb[j];
  }
  __syncthreads();
#pragma unroll
  for (int p = 0; p < 2; ++p) {
    const int i = row + 32 * p;  // a row of the transposed tile: 8 threads x 8 consecutive o
    *(bf16x8*)(dstT + (long)(i0 + i) * ld_dstT + o0 + cg * 8) = *(const bf16x8*)&sT[i * LDT + cg * 8];
  }
}

}  // namespace

extern "C" int fbl_lora_compose(const int64_t* sites_host, const int64_t* sites_dev, int n_sites, void* stream) {
  if (n_sites < 0 || n_sites > FBL_LORA_MAX_SITES) return FBL_ERR_ARG;
  if (n_sites == 0) return 0;
  if (!sites_host || !sites_dev) return FBL_ERR_ARG;
  int64_t max_tiles = 0;
  for (int n = 0; n < n_sites; ++n) {
    const int64_t* st = sites_host + (long)n * SW;
    const int64_t ldw = st[1], ld_dst = st[5], ld_dstT = st[7], ld32 = st[9], O = st[10], I = st[11], r = st[12];
    if (!st[0] || !st[2] || !st[3] || !st[4] || !st[6]) return FBL_ERR_ARG;
    if (r < 1 || r > FBL_LORA_MAX_RANK) return FBL_ERR_ARG;
    if (O < LT || I < LT || (O % LT) || (I % LT) || O > (1 << 20) || I > (1 << 20)) return FBL_ERR_SHAPE;
    if (ldw < I || ld_dst < I || ld_dstT < O || (st[8] && ld32 < I)) return FBL_ERR_SHAPE;
    if ((ldw & 3) || (ld_dst & 7) || (ld_dstT & 7) || (st[8] && (ld32 & 3))) return FBL_ERR_ALIGN;
    if (((st[0] | st[2] | st[4] | st[6] | st[8]) & 15) || (st[3] & 3)) return FBL_ERR_ALIGN;
    const int64_t tiles = (O / LT) * (I / LT);
    if (tiles > max_tiles) max_tiles = tiles;
  }
  if (max_tiles > 0x7FFFFFFF) return FBL_ERR_SHAPE;
  hipLaunchKernelGGL(lora_compose_kernel, dim3((unsigned)max_tiles, (unsigned)n_sites), dim3(256), 0, (hipStream_t)stream,
                     sites_dev);
  FBL_CHECK_LAUNCH();
  return 0;
}
