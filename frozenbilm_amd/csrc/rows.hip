// Row moves between the padded [B, S] grid and the compact row layout of the backward pass (include/fbl_rows.h) for gfx950:
// a fused gather of the saved forward operands the compact kernels read, and the zero-filling scatter that gives the adapter
// weight-gradient kernel its padded dz back.  Pure copies: HBM-bound, 16-byte accesses, no LDS.
#include "fbl_common.h"
#include "../../include/fbl_rows.h"

namespace {

typedef __attribute__((ext_vector_type(4))) unsigned int u32x4;

struct GatherArgs {
  const char* src[FBL_GATHER_MAX_TENSORS];
  char* dst[FBL_GATHER_MAX_TENSORS];
  long sld[FBL_GATHER_MAX_TENSORS], dld[FBL_GATHER_MAX_TENSORS];  // row strides, bytes
  int units[FBL_GATHER_MAX_TENSORS];                              // pieces per row (16 or 4 bytes each)
  int v16[FBL_GATHER_MAX_TENSORS];                                // 1: 16-byte pieces
  const int32_t* sel;
  int n;
};

// one row of `n` pieces, the block's 256 threads; up to four loads per thread in flight before the first store
template <typename V>
__device__ __forceinline__ void copy_row(const V* __restrict__ s, V* __restrict__ d, int n) {
  for (int j = threadIdx.x; j < n; j += 4 * 256) {
    V v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u)
      if (j + u * 256 < n) v[u] = s[j + u * 256];
#pragma unroll
    for (int u = 0; u < 4; ++u)
      if (j + u * 256 < n) d[j + u * 256] = v[u];
  }
}

// one workgroup per compact row: row sel[c] of every tensor -> its row c
__global__ __launch_bounds__(256) void gather_rows_multi_kernel(GatherArgs a) {
  const long c = blockIdx.x;
  const long r = a.sel[c];
#pragma unroll
  for (int i = 0; i < FBL_GATHER_MAX_TENSORS; ++i) {
    if (i < a.n) {  // (uniform; the tables are kernel arguments: scalar registers)
      const char* s = a.src[i] + r * a.sld[i];
      char* d = a.dst[i] + c * a.dld[i];
      if (a.v16[i]) copy_row<u32x4>((const u32x4*)s, (u32x4*)d, a.units[i]);
      else copy_row<uint32_t>((const uint32_t*)s, (uint32_t*)d, a.units[i]);
    }
  }
}

// one thread per 16-byte piece of the padded destination
__global__ __launch_bounds__(256) void scatter_rows_zero_bf16_kernel(const bf16* __restrict__ src, long ld_src,
                                                                     const int32_t* __restrict__ inv, long n_units, int upr,
                                                                     bf16* __restrict__ dst, long ld_dst) {
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= n_units) return;
  const long r = idx / upr;
  const int u = (int)(idx - r * upr);
  const int c = inv[r];
  u32x4 v = {0u, 0u, 0u, 0u};
  if (c >= 0) v = *(const u32x4*)(src + (long)c * ld_src + u * 8);
  *(u32x4*)(dst + r * ld_dst + u * 8) = v;
}

}  // namespace

extern "C" int fbl_gather_rows_multi(int n, const void* const* src, void* const* dst, const int64_t* row_bytes,
                                     const int64_t* src_ld, const int64_t* dst_ld, const int32_t* sel, int Np, void* stream) {
  if (n < 1 || n > FBL_GATHER_MAX_TENSORS || !src || !dst || !row_bytes || !src_ld || !dst_ld || !sel) return FBL_ERR_ARG;
  GatherArgs a{};
  for (int i = 0; i < n; ++i) {
    if (!src[i] || !dst[i] || row_bytes[i] <= 0 || src_ld[i] < row_bytes[i] || dst_ld[i] < row_bytes[i]) return FBL_ERR_ARG;
    if (row_bytes[i] > ((int64_t)1 << 30)) return FBL_ERR_ARG;
    const uintptr_t bits = (uintptr_t)src[i] | (uintptr_t)dst[i] | (uintptr_t)row_bytes[i] | (uintptr_t)src_ld[i] | (uintptr_t)dst_ld[i];
    if (bits & 3) return FBL_ERR_ALIGN;
    a.src[i] = (const char*)src[i];
    a.dst[i] = (char*)dst[i];
    a.sld[i] = (long)src_ld[i];
    a.dld[i] = (long)dst_ld[i];
    a.v16[i] = (bits & 15) == 0;
    a.units[i] = (int)(row_bytes[i] / (a.v16[i] ? 16 : 4));
  }
  if (Np <= 0) return 0;
  a.sel = sel;
  a.n = n;
  hipLaunchKernelGGL(gather_rows_multi_kernel, dim3(Np), dim3(256), 0, (hipStream_t)stream, a);
  FBL_CHECK_LAUNCH();
  return 0;
}

extern "C" int fbl_scatter_rows_zero_bf16(const void* src, int64_t ld_src, const int32_t* inv, int N_pad, int cols, void* dst,
                                          int64_t ld_dst, void* stream) {
  if (N_pad <= 0 || cols == 0) return 0;
  if (!src || !inv || !dst || cols < 0 || ld_src < cols || ld_dst < cols) return FBL_ERR_ARG;
  if ((cols % 8) || (ld_src % 8) || (ld_dst % 8) || ((uintptr_t)src & 15) || ((uintptr_t)dst & 15)) return FBL_ERR_ALIGN;
  const int upr = cols / 8;
  const long n_units = (long)N_pad * upr;
  hipLaunchKernelGGL(scatter_rows_zero_bf16_kernel, dim3((unsigned)((n_units + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     (const bf16*)src, (long)ld_src, inv, n_units, upr, (bf16*)dst, (long)ld_dst);
  FBL_CHECK_LAUNCH();
  return 0;
}
