// Deep prompt tuning (include/fbl_prompt_layers.h): the prompt slots' rows of a layer's materialised input overwritten with that
// layer's parameter, and the parameter's gradient as an ordered sum over the batch that clears the rows it read.  Row copies /
// row adds of B.P.H floats -- bandwidth-trivial; what matters is that they are exact (copies, one rounding to bf16) and
// reproducible (fp32 adds in ascending b, one owner per element, no atomics).
#include "fbl_common.h"
#include "../../include/fbl_prompt_layers.h"

namespace {

// one workgroup per (sample b, prompt row p)
__global__ __launch_bounds__(128) void prompt_rows_write_kernel(const float* prompt, const int32_t* row0, int S, int T, int P,
                                                                int H, float* out_f32, bf16* out_bf16) {
  const int b = blockIdx.x / P, p = blockIdx.x % P;
  const long r = (row0 ? (long)row0[b] : (long)b * S) + T + p;
  const float* src = prompt + (long)p * H;
  for (int c = threadIdx.x * 4; c < H; c += blockDim.x * 4) {
    const f32x4 x = *(const f32x4*)(src + c);
    if (out_f32) *(f32x4*)(out_f32 + r * H + c) = x;
    if (out_bf16) {
      bf16x4 y;
#pragma unroll
      for (int j = 0; j < 4; ++j) y[j] = f2bf(x[j]);
      *(bf16x4*)(out_bf16 + r * H + c) = y;
    }
  }
}

// thread = (prompt row p, 4 columns): acc = g; acc += dx[row(b) + T + p] for b = 0 .. B-1, in that order; then the same pieces of
// dx are cleared
__global__ __launch_bounds__(256) void prompt_rows_grad_kernel(float* dx, const int32_t* row0, int B, int S, int T, int P, int H,
                                                               float* g) {
  const int h4 = H / 4;
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= P * h4) return;
  const int p = idx / h4, c = (idx % h4) * 4;
  if (g) {
    float* gp = g + (long)p * H + c;
    f32x4 acc = *(const f32x4*)gp;
#pragma unroll 8
    for (int b = 0; b < B; ++b) {
      const long r = (row0 ? (long)row0[b] : (long)b * S) + T + p;
      const f32x4 x = *(const f32x4*)(dx + r * H + c);
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[j] = acc[j] + x[j];
    }
    *(f32x4*)gp = acc;
  }
  const f32x4 zero = {0.0f, 0.0f, 0.0f, 0.0f};
  for (int b = 0; b < B; ++b) {
    const long r = (row0 ? (long)row0[b] : (long)b * S) + T + p;
    *(f32x4*)(dx + r * H + c) = zero;
  }
}

inline bool misaligned(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) != 0; }

}  // namespace

extern "C" int fbl_prompt_rows_write(const float* prompt, const int32_t* row0, int B, int S, int T, int P, int H, float* out_f32,
                                     void* out_bf16, void* stream) {
  if (H <= 0 || (H % 4)) return FBL_ERR_SHAPE;
  if (P < 1 || P > FBL_PROMPT_MAX) return FBL_ERR_ARG;
  if (!prompt || (!out_f32 && !out_bf16) || B < 0 || T < 0) return FBL_ERR_ARG;
  if (!row0 && (int64_t)S < (int64_t)T + P) return FBL_ERR_SHAPE;
  if ((int64_t)B * P > 0x7FFFFFFF) return FBL_ERR_SHAPE;
  if (misaligned(prompt, 16) || misaligned(out_f32, 16) || misaligned(out_bf16, 8) || misaligned(row0, 4)) return FBL_ERR_ALIGN;
  if (B == 0) return 0;
  hipLaunchKernelGGL(prompt_rows_write_kernel, dim3((unsigned)(B * P)), dim3(128), 0, (hipStream_t)stream, prompt, row0, S, T, P,
                     H, out_f32, (bf16*)out_bf16);
  FBL_CHECK_LAUNCH();
  return 0;
}

extern "C" int fbl_prompt_rows_grad(float* dx, const int32_t* row0, int B, int S, int T, int P, int H, float* g, void* stream) {
  if (H <= 0 || (H % 4)) return FBL_ERR_SHAPE;
  if (P < 1 || P > FBL_PROMPT_MAX) return FBL_ERR_ARG;
  if (!dx || B < 0 || T < 0) return FBL_ERR_ARG;
  if (!row0 && (int64_t)S < (int64_t)T + P) return FBL_ERR_SHAPE;
  if (misaligned(dx, 16) || misaligned(g, 16) || misaligned(row0, 4)) return FBL_ERR_ALIGN;
  if (B == 0) return 0;
  const int64_t n = (int64_t)P * (H / 4);
  if (n > 0x7FFFFFFF) return FBL_ERR_SHAPE;
  hipLaunchKernelGGL(prompt_rows_grad_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, dx, row0, B, S,
                     T, P, H, g);
  FBL_CHECK_LAUNCH();
  return 0;
}
