// Prompt tuning (include/fbl_prompt.h): the embedding rows [video | prompt | text] of every sample in one launch, and the
// prompt's gradient as an ordered sum over the batch.  Both are row copies / row adds of B.P.H floats -- bandwidth-trivial; what
// matters is that they are exact (copies) and reproducible (fp32 adds in ascending b, one owner per element, no atomics).
#include "fbl_common.h"
#include "../../include/fbl_prompt.h"

namespace {

// one workgroup per row; rps rows per sample are written: S = T + P + L, or T + P when there are no ids (text rows untouched)
__global__ __launch_bounds__(128) void embed_assemble_kernel(const int64_t* ids, const float* E, const float* vproj,
                                                             const float* prompt, int T, int P, int L, int H, int rps,
                                                             float* out) {
  const int S = T + P + L;
  const int b = blockIdx.x / rps, s = blockIdx.x % rps;
  const float* src;
  if (s < T)
    src = vproj + ((long)b * T + s) * H;
  else if (s < T + P)
    src = prompt + (long)(s - T) * H;
  else
    src = E + ids[(long)b * L + (s - T - P)] * (long)H;
  float* dst = out + ((long)b * S + s) * H;
  for (int c = threadIdx.x * 4; c < H; c += blockDim.x * 4) *(f32x4*)(dst + c) = *(const f32x4*)(src + c);
}

// thread = (prompt row p, 4 columns): acc = g; acc += dt[row(b) + T + p] for b = 0 .. B-1, in that order
__global__ __launch_bounds__(256) void prompt_grad_kernel(const float* dt, const int32_t* row0, int B, int S, int T, int P,
                                                          int H, float* g) {
  const int h4 = H / 4;
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= P * h4) return;
  const int p = idx / h4, c = (idx % h4) * 4;
  float* gp = g + (long)p * H + c;
  f32x4 acc = *(const f32x4*)gp;
#pragma unroll 8
  for (int b = 0; b < B; ++b) {
    const long r = (row0 ? (long)row0[b] : (long)b * S) + T + p;
    const f32x4 x = *(const f32x4*)(dt + r * H + c);
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[j] = acc[j] + x[j];
  }
  *(f32x4*)gp = acc;
}

inline bool misaligned(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) != 0; }

}  // namespace

extern "C" int fbl_embed_assemble(const int64_t* ids, const float* E, const float* vproj, const float* prompt, int B, int T,
                                  int P, int L, int H, float* out_t, void* stream) {
  if (H <= 0 || (H % 4)) return FBL_ERR_SHAPE;
  if (P < 1 || P > FBL_PROMPT_MAX) return FBL_ERR_ARG;
  if (!prompt || !out_t || (ids && !E) || B < 0 || T < 0 || L < 0) return FBL_ERR_ARG;
  const int64_t rps = ids ? (int64_t)T + P + L : (int64_t)T + P;
  if ((int64_t)B * rps > 0x7FFFFFFF) return FBL_ERR_SHAPE;
  if (misaligned(prompt, 16) || misaligned(out_t, 16) || (ids && misaligned(E, 16)) || misaligned(vproj, 16) ||
      misaligned(ids, 8))
    return FBL_ERR_ALIGN;
  if (T > 0 && !vproj) return FBL_ERR_ARG;
  if (B == 0) return 0;
  hipLaunchKernelGGL(embed_assemble_kernel, dim3((unsigned)(B * rps)), dim3(128), 0, (hipStream_t)stream, ids, E, vproj,
                     prompt, T, P, L, H, (int)rps, out_t);
  FBL_CHECK_LAUNCH();
  return 0;
}

extern "C" int fbl_prompt_grad(const float* dt, const int32_t* row0, int B, int S, int T, int P, int H, float* g,
                               void* stream) {
  if (H <= 0 || (H % 4)) return FBL_ERR_SHAPE;
  if (P < 1 || P > FBL_PROMPT_MAX) return FBL_ERR_ARG;
  if (!dt || !g || B < 0 || T < 0) return FBL_ERR_ARG;
  if (!row0 && (int64_t)S < (int64_t)T + P) return FBL_ERR_SHAPE;
  if (misaligned(dt, 16) || misaligned(g, 16) || misaligned(row0, 4)) return FBL_ERR_ALIGN;
  if (B == 0) return 0;
  const int64_t n = (int64_t)P * (H / 4);
  if (n > 0x7FFFFFFF) return FBL_ERR_SHAPE;
  hipLaunchKernelGGL(prompt_grad_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, dt, row0, B, S,
                     T, P, H, g);
  FBL_CHECK_LAUNCH();
  return 0;
}
