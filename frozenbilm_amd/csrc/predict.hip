// What the model predicts on a set of rows (include/fbl_predict.h): top-k ids / log-probabilities, label rank and per-row
// NLL from fp32 logits [R, ldv], V up to the 128100-wide vocabulary.
//
// Scheme.  The order of the header is the order of one 64-bit key per column: the value's bits mapped to an unsigned word
// that grows with the value (NaN -> 0, below -inf; -0 -> +0) in the upper half, ~column in the lower half.  Keys of distinct
// columns differ, so "the next best column" is "the largest key below the previous winner": no taken-marks, no ties.
//   launch 1, grid (R, chunks of 8192 columns), 256 threads: each thread loads its 8 x 16 bytes up front (every logit is read
//     from HBM once), keeps the 32 values in registers and a cached best key; k rounds of (wave max by shuffles, 4 waves
//     through LDS), after each of which only the thread that owned the winner rescans its registers.  The same registers give
//     the chunk's (max, sum exp) and its share of the label's rank.  Per chunk: k keys, (m, s), one count -> workspace.
//   launch 2, one wave per row: merges the chunks' candidates by the same rule, folds (m, s) in chunk order, adds the counts,
//     turns keys back into (id, logit - lse).
// The chunk width is a constant, so every sum is taken in an order that depends on V alone; no atomics.
#include "fbl_common.h"
#include "../../include/fbl_predict.h"

#include <math.h>

namespace {

constexpr int PT = 256;                    // threads of a chunk workgroup
constexpr int PV = 8;                      // 16-byte loads per thread
constexpr int CHUNK = FBL_PREDICT_CHUNK;   // = PT * PV * 4 columns
static_assert(CHUNK == PT * PV * 4, "chunk width");
typedef unsigned long long u64;

__device__ __forceinline__ uint32_t val_key(float x) {
  if (x != x) return 0u;
  if (x == 0.f) return 0x80000000u;
  const uint32_t b = __float_as_uint(x);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float key_val(uint32_t k) {
  if (k == 0u) return __uint_as_float(0x7FC00000u);
  return (k & 0x80000000u) ? __uint_as_float(k & 0x7FFFFFFFu) : __uint_as_float(~k);
}
__device__ __forceinline__ u64 col_key(float x, int col) { return ((u64)val_key(x) << 32) | (uint32_t)(~(uint32_t)col); }

__device__ __forceinline__ u64 wave_max_u64(u64 v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const u64 w = __shfl_xor(v, o, 64);
    v = w > v ? w : v;
  }
  return v;
}

static inline __host__ __device__ int64_t n_chunks(int V) { return ((int64_t)V + CHUNK - 1) / CHUNK; }

// workspace: keys u64 [R, nch, k] | ms float [R, nch, 2] | cnt int32 [R, nch]
struct Ws {
  u64* keys;
  float* ms;
  int32_t* cnt;
};
static inline __host__ __device__ Ws ws_split(void* ws, int64_t R, int64_t nch, int k) {
  Ws w;
  w.keys = (u64*)ws;
  w.ms = (float*)(w.keys + R * nch * k);
  w.cnt = (int32_t*)(w.ms + R * nch * 2);
  return w;
}

template <bool LSE, bool LAB>
__global__ __launch_bounds__(PT) void predict_chunk_kernel(const float* __restrict__ logits, long ldv, int V, int k,
                                                          const int64_t* __restrict__ labels, Ws ws) {
  const int row = blockIdx.x, chunk = blockIdx.y, nch = gridDim.y;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const float* x = logits + (long)row * ldv;
  const int c0 = chunk * CHUNK;
  __shared__ u64 red_k[2][4];
  __shared__ float red_f[2][4];

  f32x4 v[PV];
#pragma unroll
  for (int j = 0; j < PV; ++j) {
    const int c = c0 + (j * PT + tid) * 4;
    v[j] = (c < V) ? *(const f32x4*)(x + c) : f32x4{0.f, 0.f, 0.f, 0.f};  // (c < V <= ldv, ldv % 4 == 0: c + 3 < ldv)
  }

  // the thread's largest key below `bound`; columns at or beyond V have no key
  auto scan = [&](u64 bound) {
    u64 best = 0;
#pragma unroll
    for (int j = 0; j < PV; ++j) {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int c = c0 + (j * PT + tid) * 4 + e;
        const u64 key = (c < V) ? col_key(v[j][e], c) : 0ull;
        if (key < bound && key > best) best = key;
      }
    }
    return best;
  };

  u64* out_k = ws.keys + ((long)row * nch + chunk) * k;
  u64 mine = scan(~0ull);
  for (int r = 0; r < k; ++r) {
    const u64 w = wave_max_u64(mine);
    if (lane == 0) red_k[r & 1][wv] = w;
    __syncthreads();
    const u64 a = red_k[r & 1][0], b = red_k[r & 1][1], c = red_k[r & 1][2], d = red_k[r & 1][3];
    const u64 ab = a > b ? a : b, cd = c > d ? c : d;
    const u64 win = ab > cd ? ab : cd;
    if (tid == 0) out_k[r] = win;
    if (win == 0) {  // (uniform) nothing left in this chunk: the remaining slots are empty
      if (tid == 0)
        for (int q = r + 1; q < k; ++q) out_k[q] = 0;
      break;
    }
    if (mine == win) mine = scan(win);
  }

  if (LSE) {
    float m = -INFINITY;
#pragma unroll
    for (int j = 0; j < PV; ++j) {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int c = c0 + (j * PT + tid) * 4 + e;
        if (c < V) m = fmaxf(m, v[j][e]);  // (a NaN is skipped here and enters through the sum)
      }
    }
    m = wave_max(m);
    if (lane == 0) red_f[0][wv] = m;
    __syncthreads();
    m = fmaxf(fmaxf(red_f[0][0], red_f[0][1]), fmaxf(red_f[0][2], red_f[0][3]));
    const float ms = (m == INFINITY || m == -INFINITY) ? 0.f : m;  // (inf - inf would be a NaN)
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < PV; ++j) {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int c = c0 + (j * PT + tid) * 4 + e;
        if (c < V) s += __expf(v[j][e] - ms);
      }
    }
    s = wave_sum(s);
    if (lane == 0) red_f[1][wv] = s;
    __syncthreads();
    if (tid == 0) {
      float* o = ws.ms + ((long)row * nch + chunk) * 2;
      o[0] = m;  // (s is relative to m, or to 0 where m is infinite)
      o[1] = ((red_f[1][0] + red_f[1][1]) + red_f[1][2]) + red_f[1][3];
    }
  }

  if (LAB) {
    const int64_t lab64 = labels[row];
    const bool in_row = lab64 >= 0 && lab64 < V;  // (a label outside the row is not dereferenced: rank 0, NLL NaN)
    const int lab = in_row ? (int)lab64 : 0;
    const float xl = in_row ? x[lab] : __uint_as_float(0x7FC00000u);
    int cnt = 0;
#pragma unroll
    for (int j = 0; j < PV; ++j) {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int c = c0 + (j * PT + tid) * 4 + e;
        const float xv = v[j][e];
        if (c < V && (xv > xl || (xv == xl && c < lab))) ++cnt;
      }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
    __shared__ int red_c[4];
    if (lane == 0) red_c[wv] = cnt;
    __syncthreads();
    if (tid == 0) ws.cnt[(long)row * nch + chunk] = red_c[0] + red_c[1] + red_c[2] + red_c[3];
  }
}

template <bool LSE, bool LAB>
__global__ __launch_bounds__(64) void predict_merge_kernel(const float* __restrict__ logits, long ldv, int V, int k, int nch,
                                                          const int64_t* __restrict__ labels, const float* __restrict__ row_lse,
                                                          Ws ws, int32_t* __restrict__ topk_ids, float* __restrict__ topk_logprob,
                                                          int32_t* __restrict__ label_rank, float* __restrict__ row_nll) {
  const int row = blockIdx.x, lane = threadIdx.x;
  float lse;
  if (LSE) {  // chunk order; every lane computes the same value
    const float* ms = ws.ms + (long)row * nch * 2;
    float M = -INFINITY;
    for (int c = 0; c < nch; ++c) M = fmaxf(M, ms[2 * c]);
    auto finite_or_0 = [](float m) { return (m == INFINITY || m == -INFINITY) ? 0.f : m; };
    const float M0 = finite_or_0(M);
    float S = 0.f;
    for (int c = 0; c < nch; ++c) {
      const float s = ms[2 * c + 1];
      S += (s == 0.f) ? 0.f : s * __expf(finite_or_0(ms[2 * c]) - M0);  // (an all -inf chunk adds nothing)
    }
    M = M0;
    lse = M + logf(S);
  } else {
    lse = row_lse[row];
  }
  const u64* keys = ws.keys + (long)row * nch * k;
  const int n = nch * k;
  u64 bound = ~0ull;
  for (int r = 0; r < k; ++r) {
    u64 best = 0;
    for (int i = lane; i < n; i += 64) {
      const u64 key = keys[i];
      if (key < bound && key > best) best = key;
    }
    best = wave_max_u64(best);
    if (lane == 0) {
      const bool none = best == 0;
      topk_ids[(long)row * k + r] = none ? -1 : (int32_t)(~(uint32_t)best);
      topk_logprob[(long)row * k + r] = none ? -INFINITY : key_val((uint32_t)(best >> 32)) - lse;
    }
    bound = best;  // (0: every later round finds nothing)
  }
  if (LAB) {
    int cnt = 0;
    for (int c = lane; c < nch; c += 64) cnt += ws.cnt[(long)row * nch + c];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
    if (lane == 0) {
      label_rank[row] = cnt;
      const int64_t lab = labels[row];
      row_nll[row] = (lab >= 0 && lab < V) ? lse - logits[(long)row * ldv + lab] : __uint_as_float(0x7FC00000u);
    }
  }
}

}  // namespace

extern "C" int64_t fbl_row_predict_ws_bytes(int R, int V, int k) {
  if (V < 1) return FBL_ERR_SHAPE;
  if (k < 1 || k > FBL_PREDICT_MAX_K) return FBL_ERR_ARG;
  if (R <= 0) return 0;
  const int64_t nch = n_chunks(V);
  return (int64_t)R * nch * ((int64_t)k * 8 + 2 * 4 + 4);
}

extern "C" int fbl_row_predict(const float* logits, int64_t ldv, int R, int V, int k, const int64_t* labels,
                               const float* row_lse, int32_t* topk_ids, float* topk_logprob, int32_t* label_rank,
                               float* row_nll, void* ws, int64_t ws_bytes, void* stream) {
  if (V < 1 || ldv < V || R < 0) return FBL_ERR_SHAPE;
  if (k < 1 || k > FBL_PREDICT_MAX_K) return FBL_ERR_ARG;
  if (R == 0) return 0;
  if (!logits || !topk_ids || !topk_logprob || !ws) return FBL_ERR_ARG;
  if (labels ? (!label_rank || !row_nll) : (label_rank || row_nll)) return FBL_ERR_ARG;
  if ((ldv & 3) || ((uintptr_t)logits & 15) || ((uintptr_t)ws & 7)) return FBL_ERR_ALIGN;
  if (ws_bytes < fbl_row_predict_ws_bytes(R, V, k)) return FBL_ERR_ARG;
  const int64_t nch = n_chunks(V);
  if (nch > 65535) return FBL_ERR_SHAPE;  // (chunks are the grid's y dimension)
  const Ws w = ws_split(ws, R, nch, k);
  const dim3 grid((unsigned)R, (unsigned)nch);
  int rc = fbl_bool(row_lse == nullptr, [&](auto LSE) {
    return fbl_bool(labels != nullptr, [&](auto LAB) {
      constexpr bool lse = decltype(LSE)::value, lab = decltype(LAB)::value;
      int e = fbl_launch<predict_chunk_kernel<lse, lab>>(grid, dim3(PT), 0, stream, logits, (long)ldv, V, k, labels, w);
      if (e) return e;
      return fbl_launch<predict_merge_kernel<lse, lab>>(dim3((unsigned)R), dim3(64), 0, stream, logits, (long)ldv, V, k,
                                                        (int)nch, labels, row_lse, w, topk_ids, topk_logprob, label_rank,
                                                        row_nll);
    });
  });
  return rc;
}
