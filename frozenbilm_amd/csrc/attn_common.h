// Shared pieces of the fused disentangled-attention kernels for gfx950 (attn_fwd.hip, attn_bwd.hip, attn_qrows.hip, mha.hip):
//   * the workgroup -> (tile, head, sample) mapping of the 64 x 64 tile grids (wg_coord),
//   * buffer addressing with a wave-uniform base (buf_rsrc / buf_ld16 / buf_st16),
//   * the relative-index table padded to the tile grid (load_idx_padded),
//   * the attention-probability dropout RNG (DropKey, attn_drop_*),
//   * the shape check every entry point applies (grid_shape_ok),
// and small helpers: the fp16 conversion of bias tiles (to_f16x4, saturating at +-65504), clampi, LDV, LOG2E.
#pragma once
#include "fbl_common.h"

typedef _Float16 f16;
typedef __attribute__((ext_vector_type(4))) _Float16 f16x4;

namespace attn {

constexpr int LDV = 72;  // bf16 row stride of transposed-operand tiles ([64 d][64 + 8])

__device__ __forceinline__ f16x4 to_f16x4(f32x4 v) {
  f32x4 m;
#pragma unroll
  for (int e = 0; e < 4; ++e) m[e] = __builtin_amdgcn_fmed3f(v[e], -65504.f, 65504.f);
  return __builtin_convertvector(m, f16x4);
}
__device__ __forceinline__ int clampi(int v, int lo, int hi) { return min(max(v, lo), hi); }

// Workgroup -> (tile x, head h, sample b) for a 1-D grid of nx * nh * B workgroups.
//  * the nx tiles of one (sample, head) share their K/V (or Q/dO, or transposed-operand) rows: they are placed on ONE XCD
//    (the dispatcher hands block L to XCD L % 8 -- observed, used for L2 affinity only) and dispatched back to back, so
//    those rows are fetched into one L2 once instead of into up to nx of them;
//  * samples are walked in the caller's `border` order (longest first): the work per sample grows with klen^2 and the
//    grid is several waves deep, so the long samples must not be the last ones dispatched.
struct WgCoord { int x, h, b; };
#ifdef FBL_DEBUG_SWITCHES
__device__ int g_attn_plainmap;  // measurement switch (debug builds only): 1 = plain b-major mapping
__device__ int g_attn_dbgbits;   // FBL_ATTN_DBG: ablation bits of the attention kernels (tools/README.md, bench_attn.py)
#define FBL_ATTN_PLAINMAP g_attn_plainmap
#define FBL_ATTN_DBGBITS g_attn_dbgbits
static inline void attn_debug_init() {
  static bool once = false;
  if (!once) {
    const int v = FBL_ENV_INT("FBL_ATTN_PLAINMAP", 0);
    (void)hipMemcpyToSymbol(HIP_SYMBOL(g_attn_plainmap), &v, sizeof(v));
    const int d = FBL_ENV_INT("FBL_ATTN_DBG", 0);
    (void)hipMemcpyToSymbol(HIP_SYMBOL(g_attn_dbgbits), &d, sizeof(d));
    once = true;
  }
}
#else
#define FBL_ATTN_PLAINMAP 0
#define FBL_ATTN_DBGBITS 0
static inline void attn_debug_init() {}
#endif
__device__ __forceinline__ WgCoord wg_coord(int nx, int nh, int B, const int32_t* border) {
  const int L = blockIdx.x, ng = nh * B;
  int G, x;
  if ((ng & 7) == 0 && !FBL_ATTN_PLAINMAP) {
    const int s = L >> 3;
    G = (s / nx) * 8 + (L & 7);
    x = s % nx;
  } else {
    G = L / nx;
    x = L % nx;
  }
  const int bs = G / nh;
  WgCoord c;
  c.x = x;
  c.h = G - bs * nh;
  c.b = border ? border[bs] : bs;
  return c;
}

constexpr float LOG2E = 1.4426950408889634f;

// Buffer addressing for kernels that stream several tensors per loop iteration: a 128-bit descriptor of a WAVE-UNIFORM base in
// scalar registers + a 32-bit per-lane byte offset + a scalar byte offset (the per-iteration part) -- no 64-bit per-lane
// pointers (2 VGPRs and a 64-bit add per stream and iteration otherwise).  The base passes through readfirstlane so that the
// compiler can prove it uniform (anything derived from blockIdx-dependent LOADS is "divergent" to it and every access would
// be wrapped in a waterfall loop).  Offsets must stay below 4 GiB from the base.
typedef __attribute__((ext_vector_type(4))) unsigned int u32x4;
__device__ __forceinline__ __amdgpu_buffer_rsrc_t buf_rsrc(const void* p) {
  const uint64_t a = (uint64_t)p;
  const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)a), hi = __builtin_amdgcn_readfirstlane((uint32_t)(a >> 32));
  return __builtin_amdgcn_make_buffer_rsrc((void*)(((uint64_t)hi << 32) | lo), 0, 0xffffffffu, 0x00020000);
}
__device__ __forceinline__ bf16x8 buf_ld16(__amdgpu_buffer_rsrc_t r, uint32_t voff, uint32_t soff) {
  const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(r, voff, soff, 0);
  return __builtin_bit_cast(bf16x8, v);
}
__device__ __forceinline__ void buf_st16(__amdgpu_buffer_rsrc_t r, uint32_t voff, uint32_t soff, bf16x8 v) {
  __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v), r, voff, soff, 0);
}

// Relative-index table padded to the 64-tile grid: idxp[t] = relidx[clamp(t - (Sp - S), 0, 2S-2)] with t = i - j + Sp - 1,
// so that every (i, j) of a tile (valid or padding) indexes it without a clamp.  2*Sp - 1 <= 1023 entries.
__device__ __forceinline__ void load_idx_padded(int16_t* idxp, const int16_t* relidx, int S, int Sp, int tid, int nthr) {
  for (int t = tid; t < 2 * Sp - 1; t += nthr) idxp[t] = relidx[clampi(t - (Sp - S), 0, 2 * S - 2)];
}

// ---- attention-probability dropout RNG (shared by the forward and the backward-A kernels).
// One 32-bit counter hash serves a 2x2 block of (query, key) pairs: four 16-bit fields, field (i&1)*2 + (j&1), each
// compared with a 16-bit threshold (p quantised to 1/65536; the kept values are scaled by the exact 1/(1-p_q)).
// 32-bit integer multiplies are quarter rate on CDNA, so this costs ~6x fewer issue slots than one 64-bit mix per
// element.  Keys are derived per (seed, batch*head) with the common 64-bit mixer.
struct DropKey {
  uint32_t k1, k2, thr16;
  float inv_keep;
};
__device__ __forceinline__ DropKey attn_drop_key(uint64_t seed, int bh, float p) {
  DropKey k;
  k.k1 = fbl_hash(seed, 2ull * (uint64_t)bh);
  k.k2 = fbl_hash(seed, 2ull * (uint64_t)bh + 1ull);
  const float t = p * 65536.f + 0.5f;
  k.thr16 = p > 0.f ? (uint32_t)fminf(t, 65535.f) : 0u;
  k.inv_keep = 65536.f / (65536.f - (float)k.thr16);
  return k;
}
// the two words of block (bi, bj) = (i >> 1, j >> 1); Sp2 = Sp / 2
__device__ __forceinline__ void attn_drop_block(const DropKey& k, int bi, int bj, int Sp2, uint32_t* x_out, uint32_t* y_out) {
  uint32_t x = (uint32_t)(bi * Sp2 + bj) * 0x9E3779B1u + k.k1;
  x ^= x >> 16; x *= 0x7feb352du;
  x ^= x >> 15; x *= 0x846ca68bu;
  x ^= x >> 16;
  uint32_t y = (x ^ k.k2) * 0x2c1b3c6du;
  y ^= y >> 15;
  *x_out = x;
  *y_out = y;
}
// keep factor (0 or 1/(1-p)) of the element with parities (pi, pj) inside its block
__device__ __forceinline__ float attn_drop_keep(const DropKey& k, uint32_t x, uint32_t y, int pi, int pj) {
  const uint32_t wsel = pi ? y : x;
  const uint32_t f = pj ? (wsel >> 16) : (wsel & 0xffffu);
  return f >= k.thr16 ? k.inv_keep : 0.f;
}

// ---- host side: the tile grid every fused disentangled-attention entry point accepts (S positions padded to Sp, tiles of 64)
static inline bool grid_shape_ok(int S, int Sp) { return S >= 1 && S <= 512 && Sp >= S && Sp % 64 == 0; }

}  // namespace attn
