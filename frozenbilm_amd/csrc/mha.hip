// Fused multi-head attention for gfx950, head_dim 64: BERT's self-attention (include/fbl_mha.h).
//
//   score[i,j] = scale * Q_i.K_j + (mask[j] ? 0 : -10000),   ctx = dropout(softmax_j(score)) . V
//   reference: model/bert.py:138-191 (BertSelfAttention), get_extended_attention_mask :640-642
//
// The mask is additive and on keys only: every query row is computed, padded ones included, and a sample without any
// valid key softmaxes over all of its keys (the -10000 is then a common offset).  Key tiles at or beyond klen are
// skipped: there exp(score - max) underflows to exactly 0 in fp32, so skipping changes no bit.
//
// Forward: one workgroup (4 waves) = one (sample, head, 64-query tile), key tiles of 64, fp32 online softmax in the exp2
// domain, MFMA 16x16x32 bf16.  The MFMAs are "swapped" (keys as A rows, queries as B columns) so a lane owns one query:
// the softmax statistics are in-lane + 2 shuffles and P feeds the P.V MFMA from registers; the V^T fragments come out of
// the row-major V tile through ds_read_b64_tr_b16 (attn_fwd.hip does the same around its position terms).
// Backward (no atomics, bit-reproducible, enqueue-only):
//   dkdv: one workgroup per (sample, head, 64-KEY tile), a lane owns one key; sweeps the query tiles, recomputes P^T from
//         lse, keeps dK and dV in registers (dV += dO^T.P~^T, dK += Q^T.dS^T, both with the query as contraction index).
//   dq:   one workgroup per (sample, head, 64-query tile), a lane owns one query; sweeps the key tiles (dQ += K^T.dS^T).
//   D = rowdot(dO, O) comes from fbl_attn_rowdot; dS never leaves the registers.
#include "attn_common.h"
#include "../../include/fbl_mha.h"

namespace {
using namespace attn;

struct MhaArgs {
  const bf16* q; const bf16* k; const bf16* v; const bf16* dO;
  long ldq, ldk, ldv, lddo;
  const int32_t* mask;
  const int32_t* klen;
  const int32_t* border;
  const int32_t* row0;  // packed rows (fbl_mha_*_rows): sample b owns the activation rows [row0[b], row0[b+1]); nullptr: b*S
  const float* lse;
  const float* Dv;
  float scale, p_drop;
  uint64_t seed; const uint64_t* seed_dev;
  bf16* out0; long ld0;  // forward: ctx     backward: dK (dkdv) / dQ (dq)
  bf16* out1; long ld1;  // backward dkdv: dV
  float* lse_out;
  int B, S, nh;
};

constexpr float MASK_BIAS = -10000.f * LOG2E;  // the reference's additive mask, in the exp2 domain

constexpr int SM_A = 0;             // [64][64] bf16 swizzled: K (forward, dq) or Q (dkdv)
constexpr int SM_B = SM_A + 8192;   // [64][64] bf16 swizzled: V (forward, dq) or dO (dkdv)
constexpr int SM_QS = SM_B + 8192;  // [64][64] bf16 swizzled: the forward's Q tile
constexpr int SM_F0 = SM_QS + 8192; // float [64]: key bias (forward, dq) or query lse*log2(e) (dkdv)
constexpr int SM_F1 = SM_F0 + 256;  // float [64]: query D (dkdv)
constexpr int SM_TOTAL = SM_F1 + 256;

// Keys of sample b the kernels visit: [0, klen) rounded up to whole tiles; the whole row when the sample has no valid key
// (the reference then softmaxes over all keys) or klen is not given.
__device__ __forceinline__ int key_limit(const int32_t* klen, int b, int S) {
  const int kl = klen ? min(klen[b], S) : S;
  return kl > 0 ? kl : S;
}

__device__ __forceinline__ float key_bias(int j, int pl, int m) {
  return j < pl ? (m != 0 ? 0.f : MASK_BIAS) : -INFINITY;
}

// The activation rows of sample b (q / k / v / ctx / dO / dQ / dK / dV): first row and how many of its S positions have one.
// The mask, lse and D keep the padded [B, S] indexing in both layouts.
struct Rows { long rb; int pl; };
__device__ __forceinline__ Rows sample_rows(const int32_t* row0, int b, int S) {
  Rows r;
  if (row0) {
    const int r0 = row0[b];
    r.rb = r0;
    r.pl = min(row0[b + 1] - r0, S);  // (<= 0: the sample has no row, its workgroups do nothing)
  } else {
    r.rb = (long)b * S;
    r.pl = S;
  }
  return r;
}

struct Pair { bf16x8 x[2], y[2]; int km; };

// the 64 x 64 bf16 tiles of two tensors (rows r0 .. r0+63 of this sample, clamped to the last row) into registers
__device__ __forceinline__ void load_pair(Pair& R, const bf16* x, long ldx, const bf16* y, long ldy, long rb, int r0, int pl,
                                          int col, int srow, int sch) {
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    const long r = rb + min(r0 + srow + t * 32, pl - 1);
    R.x[t] = *(const bf16x8*)(x + r * ldx + col + sch * 8);
    R.y[t] = *(const bf16x8*)(y + r * ldy + col + sch * 8);
  }
}
__device__ __forceinline__ void store_pair(char* smem, const Pair& R, int sb) {
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    *(bf16x8*)(smem + SM_A + sb + t * 4096) = R.x[t];
    *(bf16x8*)(smem + SM_B + sb + t * 4096) = R.y[t];
  }
}

// the transposed fragment of a row-major swizzled [64 rows][64 cols] tile for the MFMA whose contraction index is the row:
// A[col dt*16 + c][k-slot e] = tile[kk*32 + (e>>2)*16 + g*4 + (e&3)][dt*16 + c]   (the k-slot order of pack_p)
__device__ __forceinline__ bf16x8 tr_frag(const char* tile, int kk, int dt, int c, int g) {
  const int r = g * 4 + (c >> 2);
  const int ch = dt * 2 + ((c >> 1) & 1), sub = (c & 1) * 8;
  const char* vb = tile + r * 128 + ((ch ^ (r & 7)) << 4) + sub;
  union { tr16x4 h[2]; bf16x8 v; } u;
  u.h[0] = lds_tr16((const bf16*)(vb + kk * 4096));
  u.h[1] = lds_tr16((const bf16*)(vb + kk * 4096 + 2048));
  return u.v;
}
// B operand of that MFMA from 16 per-lane values x[nt*4 + r] (row nt*16 + g*4 + r of the 64): k-step kk
__device__ __forceinline__ bf16x8 pack_p(const float* x, int kk) {
  bf16x8 pf;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    pf[e] = f2bf(x[(2 * kk) * 4 + e]);
    pf[4 + e] = f2bf(x[(2 * kk + 1) * 4 + e]);
  }
  return pf;
}

// dropout keep factors of the 16 pairs of a lane: the lane's own index `own` (query in the forward / dq, key in dkdv) and the
// 16 others o0 + nt*16 + g*4 + r; `own_is_query` tells which side of the (query, key) pair the lane's index is
__device__ __forceinline__ void keep16(const DropKey& dk, bool live, int own, int o0, int g, int Sp2, bool own_is_query,
                                       float* kf) {
#pragma unroll
  for (int e = 0; e < 16; ++e) kf[e] = 1.f;
  if (!live) return;
#pragma unroll
  for (int nt = 0; nt < 4; ++nt)
#pragma unroll
    for (int bb = 0; bb < 2; ++bb) {
      const int o = o0 + nt * 16 + g * 4 + bb * 2;  // even
      uint32_t x, y;
      if (own_is_query) {
        attn_drop_block(dk, own >> 1, o >> 1, Sp2, &x, &y);
        kf[nt * 4 + bb * 2] = attn_drop_keep(dk, x, y, own & 1, 0);
        kf[nt * 4 + bb * 2 + 1] = attn_drop_keep(dk, x, y, own & 1, 1);
      } else {
        attn_drop_block(dk, o >> 1, own >> 1, Sp2, &x, &y);
        kf[nt * 4 + bb * 2] = attn_drop_keep(dk, x, y, 0, own & 1);
        kf[nt * 4 + bb * 2 + 1] = attn_drop_keep(dk, x, y, 1, own & 1);
      }
    }
}

// ------------------------------------------------------------------------------------------------------------ forward
__global__ __launch_bounds__(256, 2) void mha_fwd_kernel(MhaArgs a) {
  __shared__ __attribute__((aligned(16))) char smem[SM_TOTAL];
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int c = lane & 15, g = lane >> 4;
  const int S = a.S, Sp = (S + 63) & ~63;
  const WgCoord wc = wg_coord(Sp / 64, a.nh, a.B, a.border);
  const int i0 = wc.x * 64, h = wc.h, b = wc.b;
  const int i = i0 + w * 16 + c;  // this lane's query row
  const Rows rw = sample_rows(a.row0, b, S);
  const long rb = rw.rb, mb = (long)b * S;
  const int pl = rw.pl;
  if (i0 >= pl) return;  // (packed rows: a query tile the sample has no row of)
  const int nkt = (min(key_limit(a.klen, b, S), pl) + 63) / 64;
  float* kb = (float*)(smem + SM_F0);

  const DropKey dk = attn_drop_key(a.p_drop > 0.f ? fbl_seed(a.seed, a.seed_dev) : 0, b * a.nh + h, a.p_drop);
  const float k2 = a.scale * LOG2E;
  const int srow = tid >> 3, sch = tid & 7;
  const int fb0 = c * 128 + ((g ^ (c & 7)) << 4), fb1 = fb0 ^ 64;
  const int sb = srow * 128 + ((sch ^ (srow & 7)) << 4);

  Pair R;
  load_pair(R, a.k, a.ldk, a.v, a.ldv, rb, 0, pl, h * 64, srow, sch);
  R.km = a.mask[mb + min(lane, S - 1)];
#pragma unroll
  for (int t = 0; t < 2; ++t)
    *(bf16x8*)(smem + SM_QS + sb + t * 4096) = *(const bf16x8*)(a.q + (rb + min(i0 + srow + t * 32, pl - 1)) * a.ldq + h * 64 + sch * 8);

  float m_run = -INFINITY, l_run = 0.f;
  f32x4 o[4];
#pragma unroll
  for (int dt = 0; dt < 4; ++dt) o[dt] = (f32x4){0.f, 0.f, 0.f, 0.f};

  for (int jt = 0; jt < nkt; ++jt) {
    const int j0 = jt * 64;
    store_pair(smem, R, sb);
    if (tid < 64) kb[tid] = key_bias(j0 + tid, pl, R.km);
    __syncthreads();  // K / V tile, key bias (and, first time round, the Q tile) visible
    {  // next tile in flight during this one (unconditional: behind a branch later waits could not count the requests)
      const int jn = min(jt + 1, nkt - 1) * 64;
      load_pair(R, a.k, a.ldk, a.v, a.ldv, rb, jn, pl, h * 64, srow, sch);
      R.km = a.mask[mb + min(jn + lane, S - 1)];
    }
    // ---- scores, transposed: sacc[nt][r] = Q_i . K_j,  j = j0 + nt*16 + g*4 + r
    f32x4 sacc[4];
    const bf16x8 qf0 = *(const bf16x8*)(smem + SM_QS + w * 2048 + fb0), qf1 = *(const bf16x8*)(smem + SM_QS + w * 2048 + fb1);
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) {
      f32x4 acc = (f32x4){0.f, 0.f, 0.f, 0.f};
      acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(*(const bf16x8*)(smem + SM_A + nt * 2048 + fb0), qf0, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(*(const bf16x8*)(smem + SM_A + nt * 2048 + fb1), qf1, acc, 0, 0, 0);
      sacc[nt] = acc;
    }
    float p[16];
    float mx = -INFINITY;
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) {
      const f32x4 bias = *(const f32x4*)(kb + nt * 16 + g * 4);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float t = fmaf(sacc[nt][r], k2, bias[r]);
        p[nt * 4 + r] = t;
        mx = fmaxf(mx, t);
      }
    }
    mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    const float m_new = fmaxf(m_run, mx);  // finite: key j0 < pl of every visited tile has a finite score
    const float alpha = __builtin_amdgcn_exp2f(m_run - m_new);
    float psum = 0.f;
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      p[e] = __builtin_amdgcn_exp2f(p[e] - m_new);
      psum += p[e];
    }
    psum += __shfl_xor(psum, 16, 64);
    psum += __shfl_xor(psum, 32, 64);
    l_run = l_run * alpha + psum;
    m_run = m_new;
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) o[dt] *= alpha;
    float kf[16];
    keep16(dk, a.p_drop > 0.f, i, j0, g, Sp >> 1, true, kf);
#pragma unroll
    for (int e = 0; e < 16; ++e) p[e] *= kf[e];
    // ---- O^T += V^T . P^T
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      const bf16x8 pf = pack_p(p, kk);
#pragma unroll
      for (int dt = 0; dt < 4; ++dt)
        o[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(tr_frag(smem + SM_B, kk, dt, c, g), pf, o[dt], 0, 0, 0);
    }
    __syncthreads();  // the tiles are overwritten by the next key tile
  }

  if (i < pl) {
    const float inv_l = 1.f / l_run;
    bf16* op = a.out0 + (rb + i) * a.ld0 + h * 64 + g * 4;
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) {
      const f32x4 v = o[dt] * inv_l;
      *(bf16x4*)(op + dt * 16) = (bf16x4){f2bf(v[0]), f2bf(v[1]), f2bf(v[2]), f2bf(v[3])};
    }
    if (g == 0) a.lse_out[((long)b * a.nh + h) * S + i] = (m_run + __log2f(l_run)) * 0.69314718055994531f;
  }
}

// ------------------------------------------------------------------------------------------------------------ backward
// dK, dV of one 64-key tile.  MFMA roles: A = query rows (Q / dO tile in LDS), B = this wave's 16 keys (K / V fragments in
// registers): sacc[nt][r] = Q_i . K_j with j = the lane's key, i = i0 + nt*16 + g*4 + r.
__global__ __launch_bounds__(256, 2) void mha_bwd_dkdv_kernel(MhaArgs a) {
  __shared__ __attribute__((aligned(16))) char smem[SM_TOTAL];
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int c = lane & 15, g = lane >> 4;
  const int S = a.S, Sp = (S + 63) & ~63;
  const WgCoord wc = wg_coord(Sp / 64, a.nh, a.B, a.border);
  const int j0 = wc.x * 64, h = wc.h, b = wc.b;
  const int j = j0 + w * 16 + c;  // this lane's key
  const Rows rw = sample_rows(a.row0, b, S);
  const long rb = rw.rb, mb = (long)b * S;
  const int pl = rw.pl;
  if (j0 >= pl) return;  // (packed rows: a key tile the sample has no row of)
  const int kl = min(key_limit(a.klen, b, S), pl);
  const int nqt = (pl + 63) / 64;  // (query rows the sample does not have carry dO = 0: they add exact zeros)
  float* lse2 = (float*)(smem + SM_F0);
  float* Ds = (float*)(smem + SM_F1);

  f32x4 dv[4], dkk[4];
#pragma unroll
  for (int dt = 0; dt < 4; ++dt) dv[dt] = dkk[dt] = (f32x4){0.f, 0.f, 0.f, 0.f};

  if (j0 < (kl + 63) / 64 * 64) {  // (key tiles the forward skipped have P = 0: dK = dV = 0)
    const int jc = min(j, pl - 1);
    const bf16* kr = a.k + (rb + jc) * a.ldk + h * 64 + g * 8;
    const bf16* vr = a.v + (rb + jc) * a.ldv + h * 64 + g * 8;
    const bf16x8 kf0 = *(const bf16x8*)kr, kf1 = *(const bf16x8*)(kr + 32);
    const bf16x8 vf0 = *(const bf16x8*)vr, vf1 = *(const bf16x8*)(vr + 32);
    const float kbias = key_bias(j, pl, a.mask[mb + min(j, S - 1)]);
    const DropKey dk = attn_drop_key(a.p_drop > 0.f ? fbl_seed(a.seed, a.seed_dev) : 0, b * a.nh + h, a.p_drop);
    const float k2 = a.scale * LOG2E;
    const int srow = tid >> 3, sch = tid & 7;
    const int fb0 = c * 128 + ((g ^ (c & 7)) << 4), fb1 = fb0 ^ 64;
    const int sb = srow * 128 + ((sch ^ (srow & 7)) << 4);
    const float* lse_bh = a.lse + ((long)b * a.nh + h) * S;
    const float* D_bh = a.Dv + ((long)b * a.nh + h) * S;

    Pair R;
    load_pair(R, a.q, a.ldq, a.dO, a.lddo, rb, 0, pl, h * 64, srow, sch);
    float lq = 0.f, dq = 0.f;
    if (tid < 64) { lq = lse_bh[min(tid, pl - 1)]; dq = D_bh[min(tid, pl - 1)]; }
    for (int it = 0; it < nqt; ++it) {
      const int i0 = it * 64;
      store_pair(smem, R, sb);
      if (tid < 64) {
        const bool live = i0 + tid < pl;
        lse2[tid] = live ? lq * LOG2E : INFINITY;  // padding query rows: P = 0
        Ds[tid] = live ? dq : 0.f;
      }
      __syncthreads();
      {
        const int in = min(it + 1, nqt - 1) * 64;
        load_pair(R, a.q, a.ldq, a.dO, a.lddo, rb, in, pl, h * 64, srow, sch);
        if (tid < 64) { lq = lse_bh[min(in + tid, pl - 1)]; dq = D_bh[min(in + tid, pl - 1)]; }
      }
      float p[16], ds[16];
#pragma unroll
      for (int nt = 0; nt < 4; ++nt) {
        f32x4 s = (f32x4){0.f, 0.f, 0.f, 0.f}, dp = (f32x4){0.f, 0.f, 0.f, 0.f};
        s = __builtin_amdgcn_mfma_f32_16x16x32_bf16(*(const bf16x8*)(smem + SM_A + nt * 2048 + fb0), kf0, s, 0, 0, 0);
        s = __builtin_amdgcn_mfma_f32_16x16x32_bf16(*(const bf16x8*)(smem + SM_A + nt * 2048 + fb1), kf1, s, 0, 0, 0);
        dp = __builtin_amdgcn_mfma_f32_16x16x32_bf16(*(const bf16x8*)(smem + SM_B + nt * 2048 + fb0), vf0, dp, 0, 0, 0);
        dp = __builtin_amdgcn_mfma_f32_16x16x32_bf16(*(const bf16x8*)(smem + SM_B + nt * 2048 + fb1), vf1, dp, 0, 0, 0);
        const f32x4 l4 = *(const f32x4*)(lse2 + nt * 16 + g * 4);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          p[nt * 4 + r] = __builtin_amdgcn_exp2f(fmaf(s[r], k2, kbias) - l4[r]);
          ds[nt * 4 + r] = dp[r];
        }
      }
      float kf[16];
      keep16(dk, a.p_drop > 0.f, j, i0, g, Sp >> 1, false, kf);
#pragma unroll
      for (int nt = 0; nt < 4; ++nt) {
        const f32x4 d4 = *(const f32x4*)(Ds + nt * 16 + g * 4);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int e = nt * 4 + r;
          ds[e] = p[e] * fmaf(ds[e], kf[e], -d4[r]) * a.scale;
          p[e] *= kf[e];
        }
      }
      // dV^T += dO^T . P~^T,  dK^T += Q^T . dS^T   (contraction over the 64 queries of the tile)
#pragma unroll
      for (int kk = 0; kk < 2; ++kk) {
        const bf16x8 pf = pack_p(p, kk), sf = pack_p(ds, kk);
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) {
          dv[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(tr_frag(smem + SM_B, kk, dt, c, g), pf, dv[dt], 0, 0, 0);
          dkk[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(tr_frag(smem + SM_A, kk, dt, c, g), sf, dkk[dt], 0, 0, 0);
        }
      }
      __syncthreads();
    }
  }
  if (j < pl) {
    bf16* kp = a.out0 + (rb + j) * a.ld0 + h * 64 + g * 4;
    bf16* vp = a.out1 + (rb + j) * a.ld1 + h * 64 + g * 4;
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) {
      *(bf16x4*)(kp + dt * 16) = (bf16x4){f2bf(dkk[dt][0]), f2bf(dkk[dt][1]), f2bf(dkk[dt][2]), f2bf(dkk[dt][3])};
      *(bf16x4*)(vp + dt * 16) = (bf16x4){f2bf(dv[dt][0]), f2bf(dv[dt][1]), f2bf(dv[dt][2]), f2bf(dv[dt][3])};
    }
  }
}

// dQ of one 64-query tile.  MFMA roles as in the forward: A = key rows (K / V tile in LDS), B = this wave's 16 queries (Q / dO
// fragments in registers).
__global__ __launch_bounds__(256, 2) void mha_bwd_dq_kernel(MhaArgs a) {
  __shared__ __attribute__((aligned(16))) char smem[SM_TOTAL];
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int c = lane & 15, g = lane >> 4;
  const int S = a.S, Sp = (S + 63) & ~63;
  const WgCoord wc = wg_coord(Sp / 64, a.nh, a.B, a.border);
  const int i0 = wc.x * 64, h = wc.h, b = wc.b;
  const int i = i0 + w * 16 + c;  // this lane's query
  const Rows rw = sample_rows(a.row0, b, S);
  const long rb = rw.rb, mb = (long)b * S;
  const int pl = rw.pl;
  if (i0 >= pl) return;
  const int nkt = (min(key_limit(a.klen, b, S), pl) + 63) / 64;
  float* kb = (float*)(smem + SM_F0);

  const int ic = min(i, pl - 1);
  const bf16* qr = a.q + (rb + ic) * a.ldq + h * 64 + g * 8;
  const bf16* orow = a.dO + (rb + ic) * a.lddo + h * 64 + g * 8;
  const bf16x8 qf0 = *(const bf16x8*)qr, qf1 = *(const bf16x8*)(qr + 32);
  const bf16x8 of0 = *(const bf16x8*)orow, of1 = *(const bf16x8*)(orow + 32);
  const float lse2 = i < pl ? a.lse[((long)b * a.nh + h) * S + i] * LOG2E : INFINITY;
  const float Di = i < pl ? a.Dv[((long)b * a.nh + h) * S + i] : 0.f;
  const DropKey dk = attn_drop_key(a.p_drop > 0.f ? fbl_seed(a.seed, a.seed_dev) : 0, b * a.nh + h, a.p_drop);
  const float k2 = a.scale * LOG2E;
  const int srow = tid >> 3, sch = tid & 7;
  const int fb0 = c * 128 + ((g ^ (c & 7)) << 4), fb1 = fb0 ^ 64;
  const int sb = srow * 128 + ((sch ^ (srow & 7)) << 4);

  f32x4 dqa[4];
#pragma unroll
  for (int dt = 0; dt < 4; ++dt) dqa[dt] = (f32x4){0.f, 0.f, 0.f, 0.f};
  Pair R;
  load_pair(R, a.k, a.ldk, a.v, a.ldv, rb, 0, pl, h * 64, srow, sch);
  R.km = a.mask[mb + min(lane, S - 1)];
  for (int jt = 0; jt < nkt; ++jt) {
    const int j0 = jt * 64;
    store_pair(smem, R, sb);
    if (tid < 64) kb[tid] = key_bias(j0 + tid, pl, R.km);
    __syncthreads();
    {
      const int jn = min(jt + 1, nkt - 1) * 64;
      load_pair(R, a.k, a.ldk, a.v, a.ldv, rb, jn, pl, h * 64, srow, sch);
      R.km = a.mask[mb + min(jn + lane, S - 1)];
    }
    float p[16], ds[16];
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) {
      f32x4 s = (f32x4){0.f, 0.f, 0.f, 0.f}, dp = (f32x4){0.f, 0.f, 0.f, 0.f};
      s = __builtin_amdgcn_mfma_f32_16x16x32_bf16(*(const bf16x8*)(smem + SM_A + nt * 2048 + fb0), qf0, s, 0, 0, 0);
      s = __builtin_amdgcn_mfma_f32_16x16x32_bf16(*(const bf16x8*)(smem + SM_A + nt * 2048 + fb1), qf1, s, 0, 0, 0);
      dp = __builtin_amdgcn_mfma_f32_16x16x32_bf16(*(const bf16x8*)(smem + SM_B + nt * 2048 + fb0), of0, dp, 0, 0, 0);
      dp = __builtin_amdgcn_mfma_f32_16x16x32_bf16(*(const bf16x8*)(smem + SM_B + nt * 2048 + fb1), of1, dp, 0, 0, 0);
      const f32x4 bias = *(const f32x4*)(kb + nt * 16 + g * 4);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        p[nt * 4 + r] = __builtin_amdgcn_exp2f(fmaf(s[r], k2, bias[r]) - lse2);
        ds[nt * 4 + r] = dp[r];
      }
    }
    float kf[16];
    keep16(dk, a.p_drop > 0.f, i, j0, g, Sp >> 1, true, kf);
#pragma unroll
    for (int e = 0; e < 16; ++e) ds[e] = p[e] * fmaf(ds[e], kf[e], -Di) * a.scale;
    // dQ^T += K^T . dS^T  (contraction over the 64 keys of the tile)
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      const bf16x8 sf = pack_p(ds, kk);
#pragma unroll
      for (int dt = 0; dt < 4; ++dt)
        dqa[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(tr_frag(smem + SM_A, kk, dt, c, g), sf, dqa[dt], 0, 0, 0);
    }
    __syncthreads();
  }
  if (i < pl) {
    bf16* qp = a.out0 + (rb + i) * a.ld0 + h * 64 + g * 4;
#pragma unroll
    for (int dt = 0; dt < 4; ++dt)
      *(bf16x4*)(qp + dt * 16) = (bf16x4){f2bf(dqa[dt][0]), f2bf(dqa[dt][1]), f2bf(dqa[dt][2]), f2bf(dqa[dt][3])};
  }
}

// D[b,h,s] = dO_row . O_row for the rows that exist (packed layout): the lane arrangement and the summation order of
// fbl_attn_rowdot (8 lanes per (row, head), 3-step shuffle reduction), so the values are its values bit for bit.
__global__ void mha_rowdot_rows_kernel(const bf16* dO, long lddo, const bf16* O, long ldo, const int32_t* row0, float* out,
                                       int B, int S, int nh) {
  const long gid = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long idx = gid >> 3;  // (padded row, head)
  const int c = (int)(gid & 7);
  const long total = (long)B * S * nh;
  const long prow = idx < total ? idx / nh : 0;
  const int h = idx < total ? (int)(idx % nh) : 0;
  const int bb = (int)(prow / S), ss = (int)(prow % S);
  const int r0 = row0[bb];
  const bool live = idx < total && ss < row0[bb + 1] - r0;
  float s = 0.f;
  if (live) {
    const long row = (long)r0 + ss;
    const bf16x8 x = *(const bf16x8*)(dO + row * lddo + h * 64 + c * 8);
    const bf16x8 y = *(const bf16x8*)(O + row * ldo + h * 64 + c * 8);
#pragma unroll
    for (int e = 0; e < 8; ++e) s += bf2f(x[e]) * bf2f(y[e]);
  }
  s += __shfl_xor(s, 1, 64);
  s += __shfl_xor(s, 2, 64);
  s += __shfl_xor(s, 4, 64);
  if (live && c == 0) out[((long)bb * nh + h) * S + ss] = s;
}

int mha_fwd_launch(const void* q, int64_t ldq, const void* k, int64_t ldk, const void* v, int64_t ldv, const int32_t* mask,
                   const int32_t* klen, const int32_t* border, const int32_t* row0, float scale, float p_drop, uint64_t seed,
                   const uint64_t* seed_dev, void* ctx, int64_t ldo, float* lse, int B, int S, int nh, void* stream) {
  if (S < 1 || S > 512) return FBL_ERR_SHAPE;
  if ((ldq % 8) || (ldk % 8) || (ldv % 8) || (ldo % 4)) return FBL_ERR_ALIGN;
  if (!q || !k || !v || !mask || !ctx || !lse || p_drop < 0.f || p_drop >= 1.f) return FBL_ERR_ARG;
  if (B <= 0 || nh <= 0) return 0;
  MhaArgs a{};
  a.q = (const bf16*)q; a.k = (const bf16*)k; a.v = (const bf16*)v;
  a.ldq = ldq; a.ldk = ldk; a.ldv = ldv;
  a.mask = mask; a.klen = klen; a.border = border; a.row0 = row0;
  a.scale = scale; a.p_drop = p_drop; a.seed = seed; a.seed_dev = seed_dev;
  a.out0 = (bf16*)ctx; a.ld0 = ldo; a.lse_out = lse;
  a.B = B; a.S = S; a.nh = nh;
  hipLaunchKernelGGL(mha_fwd_kernel, dim3((unsigned)((S + 63) / 64 * nh * B)), dim3(256), 0, (hipStream_t)stream, a);
  FBL_CHECK_LAUNCH();
  return 0;
}

// (Dv: read by the two passes; with row0 it is also formed here first, from dO and O)
int mha_bwd_launch(const void* q, int64_t ldq, const void* k, int64_t ldk, const void* v, int64_t ldv, const void* dO,
                   int64_t lddo, const void* O, int64_t ldo, const int32_t* mask, const int32_t* klen, const int32_t* border,
                   const int32_t* row0, const float* lse, float* Dv, float scale, float p_drop, uint64_t seed,
                   const uint64_t* seed_dev, void* dQ, int64_t lddq, void* dK, int64_t lddk, void* dV, int64_t lddv, int B, int S,
                   int nh, void* stream) {
  if (S < 1 || S > 512) return FBL_ERR_SHAPE;
  if ((ldq % 8) || (ldk % 8) || (ldv % 8) || (lddo % 8) || (lddq % 4) || (lddk % 4) || (lddv % 4)) return FBL_ERR_ALIGN;
  if (row0 && (ldo % 8)) return FBL_ERR_ALIGN;
  if (!q || !k || !v || !dO || !mask || !lse || !Dv || !dQ || !dK || !dV || p_drop < 0.f || p_drop >= 1.f) return FBL_ERR_ARG;
  if (row0 && !O) return FBL_ERR_ARG;
  if (B <= 0 || nh <= 0) return 0;
  if (row0) {
    const long total = (long)B * S * nh;
    hipLaunchKernelGGL(mha_rowdot_rows_kernel, dim3((unsigned)((total * 8 + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       (const bf16*)dO, (long)lddo, (const bf16*)O, (long)ldo, row0, Dv, B, S, nh);
    FBL_CHECK_LAUNCH();
  }
  MhaArgs a{};
  a.q = (const bf16*)q; a.k = (const bf16*)k; a.v = (const bf16*)v; a.dO = (const bf16*)dO;
  a.ldq = ldq; a.ldk = ldk; a.ldv = ldv; a.lddo = lddo;
  a.mask = mask; a.klen = klen; a.border = border; a.row0 = row0; a.lse = lse; a.Dv = Dv;
  a.scale = scale; a.p_drop = p_drop; a.seed = seed; a.seed_dev = seed_dev;
  a.B = B; a.S = S; a.nh = nh;
  const dim3 grid((unsigned)((S + 63) / 64 * nh * B));
  a.out0 = (bf16*)dK; a.ld0 = lddk; a.out1 = (bf16*)dV; a.ld1 = lddv;
  hipLaunchKernelGGL(mha_bwd_dkdv_kernel, grid, dim3(256), 0, (hipStream_t)stream, a);
  FBL_CHECK_LAUNCH();
  a.out0 = (bf16*)dQ; a.ld0 = lddq; a.out1 = nullptr; a.ld1 = 0;
  hipLaunchKernelGGL(mha_bwd_dq_kernel, grid, dim3(256), 0, (hipStream_t)stream, a);
  FBL_CHECK_LAUNCH();
  return 0;
}

}  // namespace

extern "C" int fbl_mha_fwd(const void* q, int64_t ldq, const void* k, int64_t ldk, const void* v, int64_t ldv,
                           const int32_t* mask, const int32_t* klen, const int32_t* border, float scale, float p_drop,
                           uint64_t seed, const uint64_t* seed_dev, void* ctx, int64_t ldo, float* lse, int B, int S, int nh,
                           void* stream) {
  return mha_fwd_launch(q, ldq, k, ldk, v, ldv, mask, klen, border, nullptr, scale, p_drop, seed, seed_dev, ctx, ldo, lse, B, S,
                        nh, stream);
}

extern "C" int fbl_mha_fwd_rows(const void* q, int64_t ldq, const void* k, int64_t ldk, const void* v, int64_t ldv,
                                const int32_t* mask, const int32_t* klen, const int32_t* border, const int32_t* row0, float scale,
                                float p_drop, uint64_t seed, const uint64_t* seed_dev, void* ctx, int64_t ldo, float* lse, int B,
                                int S, int nh, void* stream) {
  if (S < 1 || S > 512) return FBL_ERR_SHAPE;
  if (!row0 || !klen) return FBL_ERR_ARG;
  return mha_fwd_launch(q, ldq, k, ldk, v, ldv, mask, klen, border, row0, scale, p_drop, seed, seed_dev, ctx, ldo, lse, B, S, nh,
                        stream);
}

extern "C" int fbl_mha_bwd(const void* q, int64_t ldq, const void* k, int64_t ldk, const void* v, int64_t ldv,
                           const void* dO, int64_t lddo, const int32_t* mask, const int32_t* klen, const int32_t* border,
                           const float* lse, const float* Dv, float scale, float p_drop, uint64_t seed,
                           const uint64_t* seed_dev, void* dQ, int64_t lddq, void* dK, int64_t lddk, void* dV, int64_t lddv,
                           int B, int S, int nh, void* stream) {
  return mha_bwd_launch(q, ldq, k, ldk, v, ldv, dO, lddo, nullptr, 0, mask, klen, border, nullptr, lse, (float*)Dv, scale, p_drop,
                        seed, seed_dev, dQ, lddq, dK, lddk, dV, lddv, B, S, nh, stream);
}

extern "C" int fbl_mha_bwd_rows(const void* q, int64_t ldq, const void* k, int64_t ldk, const void* v, int64_t ldv,
                                const void* dO, int64_t lddo, const void* O, int64_t ldo, const int32_t* mask,
                                const int32_t* klen, const int32_t* border, const int32_t* row0, const float* lse, float* Dv,
                                float scale, float p_drop, uint64_t seed, const uint64_t* seed_dev, void* dQ, int64_t lddq,
                                void* dK, int64_t lddk, void* dV, int64_t lddv, int B, int S, int nh, void* stream) {
  if (S < 1 || S > 512) return FBL_ERR_SHAPE;
  if (!row0 || !klen || !O) return FBL_ERR_ARG;
  return mha_bwd_launch(q, ldq, k, ldk, v, ldv, dO, lddo, O, ldo, mask, klen, border, row0, lse, Dv, scale, p_drop, seed,
                        seed_dev, dQ, lddq, dK, lddk, dV, lddv, B, S, nh, stream);
}
