// Disentangled self-attention whose QUERY rows are a gathered subset of the token rows while its keys are the whole
// sample (the enhanced mask decoder on the selected rows; include/fbl_qrows.h).
//
//   score[r,j] = scale * ( Q_r.K_j + Q_r.PK[idx(i_r-j)] + K_j.PQ[idx(i_r-j)] ),   i_r = rpos[r],   ctx[r] = dropout(softmax(score)) . V
//
// Neighbouring compact rows sit at arbitrary positions, so the Toeplitz windows of the full-grid kernels do not exist here.
// One wave owns a GROUP of up to 16 compact rows of one sample and one head and sweeps the sample's keys in tiles of 32:
//   T1[r][w] = Q_r . PK[w]   once per group, for the table rows w the group can reach  (MFMA, fp16 in LDS)
//   T2[j][w] = K_j . PQ[w]   per 16 keys, for the table rows [idx(i_max - j_lo) .. idx(i_min - j_hi)] they can reach -- one or
//                            two row tiles for a single selected row, up to the whole table for rows spread over the sample
// followed by the gather  c2p = T1[r][idx(i_r-j)],  p2c = T2[j][idx(i_r-j)].  All MFMAs are "swapped" as in attn_fwd.hip (keys /
// table rows as A rows, queries as B columns): a lane owns one query column and the softmax statistics take two shuffles.
// The backward recomputes the probabilities from the forward's lse (nothing of the forward is kept but lse and ctx):
//   rows pass  (same geometry)  dQ = dS.K + G1.PK with G1[r][w] = sum_{j: idx(i_r-j)=w} dS[r,j] collected in LDS; it leaves
//              Pd = dropout(P) and dS as bf16 [nh, R, Sp] in the caller's workspace (and per row its sample's first key row, klen),
//   keys pass  one thread per (key, 16 columns): dV_j = sum_r Pd[r,j] dO_r, dK_j = sum_r dS[r,j] (Q_r + PQ[idx(i_r-j)]), the rows
//              of the key's sample walked in order -- every key row of the layout is written, zeros where nothing arrives,
//   table pass one wave per (head, table row w): dPK[w] = sum dS[r,j] Q_r, dPQ[w] = sum dS[r,j] K_j over the pairs with
//              idx(i_r-j) = w, the compact rows in order, 64 at a time.
// Every output element has one writer that adds in a fixed order: no atomics, identical bits on identical calls.
#include "attn_common.h"
#include "../../include/fbl_qrows.h"

namespace {
using namespace attn;

constexpr int QR_MAX_SPAN2 = 512;
constexpr int QR_LDV = 72;  // bf16 row stride of the staged V / K tile ([32 keys][64 + 8])

struct QrArgs {
  const bf16* q; long ldq;
  const int32_t* rseg; const int32_t* rpos; int R;
  const bf16* k; long ldk; const bf16* v; long ldv;
  const bf16* pk; const bf16* pq; long ldp;
  const int16_t* relidx; const int32_t* mask; const int32_t* klen; const int32_t* row0;
  float scale, p_drop; uint64_t seed; const uint64_t* seed_dev;
  bf16* ctx; long ldo; float* lse;  // forward outputs (backward: inputs, ctx = O)
  const bf16* dO; long lddo;
  bf16* dQ; long lddq; bf16* dK; long lddk; bf16* dV; long lddv;
  float* dPK; float* dPQ; int rmin, rcnt;
  bf16* pw; bf16* dsw;  // workspace [nh, R, Sp] each
  int2* rinfo;          // workspace [R]: (first key row of the row's sample in the layout, its klen)
  int B, S, Sp, nh, span2;
};

__host__ __device__ constexpr int qr_ldt(int span2) { return ((span2 + 15) & ~15) + 8; }
// LDS: relidx int16 [2*Sp] | T1 f16 [16][LDT] | T2 f16 [2][16][LDT] | tile bf16 [32][QR_LDV] | (bwd) G1 f32 [16][LDT]
__host__ __device__ constexpr int qr_smem(int Sp, int span2, bool bwd) {
  return 2 * Sp * 2 + 3 * 16 * qr_ldt(span2) * 2 + 32 * QR_LDV * 2 + (bwd ? 16 * qr_ldt(span2) * 4 : 0);
}

// the group (sample b, first compact row r0, nr rows) of workgroup x; false: x is beyond the last group
// (a segment is cut to [0, R): a plan that is not one cannot make a row index leave the compact tensors)
__device__ __forceinline__ bool qr_group(const int32_t* rseg, int B, int R, int x, int* b_out, int* r0_out, int* nr_out) {
  for (int b = 0; b < B; ++b) {
    const int s0 = clampi(rseg[b], 0, R), n = min(rseg[b + 1], R) - s0, ng = n > 0 ? (n + 15) >> 4 : 0;
    if (x < ng) {
      *b_out = b; *r0_out = s0 + x * 16; *nr_out = min(16, n - x * 16);
      return true;
    }
    x -= ng;
  }
  return false;
}

// dst[t*16 + 0..3] (fp16, this lane's row and 4-column group) = TAB[t*16 + g*4 + e] . X_c for the row tiles t in [tlo, thi]:
// A = 16 table rows (tab points at this lane's head and 8-column chunk), B = x0 / x1.  Four tiles per round, their eight
// fragment loads requested before the first MFMA (one memory latency per round; a round past thi repeats the last tile).
__device__ __forceinline__ void table_tiles(const bf16* tab, long ldp, int span2, int tlo, int thi, bf16x8 x0, bf16x8 x1, f16* dst,
                                            int c) {
  for (int t = tlo; t <= thi; t += 4) {
    bf16x8 f0[4], f1[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const long ro = (long)min(min(t + u, thi) * 16 + c, span2 - 1) * ldp;
      f0[u] = *(const bf16x8*)(tab + ro);
      f1[u] = *(const bf16x8*)(tab + ro + 32);
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      f32x4 acc = (f32x4){0.f, 0.f, 0.f, 0.f};
      acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(f0[u], x0, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(f1[u], x1, acc, 0, 0, 0);
      *(f16x4*)(dst + min(t + u, thi) * 16) = to_f16x4(acc);
    }
  }
}

template <bool BWD>
__global__ __launch_bounds__(64) void qrows_kernel(QrArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int lane = threadIdx.x, c = lane & 15, g = lane >> 4;
  const int h = blockIdx.y, S = a.S, Sp = a.Sp, LDT = qr_ldt(a.span2);
  int b, r0, nr;
  if (!qr_group(a.rseg, a.B, a.R, blockIdx.x, &b, &r0, &nr)) return;

  int16_t* idx = (int16_t*)smem;
  f16* T1 = (f16*)(smem + 2 * Sp * 2);
  f16* T2 = T1 + 16 * LDT;
  bf16* tile = (bf16*)(T2 + 2 * 16 * LDT);
  float* G1 = (float*)(tile + 32 * QR_LDV);

  const bool packed = a.row0 != nullptr;
  const long rb = packed ? (long)a.row0[b] : (long)b * S;
  const int lim = packed ? min(a.row0[b + 1] - a.row0[b], S) : S;
  const int kl = min(min(a.klen[b], S), lim);
  const int r = r0 + min(c, nr - 1);  // this lane's compact row (lanes beyond the group repeat its last row and store nothing)
  const bool rowok = c < nr;
  const int pos = clampi(a.rpos[r], 0, S - 1);
  const bool qvalid = rowok && a.mask[(long)b * S + pos] != 0;
  int imin = pos, imax = pos;
#pragma unroll
  for (int o = 1; o < 16; o <<= 1) {
    imin = min(imin, __shfl_xor(imin, o, 64));
    imax = max(imax, __shfl_xor(imax, o, 64));
  }
  imin = __builtin_amdgcn_readfirstlane(imin);
  imax = __builtin_amdgcn_readfirstlane(imax);

  for (int t = lane; t < 2 * S - 1; t += 64) idx[t] = (int16_t)clampi(a.relidx[t], 0, a.span2 - 1);
  const bf16* qp = a.q + (long)r * a.ldq + h * 64 + g * 8;
  const bf16x8 qf[2] = {*(const bf16x8*)qp, *(const bf16x8*)(qp + 32)};
  bf16x8 dof[2];
  float Dr = 0.f, lse_r = INFINITY;
  if constexpr (BWD) {
    const bf16* dp = a.dO + (long)r * a.lddo + h * 64 + g * 8;
    const bf16* op = a.ctx + (long)r * a.ldo + h * 64 + g * 8;
    dof[0] = *(const bf16x8*)dp;
    dof[1] = *(const bf16x8*)(dp + 32);
    const bf16x8 o0 = *(const bf16x8*)op, o1 = *(const bf16x8*)(op + 32);
#pragma unroll
    for (int e = 0; e < 8; ++e) Dr += bf2f(dof[0][e]) * bf2f(o0[e]) + bf2f(dof[1][e]) * bf2f(o1[e]);
    Dr += __shfl_xor(Dr, 16, 64);
    Dr += __shfl_xor(Dr, 32, 64);
    lse_r = a.lse[(long)h * a.R + r];
    if (h == 0 && g == 0 && rowok) a.rinfo[r] = make_int2((int)rb, kl);
    for (int t = lane; t < 16 * LDT; t += 64) G1[t] = 0.f;
  }
  __syncthreads();  // index table (and G1) visible

  const bf16* pkh = a.pk + h * 64 + g * 8;
  const bf16* pqh = a.pq + h * 64 + g * 8;
  const int tq = S - 1;
  // ---- T1 over the table rows this group reaches: idx is monotone in delta, deltas span [imin - (kl-1), imax]
  const int w1lo = kl > 0 ? idx[clampi(imin - (kl - 1) + tq, 0, 2 * S - 2)] : 0;
  const int w1hi = kl > 0 ? idx[imax + tq] : -1;
  table_tiles(pkh, a.ldp, a.span2, w1lo >> 4, w1hi >> 4, qf[0], qf[1], T1 + c * LDT + g * 4, c);

  const DropKey dk = attn_drop_key(a.p_drop > 0.f ? fbl_seed(a.seed, a.seed_dev) : 0, b * a.nh + h, a.p_drop);
  const float k2 = a.scale * LOG2E;
  float m_run = -INFINITY, l_run = 0.f;
  f32x4 o[4];  // forward: ctx^T, backward: (dS.K)^T -- o[dt][e] <-> column dt*16 + g*4 + e of this lane's query
#pragma unroll
  for (int dt = 0; dt < 4; ++dt) o[dt] = (f32x4){0.f, 0.f, 0.f, 0.f};

  const int nkt = (kl + 31) >> 5;
  for (int jt = 0; jt < nkt; ++jt) {
    const int j0 = jt * 32;
    // K fragments of the two 16-key sub-tiles (A rows = keys), V likewise in the backward
    bf16x8 ka[2][2], va[2][2];
#pragma unroll
    for (int nt = 0; nt < 2; ++nt) {
      const long row = rb + min(j0 + nt * 16 + c, lim - 1);
      const bf16* kp = a.k + row * a.ldk + h * 64 + g * 8;
      ka[nt][0] = *(const bf16x8*)kp;
      ka[nt][1] = *(const bf16x8*)(kp + 32);
      if constexpr (BWD) {
        const bf16* vp = a.v + row * a.ldv + h * 64 + g * 8;
        va[nt][0] = *(const bf16x8*)vp;
        va[nt][1] = *(const bf16x8*)(vp + 32);
      }
    }
    // the staged row-major tile of the second product: V (forward: ctx += P.V), K (backward: dQ += dS.K)
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int id = lane + 64 * u, row = id >> 3, ch = id & 7;
      const long grow = rb + min(j0 + row, lim - 1);
      const bf16* src = BWD ? a.k + grow * a.ldk : a.v + grow * a.ldv;
      *(bf16x8*)(tile + row * QR_LDV + ch * 8) = *(const bf16x8*)(src + h * 64 + ch * 8);
    }
    f32x4 sacc[2], dpacc[2];
#pragma unroll
    for (int nt = 0; nt < 2; ++nt) {
      f32x4 acc = (f32x4){0.f, 0.f, 0.f, 0.f};
      acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ka[nt][0], qf[0], acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ka[nt][1], qf[1], acc, 0, 0, 0);
      sacc[nt] = acc;
      if constexpr (BWD) {
        f32x4 d = (f32x4){0.f, 0.f, 0.f, 0.f};
        d = __builtin_amdgcn_mfma_f32_16x16x32_bf16(va[nt][0], dof[0], d, 0, 0, 0);
        d = __builtin_amdgcn_mfma_f32_16x16x32_bf16(va[nt][1], dof[1], d, 0, 0, 0);
        dpacc[nt] = d;
      }
      // T2 of this sub-tile: keys [jl, jl+15] against the table rows idx(imin - jh) .. idx(imax - jl)
      const int jl = j0 + nt * 16, jh = min(jl + 15, S - 1);
      if (jl < kl) {
        const int w2lo = idx[clampi(imin - jh + tq, 0, 2 * S - 2)], w2hi = idx[imax - jl + tq];
        table_tiles(pqh, a.ldp, a.span2, w2lo >> 4, w2hi >> 4, ka[nt][0], ka[nt][1], T2 + (nt * 16 + c) * LDT + g * 4, c);
      }
    }
    __syncthreads();  // T1 (first tile), T2 and the staged tile visible

    // ---- scores of this lane's query against keys j0 + nt*16 + g*4 + e
    float p[8], kf[8];
    int ix[8];
    float mx = -INFINITY;
#pragma unroll
    for (int nt = 0; nt < 2; ++nt)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int j = j0 + nt * 16 + g * 4 + e;
        const bool kv = j < kl && a.mask[(long)b * S + min(j, S - 1)] != 0;
        const int w = idx[clampi(pos - j + tq, 0, 2 * S - 2)];
        ix[nt * 4 + e] = w;
        float s = -INFINITY;
        if (kv) s = sacc[nt][e] + (float)T1[c * LDT + w] + (float)T2[(nt * 16 + g * 4 + e) * LDT + w];
        p[nt * 4 + e] = s;
        mx = fmaxf(mx, s);
        kf[nt * 4 + e] = 1.f;
      }
    if (a.p_drop > 0.f) {
#pragma unroll
      for (int nt = 0; nt < 2; ++nt)
#pragma unroll
        for (int bb = 0; bb < 2; ++bb) {
          uint32_t x, y;
          attn_drop_block(dk, pos >> 1, (j0 + nt * 16 + g * 4 + bb * 2) >> 1, Sp >> 1, &x, &y);
          kf[nt * 4 + bb * 2] = attn_drop_keep(dk, x, y, pos & 1, 0);
          kf[nt * 4 + bb * 2 + 1] = attn_drop_keep(dk, x, y, pos & 1, 1);
        }
    }
    bf16x8 pf;  // B fragment of the second product: k-slot e <-> key (e>>2)*16 + g*4 + (e&3)
    if constexpr (!BWD) {
      mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
      mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
      const float m_new = fmaxf(m_run, mx);
      float alpha = 1.f, psum = 0.f;
      if (!(m_new > -INFINITY)) {
#pragma unroll
        for (int e = 0; e < 8; ++e) p[e] = 0.f;
      } else {
        alpha = __builtin_amdgcn_exp2f((m_run - m_new) * k2);
        const float mk = -m_new * k2;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          p[e] = __builtin_amdgcn_exp2f(fmaf(p[e], k2, mk));
          psum += p[e];
        }
      }
      psum += __shfl_xor(psum, 16, 64);
      psum += __shfl_xor(psum, 32, 64);
      l_run = l_run * alpha + psum;
      m_run = m_new;
#pragma unroll
      for (int dt = 0; dt < 4; ++dt) o[dt] *= alpha;
#pragma unroll
      for (int e = 0; e < 8; ++e) pf[e] = f2bf(p[e] * kf[e]);
    } else {
      // P from the forward's lse; dS = P * (keep * dP - D) * scale; Pd and dS leave as bf16, G1 collects dS per table row
      const float ml = -lse_r * LOG2E;
      bf16x4 pd4[2], ds4[2];
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float pe = (qvalid && p[e] > -INFINITY) ? __builtin_amdgcn_exp2f(fmaf(p[e], k2, ml)) : 0.f;
        const float ds = pe * (kf[e] * dpacc[e >> 2][e & 3] - Dr) * a.scale;
        pd4[e >> 2][e & 3] = f2bf(pe * kf[e]);
        ds4[e >> 2][e & 3] = f2bf(ds);
        pf[e] = ds4[e >> 2][e & 3];
      }
      if (rowok) {
        const long wo = ((long)h * a.R + r) * Sp + j0 + g * 4;
#pragma unroll
        for (int nt = 0; nt < 2; ++nt) {
          *(bf16x4*)(a.pw + wo + nt * 16) = pd4[nt];
          *(bf16x4*)(a.dsw + wo + nt * 16) = ds4[nt];
        }
      }
      // the four lanes of a query may meet in one table row: one lane group at a time, in order
      for (int gg = 0; gg < 4; ++gg) {
        if (g == gg) {
#pragma unroll
          for (int e = 0; e < 8; ++e) G1[c * LDT + ix[e]] += bf2f(pf[e]);
        }
        __syncthreads();
      }
    }
    // ---- second product, transposed: o^T[d][query] += tile^T[d][key] . pf[key][query]
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) {
      bf16x8 tf;
#pragma unroll
      for (int e = 0; e < 8; ++e) tf[e] = tile[((e >> 2) * 16 + g * 4 + (e & 3)) * QR_LDV + dt * 16 + c];
      o[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(tf, pf, o[dt], 0, 0, 0);
    }
    __syncthreads();  // T2 and the staged tile are overwritten by the next key tile
  }

  if constexpr (!BWD) {
    const bool live = qvalid && l_run > 0.f;
    const float inv_l = live ? 1.f / l_run : 0.f;
    if (rowok) {
      bf16* op = a.ctx + (long)r * a.ldo + h * 64 + g * 4;
#pragma unroll
      for (int dt = 0; dt < 4; ++dt) {
        f32x4 v = o[dt] * inv_l;
        if (!live) v = (f32x4){0.f, 0.f, 0.f, 0.f};  // masked query rows are exactly zero
        *(bf16x4*)(op + dt * 16) = (bf16x4){f2bf(v[0]), f2bf(v[1]), f2bf(v[2]), f2bf(v[3])};
      }
      if (g == 0) a.lse[(long)h * a.R + r] = live ? m_run * a.scale + __logf(l_run) : INFINITY;
    }
  } else {
    // dQ += G1 . PK over the table rows the group reached
#pragma unroll 4
    for (int w = w1lo; w <= w1hi; ++w) {
      const float g1 = G1[c * LDT + w];
      const bf16* pr = a.pk + (long)min(w, a.span2 - 1) * a.ldp + h * 64 + g * 4;
#pragma unroll
      for (int dt = 0; dt < 4; ++dt) {
        const bf16x4 t = *(const bf16x4*)(pr + dt * 16);
#pragma unroll
        for (int e = 0; e < 4; ++e) o[dt][e] = fmaf(g1, bf2f(t[e]), o[dt][e]);
      }
    }
    if (rowok) {
      bf16* qo = a.dQ + (long)r * a.lddq + h * 64 + g * 4;
#pragma unroll
      for (int dt = 0; dt < 4; ++dt) {
        f32x4 v = o[dt];
        if (!qvalid) v = (f32x4){0.f, 0.f, 0.f, 0.f};
        *(bf16x4*)(qo + dt * 16) = (bf16x4){f2bf(v[0]), f2bf(v[1]), f2bf(v[2]), f2bf(v[3])};
      }
    }
  }
}

// keys pass: thread (key jl = tid/4 of a 16-key tile, columns dc*16 .. +15); grid (key tiles, nh, B)
__global__ __launch_bounds__(64) void qrows_bwd_keys_kernel(QrArgs a) {
  const int jl = threadIdx.x >> 2, dc = threadIdx.x & 3;
  const int b = blockIdx.z, h = blockIdx.y, j = blockIdx.x * 16 + jl, S = a.S, Sp = a.Sp;
  const bool packed = a.row0 != nullptr;
  const long rb = packed ? (long)a.row0[b] : (long)b * S;
  const int lim = packed ? min(a.row0[b + 1] - a.row0[b], S) : S;
  if (j >= lim) return;  // the layout has no such row
  const int kl = min(min(a.klen[b], S), lim);
  float dk[16], dv[16];
#pragma unroll
  for (int e = 0; e < 16; ++e) dk[e] = dv[e] = 0.f;
  if (j < kl && a.mask[(long)b * S + j] != 0) {
    const int s0 = clampi(a.rseg[b], 0, a.R), s1 = min(a.rseg[b + 1], a.R);
    const int col = h * 64 + dc * 16;
    for (int r = s0; r < s1; r += 4) {  // four rows per round: their loads are requested level by level, not row by row
      float pd[4], ds[4];
      int w[4], rr[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        rr[u] = min(r + u, s1 - 1);
        const long wo = ((long)h * a.R + rr[u]) * Sp + j;
        const bool on = r + u < s1;
        pd[u] = on ? bf2f(a.pw[wo]) : 0.f;
        ds[u] = on ? bf2f(a.dsw[wo]) : 0.f;
        w[u] = clampi(a.rpos[rr[u]], 0, S - 1);
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) w[u] = clampi(a.relidx[w[u] - j + S - 1], 0, a.span2 - 1);
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const bf16* dop = a.dO + (long)rr[u] * a.lddo + col;
        const bf16* qp = a.q + (long)rr[u] * a.ldq + col;
        const bf16* pqp = a.pq + (long)w[u] * a.ldp + col;
#pragma unroll
        for (int x = 0; x < 2; ++x) {
          const bf16x8 d8 = *(const bf16x8*)(dop + x * 8), q8 = *(const bf16x8*)(qp + x * 8), t8 = *(const bf16x8*)(pqp + x * 8);
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            dv[x * 8 + e] = fmaf(pd[u], bf2f(d8[e]), dv[x * 8 + e]);
            dk[x * 8 + e] = fmaf(ds[u], bf2f(q8[e]) + bf2f(t8[e]), dk[x * 8 + e]);
          }
        }
      }
    }
  }
  bf16* kp = a.dK + (rb + j) * a.lddk + h * 64 + dc * 16;
  bf16* vp = a.dV + (rb + j) * a.lddv + h * 64 + dc * 16;
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    bf16x8 k8, v8;
#pragma unroll
    for (int e = 0; e < 8; ++e) { k8[e] = f2bf(dk[u * 8 + e]); v8[e] = f2bf(dv[u * 8 + e]); }
    *(bf16x8*)(kp + u * 8) = k8;
    *(bf16x8*)(vp + u * 8) = v8;
  }
}

// table pass: one wave per (table row w = rmin + blockIdx.x, head); lane = column d.  The pairs (r, j) with idx(i_r - j) = w are,
// for every row r, the keys j = i_r - delta with delta in [dlo, dhi) (idx is monotone): lanes look up 64 rows at a time, the
// non-zero dS values are then broadcast one by one (four in flight) and multiplied into Q_r and K_j.
__global__ __launch_bounds__(64) void qrows_bwd_table_kernel(QrArgs a) {
  const int lane = threadIdx.x, h = blockIdx.y, wi = blockIdx.x, w = a.rmin + wi, S = a.S, Sp = a.Sp;
  // dlo = first delta with idx >= w, dhi = first delta with idx > w   (as offsets t = delta + S - 1 into relidx)
  int lo = 0, hi = 2 * S - 1;
  while (lo < hi) { const int m = (lo + hi) >> 1; if (clampi(a.relidx[m], 0, a.span2 - 1) >= w) hi = m; else lo = m + 1; }
  const int tlo = lo;
  hi = 2 * S - 1;
  while (lo < hi) { const int m = (lo + hi) >> 1; if (clampi(a.relidx[m], 0, a.span2 - 1) > w) hi = m; else lo = m + 1; }
  const int dlo = tlo - (S - 1), dhi = lo - (S - 1);
  float apk = 0.f, apq = 0.f;
  const int Rv = clampi(a.rseg[a.B], 0, a.R);  // the rows the rows pass has seen
  if (dhi > dlo)
    for (int base = 0; base < Rv; base += 64) {
      const int r = min(base + lane, Rv - 1);
      const int pos = clampi(a.rpos[r], 0, S - 1);
      const int2 ri = a.rinfo[r];  // (first key row of the sample, klen), left by the rows pass
      const int jlo = max(0, pos - dhi + 1), jhi = min(ri.y - 1, pos - dlo);
      const int n = (base + lane < Rv) ? max(0, jhi - jlo + 1) : 0;
      int nmax = n;
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) nmax = max(nmax, __shfl_xor(nmax, o, 64));
      const bf16* dsrow = a.dsw + ((long)h * a.R + r) * Sp + jlo;
      const int krow = ri.x + jlo;  // key row of the first pair in the layout
      for (int t = 0; t < nmax; ++t) {
        const float ds = t < n ? bf2f(dsrow[t]) : 0.f;
        uint64_t live = __ballot(ds != 0.f);
        while (live) {
          float dsv[4];
          int rr[4], kk[4], l = 0;
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            const bool on = live != 0;  // (a spent slot re-reads the pair in front of it, times 0)
            if (on) l = __builtin_ctzll(live);
            dsv[u] = on ? __shfl(ds, l, 64) : 0.f;
            rr[u] = base + l;
            kk[u] = __shfl(krow, l, 64) + t;
            live &= live - 1;
          }
          float qv[4], kv[4];
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            qv[u] = bf2f(a.q[(long)rr[u] * a.ldq + h * 64 + lane]);
            kv[u] = bf2f(a.k[(long)kk[u] * a.ldk + h * 64 + lane]);
          }
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            apk = fmaf(dsv[u], qv[u], apk);
            apq = fmaf(dsv[u], kv[u], apq);
          }
        }
      }
    }
  a.dPK[((long)h * a.rcnt + wi) * 64 + lane] = apk;
  a.dPQ[((long)h * a.rcnt + wi) * 64 + lane] = apq;
}

inline bool mis16(const void* p) { return ((uintptr_t)p & 15) != 0; }

int qr_check(const QrArgs& a) {
  if (!a.rseg || !a.rpos || !a.klen) return FBL_ERR_ARG;
  if (a.R < 0) return FBL_ERR_ARG;
  if (!(a.p_drop >= 0.f && a.p_drop < 1.f)) return FBL_ERR_ARG;
  if (!grid_shape_ok(a.S, a.Sp) || a.span2 < 1 || a.span2 > QR_MAX_SPAN2) return FBL_ERR_SHAPE;
  if ((a.ldq % 8) || (a.ldk % 8) || (a.ldv % 8) || (a.ldp % 8) || (a.ldo % 8)) return FBL_ERR_ALIGN;
  if (mis16(a.q) || mis16(a.k) || mis16(a.v) || mis16(a.pk) || mis16(a.pq) || mis16(a.ctx)) return FBL_ERR_ALIGN;
  if (!a.q || !a.k || !a.v || !a.pk || !a.pq || !a.relidx || !a.mask || !a.ctx || !a.lse) return FBL_ERR_ARG;
  return 0;
}

// what the forward and the backward entry point take alike: the operands of the scores, the dropout seed, the shape
QrArgs qr_inputs(const void* q, int64_t ldq, const int32_t* rseg, const int32_t* rpos, int R, const void* k, int64_t ldk, const void* v,
                 int64_t ldv, const void* pk, const void* pq, int64_t ldp, const int16_t* relidx, const int32_t* mask,
                 const int32_t* klen, const int32_t* row0, float scale, float p_drop, uint64_t seed, const uint64_t* seed_dev, int B,
                 int S, int Sp, int nh, int span2) {
  QrArgs a{};
  a.q = (const bf16*)q; a.ldq = ldq; a.rseg = rseg; a.rpos = rpos; a.R = R;
  a.k = (const bf16*)k; a.ldk = ldk; a.v = (const bf16*)v; a.ldv = ldv;
  a.pk = (const bf16*)pk; a.pq = (const bf16*)pq; a.ldp = ldp;
  a.relidx = relidx; a.mask = mask; a.klen = klen; a.row0 = row0;
  a.scale = scale; a.p_drop = p_drop; a.seed = seed; a.seed_dev = seed_dev;
  a.B = B; a.S = S; a.Sp = Sp; a.nh = nh; a.span2 = span2;
  return a;
}

template <bool BWD>
int qr_launch_rows(const QrArgs& a, hipStream_t st) {
  // an upper bound of the number of 16-row groups that needs no look at rseg: sum_b ceil(n_b / 16) <= R / 16 + B
  dim3 grid((unsigned)(a.R / 16 + a.B), (unsigned)a.nh);
  return fbl_launch<qrows_kernel<BWD>>(grid, dim3(64), qr_smem(a.Sp, a.span2, BWD), st, a);
}

}  // namespace

extern "C" int fbl_disent_attn_fwd_qrows(const void* q, int64_t ldq, const int32_t* rseg, const int32_t* rpos, int R, const void* k,
                                         int64_t ldk, const void* v, int64_t ldv, const void* pk, const void* pq, int64_t ldp,
                                         const int16_t* relidx, const int32_t* mask, const int32_t* klen, const int32_t* row0,
                                         float scale, float p_drop, uint64_t seed, const uint64_t* seed_dev, void* ctx, int64_t ldo,
                                         float* lse, int B, int S, int Sp, int nh, int span2, void* stream) {
  QrArgs a = qr_inputs(q, ldq, rseg, rpos, R, k, ldk, v, ldv, pk, pq, ldp, relidx, mask, klen, row0, scale, p_drop, seed, seed_dev, B, S,
                       Sp, nh, span2);
  a.ctx = (bf16*)ctx; a.ldo = ldo; a.lse = lse;
  if (int e = qr_check(a)) return e;
  if (B <= 0 || nh <= 0 || R == 0) return 0;
  return qr_launch_rows<false>(a, (hipStream_t)stream);
}

extern "C" int64_t fbl_disent_attn_bwd_qrows_ws_bytes(int R, int Sp, int nh) {
  if (R <= 0 || Sp <= 0 || nh <= 0) return 0;
  return 2 * (int64_t)nh * R * Sp * (int64_t)sizeof(bf16) + (int64_t)R * (int64_t)sizeof(int2);
}

extern "C" int fbl_disent_attn_bwd_qrows(const void* q, int64_t ldq, const int32_t* rseg, const int32_t* rpos, int R, const void* k,
                                         int64_t ldk, const void* v, int64_t ldv, const void* pk, const void* pq, int64_t ldp,
                                         const int16_t* relidx, const int32_t* mask, const int32_t* klen, const int32_t* row0,
                                         const void* dO, int64_t lddo, const void* O, int64_t ldo, const float* lse, float scale,
                                         float p_drop, uint64_t seed, const uint64_t* seed_dev, void* dQ, int64_t lddq, void* dK,
                                         int64_t lddk, void* dV, int64_t lddv, float* dPK, float* dPQ, int rmin, int rcnt, void* ws,
                                         int64_t ws_bytes, int B, int S, int Sp, int nh, int span2, void* stream) {
  QrArgs a = qr_inputs(q, ldq, rseg, rpos, R, k, ldk, v, ldv, pk, pq, ldp, relidx, mask, klen, row0, scale, p_drop, seed, seed_dev, B, S,
                       Sp, nh, span2);
  a.ctx = (bf16*)O; a.ldo = ldo; a.lse = (float*)lse;
  a.dO = (const bf16*)dO; a.lddo = lddo;
  a.dQ = (bf16*)dQ; a.lddq = lddq; a.dK = (bf16*)dK; a.lddk = lddk; a.dV = (bf16*)dV; a.lddv = lddv;
  a.dPK = dPK; a.dPQ = dPQ; a.rmin = rmin; a.rcnt = rcnt;
  if (int e = qr_check(a)) return e;
  if ((lddo % 8) || (lddq % 8) || (lddk % 8) || (lddv % 8)) return FBL_ERR_ALIGN;
  if (mis16(dO) || mis16(dQ) || mis16(dK) || mis16(dV) || mis16(ws)) return FBL_ERR_ALIGN;
  if (!dO || !dQ || !dK || !dV || ((dPK == nullptr) != (dPQ == nullptr))) return FBL_ERR_ARG;
  if (dPK && (rmin < 0 || rcnt < 1 || rmin + rcnt > span2)) return FBL_ERR_ARG;
  if (B <= 0 || nh <= 0 || R == 0) return 0;  // nothing selected: nothing is launched, nothing is written
  if (!ws || ws_bytes < fbl_disent_attn_bwd_qrows_ws_bytes(R, Sp, nh)) return FBL_ERR_ARG;
  a.pw = (bf16*)ws;
  a.dsw = a.pw + (int64_t)nh * R * Sp;
  a.rinfo = (int2*)(a.dsw + (int64_t)nh * R * Sp);  // (Sp % 64 == 0: 8-byte aligned)
  hipStream_t st = (hipStream_t)stream;
  if (int e = qr_launch_rows<true>(a, st)) return e;
  hipLaunchKernelGGL(qrows_bwd_keys_kernel, dim3((unsigned)((S + 15) / 16), (unsigned)nh, (unsigned)B), dim3(64), 0, st, a);
  FBL_CHECK_LAUNCH();
  if (dPK) {  // (both NULL: the caller has nothing trainable behind the position tables)
    hipLaunchKernelGGL(qrows_bwd_table_kernel, dim3((unsigned)rcnt, (unsigned)nh), dim3(64), 0, st, a);
    FBL_CHECK_LAUNCH();
  }
  return 0;
}
