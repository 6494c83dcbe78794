// bf16 MFMA GEMM for gfx950:  C[M,N] = epilogue( alpha * A[M,K] . B[N,K]^T )   ("NT": both operands K-contiguous)
//
// This one kernel serves every dense contraction of the FrozenBiLM hot path (reference: the nn.Linear calls of
// model/deberta.py:255,311,329,757-765,847-853,1545 and model/adapter.py:38,42; their backward dX = dY.W is the
// same kernel on the pre-transposed frozen weight).
//
// Structure (CDNA4): 128x128x64 tile, 256 threads = 4 waves (2x2), each wave 64x64 = 4x4 v_mfma_f32_16x16x32_bf16
// accumulators.  Operand tiles go HBM -> LDS with global_load_lds_dwordx4 (no VGPR round trip), double-buffered,
// one barrier per K-step.  LDS image is [128 rows][8 x 16B chunks] with chunk ^= row&7 applied on the SOURCE
// address (LDS-DMA destinations are lane-linear) and again on the ds_read_b128 side -> conflict-free fragment reads.
// MFMA operands are swapped (weights as "A", activations as "B") so each lane owns 4 consecutive output columns
// -> 16-byte fp32 / 8-byte bf16 epilogue stores.
#include "gemm_common.h"

using namespace fblgemm;

namespace {

// Tile configurations (NW waves, wave grid WR x WC, each wave (MI*16) x 64 outputs; BM = BN = 32*NW):
//   small: 128x128, 4 waves (2x2), MI=4  -> 69.6 KiB LDS, 2 workgroups/CU   (narrow / short GEMMs)
//   big:   256x256, 8 waves (2x4), MI=8  -> 136 KiB LDS, 1 workgroup/CU     (1/3 fewer LDS bytes per MFMA)
// (the large square-ish problems run the 8-phase kernel of gemm8.hip instead of the NW = 8 configuration)
template <int NW> struct TileCfg {
  static constexpr int BM = 32 * NW, BN = 32 * NW;
  static constexpr int TILE_BYTES = BM * BK * 2;
  static constexpr int STAGE_BYTES = 2 * TILE_BYTES;
  static constexpr int SMEM_BYTES = (NW * 64 * 68 * 4 > 2 * STAGE_BYTES) ? NW * 64 * 68 * 4 : 2 * STAGE_BYTES;
};

// MI: 16-row MFMA tiles per wave along M.  The tile is (32*MI) x (32*NW); MI = NW gives the square 128/256 tiles,
// MI = 7 with NW = 8 a 224x256 tile for shapes whose 256x256 grid leaves CUs idle (8512 rows = 38 x 224 exactly:
// 228 tiles on 256 CUs for N = 1536 instead of 204 bigger ones).  LDS keeps the 32*NW-row A image; the unused rows are
// simply not fetched.
// RING: the 3-stage ring main loop of the tall, narrow problems (MI = 2, NW = 4: 64x128 tiles) instead of the 2-stage loop.
template <int NW, int ACT, int AUX, bool SPLITK, bool RING, int MI>
__global__ __launch_bounds__(NW * 64, 2) void gemm_bf16_nt_kernel(GemmArgs g) {
  using Cfg = TileCfg<NW>;
  constexpr int BM = 32 * MI;
  // LDS stage = A image | B image.  The 2-stage loop reserves the square tile's A image even for shorter tiles; the
  // ring packs the BM rows it really has (three stages of 24 KiB: two workgroups per CU still fit)
  constexpr int BN = Cfg::BN;
  constexpr int TILE_BYTES = RING ? BM * BK * 2 : Cfg::TILE_BYTES;
  constexpr int STAGE_BYTES = RING ? TILE_BYTES + Cfg::TILE_BYTES : Cfg::STAGE_BYTES;
  constexpr int WC = NW / 2;        // waves along N (2 rows of waves along M)
  constexpr int WROWS = MI * 16;    // rows of C per wave
  extern __shared__ __attribute__((aligned(16))) char smem[];  // 2 stages x (A tile | B tile)
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave / WC, wn = wave % WC;

  int tm, tn;
  tile_of_block(blockIdx.x, g.tiles_m, g.tiles_n, &tm, &tn);
  const int m0 = tm * BM, n0 = tn * BN;

  const int batch = blockIdx.y / g.splitk;
  const int ks = blockIdx.y % g.splitk;
  const int nk_total = g.K / BK;
  const int per = (nk_total + g.splitk - 1) / g.splitk;
  const int kt0 = ks * per;
  const int kt1 = min(nk_total, kt0 + per);
  if (kt0 >= kt1) return;

  const bf16* A = g.A + (long)batch * g.sA;
  const bf16* B = g.B + (long)batch * g.sB;

  // ---- LDS-DMA source addressing: instruction q covers rows (q*4+wave)*8 .. +8; lane -> row lane>>3, phys chunk lane&7
  const int lrow = lane >> 3;
  const int lchunk = (lane & 7) ^ lrow;  // logical 16B chunk fetched by this lane (row&7 == lrow)
  const bf16* a_src[4];
  const bf16* b_src[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int row = (q * NW + wave) * 8 + lrow;
    const int am = min(m0 + row, g.M - 1);
    const int bn = min(n0 + row, g.N - 1);
    a_src[q] = A + (long)am * g.lda + lchunk * 8;
    b_src[q] = B + (long)bn * g.ldb + lchunk * 8;
  }
  auto issue = [&](int kt, int stage) {
    char* base = smem + stage * STAGE_BYTES;
    const long koff = (long)kt * BK;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int off = (q * NW + wave) * 1024;
      if ((q * NW + wave) * 8 < BM) glds16(a_src[q] + koff, base + off);  // (always true for the square tiles)
      glds16(b_src[q] + koff, base + TILE_BYTES + off);
    }
  };

  f32x4 acc[4][MI];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < MI; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

  // fragment read offsets (bytes) inside a tile: row*128 + ((s*4 + lane>>4) ^ (row&7))*16
  const int frow = lane & 15, fg = lane >> 4, fsw = lane & 7;
  const int a_off0 = (wm * WROWS + frow) * 128;                 // + i*16*128 per M tile
  const int b_off0 = TILE_BYTES + (wn * 64 + frow) * 128;       // + i*16*128 per N tile

  auto mfma_block = [&](const bf16x8* af, const bf16x8* bfg) {
#pragma unroll
    for (int mi = 0; mi < MI; ++mi)
#pragma unroll
      for (int ni = 0; ni < 4; ++ni)
        acc[ni][mi] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bfg[ni], af[mi], acc[ni][mi], 0, 0, 0);
  };
  auto read_frags = [&](const char* base, int s_, bf16x8* af, bf16x8* bfg) {
    const int pc = ((s_ * 4 + fg) ^ fsw) * 16;
#pragma unroll
    for (int i = 0; i < 4; ++i) bfg[i] = *(const bf16x8*)(base + b_off0 + i * 2048 + pc);
#pragma unroll
    for (int i = 0; i < MI; ++i) af[i] = *(const bf16x8*)(base + a_off0 + i * 2048 + pc);
  };
  if constexpr (RING) {
    // ---- ring of NS = 3 stages for the tall, narrow problems (adapter bottleneck projections: about one 64x128 workgroup
    // per CU, so nothing else on the CU hides a load): two K-steps of operands in flight, ONE raw barrier per K-step.
    //   iteration kt:  wait until stage kt has landed (one younger stage may stay in flight) -> barrier (every wave's part
    //   of stage kt is in LDS AND every wave is done reading stage kt-1) -> request stage kt+2 into the slot of kt-1 ->
    //   fragments + MFMAs of stage kt.
    constexpr int NS = 3;
    constexpr int PS = 4 + ((BM + NW * 8 - 1) / (NW * 8) < 4 ? (BM + NW * 8 - 1) / (NW * 8) : 4);  // LDS-DMA requests per thread and stage
    static_assert(PS == 6, "the vmcnt immediates below are written for the 64-row configuration (2 A + 4 B requests)");
#pragma unroll
    for (int s_ = 0; s_ < NS - 1; ++s_)
      if (kt0 + s_ < kt1) issue(kt0 + s_, s_);
    for (int kt = kt0; kt < kt1; ++kt) {
      if (kt + 1 < kt1) asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
      else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
      asm volatile("" ::: "memory");
      if (kt + NS - 1 < kt1) issue(kt + NS - 1, (kt - kt0 + NS - 1) % NS);
      const char* base = smem + ((kt - kt0) % NS) * STAGE_BYTES;
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        bf16x8 af[MI], bfg[4];
        read_frags(base, s, af, bfg);
        mfma_block(af, bfg);
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // this wave's fragment reads of the stage are complete
    }
    __builtin_amdgcn_s_barrier();  // all LDS tile reads retired before the epilogue reuses the memory
  } else {
    issue(kt0, 0);
    __syncthreads();  // drains the LDS-DMA (vmcnt(0)) and publishes stage 0
    for (int kt = kt0; kt < kt1; ++kt) {
      const int stage = (kt - kt0) & 1;
      if (kt + 1 < kt1) issue(kt + 1, stage ^ 1);
      const char* base = smem + stage * STAGE_BYTES;
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        bf16x8 af[MI], bfg[4];
        read_frags(base, s, af, bfg);
        mfma_block(af, bfg);
      }
      __syncthreads();
    }
  }

  // ---- epilogue (gemm_common.h): slabs of 64 rows of this wave's tile through a wave-private LDS staging tile
  gemm_epilogue<ACT, AUX, SPLITK, MI>(g, smem, wave, lane, acc, m0 + wm * WROWS, 64, n0 + wn * 64 + (lane & 15) * 4, batch, ks);
}

// ---------------------------------------------------------------------------------------------------------------
// "TN" variant for the trainable-weight gradients:  C[M,N] += sum_k A[k,m] * B[k,n]   (A [K,M], B [K,N] row-major, the
// contraction runs over ROWS: dW = X^T . dY without materialising X^T / dY^T in HBM).  128x128x64 tile, 4 waves.
// Tiles are staged row-major in LDS (coalesced 16-byte global loads, next tile prefetched into registers) and the
// MFMA fragments -- 8 consecutive k for one m -- come out of the row-major image through the hardware transpose read
// ds_read_b64_tr_b16 (two per fragment).
// Always split-K with a workspace fold (accumulates into C).
struct GemmTnArgs {
  const bf16* A; const bf16* B; long lda, ldb;
  int M, N, K;
  float* ws; int Nw;  // partials [splitk][M][Nw]
  int splitk, tiles_m, tiles_n;
};
constexpr int TN_LD = 136;  // bf16 row stride of the staged [64 k][128 cols] tiles (272 B: 16B-aligned rows)

__global__ __launch_bounds__(256, 2) void gemm_bf16_tn_kernel(GemmTnArgs g) {
  __shared__ __attribute__((aligned(16))) bf16 sA[64 * TN_LD];
  __shared__ __attribute__((aligned(16))) bf16 sB[64 * TN_LD];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 1, wn = wave & 1;
  const int tm = blockIdx.x % g.tiles_m, tn = blockIdx.x / g.tiles_m;
  const int m0 = tm * 128, n0 = tn * 128;
  const int ks = blockIdx.y;
  const int nk = (g.K + 63) / 64;
  const int per = (nk + g.splitk - 1) / g.splitk;
  const int kt0 = ks * per, kt1 = min(nk, kt0 + per);
  const int frow = lane & 15, fg = lane >> 4;

  f32x4 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

  // staging role: 64 rows x 16 chunks(8 cols) per operand = 1024 chunks -> 4 per thread
  bf16x8 ra[4], rb[4];
  auto load_tile = [&](int kt) {
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int id = tid + t * 256;
      const int r = id >> 4, ch = id & 15;
      const int k = kt * 64 + r;
      const bool kok = k < g.K;
      const int ca = m0 + ch * 8, cb = n0 + ch * 8;
      ra[t] = (kok && ca + 8 <= g.M) ? *(const bf16x8*)(g.A + (long)k * g.lda + ca) : (bf16x8){0, 0, 0, 0, 0, 0, 0, 0};
      rb[t] = (kok && cb + 8 <= g.N) ? *(const bf16x8*)(g.B + (long)k * g.ldb + cb) : (bf16x8){0, 0, 0, 0, 0, 0, 0, 0};
    }
  };
  if (kt0 < kt1) load_tile(kt0);
  for (int kt = kt0; kt < kt1; ++kt) {
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int id = tid + t * 256;
      *(bf16x8*)(sA + (id >> 4) * TN_LD + (id & 15) * 8) = ra[t];
      *(bf16x8*)(sB + (id >> 4) * TN_LD + (id & 15) * 8) = rb[t];
    }
    __syncthreads();
    if (kt + 1 < kt1) load_tile(kt + 1);
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      bf16x8 af[4], bfg[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        // ds_read_b64_tr_b16: the 16 lanes of a group hand in the 4x16 block (rows k..k+3, 16 columns) as 16 x 8 bytes
        // and each lane gets its own column back -- 4 consecutive k of one m: two reads per MFMA fragment instead
        // of eight ds_read_u16 (semantics probed on hardware: tools/probe/tr16_probe.hip)
        const int kr = (s * 32 + fg * 8 + (frow >> 2)) * TN_LD + (frow & 3) * 4;
        const tr16x4 a0 = lds_tr16(sA + kr + wm * 64 + i * 16), a1 = lds_tr16(sA + kr + 4 * TN_LD + wm * 64 + i * 16);
        const tr16x4 b0 = lds_tr16(sB + kr + wn * 64 + i * 16), b1 = lds_tr16(sB + kr + 4 * TN_LD + wn * 64 + i * 16);
        union { tr16x4 h[2]; bf16x8 v; } ua, ub;
        ua.h[0] = a0; ua.h[1] = a1; ub.h[0] = b0; ub.h[1] = b1;
        af[i] = ua.v;
        bfg[i] = ub.v;
      }
#pragma unroll
      for (int ni = 0; ni < 4; ++ni)
#pragma unroll
        for (int mi = 0; mi < 4; ++mi)
          acc[ni][mi] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bfg[ni], af[mi], acc[ni][mi], 0, 0, 0);
    }
    __syncthreads();
  }
  // partial tile -> workspace (lane owns C[m][4 consecutive n]); rows/cols beyond M/N are skipped
#pragma unroll
  for (int mi = 0; mi < 4; ++mi) {
    const int m = m0 + wm * 64 + mi * 16 + frow;
    if (m >= g.M) continue;
#pragma unroll
    for (int ni = 0; ni < 4; ++ni) {
      const int n4 = n0 + wn * 64 + ni * 16 + fg * 4;
      if (n4 >= g.N) continue;
      *(f32x4*)(g.ws + (((long)ks * g.M + m) * g.Nw + n4)) = acc[ni][mi];
    }
  }
}

// 256x256 (or 224x256) tiles only where both dimensions fill them and the grid still covers half the chip
// (M >= 512 with a very wide N: the vocabulary GEMM of the loss on the labelled rows, [~700 x 128100 x 1536] -- 3 x 501 big tiles)
static inline bool big_tile_shape(int M, int N, int batch) {
  return batch == 1 && (M >= 2048 || (M >= 512 && N >= 16384)) && N >= 1024 &&
         ((long)((M + 255) / 256) * ((N + 255) / 256) >= 128);
}

constexpr double FBL_R128_US_PER_KTILE = 0.86;  // 128-row 8-phase tile: time per K-tile of one workgroup (measured: [5322,1536,6144] 88 us)

// CUs of the device that is current at the first call (256 if the query fails)
static int device_cu_count() {
  static const int n_cu = [] {
    int dev = 0;
    hipDeviceProp_t prop;
    if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess && prop.multiProcessorCount > 0)
      return prop.multiProcessorCount;
    return 256;
  }();
  return n_cu;
}

// out[b][m][n] += sum_ks ws[b][ks][m][n]   (deterministic split-K fold)
__global__ void splitk_reduce_kernel(const float* ws, int splitk, int M, int N, int Nw, float* out, long ldc, long sC) {
  const int b = blockIdx.y;
  const long q = (long)blockIdx.x * blockDim.x + threadIdx.x;  // float4 index inside [M][Nw/4]
  const int nq = Nw >> 2;
  if (q >= (long)M * nq) return;
  const int m = (int)(q / nq), n4 = (int)(q % nq) * 4;
  const float* p = ws + ((long)b * splitk * M + m) * Nw + n4;
  const long ks = (long)M * Nw;
  float* o = out + b * sC + (long)m * ldc + n4;
  const bool vec = (n4 + 3 < N) && ((ldc & 3) == 0) && ((sC & 3) == 0);
  f32x4 acc = vec ? *(const f32x4*)o : (f32x4){0.f, 0.f, 0.f, 0.f};
  // partials are summed in index order (deterministic); 8 independent loads in flight per thread
  int k = 0;
  for (; k + 8 <= splitk; k += 8) {
    f32x4 t[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) t[u] = *(const f32x4*)(p + (k + u) * ks);
#pragma unroll
    for (int u = 0; u < 8; ++u) acc += t[u];
  }
  for (; k < splitk; ++k) acc += *(const f32x4*)(p + k * ks);
  if (vec) {
    *(f32x4*)o = acc;
  } else {
#pragma unroll
    for (int r = 0; r < 4; ++r)
      if (n4 + r < N) o[r] += acc[r];
  }
}

}  // namespace

// Fork / join events of one (stream, aux_stream) pair.  The library owns no stream; the events are its only process
// state: created on first use for the pair (on the device that is current in the calling thread, which must be the
// streams' device), kept for the life of the process, looked up under a mutex.  One pair of events per pair of streams
// is enough: a stream is fed by one thread at a time, and re-recording an event only affects waits issued afterwards.
#include <map>
#include <mutex>
#include <utility>
static bool fork_join_events(hipStream_t s, hipStream_t aux, hipEvent_t* fork, hipEvent_t* join) {
  static std::mutex mu;
  static std::map<std::pair<hipStream_t, hipStream_t>, std::pair<hipEvent_t, hipEvent_t>> pool;
  std::lock_guard<std::mutex> lock(mu);
  auto it = pool.find({s, aux});
  if (it == pool.end()) {
    hipEvent_t f = nullptr, j = nullptr;
    if (hipEventCreateWithFlags(&f, hipEventDisableTiming) != hipSuccess) return false;
    if (hipEventCreateWithFlags(&j, hipEventDisableTiming) != hipSuccess) {
      (void)hipEventDestroy(f);
      return false;
    }
    it = pool.emplace(std::make_pair(s, aux), std::make_pair(f, j)).first;
  }
  *fork = it->second.first;
  *join = it->second.second;
  return true;
}

// ---- dispatch of the NT GEMM: a pure plan (which kernel runs which rows on which stream) and the launcher that executes it

// What runs one launch, and its tile (rows x columns)
// (the ids are public: FBL_GK_* of include/fbl.h, reported by fbl_gemm_plan_launches)
enum GemmKernel {
  G8_256 = FBL_GK_G8_256, G8_224 = FBL_GK_G8_224, G8_128 = FBL_GK_G8_128,  // 8-phase kernel (gemm8.hip), 256 columns
  G8_SPLITK = FBL_GK_G8_SPLITK,  // 8-phase 256x256 tiles, K cut into slices of GemmPlan::k8_per K-tiles, partials to the workspace
  T2_256 = FBL_GK_T2_256, T2_224 = FBL_GK_T2_224,          // 2-stage kernel, 8 waves, 256 columns
  T2_128 = FBL_GK_T2_128, T2_64_RING = FBL_GK_T2_64_RING,  // 2-stage kernel, 4 waves, 128 columns (the 64-row tiles: 3-stage ring)
  T2_128_SPLITK = FBL_GK_T2_128_SPLITK,  // 2-stage 128x128 tiles, partials to the workspace or atomically added to C
};
static int tile_rows(GemmKernel k) {
  switch (k) {
    case G8_224: case T2_224: return 224;
    case G8_128: case T2_128: case T2_128_SPLITK: return 128;
    case T2_64_RING: return 64;
    default: return 256;
  }
}
static int tile_cols(GemmKernel k) { return (k == T2_128 || k == T2_64_RING || k == T2_128_SPLITK) ? 128 : 256; }

struct GemmLaunch {
  GemmKernel kernel;
  int row0, rows;  // rows [row0, row0 + rows) of C
  int tiles_m, tiles_n;
  dim3 grid;
  bool on_aux;     // on the caller's aux stream: forked from `stream` before, joined back into it after the launches
};

struct GemmPlan {
  GemmLaunch launch[2];  // in launch order
  int n;
  int splitk, k8_per;    // K slices of every launch (G8_SPLITK: its own slicing, k8_per K-tiles per slice)
  bool fold;             // splitk_reduce_kernel folds the workspace into C after the launches
  bool big8;             // the big-tile route on the 8-phase kernel (what fbl_gemm_plan reports)
};

// What the planner needs to know about a call besides its validated GemmArgs
struct GemmCall {
  int batch;
  bool accumulate;     // C += A.B^T (split-K)
  bool dropout;        // p_drop > 0
  bool ws_given;       // the caller passed a split-K workspace pointer, used or not
  int64_t ws_floats;   // its size
  bool aux_stream;     // a second stream, distinct from `stream`, is available
  int n_cu;
};

// Pure host logic: no HIP call, no launch.
static GemmPlan plan_gemm(const GemmArgs& g, const GemmCall& c) {
  const int M = g.M, N = g.N, nk = g.K / BK, n_cu = c.n_cu;
  const bool tail = g.aux_kind == FBL_AUX_ADAPTER_TAIL;
  GemmPlan p{};
  p.splitk = g.splitk;
  p.fold = c.accumulate && g.ws;
  auto add = [&](GemmKernel k, int row0, int rows, bool on_aux) {
    const int tm = (rows + tile_rows(k) - 1) / tile_rows(k), tn = (N + tile_cols(k) - 1) / tile_cols(k);
    p.launch[p.n++] = GemmLaunch{k, row0, rows, tm, tn, dim3(tm * tn, c.batch * p.splitk), on_aux};
  };

  // big tiles only where both dimensions fill them and the grid still covers the chip
  const bool big = !c.accumulate && (!c.dropout || g.seg_n > 0 || tail) && (g.seg_n <= 0 || g.seg_n % 256 == 0) &&
                   big_tile_shape(M, N, c.batch);
  p.big8 = big && gemm8_eligible(g);
  if (big) {
    const long tn = (N + 255) / 256, t256 = tn * ((M + 255) / 256);
    // A multi-round problem of the 8-phase kernel whose partial last round still uses a good part of the chip (96..192 of 256
    // CUs; the QKV projection [9024,4608,1536]: 648 tiles of 256 rows, 738 of 224) runs as ONE plain launch instead of "whole
    // rounds + 128x128 remainder" (122 us as 224-row tiles; the split: 146).  With a nearly empty last round (FFN-up: 816
    // tiles, 48 left) the split stays better: an epilogue costs a CU 10-20 us of VALU / store time that nothing on that CU
    // overlaps, so a fourth round of full tiles (222 us) loses to three rounds plus small tiles (208 us).
    // (Rounds 2-3 delayed part of the first round by a spin-wait on the real-time clock to take the CUs out of lockstep: worth
    //  13 us on the 256-row launch, nothing on the 224-row one the problem takes now -- removed.)
    const bool single_launch = p.big8 && t256 > 256 && t256 % 256 >= 96 && t256 % 256 <= 192;
    // Wave quantisation: one 256x256 workgroup per CU, so a grid of T tiles costs ceil(T/CUs) rounds.  When the last round
    // would be less than 2/3 full, give the big tiles only as many M rows as fill whole rounds and run the remaining rows on
    // small tiles (64x128 when their 128x128 grid would leave CUs idle: 320 rows x 6144 -> 240 workgroups instead of 144).
    // The remainder runs on the caller's aux stream (if one is given), launched BEFORE the big tiles: its workgroups take their
    // CUs first, so those CUs reach their first big tile a fraction of a tile late -- the chip leaves lockstep (the epilogue of
    // a round is an HBM burst: every CU stores its tile at the same moment while the memory system idles during the main
    // loops) and the remainder costs no round of its own.  Without an aux stream it simply precedes the big tiles.
    // (A call that passes a workspace pointer is never split.)
    const long rem = t256 % n_cu;
    const int m_big = (int)((t256 - rem) / tn) * 256;  // whole rounds worth of M tiles
    if (!single_launch && !tail && !c.ws_given && t256 > n_cu && rem != 0 && rem * 3 < (long)n_cu * 2 && m_big >= 256 &&
        m_big < M && M - m_big >= 64) {
      const int m_rem = M - m_big;
      add((long)((m_rem + 127) / 128) * ((N + 127) / 128) < 200 ? T2_64_RING : T2_128, m_big, m_rem, c.aux_stream);
      GemmArgs gb = g;
      gb.M = m_big;
      // (the whole rounds keep their 256-row tiles only if their own shape still asks for big tiles)
      const GemmKernel k = !big_tile_shape(m_big, N, 1) ? T2_128
                           : (gemm8_eligible(gb) && gemm8_supports(g.act, g.aux_kind, 256)) ? G8_256 : T2_256;
      add(k, 0, m_big, false);
      return p;
    }
    // 224x256 tiles when they cover the problem in fewer (rounds x tile area) than 256x256 -- the N = 1536 GEMMs of the
    // step: 38 x 6 = 228 tiles in one round instead of 204 tiles that are 14 % bigger.  The 8-phase kernel takes the launch at
    // the first height that instantiates the epilogue (measured: [8512,1536,6144] 915 -> 1139 TFLOP/s as 256x256 8-phase
    // tiles, although only 204 of 256 CUs get one; more as 224x256).
    const long t224 = tn * ((M + 223) / 224);
    const bool r224 = ((t224 + n_cu - 1) / n_cu) * 224 * 100 < ((t256 + n_cu - 1) / n_cu) * 256 * 97;
    if (p.big8 && r224 && gemm8_supports(g.act, g.aux_kind, 224)) add(G8_224, 0, M, false);
    else if (p.big8 && gemm8_supports(g.act, g.aux_kind, 256)) add(G8_256, 0, M, false);
    else add(r224 ? T2_224 : T2_256, 0, M, false);
    return p;
  }

  const long t128 = (long)((M + 127) / 128) * ((N + 127) / 128);
  // 128-row 8-phase tiles for problems the tall tiles leave half the chip idle on (the N = 1536 dX GEMMs at the row counts
  // of packed ragged batches / small batches: M = 5322 -> 21 x 6 = 126 tiles of 256 rows, 42 x 6 = 252 of 128 rows) and
  // that would otherwise run on the 128x128 two-stage kernel.  Chosen by a two-line cost model from measured per-K-tile
  // times (tools/bench_gemm.py --set packed): rounds x (K-tiles x us per K-tile + epilogue).
  if (!c.accumulate && c.batch == 1 && !tail && g.seg_n <= 0 && !c.dropout && M >= 1024 && N >= 1024 && N <= 8192 &&
      gemm8_eligible(g) && gemm8_supports(g.act, g.aux_kind, 128)) {
    const long t8 = (long)((M + 127) / 128) * ((N + 255) / 256);
    const double us8 = (double)((t8 + n_cu - 1) / n_cu) * (nk * FBL_R128_US_PER_KTILE + 6.0);
    const double us2 = (double)((t128 + 2 * n_cu - 1) / (2 * n_cu)) * (nk * 1.17 + 5.0);
    if (us8 < 0.95 * us2) {
      add(G8_128, 0, M, false);
      return p;
    }
  }
  // Few rows against a very long K with a workspace at hand (the prediction head's backward dh = dlogits . E: [~700 x 1536 x
  // 128128]): 8-phase 256 x 256 tiles, K cut into as many slices as fill the chip (18 tiles x 14 slices), partial tiles folded by
  // splitk_reduce_kernel -- 463 -> ~235 us.
  if (c.accumulate && g.ws && c.batch == 1 && M >= 512 && N >= 1024 && nk % 2 == 0 && nk >= 128 &&
      (long)M * g.lda * 2 < (1l << 32) && (long)N * g.ldb * 2 < (1l << 32)) {
    const int tiles = ((M + 255) / 256) * ((N + 255) / 256);
    int want = n_cu / tiles;
    if (want >= 2) {
      if (want > nk / 8) want = nk / 8;
      int per = (nk + want - 1) / want;
      per += per & 1;  // even
      int s8 = (nk + per - 1) / per;
      if (nk - (s8 - 1) * per < 4) {  // a last slice of 2 K-tiles is below the kernel's shortest pipeline
        per += 2;
        s8 = (nk + per - 1) / per;
      }
      if (s8 >= 2 && per >= 8 && nk - (s8 - 1) * per >= 4 && (int64_t)s8 * M * g.Nw <= c.ws_floats) {
        p.splitk = s8;
        p.k8_per = per;
        add(G8_SPLITK, 0, M, false);
        return p;
      }
    }
  }
  if (c.accumulate) {
    add(T2_128_SPLITK, 0, M, false);
  } else {
    // 64x128 tiles for tall, narrow problems whose 128x128 grid covers less than the chip (the adapter bottleneck
    // projections: 8512 x 192 -> 134 workgroups): twice the workgroups, so twice the CUs pull operands from L2
    add(c.batch == 1 && M >= 2048 && t128 < 200 ? T2_64_RING : T2_128, 0, M, false);
  }
  return p;
}

template <int NW, int ACT, int AUX, bool SPLITK, bool RING, int MI>
static int launch_nt(const GemmArgs& g, dim3 grid, hipStream_t stream) {
  constexpr int smem_bytes = RING ? 3 * (32 * MI * BK * 2 + TileCfg<NW>::TILE_BYTES) : TileCfg<NW>::SMEM_BYTES;
  static_assert(smem_bytes >= NW * 64 * 68 * 4, "the LDS must cover the epilogue staging");
  return fbl_launch<gemm_bf16_nt_kernel<NW, ACT, AUX, SPLITK, RING, MI>>(grid, dim3(NW * 64), smem_bytes, stream, g);
}

template <int ACT, int AUX>
static int launch_two_stage(GemmKernel k, const GemmArgs& g, dim3 grid, hipStream_t stream) {
  switch (k) {
    case T2_256: return launch_nt<8, ACT, AUX, false, false, 8>(g, grid, stream);
    case T2_224: return launch_nt<8, ACT, AUX, false, false, 7>(g, grid, stream);
    case T2_64_RING: return launch_nt<4, ACT, AUX, false, true, 2>(g, grid, stream);
    default: return launch_nt<4, ACT, AUX, false, false, 4>(g, grid, stream);
  }
}

static int launch_one(const GemmLaunch& l, const GemmArgs& g, hipStream_t stream) {
  const int act = g.act, aux = g.aux_kind;
  switch (l.kernel) {
    case G8_256: return launch_gemm8(g, act, aux, 256, l.grid, stream);
    case G8_224: return launch_gemm8(g, act, aux, 224, l.grid, stream);
    case G8_128: return launch_gemm8(g, act, aux, 128, l.grid, stream);
    case G8_SPLITK: return launch_gemm8_splitk(g, stream);
    case T2_128_SPLITK: return launch_nt<4, FBL_ACT_NONE, FBL_AUX_NONE, true, false, 4>(g, l.grid, stream);
    default: break;
  }
  const GemmKernel k = l.kernel;
  if (act == FBL_ACT_GELU && aux == FBL_AUX_NONE) return launch_two_stage<FBL_ACT_GELU, FBL_AUX_NONE>(k, g, l.grid, stream);
  if (act == FBL_ACT_RELU && aux == FBL_AUX_NONE) return launch_two_stage<FBL_ACT_RELU, FBL_AUX_NONE>(k, g, l.grid, stream);
  if (act == FBL_ACT_GELU_GRAD && aux == FBL_AUX_NONE) return launch_two_stage<FBL_ACT_GELU_GRAD, FBL_AUX_NONE>(k, g, l.grid, stream);
  if (act != FBL_ACT_NONE) return FBL_ERR_ARG;
  switch (aux) {
    case FBL_AUX_NONE: return launch_two_stage<FBL_ACT_NONE, FBL_AUX_NONE>(k, g, l.grid, stream);
    case FBL_AUX_MUL_BF16: return launch_two_stage<FBL_ACT_NONE, FBL_AUX_MUL_BF16>(k, g, l.grid, stream);
    case FBL_AUX_ADD_F32: return launch_two_stage<FBL_ACT_NONE, FBL_AUX_ADD_F32>(k, g, l.grid, stream);
    case FBL_AUX_ADD_BF16: return launch_two_stage<FBL_ACT_NONE, FBL_AUX_ADD_BF16>(k, g, l.grid, stream);
    case FBL_AUX_MUL_DGELU_BF16: return launch_two_stage<FBL_ACT_NONE, FBL_AUX_MUL_DGELU_BF16>(k, g, l.grid, stream);
    case FBL_AUX_MUL_POS_BF16: return launch_two_stage<FBL_ACT_NONE, FBL_AUX_MUL_POS_BF16>(k, g, l.grid, stream);
    case FBL_AUX_ADAPTER_TAIL: return launch_two_stage<FBL_ACT_NONE, FBL_AUX_ADAPTER_TAIL>(k, g, l.grid, stream);
    default: return FBL_ERR_ARG;
  }
}

// The arguments of one launch of the plan: rows [row0, row0 + rows) of every row-indexed operand, dropout keys of the global
// rows.  (The adapter tail, whose residual operands are row-indexed too, is never split.)
static GemmArgs launch_args(GemmArgs g, const GemmPlan& p, const GemmLaunch& l) {
  const long r0 = l.row0;
  g.A += r0 * g.lda;
  if (g.rowscale) g.rowscale += r0;
  if (g.aux) g.aux = (const char*)g.aux + r0 * g.ld_aux * (g.aux_kind == FBL_AUX_ADD_F32 ? 4 : 2);
  if (g.out_f32) g.out_f32 += r0 * g.ldc;
  if (g.out_bf16) g.out_bf16 += r0 * g.ldc;
  if (g.out_pre) g.out_pre += r0 * g.ldc;
  if (g.seg_out) g.seg_out += r0 * g.seg_ld;
  g.drop_row0 += r0;
  g.M = l.rows;
  g.splitk = p.splitk;
  g.k8_per = p.k8_per;
  g.tiles_m = l.tiles_m;
  g.tiles_n = l.tiles_n;
  return g;
}

static int run_plan(const GemmPlan& p, const GemmArgs& g, int batch, hipStream_t stream, hipStream_t aux_stream) {
  hipEvent_t ev_fork = nullptr, ev_join = nullptr;
  for (int i = 0; i < p.n; ++i) {
    const GemmLaunch& l = p.launch[i];
    hipStream_t s = stream;
    if (l.on_aux) {
      if (!fork_join_events(stream, aux_stream, &ev_fork, &ev_join)) return FBL_ERR_ARG;
      if (hipEventRecord(ev_fork, stream) != hipSuccess) return FBL_ERR_ARG;
      if (hipStreamWaitEvent(aux_stream, ev_fork, 0) != hipSuccess) return FBL_ERR_ARG;
      s = aux_stream;
    }
    if (const int rc = launch_one(l, launch_args(g, p, l), s)) return rc;
    if (l.on_aux && hipEventRecord(ev_join, aux_stream) != hipSuccess) return FBL_ERR_ARG;
  }
  if (ev_join && hipStreamWaitEvent(stream, ev_join, 0) != hipSuccess) return FBL_ERR_ARG;
  if (p.fold) {
    const long nq = (long)g.M * (g.Nw >> 2);
    hipLaunchKernelGGL(splitk_reduce_kernel, dim3((unsigned)((nq + 255) / 256), batch), dim3(256), 0, stream,
                       (const float*)g.ws, p.splitk, g.M, g.N, g.Nw, g.out_f32, g.ldc, g.sC);
    FBL_CHECK_LAUNCH();
  }
  return 0;
}

// GemmArgs of C[M,N] = A[M,K] . B[N,K]^T with every option off; the entry points fill in theirs
static GemmArgs nt_args(const void* A, int64_t lda, const void* B, int64_t ldb, int M, int N, int K) {
  GemmArgs g{};
  g.A = (const bf16*)A; g.B = (const bf16*)B; g.lda = lda; g.ldb = ldb;
  g.M = M; g.N = N; g.K = K;
  g.alpha = 1.f; g.act = FBL_ACT_NONE; g.aux_kind = FBL_AUX_NONE;
  g.splitk = 1; g.drop_inv_keep = 1.f;
  return g;
}

// Validates a call and completes its GemmArgs (split-K, dropout, keys of the tail / segment outputs); fills in the planner's
// view of the call.  *empty: nothing to do (M, N or batch <= 0).  Pure host logic apart from the CU count of the current device,
// which it asks for only when n_cu <= 0.  gemm_nt and fbl_gemm_plan_launches share it, so the query cannot drift from what runs.
// splitk >= 2 asks for C += A.B^T (atomically, or through splitk_ws when that holds batch*splitk*M*roundup(N,4) floats).
// p_drop > 0 (ReLU epilogue, the second segment or the adapter tail): dropout of the activated output, element (m, n) keyed by
// (drop_seed, m*ldc + n).
static int prepare_gemm(GemmArgs& g, int batch, int splitk, float* splitk_ws, int64_t splitk_ws_floats, float p_drop,
                        bool aux_stream, int n_cu, GemmCall* c, bool* empty) {
  const int M = g.M, N = g.N, K = g.K;
  const bool tail = g.aux_kind == FBL_AUX_ADAPTER_TAIL;
  *empty = M <= 0 || N <= 0 || batch <= 0;
  if (*empty) return 0;
  if (K <= 0 || (K % BK) != 0) return FBL_ERR_SHAPE;               // K must be a multiple of 64 (callers zero-pad)
  if ((g.lda % 8) != 0 || (g.ldb % 8) != 0) return FBL_ERR_ALIGN;  // 16-byte operand rows
  if (splitk < 1) splitk = 1;
  const bool accumulate = splitk > 1;  // callers ask for splitk >= 2 when they want "out += A.B^T"
  if (splitk > 1) {  // every split must own at least one K tile
    const int nk = K / BK;
    const int per = (nk + splitk - 1) / splitk;
    splitk = (nk + per - 1) / per;
  }
  g.splitk = splitk;
  g.Nw = (N + 3) & ~3;
  if (accumulate && splitk_ws && (int64_t)batch * splitk * M * g.Nw <= splitk_ws_floats) g.ws = splitk_ws;  // (too small: unused)
  if (accumulate && g.bias && g.ws) return FBL_ERR_ARG;
  if (accumulate && (!g.out_f32 || g.out_bf16 || g.out_pre || g.act != FBL_ACT_NONE || g.aux_kind != FBL_AUX_NONE))
    return FBL_ERR_ARG;  // split-K only accumulates (atomicAdd) into a pre-initialised fp32 output
  if (!g.out_f32 && !g.out_bf16) return FBL_ERR_ARG;
  g.drop_ld = g.ldc;
  if (tail) {
    if (accumulate || batch != 1 || g.seg_n > 0 || !g.out_f32 || g.out_bf16 || g.out_pre || g.act != FBL_ACT_NONE ||
        g.rowscale || !g.aux || !g.r_t || (N & 3) || (g.ldc & 3) || (g.ld_aux & 3) || (g.ld_r & 3) ||
        (g.r_stats && (!g.r_gamma || !g.r_beta)))
      return FBL_ERR_ARG;
    g.drop_ld = N;  // keys of fbl_ln_fwd: (seed, m*H + n)
  }
  if (g.seg_n > 0) {
    // The epilogue branches per LANE on "column >= seg_n" but stages accumulators through per-WAVE LDS patches that all 64
    // lanes fill: the segment boundary must not cut a wave's column range.  A wave of the 2-stage kernels owns 64
    // contiguous columns, a wave of the 256-wide tiles (2-stage and 8-phase) two 32-column ranges 128 apart -> the
    // boundary has to be a multiple of 64, and of 256 for the wide tiles (otherwise the narrow tiles take the problem).
    if ((g.seg_n & 63) || g.seg_n >= N || !g.seg_out || accumulate || batch != 1) return FBL_ERR_ARG;
    g.drop_ld = g.seg_ld;
  }
  if (p_drop > 0.f) {
    if ((g.act != FBL_ACT_RELU && g.seg_n <= 0 && !tail) || p_drop >= 1.f || batch != 1) return FBL_ERR_ARG;
    g.drop_thresh = fbl_drop_thresh(p_drop);
    g.drop_inv_keep = 1.f / (1.f - p_drop);
  }
  *c = GemmCall{batch, accumulate, p_drop > 0.f, splitk_ws != nullptr, splitk_ws_floats, aux_stream,
                n_cu > 0 ? n_cu : device_cu_count()};
  return 0;
}

static int gemm_nt(GemmArgs g, int batch, int splitk, float* splitk_ws, int64_t splitk_ws_floats, float p_drop, void* stream,
                   void* aux_stream) {
  GemmCall c;
  bool empty;
  if (const int rc = prepare_gemm(g, batch, splitk, splitk_ws, splitk_ws_floats, p_drop,
                                  aux_stream != nullptr && aux_stream != stream, 0, &c, &empty))
    return rc;
  if (empty) return 0;
  return run_plan(plan_gemm(g, c), g, batch, (hipStream_t)stream, (hipStream_t)aux_stream);
}

// Host-side query (no launch, no HIP call): whether fbl_gemm_bf16_nt gives a plain launch of this shape to the big-tile route
// of the 8-phase kernel -- 8: 256- / 224-row tiles of gemm8.hip (a remainder of rows may go to small tiles of the 2-stage
// kernel), 2: otherwise (the 2-stage kernel, or the 128-row 8-phase tiles of a problem too short for the big ones).  That
// decision does not depend on the CU count; the planner is given the MI355X's 256.
extern "C" int fbl_gemm_plan(int M, int N, int K, int batch, int splitk) {
  const GemmCall c{batch, splitk > 1, false, false, 0, false, 256};
  return plan_gemm(nt_args(nullptr, K, nullptr, K, M, N, K), c).big8 ? 8 : 2;
}

// ---- the GemmArgs of each entry point (shared by the entry point and fbl_gemm_plan_launches)

static int plain_args(GemmArgs* g, const void* A, int64_t lda, const void* B, int64_t ldb, int M, int N, int K,
                      const float* bias, const float* rowscale, float alpha, int act, int aux_kind, const void* aux,
                      int64_t ld_aux, float* out_f32, void* out_bf16, void* out_pre_bf16, int64_t ldc, int64_t strideA,
                      int64_t strideB, int64_t strideC, int64_t strideAux, int64_t strideBias) {
  if (aux_kind == FBL_AUX_ADAPTER_TAIL) return FBL_ERR_ARG;  // (has its own entry point: fbl_adapter_up_resid_fwd)
  *g = nt_args(A, lda, B, ldb, M, N, K);
  g->bias = bias; g->rowscale = rowscale; g->alpha = alpha; g->act = act; g->aux_kind = aux_kind; g->aux = aux; g->ld_aux = ld_aux;
  g->out_f32 = out_f32; g->out_bf16 = (bf16*)out_bf16; g->out_pre = (bf16*)out_pre_bf16; g->ldc = ldc;
  g->sA = strideA; g->sB = strideB; g->sC = strideC; g->sAux = strideAux; g->sBias = strideBias;
  return 0;
}

static GemmArgs adapter_down_args(const void* x_bf16, int64_t ldx, const void* wd_bf16, int64_t ldw, int M, int A, int K,
                                  const float* bias, uint64_t seed, const uint64_t* seed_dev, void* z_bf16, int64_t ldz) {
  GemmArgs g = nt_args(x_bf16, ldx, wd_bf16, ldw, M, A, K);
  g.bias = bias; g.act = FBL_ACT_RELU; g.out_bf16 = (bf16*)z_bf16; g.ldc = ldz;
  g.drop_seed = seed; g.drop_seed_dev = seed_dev;
  return g;
}

static int dense_adapter_args(GemmArgs* g, const void* x_bf16, int64_t ldx, const void* wm_bf16, int64_t ldw, int M, int N1,
                              int A, int K, const float* bias_m, float* y_f32, void* y_bf16, int64_t ldy, uint64_t seed,
                              const uint64_t* seed_dev, void* z_bf16, int64_t ldz) {
  if (A <= 0 || (N1 & 63)) return FBL_ERR_ARG;
  *g = nt_args(x_bf16, ldx, wm_bf16, ldw, M, N1 + A, K);
  g->bias = bias_m; g->out_f32 = y_f32; g->out_bf16 = (bf16*)y_bf16; g->ldc = ldy;
  g->seg_n = N1; g->seg_out = (bf16*)z_bf16; g->seg_ld = ldz;
  g->drop_seed = seed; g->drop_seed_dev = seed_dev;
  return 0;
}

static int adapter_tail_args(GemmArgs* g, const void* z_bf16, int64_t ldz, const void* wu_bf16, int64_t ldw, int M, int H,
                             int A, const float* bias_u, const void* x_bf16, int64_t ldx, float p_drop, uint64_t seed,
                             const uint64_t* seed_dev, const float* r_t, int64_t ld_r, const float* r_stats,
                             const float* r_gamma, const float* r_beta, const int32_t* r_rowmask, float* out_t, int64_t ldt) {
  if (!z_bf16 || !wu_bf16 || !x_bf16 || !r_t || !out_t) return FBL_ERR_ARG;
  if (p_drop < 0.f || p_drop >= 1.f) return FBL_ERR_ARG;
  if (ldx % 8) return FBL_ERR_ALIGN;
  *g = nt_args(z_bf16, ldz, wu_bf16, ldw, M, H, A);
  g->bias = bias_u; g->aux_kind = FBL_AUX_ADAPTER_TAIL; g->aux = x_bf16; g->ld_aux = ldx; g->out_f32 = out_t; g->ldc = ldt;
  g->r_t = r_t; g->ld_r = ld_r; g->r_stats = r_stats; g->r_gamma = r_gamma; g->r_beta = r_beta; g->r_rowmask = r_rowmask;
  g->drop_seed = seed; g->drop_seed_dev = seed_dev;
  return 0;
}

extern "C" int fbl_gemm_bf16_nt(const void* A, int64_t lda, const void* B, int64_t ldb, int M, int N, int K,
                                const float* bias, const float* rowscale, float alpha, int act, int aux_kind,
                                const void* aux, int64_t ld_aux, float* out_f32, void* out_bf16, void* out_pre_bf16,
                                int64_t ldc, int batch, int64_t strideA, int64_t strideB, int64_t strideC,
                                int64_t strideAux, int64_t strideBias, int splitk, float* splitk_ws,
                                int64_t splitk_ws_floats, void* stream, void* aux_stream) {
  GemmArgs g;
  if (const int rc = plain_args(&g, A, lda, B, ldb, M, N, K, bias, rowscale, alpha, act, aux_kind, aux, ld_aux, out_f32,
                                out_bf16, out_pre_bf16, ldc, strideA, strideB, strideC, strideAux, strideBias))
    return rc;
  return gemm_nt(g, batch, splitk, splitk_ws, splitk_ws_floats, 0.f, stream, aux_stream);
}

// z[M, A] = dropout(relu(x[M,K] . Wd[A,K]^T + bd)): the adapter's down-projection with ReLU AND dropout in the GEMM
// epilogue (one launch instead of GEMM + fbl_dropout_bf16).  Element (m, a) is keyed by (seed, m*ldz + a).
extern "C" int fbl_adapter_down_fwd(const void* x_bf16, int64_t ldx, const void* wd_bf16, int64_t ldw, int M, int A, int K,
                                    const float* bias, float p_drop, uint64_t seed, const uint64_t* seed_dev, void* z_bf16,
                                    int64_t ldz, void* stream) {
  const GemmArgs g = adapter_down_args(x_bf16, ldx, wd_bf16, ldw, M, A, K, bias, seed, seed_dev, z_bf16, ldz);
  return gemm_nt(g, 1, 1, nullptr, 0, p_drop, stream, nullptr);
}

// One GEMM for a dense layer AND the down-projection of the adapter that follows it (model/deberta.py:255-257, 329-331:
// dense -> adapter; model/adapter.py:38-41): with Wm = [W ; Wd.W] ([N1 + A, K]; the lower A rows are the down-projection
// composed with the dense weight, rebuilt by the caller whenever Wd changes) and bm = [b ; Wd.b + bd],
//     [ y | z_pre ] = x . Wm^T + bm,     C = y (fp32 and/or bf16, N1 columns),     z = dropout_p(relu(z_pre)) (bf16, A columns).
// The bottleneck activations come out of the epilogue of the tile column(s) beyond N1 -- no separate K = N1 GEMM that
// re-reads y, no launch.  Dropout keys as in fbl_adapter_down_fwd: (seed, m*ldz + a).  N1 % 64 == 0 (a wave's column range
// must not straddle the segment boundary); the 256-wide tiles additionally need N1 % 256 == 0 and are not used otherwise.
extern "C" int fbl_dense_adapter_down_fwd(const void* x_bf16, int64_t ldx, const void* wm_bf16, int64_t ldw, int M, int N1,
                                          int A, int K, const float* bias_m, float* y_f32, void* y_bf16, int64_t ldy,
                                          float p_drop, uint64_t seed, const uint64_t* seed_dev, void* z_bf16, int64_t ldz,
                                          void* stream, void* aux_stream) {
  GemmArgs g;
  if (const int rc = dense_adapter_args(&g, x_bf16, ldx, wm_bf16, ldw, M, N1, A, K, bias_m, y_f32, y_bf16, ldy, seed, seed_dev,
                                        z_bf16, ldz))
    return rc;
  return gemm_nt(g, 1, 1, nullptr, 0, p_drop, stream, aux_stream);
}

extern "C" int fbl_adapter_up_resid_fwd(const void* z_bf16, int64_t ldz, const void* wu_bf16, int64_t ldw, int M, int H, int A,
                                        const float* bias_u, const void* x_bf16, int64_t ldx, float p_drop, uint64_t seed,
                                        const uint64_t* seed_dev, const float* r_t, int64_t ld_r, const float* r_stats, const float* r_gamma,
                                        const float* r_beta, const int32_t* r_rowmask, float* out_t, int64_t ldt,
                                        void* stream) {
  GemmArgs g;
  if (const int rc = adapter_tail_args(&g, z_bf16, ldz, wu_bf16, ldw, M, H, A, bias_u, x_bf16, ldx, p_drop, seed, seed_dev, r_t,
                                       ld_r, r_stats, r_gamma, r_beta, r_rowmask, out_t, ldt))
    return rc;
  return gemm_nt(g, 1, 1, nullptr, 0, p_drop, stream, nullptr);
}

// The whole plan of one call of an NT GEMM entry point, without running it (include/fbl.h).  The operand pointers the entry
// points would be given are stand-ins here: never dereferenced, only tested for NULL by the shared validation.
extern "C" int fbl_gemm_plan_launches(int entry, int M, int N, int K, int64_t lda, int64_t ldb, int64_t ldc, int64_t ld_aux,
                                      int seg_n, int act, int aux_kind, int flags, int batch, int splitk, int64_t ws_floats,
                                      int n_cu, int32_t* out) {
  if (!out || n_cu <= 0) return FBL_ERR_ARG;
  static const char stand_in[16] = {};
  const void* p = stand_in;
  auto has = [&](int f) { return (flags & f) ? (void*)p : nullptr; };
  const float p_drop = (flags & FBL_GPQ_DROPOUT) ? 0.5f : 0.f;
  GemmArgs g;
  int rc = 0;
  switch (entry) {
    case FBL_GEMM_ENTRY_PLAIN:
      rc = plain_args(&g, p, lda, p, ldb, M, N, K, (const float*)has(FBL_GPQ_BIAS), (const float*)has(FBL_GPQ_ROWSCALE), 1.f,
                      act, aux_kind, has(FBL_GPQ_AUX), ld_aux, (float*)has(FBL_GPQ_OUT_F32), has(FBL_GPQ_OUT_BF16),
                      has(FBL_GPQ_OUT_PRE), ldc, 0, 0, 0, 0, 0);
      if (rc == 0 && p_drop > 0.f) return FBL_ERR_ARG;  // (fbl_gemm_bf16_nt has no dropout)
      break;
    case FBL_GEMM_ENTRY_ADAPTER_DOWN:
      if (batch != 1 || splitk > 1) return FBL_ERR_ARG;
      g = adapter_down_args(p, lda, p, ldb, M, N, K, (const float*)has(FBL_GPQ_BIAS), 0, nullptr, (void*)p, ldc);
      break;
    case FBL_GEMM_ENTRY_DENSE_ADAPTER_DOWN:
      if (batch != 1 || splitk > 1) return FBL_ERR_ARG;
      rc = dense_adapter_args(&g, p, lda, p, ldb, M, seg_n, N - seg_n, K, (const float*)has(FBL_GPQ_BIAS),
                              (float*)has(FBL_GPQ_OUT_F32), has(FBL_GPQ_OUT_BF16), ldc, 0, nullptr, (void*)p, ld_aux);
      break;
    case FBL_GEMM_ENTRY_ADAPTER_TAIL:
      if (batch != 1 || splitk > 1) return FBL_ERR_ARG;
      rc = adapter_tail_args(&g, p, lda, p, ldb, M, N, K, (const float*)has(FBL_GPQ_BIAS), p, ld_aux, p_drop, 0, nullptr,
                             (const float*)p, ldc, (const float*)has(FBL_GPQ_R_NORM), (const float*)has(FBL_GPQ_R_NORM),
                             (const float*)has(FBL_GPQ_R_NORM), nullptr, (float*)p, ldc);
      break;
    default:
      return FBL_ERR_ARG;
  }
  if (rc) return rc;
  GemmCall c;
  bool empty;
  rc = prepare_gemm(g, batch, splitk, (flags & FBL_GPQ_WS) ? (float*)p : nullptr, ws_floats, p_drop,
                    (flags & FBL_GPQ_AUX_STREAM) != 0, n_cu, &c, &empty);
  if (rc) return rc;
  for (int i = 0; i < FBL_GEMM_PLAN_OUT_LEN; ++i) out[i] = 0;
  if (empty) return 0;
  const GemmPlan pl = plan_gemm(g, c);
  out[0] = pl.n; out[1] = pl.splitk; out[2] = pl.k8_per; out[3] = pl.fold; out[4] = pl.big8;
  for (int i = 0; i < pl.n; ++i) {
    out[5 + 4 * i] = pl.launch[i].kernel;
    out[6 + 4 * i] = pl.launch[i].row0;
    out[7 + 4 * i] = pl.launch[i].rows;
    out[8 + 4 * i] = pl.launch[i].on_aux;
  }
  return 0;
}

extern "C" int fbl_gemm_bf16_tn_acc(const void* A, int64_t lda, const void* B, int64_t ldb, int M, int N, int K,
                                    float* out_f32, int64_t ldc, int splitk, float* splitk_ws, int64_t splitk_ws_floats,
                                    void* stream) {
  if (M <= 0 || N <= 0 || K <= 0) return 0;
  if ((lda % 8) || (ldb % 8) || (M % 8) || (N % 8)) return FBL_ERR_ALIGN;
  if (!out_f32 || !splitk_ws) return FBL_ERR_ARG;
  if (splitk < 1) splitk = 1;
  const int nk = (K + 63) / 64;
  const int per = (nk + splitk - 1) / splitk;
  splitk = (nk + per - 1) / per;
  const int Nw = (N + 3) & ~3;
  if ((int64_t)splitk * M * Nw > splitk_ws_floats) return FBL_ERR_ARG;
  GemmTnArgs g{(const bf16*)A, (const bf16*)B, lda, ldb, M, N, K, splitk_ws, Nw, splitk, (M + 127) / 128, (N + 127) / 128};
  hipLaunchKernelGGL(gemm_bf16_tn_kernel, dim3(g.tiles_m * g.tiles_n, splitk), dim3(256), 0, (hipStream_t)stream, g);
  FBL_CHECK_LAUNCH();
  const long nq = (long)M * (Nw >> 2);
  hipLaunchKernelGGL(splitk_reduce_kernel, dim3((unsigned)((nq + 255) / 256), 1), dim3(256), 0, (hipStream_t)stream,
                     (const float*)splitk_ws, splitk, M, N, Nw, out_f32, (long)ldc, 0L);
  FBL_CHECK_LAUNCH();
  return 0;
}
