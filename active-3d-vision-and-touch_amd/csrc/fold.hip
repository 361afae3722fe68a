// fold.hip — one FoldingNet fold of the auto-encoder's decoder without any M x 512 tensor in memory (gfx950, exact fp32).
//
// Replaces, for one fold of reconstruction/autoencoder/model.py (FoldingNetDecFold1 / FoldingNetDecFold2),
//   conv3(relu(conv2(relu(conv1(cat(code, g))))))            over M = B * P points
// and autograd's backward of it.  conv1 of the concatenated input is bias_s[b] + W1g g_p (bias_s = W1[:, :512] code_b + b1,
// computed outside), so h1 = relu(bias_s[b] + W1g g_p) is a few vector operations per element and is REGENERATED into LDS by
// every kernel that needs it; the only wide products left are over W2 (512 x 512).
//
//   forward      fold_fwd_kernel   a 64-row tile per workgroup: h1 tile -> LDS, z2 = h1 W2^T on v_mfma_f32_32x32x2_f32 (wave w
//                                  owns output columns 128 w .. 128 w + 127), h2 = relu(z2 + b2) in registers, y = h2 W3^T + b3:
//                                  per-wave partials over its 128 columns, added in wave order.  Nothing is kept for the backward.
//   backward 1   fold_bwd_rows_kernel   32-row tiles of ONE sample per workgroup: h1 tile, z2 again (dW3 = dy^T h2 needs the
//                                  values of h2, not only its signs), h2 -> LDS; per column: dW3 += dy h2, dh2 = [h2 > 0] (dy W3),
//                                  db2 += dh2, the sign bits of h2 (64 bytes per row) go to the workspace for the dW2 kernel;
//                                  dh1 = dh2 W2 on the MFMA, dz1 = [h1 > 0] dh1 -> LDS; per column: d bias_s += dz1,
//                                  dW1g += dz1 g; per row: dg = dz1 W1g.  Column sums live in registers across the workgroup's
//                                  tiles and leave as one partial per workgroup.
//   backward 2   fold_dw2_kernel   dW2 = dh2^T h1: a 64-column slab of dW2 (64 x 512 accumulators, 128 registers per lane) per
//                                  workgroup, row tiles streamed past it: h1 and dh2 tiles regenerated into LDS from g, dy and
//                                  the sign bits; one partial per (slab, row group).
//   reductions   fold_finish_kernel / fold_dw2_sum_kernel / fold_db3_kernel: partials added in index order.
// Every sum over rows has a fixed order (no floating-point atomics): two runs give the same bits.  A row's forward result
// depends on that row's g and its sample's bias_s alone (the MFMA is an exact fma chain along k per output element), so a
// sample's output does not depend on the batch around it.
//
// W2 is read by the products as MFMA fragments: fold_pack_kernel lays it out once per call as [column block][k group][lane]
// float4 (1 MB each for W2 and W2^T), so a wave's operand load is one contiguous KB.
//
// FLOPs (shapes): one M x 512 x 512 product is 2 * 512 * 512 * M; forward 1, backward 3 (z2 again, dh1, dW2) per fold.
// Bytes: inputs/outputs M * (k + 3) * 4 each way, sign bits 64 M, W2 fragments from L2: 1 MB per 64 rows (forward), 2 MB per
// 32 rows (backward 1).
#include "gemm_tile.h"
#include "kernels.h"

namespace a3vt {


constexpr int kFW = 512;           // the compiled width
constexpr int kFLd = 516;          // floats per row of an LDS tile read as MFMA fragments (ds_read_b128, 4-bank row skew)
constexpr int kFPack = kFW * kFW;  // floats of one fragment image of W2
constexpr int kFSmall = 8 * kFW;   // floats of one workgroup's column partials: dW3 [3][512], db2, dW1g [512][3], d bias_s
constexpr int kFSlab = 64;         // columns of dW2 per workgroup of fold_dw2_kernel
constexpr int kFGroupsMax = 64;    // row groups of fold_dw2_kernel

// ---- host-side plan: one rule for the sizes, shared by the size query and the launchers ------------------------------------
struct FoldPlan {
  int tp;        // 32-row tiles per sample
  int chunks;    // workgroups per sample of fold_bwd_rows_kernel
  int tpc;       // tiles per such workgroup
  int groups;    // row groups of fold_dw2_kernel
  size_t off_packt, off_mask, off_small, off_part2, total;   // floats
};
static FoldPlan fold_plan(int batch, int points, bool bwd) {
  FoldPlan p{};
  p.tp = (points + 31) / 32;
  int want = 256 / batch;
  if (want < 1) want = 1;
  if (want > p.tp) want = p.tp;
  p.tpc = (p.tp + want - 1) / want;
  p.chunks = (p.tp + p.tpc - 1) / p.tpc;
  const long long ntiles = (long long)batch * p.tp;
  p.groups = ntiles < kFGroupsMax ? (int)ntiles : kFGroupsMax;
  p.off_packt = kFPack;
  p.off_mask = 2 * (size_t)kFPack;
  p.off_small = p.off_mask + (size_t)ntiles * 32 * 16;
  p.off_part2 = p.off_small + (size_t)batch * p.chunks * kFSmall;
  p.total = bwd ? p.off_part2 + (size_t)p.groups * kFPack : (size_t)kFPack;
  return p;
}
size_t fold_workspace_bytes(int batch, int points, int bwd) {
  if (batch <= 0 || points <= 0) return 0;
  return fold_plan(batch, points, bwd != 0).total * sizeof(float);
}

// ---- shared pieces ------------------------------------------------------------------------------------------------------------
// h1 of one element; the same chain everywhere, so every kernel regenerates the same bits
template <int K>
__device__ __forceinline__ float fold_h1(float bias, const float *w, const float *g) {
  float v = bias;
#pragma unroll
  for (int i = 0; i < K; ++i) v = fmaf(w[i], g[i], v);
  return relu_nan(v);
}
// (dy W3)[c] of one row, the same chain in both backward kernels
__device__ __forceinline__ float fold_t(const float *dy, float w0, float w1, float w2) {
  return fmaf(dy[2], w2, fmaf(dy[1], w1, dy[0] * w0));
}

// W2 (512 x 512 row-major, [n][k]) as MFMA fragments.  packn feeds z2 = h1 W2^T: block nb, k group kg, lane l holds
// W2[32 nb + (l & 31)][8 kg + 4 (l >> 5) + 0..3].  packt feeds dh1 = dh2 W2: block kb, n group ng, lane l holds
// W2[8 ng + 4 (l >> 5) + 0..3][32 kb + (l & 31)].
__global__ __launch_bounds__(256) void fold_pack_kernel(const float *__restrict__ w2, f32x4 *__restrict__ packn, f32x4 *__restrict__ packt) {
  const int idx = blockIdx.x * 256 + threadIdx.x;   // 16 * 64 * 64
  const int lane = idx & 63, grp = (idx >> 6) & 63, blk = idx >> 12;
  const int r = 32 * blk + (lane & 31), c = 8 * grp + 4 * (lane >> 5);
  packn[idx] = *reinterpret_cast<const f32x4 *>(w2 + (size_t)r * kFW + c);
  if (packt) {
    f32x4 v;
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = w2[(size_t)(c + j) * kFW + r];
    packt[idx] = v;
  }
}

// acc[rb][cb] (32 x 32, transposed: lane l holds row 32 rb + (l & 31) of the tile and the columns
// 128 wave + 32 cb + 8 (reg >> 2) + 4 (l >> 5) + (reg & 3)) = tile (RB * 32 x 512, in LDS) times the packed operand.
// k order per output element: 8 kg + 4 (l >> 5)-interleaved pairs, fixed.
template <int RB>
__device__ __forceinline__ void fold_product(const float *tile, const f32x4 *__restrict__ pack, int wave, int lane, f32x16 (&acc)[RB][4]) {
#pragma unroll
  for (int rb = 0; rb < RB; ++rb)
#pragma unroll
    for (int cb = 0; cb < 4; ++cb)
#pragma unroll
      for (int i = 0; i < 16; ++i) acc[rb][cb][i] = 0.f;
  const f32x4 *pw = pack + (size_t)wave * 4 * 4096 + lane;
  const float *pa = tile + (lane & 31) * kFLd + 4 * (lane >> 5);
  f32x4 w[4], wn[4];
#pragma unroll
  for (int cb = 0; cb < 4; ++cb) w[cb] = pw[cb * 4096];
#pragma unroll 2
  for (int kg = 0; kg < 64; ++kg) {
    const int kn = kg + 1 < 64 ? kg + 1 : kg;
#pragma unroll
    for (int cb = 0; cb < 4; ++cb) wn[cb] = pw[cb * 4096 + kn * 64];
    f32x4 a[RB];
#pragma unroll
    for (int rb = 0; rb < RB; ++rb) a[rb] = *reinterpret_cast<const f32x4 *>(pa + rb * 32 * kFLd + kg * 8);
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int cb = 0; cb < 4; ++cb)
#pragma unroll
        for (int rb = 0; rb < RB; ++rb)
          acc[rb][cb] = __builtin_amdgcn_mfma_f32_32x32x2f32(w[cb][j], a[rb][j], acc[rb][cb], 0, 0, 0);
#pragma unroll
    for (int cb = 0; cb < 4; ++cb) w[cb] = wn[cb];
  }
}

struct FoldArgs {
  const float *bias_s, *g, *w1g, *b2, *w3, *b3, *dy;
  float *y, *dg;
  const f32x4 *packn, *packt;
  unsigned long long *mask;
  float *small, *part2;
  int batch, points, tp, chunks, tpc, groups;
};

// ---- forward --------------------------------------------------------------------------------------------------------------------
constexpr int kFwdLds = (64 * kFLd + 4 * 64 * 3) * (int)sizeof(float);

template <int K>
__global__ __launch_bounds__(256) void fold_fwd_kernel(FoldArgs p) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float *sA = lds, *sY = lds + 64 * kFLd;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long long m = (long long)p.batch * p.points;
  const long long row0 = (long long)blockIdx.x * 64;
  {
    float w[2][K];
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
      for (int i = 0; i < K; ++i) w[h][i] = p.w1g[(tid + 256 * h) * K + i];
    int bprev = -1;
    float bias[2] = {0.f, 0.f};
#pragma unroll 4
    for (int r = 0; r < 64; ++r) {
      const long long row = row0 + r;
      float v0 = 0.f, v1 = 0.f;
      if (row < m) {
        const int b = (int)(row / p.points);
        if (b != bprev) {
          bias[0] = p.bias_s[(size_t)b * kFW + tid];
          bias[1] = p.bias_s[(size_t)b * kFW + tid + 256];
          bprev = b;
        }
        float g[K];
#pragma unroll
        for (int i = 0; i < K; ++i) g[i] = p.g[row * K + i];
        v0 = fold_h1<K>(bias[0], w[0], g);
        v1 = fold_h1<K>(bias[1], w[1], g);
      }
      sA[r * kFLd + tid] = v0;
      sA[r * kFLd + tid + 256] = v1;
    }
  }
  __syncthreads();
  f32x16 acc[2][4];
  fold_product<2>(sA, p.packn, wave, lane, acc);
  // h2 = relu(z2 + b2) and this wave's part of y = h2 W3^T, columns in a fixed order
  float part[2][3] = {{0.f, 0.f, 0.f}, {0.f, 0.f, 0.f}};
#pragma unroll
  for (int cb = 0; cb < 4; ++cb) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int n0 = wave * 128 + cb * 32 + 8 * q + 4 * (lane >> 5);
      const f32x4 b2 = *reinterpret_cast<const f32x4 *>(p.b2 + n0);
      f32x4 w3[3];
#pragma unroll
      for (int o = 0; o < 3; ++o) w3[o] = *reinterpret_cast<const f32x4 *>(p.w3 + o * kFW + n0);
#pragma unroll
      for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int rb = 0; rb < 2; ++rb) {
          const float h2 = relu_nan(acc[rb][cb][4 * q + t] + b2[t]);
#pragma unroll
          for (int o = 0; o < 3; ++o) part[rb][o] = fmaf(h2, w3[o][t], part[rb][o]);
        }
    }
  }
#pragma unroll
  for (int rb = 0; rb < 2; ++rb)
#pragma unroll
    for (int o = 0; o < 3; ++o) {
      const float other = __shfl_xor(part[rb][o], 32, 64);
      // (lower half + upper half, in that order on both sides)
      const float lo = lane < 32 ? part[rb][o] : other, hi = lane < 32 ? other : part[rb][o];
      if (lane < 32) sY[(wave * 64 + rb * 32 + lane) * 3 + o] = lo + hi;
    }
  __syncthreads();
  if (tid < 192) {
    const int r = tid / 3, o = tid - 3 * r;
    const long long row = row0 + r;
    if (row < m) {
      float v = sY[(0 * 64 + r) * 3 + o];
      v += sY[(1 * 64 + r) * 3 + o];
      v += sY[(2 * 64 + r) * 3 + o];
      v += sY[(3 * 64 + r) * 3 + o];
      p.y[row * 3 + o] = v + p.b3[o];
    }
  }
}

// ---- backward 1: everything per row tile ----------------------------------------------------------------------------------------
constexpr int kBwdLds = (2 * 32 * kFLd + 2 * 32 * 4) * (int)sizeof(float);

template <int K>
__global__ __launch_bounds__(256) void fold_bwd_rows_kernel(FoldArgs p) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float *sA = lds, *sB = lds + 32 * kFLd, *sG = lds + 2 * 32 * kFLd, *sDy = sG + 32 * 4;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = blockIdx.x / p.chunks, chunk = blockIdx.x - b * p.chunks;
  const int t0 = chunk * p.tpc, t1 = t0 + p.tpc < p.tp ? t0 + p.tpc : p.tp;
  float w1[2][K], w3[2][3], bias[2];
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int c = tid + 256 * h;
#pragma unroll
    for (int i = 0; i < K; ++i) w1[h][i] = p.w1g[c * K + i];
#pragma unroll
    for (int o = 0; o < 3; ++o) w3[h][o] = p.w3[o * kFW + c];
    bias[h] = p.bias_s[(size_t)b * kFW + c];
  }
  float a_dw3[2][3] = {{0.f, 0.f, 0.f}, {0.f, 0.f, 0.f}}, a_db2[2] = {0.f, 0.f}, a_dbias[2] = {0.f, 0.f};
  float a_dw1[2][3] = {{0.f, 0.f, 0.f}, {0.f, 0.f, 0.f}};
  for (int tile = t0; tile < t1; ++tile) {
    const int p0 = tile * 32;
    const size_t rowbase = (size_t)b * p.points + p0;
    if (tid < 32) {
      const bool valid = p0 + tid < p.points;
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        sG[tid * 4 + i] = valid && i < K ? p.g[(rowbase + tid) * K + i] : 0.f;
        sDy[tid * 4 + i] = valid ? p.dy[(rowbase + tid) * 3 + i] : 0.f;
      }
    }
    __syncthreads();
#pragma unroll 4
    for (int r = 0; r < 32; ++r) {
      const bool valid = p0 + r < p.points;
      float g[K];
#pragma unroll
      for (int i = 0; i < K; ++i) g[i] = sG[r * 4 + i];
      sA[r * kFLd + tid] = valid ? fold_h1<K>(bias[0], w1[0], g) : 0.f;
      sA[r * kFLd + tid + 256] = valid ? fold_h1<K>(bias[1], w1[1], g) : 0.f;
    }
    __syncthreads();
    f32x16 acc[1][4];
    fold_product<1>(sA, p.packn, wave, lane, acc);
#pragma unroll
    for (int cb = 0; cb < 4; ++cb)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int n0 = wave * 128 + cb * 32 + 8 * q + 4 * (lane >> 5);
        const f32x4 b2 = *reinterpret_cast<const f32x4 *>(p.b2 + n0);
        f32x4 h2;
#pragma unroll
        for (int t = 0; t < 4; ++t) h2[t] = relu_nan(acc[0][cb][4 * q + t] + b2[t]);
        *reinterpret_cast<f32x4 *>(sB + (lane & 31) * kFLd + n0) = h2;
      }
    __syncthreads();
    // per column: dW3, dh2 (in place of h2), db2, the sign bits
    unsigned long long *mrow = p.mask + ((size_t)b * p.tp + tile) * 32 * 8;
#pragma unroll 4
    for (int r = 0; r < 32; ++r) {
      const float *dy = sDy + r * 4;
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int c = tid + 256 * h;
        const float h2 = sB[r * kFLd + c];
#pragma unroll
        for (int o = 0; o < 3; ++o) a_dw3[h][o] = fmaf(dy[o], h2, a_dw3[h][o]);
        const bool on = h2 > 0.f;
        const float d = on ? fold_t(dy, w3[h][0], w3[h][1], w3[h][2]) : 0.f;
        a_db2[h] += d;
        sB[r * kFLd + c] = d;
        const unsigned long long bits = __ballot(on);
        if (lane == 0) mrow[r * 8 + 4 * h + wave] = bits;
      }
    }
    __syncthreads();
    fold_product<1>(sB, p.packt, wave, lane, acc);
#pragma unroll
    for (int cb = 0; cb < 4; ++cb)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int n0 = wave * 128 + cb * 32 + 8 * q + 4 * (lane >> 5);
        float *ph = sA + (lane & 31) * kFLd + n0;
        const f32x4 h1 = *reinterpret_cast<const f32x4 *>(ph);
        f32x4 dz;
#pragma unroll
        for (int t = 0; t < 4; ++t) dz[t] = h1[t] > 0.f ? acc[0][cb][4 * q + t] : 0.f;
        *reinterpret_cast<f32x4 *>(ph) = dz;
      }
    __syncthreads();
#pragma unroll 4
    for (int r = 0; r < 32; ++r) {
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const float dz = sA[r * kFLd + tid + 256 * h];
        a_dbias[h] += dz;
#pragma unroll
        for (int i = 0; i < K; ++i) a_dw1[h][i] = fmaf(dz, sG[r * 4 + i], a_dw1[h][i]);
      }
    }
    if (K == 3 && p.dg) {   // dg = dz1 W1g: eight lanes per row, 64 columns each, then a fixed butterfly
      const int r = tid >> 3, sub = tid & 7;
      float s[3] = {0.f, 0.f, 0.f};
#pragma unroll 8
      for (int j = 0; j < 64; ++j) {
        const int c = sub + 8 * j;
        const float dz = sA[r * kFLd + c];
#pragma unroll
        for (int i = 0; i < 3; ++i) s[i] = fmaf(dz, p.w1g[c * K + (i < K ? i : 0)], s[i]);
      }
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        s[i] += __shfl_xor(s[i], 1, 64);
        s[i] += __shfl_xor(s[i], 2, 64);
        s[i] += __shfl_xor(s[i], 4, 64);
      }
      if (sub == 0 && p0 + r < p.points) {
#pragma unroll
        for (int i = 0; i < 3; ++i) p.dg[(rowbase + r) * 3 + i] = s[i];
      }
    }
    __syncthreads();
  }
  float *out = p.small + (size_t)blockIdx.x * kFSmall;
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int c = tid + 256 * h;
#pragma unroll
    for (int o = 0; o < 3; ++o) out[o * kFW + c] = a_dw3[h][o];
    out[3 * kFW + c] = a_db2[h];
#pragma unroll
    for (int i = 0; i < 3; ++i) out[4 * kFW + c * 3 + i] = i < K ? a_dw1[h][i < K ? i : 0] : 0.f;
    out[7 * kFW + c] = a_dbias[h];
  }
}

// ---- backward 2: dW2 = dh2^T h1, a 64-column slab per workgroup -------------------------------------------------------------------
constexpr int kDw2Lds = (32 * kFW + 32 * kFSlab + 2 * 32 * 4) * (int)sizeof(float);

template <int K>
__global__ __launch_bounds__(256) void fold_dw2_kernel(FoldArgs p) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float *sH = lds, *sD = lds + 32 * kFW, *sG = sD + 32 * kFSlab, *sDy = sG + 32 * 4;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int slab = blockIdx.x, grp = blockIdx.y;
  const int ntiles = p.batch * p.tp;
  const int per = (ntiles + p.groups - 1) / p.groups;
  const int g0 = grp * per, g1 = g0 + per < ntiles ? g0 + per : ntiles;
  float w1[2][K];
#pragma unroll
  for (int h = 0; h < 2; ++h)
#pragma unroll
    for (int i = 0; i < K; ++i) w1[h][i] = p.w1g[(tid + 256 * h) * K + i];
  // this thread's eight columns of the dh2 tile: row tid >> 3, columns 8 (tid & 7) ..
  const int dr = tid >> 3, dc = 8 * (tid & 7);
  float w3[8][3];
#pragma unroll
  for (int j = 0; j < 8; ++j)
#pragma unroll
    for (int o = 0; o < 3; ++o) w3[j][o] = p.w3[o * kFW + slab * kFSlab + dc + j];
  f32x16 acc[2][4];
#pragma unroll
  for (int cb = 0; cb < 2; ++cb)
#pragma unroll
    for (int kb = 0; kb < 4; ++kb)
#pragma unroll
      for (int i = 0; i < 16; ++i) acc[cb][kb][i] = 0.f;
  int bprev = -1;
  float bias[2] = {0.f, 0.f};
  for (int gt = g0; gt < g1; ++gt) {
    const int b = gt / p.tp, tile = gt - b * p.tp;
    const int p0 = tile * 32;
    const size_t rowbase = (size_t)b * p.points + p0;
    if (b != bprev) {
      bias[0] = p.bias_s[(size_t)b * kFW + tid];
      bias[1] = p.bias_s[(size_t)b * kFW + tid + 256];
      bprev = b;
    }
    if (tid < 32) {
      const bool valid = p0 + tid < p.points;
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        sG[tid * 4 + i] = valid && i < K ? p.g[(rowbase + tid) * K + i] : 0.f;
        sDy[tid * 4 + i] = valid ? p.dy[(rowbase + tid) * 3 + i] : 0.f;
      }
    }
    __syncthreads();
#pragma unroll 4
    for (int r = 0; r < 32; ++r) {
      const bool valid = p0 + r < p.points;
      float g[K];
#pragma unroll
      for (int i = 0; i < K; ++i) g[i] = sG[r * 4 + i];
      sH[r * kFW + tid] = valid ? fold_h1<K>(bias[0], w1[0], g) : 0.f;
      sH[r * kFW + tid + 256] = valid ? fold_h1<K>(bias[1], w1[1], g) : 0.f;
    }
    {
      const unsigned long long bits = p.mask[((size_t)gt * 32 + dr) * 8 + slab];
      const float *dy = sDy + dr * 4;
#pragma unroll
      for (int j = 0; j < 8; ++j)
        sD[dr * kFSlab + dc + j] = (bits >> (dc + j)) & 1ull ? fold_t(dy, w3[j][0], w3[j][1], w3[j][2]) : 0.f;
    }
    __syncthreads();
    const float *pd = sD + (lane >> 5) * kFSlab + (lane & 31);
    const float *ph = sH + (lane >> 5) * kFW + wave * 128 + (lane & 31);
#pragma unroll 4
    for (int rs = 0; rs < 16; ++rs) {
      float a[2], h[4];
#pragma unroll
      for (int cb = 0; cb < 2; ++cb) a[cb] = pd[rs * 2 * kFSlab + cb * 32];
#pragma unroll
      for (int kb = 0; kb < 4; ++kb) h[kb] = ph[rs * 2 * kFW + kb * 32];
#pragma unroll
      for (int cb = 0; cb < 2; ++cb)
#pragma unroll
        for (int kb = 0; kb < 4; ++kb) acc[cb][kb] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[cb], h[kb], acc[cb][kb], 0, 0, 0);
    }
    __syncthreads();
  }
  // lane l holds dW2[64 slab + 32 cb + 8 (reg >> 2) + 4 (l >> 5) + (reg & 3)][128 wave + 32 kb + (l & 31)]
  float *out = p.part2 + (size_t)grp * kFPack;
#pragma unroll
  for (int cb = 0; cb < 2; ++cb)
#pragma unroll
    for (int kb = 0; kb < 4; ++kb)
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int c = slab * kFSlab + cb * 32 + 8 * (i >> 2) + 4 * (lane >> 5) + (i & 3);
        out[(size_t)c * kFW + wave * 128 + kb * 32 + (lane & 31)] = acc[cb][kb][i];
      }
}

// ---- reductions, partials in index order ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void fold_dw2_sum_kernel(const f32x4 *__restrict__ part, int groups, f32x4 *__restrict__ dw2) {
  const int idx = blockIdx.x * 256 + threadIdx.x;   // kFPack / 4
  f32x4 s = part[idx];
  for (int g = 1; g < groups; ++g) s += part[(size_t)g * (kFPack / 4) + idx];
  dw2[idx] = s;
}

// items: dW3 (3 x 512), db2 (512), dW1g (512 x k), d bias_s (batch x 512)
__global__ __launch_bounds__(256) void fold_finish_kernel(const float *__restrict__ small, int batch, int chunks, int k, float *dw3, float *db2,
                                                          float *dw1g, float *dbias) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  const int nwg = batch * chunks;
  if (idx < 4 * kFW) {
    float s = 0.f;
    for (int w = 0; w < nwg; ++w) s += small[(size_t)w * kFSmall + idx];
    if (idx < 3 * kFW) dw3[idx] = s;
    else db2[idx - 3 * kFW] = s;
  } else if (idx < 7 * kFW) {
    const int e = idx - 4 * kFW, c = e / 3, i = e - 3 * c;
    if (i < k) {
      float s = 0.f;
      for (int w = 0; w < nwg; ++w) s += small[(size_t)w * kFSmall + idx];
      dw1g[c * k + i] = s;
    }
  } else if (idx < 7 * kFW + batch * kFW) {
    const int e = idx - 7 * kFW, b = e / kFW, c = e - b * kFW;
    float s = 0.f;
    for (int w = 0; w < chunks; ++w) s += small[(size_t)(b * chunks + w) * kFSmall + 7 * kFW + c];
    dbias[e] = s;
  }
}

__global__ __launch_bounds__(256) void fold_db3_kernel(const float *__restrict__ dy, long long m, float *db3) {
  __shared__ float red[256];
  const int o = blockIdx.x, tid = threadIdx.x;
  float s = 0.f;
  for (long long r = tid; r < m; r += 256) s += dy[r * 3 + o];
  red[tid] = s;
  __syncthreads();
  for (int st = 128; st > 0; st >>= 1) {
    if (tid < st) red[tid] += red[tid + st];
    __syncthreads();
  }
  if (tid == 0) db3[o] = red[0];
}

// ---- launchers --------------------------------------------------------------------------------------------------------------------
template <int K>
static int fold_fwd_k(const FoldArgs &a, hipStream_t s) {
  static OncePerDevice once;
  once.run([] { (void)hipFuncSetAttribute((const void *)fold_fwd_kernel<K>, hipFuncAttributeMaxDynamicSharedMemorySize, kFwdLds); });
  const long long m = (long long)a.batch * a.points;
  A3VT_LAUNCH((fold_fwd_kernel<K>), dim3((unsigned)((m + 63) / 64)), dim3(256), kFwdLds, s, a);
  A3VT_CHECK_LAUNCH();
  return 0;
}

int launch_fold_fwd(const float *bias_s, const float *g, int k, const float *w1g, const float *w2, const float *b2, const float *w3,
                    const float *b3, int batch, int points, float *y, float *ws, hipStream_t s) {
  const FoldPlan pl = fold_plan(batch, points, false);
  FoldArgs a{};
  a.bias_s = bias_s, a.g = g, a.w1g = w1g, a.b2 = b2, a.w3 = w3, a.b3 = b3, a.y = y;
  a.packn = reinterpret_cast<const f32x4 *>(ws);
  a.batch = batch, a.points = points, a.tp = pl.tp;
  A3VT_LAUNCH(fold_pack_kernel, dim3(256), dim3(256), 0, s, w2, reinterpret_cast<f32x4 *>(ws), (f32x4 *)nullptr);
  A3VT_CHECK_LAUNCH();
  path_count(PATH_FOLD_FWD);
  return k == 2 ? fold_fwd_k<2>(a, s) : fold_fwd_k<3>(a, s);
}

template <int K>
static int fold_bwd_k(const FoldArgs &a, hipStream_t s) {
  static OncePerDevice once;
  once.run([] {
    (void)hipFuncSetAttribute((const void *)fold_bwd_rows_kernel<K>, hipFuncAttributeMaxDynamicSharedMemorySize, kBwdLds);
    (void)hipFuncSetAttribute((const void *)fold_dw2_kernel<K>, hipFuncAttributeMaxDynamicSharedMemorySize, kDw2Lds);
  });
  A3VT_LAUNCH((fold_bwd_rows_kernel<K>), dim3(a.batch * a.chunks), dim3(256), kBwdLds, s, a);
  A3VT_CHECK_LAUNCH();
  A3VT_LAUNCH((fold_dw2_kernel<K>), dim3(kFW / kFSlab, a.groups), dim3(256), kDw2Lds, s, a);
  A3VT_CHECK_LAUNCH();
  return 0;
}

int launch_fold_bwd(const float *bias_s, const float *g, int k, const float *w1g, const float *w2, const float *b2, const float *w3,
                    const float *dy, int batch, int points, float *dbias_s, float *dg, float *dw1g, float *dw2, float *db2,
                    float *dw3, float *db3, float *ws, hipStream_t s) {
  const FoldPlan pl = fold_plan(batch, points, true);
  FoldArgs a{};
  a.bias_s = bias_s, a.g = g, a.w1g = w1g, a.b2 = b2, a.w3 = w3, a.dy = dy, a.dg = dg;
  a.packn = reinterpret_cast<const f32x4 *>(ws);
  a.packt = reinterpret_cast<const f32x4 *>(ws + pl.off_packt);
  a.mask = reinterpret_cast<unsigned long long *>(ws + pl.off_mask);
  a.small = ws + pl.off_small;
  a.part2 = ws + pl.off_part2;
  a.batch = batch, a.points = points, a.tp = pl.tp, a.chunks = pl.chunks, a.tpc = pl.tpc, a.groups = pl.groups;
  A3VT_LAUNCH(fold_pack_kernel, dim3(256), dim3(256), 0, s, w2, reinterpret_cast<f32x4 *>(ws), reinterpret_cast<f32x4 *>(ws + pl.off_packt));
  A3VT_CHECK_LAUNCH();
  path_count(PATH_FOLD_BWD);
  const int rc = k == 2 ? fold_bwd_k<2>(a, s) : fold_bwd_k<3>(a, s);
  if (rc) return rc;
  A3VT_LAUNCH(fold_dw2_sum_kernel, dim3(kFPack / 4 / 256), dim3(256), 0, s, reinterpret_cast<const f32x4 *>(a.part2), pl.groups,
              reinterpret_cast<f32x4 *>(dw2));
  A3VT_CHECK_LAUNCH();
  A3VT_LAUNCH(fold_finish_kernel, dim3(cdiv(7 * kFW + (long long)batch * kFW, 256)), dim3(256), 0, s, a.small, batch, pl.chunks, k, dw3, db2,
              dw1g, dbias_s);
  A3VT_CHECK_LAUNCH();
  A3VT_LAUNCH(fold_db3_kernel, dim3(3), dim3(256), 0, s, dy, (long long)batch * points, db3);
  A3VT_CHECK_LAUNCH();
  return 0;
}

}  // namespace a3vt
