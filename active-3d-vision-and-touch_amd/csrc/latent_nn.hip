// latent_nn.hip — the nearest-neighbour policy's bank lookup: for every query latent the k nearest rows of a bank of latents
// (mean squared difference, ties to the lower row) and the first of them whose recorded action has not been taken yet.
//
// Reference: pterotactyl/policies/NearestNeighbor/train.py:114-137 — per element a broadcast subtract / square / mean over the
// bank, a topk of 25, then a Python walk down the 25 that synchronises with the device once per candidate.  Here: two launches.
//
//   latent_dist_kernel    a workgroup takes kLatentTile rows of the bank, a wave kLatentTile / 4 of them; the queries sit in LDS
//                         (in chunks of kLatentQueryFloats / dim queries).  ONE (query, row) pair is always summed the same way:
//                         lane l owns the columns W (64 i + l) .. + W - 1 for i = 0, 1, .. (W = 4 with 16-byte loads when
//                         dim % 4 == 0, else W = 1), adds its squares in ascending column order with one fused multiply-add
//                         each, the wave finishes with prims.h's butterfly wave_sum, and the sum is divided by dim.  Nothing in
//                         that depends on where the row or the query sits or on how many there are, so bit-identical rows get
//                         bit-identical distances.  The fp32 bits go to dist[query][row] in the scratch; a NaN is stored as the
//                         canonical positive NaN 0x7fc00000.
//   latent_select_kernel  one workgroup of 1024 threads per query.  Distances are >= 0, so their bit patterns order as unsigned
//                         integers, the canonical NaN after +inf, and the key (bits << 32) | row makes "distance, then row" one
//                         64-bit minimum (keys are unique).  Every thread keeps the smallest of its keys not yet taken, every
//                         wave the minimum of its threads' (DPP row shifts and broadcasts); each of the k_eff = min(k, bank_rows)
//                         passes takes the minimum of the 16 waves behind one barrier, after which only the thread that held
//                         it looks for its next key.  A bank of at most kLatentCachedRows rows is held in registers (16 per
//                         thread); a larger one is read from the scratch whenever a thread looks for its next key.  The first
//                         wave then applies the action rule to the k_eff listed rows with one ballot.
// No atomics, no fences between workgroups, no host synchronisation: the same bits on every call.
#include "kernels.h"
#include "prims.h"

namespace a3vt {

namespace {

using u64 = unsigned long long;
constexpr unsigned kNanBits = 0x7fc00000u;
constexpr int kSelectThreads = 1024, kSelectRegs = kLatentCachedRows / kSelectThreads;
static_assert(kSelectRegs * kSelectThreads == kLatentCachedRows, "the cached selection holds whole registers");

template <int W>
struct Cols;
template <>
struct Cols<4> {
  using type = f32x4;
  static __device__ __forceinline__ type zero() { return (f32x4){0.f, 0.f, 0.f, 0.f}; }
  static __device__ __forceinline__ float sq(type b, type q, float acc) {
    const f32x4 d = b - q;
    acc = __fmaf_rn(d[0], d[0], acc);
    acc = __fmaf_rn(d[1], d[1], acc);
    acc = __fmaf_rn(d[2], d[2], acc);
    return __fmaf_rn(d[3], d[3], acc);
  }
};
template <>
struct Cols<1> {
  using type = float;
  static __device__ __forceinline__ type zero() { return 0.f; }
  static __device__ __forceinline__ float sq(type b, type q, float acc) {
    const float d = b - q;
    return __fmaf_rn(d, d, acc);
  }
};

// W: columns per lane and load (4: dim % 4 == 0, rows and queries 16-byte aligned).  N: most column groups a lane can own,
// N * 64 * W >= dim.  R: rows a wave keeps in registers at a time.
template <int W, int N, int R>
__global__ __launch_bounds__(256) void latent_dist_kernel(const float *__restrict__ bank, int bank_rows, int dim,
                                                          const float *__restrict__ queries, int n_queries, int q_chunk,
                                                          unsigned *__restrict__ dist) {
  using V = typename Cols<W>::type;
  constexpr int kRowsPerWave = kLatentTile / 4;
  static_assert(kRowsPerWave % R == 0, "a wave's rows split into whole register groups");
  __shared__ __attribute__((aligned(16))) float qs[kLatentQueryFloats];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int groups = cdiv(dim, 64 * W);   // column groups in use (<= N)
  const int row0 = blockIdx.x * kLatentTile + wave * kRowsPerWave;
  const float fdim = (float)dim;
  for (int q0 = 0; q0 < n_queries; q0 += q_chunk) {
    const int nq = min(q_chunk, n_queries - q0);
    __syncthreads();   // (the previous chunk has been consumed)
    for (int i = threadIdx.x; i < nq * dim; i += 256) qs[i] = queries[(size_t)q0 * dim + i];
    __syncthreads();
    for (int g = 0; g < kRowsPerWave; g += R) {
      if (row0 + g >= bank_rows) break;   // (wave-uniform: this group and the later ones lie past the bank)
      V b[R][N];
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const int row = row0 + g + r;
#pragma unroll
        for (int i = 0; i < N; ++i) {
          const int col = W * (i * 64 + lane);
          b[r][i] = (i < groups && row < bank_rows && col < dim) ? *reinterpret_cast<const V *>(bank + (size_t)row * dim + col)
                                                                   : Cols<W>::zero();
        }
      }
      for (int e = 0; e < nq; ++e) {
        float acc[R];
#pragma unroll
        for (int r = 0; r < R; ++r) acc[r] = 0.f;
#pragma unroll
        for (int i = 0; i < N; ++i) {
          if (i >= groups) break;
          const int col = W * (i * 64 + lane);
          const V qv = col < dim ? *reinterpret_cast<const V *>(qs + e * dim + col) : Cols<W>::zero();   // (a column past dim adds +0)
#pragma unroll
          for (int r = 0; r < R; ++r) acc[r] = Cols<W>::sq(b[r][i], qv, acc[r]);
        }
#pragma unroll
        for (int r = 0; r < R; ++r) {
          const float d = wave_sum(acc[r]) / fdim;
          const int row = row0 + g + r;
          if (lane == 0 && row < bank_rows) dist[(size_t)(q0 + e) * bank_rows + row] = d != d ? kNanBits : f32_bits(d);
        }
      }
    }
  }
}

// 64-bit minimum over the lanes of a wave on DPP moves (all 64 lanes active; a lane without a source keeps its own value).
// Row shifts by 1, 2, 4, 8 leave each 16-lane row's minimum in its lane 15; row_bcast:15 into rows 1 and 3 and row_bcast:31 into
// rows 2 and 3 carry it to lane 63.
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ u64 dpp_min_u64(u64 v) {
  const unsigned lo = (unsigned)v, hi = (unsigned)(v >> 32);
  const u64 o = ((u64)(unsigned)__builtin_amdgcn_update_dpp((int)hi, (int)hi, CTRL, ROW_MASK, 0xf, false) << 32) |
                (unsigned)__builtin_amdgcn_update_dpp((int)lo, (int)lo, CTRL, ROW_MASK, 0xf, false);
  return o < v ? o : v;
}
__device__ __forceinline__ u64 row_min_u64(u64 v) {   // lane 15 of each 16-lane row: the row's minimum
  v = dpp_min_u64<0x111, 0xf>(v);   // row_shr:1
  v = dpp_min_u64<0x112, 0xf>(v);   // row_shr:2
  v = dpp_min_u64<0x114, 0xf>(v);   // row_shr:4
  return dpp_min_u64<0x118, 0xf>(v);   // row_shr:8
}
__device__ __forceinline__ u64 read_lane_u64(u64 v, int lane) {
  return ((u64)(unsigned)__builtin_amdgcn_readlane((int)(unsigned)(v >> 32), lane) << 32) |
         (unsigned)__builtin_amdgcn_readlane((int)(unsigned)v, lane);
}
__device__ __forceinline__ u64 wave_min_u64(u64 v) {   // every lane gets the wave's minimum
  v = row_min_u64(v);
  v = dpp_min_u64<0x142, 0xa>(v);   // row_bcast:15 -> rows 1, 3
  v = dpp_min_u64<0x143, 0xc>(v);   // row_bcast:31 -> rows 2, 3
  return read_lane_u64(v, 63);
}

template <bool CACHED>
__global__ __launch_bounds__(kSelectThreads) void latent_select_kernel(const unsigned *__restrict__ dist, int bank_rows, int k,
                                                                       const int32_t *__restrict__ bank_actions,
                                                                       const float *__restrict__ taken, int num_actions,
                                                                       int32_t *__restrict__ idx, float *__restrict__ dist_out,
                                                                       int32_t *__restrict__ action, int32_t *__restrict__ rank) {
  __shared__ u64 part[2][kSelectThreads / 64];
  __shared__ u64 sel[kLatentMaxK];
  const int e = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const unsigned *__restrict__ d = dist + (size_t)e * bank_rows;
  const int k_eff = min(k, bank_rows);
  unsigned v[kSelectRegs];
  if (CACHED) {
#pragma unroll
    for (int i = 0; i < kSelectRegs; ++i) {
      const int j = tid + i * kSelectThreads;
      v[i] = j < bank_rows ? d[j] : 0xffffffffu;   // (past the bank: above every key of a row)
    }
  }
  auto own_min = [&](u64 lo) {   // the thread's smallest key >= lo
    u64 m = ~0ull;
    if (CACHED) {
#pragma unroll
      for (int i = 0; i < kSelectRegs; ++i) {
        const u64 key = ((u64)v[i] << 32) | (unsigned)(tid + i * kSelectThreads);
        if (key >= lo && key < m) m = key;
      }
    } else {
      for (int j = tid; j < bank_rows; j += kSelectThreads) {
        const u64 key = ((u64)d[j] << 32) | (unsigned)j;
        if (key >= lo && key < m) m = key;
      }
    }
    return m;
  };
  // Every thread keeps its smallest key not yet taken, every wave the minimum of its threads'.  A pass takes the minimum of the 16
  // waves; only the thread that held it looks for its next key, and only its wave reduces again.
  static_assert(kSelectThreads / 64 == 16, "a 16-lane row holds one partial minimum per wave");
  u64 cand = own_min(0);
  u64 wmin = wave_min_u64(cand);
  for (int p = 0; p < k_eff; ++p) {
    if (lane == 0) part[p & 1][wave] = wmin;
    __syncthreads();   // (one barrier per pass: pass p + 2 rewrites this buffer only after every wave has passed barrier p + 1)
    const u64 best = read_lane_u64(row_min_u64(part[p & 1][lane & 15]), 15);
    if (tid == 0) sel[p] = best;
    if (wmin == best) {   // (wave-uniform)
      if (cand == best) cand = own_min(best + 1);
      wmin = wave_min_u64(cand);
    }
  }
  __syncthreads();
  if (wave != 0) return;
  const bool listed = lane < k_eff;
  const u64 key = listed ? sel[lane] : 0;
  const int row = (int)(unsigned)(key & 0xffffffffu);
  if (lane < k) {
    idx[(size_t)e * k + lane] = listed ? row : -1;
    dist_out[(size_t)e * k + lane] = listed ? bits_f32((unsigned)(key >> 32)) : INFINITY;
  }
  if (action) {
    int a = -1;
    bool ok = false;
    if (listed) {
      a = bank_actions[row];
      ok = a >= 0 && a < num_actions && (!taken || taken[(size_t)e * num_actions + a] == 0.f);   // (out of range: never indexes taken)
    }
    const u64 m = __ballot(ok);
    const int first = m ? __ffsll((long long)m) - 1 : 0;
    const int chosen = __shfl(a, first, 64);
    if (lane == 0) {
      action[e] = m ? chosen : -1;
      rank[e] = m ? first : -1;
    }
  }
}

template <int W, int N, int R>
void launch_dist(const float *bank, int bank_rows, int dim, const float *queries, int n_queries, unsigned *dist, hipStream_t s) {
  A3VT_LAUNCH((latent_dist_kernel<W, N, R>), dim3(cdiv(bank_rows, kLatentTile)), dim3(256), 0, s, bank, bank_rows, dim, queries,
              n_queries, kLatentQueryFloats / dim, dist);
}

}  // namespace

int launch_latent_nearest(const float *bank, const int32_t *bank_actions, int bank_rows, int dim, const float *queries,
                          const float *taken, int n_queries, int num_actions, int k, int32_t *idx, float *dist, int32_t *action,
                          int32_t *rank, void *scratch, hipStream_t s) {
  unsigned *d = static_cast<unsigned *>(scratch);
  if (dim % 4 == 0) {
    if (dim <= 256)
      launch_dist<4, 1, 4>(bank, bank_rows, dim, queries, n_queries, d, s);
    else
      launch_dist<4, 16, 1>(bank, bank_rows, dim, queries, n_queries, d, s);
  } else if (dim <= 64) {
    launch_dist<1, 1, 4>(bank, bank_rows, dim, queries, n_queries, d, s);
  } else if (dim <= 1024) {
    launch_dist<1, 16, 1>(bank, bank_rows, dim, queries, n_queries, d, s);
  } else {
    launch_dist<1, 64, 1>(bank, bank_rows, dim, queries, n_queries, d, s);
  }
  A3VT_CHECK_LAUNCH();
  if (bank_rows <= kLatentCachedRows)
    A3VT_LAUNCH(latent_select_kernel<true>, dim3(n_queries), dim3(kSelectThreads), 0, s, d, bank_rows, k, bank_actions, taken,
                num_actions, idx, dist, action, rank);
  else
    A3VT_LAUNCH(latent_select_kernel<false>, dim3(n_queries), dim3(kSelectThreads), 0, s, d, bank_rows, k, bank_actions, taken,
                num_actions, idx, dist, action, rank);
  A3VT_CHECK_LAUNCH();
  return 0;
}

}  // namespace a3vt
