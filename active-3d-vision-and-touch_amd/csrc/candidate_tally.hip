// candidate_tally.hip — what the dataset-specific policies (LEBA, MFBA) do with the (K, E) score table of one swept batch: the
// per-element greedy choice, LEBA's per-action ratio sums and visit counts, MFBA's per-action votes.
//
// Reference: pterotactyl/policies/dataset_specific/LEBA.py:115-128 and MFBA.py:95-99 — the table comes to the host and a Python
// loop over the K * E pairs updates NumPy arrays.  Here: ONE launch of ONE workgroup of 1024 threads (the work is a few hundred
// pairs at the reference's sizes, so it is bound by latency, not by a CU's throughput), in three phases behind barriers.
//
//   choice   element e is shared by G = the largest power of two <= min(64, 1024 / E) lanes of one wave; lane g walks
//            k = g, g + G, .. keeping the best eligible pair it met, and a butterfly over the G lanes combines them under the
//            total order "number < +inf < NaN, then the lower k" — so the result is the same for every G.  Lane 0 writes
//            best / best_score and keeps best in LDS for the votes.
//   tally    the pairs are taken in their order i = k * E + e, 1024 at a time: thread t of a tile divides pair i's score by its
//            element's first score (__fdiv_rn) and puts (candidate, ratio) into LDS; then thread a < A walks the tile in
//            order and acts on the pairs of its own action, its sum and its count in registers.  Every action's updates are
//            therefore made by one thread in pair order, whatever the tile size.
//   votes    thread a < A walks best[0 .. E) in LDS in order and counts its own.
// No atomics, no scratch, no host synchronisation: the same bits on every call.
#include <limits.h>

#include "common.h"
#include "kernels.h"

namespace a3vt {

namespace {

constexpr int kTallyThreads = 1024;
using i32x4 = __attribute__((ext_vector_type(4))) int;
static_assert(kTallyMaxElements <= kTallyThreads, "an element has at least one thread");
static_assert(kTallyMaxActions <= kTallyThreads, "an action has a thread");

// Does (s2, k2) come before (s1, k1)?  k == INT_MAX: no pair at all.
__device__ __forceinline__ bool comes_before(float s2, int k2, float s1, int k1) {
  if (k2 == INT_MAX) return false;
  if (k1 == INT_MAX) return true;
  const bool nan1 = s1 != s1, nan2 = s2 != s2;
  if (nan1 != nan2) return nan1;
  if (nan1 || s2 == s1) return k2 < k1;   // (-0 == +0: a tie)
  return s2 < s1;
}

__global__ __launch_bounds__(kTallyThreads) void candidate_tally_kernel(const float *__restrict__ scores,
                                                                        const int32_t *__restrict__ candidates,
                                                                        const float *__restrict__ first_score,
                                                                        const float *__restrict__ taken, int K, int E, int A, int G,
                                                                        double unvisited, double *__restrict__ sums,
                                                                        double *__restrict__ checks, double *__restrict__ votes,
                                                                        int32_t *__restrict__ best, float *__restrict__ best_score) {
  __shared__ int32_t best_s[kTallyMaxElements];
  __shared__ __attribute__((aligned(16))) int32_t cand_s[kTallyThreads];
  __shared__ float ratio_s[kTallyThreads];
  const int tid = threadIdx.x;

  if (best || best_score) {   // (uniform)
    const int e = tid / G, g = tid - e * G;
    float low = INFINITY;
    int low_k = INT_MAX, low_a = -1;
    if (e < E) {
      for (int k = g; k < K; k += G) {
        const int a = candidates[k * E + e];
        if (a < 0 || a >= A) continue;   // (never indexes taken)
        if (taken && taken[e * A + a] != 0.f) continue;
        const float s = scores[k * E + e];
        if (comes_before(s, k, low, low_k)) low = s, low_k = k, low_a = a;
      }
    }
    for (int off = 1; off < G; off <<= 1) {   // (every lane of the wave takes part; a group is G aligned lanes)
      const float s = __shfl_xor(low, off, 64);
      const int k = __shfl_xor(low_k, off, 64), a = __shfl_xor(low_a, off, 64);
      if (comes_before(s, k, low, low_k)) low = s, low_k = k, low_a = a;
    }
    if (e < E && g == 0) {
      best_s[e] = low_a;
      if (best) best[e] = low_a;
      if (best_score) best_score[e] = low;
    }
  }

  if (sums) {   // (uniform; checks comes with it)
    const int pairs = K * E;
    double sum = 0.0, count = 0.0;
    if (tid < A) sum = sums[tid], count = checks[tid];
    for (int i0 = 0; i0 < pairs; i0 += kTallyThreads) {
      const int i = i0 + tid;
      __syncthreads();   // (the tile before has been walked)
      cand_s[tid] = i < pairs ? candidates[i] : -1;   // (past the table: nobody's, so the walk may run to a multiple of 4)
      if (i < pairs) ratio_s[tid] = __fdiv_rn(scores[i], first_score[i % E]);
      __syncthreads();
      if (tid < A) {
        const int n = min(kTallyThreads, pairs - i0);
        for (int j = 0; j < n; j += 4) {   // (one 16-byte LDS read per four pairs: the walk is a chain of LDS latencies)
          const i32x4 c = *reinterpret_cast<const i32x4 *>(cand_s + j);
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            if (c[u] != tid) continue;   // (a candidate outside [0, A) is nobody's)
            const float r = ratio_s[j + u];
            sum = sum == unvisited ? (double)r : (double)((float)sum + r);
            count += 1.0;
          }
        }
      }
    }
    if (tid < A) sums[tid] = sum, checks[tid] = count;
  }

  if (votes) {   // (uniform; best is required with it, so the choice ran)
    __syncthreads();
    if (tid < A) {
      double v = votes[tid];
      for (int e = 0; e < E; ++e)
        if (best_s[e] == tid) v += 1.0;
      votes[tid] = v;
    }
  }
}

}  // namespace

int launch_candidate_tally(const float *scores, const int32_t *candidates, const float *first_score, const float *taken, int K, int E,
                           int A, double unvisited, double *sums, double *checks, double *votes, int32_t *best, float *best_score,
                           hipStream_t s) {
  int G = 1;
  while (G < 64 && 2 * G * E <= kTallyThreads) G *= 2;
  A3VT_LAUNCH(candidate_tally_kernel, dim3(1), dim3(kTallyThreads), 0, s, scores, candidates, first_score, taken, K, E, A, G, unvisited,
              sums, checks, votes, best, best_score);
  A3VT_CHECK_LAUNCH();
  return 0;
}

}  // namespace a3vt
