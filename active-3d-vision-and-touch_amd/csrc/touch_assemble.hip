// touch_assemble.hip — the K * E candidate chart and mask tensors of one greedy step from the per-episode touch table, in their
// final layout: what policies/environment.py's candidate loop built per chunk with two repeats, two indexed assignments, 4 K views
// and four cats over K dicts.
//
// The output is K * E * F * G blocks of C chart rows (3 floats) and C mask values.  Block (k, e, f, g) is the state's block
// (e, f, g), except at g == slot, where it is the table's block (e, candidates[k][e], f) and the table's code as a float.  ONE
// launch: a wave per block, the block's index taken apart once per wave (scalar work), then the lanes move C * 3 + C dwords with
// consecutive addresses.  The job is a few hundred thousand dwords at most (K = 50, E = 3, F = 4, G = 5, C = 25: 3000 blocks of 100
// dwords), so it is bound by latency: the kernel gives every SIMD of the chip a few short waves.
//
// Dwords on purpose: a block of C = 25 rows is 300 bytes, so only every fourth block starts on a 16-byte boundary (and the
// caller's tensors need only 4-byte alignment).  Values move as uint32_t: NaN payloads, infinities and -0 are bits like any other.
// No atomics, no workspace, no host synchronisation; every output dword is written by exactly one lane, and no input is written.
#include "common.h"
#include "kernels.h"

namespace a3vt {

namespace {

constexpr int kAssembleThreads = 256;                        // four waves, a block each per round
constexpr int kAssembleWaves = kAssembleThreads / kWave;
constexpr int kAssembleMaxGroups = 1 << 16;                  // workgroups of a launch; the waves stride over the blocks beyond

__global__ __launch_bounds__(kAssembleThreads) void touch_assemble_kernel(const uint32_t *__restrict__ table_charts,
                                                                          const int32_t *__restrict__ table_codes,
                                                                          const uint32_t *__restrict__ state_charts,
                                                                          const uint32_t *__restrict__ state_masks,
                                                                          const int32_t *__restrict__ candidates, int E, int A, int F, int G,
                                                                          int C, int slot, long long blocks, uint32_t *__restrict__ charts,
                                                                          uint32_t *__restrict__ masks) {
  const int lane = threadIdx.x & (kWave - 1);
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
  const int row = C * 3;                                     // dwords of a block's chart
  const long long stride = (long long)gridDim.x * kAssembleWaves;
  for (long long b = (long long)blockIdx.x * kAssembleWaves + wave; b < blocks; b += stride) {   // (uniform per wave)
    const int g = (int)(b % G);
    const long long kef = b / G;
    const int f = (int)(kef % F);
    const long long ke = kef / F;                            // = k * E + e: the index into candidates
    const int e = (int)(ke % E);
    const long long s = ((long long)e * F + f) * G + g;      // the state's block
    uint32_t *out_c = charts + b * row, *out_m = masks + b * C;
    if (g != slot) {
      for (int i = lane; i < row; i += kWave) out_c[i] = state_charts[s * row + i];
      for (int i = lane; i < C; i += kWave) out_m[i] = state_masks[s * C + i];
      continue;
    }
    const int a = candidates[ke];
    if (a < 0 || a >= A) {                                   // (never indexes the table)
      for (int i = lane; i < row; i += kWave) out_c[i] = 0u;
      for (int i = lane; i < C; i += kWave) out_m[i] = 0u;
      continue;
    }
    const long long t = ((long long)e * A + a) * F + f;      // the table's block
    const int code = min(max(table_codes[t], 0), 2);
    const uint32_t mask = __float_as_uint((float)code);
    for (int i = lane; i < row; i += kWave) out_c[i] = table_charts[t * row + i];
    for (int i = lane; i < C; i += kWave) out_m[i] = mask;
  }
}

}  // namespace

int launch_touch_assemble(const float *table_charts, const int32_t *table_codes, const float *state_charts, const float *state_masks,
                          const int32_t *candidates, int K, int E, int A, int F, int G, int C, int slot, float *charts, float *masks,
                          hipStream_t s) {
  const long long blocks = (long long)K * E * F * G;
  const long long groups = (blocks + kAssembleWaves - 1) / kAssembleWaves;
  const int grid = (int)(groups < kAssembleMaxGroups ? groups : kAssembleMaxGroups);
  A3VT_LAUNCH(touch_assemble_kernel, dim3(grid), dim3(kAssembleThreads), 0, s, reinterpret_cast<const uint32_t *>(table_charts),
              table_codes, reinterpret_cast<const uint32_t *>(state_charts), reinterpret_cast<const uint32_t *>(state_masks), candidates,
              E, A, F, G, C, slot, blocks, reinterpret_cast<uint32_t *>(charts), reinterpret_cast<uint32_t *>(masks));
  A3VT_CHECK_LAUNCH();
  return 0;
}

}  // namespace a3vt
