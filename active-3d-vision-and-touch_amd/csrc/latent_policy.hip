// latent_policy.hip — the supervised policy's value network (policies/supervised/model.py: Latent_Model, and DDQN's model of the
// same shape without the output squashing) as one launch per evaluation, its loss as one launch, its backward as two.
//
// Reference: seven small Linear layers at E = 3 rows on torch ops (about twenty launches of a few hundred multiply-adds each), a
// Python double loop of all_pred_values[j, a] picks for the loss and a per-element values[e][act] = 1e10 loop before the argmin
// (policies/supervised/train.py:119-155).
//
// The network arrives as a table of layers BY VALUE in the kernel arguments (PolicyNet: weight / bias pointers in torch's
// [out][in] layout, used in place).  One "concat" position says where the input becomes cat(previous output, latent, first_latent).
//
//   policy_fwd_kernel    one workgroup of 16 waves per row; the activations ping-pong between two LDS rows.  ONE output neuron is
//                        always summed the same way: lane l owns the columns W (64 i + l) .. + W - 1 for i = 0, 1, .. (W = 4 with
//                        16-byte loads when in % 4 == 0, else W = 1), adds its products in ascending column order with one fused
//                        multiply-add each, the wave finishes with prims.h's butterfly wave_sum, then the bias is added.  A wave
//                        takes four neighbouring neurons at a time (four independent chains).  Nothing depends on the row's
//                        position or on how many rows there are.  Wave 0 then makes the action choice over the LDS row.
//   action_value_loss_kernel   a workgroup owns 16 rows of dvalues: it clears them, then one thread per row adds that row's T terms
//                        in t order.  Workgroup 0 also sums the loss: thread p of 256 adds the pairs p, p + 256, .. in that order,
//                        wave_sum, the four wave sums in wave order.
//   policy_bwd_delta_kernel    one workgroup per row: dvalues through the output transform, then layer by layer
//                        delta_{l-1}[i] = relu'(.) sum_o W[o][i] delta_l[o], a thread owning column i, o ascending.
//   policy_bwd_grad_kernel     a workgroup owns kPolicySlab output rows of one layer: dW[o][i] = sum_e delta[e][o] in[e][i] and
//                        db[o] = sum_e delta[e][o], e ascending, one thread per element.
// No atomics, no fences between workgroups, no host synchronisation: the same bits on every call.
// The row forward, the delta chain and the gradient slab are policy_dev.h's: ddqn_latent.hip runs the same sums.
#include "policy_dev.h"

namespace a3vt {

namespace {

using u64 = unsigned long long;
constexpr int kLossThreads = 256, kLossRows = 16;

// value -> a key that orders as the contract does: numbers ascending (-0 == +0), then every NaN
__device__ __forceinline__ unsigned order_key(float v) {
  if (v != v) return 0xffffffffu;
  const unsigned b = f32_bits(v + 0.f);   // (-0 + +0 = +0)
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

__device__ __forceinline__ u64 wave_min_key(u64 v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const unsigned lo = (unsigned)__shfl_xor((int)(unsigned)v, off, 64), hi = (unsigned)__shfl_xor((int)(unsigned)(v >> 32), off, 64);
    const u64 o = ((u64)hi << 32) | lo;
    v = o < v ? o : v;
  }
  return v;
}

__global__ __launch_bounds__(kFwdThreads) void policy_fwd_kernel(PolicyNet net, const float *__restrict__ mask,
                                                                 const float *__restrict__ latent,
                                                                 const float *__restrict__ first_latent,
                                                                 const float *__restrict__ taken, float *__restrict__ values,
                                                                 int32_t *__restrict__ action, float *__restrict__ stash, int ld) {
  __shared__ __attribute__((aligned(16))) float buf[2][kPolicyMaxWidth];
  const int e = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6, ls = net.latent_size, n = net.n_layers;
  const int cur = policy_row_forward(net, mask + (size_t)e * net.layer[0].in, latent + (size_t)e * ls, first_latent + (size_t)e * ls,
                                     values + (size_t)e * net.layer[n - 1].out, stash ? stash + (size_t)e * ld : nullptr, buf);
  if (!action) return;
  __syncthreads();
  if (wave != 0) return;
  const int A = net.layer[n - 1].out;
  u64 best = ~0ull;
  for (int a = lane; a < A; a += 64)
    if (taken[(size_t)e * A + a] == 0.f) {
      const u64 key = ((u64)order_key(buf[cur][a]) << 32) | (unsigned)a;
      best = key < best ? key : best;
    }
  best = wave_min_key(best);
  if (lane == 0) action[e] = best == ~0ull ? -1 : (int32_t)(unsigned)(best & 0xffffffffu);
}

__global__ __launch_bounds__(kLossThreads) void action_value_loss_kernel(const float *__restrict__ values,
                                                                         const int32_t *__restrict__ actions,
                                                                         const float *__restrict__ targets, int T, int E, int A,
                                                                         float *__restrict__ loss, float *__restrict__ dvalues) {
  __shared__ float part[kLossThreads / 64];
  const int tid = threadIdx.x, r0 = blockIdx.x * kLossRows, rows = min(kLossRows, E - r0);
  const float n = (float)T * (float)E, two_over_n = 2.f / n;
  for (int i = tid; i < rows * A; i += kLossThreads) dvalues[(size_t)r0 * A + i] = 0.f;
  __syncthreads();
  if (tid < rows) {
    const int e = r0 + tid;
    for (int t = 0; t < T; ++t) {
      const int a = actions[(size_t)t * E + e];
      if ((unsigned)a < (unsigned)A) {   // (the host refuses others; never index outside the row)
        const size_t at = (size_t)e * A + a;
        dvalues[at] += (values[at] - targets[(size_t)t * E + e]) * two_over_n;
      }
    }
  }
  if (blockIdx.x != 0) return;
  float acc = 0.f;
  for (int p = tid; p < T * E; p += kLossThreads) {
    const int e = p % E, a = actions[p];
    if ((unsigned)a < (unsigned)A) {
      const float d = targets[p] - values[(size_t)e * A + a];
      acc = __fmaf_rn(d, d, acc);
    }
  }
  acc = wave_sum(acc);
  if ((tid & 63) == 0) part[tid >> 6] = acc;
  __syncthreads();
  if (tid == 0) {
    float s = part[0];
    for (int w = 1; w < kLossThreads / 64; ++w) s += part[w];
    loss[0] = s / n;
  }
}

__global__ __launch_bounds__(kFwdThreads) void policy_bwd_delta_kernel(PolicyNet net, const float *__restrict__ dvalues,
                                                                       const float *__restrict__ stash, float *__restrict__ delta,
                                                                       int ld) {
  __shared__ float d[2][kPolicyMaxWidth];
  const int e = blockIdx.x;
  policy_row_delta(net, dvalues + (size_t)e * net.layer[net.n_layers - 1].out, stash + (size_t)e * ld, delta + (size_t)e * ld, ld, d);
}

__global__ __launch_bounds__(kGradThreads) void policy_bwd_grad_kernel(PolicyNet net, PolicyGrads grads, const float *__restrict__ mask,
                                                                       const float *__restrict__ latent,
                                                                       const float *__restrict__ first_latent,
                                                                       const float *__restrict__ stash, const float *__restrict__ delta,
                                                                       int E, int ld, int accumulate) {
  policy_grad_slab(net, grads, mask, latent, first_latent, stash, delta, E, ld, accumulate, blockIdx.x);
}

}  // namespace

int launch_policy_fwd(const PolicyNet &net, const float *mask, const float *latent, const float *first_latent, const float *taken,
                      int rows, float *values, int32_t *action, float *stash, int ld, hipStream_t s) {
  A3VT_LAUNCH(policy_fwd_kernel, dim3(rows), dim3(kFwdThreads), 0, s, net, mask, latent, first_latent, taken, values, action, stash, ld);
  A3VT_CHECK_LAUNCH();
  return 0;
}

int launch_action_value_loss(const float *values, const int32_t *actions, const float *targets, int steps, int rows, int num_actions,
                             float *loss, float *dvalues, hipStream_t s) {
  A3VT_LAUNCH(action_value_loss_kernel, dim3(cdiv(rows, kLossRows)), dim3(kLossThreads), 0, s, values, actions, targets, steps, rows,
              num_actions, loss, dvalues);
  A3VT_CHECK_LAUNCH();
  return 0;
}

int launch_policy_bwd(const PolicyNet &net, const PolicyGrads &grads, const float *mask, const float *latent, const float *first_latent,
                      const float *dvalues, const float *stash, float *delta, int rows, int ld, int accumulate, hipStream_t s) {
  A3VT_LAUNCH(policy_bwd_delta_kernel, dim3(rows), dim3(kFwdThreads), 0, s, net, dvalues, stash, delta, ld);
  A3VT_CHECK_LAUNCH();
  A3VT_LAUNCH(policy_bwd_grad_kernel, dim3(policy_grad_slabs(net)), dim3(kGradThreads), 0, s, net, grads, mask, latent, first_latent, stash, delta, rows, ld,
              accumulate);
  A3VT_CHECK_LAUNCH();
  return 0;
}

}  // namespace a3vt
