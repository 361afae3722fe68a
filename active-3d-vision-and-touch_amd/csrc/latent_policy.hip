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
#include "kernels.h"
#include "prims.h"

namespace a3vt {

namespace {

using u64 = unsigned long long;
constexpr int kFwdThreads = 1024, kFwdWaves = kFwdThreads / 64, kNeurons = 4;
constexpr int kLossThreads = 256, kLossRows = 16, kGradThreads = 256;

// One lane's share of sum_c w[c] x[c] for kNeurons neighbouring weight rows (x in LDS, 16-byte aligned; w rows `in` floats apart).
template <int W>
__device__ __forceinline__ void dot_share(const float *__restrict__ w, const float *x, int in, int rows, int lane, float (&acc)[kNeurons]) {
#pragma unroll
  for (int r = 0; r < kNeurons; ++r) acc[r] = 0.f;
  for (int c = W * lane; c < in; c += 64 * W) {
    if (W == 4) {
      const f32x4 xv = *reinterpret_cast<const f32x4 *>(x + c);
#pragma unroll
      for (int r = 0; r < kNeurons; ++r) {
        if (r < rows) {   // (wave-uniform)
          const f32x4 wv = *reinterpret_cast<const f32x4 *>(w + (size_t)r * in + c);
          acc[r] = __fmaf_rn(wv[0], xv[0], acc[r]);
          acc[r] = __fmaf_rn(wv[1], xv[1], acc[r]);
          acc[r] = __fmaf_rn(wv[2], xv[2], acc[r]);
          acc[r] = __fmaf_rn(wv[3], xv[3], acc[r]);
        }
      }
    } else {
      const float xv = x[c];
#pragma unroll
      for (int r = 0; r < kNeurons; ++r)
        if (r < rows) acc[r] = __fmaf_rn(w[(size_t)r * in + c], xv, acc[r]);
    }
  }
}

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
  const int e = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int in0 = net.layer[0].in, ls = net.latent_size, n = net.n_layers;
  for (int i = tid; i < in0; i += kFwdThreads) buf[0][i] = mask[(size_t)e * in0 + i];
  int cur = 0, off = 0;
  for (int l = 0; l < n; ++l) {
    const PolicyLayer L = net.layer[l];
    if (l == net.concat_at) {   // cat(previous output, latent, first_latent): the previous layer wrote [0, p)
      const int p = L.in - 2 * ls;
      for (int i = tid; i < 2 * ls; i += kFwdThreads)
        buf[cur][p + i] = i < ls ? latent[(size_t)e * ls + i] : first_latent[(size_t)e * ls + i - ls];
    }
    __syncthreads();   // (the input row is complete; the other row has been consumed)
    const float *x = buf[cur];
    float *y = buf[cur ^ 1];
    const bool last = l == n - 1;
    for (int o0 = wave * kNeurons; o0 < L.out; o0 += kFwdWaves * kNeurons) {
      const int rows = min(kNeurons, L.out - o0);
      float acc[kNeurons];
      if (L.in % 4 == 0)
        dot_share<4>(L.w + (size_t)o0 * L.in, x, L.in, rows, lane, acc);
      else
        dot_share<1>(L.w + (size_t)o0 * L.in, x, L.in, rows, lane, acc);
#pragma unroll
      for (int r = 0; r < kNeurons; ++r) {
        if (r >= rows) break;
        float z = wave_sum(acc[r]) + L.b[o0 + r];
        if (L.relu) z = z < 0.f ? 0.f : z;   // (a NaN stays a NaN)
        float kept = z;                      // what the backward wants of this layer
        if (last && net.transform) {
          kept = 1.f / (1.f + expf(-z));
          z = __fsub_rn(__fmul_rn(kept, net.scale), net.offset);
        }
        if (lane == 0) {
          y[o0 + r] = z;
          if (stash) stash[(size_t)e * ld + off + o0 + r] = kept;
          if (last) values[(size_t)e * L.out + o0 + r] = z;
        }
      }
    }
    cur ^= 1;
    off += L.out;
  }
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
  const int e = blockIdx.x, tid = threadIdx.x, n = net.n_layers;
  const float *act = stash + (size_t)e * ld;
  float *del = delta + (size_t)e * ld;
  int off = ld - net.layer[n - 1].out, cur = 0;
  {
    const PolicyLayer L = net.layer[n - 1];
    for (int i = tid; i < L.out; i += kFwdThreads) {
      float g = dvalues[(size_t)e * L.out + i];
      const float a = act[off + i];
      if (net.transform) g = (g * net.scale) * (a * (1.f - a));   // (the stash keeps the sigmoid itself)
      if (L.relu) g = a > 0.f ? g : 0.f;
      d[0][i] = g;
      del[off + i] = g;
    }
  }
  for (int l = n - 1; l >= 1; --l) {
    const PolicyLayer L = net.layer[l], P = net.layer[l - 1];
    const int poff = off - P.out;
    __syncthreads();   // (delta_l is complete; the other row has been consumed)
    for (int i = tid; i < P.out; i += kFwdThreads) {   // at the concat only the first P.out input columns flow on
      const float *__restrict__ w = L.w + i;
      float acc = 0.f;
#pragma unroll 4
      for (int o = 0; o < L.out; ++o) acc = __fmaf_rn(w[(size_t)o * L.in], d[cur][o], acc);
      if (P.relu) acc = act[poff + i] > 0.f ? acc : 0.f;
      d[cur ^ 1][i] = acc;
      del[poff + i] = acc;
    }
    cur ^= 1;
    off = poff;
  }
}

__global__ __launch_bounds__(kGradThreads) void policy_bwd_grad_kernel(PolicyNet net, PolicyGrads grads, const float *__restrict__ mask,
                                                                       const float *__restrict__ latent,
                                                                       const float *__restrict__ first_latent,
                                                                       const float *__restrict__ stash, const float *__restrict__ delta,
                                                                       int E, int ld, int accumulate) {
  int b = blockIdx.x, l = 0, off = 0;
  while (b >= cdiv(net.layer[l].out, kPolicySlab)) {   // (the grid is the sum of the layers' slab counts)
    b -= cdiv(net.layer[l].out, kPolicySlab);
    off += net.layer[l].out;
    ++l;
  }
  const PolicyLayer L = net.layer[l];
  const int o0 = b * kPolicySlab, rows = min(kPolicySlab, L.out - o0), ls = net.latent_size;
  const int p = l == net.concat_at ? L.in - 2 * ls : L.in;   // input columns that come from the previous layer's row
  float *__restrict__ dw = grads.dw[l], *__restrict__ db = grads.db[l];
  for (int idx = threadIdx.x; idx < rows * L.in; idx += kGradThreads) {
    const int o = o0 + idx / L.in, i = idx % L.in;
    const float *src;
    int stride;
    if (l == 0) {
      src = mask + i, stride = L.in;
    } else if (i < p) {
      src = stash + (off - p) + i, stride = ld;
    } else if (i < p + ls) {
      src = latent + (i - p), stride = ls;
    } else {
      src = first_latent + (i - p - ls), stride = ls;
    }
    const float *__restrict__ dl = delta + off + o;
    float acc = 0.f;
    for (int e = 0; e < E; ++e) acc = __fmaf_rn(dl[(size_t)e * ld], src[(size_t)e * stride], acc);
    const size_t at = (size_t)o * L.in + i;
    dw[at] = accumulate ? dw[at] + acc : acc;
    if (i == 0) {
      float accb = 0.f;
      for (int e = 0; e < E; ++e) accb += dl[(size_t)e * ld];
      db[o] = accumulate ? db[o] + accb : accb;
    }
  }
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
  int slabs = 0;
  for (int l = 0; l < net.n_layers; ++l) slabs += cdiv(net.layer[l].out, kPolicySlab);
  A3VT_LAUNCH(policy_bwd_grad_kernel, dim3(slabs), dim3(kGradThreads), 0, s, net, grads, mask, latent, first_latent, stash, delta, rows, ld,
              accumulate);
  A3VT_CHECK_LAUNCH();
  return 0;
}

}  // namespace a3vt
