// policy_dev.h — the device code of the latent value / Q network that latent_policy.hip (the supervised policy) and
// ddqn_latent.hip (DDQN's Latent_Model) share, and the double-DQN sample rule that ddqn.hip and ddqn_latent.hip share.  ONE
// definition of every sum: a row's forward, the delta chain, a gradient slab, the TD sample and the loss tree are each written
// here once, so two kernels that call them on the same operands give the same bits.  Internal; not part of the C ABI.
#pragma once
#include "kernels.h"
#include "prims.h"

namespace a3vt {

constexpr int kFwdThreads = 1024, kFwdWaves = kFwdThreads / 64, kNeurons = 4;
constexpr int kGradThreads = 256;

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

// Row e of the network by a workgroup of kFwdThreads: the activations ping-pong between the two LDS rows of `buf`; `values` (row
// e's A outputs) is always written, `stash` (row e's ld floats, or NULL) keeps every layer's post-activation row.  Returns the
// index of the LDS row that holds the output; the caller synchronises before it reads that row.
__device__ __forceinline__ int policy_row_forward(const PolicyNet &net, const float *__restrict__ mask, const float *__restrict__ latent,
                                                  const float *__restrict__ first_latent, float *__restrict__ values,
                                                  float *__restrict__ stash, float (*buf)[kPolicyMaxWidth]) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int in0 = net.layer[0].in, ls = net.latent_size, n = net.n_layers;
  for (int i = tid; i < in0; i += kFwdThreads) buf[0][i] = mask[i];
  int cur = 0, off = 0;
  for (int l = 0; l < n; ++l) {
    const PolicyLayer L = net.layer[l];
    if (l == net.concat_at) {   // cat(previous output, latent, first_latent): the previous layer wrote [0, p)
      const int p = L.in - 2 * ls;
      for (int i = tid; i < 2 * ls; i += kFwdThreads) buf[cur][p + i] = i < ls ? latent[i] : first_latent[i - ls];
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
          if (stash) stash[off + o0 + r] = kept;
          if (last) values[o0 + r] = z;
        }
      }
    }
    cur ^= 1;
    off += L.out;
  }
  return cur;
}

// Row e's deltas by a workgroup of kFwdThreads: `dv` the row's A output gradients (global or LDS, complete before the call), `act`
// the row's stash, `del` the row of the delta table, `d` two LDS rows.
__device__ __forceinline__ void policy_row_delta(const PolicyNet &net, const float *dv, const float *__restrict__ act,
                                                 float *__restrict__ del, int ld, float (*d)[kPolicyMaxWidth]) {
  const int tid = threadIdx.x, n = net.n_layers;
  int off = ld - net.layer[n - 1].out, cur = 0;
  {
    const PolicyLayer L = net.layer[n - 1];
    for (int i = tid; i < L.out; i += kFwdThreads) {
      float g = dv[i];
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

// Slabs of kPolicySlab output rows over all layers: the grid of the gradient kernels.
inline int policy_grad_slabs(const PolicyNet &net) {
  int slabs = 0;
  for (int l = 0; l < net.n_layers; ++l) slabs += cdiv(net.layer[l].out, kPolicySlab);
  return slabs;
}

// Slab b (counted over the layers in order) of dW / db by a workgroup of kGradThreads: one thread per element, e ascending.
__device__ __forceinline__ void policy_grad_slab(const PolicyNet &net, const PolicyGrads &grads, const float *__restrict__ mask,
                                                 const float *__restrict__ latent, const float *__restrict__ first_latent,
                                                 const float *__restrict__ stash, const float *__restrict__ delta, int E, int ld,
                                                 int accumulate, int b) {
  int l = 0, off = 0;
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

// ---- the double-DQN rule (policies/DDQN/ddqn.py:100-115) ------------------------------------------------------------------

// One wave: argmax_a (pen[a] > 0 ? -1e10 : q[a]) of one row, the lowest index on a tie (index 0 when every action is
// penalised: all candidates are -1e10 then), and the sum of pen (0 / 1 entries: exact in any order).  Every lane gets both.
__device__ __forceinline__ int td_argmax(const float *pen, const float *q, int na, int lane, float &touched) {
  float t = 0.f, best = -INFINITY;
  int arg = 0x7fffffff;
  for (int a = lane; a < na; a += 64) {
    const float mk = pen[a];
    t += mk;
    const float v = mk > 0.f ? -1e10f : q[a];
    if (v > best || arg == 0x7fffffff) {   // strict: the lowest index of this lane's columns wins a tie
      best = v;
      arg = a;
    }
  }
  touched = wave_sum(t);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const float ob = __shfl_xor(best, off, 64);
    const int oa = __shfl_xor(arg, off, 64);
    if (oa != 0x7fffffff && (arg == 0x7fffffff || ob > best || (ob == best && oa < arg))) {
      best = ob;
      arg = oa;
    }
  }
  return arg;
}

// One wave, sample b, from the three Q rows of the sample: writes best_next[b], target[b], diff[b] and returns diff (lane 0's
// value is the one that counts).  done_at = budget - 1 as a float.
__device__ __forceinline__ float td_sample(const float *q_cur, const float *q_no, const float *q_nt, const float *mb,
                                           const float *__restrict__ actions, const float *__restrict__ rewards,
                                           const float *__restrict__ denom, int b, int na, float done_at, float gamma, int lane,
                                           float *__restrict__ diff, int32_t *__restrict__ best_next, float *__restrict__ target) {
  float touched;
  const int arg = td_argmax(mb, q_no, na, lane, touched);
  float d = 0.f;
  if (lane == 0) {
    int act = (int)actions[b];
    act = act < 0 ? 0 : (act >= na ? na - 1 : act);   // (an action outside the table is the caller's error: stay inside the row)
    float r = rewards[b];
    if (denom) r = r / denom[b];
    const float next = touched < done_at ? q_nt[arg] : 0.f;
    const float t = __fadd_rn(__fmul_rn(gamma, next), r);   // the reference's two roundings (no fused multiply-add)
    d = q_cur[act] - t;
    best_next[b] = arg;
    target[b] = t;
    diff[b] = d;
  }
  return d;
}

// d loss / d q_cur[b][action] for loss = mean_b diff^2 and the upstream gradient gl
__device__ __forceinline__ float td_dq(float gl, float d, int batch) { return gl * 2.f * d / (float)batch; }

// mean of sq[0 .. batch) (LDS, complete and synchronised before the call) by the whole workgroup: pairwise tree in a fixed order
// (element i takes i + stride), then / batch.
__device__ __forceinline__ void td_loss_tree(float *sq, int batch, float *__restrict__ loss) {
  int n = batch;
  while (n > 1) {
    const int half = (n + 1) >> 1;
    for (int i = threadIdx.x; i + half < n; i += blockDim.x) sq[i] += sq[i + half];
    __syncthreads();
    n = half;
  }
  if (threadIdx.x == 0) loss[0] = sq[0] / (float)batch;
}

}  // namespace a3vt
