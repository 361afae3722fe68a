// ddqn_latent.hip — DDQN's Latent_Model (policies/DDQN/model.py:15-61, the supervised value network's shape without the output
// squashing: a3vt_mlp with transform 0) as one launch per action choice and three launches per update.
//
// Reference: an update is three evaluations of the seven small Linear layers on torch ops at 16 rows, the TD rule, an autograd
// backward (policies/DDQN/ddqn.py:81-125) — about a hundred launches of a few hundred multiply-adds each; an action choice adds a
// masking op, an argmax and a copy (:127-141).
//
//   ddqn_latent_q_kernel         policy_dev.h's row forward, a workgroup per row; wave 0 then takes the argmax of
//                                (penalty > 0 ? -1e10 : q) over the LDS row by td_argmax, ddqn_td_kernel's rule.
//   ddqn_latent_fwd_kernel       a (batch, 3) grid, one role per workgroup: online(mask, latent) with the stash, online(mask_n,
//                                latent_n), target(mask_n, latent_n).  The roles sit side by side: a row's layers are a serial
//                                chain and at 16 rows the device is nearly empty.
//   ddqn_latent_td_delta_kernel  a workgroup per row: wave 0 runs td_sample on the row (ddqn_td_kernel's arithmetic), the row's dq
//                                goes to LDS ((1 * 2 * diff) / batch at the action, 0 elsewhere), then policy_dev.h's delta chain.
//   ddqn_latent_grad_kernel      a workgroup per (layer, slab of kPolicySlab rows): policy_dev.h's gradient slab, overwriting; one
//                                more workgroup squares diff into LDS and runs td_loss_tree.
// Every sum is the one latent_policy.hip and ddqn.hip run (policy_dev.h), so the outputs equal, bit for bit, a3vt_latent_policy_fwd
// x 3 + a3vt_ddqn_td + a3vt_ddqn_td_bwd(grad_loss = 1) + a3vt_latent_policy_bwd(accumulate = 0).  No atomics, no fences between
// workgroups, no host synchronisation, no allocation.
#include "policy_dev.h"

namespace a3vt {

namespace {

__global__ __launch_bounds__(kFwdThreads) void ddqn_latent_q_kernel(PolicyNet net, const float *__restrict__ mask,
                                                                    const float *__restrict__ latent,
                                                                    const float *__restrict__ first_latent,
                                                                    const float *__restrict__ penalty, float *__restrict__ q,
                                                                    int32_t *__restrict__ action) {
  __shared__ __attribute__((aligned(16))) float buf[2][kPolicyMaxWidth];
  const int e = blockIdx.x, ls = net.latent_size, A = net.layer[net.n_layers - 1].out;
  const int cur = policy_row_forward(net, mask + (size_t)e * net.layer[0].in, latent + (size_t)e * ls, first_latent + (size_t)e * ls,
                                     q + (size_t)e * A, nullptr, buf);
  if (!penalty) return;
  __syncthreads();
  if (threadIdx.x >= 64) return;
  float touched;
  const int arg = td_argmax(penalty + (size_t)e * A, buf[cur], A, threadIdx.x, touched);
  if (threadIdx.x == 0) action[e] = arg;
}

__global__ __launch_bounds__(kFwdThreads) void ddqn_latent_fwd_kernel(PolicyNet online, PolicyNet target, const float *__restrict__ mask,
                                                                      const float *__restrict__ mask_n,
                                                                      const float *__restrict__ latent,
                                                                      const float *__restrict__ latent_n,
                                                                      const float *__restrict__ first_latent,
                                                                      float *__restrict__ q_cur, float *__restrict__ q_no,
                                                                      float *__restrict__ q_nt, float *__restrict__ stash, int ld) {
  __shared__ __attribute__((aligned(16))) float buf[2][kPolicyMaxWidth];
  const int e = blockIdx.x, role = blockIdx.y;   // (workgroup-uniform)
  const int ls = online.latent_size, in0 = online.layer[0].in, A = online.layer[online.n_layers - 1].out;
  const float *fl = first_latent + (size_t)e * ls;
  if (role == 0)
    policy_row_forward(online, mask + (size_t)e * in0, latent + (size_t)e * ls, fl, q_cur + (size_t)e * A, stash + (size_t)e * ld, buf);
  else if (role == 1)
    policy_row_forward(online, mask_n + (size_t)e * in0, latent_n + (size_t)e * ls, fl, q_no + (size_t)e * A, nullptr, buf);
  else
    policy_row_forward(target, mask_n + (size_t)e * in0, latent_n + (size_t)e * ls, fl, q_nt + (size_t)e * A, nullptr, buf);
}

__global__ __launch_bounds__(kFwdThreads) void ddqn_latent_td_delta_kernel(PolicyNet net, const float *__restrict__ q_cur,
                                                                           const float *__restrict__ q_no,
                                                                           const float *__restrict__ q_nt,
                                                                           const float *__restrict__ mask,
                                                                           const float *__restrict__ actions,
                                                                           const float *__restrict__ rewards,
                                                                           const float *__restrict__ denom, int batch, float done_at,
                                                                           float gamma, const float *__restrict__ stash,
                                                                           float *__restrict__ delta, int ld, float *__restrict__ diff,
                                                                           int32_t *__restrict__ best_next, float *__restrict__ target) {
  __shared__ float d[2][kPolicyMaxWidth];
  __shared__ float dq[kTdMaxActions];
  __shared__ float row_diff;
  const int b = blockIdx.x, tid = threadIdx.x, A = net.layer[net.n_layers - 1].out;
  const size_t row = (size_t)b * A;
  if (tid < 64) {
    const float dd = td_sample(q_cur + row, q_no + row, q_nt + row, mask + row, actions, rewards, denom, b, A, done_at, gamma, tid, diff,
                               best_next, target);
    if (tid == 0) row_diff = dd;
  }
  __syncthreads();
  int act = (int)actions[b];
  act = act < 0 ? 0 : (act >= A ? A - 1 : act);
  for (int a = tid; a < A; a += kFwdThreads) dq[a] = a == act ? td_dq(1.f, row_diff, batch) : 0.f;
  __syncthreads();
  policy_row_delta(net, dq, stash + (size_t)b * ld, delta + (size_t)b * ld, ld, d);
}

__global__ __launch_bounds__(kGradThreads) void ddqn_latent_grad_kernel(PolicyNet net, PolicyGrads grads, const float *__restrict__ mask,
                                                                        const float *__restrict__ latent,
                                                                        const float *__restrict__ first_latent,
                                                                        const float *__restrict__ stash, const float *__restrict__ delta,
                                                                        int batch, int ld, int slabs, const float *__restrict__ diff,
                                                                        float *__restrict__ loss) {
  __shared__ float sq[kTdMaxBatch];
  if ((int)blockIdx.x < slabs) {   // (workgroup-uniform)
    policy_grad_slab(net, grads, mask, latent, first_latent, stash, delta, batch, ld, 0, blockIdx.x);
    return;
  }
  for (int b = threadIdx.x; b < batch; b += kGradThreads) {
    const float dd = diff[b];
    sq[b] = dd * dd;
  }
  __syncthreads();
  td_loss_tree(sq, batch, loss);
}

}  // namespace

int launch_ddqn_latent_q(const PolicyNet &net, const float *mask, const float *latent, const float *first_latent, const float *penalty,
                         int rows, float *q, int32_t *action, hipStream_t s) {
  A3VT_LAUNCH(ddqn_latent_q_kernel, dim3(rows), dim3(kFwdThreads), 0, s, net, mask, latent, first_latent, penalty, q, action);
  A3VT_CHECK_LAUNCH();
  return 0;
}

int launch_ddqn_latent_update(const PolicyNet &online, const PolicyNet &target_net, const PolicyGrads &grads, const DdqnLatentArgs &a,
                              hipStream_t s) {
  const int A = online.layer[online.n_layers - 1].out, ld = a.ld;
  float *q_no = a.scratch, *q_nt = q_no + (size_t)a.batch * A, *stash = q_nt + (size_t)a.batch * A, *delta = stash + (size_t)a.batch * ld;
  A3VT_LAUNCH(ddqn_latent_fwd_kernel, dim3(a.batch, 3), dim3(kFwdThreads), 0, s, online, target_net, a.mask, a.mask_n, a.latent, a.latent_n,
              a.first_latent, a.q_cur, q_no, q_nt, stash, ld);
  A3VT_CHECK_LAUNCH();
  A3VT_LAUNCH(ddqn_latent_td_delta_kernel, dim3(a.batch), dim3(kFwdThreads), 0, s, online, a.q_cur, q_no, q_nt, a.mask, a.actions, a.rewards,
              a.denom, a.batch, (float)(a.budget - 1), a.gamma, stash, delta, ld, a.diff, a.best_next, a.target);
  A3VT_CHECK_LAUNCH();
  const int slabs = policy_grad_slabs(online);
  A3VT_LAUNCH(ddqn_latent_grad_kernel, dim3(slabs + 1), dim3(kGradThreads), 0, s, online, grads, a.mask, a.latent, a.first_latent, stash, delta,
              a.batch, ld, slabs, a.diff, a.loss);
  A3VT_CHECK_LAUNCH();
  return 0;
}

}  // namespace a3vt
