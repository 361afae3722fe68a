// ddqn.hip — the double-DQN target, the loss and the loss gradient as one launch each.
//
// Reference: pterotactyl/policies/DDQN/ddqn.py:100-115.  With q_cur / q_next_online / q_next_target the three Q-network outputs
// [B][A] of an update, per sample b:
//   not_done  = sum_a mask[b][a] < budget - 1                                   (:88, the CURRENT mask)
//   best      = argmax_a (mask[b][a] > 0 ? -1e10 : q_next_online[b][a])         (:105 through penalise_actions; lowest index on a tie)
//   target    = gamma * (not_done ? q_next_target[b][best] : 0) + rewards[b] / denom[b]      (:109-113; denom NULL: plain rewards)
//   diff      = q_cur[b][actions[b]] - target
//   loss      = mean_b diff^2                                                    (:115)
// The reference walks the batch in a Python loop (one device sync per sample) around a dozen small launches.  Here one workgroup
// does the batch: a wave per sample (lanes over the actions), then the mean as a fixed-order tree over the squares kept in LDS —
// no atomics, the same bits on every call.  B <= 4096, A <= 304.
#include "policy_dev.h"   // td_sample, td_loss_tree: the sample rule and the loss tree, shared with ddqn_latent.hip

namespace a3vt {

namespace {

__global__ __launch_bounds__(256) void ddqn_td_kernel(const float *__restrict__ q_cur, const float *__restrict__ q_no,
                                                      const float *__restrict__ q_nt, const float *__restrict__ mask,
                                                      const float *__restrict__ actions, const float *__restrict__ rewards,
                                                      const float *__restrict__ denom, int batch, int na, float done_at, float gamma,
                                                      float *__restrict__ loss, float *__restrict__ diff,
                                                      int32_t *__restrict__ best_next, float *__restrict__ target) {
  __shared__ float sq[kTdMaxBatch];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int b = wave; b < batch; b += 4) {
    const size_t row = (size_t)b * na;
    const float d = td_sample(q_cur + row, q_no + row, q_nt + row, mask + row, actions, rewards, denom, b, na, done_at, gamma, lane, diff,
                              best_next, target);
    if (lane == 0) sq[b] = d * d;
  }
  __syncthreads();
  td_loss_tree(sq, batch, loss);
}

__global__ void ddqn_td_bwd_kernel(const float *__restrict__ diff, const float *__restrict__ actions,
                                   const float *__restrict__ grad_loss, int batch, int na, float *__restrict__ dq) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= batch * na) return;
  const int b = i / na, a = i - b * na;
  int act = (int)actions[b];
  act = act < 0 ? 0 : (act >= na ? na - 1 : act);
  dq[i] = a == act ? td_dq(grad_loss[0], diff[b], batch) : 0.f;
}

}  // namespace

int launch_ddqn_td(const float *q_cur, const float *q_next_online, const float *q_next_target, const float *mask, const float *actions,
                   const float *rewards, const float *denom, int batch, int num_actions, int budget, float gamma, float *loss,
                   float *diff, int32_t *best_next, float *target, hipStream_t s) {
  A3VT_LAUNCH(ddqn_td_kernel, dim3(1), dim3(256), 0, s, q_cur, q_next_online, q_next_target, mask, actions, rewards, denom, batch,
              num_actions, (float)(budget - 1), gamma, loss, diff, best_next, target);
  A3VT_CHECK_LAUNCH();
  return 0;
}

int launch_ddqn_td_bwd(const float *diff, const float *actions, const float *grad_loss, int batch, int num_actions, float *dq_cur,
                       hipStream_t s) {
  A3VT_LAUNCH(ddqn_td_bwd_kernel, dim3(cdiv((long long)batch * num_actions, 256)), dim3(256), 0, s, diff, actions, grad_loss, batch,
              num_actions, dq_cur);
  A3VT_CHECK_LAUNCH();
  return 0;
}

}  // namespace a3vt
