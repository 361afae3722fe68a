"""The recipe of ``g21_ddqn_trainer.npz``: what ``golden/make_golden_ddqn_trainer.py`` (which drives the REFERENCE's DDQN
``Engine``) and the trainer tests (which drive this package's) must build alike.

``env_util``'s case "b" models (four fingers, latent 200) with 50 actions, E = 2, budget 2, 700 surface points — the batches, status
tables and sensor records are ``supervised_util``'s (three training batches, one validation batch) — and a latent policy of
hidden_dim 40 and 3 layers.  ``mem_capacity`` 8, ``train_batch_size`` 2, ``burn_in`` 2, ``target_update`` 3, ``gamma`` 0.9, epsilon
0.5 -> x 0.5 -> 0.05.  The three training batches are six steps: two of burn-in, four with an update each (epsilon 0.25, 0.125,
0.0625, 0.05; the target copy at step 3); then one validation batch plays a whole episode."""
import random

import numpy as np
import torch

import supervised_util as su

FIXTURE = "g21_ddqn_trainer.npz"
ENV_CASE = su.ENV_CASE
NUM_ACTIONS, BUDGET, HIDDEN_DIM, LAYERS = 50, 2, 40, 3
SEED = 2100                                    # random.seed / np.random.seed before the training loop; torch.manual_seed too
MIN_CHOICE_GAP = 1e-2                          # the generator's condition on the two highest open Q values of every greedy decision
STORED_WEIGHTS = ("model.model.2.0.weight", "model.action_model.0.0.bias", "model.model.0.0.bias")
STEPS = 6
EPSILONS = (0.5, 0.5, 0.25, 0.125, 0.0625, 0.05)    # the epsilon each step's action was drawn under
TARGET_COPIES = (3,)


def engine_args(**kw):
    """``env_util.env_args`` of the case with the fixture's sizes plus what the engine, the learner and the replay memory read."""
    import env_util as eu
    d = dict(eval=False, num_actions=NUM_ACTIONS, budget=BUDGET, exp_type="g21", exp_id="fixture", pretrained=False, visualize=False,
             use_recon=False, use_latent=True, hidden_dim=HIDDEN_DIM, layers=LAYERS, lr=0.001, normalization="first", mem_capacity=8,
             train_batch_size=2, burn_in=2, target_update=3, gamma=0.9, epsilon_start=0.5, epsilon_decay=0.5, epsilon_end=0.05,
             train_steps=3, valid_steps=1, epochs=1, patience=70, cut=0.33)
    d.update(kw)
    return eu.env_args(ENV_CASE, **d)


def seed_loop():
    random.seed(SEED)
    np.random.seed(SEED)
    torch.manual_seed(SEED)


def open_gap(q, mask):
    """The smallest relative distance between the two highest open Q values of a row (inf with fewer than two)."""
    gap = np.inf
    q, mask = np.asarray(q, dtype=np.float64), np.asarray(mask)
    for e in range(q.shape[0]):
        v = np.sort(q[e][mask[e] == 0])[::-1]
        if v.size >= 2:
            gap = min(gap, (v[0] - v[1]) / max(abs(v[0]), abs(v[1]), 1e-30))
    return gap


class LoopLog:
    """Wraps a learner (the reference's or this package's: the same method names) and records what the fixture stores of every
    training step: the action, whether it was random, the epsilon it was drawn under, the replay indices of the update, its
    loss, and the Q rows a greedy choice saw (computed by ``q_of(learner, obs)``; NaN rows for a random step)."""

    def __init__(self, engine, q_of):
        self.rows = []
        self.engine = engine
        policy = engine.policy
        get_action, update, sampler = policy.get_action, policy.update_parameters, policy.random_sampler
        draws = []
        inner_draw = sampler.get_action

        def drawn(mask):
            draws.append(1)
            return inner_draw(mask)

        sampler.get_action = drawn

        def logged_action(obs, eps_threshold, give_random=False):
            del draws[:]
            q = q_of(policy, obs)
            action = np.asarray(get_action(obs, eps_threshold=eps_threshold, give_random=give_random))
            self.rows.append(dict(action=action.astype(np.int64), random=bool(draws), epsilon=float(eps_threshold), q=q,
                                  mask=np.asarray(torch.as_tensor(obs["mask"]).cpu()).copy(), indices=np.full(2, -1, dtype=np.int64),
                                  loss=np.float64("nan")))
            return action

        def logged_update(target_net):
            loss = update(target_net)
            if loss is not None:
                self.rows[-1]["loss"] = np.float64(loss)
                self.rows[-1]["indices"] = np.asarray(policy.replay.last_indices, dtype=np.int64).copy() \
                    if hasattr(policy.replay, "last_indices") else self.rows[-1]["indices"]
            return loss

        policy.get_action, policy.update_parameters = logged_action, logged_update


weight_sums = su.weight_sums      # (sum, sum of |.|, sum of squares) in fp64: what the fixture keeps of a tensor it does not store whole
