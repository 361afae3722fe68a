"""Drop-in for ``pterotactyl/policies/DDQN/train.py`` — the double-DQN trainer.

An episode is one batch of objects touched ``budget`` times.  Every step the learner (``ddqn.DDQN``) picks an action per object —
at random during ``burn_in`` and afterwards with probability epsilon — the environment (``environment.ActiveTouch``) performs
it, the transition enters the replay memory, and once ``burn_in`` steps have passed every step also updates the Q-network on a
replayed batch; the target network follows every ``target_update`` steps.  After each epoch the greedy policy is validated and the
state of training is checkpointed (reference :44-77, :102-172, :175-257).

``Engine(args, sampler=None, loaders=None)`` has the reference's methods (``__call__``, ``get_loaders``, ``train``, ``validate``,
``check_values_and_save``, ``resume``, ``save``, ``load``) and attributes (``steps``, ``episode``, ``epoch``, ``epsilon``,
``best_loss``, ``current_loss``, ``env``, ``replay_memory``, ``policy``, ``target_net``, ``ave_reward``, ``ave_recon``,
``window_size``, ``results_dir``, ``checkpoint_dir``); ``sampler`` goes to ``ActiveTouch``, ``loaders=(train, valid)`` injects data.
It derives from ``_core.EngineBase`` alone (the reference derives from ``submitit``'s ``Checkpointable``, which only matters to that
scheduler), and ``utils.SummaryWriter`` is a no-op stub when tensorboard is missing.  ``get_parser()`` carries every flag and
default of the reference's ``__main__`` block (:351-524) and this package's: ``--data_root``, ``--pretrained_root``, ``--recorded``
(``_core.common_parser``), ``--replay_device``, ``--fused_q_latent`` / ``--no_fused_q_latent``.

The loop is the reference's, order included: epsilon decays BEFORE the action once ``steps >= burn_in`` (:115-116); actions are
random while ``steps < burn_in`` (:119); ``add_experience`` comes before ``update_parameters`` (:129-133); the target copy happens
when ``steps % target_update == 0 and steps >= burn_in`` (:136-141); the ``ave_*`` windows are written at ``episode % window_size`` and
averaged over ``[: episode + 1]`` (:151-156); ``validate`` chooses with ``eps_threshold=-1`` (:196-198); ``check_values_and_save``
compares ``best_loss >= current_loss`` (:261); ``load`` adds 1 to ``episode`` and ``epoch`` (:341, :348).  A checkpoint is the
reference's dict of nine keys (``dqn_weights``, ``target_weights``, ``args``, ``episode``, ``steps``, ``ave_reward``, ``ave_recon``,
``epsilon``, ``epoch``) in ``{best,recent}_model`` with ``{best,recent}_replay_buffer.pt`` beside it.  A pretrained policy is the
FILE ``<pretrained_root>/policies/DDQN/{l|g}_{v_t_p|v_t_g|t_p|t_g}`` (``checkpoint["dqn_weights"]``), resolved by
``(use_latent, use_img, finger)``; ``pretrained_root`` is ``args.pretrained_root`` or ``PTEROTACTYL_PRETRAINED``
(``utils.pretrained_root``; the reference reads it from inside its package).

``args.fused_q_latent`` (this package's; ``None``: ``FUSED_Q_LATENT_DEFAULT``) is set before the learners are built: a
``Latent_Model`` on the GPU is then evaluated and updated by ``ops.ddqn_latent_q`` / ``ops.ddqn_latent_update`` (see ``ddqn.py``).

What differs from the reference, and why:

* Nothing calls ``.cuda()``: the policy, the target net and the ``ave_*`` windows live on ``policy_device()`` (the environment's
  GPU unless ``engine.device`` says otherwise).
* ``torch.cuda.empty_cache()`` after every step (:142, :206) is dropped: it returns the allocator's blocks to the driver and makes
  every following step allocate them again.
* The third replay write of ``check_values_and_save`` (:272, ``replay_memory.save(self.checkpoint_dir)``) is dropped: it lands
  BESIDE the checkpoint directory (``<checkpoint_dir>_replay_buffer.pt``) and nothing ever reads it; ``save`` has written the
  ``best`` / ``recent`` buffers already.
* ``visualize`` raises ``NotImplementedError`` (pyrender; ``_core.refuse_visualize``).
* ``reset_pybullet`` goes through ``env.reset_pybullet()``, which already handles recorded samplers.
* Checkpoints pickle ``args``, so they are read with ``weights_only=False``.
* ``args.replay_device`` (default ``None``: the host, as the reference) is passed to ``ReplayMemory(device=)``.
"""
import os

import torch

from ...utility import utils
from ...utility.utils import SummaryWriter
from .. import _core, replay
from . import ddqn

# Whether the engine turns the fused latent Q-network on when args does not say: on only if the fused update's p90 lies below the
# torch-module update's p10 at both measured sizes on an MI355X (tools/ddqn_latent_bench.py -> profiles/ddqn_latent_ab.txt).
# Measured, host wall per call at batch 16, 50 actions, latent 200, a host replay memory, both forms alternating in one process:
# one update_parameters at 4 x 200 0.578 ms (p90 0.599) against the modules' 2.190 (p10 2.108), at 5 x 300 (the l_* checkpoints)
# 0.660 (p90 0.680) against 2.418 (p10 2.384); one greedy get_action at E = 3 0.213 (p90 0.221) against 0.383 (p10 0.377) and 0.246
# (p90 0.250) against 0.381 (p10 0.375); a fused update is 3 launches + Adam's one.
FUSED_Q_LATENT_DEFAULT = True

CHECKPOINT_KEYS = ("dqn_weights", "target_weights", "args", "episode", "steps", "ave_reward", "ave_recon", "epsilon", "epoch")


class Engine(_core.EngineBase):
    shuffle_train = True
    empty_train = ""           # (the reference's)

    def __init__(self, args, sampler=None, loaders=None):
        super().__init__(args, sampler, loaders)     # (device: where the learners live)
        self.steps = 0
        self.episode = 0
        self.epoch = 0
        self.best_loss = 10000
        self.epsilon = self.args.epsilon_start
        self.target_updates = []   # the values of `steps` at which the target net was copied (tests)

        self.results_dir = os.path.join("results", args.exp_type, args.exp_id)
        os.makedirs(self.results_dir, exist_ok=True)
        self.checkpoint_dir = os.path.join("experiments/checkpoint/", self.args.exp_type, self.args.exp_id)
        os.makedirs(self.checkpoint_dir, exist_ok=True)
        utils.save_config(self.checkpoint_dir, args)

    def make_learners(self):
        """The policy and its target (:47-52): the same weights, the target in eval mode, both on ``policy_device()``."""
        if getattr(self.args, "fused_q_latent", None) is None:
            self.args.fused_q_latent = FUSED_Q_LATENT_DEFAULT
        dev = self.policy_device()
        self.replay_memory = replay.ReplayMemory(self.args, device=getattr(self.args, "replay_device", None))
        self.policy = ddqn.DDQN(self.args, self.env.mesh_info, self.replay_memory).to(dev)
        self.target_net = ddqn.DDQN(self.args, self.env.mesh_info, None).to(dev)
        self.target_net.load_state_dict(self.policy.state_dict())
        self.target_net.eval()

    def __call__(self):
        _core.refuse_visualize(self.args)
        self.make_env()
        self.make_learners()
        self.writer = SummaryWriter(os.path.join("experiments/tensorboard/", self.args.exp_type))
        self.window_size = 1000
        self.ave_reward = torch.zeros(self.window_size, device=self.policy_device())
        self.ave_recon = torch.zeros(self.window_size, device=self.policy_device())
        train_loader, valid_loaders = self.get_loaders()

        if self.args.eval:
            self.load(best=True)
            with torch.no_grad():
                self.validate(valid_loaders)
            return

        self.resume()
        for epoch in range(self.epoch, self.args.epochs):
            self.train(train_loader)
            self.env.reset_pybullet()
            if self.steps >= self.args.burn_in:
                with torch.no_grad():
                    self.validate(valid_loaders)
                self.env.reset_pybullet()
                self.check_values_and_save()
            self.epoch += 1

    def train(self, dataloader):
        ave_reward = ave_recon = None
        for v, batch in enumerate(dataloader):
            if v > self.args.train_steps - 1:
                break
            obs = self.env.reset(batch)
            all_done = False
            while not all_done:
                if self.steps >= self.args.burn_in:                   # (before the action, as the reference)
                    self.epsilon = self.policy.update_epsilon(self.epsilon, self.args)
                action = self.policy.get_action(obs, eps_threshold=self.epsilon, give_random=self.steps < self.args.burn_in)
                with torch.no_grad():
                    next_obs, reward, all_done = self.env.step(action)
                self.policy.add_experience(action, obs, next_obs, reward)
                if self.steps >= self.args.burn_in:                   # (the transition just pushed can already be drawn)
                    self.last_loss = self.policy.update_parameters(self.target_net)
                if self.steps % self.args.target_update == 0 and self.steps >= self.args.burn_in:
                    print("+" * 5 + " updating target " + "+" * 5)
                    self.target_net.load_state_dict(self.policy.state_dict())
                    self.target_updates.append(self.steps)
                obs = next_obs
                self.steps += 1

            recon = float((obs["score"] / obs["first_score"]).mean().item())
            reward = float(((obs["first_score"] - obs["score"]) / obs["first_score"]).mean().item())
            self.ave_reward[self.episode % self.window_size] = reward
            self.ave_recon[self.episode % self.window_size] = recon
            ave_reward = self.ave_reward[: self.episode + 1].mean()
            ave_recon = self.ave_recon[: self.episode + 1].mean()
            print(f"T Epoch: {self.epoch} Ep: {self.episode}, recon: {recon:.2f}, reward: {reward:.2f}, a_recon: {ave_recon:.2f}, "
                  f"a_reward: {ave_reward:.2f},  eps: {self.epsilon:.3f}, best: {self.best_loss:.3f}")
            self.episode += 1

        if self.steps >= self.args.burn_in and ave_recon is not None:
            self.writer.add_scalars("train_recon_|_", {self.args.exp_id: ave_recon}, self.steps)
            self.writer.add_scalars("train_reward_|_", {self.args.exp_id: ave_reward}, self.steps)

    def take_step(self, t, obs):
        action = self.policy.get_action(obs, eps_threshold=-1, give_random=False)       # greedy
        with torch.no_grad():
            obs, _, done = self.env.step(action)
        return action, obs, done

    def validate(self, dataloader):
        _core.refuse_visualize(self.args)
        scores, actions, names = [], [], []
        print("*" * 30)
        print("Doing Validation")
        for v, batch in enumerate(dataloader):
            names += batch["names"]
            if v > self.args.valid_steps - 1 and not self.args.eval:
                break
            cur_scores, cur_actions = self.play(self.env.reset(batch), self.take_step)
            scores.append(cur_scores)
            actions.append(cur_actions)
            now = _core.summary(cur_scores)
            print(f"Valid || E: {self.epoch}, score: {now['score']:.2f}, best score: {self.best_loss:.2f} reward = {now['reward']:.2f}")

        total = self.report(scores, actions, names, f"Total Valid || E: {self.epoch}, score: {{score:.4f}}, "
                                                    f"best score: {self.best_loss:.4f} reward = {{reward:.2f}}")
        variation = torch.std(self.chosen, dim=0).mean()
        self.current_loss = total["score"]
        if not self.args.eval:
            self.writer.add_scalars("Valid_recon_|_", {self.args.exp_id: self.current_loss}, self.steps)
            self.writer.add_scalars("Valid_reward_|_", {self.args.exp_id: total["reward"]}, self.steps)
            self.writer.add_scalars("epsilon_|_", {self.args.exp_id: self.epsilon}, self.steps)
            self.writer.add_scalars("Valid_variation_|_", {self.args.exp_id: variation}, self.steps)

    def check_values_and_save(self):
        if self.best_loss >= self.current_loss:
            improvement = self.best_loss - self.current_loss
            print(f"Saving with {improvement:.3f} improvement in Chamfer Distance on Validation Set ")
            self.best_loss = self.current_loss
            self.save(best=True)
        print("Saving DQN checkpoint")
        self.save(best=False)

    def resume(self):
        path = self.checkpoint_dir + "/recent"
        if os.path.exists(path + "_model"):
            print("Loading DQN checkpoint")
            self.load(best=False)
            print("Loading replay memory.")
            self.replay_memory.load(path)

    def save(self, best=False):
        path = self.checkpoint_dir + ("/best" if best else "/recent")
        self.replay_memory.save(path)
        torch.save({"dqn_weights": self.policy.state_dict(), "target_weights": self.target_net.state_dict(), "args": self.args,
                    "episode": self.episode, "steps": self.steps, "ave_reward": self.ave_reward, "ave_recon": self.ave_recon,
                    "epsilon": self.epsilon, "epoch": self.epoch}, path + "_model")

    def pretrained_location(self):
        prefix = "l" if self.args.use_latent else "g"
        return os.path.join(utils.pretrained_root(self.args), "policies", "DDQN", f"{prefix}_{_core.kind(self.args)}")

    def load(self, best=True):
        dev = self.policy_device()
        if self.args.pretrained:
            checkpoint = torch.load(self.pretrained_location(), map_location=dev, weights_only=False)
            self.policy.load_state_dict(checkpoint["dqn_weights"])
            return
        path = self.checkpoint_dir + ("/best_model" if best else "/recent_model")
        checkpoint = torch.load(path, map_location=dev, weights_only=False)
        self.policy.load_state_dict(checkpoint["dqn_weights"])
        self.episode = checkpoint["episode"] + 1
        if not self.args.eval:
            self.target_net.load_state_dict(checkpoint["target_weights"])
            self.steps = checkpoint["steps"]
            self.ave_reward = checkpoint["ave_reward"].to(dev)
            self.ave_recon = checkpoint["ave_recon"].to(dev)
            self.epsilon = checkpoint["epsilon"]
            self.epoch = checkpoint["epoch"] + 1


def get_parser():
    """The reference's flags and defaults (:351-522) and this package's."""
    parser = _core.common_parser(auto_location=True, pretrained=True, latent_flags=True)
    parser.add_argument("--cut", type=float, default=0.33, help="share of a GCN layer's features that is aggregated over neighbours (graph model)")
    parser.add_argument("--layers", type=int, default=4, help="layers of the Q-network")
    parser.add_argument("--hidden_dim", type=int, default=200, help="width of the Q-network's hidden layers")
    parser.add_argument("--epochs", type=int, default=1000, help="epochs to train for")
    parser.add_argument("--eval", action="store_true", default=False, help="evaluate the best checkpoint instead of training")
    parser.add_argument("--lr", type=float, default=0.0003, help="Adam's learning rate")
    parser.add_argument("--train_batch_size", type=int, default=16, help="transitions per Q-network update")
    parser.add_argument("--exp_id", type=str, default="test", help="experiment name (checkpoint and results sub-directory)")
    parser.add_argument("--patience", type=int, default=70, help="epochs without improvement tolerated (kept for the reference's flag set)")
    parser.add_argument("--normalization", type=str, choices=["first", "current", "none"], default="first",
                        help="divide the reward by the first score, the current score, or nothing")
    parser.add_argument("--mem_capacity", type=int, default=300, help="transitions the replay memory holds")
    parser.add_argument("--burn_in", type=int, default=20, help="steps of random actions before the first update")
    parser.add_argument("--gamma", type=float, default=0, help="discount of the next state's value")
    parser.add_argument("--epsilon_start", type=float, default=1.0, help="epsilon at the start")
    parser.add_argument("--epsilon_decay", type=float, default=0.9999, help="factor applied to epsilon every step after burn-in")
    parser.add_argument("--epsilon_end", type=float, default=0.01, help="floor of epsilon")
    parser.add_argument("--train_steps", type=int, default=20, help="training episodes per epoch")
    parser.add_argument("--valid_steps", type=int, default=10, help="validation episodes per epoch")
    parser.add_argument("--target_update", type=int, default=3000, help="steps between copies of the policy into the target network")
    parser.add_argument("--replay_device", type=str, default=None,
                        help="keep the replay memory on this device (default: the host, as the reference)")
    parser.add_argument("--fused_q_latent", dest="fused_q_latent", action="store_true", default=None,
                        help="evaluate and update the latent Q-network on the fused kernels")
    parser.add_argument("--no_fused_q_latent", dest="fused_q_latent", action="store_false", help="... on the torch modules")
    return parser


def main(argv=None):
    return _core.run(Engine, get_parser(), argv)


if __name__ == "__main__":
    main()
