"""What ``LEBA.py`` and ``MFBA.py`` share: the engine around the per-batch bookkeeping (the reference's two files repeat it line for
line) — the sweep over 40 % of the training batches, the replay of the trajectory chosen so far, checkpoints, ``validate``, the
flags.  A subclass says how its per-action state starts (``fresh_state``), what one swept batch adds to it (``tally_fused`` /
``tally_loop``) and which action a finished sweep chooses (``choose``).  The parts every policy engine has are
``policies/_core.py``'s."""
import os
import random
import sys

import numpy as np
import torch

from ...utility import utils
from .. import _core

SAVE_EVERY = 20


def swept_batches(training_length, seed):
    """The batches a sweep visits (reference LEBA.py:87-90): ``random.sample`` of 40 % of them after ``random.seed(seed)``."""
    random.seed(seed)
    return random.sample(range(training_length), int(training_length * 0.4))


class SweepEngine(_core.EngineBase):
    name = None                # "LEBA" / "MFBA": the checkpoint directory and the pretrained files' prefix
    state_names = ()           # the per-action float64 arrays, in the checkpoint under these keys

    def __init__(self, args, sampler=None, loaders=None):
        super().__init__(args, sampler, loaders)
        self._state = {}

    # ---- the per-action state: fp64 tensors on the environment's device with the knob on, NumPy arrays with it off ----------------
    @property
    def fused(self):
        knob = getattr(self.args, "fused_tally", None)
        return sys.modules[type(self).__module__].FUSED_TALLY_DEFAULT if knob is None else bool(knob)

    def get_state(self, name):
        """A state array as the reference keeps it: NumPy float64 (with the knob on: one copy from the device)."""
        value = self._state[name]
        return value.cpu().numpy() if isinstance(value, torch.Tensor) else value

    def set_state(self, name, value):
        value = np.array(value, dtype=np.float64)
        if value.shape != (self.args.num_actions,):
            raise ValueError(f"{self.name}: `{name}` holds {value.shape} values for {self.args.num_actions} actions")
        self._state[name] = torch.from_numpy(value).to(self.env.device) if self.fused else value

    def reset_state(self):
        for name, value in self.fresh_state().items():
            self.set_state(name, value)

    # ---- the reference's methods --------------------------------------------------------------------------------------------------
    def __call__(self):
        _core.refuse_visualize(self.args)
        self.make_env()
        data_loaders, valid_loaders = self.get_loaders()
        self.chosen_actions = []
        self.step = 0
        self.spot = 0
        self.reset_state()
        self.results_dir = os.path.join("results", self.args.exp_type)
        os.makedirs(self.results_dir, exist_ok=True)
        self.checkpoint_dir = os.path.join("experiments/checkpoint/", self.name, self.args.exp_type)
        os.makedirs(self.checkpoint_dir, exist_ok=True)
        self.checkpoint = os.path.join(self.checkpoint_dir, "actions.npy")
        with torch.no_grad():
            self.load()
            if self.args.eval:
                return self.validate(valid_loaders)
            for _ in range(self.step, self.args.num_grasps):
                self.train(data_loaders)
                self.save()

    def train(self, dataloader):
        """One sweep (reference LEBA.py:83-143, MFBA.py:76-111): the next action of the trajectory.  Batches before ``spot`` are
        skipped; batch ``spot`` itself is swept again on a resume, as in the reference."""
        print(f"Getting best action for step {len(self.chosen_actions) + 1}")
        training_instances = swept_batches(len(dataloader), self.args.seed)
        tally = self.tally_fused if self.fused else self.tally_loop
        for v, batch in enumerate(dataloader):
            if v < self.spot or v not in training_instances:
                continue
            self.spot = v
            self.env.reset(batch)
            for action in self.chosen_actions:
                self.env.step(np.array([action for _ in range(self.args.env_batch_size)]))
            tally()
            if v % SAVE_EVERY == 0:
                self.save()
        self.chosen_actions.append(self.choose())
        self.reset_state()
        self.spot = 0
        self.step += 1

    def take_step(self, t, obs):
        best_actions = np.array([self.chosen_actions[t] for _ in range(self.args.env_batch_size)])
        obs, _, done = self.env.step(best_actions)
        return best_actions, obs, done

    def validate(self, dataloader):
        """The fixed trajectory on every batch (reference LEBA.py:146-204) -> the closing figures; ``scores`` (n, steps + 1),
        ``chosen`` (n, steps) and ``names`` stay on the engine."""
        _core.refuse_visualize(self.args)
        scores, actions, names = [], [], []
        for batch in dataloader:
            names += batch["names"]
            cur_scores, cur_actions = self.play(self.env.reset(batch), self.take_step, steps=len(self.chosen_actions))
            scores.append(cur_scores)
            actions.append(cur_actions)
            now = _core.summary(cur_scores)
            print(f"Valid || score: {now['score']:.4f}, reward = {now['reward']:.4f}")
        return self.report(scores, actions, names)

    def location(self):
        """Where ``load`` reads from: the pretrained file by the reference's ``(use_img, finger)`` rule, else the checkpoint, else
        the reference's separator-less name of it; None when there is none."""
        if self.args.pretrained:
            return os.path.join(utils.pretrained_root(self.args), "policies", "dataset_specific",
                                f"{self.name}_{_core.kind(self.args)}.npy")
        for path in (self.checkpoint, self.checkpoint_dir + "actions.npy"):
            if os.path.exists(path):
                return path
        return None

    def load(self):
        location = self.location()
        if location is None:
            return
        data = np.load(location, allow_pickle=True).item()
        chosen = [np.int64(a) for a in np.asarray(data["chosen_actions"]).reshape(-1)]
        if any(a < 0 or a >= self.args.num_actions for a in chosen):
            raise ValueError(f"{self.name}: {location} holds chosen actions outside [0, {self.args.num_actions}): {chosen}")
        for name in self.state_names:
            self.set_state(name, data[name])
        self.chosen_actions = chosen
        self.spot = int(data["spot"])
        self.step = int(data["step"])

    def save(self):
        """The reference's file (LEBA.py:247-255): ``np.save`` of a dict with its keys."""
        data = {name: self.get_state(name) for name in self.state_names}
        data.update(chosen_actions=self.chosen_actions, step=self.step, spot=self.spot)
        np.save(self.checkpoint, data)


def get_parser():
    """The reference's flags and defaults (LEBA.py:259-342; MFBA's are the same) and this package's."""
    parser = _core.common_parser(auto_location=True, pretrained=True, latent_flags=True, greedy_checks=True)
    parser.add_argument("--eval", action="store_true", default=False, help="Evaluate the trained model on the test set.")
    parser.add_argument("--fused_tally", dest="fused_tally", action="store_true", default=None,
                        help="keep the per-action state on the GPU: one a3vt_candidate_tally launch per swept batch")
    parser.add_argument("--no_fused_tally", dest="fused_tally", action="store_false",
                        help="the reference's per-pair host loop on the host copy of the score table")
    return parser


def run(engine_class, argv=None):
    return _core.run(engine_class, get_parser(), argv)
