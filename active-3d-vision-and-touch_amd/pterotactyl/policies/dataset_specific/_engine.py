"""What ``LEBA.py`` and ``MFBA.py`` share: the engine around the per-batch bookkeeping (the reference's two files repeat it line for
line) — the sweep over 40 % of the training batches, the replay of the trajectory chosen so far, checkpoints, ``validate``, the
flags.  A subclass says how its per-action state starts (``fresh_state``), what one swept batch adds to it (``tally_fused`` /
``tally_loop``) and which action a finished sweep chooses (``choose``)."""
import argparse
import os
import random
import sys

import numpy as np
import torch
from torch.utils.data import DataLoader

from .. import environment
from ..baselines import _runner

KINDS = {(True, True): "v_t_p", (True, False): "v_t_g", (False, True): "t_p", (False, False): "t_g"}   # (use_img, finger)
SAVE_EVERY = 20


def swept_batches(training_length, seed):
    """The batches a sweep visits (reference LEBA.py:87-90): ``random.sample`` of 40 % of them after ``random.seed(seed)``."""
    random.seed(seed)
    return random.sample(range(training_length), int(training_length * 0.4))


class SweepEngine:
    name = None                # "LEBA" / "MFBA": the checkpoint directory and the pretrained files' prefix
    state_names = ()           # the per-action float64 arrays, in the checkpoint under these keys
    num_workers = 4

    def __init__(self, args, sampler=None, loaders=None):
        self.args = args
        self.sampler = sampler
        self.loaders = loaders
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
        if getattr(self.args, "visualize", False):
            raise NotImplementedError("visualize: the reference renders predictions and actions with utils.visualize_prediction and "
                                      "utils.visualize_actions (pyrender), which this package's utils does not have; run without "
                                      "--visualize")
        self.env = environment.ActiveTouch(self.args, sampler=self.sampler)
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

    def get_loaders(self):
        if self.loaders is not None:
            return self.loaders
        workers = getattr(self.args, "num_workers", self.num_workers)
        train_loader = [] if self.args.eval else DataLoader(self.env.train_data, batch_size=self.args.env_batch_size, shuffle=False,
                                                           num_workers=workers, collate_fn=self.env.train_data.collate)
        valid_loader = DataLoader(self.env.valid_data, batch_size=self.args.env_batch_size, shuffle=False, num_workers=workers,
                                  collate_fn=self.env.valid_data.collate)
        return train_loader, valid_loader

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

    def validate(self, dataloader):
        """The fixed trajectory on every batch (reference LEBA.py:146-204) -> the closing figures; ``scores`` (n, steps + 1),
        ``chosen`` (n, steps) and ``names`` stay on the engine."""
        if getattr(self.args, "visualize", False):
            raise NotImplementedError("visualize: needs utils.visualize_prediction / visualize_actions, which this package does not have")
        scores, actions, names = [], [], []
        for batch in dataloader:
            names += batch["names"]
            obs = self.env.reset(batch)
            cur_scores, cur_actions = [obs["score"]], []
            for action in self.chosen_actions:
                best_actions = np.array([action for _ in range(self.args.env_batch_size)])
                obs, _, _ = self.env.step(best_actions)
                cur_scores.append(obs["score"])
                cur_actions.append(torch.FloatTensor(best_actions))
            scores.append(torch.stack(cur_scores).permute(1, 0))
            actions.append(torch.stack(cur_actions).permute(1, 0) if cur_actions else torch.zeros(self.args.env_batch_size, 0))
            now = _runner.summary(scores[-1])
            print(f"Valid || score: {now['score']:.4f}, reward = {now['reward']:.4f}")
        total = _runner.summary(torch.cat(scores))
        message = f"Total Valid || score: {total['score']:.4f}, reward = {total['reward']:.4f}"
        print("*" * len(message) + "\n" + message + "\n" + "*" * len(message))
        self.scores, self.chosen, self.names = torch.cat(scores), torch.cat(actions), names
        return total

    def location(self):
        """Where ``load`` reads from: the pretrained file by the reference's ``(use_img, finger)`` rule, else the checkpoint, else
        the reference's separator-less name of it; None when there is none."""
        if self.args.pretrained:
            root = getattr(self.args, "pretrained_root", None) or os.environ.get("PTEROTACTYL_PRETRAINED")
            if not root:
                raise FileNotFoundError("a3vt: set args.pretrained_root or PTEROTACTYL_PRETRAINED to the directory the reference's "
                                        "download_models.sh fills (pterotactyl/pretrained/)")
            kind = KINDS[(bool(self.args.use_img), bool(self.args.finger))]
            return os.path.join(root, "policies", "dataset_specific", f"{self.name}_{kind}.npy")
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
    pretrained = os.environ.get("PTEROTACTYL_PRETRAINED", "")
    parser = argparse.ArgumentParser()
    parser.add_argument("--limit_data", action="store_true", default=False, help="use less data, for debugging.")
    parser.add_argument("--finger", action="store_true", default=False, help="use only one finger.")
    parser.add_argument("--touch_location", type=str, default=os.path.join(pretrained, "reconstruction/touch/best/"),
                        help="the location of the touch part prediction.")
    parser.add_argument("--vision_location", type=str, default=os.path.join(pretrained, "reconstruction/vision/t_p/"),
                        help="the location of the vision part prediction.")
    parser.add_argument("--auto_location", type=str, default=os.path.join(pretrained, "reconstruction/auto/t_p/"),
                        help="the location of the autoencoder part prediction (with --use_latent).")
    parser.add_argument("--number_points", type=int, default=30000, help="number of points sampled for the chamfer distance.")
    parser.add_argument("--seed", type=int, default=0, help="Setting for the random seed.")
    parser.add_argument("--env_batch_size", type=int, default=3, help="Size of the batch.")
    parser.add_argument("--use_img", action="store_true", default=False, help="To use the image.")
    parser.add_argument("--loss_coeff", type=float, default=9000.0, help="Coefficient for loss term.")
    parser.add_argument("--num_grasps", type=int, default=5, help="Number of grasps to train with. ")
    parser.add_argument("--num_actions", type=int, default=50)
    parser.add_argument("--use_latent", action="store_true", default=False)
    parser.add_argument("--use_recon", action="store_true", default=False)
    parser.add_argument("--eval", action="store_true", default=False, help="Evaluate the trained model on the test set.")
    parser.add_argument("--budget", type=int, default=5, help="number of graspsp to perform")
    parser.add_argument("--visualize", action="store_true", default=False, help="not built: needs pyrender")
    parser.add_argument("--exp_type", type=str, default="test", help="The experiment group.")
    parser.add_argument("--greedy_checks", type=int, default=50, help="Number of actions to check at each time step")
    parser.add_argument("--pretrained_recon", action="store_true", default=False,
                        help="use the pretrained reconstruction models to train")
    parser.add_argument("--pretrained", action="store_true", default=False, help="use the pretrained policy")
    parser.add_argument("--data_root", type=str, default=None, help="dataset directory (default: PTEROTACTYL_DATA)")
    parser.add_argument("--pretrained_root", type=str, default=None, help="pretrained/ directory (default: PTEROTACTYL_PRETRAINED)")
    parser.add_argument("--recorded", type=str, default=None,
                        help="replay touch signals from this dataset root's grasp_info/ (RecordedSampler) instead of simulating")
    parser.add_argument("--fused_tally", dest="fused_tally", action="store_true", default=None,
                        help="keep the per-action state on the GPU: one a3vt_candidate_tally launch per swept batch")
    parser.add_argument("--no_fused_tally", dest="fused_tally", action="store_false",
                        help="the reference's per-pair host loop on the host copy of the score table")
    return parser


def run(engine_class, argv=None):
    args = get_parser().parse_args(argv)
    sampler = None
    if args.recorded:
        from ..recorded import RecordedSampler
        sampler = RecordedSampler(args.recorded)
    return engine_class(args, sampler=sampler)()
