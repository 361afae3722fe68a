"""What the policy runners and trainers share on the host (``baselines/_runner.py``, ``NearestNeighbor/train.py``,
``supervised/train.py``, ``DDQN/train.py``, ``dataset_specific/_engine.py``): the common flags, the one ``main``, the
``(use_img, finger)`` map of the pretrained files, the ``visualize`` refusal, and ``EngineBase`` — construction, data loaders, the
device a policy lives on, and the validation rollout (``play`` one batch to its end, ``report`` the batches).  An engine module
holds what is its own: its flags, its step rule, its per-batch line and what it writes to its log."""
import argparse
import itertools
import os

import torch
from torch.utils.data import DataLoader

from ..utility import utils
from . import environment

# (use_img, finger) -> the name the reference's pretrained policies and reconstruction models carry
KINDS = {(True, True): "v_t_p", (True, False): "v_t_g", (False, True): "t_p", (False, False): "t_g"}


def kind(args):
    return KINDS[(bool(args.use_img), bool(args.finger))]


def summary(scores):
    """``scores`` (n, steps + 1): the reference's closing figures (``greedy.py:100-102``) — ``score`` = mean of last / first,
    ``reward`` = mean of (first - last) / first."""
    return {"score": (scores[:, -1] / scores[:, 0]).mean(), "reward": ((scores[:, 0] - scores[:, -1]) / scores[:, 0]).mean()}


def refuse_visualize(args):
    if getattr(args, "visualize", False):
        raise NotImplementedError("visualize: the reference renders predictions and actions with pyrender, which this package "
                                  "does not have; run without --visualize")


def common_parser(auto_location=False, pretrained=False, latent_flags=False, greedy_checks=False):
    """The flags every runner and trainer has, with the reference's defaults, and this package's ``--data_root``,
    ``--pretrained_root`` and ``--recorded``; the switches add the groups only some of them have."""
    root = os.environ.get("PTEROTACTYL_PRETRAINED", "")
    parser = argparse.ArgumentParser()
    add = parser.add_argument
    add("--limit_data", action="store_true", default=False, help="use less data, for debugging.")
    add("--finger", action="store_true", default=False, help="use only one finger.")
    add("--touch_location", type=str, default=os.path.join(root, "reconstruction/touch/best/"),
        help="the location of the touch part prediction.")
    add("--vision_location", type=str, default=os.path.join(root, "reconstruction/vision/t_p/"),
        help="the location of the vision part prediction.")
    if auto_location:
        add("--auto_location", type=str, default=os.path.join(root, "reconstruction/auto/t_p/"),
            help="the location of the autoencoder part prediction.")
    add("--number_points", type=int, default=30000, help="number of points sampled for the chamfer distance.")
    add("--seed", type=int, default=0, help="Setting for the random seed.")
    add("--env_batch_size", type=int, default=3, help="Size of the batch.")
    add("--use_img", action="store_true", default=False, help="To use the image.")
    add("--loss_coeff", type=float, default=9000.0, help="Coefficient for loss term.")
    add("--num_grasps", type=int, default=5, help="Number of grasps to train with. ")
    add("--num_actions", type=int, default=50, help="number of action options")
    add("--budget", type=int, default=5, help="number of graspsp to perform")
    if greedy_checks:
        add("--greedy_checks", type=int, default=50, help="Number of actions to check at each time step")
    if latent_flags:
        add("--use_latent", action="store_true", default=False, help="act on auto-encoder latents")
        add("--use_recon", action="store_true", default=False, help="act on the predicted mesh")
    add("--visualize", action="store_true", default=False, help="not built: needs pyrender")
    add("--exp_type", type=str, default="test", help="The experiment group.")
    add("--pretrained_recon", action="store_true", default=False, help="use the pretrained reconstruction models to train")
    if pretrained:
        add("--pretrained", action="store_true", default=False, help="use the pretrained policy")
    add("--data_root", type=str, default=None, help="dataset directory (default: PTEROTACTYL_DATA)")
    add("--pretrained_root", type=str, default=None, help="pretrained/ directory (default: PTEROTACTYL_PRETRAINED)")
    add("--recorded", type=str, default=None,
        help="replay touch signals from this dataset root's grasp_info/ (RecordedSampler) instead of simulating")
    return parser


def latent_only(args):
    """The ``after_parse`` of the policies that only act on latents (reference NearestNeighbor/train.py:309-310)."""
    args.use_recon = False
    args.use_latent = True


def run(engine_class, parser, argv=None, after_parse=None):
    """The one ``main``: parse, ``after_parse(args)``, the recorded sampler when ``--recorded`` names one, build and call."""
    args = parser.parse_args(argv)
    if after_parse is not None:
        after_parse(args)
    sampler = None
    if args.recorded:
        from .recorded import RecordedSampler
        sampler = RecordedSampler(args.recorded)
    return engine_class(args, sampler=sampler)()


class EngineBase:
    num_workers = 4
    shuffle_train = False      # whether the training loader shuffles
    empty_train = []           # what stands in for the training loader under --eval

    def __init__(self, args, sampler=None, loaders=None):
        self.args = args
        self.sampler = sampler      # goes to ActiveTouch
        self.loaders = loaders      # (train, valid): injected data
        self.device = None          # where the policy lives; None: the environment's device (the GPU)

    def device_or_default(self):
        return utils._device() if self.device is None else torch.device(self.device)

    policy_device = lookup_device = device_or_default

    def make_env(self):
        self.env = environment.ActiveTouch(self.args, sampler=self.sampler)

    def loader(self, data, shuffle=False):
        return DataLoader(data, batch_size=self.args.env_batch_size, shuffle=shuffle,
                          num_workers=getattr(self.args, "num_workers", self.num_workers), collate_fn=data.collate)

    def get_loaders(self):
        if self.loaders is not None:
            return self.loaders
        train_loader = self.empty_train if self.args.eval else self.loader(self.env.train_data, self.shuffle_train)
        return train_loader, self.loader(self.env.valid_data)

    def play(self, obs, take_step, steps=None):
        """One batch from its ``reset`` observation to its end -> (scores (E, steps + 1), actions (E, steps)).
        ``take_step(t, obs)`` returns ``(action, next_obs, done)``; an action that is no tensor is stored as a ``FloatTensor``.
        The batch ends after ``steps`` steps, or with ``steps=None`` when ``done`` says so."""
        scores, actions = [obs["score"]], []
        for t in itertools.count() if steps is None else range(steps):
            action, obs, done = take_step(t, obs)
            scores.append(obs["score"])
            actions.append(action if isinstance(action, torch.Tensor) else torch.FloatTensor(action))
            if steps is None and done:
                break
        actions = torch.stack(actions).permute(1, 0) if actions else torch.zeros(self.args.env_batch_size, 0)
        return torch.stack(scores).permute(1, 0), actions

    def report(self, batch_scores, batch_actions, names, banner="Total Valid || score: {score:.4f}, reward = {reward:.4f}"):
        """Closes a validation: ``scores`` (n, steps + 1), ``chosen`` (n, steps) and ``names`` stay on the engine, the starred
        ``banner`` (formatted with the closing figures) is printed -> the figures (``summary``)."""
        self.scores, self.chosen, self.names = torch.cat(batch_scores), torch.cat(batch_actions), names
        total = summary(self.scores)
        message = banner.format(**total)
        print("*" * len(message) + "\n" + message + "\n" + "*" * len(message))
        return total
