"""The validate loop the three baseline runners share (reference ``policies/baselines/{rand,even,greedy}.py``: the three files
differ in which sampler they build and in the one line that takes a step).  ``Engine(args, sampler=None)`` passes ``sampler`` on
to ``ActiveTouch`` (``policies/environment.py``); the ``visualize`` paths of the reference render with pyrender and are not
built here."""
import argparse
import os

import torch
from torch.utils.data import DataLoader

from ...utility import utils
from .. import environment
from . import baselines


def summary(scores):
    """``scores`` (n, steps + 1): the reference's closing figures (``greedy.py:100-102``) — ``score`` = mean of last / first,
    ``reward`` = mean of (first - last) / first."""
    return {"score": (scores[:, -1] / scores[:, 0]).mean(), "reward": ((scores[:, 0] - scores[:, -1]) / scores[:, 0]).mean()}


class Engine:
    policy_class = None        # the action sampler the runner builds
    resets_policy = False      # whether validate() calls policy.reset() per batch
    greedy = False             # True: env.best_step(greedy_checks); False: env.step(policy.get_action(mask))
    num_workers = 4

    def __init__(self, args, sampler=None):
        self.args = args
        self.sampler = sampler

    def __call__(self):
        if getattr(self.args, "visualize", False):
            raise NotImplementedError("visualize: the reference renders predictions and actions with pyrender, which this package "
                                      "does not have; run without --visualize")
        utils.set_seeds(self.args.seed)
        self.env = environment.ActiveTouch(self.args, sampler=self.sampler)
        self.policy = self.policy_class(self.args)
        self.results_dir = os.path.join("results", self.args.exp_type)
        with torch.no_grad():
            return self.validate(self.get_loaders())

    def get_loaders(self):
        return DataLoader(self.env.valid_data, batch_size=self.args.env_batch_size, shuffle=False,
                          num_workers=getattr(self.args, "num_workers", self.num_workers), collate_fn=self.env.valid_data.collate)

    def take_step(self, obs):
        """One step of the policy: ``(action, next_obs, reward, done)``."""
        if self.greedy:
            return self.env.best_step(greedy_checks=self.args.greedy_checks)
        action = self.policy.get_action(obs["mask"])
        return (action,) + tuple(self.env.step(action))

    def validate(self, dataloader):
        if getattr(self.args, "visualize", False):
            raise NotImplementedError("visualize: needs pyrender, which this package does not have")
        scores, actions, names = [], [], []
        for batch in dataloader:
            names += batch["names"]
            obs = self.env.reset(batch)
            if self.resets_policy:
                self.policy.reset()
            all_done = False
            cur_scores, cur_actions = [obs["score"]], []
            while not all_done:
                with torch.no_grad():
                    action, obs, reward, all_done = self.take_step(obs)
                cur_scores.append(obs["score"])
                cur_actions.append(torch.FloatTensor(action))
            scores.append(torch.stack(cur_scores).permute(1, 0))
            actions.append(torch.stack(cur_actions).permute(1, 0))
            now, so_far = summary(scores[-1]), summary(torch.cat(scores))
            print(f"Valid || score: {now['score']:.4f} reward = {now['reward']:.4f} ave: {100 * so_far['score']:.4f} %")
        total = summary(torch.cat(scores))
        message = f"Total Valid || score: {total['score']:.4f}, reward = {total['reward']:.4f}"
        print("*" * len(message) + "\n" + message + "\n" + "*" * len(message))
        self.scores, self.actions, self.names = torch.cat(scores), torch.cat(actions), names
        return total


def get_parser(greedy=False):
    """The reference runners' flags (``greedy.py:111-188``; ``--greedy_checks`` for the greedy runner alone) and this package's:
    where the dataset and the pretrained models are, and the two knobs of the greedy step."""
    pretrained = os.environ.get("PTEROTACTYL_PRETRAINED", "")
    parser = argparse.ArgumentParser()
    parser.add_argument("--limit_data", action="store_true", default=False, help="use less data, for debugging.")
    parser.add_argument("--finger", action="store_true", default=False, help="use only one finger.")
    parser.add_argument("--touch_location", type=str, default=os.path.join(pretrained, "reconstruction/touch/best/"),
                        help="the location of the touch part prediction.")
    parser.add_argument("--vision_location", type=str, default=os.path.join(pretrained, "reconstruction/vision/t_p/"),
                        help="the location of the vision part prediction.")
    parser.add_argument("--number_points", type=int, default=30000, help="number of points sampled for the chamfer distance.")
    parser.add_argument("--seed", type=int, default=0, help="Setting for the random seed.")
    parser.add_argument("--env_batch_size", type=int, default=3, help="Size of the batch.")
    parser.add_argument("--use_img", action="store_true", default=False, help="To use the image.")
    parser.add_argument("--loss_coeff", type=float, default=9000.0, help="Coefficient for loss term.")
    parser.add_argument("--num_grasps", type=int, default=5, help="Number of grasps to train with. ")
    if greedy:
        parser.add_argument("--greedy_checks", type=int, default=50, help="Number of actions to check at each time step")
    parser.add_argument("--num_actions", type=int, default=50, help="number of action options")
    parser.add_argument("--use_latent", action="store_true", default=False)
    parser.add_argument("--use_recon", action="store_true", default=False)
    parser.add_argument("--eval", type=bool, default=True, help="for evaluating on test set")
    parser.add_argument("--budget", type=int, default=5, help="number of graspsp to perform")
    parser.add_argument("--visualize", action="store_true", default=False, help="not built: needs pyrender")
    parser.add_argument("--exp_type", type=str, default="test", help="The experiment group.")
    parser.add_argument("--pretrained_recon", action="store_true", default=False,
                        help="use the pretrained reconstruction models to train")
    parser.add_argument("--data_root", type=str, default=None, help="dataset directory (default: PTEROTACTYL_DATA)")
    parser.add_argument("--pretrained_root", type=str, default=None, help="pretrained/ directory (default: PTEROTACTYL_PRETRAINED)")
    parser.add_argument("--recorded", type=str, default=None,
                        help="replay touch signals from this dataset root's grasp_info/ (RecordedSampler) instead of simulating")
    if greedy:
        parser.add_argument("--no_batched_greedy", dest="batched_greedy", action="store_false", default=None,
                            help="score the greedy candidates one at a time, as the reference does")
        parser.add_argument("--candidate_chunk", type=int, default=None, help="greedy candidates per batch (default: all)")
    return parser


def main(engine_class):
    args = get_parser(greedy=engine_class.greedy).parse_args()
    sampler = None
    if args.recorded:
        from ..recorded import RecordedSampler
        sampler = RecordedSampler(args.recorded)
    engine_class(args, sampler=sampler)()


__all__ = ["Engine", "baselines", "get_parser", "main", "summary"]
