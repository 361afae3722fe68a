"""The validate loop the three baseline runners share (reference ``policies/baselines/{rand,even,greedy}.py``: the three files
differ in which sampler they build and in the one line that takes a step).  ``Engine(args, sampler=None)`` passes ``sampler`` on
to ``ActiveTouch`` (``policies/environment.py``); the ``visualize`` paths of the reference render with pyrender and are not
built here.  The parts every policy engine has are ``policies/_core.py``'s."""
import os

import torch

from ...utility import utils
from .. import _core
from .._core import summary  # noqa: F401  (its old home)
from . import baselines


class Engine(_core.EngineBase):
    policy_class = None        # the action sampler the runner builds
    resets_policy = False      # whether validate() calls policy.reset() per batch
    greedy = False             # True: env.best_step(greedy_checks); False: env.step(policy.get_action(mask))

    def __call__(self):
        _core.refuse_visualize(self.args)
        utils.set_seeds(self.args.seed)
        self.make_env()
        self.policy = self.policy_class(self.args)
        self.results_dir = os.path.join("results", self.args.exp_type)
        with torch.no_grad():
            return self.validate(self.get_loaders())

    def get_loaders(self):
        return self.loader(self.env.valid_data)

    def take_step(self, t, obs):
        """One step of the policy: ``(action, next_obs, done)``."""
        with torch.no_grad():
            if self.greedy:
                action, obs, _, done = self.env.best_step(greedy_checks=self.args.greedy_checks)
            else:
                action = self.policy.get_action(obs["mask"])
                obs, _, done = self.env.step(action)
        return action, obs, done

    def validate(self, dataloader):
        _core.refuse_visualize(self.args)
        scores, actions, names = [], [], []
        for batch in dataloader:
            names += batch["names"]
            obs = self.env.reset(batch)
            if self.resets_policy:
                self.policy.reset()
            cur_scores, cur_actions = self.play(obs, self.take_step)
            scores.append(cur_scores)
            actions.append(cur_actions)
            now, so_far = summary(cur_scores), summary(torch.cat(scores))
            print(f"Valid || score: {now['score']:.4f} reward = {now['reward']:.4f} ave: {100 * so_far['score']:.4f} %")
        total = self.report(scores, actions, names)
        self.actions = self.chosen
        return total


def get_parser(greedy=False):
    """The reference runners' flags (``greedy.py:111-188``; ``--greedy_checks`` for the greedy runner alone) and this package's:
    where the dataset and the pretrained models are, and the two knobs of the greedy step."""
    parser = _core.common_parser(latent_flags=True, greedy_checks=greedy)
    parser.add_argument("--eval", type=bool, default=True, help="for evaluating on test set")
    if greedy:
        parser.add_argument("--no_batched_greedy", dest="batched_greedy", action="store_false", default=None,
                            help="score the greedy candidates one at a time, as the reference does")
        parser.add_argument("--candidate_chunk", type=int, default=None, help="greedy candidates per batch (default: all)")
    return parser


def main(engine_class):
    return _core.run(engine_class, get_parser(greedy=engine_class.greedy))


__all__ = ["Engine", "baselines", "get_parser", "main", "summary"]
