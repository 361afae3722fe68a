"""``pterotactyl.policies.baselines.baselines``: the random and the evenly spaced action samplers (reference
``policies/baselines/baselines.py:10-57``).  Host code; it makes the reference's ``random`` / ``numpy`` calls in the reference's
order, so a seeded run picks the same actions."""
import random

import numpy as np


def _host(mask):
    return mask.detach().cpu().numpy() if hasattr(mask, "detach") else np.asarray(mask)


class random_sampler:
    """One uniformly drawn action per sample among those its mask has not used yet."""

    def __init__(self, args):
        self.args = args

    def get_action(self, mask):
        mask = _host(mask)
        picked = []
        for row in mask:
            free = list(np.arange(self.args.num_actions))
            for used in sorted(np.where(row > 0)[0], reverse=True):
                del free[used]
            picked.append(random.choice(free))      # one draw per sample, as the reference
        return np.array(picked)


class even_sampler:
    """``num_grasps`` actions spread evenly over the action range from a random offset per environment, dealt out in order."""

    def __init__(self, args):
        self.args = args
        self.generate_points()

    def generate_points(self):
        n, grasps = self.args.num_actions, self.args.num_grasps
        self.angles = []
        for _ in range(self.args.env_batch_size):
            step = n // grasps
            offset = random.choice(range(n))        # one draw per environment, as the reference
            self.angles.append([(step * j + offset) % n for j in range(grasps)])

    def reset(self):
        self.generate_points()

    def get_action(self, mask):
        return np.array([self.angles[b].pop(0) for b in range(mask.shape[0])])
