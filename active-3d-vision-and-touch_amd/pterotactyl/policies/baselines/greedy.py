"""``pterotactyl.policies.baselines.greedy``: the myopic greedy oracle's evaluation run (reference
``policies/baselines/greedy.py``) — every step is ``ActiveTouch.best_step(greedy_checks)``.  The reference builds (and resets) an
``even_sampler`` it never asks for an action; so does this runner, which keeps Python's ``random`` stream in step with it."""
from . import _runner, baselines


class Engine(_runner.Engine):
    policy_class = baselines.even_sampler
    resets_policy = True
    greedy = True


if __name__ == "__main__":
    _runner.main(Engine)
