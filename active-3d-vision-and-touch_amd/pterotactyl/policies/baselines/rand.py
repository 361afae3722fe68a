"""``pterotactyl.policies.baselines.rand``: the random policy's evaluation run (reference ``policies/baselines/rand.py``) — each
step takes one uniformly drawn untaken action per element."""
from . import _runner, baselines


class Engine(_runner.Engine):
    policy_class = baselines.random_sampler


if __name__ == "__main__":
    _runner.main(Engine)
