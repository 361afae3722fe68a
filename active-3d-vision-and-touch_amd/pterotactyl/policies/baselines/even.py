"""``pterotactyl.policies.baselines.even``: the evenly spaced policy's evaluation run (reference ``policies/baselines/even.py``)
— per batch the sampler deals out ``num_grasps`` actions spread over the action range from a random offset."""
from . import _runner, baselines


class Engine(_runner.Engine):
    policy_class = baselines.even_sampler
    resets_policy = True
    num_workers = 10


if __name__ == "__main__":
    _runner.main(Engine)
