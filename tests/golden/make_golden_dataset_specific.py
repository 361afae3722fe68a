#!/usr/bin/env python
"""Generate ``g22_dataset_specific.npz`` by running the REAL reference's dataset-specific engines
(``policies/dataset_specific/LEBA.py`` and ``MFBA.py``) on the CPU (``python tests/golden/make_golden_dataset_specific.py``, build
container only; see ``make_golden_nn.py``, whose recipe this follows: ``oracle.ref_shim``, stubbed simulator modules,
``get_loaders`` a no-op, seeded models written to temporary checkpoint directories, the injected-sample Chamfer distance).

The models, settings and surface draws are ``env_util``'s case "b" (four fingers, E = 2, 6 actions); batches and sensor records
are ``tally_util``'s: five train batches, of which ``int(5 * 0.4) = 2`` are swept, and two validation batches.  For each engine
``Engine.train`` is driven directly for three sweeps — full search, limited search (``greedy_checks = 3``), full search — and then
``Engine.validate`` on the two validation batches.  ``LEBA.py`` imports ``tqdm.notebook``; both modules' ``tqdm`` is replaced by a
pass-through after import.

Stored (weights and images are NOT stored: the tests rebuild them from the seeds and check the checksums):
  seed                               the recipe seed the conditions below hold for
  sha:<kind>, bn:<key>               checksums of the three state dicts; every BatchNorm tensor of the touch encoder
  face_idx|u|v                       injected surface draws (3, E, 700)
  leba:<s>:action_scores|checks      LEBA's sums and visit counts at the end of sweep s, as the reference's ``argmin`` saw them
  mfba:<s>:counts                    MFBA's votes at the end of sweep s, as ``argmax`` saw them
  mfba:<s>:actions                   (swept batches, E) the greedy actions of sweep s, batch after batch
  leba|mfba:<s>:chosen               ``chosen_actions`` after sweep s
  leba|mfba:valid:scores             (VALID_BATCHES * E, 1 + 3) the scores ``validate`` prints its figures from
Asserted here, the smallest values printed; the recipe is re-seeded until the reference alone satisfies them:
  * every MFBA greedy decision has a relative gap of at least 1e-2 between its two lowest eligible scores;
  * every sweep's chosen action beats the runner-up's mean ratio (LEBA) by at least 1e-2 relative;
  * every sweep's chosen action beats the runner-up's votes (MFBA) by at least one vote;
  * at least one action is visited in both swept batches."""
import importlib
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import save  # noqa: E402  (installs the import shim)
from make_golden_env import StubSampler, reference_setup  # noqa: E402
import env_util as eu  # noqa: E402
import tally_util as tl  # noqa: E402


class PassThrough:
    """``tqdm`` without the bar: ``tqdm(iterable)`` and ``tqdm.write``."""

    def __new__(cls, iterable, *a, **k):
        return iterable

    write = staticmethod(print)


class NumpyWatch:
    """The module's ``np`` with ``argmin`` / ``argmax`` calling back first: what the engine decides a sweep on."""

    def __init__(self, seen):
        self.seen = seen

    def __getattr__(self, name):
        return getattr(np, name)

    def argmin(self, x):
        self.seen(np.array(x))
        return np.argmin(x)

    def argmax(self, x):
        self.seen(np.array(x))
        return np.argmax(x)


class Unfit(Exception):
    pass


def need(condition, message):
    if not condition:
        raise Unfit(message)


def run(name, mod, env_mod, seed, locations, root):
    """Three sweeps and a validation of the reference's ``mod.Engine`` -> the fixture's entries of that engine."""
    out, n = {}, eu.CASES[tl.CASE]["num_actions"]
    engine = mod.Engine(tl.engine_args(False, **locations))
    engine.env = env = env_mod.ActiveTouch(engine.args)
    engine.chosen_actions, engine.step, engine.spot = [], 0, 0
    if name == "leba":                                            # the state as __call__ makes it (LEBA.py:32-38, MFBA.py:31)
        engine.action_scores, engine.checks = np.array([1e10 for _ in range(n)]), np.array([1.0 for _ in range(n)])
    else:
        engine.counts = np.array([0.0 for _ in range(n)])
    engine.checkpoint = os.path.join(root, name + "_actions.npy")
    decided, scored, greedy = [], [], []
    mod.np = NumpyWatch(lambda x: decided.append({k: np.array(getattr(engine, k)) for k in
                                                  (("action_scores", "checks") if name == "leba" else ("counts",))}))
    compute_obs, best_step = env.compute_obs, env.best_step

    def logged_obs(actions=None):
        obs = compute_obs(actions)
        scored.append((None if actions is None else [int(a) for a in actions], obs["score"].numpy().astype(np.float64)))
        return obs

    def logged_best(greedy_checks=None):
        mask, start = env.current_data["mask"].numpy().copy(), len(scored)
        res = best_step(greedy_checks=greedy_checks)
        table = scored[start:-1]                                  # (the last entry is the step best_step ends with)
        full = greedy_checks is None or greedy_checks >= n
        gaps = []
        for e in range(eu.E):
            s = sorted(sc[e] for a, sc in table if not full or mask[e][a[e]] == 0)
            gaps.append((s[1] - s[0]) / s[0])
        greedy.append((np.asarray(res[0]).astype(np.int64), min(gaps)))
        return res

    env.compute_obs, env.best_step = logged_obs, logged_best
    smallest = {"decision": np.inf, "choice": np.inf}
    both = False
    with torch.no_grad():
        for s in range(tl.SWEEPS):
            engine.args.greedy_checks = tl.GREEDY_CHECKS[s]
            before = len(greedy)
            engine.train(tl.batches(seed, "train"))
            state = decided[-1]
            chosen = int(engine.chosen_actions[-1])
            if name == "leba":
                out[f"leba:{s}:action_scores"], out[f"leba:{s}:checks"] = state["action_scores"], state["checks"]
                mean = np.sort(state["action_scores"] / state["checks"])
                gap = (mean[1] - mean[0]) / mean[0]
                need(gap >= tl.MIN_GAP, f"LEBA sweep {s}: the chosen mean leads by {gap:.2e}")
                # (2 * E visits of one action need both swept batches; every full-search sweep has them, so this says nothing
                # about the limited-search sweep, whose actions may each be met in one batch only)
                both = both or state["checks"].max() >= 1 + 2 * eu.E
            else:
                out[f"mfba:{s}:counts"] = state["counts"]
                out[f"mfba:{s}:actions"] = np.stack([g[0] for g in greedy[before:]])
                votes = np.sort(state["counts"])
                gap = votes[-1] - votes[-2]
                need(gap >= 1, f"MFBA sweep {s}: votes {state['counts']}")
                decision = min(g[1] for g in greedy[before:])
                need(decision >= tl.MIN_GAP, f"MFBA sweep {s}: a greedy decision's gap is {decision:.2e}")
                smallest["decision"] = min(smallest["decision"], decision)
                both = True                                       # (LEBA's condition: MFBA visits nothing)
            smallest["choice"] = min(smallest["choice"], gap)
            out[f"{name}:{s}:chosen"] = np.array(engine.chosen_actions, dtype=np.int64)
            print(f"{name} sweep {s} (greedy_checks {tl.GREEDY_CHECKS[s]}): {state} -> {chosen}")
        need(len(set(int(a) for a in engine.chosen_actions)) == tl.SWEEPS, "an action was chosen twice")
        need(both, "no action is visited in both swept batches")
        # ---- validate: the scores it prints its figures from ------------------------------------------------------------------
        env.compute_obs, env.best_step = compute_obs, best_step
        episodes = []
        reset, step = env.reset, env.step
        env.reset = lambda batch: (lambda obs: episodes.append([obs["score"]]) or obs)(reset(batch))
        env.step = lambda actions: (lambda res: episodes[-1].append(res[0]["score"]) or res)(step(actions))
        engine.validate(tl.batches(seed, "valid"))
    out[f"{name}:valid:scores"] = torch.cat([torch.stack(ep).permute(1, 0) for ep in episodes]).numpy()
    print(f"{name}: chosen {[int(a) for a in engine.chosen_actions]}, smallest gaps {smallest}, validate scores\n{out[f'{name}:valid:scores']}")
    return out


def main():
    with reference_setup(tl.CASE) as setup:
        engines = {"leba": importlib.import_module("pterotactyl.policies.dataset_specific.LEBA"),
                   "mfba": importlib.import_module("pterotactyl.policies.dataset_specific.MFBA")}
        for mod in engines.values():
            mod.tqdm = PassThrough
        for attempt in range(200):
            seed = tl.SEED + 100 * attempt
            out = dict(setup.out, seed=np.int64(seed))
            StubSampler.records, StubSampler.log = tl.records(seed), []
            with setup.workdir() as (root, locations):
                try:
                    for name in ("mfba", "leba"):
                        out.update(run(name, engines[name], setup.env_mod, seed, locations, root))
                except Unfit as e:
                    print(f"seed {seed}: {e}: re-seeding")
                    continue
            if seed != tl.SEED:
                print(f"set tally_util.SEED = {seed}: the first seed the conditions hold for")
            save(tl.FIXTURE, **out)
            return
    raise SystemExit("no seed found")


if __name__ == "__main__":
    main()
