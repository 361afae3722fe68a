"""Drop-in for ``pterotactyl/policies/dataset_specific/LEBA.py`` — "lowest error best action", a fixed trajectory for the whole
dataset.

Every sweep adds one action to the trajectory: on 40 % of the training batches the actions chosen so far are replayed, every
remaining action (or ``greedy_checks`` of them per element) is tried, the score it reaches divided by the element's first score
is added to the action's sum, and the action with the lowest mean ratio is chosen.  ``validate`` replays the trajectory.

``Engine(args, sampler=None, loaders=None)`` has the reference's methods (``__call__``, ``get_loaders``, ``train``, ``validate``,
``load``, ``save``) and attributes (``chosen_actions``, ``step``, ``spot``, ``action_scores``, ``checks``, ``results_dir``,
``checkpoint_dir``, ``checkpoint``); ``sampler`` goes to ``ActiveTouch`` (``policies/environment.py``), ``loaders=(train, valid)``
injects data.  ``get_parser()`` carries the reference's flags and defaults (:259-342) and this package's ``--auto_location``,
``--data_root``, ``--pretrained_root``, ``--recorded``, ``--fused_tally`` / ``--no_fused_tally``.

**A swept batch is two library calls** (``args.fused_tally``, default ``FUSED_TALLY_DEFAULT``).  With the knob on
``action_scores`` and ``checks`` live on the device as fp64 tensors, the batch's first scores are uploaded once per ``reset``, and
the batch is one ``env.score_candidates(candidates, to_host=False)`` and one ``ops.candidate_tally`` (``a3vt_candidate_tally``,
csrc/candidate_tally.hip: one launch).  Nothing comes to the host until ``save()`` or the end of the sweep; the attributes read
back as NumPy float64 arrays.  With the knob off the reference's loop over the K * E pairs runs on the host copy of the table,
with the reference's own expression ``self.action_scores[action] += score`` on a 0-d fp32 tensor.

**The sum is an fp32 sum kept in a float64 array.**  ``np.float64 + <0-d fp32 tensor>`` defers to torch and gives an fp32
tensor, so the reference rounds the running sum to fp32 at every add; the kernel's contract (``include/a3vt.h``) says the same,
and the two forms here are bit-equal.

What differs from the reference, and why:

* The candidates of a batch are scored by ONE ``score_candidates`` call (the batched candidate step of ``environment.py``).  The
  reference calls ``check_step`` twice per candidate — once for ``score``, once for ``first_score`` — for the same numbers.
* The checkpoint is ``os.path.join(checkpoint_dir, "actions.npy")``.  The reference's own name, ``checkpoint_dir + "actions.npy"``
  without a separator (``experiments/checkpoint/LEBA/<exp_type>actions.npy``), is read as a fallback when the former does not exist.
* ``load`` does nothing when there is no file, and raises on a file it cannot read; the reference's bare ``except`` hides both.
  Chosen actions outside ``[0, num_actions)`` and state arrays of another length are refused.
* Pretrained trajectories resolve to ``<pretrained_root>/policies/dataset_specific/LEBA_{v_t_p,v_t_g,t_p,t_g}.npy``
  (``args.pretrained_root`` or ``PTEROTACTYL_PRETRAINED``) by the reference's ``(use_img, finger)`` rule; the reference reads them
  from inside its package.
* ``train`` resumes from ``spot`` as the reference does: batch ``spot`` itself is swept AGAIN, so sums saved after batch ``spot``
  count it twice after a resume.  Kept as it is.
* ``validate`` returns the closing figures and keeps ``scores``, ``chosen`` and ``names``; the reference prints them.
* No progress bar (``tqdm.notebook`` in the reference).
* ``visualize`` raises ``NotImplementedError``: ``utils.visualize_prediction`` and ``utils.visualize_actions`` need pyrender and
  are not in this package's ``utils``.
"""
import random

import numpy as np
import torch

from .... import ops
from . import _engine
from ._engine import get_parser  # noqa: F401  (the module's interface)

# Whether a swept batch is tallied on the device when args does not say: on only if the fused batch's p90 host wall lies below the
# loop's p10 at both sizes on an MI355X (tools/tally_bench.py -> profiles/candidate_tally_ab.txt).
FUSED_TALLY_DEFAULT = True

UNVISITED, CHOSEN = 1e10, 1e20


def remaining_candidates(chosen_actions, num_actions, env_batch_size, greedy_checks):
    """The candidates of one swept batch (reference :103-118): ``candidates[k][e]`` is the action candidate k tries on element e.
    Every action not chosen yet, for every element; with ``greedy_checks < num_actions`` per element
    ``random.sample(remaining, greedy_checks)``, drawn in element order from Python's global ``random``."""
    open_actions = [a for a in range(num_actions) if a not in chosen_actions]
    if greedy_checks < num_actions:
        per_element = [random.sample(open_actions, greedy_checks) for _ in range(env_batch_size)]
    else:
        per_element = [open_actions] * env_batch_size
    return [[per_element[e][k] for e in range(env_batch_size)] for k in range(len(per_element[0]))]


class Engine(_engine.SweepEngine):
    name = "LEBA"
    state_names = ("action_scores", "checks")

    action_scores = property(lambda self: self.get_state("action_scores"), lambda self, v: self.set_state("action_scores", v))
    checks = property(lambda self: self.get_state("checks"), lambda self, v: self.set_state("checks", v))

    def fresh_state(self):
        n = self.args.num_actions
        return {"action_scores": [UNVISITED if i not in self.chosen_actions else CHOSEN for i in range(n)], "checks": [1.0] * n}

    def candidates(self):
        return remaining_candidates(self.chosen_actions, self.args.num_actions, self.args.env_batch_size, self.args.greedy_checks)

    def tally_fused(self):
        candidates = self.candidates()
        first = self.env.current_data["first_score"].to(self.env.device, torch.float32)       # (once per reset: this is the batch's)
        scores = self.env.score_candidates(candidates, to_host=False)
        ops.candidate_tally(scores, torch.tensor(candidates, dtype=torch.int32), first, None, sums=self._state["action_scores"],
                            checks=self._state["checks"], unvisited=UNVISITED)

    def tally_loop(self):
        candidates = self.candidates()
        table = self.env.score_candidates(candidates)
        first_score = self.env.current_data["first_score"]
        action_scores, checks = self._state["action_scores"], self._state["checks"]
        for k, actions in enumerate(candidates):
            scores = table[k] / first_score
            for action, score in zip(actions, scores):       # (reference :123-128, its own expressions)
                if action_scores[action] == UNVISITED:
                    action_scores[action] = score
                else:
                    action_scores[action] += score
                checks[action] += 1.0

    def choose(self):
        return np.argmin(self.action_scores / self.checks)


def main(argv=None):
    return _engine.run(Engine, argv)


if __name__ == "__main__":
    main()
