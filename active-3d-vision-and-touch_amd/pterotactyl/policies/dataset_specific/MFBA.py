"""Drop-in for ``pterotactyl/policies/dataset_specific/MFBA.py`` — "most frequent best action", a fixed trajectory for the whole
dataset.

Every sweep adds one action to the trajectory: on 40 % of the training batches the actions chosen so far are replayed, every
element's myopic greedy action is found (the candidate phase of ``ActiveTouch.best_step``), and the action that was some
element's greedy action most often is chosen.  ``validate`` replays the trajectory.

``Engine(args, sampler=None, loaders=None)`` has the reference's methods (``__call__``, ``get_loaders``, ``train``, ``validate``,
``load``, ``save``) and attributes (``chosen_actions``, ``step``, ``spot``, ``counts``, ``results_dir``, ``checkpoint_dir``,
``checkpoint``); ``sampler`` goes to ``ActiveTouch`` (``policies/environment.py``), ``loaders=(train, valid)`` injects data.
``get_parser()`` carries the reference's flags and defaults (:224-308) and this package's ``--auto_location``, ``--data_root``,
``--pretrained_root``, ``--recorded``, ``--fused_tally`` / ``--no_fused_tally``.  ``greedy_actions`` keeps the last swept batch's
greedy actions, (E,) integers.

**A swept batch is two library calls** (``args.fused_tally``, default ``FUSED_TALLY_DEFAULT``).  With the knob on ``counts``
lives on the device as an fp64 tensor and the batch is one ``env.score_candidates(candidates, to_host=False)`` and one
``ops.candidate_tally`` (``a3vt_candidate_tally``, csrc/candidate_tally.hip: one launch makes the greedy choice and the votes);
E int32 values come to the host, to refuse an element that has no action left.  ``counts`` reads back as a NumPy float64 array.
With the knob off ``env.greedy_choice`` decides on the host copy of the table and the reference's loop bumps ``counts``.

What differs from the reference, and why:

* The greedy actions are found but not performed.  The reference calls ``env.best_step``, which also takes the step and computes
  an observation that nothing reads: the next swept batch begins with ``reset``.
* As in ``ActiveTouch.best_step`` here: the lowest eligible score wins whatever its size (the reference starts its search from
  1000), and an element with no action left raises a ``RuntimeError`` — here before anything is scored, by both forms alike.
* The checkpoint is ``os.path.join(checkpoint_dir, "actions.npy")``.  The reference's own name, ``checkpoint_dir + "actions.npy"``
  without a separator (``experiments/checkpoint/MFBA/<exp_type>actions.npy``), is read as a fallback when the former does not exist.
* ``load`` does nothing when there is no file, and raises on a file it cannot read; the reference's bare ``except`` hides both.
  Chosen actions outside ``[0, num_actions)`` and a ``counts`` of another length are refused.
* Pretrained trajectories resolve to ``<pretrained_root>/policies/dataset_specific/MFBA_{v_t_p,v_t_g,t_p,t_g}.npy``
  (``args.pretrained_root`` or ``PTEROTACTYL_PRETRAINED``) by the reference's ``(use_img, finger)`` rule; the reference reads them
  from inside its package.
* ``train`` resumes from ``spot`` as the reference does: batch ``spot`` itself is swept AGAIN, so counts saved after batch ``spot``
  hold its votes twice after a resume.  Kept as it is.
* ``validate`` returns the closing figures and keeps ``scores``, ``chosen`` and ``names``; the reference prints them.
* No progress bar.
* ``visualize`` raises ``NotImplementedError``: ``utils.visualize_prediction`` and ``utils.visualize_actions`` need pyrender and
  are not in this package's ``utils``.
"""
import numpy as np
import torch

from .... import ops
from .. import environment
from . import _engine
from ._engine import get_parser  # noqa: F401  (the module's interface)

# Whether a swept batch is tallied on the device when args does not say: on only if the fused batch's p90 host wall lies below the
# loop's p10 at both sizes on an MI355X (tools/tally_bench.py -> profiles/candidate_tally_ab.txt).
FUSED_TALLY_DEFAULT = True

CHOSEN = -1e20


class Engine(_engine.SweepEngine):
    name = "MFBA"
    state_names = ("counts",)

    counts = property(lambda self: self.get_state("counts"), lambda self, v: self.set_state("counts", v))

    def fresh_state(self):
        return {"counts": [0.0 if i not in self.chosen_actions else CHOSEN for i in range(self.args.num_actions)]}

    def open_mask(self):
        """The batch's taken mask; an element that has performed every action is refused before anything is scored, by both forms
        alike (a limited search would otherwise come back with no candidates at all)."""
        mask = self.env.current_data["mask"]
        closed = torch.where((mask != 0).all(dim=1))[0]
        if len(closed):
            raise RuntimeError(f"MFBA: element {int(closed[0])} has no action left to take")
        return mask

    def tally_fused(self):
        mask = self.open_mask()
        candidates, full = environment.candidate_actions(mask, self.args.num_actions, self.args.greedy_checks)
        scores = self.env.score_candidates(candidates, to_host=False)
        taken = mask.to(self.env.device, torch.float32) if full else None      # (a limited search drew from the open actions already)
        best, _ = ops.candidate_tally(scores, torch.tensor(candidates, dtype=torch.int32), None, taken, votes=self._state["counts"])
        self.greedy_actions = best.cpu().numpy()
        missing = np.where(self.greedy_actions < 0)[0]
        if len(missing):
            raise RuntimeError(f"MFBA: element {int(missing[0])} has no action left to take")

    def tally_loop(self):
        self.open_mask()
        actions, _ = self.env.greedy_choice(greedy_checks=self.args.greedy_checks)
        self.greedy_actions = actions
        counts = self._state["counts"]
        for a in actions:                                      # (reference :98-99)
            counts[a] += 1

    def choose(self):
        return np.argmax(self.counts)


def main(argv=None):
    return _engine.run(Engine, argv)


if __name__ == "__main__":
    main()
