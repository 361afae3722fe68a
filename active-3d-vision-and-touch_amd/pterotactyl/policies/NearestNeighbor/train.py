"""Drop-in for ``pterotactyl/policies/NearestNeighbor/train.py`` — the nearest-neighbour latent policy.

"Training" fills a bank: for 40 % of the training batches, ``budget`` greedy steps (``env.best_step``) each record, per element,
the latent observed BEFORE the step beside the action the greedy search chose.  Validation acts by lookup: at every step each
element takes the action stored with the nearest banked latent whose action it has not performed yet, searched among the
``num_grasps * 5`` nearest (reference :114-137).

``Engine(args, sampler=None, loaders=None)`` has the reference's methods (``__call__``, ``get_loaders``, ``train``, ``validate``,
``load``, ``save``) and attributes (``actions``, ``latents``, ``spot``, ``checkpoint``, ``results_dir``); ``sampler`` goes to
``ActiveTouch`` (``policies/environment.py``), ``loaders=(train, valid)`` injects data.  ``get_parser()`` carries the
reference's flags and defaults (:223-311; ``use_recon = False`` and ``use_latent = True`` are set after parsing) and this
package's ``--data_root``, ``--pretrained_root``, ``--recorded`` and ``--no_fused_lookup``.

**The lookup is one library call.**  The reference computes, per element, a broadcast subtract / square / mean over the bank, a
``topk`` and a Python walk down its result that indexes a host list with a device scalar — a device synchronisation per
candidate — and rebuilds the list of seen actions through ``.cpu()`` in every iteration.  Here ``Engine.choose(obs)`` makes one
``LatentBank.lookup``: ``ops.latent_nearest`` (``a3vt_latent_nearest``, csrc/latent_nn.hip — two launches for all elements,
with ``obs["mask"]`` as the record of what has been performed) and one copy of E integers to the host.  ``args.fused_lookup``
(default ``FUSED_LOOKUP_DEFAULT``) selects it; with the knob off the reference's per-element loop runs on torch ops
(``reference_lookup``), kept for the tests and for ``tools/nn_lookup_bench.py``.

What differs from the reference, and why:

* A bank smaller than ``k = num_grasps * 5`` is searched whole.  The reference's ``topk`` raises there.
* An element with no unperformed action among its k nearest raises a ``RuntimeError`` that names the element and the step.  The
  reference builds a short action array and fails inside ``env.step``.
* Ties between equal distances go to the lower bank index.  ``topk`` promises no order.
* The checkpoint is ``os.path.join(checkpoint_dir, "actions.npy")``.  The reference's own name, ``checkpoint_dir + "actions.npy"``
  without a separator (``experiments/checkpoint/<exp_type>actions.npy``), is read as a fallback when the former does not exist.
* Pretrained banks resolve to ``<pretrained_root>/policies/NearestNeighbor/{t_p,t_g,v_t_p,v_t_g}.npy`` (``args.pretrained_root`` or
  ``PTEROTACTYL_PRETRAINED``) by the reference's ``(use_img, finger)`` rule; the reference reads them from inside its package.
* Actions outside ``[0, num_actions)`` are refused when they are appended or loaded, on the host.
* ``train`` resumes from ``spot`` as the reference does: batches before ``spot`` are skipped and batch ``spot`` itself is swept
  AGAIN, so a bank saved after batch ``spot`` holds that batch's entries twice after a resume.  Kept as it is.
* ``visualize`` raises ``NotImplementedError`` (pyrender; ``_core.refuse_visualize``).

The flags, the ``main``, the loaders and the validation rollout every policy engine has are ``policies/_core.py``'s.
"""
import os
import random

import numpy as np
import torch

from .... import ops
from ...utility import utils
from .. import _core

# Whether validate() looks the bank up with the library call when args does not say: on only if the call's p90 host wall lies
# below the reference loop's p10 on an MI355X (tools/nn_lookup_bench.py -> profiles/nn_lookup_ab.txt).
FUSED_LOOKUP_DEFAULT = True


class LatentBank:
    """The policy's memory: latents (M, D) float32 beside the action (M,) each was followed by, and ``spot``, the last training
    batch swept.  Host lists as the reference keeps them (``actions``: ints, ``latents``: 1-D tensors); ``to(device)`` makes the
    one upload ``lookup`` searches."""

    def __init__(self, num_actions):
        self.num_actions = int(num_actions)
        self.actions, self.latents, self.spot = [], [], 0
        self._device_copy = None

    def __len__(self):
        return len(self.actions)

    def _check_actions(self, actions, where):
        a = np.asarray(actions)
        if a.size and (not np.issubdtype(a.dtype, np.integer) and not np.array_equal(a, np.round(a))):
            raise ValueError(f"LatentBank: {where} holds actions that are not integers")
        if a.size and (a.min() < 0 or a.max() >= self.num_actions):
            raise ValueError(f"LatentBank: {where} holds actions outside [0, {self.num_actions}): min {a.min()}, max {a.max()}")
        return [int(v) for v in a.reshape(-1)]

    def append(self, latents, actions):
        """``latents`` (n, D) host floats and the n actions that followed them."""
        latents = torch.as_tensor(np.asarray(latents) if not isinstance(latents, torch.Tensor) else latents).detach().cpu().float()
        actions = self._check_actions(actions, "append")
        if latents.dim() != 2 or latents.shape[0] != len(actions):
            raise ValueError(f"LatentBank: {tuple(latents.shape)} latents for {len(actions)} actions")
        if self.latents and latents.shape[1] != self.latents[0].shape[0]:
            raise ValueError(f"LatentBank: latents of width {latents.shape[1]} in a bank of width {self.latents[0].shape[0]}")
        self.actions += actions
        self.latents += [row.clone() for row in latents]
        self._device_copy = None

    def save(self, path):
        """The reference's file (:216-220): ``np.save`` of ``{"actions": (M,) ints, "latents": (M, D) float32, "spot": int}``."""
        latents = torch.stack(self.latents).numpy() if self.latents else np.zeros((0, 0), dtype=np.float32)
        with open(path, "wb") as f:          # (a file object: np.save would append ".npy" to a name without it)
            np.save(f, {"actions": np.array(self.actions, dtype=np.int64), "latents": latents, "spot": self.spot})

    def load(self, path):
        """A file ``save`` or the reference wrote (:203-206)."""
        data = np.load(path, allow_pickle=True).item()
        actions = self._check_actions(data["actions"], path)
        latents = np.asarray(data["latents"], dtype=np.float32)
        if len(actions) and (latents.ndim != 2 or latents.shape[0] != len(actions)):
            raise ValueError(f"LatentBank: {path} holds {latents.shape} latents for {len(actions)} actions")
        self.actions = actions
        self.latents = [torch.from_numpy(row.copy()) for row in latents] if len(actions) else []
        self.spot = int(data["spot"])
        self._device_copy = None
        return self

    def to(self, device):
        """One upload: (latents (M, D) float32, actions (M,) int32) on ``device``, kept until the bank changes."""
        if not len(self):
            raise RuntimeError("a3vt: the latent bank is empty: train the policy or load a bank before looking it up")
        device = torch.device(device)
        cur = self._device_copy
        if cur is None or cur[0].shape[0] != len(self) or cur[0].device.type != device.type or \
                (device.index is not None and cur[0].device.index != device.index):
            self._device_copy = (torch.stack(self.latents).to(device).contiguous(),
                                 torch.tensor(self.actions, dtype=torch.int32).to(device))
        return self._device_copy

    def lookup(self, latents, mask, k, device=None):
        """Per element the action stored with the nearest of the ``k`` nearest banked latents whose action ``mask`` (E,
        num_actions; non-zero = performed) leaves open -> (E,) NumPy integers, -1 where none of the k qualifies.  One
        ``ops.latent_nearest`` on ``device`` (default: the GPU when there is one) and one copy of E integers to the host."""
        device = utils._device() if device is None else device
        bank, actions = self.to(device)
        mask = torch.as_tensor(mask, dtype=torch.float32)
        if mask.dim() != 2 or mask.shape[1] != self.num_actions:
            raise RuntimeError(f"a3vt: the mask is {tuple(mask.shape)}, the bank's actions are [0, {self.num_actions})")
        queries = torch.as_tensor(latents, dtype=torch.float32).to(device)
        _, _, action, _ = ops.latent_nearest(bank, actions, queries, mask.to(device), k)
        return action.cpu().numpy()


def reference_lookup(latents, actions, obs_latents, mask, k):
    """The reference's per-element loop (:115-137) on torch ops, on the device of ``latents`` (M, D): ``actions`` is the host
    list; ``mask`` (E, num_actions) stands for the reference's list of seen actions (rebuilt through the host per candidate there
    too).  Returns a list with one action per element that found one — shorter than E otherwise, as the reference's."""
    out = []
    k = min(k, latents.shape[0])
    for i in range(obs_latents.shape[0]):
        latent_distance = ((latents - obs_latents[i].to(latents.device)) ** 2).mean(dim=1)
        smallest_idxs = torch.topk(latent_distance, k, largest=False, sorted=True)[1]
        for idx in smallest_idxs:
            possible_action = actions[idx]
            seen_actions = list(np.where(mask[i].data.cpu().numpy() != 0)[0])
            if possible_action not in seen_actions:
                out.append(possible_action)
                break
    return out


class Engine(_core.EngineBase):
    def __init__(self, args, sampler=None, loaders=None):
        super().__init__(args, sampler, loaders)     # (device: where the bank is searched)
        self.bank = LatentBank(args.num_actions)
        self.steps_chosen = 0

    # the reference's attributes: the bank's host lists
    actions = property(lambda self: self.bank.actions)
    latents = property(lambda self: self.bank.latents)
    spot = property(lambda self: self.bank.spot, lambda self, v: setattr(self.bank, "spot", v))

    def __call__(self):
        _core.refuse_visualize(self.args)
        self.make_env()
        self.bank = LatentBank(self.args.num_actions)
        train_loaders, valid_loaders = self.get_loaders()
        self.results_dir = os.path.join("results", self.args.exp_type)
        os.makedirs(self.results_dir, exist_ok=True)
        self.checkpoint_dir = os.path.join("experiments/checkpoint/", self.args.exp_type)
        os.makedirs(self.checkpoint_dir, exist_ok=True)
        self.checkpoint = os.path.join(self.checkpoint_dir, "actions.npy")
        with torch.no_grad():
            self.load()
            if self.args.eval:
                return self.validate(valid_loaders)
            self.train(train_loaders)
            self.save()

    def train(self, dataloader):
        """The reference's sweep (:73-98): ``random.sample`` of 40 % of the batches after ``random.seed(args.seed)``; per batch
        ``budget`` greedy steps, each recording every element's pre-step latent beside its chosen action; a save when
        ``v % 3 == 0``.  Batches before ``spot`` are skipped; batch ``spot`` itself is swept again on a resume."""
        training_length = len(dataloader)
        random.seed(self.args.seed)
        training_instances = set(random.sample(range(training_length), int(training_length * 0.4)))
        for v, batch in enumerate(dataloader):
            if v < self.spot or v not in training_instances:
                continue
            self.spot = v
            obs = self.env.reset(batch)
            for _ in range(self.args.budget):
                action, next_obs, reward, all_done = self.env.best_step(greedy_checks=self.args.greedy_checks)
                E = self.args.env_batch_size
                self.bank.append(obs["latent"][:E], [action[i] for i in range(E)])
                obs = next_obs
            if v % 3 == 0:
                self.save()

    def choose(self, obs):
        """One step of the policy -> (E,) NumPy actions."""
        k = self.args.num_grasps * 5
        fused = getattr(self.args, "fused_lookup", None)
        if FUSED_LOOKUP_DEFAULT if fused is None else fused:
            action = self.bank.lookup(obs["latent"], obs["mask"], k, device=self.lookup_device())
            missing = np.where(action < 0)[0]
        else:
            latents, _ = self.bank.to(self.lookup_device())
            found = reference_lookup(latents, self.bank.actions, obs["latent"], obs["mask"], k)
            action = np.array(found)
            # (the walk appends nothing for an element without a choice: find which one by asking each alone)
            missing = [] if len(found) == obs["latent"].shape[0] else \
                [i for i in range(obs["latent"].shape[0])
                 if not reference_lookup(latents, self.bank.actions, obs["latent"][i:i + 1], obs["mask"][i:i + 1], k)]
        if len(missing):
            raise RuntimeError(f"a3vt: nearest-neighbour policy: element {int(missing[0])} at step {self.steps_chosen} has performed "
                               f"every action stored with its {min(k, len(self.bank))} nearest latents")
        return action

    def take_step(self, t, obs):
        action = self.choose(obs)
        obs, _, done = self.env.step(action)
        self.steps_chosen += 1
        return action, obs, done

    def validate(self, dataloader):
        _core.refuse_visualize(self.args)
        scores, actions, names = [], [], []
        self.bank.to(self.lookup_device())      # (an empty bank is refused here, before any episode)
        for batch in dataloader:
            names += batch["names"]
            obs = self.env.reset(batch)
            self.steps_chosen = 0
            cur_scores, cur_actions = self.play(obs, self.take_step)
            scores.append(cur_scores)
            actions.append(cur_actions)
            now = _core.summary(cur_scores)
            print(f"Valid || score: {now['score']:.4f}, reward = {now['reward']:.4f}")
        return self.report(scores, actions, names)

    def bank_location(self):
        """Where ``load`` reads the bank from: the pretrained file by the reference's ``(use_img, finger)`` rule (:180-202), else
        the checkpoint, else the reference's separator-less name of it; None when there is none."""
        if self.args.pretrained:
            return os.path.join(utils.pretrained_root(self.args), "policies", "NearestNeighbor", _core.kind(self.args) + ".npy")
        for path in (self.checkpoint, self.checkpoint_dir + "actions.npy"):
            if os.path.exists(path):
                return path
        return None

    def load(self):
        location = self.bank_location()
        if location is not None:
            self.bank.load(location)

    def save(self):
        self.bank.save(self.checkpoint)




def get_parser():
    """The reference's flags and defaults (:223-311) and this package's."""
    parser = _core.common_parser(auto_location=True, pretrained=True, greedy_checks=True)
    parser.add_argument("--eval", action="store_true", default=False, help="for evaluating on test set")
    parser.add_argument("--no_fused_lookup", dest="fused_lookup", action="store_false", default=None,
                        help="look the bank up with the reference's per-element loop on torch ops")
    return parser


def main(argv=None):
    return _core.run(Engine, get_parser(), argv, after_parse=_core.latent_only)


if __name__ == "__main__":
    main()
