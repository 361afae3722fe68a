"""``pterotactyl.policies.replay``: the learner's ring buffer of transitions (reference ``policies/replay.py``).

Same attributes, ``push`` / ``sample`` / ``save`` / ``load`` and file format as the reference, so buffers interchange in both
directions.  New (no reference counterpart): ``device``.  With ``device=None`` the buffers live on the host as in the reference;
with a device they live there and ``sample()`` is an index-select on that device — the meshes of a batch (the largest buffers, 2 x
mem_capacity x N x 4 floats) are never copied from the host per update."""
import os

import numpy as np
import torch

from ..utility import utils

BASE_MESH_SIZE = 1824     # vertices of the vision charts
BASE_CHART_SIZE = 25      # vertices of one touch chart

_PER_SAMPLE = ("mask", "mask_n", "actions", "rewards", "score", "score_n", "first_score")
_RECON = ("mesh", "mesh_n")
_LATENT = ("latent", "latent_n", "first_latent")


class ReplayMemory:
    def __init__(self, args, device=None):
        self.args = args
        self.device = None if device is None else torch.device(device)
        cap = args.mem_capacity
        new = lambda *shape: torch.zeros(shape, device=self.device)  # noqa: E731
        self.mask, self.mask_n = new(cap, args.num_actions), new(cap, args.num_actions)
        self.actions, self.rewards = new(cap), new(cap)
        self.score, self.score_n, self.first_score = new(cap), new(cap), new(cap)
        if args.use_recon:
            n_vert = BASE_MESH_SIZE + BASE_CHART_SIZE * args.num_grasps * (1 if args.finger else 4)
            self.mesh, self.mesh_n = new(cap, n_vert, 4), new(cap, n_vert, 4)
        if args.use_latent:
            size = utils.load_model_config(args.auto_location)[0].encoding_size
            self.latent, self.latent_n, self.first_latent = new(cap, size), new(cap, size), new(cap, size)
        self.position = 0
        self.count_seen = 0

    def _names(self, with_score_n=True):
        names = [n for n in _PER_SAMPLE if with_score_n or n != "score_n"]
        return names + (list(_RECON) if self.args.use_recon else []) + (list(_LATENT) if self.args.use_latent else [])

    def push(self, action, observation, next_observation, reward):
        """Append len(action) transitions at the write position, wrapping at ``mem_capacity``."""
        for i in range(len(action)):
            at = self.position
            self.actions[at] = _item(action[i])
            self.rewards[at] = _item(reward[i])
            self.score[at] = _item(observation["score"][i])
            self.score_n[at] = _item(next_observation["score"][i])
            self.first_score[at] = _item(observation["first_score"][i])
            self.mask[at] = torch.as_tensor(observation["mask"][i])
            self.mask_n[at] = torch.as_tensor(next_observation["mask"][i])
            if self.args.use_recon:
                self.mesh[at] = torch.as_tensor(observation["mesh"][i])
                self.mesh_n[at] = torch.as_tensor(next_observation["mesh"][i])
            if self.args.use_latent:
                self.latent[at] = torch.as_tensor(observation["latent"][i])
                self.latent_n[at] = torch.as_tensor(next_observation["latent"][i])
                self.first_latent[at] = torch.as_tensor(observation["first_latent"][i])
            self.count_seen += 1
            self.position = (self.position + 1) % self.args.mem_capacity

    def sample(self):
        """``train_batch_size`` transitions drawn with replacement by ``np.random.choice`` (the reference's draw: a seeded
        ``np.random`` picks the reference's indices), or None before ``burn_in`` / a full batch has been seen."""
        if self.count_seen < self.args.burn_in or self.count_seen < self.args.train_batch_size:
            return None
        indices = np.random.choice(min(self.count_seen, self.args.mem_capacity), self.args.train_batch_size)
        self.last_indices = indices
        idx = torch.as_tensor(indices, dtype=torch.long, device=self.mask.device)
        return {n: getattr(self, n).index_select(0, idx) for n in self._names()}

    def save(self, directory):
        """The reference's file: its key set (no ``score_n``), CPU tensors, written to a temporary name and renamed."""
        data = {n: getattr(self, n).cpu() for n in self._names(with_score_n=False)}
        data["position"], data["count_seen"] = self.position, self.count_seen
        order = ["mask", "mask_n", "actions", "rewards", "score", "first_score", "position", "count_seen"]
        data = {k: data[k] for k in order + [k for k in data if k not in order]}
        torch.save(data, directory + "_replay_buffer_temp.pt")
        os.rename(directory + "_replay_buffer_temp.pt", directory + "_replay_buffer.pt")

    def load(self, directory):
        data = torch.load(directory + "_replay_buffer.pt")
        for n in self._names(with_score_n=False):
            setattr(self, n, data[n].to(self.device if self.device is not None else "cpu"))
        self.position, self.count_seen = data["position"], data["count_seen"]


def _item(x):
    return float(x)
