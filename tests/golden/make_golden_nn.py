#!/usr/bin/env python
"""Generate ``g19_nearest_neighbor.npz`` by running the REAL reference's nearest-neighbour ``Engine``
(``policies/NearestNeighbor/train.py``) on the CPU (``python tests/golden/make_golden_nn.py``, build container only; see
``make_golden_env.py``, whose recipe this follows: ``oracle.ref_shim``, stubbed simulator modules, ``get_loaders`` a no-op,
seeded models written to temporary checkpoint directories, the injected-sample Chamfer distance).

The models, settings and surface draws are ``env_util``'s case "b" (four fingers, latent, E = 2, 6 actions, budget 3,
greedy_checks 3); batches, sensor records and the bank are ``nn_policy_util``'s.  The reference's ``Engine.train`` and
``Engine.validate`` are driven directly, with lists as loaders, in a temporary working directory.

  train     three batches, of which ``int(3 * 0.4) = 1`` is swept: the resulting ``actions``, ``latents`` and ``spot``
  validate  a bank of 40 entries (``nn_policy_util.validate_bank`` and ``placed_near``) loaded through the reference's ``load`` from a
            file written here, two batches, a full episode each: per step the chosen actions, scores and latents

Stored (weights and images are NOT stored: the tests rebuild them from the seeds and check the checksums):
  sha:<kind>                     checksum of the touch (non-BatchNorm tensors) / vision / auto state dict
  bn:<key>                       every BatchNorm tensor of the touch encoder
  face_idx|u|v                   injected surface draws (3, E, 700)
  train:actions|latents|spot     the bank ``train`` built
  bank:actions|latents           the validate case's bank
  valid:<b>:<i>:score|latent|mask   the observation after call i of batch b (0 = reset);  valid:<b>:<i>:actions for i >= 1
Asserted here, the smallest value printed: at every lookup the relative gap between consecutive fp64 distances among the 26
nearest exceeds 1e-2 (one hundred times the tests' 1e-4 latent tolerance), and at least one lookup's nearest entry carries an
action that was already taken, so the skip is exercised."""
import importlib
import os
import random
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import save  # noqa: E402  (installs the import shim)
from make_golden_env import reference_setup  # noqa: E402
import env_util as eu  # noqa: E402
import nn_policy_util as nu  # noqa: E402


def main():
    c = eu.CASES[nu.CASE]
    k = 5 * 5
    with reference_setup(nu.CASE, records=nu.records()) as setup:
        env_mod, out = setup.env_mod, setup.out
        nn_mod = importlib.import_module("pterotactyl.policies.NearestNeighbor.train")
        with setup.workdir() as (root, locations):
            # ---- train ------------------------------------------------------------------------------------------------------
            engine = nn_mod.Engine(nu.engine_args(False, **locations))
            engine.env = env_mod.ActiveTouch(engine.args)
            engine.spot, engine.actions, engine.latents = 0, [], []
            engine.checkpoint = os.path.join(root, "train_actions.npy")
            with torch.no_grad():
                engine.train(nu.batches("train"))
                engine.save()
            data = np.load(engine.checkpoint, allow_pickle=True).item()
            out["train:actions"], out["train:latents"] = np.asarray(data["actions"]).astype(np.int64), data["latents"]
            out["train:spot"] = np.int64(data["spot"])
            print(f"train: spot {data['spot']}, actions {list(data['actions'])}")
            assert len(data["actions"]) == eu.E * c["budget"]
            # ---- validate ---------------------------------------------------------------------------------------------------
            first = data["latents"][0]                        # the latent of a mesh without touches: every episode starts there

            def validate(bank_latents, bank_actions, name):
                """The reference's ``load`` + ``validate`` on this bank -> [(batch, call, obs, actions)]."""
                engine = nn_mod.Engine(nu.engine_args(True, **locations))
                engine.env = env_mod.ActiveTouch(engine.args)
                engine.spot, engine.actions, engine.latents = 0, [], []
                engine.checkpoint = os.path.join(root, name)
                np.save(engine.checkpoint, {"actions": bank_actions, "latents": bank_latents, "spot": 0})
                engine.load()
                assert len(engine.actions) == len(bank_actions)
                log, state = [], {"b": -1, "i": 0}
                reset, step = engine.env.reset, engine.env.step

                def logged_reset(batch):
                    obs = reset(batch)
                    state["b"], state["i"] = state["b"] + 1, 0
                    log.append((state["b"], 0, obs, None))
                    return obs

                def logged_step(action):
                    res = step(action)
                    state["i"] += 1
                    log.append((state["b"], state["i"], res[0], np.asarray(action).astype(np.int64)))
                    return res

                engine.env.reset, engine.env.step = logged_reset, logged_step
                random.seed(0)
                with torch.no_grad():
                    engine.validate(nu.batches("valid"))
                return log

            # a first pass on the first 38 entries tells where the two elements of batch 0 are after their first step (action 0
            # for everyone: the 38th entry); the last two entries sit next to those latents, one each, with actions 1 and 2: each
            # element finds its own first, so the elements part ways there
            seeded_latents, seeded_actions = nu.validate_bank(first)
            probe = validate(seeded_latents, seeded_actions, "probe.npy")
            assert (probe[1][0], probe[1][1]) == (0, 1) and list(probe[1][3]) == [0, 0]
            placed = np.stack([nu.placed_near(probe[1][2]["latent"][e].numpy(), nu.BANK_SEED + 1 + e) for e in range(eu.E)])
            bank_latents = np.concatenate([seeded_latents, placed])
            bank_actions = np.concatenate([seeded_actions, [1, 2]]).astype(np.int64)
            assert len(bank_actions) == nu.BANK_ROWS
            out["bank:latents"], out["bank:actions"] = bank_latents, bank_actions
            log = validate(bank_latents, bank_actions, "bank.npy")
    smallest, skipped = np.inf, 0
    for n, (b, i, obs, actions) in enumerate(log):
        key = f"valid:{b}:{i}:"
        out[key + "score"], out[key + "latent"], out[key + "mask"] = obs["score"].numpy(), obs["latent"].numpy(), obs["mask"].numpy()
        if actions is not None:
            out[key + "actions"] = actions
        if i < c["budget"]:                                   # a lookup follows this observation
            chosen = log[n + 1][3]
            for e in range(eu.E):
                d = nu.distances64(bank_latents, obs["latent"][e].numpy())
                order = np.argsort(d, kind="stable")
                smallest = min(smallest, nu.smallest_gap(d[order], k + 1))
                seen = list(np.where(obs["mask"][e].numpy() != 0)[0])
                skipped += int(bank_actions[order[0]] in seen)
                assert nu.reference_walk(bank_latents, bank_actions, obs["latent"][e].numpy(), seen, k) == chosen[e]
        print(f"validate batch {b} call {i}: score {obs['score'].tolist()} actions {None if actions is None else list(actions)}")
    print(f"validate: smallest relative gap between consecutive distances among the {k + 1} nearest {smallest:.3e}; "
          f"{skipped} lookups whose nearest entry's action was already taken")
    assert smallest > nu.MIN_GAP, f"distance gap {smallest:.3e} <= {nu.MIN_GAP}: choose another nn_policy_util.BANK_SEED"
    assert skipped >= 1, "no lookup skips a taken action: choose another nn_policy_util.BANK_SEED"
    assert any(a is not None and a[0] != a[1] for _, _, _, a in log), "the two elements of a batch never choose differently"
    save(nu.FIXTURE, **out)


if __name__ == "__main__":
    main()
