#!/usr/bin/env python
"""One swept batch of the dataset-specific policies LEBA and MFBA after the candidates have been scored — ``fused_tally`` on against
off, the two forms ALTERNATING in one process (``tools/ab_protocol.py``, host wall only), at two sizes: the reference's
defaults (K = 50 candidates, E = 3 elements, A = 50 actions) and a large batch (K = 50, E = 64, A = 50).

The environment is synthetic: ``score_candidates`` answers with a (K, E) table that one small device op has just written (as the
batched candidate step leaves it: on the device, the stream busy until it is there), copied to the host unless ``to_host=False``.
What is timed is therefore what the knob changes — where the table goes and who walks it — not the scoring, which is the same in
both forms and a thousand times longer.

1. swept batch   ``Engine.tally_fused`` against ``Engine.tally_loop``, candidates included (LEBA's list, MFBA's
                 ``candidate_actions``), for both engines:
                   fused: the table stays on the device; one ``ops.candidate_tally`` (``a3vt_candidate_tally``, one launch);
                          MFBA copies E int32 to the host;
                   loop:  the table is copied to the host; the reference's Python loop over the K * E pairs (LEBA) or
                          ``choose_actions`` and E votes (MFBA).
2. tally alone   from a table already on the device: the copy plus LEBA's loop, against one ``ops.candidate_tally`` (the candidate
                 table's upload and the launch).

Every timed call ends with a device synchronise in BOTH forms, so the host wall clock holds all of a call's work (the fused LEBA
batch itself needs none until ``save()``: its figure is an upper bound).  Median / p10 / p90 over ``--calls`` calls per round,
``--rounds`` rounds in turn after ``--warmup`` calls of each.  The verdict applies the project's rule for a knob's default:
``FUSED_TALLY_DEFAULT`` is on only if the fused batch's p90 lies below the loop's p10 at BOTH sizes.

    python tools/tally_bench.py --out profiles/candidate_tally_ab.txt"""
import argparse
import json
import os
import sys
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import ab_protocol as ab  # noqa: E402  (tools/ is this script's directory)

ap = argparse.ArgumentParser()
ab.add_arguments(ap, calls=100, rounds=5, warmup=20)
ap.add_argument("--sizes", type=str, default="50x3x50,50x64x50", help="K x E x A, comma-separated (K = A: a full search)")
a = ab.parse(ap)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from a3vt_amd import ops  # noqa: E402
from a3vt_amd.pterotactyl.policies import environment  # noqa: E402
from a3vt_amd.pterotactyl.policies.dataset_specific import LEBA, MFBA  # noqa: E402

ab.require_gpu("tally_bench")
dev = torch.device("cuda", 0)


def alternate(forms):
    """The host wall alone, stopped after the closing synchronise: the forms do not end on the host."""
    return ab.alternate(forms, a.calls, a.rounds, a.warmup, clocks=("host",), host_stops="after")


class SyntheticEnv:
    """What the engines read of ``ActiveTouch`` after a ``reset``: the device, ``current_data`` and a scored table."""

    def __init__(self, args):
        g = torch.Generator().manual_seed(0)
        self.args, self.device = args, dev
        E = args.env_batch_size
        self.table = (0.5 + 2.5 * torch.rand(args.num_actions, E, generator=g)).to(dev)
        self.current_data = {"first_score": 3.0 + torch.rand(E, generator=g), "mask": torch.zeros(E, args.num_actions)}

    def score_candidates(self, candidates, to_host=True):
        scores = self.table[:len(candidates)] * 1.0            # (one device op: the table is written on the stream)
        return scores.cpu() if to_host else scores

    def greedy_choice(self, greedy_checks=None):
        candidates, full = environment.candidate_actions(self.current_data["mask"], self.args.num_actions, greedy_checks)
        scores = self.score_candidates(candidates)
        return environment.choose_actions(scores, candidates, self.current_data["mask"], full), scores


def engine_of(module, K, E, A, fused):
    args = SimpleNamespace(num_actions=A, env_batch_size=E, greedy_checks=K, seed=0, fused_tally=fused)
    engine = module.Engine(args)
    engine.env = SyntheticEnv(args)
    engine.chosen_actions = []
    engine.reset_state()
    return engine


def host_only(res):
    """The result as the JSON line has always held it: {form: stats of the host wall}."""
    return {form: r["host"] for form, r in res.items()}


def report(title, res, lines):
    return ab.report(title, res, "fused", "loop", lines, clock="host", width=6)


lines = ["# profiles/candidate_tally_ab.txt: `python tools/tally_bench.py --out profiles/candidate_tally_ab.txt`, one MI355X (the device "
         "reports itself by the name below).",
         f"# one swept batch of LEBA / MFBA after scoring, fused_tally on vs off; host wall in ms per batch, every call ending "
         f"with a device synchronise; {torch.cuda.get_device_name(0)}",
         f"# {a.calls * a.rounds} calls per form in {a.rounds} alternating rounds after {a.warmup} warm-up calls"]
result = {"device": torch.cuda.get_device_name(0), "calls": a.calls * a.rounds, "warmup": a.warmup, "sizes": {}}
verdict = {"LEBA": True, "MFBA": True}
for size in a.sizes.split(","):
    K, E, A = (int(v) for v in size.split("x"))
    entry = result["sizes"][size] = {}
    for name, module in (("LEBA", LEBA), ("MFBA", MFBA)):
        on, off = engine_of(module, K, E, A, True), engine_of(module, K, E, A, False)
        on.tally_fused()
        off.tally_loop()
        for attr in module.Engine.state_names:                   # the two forms must agree bit for bit before they are timed
            if not np.array_equal(getattr(on, attr), getattr(off, attr)):
                raise SystemExit(f"tally_bench: {name} {attr} differs between the forms at {size}")
        res = alternate({"fused": on.tally_fused, "loop": off.tally_loop})
        entry[name] = host_only(res)
        verdict[name] &= report(f"{name} swept batch, K = {K}, E = {E}, A = {A}", res, lines)
    # the tally alone, from a table on the device
    env = SyntheticEnv(SimpleNamespace(num_actions=A, env_batch_size=E))
    table = env.table[:K].contiguous()
    candidates = [[k] * E for k in range(K)]
    cand_host = torch.tensor(candidates, dtype=torch.int32)    # (on the host, as the engines build it: checked there, uploaded)
    first_host, first_dev = env.current_data["first_score"], env.current_data["first_score"].to(dev)
    sums_dev, checks_dev = torch.full((A,), 1e10, dtype=torch.float64, device=dev), torch.ones(A, dtype=torch.float64, device=dev)
    sums, checks = np.full(A, 1e10), np.ones(A)

    def launch():
        ops.candidate_tally(table, cand_host, first_dev, None, sums=sums_dev, checks=checks_dev)

    def copy_and_loop():
        host = table.cpu()
        for k, actions in enumerate(candidates):
            for action, score in zip(actions, host[k] / first_host):
                if sums[action] == 1e10:
                    sums[action] = score
                else:
                    sums[action] += score
                checks[action] += 1.0

    res = alternate({"fused": launch, "loop": copy_and_loop})
    entry["tally_alone"] = host_only(res)
    report(f"the tally alone (fused: ops.candidate_tally; loop: the table's copy and LEBA's loop), K = {K}, E = {E}, A = {A}", res, lines)
result["fused_tally_default"] = verdict
lines.append(json.dumps(result))
lines.append("# fused p90 below loop p10 at every size -> " +
             ", ".join(f"{name}.FUSED_TALLY_DEFAULT = {wins}" for name, wins in verdict.items()))
ab.emit(lines, a.out)
