#!/usr/bin/env python
"""The FoldingNet decoder of the auto-encoder, forward + backward: the fused fold kernels (csrc/fold.hip, ``fused_decoder``) against
the torch formulation (knob off), ALTERNATING the two in one process, at B = 16 and B = 32: after warm-up, device events around
windows of at least half a second each.  Prints time per call, the TFLOP/s the fused path achieves over the 6-product FLOP count
(6 x 2 x 512 x 512 x 6400 B: what a decoder step needs when nothing is computed twice; the kernels do 8), and the peak of the
allocator over one call of each.  ``--step`` instead times ``Engine.train_step`` of the auto-encoder trainer with the knob on and off
at the reference's defaults (B = 16, 20 x 300 encoder, 30 000 points, synthetic batches, a randomly initialised frozen model).
Run on the GPU box:  python tools/fold_bench.py [--step] [--rounds 3]"""
import argparse
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--step", action="store_true", help="time Engine.train_step instead of the decoder alone")
ap.add_argument("--batches", default="16,32")
ap.add_argument("--rounds", type=int, default=3, help="alternations fused / torch per batch size")
ap.add_argument("--window", type=float, default=0.5, help="seconds per timed window")
a = ap.parse_args()
from a3vt_amd import ops  # noqa: E402
from a3vt_amd.pterotactyl.reconstruction.autoencoder import model as am  # noqa: E402

dev = torch.device("cuda", 0)


def window(fn, seconds):
    """ms per call over a window of at least ``seconds`` (device events; the call count comes from a short probe)."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(3):
        fn()
    e1.record()
    torch.cuda.synchronize()
    n = max(3, int(seconds * 1e3 / max(e0.elapsed_time(e1) / 3, 1e-3)) + 1)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n, n


def peak_of(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - before) / 1e6


def alternate(name, fns, flop=None):
    """fns: {"fused": f, "torch": g}; warm both, then ``rounds`` times one window of each, in turn."""
    for fn in fns.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in fns}
    for _ in range(a.rounds):
        for k, fn in fns.items():
            ms, n = window(fn, a.window)
            times[k].append(ms)
    for k in list(ops._WORKSPACES):
        if k[0] == "fold":
            del ops._WORKSPACES[k]
    peaks = {k: peak_of(fn) for k, fn in fns.items()}
    best = {k: min(v) for k, v in times.items()}
    for k in fns:
        rate = f"  {flop / best[k] / 1e9:6.1f} TFLOP/s over the 6-product count" if flop and k == "fused" else ""
        print(f"{name} {k:5s}: {best[k]:8.3f} ms per call (windows: {', '.join(f'{t:.3f}' for t in times[k])}){rate}   peak {peaks[k]:8.1f} MB")
    print(f"{name} fused / torch = {best['fused'] / best['torch']:.3f}")


def decoder_ab(batch):
    torch.manual_seed(0)
    decs = {"fused": am.FoldingNetDec(fused=True).to(dev), "torch": am.FoldingNetDec(fused=False).to(dev)}
    decs["torch"].load_state_dict(decs["fused"].state_dict())
    code = torch.randn(batch, 512, device=dev).requires_grad_(True)
    dy = torch.randn(batch, 3, 6400, device=dev)

    def run(dec):
        def fn():
            dec.zero_grad(set_to_none=True)
            code.grad = None
            dec(code).backward(dy)
        return fn

    alternate(f"decoder fwd+bwd B={batch}", {k: run(d) for k, d in decs.items()}, flop=6 * 2 * 512 * 512 * 6400 * batch)


def step_ab(batch):
    from a3vt_amd.pterotactyl.reconstruction.autoencoder import train
    from a3vt_amd.pterotactyl.reconstruction.vision import model as vm
    from a3vt_amd.pterotactyl.utility import utils
    from a3vt_amd.synthetic import SyntheticLoader, make_args
    os.chdir(tempfile.mkdtemp(prefix="fold_bench_"))
    fns = {}
    for name, fused in (("fused", True), ("torch", False)):
        args = make_args(use_touch=True, finger=True, num_grasps=5, num_GCN_layers=20, hidden_GCN_size=300, number_points=30000,
                         encoding_size=200, exp_type="bench", exp_id=name, eval=False, epochs=1, patience=70, batch_size=batch,
                         log_interval=0, fused_decoder=fused)
        info, verts = utils.load_mesh_vision(args, "vision_charts")
        torch.manual_seed(7)
        deform = vm.Deformation(info, verts, args).to(dev)
        eng = train.Engine(args, loaders=(None, None), deform=deform)
        eng.setup()
        b = next(iter(SyntheticLoader(args, 1, batch, seed=1)))
        with torch.no_grad():
            charts = vm.prepare_mesh(b, eng.initial_mesh, args)
        img = b["img"].to(dev)
        fns[name] = (lambda e=eng, i=img, c=charts: e.train_step(i, c))
    alternate(f"Engine.train_step B={batch}", fns)


for B in (int(x) for x in a.batches.split(",")):
    (step_ab if a.step else decoder_ab)(B)
