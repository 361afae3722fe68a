#!/usr/bin/env python
"""Generate ``g17_touch_encoder.npz`` by running the REAL reference's touch chart predictor on the CPU
(``python tests/golden/make_golden_touch.py``, build container only; see ``make_golden.py`` and ``oracle.ref_shim``).

The reference ``Encoder`` is built under ``torch.manual_seed(0)``; its BatchNorm layers get seeded affine parameters and the
running statistics of a seeded calibration batch (``tests/touch_util.py::seed_batchnorm`` — with untouched running statistics
the activations collapse layer by layer and a fault in a deep convolution would not reach the output).  Stored:
  state_sha256, keys          checksum of the convolution / linear tensors (11 MB, re-derived from the seed by the tests) and the
                              state dict's key list with shapes (JSON)
  bn:<key>                    every BatchNorm tensor
  img, rot, pos, template     B = 2 inputs (images uint8)
  eval32:* / eval64:*         eval mode, the module in fp32 and the same module in fp64: ``stem`` = block 3's output (2,32,16,16),
                              ``out`` = forward (2,25,3);  e_stem / e_out = max |fp32 - fp64| of the two
  train32:* / train64:*       train mode (batch statistics): ``pred`` = predict_verts, ``g:<name>`` = gradient of L = sum(pred * R)
                              for the tensors of ``touch_util.GRAD_NAMES``;  R stored"""
import copy
import importlib
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import ref, save, state_checksum  # noqa: E402  (installs the import shim; defines no fixture when imported)
import touch_util as tu  # noqa: E402


def main():
    tm = importlib.import_module("pterotactyl.reconstruction.touch.model")
    torch.manual_seed(0)
    net = tm.Encoder()
    out = {"state_sha256": state_checksum(tu.non_bn_state(net.state_dict()))}
    tu.seed_batchnorm(net)
    sd = net.state_dict()
    out["keys"] = np.array(tu.key_list(sd))
    for k, v in sd.items():
        if tu.is_bn_key(k):
            out["bn:" + k] = v.numpy().copy()
    img = tu.images(2, 3)
    rot, pos = tu.frames(2, 4)
    template, _ = ref.utils.load_mesh_touch(os.path.join(ref.objects_dir, "touch_chart.obj"))
    template = template.float().cpu()
    out.update(img=img.numpy(), rot=rot.numpy(), pos=pos.numpy(), template=template.numpy())
    R = torch.randn(2, 75, generator=torch.Generator().manual_seed(5))
    out["R"] = R.numpy()
    for tag, dt in (("32", torch.float32), ("64", torch.float64)):
        m = copy.deepcopy(net).to(dt).eval()
        x = img.to(dt) / 255.0
        with torch.no_grad():
            stem = x
            for block in list(m.CNN_layers)[:3]:
                stem = block(stem)
            verts = template.to(dt).unsqueeze(0).repeat(2, 1, 1)
            y = m(x, {"rot": rot.to(dt), "pos": pos.to(dt)}, verts)
        out[f"eval{tag}:stem"], out[f"eval{tag}:out"] = stem.numpy(), y.numpy()
        m.train()
        pred = m.predict_verts(x)
        (pred * R.to(dt)).sum().backward()
        out[f"train{tag}:pred"] = pred.detach().numpy()
        params = dict(m.named_parameters())
        for k in tu.GRAD_NAMES:
            out[f"train{tag}:g:{k}"] = params[k].grad.numpy()
    out["e_stem"] = np.float64(np.abs(out["eval32:stem"].astype(np.float64) - out["eval64:stem"]).max())
    out["e_out"] = np.float64(np.abs(out["eval32:out"].astype(np.float64) - out["eval64:out"]).max())
    print(f"e_stem {out['e_stem']:.3e} (max |stem| {np.abs(out['eval64:stem']).max():.3f}, share > 0: {(out['eval64:stem'] > 0).mean():.2f})  "
          f"e_out {out['e_out']:.3e} (max |out| {np.abs(out['eval64:out']).max():.3f}, "
          f"max |pred| {np.abs(out['eval64:out'] - (np.einsum('bij,vj->bvi', out['rot'], out['template']) + out['pos'][:, None])).max():.3e})")
    save(tu.FIXTURE, **out)


if __name__ == "__main__":
    main()
