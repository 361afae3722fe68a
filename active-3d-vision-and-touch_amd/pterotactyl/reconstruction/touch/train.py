"""Drop-in for ``pterotactyl/reconstruction/touch/train.py`` — the trainer ``Engine`` of the touch chart predictor.

Per batch: tactile images, finger frames and the points the sensor saw; the ``Encoder`` predicts a chart in the finger's frame
and the loss is ``loss_coeff * chamfer(chart surface samples, points).mean()`` on this package's HIP surface sampling and
Chamfer distance (``utils.chamfer_distance``).

Same constructor argument (an argparse ``Namespace`` or any object with the same attributes), same public methods and
attributes (``__call__``, ``get_loaders``, ``train``, ``validate``, ``save``, ``load``, ``check_values``; ``encoder, optimizer,
verts, faces, epoch, best_loss, current_loss, checkpoint_dir``), same data sets (``recon_train`` / ``valid`` / ``test``), same
files (``<ckpt>/model``, ``/optim``, ``config.json``), same flags and defaults (``get_parser``).

Differences, as in this package's other trainers: no host synchronisation inside a step; logging every
``args.log_interval`` steps; tensorboard is optional; early stop raises ``StopIteration`` where the reference calls ``exit()``;
the optimizer is the library's one-launch Adam; the chart template is the packaged ``assets/touch_chart.npz``; ``loaders=``
injects data (tests, synthetic benchmarks); pretrained weights are looked up under ``args.pretrained_root`` /
``$PTEROTACTYL_PRETRAINED``.  Training runs torch's convolutions (the fused stem of ``model.Encoder`` is forward-only and takes
over in ``validate``, under ``no_grad``, when the model's knob is on).
"""
import argparse
import os

import torch

from . import model
from ...utility import data_loaders, utils
from ...utility.utils import SummaryWriter
from .... import ops as _ops
from .... import optim as a3vt_optim


def pretrained_location(args):
    """Directory of the pretrained touch model (the reference: ``pretrained/reconstruction/touch/best/``)."""
    return os.path.join(utils.pretrained_root(args), "reconstruction", "touch", "best")


class Engine:
    def __init__(self, args, loaders=None):
        utils.set_seeds(args.seed)
        self.epoch = 0
        self.best_loss = 10000
        self.current_loss = None
        self.args = args
        self.last_improvement = 0
        self._loaders = loaders
        self.log_interval = getattr(args, "log_interval", 10)
        self.checkpoint_dir = os.path.join("experiments/checkpoint/", args.exp_type, args.exp_id)
        os.makedirs(self.checkpoint_dir, exist_ok=True)
        utils.save_config(self.checkpoint_dir, args)
        verts, faces = utils.load_mesh_touch("touch_chart")
        self.faces = faces.to(torch.int32).contiguous()
        self.verts = verts.view(1, verts.shape[0], 3).repeat(args.batch_size, 1, 1)

    def setup(self):
        """Model and optimizer (what ``__call__`` does before touching data)."""
        self.encoder = model.Encoder(fused_stem=getattr(self.args, "fused_stem", None)).to(self.verts.device)
        self.optimizer = a3vt_optim.make_adam(list(self.encoder.parameters()), self.args.lr,
                                              library=getattr(self.args, "library_adam", True))

    def __call__(self):
        self.setup()
        writer = SummaryWriter(os.path.join("experiments/tensorboard/", self.args.exp_type))
        train_loader, valid_loader = self.get_loaders()
        if self.args.eval:
            self.load()
            with torch.no_grad():
                self.validate(valid_loader, writer)
            return self.current_loss
        for epoch in range(self.args.epochs):
            self.epoch = epoch
            self.train(train_loader, writer)
            with torch.no_grad():
                self.validate(valid_loader, writer)
            self.check_values()
        return self.best_loss

    def get_loaders(self):
        if self._loaders is not None:
            return self._loaders
        from torch.utils.data import DataLoader
        workers = getattr(self.args, "num_workers", 16)
        train_loader = ""
        if not self.args.eval:
            train_data = data_loaders.mesh_loader_touch(self.args, set_type="recon_train")
            train_loader = DataLoader(train_data, batch_size=self.args.batch_size, shuffle=True, num_workers=workers,
                                      collate_fn=train_data.collate)
        valid_data = data_loaders.mesh_loader_touch(self.args, set_type="test" if self.args.eval else "valid")
        valid_loader = DataLoader(valid_data, batch_size=self.args.batch_size, shuffle=False, num_workers=workers,
                                  collate_fn=valid_data.collate)
        return train_loader, valid_loader

    def _loss(self, batch, samples=None):
        """``loss_coeff * chamfer.mean()`` of one loader-format batch, and the batch size."""
        dev = self.verts.device
        sim_touch = batch["sim_touch"].to(dev, non_blocking=True)
        gt_points = batch["samples"].to(dev, non_blocking=True)
        ref_frame = {k: v.to(dev, non_blocking=True) for k, v in batch["ref"].items()}
        batch_size = gt_points.shape[0]
        pred_verts = self.encoder(sim_touch, ref_frame, self.verts[:batch_size])
        cd = utils.chamfer_distance(pred_verts, self.faces, gt_points, num=self.args.num_samples, samples=samples)
        return self.args.loss_coeff * cd.mean(), batch_size

    def train_step(self, batch, samples=None):
        """One optimisation step; returns the (device) scalar loss.  No host sync."""
        self.optimizer.zero_grad(set_to_none=True)
        with model.repeatable_torch_kernels():      # (the backward's convolutions too: a seeded run repeats bit for bit)
            loss, _ = self._loss(batch, samples)
            loss.backward()
        self.optimizer.step()
        return loss.detach()

    def train(self, data, writer):
        total_loss = torch.zeros((), device=self.verts.device)
        iterations = 0
        self.encoder.train()
        for k, batch in enumerate(data):
            loss = self.train_step(batch)
            total_loss += loss
            iterations += 1
            if self.log_interval and k % self.log_interval == 0:
                print(f"Train || Epoch: {self.epoch},  loss: {loss.item():.5f} || best_loss:  {self.best_loss:.5f}")
        if iterations:
            writer.add_scalars("train", {self.args.exp_id: total_loss.item() / iterations}, self.epoch)

    def validate(self, valid_loader, writer):
        total_loss = torch.zeros((), device=self.verts.device)
        self.encoder.eval()
        num_examples = 0.0
        for batch in valid_loader:
            loss, batch_size = self._loss(batch)
            num_examples += float(batch_size)
            total_loss += loss.detach() * float(batch_size)          # (weighted by the batch size, as the reference)
        total = (total_loss / max(num_examples, 1.0)).item()
        print("*******************************************************")
        print(f"Total validation loss: {total}")
        print("*******************************************************")
        if not self.args.eval:
            writer.add_scalars("valid", {self.args.exp_id: total}, self.epoch)
        self.current_loss = total

    def save(self):
        torch.save(self.encoder.state_dict(), self.checkpoint_dir + "/model")
        torch.save(self.optimizer.state_dict(), self.checkpoint_dir + "/optim")

    def check_values(self):
        if self.best_loss >= self.current_loss:
            improvement = self.best_loss - self.current_loss
            self.best_loss = self.current_loss
            print(f"Saving Model with a {improvement} improvement in point loss")
            self.save()
            self.last_improvement = 0
        else:
            self.last_improvement += 1
            if self.last_improvement == self.args.patience:
                raise StopIteration(f"Over {self.args.patience} steps since last improvement")
        print("*******************************************************")

    def load(self):
        dev = self.verts.device
        if self.args.eval and getattr(self.args, "pretrained", False):
            location = os.path.join(pretrained_location(self.args), "model")
        else:
            location = self.checkpoint_dir + "/model"
        self.encoder.load_state_dict(torch.load(location, map_location=dev))
        _ops.invalidate_bf16_copies()


def get_parser():
    """The reference trainer's flags and defaults."""
    p = argparse.ArgumentParser()
    p.add_argument("--seed", type=int, default=0, help="seed of the random generators")
    p.add_argument("--limit_data", action="store_true", default=False, help="train on a small part of the data (debugging)")
    p.add_argument("--epochs", type=int, default=1000, help="how many epochs to train")
    p.add_argument("--lr", type=float, default=0.0001, help="learning rate of Adam")
    p.add_argument("--eval", action="store_true", default=False, help="no training: score a saved model on the test set")
    p.add_argument("--batch_size", type=int, default=64, help="touches per batch")
    p.add_argument("--num_samples", type=int, default=4000, help="points sampled from each predicted chart for the loss")
    p.add_argument("--patience", type=int, default=70, help="stop after this many epochs without a better validation loss")
    p.add_argument("--loss_coeff", type=float, default=9000.0, help="factor on the Chamfer distance")
    p.add_argument("--exp_id", type=str, default="test", help="name of this run (checkpoint sub-directory)")
    p.add_argument("--exp_type", type=str, default="test", help="group of runs (checkpoint directory)")
    p.add_argument("--pretrained", action="store_true", default=False, help="with --eval: score the downloaded pretrained weights")
    # this package's knobs
    p.add_argument("--data_root", type=str, default=None, help="dataset directory (default: $PTEROTACTYL_DATA)")
    p.add_argument("--fused_stem", dest="fused_stem", action="store_true", default=model.FUSED_STEM_DEFAULT,
                   help="run the stem's convolutions on the fp32 direct-convolution kernels in validation")
    p.add_argument("--no_fused_stem", dest="fused_stem", action="store_false")
    return p


if __name__ == "__main__":
    Engine(get_parser().parse_args())()
