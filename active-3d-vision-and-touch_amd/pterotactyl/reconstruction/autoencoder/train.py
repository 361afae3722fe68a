"""Drop-in for ``pterotactyl/reconstruction/autoencoder/train.py`` — the auto-encoder trainer ``Engine``.

The auto-encoder learns a latent of the meshes a frozen, already trained ``Deformation`` predicts: per batch the frozen
model runs under ``no_grad``, the auto-encoder encodes its vertices and folds an 80 x 80 lattice back into a point cloud, and
the loss is ``loss_coeff * chamfer(mesh, cloud).mean()`` with the gradient on the cloud (reference :140-151).  The latent is
what the policies observe (``policies/environment.py`` loads this model with ``only_encode=True``).

Same constructor argument (an argparse ``Namespace`` or any object with the same attributes), same public methods and
attributes (``__call__``, ``get_loaders``, ``train``, ``validate``, ``save``, ``load``, ``check_values``, ``cluster``;
``deform, auto_encoder, optimizer, mesh_info, initial_mesh, n_vision_charts, epoch, best_loss, current_loss, train_loss,
checkpoint_dir, results_dir``), same data sets (``auto_train`` / ``valid`` / ``test``), same checkpoint files
(``<ckpt>/model``, ``/optim``), same flags and defaults (``get_parser``).

Differences, as in this package's ``vision/train.py``: no host synchronisation inside a step (the reference calls
``loss.item()`` every step); logging every ``args.log_interval`` steps; tensorboard and PIL are optional; early stop raises
``StopIteration`` instead of ``exit()``; the optimizer step is the library's one-launch Adam (``args.library_adam``);
``loaders=`` and ``deform=`` inject data and the frozen model (tests, synthetic benchmarks).  ``args.fused_decoder`` (this
package's knob) runs the FoldingNet decoder on the fused fold kernels (``ops.fold``); the trainer's default for it is
``FUSED_DECODER_DEFAULT`` below.  Single process: data-parallel training of the auto-encoder is not implemented.
"""
import argparse
import os
import random
from types import SimpleNamespace

import numpy as np
import torch

from . import model
from ..vision import model as vision_model
from ..vision.train import pretrained_location as vision_pretrained_location
from ...utility import data_loaders, utils
from ...utility.utils import SummaryWriter
from .... import ops as _ops
from .... import optim as a3vt_optim

# Whether the trainer turns the fused decoder on when ``args`` does not say.  On: measured on an MI355X, forward + backward of
# the fused decoder takes 0.62 (B = 16) / 0.57 (B = 32) of the time of the torch formulation, against a bar of 0.75
# (profiles/fold_decoder_ab.txt).  The model's own default (``AutoEncoder`` without the knob) stays off.
FUSED_DECODER_DEFAULT = True


def pretrained_location(args):
    """Directory of the pretrained auto-encoder for ``args``: the rule of ``vision/train.py::pretrained_location`` (the
    sub-directory is picked by ``(use_img, finger)``) under ``<root>/reconstruction/auto/`` (reference :221-259).
    ``args.auto_pretrained_location`` overrides it."""
    explicit = getattr(args, "auto_pretrained_location", None)
    if explicit:
        return explicit
    vision = vision_pretrained_location(SimpleNamespace(use_img=args.use_img, finger=args.finger,
                                                        pretrained_root=getattr(args, "pretrained_root", None)))
    head, sub = os.path.split(vision.rstrip(os.sep))
    return os.path.join(os.path.dirname(head), "auto", sub) + os.sep


def _with_knob(args):
    """``args`` as the model reads it: ``fused_decoder`` filled in with the trainer's default when the caller left it out."""
    if not hasattr(args, "fused_decoder"):
        try:
            args.fused_decoder = FUSED_DECODER_DEFAULT
        except AttributeError:     # an immutable record (a loaded config): a copy with the knob
            args = SimpleNamespace(**args._asdict(), fused_decoder=FUSED_DECODER_DEFAULT)
    return args


class Engine:
    def __init__(self, args, loaders=None, template="vision_charts", deform=None):
        np.random.seed(args.seed)
        torch.manual_seed(args.seed)
        self.epoch = 0
        self.best_loss = 10000
        self.args = _with_knob(args)
        self.last_improvement = 0
        self.train_loss = 0
        self.vision_chart_location = template
        self._loaders = loaders
        self._deform = deform
        self.log_interval = getattr(args, "log_interval", 10)
        self.checkpoint_dir = os.path.join("experiments/checkpoint/", args.exp_type, args.exp_id)
        os.makedirs(self.checkpoint_dir, exist_ok=True)
        self.results_dir = os.path.join("results", args.exp_type, args.exp_id)
        os.makedirs(self.results_dir, exist_ok=True)
        if deform is None:
            self._vision_config()      # a missing frozen model is an error before anything is written
        utils.save_config(self.checkpoint_dir, self.args)

    def _vision_config(self):
        location = getattr(self.args, "vision_location", None)
        if not location or not os.path.exists(os.path.join(location, "config.json")):
            raise FileNotFoundError(
                f"a3vt: no trained vision model at args.vision_location = {location!r} (the auto-encoder is trained on the meshes "
                "a frozen Deformation predicts: a directory with config.json + model, written by vision/train.py or fetched by "
                "the reference's download_models.sh; or pass Engine(..., deform=<Deformation>))")
        vision_args, weights = utils.load_model_config(location)
        if not os.path.exists(weights):
            local = os.path.join(location, "model")      # a directory that was moved after it was written
            if not os.path.exists(local):
                raise FileNotFoundError(f"a3vt: the vision model's weights are missing: {weights} (from {location}/config.json)")
            weights = local
        return vision_args, weights

    def setup(self):
        """Everything ``__call__`` does before touching data (reference :56-73)."""
        if self._deform is not None:
            self.deform = self._deform
            self.mesh_info, self.initial_mesh = self.deform.adj_info, self.deform.initial_positions
        else:
            vision_args, weights = self._vision_config()
            self.mesh_info, self.initial_mesh = utils.load_mesh_vision(vision_args, self.vision_chart_location)
            self.deform = vision_model.Deformation(self.mesh_info, self.initial_mesh, vision_args).to(self.initial_mesh.device)
            self.deform.load_state_dict(torch.load(weights, map_location=self.initial_mesh.device))
            _ops.invalidate_bf16_copies()
        self.deform.eval()
        for p in self.deform.parameters():
            p.requires_grad_(False)
        self.n_vision_charts = self.initial_mesh.shape[0]
        self.auto_encoder = model.AutoEncoder(self.mesh_info, self.initial_mesh, self.args).to(self.initial_mesh.device)
        params = list(self.auto_encoder.parameters())
        self.optimizer = a3vt_optim.make_adam(params, self.args.lr, library=getattr(self.args, "library_adam", True))

    def __call__(self):
        self.setup()
        self.load()
        writer = SummaryWriter(os.path.join("experiments/tensorboard/", self.args.exp_type))
        train_loader, valid_loaders = self.get_loaders()
        if self.args.eval:
            self.load()
            with torch.no_grad():
                self.validate(valid_loaders, writer)
            return self.current_loss
        for epoch in range(0, self.args.epochs):
            self.epoch = epoch
            self.train(train_loader, writer)
            with torch.no_grad():
                self.validate(valid_loaders, writer)
            self.check_values()
        return self.best_loss

    def get_loaders(self):
        if self._loaders is not None:
            return self._loaders
        from torch.utils.data import DataLoader   # dataset classes: utility/data_loaders.py on args.data_root
        workers = getattr(self.args, "num_workers", 16)
        train_loader = ""
        if not self.args.eval:
            train_data = data_loaders.mesh_loader_vision(self.args, set_type="auto_train")
            train_loader = DataLoader(train_data, batch_size=self.args.batch_size, shuffle=True, num_workers=workers,
                                      collate_fn=train_data.collate, pin_memory=True)
        valid_data = data_loaders.mesh_loader_vision(self.args, set_type="test" if self.args.eval else "valid")
        valid_loader = DataLoader(valid_data, batch_size=self.args.batch_size, shuffle=False, num_workers=workers,
                                  collate_fn=valid_data.collate, pin_memory=True)
        return train_loader, valid_loader

    def _loss(self, img, charts, samples=None):
        """(B,) Chamfer distances between the frozen model's meshes and the auto-encoder's clouds, and the latents."""
        with torch.no_grad():
            verts, mask = self.deform(img, charts)
        verts = verts.detach()
        pred_points, latent = self.auto_encoder(verts, mask)
        cd = utils.chamfer_distance(verts, self.mesh_info["faces_i32"], pred_points, num=self.args.number_points, samples=samples)
        return cd, latent

    def train_step(self, img, charts, samples=None):
        """One optimisation step on device tensors; returns the (device) scalar loss.  No host sync.
        ``samples``: optional injected (face_idx, u, v) surface draws (parity tests); default = the Philox stream."""
        self.optimizer.zero_grad(set_to_none=True)
        cd, _ = self._loss(img, charts, samples)
        loss = self.args.loss_coeff * cd.mean()
        loss.backward()
        self.optimizer.step()
        return loss.detach()

    def train(self, data, writer):
        dev = self.initial_mesh.device
        total_loss = torch.zeros((), device=dev)
        iterations = 0
        self.auto_encoder.train()
        for k, batch in enumerate(data_loaders.DevicePrefetcher(data, dev)):
            img = batch["img"].to(dev, non_blocking=True)
            with torch.no_grad():
                charts = vision_model.prepare_mesh(batch, self.initial_mesh, self.args)
            loss = self.train_step(img, charts)
            total_loss += loss
            iterations += 1
            if self.log_interval and k % self.log_interval == 0:
                print(f"Train || Epoch: {self.epoch}, loss: {loss.item():.2f}, b_ptp:  {self.best_loss:.2f}")
        if iterations:
            self.train_loss = total_loss.item() / iterations
            writer.add_scalars("train_loss", {self.args.exp_id: self.train_loss}, self.epoch)

    def validate(self, valid_loader, writer):
        dev = self.initial_mesh.device
        total_loss = torch.zeros((), device=dev)
        self.auto_encoder.eval()
        num_examples = 0
        latents, names = [], []
        for v, batch in enumerate(data_loaders.DevicePrefetcher(valid_loader, dev)):
            img = batch["img"].to(dev, non_blocking=True)
            batch_size = img.shape[0]
            charts = vision_model.prepare_mesh(batch, self.initial_mesh, self.args)
            cd, latent = self._loss(img, charts)
            names += list(batch["names"])
            latents.append(latent)
            total_loss += self.args.loss_coeff * cd.mean() * batch_size       # (weighted by batch size, reference :193)
            num_examples += float(batch_size)
        total = (total_loss / max(num_examples, 1.0)).item()
        print(f"Valid || Epoch: {self.epoch}, train loss: {self.train_loss:.4f}, val loss: {total:.4f}, b_ptp:  {self.best_loss:.4f}")
        print("*******************************************************")
        print(f"Validation Accuracy: {total}")
        print("*******************************************************")
        if not self.args.eval:
            writer.add_scalars("valid_ptp", {self.args.exp_id: total}, self.epoch)
        self.current_loss = total
        if self.args.eval and latents:
            self.latents, self.latent_names = torch.cat(latents), names
            self.cluster(self.latents, names)

    def save(self):
        torch.save(self.auto_encoder.state_dict(), self.checkpoint_dir + "/model")
        torch.save(self.optimizer.state_dict(), self.checkpoint_dir + "/optim")

    def load(self):
        dev = self.initial_mesh.device
        if self.args.eval and getattr(self.args, "pretrained", False):
            location_vision = vision_pretrained_location(self.args)
            location_auto = pretrained_location(self.args)
            for location in (location_vision, location_auto):
                if not os.path.exists(os.path.join(location, "model")):
                    raise FileNotFoundError(
                        f"a3vt: no pretrained model at {location} (the reference fetches its weights with download_models.sh into "
                        "pterotactyl/pretrained/; point args.pretrained_root / $PTEROTACTYL_PRETRAINED at that directory)")
            vision_args, _ = utils.load_model_config(location_vision)
            self.mesh_info, self.initial_mesh = utils.load_mesh_vision(vision_args, self.vision_chart_location)
            self.n_vision_charts = self.initial_mesh.shape[0]
            self.deform = vision_model.Deformation(self.mesh_info, self.initial_mesh, vision_args).to(dev)
            self.deform.load_state_dict(torch.load(os.path.join(location_vision, "model"), map_location=dev))
            self.deform.eval()
            auto_args, _ = utils.load_model_config(location_auto)
            self.auto_encoder = model.AutoEncoder(self.mesh_info, self.initial_mesh, _with_knob(auto_args)).to(dev)
            self.auto_encoder.load_state_dict(torch.load(os.path.join(location_auto, "model"), map_location=dev))
            _ops.invalidate_bf16_copies()
            return
        try:
            self.auto_encoder.load_state_dict(torch.load(self.checkpoint_dir + "/model", map_location=dev))
            self.optimizer.load_state_dict(torch.load(self.checkpoint_dir + "/optim", map_location=dev))
        except (FileNotFoundError, AttributeError):
            return

    def check_values(self):
        if self.best_loss >= self.current_loss:
            improvement = self.best_loss - self.current_loss
            print(f"Saving with {improvement:.3f} improvement in Chamfer Distance on Validation Set ")
            self.best_loss = self.current_loss
            self.last_improvement = 0
            self.save()
        else:
            self.last_improvement += 1
            if self.last_improvement >= self.args.patience:
                raise StopIteration(f"Over {self.args.patience} steps since last improvement")

    @staticmethod
    def nearest_latents(latents, index, k=25):
        """Indices of the ``k - 1`` latents nearest to ``latents[index]`` in squared distance, nearest first, the example itself
        excluded (reference :333-335: ``topk`` of the ``k`` smallest, the first of which is the example)."""
        d = ((latents - latents[index].unsqueeze(0)) ** 2).sum(-1)
        d[index] = -1.0                     # the example first whatever ties there are
        k = min(k, latents.shape[0])
        return torch.topk(d, k, largest=False)[1][1:]

    def cluster(self, latents, names, example_nums=20):
        """For random examples: the nearest other objects in latent space; a collage of their images per example is written to
        ``results_dir`` when PIL and the object images (``<data_root>/images_colourful``) are there.  Returns
        ``[(example, [indices of its neighbours, distinct objects, nearest first])]``."""
        examples = random.choices(range(latents.shape[0]), k=example_nums)
        out = []
        for e in examples:
            main_obj = str(names[e][0]).split("/")[-1]
            seen, picked = [main_obj], []
            for c in self.nearest_latents(latents, e).tolist():
                obj = str(names[c][0]).split("/")[-1]
                if obj not in seen:
                    seen.append(obj)
                    picked.append(c)
            out.append((e, picked))
            self._collage(len(out) - 1, seen[:5])
        return out

    def _collage(self, v, objects, crop=20, img_dim=256):
        try:
            from PIL import Image
            image_dir = os.path.join(data_loaders.data_root(self.args), "images_colourful")
        except Exception:
            return
        paths = [os.path.join(image_dir, o + ".npy") for o in objects]
        if len(paths) < 5 or not all(os.path.exists(p) for p in paths):
            return
        new_im = Image.new("RGB", (img_dim * 5, img_dim))
        for i, p in enumerate(paths):
            new_im.paste(Image.fromarray(np.load(p)), (i * img_dim, 0))
        new_im.save(f"{self.results_dir}/valid_{v}.png")


def get_parser():
    """The reference trainer's flags and defaults (:351-448); ``--vision_location`` defaults to the pretrained ``t_p`` model."""
    default_vision = vision_pretrained_location(SimpleNamespace(use_img=False, finger=True))
    p = argparse.ArgumentParser()
    p.add_argument("--cut", type=float, default=0.33, help="The shared size of features in the GCN.")
    p.add_argument("--limit_data", action="store_true", default=False, help="use less data, for debugging.")
    p.add_argument("--finger", action="store_true", default=False, help="use only one finger.")
    p.add_argument("--vision_location", type=str, default=default_vision, help="the location of the deformation prediction.")
    p.add_argument("--number_points", type=int, default=30000, help="number of points sampled for the chamfer distance.")
    p.add_argument("--encoding_size", type=int, default=200, help="size of the latent vector")
    p.add_argument("--seed", type=int, default=0, help="Setting for the random seed.")
    p.add_argument("--lr", type=float, default=0.0003, help="Initial learning rate.")
    p.add_argument("--eval", action="store_true", default=False, help="Evaluate the trained model on the test set.")
    p.add_argument("--batch_size", type=int, default=16, help="Size of the batch.")
    p.add_argument("--val_grasps", type=int, default=-1, help="number of grasps to use during validation.")
    p.add_argument("--exp_id", type=str, default="test", help="The experiment name.")
    p.add_argument("--exp_type", type=str, default="test", help="The experiment group.")
    p.add_argument("--use_img", action="store_true", default=False, help="To use the image.")
    p.add_argument("--use_touch", action="store_true", default=False, help="To use the touch information.")
    p.add_argument("--patience", type=int, default=70, help="How many epochs without improvement before training stops.")
    p.add_argument("--loss_coeff", type=float, default=9000.0, help="Coefficient for loss term.")
    p.add_argument("--num_GCN_layers", type=int, default=20, help="Number of GCN layers in the auto-encoder's encoder.")
    p.add_argument("--hidden_GCN_size", type=int, default=300, help="Size of the feature vector of each GCN layer.")
    p.add_argument("--num_grasps", type=int, default=5, help="Number of grasps to train with.")
    p.add_argument("--epochs", type=int, default=1000, help="Number of epochs to use.")
    p.add_argument("--pretrained", action="store_true", default=False, help="load the pretrained model")
    # this package's knobs
    p.add_argument("--fused_decoder", dest="fused_decoder", action="store_true", default=FUSED_DECODER_DEFAULT,
                   help="run the FoldingNet decoder on the fused fold kernels")
    p.add_argument("--no_fused_decoder", dest="fused_decoder", action="store_false")
    return p


if __name__ == "__main__":
    Engine(get_parser().parse_args())()
