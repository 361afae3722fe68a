"""Drop-in for ``pterotactyl/reconstruction/touch/model.py`` — the touch chart predictor.

``Encoder`` turns a 121 x 121 tactile image and the finger's frame into a 25-vertex chart: six ``DoubleConv`` blocks
(three 5 x 5 convolutions each, the first of stride 2: maps of 61, 31, 16, 8, 4, 2 pixels), three linear layers
(512 -> 256 -> 128 -> 75), the prediction added to the chart template and moved into the finger's frame
(``rot . v + pos``).  Same module tree as the reference (so its checkpoints load: ``CNN_layers.{0..5}.double_conv.{0,1,3,4,6}``,
``CNN_layers.{0..4}.activation.0``, ``fc.{0,1,2}.0``), modules constructed in the reference's order (so
``torch.manual_seed(s); Encoder()`` draws the reference's initial weights), same methods.

``fused_stem`` (this package's knob): in ``eval()`` mode, with gradients disabled and the input on the GPU, the nine
convolutions of blocks 1-3 (78 % of the network's multiply-adds) run on ``a3vt_conv5f_nhwc`` (csrc/conv5f.hip: exact fp32 on the
matrix pipe) over channels-last maps, their eval-mode BatchNorm and ReLU folded into the kernel's epilogue.  Blocks 4-6 and the
linear layers stay on torch, as does everything in training (the kernels are forward-only), on the CPU, or with the knob off.
The default of the knob is ``FUSED_STEM_DEFAULT``: the result of the A/B in profiles/touch_encoder_ab.txt.

This package's own entry points: ``predict_features`` (everything before ``fc``: the (B, 512) vectors ``ops.touch_chart_head``
takes; ``predict_verts`` is ``fc`` of them) and ``predict_features_nhwc`` (the same from channels-last images, which the fused
stem takes as they are).

Differences from the reference: ``transform_verts`` does not write into its argument (the reference's ``verts += pos`` is
applied to a fresh tensor there too, the result of ``bmm``; here nothing is in place) and moves ``ref`` to the vertices' device
instead of calling ``.cuda()``; the BatchNorm layers are ``BatchNorm2d`` below (training passes avoid MIOpen's kernels);
``predict_verts`` runs torch's convolutions on MIOpen's deterministic kernels (``repeatable_torch_kernels``): two calls give the
same bits, as the library's own kernels do.
"""
import contextlib

import torch
import torch.nn as nn

from .... import ops as _ops

# Whether Encoder() runs the fused stem when the caller does not say: on only if the fused forward's p90 lies below the torch
# forward's p10 at both B = 12 and B = 600 on an MI355X (tools/touch_encoder_bench.py -> profiles/touch_encoder_ab.txt).
FUSED_STEM_DEFAULT = True

FUSED_BLOCKS = 3      # the DoubleConv blocks whose convolutions csrc/conv5f.hip takes: (3,16) (16,32) (32,32)


@contextlib.contextmanager
def repeatable_torch_kernels():
    """Torch's convolutions restricted to MIOpen's deterministic kernels for the duration.  Left to itself MIOpen runs the 64- and
    128-channel convolutions of blocks 4-6 (maps of 8 pixels and fewer) on kernels whose results change from call to call
    (measured on an MI355X: block 4's output differs between any two calls on the same input, forward, eval and train mode);
    with the flag every layer repeats bit for bit.  ``Encoder.predict_verts`` runs under it; a backward pass picks its kernels
    when it runs, so a caller that wants repeatable gradients wraps ``backward()`` too (``train.Engine.train_step`` does).
    The flag is torch's process-wide one, switched for the duration and restored: a process that drives the model from several
    threads, or captures / compiles it, sets ``torch.backends.cudnn.deterministic = True`` itself once, and nothing is switched
    here."""
    b = torch.backends.cudnn
    if b.deterministic:         # already so: nothing to switch
        yield
        return
    with b.flags(enabled=b.enabled, benchmark=b.benchmark, deterministic=True, allow_tf32=b.allow_tf32):
        yield


class BatchNorm2d(nn.BatchNorm2d):
    """``nn.BatchNorm2d`` whose TRAINING passes on the GPU take torch's own kernels instead of MIOpen's: MIOpen's fp32 training
    backward was measured on an MI355X at 3.2e-2 relative error in the weight gradient and 6e-4 in the input gradient on block 1's
    (2,16,61,61) maps (torch's kernels, the CPU and fp64 agree to 1e-7; tools/experiments/miopen_bn_bwd_accuracy.py), which puts
    1.4 % of error into the gradients of the first convolution.  Same parameters, buffers and state-dict keys; eval mode is
    untouched."""

    def forward(self, x):
        if self.training and x.is_cuda:
            b = torch.backends.cudnn
            with b.flags(enabled=False, benchmark=b.benchmark, deterministic=b.deterministic, allow_tf32=b.allow_tf32):
                return super().forward(x)
        return super().forward(x)


class DoubleConv(nn.Module):
    def __init__(self, in_channels, out_channels, last=False):
        super().__init__()
        self.last = last
        self.double_conv = nn.Sequential(
            nn.Conv2d(in_channels, out_channels, kernel_size=5, padding=2, stride=2),
            BatchNorm2d(out_channels),
            nn.ReLU(inplace=True),
            nn.Conv2d(out_channels, out_channels, kernel_size=5, padding=2),
            BatchNorm2d(out_channels),
            nn.ReLU(inplace=True),
            nn.Conv2d(out_channels, out_channels, kernel_size=5, padding=2),
        )
        self.activation = nn.Sequential(BatchNorm2d(out_channels), nn.ReLU(inplace=True))

    def forward(self, x):
        x = self.double_conv(x)
        return x if self.last else self.activation(x)

    def forward_fused(self, x):
        """The block on channels-last maps through ``ops.conv5f`` (eval mode, no gradients): every convolution with the
        BatchNorm and ReLU that follow it in its epilogue."""
        seq = self.double_conv
        x = _ops.conv5f(x, seq[0], seq[1], True)
        x = _ops.conv5f(x, seq[3], seq[4], True)
        if self.last:
            return _ops.conv5f(x, seq[6], None, False)
        return _ops.conv5f(x, seq[6], self.activation[0], True)


class Encoder(nn.Module):
    def __init__(self, fused_stem=None):
        super().__init__()
        self.fused_stem = FUSED_STEM_DEFAULT if fused_stem is None else bool(fused_stem)
        blocks = [DoubleConv(3, 16), DoubleConv(16, 32), DoubleConv(32, 32), DoubleConv(32, 64), DoubleConv(64, 128),
                  DoubleConv(128, 128, last=True)]
        self.CNN_layers = nn.Sequential(*blocks)
        self.fc = nn.Sequential(nn.Sequential(nn.Linear(512, 256), nn.ReLU()), nn.Sequential(nn.Linear(256, 128), nn.ReLU()),
                                nn.Sequential(nn.Linear(128, 75)))

    def takes_fused_stem(self, touch):
        return bool(self.fused_stem and not self.training and not torch.is_grad_enabled() and touch.is_cuda
                    and touch.dtype == torch.float32)

    def stem(self, touch):
        """Blocks 1-3: (B,3,121,121) -> (B,32,16,16)."""
        if self.takes_fused_stem(touch):
            return self.stem_nhwc(touch.permute(0, 2, 3, 1).contiguous())          # channels-last once; the kernels keep it
        for block in self.CNN_layers[:FUSED_BLOCKS]:
            touch = block(touch)
        return touch

    def stem_nhwc(self, x):
        """Blocks 1-3 on the fused kernels from a contiguous channels-last map: (B,121,121,3) -> (B,32,16,16)."""
        for block in self.CNN_layers[:FUSED_BLOCKS]:
            x = block.forward_fused(x)
        # (B,32,16,16) for torch's convolutions, as a CONTIGUOUS copy (32 KB per image): on a channels-last view MIOpen's
        # deterministic kernels (repeatable_torch_kernels) take 61 ms for blocks 4-6 at B = 600 instead of 2.5
        return x.permute(0, 3, 1, 2).contiguous()

    def _features(self, x):
        """Blocks 4-6 on the stem's output -> the (B, 512) vectors ``fc`` takes."""
        for block in self.CNN_layers[FUSED_BLOCKS:]:
            x = block(x)
        return x.contiguous().view(-1, 512)

    def predict_features(self, touch):
        """(B,3,121,121) -> (B,512): everything before ``fc``."""
        with repeatable_torch_kernels():
            return self._features(self.stem(touch))

    def predict_features_nhwc(self, signal):
        """``predict_features`` of sensor images as the samplers deliver them, channels LAST: (B,121,121,3) in [0, 1].  With the
        fused stem taken the images feed ``conv5f`` as they are — no pass that moves the channels first and none that moves them
        back — and the result is ``predict_features(signal.movedim(-1, -3))`` bit for bit; otherwise they are permuted once."""
        with repeatable_torch_kernels():
            if self.takes_fused_stem(signal):
                return self._features(self.stem_nhwc(signal.contiguous()))
            return self._features(self.stem(signal.permute(0, 3, 1, 2).contiguous()))

    def predict_verts(self, touch):
        return self.fc(self.predict_features(touch))

    def transform_verts(self, verts, ref):
        """Chart vertices from the sensor's frame into the world's: ``rot . v + pos`` per sample; the inputs are left alone."""
        pos = ref["pos"].to(verts.device).view(-1, 1, 3)
        rot = ref["rot"].to(verts.device)
        return torch.bmm(rot, verts.permute(0, 2, 1)).permute(0, 2, 1) + pos

    def forward(self, gel, ref_frame, verts):
        verts = verts + self.predict_verts(gel).view(-1, verts.shape[1], 3)
        return self.transform_verts(verts, ref_frame)
