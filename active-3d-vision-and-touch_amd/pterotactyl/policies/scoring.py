"""Batched scoring of candidate touches — the forward-only caller of the hot path.

The reference's greedy search evaluates candidates one at a time: ``ActiveTouch.best_step`` (``policies/environment.py:
167-214``) calls ``compute_obs(actions)`` (:221-249) once per candidate action — a full ``Deformation`` forward, three
Chamfer draws (``get_score`` :252-257) and device-to-host copies each, up to 50 times per environment step.  Meshes in a
batch are independent through the forward pass and the Chamfer loss, so the K candidates x E environment elements can
ride in ONE batch of K*E meshes: one stack call per refinement stage (M = K*E*N rows fills the chip; E*N alone is 2-7 k
rows, less than one round of the MFMA kernel), one nearest-neighbour launch per direction, one host copy.  Results are
identical to the sequential loop given the same surface samples (tests/test_gpu_trainer.py::test_batched_scoring).

Image features depend only on the environment element, so the image encoders run once on the E images and their maps are
shared by the K candidates (the reference recomputes them per candidate).
"""
import torch

from ... import ops
from ..utility import utils

# Whether touch_slots runs the predictor's head as one launch (ops.touch_chart_head) when the caller does not say: on only if the
# fused head's p90 lies below the torch tail's p10 at both n = 12 and n = 600 on an MI355X (tools/touch_bake_bench.py ->
# profiles/touch_bake_ab.txt).  The A/B on file meets the rule (the head alone: 0.10 ms against 0.27 at both sizes), and the default
# is still off: on, every caller's charts change in their last bits (another order of the fp32 sums), which is a change of its own —
# end to end the launch saves 1 % of a 600-view touch_slots call.
FUSED_HEAD_DEFAULT = False


def stack_charts(charts_list):
    """K chart dicts (each batched over E environment elements, ``prepare_mesh`` / ``environment.py:355-364`` format)
    -> one dict batched over K*E, candidate-major (index = k*E + e)."""
    return {key: torch.cat([c[key] for c in charts_list], dim=0) for key in charts_list[0]}


def touch_slots(encoder, touch, ref_frame, status, template, fused_head=None):
    """The touch charts and masks of a batch of sensor readings — what ``ActiveTouch.get_inputs`` (``policies/environment.py:
    294-353``) does with the touch model's predictions, for any leading shape at once (environments x fingers, or candidates x
    environments x fingers: one ``Encoder`` forward for all of them).

    encoder    : ``reconstruction.touch.model.Encoder`` (run under ``no_grad``)
    touch      : (..., 3, 121, 121) tactile images in [0, 1]
    ref_frame  : {"rot": (..., 3, 3), "pos": (..., 3)} finger frames
    status     : nested lists / array of strings with the leading shape: "touch", "no_touch" or anything else (no contact made)
    template   : (25, 3) chart template
    returns    : charts (..., 25, 3), masks (..., 25, 1): "touch" -> the predicted chart, mask 2; "no_touch" -> the chart collapsed
                 to the finger's position, mask 1; otherwise zeros, mask 0 — the ``touch_charts`` / ``touch_masks`` slots of
                 ``prepare_mesh`` / ``score_actions``' chart dicts.
    fused_head : with GPU inputs, the encoder's convolutions (``predict_features``) and then ONE ``ops.touch_chart_head`` launch for
                 the three linear layers, the template, the frame and the two selects; None: ``FUSED_HEAD_DEFAULT``.  Off, and on
                 the CPU, the torch lines below run as they always have."""
    import numpy as np
    lead = tuple(touch.shape[:-3])
    dev = touch.device
    status = np.asarray(status, dtype=object).reshape(lead)
    code = torch.from_numpy(np.where(status == "touch", 2, np.where(status == "no_touch", 1, 0)).astype(np.float32)).to(dev)
    n = int(code.numel())
    if (FUSED_HEAD_DEFAULT if fused_head is None else fused_head) and touch.is_cuda:
        with torch.no_grad():
            features = encoder.predict_features(touch.reshape(n, *touch.shape[-3:]))
        _, charts, masks = ops.touch_chart_head(features, encoder.fc, template.to(dev), ref_frame["rot"].to(dev).reshape(n, 3, 3),
                                                ref_frame["pos"].to(dev).reshape(n, 3), code.reshape(n).to(torch.int32), want_slots=True)
        return charts.reshape(*lead, -1, 3), masks.reshape(*lead, -1, 1)
    pos = ref_frame["pos"].to(dev).reshape(n, 3)
    ref = {"rot": ref_frame["rot"].to(dev).reshape(n, 3, 3), "pos": pos}
    verts = template.to(dev).view(1, -1, 3).repeat(n, 1, 1)
    with torch.no_grad():
        pred = encoder(touch.reshape(n, *touch.shape[-3:]), ref, verts)
    code = code.view(n, 1, 1)
    charts = torch.where(code == 2, pred, torch.where(code == 1, pos.view(n, 1, 3).expand_as(pred), torch.zeros_like(pred)))
    masks = code.expand(n, verts.shape[1], 1)
    return charts.reshape(*lead, verts.shape[1], 3).contiguous(), masks.reshape(*lead, verts.shape[1], 1).contiguous()


def score_actions(deform, img, charts_list, gt_points, faces, number_points, loss_coeff, repeat=3, samples=None):
    """Scores of K candidate touch configurations for E environment elements.

    deform       : ``vision.model.Deformation`` (used under ``no_grad``: activations are not saved)
    img          : (E,3,256,256) images or the (E,1) dummy of image-free models
    charts_list  : K chart dicts, each what ``get_inputs(actions)`` (:260-365) builds for one candidate action
    gt_points    : (E,P,3) ground-truth clouds, shared by the candidates of an element
    samples      : optional injected (face_idx, u, v), each (repeat,E,number_points), reused for every candidate
    returns      : ``score`` (K,E) = loss_coeff * Chamfer (``get_score`` :252-257), ``verts`` (K,E,N,3), ``mask`` (K,E,N,1)
    """
    return score_charts(deform, img, stack_charts(charts_list), len(charts_list), gt_points, faces, number_points, loss_coeff,
                        repeat=repeat, samples=samples)


def score_charts(deform, img, charts, K, gt_points, faces, number_points, loss_coeff, repeat=3, samples=None):
    """``score_actions`` on the chart dict already stacked over K * E, candidate-major (``stack_charts``' result, or what
    ``ActiveTouch.score_candidates`` assembles from its touch table in one launch): the same arguments otherwise, the same results."""
    dev = charts["vision_charts"].device
    E = gt_points.shape[0]
    with torch.no_grad():
        if getattr(deform.args, "use_img", False):
            img = img.to(dev)
            gmaps = [m.repeat(K, 1, 1, 1) for m in deform.img_encoder_global(img)]
            lmaps = [m.repeat(K, 1, 1, 1) for m in deform.img_encoder_local(img)]
        else:
            gmaps, lmaps = [], []
        verts, mask = deform.deform_with_maps(charts, gmaps, lmaps)
        # the E ground-truth clouds are shared by the K candidates of each element (candidate-major batch: mesh k*E + e is
        # compared with gt[e]): uploaded, sorted and boxed once, not K times (a3vt_chamfer_fwd_shared)
        gt = gt_points.to(dev).to(torch.float32)
        if samples is not None:
            samples = tuple(s.repeat(1, K, 1) for s in samples)
        cd = utils.chamfer_distance(verts, faces, gt, num=number_points, repeat=repeat, samples=samples)
        score = loss_coeff * cd
    n = verts.shape[1]
    return score.view(K, E), verts.view(K, E, n, 3), mask.view(K, E, n, 1)


def best_actions(score, taken_mask):
    """Greedy choice of :174-180: per element the lowest-scoring candidate not already taken.
    score (K,E); taken_mask (E,K) non-zero where the action was performed before.  Returns (E,) indices."""
    s = score.t().clone()
    s[taken_mask.to(s.device) != 0] = float("inf")
    return torch.argmin(s, dim=1)
