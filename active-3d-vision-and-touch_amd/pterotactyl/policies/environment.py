"""Drop-in for ``pterotactyl/policies/environment.py`` — ``ActiveTouch``, the environment every policy drives.

Same attribute and method names, ``args`` fields, ``obs`` dict and ``reward`` / ``done`` rule as the reference (:23-378).  What
differs, and why:

* **The sampler is an argument.**  ``ActiveTouch(args, sampler=None)``: an object with the reference sampler's ``load_objects``,
  ``sample`` and ``disconnect`` (``simulator/scene/sampler.py:57-175``), or a factory ``callable(bs, vision)`` that makes one
  (``reset_pybullet`` then replaces the sampler as the reference does, :368-373; an instance is disconnected and kept).  With
  ``None`` the reference's simulator is imported when the environment is constructed — never at module import — and an
  ``ImportError`` names ``policies.recorded.RecordedSampler`` where it is not installed.
* **One greedy step is one batch** (``args.batched_greedy``, default ``BATCHED_GREEDY_DEFAULT``).  The reference's ``best_step``
  runs ``compute_obs`` once per candidate action (:174-180, :200-208).  Here the K candidates x E elements go through
  ``scoring.touch_slots`` (one touch-encoder forward over K*E*F images; not with the touch table, below) and
  ``scoring.score_charts`` (one stack call per refinement stage on K*E meshes, three surface draws, one
  shared-target search), and the (K, E) score table comes to the host in one copy.  ``args.candidate_chunk`` (default ``None``:
  all K at once) bounds the batch for a large E.  With the knob off the reference's loop runs, one ``compute_obs`` per candidate.
* **One touch table per episode** (``args.touch_table``, default ``TOUCH_TABLE_DEFAULT``; read with ``getattr``, no command-line
  flag).  The touch of action a on object e does not depend on what was touched before, and the samplers of this package are
  pure functions of (object, action, finger).  With the knob on, ``reset`` asks the sampler ONCE, for everything
  (``sampler.sample_table``: one render call for a ``RenderedSampler``), runs ONE touch-encoder forward over the E * A * F views
  (``scoring.touch_slots``) and keeps ``table_charts`` (E, A, F, 25, 3) and ``table_codes`` (E, A, F) on the device.  Every
  ``step``, ``check_step`` and candidate phase of the episode is then a gather from that table — ``ops.touch_assemble``, one
  library launch that writes the K * E stacked chart and mask tensors in their final layout — and neither the sampler, the
  encoder nor the host takes part.  With the knob off the sampler is asked once per candidate (a simulator is sequential) and
  every answer is encoded again; a sampler without ``sample_table`` (the reference's simulator) cannot serve the knob and is
  refused with it.  An action outside ``[0, num_actions)`` is refused with the table (the plain path asks the sampler, which
  answers "no_intersection").
* **The predictor's head in one launch** (``args.fused_head``, default ``scoring.FUSED_HEAD_DEFAULT``; read with ``getattr``, no
  command-line flag): every ``scoring.touch_slots`` call below passes it on.  Off, the torch lines run as they always have.
* **Candidates leave no trace.**  The reference writes every candidate into slot ``steps`` of ``touch_charts`` / ``touch_masks``
  and overwrites it in ``step``.  Here ``check_step`` and the candidates of ``best_step`` work on copies; only ``reset`` and
  ``step`` write the state.  What a caller observes is the same.
* **Latents** (``use_latent``) are computed for the meshes ``step`` produces; the batched candidates are scored without them.
* ``num_grasps`` must be 5: the reference views the charts as ``num_fingers * 5 * 25`` rows (:357, :361), where the literal 5
  is the number of grasps; other values are refused instead of being reshaped differently.
* ``score_samples`` (default ``None``): a ``(face_idx, u, v)`` triple, each ``(repeat, E, number_points)``, passed to
  ``utils.chamfer_distance`` as ``samples=`` in ``get_score`` (and repeated per candidate in the batched step): explicit surface
  draws for parity tests.
* Model locations: ``args.touch_location`` / ``vision_location`` / ``auto_location`` as in the reference; ``pretrained_recon``
  resolves them under ``args.pretrained_root`` or ``PTEROTACTYL_PRETRAINED`` (the reference's ``pretrained/`` directory).
"""
import importlib
import os
import random

import numpy as np
import torch

from ... import ops
from ..reconstruction.autoencoder import model as auto_model
from ..reconstruction.touch import model as touch_model
from ..reconstruction.vision import model as vision_model
from ..utility import data_loaders, utils
from . import scoring

# Whether best_step scores its candidates as one batch when args does not say: on only if the batched step's p90 lies below the
# loop's p10 at both chart topologies on an MI355X (tools/env_bench.py -> profiles/env_greedy_step_ab.txt).
BATCHED_GREEDY_DEFAULT = True

# Whether an episode's touches come from one table built at reset when args does not say: off until the A/B of
# tools/touch_table_bench.py (profiles/touch_table_ab.txt) is on file.
TOUCH_TABLE_DEFAULT = False

NUM_GRASPS = 5      # the literal 5 of the reference's chart views (:357, :361)


def candidate_actions(mask, num_actions, greedy_checks=None):
    """The candidates one greedy decision evaluates (:171-203).  ``mask`` (E, num_actions): non-zero where an action was taken.
    Returns ``(candidates, full)``: ``candidates[k][e]`` is the action candidate k tries on element e.

    Full search (``greedy_checks`` None or >= ``num_actions``): candidate k is action k for every element.  Limited search: per
    element ``random.sample(untaken actions, checks)`` with ``checks = min(greedy_checks, untaken actions of element 0)``, drawn
    in element order from Python's global ``random`` exactly as the reference draws them, so a seeded run picks its candidates."""
    mask = torch.as_tensor(mask)
    E = mask.shape[0]
    if greedy_checks is None or greedy_checks >= num_actions:
        return [[k] * E for k in range(num_actions)], True
    possible = [list(range(num_actions)) for _ in range(E)]
    for e in range(E):
        for action in sorted((int(a) for a in torch.where(mask[e] != 0)[0]), reverse=True):
            del possible[e][action]
    checks = min(greedy_checks, len(possible[0]))
    selected = [random.sample(possible[e], checks) for e in range(E)]
    return [[selected[e][k] for e in range(E)] for k in range(checks)], False


def choose_actions(scores, candidates, mask, full):
    """The greedy choice (:177-180, :205-208) from the host copy of the (K, E) score table: per element the lowest score, in a
    full search among the actions whose mask is 0; ties go to the earliest candidate (the reference's strict ``<`` over ascending
    k — decided here on the host, not by a device ``argmin``).  A limited search does not consult the mask again, as in the
    reference.

    Deviation: the reference starts from ``best_score = 1000`` and returns ``None`` for an element whose every score is >= 1000;
    here the lowest eligible score wins whatever its size."""
    scores = torch.as_tensor(scores).detach().cpu()
    mask = torch.as_tensor(mask)
    best = []
    for e in range(scores.shape[1]):
        pick, low = None, None
        for k in range(scores.shape[0]):
            action = candidates[k][e]
            if full and mask[e][action] != 0:
                continue
            s = float(scores[k, e])
            if pick is None or s < low:
                pick, low = action, s
        if pick is None:
            raise RuntimeError(f"ActiveTouch.best_step: element {e} has no action left to take")
        best.append(pick)
    return np.array(best)


class ActiveTouch:
    def __init__(self, args, sampler=None):
        self.args = args
        if args.num_grasps != NUM_GRASPS:
            raise ValueError(f"ActiveTouch: num_grasps must be {NUM_GRASPS} (the environment's chart layout is num_fingers * 5 * 25 "
                             f"rows, reference environment.py:357), got {args.num_grasps}")
        self._sampler_factory = self._factory_of(sampler)
        self.seed(self.args.seed)
        self.current_information = {}
        self.steps = 0
        self.score_samples = None
        self.touch_chart_location = "touch_chart"        # the packaged assets (the reference: objects/*.obj)
        self.vision_chart_location = "vision_charts"
        self.pretrained_recon_models()
        self.setup_recon()
        self.get_loaders()
        self.sampler = sampler if self._sampler_factory is None else self._sampler_factory(self.args.env_batch_size, False)
        self._use_table()

    @staticmethod
    def _factory_of(sampler):
        """None for a sampler instance; the factory otherwise (the reference's simulator when ``sampler`` is None)."""
        if sampler is None:
            try:
                sampler_module = importlib.import_module("pterotactyl.simulator.scene.sampler")
                grasping = importlib.import_module("pterotactyl.simulator.physics.grasping")
            except ImportError as e:
                raise ImportError("ActiveTouch: the reference's simulator (pterotactyl.simulator, which needs pybullet and pyrender) "
                                  "cannot be imported; pass sampler=, for instance a policies.recorded.RecordedSampler that replays "
                                  f"recorded touch signals ({e})") from e
            return lambda bs, vision: sampler_module.Sampler(grasping.Agnostic_Grasp, bs=bs, vision=vision)
        if hasattr(sampler, "sample"):
            missing = [m for m in ("load_objects", "sample", "disconnect") if not callable(getattr(sampler, m, None))]
            if missing:
                raise TypeError(f"ActiveTouch: the sampler lacks {missing}")
            return None
        if not callable(sampler):
            raise TypeError("ActiveTouch: sampler is a sampler object or a factory callable(bs, vision)")
        return sampler

    # Fix seeds
    def seed(self, seed):
        self.seed = seed
        torch.backends.cudnn.deterministic = True
        torch.backends.cudnn.benchmark = False
        torch.manual_seed(seed)
        if torch.cuda.is_available():
            torch.cuda.manual_seed_all(seed)
        np.random.seed(seed)

    # get dataloaders
    def get_loaders(self):
        if not self.args.eval:
            self.train_data = data_loaders.mesh_loader_active(self.args, set_type="RL_train")
            set_type = "valid"
        else:
            set_type = "test"
        self.valid_data = data_loaders.mesh_loader_active(self.args, set_type=set_type)

    def pretrained_recon_models(self):
        if getattr(self.args, "pretrained_recon", False):
            root = utils.pretrained_root(self.args)
            kind = ("v_t_" if self.args.use_img else "t_") + ("p" if self.args.finger else "g")     # :67-104
            self.args.touch_location = os.path.join(root, "reconstruction", "touch", "best") + "/"
            self.args.vision_location = os.path.join(root, "reconstruction", "vision", kind) + "/"
            self.args.auto_location = os.path.join(root, "reconstruction", "auto", kind) + "/"

    # initialize and load the correct reconstruction models
    def setup_recon(self):
        self.device = utils._device()
        self.touch_verts, _ = utils.load_mesh_touch(self.touch_chart_location)

        utils.load_model_config(self.args.touch_location)
        self.touch_prediction = touch_model.Encoder().to(self.device)
        self.touch_prediction.load_state_dict(torch.load(self.args.touch_location + "/model", map_location=self.device))
        self.touch_prediction.eval()

        vision_args, _ = utils.load_model_config(self.args.vision_location)
        self.mesh_info, self.initial_mesh = utils.load_mesh_vision(vision_args, self.vision_chart_location)
        self.initial_mesh = self.initial_mesh.to(self.device)
        self.n_vision_charts = self.initial_mesh.shape[0]
        self.deform = vision_model.Deformation(self.mesh_info, self.initial_mesh, vision_args).to(self.device)
        self.deform.load_state_dict(torch.load(self.args.vision_location + "/model", map_location=self.device))
        self.deform.eval()

        if self.args.use_latent:
            auto_args, _ = utils.load_model_config(self.args.auto_location)
            self.auto_encoder = auto_model.AutoEncoder(self.mesh_info, self.initial_mesh, auto_args, only_encode=True).to(self.device)
            self.auto_encoder.load_state_dict(torch.load(self.args.auto_location + "/model", map_location=self.device), strict=False)
            self.auto_encoder.eval()

    def _use_table(self):
        """Whether the episode's touches come from the touch table (``args.touch_table``); a sampler that cannot build one is
        refused."""
        knob = getattr(self.args, "touch_table", None)
        if not (TOUCH_TABLE_DEFAULT if knob is None else knob):
            return False
        if not callable(getattr(self.sampler, "sample_table", None)):
            raise ValueError(f"ActiveTouch: args.touch_table is set, and the sampler ({type(self.sampler).__name__}) has no "
                             "sample_table to build the table from")
        return True

    def build_touch_table(self):
        """``table_charts`` (E, A, F, 25, 3) and ``table_codes`` (E, A, F) int32 of the loaded objects: one ``sample_table`` call,
        one ``scoring.touch_slots`` call (one encoder forward) over the E * A * F views in (e, a, f) order."""
        table = self.sampler.sample_table(self.args.num_actions, fingers=[1] if self.args.finger else None, to_host=False)
        codes = table["touch_code"].to(self.device).to(torch.int32)
        status = np.array(["no_intersection", "no_touch", "touch"], dtype=object)[codes.cpu().numpy()]
        ref_frame = {"rot": table["finger_transform_rot_M"].to(self.device).float(),
                     "pos": table["finger_transfrom_pos"].to(self.device).float()}
        self.table_charts, _ = scoring.touch_slots(self.touch_prediction, self._images(table["touch_signal"]), ref_frame, status,
                                                   self.touch_verts, fused_head=getattr(self.args, "fused_head", None))
        self.table_codes = codes.contiguous()

    # reset the environment with new objects
    def reset(self, batch):
        self.current_data = {}
        self.steps = 0
        self.current_data["first_score"] = None
        self.current_data["batch"] = batch
        self.current_data["mask"] = torch.zeros([self.args.env_batch_size, self.args.num_actions])
        self.sampler.load_objects(batch["names"], from_dataset=True)
        if self._use_table():
            self.build_touch_table()
        obs = self.compute_obs()
        self.current_data["score"] = obs["score"]
        return obs

    # take a set in the environment with supplied actions
    def step(self, actions):
        self.update_masks(actions)
        obs = self.compute_obs(actions=actions)
        reward = self.current_data["score"] - obs["score"]
        self.current_data["score"] = obs["score"]
        self.steps += 1
        done = self.steps == self.args.budget
        return obs, reward, done

    # compute the best myopic greedy actions and perfrom them
    def best_step(self, greedy_checks=None):
        """The myopic greedy step (:167-213): score the candidates (``candidate_actions``), choose (``choose_actions``: unlike
        the reference, the lowest eligible score wins even when every score is >= 1000), then one ``step`` with the choice.
        Returns ``(actions, obs, reward, done)``."""
        actions, _ = self.greedy_choice(greedy_checks)
        obs, reward, done = self.step(actions)
        return actions, obs, reward, done

    def greedy_choice(self, greedy_checks=None):
        """The candidate phase of ``best_step`` alone: the chosen actions (E,) and the (K, E) host score table.  Changes no
        state (it consumes Python's ``random`` in a limited search)."""
        candidates, full = candidate_actions(self.current_data["mask"], self.args.num_actions, greedy_checks)
        batched = getattr(self.args, "batched_greedy", None)
        if BATCHED_GREEDY_DEFAULT if batched is None else batched:
            scores = self.score_candidates(candidates)
        else:
            scores = torch.stack([self.compute_obs(actions, commit=False)["score"] for actions in candidates])
        self.candidate_scores = scores
        return choose_actions(scores, candidates, self.current_data["mask"], full), scores

    def score_candidates(self, candidates, to_host=True):
        """(K, E) host scores of K candidate action lists: what K ``check_step`` calls would score, as one batch of K*E meshes
        (in chunks of ``args.candidate_chunk`` candidates).  The state is left alone.  ``to_host=False`` leaves the table on
        the device (for ``ops.candidate_tally``)."""
        K, E = len(candidates), self.args.env_batch_size
        chunk = getattr(self.args, "candidate_chunk", None) or K
        batch = self.current_data["batch"]
        gt = batch["gt_points"].to(self.device)
        samples = self._samples()
        scores = []
        for k0 in range(0, K, chunk):
            part = candidates[k0:k0 + chunk]
            stacked = self._table_candidates(part) if self._use_table() else self._sampled_candidates(part)
            score, _, _ = scoring.score_charts(self.deform, batch["img"], stacked, len(part), gt, self.mesh_info["faces"],
                                               self.args.number_points, self.args.loss_coeff, samples=samples)
            scores.append(score)
        scores = torch.cat(scores)
        return scores.cpu() if to_host else scores

    def _sampled_candidates(self, candidates):
        """The chart dict of n candidate action lists stacked over n * E, candidate-major: the sampler asked once per candidate,
        one ``scoring.touch_slots`` call for all of them."""
        E = self.args.env_batch_size
        signals = [self._signals(self.sampler.sample(actions, touch_point_cloud=True)) for actions in candidates]
        n = len(signals)
        touch, pos, rot = (torch.stack([s[i] for s in signals]) for i in range(3))
        slots, slot_masks = scoring.touch_slots(self.touch_prediction, touch, {"rot": rot, "pos": pos},
                                                [s[3] for s in signals], self.touch_verts,
                                                fused_head=getattr(self.args, "fused_head", None))      # (n, E, F, 25, 3 | 1)
        charts = self.touch_charts.unsqueeze(0).repeat(n, 1, 1, 1, 1, 1)
        masks = self.touch_masks.unsqueeze(0).repeat(n, 1, 1, 1, 1, 1)
        charts[:, :, :, self.steps] = slots
        masks[:, :, :, self.steps] = slot_masks
        return scoring.stack_charts([{"touch_charts": charts[k].view(E, -1, 3), "vision_charts": self.vision_charts,
                                      "touch_masks": masks[k].view(E, -1, 1), "vision_masks": self.vision_masks} for k in range(n)])

    def _table_candidates(self, candidates):
        """The same dict from the touch table: one ``ops.touch_assemble`` launch writes the stacked touch charts and masks."""
        n, E = len(candidates), self.args.env_batch_size
        charts, masks = ops.touch_assemble(self.table_charts, self.table_codes, self.touch_charts, self.touch_masks, candidates,
                                           self.steps)                                          # (n, E, F * 5 * 25, 3 | 1)
        return {"touch_charts": charts.view(n * E, -1, 3), "vision_charts": self.vision_charts.repeat(n, 1, 1),
                "touch_masks": masks.view(n * E, -1, 1), "vision_masks": self.vision_masks.repeat(n, 1, 1)}

    # check the result of perfroming a specific action
    def check_step(self, actions):
        return self.compute_obs(actions=actions, commit=False)

    # perfrom a given action and compute the new state observations
    def compute_obs(self, actions=None, commit=True):
        """The observation after ``actions`` (:221-249).  ``commit=False`` (``check_step``, the candidate loop) evaluates the
        actions on a copy of the touch state."""
        with torch.no_grad():
            charts = self.get_inputs(actions, commit=commit)
            img = self.current_data["batch"]["img"].to(self.device)
            verts, mask = self.deform(img, charts)
            if self.args.use_latent:
                latent = self.auto_encoder(verts.detach(), mask)
            score = self.get_score(verts, self.current_data["batch"]["gt_points"].to(self.device))

        if self.current_data["first_score"] is None:
            self.current_data["first_score"] = score
            if self.args.use_latent:
                self.current_data["first_latent"] = latent.data.cpu()

        mesh = torch.cat((verts, mask), dim=-1).data.cpu()
        obs = {
            "score": score.data.cpu().clone(),
            "first_score": self.current_data["first_score"].clone(),
            "mask": self.current_data["mask"].data.cpu().clone(),
            "names": self.current_data["batch"]["names"],
            "mesh": mesh.clone(),
        }
        if self.args.use_latent:
            obs["first_latent"] = self.current_data["first_latent"]
            obs["latent"] = latent.data.cpu()
        return obs

    def _samples(self):
        if self.score_samples is None:
            return None
        fi, u, v = self.score_samples
        return fi.to(self.device).to(torch.int32), u.to(self.device), v.to(self.device)

    # compute the Chamfer distance of object predictions
    def get_score(self, verts, gt_points):
        loss = utils.chamfer_distance(verts, self.mesh_info["faces"], gt_points, num=self.args.number_points,
                                      samples=self._samples())
        loss = self.args.loss_coeff * loss
        return loss.cpu()

    def _signals(self, signals):
        """One ``sampler.sample`` result -> images (E, F, 3, 121, 121) in [0, 1], positions (E, F, 3) and rotations (E, F, 3, 3)
        on the device, and the E x F status strings.  With ``finger`` it is finger 1 alone, its image truncated through uint8
        (:282-291); the four-finger branch takes the signal as it is (:319-327)."""
        status = signals["touch_status"]
        touch = signals["touch_signal"]
        if self.args.finger:
            touch = touch[:, 1:2]
            pos = signals["finger_transfrom_pos"][:, 1:2]
            rot = signals["finger_transform_rot_M"][:, 1:2]
            status = [[row[1]] for row in status]
        else:
            pos, rot = signals["finger_transfrom_pos"], signals["finger_transform_rot_M"]
            status = [list(row[:4]) for row in status]
        return self._images(touch), pos.to(self.device).float(), rot.to(self.device).float(), status

    def _images(self, signal):
        """Sensor images (..., 121, 121, 3) in 0..255, of the fingers read -> (..., 3, 121, 121) in [0, 1] on the device, the
        arithmetic of ``_signals`` and of the touch table alike: with ``finger`` truncated through uint8 first (:282-291), then
        ``/ 255.0`` in fp32.  (The truncation of images already on the device is made there: the same for values in 0..255.)"""
        if self.args.finger:
            signal = signal.to(torch.uint8).float() if signal.is_cuda else torch.FloatTensor(signal.data.numpy().astype(np.uint8))
        return signal.to(self.device).movedim(-1, -3) / 255.0

    # perform a given action and a convert the resulting signals into expected input for the reconstructor
    def get_inputs(self, actions=None, commit=True):
        """The chart dict of the reconstructor (:260-365).  ``actions=None`` (a reset) clears the touch state; otherwise the
        actions are performed and their charts fill slot ``steps`` of every finger — of the state itself, as the reference does,
        or with ``commit=False`` of a copy."""
        E = self.args.env_batch_size
        num_fingers = 1 if self.args.finger else 4
        if actions is None:
            self.touch_charts = torch.zeros((E, num_fingers, self.args.num_grasps, 25, 3), device=self.device)
            self.touch_masks = torch.zeros((E, num_fingers, self.args.num_grasps, 25, 1), device=self.device)
            self.vision_charts = self.initial_mesh.unsqueeze(0).repeat(E, 1, 1)
            self.vision_masks = 3 * torch.ones(self.vision_charts.shape[:-1], device=self.device).unsqueeze(-1)
            touch_charts, touch_masks = self.touch_charts, self.touch_masks
        elif self._use_table():
            # slot ``steps`` of every finger from the touch table; the result is a new tensor, so without commit the state is as it was
            actions = np.asarray(torch.as_tensor(actions).cpu()).reshape(1, E)
            touch_charts, touch_masks = ops.touch_assemble(self.table_charts, self.table_codes, self.touch_charts, self.touch_masks,
                                                           actions, self.steps)
            touch_charts = touch_charts.view(E, num_fingers, NUM_GRASPS, 25, 3)
            touch_masks = touch_masks.view(E, num_fingers, NUM_GRASPS, 25, 1)
            if commit:
                self.touch_charts, self.touch_masks = touch_charts, touch_masks
        else:
            touch, pos, rot, status = self._signals(self.sampler.sample(actions, touch_point_cloud=True))
            # "touch": the predicted chart, mask 2; "no_touch": the finger's position repeated, mask 1; otherwise zeros, mask 0
            # (:304-315, :339-353); predictions are indexed element * num_fingers + finger, as there
            slots, slot_masks = scoring.touch_slots(self.touch_prediction, touch, {"rot": rot, "pos": pos}, status, self.touch_verts,
                                                    fused_head=getattr(self.args, "fused_head", None))
            if commit:
                touch_charts, touch_masks = self.touch_charts, self.touch_masks
            else:
                touch_charts, touch_masks = self.touch_charts.clone(), self.touch_masks.clone()
            touch_charts[:, :, self.steps] = slots
            touch_masks[:, :, self.steps] = slot_masks
        return {
            "touch_charts": touch_charts.view(E, num_fingers * NUM_GRASPS * 25, 3).clone(),
            "vision_charts": self.vision_charts.clone(),
            "touch_masks": touch_masks.view(E, num_fingers * NUM_GRASPS * 25, 1).clone(),
            "vision_masks": self.vision_masks.clone(),
        }

    # this is perfromed due to a meoery leak in pybullet where loaded meshes are not properly deleted
    def reset_pybullet(self):
        self.sampler.disconnect()
        if self._sampler_factory is not None:
            del self.sampler
            self.sampler = self._sampler_factory(self.args.env_batch_size, True)

    # update the set of action which have been performed
    def update_masks(self, actions):
        for i in range(actions.shape[0]):
            self.current_data["mask"][i, actions[i]] = 1
