"""``pterotactyl.utility.data_loaders`` — the trainers' datasets and their wire formats.

``mesh_loader_vision`` (reference ``utility/data_loaders.py:132-258``) reads the on-disk layout the reference's
``download_data.sh`` / ``data_making`` scripts produce and yields the batch dict the trainer and ``prepare_mesh`` consume:

    <root>/point_cloud_info/<id>.npy             (30000, 3) float   surface samples of the object
    <root>/images_colourful/<id>.npy             (256, 256, 3) uint8 rendered image
    <root>/touch_charts/<id>/touch_charts.npy    50 grasps x 4 fingers x 25 vertices x (x, y, z, mask)
    <split file>                                 dict: set name -> object ids  (reference ``objects/data_split.npy``)

    batch = {"names": [(path, grasps)], "gt_points": (B,P,3) f32, "img": (B,3,256,256) f32 in [0,1] | (B,1) dummy,
             "touch_charts": (B,G,4,25,4) | (B,G,25,4) with ``finger`` | (B,1) dummy}

The data root is a directory argument (``args.data_root``, or the ``PTEROTACTYL_DATA`` environment variable) instead of
the reference's package-relative constants (:18-29) — the dataset is a download, not part of either tree.
``mesh_loader_touch`` (reference :47-127) is the touch trainer's dataset, ``mesh_loader_active`` (:263-336) the policy
environment's: see the classes.
``DevicePrefetcher`` is the host->HBM leg: pinned staging buffers and a copy stream one batch ahead of the compute
stream, so a 65 ms GPU step is not stalled by the 7.7 MB (no image) / 58 MB (image) batch upload.
"""
import os
import random
from glob import glob

import numpy as np
import torch


def data_root(args=None):
    root = getattr(args, "data_root", None) or os.environ.get("PTEROTACTYL_DATA")
    if not root:
        raise RuntimeError("a3vt: set args.data_root or PTEROTACTYL_DATA to the directory holding point_cloud_info/, "
                           "images_colourful/, touch_charts/ (the reference's download_data.sh output)")
    return root


def load_split(args=None):
    """The reference's ``objects/data_split.npy`` (:26-28): pickled dict of object-id lists per set."""
    path = getattr(args, "data_split", None) or os.path.join(data_root(args), "data_split.npy")
    return np.load(path, allow_pickle=True).item()


class mesh_loader_vision(object):
    def __init__(self, args, set_type="train"):
        self.args = args
        self.set_type = set_type
        root = data_root(args)
        self.point_dir = os.path.join(root, "point_cloud_info")
        self.touch_dir = os.path.join(root, "touch_charts")
        self.image_dir = os.path.join(root, "images_colourful")
        self.obj_dir = os.path.join(root, "object_info")
        split = load_split(args)
        training = set_type in ("recon_train", "auto_train")
        self.get_instance = self.get_training_instance if training else self.get_validation_instance
        names = [os.path.splitext(os.path.basename(f))[0] for f in glob(os.path.join(self.image_dir, "*.npy"))]
        if getattr(args, "limit_data", False):
            random.Random(0).shuffle(names)
            names = names[:2000]
        wanted = set(split[set_type])
        self.object_names = []
        seed = 0
        for n in names:
            if n in wanted and os.path.exists(os.path.join(self.point_dir, n + ".npy")) and \
                    os.path.exists(os.path.join(self.touch_dir, n)):
                for _ in range(1 if training else 5):   # validation objects appear 5x with different grasp subsets (:160-170)
                    self.object_names.append([n, seed])
                    seed += 1
        print(f"The number of {set_type} set objects found : {len(self.object_names)}")

    def __len__(self):
        return len(self.object_names)

    def get_training_instance(self, index):
        obj, _ = random.choice(self.object_names)
        count = random.choice(range(0, self.args.num_grasps + 1))
        order = list(range(50))
        random.shuffle(order)
        return obj, order[:count]

    def get_validation_instance(self, index):
        obj, seed = self.object_names[index]
        order = list(range(50))
        if getattr(self.args, "val_grasps", -1) >= 0 and self.args.eval:
            count = self.args.val_grasps
        else:
            count = random.Random(seed).choice(range(0, self.args.num_grasps + 1))
        random.Random(seed).shuffle(order)
        return obj, order[:count]

    def get_points(self, obj):
        samples = np.load(os.path.join(self.point_dir, obj + ".npy"))
        np.random.shuffle(samples)
        return torch.FloatTensor(samples[: self.args.number_points])

    def get_image(self, obj):
        if not self.args.use_img:
            return torch.empty((1))
        img = np.load(os.path.join(self.image_dir, obj + ".npy"))
        return torch.FloatTensor(img).permute(2, 0, 1) / 255.0

    def get_touch_info(self, obj, grasps):
        if not self.args.use_touch:
            return torch.ones((1))
        remaining = self.args.num_grasps - len(grasps)
        charts = torch.FloatTensor(np.load(os.path.join(self.touch_dir, obj, "touch_charts.npy"))).view(50, 4, 25, 4)
        if self.args.finger:
            return torch.cat((charts[grasps][:, 1], torch.zeros(remaining, 25, 4)))
        return torch.cat((charts[grasps], torch.zeros(remaining, 4, 25, 4)))

    def __getitem__(self, index):
        obj, grasps = self.get_instance(index)
        return {"names": (os.path.join(self.obj_dir, obj), grasps), "gt_points": self.get_points(obj),
                "img": self.get_image(obj), "touch_charts": self.get_touch_info(obj, grasps)}

    def collate(self, batch):
        out = {"names": [item["names"] for item in batch]}
        for key in ("gt_points", "img", "touch_charts"):
            out[key] = torch.stack([item[key] for item in batch])
        return out


class mesh_loader_touch(object):
    """The touch-trainer dataset (reference ``utility/data_loaders.py:47-127``): one item per successful touch,

        <root>/grasp_info/<id>/<grasp>/<finger>_touch.npy       (121, 121, 3) uint8-valued tactile image
        <root>/grasp_info/<id>/<grasp>/<finger>_points.npy      (n, 3) points of the surface the sensor saw
        <root>/grasp_info/<id>/<grasp>/<finger>_ref_frame.npy   pickled dict: rot (3, 3), pos (3,) of the finger

    for the objects of the split's ``set_type`` that also have an image and a point cloud.

        batch = {"names": [(id, grasp, finger)], "samples": (B,num_samples,3) f32, "sim_touch": (B,3,121,121) f32 in [0,1],
                 "ref": {"rot": (B,3,3), "pos": (B,3)}}"""

    def __init__(self, args, set_type="train"):
        self.args = args
        self.set_type = set_type
        root = data_root(args)
        self.grasp_dir = os.path.join(root, "grasp_info")
        point_dir, image_dir = os.path.join(root, "point_cloud_info"), os.path.join(root, "images_colourful")
        names = [os.path.splitext(os.path.basename(f))[0] for f in glob(os.path.join(image_dir, "*.npy"))]
        limit = getattr(args, "limit_data", False)
        if limit:
            random.shuffle(names)
            names = names[:3000]
        wanted = set(load_split(args)[set_type])
        self.object_names = []
        for n in names:
            if n in wanted and os.path.exists(os.path.join(point_dir, n + ".npy")) and os.path.exists(os.path.join(self.grasp_dir, n)):
                touches = glob(os.path.join(self.grasp_dir, n, "*", "*_touch.npy"))
                if limit:
                    random.shuffle(touches)
                    touches = touches[:7]
                for touch in touches:
                    grasp = os.path.basename(os.path.dirname(touch))
                    finger = os.path.basename(touch).split("_")[0]
                    self.object_names.append([n, grasp, finger])
        print(f"The number of {set_type} set objects found : {len(self.object_names)}")

    def __len__(self):
        return len(self.object_names)

    def standerdize_point_size(self, points):
        """``num_samples`` of the points in random order; a shorter file is repeated four-fold until it is long enough."""
        np.random.shuffle(points)
        points = torch.FloatTensor(points)
        while points.shape[0] < self.args.num_samples:
            points = torch.cat((points, points, points, points))
        return points[torch.randperm(points.shape[0])[: self.args.num_samples]]

    def get_finger_transforms(self, obj, grasp, finger):
        frame = np.load(os.path.join(self.grasp_dir, obj, str(grasp), f"{finger}_ref_frame.npy"), allow_pickle=True).item()
        return torch.FloatTensor(frame["rot"]), torch.FloatTensor(frame["pos"])

    def __getitem__(self, index):
        obj, grasp, finger = self.object_names[index]
        rot, pos = self.get_finger_transforms(obj, grasp, finger)
        touch = np.load(os.path.join(self.grasp_dir, obj, grasp, f"{finger}_touch.npy"))
        points = np.load(os.path.join(self.grasp_dir, obj, grasp, f"{finger}_points.npy"))
        return {"names": (obj, grasp, finger), "rot": rot, "pos": pos,
                "sim_touch": torch.FloatTensor(touch).permute(2, 0, 1).contiguous().view(3, 121, 121) / 255.0,
                "samples": self.standerdize_point_size(points)}

    def collate(self, batch):
        return {"names": [item["names"] for item in batch],
                "samples": torch.stack([item["samples"] for item in batch]),
                "sim_touch": torch.stack([item["sim_touch"] for item in batch]),
                "ref": {"rot": torch.stack([item["rot"] for item in batch]), "pos": torch.stack([item["pos"] for item in batch])}}


class mesh_loader_active(object):
    """The environment's dataset (reference ``utility/data_loaders.py:263-336``): the objects of the split's ``set_type`` that
    have an image file and a point cloud; ``limit_data`` keeps 400 of the image files (``random.Random(0)`` shuffle) before the
    filter; the length is rounded down to a multiple of ``env_batch_size``.

        batch = {"names": ["<root>/object_info/<id>"], "gt_points": (B,number_points,3) f32,
                 "img": (B,3,256,256) f32 in [0,1] | (B,1) dummy}"""

    def __init__(self, args, set_type="RL_train"):
        self.args = args
        self.set_type = set_type
        root = data_root(args)
        self.point_dir = os.path.join(root, "point_cloud_info")
        self.image_dir = os.path.join(root, "images_colourful")
        self.obj_dir = os.path.join(root, "object_info")
        names = [os.path.splitext(os.path.basename(f))[0] for f in glob(os.path.join(self.image_dir, "*.npy"))]
        if getattr(args, "limit_data", False):
            random.Random(0).shuffle(names)
            names = names[:400]
        wanted = set(load_split(args)[set_type])
        self.object_names = [n for n in names if os.path.exists(os.path.join(self.point_dir, n + ".npy")) and n in wanted]
        print(f"The number of {set_type} set objects found : {len(self.object_names)}")

    def __len__(self):
        return (len(self.object_names) // self.args.env_batch_size) * self.args.env_batch_size

    def get_instance(self, index):
        obj = self.object_names[index]
        count = random.choice(range(0, self.args.num_grasps + 1))
        order = list(range(50))
        random.shuffle(order)
        return obj, order[:count]

    def get_points(self, obj):
        samples = np.load(os.path.join(self.point_dir, obj + ".npy"))
        np.random.shuffle(samples)
        return torch.FloatTensor(samples[: self.args.number_points])

    def get_image(self, obj):
        if not self.args.use_img:
            return torch.empty((1))
        img = np.load(os.path.join(self.image_dir, obj + ".npy"))
        return torch.FloatTensor(img).permute(2, 0, 1) / 255.0

    def __getitem__(self, index):
        obj = self.object_names[index]
        return {"names": os.path.join(self.obj_dir, obj), "gt_points": self.get_points(obj), "img": self.get_image(obj)}

    def collate(self, batch):
        return {"names": [item["names"] for item in batch],
                "gt_points": torch.cat([item["gt_points"].unsqueeze(0) for item in batch]),
                "img": torch.cat([item["img"].unsqueeze(0) for item in batch])}


class DevicePrefetcher:
    """Iterates a loader of batch dicts, uploading tensors to ``device`` on a side stream one batch ahead.

    Each upload goes through a pinned staging buffer (re-used per key and shape) with ``non_blocking`` copies on a copy
    stream; the compute stream waits on the copy's event only when it first touches the batch.  Non-tensor entries
    (``names``) pass through."""

    def __init__(self, loader, device):
        self.loader, self.device = loader, torch.device(device)
        self.stream = torch.cuda.Stream(device=self.device)
        self._pinned = {}

    def _upload(self, batch):
        out, ready = {}, torch.cuda.Event()
        with torch.cuda.stream(self.stream):
            for k, v in batch.items():
                if not isinstance(v, torch.Tensor) or v.is_cuda:
                    out[k] = v
                    continue
                key = (k, tuple(v.shape), v.dtype)
                stage = self._pinned.get(key)
                if stage is None:   # two staging buffers per entry: batch n+1 is staged while batch n's copy may be in flight
                    stage = self._pinned[key] = [[torch.empty(v.shape, dtype=v.dtype, pin_memory=True), None] for _ in range(2)]
                slot = stage[0]
                stage.reverse()
                if slot[1] is not None:
                    slot[1].synchronize()   # the copy that last read this staging buffer has finished
                slot[0].copy_(v)
                out[k] = slot[0].to(self.device, non_blocking=True)
                slot[1] = ready
            ready.record(self.stream)
        return out, ready

    def __iter__(self):
        it = iter(self.loader)
        nxt = None
        try:
            nxt = self._upload(next(it))
        except StopIteration:
            return
        while nxt is not None:
            cur, ready = nxt
            try:
                nxt = self._upload(next(it))
            except StopIteration:
                nxt = None
            torch.cuda.current_stream(self.device).wait_event(ready)
            for v in cur.values():
                if isinstance(v, torch.Tensor):
                    v.record_stream(torch.cuda.current_stream(self.device))
            yield cur

    def __len__(self):
        return len(self.loader)
