"""Drop-in for ``pterotactyl/utility/pretty_render.py``: ``CameraRenderer`` and ``render_representations`` on this library's own
ray caster (``ops.scene_render``, csrc/scene_render.hip) in place of pyrender on OpenGL.

THE SHADER IS NOT PYRENDER'S.  The camera (yfov 60 degrees, 0.01 .. 10, at [0, 0.6, 0.6] turned by xyz Euler [45, 0, 180] degrees), the
four point lights of intensity 1.8, the ambient 0.3 and the colour [228, 217, 111] are the reference's (:35-76, :129); the image is
Lambert shading of ray-cast hits at pixel centres, without shadows, specular term, vertex-normal smoothing or anti-aliasing.  It is
not the metallic-roughness model, and no image of it has been compared with one of pyrender's.

Differences that callers can see:
* ``add_object(verts, faces, colour=...)`` takes arrays or tensors where the reference takes a ``trimesh.Trimesh``; ``position`` /
  ``orientation`` pose it as the reference does (xyz Euler angles, radians).
* ``add_points`` adds analytic spheres: nothing is tessellated, so 100 000 points cost 100 000 primitives, not 100 000 UV spheres.
* ``render()`` returns an (H, W, 3) uint8 array, not a ``PIL.Image`` (PIL is imported only where files are written).
* ``render_batch(scenes)`` renders many scenes in ONE library call; ``render_representations`` renders the three images of ALL its
  objects in one and returns what it rendered."""
import numpy as np
import torch

from . import utils
from ... import ops as _ops

D = _ops.RENDER_DEFAULTS


def _on_device(a, dtype, device):
    t = a.detach() if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))
    return t.to(device=device, dtype=dtype)


class CameraRenderer:
    def __init__(self, cameraResolution=[512, 512], device=None):
        self.W, self.H = int(cameraResolution[0]), int(cameraResolution[1])
        self.device = torch.device(device) if device is not None else utils._device()
        self.lights = np.array(D["lights"], np.float32)          # (:36-58)
        self.ambient, self.background = D["ambient"], D["background"]
        self.yfov, self.znear, self.zfar = D["yfov"], D["znear"], D["zfar"]
        self.meshes, self.points = [], []
        self.update_camera_pose(D["cam_pos"], utils.euler_matrix(D["cam_euler_xyz_deg"], "xyz", degrees=True))   # (:75-76)

    def update_camera_pose(self, position, orientation):
        """The camera's pose: its position and its rotation matrix (it looks down its own -z)."""
        self.cam_pos = np.asarray(position, np.float32).reshape(3)
        self.cam_rot = np.asarray(orientation, np.float32).reshape(3, 3)

    def add_object(self, verts, faces, colour=D["colour"], position=[0, 0, 0], orientation=[0, 0, 0]):
        verts, faces = _on_device(verts, torch.float32, self.device).reshape(-1, 3), _on_device(faces, torch.int32, self.device).reshape(-1, 3)
        if any(position) or any(orientation):
            pose = utils.euler2matrix(angles=orientation, translation=position)
            verts = verts @ _on_device(pose[:3, :3].T, torch.float32, self.device) + _on_device(pose[:3, 3], torch.float32, self.device)
        self.meshes.append((verts, faces, tuple(int(c) for c in colour[:3])))

    def add_points(self, points, radius, colour=[0, 0, 0]):
        self.points.append((_on_device(points, torch.float32, self.device).reshape(-1, 3), float(radius), tuple(int(c) for c in colour[:3])))

    def remove_objects(self):
        self.meshes, self.points = [], []

    def scene(self):
        """What ``render()`` would render, as an entry of ``render_batch``'s list (the objects are shared, not copied)."""
        return dict(meshes=list(self.meshes), points=list(self.points), cam_pos=self.cam_pos.copy(), cam_rot=self.cam_rot.copy(),
                    size=(self.W, self.H), camera=(self.yfov, self.znear, self.zfar), lights=self.lights, ambient=self.ambient,
                    background=self.background, device=self.device)

    def render(self):
        return render_batch([self.scene()])[0]


def scene_tables(scenes):
    """The keyword arguments of the one ``ops.scene_render`` call that renders ``CameraRenderer.scene()`` entries, one image each.
    The entries must agree on image size, camera intrinsics, lights, ambient and background (they are arguments of the call, not of
    an image)."""
    first = scenes[0]
    shared = ("size", "camera", "ambient", "background")
    for s in scenes[1:]:
        if any(s[k] != first[k] for k in shared) or not np.array_equal(s["lights"], first["lights"]):
            raise ValueError("a3vt: render_batch renders scenes of one image size, camera, lighting and background per call")
    dev = first["device"]
    verts, faces, face_rgb, centres, radii, sphere_rgb, face_offset, sphere_offset = [], [], [], [], [], [], [0], [0]
    n_verts = 0
    for s in scenes:
        for v, f, colour in s["meshes"]:
            verts.append(v)
            faces.append(f + n_verts)
            face_rgb.append(torch.tensor(colour, dtype=torch.uint8, device=dev).expand(f.shape[0], 3))
            n_verts += v.shape[0]
        for p, radius, colour in s["points"]:
            centres.append(p)
            radii.append(torch.full((p.shape[0],), radius, dtype=torch.float32, device=dev))
            sphere_rgb.append(torch.tensor(colour, dtype=torch.uint8, device=dev).expand(p.shape[0], 3))
        face_offset.append(face_offset[-1] + sum(f.shape[0] for _, f, _ in s["meshes"]))
        sphere_offset.append(sphere_offset[-1] + sum(p.shape[0] for p, _, _ in s["points"]))

    def cat(parts, shape, dtype):
        return torch.cat(parts).contiguous() if parts else torch.zeros(shape, dtype=dtype, device=dev)
    return dict(verts=cat(verts, (0, 3), torch.float32), faces=cat(faces, (0, 3), torch.int32), face_rgb=cat(face_rgb, (0, 3), torch.uint8),
                centres=cat(centres, (0, 3), torch.float32), radii=cat(radii, (0,), torch.float32),
                sphere_rgb=cat(sphere_rgb, (0, 3), torch.uint8), face_offset=face_offset, sphere_offset=sphere_offset,
                image_scene=list(range(len(scenes))), cam_pos=torch.from_numpy(np.stack([s["cam_pos"] for s in scenes])).to(dev),
                cam_rot=torch.from_numpy(np.stack([s["cam_rot"] for s in scenes])).to(dev), yfov=first["camera"][0],
                znear=first["camera"][1], zfar=first["camera"][2], width=first["size"][0], height=first["size"][1],
                lights=first["lights"], ambient=first["ambient"], background=first["background"])


def render_batch(scenes):
    """The images of many ``CameraRenderer.scene()`` entries from ONE ``ops.scene_render`` call: a list of (H, W, 3) uint8 arrays."""
    if not scenes:
        return []
    return list(_ops.scene_render(**scene_tables(scenes), want_prim=False)["rgb"].cpu().numpy())


def save_image(array, path):
    from PIL import Image
    Image.fromarray(array).save(path)


def render_representations(locations, names, meshes, faces, num_points=100000, resolution=(512, 512)):
    """``mesh.png``, ``points.png`` and ``ground_truth.png`` of every object (reference :119-158): the predicted mesh with
    ``add_faces``' tripled faces, ``num_points`` area-weighted surface samples of it (``utils.batch_sample``) as spheres of
    radius 0.01, and the ground truth from ``<name>_verts.npy`` / ``<name>_faces.npy``; all 3 x len(names) images from ONE library
    call, then written into ``locations``.  Returns ``{"images": [(mesh, points, ground_truth) arrays per object], "points": the
    (B, num_points, 3) samples}``."""
    meshes = meshes.detach().cpu().numpy() if isinstance(meshes, torch.Tensor) else np.asarray(meshes)
    faces = faces.detach().cpu().numpy() if isinstance(faces, torch.Tensor) else np.asarray(faces)
    recon_face = utils.add_faces(faces)
    camera = CameraRenderer(list(resolution))
    dev, colour = camera.device, D["colour"]
    message = "rendering the predicted objects"
    print("*" * len(message) + "\n" + message + "\n" + "*" * len(message))
    verts = torch.from_numpy(np.ascontiguousarray(meshes, np.float32)).to(dev)
    rng = torch.random.get_rng_state()          # (the samples' seed is a draw from torch's generator: looking at a result must not
    points = utils.batch_sample(verts, torch.from_numpy(recon_face.astype(np.int32)).to(dev), num=num_points)
    torch.random.set_rng_state(rng)             # move the run that is being looked at)
    scenes = []
    for i, name in enumerate(names):
        camera.add_object(verts[i], recon_face, colour=colour)
        scenes.append(camera.scene())
        camera.remove_objects()
        camera.add_points(points[i], 0.01, colour)
        scenes.append(camera.scene())
        camera.remove_objects()
        camera.add_object(np.load(name + "_verts.npy"), utils.add_faces(np.load(name + "_faces.npy")), colour=colour)
        scenes.append(camera.scene())
        camera.remove_objects()
    images = render_batch(scenes)
    images = [tuple(images[3 * i:3 * i + 3]) for i in range(len(names))]
    for location, (mesh_img, points_img, truth_img) in zip(locations, images):
        save_image(mesh_img, f"{location}/mesh.png")
        save_image(points_img, f"{location}/points.png")
        save_image(truth_img, f"{location}/ground_truth.png")
    return {"images": images, "points": points}
