"""The parts of the reference's `dust3r/viz.py` that the scene API and the demo's export need, batched on the GPU:
- sky segmentation (`segment_sky`, viz.py:345-381; `BasePCOptimizer.mask_sky`): one call segments every image of a scene (csrc/sky.hip,
  C ABI `d3r_segment_sky`) where the reference runs OpenCV and SciPy per image;
- the geometry of the GLB export (`pts3d_to_trimesh` + `cat_meshes`, viz.py:38-87, or the masked point cloud): `scene_mesh_batch`, one call
  for all views (csrc/mesh.hip, C ABI `d3r_scene_mesh`), and the camera glyphs of `add_scene_cam` (viz.py:246-319) restated without trimesh
  (`scene_camera_geometry`). dust3r_amd/glb.py writes the file, dust3r_amd/demo.py mirrors the demo's export functions.
The viewers (SceneViz, show_*) are not mirrored."""
import numpy as np
import torch

from . import _lib
from ._lib import check, current_stream, lib, ptr

OPENGL = np.array([[1, 0, 0, 0],
                   [0, -1, 0, 0],
                   [0, 0, -1, 0],
                   [0, 0, 0, 1]])

CAM_COLORS = [(255, 0, 0), (0, 0, 255), (0, 255, 0), (255, 0, 255), (255, 204, 0), (0, 204, 204),
              (128, 255, 255), (255, 128, 255), (255, 255, 128), (0, 0, 0), (128, 128, 128)]


def _as_hwc(image):
    """The image as a tensor where it already is (a contiguous numpy array is wrapped, not copied; a device tensor stays on its device)."""
    t = image.detach() if isinstance(image, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(image))
    if t.ndim != 3 or t.shape[2] != 3:
        raise ValueError(f'segment_sky takes H x W x 3 RGB images, got shape {tuple(t.shape)}')
    if t.dtype not in (torch.uint8, torch.float32):
        raise TypeError(f'segment_sky takes uint8 or float32 (in [0, 1]) images, got {t.dtype}')
    return t


@torch.no_grad()
def segment_sky_batch(images, device):
    """Sky masks of a list of H x W x 3 RGB images (numpy arrays or tensors, all uint8 or all float32 in [0, 1]; sizes may differ), computed
    in one batched call on `device`: a list of (H, W) torch.bool tensors on that device."""
    _lib.require_device()
    arrays = [_as_hwc(im) for im in images]
    if not arrays:
        return []
    is_u8 = arrays[0].dtype == torch.uint8
    if any((a.dtype == torch.uint8) != is_u8 for a in arrays):
        raise TypeError('segment_sky_batch: mix of uint8 and float32 images')
    device = torch.device(device)
    shapes = [a.shape[:2] for a in arrays]
    n, max_area = len(arrays), max(h * w for h, w in shapes)
    rgb = torch.zeros((n, max_area, 3), dtype=torch.uint8 if is_u8 else torch.float32, device=device)
    for i, a in enumerate(arrays):
        rgb[i, :a.shape[0] * a.shape[1]] = a.reshape(-1, 3)            # one copy: host -> device, or device -> device
    hs = torch.tensor([h for h, w in shapes], dtype=torch.int32, device=device)
    ws = torch.tensor([w for h, w in shapes], dtype=torch.int32, device=device)
    masks = torch.empty((n, max_area), dtype=torch.bool, device=device)
    work = torch.empty(int(lib.d3r_segment_sky_workspace_bytes(n, max_area)), dtype=torch.uint8, device=device)
    with torch.cuda.device(device):
        check(lib.d3r_segment_sky(n, ptr(rgb), int(is_u8), ptr(hs), ptr(ws), max_area, ptr(masks), ptr(work), current_stream()), 'segment_sky')
    return [masks[i, :h * w].view(h, w) for i, (h, w) in enumerate(shapes)]


def segment_sky(image):
    """The reference's `segment_sky(image)`: an H x W x 3 RGB image (numpy or tensor; float32 in [0, 1] or uint8) -> its sky mask as a CPU
    (H, W) torch.bool tensor. Runs on the current GPU."""
    return segment_sky_batch([image], torch.device('cuda', torch.cuda.current_device()))[0].cpu()


# ---- GLB export geometry -----------------------------------------------------------------------------------------------------------
def _tensor(x):
    return x.detach() if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(x))


@torch.no_grad()
def scene_mesh_batch(imgs, pts3d, masks, device, as_pointcloud=False):
    """The geometry of the demo's GLB export for all views in one GPU call (csrc/mesh.hip).

    imgs: H x W x 3 RGB images (numpy or tensors, all uint8 or all floating in [0, 1]; sizes may differ). pts3d: per view an (H, W, 3) map, or
    the padded (n, max_area, 3) tensor of `scene.get_pts3d(raw=True)`. masks: per view an (H, W) boolean map. Numpy inputs are uploaded,
    device tensors are used where they are.

    Mesh mode: the faces of the reference's `cat_meshes([pts3d_to_trimesh(img, pts, mask) ...])` as uint32 (every vertex of every view is
    kept), a colour per vertex (the mean of the colours of the valid faces that use it; include/dust3r_hip.h d3r_scene_mesh), and every
    view's points as positions. Point-cloud mode: the valid points and their colours, views in order then raster order.

    Returns a dict of host arrays: positions (N, 3) float32, colors (N, 4) uint8 (RGBA), faces (F, 3) uint32 or None, counts (n,) int64 (faces
    or points per view), bounds = (min (3,), max (3,)) float32 of the positions a face uses (mesh) or of the points (NaN components are
    skipped; +inf / -inf where no value is left), None when nothing is valid. The per-view counts are the one host synchronisation."""
    from .utils.device import host_tensor
    _lib.require_device()
    device = torch.device(device)
    n = len(masks)
    if len(imgs) < n or len(pts3d) != n:
        raise ValueError(f'scene_mesh_batch: {len(imgs)} images, {len(pts3d)} pointmaps, {n} masks')
    if n == 0:
        raise ValueError('scene_mesh_batch: no views')
    images = [_tensor(im) for im in imgs[:n]]
    images = [im.float() if im.is_floating_point() and im.dtype != torch.float32 else im for im in images]
    images = [_as_hwc(im) for im in images]
    is_u8 = images[0].dtype == torch.uint8
    if any((im.dtype == torch.uint8) != is_u8 for im in images):
        raise TypeError('scene_mesh_batch: mix of uint8 and float images')
    shapes = [tuple(im.shape[:2]) for im in images]
    areas = [h * w for h, w in shapes]
    n_vert = sum(areas)
    if n_vert >= 2 ** 32:
        raise ValueError(f'scene_mesh_batch: {n_vert} vertices do not fit uint32 indices (as_pointcloud=True or fewer views)')
    max_area = max(areas)
    if isinstance(pts3d, torch.Tensor) and pts3d.ndim == 3:          # the padded layout of scene.get_pts3d(raw=True)
        if pts3d.shape[1] < max_area or pts3d.shape[2] != 3:
            raise ValueError(f'scene_mesh_batch: padded pointmaps {tuple(pts3d.shape)} for views of up to {max_area} pixels')
        pts = pts3d.detach().to(device=device, dtype=torch.float32).contiguous()
        max_area = pts.shape[1]
    else:
        pts = torch.zeros((n, max_area, 3), dtype=torch.float32, device=device)
        for i, (p, a) in enumerate(zip(pts3d, areas)):
            p = _tensor(p)
            if p.numel() != 3 * a:
                raise ValueError(f'scene_mesh_batch: pointmap {i} has shape {tuple(p.shape)}, its image {shapes[i]}')
            pts[i, :a] = p.reshape(a, 3)
    mask = torch.zeros((n, max_area), dtype=torch.uint8, device=device)
    rgb = torch.zeros((n, max_area, 3), dtype=torch.uint8 if is_u8 else torch.float32, device=device)
    for i, (m, im, a) in enumerate(zip(masks, images, areas)):
        m = _tensor(m)
        if m.numel() != a:
            raise ValueError(f'scene_mesh_batch: mask {i} has shape {tuple(m.shape)}, its image {shapes[i]}')
        mask[i, :a] = m.reshape(a)
        rgb[i, :a] = im.reshape(a, 3)
    hs = torch.tensor([h for h, w in shapes], dtype=torch.int32, device=device)
    ws = torch.tensor([w for h, w in shapes], dtype=torch.int32, device=device)
    n_faces = sum(4 * (h - 1) * (w - 1) for h, w in shapes if h > 1 and w > 1)
    faces = None if as_pointcloud else torch.empty((max(n_faces, 1), 3), dtype=torch.int32, device=device)
    points = torch.empty((n_vert, 3), dtype=torch.float32, device=device) if as_pointcloud else None
    colors = torch.empty((n_vert,), dtype=torch.int32, device=device)
    small = torch.empty((n + 3,), dtype=torch.int64, device=device)       # counts [n] int64, then bounds [6] fp32: one read-back
    work = torch.empty(int(lib.d3r_scene_mesh_workspace_bytes(n, max_area)), dtype=torch.uint8, device=device)
    with torch.cuda.device(device):
        check(lib.d3r_scene_mesh(n, ptr(pts), ptr(mask), ptr(rgb), int(is_u8), ptr(hs), ptr(ws), max_area, int(bool(as_pointcloud)), ptr(faces),
                                 ptr(points), ptr(colors), ptr(small), ptr(small[n:].view(torch.float32)), ptr(work), current_stream()), 'scene_mesh')
        small = small.cpu()
        counts = small[:n].numpy().copy()
        lo, hi = small[n:].view(torch.float32).numpy()[:3].copy(), small[n:].view(torch.float32).numpy()[3:].copy()
        total = int(counts.sum())
        if as_pointcloud:
            positions = host_tensor((total, 3), torch.float32)
            positions.copy_(points[:total])
            col = host_tensor((total,), torch.int32)
            col.copy_(colors[:total])
            face_arr = None
        else:
            positions = host_tensor((n_vert, 3), torch.float32)
            if n * max_area == n_vert:
                positions.copy_(pts.view(n_vert, 3))
            else:
                start = 0
                for i, a in enumerate(areas):
                    positions[start:start + a].copy_(pts[i, :a])
                    start += a
            col = host_tensor((n_vert,), torch.int32)
            col.copy_(colors)
            face_host = host_tensor((total, 3), torch.int32)
            face_host.copy_(faces[:total])
            face_arr = face_host.numpy().view(np.uint32)
    return dict(positions=positions.numpy(), colors=col.numpy().view(np.uint8).reshape(-1, 4), faces=face_arr, counts=counts,
                bounds=(lo, hi) if total > 0 else None)


def _rot_z(deg):
    from scipy.spatial.transform import Rotation
    r = np.eye(4)
    r[:3, :3] = Rotation.from_euler('z', np.deg2rad(deg)).as_matrix()
    return r


def _apply(T, pts):
    return pts @ T[:3, :3].T + T[:3, 3]


# the 4-section cone of add_scene_cam (trimesh.creation.cone(width, height, sections=4)), restated: base centre, four base corners on the
# x / y axes, apex. Side faces (corner k, corner k + 1, apex); base faces contain vertex 0 and are never drawn.
_CONE_FACES = [(k + 1, (k + 1) % 4 + 1, 5) for k in range(4)] + [(0, (k + 1) % 4 + 1, k + 1) for k in range(4)]


def scene_camera_geometry(pose_c2w, focal, imsize, screen_width=0.03):
    """The camera glyph of the reference's `add_scene_cam` (viz.py:246-319) in world coordinates, without trimesh: the frustum of a camera
    at `pose_c2w` (4 x 4 camera-to-world, OpenCV axes) with its apex at the optical centre and a W/H base at depth
    height = max(sw / 10, focal sw / H), sw = screen_width.

    Returns wire_vertices (18, 3) and wire_faces (48, 3): the thin slivers that draw the frustum's 8 edges (from the 0.95-scaled and the
    2-degree rotated copies of the cone, both windings), and image_vertices (4, 3), image_faces (4, 3), image_uv (4, 2): the quad that
    carries the picture. uv (0, 0) is the base corner on the ray of pixel (0, 0), so the picture appears as the camera saw it (trimesh's cone
    vertex order, which fixes the reference's corners, is not reproduced). fp64."""
    W, H = imsize
    if isinstance(focal, np.ndarray):
        focal = focal.reshape(-1)[0]
    if not focal:
        focal = min(H, W) * 1.1
    height = max(screen_width / 10, focal * screen_width / H)
    width = screen_width * 0.5 ** 0.5
    rot45 = _rot_z(45)
    rot45[2, 3] = -height
    aspect = np.eye(4)
    aspect[0, 0] = W / H
    transform = np.asarray(pose_c2w, dtype=np.float64) @ OPENGL @ aspect @ rot45
    ang = np.arange(4) * (np.pi / 2)
    cone = np.zeros((6, 3))
    cone[1:5, 0], cone[1:5, 1] = width * np.cos(ang), width * np.sin(ang)
    cone[5, 2] = height
    verts = _apply(transform, np.r_[cone, 0.95 * cone, _apply(_rot_z(2), cone)])
    faces = []
    for a, b, c in _CONE_FACES:
        if 0 in (a, b, c):
            continue
        a2, b2, c2 = a + 6, b + 6, c + 6
        a3, b3, c3 = a + 12, b + 12, c + 12
        faces += [(a, b, b2), (a, a2, c), (c2, b, c), (a, b, b3), (a, a3, c), (c3, b, c)]
    faces += [(c, b, a) for a, b, c in faces]
    # corners 2, 1, 4, 3 are (-x, -y), (+x, -y), (+x, +y), (-x, +y) in camera axes: image top-left, top-right, bottom-right, bottom-left
    image_vertices = _apply(transform, cone[[2, 1, 4, 3]])
    return dict(wire_vertices=verts, wire_faces=np.array(faces, dtype=np.int64), image_vertices=image_vertices,
                image_faces=np.array([[0, 1, 2], [0, 2, 3], [2, 1, 0], [3, 2, 0]]), image_uv=np.float32([[0, 0], [1, 0], [1, 1], [0, 1]]))
