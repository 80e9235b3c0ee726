"""The parts of the reference's `dust3r/viz.py` that the scene API and the demo's export need, batched on the GPU:
- sky segmentation (`segment_sky`, viz.py:345-381; `BasePCOptimizer.mask_sky`): one call segments every image of a scene (csrc/sky.hip,
  C ABI `d3r_segment_sky`) where the reference runs OpenCV and SciPy per image;
- the geometry of the GLB export (`pts3d_to_trimesh` + `cat_meshes`, viz.py:38-87, or the masked point cloud): `scene_mesh_batch`, one call
  for all views (csrc/mesh.hip, C ABI `d3r_scene_mesh`), and the camera glyphs of `add_scene_cam` (viz.py:246-319) restated without trimesh
  (`scene_camera_geometry`). dust3r_amd/glb.py writes the file, dust3r_amd/demo.py mirrors the demo's export functions;
- `SceneViz` (viz.py:119-209) as a HEADLESS viewer: the same `add_pointcloud` / `add_camera` / `add_cameras`, and `render` / `show` that draw
  the scene into images with the rasteriser of csrc/render.hip (`render_batch`, C ABI `d3r_render_*`) instead of opening a window.
- the fused cloud (new): `fuse_points` merges the views' pointmaps into one voxel-fused, weighted cloud (csrc/fuse.hip, C ABI
  `d3r_fuse_bounds` / `d3r_fuse_voxels`), a `FusedCloud`; dust3r_amd/export.py writes it as PLY or as a COLMAP model. Its `cluster` /
  `keep_clusters` separate the scene from dense floaters (DBSCAN, csrc/cloud_cluster.hip); `label_colors` paints the clusters.
The interactive viewers (a window, show_raw_pointcloud*) are not mirrored."""
import math

import numpy as np
import torch

from . import _lib
from ._lib import check, current_stream, lib, ptr
from .utils.padded import pad_views, shape_tables, split_views

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


def _tensor(x):
    return x.detach() if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(x))


def _images(imgs, name, floats='float'):
    """H x W x 3 tensors, all uint8 or all float32 (floats='float': any floating dtype, converted; 'float32': only that): images, is_u8, shapes"""
    images = [_tensor(im) for im in imgs]
    if floats == 'float':
        images = [im.float() if im.is_floating_point() and im.dtype != torch.float32 else im for im in images]
    images = [_as_hwc(im) for im in images]
    is_u8 = bool(images) and images[0].dtype == torch.uint8
    if any((im.dtype == torch.uint8) != is_u8 for im in images):
        raise TypeError(f'{name}: mix of uint8 and {floats} images')
    return images, is_u8, [tuple(im.shape[:2]) for im in images]


def ingest_views(imgs, pts3d, masks, weights, device, name, shapes=None):
    """The one ingestion of scene_mesh_batch, fuse_points and cloud_tracks: (pts, mask, wgt, rgb, is_u8, shapes, row, hs, ws), the padded
    stacks of utils/padded.py on `device` and the int32 shape tables. imgs None: no rgb / is_u8, and `shapes` gives the views' (H, W);
    weights None: no wgt. A ready stack among pts3d, masks, weights sets the rows of all. Every error carries `name`, the caller's."""
    images = is_u8 = rgb = None
    if imgs is not None:
        images, is_u8, shapes = _images(imgs, name)
    row = next((x.shape[1] for x, nd in ((pts3d, 3), (masks, 2), (weights, 2)) if isinstance(x, torch.Tensor) and x.ndim == nd), None)
    pts = pad_views(pts3d, device, torch.float32, (3,), row, shapes, f'{name}: pointmap')
    mask = pad_views(masks, device, torch.uint8, (), row, shapes, f'{name}: mask')
    wgt = None if weights is None else pad_views(weights, device, torch.float32, (), row, shapes, f'{name}: weight')
    if images is not None:
        rgb = pad_views(images, device, torch.uint8 if is_u8 else torch.float32, (3,), row, shapes, f'{name}: image')
    return (pts, mask, wgt, rgb, is_u8, shapes, pts.shape[1]) + shape_tables(shapes, device)[:2]


@torch.no_grad()
def segment_sky_batch(images, device):
    """Sky masks of a list of H x W x 3 RGB images (numpy arrays or tensors, all uint8 or all float32 in [0, 1]; sizes may differ), computed
    in one batched call on `device`: a list of (H, W) torch.bool tensors on that device."""
    _lib.require_device()
    arrays, is_u8, shapes = _images(images, 'segment_sky_batch', floats='float32')
    if not arrays:
        return []
    device = torch.device(device)
    rgb = pad_views(arrays, device, torch.uint8 if is_u8 else torch.float32, tail=(3,))
    n, max_area = rgb.shape[:2]
    hs, ws, _ = shape_tables(shapes, device)
    masks = torch.empty((n, max_area), dtype=torch.bool, device=device)
    work = _lib.workspace(lib.d3r_segment_sky_workspace_bytes(n, max_area), device)
    with torch.cuda.device(device):
        check(lib.d3r_segment_sky(n, ptr(rgb), int(is_u8), ptr(hs), ptr(ws), max_area, ptr(masks), ptr(work), current_stream()), 'segment_sky')
    return split_views(masks, shapes)


def segment_sky(image):
    """The reference's `segment_sky(image)`: an H x W x 3 RGB image (numpy or tensor; float32 in [0, 1] or uint8) -> its sky mask as a CPU
    (H, W) torch.bool tensor. Runs on the current GPU."""
    return segment_sky_batch([image], torch.device('cuda', torch.cuda.current_device()))[0].cpu()


# ---- GLB export geometry -----------------------------------------------------------------------------------------------------------
@torch.no_grad()
def scene_mesh_batch(imgs, pts3d, masks, device, as_pointcloud=False, to_host=True):
    """The geometry of the demo's GLB export for all views in one GPU call (csrc/mesh.hip).

    imgs: H x W x 3 RGB images (numpy or tensors, all uint8 or all floating in [0, 1]; sizes may differ). pts3d: per view an (H, W, 3) map,
    masks: per view an (H, W) boolean map; either may instead be the ready padded stack (utils/padded.py) -- the (n, row, 3) tensor of
    `scene.get_pts3d(raw=True)`, the (n, row) tensor of `scene.get_masks(raw=True)` -- and the rest is padded to its rows. Numpy inputs are
    uploaded, device tensors are used where they are.

    Mesh mode: the faces of the reference's `cat_meshes([pts3d_to_trimesh(img, pts, mask) ...])` as uint32 (every vertex of every view is
    kept), a colour per vertex (the mean of the colours of the valid faces that use it; include/dust3r_hip.h d3r_scene_mesh), and every
    view's points as positions. Point-cloud mode: the valid points and their colours, views in order then raster order.

    Returns a dict of host arrays: positions (N, 3) float32, colors (N, 4) uint8 (RGBA), faces (F, 3) uint32 or None, counts (n,) int64 (faces
    or points per view), bounds = (min (3,), max (3,)) float32 of the positions a face uses (mesh) or of the points (NaN components are
    skipped; +inf / -inf where no value is left), None when nothing is valid. The per-view counts are the one host synchronisation.
    With to_host=False the large outputs stay on the device (what the renderer takes): positions (N, 3) float32, colors (N,) int32 packed
    r | g << 8 | b << 16 | 255 << 24, faces (F, 3) int32 as torch tensors; counts and bounds as above."""
    from .utils.device import host_tensor
    _lib.require_device()
    device = torch.device(device)
    n = len(masks)
    if len(imgs) < n or len(pts3d) != n:
        raise ValueError(f'scene_mesh_batch: {len(imgs)} images, {len(pts3d)} pointmaps, {n} masks')
    if n == 0:
        raise ValueError('scene_mesh_batch: no views')
    pts, mask, _, rgb, is_u8, shapes, max_area, hs, ws = ingest_views(imgs[:n], pts3d, masks, None, device, 'scene_mesh_batch')
    areas = [h * w for h, w in shapes]
    n_vert = sum(areas)
    if n_vert >= 2 ** 32:
        raise ValueError(f'scene_mesh_batch: {n_vert} vertices do not fit uint32 indices (as_pointcloud=True or fewer views)')
    n_faces = sum(4 * (h - 1) * (w - 1) for h, w in shapes if h > 1 and w > 1)
    faces = None if as_pointcloud else torch.empty((max(n_faces, 1), 3), dtype=torch.int32, device=device)
    points = torch.empty((n_vert, 3), dtype=torch.float32, device=device) if as_pointcloud else None
    colors = torch.empty((n_vert,), dtype=torch.int32, device=device)
    small = torch.empty((n + 3,), dtype=torch.int64, device=device)       # counts [n] int64, then bounds [6] fp32: one read-back
    work = _lib.workspace(lib.d3r_scene_mesh_workspace_bytes(n, max_area), device)
    with torch.cuda.device(device):
        check(lib.d3r_scene_mesh(n, ptr(pts), ptr(mask), ptr(rgb), int(is_u8), ptr(hs), ptr(ws), max_area, int(bool(as_pointcloud)), ptr(faces),
                                 ptr(points), ptr(colors), ptr(small), ptr(small[n:].view(torch.float32)), ptr(work), current_stream()), 'scene_mesh')
        small = small.cpu()
        counts = small[:n].numpy().copy()
        lo, hi = small[n:].view(torch.float32).numpy()[:3].copy(), small[n:].view(torch.float32).numpy()[3:].copy()
        total = int(counts.sum())
        if as_pointcloud:
            out = dict(positions=points[:total], colors=colors[:total], faces=None)
        else:       # every vertex of every view: the stack itself when no view has padding
            packed = pts.view(n_vert, 3) if n * max_area == n_vert else torch.cat([pts[i, :a] for i, a in enumerate(areas)])
            out = dict(positions=packed, colors=colors, faces=faces[:total])
        if to_host:
            for k, t in out.items():
                if t is not None:
                    out[k] = host_tensor(t.shape, t.dtype)
                    out[k].copy_(t)
            out = dict(positions=out['positions'].numpy(), colors=out['colors'].numpy().view(np.uint8).reshape(-1, 4),
                       faces=None if as_pointcloud else out['faces'].numpy().view(np.uint32))
    return dict(out, counts=counts, bounds=(lo, hi) if total > 0 else None)


# ---- the fused cloud -------------------------------------------------------------------------------------------------------------------
FUSE_MAX_AXIS_BITS = 21         # three axes in one 64-bit key


class FusedCloud:
    """The voxel-fused cloud of `fuse_points` / `scene.fuse()`: positions (M, 3) float32, colors (M, 3) uint8, weight (M,) float32 (the summed
    weights of a voxel's points), count (M,) int32 (their number), in ascending voxel-key order; numpy arrays, or torch tensors on the device
    with to_host=False. voxel_size, origin (3,) float32 (the minimum of the fused points: voxel (i, j, k) starts at origin + voxel_size (i, j,
    k)) and bounds = (min, max) of the fused points, (+inf, -inf) for an empty cloud. After `cluster`: labels (M,) int32, the cluster of every
    point (-1 = noise), and cluster_sizes (C,) int32; they follow the points through estimate_normals, build_tracks, remove_outliers,
    keep_clusters and transform. After `detect_planes`: planes (P, 4) float64 (n, d), plane_sizes (P,) int32 and plane_labels (M,) int32, the
    plane of every point (-1 = none); they follow the points the same way, and `transform` maps the planes. The three are set by
    `detect_planes` or `with_planes`, not by the constructor, whose arguments stay the eleven they were."""

    def __init__(self, positions, colors, weight, count, voxel_size, bounds, normals=None, curvature=None, tracks=None, labels=None, cluster_sizes=None):
        self.positions, self.colors, self.weight, self.count = positions, colors, weight, count
        self.voxel_size = float(voxel_size)
        self.bounds = bounds
        self.origin = bounds[0]
        self.normals, self.curvature = normals, curvature      # (M, 3) float32 and (M,) float32 of `estimate_normals`, else None
        self.tracks = tracks                                   # the `CloudTracks` of `build_tracks`, else None
        self.labels, self.cluster_sizes = labels, cluster_sizes    # (M,) int32 (-1 = noise) and (C,) int32 of `cluster`, else None
        self.planes = self.plane_sizes = self.plane_labels = None  # (P, 4) float64, (P,) int32, (M,) int32 of `detect_planes` / `with_planes`

    PER_POINT = ('positions', 'colors', 'weight', 'count', 'normals', 'curvature', 'labels')      # one row per point: what a subset masks
    PLANE_FIELDS = ('planes', 'plane_sizes', 'plane_labels')   # set after construction; plane_labels is one row per point too (PER_POINT_ROWS)
    PER_POINT_ROWS = PER_POINT + ('plane_labels',)

    def _with(self, **changes):
        """A new cloud with this cloud's fields, the named ones replaced: a deriving method says only what it changes. The attributes ARE the
        constructor's arguments, plus origin, which follows bounds, plus the three plane fields, which are set on the new cloud."""
        apart = ('origin',) + self.PLANE_FIELDS
        fields = {name: value for name, value in vars(self).items() if name not in apart}
        plane_fields = {name: changes.pop(name, getattr(self, name)) for name in self.PLANE_FIELDS}
        out = FusedCloud(**dict(fields, **changes))
        for name, value in plane_fields.items():
            setattr(out, name, value)
        return out

    def with_planes(self, planes, plane_sizes, plane_labels):
        """A new cloud carrying these planes (P, 4), their sizes (P,) and the plane of every point (M,), -1 = none: what `detect_planes`
        attaches, for planes that come from elsewhere (a file, another tool)"""
        if len(plane_labels) != len(self) or len(planes) != len(plane_sizes):
            raise ValueError(f'with_planes: {len(self)} points and {len(plane_labels)} labels, {len(planes)} planes and {len(plane_sizes)} sizes')
        return self._with(planes=np.asarray(planes, np.float64).reshape(-1, 4), plane_sizes=plane_sizes, plane_labels=plane_labels)

    def __len__(self):
        return len(self.positions)

    def save_ply(self, path):
        """Binary little-endian PLY with the per-point confidence (= weight) and count, and the normals when the cloud has them
        (export.write_ply)."""
        from .export import write_ply
        return write_ply(path, *(_to_numpy(a) for a in (self.positions, self.colors, self.weight, self.count)),
                         normals=None if self.normals is None else _to_numpy(self.normals), labels=None if self.labels is None else _to_numpy(self.labels),
                         planes=None if self.plane_labels is None else _to_numpy(self.plane_labels))

    def _neighbour_radius(self, max_dist):
        """max_dist of the neighbour searches: 8 voxels unless given. A surface sampled at spacing v holds about pi r^2 / v^2 points within
        r, so 16 neighbours lie within about 2.3 v: the default leaves a factor of three."""
        if max_dist is not None:
            return float(max_dist)
        if not (math.isfinite(self.voxel_size) and self.voxel_size > 0):
            raise ValueError(f'the cloud has no voxel size ({self.voxel_size!r}): give max_dist')
        return 8.0 * self.voxel_size

    def _subset(self, keep):
        """(cloud, mask) of the points where the device bool tensor `keep` is set: normals, curvature, labels and plane labels are carried
        along (cluster_sizes, planes and plane_sizes too: they still describe the labels), tracks are not. The mask comes back where this
        cloud's arrays are."""
        mask = keep if isinstance(self.positions, torch.Tensor) else keep.cpu().numpy()
        rows = {name: getattr(self, name) for name in self.PER_POINT_ROWS}
        return self._with(tracks=None, **{name: a[mask] for name, a in rows.items() if a is not None}), mask

    @torch.no_grad()
    def cluster(self, eps=None, min_points=10):
        """A new cloud carrying `.labels` (M,) int32 and `.cluster_sizes` (C,) int32: DBSCAN on the GPU (cloud_metrics.cluster_points,
        which has the definition; csrc/cloud_cluster.hip). Label -1 is noise, cluster 0 the largest. eps: the neighbourhood radius,
        default 2.5 voxels. A surface sampled at spacing v holds about pi r^2 / v^2 points within r, so about pi 2.5^2 = 20 within
        2.5 v: twice the default min_points of 10, which leaves room for thinner sampling, while a floater has to come within 2.5
        voxels of the surface to be joined to it. (The room is needed: the voxel size is the MEDIAN pixel footprint, and the 12.6 M-point
        cloud of tools/cloud_cluster_speed.py has 11 neighbours on average, not 20) ValueError for a cloud without a
        voxel size when eps is not given, unless it is empty. The points are the same ones: normals and tracks are kept. Arrays come
        back where this cloud's are."""
        from .cloud_metrics import _min_points, _radius_f32, cluster_points
        _min_points(min_points)
        if eps is None:
            if not (math.isfinite(self.voxel_size) and self.voxel_size > 0):
                if len(self) > 0:
                    raise ValueError(f'the cloud has no voxel size ({self.voxel_size!r}): give eps')
                eps = 1.0                                                  # an empty cloud: any radius gives the same nothing
            else:
                eps = 2.5 * self.voxel_size
        _radius_f32(eps, 'eps')
        res = cluster_points(self, eps, min_points=min_points, to_host=not isinstance(self.positions, torch.Tensor))
        return self._with(labels=res.labels, cluster_sizes=res.sizes)

    def keep_clusters(self, largest=None, min_size=None, labels=None):
        """(cloud, keep) of a clustered cloud (`cluster`), like `remove_outliers`: the points of the chosen clusters, keep (M,) bool.
        Exactly one selector: largest=N, the N largest clusters (labels 0 .. N - 1: the numbering is by decreasing size); min_size=S,
        the clusters of at least S points; labels=[...], those clusters. Noise is never kept. Normals, curvature and labels are carried
        along, cluster_sizes stays as it was (the labels are not renumbered). Tracks are DROPPED, as in `remove_outliers`: they index
        the points before the removal; call `build_tracks` on the result."""
        if sum(x is not None for x in (largest, min_size, labels)) != 1:
            raise ValueError('keep_clusters: give exactly one of largest, min_size, labels')
        if self.labels is None or self.cluster_sizes is None:
            raise ValueError('keep_clusters: the cloud has no labels: call cluster() first')
        n_clusters = len(self.cluster_sizes)
        is_int = lambda x: isinstance(x, (int, np.integer)) and not isinstance(x, bool)      # noqa: E731
        if largest is not None:
            if not is_int(largest) or largest < 0:
                raise ValueError(f'keep_clusters: largest = {largest!r} must be an int >= 0')
            chosen = np.arange(n_clusters) < largest
        elif min_size is not None:
            if not is_int(min_size) or min_size < 1:
                raise ValueError(f'keep_clusters: min_size = {min_size!r} must be an int >= 1')
            chosen = _to_numpy(self.cluster_sizes) >= min_size
        else:
            wanted = np.asarray(list(labels))
            if wanted.size and (wanted.dtype.kind not in 'iu' or wanted.min() < 0 or wanted.max() >= n_clusters):
                raise ValueError(f'keep_clusters: labels {list(labels)!r} are not clusters 0 .. {n_clusters - 1}')
            chosen = np.zeros(n_clusters, bool)
            chosen[wanted.astype(np.int64)] = True
        own = self.labels if isinstance(self.labels, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(self.labels))
        table = torch.from_numpy(np.concatenate([chosen, [False]])).to(own.device)           # the last entry answers label -1
        return self._subset(table[own.long()])

    def colored_by_label(self):
        """A new cloud whose colours are `label_colors` of its labels (what save_ply, SceneViz and the renderer then draw)"""
        if self.labels is None:
            raise ValueError('colored_by_label: the cloud has no labels: call cluster() first')
        colors = label_colors(self.labels)
        if isinstance(self.colors, torch.Tensor):
            colors = torch.from_numpy(colors).to(self.colors.device)
        return self._with(colors=colors)

    @torch.no_grad()
    def estimate_normals(self, k=16, max_dist=None, scene=None, tol=0.05, min_neighbors=3):
        """A new cloud with `normals` (M, 3) float32 and `curvature` (M,) float32, on the GPU (csrc/cloud_knn.hip): per point the k nearest
        other points within max_dist (default 8 voxels; cloud_metrics.k_nearest, exact), the fp64 scatter matrix of the point and those
        neighbours, the unit eigenvector of its smallest eigenvalue l0, curvature = l0 / (l0 + l1 + l2). A point with fewer than
        min_neighbors neighbours gets the zero normal and NaN. Without a scene the sign makes the component of largest magnitude positive;
        with a scene (the aligned scene the cloud was fused from) every normal is turned towards the cameras that see its point:
        visible = it projects onto a pixel whose depth agrees within tol (relative); the vote is weighted by the pixels' confidences, and
        falls back to all cameras for a point no view sees (cloud_metrics.orient_normals). Arrays come back where this cloud's are. The
        points are the same ones, so the cloud's tracks, when it has them, are kept."""
        from .cloud_metrics import _device_of, _points, cloud_normals, default_knn_r0, k_nearest, orient_normals
        on_device = isinstance(self.positions, torch.Tensor)
        device = scene.device if scene is not None and not on_device else _device_of(self)
        P = _points(self, device, 'cloud')
        normals = torch.zeros((len(P), 3), dtype=torch.float32, device=device)
        curvature = torch.full((len(P),), float('nan'), dtype=torch.float32, device=device)
        if len(P) > 0:
            radius = self._neighbour_radius(max_dist)
            _, idx = k_nearest(P, P, k, radius, exclude_self=True, r0=min(default_knn_r0(self, k, radius), radius), to_host=False)
            normals, curvature = cloud_normals(P, P, idx, min_neighbors=min_neighbors)
            if scene is not None:
                heights, widths, _ = scene._shape_tables
                orient_normals(P, normals, scene.get_depthmaps(raw=True), scene._im_conf, scene.get_intrinsics(), scene.get_im_poses(), heights, widths,
                               tol=tol)
        if not on_device:
            normals, curvature = normals.cpu().numpy(), curvature.cpu().numpy()
        return self._with(normals=normals, curvature=curvature)

    @torch.no_grad()
    def remove_outliers(self, k=16, std_ratio=2.0, max_dist=None):
        """(cloud, keep): statistical outlier removal on the GPU. Per point the mean distance to its k nearest other points within max_dist
        (default 8 voxels); a point is kept when it HAS k neighbours within max_dist and its mean is <= mean + std_ratio std of those
        means (cloud_metrics.outlier_threshold: host fp64 from three sums reduced on the device; the fp32 means widened to fp64 for the
        comparison). Open3D's remove_statistical_outlier with the search truncated at max_dist: a point with fewer than k neighbours
        there is an outlier. keep: (M,) bool. Normals, curvature and cluster labels, when present, are carried along. One host synchronisation more
        than `k_nearest` (the three sums). Tracks are DROPPED (they index the points before the removal): call `build_tracks` on the
        result, as `scene.fuse(tracks=True)` does."""
        from .cloud_metrics import _device_of, _points, default_knn_r0, k_nearest, knn_mean_distances, outlier_threshold
        on_device = isinstance(self.positions, torch.Tensor)
        device = _device_of(self)
        P = _points(self, device, 'cloud')
        keep = torch.zeros((len(P),), dtype=torch.bool, device=device)
        if len(P) > 0:
            radius = self._neighbour_radius(max_dist)
            d2, idx = k_nearest(P, P, k, radius, exclude_self=True, r0=min(default_knn_r0(self, k, radius), radius), to_host=False)
            mean, count, sums = knn_mean_distances(d2, idx)
            packed = torch.cat([count.double(), sums]).cpu().tolist()      # one read-back (the count is exact in fp64 below 2^53)
            threshold = outlier_threshold(int(packed[0]), packed[1], packed[2], std_ratio)
            keep = mean.double() <= threshold                              # NaN (fewer than k neighbours, or no full row at all): dropped
        return self._subset(keep)

    @torch.no_grad()
    def transform(self, S):
        """A new cloud moved by the (4, 4) similarity S = [s R | t]: the positions by d3r_cloud_transform (fp32, cloud_metrics.transform_points),
        the normals rotated by R and not renormalised; colours, weights, counts and curvature are kept, voxel_size is multiplied by s and
        the bounds are those of the moved points. The voxel keys are not recomputed: the points keep their order. Arrays come back where
        this cloud's are. The result has no tracks: the scene's cameras no longer see the moved points where the tracks say."""
        from .cloud_metrics import _bounds, _device_of, similarity_parts, transform_points
        scale = similarity_parts(S)[2]
        on_device = isinstance(self.positions, torch.Tensor)
        device = _device_of(self)
        positions, normals, bounds = self.positions, self.normals, self.bounds
        if len(self) > 0:
            positions, normals = transform_points(self.positions, S, normals=self.normals)
            with torch.cuda.device(device):
                lo, hi, n_valid = _bounds(positions, device)
            bounds = (lo, hi) if n_valid > 0 else self.bounds
            if not on_device:
                positions, normals = positions.cpu().numpy(), None if normals is None else normals.cpu().numpy()
        from .cloud_metrics import transform_planes
        planes = None if self.planes is None else transform_planes(self.planes, S)
        return self._with(positions=positions, normals=normals, voxel_size=self.voxel_size * scale, bounds=bounds, tracks=None, planes=planes)

    @torch.no_grad()
    def detect_planes(self, thr=None, max_planes=6, min_inliers=None, min_area2=None, cos_min=None, **kw):
        """A new cloud carrying `.planes` (P, 4) float64, `.plane_sizes` (P,) int32 and `.plane_labels` (M,) int32 (-1 = no plane): the
        dominant planes in extraction order, on the GPU (cloud_metrics.detect_planes, which has the definition; csrc/cloud_planes.hip).
        thr: the inlier distance, default 2 voxels: a fused point is the mean of its voxel's samples, so it lies within about half a
        voxel of the surface plus the depth noise of the views, which the voxel size (the median pixel footprint) is of the order of;
        2 voxels take both in, and two parallel surfaces closer than that were fused into one layer anyway. min_area2: the least
        twice-area of a sampled triangle, default (8 thr)^2: points that err by thr over legs of 8 thr tilt the hypothesis by 7 degrees
        at the most (cloud_metrics._plane_args), and a floor or wall spans hundreds of voxels, so few samples on it are lost.
        cos_min: with it the cloud's normals must agree with the plane's (|cos| >= cos_min; the cloud needs `estimate_normals`).
        min_inliers: default 2 % of the cloud. Further arguments (n_hyp, seed, refine_rounds, normals) go to cloud_metrics.detect_planes.
        ValueError for a cloud without a voxel size when thr is not given, unless it is empty. The points are the same ones: normals,
        labels and tracks are kept. Arrays come back where this cloud's are."""
        from .cloud_metrics import detect_planes
        if thr is None:
            if not (math.isfinite(self.voxel_size) and self.voxel_size > 0):
                if len(self) > 0:
                    raise ValueError(f'the cloud has no voxel size ({self.voxel_size!r}): give thr')
                thr = 1.0                                                  # an empty cloud: any threshold gives the same nothing
            else:
                thr = 2.0 * self.voxel_size
        res = detect_planes(self, thr, max_planes=max_planes, min_inliers=min_inliers, min_area2=min_area2, cos_min=cos_min,
                            to_host=not isinstance(self.positions, torch.Tensor), **kw)
        return self._with(planes=res.planes, plane_sizes=res.plane_sizes, plane_labels=res.plane_labels)

    def _need_planes(self, what):
        if self.planes is None or self.plane_labels is None:
            raise ValueError(f'{what}: the cloud has no planes: call detect_planes() first')

    def remove_planes(self, labels=None):
        """(cloud, keep) of a cloud with planes (`detect_planes`), like `remove_outliers`: the points that lie on none of the planes
        `labels` (default: on no plane at all), keep (M,) bool. planes, plane_sizes and the remaining plane_labels stay as they are
        (nothing is renumbered). Tracks are DROPPED, as in `remove_outliers`."""
        self._need_planes('remove_planes')
        n_planes = len(self.planes)
        gone = np.ones(n_planes, bool)
        if labels is not None:
            wanted = np.asarray(list(labels))
            if wanted.size and (wanted.dtype.kind not in 'iu' or wanted.min() < 0 or wanted.max() >= n_planes):
                raise ValueError(f'remove_planes: labels {list(labels)!r} are not planes 0 .. {n_planes - 1}')
            gone = np.zeros(n_planes, bool)
            gone[wanted.astype(np.int64)] = True
        own = self.plane_labels if isinstance(self.plane_labels, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(self.plane_labels))
        table = torch.from_numpy(np.concatenate([~gone, [True]])).to(own.device)             # the last entry answers label -1
        return self._subset(table[own.long()])

    def upright(self, scene=None, cam_centres=None, thr=None):
        """(cloud, T): the cloud moved by the (4, 4) rigid motion T that stands it on its ground: `cloud_metrics.ground_plane` of the
        detected planes -- the largest that has every camera centre (cam_centres (V, 3), or those of `scene`) on one side at more than thr
        (default 2 voxels) -- then `cloud_metrics.upright_similarity`: the ground's normal goes to (0, 1, 0) by the least rotation, the
        ground to height 0, the cameras to positive heights. ValueError when no plane qualifies. As `transform`, the result has no tracks."""
        from .cloud_metrics import ground_plane, upright_similarity
        self._need_planes('upright')
        if (scene is None) == (cam_centres is None):
            raise ValueError('upright: give exactly one of scene, cam_centres')
        if cam_centres is None:
            cam_centres = _to_numpy(scene.get_im_poses().detach())[:, :3, 3]
        if thr is None:
            thr = 2.0 * self.voxel_size if math.isfinite(self.voxel_size) and self.voxel_size > 0 else 0.0
        ground = ground_plane(self.planes, _to_numpy(self.plane_sizes), cam_centres, thr)
        if ground is None:
            raise ValueError(f'upright: none of the {len(self.planes)} planes has every camera on one side at more than {thr!r}')
        T = upright_similarity(ground)
        return self.transform(T), T

    def colored_by_plane(self):
        """A new cloud whose colours are `label_colors` of its plane labels: grey where there is no plane"""
        self._need_planes('colored_by_plane')
        colors = label_colors(self.plane_labels)
        if isinstance(self.colors, torch.Tensor):
            colors = torch.from_numpy(colors).to(self.colors.device)
        return self._with(colors=colors)

    @torch.no_grad()
    def feature_cloud(self, cell=None):
        """(positions (F, 3), normals (F, 3)) float32: the points a global registration describes (cloud_metrics.feature_cloud, which has
        the definition): of every occupied cell of a grid of side `cell` the point of lowest index, in cell order. cell: default 0.1 of the
        cloud's size, sqrt(trace of the fp64 covariance of its finite points) -- relative to the cloud itself, so the same fraction of any
        rescaled copy. The normals are the cloud's own when it has them (taken as consistently oriented: `estimate_normals(scene=...)`),
        else PCA normals turned away from the feature points' centroid. Arrays come back where this cloud's are."""
        from .cloud_metrics import feature_cloud
        positions, normals, _, _ = feature_cloud(self, cell=cell)
        if not isinstance(self.positions, torch.Tensor):
            positions, normals = positions.cpu().numpy(), normals.cpu().numpy()
        return positions, normals

    def distance_to(self, other, max_dist, to_host=True):
        """(d2, idx) of every point of this cloud in `other` (a FusedCloud or (N, 3) points) within max_dist: squared distances (+inf where
        there is none) and rows of `other` (-1); cloud_metrics.nearest_in_cloud on the GPU."""
        from .cloud_metrics import nearest_in_cloud
        return nearest_in_cloud(self, other, max_dist, to_host=to_host)

    @torch.no_grad()
    def build_tracks(self, scene, max_dist=None, max_error=None, weights='conf'):
        """A new cloud carrying `.tracks` (a `CloudTracks`): which pixel of which image of `scene` (the aligned scene the cloud was fused
        from) observes each point, by projection (`cloud_tracks`; csrc/tracks.hip). max_dist: how far from the point the observing pixel's
        own 3-D point may lie, default the cloud's voxel_size; max_error: observations whose projection lands farther than this many
        pixels from the chosen pixel are dropped (default: none is). weights: 'conf' or None as given to `scene.fuse()`, so that the
        same pixels count as valid. The tracks' arrays come back where this cloud's are."""
        if weights not in ('conf', None):
            raise ValueError(f"build_tracks: weights is 'conf' or None, got {weights!r}")
        if max_dist is None:
            if not (math.isfinite(self.voxel_size) and self.voxel_size > 0):
                if len(self) > 0:
                    raise ValueError(f'the cloud has no voxel size ({self.voxel_size!r}): give max_dist')
                max_dist = 0.0
            else:
                max_dist = self.voxel_size
        tracks = cloud_tracks(self.positions, scene.get_pts3d(raw=True), scene.get_masks(raw=True), scene._im_conf if weights == 'conf' else None,
                              scene.get_intrinsics(), scene.get_im_poses(), scene.imshapes, max_dist, max_error=max_error, device=scene.device,
                              to_host=not isinstance(self.positions, torch.Tensor))
        return self._with(tracks=tracks)


LABEL_PALETTE = np.array([(31, 119, 180), (255, 127, 14), (44, 160, 44), (214, 39, 40), (148, 103, 189), (140, 86, 75), (227, 119, 194), (188, 189, 34),
                          (23, 190, 207), (174, 199, 232), (255, 187, 120), (152, 223, 138), (255, 152, 150), (197, 176, 213), (196, 156, 148),
                          (247, 182, 210), (219, 219, 141), (158, 218, 229), (57, 59, 121), (132, 60, 57)], np.uint8)
LABEL_NOISE_COLOR = (128, 128, 128)


def label_colors(labels):
    """(n, 3) uint8 colours of cluster labels: a fixed palette of 20 by label mod 20, grey for noise (label < 0). Host arithmetic."""
    labels = _to_numpy(labels).astype(np.int64).reshape(-1)
    out = LABEL_PALETTE[np.mod(labels, len(LABEL_PALETTE))]
    out[labels < 0] = LABEL_NOISE_COLOR
    return out


def check_voxel_size(voxel_size):
    """voxel_size as np.float32; ValueError unless it is a normal positive fp32."""
    with np.errstate(over='ignore'):
        v = np.float32(voxel_size)
    if not (np.isfinite(v) and v >= np.finfo(np.float32).tiny):
        raise ValueError(f'voxel_size = {voxel_size!r} must be a normal positive float32')
    return v


def fuse_key_bits(lo, hi, voxel_size):
    """Bits of each axis in the voxel key: max(1, bit_length(floor((hi_c - lo_c) / voxel))), the quotient in float32 exactly as the kernel
    forms it for the farthest point. ValueError when an axis needs more than 21."""
    v = check_voxel_size(voxel_size)
    with np.errstate(over='ignore', invalid='ignore'):
        ext = np.floor((np.asarray(hi, np.float32) - np.asarray(lo, np.float32)) / v)
    if not (np.isfinite(ext).all() and (ext < 2.0 ** FUSE_MAX_AXIS_BITS).all()):
        raise ValueError(f"voxel_size too small for the scene's extent: {voxel_size!r} for points from {np.asarray(lo).tolist()} to "
                         f'{np.asarray(hi).tolist()} (at most 2^{FUSE_MAX_AXIS_BITS} voxels per axis)')
    return [max(1, int(e).bit_length()) for e in ext]


def default_voxel_size(depth, areas, focals):
    """The voxel size of `scene.fuse()` when none is given, the median pixel footprint: the lower median over the views of
    lower_median(depth_i over its h w pixels) / focal_i. depth: the padded (n, row) stack, areas: h w per view, focals (n,) or (n, 2) (fx, fy:
    their mean). torch, on the stack's device."""
    f = torch.as_tensor(focals, dtype=torch.float32, device=depth.device).reshape(len(areas), -1).mean(dim=1)
    per_view = torch.stack([depth[i, :a].median() for i, a in enumerate(areas)]) / f
    return float(per_view.median())


@torch.no_grad()
def fuse_points(imgs, pts3d, masks, weights, voxel_size, device, min_count=1, to_host=True):
    """The views' pointmaps merged into one de-duplicated cloud on the GPU (csrc/fuse.hip): the valid pixels -- mask set, finite point, finite
    weight > 0 -- are binned into voxels of `voxel_size` from the minimum of their bounds, and every voxel becomes one point: the weighted
    mean of its points and of their colours (fp64 sums in view-then-raster order: the same bytes on every run). include/dust3r_hip.h,
    d3r_fuse_bounds / d3r_fuse_voxels.

    imgs, pts3d, masks as for `scene_mesh_batch` (lists of maps, or the ready padded stacks of a scene); weights: per view an (H, W) map, the
    (n, row) stack, or None for ones. voxel_size: a number, or a function without arguments that gives it, called only when some pixel is
    valid (`scene.fuse()`'s default comes from the depth maps; a scene without a valid point has none and needs none). min_count: voxels of
    fewer points are dropped. Returns a `FusedCloud` (empty when nothing is valid). Two host synchronisations: the bounds, then the voxel
    count. ValueError when voxel_size is not a normal positive float32, or too small for the extent (more than 2^21 voxels along an axis)."""
    import ctypes as C
    voxel = np.float32('nan') if callable(voxel_size) else check_voxel_size(voxel_size)
    _lib.require_device()
    device = torch.device(device)
    n = len(masks)
    if len(imgs) < n or len(pts3d) != n or (weights is not None and len(weights) != n):
        raise ValueError(f'fuse_points: {len(imgs)} images, {len(pts3d)} pointmaps, {n} masks, {None if weights is None else len(weights)} weight maps')
    if n == 0:
        raise ValueError('fuse_points: no views')
    pts, mask, wgt, rgb, is_u8, _, row, hs, ws = ingest_views(imgs[:n], pts3d, masks, weights, device, 'fuse_points')
    if n * row >= 2 ** 31:
        raise ValueError(f'fuse_points: {n} rows of {row} do not fit 31-bit pixel indices (fewer views per call)')
    small = torch.empty((4,), dtype=torch.int64, device=device)           # bounds [6] fp32, then the count: one read-back
    work = _lib.workspace(max(1, lib.d3r_fuse_bounds_workspace_bytes(n, row)), device)
    with torch.cuda.device(device):
        check(lib.d3r_fuse_bounds(n, ptr(pts), ptr(mask), ptr(wgt), ptr(hs), ptr(ws), row, ptr(small.view(torch.float32)), ptr(small[3:]), ptr(work),
                                  current_stream()), 'fuse_bounds')
        host = small.cpu()
        lo, hi = host[:3].view(torch.float32).numpy()[:3].copy(), host[:3].view(torch.float32).numpy()[3:].copy()
        n_valid = int(host[3])
        cap = max(n_valid, 1)
        positions = torch.empty((cap, 3), dtype=torch.float32, device=device)
        colors = torch.empty((cap,), dtype=torch.int32, device=device)
        weight = torch.empty((cap,), dtype=torch.float32, device=device)
        count = torch.empty((cap,), dtype=torch.int32, device=device)
        m = 0
        if n_valid > 0:
            if callable(voxel_size):
                voxel = check_voxel_size(voxel_size())
            bits = fuse_key_bits(lo, hi, voxel)                            # raises before anything else is launched
            totals = torch.empty((2,), dtype=torch.int64, device=device)
            work = _lib.workspace(lib.d3r_fuse_voxels_workspace_bytes(n, row, cap), device)
            check(lib.d3r_fuse_voxels(n, ptr(pts), ptr(mask), ptr(wgt), ptr(rgb), int(is_u8), ptr(hs), ptr(ws), row, (C.c_float * 3)(*lo.tolist()),
                                      float(voxel), (C.c_int * 3)(*bits), cap, ptr(positions), ptr(colors), ptr(weight), ptr(count), ptr(totals),
                                      ptr(work), current_stream()), 'fuse_voxels')
            got, m = (int(v) for v in totals.cpu())
            if got != n_valid:
                raise _lib.D3RError(f'fuse_voxels: {got} valid pixels, the bounds pass counted {n_valid}')
        out = [positions[:m], colors[:m].view(torch.uint8).view(m, 4)[:, :3], weight[:m], count[:m]]
        if min_count > 1:
            keep = out[3] >= min_count
            out = [t[keep] for t in out]
        out[1] = out[1].contiguous()
        if to_host:
            out = [t.cpu().numpy() for t in out]
    return FusedCloud(*out, voxel_size=voxel, bounds=(lo, hi))


# ---- 2-D tracks of a cloud -------------------------------------------------------------------------------------------------------------
class CloudTracks:
    """The observations of a cloud's M points in the n images of a scene (`cloud_tracks`; include/dust3r_hip.h, d3r_cloud_tracks_count /
    d3r_cloud_tracks_fill, has the definition). T observations, numpy arrays, or torch tensors on the device with to_host=False:
    point_offsets (M + 1,) int32: point j owns observations [point_offsets[j], point_offsets[j + 1]), its TRACK, in ascending view order;
    view (T,) int32, pixel (T,) int32 (e = y W_view + x), err2 (T,) float64 (the squared distance in pixels between the point's projection
    and that pixel); image_offsets (n + 1,) int32 and image_obs (T,) int32: image v's 2-D points are the observations
    image_obs[image_offsets[v] : image_offsets[v + 1]], in ascending point index; point2d (T,) int32: the position of observation k inside
    its image's list. shapes: the images' (H, W)."""

    def __init__(self, point_offsets, view, pixel, point2d, err2, image_offsets, image_obs, shapes):
        self.point_offsets, self.view, self.pixel, self.point2d, self.err2 = point_offsets, view, pixel, point2d, err2
        self.image_offsets, self.image_obs = image_offsets, image_obs
        self.shapes = [(int(h), int(w)) for h, w in shapes]

    def __len__(self):
        return len(self.view)

    @property
    def n_points(self):
        return len(self.point_offsets) - 1

    @property
    def lengths(self):
        """(M,) the track length of every point"""
        return self.point_offsets[1:] - self.point_offsets[:-1]

    @property
    def point_index(self):
        """(T,) the point of every observation"""
        if isinstance(self.view, torch.Tensor):
            return torch.repeat_interleave(torch.arange(self.n_points, device=self.view.device), self.lengths.long())
        return np.repeat(np.arange(self.n_points), self.lengths)

    def xy(self):
        """(T, 2) the pixel (x, y) of every observation, the integers COLMAP's POINTS2D get (same dtype as `pixel`)"""
        if isinstance(self.view, torch.Tensor):
            widths = torch.tensor([w for _, w in self.shapes], dtype=self.pixel.dtype, device=self.pixel.device)[self.view.long()]
            return torch.stack([self.pixel % widths, torch.div(self.pixel, widths, rounding_mode='floor')], dim=1)
        widths = np.array([w for _, w in self.shapes], dtype=self.pixel.dtype)[self.view]
        return np.stack([self.pixel % widths, self.pixel // widths], axis=1) if len(widths) else np.zeros((0, 2), self.pixel.dtype)

    def point_error(self):
        """(M,) float64: the mean over a point's track of sqrt(err2), COLMAP's per-point error in pixels; -1 for a point without an
        observation. numpy: the sums run in track order (np.bincount); tensors: differences of one cumulative sum (deterministic on
        the device, where an index_add would not be), which may differ from the former in the last bits."""
        lengths = self.lengths
        if isinstance(self.view, torch.Tensor):
            run = torch.cat([torch.zeros(1, dtype=torch.float64, device=self.err2.device), torch.cumsum(torch.sqrt(self.err2), 0)])
            sums = run[self.point_offsets[1:].long()] - run[self.point_offsets[:-1].long()]
            return torch.where(lengths > 0, sums / lengths.clamp(min=1), torch.full_like(sums, -1.0))
        sums = np.bincount(self.point_index, weights=np.sqrt(self.err2), minlength=self.n_points)
        return np.where(lengths > 0, sums / np.maximum(lengths, 1), -1.0)

    def stats(self):
        """dict of plain numbers: observations, mean_track_length (over all points), unobserved (the share of points without an
        observation), mean_error / median_error (sqrt(err2) over the observations, pixels; None without observations) and
        observations_per_image (a list)."""
        err = np.sqrt(_to_numpy(self.err2))
        lengths = _to_numpy(self.lengths)
        per_image = np.diff(_to_numpy(self.image_offsets)).tolist()
        m = max(self.n_points, 1)
        return dict(observations=int(len(err)), mean_track_length=float(len(err) / m), unobserved=float((lengths == 0).sum() / m),
                    mean_error=float(err.mean()) if len(err) else None, median_error=float(np.median(err)) if len(err) else None,
                    observations_per_image=[int(v) for v in per_image])


def track_cameras(intrinsics, cam2world):
    """(n, 16) float64, per view what the tracks project with: the world-to-camera rows R (9, row-major) and t (3) of `export.colmap_pose`
    (the pose exactly as the COLMAP model holds it), then fx, fy, cx, cy of the (n, 3, 3) intrinsics."""
    from .export import colmap_pose, quat_to_rotmat
    K = np.asarray(_to_numpy(intrinsics), dtype=np.float64).reshape(-1, 3, 3)
    c2w = np.asarray(_to_numpy(cam2world), dtype=np.float64).reshape(-1, 4, 4)
    if len(K) != len(c2w):
        raise ValueError(f'track_cameras: {len(K)} intrinsics, {len(c2w)} poses')
    table = np.empty((len(K), 16), dtype=np.float64)
    for i in range(len(K)):
        q, t = colmap_pose(c2w[i])
        table[i, :9], table[i, 9:12] = quat_to_rotmat(q).reshape(9), t
        table[i, 12:] = K[i, 0, 0], K[i, 1, 1], K[i, 0, 2], K[i, 1, 2]
    return table


@torch.no_grad()
def cloud_tracks(positions, pts3d, masks, weights, intrinsics, cam2world, shapes, max_dist, max_error=None, device=None, to_host=True, timing=None):
    """The 2-D tracks of a cloud in the views it was fused from, on the GPU (csrc/tracks.hip): point j is observed in view v at the pixel,
    among the 3 x 3 around its rounded projection, whose own 3-D point is valid (the rule of `fuse_points`) and nearest to it within
    max_dist; the observation carries the squared distance in pixels between the projection and that pixel, and is dropped when that
    exceeds max_error^2. By projection, not voxel membership: at the default voxel size nearly every voxel holds one pixel, so membership
    tracks would have length 1. include/dust3r_hip.h (d3r_cloud_tracks_count) states the rule operation by operation;
    tests/test_tracks_cpu.py restates it in numpy, and the two agree bit for bit.

    positions (M, 3) float32, array or tensor. pts3d, masks, weights: per view the (H, W, 3) / (H, W) maps, or the ready padded stacks of a
    scene; weights may be None. intrinsics (n, 3, 3), cam2world (n, 4, 4) (`track_cameras`), shapes: the views' (H, W). max_dist >= 0,
    squared in float32. Returns a `CloudTracks`. One host synchronisation: the number of observations, to size the outputs. timing
    (optional): a dict that receives the device milliseconds of the two calls under 'count' and 'fill' (tools/tracks_speed.py)."""
    _lib.require_device()
    device = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
    shapes = [(int(h), int(w)) for h, w in shapes]
    n = len(shapes)
    if n == 0 or len(pts3d) != n or len(masks) != n or (weights is not None and len(weights) != n):
        raise ValueError(f'cloud_tracks: {n} shapes, {len(pts3d)} pointmaps, {len(masks)} masks, {None if weights is None else len(weights)} weight maps')
    with np.errstate(over='ignore'):
        r = np.float32(max_dist)
        r2 = r * r
    if not (np.isfinite(r2) and r >= 0):
        raise ValueError(f'cloud_tracks: max_dist = {max_dist!r} must be >= 0 with a finite float32 square')
    if max_error is not None and not float(max_error) >= 0:
        raise ValueError(f'cloud_tracks: max_error = {max_error!r} must be >= 0')
    from .cloud_metrics import _points
    P = _points(positions, device, 'cloud_tracks')
    m = len(P)
    pts, mask, wgt, _, _, _, row, hs, ws = ingest_views(None, pts3d, masks, weights, device, 'cloud_tracks', shapes)
    if n * row >= 2 ** 31:
        raise ValueError(f'cloud_tracks: {n} rows of {row} do not fit 31-bit pixel indices (fewer views per call)')
    cams = torch.from_numpy(track_cameras(intrinsics, cam2world)).to(device)
    if len(cams) != n:
        raise ValueError(f'cloud_tracks: {n} shapes, {len(cams)} cameras')
    thr = (0, 0.0) if max_error is None else (1, float(max_error) ** 2)
    point_off = torch.zeros((m + 1,), dtype=torch.int32, device=device)
    seen = torch.empty((max(m, 1), (n + 31) // 32), dtype=torch.int32, device=device)      # one bit per (point, view), from the first pass to the second
    total = 0
    with torch.cuda.device(device):
        events = [torch.cuda.Event(enable_timing=True) for _ in range(4)] if timing is not None else None
        args = (n, ptr(pts), ptr(mask), ptr(wgt), ptr(hs), ptr(ws), row, m, ptr(P), ptr(cams), float(r2), thr[0], thr[1])
        if m > 0:
            total_dev = torch.empty((1,), dtype=torch.int64, device=device)
            if events:
                events[0].record()
            check(lib.d3r_cloud_tracks_count(*args, ptr(point_off), ptr(seen), ptr(total_dev), current_stream()), 'cloud_tracks_count')
            if events:
                events[1].record()
            total = int(total_dev.cpu())
            if total >= 2 ** 31:
                raise ValueError(f'cloud_tracks: {total} observations do not fit 31-bit indices (fewer points or views per call)')
        cap = max(total, 1)
        view, pixel, point2d, image_obs = (torch.empty((cap,), dtype=torch.int32, device=device) for _ in range(4))
        err2 = torch.empty((cap,), dtype=torch.float64, device=device)
        image_off = torch.zeros((n + 1,), dtype=torch.int32, device=device)
        if m > 0:
            work = _lib.workspace(lib.d3r_cloud_tracks_workspace_bytes(cap), device)
            if events:
                events[2].record()
            check(lib.d3r_cloud_tracks_fill(*args, ptr(point_off), ptr(seen), total, cap, ptr(view), ptr(pixel), ptr(err2), ptr(point2d), ptr(image_off), ptr(image_obs),
                                            ptr(work), current_stream()), 'cloud_tracks_fill')
            if events:
                events[3].record()
                events[3].synchronize()
                timing['count'], timing['fill'] = events[0].elapsed_time(events[1]), events[2].elapsed_time(events[3])
        out = [point_off, view[:total], pixel[:total], point2d[:total], err2[:total], image_off, image_obs[:total]]
        if to_host:
            out = [t.cpu().numpy() for t in out]
    return CloudTracks(*out, shapes=shapes)


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


# ---- headless rendering --------------------------------------------------------------------------------------------------------------
RENDER_GUARD = 8192          # px: the largest frame, and the guard band of the vertex stage (include/dust3r_hip.h d3r_render_*)
ZQ_MAX = 0xFFFFFF


def auto_cam_size(im_poses):
    """The reference's rule (viz.py:115-116): a tenth of the median distance between the camera centres."""
    c = np.asarray(im_poses, dtype=np.float64)[:, :3, 3]
    return 0.1 * float(np.median(np.linalg.norm(c[:, None] - c[None], axis=-1)))


def pack_rgba(color, n=None):
    """Colours as the kernels take them, int32 r | g << 8 | b << 16 | 255 << 24: `color` is (..., 3) uint8, or floating in [0, 1] (converted
    like the GLB export: floor(255 c + 1/2), clamped), numpy or tensor; a single colour is repeated `n` times when `n` is given."""
    t = _tensor(color)
    if t.is_floating_point():
        t = (t.float() * 255 + 0.5).floor().clamp(0, 255)
    t = t.reshape(-1, 3).to(torch.int32)
    if ((t < 0) | (t > 255)).any():
        raise ValueError('colours are 0 ... 255 (integers) or 0 ... 1 (floating)')
    packed = t[:, 0] | (t[:, 1] << 8) | (t[:, 2] << 16) | torch.tensor(-16777216, dtype=torch.int32, device=t.device)
    if n is not None and len(packed) == 1:
        packed = packed.expand(n)
    return packed.contiguous()


def world_to_cam(cam2world):
    """(F, 4, 4) or (4, 4) camera-to-world poses -> (F, 12) float32 rows [R | t] of their inverses, inverted in fp64 on the host."""
    c2w = np.asarray(_to_numpy(cam2world), dtype=np.float64).reshape(-1, 4, 4)
    return np.ascontiguousarray(np.linalg.inv(c2w)[:, :3, :].reshape(-1, 12).astype(np.float32))


def _to_numpy(x):
    return x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)


def intrinsics_rows(focal_or_K, n_cams, size):
    """(F, 4) float32 (fx, fy, cx, cy) from a focal (scalar or one per camera; principal point W/2, H/2 as everywhere in dust3r) or from
    3 x 3 intrinsics (one or F)."""
    W, H = size
    a = np.asarray(_to_numpy(focal_or_K), dtype=np.float64)
    if a.shape[-2:] == (3, 3):
        K = np.broadcast_to(a.reshape(-1, 3, 3), (n_cams, 3, 3)) if a.size == 9 else a.reshape(-1, 3, 3)
        rows = np.stack([K[:, 0, 0], K[:, 1, 1], K[:, 0, 2], K[:, 1, 2]], axis=1)
    else:
        f = np.broadcast_to(a.reshape(-1), (n_cams,)) if a.size == 1 else a.reshape(-1)
        rows = np.stack([f, f, np.full(len(f), W / 2), np.full(len(f), H / 2)], axis=1)
    if rows.shape != (n_cams, 4) or not np.isfinite(rows).all() or (rows[:, :2] <= 0).any():
        raise ValueError(f'intrinsics for {n_cams} cameras: got shape {a.shape} (positive finite focals needed)')
    return np.ascontiguousarray(rows.astype(np.float32))


def _dev(x, device, dtype):
    return None if x is None else _tensor(x).to(device=device, dtype=dtype).contiguous()


@torch.no_grad()
def render_project(positions, w2c, intrinsics, near, device):
    """The vertex stage alone (d3r_render_project): positions (N, 3), w2c (F, 12) or (F, 16) [R | t] rows, intrinsics (F, 4) -> device
    tensors sxy (F, N, 2) int32 in 1/16 pixel and zq (F, N) int64 (0xFFFFFFFF = invalid)."""
    _lib.require_device()
    device = torch.device(device)
    pos = _dev(positions, device, torch.float32).reshape(-1, 3)
    cams = _dev(w2c, device, torch.float32)
    intr = _dev(intrinsics, device, torch.float32)
    F = cams.shape[0]
    if cams.ndim != 2 or cams.shape[1] not in (12, 16) or tuple(intr.shape) != (F, 4) or len(pos) == 0:
        raise ValueError(f'render_project: positions {tuple(pos.shape)}, w2c {tuple(cams.shape)}, intrinsics {tuple(intr.shape)}')
    sxy = torch.empty((F, len(pos), 2), dtype=torch.int32, device=device)
    zq = torch.empty((F, len(pos)), dtype=torch.int32, device=device)
    with torch.cuda.device(device):
        check(lib.d3r_render_project(len(pos), ptr(pos), F, ptr(cams), cams.shape[1], ptr(intr), float(near), ptr(sxy), ptr(zq), current_stream()),
              'render_project')
    return sxy, zq.to(torch.int64) & 0xFFFFFFFF


@torch.no_grad()
def render_batch(cam2world, intrinsics, size, device, points=None, point_colors=None, point_mask=None, vertices=None, faces=None,
                 vertex_colors=None, point_size=1, background=(255, 255, 255), near=0.01, return_depth=False, return_ids=False,
                 return_keys=False, to_host=True, stats=False):
    """F images of one scene in one call of the rasteriser (csrc/render.hip; conventions in include/dust3r_hip.h, d3r_render_*).

    cam2world: (F, 4, 4) camera-to-world poses (OpenCV axes); intrinsics: (F, 4) rows (fx, fy, cx, cy) (`intrinsics_rows`); size = (W, H).
    points (N, 3) with point_colors (N,) packed (`pack_rgba`) and point_mask (N,) or None: drawn as point_size squares, ids 0 ... N - 1.
    vertices (V, 3), faces (M, 3) indices, vertex_colors (V,) packed: drawn as triangles, ids N ... N + M - 1. Numpy inputs are uploaded,
    device tensors are used where they are.

    Returns a dict: rgb (F, H, W, 3) uint8, and on request depth (F, H, W) float32 (inf = background), ids (F, H, W) int32 (-1 =
    background), keys (F, H, W) int64 (the raw frame buffer, (zq << 32) | id, -1 = empty), stats = (candidate samples, atomics issued).
    Host arrays when to_host, else device tensors."""
    W, H = int(size[0]), int(size[1])
    if not (0 < W <= RENDER_GUARD and 0 < H <= RENDER_GUARD):
        raise ValueError(f'render: size (W, H) = {size} must lie in 1 ... {RENDER_GUARD}')
    if not 1 <= int(point_size) <= 16:
        raise ValueError(f'render: point_size {point_size} must lie in 1 ... 16')
    if not (near > 0 and np.isfinite(near)):
        raise ValueError(f'render: near = {near} must be positive and finite')
    _lib.require_device()
    device = torch.device(device)
    cams = torch.from_numpy(world_to_cam(cam2world)).to(device)
    F = cams.shape[0]
    intr = _dev(intrinsics, device, torch.float32)
    if tuple(intr.shape) != (F, 4):
        raise ValueError(f'render: {F} poses, intrinsics of shape {tuple(intr.shape)}')
    n_pts = n_faces = n_vert = 0
    pts = pcol = pmask = verts = fcs = vcol = None
    if points is not None:
        pts = _dev(points, device, torch.float32).reshape(-1, 3)
        n_pts = len(pts)
    if n_pts:
        pcol = _dev(point_colors, device, torch.int32).reshape(-1)
        pmask = None if point_mask is None else _dev(point_mask, device, torch.uint8).reshape(-1)
        if len(pcol) != n_pts or (pmask is not None and len(pmask) != n_pts):
            raise ValueError(f'render: {n_pts} points, {len(pcol)} colours, mask of {None if pmask is None else len(pmask)}')
    if faces is not None and len(faces):
        verts = _dev(vertices, device, torch.float32).reshape(-1, 3)
        fcs = _tensor(faces)
        fcs = (fcs.view(torch.int32) if fcs.dtype == torch.uint32 else fcs.to(torch.int32)).to(device).reshape(-1, 3).contiguous()
        vcol = _dev(vertex_colors, device, torch.int32).reshape(-1)
        n_faces, n_vert = len(fcs), len(verts)
        if len(vcol) != n_vert or n_vert == 0:
            raise ValueError(f'render: {n_vert} vertices, {len(vcol)} colours')
    if n_pts + n_faces >= 2 ** 31:
        raise ValueError(f'render: {n_pts} points + {n_faces} faces do not fit the 31-bit primitive id')
    bg = int(pack_rgba(np.asarray(background, dtype=np.uint8))[0]) & 0xFFFFFFFF
    fb = torch.empty((F, H, W), dtype=torch.int64, device=device)
    rgb = torch.empty((F, H, W, 3), dtype=torch.uint8, device=device)
    depth = torch.empty((F, H, W), dtype=torch.float32, device=device) if return_depth else None
    ids = torch.empty((F, H, W), dtype=torch.int32, device=device) if return_ids else None
    st = torch.zeros((2,), dtype=torch.int64, device=device) if stats else None
    with torch.cuda.device(device):
        stream = current_stream()
        check(lib.d3r_render_clear(F, W, H, ptr(fb), stream), 'render_clear')
        if n_pts:
            check(lib.d3r_render_points(n_pts, ptr(pts), ptr(pmask), 0, F, ptr(cams), 12, ptr(intr), float(near), W, H, int(point_size), ptr(fb),
                                        ptr(st), stream), 'render_points')
        if n_faces:
            check(lib.d3r_render_triangles(n_faces, ptr(fcs), n_vert, ptr(verts), n_pts, F, ptr(cams), 12, ptr(intr), float(near), W, H, ptr(fb),
                                           ptr(st), stream), 'render_triangles')
        check(lib.d3r_render_resolve(F, ptr(cams), 12, ptr(intr), float(near), W, H, ptr(fb), n_pts, 0, ptr(pcol), n_faces, n_pts, ptr(fcs), n_vert,
                                     ptr(verts), ptr(vcol), bg, ptr(rgb), ptr(depth), ptr(ids), stream), 'render_resolve')
    out = dict(rgb=rgb)
    if return_depth:
        out['depth'] = depth
    if return_ids:
        out['ids'] = ids
    if return_keys:
        out['keys'] = fb
    if to_host:
        from .utils.device import host_tensor              # huge pages for the large copies of a many-frame call
        host = {k: host_tensor(v.shape, v.dtype) for k, v in out.items()}
        for k, v in out.items():
            host[k].copy_(v)
        out = {k: v.numpy() for k, v in host.items()}
    if stats:
        out['stats'] = tuple(int(v) for v in st.cpu())
    return out


def look_at(eye, target, down=(0.0, 1.0, 0.0)):
    """Camera-to-world pose (4 x 4, fp64, OpenCV axes: x right, y down, z forward) of a camera at `eye` looking at `target`, its y axis as
    close to `down` as the viewing direction allows."""
    eye, target = np.asarray(eye, dtype=np.float64), np.asarray(target, dtype=np.float64)
    z = target - eye
    if not np.linalg.norm(z) > 0:
        raise ValueError('look_at: eye and target coincide')
    z = z / np.linalg.norm(z)
    d = np.asarray(down, dtype=np.float64)
    x = np.cross(d, z)
    if np.linalg.norm(x) < 1e-9:                          # looking along `down`: any perpendicular will do
        x = np.cross(np.roll(d, 1) + np.array([0.3, 0.5, 0.7]), z)
    x = x / np.linalg.norm(x)
    y = np.cross(z, x)
    pose = np.eye(4)
    pose[:3, 0], pose[:3, 1], pose[:3, 2], pose[:3, 3] = x, y, z, eye
    return pose


def fit_distance(radius, focal, size, margin=1.1):
    """How far from the centre of a sphere of `radius` a camera of `focal` and size (W, H) stands so that the sphere fits the frame with
    `margin`: radius margin / sin(half the smaller field of view)."""
    half = np.arctan(min(size) / (2.0 * float(focal)))
    return float(radius) * margin / np.sin(half)


def default_viewpoint(cam2world0, bounds, focal, size):
    """The viewpoint of `SceneViz.show()`: the first camera's orientation, looking at the centre of the bounds, pulled back ALONG ITS OWN
    AXIS until the bounding sphere (centre = mid point of `bounds`, radius = half their diagonal) fits the frame (`fit_distance`). Without
    a camera: looking along +z with y down. Returns the 4 x 4 camera-to-world pose (fp64)."""
    lo, hi = np.asarray(bounds[0], dtype=np.float64), np.asarray(bounds[1], dtype=np.float64)
    centre, radius = (lo + hi) / 2, max(float(np.linalg.norm(hi - lo)) / 2, 1e-6)
    pose = np.eye(4) if cam2world0 is None else np.array(_to_numpy(cam2world0), dtype=np.float64).reshape(4, 4)
    pose[:3, 3] = centre - fit_distance(radius, focal, size) * pose[:3, 2]
    return pose


def turntable_poses(bounds, n_frames, focal, size, down=(0.0, 1.0, 0.0), elevation_deg=20.0):
    """n_frames camera-to-world poses (n, 4, 4) fp64 on a circle about the axis `down` through the centre of `bounds`, raised by
    `elevation_deg` against `down`, at the distance where the bounding sphere fits the frame (`fit_distance`), each looking at the centre."""
    if n_frames < 1:
        raise ValueError(f'turntable_poses: n_frames = {n_frames}')
    lo, hi = np.asarray(bounds[0], dtype=np.float64), np.asarray(bounds[1], dtype=np.float64)
    centre, radius = (lo + hi) / 2, max(float(np.linalg.norm(hi - lo)) / 2, 1e-6)
    d = np.asarray(down, dtype=np.float64)
    d = d / np.linalg.norm(d)
    a = np.cross(d, [1.0, 0.0, 0.0])
    if np.linalg.norm(a) < 1e-6:
        a = np.cross(d, [0.0, 0.0, 1.0])
    a = a / np.linalg.norm(a)
    b = np.cross(d, a)
    dist, el = fit_distance(radius, focal, size), np.deg2rad(elevation_deg)
    poses = []
    for k in range(n_frames):
        t = 2 * np.pi * k / n_frames
        eye = centre + dist * (np.cos(el) * (np.cos(t) * a + np.sin(t) * b) - np.sin(el) * d)
        poses.append(look_at(eye, centre, down=d))
    return np.stack(poses)


class SceneViz:
    """The reference's SceneViz (viz.py:119-209) without a window: the same `add_pointcloud`, `add_camera`, `add_cameras`, and
    `render(...)` / `show(outfile=None, ...)` that draw the scene into images on the GPU (`render_batch`). Geometry is kept as it is given
    (device tensors stay on their device) and joined at the first render. Cameras are drawn as the wire glyph of `scene_camera_geometry`
    in a flat colour; the textured image quad of the reference's glyph is out of scope, `image` / `images` only give the size."""

    def __init__(self, device=None):
        self.device = None if device is None else torch.device(device)
        self._points, self._colors, self._masks = [], [], []
        self._verts, self._faces, self._vcolors = [], [], []
        self._n_vert = 0
        self.cam_poses, self.cam_focals = [], []
        self._joined = None
        self.image = None            # the last picture of show()

    # ---- geometry
    def add_pointcloud(self, pts3d, color=(0, 0, 0), mask=None):
        """pts3d: one (..., 3) map or a list of them; color: one (r, g, b) tuple for all, an image (same pixel count) or a list of images
        (uint8, or floating in [0, 1]); mask: None, one boolean map or a list."""
        if not isinstance(pts3d, (list, tuple)):
            pts3d = [pts3d]
            mask = None if mask is None else [mask]
            color = color if isinstance(color, (tuple, list)) else [color]
        elif isinstance(pts3d, tuple):
            pts3d = list(pts3d)
        flat = isinstance(color, tuple) or (isinstance(color, list) and len(color) == 3 and np.ndim(color[0]) == 0)
        if flat and len(color) != 3:
            raise ValueError(f'add_pointcloud: a colour is (r, g, b), got {color}')
        if not flat and len(color) != len(pts3d):
            raise ValueError(f'add_pointcloud: {len(pts3d)} pointmaps, {len(color)} colour images')
        if mask is not None and len(mask) != len(pts3d):
            raise ValueError(f'add_pointcloud: {len(pts3d)} pointmaps, {len(mask)} masks')
        for k, p in enumerate(pts3d):
            p = _tensor(p).reshape(-1, 3)
            if self.device is None and p.is_cuda:
                self.device = p.device
            c = pack_rgba(np.asarray(color, dtype=np.uint8), len(p)) if flat else pack_rgba(color[k])
            if len(c) != len(p):
                raise ValueError(f'add_pointcloud: pointmap {k} has {len(p)} points, its colours {len(c)}')
            m = None if mask is None or mask[k] is None else _tensor(mask[k]).reshape(-1)
            if m is not None and len(m) != len(p):
                raise ValueError(f'add_pointcloud: pointmap {k} has {len(p)} points, its mask {len(m)}')
            self._points.append(p)
            self._colors.append(c)
            self._masks.append(m)
        self._joined = None
        return self

    def add_mesh(self, vertices, faces, colors):
        """Triangles: vertices (V, 3), faces (M, 3) indices, colors one (r, g, b), (V, 3) / (V, 4) per vertex, or (V,) int32 already packed
        (`pack_rgba`; what `scene_mesh_batch(..., to_host=False)` gives). Tensors stay on their device. Vertices that no face uses (the
        export's mesh keeps every pixel of every view, masked or not) are never drawn and do not count for `bounds()`."""
        v = _tensor(vertices).reshape(-1, 3)
        f = _tensor(faces)
        f = (f.view(torch.int32) if f.dtype == torch.uint32 else f).reshape(-1, 3)
        if len(f) and (int(f.min()) < 0 or int(f.max()) >= len(v)):
            raise ValueError(f'add_mesh: face indices outside 0 ... {len(v) - 1}')
        if self._n_vert + len(v) >= 2 ** 31:
            raise ValueError('add_mesh: more than 2^31 vertices')
        col = _tensor(colors)
        if col.ndim == 1 and col.dtype == torch.int32 and len(col) == len(v):
            c = col.contiguous()
        else:
            c = pack_rgba(col, len(v)) if col.numel() == 3 else pack_rgba(col.reshape(len(v), -1)[:, :3])
        if self.device is None and v.is_cuda:
            self.device = v.device
        self._verts.append(v)
        self._faces.append(f.to(torch.int32) + self._n_vert)
        self._vcolors.append(c)
        self._n_vert += len(v)
        self._joined = None
        return self

    def add_camera(self, pose_c2w, focal=None, color=(0, 0, 0), image=None, imsize=None, cam_size=0.03):
        pose = np.asarray(_to_numpy(pose_c2w), dtype=np.float64).reshape(4, 4)
        focal = None if focal is None else _to_numpy(focal)
        if isinstance(focal, np.ndarray) and focal.shape == (3, 3):
            if imsize is None:
                imsize = (2 * focal[0, 2], 2 * focal[1, 2])
            focal = (focal[0, 0] * focal[1, 1]) ** 0.5
        if imsize is None:
            if image is None:
                raise ValueError('add_camera: give imsize (W, H), an image, or 3 x 3 intrinsics')
            imsize = tuple(image.shape[1::-1])
        if focal is not None:
            focal = float(np.asarray(focal).reshape(-1)[0])
        cam = scene_camera_geometry(pose, focal, (float(imsize[0]), float(imsize[1])), screen_width=cam_size)
        self.add_mesh(cam['wire_vertices'].astype(np.float32), cam['wire_faces'], np.asarray(color if color is not None else (0, 0, 0), dtype=np.uint8))
        self.cam_poses.append(pose)
        self.cam_focals.append(focal)
        return self

    def add_cameras(self, poses, focals=None, images=None, imsizes=None, colors=None, cam_size=0.03, color=None):
        def get(arr, idx):
            return None if arr is None else arr[idx]
        for i, pose_c2w in enumerate(poses):
            c = get(colors, i) if colors is not None else color
            self.add_camera(pose_c2w, get(focals, i), image=get(images, i), color=(0, 0, 0) if c is None else c, imsize=get(imsizes, i),
                            cam_size=cam_size)
        return self

    # ---- flat arrays
    def _device(self):
        if self.device is None:
            _lib.require_device()
            self.device = torch.device('cuda', torch.cuda.current_device())
        return self.device

    def flat_arrays(self, device=None):
        """Everything added so far as the flat tables of `render_batch`: dict(points (N, 3) fp32, point_colors (N,) int32, point_mask (N,)
        uint8 or None, vertices (V, 3), faces (M, 3) int32, vertex_colors (V,)), on `device` (default: the scene's GPU)."""
        device = torch.device(device) if device is not None else self._device()
        out = dict(points=None, point_colors=None, point_mask=None, vertices=None, faces=None, vertex_colors=None)
        if self._points:
            out['points'] = torch.cat([p.to(device=device, dtype=torch.float32) for p in self._points])
            out['point_colors'] = torch.cat([c.to(device) for c in self._colors])
            if any(m is not None for m in self._masks):
                out['point_mask'] = torch.cat([torch.ones(len(p), dtype=torch.uint8, device=device) if m is None else (m.to(device) != 0).to(torch.uint8)
                                               for p, m in zip(self._points, self._masks)])
        if self._verts:
            out['vertices'] = torch.cat([v.to(device=device, dtype=torch.float32) for v in self._verts])
            out['faces'] = torch.cat([f.to(device) for f in self._faces])
            out['vertex_colors'] = torch.cat([c.to(device) for c in self._vcolors])
        return out

    def bounds(self):
        """(min (3,), max (3,)) fp64 over what can be drawn: the finite unmasked points and the finite mesh vertices that a face uses (a
        masked-out point or an unused vertex, however far away, moves neither the framing nor the default near plane); None for an empty scene."""
        g = self._geometry()
        sets = []
        if g['points'] is not None:
            p = g['points'] if g['point_mask'] is None else g['points'][g['point_mask'] != 0]
            sets.append(p)
        if g['vertices'] is not None:
            used = torch.zeros(len(g['vertices']), dtype=torch.bool, device=g['vertices'].device)
            used[g['faces'].reshape(-1).long()] = True
            sets.append(g['vertices'][used])
        sets = [p[torch.isfinite(p).all(dim=1)] for p in sets]
        sets = [p for p in sets if len(p)]
        if not sets:
            return None
        lo = torch.stack([p.min(dim=0).values for p in sets]).min(dim=0).values
        hi = torch.stack([p.max(dim=0).values for p in sets]).max(dim=0).values
        return lo.double().cpu().numpy(), hi.double().cpu().numpy()

    def _geometry(self):
        if self._joined is None:
            self._joined = self.flat_arrays()
        return self._joined

    # ---- drawing
    def render(self, cam2world, focal, size=(1024, 768), point_size=1, background=(255, 255, 255), near=None, return_depth=False,
               return_ids=False, to_host=True):
        """The scene seen from one camera-to-world pose (4, 4) or a stack of F poses (F, 4, 4), all frames in one call. `focal`: a focal in
        pixels (principal point W/2, H/2; one value or one per pose) or 3 x 3 intrinsics K (one or F). size = (W, H). near: the near plane
        (geometry not beyond it is not drawn; depth keeps 24 bits of near / Z); default 1 % of the diagonal of the scene's bounds.
        Returns the image (H, W, 3) uint8 -- (F, H, W, 3) for a stack -- or, with return_depth / return_ids, the dict of `render_batch`."""
        poses = _to_numpy(cam2world)
        single = poses.ndim == 2
        poses = poses.reshape(-1, 4, 4)
        g = self._geometry()
        if near is None:
            near = self.default_near()
        out = render_batch(poses, intrinsics_rows(focal, len(poses), size), size, self._device(), point_size=point_size, background=background,
                           near=near, return_depth=return_depth, return_ids=return_ids, to_host=to_host, **g)
        if single:
            out = {k: v[0] for k, v in out.items()}
        return out if (return_depth or return_ids) else out['rgb']

    def default_near(self):
        """The near plane `render` uses when none is given: 1 % of the diagonal of `bounds()` (0.01 for an empty or point-sized scene)."""
        b = self.bounds()
        near = 0.01 * float(np.linalg.norm(b[1] - b[0])) if b is not None else 0.01
        return near if near > 0 else 0.01

    def default_view(self, size=(1024, 768), focal=None):
        """(pose, focal) of `show()`: the rule of `default_viewpoint` with the first camera added to the scene (its focal unless one is
        given; 1.1 min(W, H) -- dust3r's default guess -- when it has none)."""
        b = self.bounds()
        if b is None:
            raise ValueError('SceneViz: nothing to show (no finite point or vertex)')
        if focal is None:
            focal = self.cam_focals[0] if self.cam_focals and self.cam_focals[0] else 1.1 * min(size)
        return default_viewpoint(self.cam_poses[0] if self.cam_poses else None, b, focal, size), float(focal)

    def show(self, outfile=None, point_size=2, size=(1024, 768), focal=None, cam2world=None, **render_kw):
        """Never opens a window: renders one image from `cam2world` (default: `default_view`), writes it as a PNG when `outfile` is given,
        and returns it as an (H, W, 3) uint8 array, also kept as `self.image`. point_size = 2 is the reference's default."""
        pose, f = self.default_view(size, focal) if cam2world is None else (cam2world, focal if focal is not None else 1.1 * min(size))
        image = self.render(pose, f, size=size, point_size=point_size, **render_kw)
        if isinstance(image, dict):
            image = image['rgb']
        if outfile is not None:
            from .demo import _png
            with open(outfile, 'wb') as fh:
                fh.write(_png(np.asarray(image)))
        self.image = image
        return image
