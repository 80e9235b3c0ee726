"""Global alignment -- host-side mirror of the reference `dust3r/cloud_opt/base_opt.py`
(`BasePCOptimizer`, `global_alignment_loop`).

Same constructor keywords, attributes (`edges, imshapes, imsizes, im_conf, pred_i, pred_j, conf_i,
conf_j, pw_poses, pw_adaptors, min_conf_thr, conf_trf, is_symmetrized, n_imgs, n_edges,
str_edges`), getters, `compute_global_alignment(init, niter_PnP, lr, niter, schedule, lr_min)`, `clean_pointcloud()` and
`mask_sky()`.
What differs is WHERE the optimisation runs: the reference builds an autograd graph of ~25 kernels
per iteration and steps torch.optim.Adam (base_opt.py:326-366); here `global_alignment_loop` hands
the parameter tensors to the fused HIP aligner (csrc/aligner.hip, C ABI `d3r_aligner_*`), which
updates them in place. There is no CPU execution path for the loop.
"""
import copy
import ctypes as C

import numpy as np
import torch
import torch.nn as nn
import tqdm

from .. import _lib
from .._lib import check, current_stream, lib, ptr
from ..utils.geometry import geotrf, inv, xy_grid
from ..utils.padded import pad_views, shape_tables, split_views, zero_padding_
from ..utils.rigid import quat_translation_to_homogeneous, rotmat_to_unitquat
from . import init_im_poses as init_fun
from .commons import (cosine_schedule, edge_str, get_conf_trf, get_imshapes, linear_schedule, signed_expm1,
                      signed_log1p)


class _EdgeView:
    """dict-like access `view['i_j'] -> (H, W, ...)` into a stacked (E, max_area, ...) tensor."""

    def __init__(self, owner, attr, side):
        self._o, self._attr, self._side = owner, attr, side

    def _index(self, key):
        return self._o._edge_index[key]

    def __getitem__(self, key):
        e = self._index(key)
        i, j = self._o.edges[e]
        h, w = self._o.imshapes[i if self._side == 0 else j]
        t = getattr(self._o, self._attr)[e]
        return t[:h * w].view((h, w) + tuple(t.shape[1:]))

    def __contains__(self, key):
        return key in self._o._edge_index

    def keys(self):
        return self._o._edge_index.keys()

    def items(self):
        return [(k, self[k]) for k in self.keys()]

    def values(self):
        return [self[k] for k in self.keys()]

    def __len__(self):
        return len(self._o._edge_index)


class BasePCOptimizer(nn.Module):
    """Optimize a global scene given pairwise observations. Nodes: images; edges: (pred1, pred2)."""

    def __init__(self, *args, **kwargs):
        super().__init__()
        self._init_from_views(*args, **kwargs)

    def _init_from_views(self, view1, view2, pred1, pred2, dist='l1', conf='log', min_conf_thr=3, base_scale=0.5,
                         allow_pw_adaptors=False, pw_break=20, rand_pose=torch.randn, iterationsCount=None, verbose=True):
        if dist not in ('l1', 'l2'):
            raise KeyError(dist)
        if not isinstance(view1['idx'], list):
            view1['idx'] = view1['idx'].tolist()
        if not isinstance(view2['idx'], list):
            view2['idx'] = view2['idx'].tolist()
        self.edges = [(int(i), int(j)) for i, j in zip(view1['idx'], view2['idx'])]
        self.is_symmetrized = set(self.edges) == {(j, i) for i, j in self.edges}
        self.dist_name = dist
        self.verbose = verbose
        self.n_imgs = self._check_edges()
        self._edge_index = {edge_str(i, j): e for e, (i, j) in enumerate(self.edges)}

        pred1_pts, pred2_pts = pred1['pts3d'], pred2['pts3d_in_other_view']
        pred1_conf, pred2_conf = pred1['conf'], pred2['conf']
        self.imshapes = get_imshapes(self.edges, pred1_pts, pred2_pts)
        im_areas = [h * w for h, w in self.imshapes]
        self.max_area = max(im_areas)
        assert all(a % 4 == 0 for a in im_areas), 'image areas must be multiples of 4'

        def stack(seq):
            if isinstance(seq, torch.Tensor) and seq.shape[1] * seq.shape[2] == self.max_area:
                return seq.detach().float().reshape((seq.shape[0], self.max_area) + tuple(seq.shape[3:])).contiguous()
            first = torch.as_tensor(seq[0])
            return pad_views(seq, first.device, torch.float32, tail=first.shape[2:], row=self.max_area)

        self.register_buffer('_stacked_pred_i', stack(pred1_pts))
        self.register_buffer('_stacked_pred_j', stack(pred2_pts))
        self.register_buffer('_conf_i', stack(pred1_conf))
        self.register_buffer('_conf_j', stack(pred2_conf))
        self.pred_i, self.pred_j = _EdgeView(self, '_stacked_pred_i', 0), _EdgeView(self, '_stacked_pred_j', 1)
        self.conf_i, self.conf_j = _EdgeView(self, '_conf_i', 0), _EdgeView(self, '_conf_j', 1)

        self.min_conf_thr = min_conf_thr
        self.conf_mode = conf
        self.conf_trf = get_conf_trf(conf)
        self.register_buffer('_im_conf', torch.zeros((self.n_imgs, self.max_area), dtype=torch.float32, device=self._conf_i.device))
        self._compute_img_conf()

        # pre-computed pixel weights (zero in the padding, like ParameterStack(fill=max_area))
        def weights(c, side):
            w = self.conf_trf(c.clamp_min(1e-30)) if conf == 'log' else self.conf_trf(c)
            return zero_padding_(w, [im_areas[edge[side]] for edge in self.edges]).contiguous()
        self.register_buffer('_weight_i', weights(self._conf_i.clone(), 0))
        self.register_buffer('_weight_j', weights(self._conf_j.clone(), 1))

        self.base_scale = base_scale
        self.norm_pw_scale = True
        self.pw_break = pw_break
        self.POSE_DIM = 7
        self.pw_poses = nn.Parameter(rand_pose((self.n_edges, 1 + self.POSE_DIM)).float())
        self.pw_adaptors = nn.Parameter(torch.zeros((self.n_edges, 2)), requires_grad=bool(allow_pw_adaptors))     # base_opt.py:92
        self.has_im_poses = False
        self.rand_pose = rand_pose

        self.imgs = None
        if 'img' in view1 and 'img' in view2:
            from ..utils.image import rgb
            imgs = [torch.zeros((3,) + hw) for hw in self.imshapes]
            for v in range(len(self.edges)):
                imgs[view1['idx'][v]] = view1['img'][v]
                imgs[view2['idx'][v]] = view2['img'][v]
            self.imgs = rgb(imgs)
        self._grid_cache = None        # (n, max_area, 2) pixel grid of depth_to_pts3d, built on first use on the scene's device
        self._tables_cache = None      # (heights, widths, npix) int32 on the scene's device, likewise
        self._engine = None
        self._engine_sig = None

    # ------------------------------------------------------------------ bookkeeping
    @property
    def n_edges(self):
        return len(self.edges)

    @property
    def str_edges(self):
        return [edge_str(i, j) for i, j in self.edges]

    @property
    def imsizes(self):
        return [(w, h) for h, w in self.imshapes]

    @property
    def device(self):
        return self.pw_poses.device

    def _check_edges(self):
        indices = sorted({i for edge in self.edges for i in edge})
        assert indices == list(range(len(indices))), 'bad pair indices: missing values '
        return len(indices)

    @torch.no_grad()
    def _compute_img_conf(self):
        """Per image, the pixel-wise maximum of the confidences of every edge side that shows it (base_opt.py:116-123 of the reference):
        two scatter-max passes over the stacked (E, max_area) confidences instead of 2 E small launches, into the `_im_conf` stack."""
        dev = self._conf_i.device
        ei = torch.tensor([i for i, j in self.edges], device=dev)
        ej = torch.tensor([j for i, j in self.edges], device=dev)
        self._im_conf.zero_()
        self._im_conf.index_reduce_(0, ei, self._conf_i, 'amax', include_self=True)
        self._im_conf.index_reduce_(0, ej, self._conf_j, 'amax', include_self=True)

    @property
    def im_conf(self):
        """The reference's list of (H, W) confidence maps: views of the `_im_conf` stack, so `scene.im_conf[i][...] = x` writes to the scene."""
        return split_views(self._im_conf, self.imshapes)

    @im_conf.setter
    @torch.no_grad()
    def im_conf(self, maps):
        """`scene.im_conf = maps` copies the maps into the scene's stack (it does not keep the caller's tensors)."""
        for dst, src in zip(self.im_conf, maps, strict=True):
            dst.copy_(torch.as_tensor(src))

    _TRAINABLE_KEYS = ('pw_poses', 'pw_adaptors', 'im_depthmaps', 'im_poses', 'im_focals', 'im_pp')

    def state_dict(self, trainable=True):
        if trainable:
            out = {k: getattr(self, k).detach().clone() for k in self._TRAINABLE_KEYS if hasattr(self, k)}
            out.update({f'im_conf.{i}': c.clone() for i, c in enumerate(self.im_conf)})
            return out
        return {k: getattr(self, k) for k in ('_stacked_pred_i', '_stacked_pred_j', '_weight_i', '_weight_j')}

    @torch.no_grad()
    def load_state_dict(self, data, **kw):
        for k, v in data.items():
            if k in self._TRAINABLE_KEYS and hasattr(self, k):
                getattr(self, k).data.copy_(torch.as_tensor(v).to(getattr(self, k).device).reshape(getattr(self, k).shape))
            elif k.startswith('im_conf.'):
                self.im_conf[int(k.split('.')[1])].copy_(torch.as_tensor(v))
        return self

    def to(self, device, *a, **k):
        self._destroy_engine()
        return super().to(device, *a, **k)

    # ------------------------------------------------------------------ parameter access (cam-to-world)
    def get_adaptors(self):
        adapt = self.pw_adaptors
        adapt = torch.cat((adapt[:, 0:1], adapt), dim=-1)
        if self.norm_pw_scale:
            adapt = adapt - adapt.mean(dim=1, keepdim=True)
        return (adapt / self.pw_break).exp()

    def _get_poses(self, poses):
        return quat_translation_to_homogeneous(poses[:, :4], signed_expm1(poses[:, 4:7]))

    def _set_pose(self, poses, idx, R, T=None, scale=None, force=False):
        pose = poses[idx]
        if not (poses.requires_grad or force):
            return pose
        if R is not None and tuple(R.shape) == (4, 4):
            assert T is None
            T, R = R[:3, 3], R[:3, :3]
        with torch.no_grad():
            if R is not None:
                poses.data[idx, 0:4] = rotmat_to_unitquat(torch.as_tensor(R).float()).to(poses.device)
            if T is not None:
                poses.data[idx, 4:7] = signed_log1p(torch.as_tensor(T).float().to(poses.device) / (scale or 1))
            if scale is not None:
                assert poses.shape[-1] in (8, 13)
                poses.data[idx, -1] = float(np.log(float(scale)))
        return pose

    def get_pw_norm_scale_factor(self):
        if self.norm_pw_scale:
            return (np.log(self.base_scale) - self.pw_poses[:, -1].mean()).exp()
        return 1

    def get_pw_scale(self):
        return self.pw_poses[:, -1].exp() * self.get_pw_norm_scale_factor()

    def get_pw_poses(self):
        RT = self._get_poses(self.pw_poses)
        scaled = RT.clone()
        scaled[:, :3] *= self.get_pw_scale().view(-1, 1, 1)
        return scaled

    def get_masks(self, raw=False):
        masks = self._im_conf > self.min_conf_thr           # raw (new): the padded (n, max_area) stack the (H, W) masks are views of
        return masks if raw else split_views(masks, self.imshapes)

    def get_conf(self, mode=None):
        trf = self.conf_trf if mode is None else get_conf_trf(mode)
        return [trf(c) for c in self.im_conf]

    def get_pts3d(self, raw=False):
        res = self.depth_to_pts3d()
        return res if raw else split_views(res, self.imshapes)

    # ------------------------------------------------------------------ image parameters
    # A scene with image parameters keeps them in flat storage -- `_flat_im_poses` (n, 7), `_flat_im_depthmaps` (n, max_area) log-depth, zero in the
    # padding, `_flat_im_focals` (n, 1 | 2) = focal_break * log f, `_flat_im_pp` (n, 2) -- beside `focal_break` and the buffer `_pp` (n, 2) of image
    # centres; the getters and the engine binding below read these and nothing else of the scene class.
    def _get_msk_indices(self, msk):
        if msk is None:
            return range(self.n_imgs)
        if isinstance(msk, int):
            return [msk]
        if isinstance(msk, (tuple, list)):
            return self._get_msk_indices(np.array(msk))
        if msk.dtype in (bool, torch.bool, np.bool_):
            assert len(msk) == self.n_imgs
            return np.where(msk)[0]
        if np.issubdtype(msk.dtype, np.integer):
            return msk
        raise ValueError(f'bad {msk=}')

    def get_focals(self):
        """(n, 1), or (n, 2) = (fx, fy) for a scene with two focals per image."""
        return (self._flat_im_focals / self.focal_break).exp()

    def get_principal_points(self):
        return self._pp + 10 * self._flat_im_pp

    def get_intrinsics(self):
        K = torch.zeros((self.n_imgs, 3, 3), device=self.device)
        focals = self.get_focals().view(self.n_imgs, -1)
        K[:, 0, 0] = focals[:, 0]
        K[:, 1, 1] = focals[:, -1]
        K[:, :2, 2] = self.get_principal_points()
        K[:, 2, 2] = 1
        return K

    def get_im_poses(self):  # cam to world
        return self._get_poses(self._flat_im_poses)

    def get_depthmaps(self, raw=False):
        res = self._flat_im_depthmaps.exp()
        return res if raw else split_views(res, self.imshapes)

    @property
    def _grid(self):
        g = self._grid_cache
        if g is None or g.device != self.device:
            dev = self.device
            per_shape = {hw: xy_grid(hw[1], hw[0], device=dev) for hw in set(self.imshapes)}
            g = self._grid_cache = pad_views([per_shape[hw] for hw in self.imshapes], dev, torch.float32, tail=(2,), row=self.max_area)
        return g

    @property
    def _shape_tables(self):
        """(heights, widths, npix): the int32 tables the batched kernels take beside a stack, on the scene's device."""
        if self._tables_cache is None or self._tables_cache[0].device != self.device:
            self._tables_cache = shape_tables(self.imshapes, self.device)
        return self._tables_cache

    def depth_to_pts3d(self):
        focals = self.get_focals().unsqueeze(1)                 # (n,1,1 | 2): x = d (u - cx) / fx, y = d (v - cy) / fy
        pp = self.get_principal_points().unsqueeze(1)           # (n,1,2)
        depth = self.get_depthmaps(raw=True).unsqueeze(-1)      # (n,A,1)
        rel = torch.cat((depth * (self._grid - pp) / focals, depth), dim=-1)
        return geotrf(self.get_im_poses(), rel)

    @torch.no_grad()
    def clean_pointcloud(self, **kw):
        if self.device.type != 'cuda':
            raise _lib.D3RError('clean_pointcloud runs on the GPU (dust3r_amd has no CPU execution path)')
        heights, widths, _ = self._shape_tables
        _clean_stacks(self._im_conf, self.get_depthmaps(raw=True), self.get_pts3d(raw=True), self.get_intrinsics(), inv(self.get_im_poses()),
                      heights, widths, tol=kw.get('tol', 0.001), bad_conf=kw.get('bad_conf', 0))
        return self

    @torch.no_grad()
    def mask_sky(self):
        """The reference's mask_sky (base_opt.py:290-295): a copy of the scene whose im_conf is zero on the sky of each image
        (viz.segment_sky, all images in one GPU call). The scene itself is left untouched."""
        if self.imgs is None:
            raise ValueError('mask_sky needs the scene images: scene.imgs is None (the views given to global_aligner had no "img")')
        if self.device.type != 'cuda':
            raise _lib.D3RError('mask_sky runs on the GPU (dust3r_amd has no CPU execution path)')
        from ..viz import segment_sky_batch
        skies = segment_sky_batch(self.imgs, self.device)
        res = copy.deepcopy(self)
        for conf, sky in zip(res.im_conf, skies):
            conf[sky] = 0
        return res

    @torch.no_grad()
    def fuse(self, voxel_size=None, min_count=1, weights='conf', to_host=True, normals=False, outliers=None, k=16, tracks=False, max_reproj_error=None,
             clusters=None, keep_largest=None, planes=None, upright=False):
        """The scene as ONE point cloud (new; the reference exports every masked pixel of every view): the masked points of all views
        (`get_masks()` at the scene's current min_conf_thr, as the GLB export) binned into voxels of `voxel_size` and averaged per voxel,
        weighted by the images' confidences (weights='conf') or equally (weights=None); `viz.fuse_points` on the scene's padded stacks,
        csrc/fuse.hip. voxel_size=None: the median pixel footprint (`viz.default_voxel_size`: median depth / focal; a ValueError when it is
        not a positive number -- NaN depth maps or focals -- while the scene has valid points: give a voxel_size then). min_count: voxels of
        fewer points are dropped. outliers=std_ratio: statistical outlier removal on the fused cloud first (`FusedCloud.remove_outliers`
        over k neighbours); clusters=True, or a dict of eps / min_points: then density clustering (`FusedCloud.cluster`; csrc/cloud_cluster.hip),
        the cloud carries `.labels` and `.cluster_sizes`; keep_largest=N (implies clusters): only the N largest clusters stay
        (`FusedCloud.keep_clusters`), which drops the dense floaters the outlier removal keeps; normals=True: then normals from k neighbours, turned towards the cameras of this scene that see each point
        (`FusedCloud.estimate_normals(scene=self)`; csrc/cloud_knn.hip). tracks=True: last, on the final points, the 2-D tracks -- which
        pixel of which image observes each point, by projection within one voxel_size -- as `cloud.tracks` (`FusedCloud.build_tracks`;
        csrc/tracks.hip), observations landing more than max_reproj_error pixels off dropped; `export.write_colmap` then writes POINTS2D
        and tracks. planes=N, or a dict of the arguments of `FusedCloud.detect_planes`: after the outlier and cluster removal and before
        the tracks, the N dominant planes (csrc/cloud_planes.hip); the cloud carries `.planes`, `.plane_sizes` and `.plane_labels`.
        upright=True (implies planes, 6 unless given): last, the cloud is stood on its ground plane (`FusedCloud.upright(scene=self)`: a
        ValueError when no plane has every camera on one side). The tracks are built BEFORE that motion, in the scene's frame, and the
        motion then drops them, as `FusedCloud.transform` always does: the scene's cameras do not see the moved points where the tracks
        say, so tracks=True together with upright=True returns a cloud without tracks. Returns a `viz.FusedCloud` (`.save_ply(path)`; `export.write_colmap` takes it)."""
        if self.imgs is None:
            raise ValueError('fuse needs the scene images: scene.imgs is None (the views given to global_aligner had no "img")')
        if self.device.type != 'cuda':
            raise _lib.D3RError('fuse runs on the GPU (dust3r_amd has no CPU execution path)')
        if weights not in ('conf', None):
            raise ValueError(f"fuse: weights is 'conf' or None, got {weights!r}")
        if keep_largest is not None and not clusters:
            clusters = True
        if upright and planes is None:
            planes = 6
        plane_args = dict(planes) if isinstance(planes, dict) else {} if planes is None else dict(max_planes=planes)
        if set(plane_args) - {'thr', 'max_planes', 'min_inliers', 'min_area2', 'cos_min', 'n_hyp', 'seed', 'refine_rounds', 'normals'}:
            raise ValueError(f'fuse: planes is a number of planes or a dict of the arguments of FusedCloud.detect_planes, got {planes!r}')
        cluster_args = dict(clusters) if isinstance(clusters, dict) else {}
        if set(cluster_args) - {'eps', 'min_points'}:
            raise ValueError(f"fuse: clusters is True or a dict of 'eps' / 'min_points', got {clusters!r}")
        from ..viz import default_voxel_size, fuse_points
        if voxel_size is None:       # evaluated once the bounds pass has found a valid point
            def voxel_size():
                return default_voxel_size(self.get_depthmaps(raw=True), [h * w for h, w in self.imshapes], self.get_focals())
        cloud = fuse_points(self.imgs, self.get_pts3d(raw=True), self.get_masks(raw=True), self._im_conf if weights == 'conf' else None, voxel_size,
                            self.device, min_count=min_count, to_host=to_host)
        if outliers is not None:
            cloud, _ = cloud.remove_outliers(k=k, std_ratio=outliers)
        if clusters:
            cloud = cloud.cluster(**cluster_args)
            if keep_largest is not None:
                cloud, _ = cloud.keep_clusters(largest=keep_largest)
        if normals:
            cloud = cloud.estimate_normals(k=k, scene=self)
        if planes is not None:
            cloud = cloud.detect_planes(**plane_args)
        if tracks:
            cloud = cloud.build_tracks(self, max_error=max_reproj_error, weights=weights)
        if upright:
            cloud, _ = cloud.upright(scene=self)
        return cloud

    @torch.no_grad()
    def show(self, show_pw_cams=False, show_pw_pts3d=False, cam_size=None, cam_colors=None, **kw):
        """The reference's show() (base_opt.py:297-323) without a window: the masked cloud in the images' colours (a random colour per view
        when the scene has no images), one glyph per camera in a random colour, on request the pairwise cameras and clouds; drawn on the GPU
        by `viz.SceneViz.show(**kw)` (outfile=..., size=..., point_size=...). Returns the SceneViz; the picture is its `.image`. The colours are
        drawn from numpy's global generator as in the reference, so two calls differ in them (the rasteriser itself is deterministic);
        cam_colors (new): one (r, g, b) per image instead, for the same picture on every call."""
        if self.device.type != 'cuda':
            raise _lib.D3RError('show renders on the GPU (dust3r_amd has no CPU execution path)')
        from ..viz import SceneViz, auto_cam_size
        viz = SceneViz(self.device)
        pts3d, masks = self.get_pts3d(), self.get_masks()
        if cam_colors is None:
            colors = [tuple(c) for c in np.random.randint(0, 256, size=(self.n_imgs, 3)).tolist()]
        else:
            colors = [tuple(int(v) for v in c) for c in cam_colors]
            if len(colors) != self.n_imgs or any(len(c) != 3 for c in colors):
                raise ValueError(f'show: cam_colors needs one (r, g, b) per image, {self.n_imgs} here')
        if self.imgs is None:
            for n in range(self.n_imgs):
                viz.add_pointcloud(pts3d[n], colors[n], masks[n])
        else:
            viz.add_pointcloud(list(pts3d), list(self.imgs), list(masks))
        im_poses = self.get_im_poses().detach().cpu().numpy()
        if cam_size is None:
            cam_size = auto_cam_size(im_poses)
        viz.add_cameras(im_poses, self.get_focals().detach().cpu().numpy().reshape(-1), colors=colors, imsizes=self.imsizes, cam_size=cam_size)
        if show_pw_cams:
            pw_poses = self.get_pw_poses().detach()
            viz.add_cameras(pw_poses.cpu().numpy(), imsizes=[self.imsizes[i] for i, j in self.edges], color=(192, 0, 192), cam_size=cam_size)
            if show_pw_pts3d:
                pts = [self.pred_i[edge_str(i, j)] @ pw_poses[e, :3, :3].T + pw_poses[e, :3, 3] for e, (i, j) in enumerate(self.edges)]
                viz.add_pointcloud(pts, (128, 0, 128))
        viz.show(**kw)
        return viz

    @torch.no_grad()
    def render_views(self, point_size=1, as_mesh=False, return_depth=False):
        """The fused scene re-drawn from every view's own camera, intrinsics and size -- does the cloud, seen from camera i, look like
        picture i? All views of one size share one call of the rasteriser (one call in all when the sizes agree). The cloud is the masked
        points (`get_masks()`), or with as_mesh the mesh of the GLB export. Returns a list of (H, W, 3) uint8 images, or with return_depth
        a list of (image, depth (H, W) float32, inf where nothing was drawn)."""
        if self.imgs is None:
            raise ValueError('render_views needs the scene images: scene.imgs is None (the views given to global_aligner had no "img")')
        if self.device.type != 'cuda':
            raise _lib.D3RError('render_views renders on the GPU (dust3r_amd has no CPU execution path)')
        from ..viz import SceneViz, scene_mesh_batch
        viz = SceneViz(self.device)
        if as_mesh:
            geo = scene_mesh_batch(self.imgs, self.get_pts3d(raw=True), self.get_masks(raw=True), self.device, to_host=False)
            if len(geo['faces']):
                viz.add_mesh(geo['positions'], geo['faces'], geo['colors'])
        else:
            viz.add_pointcloud(list(self.get_pts3d()), list(self.imgs), list(self.get_masks()))
        poses, K = self.get_im_poses().detach(), self.get_intrinsics().detach()
        out = [None] * self.n_imgs
        if viz.bounds() is None:
            return [np.full((h, w, 3), 255, np.uint8) if not return_depth else (np.full((h, w, 3), 255, np.uint8), np.full((h, w), np.inf, np.float32))
                    for h, w in self.imshapes]
        for shape in sorted(set(map(tuple, self.imshapes))):
            idx = [i for i, s in enumerate(self.imshapes) if tuple(s) == shape]
            res = viz.render(poses[idx], K[idx], size=(shape[1], shape[0]), point_size=point_size, return_depth=return_depth)
            for k, i in enumerate(idx):
                out[i] = (res['rgb'][k], res['depth'][k]) if return_depth else res[k]
        return out

    # ------------------------------------------------------------------ engine binding
    def _engine_tensors(self):
        """The six tensors the engine reads and updates in place, under their parameter names and in d3r_aligner_create's order: pw_poses (E, 8),
        pw_adaptors (E, 2), im_poses (n, 7), im_depthmaps (n, max_area), im_focals (n, 1 | 2), im_pp (n, 2); the scene's own storage, never a copy."""
        return {'pw_poses': self.pw_poses.data, 'pw_adaptors': self.pw_adaptors.data, 'im_poses': self._flat_im_poses.data,
                'im_depthmaps': self._flat_im_depthmaps.data, 'im_focals': self._flat_im_focals.data, 'im_pp': self._flat_im_pp.data}

    def _engine_setup(self):
        """What the scene class decides about its engine: (opt_im_poses, opt_im_focals, {_lib.ALIGNER_OPT_*: value} to set after create,
        {_lib.ALIGNER_TRAIN_*: (n,) bool array} of per-image trainability or None)."""
        raise NotImplementedError()

    def _ensure_engine(self):
        """The engine handle of the scene as it is now: a new engine whenever what it was created from -- the tensors' addresses, the loss, what is
        trainable, the options -- has changed since the last call."""
        _lib.require_device()
        if self.device.type != 'cuda':
            raise _lib.D3RError('the aligner is not on a GPU: call .to("cuda") (dust3r_amd has no CPU execution path)')
        tensors = self._engine_tensors()
        opt_im_poses, opt_im_focals, options, masks = self._engine_setup()
        masks = {kind: np.asarray(m, dtype=bool) for kind, m in (masks or {}).items()}
        sig = (self.norm_pw_scale, self.dist_name, bool(opt_im_poses), bool(opt_im_focals), tuple((k, int(v)) for k, v in options.items()),
               tuple((k, tuple(m.tolist())) for k, m in masks.items()), tuple(t.data_ptr() for t in tensors.values()))
        if self._engine is not None and sig == self._engine_sig:
            return self._engine
        self._destroy_engine()
        inputs = {k: getattr(self, k) for k in ('_stacked_pred_i', '_stacked_pred_j', '_weight_i', '_weight_j')}
        for k, t in (*inputs.items(), *tensors.items()):
            assert t.is_cuda and t.is_contiguous() and t.dtype == torch.float32, f'{k} must be a contiguous fp32 CUDA tensor'
        arr = lambda v: (C.c_int * len(v))(*v)  # noqa: E731
        ei, ej = arr([i for i, j in self.edges]), arr([j for i, j in self.edges])
        hh, ww = arr([h for h, w in self.imshapes]), arr([w for h, w in self.imshapes])
        h = C.c_void_p()
        with torch.cuda.device(self.device):
            check(lib.d3r_aligner_create(C.byref(h), self.n_imgs, self.n_edges, ei, ej, hh, ww, self.max_area, *map(ptr, inputs.values()),
                                         *map(ptr, tensors.values()), float(self.base_scale), float(self.pw_break), float(self.focal_break),
                                         int(self.dist_name == 'l2'), int(self.norm_pw_scale), int(opt_im_poses), int(opt_im_focals), 1024,
                                         current_stream()), 'aligner_create')
            try:
                for opt, value in options.items():
                    check(lib.d3r_aligner_set_option(h, opt, int(value)), f'set_option({opt})')
                for kind, m in masks.items():
                    check(lib.d3r_aligner_set_trainable(h, kind, bytes(m.astype(np.uint8))), f'set_trainable({kind})')
            except Exception:
                lib.d3r_aligner_destroy(h)
                raise
        self._engine, self._engine_sig = h, sig
        return h

    def _destroy_engine(self):
        if getattr(self, '_engine', None) is not None:
            lib.d3r_aligner_destroy(self._engine)
            self._engine = None

    def __deepcopy__(self, memo):
        """Every tensor is copied; the copy has no engine and builds its own on first use: the engine handle is a native pointer into this
        scene's tensors."""
        res = type(self).__new__(type(self))
        memo[id(self)] = res
        for k, v in self.__dict__.items():
            res.__dict__[k] = None if k in ('_engine', '_engine_sig') else copy.deepcopy(v, memo)
        return res

    def __del__(self):
        try:
            self._destroy_engine()
        except Exception:
            pass

    @torch.no_grad()
    def forward(self, ret_details=False):
        """The alignment loss of the scene class (optimizer.py:188-201, or base_opt.py:246-273 for the Modular scene), evaluated by the engine (no
        parameter update)."""
        if ret_details:
            raise NotImplementedError('ret_details: the per-pair loss matrix is not computed by the engine')
        loss = torch.empty(1, dtype=torch.float32, device=self.device)
        check(lib.d3r_aligner_loss_grad(self._ensure_engine(), ptr(loss), None, None, None, None, None, None, current_stream()), 'aligner_loss')
        return loss[0]

    @torch.no_grad()
    def loss_and_grads(self):
        """(loss, {name: grad}) of one forward/backward without a step -- the engine's analytic gradients, each shaped like its tensor of
        _engine_tensors() and given for frozen entries too."""
        eng = self._ensure_engine()
        loss = torch.empty(1, dtype=torch.float32, device=self.device)
        g = {k: torch.zeros_like(t) for k, t in self._engine_tensors().items()}
        check(lib.d3r_aligner_loss_grad(eng, ptr(loss), ptr(g['pw_poses']), ptr(g['im_poses']), ptr(g['im_depthmaps']),
                                        ptr(g['im_focals']), ptr(g['im_pp']), ptr(g['pw_adaptors']), current_stream()), 'aligner_loss_grad')
        return loss[0], g

    def set_reduction(self, use_dpp=True):
        check(lib.d3r_aligner_set_option(self._ensure_engine(), _lib.ALIGNER_OPT_DPP_REDUCE, int(use_dpp)), 'set_option')

    def compute_global_alignment(self, init=None, niter_PnP=10, group=None, **kw):
        """`group` (new; the reference's loop is single-device): a torch.distributed process group (or True for the default one) whose ranks each hold this
        scene -- the return value of `inference_sharded` -- and then share the loop: every rank owns a contiguous range of images (global_alignment_loop_sharded).
        The initialisation runs replicated (it is deterministic); poses, focals and the final loss are the same on every rank, bit for bit what one GPU computes."""
        if init is None:
            pass
        elif init in ('msp', 'mst'):
            init_fun.init_minimum_spanning_tree(self, niter_PnP=niter_PnP)
        elif init == 'known_poses':
            init_fun.init_from_known_poses(self, min_conf_thr=self.min_conf_thr, niter_PnP=niter_PnP)
        else:
            raise ValueError(f'bad value for {init=}')
        if group is not None and group is not False:
            return global_alignment_loop_sharded(self, group=None if group is True else group, **kw)
        return global_alignment_loop(self, **kw)


def _loop_start(net, niter, schedule):
    """What both loops begin with: (engine handle with its Adam state reset -- a fresh optimiser per call, as in the reference --, schedule id),
    or None when there is nothing to iterate."""
    if schedule not in ('cosine', 'linear'):
        raise ValueError(f'bad lr {schedule=}')
    if niter <= 0:
        return None
    eng = net._ensure_engine()
    check(lib.d3r_aligner_set_option(eng, _lib.ALIGNER_OPT_RESET_ADAM, 0), 'reset adam')
    return eng, _lib.SCHEDULE_COSINE if schedule == 'cosine' else _lib.SCHEDULE_LINEAR


def global_alignment_loop(net, lr=0.01, niter=300, schedule='cosine', lr_min=1e-6):
    """Mirror of base_opt.py:326-349: Adam(lr, betas=(0.9, 0.9)), lr scheduled per iteration; returns the
    loss of the last iteration. The iterations run inside the fused HIP aligner."""
    start = _loop_start(net, niter, schedule)
    if start is None:
        return float('inf')
    eng, sched = start
    verbose = net.verbose
    if verbose:
        print('Global alignement - optimizing for:')
        print(net.trainable_names())
    chunk = min(niter, 50 if verbose else 1024)
    losses = torch.empty(chunk, dtype=torch.float32, device=net.device)
    loss = float('inf')
    bar = tqdm.tqdm(total=niter) if verbose else None
    done = 0
    while done < niter:
        k = min(chunk, niter - done)
        check(lib.d3r_aligner_run(eng, k, done, niter, float(lr), float(lr_min), sched, ptr(losses), current_stream()), 'aligner_run')
        done += k
        if verbose or done >= niter:
            loss = float(losses[k - 1])                                    # the only host synchronisation
        if bar is not None:
            t = (done - 1) / niter
            cur = cosine_schedule(t, lr, lr_min) if schedule == 'cosine' else linear_schedule(t, lr, lr_min)
            bar.set_postfix_str(f'lr={cur:g} loss={loss:g}')
            bar.update(k)
    if bar is not None:
        bar.close()
    return loss


def image_ranges(edges, imshapes, world):
    """Contiguous image ranges [(first, count)] * world with balanced work: the main pass of an image costs its area times (the edge sides projected onto it + 1.5
    for its own depth map and Adam state: 32 B per edge-side pixel against 24 + 24 B per pixel). Ranks beyond the number of images get empty ranges."""
    n = len(imshapes)
    sides = [0] * n
    for i, j in edges:
        sides[i] += 1
        sides[j] += 1
    cost = [(sides[k] + 1.5) * imshapes[k][0] * imshapes[k][1] for k in range(n)]
    cum = [0.0]
    for c in cost:
        cum.append(cum[-1] + c)
    cuts = [0]
    for r in range(1, world):
        target = cum[-1] * r / world
        k = cuts[-1]
        while k < n and cum[k + 1] <= target:
            k += 1
        if k < n and target - cum[k] > cum[k + 1] - target:       # the nearer of the two neighbouring cuts
            k += 1
        cuts.append(max(k, cuts[-1]))
    cuts.append(n)
    return [(cuts[r], cuts[r + 1] - cuts[r]) for r in range(world)]


@torch.no_grad()
def global_alignment_loop_sharded(net, group=None, lr=0.01, niter=300, schedule='cosine', lr_min=1e-6):
    """global_alignment_loop over the ranks of `group` (one process per GPU; every rank holds the whole scene). Rank r runs the main pass of ITS images
    (include/dust3r_hip.h, d3r_aligner_set_image_range / step_begin / step_end); the reduced fp64 sums ((2 E + n) x 16 doubles: 160 KB at 100 views / 600 edges) are
    all-reduced once per iteration, and the pose / focal step runs replicated. Every partial record belongs to one image, i.e. to one rank: the other ranks add exact
    zeros, so losses and parameters are bit-identical to the single-GPU loop for any number of ranks. Start: all six parameter tensors are broadcast from rank 0 (a
    random `init=None` start differs between processes, for frozen tensors too); end: every rank receives the other ranks' rows of im_depthmaps."""
    import torch.distributed as dist
    start = _loop_start(net, niter, schedule)
    if start is None:
        return float('inf')
    eng, sched = start
    world, rank = dist.get_world_size(group), dist.get_rank(group)
    # ALL six parameter tensors, frozen ones included: a frozen tensor without a preset still holds its per-process random start (init=None), and the replicated
    # pose / focal step would then diverge silently between ranks (a few KB apart from the depth maps)
    tensors = net._engine_tensors()
    for t in tensors.values():
        dist.broadcast(t, src=dist.get_global_rank(group, 0) if group is not None else 0, group=group)
    ranges = image_ranges(net.edges, net.imshapes, world)
    first, count = ranges[rank]
    check(lib.d3r_aligner_set_image_range(eng, first, count), 'set_image_range')
    red_ptr, red_n = C.c_void_p(), C.c_longlong()
    check(lib.d3r_aligner_reduced_sums(eng, C.byref(red_ptr), C.byref(red_n)), 'reduced_sums')
    # the engine's reduction buffer seen as a tensor (no copy): the collective works on it in place
    red = _device_view(red_ptr.value, int(red_n.value), torch.float64, net.device)
    cap = int(getattr(net, '_engine_max_iters', 1024))
    losses = torch.empty(min(niter, cap), dtype=torch.float32, device=net.device)
    done, loss = 0, float('inf')
    try:
        while done < niter:
            k_run = min(cap, niter - done)
            for k in range(k_run):
                check(lib.d3r_aligner_step_begin(eng, k, done, niter, float(lr), float(lr_min), sched, current_stream()), 'aligner_step_begin')
                dist.all_reduce(red, op=dist.ReduceOp.SUM, group=group)
                check(lib.d3r_aligner_step_end(eng, k, done, niter, float(lr), float(lr_min), sched, current_stream()), 'aligner_step_end')
            check(lib.d3r_aligner_read_losses(eng, k_run, ptr(losses), current_stream()), 'aligner_read_losses')
            done += k_run
            loss = float(losses[k_run - 1])
    finally:
        # never raise from here: an error of the loop above must reach the caller as itself (the other ranks see it as a collective timeout)
        rc = lib.d3r_aligner_set_image_range(eng, 0, net.n_imgs)
        if rc != 0:
            import logging
            logging.getLogger('dust3r_amd').error('d3r_aligner_set_image_range(all) failed with code %d after the sharded loop', rc)
    # every rank's own rows of the log-depth maps -> all ranks (sum with zeros elsewhere: exact)
    depth = tensors['im_depthmaps']
    own = torch.zeros_like(depth)
    own[first:first + count] = depth[first:first + count]
    dist.all_reduce(own, op=dist.ReduceOp.SUM, group=group)
    depth.copy_(own)
    return loss


def _device_view(address, numel, dtype, device):
    """A torch tensor over `numel` elements of device memory the engine owns (no copy, no ownership)."""
    class _Span:
        pass
    span = _Span()
    itemsize = torch.empty((), dtype=dtype).element_size()
    span.__cuda_array_interface__ = {'shape': (numel,), 'typestr': {torch.float64: '<f8', torch.float32: '<f4'}[dtype], 'data': (int(address), False), 'version': 2,
                                     'strides': None}
    t = torch.as_tensor(span, device=device)
    assert t.data_ptr() == int(address) and t.numel() == numel and t.element_size() == itemsize
    return t


@torch.no_grad()
def _clean_stacks(conf, depth, pts3d, K, cams, heights, widths, tol=0.001, bad_conf=0):
    """d3r_clean_pointcloud on padded stacks: conf (n, row) fp32, updated IN PLACE in the kernel's order (image i sees the cleaned confidences of
    the images before it), depth (n, row), pts3d (n, row, 3), K (n, 3, 3), cams (n, 4, 4) world-to-camera, heights / widths (n,) int32."""
    _lib.require_device()
    n, row = conf.shape
    depth, pts3d = depth.detach().float().contiguous(), pts3d.detach().float().contiguous()
    assert conf.is_cuda and conf.is_contiguous() and conf.dtype == torch.float32 and depth.shape == (n, row) and pts3d.shape == (n, row, 3)
    Kc = K.float().contiguous().reshape(n, 9)
    w2c = cams.float().contiguous().reshape(n, 16)
    with torch.cuda.device(conf.device):
        check(lib.d3r_clean_pointcloud(n, ptr(conf), ptr(depth), ptr(pts3d), ptr(Kc), ptr(w2c), ptr(heights), ptr(widths), row, float(tol),
                                       float(bad_conf), current_stream()), 'clean_pointcloud')


@torch.no_grad()
def clean_pointcloud_hip(im_confs, K, cams, depthmaps, all_pts3d, tol=0.001, bad_conf=0):
    """The reference's `clean_pointcloud` (base_opt.py:369-405: a point of image i that projects IN FRONT of image j's depthmap while
    being less confident than the pixel it lands on gets its confidence clipped to `bad_conf`; images visited in order, each seeing
    the already cleaned confidences of the earlier ones), computed by d3r_clean_pointcloud: n launches, one thread per pixel walking
    the other cameras, instead of n (n - 1) rounds of ~15 elementwise torch kernels. This is the list front end (the new confidences are
    returned, the inputs left alone); a scene runs the same call on its own stacks."""
    dev = im_confs[0].device
    shapes = [tuple(c.shape) for c in im_confs]
    conf = pad_views(im_confs, dev, torch.float32, name='clean_pointcloud: confidence map')
    depth = pad_views(depthmaps, dev, torch.float32, shapes=shapes, name='clean_pointcloud: depth map')
    pts = pad_views(all_pts3d, dev, torch.float32, tail=(3,), shapes=shapes, name='clean_pointcloud: pointmap')
    _clean_stacks(conf, depth, pts, K, cams, *shape_tables(shapes, dev)[:2], tol=tol, bad_conf=bad_conf)
    return [c.to(im_confs[i].dtype) for i, c in enumerate(split_views(conf, shapes))]
