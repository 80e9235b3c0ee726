"""`ModularPointCloudOptimizer` -- host-side mirror of the reference `dust3r/cloud_opt/modular_optimizer.py`:
the alignment scene that can freeze PART of the cameras (`preset_pose` / `preset_focal` / `preset_principal_point` /
`preset_intrinsics` on a subset of images), with separate x and y focals (`fx_and_fy=True`) and the loss of
`BasePCOptimizer.forward` (base_opt.py:246-273: the mean over each edge side's image, averaged over edges).

Storage. The reference keeps one `nn.Parameter` per image in `ParameterList`s and freezes single entries. Here the values
live in flat contiguous fp32 tensors the fused HIP aligner reads and updates in place (`_flat_im_poses` (n, 7),
`_flat_im_depthmaps` (n, max_area) log-depth zero padded like PointCloudOptimizer's, `_flat_im_focals` (n, 1 | 2),
`_flat_im_pp` (n, 2)), and `im_poses`, `im_depthmaps`, `im_focals`, `im_pp` are lists of per-image `nn.Parameter`s that
ALIAS rows of that storage: `scene.im_poses[i].requires_grad` answers per image (init_im_poses.get_known_poses reads it),
`param.data[:] = ...` writes where the engine reads, and `state_dict()` uses the reference's keys (`im_poses.<i>`,
`im_depthmaps.<i>` as (H, W), ...). The per-image `requires_grad` flags become the engine's trainability masks
(d3r_aligner_set_trainable): frozen entries get no Adam update, as in the reference where they are not in the optimiser.
"""
import ctypes as C

import numpy as np
import torch
import torch.nn as nn

from .. import _lib
from .._lib import check, current_stream, lib, ptr
from ..utils.device import to_numpy
from ..utils.geometry import geotrf
from .base_opt import BasePCOptimizer
from .optimizer import PointCloudOptimizer

_ENTRIES = ('im_poses', 'im_depthmaps', 'im_focals', 'im_pp')
# C ABI (include/dust3r_hip.h)
_OPT_OPTIMIZE_PP, _OPT_ADAPTORS, _OPT_EDGE_MEAN_LOSS, _OPT_FX_AND_FY = 3, 4, 6, 7
_TRAIN_KIND = {'im_poses': 0, 'im_focals': 1, 'im_pp': 2}


class ParamEntries(list):
    """The per-image parameters of one group (the reference's `nn.ParameterList`), each a view of one row of the flat storage."""

    def requires_grad_(self, requires_grad=True):
        for p in self:
            p.requires_grad_(requires_grad)
        return self


class ModularPointCloudOptimizer(BasePCOptimizer):
    """Optimize a global scene given pairwise observations; unlike PointCloudOptimizer, parts of it (single poses, focals,
    principal points) can be fixed. Graph nodes: images; edges: (pred1, pred2)."""

    def __init__(self, *args, optimize_pp=False, fx_and_fy=False, focal_brake=20, **kwargs):
        super().__init__(*args, **kwargs)
        self.has_im_poses = True
        self.focal_brake = focal_brake
        self.fx_and_fy = bool(fx_and_fy)
        n = self.n_imgs
        # the reference's initial distributions, drawn in its order (modular_optimizer.py:29-35): one randn(H, W) per image, then the poses
        depth = torch.zeros((n, self.max_area))
        for k, (H, W) in enumerate(self.imshapes):
            depth[k, :H * W] = (torch.randn(H, W) / 10 - 3).reshape(-1)
        poses = torch.stack([self.rand_pose(self.POSE_DIM) for _ in range(n)]).float()
        focals = torch.tensor([[self.focal_brake * np.log(max(H, W))] * (2 if self.fx_and_fy else 1) for H, W in self.imshapes], dtype=torch.float32)
        self.register_buffer('_flat_im_depthmaps', depth)
        self.register_buffer('_flat_im_poses', poses.contiguous())
        self.register_buffer('_flat_im_focals', focals)
        self.register_buffer('_flat_im_pp', torch.zeros((n, 2)))
        self.register_buffer('_pp', torch.tensor([(w / 2, h / 2) for h, w in self.imshapes], dtype=torch.float32))
        self._grid_cache = None
        self._bind_entries({'im_pp': [bool(optimize_pp)] * n})

    # ------------------------------------------------------------------ per-image views of the flat storage
    def _bind_entries(self, flags=None):
        """(Re)creates the per-image parameters over the flat tensors (after construction and after .to()), keeping their requires_grad flags."""
        flags = dict(flags or {})
        for name in _ENTRIES:
            if name not in flags:
                old = getattr(self, name, None)
                flags[name] = [p.requires_grad for p in old] if old is not None else [True] * self.n_imgs
            flat = getattr(self, '_flat_' + name)
            if name == 'im_depthmaps':
                rows = [flat[k, :H * W].view(H, W) for k, (H, W) in enumerate(self.imshapes)]
            else:
                rows = [flat[k] for k in range(self.n_imgs)]
            object.__setattr__(self, name, ParamEntries(nn.Parameter(r, requires_grad=f) for r, f in zip(rows, flags[name])))

    @property
    def focal_break(self):
        """The reference spells this scene's keyword `focal_brake`; the scene bootstrap reads the PointCloudOptimizer spelling."""
        return self.focal_brake

    def _trainable(self, name):
        return np.array([p.requires_grad for p in getattr(self, name)], dtype=bool)

    def trainable_names(self):
        names = [k for k in ('pw_poses', 'pw_adaptors') if getattr(self, k).requires_grad]
        return names + [k for k in _ENTRIES if self._trainable(k).any()]

    def to(self, device, *a, **k):
        super().to(device, *a, **k)
        self._bind_entries()
        return self

    def __deepcopy__(self, memo):
        res = super().__deepcopy__(memo)
        res._bind_entries()           # nn.Parameter copies are clones: make the copy's per-image parameters views of ITS flat storage again
        return res

    def state_dict(self, trainable=True):
        """The reference's keys: pw_poses, pw_adaptors, im_conf.<i>, im_depthmaps.<i> (H, W), im_poses.<i> (7,), im_focals.<i> (1,) | (2,), im_pp.<i> (2,)."""
        if not trainable:
            return super().state_dict(trainable=False)
        out = {k: getattr(self, k).detach().clone() for k in ('pw_poses', 'pw_adaptors')}
        out.update({f'im_conf.{i}': c.clone() for i, c in enumerate(self.im_conf)})
        for name in _ENTRIES:
            out.update({f'{name}.{i}': p.detach().clone() for i, p in enumerate(getattr(self, name))})
        return out

    @torch.no_grad()
    def load_state_dict(self, data, **kw):
        """Accepts the reference's keys (state_dict() above, or one recorded from the reference's class) and, for the four image groups,
        also whole stacked tensors under the group's name: im_poses (n, 7), im_depthmaps (n, max_area), im_focals (n, 1 | 2), im_pp (n, 2)."""
        for k, v in data.items():
            v = torch.as_tensor(v)
            if k in ('pw_poses', 'pw_adaptors'):
                getattr(self, k).data.copy_(v.to(self.device).reshape(getattr(self, k).shape))
            elif k.startswith('im_conf.'):
                self.im_conf[int(k.split('.')[1])].copy_(v)
            elif k in _ENTRIES:
                flat = getattr(self, '_flat_' + k)
                flat.copy_(v.to(self.device).reshape(self.n_imgs, -1).expand_as(flat))
            elif k.split('.')[0] in _ENTRIES and k.count('.') == 1:
                name, i = k.split('.')
                p = getattr(self, name)[int(i)]
                p.data.copy_(v.to(self.device).reshape(p.shape))
        return self

    # ------------------------------------------------------------------ presets (modular_optimizer.py:37-92)
    _get_msk_indices = PointCloudOptimizer._get_msk_indices

    def _no_grad(self, tensor):
        return tensor.requires_grad_(False)

    def preset_pose(self, known_poses, pose_msk=None):  # cam-to-world
        if isinstance(known_poses, torch.Tensor) and known_poses.ndim == 2:
            known_poses = [known_poses]
        for idx, pose in zip(self._get_msk_indices(pose_msk), known_poses):
            if self.verbose:
                print(f' (setting pose #{idx} = {pose[:3, 3]})')
            self._no_grad(self._set_pose(self.im_poses, idx, torch.as_tensor(pose), force=True))
        # normalize scale if there's less than 1 known pose
        n_known_poses = sum((p.requires_grad is False) for p in self.im_poses)
        self.norm_pw_scale = (n_known_poses <= 1)

    def preset_intrinsics(self, known_intrinsics, msk=None):
        if isinstance(known_intrinsics, torch.Tensor) and known_intrinsics.ndim == 2:
            known_intrinsics = [known_intrinsics]
        for K in known_intrinsics:
            assert K.shape == (3, 3)
        self.preset_focal([K.diagonal()[:2].mean() for K in known_intrinsics], msk)
        self.preset_principal_point([K[:2, 2] for K in known_intrinsics], msk)

    def preset_focal(self, known_focals, msk=None):
        for idx, focal in zip(self._get_msk_indices(msk), known_focals):
            if self.verbose:
                print(f' (setting focal #{idx} = {focal})')
            self._no_grad(self._set_focal(idx, focal, force=True))

    def preset_principal_point(self, known_pp, msk=None):
        for idx, pp in zip(self._get_msk_indices(msk), known_pp):
            if self.verbose:
                print(f' (setting principal point #{idx} = {pp})')
            self._no_grad(self._set_principal_point(idx, pp, force=True))

    def _set_pose(self, poses, idx, R, T=None, scale=None, force=False):
        if poses is not self.im_poses:                          # pw_poses: one tensor, as in every scene
            return super()._set_pose(poses, idx, R, T, scale, force)
        pose = poses[idx]
        if pose.requires_grad or force:                         # can only init a parameter not already initialized
            super()._set_pose(self._flat_im_poses, idx, R, T, scale, force=True)
        return pose

    def _set_focal(self, idx, focal, force=False):
        param = self.im_focals[idx]
        if param.requires_grad or force:
            with torch.no_grad():
                param.data[:] = float(self.focal_brake * np.log(float(focal)))
        return param

    def _set_principal_point(self, idx, pp, force=False):
        param = self.im_pp[idx]
        H, W = self.imshapes[idx]
        if param.requires_grad or force:
            with torch.no_grad():
                param.data[:] = torch.as_tensor((np.asarray(to_numpy(pp), np.float32) - (W / 2, H / 2)) / 10, dtype=torch.float32)
        return param

    def _set_depthmap(self, idx, depth, force=False):
        param = self.im_depthmaps[idx]
        if param.requires_grad or force:
            with torch.no_grad():
                param.data[:] = torch.as_tensor(depth).log().nan_to_num(neginf=0).to(param.device)
        return param

    # ------------------------------------------------------------------ getters (modular_optimizer.py:94-151)
    def get_focals(self):
        """(n, 1), or (n, 2) = (fx, fy) with fx_and_fy."""
        return (self._flat_im_focals / self.focal_brake).exp()

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
        if not raw:
            res = [dm[:h * w].view(h, w) for dm, (h, w) in zip(res, self.imshapes)]
        return res

    _grid = PointCloudOptimizer._grid

    def depth_to_pts3d(self):
        focals = self.get_focals().unsqueeze(1)                 # (n,1,1 | 2): x = d (u - cx) / fx, y = d (v - cy) / fy
        pp = self.get_principal_points().unsqueeze(1)           # (n,1,2)
        depth = self.get_depthmaps(raw=True).unsqueeze(-1)      # (n,A,1)
        rel = torch.cat((depth * (self._grid - pp) / focals, depth), dim=-1)
        return geotrf(self.get_im_poses(), rel)

    # ------------------------------------------------------------------ engine binding
    def _ensure_engine(self):
        _lib.require_device()
        if self.device.type != 'cuda':
            raise _lib.D3RError('the aligner is not on a GPU: call .to("cuda") (dust3r_amd has no CPU execution path)')
        masks = {k: self._trainable(k) for k in ('im_poses', 'im_focals', 'im_pp')}
        sig = (self.norm_pw_scale, self.pw_adaptors.requires_grad, self.dist_name, self.fx_and_fy,
               tuple(tuple(m.tolist()) for m in masks.values()),
               tuple(t.data_ptr() for t in (self.pw_poses, self.pw_adaptors, self._flat_im_depthmaps, self._flat_im_poses, self._flat_im_focals, self._flat_im_pp)))
        if self._engine is not None and sig == self._engine_sig:
            return self._engine
        self._destroy_engine()
        for k in ('_stacked_pred_i', '_stacked_pred_j', '_weight_i', '_weight_j', 'pw_poses', 'pw_adaptors', '_flat_im_poses',
                  '_flat_im_depthmaps', '_flat_im_focals', '_flat_im_pp'):
            t = getattr(self, k)
            assert t.is_cuda and t.is_contiguous() and t.dtype == torch.float32, f'{k} must be a contiguous fp32 CUDA tensor'
        n, E = self.n_imgs, self.n_edges
        arr = lambda v: (C.c_int * len(v))(*v)  # noqa: E731
        ei, ej = arr([i for i, j in self.edges]), arr([j for i, j in self.edges])
        hh, ww = arr([h for h, w in self.imshapes]), arr([w for h, w in self.imshapes])
        h = C.c_void_p()
        with torch.cuda.device(self.device):
            # opt_im_poses / opt_im_focals = 1: the per-image masks below decide
            check(lib.d3r_aligner_create(C.byref(h), n, E, ei, ej, hh, ww, self.max_area, ptr(self._stacked_pred_i),
                                         ptr(self._stacked_pred_j), ptr(self._weight_i), ptr(self._weight_j), ptr(self.pw_poses.data),
                                         ptr(self.pw_adaptors.data), ptr(self._flat_im_poses), ptr(self._flat_im_depthmaps),
                                         ptr(self._flat_im_focals), ptr(self._flat_im_pp), float(self.base_scale), float(self.pw_break),
                                         float(self.focal_brake), int(self.dist_name == 'l2'), int(self.norm_pw_scale), 1, 1, 1024,
                                         current_stream()), 'aligner_create')
            try:
                check(lib.d3r_aligner_set_option(h, _OPT_OPTIMIZE_PP, int(masks['im_pp'].any())), 'set_option(optimize_pp)')
                check(lib.d3r_aligner_set_option(h, _OPT_ADAPTORS, int(self.pw_adaptors.requires_grad)), 'set_option(allow_pw_adaptors)')
                check(lib.d3r_aligner_set_option(h, _OPT_EDGE_MEAN_LOSS, 1), 'set_option(edge_mean_loss)')
                check(lib.d3r_aligner_set_option(h, _OPT_FX_AND_FY, int(self.fx_and_fy)), 'set_option(fx_and_fy)')
                for name, m in masks.items():
                    check(lib.d3r_aligner_set_trainable(h, _TRAIN_KIND[name], bytes(m.astype(np.uint8))), f'set_trainable({name})')
            except Exception:
                lib.d3r_aligner_destroy(h)
                raise
        self._engine, self._engine_sig = h, sig
        return h

    @torch.no_grad()
    def forward(self, ret_details=False):
        """The alignment loss (base_opt.py:246-273), evaluated by the engine (no parameter update)."""
        if ret_details:
            raise NotImplementedError('ret_details: the per-pair loss matrix is not computed by the engine')
        eng = self._ensure_engine()
        loss = torch.empty(1, dtype=torch.float32, device=self.device)
        check(lib.d3r_aligner_loss_grad(eng, ptr(loss), None, None, None, None, None, None, current_stream()), 'aligner_loss')
        return loss[0]

    @torch.no_grad()
    def loss_and_grads(self):
        """(loss, {name: grad}) of one forward/backward without a step. Image groups come flat: im_poses (n, 7), im_depthmaps (n, max_area),
        im_focals (n, 1 | 2), im_pp (n, 2); gradients are given for frozen entries too."""
        eng = self._ensure_engine()
        loss = torch.empty(1, dtype=torch.float32, device=self.device)
        g = {k: torch.zeros_like(getattr(self, k).data) for k in ('pw_poses', 'pw_adaptors')}
        g.update({k: torch.zeros_like(getattr(self, '_flat_' + k)) for k in _ENTRIES})
        check(lib.d3r_aligner_loss_grad(eng, ptr(loss), ptr(g['pw_poses']), ptr(g['im_poses']), ptr(g['im_depthmaps']),
                                        ptr(g['im_focals']), ptr(g['im_pp']), ptr(g['pw_adaptors']), current_stream()), 'aligner_loss_grad')
        return loss[0], g

    def compute_global_alignment(self, init=None, niter_PnP=10, group=None, **kw):
        if group is not None and group is not False:
            raise NotImplementedError('ModularPointCloudOptimizer runs on one GPU: the multi-rank loop (group=) is implemented for PointCloudOptimizer only')
        if init == 'known_poses':
            # the reference's init_from_known_poses needs get_known_focal_mask, which its ModularPointCloudOptimizer does not implement
            raise NotImplementedError("init='known_poses' is not available for ModularPointCloudOptimizer (as in the reference): use init='mst'")
        return super().compute_global_alignment(init=init, niter_PnP=niter_PnP, **kw)
