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
import numpy as np
import torch
import torch.nn as nn

from .. import _lib
from ..utils.device import to_numpy
from ..utils.padded import pad_views, split_views
from .base_opt import BasePCOptimizer

_ENTRIES = ('im_poses', 'im_depthmaps', 'im_focals', 'im_pp')


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
        depth = pad_views([torch.randn(H, W) / 10 - 3 for H, W in self.imshapes], 'cpu', torch.float32, row=self.max_area)
        poses = torch.stack([self.rand_pose(self.POSE_DIM) for _ in range(n)]).float()
        focals = torch.tensor([[self.focal_brake * np.log(max(H, W))] * (2 if self.fx_and_fy else 1) for H, W in self.imshapes], dtype=torch.float32)
        self.register_buffer('_flat_im_depthmaps', depth)
        self.register_buffer('_flat_im_poses', poses.contiguous())
        self.register_buffer('_flat_im_focals', focals)
        self.register_buffer('_flat_im_pp', torch.zeros((n, 2)))
        self.register_buffer('_pp', torch.tensor([(w / 2, h / 2) for h, w in self.imshapes], dtype=torch.float32))
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
            rows = split_views(flat, self.imshapes) if name == 'im_depthmaps' else [flat[k] for k in range(self.n_imgs)]
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

    # ------------------------------------------------------------------ getters (modular_optimizer.py:94-151) and engine binding: BasePCOptimizer's
    def _engine_setup(self):
        masks = {_lib.ALIGNER_TRAIN_POSES: self._trainable('im_poses'), _lib.ALIGNER_TRAIN_FOCALS: self._trainable('im_focals'),
                 _lib.ALIGNER_TRAIN_PP: self._trainable('im_pp')}
        options = {_lib.ALIGNER_OPT_OPTIMIZE_PP: masks[_lib.ALIGNER_TRAIN_PP].any(), _lib.ALIGNER_OPT_OPTIMIZE_ADAPTORS: self.pw_adaptors.requires_grad,
                   _lib.ALIGNER_OPT_EDGE_MEAN_LOSS: 1, _lib.ALIGNER_OPT_FX_AND_FY: self.fx_and_fy}
        return 1, 1, options, masks           # opt_im_poses / opt_im_focals = 1: the per-image masks decide

    def compute_global_alignment(self, init=None, niter_PnP=10, group=None, **kw):
        if group is not None and group is not False:
            raise NotImplementedError('ModularPointCloudOptimizer runs on one GPU: the multi-rank loop (group=) is implemented for PointCloudOptimizer only')
        if init == 'known_poses':
            # the reference's init_from_known_poses needs get_known_focal_mask, which its ModularPointCloudOptimizer does not implement
            raise NotImplementedError("init='known_poses' is not available for ModularPointCloudOptimizer (as in the reference): use init='mst'")
        return super().compute_global_alignment(init=init, niter_PnP=niter_PnP, **kw)
