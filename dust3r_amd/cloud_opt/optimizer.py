"""`PointCloudOptimizer` -- host-side mirror of the reference `dust3r/cloud_opt/optimizer.py:16-237`.

Holds the reference's parameter tensors under the reference's names and parameterisation
(`im_depthmaps` log-depth (n, max_area), `im_poses` (n, 7) quat XYZW + signed-log translation,
`im_focals` (n, 1) = focal_break * log f, `im_pp` (n, 2), `pw_poses` (E, 8)) and exposes the same
getters / presets. `forward()` (the loss) and the optimisation loop are evaluated by the fused HIP
aligner, which reads and updates these tensors in place.
"""
import numpy as np
import torch
import torch.nn as nn

from .. import _lib
from ..utils.device import to_numpy
from ..utils.padded import pad_views
from .base_opt import BasePCOptimizer


class PointCloudOptimizer(BasePCOptimizer):
    def __init__(self, *args, optimize_pp=False, focal_break=20, **kwargs):
        super().__init__(*args, **kwargs)
        self.has_im_poses = True
        self.focal_break = focal_break
        n = self.n_imgs
        # same initial distributions as optimizer.py:29-34
        areas = torch.tensor([H * W for H, W in self.imshapes])
        depth0 = torch.randn((n, self.max_area)).div_(10).sub_(3)                            # one draw for all images, scaled in place (79 MB at 100 views: no second and third copy to page in)
        if int(areas.min()) < self.max_area:
            depth0.mul_(torch.arange(self.max_area)[None, :] < areas[:, None])                  # zero in the padding
        self.im_depthmaps = nn.Parameter(depth0)
        self.im_poses = nn.Parameter(torch.stack([self.rand_pose(self.POSE_DIM) for _ in range(n)]).float())
        self.im_focals = nn.Parameter(torch.tensor([[self.focal_break * np.log(max(H, W))] for H, W in self.imshapes], dtype=torch.float32))
        self.im_pp = nn.Parameter(torch.zeros((n, 2)), requires_grad=bool(optimize_pp))       # optimizer.py:34: im_pp.requires_grad_(optimize_pp)
        self.imshape = self.imshapes[0]
        self.register_buffer('_pp', torch.tensor([(w / 2, h / 2) for h, w in self.imshapes], dtype=torch.float32))
        self.register_buffer('_ei', torch.tensor([i for i, j in self.edges]))
        self.register_buffer('_ej', torch.tensor([j for i, j in self.edges]))
        im_areas = [h * w for h, w in self.imshapes]
        self.total_area_i = sum(im_areas[i] for i, j in self.edges)
        self.total_area_j = sum(im_areas[j] for i, j in self.edges)

    def trainable_names(self):
        return [k for k in ('pw_poses', 'pw_adaptors', 'im_depthmaps', 'im_poses', 'im_focals', 'im_pp') if getattr(self, k).requires_grad]

    # ------------------------------------------------------------------ presets (optimizer.py:63-125)
    def _check_all_imgs_are_selected(self, msk):
        assert np.all(self._get_msk_indices(msk) == np.arange(self.n_imgs)), 'incomplete mask!'

    def preset_pose(self, known_poses, pose_msk=None):
        self._check_all_imgs_are_selected(pose_msk)
        if isinstance(known_poses, torch.Tensor) and known_poses.ndim == 2:
            known_poses = [known_poses]
        for idx, pose in zip(self._get_msk_indices(pose_msk), known_poses):
            if self.verbose:
                print(f' (setting pose #{idx} = {pose[:3, 3]})')
            assert self.im_poses.requires_grad, 'it must be True at this point, otherwise no modification occurs'
            self._set_pose(self.im_poses, idx, torch.as_tensor(pose))
        self.im_poses.requires_grad_(False)
        self.norm_pw_scale = False
        self._destroy_engine()

    def preset_focal(self, known_focals, msk=None):
        self._check_all_imgs_are_selected(msk)
        for idx, focal in zip(self._get_msk_indices(msk), known_focals):
            if self.verbose:
                print(f' (setting focal #{idx} = {focal})')
            assert self.im_focals.requires_grad
            self._set_focal(idx, focal)
        self.im_focals.requires_grad_(False)
        self._destroy_engine()

    def preset_principal_point(self, known_pp, msk=None):
        self._check_all_imgs_are_selected(msk)
        for idx, pp in zip(self._get_msk_indices(msk), known_pp):
            if self.verbose:
                print(f' (setting principal point #{idx} = {pp})')
            self._set_principal_point(idx, pp, force=True)
        self.im_pp.requires_grad_(False)
        self._destroy_engine()

    def _set_focal(self, idx, focal, force=False):
        if self.im_focals.requires_grad or force:
            with torch.no_grad():
                self.im_focals.data[idx] = float(self.focal_break * np.log(float(focal)))
        return self.im_focals[idx]

    def _set_principal_point(self, idx, pp, force=False):
        H, W = self.imshapes[idx]
        if self.im_pp.requires_grad or force:
            with torch.no_grad():
                self.im_pp.data[idx] = torch.as_tensor((np.asarray(to_numpy(pp), np.float32) - (W / 2, H / 2)) / 10, dtype=torch.float32)
        return self.im_pp[idx]

    def _set_depthmap(self, idx, depth, force=False):
        if self.im_depthmaps.requires_grad or force:
            with torch.no_grad():
                row = pad_views([depth], depth.device, depth.dtype, row=self.max_area)[0]
                self.im_depthmaps.data[idx] = row.log().nan_to_num(neginf=0).to(self.im_depthmaps.device)     # zero in the padding
        return self.im_depthmaps[idx]

    # ------------------------------------------------------------------ getters (optimizer.py:127-186) and engine binding: BasePCOptimizer's,
    # over the parameters themselves as the flat storage
    _flat_im_poses = property(lambda self: self.im_poses)
    _flat_im_depthmaps = property(lambda self: self.im_depthmaps)
    _flat_im_focals = property(lambda self: self.im_focals)
    _flat_im_pp = property(lambda self: self.im_pp)

    def get_known_focal_mask(self):
        return torch.tensor([not self.im_focals.requires_grad] * self.n_imgs)

    def _engine_setup(self):
        options = {_lib.ALIGNER_OPT_OPTIMIZE_PP: self.im_pp.requires_grad, _lib.ALIGNER_OPT_OPTIMIZE_ADAPTORS: self.pw_adaptors.requires_grad}
        return self.im_poses.requires_grad, self.im_focals.requires_grad, options, None
