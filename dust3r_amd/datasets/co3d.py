"""Preprocessed Co3d_v2 (the reference's dust3r/datasets/co3d.py, the dataset of its README evaluation command). Same layout on disk:
ROOT/selected_seqs_{split}.json = {object: {instance: [frame numbers]}}, ROOT/object/instance/images/frameNNNNNN.jpg + .npz
(camera_pose, camera_intrinsics, maximum_depth), depths/frameNNNNNN.jpg.geometric.png (16 bit, scaled by maximum_depth) and
masks/frameNNNNNN.png. Same pair combinations, mask_bg modes, +-4 index jitter and invalidation / retry logic, with the same draws
from the generator. Files are read with PIL (no cv2).

The invalidation table is state shared by every item: a frame found without valid depth is avoided from then on. Under the loader's
thread pool (as under the reference's worker processes, each with a table of its own) WHEN a frame becomes invalid depends on which
item met it first, so an epoch repeats bit for bit only on data without such frames, or once the table has settled."""
import json
import os.path as osp
import threading
from collections import deque

import numpy as np
import PIL.Image

from .base.base_stereo_view_dataset import BaseStereoViewDataset


def _imread(path, unchanged=False):
    with PIL.Image.open(path) as im:
        return np.asarray(im if unchanged else im.convert('RGB')).copy()


_FILES = dict(meta=('images', 'frame{:06n}.npz'), image=('images', 'frame{:06n}.jpg'), depth=('depths', 'frame{:06n}.jpg.geometric.png'),
              mask=('masks', 'frame{:06n}.png'))
MAX_STEP, STEP, FRAMES = 30, 5, 100      # pairs of the 100 frames around an object that are 5, 10, ..., 30 frames apart


class Co3d(BaseStereoViewDataset):
    def __init__(self, mask_bg=True, *args, ROOT, **kwargs):
        super().__init__(*args, **kwargs)
        if mask_bg not in (True, False, 'rand'):
            raise AssertionError(f"mask_bg is True, False or 'rand', got {mask_bg!r}")
        self.ROOT, self.mask_bg, self.dataset_label = ROOT, mask_bg, 'Co3d_v2'
        with open(osp.join(ROOT, f'selected_seqs_{self.split}.json')) as f:
            selected = json.load(f)
        self.scenes = {(obj, inst): frames for obj, insts in selected.items() for inst, frames in insts.items()}      # an object without instances adds nothing
        self.scene_list = list(self.scenes)
        self.combinations = [(i, i + d) for i in range(FRAMES) for d in range(1, MAX_STEP + 1) if d % STEP == 0 and i + d < FRAMES]
        self.invalidate = {scene: {} for scene in self.scene_list}      # per scene and resolution: frames found without valid depth
        self._invalidate_lock = threading.Lock()

    def __len__(self):
        return len(self.scene_list) * len(self.combinations)

    def _file(self, kind, obj, instance, view_idx):
        folder, name = _FILES[kind]
        return osp.join(self.ROOT, obj, instance, folder, name.format(view_idx))

    def _get_metadatapath(self, obj, instance, view_idx):
        return self._file('meta', obj, instance, view_idx)

    def _get_impath(self, obj, instance, view_idx):
        return self._file('image', obj, instance, view_idx)

    def _get_depthpath(self, obj, instance, view_idx):
        return self._file('depth', obj, instance, view_idx)

    def _get_maskpath(self, obj, instance, view_idx):
        return self._file('mask', obj, instance, view_idx)

    def _read_depthmap(self, depthpath, input_metadata):
        """16-bit PNG -> metres: the stored fraction of the frame's maximum_depth (a NaN maximum reads as 0)"""
        fraction = _imread(depthpath, unchanged=True).astype(np.float32) / 65535
        return fraction * np.nan_to_num(input_metadata['maximum_depth'])

    def _get_views(self, idx, resolution, rng):
        obj, instance = self.scene_list[idx // len(self.combinations)]
        image_pool = self.scenes[obj, instance]
        im1_idx, im2_idx = self.combinations[idx % len(self.combinations)]
        last = len(image_pool) - 1
        with self._invalidate_lock:
            invalid = self.invalidate[obj, instance].setdefault(resolution, [False] * len(image_pool))
        # draw order: the background choice ('rand' only), the jitter of view 2 then view 1, a direction per invalidated frame met
        mask_bg = (self.mask_bg == True) or (self.mask_bg == 'rand' and rng.choice(2))      # noqa: E712
        todo = deque(max(0, min(im_idx + rng.integers(-4, 5), last)) for im_idx in [im2_idx, im1_idx])
        views = []
        while len(todo) > 0:
            im_idx = todo.pop()
            if invalid[im_idx]:
                direction = 2 * rng.choice(2) - 1
                for offset in range(1, len(image_pool)):
                    tentative = (im_idx + direction * offset) % len(image_pool)
                    if not invalid[tentative]:
                        im_idx = tentative
                        break
            view_idx = image_pool[im_idx]
            impath = self._get_impath(obj, instance, view_idx)
            input_metadata = np.load(self._get_metadatapath(obj, instance, view_idx))
            camera_pose = input_metadata['camera_pose'].astype(np.float32)
            intrinsics = input_metadata['camera_intrinsics'].astype(np.float32)
            rgb_image = _imread(impath)
            depthmap = self._read_depthmap(self._get_depthpath(obj, instance, view_idx), input_metadata)
            if mask_bg:
                maskmap = _imread(self._get_maskpath(obj, instance, view_idx), unchanged=True).astype(np.float32)
                depthmap *= (maskmap / 255.0) > 0.1
            rgb_image, depthmap, intrinsics = self._crop_resize_if_necessary(rgb_image, depthmap, intrinsics, resolution, rng=rng, info=impath)
            if (depthmap > 0.0).sum() == 0:                  # no valid depth in the window: never use this frame again, take another
                invalid[im_idx] = True
                todo.append(im_idx)
                continue
            views.append(dict(img=rgb_image, depthmap=depthmap, camera_pose=camera_pose, camera_intrinsics=intrinsics,
                              dataset=self.dataset_label, label=osp.join(obj, instance), instance=osp.split(impath)[1]))
        return views
