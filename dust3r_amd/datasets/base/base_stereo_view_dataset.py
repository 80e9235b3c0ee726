"""Base class of the stereo-view datasets (the reference's dust3r/datasets/base/base_stereo_view_dataset.py), split in a host half and
a device half. A subclass overrides `_get_views(idx, resolution, rng)` and calls `_crop_resize_if_necessary` exactly as a reference
subclass does; what comes back is a pair of lazy handles (the source arrays plus a CropResizePlan), not pixels. `planned_views(idx)`
finishes the host half: the checks, `true_shape`, `idx`, the portrait permutation of the intrinsics and `view['rng']`, consuming the
generator exactly as the reference does. The pixels -- `img`, `depthmap`, `pts3d`, `valid_mask` -- are produced for a whole batch by
`prepare.prepare_views` (csrc/views.hip); `dataset[idx]` runs that path on its two views, the loader on the 2 B views of a batch."""
import threading

import numpy as np
import torch

from ..utils.cropping import nearest_indices, plan_crop_resize
from ..utils.transforms import ColorJitter, ImgNorm  # noqa: F401  (names a `transform=` string may evaluate to)
from .easy_dataset import EasyDataset


class LazyImage:
    """The source picture (uint8 H0 x W0 x 3) and the plan of its crop / resample / crop."""

    def __init__(self, source, plan):
        self.source, self.plan = source, plan

    @property
    def size(self):
        return self.plan.size


class LazyDepth:
    """The source depth map (fp32 H0 x W0) and the same plan. Comparisons are answered from the nearest-sampled depth on the host
    (one gather of the final window, cached), which is all a subclass needs to count valid pixels."""

    def __init__(self, source, plan):
        self.source, self.plan = source, plan
        self._sampled = None

    @property
    def shape(self):
        w, h = self.plan.size
        return (h, w)

    def sampled(self):
        if self._sampled is None:
            sy, sx = nearest_indices(self.plan)
            self._sampled = self.source[sy[:, None], sx[None, :]]
        return self._sampled

    def __gt__(self, other):
        return self.sampled() > other


class BaseStereoViewDataset(EasyDataset):
    def __init__(self, *, split=None, resolution=None, transform=ImgNorm, aug_crop=False, seed=None):
        self.num_views = 2
        self.split = split
        self._set_resolutions(resolution)
        if isinstance(transform, str):
            transform = eval(transform)
        if transform is not ImgNorm:
            raise NotImplementedError(f'transform={transform!r}: ImgNorm is the only transform executed (ColorJitter is a training augmentation)')
        self.transform = transform
        self.aug_crop = aug_crop
        self.seed = seed
        self._rng_lock = threading.Lock()

    def __len__(self):
        return len(self.scenes)

    def get_stats(self):
        return f'{len(self)} pairs'

    def __repr__(self):
        resolutions_str = '[' + ';'.join(f'{w}x{h}' for w, h in self._resolutions) + ']'
        text = (f'{type(self).__name__}({self.get_stats()},split={self.split!r},seed={self.seed!r},resolutions={resolutions_str},'
                f'transform={self.transform!r})')
        return text.replace('\n', '').replace('   ', '')

    def _get_views(self, idx, resolution, rng):
        raise NotImplementedError()

    def _set_resolutions(self, resolutions):
        assert resolutions is not None, 'undefined resolution'
        def as_pair(resolution):      # an int is a square; a pair is (width, height), landscape
            pair = (resolution,) * 2 if isinstance(resolution, int) else tuple(resolution)
            assert len(pair) == 2 and all(isinstance(x, int) for x in pair), f'a resolution is an int or (width, height) ints, got {resolution!r}'
            assert pair[0] >= pair[1], f'resolutions are landscape, got {pair}'
            return pair
        self._resolutions = [as_pair(r) for r in (resolutions if isinstance(resolutions, list) else [resolutions])]

    def _crop_resize_if_necessary(self, image, depthmap, intrinsics, resolution, rng=None, info=None):
        """(image, depthmap, intrinsics2) as subclasses expect; image and depthmap are lazy handles that share one plan."""
        image = np.asarray(image, dtype=np.uint8)
        assert image.ndim == 3 and image.shape[2] == 3 and tuple(depthmap.shape[:2]) == image.shape[:2], f'bad picture / depth map in view={info}'
        plan = plan_crop_resize((image.shape[1], image.shape[0]), intrinsics, resolution, aug_crop=self.aug_crop, rng=rng)
        return LazyImage(image, plan), LazyDepth(np.asarray(depthmap, dtype=np.float32), plan), plan.intrinsics

    def planned_views(self, idx):
        """The host half of `dataset[idx]`: every key of the finished views except the pixel outputs, with `img` / `depthmap` still lazy."""
        if isinstance(idx, tuple):
            idx, ar_idx = int(idx[0]), int(idx[1])
        else:
            assert len(self._resolutions) == 1, 'a dataset with several resolutions is indexed with (idx, resolution index)'
            idx, ar_idx = int(idx), 0
        resolution = self._resolutions[ar_idx]
        if self.seed:                        # reseeded per item: a generator of its own, so items can be prepared on several threads
            return self._planned_views(idx, ar_idx, resolution, np.random.default_rng(seed=self.seed + idx))
        with self._rng_lock:                 # one generator for the life of the dataset: items take turns
            if not hasattr(self, '_rng'):
                self._rng = np.random.default_rng(seed=torch.initial_seed())
            return self._planned_views(idx, ar_idx, resolution, self._rng)

    def _planned_views(self, idx, ar_idx, resolution, rng):
        views = self._get_views(idx, resolution, rng)
        assert len(views) == self.num_views
        for v, view in enumerate(views):
            assert 'pts3d' not in view, f'pts3d should not be there, they will be computed afterwards based on intrinsics+depthmap for view {view_name(view)}'
            assert 'valid_mask' not in view
            assert isinstance(view['img'], LazyImage) and isinstance(view['depthmap'], LazyDepth), 'views come from _crop_resize_if_necessary'
            view['idx'] = (idx, ar_idx, v)
            width, height = view['img'].size
            view['true_shape'] = np.int32((height, width))
            assert 'camera_intrinsics' in view
            if 'camera_pose' not in view:
                view['camera_pose'] = np.full((4, 4), np.nan, dtype=np.float32)
            else:
                assert np.isfinite(view['camera_pose']).all(), f'NaN in camera pose for view {view_name(view)}'
            assert np.isfinite(view['depthmap'].sampled()).all(), f'NaN in depthmap for view {view_name(view)}'
            K = np.float32(view['camera_intrinsics'])
            assert K[0, 1] == 0.0 and K[1, 0] == 0.0, f'skew in the intrinsics of view {view_name(view)}'
            view['K_pixels'] = K                  # the intrinsics the back-projection uses (before the portrait permutation)
            for key, val in view.items():
                if key not in ('img', 'depthmap'):
                    res, err_msg = is_good_type(key, val)
                    assert res, f'{err_msg} with {key}={val} for view {view_name(view)}'
        for view in views:
            height, width = view['true_shape']
            if width < height:                    # portrait views are stored transposed: rows and columns of the intrinsics swap too
                view['camera_intrinsics'] = view['camera_intrinsics'][[1, 0, 2]]
            view['rng'] = int.from_bytes(rng.bytes(4), 'big')
        return views

    def plan(self, idx):
        """`dataset[idx]` without the pixel outputs (host only): `plan` holds each view's CropResizePlan."""
        views = self.planned_views(idx)
        for view in views:
            view['plan'] = view.pop('img').plan
            del view['depthmap'], view['K_pixels']
        return views

    def __getitem__(self, idx):
        from ..prepare import prepare_views
        views = self.planned_views(idx)
        prepare_views(views)
        return views


_ARRAY_DTYPES = (np.float32, torch.float32, bool, np.int32, np.int64, np.uint8)


def is_good_type(key, v):
    """(ok, message): view values are strings, ints, tuples or arrays / tensors of the dtypes the collation keeps"""
    ok = isinstance(v, (str, int, tuple)) or v.dtype in _ARRAY_DTYPES
    return ok, None if ok else f'bad {v.dtype=}'


def view_name(view, batch_index=None):
    """'dataset/label/instance' of a view, or of row `batch_index` of a collated one"""
    whole = batch_index is None or batch_index == slice(None)
    return '/'.join(str(view[key] if whole else view[key][batch_index]) for key in ('dataset', 'label', 'instance'))


_TRANSPOSED = (('img', (1, 2)), ('valid_mask', (0, 1)), ('depthmap', (0, 1)), ('pts3d', (0, 1)))      # key, the axes (row, column)


def transpose_to_landscape(view):
    """A finished portrait view with (height, width) arrays -> rows and columns swapped, as the kernels store it, and the first two
    rows of the intrinsics with them."""
    height, width = view['true_shape']
    if width >= height:
        return
    for key, (row, col) in _TRANSPOSED:
        assert (view[key].shape[row], view[key].shape[col]) == (height, width), f'{key} is not {height} x {width}'
        view[key] = view[key].swapaxes(row, col)
    view['camera_intrinsics'] = view['camera_intrinsics'][[1, 0, 2]]
