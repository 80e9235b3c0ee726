"""Seeded RGB-D views for the dataset tests, fixtures and tools/dataset_speed.py: every value is an integer hash of (seed, stream,
index), so every machine produces the same bytes (no library random generator, no transcendental function)."""
import numpy as np

from .base.base_stereo_view_dataset import BaseStereoViewDataset


def _hash32(seed, stream, n):
    x = np.arange(n, dtype=np.uint64) + np.uint64((seed * 0x9E3779B1 + stream * 0x85EBCA77 + 0x165667B1) & 0xFFFFFFFF)
    x &= np.uint64(0xFFFFFFFF)
    for mul, sh in ((0x85EBCA6B, 16), (0xC2B2AE35, 13), (0x27D4EB2F, 16)):
        x ^= x >> np.uint64(sh)
        x = (x * np.uint64(mul)) & np.uint64(0xFFFFFFFF)
    return x ^ (x >> np.uint64(16))


def synthetic_view(seed, W, H, pp=(0.5, 0.5), holes=0.1):
    """dict(rgb uint8 (H, W, 3): a smooth pattern plus noise; depth fp32 (H, W) in [1, 4) with about `holes` of the pixels at 0; K fp32
    with the principal point at `pp` (fractions of the size); pose fp32 cam2world: a 3-4-5 rotation about z plus a translation)."""
    f32 = np.float32
    yy, xx = np.mgrid[0:H, 0:W]
    noise = (_hash32(seed, 1, H * W * 3) >> np.uint64(26)).reshape(H, W, 3).astype(np.int64)
    rgb = ((xx[..., None] * (np.arange(3) + 2) + yy[..., None] * (3 - np.arange(3)) + noise) & 255).astype(np.uint8)
    u = (_hash32(seed, 2, H * W) >> np.uint64(8)).astype(np.float32) * f32(2.0 ** -24)
    depth = (f32(1.0) + f32(3.0) * u).reshape(H, W)
    hole = (_hash32(seed, 3, H * W) >> np.uint64(8)).astype(np.float32) * f32(2.0 ** -24) < f32(holes)
    depth[hole.reshape(H, W)] = 0
    K = np.eye(3, dtype=np.float32)
    K[0, 0] = K[1, 1] = f32(1.25) * f32(max(W, H))
    K[0, 2], K[1, 2] = f32(pp[0] * W), f32(pp[1] * H)
    pose = np.eye(4, dtype=np.float32)
    pose[0, 0], pose[0, 1], pose[1, 0], pose[1, 1] = f32(0.6), f32(-0.8), f32(0.8), f32(0.6)
    pose[:3, 3] = ((_hash32(seed, 4, 3) >> np.uint64(8)).astype(np.float32) * f32(2.0 ** -24) - f32(0.5)) * f32(4.0)
    return dict(rgb=rgb, depth=depth.astype(np.float32), K=K, pose=pose)


class SyntheticViewsMixin:
    """`_get_views` over generated sources, written against the base-class interface only, so the fixture tool can put it in front of
    the reference's base class as well. `sources` is a list of (W, H, principal point); pair idx takes entries 2 idx and 2 idx + 1."""

    def _init_sources(self, sources, n_pairs, in_memory=False):
        self.sources, self.scenes = list(sources), list(range(n_pairs))
        self._memory = {} if in_memory else None

    def _source(self, idx, v):
        W, H, pp = self.sources[(2 * idx + v) % len(self.sources)]
        if self._memory is None:
            return synthetic_view(1000 + 2 * idx + v, W, H, pp)
        key = (2 * idx + v) % max(len(self.sources), 2)
        if key not in self._memory:
            self._memory[key] = synthetic_view(1000 + key, W, H, pp)
        return self._memory[key]

    def _get_views(self, idx, resolution, rng):
        views = []
        for v in range(2):
            src = self._source(idx, v)
            image, depthmap, intrinsics = self._crop_resize_if_necessary(src['rgb'], src['depth'], src['K'], resolution, rng=rng, info=(idx, v))
            views.append(dict(img=image, depthmap=depthmap, camera_pose=src['pose'], camera_intrinsics=intrinsics, dataset='Synthetic',
                              label=f'pair{idx}', instance=f'view{v}'))
        return views


class SyntheticStereo(SyntheticViewsMixin, BaseStereoViewDataset):
    def __init__(self, sources, n_pairs, in_memory=False, **kwargs):
        super().__init__(**kwargs)
        self._init_sources(sources, n_pairs, in_memory)
