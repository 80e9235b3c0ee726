"""Seeded pairs WITH ground truth for the criterion tests and tools/loss_speed.py. Every number is an integer hash of (seed, stream,
index) scaled by a power of two and combined by single fp32 additions and multiplications in a fixed order, so every machine produces
the same bits (no transcendental function, no BLAS, no library random generator)."""
import zlib

import numpy as np
import torch


def _hash01(seed, stream, shape):
    """fp32 in [0, 1): the top 24 bits of a 32-bit mix of (seed, stream, index), times 2^-24 (exact)."""
    n = int(np.prod(shape))
    x = np.arange(n, dtype=np.uint64) + np.uint64((seed * 0x9E3779B1 + stream * 0x85EBCA77 + 0x165667B1) & 0xFFFFFFFF)
    x &= np.uint64(0xFFFFFFFF)
    for mul, sh in ((0x85EBCA6B, 16), (0xC2B2AE35, 13), (0x27D4EB2F, 16)):      # products of 32-bit values fit 64 bits
        x ^= x >> np.uint64(sh)
        x = (x * np.uint64(mul)) & np.uint64(0xFFFFFFFF)
    x ^= x >> np.uint64(16)
    return ((x >> np.uint64(8)).astype(np.float32) * np.float32(2.0 ** -24)).reshape(shape)


def _camera_points(seed, stream, B, H, W):
    """A bumpy surface in front of a camera: depth in [1.5, 3.5), x and y from the pixel rays."""
    f32 = np.float32
    z = f32(1.5) + f32(2.0) * _hash01(seed, stream, (B, H, W))
    u = ((np.arange(W, dtype=np.float32) + f32(0.5)) * f32(1.0 / W) - f32(0.5))[None, None, :]
    v = ((np.arange(H, dtype=np.float32) + f32(0.5)) * f32(1.0 / H) - f32(0.5))[None, :, None]
    return np.stack((u * z, v * z, z), axis=-1).astype(np.float32)


def _apply(R, t, p):
    """R p + t with one fp32 product / sum per step, in a fixed order"""
    return np.stack([(p[..., 0] * R[:, i, 0, None, None] + p[..., 1] * R[:, i, 1, None, None]) + p[..., 2] * R[:, i, 2, None, None]
                     + t[:, i, None, None] for i in range(3)], axis=-1).astype(np.float32)


def gt_pairs(B, H, W, seed=0, invalid=0.3, empty_view2=(), scale=1.7, noise=0.1):
    """(view1, view2, pred1, pred2) of B pairs in the reference's collated format. Views: `img` (B, 3, H, W) in [-1, 1), `pts3d` world
    points, `camera_pose` (view 1: a 3-4-5 rotation about z plus a translation), `valid_mask` (about `invalid` of the pixels off; all of
    view 2 off for the pairs in `empty_view2`), `true_shape`. Predictions: the ground truth in camera 1's frame times `scale` plus
    uniform noise of width `noise`, `conf` in [1, 6)."""
    f32 = np.float32
    cam = [_camera_points(seed, 1, B, H, W), _camera_points(seed, 2, B, H, W)]
    cam[1][..., 0] += f32(0.25)                                   # view 2 looks at a shifted patch
    R = np.zeros((B, 3, 3), np.float32)
    R[:, 0, 0], R[:, 0, 1], R[:, 1, 0], R[:, 1, 1], R[:, 2, 2] = f32(0.6), f32(-0.8), f32(0.8), f32(0.6), f32(1.0)
    t = (_hash01(seed, 3, (B, 3)) - f32(0.5)) * f32(4.0)
    pose1 = np.tile(np.eye(4, dtype=np.float32), (B, 1, 1))
    pose1[:, :3, :3], pose1[:, :3, 3] = R, t
    pose2 = pose1.copy()
    pose2[:, 0, 3] += f32(0.25)
    views, preds = [], []
    for k in (0, 1):
        valid = _hash01(seed, 4 + k, (B, H, W)) >= f32(invalid)
        if k == 1:
            for b in empty_view2:
                valid[b] = False
        views.append(dict(img=torch.from_numpy(_hash01(seed, 6 + k, (B, 3, H, W)) * f32(2.0) - f32(1.0)),
                          pts3d=torch.from_numpy(_apply(R, t, cam[k])), camera_pose=torch.from_numpy(pose1 if k == 0 else pose2),
                          valid_mask=torch.from_numpy(valid), true_shape=torch.tensor([[H, W]] * B, dtype=torch.int32)))
        pts = cam[k] * f32(scale) + (_hash01(seed, 8 + k, (B, H, W, 3)) - f32(0.5)) * f32(noise)
        conf = f32(1.0) + f32(5.0) * _hash01(seed, 10 + k, (B, H, W))
        preds.append({'pts3d' if k == 0 else 'pts3d_in_other_view': torch.from_numpy(pts.astype(np.float32)), 'conf': torch.from_numpy(conf)})
    return views[0], views[1], preds[0], preds[1]


def checksum(*dicts):
    """crc32 over the bytes of every tensor of the given dicts (keys in sorted order)"""
    crc = 0
    for d in dicts:
        for key in sorted(d):
            crc = zlib.crc32(d[key].contiguous().numpy().tobytes(), crc)
    return crc
