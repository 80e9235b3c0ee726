"""scene.fuse() without a GPU: the numpy restatement of the voxel fusion (csrc/fuse.hip; tests/test_fuse_gpu.py holds the kernels to it
exactly), held itself by hand-worked cases; the default voxel size; the key-size and voxel-size guards; the PLY writer and reader; the COLMAP
writer, both encodings, parsed back by the small reader below."""
import os
import re
import struct

import numpy as np
import pytest
import torch

from test_glb_cpu import restated_q


# ---- restatement --------------------------------------------------------------------------------------------------------------------
def restated_fuse(imgs, pts, masks, weights, voxel_size, min_count=1):
    """imgs / pts / masks / weights: per view (H, W, 3) / (H, W, 3) / (H, W) / (H, W) arrays (weights None: ones). A pixel is valid when its
    mask is set, its point finite and its weight finite and > 0. Valid pixels, views in order then raster order, get the voxel
    floor((p - lo) / voxel) in float32 (lo = their minimum), packed into an int64 key with bit_length(floor((hi - lo) / voxel)) bits per axis;
    a stable sort by key; per run of equal keys float64 sums in that order (np.bincount adds in input order): W = sum w, S = sum w p,
    C = sum w q. Returns positions = float32(S / W), colors = floor(C / W + 1/2) clamped, weight = float32(W), count, bounds, bits."""
    P = np.concatenate([np.asarray(p, np.float32).reshape(-1, 3) for p in pts])
    m = np.concatenate([np.asarray(k).reshape(-1) != 0 for k in masks])
    w = np.ones(len(P), np.float32) if weights is None else np.concatenate([np.asarray(k, np.float32).reshape(-1) for k in weights])
    q = np.concatenate([restated_q(im).reshape(-1, 3) for im in imgs])
    valid = m & np.isfinite(P).all(axis=1) & np.isfinite(w) & (w > 0)
    P, w, q = P[valid], w[valid], q[valid]
    v = np.float32(voxel_size)
    if len(P) == 0:
        inf = np.full(3, np.inf, np.float32)
        return dict(positions=np.zeros((0, 3), np.float32), colors=np.zeros((0, 3), np.uint8), weight=np.zeros(0, np.float32),
                    count=np.zeros(0, np.int32), bounds=(inf, -inf), bits=None, n_valid=0)
    lo, hi = P.min(axis=0), P.max(axis=0)
    cell = np.floor((P - lo) / v)
    assert cell.dtype == np.float32
    bits = [max(1, int(e).bit_length()) for e in np.floor((hi - lo) / v)]
    assert max(bits) <= 21
    c = cell.astype(np.int64)
    key = c[:, 0] | (c[:, 1] << bits[0]) | (c[:, 2] << (bits[0] + bits[1]))
    order = np.argsort(key, kind='stable')
    ks = key[order]
    seg = np.cumsum(np.r_[True, ks[1:] != ks[:-1]]) - 1
    wd = w[order].astype(np.float64)
    W = np.bincount(seg, weights=wd)
    S = np.stack([np.bincount(seg, weights=wd * P[order, k].astype(np.float64)) for k in range(3)], axis=1)
    C = np.stack([np.bincount(seg, weights=wd * q[order, k].astype(np.float64)) for k in range(3)], axis=1)
    out = dict(positions=(S / W[:, None]).astype(np.float32), colors=np.clip(np.floor(C / W[:, None] + 0.5), 0, 255).astype(np.uint8),
               weight=W.astype(np.float32), count=np.bincount(seg).astype(np.int32))
    if min_count > 1:
        keep = out['count'] >= min_count
        out = {k: a[keep] for k, a in out.items()}
    return dict(out, bounds=(lo, hi), bits=bits, n_valid=len(P))


def check_cloud(cloud, want):
    """a viz.FusedCloud against the restatement: the same bytes"""
    from dust3r_amd.viz import _to_numpy
    got = {k: _to_numpy(getattr(cloud, k)) for k in ('positions', 'colors', 'weight', 'count')}
    assert len(cloud) == len(want['positions'])
    for k, dt, tail in (('positions', np.float32, (3,)), ('colors', np.uint8, (3,)), ('weight', np.float32, ()), ('count', np.int32, ())):
        assert got[k].dtype == dt and got[k].shape == (len(want[k]),) + tail, k
        assert np.array_equal(got[k], want[k]), k
    assert np.array_equal(cloud.bounds[0], want['bounds'][0]) and np.array_equal(cloud.bounds[1], want['bounds'][1])
    assert np.array_equal(cloud.origin, want['bounds'][0])


def _one_view(points, colors, weights=None, mask=None):
    n = len(points)
    return dict(imgs=[np.asarray(colors, np.uint8).reshape(1, n, 3)], pts=[np.asarray(points, np.float32).reshape(1, n, 3)],
                masks=[np.ones((1, n), bool) if mask is None else np.asarray(mask, bool).reshape(1, n)],
                weights=None if weights is None else [np.asarray(weights, np.float32).reshape(1, n)])


# ---- the restatement itself, by hand ----------------------------------------------------------------------------------------------------
def test_two_points_in_one_voxel_weights_1_and_3():
    s = _one_view([(0, 0, 0), (0.5, 0.25, 0), (2.5, 2.5, 2.5)], [(10, 20, 30), (50, 60, 70), (1, 2, 3)], [1, 3, 2])
    r = restated_fuse(s['imgs'], s['pts'], s['masks'], s['weights'], 1.0)
    assert r['positions'].tolist() == [[0.375, 0.1875, 0.0], [2.5, 2.5, 2.5]]
    assert r['colors'].tolist() == [[40, 50, 60], [1, 2, 3]]
    assert r['weight'].tolist() == [4.0, 2.0] and r['count'].tolist() == [2, 1]
    assert r['bits'] == [2, 2, 2] and r['n_valid'] == 3


def test_a_point_on_a_voxel_face_belongs_to_the_upper_voxel():
    below = np.nextafter(np.float32(1), np.float32(0))
    s = _one_view([(0, 0, 0), (below, 0, 0), (1, 0, 0), (2, 0, 0)], [(0, 0, 0)] * 4)
    r = restated_fuse(s['imgs'], s['pts'], s['masks'], None, 1.0)
    assert r['count'].tolist() == [2, 1, 1]
    assert r['positions'][:, 0].tolist() == [float(np.float32(np.float64(below) / 2)), 1.0, 2.0]
    assert r['bits'] == [2, 1, 1]


def test_negative_coordinates_count_from_the_minimum():
    s = _one_view([(-2.5, -1, -7), (-1.625, -1, -7), (-1.5, -1, -7), (-0.25, -1, -7)], [(9, 9, 9)] * 4)
    r = restated_fuse(s['imgs'], s['pts'], s['masks'], None, 1.0)
    assert r['count'].tolist() == [2, 1, 1]                       # floors 0, 0 (0.875), 1, 2 of (x + 2.5)
    assert r['positions'].tolist() == [[-2.0625, -1.0, -7.0], [-1.5, -1.0, -7.0], [-0.25, -1.0, -7.0]]
    assert r['bounds'][0].tolist() == [-2.5, -1.0, -7.0]


def test_nan_points_bad_weights_and_masked_pixels_are_dropped():
    pts = [(0, 0, 0), (np.nan, 0, 0), (0.5, 0.5, 0.5), (0.25, 0.25, 0.25), (0, np.inf, 0), (0.75, 0, 0), (100, 100, 100), (0.5, 0, 0), (0.1, 0, 0)]
    w = [1, 1, 0, 1, 1, np.nan, 1, -2, np.inf]
    mask = [1, 1, 1, 1, 1, 1, 0, 1, 1]
    s = _one_view(pts, [(200, 100, 0)] * 9, w, mask)
    r = restated_fuse(s['imgs'], s['pts'], s['masks'], s['weights'], 1.0)
    assert r['n_valid'] == 2 and r['count'].tolist() == [2]           # points 0 and 3 are left; the masked far point moves no bound
    assert r['positions'].tolist() == [[0.125, 0.125, 0.125]] and r['bounds'][1].tolist() == [0.25, 0.25, 0.25]
    assert r['colors'].tolist() == [[200, 100, 0]]
    none = restated_fuse(s['imgs'], s['pts'], [np.zeros((1, 9), bool)], s['weights'], 1.0)
    assert len(none['positions']) == 0 and none['bounds'][0].tolist() == [np.inf] * 3 and none['bounds'][1].tolist() == [-np.inf] * 3


def test_colour_means_round_half_up():
    s = _one_view([(0, 0, 0), (0.5, 0, 0), (5, 0, 0), (5.5, 0, 0)], [(10, 0, 254), (11, 1, 255), (7, 7, 7), (8, 8, 8)], [1, 1, 3, 1])
    r = restated_fuse(s['imgs'], s['pts'], s['masks'], s['weights'], 1.0)
    assert r['colors'].tolist() == [[11, 1, 255], [7, 7, 7]]            # 10.5 -> 11, 0.5 -> 1, 254.5 -> 255; 7.25 -> 7


def test_float_images_use_the_export_colour_rule_and_min_count():
    img = np.float32([[(0.0, 1.0, 0.25), (0.5, 0.999, 0.2)]])                        # 63.75 + 0.5 -> 64; 127.5 + 0.5 -> 128; 254.745...; 51.0...
    r = restated_fuse([img], [np.float32([[(0, 0, 0), (3, 0, 0)]])], [np.ones((1, 2), bool)], None, 1.0)
    assert r['colors'].tolist() == [[0, 255, 64], [128, 255, 51]]
    s = _one_view([(0, 0, 0), (0.5, 0, 0), (5, 0, 0)], [(1, 1, 1)] * 3)
    r = restated_fuse(s['imgs'], s['pts'], s['masks'], None, 1.0, min_count=2)
    assert r['count'].tolist() == [2] and r['positions'].tolist() == [[0.25, 0, 0]]


def test_bincount_adds_in_input_order():
    """what the restatement relies on: the float64 sums of np.bincount are the sequential sums"""
    rng = np.random.default_rng(0)
    seg = np.sort(rng.integers(0, 50, size=2000))
    x = rng.normal(size=2000) * 10.0 ** rng.integers(-8, 8, size=2000)
    want = np.zeros(50)
    for s, v in zip(seg, x):
        want[s] += v
    assert np.array_equal(np.bincount(seg, weights=x, minlength=50), want)


# ---- the rules of viz.py ------------------------------------------------------------------------------------------------------------------
def test_default_voxel_is_the_median_pixel_footprint():
    from dust3r_amd.viz import default_voxel_size
    depth = torch.full((4, 8), 1e9)                                    # the padding must not enter
    depth[0, :4] = torch.tensor([4.0, 1.0, 3.0, 2.0])                 # lower median 2
    depth[1, :6] = torch.tensor([5.0, 1.0, 3.0, 2.0, 4.0, 6.0])       # 3
    depth[2, :4] = torch.tensor([8.0, 8.0, 9.0, 7.0])                 # 8
    depth[3, :5] = torch.tensor([1.0, 1.0, 5.0, 9.0, 9.0])            # 5
    assert default_voxel_size(depth, [4, 6, 4, 5], torch.tensor([2.0, 4.0, 2.0, 10.0])) == 0.75       # 1, 0.75, 4, 0.5 -> lower median of four
    fxy = torch.tensor([[1.0, 3.0], [2.0, 6.0], [1.0, 3.0], [10.0, 10.0]])                              # fx_and_fy: the mean
    assert default_voxel_size(depth, [4, 6, 4, 5], fxy) == 0.75
    assert default_voxel_size(depth[:3], [4, 6, 4], [[2.0], [4.0], [2.0]]) == 1.0                       # odd count: the middle


@pytest.mark.parametrize('bad', [0.0, -1.0, float('nan'), float('inf'), 1e-45, 1e-39, 1e39])
def test_voxel_size_must_be_a_normal_positive_float32(bad):
    from dust3r_amd.viz import check_voxel_size, fuse_points
    with pytest.raises(ValueError, match='normal positive float32'):
        check_voxel_size(bad)
    with pytest.raises(ValueError, match='normal positive float32'):      # before the device is asked for
        fuse_points([np.zeros((1, 1, 3), np.uint8)], [np.zeros((1, 1, 3), np.float32)], [np.ones((1, 1), bool)], None, bad, 'cuda')
    assert check_voxel_size(np.finfo(np.float32).tiny) == np.finfo(np.float32).tiny


def test_key_bits_and_the_extent_guard():
    from dust3r_amd.viz import fuse_key_bits
    lo = np.float32([0, -1, 5])
    assert fuse_key_bits(lo, np.float32([0, -1, 5]), 0.5) == [1, 1, 1]
    assert fuse_key_bits(lo, np.float32([0.75, 0, 9]), 0.25) == [2, 3, 5]            # floors 3, 4, 16
    assert fuse_key_bits(lo, np.float32([2 ** 21 - 1, -1, 5]), 1.0) == [21, 1, 1]
    for hi, v in (([2 ** 21, -1, 5], 1.0), ([1, 0, 6], 1e-7), ([3e38, 0, 6], 1.0), ([0, 3e38, 6], 1e-30)):
        with pytest.raises(ValueError, match="voxel_size too small for the scene's extent"):
            fuse_key_bits(lo, np.float32(hi), v)
    lo2, hi2 = np.float32([-3e38, 0, 0]), np.float32([3e38, 0, 0])                     # the extent overflows float32
    with pytest.raises(ValueError, match="voxel_size too small for the scene's extent"):
        fuse_key_bits(lo2, hi2, 1e30)


# ---- PLY ----------------------------------------------------------------------------------------------------------------------------------
def _cloud_arrays(rng, n):
    return (rng.normal(size=(n, 3)).astype(np.float32), rng.integers(0, 256, size=(n, 3)).astype(np.uint8),
            rng.random(n).astype(np.float32) * 9, rng.integers(1, 50, size=n).astype(np.int32))


@pytest.mark.parametrize('n', [0, 1, 1000])
def test_ply_round_trip(tmp_path, n):
    from dust3r_amd.export import read_ply, write_ply
    pos, col, wgt, cnt = _cloud_arrays(np.random.default_rng(n), n)
    if n:
        pos[0] = [np.float32(-0.0), np.finfo(np.float32).max, np.finfo(np.float32).tiny]
    path = str(tmp_path / 'a.ply')
    assert write_ply(path, pos, col, wgt, cnt) == path
    raw = open(path, 'rb').read()
    head = raw[:raw.index(b'end_header\n')].decode('ascii').split('\n')
    assert head[:2] == ['ply', 'format binary_little_endian 1.0'] and f'element vertex {n}' in head
    assert [ln for ln in head if ln.startswith('property')] == ['property float x', 'property float y', 'property float z', 'property uchar red',
                                                                'property uchar green', 'property uchar blue', 'property float confidence', 'property int count']
    assert len(raw) == raw.index(b'end_header\n') + 11 + n * 23
    got = read_ply(path)
    assert got['positions'].tobytes() == pos.tobytes() and got['positions'].shape == (n, 3) and got['positions'].dtype == np.float32
    assert np.array_equal(got['colors'], col) and got['colors'].dtype == np.uint8 and got['colors'].shape == (n, 3)
    assert got['confidence'].tobytes() == wgt.tobytes() and got['count'].tobytes() == cnt.tobytes() and got['count'].dtype == np.int32
    write_ply(path, pos, np.c_[col, np.full((n, 1), 255, np.uint8)])                 # RGBA in, no optional columns
    got = read_ply(path)
    assert sorted(got) == ['colors', 'positions'] and np.array_equal(got['colors'], col) and got['positions'].tobytes() == pos.tobytes()
    assert os.path.getsize(path) == open(path, 'rb').read().index(b'end_header\n') + 11 + n * 15


def test_ply_rejects_other_dialects_and_bad_lengths(tmp_path):
    from dust3r_amd.export import read_ply, write_ply
    path = str(tmp_path / 'b.ply')
    with pytest.raises(ValueError, match='values of confidence'):
        write_ply(path, np.zeros((2, 3), np.float32), np.zeros((2, 3), np.uint8), weight=np.zeros(3, np.float32))
    open(path, 'w').write('ply\nformat ascii 1.0\nelement vertex 0\nproperty float x\nend_header\n')
    with pytest.raises(ValueError, match='binary little-endian'):
        read_ply(path)
    write_ply(path, np.zeros((2, 3), np.float32), np.zeros((2, 3), np.uint8))
    open(path, 'ab').write(b'\0')
    with pytest.raises(ValueError, match='bytes of data'):
        read_ply(path)


def test_fused_cloud_object_and_save_ply(tmp_path):
    from dust3r_amd.export import read_ply
    from dust3r_amd.viz import FusedCloud
    pos, col, wgt, cnt = _cloud_arrays(np.random.default_rng(3), 17)
    lo, hi = pos.min(0), pos.max(0)
    for wrap in (lambda a: a, torch.from_numpy):
        cloud = FusedCloud(wrap(pos), wrap(col), wrap(wgt), wrap(cnt), np.float32(0.125), (lo, hi))
        assert len(cloud) == 17 and cloud.voxel_size == 0.125 and cloud.origin is lo and cloud.bounds == (lo, hi)
        got = read_ply(cloud.save_ply(str(tmp_path / 'c.ply')))
        assert got['positions'].tobytes() == pos.tobytes() and np.array_equal(got['colors'], col)
        assert got['confidence'].tobytes() == wgt.tobytes() and np.array_equal(got['count'], cnt)


# ---- COLMAP -------------------------------------------------------------------------------------------------------------------------------
def read_colmap(sparse, binary):
    """cameras / images / points3D of a COLMAP model directory, either encoding -> (cameras, images, points): lists of dicts"""
    cams, imgs, pts = [], [], []
    if binary:
        raw = open(os.path.join(sparse, 'cameras.bin'), 'rb').read()
        (n,), o = struct.unpack_from('<Q', raw), 8
        for _ in range(n):
            cid, model, w, h = struct.unpack_from('<iiQQ', raw, o)
            cams.append(dict(id=cid, model=model, width=w, height=h, params=struct.unpack_from('<4d', raw, o + 24)))
            o += 24 + 32
        assert o == len(raw)
        raw = open(os.path.join(sparse, 'images.bin'), 'rb').read()
        (n,), o = struct.unpack_from('<Q', raw), 8
        for _ in range(n):
            iid, *qt = struct.unpack_from('<i7d', raw, o)
            (cid,) = struct.unpack_from('<i', raw, o + 60)
            end = raw.index(b'\0', o + 64)
            (n2d,) = struct.unpack_from('<Q', raw, end + 1)
            imgs.append(dict(id=iid, q=qt[:4], t=qt[4:], camera_id=cid, name=raw[o + 64:end].decode('utf-8'), n2d=n2d))
            o = end + 1 + 8 + 24 * n2d
        assert o == len(raw)
        raw = open(os.path.join(sparse, 'points3D.bin'), 'rb').read()
        (n,), o = struct.unpack_from('<Q', raw), 8
        for _ in range(n):
            pid, x, y, z, r, g, b, err, track = struct.unpack_from('<Q3d3BdQ', raw, o)
            pts.append(dict(id=pid, xyz=(x, y, z), rgb=(r, g, b), error=err, track=track))
            o += 51 + 8 * track
        assert o == len(raw)
        return cams, imgs, pts
    model_ids = {'PINHOLE': 1}
    lines = open(os.path.join(sparse, 'cameras.txt')).read().split('\n')
    assert lines[0].startswith('# Camera list') and lines[-1] == ''
    for ln in (x for x in lines[:-1] if not x.startswith('#')):
        f = ln.split()
        cams.append(dict(id=int(f[0]), model=model_ids[f[1]], width=int(f[2]), height=int(f[3]), params=tuple(float(v) for v in f[4:])))
    assert int(re.search(r'# Number of cameras: (\d+)', '\n'.join(lines)).group(1)) == len(cams)
    lines = open(os.path.join(sparse, 'images.txt')).read().split('\n')
    assert lines[0].startswith('# Image list') and lines[-1] == ''
    body = [x for x in lines[:-1] if not x.startswith('#')]
    assert len(body) % 2 == 0
    for first, second in zip(body[::2], body[1::2]):
        f = first.split()
        imgs.append(dict(id=int(f[0]), q=[float(v) for v in f[1:5]], t=[float(v) for v in f[5:8]], camera_id=int(f[8]), name=f[9], n2d=len(second.split()) // 3))
    assert int(re.search(r'# Number of images: (\d+)', '\n'.join(lines)).group(1)) == len(imgs)
    lines = open(os.path.join(sparse, 'points3D.txt')).read().split('\n')
    assert lines[0].startswith('# 3D point list') and lines[-1] == ''
    for ln in (x for x in lines[:-1] if not x.startswith('#')):
        f = ln.split()
        pts.append(dict(id=int(f[0]), xyz=tuple(float(v) for v in f[1:4]), rgb=tuple(int(v) for v in f[4:7]), error=float(f[7]), track=(len(f) - 8) // 2))
    assert int(re.search(r'# Number of points: (\d+)', '\n'.join(lines)).group(1)) == len(pts)
    return cams, imgs, pts


def _rot(q):
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def check_colmap_model(outdir, binary, c2w, K, shapes, names, positions, colors, images=None):
    """the model under outdir against the scene's poses (n, 4, 4), intrinsics (n, 3, 3), image shapes and the cloud"""
    import PIL.Image
    cams, imgs, pts = read_colmap(os.path.join(outdir, 'sparse', '0'), binary)
    n = len(shapes)
    assert [c['id'] for c in cams] == list(range(1, n + 1)) and [i['id'] for i in imgs] == list(range(1, n + 1))
    assert [i['camera_id'] for i in imgs] == list(range(1, n + 1)) and [i['name'] for i in imgs] == list(names)
    assert all(i['n2d'] == 0 for i in imgs)
    for k, (cam, im) in enumerate(zip(cams, imgs)):
        assert cam['model'] == 1 and (cam['height'], cam['width']) == tuple(shapes[k])
        assert cam['params'] == (float(K[k][0, 0]), float(K[k][1, 1]), float(K[k][0, 2]), float(K[k][1, 2]))
        q, t = np.array(im['q']), np.array(im['t'])
        assert abs(np.linalg.norm(q) - 1) < 1e-12 and q[0] >= 0
        assert np.abs(_rot(q) @ c2w[k][:3, :3] - np.eye(3)).max() < 1e-12
        assert np.abs(_rot(q) @ c2w[k][:3, 3] + t).max() < 1e-12
    assert [p['id'] for p in pts] == list(range(1, len(positions) + 1))
    assert all(p['error'] == 0 and p['track'] == 0 for p in pts)
    assert np.array_equal(np.array([p['xyz'] for p in pts]).reshape(-1, 3), np.asarray(positions, np.float64))
    assert np.array_equal(np.array([p['rgb'] for p in pts], dtype=np.uint8).reshape(-1, 3), colors)
    if images is not None:
        for name, (h, w), img in zip(names, shapes, images):
            got = np.asarray(PIL.Image.open(os.path.join(outdir, 'images', name)))
            assert got.shape == (h, w, 3) and np.array_equal(got, np.uint8(255 * np.asarray(img)))
    else:
        assert not os.path.exists(os.path.join(outdir, 'images'))


class _Scene:
    """what write_colmap reads of a scene"""

    def __init__(self, rng, shapes, as_tensors):
        from scipy.spatial.transform import Rotation
        n = len(shapes)
        self.imshapes = shapes
        self.c2w = np.tile(np.eye(4), (n, 1, 1))
        rotvec = rng.normal(size=(n, 3))
        rotvec[0] = [np.pi - 1e-9, 0, 0]                      # a half turn: the quaternion's w is (next to) zero
        rotvec[1] = 0
        self.c2w[:, :3, :3] = Rotation.from_rotvec(rotvec).as_matrix()
        self.c2w[:, :3, 3] = rng.normal(size=(n, 3))
        self.K = np.tile(np.eye(3), (n, 1, 1))
        for k, (h, w) in enumerate(shapes):
            self.K[k, 0, 0], self.K[k, 1, 1], self.K[k, 0, 2], self.K[k, 1, 2] = 100 + k, 90 + k / 3, w / 2 + 0.25, h / 2 - 0.5
        self.imgs = [rng.random((h, w, 3)).astype(np.float32) for h, w in shapes]
        self.wrap = (lambda a: torch.from_numpy(a)) if as_tensors else (lambda a: a)

    def get_im_poses(self):
        return self.wrap(self.c2w)

    def get_intrinsics(self):
        return self.wrap(self.K)


@pytest.mark.parametrize('binary', [True, False])
@pytest.mark.parametrize('n_points', [0, 257])
def test_write_colmap(tmp_path, binary, n_points):
    from dust3r_amd.export import write_colmap
    from dust3r_amd.viz import FusedCloud
    rng = np.random.default_rng(7 + n_points)
    shapes = [(6, 8), (8, 6), (6, 8), (4, 12), (5, 5)]
    scene = _Scene(rng, shapes, as_tensors=binary)
    pos, col, wgt, cnt = _cloud_arrays(rng, n_points)
    cloud = FusedCloud(pos, col, wgt, cnt, 0.1, (np.zeros(3, np.float32), np.ones(3, np.float32)))
    out = str(tmp_path / 'model')
    files = write_colmap(out, scene, cloud, binary=binary)
    ext = 'bin' if binary else 'txt'
    names = [f'{i:06d}.png' for i in range(len(shapes))]
    assert files == [os.path.join(out, 'sparse', '0', f'{s}.{ext}') for s in ('cameras', 'images', 'points3D')] + [os.path.join(out, 'images', nm) for nm in names]
    assert sorted(os.listdir(os.path.join(out, 'sparse', '0'))) == sorted(f'{s}.{ext}' for s in ('cameras', 'images', 'points3D'))
    check_colmap_model(out, binary, scene.c2w, scene.K, shapes, names, pos, col, scene.imgs)
    # given names, no pictures
    out2 = str(tmp_path / 'model2')
    given = [f'frame_{i}.jpg' for i in range(len(shapes))]
    write_colmap(out2, scene, cloud, names=given, binary=binary, write_images=False)
    check_colmap_model(out2, binary, scene.c2w, scene.K, shapes, given, pos, col, None)


def test_write_colmap_errors(tmp_path):
    from dust3r_amd.export import write_colmap
    from dust3r_amd.viz import FusedCloud
    scene = _Scene(np.random.default_rng(0), [(4, 4), (4, 4)], as_tensors=False)
    cloud = FusedCloud(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.uint8), np.zeros(0, np.float32), np.zeros(0, np.int32), 1.0, (None, None))
    with pytest.raises(ValueError, match='2 names|1 names'):
        write_colmap(str(tmp_path), scene, cloud, names=['only_one.png'])
    scene.imgs = None
    with pytest.raises(ValueError, match='scene.imgs is None'):
        write_colmap(str(tmp_path), scene, cloud)
    assert len(write_colmap(str(tmp_path), scene, cloud, write_images=False)) == 3


# ---- the build ----------------------------------------------------------------------------------------------------------------------------
def test_fuse_entry_points_are_exported():
    from dust3r_amd import _lib
    assert {'d3r_fuse_bounds', 'd3r_fuse_bounds_workspace_bytes', 'd3r_fuse_voxels', 'd3r_fuse_voxels_workspace_bytes'} <= set(_lib.EXPORTED)
    assert _lib.lib.d3r_fuse_bounds_workspace_bytes(0, 16) == 0 and _lib.lib.d3r_fuse_voxels_workspace_bytes(3, 0, 5) == 0
    assert _lib.lib.d3r_fuse_voxels_workspace_bytes(3, 100, 0) == 0 and _lib.lib.d3r_fuse_voxels_workspace_bytes(2, 2 ** 30, 5) == 0
    assert _lib.lib.d3r_fuse_bounds_workspace_bytes(3, 5000) > 0
    # two key and two index buffers of `capacity` rows and the tile tables
    assert 24 * 10 ** 6 <= _lib.lib.d3r_fuse_voxels_workspace_bytes(3, 5000, 10 ** 6) < 25 * 10 ** 6


def test_fuse_resource_report_has_no_scratch():
    """read only: the report is what the build left next to the object; nothing is built or touched here"""
    from dust3r_amd import _lib
    path = os.path.join(os.path.dirname(_lib.LIB_PATH), 'fuse.resources.txt')
    if not os.path.exists(path):
        pytest.skip('no fuse.resources.txt: the library was not built by dust3r_amd/build.py')
    report = open(path).read()
    kernels = re.findall(r'Function Name: (\S+)', report)
    assert len(kernels) == 10 and all('fuse_' in k for k in kernels)
    assert re.findall(r'ScratchSize \[bytes/lane\]: (\d+)', report) == ['0'] * len(kernels)
