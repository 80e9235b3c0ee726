"""scene.fuse() on the GPU: the kernels of csrc/fuse.hip (viz.fuse_points) against the numpy restatement of tests/test_fuse_cpu.py. Every
comparison is exact (np.array_equal on positions, colours, weight, count and the voxel count): the keys are fp32 and IEEE, the sort is stable
and the fp64 sums run in one fixed order, so there is nothing to tolerate. Then scene.fuse() on aligned scenes and the command line."""
import argparse
import copy
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from test_fuse_cpu import check_cloud, restated_fuse

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(40, 52), (37, 29), (33, 31)]            # 2080 = two tiles + 32, 1073 = one tile + 49, 1023 = one tile - 1


def _views(rng, shapes, extent, u8=True, mask_rate=0.7, weights=True):
    imgs, pts, masks, wgts = [], [], [], []
    for H, W in shapes:
        imgs.append(rng.integers(0, 256, size=(H, W, 3)).astype(np.uint8) if u8 else rng.random((H, W, 3)).astype(np.float32))
        pts.append((rng.random((H, W, 3)) * extent).astype(np.float32))
        masks.append(rng.random((H, W)) < mask_rate)
        wgts.append((rng.random((H, W)) * 4 + 0.01).astype(np.float32))
    return imgs, pts, masks, (wgts if weights else None)


def _poisoned_stacks(pts, masks, wgts, row, device):
    """the padded stacks with NaN behind every view in pts / weight and 0xFF in the mask, built on the device"""
    n = len(pts)
    P = torch.full((n, row, 3), float('nan'), device=device)
    M = torch.full((n, row), 0xFF, dtype=torch.uint8, device=device)
    Wt = None if wgts is None else torch.full((n, row), float('nan'), device=device)
    for i, p in enumerate(pts):
        a = p.shape[0] * p.shape[1]
        P[i, :a] = torch.from_numpy(p.reshape(a, 3)).to(device)
        M[i, :a] = torch.from_numpy(masks[i].reshape(a).astype(np.uint8)).to(device)
        if wgts is not None:
            Wt[i, :a] = torch.from_numpy(wgts[i].reshape(a)).to(device)
    return P, M, Wt


@pytest.mark.parametrize('u8', [True, False])
def test_tiles_padding_and_stability(gpu, u8):
    """Views of two tiles + 32, one tile + 49 and one tile - 1 pixels in one poisoned stack; about 500 voxels, each with points of several
    tiles and several views, so a scatter that is not stable (or a sum in another order) changes the low bits of the fp64 sums."""
    from dust3r_amd.viz import fuse_points
    rng = np.random.default_rng(10 + u8)
    imgs, pts, masks, wgts = _views(rng, SHAPES, 4.0, u8=u8)
    pts[1][3, 4] = np.nan                                              # invalid pixels inside the views too
    wgts[0][5, 6], wgts[2][7, 8], wgts[2][9, 1] = 0.0, np.inf, -1.0
    want = restated_fuse(imgs, pts, masks, wgts, 0.5)
    assert 400 < len(want['positions']) <= 512 and want['count'].max() > 8
    check_cloud(fuse_points(imgs, pts, masks, wgts, 0.5, gpu), want)                                   # numpy maps, padded by the call
    P, M, Wt = _poisoned_stacks(pts, masks, wgts, 2080 + 12, gpu)
    check_cloud(fuse_points(imgs, P, M, Wt, 0.5, gpu), want)                                           # ready stacks, poisoned padding
    check_cloud(fuse_points([torch.from_numpy(im).to(gpu) for im in imgs], P, [torch.from_numpy(m).to(gpu) for m in masks], Wt, 0.5, gpu), want)


def test_wide_keys(gpu):
    """12 bits per axis: 36 key bits, nine passes, the last over the high word alone. Points come in clusters so that voxels are shared."""
    from dust3r_amd.viz import fuse_points
    rng = np.random.default_rng(3)
    imgs, pts, masks, wgts = _views(rng, SHAPES, 0.5)
    centres = (rng.random((300, 3)) * 1000).astype(np.float32)
    for p in pts:
        p += centres[rng.integers(0, 300, size=p.shape[:2])]
    want = restated_fuse(imgs, pts, masks, wgts, 0.25)
    assert sum(want['bits']) > 32 and len(want['positions']) < 0.8 * want['n_valid']
    check_cloud(fuse_points(imgs, pts, masks, wgts, 0.25, gpu), want)


def test_an_axis_of_exactly_21_bits(gpu):
    from dust3r_amd.viz import fuse_points
    rng = np.random.default_rng(4)
    imgs, pts, masks, wgts = _views(rng, SHAPES, 3.0)
    for p in pts:
        p[..., 1] += (rng.integers(0, 2 ** 21 - 4, size=p.shape[:2]) // 1000 * 1000).astype(np.float32)       # exact in fp32
    masks[0][0, :2] = True
    pts[0][0, 0], pts[0][0, 1] = (0, 0, 0), (1, 2 ** 21 - 1, 1)
    wgts[0][0, :2] = 1.0
    want = restated_fuse(imgs, pts, masks, wgts, 1.0)
    assert want['bits'][1] == 21 and sum(want['bits']) == 25
    check_cloud(fuse_points(imgs, pts, masks, wgts, 1.0, gpu), want)
    pts[0][0, 1] = (1, 2 ** 21, 1)                                     # one voxel more: 22 bits
    with pytest.raises(ValueError, match="voxel_size too small for the scene's extent"):
        fuse_points(imgs, pts, masks, wgts, 1.0, gpu)


def test_degenerate_inputs(gpu):
    from dust3r_amd.viz import fuse_points
    rng = np.random.default_rng(5)
    imgs, pts, masks, wgts = _views(rng, SHAPES, 1.0)
    one = restated_fuse(imgs, pts, masks, wgts, 100.0)                 # everything in one voxel: one thread sums 2900 points in order
    assert len(one['positions']) == 1 and one['count'][0] == one['n_valid'] > 2500
    check_cloud(fuse_points(imgs, pts, masks, wgts, 100.0, gpu), one)
    single = [np.zeros(m.shape, bool) for m in masks]                  # exactly one valid point
    single[1][20, 7] = True
    want = restated_fuse(imgs, pts, single, wgts, 0.01)
    assert want['n_valid'] == 1 and np.array_equal(want['positions'][0], pts[1][20, 7])
    check_cloud(fuse_points(imgs, pts, single, wgts, 0.01, gpu), want)
    nothing = [np.zeros(m.shape, bool) for m in masks]                 # nothing valid: an empty cloud, bounds (+inf, -inf)
    cloud = fuse_points(imgs, pts, nothing, wgts, 0.01, gpu)
    check_cloud(cloud, restated_fuse(imgs, pts, nothing, wgts, 0.01))
    assert len(cloud) == 0 and cloud.bounds[0].tolist() == [np.inf] * 3 and cloud.bounds[1].tolist() == [-np.inf] * 3
    cloud = fuse_points(imgs, pts, masks, [np.zeros_like(w) for w in wgts], 0.01, gpu, to_host=False)       # no positive weight: the same
    assert len(cloud) == 0 and cloud.positions.is_cuda and cloud.positions.shape == (0, 3) and cloud.colors.shape == (0, 3)
    want = restated_fuse(imgs, pts, masks, None, 0.1)                  # weights=None: ones
    assert np.array_equal(want['weight'], want['count'].astype(np.float32))
    check_cloud(fuse_points(imgs, pts, masks, None, 0.1, gpu), want)
    want2 = restated_fuse(imgs, pts, masks, wgts, 0.1, min_count=2)    # thin voxels dropped, order kept
    assert 0 < len(want2['positions']) < len(want['positions']) and want2['count'].min() == 2
    check_cloud(fuse_points(imgs, pts, masks, wgts, 0.1, gpu, min_count=2), want2)


def test_indices_past_2_24(gpu):
    """Rows of 2^23 + 4 elements: the flat indices of views 1 and 2 pass 2^23 and 2^24 while a few thousand pixels are real; the padding is NaN
    (0xFF in the mask). An index that went through fp32 would land on a neighbour."""
    from dust3r_amd.viz import fuse_points
    rng = np.random.default_rng(6)
    imgs, pts, masks, wgts = _views(rng, SHAPES[::-1], 2.0)
    want = restated_fuse(imgs, pts, masks, wgts, 0.25)
    P, M, Wt = _poisoned_stacks(pts, masks, wgts, 2 ** 23 + 4, gpu)
    assert 2 * P.shape[1] + 1000 > 2 ** 24
    check_cloud(fuse_points(imgs, P, M, Wt, 0.25, gpu), want)


def test_determinism_on_four_large_views(gpu):
    """4 x 512 x 384: 192 tiles per view, 135 sort tiles; two calls give the same bytes, and they are the restatement's."""
    from dust3r_amd.viz import fuse_points
    rng = np.random.default_rng(7)
    imgs, pts, masks, wgts = _views(rng, [(384, 512)] * 4, 1.0)
    for p in pts:
        p *= np.float32([6, 4, 2])
    dev = [[torch.from_numpy(a).to(gpu) for a in seq] for seq in (imgs, pts, masks, wgts)]
    a = fuse_points(*dev, 0.05, gpu)
    b = fuse_points(*dev, 0.05, gpu)
    for k in ('positions', 'colors', 'weight', 'count'):
        assert getattr(a, k).tobytes() == getattr(b, k).tobytes(), k
    want = restated_fuse(imgs, pts, masks, wgts, 0.05)
    assert len(want['positions']) > 200000 and want['count'].max() > 5
    check_cloud(a, want)


def test_error_returns(gpu):
    """the C entry points refuse what they cannot run, before any launch"""
    import ctypes as C
    from dust3r_amd._lib import current_stream, lib, ptr
    n, row, cap = 2, 64, 128
    pts = torch.zeros((n, row, 3), device=gpu)
    mask = torch.ones((n, row), dtype=torch.uint8, device=gpu)
    rgb = torch.zeros((n, row, 3), dtype=torch.uint8, device=gpu)
    hw = torch.full((n,), 8, dtype=torch.int32, device=gpu)
    small = torch.zeros(4, dtype=torch.int64, device=gpu)
    work = torch.empty(int(lib.d3r_fuse_voxels_workspace_bytes(n, row, cap)) + int(lib.d3r_fuse_bounds_workspace_bytes(n, row)), dtype=torch.uint8, device=gpu)
    out = [torch.empty((cap, 3), device=gpu), torch.empty(cap, dtype=torch.int32, device=gpu), torch.empty(cap, device=gpu),
           torch.empty(cap, dtype=torch.int32, device=gpu), torch.empty(2, dtype=torch.int64, device=gpu)]

    def bounds(**kw):
        a = dict(dict(n=n, pts=ptr(pts), mask=ptr(mask), h=ptr(hw), w=ptr(hw), row=row, b=ptr(small), c=ptr(small[3:]), work=ptr(work)), **kw)
        return lib.d3r_fuse_bounds(a['n'], a['pts'], a['mask'], None, a['h'], a['w'], a['row'], a['b'], a['c'], a['work'], current_stream())

    def voxels(lo=(0.0, 0.0, 0.0), voxel=1.0, bits=(1, 1, 1), **kw):
        a = dict(dict(n=n, pts=ptr(pts), mask=ptr(mask), rgb=ptr(rgb), row=row, cap=cap, pos=ptr(out[0]), work=ptr(work)), **kw)
        return lib.d3r_fuse_voxels(a['n'], a['pts'], a['mask'], None, a['rgb'], 1, ptr(hw), ptr(hw), a['row'], (C.c_float * 3)(*lo), voxel, (C.c_int * 3)(*bits),
                                   a['cap'], a['pos'], ptr(out[1]), ptr(out[2]), ptr(out[3]), ptr(out[4]), a['work'], current_stream())
    assert bounds() == 0 and voxels() == 0
    for kw in (dict(n=0), dict(n=65536), dict(row=0), dict(pts=None), dict(mask=None), dict(b=None), dict(c=None), dict(work=None)):
        assert bounds(**kw) == -1, kw
    for kw in (dict(n=0), dict(row=-1), dict(cap=0), dict(pts=None), dict(rgb=None), dict(pos=None), dict(work=None), dict(voxel=0.0), dict(voxel=float('nan')),
               dict(voxel=float('inf')), dict(bits=(0, 1, 1)), dict(bits=(1, 22, 1)), dict(lo=(0.0, float('nan'), 0.0)), dict(lo=(float('-inf'), 0.0, 0.0))):
        assert voxels(**kw) == -1, kw
    torch.cuda.synchronize()
    assert out[4].tolist() == [128, 1]                                 # the good call: 2 x 64 zeros in one voxel


# ---- scenes ---------------------------------------------------------------------------------------------------------------------------
def _write_images(tmp_path, sizes):
    import PIL.Image
    from dust3r_amd.synthetic import synthetic_photo
    paths = []
    for k, (W, H) in enumerate(sizes):
        p = os.path.join(str(tmp_path), f'view{k}.png')
        PIL.Image.fromarray(synthetic_photo(W, H, seed=20 + k)).save(p)
        paths.append(p)
    return paths


def _scene(gpu, n, H, W, seed):
    """An aligned scene with images, through the call sequence of the demo's body (global_aligner, PairViewer for two images, else init='mst'
    and a few iterations, as tests/test_glb_gpu.py builds its scenes) -- but on the consistent pairwise pointmaps of synthetic_scene: the
    random-weight network of that file gives NaN depth maps, and a cloud of no valid point says nothing about the fusion."""
    from dust3r_amd.cloud_opt import GlobalAlignerMode, global_aligner
    from dust3r_amd.synthetic import outdoor_scene, synthetic_scene
    out, _, _ = synthetic_scene(n, H, W, seed=seed, scene_graph='complete', symmetrize=True, noise=0.002, device=gpu)
    pics = [torch.from_numpy(outdoor_scene(H, W, seed=i)).permute(2, 0, 1).float() / 127.5 - 1 for i in range(n)]
    for view in ('view1', 'view2'):
        out[view]['img'] = torch.stack([pics[int(i)] for i in out[view]['idx']])
    mode = GlobalAlignerMode.PointCloudOptimizer if n > 2 else GlobalAlignerMode.PairViewer
    scene = global_aligner(out, device=gpu, mode=mode, verbose=False)
    if mode == GlobalAlignerMode.PointCloudOptimizer:
        scene.compute_global_alignment(init='mst', niter=20, schedule='linear', lr=0.01)
    return scene


@pytest.fixture(scope='module')
def scenes(gpu):
    return dict(multi=_scene(gpu, 3, 40, 52, 1), pair=_scene(gpu, 2, 36, 48, 2))      # the default min_conf_thr masks a part of every view


def _restated_scene_fuse(scene, voxel_size, weights=True, min_count=1):
    with torch.no_grad():
        pts = [p.detach().cpu().numpy() for p in scene.get_pts3d()]
        msk = [m.cpu().numpy() for m in scene.get_masks()]
        conf = [c.detach().cpu().numpy() for c in scene.im_conf]
    return restated_fuse(scene.imgs, pts, msk, conf if weights else None, voxel_size, min_count=min_count), sum(int(m.sum()) for m in msk)


def _restated_default_voxel(scene):
    """the median pixel footprint, in numpy: lower medians, fp32 division"""
    with torch.no_grad():
        depths = [d.detach().cpu().numpy() for d in scene.get_depthmaps()]
        focals = scene.get_focals().detach().cpu().numpy().reshape(len(depths), -1)
    per_view = np.sort(np.float32([np.sort(d.reshape(-1))[(d.size - 1) // 2] / f.mean(dtype=np.float32) for d, f in zip(depths, focals)]))
    return float(per_view[(len(per_view) - 1) // 2])


@pytest.mark.parametrize('which', ['multi', 'pair'])
def test_scene_fuse(gpu, scenes, which):
    from dust3r_amd.viz import FusedCloud
    scene = copy.deepcopy(scenes[which])
    cloud = scene.fuse()
    assert isinstance(cloud, FusedCloud) and isinstance(cloud.positions, np.ndarray)
    assert cloud.voxel_size == _restated_default_voxel(scene)
    want, n_masked = _restated_scene_fuse(scene, cloud.voxel_size)
    check_cloud(cloud, want)
    assert 0 < len(cloud) < n_masked
    coarse = scene.fuse(voxel_size=4 * cloud.voxel_size, min_count=2, weights=None, to_host=False)
    assert all(isinstance(t, torch.Tensor) and t.is_cuda for t in (coarse.positions, coarse.colors, coarse.weight, coarse.count))
    check_cloud(coarse, _restated_scene_fuse(scene, 4 * cloud.voxel_size, weights=False, min_count=2)[0])
    assert len(coarse) < len(cloud)
    with pytest.raises(ValueError, match="weights is 'conf' or None"):
        scene.fuse(weights='depth')
    scene.min_conf_thr = float('inf')                                  # nothing passes the mask: an empty cloud, and no voxel size is asked for
    empty = scene.fuse()
    assert len(empty) == 0 and empty.bounds[0].tolist() == [np.inf] * 3 and np.isnan(empty.voxel_size)


@pytest.mark.parametrize('which', ['multi', 'pair'])
def test_scene_fuse_after_clean_pointcloud_and_mask_sky(gpu, scenes, which):
    scene = copy.deepcopy(scenes[which]).clean_pointcloud().mask_sky()
    cloud = scene.fuse()
    want, n_masked = _restated_scene_fuse(scene, cloud.voxel_size)
    check_cloud(cloud, want)
    assert len(cloud) < n_masked


def test_scene_fuse_without_images_raises(gpu, scenes):
    s = copy.deepcopy(scenes['pair'])
    s.imgs = None
    with pytest.raises(ValueError, match='scene.imgs is None'):
        s.fuse()


# ---- the command line -----------------------------------------------------------------------------------------------------------------
def test_command_line_writes_ply_and_colmap(gpu, tmp_path):
    """python -m dust3r_amd.demo on three tiny pictures in a fresh child process: with --fuse --ply --colmap it writes scene.ply and colmap/,
    which read_ply and the COLMAP reader accept and which agree with each other and with cameras.json; without them it writes neither.
    The checkpoint has random weights: its three-view scenes come out with NaN focals and depth maps (measured: no finite point at any
    picture size or iteration count), so the cloud in these files is the empty one; clouds with points are the tests above."""
    import json
    from dust3r_amd.export import read_ply
    from dust3r_amd.synthetic import MODEL_CONFIGS
    from oracle.dust3r_ref import build_ref_model
    cfg = MODEL_CONFIGS['tiny_dpt']
    state = {k: v for k, v in build_ref_model('tiny_dpt').state_dict().items() if not k.startswith('dec_blocks2')}
    model_str = ("AsymmetricCroCo3DStereo(pos_embed='RoPE100', patch_embed_cls='ManyAR_PatchEmbed', img_size=(64, 64), head_type='dpt', output_mode='pts3d', "
                 "depth_mode=('exp', -inf, inf), conf_mode=('exp', 1, inf), enc_embed_dim=%d, enc_depth=%d, enc_num_heads=%d, dec_embed_dim=%d, dec_depth=%d, dec_num_heads=%d)"
                 % (cfg['enc_embed_dim'], cfg['enc_depth'], cfg['enc_num_heads'], cfg['dec_embed_dim'], cfg['dec_depth'], cfg['dec_num_heads']))
    ckpt = str(tmp_path / 'tiny_dpt.pth')
    torch.save({'args': argparse.Namespace(model=model_str), 'model': state}, ckpt)
    pics = tmp_path / 'pics'
    pics.mkdir()
    _write_images(pics, [(80, 60), (60, 80), (80, 60)])
    base = [sys.executable, '-m', 'dust3r_amd.demo', str(pics), '--weights', ckpt, '--image_size', '224', '--niter', '5', '--min_conf_thr', '1.0', '--silent']
    out = tmp_path / 'fused'
    r = subprocess.run(base + ['--outdir', str(out), '--fuse', '--ply', '--colmap'], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert os.path.isfile(out / 'scene.glb')
    cloud = read_ply(str(out / 'scene.ply'))
    assert sorted(cloud) == ['colors', 'confidence', 'count', 'positions'] and len(cloud['positions']) == len(cloud['count'])
    cams = json.loads((out / 'cameras.json').read_text())
    shapes = [(h, w) for w, h in cams['image_sizes']]
    assert len(shapes) == 3
    import PIL.Image
    from test_fuse_cpu import read_colmap
    cameras, images, points = read_colmap(str(out / 'colmap' / 'sparse' / '0'), True)
    assert [c['id'] for c in cameras] == [1, 2, 3] and [i['name'] for i in images] == [f'{i:06d}.png' for i in range(3)]
    for cam, im, (h, w), f in zip(cameras, images, shapes, cams['focals']):
        assert cam['model'] == 1 and (cam['height'], cam['width']) == (h, w) and np.array_equal(cam['params'][:2], (f[0], f[-1]), equal_nan=True)
        assert im['camera_id'] == im['id'] and im['n2d'] == 0             # (the poses of this scene are NaN: tests/test_fuse_cpu.py holds the pose algebra)
        assert PIL.Image.open(out / 'colmap' / 'images' / im['name']).size == (w, h)
    assert [p['id'] for p in points] == list(range(1, len(cloud['positions']) + 1))           # the same cloud in both files
    assert np.array_equal(np.array([p['xyz'] for p in points], dtype=np.float64).reshape(-1, 3), cloud['positions'].astype(np.float64))
    assert np.array_equal(np.array([p['rgb'] for p in points], dtype=np.uint8).reshape(-1, 3), cloud['colors'])
    plain = tmp_path / 'plain'
    r = subprocess.run(base + ['--outdir', str(plain)], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert os.path.isfile(plain / 'scene.glb') and not os.path.exists(plain / 'scene.ply') and not os.path.exists(plain / 'colmap')
