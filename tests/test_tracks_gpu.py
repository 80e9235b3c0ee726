"""2-D tracks on the GPU: the kernels of csrc/tracks.hip (viz.cloud_tracks) against the numpy restatement of tests/test_tracks_cpu.py. Every
comparison is exact (np.array_equal on every integer output and on err2): the projection is fp64 + * / and floor with every operation
rounded on its own, the distances are fp32 and IEEE, the sort is stable, so there is nothing to tolerate. Then scene.fuse(tracks=True) on
aligned scenes, the COLMAP model they give, and the command line."""
import argparse
import copy
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from test_fuse_gpu import _poisoned_stacks, _scene, _write_images
from test_tracks_cpu import (EDGE_MAX_DIST, EDGE_MAX_ERROR, EDGE_POINTS, FIELDS, SHAPES, SURFACE_MAX_DIST, check_tracks, colmap_invariant, edge_case_inputs,
                             restated_tracks, surface_case_conditions, surface_views)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def surface():
    from dust3r_amd.viz import track_cameras
    pts, masks, wgts, K, c2w = surface_views(SHAPES, seed=1)
    return dict(pts=pts, masks=masks, wgts=wgts, K=K, c2w=c2w, cams=track_cameras(K, c2w))


def _single_view_cloud(gpu, pts, v):
    """the pixels of view v as a cloud from fuse_points: a voxel far below the pixel spacing, every pixel valid, so one point per pixel"""
    from dust3r_amd.viz import fuse_points
    H, W = pts[v].shape[:2]
    cloud = fuse_points([np.zeros((H, W, 3), np.uint8)], [pts[v]], [np.ones((H, W), bool)], None, 1e-4, gpu)
    assert len(cloud) == H * W
    return cloud.positions


@pytest.fixture(scope='module')
def clouds(gpu, surface):
    return {1073: _single_view_cloud(gpu, surface['pts'], 1), 2080: _single_view_cloud(gpu, surface['pts'], 0)}


@pytest.fixture(scope='module')
def surface_want(surface, clouds):
    """the restatement of the two surface cases, computed once"""
    s = surface
    return {m: restated_tracks(P, s['pts'], s['masks'], s['wgts'], s['cams'], SURFACE_MAX_DIST) for m, P in clouds.items()}


@pytest.mark.parametrize('m', [1073, 2080])
def test_consistent_views(gpu, surface, clouds, surface_want, m):
    """Three views of a noisy surface (two tiles + 32, one tile + 49, one tile - 1 pixels) in one poisoned stack, a cloud of one tile + 49
    or two tiles + 32 points: tracks of length about 2.6, pixels claimed by several points, points no view sees, off-centre choices."""
    from dust3r_amd.viz import cloud_tracks
    s, P, want = surface, clouds[m], surface_want[m]
    assert len(P) == m
    surface_case_conditions(want, P, s['cams'], SHAPES)
    check_tracks(cloud_tracks(P, s['pts'], s['masks'], s['wgts'], s['K'], s['c2w'], SHAPES, SURFACE_MAX_DIST, device=gpu), want)      # numpy maps
    stacks = _poisoned_stacks(s['pts'], s['masks'], s['wgts'], 2080 + 12, gpu)
    got = cloud_tracks(torch.from_numpy(P).to(gpu), *stacks, torch.from_numpy(s['K']).to(gpu), torch.from_numpy(s['c2w']).to(gpu), SHAPES, SURFACE_MAX_DIST,
                       device=gpu, to_host=False)
    assert all(getattr(got, k).is_cuda for k in FIELDS)
    check_tracks(got, want)
    assert np.array_equal(got.point_error().cpu().numpy() >= 0, np.diff(want['point_offsets']) > 0)
    # no weights: more pixels are valid
    check_tracks(cloud_tracks(P, stacks[0], stacks[1], None, s['K'], s['c2w'], SHAPES, SURFACE_MAX_DIST, device=gpu),
                 restated_tracks(P, s['pts'], s['masks'], None, s['cams'], SURFACE_MAX_DIST))


def test_hand_made_cases(gpu):
    """every case of tests/test_tracks_cpu.py in one launch: the answers written down by hand there"""
    from dust3r_amd.viz import cloud_tracks, track_cameras
    P, pts, masks, wgts, cams, shapes = edge_case_inputs()
    K = np.tile(np.eye(3), (2, 1, 1))
    c2w = np.tile(np.eye(4), (2, 1, 1))
    c2w[1, 0, 3] = -1.0
    assert np.array_equal(track_cameras(K, c2w), cams)
    got = cloud_tracks(P, pts, masks, wgts, K, c2w, shapes, EDGE_MAX_DIST, max_error=EDGE_MAX_ERROR, device=gpu)
    assert list(zip(got.view.tolist(), got.pixel.tolist())) == [o for _, obs in EDGE_POINTS for o in obs]
    assert got.lengths.tolist() == [len(obs) for _, obs in EDGE_POINTS]
    check_tracks(got, restated_tracks(P, pts, masks, wgts, cams, EDGE_MAX_DIST, EDGE_MAX_ERROR))
    stacks = _poisoned_stacks(pts, masks, wgts, 61, gpu)
    free = cloud_tracks(P, *stacks, K, c2w, shapes, EDGE_MAX_DIST, device=gpu)
    assert len(free) == len(got) + 1
    check_tracks(free, restated_tracks(P, pts, masks, wgts, cams, EDGE_MAX_DIST))
    check_tracks(cloud_tracks(P, stacks[0], stacks[1], None, K, c2w, shapes, EDGE_MAX_DIST, max_error=EDGE_MAX_ERROR, device=gpu),
                 restated_tracks(P, pts, masks, None, cams, EDGE_MAX_DIST, EDGE_MAX_ERROR))
    check_tracks(cloud_tracks(P, *stacks, K, c2w, shapes, 0.0, device=gpu), restated_tracks(P, pts, masks, wgts, cams, 0.0))      # r2 = 0: exact hits only
    with pytest.raises(ValueError, match='max_dist'):
        cloud_tracks(P, *stacks, K, c2w, shapes, -1.0, device=gpu)
    with pytest.raises(ValueError, match='max_dist'):
        cloud_tracks(P, *stacks, K, c2w, shapes, 1e30, device=gpu)
    with pytest.raises(ValueError, match='max_error'):
        cloud_tracks(P, *stacks, K, c2w, shapes, 1.0, max_error=float('nan'), device=gpu)


def test_twenty_views(gpu):
    """more than 16 views: the sort by view takes two passes, and ends in the other buffer; 16 and 17 views on either side of that"""
    from dust3r_amd.viz import cloud_tracks, track_cameras
    shapes = [(12, 9)] * 20
    pts, masks, wgts, K, c2w = surface_views(shapes, seed=2, noise=0.02)
    P = np.concatenate([pts[0].reshape(-1, 3), pts[13].reshape(-1, 3)])
    want = restated_tracks(P, pts, masks, wgts, track_cameras(K, c2w), 0.3)
    per_image = np.diff(want['image_offsets'])
    assert per_image.min() > 0 and np.diff(want['point_offsets']).max() > 16
    check_tracks(cloud_tracks(P, pts, masks, wgts, K, c2w, shapes, 0.3, device=gpu), want)
    check_tracks(cloud_tracks(P, pts[:17], masks[:17], wgts[:17], K[:17], c2w[:17], shapes[:17], 0.3, device=gpu),
                 restated_tracks(P, pts[:17], masks[:17], wgts[:17], track_cameras(K[:17], c2w[:17]), 0.3))
    check_tracks(cloud_tracks(P, pts[:16], masks[:16], wgts[:16], K[:16], c2w[:16], shapes[:16], 0.3, device=gpu),
                 restated_tracks(P, pts[:16], masks[:16], wgts[:16], track_cameras(K[:16], c2w[:16]), 0.3))


def test_degenerate_inputs(gpu, surface, clouds):
    from dust3r_amd.viz import cloud_tracks
    s, P = surface, clouds[1073]
    one = restated_tracks(P, s['pts'][:1], s['masks'][:1], s['wgts'][:1], s['cams'][:1], SURFACE_MAX_DIST)                 # n = 1: no sort pass
    assert len(one['view']) > 500 and one['image_offsets'].tolist() == [0, len(one['view'])]
    check_tracks(cloud_tracks(P, s['pts'][:1], s['masks'][:1], s['wgts'][:1], s['K'][:1], s['c2w'][:1], SHAPES[:1], SURFACE_MAX_DIST, device=gpu), one)
    j = int(np.argmax(np.diff(restated_tracks(P, s['pts'], s['masks'], s['wgts'], s['cams'], SURFACE_MAX_DIST)['point_offsets'])))
    single = restated_tracks(P[j:j + 1], s['pts'], s['masks'], s['wgts'], s['cams'], SURFACE_MAX_DIST)                     # M = 1
    assert single['point_offsets'].tolist() == [0, 3]
    check_tracks(cloud_tracks(P[j:j + 1], s['pts'], s['masks'], s['wgts'], s['K'], s['c2w'], SHAPES, SURFACE_MAX_DIST, device=gpu), single)
    far = P + np.float32([0, 0, -100])                                                                                    # behind every camera
    unseen = restated_tracks(far, s['pts'], s['masks'], s['wgts'], s['cams'], SURFACE_MAX_DIST)
    assert len(unseen['view']) == 0 and unseen['point_offsets'].tolist() == [0] * 1074 and unseen['image_offsets'].tolist() == [0] * 4
    got = cloud_tracks(far, s['pts'], s['masks'], s['wgts'], s['K'], s['c2w'], SHAPES, SURFACE_MAX_DIST, device=gpu)
    check_tracks(got, unseen)
    assert got.stats()['observations'] == 0 and (got.point_error() == -1).all()
    empty = cloud_tracks(np.zeros((0, 3), np.float32), s['pts'], s['masks'], s['wgts'], s['K'], s['c2w'], SHAPES, SURFACE_MAX_DIST, device=gpu)
    check_tracks(empty, restated_tracks(np.zeros((0, 3), np.float32), s['pts'], s['masks'], s['wgts'], s['cams'], SURFACE_MAX_DIST))


def test_max_error(gpu, surface, clouds, surface_want):
    from dust3r_amd.viz import cloud_tracks
    s, P, full = surface, clouds[2080], surface_want[2080]
    max_error = float(np.median(np.sqrt(full['err2'])))
    want = restated_tracks(P, s['pts'], s['masks'], s['wgts'], s['cams'], SURFACE_MAX_DIST, max_error)
    assert 0.1 < 1 - len(want['view']) / len(full['view']) < 0.9
    assert np.sqrt(want['err2']).max() <= max_error
    check_tracks(cloud_tracks(P, s['pts'], s['masks'], s['wgts'], s['K'], s['c2w'], SHAPES, SURFACE_MAX_DIST, max_error=max_error, device=gpu), want)


def test_zero_and_infinite_weights_inside_a_window(gpu, surface, clouds, surface_want):
    from dust3r_amd.viz import cloud_tracks
    s, P, before = surface, clouds[2080], surface_want[2080]
    wgts = [w.copy() for w in s['wgts']]
    k = int(np.flatnonzero((before['view'] == 1) & (before['pixel'] % 29 > 0) & (before['pixel'] % 29 < 28))[40])      # an observation in view 1
    y, x = divmod(int(before['pixel'][k]), 29)
    wgts[1][y, x], wgts[1][y, x + 1], wgts[1][y, x - 1] = np.inf, 0.0, np.nan
    want = restated_tracks(P, s['pts'], s['masks'], wgts, s['cams'], SURFACE_MAX_DIST)
    changed = (len(want['view']) != len(before['view'])) or not np.array_equal(want['pixel'], before['pixel'])
    assert changed and not ((want['view'] == 1) & np.isin(want['pixel'], [y * 29 + x - 1, y * 29 + x, y * 29 + x + 1])).any()
    check_tracks(cloud_tracks(P, s['pts'], s['masks'], wgts, s['K'], s['c2w'], SHAPES, SURFACE_MAX_DIST, device=gpu), want)


def test_indices_past_2_24(gpu):
    """Rows of 2^23 + 4 elements: the flat indices of views 1 and 2 pass 2^23 and 2^24 while a few thousand pixels are real; the padding is NaN
    (0xFF in the mask). An index that went through fp32 would gather a neighbour."""
    from dust3r_amd.viz import cloud_tracks, track_cameras
    shapes = SHAPES[::-1]
    pts, masks, wgts, K, c2w = surface_views(shapes, seed=3)
    P = pts[2].reshape(-1, 3)
    want = restated_tracks(P, pts, masks, wgts, track_cameras(K, c2w), SURFACE_MAX_DIST)
    assert np.bincount(want['view'], minlength=3).min() > 500
    stacks = _poisoned_stacks(pts, masks, wgts, 2 ** 23 + 4, gpu)
    assert 2 * stacks[0].shape[1] + 1000 > 2 ** 24
    check_tracks(cloud_tracks(P, *stacks, K, c2w, shapes, SURFACE_MAX_DIST, device=gpu), want)


def test_determinism(gpu, surface, clouds, surface_want):
    from dust3r_amd.viz import cloud_tracks
    s, P = surface, torch.from_numpy(clouds[2080]).to(gpu)
    stacks = _poisoned_stacks(s['pts'], s['masks'], s['wgts'], 2080, gpu)
    a = cloud_tracks(P, *stacks, s['K'], s['c2w'], SHAPES, SURFACE_MAX_DIST, device=gpu, to_host=False)
    b = cloud_tracks(P, *stacks, s['K'], s['c2w'], SHAPES, SURFACE_MAX_DIST, device=gpu, to_host=False)
    for k in FIELDS:
        assert getattr(a, k).cpu().numpy().tobytes() == getattr(b, k).cpu().numpy().tobytes(), k
    check_tracks(a, surface_want[2080])


def test_error_returns(gpu):
    """the C entry points refuse what they cannot run, before any launch"""
    from dust3r_amd._lib import current_stream, lib, ptr
    n, row, m, cap = 2, 64, 10, 64
    pts = torch.zeros((n, row, 3), device=gpu)
    pts[..., 2] = 1.0
    mask = torch.ones((n, row), dtype=torch.uint8, device=gpu)
    hw = torch.full((n,), 8, dtype=torch.int32, device=gpu)
    P = torch.zeros((m, 3), device=gpu)
    P[:, 2] = 1.0
    cams = torch.zeros((n, 16), dtype=torch.float64, device=gpu)
    cams[:, [0, 4, 8, 12, 13]] = 1.0
    off = torch.zeros(m + 1, dtype=torch.int32, device=gpu)
    seen = torch.zeros((m, 1), dtype=torch.int32, device=gpu)
    total = torch.zeros(1, dtype=torch.int64, device=gpu)
    ints = [torch.zeros(cap, dtype=torch.int32, device=gpu) for _ in range(4)]
    err2 = torch.zeros(cap, dtype=torch.float64, device=gpu)
    image_off = torch.zeros(n + 1, dtype=torch.int32, device=gpu)
    work = torch.empty(int(lib.d3r_cloud_tracks_workspace_bytes(cap)), dtype=torch.uint8, device=gpu)

    def common(a):
        return (a['n'], a['pts'], a['mask'], None, a['h'], ptr(hw), a['row'], a['m'], a['P'], a['cams'], a['r2'], a['has_thr'], a['thr2'])
    base = dict(n=n, pts=ptr(pts), mask=ptr(mask), h=ptr(hw), row=row, m=m, P=ptr(P), cams=ptr(cams), r2=0.25, has_thr=0, thr2=0.0)

    def count(**kw):
        a = dict(dict(base, off=ptr(off), seen=ptr(seen), total=ptr(total)), **kw)
        return lib.d3r_cloud_tracks_count(*common(a), a['off'], a['seen'], a['total'], current_stream())

    def fill(**kw):
        a = dict(dict(base, off=ptr(off), seen=ptr(seen), T=20, cap=cap, view=ptr(ints[0]), err2=ptr(err2), image_off=ptr(image_off), work=ptr(work)), **kw)
        return lib.d3r_cloud_tracks_fill(*common(a), a['off'], a['seen'], a['T'], a['cap'], a['view'], ptr(ints[1]), a['err2'], ptr(ints[2]), a['image_off'], ptr(ints[3]),
                                         a['work'], current_stream())
    assert count() == 0
    torch.cuda.synchronize()
    assert int(total) == 20 and off.tolist() == list(range(0, 21, 2))            # every point lands on pixel (0, 0) of both views
    assert seen.tolist() == [[3]] * m
    assert fill() == 0
    torch.cuda.synchronize()
    assert ints[0][:20].tolist() == [0, 1] * 10 and image_off.tolist() == [0, 10, 20] and ints[3][:20].tolist() == list(range(0, 20, 2)) + list(range(1, 20, 2))
    bad = (dict(n=0), dict(n=65536), dict(row=0), dict(row=2 ** 30), dict(m=0), dict(m=-3), dict(pts=None), dict(mask=None), dict(h=None), dict(P=None),
           dict(cams=None), dict(r2=-1.0), dict(r2=float('nan')), dict(r2=float('inf')), dict(has_thr=1, thr2=-1.0), dict(has_thr=1, thr2=float('nan')),
           dict(off=None), dict(seen=None))
    for kw in bad + (dict(total=None),):
        assert count(**kw) == -1, kw
    for kw in bad + (dict(T=-1), dict(T=cap + 1), dict(T=2 ** 31, cap=2 ** 31 - 1), dict(cap=0), dict(view=None), dict(err2=None), dict(image_off=None),
                     dict(work=None)):
        assert fill(**kw) == -1, kw
    torch.cuda.synchronize()


def test_more_than_32_views(gpu):
    """70 views: three words of the (point, view) bits between the two passes, the last one partly used; view 31 / 32 / 63 / 64 observe"""
    from dust3r_amd.viz import cloud_tracks, track_cameras
    shapes = [(12, 9), (9, 12)] * 35
    pts, masks, wgts, K, c2w = surface_views(shapes, seed=4, noise=0.02)
    P = np.concatenate([pts[31].reshape(-1, 3), pts[64].reshape(-1, 3), pts[69].reshape(-1, 3) + np.float32([0, 0, -50])])
    want = restated_tracks(P, pts, masks, wgts, track_cameras(K, c2w), 0.3)
    per_image = np.diff(want['image_offsets'])
    assert per_image[[0, 31, 32, 63, 64, 69]].min() > 0 and np.diff(want['point_offsets']).max() > 40 and (np.diff(want['point_offsets']) == 0).sum() >= 108
    check_tracks(cloud_tracks(P, pts, masks, wgts, K, c2w, shapes, 0.3, device=gpu), want)
    check_tracks(cloud_tracks(P, pts[:64], masks[:64], wgts[:64], K[:64], c2w[:64], shapes[:64], 0.3, device=gpu),
                 restated_tracks(P, pts[:64], masks[:64], wgts[:64], track_cameras(K[:64], c2w[:64]), 0.3))


# ---- scenes ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def scenes(gpu):
    return dict(multi=_scene(gpu, 3, 40, 52, 1), pair=_scene(gpu, 2, 36, 48, 2))


def _restated_scene_tracks(scene, cloud, max_error=None):
    """the restatement on the scene's own stacks, with the poses as the COLMAP model holds them"""
    from dust3r_amd.export import colmap_cameras, quat_to_rotmat
    with torch.no_grad():
        pts = [p.detach().cpu().numpy() for p in scene.get_pts3d()]
        msk = [m.cpu().numpy() for m in scene.get_masks()]
        conf = [c.detach().cpu().numpy() for c in scene.im_conf]
        cams = np.array([[*quat_to_rotmat(c['q']).reshape(9), *c['t'], *c['params']] for c in colmap_cameras(scene)])
    positions = cloud.positions.cpu().numpy() if isinstance(cloud.positions, torch.Tensor) else cloud.positions
    return restated_tracks(positions, pts, msk, conf, cams, cloud.voxel_size, max_error)


@pytest.mark.parametrize('which', ['multi', 'pair'])
def test_scene_fuse_with_tracks(gpu, scenes, which, tmp_path):
    from dust3r_amd.export import read_colmap, write_colmap
    from dust3r_amd.viz import CloudTracks
    scene = copy.deepcopy(scenes[which])
    plain = scene.fuse()
    assert plain.tracks is None
    cloud = scene.fuse(tracks=True)
    assert isinstance(cloud.tracks, CloudTracks) and isinstance(cloud.tracks.view, np.ndarray) and np.array_equal(cloud.positions, plain.positions)
    want = _restated_scene_tracks(scene, cloud)
    err = np.sqrt(want['err2'])
    assert len(err) > len(cloud) and err.mean() < 1.0                          # a consistent scene: the cloud lands where it came from
    check_tracks(cloud.tracks, want)
    stats = cloud.tracks.stats()
    assert stats['observations'] == len(err) and stats['mean_error'] == float(err.mean()) and len(stats['observations_per_image']) == scene.n_imgs
    for binary in (True, False):
        out = str(tmp_path / ('bin' if binary else 'txt'))
        write_colmap(out, scene, cloud, binary=binary)
        cams, images, points = read_colmap(os.path.join(out, 'sparse', '0'))
        assert colmap_invariant(images, points) == len(err) and [len(im['xys']) for im in images] == stats['observations_per_image']
        assert np.array_equal([p['error'] for p in points], cloud.tracks.point_error())
    # max_reproj_error, the device arm, and what the other methods of the cloud do with tracks
    thr = float(np.median(err))
    dev = scene.fuse(tracks=True, max_reproj_error=thr, to_host=False, normals=True)
    assert dev.tracks.view.is_cuda and dev.normals is not None
    cut = _restated_scene_tracks(scene, dev, thr)
    assert 0.1 < 1 - len(cut['view']) / len(err) < 0.9
    check_tracks(dev.tracks, cut)
    assert cloud.estimate_normals().tracks is cloud.tracks and cloud.remove_outliers()[0].tracks is None
    assert cloud.transform(np.diag([2.0, 2.0, 2.0, 1.0])).tracks is None
    wide = cloud.build_tracks(scene, max_dist=3 * cloud.voxel_size, weights=None)
    assert len(wide.tracks) >= len(cloud.tracks) and wide.tracks is not cloud.tracks
    scene.min_conf_thr = float('inf')                                          # nothing passes the mask: an empty cloud with empty tracks
    empty = scene.fuse(tracks=True)
    assert len(empty) == 0 and len(empty.tracks) == 0 and empty.tracks.point_offsets.tolist() == [0]


# ---- the command line -----------------------------------------------------------------------------------------------------------------
def test_command_line_writes_tracks(gpu, tmp_path):
    """python -m dust3r_amd.demo --colmap --colmap_tracks in a fresh child process writes a model read_colmap accepts, whose tracks and
    POINTS2D name each other, and the tracks' statistics into cameras.json. The checkpoint has random weights (tests/test_fuse_gpu.py: its
    scenes have no finite point), so the model here is the empty one; models with points are the tests above."""
    from dust3r_amd.export import read_colmap
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
    out = tmp_path / 'out'
    cmd = [sys.executable, '-m', 'dust3r_amd.demo', str(pics), '--weights', ckpt, '--image_size', '224', '--niter', '5', '--min_conf_thr', '1.0', '--silent',
           '--outdir', str(out), '--colmap', '--colmap_tracks', '--max_reproj_error', '2.0']
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    cams, images, points = read_colmap(str(out / 'colmap' / 'sparse' / '0'))
    assert len(cams) == len(images) == 3
    n_obs = colmap_invariant(images, points)
    stats = json.loads((out / 'cameras.json').read_text())['tracks']
    assert stats['observations'] == n_obs and stats['observations_per_image'] == [len(im['xys']) for im in images]
    assert set(stats) == {'observations', 'mean_track_length', 'unobserved', 'mean_error', 'median_error', 'observations_per_image'}
    r = subprocess.run(cmd[:-4] + ['--colmap_tracks'], capture_output=True, text=True, timeout=600, cwd=ROOT)      # the flag needs --colmap: refused before any work
    assert r.returncode == 2 and '--colmap_tracks needs --colmap' in r.stderr
