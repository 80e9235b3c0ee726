"""The headless renderer on the GPU (csrc/render.hip through dust3r_amd.viz): the vertex stage against the fp64 restatement of
tests/test_render_cpu.py within the bound its arithmetic gives, the integer raster stage against the numpy restatement bit for bit, a scene's
view re-projected onto its own pixels, and scene.show() / scene.render_views() / demo.render_turntable end to end."""
import os

import numpy as np
import pytest
import torch

from test_render_cpu import EMPTY, GUARD, INVALID, ZQ_MAX, restated_project, restated_raster, zq_of

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -24


def vertex_bounds(positions, w2c, intr, near):
    """What the fp32 vertex stage may differ by from its fp64 restatement `r`, from the arithmetic alone (eps = 2^-24):
      X, Y, Z   three chained fmas: |dX| <= bX = 4 eps (|R_row| . |p| + |t|)   (gamma_3 of the standard dot-product bound, rounded up to 4 eps)
      u = X / Z one correctly rounded division of perturbed operands: |du| <= (bX + |u| bZ) / (Z - bZ) + eps |u|
      x = fma(fx, u, cx): |dx| <= fx |du| + eps |x|; the product by 16 is exact
      q = rint((near / Z) ZQ_MAX): near / Z carries Z's error and one rounding, the product one more:
          |dq| <= ZQ_MAX (near / Z) (bZ / (Z - bZ) + 2 eps) + 1/2 before the two rint()s
    Returns dict(bZ, dx, dy, dq) per vertex (inf where Z - bZ <= 0)."""
    p = np.abs(np.asarray(positions, dtype=np.float64).reshape(-1, 3))
    M = np.abs(np.asarray(w2c, dtype=np.float64)[:12].reshape(3, 4))
    r = restated_project(positions, w2c, intr, near)
    b = 4 * EPS * (np.where(np.isfinite(p), p, 0) @ M[:, :3].T + M[:, 3])
    with np.errstate(divide='ignore', invalid='ignore'):
        Zm = np.where(r['Z'] - b[:, 2] > 0, r['Z'] - b[:, 2], np.nan)
        out = {}
        for k, (name, f) in enumerate((('dx', intr[0]), ('dy', intr[1]))):
            u = (r['x' if k == 0 else 'y'] - intr[2 + k]) / f
            du = (b[:, k] + np.abs(u) * b[:, 2]) / Zm + EPS * np.abs(u)
            out[name] = np.nan_to_num(f * du + EPS * np.abs(r['x' if k == 0 else 'y']), nan=np.inf)
        out['dq'] = np.nan_to_num(ZQ_MAX * (near / r['Z']) * (b[:, 2] / Zm + 2 * EPS) + 0.5, nan=np.inf)
    out['bZ'] = b[:, 2]
    return out, r


def _look_at(eye, target):
    from dust3r_amd.viz import look_at
    return look_at(np.asarray(eye, dtype=np.float64), np.asarray(target, dtype=np.float64))


def _cams(rng, n, target, dist):
    poses = []
    for _ in range(n):
        d = rng.normal(size=3)
        poses.append(_look_at(np.asarray(target) + dist * d / np.linalg.norm(d), np.asarray(target) + rng.normal(size=3) * 0.2))
    return np.stack(poses)


def test_vertex_stage_against_fp64(gpu):
    """d3r_render_project vs the fp64 restatement, with the bounds of `vertex_bounds` (derived there): snapped coordinates within ONE 1/16-px
    unit; Z recovered from zq, near ZQ_MAX / q, within Z dq / (q - dq) of the fp64 Z (q = (near / Z) ZQ_MAX, dq as derived, + 1/2 for the
    restatement's own rint); validity flags EQUAL for every vertex further than the bounds from the near plane and from the guard band --
    at most 1 % of the vertices may lie inside those bands (asserted: a property of the seeded inputs)."""
    from dust3r_amd.viz import intrinsics_rows, render_project, world_to_cam
    rng = np.random.default_rng(11)
    N, near = 40000, 0.5
    pts = rng.uniform(-4, 4, size=(N, 3)).astype(np.float32)
    pts[:5] = [[np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf], [np.nan] * 3, [1e30, 1e30, 1e30]]
    w2c = world_to_cam(_cams(rng, 3, (0, 0, 0), 3.0))
    intr = intrinsics_rows([300.0, 5000.0, 40000.0], 3, (640, 480))
    sxy, zq = render_project(pts, w2c, intr, near, gpu)
    sxy, zq = sxy.cpu().numpy().astype(np.int64), zq.cpu().numpy()
    n_band = n_checked = 0
    kinds = np.zeros(3, int)
    for f in range(3):
        b, r = vertex_bounds(pts, w2c[f], intr[f].astype(np.float64), near)
        got_valid = zq[f] != INVALID
        assert not got_valid[:5].any()
        with np.errstate(invalid='ignore'):
            behind = r['finite'] & (r['Z'] < near - b['bZ'])
            front = r['finite'] & (r['Z'] > near + b['bZ'])
            clear_in = front & (np.abs(r['x']) < GUARD - b['dx']) & (np.abs(r['y']) < GUARD - b['dy'])
            clear_out = front & ((np.abs(r['x']) > GUARD + b['dx']) | (np.abs(r['y']) > GUARD + b['dy']))
        decided = ~r['finite'] | behind | clear_in | clear_out
        n_band += int((~decided).sum())
        assert np.array_equal(got_valid[decided], r['valid'][decided])
        kinds += np.array([clear_in.sum(), clear_out.sum(), behind.sum()])
        both = got_valid & r['valid']
        n_checked += int(both.sum())
        assert (sxy[f][~got_valid] == 0).all()
        assert np.abs(sxy[f][both, 0] - r['sx'][both]).max() <= 1 and np.abs(sxy[f][both, 1] - r['sy'][both]).max() <= 1
        q = near / r['Z'][both] * ZQ_MAX
        dq = b['dq'][both] + 0.5
        assert (q > 4 * dq).all()
        Z_back = near * ZQ_MAX / (ZQ_MAX - zq[f][both]).astype(np.float64)
        err, bound = np.abs(Z_back - r['Z'][both]), r['Z'][both] * dq / (q - dq)
        print(f'camera {f}: {both.sum()} valid, max |dsx| {np.abs(sxy[f][both, 0] - r["sx"][both]).max()}, max Z error / bound {np.max(err / bound):.3f}')
        assert (err <= bound).all()
    print(f'{n_band} of {3 * N} vertices inside the near / guard bands, {n_checked} compared')
    assert n_band <= 0.01 * 3 * N
    assert (kinds > 1000).all(), kinds          # inside, outside the guard band, behind the near plane: every kind is present


# ---- raster stage, exact ----------------------------------------------------------------------------------------------------------------
def _depth_from(keys, near):
    q = (ZQ_MAX - zq_of(keys)).astype(np.float32)
    with np.errstate(divide='ignore'):
        d = (np.float32(near) * np.float32(ZQ_MAX)) / q
    return np.where(keys == EMPTY, np.float32(np.inf), d).astype(np.float32)


def _check_exact(gpu, poses, intr, size, near, points=None, pcol=None, pmask=None, verts=None, faces=None, vcol=None, point_size=1,
                 background=(255, 255, 255)):
    """render_batch's keys, ids, rgb and depth == the numpy raster stage fed with the GPU's OWN snapped vertices (d3r_render_project)"""
    from dust3r_amd.viz import render_batch, render_project, world_to_cam
    W, H = size
    kw = dict(points=points, point_colors=pcol, point_mask=pmask, vertices=verts, faces=faces, vertex_colors=vcol, point_size=point_size,
              background=background, near=near, return_depth=True, return_ids=True, return_keys=True)
    got = render_batch(poses, intr, size, gpu, **kw)
    w2c = world_to_cam(poses)
    n_pts = 0 if points is None else len(points)
    if points is not None:
        psxy, pzq = [t.cpu().numpy() for t in render_project(points, w2c, intr, near, gpu)]
    if faces is not None:
        vsxy, vzq = [t.cpu().numpy() for t in render_project(verts, w2c, intr, near, gpu)]
    drawn = 0
    for f in range(len(poses)):
        P = None if points is None else dict(sx=psxy[f, :, 0], sy=psxy[f, :, 1], zq=pzq[f], mask=pmask, rgba=np.asarray(pcol), point_size=point_size)
        T = None if faces is None else dict(sx=vsxy[f, :, 0], sy=vsxy[f, :, 1], zq=vzq[f], faces=np.asarray(faces).astype(np.int64), rgba=np.asarray(vcol),
                                            id_base=n_pts)
        keys, ids, rgb = restated_raster(W, H, points=P, tris=T, background=background)
        assert np.array_equal(got['keys'][f].view(np.uint64), keys), f'camera {f}: keys'
        assert np.array_equal(got['ids'][f], ids), f'camera {f}: ids'
        assert np.array_equal(got['rgb'][f], rgb), f'camera {f}: rgb'
        assert np.array_equal(got['depth'][f], _depth_from(keys, near)), f'camera {f}: depth'
        drawn += int((ids >= 0).sum())
    return got, drawn


def _colors(rng, n):
    from dust3r_amd.viz import pack_rgba
    return pack_rgba(rng.integers(0, 256, size=(n, 3)).astype(np.uint8)).numpy()


@pytest.mark.parametrize('point_size', [1, 2, 3])
def test_points_equal_the_restatement(gpu, point_size):
    from dust3r_amd.viz import intrinsics_rows
    rng = np.random.default_rng(point_size)
    N, size = 6000, (80, 60)
    pts = (rng.normal(size=(N, 3)) * 1.5).astype(np.float32)
    pts[:3] = [[np.nan, 0, 0], [np.inf, 0, 0], [0, 0, 0]]
    pts[10:400] = pts[400:790]                                     # equal points: equal depth, the lower id wins
    mask = rng.random(N) < 0.8
    poses = _cams(rng, 2, (0, 0, 0), 5.0)
    for m in (mask, None):
        _, drawn = _check_exact(gpu, poses, intrinsics_rows([70.0, 40.0], 2, size), size, 0.3, points=pts, pcol=_colors(rng, N), pmask=m,
                                point_size=point_size, background=(1, 2, 3))
        assert drawn > 1500


def _mesh_views(rng):
    spec = [(7, 5, 'random'), (16, 12, 'random'), (12, 16, 'true'), (1, 9, 'true'), (33, 40, 'random'), (40, 50, 'sparse'), (2, 2, 'true')]
    imgs, pts, masks = [], [], []
    for k, (H, W, kind) in enumerate(spec):
        imgs.append(rng.integers(0, 256, size=(H, W, 3)).astype(np.uint8))
        v, u = np.mgrid[:H, :W]
        surf = np.stack([(u - W / 2) / 20 + k - 3, (v - H / 2) / 20, 0.3 * np.sin(u / 3.0 + k) + 0.2 * k], axis=-1)
        pts.append((surf + rng.normal(size=(H, W, 3)) * 0.01).astype(np.float32))
        masks.append({'true': np.ones((H, W), bool), 'random': rng.random((H, W)) < 0.8, 'sparse': rng.random((H, W)) < 0.6}[kind])
    return imgs, pts, masks


def test_scene_mesh_equals_the_restatement(gpu):
    """the mesh of scene_mesh_batch for small views of mixed sizes, from afar (faces of about a pixel: the one-thread path) and close up
    (faces of hundreds of pixels, partly outside the frame: the wave path)"""
    from dust3r_amd.viz import intrinsics_rows, pack_rgba, scene_mesh_batch
    rng = np.random.default_rng(21)
    geo = scene_mesh_batch(*_mesh_views(rng), gpu)
    vcol = pack_rgba(geo['colors'][:, :3]).numpy()
    size = (96, 72)
    poses = np.stack([_look_at((0, 0.5, -9), (0, 0, 0)), _look_at((6, -3, -7), (0.5, 0, 0)), _look_at((-1.0, 0.2, -0.8), (-0.5, 0, 0.3))])
    _, drawn = _check_exact(gpu, poses, intrinsics_rows([90.0, 70.0, 60.0], 3, size), size, 0.05, verts=geo['positions'], faces=geo['faces'], vcol=vcol)
    assert drawn > 1000          # not vacuous: a good part of the 3 x 96 x 72 pixels shows a face


def test_camera_glyphs_and_points_in_one_frame(gpu):
    """the wire glyphs are long thin slivers (the wave path), alone and together with a cloud (ids of the faces start after the points)"""
    from dust3r_amd.viz import SceneViz, intrinsics_rows
    rng = np.random.default_rng(5)
    viz = SceneViz(gpu)
    cams = _cams(rng, 4, (0, 0, 0), 2.0)
    viz.add_cameras(cams, focals=[50.0, 80.0, 50.0, 65.0], imsizes=[(64, 48), (48, 64), (64, 48), (32, 32)],
                    colors=[(255, 0, 0), (0, 255, 0), (0, 0, 255), (200, 100, 0)], cam_size=0.8)
    g = {k: (None if v is None else v.cpu().numpy()) for k, v in viz.flat_arrays().items()}
    size = (160, 120)
    poses = np.stack([_look_at((0, -1, -6), (0, 0, 0)), _look_at((4, 4, 3), (0, 0, 0))])
    intr = intrinsics_rows(150.0, 2, size)
    _, drawn = _check_exact(gpu, poses, intr, size, 0.05, verts=g['vertices'], faces=g['faces'], vcol=g['vertex_colors'])
    assert drawn > 300
    N = 5000
    pts = (rng.normal(size=(N, 3)) * 0.8).astype(np.float32)
    got, _ = _check_exact(gpu, poses, intr, size, 0.05, points=pts, pcol=_colors(rng, N), pmask=rng.random(N) < 0.9, verts=g['vertices'],
                          faces=g['faces'], vcol=g['vertex_colors'], point_size=2)
    assert (got['ids'] >= N).sum() > 100 and ((got['ids'] >= 0) & (got['ids'] < N)).sum() > 1000


def test_faces_much_larger_than_the_frame(gpu):
    from dust3r_amd.viz import intrinsics_rows
    rng = np.random.default_rng(8)
    verts = np.float32([[-50, -40, 1], [60, -45, 1.5], [5, 70, 1.2],            # spans thousands of pixels around the frame
                        [-0.2, -0.1, 2], [30, 0.1, 2.5], [-0.1, 20, 3],            # one corner inside
                        [0, 0, 0.5], [1, 0, -1], [0, 1, 2],                        # a vertex behind the near plane: dropped whole
                        [-500, -500, 1], [500, -500, 1], [0, 500, 1],              # beyond the guard band: dropped whole
                        [0.05, 0.02, 0.9], [0.3, 0.02, 0.9], [0.05, 0.3, 0.9]])    # small, in front of everything
    faces = np.array([[0, 1, 2], [2, 1, 0], [3, 4, 5], [6, 7, 8], [9, 10, 11], [12, 14, 13], [0, 0, 1]])
    size = (64, 48)
    got, drawn = _check_exact(gpu, np.eye(4)[None], intrinsics_rows(100.0, 1, size), size, 0.1, verts=verts, faces=faces, vcol=_colors(rng, len(verts)))
    assert drawn == 64 * 48 and set(np.unique(got['ids'])) <= {0, 2, 5}


def test_batched_cameras_equal_single_calls_and_runs_are_identical(gpu):
    from dust3r_amd.viz import SceneViz, intrinsics_rows, render_batch
    rng = np.random.default_rng(13)
    N, size = 20000, (128, 96)
    pts = torch.from_numpy((rng.normal(size=(N, 3)) * 1.2).astype(np.float32)).to(gpu)
    viz = SceneViz(gpu).add_pointcloud(pts, rng.integers(0, 256, size=(N, 3)).astype(np.uint8))
    viz.add_cameras(_cams(rng, 3, (0, 0, 0), 1.5), focals=[50.0] * 3, imsizes=[(64, 48)] * 3, colors=[(255, 0, 0)] * 3, cam_size=0.5)
    g = viz.flat_arrays()
    poses, intr = _cams(rng, 5, (0, 0, 0), 5.0), intrinsics_rows([90.0, 100, 110, 120, 130], 5, size)
    kw = dict(point_size=2, near=0.1, return_depth=True, return_ids=True, return_keys=True, **g)
    a = render_batch(poses, intr, size, gpu, **kw)
    b = render_batch(poses, intr, size, gpu, **kw)
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k
    for f in range(5):
        one = render_batch(poses[f:f + 1], intr[f:f + 1], size, gpu, **kw)
        for k in a:
            assert a[k][f].tobytes() == one[k][0].tobytes(), (k, f)
    assert (a['ids'] >= 0).mean() > 0.2
    dev = render_batch(poses, intr, size, gpu, to_host=False, **kw)
    assert dev['rgb'].is_cuda and np.array_equal(dev['rgb'].cpu().numpy(), a['rgb'])


# ---- scenes -----------------------------------------------------------------------------------------------------------------------------
def _picture(H, W, seed):
    from dust3r_amd.synthetic import synthetic_photo
    return synthetic_photo(W, H, seed=seed).astype(np.float32) / 255


def _synthetic(gpu, n, H, W, mode=None, perturb=True, seed=3, outdoor=False):
    from dust3r_amd.cloud_opt import GlobalAlignerMode, global_aligner
    from dust3r_amd.synthetic import synthetic_scene
    out, init, gt = synthetic_scene(n, H, W, seed=seed, symmetrize=True, perturb=perturb)
    scene = global_aligner(out, gpu, mode=mode or GlobalAlignerMode.PointCloudOptimizer, verbose=False)
    if type(scene).__name__ != 'PairViewer':
        scene.load_state_dict(init)
    if outdoor:                                    # sky above a skyline: mask_sky leaves the lower part
        from dust3r_amd.synthetic import outdoor_scene
        scene.imgs = [outdoor_scene(H, W, seed=k).astype(np.float32) / 255 for k in range(n)]
    else:
        scene.imgs = [_picture(H, W, 40 + k) for k in range(n)]
    return scene


def test_a_view_projects_onto_its_own_pixels(gpu):
    """view i alone, from its own pose, intrinsics and size, point_size 1: pixel p shows point p in the picture's 8-bit colour -- for ALL
    pixels (the fp32 projection error is far below half a pixel at these sizes)"""
    from dust3r_amd.viz import SceneViz
    scene = _synthetic(gpu, 4, 32, 48)
    with torch.no_grad():
        pts, poses, K = scene.get_pts3d(), scene.get_im_poses(), scene.get_intrinsics()
    for i, (H, W) in enumerate(scene.imshapes):
        assert torch.isfinite(pts[i]).all()
        out = SceneViz(gpu).add_pointcloud(pts[i], scene.imgs[i]).render(poses[i], K[i], size=(W, H), point_size=1, near=0.05, return_ids=True)
        assert np.array_equal(out['ids'], np.arange(H * W, dtype=np.int32).reshape(H, W))
        assert np.array_equal(out['rgb'], np.round(scene.imgs[i] * 255).astype(np.uint8))


def _decode(path):
    import PIL.Image
    return np.asarray(PIL.Image.open(path).convert('RGB'))


def _not_constant(img):
    return len(np.unique(img.reshape(-1, 3), axis=0)) > 1


@pytest.mark.parametrize('kind', ['PointCloudOptimizer', 'ModularPointCloudOptimizer', 'PairViewer'])
def test_show_render_views_and_turntable_end_to_end(gpu, tmp_path, kind):
    from dust3r_amd.cloud_opt import GlobalAlignerMode
    from dust3r_amd.demo import render_turntable
    from dust3r_amd.viz import SceneViz
    n = 2 if kind == 'PairViewer' else 3
    scene = _synthetic(gpu, n, 32, 48, mode=getattr(GlobalAlignerMode, kind), outdoor=True)
    assert type(scene).__name__ == kind
    scene.min_conf_thr = 0.5
    out = os.path.join(str(tmp_path), 'show.png')
    viz = scene.show(outfile=out, size=(160, 120), show_pw_cams=True, show_pw_pts3d=(kind != 'PairViewer'))
    assert isinstance(viz, SceneViz) and viz.image.shape == (120, 160, 3) and viz.image.dtype == np.uint8
    assert np.array_equal(_decode(out), viz.image) and _not_constant(viz.image)
    assert scene.show(size=(64, 48), cam_size=0.1).image.shape == (48, 64, 3)                    # no file
    for as_mesh in (False, True):
        views = scene.render_views(as_mesh=as_mesh)
        assert len(views) == n and all(v.shape == (32, 48, 3) and v.dtype == np.uint8 and _not_constant(v) for v in views)
    img, depth = scene.render_views(return_depth=True)[0]
    assert depth.shape == (32, 48) and depth.dtype == np.float32 and np.isfinite(depth).any() and (depth[np.isfinite(depth)] > 0).all()
    for as_pc in (True, False):
        names = render_turntable(os.path.join(str(tmp_path), f'tt{int(as_pc)}'), scene, n_frames=5, size=(96, 72), as_pointcloud=as_pc, min_conf_thr=1.5,
                                 clean_depth=as_pc, mask_sky=not as_pc)
        assert len(names) == 5 and [os.path.basename(p) for p in names] == [f'turntable_{k:03d}.png' for k in range(5)]
        frames = [_decode(p) for p in names]
        assert all(f.shape == (72, 96, 3) and _not_constant(f) for f in frames)
        assert len({f.tobytes() for f in frames}) == 5
    scene.imgs = None
    viz = scene.show(size=(64, 48))                                                                  # a random colour per view
    assert _not_constant(viz.image)
    with pytest.raises(ValueError, match='scene.imgs is None'):
        scene.render_views()


def test_render_views_of_the_ground_truth_scene_show_the_pictures(gpu):
    """The fused ground-truth scene seen from camera i agrees with picture i on every pixel whose own point is the nearest along its ray.
    "Nearest" is decided by the fp64 restatement with the slack of the fp32 vertex stage (`vertex_bounds`; snapped coordinates within one unit,
    test_vertex_stage_against_fp64): a point of ANOTHER view competes for every pixel it can reach with its coordinates moved by 1.5 / 16 px,
    at its depth lowered by dq; the own point must beat all of them at its depth raised by dq. Pixels that are nearer only within that slack
    are left out; the rest must show the picture. For this seed the fp64 restatement finds 2228 of the 6144 pixels (36 %) decided that way;
    the test asks for at least 2100, so that the check cannot quietly shrink."""
    from dust3r_amd.viz import world_to_cam
    n, H, W = 4, 32, 48
    scene = _synthetic(gpu, n, H, W, perturb=False, seed=6)
    scene.min_conf_thr = 0.0
    with torch.no_grad():
        pts = np.concatenate([p.reshape(-1, 3).cpu().numpy() for p in scene.get_pts3d()])
        poses, K = scene.get_im_poses().cpu().numpy(), scene.get_intrinsics().cpu().numpy()
    views = scene.render_views(point_size=1)
    near = 0.01 * float(np.linalg.norm(pts.max(axis=0) - pts.min(axis=0)))                      # SceneViz.render's default
    total = 0
    for i in range(n):
        intr = np.float32([K[i, 0, 0], K[i, 1, 1], K[i, 0, 2], K[i, 1, 2]]).astype(np.float64)
        b, r = vertex_bounds(pts, world_to_cam(poses[i])[0], intr, near)
        own = np.arange(i * H * W, (i + 1) * H * W)
        assert r['valid'][own].all()
        rival = np.full((H, W), np.inf)
        other = r['valid'].copy()
        other[own] = False
        x, y, zmin = r['x'][other], r['y'][other], (r['zq'] - b['dq'] - 0.5)[other]
        s = 1.5 / 16 + np.maximum(b['dx'], b['dy'])[other]
        for px in (np.floor(x + 0.5 - s), np.floor(x + 0.5 + s)):
            for py in (np.floor(y + 0.5 - s), np.floor(y + 0.5 + s)):
                inside = (px >= 0) & (px < W) & (py >= 0) & (py < H)
                np.minimum.at(rival, (py[inside].astype(int), px[inside].astype(int)), zmin[inside])
        wins = ((r['zq'] + b['dq'] + 0.5)[own].reshape(H, W) < rival)
        total += int(wins.sum())
        want = np.round(scene.imgs[i] * 255).astype(np.uint8)
        assert np.array_equal(views[i][wins], want[wins]), f'view {i}'
    print(f'{total} of {n * H * W} pixels show their own point')
    assert total >= 2100


def test_mesh_mode_frames_by_the_masked_geometry(gpu, tmp_path):
    """Pixels behind the mask that lie far away (sky, low confidence) are still vertices of the export's mesh. They must not reach the
    framing or the near plane: the device-resident mesh of scene_mesh_batch(to_host=False) equals the host one, SceneViz.bounds() equals the
    kernel's bounds of the vertices a face uses, and render_views(as_mesh=True) / render_turntable(as_pointcloud=False) of a scene with such
    outliers give the pictures of the scene with the outliers moved somewhere else."""
    from dust3r_amd.demo import render_turntable
    from dust3r_amd.viz import SceneViz, scene_mesh_batch
    rng = np.random.default_rng(31)
    imgs, pts, masks = _mesh_views(rng)
    for p, m in zip(pts, masks):
        p[~m] = p[~m] * 1000 + 5000                                      # every masked-out pixel is an outlier
    host = scene_mesh_batch(imgs, pts, masks, gpu)
    dev = scene_mesh_batch(imgs, pts, masks, gpu, to_host=False)
    assert dev['positions'].is_cuda and dev['faces'].dtype == torch.int32 and dev['colors'].dtype == torch.int32
    assert np.array_equal(dev['positions'].cpu().numpy(), host['positions'])
    assert np.array_equal(dev['faces'].cpu().numpy().view(np.uint32), host['faces'])
    assert np.array_equal(dev['colors'].cpu().numpy().view(np.uint8).reshape(-1, 4), host['colors'])
    for geo in (host, dev):
        lo, hi = SceneViz(gpu).add_mesh(geo['positions'], geo['faces'], geo['colors']).bounds()
        assert np.array_equal(lo, host['bounds'][0].astype(np.float64)) and np.array_equal(hi, host['bounds'][1].astype(np.float64))
        assert hi.max() < 100
    # a scene whose low-confidence pixels lie far away, twice: the outliers in two different places
    pictures = []
    for shift in (300.0, -7000.0):
        scene = _synthetic(gpu, 3, 32, 48, outdoor=True)
        with torch.no_grad():
            low = scene.im_depthmaps.new_zeros(scene.im_depthmaps.shape, dtype=torch.bool)
            low[:, ::7] = True
            for i, c in enumerate(scene.im_conf):
                c.view(-1)[low[i, :c.numel()]] = 0.5
            scene.im_depthmaps.data[low] = float(np.log(abs(shift)))      # log-depth: these pixels sit hundreds of scene sizes away
        scene.min_conf_thr = 1.0
        views = scene.render_views(as_mesh=True)
        names = render_turntable(os.path.join(str(tmp_path), f'tt{int(shift)}'), scene, n_frames=3, size=(96, 72), as_pointcloud=False,
                                 min_conf_thr=float(np.exp(1.0) - 1))
        pictures.append(views + [_decode(p) for p in names])
        assert all(_not_constant(v) for v in pictures[-1])
    for a, b in zip(*pictures):
        assert np.array_equal(a, b)
