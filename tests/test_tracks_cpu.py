"""2-D tracks of a cloud (viz.cloud_tracks, csrc/tracks.hip): `restated_tracks` is THE definition in numpy (include/dust3r_hip.h,
d3r_cloud_tracks_count states it in words), pinned here on hand-made cases whose answers are written down by hand; tests/test_tracks_gpu.py
holds the kernels to it bit for bit. Then what needs no GPU: viz.CloudTracks, the COLMAP model with tracks and its reader, the build."""
import os
import re

import numpy as np
import pytest

from test_fuse_cpu import _Scene

SHAPES = [(40, 52), (37, 29), (33, 31)]            # 2080 = two tiles + 32, 1073 = one tile + 49, 1023 = one tile - 1


def restated_tracks(positions, pts, masks, weights, cams, max_dist, max_error=None):
    """positions (M, 3) float32; pts / masks / weights: per view (H, W, 3) float32, (H, W) bool, (H, W) float32 (weights may be None); cams
    (n, 16) float64 = R (9, row-major), t (3), fx, fy, cx, cy. numpy rounds every operation on its own, which is the rule. Vectorised over
    the points; loops over the views and the nine offsets. Returns the arrays of viz.CloudTracks."""
    P = np.asarray(positions, dtype=np.float32).reshape(-1, 3)
    cams = np.asarray(cams, dtype=np.float64).reshape(-1, 16)
    M, n = len(P), len(pts)
    r = np.float32(max_dist)
    r2 = r * r
    assert r2.dtype == np.float32
    x, y, z = (P[:, c].astype(np.float64) for c in range(3))
    seen, pix, err = np.zeros((n, M), bool), np.zeros((n, M), np.int64), np.zeros((n, M), np.float64)
    with np.errstate(all='ignore'):
        for v in range(n):
            H, W = pts[v].shape[:2]
            R, t, (fx, fy, cx, cy) = cams[v, :9].reshape(3, 3), cams[v, 9:12], cams[v, 12:]
            X = [((R[k, 0] * x + R[k, 1] * y) + R[k, 2] * z) + t[k] for k in range(3)]
            ok = X[2] > 0
            u, w = fx * (X[0] / X[2]) + cx, fy * (X[1] / X[2]) + cy
            iu, iw = np.floor(u + 0.5), np.floor(w + 0.5)
            ok &= (iu >= 0) & (iu < W) & (iw >= 0) & (iw < H)                                      # in fp64, before any conversion to int
            px, py = np.where(ok, iu, 0).astype(np.int64), np.where(ok, iw, 0).astype(np.int64)
            flat = np.asarray(pts[v], dtype=np.float32).reshape(-1, 3)
            valid = np.asarray(masks[v]).reshape(-1).astype(bool) & np.isfinite(flat).all(axis=1)
            if weights is not None:
                wv = np.asarray(weights[v], dtype=np.float32).reshape(-1)
                valid &= np.isfinite(wv) & (wv > 0)
            best, best_e = np.zeros(M, np.float32), np.full(M, -1, np.int64)
            for b in (-1, 0, 1):                                                                  # ascending e: the first of equal d2 stays
                for a in (-1, 0, 1):
                    xx, yy = px + a, py + b
                    inside = ok & (xx >= 0) & (xx < W) & (yy >= 0) & (yy < H)
                    e = np.where(inside, yy * W + xx, 0)
                    p = flat[e]
                    dx, dy, dz = p[:, 0] - P[:, 0], p[:, 1] - P[:, 1], p[:, 2] - P[:, 2]
                    d2 = (dx * dx + dy * dy) + dz * dz
                    assert d2.dtype == np.float32
                    better = inside & valid[e] & (d2 <= r2) & ((best_e < 0) | (d2 < best))
                    best, best_e = np.where(better, d2, best), np.where(better, e, best_e)
            got = best_e >= 0
            ex, ey = u - (best_e % W), w - (best_e // W)
            e2 = ex * ex + ey * ey
            if max_error is not None:
                got &= ~(e2 > float(max_error) ** 2)
            seen[v], pix[v], err[v] = got, best_e, e2
    point, view = np.nonzero(seen.T)                                                               # point, then view
    pixel, err2 = pix.T[seen.T], err.T[seen.T]
    T = len(view)
    image_obs = np.argsort(view, kind='stable')
    image_offsets = np.concatenate([[0], np.cumsum(np.bincount(view, minlength=n))])
    point2d = np.zeros(T, np.int64)
    point2d[image_obs] = np.arange(T) - image_offsets[view[image_obs]]
    return dict(point_offsets=np.concatenate([[0], np.cumsum(seen.sum(axis=0))]).astype(np.int32), view=view.astype(np.int32), pixel=pixel.astype(np.int32),
                point2d=point2d.astype(np.int32), err2=err2.astype(np.float64), image_offsets=image_offsets.astype(np.int32), image_obs=image_obs.astype(np.int32))


FIELDS = ('point_offsets', 'view', 'pixel', 'point2d', 'err2', 'image_offsets', 'image_obs')


def check_tracks(got, want):
    """a viz.CloudTracks (numpy or device arrays) against the restatement: every array equal, dtype included"""
    for k in FIELDS:
        g = getattr(got, k)
        g = g.cpu().numpy() if hasattr(g, 'cpu') else g
        assert g.dtype == want[k].dtype and g.shape == want[k].shape, (k, g.dtype, g.shape, want[k].shape)
        assert np.array_equal(g, want[k]), (k, int((g != want[k]).sum()))


def tracks_of(want, shapes):
    from dust3r_amd.viz import CloudTracks
    return CloudTracks(*(want[k] for k in FIELDS), shapes=shapes)


# ---- the hand-made cases ------------------------------------------------------------------------------------------------------------------
EDGE_MAX_DIST, EDGE_MAX_ERROR = 0.5, 1.5            # r2 = 0.25, thr2 = 2.25
EPS = 2.0 ** -20
# per point its observations (view, pixel) under EDGE_MAX_ERROR, by hand. View 0: 6 x 8, the identity camera with fx = fy = 1, cx = cy = 0,
# so that a point (x, y, 1) projects to (x, y); view 1: 5 x 9, the same camera moved so that it projects to (x + 1, y).
EDGE_POINTS = [
    ((2, 2, -1), []),                                   # 0 behind both cameras
    ((2.5, 1, 1), [(0, 12)]),                           # 1 u + 0.5 = 3 exactly: iu = 3, so pixel (4, 1) is in the window; e2 = 2.25 = thr2: kept
    ((0, 0, 1), [(0, 9)]),                              # 2 the window clipped at the corner (0, 0): pixel (1, 1)
    ((7, 5, 1), [(0, 38)]),                             # 3 ... and at the corner (7, 5): pixel (6, 4)
    ((0, 1, 1), [(0, 8)]),                              # 4 x = -1 is outside: pixel (7, 0), where y W + x would land, holds the point itself
    ((4, 3, 1), [(0, 29)]),                             # 5 the centre pixel is masked out, the neighbour (5, 3) is taken
    ((2, 4, 1), [(0, 33)]),                             # 6 (1, 4) and (3, 4) at equal d2: the lower index
    ((6, 2, 1), [(0, 22)]),                             # 7 d2 == r2: kept
    ((6, 0, 1), []),                                    # 8 d2 one ulp above r2
    ((2.5, 2 + EPS, 1), []),                            # 9 e2 = 2.25 + 2^-40 > thr2: dropped ((0, 20) without a threshold)
    ((np.nextafter(np.float32(2.5), np.float32(3)), 5, 1), [(0, 44)]),      # 10 e2 just below thr2
    ((2.0 ** 41, 1, 1), []), ((-2.0 ** 41, 1, 1), []), ((3e38, 1, 1e-38), []),      # 11-13 |u| > 2^40
    ((np.nan, 1, 1), []), ((1, 1, np.nan), []),         # 14, 15
    ((5, 0.9, 1), [(0, 13), (1, 15)]), ((5, 1.1, 1), [(0, 13), (1, 15)]),      # 16, 17 claim the same pixel, in both views
    ((3, 3, 1), []),                                    # 18 in front of both cameras, nothing near it
    ((1, 3, 1), [(0, 25), (1, 29)]),                    # 19 seen by both: ascending view
    ((1, 5, 1), [(0, 42)]),                             # 20 the centre has an infinite weight, (0, 5) a zero weight, (2, 5) is taken
]


def edge_case_inputs():
    """(positions, pts, masks, weights, cams, shapes) of the hand-made cases"""
    shapes = [(6, 8), (5, 9)]
    pts = [np.full((h, w, 3), 100.0, np.float32) for h, w in shapes]
    masks = [np.ones((h, w), bool) for h, w in shapes]
    wgts = [np.ones((h, w), np.float32) for h, w in shapes]
    P = np.array([p for p, _ in EDGE_POINTS], dtype=np.float32)

    def put(v, x, y, p):
        pts[v][y, x] = p
    put(0, 4, 1, P[1])
    put(0, 1, 1, P[2])
    put(0, 6, 4, P[3])
    put(0, 7, 0, P[4])
    put(0, 0, 1, (0, 1, 1.25))
    put(0, 4, 3, P[5])
    masks[0][3, 4] = False
    put(0, 5, 3, (4.1, 3, 1))
    put(0, 1, 4, (2, 4, 1.25))
    put(0, 3, 4, (2, 4, 1.25))
    put(0, 6, 2, (6, 2, 1.5))
    put(0, 6, 0, (6, 0, np.nextafter(np.float32(1.5), np.float32(2))))
    put(0, 4, 2, P[9])
    put(0, 4, 5, P[10])
    put(0, 5, 1, (5, 1, 1))
    put(1, 6, 1, (5, 1, 1))
    put(0, 1, 3, P[19])
    put(1, 2, 3, P[19])
    put(0, 1, 5, P[20])
    wgts[0][5, 1] = np.inf
    put(0, 0, 5, P[20])
    wgts[0][5, 0] = 0.0
    put(0, 2, 5, (1, 5, 1.2))
    wgts[0][5, 2] = 2.0
    cams = np.zeros((2, 16))
    cams[:, [0, 4, 8]] = 1.0
    cams[:, 12:14] = 1.0
    cams[1, 9] = 1.0
    return P, pts, masks, wgts, cams, shapes


def test_restatement_on_hand_made_cases():
    P, pts, masks, wgts, cams, shapes = edge_case_inputs()
    got = restated_tracks(P, pts, masks, wgts, cams, EDGE_MAX_DIST, EDGE_MAX_ERROR)
    want = [obs for _, obs in EDGE_POINTS]
    lengths = [len(o) for o in want]
    assert got['point_offsets'].tolist() == np.concatenate([[0], np.cumsum(lengths)]).tolist()
    assert list(zip(got['view'].tolist(), got['pixel'].tolist())) == [o for obs in want for o in obs]
    e2 = {j: got['err2'][got['point_offsets'][j]:got['point_offsets'][j + 1]].tolist() for j in range(len(P))}
    assert e2[1] == [2.25] and e2[2] == [2.0] and e2[3] == [2.0] and e2[4] == [0.0] and e2[5] == [1.0] and e2[6] == [1.0] and e2[7] == [0.0]
    assert 2.2499 < e2[10][0] < 2.25 and e2[19] == [0.0, 0.0] and e2[20] == [1.0]
    assert np.allclose(e2[16], 0.1 ** 2, rtol=1e-6) and e2[16][0] == e2[16][1]
    # image 0 lists its observations in ascending point order, image 1 the three points it sees
    assert got['image_offsets'].tolist() == [0, 12, 15]
    assert got['image_obs'].tolist() == [0, 1, 2, 3, 4, 5, 6, 7, 8, 10, 12, 14, 9, 11, 13]
    assert got['point2d'].tolist() == [0, 1, 2, 3, 4, 5, 6, 7, 8, 0, 9, 1, 10, 2, 11]
    # without the threshold point 9 has its observation, e2 one step above thr2
    free = restated_tracks(P, pts, masks, wgts, cams, EDGE_MAX_DIST)
    k = free['point_offsets'][9]
    assert free['point_offsets'][10] - k == 1 and (free['view'][k], free['pixel'][k]) == (0, 20) and free['err2'][k] == 2.25 + 2.0 ** -40
    assert len(free['view']) == len(got['view']) + 1
    # without weights (0, 5) and the centre (1, 5) of point 20 are ordinary pixels, both at d2 = 0: the lower index, one pixel off
    plain = restated_tracks(P, pts, masks, None, cams, EDGE_MAX_DIST, EDGE_MAX_ERROR)
    assert plain['pixel'][plain['point_offsets'][20]] == 40 and plain['err2'][plain['point_offsets'][20]] == 1.0


# ---- consistent synthetic views --------------------------------------------------------------------------------------------------------------
def _look_at(eye, target):
    fwd = np.asarray(target, float) - np.asarray(eye, float)
    fwd /= np.linalg.norm(fwd)
    right = np.cross([0.0, 1.0, 0.0], fwd)
    right /= np.linalg.norm(right)
    c2w = np.eye(4)
    c2w[:3, 0], c2w[:3, 1], c2w[:3, 2], c2w[:3, 3] = right, np.cross(fwd, right), fwd, eye
    return c2w


def _height(x, y):
    return 0.05 * np.sin(3 * x) * np.cos(2 * y)


def surface_views(shapes, seed, noise=0.004, extent=1.15, mask_rate=0.95):
    """Views of the surface z = 0.05 sin(3 x) cos(2 y) from cameras about 3 units in front of it, each framing |x|, |y| < extent: pointmaps by
    ray casting (fixed-point iteration on the ray parameter) plus Gaussian noise. Returns (pts, masks, weights, K (n, 3, 3), c2w (n, 4, 4))."""
    rng = np.random.default_rng(seed)
    pts, masks, wgts, Ks, poses = [], [], [], [], []
    for i, (H, W) in enumerate(shapes):
        eye = np.array([0.5 * np.cos(2.1 * i + seed), 0.4 * np.sin(1.7 * i + seed), -3.0 - 0.1 * i])
        c2w = _look_at(eye, (0.0, 0.0, 0.0))
        f = 0.5 * min(H, W) * 3.0 / extent
        K = np.array([[f, 0, W / 2 + 0.25], [0, f * 1.02, H / 2 - 0.5], [0, 0, 1]])
        xs, ys = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
        d = np.stack([(xs - K[0, 2]) / K[0, 0], (ys - K[1, 2]) / K[1, 1], np.ones_like(xs)], axis=-1) @ c2w[:3, :3].T
        t = -eye[2] / d[..., 2]
        for _ in range(30):
            hit = eye + t[..., None] * d
            t = (_height(hit[..., 0], hit[..., 1]) - eye[2]) / d[..., 2]
        hit = eye + t[..., None] * d + rng.normal(size=(H, W, 3)) * noise
        pts.append(hit.astype(np.float32))
        masks.append(rng.random((H, W)) < mask_rate)
        wgts.append((rng.random((H, W)) * 4 + 0.01).astype(np.float32))
        Ks.append(K)
        poses.append(c2w)
    return pts, masks, wgts, np.stack(Ks), np.stack(poses)


def off_centre_share(got, positions, cams, shapes):
    """the share of observations whose pixel is not the rounded projection itself"""
    P = np.asarray(positions, np.float64)
    point = np.repeat(np.arange(len(P)), np.diff(got['point_offsets']))
    c = cams[got['view']]
    X = [c[:, 3 * k] * P[point, 0] + c[:, 3 * k + 1] * P[point, 1] + c[:, 3 * k + 2] * P[point, 2] + c[:, 9 + k] for k in range(3)]
    iu, iw = np.floor(c[:, 12] * X[0] / X[2] + c[:, 14] + 0.5), np.floor(c[:, 13] * X[1] / X[2] + c[:, 15] + 0.5)
    widths = np.array([w for _, w in shapes])[got['view']]
    return float(((got['pixel'] % widths != iu) | (got['pixel'] // widths != iw)).mean())


def claimed_twice(got):
    """the number of (view, pixel) pairs that more than one point observes"""
    _, counts = np.unique(np.stack([got['view'], got['pixel']], axis=1), axis=0, return_counts=True)
    return int((counts > 1).sum())


SURFACE_MAX_DIST = 0.06            # about one pixel footprint of the finest view


def surface_case_conditions(got, positions, cams, shapes):
    """what the synthetic case must show so that it cannot pass empty"""
    lengths = np.diff(got['point_offsets'])
    assert lengths.mean() > 1.5, lengths.mean()
    assert claimed_twice(got) >= 1 and (lengths == 0).sum() >= 1
    assert off_centre_share(got, positions, cams, shapes) >= 0.01


def test_restatement_on_consistent_views():
    """the clouds here are the valid pixels of one view themselves (the GPU file takes them from fuse_points at a voxel below the pixel spacing)"""
    from dust3r_amd.viz import track_cameras
    pts, masks, wgts, K, c2w = surface_views(SHAPES, seed=1)
    cams = track_cameras(K, c2w)
    for v in (0, 1):
        P = pts[v].reshape(-1, 3)
        got = restated_tracks(P, pts, masks, wgts, cams, SURFACE_MAX_DIST)
        surface_case_conditions(got, P, cams, SHAPES)
        err = np.sqrt(got['err2'])
        assert np.median(err) < 0.6 and err.max() <= 1.5 * np.sqrt(2) + 1e-9


# ---- CloudTracks, the COLMAP model ----------------------------------------------------------------------------------------------------------
def colmap_invariant(images, points):
    """every track element (image, idx) names a POINTS2D entry whose point3D_id is that point, and every POINTS2D entry is named by one"""
    by_id = {im['id']: im for im in images}
    n_elements = 0
    for p in points:
        assert len({(int(i), int(k)) for i, k in p['track']}) == len(p['track'])
        for image_id, idx in p['track']:
            assert by_id[int(image_id)]['point3D_ids'][int(idx)] == p['id']
        assert (p['error'] == -1) == (len(p['track']) == 0)
        n_elements += len(p['track'])
    assert n_elements == sum(len(im['point3D_ids']) for im in images)
    ids = {p['id'] for p in points}
    assert all(int(i) in ids for im in images for i in im['point3D_ids'])
    return n_elements


def _edge_cloud(with_tracks=True):
    from dust3r_amd.viz import FusedCloud
    P, pts, masks, wgts, cams, shapes = edge_case_inputs()
    want = restated_tracks(P, pts, masks, wgts, cams, EDGE_MAX_DIST, EDGE_MAX_ERROR)
    P = np.nan_to_num(P, nan=7.0)
    rng = np.random.default_rng(3)
    cloud = FusedCloud(P, rng.integers(0, 256, size=(len(P), 3)).astype(np.uint8), np.ones(len(P), np.float32), np.ones(len(P), np.int32), 0.5,
                       (P.min(axis=0), P.max(axis=0)), tracks=tracks_of(want, shapes) if with_tracks else None)
    return cloud, want, shapes


def test_cloud_tracks_object():
    cloud, want, shapes = _edge_cloud()
    t = cloud.tracks
    assert len(t) == 15 and t.n_points == 21 and t.lengths.tolist() == [len(o) for _, o in EDGE_POINTS]
    assert t.xy().tolist() == [[e % shapes[v][1], e // shapes[v][1]] for _, obs in EDGE_POINTS for v, e in obs]
    err = t.point_error()
    assert err.dtype == np.float64 and err[0] == -1 and err[1] == 1.5 and err[4] == 0 and err[19] == 0 and err[20] == 1
    assert err[16] == (np.sqrt(want['err2'][8]) + np.sqrt(want['err2'][9])) / 2
    s = t.stats()
    assert s['observations'] == 15 and s['mean_track_length'] == 15 / 21 and s['unobserved'] == 9 / 21 and s['observations_per_image'] == [12, 3]
    assert s['mean_error'] == float(np.sqrt(want['err2']).mean()) and s['median_error'] == float(np.median(np.sqrt(want['err2'])))
    import torch
    tt = tracks_of({k: torch.from_numpy(v) for k, v in want.items()}, shapes)                     # the tensor arms, on the host
    assert tt.xy().tolist() == t.xy().tolist() and tt.lengths.tolist() == t.lengths.tolist()
    assert np.allclose(tt.point_error().numpy(), err, rtol=0, atol=1e-12) and tt.stats() == s
    empty = tracks_of(restated_tracks(np.zeros((0, 3), np.float32), *edge_case_inputs()[1:5], 0.5), shapes)
    assert len(empty) == 0 and empty.xy().shape == (0, 2) and empty.point_error().shape == (0,) and empty.stats()['mean_error'] is None


@pytest.mark.parametrize('as_tensors', [False, True])
def test_colmap_round_trip_with_tracks(tmp_path, as_tensors):
    from dust3r_amd.export import read_colmap, write_colmap
    cloud, want, shapes = _edge_cloud()
    scene = _Scene(np.random.default_rng(5), shapes, as_tensors=as_tensors)
    models = {}
    for binary in (True, False):
        out = str(tmp_path / ('bin' if binary else 'txt'))
        files = write_colmap(out, scene, cloud, binary=binary, write_images=False)
        assert len(files) == 3
        models[binary] = read_colmap(os.path.join(out, 'sparse', '0'))
    for cams, images, points in models.values():
        assert colmap_invariant(images, points) == 15
        assert [len(im['xys']) for im in images] == [12, 3] and [len(p['track']) for p in points] == [len(o) for _, o in EDGE_POINTS]
        for v, im in enumerate(images):
            obs = want['image_obs'][want['image_offsets'][v]:want['image_offsets'][v + 1]]
            assert im['xys'].dtype == np.float64 and np.array_equal(im['xys'], cloud.tracks.xy()[obs])
            assert im['point3D_ids'].tolist() == sorted(im['point3D_ids'].tolist())               # ascending point id
        for j, p in enumerate(points):
            assert p['track'][:, 0].tolist() == [v + 1 for v, _ in EDGE_POINTS[j][1]] and p['error'] == cloud.tracks.point_error()[j]
            assert p['xyz'] == tuple(float(c) for c in cloud.positions[j]) and p['rgb'] == tuple(cloud.colors[j].tolist())
    (cb, ib, pb), (ct, it, pt) = models[True], models[False]
    assert cb == ct and len(ib) == len(it) and len(pb) == len(pt)
    for a, b in zip(ib, it):
        assert {k: v for k, v in a.items() if k not in ('xys', 'point3D_ids')} == {k: v for k, v in b.items() if k not in ('xys', 'point3D_ids')}
        assert np.array_equal(a['xys'], b['xys']) and np.array_equal(a['point3D_ids'], b['point3D_ids'])
    for a, b in zip(pb, pt):
        assert {k: v for k, v in a.items() if k != 'track'} == {k: v for k, v in b.items() if k != 'track'} and np.array_equal(a['track'], b['track'])
    head = open(tmp_path / 'txt' / 'sparse' / '0' / 'images.txt').read().split('\n')[3]
    assert head == '# Number of images: 2, mean observations per image: 7.5'
    assert f'mean track length: {15 / 21!r}' in open(tmp_path / 'txt' / 'sparse' / '0' / 'points3D.txt').read().split('\n')[2]


def test_points_file_is_written_in_blocks(tmp_path, monkeypatch):
    """points3D.bin with tracks goes out in blocks of points: blocks of 4 give the bytes of one block"""
    from dust3r_amd import export
    cloud, _, shapes = _edge_cloud()
    scene = _Scene(np.random.default_rng(5), shapes, as_tensors=False)
    export.write_colmap(str(tmp_path / 'a'), scene, cloud, write_images=False)
    monkeypatch.setattr(export, '_POINT_CHUNK', 4)
    export.write_colmap(str(tmp_path / 'b'), scene, cloud, write_images=False)
    assert open(tmp_path / 'a' / 'sparse' / '0' / 'points3D.bin', 'rb').read() == open(tmp_path / 'b' / 'sparse' / '0' / 'points3D.bin', 'rb').read()


def test_tracks_of_another_cloud_are_refused(tmp_path):
    from dust3r_amd.export import write_colmap
    cloud, _, shapes = _edge_cloud()
    with pytest.raises(ValueError, match='tracks of 21 points in 2 images'):
        write_colmap(str(tmp_path), _Scene(np.random.default_rng(5), shapes + [(4, 4)], as_tensors=False), cloud, write_images=False)


# the model of a trackless cloud, as write_colmap wrote it before tracks existed: the formats spelled out once more
def _trackless_model(cams, xyz, rgb, binary):
    import struct
    if binary:
        c = struct.pack('<Q', len(cams)) + b''.join(struct.pack('<iiQQ4d', k['id'], 1, k['width'], k['height'], *k['params']) for k in cams)
        i = struct.pack('<Q', len(cams)) + b''.join(struct.pack('<i4d3di', k['id'], *k['q'], *k['t'], k['id']) + k['name'].encode() + b'\0' + struct.pack('<Q', 0)
                                                    for k in cams)
        p = struct.pack('<Q', len(xyz)) + b''.join(struct.pack('<Q3d3BdQ', j + 1, *xyz[j], *rgb[j], 0.0, 0) for j in range(len(xyz)))
        return c, i, p
    c = ('# Camera list with one line of data per camera:\n#   CAMERA_ID, MODEL, WIDTH, HEIGHT, PARAMS[]\n' + f'# Number of cameras: {len(cams)}\n' +
         ''.join(f"{k['id']} PINHOLE {k['width']} {k['height']} " + ' '.join(repr(float(v)) for v in k['params']) + '\n' for k in cams))
    i = ('# Image list with two lines of data per image:\n#   IMAGE_ID, QW, QX, QY, QZ, TX, TY, TZ, CAMERA_ID, NAME\n#   POINTS2D[] as (X, Y, POINT3D_ID)\n' +
         f'# Number of images: {len(cams)}, mean observations per image: 0\n' +
         ''.join(f"{k['id']} " + ' '.join(repr(float(v)) for v in (*k['q'], *k['t'])) + f" {k['id']} {k['name']}\n\n" for k in cams))
    p = ('# 3D point list with one line of data per point:\n#   POINT3D_ID, X, Y, Z, R, G, B, ERROR, TRACK[] as (IMAGE_ID, POINT2D_IDX)\n' +
         f'# Number of points: {len(xyz)}, mean track length: 0\n' +
         ''.join(f'{j + 1} {float(xyz[j][0])!r} {float(xyz[j][1])!r} {float(xyz[j][2])!r} {rgb[j][0]} {rgb[j][1]} {rgb[j][2]} 0\n' for j in range(len(xyz))))
    return c.encode(), i.encode(), p.encode()


@pytest.mark.parametrize('binary', [True, False])
def test_trackless_cloud_writes_the_bytes_it_always_wrote(tmp_path, binary):
    from dust3r_amd.export import colmap_cameras, read_colmap, write_colmap
    cloud, _, shapes = _edge_cloud(with_tracks=False)
    assert cloud.tracks is None
    scene = _Scene(np.random.default_rng(6), shapes, as_tensors=False)
    files = write_colmap(str(tmp_path), scene, cloud, binary=binary, write_images=False)
    want = _trackless_model(colmap_cameras(scene), cloud.positions.astype(np.float64).tolist(), cloud.colors.tolist(), binary)
    for name, data in zip(files, want):
        assert open(name, 'rb').read() == data, name
    cams, images, points = read_colmap(os.path.join(str(tmp_path), 'sparse', '0'))
    assert all(len(im['xys']) == 0 for im in images) and all(len(p['track']) == 0 and p['error'] == 0 for p in points) and len(points) == 21


def test_fused_cloud_carries_and_drops_tracks():
    """the constructor keeps them; the docstrings say which methods keep and which drop them (those run on the GPU: tests/test_tracks_gpu.py)"""
    from dust3r_amd.viz import FusedCloud
    cloud, _, _ = _edge_cloud()
    assert cloud.tracks is not None and FusedCloud(cloud.positions, cloud.colors, cloud.weight, cloud.count, 0.5, cloud.bounds).tracks is None


def test_track_cameras_are_the_poses_of_the_model():
    from dust3r_amd.export import colmap_cameras, quat_to_rotmat
    from dust3r_amd.viz import track_cameras
    scene = _Scene(np.random.default_rng(8), [(6, 8), (8, 6), (5, 5)], as_tensors=True)
    table = track_cameras(scene.get_intrinsics(), scene.get_im_poses())
    assert table.dtype == np.float64 and table.shape == (3, 16)
    for row, cam in zip(table, colmap_cameras(scene)):
        assert np.array_equal(row[:9].reshape(3, 3), quat_to_rotmat(cam['q'])) and np.array_equal(row[9:12], cam['t']) and tuple(row[12:]) == cam['params']


def test_demo_flags():
    from dust3r_amd.demo import get_args_parser, wants_fuse
    parse = lambda *extra: get_args_parser().parse_args(['pics', '--weights', 'w.pth', *extra])      # noqa: E731
    plain = parse('--colmap')
    assert plain.colmap_tracks is False and plain.max_reproj_error is None
    a = parse('--colmap', '--colmap_tracks', '--max_reproj_error', '1.5')
    assert a.colmap_tracks is True and a.max_reproj_error == 1.5 and wants_fuse(a)


# ---- the build ----------------------------------------------------------------------------------------------------------------------------
def test_tracks_entry_points_are_exported():
    from dust3r_amd import _lib
    assert {'d3r_cloud_tracks_workspace_bytes', 'd3r_cloud_tracks_count', 'd3r_cloud_tracks_fill'} <= set(_lib.EXPORTED)
    assert _lib.lib.d3r_cloud_tracks_workspace_bytes(0) == 0 and _lib.lib.d3r_cloud_tracks_workspace_bytes(-5) == 0
    # two key buffers and one index buffer of `capacity` rows and the digit counts
    assert 20 * 10 ** 6 <= _lib.lib.d3r_cloud_tracks_workspace_bytes(10 ** 6) < 21 * 10 ** 6


def test_tracks_resource_report_has_no_scratch():
    """read only: the report is what the build left next to the object; nothing is built or touched here"""
    from dust3r_amd import _lib
    path = os.path.join(os.path.dirname(_lib.LIB_PATH), 'tracks.resources.txt')
    if not os.path.exists(path):
        pytest.skip('no tracks.resources.txt: the library was not built by dust3r_amd/build.py')
    report = open(path).read()
    kernels = re.findall(r'Function Name: (\S+)', report)
    assert sum('tracks_' in k for k in kernels) == 5 and all('tracks_' in k or 'fuse_' in k for k in kernels)
    assert re.findall(r'ScratchSize \[bytes/lane\]: (\d+)', report) == ['0'] * len(kernels)
