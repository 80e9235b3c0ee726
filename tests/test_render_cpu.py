"""The headless renderer (csrc/render.hip, dust3r_amd.viz.render_batch / SceneViz) without a GPU: a numpy restatement of its two stages --
the vertex stage in fp64, the integer raster stage exactly -- checked against hand-worked cases so that tests/test_render_gpu.py can hold the
kernels to it, and the host logic (default viewpoint, turntable poses, argument validation, the add_pointcloud overloads)."""
import numpy as np
import pytest
import torch

GUARD = 8192
ZQ_MAX = 0xFFFFFF
INVALID = 0xFFFFFFFF
EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)


# ---- the restatement ------------------------------------------------------------------------------------------------------------------
def restated_project(positions, w2c, intr, near):
    """fp64 vertex stage for ONE camera: positions (N, 3), w2c (12,) or (16,) rows [R | t], intr (fx, fy, cx, cy). Returns dict(sx, sy
    (int64, 1/16 px), zq (int64, INVALID where not valid), valid, x, y, Z (the continuous fp64 values, NaN-free only where finite))."""
    p = np.asarray(positions, dtype=np.float64).reshape(-1, 3)
    M = np.asarray(w2c, dtype=np.float64)[:12].reshape(3, 4)
    fx, fy, cx, cy = [float(v) for v in intr]
    finite = np.isfinite(p).all(axis=1)
    q = np.where(finite[:, None], p, 0.0)
    cam = q @ M[:, :3].T + M[:, 3]
    Z = cam[:, 2]
    with np.errstate(divide='ignore', invalid='ignore'):
        x = fx * (cam[:, 0] / Z) + cx
        y = fy * (cam[:, 1] / Z) + cy
        valid = finite & (Z > near) & (np.abs(x) <= GUARD) & (np.abs(y) <= GUARD)
        sx = np.where(valid, np.rint(16 * np.where(valid, x, 0)), 0).astype(np.int64)
        sy = np.where(valid, np.rint(16 * np.where(valid, y, 0)), 0).astype(np.int64)
        zq = np.where(valid, ZQ_MAX - np.rint(near / np.where(valid, Z, 1.0) * ZQ_MAX), INVALID).astype(np.int64)
    return dict(sx=sx, sy=sy, zq=zq, valid=valid, x=x, y=y, Z=Z, finite=finite)


def splat_offsets(point_size):
    return list(range(-((point_size - 1) // 2), point_size // 2 + 1))


def _key(zq, prim):
    return (np.uint64(zq) << np.uint64(32)) | np.uint64(prim)


def _edge(ax, ay, bx, by, px, py):
    return (bx - ax) * (py - ay) - (by - ay) * (px - ax)


def _top_left(ax, ay, bx, by):
    return by < ay or (by == ay and bx > ax)


def face_samples(v, W, H):
    """The pixels a face covers. v: three (sx, sy, zq) integer triples in the face's own order. Returns (px, py, zq, (w_a, w_b, w_c), area2)
    with Python-int weights belonging to the vertices in the GIVEN order, or None for a face that draws nothing."""
    (x0, y0, z0), (x1, y1, z1), (x2, y2, z2) = [tuple(int(t) for t in u) for u in v]
    if INVALID in (z0, z1, z2):
        return None
    area2 = _edge(x0, y0, x1, y1, x2, y2)
    if area2 == 0:
        return None
    swapped = area2 < 0
    if swapped:
        (x1, y1, z1), (x2, y2, z2) = (x2, y2, z2), (x1, y1, z1)
        area2 = -area2
    bx0, bx1 = max(-(-min(x0, x1, x2) // 16), 0), min(max(x0, x1, x2) // 16, W - 1)
    by0, by1 = max(-(-min(y0, y1, y2) // 16), 0), min(max(y0, y1, y2) // 16, H - 1)
    if bx0 > bx1 or by0 > by1:
        return None
    py, px = np.meshgrid(np.arange(by0, by1 + 1, dtype=np.int64), np.arange(bx0, bx1 + 1, dtype=np.int64), indexing='ij')
    px, py = px.ravel(), py.ravel()
    qx, qy = 16 * px, 16 * py
    edges = [((x1, y1), (x2, y2)), ((x2, y2), (x0, y0)), ((x0, y0), (x1, y1))]
    w, cover = [], np.ones(len(px), bool)
    for (a, b) in edges:
        e = _edge(a[0], a[1], b[0], b[1], qx, qy)                # |e| < 2^37: int64 is exact
        cover &= (e > 0) | ((e == 0) & _top_left(a[0], a[1], b[0], b[1]))
        w.append(e)
    px, py, w = px[cover], py[cover], [e[cover] for e in w]
    zq = (w[0] * z0 + w[1] * z1 + w[2] * z2) // area2           # < 2^61
    if swapped:
        w = [w[0], w[2], w[1]]
    return px, py, zq, w, area2


def restated_raster(W, H, points=None, tris=None, background=(255, 255, 255)):
    """The integer raster stage for one camera. points: dict(sx, sy, zq (INVALID = skip), mask or None, rgba (N,) packed, point_size, id_base);
    tris: dict(sx, sy, zq per VERTEX, faces (M, 3), rgba (V,) packed, id_base). Returns keys (H, W) uint64, ids (H, W) int32, rgb (H, W, 3) uint8."""
    keys = np.full((H, W), EMPTY, dtype=np.uint64)
    if points is not None:
        sx, sy, zq = [np.asarray(points[k], dtype=np.int64) for k in ('sx', 'sy', 'zq')]
        use = zq != INVALID
        if points.get('mask') is not None:
            use &= np.asarray(points['mask']).astype(bool)
        idx = np.nonzero(use)[0]
        bx, by = (sx[idx] + 8) // 16, (sy[idx] + 8) // 16
        k = _key(zq[idx], idx + points.get('id_base', 0))
        for dy in splat_offsets(points.get('point_size', 1)):
            for dx in splat_offsets(points.get('point_size', 1)):
                x, y = bx + dx, by + dy
                inside = (x >= 0) & (x < W) & (y >= 0) & (y < H)
                np.minimum.at(keys, (y[inside], x[inside]), k[inside])
    if tris is not None:
        tsx, tsy, tzq = [np.asarray(tris[k], dtype=np.int64) for k in ('sx', 'sy', 'zq')]
        for j, f in enumerate(np.asarray(tris['faces'], dtype=np.int64)):
            s = face_samples([(tsx[i], tsy[i], tzq[i]) for i in f], W, H)
            if s is None:
                continue
            px, py, zq, _, _ = s
            keys[py, px] = np.minimum(keys[py, px], _key(zq, j + tris['id_base']))
    return (keys,) + restated_resolve(keys, points, tris, background)


def restated_resolve(keys, points, tris, background=(255, 255, 255)):
    H, W = keys.shape
    ids = np.where(keys == EMPTY, -1, (keys & np.uint64(0xFFFFFFFF)).astype(np.int64)).astype(np.int32)
    rgb = np.empty((H, W, 3), np.uint8)
    rgb[:] = np.asarray(background, dtype=np.uint8)
    n_pts = 0 if points is None else len(points['zq'])
    pbase = 0 if points is None else points.get('id_base', 0)
    for y, x in zip(*np.nonzero(ids >= 0)):
        prim = int(ids[y, x])
        if 0 <= prim - pbase < n_pts:
            c = int(np.asarray(points['rgba'])[prim - pbase]) & 0xFFFFFFFF
            rgb[y, x] = [c & 0xFF, (c >> 8) & 0xFF, (c >> 16) & 0xFF]
        else:
            f = np.asarray(tris['faces'], dtype=np.int64)[prim - tris['id_base']]
            v = [(int(tris['sx'][i]), int(tris['sy'][i]), int(tris['zq'][i])) for i in f]
            area2 = abs(_edge(v[0][0], v[0][1], v[1][0], v[1][1], v[2][0], v[2][1]))
            qx, qy = 16 * int(x), 16 * int(y)
            sign = 1 if _edge(v[0][0], v[0][1], v[1][0], v[1][1], v[2][0], v[2][1]) > 0 else -1
            w = [sign * _edge(v[1][0], v[1][1], v[2][0], v[2][1], qx, qy), sign * _edge(v[2][0], v[2][1], v[0][0], v[0][1], qx, qy),
                 sign * _edge(v[0][0], v[0][1], v[1][0], v[1][1], qx, qy)]
            cols = [int(np.asarray(tris['rgba'])[i]) & 0xFFFFFFFF for i in f]
            rgb[y, x] = [(sum(wk * ((c >> sh) & 0xFF) for wk, c in zip(w, cols)) + area2 // 2) // area2 for sh in (0, 8, 16)]
    return ids, rgb


def zq_of(keys):
    return (keys >> np.uint64(32)).astype(np.int64)


def rgba(r, g, b):
    return np.int32(r | (g << 8) | (b << 16)) | np.int32(-16777216)


def _tri(verts, faces, cols=None, id_base=0, zq=None):
    verts = np.asarray(verts, dtype=np.int64)
    n = len(verts)
    return dict(sx=verts[:, 0], sy=verts[:, 1], zq=np.full(n, 1000, np.int64) if zq is None else np.asarray(zq, dtype=np.int64), faces=np.asarray(faces),
                rgba=np.array([rgba(10, 20, 30)] * n) if cols is None else np.asarray(cols), id_base=id_base)


# ---- hand-worked cases of the raster stage --------------------------------------------------------------------------------------------
SQUARE = [(16, 16), (80, 16), (80, 80), (16, 80)]            # corners at pixel centres 1 and 5: covers centres 1 ... 4 (right and bottom edges open)


@pytest.mark.parametrize('faces', [[(0, 1, 2), (0, 2, 3)], [(0, 2, 1), (0, 3, 2)], [(0, 2, 3), (0, 1, 2)], [(2, 0, 1), (3, 2, 0)],
                                   [(0, 1, 3), (1, 2, 3)], [(3, 1, 0), (1, 3, 2)]])
def test_two_faces_sharing_a_diagonal_cover_each_pixel_once(faces):
    W = H = 8
    count = np.zeros((H, W), int)
    for f in faces:
        px, py, _, _, _ = face_samples([SQUARE[i] + (5,) for i in f], W, H)
        np.add.at(count, (py, px), 1)
    want = np.zeros((H, W), int)
    want[1:5, 1:5] = 1                                          # top and left edges (through centres 1) in, right and bottom (centres 5) out
    assert np.array_equal(count, want)
    keys, ids, _ = restated_raster(W, H, tris=_tri(SQUARE, faces, id_base=7))
    assert set(ids[1:5, 1:5].ravel()) == {7, 8} and (ids[want == 0] == -1).all()
    assert (zq_of(keys)[want == 1] == 1000).all()


def test_edge_through_pixel_centres_belongs_to_one_side():
    """(0,0)-(4,4) px diagonal: the centres (k, k) lie exactly on it. For the lower-left face the diagonal runs up-right seen clockwise... by the
    rule it is a LEFT edge of the upper-right face only when that face's edge goes up; worked by hand: the face (0,0),(4,0),(4,4) has the
    diagonal as the edge (4,4) -> (0,0), going up: it owns the centres on the diagonal."""
    W = H = 6
    upper = face_samples([(0, 0, 1), (64, 0, 1), (64, 64, 1)], W, H)
    lower = face_samples([(0, 0, 1), (64, 64, 1), (0, 64, 1)], W, H)
    up = set(zip(upper[0].tolist(), upper[1].tolist()))
    lo = set(zip(lower[0].tolist(), lower[1].tolist()))
    # upper: top edge y = 0 in, right edge x = 4 out, diagonal in -> x in [y, 3]
    assert up == {(x, y) for y in range(4) for x in range(y, 4)}
    # lower: left edge x = 0 in, bottom edge y = 4 out, diagonal out -> x in [0, y - 1], y in 1 ... 3
    assert lo == {(x, y) for y in range(1, 4) for x in range(0, y)}
    assert not (up & lo)


def test_zero_area_and_invalid_faces_draw_nothing():
    assert face_samples([(0, 0, 1), (32, 32, 1), (64, 64, 1)], 8, 8) is None
    assert face_samples([(16, 16, 1), (16, 16, 1), (64, 0, 1)], 8, 8) is None
    assert face_samples([(0, 0, 1), (64, 0, INVALID), (64, 64, 1)], 8, 8) is None
    assert face_samples([(-64, -64, 1), (-16, -64, 1), (-16, -16, 1)], 8, 8) is None        # outside the frame
    keys, ids, rgb = restated_raster(4, 4, tris=_tri([(0, 0), (32, 32), (64, 64)], [(0, 1, 2)]))
    assert (keys == EMPTY).all() and (ids == -1).all() and (rgb == 255).all()


def test_points_lower_id_wins_at_equal_depth_and_nearer_wins():
    pts = dict(sx=[40, 41, 33], sy=[24, 25, 30], zq=[500, 500, 400], mask=None, rgba=[rgba(1, 2, 3), rgba(4, 5, 6), rgba(7, 8, 9)], point_size=1)
    keys, ids, rgb = restated_raster(6, 4, points=pts, background=(0, 0, 0))
    # (40 + 8) // 16 = 3, (24 + 8) // 16 = 2: points 0 and 1 share pixel (3, 2); point 2 lands on (2, 2)
    assert ids[2, 3] == 0 and tuple(rgb[2, 3]) == (1, 2, 3)
    assert ids[2, 2] == 2 and tuple(rgb[2, 2]) == (7, 8, 9)
    assert (ids >= 0).sum() == 2
    pts['zq'] = [500, 499, 400]
    assert restated_raster(6, 4, points=pts)[1][2, 3] == 1
    pts['mask'] = [1, 0, 1]
    assert restated_raster(6, 4, points=pts)[1][2, 3] == 0
    pts['id_base'] = 10
    assert restated_raster(6, 4, points=pts)[1][2, 3] == 10


def test_pixel_of_a_point_rounds_half_up():
    """a pixel covers [p - 1/2, p + 1/2): sx = 16 p - 8 is the first unit of pixel p, 16 p + 7 the last"""
    for sx, want in [(-9, -1), (-8, 0), (7, 0), (8, 1), (23, 1), (24, 2)]:
        assert (sx + 8) // 16 == want


def test_splat_offsets():
    assert splat_offsets(1) == [0]
    assert splat_offsets(2) == [0, 1]
    assert splat_offsets(3) == [-1, 0, 1]
    assert splat_offsets(4) == [-1, 0, 1, 2]
    pts = dict(sx=[32], sy=[32], zq=[9], mask=None, rgba=[rgba(0, 0, 0)], point_size=3)
    ids = restated_raster(6, 6, points=pts)[1]
    assert np.array_equal(np.argwhere(ids == 0), [(y, x) for y in (1, 2, 3) for x in (1, 2, 3)])
    pts.update(point_size=2, sx=[0], sy=[80])                       # clipped at the frame: base (0, 5), offsets 0, +1
    assert np.array_equal(np.argwhere(restated_raster(6, 6, points=pts)[1] == 0), [(5, 0), (5, 1)])


def test_large_face_interpolates_to_the_vertex_values_at_its_corners():
    verts = [(0, 0), (160 * 16, 0), (0, 120 * 16)]
    zq = [100, 90000, 16000000]
    cols = [rgba(255, 0, 10), rgba(0, 255, 20), rgba(3, 7, 250)]
    for faces in ([(0, 1, 2)], [(0, 2, 1)], [(2, 0, 1)]):
        keys, ids, rgb = restated_raster(161, 121, tris=_tri(verts, faces, cols, zq=zq))
        assert ids[0, 0] == 0 and zq_of(keys)[0, 0] == 100 and tuple(rgb[0, 0]) == (255, 0, 10)         # the corner on the top-left edges is covered
        assert ids[0, 160] == -1 and ids[120, 0] == -1                                                # the other two lie on open edges
        px, py, z, w, area2 = face_samples([verts[i] + (zq[i],) for i in faces[0]], 161, 121)
        assert area2 == 160 * 16 * 120 * 16
        # next to the corners the weights are the hand values: pixel (159, 0) is 1/160 from v1 towards v0
        at = {(int(x), int(y)): k for k, (x, y) in enumerate(zip(px, py))}
        k = at[(159, 0)]
        by_vertex = {faces[0][i]: int(w[i][k]) for i in range(3)}
        assert by_vertex == {0: area2 // 160, 1: area2 * 159 // 160, 2: 0}
        assert int(z[k]) == (100 * 1 + 90000 * 159) // 160
        assert tuple(rgb[0, 159]) == ((255 * 1 + 80) // 160, (255 * 159 + 80) // 160, (10 + 20 * 159 + 80) // 160)
        k = at[(0, 119)]
        assert int(z[k]) == (100 * 1 + 16000000 * 119) // 120
    # the vertex values themselves, at corners moved inside the frame's open side: a face whose three corners are covered samples
    verts = [(16, 16), (1616, 16), (17, 1616)]
    px, py, z, w, area2 = face_samples([verts[i] + (zq[i],) for i in range(3)], 200, 200)
    at = {(int(x), int(y)): k for k, (x, y) in enumerate(zip(px, py))}
    assert int(z[at[(1, 1)]]) == 100 and [int(w[i][at[(1, 1)]]) for i in range(3)] == [area2, 0, 0]


def test_bounds_of_the_integer_arithmetic():
    """|sx| <= 2^17 and samples within the same range: an edge function < 2^37, area2 zq < 2^61, the colour sum < 2^46: all in int64"""
    s = 16 * GUARD
    e = _edge(-s, -s, s, -s, s, s)
    assert e == (2 * s) ** 2 == 2 ** 36 and 2 * e * ZQ_MAX < 2 ** 63 and 2 * e * 255 + e < 2 ** 63
    out = face_samples([(-s, -s, ZQ_MAX), (s, -s, ZQ_MAX), (0, s, ZQ_MAX)], 4, 4)
    assert len(out[0]) == 16 and (out[2] == ZQ_MAX).all()


# ---- the vertex stage -----------------------------------------------------------------------------------------------------------------
def test_restated_project_by_hand():
    w2c = np.eye(4)[:3].reshape(-1)
    intr = (100.0, 50.0, 32.0, 24.0)
    p = np.array([[0, 0, 2.0], [1, -1, 4.0], [0, 0, 0.05], [np.nan, 0, 1], [0, 0, np.inf], [1000.0, 0, 1.0], [0.3, 0.2, 1.0]])
    r = restated_project(p, w2c, intr, near=0.1)
    assert r['valid'].tolist() == [True, True, False, False, False, False, True]
    assert (r['sx'][0], r['sy'][0]) == (512, 384)                                    # the principal point, in 1/16 px
    assert (r['sx'][1], r['sy'][1]) == (16 * 57, 16 * 24 - 200)                     # 32 + 25, 24 - 12.5
    assert r['zq'][0] == ZQ_MAX - round(0.05 * ZQ_MAX) and r['zq'][2] == INVALID
    assert r['zq'][1] > r['zq'][0]                                                   # farther = larger
    # 1000 * 100 + 32 px is outside the guard band
    assert abs(r['x'][5]) > GUARD
    # zq is linear in 1 / Z: Z back from zq
    Z = 0.1 * ZQ_MAX / (ZQ_MAX - r['zq'][[0, 1, 6]])
    assert np.allclose(Z, [2, 4, 1], rtol=1e-6)
    # a pointmap's own pixel: (u - W/2) / f * d unprojects to exactly (u, v)
    u, v, f, d = 13, 7, 60.0, 3.0
    r = restated_project([[(u - 32) / f * d, (v - 24) / f * d, d]], w2c, (f, f, 32.0, 24.0), near=0.1)
    assert (r['sx'][0], r['sy'][0]) == (16 * u, 16 * v)


# ---- host logic -------------------------------------------------------------------------------------------------------------------------
def _is_rigid(pose):
    R = pose[:3, :3]
    return np.allclose(R @ R.T, np.eye(3), atol=1e-12) and np.isclose(np.linalg.det(R), 1) and np.allclose(pose[3], [0, 0, 0, 1])


def test_turntable_poses_are_rigid_and_look_at_the_centre():
    from dust3r_amd.viz import fit_distance, turntable_poses
    lo, hi = np.array([-1.0, -2, 0]), np.array([3.0, 2, 4])
    centre, radius = (lo + hi) / 2, np.linalg.norm(hi - lo) / 2
    for down in ((0, 1, 0), (1, 0, 0), (0.2, -0.9, 0.3)):
        poses = turntable_poses((lo, hi), 12, 500.0, (640, 480), down=down, elevation_deg=25)
        assert poses.shape == (12, 4, 4)
        dist = fit_distance(radius, 500.0, (640, 480))
        d = np.asarray(down, float) / np.linalg.norm(down)
        for P in poses:
            assert _is_rigid(P)
            to_centre = centre - P[:3, 3]
            assert np.isclose(np.linalg.norm(to_centre), dist)
            assert np.allclose(P[:3, 2], to_centre / dist, atol=1e-12)               # the optical axis passes through the centre
            assert P[:3, 1] @ d > 0                                                 # y points down
            assert np.isclose((P[:3, 3] - centre) @ d / dist, -np.sin(np.deg2rad(25)))   # raised against `down`
        assert len({tuple(np.round(P[:3, 3], 9)) for P in poses}) == 12
    # the sphere fits: its silhouette angle is below the half field of view of the smaller side
    assert np.arcsin(radius / dist) < np.arctan(480 / 2 / 500.0)
    with pytest.raises(ValueError):
        turntable_poses((lo, hi), 0, 500.0, (640, 480))


def test_default_viewpoint_rule():
    from dust3r_amd.viz import default_viewpoint, fit_distance, look_at
    cam = look_at([0.0, 0, -3], [0.5, 0.2, 0])
    lo, hi = np.array([-1.0, -1, -1]), np.array([1.0, 2, 1])
    P = default_viewpoint(cam, (lo, hi), 400.0, (320, 240))
    assert _is_rigid(P) and np.allclose(P[:3, :3], cam[:3, :3])                       # the first camera's orientation
    centre, radius = (lo + hi) / 2, np.linalg.norm(hi - lo) / 2
    dist = fit_distance(radius, 400.0, (320, 240))
    assert np.allclose(P[:3, 3] + dist * P[:3, 2], centre)                            # pulled back along its own axis from the centre
    # every corner of the bounds projects inside the frame
    corners = np.array([[x, y, z] for x in (lo[0], hi[0]) for y in (lo[1], hi[1]) for z in (lo[2], hi[2])])
    r = restated_project(corners, np.linalg.inv(P)[:3].reshape(-1), (400.0, 400.0, 160.0, 120.0), near=1e-3)
    assert r['valid'].all() and (r['x'] >= 0).all() and (r['x'] <= 319).all() and (r['y'] >= 0).all() and (r['y'] <= 239).all()
    assert np.allclose(default_viewpoint(None, (lo, hi), 400.0, (320, 240))[:3, :3], np.eye(3))


def test_intrinsics_rows_and_world_to_cam():
    from dust3r_amd.viz import intrinsics_rows, look_at, world_to_cam
    assert np.array_equal(intrinsics_rows(100.0, 2, (64, 48)), np.float32([[100, 100, 32, 24]] * 2))
    assert np.array_equal(intrinsics_rows([100.0, 50.0], 2, (64, 48)), np.float32([[100, 100, 32, 24], [50, 50, 32, 24]]))
    K = np.array([[80.0, 0, 30], [0, 90, 20], [0, 0, 1]])
    assert np.array_equal(intrinsics_rows(K, 3, (64, 48)), np.float32([[80, 90, 30, 20]] * 3))
    assert np.array_equal(intrinsics_rows(torch.tensor(np.stack([K, 2 * K])), 2, (64, 48))[1], np.float32([160, 180, 60, 40]))
    for bad in ([1.0, 2.0, 3.0], -5.0, np.nan):
        with pytest.raises(ValueError):
            intrinsics_rows(bad, 2, (64, 48))
    P = look_at([1.0, 2, 3], [0, 0, 0])
    rows = world_to_cam(P)
    assert rows.shape == (1, 12) and rows.dtype == np.float32
    assert np.allclose(rows.reshape(3, 4) @ np.array([1.0, 2, 3, 1]), 0, atol=1e-6)     # the camera centre maps to the origin
    assert world_to_cam(np.stack([P, P])).shape == (2, 12)


def test_add_pointcloud_overloads_give_the_flat_arrays():
    from dust3r_amd.viz import SceneViz, pack_rgba
    rng = np.random.default_rng(0)
    p1, p2 = rng.normal(size=(3, 4, 3)).astype(np.float32), rng.normal(size=(2, 5, 3)).astype(np.float32)
    im1, im2 = rng.random((3, 4, 3)).astype(np.float32), rng.random((2, 5, 3)).astype(np.float32)
    m1, m2 = rng.random((3, 4)) < 0.5, rng.random((2, 5)) < 0.5

    def q(im):
        v = np.floor(im.reshape(-1, 3) * np.float32(255) + np.float32(0.5)).clip(0, 255).astype(np.int64)
        return (v[:, 0] | (v[:, 1] << 8) | (v[:, 2] << 16) | (255 << 24)).astype(np.uint32).view(np.int32)
    # a list of maps, a list of images, a list of masks
    g = SceneViz().add_pointcloud([p1, torch.from_numpy(p2)], [im1, im2], [m1, torch.from_numpy(m2)]).flat_arrays('cpu')
    assert np.array_equal(g['points'].numpy(), np.r_[p1.reshape(-1, 3), p2.reshape(-1, 3)])
    assert np.array_equal(g['point_colors'].numpy(), np.r_[q(im1), q(im2)])
    assert np.array_equal(g['point_mask'].numpy(), np.r_[m1.ravel(), m2.ravel()].astype(np.uint8)) and g['point_mask'].dtype == torch.uint8
    assert g['faces'] is None and g['vertices'] is None
    # one map, one colour for all, no mask; then one map with a uint8 image and a mask
    v = SceneViz().add_pointcloud(p1, (1, 2, 3))
    g = v.flat_arrays('cpu')
    assert g['point_mask'] is None and (g['point_colors'].numpy().view(np.uint32) == (1 | 2 << 8 | 3 << 16 | 255 << 24)).all() and len(g['points']) == 12
    u8 = (im2 * 255).astype(np.uint8)
    g = v.add_pointcloud(p2, u8, m2).flat_arrays('cpu')
    assert len(g['points']) == 22 and np.array_equal(g['point_mask'].numpy(), np.r_[np.ones(12), m2.ravel()].astype(np.uint8))
    assert np.array_equal(g['point_colors'].numpy()[12:].view(np.uint8).reshape(-1, 4)[:, :3], u8.reshape(-1, 3))
    # a flat colour as a list for a list of maps
    g = SceneViz().add_pointcloud([p1, p2], (9, 8, 7)).flat_arrays('cpu')
    assert len(g['point_colors']) == 22 and (g['point_colors'] == int(pack_rgba(np.uint8([9, 8, 7]))[0])).all()
    for bad in (dict(pts3d=[p1, p2], color=[im1]), dict(pts3d=[p1], color=[im2]), dict(pts3d=[p1], color=(1, 2, 3), mask=[m2]),
                dict(pts3d=[p1, p2], color=(1, 2, 3), mask=[m1])):
        with pytest.raises(ValueError):
            SceneViz().add_pointcloud(**bad)


def test_add_camera_appends_the_wire_glyph_and_bounds_skip_masked_points():
    from dust3r_amd.viz import SceneViz, auto_cam_size, look_at, scene_camera_geometry
    P = look_at([0.0, 0, -2], [0, 0, 0])
    v = SceneViz().add_pointcloud(np.float32([[0, 0, 0], [5, 5, 5], [np.nan, 0, 0]]), (0, 0, 0), np.array([True, False, True]))
    assert np.array_equal(v.flat_arrays('cpu')['points'].shape, (3, 3))
    v.device = torch.device('cpu')
    lo, hi = v.bounds()
    assert np.array_equal(lo, [0, 0, 0]) and np.array_equal(hi, [0, 0, 0])               # the masked and the NaN point are left out
    v.add_cameras([P, P], focals=[50.0, 60.0], imsizes=[(64, 48), (48, 64)], colors=[(255, 0, 0), (0, 255, 0)], cam_size=0.1)
    g = v.flat_arrays('cpu')
    cam = scene_camera_geometry(P, 50.0, (64, 48), screen_width=0.1)
    assert g['vertices'].shape == (36, 3) and g['faces'].shape == (96, 3) and g['faces'].dtype == torch.int32
    assert np.allclose(g['vertices'][:18].numpy(), cam['wire_vertices'], atol=1e-6)
    assert np.array_equal(g['faces'][:48].numpy(), cam['wire_faces']) and np.array_equal(g['faces'][48:].numpy() - 18, cam['wire_faces'])
    assert (g['vertex_colors'][:18].numpy().view(np.uint32) == (255 | 255 << 24)).all()
    assert v.cam_focals == [50.0, 60.0] and len(v.cam_poses) == 2
    with pytest.raises(ValueError):
        SceneViz().add_camera(P, 50.0)                                              # no size known
    poses = np.stack([look_at([float(k), 0, 0], [float(k), 0, 1]) for k in range(3)])
    assert np.isclose(auto_cam_size(poses), 0.1)                                     # distances 0 (x3), 1 (x4), 2 (x2): median 1


def test_unused_vertices_and_masked_points_move_neither_the_framing_nor_the_near_plane():
    """the export's mesh keeps every pixel as a vertex, masked or not: a masked-out vertex far away (sky, low confidence) that no face uses
    must change neither bounds(), nor the turntable, nor the default viewpoint, nor the default near plane -- in mesh and in point-cloud mode"""
    from dust3r_amd.viz import SceneViz, look_at, turntable_poses
    verts = np.float32([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0.5]])
    faces = np.array([[0, 1, 2], [2, 1, 3]])
    far = np.float32([[900, -700, 5000], [np.nan, 0, 0], [-4000, 10, 10]])
    cam = look_at([0.5, 0.5, -3], [0.5, 0.5, 0])

    def views(add):
        v = SceneViz()
        v.device = torch.device('cpu')
        add(v)
        v.add_camera(cam, 60.0, imsize=(64, 48), cam_size=0.1)
        b = v.bounds()
        pose, f = v.default_view((64, 48))
        return b, v.default_near(), pose, turntable_poses(b, 6, 70.0, (64, 48))
    want = views(lambda v: v.add_mesh(verts, faces, (1, 2, 3)))
    got = views(lambda v: v.add_mesh(np.r_[verts, far], faces, (1, 2, 3)))
    for a, b in zip(want, got):
        assert np.array_equal(np.asarray(a), np.asarray(b))
    assert want[0][1][2] == 0.5 and want[1] == 0.01 * float(np.linalg.norm(want[0][1] - want[0][0]))
    packed = torch.full((7,), -1, dtype=torch.int32)                                  # colours already packed, faces as int32 tensors
    v = SceneViz().add_mesh(torch.from_numpy(np.r_[verts, far]), torch.from_numpy(faces.astype(np.int32)), packed)
    v.device = torch.device('cpu')
    assert np.array_equal(v.bounds()[1], [1, 1, 0.5]) and v.flat_arrays('cpu')['faces'].dtype == torch.int32
    want = views(lambda v: v.add_pointcloud(verts, (1, 2, 3)))
    got = views(lambda v: v.add_pointcloud(np.r_[verts, far], (1, 2, 3), np.r_[np.ones(4, bool), np.zeros(3, bool)]))
    for a, b in zip(want, got):
        assert np.array_equal(np.asarray(a), np.asarray(b))
    with pytest.raises(ValueError):
        SceneViz().add_mesh(verts, np.array([[0, 1, 4]]), (1, 2, 3))


def test_render_arguments_are_validated_before_the_device_is_touched():
    from dust3r_amd.viz import SceneViz, render_batch
    pose, intr = np.eye(4)[None], np.float32([[10, 10, 4, 4]])
    for kw in (dict(size=(0, 8)), dict(size=(8, 8193)), dict(size=(8, 8), point_size=0), dict(size=(8, 8), point_size=17),
               dict(size=(8, 8), near=0.0), dict(size=(8, 8), near=float('nan'))):
        with pytest.raises(ValueError):
            render_batch(pose, intr, device='cuda:0', **kw)
    with pytest.raises(ValueError, match='nothing to show'):
        v = SceneViz()
        v.device = torch.device('cpu')
        v.default_view()


def test_c_abi_declares_the_render_entry_points():
    import os
    from dust3r_amd import _lib
    names = {'d3r_render_project', 'd3r_render_clear', 'd3r_render_points', 'd3r_render_triangles', 'd3r_render_resolve'}
    assert names <= set(_lib.EXPORTED)
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'dust3r_hip.h')).read()
    assert all(f'int {n}(' in header for n in names)


def test_render_kernels_use_no_scratch():
    import os
    import re
    from dust3r_amd.build import CSRC, build
    rep = os.path.join(CSRC, 'render.resources.txt')
    if not os.path.exists(rep) or os.path.getmtime(rep) < os.path.getmtime(os.path.join(CSRC, 'render.hip')):
        os.utime(os.path.join(CSRC, 'render.hip'))
        build(force=False, verbose=False)
    txt = open(rep).read()
    kernels = re.findall(r'Function Name: (\S*render_\w+_kernel\S*)', txt)
    scratch = [int(x) for x in re.findall(r'ScratchSize \[bytes/lane\]: (\d+)', txt)]
    assert len(kernels) == 6 and len(scratch) == 6 and all(v == 0 for v in scratch), list(zip(kernels, scratch))
