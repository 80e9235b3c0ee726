"""File formats other tools read, for the fused cloud of `scene.fuse()` (viz.FusedCloud): binary PLY, and a COLMAP model (sparse/0 +
images/, the layout Gaussian-splatting trainers take). Host only: struct and numpy; bulk bytes go out through memoryview, as in glb.py.

A cloud that carries tracks (`FusedCloud.build_tracks`, `scene.fuse(tracks=True)`) is written with them: every image's POINTS2D and every
point's track and mean reprojection error; a cloud without them gives the model as before (no image has a 2-D point, every track is
empty). `read_colmap` reads either encoding back.

Out of scope: meshing, TSDF fusion, normals in the COLMAP model, ASCII PLY."""
import os
import struct

import numpy as np

_PLY_VERTEX = [('x', '<f4'), ('y', '<f4'), ('z', '<f4'), ('red', 'u1'), ('green', 'u1'), ('blue', 'u1')]
_PLY_TYPES = {'<f4': 'float', 'u1': 'uchar', '<i4': 'int'}
_PLY_NORMAL = [('nx', '<f4'), ('ny', '<f4'), ('nz', '<f4')]       # directly after z, where MeshLab, Open3D and Poisson reconstruction expect them
_PLY_OPTIONAL = {'confidence': '<f4', 'count': '<i4', 'label': '<i4', 'plane': '<i4'}

CAMERA_MODEL_PINHOLE = 1        # COLMAP's model id of PINHOLE (fx, fy, cx, cy)


def _host(x):
    """numpy array of a numpy array or a (device) tensor"""
    return x.detach().cpu().numpy() if hasattr(x, 'detach') else np.asarray(x)


def _rgb_rows(colors, n):
    """(n, 3) uint8 of (n, 3) or (n, 4) colours (alpha dropped)"""
    colors = np.asarray(_host(colors), dtype=np.uint8)
    return colors.reshape(n, colors.shape[-1] if colors.ndim > 1 else 3)[:, :3]


# ---- PLY ------------------------------------------------------------------------------------------------------------------------------
def write_ply(path, positions, colors, weight=None, count=None, normals=None, labels=None, planes=None):
    """Binary little-endian PLY: per vertex `float x y z`, `float nx ny nz` when normals are given, `uchar red green blue`, then
    `float confidence` (weight), `int count`, `int label` (the cluster of `FusedCloud.cluster`, -1 = noise) and `int plane` (the plane of
    `FusedCloud.detect_planes`, -1 = none) when given. positions (M, 3), colors (M, 3) or (M, 4) (alpha dropped), weight (M,), count
    (M,), normals (M, 3), labels and planes (M,) integers. Without normals, labels and planes the file is the one the four-argument call
    writes. Returns the path."""
    positions = np.asarray(_host(positions), dtype=np.float32).reshape(-1, 3)
    colors = _rgb_rows(colors, len(positions))
    fields = list(_PLY_VERTEX)
    extra = {}
    if normals is not None:
        normals = np.asarray(_host(normals), dtype=np.float32)
        if normals.shape != positions.shape:
            raise ValueError(f'write_ply: {len(positions)} positions, normals of shape {normals.shape}')
        fields[3:3] = _PLY_NORMAL
        extra.update(nx=normals[:, 0], ny=normals[:, 1], nz=normals[:, 2])
    for name, arr in (('confidence', weight), ('count', count), ('label', labels), ('plane', planes)):
        if arr is not None:
            extra[name] = np.asarray(_host(arr)).reshape(-1)
            if name in ('label', 'plane') and extra[name].dtype.kind not in 'iu':
                raise ValueError(f'write_ply: {name}s are integers, got {extra[name].dtype}')
            if len(extra[name]) != len(positions):
                raise ValueError(f'write_ply: {len(positions)} positions, {len(extra[name])} values of {name}')
            fields.append((name, _PLY_OPTIONAL[name]))
    rows = np.empty(len(positions), dtype=np.dtype(fields))
    rows['x'], rows['y'], rows['z'] = positions[:, 0], positions[:, 1], positions[:, 2]
    rows['red'], rows['green'], rows['blue'] = colors[:, 0], colors[:, 1], colors[:, 2]
    for name, arr in extra.items():
        rows[name] = arr
    header = ['ply', 'format binary_little_endian 1.0', 'comment dust3r_amd fused cloud', f'element vertex {len(rows)}']
    header += [f'property {_PLY_TYPES[t]} {name}' for name, t in fields] + ['end_header']
    with open(path, 'wb') as f:
        f.write(('\n'.join(header) + '\n').encode('ascii'))
        f.write(memoryview(rows).cast('B'))
    return path


def read_ply(path):
    """Reads the dialect `write_ply` writes (binary little-endian, one vertex element, the properties above in that order): a dict of
    positions (M, 3) float32, colors (M, 3) uint8 and, when present, normals (M, 3) float32, confidence (M,) float32, count (M,) int32, label (M,) int32 and plane (M,) int32."""
    with open(path, 'rb') as f:
        raw = f.read()
    end = raw.find(b'end_header\n')
    if not raw.startswith(b'ply\n') or end < 0:
        raise ValueError(f'{path}: not a PLY file')
    lines = raw[:end].decode('ascii').split('\n')
    if 'format binary_little_endian 1.0' not in lines:
        raise ValueError(f'{path}: only binary little-endian PLY is read')
    elements = [ln.split() for ln in lines if ln.startswith('element ')]
    if len(elements) != 1 or elements[0][1] != 'vertex':
        raise ValueError(f'{path}: one vertex element expected, got {elements}')
    n = int(elements[0][2])
    props = [tuple(ln.split()[1:]) for ln in lines if ln.startswith('property ')]
    names = {v: k for k, v in _PLY_TYPES.items()}
    fields = [(name, names[t]) for t, name in props]
    want = list(_PLY_VERTEX) + [(k, v) for k, v in _PLY_OPTIONAL.items() if k in dict(fields)]
    if 'nx' in dict(fields):
        want[3:3] = _PLY_NORMAL
    if fields != want:
        raise ValueError(f'{path}: vertex properties {props} are not the ones write_ply writes')
    dtype = np.dtype(fields)
    body = raw[end + len(b'end_header\n'):]
    if len(body) != n * dtype.itemsize:
        raise ValueError(f'{path}: {len(body)} bytes of data for {n} vertices of {dtype.itemsize} bytes')
    rows = np.frombuffer(body, dtype=dtype)
    out = dict(positions=np.stack([rows['x'], rows['y'], rows['z']], axis=1) if n else np.zeros((0, 3), np.float32),
               colors=np.stack([rows['red'], rows['green'], rows['blue']], axis=1) if n else np.zeros((0, 3), np.uint8))
    if 'nx' in rows.dtype.names:
        out['normals'] = np.stack([rows['nx'], rows['ny'], rows['nz']], axis=1) if n else np.zeros((0, 3), np.float32)
    for name in _PLY_OPTIONAL:
        if name in rows.dtype.names:
            out[name] = rows[name].copy()
    return out


# ---- COLMAP ---------------------------------------------------------------------------------------------------------------------------
def rotmat_to_quat(R):
    """Unit quaternion (qw, qx, qy, qz), qw >= 0, of a 3 x 3 rotation matrix, fp64: the largest of the four candidates as the pivot."""
    R = np.asarray(R, dtype=np.float64)
    t = [R[0, 0] + R[1, 1] + R[2, 2], R[0, 0] - R[1, 1] - R[2, 2], R[1, 1] - R[0, 0] - R[2, 2], R[2, 2] - R[0, 0] - R[1, 1]]
    k = int(np.argmax(t))
    if k == 0:
        q = [1 + t[0], R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]]
    elif k == 1:
        q = [R[2, 1] - R[1, 2], 1 + t[1], R[0, 1] + R[1, 0], R[0, 2] + R[2, 0]]
    elif k == 2:
        q = [R[0, 2] - R[2, 0], R[0, 1] + R[1, 0], 1 + t[2], R[1, 2] + R[2, 1]]
    else:
        q = [R[1, 0] - R[0, 1], R[0, 2] + R[2, 0], R[1, 2] + R[2, 1], 1 + t[3]]
    q = np.array(q)
    q = q / np.linalg.norm(q)
    return -q if q[0] < 0 else q


def quat_to_rotmat(q):
    w, x, y, z = np.asarray(q, dtype=np.float64)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def colmap_pose(cam2world):
    """(q, t) of one (4, 4) cam2world matrix as the COLMAP model holds the pose: the world-to-camera rotation of the fp64 inverse as a unit
    quaternion with qw >= 0, and t = -R(q) c with c the camera centre. R(q) = `quat_to_rotmat(q)` and t are the world-to-camera rows the
    2-D tracks project with (viz.track_cameras), so the tracks belong to the poses in the file."""
    cam2world = np.asarray(cam2world, dtype=np.float64)
    q = rotmat_to_quat(np.linalg.inv(cam2world)[:3, :3])
    return q, -quat_to_rotmat(q) @ cam2world[:3, 3]


def colmap_cameras(scene, names=None):
    """Per image of the scene what COLMAP keeps: dict(id, name, width, height, params (fx, fy, cx, cy), q (qw, qx, qy, qz), t): one PINHOLE
    camera per image from `get_intrinsics()` and `imshapes` (the images the network saw), the world-to-camera pose from the inverse of
    `get_im_poses()` in fp64 -- a unit quaternion with qw >= 0, and t = -R(q) c with c the camera centre, so that (q, t) is consistent."""
    K = np.asarray(_host(scene.get_intrinsics()), dtype=np.float64)
    c2w = np.asarray(_host(scene.get_im_poses()), dtype=np.float64)
    shapes = [(int(h), int(w)) for h, w in scene.imshapes]
    if names is None:
        names = [f'{i:06d}.png' for i in range(len(shapes))]
    if not (len(K) == len(c2w) == len(shapes) == len(names)):
        raise ValueError(f'write_colmap: {len(K)} intrinsics, {len(c2w)} poses, {len(shapes)} images, {len(names)} names')
    cams = []
    for i, ((h, w), name) in enumerate(zip(shapes, names)):
        q, t = colmap_pose(c2w[i])
        cams.append(dict(id=i + 1, name=str(name), width=w, height=h, params=(K[i, 0, 0], K[i, 1, 1], K[i, 0, 2], K[i, 1, 2]), q=q, t=t))
    return cams


_POINT_ROW = np.dtype([('id', '<u8'), ('xyz', '<f8', (3,)), ('rgb', 'u1', (3,)), ('error', '<f8'), ('track', '<u8')])      # 51 bytes, then the track
_POINT2D_ROW = np.dtype([('x', '<f8'), ('y', '<f8'), ('id', '<i8')])
_TRACK_ROW = np.dtype([('image', '<i4'), ('idx', '<i4')])
_POINT_CHUNK = 1 << 18          # points per block of points3D.bin with tracks: bounds the index arrays of the byte scatter


def _track_arrays(tracks, n_points, n_images):
    """the host arrays the writers need of a `viz.CloudTracks`; ValueError when it does not belong to this cloud and scene"""
    off = np.asarray(_host(tracks.point_offsets), dtype=np.int64)
    image_off = np.asarray(_host(tracks.image_offsets), dtype=np.int64)
    if len(off) != n_points + 1 or len(image_off) != n_images + 1:
        raise ValueError(f'write_colmap: tracks of {len(off) - 1} points in {len(image_off) - 1} images, the model has {n_points} and {n_images}')
    return dict(off=off, image_off=image_off, image_obs=np.asarray(_host(tracks.image_obs), dtype=np.int64), view=np.asarray(_host(tracks.view), dtype=np.int64),
                point2d=np.asarray(_host(tracks.point2d), dtype=np.int64), xy=np.asarray(_host(tracks.xy()), dtype=np.float64).reshape(-1, 2),
                error=np.asarray(_host(tracks.point_error()), dtype=np.float64), point=np.repeat(np.arange(n_points, dtype=np.int64), np.diff(off)))


def _write_points_bin_with_tracks(f, xyz, rgb, tr):
    """points3D.bin with tracks: rows of 51 bytes, each followed by its track of (image_id, point2d_idx) int32 pairs; written in blocks
    of _POINT_CHUNK points, each block one byte buffer filled by two index scatters"""
    off = tr['off']
    f.write(struct.pack('<Q', len(xyz)))
    for a in range(0, len(xyz), _POINT_CHUNK):
        b = min(a + _POINT_CHUNK, len(xyz))
        rows = np.zeros(b - a, dtype=_POINT_ROW)
        rows['id'] = np.arange(a + 1, b + 1, dtype=np.uint64)
        rows['xyz'], rows['rgb'], rows['error'], rows['track'] = xyz[a:b], rgb[a:b], tr['error'][a:b], off[a + 1:b + 1] - off[a:b]
        k0, k1 = off[a], off[b]
        pairs = np.empty(k1 - k0, dtype=_TRACK_ROW)
        pairs['image'], pairs['idx'] = tr['view'][k0:k1] + 1, tr['point2d'][k0:k1]
        buf = np.empty(_POINT_ROW.itemsize * (b - a) + _TRACK_ROW.itemsize * (k1 - k0), dtype=np.uint8)
        starts = _POINT_ROW.itemsize * np.arange(b - a, dtype=np.int64) + _TRACK_ROW.itemsize * (off[a:b] - k0)
        buf[(starts[:, None] + np.arange(_POINT_ROW.itemsize)).reshape(-1)] = rows.view(np.uint8)
        where = _POINT_ROW.itemsize * (tr['point'][k0:k1] - a + 1) + _TRACK_ROW.itemsize * np.arange(k1 - k0, dtype=np.int64)
        buf[(where[:, None] + np.arange(_TRACK_ROW.itemsize)).reshape(-1)] = pairs.view(np.uint8)
        f.write(memoryview(buf))


def write_colmap(outdir, scene, cloud, names=None, binary=True, write_images=True):
    """A COLMAP model of an aligned scene and its fused cloud: outdir/sparse/0/{cameras,images,points3D}.{bin|txt} and, with write_images,
    outdir/images/<name> (PNG of np.uint8(255 * scene.imgs[i])). Cameras and poses: `colmap_cameras`; the points are the cloud's, ids
    1 ... M. Without tracks (cloud.tracks is None) no image has 2-D points and every point has error 0 and an empty track. With tracks
    (`FusedCloud.build_tracks`) image v's POINTS2D are its observations (x, y, point3D_id) in ascending point id -- (x, y) the observing
    pixel as integers, in the convention of the camera parameters written (no half-pixel shift on either side) --, every point carries its
    track (image_id, point2d_idx) in ascending image id and, as its error, the mean distance in pixels between its projections and those
    pixels; a point without an observation gets error -1 and an empty track; the text headers' means are filled in. names: the image
    file names, default f'{i:06d}.png'. Returns the list of files."""
    cams = colmap_cameras(scene, names)
    xyz = np.asarray(_host(cloud.positions), dtype=np.float64).reshape(-1, 3)
    rgb = _rgb_rows(cloud.colors, len(xyz))
    tracks = getattr(cloud, 'tracks', None)
    tr = None if tracks is None else _track_arrays(tracks, len(xyz), len(cams))
    if write_images and getattr(scene, 'imgs', None) is None:
        raise ValueError('write_colmap needs the scene images: scene.imgs is None (write_images=False writes the model alone)')
    sparse = os.path.join(outdir, 'sparse', '0')
    os.makedirs(sparse, exist_ok=True)
    ext = 'bin' if binary else 'txt'
    files = [os.path.join(sparse, f'{stem}.{ext}') for stem in ('cameras', 'images', 'points3D')]
    if binary:
        with open(files[0], 'wb') as f:
            f.write(struct.pack('<Q', len(cams)))
            for c in cams:
                f.write(struct.pack('<iiQQ4d', c['id'], CAMERA_MODEL_PINHOLE, c['width'], c['height'], *c['params']))
        with open(files[1], 'wb') as f:
            f.write(struct.pack('<Q', len(cams)))
            for v, c in enumerate(cams):
                obs = tr['image_obs'][tr['image_off'][v]:tr['image_off'][v + 1]] if tr else ()
                f.write(struct.pack('<i4d3di', c['id'], *c['q'], *c['t'], c['id']) + c['name'].encode('utf-8') + b'\0' + struct.pack('<Q', len(obs)))
                if len(obs):
                    p2d = np.empty(len(obs), dtype=_POINT2D_ROW)
                    p2d['x'], p2d['y'], p2d['id'] = tr['xy'][obs, 0], tr['xy'][obs, 1], tr['point'][obs] + 1
                    f.write(memoryview(p2d).cast('B'))
        with open(files[2], 'wb') as f:
            if tr:
                _write_points_bin_with_tracks(f, xyz, rgb, tr)
            else:
                rows = np.zeros(len(xyz), dtype=_POINT_ROW)
                rows['id'] = np.arange(1, len(xyz) + 1, dtype=np.uint64)
                rows['xyz'], rows['rgb'] = xyz, rgb
                f.write(struct.pack('<Q', len(rows)))
                f.write(memoryview(rows).cast('B'))
    else:
        n_obs = len(tr['view']) if tr else 0
        with open(files[0], 'w') as f:
            f.write('# Camera list with one line of data per camera:\n#   CAMERA_ID, MODEL, WIDTH, HEIGHT, PARAMS[]\n'
                    f'# Number of cameras: {len(cams)}\n')
            for c in cams:
                f.write(f"{c['id']} PINHOLE {c['width']} {c['height']} " + ' '.join(repr(float(v)) for v in c['params']) + '\n')
        with open(files[1], 'w') as f:
            f.write('# Image list with two lines of data per image:\n#   IMAGE_ID, QW, QX, QY, QZ, TX, TY, TZ, CAMERA_ID, NAME\n'
                    f'#   POINTS2D[] as (X, Y, POINT3D_ID)\n# Number of images: {len(cams)}, mean observations per image: '
                    f'{repr(n_obs / max(len(cams), 1)) if tr else 0}\n')
            for k, c in enumerate(cams):
                points2d = ''
                if tr:
                    obs = tr['image_obs'][tr['image_off'][k]:tr['image_off'][k + 1]]
                    points2d = ' '.join(f'{x!r} {y!r} {p + 1}' for (x, y), p in zip(tr['xy'][obs].tolist(), tr['point'][obs].tolist()))
                f.write(f"{c['id']} " + ' '.join(repr(float(v)) for v in (*c['q'], *c['t'])) + f" {c['id']} {c['name']}\n{points2d}\n")
        with open(files[2], 'w') as f:
            f.write('# 3D point list with one line of data per point:\n#   POINT3D_ID, X, Y, Z, R, G, B, ERROR, TRACK[] as (IMAGE_ID, POINT2D_IDX)\n'
                    f'# Number of points: {len(xyz)}, mean track length: {repr(n_obs / max(len(xyz), 1)) if tr else 0}\n')
            if tr:
                off, image, idx = tr['off'].tolist(), (tr['view'] + 1).tolist(), tr['point2d'].tolist()
                for i, (p, c, e) in enumerate(zip(xyz, rgb, tr['error'].tolist())):
                    track = ''.join(f' {image[k]} {idx[k]}' for k in range(off[i], off[i + 1]))
                    f.write(f'{i + 1} {float(p[0])!r} {float(p[1])!r} {float(p[2])!r} {c[0]} {c[1]} {c[2]} {e!r}{track}\n')
            else:
                f.write(''.join(f'{i + 1} {float(p[0])!r} {float(p[1])!r} {float(p[2])!r} {c[0]} {c[1]} {c[2]} 0\n' for i, (p, c) in enumerate(zip(xyz, rgb))))
    if write_images:
        import PIL.Image
        os.makedirs(os.path.join(outdir, 'images'), exist_ok=True)
        for c, img in zip(cams, scene.imgs):
            img = _host(img)
            if img.dtype != np.uint8:
                img = np.uint8(255 * img)                 # as the GLB export's textures
            name = os.path.join(outdir, 'images', c['name'])
            PIL.Image.fromarray(img).save(name)
            files.append(name)
    return files


_MODEL_NAMES = {CAMERA_MODEL_PINHOLE: 'PINHOLE'}


def read_colmap(sparse_dir):
    """(cameras, images, points) of the COLMAP model in sparse_dir, binary when cameras.bin is there, else text; what `write_colmap`
    writes, PINHOLE cameras only. cameras: dicts of id, model (the id, 1), width, height, params (fx, fy, cx, cy). images: dicts of id, q
    (qw, qx, qy, qz), t, camera_id, name, xys (n2d, 2) float64 and point3D_ids (n2d,) int64. points: dicts of id, xyz, rgb, error and
    track (L, 2) int32 rows (image_id, point2d_idx). A reader for tests and small tools: one Python object per point."""
    cams, imgs, pts = [], [], []
    if os.path.exists(os.path.join(sparse_dir, 'cameras.bin')):
        raw = open(os.path.join(sparse_dir, 'cameras.bin'), 'rb').read()
        (n,), o = struct.unpack_from('<Q', raw), 8
        for _ in range(n):
            cid, model, w, h = struct.unpack_from('<iiQQ', raw, o)
            if model not in _MODEL_NAMES:
                raise ValueError(f'{sparse_dir}: camera model {model} is not read (PINHOLE only)')
            cams.append(dict(id=cid, model=model, width=w, height=h, params=struct.unpack_from('<4d', raw, o + 24)))
            o += 56
        if o != len(raw):
            raise ValueError(f'{sparse_dir}/cameras.bin: {len(raw) - o} bytes left over')
        raw = open(os.path.join(sparse_dir, 'images.bin'), 'rb').read()
        (n,), o = struct.unpack_from('<Q', raw), 8
        for _ in range(n):
            f = struct.unpack_from('<i4d3di', raw, o)
            end = raw.index(b'\0', o + 64)
            (n2d,) = struct.unpack_from('<Q', raw, end + 1)
            p2d = np.frombuffer(raw, dtype=_POINT2D_ROW, count=n2d, offset=end + 9)
            imgs.append(dict(id=f[0], q=list(f[1:5]), t=list(f[5:8]), camera_id=f[8], name=raw[o + 64:end].decode('utf-8'),
                             xys=np.stack([p2d['x'], p2d['y']], axis=1) if n2d else np.zeros((0, 2)), point3D_ids=p2d['id'].astype(np.int64)))
            o = end + 9 + _POINT2D_ROW.itemsize * n2d
        if o != len(raw):
            raise ValueError(f'{sparse_dir}/images.bin: {len(raw) - o} bytes left over')
        raw = open(os.path.join(sparse_dir, 'points3D.bin'), 'rb').read()
        (n,), o = struct.unpack_from('<Q', raw), 8
        for _ in range(n):
            pid, x, y, z, r, g, b, err, length = struct.unpack_from('<Q3d3BdQ', raw, o)
            track = np.frombuffer(raw, dtype='<i4', count=2 * length, offset=o + _POINT_ROW.itemsize).reshape(length, 2)
            pts.append(dict(id=pid, xyz=(x, y, z), rgb=(r, g, b), error=err, track=track))
            o += _POINT_ROW.itemsize + _TRACK_ROW.itemsize * length
        if o != len(raw):
            raise ValueError(f'{sparse_dir}/points3D.bin: {len(raw) - o} bytes left over')
        return cams, imgs, pts
    ids = {name: k for k, name in _MODEL_NAMES.items()}

    def data_lines(stem):
        lines = open(os.path.join(sparse_dir, stem + '.txt')).read().split('\n')
        if lines and lines[-1] == '':
            lines.pop()
        return [ln for ln in lines if not ln.startswith('#')]
    for ln in data_lines('cameras'):
        f = ln.split()
        if f[1] not in ids:
            raise ValueError(f'{sparse_dir}: camera model {f[1]} is not read (PINHOLE only)')
        cams.append(dict(id=int(f[0]), model=ids[f[1]], width=int(f[2]), height=int(f[3]), params=tuple(float(v) for v in f[4:8])))
    body = data_lines('images')
    if len(body) % 2:
        raise ValueError(f'{sparse_dir}/images.txt: two lines per image expected')
    for first, second in zip(body[::2], body[1::2]):
        f, p = first.split(), second.split()
        if len(p) % 3:
            raise ValueError(f'{sparse_dir}/images.txt: POINTS2D of image {f[0]} are not triples')
        imgs.append(dict(id=int(f[0]), q=[float(v) for v in f[1:5]], t=[float(v) for v in f[5:8]], camera_id=int(f[8]), name=f[9],
                         xys=np.array([float(v) for v in p], dtype=np.float64).reshape(-1, 3)[:, :2], point3D_ids=np.array([int(v) for v in p[2::3]], dtype=np.int64)))
    for ln in data_lines('points3D'):
        f = ln.split()
        if len(f) < 8 or len(f) % 2:
            raise ValueError(f'{sparse_dir}/points3D.txt: bad line of point {f[0] if f else "?"}')
        pts.append(dict(id=int(f[0]), xyz=tuple(float(v) for v in f[1:4]), rgb=tuple(int(v) for v in f[4:7]), error=float(f[7]),
                        track=np.array([int(v) for v in f[8:]], dtype=np.int32).reshape(-1, 2)))
    return cams, imgs, pts
