"""File formats other tools read, for the fused cloud of `scene.fuse()` (viz.FusedCloud): binary PLY, and a COLMAP model (sparse/0 +
images/, the layout Gaussian-splatting trainers take). Host only: struct and numpy; bulk bytes go out through memoryview, as in glb.py.

Out of scope: meshing, TSDF fusion, normals in the COLMAP model, 2-D tracks in the COLMAP model (every image has no 2-D points, every point an empty track),
ASCII PLY."""
import os
import struct

import numpy as np

_PLY_VERTEX = [('x', '<f4'), ('y', '<f4'), ('z', '<f4'), ('red', 'u1'), ('green', 'u1'), ('blue', 'u1')]
_PLY_TYPES = {'<f4': 'float', 'u1': 'uchar', '<i4': 'int'}
_PLY_NORMAL = [('nx', '<f4'), ('ny', '<f4'), ('nz', '<f4')]       # directly after z, where MeshLab, Open3D and Poisson reconstruction expect them
_PLY_OPTIONAL = {'confidence': '<f4', 'count': '<i4'}

CAMERA_MODEL_PINHOLE = 1        # COLMAP's model id of PINHOLE (fx, fy, cx, cy)


def _host(x):
    """numpy array of a numpy array or a (device) tensor"""
    return x.detach().cpu().numpy() if hasattr(x, 'detach') else np.asarray(x)


def _rgb_rows(colors, n):
    """(n, 3) uint8 of (n, 3) or (n, 4) colours (alpha dropped)"""
    colors = np.asarray(_host(colors), dtype=np.uint8)
    return colors.reshape(n, colors.shape[-1] if colors.ndim > 1 else 3)[:, :3]


# ---- PLY ------------------------------------------------------------------------------------------------------------------------------
def write_ply(path, positions, colors, weight=None, count=None, normals=None):
    """Binary little-endian PLY: per vertex `float x y z`, `float nx ny nz` when normals are given, `uchar red green blue`, then
    `float confidence` (weight) and `int count` when given. positions (M, 3), colors (M, 3) or (M, 4) (alpha dropped), weight (M,),
    count (M,), normals (M, 3). Without normals the file is the one the four-argument call writes. Returns the path."""
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
    for name, arr in (('confidence', weight), ('count', count)):
        if arr is not None:
            extra[name] = np.asarray(_host(arr)).reshape(-1)
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
    positions (M, 3) float32, colors (M, 3) uint8 and, when present, normals (M, 3) float32, confidence (M,) float32 and count (M,) int32."""
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
        q = rotmat_to_quat(np.linalg.inv(c2w[i])[:3, :3])
        cams.append(dict(id=i + 1, name=str(name), width=w, height=h, params=(K[i, 0, 0], K[i, 1, 1], K[i, 0, 2], K[i, 1, 2]), q=q,
                         t=-quat_to_rotmat(q) @ c2w[i, :3, 3]))
    return cams


def write_colmap(outdir, scene, cloud, names=None, binary=True, write_images=True):
    """A COLMAP model of an aligned scene and its fused cloud: outdir/sparse/0/{cameras,images,points3D}.{bin|txt} and, with write_images,
    outdir/images/<name> (PNG of np.uint8(255 * scene.imgs[i])). Cameras and poses: `colmap_cameras`; no image has 2-D points; the points
    are the cloud's, ids 1 ... M, error 0, empty tracks. names: the image file names, default f'{i:06d}.png'. Returns the list of files."""
    cams = colmap_cameras(scene, names)
    xyz = np.asarray(_host(cloud.positions), dtype=np.float64).reshape(-1, 3)
    rgb = _rgb_rows(cloud.colors, len(xyz))
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
            for c in cams:
                f.write(struct.pack('<i4d3di', c['id'], *c['q'], *c['t'], c['id']) + c['name'].encode('utf-8') + b'\0' + struct.pack('<Q', 0))
        rows = np.zeros(len(xyz), dtype=np.dtype([('id', '<u8'), ('xyz', '<f8', (3,)), ('rgb', 'u1', (3,)), ('error', '<f8'), ('track', '<u8')]))
        rows['id'] = np.arange(1, len(xyz) + 1, dtype=np.uint64)
        rows['xyz'], rows['rgb'] = xyz, rgb
        with open(files[2], 'wb') as f:
            f.write(struct.pack('<Q', len(rows)))
            f.write(memoryview(rows).cast('B'))
    else:
        with open(files[0], 'w') as f:
            f.write('# Camera list with one line of data per camera:\n#   CAMERA_ID, MODEL, WIDTH, HEIGHT, PARAMS[]\n'
                    f'# Number of cameras: {len(cams)}\n')
            for c in cams:
                f.write(f"{c['id']} PINHOLE {c['width']} {c['height']} " + ' '.join(repr(float(v)) for v in c['params']) + '\n')
        with open(files[1], 'w') as f:
            f.write('# Image list with two lines of data per image:\n#   IMAGE_ID, QW, QX, QY, QZ, TX, TY, TZ, CAMERA_ID, NAME\n'
                    f'#   POINTS2D[] as (X, Y, POINT3D_ID)\n# Number of images: {len(cams)}, mean observations per image: 0\n')
            for c in cams:
                f.write(f"{c['id']} " + ' '.join(repr(float(v)) for v in (*c['q'], *c['t'])) + f" {c['id']} {c['name']}\n\n")
        with open(files[2], 'w') as f:
            f.write('# 3D point list with one line of data per point:\n#   POINT3D_ID, X, Y, Z, R, G, B, ERROR, TRACK[] as (IMAGE_ID, POINT2D_IDX)\n'
                    f'# Number of points: {len(xyz)}, mean track length: 0\n')
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
