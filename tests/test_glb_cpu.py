"""The demo's GLB export (dust3r_amd/demo.py, viz.scene_mesh_batch / scene_camera_geometry, glb.py) without a GPU: the numpy restatement of the
reference's mesh (pts3d_to_trimesh + cat_meshes, dust3r/viz.py:38-87) and of the vertex-colour definition, pinned to what the reference's own
code recorded (tests/golden/glb_reference.pt, tools/make_glb_golden.py); the public signatures and constants; the writer, read back by the
small GLB reader below; the size guard; the camera glyphs. tests/test_glb_gpu.py holds the kernels to the same restatement."""
import inspect
import json
import os
import struct

import numpy as np
import pytest
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'glb_reference.pt')


def _golden():
    return torch.load(GOLDEN, weights_only=False)


# ---- restatement --------------------------------------------------------------------------------------------------------------------
def restated_q(img):
    """colour of every pixel as uint8: the byte itself, or floor(255 c + 1/2) clamped to [0, 255] in fp32"""
    img = np.asarray(img)
    if img.dtype == np.uint8:
        return img
    q = np.floor(np.float32(255) * img.astype(np.float32) + np.float32(0.5))
    return np.clip(q, 0, 255).astype(np.uint8)


def restated_faces(shapes, masks):
    """faces of cat_meshes([pts3d_to_trimesh(...) ...]) and, per face, the flat index (over all views) of the pixel that gives its colour"""
    faces, src, off = [], [], 0
    for (H, W), m in zip(shapes, masks):
        idx = np.arange(H * W).reshape(H, W)
        i1, i2, i3, i4 = idx[:-1, :-1].ravel(), idx[:-1, 1:].ravel(), idx[1:, :-1].ravel(), idx[1:, 1:].ravel()
        valid = np.asarray(m).reshape(-1).astype(bool)
        up, lo = valid[i1] & valid[i2] & valid[i3], valid[i2] & valid[i3] & valid[i4]
        fu, fl = np.c_[i1, i2, i3][up] + off, np.c_[i2, i3, i4][lo] + off
        faces += [fu, fu[:, ::-1], fl, fl[:, ::-1]]
        src += [i1[up] + off, i1[up] + off, i4[lo] + off, i4[lo] + off]
        off += H * W
    return np.concatenate(faces).astype(np.int64).reshape(-1, 3), np.concatenate(src).astype(np.int64)


def vertex_colors(n_vert, faces, face_q, own_q):
    """the definition: per vertex, the per-channel integer mean (sum + n // 2) // n of the colours of the faces that use it (reversed copies
    included), its own colour when no face does; alpha 255"""
    s = np.zeros((n_vert, 3), np.int64)
    n = np.zeros(n_vert, np.int64)
    for k in range(3):
        np.add.at(s, faces[:, k], face_q.astype(np.int64))
        np.add.at(n, faces[:, k], 1)
    out = np.empty((n_vert, 4), np.uint8)
    used = n > 0
    out[used, :3] = (s[used] + n[used, None] // 2) // n[used, None]
    out[~used, :3] = own_q[~used]
    out[:, 3] = 255
    return out


def restated_mesh(imgs, pts, masks):
    shapes = [np.asarray(im).shape[:2] for im in imgs]
    faces, src = restated_faces(shapes, masks)
    q = np.concatenate([restated_q(im).reshape(-1, 3) for im in imgs])
    positions = np.concatenate([np.asarray(p, np.float32).reshape(-1, 3) for p in pts])
    colors = vertex_colors(len(q), faces, q[src], q)
    used = np.unique(faces)
    bounds = (positions[used].min(0), positions[used].max(0)) if len(used) else None
    return dict(faces=faces, colors=colors, positions=positions, bounds=bounds)


def restated_pointcloud(imgs, pts, masks):
    m = [np.asarray(k).reshape(-1).astype(bool) for k in masks]
    positions = np.concatenate([np.asarray(p, np.float32).reshape(-1, 3)[k] for p, k in zip(pts, m)])
    q = np.concatenate([restated_q(im).reshape(-1, 3)[k] for im, k in zip(imgs, m)])
    colors = np.concatenate([q, np.full((len(q), 1), 255, np.uint8)], axis=1)
    bounds = (positions.min(0), positions.max(0)) if len(positions) else None
    return dict(positions=positions, colors=colors, bounds=bounds)


# ---- reader -------------------------------------------------------------------------------------------------------------------------
_NP = {5126: np.float32, 5125: np.uint32, 5121: np.uint8}
_WIDTH = {'SCALAR': 1, 'VEC2': 2, 'VEC3': 3, 'VEC4': 4}


def read_glb(path):
    """Parses a .glb and checks its framing: magic, version, total length, one JSON and one BIN chunk, 4-byte alignment of the chunks and
    of every bufferView, accessors inside their views. Returns (json document, accessor reader, bufferView reader)."""
    raw = open(path, 'rb').read()
    magic, version, total = struct.unpack_from('<III', raw, 0)
    assert magic == 0x46546C67 and version == 2 and total == len(raw)
    jlen, jtype = struct.unpack_from('<II', raw, 12)
    assert jtype == 0x4E4F534A and jlen % 4 == 0
    doc = json.loads(raw[20:20 + jlen].decode())
    assert doc['asset']['version'] == '2.0'
    pos = 20 + jlen
    bin_ = b''
    if pos < len(raw):
        blen, btype = struct.unpack_from('<II', raw, pos)
        assert btype == 0x004E4942 and blen % 4 == 0 and pos + 8 + blen == len(raw)
        bin_ = raw[pos + 8:]
        assert doc['buffers'] == [dict(byteLength=blen)]
    else:
        assert 'buffers' not in doc
    for v in doc.get('bufferViews', []):
        assert v['byteOffset'] % 4 == 0 and v['byteOffset'] + v['byteLength'] <= len(bin_)

    def view(i):
        v = doc['bufferViews'][i]
        return bin_[v['byteOffset']:v['byteOffset'] + v['byteLength']]

    def accessor(i):
        a = doc['accessors'][i]
        assert a['count'] > 0
        width = _WIDTH[a['type']]
        data = np.frombuffer(view(a['bufferView']), dtype=_NP[a['componentType']])
        assert data.size == a['count'] * width
        return data.reshape(a['count'], width) if width > 1 else data
    return doc, accessor, view


def root_matrix(doc):
    """node 0's matrix (column-major) as a row-major 4 x 4"""
    return np.array(doc['nodes'][0]['matrix'], dtype=np.float64).reshape(4, 4).T


# ---- tests --------------------------------------------------------------------------------------------------------------------------
def test_restated_faces_and_colours_equal_the_reference():
    g = _golden()
    assert len(g['cases']) >= 4
    for case in g['cases']:
        imgs = [im.numpy() for im in case['imgs']]
        masks = [m.numpy() for m in case['masks']]
        faces, src = restated_faces([im.shape[:2] for im in imgs], masks)
        assert np.array_equal(faces, case['faces'].numpy().astype(np.int64))
        flat = np.concatenate([im.reshape(-1, 3) for im in imgs])
        assert np.array_equal(flat[src], case['face_colors'].numpy())        # the reference's face colours, bit for bit


def test_vertex_colour_definition_on_the_reference_faces():
    """The restated vertex colours (built on the restated faces) equal the definition evaluated on the reference's own faces and face colours."""
    for case in _golden()['cases']:
        imgs = [im.numpy() for im in case['imgs']]
        pts = [np.zeros(im.shape, np.float32) for im in imgs]
        mine = restated_mesh(imgs, pts, [m.numpy() for m in case['masks']])
        own = np.concatenate([restated_q(im).reshape(-1, 3) for im in imgs])
        ref = vertex_colors(len(own), case['faces'].numpy().astype(np.int64), restated_q(case['face_colors'].numpy()), own)
        assert np.array_equal(mine['colors'], ref)
        # counting every face twice leaves the means unchanged (the reason the reversed copies do not matter)
        fq = restated_q(case['face_colors'].numpy())
        f = case['faces'].numpy().astype(np.int64)
        assert np.array_equal(vertex_colors(len(own), np.concatenate([f, f]), np.concatenate([fq, fq]), own), ref)


def test_vertex_colour_rounding():
    """two faces, colours 0 and 1 -> (1 + 1) // 2 = 1; three faces 0, 0, 2 -> (2 + 1) // 3 = 1; a vertex no face uses keeps its own q"""
    faces = np.array([[0, 1, 2], [0, 3, 4], [5, 6, 0]])
    q = np.array([[0, 0, 0], [1, 2, 255], [2, 4, 255]], np.uint8)
    own = np.arange(8 * 3, dtype=np.uint8).reshape(8, 3)
    col = vertex_colors(8, faces, q, own)
    assert col[0].tolist() == [(0 + 1 + 2 + 1) // 3, (0 + 2 + 4 + 1) // 3, (0 + 255 + 255 + 1) // 3, 255]
    assert col[7].tolist() == own[7].tolist() + [255]
    assert restated_q(np.float32([[[0.5 / 255, 1.5 / 255, 2.0]]])).tolist() == [[[1, 2, 255]]]


def test_signatures_and_constants_equal_the_reference():
    from dust3r_amd import demo, viz
    g = _golden()
    for name, sig in g['signatures'].items():
        assert str(inspect.signature(getattr(demo, name))) == sig
    assert np.array_equal(viz.OPENGL, g['OPENGL'].numpy()) and viz.OPENGL.dtype == g['OPENGL'].numpy().dtype
    assert [tuple(c) for c in viz.CAM_COLORS] == [tuple(c) for c in g['CAM_COLORS']]


def _hand_made(as_pointcloud, rng):
    imgs = [rng.random((4, 6, 3)).astype(np.float32), rng.random((5, 3, 3)).astype(np.float32)]
    pts = [rng.normal(size=im.shape).astype(np.float32) for im in imgs]
    masks = [rng.random(im.shape[:2]) < 0.8 for im in imgs]
    if as_pointcloud:
        r = restated_pointcloud(imgs, pts, masks)
        geo = dict(positions=r['positions'], colors=r['colors'], faces=None, bounds=r['bounds'])
    else:
        r = restated_mesh(imgs, pts, masks)
        geo = dict(positions=r['positions'], colors=r['colors'], faces=r['faces'].astype(np.uint32), bounds=r['bounds'])
    poses = np.stack([np.eye(4), np.eye(4)])
    poses[1, :3, 3] = [0.3, -0.1, 0.2]
    return imgs, geo, poses, np.float32([[5.0], [4.0]])


@pytest.mark.parametrize('as_pointcloud', [False, True])
def test_writer_round_trip(tmp_path, as_pointcloud):
    from dust3r_amd.demo import _rot_y180, write_scene_glb
    from dust3r_amd.viz import OPENGL
    rng = np.random.default_rng(3)
    imgs, geo, poses, focals = _hand_made(as_pointcloud, rng)
    path = str(tmp_path / 'scene.glb')
    total = write_scene_glb(path, geo, imgs, focals, poses, cam_size=0.05, as_pointcloud=as_pointcloud)
    assert os.path.getsize(path) == total
    doc, acc, view = read_glb(path)
    assert np.allclose(root_matrix(doc), np.linalg.inv(poses[0] @ OPENGL @ _rot_y180()), atol=0, rtol=0)
    assert doc['scenes'][doc['scene']]['nodes'] == [0] and len(doc['nodes'][0]['children']) == len(doc['nodes']) - 1
    scene = [n for n in doc['nodes'] if n.get('name') == 'scene']
    assert len(scene) == 1
    prim = doc['meshes'][scene[0]['mesh']]['primitives'][0]
    pa = doc['accessors'][prim['attributes']['POSITION']]
    assert pa['componentType'] == 5126 and pa['type'] == 'VEC3' and pa['count'] == len(geo['positions'])
    assert np.array_equal(np.float32(pa['min']), geo['bounds'][0]) and np.array_equal(np.float32(pa['max']), geo['bounds'][1])
    assert acc(prim['attributes']['POSITION']).tobytes() == geo['positions'].tobytes()
    ca = doc['accessors'][prim['attributes']['COLOR_0']]
    assert ca['componentType'] == 5121 and ca['type'] == 'VEC4' and ca['normalized'] is True
    assert np.array_equal(acc(prim['attributes']['COLOR_0']), geo['colors'])
    if as_pointcloud:
        assert prim['mode'] == 0 and 'indices' not in prim
    else:
        ia = doc['accessors'][prim['indices']]
        assert prim['mode'] == 4 and ia['componentType'] == 5125 and ia['count'] == geo['faces'].size
        assert np.array_equal(acc(prim['indices']), geo['faces'].reshape(-1))
    # one wireframe and one textured picture per camera
    cams = [n for n in doc['nodes'] if n.get('name', '').startswith('camera_') and not n['name'].endswith('_image')]
    pics = [n for n in doc['nodes'] if n.get('name', '').endswith('_image')]
    assert len(cams) == 2 and len(pics) == 2 and len(doc['images']) == 2
    for i, node in enumerate(pics):
        import io
        import PIL.Image
        mat = doc['materials'][doc['meshes'][node['mesh']]['primitives'][0]['material']]
        img = doc['images'][doc['textures'][mat['pbrMetallicRoughness']['baseColorTexture']['index']]['source']]
        assert img['mimeType'] == 'image/png'
        assert np.array_equal(np.asarray(PIL.Image.open(io.BytesIO(view(img['bufferView'])))), np.uint8(255 * imgs[i]))


def test_writer_without_geometry_and_transparent_cams(tmp_path):
    from dust3r_amd.demo import write_scene_glb
    imgs, geo, poses, focals = _hand_made(False, np.random.default_rng(4))
    geo = dict(positions=geo['positions'], colors=geo['colors'], faces=np.zeros((0, 3), np.uint32), bounds=None)
    path = str(tmp_path / 'scene.glb')
    write_scene_glb(path, geo, imgs, focals, poses, transparent_cams=True, cam_color=[(1, 2, 3), (4, 5, 6)])
    doc, acc, _ = read_glb(path)
    assert [n['name'] for n in doc['nodes']] == ['world', 'camera_0', 'camera_1'] and 'images' not in doc
    for k, node in enumerate(doc['nodes'][1:]):
        col = acc(doc['meshes'][node['mesh']]['primitives'][0]['attributes']['COLOR_0'])
        assert np.array_equal(col, np.tile(np.uint8([1 + 3 * k, 2 + 3 * k, 3 + 3 * k, 255]), (len(col), 1)))
    for a in doc['accessors']:
        assert a['count'] > 0


def test_size_guard_raises_before_the_file_exists(tmp_path):
    from dust3r_amd.demo import write_scene_glb
    imgs, _, poses, focals = _hand_made(True, np.random.default_rng(5))
    n = 400_000_000                                     # 16 bytes per point: 6.4 GB, past the uint32 length (broadcast: no memory)
    geo = dict(positions=np.broadcast_to(np.float32([1, 2, 3]), (n, 3)), colors=np.broadcast_to(np.uint8([9, 9, 9, 255]), (n, 4)), faces=None,
               bounds=(np.float32([1, 2, 3]), np.float32([1, 2, 3])))
    path = str(tmp_path / 'scene.glb')
    with pytest.raises(ValueError, match=r'(?s)\d+ bytes.*as_pointcloud=True.*min_conf_thr'):
        write_scene_glb(path, geo, imgs, focals, poses, as_pointcloud=True)
    assert not os.path.exists(path)


# the frustum's 8 edges as index pairs into the wireframe's vertices: apex 5 to each base corner 1-4, and the base's sides
FRUSTUM_EDGES = {frozenset((5, c)) for c in (1, 2, 3, 4)} | {frozenset((c, c % 4 + 1)) for c in (1, 2, 3, 4)}


@pytest.mark.parametrize('focal,imsize', [(np.float32([300.0]), (512, 384)), (np.float32(250.0), (288, 512)), (0.0, (64, 48))])
def test_camera_glyph(focal, imsize):
    from scipy.spatial.transform import Rotation
    from dust3r_amd.viz import scene_camera_geometry
    rng = np.random.default_rng(11)
    pose = np.eye(4)
    pose[:3, :3] = Rotation.from_rotvec(rng.normal(size=3)).as_matrix()
    pose[:3, 3] = rng.normal(size=3)
    sw = 0.05
    cam = scene_camera_geometry(pose, focal, imsize, screen_width=sw)
    V, F = cam['wire_vertices'], cam['wire_faces']
    assert F.shape == (48, 3) and V.shape == (18, 3)
    edges = FRUSTUM_EDGES
    covered = set()
    for f in F:
        orig = [int(v) for v in f if 1 <= v <= 5]
        assert len(orig) == 2 and frozenset(orig) in edges, f
        covered.add(frozenset(orig))
        other = [int(v) for v in f if not 1 <= v <= 5][0]
        assert min(np.linalg.norm(V[other] - V[o]) for o in orig) < 0.06 * np.linalg.norm(V[orig[0]] - V[orig[1]])   # a sliver along the edge
    assert covered == edges
    assert {tuple(f) for f in F[:24]} == {tuple(f[::-1]) for f in F[24:]}            # both windings
    assert np.allclose(V[5], pose[:3, 3], atol=1e-12)                               # apex = camera centre
    W, H = imsize
    f0 = (focal.reshape(-1)[0] if isinstance(focal, np.ndarray) else focal) or min(H, W) * 1.1
    height = max(sw / 10, f0 * sw / H)
    local = (V[1:5] - pose[:3, 3]) @ pose[:3, :3]                                   # base corners in camera axes
    assert np.allclose(local[:, 2], height, rtol=1e-12)
    assert np.allclose(np.abs(local[:, 0]) / np.abs(local[:, 1]), W / H, rtol=1e-12)
    assert np.allclose(np.abs(local[:, 1]), sw / 2, rtol=1e-12)
    # the picture: uv (0, 0) on pixel (0, 0)'s side (x < 0, y < 0 in camera axes), u along +x, v along +y
    quad = (cam['image_vertices'] - pose[:3, 3]) @ pose[:3, :3]
    uv = cam['image_uv']
    for (u, v), p in zip(uv, quad):
        assert np.sign(p[0]) == (1 if u else -1) and np.sign(p[1]) == (1 if v else -1) and np.isclose(p[2], height)
    assert uv[0].tolist() == [0, 0]


def test_mesh_resource_report_has_no_scratch():
    import re
    from dust3r_amd import _lib
    path = os.path.join(os.path.dirname(_lib.LIB_PATH), 'mesh.resources.txt')
    assert os.path.exists(path), 'built by dust3r_amd/build.py'
    report = open(path).read()
    kernels = re.findall(r'Function Name: (\S+)', report)
    assert len(kernels) == 10 and all('mesh_' in k for k in kernels)
    assert re.findall(r'ScratchSize \[bytes/lane\]: (\d+)', report) == ['0'] * len(kernels)
    assert {'d3r_scene_mesh', 'd3r_scene_mesh_workspace_bytes'} <= set(_lib.EXPORTED)
