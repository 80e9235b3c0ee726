"""The GLB export on the GPU: the kernels of csrc/mesh.hip (viz.scene_mesh_batch) against the numpy restatement of tests/test_glb_cpu.py,
exactly; determinism; indices past 2^24; and dust3r_amd.demo.get_3D_model_from_scene end to end on scenes built by the demo's body, read back
with the test's GLB reader."""
import copy
import io
import os

import numpy as np
import pytest
import torch

from test_glb_cpu import read_glb, restated_faces, restated_mesh, restated_pointcloud, root_matrix

pytestmark = pytest.mark.gpu


def _views(rng, u8):
    """(H, W, mask kind): mixed sizes and orientations, h = 1 and w = 1, all-false / all-true masks, isolated valid pixels, views of many tiles"""
    spec = [(7, 5, 'random'), (16, 12, 'random'), (12, 16, 'random'), (1, 9, 'true'), (9, 1, 'true'), (6, 8, 'false'), (5, 7, 'true'),
            (33, 40, 'isolated'), (40, 50, 'random'), (70, 90, 'sparse'), (2, 2, 'true'), (96, 64, 'random')]
    imgs, pts, masks = [], [], []
    for H, W, kind in spec:
        if u8:
            imgs.append(rng.integers(0, 256, size=(H, W, 3)).astype(np.uint8))
        else:
            im = rng.random((H, W, 3)).astype(np.float32)
            im.reshape(-1)[:6] = [0.0, 1.0, 0.5 / 255, 1.5 / 255, 254.5 / 255, 1.0 - 1e-7]   # rounding edges
            imgs.append(im)
        pts.append(rng.normal(size=(H, W, 3)).astype(np.float32) * 3 + 1)
        if kind == 'isolated':
            m = np.zeros((H, W), bool)
            m[::3, ::3] = True
        else:
            m = {'true': np.ones((H, W), bool), 'false': np.zeros((H, W), bool), 'random': rng.random((H, W)) < 0.7,
                 'sparse': rng.random((H, W)) < 0.35}[kind]
        masks.append(m)
    return imgs, pts, masks


def _check(got, want, as_pointcloud, counts):
    assert got['positions'].dtype == np.float32 and got['colors'].dtype == np.uint8
    assert np.array_equal(got['positions'], want['positions'])
    assert np.array_equal(got['colors'], want['colors'])
    if as_pointcloud:
        assert got['faces'] is None
    else:
        assert got['faces'].dtype == np.uint32 and np.array_equal(got['faces'].astype(np.int64), want['faces'])
    assert got['counts'].tolist() == counts
    if want['bounds'] is None:
        assert got['bounds'] is None
    else:
        assert np.array_equal(got['bounds'][0], want['bounds'][0]) and np.array_equal(got['bounds'][1], want['bounds'][1])


def _per_view_counts(masks, as_pointcloud):
    if as_pointcloud:
        return [int(m.sum()) for m in masks]
    return [len(restated_faces([m.shape], [m])[0]) for m in masks]


@pytest.mark.parametrize('u8', [True, False])
@pytest.mark.parametrize('as_pointcloud', [False, True])
def test_kernels_equal_the_restatement(gpu, u8, as_pointcloud):
    from dust3r_amd.viz import scene_mesh_batch
    rng = np.random.default_rng(1 + 2 * u8 + as_pointcloud)
    imgs, pts, masks = _views(rng, u8)
    want = (restated_pointcloud if as_pointcloud else restated_mesh)(imgs, pts, masks)
    counts = _per_view_counts(masks, as_pointcloud)
    got = scene_mesh_batch(imgs, pts, masks, gpu, as_pointcloud=as_pointcloud)                 # numpy inputs
    _check(got, want, as_pointcloud, counts)
    # device tensors, pointmaps in the padded (n, max_area, 3) layout of scene.get_pts3d(raw=True)
    A = max(p.shape[0] * p.shape[1] for p in pts) + 5
    padded = torch.zeros((len(pts), A, 3), device=gpu)
    for i, p in enumerate(pts):
        padded[i, :p.shape[0] * p.shape[1]] = torch.from_numpy(p.reshape(-1, 3))
    got = scene_mesh_batch([torch.from_numpy(im).to(gpu) for im in imgs], padded, [torch.from_numpy(m).to(gpu) for m in masks], gpu,
                           as_pointcloud=as_pointcloud)
    _check(got, want, as_pointcloud, counts)


def test_nothing_valid(gpu):
    from dust3r_amd.viz import scene_mesh_batch
    imgs = [np.zeros((5, 4, 3), np.float32), np.zeros((1, 1, 3), np.float32)]
    pts = [np.ones((5, 4, 3), np.float32), np.ones((1, 1, 3), np.float32)]
    masks = [np.eye(5, 4, dtype=bool), np.ones((1, 1), bool)]         # diagonal pixels: no triangle has three valid pixels
    got = scene_mesh_batch(imgs, pts, masks, gpu)
    assert got['bounds'] is None and got['faces'].shape == (0, 3) and got['counts'].tolist() == [0, 0]
    assert np.array_equal(got['colors'], restated_mesh(imgs, pts, masks)['colors'])
    got = scene_mesh_batch(imgs, pts, [np.zeros((5, 4), bool), np.zeros((1, 1), bool)], gpu, as_pointcloud=True)
    assert got['bounds'] is None and len(got['positions']) == 0


def test_large_scene_indices_past_2_24_and_determinism(gpu):
    """92 views of 512 x 384: vertex indices reach 18.1 M > 2^24 (a float-typed offset would round them). The last views' faces are restated
    with their offsets; two calls give the same bytes."""
    from dust3r_amd.viz import scene_mesh_batch
    n, H, W = 92, 384, 512
    g = torch.Generator(device=gpu)
    g.manual_seed(5)
    pts = torch.randn((n, H * W, 3), device=gpu, generator=g)
    masks = [m for m in (torch.rand((n, H, W), device=gpu, generator=g) < 0.7)]
    imgs = [im for im in torch.randint(0, 256, (n, H, W, 3), device=gpu, generator=g, dtype=torch.uint8)]
    a = scene_mesh_batch(imgs, pts, masks, gpu)
    b = scene_mesh_batch(imgs, pts, masks, gpu)
    for k in ('positions', 'colors', 'faces', 'counts'):
        assert a[k].tobytes() == b[k].tobytes(), k
    assert a['faces'].max() >= 2 ** 24
    last = 2
    m_last = [m.cpu().numpy() for m in masks[-last:]]
    faces, _ = restated_faces([(H, W)] * last, m_last)
    n_before = int(a['counts'][:-last].sum())
    assert np.array_equal(a['faces'][n_before:].astype(np.int64), faces + (n - last) * H * W)
    assert int(a['counts'].sum()) == len(a['faces'])


# ---- end to end ---------------------------------------------------------------------------------------------------------------------
def _write_images(tmp_path, sizes):
    import PIL.Image
    from dust3r_amd.synthetic import synthetic_photo
    paths = []
    for k, (W, H) in enumerate(sizes):
        p = os.path.join(str(tmp_path), f'view{k}.png')
        PIL.Image.fromarray(synthetic_photo(W, H, seed=20 + k)).save(p)
        paths.append(p)
    return paths


def _engine(gpu):
    from dust3r_amd.model import AsymmetricCroCo3DStereo
    from dust3r_amd.synthetic import MODEL_CONFIGS
    from oracle.dust3r_ref import build_ref_model
    m = AsymmetricCroCo3DStereo(landscape_only=False, **MODEL_CONFIGS['tiny_dpt'])
    m.load_state_dict(build_ref_model('tiny_dpt').state_dict())
    return m.to(gpu)


def _scene(files, model, device, image_size, niter):
    """dust3r/demo.py:135-186 up to the aligned scene (the body of tests/test_demo_flow_gpu.py)"""
    from dust3r_amd.cloud_opt import GlobalAlignerMode, global_aligner
    from dust3r_amd.image_pairs import make_pairs
    from dust3r_amd.inference import inference
    from dust3r_amd.utils.image import load_images
    imgs = load_images(files, size=image_size, verbose=False, patch_size=model.patch_size, square_ok=False)
    pairs = make_pairs(imgs, scene_graph='complete', prefilter=None, symmetrize=True)
    output = inference(pairs, model, device, batch_size=1, verbose=False)
    mode = GlobalAlignerMode.PointCloudOptimizer if len(imgs) > 2 else GlobalAlignerMode.PairViewer
    scene = global_aligner(output, device=device, mode=mode, verbose=False)
    if mode == GlobalAlignerMode.PointCloudOptimizer:
        scene.compute_global_alignment(init='mst', niter=niter, schedule='linear', lr=0.01)
    return scene


@pytest.fixture(scope='module')
def scenes(gpu, tmp_path_factory):
    tmp = tmp_path_factory.mktemp('glb_scenes')
    model = _engine(gpu)
    multi = _scene(_write_images(tmp, [(200, 150), (150, 200), (200, 150)]), model, gpu, 96, 20)
    pair = _scene(_write_images(tmp, [(200, 150), (180, 150)]), model, gpu, 128, 10)
    return dict(multi=multi, pair=pair)


ARMS = [  # as_pointcloud, mask_sky, clean_depth, transparent_cams
    (False, False, False, False), (True, False, False, False), (False, True, True, False), (True, True, False, True), (False, False, True, True)]


@pytest.mark.parametrize('which', ['multi', 'pair'])
@pytest.mark.parametrize('as_pointcloud,mask_sky,clean_depth,transparent_cams', ARMS)
def test_get_3D_model_from_scene(gpu, scenes, tmp_path, which, as_pointcloud, mask_sky, clean_depth, transparent_cams):
    import PIL.Image
    from scipy.spatial.transform import Rotation
    from dust3r_amd.demo import get_3D_model_from_scene
    from dust3r_amd.viz import OPENGL
    min_conf_thr = 2.0
    # the expected values, from the reference's formula on a copy that went through the same post-processing
    ref = copy.deepcopy(scenes[which])
    if clean_depth:
        ref = ref.clean_pointcloud()
    if mask_sky:
        ref = ref.mask_sky()
    with torch.no_grad():
        pts = [p.detach().cpu().numpy() for p in ref.get_pts3d()]
        c2w = ref.get_im_poses().detach().cpu().numpy()
        ref.min_conf_thr = float(ref.conf_trf(torch.tensor(min_conf_thr)))
        msk = [m.cpu().numpy() for m in ref.get_masks()]
    imgs = ref.imgs
    out = get_3D_model_from_scene(str(tmp_path), True, copy.deepcopy(scenes[which]), min_conf_thr=min_conf_thr, as_pointcloud=as_pointcloud,
                                  mask_sky=mask_sky, clean_depth=clean_depth, transparent_cams=transparent_cams)
    assert out == os.path.join(str(tmp_path), 'scene.glb')
    doc, acc, view = read_glb(out)
    rot = np.eye(4)
    rot[:3, :3] = Rotation.from_euler('y', np.deg2rad(180)).as_matrix()
    T = np.linalg.inv(c2w[0] @ OPENGL @ rot)                                    # demo.py:100-102
    # (a random-weight network can give degenerate poses and points: NaN compares equal to NaN below)
    assert np.allclose(root_matrix(doc), T, rtol=1e-6, atol=1e-6, equal_nan=True)
    want = (restated_pointcloud if as_pointcloud else restated_mesh)(imgs, pts, msk)
    nodes = {n.get('name'): n for n in doc['nodes']}
    if want['bounds'] is None:
        assert 'scene' not in nodes
    else:
        prim = doc['meshes'][nodes['scene']['mesh']]['primitives'][0]
        P = acc(prim['attributes']['POSITION'])
        assert np.array_equal(P, want['positions'], equal_nan=True)              # untransformed fp32 points, bit for bit
        world = P.astype(np.float64) @ root_matrix(doc)[:3, :3].T + root_matrix(doc)[:3, 3]
        assert np.allclose(world, want['positions'].astype(np.float64) @ T[:3, :3].T + T[:3, 3], rtol=1e-5, atol=1e-5, equal_nan=True)
        pa = doc['accessors'][prim['attributes']['POSITION']]
        used = P[np.unique(acc(prim['indices']))] if not as_pointcloud else P
        for k in range(3):
            col = used[:, k][np.isfinite(used[:, k])]
            assert (pa['min'][k], pa['max'][k]) == ((float(col.min()), float(col.max())) if len(col) else (0.0, 0.0))
        assert np.array_equal(acc(prim['attributes']['COLOR_0']), want['colors'])
        if as_pointcloud:
            assert prim['mode'] == 0
        else:
            assert prim['mode'] == 4 and np.array_equal(acc(prim['indices']).astype(np.int64), want['faces'].reshape(-1))
    n = len(imgs)
    assert sorted(k for k in nodes if k and k.startswith('camera_') and not k.endswith('_image')) == sorted(f'camera_{i}' for i in range(n))
    pics = [nodes.get(f'camera_{i}_image') for i in range(n)]
    if transparent_cams:
        assert all(p is None for p in pics) and 'images' not in doc
    else:
        for i, node in enumerate(pics):
            mat = doc['materials'][doc['meshes'][node['mesh']]['primitives'][0]['material']]
            img = doc['images'][doc['textures'][mat['pbrMetallicRoughness']['baseColorTexture']['index']]['source']]
            assert np.array_equal(np.asarray(PIL.Image.open(io.BytesIO(view(img['bufferView'])))), np.uint8(255 * imgs[i]))


def test_get_3D_model_from_scene_without_images_raises(gpu, scenes, tmp_path):
    from dust3r_amd.demo import get_3D_model_from_scene
    s = copy.deepcopy(scenes['pair'])
    s.imgs = None
    with pytest.raises(ValueError, match='scene.imgs is None'):
        get_3D_model_from_scene(str(tmp_path), True, s)
    assert get_3D_model_from_scene(str(tmp_path), True, None) is None
