"""A scene hands its padded stacks (`_im_conf`, `get_depthmaps(raw=True)`, `get_pts3d(raw=True)`, `get_masks(raw=True)`, `_shape_tables`) to the
GPU post-processing calls. Everything here is bit equality: the stacks against the lists, the consumers with poisoned padding against
themselves before the poison, a scene before and after a device round trip."""
import copy

import numpy as np
import pytest
import torch

from dust3r_amd.synthetic import outdoor_scene, synthetic_mixed_scene
from dust3r_amd.utils.padded import split_views

pytestmark = pytest.mark.gpu
SHAPES = [(16, 24), (24, 16), (8, 12)]          # the third image is smaller than max_area: real padding
THR = 90.0                                       # conf_trf(90) = log 90 = 4.5: a part of every confidence map passes


def _scene(gpu, shapes, mode):
    from dust3r_amd.cloud_opt import GlobalAlignerMode, global_aligner
    out = synthetic_mixed_scene(shapes, seed=3)
    pics = [torch.from_numpy(outdoor_scene(h, w, seed=i)).permute(2, 0, 1).float() / 127.5 - 1 for i, (h, w) in enumerate(shapes)]
    for view in ('view1', 'view2'):
        out[view]['img'] = [pics[i] for i in out[view]['idx']]
    torch.manual_seed(0)
    scene = global_aligner(out, gpu, mode=GlobalAlignerMode(mode), verbose=False)
    scene.compute_global_alignment(init='mst', niter=3, schedule='linear', lr=0.01)
    return scene


def _glb_bytes(tmp_path, scene, as_pointcloud):
    from dust3r_amd.demo import get_3D_model_from_scene
    with open(get_3D_model_from_scene(str(tmp_path), True, scene, min_conf_thr=THR, as_pointcloud=as_pointcloud), 'rb') as f:
        return f.read()


def _bytes(x):
    return x.detach().cpu().contiguous().numpy().tobytes() if isinstance(x, torch.Tensor) else np.ascontiguousarray(x).tobytes()


def _equal_lists(a, b):
    """Bit for bit (a NaN equals the same NaN: random pointmaps can give a degenerate camera)."""
    return len(a) == len(b) and all(x.shape == y.shape and x.dtype == y.dtype and _bytes(x) == _bytes(y) for x, y in zip(a, b))


def _one_storage(scene):
    return {c.untyped_storage().data_ptr() for c in scene.im_conf} == {scene._im_conf.untyped_storage().data_ptr()}


def test_pair_viewer_honours_raw(gpu, tmp_path):
    from dust3r_amd.demo import write_scene_glb
    from dust3r_amd.utils.device import to_numpy
    from dust3r_amd.viz import scene_mesh_batch
    scene = _scene(gpu, SHAPES[:2], 'PairViewer')
    pts, depth = scene.get_pts3d(raw=True), scene.get_depthmaps(raw=True)
    assert pts.shape == (2, 384, 3) and depth.shape == (2, 384) and pts.is_contiguous() and depth.is_contiguous()
    assert _equal_lists(split_views(pts, SHAPES[:2]), scene.get_pts3d()) and _equal_lists(split_views(depth, SHAPES[:2]), scene.get_depthmaps())
    assert [tuple(p.shape) for p in scene.get_pts3d()] == [(16, 24, 3), (24, 16, 3)]
    for as_pointcloud in (False, True):
        got = _glb_bytes(tmp_path, scene, as_pointcloud)
        # the list path: per-view maps into scene_mesh_batch, the file written from its result
        with torch.no_grad():
            scene.min_conf_thr = float(scene.conf_trf(torch.tensor(THR)))
            geo = scene_mesh_batch(to_numpy(scene.imgs), scene.get_pts3d(), scene.get_masks(), gpu, as_pointcloud=as_pointcloud)
        assert geo['counts'].sum() > 0
        listed = str(tmp_path / 'listed.glb')
        write_scene_glb(listed, geo, to_numpy(scene.imgs), to_numpy(scene.get_focals().cpu()), to_numpy(scene.get_im_poses().cpu()),
                        cam_size=0.05, as_pointcloud=as_pointcloud)
        with open(listed, 'rb') as f:
            assert f.read() == got


@pytest.mark.parametrize('mode', ['PointCloudOptimizer', 'ModularPointCloudOptimizer'])
def test_no_consumer_reads_the_padding(gpu, tmp_path, mode):
    """NaN behind every image's h * w in `_im_conf` and in the third image's depth row (so in `get_pts3d(raw=True)` too): every consumer
    gives what it gave before. (The alignment loop is not run again: its zero weights times NaN would be NaN by design.)"""
    from dust3r_amd.demo import scene_gallery
    scene = _scene(gpu, SHAPES, mode)

    def consumers():
        cleaned = copy.deepcopy(scene).clean_pointcloud()
        return dict(gallery=scene_gallery(scene), mesh=_glb_bytes(tmp_path, scene, False), cloud=_glb_bytes(tmp_path, scene, True),
                    views=scene.render_views(), mesh_views=scene.render_views(as_mesh=True),
                    cleaned=[c.clone() for c in cleaned.im_conf], sky=[c.clone() for c in scene.mask_sky().im_conf])
    before = consumers()
    with torch.no_grad():
        for i, (h, w) in enumerate(SHAPES):
            scene._im_conf[i, h * w:] = float('nan')
        scene._flat_im_depthmaps.data[2, 8 * 12:] = float('nan')
        assert torch.isnan(scene._im_conf[2, 96:]).all() and torch.isnan(scene.get_pts3d(raw=True)[2, 96:]).all()
        assert all(torch.isfinite(c).all() for c in scene.im_conf)
    after = consumers()
    print('clean_pointcloud clipped', sum(int((a != b).sum()) for a, b in zip(before['cleaned'], scene.im_conf)), 'confidences, mask_sky',
          sum(int((a != b).sum()) for a, b in zip(before['sky'], scene.im_conf)))
    assert len(after['gallery']) == 9 and _equal_lists(after['gallery'], before['gallery'])
    assert after['mesh'] == before['mesh'] and after['cloud'] == before['cloud']
    for key in ('views', 'mesh_views'):
        assert len(after[key]) == 3 and _equal_lists(after[key], before[key])
    assert _equal_lists(after['cleaned'], before['cleaned']) and _equal_lists(after['sky'], before['sky'])


def test_to_keeps_the_stack(gpu):
    from dust3r_amd.demo import scene_gallery
    scene = _scene(gpu, SHAPES, 'PointCloudOptimizer')
    before = scene_gallery(scene)
    assert scene.to('cpu') is scene and scene._im_conf.device.type == 'cpu' and _one_storage(scene)
    assert scene.to(gpu) is scene and scene._im_conf.is_cuda and _one_storage(scene)
    assert scene._shape_tables[2].is_cuda and scene._shape_tables[2].tolist() == [384, 384, 96]
    after = scene_gallery(scene)
    assert len(after) == 9 and _equal_lists(after, before)
