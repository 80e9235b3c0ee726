"""GPU tests (-m gpu) of dust3r_amd.datasets: d3r_prepare_views against live Pillow and the stated depth rule, whole views against
what the reference recorded (tests/golden/datasets_*.pt), Co3d over a tree written here, the loader, and evaluate() over a loader."""
import json
import os
import re
import sys

import numpy as np
import PIL.Image
import pytest
import torch

from dust3r_amd import _lib
from dust3r_amd.datasets import Co3d, SyntheticStereo, get_data_loader
from dust3r_amd.datasets.prepare import prepare_views
from dust3r_amd.datasets.synthetic import synthetic_view

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, 'tests', 'golden')
sys.path.insert(0, os.path.join(ROOT, 'tools'))
from make_datasets_golden import CASES  # noqa: E402
DEV = 'cuda'


def _img_norm(u8_hwc):
    return (torch.from_numpy(np.array(u8_hwc, dtype=np.uint8, order='C')).permute(2, 0, 1).float().div(255) - 0.5) / 0.5


def restated_view(rgb, depth, plan, K, pose):
    """crop -> live Pillow resize -> crop -> ImgNorm, and the stated depth rule, on the host; (img, depthmap, valid) before the transpose."""
    pil = PIL.Image.fromarray(rgb).crop(plan.crop1).resize(plan.resample_size, PIL.Image.LANCZOS if plan.filter == 'lanczos' else PIL.Image.BICUBIC)
    img = _img_norm(np.asarray(pil.crop(plan.crop2)))
    l1, t1, r1, b1 = plan.crop1
    (rw, rh), (l2, t2, r2, b2) = plan.resample_size, plan.crop2
    sx = np.minimum(np.floor(np.arange(rw) * (r1 - l1) / rw).astype(int), r1 - l1 - 1)
    sy = np.minimum(np.floor(np.arange(rh) * (b1 - t1) / rh).astype(int), b1 - t1 - 1)
    d = depth[t1:b1, l1:r1][sy[:, None], sx[None, :]][t2:b2, l2:r2]
    return img, d


def _compare_with_restatement(view, rgb, depth, plan):
    img, d = restated_view(rgb, depth, plan, None, None)
    if plan.size[0] < plan.size[1]:
        img, d = img.swapaxes(1, 2), d.T
    assert torch.equal(view['img'].cpu(), img.contiguous()), 'img differs from crop -> Pillow -> crop -> ImgNorm'
    assert view['depthmap'].cpu().numpy().tobytes() == np.ascontiguousarray(d).tobytes()
    pts = view['pts3d'].cpu()
    assert torch.equal(view['valid_mask'].cpu(), torch.from_numpy(np.ascontiguousarray(d > 0)) & pts.isfinite().all(dim=-1))


def test_prepare_views_mixed_sources_equal_pillow_bit_for_bit():
    sources = [(640, 480, (0.5, 0.5)), (333, 500, (0.5, 0.5)), (1333, 1000, (0.4, 0.55)), (150, 100, (0.5, 0.5)), (500, 640, (0.45, 0.5)), (1920, 1080, (0.5, 0.5)),
               (641, 479, (1 / 3, 0.5)), (256, 192, (0.5, 0.5))]
    ds = SyntheticStereo(sources, 4, resolution=(256, 192), seed=3)
    views = [v for i in range(4) for v in ds.planned_views(i)]
    handles = [(v['img'].source, v['depthmap'].source, v['img'].plan) for v in views]
    assert {p.filter for _, _, p in handles} == {'lanczos', 'bicubic'} and len({p.source_size for _, _, p in handles}) == 8
    img, depthmap, pts3d, valid = prepare_views(views, DEV)
    assert img.shape == (8, 3, 192, 256) and img.is_cuda and valid.dtype == torch.bool and pts3d.shape == (8, 192, 256, 3)
    for view, (rgb, depth, plan) in zip(views, handles):
        _compare_with_restatement(view, rgb, depth, plan)


def test_prepare_views_taps_beyond_the_staged_run_equal_pillow():
    """A 62.5 : 1 horizontal reduction: 64 neighbouring output columns tap about 4300 source pixels = 12.9 KB per row, more than the
    12 KiB a wave of the horizontal pass stages in LDS, so the last columns of every tile read their taps from global memory."""
    ds = SyntheticStereo([(16000, 1000, (0.5, 0.5))], 1, resolution=(256, 16), seed=2)
    views = ds.planned_views(0)
    handles = [(v['img'].source, v['depthmap'].source, v['img'].plan) for v in views]
    assert all(p.resample_size == (256, 16) and p.filter == 'lanczos' and p.crop1 == (0, 0, 16000, 1000) for _, _, p in handles)
    prepare_views(views, DEV)
    for view, (rgb, depth, plan) in zip(views, handles):
        _compare_with_restatement(view, rgb, depth, plan)


def _pts3d_bound_check(pts, ref):
    pose = ref['camera_pose'].numpy().astype(np.float64)
    Xw = ref['pts3d'].numpy().astype(np.float64)
    X_cam = (Xw - pose[:3, 3]) @ pose[:3, :3]
    bound = 4 * 2.0 ** -23 * (np.abs(X_cam) @ np.abs(pose[:3, :3]).T + np.abs(pose[:3, 3]))
    err = np.abs(pts.cpu().numpy().astype(np.float64) - Xw)
    print('pts3d worst err / bound', float((err / np.maximum(bound, 1e-300)).max()))
    assert (err <= bound).all()


@pytest.mark.parametrize('name', sorted(CASES))
def test_views_equal_the_reference(name):
    """img, depthmap, valid_mask, camera_intrinsics, true_shape, idx and rng exact; pts3d componentwise within
    4 * 2^-23 * (|R| |X_cam| + |t|), every pixel included."""
    gold = torch.load(os.path.join(GOLD, f'datasets_{name}.pt'), weights_only=False)
    sources, n_pairs, kw, _ = CASES[name]
    ds = SyntheticStereo(sources, n_pairs, **kw)
    for idx, ref_views in zip(gold['indices'], gold['views']):
        for view, ref in zip(ds[idx], ref_views):
            assert set(view) == {'img', 'depthmap', 'camera_pose', 'camera_intrinsics', 'dataset', 'label', 'instance', 'idx', 'true_shape', 'pts3d', 'valid_mask', 'rng'}
            assert view['img'].dtype == torch.float32 and view['img'].is_cuda
            assert torch.equal(view['img'].cpu(), (ref['img_u8'].float().div(255) - 0.5) / 0.5)
            assert torch.equal(view['depthmap'].cpu(), ref['depthmap']) and torch.equal(view['valid_mask'].cpu(), ref['valid_mask'])
            assert view['camera_intrinsics'].tobytes() == ref['camera_intrinsics'].numpy().tobytes()
            assert view['true_shape'].tolist() == ref['true_shape'].tolist() and view['idx'] == ref['idx'] and view['rng'] == ref['rng']
            _pts3d_bound_check(view['pts3d'], ref)


def _write_co3d(root, n_frames=8, empty=(), size=(120, 90)):
    W, H = size
    seqs = {'apple': {'seq1': list(range(1, n_frames + 1))}, 'empty': {}}
    os.makedirs(root, exist_ok=True)
    for split in ('test',):
        json.dump(seqs, open(os.path.join(root, f'selected_seqs_{split}.json'), 'w'))
    base = os.path.join(root, 'apple', 'seq1')
    for d in ('images', 'depths', 'masks'):
        os.makedirs(os.path.join(base, d), exist_ok=True)
    for k, frame in enumerate(seqs['apple']['seq1']):
        sv = synthetic_view(50 + frame, W, H, (0.5, 0.5))
        PIL.Image.fromarray(sv['rgb']).save(os.path.join(base, 'images', f'frame{frame:06d}.jpg'), quality=90)
        depth16 = np.zeros((H, W), np.uint16) if k in empty else np.round(sv['depth'] / 4.0 * 65535).astype(np.uint16)
        PIL.Image.fromarray(depth16).save(os.path.join(base, 'depths', f'frame{frame:06d}.jpg.geometric.png'))
        mask = np.zeros((H, W), np.uint8)
        mask[:, : W // 2] = 255
        PIL.Image.fromarray(mask).save(os.path.join(base, 'masks', f'frame{frame:06d}.png'))
        np.savez(os.path.join(base, 'images', f'frame{frame:06d}.npz'), camera_pose=sv['pose'].astype(np.float64), camera_intrinsics=sv['K'].astype(np.float64),
                 maximum_depth=np.float64(4.0))
    return base


def test_co3d_over_a_written_tree(tmp_path):
    root = str(tmp_path / 'co3d')
    base = _write_co3d(root, n_frames=8, empty=(3,))
    ds = Co3d(split='test', ROOT=root, resolution=(64, 48), seed=7, mask_bg=False)
    assert len(ds.scene_list) == 1 and len(ds.combinations) == len([1 for i in range(100) for j in range(i + 1, 100) if (j - i) <= 30 and (j - i) % 5 == 0])
    assert len(ds) == len(ds.combinations) and ds.combinations[0] == (0, 5)
    # pair selection and the generator stream, restated: jitter of view 2 then view 1, clamped to the pool
    idx = 0
    rng = np.random.default_rng(7 + idx)
    picks = [max(0, min(im + int(rng.integers(-4, 5)), 7)) for im in (5, 0)]
    views = ds[idx]
    frames = [int(re.search(r'frame(\d+)', v['instance']).group(1)) - 1 for v in views]
    assert 3 not in picks, 'with seed 7 the jittered picks are frames 7 and 1: neither is the all-zero-depth frame'
    assert frames == picks[::-1]
    assert all(v['dataset'] == 'Co3d_v2' and v['label'] == os.path.join('apple', 'seq1') for v in views)
    # the views equal the restated pipeline on the files as PIL decodes them
    for v, plan_view in zip(views, ds.plan(idx)):
        frame = int(re.search(r'frame(\d+)', v['instance']).group(1))
        rgb = np.asarray(PIL.Image.open(os.path.join(base, 'images', f'frame{frame:06d}.jpg')).convert('RGB'))
        depth = (np.asarray(PIL.Image.open(os.path.join(base, 'depths', f'frame{frame:06d}.jpg.geometric.png'))).astype(np.float32) / 65535) * np.float64(4.0)
        _compare_with_restatement(v, rgb, depth.astype(np.float32), plan_view['plan'])
        assert v['instance'] == plan_view['instance']
    # an all-zero-depth frame is invalidated and replaced, whichever pair meets it
    for i in range(len(ds)):
        for v in ds.plan(i):
            assert 'frame000004' not in v['instance']
    assert ds.invalidate['apple', 'seq1'][(64, 48)][3] is True and sum(ds.invalidate['apple', 'seq1'][(64, 48)]) == 1
    # mask_bg: True zeroes the depth outside the mask, 'rand' draws rng.choice(2) first
    masked = Co3d(split='test', ROOT=root, resolution=(64, 48), seed=7, mask_bg=True)[idx]
    for m, v in zip(masked, views):
        if m['instance'] == v['instance']:
            assert bool((m['depthmap'][:, 40:] == 0).all()) and torch.equal(m['depthmap'][:, :24], v['depthmap'][:, :24]) and torch.equal(m['img'], v['img'])
    rand = Co3d(split='test', ROOT=root, resolution=(64, 48), seed=7, mask_bg='rand')
    draw = int(np.random.default_rng(7 + idx).choice(2))
    assert bool((rand[idx][0]['depthmap'][:, 40:] == 0).all()) == bool(draw)


def _hand_collate(pairs):
    out = []
    for side in (0, 1):
        vs = [p[side] for p in pairs]
        col = {}
        for k in vs[0]:
            x = vs[0][k]
            if isinstance(x, torch.Tensor):
                col[k] = torch.stack([v[k] for v in vs])
            elif isinstance(x, np.ndarray):
                col[k] = torch.from_numpy(np.stack([v[k] for v in vs]))
            elif isinstance(x, tuple):
                col[k] = [torch.tensor([v[k][i] for v in vs]) for i in range(3)]
            elif isinstance(x, str):
                col[k] = [v[k] for v in vs]
            else:
                col[k] = torch.tensor([v[k] for v in vs])
        out.append(col)
    return tuple(out)


def _same(a, b):
    if isinstance(a, torch.Tensor):
        return a.dtype == b.dtype and torch.equal(a.cpu(), b.cpu())
    if isinstance(a, list):
        return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    return a == b


def _loader(landscape=False):
    sources, _, kw, _ = CASES['tworesolutions']
    if landscape:      # a model built with landscape_only=False wants one true_shape per batch: no portrait or near-square sources
        sources = [(200, 150, (0.5, 0.5)), (200, 150, (0.45, 0.5)), (240, 150, (0.5, 0.5))]      # first crops 200, 180 and 240 wide, 150 high
    return get_data_loader(8 @ SyntheticStereo(sources, 6, **kw), batch_size=2, num_workers=4, device=DEV)


def test_loader_batches_equal_hand_collated_items_and_repeat():
    loader = _loader()
    assert len(loader) == 4
    epochs = []
    for _ in range(2):
        loader.dataset.set_epoch(1)      # epoch 1: the sampler's four feature draws are 0, 1, 0, 1, so both resolutions occur
        loader.sampler.set_epoch(1)
        epochs.append(list(loader))
    indices = list(loader.sampler)
    shapes = set()
    for b, batch in enumerate(epochs[0]):
        view1, view2 = batch
        tensors = [t for v in view1.values() for t in (v if isinstance(v, list) else [v]) if isinstance(t, torch.Tensor)]
        assert len(tensors) == 11 and all(t.is_cuda for t in tensors), 'every tensor of a batch is on the device'
        assert view1['img'].shape[:2] == (2, 3) and view1['valid_mask'].dtype == torch.bool and view1['true_shape'].dtype == torch.int32
        assert isinstance(view1['idx'], list) and len(view1['idx']) == 3 and isinstance(view1['label'], list) and view1['rng'].dtype == torch.int64
        shapes.add(tuple(view1['img'].shape[-2:]))
        hand = _hand_collate([loader.dataset[i] for i in indices[2 * b:2 * b + 2]])
        for side in (0, 1):
            assert set(batch[side]) == set(hand[side])
            for k in hand[side]:
                assert _same(batch[side][k], hand[side][k]), k
                assert _same(batch[side][k], epochs[1][b][side][k]), k
    assert shapes == {(32, 48), (32, 32)}


def test_evaluate_over_a_loader_equals_hand_collated_batches():
    import dust3r_amd.losses as L
    from dust3r_amd.evaluation import evaluate
    from dust3r_amd.inference import loss_of_one_batch
    from dust3r_amd.model import AsymmetricCroCo3DStereo
    from dust3r_amd.synthetic import MODEL_CONFIGS
    from oracle.dust3r_ref import build_ref_model
    model = AsymmetricCroCo3DStereo(landscape_only=False, **MODEL_CONFIGS['tiny_dpt'])
    model.load_state_dict(build_ref_model('tiny_dpt').state_dict())
    model = model.to(DEV)
    crit = eval("Regr3D_ScaleShiftInv(L21, gt_scale=True)", vars(L))
    loader = _loader(landscape=True)
    loader.dataset.set_epoch(0)
    loader.sampler.set_epoch(0)
    table = evaluate(model, crit, loader, DEV)
    indices = list(loader.sampler)
    hand = [_hand_collate([loader.dataset[i] for i in indices[2 * b:2 * b + 2]]) for b in range(len(loader))]
    assert table == evaluate(model, crit, hand, DEV)
    assert set(table) >= {'loss_avg', 'loss_med'} and all(np.isfinite(v) for v in table.values())
    res = loss_of_one_batch(next(iter(loader)), model, crit, DEV)
    assert np.isfinite(float(res['loss'][0]))


def test_views_resource_report_has_no_scratch():
    path = os.path.join(os.path.dirname(_lib.LIB_PATH), 'views.resources.txt')
    assert os.path.exists(path), 'built by dust3r_amd/build.py'
    report = open(path).read()
    kernels = re.findall(r'Function Name: (\S+)', report)
    assert sum('views_' in k for k in kernels) == 3
    assert re.findall(r'ScratchSize \[bytes/lane\]: (\d+)', report) == ['0'] * len(kernels)
    assert {'d3r_prepare_views', 'd3r_view_plan_bytes', 'd3r_selftest_resample_host'} <= set(_lib.EXPORTED)
