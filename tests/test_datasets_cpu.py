"""CPU tests (-m "not gpu") of dust3r_amd.datasets: the plans and the generator stream against what the reference recorded
(tests/golden/datasets_*.pt, tools/make_datasets_golden.py), the dataset algebra, the BatchedRandomSampler streams, the host build of
the resampler's shared arithmetic against live Pillow, and the binding of the reference's dust3r.datasets imports through the alias."""
import json
import os
import subprocess
import sys

import numpy as np
import PIL.Image
import pytest
import torch

from dust3r_amd import _lib
from dust3r_amd.datasets import (BatchedRandomSampler, CatDataset, ColorJitter, MulDataset, ResizedDataset, SyntheticStereo, get_data_loader)
from dust3r_amd.datasets.prepare import coefficient_table, fill_plan, resample_host
from dust3r_amd.datasets.synthetic import synthetic_view

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, 'tests', 'golden')
sys.path.insert(0, os.path.join(ROOT, 'tools'))
from make_datasets_golden import CASES  # noqa: E402  (the fixture tool's case table: sources, pairs, keywords)


def _dataset(name):
    sources, n_pairs, kw, _ = CASES[name]
    return SyntheticStereo(sources, n_pairs, **kw)


@pytest.mark.parametrize('name', sorted(CASES))
def test_plans_equal_the_reference_float_for_float(name):
    gold = torch.load(os.path.join(GOLD, f'datasets_{name}.pt'), weights_only=False)
    ds = _dataset(name)
    filters, flipped = set(), 0
    for idx, ref_views in zip(gold['indices'], gold['views']):
        views = ds.plan(idx)
        assert len(views) == len(ref_views) == 2
        for view, ref in zip(views, ref_views):
            plan = view['plan']
            assert (plan.crop1, plan.resample_size, plan.filter, plan.crop2) == (ref['crop1'], ref['resample_size'], ref['filter'], ref['crop2'])
            K = view['camera_intrinsics']
            assert K.dtype == np.float32 and K.tobytes() == ref['camera_intrinsics'].numpy().tobytes()
            assert view['true_shape'].dtype == np.int32 and view['true_shape'].tolist() == ref['true_shape'].tolist()
            assert view['idx'] == ref['idx'] and view['rng'] == ref['rng']
            assert (view['dataset'], view['label'], view['instance']) == ref['names']
            assert view['camera_pose'].tobytes() == ref['camera_pose'].numpy().tobytes()
            assert 'img' not in view and 'pts3d' not in view
            filters.add(plan.filter)
            flipped += plan.size[0] < plan.size[1]
    if name == 'views':      # the cases the fixtures must cover
        assert filters == {'lanczos', 'bicubic'} and flipped >= 1
        crops = [v['crop1'] for views in gold['views'] for v in views]
        assert any((r - l) <= 2 * 210 // 3 for l, t, r, b in crops), 'a first crop that removes a third of the picture'


def test_dataset_algebra():
    a, b = _dataset('views'), _dataset('views')
    assert len(2 * a) == 6 and len(10 @ a) == 10 and len(a + b) == 6 and len(2 * (a + b)) == 12
    assert isinstance(2 * a, MulDataset) and isinstance(10 @ a, ResizedDataset) and isinstance(a + b, CatDataset)
    base = "SyntheticStereo(3 pairs,split=None,seed=777,resolutions=[64x48]"
    norm = ",transform=Compose( ToTensor() Normalize(mean=(0.5, 0.5, 0.5), std=(0.5, 0.5, 0.5))))"
    assert repr(a) == base + norm
    assert repr(2 * a) == '2*' + base + norm
    assert repr(1000 @ a) == '1_000 @ ' + base + norm and repr(1000000 @ a).startswith('1_000_000 @ ')
    assert repr(a + b) == base + ')' + ' + ' + base + ')'
    assert (2 * a)._resolutions == [(64, 48)] and (a + b)._resolutions == [(64, 48)]
    # routing
    assert [v['idx'][0] for v in (2 * a).plan(5)] == [2, 2]
    assert [v['idx'][0] for v in (a + b).plan(4)] == [1, 1]
    with pytest.raises(IndexError):
        (a + b).plan(6)
    r = 7 @ a
    with pytest.raises(AssertionError, match='set_epoch'):
        r.plan(0)
    gold = json.load(open(os.path.join(GOLD, 'datasets_sampler.json')))['resized_25_of_10']
    for epoch in (0, 3):
        rr = ResizedDataset(25, list(range(10)))
        rr.set_epoch(epoch)
        assert [int(x) for x in rr._idxs_mapping] == gold[str(epoch)]
    r.set_epoch(0)
    assert r.plan(3)[0]['idx'][0] == int(r._idxs_mapping[3])
    two = _dataset('tworesolutions')
    assert (4 @ two).make_sampler(2).pool_size == 2
    r2 = 4 @ two
    r2.set_epoch(1)
    assert r2.plan((1, 1))[0]['idx'][:2] == (int(r2._idxs_mapping[1]), 1)
    with pytest.raises(AssertionError):
        (a + two)._resolutions
    with pytest.raises(NotImplementedError):
        SyntheticStereo([(64, 48, (0.5, 0.5))], 1, resolution=32, transform=ColorJitter)
    with pytest.raises(NotImplementedError):
        SyntheticStereo([(64, 48, (0.5, 0.5))], 1, resolution=32, transform='ColorJitter')


def test_batched_random_sampler_streams_equal_the_reference():
    streams = json.load(open(os.path.join(GOLD, 'datasets_sampler.json')))['streams']
    assert {(s['epoch'], s['world_size'], s['drop_last']) for s in streams} == {(0, 1, True), (3, 1, True), (0, 1, False), (3, 1, False), (0, 2, True), (3, 2, True)}
    for s in streams:
        sampler = BatchedRandomSampler(range(s['n']), s['batch_size'], s['pool_size'], world_size=s['world_size'], rank=s['rank'], drop_last=s['drop_last'])
        sampler.set_epoch(s['epoch'])
        assert len(sampler) == s['length']
        assert [[int(a), int(b)] for a, b in sampler] == s['stream']


RESAMPLE_CASES = [((640, 480), (512, 384)), ((641, 479), (299, 224)), ((1333, 1000), (512, 384)), ((500, 375), (224, 168)), ((1920, 1080), (512, 288)),
                  ((300, 200), (512, 342))]


@pytest.mark.parametrize('kind', ['noise', 'smooth'])
@pytest.mark.parametrize('src,dst', RESAMPLE_CASES)
def test_host_resampler_equals_pillow_byte_for_byte(src, dst, kind):
    (W, H), (w, h) = src, dst
    if kind == 'noise':
        a = np.random.RandomState(W + h).randint(0, 256, (H, W, 3)).astype(np.uint8)
    else:
        a = ((np.arange(W)[None, :, None] * 2 + np.arange(H)[:, None, None] * 3 + np.arange(3) * 40) % 256).astype(np.uint8)
    name, pil = ('lanczos', PIL.Image.LANCZOS) if w < W else ('bicubic', PIL.Image.BICUBIC)
    ref = np.asarray(PIL.Image.fromarray(a).resize((w, h), pil))
    assert int((resample_host(a, (0, 0, W, H), (w, h), name) != ref).sum()) == 0


def test_host_resampler_clamps_at_the_crop_edge():
    a = synthetic_view(3, 400, 300)['rgb']
    box = (37, 21, 337, 251)
    ref = np.asarray(PIL.Image.fromarray(a).crop(box).resize((111, 85), PIL.Image.LANCZOS))
    assert int((resample_host(a, box, (111, 85), 'lanczos') != ref).sum()) == 0
    uncropped = np.asarray(PIL.Image.fromarray(a).resize((148, 111), PIL.Image.LANCZOS))
    assert uncropped.shape != ref.shape
    k, b = coefficient_table(300, 111, 'lanczos')
    assert k.dtype == np.int32 and b[0, 0] == 0 and int(b[-1].sum()) == 300 and (k.sum(axis=1) - (1 << 22)).__abs__().max() <= k.shape[1]


def test_host_depth_path_equals_the_reference_views():
    """The host build of the depth gather / back-projection against the reference's views: depthmap and valid_mask exact, pts3d within
    4 * 2^-23 * (|R| |X_cam| + |t|) (three products and three sums in another order, plus the rounding of X_cam)."""
    gold = torch.load(os.path.join(GOLD, 'datasets_views.pt'), weights_only=False)
    ds = _dataset('views')
    for idx, ref_views in zip(gold['indices'], gold['views']):
        for view, ref in zip(ds.planned_views(idx), ref_views):
            H, W = ref['depthmap'].shape
            entry = fill_plan(_lib.ViewPlan(), view, H, W)
            depth_src = np.ascontiguousarray(view['depthmap'].source)
            entry.depth = depth_src.ctypes.data
            d, p, m = np.empty((H, W), np.float32), np.empty((H, W, 3), np.float32), np.empty((H, W), np.uint8)
            vp = lambda a: a.ctypes.data_as(_lib.C.c_void_p)      # noqa: E731
            _lib.check(_lib.lib.d3r_selftest_depth_host(entry, H, W, vp(d), vp(p), vp(m)), 'selftest_depth_host')
            assert d.tobytes() == ref['depthmap'].numpy().tobytes()
            assert np.array_equal(m.astype(bool), ref['valid_mask'].numpy())
            positive = view['depthmap'] > 0                        # what Co3d counts: the view before the portrait transpose
            assert np.array_equal(positive if positive.shape == (H, W) else positive.T, ref['depthmap'].numpy() > 0)
            _check_pts3d(p, ref, view['K_pixels'])


def _check_pts3d(p, ref, K_unused=None):
    pose = ref['camera_pose'].numpy().astype(np.float64)
    Xw = ref['pts3d'].numpy().astype(np.float64)
    X_cam = (Xw - pose[:3, 3]) @ pose[:3, :3]            # R is orthonormal: the camera-frame points, to fp64
    bound = 4 * 2.0 ** -23 * (np.abs(X_cam) @ np.abs(pose[:3, :3]).T + np.abs(pose[:3, 3]))
    err = np.abs(p.astype(np.float64) - Xw)
    print('pts3d max err / bound', float((err / np.maximum(bound, 1e-300)).max()))
    assert (err <= bound).all()


def test_loader_threads_and_signature():
    import inspect
    from dust3r_amd.datasets import load_threads
    assert list(inspect.signature(get_data_loader).parameters)[:6] == ['dataset', 'batch_size', 'num_workers', 'shuffle', 'drop_last', 'pin_mem']
    assert 1 <= load_threads(8) <= 8 and load_threads(64) <= 16 and load_threads(0) == 1
    loader = get_data_loader("4 @ SyntheticStereo([(64, 48, (0.5, 0.5))], 2, resolution=32, seed=1)", batch_size=2, num_workers=2)
    assert len(loader) == 2 and isinstance(loader.sampler, BatchedRandomSampler) and isinstance(loader.dataset, ResizedDataset)


def test_reference_datasets_imports_bind_through_the_alias():
    """with dust3r.datasets aliased to dust3r_amd.datasets, every name the reference's own files import from it
    (tests/golden/datasets_sampler.json 'imports', recorded by tools/make_datasets_golden.py) is this package's object."""
    imports = json.load(open(os.path.join(GOLD, 'datasets_sampler.json')))['imports']
    assert {n for _, names in imports for n in names} >= {'get_data_loader', 'BaseStereoViewDataset'}
    stmts = '\n'.join(f"from {mod} import {', '.join(names)}" for mod, names in imports)
    code = r"""
import sys, types
sys.path.insert(0, %r)
import dust3r_amd, dust3r_amd.datasets as D
m = types.ModuleType('dust3r')
m.__path__ = []
sys.modules['dust3r'] = m
for name in [k for k in sys.modules if k == 'dust3r_amd.datasets' or k.startswith('dust3r_amd.datasets.')]:
    sys.modules['dust3r.' + name[len('dust3r_amd.'):]] = sys.modules[name]
%s
from dust3r.datasets import Co3d, BatchedRandomSampler, ImgNorm, ColorJitter
from dust3r.datasets.base.easy_dataset import EasyDataset, MulDataset, ResizedDataset, CatDataset
assert get_data_loader is D.get_data_loader and BaseStereoViewDataset is D.BaseStereoViewDataset and Co3d is D.Co3d
print('aliases ok')
""" % (ROOT, stmts)
    r = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and 'aliases ok' in r.stdout, r.stderr[-2000:]
