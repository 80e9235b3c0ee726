"""The padded layout (dust3r_amd/utils/padded.py) and the scene's open ownership of its stacks, off the GPU: pad / split / tables round
trips, `im_conf` as views of the `_im_conf` buffer through construction, .to(), deepcopy, assignment, and the state dicts."""
import copy

import numpy as np
import pytest
import torch

from dust3r_amd.synthetic import synthetic_mixed_scene
from dust3r_amd.utils.padded import pad_views, shape_tables, split_views

SHAPES = [(16, 24), (24, 16), (8, 12)]          # the third image is smaller than max_area: real padding


@pytest.fixture(scope='module')
def output():
    return synthetic_mixed_scene(SHAPES, seed=3)          # per-pair lists, complete symmetrised graph; read-only


def _scene(output, mode):
    from dust3r_amd.cloud_opt import GlobalAlignerMode, global_aligner
    torch.manual_seed(0)
    return global_aligner(output, 'cpu', mode=GlobalAlignerMode(mode), verbose=False)


def _one_storage(scene):
    return {c.untyped_storage().data_ptr() for c in scene.im_conf} == {scene._im_conf.untyped_storage().data_ptr()}


@pytest.mark.parametrize('dtype', [torch.float32, torch.uint8, torch.bool])
@pytest.mark.parametrize('tail', [(), (3,)])
@pytest.mark.parametrize('source', ['numpy', 'tensor'])
def test_pad_split_round_trip(dtype, tail, source):
    rng = np.random.default_rng(5)
    maps = [torch.from_numpy(rng.integers(0, 2 if dtype == torch.bool else 200, size=hw + tail)).to(dtype) for hw in SHAPES]
    given = [m.numpy() for m in maps] if source == 'numpy' else maps
    stack = pad_views(given, 'cpu', dtype, tail=tail)
    assert stack.shape == (3, 384) + tail and stack.dtype == dtype and stack.is_contiguous() and stack.data_ptr() % 16 == 0
    views = split_views(stack, SHAPES)
    for v, m, (h, w) in zip(views, maps, SHAPES):
        assert v.shape == (h, w) + tail and torch.equal(v, m) and v.untyped_storage().data_ptr() == stack.untyped_storage().data_ptr()
    assert not stack[2, 8 * 12:].any() and not stack[0, 384:].any()          # zeros behind every view
    views[2][1, 2] = 1                                                         # a view writes to the stack
    assert stack[2, 12 + 2].all()
    # rows: the largest area rounded up to a multiple of 4, or as asked
    odd = [np.ones((3, 3) + tail, np.float32), np.ones((1, 2) + tail, np.float32)]
    assert pad_views(odd, 'cpu', torch.float32, tail=tail).shape == (2, 12) + tail
    assert pad_views(odd, 'cpu', torch.float32, tail=tail, row=9).shape == (2, 9) + tail
    with pytest.raises(ValueError):
        pad_views(odd, 'cpu', torch.float32, tail=tail, row=8)


def test_shape_tables():
    heights, widths, npix = shape_tables(SHAPES, 'cpu')
    for t, want in ((heights, [16, 24, 8]), (widths, [24, 16, 12]), (npix, [384, 384, 96])):
        assert t.dtype == torch.int32 and t.tolist() == want and t.is_contiguous()
    assert heights.untyped_storage().data_ptr() == npix.untyped_storage().data_ptr()          # one array, one upload


def test_pad_views_names_the_wrong_sized_map():
    maps = [np.zeros((4, 4, 3), np.float32), np.zeros((4, 4, 2), np.float32), np.zeros((2, 4, 3), np.float32)]
    with pytest.raises(ValueError, match=r'pointmap 1 has shape \(4, 4, 2\)'):
        pad_views(maps, 'cpu', torch.float32, tail=(3,), name='pointmap')
    with pytest.raises(ValueError, match=r'mask 2 has shape \(2, 4\)'):
        pad_views([np.zeros((4, 4)), np.zeros((4, 4)), np.zeros((2, 4))], 'cpu', torch.uint8, shapes=[(4, 4)] * 3, name='mask')


def test_pad_views_passes_a_ready_stack_on():
    stack = torch.arange(3 * 384 * 3, dtype=torch.float32).reshape(3, 384, 3)
    assert pad_views(stack, 'cpu', torch.float32, tail=(3,), shapes=SHAPES).data_ptr() == stack.data_ptr()          # no copy where none is needed
    masks = stack[..., 0] > 500
    as_u8 = pad_views(masks, 'cpu', torch.uint8, row=384, shapes=SHAPES)
    assert as_u8.dtype == torch.uint8 and torch.equal(as_u8.bool(), masks)
    for kw in (dict(row=388), dict(shapes=[(16, 25)] * 3)):          # another row length; a view that does not fit the rows
        with pytest.raises(ValueError, match='padded stack'):
            pad_views(stack, 'cpu', torch.float32, tail=(3,), **kw)


@pytest.mark.parametrize('mode', ['PointCloudOptimizer', 'ModularPointCloudOptimizer', 'PairViewer'])
def test_im_conf_is_views_of_one_buffer(output, mode):
    if mode == 'PairViewer':
        output = synthetic_mixed_scene(SHAPES[:2], seed=3)
    scene = _scene(output, mode)
    n = scene.n_imgs
    assert '_im_conf' in scene._buffers and scene._im_conf.shape == (n, 384) and 'im_conf' not in scene.__dict__
    assert [tuple(c.shape) for c in scene.im_conf] == SHAPES[:n] and _one_storage(scene)
    # the reference's rule: per image the maximum over the edge sides that show it
    for i, c in enumerate(scene.im_conf):
        want = torch.stack([scene.conf_i[k] for k in scene.str_edges if k.startswith(f'{i}_')]
                           + [scene.conf_j[k] for k in scene.str_edges if k.endswith(f'_{i}')]).amax(0)
        assert torch.equal(c, want)
    before = scene._im_conf.clone()
    assert scene.to('cpu') is scene and _one_storage(scene) and torch.equal(scene._im_conf, before)
    res = copy.deepcopy(scene)
    assert _one_storage(res) and res._im_conf.untyped_storage().data_ptr() != scene._im_conf.untyped_storage().data_ptr()
    assert torch.equal(res._im_conf, before)
    res.im_conf[n - 1][1, 2] = -7.0
    assert float(res._im_conf[n - 1, 12 + 2 if n == 3 else 16 + 2]) == -7.0 and torch.equal(scene._im_conf, before)


def test_im_conf_assignment_copies_into_the_buffer(output):
    scene = _scene(output, 'PointCloudOptimizer')
    buffer = scene._im_conf
    mine = [c.clone() + 1 for c in scene.im_conf]
    scene.im_conf = mine
    assert scene._im_conf is buffer and _one_storage(scene)
    assert all(torch.equal(a, b) for a, b in zip(scene.im_conf, mine))
    scene.im_conf[1][2:4, 3:5] = 0
    assert not scene._im_conf[1].view(24, 16)[2:4, 3:5].any() and mine[1][2:4, 3:5].all()          # the caller's tensors are not kept
    assert int((scene._im_conf[1] == 0).sum()) == 4
    with pytest.raises(ValueError):
        scene.im_conf = mine[:2]


@pytest.mark.parametrize('mode', ['PointCloudOptimizer', 'ModularPointCloudOptimizer'])
def test_state_dict_keeps_the_reference_keys(output, mode):
    scene = _scene(output, mode)
    state = scene.state_dict()
    assert {k for k in state if 'im_conf' in k} == {'im_conf.0', 'im_conf.1', 'im_conf.2'}
    for i, c in enumerate(scene.im_conf):
        assert torch.equal(state[f'im_conf.{i}'], c) and state[f'im_conf.{i}'].data_ptr() != c.data_ptr()
    other = _scene(output, mode)
    with torch.no_grad():
        other._im_conf.fill_(-1.0)
    other.load_state_dict(state)
    assert all(torch.equal(a, b) for a, b in zip(other.im_conf, scene.im_conf))
    assert torch.equal(other._im_conf[2, 96:], torch.full((288,), -1.0))          # only the views are written
    for k, v in state.items():
        assert torch.equal(other.state_dict()[k], v), k
