"""The engine binding both alignment scenes share (BasePCOptimizer._ensure_engine): when the engine is kept, when it is rebuilt, that a rebuilt
engine computes what a fresh one does, and that a failure after d3r_aligner_create releases the handle. One 3-image scene of mixed sizes."""
import copy

import pytest
import torch

from dust3r_amd.synthetic import synthetic_mixed_scene

pytestmark = pytest.mark.gpu
SHAPES = [(8, 12), (12, 8), (8, 12)]


@pytest.fixture(scope='module')
def output():
    return synthetic_mixed_scene(SHAPES, seed=0)         # all six directed edges; read-only


def _scene(gpu, output, mode):
    from dust3r_amd.cloud_opt import GlobalAlignerMode, global_aligner
    torch.manual_seed(0)                                  # the scenes draw their start (init=None)
    return global_aligner(output, gpu, mode=GlobalAlignerMode(mode), verbose=False)


MODES = ['PointCloudOptimizer', 'ModularPointCloudOptimizer']


@pytest.mark.parametrize('mode', MODES)
def test_engine_is_kept_until_trainability_changes(gpu, output, mode):
    scene = _scene(gpu, output, mode)
    first = scene.forward()
    handle, sig = scene._engine.value, scene._engine_sig
    assert torch.isfinite(first) and torch.equal(scene.forward(), first)
    assert scene._engine.value == handle and scene._engine_sig == sig
    if mode == 'PointCloudOptimizer':
        scene.preset_focal([15.0] * 3)
    else:
        scene.preset_focal([15.0], 1)
    loss = scene.forward()
    assert scene._engine_sig != sig and not torch.equal(loss, first)
    twin = copy.deepcopy(scene)
    assert twin._engine is None
    assert torch.equal(twin.forward(), loss) and twin._engine.value != scene._engine.value


@pytest.mark.parametrize('mode', MODES)
def test_short_alignment_equals_its_deepcopy(gpu, output, mode):
    scene = _scene(gpu, output, mode)
    twin = copy.deepcopy(scene)
    losses = [s.compute_global_alignment(init=None, niter=5, schedule='linear') for s in (scene, twin)]
    assert losses[0] == losses[1] and losses[0] == losses[0]          # equal and not NaN
    for (k, a), b in zip(scene._engine_tensors().items(), twin._engine_tensors().values()):
        assert a.data_ptr() != b.data_ptr() and torch.equal(a, b), k
    assert torch.equal(scene.forward(), twin.forward())


def test_failure_after_create_destroys_the_handle(gpu, output, monkeypatch):
    from dust3r_amd._lib import D3RError, lib
    scene = _scene(gpu, output, 'PointCloudOptimizer')
    real_create, real_set, real_destroy = lib.d3r_aligner_create, lib.d3r_aligner_set_option, lib.d3r_aligner_destroy
    created, destroyed, refused = [], [], []

    def create(out, *args):
        rc = real_create(out, *args)
        created.append(out._obj.value)
        return rc

    def set_option(h, opt, value):
        if not refused:
            refused.append(opt)
            return -1                                                   # D3R_ERR_INVALID: the host's argument-error path
        return real_set(h, opt, value)

    def destroy(h):
        destroyed.append(h.value)
        return real_destroy(h)

    monkeypatch.setattr(lib, 'd3r_aligner_create', create)
    monkeypatch.setattr(lib, 'd3r_aligner_set_option', set_option)
    monkeypatch.setattr(lib, 'd3r_aligner_destroy', destroy)
    with pytest.raises(D3RError):
        scene._ensure_engine()
    assert len(created) == 1 and created[0] and destroyed == created and scene._engine is None
    assert torch.isfinite(scene.forward()) and len(created) == 2 and scene._engine.value == created[1]
