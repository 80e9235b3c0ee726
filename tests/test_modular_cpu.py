"""Host logic of the ModularPointCloudOptimizer scene (no device): mask parsing, per-image requires_grad, the reference's state_dict keys,
getters and intrinsics against the states recorded from the unmodified reference (tests/golden/aligner_modular_*.pt), and the
register / scratch report of the aligner kernels."""
import os
import re

import numpy as np
import pytest
import torch

from dust3r_amd.synthetic import synthetic_scene

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


def _gold(name):
    return torch.load(os.path.join(GOLD, name), weights_only=False)


def _modular(out, **kw):
    from dust3r_amd.cloud_opt import GlobalAlignerMode, global_aligner
    return global_aligner(out, 'cpu', mode=GlobalAlignerMode.ModularPointCloudOptimizer, verbose=False, **kw)


@pytest.fixture(scope='module')
def trace():
    return _gold('aligner_modular_trace.pt')


def test_mode_is_wired(trace):
    from dust3r_amd.cloud_opt import ModularPointCloudOptimizer
    scene = _modular(synthetic_scene(**trace['scene_args'])[0])
    assert isinstance(scene, ModularPointCloudOptimizer) and scene.has_im_poses and scene.focal_brake == 20


def test_mask_parsing(trace):
    scene = _modular(synthetic_scene(**trace['scene_args'])[0])
    assert list(scene._get_msk_indices(None)) == [0, 1, 2, 3]
    assert list(scene._get_msk_indices(2)) == [2]
    assert list(scene._get_msk_indices([0, 2])) == [0, 2]
    assert list(scene._get_msk_indices(np.array([False, True, True, False]))) == [1, 2]
    assert list(scene._get_msk_indices(torch.tensor([True, False, False, True]))) == [0, 3]
    with pytest.raises(AssertionError):
        scene._get_msk_indices(np.array([True, False]))


def test_partial_presets_freeze_single_images(trace):
    scene = _modular(synthetic_scene(**trace['scene_args'])[0], fx_and_fy=True)
    scene.load_state_dict(trace['start_state'])
    assert scene.norm_pw_scale
    scene.preset_pose(trace['known_poses'], trace['pose_msk'])
    scene.preset_focal(trace['known_focals'], trace['focal_msk'])
    assert [p.requires_grad for p in scene.im_poses] == trace['masks']['im_poses'] == [False, True, False, True]
    assert [p.requires_grad for p in scene.im_focals] == trace['masks']['im_focals'] == [True, False, True, True]
    assert [p.requires_grad for p in scene.im_pp] == [False] * 4
    assert scene.norm_pw_scale is False
    assert scene.trainable_names() == ['pw_poses', 'im_poses', 'im_depthmaps', 'im_focals']
    # the preset values: what the reference wrote (its quaternion from roma, ours from utils.rigid: fp32 rounding apart)
    for k, v in trace['preset_state'].items():
        got = scene.state_dict()[k]
        assert got.shape == v.shape, k
        assert float((got - v).abs().max()) < 1e-5, k
    # a second _set_* without force leaves a frozen entry alone, writes a trainable one (fx and fy alike)
    f1 = scene.im_focals[1].detach().clone()
    scene._set_focal(1, 99.0)
    scene._set_focal(0, 99.0)
    assert torch.equal(scene.im_focals[1].detach(), f1)
    assert torch.allclose(scene.get_focals()[0], torch.tensor([99.0, 99.0]))


def test_state_dict_uses_the_reference_keys_and_aliases_the_flat_storage(trace):
    scene = _modular(synthetic_scene(**trace['scene_args'])[0], fx_and_fy=True)
    scene.load_state_dict(trace['final_state'])
    st = scene.state_dict()
    ref_keys = set(trace['final_state'])
    assert ref_keys <= set(st) and {k for k in st if not k.startswith('im_conf.')} == ref_keys
    for k, v in trace['final_state'].items():
        assert torch.equal(st[k], v), k
    assert st['im_depthmaps.0'].shape == (24, 32) and st['im_focals.0'].shape == (2,) and st['im_poses.0'].shape == (7,)
    # the per-image parameters are views of the engine's flat tensors
    for i in range(scene.n_imgs):
        assert torch.equal(scene._flat_im_poses[i], trace['final_state'][f'im_poses.{i}'])
        assert torch.equal(scene._flat_im_depthmaps[i], trace['final_state'][f'im_depthmaps.{i}'].flatten())
        assert scene.im_poses[i].data_ptr() == scene._flat_im_poses[i].data_ptr()
    with torch.no_grad():
        scene.im_focals[3].data[:] = 5.0
    assert torch.equal(scene._flat_im_focals[3], torch.tensor([5.0, 5.0]))
    # stacked tensors load too (synthetic_scene's initial state): an (n, 1) focal fills fx and fy
    init = synthetic_scene(**trace['scene_args'])[1]
    scene.load_state_dict(init)
    assert torch.equal(scene._flat_im_focals, init['im_focals'].expand(4, 2))


def test_getters_match_the_reference(trace):
    scene = _modular(synthetic_scene(**trace['scene_args'])[0], fx_and_fy=True)
    scene.load_state_dict(trace['final_state'])
    f = scene.get_focals()
    assert f.shape == (4, 2)
    assert torch.allclose(f, trace['focals'], rtol=1e-6, atol=0)
    assert torch.allclose(scene.get_im_poses(), trace['im_poses'], rtol=0, atol=1e-5)
    K = scene.get_intrinsics()
    assert torch.equal(K[:, 0, 0], f[:, 0]) and torch.equal(K[:, 1, 1], f[:, 1])
    assert torch.equal(K[:, :2, 2], scene.get_principal_points()) and torch.equal(K[:, 2, 2], torch.ones(4))
    assert torch.equal(scene.get_principal_points(), torch.tensor([[16.0, 12.0]] * 4))
    depth = scene.get_depthmaps()
    assert len(depth) == 4 and depth[0].shape == (24, 32)
    # points: x = d (u - cx) / fx, y = d (v - cy) / fy, then the camera pose
    pts = scene.get_pts3d()
    c2w = scene.get_im_poses()
    v, u = 5, 7
    d = depth[2][v, u]
    cam = torch.stack((d * (u - 16.0) / f[2, 0], d * (v - 12.0) / f[2, 1], d))
    assert torch.allclose(pts[2][v, u], c2w[2, :3, :3] @ cam + c2w[2, :3, 3], atol=1e-5)
    assert len(scene.get_masks()) == 4 and len(scene.get_conf()) == 4


def test_isotropic_focals_and_preset_intrinsics():
    scene = _modular(synthetic_scene(3, 16, 24, seed=0, symmetrize=True)[0], optimize_pp=True)
    assert scene.get_focals().shape == (3, 1) and scene._flat_im_focals.shape == (3, 1)
    assert all(p.requires_grad for p in scene.im_pp)
    K = torch.tensor([[30.0, 0, 11.0], [0, 34.0, 9.0], [0, 0, 1]])
    scene.preset_intrinsics(K, 1)
    assert torch.allclose(scene.get_focals()[1], torch.tensor([32.0]))      # the mean of the diagonal (modular_optimizer.py:47-53)
    assert torch.allclose(scene.get_principal_points()[1], torch.tensor([11.0, 9.0]))
    assert [p.requires_grad for p in scene.im_pp] == [True, False, True]
    assert [p.requires_grad for p in scene.im_focals] == [True, False, True]


def test_global_aligner_accepts_reference_state(trace):
    """A state recorded from the reference's class (its own keys, im_conf included) loads directly."""
    scene = _modular(synthetic_scene(**trace['scene_args'])[0], fx_and_fy=True)
    st = dict(trace['final_state'])
    st.update({f'im_conf.{i}': c for i, c in enumerate(scene.im_conf)})
    scene.load_state_dict(st)
    assert torch.equal(scene._flat_im_focals[1], st['im_focals.1'])


def test_aligner_kernel_registers_and_scratch():
    """aligner.hip's resource report (dust3r_amd/build.py writes it next to the object when it compiles the file; build() runs before the suite).
    The PointCloudOptimizer main kernels keep the registers they had before the Modular scene was added (126 / 122 VGPRs). The step kernels, whose
    per-edge and per-image bodies both scenes share: one edge per thread 226 VGPRs at 256 threads and 128 + 388 B/lane of scratch at 1024 (the
    spill predates the Modular scene, then 392 B/lane), strided loops 159. The Modular instances use no scratch, and the Modular scene has no
    1024-thread step (it takes the strided kernel above 256 edges / images)."""
    from dust3r_amd.build import CSRC
    rep = os.path.join(CSRC, 'aligner.resources.txt')
    assert os.path.exists(rep), f'{rep} is missing: build() writes it'
    info, cur = {}, None
    for line in open(rep):
        m = re.search(r'Function Name: (\S+)', line)
        if m:
            cur = info.setdefault(m.group(1), {})
        for key, pat in (('vgpr', r'VGPRs: (\d+)'), ('scratch', r'ScratchSize \[bytes/lane\]: (\d+)')):
            m = re.search(pat, line)
            if m and cur is not None:
                cur[key] = int(m.group(1))
    pco = {'_ZN3d3r19aligner_main_kernelILb1ELb0EEEvNS_11AlignerViewE': (126, 0), '_ZN3d3r19aligner_main_kernelILb0ELb0EEEvNS_11AlignerViewE': (122, 0),
           '_ZN3d3r21aligner_small1_kernelILi256ELb0EEEvNS_9SmallViewE': (226, 0), '_ZN3d3r21aligner_small1_kernelILi1024ELb0EEEvNS_9SmallViewE': (128, 388),
           '_ZN3d3r20aligner_small_kernelILb0EEEvNS_9SmallViewE': (159, 0)}
    for k, (vgpr, scratch) in pco.items():
        assert (info[k]['vgpr'], info[k]['scratch']) == (vgpr, scratch), (k, info[k])
    modular = [k for k in info if re.search(r'aligner_(main|small1?)_kernel', k) and 'Lb1EEEv' in k]     # MOD = true is the last template argument
    assert sorted(modular) == sorted(['_ZN3d3r19aligner_main_kernelILb1ELb1EEEvNS_11AlignerViewE', '_ZN3d3r19aligner_main_kernelILb0ELb1EEEvNS_11AlignerViewE',
                                      '_ZN3d3r21aligner_small1_kernelILi256ELb1EEEvNS_9SmallViewE', '_ZN3d3r20aligner_small_kernelILb1EEEvNS_9SmallViewE']), modular
    for k in modular:
        assert info[k]['scratch'] == 0, (k, info[k])
    for l2 in ('0', '1'):
        assert info[f'_ZN3d3r19aligner_main_kernelILb{l2}ELb1EEEvNS_11AlignerViewE']['vgpr'] <= info[f'_ZN3d3r19aligner_main_kernelILb{l2}ELb0EEEvNS_11AlignerViewE']['vgpr']
