"""GPU parity of the ModularPointCloudOptimizer scene on the fused aligner against the UNMODIFIED reference class
(tests/golden/aligner_modular_*.pt, written by tools/make_modular_golden.py): loss and gradients per configuration, a
300-iteration trace with partial presets, init='mst' with two known poses, and the engine's Modular-specific paths."""
import os

import pytest
import torch

from dust3r_amd.synthetic import synthetic_mixed_scene, synthetic_scene

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


def _gold(name):
    return torch.load(os.path.join(GOLD, name), weights_only=False)


def rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def _output(case):
    if case['scene'] == 'synthetic_mixed_scene':
        return synthetic_mixed_scene(**case['scene_args'])
    return synthetic_scene(**case['scene_args'])[0]


def _modular(gpu, out, **kw):
    from dust3r_amd.cloud_opt import GlobalAlignerMode, global_aligner
    return global_aligner(out, gpu, mode=GlobalAlignerMode.ModularPointCloudOptimizer, verbose=False, **kw)


def _stacked(scene, grads, name):
    """The engine's flat gradient of an image group as the reference's per-image list."""
    g = grads[name]
    if name == 'im_depthmaps':
        return [g[i, :h * w].view(h, w) for i, (h, w) in enumerate(scene.imshapes)]
    return list(g)


@pytest.mark.parametrize('name', ['isotropic', 'fx_and_fy', 'optimize_pp', 'l2', 'conf_sqrt', 'mixed_sizes', 'mixed_sizes_fx_and_fy'])
def test_loss_and_gradients_match_reference(gpu, name):
    case = next(c for c in _gold('aligner_modular_grads.pt')['cases'] if c['name'] == name)
    scene = _modular(gpu, _output(case), **case['kw'])
    scene.load_state_dict(case['state'])
    loss, grads = scene.loss_and_grads()
    assert abs(float(loss) / case['loss'] - 1) < 1e-5, (float(loss), case['loss'])
    assert abs(float(scene()) / case['loss'] - 1) < 1e-5
    for k, ref in case['grads'].items():
        if k == 'pw_poses':
            got, ref = grads[k], ref
        else:
            got, ref = torch.cat([g.flatten() for g in _stacked(scene, grads, k)]), torch.cat([r.flatten() for r in ref])     # images of several sizes
        err = rel(got, ref)
        print(name, k, f'{err:.2e}')
        assert err < 3e-4, (k, err)


def test_mixed_area_fixture_tells_the_two_weightings_apart(gpu):
    """The images of the mixed-size fixture have different areas (384 and 768 pixels), so the reference's per-edge mean (1 / (E area_k)) and
    PointCloudOptimizer's weighting (1 / sum of areas) give different losses there: the parity above pins D3R_ALIGNER_OPT_EDGE_MEAN_LOSS."""
    from dust3r_amd.cloud_opt import GlobalAlignerMode, global_aligner
    case = next(c for c in _gold('aligner_modular_grads.pt')['cases'] if c['name'] == 'mixed_sizes')
    modular = _modular(gpu, _output(case))
    modular.load_state_dict(case['state'])
    pco = global_aligner(_output(case), gpu, mode=GlobalAlignerMode.PointCloudOptimizer, verbose=False)
    pco.load_state_dict({k: getattr(modular, '_flat_' + k) for k in ('im_poses', 'im_depthmaps', 'im_focals', 'im_pp')}
                        | {k: getattr(modular, k).data for k in ('pw_poses', 'pw_adaptors')})
    l_mod, l_pco = float(modular()), float(pco())
    print(f'mixed areas: per-edge-mean loss {l_mod:.6f} (reference {case["loss"]:.6f}), sum-of-areas weighting {l_pco:.6f}')
    assert abs(l_mod / case['loss'] - 1) < 1e-5
    assert abs(l_pco / case['loss'] - 1) > 1e-2


def _trace_scene(gpu, g):
    scene = _modular(gpu, synthetic_scene(**g['scene_args'])[0], **g['kw'])
    scene.load_state_dict(g['start_state'])
    scene.preset_pose(g['known_poses'], g['pose_msk'])
    scene.preset_focal(g['known_focals'], g['focal_msk'])
    return scene


def test_partial_presets_trace_matches_reference(gpu):
    """300 cosine iterations with the poses of images 0 and 2 and the focal of image 1 preset (fx_and_fy) against the reference's trace:
    early losses tight, end state at test_reference_golden_trace's tolerances. Frozen entries are bit-unchanged, trainable ones move."""
    g = _gold('aligner_modular_trace.pt')
    scene = _trace_scene(gpu, g)
    assert {k: [p.requires_grad for p in getattr(scene, k)] for k in g['masks']} == g['masks']
    assert scene.norm_pw_scale is False and g['norm_pw_scale'] is False
    # the presets write what the reference's presets write (rotmat -> quaternion in fp32: 1e-6), then the recorded start is loaded bit for bit
    for i in g['pose_msk']:
        assert float((scene.im_poses[i].detach().cpu() - g['preset_state'][f'im_poses.{i}']).abs().max()) < 1e-5
    scene.load_state_dict(g['preset_state'])
    loss0, grads = scene.loss_and_grads()
    assert abs(float(loss0) / g['loss0'] - 1) < 1e-5
    for k in ('im_poses', 'im_focals'):
        got = torch.stack([gr for gr, r in zip(_stacked(scene, grads, k), g['grads0'][k]) if r is not None])
        ref = torch.stack([r for r in g['grads0'][k] if r is not None])
        assert rel(got, ref) < 3e-4, k
    before = {k: v.clone() for k, v in scene.state_dict().items()}
    from dust3r_amd.cloud_opt.base_opt import global_alignment_loop
    final = global_alignment_loop(scene, lr=0.01, niter=g['niter'], schedule='cosine')
    after = scene.state_dict()
    for i, frozen in enumerate(not m for m in g['masks']['im_poses']):
        same = torch.equal(after[f'im_poses.{i}'], before[f'im_poses.{i}'])
        assert same == frozen, (i, frozen)
    for i, frozen in enumerate(not m for m in g['masks']['im_focals']):
        same = torch.equal(after[f'im_focals.{i}'], before[f'im_focals.{i}'])
        assert same == frozen, (i, frozen)
    assert all(torch.equal(after[f'im_pp.{i}'], before[f'im_pp.{i}']) for i in range(scene.n_imgs))
    print(f'modular trace: final loss {final:.6f} vs reference {g["final_loss"]:.6f}')
    assert abs(final / g['final_loss'] - 1) < 5e-3
    assert float((scene.get_im_poses().cpu() - g['im_poses']).abs().max()) < 5e-3
    assert scene.get_focals().shape == g['focals'].shape == (4, 2)
    assert float((scene.get_focals().cpu() / g['focals'] - 1).abs().max()) < 5e-3


def test_early_iterations_track_reference(gpu):
    """The first 20 losses of the partial-preset trace, one iteration per engine call."""
    from dust3r_amd._lib import check, current_stream, lib, ptr
    g = _gold('aligner_modular_trace.pt')
    scene = _trace_scene(gpu, g)
    scene.load_state_dict(g['preset_state'])
    eng = scene._ensure_engine()
    check(lib.d3r_aligner_set_option(eng, 2, 0), 'reset adam')
    losses = torch.empty(20, dtype=torch.float32, device=scene.device)
    check(lib.d3r_aligner_run(eng, 20, 0, g['niter'], 0.01, 1e-6, 0, ptr(losses), current_stream()), 'aligner_run')
    err = float((losses.cpu().double() / g['losses'][:20].double() - 1).abs().max())
    print(f'first 20 losses: max rel err {err:.2e}')
    assert err < 1e-4


def test_norm_pw_scale_follows_known_poses(gpu):
    g = _gold('aligner_modular_trace.pt')
    out = synthetic_scene(**g['scene_args'])[0]
    for n_known, expect in ((0, True), (1, True), (2, False), (3, False)):
        scene = _modular(gpu, out)
        if n_known:
            scene.preset_pose(g['known_poses'][[0] * n_known], list(range(n_known)))
        assert scene.norm_pw_scale is expect, n_known
        assert [p.requires_grad for p in scene.im_poses] == [i >= n_known for i in range(scene.n_imgs)]


def test_mst_init_with_two_known_poses(gpu):
    """init='mst' with the poses of images 0 and 3 known, on a scene that converges (reference: 0.0086 -> 0.0076): the known poses are bit-unchanged
    by the init and the loop, the start is within the PnP tolerance of the existing bootstrap test (2 %), the end loss within 1 % and the end poses
    within 5e-3 of the reference's."""
    g = _gold('aligner_modular_mst.pt')
    scene = _modular(gpu, synthetic_scene(**g['scene_args'])[0])
    scene.preset_pose(g['known_poses'], g['pose_msk'])
    preset = torch.stack([p.detach().clone() for p in scene.im_poses])
    from dust3r_amd.cloud_opt import init_im_poses
    init_im_poses.init_minimum_spanning_tree(scene, niter_PnP=10)
    poses = torch.stack([p.detach().clone() for p in scene.im_poses])
    for i in g['pose_msk']:
        assert torch.equal(poses[i], preset[i]), i                   # known poses: bit-unchanged by the init
    loss = float(scene())
    print(f'modular mst: init loss {loss:.5f} (reference {g["init_loss"]:.5f}), '
          f'init poses {float((scene.get_im_poses().cpu() - g["init_poses"]).abs().max()):.2e} from the reference\'s')
    assert abs(loss / g['init_loss'] - 1) < 0.02
    final = scene.compute_global_alignment(init=None, niter=g['niter'], schedule='cosine', lr=0.01)
    for i in g['pose_msk']:
        assert torch.equal(scene.im_poses[i].detach(), preset[i])
    err = float((scene.get_im_poses().cpu() - g['final_poses']).abs().max())
    print(f'modular mst: final loss {final:.5f} (reference {g["final_loss"]:.5f}), end poses {err:.2e} from the reference\'s')
    assert abs(final / g['final_loss'] - 1) < 1e-2
    assert err < 5e-3


def test_loop_from_the_reference_mst_start(gpu):
    """The 100 iterations after the reference's own MST start (its state recorded in the fixture): the same loop from the same bits. The end poses are
    held to 5e-3; the reference's fp32 loop itself ends 1.25e-3 from the same loop evaluated in fp64 (recorded as fp32_vs_fp64_final_poses)."""
    from dust3r_amd.cloud_opt.base_opt import global_alignment_loop
    g = _gold('aligner_modular_mst.pt')
    scene = _modular(gpu, synthetic_scene(**g['scene_args'])[0])
    scene.preset_pose(g['known_poses'], g['pose_msk'])
    scene.load_state_dict(g['init_state'])
    assert abs(float(scene()) / g['init_loss'] - 1) < 1e-5
    final = global_alignment_loop(scene, lr=0.01, niter=g['niter'], schedule='cosine')
    err = float((scene.get_im_poses().cpu() - g['final_poses']).abs().max())
    print(f'loop from the reference mst start: final loss {final:.6f} (reference {g["final_loss"]:.6f}), end poses {err:.2e} '
          f'(reference fp32 vs fp64: {g["fp32_vs_fp64_final_poses"]:.2e})')
    assert abs(final / g['final_loss'] - 1) < 5e-3
    assert err < 5e-3


def test_compute_global_alignment_mst_entry_point(gpu):
    g = _gold('aligner_modular_mst.pt')
    scene = _modular(gpu, synthetic_scene(**g['scene_args'])[0])
    scene.preset_pose(g['known_poses'], g['pose_msk'])
    final = scene.compute_global_alignment(init='mst', niter=g['niter'], schedule='cosine', lr=0.01)
    assert abs(final / g['final_loss'] - 1) < 1e-2
    assert float((scene.get_im_poses().cpu() - g['final_poses']).abs().max()) < 5e-3


def test_pose_step_kernels_agree_modular(gpu):
    """The one-image-per-thread and strided-loop pose / focal steps in the Modular configuration (fx_and_fy, optimize_pp, partial masks).
    As in test_pose_step_kernels_agree the two runs end on the same bits: the same last loss, torch.equal on every entry of the state."""
    from dust3r_amd._lib import check, lib
    from dust3r_amd.cloud_opt.base_opt import global_alignment_loop
    g = _gold('aligner_modular_trace.pt')
    gen = torch.Generator().manual_seed(9)
    pp = 0.2 * torch.randn((4, 2), generator=gen)
    results = []
    for generic in (0, 1):
        scene = _modular(gpu, synthetic_scene(**g['scene_args'])[0], fx_and_fy=True, optimize_pp=True)
        scene.load_state_dict(g['start_state'])
        scene.load_state_dict({'im_pp': pp})
        scene.preset_pose(g['known_poses'], g['pose_msk'])
        scene.preset_focal(g['known_focals'], g['focal_msk'])
        scene.preset_principal_point([torch.tensor([16.5, 12.5])], [3])
        check(lib.d3r_aligner_set_option(scene._ensure_engine(), 5, generic), 'set_option(generic small kernel)')
        loss, grads = scene.loss_and_grads()
        last = global_alignment_loop(scene, lr=0.01, niter=10, schedule='cosine', lr_min=1e-6)
        results.append((float(loss), {k: v.clone() for k, v in grads.items()}, last, {k: v.clone() for k, v in scene.state_dict().items()}))
    (l0, g0, e0, s0), (l1, g1, e1, s1) = results
    assert abs(l0 / l1 - 1) < 1e-6 and abs(e0 / e1 - 1) < 1e-5
    for k in g0:
        assert rel(g0[k], g1[k]) < 1e-5, k
    for k in s0:
        assert rel(s0[k], s1[k]) < 1e-5, k
    assert e0 == e1, (e0, e1)
    for k in s0:
        assert torch.equal(s0[k], s1[k]), k
    assert torch.equal(s0['im_pp.3'], s1['im_pp.3']) and not torch.equal(s0['im_pp.0'], pp[0].to(s0['im_pp.0'].device))


def test_preset_after_run_rebinds_engine(gpu):
    g = _gold('aligner_modular_trace.pt')
    scene = _modular(gpu, synthetic_scene(**g['scene_args'])[0], fx_and_fy=True)
    scene.load_state_dict(g['start_state'])
    scene.compute_global_alignment(init=None, niter=5, schedule='cosine', lr=0.01)
    scene.preset_focal([40.0], [2])
    f2 = scene.im_focals[2].detach().clone()
    scene.compute_global_alignment(init=None, niter=5, schedule='cosine', lr=0.01)
    assert torch.equal(scene.im_focals[2].detach(), f2)


def test_group_and_known_poses_init_raise(gpu):
    g = _gold('aligner_modular_mst.pt')
    scene = _modular(gpu, synthetic_scene(**g['scene_args'])[0])
    with pytest.raises(NotImplementedError):
        scene.compute_global_alignment(init=None, niter=5, group=True)
    scene.preset_pose(g['known_poses'], g['pose_msk'])
    with pytest.raises(NotImplementedError):
        scene.compute_global_alignment(init='known_poses', niter=5)


def test_engine_refuses_split_step_in_modular_mode(gpu):
    from dust3r_amd._lib import current_stream, lib
    g = _gold('aligner_modular_mst.pt')
    scene = _modular(gpu, synthetic_scene(**g['scene_args'])[0])
    eng = scene._ensure_engine()
    assert lib.d3r_aligner_step_begin(eng, 0, 0, 10, 0.01, 1e-6, 0, current_stream()) == -1
    assert lib.d3r_aligner_step_end(eng, 0, 0, 10, 0.01, 1e-6, 0, current_stream()) == -1


def test_clean_pointcloud_fx_and_fy_matches_reference(gpu):
    """clean_pointcloud() of an fx_and_fy scene (d3r_clean_pointcloud reads the full K) against the reference's clean_pointcloud on the same
    state. fp32 projections in another association order can flip a rounded pixel index at an exact .5, so a vanishing fraction may differ."""
    g = _gold('aligner_modular_trace.pt')
    scene = _modular(gpu, synthetic_scene(**g['scene_args'])[0], **g['kw'])
    # the reference's confidences as they were before its clean_pointcloud call (im_conf.* of its state): the comparisons of confidences
    # are exact, so both sides start from the same bits
    scene.load_state_dict(g['clean_state'] | {f'im_conf.{i}': c for i, c in enumerate(g['clean_conf0'])})
    before = [c.clone() for c in scene.im_conf]
    scene.clean_pointcloud()
    changed = sum(int((a != b).sum()) for a, b in zip(before, scene.im_conf))
    diff = sum(int((r != c.cpu()).sum()) for r, c in zip(g['clean_conf'], scene.im_conf))
    total = sum(c.numel() for c in before)
    print(f'clean_pointcloud fx_and_fy: {changed} clipped here, {g["clean_changed"]} by the reference, {diff} of {total} differ')
    assert g['clean_changed'] > 0 and diff <= max(2, total // 5000)
