"""GPU parity of PointCloudOptimizer on the fused aligner (csrc/aligner.hip) OUTSIDE the default setting that tests/test_aligner_gpu.py
pins: dist='l2' (aligner_main_kernel<L2 = true, MODULAR = false>), conf='sqrt' | 'id' | 'm1', norm_pw_scale=False (what preset_pose
leaves), images of several sizes, images with more incident edge sides than one batch of the edge walk (EBATCH = 64), and every arm of
the pose / focal step's dispatch (launch_small: one edge per thread at 256 or 1024 threads, the strided-loop kernel above that).

The arbiter is oracle/aligner_ref.py in fp64 autograd on the CPU, evaluated here; tests/golden/aligner_pco_options.pt (the unmodified
reference class in fp32, tools/make_pco_golden.py) stands next to it. The bars are those of the existing aligner tests:
  loss 1e-5, every gradient 5e-5 (max-abs over max-abs) against fp64      test_loss_and_gradients_match_autograd
  gradients 3e-4 against the reference's fp32 golden                       test_reference_golden_trace / test_modular_aligner_gpu
  after 20 cosine iterations at lr = 0.01 against the fp32 oracle: loss 1e-3, poses / depth 2e-3, focals 1e-4
                                                                          test_short_trajectory_matches_oracle
  two kernels for one step: loss 1e-6, gradients / state 1e-5,             test_pose_step_kernels_agree
  and the same bits after the iterations
fp32 autograd itself sits at most 5.9e-6 from fp64 on these scenes, so 5e-5 is the same ~10x margin the existing tests carry; the one
exception is the gradient of the (frozen) im_poses on the 200-image scene with every pose preset, where fp32 autograd is 1.2e-5 from
fp64 and so is the engine.
"""
import os
import sys

import pytest
import torch

from dust3r_amd.synthetic import synthetic_scene

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

GROUPS = ('pw_poses', 'im_poses', 'im_depthmaps', 'im_focals')
ALL_GROUPS = GROUPS + ('pw_adaptors', 'im_pp')
CASES = ['l2', 'conf_sqrt', 'conf_id', 'conf_m1', 'preset_all', 'preset_pose_only', 'preset_all_adaptors', 'mixed_sizes', 'mixed_sizes_l2', 'oneref_70']
_cache = {}


def _case(name):
    if 'gold' not in _cache:
        _cache['gold'] = torch.load(os.path.join(GOLD, 'aligner_pco_options.pt'), weights_only=False)
    return next(c for c in _cache['gold']['cases'] if c['name'] == name)


def rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def _pco(gpu, out, **kw):
    from dust3r_amd.cloud_opt import GlobalAlignerMode, global_aligner
    return global_aligner(out, gpu, mode=GlobalAlignerMode.PointCloudOptimizer, verbose=False, **kw)


def _case_scene(gpu, case, out):
    """The scene of a golden case: constructor keywords, the presets the reference ran, then the recorded state bit for bit."""
    scene = _pco(gpu, out, **case['kw'])
    if case['preset']:
        scene.preset_pose(list(case['known_poses']))
        # the preset writes what the reference's preset wrote (rotation matrix -> quaternion in fp32)
        assert float((scene.im_poses.detach().cpu() - case['state']['im_poses']).abs().max()) < 1e-5
    if case['known_focals'] is not None:
        scene.preset_focal(case['known_focals'])
        assert float((scene.im_focals.detach().cpu() - case['state']['im_focals']).abs().max()) < 1e-5
    scene.load_state_dict(case['state'])
    assert scene.norm_pw_scale is case['norm_pw_scale']
    assert sorted(scene.trainable_names()) == sorted(case['trainable'])
    return scene


def _check_against_fp64(tag, scene, out, state, **kw):
    """One evaluation against fp64 autograd: the loss and the gradient of every group the engine exports (all six, frozen or not: the
    oracle differentiates them all the same), then forward() == the loss. Returns (loss, grads) of the engine."""
    from oracle.aligner_ref import AlignerRef
    ref = AlignerRef(out, dtype=torch.float64, **kw).load_state(state, optimize_pp=True, allow_pw_adaptors=True)
    loss_ref, g_ref = ref.grads()
    loss, g = scene.loss_and_grads()
    errs = {k: rel(g[k].reshape(g_ref[k].shape), g_ref[k]) for k in ALL_GROUPS}
    e_loss = abs(float(loss) / loss_ref - 1)
    print(f'{tag}: vs fp64 loss {e_loss:.2e}  ' + '  '.join(f'{k} {v:.2e}' for k, v in errs.items()))
    assert e_loss < 1e-5, (tag, float(loss), loss_ref)
    for k, v in errs.items():
        assert v < 5e-5, (tag, k, v)
    assert abs(float(scene()) / loss_ref - 1) < 1e-5, tag
    return loss, g


def _check_trajectory(tag, scene, ref32, ref_losses, last):
    """The end of a short Adam run against the fp32 oracle's torch-Adam run of the same length."""
    st = ref32.state()
    errs = {k: rel(getattr(scene, k).data, st[k]) for k in GROUPS + (('pw_adaptors',) if scene.pw_adaptors.requires_grad else ())}
    e_loss = abs(last / ref_losses[-1] - 1)
    print(f'{tag}: after {len(ref_losses)} iterations vs the fp32 oracle: loss {e_loss:.2e}  ' + '  '.join(f'{k} {v:.2e}' for k, v in errs.items()))
    assert e_loss < 1e-3, (tag, last, ref_losses[-1])
    assert errs['im_poses'] < 2e-3 and errs['pw_poses'] < 2e-3 and errs['im_depthmaps'] < 2e-3 and errs['im_focals'] < 1e-4, (tag, errs)
    assert errs.get('pw_adaptors', 0.0) < 2e-3, (tag, errs)         # test_principal_point_and_adaptor_parameters' bar
    assert ref_losses[-1] < 0.98 * ref_losses[0], tag             # the run went somewhere


# ---- a. the option matrix ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', CASES)
def test_option_loss_and_gradients(gpu, name):
    """Every case of aligner_pco_options.pt through global_aligner(..., mode=PointCloudOptimizer): loss and gradients against fp64 autograd
    and against the unmodified reference's fp32 values, forward() == the loss, and -- on the oracle alone -- the option is not a no-op: the
    loss at the same state under the defaults differs by more than 1e-2 (for images of several sizes: under the Modular scene's per-edge
    mean, and under one area for all images; for the un-normalised adaptors also: with the adaptors centred by hand). All cases have at most 138 edges and images: the step runs in aligner_small1_kernel<256>."""
    from test_oracle_pins import pco_case_oracle
    case = _case(name)
    ref64, out = pco_case_oracle(case, torch.float64)
    scene = _case_scene(gpu, case, out)
    kw = {k: v for k, v in case['kw'].items() if k in ('dist', 'conf')} | dict(norm_pw_scale=case['norm_pw_scale'])
    loss, g = _check_against_fp64(name, scene, out, case['state'], **kw)
    e_loss = abs(float(loss) / case['loss'] - 1)
    errs = {k: rel(g[k].reshape(r.shape), r) for k, r in case['grads'].items()}
    print(f'{name}: vs the reference fp32 golden: loss {e_loss:.2e}  ' + '  '.join(f'{k} {v:.2e}' for k, v in errs.items()))
    assert e_loss < 1e-5
    for k, v in errs.items():
        assert v < 3e-4, (name, k, v)
    with torch.no_grad():
        l_opt = float(ref64.loss())
        if case['scene'] == 'synthetic_mixed_scene':
            others = {'per-edge mean': float(ref64.edge_mean_loss())}
            ref64.total_area_i = ref64.total_area_j = len(ref64.edges) * ref64.A
            others['one area for all images'] = float(ref64.loss())
            areas = torch.tensor([h * w for h, w in scene.imshapes])
            pad = torch.arange(scene.max_area)[None, :] >= areas[:, None]
            assert int(pad.sum()) > 0 and not bool(g['im_depthmaps'].cpu()[pad].any())        # zero weight: exactly zero gradient in the padding
        elif name == 'oneref_70':
            others = {}                                                                       # the defaults on another graph: nothing to tell apart
        else:
            others = {'defaults': float(pco_case_oracle(case, torch.float64, dist='l1', conf='log', norm_pw_scale=True)[0].loss())}
            if name == 'preset_all_adaptors':       # ... and the adaptors alone: the same state with (a0, a0, a1) centred by hand
                a = case['state']['pw_adaptors']
                centred = dict(case, state=dict(case['state'], pw_adaptors=a - ((2 * a[:, 0] + a[:, 1]) / 3)[:, None]))
                others['centred adaptors'] = float(pco_case_oracle(centred, torch.float64)[0].loss())
    for what, l_other in others.items():
        print(f'{name}: oracle loss {l_opt:.6f}, under {what} {l_other:.6f} (ratio {l_opt / l_other:.3f})')
        assert abs(l_opt / l_other - 1) > 1e-2, (name, what)


# ---- b. short trajectories ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['l2', 'preset_all', 'preset_all_adaptors', 'mixed_sizes'])
def test_option_short_trajectory(gpu, name):
    """20 cosine iterations at lr = 0.01 from the golden state: the loss of EVERY iteration (d3r_aligner_run's history) against the fp32
    oracle's torch-Adam run and against the unmodified reference's recorded losses, the end state against the oracle's. Frozen groups are
    bit-unchanged; in the mixed-size scene the padded log-depths are still exactly 0.0 (zero weight, zero gradient, no Adam step) and the
    getters return the per-image shapes."""
    from dust3r_amd._lib import check, current_stream, lib, ptr
    from test_oracle_pins import pco_case_oracle
    case = _case(name)
    ref32, out = pco_case_oracle(case)
    ref_losses = ref32.run(niter=20, lr=0.01, schedule='cosine', lr_min=1e-6)
    scene = _case_scene(gpu, case, out)
    eng = scene._ensure_engine()
    check(lib.d3r_aligner_set_option(eng, 2, 0), 'reset adam')
    losses = torch.empty(20, dtype=torch.float32, device=gpu)
    check(lib.d3r_aligner_run(eng, 20, 0, 20, 0.01, 1e-6, 0, ptr(losses), current_stream()), 'aligner_run')
    hist = losses.cpu().tolist()
    e_or = max(abs(hist[i] / ref_losses[i] - 1) for i in range(20))
    e_gold = max(abs(hist[i] / float(case['losses'][i]) - 1) for i in range(20))
    print(f'{name}: 20 per-iteration losses: vs the fp32 oracle {e_or:.2e}, vs the reference golden {e_gold:.2e}')
    assert e_or < 1e-3 and e_gold < 1e-3
    _check_trajectory(name, scene, ref32, ref_losses, hist[-1])
    for k in ('im_poses', 'im_focals', 'im_pp', 'pw_adaptors'):
        moved = not torch.equal(getattr(scene, k).data.cpu(), case['state'][k])
        assert moved == (k in case['trainable']), (name, k)
    assert not torch.equal(scene.pw_poses.data.cpu(), case['state']['pw_poses'])
    assert [tuple(p.shape) for p in scene.get_pts3d()] == [hw + (3,) for hw in scene.imshapes]
    assert [tuple(d.shape) for d in scene.get_depthmaps()] == [tuple(hw) for hw in scene.imshapes]
    if name == 'mixed_sizes':
        assert len(set(scene.imshapes)) == 2
        areas = torch.tensor([h * w for h, w in scene.imshapes])
        pad = torch.arange(scene.max_area)[None, :] >= areas[:, None]
        assert int(pad.sum()) == 2 * 384 and bool((scene.im_depthmaps.data.cpu()[pad] == 0.0).all())


# ---- c. graph shapes: the edge walk's batches and the dispatch of the pose / focal step --------------------------------------------
_scenes = {}


def _graph_scene(n, H, W, graph, sym):
    key = (n, H, W, graph, sym)
    if key not in _scenes:
        _scenes.clear()                                    # one scene at a time (the largest holds 1122 edges of 1056 pixels)
        _scenes[key] = synthetic_scene(n, H, W, seed=n, scene_graph=graph, symmetrize=sym)
    return _scenes[key]


def _run_arm(gpu, tag, out, state, generic, presets=None, niter=10, **kw):
    """One evaluation and `niter` Adam iterations with the pose / focal step's dispatch left alone or pinned to the strided-loop kernel.
    Returns (scene, the state the run started from -- with what the presets wrote --, loss, gradients, last loss)."""
    from dust3r_amd import _lib
    from dust3r_amd._lib import check, lib
    from dust3r_amd.cloud_opt.base_opt import global_alignment_loop
    scene = _pco(gpu, out, **{k: v for k, v in kw.items() if k != 'norm_pw_scale'})
    scene.load_state_dict(state)
    if presets is not None:
        scene.preset_pose(list(presets[0]))
        scene.preset_focal(presets[1])
    start = {k: getattr(scene, k).detach().cpu().clone() for k in ('pw_poses', 'pw_adaptors', 'im_poses', 'im_depthmaps', 'im_focals', 'im_pp')}
    check(lib.d3r_aligner_set_option(scene._ensure_engine(), _lib.ALIGNER_OPT_GENERIC_SMALL, int(generic)), 'set_option(generic small kernel)')
    if generic:
        loss, g = scene.loss_and_grads()
    else:
        loss, g = _check_against_fp64(tag, scene, out, start, **kw)
    last = global_alignment_loop(scene, lr=0.01, niter=niter, schedule='cosine', lr_min=1e-6)
    return scene, start, float(loss), {k: v.clone() for k, v in g.items()}, last


_arm_results = {}


def _graph_arm(gpu, arm):
    """Everything that is asserted about one arm of ARMS except the agreement of the two step kernels after the iterations; that
    comparison's figures are returned (and kept for the test that asserts them)."""
    if arm in _arm_results:
        return _arm_results[arm]
    from oracle.aligner_ref import AlignerRef
    (n, H, W, graph, sym), spec = ARMS[arm][0], dict(ARMS[arm][1])
    n_edges, busiest = spec.pop('n_edges'), spec.pop('busiest')
    natural_is_generic, preset, kw = spec.pop('natural_is_generic', False), spec.pop('preset', False), spec
    out, init, gt = _graph_scene(n, H, W, graph, sym)
    tag = arm
    state, presets, frozen = init, None, ()
    if preset:          # as the golden's preset_all: known cameras in the start state's world, every pairwise scale raised by 0.3
        poses = gt['cam2world'].clone()
        poses[:, :3, 3] *= gt['world_scale']
        presets, frozen = (poses, [float(gt['focal'])] * n), ('im_poses', 'im_focals')
        kw = dict(kw, norm_pw_scale=False)
        state = dict(init, pw_poses=init['pw_poses'].clone())
        state['pw_poses'][:, 7] += 0.3
    (scene, state, loss, g, last), (scene_g, _, loss_g, g_g, last_g) = [_run_arm(gpu, tag, out, state, generic, presets=presets, **kw)
                                                                         for generic in (False, True)]
    assert scene.norm_pw_scale is (not preset)
    assert scene.n_edges == n_edges
    sides = [0] * n
    for i, j in scene.edges:
        sides[i] += 1
        sides[j] += 1
    assert max(sides) == busiest, max(sides)
    ref32 = AlignerRef(out, **kw).load_state(state, frozen=frozen)
    ref_losses = ref32.run(niter=10, lr=0.01, schedule='cosine', lr_min=1e-6)
    _check_trajectory(tag, scene, ref32, ref_losses, last)
    if preset:
        assert torch.equal(scene.im_poses.data.cpu(), state['im_poses']) and torch.equal(scene.im_focals.data.cpu(), state['im_focals'])
    # the same evaluation with the strided-loop kernel pinned
    e_g = {k: rel(g[k], g_g[k]) for k in g}
    print(f'{tag}: natural dispatch vs strided-loop kernel, one evaluation: loss {abs(loss / loss_g - 1):.1e}  ' + '  '.join(f'{k} {v:.1e}' for k, v in e_g.items()))
    assert abs(loss / loss_g - 1) < 1e-6
    assert max(e_g.values()) < 1e-5, e_g
    if natural_is_generic:              # the same kernel twice: fixed-order sums, so the same bits
        assert loss == loss_g and all(torch.equal(g[k], g_g[k]) for k in g)
    # ... and after the 10 iterations: the figures test_graph_arm_step_kernels_agree_after_iterations asserts
    e_s = {k: rel(getattr(scene, k).data, getattr(scene_g, k).data) for k in GROUPS}
    d = (scene.im_depthmaps.data - scene_g.im_depthmaps.data).abs()
    off = int((d > 1e-5 * float(scene_g.im_depthmaps.data.abs().max())).sum())
    st32 = ref32.state()
    res = dict(scene=scene, out=out, init=init, end_loss=abs(last / last_g - 1), end_state=e_s, depth_beyond=off, depth_total=d.numel(),
               oracle_depth=rel(scene.im_depthmaps.data, st32['im_depthmaps']), last=(last, last_g),
               end_equal={k: torch.equal(getattr(scene, k).data, getattr(scene_g, k).data) for k in ALL_GROUPS})
    _arm_results[arm] = res            # the largest scene holds 40 MB on the device
    return res


# The smallest scenes that reach each arm: synthetic_scene(n, H, W, seed=n, scene_graph, symmetrize). 8 x 12 = 96 pixels is one workgroup
# per image with 24 active threads and three idle waves. The test cannot observe which kernel ran: the rule is launch_small's
# (need = max(E, n): <= 256 aligner_small1_kernel<256>, <= 1024 aligner_small1_kernel<1024>, above that the strided-loop aligner_small_kernel).
ARMS = {
    # oneref, not symmetrised: image 0 has 64 incident edge sides -- one batch of the edge walk, exactly full. need = 65: small1<256>
    'oneref n=65': ((65, 8, 12, 'oneref', False), dict(n_edges=64, busiest=64)),
    # 65 sides: a second batch of ONE edge (sh_es / sh_part reused across the barrier, g[k] carried over). need = 66: small1<256>
    'oneref n=66': ((66, 8, 12, 'oneref', False), dict(n_edges=65, busiest=65)),
    # the golden's oneref_70: image 0 walks 138 sides in three batches (64 + 64 + 10). need = 138: small1<256>
    'oneref sym n=70': ((70, 8, 12, 'oneref', True), dict(n_edges=138, busiest=138)),
    # E = 256: the last size of small1<256>, every thread owns an edge
    'oneref sym n=129': ((129, 8, 12, 'oneref', True), dict(n_edges=256, busiest=256)),
    # E = 258: the first size of small1<1024>
    'oneref sym n=130': ((130, 8, 12, 'oneref', True), dict(n_edges=258, busiest=258)),
    # E = 256 would fit 256 threads, n = 257 does not: need = max(E, n) = 257 selects small1<1024>, whose last image thread has no edge
    'oneref n=257': ((257, 8, 12, 'oneref', False), dict(n_edges=256, busiest=256)),
    # 870 edges, 58 sides on every image (one batch). need = 870: small1<1024>
    'complete sym n=30': ((30, 8, 12, 'complete', True), dict(n_edges=870, busiest=58)),
    # image 0 walks 398 sides in 7 batches (6 x 64 + 14). need = 398: small1<1024>
    'oneref sym n=200': ((200, 8, 12, 'oneref', True), dict(n_edges=398, busiest=398)),
    # the same with every pose and focal preset: norm_pw_scale False, every pairwise scale raised by 0.3 (as the golden's preset_all)
    'oneref sym n=200 preset_all': ((200, 8, 12, 'oneref', True), dict(n_edges=398, busiest=398, preset=True)),
    # E = 1024: the last size of small1<1024>; image 0 walks 16 full batches
    'oneref sym n=513': ((513, 8, 12, 'oneref', True), dict(n_edges=1024, busiest=1024)),
    # E = 1026: the first size the dispatch itself sends to the strided-loop aligner_small_kernel; 16 batches and one of two edges
    'oneref sym n=514': ((514, 8, 12, 'oneref', True), dict(n_edges=1026, busiest=1026, natural_is_generic=True)),
    # 24 x 44: 1122 edges -> aligner_small_kernel by dispatch; 66 sides per image -> two batches (64 + 2); 1056 pixels -> two workgroups per
    # image, the second with 32 pixels (8 active threads)
    'complete sym n=34 24x44': ((34, 24, 44, 'complete', True), dict(n_edges=1122, busiest=66, natural_is_generic=True)),
    'complete sym n=34 24x44 l2': ((34, 24, 44, 'complete', True), dict(n_edges=1122, busiest=66, natural_is_generic=True, dist='l2')),
}


@pytest.mark.parametrize('arm', list(ARMS))
def test_graph_arm_matches_oracles(gpu, arm):
    """Every arm of ARMS (the comment of each entry names the batches of the edge walk and the launch_small arm its sizes select): one
    evaluation against fp64 autograd, 10 Adam iterations against the fp32 oracle's torch-Adam run, and the same evaluation with
    D3R_ALIGNER_OPT_GENERIC_SMALL pinned: loss 1e-6, every gradient 1e-5, as test_pose_step_kernels_agree -- bit for bit where the
    dispatch takes the strided-loop kernel by itself. Preset groups are bit-unchanged by the iterations."""
    _graph_arm(gpu, arm)


@pytest.mark.parametrize('arm', list(ARMS))
def test_graph_arm_step_kernels_agree_after_iterations(gpu, arm):
    """The second half of test_pose_step_kernels_agree on every arm: after the 10 Adam iterations the run with the natural dispatch and the
    run with the strided-loop kernel pinned agree to 1e-5 in the last loss and in every parameter group.

    This is the test that found the step's two kernels rounding differently: with quat_to_rotmat and the Adam update contracted into FMAs
    one way in aligner_small1_kernel and another way in aligner_small_kernel, their first evaluations agreed to 1e-6 but not in the bits,
    and after 10 iterations ONE log-depth of 6240 / 6720 / 12384 ended 2.0e-5 / 1.2e-5 / 5.5e-5 apart on 'oneref n=65', 'oneref sym n=70'
    and 'oneref sym n=129' (Adam's m / sqrt(v) at a pixel whose gradient passes through zero). With contraction off in that arithmetic
    (csrc/aligner_math.hpp) the two runs agree bit for bit on all thirteen arms, and since both kernels call one set of per-edge and
    per-image functions (csrc/aligner.hip) that is asserted: the same last loss and torch.equal on all six parameter groups, on every arm."""
    r = _graph_arm(gpu, arm)
    print(f'{arm}: natural dispatch vs strided-loop kernel after 10 iterations: last loss {r["end_loss"]:.1e}  '
          + '  '.join(f'{k} {v:.1e}' for k, v in r['end_state'].items())
          + f'  ({r["depth_beyond"]} of {r["depth_total"]} log-depths beyond 1e-5; the same run vs the fp32 oracle: im_depthmaps {r["oracle_depth"]:.1e})')
    assert r['end_loss'] < 1e-5
    assert max(r['end_state'].values()) < 1e-5, r['end_state']
    assert r['last'][0] == r['last'][1], r['last']
    assert all(r['end_equal'].values()), r['end_equal']


def test_many_batches_both_reductions(gpu):
    """The 7-batch scene (oneref symmetrised, n = 200; aligner_small1_kernel<1024>) with the DPP and the shuffle wave reduction: each
    against fp64, and against each other at test_dpp_and_shuffle_reductions_agree's bars."""
    r = _graph_arm(gpu, 'oneref sym n=200')
    scene, out, init = r['scene'], r['out'], r['init']
    scene.load_state_dict(init)
    res = []
    for dpp in (True, False):
        scene.set_reduction(dpp)
        res.append(_check_against_fp64(f'oneref sym n=200, {"dpp" if dpp else "shuffle"} reduction', scene, out, init))
    scene.set_reduction(True)
    (l1, g1), (l2, g2) = res
    assert abs(float(l1) / float(l2) - 1) < 1e-6
    for k in g1:
        assert rel(g1[k], g2[k]) < 1e-5, k


