"""Generates tests/golden/aligner_modular_*.pt by running the UNMODIFIED reference ModularPointCloudOptimizer
(dust3r/cloud_opt/modular_optimizer.py, through oracle/ref_import.py) on the CPU, in fp32.

    python tools/make_modular_golden.py

The pairwise predictions are NOT stored: they are regenerated at test time from the seeds recorded in each fixture
(dust3r_amd.synthetic.synthetic_scene / synthetic_mixed_scene). Stored: the parameter states in the reference's own
state_dict keys (im_poses.<i>, im_depthmaps.<i> (H, W), im_focals.<i>, im_pp.<i>; im_conf.* left out, both sides derive it
from the predictions), and what the reference computed from them.

  aligner_modular_grads.pt   (a) one loss + gradient evaluation per configuration: isotropic, fx_and_fy with fx != fy, optimize_pp,
                                 dist='l2', conf='sqrt', and a scene with two image areas (isotropic, and fx != fy)
  aligner_modular_trace.pt   (b) 300 cosine iterations with poses of images 0 and 2 and the focal of image 1 preset, fx_and_fy;
                                 plus clean_pointcloud() at the start of the loop (image 0 pulled 22 % closer so that it clips)
  aligner_modular_mst.pt     (c) init='mst' with two known poses: initial loss, state and poses after the init, poses after 100 iterations,
                                 and how far the same 100 iterations evaluated in fp64 end from those fp32 poses
"""
import copy
import math
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)

from oracle.ref_import import import_reference  # noqa: E402

import_reference()
import dust3r.cloud_opt.base_opt as ref_base  # noqa: E402
import dust3r.cloud_opt.init_im_poses as ref_init  # noqa: E402
from dust3r.cloud_opt import GlobalAlignerMode, global_aligner  # noqa: E402

from dust3r_amd.synthetic import synthetic_mixed_scene, synthetic_scene  # noqa: E402

OUT = os.path.join(ROOT, 'tests', 'golden')
FB = 20.0           # focal_brake (the reference's default)


def ref_scene(out, **kw):
    torch.manual_seed(0)
    return global_aligner(copy.deepcopy(out), 'cpu', mode=GlobalAlignerMode.ModularPointCloudOptimizer, verbose=False, **kw)


def trainable_state(scene):
    return {k: v.detach().clone() for k, v in scene.state_dict(trainable=True).items() if not k.startswith('im_conf.')}


def state_from_init(init, imshapes, fx_and_fy=False, fy_ratio=1.0, pp=None):
    """synthetic_scene's initial state (stacked tensors) in the reference Modular scene's keys."""
    st = dict(pw_poses=init['pw_poses'].clone(), pw_adaptors=init['pw_adaptors'].clone())
    for i, (H, W) in enumerate(imshapes):
        st[f'im_poses.{i}'] = init['im_poses'][i].clone()
        st[f'im_depthmaps.{i}'] = init['im_depthmaps'][i, :H * W].reshape(H, W).clone()
        fx = float(init['im_focals'][i, 0])
        st[f'im_focals.{i}'] = torch.tensor([fx, fx + FB * math.log(fy_ratio)] if fx_and_fy else [fx], dtype=torch.float32)
        st[f'im_pp.{i}'] = pp[i].clone() if pp is not None else torch.zeros(2)
    return st


def grads_of(scene):
    loss = scene()
    loss.backward()
    g = dict(pw_poses=scene.pw_poses.grad.clone())
    for name in ('im_poses', 'im_focals', 'im_pp', 'im_depthmaps'):
        params = list(getattr(scene, name))
        if any(p.grad is not None for p in params):
            g[name] = [p.grad.clone() if p.grad is not None else None for p in params]      # None: a frozen entry
    scene.zero_grad()
    return float(loss), g


def grads_golden():
    cases = []
    scene_args = dict(n_views=4, H=16, W=24, seed=1, symmetrize=True)
    out, init, gt = synthetic_scene(**scene_args)
    imshapes = [(scene_args['H'], scene_args['W'])] * scene_args['n_views']
    pp = 0.3 * torch.randn((4, 2), generator=torch.Generator().manual_seed(11))
    for name, kw, st_kw in (('isotropic', {}, {}),
                            ('fx_and_fy', dict(fx_and_fy=True), dict(fx_and_fy=True, fy_ratio=1.08)),
                            ('optimize_pp', dict(optimize_pp=True), dict(pp=pp)),
                            ('l2', dict(dist='l2'), {}),
                            ('conf_sqrt', dict(conf='sqrt'), {})):
        scene = ref_scene(out, **kw)
        state = state_from_init(init, imshapes, **st_kw)
        scene.load_state_dict(scene.state_dict(trainable=True) | state)
        loss, g = grads_of(scene)
        cases.append(dict(name=name, scene='synthetic_scene', scene_args=scene_args, kw=kw, state=state, loss=loss, grads=g))
    # two image sizes: the reference's own seeded random start (no consistent geometry needed for gradient parity)
    # the areas differ (384 and 768 pixels): only then does the per-edge mean, 1 / (E area_k), differ from PointCloudOptimizer's 1 / sum of areas
    mixed_args = dict(shapes=[(16, 24), (24, 32), (16, 24)], seed=2)
    out = synthetic_mixed_scene(**mixed_args)
    for name, kw in (('mixed_sizes', {}), ('mixed_sizes_fx_and_fy', dict(fx_and_fy=True))):
        scene = ref_scene(out, **kw)
        state = trainable_state(scene)
        if kw:                                                          # fx != fy: fy = 1.07 fx on every image
            for i in range(scene.n_imgs):
                state[f'im_focals.{i}'][1] += FB * math.log(1.07)
            scene.load_state_dict(scene.state_dict(trainable=True) | state)
        loss, g = grads_of(scene)
        cases.append(dict(name=name, scene='synthetic_mixed_scene', scene_args=mixed_args, kw=kw, state=state, loss=loss, grads=g))
    return dict(kind='aligner_modular_grads', cases=cases)


def run_with_losses(scene, **kw):
    losses = []
    orig = ref_base.global_alignment_iter

    def spy(*a, **k):
        loss, lr = orig(*a, **k)
        losses.append(loss)
        return loss, lr
    ref_base.global_alignment_iter = spy
    try:
        final = scene.compute_global_alignment(init=None, **kw)
    finally:
        ref_base.global_alignment_iter = orig
    return float(final), torch.tensor(losses)


def trace_golden(niter=300):
    scene_args = dict(n_views=4, H=24, W=32, seed=0, symmetrize=True)
    out, init, gt = synthetic_scene(**scene_args)
    imshapes = [(scene_args['H'], scene_args['W'])] * scene_args['n_views']
    scene = ref_scene(out, fx_and_fy=True)
    start = state_from_init(init, imshapes, fx_and_fy=True, fy_ratio=1.05)
    scene.load_state_dict(scene.state_dict(trainable=True) | start)
    pose_msk, focal_msk = [0, 2], [1]
    known_poses = gt['cam2world'][pose_msk].clone()
    known_focals = [float(gt['focal'])]
    scene.preset_pose(known_poses, pose_msk)
    scene.preset_focal(known_focals, focal_msk)
    preset_state = trainable_state(scene)             # the start of the loop (presets applied)
    masks = {name: [bool(p.requires_grad) for p in getattr(scene, name)] for name in ('im_poses', 'im_focals', 'im_pp')}
    loss0, grads0 = grads_of(scene)
    final, losses = run_with_losses(scene, niter=niter, schedule='cosine', lr=0.01)
    final_state = trainable_state(scene)
    res = dict(kind='aligner_modular_trace', scene_args=scene_args, kw=dict(fx_and_fy=True), start_state=start, pose_msk=pose_msk,
               known_poses=known_poses, focal_msk=focal_msk, known_focals=known_focals, preset_state=preset_state, masks=masks,
               norm_pw_scale=bool(scene.norm_pw_scale), loss0=loss0, grads0=grads0, niter=niter, losses=losses, final_loss=final,
               im_poses=scene.get_im_poses().detach().clone(), focals=scene.get_focals().detach().clone(), final_state=final_state)
    # clean_pointcloud at the start of the loop, image 0 pulled 22 % closer (its points now sit in front of the other views' depth). Not at the final
    # state: there the surfaces agree to ~1e-3, the size of clean_pointcloud's own tolerance, and fp32 rounding decides many of its comparisons
    clean_state = dict(preset_state)
    clean_state['im_depthmaps.0'] = clean_state['im_depthmaps.0'] - 0.25
    scene = ref_scene(out, fx_and_fy=True)
    scene.load_state_dict(scene.state_dict(trainable=True) | clean_state)
    with torch.no_grad():
        conf_before = [c.clone() for c in scene.im_conf]
        scene.clean_pointcloud()
    res.update(clean_state=clean_state, clean_conf0=conf_before, clean_conf=[c.detach().clone() for c in scene.im_conf],
               clean_changed=int(sum(int((a != b).sum()) for a, b in zip(conf_before, scene.im_conf))))
    return res


def mst_golden(niter=100):
    scene_args = dict(n_views=5, H=32, W=48, seed=5, symmetrize=True, noise=0.002)
    out, _, gt = synthetic_scene(**scene_args)
    scene = ref_scene(out)
    pose_msk = [0, 3]
    known_poses = gt['cam2world'][pose_msk].clone()
    scene.preset_pose(known_poses, pose_msk)
    preset_poses = torch.stack([p.detach().clone() for p in scene.im_poses])
    ref_init.init_minimum_spanning_tree(scene, niter_PnP=10)
    with torch.no_grad():
        init_loss = float(scene())
    init_poses = scene.get_im_poses().detach().clone()
    init_focals = scene.get_focals().detach().clone()
    init_state = trainable_state(scene)
    final, losses = run_with_losses(scene, niter=niter, schedule='cosine', lr=0.01)
    final_poses = scene.get_im_poses().detach().clone()
    # the reference's own fp32 rounding floor for the end poses: the same loop from the same start evaluated in fp64
    other = ref_scene(out)
    other.preset_pose(known_poses, pose_msk)
    other.load_state_dict(other.state_dict(trainable=True) | init_state)
    other = other.double()
    run_with_losses(other, niter=niter, schedule='cosine', lr=0.01)
    fp32_vs_fp64 = float((other.get_im_poses().detach() - final_poses.double()).abs().max())
    return dict(kind='aligner_modular_mst', scene_args=scene_args, pose_msk=pose_msk, known_poses=known_poses, preset_poses=preset_poses,
                init_loss=init_loss, init_poses=init_poses, init_focals=init_focals, init_state=init_state, niter=niter, final_loss=final,
                losses=losses, final_poses=final_poses, final_focals=scene.get_focals().detach().clone(), fp32_vs_fp64_final_poses=fp32_vs_fp64)


FIXTURES = {'aligner_modular_grads.pt': grads_golden, 'aligner_modular_trace.pt': trace_golden, 'aligner_modular_mst.pt': mst_golden}


if __name__ == '__main__':
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    only = sys.argv[1:]
    for fname, fn in FIXTURES.items():
        if only and fname not in only:
            continue
        res = fn()
        torch.save(res, os.path.join(OUT, fname))
        print('wrote', fname, os.path.getsize(os.path.join(OUT, fname)), 'bytes')
