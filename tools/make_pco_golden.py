"""Generates tests/golden/aligner_pco_options.pt by running the UNMODIFIED reference PointCloudOptimizer
(dust3r/cloud_opt/optimizer.py, through oracle/ref_import.py) on the CPU, in fp32, in the settings the default-only fixtures
(aligner_4v.pt, aligner_c4.pt) leave out.

    python tools/make_pco_golden.py

The pairwise predictions are NOT stored: they are regenerated at test time from the seeds recorded in each case
(dust3r_amd.synthetic.synthetic_scene / synthetic_mixed_scene). Stored per case: the scene arguments, the constructor keywords, what was
preset, the state the loss was evaluated at (the reference's state_dict keys: pw_poses, pw_adaptors, im_poses, im_depthmaps (n, max_area),
im_focals, im_pp), the fp32 loss, the gradient of every trainable group, and the losses of a 20-iteration cosine run from that state.

  l2, conf_sqrt, conf_id, conf_m1     dist / conf other than the defaults, 4 views of 16 x 24
  preset_all                          preset_pose + preset_focal on every image: im_poses and im_focals frozen, norm_pw_scale False
  preset_pose_only                    preset_pose alone
  preset_all_adaptors                 preset_all with allow_pw_adaptors=True and non-zero pw_adaptors: the adaptors are not centred either
  mixed_sizes, mixed_sizes_l2         three images of two areas (384 and 768 pixels): the ParameterStack(fill=max_area) path
  oneref_70                           70 images, 138 edges all incident to image 0

In the preset cases every pw_poses[:, 7] of synthetic_scene's start is raised by 0.3 first: that start has mean_e pw_poses[e, 7] within
0.2 % of log(base_scale), where normalising the pairwise scales changes nothing one could measure.
"""
import copy
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)

from oracle.ref_import import import_reference  # noqa: E402

import_reference()
import dust3r.cloud_opt.base_opt as ref_base  # noqa: E402
from dust3r.cloud_opt import GlobalAlignerMode, global_aligner  # noqa: E402

from dust3r_amd.synthetic import synthetic_mixed_scene, synthetic_scene  # noqa: E402

OUT = os.path.join(ROOT, 'tests', 'golden')
NAME = 'aligner_pco_options.pt'
NITER = 20
GROUPS = ('pw_poses', 'pw_adaptors', 'im_poses', 'im_depthmaps', 'im_focals', 'im_pp')
PW_SCALE_SHIFT = 0.3


def ref_scene(out, **kw):
    torch.manual_seed(0)
    return global_aligner(copy.deepcopy(out), 'cpu', mode=GlobalAlignerMode.PointCloudOptimizer, verbose=False, **kw)


def trainable_state(scene):
    st = scene.state_dict(trainable=True)
    return {k: st[k].detach().clone() for k in GROUPS}


def grads_of(scene):
    loss = scene()
    loss.backward()
    g = {k: getattr(scene, k).grad.clone() for k in GROUPS if getattr(scene, k).grad is not None}
    scene.zero_grad()
    return float(loss), g


def run_with_losses(scene, **kw):
    losses = []
    orig = ref_base.global_alignment_iter

    def spy(*a, **k):
        loss, lr = orig(*a, **k)
        losses.append(loss)
        return loss, lr
    ref_base.global_alignment_iter = spy
    try:
        scene.compute_global_alignment(init=None, **kw)
    finally:
        ref_base.global_alignment_iter = orig
    return torch.tensor(losses)


def record(name, scene_fn, scene_args, kw, scene, preset=None, known_poses=None, known_focals=None):
    state = trainable_state(scene)
    trainable = [k for k in GROUPS if getattr(scene, k).requires_grad]
    loss, grads = grads_of(scene)
    assert sorted(grads) == sorted(trainable), (name, sorted(grads), trainable)
    losses = run_with_losses(scene, niter=NITER, schedule='cosine', lr=0.01)
    print(f'{name:18s} loss {loss:.6f}  trainable {trainable}  norm_pw_scale {scene.norm_pw_scale}  loss[{NITER - 1}] {float(losses[-1]):.6f}')
    return dict(name=name, scene=scene_fn, scene_args=scene_args, kw=kw, preset=preset, known_poses=known_poses, known_focals=known_focals,
                norm_pw_scale=bool(scene.norm_pw_scale), trainable=trainable, state=state, loss=loss, grads=grads, niter=NITER, losses=losses)


def options_golden():
    cases = []
    args = dict(n_views=4, H=16, W=24, seed=4, symmetrize=True)
    out, init, gt = synthetic_scene(**args)
    for name, kw in (('l2', dict(dist='l2')), ('conf_sqrt', dict(conf='sqrt')), ('conf_id', dict(conf='id')), ('conf_m1', dict(conf='m1'))):
        scene = ref_scene(out, **kw)
        scene.load_state_dict(scene.state_dict(trainable=True) | init)
        cases.append(record(name, 'synthetic_scene', args, kw, scene))
    # presets: the ground-truth cameras in the world of the start state (synthetic_scene rescales its world by gt['world_scale'])
    known_poses = gt['cam2world'].clone()
    known_poses[:, :3, 3] *= gt['world_scale']
    known_focals = [float(gt['focal'])] * args['n_views']
    shifted = dict(init, pw_poses=init['pw_poses'].clone())
    shifted['pw_poses'][:, 7] += PW_SCALE_SHIFT
    # non-zero adaptors: with zeros, centring them (norm_pw_scale True) or not (False) gives the same exp(0)
    adaptors = dict(shifted, pw_adaptors=0.5 * torch.randn((len(out['view1']['idx']), 2), generator=torch.Generator().manual_seed(5)))
    for name, focal, kw, start in (('preset_all', True, {}, shifted), ('preset_pose_only', False, {}, shifted),
                                   ('preset_all_adaptors', True, dict(allow_pw_adaptors=True), adaptors)):
        scene = ref_scene(out, **kw)
        scene.load_state_dict(scene.state_dict(trainable=True) | start)
        scene.preset_pose([p for p in known_poses])
        if focal:
            scene.preset_focal(known_focals)
        assert scene.norm_pw_scale is False
        cases.append(record(name, 'synthetic_scene', args, kw, scene, preset='all' if focal else 'pose', known_poses=known_poses,
                            known_focals=known_focals if focal else None))
    # two image areas, the reference's own seeded random start (no consistent geometry needed for loss / gradient parity)
    margs = dict(shapes=[(16, 24), (24, 32), (16, 24)], seed=2)
    mout = synthetic_mixed_scene(**margs)
    for name, kw in (('mixed_sizes', {}), ('mixed_sizes_l2', dict(dist='l2'))):
        cases.append(record(name, 'synthetic_mixed_scene', margs, kw, ref_scene(mout, **kw)))
    # one image with 138 incident edge sides
    oargs = dict(n_views=70, H=8, W=12, seed=70, scene_graph='oneref', symmetrize=True)
    out, init, gt = synthetic_scene(**oargs)
    scene = ref_scene(out)
    scene.load_state_dict(scene.state_dict(trainable=True) | init)
    cases.append(record('oneref_70', 'synthetic_scene', oargs, {}, scene))
    return dict(kind='aligner_pco_options', pw_scale_shift=PW_SCALE_SHIFT, cases=cases)


if __name__ == '__main__':
    # one thread: the backward of proj_pts3d[_ei] adds 138 edges' gradients into image 0 (oneref_70), in thread order otherwise -- the
    # fixture is then reproduced bit for bit by a second run
    torch.set_num_threads(1)
    res = options_golden()
    torch.save(res, os.path.join(OUT, NAME))
    print('wrote', NAME, os.path.getsize(os.path.join(OUT, NAME)), 'bytes')
