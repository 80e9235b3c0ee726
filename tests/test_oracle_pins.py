"""CPU tests (-m "not gpu"): the oracle restatements against the golden vectors generated from the
UNMODIFIED reference files (tests/golden, oracle/make_golden.py): outputs of seeded runs, and the reference functions'
answers on stored inputs (tests/golden/reference_pins.pt)."""
import os

import pytest
import torch

from dust3r_amd.synthetic import MODEL_CONFIGS, OUT_GAIN, synthetic_image_list, synthetic_scene, synthetic_state_dict, synthetic_views
from oracle.aligner_ref import AlignerRef
from oracle.dust3r_ref import build_ref_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


def _g(name):
    return torch.load(os.path.join(GOLD, name), weights_only=False)


@pytest.mark.parametrize('name', ['forward_tiny_dpt.pt', 'forward_tiny_linear.pt'])
def test_forward_oracle_equals_reference_golden(name):
    g = _g(name)
    m = build_ref_model(g['config'], seed=g['weight_seed'])
    v1, v2 = synthetic_views(g['B'], g['H'], g['W'], seed=g['view_seed'])
    with torch.no_grad():
        r1, r2 = m(v1, v2)
    # same ops in the same order as the reference run that produced the fixture: bit-exact on one machine,
    # 1e-5 across BLAS builds
    for a, b in ((r1['pts3d'], g['pts3d']), (r1['conf'], g['conf']), (r2['pts3d_in_other_view'], g['pts3d_in_other_view']), (r2['conf'], g['conf2'])):
        assert a.shape == b.shape
        assert float((a - b).abs().max() / b.abs().max()) < 1e-5


def test_forward_oracle_postprocess_modes_equal_reference_golden():
    """heads/postprocess.py:23-58 modes other than the released checkpoints' (depth 'linear' / 'square', conf 'sigmoid', finite bounds):
    the oracle against the fixture the unmodified reference model produced (oracle/make_golden.py forward_modes_golden)."""
    from oracle.dust3r_ref import DUSt3RRef
    g = _g('forward_post_modes.pt')
    v1, v2 = synthetic_views(g['B'], g['H'], g['W'], seed=g['view_seed'])
    seen = set()
    for c in g['cases']:
        m = DUSt3RRef(depth_mode=c['depth_mode'], conf_mode=c['conf_mode'], **MODEL_CONFIGS[c['config']]).eval()
        m.load_state_dict(synthetic_state_dict(m.state_dict(), g['weight_seed'], OUT_GAIN[c['config']]))
        with torch.no_grad():
            r1, r2 = m(v1, v2)
        for a, b in ((r1['pts3d'], c['pts3d']), (r1['conf'], c['conf']), (r2['pts3d_in_other_view'], c['pts3d_in_other_view']), (r2['conf'], c['conf2'])):
            assert a.shape == b.shape and float((a - b).abs().max() / b.abs().max()) < 1e-5, (c['config'], c['depth_mode'], c['conf_mode'])
        seen.add((c['depth_mode'][0], c['conf_mode'][0]))
    assert {d for d, _ in seen} == {'exp', 'linear', 'square'} and {k for _, k in seen} == {'exp', 'sigmoid'}


def test_inference_structure_golden():
    """make_pairs + collate + output dict layout of the mirror == the reference's inference() golden."""
    from dust3r_amd.image_pairs import make_pairs
    from dust3r_amd.utils.device import collate_with_cat
    g = _g('inference_tiny_dpt.pt')
    imgs = synthetic_image_list(g['n_views'], g['H'], g['W'], seed=g['view_seed'])
    pairs = make_pairs(imgs, scene_graph='complete', prefilter=None, symmetrize=True)
    assert [a['idx'] for a, b in pairs] == g['idx1'] and [b['idx'] for a, b in pairs] == g['idx2']
    m = build_ref_model(g['config'])
    res = []
    for k in range(0, len(pairs), 2):
        v1, v2 = collate_with_cat(pairs[k:k + 2])
        with torch.no_grad():
            p1, p2 = m(v1, v2)
        res.append(dict(view1=v1, view2=v2, pred1=p1, pred2=p2, loss=None))
    out = collate_with_cat(res)
    assert out['view1']['idx'] == g['idx1'] and out['loss'] is None
    assert float((out['pred1']['pts3d'] - g['pts3d']).abs().max() / g['pts3d'].abs().max()) < 1e-5
    assert float((out['pred2']['conf'] - g['conf2']).abs().max()) < 1e-4


def test_aligner_oracle_against_reference_golden():
    g = _g('aligner_4v.pt')
    out, init, gt = synthetic_scene(g['n_views'], g['H'], g['W'], seed=g['seed'], symmetrize=True)
    al = AlignerRef(out).load_state(init)
    loss0, grads = al.grads()
    assert abs(loss0 - g['loss0']) < 1e-6 * abs(g['loss0']) + 1e-7
    for k, ref in g['grads'].items():
        err = float((grads[k] - ref).abs().max() / ref.abs().max())
        assert err < 2e-4, (k, err)           # same math, different fp32 op order (einsum vs matmul)
    losses = al.run(niter=g['niter'])
    ref_losses = g['losses']
    # identical trajectories early on; Adam(b2=0.9) on the un-squared norm is chaotic at the 1e-3 level later
    # (DESIGN.md "aligner parity floor"): compare the early trace tightly and the end state loosely
    assert float((torch.tensor(losses[:10]) / ref_losses[:10] - 1).abs().max()) < 1e-4
    assert abs(losses[-1] / float(ref_losses[-1]) - 1) < 2e-3
    assert float((al.im_poses().detach() - g['im_poses']).abs().max()) < 5e-3
    assert float((al.focals().detach().flatten() / g['focals'].flatten() - 1).abs().max()) < 5e-3


def pco_case_oracle(case, dtype=torch.float32, **override):
    """AlignerRef in the setting of one case of tests/golden/aligner_pco_options.pt, at the case's state. `override`: constructor
    keywords that replace the case's (the GPU tests evaluate the same state under the defaults to show that an option acts)."""
    from dust3r_amd.synthetic import synthetic_mixed_scene
    out = synthetic_mixed_scene(**case['scene_args']) if case['scene'] == 'synthetic_mixed_scene' else synthetic_scene(**case['scene_args'])[0]
    kw = {k: v for k, v in case['kw'].items() if k in ('dist', 'conf')} | dict(norm_pw_scale=case['norm_pw_scale']) | override
    frozen = tuple(k for k in ('im_poses', 'im_focals') if k not in case['trainable'])
    al = AlignerRef(out, dtype=dtype, **kw)
    return al.load_state(case['state'], frozen=frozen, optimize_pp='im_pp' in case['trainable'], allow_pw_adaptors='pw_adaptors' in case['trainable']), out


def test_aligner_oracle_options_against_reference_golden():
    """AlignerRef in fp32 against the unmodified reference PointCloudOptimizer in every setting recorded by tools/make_pco_golden.py
    (dist='l2', conf='sqrt' | 'id' | 'm1', every pose / focal preset, images of two areas, 138 edge sides on one image), at the bars of
    test_aligner_oracle_against_reference_golden: loss, the gradient of every trainable group (and no other), the first 10 losses."""
    g = _g('aligner_pco_options.pt')
    assert [c['name'] for c in g['cases']] == ['l2', 'conf_sqrt', 'conf_id', 'conf_m1', 'preset_all', 'preset_pose_only', 'preset_all_adaptors',
                                               'mixed_sizes', 'mixed_sizes_l2', 'oneref_70']
    for case in g['cases']:
        al, _ = pco_case_oracle(case)
        loss0, grads = al.grads()
        assert abs(loss0 - case['loss']) < 1e-6 * abs(case['loss']) + 1e-7, (case['name'], loss0, case['loss'])
        assert sorted(grads) == sorted(case['grads']) == sorted(case['trainable'])
        worst = 0.0
        for k, ref in case['grads'].items():
            err = float((grads[k] - ref).abs().max() / ref.abs().max())
            worst = max(worst, err)
            assert err < 2e-4, (case['name'], k, err)
        losses = al.run(niter=case['niter'])
        lerr = float((torch.tensor(losses[:10]) / case['losses'][:10] - 1).abs().max())
        print(f'{case["name"]:18s} loss {abs(loss0 / case["loss"] - 1):.1e}  gradients {worst:.1e}  first 10 losses {lerr:.1e}')
        assert lerr < 1e-4, (case['name'], lerr)
        st = al.state()
        for k in ('im_poses', 'im_focals', 'im_pp', 'pw_adaptors'):
            if k not in case['trainable']:
                assert torch.equal(st[k], case['state'][k]), (case['name'], k)          # frozen groups did not move
    presets = {c['name']: c for c in g['cases'] if c['preset']}
    assert presets['preset_all']['trainable'] == ['pw_poses', 'im_depthmaps'] and not presets['preset_all']['norm_pw_scale']
    assert presets['preset_pose_only']['trainable'] == ['pw_poses', 'im_depthmaps', 'im_focals'] and not presets['preset_pose_only']['norm_pw_scale']
    assert presets['preset_all_adaptors']['trainable'] == ['pw_poses', 'pw_adaptors', 'im_depthmaps'] and not presets['preset_all_adaptors']['norm_pw_scale']
    assert float(presets['preset_all_adaptors']['state']['pw_adaptors'].abs().min()) > 0


def test_aligner_oracle_edge_mean_weighting_against_reference_golden():
    """AlignerRef.edge_mean_loss() -- the weighting the mixed-size PointCloudOptimizer tests must tell their result apart from -- against the
    unmodified reference ModularPointCloudOptimizer on images of two areas (aligner_modular_grads.pt, 'mixed_sizes'), and the distance of
    the two weightings at that state."""
    from dust3r_amd.synthetic import synthetic_mixed_scene
    case = next(c for c in _g('aligner_modular_grads.pt')['cases'] if c['name'] == 'mixed_sizes')
    al = AlignerRef(synthetic_mixed_scene(**case['scene_args']))
    n, st = al.n_imgs, case['state']
    depth = torch.zeros((n, al.A))
    for i, (h, w) in enumerate(al.imshapes):
        depth[i, :h * w] = st[f'im_depthmaps.{i}'].flatten()
    al.load_state(dict(pw_poses=st['pw_poses'], pw_adaptors=st['pw_adaptors'], im_depthmaps=depth,
                       **{k: torch.stack([st[f'{k}.{i}'] for i in range(n)]) for k in ('im_poses', 'im_focals', 'im_pp')}))
    with torch.no_grad():
        mean, area = float(al.edge_mean_loss()), float(al.loss())
    assert abs(mean - case['loss']) < 1e-6 * abs(case['loss']) + 1e-7, (mean, case['loss'])
    assert abs(area / mean - 1) > 1e-2


def test_forward_oracle_equals_live_reference():
    """The oracle against the unmodified reference model on the same weights and views (tests/golden/reference_pins.pt `forward`): the same module tree
    (state-dict keys) and the same outputs. The ops and their order are the reference's, but a stored vector only matches bit for bit at the thread count
    it was recorded with (measured: up to 4e-6 between thread counts on one host), hence the cross-BLAS bar of the other forward fixtures."""
    g = _g('reference_pins.pt')['forward']
    m = build_ref_model(g['config'], seed=g['weight_seed'])
    assert sorted(m.state_dict().keys()) == g['keys']
    v1, v2 = synthetic_views(g['B'], g['H'], g['W'], seed=g['view_seed'])
    with torch.no_grad():
        b1, b2 = m(v1, v2)
    for a, b in ((b1['pts3d'], g['pts3d']), (b2['conf'], g['conf2'])):
        assert a.shape == b.shape
        assert float((a - b).abs().max() / b.abs().max()) < 1e-5


def test_state_dict_keys_match_reference_for_release_configs():
    """The engine's expected checkpoint keys/shapes == the reference model's own state_dict (restated croco underneath), as recorded in
    tests/golden/reference_pins.pt `state_dict_shapes`."""
    from dust3r_amd.model import expected_state
    shapes = _g('reference_pins.pt')['state_dict_shapes']
    for cfg in ('tiny_dpt', 'tiny_linear'):
        c = MODEL_CONFIGS[cfg]
        spec = expected_state(dict(enc_embed_dim=c['enc_embed_dim'], enc_depth=c['enc_depth'], dec_embed_dim=c['dec_embed_dim'],
                                   dec_depth=c['dec_depth'], patch_size=16, head_type=c['head_type']))
        sd = shapes[cfg]
        assert set(spec) == set(sd), (set(spec) ^ set(sd))
        for k, shape in spec.items():
            assert tuple(sd[k]) == tuple(shape), k


def test_cloud_restatements_equal_live_reference():
    """oracle/cloud_ref.py (Weiszfeld focal, clean_pointcloud) against what the unmodified reference functions returned on the same inputs
    (tests/golden/reference_pins.pt `focal`, `clean_pointcloud`)."""
    from dust3r_amd.synthetic import synthetic_scene
    from oracle.cloud_ref import clean_pointcloud_ref, estimate_focal_weiszfeld
    pins = _g('reference_pins.pt')
    fg = pins['focal']
    out, init, gt = synthetic_scene(fg['n_views'], fg['H'], fg['W'], seed=fg['seed'], symmetrize=True, noise=fg['noise'])
    for e, f_ref in zip(fg['edges'], fg['values']):
        assert abs(estimate_focal_weiszfeld(out['pred1']['pts3d'][e]) / f_ref - 1) < 1e-5
    # clean_pointcloud: world clouds of 4 views with one of them pulled towards its camera
    c = pins['clean_pointcloud']
    confs = c['confs']
    got = clean_pointcloud_ref([x.clone() for x in confs], c['K'], c['w2c'], c['depth'], c['pts'], tol=c['tol'], bad_conf=c['bad_conf'])
    changed = sum(int((r != x).sum()) for r, x in zip(c['out'], confs))
    assert changed > 50
    assert all(torch.equal(a, b) for a, b in zip(c['out'], got))


@pytest.mark.parametrize('n', [2, 3, 7])
def test_align_pose_sets_equals_live_reference(n):
    """dust3r_amd.cloud_opt.bootstrap.align_pose_sets (init='known_poses', PairViewer) against what the unmodified
    init_im_poses.align_multiple_poses returned on the same poses (tests/golden/reference_pins.pt `align_pose_sets`): the epsilon of the "point down
    the optical axis" is the median of the CONDENSED pairwise centre distances (geometry.py:364-366, scipy pdist) -- with 2 poses that is d / 100, not d / 200."""
    import numpy as np
    from dust3r_amd.cloud_opt.bootstrap import align_pose_sets, split_similarity
    g = _g('reference_pins.pt')['align_pose_sets'][n]
    s, R, t = split_similarity(align_pose_sets(g['src'].numpy(), g['dst'].numpy()))
    assert abs(float(s) / g['s'] - 1) < 1e-9
    assert np.abs(np.asarray(R) - g['R'].numpy()).max() < 1e-9 and np.abs(np.asarray(t).ravel() - g['T'].numpy().ravel()).max() < 1e-8


def test_reference_demo_binds_to_the_engine_through_the_integration_aliases():
    """with `dust3r.<hot-path module>` aliased to `dust3r_amd.<module>`, every name the reference's OWN dust3r/demo.py imports
    from those modules (its `from dust3r.<module> import ...` statements, recorded in tests/golden/reference_pins.pt `demo_imports`) resolves to the
    engine's. The import statements run in a fresh interpreter against the aliased module table."""
    import subprocess
    import sys
    imports = _g('reference_pins.pt')['demo_imports']
    aliased = ('model', 'inference', 'image_pairs', 'cloud_opt', 'utils.image', 'utils.device')
    bound = [(mod, names) for mod, names in imports if mod[len('dust3r.'):] in aliased]
    assert {n for _, names in bound for n in names} >= {'inference', 'make_pairs', 'load_images', 'global_aligner', 'GlobalAlignerMode'}
    stmts = '\n'.join(f"from {mod} import {', '.join(names)}" for mod, names in bound)
    code = r"""
import sys, types
sys.path.insert(0, %r)
import dust3r_amd, dust3r_amd.model, dust3r_amd.inference, dust3r_amd.image_pairs, dust3r_amd.cloud_opt, dust3r_amd.utils.image, dust3r_amd.utils.device
dust3r = types.ModuleType('dust3r')
dust3r.__path__ = []
sys.modules['dust3r'] = dust3r
for name in %r:
    sys.modules['dust3r.' + name] = sys.modules['dust3r_amd.' + name]
%s
import dust3r_amd.inference as I, dust3r_amd.image_pairs as P, dust3r_amd.cloud_opt as Cl, dust3r_amd.utils.image as U
assert inference is I.inference and make_pairs is P.make_pairs and load_images is U.load_images
assert global_aligner is Cl.global_aligner and GlobalAlignerMode is Cl.GlobalAlignerMode
print('aliases ok')
""" % (ROOT, aliased, stmts)
    r = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and 'aliases ok' in r.stdout, r.stderr[-2000:]
