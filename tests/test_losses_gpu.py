"""Ground-truth evaluation on the GPU: the median selection against torch.nanmedian, every recorded criterion and stage statistic against
the reference's fp64 record (tests/golden/losses_small.pt, losses_full.json, evaluate_small.pt, written by tools/make_loss_golden.py from
the unmodified reference), determinism and batch independence, and the end-to-end paths (loss_of_one_batch, evaluate).

The bar is a relative error of 1e-5 against fp64 (absolute 1e-6 where the expected value is 0), the bar tests/test_aligner_gpu.py holds a
GPU loss to. Every test prints the maximum it measured next to the deviation of the reference's own fp32 run."""
import json
import math
import os

import pytest
import torch

import dust3r_amd.losses as L
from dust3r_amd.synthetic_gt import gt_pairs

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(__file__), 'golden')
RTOL, ATOL0 = 1e-5, 1e-6
DEV = 'cuda:0'


def _small():
    return torch.load(os.path.join(GOLDEN, 'losses_small.pt'), weights_only=False)


def _err(got, want):
    """relative error; absolute where the expected value is 0; 0 when both are NaN"""
    got, want = float(got), float(want)
    if math.isnan(want):
        return 0.0 if math.isnan(got) else math.inf
    if want == 0.0:
        return abs(got) * (RTOL / ATOL0)           # scaled so that one bar serves both
    return abs(got / want - 1)


def _build(case):
    crit = eval(case['expr'], vars(L))
    return crit if case['reduction'] == 'mean' else crit.with_reduction(case['reduction'])


# ------------------------------------------------------------------------------------------------ selection
def _check_median(vals1, vals2=None, mask1=None, mask2=None):
    got = L.masked_median(vals1.to(DEV), None if vals2 is None else vals2.to(DEV), None if mask1 is None else mask1.to(DEV),
                          None if mask2 is None else mask2.to(DEV)).cpu()
    rows = []
    for v, m in ((vals1, mask1), (vals2, mask2)):
        if v is not None:
            rows.append(v if m is None else torch.where(m, v, torch.full_like(v, float('nan'))))
    want = torch.nanmedian(torch.cat(rows, dim=1), dim=1).values
    both_nan = got.isnan() & want.isnan()
    assert bool(((got == want) | both_nan).all()), (got, want)
    return got


def test_median_selection_equals_nanmedian():
    g = torch.Generator().manual_seed(0)
    _check_median(torch.randn(5, 1000, generator=g), torch.randn(5, 1000, generator=g))                         # random normals, even n
    _check_median(torch.randn(3, 1001, generator=g))                                                           # odd n, scalar loads (N % 4 != 0)
    ties = torch.tensor([-1.5, 0.0, 0.25, 0.25, 7.0])[torch.randint(0, 5, (4, 4096), generator=g)]
    _check_median(ties, ties.flip(1))                                                                          # heavy ties
    z = torch.tensor([[-0.0, 0.0, -0.0, 0.0], [-1.0, -0.0, 0.0, -2.0], [-3.0, -1.0, -2.0, -4.0]])
    _check_median(z)                                                                                           # negatives and both zeros
    inf = torch.randn(4, 64, generator=g)
    inf[0, :40] = float('inf')
    inf[1, :40] = -float('inf')
    inf[2, 3], inf[2, 9] = float('inf'), -float('inf')
    _check_median(inf)                                                                                         # +-inf present
    one = torch.randn(2, 8, generator=g)
    m = torch.zeros(2, 8, dtype=torch.bool)
    m[0, 5] = True                                                                                             # n = 1
    m[1, 2] = m[1, 6] = True                                                                                   # n = 2: the lower one
    got = _check_median(one, None, m)
    assert float(got[1]) == float(min(one[1, 2], one[1, 6]))
    v = torch.randn(6, 512, generator=g)
    m = torch.rand(6, 512, generator=g) < torch.tensor([0.0, 0.1, 0.5, 0.9, 1.0, 0.3])[:, None]                 # rows of different n, an all-masked row
    m2 = torch.rand(6, 512, generator=g) < 0.5
    m2[0] = False
    got = _check_median(v, v * 2 + 1, m, m2)
    assert bool(got[0].isnan()) and not bool(got[1:].isnan().any())
    nan = torch.randn(2, 100, generator=g)
    nan[0, ::3] = float('nan')
    _check_median(nan)                                                                                         # a NaN counts as masked
    big = torch.randn(1, 384 * 512, generator=g)
    _check_median(big, torch.randn(1, 384 * 512, generator=g))                                                 # n = 2 * 384 * 512
    _check_median(big, big.clone(), big > 0.3, big < -0.1)


# ------------------------------------------------------------------------------------------------ criteria
STAT_COLUMNS = dict(n1=(L.N1, 1), n2=(L.N2, 1), norm_pr=(L.NORM_PR, 1), norm_gt=(L.NORM_GT, 1), shift_pr=(L.SHIFT_PR, 1), shift_gt=(L.SHIFT_GT, 1),
                    center_pr=(L.CENTER_PR, 3), center_gt=(L.CENTER_GT, 3), scale_pr=(L.SCALE_PR, 1), scale_gt=(L.SCALE_GT, 1))


def _stage_stats(case, inputs):
    crit = eval(case['expr'], vars(L))
    crit = crit.pixel_loss if isinstance(crit, L.ConfLoss) else crit
    stats, _, _ = crit.evaluate(*inputs, **case['kwargs'])
    return stats.cpu()


def test_every_recorded_criterion_matches_fp64():
    rec = _small()
    inputs = rec['inputs']
    worst, worst_ref, n_compared = 0.0, 0.0, 0
    for case in rec['cases']:
        if case['reduction'] == 'none':
            continue                                   # compared pixel by pixel in test_per_pixel_maps
        loss, details = _build(case)(*inputs, **case['kwargs'])
        assert isinstance(loss, torch.Tensor) and loss.ndim == 0 and not loss.requires_grad
        assert set(details) == set(case['details64']), case['expr']
        errs = {'loss': _err(loss, case['loss64'])}
        refs = [_err(case['loss32'], case['loss64'])]
        for k, want in case['details64'].items():
            errs[k] = _err(details[k], want)
            refs.append(_err(case['details32'][k], want))
        if case['stats64'] is not None:
            stats = _stage_stats(case, inputs)
            for name, want in case['stats64'].items():
                col, width = STAT_COLUMNS[name]
                got = stats[:, col:col + width].reshape(want.shape)
                errs[name] = max(_err(g, w) for g, w in zip(got.flatten(), want.flatten()))
        n_compared += len(errs)
        print(f'{case["repr"]} {case["kwargs"]} {case["reduction"]}: max rel err {max(errs.values()):.2e} ({max(errs, key=errs.get)}), '
              f'reference fp32 vs fp64 {max(refs):.2e}')
        worst, worst_ref = max(worst, max(errs.values())), max(worst_ref, max(refs))
        assert max(errs.values()) <= RTOL, (case['expr'], errs)
    print(f'criteria: {n_compared} values compared, max rel err {worst:.2e}; reference fp32 vs fp64 {worst_ref:.2e}')
    assert n_compared > 100


def test_full_size_matches_fp64():
    rec = json.load(open(os.path.join(GOLDEN, 'losses_full.json')))
    inputs = [{k: v.to(DEV) for k, v in d.items()} for d in gt_pairs(**rec['generator'])]
    for case in rec['cases']:
        loss, details = eval(case['expr'], vars(L))(*inputs)
        errs = {'loss': _err(loss, case['loss64']), **{k: _err(details[k], v) for k, v in case['details64'].items()}}
        ref = max([_err(case['loss32'], case['loss64'])] + [_err(case['details32'][k], v) for k, v in case['details64'].items()])
        print(f'full size {case["repr"]}: max rel err {max(errs.values()):.2e}, reference fp32 vs fp64 {ref:.2e}')
        assert set(details) == set(case['details64']) and max(errs.values()) <= RTOL, errs


def _rows(d, idx):
    return {k: v[idx] for k, v in d.items()}


def test_batch_independence_and_determinism():
    data = [{k: v.to(DEV) for k, v in d.items()} for d in gt_pairs(8, 64, 96, seed=3, empty_view2=(5,))]
    for expr, alpha in (("Regr3D_ScaleShiftInv(L21, gt_scale=True)", None), ("Regr3D(L21, norm_mode='median_dis')", 0.2), ("Regr3D(L21, norm_mode='sqrt_dis')", None)):
        crit = eval(expr, vars(L))
        whole = crit.evaluate(*data, alpha=alpha)[0].cpu()
        again = crit.evaluate(*data, alpha=alpha)[0].cpu()
        assert torch.equal(whole.view(torch.int64), again.view(torch.int64))
        for b in range(8):
            one = crit.evaluate(*[_rows(d, slice(b, b + 1)) for d in data], alpha=alpha)[0].cpu()
            assert torch.equal(one.view(torch.int64), whole[b:b + 1].view(torch.int64)), (expr, b)
        perm = torch.tensor([3, 7, 0, 5, 1, 6, 2, 4])
        shuffled = crit.evaluate(*[_rows(d, perm.to(DEV)) for d in data], alpha=alpha)[0].cpu()
        assert torch.equal(shuffled.view(torch.int64), whole[perm].view(torch.int64))


def test_empty_views_do_not_poison_the_batch():
    rec = _small()
    inputs = rec['inputs']
    assert not inputs[1]['valid_mask'][2].any()
    case = rec['cases'][0]
    crit = eval(case['expr'], vars(L))
    stats = crit.evaluate(*inputs)[0].cpu()
    assert float(stats[2, L.N2]) == 0 and float(stats[2, L.SUM_L2]) == 0 and bool(stats[:, [L.SUM_L1, L.SUM_L2]].isfinite().all())
    loss, details = crit(*inputs)
    assert math.isfinite(float(loss)) and _err(loss, case['loss64']) <= RTOL
    # both views of one pair empty: its medians are NaN and touch nothing
    both = [dict(d) for d in inputs]
    for k in (0, 1):
        both[k]['valid_mask'] = both[k]['valid_mask'].clone()
        both[k]['valid_mask'][1] = False
    stats2 = crit.evaluate(*both)[0].cpu()
    assert bool(stats2[1, L.SHIFT_PR].isnan()) and stats2[1, [L.N1, L.N2, L.SUM_L1, L.SUM_L2]].tolist() == [0, 0, 0, 0]
    assert torch.equal(stats2[[0, 3]].view(torch.int64), stats[[0, 3]].view(torch.int64))
    assert math.isfinite(float(crit(*both)[0]))
    # nothing valid at all: the reference's guarded mean gives 0
    none = [dict(d) for d in inputs]
    for k in (0, 1):
        none[k]['valid_mask'] = torch.zeros_like(none[k]['valid_mask'])
    assert float(L.Regr3D(L.L21)(*none)[0]) == 0.0


def test_per_pixel_maps():
    """l = |pred - gt| is a difference of points of the scene's magnitude S, so fp32 rounding of the operands bounds its ABSOLUTE error by a
    few ulp of S whatever l is; a pixel where the prediction is nearly right has a small l and an arbitrary relative error (the reference's
    own fp32 run differs from its fp64 run by 8.6e-5 of l at the worst pixel of this fixture). The bar per pixel is therefore RTOL * S,
    S = the largest ground-truth distance to camera 1; the means over pixels (the details) are held to RTOL as everywhere."""
    rec = _small()
    cases = [c for c in rec['cases'] if c['reduction'] == 'none']
    assert cases
    v1, v2 = rec['inputs'][:2]
    to_cam1 = torch.linalg.inv(v1['camera_pose'].double())
    S = max(float((v['pts3d'].double() @ to_cam1[:, None, :3, :3].transpose(-1, -2) + to_cam1[:, None, None, :3, 3]).norm(dim=-1).max()) for v in (v1, v2))
    for case in cases:
        ((l1, m1), (l2, m2)), details = _build(case)(*rec['inputs'], **case['kwargs'])
        want = case['loss64']
        assert torch.equal(m1.cpu(), want['m1']) and torch.equal(m2.cpu(), want['m2'])
        assert l1.shape == want['l1'].shape and l2.shape == want['l2'].shape
        err = max(float((l1.cpu().double() - want['l1']).abs().max()), float((l2.cpu().double() - want['l2']).abs().max())) / S
        ref = max(float((case['loss32']['l1'].double() - want['l1']).abs().max()), float((case['loss32']['l2'].double() - want['l2']).abs().max())) / S
        print(f'per-pixel {case["repr"]}: max abs err / scene size {err:.2e} (scene size {S:.2f}), reference fp32 vs fp64 {ref:.2e}')
        assert err <= RTOL
        assert set(details) == set(case['details64']) and all(_err(details[k], v) <= RTOL for k, v in case['details64'].items())


def test_geometry_helpers():
    from dust3r_amd.utils.geometry import get_joint_pointcloud_center_scale, get_joint_pointcloud_depth, normalize_pointcloud
    rec = _small()
    v1, v2, p1, p2 = rec['inputs']
    q1, q2, m1, m2 = p1['pts3d'], p2['pts3d_in_other_view'], v1['valid_mask'], v2['valid_mask']
    h = rec['helpers']
    worst = 0.0
    for mode, want in h['norm_factor'].items():
        a, b, f = normalize_pointcloud(q1, q2, mode, m1, m2, ret_factor=True)
        assert a.shape == q1.shape and b.shape == q2.shape and f.shape == (4, 1, 1, 1)
        worst = max(worst, max(_err(g, w) for g, w in zip(f.flatten(), want)))
        if mode == 'avg_warp-log1p':
            for got, w in zip((a, b), h['warp_pts']):
                worst = max(worst, float((got[:1].double() - w.double()).norm(dim=-1).max() / w.double().norm(dim=-1).max()))      # invalid points warp to 0
    single = normalize_pointcloud(q1, None, 'avg_dis', m1)
    assert isinstance(single, torch.Tensor) and single.shape == q1.shape
    z = get_joint_pointcloud_depth(q1[..., 2], q2[..., 2], m1, m2)
    worst = max(worst, max(_err(g, w) for g, w in zip(z, h['depth'])))
    z = get_joint_pointcloud_depth(q1[..., 2], None, m1)
    worst = max(worst, max(_err(g, w) for g, w in zip(z, h['depth_one_view'])))
    with pytest.raises(NotImplementedError):
        get_joint_pointcloud_depth(q1[..., 2], q2[..., 2], m1, m2, quantile=0.3)
    for name, kw in (('default', {}), ('z_only', dict(z_only=True)), ('no_center', dict(center=False))):
        c, s = get_joint_pointcloud_center_scale(q1, q2, m1, m2, **kw)
        wc, ws = h['center_scale'][name]
        assert c.shape == wc.shape == (4, 1, 1, 3) and s.shape == ws.shape == (4, 1, 1, 1)
        worst = max(worst, max(_err(g, w) for g, w in zip(c.flatten(), wc.flatten())), max(_err(g, w) for g, w in zip(s.flatten(), ws.flatten())))
    with pytest.raises(ValueError):
        normalize_pointcloud(q1, q2, 'avg_dist', m1, m2)
    print(f'geometry helpers: max rel err {worst:.2e}')
    assert worst <= RTOL


# ------------------------------------------------------------------------------------------------ end to end
def _tiny_model():
    from dust3r_amd.model import AsymmetricCroCo3DStereo
    from dust3r_amd.synthetic import MODEL_CONFIGS
    from oracle.dust3r_ref import build_ref_model
    m = AsymmetricCroCo3DStereo(landscape_only=False, **MODEL_CONFIGS['tiny_dpt'])
    m.load_state_dict(build_ref_model('tiny_dpt').state_dict())
    return m.to(DEV)


def _batch(B, seed):
    v1, v2, _, _ = gt_pairs(B, 32, 48, seed=seed)
    return v1, v2


def test_loss_of_one_batch_with_a_criterion():
    from dust3r_amd.inference import loss_of_one_batch
    model = _tiny_model()
    crit = eval("ConfLoss(Regr3D(L21, norm_mode='avg_dis'), alpha=0.2) + 0.5*Regr3D_ScaleShiftInv(L21, gt_scale=True)", vars(L))
    plain = loss_of_one_batch(_batch(3, 7), model, None, DEV, symmetrize_batch=True)
    assert plain['loss'] is None and set(plain) == {'view1', 'view2', 'pred1', 'pred2', 'loss'}
    res = loss_of_one_batch(_batch(3, 7), model, crit, DEV, symmetrize_batch=True)
    for side, key in (('pred1', 'pts3d'), ('pred1', 'conf'), ('pred2', 'pts3d_in_other_view'), ('pred2', 'conf')):
        assert torch.equal(res[side][key], plain[side][key])                       # criterion=None output unchanged
    assert res['pred1']['pts3d'].shape == (6, 32, 48, 3) and res['pred1']['pts3d'].is_cuda
    loss, details = res['loss']
    loss2, details2 = crit(res['view1'], res['view2'], res['pred1'], res['pred2'])
    assert float(loss) == float(loss2) and details == details2 and math.isfinite(float(loss))
    assert set(details) == {'conf_loss_1', 'conf_loss2', 'Regr3D_pts3d_1', 'Regr3D_pts3d_2', 'Regr3D_ScaleShiftInv_pts3d_1', 'Regr3D_ScaleShiftInv_pts3d_2'}
    only = loss_of_one_batch(_batch(3, 7), model, crit, DEV, symmetrize_batch=True, ret='loss')
    assert float(only[0]) == float(loss) and only[1] == details


def test_evaluate_reproduces_the_record():
    from dust3r_amd.evaluation import evaluate
    rec = torch.load(os.path.join(GOLDEN, 'evaluate_small.pt'), weights_only=False)
    calls = iter(rec['preds'])

    def stub(view1, view2):
        assert view1['img'].shape[0] == 4                                         # the symmetrised batch
        return tuple({k: v.to(DEV) for k, v in d.items()} for d in next(calls))
    table = evaluate(stub, eval(rec['expr'], vars(L)), rec['batches'], DEV, symmetrize_batch=True)
    assert set(table) == set(rec['table'])
    errs = {k: _err(table[k], v) for k, v in rec['table'].items()}
    print(f'evaluate: {len(errs)} entries, max rel err {max(errs.values()):.2e}')
    assert max(errs.values()) <= RTOL, errs


def test_evaluate_does_not_depend_on_the_engine_batch():
    from dust3r_amd.evaluation import evaluate
    model = _tiny_model()
    crit = eval("Regr3D_ScaleShiftInv(L21, gt_scale=True)", vars(L))
    tables = [evaluate(model, crit, [_batch(3, 20 + k) for k in range(3)], DEV, engine_batch=eb) for eb in (1, 32)]
    assert tables[0] == tables[1] and set(tables[0]) == {f'{k}_{s}' for k in ('loss', 'Regr3D_ScaleShiftInv_pts3d_1', 'Regr3D_ScaleShiftInv_pts3d_2')
                                                         for s in ('avg', 'med')}
    assert all(math.isfinite(v) for v in tables[0].values())
