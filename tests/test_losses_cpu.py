"""Ground-truth evaluation without a device: the criterion algebra of dust3r_amd.losses (names, `repr`, `+` / `*` chaining, with_reduction),
`eval` of the README's criterion strings, argument validation, the resource report of losses.hip and the hashed ground-truth generator."""
import json
import os
import re

import pytest
import torch

import dust3r_amd.losses as L
from dust3r_amd.synthetic_gt import checksum, gt_pairs

GOLDEN = os.path.join(os.path.dirname(__file__), 'golden')
README_TEST = "Regr3D_ScaleShiftInv(L21, gt_scale=True)"
README_TRAIN = "ConfLoss(Regr3D(L21, norm_mode='avg_dis'), alpha=0.2)"


def _small():
    return torch.load(os.path.join(GOLDEN, 'losses_small.pt'), weights_only=False)


def test_repr_strings_equal_the_recorded_ones():
    for case in _small()['cases']:
        crit = eval(case['expr'], vars(L))
        if case['reduction'] != 'mean':
            crit = crit.with_reduction(case['reduction'])
        assert repr(crit) == case['repr'], case['expr']


def test_readme_strings_build_criteria():
    test, train = eval(README_TEST, vars(L)), eval(README_TRAIN, vars(L))
    assert isinstance(test, L.Regr3D_ScaleShiftInv) and test.gt_scale is True and test.norm_mode == 'avg_dis'
    assert test._shift_inv and test._scale_inv and not L.Regr3D._shift_inv and not L.Regr3D_ShiftInv._scale_inv
    assert isinstance(train, L.ConfLoss) and train.alpha == 0.2 and train.pixel_loss.criterion.reduction == 'none'
    assert repr(test) == 'Regr3D_ScaleShiftInv(L21Loss())' and repr(train) == 'ConfLoss(Regr3D(L21Loss()))'
    assert test.to('cpu') is test and train.eval() is train


def test_chaining_and_scaling():
    a, b, c = L.Regr3D(L.L21), L.Regr3D_ShiftInv(L.L21), L.ConfLoss(L.Regr3D(L.L21), alpha=0.2)
    s = c + 0.5 * b + a * 2
    assert repr(s) == 'ConfLoss(Regr3D(L21Loss())) + 0.5*Regr3D_ShiftInv(L21Loss()) + 2*Regr3D(L21Loss())'
    assert (a._alpha, a._loss2, b._alpha, b._loss2, c._loss2) == (1, None, 1, None, None)       # the operands stay as they were
    assert s._loss2._alpha == 0.5 and s._loss2._loss2._alpha == 2
    assert repr(0.25 * a) == '0.25*Regr3D(L21Loss())' and repr(a * 1) == 'Regr3D(L21Loss())'
    with pytest.raises(TypeError):
        a + 1
    with pytest.raises(TypeError):
        a * 'x'


def test_with_reduction_copies():
    a = L.Regr3D(L.L21) + L.Regr3D_ScaleInv(L.L21)
    n = a.with_reduction('none')
    assert n is not a and n.criterion.reduction == 'none' and n._loss2.criterion.reduction == 'none'
    assert a.criterion.reduction == 'mean' and a._loss2.criterion.reduction == 'mean' and L.L21.reduction == 'mean'
    assert L.Regr3D(L.L21).criterion is not L.L21
    with pytest.raises(TypeError):
        (L.Regr3D(L.L21) + L.ConfLoss(L.Regr3D(L.L21))).with_reduction('none')


def test_pixel_criterion_on_plain_tensors():
    a, b = torch.tensor([[3.0, 0.0, 4.0], [0.0, 0.0, 0.0]]), torch.zeros(2, 3)
    assert float(L.L21(a, b)) == 2.5
    assert L.L21Loss('none')(a, b).tolist() == [5.0, 0.0] and float(L.L21Loss('sum')(a, b)) == 5.0
    assert float(L.L21(a[:0], b[:0])) == 0.0
    with pytest.raises(ValueError):
        L.L21(torch.zeros(2, 4), torch.zeros(2, 4))
    with pytest.raises(ValueError):
        L.L21Loss('max')(a, b)


def test_argument_validation():
    with pytest.raises(TypeError):
        L.Regr3D(None)
    with pytest.raises(TypeError):
        L.Regr3D('L21')
    with pytest.raises(ValueError):
        L.Regr3D(L.L21, norm_mode='avg_dist')
    with pytest.raises(ValueError):
        L.ConfLoss(L.Regr3D(L.L21), alpha=0)
    with pytest.raises(TypeError):
        L.ConfLoss(L.L21)
    assert L.Regr3D(L.L21, norm_mode=False).norm_mode is False
    from dust3r_amd.inference import get_pred_pts3d
    x = torch.zeros(1, 2, 2, 3)
    assert get_pred_pts3d({}, dict(pts3d=x)) is x and get_pred_pts3d({}, dict(pts3d_in_other_view=x), use_pose=True) is x
    with pytest.raises(ValueError):
        get_pred_pts3d({}, dict(pts3d_in_other_view=x))
    with pytest.raises(NotImplementedError):
        get_pred_pts3d({}, dict(depth=x, pseudo_focal=x))
    pose = torch.eye(4)[None].clone()
    pose[0, 0, 3] = 2.0
    assert get_pred_pts3d({}, dict(pts3d=x, camera_pose=pose), use_pose=True)[0, 0, 0].tolist() == [2.0, 0.0, 0.0]


def test_criterion_off_the_gpu_raises():
    from dust3r_amd._lib import D3RError
    if torch.cuda.is_available():
        return
    v1, v2, p1, p2 = gt_pairs(1, 8, 8)
    with pytest.raises(D3RError):
        eval(README_TEST, vars(L))(v1, v2, p1, p2)


def test_resource_report_has_no_scratch():
    from dust3r_amd import _lib
    path = os.path.join(os.path.dirname(_lib.LIB_PATH), 'losses.resources.txt')
    if not os.path.exists(path):
        pytest.skip('no resource report next to the library (written by dust3r_amd/build.py)')
    report = open(path).read()
    kernels = re.findall(r'Function Name: (\S+)', report)
    assert sum('losses' in k for k in kernels) == len(kernels) >= 10
    assert any('pass_kernel' in k for k in kernels) and any('scan_kernel' in k for k in kernels)
    assert re.findall(r'ScratchSize \[bytes/lane\]: (\d+)', report) == ['0'] * len(kernels)
    assert {'d3r_pair_criterion', 'd3r_pair_criterion_workspace_bytes', 'd3r_pair_criterion_passes', 'd3r_masked_median'} <= set(_lib.EXPORTED)
    assert _lib.lib.d3r_pair_criterion_workspace_bytes(2, 1000) >= 2 * 6 * 2048 * 4
    assert L.criterion_passes(norm_mode='avg_dis', gt_scale=True, shift_inv=True, scale_inv=True) == 11
    assert L.criterion_passes(norm_mode='avg_dis') == 2 and L.criterion_passes(norm_mode='median_dis', stop_after=L.STAGE_NORM) == 4


def test_hashed_generator_is_reproducible():
    rec = _small()
    data = gt_pairs(**rec['generator'])
    assert checksum(*data) == rec['checksum']
    for got, want in zip(data, rec['inputs']):
        for k, v in want.items():
            assert torch.equal(got[k], v), k
    assert not data[1]['valid_mask'][2].any() and 0.6 < float(data[0]['valid_mask'].float().mean()) < 0.8
    assert 1.0 <= float(data[2]['conf'].min()) and float(data[3]['conf'].max()) < 6.0
    full = json.load(open(os.path.join(GOLDEN, 'losses_full.json')))
    assert checksum(*gt_pairs(**full['generator'])) == full['checksum']
