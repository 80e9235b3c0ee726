"""Records the fixtures of the criterion tests from the UNMODIFIED reference (imported through oracle.ref_import; build machine only):
tests/golden/losses_small.pt, losses_full.json, evaluate_small.pt. Everything is evaluated in fp64 (the expected values) and in the
reference's own fp32 (recorded next to them: its distance to fp64 is the yardstick the GPU results are printed against).

    python tools/make_loss_golden.py
"""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from dust3r_amd.synthetic_gt import checksum, gt_pairs  # noqa: E402
from oracle.ref_import import import_reference  # noqa: E402

GOLDEN = os.path.join(ROOT, 'tests', 'golden')
README_TEST = "Regr3D_ScaleShiftInv(L21, gt_scale=True)"
README_TRAIN = "ConfLoss(Regr3D(L21, norm_mode='avg_dis'), alpha=0.2)"
# (expression, keyword arguments of the call, reduction)
CASES = [(README_TEST, {}, 'mean'), (README_TRAIN, {}, 'mean')] + \
        [(f"Regr3D(L21, norm_mode={m!r})", {}, 'mean') for m in ('avg_dis', 'avg_log1p', 'avg_warp-log1p', 'median_dis', 'sqrt_dis', False)] + \
        [("Regr3D(L21, gt_scale=True)", {}, 'mean'), ("Regr3D_ShiftInv(L21)", {}, 'mean'), ("Regr3D_ScaleInv(L21)", {}, 'mean'),
         ("Regr3D_ScaleInv(L21, gt_scale=True)", {}, 'mean'), ("Regr3D_ScaleShiftInv(L21, gt_scale=False)", {}, 'mean'),
         ("ConfLoss(Regr3D_ScaleShiftInv(L21, gt_scale=True), alpha=0.5)", {}, 'mean'),
         ("ConfLoss(Regr3D(L21), alpha=0.2) + 0.5*Regr3D_ScaleShiftInv(L21, gt_scale=True)", {}, 'mean'),
         ("Regr3D(L21)", {'dist_clip': 3.0}, 'mean'), ("Regr3D(L21)", {}, 'sum'), ("Regr3D_ScaleShiftInv(L21, gt_scale=True)", {}, 'none')]


def cast(d, dtype):
    return {k: (v.to(dtype) if v.is_floating_point() else v.clone()) for k, v in d.items()}


def main():
    import_reference()
    import dust3r.losses as RL
    from dust3r.inference import loss_of_one_batch as ref_loss_of_one_batch
    from dust3r.utils import geometry as RG

    def build(expr, reduction):
        crit = eval(expr, vars(RL))
        return crit if reduction == 'mean' else crit.with_reduction(reduction)

    def run(expr, kw, reduction, data, dtype):
        v1, v2, p1, p2 = (cast(d, dtype) for d in data)
        crit = build(expr, reduction)
        loss, details = crit(v1, v2, p1, p2, **kw)
        if reduction == 'none':
            (l1, m1), (l2, m2) = loss
            return dict(l1=l1, l2=l2, m1=m1, m2=m2), details, repr(crit)
        return float(loss), details, repr(crit)

    def stages(expr, kw, data):
        """the per-pair statistics of a single Regr3D-family term, by the reference's own geometry functions, fp64"""
        crit = eval(expr, vars(RL))
        if isinstance(crit, RL.ConfLoss):
            crit = crit.pixel_loss
        if not isinstance(crit, RL.Regr3D) or crit._loss2 is not None:
            return None
        v1, v2, p1, p2 = (cast(d, torch.float64) for d in data)
        to_cam1 = RG.inv(v1['camera_pose'])
        g1, g2 = RG.geotrf(to_cam1, v1['pts3d']), RG.geotrf(to_cam1, v2['pts3d'])
        m1, m2 = v1['valid_mask'].clone(), v2['valid_mask'].clone()
        if kw.get('dist_clip') is not None:
            m1, m2 = m1 & (g1.norm(dim=-1) <= kw['dist_clip']), m2 & (g2.norm(dim=-1) <= kw['dist_clip'])
        q1, q2 = p1['pts3d'], p2['pts3d_in_other_view']
        st = dict(n1=m1.flatten(1).sum(1).double(), n2=m2.flatten(1).sum(1).double())
        if crit.norm_mode:
            q1, q2, f = RG.normalize_pointcloud(q1, q2, crit.norm_mode, m1, m2, ret_factor=True)
            st['norm_pr'] = f.flatten()
            if not crit.gt_scale:
                g1, g2, f = RG.normalize_pointcloud(g1, g2, crit.norm_mode, m1, m2, ret_factor=True)
                st['norm_gt'] = f.flatten()
        if isinstance(crit, RL.Regr3D_ShiftInv):
            st['shift_gt'] = RG.get_joint_pointcloud_depth(g1[..., 2], g2[..., 2], m1, m2)
            st['shift_pr'] = RG.get_joint_pointcloud_depth(q1[..., 2], q2[..., 2], m1, m2)
            g1, g2, q1, q2 = g1.clone(), g2.clone(), q1.clone(), q2.clone()
            for p, s in ((g1, st['shift_gt']), (g2, st['shift_gt']), (q1, st['shift_pr']), (q2, st['shift_pr'])):
                p[..., 2] -= s[:, None, None]
        if isinstance(crit, RL.Regr3D_ScaleInv):
            c, s = RG.get_joint_pointcloud_center_scale(g1, g2, m1, m2)
            st['center_gt'], st['scale_gt'] = c.reshape(-1, 3), s.flatten()
            c, s = RG.get_joint_pointcloud_center_scale(q1, q2, m1, m2)
            st['center_pr'], st['scale_pr'] = c.reshape(-1, 3), s.flatten()
        return st

    # ---------------------------------------------------------------------------------------------- losses_small.pt
    data = gt_pairs(4, 32, 48, seed=0, invalid=0.3, empty_view2=(2,))
    inputs = [{k: v for k, v in d.items() if k != 'img'} for d in data]
    cases = []
    for expr, kw, reduction in CASES:
        e64, d64, name = run(expr, kw, reduction, inputs, torch.float64)
        e32, d32, _ = run(expr, kw, reduction, inputs, torch.float32)
        if reduction != 'none':
            assert abs(e64) >= 0.01, (expr, e64)
            print(f'{name:100s} {reduction:5s} fp64 {e64:+.9f}  fp32 rel dev {abs(e32 / e64 - 1):.2e}')
        cases.append(dict(expr=expr, kwargs=kw, reduction=reduction, repr=name, loss64=e64, details64=d64, loss32=e32, details32=d32,
                          stats64=stages(expr, kw, inputs)))
    v1, v2, p1, p2 = (cast(d, torch.float64) for d in inputs)
    q1, q2, m1, m2 = p1['pts3d'], p2['pts3d_in_other_view'], v1['valid_mask'], v2['valid_mask']
    helpers = dict(norm_factor={m: RG.normalize_pointcloud(q1, q2, m, m1, m2, ret_factor=True)[2].flatten()
                                for m in ('avg_dis', 'avg_log1p', 'avg_warp-log1p', 'median_dis', 'sqrt_dis')},
                   warp_pts=[t[:1].float() for t in RG.normalize_pointcloud(q1, q2, 'avg_warp-log1p', m1, m2)],      # pair 0
                   depth=RG.get_joint_pointcloud_depth(q1[..., 2], q2[..., 2], m1, m2),
                   depth_one_view=RG.get_joint_pointcloud_depth(q1[..., 2], None, m1),
                   center_scale={name: [t.clone() for t in RG.get_joint_pointcloud_center_scale(q1, q2, m1, m2, **kw)]
                                 for name, kw in (('default', {}), ('z_only', dict(z_only=True)), ('no_center', dict(center=False)))})
    torch.save(dict(inputs=inputs, checksum=checksum(*data), generator=dict(B=4, H=32, W=48, seed=0, invalid=0.3, empty_view2=(2,)),
                    cases=cases, helpers=helpers), os.path.join(GOLDEN, 'losses_small.pt'))

    # ---------------------------------------------------------------------------------------------- losses_full.json
    gen = dict(B=8, H=384, W=512, seed=1, invalid=0.3)
    data = gt_pairs(**gen)
    full = dict(generator=gen, checksum=checksum(*data), cases=[])
    for expr in (README_TEST, README_TRAIN):
        e64, d64, name = run(expr, {}, 'mean', data, torch.float64)
        e32, d32, _ = run(expr, {}, 'mean', data, torch.float32)
        print(f'full {name}: fp64 {e64:+.9f}, fp32 rel dev {abs(e32 / e64 - 1):.2e}')
        full['cases'].append(dict(expr=expr, repr=name, loss64=e64, details64=d64, loss32=e32, details32=d32))
    with open(os.path.join(GOLDEN, 'losses_full.json'), 'w') as f:
        json.dump(full, f, indent=1)

    # ---------------------------------------------------------------------------------------------- evaluate_small.pt
    expr = "ConfLoss(Regr3D(L21), alpha=0.2) + 0.5*Regr3D_ScaleShiftInv(L21, gt_scale=True)"
    crit = eval(expr, vars(RL))
    batches, preds, history = [], [], {}
    for k in range(5):
        a1, a2, _, _ = gt_pairs(2, 12, 16, seed=10 + k)
        s1, s2, q1, q2 = gt_pairs(4, 12, 16, seed=100 + k, scale=1.3 + 0.1 * k)      # what the stub "predicts" for the symmetrised batch
        batches.append((a1, a2))
        preds.append((dict(pts3d=q1['pts3d'], conf=q1['conf']), dict(pts3d_in_other_view=q2['pts3d_in_other_view'], conf=q2['conf'])))
        calls = iter([preds[-1]])
        stub = lambda view1, view2: tuple(cast(d, torch.float64) for d in next(calls))      # noqa: E731
        batch = tuple(cast(d, torch.float64) for d in (a1, a2))
        loss, details = ref_loss_of_one_batch(batch, stub, crit, 'cpu', symmetrize_batch=True, ret='loss')
        for key, v in dict(loss=float(loss), **details).items():
            history.setdefault(key, []).append(float(v))
    table = {}
    for key, values in history.items():
        t = torch.tensor(values, dtype=torch.float64)
        table[f'{key}_avg'], table[f'{key}_med'] = float(t.mean()), float(t.median())
    torch.save(dict(expr=expr, batches=batches, preds=preds, history=history, table=table), os.path.join(GOLDEN, 'evaluate_small.pt'))
    for name in ('losses_small.pt', 'losses_full.json', 'evaluate_small.pt'):
        print(name, os.path.getsize(os.path.join(GOLDEN, name)), 'bytes')


if __name__ == '__main__':
    main()
