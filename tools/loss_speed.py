"""Times the fused criterion call (d3r_pair_criterion through dust3r_amd.losses) for 32 and 64 pairs of 512 x 384 resident on the device, for
the two criterion strings of the reference's README, against (a) the floor of reading every input once at the achievable HBM copy rate and
(b) a plain torch composition of the same formulae on the same device; then `evaluate` on the full-size model with random weights:
pairs/s with the criterion against pairs/s of the forward alone in the same process. One process, prints one JSON line per measurement.

    timeout 900 python tools/loss_speed.py [--no-model]
"""
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import dust3r_amd.losses as L  # noqa: E402
from dust3r_amd.synthetic_gt import gt_pairs  # noqa: E402

COPY_RATE = 4.0e12          # bytes/s: the achievable read rate of a streaming kernel on the MI355X (of 8 TB/s peak)
BYTES_PER_PIXEL = 2 * (12 + 12 + 4 + 1)      # both views: ground truth, prediction, confidence, mask
CRITERIA = ("Regr3D_ScaleShiftInv(L21, gt_scale=True)", "ConfLoss(Regr3D(L21, norm_mode='avg_dis'), alpha=0.2)")


def device_ms(fn, reps=25, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return statistics.median(times)


def torch_composition(expr, v1, v2, p1, p2):
    """the same criterion from plain torch ops (masked medians by sorting NaN-padded rows), everything on the device"""
    B = v1['pts3d'].shape[0]
    T = torch.linalg.inv(v1['camera_pose'])
    g = [(v['pts3d'].reshape(B, -1, 3) @ T[:, :3, :3].transpose(1, 2) + T[:, None, :3, 3]) for v in (v1, v2)]
    q = [p1['pts3d'].reshape(B, -1, 3), p2['pts3d_in_other_view'].reshape(B, -1, 3)]
    m = [v['valid_mask'].reshape(B, -1) for v in (v1, v2)]
    allm = torch.cat(m, 1)
    nan = torch.full((), float('nan'), device=allm.device)

    def jmed(a, b):
        return torch.where(allm, torch.cat((a, b), 1), nan).nanmedian(dim=1).values
    n = allm.sum(1)
    f = (torch.cat(q, 1).norm(dim=-1) * allm).sum(1) / (n + 1e-8)
    q = [x / f.clip(min=1e-8)[:, None, None] for x in q]
    if expr.startswith('ConfLoss'):
        g_f = (torch.cat(g, 1).norm(dim=-1) * allm).sum(1) / (n + 1e-8)
        g = [x / g_f.clip(min=1e-8)[:, None, None] for x in g]
        conf = [p1['conf'].reshape(B, -1), p2['conf'].reshape(B, -1)]
        out = 0
        for k in (0, 1):
            l = (q[k] - g[k]).norm(dim=-1)
            out = out + ((l * conf[k] - 0.2 * conf[k].log()) * m[k]).sum() / m[k].sum()
        return out
    sides = []
    for pts in (g, q):
        sh = jmed(pts[0][..., 2], pts[1][..., 2])
        pts = [torch.cat((x[..., :2], x[..., 2:] - sh[:, None, None]), -1) for x in pts]
        c = torch.stack([jmed(pts[0][..., i], pts[1][..., i]) for i in range(3)], -1)
        s = jmed((pts[0] - c[:, None]).norm(dim=-1), (pts[1] - c[:, None]).norm(dim=-1))
        sides.append((pts, s))
    (g, gs), (q, qs) = sides
    r = (gs / qs.clip(1e-3, 1e3))[:, None, None]
    return sum((((q[k] * r - g[k]).norm(dim=-1)) * m[k]).sum() / m[k].sum() for k in (0, 1))


def main():
    dev = 'cuda:0'
    H, W = 384, 512
    for B in (() if '--model-only' in sys.argv else (32, 64)):
        data = [{k: v.to(dev) for k, v in d.items()} for d in gt_pairs(B, H, W, seed=2)]
        floor_ms = B * H * W * BYTES_PER_PIXEL / COPY_RATE * 1e3
        for expr in CRITERIA:
            crit = eval(expr, vars(L))
            pixel = crit.pixel_loss if isinstance(crit, L.ConfLoss) else crit
            alpha = crit.alpha if isinstance(crit, L.ConfLoss) else None
            fused = device_ms(lambda: pixel.evaluate(*data, alpha=alpha))
            plain = device_ms(lambda: torch_composition(expr, *data), reps=20, warm=2)
            passes = L.criterion_passes(norm_mode=pixel.norm_mode, gt_scale=pixel.gt_scale, shift_inv=pixel._shift_inv, scale_inv=pixel._scale_inv)
            value, ref = float(crit(*data)[0]), float(torch_composition(expr, *data))
            print(json.dumps(dict(what='criterion', criterion=expr, pairs=B, fused_ms=round(fused, 4), fused_us_per_pair=round(fused / B * 1e3, 2),
                                  passes=passes, read_once_floor_ms=round(floor_ms, 4), torch_ms=round(plain, 3), fused_value=value, torch_value=ref)), flush=True)
    if '--no-model' in sys.argv:
        return
    from dust3r_amd.evaluation import evaluate
    from dust3r_amd.inference import loss_of_one_batch
    from dust3r_amd.model import AsymmetricCroCo3DStereo
    from dust3r_amd.synthetic import MODEL_CONFIGS, OUT_GAIN, synthetic_state_dict
    name = 'DUSt3R_ViTLarge_BaseDecoder_512_dpt'
    model = AsymmetricCroCo3DStereo(landscape_only=False, **MODEL_CONFIGS[name])
    model.load_state_dict(synthetic_state_dict({k: torch.empty(v, device='meta') for k, v in model._spec.items()}, 0, OUT_GAIN[name], device=dev))
    model = model.to(dev)
    B, n_batches = 16, 4                                                    # symmetrised: 32 pairs per engine call
    batches = [tuple({k: v.to(dev) for k, v in d.items()} for d in gt_pairs(B, H, W, seed=30 + k)[:2]) for k in range(n_batches)]
    crit = eval(CRITERIA[0], vars(L))

    def wall(fn):
        import time
        fn()
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t
    pairs = 2 * B * n_batches
    t_eval = wall(lambda: evaluate(model, crit, batches, dev, symmetrize_batch=True))
    t_fwd = wall(lambda: [loss_of_one_batch(b, model, None, dev, symmetrize_batch=True) for b in batches])
    print(json.dumps(dict(what='evaluate', model=name, criterion=CRITERIA[0], pairs=pairs, pairs_per_s_with_criterion=round(pairs / t_eval, 1),
                          pairs_per_s_forward_only=round(pairs / t_fwd, 1), criterion_share=round(1 - t_fwd / t_eval, 4))), flush=True)


if __name__ == '__main__':
    main()
