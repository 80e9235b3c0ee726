"""Speed of the dataset view pipeline on the GPU (run on the MI355X box):
  python tools/dataset_speed.py [--pairs 32] [--big-pairs 32] [--repeats 7] [--evaluate]
For a batch of pairs at 512x384 from 640x480 and from 4032x3024 sources, EVERY VIEW WITH A SOURCE ARRAY OF ITS OWN (built once, outside
the timed regions), so uploads and source reads are those of a real batch:
  kernels   the three launches of d3r_prepare_views alone (events around the call into the library), sources resident in HBM, with the
            bytes they must move (source crops read once + results written once) over the measured HBM copy rate
  call      the same prepare_views call as the host sees it (plans, table lookup, allocations, enqueue), sources resident
  batch     the whole batch from decoded host arrays: upload of every source, then the call
  host      the same pipeline as PIL + numpy per view on 16 host threads (the reference's route)
--evaluate: evaluate() in pairs/s over a loader with in-memory distinct sources against evaluate() over the same batches pre-collated
and resident. Shader clock and power are sampled while each GPU figure is taken (bench.py's Telemetry)."""
import argparse
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import PIL.Image
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench import Telemetry  # noqa: E402
from dust3r_amd.datasets import SyntheticStereo, get_data_loader  # noqa: E402
from dust3r_amd.datasets.prepare import prepare_views  # noqa: E402
from dust3r_amd.datasets.synthetic import synthetic_view  # noqa: E402
from dust3r_amd.datasets.utils.cropping import nearest_indices  # noqa: E402

HBM_COPY = 6.29e12      # measured float4 copy rate of the MI355X (bytes / s)


class DistinctSources(SyntheticStereo):
    """One source per view of the dataset, each an array of its own with contents of its own, held in memory."""

    def __init__(self, W, H, n_pairs, **kwargs):
        super().__init__([(W, H, (0.5, 0.5))], n_pairs, **kwargs)
        base = [synthetic_view(7, W, H, (0.5, 0.5)), synthetic_view(8, W, H, (0.48, 0.52))]
        self._views = []
        for k in range(2 * n_pairs):
            b = base[k % 2]
            self._views.append(dict(b, rgb=b['rgb'] + np.uint8((3 * k) % 256), depth=np.roll(b['depth'], k, axis=1).copy()))

    def _source(self, idx, v):
        return self._views[2 * idx + v]


def spread(values):
    return float(np.median(values)), float(np.min(values)), float(np.max(values))


def timed(fn, repeats, warmup=2):
    out = []
    for i in range(warmup + repeats):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if i >= warmup:
            out.append((time.perf_counter() - t) * 1e3)
    return spread(out)


def host_view(view):
    """The reference's per-view route: crop, PIL resize, crop, normalise, nearest depth, back-projection in numpy."""
    plan, rgb, depth = view['img'].plan, view['img'].source, view['depthmap'].source
    pil = PIL.Image.fromarray(rgb).crop(plan.crop1).resize(plan.resample_size, PIL.Image.LANCZOS if plan.filter == 'lanczos' else PIL.Image.BICUBIC).crop(plan.crop2)
    img = (torch.from_numpy(np.array(pil)).permute(2, 0, 1).float().div(255) - 0.5) / 0.5
    sy, sx = nearest_indices(plan)
    z = depth[sy[:, None], sx[None, :]]
    K, pose = view['K_pixels'], view['camera_pose']
    u, v = np.meshgrid(np.arange(z.shape[1]), np.arange(z.shape[0]))
    X = np.stack(((u - K[0, 2]) * z / K[0, 0], (v - K[1, 2]) * z / K[1, 1], z), axis=-1).astype(np.float32)
    pts = np.einsum('ik, vuk -> vui', pose[:3, :3], X) + pose[:3, 3]
    return img, z, pts, (z > 0) & np.isfinite(pts).all(axis=-1)


def clocks(t):
    return 'no telemetry' if not t else f"sclk {t['sclk_mhz_mean']:.0f} MHz mean [{t['sclk_mhz_min']:.0f}, {t['sclk_mhz_max']:.0f}], {t['power_w_mean']:.0f} W mean"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--pairs', type=int, default=32)
    ap.add_argument('--big-pairs', type=int, default=32, help='pairs of the 4032x3024 case (64 such sources are 5.5 GB of host memory)')
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--evaluate', action='store_true')
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    for (W0, H0), pairs in (((640, 480), args.pairs), ((4032, 3024), args.big_pairs)):
        ds = DistinctSources(W0, H0, pairs, resolution=(512, 384), seed=1)
        plan_views = lambda: [v for i in range(pairs) for v in ds.planned_views(i)]      # noqa: E731
        n = 2 * pairs
        assert len({id(v['img'].source) for v in plan_views()}) == n
        src_bytes = sum((p.crop1[2] - p.crop1[0]) * (p.crop1[3] - p.crop1[1]) * 3 for p in (v['img'].plan for v in plan_views())) + n * 512 * 384 * 32   # a 32-byte sector per depth sample
        out_bytes = n * 512 * 384 * (12 + 4 + 12 + 1)
        upload_bytes = n * W0 * H0 * 7
        tele = Telemetry(dev).start()
        resident, kernel_ms, call_ms = {}, [], []
        planned = [plan_views() for _ in range(args.repeats + 2)]      # planned beforehand: the calls run back to back, so the chip does not idle down to its sleep clock between them
        for i in range(args.repeats + 2):
            views, timing = planned[i], {}
            torch.cuda.synchronize()
            t = time.perf_counter()
            prepare_views(views, dev, resident=resident, timing=timing)
            torch.cuda.synchronize()
            if i >= 2:
                call_ms.append((time.perf_counter() - t) * 1e3)
                kernel_ms.append(timing['kernels'][0].elapsed_time(timing['kernels'][1]))
        k_tele = tele.stop()
        resident.clear()
        tele = Telemetry(dev).start()
        whole = timed(lambda: prepare_views(plan_views(), dev), args.repeats)
        w_tele = tele.stop()
        plan_ms = timed(plan_views, 3, warmup=1)
        with ThreadPoolExecutor(16) as pool:
            host = timed(lambda: list(pool.map(host_view, plan_views())), 3, warmup=1)
        floor_ms = (src_bytes + out_bytes) / HBM_COPY * 1e3
        k, c = spread(kernel_ms), spread(call_ms)
        print(f'{W0}x{H0} -> 512x384, {pairs} pairs, {n} distinct sources ({upload_bytes / 1e6:.0f} MB rgb + fp32 depth), median [min, max] ms:\n'
              f'  kernels {k[0]:.3f} [{k[1]:.3f}, {k[2]:.3f}]; must move {(src_bytes + out_bytes) / 1e6:.0f} MB = {floor_ms:.3f} ms at the copy rate: {k[0] / floor_ms:.1f}x ({clocks(k_tele)})\n'
              f'  call, sources resident {c[0]:.2f} [{c[1]:.2f}, {c[2]:.2f}] (of which planning on one thread {plan_ms[0]:.2f})\n'
              f'  batch from host arrays {whole[0]:.1f} [{whole[1]:.1f}, {whole[2]:.1f}] = upload at {upload_bytes / 1e6 / max(whole[0] - c[0], 1e-3):.1f} GB/s + call ({clocks(w_tele)})\n'
              f'  PIL + numpy on 16 threads {host[0]:.1f} [{host[1]:.1f}, {host[2]:.1f}]', flush=True)
        del ds
    if args.evaluate:
        import dust3r_amd.losses as L
        from dust3r_amd.evaluation import evaluate
        from dust3r_amd.model import AsymmetricCroCo3DStereo
        from dust3r_amd.synthetic import MODEL_CONFIGS, OUT_GAIN, synthetic_state_dict
        cfg = 'DUSt3R_ViTLarge_BaseDecoder_512_dpt'
        model = AsymmetricCroCo3DStereo(landscape_only=False, **MODEL_CONFIGS[cfg])
        model.load_state_dict(synthetic_state_dict({k: torch.empty(v, device='meta') for k, v in model._spec.items()}, 0, OUT_GAIN[cfg], device=dev))
        model = model.to(dev)
        crit = eval("Regr3D_ScaleShiftInv(L21, gt_scale=True)", vars(L))
        total = 4 * args.pairs
        ds = DistinctSources(640, 480, total, resolution=(512, 384), seed=1)
        loader = get_data_loader(ds, batch_size=args.pairs, num_workers=16, device=dev)
        loader.sampler.set_epoch(0)
        resident = list(loader)
        for sym in (True, False):
            for name, batches in (('resident', lambda: resident), ('loader', lambda: loader)):
                rates, tele = [], Telemetry(dev).start()
                for _ in range(4):
                    torch.cuda.synchronize()
                    t = time.perf_counter()
                    evaluate(model, crit, batches(), dev, symmetrize_batch=sym)
                    torch.cuda.synchronize()
                    rates.append(total / (time.perf_counter() - t))
                print(f'evaluate, {total} pairs, symmetrize_batch={sym}, {name} batches: {np.median(rates[1:]):.1f} pairs/s {["%.1f" % r for r in rates]} ({clocks(tele.stop())})', flush=True)


if __name__ == '__main__':
    main()
