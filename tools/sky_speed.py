"""Times the batched GPU sky segmentation (d3r_segment_sky, dust3r_amd/viz.py) of 20 and 100 pictures of 512 x 384 against the numpy / SciPy
restatement of the reference's per-image segment_sky (tests/test_sky_cpu.py) on a pool of host threads, and checks that both agree.

    python tools/sky_speed.py [--threads 16] [--reps 20]

GPU: device events around the kernels alone (pictures already on the GPU, workspace allocated), and a host clock around the whole
segment_sky_batch call from numpy (upload included). Host: wall clock of the restatement over all pictures, one picture per task."""
import argparse
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]

import numpy as np  # noqa: E402
import torch  # noqa: E402

from dust3r_amd import _lib  # noqa: E402
from dust3r_amd._lib import check, current_stream, lib, ptr  # noqa: E402
from dust3r_amd.viz import segment_sky_batch  # noqa: E402
from dust3r_amd.synthetic import outdoor_scene  # noqa: E402
# the one restatement of the reference's segment_sky, which the GPU tests also hold the kernels to
from test_sky_cpu import restated_segment_sky  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--threads', type=int, default=16)
    ap.add_argument('--reps', type=int, default=20)
    args = ap.parse_args()
    _lib.require_device()
    dev = torch.device('cuda:0')
    H, W = 384, 512
    results = []
    for n in (20, 100):
        imgs = [outdoor_scene(H, W, seed=k, horizon=0.3 + 0.4 * (k % 5) / 4) for k in range(n)]
        f32 = [im.astype(np.float32) / 255 for im in imgs]                    # the layout of scene.imgs
        # GPU, kernels only
        rgb = torch.from_numpy(np.stack(f32)).reshape(n, H * W, 3).to(dev)
        hs = torch.full((n,), H, dtype=torch.int32, device=dev)
        ws = torch.full((n,), W, dtype=torch.int32, device=dev)
        out = torch.empty((n, H * W), dtype=torch.uint8, device=dev)
        work = torch.empty(int(lib.d3r_segment_sky_workspace_bytes(n, H * W)), dtype=torch.uint8, device=dev)

        def launch():
            check(lib.d3r_segment_sky(n, ptr(rgb), 0, ptr(hs), ptr(ws), H * W, ptr(out), ptr(work), current_stream()), 'segment_sky')
        for _ in range(3):
            launch()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.reps):
            launch()
        e1.record()
        torch.cuda.synchronize()
        kernel_ms = e0.elapsed_time(e1) / args.reps
        # GPU, the whole call from host pictures
        segment_sky_batch(f32, dev)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.reps):
            masks = segment_sky_batch(f32, dev)
        torch.cuda.synchronize()
        call_ms = (time.perf_counter() - t0) * 1e3 / args.reps
        # host restatement
        with ThreadPoolExecutor(args.threads) as ex:
            list(ex.map(restated_segment_sky, f32[:args.threads]))
            t0 = time.perf_counter()
            ref = list(ex.map(restated_segment_sky, f32))
            host_ms = (time.perf_counter() - t0) * 1e3
        same = all(np.array_equal(m.cpu().numpy(), r) for m, r in zip(masks, ref))
        same = same and np.array_equal(out.view(n, H, W).cpu().numpy().astype(bool), np.stack(ref))
        row = dict(images=n, H=H, W=W, gpu_kernels_ms=round(kernel_ms, 3), gpu_call_ms=round(call_ms, 3), host_threads=args.threads,
                   host_restatement_ms=round(host_ms, 1), identical=bool(same))
        print(json.dumps(row), flush=True)
        results.append(row)
        assert same, 'GPU masks differ from the restatement'
    return results


if __name__ == '__main__':
    main()
