"""Times the demo's depth / confidence gallery (d3r_scene_gallery, dust3r_amd/demo.py) for 100 views of 512 x 384 against the formulae of the
reference's get_reconstructed_scene (dust3r/demo.py:168-184) in numpy + matplotlib on a pool of host threads, and checks that both agree.

    python tools/demo_speed.py [--views 100] [--threads 16] [--reps 500]

GPU: device events around the two kernels alone (stacks already on the GPU, outputs and workspace allocated), and a host clock around the
call plus the copies into host arrays (what scene_gallery does after reading the scene). Host: wall clock of the formulae over all images,
one image per task (the two maxima first, as the reference does); without matplotlib the colour map is this package's table (said in the
output). The share of the HBM floor: the bytes the two kernels must move -- pass 1 reads both stacks, pass 2 reads them again and writes
one fp32 and one 4 x fp32 picture per pixel: 36 bytes per pixel -- over the 8 TB/s peak, over the measured kernel time."""
import argparse
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from dust3r_amd import _lib  # noqa: E402
from dust3r_amd._lib import check, current_stream, lib, ptr  # noqa: E402
from dust3r_amd.demo import _device_table, gallery_images, gallery_table  # noqa: E402
from dust3r_amd.utils.device import host_tensor  # noqa: E402

HBM_PEAK = 8.0e12           # bytes / s (MI355X specification); about 6.3e12 is what a streaming kernel reaches
BYTES_PER_PIXEL = 2 * 4 + 2 * 4 + 4 + 16


def host_colour_map():
    try:
        import matplotlib
        cmap = matplotlib.colormaps['jet']
        return (lambda x: cmap(x)), f'matplotlib {matplotlib.__version__}'
    except ImportError:
        from test_demo_gpu import restated_index
        lut = (gallery_table().astype(np.float64) - 0.5) * 2
        return (lambda x: lut[restated_index(x)]), "this package's table (matplotlib is not installed)"


def rgb(x):
    return ((x * 0.5) + 0.5).clip(min=0, max=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--views', type=int, default=100)
    ap.add_argument('--threads', type=int, default=16)
    ap.add_argument('--reps', type=int, default=500)
    args = ap.parse_args()
    _lib.require_device()
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    dev = torch.device('cuda:0')
    n, H, W = args.views, 384, 512
    A = H * W
    g = torch.Generator(device=dev).manual_seed(0)
    depth = torch.exp(torch.randn((n, A), generator=g, device=dev) / 2)
    conf = 1 + torch.exp(torch.randn((n, A), generator=g, device=dev))
    npix = torch.full((n,), A, dtype=torch.int32, device=dev)
    table = _device_table(dev)
    out_d = torch.empty((n, A), dtype=torch.float32, device=dev)
    out_c = torch.empty((n, A, 4), dtype=torch.float32, device=dev)
    maxima = torch.empty((2,), dtype=torch.float32, device=dev)
    work = torch.empty(int(lib.d3r_scene_gallery_workspace_bytes(n, A)), dtype=torch.uint8, device=dev)

    def launch():
        check(lib.d3r_scene_gallery(n, ptr(depth), ptr(conf), ptr(npix), A, ptr(table), ptr(out_d), ptr(out_c), ptr(maxima), ptr(work), current_stream()),
              'scene_gallery')
    for _ in range(5):
        launch()
    torch.cuda.synchronize()
    times = []
    for _ in range(3):                                   # three windows: the spread
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.reps):
            launch()
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1) / args.reps)
    kernel_ms = sorted(times)[1]

    # the call and the copies into host arrays
    host_d, host_c = host_tensor((n, A)), host_tensor((n, A, 4))

    def to_host():
        d, c, _ = gallery_images(depth, conf, npix)
        host_d.copy_(d)
        host_c.copy_(c)
        torch.cuda.synchronize()
    to_host()
    t0 = time.perf_counter()
    for _ in range(5):
        to_host()
    call_ms = (time.perf_counter() - t0) * 1e3 / 5

    # the reference's formulae on the host
    cmap, cmap_name = host_colour_map()
    depths, confs = list(depth.cpu().numpy().reshape(n, H, W)), list(conf.cpu().numpy().reshape(n, H, W))

    def per_image(i, dmax, cmax):
        return rgb(depths[i] / dmax), rgb(cmap(confs[i] / cmax))

    def host_run(ex):
        dmax = max(ex.map(lambda d: d.max(), depths))
        cmax = max(ex.map(lambda c: c.max(), confs))
        return list(ex.map(lambda i: per_image(i, dmax, cmax), range(n))), (dmax, cmax)
    with ThreadPoolExecutor(args.threads) as ex:
        host_run(ex)
        t0 = time.perf_counter()
        ref, ref_max = host_run(ex)
        host_ms = (time.perf_counter() - t0) * 1e3
    got_d, got_c = host_d.numpy().reshape(n, H, W), host_c.numpy().reshape(n, H, W, 4)
    same = maxima.cpu().tolist() == [float(ref_max[0]), float(ref_max[1])]
    same = same and all(np.array_equal(got_d[i], ref[i][0]) and np.array_equal(got_c[i], np.float32(ref[i][1])) for i in range(n))
    floor_ms = n * A * BYTES_PER_PIXEL / HBM_PEAK * 1e3
    row = dict(views=n, H=H, W=W, gpu_kernels_ms=round(kernel_ms, 4), gpu_kernels_ms_windows=[round(t, 4) for t in times],
               bytes_moved=n * A * BYTES_PER_PIXEL, achieved_TBps=round(n * A * BYTES_PER_PIXEL / (kernel_ms * 1e-3) / 1e12, 3),
               hbm_floor_ms_at_8TBps=round(floor_ms, 4), share_of_hbm_floor=round(floor_ms / kernel_ms, 3),
               gpu_call_to_host_arrays_ms=round(call_ms, 2), host_threads=args.threads, host_colour_map=cmap_name,
               host_formulae_ms=round(host_ms, 1), identical=bool(same))
    print(json.dumps(row), flush=True)
    assert same, 'GPU gallery differs from the host formulae'
    return row


if __name__ == '__main__':
    main()
