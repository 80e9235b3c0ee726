"""Times scene.fuse() on the 100-view 512 x 384 scene of tools/glb_speed.py (geometry resident on the GPU, masks keep ~70 % of the pixels):
- calls: device events around d3r_fuse_bounds and d3r_fuse_voxels alone (inputs, outputs and workspace allocated), medians after warm-up,
  and the bytes each stage has to move (from the shapes) against the measured device-to-device copy rate;
- scene.fuse(): host clock from the scene to the host arrays; save_ply and write_colmap to /dev/shm;
- comparators: the numpy restatement of tests/test_fuse_cpu.py on the host (numpy's sort and bincount are single-threaded; --threads only
  bounds the BLAS / OpenMP pools), and the same pipeline as torch ops on the same GPU (torch.sort, unique_consecutive, index_add_).
Per-kernel device times come from a kernel trace taken in a run of its own:

    python tools/fuse_speed.py [--views 100] [--reps 7] [--threads 16]          # the table above, one JSON line per row
    <profiler> --kernel-trace ... -- python tools/fuse_speed.py --profile-run    # three calls after warm-up, nothing else
    python tools/fuse_speed.py --summarise <kernel_trace.csv>                    # per stage and per sort pass, median over the calls"""
import argparse
import csv
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests'), os.path.join(ROOT, 'tools')]

import numpy as np  # noqa: E402

STAGES = ('bounds', 'key+compact', 'sort', 'heads', 'reduce')


def stage_of(kernel_name):
    """the stage a kernel of csrc/fuse.hip belongs to, from its (mangled or demangled) name; None for other kernels"""
    if 'fuse_bounds' in kernel_name:
        return 'bounds'
    if 'fuse_hist' in kernel_name or 'fuse_scatter' in kernel_name:
        return 'sort'
    if 'fuse_reduce' in kernel_name:
        return 'reduce'
    if 'fuse_flag' in kernel_name:
        return 'heads' if ('ILi1E' in kernel_name or '<1' in kernel_name.replace(' ', '')) else 'key+compact'
    if 'fuse_scan' in kernel_name:
        return 'scan'
    return None


def summarise(path):
    """Groups the dispatches of a kernel trace into calls (a call starts at fuse_bounds_kernel) and stages; a scan belongs to the stage of the
    kernel before it, a sort pass is hist + scan + scatter. Prints the median over the calls of every stage and of every sort pass."""
    rows = list(csv.DictReader(open(path)))
    rows = [r for r in rows if stage_of(r['Kernel_Name'])]
    rows.sort(key=lambda r: int(r['Start_Timestamp']))
    calls, cur = [], None
    for r in rows:
        name = r['Kernel_Name']
        us = (int(r['End_Timestamp']) - int(r['Start_Timestamp'])) / 1e3
        st = stage_of(name)
        if st == 'bounds' and 'final' not in name:
            cur = dict(stages={s: 0.0 for s in STAGES}, passes=[], last='bounds', launches=0)
            calls.append(cur)
        if cur is None:
            continue
        if st == 'scan':
            st = cur['last']
        if st == 'sort':
            if 'fuse_hist' in name:
                cur['passes'].append(0.0)
            cur['passes'][-1] += us
        cur['stages'][st] += us
        cur['last'] = st
        cur['launches'] += 1
    calls = [c for c in calls if c['stages']['reduce'] > 0]
    if not calls:
        raise SystemExit(f'{path}: no complete fuse call in the trace')
    out = dict(calls=len(calls), launches_per_call=calls[-1]['launches'], sort_passes=len(calls[-1]['passes']))
    for s in STAGES:
        out[f'{s}_us'] = round(statistics.median(c['stages'][s] for c in calls), 1)
    out['total_us'] = round(statistics.median(sum(c['stages'].values()) for c in calls), 1)
    out['sort_pass_us'] = [round(statistics.median(c['passes'][k] for c in calls), 1) for k in range(len(calls[-1]['passes']))]
    print(json.dumps(out), flush=True)
    return out


def stage_bytes(n_pix, n_valid, n_voxels, passes, float_rgb=True):
    """what each stage has to read and write, from the shapes: pixels (mask 1 B, weight 4 B, point 12 B), pairs (key 8 B, index 4 B)"""
    pix = n_pix * (1 + 4) + n_valid * 12
    return {'bounds': pix, 'key+compact': 2 * pix + n_valid * 12, 'sort': passes * n_valid * (8 + 12 + 12), 'heads': 2 * n_valid * 8 + n_voxels * 4,
            'reduce': n_valid * (4 + 12 + 4 + (12 if float_rgb else 3)) + n_voxels * 4 + n_voxels * 24}


def torch_fuse(pts, mask, weight, rgb, voxel):
    """the same pipeline as torch ops on the device (float colours quantised by the export's rule first); index_add_ adds in no fixed order"""
    import torch
    valid = (mask != 0) & torch.isfinite(pts).all(dim=-1) & torch.isfinite(weight) & (weight > 0)
    P, w = pts[valid], weight[valid].double()
    q = (rgb[valid] * 255 + 0.5).floor().clamp(0, 255).double()
    lo, hi = P.min(dim=0).values, P.max(dim=0).values
    ext = ((hi - lo) / voxel).floor().cpu().numpy()
    bits = [max(1, int(e).bit_length()) for e in ext]
    cell = ((P - lo) / voxel).floor().long()
    key = cell[:, 0] | (cell[:, 1] << bits[0]) | (cell[:, 2] << (bits[0] + bits[1]))
    ks, order = torch.sort(key, stable=True)
    _, inv, counts = torch.unique_consecutive(ks, return_inverse=True, return_counts=True)
    M = len(counts)
    wo = w[order]
    W = torch.zeros(M, dtype=torch.float64, device=pts.device).index_add_(0, inv, wo)
    S = torch.zeros((M, 3), dtype=torch.float64, device=pts.device).index_add_(0, inv, wo[:, None] * P[order].double())
    C = torch.zeros((M, 3), dtype=torch.float64, device=pts.device).index_add_(0, inv, wo[:, None] * q[order])
    return (S / W[:, None]).float(), (C / W[:, None] + 0.5).floor().clamp(0, 255).to(torch.uint8), W.float(), counts.int()


def median_ms(fn, reps, sync):
    ts = []
    for _ in range(reps):
        sync()
        t0 = time.perf_counter()
        fn()
        sync()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--views', type=int, default=100)
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--threads', type=int, default=16)
    ap.add_argument('--voxel', type=float, default=None, help='default: the scene\'s median pixel footprint')
    ap.add_argument('--profile-run', action='store_true')
    ap.add_argument('--summarise', default=None, metavar='CSV')
    ap.add_argument('--skip-host', action='store_true', help='leave the numpy restatement out')
    args = ap.parse_args()
    if args.summarise:
        return summarise(args.summarise)
    import ctypes as C
    import torch
    torch.set_num_threads(args.threads)
    from dust3r_amd import _lib
    from dust3r_amd._lib import check, current_stream, lib, ptr
    from dust3r_amd.export import write_colmap
    from dust3r_amd.viz import default_voxel_size, fuse_key_bits, fuse_points
    from glb_speed import make_scene
    _lib.require_device()
    dev = torch.device('cuda:0')
    n, H, W = args.views, 384, 512
    scene = make_scene(n, H, W, dev)
    with torch.no_grad():
        pts = scene.get_pts3d(raw=True).contiguous()
        scene.min_conf_thr = float(scene.conf_trf(torch.tensor(3.0)))
        mask = scene.get_masks(raw=True).to(torch.uint8)
        weight = scene._im_conf
        voxel = args.voxel or default_voxel_size(scene.get_depthmaps(raw=True), [H * W] * n, scene.get_focals())
    A = pts.shape[1]
    rgb = torch.from_numpy(np.stack(scene.imgs)).reshape(n, A, 3).to(dev)
    hs, ws = scene._shape_tables[:2]
    sync = torch.cuda.synchronize

    if args.profile_run:
        for _ in range(5):
            fuse_points(scene.imgs, pts, mask, weight, voxel, dev, to_host=False)
        sync()
        return None

    # the two calls alone
    small = torch.empty(4, dtype=torch.int64, device=dev)
    work_b = torch.empty(int(lib.d3r_fuse_bounds_workspace_bytes(n, A)), dtype=torch.uint8, device=dev)

    def bounds():
        check(lib.d3r_fuse_bounds(n, ptr(pts), ptr(mask), ptr(weight), ptr(hs), ptr(ws), A, ptr(small.view(torch.float32)), ptr(small[3:]), ptr(work_b),
                                  current_stream()), 'fuse_bounds')
    bounds()
    host = small.cpu()
    lo, hi, n_valid = host[:3].view(torch.float32).numpy()[:3].copy(), host[:3].view(torch.float32).numpy()[3:].copy(), int(host[3])
    bits = fuse_key_bits(lo, hi, voxel)
    out = [torch.empty((n_valid, 3), device=dev), torch.empty(n_valid, dtype=torch.int32, device=dev), torch.empty(n_valid, device=dev),
           torch.empty(n_valid, dtype=torch.int32, device=dev), torch.empty(2, dtype=torch.int64, device=dev)]
    work_v = torch.empty(int(lib.d3r_fuse_voxels_workspace_bytes(n, A, n_valid)), dtype=torch.uint8, device=dev)
    lo_c, bits_c = (C.c_float * 3)(*lo.tolist()), (C.c_int * 3)(*bits)

    def voxels():
        check(lib.d3r_fuse_voxels(n, ptr(pts), ptr(mask), ptr(weight), ptr(rgb), 0, ptr(hs), ptr(ws), A, lo_c, float(voxel), bits_c, n_valid, ptr(out[0]),
                                  ptr(out[1]), ptr(out[2]), ptr(out[3]), ptr(out[4]), ptr(work_v), current_stream()), 'fuse_voxels')

    def device_ms(fn):
        for _ in range(3):
            fn()
        sync()
        ts = []
        for _ in range(args.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            sync()
            ts.append(e0.elapsed_time(e1))
        return statistics.median(ts)
    bounds_ms, voxels_ms = device_ms(bounds), device_ms(voxels)
    n_voxels = int(out[4].cpu()[1])
    passes = -(-sum(bits) // 4)
    src = torch.empty(2 ** 28, dtype=torch.uint8, device=dev)
    dst = torch.empty_like(src)
    copy_ms = device_ms(lambda: dst.copy_(src))
    copy_gbs = 2 * src.numel() / copy_ms / 1e6                         # read + write
    del src, dst
    nbytes = stage_bytes(n * A, n_valid, n_voxels, passes)
    print(json.dumps(dict(row='calls', views=n, H=H, W=W, pixels=n * A, valid=n_valid, voxels=n_voxels, voxel_size=float(voxel), key_bits=bits,
                          sort_passes=passes, bounds_ms=round(bounds_ms, 3), voxels_ms=round(voxels_ms, 3),
                          workspace_MB=round((work_b.numel() + work_v.numel()) / 2 ** 20, 1), copy_GBps=round(copy_gbs, 1),
                          stage_MB={k: round(v / 1e6, 1) for k, v in nbytes.items()},
                          bounds_GBps=round(nbytes['bounds'] / bounds_ms / 1e6, 1),
                          voxels_GBps=round(sum(v for k, v in nbytes.items() if k != 'bounds') / voxels_ms / 1e6, 1))), flush=True)
    del out, work_v, work_b

    # the whole call, and the files
    with torch.no_grad():
        scene.fuse(voxel_size=voxel)
        fuse_ms = median_ms(lambda: scene.fuse(voxel_size=voxel), args.reps, sync)
        cloud = scene.fuse(voxel_size=voxel)
    outdir = tempfile.mkdtemp(dir='/dev/shm' if os.path.isdir('/dev/shm') else tempfile.gettempdir())
    t0 = time.perf_counter()
    ply = cloud.save_ply(os.path.join(outdir, 'scene.ply'))
    ply_ms = (time.perf_counter() - t0) * 1e3
    ply_mb = os.path.getsize(ply) / 2 ** 20
    t0 = time.perf_counter()
    files = write_colmap(os.path.join(outdir, 'colmap'), scene, cloud)
    colmap_ms = (time.perf_counter() - t0) * 1e3
    colmap_mb = sum(os.path.getsize(f) for f in files) / 2 ** 20
    for f in [ply] + files:
        os.remove(f)
    print(json.dumps(dict(row='scene.fuse', views=n, points=len(cloud), scene_fuse_to_host_ms=round(fuse_ms, 1), save_ply_ms=round(ply_ms, 1),
                          ply_MB=round(ply_mb, 1), write_colmap_ms=round(colmap_ms, 1), colmap_MB=round(colmap_mb, 1))), flush=True)

    # comparators
    with torch.no_grad():
        torch_fuse(pts, mask, weight, rgb, voxel)
        torch_ms = median_ms(lambda: torch_fuse(pts, mask, weight, rgb, voxel), args.reps, sync)
        got = torch_fuse(pts, mask, weight, rgb, voxel)
    same = len(got[0]) == len(cloud) and bool(np.array_equal(got[3].cpu().numpy(), cloud.count))
    row = dict(row='comparators', views=n, torch_ops_ms=round(torch_ms, 1), torch_same_voxels=same,
               torch_max_position_diff=float(np.abs(got[0].cpu().numpy() - cloud.positions).max()) if same else None)
    del got
    if not args.skip_host:
        from test_fuse_cpu import restated_fuse
        with torch.no_grad():
            host_pts = [p.cpu().numpy() for p in scene.get_pts3d()]
            host_msk = [m.cpu().numpy() for m in scene.get_masks()]
            host_w = [c.cpu().numpy() for c in scene.im_conf]
        t0 = time.perf_counter()
        want = restated_fuse(scene.imgs, host_pts, host_msk, host_w, voxel)
        row.update(host_threads=args.threads, host_restatement_ms=round((time.perf_counter() - t0) * 1e3, 1),
                   equals_restatement=all(bool(np.array_equal(getattr(cloud, k), want[k])) for k in ('positions', 'colors', 'weight', 'count')))
    print(json.dumps(row), flush=True)
    return None


if __name__ == '__main__':
    main()
