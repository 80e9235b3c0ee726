"""Times the cloud-to-cloud metrics (dust3r_amd/cloud_metrics.py, csrc/cloud_nn.hip) on the 100-view 512 x 384 scene of tools/glb_speed.py:
the scene is fused, then fused again with seeded noise of half a voxel on its points -- two clouds of the same size, about a voxel apart.
- ladder: device events around d3r_cloud_grid_build and d3r_cloud_nearest of every pass of the radius ladder (pred -> gt), the distance
  evaluations per query (the kernel's own counter) and per second, the queries each pass resolved;
- stats: d3r_cloud_distance_stats and d3r_masked_median alone;
- cloud_metrics: host clock around the whole call, both directions, to the dict;
- pointmap: the exhaustive d3r_nearest_neighbors at 196 608 x 196 608 (two views of the scene) against the grid at the same size, max_dist
  so large that every query is resolved (the two answer the same question then), and whether they agree;
- host: scipy.spatial.cKDTree(...).query(workers=threads, distance_upper_bound=max_dist) on the same clouds, at the full size when --host-full,
  else at --host-points points per side.
Per-kernel device times come from a kernel trace taken in a run of its own:

    python tools/cloud_metrics_speed.py [--views 100] [--reps 5] [--threads 16]           # the rows above, one JSON line each
    <profiler> --kernel-trace ... -- python tools/cloud_metrics_speed.py --profile-run     # two nearest_in_cloud calls after warm-up
    python tools/cloud_metrics_speed.py --summarise <kernel_trace.csv>                     # per stage, per call"""
import argparse
import csv
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests'), os.path.join(ROOT, 'tools')]

import numpy as np  # noqa: E402

STAGES = ('bounds', 'key+compact', 'sort', 'heads', 'gather+cells', 'init', 'query')


def stage_of(name):
    """the stage a kernel of csrc/cloud_nn.hip / cloud_knn.hip / fuse_grid.hpp belongs to, from its (mangled or demangled) name; None for other kernels"""
    for key, stage in (('fuse_bounds', 'bounds'), ('fuse_hist', 'sort'), ('fuse_scatter', 'sort'), ('cloud_gather', 'gather+cells'),
                       ('cloud_cells', 'gather+cells'), ('cloud_knn_init', 'init'), ('cloud_shape', 'init'), ('cloud_knn_kernel', 'query'), ('fuse_scan', 'scan')):
        if key in name:
            return stage
    if 'fuse_flag' in name:
        return 'heads' if ('ILi1E' in name or '<1' in name.replace(' ', '')) else 'key+compact'
    return None


def summarise(path):
    """Groups the dispatches of a kernel trace into calls (a call starts at fuse_bounds_kernel; only those that reach cloud_knn_kernel count)
    and stages (a scan belongs to the stage of the kernel before it). Prints the median over the calls of every stage."""
    rows = [r for r in csv.DictReader(open(path)) if stage_of(r['Kernel_Name'])]
    rows.sort(key=lambda r: int(r['Start_Timestamp']))
    calls, cur = [], None
    for r in rows:
        st = stage_of(r['Kernel_Name'])
        if st == 'bounds' and 'final' not in r['Kernel_Name']:
            cur = dict(stages={s: 0.0 for s in STAGES}, last='bounds', launches=0)
            calls.append(cur)
        if cur is None:
            continue
        st = cur['last'] if st == 'scan' else st
        cur['stages'][st] += (int(r['End_Timestamp']) - int(r['Start_Timestamp'])) / 1e3
        cur['last'] = st
        cur['launches'] += 1
    calls = [c for c in calls if c['stages']['query'] > 0]             # (scene.fuse() starts with the bounds kernels too)
    if not calls:
        raise SystemExit(f'{path}: no nearest_in_cloud call in the trace')
    out = dict(calls=len(calls), launches_per_call=calls[-1]['launches'])
    for s in STAGES:
        out[f'{s}_us'] = round(statistics.median(c['stages'][s] for c in calls), 1)
    out['total_us'] = round(statistics.median(sum(c['stages'].values()) for c in calls), 1)
    print(json.dumps(out), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--views', type=int, default=100)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--threads', type=int, default=16)
    ap.add_argument('--host-points', type=int, default=1000000)
    ap.add_argument('--host-full', action='store_true', help='the KD-tree at the full size too')
    ap.add_argument('--skip-host', action='store_true')
    ap.add_argument('--profile-run', action='store_true')
    ap.add_argument('--summarise', default=None, metavar='CSV')
    args = ap.parse_args()
    if args.summarise:
        return summarise(args.summarise)
    import ctypes as C
    import torch
    torch.set_num_threads(args.threads)
    from dust3r_amd import _lib
    from dust3r_amd._lib import check, current_stream, lib, ptr
    from dust3r_amd.cloud_metrics import _bounds, cloud_metrics, distance_stats, grid_cell, ladder_radii, nearest_in_cloud
    from dust3r_amd.viz import default_voxel_size, fuse_points
    from glb_speed import make_scene
    _lib.require_device()
    dev = torch.device('cuda:0')
    n, H, W = args.views, 384, 512
    sync = torch.cuda.synchronize
    scene = make_scene(n, H, W, dev)
    with torch.no_grad():
        pts = scene.get_pts3d(raw=True).contiguous()
        scene.min_conf_thr = float(scene.conf_trf(torch.tensor(3.0)))
        mask = scene.get_masks(raw=True).to(torch.uint8)
        voxel = default_voxel_size(scene.get_depthmaps(raw=True), [H * W] * n, scene.get_focals())
        g = torch.Generator(device=dev).manual_seed(7)
        noisy = pts + 0.5 * voxel * torch.randn(pts.shape, device=dev, generator=g)
        gt = fuse_points(scene.imgs, pts, mask, scene._im_conf, voxel, dev, to_host=False)
        pred = fuse_points(scene.imgs, noisy, mask, scene._im_conf, voxel, dev, to_host=False)
    del noisy
    max_dist, thresholds = 16 * voxel, [voxel, 2 * voxel, 4 * voxel]
    P, G = pred.positions.contiguous(), gt.positions.contiguous()
    nq, nr = len(P), len(G)

    if args.profile_run:
        for _ in range(4):
            nearest_in_cloud(P, G, max_dist, r0=2 * voxel, to_host=False)
        sync()
        return None

    def device_ms(fn, reps=args.reps, warm=2):
        for _ in range(warm):
            fn()
        sync()
        ts = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            sync()
            ts.append(e0.elapsed_time(e1))
        return statistics.median(ts)

    # the ladder, pass by pass (what nearest_in_cloud does, with events around the two calls)
    lo, hi, n_valid = _bounds(G, dev)
    work = torch.empty(int(lib.d3r_cloud_grid_workspace_bytes(nr, nq)), dtype=torch.uint8, device=dev)
    lo_c = (C.c_float * 3)(*lo.tolist())
    d2 = torch.empty(nq, dtype=torch.float32, device=dev)
    idx = torch.empty(nq, dtype=torch.int32, device=dev)
    evals = torch.zeros(nq, dtype=torch.int32, device=dev)
    passes, total_ms, total_evals = [], 0.0, 0
    state = None
    for k, r in enumerate(ladder_radii(2 * voxel, max_dist)):
        cell, bits = grid_cell(lo, hi, r)
        bits_c = (C.c_int * 3)(*bits)
        if k == 0:
            d2.fill_(float('inf'))
            idx.fill_(-1)
        state = (d2.clone(), idx.clone())                              # every repetition of a pass starts from what the pass before left

        def build():
            check(lib.d3r_cloud_grid_build(nr, ptr(G), lo_c, float(cell), bits_c, ptr(work), current_stream()), 'cloud_grid_build')

        def query(count=None):
            d2.copy_(state[0])
            idx.copy_(state[1])
            check(lib.d3r_cloud_nearest(nr, nq, ptr(P), float(r), lo_c, float(cell), bits_c, int(k > 0), ptr(d2), ptr(idx), ptr(count), ptr(work),
                                        current_stream()), 'cloud_nearest')
        copy_ms = device_ms(lambda: (d2.copy_(state[0]), idx.copy_(state[1])))
        build_ms = device_ms(build)
        query_ms = device_ms(query) - copy_ms
        evals.zero_()
        query(evals)
        ev, open_before, open_after = int(evals.sum(dtype=torch.int64)), int((state[1] < 0).sum()), int((idx < 0).sum())
        passes.append(dict(radius=float(r), cell=float(cell), key_bits=bits, build_ms=round(build_ms, 3), nearest_ms=round(query_ms, 3), queries=open_before,
                           resolved=open_before - open_after, evaluations=ev, evaluations_per_query=round(ev / max(open_before, 1), 1)))
        total_ms += build_ms + query_ms
        total_evals += ev
    print(json.dumps(dict(row='ladder', views=n, voxel_size=float(voxel), max_dist=float(max_dist), n_query=nq, n_ref=nr, n_ref_valid=n_valid,
                          workspace_MB=round(work.numel() / 2 ** 20, 1), passes=passes, total_ms=round(total_ms, 3),
                          evaluations_per_query=round(total_evals / nq, 1), evaluations_per_s=round(total_evals / total_ms * 1e3, 0),
                          found=int((idx >= 0).sum()))), flush=True)
    del state, work

    # the statistics
    stats_ms = device_ms(lambda: distance_stats(P, d2, idx, thresholds))
    print(json.dumps(dict(row='stats', n=nq, stats_and_median_ms=round(stats_ms, 3))), flush=True)

    # the whole call
    ts = []
    for rep in range(args.reps + 1):
        sync()
        t0 = time.perf_counter()
        m = cloud_metrics(pred, gt, max_dist, thresholds)
        ts.append((time.perf_counter() - t0) * 1e3)
    print(json.dumps(dict(row='cloud_metrics', points=(nq, nr), call_ms=round(statistics.median(ts[1:]), 1),
                          metrics={k: m[k] for k in ('accuracy', 'completeness', 'overall', 'precision', 'recall', 'fscore', 'outliers_pred')})), flush=True)

    # pointmap size: the exhaustive kernel against the grid
    a, b = pts[0, :H * W].contiguous(), pts[1, :H * W].contiguous()
    out = torch.empty(len(a), dtype=torch.int32, device=dev)
    ex_ms = device_ms(lambda: check(lib.d3r_nearest_neighbors(ptr(a), len(a), ptr(b), len(b), ptr(out), current_stream()), 'nearest_neighbors'), warm=1)
    far = float((torch.cat((a, b)).max(dim=0).values - torch.cat((a, b)).min(dim=0).values).norm()) * 1.01
    grid_ms = []
    for rep in range(args.reps + 1):
        sync()
        t0 = time.perf_counter()
        gi = nearest_in_cloud(a, b, far, r0=2 * voxel, to_host=False)[1]
        sync()
        grid_ms.append((time.perf_counter() - t0) * 1e3)
    ev = torch.zeros(len(a), dtype=torch.int32, device=dev)
    nearest_in_cloud(a, b, far, r0=2 * voxel, to_host=False, evals=ev)
    ev = int(ev.sum(dtype=torch.int64))
    print(json.dumps(dict(row='pointmap', n=len(a), exhaustive_ms=round(ex_ms, 2), exhaustive_evaluations_per_s=round(len(a) * len(b) / ex_ms * 1e3, 0),
                          grid_ms=round(statistics.median(grid_ms[1:]), 2), grid_evaluations_per_query=round(ev / len(a), 1),
                          grid_passes=len(ladder_radii(2 * voxel, far)), same_indices=bool(torch.equal(gi, out)))), flush=True)

    # the host
    if not args.skip_host:
        from scipy.spatial import cKDTree
        Ph, Gh = P.cpu().numpy(), G.cpu().numpy()
        for size in ([len(Ph)] if args.host_full else []) + [min(args.host_points, len(Ph))]:
            rng = np.random.default_rng(0)
            q = Ph if size == len(Ph) else Ph[np.sort(rng.choice(len(Ph), size, replace=False))]
            ref = Gh if size == len(Ph) else Gh[np.sort(rng.choice(len(Gh), min(size, len(Gh)), replace=False))]
            t0 = time.perf_counter()
            tree = cKDTree(ref)
            t1 = time.perf_counter()
            dist, nn = tree.query(q, workers=args.threads, distance_upper_bound=max_dist)
            t2 = time.perf_counter()
            row = dict(row='host', threads=args.threads, n_query=len(q), n_ref=len(ref), build_ms=round((t1 - t0) * 1e3, 1), query_ms=round((t2 - t1) * 1e3, 1))
            if size == len(Ph):
                row['found_equal'] = bool(np.array_equal(np.isfinite(dist), (idx >= 0).cpu().numpy()))
            print(json.dumps(row), flush=True)
    return None


if __name__ == '__main__':
    main()
