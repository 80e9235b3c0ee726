"""Times the k nearest neighbours, the normals and the outlier removal of the fused cloud (dust3r_amd/cloud_metrics.py k_nearest,
viz.FusedCloud.estimate_normals / remove_outliers, csrc/cloud_knn.hip) on the workload of tools/cloud_metrics_speed.py: the 100-view
512 x 384 scene of tools/glb_speed.py fused, and fused again with seeded noise of half a voxel on its points.
- knn: per cloud and per ladder (the chosen one -- r_0 = default_knn_r0 = 4 voxels at k = 16, KNN_LADDER_STEP = 2, cells of KNN_CELL_FACTOR r
  -- and its alternatives: r_0 = 2 voxels, a step of 4, cells of r / 2), device events around d3r_cloud_grid_build and d3r_cloud_knn of every
  rung at k = 16, exclude_self, max_dist = 8 voxels: the queries each rung takes and resolves, the distance evaluations per query (the
  kernel's own counter);
- single: the single-neighbour ladder (d3r_cloud_nearest) of the cloud in itself, the floor the grid walk sets;
- consumers: d3r_cloud_knn_distances, d3r_cloud_normals and d3r_cloud_orient_normals alone, device events;
- calls: host clock around the whole estimate_normals(scene=scene) and remove_outliers calls;
- host: scipy.spatial.cKDTree(...).query(k=17, workers=threads, distance_upper_bound=max_dist) on the same cloud when SciPy is importable,
  at the full size when --host-full, else at --host-points points.

    python tools/cloud_normals_speed.py [--views 100] [--reps 5] [--threads 16]           # the rows above, one JSON line each"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests'), os.path.join(ROOT, 'tools')]

import numpy as np  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--views', type=int, default=100)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--threads', type=int, default=16)
    ap.add_argument('--k', type=int, default=16)
    ap.add_argument('--host-points', type=int, default=1000000)
    ap.add_argument('--host-full', action='store_true', help='the KD-tree at the full size too')
    ap.add_argument('--skip-host', action='store_true')
    ap.add_argument('--clouds', default='fused,noisy')
    args = ap.parse_args()
    import ctypes as C
    import torch
    torch.set_num_threads(args.threads)
    from dust3r_amd import _lib
    from dust3r_amd._lib import check, current_stream, lib, ptr
    from dust3r_amd.cloud_metrics import (KNN_CELL_FACTOR, KNN_LADDER_STEP, _bounds, default_knn_r0, cloud_normals, grid_cell, k_nearest, knn_mean_distances, ladder_radii,
                                          nearest_in_cloud, orient_normals)
    from dust3r_amd.viz import default_voxel_size, fuse_points
    from glb_speed import make_scene
    _lib.require_device()
    dev = torch.device('cuda:0')
    n, H, W, k = args.views, 384, 512, args.k
    sync = torch.cuda.synchronize
    scene = make_scene(n, H, W, dev)
    with torch.no_grad():
        pts = scene.get_pts3d(raw=True).contiguous()
        scene.min_conf_thr = float(scene.conf_trf(torch.tensor(3.0)))
        mask = scene.get_masks(raw=True).to(torch.uint8)
        voxel = default_voxel_size(scene.get_depthmaps(raw=True), [H * W] * n, scene.get_focals())
        g = torch.Generator(device=dev).manual_seed(7)
        noisy = pts + 0.5 * voxel * torch.randn(pts.shape, device=dev, generator=g)
        clouds = dict(fused=fuse_points(scene.imgs, pts, mask, scene._im_conf, voxel, dev, to_host=False),
                      noisy=fuse_points(scene.imgs, noisy, mask, scene._im_conf, voxel, dev, to_host=False))
    del noisy, pts, mask
    max_dist = 8 * voxel
    r0 = default_knn_r0(clouds['fused'], k, max_dist)
    clouds = {name: clouds[name] for name in args.clouds.split(',')}

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

    for name, cloud in clouds.items():
        P = cloud.positions.contiguous()
        m = len(P)
        lo, hi, n_valid = _bounds(P, dev)
        work = torch.empty(int(lib.d3r_cloud_grid_workspace_bytes(m, m)), dtype=torch.uint8, device=dev)
        lo_c = (C.c_float * 3)(*lo.tolist())
        d2 = torch.empty((m, k), dtype=torch.float32, device=dev)
        idx = torch.empty((m, k), dtype=torch.int32, device=dev)
        evals = torch.zeros(m, dtype=torch.int32, device=dev)
        # the k-neighbour ladder, rung by rung (what k_nearest does, with events around the two calls)
        chosen = (r0, KNN_LADDER_STEP, KNN_CELL_FACTOR)
        for first, step, factor in (chosen, (r0, KNN_LADDER_STEP, 0.5), (2 * voxel, KNN_LADDER_STEP, KNN_CELL_FACTOR), (2 * voxel, 4.0, KNN_CELL_FACTOR)):
            rungs, total_ms, total_evals = [], 0.0, 0
            for j, r in enumerate(ladder_radii(first, max_dist, step=step)):
                cell, bits = grid_cell(lo, hi, np.float32(float(r) * factor))
                bits_c = (C.c_int * 3)(*bits)
                if j == 0:
                    d2.fill_(float('inf'))
                    idx.fill_(-1)
                last = idx[:, k - 1].clone()                           # a rung only reads the last column of what the rung before left

                def build():
                    check(lib.d3r_cloud_grid_build(m, ptr(P), lo_c, float(cell), bits_c, ptr(work), current_stream()), 'cloud_grid_build')

                def query(count=None):
                    idx[:, k - 1] = last
                    check(lib.d3r_cloud_knn(m, m, ptr(P), k, float(r), lo_c, float(cell), bits_c, 1, int(j > 0), ptr(d2), ptr(idx), ptr(count), ptr(work),
                                            current_stream()), 'cloud_knn')
                copy_ms = device_ms(lambda: idx[:, k - 1].copy_(last))
                build_ms = device_ms(build)
                query_ms = device_ms(query) - copy_ms
                evals.zero_()
                query(evals)
                ev, open_before, open_after = int(evals.sum(dtype=torch.int64)), int((last < 0).sum()), int((idx[:, k - 1] < 0).sum())
                rungs.append(dict(radius=float(r), cell=float(cell), key_bits=bits, build_ms=round(build_ms, 3), knn_ms=round(query_ms, 3), queries=open_before,
                                  resolved=open_before - open_after, evaluations=ev, evaluations_per_query=round(ev / max(open_before, 1), 1)))
                total_ms += build_ms + query_ms
                total_evals += ev
            print(json.dumps(dict(row='knn', cloud=name, k=k, r0_voxels=round(first / voxel, 2), step=step, cell_factor=factor, chosen=(first, step, factor) == chosen, views=n, voxel_size=float(voxel),
                                  max_dist=float(max_dist), n=m, workspace_MB=round(work.numel() / 2 ** 20, 1), rungs=rungs, total_ms=round(total_ms, 3),
                                  evaluations_per_query=round(total_evals / m, 1), evaluations_per_s=round(total_evals / total_ms * 1e3, 0),
                                  full_rows=int((idx[:, k - 1] >= 0).sum()))), flush=True)
        del work
        # the single-neighbour ladder of the same cloud in itself: the floor the grid walk sets
        ev1 = torch.zeros(m, dtype=torch.int32, device=dev)
        nearest_in_cloud(P, P, max_dist, r0=2 * voxel, to_host=False, evals=ev1)
        single_ms = device_ms(lambda: nearest_in_cloud(P, P, max_dist, r0=2 * voxel, to_host=False))
        knn_call_ms = device_ms(lambda: k_nearest(P, P, k, max_dist, exclude_self=True, r0=r0, to_host=False))
        print(json.dumps(dict(row='single', cloud=name, n=m, nearest_in_cloud_ms=round(single_ms, 3), evaluations_per_query=round(int(ev1.sum(dtype=torch.int64)) / m, 1),
                              k_nearest_ms=round(knn_call_ms, 3), ratio=round(knn_call_ms / single_ms, 2))), flush=True)
        # the consumers alone
        d2, idx = k_nearest(P, P, k, max_dist, exclude_self=True, r0=r0, to_host=False)
        mean_ms = device_ms(lambda: knn_mean_distances(d2, idx))
        normals_ms = device_ms(lambda: cloud_normals(P, P, idx))
        normals, _ = cloud_normals(P, P, idx)
        heights, widths, _ = scene._shape_tables
        with torch.no_grad():
            stacks = (scene.get_depthmaps(raw=True), scene._im_conf, scene.get_intrinsics(), scene.get_im_poses())
            orient_ms = device_ms(lambda: orient_normals(P, normals, *stacks, heights, widths, tol=0.05))
            seen = orient_normals(P, normals, *stacks, heights, widths, tol=0.05)
        print(json.dumps(dict(row='consumers', cloud=name, n=m, views=n, mean_distances_ms=round(mean_ms, 3), normals_ms=round(normals_ms, 3),
                              orient_ms=round(orient_ms, 3), seen_by_a_view=int((seen > 0).sum()), mean_views_seeing=round(float(seen.float().mean()), 2))), flush=True)
        del d2, idx, normals, seen
        # the whole calls, host clock
        ts, to = [], []
        for rep in range(args.reps + 1):
            sync()
            t0 = time.perf_counter()
            with_normals = cloud.estimate_normals(k=k, scene=scene)
            sync()
            ts.append((time.perf_counter() - t0) * 1e3)
            t0 = time.perf_counter()
            kept, keep = cloud.remove_outliers(k=k, std_ratio=2.0)
            sync()
            to.append((time.perf_counter() - t0) * 1e3)
        zero = int((with_normals.normals == 0).all(dim=1).sum())
        print(json.dumps(dict(row='calls', cloud=name, n=m, estimate_normals_ms=round(statistics.median(ts[1:]), 1), zero_normals=zero,
                              remove_outliers_ms=round(statistics.median(to[1:]), 1), kept=len(kept))), flush=True)
        del with_normals, kept, keep
        # the host
        if not args.skip_host:
            try:
                from scipy.spatial import cKDTree
            except ImportError:
                print(json.dumps(dict(row='host', skipped='SciPy is not importable')), flush=True)
                continue
            Ph = P.cpu().numpy()
            for size in ([len(Ph)] if args.host_full else []) + [min(args.host_points, len(Ph))]:
                rng = np.random.default_rng(0)
                q = Ph if size == len(Ph) else Ph[np.sort(rng.choice(len(Ph), size, replace=False))]
                t0 = time.perf_counter()
                tree = cKDTree(q)
                t1 = time.perf_counter()
                tree.query(q, k=k + 1, workers=args.threads, distance_upper_bound=max_dist)
                t2 = time.perf_counter()
                print(json.dumps(dict(row='host', cloud=name, threads=args.threads, n=len(q), k=k + 1, build_ms=round((t1 - t0) * 1e3, 1),
                                      query_ms=round((t2 - t1) * 1e3, 1))), flush=True)
    return None


if __name__ == '__main__':
    main()
