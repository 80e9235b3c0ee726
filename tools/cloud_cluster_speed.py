"""Times the density clustering of the fused cloud (dust3r_amd/cloud_metrics.py cluster_points, viz.FusedCloud.cluster / keep_clusters,
csrc/cloud_cluster.hip) on the workload of tools/cloud_normals_speed.py: the 100-view 512 x 384 scene of tools/glb_speed.py fused, at the
defaults of FusedCloud.cluster (eps = 2.5 voxels, min_points = 10).
- stages: device events around d3r_cloud_grid_build and after every stage of d3r_cloud_cluster (its stage_events): grid, count,
  components (union + flatten), border, numbering; the distance evaluations per point of the counting walk (the kernel's own counter; the
  union and border walks cover the same ranges), and what came out: clusters, core / border / noise points, the largest sizes;
- calls: host clock around the whole FusedCloud.cluster() and keep_clusters(largest=1) calls, device arrays;
- host: scipy.spatial.cKDTree.query_pairs(eps) + scipy.sparse.csgraph.connected_components on the core graph, on --host-points consecutive
  points of the cloud (its order is the voxel keys': a slab of the scene at full density; the full pair list, about ten pairs per point at
  16 bytes each, is read back only with --host-full). query_pairs takes no `workers`: SciPy runs it on one thread whatever --threads
  says; the neighbour COUNTS alone, query_ball_point(return_length=True, workers=threads), are timed next to it as the part that scales.

    python tools/cloud_cluster_speed.py [--views 100] [--reps 5] [--threads 16]           # the rows above, one JSON line each"""
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
    ap.add_argument('--eps-voxels', type=float, default=2.5)
    ap.add_argument('--min-points', type=int, default=10)
    ap.add_argument('--host-points', type=int, default=1000000)
    ap.add_argument('--host-full', action='store_true', help='the KD-tree at the full size too')
    ap.add_argument('--skip-host', action='store_true')
    args = ap.parse_args()
    import torch
    torch.set_num_threads(args.threads)
    from dust3r_amd import _lib
    from dust3r_amd.cloud_metrics import cluster_points
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
        cloud = fuse_points(scene.imgs, pts, mask, scene._im_conf, voxel, dev, to_host=False)
    del pts, mask
    P = cloud.positions.contiguous()
    m = len(P)
    eps, min_points = args.eps_voxels * voxel, args.min_points

    # the stages: d3r_cloud_cluster records an event after each of its four; `start` stands before the bounds pass
    per_stage = {k: [] for k in ('count', 'components', 'border', 'numbering')}
    total = []
    for rep in range(args.reps + 2):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        for e in ev:
            e.record()                                                     # creates the handles d3r_cloud_cluster records on
        sync()
        start = torch.cuda.Event(enable_timing=True)
        start.record()
        res = cluster_points(P, eps, min_points=min_points, to_host=False, stage_events=ev)
        sync()
        if rep >= 2:
            total.append(start.elapsed_time(ev[3]))
            for k, a, b in (('count', None, 0), ('components', 0, 1), ('border', 1, 2), ('numbering', 2, 3)):
                per_stage[k].append((start if a is None else ev[a]).elapsed_time(ev[b]))
    # `count` above holds bounds + grid + count; the bounds pass and the grid build alone, as cluster_points issues them
    import ctypes as C
    from dust3r_amd._lib import check, current_stream, lib, ptr
    from dust3r_amd.cloud_metrics import _bounds, grid_cell
    lo, hi, _ = _bounds(P, dev)
    cell, bits = grid_cell(lo, hi, np.float32(eps))
    lo_c, bits_c = (C.c_float * 3)(*lo.tolist()), (C.c_int * 3)(*bits)
    grid = torch.empty(int(lib.d3r_cloud_grid_workspace_bytes(m, 1)), dtype=torch.uint8, device=dev)

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
    grid_ms = device_ms(lambda: check(lib.d3r_cloud_grid_build(m, ptr(P), lo_c, float(cell), bits_c, ptr(grid), current_stream()), 'cloud_grid_build'))
    bounds_ms = device_ms(lambda: _bounds(P, dev))
    del grid
    med = {k: statistics.median(v) for k, v in per_stage.items() if v}
    head_ms = med['count']                                                 # start -> end of the count: bounds (with its read-back), grid, count
    evals = torch.zeros(m, dtype=torch.int32, device=dev)
    res = cluster_points(P, eps, min_points=min_points, to_host=False, evals=evals)
    n_eval = int(evals.sum(dtype=torch.int64))
    labelled, core = res.labels >= 0, res.core
    print(json.dumps(dict(row='stages', views=n, voxel_size=float(voxel), eps=float(eps), eps_voxels=args.eps_voxels, min_points=min_points, n=m,
                          cell=float(cell), key_bits=bits, bounds_ms=round(bounds_ms, 3), grid_ms=round(grid_ms, 3),
                          count_ms=round(head_ms - bounds_ms - grid_ms, 3), components_ms=round(med['components'], 3), border_ms=round(med['border'], 3),
                          numbering_ms=round(med['numbering'], 3), device_total_ms=round(statistics.median(total), 3),
                          workspace_MB=round((int(lib.d3r_cloud_grid_workspace_bytes(m, 1)) + int(lib.d3r_cloud_cluster_workspace_bytes(m))) / 2 ** 20, 1),
                          evaluations_per_point=round(n_eval / m, 1), mean_neighbours=round(float(res.n_neighbors.float().mean()), 2),
                          clusters=len(res.sizes), core=int(core.sum()), border=int((labelled & ~core).sum()), noise=int((~labelled).sum()),
                          largest=res.sizes[:10].tolist())), flush=True)
    del evals
    # the whole calls, host clock
    tc, tk = [], []
    for rep in range(args.reps + 1):
        sync()
        t0 = time.perf_counter()
        clustered = cloud.cluster()
        sync()
        tc.append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter()
        kept, keep = clustered.keep_clusters(largest=1)
        sync()
        tk.append((time.perf_counter() - t0) * 1e3)
    print(json.dumps(dict(row='calls', n=m, cluster_ms=round(statistics.median(tc[1:]), 1), keep_clusters_ms=round(statistics.median(tk[1:]), 1),
                          kept=len(kept))), flush=True)
    del clustered, kept, keep
    # the host
    if not args.skip_host:
        try:
            from scipy.sparse import coo_matrix
            from scipy.sparse.csgraph import connected_components
            from scipy.spatial import cKDTree
        except ImportError:
            print(json.dumps(dict(row='host', skipped='SciPy is not importable')), flush=True)
            return None
        Ph = P.cpu().numpy()
        for size in ([len(Ph)] if args.host_full else []) + [min(args.host_points, len(Ph))]:
            first = (len(Ph) - size) // 2
            q = Ph[first:first + size]                                     # consecutive in voxel-key order: a slab at full density
            t0 = time.perf_counter()
            tree = cKDTree(q)
            t1 = time.perf_counter()
            counts = tree.query_ball_point(q, float(eps), workers=args.threads, return_length=True)
            t2 = time.perf_counter()
            pairs = tree.query_pairs(float(eps), output_type='ndarray')
            t3 = time.perf_counter()
            is_core = counts >= min_points
            both = is_core[pairs[:, 0]] & is_core[pairs[:, 1]]
            n_comp, comp = connected_components(coo_matrix((np.ones(int(both.sum()), np.int8), (pairs[both, 0], pairs[both, 1])), shape=(size, size)),
                                                directed=False)
            t4 = time.perf_counter()
            print(json.dumps(dict(row='host', threads=args.threads, n=size, first=first, build_ms=round((t1 - t0) * 1e3, 1), counts_ms=round((t2 - t1) * 1e3, 1),
                                  query_pairs_ms=round((t3 - t2) * 1e3, 1), pairs=len(pairs), components_ms=round((t4 - t3) * 1e3, 1),
                                  clusters=int(len(np.unique(comp[is_core]))), core=int(is_core.sum()))), flush=True)
    return None


if __name__ == '__main__':
    main()
