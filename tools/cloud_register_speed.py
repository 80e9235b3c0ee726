"""Times the registration of one fused cloud onto another (dust3r_amd/cloud_metrics.py register_clouds, csrc/cloud_icp.hip) on the workload
of tools/cloud_normals_speed.py: the 100-view 512 x 384 scene of tools/glb_speed.py fused (the reference, with normals), and fused again
with seeded noise of half a voxel on its points, that cloud moved by the inverse of a known similarity (the source): 0.2 degrees, 0.2 % and
a shift of 5.4 voxels, which displaces the points by up to 10 voxels; the stages' gates are 16, 8 and 4 voxels.
- iteration: device events around the three parts of one iteration at the starting similarity, per stage gate: d3r_cloud_transform, the
  ladder of d3r_cloud_nearest over the kept grids, d3r_cloud_icp_sums (both metrics), and the one-off d3r_cloud_grid_build of the stage's
  rungs; the sums kernel's time against its HBM read floor (per source row 12 B point + 4 B d2 + 4 B idx, per used row 12 B
  of the reference point and, for the plane metric, 12 B of its normal, at --hbm-tbps);
- call: host clock around the whole register_clouds call, both metrics, with its iterations and the distance of its result from the truth;
- host: the same loop with scipy.spatial.cKDTree(workers=threads) as the nearest neighbour and numpy for the rest, --host-iters iterations
  at --host-points points (the full clouds with --host-full), when SciPy is importable.

    python tools/cloud_register_speed.py [--views 100] [--reps 5] [--threads 16]          # the rows above, one JSON line each"""
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
    ap.add_argument('--hbm-tbps', type=float, default=6.29, help='the achievable HBM rate the read floor is stated against')
    ap.add_argument('--host-points', type=int, default=1000000)
    ap.add_argument('--host-full', action='store_true', help='the host loop at the full size')
    ap.add_argument('--host-iters', type=int, default=3)
    ap.add_argument('--skip-host', action='store_true')
    args = ap.parse_args()
    import ctypes as C
    import torch
    torch.set_num_threads(args.threads)
    from dust3r_amd import _lib
    from dust3r_amd._lib import check, current_stream, lib, ptr
    from dust3r_amd.cloud_metrics import _bounds, _ReferenceGrids, default_r0, icp_sums, ladder_radii, register_clouds, similarity_parts
    from dust3r_amd.viz import default_voxel_size, fuse_points
    from glb_speed import make_scene
    from test_cloud_icp_cpu import restated_transform, restated_update, similarity, similarity_distance
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
        dst = fuse_points(scene.imgs, pts, mask, scene._im_conf, voxel, dev, to_host=False)
        src = fuse_points(scene.imgs, noisy, mask, scene._im_conf, voxel, dev, to_host=False)
    del noisy, pts, mask
    t0 = time.perf_counter()
    dst = dst.estimate_normals(k=16)
    sync()
    normals_ms = (time.perf_counter() - t0) * 1e3
    lo, hi, _ = _bounds(dst.positions, dev)
    centre = (0.5 * (lo.astype(np.float64) + hi.astype(np.float64)))
    # 0.2 degrees and 0.2 % about the middle and a shift of (4, -3, 2) voxels: at the rim of the scene (2 units from the middle, 1200 voxels)
    # the turn moves a point by 4 voxels and the scale by 2.4, inside the first gate of 16 voxels, as a coarse alignment has to be
    truth = similarity((1, 2, 3), 0.2, 1.002, (0, 0, 0))
    truth[:3, 3] = centre - truth[:3, :3] @ centre + np.array([4.0, -3.0, 2.0]) * voxel
    src = src.transform(np.linalg.inv(truth))
    stages = [16 * voxel, 8 * voxel, 4 * voxel]
    P, Q, QN = src.positions.contiguous(), dst.positions.contiguous(), dst.normals.contiguous()
    m, mr = len(P), len(Q)

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

    # one iteration, part by part, at the starting similarity
    S0 = np.eye(4)
    M = similarity_parts(S0)[0]
    M_c = (C.c_float * 12)(*M.tolist())
    moved = torch.empty_like(P)
    d2 = torch.empty((m,), dtype=torch.float32, device=dev)
    idx = torch.empty((m,), dtype=torch.int32, device=dev)
    transform_ms = device_ms(lambda: check(lib.d3r_cloud_transform(m, ptr(P), M_c, ptr(moved), None, None, None, current_stream()), 'cloud_transform'))
    for gate in stages:
        radii = ladder_radii(min(default_r0(dst, gate), float(gate)), gate)
        build_ms = device_ms(lambda: _ReferenceGrids(Q, lo, hi, radii, m), reps=3, warm=1)
        grids = _ReferenceGrids(Q, lo, hi, radii, m)
        nearest_ms = device_ms(lambda: grids.search(moved, d2, idx))
        row = dict(row='iteration', views=n, voxel_size=float(voxel), n_src=m, n_ref=mr, gate_voxels=round(float(gate) / voxel, 2), rungs=[float(r) for r in radii],
                   grid_build_once_ms=round(build_ms, 3), transform_ms=round(transform_ms, 3), nearest_ms=round(nearest_ms, 3))
        for metric in ('point', 'plane'):
            kw = dict(ref_normals=QN if metric == 'plane' else None)
            sums_ms = device_ms(lambda: icp_sums(moved, Q, d2, idx, metric, gate, centre, **kw))
            used = int(icp_sums(moved, Q, d2, idx, metric, gate, centre, **kw)[0])
            read = m * (12 + 4 + 4) + used * (24 if metric == 'plane' else 12)
            floor_ms = read / (args.hbm_tbps * 1e12) * 1e3
            row.update({f'sums_{metric}_ms': round(sums_ms, 3), f'pairs_{metric}': used, f'sums_{metric}_read_MB': round(read / 1e6, 1),
                        f'sums_{metric}_floor_ms': round(floor_ms, 4), f'sums_{metric}_fraction_of_floor_rate': round(floor_ms / sums_ms, 3)})
        row['iteration_plane_ms'] = round(transform_ms + nearest_ms + row['sums_plane_ms'], 3)
        row['nearest_share_plane'] = round(nearest_ms / row['iteration_plane_ms'], 3)
        print(json.dumps(row), flush=True)
        del grids
    # the whole calls, host clock
    for metric in ('plane', 'point'):
        ts = []
        for rep in range(min(args.reps, 3)):
            sync()
            t0 = time.perf_counter()
            reg = register_clouds(src, dst, stages, metric=metric)
            sync()
            ts.append((time.perf_counter() - t0) * 1e3)
        ang, ds, dt = similarity_distance(reg.similarity, truth)
        print(json.dumps(dict(row='call', metric=metric, n_src=m, n_ref=mr, stages_voxels=[round(float(s) / voxel, 2) for s in stages], call_ms=round(statistics.median(ts), 1),
                              iterations=reg.iterations, ms_per_iteration=round(statistics.median(ts) / reg.iterations, 2), converged=reg.converged, reason=reg.reason,
                              pairs=reg.n_pairs, rmse_voxels=round(reg.rmse / voxel, 4), from_truth_deg=ang, from_truth_scale=ds, from_truth_translation_voxels=dt / voxel,
                              reference_normals_ms=round(normals_ms, 1))), flush=True)
    if args.skip_host:
        return None
    try:
        from scipy.spatial import cKDTree
    except ImportError:
        print(json.dumps(dict(row='host', skipped='SciPy is not importable')), flush=True)
        return None
    Ph, Qh, Nh = P.cpu().numpy(), Q.cpu().numpy(), QN.cpu().numpy()
    rng = np.random.default_rng(0)
    if not args.host_full:
        Ph = Ph[np.sort(rng.choice(len(Ph), min(args.host_points, len(Ph)), replace=False))]
        keep = np.sort(rng.choice(len(Qh), min(args.host_points, len(Qh)), replace=False))
        Qh, Nh = Qh[keep], Nh[keep]
    t0 = time.perf_counter()
    tree = cKDTree(Qh)
    tree_ms = (time.perf_counter() - t0) * 1e3
    S, gate, c64, parts = np.eye(4), float(stages[0]), centre, dict(transform=[], nearest=[], sums_update=[])
    for it in range(args.host_iters):
        t0 = time.perf_counter()
        mv = restated_transform(Ph, S[:3, :4].astype(np.float32).reshape(12))
        t1 = time.perf_counter()
        dist, j = tree.query(mv, k=1, workers=args.threads, distance_upper_bound=gate)
        t2 = time.perf_counter()
        ok = np.isfinite(dist) & (np.abs(Nh[np.minimum(j, len(Qh) - 1)]).sum(axis=1) > 0)
        a, y, nn = mv[ok].astype(np.float64) - c64, Qh[j[ok]].astype(np.float64) - c64, Nh[j[ok]].astype(np.float64)
        A, v = restated_update('plane', a, y, nn, True)
        D = np.eye(4)
        D[:3, :3], D[:3, 3] = A, c64 + v - A @ c64
        S = D @ S
        t3 = time.perf_counter()
        for key, dt_ in zip(('transform', 'nearest', 'sums_update'), (t1 - t0, t2 - t1, t3 - t2)):
            parts[key].append(dt_ * 1e3)
    print(json.dumps(dict(row='host', threads=args.threads, n_src=len(Ph), n_ref=len(Qh), gate_voxels=round(gate / voxel, 2), tree_build_once_ms=round(tree_ms, 1),
                          iterations=args.host_iters, **{f'{k}_ms': round(statistics.median(v), 1) for k, v in parts.items()},
                          iteration_ms=round(sum(statistics.median(v) for v in parts.values()), 1))), flush=True)
    return None


if __name__ == '__main__':
    main()
