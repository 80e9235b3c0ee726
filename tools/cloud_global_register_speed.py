"""Times the global registration of one fused cloud onto another (dust3r_amd/cloud_metrics.py global_registration, csrc/cloud_features.hip)
on the workload of tools/cloud_register_speed.py: the 100-view 512 x 384 scene of tools/glb_speed.py fused with camera-oriented normals (the
destination), and fused again with seeded noise of half a voxel on its points, that cloud moved by the inverse of a similarity of 140
degrees and scale 2.7 (the source). The feature cell is a fraction of each cloud's size chosen so that about --features points remain.
- stage: device events, the median of --reps, around the grid build and d3r_cloud_grid_heads, the k nearest neighbours, d3r_cloud_spfh,
  d3r_cloud_fpfh, the two passes of d3r_feature_nearest, d3r_sim3_ransac at --hypotheses;
- matching: the distance evaluations per second of d3r_feature_nearest and the fraction of the fp32 vector rate (--vector-tflops, which
  counts an FMA as two operations; the file is built without contraction) that its 99 operations per pair amount to;
- call: host clock around the whole global_registration call, and the distance of its result, and of the ICP that follows, from the truth;
- host: the same pipeline on --threads host threads: scipy.spatial.cKDTree in 33 dimensions for the two matching passes, the numpy RANSAC
  of tests/test_cloud_global_cpu.py (at --host-hypotheses, scaled), when SciPy is importable.

    python tools/cloud_global_register_speed.py [--views 100] [--reps 5] [--threads 16]          # the rows above, one JSON line each"""
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
    ap.add_argument('--features', type=int, default=50000)
    ap.add_argument('--hypotheses', type=int, default=1 << 20)
    ap.add_argument('--host-hypotheses', type=int, default=1 << 16)
    ap.add_argument('--vector-tflops', type=float, default=157.3)
    ap.add_argument('--skip-host', action='store_true')
    args = ap.parse_args()
    import torch
    torch.set_num_threads(args.threads)
    from dust3r_amd import _lib
    from dust3r_amd._lib import check, current_stream, lib, ptr
    from dust3r_amd.cloud_metrics import (_bounds, _ReferenceGrids, FEATURE_KNN_RADIUS, cloud_size, feature_cloud, feature_nearest, fpfh_features,
                                          global_registration, k_nearest, match_features, register_clouds, sim3_ransac, spfh_counts)
    from dust3r_amd.viz import default_voxel_size, fuse_points
    from glb_speed import make_scene
    from test_cloud_icp_cpu import similarity, similarity_distance
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
        dst = fuse_points(scene.imgs, pts, mask, scene._im_conf, voxel, dev, to_host=False).estimate_normals(k=16, scene=scene)
        src = fuse_points(scene.imgs, noisy, mask, scene._im_conf, voxel, dev, to_host=False).estimate_normals(k=16, scene=scene)
    del noisy, pts, mask
    truth = similarity((-2, 1, 0.5), 140.0, 2.7, (3, -5, 1.5))
    src = src.transform(np.linalg.inv(truth))

    def device_ms(fn, reps=args.reps, warm=1):
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

    # the fraction of a cloud's size that leaves about --features points: a surface holds about 1 / cell^2 cells
    size_d, size_s = cloud_size(dst.positions)[0], cloud_size(src.positions)[0]
    frac = 0.02
    for _ in range(4):
        count = len(feature_cloud(dst, cell=frac * size_d)[0])
        frac *= (count / args.features) ** 0.5
    cells = (frac * size_s, frac * size_d)
    rows, feats = {}, []
    for name, cloud, cell in (('src', src, cells[0]), ('dst', dst, cells[1])):
        P = cloud.positions.contiguous()
        lo, hi, _ = _bounds(P, dev)
        heads = torch.empty((len(P),), dtype=torch.int32, device=dev)
        count = torch.zeros((1,), dtype=torch.int32, device=dev)
        build_ms = device_ms(lambda: _ReferenceGrids(P, lo, hi, [cell], 1), reps=3)
        grids = _ReferenceGrids(P, lo, hi, [cell], 1)
        heads_ms = device_ms(lambda: check(lib.d3r_cloud_grid_heads(len(P), ptr(heads), ptr(count), ptr(grids.rungs[0][3]), current_stream()), 'heads'))
        F, N, cell, _ = feature_cloud(cloud, cell=cell)
        radius = FEATURE_KNN_RADIUS * cell
        knn = lambda: k_nearest(F, F, 32, radius, exclude_self=True, r0=min(cell * 32 ** 0.5, radius), to_host=False)      # noqa: E731
        knn_ms = device_ms(knn)
        d2, idx = knn()
        spfh_ms = device_ms(lambda: spfh_counts(F, N, idx))
        counts = spfh_counts(F, N, idx)
        fpfh_ms = device_ms(lambda: fpfh_features(d2, idx, counts))
        feats.append((F, fpfh_features(d2, idx, counts)))
        rows[name] = dict(points=len(P), features=len(F), cell=float(cell), cell_over_voxel=round(float(cell) / cloud.voxel_size, 2), full_rows=int((idx[:, -1] >= 0).sum()),
                          grid_build_ms=round(build_ms, 3), heads_ms=round(heads_ms, 4), knn_ms=round(knn_ms, 3), spfh_ms=round(spfh_ms, 4),
                          fpfh_ms=round(fpfh_ms, 4))
        del grids
    (Ps, Fs), (Pd, Fd) = feats
    fwd_ms, bwd_ms = device_ms(lambda: feature_nearest(Fs, Fd)), device_ms(lambda: feature_nearest(Fd, Fs))
    pairs = len(Fs) * len(Fd)
    rate = 2 * pairs / ((fwd_ms + bwd_ms) * 1e-3)
    ia, ib = match_features(Fs, Fd)
    p, q, thr = Ps[ia].contiguous(), Pd[ib].contiguous(), 0.5 * cells[1]
    ransac_ms = device_ms(lambda: sim3_ransac(p, q, args.hypotheses, thr))
    best = sim3_ransac(p, q, args.hypotheses, thr)[0].cpu().numpy()
    print(json.dumps(dict(row='stage', views=n, voxel_size=float(voxel), cell_fraction_of_size=frac, src=rows['src'], dst=rows['dst'],
                          match_forward_ms=round(fwd_ms, 3), match_backward_ms=round(bwd_ms, 3), matches=len(ia), hypotheses=args.hypotheses,
                          ransac_ms=round(ransac_ms, 3), ransac_valid=int(best[2]), ransac_best=int(best[1]))), flush=True)
    print(json.dumps(dict(row='matching', pairs_per_pass=pairs, evaluations_per_s=rate, fp32_ops_per_pair=99, tflops=round(rate * 99 / 1e12, 2),
                          nominal_vector_tflops=args.vector_tflops, fraction_of_nominal=round(rate * 99 / 1e12 / args.vector_tflops, 4),
                          fraction_of_the_rate_without_fma=round(rate * 99 / 1e12 / (args.vector_tflops / 2), 4))), flush=True)
    ts = []
    for _ in range(min(args.reps, 5)):
        sync()
        t0 = time.perf_counter()
        res = global_registration(src, dst, cell=cells, n_hyp=args.hypotheses)
        sync()
        ts.append((time.perf_counter() - t0) * 1e3)
    call = dict(row='call', call_ms=round(statistics.median(ts), 1), n_features=res.n_features, n_matches=res.n_matches, n_inliers=res.n_inliers,
                n_valid=res.n_valid, mirrored=res.mirrored, reason=res.reason)
    if res.similarity is not None:
        ang, ds, dt = similarity_distance(res.similarity, truth)
        call.update(from_truth_deg=ang, from_truth_scale=ds, from_truth_translation_voxels=dt / voxel)
        stages = [4 * thr, 2 * thr, thr]
        reg = register_clouds(src, dst, stages, init=res.similarity)
        ang, ds, dt = similarity_distance(reg.similarity, truth)
        call.update(icp_stages_voxels=[round(s / voxel, 1) for s in stages], icp_iterations=reg.iterations, icp_converged=reg.converged,
                    after_icp_deg=ang, after_icp_scale=ds, after_icp_translation_voxels=dt / voxel)
    print(json.dumps(call), flush=True)
    if args.skip_host:
        return None
    try:
        from scipy.spatial import cKDTree
    except ImportError:
        print(json.dumps(dict(row='host', skipped='SciPy is not importable')), flush=True)
        return None
    from test_cloud_global_cpu import restated_ransac
    fs, fd = Fs.cpu().numpy(), Fd.cpu().numpy()
    t0 = time.perf_counter()
    tree_d, tree_s = cKDTree(fd), cKDTree(fs)
    t1 = time.perf_counter()
    ab = tree_d.query(fs, k=1, workers=args.threads)[1]
    t2 = time.perf_counter()
    ba = tree_s.query(fd, k=1, workers=args.threads)[1]
    t3 = time.perf_counter()
    ja = np.flatnonzero(ba[ab] == np.arange(len(fs)))
    host = dict(row='host', threads=args.threads, tree_build_ms=round((t1 - t0) * 1e3, 1), match_forward_ms=round((t2 - t1) * 1e3, 1),
                match_backward_ms=round((t3 - t2) * 1e3, 1), matches=len(ja), matches_shared_with_the_device=int(np.isin(ja, ia.cpu().numpy()).sum()))
    host['matching_ratio'] = round((t3 - t1) * 1e3 / (fwd_ms + bwd_ms), 1)
    print(json.dumps(host), flush=True)
    t0 = time.perf_counter()
    want = restated_ransac(p.cpu().numpy(), q.cpu().numpy(), 0, args.host_hypotheses, thr)
    ms = (time.perf_counter() - t0) * 1e3
    per_hyp = ms / args.host_hypotheses
    print(json.dumps(dict(row='host_ransac', hypotheses=args.host_hypotheses, ms=round(ms, 1), valid=want['n_valid'], best=want['count'],
                          ms_scaled_to_device_hypotheses=round(per_hyp * args.hypotheses, 1),
                          ransac_ratio=round(per_hyp * args.hypotheses / ransac_ms, 1))), flush=True)
    return None


if __name__ == '__main__':
    main()
