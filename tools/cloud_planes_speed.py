"""Times the plane detection of the fused cloud (dust3r_amd/cloud_metrics.py plane_ransac / segment_plane / detect_planes,
viz.FusedCloud.detect_planes, csrc/cloud_planes.hip) on the workload of tools/cloud_cluster_speed.py: the 100-view 512 x 384 scene of
tools/glb_speed.py fused, at the defaults of FusedCloud.detect_planes (thr = 2 voxels, min_area2 = (8 thr)^2, 4096 hypotheses).
- score: device events around d3r_plane_ransac (hypotheses, scoring, selection, mask: the scoring kernel is all but a few microseconds
  of it) without and with normals; plane tests per second, and the fraction of the fp32 vector rate they amount to at 6 operations a
  test (3 products, 3 sums; 11 with normals) against --peak-tflops (157.3: 256 CUs x 128 lanes x 2 x 2.4 GHz, the data sheet's vector fp32);
- support: device events around d3r_plane_support (one refit round without its read-back);
- calls: host clock around segment_plane (RANSAC + 3 refits) and FusedCloud.detect_planes(max_planes=6), device arrays, and what came out;
- host: the same RANSAC restated in numpy (per hypothesis one vectorised pass over the points: the distance, the comparison, the count; what
  Open3D's segment_plane does per iteration), the hypotheses spread over --threads threads, on --host-points points and --host-hyp
  hypotheses; the time for 4096 hypotheses is that scaled.
Every row is one JSON line, on stdout and in profiles/cloud_planes/cloud_planes_speed.log.

    python tools/cloud_planes_speed.py [--views 100] [--reps 5] [--threads 16]"""
import argparse
import json
import os
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests'), os.path.join(ROOT, 'tools')]

import numpy as np  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--views', type=int, default=100)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--threads', type=int, default=16)
    ap.add_argument('--n-hyp', type=int, default=4096)
    ap.add_argument('--thr-voxels', type=float, default=2.0)
    ap.add_argument('--peak-tflops', type=float, default=157.3)
    ap.add_argument('--min-inliers', type=int, default=1000,
                    help='of detect_planes: low, so that the bumpy synthetic scene, which has no plane of 2 %% of its points, gives six rounds')
    ap.add_argument('--host-points', type=int, default=1000000)
    ap.add_argument('--host-hyp', type=int, default=256)
    ap.add_argument('--skip-host', action='store_true')
    ap.add_argument('--log', default=os.path.join(ROOT, 'profiles', 'cloud_planes', 'cloud_planes_speed.log'))
    args = ap.parse_args()
    import torch
    torch.set_num_threads(args.threads)
    from dust3r_amd import _lib
    from dust3r_amd.cloud_metrics import plane_ransac, plane_support, segment_plane
    from dust3r_amd.viz import default_voxel_size, fuse_points
    from glb_speed import make_scene
    _lib.require_device()
    dev = torch.device('cuda:0')
    n, H, W = args.views, 384, 512
    sync = torch.cuda.synchronize
    os.makedirs(os.path.dirname(args.log), exist_ok=True)
    log = open(args.log, 'w')
    log.write(f'# python tools/cloud_planes_speed.py --views {n} --reps {args.reps} --threads {args.threads}   (one MI355X, one visit; {n} views of '
              f'{W} x {H} fused; thr = {args.thr_voxels} voxels, {args.n_hyp} hypotheses; medians of {args.reps})\n')

    def emit(**row):
        line = json.dumps(row)
        print(line, flush=True)
        log.write(line + '\n')
        log.flush()

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
    thr = args.thr_voxels * voxel
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    N = torch.nn.functional.normalize(torch.randn(m, 3, device=dev, generator=g), dim=1).contiguous()      # the kernel's cost does not depend on their values

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

    for normals, ops in ((None, 6), (N, 11)):
        ms = device_ms(lambda: plane_ransac(P, thr, args.n_hyp, normals, None if normals is None else 0.9))
        best = plane_ransac(P, thr, args.n_hyp, normals, None if normals is None else 0.9)[0].cpu().numpy()
        tests = m * best[2]                                                # invalid hypotheses are not scored
        emit(row='score', normals=normals is not None, n=m, n_hyp=args.n_hyp, valid=int(best[2]), thr=float(thr), ransac_ms=round(ms, 3),
             plane_tests_per_s=round(tests / (ms * 1e-3), 0), fp32_ops_per_test=ops, tflops=round(tests * ops / (ms * 1e-3) / 1e12, 2),
             fraction_of_vector_fp32=round(tests * ops / (ms * 1e-3) / 1e12 / args.peak_tflops, 3), best_count=int(best[1]))
    model = best[3:7]
    centre = (-model[3] * model[:3]).astype(np.float32)
    emit(row='support', n=m, support_ms=round(device_ms(lambda: plane_support(P, model, thr, centre)), 3),
         support_with_normals_ms=round(device_ms(lambda: plane_support(P, model, thr, centre, N, 0.9)), 3))
    ts, td = [], []
    for rep in range(args.reps + 1):
        sync()
        t0 = time.perf_counter()
        plane = segment_plane(P, thr, n_hyp=args.n_hyp, to_host=False)
        sync()
        ts.append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter()
        found = cloud.detect_planes(max_planes=6, n_hyp=args.n_hyp, min_inliers=args.min_inliers)
        sync()
        td.append((time.perf_counter() - t0) * 1e3)
    emit(row='calls', n=m, segment_plane_ms=round(statistics.median(ts[1:]), 1), segment_count=plane.count, segment_rms_voxels=round(plane.rms / voxel, 3),
         detect_planes_ms=round(statistics.median(td[1:]), 1), min_inliers=args.min_inliers, planes=len(found.planes),
         sizes=[int(s) for s in found.plane_sizes.cpu().tolist()])
    if not args.skip_host:
        from test_cloud_global_cpu import restated_samples
        Ph = P.cpu().numpy()
        size = min(args.host_points, len(Ph))
        first = (len(Ph) - size) // 2
        q = np.ascontiguousarray(Ph[first:first + size])                   # consecutive in voxel-key order: a slab at full density
        x, y, z = (np.ascontiguousarray(q[:, c]) for c in range(3))
        pick = restated_samples(0, args.host_hyp, size)
        t = np.float32(thr)

        def score(h):
            p0, p1, p2 = (q[pick[h, c]].astype(np.float64) for c in range(3))
            c = np.cross(p1 - p0, p2 - p0)
            ln = np.linalg.norm(c)
            if not ln >= (8.0 * float(t)) ** 2:
                return -1
            nrm = (c / ln).astype(np.float32)
            d = np.float32(-(c / ln) @ p0)
            return int(np.count_nonzero(np.abs(nrm[0] * x + nrm[1] * y + nrm[2] * z + d) <= t))
        t0 = time.perf_counter()
        with ThreadPoolExecutor(args.threads) as ex:
            counts = list(ex.map(score, range(args.host_hyp)))
        dt = time.perf_counter() - t0
        scored = sum(c >= 0 for c in counts)
        emit(row='host', threads=args.threads, n=size, first=first, n_hyp=args.host_hyp, scored=scored, ms=round(dt * 1e3, 1),
             plane_tests_per_s=round(size * scored / dt, 0), ms_for_4096_hypotheses=round(dt * 1e3 * 4096 / max(scored, 1), 0), best_count=max(counts))
    log.close()
    return None


if __name__ == '__main__':
    main()
