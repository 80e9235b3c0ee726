"""Times visual localization on the GPU against host restatements, and checks that both agree:
  * d3r_match_pairs for 20 pairs of 512 x 384 (device events around the match_pairs call: record upload, kernels, count readback), against this package's find_reciprocal_matches one
    pair at a time (masking included, GPU) and SciPy cKDTree queries on a pool of host threads;
  * d3r_pnp_ransac for 100 jobs x 100 000 correspondences at 30 % outliers, against a numpy restatement of the same RANSAC (P3P from
    the library's host build, vectorised scoring, same stopping rule) on a pool of host threads;
  * localize for 20 queries x 10 map views on the synthetic-weight engine (wall clock), against the per-query loop restated from
    visloc.py (one inference per pair, host masks, find_reciprocal_matches, run_pnp per query).

    python tools/visloc_speed.py [--threads 16] [--reps 5]"""
import argparse
import ctypes as C
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
from dust3r_amd.visloc import localization as L  # noqa: E402


def _sync_ms(fn, reps):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps, out


def bench_match(dev, threads, reps):
    from scipy.spatial import cKDTree
    from dust3r_amd.utils.geometry import find_reciprocal_matches
    H, W, n = 384, 512, 20
    g = torch.Generator(device='cpu').manual_seed(0)
    pairs = []
    for _ in range(n):
        pq = torch.randn((H, W, 3), generator=g)
        pm = pq + 0.05 * torch.randn((H, W, 3), generator=g)
        pairs.append(tuple(t.to(dev) for t in (pq, 1 + torch.exp(torch.randn((H, W), generator=g)), pm,
                                               1 + torch.exp(torch.randn((H, W), generator=g)))) + ((torch.rand((H, W), generator=g) < 0.9).to(dev),))
    thr = 1.5
    gpu_ms, got = _sync_ms(lambda: L.match_pairs(pairs, thr, dev), reps)

    def one(p):
        pq, cq, pm, cm, vm = p
        mq, mm = (cq >= thr).reshape(-1), ((cm >= thr) & vm).reshape(-1)
        recip, nn2, _ = find_reciprocal_matches(pq.reshape(-1, 3)[mq], pm.reshape(-1, 3)[mm])
        return torch.nonzero(mq)[:, 0][nn2][recip], torch.nonzero(mm)[:, 0][recip]
    per_pair_ms, ref = _sync_ms(lambda: [one(p) for p in pairs], 1)
    same = all(torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) for a, b in zip(got, ref))
    host = [tuple(t.cpu().numpy() for t in p) for p in pairs]

    def kd(p):
        pq, cq, pm, cm, vm = p
        PQ, PM = pq.reshape(-1, 3)[(cq >= thr).ravel()], pm.reshape(-1, 3)[((cm >= thr) & vm).ravel()]
        nn1 = cKDTree(PM).query(PQ, workers=1)[1]
        nn2 = cKDTree(PQ).query(PM, workers=1)[1]
        return int((nn1[nn2] == np.arange(len(nn2))).sum())
    with ThreadPoolExecutor(threads) as ex:
        t0 = time.perf_counter()
        kd_counts = list(ex.map(kd, host))
        kd_ms = (time.perf_counter() - t0) * 1e3
    return dict(stage='match_pairs', pairs=n, H=H, W=W, match_pairs_call_ms=round(gpu_ms, 2), per_pair_find_reciprocal_matches_ms=round(per_pair_ms, 2),
                scipy_kdtree_ms=round(kd_ms, 1), host_threads=threads, identical=bool(same),
                matches=sum(len(a[0]) for a in got), kdtree_matches=sum(kd_counts))


def _numpy_ransac(job, seed=0):
    """numpy restatement of the device RANSAC: same sampler, P3P from the host build, vectorised scoring, same stopping rule"""
    from dust3r_amd.visloc.localization import PNP_SETTINGS
    uv, X, fx, fy, cx, cy, thr = job
    max_iters, conf = PNP_SETTINGS['cv2']
    n = len(uv)
    best, niters, h = 0, max_iters, 0
    lib = _lib.lib
    pose = np.zeros(12)
    a, b = uv[:, 0] - cx, uv[:, 1] - cy
    rng = np.random.default_rng(seed)
    while h < niters:
        idx = rng.choice(n, 4, replace=False)
        if lib.d3r_selftest_p3p_host(np.ascontiguousarray(uv[idx], np.float64).ctypes.data_as(C.c_void_p),
                                     np.ascontiguousarray(X[idx], np.float64).ctypes.data_as(C.c_void_p), fx, fy, cx, cy,
                                     pose.ctypes.data_as(C.c_void_p)):
            P = pose.reshape(3, 4)
            Y = X @ P[:, :3].T.astype(np.float32) + P[:, 3].astype(np.float32)
            ex, ey = fx * Y[:, 0] - a * Y[:, 2], fy * Y[:, 1] - b * Y[:, 2]
            c = int(((Y[:, 2] > 0) & (ex * ex + ey * ey <= thr * thr * Y[:, 2] ** 2)).sum())
            if c > max(best, 3):
                best = c
                niters = lib.d3r_selftest_ransac_iters_host(conf, (n - c) / n, 4, niters)
        h += 1
    return best


def bench_pnp(dev, threads, reps):
    from dust3r_amd.synthetic import PNP_K as K, pnp_problem
    jobs = [pnp_problem(100_000, 0.3, 0.5, seed=1000 + k) for k in range(100)]
    pjobs = [(uv, X, K, None, 5.0) for uv, X, _, _ in jobs]
    L.run_pnp_batch(pjobs[:2], device=dev)
    # device time of the d3r_pnp_ransac call alone (inputs already resident)
    p2 = [torch.from_numpy(uv).to(dev) for uv, _, _, _ in jobs]
    p3 = [torch.from_numpy(X).to(dev) for _, X, _, _ in jobs]
    gpu_ms, res = _sync_ms(lambda: L.run_pnp_batch([(a, b, K, None, 5.0) for a, b in zip(p2, p3)], device=dev), reps)
    ok = sum(r[0] for r in res)
    # 'pycolmap' mode: a 100 000-hypothesis budget, so 782 rounds are launched although every job stops after its first few
    colmap_ms, _ = _sync_ms(lambda: L.run_pnp_batch([(a, b, K, None, 5.0) for a, b in zip(p2, p3)], mode='pycolmap', device=dev), reps)
    host_jobs = [(uv, X, K[0, 0], K[1, 1], K[0, 2], K[1, 2], 5.0) for uv, X, _, _ in jobs]
    with ThreadPoolExecutor(threads) as ex:
        t0 = time.perf_counter()
        host_best = list(ex.map(_numpy_ransac, host_jobs))
        host_ms = (time.perf_counter() - t0) * 1e3
    return dict(stage='pnp_ransac', jobs=100, points=100_000, outliers=0.3, gpu_call_ms=round(gpu_ms, 2), gpu_call_pycolmap_mode_ms=round(colmap_ms, 2), numpy_ransac_ms=round(host_ms, 1),
                host_threads=threads, successes=int(ok), numpy_min_support=int(min(host_best)))


class _Picture:                      # what localize reads of a query's 'rgb' (a PIL image in the reference datasets): its size
    def __init__(self, W, H):
        self.size = (W, H)


def bench_localize(dev, reps):
    from dust3r_amd.inference import inference
    from dust3r_amd.model import AsymmetricCroCo3DStereo
    from dust3r_amd.synthetic import MODEL_CONFIGS
    from dust3r_amd.utils.geometry import find_reciprocal_matches, geotrf, xy_grid
    from oracle.dust3r_ref import build_ref_model
    m = AsymmetricCroCo3DStereo(landscape_only=False, **MODEL_CONFIGS['tiny_dpt'])
    m.load_state_dict(build_ref_model('tiny_dpt').state_dict())
    model = m.to(dev)
    H, W = 64, 96
    g = torch.Generator(device='cpu').manual_seed(1)
    queries = []
    for _ in range(20):
        views = [dict(rgb_rescaled=torch.rand((3, H, W), generator=g) * 2 - 1, to_orig=np.diag([2.0, 2.0, 1.0]), rgb=_Picture(2 * W, 2 * H),
                      intrinsics=np.array([[150.0, 0, W], [0, 150.0, H], [0, 0, 1]]), distortion=None)]
        for _ in range(10):
            views.append(dict(rgb_rescaled=torch.rand((3, H, W), generator=g) * 2 - 1, pts3d_rescaled=torch.randn((H, W, 3), generator=g),
                              valid_rescaled=torch.rand((H, W), generator=g) < 0.9))
        queries.append(views)
    L.localize(queries[:1], model, dev)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        L.localize(queries, model, dev)
    torch.cuda.synchronize()
    batched_ms = (time.perf_counter() - t0) * 1e3 / reps

    def loop():
        for views in queries:
            qv = views[0]
            q2d, q3d = [], []
            for mv in views[1:]:
                imgs = [dict(img=img.unsqueeze(0), true_shape=np.int32([img.shape[1:]]), idx=i, instance=str(i))
                        for i, img in enumerate([qv['rgb_rescaled'], mv['rgb_rescaled']])]
                out = inference([tuple(imgs)], model, dev, batch_size=1, verbose=False)
                masks = [(out['pred1']['conf'][0] >= 3.0).numpy(), ((out['pred2']['conf'][0] >= 3.0) & mv['valid_rescaled']).numpy()]
                pts = [out['pred1']['pts3d'][0].numpy()[masks[0]], out['pred2']['pts3d_in_other_view'][0].numpy()[masks[1]]]
                grids = [xy_grid(W, H)[masks[0]], xy_grid(W, H)[masks[1]]]
                if len(pts[0]) == 0 or len(pts[1]) == 0:
                    continue
                recip, nn2, _ = find_reciprocal_matches(pts[0], pts[1])
                m1 = grids[1][recip]
                m0 = geotrf(qv['to_orig'], grids[0][nn2][recip].astype(np.float64) + 0.5, norm=True) - 0.5
                if len(m1):
                    q3d.append(mv['pts3d_rescaled'][m1[:, 1], m1[:, 0]].numpy())
                    q2d.append(m0)
            if q2d:
                L.run_pnp(np.concatenate(q2d).astype(np.float32), np.concatenate(q3d), qv['intrinsics'], None)
    loop()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    loop()
    torch.cuda.synchronize()
    loop_ms = (time.perf_counter() - t0) * 1e3
    return dict(stage='localize', queries=20, map_views=10, H=H, W=W, model='tiny_dpt', batched_ms=round(batched_ms, 1), per_query_loop_ms=round(loop_ms, 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--threads', type=int, default=16)
    ap.add_argument('--reps', type=int, default=5)
    args = ap.parse_args()
    _lib.require_device()
    dev = torch.device('cuda:0')
    rows = [bench_match(dev, args.threads, args.reps), bench_pnp(dev, args.threads, args.reps), bench_localize(dev, args.reps)]
    for r in rows:
        print(json.dumps(r), flush=True)
    assert rows[0]['identical'], 'd3r_match_pairs differs from find_reciprocal_matches'
    return rows


if __name__ == '__main__':
    main()
