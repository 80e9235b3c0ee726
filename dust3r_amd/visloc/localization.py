"""Mirror of the reference's `dust3r_visloc/localization.py` (`run_pnp`) plus the batched pieces of its caller, the per-query loop of
`visloc.py:72-165`: mutual nearest-neighbour matching of many (query, map view) pairs in one `d3r_match_pairs` call, PnP-RANSAC of many
queries in one `d3r_pnp_ransac` call (csrc/visloc.hip), and `localize`, which runs the whole loop for many queries at once.

Differences from the reference, by design:
  * no mode is RNG-identical to its library: 'cv2' (OpenCV SOLVEPNP_SQPNP RANSAC), 'poselib' and 'pycolmap' all run the same solver
    (P3P minimal samples, Levenberg-Marquardt polish), each with its library's iteration / confidence settings. The reference's
    +0.5 pixel-centre shift and OpenCV -> COLMAP intrinsics conversion of the last two modes cancel and are not applied.
  * the sampler is a counter-based generator keyed by `seed` and the hypothesis index: results are deterministic, and do not
    depend on the other jobs of a batch.
  * 'pycolmap' keeps its library's 100 000-hypothesis budget and confidence, not its `min_num_trials=1000` floor: the stopping rule
    alone ends a job (after at least one round of 128 hypotheses).
  * `run_pnp` lets errors propagate, where the reference catches every exception, prints it and returns (False, None): a device or
    input error here is a fault to report, not a query that failed to localize.
  * `localize` subsamples to `pnp_max_points` with a seeded generator (`subsample_indices`); the reference's `random.sample` is not
    reproducible.
"""
import ctypes as C
import math

import numpy as np
import torch

from .. import _lib
from .._lib import MatchJob, PnpRansacJob, PnpRansacParams, check, current_stream, lib, ptr
from ..utils.geometry import geotrf

MAX_CALL = 65535                     # pairs per d3r_match_pairs call, jobs per d3r_pnp_ransac call (grid y / z limit)
# device bytes per (query, map view) pair and pixel in localize: the inference output kept on the device (fp32 pts3d + conf of both
# views, 32 B), the d3r_match_pairs workspace (48 B) and its pair buffer (8 B). 512 x 384: about 17 MB per pair.
BYTES_PER_PAIR_PIXEL = 88
PNP_SETTINGS = {                     # mode -> (hypothesis budget, confidence), as dust3r_visloc/localization.py sets them
    'cv2': (10_000, 0.9999),
    'poselib': (10_000, 0.9999),
    'pycolmap': (100_000, 0.9999),
}


def _device(device=None):
    if device is None:
        return torch.device('cuda', torch.cuda.current_device())
    return torch.device(device)


def _records(recs, cls, dev):
    """ctypes records -> a DEVICE byte tensor holding the array"""
    arr = (cls * len(recs))(*recs)
    host = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8)
    return host.to(dev)


# ---- matching --------------------------------------------------------------------------------------------------------------------
def match_pairs(pairs, conf_thr, device=None):
    """Mutual nearest neighbours of many (query, map view) pointmap pairs in one d3r_match_pairs call.

    pairs: list of (pts_query (H0, W0, 3), conf_query (H0, W0), pts_map (H1, W1, 3), conf_map (H1, W1), valid_map (H1, W1) bool or None).
    A query pixel is used when conf >= conf_thr, a map pixel when conf >= conf_thr and valid (visloc.py:90-91). Returns one
    (query_pixel, map_pixel) pair of int64 DEVICE tensors of flat pixel indices per pair, in ascending map order: the
    `pts2d_list[0][nnM_in_PQ][reciprocal_in_PM]` / `pts2d_list[1][reciprocal_in_PM]` of visloc.py:105-107."""
    _lib.require_device()
    dev = _device(device)
    if len(pairs) > MAX_CALL:
        return [m for i in range(0, len(pairs), MAX_CALL) for m in match_pairs(pairs[i:i + MAX_CALL], conf_thr, dev)]
    if len(pairs) == 0:
        return []
    keep, jobs = [], []
    for pq, cq, pm, cm, vm in pairs:
        pq = torch.as_tensor(pq).to(dev, torch.float32).contiguous()
        cq = torch.as_tensor(cq).to(dev, torch.float32).contiguous()
        pm = torch.as_tensor(pm).to(dev, torch.float32).contiguous()
        cm = torch.as_tensor(cm).to(dev, torch.float32).contiguous()
        vm = None if vm is None else torch.as_tensor(vm).to(dev).to(torch.uint8).contiguous()
        nq, nm = cq.numel(), cm.numel()
        assert pq.numel() == 3 * nq and pm.numel() == 3 * nm and (vm is None or vm.numel() == nm), 'pointmap / confidence shapes differ'
        keep += [pq, cq, pm, cm, vm]
        jobs.append(MatchJob(pq.data_ptr(), cq.data_ptr(), pm.data_ptr(), cm.data_ptr(), vm.data_ptr() if vm is not None else None,
                             nq, nm, float(conf_thr), 0))
    max_pixels = max(max(j.n_query, j.n_map) for j in jobs)
    n = len(jobs)
    with torch.cuda.device(dev):
        rec = _records(jobs, MatchJob, dev)
        work = _lib.workspace(lib.d3r_match_pairs_workspace(n, max_pixels), dev)
        counts = torch.empty(n, dtype=torch.int32, device=dev)
        out = torch.empty((n, max_pixels, 2), dtype=torch.int32, device=dev)
        check(lib.d3r_match_pairs(n, ptr(rec), max_pixels, ptr(work), ptr(counts), ptr(out), current_stream()), 'match_pairs')
        counts = counts.cpu().tolist()
    return [(out[i, :c, 0].long(), out[i, :c, 1].long()) for i, c in enumerate(counts)]


# ---- undistortion / PnP ---------------------------------------------------------------------------------------------------------
def undistort_points(pts2D, K, distortion, iterations=5):
    """cv2.undistortPoints(pts2D, K, distortion, R=None, P=K) for the 4-coefficient OpenCV model (k1, k2, p1, p2): OpenCV's
    fixed-point iteration with its default criteria (5 iterations), in fp64 on the tensor's device. Returns fp64 pixels."""
    pts = torch.as_tensor(pts2D).to(torch.float64)
    K = torch.as_tensor(np.asarray(K, dtype=np.float64), device=pts.device)
    k1, k2, p1, p2 = (list(np.asarray(distortion, dtype=np.float64).ravel()) + [0.0] * 4)[:4]
    fx, fy, cx, cy, skew = K[0, 0], K[1, 1], K[0, 2], K[1, 2], K[0, 1]
    y0 = (pts[:, 1] - cy) / fy
    x0 = (pts[:, 0] - cx - skew * y0) / fx
    x, y = x0.clone(), y0.clone()
    frozen = torch.zeros_like(x0, dtype=torch.bool)
    for _ in range(iterations):
        r2 = x * x + y * y
        icdist = 1.0 / (1.0 + (k2 * r2 + k1) * r2)
        frozen = frozen | (icdist < 0)                 # OpenCV stops there and keeps the distorted coordinates
        dx = 2 * p1 * x * y + p2 * (r2 + 2 * x * x)
        dy = p1 * (r2 + 2 * y * y) + 2 * p2 * x * y
        x = torch.where(frozen, x0, (x0 - dx) * icdist)
        y = torch.where(frozen, y0, (y0 - dy) * icdist)
    hx = K[0, 0] * x + K[0, 1] * y + K[0, 2]
    hy = K[1, 0] * x + K[1, 1] * y + K[1, 2]
    hw = K[2, 0] * x + K[2, 1] * y + K[2, 2]
    return torch.stack((hx / hw, hy / hw), dim=-1)


def run_pnp_batch(jobs, mode='cv2', seed=0, device=None, return_inliers=False, return_stats=False):
    """PnP-RANSAC of many problems in one d3r_pnp_ransac call (one per MAX_CALL jobs). jobs: list of (pts2D (n, 2), pts3D (n, 3),
    K (3, 3), distortion (4 OpenCV coefficients) or None, reprojectionError in pixels). Returns one (True, cam2world 4x4 float64) or
    (False, None) per job (with return_inliers: (success, cam2world, inlier mask bool numpy or None)). Problems with n <= 4 fail
    without a launch. return_stats: (results, stats) with stats[k] = (hypotheses drawn, index of the best one), None without a launch."""
    assert mode in PNP_SETTINGS, mode
    if len(jobs) > MAX_CALL:
        parts = [run_pnp_batch(jobs[i:i + MAX_CALL], mode, seed, device, return_inliers, return_stats) for i in range(0, len(jobs), MAX_CALL)]
        if not return_stats:
            return [r for part in parts for r in part]
        return [r for part in parts for r in part[0]], [t for part in parts for t in part[1]]
    max_iters, confidence = PNP_SETTINGS[mode]
    _lib.require_device()
    dev = _device(device)
    results = [None] * len(jobs)
    stats = [None] * len(jobs)
    keep, recs, where = [], [], []
    for k, (pts2D, pts3D, K, distortion, reproj) in enumerate(jobs):
        n = len(pts2D)
        if n <= 4:
            results[k] = (False, None, None) if return_inliers else (False, None)
            continue
        assert len(pts3D) == n
        p2 = torch.as_tensor(pts2D).to(dev)
        if distortion is not None:
            p2 = undistort_points(p2, K, distortion)
        p2 = p2.to(torch.float32).reshape(n, 2).contiguous()
        p3 = torch.as_tensor(pts3D).to(dev, torch.float32).reshape(n, 3).contiguous()
        mask = torch.empty(n, dtype=torch.uint8, device=dev)
        K = np.asarray(K, dtype=np.float64)
        keep += [p2, p3, mask]
        recs.append(PnpRansacJob(p2.data_ptr(), p3.data_ptr(), mask.data_ptr(), n, max_iters, float(K[0, 0]), float(K[1, 1]), float(K[0, 2]),
                                 float(K[1, 2]), float(reproj), float(confidence), int(seed) & 0xFFFFFFFFFFFFFFFF))
        where.append((k, mask))
    if recs:
        m = len(recs)
        params = PnpRansacParams(max(r.max_iters for r in recs), max(r.n for r in recs))
        with torch.cuda.device(dev):
            rec = _records(recs, PnpRansacJob, dev)
            work = _lib.workspace(lib.d3r_pnp_ransac_workspace(m, params.max_points), dev)
            poses = torch.empty((m, 12), dtype=torch.float64, device=dev)
            inl = torch.empty(m, dtype=torch.int32, device=dev)
            status = torch.empty(m, dtype=torch.int32, device=dev)
            st = torch.empty((m, 2), dtype=torch.int32, device=dev)
            check(lib.d3r_pnp_ransac(m, ptr(rec), C.byref(params), ptr(work), ptr(poses), ptr(inl), ptr(status), ptr(st),
                                     current_stream()), 'pnp_ransac')
            poses, status, st = poses.cpu().numpy(), status.cpu().numpy(), st.cpu().numpy()
        for r, (k, mask) in enumerate(where):
            stats[k] = (int(st[r, 0]), int(st[r, 1]))
            if not status[r]:
                results[k] = (False, None, None) if return_inliers else (False, None)
                continue
            w2c = np.eye(4)
            w2c[:3, :] = poses[r].reshape(3, 4)
            c2w = np.linalg.inv(w2c)
            results[k] = (True, c2w, mask.bool().cpu().numpy()) if return_inliers else (True, c2w)
    return (results, stats) if return_stats else results


def run_pnp(pts2D, pts3D, K, distortion=None, mode='cv2', reprojectionError=5, img_size=None, seed=0):
    """dust3r_visloc.localization.run_pnp: (True, cam2world 4x4 float64) or (False, None); len(pts2D) <= 4 fails. `distortion`: the
    4-coefficient OpenCV model. `img_size` is accepted for the signature (the reference only hands it to the COLMAP camera record)."""
    assert mode in ['cv2', 'poselib', 'pycolmap']
    if len(pts2D) <= 4:
        return False, None
    return run_pnp_batch([(pts2D, pts3D, K, distortion, reprojectionError)], mode=mode, seed=seed)[0]


# ---- the visloc.py loop, batched --------------------------------------------------------------------------------------------------
def subsample_indices(n, k, seed, query_index):
    """The `pnp_max_points` subsample of one query: k of n indices without replacement, from a generator seeded by (seed, query)."""
    return np.random.default_rng((int(seed), int(query_index))).choice(n, size=k, replace=False)


def _pixels_to_orig(pix, width, to_orig):
    """flat pixel indices of the rescaled query -> original-image coordinates (visloc.py:109-122): +0.5, to_orig, -0.5; fp64"""
    xy = torch.stack(((pix % width).double(), (pix // width).double()), dim=-1) + 0.5
    xy = geotrf(torch.as_tensor(np.asarray(to_orig, dtype=np.float64), device=xy.device), xy, norm=True)
    return xy - 0.5


def _pair_images(query_view, map_view):
    imgs = []
    for idx, img in enumerate([query_view['rgb_rescaled'], map_view['rgb_rescaled']]):
        imgs.append(dict(img=img.unsqueeze(0), true_shape=np.int32([img.shape[1:]]), idx=idx, instance=str(idx)))
    return tuple(imgs)


def localize(queries, model, device, conf_thr=3.0, reprojection_error=5.0, reprojection_error_diag_ratio=None, pnp_max_points=100_000,
             seed=0, output=None, pnp_mode='cv2', max_pairs_per_call=256):
    """The per-query loop of visloc.py:72-165 for many queries at once. queries: list of view lists in the reference dataset format
    (views[0] the query with 'rgb_rescaled', 'to_orig', 'intrinsics', 'distortion', 'rgb'; views[1:] map views that also have
    'pts3d_rescaled' and 'valid_rescaled'). `output`: a precomputed inference() result over all (query, map view) pairs in that order.
    Returns (results, match_counts): results[q] = (success, cam2world 4x4 float64 or None); match_counts[q] = the number of mutual
    matches with each map view.

    The queries are processed in chunks of whole queries with at most `max_pairs_per_call` pairs (a query with more map views forms a
    chunk of its own). Per chunk: one inference() over its pairs, one d3r_match_pairs call, the rescale and the 3-D gather on the
    device, the seeded subsample, one d3r_pnp_ransac call. Every stage is independent per pair and per query, so the result is the same
    bits for any chunk size; the chunk size bounds device memory at about BYTES_PER_PAIR_PIXEL bytes per pair and pixel (17 MB per
    512 x 384 pair, 4.4 GB for the default 256 pairs)."""
    assert max_pairs_per_call >= 1
    dev = _device(device)
    results, match_counts = [], []
    q0, p0 = 0, 0
    while q0 < len(queries):
        q1, npairs = q0, 0
        while q1 < len(queries) and (q1 == q0 or npairs + len(queries[q1]) - 1 <= max_pairs_per_call):
            npairs += len(queries[q1]) - 1
            q1 += 1
        res, cnt = _localize_chunk(queries, q0, q1, p0, model, dev, conf_thr, reprojection_error, reprojection_error_diag_ratio,
                                   pnp_max_points, seed, output, pnp_mode)
        results += res
        match_counts += cnt
        q0, p0 = q1, p0 + npairs
    return results, match_counts


def _localize_chunk(queries, q0, q1, p0, model, dev, conf_thr, reprojection_error, reprojection_error_diag_ratio, pnp_max_points, seed,
                    output, pnp_mode):
    """localize() for queries[q0:q1], whose pairs are p0, p0 + 1, ... of the whole list (the rows of a precomputed `output`)"""
    from ..inference import inference
    pairs, owner = [], []
    for q in range(q0, q1):
        views = queries[q]
        for m in range(1, len(views)):
            pairs.append(_pair_images(views[0], views[m]))
            owner.append((q, m))
    if output is None:
        base = 0
        output = inference(pairs, model, dev, batch_size=1, verbose=False, output_device=dev) if pairs else None
    else:
        base = p0
    match_in = []
    for p, (q, m) in enumerate(owner):
        map_view = queries[q][m]
        match_in.append((output['pred1']['pts3d'][base + p], output['pred1']['conf'][base + p],
                         output['pred2']['pts3d_in_other_view'][base + p], output['pred2']['conf'][base + p], map_view['valid_rescaled']))
    matches = match_pairs(match_in, conf_thr, dev)
    per_query = {q: ([], []) for q in range(q0, q1)}
    match_counts = {q: [] for q in range(q0, q1)}
    for p, (q, m) in enumerate(owner):
        qpix, mpix = matches[p]
        match_counts[q].append(int(qpix.numel()))
        if qpix.numel() == 0:
            continue
        query_view, map_view = queries[q][0], queries[q][m]
        width = int(query_view['rgb_rescaled'].shape[2])
        pts3d = torch.as_tensor(map_view['pts3d_rescaled']).to(dev).reshape(-1, 3)[mpix]
        per_query[q][0].append(_pixels_to_orig(qpix, width, query_view['to_orig']))
        per_query[q][1].append(pts3d)
    jobs, job_query = [], []
    results = {q: (False, None) for q in range(q0, q1)}
    for q, (p2, p3) in per_query.items():
        if not p2:
            continue
        p2 = torch.cat(p2).to(torch.float32)
        p3 = torch.cat(p3)
        if len(p2) > pnp_max_points:
            idx = torch.as_tensor(subsample_indices(len(p2), pnp_max_points, seed, q), device=dev)
            p2, p3 = p2[idx], p3[idx]
        query_view = queries[q][0]
        W, H = query_view['rgb'].size
        err = reprojection_error_diag_ratio * math.sqrt(W ** 2 + H ** 2) if reprojection_error_diag_ratio is not None else reprojection_error
        jobs.append((p2, p3, query_view['intrinsics'], query_view['distortion'], err))
        job_query.append(q)
    for q, res in zip(job_query, run_pnp_batch(jobs, mode=pnp_mode, seed=seed, device=dev)):
        results[q] = res
    return [results[q] for q in range(q0, q1)], [match_counts[q] for q in range(q0, q1)]
