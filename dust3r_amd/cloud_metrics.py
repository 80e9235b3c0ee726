"""Cloud-to-cloud metrics on the GPU (new; the reference's paper reports them, its code has none): accuracy, completeness, overall (Chamfer),
precision / recall / F-score at a distance, of one cloud against another -- csrc/cloud_nn.hip, C ABI `d3r_cloud_grid_build` /
`d3r_cloud_nearest` / `d3r_cloud_distance_stats` (include/dust3r_hip.h).

    d2, idx = nearest_in_cloud(query, ref, max_dist)        # the truncated exact nearest neighbour of every query point
    m = cloud_metrics(pred, gt, max_dist, thresholds)       # the dict of the metrics

The nearest neighbour is DEFINED without a grid: for a query with three finite coordinates, the lowest index among the reference points
(with three finite coordinates) of minimal fp32 squared distance, when that minimum is <= max_dist^2 (fp32); else, and for a non-finite
query, idx = -1 and d2 = +inf. The kernels give what an fp32 brute force over all pairs gives, bit for bit ("Cloud metrics").
A uniform grid with cells as large as max_dist would make every query walk thousands of points when the clouds are much denser than
max_dist, so the search runs as a radius ladder: r_k = min(r_0 4^k, max_dist), each pass on a grid of cell r_k and only for the queries no
earlier pass resolved. A neighbour found within r_k is the global nearest and all its ties lie within r_k, so the ladder's result is the
single search's at max_dist."""
import ctypes as C
import math

import numpy as np
import torch

from . import _lib
from ._lib import check, current_stream, lib, ptr

MAX_THRESHOLDS = 8      # D3R_CLOUD_MAX_THRESHOLDS
LADDER_STEP = 4.0


def _radius_f32(x, what):
    """x as np.float32; ValueError unless it is positive and its fp32 square is a normal number (about 1.1e-19 <= x <= 1.8e19): with a
    subnormal or infinite r r the comparison d2 <= r r no longer bounds the coordinates, and the grid's argument needs that"""
    with np.errstate(over='ignore', under='ignore'):
        v = np.float32(x)
        v2 = v * v
    if not (v > 0 and np.isfinite(v2) and v2 >= np.finfo(np.float32).tiny):
        raise ValueError(f'{what} = {x!r} must be a positive float32 whose square is a normal float32')
    return v


def default_r0(ref, max_dist):
    """the first radius of the ladder: twice the reference cloud's voxel size when it is a FusedCloud with one, else max_dist / 16"""
    voxel = getattr(ref, 'voxel_size', None)
    return 2.0 * voxel if voxel is not None and math.isfinite(voxel) and voxel > 0 else float(max_dist) / 16


def _device_of(*clouds):
    for c in clouds:
        c = getattr(c, 'positions', c)
        if isinstance(c, torch.Tensor) and c.is_cuda:
            return c.device
    return torch.device('cuda')


def _points(cloud, device, what):
    """(N, 3) float32 contiguous on the device, from an array, a tensor or a FusedCloud"""
    p = getattr(cloud, 'positions', cloud)
    t = p if isinstance(p, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(p, dtype=np.float32)))
    if t.ndim != 2 or t.shape[1] != 3:
        raise ValueError(f'{what}: expected (N, 3) points, got {tuple(t.shape)}')
    if len(t) >= 2 ** 31:
        raise ValueError(f'{what}: {len(t)} points do not fit 31-bit indices')
    return t.to(device=device, dtype=torch.float32).contiguous()


def ladder_radii(r0, max_dist):
    """r_k = min(r_0 4^k, max_dist) as float32; the last is exactly max_dist"""
    r0, max_dist = _radius_f32(r0, 'r0'), _radius_f32(max_dist, 'max_dist')
    out, k = [], 0
    while True:
        r = np.float32(min(float(r0) * LADDER_STEP ** k, float(max_dist)))
        if not r < max_dist:
            return out + [max_dist]
        out.append(r)
        k += 1


def grid_cell(lo, hi, r):
    """(cell, bits): cell = r, doubled until every axis of the extent fits 21 bits (viz.fuse_key_bits)"""
    from .viz import fuse_key_bits
    cell = np.float32(r)
    while True:
        try:
            return cell, fuse_key_bits(lo, hi, cell)
        except ValueError:
            if not np.isfinite(cell * np.float32(2)):
                raise
            cell = cell * np.float32(2)


def _bounds(pts, device):
    """(lo, hi, n_valid) of the finite points: d3r_fuse_bounds on the cloud as one view of 1 x n. One host synchronisation."""
    n = len(pts)
    ones = torch.ones((n,), dtype=torch.uint8, device=device)
    h, w = torch.ones((1,), dtype=torch.int32, device=device), torch.full((1,), n, dtype=torch.int32, device=device)
    small = torch.empty((4,), dtype=torch.int64, device=device)
    work = torch.empty(max(1, int(lib.d3r_fuse_bounds_workspace_bytes(1, n))), dtype=torch.uint8, device=device)
    check(lib.d3r_fuse_bounds(1, ptr(pts), ptr(ones), None, ptr(h), ptr(w), n, ptr(small.view(torch.float32)), ptr(small[3:]), ptr(work),
                              current_stream()), 'fuse_bounds')
    host = small.cpu()
    b = host[:3].view(torch.float32).numpy()
    return b[:3].copy(), b[3:].copy(), int(host[3])


@torch.no_grad()
def nearest_in_cloud(query, ref, max_dist, r0=None, to_host=True, evals=None):
    """(d2, idx) of every query point in `ref` within max_dist, as defined at the top: d2 (N,) float32 squared distances (+inf where none),
    idx (N,) int32 rows of `ref` (-1 where none). query, ref: (N, 3) arrays, tensors or FusedClouds. r0: the first radius of the ladder;
    default twice ref.voxel_size for a FusedCloud, else max_dist / 16. One host synchronisation (the reference cloud's bounds). evals
    (optional): an int32 device tensor (N,) that accumulates the distance evaluations per query (tools/cloud_metrics_speed.py)."""
    max_dist = _radius_f32(max_dist, 'max_dist')
    _lib.require_device()
    device = _device_of(query, ref)
    if r0 is None:
        r0 = default_r0(ref, max_dist)
    radii = ladder_radii(min(float(_radius_f32(r0, 'r0')), float(max_dist)), max_dist)
    Q, R = _points(query, device, 'query'), _points(ref, device, 'ref')
    nq, nr = len(Q), len(R)
    d2 = torch.full((nq,), float('inf'), dtype=torch.float32, device=device)
    idx = torch.full((nq,), -1, dtype=torch.int32, device=device)
    if nq > 0 and nr > 0:
        with torch.cuda.device(device):
            lo, hi, n_valid = _bounds(R, device)
            if n_valid > 0:
                size = int(lib.d3r_cloud_grid_workspace_bytes(nr, nq))
                if size == 0:
                    raise ValueError(f'nearest_in_cloud: clouds of {nq} and {nr} points are too large')
                work = torch.empty(size, dtype=torch.uint8, device=device)
                lo_c = (C.c_float * 3)(*lo.tolist())
                for k, r in enumerate(radii):
                    cell, bits = grid_cell(lo, hi, r)
                    bits_c = (C.c_int * 3)(*bits)
                    check(lib.d3r_cloud_grid_build(nr, ptr(R), lo_c, float(cell), bits_c, ptr(work), current_stream()), 'cloud_grid_build')
                    check(lib.d3r_cloud_nearest(nr, nq, ptr(Q), float(r), lo_c, float(cell), bits_c, int(k > 0), ptr(d2), ptr(idx), ptr(evals),
                                                ptr(work), current_stream()), 'cloud_nearest')
    if to_host:
        return d2.cpu().numpy(), idx.cpu().numpy()
    return d2, idx


@torch.no_grad()
def distance_stats(points, d2, idx, thresholds):
    """The sums and counts of one direction, on the device: counts (2 + 8,) int64 = (n_valid, n_found, count_j ...), sums (2,) float64 =
    (sum of distances, sum of squared distances) over the found points, median_d2 (1,) float64 = the lower median of d2 over the found
    points (NaN when none). d3r_cloud_distance_stats and d3r_masked_median; no synchronisation."""
    if len(thresholds) > MAX_THRESHOLDS:
        raise ValueError(f'at most {MAX_THRESHOLDS} thresholds, got {len(thresholds)}')
    tau = [float(np.float32(t)) for t in thresholds]
    if not all(math.isfinite(t) and t >= 0 for t in tau):
        raise ValueError(f'thresholds must be finite and >= 0: {list(thresholds)!r}')
    _lib.require_device()
    device = d2.device
    n = len(d2)
    counts = torch.zeros((2 + MAX_THRESHOLDS,), dtype=torch.int64, device=device)
    sums = torch.zeros((2,), dtype=torch.float64, device=device)
    median = torch.full((1,), float('nan'), dtype=torch.float64, device=device)
    if n > 0:
        with torch.cuda.device(device):
            work = torch.empty(int(lib.d3r_cloud_distance_stats_workspace_bytes(n)), dtype=torch.uint8, device=device)
            check(lib.d3r_cloud_distance_stats(n, ptr(points), ptr(d2), ptr(idx), len(tau), (C.c_float * max(len(tau), 1))(*tau), ptr(counts), ptr(sums),
                                               ptr(work), current_stream()), 'cloud_distance_stats')
            found = (idx >= 0).to(torch.uint8)
            work = torch.empty(int(lib.d3r_pair_criterion_workspace_bytes(1, n)), dtype=torch.uint8, device=device)
            check(lib.d3r_masked_median(1, n, ptr(d2), None, ptr(found), None, ptr(median), ptr(work), current_stream()), 'masked_median')
    return counts, sums, median


def compose_metrics(pred, gt, thresholds):
    """The dict of `cloud_metrics` from the two directions' numbers; pred, gt: dicts with n_valid, n_found, sum_d, sum_d2, median_d2 and
    counts (one per threshold). Host arithmetic in fp64. The DTU convention: the means run over the FOUND points (pairs beyond max_dist are
    outliers, not clamped), NaN when none is found; precision / recall are over the VALID points, NaN when there is none."""
    def mean(s):
        return s['sum_d'] / s['n_found'] if s['n_found'] > 0 else float('nan')

    def median(s):
        return math.sqrt(s['median_d2']) if s['n_found'] > 0 else float('nan')

    def ratio(a, b):
        return a / b if b > 0 else float('nan')
    acc, comp = mean(pred), mean(gt)
    precision = [ratio(c, pred['n_valid']) for c in pred['counts']]
    recall = [ratio(c, gt['n_valid']) for c in gt['counts']]
    fscore = [0.0 if p + r == 0 else 2 * p * r / (p + r) for p, r in zip(precision, recall)]
    out = dict(accuracy=acc, accuracy_median=median(pred), completeness=comp, completeness_median=median(gt), overall=(acc + comp) / 2,
               thresholds=[float(t) for t in thresholds], precision=precision, recall=recall, fscore=fscore,
               outliers_pred=1 - ratio(pred['n_found'], pred['n_valid']), outliers_gt=1 - ratio(gt['n_found'], gt['n_valid']))
    for side, s in (('pred', pred), ('gt', gt)):
        out.update({f'n_valid_{side}': int(s['n_valid']), f'n_found_{side}': int(s['n_found']), f'sum_d_{side}': float(s['sum_d']),
                    f'sum_d2_{side}': float(s['sum_d2']), f'median_d2_{side}': float(s['median_d2']), f'counts_{side}': [int(c) for c in s['counts']]})
    return out


def _side(counts, sums, median, n_tau):
    counts, sums, median = counts.tolist(), sums.tolist(), median.tolist()
    return dict(n_valid=counts[0], n_found=counts[1], counts=counts[2:2 + n_tau], sum_d=sums[0], sum_d2=sums[1], median_d2=median[0])


@torch.no_grad()
def cloud_metrics(pred, gt, max_dist, thresholds, to_host=True, r0=None, details=None):
    """The metrics of a predicted cloud against a ground-truth cloud, distances truncated at max_dist (see `compose_metrics`):
    accuracy / accuracy_median (pred -> gt), completeness / completeness_median (gt -> pred), overall, precision / recall / fscore per
    threshold, outliers_pred / outliers_gt, and the raw counts and sums. pred, gt: (N, 3) arrays, tensors or FusedClouds. to_host=False:
    the raw device tensors (pred=(counts, sums, median_d2), gt=...) without a synchronisation beyond the two bounds read-backs; compose
    them with `compose_metrics` later. details: a dict that receives d2 / idx of both directions (device tensors)."""
    thresholds = list(thresholds)
    _lib.require_device()
    device = _device_of(pred, gt)
    P, G = _points(pred, device, 'pred'), _points(gt, device, 'gt')
    d2p, ip = nearest_in_cloud(P, G, max_dist, r0=default_r0(gt, max_dist) if r0 is None else r0, to_host=False)
    d2g, ig = nearest_in_cloud(G, P, max_dist, r0=default_r0(pred, max_dist) if r0 is None else r0, to_host=False)
    sp, sg = distance_stats(P, d2p, ip, thresholds), distance_stats(G, d2g, ig, thresholds)
    if details is not None:
        details.update(d2_pred=d2p, idx_pred=ip, d2_gt=d2g, idx_gt=ig)
    if not to_host:
        return dict(pred=sp, gt=sg, thresholds=thresholds)
    packed = torch.cat([t.double() for t in sp + sg]).cpu()            # one read-back (int64 counts are exact in fp64 below 2^53)
    k = 2 + MAX_THRESHOLDS
    cut = lambda o: (packed[o:o + k].long(), packed[o + k:o + k + 2], packed[o + k + 2:o + k + 3])      # noqa: E731
    return compose_metrics(_side(*cut(0), len(thresholds)), _side(*cut(k + 3), len(thresholds)), thresholds)
