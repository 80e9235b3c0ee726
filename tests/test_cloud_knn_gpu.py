"""The k nearest neighbours, normals and outlier removal of the fused cloud on the GPU: the kernels of csrc/cloud_knn.hip against the numpy
restatements of tests/test_cloud_knn_cpu.py. Neighbours are compared exactly (np.array_equal on d2 and idx): the definition is an fp32 brute
force over all pairs with np.lexsort, the kernel evaluates the same fp32 expression on a subset that holds every point within r. The mean
distances are compared exactly too (one fixed fp64 summation order, IEEE square roots), the reduced sums to 1e-12 relative, the normals to
the final fp32 rounding, the orientation's visibility exactly and its vote by sign. The clouds are a few thousand points."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch

from test_cloud_knn_cpu import (brute_force_knn, lead_positive, restated_means, restated_normals, restated_orientation, restated_threshold)
from test_cloud_metrics_cpu import brute_force, valid_rows

pytestmark = pytest.mark.gpu

F32 = np.float32
KS = [1, 7, 8, 9, 16, 17, 32]


# ---- 1. exact k neighbours ------------------------------------------------------------------------------------------------------------
def _isolated(R, max_dist, n=3):
    """n points beyond the cloud, 10 max_dist from it and from each other: rows without a candidate"""
    hi = R[valid_rows(R)].max(axis=0)
    return np.stack([hi + F32(10 * max_dist) * F32(j + 1) for j in range(n)]).astype(F32)


def _case(name):
    """(R, max_dist) of the named reference cloud"""
    rng = np.random.default_rng(sum(map(ord, name)))
    if name == 'uniform':          # a sparse cube and a dense corner: empty, short and full rows at one max_dist
        R = np.concatenate([rng.random((2000, 3)), rng.random((1000, 3)) * 0.2]).astype(F32)
        return np.concatenate([R, _isolated(R, 0.06)]), 0.06
    if name == 'one_cell':         # everything within one cell of the last rung; the four sites are s sqrt(2) > max_dist apart
        max_dist = 0.5
        s = F32(0.95 * max_dist)
        tiny = lambda n: (rng.random((n, 3)) * 0.02).astype(F32)      # noqa: E731
        return np.concatenate([tiny(2000), tiny(5) + F32([s, s, 0]), tiny(1) + F32([s, 0, s]), tiny(1) + F32([0, s, s])]), max_dist
    if name == 'lattice':          # integer coordinates: d2 in {0, 1, 2, 3, 4}, 32 neighbours within 2 inside the block, many ties
        g = np.arange(14, dtype=F32)
        R = np.stack(np.meshgrid(g, g, g, indexing='ij'), axis=-1).reshape(-1, 3)
        return np.concatenate([R[rng.permutation(len(R))], _isolated(R, 2.0)]), 2.0
    if name == 'duplicates':       # every point twice, at indices i and i + n: d2 = 0 ties fall to the lower index
        P = np.concatenate([rng.random((1000, 3)), rng.random((500, 3)) * 0.15]).astype(F32)
        return np.concatenate([P, P, _isolated(P, 0.08)]), 0.08
    if name == 'nonfinite':
        R = np.concatenate([rng.random((2500, 3)), rng.random((500, 3)) * 0.15]).astype(F32)
        R[::37, 0], R[5::53, 2], R[7::91, 1] = np.nan, np.inf, -np.inf
        return np.concatenate([R, _isolated(R, 0.07)]), 0.07
    if name == 'offset':           # one ulp at 1e4 is 1e-3: the cloud collapses onto the representable numbers
        R = (np.concatenate([rng.random((2000, 3)), rng.random((1000, 3)) * 0.2]) + 1e4).astype(F32)
        return np.concatenate([R, _isolated(R, 0.06)]), 0.06
    raise KeyError(name)


def _queries(R, max_dist, rng):
    """another cloud on the query side: jittered copies of every second reference point, far queries, non-finite rows"""
    ok = R[valid_rows(R)]
    Q = (ok[::2] + (rng.standard_normal((len(ok[::2]), 3)) * 0.3 * max_dist).astype(F32)).astype(F32)
    far = ok.max(axis=0) + F32(3 * max_dist) * (1 + rng.random((20, 3))).astype(F32)
    Q = np.concatenate([Q, far.astype(F32)])
    Q[3::61, 1], Q[11::83, 0] = np.nan, np.inf
    return Q


CASES = ['uniform', 'one_cell', 'lattice', 'duplicates', 'nonfinite', 'offset']


@pytest.fixture(scope='module')
def knn_reference():
    """the brute force at k = 32 of every (case, exclude_self), computed once; a smaller k is its first columns by definition"""
    cache = {}

    def get(name, exclude_self):
        if (name, exclude_self) not in cache:
            R, max_dist = _case(name)
            Q = R if exclude_self else _queries(R, max_dist, np.random.default_rng(len(name)))
            cache[name, exclude_self] = (Q, R, max_dist, brute_force_knn(Q, R, 32, max_dist, exclude_self=exclude_self))
        return cache[name, exclude_self]
    return get


@pytest.mark.parametrize('exclude_self', [False, True])
@pytest.mark.parametrize('name', CASES)
def test_exact_k_neighbours(gpu, knn_reference, name, exclude_self):
    """every k against the brute force, through a ladder of three rungs (r_0 = max_dist / 4, step 2); k = 1 against nearest_in_cloud; one
    rung alone; two runs give the same bytes. The inputs leave rows empty, short and full (asserted on the brute force)."""
    from dust3r_amd.cloud_metrics import KNN_LADDER_STEP, k_nearest, ladder_radii, nearest_in_cloud
    Q, R, max_dist, (want_d2, want_idx) = knn_reference(name, exclude_self)
    assert 2000 <= len(R) <= 4000
    n_cand = (want_idx >= 0).sum(axis=1)
    assert (n_cand == 0).sum() > (valid_rows(Q) == 0).sum() and ((n_cand > 0) & (n_cand < 32)).any() and (n_cand == 32).any()
    r0 = max_dist / 4
    assert len(ladder_radii(r0, max_dist, step=KNN_LADDER_STEP)) >= 3
    Qd, Rd = torch.from_numpy(Q).to(gpu), torch.from_numpy(R).to(gpu)
    if exclude_self:
        Qd = Rd
    for k in KS:
        d2, idx = k_nearest(Qd, Rd, k, max_dist, exclude_self=exclude_self, r0=r0)
        assert d2.dtype == F32 and idx.dtype == np.int32 and d2.shape == idx.shape == (len(Q), k)
        assert np.array_equal(idx, want_idx[:, :k]), k
        assert np.array_equal(d2, want_d2[:, :k]), k
    ev = torch.zeros(len(Q), dtype=torch.int32, device=gpu)
    one = k_nearest(Qd, Rd, 16, max_dist, exclude_self=exclude_self, r0=max_dist, evals=ev)                  # one rung: no ladder
    again = k_nearest(Q, R, 16, max_dist, exclude_self=exclude_self, r0=r0, to_host=False)                   # host arrays in, device out
    assert np.array_equal(one[1], want_idx[:, :16]) and np.array_equal(one[0], want_d2[:, :16])
    assert again[0].is_cuda and again[0].cpu().numpy().tobytes() == one[0].tobytes() and again[1].cpu().numpy().tobytes() == one[1].tobytes()
    assert (ev.cpu().numpy()[n_cand > 0] > 0).all()
    if not exclude_self:
        near = nearest_in_cloud(Qd, Rd, max_dist, r0=r0)
        got = k_nearest(Qd, Rd, 1, max_dist, r0=r0)
        assert np.array_equal(got[0][:, 0], near[0]) and np.array_equal(got[1][:, 0], near[1])
        want = brute_force(Q, R, max_dist)
        assert np.array_equal(near[1], want[1])


def test_k_nearest_arguments_and_empty_sides(gpu):
    from dust3r_amd.cloud_metrics import k_nearest
    rng = np.random.default_rng(5)
    Q, R = rng.random((300, 3)).astype(F32), rng.random((200, 3)).astype(F32)
    for k in (0, 33, -1):
        with pytest.raises(ValueError, match='outside'):
            k_nearest(Q, R, k, 0.5)
    with pytest.raises(ValueError, match='exclude_self needs'):
        k_nearest(Q, R, 4, 0.5, exclude_self=True)
    d2, idx = k_nearest(Q, np.full((50, 3), np.nan, F32), 5, 0.5)      # an empty reference after validity filtering
    assert d2.shape == (300, 5) and np.isinf(d2).all() and (idx == -1).all()
    d2, idx = k_nearest(np.zeros((0, 3), F32), R, 5, 0.5)
    assert d2.shape == (0, 5) and idx.shape == (0, 5)
    d2, idx = k_nearest(R[:3], R[:3], 8, 10.0, exclude_self=True)      # fewer reference points than k: two neighbours each
    assert ((idx >= 0).sum(axis=1) == 2).all() and (idx[:, 2:] == -1).all() and np.isinf(d2[:, 2:]).all()


def test_knn_error_returns(gpu):
    """the C entry points refuse what they cannot run, before any launch"""
    from dust3r_amd._lib import current_stream, lib, ptr
    nr, nq, k = 64, 40, 4
    R, Q = torch.rand((nr, 3), device=gpu), torch.rand((nq, 3), device=gpu)
    work = torch.empty(int(lib.d3r_cloud_grid_workspace_bytes(nr, nq)) + int(lib.d3r_cloud_knn_distances_workspace_bytes(nq)), dtype=torch.uint8, device=gpu)
    d2, idx = torch.empty((nq, 32), device=gpu), torch.empty((nq, 32), dtype=torch.int32, device=gpu)
    mean, count, sums = torch.empty(nq, device=gpu), torch.empty(1, dtype=torch.int64, device=gpu), torch.empty(2, dtype=torch.float64, device=gpu)
    normals, curv, seen = torch.zeros((nq, 3), device=gpu), torch.empty(nq, device=gpu), torch.empty(nq, dtype=torch.int32, device=gpu)
    depth, conf = torch.ones((2, 16), device=gpu), torch.ones((2, 16), device=gpu)
    Ks, Ms, cs = torch.eye(3, device=gpu).repeat(2, 1, 1), torch.eye(4, device=gpu).repeat(2, 1, 1), torch.zeros((2, 3), device=gpu)
    hw = torch.full((2,), 4, dtype=torch.int32, device=gpu)

    def host(ctype, values):
        return None if values is None else (ctype * max(len(values), 1))(*values)

    def knn(lo=(0.0, 0.0, 0.0), cell=0.25, bits=(3, 3, 3), r=0.25, **kw):
        a = dict(dict(nr=nr, nq=nq, q=ptr(Q), k=k, d2=ptr(d2), idx=ptr(idx), work=ptr(work)), **kw)
        return lib.d3r_cloud_knn(a['nr'], a['nq'], a['q'], a['k'], r, host(C.c_float, lo), cell, host(C.c_int, bits), 0, 0, a['d2'], a['idx'], None, a['work'],
                                 current_stream())

    def dist(**kw):
        a = dict(dict(n=nq, k=k, d2=ptr(d2), idx=ptr(idx), mean=ptr(mean), count=ptr(count), sums=ptr(sums), work=ptr(work)), **kw)
        return lib.d3r_cloud_knn_distances(a['n'], a['k'], a['d2'], a['idx'], a['mean'], a['count'], a['sums'], a['work'], current_stream())

    def nrm(**kw):
        a = dict(dict(n=nq, p=ptr(Q), nr=nr, ref=ptr(R), k=k, idx=ptr(idx), m=3, out=ptr(normals), curv=ptr(curv)), **kw)
        return lib.d3r_cloud_normals(a['n'], a['p'], a['nr'], a['ref'], a['k'], a['idx'], a['m'], a['out'], a['curv'], current_stream())

    def orient(**kw):
        a = dict(dict(n=nq, p=ptr(Q), nrm=ptr(normals), seen=ptr(seen), nv=2, depth=ptr(depth), conf=ptr(conf), K=ptr(Ks), M=ptr(Ms), c=ptr(cs), h=ptr(hw),
                      w=ptr(hw), area=16, tol=0.05), **kw)
        return lib.d3r_cloud_orient_normals(a['n'], a['p'], a['nrm'], a['seen'], a['nv'], a['depth'], a['conf'], a['K'], a['M'], a['c'], a['h'], a['w'],
                                            a['area'], a['tol'], current_stream())
    assert lib.d3r_cloud_grid_build(nr, ptr(R), host(C.c_float, (0.0, 0.0, 0.0)), 0.25, host(C.c_int, (3, 3, 3)), ptr(work), current_stream()) == 0
    assert knn() == 0 and dist() == 0 and nrm() == 0 and orient() == 0
    for kw in (dict(k=0), dict(k=33), dict(k=-3), dict(nr=0), dict(nq=0), dict(q=None), dict(d2=None), dict(idx=None), dict(work=None), dict(lo=None),
               dict(bits=None), dict(cell=0.0), dict(cell=float('nan')), dict(bits=(0, 3, 3)), dict(bits=(3, 22, 3)), dict(lo=(0.0, float('nan'), 0.0)),
               dict(r=0.0), dict(r=-0.5), dict(r=float('nan')), dict(r=float('inf')), dict(r=1e-20), dict(r=3e38)):
        assert knn(**kw) == -1, kw
    assert knn(k=1) == 0 and knn(k=32) == 0 and knn() == 0             # the ends of the range of k, then the call checked below
    for kw in (dict(n=0), dict(k=0), dict(k=33), dict(d2=None), dict(idx=None), dict(mean=None), dict(count=None), dict(sums=None), dict(work=None)):
        assert dist(**kw) == -1, kw
    for kw in (dict(n=0), dict(nr=0), dict(k=0), dict(k=33), dict(p=None), dict(ref=None), dict(idx=None), dict(m=1), dict(out=None), dict(curv=None)):
        assert nrm(**kw) == -1, kw
    for kw in (dict(n=0), dict(p=None), dict(nrm=None), dict(seen=None), dict(nv=0), dict(depth=None), dict(conf=None), dict(K=None), dict(M=None),
               dict(c=None), dict(h=None), dict(w=None), dict(area=0), dict(tol=-0.1), dict(tol=1.0), dict(tol=float('nan'))):
        assert orient(**kw) == -1, kw
    torch.cuda.synchronize()
    want = brute_force_knn(Q.cpu().numpy(), R.cpu().numpy(), k, 0.25)  # the good call ran
    assert np.array_equal(idx.cpu().numpy().reshape(-1)[:nq * k].reshape(nq, k), want[1])


# ---- 2. distances and the outlier mask ------------------------------------------------------------------------------------------------
def _noisy_plane(rng, n=3000, noise=0.003):
    P = rng.random((n, 3))
    P[:, 2] = noise * rng.standard_normal(n)
    return P.astype(F32)


def test_mean_distances_and_outlier_mask(gpu):
    """a noisy plane, 1 % scatter hovering 0.05 - 0.12 above it (all k neighbours within max_dist, a large mean) and 1 % far scatter (fewer
    than k neighbours). mean_out bit for bit; the three sums against math.fsum to 1e-12 relative (fp64 sums of fewer than 1e4 positive
    terms differ by at most n eps); the keep mask equal wherever the mean is not within 1e-9 relative of the threshold -- nowhere here."""
    from dust3r_amd.cloud_metrics import k_nearest, knn_mean_distances
    from dust3r_amd.viz import FusedCloud
    rng = np.random.default_rng(31)
    plane = _noisy_plane(rng)
    hover = rng.random((30, 3)) * [1, 1, 0.07] + [0, 0, 0.05]
    far = rng.random((30, 3)) * 3 + [0, 0, 0.5]
    P = np.concatenate([plane, hover.astype(F32), far.astype(F32)])
    k, max_dist, ratio = 16, 0.15, 2.0
    d2, idx = k_nearest(P, P, k, max_dist, exclude_self=True, to_host=False)
    want = brute_force_knn(P, P, k, max_dist, exclude_self=True)
    assert np.array_equal(idx.cpu().numpy(), want[1]) and np.array_equal(d2.cpu().numpy(), want[0])
    runs = [[t.cpu().numpy() for t in knn_mean_distances(d2, idx)] for _ in range(2)]
    for a, b in zip(*runs):
        assert a.tobytes() == b.tobytes()
    mean, count, sums = runs[0]
    want_mean, full = restated_means(*want)
    assert 20 <= (~full).sum() <= 40 and mean.dtype == F32
    assert np.array_equal(mean, want_mean, equal_nan=True)
    m = want_mean[full].astype(np.float64)
    s1, s2 = math.fsum(m), math.fsum(m * m)
    print(f'count {count[0]} / {full.sum()}; sum relative {abs(sums[0] - s1) / s1:.3e}, sum of squares relative {abs(sums[1] - s2) / s2:.3e}')
    assert count[0] == full.sum() and abs(sums[0] - s1) <= 1e-12 * s1 and abs(sums[1] - s2) <= 1e-12 * s2
    threshold = restated_threshold(want_mean[full], ratio)
    with np.errstate(invalid='ignore'):
        want_keep = want_mean.astype(np.float64) <= threshold
        close = np.abs(want_mean.astype(np.float64) - threshold) <= 1e-9 * threshold
    assert not close.any()                                             # no point of this input sits on the threshold
    assert not want_keep[~full].any() and 10 <= (~want_keep[:3000]).sum() + 0 <= 300 and not want_keep[3000:3030].all()
    cloud = FusedCloud(P, np.zeros((len(P), 3), np.uint8), np.ones(len(P), F32), np.ones(len(P), np.int32), 0.02, (P.min(axis=0), P.max(axis=0)))
    kept, keep = cloud.remove_outliers(k=k, std_ratio=ratio, max_dist=max_dist)
    assert keep.dtype == bool and np.array_equal(keep, want_keep)
    assert len(kept) == want_keep.sum() and np.array_equal(kept.positions, P[want_keep]) and kept.normals is None
    dev = FusedCloud(*(torch.from_numpy(a).to(gpu) for a in (P, np.zeros((len(P), 3), np.uint8), np.ones(len(P), F32), np.ones(len(P), np.int32))), 0.02,
                     (P.min(axis=0), P.max(axis=0)))
    kept_dev, keep_dev = dev.remove_outliers(k=k, std_ratio=ratio, max_dist=max_dist)
    assert kept_dev.positions.is_cuda and np.array_equal(keep_dev.cpu().numpy(), want_keep)


# ---- 3. normals -----------------------------------------------------------------------------------------------------------------------
def _sphere(rng, n=3000, noise=0.002):
    P = rng.standard_normal((n, 3))
    P /= np.linalg.norm(P, axis=1, keepdims=True)
    return (P * (1 + noise * rng.standard_normal((n, 1)))).astype(F32)


LONELY = np.array([[50, 0, 0], [0, 50, 0], [0, 0, 50], [80, 80, 80], [80.01, 80, 80], [-90, 0, 0], [-90.01, 0, 0], [-90, 0.01, 0]], F32)


@pytest.mark.parametrize('k', [8, 16])
@pytest.mark.parametrize('shape', ['sphere', 'plane'])
def test_normals(gpu, shape, k):
    """np.linalg.eigh in fp64 on the kernel's own neighbour rows (exact by test 1). After the sign convention every fp32 component within
    2.4e-7 (two units in the last place at 1.0: the fp64 eigenvector error at these gaps is about 1e-12, so only the final rounding is
    left), for the points with (l1 - l0) / l2 >= 1e-3 -- all of them here, asserted; curvature within 1e-6 relative. Eight lonely points
    (0, 0, 1, 1, 2, 2, 2 neighbours ... fewer than 3) get the zero normal and NaN. On the sphere at k = 16 the normal is radial."""
    from dust3r_amd.cloud_metrics import cloud_normals, k_nearest
    rng = np.random.default_rng(41 + k)
    surface, max_dist = (_sphere(rng), 0.5) if shape == 'sphere' else (_noisy_plane(rng), 0.2)
    P = np.concatenate([surface, LONELY])
    d2, idx = k_nearest(P, P, k, max_dist, exclude_self=True, to_host=False)
    Pd = torch.from_numpy(P).to(gpu)
    normals, curv = (t.cpu().numpy() for t in cloud_normals(Pd, Pd, idx))
    again = [t.cpu().numpy() for t in cloud_normals(P, P, idx)]
    assert normals.dtype == F32 and curv.dtype == F32 and normals.tobytes() == again[0].tobytes() and curv.tobytes() == again[1].tobytes()
    want_n, want_c, lam, found = restated_normals(P, P, idx.cpu().numpy())
    few = found < 3
    assert few.sum() == len(LONELY) and few[-len(LONELY):].all() and (found[:3000] == k).all()
    assert (normals[few] == 0).all() and np.isnan(curv[few]).all()
    gap = (lam[~few, 1] - lam[~few, 0]) / lam[~few, 2]
    print(f'{shape} k = {k}: smallest gap ratio {gap.min():.4f}')
    assert (gap >= 1e-3).all()                                         # the bar applies to every point (at most 1 % may fall outside)
    got = lead_positive(normals[~few].astype(np.float64))
    err = np.abs(got - want_n[~few]).max()
    cerr = np.abs(curv[~few].astype(np.float64) / want_c[~few] - 1).max()
    print(f'largest component error {err:.3e} (bar 2.4e-7), largest relative curvature error {cerr:.3e} (bar 1e-6)')
    assert np.array_equal(got, normals[~few].astype(np.float64))       # the kernel's sign already is the convention's
    assert err <= 2.4e-7 and cerr <= 1e-6
    if shape == 'sphere' and k == 16:
        radial = surface.astype(np.float64) / np.linalg.norm(surface.astype(np.float64), axis=1, keepdims=True)
        assert (np.abs((normals[:3000].astype(np.float64) * radial).sum(axis=1)) >= 0.99).all()


# ---- 4. orientation -------------------------------------------------------------------------------------------------------------------
RADIUS = 0.6


def _orientation_scene():
    """four views of 32 x 48 and 48 x 32 around a sphere of radius 0.6 at the origin: the cameras of synthetic_scene (a circle of radius 2,
    looking at the origin), focal 1.2 W, the depth of the sphere by ray intersection, 1000 where the ray misses; random confidences"""
    from dust3r_amd.synthetic import synthetic_scene
    _, _, gt = synthetic_scene(4, 32, 48, seed=0)
    c2w = gt['cam2world'].numpy().astype(np.float64)
    shapes = [(32, 48), (48, 32), (32, 48), (48, 32)]
    rng = np.random.default_rng(51)
    depth, conf, K = [], [], []
    for (h, w), T in zip(shapes, c2w):
        f = 1.2 * w
        vs, us = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing='ij')
        rays = np.stack(((us - w / 2) / f, (vs - h / 2) / f, np.ones_like(us)), axis=-1) @ T[:3, :3].T
        c = T[:3, 3]
        a, b, cc = (rays * rays).sum(-1), 2 * (rays @ c), c @ c - RADIUS ** 2
        disc = b * b - 4 * a * cc
        t = np.where(disc > 0, (-b - np.sqrt(np.maximum(disc, 0))) / (2 * a), 1000.0)
        depth.append(t.astype(F32))
        conf.append((1 + 2 * rng.random((h, w))).astype(F32))
        K.append(np.array([[f, 0, w / 2], [0, f, h / 2], [0, 0, 1]], F32))
    return shapes, c2w.astype(F32), depth, conf, np.stack(K)


def test_orientation(gpu):
    """n_seen exactly the restatement's (fp32 projection in the kernel's operation order); the sign the restated fp64 vote's wherever
    |s| >= 1e-9 sum w (everywhere here, asserted: at most 1 % may be left out); a seen point faces at least one camera that sees it; points
    inside the sphere and beside every view are seen by none and take the all-cameras vote."""
    from dust3r_amd.cloud_metrics import orient_normals
    from dust3r_amd.utils.padded import pad_views, shape_tables
    shapes, c2w, depth, conf, K = _orientation_scene()
    rng = np.random.default_rng(52)
    S = rng.standard_normal((2500, 3))
    S /= np.linalg.norm(S, axis=1, keepdims=True)
    surface = S * RADIUS * (1 + 0.001 * rng.standard_normal((2500, 1)))
    inside = rng.standard_normal((40, 3)) * 0.05                       # behind the surface for every camera
    beside = np.array([0, 5, 0]) + rng.standard_normal((40, 3)) * 0.2  # above every view's field
    P = np.concatenate([surface, inside, beside]).astype(F32)
    N = np.concatenate([S * rng.choice([-1.0, 1.0], size=(2500, 1)), rng.standard_normal((80, 3))])
    N = (N / np.linalg.norm(N, axis=1, keepdims=True)).astype(F32)
    row = 1600                                                         # 64 elements of padding behind every view, poisoned
    dstack, cstack = (pad_views(maps, gpu, torch.float32, (), row) for maps in (depth, conf))
    dstack[:, 1536:], cstack[:, 1536:] = float('nan'), float('nan')
    hs, ws, _ = shape_tables(shapes, gpu)
    # the wrapper inverts cam2world itself (torch, fp32): the restatement takes the matrices the kernel was given
    from dust3r_amd.utils.geometry import inv
    w2c = inv(torch.from_numpy(c2w).to(gpu)).cpu().numpy()
    n_seen, s, sum_w, seen, cosines = restated_orientation(P, N, depth, conf, K, w2c, c2w[:, :3, 3], shapes, 0.05)
    assert (n_seen[:2500] > 0).sum() > 1500 and (n_seen[:2500] > 1).sum() > 200 and (n_seen[2500:] == 0).all()
    decided = np.abs(s) >= 1e-9 * sum_w
    assert (~decided).sum() <= 0.01 * len(P) and (s[decided] < 0).sum() > 500
    runs = []
    for _ in range(2):
        Nd = torch.from_numpy(N).to(gpu)
        got_seen = orient_normals(torch.from_numpy(P).to(gpu), Nd, dstack, cstack, torch.from_numpy(K).to(gpu), torch.from_numpy(c2w).to(gpu), hs, ws, tol=0.05)
        runs.append((Nd.cpu().numpy(), got_seen.cpu().numpy()))
    assert runs[0][0].tobytes() == runs[1][0].tobytes() and runs[0][1].tobytes() == runs[1][1].tobytes()
    out, got_seen = runs[0]
    assert got_seen.dtype == np.int32 and np.array_equal(got_seen, n_seen)
    flipped = (out != N).any(axis=1)
    assert np.array_equal(out, np.where(flipped[:, None], -N, N))      # a normal is kept or negated, nothing else
    assert np.array_equal(flipped[decided], s[decided] < 0)
    facing = ((np.where(flipped[:, None], -cosines, cosines) >= 0) & seen).any(axis=1)
    assert facing[n_seen > 0].all()
    unseen = n_seen == 0                                               # the fallback: the unweighted sum over all cameras
    assert unseen.sum() >= 80 and np.array_equal(flipped[unseen & decided], cosines[unseen & decided].sum(axis=1) < 0)
    assert 0 < flipped[unseen].sum() < unseen.sum()


# ---- 5. through the API ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def scene(gpu):
    from test_fuse_gpu import _scene
    return _scene(gpu, 4, 32, 48, 3)


def test_scene_fuse_defaults_are_untouched_and_the_new_arguments_work(gpu, scene):
    from dust3r_amd.viz import FusedCloud
    a, b = scene.fuse(), scene.fuse()
    assert a.normals is None and a.curvature is None and len(a) > 300
    for name in ('positions', 'colors', 'weight', 'count'):
        assert getattr(a, name).tobytes() == getattr(b, name).tobytes()
    cloud = scene.fuse(normals=True, outliers=2.0)
    assert isinstance(cloud, FusedCloud) and 0 < len(cloud) <= len(a)
    assert cloud.normals.shape == (len(cloud), 3) and cloud.normals.dtype == F32 and cloud.curvature.shape == (len(cloud),)
    norm = np.linalg.norm(cloud.normals.astype(np.float64), axis=1)
    zero = (cloud.normals == 0).all(axis=1)
    assert (np.abs(norm[~zero] - 1) <= 1e-6).all() and (~zero).sum() > 0.9 * len(cloud) and np.isnan(cloud.curvature[zero]).all()
    kept, keep = a.remove_outliers(k=16, std_ratio=2.0)                # the same two steps by hand
    assert np.array_equal(cloud.positions, kept.positions) and keep.sum() == len(cloud)
    by_hand = kept.estimate_normals(k=16, scene=scene)
    assert by_hand.normals.tobytes() == cloud.normals.tobytes()
    unoriented = kept.estimate_normals(k=16)                           # no scene: the sign convention; the cameras turn some of them
    lead = np.take_along_axis(unoriented.normals, np.abs(unoriented.normals).argmax(axis=1)[:, None], axis=1)[:, 0]
    assert (lead[~zero] > 0).all() and np.array_equal(np.abs(unoriented.normals), np.abs(cloud.normals))
    turned = (unoriented.normals != cloud.normals).any(axis=1)
    assert 0 < turned.sum() < len(cloud)
    dev = scene.fuse(normals=True, to_host=False)
    assert dev.normals.is_cuda and dev.positions.is_cuda and len(dev) == len(a)


def test_command_line_writes_normals(gpu, scene, tmp_path):
    """--fuse_normals --ply through the demo's main (in this process: the child-process run of the command line is tests/test_fuse_gpu.py's)
    on the random-weight checkpoint and the three pictures of that test, whose cloud is empty: the PLY carries the normal properties; then the demo's writer on a
    scene with points, where read_ply returns unit normals."""
    import argparse
    from dust3r_amd import demo
    from dust3r_amd.export import read_ply
    from dust3r_amd.synthetic import MODEL_CONFIGS
    from oracle.dust3r_ref import build_ref_model
    from test_fuse_gpu import _write_images
    cfg = MODEL_CONFIGS['tiny_dpt']
    state = {k: v for k, v in build_ref_model('tiny_dpt').state_dict().items() if not k.startswith('dec_blocks2')}
    model_str = ("AsymmetricCroCo3DStereo(pos_embed='RoPE100', patch_embed_cls='ManyAR_PatchEmbed', img_size=(64, 64), head_type='dpt', output_mode='pts3d', "
                 "depth_mode=('exp', -inf, inf), conf_mode=('exp', 1, inf), enc_embed_dim=%d, enc_depth=%d, enc_num_heads=%d, dec_embed_dim=%d, dec_depth=%d, dec_num_heads=%d)"
                 % (cfg['enc_embed_dim'], cfg['enc_depth'], cfg['enc_num_heads'], cfg['dec_embed_dim'], cfg['dec_depth'], cfg['dec_num_heads']))
    ckpt = str(tmp_path / 'tiny_dpt.pth')
    torch.save({'args': argparse.Namespace(model=model_str), 'model': state}, ckpt)
    pics = tmp_path / 'pics'
    pics.mkdir()
    _write_images(pics, [(80, 60), (60, 80), (80, 60)])
    out = tmp_path / 'out'
    assert demo.main([str(pics), '--weights', ckpt, '--image_size', '224', '--niter', '5', '--min_conf_thr', '1.0', '--silent', '--outdir', str(out),
                      '--fuse_normals', '--ply']) == 0
    cloud = read_ply(str(out / 'scene.ply'))
    assert sorted(cloud) == ['colors', 'confidence', 'count', 'normals', 'positions'] and cloud['normals'].shape == cloud['positions'].shape
    import copy
    written = demo.write_fused(str(tmp_path), copy.deepcopy(scene), min_conf_thr=1.0, normals=True, outliers=2.0)
    cloud = read_ply(written[0])
    norm = np.linalg.norm(cloud['normals'].astype(np.float64), axis=1)
    assert len(norm) > 300 and (np.abs(norm[norm > 0] - 1) <= 1e-6).all() and (norm > 0).mean() > 0.9


# ---- 6. the resource report -----------------------------------------------------------------------------------------------------------
def test_resource_report_has_no_scratch():
    """read only: the report is what the build left next to the object; nothing is built or touched here"""
    from dust3r_amd import _lib
    path = os.path.join(os.path.dirname(_lib.LIB_PATH), 'cloud_knn.resources.txt')
    if not os.path.exists(path):
        pytest.skip('no cloud_knn.resources.txt: the library was not built by dust3r_amd/build.py')
    report = open(path).read()
    kernels = re.findall(r'Function Name: (\S+)', report)
    new = [k for k in kernels if 'cloud_' in k]
    assert len(new) == 10 and sum('cloud_knn_kernel' in k for k in new) == 4 and sum('cloud_sums_final_kernel' in k for k in new) == 1 and all('cloud_' in k or 'fuse_' in k for k in kernels)
    assert re.findall(r'ScratchSize \[bytes/lane\]: (\d+)', report) == ['0'] * len(kernels)
