"""GPU tests of visual localization (csrc/visloc.hip, dust3r_amd.visloc): batched matching against this package's find_reciprocal_matches,
PnP-RANSAC on synthetic problems against ground truth and an fp64 Levenberg-Marquardt written here, undistortion, batch determinism,
and `localize` end to end on exact geometry and on the engine against a step-by-step restatement of visloc.py's loop."""
import numpy as np
import pytest
import torch

from test_visloc_cpu import CX, CY, FX, FY, IMG_H, IMG_W, K, pnp_abi

pytestmark = pytest.mark.gpu


def _problem(n, outliers, noise, seed):
    from dust3r_amd.synthetic import pnp_problem
    return pnp_problem(n, outliers, noise, seed, K=K, size=(IMG_W, IMG_H))


def _lm_reference(uv, X, w2c0, iters=50):
    """fp64 Gauss-Newton / LM on the reprojection error (rotation vector about the camera frame + translation), from w2c0"""
    R, t = w2c0[:3, :3].copy(), w2c0[:3, 3].copy()
    X = X.astype(np.float64)
    uv = uv.astype(np.float64)
    lam = 1e-3

    def cost(R, t):
        Y = X @ R.T + t
        r = np.c_[FX * Y[:, 0] / Y[:, 2] + CX - uv[:, 0], FY * Y[:, 1] / Y[:, 2] + CY - uv[:, 1]]
        return (r ** 2).sum(), Y, r

    c, Y, r = cost(R, t)
    for _ in range(iters):
        x, y, z = Y.T
        Ju = np.stack([FX * -x * y / z ** 2, FX * (z ** 2 + x * x) / z ** 2, -FX * y / z, FX / z, 0 * z, -FX * x / z ** 2], 1)
        Jv = np.stack([-FY * (z ** 2 + y * y) / z ** 2, FY * x * y / z ** 2, FY * x / z, 0 * z, FY / z, -FY * y / z ** 2], 1)
        A = Ju.T @ Ju + Jv.T @ Jv
        g = Ju.T @ r[:, 0] + Jv.T @ r[:, 1]
        d = np.linalg.solve(A + lam * np.diag(np.diag(A)), -g)
        w = d[:3]
        th = np.linalg.norm(w)
        Kx = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
        E = np.eye(3) + (np.sin(th) / th if th > 0 else 1) * Kx + ((1 - np.cos(th)) / th ** 2 if th > 0 else 0.5) * Kx @ Kx
        R2, t2 = E @ R, E @ t + d[3:]
        c2, Y2, r2 = cost(R2, t2)
        if c2 < c:
            R, t, c, Y, r, lam = R2, t2, c2, Y2, r2, lam * 0.1
        else:
            lam *= 10
    out = np.eye(4)
    out[:3, :3], out[:3, 3] = R, t
    return out


# ---- matching ------------------------------------------------------------------------------------------------------------------------
def _expected_matches(pq, cq, pm, cm, vm, thr):
    from dust3r_amd.utils.geometry import find_reciprocal_matches
    mq = (cq >= thr).reshape(-1)
    mm = (cm >= thr).reshape(-1) & (vm.reshape(-1) if vm is not None else True)
    PQ, PM = pq.reshape(-1, 3)[mq], pm.reshape(-1, 3)[mm]
    if len(PQ) == 0 or len(PM) == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    recip, nn2, _ = find_reciprocal_matches(PQ, PM)
    iq, im = torch.nonzero(mq)[:, 0], torch.nonzero(mm)[:, 0]
    return iq[nn2][recip].cpu().numpy(), im[recip].cpu().numpy()


def test_match_pairs_equals_find_reciprocal_matches(gpu):
    from dust3r_amd.visloc import match_pairs
    g = torch.Generator(device='cpu').manual_seed(0)
    shapes = [(32, 48), (48, 32), (24, 40), (64, 64), (16, 16), (40, 24)]
    thr = 1.5
    pairs = []
    for k in range(44):
        (h0, w0), (h1, w1) = shapes[k % 6], shapes[(3 * k + 1) % 6]
        pq = torch.randn((h0, w0, 3), generator=g)
        pm = torch.randn((h1, w1, 3), generator=g)
        if k % 4 == 1:                                            # coarse grid: exact distance ties between distinct points
            pq, pm = (pq * 2).round() / 2, (pm * 2).round() / 2
        if k % 4 == 2:                                            # the map is the query, shifted a little: many mutual pairs
            pm = pq[:h1, :w1] + 0.01 * torch.randn(pq[:h1, :w1].shape, generator=g) if (h1 <= h0 and w1 <= w0) else pm
            pm = pm.contiguous()
            h1, w1 = pm.shape[:2]
        cq = 1 + torch.exp(torch.randn((h0, w0), generator=g))
        cm = 1 + torch.exp(torch.randn((h1, w1), generator=g))
        vm = torch.rand((h1, w1), generator=g) < 0.8
        if k == 5:
            cq[:] = 1.0                                           # empty query side
        if k == 6:
            vm[:] = False                                         # empty map side
        pairs.append((pq, cq, pm, cm, None if k % 7 == 3 else vm))
    pairs.append((torch.randn((384, 512, 3), generator=g), 1 + torch.exp(torch.randn((384, 512), generator=g)),
                  torch.randn((384, 512, 3), generator=g), 1 + torch.exp(torch.randn((384, 512), generator=g)), None))
    got = match_pairs([tuple(None if t is None else t.to(gpu) for t in p) for p in pairs], thr, gpu)
    assert len(got) == len(pairs)
    total = 0
    for k, ((pq, cq, pm, cm, vm), (gq, gm)) in enumerate(zip(pairs, got)):
        eq, em = _expected_matches(pq.to(gpu), cq.to(gpu), pm.to(gpu), cm.to(gpu), None if vm is None else vm.to(gpu), thr)
        assert np.array_equal(gq.cpu().numpy(), eq) and np.array_equal(gm.cpu().numpy(), em), k
        total += len(eq)
    assert len(got[5][0]) == 0 and len(got[6][0]) == 0 and total > 1000


# ---- PnP-RANSAC ------------------------------------------------------------------------------------------------------------------------
def _pose_err(c2w, w2c):
    return np.abs(np.linalg.inv(c2w)[:3, :] - w2c[:3, :]).max()


PNP_CASES = [(n, o, s) for n in (2000, 100_000) for o in (0.0, 0.3, 0.6) for s in (0.0, 0.5)] + [(6, 0.0, 0.0), (6, 0.0, 0.5)]


@pytest.mark.parametrize('n,outliers,noise', PNP_CASES)
def test_pnp_synthetic(gpu, n, outliers, noise):
    from dust3r_amd.visloc.localization import run_pnp_batch
    uv, X, w2c, inl = _problem(n, outliers, noise, seed=n + int(10 * outliers) + int(100 * noise))
    ok, c2w, mask = run_pnp_batch([(uv, X, K, None, 5.0)], device=gpu, return_inliers=True)[0]
    assert ok
    assert np.array_equal(mask, inl)
    if noise == 0:
        assert _pose_err(c2w, w2c) < 1e-6
    else:
        ref = _lm_reference(uv[inl], X[inl], w2c)
        assert _pose_err(c2w, ref) < 1e-5


def test_pnp_failures(gpu):
    from dust3r_amd.visloc import run_pnp
    from dust3r_amd.visloc.localization import run_pnp_batch
    uv, X, _, _ = _problem(6, 0.0, 0.0, seed=1)
    assert run_pnp(uv[:4], X[:4], K) == (False, None)
    assert run_pnp(uv[:3], X[:3], K) == (False, None)
    rng = np.random.RandomState(2)
    jobs = []
    for n in (8, 30):                                             # pure outliers: no hypothesis beyond its sample
        jobs.append((np.c_[rng.uniform(0, IMG_W, n), rng.uniform(0, IMG_H, n)].astype(np.float32), rng.normal(size=(n, 3)).astype(np.float32) + [0, 0, 5],
                     K, None, 5.0))
    for ok, pose in run_pnp_batch(jobs, device=gpu):
        assert ok is False and pose is None


def _distort(uv, dist):
    k1, k2, p1, p2 = dist
    x, y = (uv[:, 0] - CX) / FX, (uv[:, 1] - CY) / FY
    r2 = x * x + y * y
    rad = 1 + k1 * r2 + k2 * r2 * r2
    xd = x * rad + 2 * p1 * x * y + p2 * (r2 + 2 * x * x)
    yd = y * rad + p1 * (r2 + 2 * y * y) + 2 * p2 * x * y
    return np.c_[FX * xd + CX, FY * yd + CY]


def test_pnp_distortion(gpu):
    from dust3r_amd.visloc import run_pnp
    uv, X, w2c, _ = _problem(2000, 0.0, 0.0, seed=7)
    dist = [-0.08, 0.02, 0.0015, -0.001]
    ok0, c2w0 = run_pnp(uv, X, K, None)
    ok1, c2w1 = run_pnp(_distort(uv.astype(np.float64), dist).astype(np.float32), X, K, dist)
    assert ok0 and ok1
    assert np.abs(c2w1 - c2w0).max() < 1e-5 and _pose_err(c2w1, w2c) < 1e-5


def test_pnp_batch_is_bit_identical_to_single_jobs(gpu):
    from dust3r_amd.visloc.localization import run_pnp_batch
    rng = np.random.RandomState(11)
    jobs = []
    for k in range(50):
        n = int(rng.choice([6, 50, 700, 5000]))
        uv, X, _, _ = _problem(n, 0.0 if n == 6 else float(rng.choice([0.0, 0.3, 0.6])), float(rng.choice([0.0, 0.5])), seed=100 + k)
        jobs.append((uv, X, K, None, float(rng.choice([3.0, 5.0]))))
    batch = run_pnp_batch(jobs, device=gpu, return_inliers=True)
    again = run_pnp_batch(jobs, device=gpu, return_inliers=True)
    for k, job in enumerate(jobs):
        alone = run_pnp_batch([job], device=gpu, return_inliers=True)[0]
        for other in (alone, again[k]):
            assert batch[k][0] == other[0]
            assert np.array_equal(batch[k][1], other[1]) and np.array_equal(batch[k][2], other[2]), k
    assert sum(r[0] for r in batch) == 50


# ---- localize ----------------------------------------------------------------------------------------------------------------------------
class _Picture:
    def __init__(self, W, H):
        self.size = (W, H)


def test_localize_exact_geometry(gpu):
    """Query and map views from synthetic_scene's cameras, focal and depth: the query's pointmap is its camera-frame surface; each map
    view holds a shuffled subset of the same surface (world points in pts3d_rescaled, query-frame points as the prediction) plus far
    clutter. localize on that exact `output` recovers the query cameras."""
    from dust3r_amd.synthetic import synthetic_scene
    from dust3r_amd.visloc import get_pose_error, localize
    H, W = 48, 64
    _, _, gt = synthetic_scene(4, H, W, seed=3, noise=0.0)
    c2w, depth, f = gt['cam2world'].double().numpy(), gt['depth'].double().numpy(), gt['focal']
    vs, us = np.meshgrid(np.arange(H), np.arange(W), indexing='ij')
    rng = np.random.RandomState(0)
    queries, p1, c1, p2, c2 = [], [], [], [], []
    for qi in (0, 2):
        cam = np.stack(((us - W / 2) / f * depth[qi], (vs - H / 2) / f * depth[qi], depth[qi]), -1)          # query camera frame
        query = dict(rgb_rescaled=torch.zeros(3, H, W), to_orig=np.diag([2.0, 2.0, 1.0]), rgb=_Picture(2 * W, 2 * H), distortion=None,
                     intrinsics=np.array([[2 * f, 0, W + 0.5], [0, 2 * f, H + 0.5], [0, 0, 1]]))      # the original image is twice as large
        views = [query]
        for m in range(2):
            src = rng.permutation(H * W).reshape(H, W)
            clutter = rng.rand(H, W) < 0.4
            qf = np.where(clutter[..., None], rng.normal(size=(H, W, 3)) + [0, 0, 50], cam.reshape(-1, 3)[src])
            wf = qf @ c2w[qi, :3, :3].T + c2w[qi, :3, 3]
            views.append(dict(rgb_rescaled=torch.zeros(3, H, W), pts3d_rescaled=torch.from_numpy(wf.astype(np.float32)),
                              valid_rescaled=torch.from_numpy(rng.rand(H, W) < 0.9)))
            p1.append(torch.from_numpy(cam.astype(np.float32)))
            c1.append(torch.full((H, W), 5.0))
            p2.append(torch.from_numpy(qf.astype(np.float32)))
            c2.append(torch.full((H, W), 5.0))
        queries.append(views)
    output = dict(pred1=dict(pts3d=torch.stack(p1), conf=torch.stack(c1)), pred2=dict(pts3d_in_other_view=torch.stack(p2), conf=torch.stack(c2)))
    results, counts = localize(queries, None, gpu, conf_thr=3.0, output=output)
    results1, counts1 = localize(queries, None, gpu, conf_thr=3.0, output=output, max_pairs_per_call=1)      # one query per chunk
    assert counts1 == counts and all(a[0] == b[0] and np.array_equal(a[1], b[1]) for a, b in zip(results, results1))
    for (ok, pose), qi, cnt in zip(results, (0, 2), counts):
        assert ok and min(cnt) > 0.4 * H * W
        assert np.abs(pose - c2w[qi]).max() < 1e-4
        t_err, r_err = get_pose_error(pose, c2w[qi])
        assert float(t_err) < 1e-4 and float(r_err) < 1e-3


def test_localize_equals_visloc_loop_on_the_engine(gpu):
    """localize() against visloc.py:72-165 restated step by step from this package's inference, find_reciprocal_matches, xy_grid, geotrf
    and run_pnp (one inference per pair, host masks and gathers), with the same subsample seed: bit-identical poses and match counts."""
    from dust3r_amd.inference import inference
    from dust3r_amd.model import AsymmetricCroCo3DStereo
    from dust3r_amd.synthetic import MODEL_CONFIGS
    from dust3r_amd.utils.geometry import find_reciprocal_matches, geotrf, xy_grid
    from dust3r_amd.visloc import localize, run_pnp, subsample_indices
    from oracle.dust3r_ref import build_ref_model
    m = AsymmetricCroCo3DStereo(landscape_only=False, **MODEL_CONFIGS['tiny_dpt'])
    m.load_state_dict(build_ref_model('tiny_dpt').state_dict())
    model = m.to(gpu)
    H, W = 32, 48
    g = torch.Generator(device='cpu').manual_seed(5)
    rng = np.random.RandomState(5)
    queries = []
    for q in range(3):
        query = dict(rgb_rescaled=torch.rand((3, H, W), generator=g) * 2 - 1, to_orig=np.array([[1.5, 0, 0.25], [0, 1.5, -0.5], [0, 0, 1]]),
                     rgb=_Picture(72, 48), intrinsics=np.array([[60.0, 0, 36.0], [0, 55.0, 24.0], [0, 0, 1]]),
                     distortion=[0.01, -0.002, 0.0, 0.0] if q == 1 else None)
        views = [query]
        for _ in range(2):
            views.append(dict(rgb_rescaled=torch.rand((3, H, W), generator=g) * 2 - 1, pts3d_rescaled=torch.randn((H, W, 3), generator=g),
                              valid_rescaled=torch.from_numpy(rng.rand(H, W) < 0.85)))
        queries.append(views)
    conf_thr, max_points, seed = 1.2, 600, 9
    results, counts = localize(queries, model, gpu, conf_thr=conf_thr, pnp_max_points=max_points, seed=seed, reprojection_error=8.0)
    for chunk in (1, 4):                  # one query per chunk, two queries per chunk: the same bits
        r2, c2 = localize(queries, model, gpu, conf_thr=conf_thr, pnp_max_points=max_points, seed=seed, reprojection_error=8.0,
                          max_pairs_per_call=chunk)
        assert c2 == counts
        assert all(a[0] == b[0] and ((a[1] is None and b[1] is None) or np.array_equal(a[1], b[1])) for a, b in zip(results, r2))
    for q, views in enumerate(queries):
        query_view = views[0]
        q2d, q3d, cnts = [], [], []
        for map_view in views[1:]:
            imgs = []
            for idx, img in enumerate([query_view['rgb_rescaled'], map_view['rgb_rescaled']]):
                imgs.append(dict(img=img.unsqueeze(0), true_shape=np.int32([img.shape[1:]]), idx=idx, instance=str(idx)))
            output = inference([tuple(imgs)], model, gpu, batch_size=1, verbose=False)
            pred1, pred2 = output['pred1'], output['pred2']
            masks = [pred1['conf'].squeeze(0) >= conf_thr, (pred2['conf'].squeeze(0) >= conf_thr) & map_view['valid_rescaled']]
            pts3d = [pred1['pts3d'].squeeze(0), pred2['pts3d_in_other_view'].squeeze(0)]
            p2l, p3l = [], []
            for i in range(2):
                conf_i = masks[i].cpu().numpy()
                ts = imgs[i]['true_shape'][0]
                p2l.append(xy_grid(ts[1], ts[0])[conf_i])
                p3l.append(pts3d[i].detach().cpu().numpy()[conf_i])
            PQ, PM = p3l
            if len(PQ) == 0 or len(PM) == 0:
                cnts.append(0)
                continue
            recip, nnM, num = find_reciprocal_matches(PQ, PM)
            cnts.append(num)
            m1 = p2l[1][recip]
            m0 = p2l[0][nnM][recip].astype(np.float64) + 0.5
            m0 = geotrf(query_view['to_orig'], m0, norm=True) - 0.5
            v3 = map_view['pts3d_rescaled'][m1[:, 1], m1[:, 0]]
            if len(v3):
                q3d.append(v3.cpu().numpy())
                q2d.append(m0)
        assert cnts == counts[q]
        p2 = np.concatenate(q2d).astype(np.float32)
        p3 = np.concatenate(q3d)
        if len(p2) > max_points:
            idx = subsample_indices(len(p2), max_points, seed, q)
            p2, p3 = p2[idx], p3[idx]
        ok, pose = run_pnp(p2, p3, query_view['intrinsics'], query_view['distortion'], 'cv2', 8.0, img_size=[72, 48], seed=seed)
        assert results[q][0] == ok
        assert (pose is None and results[q][1] is None) or np.array_equal(pose, results[q][1])
    assert sum(sum(c) for c in counts) > 0


# ---- kernel-level failure paths, stopping and tie rules, call splitting, padding ---------------------------------------------------------
def _pnp_abi(jobs, gpu, max_iters=10_000):
    """d3r_pnp_ransac straight through the C ABI (test_visloc_cpu.pnp_abi, shared with test_visloc_ransac_gpu.py):
    [(status, inliers, drawn, best index)]"""
    return pnp_abi(jobs, gpu, max_iters)[0]


def test_pnp_kernel_failures_stopping_and_ties(gpu):
    uv, X, _, _ = _problem(2000, 0.0, 0.0, seed=21)
    uv6, X6, _, _ = _problem(2000, 0.6, 0.5, seed=22)
    rng = np.random.RandomState(23)
    junk = (np.c_[rng.uniform(0, IMG_W, 8), rng.uniform(0, IMG_H, 8)], rng.normal(size=(8, 3)) + [0, 0, 5])
    out = _pnp_abi([(uv[:4], X[:4]), (uv[:3], X[:3]), junk, (uv, X), (uv6, X6)], gpu)
    assert out[0] == (0, 0, 0, -1) and out[1] == (0, 0, 0, -1)       # n <= 4: failure in the kernel, nothing drawn
    assert out[2][0] == 0 and out[2][2] >= 128                         # pure outliers: no hypothesis beyond its sample
    # noiseless, no outliers: every valid hypothesis of the first round has full support, so the tie goes to the lowest index and the
    # stopping rule (budget 0 once the support is n) ends the job after one round of 128
    assert out[3] == (1, 2000, 128, 0)
    # 60 % outliers: RANSACUpdateNumIters at confidence 0.9999 asks for ~355 hypotheses; the job stops well before its 10 000 budget
    assert out[4][0] == 1 and 128 <= out[4][2] <= 1024 and out[4][3] >= 0


def test_calls_split_above_the_launch_limit(gpu, monkeypatch):
    """match_pairs / run_pnp_batch split lists longer than MAX_CALL into several calls with the same results"""
    from dust3r_amd.visloc import localization as L
    g = torch.Generator(device='cpu').manual_seed(3)
    pairs = [(torch.randn((8, 12, 3), generator=g), 1 + torch.exp(torch.randn((8, 12), generator=g)), torch.randn((12, 8, 3), generator=g),
              1 + torch.exp(torch.randn((12, 8), generator=g)), None) for _ in range(20)]
    jobs = [(*_problem(300, 0.3, 0.5, seed=40 + k)[:2], K, None, 5.0) for k in range(9)]
    whole_m, whole_p = L.match_pairs(pairs, 1.5, gpu), L.run_pnp_batch(jobs, device=gpu)
    monkeypatch.setattr(L, 'MAX_CALL', 4)
    split_m, split_p = L.match_pairs(pairs, 1.5, gpu), L.run_pnp_batch(jobs, device=gpu)
    assert all(torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) for a, b in zip(whole_m, split_m)) and len(split_m) == 20
    assert all(a[0] == b[0] and np.array_equal(a[1], b[1]) for a, b in zip(whole_p, split_p)) and len(split_p) == 9


def test_match_pairs_never_returns_a_padding_slot(gpu):
    """every real distance overflows to inf, while a point at the old tail padding (3e18) would be at ~1.5e38: no candidate beats the
    initial best, so each point keeps index 0 of the other side -- never a slot past the side's count (1 000 and 1 500 points:
    partial LDS tiles on both sides)"""
    from dust3r_amd.visloc import match_pairs
    pq = torch.full((20, 50, 3), 1e19, device=gpu)
    pm = torch.full((30, 50, 3), -1e19, device=gpu)
    one = torch.full((20, 50), 5.0, device=gpu)
    (q, m), = match_pairs([(pq, one, pm, torch.full((30, 50), 5.0, device=gpu), None)], 3.0, gpu)
    assert q.tolist() == [0] and m.tolist() == [0]
