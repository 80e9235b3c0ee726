"""GPU tests of the scene-bootstrap kernels (csrc/bootstrap.hip) at kernel level: the nine C entry points are called directly
(dust3r_amd._lib.lib) on tensors built here and compared with plain fp64 restatements of the header comments in
include/dust3r_hip.h. Every bound is derived from the arithmetic the header promises (fp32 per point, fp64 across points), never from
what the kernels return; the derivations stand next to the assertions.

Layout rules of the module: every array is its own torch allocation (so every pointer is 16-byte aligned), sub-rows start at multiples of
4 floats, and whatever is allocated past the valid length -- row padding up to `ld`, point slots from n up to round_up(n, 4) + 4 -- holds
NaN, so that a kernel reading one slot too far fails loudly. Nothing here passes a misaligned or out-of-range pointer to a kernel.

The input builders and references are numpy / torch on the CPU (`check_input_conditions` evaluates every condition the tests put on
their inputs without a GPU; tests/test_bootstrap_cpu.py runs it)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

U = 2.0 ** -24                 # unit roundoff of fp32
ERR_INVALID = -1               # D3R_ERR_INVALID


def round_up(n, m):
    return (n + m - 1) // m * m


def dev(gpu, a, slots=0):
    """`a` in an allocation of its own of max(slots, a.size) elements; what lies past the data holds NaN (floats) / -1 (integers)."""
    flat = torch.from_numpy(np.ascontiguousarray(a).reshape(-1))
    t = torch.empty(max(slots, flat.numel()), dtype=flat.dtype, device=gpu)
    t.fill_(float('nan') if t.dtype.is_floating_point else -1)
    t[:flat.numel()] = flat.to(gpu)
    assert t.data_ptr() % 16 == 0
    return t


def dev_points(gpu, pts):
    """(n, 3) cloud with NaN point slots from n up to round_up(n, 4) + 4."""
    return dev(gpu, pts, (round_up(len(pts), 4) + 4) * 3)


def dev_scalars(gpu, w):
    return dev(gpu, w, round_up(len(w), 4) + 4)


def table(gpu, tensors):
    return torch.tensor([t.data_ptr() for t in tensors], dtype=torch.int64).to(gpu)


def call(gpu, fn, *args):
    from dust3r_amd._lib import current_stream
    with torch.cuda.device(gpu):
        return fn(*args, current_stream())


def P(t):
    return C.c_void_p(t.data_ptr())


def bits(t):
    return t.cpu().contiguous().view(torch.int64 if t.element_size() == 8 else torch.int32)


# ------------------------------------------------------------------------------------------------------------ 1. d3r_row_means
ROW_COLS = [1, 3, 4, 7, 1023, 1024, 1025, 1027, 2050]


def row_means_case(cols):
    """5 rows of confidence-like values (1 ... 50), row stride round_up(cols, 4) + 4 with NaN padding."""
    rng = np.random.RandomState(100 + cols)
    ld = round_up(cols, 4) + 4
    x = np.full((5, ld), np.nan, np.float32)
    x[:, :cols] = rng.uniform(1, 50, (5, cols)).astype(np.float32)
    return x, ld


@pytest.mark.parametrize('cols', ROW_COLS)
def test_row_means_ragged_columns(gpu, cols):
    """The float4 body, the `c + 4 > cols` tail and more than one trip of the 1024-column stride against the fp64 mean.
    Bound: four fp32 values are added pairwise (2 roundings), everything else accumulates in fp64, the mean is rounded to fp32 once:
    |got - ref| <= 3 * 2^-24 * mean|x| (+ fp64 dust); asserted at 4 * 2^-24 * mean|x|."""
    from dust3r_amd._lib import lib
    x, ld = row_means_case(cols)
    xd = dev(gpu, x)
    out = dev(gpu, np.full(5 + 1, np.nan, np.float32))
    assert call(gpu, lib.d3r_row_means, P(xd), 5, cols, ld, P(out)) == 0
    got = out.cpu().double().numpy()
    ref = x[:, :cols].astype(np.float64).mean(axis=1)
    bound = 4 * U * np.abs(x[:, :cols].astype(np.float64)).mean(axis=1)
    print(f'row_means cols={cols}: max err {np.abs(got[:5] - ref).max():.3e}, bound {bound.min():.3e}')
    assert (np.abs(got[:5] - ref) <= bound).all(), (got[:5], ref)
    assert np.isnan(got[5])                                             # one mean per row, nothing past them


def test_row_means_rejects_bad_layout(gpu):
    """D3R_ERR_INVALID, nothing launched: a row stride that is no multiple of 4 floats or shorter than the row, and an x that is not
    16-byte aligned (the kernel loads float4: include/dust3r_hip.h)."""
    from dust3r_amd._lib import lib
    xd = dev(gpu, np.ones(64, np.float32))
    out = dev(gpu, np.full(4, np.nan, np.float32))
    assert call(gpu, lib.d3r_row_means, P(xd), 2, 7, 9, P(out)) == ERR_INVALID          # ld & 3
    assert call(gpu, lib.d3r_row_means, P(xd), 2, 8, 4, P(out)) == ERR_INVALID          # ld < cols
    assert call(gpu, lib.d3r_row_means, C.c_void_p(xd.data_ptr() + 4), 2, 7, 8, P(out)) == ERR_INVALID
    assert call(gpu, lib.d3r_row_means, C.c_void_p(xd.data_ptr() + 16), 2, 7, 8, P(out)) == 0
    o = out.cpu()
    assert torch.equal(o[:2], torch.ones(2)) and bool(torch.isnan(o[2:]).all())


# ------------------------------------------------------------------------------------------------------- 2. d3r_similarity_moments
MOM_NPIX = [1, 3, 5, 1023, 1025, 2047, 2048, 2049, 2051, 4099]         # 1, 2 and 3 chunks of 2048 points; every tail length mod 4
MOM_ALONE = 8                                                            # the 2051-point job, repeated alone (nchunk = 2 instead of 3)


@functools.lru_cache(None)
def moments_job(k):
    """Signed, offset, asymmetric clouds (a transposed Sxy cannot pass) and weights in (0, 5] with a few exact zeros."""
    n = MOM_NPIX[k]
    rng = np.random.RandomState(200 + k)
    x = rng.randn(n, 3) + np.array([0.5, -1.0, 2.0])
    y = 0.7 * x @ rng.randn(3, 3).T + 0.3 * rng.randn(n, 3) + np.array([-1.5, 0.25, 1.0])
    w = 5.0 * (1.0 - rng.rand(n))
    if n > 16:
        w[rng.rand(n) < 0.05] = 0.0
    return x.astype(np.float32), y.astype(np.float32), w.astype(np.float32)


def moments_reference(x, y, w):
    """The 17 moments { W, Sx, Sy, Sxy[a][b] = sum w x_a y_b, Sxx } in fp64 and, per moment, sum_p |term_p|."""
    x, y, w = x.astype(np.float64), y.astype(np.float64), w.astype(np.float64)[:, None]
    terms = np.concatenate((w, w * x, w * y, (w[:, :, None] * x[:, :, None] * y[:, None, :]).reshape(len(x), 9),
                            (w * x * x).sum(axis=1, keepdims=True)), axis=1)
    return terms.sum(axis=0), np.abs(terms).sum(axis=0)


def run_moments(gpu, ks):
    from dust3r_amd._lib import lib
    jobs = [moments_job(k) for k in ks]
    keep = [(dev_points(gpu, x), dev_points(gpu, y), dev_scalars(gpu, w)) for x, y, w in jobs]
    npix = [len(j[0]) for j in jobs]
    nbytes = int(lib.d3r_similarity_moments_workspace(len(jobs), max(npix)))
    assert nbytes == len(jobs) * ((max(npix) + 2047) // 2048) * 17 * 8
    ws = dev(gpu, np.full(nbytes // 8, np.nan))
    out = dev(gpu, np.full((len(jobs) + 1) * 17, np.nan))
    src, tgt, wgt = (table(gpu, [k[c] for k in keep]) for c in range(3))
    npix_d = dev(gpu, np.array(npix, np.int32))
    assert call(gpu, lib.d3r_similarity_moments, len(jobs), P(src), P(tgt), P(wgt), P(npix_d), max(npix), P(ws), P(out)) == 0
    res = out.cpu().view(len(jobs) + 1, 17)
    assert bool(torch.isnan(res[-1]).all())
    return res[:-1].clone()


@pytest.fixture(scope='module')
def moments_runs(gpu):
    every = list(range(len(MOM_NPIX)))
    return run_moments(gpu, every), run_moments(gpu, every), run_moments(gpu, [MOM_ALONE])


def test_similarity_moments_ragged_jobs(moments_runs):
    """Ragged jobs in one launch (1, 2 and 3 chunks in use, every tail length) against fp64.
    Bound per moment: a per-thread fp32 partial holds at most 12 terms (Sxx: 3 x 4 points), each term from 2 multiplies, added in turn
    (<= 11 more roundings on partial sums that never exceed sum |term|); everything after is fp64: |got - ref| <= 13 * 2^-24 * sum_p |term_p|,
    asserted at 16 * 2^-24 * sum_p |term_p| (absolute-value sum in fp64), so moments that nearly cancel are held to the same scale."""
    got = moments_runs[0].numpy()
    for k, n in enumerate(MOM_NPIX):
        ref, scale = moments_reference(*moments_job(k))
        err, bound = np.abs(got[k] - ref), 16 * U * scale
        print(f'moments job {k} npix={n}: max err / bound {float((err / np.maximum(bound, 1e-300)).max()):.3f}')
        assert (err <= bound).all(), (k, n, got[k], ref)


def test_similarity_moments_bit_reproducible(moments_runs):
    """Fixed summation order: the same call into a fresh NaN workspace and output gives the same bits, and the 2051-point job gives the
    same bits alone (nchunk = 2) as inside the ragged call (nchunk = 3): its chunking does not depend on max_points."""
    first, second, alone = moments_runs
    assert torch.equal(bits(first), bits(second))
    assert torch.equal(bits(first[MOM_ALONE]), bits(alone[0]))


# --------------------------------------------------------------------------------------------------------- 3. d3r_weiszfeld_focals
WZ_SHAPES = [(5, 7), (9, 13), (31, 33), (32, 32), (25, 41), (40, 56)]    # below, at and above the 1024-thread block; odd widths


@functools.lru_cache(None)
def pinhole_map(H, W, seed, spoil=False):
    """Synthetic pinhole cloud: focal 0.9 max(H, W), depth in [1, 3], 1 % noise. spoil: 5 % of the pixels get Z = 0, X = +-inf or X = NaN."""
    rng = np.random.RandomState(seed)
    f = 0.9 * max(H, W)
    v, u = np.mgrid[0:H, 0:W].astype(np.float64)
    d = rng.uniform(1, 3, (H, W))
    pts = np.stack(((u - W / 2) / f * d, (v - H / 2) / f * d, d), axis=-1) * (1 + 0.01 * rng.randn(H, W, 3))
    pts = pts.reshape(-1, 3).astype(np.float32)
    if spoil:
        bad = np.nonzero(rng.rand(H * W) < 0.05)[0]
        kind = rng.randint(0, 4, len(bad))
        pts[bad[kind == 0], 2] = 0.0
        pts[bad[kind == 1], 0] = np.inf
        pts[bad[kind == 2], 0] = -np.inf
        pts[bad[kind == 3], 0] = np.nan
        assert len(bad) >= 4
    return pts


def weiszfeld_reference(pts, H, W, iterations):
    """fp64 restatement of the reference's estimate_focal_knowing_depth(focal_mode='weiszfeld'), principal point at the image centre.
    Returns the focal and the two absolute-value sums of the closed-form start."""
    p = pts.astype(np.float64)
    v, u = np.mgrid[0:H, 0:W].astype(np.float64)
    px = np.stack((u - W / 2, v - H / 2), axis=-1).reshape(-1, 2)
    with np.errstate(divide='ignore', invalid='ignore'):
        r = p[:, :2] / p[:, 2:3]
        r = np.where(np.isfinite(r), r, 0.0)                                 # nan_to_num(posinf=0, neginf=0)
        dpx, dxx = (r * px).sum(axis=-1), (r * r).sum(axis=-1)
        f = dpx.sum() / dxx.sum()
        for _ in range(iterations):
            wgt = 1.0 / np.maximum(np.linalg.norm(px - f * r, axis=-1), 1e-8)
            f = (wgt * dpx).sum() / (wgt * dxx).sum()
    return float(np.fmax(f, 0.0)), float(np.abs(r * px).sum()), float(dxx.sum())      # clip(min=0); NaN (0 / 0) -> 0 like fmaxf


def run_weiszfeld(gpu, maps, shapes, iterations):
    from dust3r_amd._lib import lib
    keep = [dev_points(gpu, m) for m in maps]
    hs, ws = dev(gpu, np.array([s[0] for s in shapes], np.int32)), dev(gpu, np.array([s[1] for s in shapes], np.int32))
    out, ptrs = dev(gpu, np.full(len(maps) + 1, np.nan, np.float32)), table(gpu, keep)
    assert call(gpu, lib.d3r_weiszfeld_focals, len(maps), P(ptrs), P(hs), P(ws), iterations, P(out)) == 0
    res = out.cpu()
    assert bool(torch.isnan(res[-1]))
    return res[:-1].clone()


def test_weiszfeld_focals_ragged_maps(gpu):
    """Six maps of different shapes in one call (hs[job], ws[job] per job, the p / W split at odd widths, maps below / at / above one
    block) against the fp64 restatement at relative 1e-5 (the figure tests/test_aligner_gpu.py already holds this kernel to), and the
    closed-form start (iterations = 0) against the closed form. Bound there: per pixel a = X / Z (1 rounding), a px + b py (<= 2 more),
    a a + b b (<= 2 + 2): each fp32 term within 4 * 2^-24 of its absolute value, the rest fp64, one fp32 rounding of the focal. Asserted with
    relative 8 * 2^-24 on each of the two absolute-value sums: |got - S1 / S2| <= (e1 + |ref| e2) / (S2 - e2), e1 = 8 * 2^-24 sum |a px| + |b py|,
    e2 = 8 * 2^-24 S2."""
    maps = [pinhole_map(H, W, 300 + k) for k, (H, W) in enumerate(WZ_SHAPES)]
    got = run_weiszfeld(gpu, maps, WZ_SHAPES, 10).double().numpy()
    got0 = run_weiszfeld(gpu, maps, WZ_SHAPES, 0).double().numpy()
    for k, (H, W) in enumerate(WZ_SHAPES):
        ref, _, _ = weiszfeld_reference(maps[k], H, W, 10)
        ref0, a1, a2 = weiszfeld_reference(maps[k], H, W, 0)
        bound0 = (8 * U * a1 + abs(ref0) * 8 * U * a2) / (a2 - 8 * U * a2)
        print(f'weiszfeld {H}x{W}: 10 iterations {got[k]:.6f} vs {ref:.6f} (rel {abs(got[k] / ref - 1):.2e}); closed form err {abs(got0[k] - ref0):.3e} bound {bound0:.3e}')
        assert abs(ref / (0.9 * max(H, W)) - 1) < 0.05                           # the reference itself finds the focal of the cloud
        assert abs(got[k] / ref - 1) < 1e-5
        assert abs(got0[k] - ref0) <= bound0


def test_weiszfeld_focals_non_finite_points(gpu):
    """nan_to_num(posinf=0, neginf=0): pixels with Z = 0, X = +-inf or X = NaN contribute zero. A job whose map is all Z = 0 returns 0
    (0 / 0, then clip(min=0)) and leaves the other jobs of the call bit-identical to a call without it."""
    shapes = [(25, 41), (40, 56)]
    maps = [pinhole_map(H, W, 310 + k, spoil=True) for k, (H, W) in enumerate(shapes)]
    got = run_weiszfeld(gpu, maps, shapes, 10).double().numpy()
    for k, (H, W) in enumerate(shapes):
        ref, _, _ = weiszfeld_reference(maps[k], H, W, 10)
        clean, _, _ = weiszfeld_reference(pinhole_map(H, W, 310 + k), H, W, 10)
        print(f'weiszfeld spoiled {H}x{W}: {got[k]:.6f} vs {ref:.6f} (rel {abs(got[k] / ref - 1):.2e}; unspoiled map {clean:.6f})')
        assert abs(got[k] / ref - 1) < 1e-5 and abs(ref / (0.9 * max(H, W)) - 1) < 0.05
    flat = pinhole_map(9, 13, 320).copy()
    flat[:, 2] = 0.0
    assert weiszfeld_reference(flat, 9, 13, 10)[0] == 0.0
    with_flat = run_weiszfeld(gpu, [maps[0], flat, maps[1]], [shapes[0], (9, 13), shapes[1]], 10)
    alone = run_weiszfeld(gpu, maps, shapes, 10)
    assert float(with_flat[1]) == 0.0
    assert torch.equal(bits(with_flat[[0, 2]]), bits(alone))


# ------------------------------------------------------------------------------------------------------------- 4. d3r_anchor_depth
AD_MAX_AREA = 1000                                                       # not a multiple of the 256-thread block
AD_NPIX = [1, 255, 256, 257, 1000]


@functools.lru_cache(None)
def anchor_depth_case():
    """Rows and maps built so that z = row . (p, 1) is >= 0.3 on about two thirds of the points and <= -0.05 on the rest (never in
    (0, 0.25): the log amplifies the fp32 dot-product error near 0), plus one exact z = 0 and one map with NaN points."""
    rng = np.random.RandomState(400)
    m = rng.randn(len(AD_NPIX), 3)
    m *= (rng.uniform(0.7, 1.3, len(AD_NPIX)) / np.linalg.norm(m, axis=1))[:, None]
    rows = np.concatenate((m, rng.uniform(-0.5, 0.5, (len(AD_NPIX), 1))), axis=1)
    rows[2, 3] = 0.0
    rows = rows.astype(np.float32)
    maps = []
    for k, n in enumerate(AD_NPIX):
        mk, m3 = rows[k, :3].astype(np.float64), float(rows[k, 3])
        q0 = rng.uniform(-1, 1, (n, 3))
        z = np.where(rng.rand(n) < 1 / 3, -rng.uniform(0.05, 2, n), rng.uniform(0.3, 4, n))
        q = q0 + mk * ((z - m3 - q0 @ mk) / (mk @ mk))[:, None]
        if k == 2:
            q[5] = 0.0                                                       # z = 0 exactly: log -> -inf -> 0
        if k == 4:
            nan = np.nonzero(rng.rand(n) < 0.02)[0]
            q[nan[::2]] = np.nan
            q[nan[1::2], 1] = np.nan
        maps.append(q.astype(np.float32))
    return rows, maps


def anchor_depth_reference():
    """Per image: fp64 z (NaN where the point is), and |m0 q0| + |m1 q1| + |m2 q2| + |m3|."""
    rows, maps = anchor_depth_case()
    out = []
    for r, q in zip(rows.astype(np.float64), maps):
        q = q.astype(np.float64)
        out.append((q @ r[:3] + r[3], np.abs(q * r[:3]).sum(axis=1) + abs(r[3])))
    return out


def check_anchor_depth_inputs():
    n_neg = n_all = 0
    for k, (z, scale) in enumerate(anchor_depth_reference()):
        ok = ~np.isnan(z)
        assert not ((z[ok] > 0) & (z[ok] < 0.25)).any(), 'a point with z in (0, 0.25)'
        assert (np.abs(z[ok]) > 100 * 4 * U * scale[ok]).all() or k == 2      # the sign of z is beyond fp32's reach (image 2 holds the exact zero)
        pos = ok & (z >= 0.25)
        # why absolute 1e-5 on log z is attainable: dz <= 4 * 2^-24 scale, d(log z) <= dz / (z - dz), plus logf's own rounding (a few ulp of |log z| <= 2)
        assert (4 * U * scale[pos] / (z[pos] - 4 * U * scale[pos]) + 8 * U * np.maximum(np.abs(np.log(z[pos])), 1)).max() < 1e-5
        n_neg, n_all = n_neg + int((z[ok] <= 0).sum()), n_all + int(ok.sum())
    assert 0.25 < n_neg / n_all < 0.42                                       # about a third with z <= 0
    assert np.isnan(anchor_depth_reference()[4][0]).sum() >= 4 and anchor_depth_reference()[2][0][5] == 0.0


@pytest.mark.parametrize('take_log', [0, 1])
def test_anchor_depth_ragged_images(gpu, take_log):
    """npix below, at and above one block and up to a max_area that is no multiple of 256: padding [img][p >= npix] exactly 0, the
    sentinel row after the last image untouched. take_log = 0: z within 4 * 2^-24 (|m0 q0| + |m1 q1| + |m2 q2| + |m3|) (3 products, 3
    sums); NaN points give NaN. take_log = 1: exactly 0 where z <= 0 or NaN (log().nan_to_num(neginf=0) of the reference plus the
    aligner's zero padding), absolute 1e-5 on log z where z >= 0.25 (the figure of tests/test_aligner_gpu.py)."""
    from dust3r_amd._lib import lib
    check_anchor_depth_inputs()
    rows, maps = anchor_depth_case()
    n = len(AD_NPIX)
    keep = [dev_points(gpu, q) for q in maps]
    out = dev(gpu, np.full((n + 1) * AD_MAX_AREA, np.nan, np.float32))
    ptrs, rows_d, npix_d = table(gpu, keep), dev(gpu, rows), dev(gpu, np.array(AD_NPIX, np.int32))
    assert call(gpu, lib.d3r_anchor_depth, n, P(ptrs), P(rows_d), P(npix_d), AD_MAX_AREA, take_log, P(out)) == 0
    got = out.cpu().view(n + 1, AD_MAX_AREA).double().numpy()
    assert np.isnan(got[n]).all()
    for k, (z, scale) in enumerate(anchor_depth_reference()):
        npix = AD_NPIX[k]
        assert (got[k, npix:] == 0).all() and not np.signbit(got[k, npix:]).any()
        g, nan = got[k, :npix], np.isnan(z)
        if not take_log:
            assert np.isnan(g[nan]).all()
            err = np.abs(g[~nan] - z[~nan])
            print(f'anchor depth image {k}: max err / bound {float((err / np.maximum(4 * U * scale[~nan], 1e-300)).max()):.3f}')
            assert (err <= 4 * U * scale[~nan]).all()
        else:
            dead = nan | (z <= 0)
            assert (g[dead] == 0).all()
            live = ~dead
            assert (z[live] >= 0.25).all()
            err = np.abs(g[live] - np.log(z[live]))
            print(f'anchor log-depth image {k}: {int(dead.sum())} of {npix} points at 0, max err {float(err.max(initial=0)):.3e}')
            assert (err < 1e-5).all()


# ---------------------------------------------------------------------------------------------------- 5 / 6. d3r_pnp_score, d3r_pnp_sums
PNP_SHAPES = [(3, 5), (16, 17), (160, 168)]          # 160 x 168 = 26 880 points > 96 blocks x 256 threads: a second, ragged trip of the grid-stride loop
REPROJ = 2.0                                         # pixels; its square is exact in fp32
CONF_THR = 3.0
PNP_SEEDS = [503, 519, 502]                          # chosen on the CPU so that the conditions of check_pnp_score_case hold (they are asserted)


def rotation(axis, angle):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * K @ K


class PnpCase:
    """One image job with an unambiguous consensus set, built in fp64 from the pose: per pixel (u, v) a residual r with |r| <= 0.8 REPROJ
    (inliers) or |r| >= 1.25 REPROJ (outliers, 20 %) and a depth d in [1, 3]; Xc = d ((u + r_u - ppx) / f, (v + r_v - ppy) / f, 1),
    world = R^T (Xc - t), map = G^-1 world, rounded to fp32 (which moves residuals by ~1e-5 px, far inside the gap). A tenth of the
    outliers sit BEHIND the camera (d < 0) with an inlier-sized residual: only the z > 0 test keeps them out. Confidences: mostly above
    the threshold, 10 % exactly equal to it (excluded: conf > thr), 1 % NaN (excluded). residuals=False: exact geometry, every point an inlier."""

    def __init__(self, H, W, seed, residuals=True):
        rng = np.random.RandomState(seed)
        n = H * W
        self.H, self.W, self.n = H, W, n
        self.f, self.ppx, self.ppy = np.float32(1.125 * max(H, W)), np.float32(W / 2 + 0.25), np.float32(H / 2 - 0.25)
        self.pose = np.concatenate((rotation(rng.randn(3), 0.3), [[0.2], [-0.1], [0.3]]), axis=1).astype(np.float32)     # world -> camera
        self.G = np.concatenate((rotation(rng.randn(3), 0.5), [[0.4], [-0.3], [0.2]]), axis=1).astype(np.float32)       # map -> world, rigid
        p = np.arange(n)
        self.uv = np.stack((p % W, p // W), axis=1).astype(np.float64)
        order = rng.permutation(n)                                           # exact shares, so that the 15-point job has its outliers too
        outlier, behind = np.zeros(n, bool), np.zeros(n, bool)
        outlier[order[:int(np.ceil(0.2 * n))]] = True
        behind[order[:int(np.ceil(0.02 * n))]] = True
        mag =np.where(outlier & ~behind, rng.uniform(1.25, 3.0, n), rng.uniform(0.0, 0.8, n)) * REPROJ
        ang = rng.uniform(0, 2 * np.pi, n)
        d = rng.uniform(1, 3, n)
        if residuals:
            d[behind] *= -1
        else:
            outlier[:], behind[:], mag[:] = False, False, 0.0
        r = mag[:, None] * np.stack((np.cos(ang), np.sin(ang)), axis=1)
        f, pp = float(self.f), np.array([float(self.ppx), float(self.ppy)])
        Xc = d[:, None] * np.concatenate(((self.uv + r - pp) / f, np.ones((n, 1))), axis=1)
        P64, G64 = self.pose.astype(np.float64), self.G.astype(np.float64)
        world = np.linalg.solve(P64[:, :3], (Xc - P64[:, 3]).T).T
        self.map = np.linalg.solve(G64[:, :3], (world - G64[:, 3]).T).T.astype(np.float32)
        conf = rng.uniform(3.5, 50, n).astype(np.float32)
        order = rng.permutation(n)
        conf[order[:int(np.ceil(0.10 * n))]] = CONF_THR
        conf[order[-int(np.ceil(0.01 * n)):]] = np.nan
        self.conf = conf
        with np.errstate(invalid='ignore'):
            self.mask = conf > np.float32(CONF_THR)
        self.inlier = self.mask & ~outlier                                   # by construction; the references below recompute it from the fp32 inputs
        self.outlier, self.behind = outlier, behind

    def world(self):
        """World points in fp64 from the fp32 inputs the kernel gets."""
        G = self.G.astype(np.float64)
        return self.map.astype(np.float64) @ G[:, :3].T + G[:, 3]

    def reproject(self, pose):
        """Camera points and reprojection residuals (predicted - pixel) in fp64 under a world -> camera pose (3, 4)."""
        pose = np.asarray(pose, np.float64)
        Xc = self.world() @ pose[:, :3].T + pose[:, 3]
        with np.errstate(divide='ignore', invalid='ignore'):
            r = float(self.f) * Xc[:, :2] / Xc[:, 2:3] + np.array([float(self.ppx), float(self.ppy)]) - self.uv
        return Xc, r


@functools.lru_cache(None)
def pnp_case(k, residuals=True):
    H, W = PNP_SHAPES[k]
    return PnpCase(H, W, PNP_SEEDS[k], residuals)


def check_pnp_case(case):
    """The residual gap holds on the fp32 inputs: every masked point in front of the camera is either within 0.8 REPROJ (+ rounding) or
    beyond 1.25 REPROJ, exactly as constructed; the points behind the camera would pass the distance test."""
    Xc, r = case.reproject(case.pose)
    err = np.linalg.norm(r, axis=1)
    front = Xc[:, 2] > 0
    assert (front == ~case.behind).all() and (np.abs(Xc[:, 2]) > 0.5).all()
    assert (err[~case.outlier] < 0.8 * REPROJ + 1e-3).all() and (err[case.outlier & ~case.behind] > 1.25 * REPROJ - 1e-3).all()
    assert (err[case.behind] < 0.8 * REPROJ + 1e-3).all()
    return int(case.inlier.sum())


def pnp_records(gpu, cases):
    """DEVICE array of job records { map, conf, G, f, ppx, ppy, thr, H, W } (include/dust3r_hip.h) + the tensors they point to."""
    from dust3r_amd._lib import lib
    from dust3r_amd.cloud_opt.bootstrap import _PnpJobRec
    assert lib.d3r_pnp_job_bytes() == C.sizeof(_PnpJobRec)
    keep = [(dev_points(gpu, c.map), dev_scalars(gpu, c.conf)) for c in cases]
    recs = (_PnpJobRec * len(cases))()
    for r, c, (m, cf) in zip(recs, cases, keep):
        r.map, r.conf = m.data_ptr(), cf.data_ptr()
        for i, v in enumerate(c.G.reshape(12)):
            r.G[i] = float(v)
        r.f, r.ppx, r.ppy, r.thr, r.H, r.W = float(c.f), float(c.ppx), float(c.ppy), CONF_THR, c.H, c.W
    return torch.frombuffer(bytearray(bytes(recs)), dtype=torch.uint8).to(gpu), keep


# -- 5. consensus counts
LADDER = (0.6, 3.0, 2.0, 0.5)                        # image shift of the first and the last rung in pixels, roll per unit of tilt, stride modulation


def pnp_hypotheses(case, n_hyp):
    """(n_hyp, 3, 4) fp32: the true pose; a copy turned a quarter turn about the camera's y axis (z' = -x: half the points behind the
    camera); then a ladder of copies perturbed by growing rotations about the camera origin and translations, shifting the image by
    0.7 ... 3.7 px, so that counts fall from about all inliers to about none."""
    P64 = case.pose.astype(np.float64)
    hyps = [P64]
    if n_hyp > 1:
        hyps.append(rotation([0, 1, 0], np.pi / 2) @ P64)
    rungs = n_hyp - 2
    for k in range(rungs):
        x = k / max(rungs - 1, 1)                                             # longer strides at both ends, where the counts move slowly
        shift = LADDER[0] + (LADDER[1] - LADDER[0]) * (x + LADDER[3] * np.sin(2 * np.pi * x) / (2 * np.pi))   # pixels
        w = 0.75 * shift / float(case.f) * np.array([0.8, -0.6, LADDER[2]])    # f theta px by the rotation, towards (-0.6, -0.8), plus a roll that
        Q = rotation(w, np.linalg.norm(w)) @ P64                               # grows with the radius (it spreads the errors: fewer points near the threshold)
        Q[:, 3] += np.array([-0.6, -0.8, 0.0]) * 0.25 * shift * 2.0 / float(case.f)   # ... and f dt / depth by the translation (depth ~ 2), same direction
        hyps.append(Q)
    return np.stack(hyps).astype(np.float32)


def pnp_score_reference(case, hyps, thr=REPROJ):
    """Per hypothesis (lo, hi): lo counts the decided inliers, hi adds the undecided points -- fp64 error within 1e-3 px of thr, or |zc| < 1e-4."""
    lo, hi = [], []
    for h in hyps:
        Xc, r = case.reproject(h)
        err, zc = np.linalg.norm(r, axis=1), Xc[:, 2]
        with np.errstate(invalid='ignore'):
            und = case.mask & ((np.abs(zc) < 1e-4) | (np.abs(err - thr) <= 1e-3))
            dec = case.mask & ~und & (zc > 0) & (err < thr)
        lo.append(int(dec.sum()))
        hi.append(int(dec.sum() + und.sum()))
    return np.array(lo), np.array(hi)


def check_pnp_score_case(case, k, n_hyp):
    """Conditions on the inputs of job k, on the reference alone: undecided points are at most 0.1 % of the job's points for every
    hypothesis (none at all in the two small jobs), the true pose has none and counts exactly the constructed consensus set, the
    quarter-turn hypothesis has about half the points behind the camera, the ladder falls from about all inliers (>= 80 %) to about none
    (<= 20 %), and its rungs lie more than ten times that 0.1 % (1 % of the job's points) apart. 30 rungs cannot lie 1 % apart inside the 10
    inliers of the 15-point job, nor with any regularity inside the 193 of the 272-point job: at n_hyp = 32 those two jobs are required
    to fall monotonically over the same span instead; at n_hyp = 7 every job meets the condition as stated."""
    n_in = check_pnp_case(case)
    hyps = pnp_hypotheses(case, n_hyp)
    lo, hi = pnp_score_reference(case, hyps)
    assert ((hi - lo) <= 0.001 * case.n).all(), (k, hi - lo)
    assert lo[0] == hi[0] == n_in and n_in > 0.5 * case.n
    if n_hyp > 1:
        zc = case.reproject(hyps[1])[0][:, 2]
        assert 0.3 < (zc < 0).mean() < 0.7
    if n_hyp > 2:
        ladder = lo[2:]
        assert ladder[0] >= 0.8 * n_in and ladder[-1] <= 0.2 * n_in, (k, ladder)
        steps = ladder[:-1] - ladder[1:]
        if n_hyp == 7 or k == 2:
            assert (steps > 10 * 0.001 * case.n).all(), (k, ladder)
        else:
            assert (steps >= 0).all(), (k, ladder)
    return lo, hi


def check_pnp_score_inputs(n_hyp):
    return [check_pnp_score_case(pnp_case(k), k, n_hyp) for k in range(len(PNP_SHAPES))]


@pytest.mark.parametrize('n_hyp', [1, 7, 32])
def test_pnp_score_counts(gpu, n_hyp):
    """Three jobs in one call, the last taking a second ragged trip of the grid-stride loop; non-trivial G; confidences equal to the
    threshold and NaN excluded; points behind the camera; counts pre-filled with garbage; the slots h >= n_hyp hold the TRUE pose and
    must still come back 0. lo <= count <= hi per hypothesis, the true pose exactly (nothing undecided by construction)."""
    from dust3r_amd._lib import lib
    maxh = int(lib.d3r_pnp_max_hypotheses())
    assert maxh == 32
    refs = check_pnp_score_inputs(n_hyp)
    cases = [pnp_case(k) for k in range(len(PNP_SHAPES))]
    recs, keep = pnp_records(gpu, cases)
    hyp = np.stack([np.broadcast_to(c.pose, (maxh, 3, 4)).copy() for c in cases])
    for k, c in enumerate(cases):
        hyp[k, :n_hyp] = pnp_hypotheses(c, n_hyp)
    counts = dev(gpu, np.full((len(cases) + 1) * maxh, 0x5a5a5a5a, np.int32))
    hyp_d = dev(gpu, hyp)
    assert call(gpu, lib.d3r_pnp_score, len(cases), P(recs), P(hyp_d), n_hyp, REPROJ, P(counts)) == 0
    got = counts.cpu().view(len(cases) + 1, maxh).numpy()
    assert (got[-1] == 0x5a5a5a5a).all()
    for k, (lo, hi) in enumerate(refs):
        print(f'pnp_score job {k} n_hyp={n_hyp}: counts {got[k, :n_hyp].tolist()} lo {lo.tolist()} hi {hi.tolist()}')
        assert (got[k, n_hyp:] == 0).all()
        assert got[k, 0] == lo[0]
        assert (lo <= got[k, :n_hyp]).all() and (got[k, :n_hyp] <= hi).all()


# -- 6. Gauss-Newton sums
TRIU = np.triu_indices(6)                                                # upper triangle, row-major: (0,0) (0,1) ... (0,5) (1,1) ...


def pnp_jacobians(case, pose):
    """(n, 2, 6) Jacobian of the projection by the pose increment, from autograd in fp64: d proj(exp([w]x) R X + t + dt) / d(w, dt) at 0.
    The independent statement of the convention the host polish relies on (R <- exp([w]x) R, t <- t + dt)."""
    pose = torch.from_numpy(np.asarray(pose, np.float64))
    R, t = pose[:, :3], pose[:, 3]
    f, pp = float(case.f), torch.tensor([float(case.ppx), float(case.ppy)], dtype=torch.float64)

    def proj(delta, X):
        w, z = delta[:3], delta.new_zeros(())
        K = torch.stack((torch.stack((z, -w[2], w[1])), torch.stack((w[2], z, -w[0])), torch.stack((-w[1], w[0], z))))
        Xc = torch.linalg.matrix_exp(K) @ (R @ X) + t + delta[3:]
        return f * Xc[:2] / Xc[2] + pp
    J = torch.func.vmap(torch.func.jacrev(proj), in_dims=(None, 0))(torch.zeros(6, dtype=torch.float64), torch.from_numpy(case.world()))
    return J.numpy()


def sum_terms(J, r):
    """(n, 28) per-point terms of J^T J (21, upper triangle row-major), J^T r (6) and the cost."""
    JtJ = (J[:, :, TRIU[0]] * J[:, :, TRIU[1]]).sum(axis=1)
    return np.concatenate((JtJ, (J * r[:, :, None]).sum(axis=1), (r * r).sum(axis=1, keepdims=True)), axis=1)


def pnp_sums_reference(case, pose, thr=REPROJ):
    """fp64: (29 sums, per-sum sum_p |term_p| (28), inlier mask)."""
    Xc, r = case.reproject(pose)
    with np.errstate(invalid='ignore'):
        inl = case.mask & (Xc[:, 2] > 0) & ((r * r).sum(axis=1) < thr * thr)
    terms = sum_terms(pnp_jacobians(case, pose)[inl], r[inl])
    return np.concatenate((terms.sum(axis=0), [inl.sum()])), np.abs(terms).sum(axis=0), inl


def pnp_sums_float32(case, pose, inl):
    """The same per-point expressions once in numpy float32 (chain rule d proj / d Xc . [ -[Xc - t]x | I ], with the cancellation of
    Xc - t that a closed-form bound would have to carry), sums in fp64: measures what fp32 arithmetic costs on THESE inputs. A
    restatement for the tolerance only; the reference is autograd."""
    f32 = np.float32
    pose, G = np.asarray(pose, f32), case.G
    X = (case.map[inl][:, None, :] * G[:, :3][None]).sum(axis=2, dtype=f32) + G[:, 3]
    Xc = (X[:, None, :] * pose[:, :3][None]).sum(axis=2, dtype=f32) + pose[:, 3]
    iz = f32(1) / Xc[:, 2]
    r = case.f * Xc[:, :2] * iz[:, None] + np.array([case.ppx, case.ppy], f32) - case.uv[inl].astype(f32)
    Xr = Xc - pose[:, 3]
    n, o = len(X), np.zeros(len(X), f32)
    fx = case.f * iz
    dproj = np.stack((np.stack((fx, o, -case.f * Xc[:, 0] * iz * iz), axis=1), np.stack((o, fx, -case.f * Xc[:, 1] * iz * iz), axis=1)), axis=1)   # (n, 2, 3)
    S = np.stack((np.stack((o, Xr[:, 2], -Xr[:, 1]), axis=1), np.stack((-Xr[:, 2], o, Xr[:, 0]), axis=1), np.stack((Xr[:, 1], -Xr[:, 0], o), axis=1)), axis=1)   # -[Xr]x
    J = np.concatenate((np.einsum('nij,njk->nik', dproj, S).astype(f32), dproj), axis=2)
    terms = sum_terms(J, r)
    assert terms.dtype == f32 and terms.shape == (n, 28)
    return terms.astype(np.float64).sum(axis=0)


def run_pnp_sums(gpu, recs, poses, thr=REPROJ):
    from dust3r_amd._lib import lib
    n = len(poses)
    assert int(lib.d3r_pnp_sum_count()) == 29
    ws = dev(gpu, np.full(int(lib.d3r_pnp_workspace(n)) // 8, np.nan))
    out = dev(gpu, np.full((n + 1) * 29, np.nan))
    poses_d = dev(gpu, np.asarray(poses, np.float32))
    assert call(gpu, lib.d3r_pnp_sums, n, P(recs), P(poses_d), thr, P(ws), P(out)) == 0
    res = out.cpu().view(n + 1, 29)
    assert bool(torch.isnan(res[-1]).all())
    return res[:-1].clone()


@pytest.fixture(scope='module')
def pnp_sums_runs(gpu):
    cases = [pnp_case(k) for k in range(len(PNP_SHAPES))]
    recs, keep = pnp_records(gpu, cases)
    poses = [c.pose for c in cases]
    lost = [p.copy() for p in poses]
    lost[0][0, 3] += 100.0                                                   # job 0 sees no inlier under this pose
    return run_pnp_sums(gpu, recs, poses), run_pnp_sums(gpu, recs, poses), run_pnp_sums(gpu, recs, lost)


def test_pnp_sums_match_autograd(pnp_sums_runs):
    """out[28] is the inlier count exactly; out[0:21] = J^T J (upper triangle, row-major), out[21:27] = J^T r, out[27] = cost, with J from
    autograd in fp64. Tolerance per sum, from the reference alone: e32 = |the same expressions in numpy float32 - fp64|, and the kernel must
    stay within 4 * max(e32, 2^-24 * sum_p |term_p|) (4: FMA contraction and another association order than numpy's)."""
    got = pnp_sums_runs[0].numpy()
    for k in range(len(PNP_SHAPES)):
        case = pnp_case(k)
        n_in = check_pnp_case(case)
        ref, scale, inl = pnp_sums_reference(case, case.pose)
        assert ref[28] == n_in and (inl == case.inlier).all()
        e32 = np.abs(pnp_sums_float32(case, case.pose, inl) - ref[:28])
        err, bound = np.abs(got[k, :28] - ref[:28]), 4 * np.maximum(e32, U * scale)
        print(f'pnp_sums job {k} ({case.H}x{case.W}, {n_in} inliers of {case.n}): sum, reference, kernel error, e32, 2^-24 sum|term|, error / bound')
        for i in range(28):
            print(f'  out[{i:2d}] {ref[i]: .9e} {err[i]:.3e} {e32[i]:.3e} {U * scale[i]:.3e} {err[i] / max(bound[i], 1e-300):.3f}')
        assert got[k, 28] == n_in
        assert (err <= bound).all(), (k, np.nonzero(err > bound)[0])


def test_pnp_sums_bit_reproducible(pnp_sums_runs):
    """Fixed summation order: the same call twice, workspace pre-filled with NaN, gives the same bits. A job whose pose sees no inlier
    returns 29 zeros and leaves the other jobs of the call as they were."""
    first, second, lost = pnp_sums_runs
    assert torch.equal(bits(first), bits(second))
    assert bool((lost[0] == 0).all())
    assert torch.equal(bits(lost[1:]), bits(first[1:]))


def test_pnp_sums_gauss_newton_step(gpu):
    """The convention, closed: on exact geometry, from the true pose perturbed by 1e-2 (rotation vector and translation), ONE Gauss-Newton
    step with the kernel's sums -- solved in fp64 here, applied as R <- exp([w]x) R, t <- t + dt -- takes the cost below 1 % of its start
    (quadratic convergence on consistent data; a sign or ordering error in J breaks it). The band is 16 px here so that the consensus set
    is the whole masked map before and after."""
    cases = [pnp_case(k, False) for k in range(len(PNP_SHAPES))]
    recs, keep = pnp_records(gpu, cases)
    start = []
    for k, c in enumerate(cases):
        rng = np.random.RandomState(600 + k)
        w, dt = rng.randn(3), rng.randn(3)
        Q = c.pose.astype(np.float64)
        Q = np.concatenate((rotation(w, 1e-2) @ Q[:, :3], (Q[:, 3] + 1e-2 * dt / np.linalg.norm(dt))[:, None]), axis=1)
        start.append(Q)
    g0 = run_pnp_sums(gpu, recs, start, thr=16.0).numpy()
    stepped = []
    for k, Q in enumerate(start):
        H = np.zeros((6, 6))
        H[TRIU] = g0[k, :21]
        H = H + H.T - np.diag(np.diag(H))
        d = np.linalg.solve(H, -g0[k, 21:27])
        w = d[:3]
        K = torch.tensor([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]], dtype=torch.float64)
        stepped.append(np.concatenate((torch.linalg.matrix_exp(K).numpy() @ Q[:, :3], (Q[:, 3] + d[3:])[:, None]), axis=1))
    g1 = run_pnp_sums(gpu, recs, stepped, thr=16.0).numpy()
    for k, c in enumerate(cases):
        print(f'pnp_sums Gauss-Newton job {k}: cost {g0[k, 27]:.4e} -> {g1[k, 27]:.4e} over {int(g0[k, 28])} points')
        assert g0[k, 28] == g1[k, 28] == int(c.mask.sum())
        assert g1[k, 27] < 0.01 * g0[k, 27]


def check_input_conditions():
    """Everything the tests above require of their inputs, evaluated on the references alone (no GPU)."""
    check_anchor_depth_inputs()
    for n_hyp in (1, 7, 32):
        check_pnp_score_inputs(n_hyp)
    for k in range(len(PNP_SHAPES)):
        check_pnp_case(pnp_case(k))
        exact = pnp_case(k, False)
        assert np.linalg.norm(exact.reproject(exact.pose)[1], axis=1).max() < 1e-3 and (exact.reproject(exact.pose)[0][:, 2] > 0.5).all()
