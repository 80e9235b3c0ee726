"""CPU pins of the references that tests/test_ln_fold_gpu.py holds the folded-LayerNorm chain to (oracle/ln_fold_ref.py), of the conditions on their inputs, and
of the argument checks of the chain's four entry points (d3r_ln_finalize, d3r_ln_fold_pack, d3r_linear_ln, d3r_layernorm_x3rows). No device."""
import ctypes as C
import os
import re

import numpy as np
import torch

from oracle.heads_ref import fold_inputs, layernorm_stats
from oracle import ln_fold_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# threads of a tile per row of it, clipped to 1 / 2 / 4: how many adjacent lanes form one row's statistics in a consumer's prologue (gemm.hip, ln_part_in)
TILE_TPR = {'0': 2, '0w8': 4, '1': 2, '2': 2, '3': 1, '7': 1, '8': 4, '9': 1, '11': 2}
TILE_TYPEDEF = {'0': 'Cfg128', '0w8': 'Cfg128w8', '1': 'Cfg256', '2': 'Cfg256x128', '3': 'Cfg512x128', '7': 'Cfg256x128r', '8': 'Cfg64s3', '9': 'Cfg384x192', '11': 'Cfg96x64'}


def _r(x):
    from dust3r_amd import ops
    return ops.unpack_x3(ops.pack_x3(x))


def test_threads_per_row_of_every_tile():
    """TILE_TPR (which tile exercises ln_row_stats<1>, <2>, <4>) against the tile table of gemm.hip: GemmCfg<NWI, NWJ, FI, FJ, ...> has NT = 64 NWI NWJ threads
    and BM = 16 NWJ FJ rows; TPR = NT / BM clipped to 1, 2, 4. All three values occur."""
    src = open(os.path.join(ROOT, 'dust3r_amd', 'csrc', 'gemm.hip')).read()
    for cfg, name in TILE_TYPEDEF.items():
        m = re.search(r'typedef GemmCfg<(\d+), (\d+), (\d+), (\d+)[^>]*> ' + name + ';', src)
        assert m, name
        nwi, nwj, fi, fj = map(int, m.groups())
        nt, bm = 64 * nwi * nwj, 16 * nwj * fj
        assert TILE_TPR[cfg] == (4 if nt // bm >= 4 else 2 if nt // bm >= 2 else 1), (cfg, nt, bm)
    assert set(TILE_TPR.values()) == {1, 2, 4}


def test_finalize_reference_and_edge_rows():
    """finalize_ref on exact inputs is the two-pass LayerNorm statistic; the edge rows are what the GPU test says they are: the 0.25 k rows have exact partials (var
    exactly 0, rstd = 1 / sqrt(eps)); the CONST_VALUES rows leave q / C - mean^2 slightly NEGATIVE for some (value, C) and slightly POSITIVE for others -- 0.2 alone shows
    both signs across the C list -- so the clamp and its neighbourhood are both exercised; the offset rows have |mean| = 100 std within 1 %."""
    eps = 1e-6
    signs = {}
    for C_ in R.FINALIZE_C:
        x = _r(R.finalize_rows(64, C_, C_))
        rstd, nmr, var = R.finalize_ref(R.partials(x), C_, eps)
        mean2, rstd2 = layernorm_stats(x, eps)
        assert float((rstd / rstd2 - 1).abs().max()) < 1e-5 and float((nmr + mean2 * rstd2).abs().max()) < 1e-5
        xe, sl = R.finalize_edge_rows(C_, 7 * C_)
        xe = _r(xe)
        assert torch.equal(_r(xe), xe)
        part = R.partials(xe)
        rstd, nmr, var = R.finalize_ref(part, C_, eps)
        g = xe[sl['quarter']].view(4, C_ // 32, 32).double()
        assert torch.equal(part[sl['quarter'], :, 0].double(), g.sum(-1)) and torch.equal(part[sl['quarter'], :, 1].double(), (g * g).sum(-1))
        if C_ & (C_ - 1) == 0:       # 1 / C exact: var is exactly 0
            assert bool((var[sl['quarter']] == 0).all()) and bool((rstd[sl['quarter']] == float(np.float32(eps)) ** -0.5).all())
        assert float((rstd[sl['quarter']] - 1000.0).abs().max()) < 1e-3
        assert bool((xe[sl['const']].std(dim=-1) == 0).all())
        for v, s in zip(R.CONST_VALUES, var[sl['const']].tolist()):
            signs.setdefault(v, []).append(s)
            assert abs(s) < 64 * R.U * v * v, (v, C_, s)      # a few ulp of mean^2
        mean, _ = layernorm_stats(xe[sl['offset']], eps)
        ratio = mean.abs() / xe[sl['offset']].double().std(dim=-1, unbiased=False)
        assert bool((ratio > 99).all()) and bool((ratio < 101).all()), ratio
        assert bool(torch.isfinite(rstd).all()) and bool(torch.isfinite(nmr).all())
    assert min(signs[0.2]) < 0 < max(signs[0.2]), signs[0.2]
    every = [s for v in signs.values() for s in v]
    assert sum(s < 0 for s in every) >= 6 and sum(s > 0 for s in every) >= 6, signs


def test_fold_identity_and_consumer_inputs():
    """On the plain consumer's shapes: the folded form consumer_ref evaluates equals LN(x; gamma, beta) W~^T + b with W~ = r(gamma W) / gamma in fp64; the rows satisfy
    |mean| <= 2 std (what keeps T of the order of S in the bound) except the constant rows, whose reference is b + W beta; c = 2 + 6 K / 256."""
    eps = 1e-6
    for i, (M, N, K) in enumerate(R.CONSUMER_SHAPES):
        const_rows = 4 if i == 0 else 0
        x, gamma, beta, W, b = fold_inputs(M, 1, 1, K, N, n_regions=1, seed=300 + i, const_rows=const_rows)
        x, wg = _r(x), _r(W * gamma)
        mean, rstd = layernorm_stats(x, eps)
        std = x.double().std(dim=-1, unbiased=False)
        live = slice(0, M - const_rows)
        assert bool((mean[live].abs() <= 2 * std[live]).all())
        colsum, bf, _ = R.fold_pack_ref(W, gamma, beta, b, wg)
        y, A, S, T = R.consumer_ref(x, wg, colsum, bf, mean, rstd)
        wt = wg.double() / gamma.double()
        direct = torch.nn.functional.layer_norm(x.double(), (K,), gamma.double(), None, eps) @ wt.T + bf
        assert float((y - direct).abs().max() / direct.abs().max()) < 1e-11
        if const_rows:
            assert float((y[M - const_rows:] - bf[None, :]).abs().max()) < 1e-9
        assert bool((A >= y.abs() * (1 - 1e-12)).all())
        assert R.consumer_c(K) == 2 + 6 * K / 256


def test_fold_pack_reference():
    """fold_pack_ref: colsum is the sum of the ROUNDED operand (it differs from the sum of W gamma by what the 22-bit rounding leaves: visible, so a kernel that
    summed the unrounded product would be caught by the 1-ulp check wherever the two fp32 values differ -- asserted for some row of every shape), b' = b + W beta."""
    for i, (N, K) in enumerate(R.FOLD_PACK_SHAPES):
        W, gamma, beta, bias = R.fold_pack_inputs(N, K, 500 + i)
        wg = _r(W * gamma)
        colsum, bf, slack = R.fold_pack_ref(W, gamma, beta, bias, wg)
        unrounded = (W * gamma).double().sum(-1)
        apart = (colsum.float() != unrounded.float())
        assert bool(apart.any()), (N, K)
        assert float((bf - (bias.double() + W.double() @ beta.double())).abs().max()) < 1e-12 and bool((slack < 1e-12).all())


def test_chain_inputs_and_statistics_bound():
    """The chain's producer rows in fp64 have |mean| <= 2 std at ratio 0 and |mean| / std within 25 % of 10 / 100 otherwise; and chain_stat_bounds holds for the
    numpy restatement of the producer's tree (sums of the fp32 values BEFORE their split-fp16 rounding) + finalize_ref against the two-pass statistics of the rounded
    rows -- the derivation of k = 35, checked where no kernel is involved."""
    eps = 1e-6
    for C_ in R.CHAIN_C:
        for ratio in (0, 10, 100):
            act, Wp, bp, res, W2, gamma, beta, b2 = R.chain_inputs(333, 64, C_, 192, ratio, 900 + C_ + ratio)
            v64 = _r(act).double() @ _r(Wp).double().T + bp.double() + _r(res).double()
            mean, _ = layernorm_stats(v64, eps)
            q = mean.abs() / v64.std(dim=-1, unbiased=False)
            if ratio == 0:
                assert bool((q <= 2).all()), float(q.max())
            else:
                assert bool((q > 0.75 * ratio).all()) and bool((q < 1.25 * ratio).all()), (float(q.min()), float(q.max()))
            v = v64.float()
            xs = _r(v).double()
            rstd, nmr, _ = R.finalize_ref(R.producer_partials_emulated(v.numpy()), C_, eps)
            mean2, rstd2 = layernorm_stats(xs, eps)
            d_rstd, d_mean = R.chain_stat_bounds(xs)
            assert bool(((rstd / rstd2 - 1).abs() <= d_rstd).all()), float(((rstd / rstd2 - 1).abs() / d_rstd).max())
            assert bool(((-nmr / rstd - mean2).abs() <= d_mean).all())
    assert R.K_VAR == 35


def test_ln_entry_points_reject_bad_arguments():
    """Argument checks of the four entry points (host side: they return before any launch)."""
    from dust3r_amd import _lib
    lib = _lib.lib
    assert {'d3r_ln_finalize', 'd3r_ln_fold_pack', 'd3r_linear_ln', 'd3r_layernorm_x3rows'} <= set(_lib.EXPORTED)
    buf = (C.c_float * 64)()
    x3 = _lib.DTYPE_F16X3
    fin = lambda part=buf, rows=4, Cc=128, rstd=buf, nmr=buf: lib.d3r_ln_finalize(part, rows, Cc, 1e-6, rstd, nmr, None)      # noqa: E731
    assert fin(part=None) == -1 and fin(rstd=None) == -1 and fin(nmr=None) == -1 and fin(rows=0) == -1 and fin(Cc=48) == -1 and fin(Cc=2080) == -1 and fin(Cc=0) == -1
    pack = lambda W=buf, g=buf, b=buf, dst=buf, cs=buf, bo=buf, N=4, K=32, dt=x3: lib.d3r_ln_fold_pack(W, g, b, None, dst, cs, bo, N, K, dt, None)      # noqa: E731
    assert pack(W=None) == -1 and pack(g=None) == -1 and pack(b=None) == -1 and pack(dst=None) == -1 and pack(cs=None) == -1 and pack(bo=None) == -1
    assert pack(N=0) == -1 and pack(K=0) == -1 and pack(K=12) == -1
    for dt in (_lib.DTYPE_BF16, _lib.DTYPE_F16, _lib.DTYPE_F32, _lib.DTYPE_F16F8, _lib.DTYPE_F16X2F8, 9):      # split-fp16 is the only layout a fold engine packs
        assert pack(dt=dt) == -1
    lin = lambda act=buf, wgt=buf, out=buf, M=8, N=64, K=128, epi=0, rstd=buf, nmr=buf, cs=buf, part=None: \
        lib.d3r_linear_ln(act, wgt, None, out, M, N, K, epi, rstd, nmr, cs, part, 1e-6, None)      # noqa: E731
    assert lin(act=None) == -1 and lin(wgt=None) == -1 and lin(out=None) == -1 and lin(rstd=None) == -1 and lin(nmr=None) == -1 and lin(cs=None) == -1
    assert lin(M=0) == -1 and lin(N=60) == -1 and lin(K=0) == -1 and lin(epi=1) == -1 and lin(epi=3) == -1
    assert lin(part=buf, K=4096) == -1 and lin(part=buf, K=48) == -1
    ln = lambda rows=buf, g=buf, b=buf, out=buf, M=4, Cc=64: lib.d3r_layernorm_x3rows(rows, g, b, out, M, Cc, 1e-6, None)      # noqa: E731
    assert ln(rows=None) == -1 and ln(g=None) == -1 and ln(b=None) == -1 and ln(out=None) == -1 and ln(M=0) == -1 and ln(Cc=12) == -1 and ln(Cc=2056) == -1
