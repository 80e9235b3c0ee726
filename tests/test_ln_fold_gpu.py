"""The folded-LayerNorm chain of the default engine (csrc/kernels.hpp GemmParams::ln_*) at KERNEL level, one launch at a time, against plain fp64
(oracle/ln_fold_ref.py, pinned on the CPU by tests/test_ln_fold_cpu.py) on the SAME, already rounded, operands:

  a  d3r_ln_finalize                      test_ln_finalize               partial (sum, sum of squares) pairs -> rstd, -mean rstd; and the same statistics formed by a
                                                                         consumer GEMM's prologue (ln_row_stats<1 | 2 | 4>) bit for bit
  b  d3r_ln_fold_pack                     test_ln_fold_pack              W diag(gamma) in split-fp16 rows, colsum of the ROUNDED rows, b' = b + W beta
  c  d3r_linear_ln, one tile per block    test_plain_consumer            typed store and GELU, statistics passed in (route A) or formed by the launch (route B), every tile
                                                                         configuration, wide and direct epilogue
  d  d3r_linear_ln, persistent kernel     test_persistent_consumer       gemm_p4.hip with has_ln, against the one-tile-per-block kernels
  e  d3r_layernorm_x3rows                 test_layernorm_x3rows          enc_norm / dec_norm: LayerNorm from split-fp16 rows into split-fp16 rows
  f  producer -> finalize -> consumer     test_chain_on_real_buffers     the only place where the producer's fp32 sums of squares meet a true variance

Every bound is computed per element from reference quantities and reported as "largest share of the bound"; every output array is pre-filled with a sentinel and has a
guard band on both sides. d3r_gemm_tile_config is asked before every pinned launch: an arm whose pin the dispatch ignores is reported with the reason and not run, and no
configuration may be ignored for every shape.

Single-line mutations and the test that fails on each (the first three were built and run once on an MI355X: 9, 10 and 4 of the 36 cases failed; the rest by reading):
  nmr with the wrong sign (ln_finalize_kernel or ln_row_stats)          a (2 ulp of fp64; route B against ln_finalize bit for bit), c route B, f
  colsum taken from the unrounded W gamma (ln_fold_vectors_kernel)      b only (1 ulp of the fp64 sum of the decoded rows: 7 ... 1600 ulp off -- relative to sum |w| still 1e-7, so inside every output bound)
  the g + 32 pair dropped in ln_finalize_kernel                         a at C = 1056 / 2048 (2 ulp; bit equality with route B), f at C = 1056 / 2048
  the same in ln_row_stats<TPR> for one TPR                             a (bit equality with ln_finalize on that TPR's tile), c route B at K = 2048
  kscale[c] indexed by the row, or the pack skipping kscale              b (rows bitwise against pack_x3(W * gamma))
  fma(acc, rstd, fma(colsum, nmr, b)) with rstd / nmr of another row     c, d (per-element bound; rows differ in mean and spread)
  colsum of another column in one epilogue (direct, wide or persistent)  c NOWIDE 0 / 1, d
  a statistic or an output element written past M / M x N               the sentinel checks
"""
import pytest
import torch
import torch.nn.functional as F

from oracle import ln_fold_ref as R
from oracle.heads_ref import fold_inputs, layernorm_stats
from test_ln_fold_cpu import TILE_TPR

pytestmark = pytest.mark.gpu

EPS = 1e-6
GUARD = 256                 # elements of sentinel before and after every destination
SENT = -7.5                 # exact in fp16; a split-fp16 element left alone decodes to -15
STAT_SENT = 1.0e30
CFGS = ['0', '0w8', '1', '2', '3', '7', '8', '9', '11']      # test_linear_split_fp16's
TPR_TILE = {1: '7', 2: '0', 4: '8'}                           # one tile per threads-per-row value of the consumer's prologue (TILE_TPR)
EPI_CODE = {'store': 0, 'gelu': 2}

_cache = {}


def _say(line):
    print(line)


def _pin(monkeypatch, cfg):
    if cfg is None:
        monkeypatch.delenv('D3R_GEMM_CFG', raising=False)
        monkeypatch.delenv('D3R_GEMM_T128W8', raising=False)
        return
    monkeypatch.setenv('D3R_GEMM_CFG', cfg[:-2] if cfg.endswith('w8') else cfg)
    monkeypatch.setenv('D3R_GEMM_T128W8', '1000000' if cfg.endswith('w8') else '0')      # eight waves for every 128 x 128 launch, or for none


def _tile(M, N, K, epi):
    """the tile configuration gemm_plan answers for this launch under the current environment (the ln_* fields of a route-A launch do not enter the plan; ln_part_in
    only keeps a launch off the persistent kernel, which a pinned configuration does as well)"""
    from dust3r_amd._lib import DTYPE_F16X3, lib
    return lib.d3r_gemm_tile_config(DTYPE_F16X3, M, N, K, EPI_CODE[epi], 0)


def pin_infeasible(cfg, N):
    """None when gemm_plan (gemm_plan.hpp) lets a plain split-fp16 nn.Linear launch of N columns take the pinned configuration, else the reason"""
    if cfg == '9' and (N + 191) // 192 * 192 > (N + 255) // 256 * 256:
        return f'N = {N}: whole 192-column tiles would read past the round_up(N, 256) weight rows the loader allocates'
    return None


def _r(x):
    from dust3r_amd import ops
    return ops.unpack_x3(ops.pack_x3(x))


def _bits(t):
    return t.view({2: torch.int16, 4: torch.int32}[t.element_size()])


class _Out:
    """an fp16 destination of n elements between two guard bands, everything pre-filled with the sentinel"""

    def __init__(self, dev, n):
        self.n, self.g = n, 2 * GUARD
        self.buf = torch.full((self.g + n + self.g,), SENT, dtype=torch.float16, device=dev)
        self.sent = int(_bits(torch.full((1,), SENT, dtype=torch.float16))[0])

    def arg(self):
        return self.buf[self.g:]

    def raw(self, what):
        bits = _bits(self.buf)
        assert bool((bits[:self.g] == self.sent).all()), f'{what}: the guard band BEFORE the destination was written'
        assert bool((bits[self.g + self.n:] == self.sent).all()), f'{what}: the guard band AFTER the destination was written'
        return bits[self.g:self.g + self.n].clone()


def _stats_buf(dev, M):
    return torch.full((2, M + GUARD), STAT_SENT, dtype=torch.float32, device=dev)


def _consume(dev, act_rows, wrows, bias, N, epi, rstd, nmr, colsum, part_in, what):
    """one d3r_linear_ln launch into a guarded destination -> the stored rows as int16 (M, 2 N)"""
    from dust3r_amd import ops
    M = act_rows.shape[0]
    dst = _Out(dev, M * 2 * N)
    ops.linear_ln(act_rows, wrows, bias, N, epi, rstd, nmr, colsum, part_in=part_in, eps=EPS, out=dst.arg())
    torch.cuda.synchronize()
    return dst.raw(what).view(M, 2 * N)


def _decode(raw):
    from dust3r_amd import ops
    return ops.unpack_x3(raw.view(torch.float16)).double()


def _ulps(got, ref):
    return float(((got.double() - ref).abs() / R.ulp32(ref)).max())


# ------------------------------------------------------------------------------------------------------------------------------------------ a
def _finalize_case(dev, C, x, wrows, colsum, what, monkeypatch, edge=None):
    from dust3r_amd import ops
    rows = x.shape[0]
    x = _r(x)
    part = R.partials(x).to(dev)                     # fp32, summed on the host side of the launch
    rstd_ref, nmr_ref, var_ref = R.finalize_ref(part, C, EPS)
    st = _stats_buf(dev, rows)
    ops.ln_finalize(part, C, EPS, rstd=st[0], nmr=st[1])
    torch.cuda.synchronize()
    assert bool((st[:, rows:] == STAT_SENT).all()), f'{what}: ln_finalize wrote past row {rows}'
    assert bool(torch.isfinite(st[:, :rows]).all()), what
    ur, un = _ulps(st[0, :rows], rstd_ref), _ulps(st[1, :rows], nmr_ref)
    line = f'{what}: ln_finalize, ulp from fp64: rstd {ur:.2f} nmr {un:.2f} (bound 2)'
    assert ur <= 2.0 and un <= 2.0, line
    if edge is not None:
        q = st[0, :rows][edge['quarter']]
        assert float((q - 1000.0).abs().max()) < 1e-3, f'{what}: constant rows: rstd {q.tolist()} is not 1 / sqrt(eps)'
        neg = int((var_ref[edge['const']] < 0).sum())
        line += f'; constant rows: {neg} of {len(R.CONST_VALUES)} with q / C - mean^2 < 0 (clamped)'
    # route B: the same statistics formed by a consumer GEMM's prologue, one tile per threads-per-row value -- bit for bit ("EXACTLY the arithmetic", kernels.hpp)
    xr = ops.pack_x3(x).to(dev)
    N = 192
    for tpr, cfg in TPR_TILE.items():
        _pin(monkeypatch, cfg)
        assert TILE_TPR[cfg] == tpr and _tile(rows, N, C, 'store') == int(cfg), f'{what}: tile {cfg} (TPR {tpr}) was not taken'
        sb = _stats_buf(dev, rows)
        _consume(dev, xr, wrows, None, N, 'store', sb[0], sb[1], colsum, part, f'{what} route B tile {cfg}')
        assert bool((sb[:, rows:] == STAT_SENT).all()), f'{what}: route B on tile {cfg} wrote statistics past row {rows}'
        for name, a, b in (('rstd', sb[0, :rows], st[0, :rows]), ('nmr', sb[1, :rows], st[1, :rows])):
            nd = int((_bits(a) != _bits(b)).sum())
            assert nd == 0, f'{what}: {name} of route B on tile {cfg} (TPR {tpr}) differs from ln_finalize in {nd} of {rows} rows'
    _say(line + '; route B on tiles 7 / 0 / 8 (TPR 1 / 2 / 4): bitwise equal')
    return max(ur, un)


@pytest.mark.parametrize('C', R.FINALIZE_C)
def test_ln_finalize(gpu, C, monkeypatch):
    """d3r_ln_finalize alone, G = C / 32 = 1, 4, 24, 32, 33, 64 pairs per row (lanes g < G only; the g + 32 pair on one lane; on all), rows = 1, 7, 8, 9, 1001 (eight rows
    per block: a partial last block and its clamped row) of real random rows, and the edge rows of oracle/ln_fold_ref.py finalize_edge_rows: constant rows with exact
    partials (rstd = 1 / sqrt(eps) to 1e-3, finite), constant rows whose fp32 partials leave q / C - mean^2 a few ulp either side of zero (the clamp; 11.7 and 29.0 would
    give the root a negative argument without it), rows with |mean| = 100 std.
    rstd and nmr within 2 ulp of the fp64 evaluation of the kernel's OWN fp32 inputs -- the pairs, eps, and the factor 1 / C as the fp32 quotient the launch forms (rstd: fp64
    arithmetic and one rounding; nmr = fp32(-mean) x rstd: three roundings, at most 2 ulp of the product: with significands a, b in [1, 2) the three half-ulps weigh
    (a + b + 1) / 2 <= 2 where a b < 2 and (a + b + 2) / 4 <= 1.5 otherwise); nothing written past `rows`.
    For each case route B of d3r_linear_ln runs on the same pairs on tiles 7, 0 and 8 -- 1, 2 and 4 threads per row (tests/test_ln_fold_cpu.py reads that off gemm.hip's tile
    table) -- and the rstd / nmr it writes must equal ln_finalize's bit for bit: the claim of kernels.hpp (ln_row_stats) that no test held for one thread per row."""
    from dust3r_amd import ops
    monkeypatch.delenv('D3R_GEMM_NOWIDE', raising=False)
    monkeypatch.delenv('D3R_GEMM_PERSIST', raising=False)
    g = torch.Generator(device='cpu').manual_seed(C)
    W = torch.randn((192, C), generator=g) / C ** 0.5
    wrows, colsum = ops.pad_rows(ops.pack_x3(W)).to(gpu), ops.pad_rows(W.sum(-1)).to(gpu)
    worst = 0.0
    for rows in R.FINALIZE_ROWS:
        worst = max(worst, _finalize_case(gpu, C, R.finalize_rows(rows, C, 1000 * C + rows), wrows, colsum, f'C {C} rows {rows}', monkeypatch))
    xe, sl = R.finalize_edge_rows(C, 7 * C)
    worst = max(worst, _finalize_case(gpu, C, xe, wrows, colsum, f'C {C} edge rows', monkeypatch, edge=sl))
    _say(f'ln_finalize C {C}: largest share of the bound (2 ulp): {worst / 2:.3f}')


# ------------------------------------------------------------------------------------------------------------------------------------------ b
@pytest.mark.parametrize('with_bias', [True, False])
@pytest.mark.parametrize('N,K', R.FOLD_PACK_SHAPES)
def test_ln_fold_pack(gpu, N, K, with_bias):
    """d3r_ln_fold_pack = the two launches finalize_fold (engine.hip) makes for one matrix, through the engine's own function. (N, K): N no multiple of the four rows per
    block (6, 130), K below one lane stride with idle lanes (32), K no multiple of 64 (32, 96), the engine's widths (1024, 2048); with and without bias_in.
      rows      bitwise those of ops.pack_x3(W * gamma): the fp32 product is the same IEEE multiply on both sides; rows >= N stay zero
      colsum    within 1 ulp of fp32(sum_k, in fp64, of the DECODED packed row): the sum of the rounded operand is what the fold identity needs, not sum_k gamma_k W_nk
      bias_out  within 1 ulp + K 2^-53 sum_k |beta_k W_nk| of b + W beta in fp64; elements >= N of both vectors untouched"""
    from dust3r_amd import ops
    W, gamma, beta, bias = [t.to(gpu) for t in R.fold_pack_inputs(N, K, 500 + R.FOLD_PACK_SHAPES.index((N, K)))]
    bias = bias if with_bias else None
    rows, colsum, bfold = ops.ln_fold_pack(W, gamma, beta, bias)
    torch.cuda.synchronize()
    want = ops.pack_x3(W * gamma)
    nd = int((_bits(rows[:N]) != _bits(want)).sum())
    assert nd == 0, f'({N}, {K}): {nd} of {want.numel()} storage elements differ from pack_x3(W * gamma)'
    assert int((_bits(rows[N:]) != 0).sum()) == 0, f'({N}, {K}): a row >= N was written'
    assert int((_bits(colsum[N:]) != 0).sum()) == 0 and int((_bits(bfold[N:]) != 0).sum()) == 0, f'({N}, {K}): colsum / bias_out written past N'
    cs_ref, bf_ref, slack = R.fold_pack_ref(W, gamma, beta, bias, ops.unpack_x3(rows[:N]))
    uc = _ulps(colsum[:N], cs_ref)
    ub = float((((bfold[:N].double() - bf_ref).abs() - slack).clamp_min(0) / R.ulp32(bf_ref)).max())
    unrounded = int((colsum[:N] != (W * gamma).double().sum(-1).float()).sum())
    _say(f'ln_fold_pack ({N}, {K}){"" if with_bias else " no bias"}: rows bitwise; ulp from fp64: colsum {uc:.2f} bias_out {ub:.2f} (bound 1); largest share of the bound '
         f'{max(uc, ub):.3f}; colsum differs from fp32(sum of the UNROUNDED W gamma) in {unrounded} of {N} rows')
    assert uc <= 1.0 and ub <= 1.0


# ------------------------------------------------------------------------------------------------------------------------------------------ c
def _consumer_case(dev, M, N, K, seed, const_rows=0):
    """inputs and fp64 references of one plain consumer shape, built once and shared by every arm"""
    key = ('case', M, N, K, seed)
    if key not in _cache:
        from dust3r_amd import ops
        x, gamma, beta, W, b = fold_inputs(M, 1, 1, K, N, n_regions=1, seed=seed, const_rows=const_rows)
        x, wg = _r(x).to(dev), _r(W * gamma).to(dev)      # the rows and the weights the kernel reads, exactly
        colsum, bf, _ = R.fold_pack_ref(W.to(dev), gamma.to(dev), beta.to(dev), b.to(dev), wg)
        mean, rstd = layernorm_stats(x, EPS)
        assert bool(torch.isfinite(rstd).all())
        y, A, S, T = R.consumer_ref(x, wg, colsum, bf, mean, rstd)
        c = R.consumer_c(K)
        e_torch = R.gelu_torch_error(y)
        part = R.partials(x.cpu()).to(dev)
        rstd_b, nmr_b, _ = R.finalize_ref(part, K, EPS)
        g = torch.Generator(device='cpu').manual_seed(seed + 1)
        _cache[key] = dict(
            x=x, wg=wg, xr=ops.pack_x3(x), wrows=ops.pad_rows(ops.pack_x3(wg)), bias=ops.pad_rows(bf.float()), colsum=ops.pad_rows(colsum.float()),
            rstd=rstd.float(), nmr=(-mean * rstd).float(), part=part, rstd_b=rstd_b, nmr_b=nmr_b, c=c, e_torch=e_torch,
            ref={'store': y, 'gelu': R.gelu64(y)},
            bound={'store': c * 2.0 ** -21 * A, 'gelu': R.GELU_SLOPE * c * 2.0 ** -21 * A + 4 * e_torch},
            any_colsum=ops.pad_rows(3.0 * torch.randn(N, generator=g)).to(dev), ones=torch.ones(M, device=dev), zeros=torch.zeros(M, device=dev), const_rows=const_rows)
    return _cache[key]


@pytest.mark.parametrize('cfg', CFGS)
def test_plain_consumer(gpu, cfg, monkeypatch):
    """The plain consumer (EPI_T `store`, EPI_GELU `gelu`: fc1 + GELU and the cross-attention projections of the engine) under one pinned tile configuration, with
    D3R_GEMM_NOWIDE 0 (LDS-staged wide epilogue) and 1 (direct stores), on (M, N, K) = (300, 192, 256) -- its last 4 rows constant --, (77, 96, 768), (515, 328, 64),
    (1000, 384, 1024), (130, 256, 2048).
    Reference (oracle/ln_fold_ref.py consumer_ref): fp64 y = rstd_m (sum_k x_mk wg_nk - mean_m colsum_n) + b'_n on exactly the operands the kernel reads.
      store   |out - y| <= c 2^-21 A, A = rstd sum |x wg| + |colsum nmr| + |b'|, c = 2 + 6 K / 256 -- the bound of test_heads_folded_layernorm_consumer with its rotation and
              table terms dropped: 0.5 (lo.lo products) + 6 K / 256 (fp32 accumulation) on S, 0.625 (the two fmas on fp32-rounded operands) + 0.5 (split-fp16 store) on A
      gelu    |out - gelu(y)| <= 1.13 c 2^-21 A + 4 E, 1.13 = max |gelu'| (the store's 2^-22 |gelu(y)| <= 2^-22 A is inside the first term), E = max |F.gelu(fp32) - F.gelu(fp64)|
              of torch on the same pre-activations: the error of an fp32 erf evaluation is the one number that cannot be derived; it is measured on torch, not on the kernel,
              and the kernel -- another approximation of the same precision class -- is allowed 4 x. Measured on MI355X: E = 3.6e-7 ... 4.5e-7 over the five shapes (half an
              fp32 ulp of the largest pre-activations, |y| up to 8); the kernel's own distance |gelu_out - gelu64(its stored pre-activation)| 1.2e-6 ... 1.4e-6, which is the
              2^-22 |gelu| of its split-fp16 store at those |y| and sits in the first term, not in 4 E.
      plumbing, independent of E: a launch with rstd = 1, nmr = 0 and an arbitrary finite colsum is bitwise ops.linear_x3 on the same operands, `store` and `gelu`
              (kernels.hpp: fma(acc, 1, fma(s, 0, b)) = acc + b)
      route B: the statistics the launch wrote are within 2 ulp of the fp64 evaluation of its inputs, nothing past M; its output is bitwise that of a route-A launch fed them
      wide and direct epilogue: BITWISE equal, `store` and `gelu` (both write fma(acc, rstd, fma(colsum, nmr, b')) with explicit fmas and call the same gelu4; there is no
              rotation here whose contraction could differ, so the 1e-6 allowance of the heads test does not apply), and bitwise equal across tile configurations
              (the MFMA order per output element does not depend on the tile).
    A pin the dispatch ignores is reported with the reason (only 9 at N = 256: 2 x 192 columns > the 256 weight rows) and asserted to be ignored for exactly that reason."""
    from dust3r_amd import ops
    monkeypatch.delenv('D3R_GEMM_PERSIST', raising=False)
    _pin(monkeypatch, cfg)
    code = int(cfg[:-2]) if cfg.endswith('w8') else int(cfg)
    taken, worst = 0, {'store': 0.0, 'gelu': 0.0}
    for si, (M, N, K) in enumerate(R.CONSUMER_SHAPES):
        cs = _consumer_case(gpu, M, N, K, 300 + si, const_rows=4 if si == 0 else 0)
        for nowide in ('0', '1'):
            monkeypatch.setenv('D3R_GEMM_NOWIDE', nowide)
            for epi in ('store', 'gelu'):
                what = f'cfg {cfg} NOWIDE {nowide} ({M}, {N}, {K}) {epi}'
                got, why = _tile(M, N, K, epi), pin_infeasible(cfg, N)
                if why is not None:
                    assert got != code, f'{what}: taken although: {why}'
                    if nowide == '0' and epi == 'store':
                        _say(f'cfg {cfg} ({M}, {N}, {K}): skipped (runs tile {got}): {why}')
                    continue
                assert got == code, f'{what}: the pin was ignored (runs tile {got}) for a reason the stated rules do not name'
                taken += 1
                # route A
                raw_a = _consume(gpu, cs['xr'], cs['wrows'], cs['bias'], N, epi, cs['rstd'], cs['nmr'], cs['colsum'], None, what + ' A')
                out = _decode(raw_a)
                assert bool(torch.isfinite(out).all()), what
                share = float(((out - cs['ref'][epi]).abs() / cs['bound'][epi]).max())
                worst[epi] = max(worst[epi], share)
                line = f'{what}: tile {got}; route A, largest share of the bound (c = {cs["c"]:g}) {share:.3f}'
                if epi == 'gelu':
                    pre = _cache[('first', M, N, K, 'store')][1]
                    own = float((out - R.gelu64(_decode(pre))).abs().max())
                    line += f'; erf: torch fp32 E = {cs["e_torch"]:.2e} (allowed 4 E), kernel |gelu_out - gelu64(stored pre-activation)| = {own:.2e}'
                assert share <= 1.0, line
                if cs['const_rows']:
                    assert share <= 1.0 and bool(torch.isfinite(out[M - cs['const_rows']:]).all())
                # bitwise across tile configurations and across the two epilogue routes
                first = _cache.setdefault(('first', M, N, K, epi), (f'{cfg} NOWIDE {nowide}', raw_a))
                nd = int((first[1] != raw_a).sum())
                assert nd == 0, f'{what}: {nd} of {raw_a.numel()} storage elements differ from configuration {first[0]}'
                # plumbing: (rstd, nmr) = (1, 0) and any colsum is the plain nn.Linear, bit for bit
                raw_p = _consume(gpu, cs['xr'], cs['wrows'], cs['bias'], N, epi, cs['ones'], cs['zeros'], cs['any_colsum'], None, what + ' (1, 0, any)')
                lin = ops.linear_x3(cs['x'], cs['wg'], cs['bias'][:N], epi)
                assert torch.equal(ops.unpack_x3(raw_p.view(torch.float16)), lin), f'{what}: rstd = 1, nmr = 0 is not ops.linear_x3 bit for bit'
                # route B
                st = _stats_buf(gpu, M)
                raw_b = _consume(gpu, cs['xr'], cs['wrows'], cs['bias'], N, epi, st[0], st[1], cs['colsum'], cs['part'], what + ' B')
                assert bool((st[:, M:] == STAT_SENT).all()), f'{what}: statistics written past row M'
                ur, un = _ulps(st[0, :M], cs['rstd_b']), _ulps(st[1, :M], cs['nmr_b'])
                assert ur <= 2.0 and un <= 2.0, f'{what}: route B statistics {ur:.2f} / {un:.2f} ulp from fp64'
                raw_a2 = _consume(gpu, cs['xr'], cs['wrows'], cs['bias'], N, epi, st[0, :M].clone(), st[1, :M].clone(), cs['colsum'], None, what + " A'")
                assert torch.equal(raw_b, raw_a2), f'{what}: route B differs from route A fed the statistics it wrote'
                _say(line + f'; route B statistics {ur:.2f} / {un:.2f} ulp from fp64, output bitwise route A on them')
    _say(f'plain consumer cfg {cfg}: {taken} arms taken; largest share of the bound: store {worst["store"]:.3f} gelu {worst["gelu"]:.3f}')
    assert taken >= 16, f'configuration {cfg} was taken for {taken} arms only'


# ------------------------------------------------------------------------------------------------------------------------------------------ d
@pytest.mark.parametrize('M,N,K', [(2048, 256, 768), (2048, 128, 576), (6144, 4096, 576)])
def test_persistent_consumer(gpu, M, N, K, monkeypatch):
    """The consumer on the persistent kernel (gemm_p4.hip, has_ln): what fc1 + GELU of the 32-pair step runs. (2048, 256, 768) and (2048, 128, 576) are the smallest
    problems the kernel takes (whole 256 x 128 tiles, >= 18 K steps, >= 8 tiles: one tile per block); (6144, 4096, 576) is 768 tiles on 256 resident blocks: first,
    overlapped and last tile. Route-A statistics (the kernel declines ln_part_in), `store` and `gelu`, D3R_GEMM_PERSIST=1 against 0: d3r_gemm_tile_config must answer 10 and
    not 10, the outputs must be BITWISE identical and both within the plain consumer's bound (test_plain_consumer)."""
    monkeypatch.delenv('D3R_GEMM_NOWIDE', raising=False)
    _pin(monkeypatch, None)
    cs = _consumer_case(gpu, M, N, K, 700 + K + N)
    raws = {}
    for mode in ('1', '0'):
        monkeypatch.setenv('D3R_GEMM_PERSIST', mode)
        for epi in ('store', 'gelu'):
            what = f'persistent consumer ({M}, {N}, {K}) {epi} PERSIST {mode}'
            got = _tile(M, N, K, epi)
            assert (got == 10) == (mode == '1'), f'{what}: runs tile {got}'
            raw = _consume(gpu, cs['xr'], cs['wrows'], cs['bias'], N, epi, cs['rstd'], cs['nmr'], cs['colsum'], None, what)
            share = float(((_decode(raw) - cs['ref'][epi]).abs() / cs['bound'][epi]).max())
            _say(f'{what}: tile {got}; largest share of the bound (c = {cs["c"]:g}) {share:.3f}')
            assert share <= 1.0, what
            raws[(mode, epi)] = raw
    for epi in ('store', 'gelu'):
        nd = int((raws[('1', epi)] != raws[('0', epi)]).sum())
        assert nd == 0, f'({M}, {N}, {K}) {epi}: {nd} storage elements differ between the persistent and the one-tile-per-block kernel'
    _cache.pop(('case', M, N, K, 700 + K + N))


# ------------------------------------------------------------------------------------------------------------------------------------------ e
@pytest.mark.parametrize('rows,C', [(7, 128), (513, 1024), (33, 1032), (5, 2048), (9, 16)])
def test_layernorm_x3rows(gpu, rows, C):
    """layernorm_kernel<F16X3, X3IN = true> (enc_norm / dec_norm of the default engine): split-fp16 rows in, split-fp16 rows out, within 2e-6 of the fp64 LayerNorm of the
    DECODED rows relative to the output maximum -- test_layernorm_split_fp16_rows' bar: the same kernel body behind another load. Whether it is bitwise
    ops.layernorm_x3 on the decoded fp32 rows is printed, not asserted (the two instances may contract differently). Nothing outside the rows x C destination is written."""
    from dust3r_amd import ops
    g = torch.Generator(device='cpu').manual_seed(rows * 3 + C)
    x = _r(torch.randn((rows, C), generator=g) * 3 + 0.5).to(gpu)
    gamma, beta = (1 + 0.1 * torch.randn(C, generator=g)).to(gpu), (0.1 * torch.randn(C, generator=g)).to(gpu)
    ref = F.layer_norm(x.double(), (C,), gamma.double(), beta.double(), eps=EPS)
    dst = _Out(gpu, rows * 2 * C)
    ops.layernorm_x3rows(ops.pack_x3(x), gamma, beta, EPS, out=dst.arg())
    torch.cuda.synchronize()
    out = ops.unpack_x3(dst.raw(f'layernorm_x3rows ({rows}, {C})').view(rows, 2 * C).view(torch.float16))
    err = float((out.double() - ref).abs().max() / ref.abs().max())
    same = torch.equal(out, ops.layernorm_x3(x, gamma, beta, eps=EPS))
    _say(f'layernorm_x3rows ({rows}, {C}): err {err:.2e} / 2e-06, largest share of the bound {err / 2e-6:.3f}; {"bitwise equal to" if same else "NOT bitwise"} ops.layernorm_x3 '
         f'on the decoded rows')
    assert err < 2e-6


# ------------------------------------------------------------------------------------------------------------------------------------------ f
@pytest.mark.parametrize('C', R.CHAIN_C)
def test_chain_on_real_buffers(gpu, C, monkeypatch):
    """ops.linear_x3res(with_sums) -> d3r_ln_finalize -> d3r_ln_fold_pack'd weights -> d3r_linear_ln(store) on the buffers the launches hand each other, hidden width
    C = 256, 1056, 2048 (G = 8, 33, 64), M = 333, against fp64 (oracle/ln_fold_ref.py chain_ref)
        y = LN_two-pass(xs) W~^T + b',   xs = the DECODED stored rows,  W~_nk = decoded packed row n, element k, / gamma_k,  b' = b + W beta
          = rstd (xs wg^T - mean colsum) + b' with the two-pass mean / rstd of xs.
    Bound per element = the plain consumer's c 2^-21 A + the statistics term d_rstd (S + T) + rstd |colsum| d_mean (1 + d_rstd) (chain_stat_bounds): the producer sums the
    fp32 values BEFORE their split-fp16 rounding (4 U relative on x, 8 U on x^2), a sum passes 5 additions, a sum of squares a product and 5 additions, 1 / C is an fp32
    quotient: |d mean| <= 10 U E|x|, |d E x^2| <= 15 U E x^2, so the relative error of rstd is <= k / 2 U (1 + mean^2 / var) with k = 15 + 2 x 10 = 35 (to first order; the
    test uses (1 - e)^-1/2 - 1 with e = k U (1 + mean^2 / var)), + U for its rounding. The CPU test checks this derivation on a numpy restatement of the producer's tree.
    Run 1: |mean| <= 2 std on every stored row (asserted on the host): the bound holds AND the distance to the two-pass reference is below 1e-5 of the output maximum -- two
    orders inside the engine's 1e-3 bar, the meaning given here to "by orders of magnitude". Run 2: |mean| / std = 10 and 100: only the derived bound is asserted; the
    distances are printed for DESIGN.md 4.0. Measured on MI355X, max |out - two-pass| / max |y| (largest share of the bound) at C = 256 / 1056 / 2048: ratio <= 2:
    3.5e-7 / 6.2e-7 / 1.4e-6 (0.035 / 0.010 / 0.008); ratio 10: 2.8e-6 / 5.3e-6 / 5.7e-6 (0.001); ratio 100: 1.8e-4 / 2.0e-4 / 9.3e-5 (< 0.001), rstd 1.3e-4 ... 4.0e-4
    from the two-pass value against a bound of 1.1e-2 ... 1.3e-2. Route B on the same buffers is bitwise ln_finalize + route A."""
    from dust3r_amd import ops
    monkeypatch.delenv('D3R_GEMM_NOWIDE', raising=False)
    monkeypatch.delenv('D3R_GEMM_PERSIST', raising=False)
    _pin(monkeypatch, None)
    M, Kp, N2 = 333, 64, 192
    for ratio in (0, 10, 100):
        act, Wp, bp, res, W2, gamma, beta, b2 = [t.to(gpu) for t in R.chain_inputs(M, Kp, C, N2, ratio, 900 + C + ratio)]
        rows32, part, rows_raw = ops.linear_x3res(_r(act), _r(Wp), bp, _r(res), with_sums=True)
        st = _stats_buf(gpu, M)
        ops.ln_finalize(part, C, EPS, rstd=st[0], nmr=st[1])
        wrows, colsum, bfold = ops.ln_fold_pack(W2, gamma, beta, b2)
        what = f'chain C {C} |mean| / std ~ {ratio}'
        raw = _consume(gpu, rows_raw, wrows, bfold, N2, 'store', st[0], st[1], colsum, None, what)
        assert bool((st[:, M:] == STAT_SENT).all())
        xs = rows32.double()
        y, bound, mean, rstd = R.chain_ref(xs, ops.unpack_x3(wrows[:N2]), W2, gamma, beta, b2, EPS)
        q = (mean.abs() * rstd).cpu()                                   # |mean| / sqrt(var + eps)
        if ratio == 0:
            assert bool((q <= 2).all()), f'{what}: input condition |mean| <= 2 std violated: {float(q.max()):.2f}'
        out = _decode(raw)
        share = float(((out - y).abs() / bound).max())
        dist = float((out - y).abs().max() / y.abs().max())
        d_rstd = float((st[0, :M].double() / rstd - 1).abs().max())
        d_rstd_bound = float(R.chain_stat_bounds(xs)[0].max())
        _say(f'{what} (measured {float(q.min()):.1f} .. {float(q.max()):.1f}): largest share of the bound {share:.3f}; max |out - two-pass| / max |y| = {dist:.2e}; '
             f'rstd: max relative distance from two-pass {d_rstd:.2e} (bound {d_rstd_bound:.2e}, k = {R.K_VAR})')
        assert share <= 1.0, what
        if ratio == 0:
            assert dist < 1e-5, what
        sb = _stats_buf(gpu, M)
        raw_b = _consume(gpu, rows_raw, wrows, bfold, N2, 'store', sb[0], sb[1], colsum, part, what + ' route B')
        assert torch.equal(_bits(sb[:, :M]), _bits(st[:, :M])) and torch.equal(raw_b, raw), f'{what}: route B differs from ln_finalize + route A'
