"""The attention-projection GEMM epilogue (EPI_HEADS of csrc/gemm.hip: bias, folded-LayerNorm correction, 2-D RoPE, scatter into [B][H][ntok][64] /
[B][H][64][ldv]) at KERNEL level, one launch at a time through d3r_linear_heads, against plain fp64 (oracle/heads_ref.py, pinned on the CPU by
tests/test_gemm_heads_cpu.py against nn.Linear + reshape + croco's RoPE2D) on the SAME, already rounded, operands.

Routes and the smallest shape (B, th, tw) that reaches each:
  direct stores, q / k                       every dtype at ntok % 32 != 0 (split-fp16 / fp8), fp32 always, every dtype under D3R_GEMM_NOWIDE=1
  operand-role swap, store4                  (5, 4, 6): ntok % 4 == 0
  operand-role swap, per-token scalar stores (50, 2, 3) and (7, 3, 5): four tokens straddle an image boundary
  wide 16-bit staging tile, q / k            bf16 / fp16, every shape (V^T blocks of ntok % 64 != 0 launches still swap and store directly)
  LDS-transposed V^T (vt_wide)               bf16 / fp16 at (2, 8, 8): ntok % 64 == 0; the only route the non-square tiles 2 / 3 can take
  wide split-fp16 staging tile (+ swap)      split-fp16 / fp8 modes at (3, 8, 12), (2, 8, 8), (1, 21, 32): ntok % 32 == 0
Every value bound is the one tests/test_kernels_gpu.py uses for the same dtype's typed store, relative to max |ref| of the REGION (a wrong V^T cannot
hide under a larger q): OUT_TOL for bf16 / fp16, 2e-5 fp32, 3e-6 split-fp16; the fp8 modes are held to 3e-6 against the fp64 emulation of their
contraction (oracle/f8_ref.py) like the fp32 outputs of test_linear_fp16_fp8 / test_linear_2p5_unit, because their heads are split-fp16 rows (22 bits),
not fp16 + fp8 activation rows. The reference rotates with the EXACT angles; the kernel's table is within pos inv_freq 2^-23 + 2^-24 of them
(test_rope_table), which is inside every one of these bounds' budget only because positions stay <= 31 here.

Single-line mutations of gemm.hip and the test that fails on each (the first six were also built and run once; the rest by reading):
  load_rope_half reads tx for the y half (wide split-fp16 route)        test_heads_layout_and_values fp16x3 / fp16f8 / fp16x2f8, fold, split-K
  `pos = half ? ty : tx` in the direct epilogue                         ... every dtype's direct arms (fp32 all; others at ntok % 32 != 0, NOWIDE), fold
  load_rope_rows hands the x rows to the y pairs (wide 16-bit route)    ... bf16 / fp16, every configuration
  V^T quads not split at an image boundary (`t + 3 < ntok` dropped)     ... every dtype at (50,2,3) / (7,3,5): values AND the pad-column sentinel
  colsum of the `+ 16` half taken from the first half (direct route)    test_heads_folded_layernorm_consumer only ((50,2,3): the direct fold route)
  `b * heads + h` with another head count in a V^T store                ... every launch with B > 1 on that route (values; region scales differ)
  bias added after the rotation                                         values of every rotated region: the bias differs per column, so it does not commute
  regions exchanged / head_c misread                                    values: the regions' weights differ in scale by 2x
  a pad column [ntok, ldv) or an element past a destination written     the sentinel checks (pads, 256-element guard bands on both sides)
  ty / tx exchanged everywhere                                          values at th != tw (all shapes but (2,8,8) and (2,14,14))
Unobservable here: the store policy (non-temporal or not), the clamped dummy reads of absent operands, the `swap && ntok % 64 == 0` arm of the wide 16-bit
read phase (dead: a swapped block never takes that epilogue), one thread per row in the in-kernel statistics (tiles no heads launch takes), and anything
that needs positions above 31 or a table other than base 100 under the GEMM (the table itself is pinned to 512 rows and two bases).
"""
import math

import numpy as np
import pytest
import torch

from oracle.heads_ref import fold_inputs, heads_ref, layernorm_stats, rope_angles, rope_table_bound, rope_table_emulated, scatter_heads
from test_kernels_gpu import OUT_TOL

pytestmark = pytest.mark.gpu

BASE = 100.0
GUARD = 256                 # elements of sentinel before and after every destination
SENT = -7.5                 # exact in every storage type; a split-fp16 element left alone decodes to -15
SHAPES = [(50, 2, 3), (7, 3, 5), (5, 4, 6), (2, 8, 8), (3, 8, 12), (2, 14, 14), (1, 21, 32)]
RRV = ('rope', 'rope', 'vt')
# (kinds, head_c, K); the one [PLAIN, VT] case per dtype runs on every shape as well
LAYOUTS = [(RRV, 128, 128), (RRV, 256, 256), (RRV, 768, 128), (('rope',), 256, 128), (('rope', 'vt'), 256, 256), (('plain', 'vt'), 128, 128)]
CFGS = {'fp32': ['0', '1', '2', '3'], 'bf16': ['0', '1', '2', '3'], 'fp16': ['0', '1', '2', '3'],
        'fp16x3': ['0', '0w8', '1', '2', '3', '7', '8', '9', '11'],      # test_linear_split_fp16's
        'fp16f8': ['0', '1', '2', '3'],                                    # test_linear_fp16_fp8's
        'fp16x2f8': ['0', '1']}                                            # test_linear_2p5_unit's
TOL = {'fp32': 2e-5, 'bf16': OUT_TOL[torch.bfloat16], 'fp16': OUT_TOL[torch.float16], 'fp16x3': 3e-6, 'fp16f8': 3e-6, 'fp16x2f8': 3e-6}
# configurations that gemm_plan (gemm_plan.hpp) must take for some shape of the list, per dtype
MUST_TAKE = {'fp32': {'0', '1'}, 'bf16': {'0', '1', '2', '3'}, 'fp16': {'0', '1', '2', '3'}, 'fp16x3': {'0', '0w8', '1', '8'}, 'fp16f8': {'0', '1'},
             'fp16x2f8': {'0', '1'}}

_cache = {}                 # inputs, references and the first configuration's raw outputs, shared by the arms of the sweeps


def _say(line):
    print(line)


def _rup(a, b):
    return (a + b - 1) // b * b


def pin_infeasible(dtype, cfg, head_c, ntok, nowide=False):
    """None when the rules stated in include/dust3r_hip.h (d3r_linear_heads_tile_config) let a heads launch take the pinned configuration, else the reason."""
    if cfg.endswith('w8'):
        return None if dtype == 'fp16x3' else 'the eight-wave 128x128 tile exists in split-fp16 only'
    if cfg == '0':
        return None
    if cfg == '8':
        return None if dtype == 'fp16x3' else 'the 64x64 tile exists in split-fp16 only'
    if cfg == '1':
        return None if head_c % 256 == 0 else f'head_c = {head_c} is no multiple of 256: a 256-wide tile would span two regions'
    if cfg in ('2', '3'):
        if dtype in ('bf16', 'fp16') and ntok % 64 == 0 and not nowide:
            return None
        why = 'D3R_GEMM_NOWIDE is set' if nowide else ('ntok % 64 != 0' if dtype in ('bf16', 'fp16') else f'{dtype} has no such route')
        return ('a non-square tile cannot swap the MFMA operand roles for V^T; only bf16 / fp16 at ntok % 64 == 0 transpose V^T in the staging tile '
                f'instead ({why})')
    return f'configuration {cfg} is never taken by a heads launch (its kernel has no V^T route)'


def _pin(monkeypatch, cfg):
    if cfg is None:
        monkeypatch.delenv('D3R_GEMM_CFG', raising=False)
        monkeypatch.delenv('D3R_GEMM_T128W8', raising=False)
        return
    monkeypatch.setenv('D3R_GEMM_CFG', cfg[:-2] if cfg.endswith('w8') else cfg)
    monkeypatch.setenv('D3R_GEMM_T128W8', '1000000' if cfg.endswith('w8') else '0')


def _pin_code(cfg):
    return 12 if cfg.endswith('w8') else int(cfg)


def _inputs(dev, B, th, tw, kinds, head_c, K):
    key = ('in', B, th, tw, kinds, head_c, K)
    if key not in _cache:
        g = torch.Generator(device='cpu').manual_seed(B * 1000 + th * 37 + tw + head_c + len(kinds))
        M, N = B * th * tw, len(kinds) * head_c
        x = torch.randn((M, K), generator=g)
        W = torch.randn((N, K), generator=g) / math.sqrt(K)
        W = W * torch.tensor([1.0, 0.5, 2.0])[:len(kinds)].repeat_interleave(head_c)[:, None]      # unequal scale per region
        b = torch.randn(N, generator=g)                                                            # differs per column
        _cache[key] = (x.to(dev), W.to(dev), b.to(dev))
    return _cache[key]


def _product(dtype, x, W):
    """fp64 (M, N): the product of the operands as the mode rounds them"""
    from dust3r_amd import ops
    from oracle.f8_ref import f16f8_matmul, f16x2f8_matmul
    if dtype == 'fp16f8':
        return f16f8_matmul(x, W)
    if dtype == 'fp16x2f8':
        return f16x2f8_matmul(x, W)
    if dtype == 'fp16x3':
        return ops.unpack_x3(ops.pack_x3(x)).double() @ ops.unpack_x3(ops.pack_x3(W)).double().T
    tdt = {'fp32': torch.float32, 'bf16': torch.bfloat16, 'fp16': torch.float16}[dtype]
    return x.to(tdt).double() @ W.to(tdt).double().T


def _reference(dev, dtype, B, th, tw, kinds, head_c, K, bias):
    key = ('ref', dtype, B, th, tw, kinds, head_c, K, bias)
    if key not in _cache:
        x, W, b = _inputs(dev, B, th, tw, kinds, head_c, K)
        y = _product(dtype, x, W)
        if bias:
            y = y + b.double()
        _cache[key] = heads_ref(None, None, None, list(kinds), head_c, th * tw, tw, base=BASE, y=y)
    return _cache[key]


def _bits(t):
    return t.view({2: torch.int16, 4: torch.int32}[t.element_size()])


class _Dst:
    """the destinations of one launch, each between two guard bands, everything pre-filled with the sentinel"""

    def __init__(self, dev, dtype, kinds, B, H, ntok, ldv):
        from dust3r_amd import ops
        self.sdt, self.per = ops._HEAD_STORE[dtype]
        self.kinds, self.B, self.H, self.ntok, self.ldv = kinds, B, H, ntok, ldv
        self.n = [ops.heads_dst_numel(k, B, H, ntok, ldv, dtype) for k in kinds]
        self.g = GUARD * self.per
        self.buf = [torch.full((self.g + n + self.g,), SENT, dtype=self.sdt, device=dev) for n in self.n]
        self.sent = int(_bits(torch.full((1,), SENT, dtype=self.sdt))[0])

    def args(self):
        return [b[self.g:] for b in self.buf]

    def raw(self):
        return [_bits(b[self.g:self.g + n]).clone() for b, n in zip(self.buf, self.n)]

    def check_untouched(self, what):
        for r, (b, n, k) in enumerate(zip(self.buf, self.n, self.kinds)):
            bits = _bits(b)
            assert bool((bits[:self.g] == self.sent).all()), f'{what}: region {r} ({k}): the guard band BEFORE the destination was written'
            assert bool((bits[self.g + n:] == self.sent).all()), f'{what}: region {r} ({k}): the guard band AFTER the destination was written'
            if k == 'vt' and self.ldv > self.ntok:
                v = bits[self.g:self.g + n]
                if self.per == 2:      # split-fp16 rows: [hi x8][lo x8] per 8 logical columns
                    v = v.view(self.B, self.H, 64, self.ldv // 8, 2, 8).permute(0, 1, 2, 4, 3, 5).reshape(self.B, self.H, 64, 2, self.ldv)
                else:
                    v = v.view(self.B, self.H, 64, self.ldv)
                assert bool((v[..., self.ntok:] == self.sent).all()), f'{what}: region {r}: a padding column [ntok, ldv) of V^T was written'


def _launch(dev, dtype, table, B, th, tw, kinds, head_c, K, ldv=None, bias=True, ln=None, splitk=None, what='', xw=None):
    from dust3r_amd import ops
    ntok = th * tw
    ldv = ldv or _rup(ntok, 64)
    x, W, b = xw if xw is not None else _inputs(dev, B, th, tw, kinds, head_c, K)
    dst = _Dst(dev, dtype, kinds, B, head_c // 64, ntok, ldv)
    outs = ops.linear_heads(x, W, b if bias else None, list(kinds), head_c, ntok, tw, ldv, table, dtype=dtype, dsts=dst.args(), ln=ln, splitk=splitk)
    torch.cuda.synchronize()
    dst.check_untouched(what)
    return outs, dst.raw()


def _errors(outs, refs, kinds, ntok):
    """max |out - ref| / max |ref| per region"""
    errs = []
    for o, r, k in zip(outs, refs, kinds):
        o = o[..., :ntok] if k == 'vt' else o
        assert o.shape == r.shape
        errs.append(float((o.double() - r).abs().max() / r.abs().max()))
    return errs


@pytest.fixture(scope='module')
def table(gpu):
    from dust3r_amd import ops
    return ops.rope_table(512, BASE, 1.0, device=gpu)


@pytest.mark.parametrize('base', [100.0, 10000.0])
def test_rope_table(gpu, base):
    """d3r_rope_table(512, base, 1) against the numpy restatement of the kernel's own formula (fp64 pow rounded to fp32, fp32 product with pos, fp64 cos / sin
    rounded to fp32): within 1 ulp (the two libms may round cos / sin differently in the last place); and against the exact fp64 cos / sin of
    pos F0 / base^(i/16) within the derived bound pos inv_freq 2^-23 + 2^-24 (oracle/heads_ref.py rope_table_bound)."""
    from dust3r_amd import ops
    tab = ops.rope_table(512, base, 1.0, device=gpu).cpu().numpy()
    emu = rope_table_emulated(512, base, 1.0)
    assert tab.shape == emu.shape == (512, 16, 2)
    ulps = np.abs(tab.astype(np.float64) - emu.astype(np.float64)) / np.spacing(np.maximum(np.abs(emu), np.float32(2.0 ** -126))).astype(np.float64)
    ang, bound = rope_angles(512, base), rope_table_bound(512, base)
    dc = (torch.from_numpy(tab[..., 0]).double() - ang.cos()).abs()
    ds = (torch.from_numpy(tab[..., 1]).double() - ang.sin()).abs()
    _say(f'rope table base {base:g}: max {ulps.max():.2f} ulp from the emulated formula; max |table - exact| {float(torch.maximum(dc, ds).max()):.3e}, '
         f'largest share of its bound {float((torch.maximum(dc, ds) / bound).max()):.3f}')
    assert ulps.max() <= 1.0
    assert bool((dc <= bound).all()) and bool((ds <= bound).all())


@pytest.mark.parametrize('dtype,cfg', [(d, c) for d in CFGS for c in CFGS[d]])
def test_heads_layout_and_values(gpu, table, dtype, cfg, monkeypatch):
    """Every (shape, layout) of the issue under one pinned tile configuration: values per region against fp64 within the dtype's typed-store bound, the V^T
    padding and the guard bands around every destination untouched bit for bit, and the raw outputs bitwise equal to those of the first configuration
    that ran the same (dtype, shape, layout) -- the MFMA order per output does not depend on the tile (fold section), and neither may the
    epilogue's arithmetic. d3r_linear_heads_tile_config is asked first: an arm whose pin the heuristic ignores is SKIPPED with the reason (it would run the
    default tile under another name), and the rules that name the reason are checked against the heuristic both ways. Extra arms: ldv = rup(ntok, 64) + 64,
    no bias, and (configuration '0') D3R_GEMM_NOWIDE=1, where for split-fp16 the wide and the direct route are compared: bitwise on V^T / plain regions
    (both form fma(acc, 1, fma(0, 0, b)) = acc + b), 1e-6 relative on rotated regions (the same source expression u cos - v sin in two places, which
    hipcc is free to contract into an fma differently in each)."""
    from dust3r_amd import ops
    monkeypatch.delenv('D3R_GEMM_NOWIDE', raising=False)
    _pin(monkeypatch, cfg)
    arms = [(B, th, tw, kinds, head_c, K, 0, True) for (B, th, tw) in SHAPES for (kinds, head_c, K) in LAYOUTS]
    arms += [(2, 8, 8, RRV, 128, 128, 64, True), (5, 4, 6, RRV, 128, 128, 64, True), (3, 8, 12, RRV, 256, 256, 64, True),      # ldv = rup(ntok, 64) + 64
             (7, 3, 5, RRV, 128, 128, 0, False), (3, 8, 12, RRV, 256, 256, 0, False)]                                            # without a bias
    taken, skipped = 0, {}
    for (B, th, tw, kinds, head_c, K, ldv_extra, bias) in arms:
        ntok, M = th * tw, B * th * tw
        ldv = _rup(ntok, 64) + ldv_extra
        got = ops.heads_tile_config(M, K, list(kinds), head_c, ntok, tw, ldv, dtype)
        assert got >= 0
        why = pin_infeasible(dtype, cfg, head_c, ntok)
        if why is not None:
            assert got != _pin_code(cfg) or cfg == '0', f'{dtype} cfg {cfg}: taken although the rules say: {why}'
            skipped[why] = skipped.get(why, 0) + 1
            continue
        assert got == _pin_code(cfg), f'{dtype} cfg {cfg} ({B},{th},{tw}) head_c {head_c}: ignored (runs {got}) for a reason the stated rules do not name'
        taken += 1
        what = f'{dtype} cfg {cfg} ({B},{th},{tw}) {"|".join(kinds)} head_c {head_c} K {K} ldv {ldv}{"" if bias else " no bias"}'
        outs, raw = _launch(gpu, dtype, table, B, th, tw, kinds, head_c, K, ldv=ldv, bias=bias, what=what)
        errs = _errors(outs, _reference(gpu, dtype, B, th, tw, kinds, head_c, K, bias), kinds, ntok)
        _say(f'{what}: tile {got}; err / bound ' + ' '.join(f'{k} {e:.2e}/{TOL[dtype]:.0e}' for k, e in zip(kinds, errs)))
        assert all(e < TOL[dtype] for e in errs), what
        first = _cache.setdefault(('first', dtype, B, th, tw, kinds, head_c, K, ldv, bias), (cfg, raw))
        if first[0] != cfg:
            for r, (a, b_) in enumerate(zip(first[1], raw)):
                ndiff = int((a != b_).sum())
                if ndiff:
                    _say(f'    tile dependence: region {r} ({kinds[r]}) differs in {ndiff} of {a.numel()} storage elements between cfg {first[0]} and cfg {cfg}')
                assert ndiff == 0, f'{what}: region {r} is not bitwise equal to configuration {first[0]}'
    for why, n in skipped.items():
        _say(f'{dtype} cfg {cfg}: {n} arms skipped: {why}')
    if cfg == '0':      # the direct routes of every dtype
        monkeypatch.setenv('D3R_GEMM_NOWIDE', '1')
        for (B, th, tw, kinds, head_c, K) in [(2, 8, 8, RRV, 256, 256), (3, 8, 12, RRV, 256, 256), (50, 2, 3, ('plain', 'vt'), 128, 128)]:
            ntok = th * tw
            what = f'{dtype} cfg 0 NOWIDE ({B},{th},{tw}) {"|".join(kinds)} head_c {head_c}'
            outs, raw = _launch(gpu, dtype, table, B, th, tw, kinds, head_c, K, what=what)
            refs = _reference(gpu, dtype, B, th, tw, kinds, head_c, K, True)
            errs = _errors(outs, refs, kinds, ntok)
            line = f'{what}: err / bound ' + ' '.join(f'{k} {e:.2e}/{TOL[dtype]:.0e}' for k, e in zip(kinds, errs))
            assert all(e < TOL[dtype] for e in errs), what
            wide = _cache[('first', dtype, B, th, tw, kinds, head_c, K, _rup(ntok, 64), True)]
            if dtype == 'fp16x3' and wide[0] == '0':
                for r, k in enumerate(kinds):
                    if k == 'rope':
                        a, b_ = ops.unpack_x3(wide[1][r].view(torch.float16)).double(), ops.unpack_x3(raw[r].view(torch.float16)).double()
                        rel = float((a - b_).abs().max() / refs[r].abs().max())
                        line += f'; wide vs direct {k} {rel:.1e} ({"bitwise" if torch.equal(wide[1][r], raw[r]) else "not bitwise"})'
                        assert rel <= 1e-6, what
                    else:
                        assert torch.equal(wide[1][r], raw[r]), f'{what}: region {r} ({k}) differs between the wide and the direct route'
            _say(line)
    if taken == 0:
        assert cfg not in MUST_TAKE[dtype], f'{dtype}: configuration {cfg} was taken for no shape of the list'
        pytest.skip(f'{dtype} cfg {cfg}: infeasible for every arm: ' + '; '.join(skipped))


def _fold_case(dev, B, th, tw, K, head_c, const_rows, seed):
    from dust3r_amd import ops
    x, gamma, beta, W, b = fold_inputs(B, th, tw, K, head_c, seed=seed, const_rows=const_rows)
    x = ops.unpack_x3(ops.pack_x3(x))                              # the rows the kernel reads, exactly
    wg = ops.unpack_x3(ops.pack_x3(W * gamma))                     # r(gamma_k W_nk): the weights the kernel reads, exactly
    colsum = wg.double().sum(-1)                                   # of the rounded operand, fp64
    bf = b.double() + W.double() @ beta.double()                   # b' = b + W beta
    return [t.to(dev) for t in (x, wg, colsum, bf)]


def _ulp32(v):
    return torch.from_numpy(np.spacing(np.abs(v.cpu().numpy().astype(np.float32))).astype(np.float64)).to(v.device)


def test_heads_folded_layernorm_consumer(gpu, table, monkeypatch):
    """The consumer side of the folded LayerNorm (split-fp16): weights r(W diag(gamma)), colsum_n = sum_k r(gamma_k W_nk), b' = b + W beta, statistics
    either passed in (route A: fp64 on the host, rounded to fp32) or formed by the launch from the 32-column (sum x, sum x^2) pairs (route B).

    Reference: fp64 RoPE(LN(x) W~^T + b) with W~_nk = r(gamma_k W_nk) / gamma_k, i.e. rstd_m (sum_k x_mk w~_nk - mean_m colsum_n) + b'_n on exactly the
    operands the kernel reads (x is pre-rounded to split-fp16; the fold identity itself is pinned in fp64 by tests/test_gemm_heads_cpu.py).
    Bound per element, from reference quantities only, with S = rstd_m sum_k |x_mk w~_nk|, T = |colsum_n nmr_m|, Bn = |b'_n|, A = S + T + Bn and
    u = 2^-24 (fp32), 2^-21 = 8 u:
      - the lo.lo products the three-MFMA scheme drops: |x_lo w_lo| <= 2^-22 |x w|                                       0.5  x 2^-21 S
      - fp32 accumulation: 3 K / 32 MFMAs add into the accumulator (three per 32 k), each allowed two roundings of a
        partial sum <= sum |x w| (one inside the MFMA's own 32-term sum, one on the add): 6 K / 32 u                     6 K / 256 x 2^-21 S
      - fma(colsum, nmr, b'): colsum, nmr and b' rounded to fp32 (u T, u T, u Bn) and the fma's rounding (u (T + Bn));
        fma(acc, rstd, .): rstd rounded (u S) and the fma's rounding (u A): <= 5 u A                                      0.625 x 2^-21 A
      - the rotation u cos - v sin in fp32: two roundings of terms <= |u| + |v|                                           0.25 x 2^-21 (A_u + A_v)
      - the split-fp16 store: 2^-22 relative                                                                              0.5  x 2^-21 (A_u + A_v)
    so c = 2 + 6 K / 256 (8 at K = 256, 5 at K = 128) on A for unrotated regions and on A_u + A_v of the pair (c, c + 16) for rotated ones (|cos|, |sin| <= 1
    carry each partner's error over in full). The table's distance from the exact angles (test_rope_table's bound) is not an error of this epilogue and is
    added as its own term, (|u_ref| + |v_ref|) (pos inv_freq 2^-23 + 2^-24). The cancellation in acc - mean colsum is inside the bound because S and T enter
    separately; the input condition |mean| <= 2 std (asserted on the CPU) keeps T of the order of S.
    Constant rows (std = 0): rstd = 1 / sqrt(eps) must be finite and the output is b + W beta, rotated, within the same bound (S carries the factor 1000).

    Route B: the statistics the launch wrote are within 2 ulp of the fp64 evaluation of ITS inputs (the fp32 partial sums; kernel: fp64 sums, one rounding
    of rstd, nmr = fp32(-mean) * rstd), bitwise equal across the taken tile configurations (threads per row: 2 on the 128x128 and 256x256 tiles, 4 on the
    eight-wave and 64x64 ones; TPR = 1 belongs to tiles no heads launch can take), rows past M untouched; its outputs are bitwise those of a route-A
    launch fed the same statistics."""
    from dust3r_amd import ops
    monkeypatch.delenv('D3R_GEMM_NOWIDE', raising=False)
    eps = 1e-6
    for si, (B, th, tw) in enumerate([(50, 2, 3), (3, 8, 12), (1, 21, 32)]):
        for K, head_c in ((128, 128), (256, 256)):
            ntok, M, N = th * tw, B * th * tw, 3 * head_c
            const_rows = 4 if (B, th, tw) == (3, 8, 12) else 0
            x, wg, colsum, bf = _fold_case(gpu, B, th, tw, K, head_c, const_rows, 100 + si)
            mean, rstd = layernorm_stats(x, eps)
            assert bool(torch.isfinite(rstd).all())
            nmr = -mean * rstd
            y = rstd[:, None] * (x.double() @ wg.double().T - mean[:, None] * colsum[None, :]) + bf[None, :]
            if const_rows:
                assert float((y[M - const_rows:] - bf[None, :]).abs().max()) < 1e-9       # the reference of the constant rows IS b + W beta (fp64 noise x 1000)
            ang = rope_angles(max(th, tw), BASE)
            refs = scatter_heads(y, RRV, head_c, ntok, tw, ang.cos().to(gpu), ang.sin().to(gpu))
            c = 2 + 6 * K / 256
            A = rstd[:, None] * (x.double().abs() @ wg.double().abs().T) + (colsum[None, :] * nmr[:, None]).abs() + bf.abs()[None, :]
            one, zero = torch.ones_like(ang).to(gpu), torch.zeros_like(ang).to(gpu)
            A_l = scatter_heads(A, ('plain', 'plain', 'vt'), head_c, ntok, tw, one, zero)
            y_l = scatter_heads(y.abs(), ('plain', 'plain', 'vt'), head_c, ntok, tw, one, zero)
            t = torch.arange(ntok)
            tb = rope_table_bound(max(th, tw), BASE)
            tabd = torch.cat((tb[t // tw], tb[t // tw], tb[t % tw], tb[t % tw]), dim=-1).to(gpu)      # (ntok, 64): the table bound of each (token, column)
            pair = lambda v: v.view(*v.shape[:-1], 2, 2, 16).sum(-2, keepdim=True).expand(*v.shape[:-1], 2, 2, 16).reshape(v.shape)      # noqa: E731
            bounds = [c * 2.0 ** -21 * pair(A_l[r]) + pair(y_l[r]) * tabd for r in (0, 1)] + [c * 2.0 ** -21 * A_l[2]]
            ln_a = dict(rstd=rstd.float(), nmr=nmr.float(), colsum=colsum.float(), eps=eps)
            part = torch.stack((x.view(M, K // 32, 32).sum(-1), (x * x).view(M, K // 32, 32).sum(-1)), dim=-1).contiguous()      # fp32, on the host side of the launch
            s64, t64 = part[..., 0].double().sum(-1), part[..., 1].double().sum(-1)
            mean_b = s64 / K
            rstd_b = 1.0 / torch.sqrt((t64 / K - mean_b * mean_b).clamp_min(0.0) + float(np.float32(eps)))
            nmr_b = -mean_b * rstd_b
            stats0 = None
            for cfg in ('0', '0w8', '1', '8'):
                _pin(monkeypatch, cfg)
                got = ops.heads_tile_config(M, K, list(RRV), head_c, ntok, tw, _rup(ntok, 64), 'fp16x3')
                why = pin_infeasible('fp16x3', cfg, head_c, ntok)
                if why is not None:
                    assert got != _pin_code(cfg)
                    _say(f'fold ({B},{th},{tw}) head_c {head_c} cfg {cfg}: skipped: {why}')
                    continue
                assert got == _pin_code(cfg)
                what = f'fold ({B},{th},{tw}) head_c {head_c} K {K} cfg {cfg}'
                xw = (x, wg, bf.float())
                outs, raw_a = _launch(gpu, 'fp16x3', table, B, th, tw, RRV, head_c, K, ln=ln_a, what=what + ' A', xw=xw)
                worst = []
                for r, (o, ref, bd) in enumerate(zip(outs, refs, bounds)):
                    o = o[..., :ntok] if r == 2 else o
                    assert bool(torch.isfinite(o).all())
                    ratio = (o.double() - ref).abs() / bd
                    worst.append(float(ratio.max()))
                _say(f'{what}: route A, largest share of the computed bound (c = {c:g}): q {worst[0]:.3f} k {worst[1]:.3f} v {worst[2]:.3f}')
                assert max(worst) <= 1.0, what
                # route B: statistics formed by the launch, written into sentinel-filled arrays with a guard band
                st = torch.full((2, M + GUARD), 1.0e30, dtype=torch.float32, device=gpu)
                ln_b = dict(rstd=st[0], nmr=st[1], colsum=colsum.float(), part_in=part, eps=eps)
                _, raw_b = _launch(gpu, 'fp16x3', table, B, th, tw, RRV, head_c, K, ln=ln_b, what=what + ' B', xw=xw)
                assert bool((st[:, M:] == 1.0e30).all()), f'{what}: statistics written past row M'
                ur, un = float(((st[0, :M].double() - rstd_b).abs() / _ulp32(rstd_b)).max()), float(((st[1, :M].double() - nmr_b).abs() / _ulp32(nmr_b)).max())
                _say(f'{what}: route B statistics, ulp from fp64: rstd {ur:.2f} nmr {un:.2f}')
                assert ur <= 2.0 and un <= 2.0, what
                if stats0 is None:
                    stats0 = st[:, :M].clone()
                assert torch.equal(st[:, :M], stats0), f'{what}: the statistics depend on the tile configuration'
                ln_a2 = dict(rstd=st[0, :M].clone(), nmr=st[1, :M].clone(), colsum=colsum.float(), eps=eps)
                _, raw_a2 = _launch(gpu, 'fp16x3', table, B, th, tw, RRV, head_c, K, ln=ln_a2, what=what + " A'", xw=xw)
                for r in range(3):
                    assert torch.equal(raw_b[r], raw_a2[r]), f'{what}: route B region {r} differs from route A fed the same statistics'
                if const_rows:      # std = 0 rows: the output is b + W beta, rotated (refs), within the bound -- covered above; and finite
                    assert bool(torch.isfinite(st[:, M - const_rows:M]).all()) and float((st[0, M - const_rows:M] - 1000.0).abs().max()) < 1e-3


def test_heads_split_k(gpu, table, monkeypatch):
    """Split-K under the heads epilogue (split-fp16, no pin): (1, 8, 12), [ROPE, ROPE, VT], head_c 256, K = 1024 goes to the 64x64 tile (24 tiles), and with
    the loan launch_gemm splits it in 2 (16 K steps of 32 per slice). Contract of the ticket counters, from the combine in gemm.hip: the CALLER zeroes
    them once; the block that draws a tile's last ticket stores 0 back before it combines, so they are zero again after every launch and the next launch
    needs nothing from the caller. Both runs are held to the 3e-6 bound; two consecutive launches on the same loaned buffers are bitwise equal with the
    counters untouched in between; that the split was taken shows in the slab, which no longer holds its pre-fill over exactly tiles x 2 x 64 x 64 floats
    (and does beyond), while the counters read zero after each launch."""
    from dust3r_amd import ops
    monkeypatch.delenv('D3R_GEMM_NOWIDE', raising=False)
    _pin(monkeypatch, None)
    B, th, tw, head_c, K = 1, 8, 12, 256, 1024
    ntok, M, N = th * tw, B * th * tw, 3 * head_c
    assert ops.heads_tile_config(M, K, list(RRV), head_c, ntok, tw, 128, 'fp16x3') == 8
    refs = _reference(gpu, 'fp16x3', B, th, tw, RRV, head_c, K, True)
    outs, raw0 = _launch(gpu, 'fp16x3', table, B, th, tw, RRV, head_c, K, what='split-K: without the loan')
    e0 = _errors(outs, refs, RRV, ntok)
    tiles = (M + 63) // 64 * (N // 64)
    used = tiles * 2 * 64 * 64
    slab = torch.full((used + 4096,), 3.0e38, dtype=torch.float32, device=gpu)
    cnt = torch.zeros(64, dtype=torch.int32, device=gpu)
    outs, raw1 = _launch(gpu, 'fp16x3', table, B, th, tw, RRV, head_c, K, splitk=(slab, cnt), what='split-K: with the loan')
    e1 = _errors(outs, refs, RRV, ntok)
    _say(f'split-K (1,8,12) head_c 256 K 1024: err / bound without the loan ' + ' '.join(f'{e:.2e}/3e-06' for e in e0) + '; with ' + ' '.join(f'{e:.2e}/3e-06' for e in e1))
    assert all(e < 3e-6 for e in e0 + e1)
    assert bool((slab[:used] != 3.0e38).all()) and bool((slab[used:] == 3.0e38).all()), 'the split was not taken as expected (slab pre-fill)'
    assert int(cnt.abs().sum()) == 0, 'the ticket counters are not re-armed'
    _, raw2 = _launch(gpu, 'fp16x3', table, B, th, tw, RRV, head_c, K, splitk=(slab, cnt), what='split-K: second launch on the same buffers')
    assert int(cnt.abs().sum()) == 0
    for r in range(3):
        assert torch.equal(raw1[r], raw2[r]), f'region {r}: two launches on the same loaned buffers differ'
