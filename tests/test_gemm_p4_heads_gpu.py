"""The q | k attention projections on the persistent split-fp16 GEMM (csrc/gemm_p4.hip, EPK_HEADS / EPK_HEADS_D: bias / folded LayerNorm, 2-D RoPE and the head
scatter in the drain), one launch at a time through d3r_linear_heads: D3R_GEMM_PERSIST=1 against =0 on the same operands.

Every destination must be BYTE-equal between the two kernels (guard bands included: nothing outside a destination is written), and the =0 result within the
bound tests/test_gemm_heads_gpu.py::test_heads_layout_and_values uses for split-fp16 (3e-6 of the region's max |ref|) of an fp64 reference written here:
y = x W^T (+ b, or the folded-LayerNorm expression rstd_m y + nmr_m colsum_n + b_n) on the operands as split-fp16 rounds them, then croco's RoPE2D per head
(columns 0-31 rotate with the token's row, 32-63 with its column; pairs (c, c + 16) inside a half; angle pos / 100^(i / 16)).

Shapes (M, token grid, images, head_c, K): what each exercises in the kernel
  2048, 16 x 16,  8, 256,  768   32 tiles, 24 K steps: 16 draining steps and 8 behind them
  1536, 24 x 32,  2, 256, 1024   24 tiles, 32 K steps
  2048, 16 x 16,  8, 128, 1536   16 tiles, 48 K steps: most of a tile's steps run behind the drain; one region per 128-column tile
   768,  6 x  8, 16, 256,  768   12 tiles; an image boundary every 48 rows inside a 256-row tile; ntok % 32 != 0: gemm.hip's direct epilogue is the =0 side
 12288, 24 x 32, 16, 768,  768   576 tiles on 256 blocks: first, overlapped and last tile of a block; 12 heads per region
and (512, 16 x 16, 2, 128, 768): 4 tiles < 8, which the forced mode must hand to the one-tile-per-block kernels and report so.
"""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

BASE = 100.0
GUARD = 256 * 2             # storage elements (fp16) of sentinel around every destination
SENT = -7.5
TOL = 3e-6                  # test_heads_layout_and_values, fp16x3
KINDS = ('rope', 'rope')
SHAPES = [(8, 16, 16, 256, 768), (2, 24, 32, 256, 1024), (8, 16, 16, 128, 1536), (16, 6, 8, 256, 768), (16, 24, 32, 768, 768)]


def _rup(a, b):
    return (a + b - 1) // b * b


@pytest.fixture(scope='module')
def table(gpu):
    from dust3r_amd import ops
    return ops.rope_table(512, BASE, 1.0, device=gpu)


def _rope_ref(y, head_c, th, tw):
    """fp64 (M, R head_c) -> one (B, H, ntok, 64) tensor per region, rotated"""
    ntok, H = th * tw, head_c // 64
    B = y.shape[0] // ntok
    t = torch.arange(ntok, device=y.device)
    inv = BASE ** (-torch.arange(16, device=y.device, dtype=torch.float64) / 16.0)
    outs = []
    for r in range(y.shape[1] // head_c):
        v = y[:, r * head_c:(r + 1) * head_c].reshape(B, ntok, H, 2, 2, 16).permute(0, 2, 1, 3, 4, 5).clone()      # (B, H, ntok, half, u | v, 16)
        for half, pos in ((0, t // tw), (1, t % tw)):
            ang = pos.double()[:, None] * inv[None, :]
            c, s = ang.cos()[None, None], ang.sin()[None, None]
            u, w = v[:, :, :, half, 0].clone(), v[:, :, :, half, 1].clone()
            v[:, :, :, half, 0] = u * c - w * s
            v[:, :, :, half, 1] = w * c + u * s
        outs.append(v.reshape(B, H, ntok, 64))
    return outs


def _case(dev, B, th, tw, head_c, K):
    from dust3r_amd import ops
    g = torch.Generator(device='cpu').manual_seed(B * 1000 + th * 37 + tw + head_c + K)
    M, N = B * th * tw, 2 * head_c
    r = lambda t: ops.unpack_x3(ops.pack_x3(t))      # noqa: E731
    x = r(torch.randn((M, K), generator=g)).to(dev)
    W = r(torch.randn((N, K), generator=g) / math.sqrt(K) * torch.tensor([1.0, 0.5]).repeat_interleave(head_c)[:, None]).to(dev)      # unequal scale per region
    b = torch.randn(N, generator=g).to(dev)
    rstd = (0.5 + torch.rand(M, generator=g)).to(dev)
    nmr = (torch.rand(M, generator=g) - 0.5).to(dev)
    colsum = torch.randn(N, generator=g).to(dev)
    acc = x.double() @ W.double().T
    refs = {'bias': _rope_ref(acc + b.double(), head_c, th, tw),
            'none': _rope_ref(acc, head_c, th, tw),
            'fold': _rope_ref(rstd.double()[:, None] * acc + nmr.double()[:, None] * colsum.double()[None, :] + b.double(), head_c, th, tw)}
    return x, W, b, dict(rstd=rstd, nmr=nmr, colsum=colsum, eps=1e-6), refs


def _run(dev, table, x, W, b, ln, B, th, tw, head_c, what):
    from dust3r_amd import ops
    ntok, H = th * tw, head_c // 64
    n = ops.heads_dst_numel('rope', B, H, ntok, _rup(ntok, 64), 'fp16x3')
    bufs = [torch.full((GUARD + n + GUARD,), SENT, dtype=torch.float16, device=dev) for _ in KINDS]
    outs = ops.linear_heads(x, W, b, list(KINDS), head_c, ntok, tw, _rup(ntok, 64), table, dtype='fp16x3', dsts=[t[GUARD:] for t in bufs], ln=ln)
    torch.cuda.synchronize()
    for r, t in enumerate(bufs):
        assert bool((t[:GUARD] == SENT).all()) and bool((t[GUARD + n:] == SENT).all()), f'{what}: a guard band of region {r} was written'
    return outs, [t.view(torch.int16).clone() for t in bufs]


@pytest.mark.parametrize('B,th,tw,head_c,K', SHAPES)
def test_persistent_heads_is_byte_equal(gpu, table, B, th, tw, head_c, K, monkeypatch):
    from dust3r_amd import ops
    for name in ('D3R_GEMM_NOWIDE', 'D3R_GEMM_CFG', 'D3R_GEMM_T128W8'):
        monkeypatch.delenv(name, raising=False)
    ntok, M = th * tw, B * th * tw
    x, W, b, ln, refs = _case(gpu, B, th, tw, head_c, K)
    for arm, (bias, fold) in (('bias', (b, None)), ('fold', (b, ln)), ('none', (None, None))):
        raws = {}
        for mode in ('1', '0'):
            monkeypatch.setenv('D3R_GEMM_PERSIST', mode)
            what = f'heads ({M} = {B} x {th} x {tw}, head_c {head_c}, K {K}) {arm} PERSIST {mode}'
            got = ops.heads_tile_config(M, K, list(KINDS), head_c, ntok, tw, _rup(ntok, 64), 'fp16x3')
            assert (got == 10) == (mode == '1'), f'{what}: runs tile {got}'
            outs, raws[mode] = _run(gpu, table, x, W, bias, fold, B, th, tw, head_c, what)
            errs = [float((o.double() - r).abs().max() / r.abs().max()) for o, r in zip(outs, refs[arm])]
            print(f'{what}: tile {got}; err / bound ' + ' '.join(f'{e:.2e}/{TOL:.0e}' for e in errs))
            if mode == '0':
                assert all(e < TOL for e in errs), what
        for r in range(len(KINDS)):
            nd = int((raws['1'][r] != raws['0'][r]).sum())
            assert nd == 0, f'({M}, head_c {head_c}, K {K}) {arm}: region {r}: {nd} of {raws["0"][r].numel()} storage elements differ between the two kernels'


def test_forced_mode_falls_back_below_eight_tiles(gpu, table, monkeypatch):
    """D3R_GEMM_PERSIST=1 on a launch of 4 tiles of 256 x 128: the persistent kernel's grid is a multiple of 8 blocks, so the launch runs on a one-tile-per-block
    kernel, the query says so, and the result is the =0 one."""
    from dust3r_amd import ops
    for name in ('D3R_GEMM_NOWIDE', 'D3R_GEMM_CFG', 'D3R_GEMM_T128W8'):
        monkeypatch.delenv(name, raising=False)
    B, th, tw, head_c, K = 2, 16, 16, 128, 768
    ntok, M = th * tw, B * th * tw
    x, W, b, ln, refs = _case(gpu, B, th, tw, head_c, K)
    raws = {}
    for mode in ('1', '0'):
        monkeypatch.setenv('D3R_GEMM_PERSIST', mode)
        got = ops.heads_tile_config(M, K, list(KINDS), head_c, ntok, tw, _rup(ntok, 64), 'fp16x3')
        assert 0 <= got != 10, f'PERSIST {mode}: a launch of 4 tiles reports tile {got}'
        raws[mode] = (got, _run(gpu, table, x, W, b, None, B, th, tw, head_c, f'4 tiles PERSIST {mode}'))
    assert raws['1'][0] == raws['0'][0]
    errs = [float((o.double() - r).abs().max() / r.abs().max()) for o, r in zip(raws['0'][1][0], refs['bias'])]
    assert all(e < TOL for e in errs)
    assert all(torch.equal(a, c) for a, c in zip(raws['1'][1][1], raws['0'][1][1]))
