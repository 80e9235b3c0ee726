"""The DPT head's kernels alone, in the default engine's split-fp16 operand layout, against plain torch in FLOAT64 on the same operands: the implicit-GEMM
convolution (AMODE_CONV), ConvTranspose2d as a GEMM with a scatter epilogue (EPI_CONVT), the device weight packers that feed both, the fused tail
(EPI_HEAD4: 3x3 conv + ReLU + Conv2d(C, 4, 1) + postprocess on the accumulators), head_final_kernel and linear_head_post_kernel -- called through the
entry points the engine's own launches are built by (include/dust3r_hip.h: d3r_pack_conv_weight ... d3r_linear_head_post).

Operands. Every fp32 input is first rounded to what a split-fp16 row holds (hi + lo, ops.unpack_x3(ops.pack_x3(x))) -- or to the 16-bit type in the
head_final cases of those types --, so the reference works on EXACTLY the values the kernel reads. References: F.conv2d, F.conv_transpose2d(stride = k),
F.pixel_shuffle and the postprocess formulas restated in fp64 (tests/test_dpt_head_cpu.py checks those restatements without a GPU).

Tolerances, none read off the kernels:
  * pre-activation values (convolution, transposed convolution, the 'linear' depth mode of the tails) in split-fp16 or fp32 rows: X3_TOL = 3e-6 of the
    reference's max-abs, the project's bound for this arithmetic (tests/test_kernels_gpu.py test_linear_split_fp16: 22-bit operands, fp32 accumulation,
    at most one 22-bit output rounding). It holds for the K = 2304 convolution too (figures in test_conv_split_fp16's docstring).
    16-bit and fp32 rows of head_final: OUT_TOL of tests/test_kernels_gpu.py.
  * nonlinear postprocess modes: with delta = that bound as an absolute value, per pixel twice the largest deviation of the fp64 postprocess over the
    eight points (reference pre-activation +- delta e_i), plus 4 fp32 ulp of the result for expm1f / expf (test_dpt_head_cpu.postprocess_bound).
    Inputs are scaled so that |xyz| <= 3 and |confidence logit| <= 4 (asserted on the fp64 reference where the case is built): the bound then stays
    below 2e-4 absolute (printed per case), where a wrong tap or a mis-masked channel moves the result by 1e-2 ... 1 (a dropped operand half, ~1e-4 of the scale, is caught by X3_TOL above).
  * permutations and masks are exact: device packers against the Python packing, padding channels, sentinels around and inside the outputs, the wide
    against the direct epilogue.
  * the fused tail against the two-kernel tail: the 2e-5 per pixel of tests/test_forward_gpu.py::test_fused_head_tail_equals_the_two_kernel_route.
"""
import functools
import math

import pytest
import torch
import torch.nn.functional as F

from test_dpt_head_cpu import INF, POST_MODES, conv_weight_rows, convt_bias_rows, convt_weight_rows, postprocess64, postprocess_bound
from test_kernels_gpu import OUT_TOL

pytestmark = pytest.mark.gpu

X3_TOL = 3e-6
SENT = -1234.5          # sentinel of the guard regions: exact in fp16 and fp32
# D3R_GEMM_CFG values a split-fp16 convolution launch can be pinned to (gemm_plan.hpp gemm_plan): 0 = 128 x 128 (by four waves, and '0w8' by eight),
# 1 = 256 x 256, 2 = 256 x 128, 3 = 512 x 128, 7 = 256 x 128 by four waves with the weights of a K step in registers, 8 = 64 x 64, 11 = 96 x 64;
# 'auto' = the heuristic. 9 (384 x 192) is for nn.Linear operands only: the transposed convolution's GEMM takes it where its columns are whole tiles
# (the 96 -> 96, k = 4 case: N = 1536), elsewhere the pin is ignored and the heuristic's tile runs.
CONV_CFGS = ['auto', '0', '0w8', '1', '2', '3', '7', '8', '11']
CONVT_CFGS = CONV_CFGS + ['9']


def pin_tile(monkeypatch, cfg):
    if cfg == 'auto':
        monkeypatch.delenv('D3R_GEMM_CFG', raising=False)
        monkeypatch.delenv('D3R_GEMM_T128W8', raising=False)
    else:
        monkeypatch.setenv('D3R_GEMM_CFG', cfg[:-2] if cfg.endswith('w8') else cfg)
        monkeypatch.setenv('D3R_GEMM_T128W8', '1000000' if cfg.endswith('w8') else '0')


def rnd22(x):
    """fp32 -> the value a split-fp16 row holds for it: hi + lo, hi = fp16(x), lo = fp16(x - hi) (ops.pack_x3 / unpack_x3, any shape)"""
    hi = x.float().half()
    return hi.float() + (x.float() - hi.float()).half().float()


def relmax(out, ref):
    """max |out - ref| relative to the reference's max-abs, in fp64"""
    ref = ref.double()
    return float((out.double().cpu() - ref.cpu()).abs().max() / ref.abs().max())


def bits(t):
    return t.view(torch.int16) if t.dtype in (torch.float16, torch.bfloat16) else t.view(torch.int32)


# ---------------------------------------------------------------------------------------------------------------- convolution
CONV_CASES = {   # B, H, W, Cin, Cout, k, stride, pad [, cin_pad] and what the launch adds
    'border_3x7x5_32to128': dict(g=(3, 7, 5, 32, 128, 3, 1, 1)),                             # one K slice per tap, M = 105 below every tile, tiles straddle images
    'stride2_21x32_96to96': dict(g=(1, 21, 32, 96, 96, 3, 2, 1)),                            # stride 2 with odd H, Cout below n_pad, cstride 96
    'k2304_residuals': dict(g=(2, 12, 16, 256, 256, 3, 1, 1), bias=False, res=True),         # the long K loop; res1 + res2 + ReLU copy
    'k2304_relu': dict(g=(2, 12, 16, 256, 256, 3, 1, 1), relu=True),
    'one_by_one_64to128': dict(g=(2, 6, 8, 64, 128, 1, 1, 0)),
    'padded_24to64': dict(g=(1, 9, 11, 24, 64, 3, 1, 1), cin_pad=32),                        # the 8 pad channels of the rows hold finite non-zero values
}


@functools.lru_cache(maxsize=None)
def conv_case(name):
    c = CONV_CASES[name]
    B, H, W, Cin, Cout, k, stride, pad = c['g']
    cin_pad = c.get('cin_pad', Cin)
    g = torch.Generator(device='cpu').manual_seed(sum(c['g']) + len(name))
    x = rnd22(torch.randn((B, H, W, cin_pad), generator=g))
    if cin_pad > Cin:
        x[..., Cin:] = rnd22(50.0 * torch.randn((B, H, W, cin_pad - Cin), generator=g) + 7.0)
    w = rnd22(torch.randn((Cout, Cin, k, k), generator=g) / math.sqrt(Cin * k * k))
    b = torch.randn(Cout, generator=g) if c.get('bias', True) else None
    ref = F.conv2d(x[..., :Cin].double().permute(0, 3, 1, 2), w.double(), None if b is None else b.double(), stride=stride, padding=pad).permute(0, 2, 3, 1)
    res = None
    if c.get('res'):
        res = (rnd22(torch.randn(ref.shape, generator=g)), rnd22(torch.randn(ref.shape, generator=g)))
        ref = ref + res[0].double() + res[1].double()
    if c.get('relu'):
        ref = ref.clamp_min(0)
    return dict(x=x, w=w, b=b, res=res, ref=ref.contiguous(), cin_pad=cin_pad, relu=bool(c.get('relu')))


@pytest.mark.parametrize('cfg', CONV_CFGS)
@pytest.mark.parametrize('name', list(CONV_CASES))
def test_conv_split_fp16(gpu, name, cfg, monkeypatch):
    """AMODE_CONV with D3R_F16X3 operands on every tile shape, fed by the device packer (PACK_CONV, bit-equal to ops.pack_conv_weight of the channel-padded
    tensor in split rows), against fp64 F.conv2d within X3_TOL; the LDS-staged and the direct epilogue (by D3R_GEMM_NOWIDE and by the launch's own flag) agree
    bit for bit. padded_24to64: cin_pad = 32 > Cin = 24 -- the result equals the 24-channel convolution whatever the rows hold in the pad channels.
    K = 2304 (k2304_*): X3_TOL holds -- measured on an MI355X against the fp64 F.conv2d reference, 7.1e-7 (residuals) and 8.5e-7 (ReLU) of the reference's
    max-abs, the same figure on every tile shape and epilogue (for scale: torch's own fp32 CPU convolution of these operands is 1.2e-6 / 1.5e-6 from the same
    reference), so the issue's fallback bound of four times torch's fp32 error is not used."""
    from dust3r_amd import ops
    c = conv_case(name)
    B, H, W, Cin, Cout, k, stride, pad = CONV_CASES[name]['g']
    pin_tile(monkeypatch, cfg)
    x, w = c['x'].to(gpu), c['w'].to(gpu)
    b = None if c['b'] is None else c['b'].to(gpu)
    wp = ops.pack_conv_weight_device(w, cin_pad=c['cin_pad'])
    want = ops.pack_x3(ops.pad_rows(conv_weight_rows(c['w'], c['cin_pad'])))
    assert wp.shape == want.shape and torch.equal(bits(wp.cpu()), bits(want)), 'device packer (PACK_CONV) != Python packing'
    res = (None, None) if c['res'] is None else tuple(r.to(gpu) for r in c['res'])
    got = []
    for env, flag in (('0', False), ('1', False), ('0', True)):
        monkeypatch.setenv('D3R_GEMM_NOWIDE', env)
        o = ops.conv2d_nhwc_x(x, wp, b, Cout, k, stride, pad, cin_pad=c['cin_pad'], relu=c['relu'], nowide=flag, res1=res[0], res2=res[1], relu_copy=c['res'] is not None)
        o = o if isinstance(o, tuple) else (o,)
        err = relmax(o[0], c['ref'])
        print(f'conv x3 {name} cfg={cfg} nowide={env}/{flag}: rel err {err:.2e}')
        assert o[0].shape == c['ref'].shape and err < X3_TOL
        if len(o) == 2:
            assert relmax(o[1], c['ref'].clamp_min(0)) < X3_TOL, 'ReLU copy'
        got.append(o)
    for other in got[1:]:
        for a, bb in zip(got[0], other):
            assert torch.equal(a, bb), 'wide and direct epilogue differ'


def test_conv_rejects_a_partial_k_step(gpu):
    """cin_pad = 24 is not a whole K step of 32 channels: D3R_ERR_INVALID, and nothing is launched (the output keeps its sentinel)."""
    from dust3r_amd import _lib, ops
    from dust3r_amd._lib import lib, ptr
    c = conv_case('padded_24to64')
    x = ops.pack_x3(c['x'].to(gpu))
    wp = ops.pack_conv_weight_device(c['w'].to(gpu), cin_pad=32)
    out = torch.full((1, 9, 11, 128), SENT, dtype=torch.float16, device=gpu)
    before = out.clone()
    rc = lib.d3r_conv2d_nhwc_x(ptr(x), ptr(wp), None, ptr(out), None, None, None, 1, 9, 11, 32, 24, 64, 64, 64, 3, 1, 1, 0, ptr(ops._zero_page(gpu)), _lib.DTYPE_F16X3,
                               _lib.current_stream())
    torch.cuda.synchronize()
    assert rc == -1 and _lib.ERRORS[rc] == 'invalid argument' and torch.equal(bits(out), bits(before))


# ---------------------------------------------------------------------------------------------------------------- transposed convolution
CONVT_CASES = {   # B, th, tw, Cin, Cout, cin_pad, cout_pad
    't3x5_32to32': (2, 3, 5, 32, 32, 32, 32),
    't3x5_24to24_pad32': (2, 3, 5, 24, 24, 32, 32),
    't5x7_96to96': (3, 5, 7, 96, 96, 96, 96),          # M = 105 (ragged in every tile), N = 16 x 96 / 4 x 96: several column tiles
}


@functools.lru_cache(maxsize=None)
def convt_case(name, k):
    B, th, tw, Cin, Cout, cin_pad, cout_pad = CONVT_CASES[name]
    g = torch.Generator(device='cpu').manual_seed(B + th * tw + Cin + k)
    x = rnd22(torch.randn((B, th, tw, cin_pad), generator=g))
    if cin_pad > Cin:
        x[..., Cin:] = rnd22(50.0 * torch.randn((B, th, tw, cin_pad - Cin), generator=g) + 7.0)
    w = rnd22(torch.randn((Cin, Cout, k, k), generator=g) / math.sqrt(Cin))
    b = torch.randn(Cout, generator=g)
    ref = F.conv_transpose2d(x[..., :Cin].double().permute(0, 3, 1, 2), w.double(), b.double(), stride=k).permute(0, 2, 3, 1).contiguous()
    return dict(x=x, w=w, b=b, ref=ref)


@pytest.mark.parametrize('cfg', CONVT_CFGS)
@pytest.mark.parametrize('k', [4, 2])
@pytest.mark.parametrize('name', list(CONVT_CASES))
def test_conv_transpose_split_fp16(gpu, name, k, cfg, monkeypatch):
    """EPI_CONVT (ConvTranspose2d, kernel = stride = k, as the head's act_postprocess runs it) with weights and bias from the device packers (PACK_CONVT,
    pack_convt_bias_kernel: bit-equal to their Python statement): every output pixel and channel against fp64 F.conv_transpose2d within X3_TOL, the padding
    channels co >= Cout exactly zero, and not a byte outside [B][k th][k tw][ldo] touched (sentinel guards on both sides; the extent itself starts as
    sentinels too, so a pixel the scatter misses shows)."""
    from dust3r_amd import ops
    B, th, tw, Cin, Cout, cin_pad, cout_pad = CONVT_CASES[name]
    c = convt_case(name, k)
    pin_tile(monkeypatch, cfg)
    wp = ops.pack_conv_weight_device(c['w'].to(gpu), cin_pad=cin_pad, transposed=True, cout_pad=cout_pad)
    bp = ops.pack_convt_bias_device(c['b'].to(gpu), k, cout_pad)
    assert torch.equal(bits(wp.cpu()), bits(ops.pack_x3(ops.pad_rows(convt_weight_rows(c['w'], cin_pad, cout_pad))))), 'device packer (PACK_CONVT) != Python statement'
    assert torch.equal(bp.cpu(), ops.pad_rows(convt_bias_rows(c['b'], k, cout_pad))), 'pack_convt_bias != Python statement'
    G, n = 4096, B * k * th * k * tw * cout_pad * 2                       # storage elements (fp16): guard, extent
    buf = torch.full((G + n + G,), SENT, dtype=torch.float16, device=gpu)
    out = ops.convt_gemm(c['x'].to(gpu), wp, bp, k, cout_pad, cin_pad=cin_pad, out=buf[G:])
    assert bool((buf[:G] == SENT).all()) and bool((buf[G + n:] == SENT).all()), 'stores outside the output extent'
    err = relmax(out[..., :Cout], c['ref'])
    print(f'convt x3 {name} k={k} cfg={cfg}: rel err {err:.2e}')
    assert out.shape[:3] == c['ref'].shape[:3] and err < X3_TOL
    assert bool((out[..., Cout:] == 0).all())
    if cout_pad > Cout:
        assert bool((bits(buf[G:G + n]).view(-1, 2 * cout_pad // 16, 2, 8)[:, Cout // 8:] == 0).all()), 'padding channels are not zero'


# ---------------------------------------------------------------------------------------------------------------- the head's tail
def check_post(tag, pts, conf, pre, delta, post):
    """pts (npix, 3), conf (npix,) of a kernel against the fp64 postprocess of the reference pre-activation `pre` (npix, 4) under the derived bound
    (module docstring); everything on the device of `pts`."""
    pre = pre.to(pts.device)
    p0, c0 = postprocess64(pre, post)
    bp, bc = postprocess_bound(pre, delta, post)
    ep, ec = (pts.double() - p0).abs(), (conf.double() - c0).abs()
    print(f'{tag} {post}: pts err / bound {float((ep / bp[:, None]).max()):.3f} (bound <= {float(bp.max()):.2e}), conf err / bound {float((ec / bc).max()):.3f} '
          f'(bound <= {float(bc.max()):.2e})')
    assert bool((ep <= bp[:, None]).all()), (tag, post, 'pts')
    assert bool((ec <= bc).all()), (tag, post, 'conf')


def assert_scale(pre):
    """the scale the tolerance derivation assumes, checked on the fp64 reference"""
    assert float(pre[..., :3].double().norm(dim=-1).max()) <= 3.0 and float(pre[..., 3].abs().max()) <= 4.0


def outputs(npix, strides, device):
    """(record buffer or None, pts, conf): separate tensors for strides (3, 1); for (8, 8) the packed records [pts1 conf1 pts2 conf2], pre-filled with sentinels"""
    if strides == (3, 1):
        return None, None, None
    rec = torch.full((npix, 8), SENT, dtype=torch.float32, device=device)
    return rec, rec.view(-1), rec.view(-1)[3:]


TAIL_GEOM = {   # tile shape -> (D3R_GEMM_CFG, B, H, W)
    # 384 pixels: below one tile; conv_head4 forces the four-wave 256 x 128 shape for every pixel count the heuristic does not give the 512 x 128 tile
    'r256': ('auto', 1, 16, 24),
    # The heuristic picks 512 x 128 from 512 tiles on (gemm_plan.hpp gemm_plan: cdiv(M, 512) >= 512, i.e. M >= 261 633 pixels). Such an image is 134 MB of input
    # rows and a 77 GFLOP fp64 reference convolution (seconds on the CPU, gigabytes of im2col): too large for a test of a few seconds, so the shape is pinned
    # with D3R_GEMM_CFG: 960 pixels = one full tile and a ragged one (448 rows)
    't512': ('3', 1, 24, 40),
}


@functools.lru_cache(maxsize=None)
def tail_case(tile, C):
    _, B, H, W = TAIL_GEOM[tile]
    g = torch.Generator(device='cpu').manual_seed(H * W + C)
    x = rnd22(torch.randn((B, H, W, 128), generator=g))
    w = rnd22(torch.randn((C, 128, 3, 3), generator=g) / math.sqrt(128 * 9))
    b = 0.3 * torch.randn(C, generator=g)
    w4 = 0.8 * torch.randn((4, C), generator=g) / math.sqrt(C)
    b4 = 0.1 * torch.randn(4, generator=g)
    feat = F.conv2d(x.double().permute(0, 3, 1, 2), w.double(), b.double(), padding=1).permute(0, 2, 3, 1).clamp_min(0).reshape(-1, C)
    pre = feat @ w4.double().T + b4.double()
    assert_scale(pre)
    return dict(x=x, w=w, b=b, w4=w4, b4=b4, pre=pre)


@pytest.mark.parametrize('strides', [(3, 1), (8, 8)])
@pytest.mark.parametrize('C', [128, 64])
@pytest.mark.parametrize('tile', list(TAIL_GEOM))
def test_head_tail_fused_and_two_kernel(gpu, tile, C, strides, monkeypatch):
    """3x3 128 -> C + ReLU + 1x1 C -> 4 + postprocess: the fused launch (EPI_HEAD4, both tile shapes) and the conv + head_final_kernel route, each against the
    SAME fp64 reference in all three depth modes x both conf modes (with and without finite bounds), and against each other within 2e-5 per pixel. C = 64: the
    columns >= C of the 128-wide tile must not enter the 1x1 sum. Strides (8, 8): the packed records; the other four floats of every record keep their sentinel."""
    from dust3r_amd import ops
    c = tail_case(tile, C)
    pin_tile(monkeypatch, TAIL_GEOM[tile][0])
    x, b, w4, b4 = (c[k].to(gpu) for k in ('x', 'b', 'w4', 'b4'))
    wp = ops.pack_conv_weight_device(c['w'].to(gpu))
    npix = x.shape[0] * x.shape[1] * x.shape[2]
    h2 = ops.conv2d_nhwc_x(x, wp, b, C, 3, 1, 1, relu=True).reshape(npix, C)          # the two-kernel route's 22-bit map
    delta = X3_TOL * float(c['pre'].abs().max())
    for post in POST_MODES:
        rec_f, pts, conf = outputs(npix, strides, gpu)
        launched, pts_f, conf_f = ops.conv_head4(x, wp, b, w4, b4, C, post, strides, pts=pts, conf=conf)
        assert launched, 'conv_head4 declined a 3x3 convolution to <= 128 channels'
        rec_2, pts, conf = outputs(npix, strides, gpu)
        pts_2, conf_2 = ops.head_final(h2, w4, b4, post, strides, pts=pts, conf=conf)
        check_post(f'fused tail {tile} C={C} {strides}', pts_f, conf_f, c['pre'], delta, post)
        check_post(f'two-kernel tail {tile} C={C} {strides}', pts_2, conf_2, c['pre'], delta, post)
        rel = float(((pts_f - pts_2).norm(dim=-1) / pts_2.norm(dim=-1).clamp_min(1e-8)).max())
        print(f'fused vs two-kernel {tile} C={C} {post}: max per-pixel rel diff {rel:.2e}')
        assert rel < 2e-5 and float(((conf_f - conf_2).abs() / conf_2).max()) < 1e-5
        for rec in (rec_f, rec_2):
            assert rec is None or bool((rec[:, 4:] == SENT).all()), 'the second view of a packed record was written'


def test_head_tail_declines_what_no_wave_can_hold(gpu):
    """conv_head4 answers D3R_DECLINED, and writes nothing, for more than 128 channels, a channel count that is no multiple of 4, another kernel size and a
    precision mode without the tile -- so that 'not launched' cannot pass for 'launched'."""
    from dust3r_amd import ops
    c = tail_case('r256', 128)
    x = c['x'].to(gpu)
    for Cout, k, dtype in ((256, 3, 'fp16x3'), (66, 3, 'fp16x3'), (128, 1, 'fp16x3'), (128, 3, 'bf16')):
        w = torch.zeros((Cout, 128, k, k), device=gpu)
        wp = ops.pack_conv_weight_device(w, dtype=dtype)
        rec, pts, conf = outputs(384, (8, 8), gpu)
        launched, _, _ = ops.conv_head4(x, wp, None, torch.zeros((4, Cout), device=gpu), torch.zeros(4, device=gpu), Cout, strides=(8, 8), k=k, dtype=dtype, pts=pts, conf=conf)
        torch.cuda.synchronize()
        assert not launched and bool((rec == SENT).all()), (Cout, k, dtype)


HEAD_FINAL_DTYPES = ['fp32', 'bf16', 'fp16', 'fp16x3']
BIG = 16 * 65536 + 21       # pixels past 65536 blocks of 16: the grid-stride loop


@functools.lru_cache(maxsize=None)
def head_final_case(C, npix):
    g = torch.Generator(device='cpu').manual_seed(C + npix % 1000)
    feat = torch.randn((npix, C), generator=g).clamp_min(0)
    w4 = 0.5 * torch.randn((4, C), generator=g) / math.sqrt(C)
    b4 = 0.1 * torch.randn(4, generator=g)
    assert_scale(feat.double() @ w4.double().T + b4.double())
    return feat, w4, b4


@pytest.mark.parametrize('dtype', HEAD_FINAL_DTYPES)
@pytest.mark.parametrize('C,npix', [(128, 37), (64, 37), (8, 37), (256, 37), (8, BIG)])
def test_head_final(gpu, C, npix, dtype):
    """head_final_kernel alone: the hoisted weights (C = 128), lanes 8-15 of a pixel's sixteen masked (64), one live lane (8), the non-hoisted loop (256);
    37 pixels = three blocks, the last with dead lane groups under the DPP row sum; 16 x 65536 + 21 pixels: the grid-stride loop past the block cap.
    Reference: fp64 on the features already rounded to the dtype."""
    from dust3r_amd import _lib, ops
    feat, w4, b4 = head_final_case(C, npix)
    feat = (rnd22(feat) if dtype == 'fp16x3' else feat.to(_lib.TORCH_DTYPE[_lib.DTYPES[dtype]]).float()).to(gpu)
    w4, b4 = w4.to(gpu), b4.to(gpu)
    pre = feat.double() @ w4.double().T + b4.double()
    tol = X3_TOL if dtype == 'fp16x3' else OUT_TOL[_lib.TORCH_DTYPE[_lib.DTYPES[dtype]]]
    delta = tol * float(pre.abs().max())
    for post, strides in ((('exp', 'exp', 1.0, INF), (3, 1)), (('linear', 'sigmoid', 1.0, 10.0), (8, 8)), (('square', 'exp', 0.5, 3.0), (3, 1))):
        rec, pts, conf = outputs(npix, strides, gpu)
        pts, conf = ops.head_final(feat, w4, b4, post, strides, dtype=dtype, pts=pts, conf=conf)
        check_post(f'head_final {dtype} C={C} npix={npix}', pts, conf, pre, delta, post)
        assert rec is None or bool((rec[:, 4:] == SENT).all())


@pytest.mark.parametrize('B,th,tw,ps', [(2, 3, 5, 4), (1, 2, 3, 16), (1, 129, 128, 16)])
def test_linear_head_post(gpu, B, th, tw, ps):
    """linear_head_post_kernel against fp64 F.pixel_shuffle + postprocess; 129 x 128 tokens at patch size 16 are 4 227 072 pixels, past 16384 blocks of 256:
    its grid-stride loop. The 'linear' depth mode is a permutation of the input: exact."""
    from dust3r_amd import ops
    g = torch.Generator(device='cpu').manual_seed(B * th * tw + ps)
    feat = (0.45 * torch.randn((B * th * tw, 4 * ps * ps), generator=g)).to(gpu)
    pre = F.pixel_shuffle(feat.view(B, th, tw, 4 * ps * ps).permute(0, 3, 1, 2), ps).permute(0, 2, 3, 1).reshape(-1, 4)
    assert_scale(pre)
    npix = pre.shape[0]
    delta = X3_TOL * float(pre.abs().max())
    big = npix > 1 << 20
    modes = [(('exp', 'exp', 1.0, INF), (3, 1)), (('linear', 'sigmoid', 1.0, 10.0), (8, 8))] if big else [(p, s) for p in POST_MODES for s in ((3, 1), (8, 8))]
    for post, strides in modes:
        rec, pts, conf = outputs(npix, strides, gpu)
        pts, conf = ops.linear_head_post(feat, B, th, tw, ps, post, strides, pts=pts, conf=conf)
        check_post(f'linear_head_post {B}x{th}x{tw} ps={ps} {strides}', pts, conf, pre, delta, post)
        if post[0] == 'linear':
            assert torch.equal(pts, pre[:, :3])
        assert rec is None or bool((rec[:, 4:] == SENT).all())
