"""The DPT head's x2 bilinear map interpolated inside the 3x3 convolution that reads it (AMODE_CONV_UP2, csrc/gemm_up2.hip) against the route it replaces:
upsample2x_quad_kernel into memory, then the convolution on the materialised map. The two routes must agree BIT FOR BIT -- the fused kernel evaluates every map
pixel with the stand-alone kernel's arithmetic (csrc/kernels.hpp up2_*) and runs the same MFMA sequence per output element -- so every comparison here is
torch.equal; the interpolation itself is pinned against fp64 by test_kernels_gpu.py::test_upsample2x_split_fp16 and the convolution + tail by
test_dpt_head_gpu.py, whose bound (X3_TOL through check_post) is re-asserted on the fused launch.

Two consumers have the fused launch: head.0 (EPI_T: typed store with bias, 256 -> 128 channels, on the x2 map of refinenet-0's output) and head.2 with the fused
head tail (EPI_HEAD4, 128 -> 128, on the x2 map of head.0's output).

Tile: 16 x 32 output pixels. D3R_UP2_MIN_TILES lowers the one-tile-per-compute-unit floor of the dispatch so that small maps reach the kernel."""
import ctypes as C
import functools
import math

import pytest
import torch
import torch.nn.functional as F

from test_dpt_head_cpu import POST_MODES
from test_dpt_head_gpu import SENT, X3_TOL, assert_scale, bits, check_post, outputs, relmax, rnd22

pytestmark = pytest.mark.gpu

# B, Hi, Wi of the low-resolution source -> the map is (2 Hi, 2 Wi)
GEOM = {
    '2x2_tiles': (2, 16, 32),      # 32 x 64: interior seams on both axes, two images
    'one_tile': (1, 8, 16),        # 16 x 32: every halo pixel lies outside the map
    'column_of_tiles': (3, 16, 16),  # 32 x 32: one tile wide, two high, three images
}


@functools.lru_cache(maxsize=None)
def case(name, C_out=128):
    B, Hi, Wi = GEOM[name] if name in GEOM else name
    g = torch.Generator(device='cpu').manual_seed(B * 1000 + Hi * Wi + C_out)
    x = rnd22(torch.randn((B, Hi, Wi, 128), generator=g))
    w = rnd22(torch.randn((C_out, 128, 3, 3), generator=g) / math.sqrt(128 * 9))
    b = 0.3 * torch.randn(C_out, generator=g)
    w4 = 0.8 * torch.randn((4, C_out), generator=g) / math.sqrt(C_out)
    b4 = 0.1 * torch.randn(4, generator=g)
    return dict(x=x, w=w, b=b, w4=w4, b4=b4)


def two_kernel(ops, x, wp, b, w4, b4, C_out, post, strides, gpu):
    """today's route: the map in memory, then conv_head4 on it. The convolution reads the split rows the upsampling kernel stored, as in the engine: through fp32 and
    ops.pack_x3 a value whose lo half was rounded up to half an ulp of hi comes back as another (hi, lo) pair of the same sum (about one element in 4000), and the
    dropped lo x lo terms of the three-MFMA product then differ in the last bit of the sums (measured: 1 % of the output pixels, 4e-8 relative)."""
    rows = ops.upsample2x_x3(x, rows=True)
    npix = rows.shape[0] * rows.shape[1] * rows.shape[2]
    rec, pts, conf = outputs(npix, strides, gpu)
    launched, pts, conf = ops.conv_head4(rows, wp, b, w4, b4, C_out, post, strides, pts=pts, conf=conf, x_rows=True)
    assert launched
    return ops.unpack_x3(rows), rec, pts, conf


@functools.lru_cache(maxsize=None)
def case_t(name):
    B, Hi, Wi = GEOM[name]
    g = torch.Generator(device='cpu').manual_seed(B * 77 + Hi * Wi)
    x = rnd22(torch.randn((B, Hi, Wi, 256), generator=g))
    w = rnd22(torch.randn((128, 256, 3, 3), generator=g) / math.sqrt(256 * 9))
    b = 0.3 * torch.randn(128, generator=g)
    return dict(x=x, w=w, b=b)


@pytest.mark.parametrize('name', list(GEOM))
def test_fused_up2_conv_typed_store_equals_the_two_kernel_route(gpu, name, monkeypatch):
    """x2 + 3x3 256 -> 128 with bias, typed split-fp16 store (EPI_T, as head.0 uses it) in ONE launch against upsample2x_x3 -> conv2d_nhwc_x on the stored rows: the raw
    bits are equal, the result is within X3_TOL of fp64 F.conv2d applied to the map upsample2x_x3 produced, and the sentinels around the output rows -- 8 guard channels
    behind the 128 of every pixel (ldo = 136) -- are untouched by both routes."""
    from dust3r_amd import ops
    monkeypatch.setenv('D3R_UP2_MIN_TILES', '1')
    B, Hi, Wi = GEOM[name]
    assert ops.up2_conv_route(B, Hi, Wi, 256, 128, head4=False), 'whole tiles, floor lowered: the dispatch must pick the fused launch'
    c = case_t(name)
    x, b = c['x'].to(gpu), c['b'].to(gpu)
    wp = ops.pack_conv_weight_device(c['w'].to(gpu))
    guard = lambda: ops.pack_x3(torch.full((B, 2 * Hi, 2 * Wi, 136), SENT, dtype=torch.float32, device=gpu))
    rows = ops.upsample2x_x3(x, rows=True)
    two = ops.conv2d_nhwc_x(rows, wp, b, 128, 3, 1, 1, ldo=136, x_rows=True, out_rows=guard())
    one = ops.up2_conv2d_nhwc_x(x, wp, b, 128, out_rows=guard(), ldo=136)
    assert torch.equal(bits(one), bits(two))
    val = ops.unpack_x3(one)
    assert bool((val[..., 128:] == SENT).all()) and bool((ops.unpack_x3(two)[..., 128:] == SENT).all()), 'guard channels written'
    ref = F.conv2d(ops.unpack_x3(rows).cpu().double().permute(0, 3, 1, 2), c['w'].double(), c['b'].double(), padding=1).permute(0, 2, 3, 1)
    err = relmax(val[..., :128], ref)
    print(f'fused x2 + conv typed store {name}: rel err {err:.2e}')
    assert err < X3_TOL


def test_typed_store_entry_point_falls_back(gpu, monkeypatch):
    """24 x 32 is not whole tiles: the host query reports the two launches, the entry point runs them through its scratch map, same bits as the explicit route."""
    from dust3r_amd import ops
    monkeypatch.setenv('D3R_UP2_MIN_TILES', '1')
    assert not ops.up2_conv_route(1, 12, 16, 256, 128, head4=False)
    g = torch.Generator(device='cpu').manual_seed(5)
    x = rnd22(torch.randn((1, 12, 16, 256), generator=g)).to(gpu)
    wp = ops.pack_conv_weight_device(rnd22(torch.randn((128, 256, 3, 3), generator=g) / 48.0).to(gpu))
    b = torch.randn(128, generator=g).to(gpu)
    zeros = lambda: ops.pack_x3(torch.zeros((1, 24, 32, 128), device=gpu))
    two = ops.conv2d_nhwc_x(ops.upsample2x_x3(x, rows=True), wp, b, 128, 3, 1, 1, x_rows=True, out_rows=zeros())
    one = ops.up2_conv2d_nhwc_x(x, wp, b, 128, out_rows=zeros())
    assert torch.equal(bits(one), bits(two))


@pytest.mark.parametrize('post', POST_MODES)
@pytest.mark.parametrize('name', list(GEOM))
def test_fused_up2_conv_head4_equals_the_two_kernel_route(gpu, name, post, monkeypatch):
    """x2 + 3x3 128 -> 128 + ReLU + 1x1 + postprocess in ONE launch, every postprocess mode, packed records (8, 8): bit-equal to upsample2x_x3 -> conv_head4, the
    other half of every record keeps its sentinel, and (first mode only: the reference convolution is the expensive part) within the derived bound of the fp64
    reference computed from the map upsample2x_x3 produced."""
    from dust3r_amd import ops
    monkeypatch.setenv('D3R_UP2_MIN_TILES', '1')
    B, Hi, Wi = GEOM[name]
    assert ops.up2_conv_route(B, Hi, Wi, 128, 128), 'whole tiles, floor lowered: the dispatch must pick the fused launch'
    c = case(name)
    x, b, w4, b4 = (c[k].to(gpu) for k in ('x', 'b', 'w4', 'b4'))
    wp = ops.pack_conv_weight_device(c['w'].to(gpu))
    up, rec_2, pts_2, conf_2 = two_kernel(ops, x, wp, b, w4, b4, 128, post, (8, 8), gpu)
    npix = B * 4 * Hi * Wi
    rec_f, pts, conf = outputs(npix, (8, 8), gpu)
    launched, pts_f, conf_f = ops.up2_conv_head4(x, wp, b, w4, b4, 128, post, (8, 8), pts=pts, conf=conf)
    assert launched
    assert torch.equal(bits(pts_f.contiguous()), bits(pts_2.contiguous())) and torch.equal(bits(conf_f.contiguous()), bits(conf_2.contiguous()))
    assert bool((rec_f[:, 4:] == SENT).all()), 'the second view of a packed record was written'
    if post == POST_MODES[0]:
        feat = F.conv2d(up.cpu().double().permute(0, 3, 1, 2), c['w'].double(), c['b'].double(), padding=1).permute(0, 2, 3, 1).clamp_min(0).reshape(-1, 128)
        pre = feat @ c['w4'].double().T + c['b4'].double()
        assert_scale(pre)
        check_post(f'fused x2 + conv + tail {name}', pts_f, conf_f, pre, X3_TOL * float(pre.abs().max()), post)


def test_fused_up2_fewer_output_channels(gpu, monkeypatch):
    """C = 64 output channels (the tail must ignore columns >= C) and separate outputs (3, 1): bit-equal."""
    from dust3r_amd import ops
    monkeypatch.setenv('D3R_UP2_MIN_TILES', '1')
    c = case('2x2_tiles', 64)
    x, b, w4, b4 = (c[k].to(gpu) for k in ('x', 'b', 'w4', 'b4'))
    wp = ops.pack_conv_weight_device(c['w'].to(gpu))
    assert ops.up2_conv_route(2, 16, 32, 128, 64)
    _, _, pts_2, conf_2 = two_kernel(ops, x, wp, b, w4, b4, 64, POST_MODES[0], (3, 1), gpu)
    launched, pts_f, conf_f = ops.up2_conv_head4(x, wp, b, w4, b4, 64, POST_MODES[0], (3, 1))
    assert launched and torch.equal(bits(pts_f), bits(pts_2)) and torch.equal(bits(conf_f), bits(conf_2))


@pytest.mark.parametrize('geom,floor', [((1, 12, 16), '1'), ((1, 8, 16), None)])
def test_entry_point_falls_back_where_the_tile_grid_does_not_fit(gpu, geom, floor, monkeypatch):
    """24 x 32 is not whole 16-row tiles; one tile is fewer than one per compute unit (no floor override): the host query reports the two-launch route, the entry
    point runs it through its scratch map, and the results are those of the explicit two-kernel route."""
    from dust3r_amd import ops
    if floor is None:
        monkeypatch.delenv('D3R_UP2_MIN_TILES', raising=False)
    else:
        monkeypatch.setenv('D3R_UP2_MIN_TILES', floor)
    B, Hi, Wi = geom
    assert not ops.up2_conv_route(B, Hi, Wi, 128, 128)
    c = case(geom)
    x, b, w4, b4 = (c[k].to(gpu) for k in ('x', 'b', 'w4', 'b4'))
    wp = ops.pack_conv_weight_device(c['w'].to(gpu))
    _, _, pts_2, conf_2 = two_kernel(ops, x, wp, b, w4, b4, 128, POST_MODES[0], (3, 1), gpu)
    launched, pts_f, conf_f = ops.up2_conv_head4(x, wp, b, w4, b4, 128, POST_MODES[0], (3, 1))
    assert launched and torch.equal(bits(pts_f), bits(pts_2)) and torch.equal(bits(conf_f), bits(conf_2))


def test_engine_forward_is_bit_identical_and_skips_the_map(gpu, monkeypatch):
    """The tiny DPT model on 32 x 64 images (head maps of whole tiles; the tile floor lowered): the four forward outputs are equal between D3R_HEAD_UPFUSE=0 and the
    default, and the profiled forward of the default arm has four "other" launches (kind 17) fewer -- per head, neither the x2 map of refinenet-0's output nor that
    of head.0's output is launched."""
    from dust3r_amd._lib import lib
    from oracle.dust3r_ref import build_ref_model
    from test_forward_gpu import engine_from_oracle
    from dust3r_amd.synthetic import synthetic_views
    monkeypatch.setenv('D3R_UP2_MIN_TILES', '1')
    eng = engine_from_oracle(build_ref_model('tiny_dpt'), 'tiny_dpt', 'fp16x3', gpu)
    v1, v2 = synthetic_views(2, 32, 64, seed=5)
    out, other = {}, {}
    for arm in ('0', '1'):
        monkeypatch.setenv('D3R_HEAD_UPFUSE', arm)
        e1, e2 = eng(v1, v2)
        out[arm] = [t.clone() for t in (e1['pts3d'], e2['pts3d_in_other_view'], e1['conf'], e2['conf'])]
        lib.d3r_model_set_option(eng._engine, 1, 1)
        eng(v1, v2)
        torch.cuda.synchronize()
        n, ms, work = C.c_int(), C.c_double(), C.c_double()
        assert lib.d3r_model_profile_read(eng._engine, 17, C.byref(n), C.byref(ms), C.byref(work)) == 0
        lib.d3r_model_set_option(eng._engine, 1, 0)
        other[arm] = n.value
    for a, b in zip(out['1'], out['0']):
        assert torch.equal(bits(a), bits(b))
    assert other['0'] - other['1'] == 4, other
