"""CPU tests of the fp64 restatements that tests/test_dpt_head_gpu.py holds the DPT head's kernels to: a reference that is wrong in the same
way as a kernel pins nothing. The postprocess formulas (dust3r/heads/postprocess.py:10-58, csrc/common.hpp postprocess_store) are checked against
the reference's own outputs (tests/golden/forward_post_modes.pt) and against values computed by hand; the statement of the weight-row layouts of the
transposed convolution (csrc/elementwise.hip PACK_CONVT, pack_convt_bias_kernel) against a direct loop and against F.conv_transpose2d."""
import math
import os

import torch
import torch.nn.functional as F

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
INF = float('inf')
DEPTH_MODES = ('exp', 'linear', 'square')
CONF_MODES = (('exp', 1.0, INF), ('exp', 0.5, 3.0), ('sigmoid', 1.0, 10.0))      # the released checkpoints'; a finite clamp; finite sigmoid bounds
POST_MODES = [(d,) + c for d in DEPTH_MODES for c in CONF_MODES]                    # (depth_mode, conf_mode, vmin, vmax)


def postprocess64(pre, post):
    """pre (..., 4) = (x, y, z, confidence logit) -> (pts (..., 3), conf (...)) in fp64; post = (depth_mode, conf_mode, vmin, vmax)."""
    depth, conf, vmin, vmax = post
    pre = pre.double()
    xyz, cl = pre[..., :3], pre[..., 3]
    if depth == 'linear':
        pts = xyz
    else:
        d = xyz.norm(dim=-1, keepdim=True)
        pts = xyz / d.clamp_min(1e-8) * (torch.expm1(d) if depth == 'exp' else d * d)
    if conf == 'exp':
        c = vmin + cl.exp().clamp_max(vmax - vmin)
    else:
        c = (vmax - vmin) * torch.sigmoid(cl) + vmin
    return pts, c


def ulp32(v):
    """the fp32 unit in the last place of |v| (fp64 tensor)"""
    return torch.exp2(torch.floor(torch.log2(v.abs().clamp_min(2.0 ** -126))) - 23)


def postprocess_bound(pre, delta, post):
    """What a pre-activation error of `delta` (absolute, per coordinate) may become behind the postprocess, per pixel and from the reference alone:
    the largest deviation of the fp64 postprocess over the eight points pre +- delta e_i, doubled, plus 4 fp32 ulp of the result (expm1f / expf).
    Returns (bound of |pts - ref| per component (...), bound of |conf - ref| (...)). depth_mode 'linear' hands the coordinates through: delta itself."""
    pre = pre.double()
    p0, c0 = postprocess64(pre, post)
    dev_p, dev_c = torch.zeros_like(c0), torch.zeros_like(c0)
    for i in range(4):
        for s in (1.0, -1.0):
            q = pre.clone()
            q[..., i] += s * delta
            p, c = postprocess64(q, post)
            dev_p = torch.maximum(dev_p, (p - p0).abs().amax(-1))
            dev_c = torch.maximum(dev_c, (c - c0).abs())
    bound_p = 2 * dev_p + 4 * ulp32(p0.abs().amax(-1))
    if post[0] == 'linear':
        bound_p = torch.full_like(dev_p, delta)
    return bound_p, 2 * dev_c + 4 * ulp32(c0)


def convt_weight_rows(w, cin_pad, cout_pad):
    """ConvTranspose2d weight (Cin, Cout, k, k) -> the GEMM's weight rows (k*k*cout_pad, cin_pad): row (ky*k + kx) * cout_pad + co, column ci; padding zero."""
    Cin, Cout, k, _ = w.shape
    rows = w.new_zeros((k * k, cout_pad, cin_pad))
    rows[:, :Cout, :Cin] = w.permute(2, 3, 1, 0).reshape(k * k, Cout, Cin)
    return rows.reshape(k * k * cout_pad, cin_pad)


def convt_bias_rows(b, k, cout_pad):
    """ConvTranspose2d bias (Cout,) -> (k*k*cout_pad,): one copy per tap, padding zero."""
    rows = b.new_zeros((k * k, cout_pad))
    rows[:, :b.numel()] = b
    return rows.reshape(-1)


def conv_weight_rows(w, cin_pad):
    """Conv2d weight (Cout, Cin, k, k) -> (Cout, k*k*cin_pad) in the K order of d3r_conv2d_nhwc over cin_pad channels, 32 channels per K step (split-fp16
    and fp32 rows: 4 bytes per element): ops.pack_conv_weight of the tensor with its channels zero-padded."""
    from dust3r_amd import ops
    Cout, Cin = w.shape[:2]
    return ops.pack_conv_weight(F.pad(w.float(), (0, 0, 0, 0, 0, cin_pad - Cin)), dtype=torch.float32)[:Cout]


def _golden_cases(config):
    g = torch.load(os.path.join(GOLD, 'forward_post_modes.pt'), weights_only=False)
    cases = [c for c in g['cases'] if c['config'] == config]
    lin = [c for c in cases if c['depth_mode'][0] == 'linear' and tuple(c['conf_mode']) == ('exp', 1, INF)]
    assert len(lin) == 1
    return lin[0], [c for c in cases if c is not lin[0]]


def test_postprocess_restatement_matches_reference_golden():
    """The goldens hold the reference's outputs for five (depth_mode, conf_mode) pairs per head on the SAME weights and views. The ('linear', ('exp', 1, inf))
    case exposes the head's pre-activation: pts3d IS xyz and conf - 1 = exp(logit). From it the restatement must reproduce the other four cases -- 'exp' and
    'square' depth, 'exp' with a finite clamp (reached: conf = vmax on the linear head) and 'sigmoid' -- to the fp32 rounding of the reference's own
    arithmetic (1e-5 of the output scale, the bar tests/test_oracle_pins.py holds the oracle to)."""
    seen, clamped = set(), 0
    for config in ('tiny_dpt', 'tiny_linear'):
        lin, others = _golden_cases(config)
        assert len(others) == 4
        for pk, ck in (('pts3d', 'conf'), ('pts3d_in_other_view', 'conf2')):
            pre = torch.cat((lin[pk].double(), torch.log(lin[ck].double() - 1.0)[..., None]), dim=-1)
            for c in others:
                post = (c['depth_mode'][0],) + tuple(c['conf_mode'])
                pts, conf = postprocess64(pre, post)
                assert float((pts - c[pk].double()).abs().max() / c[pk].abs().max()) < 1e-5, (config, post)
                assert float((conf - c[ck].double()).abs().max() / c[ck].abs().max()) < 1e-5, (config, post)
                seen.add(post[:2])
                clamped += int((c[ck] == c['conf_mode'][2]).sum()) if post[1] == 'exp' else 0
    assert seen == {('exp', 'exp'), ('exp', 'sigmoid'), ('square', 'exp'), ('square', 'sigmoid')} and clamped > 0


def test_postprocess_restatement_hand_values():
    """Every mode at points where the result is known in closed form: |xyz| = 5 (3-4-5), d -> 0 (the 1e-8 floor: no 0 / 0), the cmax clamp."""
    pre = torch.tensor([[3.0, 0.0, 4.0, 0.0], [0.0, 0.0, 0.0, math.log(3.0)], [1e-12, 0.0, 0.0, math.log(10.0)]], dtype=torch.float64)
    e5 = 147.4131591025766      # expm1(5)
    want_pts = {'linear': [[3, 0, 4], [0, 0, 0], [1e-12, 0, 0]],
                'exp': [[0.6 * e5, 0, 0.8 * e5], [0, 0, 0], [1e-4 * 1e-12, 0, 0]],      # d < 1e-8: xyz / 1e-8 * expm1(d), expm1(1e-12) = 1e-12 (1 + 5e-13)
                'square': [[15, 0, 20], [0, 0, 0], [1e-4 * 1e-24, 0, 0]]}
    want_conf = {('exp', 1.0, INF): [2, 4, 11], ('exp', 0.5, 3.0): [1.5, 3.0, 3.0], ('exp', 0.0, 5.0): [1, 3, 5], ('sigmoid', 1.0, 10.0): [5.5, 7.75, 1 + 9 * 10 / 11],
                 ('sigmoid', 0.0, 1.0): [0.5, 0.75, 10 / 11]}
    for depth, wp in want_pts.items():
        for cm, wc in want_conf.items():
            pts, conf = postprocess64(pre, (depth,) + cm)
            assert torch.isfinite(pts).all() and torch.isfinite(conf).all()
            assert torch.allclose(pts, torch.tensor(wp, dtype=torch.float64), rtol=1e-12, atol=0), (depth, pts)
            assert torch.allclose(conf, torch.tensor(wc, dtype=torch.float64), rtol=1e-12, atol=0), (cm, conf)


def test_postprocess_bound_covers_a_pre_activation_error():
    """The tolerance of the nonlinear modes: within the scale the GPU tests keep (|xyz| <= 3, |logit| <= 4) a pre-activation error of up to delta / 2 in every
    coordinate at once stays inside the bound, and the bound stays a small multiple of delta (2 delta e^|xyz| at most, plus the ulps): far below O(0.1)."""
    g = torch.Generator().manual_seed(3)
    pre = (torch.rand((4000, 4), generator=g, dtype=torch.float64) * 2 - 1) * torch.tensor([1.7, 1.7, 1.7, 4.0], dtype=torch.float64)
    delta = 1e-5
    err = (torch.rand((4000, 4), generator=g, dtype=torch.float64) - 0.5) * delta
    for post in POST_MODES:
        bp, bc = postprocess_bound(pre, delta, post)
        p0, c0 = postprocess64(pre, post)
        p1, c1 = postprocess64(pre + err, post)
        assert bool(((p1 - p0).abs() <= bp[:, None]).all()) and bool(((c1 - c0).abs() <= bc).all()), post
        assert float(bp.max()) < 2.5 * delta * math.exp(3.0) + 1e-5 and float(bc.max()) < 2.5 * delta * math.exp(4.0) + 1e-5, post


def test_convt_layout_statement_against_a_direct_loop():
    """convt_weight_rows / convt_bias_rows (what the GPU test compares the device packers with) against the loop of csrc/elementwise.hip, and the GEMM + scatter
    they feed against F.conv_transpose2d(stride = k): out[b, k y + ky, k x + kx, co] = sum_ci in[b, y, x, ci] w[ci, co, ky, kx] + bias[co]."""
    g = torch.Generator().manual_seed(11)
    for Cin, Cout, k, cin_pad, cout_pad in ((3, 5, 2, 8, 8), (4, 4, 4, 4, 4)):
        w = torch.randn((Cin, Cout, k, k), generator=g, dtype=torch.float64)
        b = torch.randn(Cout, generator=g, dtype=torch.float64)
        rows, brow = convt_weight_rows(w, cin_pad, cout_pad), convt_bias_rows(b, k, cout_pad)
        want, bwant = torch.zeros((k * k * cout_pad, cin_pad), dtype=torch.float64), torch.zeros(k * k * cout_pad, dtype=torch.float64)
        for ci in range(Cin):
            for co in range(Cout):
                for ky in range(k):
                    for kx in range(k):
                        want[(ky * k + kx) * cout_pad + co, ci] = w[ci, co, ky, kx]
        for t in range(k * k):
            for co in range(Cout):
                bwant[t * cout_pad + co] = b[co]
        assert torch.equal(rows, want) and torch.equal(brow, bwant)
        B, th, tw = 2, 3, 2
        x = torch.randn((B, th, tw, cin_pad), generator=g, dtype=torch.float64)
        y = (x.reshape(-1, cin_pad) @ rows.T + brow).reshape(B, th, tw, k, k, cout_pad)             # row m = input pixel, column (tap, co)
        out = y.permute(0, 1, 3, 2, 4, 5).reshape(B, th * k, tw * k, cout_pad)                       # (b, y, ky, x, kx, co)
        ref = F.conv_transpose2d(x[..., :Cin].permute(0, 3, 1, 2), w, b, stride=k).permute(0, 2, 3, 1)
        assert torch.allclose(out[..., :Cout], ref, rtol=1e-12, atol=1e-12) and float(out[..., Cout:].abs().max() if cout_pad > Cout else 0.0) == 0.0


def test_conv_layout_statement_against_a_direct_loop():
    """conv_weight_rows (ops.pack_conv_weight over zero-padded channels) against the K order the header states: k = (ci / S) (k k S) + (ky k + kx) S + ci % S."""
    g = torch.Generator().manual_seed(12)
    Cout, Cin, k, cin_pad, S = 3, 40, 3, 64, 32
    w = torch.randn((Cout, Cin, k, k), generator=g)
    rows = conv_weight_rows(w, cin_pad)
    want = torch.zeros((Cout, k * k * cin_pad))
    for co in range(Cout):
        for ci in range(Cin):
            for t in range(k * k):
                want[co, (ci // S) * (k * k * S) + t * S + ci % S] = w[co, ci, t // k, t % k]
    assert torch.equal(rows, want)


def test_head_kernel_entry_points_check_their_arguments_on_the_host():
    """The kernel-level entry points of the DPT head are exported, and refuse what they cannot launch before touching a device: NULL operands, a channel
    count that is no whole K step (the padded-channel case of the GPU test with cin_pad = 24), an unknown flag or postprocess mode -- D3R_ERR_INVALID;
    d3r_conv_head4 on more than 128 channels -- D3R_DECLINED, distinct from both D3R_OK and an error."""
    import ctypes as C
    from dust3r_amd import _lib
    lib = _lib.lib
    names = {'d3r_pack_conv_weight', 'd3r_pack_convt_bias', 'd3r_conv2d_nhwc_x', 'd3r_convt_gemm', 'd3r_conv_head4', 'd3r_head_final', 'd3r_linear_head_post'}
    assert names <= set(_lib.EXPORTED)
    buf = C.create_string_buffer(64)
    p, X3 = C.cast(buf, C.c_void_p), _lib.DTYPE_F16X3
    conv = lambda cin_pad, flags=0, inp=p: lib.d3r_conv2d_nhwc_x(inp, p, None, p, None, None, None, 1, 9, 11, 32, cin_pad, 64, 64, 64, 3, 1, 1, flags, p, X3, None)   # noqa: E731
    assert conv(24) == -1 and conv(32, flags=2) == -1 and conv(32, inp=None) == -1 and _lib.ERRORS[-1] == 'invalid argument'
    assert lib.d3r_pack_conv_weight(p, p, 0, 64, 24, 3, 24, 0, X3, None) == -1 and lib.d3r_pack_conv_weight(p, p, 1, 24, 24, 4, 32, 26, X3, None) == -1
    assert lib.d3r_pack_convt_bias(p, p, 24, 16, 4, None) == -1
    assert lib.d3r_convt_gemm(p, p, p, p, 2, 3, 5, 32, 24, 32, 4, 32, X3, None) == -1 and lib.d3r_convt_gemm(p, p, p, p, 2, 3, 5, 32, 32, 32, 4, 24, X3, None) == -1
    head4 = lambda Cout, depth=0, vmin=1.0: lib.d3r_conv_head4(p, p, None, p, p, p, p, 1, 16, 24, 128, 128, Cout, 3, 3, 1, depth, 0, vmin, INF, p, X3, None)   # noqa: E731
    assert head4(256) == _lib.DECLINED == 1 and head4(66) == _lib.DECLINED and head4(128, depth=3) == -1 and head4(128, vmin=INF) == -1
    assert lib.d3r_head_final(p, 12, p, p, p, p, 37, 3, 1, 0, 0, 1.0, INF, X3, None) == -1 and lib.d3r_head_final(p, 8, p, p, p, p, 37, 3, 1, 0, 1, 1.0, INF, X3, None) == -1
    assert lib.d3r_linear_head_post(p, p, None, 1, 2, 3, 16, 3, 1, 0, 0, 1.0, INF, None) == -1 and lib.d3r_linear_head_post(p, p, p, 1, 2, 3, 16, 2, 1, 0, 0, 1.0, INF, None) == -1
