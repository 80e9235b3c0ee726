"""CPU pins of the reference that tests/test_gemm_heads_gpu.py holds the attention-projection epilogue to (oracle/heads_ref.py), and of the input
conditions its folded-LayerNorm bound relies on. No device."""
import ctypes as C

import numpy as np
import torch

from oracle.croco_ref.models.pos_embed import RoPE2D
from oracle.heads_ref import fold_inputs, heads_ref, layernorm_stats, rope_angles, rope_table_bound, rope_table_emulated

FOLD_SHAPES = [(50, 2, 3), (3, 8, 12), (1, 21, 32)]      # the shapes of the GPU fold cases


def _positions(B, th, tw):
    yy, xx = torch.meshgrid(torch.arange(th), torch.arange(tw), indexing='ij')
    return torch.stack((yy.flatten(), xx.flatten()), dim=-1)[None].expand(B, -1, -1).contiguous()


def test_reference_equals_linear_reshape_rope2d():
    """heads_ref == nn.Linear -> croco's reshape -> RoPE2D in fp64 to 1e-12, for a self-attention qkv (blocks.py Attention: qkv.reshape(B, N, 3, H, D)
    .transpose(1, 3)) and a cross-attention k | v (CrossAttention: projk / projv .reshape(B, Nk, H, D).permute(0, 2, 1, 3)), th != tw, a per-column
    bias. RoPE2D forms its angles in fp32: the comparison feeds heads_ref that module's own angles (its cos / sin, bit for bit, through the table
    it caches), which pins the layout, the halves, the pairs, ty / tx and the bias-before-rotation order; the angle FORMULA is pinned separately below."""
    torch.manual_seed(3)
    for (B, th, tw, H, K) in [(3, 4, 6, 2, 64), (2, 5, 3, 4, 32)]:
        ntok, Cc = th * tw, H * 64
        pos = _positions(B, th, tw)
        rope = RoPE2D(freq=100.0)
        cos, sin = rope.get_cos_sin(32, max(th, tw), torch.device('cpu'), torch.float64)

        ang = (cos[:, :16], sin[:, :16])
        x = torch.randn(B * ntok, K, dtype=torch.float64)
        # self-attention: one Linear(K, 3 C)
        qkv = torch.nn.Linear(K, 3 * Cc).double()
        with torch.no_grad():
            qkv.bias.copy_(torch.randn(3 * Cc) * 2)
            t = qkv(x).reshape(B, ntok, 3, H, 64).transpose(1, 3)
            q, k, v = rope(t[:, :, 0], pos), rope(t[:, :, 1], pos), t[:, :, 2]
            got = heads_ref(x, qkv.weight, qkv.bias, ['rope', 'rope', 'vt'], Cc, ntok, tw, cos_sin=ang)
        for a, b_ in zip(got, (q, k, v.transpose(-1, -2))):
            assert a.shape == b_.shape and float((a - b_).abs().max()) < 1e-12
        # cross-attention: projk and projv as one k | v launch
        pk, pv = torch.nn.Linear(K, Cc).double(), torch.nn.Linear(K, Cc).double()
        with torch.no_grad():
            kk = rope(pk(x).reshape(B, ntok, H, 64).permute(0, 2, 1, 3), pos)
            vv = pv(x).reshape(B, ntok, H, 64).permute(0, 2, 1, 3)
            got = heads_ref(x, torch.cat((pk.weight, pv.weight)), torch.cat((pk.bias, pv.bias)), ['rope', 'vt'], Cc, ntok, tw, cos_sin=ang)
            plain = heads_ref(x, pv.weight, pv.bias, ['plain'], Cc, ntok, tw)
        assert float((got[0] - kk).abs().max()) < 1e-12 and float((got[1] - vv.transpose(-1, -2)).abs().max()) < 1e-12
        assert float((plain[0] - vv).abs().max()) < 1e-12


def test_reference_angles_against_rope2d_and_the_table_formula():
    """The exact angles heads_ref rotates with by default, pos F0 / base^(i/16), against (a) the cos / sin RoPE2D caches and (b) the restatement of the
    table kernel's formula: both within the derived bound pos inv_freq 2^-23 + 2^-24 (oracle/heads_ref.py rope_table_bound) -- so a GPU comparison
    against the exact angles is a comparison with the reference's arithmetic up to that, stated, amount."""
    for base in (100.0, 10000.0):
        ang, bound = rope_angles(64, base), rope_table_bound(64, base)
        cos, sin = RoPE2D(freq=base).get_cos_sin(32, 64, torch.device('cpu'), torch.float64)
        # RoPE2D rounds inv_freq = 1 / base^(i/16) through two more fp32 operations (the power, the reciprocal): 2^-23 more on the angle
        slack = ang * 2.0 ** -23
        assert bool(((cos[:, :16] - ang.cos()).abs() <= bound + slack).all()) and bool(((sin[:, :16] - ang.sin()).abs() <= bound + slack).all())
        assert torch.equal(cos[:, :16], cos[:, 16:])      # the (c, c + 16) pair shares one angle
        tab = torch.from_numpy(rope_table_emulated(64, base)).double()
        assert bool(((tab[..., 0] - ang.cos()).abs() <= bound).all()) and bool(((tab[..., 1] - ang.sin()).abs() <= bound).all())
        assert float((tab[..., 0] - ang.cos()).abs().max()) > 0      # (and it is not the same computation twice)


def test_reference_fold_identity_and_input_conditions():
    """The folded form the kernel evaluates, rstd (x (W diag(gamma))^T - mean colsum) + (b + W beta), equals LN(x; gamma, beta) W^T + b in fp64; and the
    fold cases' inputs satisfy what the GPU bound assumes: |mean| <= 2 std on every non-constant row, the constant rows have std exactly 0 in fp64 and
    (sum, sum of squares) partials that are exact in fp32, and the rows are exactly representable in split-fp16 after the test's pre-rounding."""
    from dust3r_amd import ops
    for i, (B, th, tw) in enumerate(FOLD_SHAPES):
        for K, head_c in ((128, 128), (256, 256)):
            const_rows = 4 if (B, th, tw) == (3, 8, 12) else 0
            x, gamma, beta, W, b = fold_inputs(B, th, tw, K, head_c, seed=100 + i, const_rows=const_rows)
            x = ops.unpack_x3(ops.pack_x3(x))
            assert torch.equal(ops.unpack_x3(ops.pack_x3(x)), x)
            M = x.shape[0]
            mean, rstd = layernorm_stats(x, 1e-6)
            std = x.double().std(dim=-1, unbiased=False)
            live = slice(0, M - const_rows)
            assert bool((mean[live].abs() <= 2 * std[live]).all()), float((mean[live].abs() / std[live]).max())
            if const_rows:
                assert bool((std[M - const_rows:] == 0).all()) and bool((rstd[M - const_rows:] == 1e-6 ** -0.5).all())
                part = x[M - const_rows:].view(const_rows, K // 32, 32)
                assert torch.equal(part.sum(-1).double(), part.double().sum(-1)) and torch.equal((part * part).sum(-1).double(), (part.double() ** 2).sum(-1))
            Wg = (W.double() * gamma.double())
            folded = rstd[:, None] * (x.double() @ Wg.T - mean[:, None] * Wg.sum(-1)[None, :]) + (b.double() + W.double() @ beta.double())
            direct = torch.nn.functional.layer_norm(x.double(), (K,), gamma.double(), beta.double(), 1e-6) @ W.double().T + b.double()
            assert float((folded - direct).abs().max() / direct.abs().max()) < 1e-12
            got = heads_ref(x, W, b, ['rope', 'rope', 'vt'], head_c, th * tw, tw, ln=(gamma, beta, 1e-6))
            want = heads_ref(None, None, None, ['rope', 'rope', 'vt'], head_c, th * tw, tw, y=direct)
            for a, c in zip(got, want):
                assert float((a - c).abs().max()) < 1e-12
            # unequal region scales and a per-column bias: what makes a region mix-up or a bias-after-rotation visible
            rms = [float(W[r * head_c:(r + 1) * head_c].pow(2).mean().sqrt()) for r in range(3)]
            assert rms[1] < 0.6 * rms[0] and rms[2] > 1.7 * rms[0] and float(b.std()) > 0.5


def test_heads_entry_points_reject_bad_arguments():
    """d3r_linear_heads / d3r_linear_heads_tile_config / d3r_rope_table argument checks (host side: they return before any launch)."""
    from dust3r_amd import _lib
    lib = _lib.lib
    assert {'d3r_linear_heads', 'd3r_linear_heads_tile_config', 'd3r_rope_table'} <= set(_lib.EXPORTED)
    x3 = _lib.DTYPE_F16X3
    kinds = (C.c_int * 3)(_lib.HEAD_ROPE, _lib.HEAD_ROPE, _lib.HEAD_VT)
    cfg = lambda M=96, K=128, nreg=3, head_c=128, kk=kinds, heads=2, ntok=24, tok_w=6, ldv=64, max_pos=512, dt=x3: \
        lib.d3r_linear_heads_tile_config(M, K, nreg, head_c, kk, heads, ntok, tok_w, ldv, max_pos, dt)      # noqa: E731
    assert cfg() >= 0
    assert cfg(heads=3) == -1 and cfg(M=100) == -1 and cfg(tok_w=5) == -1 and cfg(max_pos=5) == -1 and cfg(ldv=32) == -1 and cfg(ldv=96) == -1
    assert cfg(nreg=0) == -1 and cfg(nreg=4) == -1 and cfg(dt=9) == -1 and cfg(kk=(C.c_int * 3)(1, 4, 2)) == -1 and cfg(kk=None) == -1
    assert cfg(ntok=96, tok_w=12, ldv=128, max_pos=12) >= 0 and cfg(ntok=96, tok_w=12, ldv=128, max_pos=11) == -1      # max(ntok / tok_w, tok_w) against the table's rows
    buf = (C.c_float * 64)()
    dsts = (C.c_void_p * 3)(C.addressof(buf), C.addressof(buf), C.addressof(buf))
    call = lambda act=buf, wgt=buf, dd=dsts, tab=buf, rstd=None, nmr=None, cs=None, dt=x3, **kw: lib.d3r_linear_heads(      # noqa: E731
        act, wgt, None, kw.get('M', 96), 128, 3, 128, kinds, dd, kw.get('heads', 2), 24, 6, kw.get('ldv', 64), tab, 512, rstd, nmr, cs, None, 1e-6, None, 0, None, 0, dt, None)
    assert call(act=None) == -1 and call(wgt=None) == -1 and call(dd=None) == -1 and call(tab=None) == -1
    assert call(dd=(C.c_void_p * 3)(C.addressof(buf), None, C.addressof(buf))) == -1
    assert call(heads=3) == -1 and call(M=100) == -1 and call(ldv=100) == -1
    assert call(rstd=buf) == -1 and call(rstd=buf, nmr=buf, cs=buf, dt=_lib.DTYPE_F16) == -1      # statistics: all three, split-fp16 only
    assert lib.d3r_rope_table(None, 8, 100.0, 1.0, None) == -1 and lib.d3r_rope_table(buf, 0, 100.0, 1.0, None) == -1


def test_heads_tile_config_reports_ignored_pins(monkeypatch):
    """The feasibility rules of the header as the host function reports them: an infeasible D3R_GEMM_CFG is ignored, and the query shows it."""
    from dust3r_amd import ops
    q = lambda dt, ntok, tw, head_c=256, B=2: ops.heads_tile_config(B * ntok, 128, ['rope', 'rope', 'vt'], head_c, ntok, tw, (ntok + 63) // 64 * 64, dt)      # noqa: E731
    monkeypatch.delenv('D3R_GEMM_NOWIDE', raising=False)
    monkeypatch.setenv('D3R_GEMM_T128W8', '0')
    for pin, want in (('0', 0), ('1', 1), ('8', 8)):
        monkeypatch.setenv('D3R_GEMM_CFG', pin)
        assert q('fp16x3', 96, 12) == want
    monkeypatch.setenv('D3R_GEMM_CFG', '1')
    assert q('fp16x3', 96, 12, head_c=128) != 1      # a 256-wide tile would span two regions
    for pin in ('2', '3', '7', '9', '11'):
        monkeypatch.setenv('D3R_GEMM_CFG', pin)
        assert q('fp16x3', 64, 8) != int(pin) and q('fp32', 64, 8) != int(pin) and q('fp16f8', 64, 8) != int(pin)
    for pin in ('2', '3'):
        monkeypatch.setenv('D3R_GEMM_CFG', pin)
        assert q('bf16', 64, 8) == int(pin) and q('fp16', 64, 8) == int(pin) and q('bf16', 96, 12) != int(pin)
        monkeypatch.setenv('D3R_GEMM_NOWIDE', '1')
        assert q('bf16', 64, 8) != int(pin)
        monkeypatch.delenv('D3R_GEMM_NOWIDE')
    monkeypatch.setenv('D3R_GEMM_CFG', '8')
    assert q('bf16', 64, 8) == 0 and q('fp16x2f8', 64, 8) == 0      # the 64 x 64 tile exists in split-fp16 only
    monkeypatch.setenv('D3R_GEMM_CFG', '0')
    monkeypatch.setenv('D3R_GEMM_T128W8', '1000000')
    assert q('fp16x3', 96, 12) == 12 and q('fp16', 96, 12) == 0      # eight waves: split-fp16 only
