"""oracle/heads_ref.py -- TEST INFRASTRUCTURE ONLY.

What one attention-projection launch of the engine (d3r_linear_heads: the GEMM with its head-scatter epilogue, csrc/gemm.hip EPI_HEADS) has to
compute, in plain fp64: the nn.Linear of croco's Attention / CrossAttention (qkv, projq, projk | projv), optionally behind the block's LayerNorm,
the split into regions and heads, croco's RoPE2D on the q / k regions, and the layouts the attention kernel reads. tests/test_gemm_heads_cpu.py pins
it against nn.Linear + reshape + oracle.croco_ref RoPE2D; tests/test_gemm_heads_gpu.py holds the kernel to it.
"""
import numpy as np
import torch


def rope_angles(max_pos, base, F0=1.0):
    """(max_pos, 16) fp64: pos * F0 / base^(i/16), exact to fp64."""
    inv_freq = F0 / torch.tensor(float(base), dtype=torch.float64) ** (torch.arange(16, dtype=torch.float64) / 16.0)
    return torch.arange(max_pos, dtype=torch.float64)[:, None] * inv_freq[None, :]


def rope_table_emulated(max_pos, base, F0=1.0):
    """numpy restatement of rope_table_kernel's own formula (csrc/elementwise.hip): inv_freq = fp32(F0 / pow(base, i / 16)) formed in fp64, the angle the
    fp32 product with pos, cos / sin in fp64 rounded to fp32. Returns (max_pos, 16, 2) fp32."""
    inv_freq = (np.float64(np.float32(F0)) / np.power(np.float64(np.float32(base)), np.arange(16, dtype=np.float64) / 16.0)).astype(np.float32)
    ang = (np.arange(max_pos, dtype=np.float32)[:, None] * inv_freq[None, :]).astype(np.float32).astype(np.float64)
    return np.stack((np.cos(ang).astype(np.float32), np.sin(ang).astype(np.float32)), axis=-1)


def rope_table_bound(max_pos, base, F0=1.0):
    """(max_pos, 16) fp64: |table - exact| <= pos inv_freq 2^-23 + 2^-24 -- the angle carries the fp32 rounding of inv_freq and of the product (2^-24 relative
    each, |d cos| <= |d angle|), the entry its own rounding to fp32 (half an ulp of a value <= 1)."""
    return rope_angles(max_pos, base, F0) * 2.0 ** -23 + 2.0 ** -24


def layernorm_stats(x, eps):
    """fp64 (mean, rstd) per row, the biased variance with eps inside the root (nn.LayerNorm)."""
    x = x.double()
    mean = x.mean(-1)
    var = ((x - mean[:, None]) ** 2).mean(-1)
    return mean, 1.0 / torch.sqrt(var + eps)


def rope_rotate(yr, tok_w, cos, sin):
    """yr (B, ntok, H, 64) fp64 -> rotated copy: columns 0-31 with ty = t // tok_w, 32-63 with tx = t % tok_w; pairs (c, c + 16); cos, sin (max_pos, 16)."""
    ntok = yr.shape[1]
    t = torch.arange(ntok, device=yr.device)
    out = yr.clone()
    for half, pos in enumerate((t // tok_w, t % tok_w)):
        c, s = cos[pos][None, :, None, :], sin[pos][None, :, None, :]      # (1, ntok, 1, 16)
        u, v = yr[..., half * 32: half * 32 + 16], yr[..., half * 32 + 16: half * 32 + 32]
        out[..., half * 32: half * 32 + 16] = u * c - v * s
        out[..., half * 32 + 16: half * 32 + 32] = v * c + u * s
    return out


def scatter_heads(y, kinds, head_c, ntok, tok_w, cos, sin):
    """y (M, N) fp64, N = len(kinds) * head_c -> per region the fp64 tensor the launch stores: 'rope' / 'plain' (B, H, ntok, 64), 'vt' (B, H, 64, ntok)
    (the columns [ntok, ldv) of a V^T destination are padding the launch never writes: not part of the reference)."""
    M = y.shape[0]
    B, H = M // ntok, head_c // 64
    out = []
    for r, kind in enumerate(kinds):
        yr = y[:, r * head_c: (r + 1) * head_c].reshape(B, ntok, H, 64)
        if kind == 'rope':
            yr = rope_rotate(yr, tok_w, cos, sin)
        yr = yr.permute(0, 2, 1, 3)                            # (B, H, ntok, 64)
        out.append(yr.transpose(-1, -2).contiguous() if kind == 'vt' else yr.contiguous())
    return out


def heads_ref(x, W, b, kinds, head_c, ntok, tok_w, base=100.0, F0=1.0, ln=None, cos_sin=None, y=None):
    """x (M, K), W (N, K), b (N,) or None -> list of fp64 regions (scatter_heads). ln = (gamma, beta, eps): the rows go through LayerNorm first.
    cos_sin: (cos, sin) tables (max_pos, 16) other than those of the exact angles; y: the (M, N) product formed elsewhere (the fp8 modes' emulation)."""
    if y is None:
        xd = x.double()
        if ln is not None:
            gamma, beta, eps = ln
            mean, rstd = layernorm_stats(xd, eps)
            xd = (xd - mean[:, None]) * rstd[:, None] * gamma.double() + beta.double()
        y = xd @ W.double().T
        if b is not None:
            y = y + b.double()
    if cos_sin is None:
        angles = rope_angles(max(ntok // tok_w, tok_w), base, F0)
        cos_sin = (angles.cos(), angles.sin())
    return scatter_heads(y.double(), kinds, head_c, ntok, tok_w, cos_sin[0].double().to(y.device), cos_sin[1].double().to(y.device))


def fold_inputs(B, th, tw, K, head_c, n_regions=3, seed=0, const_rows=0):
    """The inputs of the folded-LayerNorm cases: rows x = randn + 0.5 randn_row (so that |mean| <= 2 std holds with a wide margin: the ratio is ~0.5 |N(0,1)|),
    the last `const_rows` rows constant (std = 0); gamma = 1 +- 0.1, beta = +-0.1; W (N, K) with one scale per region; a bias that differs per column."""
    g = torch.Generator(device='cpu').manual_seed(seed)
    M, N = B * th * tw, n_regions * head_c
    x = torch.randn((M, K), generator=g) + 0.5 * torch.randn((M, 1), generator=g)
    if const_rows:
        x[M - const_rows:] = (0.25 * torch.arange(1, const_rows + 1, dtype=torch.float32))[:, None]
    gamma = 1 + 0.1 * torch.randn(K, generator=g)
    beta = 0.1 * torch.randn(K, generator=g)
    W = torch.randn((N, K), generator=g) / K ** 0.5
    W = W * torch.tensor([1.0, 0.5, 2.0])[:n_regions].repeat_interleave(head_c)[:, None]
    b = torch.randn(N, generator=g)
    return x, gamma, beta, W, b
