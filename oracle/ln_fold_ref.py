"""oracle/ln_fold_ref.py -- TEST INFRASTRUCTURE ONLY.

The folded-LayerNorm chain of the default engine (csrc/kernels.hpp GemmParams::ln_*) in plain fp64, launch by launch, with the inputs of
its kernel tests and the per-element error bounds those tests assert. tests/test_ln_fold_cpu.py pins the references and the conditions on the inputs
without a device; tests/test_ln_fold_gpu.py holds the kernels to them. Everything here is numpy / torch on whatever device its arguments live on.
"""
import numpy as np
import torch

from oracle.heads_ref import layernorm_stats

U = 2.0 ** -24                                  # unit roundoff of fp32
FINALIZE_C = [32, 128, 768, 1024, 1056, 2048]   # G = C / 32 = 1, 4, 24, 32, 33, 64: lanes g < G only; the g + 32 pair on one lane; on every lane
FINALIZE_ROWS = [1, 7, 8, 9, 1001]              # eight rows per block: a partial last block, the clamped row of its idle lanes
CONST_VALUES = [0.2, 0.1, 0.3, 2.3, 11.7, 29.0]  # constant rows whose fp32 (sum, sum of squares) leave q / C - mean^2 a few ulp either side of zero
FOLD_PACK_SHAPES = [(6, 32), (130, 96), (192, 256), (768, 1024), (256, 2048)]
CONSUMER_SHAPES = [(300, 192, 256), (77, 96, 768), (515, 328, 64), (1000, 384, 1024), (130, 256, 2048)]
CHAIN_C = [256, 1056, 2048]
# statistics of the producer against the two-pass statistics of the rows it STORED (chain_stat_bounds): roundings counted in units of U
K_MEAN, K_SQ = 10, 15
K_VAR = K_SQ + 2 * K_MEAN                      # = 35: the k of `relative error of rstd <= k / 2 U (1 + mean^2 / var)`


def inv_c32(C):
    """1 / C as the launches receive it: the fp32 quotient (GemmParams::ln_inv_c, launch_ln_finalize) -- inexact unless C is a power of two"""
    return float(np.float32(1.0) / np.float32(C))


def ulp32(v):
    """fp64 tensor: the spacing of fp32 at |v| (the smallest subnormal at 0)"""
    return torch.from_numpy(np.spacing(np.abs(v.detach().cpu().numpy().astype(np.float32))).astype(np.float64)).to(v.device)


def partials(x):
    """x (rows, C) fp32 -> (rows, C / 32, 2) fp32 (sum, sum of squares) of every 32-column group, summed in fp32 like the producer does (the ORDER is torch's,
    not the producer's: ln_finalize is held to the fp64 evaluation of whatever fp32 pairs it is given)."""
    rows, C = x.shape
    g = x.float().view(rows, C // 32, 32)
    return torch.stack((g.sum(-1), (g * g).sum(-1)), dim=-1).contiguous()


def producer_partials_emulated(v):
    """numpy restatement of the producer's fixed tree (csrc/kernels.hpp ln_quad_sums + the three lane exchanges of the typed-stream epilogue) on the fp32 values v
    (rows, C) BEFORE their rounding to split-fp16: per 32 columns, 8 quads of (x + y) + (z + w) / (xx + yy) + (zz + ww) with rounded products, then pairwise sums over
    the 8 quads (xor 1, 2, 4: adjacent pairing; fp addition commutes). Returns (rows, C / 32, 2) fp32."""
    v = np.asarray(v, dtype=np.float32)
    rows, C = v.shape
    q = v.reshape(rows, C // 32, 8, 4)
    sq = q * q
    sm = (q[..., 0] + q[..., 1]) + (q[..., 2] + q[..., 3])
    ss = (sq[..., 0] + sq[..., 1]) + (sq[..., 2] + sq[..., 3])
    for _ in range(3):
        sm, ss = sm[..., 0::2] + sm[..., 1::2], ss[..., 0::2] + ss[..., 1::2]
    return torch.from_numpy(np.stack((sm[..., 0], ss[..., 0]), axis=-1).astype(np.float32))


def finalize_ref(part, C, eps):
    """fp64 (rstd, nmr, var before the clamp) of d3r_ln_finalize's OWN inputs: the fp32 pairs summed in fp64, the factor 1 / C and eps as the fp32 values the kernel
    receives, var = q / C - mean^2 clamped at 0; nmr = -mean rstd. (With the exact 1 / C instead, var moves by (1 - mean^2 / var) 2^-24 relative where C is no power of
    two: thousands of ulp of rstd at |mean| = 100 std. Both routes read the same fp32 factor; chain_stat_bounds counts it against the two-pass statistics.)"""
    s, q = part[..., 0].double().sum(-1), part[..., 1].double().sum(-1)
    mean = s * inv_c32(C)
    var = q * inv_c32(C) - mean * mean
    rstd = 1.0 / torch.sqrt(var.clamp_min(0.0) + float(np.float32(eps)))
    return rstd, -mean * rstd, var


def finalize_rows(rows, C, seed):
    """`rows` random rows of the consumer tests' kind (randn + 0.5 randn per row), fp32"""
    g = torch.Generator(device='cpu').manual_seed(seed)
    return torch.randn((rows, C), generator=g) + 0.5 * torch.randn((rows, 1), generator=g)


def finalize_edge_rows(C, seed):
    """The edge rows of the ln_finalize test, fp32 (rows, C), and the slices of the three kinds:
      quarter   constant rows 0.25 k (partials exact in fp32: var is exactly 0, rstd = 1 / sqrt(eps))
      const     constant rows of CONST_VALUES (partials inexact: q / C - mean^2 lands a few ulp of mean^2 either side of zero -- the clamp)
      offset    rows with |mean| = 100 std (randn + 100, randn - 100, 0.01 randn + 1)"""
    g = torch.Generator(device='cpu').manual_seed(seed)
    quarter = (0.25 * torch.arange(1, 5, dtype=torch.float32))[:, None].expand(4, C)
    const = torch.tensor(CONST_VALUES, dtype=torch.float32)[:, None].expand(len(CONST_VALUES), C)
    r = torch.randn((3, C), generator=g).double()
    r = (r - r.mean(-1, keepdim=True)) / r.std(dim=-1, unbiased=False, keepdim=True)      # mean 0, std 1 exactly (before the roundings to fp32 / split-fp16)
    offset = torch.stack((r[0] + 100.0, r[1] - 100.0, 0.01 * r[2] + 1.0)).float()
    x = torch.cat((quarter, const, offset)).contiguous()
    return x, dict(quarter=slice(0, 4), const=slice(4, 4 + len(CONST_VALUES)), offset=slice(4 + len(CONST_VALUES), x.shape[0]))


def fold_pack_inputs(N, K, seed):
    """W (N, K), gamma = 1 +- 0.1, beta = +-0.1, bias (N,), fp32"""
    g = torch.Generator(device='cpu').manual_seed(seed)
    W = torch.randn((N, K), generator=g) / K ** 0.5
    return W, 1 + 0.1 * torch.randn(K, generator=g), 0.1 * torch.randn(K, generator=g), torch.randn(N, generator=g)


def fold_pack_ref(W, gamma, beta, bias, decoded_rows):
    """fp64 (colsum, bias_fold, slack of bias_fold) of the fold of one matrix: colsum of the DECODED packed rows (the operand the consumer GEMM reads -- the fold
    identity rstd (x wg^T - mean colsum) holds for exactly that operand, not for W gamma before its rounding), bias_fold = b + W beta, and the fp64 summation
    slack K 2^-53 sum_k |beta_k W_nk| the bias check allows on top of its ulp."""
    colsum = decoded_rows.double().sum(-1)
    bw = W.double() * beta.double()[None, :]
    bf = bw.sum(-1) + (bias.double() if bias is not None else 0.0)
    return colsum, bf, W.shape[1] * 2.0 ** -53 * bw.abs().sum(-1)


def consumer_c(K):
    """c of the plain consumer's bound c 2^-21 A (consumer_ref)"""
    return 2 + 6 * K / 256


def consumer_ref(x, wg, colsum, bf, mean, rstd):
    """fp64 (y, A, S, T) of one plain consumer launch on the operands the kernel reads (x, wg already rounded to split-fp16; colsum, bf, mean, rstd fp64):
      y = rstd_m (sum_k x_mk wg_nk - mean_m colsum_n) + bf_n        S = rstd_m sum_k |x_mk wg_nk|        T = |colsum_n mean_m rstd_m|        A = S + T + |bf_n|
    The `store` output is within consumer_c(K) 2^-21 A of y; with u = 2^-24, 2^-21 = 8 u (the derivation of test_heads_folded_layernorm_consumer without its rotation
    and table terms):
      lo.lo products the three-MFMA scheme drops, |x_lo w_lo| <= 2^-22 |x w|                                                       0.5 x 2^-21 S
      fp32 accumulation, 3 K / 32 MFMAs each allowed two roundings of a partial sum <= sum |x w|: 6 K / 32 u                       6 K / 256 x 2^-21 S
      fma(colsum, nmr, b') on operands rounded to fp32 (u T, u T, u |b'|) + its rounding (u (T + |b'|)); fma(acc, rstd, .): u S + u A  0.625 x 2^-21 A
      the split-fp16 store, 2^-22 relative                                                                                          0.5 x 2^-21 A
    so c = 0.5 + 6 K / 256 + 0.625 + 0.5 <= 2 + 6 K / 256."""
    xd, wd = x.double(), wg.double()
    y = rstd[:, None] * (xd @ wd.T - mean[:, None] * colsum[None, :]) + bf[None, :]
    S = rstd[:, None] * (xd.abs() @ wd.abs().T)
    T = (colsum[None, :] * (mean * rstd)[:, None]).abs()
    return y, S + T + bf.abs()[None, :], S, T


def gelu64(y):
    return torch.nn.functional.gelu(y.double())


def gelu_torch_error(y):
    """The one figure of the GELU bound that cannot be derived, measured on torch and NOT on the kernel: max |F.gelu(fp32) - F.gelu(fp64)| over the fp32-rounded
    pre-activations y (the error of an fp32 erf evaluation and the products around it). The kernel is allowed 4 x this: another approximation of the same class."""
    y32 = y.float()
    return float((torch.nn.functional.gelu(y32).double() - gelu64(y32)).abs().max())


GELU_SLOPE = 1.13      # max |gelu'| = Phi(x) + x phi(x) at x = sqrt(2): 1.1290 -- how far an error of the pre-activation can grow


def chain_inputs(M, Kp, C, N2, ratio, seed):
    """One producer -> finalize -> consumer chain: the producer nn.Linear (act (M, Kp), Wp (C, Kp), bp, residual (M, C)) stores rows of hidden width C with
    |mean| / std ~ ratio (ratio 0: the consumer tests' kind, ~0.5 |N(0, 1)|); the consumer is LayerNorm(gamma, beta) + nn.Linear(W2 (N2, C), b2)."""
    g = torch.Generator(device='cpu').manual_seed(seed)
    act = torch.randn((M, Kp), generator=g)
    Wp = 0.2 * torch.randn((C, Kp), generator=g) / Kp ** 0.5
    bp = 0.05 * torch.randn(C, generator=g)
    sign = torch.where(torch.rand((M, 1), generator=g) < 0.5, -1.0, 1.0)
    res = torch.randn((M, C), generator=g) + (0.5 * torch.randn((M, 1), generator=g) if ratio == 0 else sign * float(ratio))
    W2, gamma, beta, b2 = fold_pack_inputs(N2, C, seed + 1)
    return act, Wp, bp, res, W2, gamma, beta, b2


def chain_stat_bounds(xs):
    """xs (M, C) fp64, the rows the producer STORED. The producer sums the fp32 values v BEFORE their rounding to split-fp16 (xs = v (1 + e), |e| <= 2^-22 = 4 U),
    in one fixed tree: a sum passes 5 additions (two inside a lane's quad, three lane exchanges), a sum of squares one product and the same 5 additions; ln_finalize
    adds the pairs in fp64 (nothing against U) and multiplies by the fp32 quotient 1 / C (one more U, inv_c32). With every term of a sum of squares positive:
        |mean^ - mean| <= (5 + 4 + 1) U E|x|  = K_MEAN U E|x|            |q^ / C - E x^2| <= (6 + 2 x 4 + 1) U E x^2 = K_SQ U E x^2
        |var^ - var| <= K_SQ U E x^2 + 2 |mean| K_MEAN U E|x| + (K_MEAN U E|x|)^2 <= (K_SQ + 2 K_MEAN) U (var + mean^2) (1 + tiny)   as E|x|, |mean| <= sqrt(E x^2)
    so var^ = var (1 + e), |e| <= e_max = K_VAR U (1 + mean^2 / var) (1 + 1e-6), and the relative error of rstd is at most (1 - e_max)^-1/2 - 1 -- to first order
    K_VAR / 2 U (1 + mean^2 / var), k = 35 -- plus U for its own rounding to fp32. Returns (d_rstd relative, d_mean absolute), fp64 per row; d_rstd = inf where
    e_max >= 1 (the statistics carry no information there)."""
    mean = xs.mean(-1)
    var = ((xs - mean[:, None]) ** 2).mean(-1)
    e_max = K_VAR * U * (1 + mean * mean / var) * (1 + 1e-6)
    d_rstd = torch.where(e_max < 1, (1 - e_max.clamp_max(0.999)) ** -0.5 - 1, torch.full_like(e_max, float('inf'))) + U
    return d_rstd, K_MEAN * U * xs.abs().mean(-1)


def chain_ref(xs, wg, W2, gamma, beta, b2, eps):
    """fp64 reference and bound of the chain's consumer output on the rows the producer stored (xs, decoded) and the packed weights (wg, decoded):
    y = LN_two-pass(xs) W~^T + b', W~_nk = wg_nk / gamma_k, b' = b2 + W2 beta  =  rstd (xs wg^T - mean colsum) + b' with the TWO-PASS mean / rstd of xs.
    bound = consumer_c(C) 2^-21 A  +  d_rstd (S + T)  +  rstd |colsum| d_mean (1 + d_rstd)      (consumer_ref; chain_stat_bounds).
    Returns (y, bound, mean, rstd)."""
    mean, rstd = layernorm_stats(xs, eps)
    colsum, bf, _ = fold_pack_ref(W2, gamma, beta, b2, wg)
    y, A, S, T = consumer_ref(xs, wg, colsum, bf, mean, rstd)
    d_rstd, d_mean = chain_stat_bounds(xs.double())
    bound = consumer_c(xs.shape[1]) * 2.0 ** -21 * A + d_rstd[:, None] * (S + T) + (rstd * d_mean * (1 + d_rstd))[:, None] * colsum.abs()[None, :]
    return y, bound, mean, rstd
