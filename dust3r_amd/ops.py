"""Thin torch-tensor wrappers over the building-block entry points of libdust3r_hip.so
(d3r_rope2d / d3r_layernorm / d3r_linear / d3r_linear_heads / d3r_conv2d_nhwc / d3r_attention / d3r_upsample2x_nhwc).

`rope_2d` is the drop-in for the reference's only native op, croco's `curope.rope_2d(tokens,
positions, base, F0)` (in place; see include/dust3r_hip.h). The other wrappers exist so the parity
tests can pin each kernel against PyTorch; the model engine calls the kernels from C++ directly.
"""
import torch

from . import _lib
from ._lib import check, current_stream, lib, ptr


def _dt(t):
    return {torch.bfloat16: _lib.DTYPE_BF16, torch.float16: _lib.DTYPE_F16, torch.float32: _lib.DTYPE_F32}[t.dtype]


def rope_2d(tokens, positions, base, F0=1.0):
    """In-place 2-D RoPE on tokens (B, N, H, D) contiguous; positions (B, N, 2) int64 (y, x)."""
    _lib.require_device()
    assert tokens.is_cuda and tokens.is_contiguous() and tokens.ndim == 4, 'tokens must be a contiguous CUDA (B,N,H,D) tensor'
    B, N, H, D = tokens.shape
    assert D % 4 == 0, 'D must be a multiple of 4'
    assert positions.shape == (B, N, 2) and positions.dtype == torch.int64 and positions.is_contiguous()
    check(lib.d3r_rope2d(ptr(tokens), ptr(positions), B, N, H, D, float(base), float(F0), _dt(tokens), current_stream()), 'rope2d')
    return tokens


def layernorm(x, gamma, beta, eps=1e-6, dtype=torch.bfloat16):
    _lib.require_device()
    rows, Cc = x.shape
    out = torch.empty((rows, Cc), dtype=dtype, device=x.device)
    check(lib.d3r_layernorm(ptr(x), ptr(gamma), ptr(beta), ptr(out), rows, Cc, eps, _dt(out), current_stream()), 'layernorm')
    return out


def layernorm_x3(x, gamma, beta, eps=1e-6):
    """LayerNorm into split-fp16 rows (the default engine's operand layout), returned unpacked as fp32 = hi + lo."""
    _lib.require_device()
    rows, Cc = x.shape
    out = torch.empty((rows, 2 * Cc), dtype=torch.float16, device=x.device)
    check(lib.d3r_layernorm(ptr(x), ptr(gamma), ptr(beta), ptr(out), rows, Cc, eps, _lib.DTYPE_F16X3, current_stream()), 'layernorm(x3)')
    return unpack_x3(out)


def pad_rows(w, mult=256):
    n = w.shape[0]
    n_pad = (n + mult - 1) // mult * mult
    if n_pad == n:
        return w.contiguous()
    return torch.cat((w, w.new_zeros((n_pad - n,) + tuple(w.shape[1:]))), dim=0).contiguous()


def linear(act, weight, bias=None, epilogue='store', residual=None):
    """act (M,K), weight (N,K) in the same 16/32-bit dtype -> (M,N). epilogue: 'store' | 'f32' | 'gelu'."""
    _lib.require_device()
    M, K = act.shape
    N = weight.shape[0]
    wp = pad_rows(weight)
    bp = None if bias is None else pad_rows(bias.float())
    epi = {'store': 0, 'f32': 1, 'gelu': 2}[epilogue]
    out = torch.empty((M, N), dtype=torch.float32 if epi == 1 else act.dtype, device=act.device)
    check(lib.d3r_linear(ptr(act), ptr(wp), ptr(bp), ptr(out), ptr(residual), M, N, K, epi, _dt(act), current_stream()), 'linear')
    return out


def pack_x3(x):
    """fp32 (..., K) with K % 8 == 0 -> the engine's split-fp16 row layout, an fp16 tensor (..., 2K): per 8 logical elements
    a 32-byte group [hi x8][lo x8], hi = fp16(x), lo = fp16(x - hi) (csrc/common.hpp, Traits<D3R_F16X3>)."""
    x = x.float()
    hi = x.half()
    lo = (x - hi.float()).half()
    sh = x.shape
    g = torch.stack((hi.reshape(*sh[:-1], sh[-1] // 8, 8), lo.reshape(*sh[:-1], sh[-1] // 8, 8)), dim=-2)
    return g.reshape(*sh[:-1], sh[-1] * 2).contiguous()


def unpack_x3(t):
    """Inverse of pack_x3: fp16 (..., 2K) -> fp32 (..., K) = hi + lo."""
    sh = t.shape
    g = t.reshape(*sh[:-1], sh[-1] // 16, 2, 8).float()
    return (g[..., 0, :] + g[..., 1, :]).reshape(*sh[:-1], sh[-1] // 2)


def linear_x3res(act, weight, bias=None, residual=None, with_sums=True):
    """nn.Linear as the producer of a folded LayerNorm (d3r_linear_x3res, split-fp16): returns (rows fp32 = act . weight^T + bias + residual, rounded to
    split-fp16 like the engine's residual stream, and -- with_sums -- the (sum, sum of squares) pairs [M][N / 32][2] of the stored rows)."""
    _lib.require_device()
    M, K = act.shape
    N = weight.shape[0]
    ap, wp = pack_x3(act), pad_rows(pack_x3(weight))
    bp = None if bias is None else pad_rows(bias.float())
    rp = None if residual is None else pack_x3(residual)
    out = torch.empty((M, 2 * N), dtype=torch.float16, device=act.device)
    part = torch.zeros((M, N // 32, 2), dtype=torch.float32, device=act.device) if with_sums else None
    check(lib.d3r_linear_x3res(ptr(ap), ptr(wp), ptr(bp), ptr(out), ptr(rp), ptr(part), M, N, K, current_stream()), 'linear_x3res')
    return unpack_x3(out), part, out


def linear_x3(act, weight, bias=None, epilogue='store', residual=None):
    """`linear` in the split-fp16 precision mode: act (M,K), weight (N,K) fp32 (N, K multiples of 8) are packed to the
    x3 layout, the result comes back as fp32 (unpacked for the 'store' / 'gelu' epilogues)."""
    _lib.require_device()
    M, K = act.shape
    N = weight.shape[0]
    ap, wp = pack_x3(act), pad_rows(pack_x3(weight))
    bp = None if bias is None else pad_rows(bias.float())
    epi = {'store': 0, 'f32': 1, 'gelu': 2}[epilogue]
    out = torch.empty((M, N), dtype=torch.float32, device=act.device) if epi == 1 else torch.empty((M, 2 * N), dtype=torch.float16, device=act.device)
    check(lib.d3r_linear(ptr(ap), ptr(wp), ptr(bp), ptr(out), ptr(residual), M, N, K, epi, _lib.DTYPE_F16X3, current_stream()), 'linear(x3)')
    return out if epi == 1 else unpack_x3(out)


def ln_finalize(part, C, eps=1e-6, rstd=None, nmr=None):
    """d3r_ln_finalize: part (rows, C // 32, 2) fp32, the (sum, sum of squares) pairs of linear_x3res -> (rstd, nmr) fp32. rstd / nmr: the CALLER's arrays of at
    least `rows` elements (what the launch leaves untouched stays visible); None: allocated here."""
    _lib.require_device()
    rows = part.shape[0]
    assert part.dtype == torch.float32 and part.shape == (rows, C // 32, 2)
    rstd = torch.empty(rows, dtype=torch.float32, device=part.device) if rstd is None else rstd
    nmr = torch.empty(rows, dtype=torch.float32, device=part.device) if nmr is None else nmr
    assert rstd.numel() >= rows and nmr.numel() >= rows and rstd.dtype == nmr.dtype == torch.float32
    check(lib.d3r_ln_finalize(ptr(part), rows, C, float(eps), ptr(rstd), ptr(nmr), current_stream()), 'ln_finalize')
    return rstd, nmr


def ln_fold_pack(W, gamma, beta, bias=None, dtype='fp16x3'):
    """d3r_ln_fold_pack, the load-time fold of nn.Linear(W (N, K), bias) behind LayerNorm(gamma, beta): returns (rows, colsum, bias_fold) as the consumer launches
    take them -- rows fp16 (round_up(N, 256), 2 K) zeroed HERE before the launch (rows >= N must come back zero), colsum / bias_fold fp32 of round_up(N, 256)
    elements pre-filled with zero (elements >= N likewise)."""
    _lib.require_device()
    N, K = W.shape
    n_rows = (N + 255) // 256 * 256
    rows = torch.zeros((n_rows, 2 * K), dtype=torch.float16, device=W.device)
    colsum = torch.zeros(n_rows, dtype=torch.float32, device=W.device)
    bias_fold = torch.zeros(n_rows, dtype=torch.float32, device=W.device)
    W, gamma, beta = W.float().contiguous(), gamma.float().contiguous(), beta.float().contiguous()
    bias = None if bias is None else bias.float().contiguous()
    check(lib.d3r_ln_fold_pack(ptr(W), ptr(gamma), ptr(beta), ptr(bias), ptr(rows), ptr(colsum), ptr(bias_fold), N, K, _lib.DTYPES[dtype], current_stream()),
          'ln_fold_pack')
    return rows, colsum, bias_fold


def linear_ln(act_rows, wgt_rows, bias_fold, N, epilogue, rstd, nmr, colsum, part_in=None, eps=1e-6, out=None):
    """d3r_linear_ln, the plain consumer of a folded LayerNorm: act_rows fp16 (M, 2 K) split-fp16 rows, wgt_rows / bias_fold / colsum as ln_fold_pack returns
    them (round_up(N, 256) rows), epilogue 'store' | 'gelu'. rstd / nmr fp32 (M,) are read, or -- part_in (M, K // 32, 2) given -- WRITTEN by the launch.
    out: the caller's fp16 destination of at least M * 2 N elements (nothing here fills it); None: allocated here. Returns the stored rows, fp16 (M, 2 N)."""
    _lib.require_device()
    M, K = act_rows.shape[0], act_rows.shape[1] // 2
    assert act_rows.dtype == wgt_rows.dtype == torch.float16 and wgt_rows.shape == ((N + 255) // 256 * 256, 2 * K)
    assert colsum.numel() >= wgt_rows.shape[0] and (bias_fold is None or bias_fold.numel() >= wgt_rows.shape[0])
    assert rstd.numel() >= M and nmr.numel() >= M and rstd.dtype == nmr.dtype == colsum.dtype == torch.float32
    assert part_in is None or (part_in.dtype == torch.float32 and part_in.shape == (M, K // 32, 2))
    out = torch.empty(M * 2 * N, dtype=torch.float16, device=act_rows.device) if out is None else out
    assert out.dtype == torch.float16 and out.numel() >= M * 2 * N
    check(lib.d3r_linear_ln(ptr(act_rows), ptr(wgt_rows), ptr(bias_fold), ptr(out), M, N, K, {'store': 0, 'gelu': 2}[epilogue], ptr(rstd), ptr(nmr), ptr(colsum),
                            ptr(part_in), float(eps), current_stream()), 'linear_ln')
    return out[:M * 2 * N].view(M, 2 * N)


def layernorm_x3rows(rows, gamma, beta, eps=1e-6, out=None):
    """d3r_layernorm_x3rows: LayerNorm from split-fp16 rows fp16 (M, 2 C) into split-fp16 rows (the enc_norm / dec_norm launch of a fold engine). out: the caller's
    fp16 destination of at least M * 2 C elements; None: allocated here. Returns the stored rows, fp16 (M, 2 C)."""
    _lib.require_device()
    M, C2 = rows.shape
    assert rows.dtype == torch.float16
    out = torch.empty(M * C2, dtype=torch.float16, device=rows.device) if out is None else out
    assert out.dtype == torch.float16 and out.numel() >= M * C2
    check(lib.d3r_layernorm_x3rows(ptr(rows), ptr(gamma), ptr(beta), ptr(out), M, C2 // 2, float(eps), current_stream()), 'layernorm_x3rows')
    return out[:M * C2].view(M, C2)


def upsample2x_x3(x, out_hw=None, rows=False):
    """`upsample2x_nhwc` on split-fp16 maps: x (B,H,W,C) fp32, C % 8 == 0, packed along the channel axis; fp32 result, or -- rows=True -- the split rows
    (B,Ho,Wo,2C) fp16 exactly as the kernel stored them (unpacking to fp32 and packing again may re-split a value into another (hi, lo) pair)."""
    _lib.require_device()
    B, H, W, Cc = x.shape
    Ho, Wo = out_hw if out_hw is not None else (2 * H, 2 * W)
    xp = pack_x3(x)
    out = torch.empty((B, Ho, Wo, 2 * Cc), dtype=torch.float16, device=x.device)
    check(lib.d3r_upsample2x_nhwc(ptr(xp), ptr(out), B, H, W, Cc, Ho, Wo, _lib.DTYPE_F16X3, current_stream()), 'upsample2x(x3)')
    return out if rows else unpack_x3(out)


def _e4m3(x):
    """Round to OCP e4m3 (the encoding v_cvt_pk_fp8_f32 produces on gfx950: nearest even, subnormals kept), saturating at +-448
    as the kernels clamp before converting. Returns the bytes (uint8)."""
    return x.float().clamp(-448.0, 448.0).to(torch.float8_e4m3fn).view(torch.uint8)


def pack_f8(x, weight=False):
    """fp32 (..., K), K % 64 == 0 -> the fp16 + fp8 row layout as uint8 (..., 4K): per 64 logical elements a 256-byte super-group
    [hi fp16 x64 | a8 e4m3 x64 | b8 e4m3 x64]; activations a8 = e4m3(hi), b8 = e4m3(lo 2^11); weights a8 = e4m3(lo 2^17),
    b8 = e4m3(hi 2^6)  (hi = fp16(x), lo = x - hi; csrc/common.hpp, Traits<D3R_F16F8>)."""
    x = x.float().clamp(-65504.0, 65504.0)
    sh = x.shape
    assert sh[-1] % 64 == 0
    hi = x.half()
    lo = x - hi.float()
    h8 = _e4m3(hi.float() * (64.0 if weight else 1.0))
    l8 = _e4m3(lo * (131072.0 if weight else 2048.0))
    a8, b8 = (l8, h8) if weight else (h8, l8)
    g = lambda t: t.reshape(*sh[:-1], sh[-1] // 64, -1)
    out = torch.cat((g(hi.view(torch.uint8)), g(a8), g(b8)), dim=-1)
    return out.reshape(*sh[:-1], sh[-1] * 4).contiguous()


def unpack_f8(t, weight=False, parts=False):
    """Inverse of pack_f8 (uint8 (..., 4K) -> fp32 (..., K)): the value an element stands for, hi + lo8 2^-11 (activations) or
    hi + lo8 2^-17 (weights). parts=True returns (hi fp32, a8 bytes, b8 bytes)."""
    sh = t.shape
    g = t.reshape(*sh[:-1], sh[-1] // 256, 256)
    hi = g[..., :128].contiguous().view(torch.float16).float().reshape(*sh[:-1], sh[-1] // 4)
    a8 = g[..., 128:192].reshape(*sh[:-1], sh[-1] // 4)
    b8 = g[..., 192:].reshape(*sh[:-1], sh[-1] // 4)
    if parts:
        return hi, a8, b8
    lo8 = (a8 if weight else b8).contiguous().view(torch.float8_e4m3fn).float()
    return hi + lo8 / (131072.0 if weight else 2048.0)


def linear_f8(act, weight, bias=None, epilogue='store', residual=None):
    """`linear` in the fp16 + fp8 mode: act (M,K), weight (N,K) fp32 (K % 64 == 0; N % 64 == 0 for 'store' / 'gelu') are packed to the
    activation / weight row layouts; 'f32' returns the fp32 result, the others the decoded activation rows."""
    _lib.require_device()
    M, K = act.shape
    N = weight.shape[0]
    ap, wp = pack_f8(act), pad_rows(pack_f8(weight, weight=True))
    bp = None if bias is None else pad_rows(bias.float())
    epi = {'store': 0, 'f32': 1, 'gelu': 2}[epilogue]
    out = torch.empty((M, N), dtype=torch.float32, device=act.device) if epi == 1 else torch.empty((M, 4 * N), dtype=torch.uint8, device=act.device)
    check(lib.d3r_linear(ptr(ap), ptr(wp), ptr(bp), ptr(out), ptr(residual), M, N, K, epi, _lib.DTYPE_F16F8, current_stream()), 'linear(f16f8)')
    return out if epi == 1 else unpack_f8(out)


def pack_w5(w):
    """fp32 weights (N, K), K % 128 == 0 -> the 2.5-unit weight rows as uint8 (N, 5K): per 128 logical k five 128-byte chunks
    [w_hi k 0..63 fp16 | w_lo k 0..63 fp16 | w_hi k 64..127 | w_lo k 64..127 | e4m3(w_hi 2^6) k 0..127]  (csrc/common.hpp, Traits<D3R_F16X2F8>)."""
    w = w.float().clamp(-65504.0, 65504.0)
    N, K = w.shape
    assert K % 128 == 0
    hi = w.half()
    lo = (w - hi.float()).half()
    h8 = _e4m3(hi.float() * 64.0)
    hb, lb = hi.view(torch.uint8).reshape(N, K // 128, 2, 128), lo.view(torch.uint8).reshape(N, K // 128, 2, 128)
    out = torch.cat((hb[:, :, 0], lb[:, :, 0], hb[:, :, 1], lb[:, :, 1], h8.reshape(N, K // 128, 128)), dim=-1)
    return out.reshape(N, 5 * K).contiguous()


def linear_x2f8(act, weight, bias=None, epilogue='store', residual=None):
    """`linear` in the 2.5-unit mode (D3R_DTYPE_F16X2F8): fp16 + fp8 activation rows x five-chunk weight rows; K % 128 == 0."""
    _lib.require_device()
    M, K = act.shape
    N = weight.shape[0]
    ap, wp = pack_f8(act), pad_rows(pack_w5(weight))
    bp = None if bias is None else pad_rows(bias.float())
    epi = {'store': 0, 'f32': 1, 'gelu': 2}[epilogue]
    out = torch.empty((M, N), dtype=torch.float32, device=act.device) if epi == 1 else torch.empty((M, 4 * N), dtype=torch.uint8, device=act.device)
    check(lib.d3r_linear(ptr(ap), ptr(wp), ptr(bp), ptr(out), ptr(residual), M, N, K, epi, _lib.DTYPE_F16X2F8, current_stream()), 'linear(f16x2f8)')
    return out if epi == 1 else unpack_f8(out)


_HEAD_KINDS = {'rope': _lib.HEAD_ROPE, 'vt': _lib.HEAD_VT, 'plain': _lib.HEAD_PLAIN}
# destination element type of an attention-projection launch per precision mode (the fp8 modes hand split-fp16 rows to the attention kernel),
# and the storage elements per logical element
_HEAD_STORE = {'fp32': (torch.float32, 1), 'bf16': (torch.bfloat16, 1), 'fp16': (torch.float16, 1), 'fp16x3': (torch.float16, 2), 'fp16f8': (torch.float16, 2),
               'fp16x2f8': (torch.float16, 2)}


def rope_table(max_pos, base, F0=1.0, device='cuda'):
    """d3r_rope_table: (max_pos, 16, 2) fp32 (cos, sin) pairs of pos * F0 / base^(i/16)."""
    _lib.require_device()
    t = torch.empty((max_pos, 16, 2), dtype=torch.float32, device=device)
    check(lib.d3r_rope_table(ptr(t), max_pos, float(base), float(F0), current_stream()), 'rope_table')
    return t


def heads_dst_numel(kind, B, H, ntok, ldv, dtype):
    """storage elements of one destination of linear_heads (q / k: B H ntok 64, V^T: B H 64 ldv logical elements)"""
    return B * H * 64 * (ldv if kind == 'vt' else ntok) * _HEAD_STORE[dtype][1]


def heads_tile_config(M, K, kinds, head_c, ntok, tok_w, ldv, dtype, max_pos=512):
    """d3r_linear_heads_tile_config (host only): the tile configuration that launch runs on, environment pins applied."""
    import ctypes as C
    kk = (C.c_int * 3)(*([_HEAD_KINDS[k] for k in kinds] + [0] * (3 - len(kinds))))
    return lib.d3r_linear_heads_tile_config(M, K, len(kinds), head_c, kk, head_c // 64, ntok, tok_w, ldv, max_pos, _lib.DTYPES[dtype])


def linear_heads(act, weight, bias, kinds, head_c, ntok, tok_w, ldv, table, dtype='fp16x3', dsts=None, ln=None, splitk=None):
    """One attention-projection launch (d3r_linear_heads): act (M, K), weight (N, K) fp32, N = len(kinds) * head_c, kinds of 'rope' | 'vt' | 'plain';
    the operands are packed for `dtype` (a key of _lib.DTYPES). dsts: one flat tensor per region in the mode's destination type, at least
    heads_dst_numel elements, filled by the CALLER (nothing here zeroes them: what the launch leaves untouched stays visible); None: allocated here,
    filled with 1.0. ln: dict(rstd, nmr, colsum[, part_in, eps]) of fp32 tensors -- the folded-LayerNorm consumer; splitk: (slab fp32, counters int32).
    Returns the regions as fp32: q / k (B, H, ntok, 64), V^T (B, H, 64, ldv)."""
    import ctypes as C
    _lib.require_device()
    M, K = act.shape
    N = weight.shape[0]
    B, H = M // ntok, head_c // 64
    if dtype == 'fp16x3':
        ap, wp = pack_x3(act), pad_rows(pack_x3(weight))
    elif dtype == 'fp16f8':
        ap, wp = pack_f8(act), pad_rows(pack_f8(weight, weight=True))
    elif dtype == 'fp16x2f8':
        ap, wp = pack_f8(act), pad_rows(pack_w5(weight))
    else:
        tdt = _lib.TORCH_DTYPE[_lib.DTYPES[dtype]]
        ap, wp = act.to(tdt).contiguous(), pad_rows(weight.to(tdt))
    bp = None if bias is None else pad_rows(bias.float())
    sdt, per = _HEAD_STORE[dtype]
    if dsts is None:
        dsts = [torch.ones(heads_dst_numel(k, B, H, ntok, ldv, dtype), dtype=sdt, device=act.device) for k in kinds]
    for d, k in zip(dsts, kinds):
        assert d.dtype == sdt and d.is_contiguous() and d.numel() >= heads_dst_numel(k, B, H, ntok, ldv, dtype)
    kk = (C.c_int * 3)(*([_HEAD_KINDS[k] for k in kinds] + [0] * (3 - len(kinds))))
    dd = (C.c_void_p * 3)(*([d.data_ptr() for d in dsts] + [None] * (3 - len(kinds))))
    ln = ln or {}
    colsum = None if ln.get('colsum') is None else pad_rows(ln['colsum'].float())
    slab, cnt = splitk if splitk is not None else (None, None)
    check(lib.d3r_linear_heads(ptr(ap), ptr(wp), ptr(bp), M, K, len(kinds), head_c, kk, dd, H, ntok, tok_w, ldv, ptr(table), table.shape[0],
                               ptr(ln.get('rstd')), ptr(ln.get('nmr')), ptr(colsum), ptr(ln.get('part_in')), float(ln.get('eps', 1e-6)),
                               ptr(slab), 0 if slab is None else slab.numel(), ptr(cnt), 0 if cnt is None else cnt.numel(),
                               _lib.DTYPES[dtype], current_stream()), f'linear_heads({dtype})')
    out = []
    for d, k in zip(dsts, kinds):
        v = d[:heads_dst_numel(k, B, H, ntok, ldv, dtype)].view((B, H, 64, ldv * per) if k == 'vt' else (B, H, ntok, 64 * per))
        out.append(unpack_x3(v) if per == 2 else v.float())
    return out


def layernorm_f8(x, gamma, beta, eps=1e-6):
    """LayerNorm into fp16 + fp8 activation rows (uint8 (rows, 4C))."""
    _lib.require_device()
    rows, Cc = x.shape
    out = torch.empty((rows, 4 * Cc), dtype=torch.uint8, device=x.device)
    check(lib.d3r_layernorm(ptr(x), ptr(gamma), ptr(beta), ptr(out), rows, Cc, eps, _lib.DTYPE_F16F8, current_stream()), 'layernorm(f16f8)')
    return out


def pack_conv_weight(w, dtype=None):
    """torch (Cout, Cin, kh, kw) -> (round_up(Cout,256), kh*kw*Cin) in the K order d3r_conv2d_nhwc expects (include/dust3r_hip.h):
    channel slices of one K step (128 bytes) outermost, then the taps, then the channels of the slice."""
    Cout, Cin, kh, kw = w.shape
    S = 128 // torch.empty((), dtype=dtype or w.dtype).element_size()
    assert Cin % S == 0, f'{Cin=} must be a multiple of {S}'
    return pad_rows(w.reshape(Cout, Cin // S, S, kh * kw).permute(0, 1, 3, 2).reshape(Cout, -1))


_zero_pages = {}


def _zero_page(device):
    if device not in _zero_pages:
        _zero_pages[device] = torch.zeros(4096, dtype=torch.uint8, device=device)
    return _zero_pages[device]


def conv2d_nhwc(x, weight, bias=None, stride=1, pad=0, relu=False, res1=None, res2=None, relu_copy=False):
    """x (B,H,W,Cin) NHWC; weight torch layout (Cout,Cin,k,k); returns (B,Ho,Wo,Cout) [, relu copy]."""
    _lib.require_device()
    B, H, W, Cin = x.shape
    Cout, _, k, _ = weight.shape
    wp = pack_conv_weight(weight.to(x.dtype))
    bp = None if bias is None else pad_rows(bias.float())
    Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    out = torch.empty((B, Ho, Wo, Cout), dtype=x.dtype, device=x.device)
    out2 = torch.empty_like(out) if relu_copy else None
    check(lib.d3r_conv2d_nhwc(ptr(x), ptr(wp), ptr(bp), ptr(out), ptr(res1), ptr(res2), ptr(out2), B, H, W, Cin, Cout, k, stride,
                              pad, int(relu), ptr(_zero_page(x.device)), _dt(x), current_stream()), 'conv2d_nhwc')
    return (out, out2) if relu_copy else out


# ---- the DPT head's kernels alone (include/dust3r_hip.h: d3r_pack_conv_weight ... d3r_linear_head_post). Tensors go in and come out as fp32 LOGICAL values;
# `dtype` (a key of _lib.DTYPES: 'fp32' | 'bf16' | 'fp16' | 'fp16x3') is the layout the kernel works on. `out` / `pts` / `conf`: storage the CALLER filled
# (what a launch leaves untouched stays visible to it); None: allocated here, zeroed.
def to_rows(x, dtype='fp16x3'):
    """fp32 (..., C) -> the storage rows of `dtype` (split-fp16: pack_x3, an fp16 tensor (..., 2C))."""
    return pack_x3(x) if dtype == 'fp16x3' else x.to(_lib.TORCH_DTYPE[_lib.DTYPES[dtype]]).contiguous()


def from_rows(t, dtype='fp16x3'):
    return unpack_x3(t) if dtype == 'fp16x3' else t.float()


def _post_args(post):
    """(depth_mode, conf_mode, vmin, vmax) with the reference's names -> the arguments of d3r_model_set_postprocess"""
    depth, conf, vmin, vmax = post
    return ('exp', 'linear', 'square').index(depth), ('exp', 'sigmoid').index(conf), float(vmin), float(vmax)


def pack_conv_weight_device(w, cin_pad=None, dtype='fp16x3', transposed=False, cout_pad=None):
    """d3r_pack_conv_weight, the engine's loader: fp32 Conv2d weight (Cout, Cin, k, k) -> storage rows (round_up(Cout, 256), k*k*cin_pad), or --
    transposed -- ConvTranspose2d weight (Cin, Cout, k, k) -> (round_up(k*k*cout_pad, 256), cin_pad)."""
    _lib.require_device()
    w = w.float().contiguous()
    Cout, Cin = (w.shape[1], w.shape[0]) if transposed else (w.shape[0], w.shape[1])
    k = w.shape[2]
    cin_pad, cout_pad = cin_pad or Cin, cout_pad or Cout
    rows, cols = ((k * k * cout_pad + 255) // 256 * 256, cin_pad) if transposed else ((Cout + 255) // 256 * 256, k * k * cin_pad)
    dst = to_rows(torch.zeros((rows, cols), dtype=torch.float32, device=w.device), dtype)
    check(lib.d3r_pack_conv_weight(ptr(w), ptr(dst), int(transposed), Cout, Cin, k, cin_pad, cout_pad, _lib.DTYPES[dtype], current_stream()), 'pack_conv_weight')
    return dst


def pack_convt_bias_device(b, k, cout_pad=None):
    """d3r_pack_convt_bias: (Cout,) -> fp32 (round_up(k*k*cout_pad, 256),), element (ky*k + kx) * cout_pad + co = b[co]."""
    _lib.require_device()
    b = b.float().contiguous()
    cout_pad = cout_pad or b.numel()
    dst = torch.zeros((k * k * cout_pad + 255) // 256 * 256, dtype=torch.float32, device=b.device)
    check(lib.d3r_pack_convt_bias(ptr(b), ptr(dst), b.numel(), cout_pad, k, current_stream()), 'pack_convt_bias')
    return dst


def conv2d_nhwc_x(x, wp, bias, Cout, k, stride=1, pad=0, cin_pad=None, relu=False, nowide=False, res1=None, res2=None, relu_copy=False, n_store=None, ldo=None,
                  dtype='fp16x3', x_rows=False, out_rows=None):
    """d3r_conv2d_nhwc_x (the engine's conv()): x (B, H, W, cstride) of which the first cin_pad channels are read, wp from pack_conv_weight_device, bias (Cout,) or None;
    res1 / res2 (B, Ho, Wo, ldo). Returns (B, Ho, Wo, ldo) [, its ReLU copy]."""
    _lib.require_device()
    B, H, W, cstride = x.shape
    if x_rows:      # x: the split-fp16 storage rows of another kernel (upsample2x_x3(rows=True)), handed over untouched
        assert dtype == 'fp16x3' and x.dtype == torch.float16 and cstride % 2 == 0
        cstride //= 2
    cin_pad = cin_pad or cstride
    n_store = Cout if n_store is None else n_store
    ldo = n_store if ldo is None else ldo
    Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    xr = x.contiguous() if x_rows else to_rows(x, dtype)
    bp = None if bias is None else pad_rows(bias.float())
    out = out_rows if out_rows is not None else to_rows(torch.zeros((B, Ho, Wo, ldo), dtype=torch.float32, device=x.device), dtype)
    out2 = torch.zeros_like(out) if relu_copy else None
    r1, r2 = (None if r is None else to_rows(r, dtype) for r in (res1, res2))
    flags = (_lib.CONV_RELU if relu else 0) | (_lib.CONV_NOWIDE if nowide else 0)
    check(lib.d3r_conv2d_nhwc_x(ptr(xr), ptr(wp), ptr(bp), ptr(out), ptr(r1), ptr(r2), ptr(out2), B, H, W, cstride, cin_pad, Cout, n_store, ldo, k, stride, pad, flags,
                                ptr(_zero_page(x.device)), _lib.DTYPES[dtype], current_stream()), f'conv2d_nhwc_x({dtype})')
    if out_rows is not None:      # the caller's storage rows, as stored
        return out
    return (from_rows(out, dtype), from_rows(out2, dtype)) if relu_copy else from_rows(out, dtype)


def convt_gemm(x, wp, bp, k, cout_pad, cin_pad=None, ldo=None, dtype='fp16x3', out=None):
    """d3r_convt_gemm (ConvTranspose2d, kernel = stride = k): x (B, th, tw, lda), wp / bp from pack_conv_weight_device(transposed=True) / pack_convt_bias_device.
    Returns (B, k*th, k*tw, ldo)."""
    _lib.require_device()
    B, th, tw, lda = x.shape
    cin_pad = cin_pad or lda
    ldo = cout_pad if ldo is None else ldo
    xr = to_rows(x, dtype)
    if out is None:
        out = to_rows(torch.zeros((B, k * th, k * tw, ldo), dtype=torch.float32, device=x.device), dtype)
    check(lib.d3r_convt_gemm(ptr(xr), ptr(wp), ptr(bp), ptr(out), B, th, tw, lda, cin_pad, cout_pad, k, ldo, _lib.DTYPES[dtype], current_stream()), f'convt_gemm({dtype})')
    n = B * k * th * k * tw * ldo
    per = 2 if dtype == 'fp16x3' else 1
    return from_rows(out.view(-1)[:n * per].view(B, k * th, k * tw, ldo * per), dtype)


def _head_outputs(npix, strides, pts, conf, device):
    ps, cs = strides
    if pts is None:
        pts = torch.zeros(npix * ps, dtype=torch.float32, device=device)
    if conf is None:
        conf = torch.zeros(npix * cs, dtype=torch.float32, device=device)
    assert pts.dtype == conf.dtype == torch.float32 and pts.numel() >= (npix - 1) * ps + 3 and conf.numel() >= (npix - 1) * cs + 1
    return pts, conf


def _head_views(npix, strides, pts, conf):
    """(npix, 3) and (npix,) strided views of the two outputs"""
    ps, cs = strides
    return pts.as_strided((npix, 3), (ps, 1)), conf.as_strided((npix,), (cs,))


def conv_head4(x, wp, bias, w4, b4, Cout, post=('exp', 'exp', 1.0, float('inf')), strides=(3, 1), cin_pad=None, k=3, dtype='fp16x3', pts=None, conf=None, x_rows=False):
    """d3r_conv_head4 (the engine's conv_head4(): 3x3 conv + ReLU + 1x1 conv to 4 + postprocess in one launch): x (B, H, W, cstride), w4 (4, Cout), b4 (4,);
    x_rows=True: x is already the split-fp16 rows (B, H, W, 2 cstride) of another kernel (upsample2x_x3(rows=True)), handed over untouched.
    Returns (launched, pts (B*H*W, 3), conf (B*H*W,)); launched False = the entry point declined and wrote nothing."""
    _lib.require_device()
    B, H, W, cstride = x.shape
    if x_rows:
        assert dtype == 'fp16x3' and x.dtype == torch.float16 and cstride % 2 == 0
        cstride //= 2
    npix = B * H * W
    pts, conf = _head_outputs(npix, strides, pts, conf, x.device)
    xr = x.contiguous() if x_rows else to_rows(x, dtype)
    bp = None if bias is None else pad_rows(bias.float())
    w4, b4 = w4.float().contiguous(), b4.float().contiguous()
    rc = lib.d3r_conv_head4(ptr(xr), ptr(wp), ptr(bp), ptr(w4), ptr(b4), ptr(pts), ptr(conf), B, H, W, cstride,
                            cin_pad or cstride, Cout, k, strides[0], strides[1], *_post_args(post), ptr(_zero_page(x.device)), _lib.DTYPES[dtype], current_stream())
    if rc != _lib.DECLINED:
        check(rc, f'conv_head4({dtype})')
    return (rc == 0,) + _head_views(npix, strides, pts, conf)


def up2_conv_route(B, Hi, Wi, Cin, Cout, cstride=None, dtype='fp16x3', head4=True):
    """d3r_up2_conv_route (host only): True = up2_conv_head4 (head4=False: up2_conv2d_nhwc_x) interpolates the x2 map inside the convolution, False = it runs the two launches."""
    rc = lib.d3r_up2_conv_route(_lib.DTYPES[dtype], B, Hi, Wi, cstride or Cin, Cin, Cout, int(head4))
    if rc not in (0, 1):
        check(rc, f'up2_conv_route({dtype})')
    return rc == 1


def _up2_scratch(fused, B, Hi, Wi, cstride, dtype, device):
    """the map the two-launch route goes through; None where the one-launch route runs (the entry points accept NULL there)"""
    return None if fused else to_rows(torch.zeros((B, 2 * Hi, 2 * Wi, cstride), dtype=torch.float32, device=device), dtype)


def up2_conv_head4(x, wp, bias, w4, b4, Cout, post=('exp', 'exp', 1.0, float('inf')), strides=(3, 1), cin_pad=None, dtype='fp16x3', pts=None, conf=None):
    """d3r_up2_conv_head4: conv_head4 (3x3) on the x2 bilinear map of x (B, Hi, Wi, cstride), in one launch where up2_conv_route says so, else through a scratch map.
    Returns (launched, pts (B*2Hi*2Wi, 3), conf (B*2Hi*2Wi,))."""
    _lib.require_device()
    B, Hi, Wi, cstride = x.shape
    npix = B * 4 * Hi * Wi
    pts, conf = _head_outputs(npix, strides, pts, conf, x.device)
    xr = to_rows(x, dtype)
    scratch = _up2_scratch(up2_conv_route(B, Hi, Wi, cin_pad or cstride, Cout, cstride, dtype), B, Hi, Wi, cstride, dtype, x.device)
    bp = None if bias is None else pad_rows(bias.float())
    w4, b4 = w4.float().contiguous(), b4.float().contiguous()
    rc = lib.d3r_up2_conv_head4(ptr(xr), ptr(scratch), ptr(wp), ptr(bp), ptr(w4), ptr(b4), ptr(pts), ptr(conf), B, Hi, Wi, cstride, cin_pad or cstride, Cout,
                                strides[0], strides[1], *_post_args(post), ptr(_zero_page(x.device)), _lib.DTYPES[dtype], current_stream())
    if rc != _lib.DECLINED:
        check(rc, f'up2_conv_head4({dtype})')
    return (rc == 0,) + _head_views(npix, strides, pts, conf)


def up2_conv2d_nhwc_x(x, wp, bias, Cout, relu=False, cin_pad=None, dtype='fp16x3', out_rows=None, ldo=None):
    """d3r_up2_conv2d_nhwc_x: conv2d_nhwc_x (3x3, stride 1, pad 1) on the x2 bilinear map of x (B, Hi, Wi, cstride). out_rows: the storage rows (B, 2Hi, 2Wi, ldo) to
    write into (split-fp16: an fp16 tensor of 2 ldo per pixel), e.g. pre-filled with sentinels. Returns the storage rows."""
    _lib.require_device()
    B, Hi, Wi, cstride = x.shape
    ldo = Cout if ldo is None else ldo
    xr = to_rows(x, dtype)
    if out_rows is None:
        out_rows = to_rows(torch.zeros((B, 2 * Hi, 2 * Wi, ldo), dtype=torch.float32, device=x.device), dtype)
    scratch = _up2_scratch(up2_conv_route(B, Hi, Wi, cin_pad or cstride, Cout, cstride, dtype, head4=False) and ldo % 8 == 0, B, Hi, Wi, cstride, dtype, x.device)
    bp = None if bias is None else pad_rows(bias.float())
    check(lib.d3r_up2_conv2d_nhwc_x(ptr(xr), ptr(scratch), ptr(wp), ptr(bp), ptr(out_rows), B, Hi, Wi, cstride, cin_pad or cstride, Cout, ldo,
                                    _lib.CONV_RELU if relu else 0, ptr(_zero_page(x.device)), _lib.DTYPES[dtype], current_stream()), f'up2_conv2d_nhwc_x({dtype})')
    return out_rows


def head_final(feat, w4, b4, post=('exp', 'exp', 1.0, float('inf')), strides=(3, 1), dtype='fp16x3', pts=None, conf=None):
    """d3r_head_final: feat (npix, C) ReLU'd features, w4 (4, C), b4 (4,) -> pts (npix, 3), conf (npix,)."""
    _lib.require_device()
    npix, Cc = feat.shape
    pts, conf = _head_outputs(npix, strides, pts, conf, feat.device)
    fr = to_rows(feat, dtype)
    w4, b4 = w4.float().contiguous(), b4.float().contiguous()
    check(lib.d3r_head_final(ptr(fr), Cc, ptr(w4), ptr(b4), ptr(pts), ptr(conf), npix, strides[0], strides[1],
                             *_post_args(post), _lib.DTYPES[dtype], current_stream()), f'head_final({dtype})')
    return _head_views(npix, strides, pts, conf)


def linear_head_post(feat, B, th, tw, ps, post=('exp', 'exp', 1.0, float('inf')), strides=(3, 1), pts=None, conf=None):
    """d3r_linear_head_post: feat fp32 (B*th*tw, 4*ps*ps) -> pts (B*th*ps*tw*ps, 3), conf (B*th*ps*tw*ps,)."""
    _lib.require_device()
    npix = B * th * ps * tw * ps
    assert feat.shape == (B * th * tw, 4 * ps * ps) and feat.dtype == torch.float32
    pts, conf = _head_outputs(npix, strides, pts, conf, feat.device)
    check(lib.d3r_linear_head_post(ptr(feat), ptr(pts), ptr(conf), B, th, tw, ps, strides[0], strides[1], *_post_args(post), current_stream()), 'linear_head_post')
    return _head_views(npix, strides, pts, conf)


def attention(q, k, vt, Nk=None, scale=0.125):
    """q (B,H,Nq,64), k (B,H,Nk,64), vt (B,H,64,ldv) with ldv % 64 == 0 and zero padding -> (B,Nq,H*64)."""
    _lib.require_device()
    B, H, Nq, D = q.shape
    assert D == 64
    Nk = k.shape[2] if Nk is None else Nk
    ldv = vt.shape[3]
    out = torch.empty((B, Nq, H * 64), dtype=q.dtype, device=q.device)
    check(lib.d3r_attention(ptr(q), ptr(k), ptr(vt), ptr(out), B, H, Nq, Nk, ldv, scale, _dt(q), current_stream()), 'attention')
    return out


def attention_x3(q, k, v, scale=0.125, out_rows='fp16x3'):
    """`attention` in the split-fp16 precision mode: q (B,H,Nq,64), k, v (B,H,Nk,64) fp32 are packed to the x3 row layout (q, k per
    token; v transposed to (B,H,64,ldv) with the keys zero padded to a multiple of 64), the (B,Nq,H*64) result comes back as fp32.
    out_rows='fp16f8' (or 'fp16x2f8'): the kernel stores the fp16 + fp8 activation rows of those GEMM modes (d3r_attention_rows), decoded here."""
    _lib.require_device()
    B, H, Nq, D = q.shape
    Nk = k.shape[2]
    assert D == 64
    ldv = (Nk + 63) // 64 * 64
    vt = torch.zeros((B, H, 64, ldv), dtype=torch.float32, device=q.device)
    vt[..., :Nk] = v.float().transpose(-1, -2)
    qp, kp, vp = pack_x3(q), pack_x3(k), pack_x3(vt)
    if _lib.DTYPES[out_rows] == _lib.DTYPE_F16X3:
        out = torch.empty((B, Nq, H * 64 * 2), dtype=torch.float16, device=q.device)
        check(lib.d3r_attention(ptr(qp), ptr(kp), ptr(vp), ptr(out), B, H, Nq, Nk, ldv, scale, _lib.DTYPE_F16X3, current_stream()), 'attention(x3)')
        return unpack_x3(out)
    out = torch.empty((B, Nq, H * 64 * 4), dtype=torch.uint8, device=q.device)
    check(lib.d3r_attention_rows(ptr(qp), ptr(kp), ptr(vp), ptr(out), B, H, Nq, Nk, ldv, scale, _lib.DTYPE_F16X3, _lib.DTYPES[out_rows], current_stream()),
          f'attention(x3 -> {out_rows})')
    return unpack_f8(out)


def upsample2x_nhwc(x, out_hw=None):
    _lib.require_device()
    B, H, W, Cc = x.shape
    Ho, Wo = out_hw if out_hw is not None else (2 * H, 2 * W)
    out = torch.empty((B, Ho, Wo, Cc), dtype=x.dtype, device=x.device)
    check(lib.d3r_upsample2x_nhwc(ptr(x), ptr(out), B, H, W, Cc, Ho, Wo, _dt(x), current_stream()), 'upsample2x')
    return out
