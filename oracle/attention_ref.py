"""oracle/attention_ref.py -- TEST INFRASTRUCTURE ONLY.

softmax(Q K^T scale) V as csrc/attention.hip evaluates it, three ways, for tests/test_attention_cpu.py (no device) and tests/test_attention_gpu.py:

    attention_fp64            the exact result, in fp64, of the operands AS STORED (after their rounding to the arm's operand type)
    elementwise_bound         one DERIVED bound per output element on |kernel - attention_fp64| (derivation below; no constant comes from a GPU run)
    online_softmax_emulated   an fp32 emulation of the online-softmax algorithm both kernels implement, with deliberate defects (`variant`):
                              the CPU tests show that the emulation stays inside the bound and that every defect leaves it on a named case,
                              which is the evidence that the GPU comparison can fail.

and the seeded input builders of the cases. torch on the CPU; no product import.

ARMS (name -> operand type, output rows). The three split-fp16 arms differ in the kernel that runs (an environment switch of the tests), not in arithmetic:
one emulation class covers them.

THE BOUND, term by term. Everything is per query row; `nat` marks a quantity in units of the softmax argument (natural logarithm). u = 2^-24.
Perturbing the argument of key j by delta_j changes the probability row by at most  T = 2 sum_j p_j |delta_j| exp(3 max_j |delta_j|)  in the 1-norm
(p'_j = p_j e^{delta_j} / Z', |log Z'| <= sum p |delta| e^{max}, |e^x - 1| <= |x| e^{|x|}); for one uniform bound eps this is the familiar 2 eps. delta_j sums

  (a) score error (nat, uniform over the row): scale A (a_op + 65 u), A = max_j sum_d |q_d k_jd|. 64 products enter one fp32 accumulator, in any grouping
      at most 64 roundings, one more for the product with the constant; a_op = 0 for fp32 (the MFMA is a fused multiply-add), bf16 and fp16 (a product of
      two 8- or 11-bit significands is exact in fp32); split-fp16 drops lo * lo (2^-22 relative to |q k|) and the two lo halves are themselves rounded
      (2^-22 each): a_op = 3 * 2^-22. The term is ZERO where no rounding can occur: every product is a multiple of one power of two g, A / g <= 2^24 (so
      every partial sum, in any order, is an fp32 number) and -- split-fp16 -- the lo halves are zero (_scores_exact; the large-score case is built so).
  (b) the constant c = scale log2(e) is an fp32 product of an fp32 constant (2 roundings) and the exponent argument fma(s, c, -m c) is rounded once:
      3 u (m - s_j) scale -- relative to the GAP of key j, so it is weighted by p_j and vanishes for the keys that carry the mass.
  (c) exp2 in hardware: 1 ulp = 2 u relative, once for the key and once per rescale of a later tile: 2 u ntiles.
  (d) the running maximum. A key of tile t is exponentiated against fl(m_t c) and later multiplied by exp2(fl(fl(m_{u-1} - m_u) c)) for every later tile u.
      Against the final maximum m_T these roundings do not cancel: u scale (|m_T| + |m_t| + 2 (m_T - m_t)) nat. It grows with the SCORE MAGNITUDE, which
      is why one global tolerance cannot hold at sharp heads. It is zero for the keys whose tile already saw the final maximum (then every later
      m_{u-1} - m_u is 0 and both sides use the same fl(m_T c)); the bound uses that only where the scores are exact (a), so that the kernel's maxima
      are the reference's.
P and the accumulators:
  (e) P is rounded to the operand type before P V while the row sum uses the unrounded values: u_P sum_j p_j = u_P with u_P = u (fp32), 2^-8 (bf16),
      2^-11 (fp16), 2^-22 (split: hi, then lo = fp16(p - hi)); fp16 and the split also have fp16's subnormal spacing 2^-24 under 2^-14: an absolute
      min(2^-25, e_j) per key on e_j = exp(s_j - m) <= 1, divided by the row sum l >= 1 ("about 2^-21" for a row of a few mid-sized probabilities).
  (f) fp32 accumulation over the Nk keys: T_acc additions per key into an output accumulator (T_acc = 3 MFMA terms for the split, else 1) and one into the
      row sum. Adding x to a costs at most min(u |a + x|, |x|) (a itself is an fp32 number, so the nearest one to a + x is no farther than |x|): relative to
      the row sum, min(u, p_j) per addition, i.e. n_eff = sum_j min(1, p_j / u) <= Nk effective keys -- a key far below the maximum cannot cost more than
      it weighs. With one rescale multiplication per tile on each accumulator, the reciprocal and the final product:
      ((T_acc + 1) n_eff + 2 ntiles + 2) u, relative to sum_j p_j |v_jd| <= max_j |v_jd|.
  (g) the stored row: u_out |o|, u_out = u (fp32), 2^-8 (bf16), 2^-11 (fp16) + 2^-25 absolute (subnormal), 2^-22 + 2^-25 (split rows); the fp16 + fp8 rows
      hold hi = fp16(o) and e4m3(lo 2^11) (4 significant bits, subnormal spacing 2^-9, saturating at 448): 2^-15 |o| + 2^-21 while |o| < 448 (lo 2^11 <= 2^e
      for |o| in [2^e, 2^(e+1)) cannot saturate), else plain fp16, 2^-11 |o|.
Combination:  bound = SAFETY [ (T + u_P' + acc) max_j |v_jd|  +  out_err(|o| + the first part) ],  SAFETY = 2, stated here once: it covers what the model
leaves out (the order inside an MFMA, flushed subnormal exponentials, second-order products of the terms).
"""
import math

import numpy as np
import torch

U = 2.0 ** -24
SAFETY = 2.0
TILE = 64
MASKED = -1e30
LOG2E32 = np.float32(1.44269504088896340736)

ARMS = {'fp32': ('fp32', 'same'), 'bf16': ('bf16', 'same'), 'fp16': ('fp16', 'same'),
        'x3-v1': ('x3', 'same'), 'x3-reg': ('x3', 'same'), 'x3-dma': ('x3', 'same'),
        'x3-v1+f8': ('x3', 'f8'), 'x3-reg+f8': ('x3', 'f8'), 'x3-dma+f8': ('x3', 'f8')}
EMULATION_CLASSES = ['fp32', 'bf16', 'fp16', 'x3-dma', 'x3-dma+f8']      # one arm per distinct arithmetic
A_OP = {'fp32': 0.0, 'bf16': 0.0, 'fp16': 0.0, 'x3': 3 * 2.0 ** -22}
U_P = {'fp32': U, 'bf16': 2.0 ** -8, 'fp16': 2.0 ** -11, 'x3': 2.0 ** -22}
VARIANTS = ['mask_off_by_one', 'no_rescale_when_max_moves', 'unfused_exponent', 'halves_disagree_on_max', 'p_not_rounded']

# (B, H, Nq, Nk): every Nq of {1, 31, 32, 33, 127, 128, 129, 257} and every Nk of {1, 63, 64, 65, 127, 129, 191, 193, 321} at least twice (1 to 6 key tiles,
# odd and even counts: both tails of the pipelined loop); workgroups B H ceil(Nq / 128) = 1, 3, 5, 6, 9, 12, 17
SHAPES = [(1, 1, 1, 1), (1, 1, 31, 63), (1, 1, 32, 64), (1, 1, 33, 65), (2, 3, 127, 127), (1, 5, 128, 129), (3, 1, 129, 191), (1, 1, 257, 193), (3, 1, 257, 321),
          (1, 17, 1, 321), (1, 5, 31, 1), (3, 1, 32, 193), (2, 3, 33, 191), (1, 1, 127, 129), (1, 17, 128, 127), (2, 3, 129, 65), (1, 5, 33, 63), (3, 1, 31, 64)]
OUTLIER_SHAPES = [(1, 1, 33, 65), (2, 3, 127, 127), (1, 5, 128, 129), (3, 1, 257, 321)]
LARGE_SHAPES = [(1, 1, 33, 65), (2, 3, 129, 129), (1, 5, 31, 193)]
LARGE_PLACEMENTS = ['first', 'last', 'grow']
SCALE_SHAPES = [(2, 3, 33, 191), (1, 5, 129, 65)]
SCALES = [0.1, 1.0]
PAD_NK = [1, 65, 129, 193]
POSITION_BH = [(2, 3), (1, 17)]


def workgroups(B, H, Nq):
    return B * H * ((Nq + 127) // 128)


# ---------------------------------------------------------------------------------------------------------------- operands as stored
def split_x3(x):
    """fp32 -> (hi, lo) fp32 values of the split-fp16 pair: hi = fp16(x), lo = fp16(x - hi)"""
    x = x.float()
    hi = x.half().float()
    return hi, (x - hi).half().float()


def stored(x, operand):
    """the value (fp64) an fp32 input stands for once stored in the arm's operand type"""
    x = x.float()
    if operand == 'bf16':
        return x.bfloat16().double()
    if operand == 'fp16':
        return x.half().double()
    if operand == 'x3':
        hi, lo = split_x3(x)
        return hi.double() + lo.double()
    return x.double()


def scale32(scale):
    """the C ABI takes the scale as a float: that value is the operand"""
    return float(np.float32(scale))


def to_rows(o):
    """(B, H, Nq, 64) -> the output layout (B, Nq, H * 64)"""
    B, H, Nq, D = o.shape
    return o.permute(0, 2, 1, 3).reshape(B, Nq, H * D)


def attention_fp64(q, k, v, scale):
    """softmax(q k^T scale) v in fp64 of the operands as given (pass them through `stored`): q (B,H,Nq,64), k, v (B,H,Nk,64) -> (B, Nq, H*64)"""
    s = (q.double() @ k.double().transpose(-1, -2)) * scale32(scale)
    return to_rows(torch.softmax(s, dim=-1) @ v.double())


# ---------------------------------------------------------------------------------------------------------------- the bound
def _quantum(x):
    """the largest power of two 2^-e, 0 <= e <= 30, of which every entry of x is an integer multiple; None if there is none"""
    for e in range(31):
        y = x * 2.0 ** e
        if bool((y == y.round()).all()):
            return 2.0 ** -e
    return None


def _scores_exact(qs, ks, operand, A):
    """True where the kernel's fp32 scores carry no rounding at all (term (a) of the derivation)"""
    if operand == 'x3' and not (bool((qs == qs.float().half().double()).all()) and bool((ks == ks.float().half().double()).all())):
        return False
    gq, gk = _quantum(qs), _quantum(ks)
    return gq is not None and gk is not None and float(A.max()) / (gq * gk) <= 2.0 ** 24


def _out_err(a, operand, rows):
    """term (g): rounding of a stored output element of magnitude <= a"""
    if rows == 'f8':
        return torch.where(a < 448.0, a * 2.0 ** -15 + 2.0 ** -21, a * 2.0 ** -11)
    if operand == 'x3':
        return a * 2.0 ** -22 + 2.0 ** -25
    if operand == 'fp16':
        return a * 2.0 ** -11 + 2.0 ** -25
    return a * (2.0 ** -8 if operand == 'bf16' else U)


def elementwise_bound(q, k, v, scale, arm):
    """fp32 inputs (B,H,Nq,64), (B,H,Nk,64) x2 -> (B, Nq, H*64) fp64: the derived bound of the module docstring on |kernel - attention_fp64(stored operands)|"""
    operand, rows = ARMS[arm]
    qs, ks, vs = stored(q, operand), stored(k, operand), stored(v, operand)
    sc = scale32(scale)
    Nk = ks.shape[2]
    nt = (Nk + TILE - 1) // TILE
    s = (qs @ ks.transpose(-1, -2)) * sc                                       # nat
    m = s.max(dim=-1, keepdim=True).values
    e = torch.exp(s - m)
    l = e.sum(dim=-1, keepdim=True)
    p = e / l
    o = p @ vs
    A = (qs.abs() @ ks.abs().transpose(-1, -2)).max(dim=-1, keepdim=True).values
    exact = _scores_exact(qs, ks, operand, A)
    eps_s = 0.0 if exact else sc * A * (A_OP[operand] + 65 * U)              # (a)
    sp = torch.nn.functional.pad(s, (0, nt * TILE - Nk), value=float('-inf'))
    run = sp.reshape(*s.shape[:-1], nt, TILE).max(dim=-1).values.cummax(dim=-1).values      # running maximum after each tile
    m_t = run.repeat_interleave(TILE, dim=-1)[..., :Nk]
    d_max = U * (m.abs() + m_t.abs() + 2 * (m - m_t))                          # (d)
    if exact:
        d_max = d_max * (m_t != m)
    delta = eps_s + 3 * U * (m - s) + 2 * U * nt + d_max                       # (a) + (b) + (c) + (d)
    T = 2 * (p * delta).sum(dim=-1, keepdim=True) * math.exp(3 * float(delta.max()))
    u_p = torch.full_like(l, U_P[operand])                                      # (e)
    if operand in ('fp16', 'x3'):
        u_p = u_p + e.clamp(max=2.0 ** -25).sum(dim=-1, keepdim=True) / l
    n_eff = (p / U).clamp(max=1.0).sum(dim=-1, keepdim=True)
    acc = ((4 if operand == 'x3' else 2) * n_eff + 2 * nt + 2) * U             # (f)
    vmax = vs.abs().max(dim=2, keepdim=True).values                             # (B, H, 1, 64)
    first = (T + u_p + acc) * vmax
    return to_rows(SAFETY * (first + _out_err(o.abs() + first, operand, rows)))


# ---------------------------------------------------------------------------------------------------------------- the emulation
def _store_rows(o, operand, rows):
    """fp32 (..., 64) -> the value the stored output row decodes to (fp64)"""
    if rows == 'f8':
        o = o.clamp(-65504.0, 65504.0)
        hi = o.half().float()
        lo8 = ((o - hi) * 2048.0).clamp(-448.0, 448.0).to(torch.float8_e4m3fn).float()
        return hi.double() + lo8.double() / 2048.0
    return stored(o, operand)


def online_softmax_emulated(q, k, v, scale, arm, variant=None):
    """The algorithm of both kernels in fp32 on the CPU: 64-key tiles, running maximum from -1e30, p = exp2(fma(s, c, -fl(m c))), rescale by
    exp2((m_old - m_new) c), keys >= Nk masked to -1e30, P rounded to the operand type in front of P V, one division at the end, the output row rounded as
    stored. The ORDER of the fp32 sums is torch's, not the MFMAs'. variant: one of VARIANTS, a deliberate defect -- except 'p_not_rounded', which is harmless.
    Returns (B, Nq, H*64) fp64."""
    assert variant is None or variant in VARIANTS
    operand, rows = ARMS[arm]
    f32 = torch.float32
    c = float(np.float32(np.float32(scale) * LOG2E32))
    Nk = k.shape[2]
    nt = (Nk + TILE - 1) // TILE
    padk = nt * TILE - Nk
    T_ = lambda x: x.transpose(-1, -2)      # noqa: E731
    if operand == 'x3':
        (qh, ql), (kh, kl), (vh, vl) = split_x3(q), split_x3(k), split_x3(v)
        S = (ql @ T_(kh) + qh @ T_(kl)) + qh @ T_(kh)
        vh, vl = (torch.nn.functional.pad(x, (0, 0, 0, padk)) for x in (vh, vl))
    else:
        qs, ks, vs = (stored(x, operand).float() for x in (q, k, v))
        S = qs @ T_(ks)
        vs = torch.nn.functional.pad(vs, (0, 0, 0, padk))
    S = torch.nn.functional.pad(S, (0, padk))                                 # keys beyond Nk: whatever the tile holds, masked below
    lead = S.shape[:-1]
    m_run = torch.full(lead, MASKED, dtype=f32)
    l = torch.zeros(lead, dtype=f32)
    o = torch.zeros(*lead, 64, dtype=f32)
    limit = Nk - 1 if variant == 'mask_off_by_one' else Nk
    for t in range(nt):
        sl = slice(t * TILE, (t + 1) * TILE)
        key = torch.arange(t * TILE, (t + 1) * TILE)
        st = torch.where(key < limit, S[..., sl], torch.tensor(MASKED, dtype=f32))
        if variant == 'halves_disagree_on_max':
            ma = torch.maximum(m_run, st[..., :32].max(dim=-1).values)
            mb = torch.maximum(m_run, st[..., 32:].max(dim=-1).values)
            m_new = torch.maximum(ma, mb)
            m_key = torch.cat((ma[..., None].expand(*lead, 32), mb[..., None].expand(*lead, 32)), dim=-1)
        else:
            m_new = torch.maximum(m_run, st.max(dim=-1).values)
            m_key = m_new[..., None]
        alpha = torch.exp2(((m_run - m_new) * c).double()).float()
        if variant == 'no_rescale_when_max_moves':
            alpha = torch.ones_like(alpha)
        mc = m_key * c                                                         # fp32 product
        if variant == 'unfused_exponent':
            arg = st * c - mc                                                  # s c rounded before the subtraction
        else:
            arg = (st.double() * c - mc.double()).float()                      # fma: the fp32 x fp32 product is exact in fp64
        pr = torch.exp2(arg.double()).float()
        l = l * alpha + pr.sum(dim=-1)
        m_run = m_new
        if operand == 'x3':
            if variant == 'p_not_rounded':
                pv = pr @ (vh[..., sl, :] + vl[..., sl, :])
            else:
                ph, pl = split_x3(pr)
                pv = (ph @ vl[..., sl, :] + pl @ vh[..., sl, :]) + ph @ vh[..., sl, :]
        else:
            pp = pr if (variant == 'p_not_rounded' or operand == 'fp32') else stored(pr, operand).float()
            pv = pp @ vs[..., sl, :]
        o = o * alpha[..., None] + pv
    out = o * (1.0 / l)[..., None]
    return to_rows(_store_rows(out, operand, rows))


# ---------------------------------------------------------------------------------------------------------------- the cases
def _gen(*key):
    return torch.Generator().manual_seed(int(sum((i + 1) * 1000003 * int(x) for i, x in enumerate(key)) % (2 ** 31)))


def random_case(B, H, Nq, Nk, seed=0):
    """case 1: q, k ~ 1.5 N(0,1), v ~ N(0,1). Conditions: the scaled scores at scale 0.125 stay below 60 in magnitude (no sharp head here)."""
    g = _gen(1, B, H, Nq, Nk, seed)
    q = torch.randn((B, H, Nq, 64), generator=g) * 1.5
    k = torch.randn((B, H, Nk, 64), generator=g) * 1.5
    v = torch.randn((B, H, Nk, 64), generator=g)
    return q, k, v, {'score_absmax_at_0.125': float((q.double() @ k.double().transpose(-1, -2)).abs().max()) * 0.125}


def outlier_case(B, H, Nq, Nk, seed=0):
    """case 2: the random case with column d of v scaled by 2^e_d, e_d running from -10 to 10. Conditions: the exponents, and the ratio between the largest
    column maximum and the smallest (what a per-tensor error measure hides)."""
    q, k, v, _ = random_case(B, H, Nq, Nk, seed + 17)
    expo = torch.round(torch.linspace(-10, 10, 64))
    v = v * (2.0 ** expo)
    cm = v.abs().amax(dim=(0, 1, 2))
    return q, k, v, {'expo_min': float(expo.min()), 'expo_max': float(expo.max()), 'column_ratio': float(cm.max() / cm.min())}


LARGE_SCALE = 0.125
LARGE_CH = (5, 22, 41, 58)          # one channel per 16-wide k-step, both lane halves of the MFMA operand layout
LARGE_NEAR_SHARE, LARGE_OFFMAX_SHARE = 0.999, 0.25


def large_score_case(B, H, Nq, Nk, placement, seed=0):
    """case 3 (scale 0.125): small integers on four channels. Query i has a in 72..80 on channel c0 and 8 on c1; a NEAR key has 80 on c0 and an integer f in
    -4..0 on c1: scaled score 10 a + f, i.e. 720..800, gaps 0..4 below the row maximum. Every other key has 80 - r, r >= 5, on c0 (and small integers on c1..c3):
    at least 42 below. Near keys sit in every tile; `placement` says where the maximum is: 'first' (tile 0, with an exact tie in tile 1), 'last' (the last
    tile, 1 above the level of every earlier tile), 'grow' (the tile maximum rises by 1 from tile to tile). Conditions returned (asserted by the tests): every operand is a bf16 / fp16 number, the fp32
    scores equal the fp64 ones, the near keys hold at least LARGE_NEAR_SHARE of every row's mass in at least two tiles, those other than the maximum at least
    LARGE_OFFMAX_SHARE, and the tile of the first maximum."""
    assert placement in LARGE_PLACEMENTS and Nk > TILE
    g = _gen(3, B, H, Nq, Nk, seed, LARGE_PLACEMENTS.index(placement))
    ri = lambda lo, hi, shape: torch.randint(lo, hi + 1, shape, generator=g).float()      # noqa: E731
    c0, c1, c2, c3 = LARGE_CH
    nt = (Nk + TILE - 1) // TILE
    q = torch.zeros((B, H, Nq, 64))
    k = torch.zeros((B, H, Nk, 64))
    i = torch.arange(Nq)
    for b in range(B):
        for h in range(H):
            q[b, h, :, c0] = (72 + (i + 3 * b + 5 * h) % 9).float()
    q[..., c1] = 8.0
    q[..., c2], q[..., c3] = ri(-3, 3, (B, H, Nq)), ri(-3, 3, (B, H, Nq))
    k[..., c0] = 80.0 - ri(5, 40, (B, H, Nk))
    k[..., c1] = ri(-4, 0, (B, H, Nk))
    k[..., c2], k[..., c3] = ri(-3, 3, (B, H, Nk)), ri(-3, 3, (B, H, Nk))
    near = {}
    for t in range(nt):
        n_t = min(TILE, Nk - t * TILE)
        if placement == 'first':
            f0 = 0 if t <= 1 else -((t % 4) + 1)
        elif placement == 'last':
            f0 = 0 if t == nt - 1 else -1
        else:
            f0 = -min(4, nt - 1 - t)
        f1 =-1 if (placement == 'first' and t == 0) else max(f0 - 1, -4)
        for pos, f in (((13 * (t + 1)) % n_t, f0), ((13 * (t + 1) + 37) % n_t, f1)):
            near.setdefault(t * TILE + pos, f)
    for j, f in near.items():
        k[..., j, :] = 0.0
        k[..., j, c0], k[..., j, c1] = 80.0, float(f)
    v = torch.randn((B, H, Nk, 64), generator=g)
    s64 = q.double() @ k.double().transpose(-1, -2)
    p = torch.softmax(s64 * LARGE_SCALE, dim=-1)
    idx = torch.tensor(sorted(near))
    pn = p[..., idx]
    amax = s64.argmax(dim=-1)                                                  # first maximum
    cond = {'operands_exact': all(bool((x == x.bfloat16().float()).all()) and bool((x == x.half().float()).all()) for x in (q, k)),
            'scores_exact': bool(((q @ k.transpose(-1, -2)).double() == s64).all()),
            'score_min_max': float(s64.max(dim=-1).values.min()) * LARGE_SCALE,
            'near_share': float(pn.sum(-1).min()),
            'offmax_share': float((pn.sum(-1) - pn.max(dim=-1).values).min()),
            'near_tiles': len({j // TILE for j in near}),
            'max_tiles': sorted({int(x) // TILE for x in amax.flatten()}),
            'ntiles': nt}
    return q, k, v, cond


def check_large_conditions(cond, placement):
    """the conditions large_score_case is built to satisfy"""
    assert cond['operands_exact'] and cond['scores_exact']
    assert cond['score_min_max'] >= 710.0                                       # s c >= 1024: one fp32 ulp of the product s c is 2^-13
    assert cond['near_share'] >= LARGE_NEAR_SHARE and cond['offmax_share'] >= LARGE_OFFMAX_SHARE and cond['near_tiles'] >= 2
    assert cond['max_tiles'] == ([0] if placement == 'first' else [cond['ntiles'] - 1])


def value_cases():
    """every (name, builder arguments, scale) of the value cases 1-4, each as a callable returning (q, k, v, conditions)"""
    out = []
    for sh in SHAPES:
        out.append((f'random{sh}', (lambda sh=sh: random_case(*sh)), 0.125))
    for sh in OUTLIER_SHAPES:
        out.append((f'outlier{sh}', (lambda sh=sh: outlier_case(*sh)), 0.125))
    for sh in LARGE_SHAPES:
        for pl in LARGE_PLACEMENTS:
            out.append((f'large:{pl}{sh}', (lambda sh=sh, pl=pl: large_score_case(*sh, pl)), LARGE_SCALE))
    for sh in SCALE_SHAPES:
        for sc in SCALES:
            out.append((f'scale{sc}{sh}', (lambda sh=sh: random_case(*sh, seed=5)), sc))
    return out


def ratio(got, ref, bound):
    """largest |got - ref| / bound; inf where the result is not finite"""
    r = (got.double() - ref).abs() / bound
    return float('inf') if not bool(torch.isfinite(r).all()) else float(r.max())
