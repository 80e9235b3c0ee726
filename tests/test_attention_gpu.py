"""The attention kernels of csrc/attention.hip at kernel level against fp64, element by element (oracle/attention_ref.py: the reference of the operands as
stored, the derived per-element bound, the seeded cases; tests/test_attention_cpu.py shows without a device that the bound holds for a correct fp32
evaluation and that subtly wrong ones leave it).

Arms and the instantiation launch_attention dispatches for each (the x3 kernel is chosen by the environment, read on every launch):
    fp32        attention_kernel<D3R_F32>
    bf16        attention_kernel<D3R_BF16>
    fp16        attention_kernel<D3R_F16>
    x3-v1       attention_kernel<D3R_F16X3>                       D3R_ATTN_V1=1
    x3-reg      attention_x3_kernel<D3R_F16X3, false, false>      D3R_ATTN_DMA=0
    x3-dma      attention_x3_kernel<D3R_F16X3, true, true>        the default
    x3-v1+f8    attention_kernel<D3R_F16X3, D3R_F16F8>            fp16 + fp8 output rows through d3r_attention_rows
    x3-reg+f8   attention_x3_kernel<D3R_F16F8, false, false>
    x3-dma+f8   attention_x3_kernel<D3R_F16F8, true, true>
Every launch writes into a buffer with 256 sentinel elements in front of and behind the output; both guards must be intact and no sentinel left inside."""
import ctypes as C
import functools

import pytest
import torch

from oracle import attention_ref as R

pytestmark = pytest.mark.gpu

ARMS = list(R.ARMS)
SENTINEL_BYTE, SENTINEL_WORD = 0xA5, -1515870811      # 0xA5A5A5A5 as int32
CASES = {name: (build, scale) for name, build, scale in R.value_cases()}


def _set_arm(monkeypatch, arm):
    kern = arm.split('+')[0]
    monkeypatch.setenv('D3R_ATTN_V1', '1' if kern == 'x3-v1' else '0')
    monkeypatch.setenv('D3R_ATTN_DMA', '0' if kern == 'x3-reg' else '1')


def _pack(x, operand):
    from dust3r_amd import ops
    tdt = {'fp32': torch.float32, 'bf16': torch.bfloat16, 'fp16': torch.float16}
    return ops.pack_x3(x) if operand == 'x3' else x.to(tdt[operand]).contiguous()


def run_arm(gpu, arm, q, k, v, scale, ldv=None, pad=None, out_rows=None):
    """One guarded launch. q (B,H,Nq,64), k, v (B,H,Nk,64) fp32 on the CPU; pad: the (B,H,64,ldv) fp32 image the V^T columns are written into (None: zeros);
    out_rows: a dtype id sent through d3r_attention_rows (None: the arm's entry point). Returns (decoded fp64 (B,Nq,H*64) on the CPU, stored bytes)."""
    from dust3r_amd import _lib, ops
    operand, rows = R.ARMS[arm]
    B, H, Nq, _ = q.shape
    Nk = k.shape[2]
    ldv = (Nk + 63) // 64 * 64 if ldv is None else ldv
    vt = torch.zeros((B, H, 64, ldv)) if pad is None else pad.clone()
    vt[..., :Nk] = v.transpose(-1, -2)
    qp, kp, vp = (_pack(x.to(gpu), operand) for x in (q, k, vt))
    if out_rows is None and rows == 'f8':
        out_rows = _lib.DTYPE_F16F8
    f8 = out_rows in (_lib.DTYPE_F16F8, _lib.DTYPE_F16X2F8)
    eb = 4 if (f8 or operand in ('fp32', 'x3')) else 2      # stored bytes per logical element
    n, guard = B * Nq * H * 64 * eb, 256 * eb
    buf = torch.full((guard + n + guard,), SENTINEL_BYTE, dtype=torch.uint8, device=gpu)
    out = buf[guard:guard + n]
    dt = {'fp32': _lib.DTYPE_F32, 'bf16': _lib.DTYPE_BF16, 'fp16': _lib.DTYPE_F16, 'x3': _lib.DTYPE_F16X3}[operand]
    args = (_lib.ptr(qp), _lib.ptr(kp), _lib.ptr(vp), C.c_void_p(out.data_ptr()), B, H, Nq, Nk, ldv, scale, dt)
    if out_rows is None:
        _lib.check(_lib.lib.d3r_attention(*args, _lib.current_stream()), f'attention {arm}')
    else:
        _lib.check(_lib.lib.d3r_attention_rows(*args, out_rows, _lib.current_stream()), f'attention_rows {arm}')
    torch.cuda.synchronize()
    words, g = buf.view(torch.int32), guard // 4
    assert bool((words[:g] == SENTINEL_WORD).all()), (arm, 'guard in front of the output overwritten', tuple(q.shape), Nk)
    assert bool((words[-g:] == SENTINEL_WORD).all()), (arm, 'guard behind the output overwritten', tuple(q.shape), Nk)
    left = int((words[g:-g] == SENTINEL_WORD).sum())
    assert left == 0, (arm, f'{left} sentinel words left inside the output', tuple(q.shape), Nk)
    raw = out.clone()
    if f8:
        dec = ops.unpack_f8(raw.view(B, Nq, H * 256))
    elif operand == 'x3':
        dec = ops.unpack_x3(raw.view(torch.float16).view(B, Nq, H * 128))
    else:
        dec = raw.view({'fp32': torch.float32, 'bf16': torch.bfloat16, 'fp16': torch.float16}[operand]).view(B, Nq, H * 64)
    return dec.double().cpu(), raw


@functools.lru_cache(maxsize=None)
def _inputs(name):
    return CASES[name][0]()


@functools.lru_cache(maxsize=None)
def _ref_and_bound(name, operand, rows):
    """computed once per arithmetic class, shared by the arms of that class, never modified"""
    q, k, v, _ = _inputs(name)
    cls = next(a for a in R.EMULATION_CLASSES if R.ARMS[a] == (operand, rows))
    scale = CASES[name][1]
    return R.attention_fp64(R.stored(q, operand), R.stored(k, operand), R.stored(v, operand), scale), R.elementwise_bound(q, k, v, scale, cls)


@pytest.mark.parametrize('arm', ARMS)
def test_every_element_within_the_derived_bound(gpu, arm, monkeypatch):
    """Cases 1-4 (random on every shape of the list, outlier channels, large exact scores with near ties in three placements, scale 0.1 and 1.0): every output
    element within elementwise_bound of the fp64 result of the stored operands. Prints the largest error / bound ratio of the arm."""
    _set_arm(monkeypatch, arm)
    worst, over = (0.0, ''), []
    for name in CASES:
        q, k, v, _ = _inputs(name)
        ref, bound = _ref_and_bound(name, *R.ARMS[arm])
        got, _ = run_arm(gpu, arm, q, k, v, CASES[name][1])
        r = R.ratio(got, ref, bound)
        if r >= worst[0]:
            worst = (r, name)
        if not r < 1.0:
            over.append((name, r))
    print(f'attention {arm:10s}: largest error / bound {worst[0]:.3f} ({worst[1]}) over {len(CASES)} cases')
    assert not over, (arm, over)


@pytest.mark.parametrize('arm', ARMS)
def test_stale_vt_padding_changes_no_bit(gpu, arm, monkeypatch):
    """Case 5: columns Nk .. ldv-1 of V^T hold finite values up to 1e4 (what the other image's layout leaves in the engine's workspace), ldv the rounded-up key
    count and one tile more: the stored rows are the bits of the zero-padded call."""
    _set_arm(monkeypatch, arm)
    B, H, Nq = 2, 3, 33
    for Nk in R.PAD_NK:
        q, k, v, _ = R.random_case(B, H, Nq, Nk, seed=9)
        base = (Nk + 63) // 64 * 64
        outs = []
        for ldv in (base, base + 64):
            g = torch.Generator().manual_seed(1000 + Nk + ldv)
            pad = (torch.rand((B, H, 64, ldv), generator=g) * 2 - 1) * 1e4
            zero = run_arm(gpu, arm, q, k, v, 0.125, ldv=ldv)[1]
            stale = run_arm(gpu, arm, q, k, v, 0.125, ldv=ldv, pad=pad)[1]
            assert torch.equal(zero, stale), (arm, Nk, ldv, int((zero != stale).sum()))
            outs.append(zero)
        assert torch.equal(outs[0], outs[1]), (arm, Nk, 'ldv')


@pytest.mark.parametrize('arm', ARMS)
def test_every_batch_and_head_has_the_bits_of_its_own_launch(gpu, arm, monkeypatch):
    """Case 6: every (b, h) of a (2, 3) and of a (1, 17) call, run alone with B = H = 1, stores the bytes of its slice of the batched call (grids of 12 and 34
    workgroups against 2: xcd_remap and the (b, h, query block) decomposition)."""
    _set_arm(monkeypatch, arm)
    Nq, Nk = 129, 65
    for B, H in R.POSITION_BH:
        q, k, v, _ = R.random_case(B, H, Nq, Nk, seed=4)
        full = run_arm(gpu, arm, q, k, v, 0.125)[1]
        full = full.view(B, Nq, H, -1)
        for b in range(B):
            for h in range(H):
                one = run_arm(gpu, arm, q[b:b + 1, h:h + 1], k[b:b + 1, h:h + 1], v[b:b + 1, h:h + 1], 0.125)[1]
                assert torch.equal(one.view(Nq, -1), full[b, :, h]), (arm, B, H, b, h)


@pytest.mark.parametrize('rows', ['', '+f8'])
def test_staging_arms_are_bit_identical_on_every_ragged_shape(gpu, rows, monkeypatch):
    """Case 7: register staging with packed softmax slices against DMA staging with scalar ones, on every shape of the list."""
    for sh in R.SHAPES:
        q, k, v, _ = _inputs(f'random{sh}')
        outs = []
        for arm in ('x3-reg' + rows, 'x3-dma' + rows):
            _set_arm(monkeypatch, arm)
            outs.append(run_arm(gpu, arm, q, k, v, 0.125)[1])
        assert torch.equal(outs[0], outs[1]), (sh, rows, int((outs[0] != outs[1]).sum()))


def test_rows_entry_point_names_the_same_kernels(gpu, monkeypatch):
    """d3r_attention_rows with the operands' own layout stores the bytes of d3r_attention; fp16x2f8 names the fp16 + fp8 rows; ops.attention_x3(out_rows=) decodes
    the same launch."""
    from dust3r_amd import _lib, ops
    q, k, v, _ = _inputs('random(1, 5, 33, 63)')
    for arm, dt in (('fp32', _lib.DTYPE_F32), ('bf16', _lib.DTYPE_BF16), ('fp16', _lib.DTYPE_F16), ('x3-dma', _lib.DTYPE_F16X3), ('x3-v1', _lib.DTYPE_F16X3)):
        _set_arm(monkeypatch, arm)
        assert torch.equal(run_arm(gpu, arm, q, k, v, 0.125)[1], run_arm(gpu, arm, q, k, v, 0.125, out_rows=dt)[1]), arm
    _set_arm(monkeypatch, 'x3-dma+f8')
    dec, raw = run_arm(gpu, 'x3-dma+f8', q, k, v, 0.125)
    assert torch.equal(raw, run_arm(gpu, 'x3-dma', q, k, v, 0.125, out_rows=_lib.DTYPE_F16X2F8)[1])
    assert torch.equal(ops.attention_x3(q.to(gpu), k.to(gpu), v.to(gpu), scale=0.125, out_rows='fp16f8').double().cpu(), dec)
    assert torch.equal(ops.attention_x3(q.to(gpu), k.to(gpu), v.to(gpu), scale=0.125).double().cpu(), run_arm(gpu, 'x3-dma', q, k, v, 0.125)[0])
