"""CPU pins of what tests/test_attention_gpu.py holds the attention kernels to (oracle/attention_ref.py): the derived per-element bound contains an fp32
emulation of the kernels' algorithm on every value case and every arm, every deliberate defect of that emulation leaves the bound on a named case, the
inputs satisfy the conditions they are built for, and the C entry points reject bad arguments before any launch. No device.

Which case catches which defect (asserted below, ratios printed with -s):
    mask_off_by_one              random (1, 1, 31, 63)        every arm     (the last key of a ragged tile is dropped)
    halves_disagree_on_max       random (1, 1, 32, 64)        every arm
    no_rescale_when_max_moves    large:grow (2, 3, 129, 129)  every arm
    unfused_exponent             large:first, every shape     fp32 and split-fp16 arms with split-fp16 rows; NOT caught by any random case on any arm.
                                 Rounding s c first costs half an ulp of |s c| >= 1024, 2^-14, per key: below the unit roundoff of a bf16 / fp16 P or of
                                 an fp16 + fp8 output row, so those arms cannot see it at scores of several hundred, and it drowns in the rounding of m c
                                 (term (d) of the bound) once the maximum moves between tiles -- hence the placement with the maximum in the first tile.
    p_not_rounded                passes everywhere (not a defect)
The bit-identity cases (stale V^T padding, position independence, staging arms) have no value to bound and live in the GPU file only."""
import ctypes as C
import functools

from oracle import attention_ref as R

CASES = {name: (build, scale) for name, build, scale in R.value_cases()}


@functools.lru_cache(maxsize=None)
def _inputs(name):
    return CASES[name][0]()


@functools.lru_cache(maxsize=None)
def _ref_and_bound(name, arm):
    q, k, v, _ = _inputs(name)
    scale, op = CASES[name][1], R.ARMS[arm][0]
    return R.attention_fp64(R.stored(q, op), R.stored(k, op), R.stored(v, op), scale), R.elementwise_bound(q, k, v, scale, arm)


def _ratio(name, arm, variant=None):
    q, k, v, _ = _inputs(name)
    ref, bound = _ref_and_bound(name, arm)
    return R.ratio(R.online_softmax_emulated(q, k, v, CASES[name][1], arm, variant), ref, bound)


def test_shape_list_covers_what_the_kernels_branch_on():
    nq, nk = [s[2] for s in R.SHAPES], [s[3] for s in R.SHAPES]
    assert all(nq.count(x) >= 2 for x in (1, 31, 32, 33, 127, 128, 129, 257)) and all(nk.count(x) >= 2 for x in (1, 63, 64, 65, 127, 129, 191, 193, 321))
    assert {(s[0], s[1]) for s in R.SHAPES} <= {(1, 1), (2, 3), (1, 5), (3, 1), (1, 17)}
    assert {1, 3, 5, 6, 9, 17} <= {R.workgroups(*s[:3]) for s in R.SHAPES}
    assert {(s[3] + 63) // 64 for s in R.SHAPES} == {1, 2, 3, 4, 6}      # one tile left and two tiles left, with and without full double steps in front


def test_inputs_satisfy_their_conditions():
    for name in CASES:
        cond = _inputs(name)[3]
        if name.startswith('large:'):
            R.check_large_conditions(cond, name.split(':')[1].split('(')[0])
        elif name.startswith('outlier'):
            assert cond['expo_min'] == -10 and cond['expo_max'] == 10 and cond['column_ratio'] > 2.0 ** 17
        elif name.startswith('random'):
            assert cond['score_absmax_at_0.125'] < 60.0


def test_emulation_stays_within_the_bound_on_every_case_and_arm():
    """variant=None and the harmless 'p_not_rounded': the bound and the inputs hold without a GPU. Largest error / bound ratio per arm printed."""
    worst = {}
    for name in CASES:
        for cls in R.EMULATION_CLASSES:
            r, rp = _ratio(name, cls), _ratio(name, cls, 'p_not_rounded')
            assert r < 1.0 and rp < 1.0, (name, cls, r, rp)
            if r >= worst.get(cls, (-1.0, ''))[0]:
                worst[cls] = (r, name)
    for arm, (op, rows) in R.ARMS.items():
        cls = next(c for c in R.EMULATION_CLASSES if R.ARMS[c] == (op, rows))
        print(f'emulation {arm:10s}: largest error / bound {worst[cls][0]:.3f} ({worst[cls][1]})')


def test_bound_follows_the_score_magnitude_and_the_column():
    """what one global tolerance cannot do: the bound of a large-score row whose maximum moves is far above the one of a row whose maximum stays (term (d)),
    and the bound of a small column is small (outlier channels)."""
    b_first = _ref_and_bound('large:first(2, 3, 129, 129)', 'x3-dma')[1]
    b_grow = _ref_and_bound('large:grow(2, 3, 129, 129)', 'x3-dma')[1]
    assert float(b_grow.median()) > 5 * float(b_first.median())
    b = _ref_and_bound('outlier(2, 3, 127, 127)', 'x3-dma')[1].reshape(2, 127, 3, 64)
    assert float(b[..., 0].max()) < 2.0 ** -15 * float(b[..., 63].min())


def test_every_defect_is_caught_by_its_named_case():
    every = R.EMULATION_CLASSES
    table = [('mask_off_by_one', 'random(1, 1, 31, 63)', every), ('halves_disagree_on_max', 'random(1, 1, 32, 64)', every),
             ('no_rescale_when_max_moves', 'large:grow(2, 3, 129, 129)', every)]
    table += [('unfused_exponent', f'large:first{sh}', ['fp32', 'x3-dma']) for sh in R.LARGE_SHAPES]
    for variant, name, classes in table:
        for cls in classes:
            r = _ratio(name, cls, variant)
            print(f'{variant:26s} {name:30s} {cls:10s}: error / bound {r:.3g}')
            assert not r < 1.0, (variant, name, cls, r)
    for name in CASES:
        if name.startswith('random'):
            for cls in every:
                r = _ratio(name, cls, 'unfused_exponent')
                assert r < 1.0, ('the random case must not see the un-fused exponent', name, cls, r)
    worst = max(_ratio(name, cls, 'unfused_exponent') for name in CASES if name.startswith('random') for cls in every)
    print(f'unfused_exponent on the random cases: largest error / bound {worst:.3g} (not caught)')


def test_attention_entry_points_reject_bad_arguments():
    """d3r_attention / d3r_attention_rows argument checks (host side: they return before any launch)."""
    from dust3r_amd import _lib
    lib = _lib.lib
    assert {'d3r_attention', 'd3r_attention_rows'} <= set(_lib.EXPORTED)
    x3, f8, x2f8 = _lib.DTYPE_F16X3, _lib.DTYPE_F16F8, _lib.DTYPE_F16X2F8
    buf = (C.c_float * 64)()
    INVALID, LAUNCH_INVALID = -1, 1001      # D3R_ERR_INVALID; 1000 + hipErrorInvalidValue of the launcher's own checks

    def plain(q=buf, k=buf, vt=buf, out=buf, B=1, H=1, Nq=5, Nk=70, ldv=128, dt=x3):
        return lib.d3r_attention(q, k, vt, out, B, H, Nq, Nk, ldv, 0.125, dt, None)

    def rows(q=buf, k=buf, vt=buf, out=buf, B=1, H=1, Nq=5, Nk=70, ldv=128, dt=x3, out_rows=f8):
        return lib.d3r_attention_rows(q, k, vt, out, B, H, Nq, Nk, ldv, 0.125, dt, out_rows, None)

    for call in (plain, rows):
        assert call(q=None) == INVALID and call(k=None) == INVALID and call(vt=None) == INVALID and call(out=None) == INVALID
        assert call(B=0) == LAUNCH_INVALID and call(H=0) == LAUNCH_INVALID and call(Nq=0) == LAUNCH_INVALID and call(Nk=0) == LAUNCH_INVALID
        assert call(B=-1) == LAUNCH_INVALID and call(Nk=-3) == LAUNCH_INVALID
        assert call(ldv=100) == LAUNCH_INVALID and call(ldv=64) == LAUNCH_INVALID and call(Nk=129, ldv=128) == LAUNCH_INVALID
    assert plain(dt=f8, ldv=128) == LAUNCH_INVALID and plain(dt=9) == LAUNCH_INVALID      # no attention kernel takes fp16 + fp8 operands
    # an output layout the operand type does not support
    assert rows(out_rows=-1) == INVALID and rows(out_rows=6) == INVALID
    for dt in (_lib.DTYPE_BF16, _lib.DTYPE_F16, _lib.DTYPE_F32):
        assert rows(dt=dt, out_rows=f8) == LAUNCH_INVALID and rows(dt=dt, out_rows=x2f8) == LAUNCH_INVALID and rows(dt=dt, out_rows=x3) == LAUNCH_INVALID
    assert rows(dt=x3, out_rows=_lib.DTYPE_F32) == LAUNCH_INVALID and rows(dt=x3, out_rows=_lib.DTYPE_F16) == LAUNCH_INVALID
    assert rows(dt=f8, out_rows=f8) == LAUNCH_INVALID
