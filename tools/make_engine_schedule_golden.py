"""Records tests/golden/engine_schedule.json on the GPU: for ten small engine calls, the bytes the first call adds to the engine's workspace
(device_bytes() after minus before) and, with D3R_MODEL_OPT_PROFILE on, the ordered list of (kind, M, N, K) of every launch the call enqueues
(d3r_model_profile_launch). tests/test_forward_gpu.py::test_engine_schedule_matches_recorded replays the cases and requires equality: run this
BEFORE a change to the host side of the forward (csrc/engine.hip) that is meant to leave the launch sequence and the workspace layout alone.

    python tools/make_engine_schedule_golden.py
"""
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

OUT = os.path.join(ROOT, 'tests', 'golden', 'engine_schedule.json')
ENV_VARS = ('D3R_LN_FOLD', 'D3R_LN_INLINE_ROWS')
# name, configuration, precision, B, (H, W) of view 1, (H, W) of view 2, environment at engine creation, entry points
CASES = [
    dict(name='default', config='tiny_dpt', precision='fp16x3', B=1, hw1=[32, 48], hw2=[32, 48], env={}, calls=['forward']),
    dict(name='ln_finalize launched', config='tiny_dpt', precision='fp16x3', B=1, hw1=[32, 48], hw2=[32, 48], env={'D3R_LN_INLINE_ROWS': '0'}, calls=['forward']),
    dict(name='unfolded', config='tiny_dpt', precision='fp16x3', B=1, hw1=[32, 48], hw2=[32, 48], env={'D3R_LN_FOLD': '0'}, calls=['forward']),
    dict(name='mixed view sizes', config='tiny_dpt', precision='fp16x3', B=2, hw1=[32, 48], hw2=[48, 32], env={}, calls=['forward']),
    dict(name='two head chunks', config='tiny_dpt', precision='fp16x3', B=33, hw1=[32, 32], hw2=[32, 32], env={}, calls=['forward']),
    dict(name='fp32', config='tiny_dpt', precision='fp32', B=1, hw1=[32, 48], hw2=[32, 48], env={}, calls=['forward']),
    dict(name='bf16', config='tiny_dpt', precision='bf16', B=1, hw1=[32, 48], hw2=[32, 48], env={}, calls=['forward']),
    dict(name='fp16f8', config='tiny_dpt', precision='fp16f8', B=1, hw1=[32, 48], hw2=[32, 48], env={}, calls=['forward']),
    dict(name='linear head', config='tiny_linear', precision='fp16x3', B=3, hw1=[32, 32], hw2=[32, 32], env={}, calls=['forward']),
    dict(name='encode then decode', config='tiny_dpt', precision='fp16x3', B=1, hw1=[32, 48], hw2=[32, 48], env={}, calls=['encode', 'decode']),
]


def run_case(case, dev):
    """one fresh engine: [{call, workspace_bytes (growth of device_bytes() over the call), launches ((kind, M, N, K) in enqueue order)}] for the case's calls"""
    import torch
    from dust3r_amd._lib import lib
    from dust3r_amd.model import AsymmetricCroCo3DStereo
    from dust3r_amd.synthetic import MODEL_CONFIGS, synthetic_views
    from oracle.dust3r_ref import build_ref_model
    saved = {name: os.environ.pop(name, None) for name in ENV_VARS}
    os.environ.update(case['env'])
    try:
        model = AsymmetricCroCo3DStereo(precision=case['precision'], landscape_only=False, **MODEL_CONFIGS[case['config']])
        model.load_state_dict(build_ref_model(case['config']).state_dict(), strict=True)
        model = model.to(dev)          # the engine reads the switches here
    finally:
        for name in ENV_VARS:
            os.environ.pop(name, None)
        os.environ.update({name: v for name, v in saved.items() if v is not None})
    B, (H1, W1), (H2, W2) = case['B'], case['hw1'], case['hw2']
    v1, v2 = synthetic_views(B, H1, W1, seed=1)[0], synthetic_views(B, H2, W2, seed=2)[1]
    lib.d3r_model_set_option(model._engine, 1, 1)      # D3R_MODEL_OPT_PROFILE
    out, feat = [], None
    kind, M, N, K, ms, work = C.c_int(), C.c_int(), C.c_int(), C.c_int(), C.c_double(), C.c_double()
    for call in case['calls']:
        before = model.device_bytes()
        if call == 'forward':
            model(v1, v2)
        elif call == 'encode':
            feat = model.encode_images(torch.cat((v1['img'], v2['img'])))
        else:
            model.decode_pairs(feat, H1, W1)
        torch.cuda.synchronize()
        rec = dict(call=call, workspace_bytes=model.device_bytes() - before, launches=[])
        while lib.d3r_model_profile_launch(model._engine, len(rec['launches']), C.byref(kind), C.byref(M), C.byref(N), C.byref(K), C.byref(ms), C.byref(work)) == 0:
            rec['launches'].append([kind.value, M.value, N.value, K.value])
        out.append(rec)
    model._destroy_engine()
    return out


def main():
    import torch
    dev = torch.device('cuda:0')
    table = dict(cases=CASES, recorded=[run_case(case, dev) for case in CASES])
    for case, rec in zip(CASES, table['recorded']):
        print(case['name'], [(r['call'], r['workspace_bytes'], len(r['launches'])) for r in rec])
    with open(OUT, 'w') as f:
        json.dump(table, f, separators=(',', ':'))
        f.write('\n')
    print(OUT, os.path.getsize(OUT), 'bytes')


if __name__ == '__main__':
    main()
