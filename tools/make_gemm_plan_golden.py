"""Records tests/golden/gemm_plan_table.json: what the two host queries of the GEMM dispatch (d3r_gemm_tile_config, d3r_linear_heads_tile_config;
no device needed, the CU count falls back to the MI355X's 256) answer over a grid of shapes, operand types, epilogues and D3R_GEMM_* environments.
tests/test_host_cpu.py::test_gemm_plan_matches_recorded_table replays the grid and requires the same answers: run this BEFORE a change to the
dispatch that is meant to leave the decision alone, not after. D3R_GEMM_NOWIDE is recorded for the heads query only.

    python tools/make_gemm_plan_golden.py
"""
import ctypes as C
import itertools
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from dust3r_amd import _lib  # noqa: E402

OUT = os.path.join(ROOT, 'tests', 'golden', 'gemm_plan_table.json')
ENV_VARS = ('D3R_GEMM_CFG', 'D3R_GEMM_PERSIST', 'D3R_GEMM_T128W8', 'D3R_GEMM_NOWIDE')
CODES = '0123456789abc'      # one character per answer: tile codes 0 .. 11 of d3r_gemm_tile_config, c = D3R_TILE_128W8 (12)
DTYPES = ['bf16', 'fp16', 'fp32', 'fp16x3', 'fp16f8', 'fp16x2f8']
TILE_GRID = dict(
    order='for dtype, for M, for N, for K, for epilogue (innermost)',
    dtype=DTYPES,
    M=[96, 768, 1152, 1536, 2304, 3072, 6144, 12288, 16896, 24576, 49152, 196608, 6291456],
    N=[96, 128, 256, 768, 1024, 1536, 2304, 3072, 4096],
    K=[768, 1024, 3072, 4096],
    epilogue=[['plain', 0, 0], ['fp32', 1, 0], ['fp32 + residual', 1, 1], ['gelu', 2, 0]])      # name, `epilogue`, `with_residual` of d3r_gemm_tile_config
TILE_ENVS = [{}, {'D3R_GEMM_PERSIST': '0'}, {'D3R_GEMM_PERSIST': '1'}, {'D3R_GEMM_T128W8': '0'}] + \
            [{'D3R_GEMM_CFG': str(c)} for c in (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 11)]
# dtypes and region-kind lists of tests/test_gemm_heads_gpu.py (CFGS, LAYOUTS); M = B th tw, ntok = th tw, tok_w = tw, ldv = round_up(ntok, 64),
# heads = head_c / 64, K = head_c, max_pos = 512
HEADS_GRID = dict(
    order='for dtype, for kinds, for (th, tw), for B, for head_c (innermost)',
    dtype=['fp32', 'bf16', 'fp16', 'fp16x3', 'fp16f8', 'fp16x2f8'],
    kinds=[['rope', 'rope', 'vt'], ['rope'], ['rope', 'vt'], ['plain', 'vt']],
    tokens=[[2, 2], [8, 8], [24, 32], [32, 32]],
    B=[1, 2, 64],
    head_c=[768, 1024])
HEADS_ENVS = [{}, {'D3R_GEMM_NOWIDE': '1'}]
KIND = {'rope': _lib.HEAD_ROPE, 'vt': _lib.HEAD_VT, 'plain': _lib.HEAD_PLAIN}


def set_env(env):
    for name in ENV_VARS:
        os.environ.pop(name, None)
    os.environ.update(env)


def encode(codes):
    assert all(0 <= c < len(CODES) for c in codes), sorted(set(codes))
    return ''.join(CODES[c] for c in codes)


def tile_answers(grid):
    lib = _lib.lib
    return encode([lib.d3r_gemm_tile_config(_lib.DTYPES[dt], M, N, K, epi, res)
                   for dt, M, N, K, (_, epi, res) in itertools.product(grid['dtype'], grid['M'], grid['N'], grid['K'], grid['epilogue'])])


def heads_answers(grid):
    lib = _lib.lib
    out = []
    for dt, kinds, (th, tw), B, head_c in itertools.product(grid['dtype'], grid['kinds'], grid['tokens'], grid['B'], grid['head_c']):
        ntok = th * tw
        kk = (C.c_int * 3)(*([KIND[k] for k in kinds] + [0] * (3 - len(kinds))))
        out.append(lib.d3r_linear_heads_tile_config(B * ntok, head_c, len(kinds), head_c, kk, head_c // 64, ntok, tw, (ntok + 63) // 64 * 64, 512, _lib.DTYPES[dt]))
    return encode(out)


def replay(table):
    """the answers of THIS build over the recorded grids, in the file's layout (the test compares them with the file's)"""
    saved = {name: os.environ.get(name) for name in ENV_VARS}
    try:
        got = {}
        for key, fn in (('tile_config', tile_answers), ('heads_tile_config', heads_answers)):
            got[key] = []
            for env in table[key]['envs']:
                set_env(env)
                got[key].append(fn(table[key]['grid']))
        return got
    finally:
        set_env({k: v for k, v in saved.items() if v is not None})


def main():
    table = dict(codes=CODES, tile_config=dict(grid=TILE_GRID, envs=TILE_ENVS), heads_tile_config=dict(grid=HEADS_GRID, envs=HEADS_ENVS))
    got = replay(table)
    for key in got:
        table[key]['answers'] = got[key]
        print(key, len(got[key]), 'environments x', len(got[key][0]), 'points; codes seen:', ''.join(sorted(set(''.join(got[key])))))
    with open(OUT, 'w') as f:
        json.dump(table, f, separators=(',', ':'))
        f.write('\n')
    print(OUT, os.path.getsize(OUT), 'bytes')


if __name__ == '__main__':
    main()
