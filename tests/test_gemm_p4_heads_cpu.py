"""The dispatch of the attention projections onto the persistent GEMM (csrc/gemm_plan.hpp, gemm_p4_eligible), through the host query d3r_linear_heads_tile_config:
no device."""
import pytest

ENV = ('D3R_GEMM_CFG', 'D3R_GEMM_PERSIST', 'D3R_GEMM_T128W8', 'D3R_GEMM_NOWIDE')


@pytest.fixture
def cfg(monkeypatch):
    from dust3r_amd import ops
    for name in ENV:
        monkeypatch.delenv(name, raising=False)

    def ask(kinds, pairs, head_c, th=24, tw=32, K=None, dtype='fp16x3', images=2):      # images per pair in one launch: 2 in the encoder, 1 per decoder side
        ntok = th * tw
        return ops.heads_tile_config(images * pairs * ntok, K or head_c, list(kinds), head_c, ntok, tw, (ntok + 63) // 64 * 64, dtype)
    return ask


def test_encoder_qk_launch_takes_the_persistent_kernel(cfg, monkeypatch):
    """[rope, rope] at M = 49152 (32 pairs of 24 x 32 tokens), head_c = 1024: 3072 tiles = 12 whole rounds of 256 CUs -> configuration 10 by default; never under
    D3R_GEMM_PERSIST=0, D3R_GEMM_NOWIDE=1 or a pinned tile, never at one pair per call (96 tiles), never for another operand type."""
    qk = ('rope', 'rope')
    assert cfg(qk, 32, 1024) == 10
    assert cfg(qk, 1, 1024) != 10
    assert cfg(qk, 32, 1024, dtype='bf16') != 10 and cfg(qk, 32, 1024, dtype='fp16f8') != 10
    for name, val in (('D3R_GEMM_PERSIST', '0'), ('D3R_GEMM_NOWIDE', '1'), ('D3R_GEMM_CFG', '1')):
        monkeypatch.setenv(name, val)
        assert cfg(qk, 32, 1024) != 10, name
        monkeypatch.delenv(name)


def test_launches_the_drain_cannot_store_stay(cfg, monkeypatch):
    """V^T and unrotated regions are declined whatever the mode; so is a token count that lets a 16-row fragment straddle two images, a grid past the kernel's table
    copy, fewer than 18 K steps and fewer than 8 tiles. By default the q | k | v launch, the decoder's q | k (4.5 rounds) and one-region launches keep their recorded tiles."""
    monkeypatch.setenv('D3R_GEMM_PERSIST', '1')
    assert cfg(('rope', 'rope'), 32, 1024) == 10 and cfg(('rope',), 32, 1024) == 10 and cfg(('rope', 'rope', 'rope'), 32, 1024) == 10
    for kinds in (('rope', 'rope', 'vt'), ('rope', 'vt'), ('vt',), ('plain', 'plain')):
        assert cfg(kinds, 32, 1024) != 10, kinds
    assert cfg(('rope', 'rope'), 32, 1024, th=3, tw=8) != 10            # ntok = 24
    assert cfg(('rope', 'rope'), 4, 1024, th=2, tw=128) != 10           # 128 positions along x
    assert cfg(('rope', 'rope'), 32, 512, K=512) != 10                  # 16 K steps
    assert cfg(('rope', 'rope'), 2, 128, th=16, tw=16, K=768) == 10     # 4 x 2 = 8 tiles
    assert cfg(('rope', 'rope'), 1, 128, th=16, tw=16, K=768) != 10     # 2 x 2 = 4 tiles
    monkeypatch.delenv('D3R_GEMM_PERSIST')
    assert cfg(('rope', 'rope', 'vt'), 32, 1024) == 1                   # as issued before the split, as recorded
    assert cfg(('rope', 'rope'), 32, 768, images=1) != 10                         # the decoder's side: 24576 x 1536 = 1152 tiles = 4.5 rounds
    assert cfg(('rope',), 32, 1024) != 10 and cfg(('vt',), 32, 1024) == 1


def test_heads_instances_have_no_scratch():
    """hipcc's resource report of gemm_p4_heads.hip (written next to the object by the build, read only here): the two attention-projection instances keep both accumulator
    sets in registers -- no scratch, no spilled VGPR, one wave per SIMD -- like the four instances of gemm_p4.hip that tests/test_host_cpu.py checks."""
    import os
    import re
    from dust3r_amd.build import CSRC
    rep = os.path.join(CSRC, 'gemm_p4_heads.resources.txt')
    assert os.path.exists(rep), 'the build writes the report next to gemm_p4_heads.o'
    blocks = re.split(r'(?=Function Name: )', open(rep).read())
    heads = [b for b in blocks if re.match(r'Function Name: \S*gemm_p4_heads_kernel', b)]
    assert sorted(int(re.search(r'gemm_p4_heads_kernelILi(\d+)E', b).group(1)) for b in heads) == [4, 5]
    for b in heads:
        assert int(re.search(r'ScratchSize \[bytes/lane\]: (\d+)', b).group(1)) == 0, b
        assert int(re.search(r'VGPRs Spill: (\d+)', b).group(1)) == 0 and int(re.search(r'Occupancy \[waves/SIMD\]: (\d+)', b).group(1)) == 1, b
