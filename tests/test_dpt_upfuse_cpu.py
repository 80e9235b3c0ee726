"""The dispatch of the fused x2 bilinear map + 3x3 convolution (csrc/gemm_plan.hpp conv_up2_fused) through its host query d3r_up2_conv_route: no GPU, no launch.
Without a device the rule counts the MI355X's 256 compute units."""
import pytest


def route(*a, **k):
    from dust3r_amd import ops
    return ops.up2_conv_route(*a, **k)


def test_eligible_geometries(monkeypatch):
    monkeypatch.delenv('D3R_UP2_MIN_TILES', raising=False)
    monkeypatch.delenv('D3R_GEMM_CFG', raising=False)
    assert route(32, 192, 256, 128, 128)        # the 32-pair step at 512 x 384: 12288 tiles of 16 x 32
    assert route(1, 192, 256, 128, 128)         # one pair: 384 tiles, more than one per compute unit
    assert route(3, 112, 112, 128, 128)         # 224 x 224: 98 tiles per image, three images fill the chip ...
    assert route(1, 192, 256, 128, 64)          # fewer output channels


def test_ineligible_geometries(monkeypatch):
    monkeypatch.delenv('D3R_UP2_MIN_TILES', raising=False)
    monkeypatch.delenv('D3R_GEMM_CFG', raising=False)
    assert not route(2, 112, 112, 128, 128)     # ... two do not: 196 tiles
    assert not route(32, 256, 168, 128, 128)    # portrait 512 x 336: 336 is not whole 32-pixel tiles
    assert not route(32, 100, 256, 128, 128)    # 200 rows: not whole 16-pixel tiles
    assert not route(32, 192, 256, 128, 256)    # more channels than a wave holds
    assert not route(32, 192, 256, 128, 126)    # the tail works on groups of four channels
    assert not route(32, 192, 256, 48, 128, cstride=48)     # not whole 32-channel K slices
    monkeypatch.setenv('D3R_GEMM_CFG', '3')     # a pinned tile configuration keeps the generic kernel
    assert not route(32, 192, 256, 128, 128)


def test_typed_store_route(monkeypatch):
    """head4=False: the typed-store launch (head.0, 256 -> 128 channels on the 192 x 256 map of a 512 x 384 image: 96 tiles per image)."""
    monkeypatch.delenv('D3R_UP2_MIN_TILES', raising=False)
    monkeypatch.delenv('D3R_GEMM_CFG', raising=False)
    assert route(32, 96, 128, 256, 128, head4=False)
    assert route(3, 96, 128, 256, 128, head4=False)           # 288 tiles
    assert not route(2, 96, 128, 256, 128, head4=False)       # 192 tiles: fewer than one per compute unit
    assert not route(32, 96, 128, 256, 124, head4=False)      # whole 8-channel groups are stored
    assert not route(32, 128, 84, 256, 128, head4=False)      # portrait: 168 columns are not whole tiles
    assert not route(32, 96, 128, 256, 128, head4=False, dtype='bf16')


def test_tile_floor_override(monkeypatch):
    monkeypatch.delenv('D3R_GEMM_CFG', raising=False)
    monkeypatch.delenv('D3R_UP2_MIN_TILES', raising=False)
    assert not route(1, 8, 16, 128, 128)
    monkeypatch.setenv('D3R_UP2_MIN_TILES', '1')
    assert route(1, 8, 16, 128, 128)
    assert not route(1, 12, 16, 128, 128)       # the floor does not make 24 rows whole tiles


@pytest.mark.parametrize('dtype', ['bf16', 'fp16', 'fp32'])
def test_other_precisions_are_refused(dtype, monkeypatch):
    monkeypatch.setenv('D3R_UP2_MIN_TILES', '1')
    assert not route(32, 192, 256, 128, 128, dtype=dtype)


def test_fused_kernel_keeps_its_accumulators_in_registers():
    """The compiler's resource report of csrc/gemm_up2.hip (written next to the library by dust3r_amd/build.py): two instances, no scratch, no spill, two waves per
    SIMD -- 128 accumulators, the staging temporaries and the DMA addresses fit the 256 registers of a 512-thread block."""
    import os
    import re
    from dust3r_amd import _lib
    path = os.path.join(os.path.dirname(_lib.LIB_PATH), 'gemm_up2.resources.txt')
    assert os.path.exists(path), 'built by dust3r_amd/build.py'
    report = open(path).read()
    assert len(re.findall(r'Function Name: \S*conv_up2_kernel', report)) == 2      # the head-tail and the typed-store instance
    assert re.findall(r'ScratchSize \[bytes/lane\]: (\d+)', report) == ['0', '0']
    assert re.findall(r'VGPRs Spill: (\d+)', report) == ['0', '0'] and re.findall(r'SGPRs Spill: (\d+)', report) == ['0', '0']
    assert re.findall(r'Occupancy \[waves/SIMD\]: (\d+)', report) == ['2', '2']
