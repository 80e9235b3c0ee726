"""The engine's split of a q | k | v projection (csrc/engine.hip gemm_heads): where the plan puts the q | k prefix on the persistent GEMM, q | k go there and V goes
out as a [vt] launch of its own -- and every output of the forward stays what the single launch gives, bit for bit.

One forward of two 512 x 384 pairs, D3R_GEMM_PERSIST=1 (every eligible launch on the persistent kernel: both the encoder's and the decoder's projections split) against
=0 (no launch splits), on one model. The configuration is the smallest the persistent kernel takes: it needs >= 18 K steps of 32, so the widths are 768 (encoder, 12
heads) and 640 (decoder, 10 heads), one block each, linear head. D3R_LN_INLINE_ROWS=0 at creation: calls this small otherwise form the LayerNorm statistics in the
consumer's prologue, which that kernel declines."""
import pytest
import torch

pytestmark = pytest.mark.gpu

CFG = dict(pos_embed='RoPE100', img_size=(512, 512), head_type='linear', enc_embed_dim=768, enc_depth=1, enc_num_heads=12, dec_embed_dim=640, dec_depth=1, dec_num_heads=10)


def test_split_projection_leaves_the_forward_bit_identical(gpu, monkeypatch):
    from dust3r_amd import ops
    from dust3r_amd.model import AsymmetricCroCo3DStereo
    from dust3r_amd.synthetic import synthetic_state_dict, synthetic_views
    for name in ('D3R_GEMM_NOWIDE', 'D3R_GEMM_CFG', 'D3R_GEMM_T128W8', 'D3R_GRAPH_MAX_PAIRS'):
        monkeypatch.delenv(name, raising=False)
    monkeypatch.setenv('D3R_LN_INLINE_ROWS', '0')
    model = AsymmetricCroCo3DStereo(precision=None, landscape_only=False, **CFG)
    model.load_state_dict(synthetic_state_dict({k: torch.empty(v, device='meta') for k, v in model._spec.items()}, 7, 1.0, device=gpu))
    model.to(gpu)
    assert model.precision == 'fp16x3'
    v1, v2 = synthetic_views(2, 384, 512, seed=3, device=gpu)
    ntok, tw = 24 * 32, 32
    outs = {}
    for mode in ('1', '0'):
        monkeypatch.setenv('D3R_GEMM_PERSIST', mode)
        # the q | k prefix of the encoder's launch (4 images) and of one decoder side's (2 images), as gemm_heads asks the plan
        enc = ops.heads_tile_config(4 * ntok, 768, ['rope', 'rope'], 768, ntok, tw, ntok, 'fp16x3')
        dec = ops.heads_tile_config(2 * ntok, 640, ['rope', 'rope'], 640, ntok, tw, ntok, 'fp16x3')
        assert (enc == 10) == (dec == 10) == (mode == '1'), (mode, enc, dec)
        with torch.no_grad():
            r1, r2 = model(v1, v2)
        torch.cuda.synchronize()
        outs[mode] = [r1['pts3d'].clone(), r1['conf'].clone(), r2['pts3d_in_other_view'].clone(), r2['conf'].clone()]
    for a, b in zip(outs['1'], outs['0']):
        assert int(a.view(torch.int32).unique().numel()) > 1000      # a computed map, not a constant
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
