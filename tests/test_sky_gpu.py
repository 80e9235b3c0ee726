"""Sky segmentation on the GPU (csrc/sky.hip): the colour stage over every RGB colour, the full segmentation against the numpy / SciPy
restatement of the reference's `segment_sky` (test_sky_cpu.py) on pictures and on masks built to stress the tiled connected components,
`mask_sky()` on each scene class, and the demo body followed by `mask_sky` (dust3r/demo.py:110-132). Every comparison is exact."""
import gc
import math
import os

import numpy as np
import pytest
import torch

from dust3r_amd.synthetic import outdoor_scene, sky_mask_picture
from test_sky_cpu import restated_color_mask, restated_segment_sky

pytestmark = pytest.mark.gpu


def _all_colours():
    c = np.arange(1 << 24, dtype=np.int64)
    return np.stack([c >> 16, (c >> 8) & 255, c & 255], axis=-1).astype(np.uint8).reshape(4096, 4096, 3)


def _color_mask_gpu(image, dev):
    from dust3r_amd._lib import check, current_stream, lib, ptr
    H, W = image.shape[:2]
    t = torch.from_numpy(np.ascontiguousarray(image)).to(dev)
    hw = torch.tensor([H], dtype=torch.int32, device=dev), torch.tensor([W], dtype=torch.int32, device=dev)
    out = torch.empty((1, H * W), dtype=torch.uint8, device=dev)
    check(lib.d3r_sky_color_mask(1, ptr(t), int(image.dtype == np.uint8), ptr(hw[0]), ptr(hw[1]), H * W, ptr(out), current_stream()), 'sky_color_mask')
    return out.view(H, W).cpu().numpy().astype(bool)


def test_colour_stage_on_every_colour(gpu):
    img = _all_colours()
    want = restated_color_mask(img)
    assert 0 < want.sum() < want.size
    assert np.array_equal(_color_mask_gpu(img, gpu), want)
    f = img.astype(np.float32) / 255                          # the scene's images: fp32 c / 255
    assert np.array_equal(_color_mask_gpu(f, gpu), restated_color_mask(f))
    del f
    # off the 1/255 grid and outside [0, 1]: clip, fp32 product and truncation of step 1
    g = np.random.RandomState(0).uniform(-0.1, 1.1, (1024, 1024, 3)).astype(np.float32)
    assert np.array_equal(_color_mask_gpu(g, gpu), restated_color_mask(g))


def _check_batch(images, dev):
    from dust3r_amd.viz import segment_sky_batch
    got = segment_sky_batch(images, dev)
    for k, (img, m) in enumerate(zip(images, got)):
        want = restated_segment_sky(img)
        assert m.dtype == torch.bool and tuple(m.shape) == want.shape
        m = m.cpu().numpy()
        assert np.array_equal(m, want), f'image {k} {want.shape}: {int((m != want).sum())} pixels differ'
    return got


SHAPES = [(384, 512), (512, 384), (288, 512), (224, 224)]


@pytest.mark.parametrize('H,W', SHAPES)
def test_outdoor_scenes(gpu, H, W):
    imgs = [outdoor_scene(H, W, seed=s, horizon=h) for s, h in ((1, 0.3), (2, 0.5), (3, 0.7))]
    got = _check_batch(imgs, gpu)
    assert all(m.any() for m in got)
    _check_batch([im.astype(np.float32) / 255 for im in imgs], gpu)            # the fp32 [0, 1] layout of scene.imgs


def test_ragged_batch(gpu):
    imgs = [outdoor_scene(H, W, seed=10 + k) for k, (H, W) in enumerate(SHAPES + SHAPES[::-1])]
    _check_batch(imgs, gpu)


def _spiral(H, W, width=5):
    """A single width-`width` rectangular spiral path with `width`-pixel gaps, from the border to the centre."""
    m = np.zeros((H, W), bool)
    top, left, bottom, right = 0, 0, H, W
    while bottom - top > 2 * width and right - left > 2 * width:
        m[top:top + width, left:right] = True                                   # top edge, left to right
        m[top:bottom, right - width:right] = True                               # right edge, down
        m[bottom - width:bottom, left:right] = True                             # bottom edge, right to left
        m[top + 2 * width:bottom, left:left + width] = True                     # left edge, up to a gap below the next turn
        m[top + 2 * width:top + 3 * width, left:left + 3 * width] = True        # step in to the next ring
        top, left, bottom, right = top + 2 * width, left + 2 * width, bottom - 2 * width, right - 2 * width
    return m


def test_spirals_and_combs(gpu):
    sp = _spiral(384, 512)
    comb = np.zeros((384, 512), bool)
    comb[0:5, :] = True
    for x in range(0, 512, 10):
        comb[:, x:x + 5] = True                                                 # teeth hanging from one bar, across 12 tile rows
    comb2 = np.zeros((384, 512), bool)
    for x in range(3, 505, 10):
        comb2[(x // 10) % 7 * 5:384 - 3, x:x + 5] = True                      # teeth of different lengths...
    comb2[380:384, :] = False
    comb2[372:377, 3:505] = True                                               # ...joined by a bar at the bottom
    comb2[100:105, 200:300] = True                                             # and a separate bar
    got = _check_batch([sky_mask_picture(sp), sky_mask_picture(comb), sky_mask_picture(comb2), sky_mask_picture(sp.T.copy())], gpu)
    assert got[0].sum() == restated_segment_sky(sky_mask_picture(sp)).sum() > 10000


def test_many_images_in_one_call(gpu):
    """48 images of tall combs and spirals at once: thousands of workgroups link, chase and flatten concurrently, and every mask stays
    exact (the roots a pixel ends on must not depend on which thread stores last)."""
    sp = _spiral(384, 512)
    comb = np.zeros((384, 512), bool)
    comb[379:384, :] = True
    for x in range(0, 512, 10):
        comb[:, x:x + 5] = True
    pics = [sky_mask_picture(m) for m in (sp, comb, sp[::-1].copy(), comb[:, ::-1].copy())]
    want = [restated_segment_sky(p) for p in pics]
    from dust3r_amd.viz import segment_sky_batch
    got = segment_sky_batch([pics[k % 4] for k in range(48)], gpu)
    for k, m in enumerate(got):
        assert np.array_equal(m.cpu().numpy(), want[k % 4]), k


def test_tile_corners_diagonals_and_borders(gpu):
    m = np.zeros((200, 260), bool)
    for ty in (32, 64, 96, 128):                  # 6 x 6 squares meeting only diagonally, exactly at a tile corner (32-pixel tiles)
        for tx in (32, 96, 160, 224):
            m[ty - 6:ty, tx - 6:tx] = True
            m[ty:ty + 6, tx:tx + 6] = True
    m[150:160, 60:70] = m[160:170, 50:60] = True   # 10 x 10 squares joined diagonally, away from tile edges
    m[0:10, 0:40] = True                            # touching the top-left corner
    m[190:200, 200:260] = True                      # bottom-right corner
    m[60:140, 0:5] = True                           # a width-5 bar on the left border
    m[60:140, 255:260] = True                       # and on the right border
    m[180:200, 100:106] = True                      # bottom border
    n = np.zeros((64, 64), bool)
    n[27:37, 27:37] = True                          # one blob straddling the four tiles of an image
    _check_batch([sky_mask_picture(m), sky_mask_picture(n), sky_mask_picture(m[::-1, ::-1].copy())], gpu)


def test_area_threshold_and_empty_or_full(gpu):
    m = np.zeros((96, 160), bool)
    m[2:13, 2:20] = True                    # 11 x 18 = 198 = a_max
    m[30:39, 2:13] = True                   # 99 = a_max / 2: dropped
    m[30:40, 40:50] = True                  # 100 = a_max / 2 + 1: kept
    m[60:70, 27:37] = True                  # another 100, straddling a tile edge
    empty, full = np.zeros((70, 90), bool), np.ones((70, 90), bool)
    got = _check_batch([sky_mask_picture(m), sky_mask_picture(empty), sky_mask_picture(full)], gpu)
    assert int(got[0].sum()) == 398 and not got[1].any() and got[2].all()


def test_segment_sky_api(gpu):
    from dust3r_amd.viz import segment_sky
    img = outdoor_scene(96, 128, seed=5)
    for x in (img, torch.from_numpy(img), img.astype(np.float32) / 255, torch.from_numpy(img.astype(np.float32) / 255).to(gpu)):
        m = segment_sky(x)
        assert m.dtype == torch.bool and m.device.type == 'cpu' and np.array_equal(m.numpy(), restated_segment_sky(np.asarray(x.cpu() if isinstance(x, torch.Tensor) else x)))


# ------------------------------------------------------------------ mask_sky on the scene classes
def _write_outdoor(tmp_path, sizes, horizons):
    import PIL.Image
    paths = []
    for k, ((W, H), h) in enumerate(zip(sizes, horizons)):
        p = os.path.join(str(tmp_path), f'view{k}.png')
        PIL.Image.fromarray(outdoor_scene(H, W, seed=40 + k, horizon=h)).save(p)
        paths.append(p)
    return paths


def _bits(t):
    return t.detach().contiguous().view(torch.int32).clone()


def _params(scene):
    return {k: _bits(v) for k, v in scene.state_dict().items() if not k.startswith('im_conf')}


def _check_mask_sky(scene, dev, run_after):
    from dust3r_amd.viz import segment_sky_batch
    before = [c.clone() for c in scene.im_conf]
    skies = segment_sky_batch(scene.imgs, dev)
    for img, sky in zip(scene.imgs, skies):
        assert np.array_equal(sky.cpu().numpy(), restated_segment_sky(img))
    assert any(s.any() for s in skies)
    res = scene.mask_sky()
    assert res is not scene and type(res) is type(scene) and res._engine is None
    for i, sky in enumerate(skies):
        assert torch.equal(scene.im_conf[i], before[i])
        assert (res.im_conf[i][sky] == 0).all() and torch.equal(res.im_conf[i][~sky], before[i][~sky])
    if not run_after:
        return res
    # both scenes go on independently, each with its own engine
    # (a random-weight network may give a nan loss, as in the reference: parameters are then compared only where they must not move)
    p_scene, p_res = _params(scene), _params(res)
    loss = scene.compute_global_alignment(init=None, niter=5, schedule='linear', lr=0.01)
    assert all(torch.equal(v, _params(res)[k]) for k, v in p_res.items())
    if math.isfinite(loss):
        assert any(not torch.equal(v, _params(scene)[k]) for k, v in p_scene.items())
    p_scene = _params(scene)
    loss = res.compute_global_alignment(init=None, niter=5, schedule='linear', lr=0.01)
    assert res._engine is not None and res._engine.value != scene._engine.value
    assert all(torch.equal(v, _params(scene)[k]) for k, v in p_scene.items())
    if math.isfinite(loss):
        assert any(not torch.equal(v, _params(res)[k]) for k, v in p_res.items())
    return res


@pytest.mark.parametrize('mode', ['PointCloudOptimizer', 'ModularPointCloudOptimizer', 'PairViewer'])
def test_mask_sky_on_each_scene_class(gpu, tmp_path, mode):
    from test_demo_flow_gpu import _engine, reconstruct
    from dust3r_amd.cloud_opt import GlobalAlignerMode, global_aligner
    n = 2 if mode == 'PairViewer' else 3
    files = _write_outdoor(tmp_path, [(200, 150)] * n, [0.3, 0.5, 0.6][:n])
    scene, _, out = reconstruct(files, _engine(gpu), gpu, image_size=96, schedule='linear', niter=10, min_conf_thr=3.0, clean_depth=False,
                                scenegraph_type='complete')
    if mode == 'ModularPointCloudOptimizer':
        scene = global_aligner(out['output'], device=gpu, mode=GlobalAlignerMode.ModularPointCloudOptimizer, verbose=False)
        scene.compute_global_alignment(init='mst', niter=10, schedule='linear', lr=0.01)
    assert type(scene).__name__ == mode
    if mode != 'PairViewer':
        assert scene._engine is not None
    res = _check_mask_sky(scene, gpu, run_after=mode != 'PairViewer')
    # the original goes away: the copy keeps working on its own storage and engine
    conf_res = [c.clone() for c in res.im_conf]
    del scene
    gc.collect()
    torch.cuda.synchronize()
    if mode != 'PairViewer':
        res.compute_global_alignment(init=None, niter=5, schedule='linear', lr=0.01)
    assert all(torch.equal(a, b) for a, b in zip(res.im_conf, conf_res))
    assert res.get_pts3d()[0].shape[-1] == 3 and len(res.get_masks()) == n


def test_demo_body_then_mask_sky(gpu, tmp_path):
    """dust3r/demo.py:110-132 with clean_depth and the "Mask sky" box ticked: clean_pointcloud, then mask_sky, then the getters."""
    from test_demo_flow_gpu import _engine, reconstruct
    from dust3r_amd.viz import segment_sky_batch
    files = _write_outdoor(tmp_path, [(200, 150)] * 3, [0.25, 0.45, 0.65])
    # min_conf_thr = 1 (the demo slider's low end): every pixel clean_pointcloud kept counts, so every kept sky pixel must be lost
    scene, _, out = reconstruct(files, _engine(gpu), gpu, image_size=96, schedule='linear', niter=20, min_conf_thr=1.0, clean_depth=True,
                                scenegraph_type='complete')
    masked = scene.mask_sky()
    skies = segment_sky_batch(scene.imgs, gpu)
    before, after = scene.get_masks(), masked.get_masks()
    for b, a, sky in zip(before, after, skies):
        assert not (a & ~b).any()
        assert torch.equal(b & ~a, b & sky)
    most = int(torch.stack([s.sum() for s in skies]).argmax())
    assert (before[most] & ~after[most]).sum() > 0
    assert len(masked.get_pts3d()) == 3 and masked.get_focals().shape == (3, 1) and masked.get_im_poses().shape == (3, 4, 4)
