"""Sky segmentation without a device: the numpy / SciPy restatement of the reference's `segment_sky` (dust3r/viz.py:345-381) that the
GPU tests (test_sky_gpu.py) hold the kernels to, its HSV stage on anchor colours (and against OpenCV where cv2 is importable), the
scene's `__deepcopy__` (the first step of `mask_sky`) and `mask_sky` off the GPU."""
import copy

import numpy as np
import pytest
import torch

from dust3r_amd.synthetic import GROUND_RGB, SKY_RGB, outdoor_scene, sky_mask_picture, synthetic_scene


# ------------------------------------------------------------------ the restatement (numpy + SciPy; OpenCV is not needed)
def _cv_round_table(num, den_scale):
    """OpenCV's sdiv_table / hdiv_table180: cvRound(num / (den_scale * i)), 0 at i = 0."""
    i = np.arange(1, 256, dtype=np.float64)
    return np.concatenate([[0], np.rint(num / (den_scale * i))]).astype(np.int64)


_SDIV = _cv_round_table(255 << 12, 1.0)
_HDIV180 = _cv_round_table(180 << 12, 6.0)


def restated_to_u8(image):
    """Step 1 of the reference: floating images become np.uint8(255 * image.clip(0, 1)) (a product in the image's own precision, truncated)."""
    a = np.asarray(image)
    return np.uint8(255 * a.clip(min=0, max=1)) if np.issubdtype(a.dtype, np.floating) else a


def restated_hsv(rgb_u8):
    """Restatement of OpenCV's 8-bit cvtColor(image, COLOR_BGR2HSV) (RGB2HSV_b: hsv_shift = 12, H in [0, 180)) applied, as the reference
    does, to RGB data: OpenCV's "b" is the image's R channel and its "r" the B channel. Returns int64 arrays H, S, V."""
    x = np.asarray(rgb_u8).astype(np.int64)
    b, g, r = x[..., 0], x[..., 1], x[..., 2]
    v = np.maximum(np.maximum(b, g), r)
    diff = v - np.minimum(np.minimum(b, g), r)
    s = (diff * _SDIV[v] + (1 << 11)) >> 12
    h = np.where(v == r, g - b, np.where(v == g, b - r + 2 * diff, r - g + 4 * diff))
    h = (h * _HDIV180[diff] + (1 << 11)) >> 12
    h = h + np.where(h < 0, 180, 0)
    return h, s, v


def restated_color_mask(image):
    """Steps 1-3: inRange(hsv, [0, 0, 100], [30, 255, 255]) or one of the three luminous-grey rules."""
    h, s, v = restated_hsv(restated_to_u8(image))
    return ((h <= 30) & (v >= 100)) | ((s < 10) & (v > 150)) | ((s < 30) & (v > 180)) | ((s < 50) & (v > 220))


def restated_segment_sky(image):
    """Restatement of the reference's segment_sky: colour mask, binary_opening with a 5x5 square, 8-connected components
    (scipy.ndimage.label with a 3x3 structure: the components of cv2.connectedComponentsWithStats(connectivity=8)), and every component
    of area a with 2 a > a_max kept. Returns a numpy bool (H, W) array."""
    from scipy import ndimage
    opened = ndimage.binary_opening(restated_color_mask(image), structure=np.ones((5, 5)))
    labels, n = ndimage.label(opened, structure=np.ones((3, 3)))
    if n == 0:
        return np.zeros(opened.shape, dtype=bool)
    areas = np.bincount(labels.ravel())[1:]
    return np.concatenate([[False], 2 * areas > areas.max()])[labels]


def test_restated_hsv_anchor_colours():
    # (R, G, B) of the picture -> (H, S, V) OpenCV reports for the same bytes read as BGR
    cases = {(0, 0, 255): (0, 255, 255),            # pure blue: OpenCV's "red"
             (0, 255, 0): (60, 255, 255),
             (255, 0, 0): (120, 255, 255),          # pure red: OpenCV's "blue"
             (0, 0, 0): (0, 0, 0), (128, 128, 128): (0, 0, 128), (255, 255, 255): (0, 0, 255),
             (135, 206, 235): (21, 109, 235), (90, 140, 210): (13, 146, 210)}
    for rgb, hsv in cases.items():
        got = tuple(c.item() for c in restated_hsv(np.array([[rgb]], np.uint8)))
        assert got == hsv, (rgb, got, hsv)


def test_restated_colour_rules():
    assert restated_color_mask(np.array([[SKY_RGB]], np.uint8)).all()
    assert not restated_color_mask(np.array([[GROUND_RGB]], np.uint8)).any()
    greys = np.array([[(g, g, g) for g in (99, 100, 150, 151, 255)]], np.uint8)
    assert restated_color_mask(greys).tolist() == [[False, True, True, True, True]]      # H = 0 passes at V >= 100
    # step 1 clips, multiplies in fp32 and truncates (c / 255 round-trips exactly for every byte c)
    u8 = restated_to_u8(np.float32([0.5 / 255, 254.9 / 255, 1.0, 1.7, -0.2]))
    assert u8.dtype == np.uint8 and u8.tolist() == [0, 254, 255, 255, 0]
    c = np.arange(256)
    assert (restated_to_u8(np.float32(c) / 255) == c).all()


def test_restated_segmentation_on_an_outdoor_scene():
    img = outdoor_scene(96, 128, seed=3)
    sky = restated_segment_sky(img)
    assert sky.shape == (96, 128) and sky.dtype == bool
    assert sky[:10].mean() > 0.5 and sky[-10:].mean() < 0.05
    # fp32 in [0, 1] input goes through the truncation of step 1
    assert restated_segment_sky(img.astype(np.float32) / 255).shape == sky.shape


def test_restated_area_rule():
    m = np.zeros((64, 96), bool)
    m[2:13, 2:20] = True                    # 11 x 18 = 198: a_max
    m[30:39, 2:13] = True                   # 9 x 11 = 99 = a_max / 2: dropped
    m[30:40, 40:50] = True                  # 10 x 10 = 100: kept
    sky = restated_segment_sky(sky_mask_picture(m))
    assert sky.sum() == 298 and sky[2:13, 2:20].all() and not sky[30:39, 2:13].any() and sky[30:40, 40:50].all()
    assert not restated_segment_sky(sky_mask_picture(np.zeros((20, 20), bool))).any()
    assert restated_segment_sky(sky_mask_picture(np.ones((20, 20), bool))).all()


def test_restated_hsv_matches_opencv_on_every_colour():
    cv2 = pytest.importorskip('cv2')
    c = np.arange(1 << 24, dtype=np.int64)
    img = np.stack([c >> 16, (c >> 8) & 255, c & 255], axis=-1).astype(np.uint8).reshape(4096, 4096, 3)
    hsv = cv2.cvtColor(img, cv2.COLOR_BGR2HSV)
    h, s, v = restated_hsv(img)
    assert (hsv[..., 0] == h).all() and (hsv[..., 1] == s).all() and (hsv[..., 2] == v).all()


# ------------------------------------------------------------------ the scene's deepcopy and mask_sky off the GPU
def _scene_with_images(mode):
    from dust3r_amd.cloud_opt import GlobalAlignerMode, global_aligner
    n = 2 if mode == 'PairViewer' else 3
    out, _, _ = synthetic_scene(n, 32, 48, seed=4, symmetrize=True)
    for view in ('view1', 'view2'):
        out[view]['img'] = torch.stack([torch.from_numpy(outdoor_scene(32, 48, seed=i)).permute(2, 0, 1).float() / 127.5 - 1
                                        for i in out[view]['idx']])
    return global_aligner(out, 'cpu', mode=getattr(GlobalAlignerMode, mode), verbose=False)


def _storages(scene):
    ptrs = set()
    for v in list(scene.__dict__.values()) + list(scene._parameters.values()) + list(scene._buffers.values()):
        for t in (v if isinstance(v, (list, tuple)) else [v]):
            if isinstance(t, torch.Tensor):
                ptrs.add(t.untyped_storage().data_ptr())
    ptrs.discard(0)
    return ptrs


@pytest.mark.parametrize('mode', ['PointCloudOptimizer', 'ModularPointCloudOptimizer', 'PairViewer'])
def test_deepcopy_copies_every_tensor_and_no_engine(mode):
    """copy.deepcopy, the first step of mask_sky. With no engine (a CPU scene) nn.Module's own deepcopy already works for PointCloudOptimizer
    and PairViewer, so only the Modular case (per-image parameters rebound to the copy's flat storage) needs __deepcopy__ here; the case it
    exists for, a live engine handle, is covered on the GPU (test_sky_gpu.py::test_mask_sky_on_each_scene_class)."""
    scene = _scene_with_images(mode)
    assert scene._engine is None and scene.imgs is not None
    res = copy.deepcopy(scene)
    assert type(res) is type(scene) and res is not scene and res._engine is None and res._engine_sig is None
    assert not (_storages(res) & _storages(scene))
    for a, b in zip(res.im_conf, scene.im_conf):
        assert torch.equal(a, b)
    # views of one storage stay views of one (new) storage
    assert len({c.untyped_storage().data_ptr() for c in res.im_conf}) == 1
    assert res.conf_i[res.str_edges[0]].data_ptr() == res._conf_i.data_ptr()
    for k, v in scene.state_dict().items():
        assert torch.equal(res.state_dict()[k], v), k
    if mode == 'ModularPointCloudOptimizer':
        for name in ('im_poses', 'im_depthmaps', 'im_focals', 'im_pp'):
            flat = getattr(res, '_flat_' + name)
            for k, p in enumerate(getattr(res, name)):
                assert p.untyped_storage().data_ptr() == flat.untyped_storage().data_ptr()
                assert p.requires_grad == getattr(scene, name)[k].requires_grad
        res.im_poses[1].data[0] = 0.25               # the copy's per-image parameters still write into its own flat storage
        assert float(res._flat_im_poses[1, 0]) == 0.25 and float(scene._flat_im_poses[1, 0]) != 0.25
    res.im_conf[0][0, 0] = -7.0
    assert float(scene.im_conf[0][0, 0]) != -7.0


def test_mask_sky_off_the_gpu_raises():
    from dust3r_amd._lib import D3RError
    scene = _scene_with_images('PointCloudOptimizer')
    with pytest.raises(D3RError):
        scene.mask_sky()


def test_mask_sky_without_images_raises():
    from dust3r_amd.cloud_opt import global_aligner
    out, _, _ = synthetic_scene(3, 32, 48, seed=4, symmetrize=True)
    scene = global_aligner(out, 'cpu', verbose=False)
    assert scene.imgs is None
    with pytest.raises(ValueError, match='imgs'):
        scene.mask_sky()


def test_segment_sky_resource_report_has_no_scratch():
    import os
    import re
    from dust3r_amd import _lib
    path = os.path.join(os.path.dirname(_lib.LIB_PATH), 'sky.resources.txt')
    assert os.path.exists(path), 'built by dust3r_amd/build.py'
    report = open(path).read()
    kernels = re.findall(r'Function Name: (\S+)', report)
    assert sum('sky' in k for k in kernels) == 6
    assert re.findall(r'ScratchSize \[bytes/lane\]: (\d+)', report) == ['0'] * len(kernels)
    assert {'d3r_segment_sky', 'd3r_segment_sky_workspace_bytes', 'd3r_sky_color_mask'} <= set(_lib.EXPORTED)
    assert _lib.lib.d3r_segment_sky_workspace_bytes(2, 1000) >= 2 * 2 * 1000 * 4
