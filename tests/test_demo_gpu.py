"""The demo's entry point on the GPU: the gallery kernels (csrc/gallery.hip, C ABI d3r_scene_gallery) against what the reference's own
get_reconstructed_scene returned for the recorded scenes (tests/golden/demo_reference.pt, tools/make_demo_golden.py), a case large enough
for a second grid-stride trip, the error returns, `get_reconstructed_scene` end to end on files, and the command line as a child process.

Equality is exact everywhere. "Bit-equal" below: NaNs sit in the same places (a NaN's sign and payload differ between processors and are
not compared) and every other value has the same 32 bits, so -0.0 is told from 0.0."""
import argparse
import ctypes as C
import functools
import json
import os
import struct
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'demo_reference.pt')
SENTINEL = -7.0


@functools.lru_cache(None)
def golden():
    return torch.load(GOLDEN, weights_only=False)


def table():
    """the reference's colour table from the record alone: float32(lut * 0.5 + 0.5), the bad row last"""
    g = golden()
    return np.float32(np.concatenate([g['jet'].numpy(), g['jet_bad'].numpy()[None]]) * 0.5 + 0.5)


def bit_equal(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    nan = np.isnan(a)
    return a.shape == b.shape and np.array_equal(nan, np.isnan(b)) and np.array_equal(a.view(np.uint32)[~nan], b.view(np.uint32)[~nan])


# ---- numpy restatement of the end of get_reconstructed_scene (pinned to the record by test_restatement_equals_the_record) --------------------
def restated_index(r):
    r = np.asarray(r, dtype=np.float32)
    with np.errstate(invalid='ignore', over='ignore'):
        x = r * np.float32(256)
        idx = np.where(x >= 256, 255, np.where(x < 0, 0, np.nan_to_num(x, nan=0.0, posinf=0.0, neginf=0.0).astype(np.int64)))
    return np.where(np.isnan(r), 256, idx)


def restated_gallery(depths, confs):
    """(depth pictures, confidence pictures, (dmax, cmax)) of float32 maps; the maxima propagate NaN like numpy.max"""
    depths, confs = [np.asarray(d, dtype=np.float32) for d in depths], [np.asarray(c, dtype=np.float32) for c in confs]
    dmax, cmax = np.max(np.concatenate([d.reshape(-1) for d in depths])), np.max(np.concatenate([c.reshape(-1) for c in confs]))
    tab = table()
    with np.errstate(invalid='ignore', divide='ignore', over='ignore'):
        out_d = [((d / dmax) * np.float32(0.5) + np.float32(0.5)).clip(min=0, max=1) for d in depths]
        out_c = [tab[restated_index(c / cmax)] for c in confs]
    return out_d, out_c, (dmax, cmax)


# ---- the C call on tensors the test allocates ---------------------------------------------------------------------------------------------
def run_gallery(gpu, depths, confs, tab=None):
    """d3r_scene_gallery on padded rows with NaN / 1e30 poison behind every valid length (the longest image included) and a sentinel in every
    output. Returns per image the depth picture and the confidence picture, and the two maxima; asserts the padding of the outputs was not
    written and the inputs were not changed."""
    from dust3r_amd._lib import check, current_stream, lib, ptr
    n = len(depths)
    areas = [int(np.asarray(d).size) for d in depths]
    row = -(-max(areas) // 4) * 4 + 4
    poison = np.where(np.arange(row) % 2 == 0, np.float32(np.nan), np.float32(1e30)).astype(np.float32)
    d_host, c_host = np.tile(poison, (n, 1)), np.tile(poison[::-1].copy(), (n, 1))
    for i, (d, c) in enumerate(zip(depths, confs)):
        d_host[i, :areas[i]] = np.asarray(d, dtype=np.float32).reshape(-1)
        c_host[i, :areas[i]] = np.asarray(c, dtype=np.float32).reshape(-1)
    d_dev, c_dev = torch.from_numpy(d_host).to(gpu), torch.from_numpy(c_host).to(gpu)
    npix = torch.tensor(areas, dtype=torch.int32).to(gpu)
    tab_dev = torch.from_numpy(table() if tab is None else tab).to(gpu)
    out_d = torch.full((n, row), SENTINEL, dtype=torch.float32, device=gpu)
    out_c = torch.full((n, row, 4), SENTINEL, dtype=torch.float32, device=gpu)
    maxima = torch.full((2,), SENTINEL, dtype=torch.float32, device=gpu)
    work = torch.empty(int(lib.d3r_scene_gallery_workspace_bytes(n, row)), dtype=torch.uint8, device=gpu)
    check(lib.d3r_scene_gallery(n, ptr(d_dev), ptr(c_dev), ptr(npix), row, ptr(tab_dev), ptr(out_d), ptr(out_c), ptr(maxima), ptr(work), current_stream()),
          'scene_gallery')
    torch.cuda.synchronize()
    od, oc = out_d.cpu().numpy(), out_c.cpu().numpy()
    assert bit_equal(d_dev.cpu().numpy(), d_host) and bit_equal(c_dev.cpu().numpy(), c_host)
    for i, a in enumerate(areas):
        assert (od[i, a:] == SENTINEL).all() and (oc[i, a:] == SENTINEL).all(), f'image {i}: written behind its {a} pixels'
    shapes = [np.asarray(d).shape for d in depths]
    return ([od[i, :a].reshape(s) for i, (a, s) in enumerate(zip(areas, shapes))], [oc[i, :a].reshape(s + (4,)) for i, (a, s) in enumerate(zip(areas, shapes))],
            maxima.cpu().numpy())


SCENES = ['ragged', 'odd', 'one_pixel', 'zero_conf', 'nan_depth']


@pytest.mark.parametrize('name', SCENES)
def test_restatement_equals_the_record(name):
    s = golden()['scenes'][name]
    out_d, out_c, maxima = restated_gallery([d.numpy() for d in s['depth']], [c.numpy() for c in s['conf']])
    assert bit_equal(np.float32(maxima), s['maxima'].numpy())
    for i in range(len(out_d)):
        assert bit_equal(out_d[i], s['out_depth'][i].numpy()) and bit_equal(out_c[i], np.float32(s['out_conf'][i].numpy()))


@pytest.mark.parametrize('name', SCENES)
def test_gallery_kernels_equal_the_reference(gpu, name):
    s = golden()['scenes'][name]
    got_d, got_c, maxima = run_gallery(gpu, [d.numpy() for d in s['depth']], [c.numpy() for c in s['conf']])
    assert bit_equal(maxima, s['maxima'].numpy()), (maxima, s['maxima'])
    for i in range(len(got_d)):
        want_d, want_c = s['out_depth'][i].numpy(), np.float32(s['out_conf'][i].numpy())
        assert want_d.dtype == np.float32 and bit_equal(got_d[i], want_d), (name, i)
        assert bit_equal(got_c[i], want_c), (name, i)
    if name == 'nan_depth':
        assert np.isnan(maxima[0]) and all(np.isnan(d).all() for d in got_d) and not any(np.isnan(c).any() for c in got_c)
    if name == 'zero_conf':
        assert maxima[1] == 0 and all((c == 0.5).all() for c in got_c)


def launch_bound():
    from dust3r_amd._lib import lib
    b, t, v = C.c_int(), C.c_int(), C.c_int()
    lib.d3r_scene_gallery_launch_bound(C.byref(b), C.byref(t), C.byref(v))
    return b.value, t.value, v.value


@functools.lru_cache(None)
def big_case():
    """Three images whose rows together are longer than one trip of the capped grid (so the last image lies in the second trip, computed by
    the first workgroups again) with pixel counts that leave 0, 3 and 1 pixels of a last group; drawn once for both placements."""
    blocks, threads, vec = launch_bound()
    per_trip = blocks * threads * vec
    area = (per_trip // 3 // 4) * 4 + 4096
    assert 3 * (area + 4) > per_trip and 3 * (area + 4) < 1000000
    rng = np.random.default_rng(3)
    areas = [area, area - 5, area - 3]
    depths = [np.exp(rng.normal(size=a)).astype(np.float32) for a in areas]
    confs = [(1 + np.exp(rng.normal(size=a))).astype(np.float32) for a in areas]
    return depths, confs


@pytest.mark.parametrize('where', ['last', 'first'])
def test_second_grid_stride_trip_and_many_partials(gpu, where):
    depths, confs = big_case()
    img, pix = (len(depths) - 1, depths[-1].size - 1) if where == 'last' else (0, 0)
    depths, confs = [d.copy() for d in depths], [c.copy() for c in confs]
    depths[img][pix], confs[img][pix] = 1000.0, 4096.0
    want_d, want_c, want_max = restated_gallery(depths, confs)
    assert want_max == (1000.0, 4096.0)
    got_d, got_c, maxima = run_gallery(gpu, depths, confs)
    assert maxima.tolist() == [1000.0, 4096.0]
    for i in range(len(depths)):
        assert bit_equal(got_d[i], want_d[i]) and bit_equal(got_c[i], want_c[i]), i
    assert got_d[img][pix] == 1.0 and got_c[img][pix].tolist() == table()[255].tolist()


def test_table_rows_are_looked_up_not_computed(gpu):
    """another table in, its rows out: the kernel holds no colour of its own"""
    s = golden()['scenes']['ragged']
    tab = np.arange(257 * 4, dtype=np.float32).reshape(257, 4)
    _, got_c, _ = run_gallery(gpu, [d.numpy() for d in s['depth']], [c.numpy() for c in s['conf']], tab=tab)
    for c, idx in zip(got_c, s['indices']):
        assert np.array_equal(c, tab[idx.numpy()])


def test_error_returns(gpu):
    from dust3r_amd._lib import current_stream, lib, ptr
    n, row = 2, 16
    f = lambda *shape: torch.zeros(shape, dtype=torch.float32, device=gpu)  # noqa: E731
    depth, conf, tab, out_d, out_c, maxima = f(n, row + 4), f(n, row + 4), f(257 * 4 + 4), f(n, row + 4), f(n, row + 4, 4), f(2)
    npix = torch.tensor([16, 12], dtype=torch.int32).to(gpu)
    work = torch.empty(max(1, int(lib.d3r_scene_gallery_workspace_bytes(n, row))), dtype=torch.uint8, device=gpu)
    good = dict(n=n, depth=ptr(depth), conf=ptr(conf), npix=ptr(npix), row=row, tab=ptr(tab), out_d=ptr(out_d), out_c=ptr(out_c), maxima=ptr(maxima), work=ptr(work))

    def call(**kw):
        a = dict(good, **kw)
        return lib.d3r_scene_gallery(a['n'], a['depth'], a['conf'], a['npix'], a['row'], a['tab'], a['out_d'], a['out_c'], a['maxima'], a['work'], current_stream())
    assert call() == 0
    for key in ('depth', 'conf', 'npix', 'tab', 'out_d', 'out_c', 'maxima', 'work'):
        assert call(**{key: None}) == -1, key
    for kw in (dict(n=0), dict(n=-1), dict(row=0), dict(row=-16), dict(row=6), dict(row=18)):
        assert call(**kw) == -1, kw
    off = lambda t: C.c_void_p(t.data_ptr() + 4)  # noqa: E731  (4 bytes past a 16-byte boundary, inside the tensor)
    for key, t in (('depth', depth), ('conf', conf), ('tab', tab), ('out_d', out_d), ('out_c', out_c)):
        assert call(**{key: off(t)}) == -1, key
    assert lib.d3r_scene_gallery_workspace_bytes(0, 16) == 0 and lib.d3r_scene_gallery_workspace_bytes(2, 6) == 0
    torch.cuda.synchronize()


# ---- end to end -----------------------------------------------------------------------------------------------------------------------
def _write_images(tmp_path, sizes):
    import PIL.Image
    from dust3r_amd.synthetic import synthetic_photo
    paths = []
    for k, (W, H) in enumerate(sizes):
        p = os.path.join(str(tmp_path), f'view{k}.png')
        PIL.Image.fromarray(synthetic_photo(W, H, seed=20 + k)).save(p)
        paths.append(p)
    return paths


@pytest.fixture(scope='module')
def engine(gpu):
    from dust3r_amd.model import AsymmetricCroCo3DStereo
    from dust3r_amd.synthetic import MODEL_CONFIGS
    from oracle.dust3r_ref import build_ref_model
    m = AsymmetricCroCo3DStereo(landscape_only=False, **MODEL_CONFIGS['tiny_dpt'])
    m.load_state_dict(build_ref_model('tiny_dpt').state_dict())
    return m.to(gpu)


def read_glb(path):
    data = open(path, 'rb').read()
    magic, version, length = struct.unpack('<4sII', data[:12])
    assert magic == b'glTF' and version == 2 and length == len(data)
    clen, ctype = struct.unpack('<I4s', data[12:20])
    assert ctype == b'JSON'
    return json.loads(data[20:20 + clen])


def check_gallery(scene, imgs, shapes):
    n = len(shapes)
    assert len(imgs) == 3 * n
    with torch.no_grad():
        depths = [d.detach().cpu().numpy() for d in scene.get_depthmaps()]
        confs = [c.detach().cpu().numpy() for c in scene.im_conf]
    want_d, want_c, _ = restated_gallery(depths, confs)
    for i, (h, w) in enumerate(shapes):
        rgb, d, c = imgs[3 * i:3 * i + 3]
        assert rgb is scene.imgs[i] and rgb.shape == (h, w, 3)
        assert isinstance(d, np.ndarray) and d.dtype == np.float32 and d.shape == (h, w)
        assert isinstance(c, np.ndarray) and c.dtype == np.float32 and c.shape == (h, w, 4)
        assert bit_equal(d, want_d[i]) and bit_equal(c, want_c[i]), i


@pytest.mark.parametrize('sizes,image_size,shapes,kind,kw', [
    ([(160, 160)], 128, [(96, 128)] * 2, 'PairViewer', dict(as_pointcloud=False, mask_sky=False, clean_depth=True, scenegraph_type='complete')),
    ([(200, 150), (150, 200)], 96, [(64, 96), (96, 64)], 'PairViewer', dict(as_pointcloud=True, mask_sky=True, clean_depth=False, scenegraph_type='swin')),
    ([(200, 150), (150, 200), (200, 150)], 96, [(64, 96), (96, 64), (64, 96)], 'PointCloudOptimizer',
     dict(as_pointcloud=False, mask_sky=False, clean_depth=True, scenegraph_type='oneref')),
])
def test_get_reconstructed_scene_on_files(gpu, engine, tmp_path, sizes, image_size, shapes, kind, kw):
    from dust3r_amd.demo import get_reconstructed_scene, scene_gallery
    files = _write_images(tmp_path, sizes)
    outdir = str(tmp_path / 'out')
    os.makedirs(outdir)
    scene, outfile, imgs = get_reconstructed_scene(outdir, engine, gpu, True, image_size, files, 'linear', 10, 3.0, kw['as_pointcloud'], kw['mask_sky'],
                                                   kw['clean_depth'], False, 0.05, kw['scenegraph_type'], 1, 0)
    assert type(scene).__name__ == kind and [tuple(s) for s in scene.imshapes] == shapes
    assert outfile == os.path.join(outdir, 'scene.glb') and os.path.isfile(outfile)
    doc = read_glb(outfile)
    assert doc['asset']['version'] == '2.0' and sum(n.get('name', '').startswith('camera_') and not n['name'].endswith('_image') for n in doc['nodes']) == len(shapes)
    check_gallery(scene, imgs, shapes)
    check_gallery(scene, scene_gallery(scene), shapes)          # the same pictures again, on its own


def test_scene_gallery_on_a_modular_scene_and_on_copied_maps(gpu):
    """ModularPointCloudOptimizer, and a scene that was assigned confidence maps of the caller's (`scene.im_conf = [...]`): the setter copies
    them into the scene's stack, which the gallery then reads like any other."""
    from dust3r_amd.cloud_opt import GlobalAlignerMode, global_aligner
    from dust3r_amd.demo import scene_gallery
    from dust3r_amd.synthetic import synthetic_scene
    out, _, _ = synthetic_scene(3, 32, 48, seed=1, scene_graph='complete', symmetrize=True, noise=0.002, device=gpu)
    for v in ('view1', 'view2'):
        out[v]['img'] = torch.rand((len(out[v]['idx']), 3, 32, 48)) * 2 - 1
    scene = global_aligner(out, device=gpu, mode=GlobalAlignerMode.ModularPointCloudOptimizer, verbose=False)
    scene.compute_global_alignment(init='mst', niter=5, schedule='linear', lr=0.01)
    check_gallery(scene, scene_gallery(scene), [(32, 48)] * 3)
    scene.im_conf = [c.clone() for c in scene.im_conf]
    scene.im_conf[1][4:9, 3:20] = 0
    check_gallery(scene, scene_gallery(scene), [(32, 48)] * 3)


def test_command_line_in_a_child_process(gpu, tmp_path):
    """python -m dust3r_amd.demo on a folder of two pictures and a tiny checkpoint file written here: scene.glb, the gallery and cameras.json
    (and two turntable frames). The weights are random, so the confidence threshold is the page's lowest: every pixel stays."""
    import PIL.Image
    from dust3r_amd.synthetic import MODEL_CONFIGS
    from oracle.dust3r_ref import build_ref_model
    cfg = MODEL_CONFIGS['tiny_dpt']
    state = {k: v for k, v in build_ref_model('tiny_dpt').state_dict().items() if not k.startswith('dec_blocks2')}
    model_str = ("AsymmetricCroCo3DStereo(pos_embed='RoPE100', patch_embed_cls='ManyAR_PatchEmbed', img_size=(64, 64), head_type='dpt', output_mode='pts3d', "
                 "depth_mode=('exp', -inf, inf), conf_mode=('exp', 1, inf), enc_embed_dim=%d, enc_depth=%d, enc_num_heads=%d, dec_embed_dim=%d, dec_depth=%d, dec_num_heads=%d)"
                 % (cfg['enc_embed_dim'], cfg['enc_depth'], cfg['enc_num_heads'], cfg['dec_embed_dim'], cfg['dec_depth'], cfg['dec_num_heads']))
    ckpt = str(tmp_path / 'tiny_dpt.pth')
    torch.save({'args': argparse.Namespace(model=model_str), 'model': state}, ckpt)
    pics = tmp_path / 'pics'
    pics.mkdir()
    _write_images(pics, [(200, 150), (150, 200)])
    out = tmp_path / 'out'
    r = subprocess.run([sys.executable, '-m', 'dust3r_amd.demo', str(pics), '--weights', ckpt, '--outdir', str(out), '--image_size', '224', '--niter', '5',
                        '--min_conf_thr', '1.0', '--scenegraph_type', 'swin', '--winsize', '9', '--silent', '--turntable', '2'], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert read_glb(str(out / 'scene.glb'))['asset']['version'] == '2.0'
    cams = json.loads((out / 'cameras.json').read_text())
    assert np.asarray(cams['cam2world']).shape == (2, 4, 4) and len(cams['focals']) == 2 and cams['image_sizes'] == [[224, 224], [224, 224]]      # size 224: load_images crops to a square
    for k, (w, h) in enumerate(cams['image_sizes']):
        for kind, mode in (('rgb', 'RGB'), ('depth', 'L'), ('conf', 'RGBA')):
            im = PIL.Image.open(out / 'gallery' / f'view{k}_{kind}.png')
            assert im.size == (w, h) and im.mode == mode, (k, kind, im.size, im.mode)
    assert sorted(os.listdir(out / 'turntable')) == ['turntable_000.png', 'turntable_001.png']
