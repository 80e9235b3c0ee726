"""The demo's entry point (dust3r_amd/demo.py: get_reconstructed_scene, scenegraph_options, the command line, the gallery's table and index
rule) without a GPU, pinned to what the reference's own dust3r/demo.py and matplotlib recorded (tests/golden/demo_reference.pt,
tools/make_demo_golden.py). tests/test_demo_gpu.py holds the gallery kernels and the end-to-end run to the same record."""
import ctypes as C
import inspect
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'demo_reference.pt')

from dust3r_amd import demo  # noqa: E402


@pytest.fixture(scope='module')
def golden():
    return torch.load(GOLDEN, weights_only=False)


def host_indices(ratios):
    from dust3r_amd import _lib
    r = np.ascontiguousarray(ratios, dtype=np.float32).reshape(-1)
    out = np.full(r.size, -1, dtype=np.int32)
    _lib.check(_lib.lib.d3r_selftest_gallery_index_host(r.ctypes.data_as(C.c_void_p), r.size, out.ctypes.data_as(C.c_void_p)), 'selftest_gallery_index_host')
    return out


def test_jet_table_is_matplotlibs(golden):
    jet = golden['jet'].numpy()
    assert jet.dtype == np.float64 and jet.shape == (256, 4)
    assert np.array_equal(demo.jet_lut(), jet)
    assert golden['jet_bad'].tolist() == [0.0, 0.0, 0.0, 0.0]


def test_gallery_table_carries_rgbs_affine_map(golden):
    lut = np.concatenate([golden['jet'].numpy(), golden['jet_bad'].numpy()[None]])
    table = demo.gallery_table()
    assert table.dtype == np.float32 and table.shape == (257, 4)
    assert np.array_equal(table, np.float32(lut * 0.5 + 0.5))
    assert table[demo.GALLERY_BAD_ROW].tolist() == [0.5, 0.5, 0.5, 0.5]


def test_table_reproduces_the_reference_colours(golden):
    """table[recorded row] is np.float32 of the confidence picture the reference returned, for every pixel of every scene"""
    table = demo.gallery_table()
    for name, s in golden['scenes'].items():
        for idx, out in zip(s['indices'], s['out_conf']):
            assert np.array_equal(table[idx.numpy()], np.float32(out.numpy())), name


def test_index_rule_on_the_recorded_ratios(golden):
    for name, s in golden['scenes'].items():
        for ratio, idx in zip(s['ratios'], s['indices']):
            assert np.array_equal(host_indices(ratio.numpy()), idx.numpy().reshape(-1)), name


def test_index_rule_on_the_edges(golden):
    ratios, idx = golden['edge_ratios'].numpy(), golden['edge_indices'].numpy()
    one, k = np.float32(1), np.arange(257, dtype=np.float32) / 256
    wanted = np.concatenate([np.float32([0.0, -0.0, 1.0, np.nextafter(one, np.float32(0)), np.nan, -1e-3, np.inf]), k, np.nextafter(k[1:], np.float32(0))])
    have = {v.tobytes() for v in ratios}
    assert all(v.tobytes() in have for v in wanted)           # the record holds every edge (bit patterns: -0.0 and NaN count)
    assert np.array_equal(host_indices(ratios), idx)
    at = lambda v: int(idx[[r.tobytes() == np.float32(v).tobytes() for r in ratios].index(True)])  # noqa: E731
    assert (at(0.0), at(-0.0), at(1.0), at(np.nextafter(one, np.float32(0))), at(np.nan), at(-1e-3), at(np.inf)) == (0, 0, 255, 255, 256, 0, 255)
    assert [at(v) for v in k[:256]] == list(range(256)) and [at(v) for v in np.nextafter(k[1:], np.float32(0))] == list(range(256))


def test_index_selftest_rejects_null():
    from dust3r_amd import _lib
    assert _lib.lib.d3r_selftest_gallery_index_host(None, 3, None) == -1
    assert _lib.lib.d3r_selftest_gallery_index_host(None, 0, None) == 0
    assert {'d3r_scene_gallery', 'd3r_scene_gallery_workspace_bytes', 'd3r_scene_gallery_launch_bound', 'd3r_selftest_gallery_index_host'} <= set(_lib.EXPORTED)


def test_workspace_query_and_launch_bound():
    from dust3r_amd import _lib
    b, t, v = C.c_int(), C.c_int(), C.c_int()
    _lib.lib.d3r_scene_gallery_launch_bound(C.byref(b), C.byref(t), C.byref(v))
    assert b.value > 1 and t.value % 64 == 0 and v.value == 4
    assert b.value * t.value * v.value < 1000000            # a second grid-stride trip is testable under a million pixels
    ws = _lib.lib.d3r_scene_gallery_workspace_bytes
    assert ws(1, 4) >= 8 and ws(100, 512 * 384) >= 2 * 4 * b.value
    assert ws(0, 4) == 0 and ws(1, 0) == 0 and ws(1, 6) == 0 and ws(-1, 4) == 0


def test_scenegraph_options_is_the_reference_rule(golden):
    assert len(golden['scenegraph']) == 15
    for row in golden['scenegraph']:
        for winsize, refid in ((5, 3), (None, None), (1, 0)):          # the incoming values do not enter
            got = demo.scenegraph_options(row['num_files'], winsize, refid, row['scenegraph_type'])
            assert got == (tuple(row['winsize']), tuple(row['refid'])), row


def test_signature_is_the_reference(golden):
    assert str(inspect.signature(demo.get_reconstructed_scene)) == golden['signatures']['get_reconstructed_scene']


def test_get_reconstructed_scene_issues_the_recorded_calls(golden, monkeypatch):
    """The stages, their order and their arguments, with the recording stand-ins of the fixture's maker patched into dust3r_amd.demo (the
    gallery, which needs the GPU, is replaced too: tests/test_demo_gpu.py covers it)."""
    from make_demo_golden import Recorder, fake_model, small_arrays
    assert sorted({(c['n_files'], c['kwargs']['scenegraph_type']) for c in golden['calls']}) == [(n, g) for n in (1, 2, 4) for g in ('complete', 'oneref', 'swin')]
    arrays = small_arrays(np.random.default_rng(5), [(4, 4), (4, 4)])
    for case in golden['calls']:
        rec = Recorder(case['n_files'], *arrays)
        for name, fn in rec.stubs().items():
            monkeypatch.setattr(demo, name, fn)
        monkeypatch.setattr(demo, 'scene_gallery', lambda scene: ['GALLERY', scene])
        scene, outfile, imgs = demo.get_reconstructed_scene('OUT', fake_model(case['square_ok']), 'cpu', True, 512, [f'im{i}.png' for i in range(case['n_files'])],
                                                            **case['kwargs'])
        assert scene is rec.scene and outfile == os.path.join('OUT', 'scene.glb') and imgs == ['GALLERY', rec.scene]
        assert rec.calls == case['calls'], case
        names = [c[0] for c in rec.calls]
        assert ('scene.compute_global_alignment' in names) == (case['n_files'] > 2)


def test_parser_has_the_ui_defaults():
    p = demo.get_args_parser()
    a = p.parse_args(['a.png', 'b.png', '--weights', 'w.pth'])
    assert (a.images, a.weights, a.model_name, a.outdir) == (['a.png', 'b.png'], 'w.pth', None, '.')
    assert (a.image_size, a.device, a.silent) == (512, 'cuda', False)
    assert (a.schedule, a.niter, a.min_conf_thr, a.cam_size, a.scenegraph_type) == ('linear', 300, 3.0, 0.05, 'complete')
    assert (a.as_pointcloud, a.mask_sky, a.clean_depth, a.transparent_cams, a.turntable) == (False, False, True, False, 0)
    assert (a.winsize, a.refid) == (None, None)
    a = p.parse_args(['dir', '--model_name', 'snap', '--image_size', '224', '--no-clean_depth', '--as_pointcloud', '--mask_sky', '--transparent_cams',
                      '--schedule', 'cosine', '--scenegraph_type', 'swin', '--winsize', '2', '--turntable', '8', '--silent'])
    assert (a.model_name, a.weights, a.image_size, a.clean_depth, a.as_pointcloud, a.mask_sky, a.transparent_cams) == ('snap', None, 224, False, True, True, True)
    assert (a.schedule, a.scenegraph_type, a.winsize, a.turntable, a.silent) == ('cosine', 'swin', 2, 8, True)
    for bad in (['a.png'], ['a.png', '--weights', 'w', '--model_name', 'm'], ['--weights', 'w'], ['a.png', '--weights', 'w', '--image_size', '300'],
                ['a.png', '--weights', 'w', '--server_port', '80'], ['a.png', '--weights', 'w', '--tmp_dir', 't']):
        with pytest.raises(SystemExit):
            p.parse_args(bad)


def test_winsize_and_refid_are_clamped():
    clamp = demo.clamp_scenegraph
    assert clamp(10, None, None, 'swin') == (5, 0)          # the controls' defaults: the largest window, reference 0
    assert clamp(10, 99, 99, 'swin') == (5, 9) and clamp(10, 0, -4, 'oneref') == (1, 0) and clamp(10, 3, 4, 'complete') == (3, 4)
    assert clamp(1, 7, 7, 'oneref') == (1, 0) and clamp(2, 2, 1, 'swin') == (1, 1) and clamp(4, 2, 3, 'swin') == (2, 3)


def test_input_files_expand_one_folder(tmp_path):
    for name in ('b.PNG', 'a.jpg', 'notes.txt'):
        (tmp_path / name).write_bytes(b'')
    assert demo._input_files([str(tmp_path)]) == [str(tmp_path / 'a.jpg'), str(tmp_path / 'b.PNG')]
    assert demo._input_files(['x.png', 'y.png']) == ['x.png', 'y.png']


def test_product_does_not_import_matplotlib():
    import subprocess
    r = subprocess.run([sys.executable, '-c', 'import sys; import dust3r_amd.demo; print(any(m.split(".")[0] in ("matplotlib", "gradio") for m in sys.modules))'],
                       capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 0 and r.stdout.strip() == 'False', r.stdout + r.stderr
