"""Records tests/golden/demo_reference.pt from the reference's UNMODIFIED dust3r/demo.py (imported through oracle.ref_import; trimesh is the
oracle's inert shim, gradio a stub whose Slider records its keywords, matplotlib the real one). The module-level names load_images,
make_pairs, inference, global_aligner and get_3D_model_from_scene of the reference module are replaced by the recording stand-ins below
(`Recorder`), and the reference's own get_reconstructed_scene and set_scenegraph_options are called:
- 'scenes': small scenes of stored rgb / depth / confidence arrays and the depth / confidence pictures of the `imgs` the reference returned for
  them, with every confidence ratio c / cmax and the colour-table row matplotlib took for it;
- 'edge_ratios' / 'edge_indices': the same for a list of edge values of the index rule;
- 'calls': the calls and keyword arguments of each stage for 1, 2 and 4 pictures x complete / swin / oneref;
- 'scenegraph': the set_scenegraph_options table; 'jet': matplotlib's jet table and its "bad" colour; 'signatures'.
Only arrays, names and numbers are stored. tests/test_demo_cpu.py and tests/test_demo_gpu.py hold dust3r_amd/demo.py and csrc/gallery.hip
to these; they import `Recorder` from here (nothing at import time touches the reference).

    python tools/make_demo_golden.py"""
import enum
import inspect
import os
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

OUT = os.path.join(ROOT, 'tests', 'golden', 'demo_reference.pt')
STAGES = ('load_images', 'make_pairs', 'inference', 'global_aligner', 'get_3D_model_from_scene')

# the argument sets of the recorded runs: (number of pictures, model has square_ok, keyword values of get_reconstructed_scene after filelist)
CALL_CASES = [
    (n, square_ok, dict(schedule=schedule, niter=niter, min_conf_thr=thr, as_pointcloud=pc, mask_sky=sky, clean_depth=clean, transparent_cams=tc,
                        cam_size=cs, scenegraph_type=graph, winsize=win, refid=ref))
    for n, square_ok, schedule, niter, thr, pc, sky, clean, tc, cs, graph, win, ref in [
        (1, None, 'linear', 300, 3.0, False, False, True, False, 0.05, 'complete', 1, 0),
        (1, True, 'cosine', 10, 2.0, True, False, False, True, 0.03, 'swin', 1, 0),
        (1, False, 'linear', 5, 3.0, False, True, True, False, 0.05, 'oneref', 1, 0),
        (2, True, 'linear', 300, 3.0, False, False, True, False, 0.05, 'complete', 1, 0),
        (2, None, 'cosine', 20, 1.5, True, True, False, False, 0.01, 'swin', 1, 1),
        (2, False, 'linear', 7, 3.0, False, False, True, True, 0.1, 'oneref', 1, 1),
        (4, True, 'linear', 300, 3.0, False, False, True, False, 0.05, 'complete', 2, 0),
        (4, None, 'cosine', 50, 4.0, True, False, True, False, 0.02, 'swin', 2, 0),
        (4, False, 'linear', 0, 3.0, False, True, False, True, 0.05, 'oneref', 1, 3),
    ]
]


class Tag:
    """A named stand-in for what a stage returns (or for the model)."""

    def __init__(self, name, **attrs):
        self._name = name
        self.__dict__.update(attrs)


def describe(x):
    """A value as names and numbers only."""
    if isinstance(x, (Tag, FakeScene)):
        return x._name
    if isinstance(x, enum.Enum):
        return f'{type(x).__name__}.{x.name}'
    if isinstance(x, dict) and 'idx' in x and 'img' in x:
        return f'VIEW idx={x["idx"]} instance={x["instance"]}'
    if isinstance(x, (list, tuple)):
        return [describe(v) for v in x]
    if isinstance(x, (torch.device, np.floating, np.integer)):
        return str(x)
    assert x is None or isinstance(x, (str, int, float, bool)), type(x)
    return x


class FakeScene:
    """What global_aligner's stand-in returns: the getters the end of get_reconstructed_scene reads, over stored arrays."""
    _name = 'SCENE'

    def __init__(self, recorder, rgb, depth, conf):
        self._recorder = recorder
        self.imgs = [np.asarray(a) for a in rgb]
        self._depth = [torch.as_tensor(a) for a in depth]
        self.im_conf = [torch.as_tensor(a) for a in conf]

    def get_depthmaps(self):
        return list(self._depth)

    def compute_global_alignment(self, *args, **kwargs):
        self._recorder.record('scene.compute_global_alignment', args, kwargs)
        return 0.0


class Recorder:
    """Recording stand-ins for the five stages: `stubs()` maps each module-level name to one; `calls` lists (name, args, kwargs), described."""

    def __init__(self, n_files, rgb, depth, conf):
        self.calls = []
        self.n_files = n_files
        self.scene = FakeScene(self, rgb, depth, conf)

    def record(self, name, args, kwargs):
        self.calls.append((name, [describe(a) for a in args], {k: describe(v) for k, v in sorted(kwargs.items())}))

    def load_images(self, *args, **kwargs):
        self.record('load_images', args, kwargs)
        return [dict(img=torch.zeros(1, 3, 2, 2), true_shape=np.int32([[2, 2]]), idx=i, instance=str(i)) for i in range(self.n_files)]

    def make_pairs(self, *args, **kwargs):
        self.record('make_pairs', args, kwargs)
        return Tag('PAIRS')

    def inference(self, *args, **kwargs):
        self.record('inference', args, kwargs)
        return Tag('OUTPUT')

    def global_aligner(self, *args, **kwargs):
        self.record('global_aligner', args, kwargs)
        return self.scene

    def get_3D_model_from_scene(self, *args, **kwargs):
        self.record('get_3D_model_from_scene', args, kwargs)
        return os.path.join(args[0], 'scene.glb')

    def stubs(self):
        return {name: getattr(self, name) for name in STAGES}


def fake_model(square_ok):
    """square_ok None: a model without the attribute (the probe of get_reconstructed_scene falls back to False)."""
    return Tag('MODEL', patch_size=16) if square_ok is None else Tag('MODEL', patch_size=16, square_ok=square_ok)


def small_arrays(rng, shapes):
    rgb = [rng.random((h, w, 3)).astype(np.float32) for h, w in shapes]
    depth = [np.exp(rng.normal(size=(h, w)) / 2).astype(np.float32) for h, w in shapes]
    conf = [(1 + np.exp(rng.normal(size=(h, w)))).astype(np.float32) for h, w in shapes]
    return rgb, depth, conf


def gallery_scenes():
    """name -> (rgb, depth, conf) lists of arrays."""
    rng = np.random.default_rng(11)
    scenes = {}
    # ragged sizes; the maximum 16 sits in several pixels, zeros as clean_pointcloud / mask_sky leave them, every ratio k / 256 and its lower neighbour
    rgb, depth, conf = small_arrays(rng, [(16, 32), (32, 16), (8, 8)])
    conf = [np.minimum(c, np.float32(15.5)) for c in conf]
    conf[0][3, 5] = conf[0][15, 31] = conf[2][0, 0] = 16.0
    conf[0][8:12, 4:20] = 0
    conf[2][6:, :] = 0
    k = np.arange(257, dtype=np.float32) / 16                       # (k / 16) / 16 = k / 256 exactly
    flat = conf[1].reshape(-1)
    flat[:257] = k
    flat[257:512] = np.nextafter(k[1:256], np.float32(0))
    depth[1][31, 15] = depth[1].max() * 3                              # the depth maximum in the last pixel of an image
    scenes['ragged'] = (rgb, depth, conf)
    # pixel counts that are no multiple of 4 (no height of 3: rgb() takes a 3 x W x 4 colour picture for channels-first and transposes it)
    scenes['odd'] = small_arrays(rng, [(5, 7), (5, 5), (2, 3)])
    scenes['one_pixel'] = small_arrays(rng, [(1, 1)])
    rgb, depth, conf = small_arrays(rng, [(4, 6), (6, 4)])
    scenes['zero_conf'] = (rgb, depth, [np.zeros_like(c) for c in conf])              # 0 / 0: the bad colour everywhere
    rgb, depth, conf = small_arrays(rng, [(6, 8), (8, 6)])
    depth[0][2, 3] = np.nan      # in the FIRST image: python's max() over the per-image maxima keeps a NaN only from there
    scenes['nan_depth'] = (rgb, depth, conf)
    return scenes


EDGE_RATIOS = np.concatenate([
    np.float32([0.0, -0.0, 1.0, np.nextafter(np.float32(1), np.float32(0)), np.nan, -1e-3, np.inf, -np.inf, 1e-45, -1e-45, 1.5, np.nextafter(np.float32(1), np.float32(2))]),
    np.arange(257, dtype=np.float32) / 256, np.nextafter(np.arange(1, 257, dtype=np.float32) / 256, np.float32(0))]).astype(np.float32)


def _stub_module(name, **attrs):
    mod = types.ModuleType(name)
    for k, v in attrs.items():
        setattr(mod, k, v)
    sys.modules[name] = mod


class _Slider:
    def __init__(self, **kwargs):
        self.kwargs = kwargs


def main():
    import warnings
    from oracle.ref_import import REFERENCE_ROOT, import_reference
    import_reference()
    _stub_module('gradio', Slider=_Slider)
    import matplotlib
    import matplotlib.colors
    import dust3r.demo as D
    assert os.path.realpath(D.__file__).startswith(os.path.realpath(REFERENCE_ROOT))
    cmap = matplotlib.colormaps['jet']
    jet = cmap(np.arange(256))
    # jet repeats a colour (blue between 0.11 and 0.125), so a returned colour does not name its row: the row comes from a colour map whose
    # k-th colour carries k in its red channel, through the same Colormap.__call__ (same defaults for under / over / bad as jet)
    ramp = matplotlib.colors.ListedColormap([(k / 255, 0.0, 0.0) for k in range(256)])

    def indices(ratios):
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            out = ramp(np.asarray(ratios, dtype=np.float32).reshape(-1))
        return np.where(out[:, 3] == 0, 256, np.rint(out[:, 0] * 255)).astype(np.int32)

    def reference_run(n_files, square_ok, kwargs, arrays):
        rec = Recorder(n_files, *arrays)
        for name, fn in rec.stubs().items():
            setattr(D, name, fn)
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            scene, outfile, imgs = D.get_reconstructed_scene('OUT', fake_model(square_ok), 'cpu', True, 512, [f'im{i}.png' for i in range(n_files)], **kwargs)
        assert scene is rec.scene and outfile == os.path.join('OUT', 'scene.glb')
        return rec, imgs

    scenes = {}
    for name, arrays in gallery_scenes().items():
        rgb, depth, conf = arrays
        rec, imgs = reference_run(max(2, len(rgb)), True, CALL_CASES[3][2], arrays)
        assert len(imgs) == 3 * len(rgb) and all(imgs[3 * i] is rec.scene.imgs[i] for i in range(len(rgb)))
        out_depth, out_conf = [imgs[3 * i + 1] for i in range(len(rgb))], [imgs[3 * i + 2] for i in range(len(rgb))]
        assert all(d.dtype == np.float32 for d in out_depth) and all(c.dtype == np.float64 and c.shape[2] == 4 for c in out_conf)
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            cmax = max([c.max() for c in conf])
            ratios = [c / cmax for c in conf]
            dmax = max([d.max() for d in depth])
        scenes[name] = dict(rgb=[torch.from_numpy(a) for a in rgb], depth=[torch.from_numpy(a) for a in depth], conf=[torch.from_numpy(a) for a in conf],
                            out_depth=[torch.from_numpy(a) for a in out_depth], out_conf=[torch.from_numpy(a) for a in out_conf],
                            ratios=[torch.from_numpy(np.float32(r)) for r in ratios], indices=[torch.from_numpy(indices(r).reshape(r.shape)) for r in ratios],
                            maxima=torch.tensor([dmax, cmax], dtype=torch.float32))

    calls = []
    arrays = small_arrays(np.random.default_rng(5), [(4, 4), (4, 4)])
    for n_files, square_ok, kwargs in CALL_CASES:
        rec, _ = reference_run(n_files, square_ok, kwargs, arrays)
        calls.append(dict(n_files=n_files, square_ok=square_ok, kwargs=kwargs, calls=rec.calls))

    scenegraph = []
    for num_files in (None, 1, 2, 3, 10):
        for graph in ('complete', 'swin', 'oneref'):
            inputfiles = None if num_files is None else [f'im{i}.png' for i in range(num_files)]
            win, ref = D.set_scenegraph_options(inputfiles, 5, 3, graph)
            scenegraph.append(dict(num_files=num_files, scenegraph_type=graph,
                                   winsize=tuple(win.kwargs[k] for k in ('value', 'minimum', 'maximum', 'visible')),
                                   refid=tuple(ref.kwargs[k] for k in ('value', 'minimum', 'maximum', 'visible'))))

    rec = dict(scenes=scenes, edge_ratios=torch.from_numpy(EDGE_RATIOS), edge_indices=torch.from_numpy(indices(EDGE_RATIOS)), calls=calls,
               scenegraph=scenegraph, jet=torch.from_numpy(jet), jet_bad=torch.from_numpy(np.asarray(cmap(np.nan))),
               matplotlib_version=matplotlib.__version__,
               signatures={'get_reconstructed_scene': str(inspect.signature(D.get_reconstructed_scene))})
    torch.save(rec, OUT)
    print(OUT, os.path.getsize(OUT), 'bytes', rec['signatures'], 'matplotlib', matplotlib.__version__)


if __name__ == '__main__':
    main()
