"""Records tests/golden/glb_reference.pt from the reference's UNMODIFIED dust3r/viz.py and dust3r/demo.py (imported through oracle.ref_import;
trimesh is the oracle's inert shim -- pts3d_to_trimesh and cat_meshes are pure numpy -- and gradio / matplotlib are stubbed here):
- `faces` and `face_colors` of cat_meshes([pts3d_to_trimesh(img, pts, mask) ...]) for a few small multi-view cases, with their inputs;
- the reference's OPENGL and CAM_COLORS;
- the inspect.signature strings of get_3D_model_from_scene and _convert_scene_output_to_glb.
tests/test_glb_cpu.py holds the restatement (and through it the GPU kernels) to these.

    python tools/make_glb_golden.py"""
import inspect
import os
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

OUT = os.path.join(ROOT, 'tests', 'golden', 'glb_reference.pt')

# (H, W, mask kind) per view; each case is one cat_meshes call
CASES = [
    [(7, 5, 'random')],
    [(16, 12, 'random'), (12, 16, 'random')],
    [(1, 9, 'true'), (6, 8, 'false'), (5, 7, 'true')],
    [(9, 1, 'true'), (8, 6, 'random'), (7, 5, 'sparse')],
]


def _stub(name, **attrs):
    mod = types.ModuleType(name)
    for k, v in attrs.items():
        setattr(mod, k, v)
    sys.modules.setdefault(name, mod)


def main():
    from oracle.ref_import import REFERENCE_ROOT, import_reference
    import_reference()
    _stub('gradio')
    _stub('matplotlib')
    _stub('matplotlib.pyplot')
    import dust3r.viz as V
    import dust3r.demo as D
    assert os.path.realpath(V.__file__).startswith(os.path.realpath(REFERENCE_ROOT))
    rng = np.random.default_rng(7)
    cases = []
    for spec in CASES:
        views = []
        for H, W, kind in spec:
            img = (rng.integers(0, 256, size=(H, W, 3)) / 255).astype(np.float32)
            pts = rng.normal(size=(H, W, 3)).astype(np.float32)
            mask = {'true': np.ones((H, W), bool), 'false': np.zeros((H, W), bool), 'random': rng.random((H, W)) < 0.7,
                    'sparse': rng.random((H, W)) < 0.3}[kind]
            views.append((img, pts, mask))
        out = V.cat_meshes([V.pts3d_to_trimesh(img, pts, mask) for img, pts, mask in views])
        cases.append(dict(imgs=[torch.from_numpy(v[0]) for v in views], masks=[torch.from_numpy(v[2]) for v in views],
                          faces=torch.from_numpy(out['faces'].astype(np.int32)), face_colors=torch.from_numpy(out['face_colors'].astype(np.float32))))
    rec = dict(cases=cases, OPENGL=torch.from_numpy(np.asarray(V.OPENGL)), CAM_COLORS=[tuple(c) for c in V.CAM_COLORS],
               signatures={name: str(inspect.signature(getattr(D, name))) for name in ('get_3D_model_from_scene', '_convert_scene_output_to_glb')})
    torch.save(rec, OUT)
    print(OUT, os.path.getsize(OUT), 'bytes', rec['signatures'])


if __name__ == '__main__':
    main()
