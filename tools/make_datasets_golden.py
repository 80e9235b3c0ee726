"""Records tests/golden/datasets_*.pt from the UNMODIFIED reference dataset code (runs only where the reference is present).

The reference is imported through oracle.ref_import.import_reference(); what its shims lack is added here at run time: a placeholder
ColorJitter, cv2.resize / INTER_NEAREST / IMREAD_UNCHANGED by the documented nearest-neighbour rule (sx = min(floor(dx * in / out),
in - 1); parity-unpinned against a real opencv-python) and a PIL-backed imread. Inputs come from dust3r_amd.datasets.synthetic (the
tests rebuild them); the files hold outputs only. `img` is stored as the uint8 it was normalised from (the test maps it through the
same torch expression). The crop boxes, resample size and filter of every view are captured from the calls the reference makes."""
import json
import os
import re
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
GOLD = os.path.join(ROOT, 'tests', 'golden')

CASES = {      # name -> (sources (W, H, principal point), pairs, constructor keywords, indices)
    'views': ([(200, 150, (0.5, 0.5)), (150, 200, (0.5, 0.5)), (160, 150, (0.5, 0.5)), (50, 40, (0.5, 0.5)), (210, 150, (1 / 3, 0.5)), (200, 150, (0.5, 0.6))],
              3, dict(resolution=(64, 48), seed=777), [0, 1, 2]),
    'aug': ([(200, 150, (0.5, 0.5)), (160, 150, (0.5, 0.5)), (150, 210, (0.5, 0.4)), (40, 30, (0.5, 0.5))], 2, dict(resolution=(48, 32), seed=5, aug_crop=16), [0, 1]),
    'tworesolutions': ([(200, 150, (0.5, 0.5)), (150, 200, (0.5, 0.5)), (150, 150, (0.5, 0.5)), (180, 150, (0.45, 0.5))], 6,
                       dict(resolution=[(48, 32), (32, 32)], seed=11), 'sampler'),
}
SAMPLERS = [dict(n=37, batch_size=4, pool_size=3, world_size=1, rank=0, drop_last=True), dict(n=37, batch_size=4, pool_size=3, world_size=1, rank=0, drop_last=False),
            dict(n=37, batch_size=4, pool_size=3, world_size=2, rank=0, drop_last=True), dict(n=37, batch_size=4, pool_size=3, world_size=2, rank=1, drop_last=True)]


def install_shims():
    import PIL.Image
    from oracle.ref_import import import_reference
    import_reference()
    import cv2
    import torchvision.transforms as tvf

    def resize(src, dsize, fx=0, fy=0, interpolation=0):
        w, h = int(dsize[0]), int(dsize[1])
        sx = np.minimum(np.floor(np.arange(w) * src.shape[1] / w).astype(np.int64), src.shape[1] - 1)
        sy = np.minimum(np.floor(np.arange(h) * src.shape[0] / h).astype(np.int64), src.shape[0] - 1)
        return src[sy[:, None], sx[None, :]]
    cv2.resize, cv2.INTER_NEAREST, cv2.IMREAD_UNCHANGED = resize, 0, -1
    cv2.imread = lambda path, flags=1: np.asarray(PIL.Image.open(path) if flags == -1 else PIL.Image.open(path).convert('RGB'))[..., ::(1 if flags == -1 else -1)]
    cv2.cvtColor = lambda img, code: img[..., ::-1]
    tvf.ColorJitter = lambda *a, **k: (lambda x: x)


def main():
    install_shims()
    import dust3r.datasets.utils.cropping as cropping
    from dust3r.datasets.base.base_stereo_view_dataset import BaseStereoViewDataset
    from dust3r.datasets.base.batched_sampler import BatchedRandomSampler
    from dust3r_amd.datasets.synthetic import SyntheticViewsMixin
    from oracle.ref_import import REFERENCE_ROOT

    class RefSynthetic(SyntheticViewsMixin, BaseStereoViewDataset):
        def __init__(self, sources, n_pairs, **kwargs):
            BaseStereoViewDataset.__init__(self, **kwargs)
            self._init_sources(sources, n_pairs)

    log = []
    crop0, resize0 = cropping.crop_image_depthmap, cropping.ImageList.resize
    cropping.crop_image_depthmap = lambda image, depthmap, K, bbox: (log.append(('crop', tuple(int(x) for x in bbox))), crop0(image, depthmap, K, bbox))[1]
    cropping.ImageList.resize = lambda self, size, resample=None: (log.append(('resize', tuple(int(x) for x in size), 'lanczos' if resample == cropping.lanczos else 'bicubic')),
                                                                    resize0(self, size, resample=resample))[1]

    def record(ds, idx):
        del log[:]
        views = ds[idx]
        out = []
        for v, view in enumerate(views):
            (_, crop1), (_, rs, filt), (_, crop2) = log[3 * v:3 * v + 3]
            u8 = torch.round((view['img'] * 0.5 + 0.5) * 255).to(torch.uint8)
            assert torch.equal((u8.float().div(255) - 0.5) / 0.5, view['img'])
            out.append(dict(crop1=crop1, resample_size=rs, filter=filt, crop2=crop2, img_u8=u8, depthmap=torch.from_numpy(np.ascontiguousarray(view['depthmap'])),
                            pts3d=torch.from_numpy(np.ascontiguousarray(view['pts3d'])), valid_mask=torch.from_numpy(np.ascontiguousarray(view['valid_mask'])),
                            camera_intrinsics=torch.from_numpy(np.ascontiguousarray(view['camera_intrinsics'])), camera_pose=torch.from_numpy(view['camera_pose']),
                            true_shape=torch.from_numpy(view['true_shape']), idx=tuple(int(x) for x in view['idx']), rng=view['rng'],
                            names=(view['dataset'], view['label'], view['instance'])))
        return out

    for name, (sources, n_pairs, kw, indices) in CASES.items():
        ds = RefSynthetic(sources, n_pairs, **kw)
        if indices == 'sampler':
            sampler = ds.make_sampler(2, shuffle=True, drop_last=True)
            sampler.set_epoch(0)
            indices = [tuple(int(x) for x in i) for i in sampler][:4]
        gold = dict(indices=indices, views=[record(ds, i) for i in indices], numpy=np.__version__)
        path = os.path.join(GOLD, f'datasets_{name}.pt')
        torch.save(gold, path)
        print(path, os.path.getsize(path))

    streams = []
    for cfg in SAMPLERS:
        for epoch in (0, 3):
            s = BatchedRandomSampler(range(cfg['n']), cfg['batch_size'], cfg['pool_size'], world_size=cfg['world_size'], rank=cfg['rank'], drop_last=cfg['drop_last'])
            s.set_epoch(epoch)
            streams.append(dict(cfg, epoch=epoch, length=len(s), stream=[[int(a), int(b)] for a, b in s]))
    resized = {}
    for epoch in (0, 3):
        import dust3r.datasets.base.easy_dataset as easy
        r = easy.ResizedDataset(25, list(range(10)))
        r.set_epoch(epoch)
        resized[str(epoch)] = [int(x) for x in r._idxs_mapping]
    imports = []
    for fname in ('dust3r/training.py', 'dust3r/datasets/co3d.py'):
        for m in re.finditer(r'^from (dust3r\.datasets[\w.]*) import ([^\n#]+)', open(os.path.join(REFERENCE_ROOT, fname)).read(), re.M):
            names = [n.strip() for n in m.group(2).split(',') if n.strip()]
            if names != ['*']:
                imports.append([m.group(1), names])
    with open(os.path.join(GOLD, 'datasets_sampler.json'), 'w') as f:
        json.dump(dict(streams=streams, resized_25_of_10=resized, imports=imports), f)
    print(imports)


if __name__ == '__main__':
    main()
