"""Datasets and the batch loader (the reference's dust3r/datasets): `Co3d`, the dataset algebra, `BatchedRandomSampler` and
`get_data_loader`. Views are decoded and PLANNED on a thread pool of this process and their pixels are produced per batch on the GPU
(csrc/views.hip), where `loss_of_one_batch` wants them; see DESIGN.md section 4.9."""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from .base.base_stereo_view_dataset import BaseStereoViewDataset, is_good_type, transpose_to_landscape, view_name  # noqa: F401
from .base.batched_sampler import BatchedRandomSampler  # noqa: F401
from .base.easy_dataset import CatDataset, EasyDataset, MulDataset, ResizedDataset  # noqa: F401
from .co3d import Co3d  # noqa: F401
from .prepare import prepare_views
from .synthetic import SyntheticStereo  # noqa: F401
from .utils.transforms import *  # noqa: F401,F403
from .utils.transforms import ColorJitter, ImgNorm  # noqa: F401



class SequentialSampler:
    def __init__(self, dataset):
        self.n = len(dataset)

    def __len__(self):
        return self.n

    def __iter__(self):
        return iter(range(self.n))


class RandomSampler(SequentialSampler):
    def __iter__(self):
        return iter(torch.randperm(self.n).tolist())


def collate_views(pairs, pixels=None):
    """[(view1, view2), ...] of finished views -> (view1, view2) in torch's default-collate structure on the views' device: arrays and tensors stacked,
    strings in lists, `idx` a list of three tensors, `rng` a tensor. `pixels` = the (img, depthmap, pts3d, valid_mask) tensors of the
    batch laid out view-1-first, whose halves are used as they are instead of stacking the per-view slices again."""
    B = len(pairs)
    out = []
    for side in (0, 1):
        views = [pair[side] for pair in pairs]
        device = views[0]['img'].device
        col = {}
        for key, first in views[0].items():
            vals = [v[key] for v in views]
            if pixels is not None and key in ('img', 'depthmap', 'pts3d', 'valid_mask'):
                col[key] = pixels[('img', 'depthmap', 'pts3d', 'valid_mask').index(key)][side * B:(side + 1) * B]
            elif isinstance(first, torch.Tensor):
                col[key] = torch.stack(vals)
            elif isinstance(first, np.ndarray):
                col[key] = torch.from_numpy(np.stack(vals)).to(device)
            elif isinstance(first, str):
                col[key] = vals
            elif isinstance(first, tuple):
                col[key] = [torch.tensor([int(v[i]) for v in vals], device=device) for i in range(len(first))]
            else:
                col[key] = torch.tensor(vals, device=device)
        out.append(col)
    return tuple(out)


class ViewLoader:
    """Iterable of collated (view1, view2) batches with `.dataset`, `.sampler` and `__len__`. Two stages run ahead of the consumer, both
    on threads of this process (never worker processes: a process that has opened the GPU must not fork, and workers would each open
    the card): `threads` threads decode and plan the items of the next batches, and one more thread uploads a planned batch and
    enqueues its kernels on a stream of its own. The consumer's stream waits for that batch's event, so decoding, planning, upload and
    the view kernels of batch i + 1 all overlap the forward of batch i. `depth` batches are in flight."""
    depth = 2

    def __init__(self, dataset, sampler, batch_size, drop_last, threads, device=None):
        self.dataset, self.sampler, self.batch_size, self.drop_last, self.threads = dataset, sampler, batch_size, drop_last, threads
        self.device = None if device is None else torch.device(device)

    def __len__(self):
        n = len(self.sampler)
        return n // self.batch_size if self.drop_last else -(-n // self.batch_size)

    def _index_batches(self):
        batch = []
        for idx in self.sampler:
            batch.append(idx)
            if len(batch) == self.batch_size:
                yield batch
                batch = []
        if batch and not self.drop_last:
            yield batch

    def _finish(self, futures, device, stream):
        pairs = [f.result() for f in futures]
        views = [p[0] for p in pairs] + [p[1] for p in pairs]
        with torch.cuda.device(device), torch.cuda.stream(stream):
            batch = collate_views(pairs, pixels=prepare_views(views, device))
            ready = torch.cuda.Event()
            ready.record(stream)
        return batch, ready

    def __iter__(self):
        from collections import deque
        device = torch.device('cuda', torch.cuda.current_device()) if self.device is None else self.device
        stream = torch.cuda.Stream(device)
        with ThreadPoolExecutor(max_workers=self.threads) as pool, ThreadPoolExecutor(max_workers=1) as finisher:
            in_flight, batches = deque(), self._index_batches()

            def feed():
                for batch in batches:
                    futures = [pool.submit(self.dataset.planned_views, idx) for idx in batch]
                    in_flight.append(finisher.submit(self._finish, futures, device, stream))
                    if len(in_flight) >= self.depth:
                        return
            feed()
            while in_flight:
                batch, ready = in_flight.popleft().result()
                feed()
                consumer = torch.cuda.current_stream(device)
                consumer.wait_event(ready)
                for view in batch:                     # allocated on the loader's stream, used on the consumer's
                    for value in view.values():
                        for t in (value if isinstance(value, list) else [value]):
                            if isinstance(t, torch.Tensor):
                                t.record_stream(consumer)
                yield batch


def load_threads(num_workers):
    """min(num_workers, 16), DUST3R_AMD_LOAD_THREADS and the CPUs this process can use: the rule of utils.image.load_images."""
    from ..utils.device import usable_cpus
    return max(1, min(int(num_workers) if num_workers else 1, 16, int(os.environ.get('DUST3R_AMD_LOAD_THREADS', 16)), usable_cpus()))


def get_data_loader(dataset, batch_size, num_workers=8, shuffle=True, drop_last=True, pin_mem=True, device=None):
    """The reference's get_data_loader. `dataset` may be a string evaluated in this namespace, e.g.
    "1000 @ Co3d(split='test', ROOT='data/co3d_subset_processed', resolution=224, seed=777)". `pin_mem` is accepted and unused:
    sources go to the device through utils.device.upload_rows."""
    if isinstance(dataset, str):
        dataset = eval(dataset)
    world_size = torch.distributed.get_world_size() if torch.distributed.is_available() and torch.distributed.is_initialized() else 1
    rank = torch.distributed.get_rank() if world_size > 1 else 0
    try:
        sampler = dataset.make_sampler(batch_size, shuffle=shuffle, world_size=world_size, rank=rank, drop_last=drop_last)
    except (AttributeError, NotImplementedError):
        assert world_size == 1, 'multi-rank loading needs a dataset with make_sampler'
        sampler = RandomSampler(dataset) if shuffle else SequentialSampler(dataset)
    return ViewLoader(dataset, sampler, batch_size, drop_last, load_threads(num_workers), device)
