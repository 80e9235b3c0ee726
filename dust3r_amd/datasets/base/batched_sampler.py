"""Random sampling where every batch shares one feature (the aspect-ratio index). For the same (len, batch_size, pool_size,
world_size, rank, drop_last, epoch) the stream equals the reference's dust3r/datasets/base/batched_sampler.py, which
tests/golden/datasets_sampler.json pins: generator seeded with epoch + 777, draw 1 a shuffle of arange(total), draw 2 one feature per
batch, then each rank's run of whole batches."""
import numpy as np
import torch


def round_by(total, multiple, up=False):
    """`total` rounded down (or up) to a multiple of `multiple`"""
    return (total + (multiple - 1 if up else 0)) // multiple * multiple


class BatchedRandomSampler:
    """Yields (sample_idx, feat_idx); each run of `batch_size` indices has the same feat_idx, drawn from `pool_size` values."""

    def __init__(self, dataset, batch_size, pool_size, world_size=1, rank=0, drop_last=True):
        if world_size > 1 and not drop_last:
            raise AssertionError('must drop the last batch in distributed mode')
        self.batch_size, self.pool_size, self.world_size, self.rank = batch_size, pool_size, world_size, rank
        self.len_dataset = len(dataset)
        self.total_size = round_by(self.len_dataset, batch_size * world_size) if drop_last else self.len_dataset
        self.epoch = None

    def __len__(self):
        return self.total_size // self.world_size

    def set_epoch(self, epoch):
        self.epoch = epoch

    def _generator(self):
        if self.epoch is not None:
            return np.random.default_rng(seed=self.epoch + 777)
        if (self.world_size, self.rank) != (1, 0):
            raise AssertionError('use set_epoch() if distributed mode is used')
        return np.random.default_rng(seed=int(torch.randint(0, 2 ** 62, ()).item()))      # no epoch given: a fresh order every pass

    def __iter__(self):
        rng = self._generator()
        order = np.arange(self.total_size)
        rng.shuffle(order)
        n_batches = -(-self.total_size // self.batch_size)
        feature = np.repeat(rng.integers(self.pool_size, size=n_batches), self.batch_size)[:self.total_size]
        batches_per_rank = -(-self.total_size // (self.world_size * self.batch_size))
        mine = slice(self.rank * batches_per_rank * self.batch_size, (self.rank + 1) * batches_per_rank * self.batch_size)
        yield from zip(order[mine], feature[mine])
