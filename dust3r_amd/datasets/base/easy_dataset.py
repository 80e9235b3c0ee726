"""Datasets that resize and combine (the reference's dust3r/datasets/base/easy_dataset.py):
    2 * dataset          every element twice
    10 @ dataset         exactly 10 elements (a per-epoch permutation, repeated if the dataset is shorter)
    dataset1 + dataset2  concatenation
Every wrapper resolves an index to (leaf dataset, leaf index) with `_route`, so that `dataset[idx]`, `dataset.plan(idx)` and the
loader's host-side preparation all take the same path."""
import numpy as np

from .batched_sampler import BatchedRandomSampler


def _split(idx):
    return idx if isinstance(idx, tuple) else (idx, None)


def _join(idx, other):
    return idx if other is None else (idx, other)


class EasyDataset:
    def __add__(self, other):
        return CatDataset([self, other])

    def __rmul__(self, factor):
        return MulDataset(factor, self)

    def __rmatmul__(self, factor):
        return ResizedDataset(factor, self)

    def set_epoch(self, epoch):
        pass

    def make_sampler(self, batch_size, shuffle=True, world_size=1, rank=0, drop_last=True):
        if not shuffle:
            raise NotImplementedError()
        return BatchedRandomSampler(self, batch_size, len(self._resolutions), world_size=world_size, rank=rank, drop_last=drop_last)

    # wrappers override _route; leaves override __getitem__ / plan / planned_views
    def _route(self, idx):
        raise NotImplementedError()

    def __getitem__(self, idx):
        dataset, idx = self._route(idx)
        return dataset[idx]

    def plan(self, idx):
        dataset, idx = self._route(idx)
        return dataset.plan(idx)

    def planned_views(self, idx):
        dataset, idx = self._route(idx)
        return dataset.planned_views(idx)


class _Wrapper(EasyDataset):
    """One dataset behind a positive integer: the repeat count of `k * ds`, the length of `n @ ds`."""

    def __init__(self, number, dataset):
        if not (isinstance(number, int) and number > 0):
            raise AssertionError(f'{type(self).__name__} needs a positive int, got {number!r}')
        self.dataset = dataset
        self._number = number

    @property
    def _resolutions(self):
        return self.dataset._resolutions


class MulDataset(_Wrapper):
    multiplicator = property(lambda self: self._number)

    def __len__(self):
        return len(self.dataset) * self._number

    def __repr__(self):
        return f'{self._number}*{self.dataset!r}'

    def _route(self, idx):
        idx, other = _split(idx)
        return self.dataset, _join(idx // self.multiplicator, other)

    def set_epoch(self, epoch):
        self.dataset.set_epoch(epoch)


class ResizedDataset(_Wrapper):
    new_size = property(lambda self: self._number)

    def __len__(self):
        return self._number

    def __repr__(self):
        return f'{self.new_size:_} @ {repr(self.dataset)}'

    def set_epoch(self, epoch):
        rng = np.random.default_rng(seed=epoch + 777)
        perm = rng.permutation(len(self.dataset))
        repeats = 1 + (len(self) - 1) // len(self.dataset)
        self._idxs_mapping = np.concatenate([perm] * repeats)[:self.new_size]
        assert len(self._idxs_mapping) == self.new_size

    def _route(self, idx):
        assert hasattr(self, '_idxs_mapping'), 'You need to call dataset.set_epoch() to use ResizedDataset.__getitem__()'
        idx, other = _split(idx)
        return self.dataset, _join(self._idxs_mapping[idx], other)


class CatDataset(EasyDataset):
    def __init__(self, datasets):
        strangers = [type(d).__name__ for d in datasets if not isinstance(d, EasyDataset)]
        if strangers:
            raise AssertionError(f'only EasyDatasets concatenate, got {strangers}')
        self.datasets = datasets
        self._cum_sizes = np.add.accumulate(list(map(len, datasets)))      # _cum_sizes[k] = items in datasets[0..k]

    def __len__(self):
        return int(self._cum_sizes[-1])

    def __repr__(self):
        norm = ',transform=Compose( ToTensor() Normalize(mean=(0.5, 0.5, 0.5), std=(0.5, 0.5, 0.5)))'      # too long to print per dataset
        return ' + '.join(repr(dataset).replace(norm, '') for dataset in self.datasets)

    def set_epoch(self, epoch):
        [dataset.set_epoch(epoch) for dataset in self.datasets]

    def _route(self, idx):
        idx, other = _split(idx)
        if not (0 <= idx < len(self)):
            raise IndexError()
        db_idx = np.searchsorted(self._cum_sizes, idx, 'right')
        new_idx = idx - (self._cum_sizes[db_idx - 1] if db_idx > 0 else 0)
        return self.datasets[db_idx], _join(new_idx, other)

    @property
    def _resolutions(self):
        first, *others = (dataset._resolutions for dataset in self.datasets)
        if any(tuple(other) != tuple(first) for other in others):
            raise AssertionError('concatenated datasets must share their resolutions')
        return first
