"""Ground-truth evaluation loop: the body of the reference's `test_one_epoch` (dust3r/training.py:342-377) without its logger.

    table = evaluate(model, criterion, batches, device)

`batches` is any iterable of collated (view1, view2) with the reference's keys (`img`, `pts3d`, `camera_pose`, `valid_mask`,
`true_shape`). Every batch goes through `loss_of_one_batch` (forward on the engine, then the criterion on the device: the predictions never
leave HBM); the table holds, for `loss` and every key of the criterion's details, `<key>_avg` = the mean of the per-batch values and
`<key>_med` = their lower median -- what the reference's SmoothedValue reports with an unbounded window. `batches` can be a
`dust3r_amd.datasets.get_data_loader(...)`: its batches are prepared on the GPU and arrive where the criterion reads them. Multi-rank
evaluation is out of scope (ranks would add their per-pair sums and counts, see dust3r_amd/losses.py)."""
import torch

from .inference import loss_of_one_batch


def _call_in_chunks(model, engine_batch):
    """The model called `engine_batch` pairs at a time (the engine's results do not depend on how a batch is cut)."""
    if engine_batch is None:
        return model
    step = max(int(engine_batch), 1)

    def run(view1, view2):
        n = len(view1['img'])
        if n <= step:
            return model(view1, view2)
        cut = lambda view, i: {k: v[i:i + step] for k, v in view.items()}      # noqa: E731
        parts = [model(cut(view1, i), cut(view2, i)) for i in range(0, n, step)]
        return tuple({k: torch.cat([p[side][k] for p in parts]) for k in parts[0][side]} for side in (0, 1))
    return run


@torch.no_grad()
def evaluate(model, criterion, batches, device, symmetrize_batch=True, engine_batch=None):
    history = {}
    run = _call_in_chunks(model, engine_batch)
    for batch in batches:
        value, details = loss_of_one_batch(batch, run, criterion, device, symmetrize_batch=symmetrize_batch, ret='loss')
        for key, v in dict(loss=float(value), **details).items():
            history.setdefault(key, []).append(float(v))
    table = {}
    for key, values in history.items():
        t = torch.tensor(values, dtype=torch.float64)
        table[f'{key}_avg'] = float(t.mean())
        table[f'{key}_med'] = float(t.median())
    return table
