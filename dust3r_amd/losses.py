"""Ground-truth evaluation: the reference's criterion algebra (`dust3r/losses.py`) with its names, signatures and `repr` strings, evaluated
forward-only by the fused HIP entry point `d3r_pair_criterion` (dust3r_amd/csrc/losses.hip).

    criterion = eval("Regr3D_ScaleShiftInv(L21, gt_scale=True)")          # or ConfLoss(Regr3D(L21, norm_mode='avg_dis'), alpha=0.2)
    loss, details = criterion(view1, view2, pred1, pred2)

`view*` carry the ground truth (`pts3d` world points, `camera_pose`, `valid_mask`), `pred*` the network output (`pts3d`,
`pts3d_in_other_view`, `conf`). CPU tensors are moved to the GPU, device tensors are used in place. The kernels return per-pair sums and
counts; the reductions of the reference (a mean over the valid pixels of the whole batch) are composed here from them.

GRADIENTS DO NOT EXIST HERE: `loss` is a 0-dim tensor without a graph. Training (backward, optimisers, `find_opt_scaling`) is out of scope.
Multi-rank evaluation would only need the per-rank (sums, counts) of `pair_criterion` added up before the division.
"""
import copy as _copy
import ctypes as C

import torch

NORM_MODES = {None: 0, False: 0, '': 0, 'avg_dis': 1, 'avg_log1p': 2, 'avg_warp-log1p': 3, 'median_dis': 4, 'sqrt_dis': 5}
STAGE_ALL, STAGE_NORM, STAGE_SHIFT, STAGE_SCALE = 0, 1, 2, 3
CENTER_FULL, CENTER_Z_ONLY, CENTER_NONE = 0, 1, 2
# columns of the statistics array (D3R_CRIT_* of include/dust3r_hip.h)
N1, N2, NORM_PR, NORM_GT, SHIFT_PR, SHIFT_GT, CENTER_PR, CENTER_GT, SCALE_PR, SCALE_GT, SUM_L1, SUM_L2, SUM_CONF1, SUM_CONF2, NSTAT = \
    0, 1, 2, 3, 4, 5, 6, 9, 12, 13, 14, 15, 16, 17, 24


# ------------------------------------------------------------------------------------------------ the kernels' Python face
def _device_of(*tensors):
    for t in tensors:
        if isinstance(t, torch.Tensor) and t.is_cuda:
            return t.device
    return torch.device('cuda', torch.cuda.current_device())


def _f32(t, dev):
    return None if t is None else torch.as_tensor(t).to(device=dev, dtype=torch.float32).contiguous()


def _mask(t, like, dev):
    if t is None:
        return torch.ones(like.shape[:2], dtype=torch.uint8, device=dev)
    t = torch.as_tensor(t).to(dev).reshape(like.shape[0], -1)
    t = t.view(torch.uint8) if t.dtype == torch.bool else (t != 0).view(torch.uint8)
    return t.contiguous()


def pair_criterion(gt_pts1, gt_pts2, inv_pose1, valid1, valid2, pr_pts1, pr_pts2, conf1=None, conf2=None, *, norm_mode='avg_dis',
                   gt_scale=False, shift_inv=False, scale_inv=False, center_mode=CENTER_FULL, dist_clip=None, alpha=None,
                   stop_after=STAGE_ALL, maps=False):
    """One call of `d3r_pair_criterion` for B pairs: points (B, ..., 3), masks (B, ...), poses (B, 4, 4). Returns (stats, map1, map2):
    `stats` a (B, 24) fp64 DEVICE tensor of counts, per-pair statistics and sums (columns named above), the maps (B, N) or None.
    Nothing is synchronised: the caller reads `stats` when it needs the numbers."""
    from . import _lib
    from ._lib import CriterionOpts, check, current_stream, lib, ptr
    _lib.require_device()
    if norm_mode not in NORM_MODES:
        raise ValueError(f'bad norm_mode={norm_mode!r}')
    dev = _device_of(gt_pts1, pr_pts1, gt_pts2, pr_pts2)
    B = gt_pts1.shape[0]
    g1, p1 = _f32(gt_pts1, dev).reshape(B, -1, 3), _f32(pr_pts1, dev).reshape(B, -1, 3)
    N = g1.shape[1]
    g2 = p2 = m2 = None
    if gt_pts2 is not None:
        g2, p2 = _f32(gt_pts2, dev).reshape(B, -1, 3), _f32(pr_pts2, dev).reshape(B, -1, 3)
        m2 = _mask(valid2, g2, dev)
    m1 = _mask(valid1, g1, dev)
    for t in (p1, g2, p2):
        if t is not None and t.shape != g1.shape:
            raise ValueError(f'ground truth and predictions of both views must share one shape, got {tuple(t.shape)} and {tuple(g1.shape)}')
    pose = _f32(inv_pose1, dev).reshape(B, 16)
    use_conf = alpha is not None
    c1 = c2 = None
    if use_conf:
        if not alpha > 0:
            raise ValueError('alpha must be positive')
        c1 = _f32(conf1, dev).reshape(B, N)
        c2 = _f32(conf2, dev).reshape(B, N) if g2 is not None else None
    opts = CriterionOpts(NORM_MODES[norm_mode], int(bool(gt_scale)), int(bool(shift_inv)), int(bool(scale_inv)), int(center_mode), int(use_conf),
                         int(dist_clip is not None), int(stop_after), float(dist_clip or 0.0), float(alpha or 0.0))
    stats = torch.empty((B, NSTAT), dtype=torch.float64, device=dev)
    map1 = torch.empty((B, N), dtype=torch.float32, device=dev) if maps else None
    map2 = torch.empty((B, N), dtype=torch.float32, device=dev) if maps and g2 is not None else None
    with torch.cuda.device(dev):
        work = _lib.workspace(lib.d3r_pair_criterion_workspace_bytes(B, N), dev)
        check(lib.d3r_pair_criterion(B, N, ptr(g1), ptr(g2), ptr(pose), ptr(m1), ptr(m2), ptr(p1), ptr(p2), ptr(c1), ptr(c2), C.byref(opts),
                                     ptr(stats), ptr(map1), ptr(map2), ptr(work), current_stream()), 'pair_criterion')
    return stats, map1, map2


def criterion_passes(**kw):
    """Streaming passes over the inputs that `pair_criterion` makes with these options."""
    from ._lib import CriterionOpts, lib
    opts = CriterionOpts(NORM_MODES[kw.get('norm_mode', 'avg_dis')], int(bool(kw.get('gt_scale'))), int(bool(kw.get('shift_inv'))),
                         int(bool(kw.get('scale_inv'))), 0, 0, 0, int(kw.get('stop_after', 0)), 0.0, 0.0)
    return int(lib.d3r_pair_criterion_passes(C.byref(opts)))


def masked_median(vals1, vals2=None, mask1=None, mask2=None):
    """Lower median (torch.nanmedian's element; NaN for an empty row) of every row of vals1 (B, N) joined with the same row of vals2,
    over the unmasked, non-NaN entries. Returns a (B,) fp32 DEVICE tensor."""
    from . import _lib
    from ._lib import check, current_stream, lib, ptr
    _lib.require_device()
    dev = _device_of(vals1, vals2)
    v1 = _f32(vals1, dev)
    B = v1.shape[0]
    v1 = v1.reshape(B, -1)
    v2 = _f32(vals2, dev).reshape(B, -1) if vals2 is not None else None
    if v2 is not None and v2.shape != v1.shape:
        raise ValueError('both value arrays must share one shape')
    m1 = _mask(mask1, v1, dev) if mask1 is not None else None
    m2 = _mask(mask2, v2, dev) if (mask2 is not None and v2 is not None) else None
    out = torch.empty(B, dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        work = _lib.workspace(lib.d3r_pair_criterion_workspace_bytes(B, v1.shape[1]), dev)
        check(lib.d3r_masked_median(B, v1.shape[1], ptr(v1), ptr(v2), ptr(m1), ptr(m2), ptr(out), ptr(work), current_stream()), 'masked_median')
    return out.float()


# ------------------------------------------------------------------------------------------------ pixel criteria
class BaseCriterion:
    def __init__(self, reduction='mean'):
        self.reduction = reduction

    def __repr__(self):
        return f'{type(self).__name__}()'

    def to(self, *args, **kwargs):       # the criteria hold no tensors
        return self


class LLoss(BaseCriterion):
    """Distance between two point sets (..., d), d <= 3, reduced by `reduction` ('none', 'sum', 'mean'). Inside a Regr3D the distance is
    evaluated by the fused kernel; called directly it is plain torch on the tensors' device."""

    def __call__(self, a, b):
        if a.shape != b.shape or a.ndim < 2 or not 1 <= a.shape[-1] <= 3:
            raise ValueError(f'Bad shape = {tuple(a.shape)}')
        dist = self.distance(a, b)
        if self.reduction == 'none':
            return dist
        if self.reduction == 'sum':
            return dist.sum()
        if self.reduction == 'mean':
            return dist.mean() if dist.numel() else dist.new_zeros(())
        raise ValueError(f'bad {self.reduction=} mode')

    forward = __call__

    def distance(self, a, b):
        raise NotImplementedError()


class L21Loss(LLoss):
    """Euclidean distance between 3-D points"""

    def distance(self, a, b):
        return torch.linalg.vector_norm(a - b, dim=-1)


L21 = L21Loss()


# ------------------------------------------------------------------------------------------------ the algebra
class Criterion:
    def __init__(self, criterion=None):
        if not isinstance(criterion, BaseCriterion):
            raise TypeError(f'{criterion} is not a proper criterion!')
        self.criterion = _copy.copy(criterion)

    def get_name(self):
        return f'{type(self).__name__}({self.criterion})'

    def with_reduction(self, mode='none'):
        """A deep copy whose pixel criteria (along the whole `+` chain) use reduction `mode`."""
        res = _copy.deepcopy(self)
        term = res
        while term is not None:
            if not isinstance(term, Criterion):
                raise TypeError(f'{term} has no pixel criterion')
            term.criterion.reduction = mode
            term = term._loss2
        return res


class MultiLoss:
    """Terms that combine as `a + 0.5 * b` and report each term's value in `details`."""

    def __init__(self):
        self._alpha = 1
        self._loss2 = None

    def compute_loss(self, *args, **kwargs):
        raise NotImplementedError()

    def get_name(self):
        raise NotImplementedError()

    def to(self, *args, **kwargs):
        return self

    def eval(self):
        return self

    def train(self, mode=True):
        return self

    def __mul__(self, alpha):
        if not isinstance(alpha, (int, float)):
            raise TypeError('a criterion is scaled by a number')
        res = _copy.copy(self)
        res._alpha = alpha
        return res
    __rmul__ = __mul__

    def __add__(self, other):
        if not isinstance(other, MultiLoss):
            raise TypeError('only criteria add up')
        res = last = _copy.copy(self)
        while last._loss2 is not None:            # copy the chain so that the operands stay as they were
            last._loss2 = _copy.copy(last._loss2)
            last = last._loss2
        last._loss2 = other
        return res

    def __repr__(self):
        name = self.get_name()
        if self._alpha != 1:
            name = f'{self._alpha:g}*{name}'
        if self._loss2:
            name = f'{name} + {self._loss2}'
        return name

    def __call__(self, *args, **kwargs):
        loss = self.compute_loss(*args, **kwargs)
        if isinstance(loss, tuple):
            loss, details = loss
        else:
            details = {self.get_name(): float(loss)} if loss.ndim == 0 else {}
        if self._alpha != 1:
            loss = loss * self._alpha
        if self._loss2:
            loss2, details2 = self._loss2(*args, **kwargs)
            loss = loss + loss2
            details = {**details, **details2}
        return loss, details

    forward = __call__


def _ratio(num, den):
    """sum / count over the batch; 0 when nothing is valid (the reference's mean with its empty-set guard)"""
    return torch.where(den > 0, num / den.clamp(min=1), torch.zeros_like(num))


class Regr3D(Criterion, MultiLoss):
    """All 3-D points against the ground truth, both expressed in view 1's camera: view 1 is the anchor (asymmetric).
    norm_mode: '{avg,median,sqrt}_dis', 'avg_log1p', 'avg_warp-log1p' or a false value; gt_scale: the ground truth keeps its scale."""
    _shift_inv = False
    _scale_inv = False

    def __init__(self, criterion, norm_mode='avg_dis', gt_scale=False):
        Criterion.__init__(self, criterion)
        MultiLoss.__init__(self)
        if norm_mode and norm_mode not in NORM_MODES:
            raise ValueError(f'bad norm_mode={norm_mode!r}')
        if not isinstance(self.criterion, L21Loss):
            raise NotImplementedError('the fused kernels evaluate the L21 pixel criterion')
        self.norm_mode = norm_mode
        self.gt_scale = gt_scale

    def evaluate(self, gt1, gt2, pred1, pred2, alpha=None, maps=False, dist_clip=None):
        """The kernel call for this criterion: (stats, map1, map2) of `pair_criterion`."""
        from .inference import get_pred_pts3d
        if dist_clip is not None and (self._shift_inv or self._scale_inv):
            raise TypeError(f'{type(self).__name__} takes no dist_clip')        # as the reference's signatures
        pr1 = get_pred_pts3d(gt1, pred1, use_pose=False)
        pr2 = get_pred_pts3d(gt2, pred2, use_pose=True)
        inv_pose = torch.linalg.inv(torch.as_tensor(gt1['camera_pose']).float().cpu())      # B tiny matrices: on the host
        return pair_criterion(gt1['pts3d'], gt2['pts3d'], inv_pose, gt1['valid_mask'], gt2['valid_mask'], pr1, pr2,
                              pred1.get('conf') if alpha is not None else None, pred2.get('conf') if alpha is not None else None,
                              norm_mode=self.norm_mode or None, gt_scale=self.gt_scale, shift_inv=self._shift_inv, scale_inv=self._scale_inv,
                              dist_clip=dist_clip, alpha=alpha, maps=maps)

    def _masks(self, gt1, gt2, dist_clip, dev):
        from .utils.geometry import geotrf, inv
        masks = []
        for gt in (gt1, gt2):
            m = torch.as_tensor(gt['valid_mask']).to(dev).bool()
            if dist_clip is not None:
                pts = geotrf(inv(torch.as_tensor(gt1['camera_pose']).float().to(dev)), torch.as_tensor(gt['pts3d']).float().to(dev))
                m = m & (pts.norm(dim=-1) <= dist_clip)
            masks.append(m)
        return masks

    def compute_loss(self, gt1, gt2, pred1, pred2, **kw):
        mode = self.criterion.reduction
        if mode not in ('none', 'sum', 'mean'):
            raise ValueError(f'bad reduction={mode!r} mode')
        stats, map1, map2 = self.evaluate(gt1, gt2, pred1, pred2, maps=mode == 'none', **kw)
        tot = stats.sum(dim=0)
        name = type(self).__name__
        if mode == 'none':      # the per-pixel losses of the valid pixels, as the reference returns them
            m1, m2 = self._masks(gt1, gt2, kw.get('dist_clip'), stats.device)
            l1, l2 = map1.reshape(m1.shape)[m1], map2.reshape(m2.shape)[m2]
            details = {name + '_pts3d_1': float(l1.mean()), name + '_pts3d_2': float(l2.mean())}
            return ((l1, m1), (l2, m2)), details
        if mode == 'sum':
            l1, l2 = tot[SUM_L1], tot[SUM_L2]
        else:
            l1, l2 = _ratio(tot[SUM_L1], tot[N1]), _ratio(tot[SUM_L2], tot[N2])
        vals = torch.stack((l1, l2, l1 + l2)).float().cpu()          # the one read-back of this term
        return vals[2], {name + '_pts3d_1': float(vals[0]), name + '_pts3d_2': float(vals[1])}


class ConfLoss(MultiLoss):
    """Regression weighted by the predicted confidence: mean over valid pixels of  l * conf - alpha * log(conf)  per view."""

    def __init__(self, pixel_loss, alpha=1):
        super().__init__()
        if not alpha > 0:
            raise ValueError('alpha must be positive')
        if not isinstance(pixel_loss, Regr3D):
            raise TypeError('ConfLoss weights a Regr3D-family pixel loss')
        self.alpha = alpha
        self.pixel_loss = pixel_loss.with_reduction('none')

    def get_name(self):
        return f'ConfLoss({self.pixel_loss})'

    def compute_loss(self, gt1, gt2, pred1, pred2, **kw):
        stats, _, _ = self.pixel_loss.evaluate(gt1, gt2, pred1, pred2, alpha=self.alpha, **kw)
        tot = stats.sum(dim=0)
        c1, c2 = _ratio(tot[SUM_CONF1], tot[N1]), _ratio(tot[SUM_CONF2], tot[N2])
        vals = torch.stack((c1, c2, c1 + c2, tot[SUM_L1] / tot[N1], tot[SUM_L2] / tot[N2])).float().cpu()
        name = type(self.pixel_loss).__name__
        return vals[2], dict(conf_loss_1=float(vals[0]), conf_loss2=float(vals[1]),
                             **{name + '_pts3d_1': float(vals[3]), name + '_pts3d_2': float(vals[4])})


class Regr3D_ShiftInv(Regr3D):
    """Regr3D invariant to a depth shift: the joint median depth is subtracted on each side."""
    _shift_inv = True


class Regr3D_ScaleInv(Regr3D):
    """Regr3D invariant to scale: each side is measured by its median distance to its median centre; with gt_scale the prediction
    is brought to the ground truth's scale instead."""
    _scale_inv = True


class Regr3D_ScaleShiftInv(Regr3D_ScaleInv, Regr3D_ShiftInv):
    """The shift first, then the scale."""
