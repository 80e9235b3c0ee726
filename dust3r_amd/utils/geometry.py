"""Geometry helpers of the hot path. The reference's `dust3r/utils/geometry.py` offers general-purpose versions (`xy_grid` :15-37,
`geotrf` :40-101, `inv` :104-111); this package needs three call shapes only -- a pixel grid, "apply a batch of 4x4 (or one 4x4 / 3x3) to
points", and a matrix inverse -- plus `find_reciprocal_matches` (:345-361) on the GPU."""
import numpy as np
import torch


def xy_grid(W, H, device=None, origin=(0, 0), **arange_kw):
    """(H, W, 2) pixel grid, out[v, u] = (u + origin[0], v + origin[1]); a numpy array when device is None, else a tensor there."""
    if device is None:
        u, v = np.meshgrid(np.arange(origin[0], origin[0] + W, **arange_kw), np.arange(origin[1], origin[1] + H, **arange_kw), indexing='xy')
        return np.stack((u, v), axis=-1)
    u, v = torch.meshgrid(torch.arange(origin[0], origin[0] + W, device=device, **arange_kw),
                          torch.arange(origin[1], origin[1] + H, device=device, **arange_kw), indexing='xy')
    return torch.stack((u, v), dim=-1)


def geotrf(Trf, pts, ncol=None, norm=False):
    """Points (..., d) through transforms of size (d+1)x(d+1) (affine part applied, homogeneous row ignored) or d x d.
    Trf is one matrix, or a batch (B, ., .) matching the leading dimension of pts (B, ..., d). `norm` divides by the last
    coordinate (projection) and scales by it -- for one (d+1)x(d+1) matrix, by the homogeneous coordinate of the full product, as the
    reference does (also for a batch of them, except for torch pts (B, H, W, d), where the reference is affine too); `ncol` keeps
    the first columns. numpy in -> numpy out, torch in -> torch out."""
    is_np = isinstance(Trf, np.ndarray)
    pts = np.asarray(pts) if is_np else torch.as_tensor(pts, dtype=Trf.dtype, device=Trf.device)
    d = pts.shape[-1]
    einsum_path = not is_np and Trf.ndim == 3 and pts.ndim == 4
    if norm and Trf.ndim in (2, 3) and Trf.shape[-1] == d + 1 and not einsum_path:
        # homogeneous (d+1)x(d+1) matrices (a homography; visloc.py:116-117's to_orig): the full projective product divided by the
        # homogeneous coordinate, as the reference does -- one matrix, or one per leading index of pts. The reference's torch
        # einsum path (B matrices, pts (B, H, W, d)) is affine and divides by the last coordinate, as below. Elementwise, in a fixed
        # order, so numpy and torch give the same bits.
        def coef(i, k):                                  # Trf[i, k], or Trf[:, i, k] broadcast over pts (B, ..., d)
            return Trf[:, i, k].reshape((-1,) + (1,) * (pts.ndim - 2)) if Trf.ndim == 3 else Trf[i, k]
        rows = []
        for i in range(d + 1):
            acc = pts[..., 0] * coef(i, 0)
            for k in range(1, d):
                acc = acc + pts[..., k] * coef(i, k)
            rows.append(acc + coef(i, d))
        out = (np.stack if is_np else torch.stack)(rows[:d], -1) / rows[d][..., None]
        if norm != 1:
            out = out * norm
        return out[..., :ncol] if ncol else out
    lin = Trf[..., :d, :d]
    shift = Trf[..., :d, d] if Trf.shape[-1] == d + 1 else None
    if Trf.ndim == 3:                                  # one transform per leading index of pts
        flat = pts.reshape(pts.shape[0], -1, d)
        out = flat @ (lin.swapaxes(-1, -2))
        if shift is not None:
            out = out + shift[:, None, :]
    else:
        out = pts.reshape(-1, d) @ (lin.T if is_np else lin.transpose(-1, -2))
        if shift is not None:
            out = out + shift
    out = out.reshape(pts.shape)
    if norm:
        out = out / out[..., -1:]
        if norm != 1:
            out = out * norm
    return out[..., :ncol] if ncol else out


def inv(mat):
    if isinstance(mat, torch.Tensor):
        return torch.linalg.inv(mat)
    if isinstance(mat, np.ndarray):
        return np.linalg.inv(mat)
    raise ValueError(f'bad matrix type = {type(mat)}')


def find_reciprocal_matches(P1, P2):
    """Mirror of the reference `find_reciprocal_matches` (dust3r/utils/geometry.py:345-361; caller visloc.py:105): mutual nearest
    neighbours between two 3-D point sets. Returns (reciprocal_in_P2 bool (len P2), nn2_in_P1 int (len P2), number of matches),
    numpy arrays for numpy inputs and torch tensors for torch inputs. The two nearest-neighbour queries run as exhaustive scans
    on the GPU (d3r_nearest_neighbors) instead of SciPy KD-trees; exact distance ties resolve to the lowest index."""
    import ctypes as C

    from .. import _lib
    from .._lib import check, current_stream, lib, ptr
    _lib.require_device()
    as_numpy = isinstance(P1, np.ndarray)
    dev = P1.device if (isinstance(P1, torch.Tensor) and P1.is_cuda) else torch.device('cuda', torch.cuda.current_device())
    a = torch.as_tensor(P1, dtype=torch.float32).reshape(-1, 3).to(dev).contiguous()
    b = torch.as_tensor(P2, dtype=torch.float32).reshape(-1, 3).to(dev).contiguous()
    nn1_in_P2 = torch.empty(len(a), dtype=torch.int32, device=dev)
    nn2_in_P1 = torch.empty(len(b), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        check(lib.d3r_nearest_neighbors(ptr(a), len(a), ptr(b), len(b), ptr(nn1_in_P2), current_stream()), 'nearest_neighbors')
        check(lib.d3r_nearest_neighbors(ptr(b), len(b), ptr(a), len(a), ptr(nn2_in_P1), current_stream()), 'nearest_neighbors')
    nn1, nn2 = nn1_in_P2.long(), nn2_in_P1.long()
    reciprocal_in_P2 = nn1[nn2] == torch.arange(len(nn2), device=dev)
    count = int(reciprocal_in_P2.sum())
    if as_numpy:
        return reciprocal_in_P2.cpu().numpy(), nn2.cpu().numpy(), count
    return reciprocal_in_P2, nn2, count


# ---------------------------------------------------------------------------------------------------------------------------------
# The joint statistics the regression criteria are built from (dust3r/utils/geometry.py:249-342), as thin callers of the fused
# criterion kernels (dust3r_amd/csrc/losses.hip through dust3r_amd.losses.pair_criterion / masked_median). Results come back on the
# device of the inputs.
def _joint_stats(pts1, pts2, valid1, valid2, **kw):
    from ..losses import pair_criterion
    if pts1.ndim < 3 or pts1.shape[-1] != 3 or (pts2 is not None and (pts2.ndim < 3 or pts2.shape[-1] != 3)):
        raise ValueError('points must be (B, ..., 3)')
    if pts2 is not None and pts2.shape != pts1.shape:
        raise ValueError('both views must share one shape')
    eye = torch.eye(4).expand(pts1.shape[0], 4, 4)
    stats, _, _ = pair_criterion(pts1, pts2, eye, valid1, valid2, pts1, pts2, **kw)
    return stats


def normalize_pointcloud(pts1, pts2, norm_mode='avg_dis', valid1=None, valid2=None, ret_factor=False):
    """Both pointmaps divided by their JOINT norm factor: the mean over valid points of |p| ('avg_dis'), of log1p|p| ('avg_log1p',
    and 'avg_warp-log1p', which first rescales every point to length log1p|p|), the median of |p| ('median_dis') or the squared mean
    of sqrt|p| ('sqrt_dis'); the factor is clipped below at 1e-8."""
    from ..losses import NORM_MODES, NORM_PR, STAGE_NORM
    if not norm_mode or norm_mode not in NORM_MODES:
        raise ValueError(f'bad norm_mode={norm_mode!r}')
    stats = _joint_stats(pts1, pts2, valid1, valid2, norm_mode=norm_mode, gt_scale=True, stop_after=STAGE_NORM)
    factor = stats[:, NORM_PR].float().to(pts1.device).reshape((-1,) + (1,) * (pts1.ndim - 1))

    def apply(p, valid):
        if norm_mode == 'avg_warp-log1p':      # an invalid point counts as the origin, as in the reference: its warp factor is 0
            d = p.norm(dim=-1, keepdim=True)
            if valid is not None:
                d = d * torch.as_tensor(valid).to(p.device).reshape(d.shape)
            p = p * (torch.log1p(d) / d.clip(min=1e-8))
        return p / factor
    res = apply(pts1, valid1) if pts2 is None else (apply(pts1, valid1), apply(pts2, valid2))
    if ret_factor:
        res = (res if isinstance(res, tuple) else (res,)) + (factor,)
    return res


def get_joint_pointcloud_depth(z1, z2, valid_mask1, valid_mask2=None, quantile=0.5):
    """(B,) joint median (the lower one, as torch.nanmedian) of the valid depths of both views."""
    if quantile != 0.5:
        raise NotImplementedError('only the median (quantile=0.5) is selected on the GPU')
    from ..losses import masked_median
    return masked_median(z1, z2, valid_mask1, valid_mask2).to(z1.device)


def get_joint_pointcloud_center_scale(pts1, pts2, valid_mask1=None, valid_mask2=None, z_only=False, center=True):
    """(centre (B, 1, 1, 3), scale (B, 1, 1, 1)): the per-coordinate joint median of the valid points (x and y zeroed when z_only) and the
    joint median distance to it (to the origin when center is False)."""
    from ..losses import CENTER_FULL, CENTER_NONE, CENTER_PR, CENTER_Z_ONLY, SCALE_PR, STAGE_SCALE
    # z_only zeroes the centre's x and y before the distances are taken; center=False keeps the centre out of them
    stats = _joint_stats(pts1, pts2, valid_mask1, valid_mask2, norm_mode=None, scale_inv=True, stop_after=STAGE_SCALE,
                         center_mode=CENTER_NONE if not center else (CENTER_Z_ONLY if z_only else CENTER_FULL))
    ctr = stats[:, CENTER_PR:CENTER_PR + 3].float().to(pts1.device)
    if z_only:
        ctr[:, :2] = 0
    return ctr[:, None, None, :], stats[:, SCALE_PR].float().to(pts1.device)[:, None, None, None]
