"""The device half of the view pipeline: the integer coefficient tables of the resampler (built here, on the host, in fp64) and the
one call per batch into csrc/views.hip (`d3r_prepare_views`).

The tables restate Pillow's `precompute_coeffs` + `normalize_coeffs_8bpc` (src/libImaging/Resample.c): per output sample the window
[xmin, xmax) around centre (xx + 0.5) * scale with support * max(scale, 1), the filter evaluated at (x + xmin - centre + 0.5) /
max(scale, 1), a running sum in tap order, the normalisation, and the rounding to PRECISION_BITS = 22 fractional bits with +-0.5.
`sin` is only ever evaluated here: one different last bit on a device would move a rounded coefficient."""
import ctypes as C
import functools

import numpy as np
import torch

from .. import _lib
from ..utils.device import upload_rows
from .utils.cropping import BICUBIC, LANCZOS
from .utils.transforms import norm_table

PRECISION_BITS = 32 - 8 - 2
_SUPPORT = {LANCZOS: 3.0, BICUBIC: 2.0}


def _sinc(x):
    px = x * np.pi
    with np.errstate(invalid='ignore', divide='ignore'):
        return np.where(x == 0.0, 1.0, np.sin(px) / px)


def _filter(name, x):
    if name == LANCZOS:
        return np.where((-3.0 <= x) & (x < 3.0), _sinc(x) * _sinc(x / 3), 0.0)
    a = -0.5
    x = np.abs(x)
    return np.where(x < 1.0, ((a + 2.0) * x - (a + 3.0)) * x * x + 1, np.where(x < 2.0, (((x - 5) * x + 8) * x - 4) * a, 0.0))


@functools.lru_cache(maxsize=256)
def coefficient_table(in_size, out_size, name):
    """(coefficients int32 [out][ksize], bounds int32 [out][2] = {first source sample, taps}) for one axis."""
    scale = in_size / out_size
    filterscale = max(scale, 1.0)
    support = _SUPPORT[name] * filterscale
    ksize = int(np.ceil(support)) * 2 + 1
    center = (np.arange(out_size) + 0.5) * scale
    ss = 1.0 / filterscale
    xmin = np.maximum((center - support + 0.5).astype(np.int64), 0)            # a cast truncates; negative values end at 0 either way
    xmax = np.minimum((center + support + 0.5).astype(np.int64), in_size)
    count = xmax - xmin
    x = np.arange(ksize, dtype=np.int64)[None, :]
    w = np.where(x < count[:, None], _filter(name, ((x + xmin[:, None]) - center[:, None] + 0.5) * ss), 0.0)
    ww = np.cumsum(w, axis=1)[:, -1:]                                           # the running sum, in tap order
    k = np.where(ww != 0.0, w / np.where(ww != 0.0, ww, 1.0), w)
    fixed = np.trunc(np.where(k < 0, -0.5 + k * (1 << PRECISION_BITS), 0.5 + k * (1 << PRECISION_BITS))).astype(np.int32)
    bounds = np.stack((xmin, count), axis=1).astype(np.int32)
    fixed.setflags(write=False)
    bounds.setflags(write=False)
    return fixed, bounds


def resample_host(source, crop1, resample_size, name):
    """The first crop of `source` (uint8 H0 x W0 x 3) resampled to `resample_size` (w, h) by the HOST build of the kernels' arithmetic
    (d3r_selftest_resample_host): what the CPU tests compare with Pillow."""
    source = np.ascontiguousarray(source, dtype=np.uint8)
    l, t, r, b = crop1
    rw, rh = resample_size
    kx, bx = coefficient_table(r - l, rw, name)
    ky, by = coefficient_table(b - t, rh, name)
    out = np.empty((rh, rw, 3), np.uint8)
    p = lambda a: a.ctypes.data_as(C.c_void_p)      # noqa: E731
    _lib.check(_lib.lib.d3r_selftest_resample_host(p(source), source.shape[1], source.shape[0], l, t, r - l, b - t, rw, rh, p(kx), p(bx), kx.shape[1],
                                                   p(ky), p(by), ky.shape[1], p(out)), 'selftest_resample_host')
    return out


def fill_plan(entry, view, H, W):
    """The geometry, intrinsics and pose of one planned view into a _lib.ViewPlan (pointers and workspace fields are left to the caller)."""
    plan = view['img'].plan
    (l1, t1, r1, b1), (l2, t2, r2, b2) = plan.crop1, plan.crop2
    entry.src_w, entry.src_h = plan.source_size
    entry.crop_l, entry.crop_t, entry.crop_w, entry.crop_h = l1, t1, r1 - l1, b1 - t1
    entry.rs_w, entry.rs_h = plan.resample_size
    entry.off_x, entry.off_y, entry.w, entry.h = l2, t2, r2 - l2, b2 - t2
    entry.transpose = int(entry.w < entry.h)
    assert (entry.h, entry.w) == ((W, H) if entry.transpose else (H, W)), 'the views of a batch must share one shape'
    K = view['K_pixels']
    entry.fu, entry.fv, entry.cu, entry.cv = float(K[0, 0]), float(K[1, 1]), float(K[0, 2]), float(K[1, 2])
    pose = np.asarray(view['camera_pose'], dtype=np.float32)
    for i in range(12):
        entry.pose[i] = float(pose[i // 4, i % 4])
    return entry


_device_tables = {}
_norm_tables = {}


def _table_on(device, key):
    """int32 coefficient and bounds tables of one (in, out, filter) on `device`, uploaded once."""
    full = (str(device),) + key
    if full not in _device_tables:
        if len(_device_tables) > 512:
            _device_tables.clear()
        k, b = coefficient_table(*key)
        _device_tables[full] = (torch.from_numpy(k.copy()).to(device), torch.from_numpy(b.copy()).to(device), k.shape[1], b)
    return _device_tables[full]


@torch.no_grad()
def prepare_views(views, device=None, resident=None, timing=None):
    """Finish a list of planned views IN PLACE, in one call of d3r_prepare_views: `img` (3, H, W) fp32, `depthmap` (H, W) fp32, `pts3d`
    (H, W, 3) fp32 and `valid_mask` (H, W) bool become slices of four tensors resident on `device`. Returns those tensors
    (n, ...) in the order of `views`. Sources go up in one piece each through utils.device.upload_rows; the call returns once the
    uploads have left host memory (the kernels stay asynchronous), so the host arrays may be released at once.
    `resident`: a dict the caller keeps, {id(source array): device tensor}; sources found there are not uploaded again (measurements).
    `timing`: a dict that receives `kernels` = (start, end) events around the three launches alone."""
    _lib.require_device()
    device = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
    n = len(views)
    w0, h0 = views[0]['img'].size
    H, W = min(w0, h0), max(w0, h0)
    plans = (_lib.ViewPlan * n)()
    assert C.sizeof(_lib.ViewPlan) == _lib.lib.d3r_view_plan_bytes()
    keep, uploaded, offset = [], ({} if resident is None else resident), 0
    with torch.cuda.device(device):
        for entry, view in zip(plans, views):
            plan = view['img'].plan
            fill_plan(entry, view, H, W)
            for name, handle, dtype in (('rgb', view['img'], np.uint8), ('depth', view['depthmap'], np.float32)):
                src = handle.source
                if id(src) not in uploaded:
                    host = np.ascontiguousarray(src, dtype=dtype)               # may be a converted copy: it is what must outlive the upload
                    if not host.flags.writeable:
                        host = host.copy()
                    uploaded[id(src)] = upload_rows(torch.from_numpy(host), device)
                    keep.append((src, host))
                setattr(entry, name, uploaded[id(src)].data_ptr())
            kx, bx, entry.kxs, _ = _table_on(device, (entry.crop_w, entry.rs_w, plan.filter))
            ky, by, entry.kys, by_host = _table_on(device, (entry.crop_h, entry.rs_h, plan.filter))
            entry.kx, entry.bx, entry.ky, entry.by = kx.data_ptr(), bx.data_ptr(), ky.data_ptr(), by.data_ptr()
            rows = by_host[entry.off_y:entry.off_y + entry.h]                      # the crop rows the kept output rows tap
            entry.row0 = int(rows[:, 0].min())
            entry.nrows = int((rows[:, 0] + rows[:, 1]).max()) - entry.row0
            entry.tmp_off = offset
            offset += (entry.nrows * entry.w * 3 + 255) // 256 * 256
        if str(device) not in _norm_tables:
            _norm_tables[str(device)] = norm_table().to(device)
        plans_dev = torch.frombuffer(bytearray(bytes(plans)), dtype=torch.uint8).to(device)
        if keep:                                                                # the host arrays are read by copies still in flight
            uploads_done = torch.cuda.Event()
            uploads_done.record()
            uploads_done.synchronize()
        workspace = torch.empty(max(offset, 256), dtype=torch.uint8, device=device)
        img = torch.empty((n, 3, H, W), dtype=torch.float32, device=device)
        depthmap = torch.empty((n, H, W), dtype=torch.float32, device=device)
        pts3d = torch.empty((n, H, W, 3), dtype=torch.float32, device=device)
        valid = torch.empty((n, H, W), dtype=torch.uint8, device=device)
        if timing is not None:
            timing['kernels'] = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
            timing['kernels'][0].record()
        _lib.check(_lib.lib.d3r_prepare_views(n, plans, _lib.ptr(plans_dev), H, W, _lib.ptr(_norm_tables[str(device)]), _lib.ptr(workspace),
                                              workspace.numel(), _lib.ptr(img), _lib.ptr(depthmap), _lib.ptr(pts3d), _lib.ptr(valid),
                                              _lib.current_stream()), 'prepare_views')
        if timing is not None:
            timing['kernels'][1].record()
    valid = valid.view(torch.bool)
    for i, view in enumerate(views):
        view['img'], view['depthmap'], view['pts3d'], view['valid_mask'] = img[i], depthmap[i], pts3d[i], valid[i]
        del view['K_pixels']
    return img, depthmap, pts3d, valid
