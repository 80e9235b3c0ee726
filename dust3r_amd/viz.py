"""Sky segmentation of the reference's `dust3r/viz.py` (`segment_sky`, viz.py:345-381), the part of that module the scene API needs
(`BasePCOptimizer.mask_sky`). The reference runs it per image on the host with OpenCV and SciPy; here one call segments every image of a
scene on the GPU (csrc/sky.hip, C ABI `d3r_segment_sky`). The rest of the reference's viz.py (trimesh scene export) is not mirrored."""
import numpy as np
import torch

from . import _lib
from ._lib import check, current_stream, lib, ptr


def _as_hwc(image):
    """The image as a tensor where it already is (a contiguous numpy array is wrapped, not copied; a device tensor stays on its device)."""
    t = image.detach() if isinstance(image, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(image))
    if t.ndim != 3 or t.shape[2] != 3:
        raise ValueError(f'segment_sky takes H x W x 3 RGB images, got shape {tuple(t.shape)}')
    if t.dtype not in (torch.uint8, torch.float32):
        raise TypeError(f'segment_sky takes uint8 or float32 (in [0, 1]) images, got {t.dtype}')
    return t


@torch.no_grad()
def segment_sky_batch(images, device):
    """Sky masks of a list of H x W x 3 RGB images (numpy arrays or tensors, all uint8 or all float32 in [0, 1]; sizes may differ), computed
    in one batched call on `device`: a list of (H, W) torch.bool tensors on that device."""
    _lib.require_device()
    arrays = [_as_hwc(im) for im in images]
    if not arrays:
        return []
    is_u8 = arrays[0].dtype == torch.uint8
    if any((a.dtype == torch.uint8) != is_u8 for a in arrays):
        raise TypeError('segment_sky_batch: mix of uint8 and float32 images')
    device = torch.device(device)
    shapes = [a.shape[:2] for a in arrays]
    n, max_area = len(arrays), max(h * w for h, w in shapes)
    rgb = torch.zeros((n, max_area, 3), dtype=torch.uint8 if is_u8 else torch.float32, device=device)
    for i, a in enumerate(arrays):
        rgb[i, :a.shape[0] * a.shape[1]] = a.reshape(-1, 3)            # one copy: host -> device, or device -> device
    hs = torch.tensor([h for h, w in shapes], dtype=torch.int32, device=device)
    ws = torch.tensor([w for h, w in shapes], dtype=torch.int32, device=device)
    masks = torch.empty((n, max_area), dtype=torch.bool, device=device)
    work = torch.empty(int(lib.d3r_segment_sky_workspace_bytes(n, max_area)), dtype=torch.uint8, device=device)
    with torch.cuda.device(device):
        check(lib.d3r_segment_sky(n, ptr(rgb), int(is_u8), ptr(hs), ptr(ws), max_area, ptr(masks), ptr(work), current_stream()), 'segment_sky')
    return [masks[i, :h * w].view(h, w) for i, (h, w) in enumerate(shapes)]


def segment_sky(image):
    """The reference's `segment_sky(image)`: an H x W x 3 RGB image (numpy or tensor; float32 in [0, 1] or uint8) -> its sky mask as a CPU
    (H, W) torch.bool tensor. Runs on the current GPU."""
    return segment_sky_batch([image], torch.device('cuda', torch.cuda.current_device()))[0].cpu()
