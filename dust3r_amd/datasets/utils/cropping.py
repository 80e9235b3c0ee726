"""The geometry of `_crop_resize_if_necessary` as a PLAN: what the reference's dust3r/datasets/utils/cropping.py does to a picture, its
depth map and its intrinsics, evaluated on the sizes alone (a few dozen flops of host numpy, the same numpy operations in the same
order and dtypes, so the output intrinsics are equal float for float). The pixels are produced later, per batch, by csrc/views.hip."""
from dataclasses import dataclass

import numpy as np

LANCZOS, BICUBIC = 'lanczos', 'bicubic'


@dataclass
class CropResizePlan:
    source_size: tuple        # (W0, H0)
    crop1: tuple              # (l, t, r, b) in the source: centred on the rounded principal point
    scale_final: float        # max(out / in) + 1e-8
    resample_size: tuple      # floor(crop size * scale_final), (w, h)
    filter: str               # LANCZOS when scale_final < 1, else BICUBIC
    crop2: tuple              # (l, t, r, b) in the resampled picture
    intrinsics: np.ndarray    # of the final window

    @property
    def size(self):           # (w, h) of the view before the portrait transpose
        return self.crop2[2] - self.crop2[0], self.crop2[3] - self.crop2[1]


def _shift_principal_point(K, l, t):
    K = K.copy()
    K[0, 2] -= l
    K[1, 2] -= t
    return K


def camera_matrix_of_crop(K, input_resolution, output_resolution, scaling=1, offset_factor=0.5):
    """Intrinsics after scaling by `scaling` and removing `offset_factor` of the margins (pixel centres at +0.5 while scaling)."""
    margins = np.asarray(input_resolution) * scaling - output_resolution
    assert np.all(margins >= 0.0)
    offset = offset_factor * margins
    K = K.copy()
    K[0, 2] += 0.5
    K[1, 2] += 0.5
    K[:2, :] *= scaling
    K[:2, 2] -= offset
    K[0, 2] -= 0.5
    K[1, 2] -= 0.5
    return K


def plan_crop_resize(source_size, intrinsics, resolution, aug_crop=False, rng=None):
    W, H = source_size
    cx, cy = intrinsics[:2, 2].round().astype(int)
    mx, my = min(cx, W - cx), min(cy, H - cy)
    crop1 = (int(cx - mx), int(cy - my), int(cx + mx), int(cy + my))
    K = _shift_principal_point(intrinsics, crop1[0], crop1[1])
    W, H = crop1[2] - crop1[0], crop1[3] - crop1[1]
    assert W > 0 and H > 0, f'principal point outside the picture: {intrinsics[:2, 2]} for {source_size}'

    assert resolution[0] >= resolution[1]
    if H > 1.1 * W:                                              # portrait
        resolution = resolution[::-1]
    elif 0.9 < H / W < 1.1 and resolution[0] != resolution[1]:   # near-square: portrait or landscape at random
        if rng.integers(2):
            resolution = resolution[::-1]

    target = np.array(resolution)
    if aug_crop > 1:
        target += rng.integers(0, aug_crop)
    input_resolution = np.array((W, H))
    scale_final = max(target / (W, H)) + 1e-8
    output_resolution = np.floor(input_resolution * scale_final).astype(int)
    K = camera_matrix_of_crop(K, input_resolution, output_resolution, scaling=scale_final)
    rs = (int(output_resolution[0]), int(output_resolution[1]))

    K2 = camera_matrix_of_crop(K, rs, resolution, offset_factor=0.5)
    l, t = np.int32(np.round(K[:2, 2] - K2[:2, 2]))
    crop2 = (int(l), int(t), int(l) + resolution[0], int(t) + resolution[1])
    assert crop2[0] >= 0 and crop2[1] >= 0 and crop2[2] <= rs[0] and crop2[3] <= rs[1], (crop2, rs)
    return CropResizePlan(tuple(source_size), crop1, float(scale_final), rs, LANCZOS if scale_final < 1 else BICUBIC, crop2,
                          _shift_principal_point(K, l, t))


def nearest_indices(plan):
    """(sy, sx): the source row / column of every pixel of the final window under OpenCV's INTER_NEAREST rule with a given dsize,
    floor(d * in / out) capped at in - 1, through both crops. Parity-unpinned against a real opencv-python (none is installed)."""
    l1, t1, r1, b1 = plan.crop1
    (rw, rh), (l2, t2, r2, b2) = plan.resample_size, plan.crop2
    sx = np.minimum(np.arange(l2, r2, dtype=np.int64) * (r1 - l1) // rw, r1 - l1 - 1) + l1
    sy = np.minimum(np.arange(t2, b2, dtype=np.int64) * (b1 - t1) // rh, b1 - t1 - 1) + t1
    return sy, sx
