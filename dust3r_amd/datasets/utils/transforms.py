"""The dataset transforms by name (the reference's dust3r/datasets/utils/transforms.py). `ImgNorm` is the only one executed, and it is
executed by the view kernels (a 256-entry table of `(u8.float().div(255) - 0.5) / 0.5`, computed by torch); `ColorJitter` is a
training augmentation: it exists as a name so that dataset strings evaluate, and a dataset constructed with it raises."""
import numpy as np
import torch


class _ImgNorm:
    """ToTensor + Normalize((0.5, 0.5, 0.5), (0.5, 0.5, 0.5)); prints like torchvision's Compose, which dataset reprs embed."""

    def __call__(self, pil_img):
        u8 = torch.from_numpy(np.array(pil_img, dtype=np.uint8, order='C'))
        return (u8.permute(2, 0, 1).float().div(255) - 0.5) / 0.5

    def __repr__(self):
        return 'Compose(\n    ToTensor()\n    Normalize(mean=(0.5, 0.5, 0.5), std=(0.5, 0.5, 0.5))\n)'


class _ColorJitter:
    def __call__(self, pil_img):
        raise NotImplementedError('ColorJitter is a training augmentation; dust3r_amd.datasets executes ImgNorm only')

    def __repr__(self):
        return 'Compose(\n    ColorJitter(brightness=(0.5, 1.5), contrast=(0.5, 1.5), saturation=(0.5, 1.5), hue=(-0.1, 0.1))\n    ' + repr(ImgNorm) + '\n)'


ImgNorm = _ImgNorm()
ColorJitter = _ColorJitter()


def norm_table():
    """The ImgNorm value of each of the 256 bytes, as torch computes it on the host."""
    return (torch.arange(256, dtype=torch.int32).to(torch.uint8).float().div(255) - 0.5) / 0.5
