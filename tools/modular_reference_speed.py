"""The UNMODIFIED reference ModularPointCloudOptimizer (through oracle/ref_import.py) timed on the host CPU, for scale next to the engine's
Modular figure (profiles/modular/modular_speed.log). A smaller scene than the engine's 20 views / 190 edges at 512x384: the reference's per-edge
autograd loop runs a few iterations per second here.

    python tools/modular_reference_speed.py [--threads 16]
"""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import make_modular_golden as M  # noqa: E402  (imports the reference)

from dust3r_amd.synthetic import synthetic_scene  # noqa: E402

if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--threads', type=int, default=16)
    ap.add_argument('--niter', type=int, default=20)
    args = ap.parse_args()
    torch.set_num_threads(args.threads)
    n, H, W = 8, 96, 128
    out, init, gt = synthetic_scene(n, H, W, seed=0, symmetrize=False)
    scene = M.ref_scene(out)
    scene.load_state_dict(scene.state_dict(trainable=True) | M.state_from_init(init, [(H, W)] * n))
    scene.compute_global_alignment(init=None, niter=2, schedule='cosine', lr=0.01)          # warm-up
    t = time.perf_counter()
    scene.compute_global_alignment(init=None, niter=args.niter, schedule='cosine', lr=0.01)
    dt = time.perf_counter() - t
    print(f'reference ModularPointCloudOptimizer on the CPU ({args.threads} threads, {os.cpu_count()} logical CPUs on the host), {n} views {H}x{W}, '
          f'{len(scene.edges)} edges, {args.niter} cosine iterations: {dt:.2f} s = {args.niter / dt:.1f} it/s')
