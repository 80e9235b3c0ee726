"""Times the demo's GLB export for 20 and 100 views of 512 x 384, mesh and point-cloud mode:
- kernels: device events around d3r_scene_mesh alone (inputs on the GPU, outputs and workspace allocated);
- scene_mesh_batch: host clock from the scene's device tensors to the host arrays (upload of the images included);
- export: the whole dust3r_amd.demo.get_3D_model_from_scene writing scene.glb to /dev/shm, and the file size;
- host: the reference's mesh path in numpy (pts3d_to_trimesh per view, the same steps, then cat_meshes; not trimesh's own export) on a
  pool of host threads, one view per task.
The scene is a synthetic one (dust3r_amd.synthetic.synthetic_scene, a sliding-window graph) at its initial state; masks keep ~70 % of
the pixels.

    python tools/glb_speed.py [--threads 16] [--reps 5] [--views 20,100]"""
import argparse
import json
import os
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]

import numpy as np  # noqa: E402
import torch  # noqa: E402

from dust3r_amd import _lib  # noqa: E402
from dust3r_amd._lib import check, current_stream, lib, ptr  # noqa: E402
from dust3r_amd.cloud_opt import global_aligner  # noqa: E402
from dust3r_amd.demo import get_3D_model_from_scene  # noqa: E402
from dust3r_amd.synthetic import outdoor_scene, synthetic_scene  # noqa: E402
from dust3r_amd.viz import scene_mesh_batch  # noqa: E402


def reference_mesh_view(img, pts, valid):
    """the reference's pts3d_to_trimesh (viz.py:38-75) on one view, the same numpy steps: every quad's four triangles, their colours, then
    the faces whose three pixels are valid"""
    H, W = valid.shape
    idx = np.arange(H * W).reshape(H, W)
    idx1, idx2, idx3, idx4 = idx[:-1, :-1].ravel(), idx[:-1, 1:].ravel(), idx[1:, :-1].ravel(), idx[1:, 1:].ravel()
    faces = np.concatenate((np.c_[idx1, idx2, idx3], np.c_[idx3, idx2, idx1], np.c_[idx2, idx3, idx4], np.c_[idx4, idx3, idx2]), axis=0)
    face_colors = np.concatenate((img[:-1, :-1].reshape(-1, 3), img[:-1, :-1].reshape(-1, 3), img[1:, 1:].reshape(-1, 3),
                                  img[1:, 1:].reshape(-1, 3)), axis=0)
    valid_faces = valid.ravel()[faces].all(axis=-1)
    return dict(vertices=pts.reshape(-1, 3), faces=faces[valid_faces], face_colors=face_colors[valid_faces])


def cat_meshes(meshes):
    n_vertices = np.cumsum([0] + [len(m['vertices']) for m in meshes])
    return dict(vertices=np.concatenate([m['vertices'] for m in meshes]), face_colors=np.concatenate([m['face_colors'] for m in meshes]),
                faces=np.concatenate([m['faces'] + n for m, n in zip(meshes, n_vertices)]))


def make_scene(n, H, W, dev):
    out, init, _ = synthetic_scene(n, H, W, seed=3, scene_graph='swin-1', device=dev, device_rng=True)
    scene = global_aligner(out, dev, verbose=False)
    scene.load_state_dict(init)
    scene.imgs = [outdoor_scene(H, W, seed=k).astype(np.float32) / 255 for k in range(n)]
    g = torch.Generator(device=dev)
    g.manual_seed(n)
    with torch.no_grad():
        for c in scene.im_conf:
            c.copy_(torch.where(torch.rand(c.shape, device=dev, generator=g) < 0.7, 10.0, 1.0))
    return scene


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--threads', type=int, default=16)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--views', default='20,100')
    args = ap.parse_args()
    _lib.require_device()
    dev = torch.device('cuda:0')
    H, W = 384, 512
    outdir = '/dev/shm' if os.path.isdir('/dev/shm') else tempfile.gettempdir()
    outdir = tempfile.mkdtemp(dir=outdir)
    rows = []
    for n in [int(v) for v in args.views.split(',')]:
        scene = make_scene(n, H, W, dev)
        with torch.no_grad():
            pts = scene.get_pts3d(raw=True).contiguous()
            scene.min_conf_thr = float(scene.conf_trf(torch.tensor(3.0)))
            masks = scene.get_masks()
            host_pts = [p.cpu().numpy() for p in scene.get_pts3d()]
        imgs = scene.imgs
        host_masks = [m.cpu().numpy() for m in masks]
        for as_pc in (False, True):
            # kernels only
            A = pts.shape[1]
            mask = torch.stack([m.reshape(-1) for m in masks]).to(torch.uint8)
            rgb = torch.from_numpy(np.stack(imgs)).reshape(n, A, 3).to(dev)
            hs = torch.full((n,), H, dtype=torch.int32, device=dev)
            ws = torch.full((n,), W, dtype=torch.int32, device=dev)
            faces = None if as_pc else torch.empty((n * 4 * (H - 1) * (W - 1), 3), dtype=torch.int32, device=dev)
            points = torch.empty((n * A, 3), device=dev) if as_pc else None
            colors = torch.empty((n * A,), dtype=torch.int32, device=dev)
            small = torch.empty((n + 3,), dtype=torch.int64, device=dev)
            work = torch.empty(int(lib.d3r_scene_mesh_workspace_bytes(n, A)), dtype=torch.uint8, device=dev)

            def launch():
                check(lib.d3r_scene_mesh(n, ptr(pts), ptr(mask), ptr(rgb), 0, ptr(hs), ptr(ws), A, int(as_pc), ptr(faces), ptr(points), ptr(colors),
                                         ptr(small), ptr(small[n:].view(torch.float32)), ptr(work), current_stream()), 'scene_mesh')
            for _ in range(3):
                launch()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.reps):
                launch()
            e1.record()
            torch.cuda.synchronize()
            kernel_ms = e0.elapsed_time(e1) / args.reps
            del faces, points, colors, work
            # scene_mesh_batch from the scene's tensors
            scene_mesh_batch(imgs, pts, masks, dev, as_pointcloud=as_pc)
            t0 = time.perf_counter()
            for _ in range(args.reps):
                geo = scene_mesh_batch(imgs, pts, masks, dev, as_pointcloud=as_pc)
            batch_ms = (time.perf_counter() - t0) * 1e3 / args.reps
            n_out = len(geo['faces']) if not as_pc else len(geo['positions'])
            del geo
            # the whole export
            t0 = time.perf_counter()
            path = get_3D_model_from_scene(outdir, True, scene, min_conf_thr=3.0, as_pointcloud=as_pc)
            export_ms = (time.perf_counter() - t0) * 1e3
            size = os.path.getsize(path)
            os.remove(path)
            row = dict(views=n, H=H, W=W, mode='pointcloud' if as_pc else 'mesh', faces_or_points=n_out, kernels_ms=round(kernel_ms, 3),
                       scene_mesh_batch_ms=round(batch_ms, 1), export_ms=round(export_ms, 1), file_MB=round(size / 2 ** 20, 1))
            if not as_pc:
                with ThreadPoolExecutor(args.threads) as ex:
                    list(ex.map(reference_mesh_view, imgs[:args.threads], host_pts[:args.threads], host_masks[:args.threads]))
                    t0 = time.perf_counter()
                    meshes = list(ex.map(reference_mesh_view, imgs, host_pts, host_masks))
                    cat_meshes(meshes)
                    host_ms = (time.perf_counter() - t0) * 1e3
                row.update(host_threads=args.threads, host_reference_mesh_ms=round(host_ms, 1))
            print(json.dumps(row), flush=True)
            rows.append(row)
        del scene, pts, masks
        torch.cuda.empty_cache()
    os.rmdir(outdir)
    return rows


if __name__ == '__main__':
    main()
