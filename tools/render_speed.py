"""Times the headless renderer (csrc/render.hip, viz.render_batch) on the 100-view 512 x 384 scene of tools/glb_speed.py, frames of 1024 x 768:
- device: device events around viz.render_batch with the outputs left on the GPU -- the device time of the call: the clear, the draw and
  resolve kernels, and the wrapper's small uploads (poses, intrinsics) and allocations; not a per-kernel trace. One frame and a 36-frame
  turntable in one call; the point cloud (every pixel of every view), the mesh of the GLB export, and the point cloud with the camera
  glyphs that scene.show() and render_turntable add (48 slivers per camera: the wave path of the triangle kernel);
- call: host clock around viz.render_batch, geometry resident on the GPU (device tensors in), host images out. Building the geometry
  (scene_mesh_batch, the colours' upload) is not part of it: `mesh_build_ms` gives scene_mesh_batch(to_host=False) on its own;
- 36 one-frame calls against the one 36-frame call, ALTERNATED in the same run (the reason for the camera dimension): medians, the
  quartiles of each, and in how many of the rounds the one call was the faster of the pair;
- the share of atomics that the load in front of the atomic skipped (the counting build of the kernels, one extra run);
- host: the numpy restatement's vectorised point path (tests/test_render_cpu.py: restated_project + np.minimum.at) on a pool of host
  threads, one chunk of points per task and a final minimum over the tasks' buffers.
Each figure is the median of --reps runs after warm-up; a one-frame point-cloud call lasts a fraction of a millisecond, so its figures
carry the launch and wrapper overheads and are no bandwidth measurement.

    python tools/render_speed.py [--views 100] [--frames 36] [--reps 15] [--threads 16] [--no-mesh] [--no-host]"""
import argparse
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests'), os.path.join(ROOT, 'tools')]

import numpy as np  # noqa: E402
import torch  # noqa: E402

from dust3r_amd import _lib  # noqa: E402
from dust3r_amd.viz import SceneViz, intrinsics_rows, render_batch, scene_mesh_batch, turntable_poses, world_to_cam  # noqa: E402


def median_ms(fn, reps, device_events):
    fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        if device_events:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            times.append(e0.elapsed_time(e1))
        else:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            times.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(times))


def alternated(one_call, many_calls, reps):
    """the two variants of the turntable in turns, host clock: medians, quartiles, and the rounds the one call won"""
    one_call(), many_calls()
    a, b = [], []
    for _ in range(reps):
        for fn, out in ((one_call, a), (many_calls, b)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            out.append((time.perf_counter() - t0) * 1e3)
    q = lambda v: [round(float(x), 3) for x in np.percentile(v, [25, 50, 75])]      # noqa: E731
    return q(a), q(b), int(sum(x <= y for x, y in zip(a, b)))


def host_points(pts, mask, w2c, intr, near, size, threads):
    from test_render_cpu import EMPTY, INVALID, restated_project
    W, H = size
    chunks = np.array_split(np.arange(len(pts)), threads)

    def work(idx):
        r = restated_project(pts[idx], w2c, intr, near)
        keys = np.full((H, W), EMPTY, dtype=np.uint64)
        use = (r['zq'] != INVALID) & mask[idx]
        bx, by = (r['sx'][use] + 8) // 16, (r['sy'][use] + 8) // 16
        k = (r['zq'][use].astype(np.uint64) << np.uint64(32)) | idx[use].astype(np.uint64)
        inside = (bx >= 0) & (bx < W) & (by >= 0) & (by < H)
        np.minimum.at(keys, (by[inside], bx[inside]), k[inside])
        return keys
    t0 = time.perf_counter()
    with ThreadPoolExecutor(threads) as ex:
        keys = np.minimum.reduce(list(ex.map(work, chunks)))
    return (time.perf_counter() - t0) * 1e3, keys


def main():
    from glb_speed import make_scene
    from dust3r_amd.viz import CAM_COLORS, auto_cam_size
    ap = argparse.ArgumentParser()
    ap.add_argument('--views', type=int, default=100)
    ap.add_argument('--frames', type=int, default=36)
    ap.add_argument('--reps', type=int, default=15)
    ap.add_argument('--threads', type=int, default=16)
    ap.add_argument('--no-mesh', action='store_true')
    ap.add_argument('--no-host', action='store_true')
    args = ap.parse_args()
    _lib.require_device()
    dev = torch.device('cuda:0')
    H, W, size, focal, near = 384, 512, (1024, 768), 1.1 * 768, 0.05
    scene = make_scene(args.views, H, W, dev)
    with torch.no_grad():
        scene.min_conf_thr = float(scene.conf_trf(torch.tensor(3.0)))
        masks = scene.get_masks()
        pts3d = scene.get_pts3d(raw=True).contiguous()
        cams2world = scene.get_im_poses().cpu().numpy()
        focals = scene.get_focals().cpu().numpy().reshape(-1)
    viz = SceneViz(dev).add_pointcloud([p for p in pts3d], scene.imgs, masks)
    cloud = viz.flat_arrays()
    bounds = viz.bounds()
    poses = turntable_poses(bounds, args.frames, focal, size)
    intr = intrinsics_rows(focal, args.frames, size)
    viz.add_cameras(cams2world, focals, imsizes=scene.imsizes, colors=[CAM_COLORS[i % len(CAM_COLORS)] for i in range(args.views)],
                    cam_size=auto_cam_size(cams2world))
    modes = [('pointcloud', cloud, len(cloud['points'])), ('pointcloud+glyphs', viz.flat_arrays(), len(cloud['points']))]
    build_ms = None
    if not args.no_mesh:
        def build():
            geo = scene_mesh_batch(scene.imgs, pts3d, masks, dev, to_host=False)
            return SceneViz(dev).add_mesh(geo['positions'], geo['faces'], geo['colors']).flat_arrays()
        build_ms = round(median_ms(build, 5, False), 2)
        mesh = build()
        modes.append(('mesh', mesh, len(mesh['faces'])))
    for name, g, n_prim in modes:
        def call(p, i, **kw):
            return render_batch(p, i, size, dev, near=near, **g, **kw)
        row = dict(mode=name, views=args.views, primitives=n_prim, size=list(size), frames=args.frames, reps=args.reps)
        if name == 'mesh':
            row['mesh_build_ms'] = build_ms
        if g['faces'] is not None and name != 'mesh':
            row['glyph_faces'] = len(g['faces'])
        # read floor of one frame: positions 12 B (+ mask 1 B + colour 4 B at the resolve, bounded by 15 B) per point; 12 B of indices and
        # 36 B of gathered positions per face
        floor_bytes = n_prim * (48 if name == 'mesh' else 15)
        row['device_1_ms'] = round(median_ms(lambda: call(poses[:1], intr[:1], to_host=False), args.reps, True), 3)
        row['device_F_ms'] = round(median_ms(lambda: call(poses, intr, to_host=False), args.reps, True), 3)
        row['call_1_ms'] = round(median_ms(lambda: call(poses[:1], intr[:1]), args.reps, False), 3)
        qa, qb, wins = alternated(lambda: call(poses, intr), lambda: [call(poses[k:k + 1], intr[k:k + 1]) for k in range(args.frames)],
                                  args.reps if name != 'mesh' else max(5, args.reps // 3))
        row.update(call_F_ms=qa[1], call_F_quartiles=qa, F_single_calls_ms=qb[1], F_single_calls_quartiles=qb, one_call_faster_in_rounds=wins,
                   batched_not_slower=bool(qa[1] <= qb[1]))
        row['read_floor_GB'] = round(floor_bytes / 1e9, 3)
        row['read_GBps_1'] = round(floor_bytes / 1e9 / (row['device_1_ms'] / 1e3), 1)
        row['hbm_floor_fraction_1'] = round(row['read_GBps_1'] / 8000, 4)          # of the 8 TB/s HBM3E peak
        cand, issued = call(poses[:1], intr[:1], stats=True)['stats']
        row.update(candidates_1=cand, atomics_issued_1=issued, atomics_skipped_share_1=round(1 - issued / max(cand, 1), 4))
        cand, issued = call(poses, intr, stats=True, to_host=False)['stats']
        row.update(atomics_skipped_share_F=round(1 - issued / max(cand, 1), 4), atomic_GBps_1=round(row['atomics_issued_1'] * 8 / 1e9 / (row['device_1_ms'] / 1e3), 1))
        if name == 'pointcloud' and not args.no_host:
            got = call(poses[:1], intr[:1], return_keys=True)['keys'][0].view(np.uint64)
            ms, keys = host_points(g['points'].cpu().numpy(), g['point_mask'].cpu().numpy().astype(bool), world_to_cam(poses[:1])[0],
                                   intr[0].astype(np.float64), near, size, args.threads)
            row.update(host_threads=args.threads, host_numpy_points_1_ms=round(ms, 1),
                       host_pixels_differing=int((got != keys).sum()))       # fp64 against fp32 snapping: a few pixels may differ
        print(json.dumps(row), flush=True)


if __name__ == '__main__':
    main()
