"""Times the 2-D tracks (FusedCloud.build_tracks, csrc/tracks.hip) on the 100-view 512 x 384 scene of tools/fuse_speed.py and its fused cloud:
- calls: device events around d3r_cloud_tracks_count and d3r_cloud_tracks_fill (viz.cloud_tracks' own timing hook), medians after warm-up,
  the pairs (point, view) tested per second and the mean track length; viz.fuse_points on the same scene in the same run, so that the
  added cost is stated against it;
- the whole build_tracks call on the host clock (to host arrays and left on the device), and write_colmap with and without tracks to /dev/shm;
- the host figure: the numpy restatement of tests/test_tracks_cpu.py on --threads host threads over every --host-stride-th point of the
  cloud in blocks (the whole cloud would need the (views, points) tables of the restatement in memory), compared with the device result.
Per-pass device times (count / fill / sort / link) come from a kernel trace taken in a run of its own:

    python tools/tracks_speed.py [--views 100] [--reps 5] [--threads 16]            # the rows above, one JSON line per row
    <profiler> --kernel-trace ... -- python tools/tracks_speed.py --profile-run      # three calls after warm-up, nothing else
    python tools/tracks_speed.py --summarise <kernel_trace.csv>                      # per pass, median over the calls"""
import argparse
import csv
import json
import os
import statistics
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests'), os.path.join(ROOT, 'tools')]

import numpy as np  # noqa: E402

PASSES = ('count', 'fill', 'sort', 'link')


def pass_of(kernel_name, last):
    """the pass a kernel of a tracks call belongs to, from its (mangled or demangled) name; a scan belongs to the pass before it"""
    if 'tracks_walk' in kernel_name:
        return 'fill' if ('ILb1E' in kernel_name or '<true' in kernel_name.replace(' ', '')) else 'count'
    if 'tracks_total' in kernel_name:
        return 'count'
    if 'fuse_hist' in kernel_name or 'fuse_scatter' in kernel_name:
        return 'sort'
    if 'tracks_image_off' in kernel_name or 'tracks_point2d' in kernel_name:
        return 'link'
    if 'fuse_scan' in kernel_name:
        return last
    return None


def summarise(path):
    """Groups the dispatches of a kernel trace into calls (a call starts at the counting walk) and passes; prints the medians over the calls."""
    rows = sorted(csv.DictReader(open(path)), key=lambda r: int(r['Start_Timestamp']))
    calls, cur = [], None
    for r in rows:
        name = r['Kernel_Name']
        p = pass_of(name, cur['last'] if cur else None)
        if p == 'count' and 'tracks_walk' in name:
            cur = dict(passes={k: 0.0 for k in PASSES}, last=None, launches=0)
            calls.append(cur)
        if cur is None or p is None:      # (the scene and its cloud are made before the first call: --profile-run runs nothing else after it)
            continue
        cur['passes'][p] += (int(r['End_Timestamp']) - int(r['Start_Timestamp'])) / 1e3
        cur['last'] = p
        cur['launches'] += 1
    calls = [c for c in calls if c['passes']['link'] > 0]
    if not calls:
        raise SystemExit(f'{path}: no complete tracks call in the trace')
    out = dict(calls=len(calls), launches_per_call=calls[-1]['launches'])
    for k in PASSES:
        out[f'{k}_us'] = round(statistics.median(c['passes'][k] for c in calls), 1)
    out['total_us'] = round(statistics.median(sum(c['passes'].values()) for c in calls), 1)
    print(json.dumps(out), flush=True)
    return out


def median_ms(fn, reps, sync):
    ts = []
    for _ in range(reps):
        sync()
        t0 = time.perf_counter()
        fn()
        sync()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--views', type=int, default=100)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--threads', type=int, default=16)
    ap.add_argument('--host-stride', type=int, default=16, help='the host restatement runs on every N-th point of the cloud')
    ap.add_argument('--profile-run', action='store_true')
    ap.add_argument('--summarise', default=None, metavar='CSV')
    ap.add_argument('--skip-host', action='store_true', help='leave the numpy restatement out')
    args = ap.parse_args()
    if args.summarise:
        return summarise(args.summarise)
    import torch
    torch.set_num_threads(args.threads)
    from dust3r_amd import _lib
    from dust3r_amd.export import write_colmap
    from dust3r_amd.viz import cloud_tracks, fuse_points, track_cameras
    from glb_speed import make_scene
    _lib.require_device()
    dev = torch.device('cuda:0')
    n, H, W = args.views, 384, 512
    scene = make_scene(n, H, W, dev)
    sync = torch.cuda.synchronize
    with torch.no_grad():
        scene.min_conf_thr = float(scene.conf_trf(torch.tensor(3.0)))
        cloud = scene.fuse(to_host=False)
        pts, mask, weight = scene.get_pts3d(raw=True).contiguous(), scene.get_masks(raw=True).to(torch.uint8), scene._im_conf
        K, c2w = scene.get_intrinsics(), scene.get_im_poses()

    def tracks(timing=None, to_host=False):
        return cloud_tracks(cloud.positions, pts, mask, weight, K, c2w, scene.imshapes, cloud.voxel_size, device=dev, to_host=to_host, timing=timing)

    if args.profile_run:
        for _ in range(5):
            tracks()
        sync()
        return None

    with torch.no_grad():
        for _ in range(2):
            got = tracks()
        timings = []
        for _ in range(args.reps):
            t = {}
            tracks(timing=t)
            timings.append(t)
        count_ms, fill_ms = (statistics.median(t[k] for t in timings) for k in ('count', 'fill'))
        fuse_ms = median_ms(lambda: fuse_points(scene.imgs, pts, mask, weight, cloud.voxel_size, dev, to_host=False), args.reps, sync)
        stats = got.stats()
        m, T = len(cloud), len(got)
        print(json.dumps(dict(row='calls', views=n, H=H, W=W, points=m, max_dist=cloud.voxel_size, observations=T, mean_track_length=round(stats['mean_track_length'], 3),
                              unobserved=round(stats['unobserved'], 4), mean_error_px=round(stats['mean_error'], 4), median_error_px=round(stats['median_error'], 4),
                              count_ms=round(count_ms, 3), fill_ms=round(fill_ms, 3), pairs=m * n, pairs_per_s_count=round(m * n / count_ms * 1e3, -6),
                              workspace_MB=round(int(_lib.lib.d3r_cloud_tracks_workspace_bytes(max(T, 1))) / 2 ** 20, 1),
                              fuse_points_device_ms=round(fuse_ms, 2))), flush=True)

        # the whole call, and the files
        device_call_ms = median_ms(lambda: cloud.build_tracks(scene), args.reps, sync)
        host_cloud = scene.fuse()
        host_call_ms = median_ms(lambda: host_cloud.build_tracks(scene), args.reps, sync)
        with_tracks = host_cloud.build_tracks(scene)
    outdir = tempfile.mkdtemp(dir='/dev/shm' if os.path.isdir('/dev/shm') else tempfile.gettempdir())
    row = dict(row='build_tracks', views=n, build_tracks_on_device_ms=round(device_call_ms, 1), build_tracks_to_host_ms=round(host_call_ms, 1))
    for name, c in (('write_colmap_without_tracks', host_cloud), ('write_colmap_with_tracks', with_tracks)):
        t0 = time.perf_counter()
        files = write_colmap(os.path.join(outdir, 'colmap'), scene, c, write_images=False)
        row[name + '_ms'] = round((time.perf_counter() - t0) * 1e3, 1)
        row[name + '_MB'] = round(sum(os.path.getsize(f) for f in files) / 2 ** 20, 1)
        for f in files:
            os.remove(f)
    print(json.dumps(row), flush=True)

    if not args.skip_host:
        from test_tracks_cpu import restated_tracks
        with torch.no_grad():
            host_pts = [p.cpu().numpy() for p in scene.get_pts3d()]
            host_msk = [m.cpu().numpy() for m in scene.get_masks()]
            host_w = [c.cpu().numpy() for c in scene.im_conf]
            cams = track_cameras(K, c2w)
        sub = np.ascontiguousarray(host_cloud.positions[::args.host_stride])
        blocks = np.array_split(np.arange(len(sub)), max(1, min(4 * args.threads, len(sub) // 4096 + 1)))
        t0 = time.perf_counter()
        with ThreadPoolExecutor(args.threads) as ex:
            parts = list(ex.map(lambda b: restated_tracks(sub[b], host_pts, host_msk, host_w, cams, host_cloud.voxel_size), blocks))
        host_ms = (time.perf_counter() - t0) * 1e3
        tr = with_tracks.tracks
        picked = np.repeat(np.arange(len(host_cloud)) % args.host_stride == 0, tr.lengths)
        same = all(bool(np.array_equal(np.concatenate([p[k] for p in parts]), getattr(tr, k)[picked])) for k in ('view', 'pixel', 'err2'))
        same = same and bool(np.array_equal(np.concatenate([np.diff(p['point_offsets']) for p in parts]), tr.lengths[::args.host_stride]))
        print(json.dumps(dict(row='host', host_threads=args.threads, host_points=len(sub), host_pairs=len(sub) * n, host_restatement_ms=round(host_ms, 1),
                              pairs_per_s_host=round(len(sub) * n / host_ms * 1e3, -5), equals_restatement=same)), flush=True)
    return None


if __name__ == '__main__':
    main()
