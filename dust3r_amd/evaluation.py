"""Ground-truth evaluation loop: the body of the reference's `test_one_epoch` (dust3r/training.py:342-377) without its logger.

    table = evaluate(model, criterion, batches, device)

`batches` is any iterable of collated (view1, view2) with the reference's keys (`img`, `pts3d`, `camera_pose`, `valid_mask`,
`true_shape`). Every batch goes through `loss_of_one_batch` (forward on the engine, then the criterion on the device: the predictions never
leave HBM); the table holds, for `loss` and every key of the criterion's details, `<key>_avg` = the mean of the per-batch values and
`<key>_med` = their lower median -- what the reference's SmoothedValue reports with an unbounded window. `batches` can be a
`dust3r_amd.datasets.get_data_loader(...)`: its batches are prepared on the GPU and arrive where the criterion reads them. Multi-rank
evaluation is out of scope (ranks would add their per-pair sums and counts, see dust3r_amd/losses.py).

    metrics = evaluate_scene(scene, gt_views)

scores an aligned SCENE against ground-truth views (new; the reference has no such code): the scene is registered to the ground truth, both
sides are voxel-fused at one voxel size and the two clouds are compared by `dust3r_amd.cloud_metrics` (accuracy, completeness, Chamfer,
precision / recall / F-score), all on the GPU. `python -m dust3r_amd.evaluation PRED.ply GT.ply --max-dist D` does the last step on two
PLY files; with --register the predicted cloud is first registered onto the other by Sim(3) ICP (cloud_metrics.register_clouds), which
`evaluate_scene(refine='icp')` does after its own alignment."""
import json
import math
import sys

import numpy as np
import torch

from .inference import loss_of_one_batch


def _call_in_chunks(model, engine_batch):
    """The model called `engine_batch` pairs at a time (the engine's results do not depend on how a batch is cut)."""
    if engine_batch is None:
        return model
    step = max(int(engine_batch), 1)

    def run(view1, view2):
        n = len(view1['img'])
        if n <= step:
            return model(view1, view2)
        cut = lambda view, i: {k: v[i:i + step] for k, v in view.items()}      # noqa: E731
        parts = [model(cut(view1, i), cut(view2, i)) for i in range(0, n, step)]
        return tuple({k: torch.cat([p[side][k] for p in parts]) for k in parts[0][side]} for side in (0, 1))
    return run


@torch.no_grad()
def evaluate(model, criterion, batches, device, symmetrize_batch=True, engine_batch=None):
    history = {}
    run = _call_in_chunks(model, engine_batch)
    for batch in batches:
        value, details = loss_of_one_batch(batch, run, criterion, device, symmetrize_batch=symmetrize_batch, ret='loss')
        for key, v in dict(loss=float(value), **details).items():
            history.setdefault(key, []).append(float(v))
    table = {}
    for key, values in history.items():
        t = torch.tensor(values, dtype=torch.float64)
        table[f'{key}_avg'] = float(t.mean())
        table[f'{key}_med'] = float(t.median())
    return table


# ---- a scene against ground-truth views ------------------------------------------------------------------------------------------------
def _stack_moments(src, tgt, wgt, areas):
    """(17,) weighted Umeyama moments of the padded stacks src -> tgt (n, row, 3) with weights (n, row): one d3r_similarity_moments job per
    view (its h w elements), added in fp64 on the host (the moments are additive). Rows of pad_views / a scene are multiples of 4
    elements, so every row starts on 16 bytes, as the kernel's float4 loads need."""
    from ._lib import check, current_stream, lib, ptr, workspace
    n, dev = len(areas), src.device
    addrs = [[t.data_ptr() + i * t.stride(0) * 4 for i in range(n)] for t in (src, tgt, wgt)]
    if not all(a % 16 == 0 for table in addrs for a in table):
        raise ValueError('evaluate_scene: the stacks must have rows of a multiple of 4 elements (16-byte aligned rows)')
    tables = [torch.tensor(table, dtype=torch.int64).to(dev) for table in addrs]
    npix = torch.tensor(areas, dtype=torch.int32).to(dev)
    out = torch.empty((n, 17), dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        ws = workspace(lib.d3r_similarity_moments_workspace(n, max(areas)), dev)
        check(lib.d3r_similarity_moments(n, ptr(tables[0]), ptr(tables[1]), ptr(tables[2]), ptr(npix), max(areas), ptr(ws), ptr(out), current_stream()),
              'similarity_moments')
    return out.cpu().numpy().sum(axis=0)


def pose_errors(pred_c2w, gt_c2w):
    """(ate_rmse, mean rotation error, max rotation error in degrees) of cam-to-world poses (n, 4, 4) whose rotation blocks are rotations;
    fp64 on the host. The angle between Rp and Rg is 2 asin(||Rp - Rg||_F / (2 sqrt 2)) (||R - I||_F = 2 sqrt 2 sin(angle / 2)): accurate
    near zero, where arccos((trace - 1) / 2) has a noise floor of sqrt(2 eps)."""
    P, G = np.asarray(pred_c2w, np.float64), np.asarray(gt_c2w, np.float64)
    ate = math.sqrt(float(((P[:, :3, 3] - G[:, :3, 3]) ** 2).sum(axis=1).mean()))
    chord = np.sqrt(((P[:, :3, :3] - G[:, :3, :3]) ** 2).sum(axis=(1, 2))) / (2 * math.sqrt(2))
    ang = np.degrees(2 * np.arcsin(np.clip(chord, 0.0, 1.0)))
    return ate, float(ang.mean()), float(ang.max())


@torch.no_grad()
def evaluate_scene(scene, gt_views, align='points', voxel_size=None, max_dist=None, thresholds=None, return_details=False, refine=None,
                   refine_kw=None):
    """The cloud metrics of an aligned scene against ground truth. gt_views: per image a dict with `pts3d` (H, W, 3) world points,
    `valid_mask` (H, W) and optionally `camera_pose` (4, 4) cam-to-world (the keys of dust3r_amd.datasets).
    1. the similarity S that takes the scene into the ground truth's frame. align='points': one weighted Umeyama over all pixels valid on
       both sides (the scene's mask and finite point, the ground truth's valid_mask and finite point; weight 1, the others zeroed with
       weight 0) -- the 17 moments per image by d3r_similarity_moments, added in fp64 on the host, finished by
       bootstrap.similarity_from_moments. align='poses': bootstrap.align_pose_sets of the scene's poses onto the camera_poses. None: identity.
       A (4, 4) array: that similarity.
    2. both sides through viz.fuse_points at one voxel_size (default: the scene's default_voxel_size times the scale of S): the scene's
       masked points, moved by S, weighted by confidence; the ground truth's valid points weighted by ones.
    3. cloud_metrics(pred cloud, gt cloud, max_dist, thresholds); defaults thresholds = (1, 2, 4) voxel_size, max_dist = 16 voxel_size.
    refine='icp': after step 2 the scene's cloud is registered onto the ground truth's by cloud_metrics.register_clouds(pred_cloud, gt_cloud,
    **refine_kw) (default max_dist: this call's; the plane metric takes the normals of the ground-truth cloud), the result is composed into
    S, the scene is moved by the refined S and fused again at the unchanged voxel size, and step 3 scores that cloud. The refinement is
    ACCEPTED when it lowers `overall` (the Chamfer distance it exists to reduce); otherwise everything is that of the first alignment, so
    refining never reports a worse overall. `scale` and the pose errors are those of the S that was kept; the details gain `registration`
    and `refined` (whether it was accepted). None: no refinement.
    With camera_pose in every view: ate_rmse and rot_err_mean_deg / rot_err_max_deg of the scene's poses moved by S (fp64, host).
    return_details: (metrics, details) with every stage's output: similarity (4, 4), scale, pred_pts / gt_pts / pred_mask / gt_mask
    (the padded stacks that were fused), pred_cloud / gt_cloud, d2_pred / idx_pred / d2_gt / idx_gt, voxel_size, max_dist, thresholds."""
    from . import _lib
    from .cloud_metrics import cloud_metrics
    from .cloud_opt.bootstrap import align_pose_sets, similarity_from_moments, split_similarity
    from .utils.padded import pad_views
    from .viz import default_voxel_size, fuse_points
    given = None if align is None or isinstance(align, str) else np.array(align, np.float64)
    if given is None and align not in ('points', 'poses', None):
        raise ValueError(f"evaluate_scene: align is 'points', 'poses' or None (or a (4, 4) similarity), got {align!r}")
    if refine not in ('icp', None):
        raise ValueError(f"evaluate_scene: refine is 'icp' or None, got {refine!r}")
    if scene.device.type != 'cuda':
        raise _lib.D3RError('evaluate_scene runs on the GPU (dust3r_amd has no CPU execution path)')
    _lib.require_device()
    if scene.imgs is None:
        raise ValueError('evaluate_scene needs the scene images: scene.imgs is None (the views given to global_aligner had no "img")')
    if len(gt_views) != scene.n_imgs:
        raise ValueError(f'evaluate_scene: {len(gt_views)} ground-truth views for a scene of {scene.n_imgs} images')
    dev, shapes = scene.device, [tuple(s) for s in scene.imshapes]
    areas = [h * w for h, w in shapes]
    pred = scene.get_pts3d(raw=True).detach().contiguous()
    row = pred.shape[1]
    pred_mask = scene.get_masks(raw=True)
    gt = pad_views([v['pts3d'] for v in gt_views], dev, torch.float32, (3,), row, shapes, 'evaluate_scene: ground-truth pointmap')
    gt_mask = pad_views([v['valid_mask'] for v in gt_views], dev, torch.uint8, (), row, shapes, 'evaluate_scene: valid_mask') != 0
    has_poses = all(v.get('camera_pose') is not None for v in gt_views)
    gt_poses = np.stack([np.asarray(torch.as_tensor(v['camera_pose']).detach().cpu(), np.float64) for v in gt_views]) if has_poses else None
    poses = scene.get_im_poses().detach().double().cpu().numpy()
    if given is not None:
        from .cloud_metrics import similarity_parts
        similarity_parts(given)
        S = given
    elif align == 'points':
        both = pred_mask & gt_mask & torch.isfinite(pred).all(dim=-1) & torch.isfinite(gt).all(dim=-1)
        wgt = both.float().contiguous()
        moments = _stack_moments(torch.where(both[..., None], pred, 0.0).contiguous(), torch.where(both[..., None], gt, 0.0).contiguous(), wgt, areas)
        if not moments[0] > 0:
            raise ValueError('evaluate_scene: no pixel is valid on both sides; nothing to register')
        S = similarity_from_moments(moments)
    elif align == 'poses':
        if not has_poses:
            raise ValueError("evaluate_scene: align='poses' needs camera_pose in every ground-truth view")
        S = align_pose_sets(poses, gt_poses)
    else:
        S = np.eye(4)
    def move(S):
        A = torch.tensor(S[:3, :3], dtype=torch.float32, device=dev)
        return (pred @ A.T + torch.tensor(S[:3, 3], dtype=torch.float32, device=dev)).contiguous()
    scale, R, t = split_similarity(S)
    aligned = move(S) if align is not None else pred
    if voxel_size is None:
        voxel_size = default_voxel_size(scene.get_depthmaps(raw=True), areas, scene.get_focals()) * scale
    thresholds = [k * voxel_size for k in (1, 2, 4)] if thresholds is None else list(thresholds)
    max_dist = 16 * voxel_size if max_dist is None else max_dist
    pred_cloud = fuse_points(scene.imgs, aligned, pred_mask, scene._im_conf, voxel_size, dev, to_host=False)
    gt_cloud = fuse_points(scene.imgs, gt, gt_mask, None, voxel_size, dev, to_host=False)
    details = {}
    metrics = cloud_metrics(pred_cloud, gt_cloud, max_dist, thresholds, details=details)
    if refine == 'icp':
        from .cloud_metrics import register_clouds
        registration = register_clouds(pred_cloud, gt_cloud, **dict(dict(max_dist=max_dist), **(refine_kw or {})))
        S_new = registration.similarity @ S
        moved = move(S_new)
        cloud_new = fuse_points(scene.imgs, moved, pred_mask, scene._im_conf, voxel_size, dev, to_host=False)
        details_new = {}
        metrics_new = cloud_metrics(cloud_new, gt_cloud, max_dist, thresholds, details=details_new)
        accepted = metrics_new['overall'] < metrics['overall']             # False for a NaN on either side: the first alignment stays
        if accepted:
            S, aligned, pred_cloud, metrics, details = S_new, moved, cloud_new, metrics_new, details_new
            scale, R, t = split_similarity(S)
        details.update(registration=registration, refined=accepted)
    metrics.update(voxel_size=float(voxel_size), max_dist=float(max_dist), scale=scale)
    if has_poses:
        moved = poses.copy()
        moved[:, :3, :3] = R @ poses[:, :3, :3]
        moved[:, :3, 3] = poses[:, :3, 3] @ S[:3, :3].T + S[:3, 3]
        metrics['ate_rmse'], metrics['rot_err_mean_deg'], metrics['rot_err_max_deg'] = pose_errors(moved, gt_poses)
    if not return_details:
        return metrics
    details.update(similarity=S, scale=scale, pred_pts=aligned, gt_pts=gt, pred_mask=pred_mask, gt_mask=gt_mask, pred_cloud=pred_cloud,
                   gt_cloud=gt_cloud, voxel_size=float(voxel_size), max_dist=float(max_dist), thresholds=[float(x) for x in thresholds])
    return metrics, details


def main(argv=None):
    """python -m dust3r_amd.evaluation PRED.ply GT.ply --max-dist D [--thresholds T ...]: the dict of cloud_metrics as one JSON line.
    --register [--init FILE] [--rigid] [--metric point|plane] [--register-dist D1 D2 ...]: PRED is first registered onto GT by
    cloud_metrics.register_clouds (stages --register-dist, default 4 D, 2 D, D) and moved; the line gains similarity (4 x 4, row-major
    lists), registration_rmse and registration_pairs. --global [--feature-cell C] [--ransac-iters H] [--seed S] (with --register, instead of
    --init): the registration starts from cloud_metrics.global_registration -- FPFH features, exhaustive matching and a Sim(3) RANSAC of H
    hypotheses, with the PLY files' normals when they have them -- so PRED may be rotated and scaled by anything; the line gains
    global_similarity, global_inliers and global_matches."""
    args = parse_args(argv)
    from .cloud_metrics import cloud_metrics
    from .export import read_ply
    plys = [read_ply(p) for p in (args.pred, args.gt)]
    clouds = [p['positions'] for p in plys]
    thresholds = [args.max_dist / 16, args.max_dist / 8, args.max_dist / 4] if args.thresholds is None else args.thresholds
    if not args.register:
        print(json.dumps(cloud_metrics(clouds[0], clouds[1], args.max_dist, thresholds)))
        return 0
    from .cloud_metrics import register_clouds, transform_points
    init = None if args.init is None else np.loadtxt(args.init, dtype=np.float64).reshape(4, 4)
    stages = [4 * args.max_dist, 2 * args.max_dist, args.max_dist] if args.register_dist is None else args.register_dist
    details = {}
    if args.global_register:
        init = 'global'
        global_kw = dict(src_normals=plys[0].get('normals'), dst_normals=plys[1].get('normals'), cell=args.feature_cell, n_hyp=args.ransac_iters,
                         seed=args.seed)
    reg = register_clouds(clouds[0], clouds[1], stages, init=init, with_scale=not args.rigid, metric=args.metric,
                          global_kw=global_kw if args.global_register else None, details=details)
    moved, _ = transform_points(clouds[0], reg.similarity)
    out = cloud_metrics(moved, clouds[1], args.max_dist, thresholds)
    out.update(similarity=reg.similarity.tolist(), registration_rmse=reg.rmse, registration_pairs=reg.n_pairs)
    if args.global_register:
        g = details['global']
        out.update(global_similarity=g.similarity.tolist(), global_inliers=g.n_inliers, global_matches=g.n_matches)
    print(json.dumps(out))
    return 0


def parse_args(argv=None):
    """the command line of `main`"""
    import argparse
    parser = argparse.ArgumentParser(prog='python -m dust3r_amd.evaluation', description='cloud-to-cloud metrics of two PLY files on the GPU')
    parser.add_argument('pred')
    parser.add_argument('gt')
    parser.add_argument('--max-dist', type=float, required=True, help='distances beyond it are outliers')
    parser.add_argument('--thresholds', type=float, nargs='*', default=None, help='precision / recall distances (default: max-dist / 16, / 8, / 4)')
    parser.add_argument('--register', action='store_true', help='register PRED onto GT by Sim(3) ICP before scoring')
    parser.add_argument('--init', default=None, help='a text file with the 4 x 4 similarity the registration starts from')
    parser.add_argument('--rigid', action='store_true', help='keep the scale of --init (no scale unknown)')
    parser.add_argument('--metric', choices=('point', 'plane'), default='plane', help='the residual of the registration')
    parser.add_argument('--register-dist', type=float, nargs='+', default=None, help='the pair gates of the stages, coarse to fine (default: 4, 2, 1 max-dist)')
    parser.add_argument('--global', dest='global_register', action='store_true',
                        help='start the registration from a global one (FPFH features, Sim(3) RANSAC): no --init needed')
    parser.add_argument('--feature-cell', type=float, default=None, help='the cell of the feature clouds of --global (default: 0.1 of each cloud\'s size)')
    parser.add_argument('--ransac-iters', type=int, default=65536, help='the hypotheses of the RANSAC of --global')
    parser.add_argument('--seed', type=int, default=0, help='the seed of the RANSAC of --global')
    args = parser.parse_args(argv)
    if not args.register and (args.init is not None or args.rigid or args.register_dist is not None or args.metric != 'plane'):
        parser.error('--init, --rigid, --metric and --register-dist need --register')
    if args.global_register and (not args.register or args.init is not None):
        parser.error('--global needs --register and excludes --init')
    if not args.global_register and (args.feature_cell is not None or args.ransac_iters != 65536 or args.seed != 0):
        parser.error('--feature-cell, --ransac-iters and --seed need --global')
    return args


if __name__ == '__main__':
    sys.exit(main())
