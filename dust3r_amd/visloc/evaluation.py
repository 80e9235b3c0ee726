"""Mirror of the reference's `dust3r_visloc/evaluation.py` (aggregate_stats, get_pose_error, export_results) without `quaternion` and
`roma`: the rotation distance and the rotation -> quaternion conversion are written out in numpy / torch here. aggregate_stats gives the same text; export_results writes
the same format, with quaternions in the w >= 0 convention (numpy-quaternion takes them from an eigen-decomposition and leaves the sign
to it, so a line can differ from the reference's in sign and in the last digits while describing the same rotation)."""
import os

import numpy as np
import torch

THRESHOLDS = [(0.1, 1), (0.25, 2), (0.5, 5), (5, 10)]       # (metres, degrees) of the accuracy columns


def aggregate_stats(info_str, pose_errors, angular_errors):
    """'<info>: <n> images - median_pos_error=..., median_angular_error=...' then '  - acc@<t>m,<a>deg=<percent>' per threshold."""
    median_pos_error = np.median(pose_errors)
    median_angular_error = np.median(angular_errors)
    out_str = f'{info_str}: {len(pose_errors)} images - {median_pos_error=}, {median_angular_error=}'
    for trl_thr, ang_thr in THRESHOLDS:
        hits = sum(bool((p < trl_thr) and (a < ang_thr)) for p, a in zip(pose_errors, angular_errors))
        metric = f'acc@{trl_thr:g}m,{ang_thr}deg'
        out_str += f'  - {metric:12s}={float(100 * hits / len(pose_errors)):.3f}'
    return out_str


def rotation_angle(R1, R2):
    """Geodesic distance (radians) between rotation matrices: acos((trace(R1^T R2) - 1) / 2), clamped to [-1, 1]."""
    M = R1.transpose(-2, -1) @ R2
    cos = 0.5 * (M[..., 0, 0] + M[..., 1, 1] + M[..., 2, 2] - 1.0)
    return torch.acos(torch.clamp(cos, -1.0, 1.0))


def get_pose_error(pr_camtoworld, gt_cam_to_world):
    """(translation error, rotation error in degrees) between two cam2world 4x4 matrices, as 0-d float64 tensors."""
    pr = torch.as_tensor(np.asarray(pr_camtoworld, dtype=np.float64))
    gt = torch.as_tensor(np.asarray(gt_cam_to_world, dtype=np.float64))
    abs_transl_error = torch.linalg.norm(pr[:3, 3] - gt[:3, 3])
    abs_angular_error = rotation_angle(pr[:3, :3], gt[:3, :3]) * 180 / np.pi
    return abs_transl_error, abs_angular_error


def rotation_to_quaternion(R):
    """Unit quaternion (w, x, y, z) of a rotation matrix, w >= 0 (Shepperd's method: the largest of the four diagonal forms)."""
    R = np.asarray(R, dtype=np.float64)
    tr = R[0, 0] + R[1, 1] + R[2, 2]
    cands = [tr, R[0, 0], R[1, 1], R[2, 2]]
    k = int(np.argmax(cands))
    if k == 0:
        s = 2.0 * np.sqrt(1.0 + tr)
        q = [0.25 * s, (R[2, 1] - R[1, 2]) / s, (R[0, 2] - R[2, 0]) / s, (R[1, 0] - R[0, 1]) / s]
    elif k == 1:
        s = 2.0 * np.sqrt(1.0 + R[0, 0] - R[1, 1] - R[2, 2])
        q = [(R[2, 1] - R[1, 2]) / s, 0.25 * s, (R[0, 1] + R[1, 0]) / s, (R[0, 2] + R[2, 0]) / s]
    elif k == 2:
        s = 2.0 * np.sqrt(1.0 + R[1, 1] - R[0, 0] - R[2, 2])
        q = [(R[0, 2] - R[2, 0]) / s, (R[0, 1] + R[1, 0]) / s, 0.25 * s, (R[1, 2] + R[2, 1]) / s]
    else:
        s = 2.0 * np.sqrt(1.0 + R[2, 2] - R[0, 0] - R[1, 1])
        q = [(R[1, 0] - R[0, 1]) / s, (R[0, 2] + R[2, 0]) / s, (R[1, 2] + R[2, 1]) / s, 0.25 * s]
    q = np.array(q)
    q /= np.linalg.norm(q)
    return -q if q[0] < 0 else q


def export_results(output_dir, xp_label, query_names, poses_pred):
    """<output_dir>/<xp_label>_results.txt (full query names) and _ltvl.txt (base names): one line per query,
    'name qw qx qy qz tx ty tz' of the world -> camera pose (identity for a failed query). Nothing when output_dir is None."""
    if output_dir is None:
        return
    os.makedirs(output_dir, exist_ok=True)
    lines, lines_ltvl = [], []
    for name, c2w in zip(query_names, poses_pred):
        w2c = np.eye(4) if c2w is None else np.linalg.inv(c2w)
        pose = rotation_to_quaternion(w2c[:3, :3]).tolist() + w2c[:3, 3].flatten().tolist()
        lines.append(' '.join(str(v) for v in [name] + pose) + '\n')
        lines_ltvl.append(' '.join(str(v) for v in [os.path.basename(name)] + pose) + '\n')
    with open(os.path.join(output_dir, xp_label + '_results.txt'), 'wt') as f:
        f.write(''.join(lines))
    with open(os.path.join(output_dir, xp_label + '_ltvl.txt'), 'wt') as f:
        f.write(''.join(lines_ltvl))
