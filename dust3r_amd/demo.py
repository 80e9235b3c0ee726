"""The export stage of the reference's gradio demo (dust3r/demo.py:66-132): `get_3D_model_from_scene` and `_convert_scene_output_to_glb`,
same signatures, same return value (the path of outdir/scene.glb), without trimesh. The mesh or point cloud is built on the GPU for all
views in one call (viz.scene_mesh_batch), the camera glyphs on the host (viz.scene_camera_geometry), and glb.GlbBuilder writes a glTF 2.0
binary:
- root node: matrix inv(cams2world[0] @ OPENGL @ rot_y180) (the reference's scene.apply_transform), every other node its child; positions
  are the untransformed fp32 points;
- the scene: a TRIANGLES primitive (indices, POSITION, COLOR_0 = the face colours averaged onto the vertices) or, with as_pointcloud, a
  POINTS primitive (POSITION, COLOR_0); left out when nothing is valid;
- one wireframe per camera and, unless transparent_cams, its picture on a textured quad (PNG of np.uint8(255 * img)).
`render_turntable` (new; the reference has no headless output) draws the same scene into PNG frames on the GPU instead.

The function users call, `get_reconstructed_scene` (dust3r/demo.py:135-186): files -> load_images -> make_pairs -> inference -> global_aligner ->
compute_global_alignment -> get_3D_model_from_scene, and the rgb / depth / confidence gallery it returns (`scene_gallery`: one GPU call
for all images, csrc/gallery.hip, no matplotlib). `scenegraph_options` is the rule of set_scenegraph_options as plain data, and
`python -m dust3r_amd.demo` the command line in place of the gradio page; its --fuse / --ply / --colmap (new) also write the fused cloud of
`scene.fuse()` as scene.ply and as a COLMAP model (`write_fused`, dust3r_amd/export.py); --fuse_normals / --fuse_outliers add normals and
statistical outlier removal, --fuse_clusters / --fuse_keep_largest density clustering and the removal of all but the largest clusters,
--fuse_planes / --fuse_upright the dominant planes and the cloud stood on its ground."""
import argparse
import copy
import json
import math
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from . import _lib
from .cloud_opt import GlobalAlignerMode, global_aligner
from .glb import ARRAY_BUFFER, FLOAT, POINTS, TRIANGLES, GlbBuilder
from .image_pairs import make_pairs
from .inference import inference
from .utils.device import host_tensor, to_numpy, usable_cpus
from .utils.image import IMAGE_EXTENSIONS, load_images
from .viz import CAM_COLORS, OPENGL, SceneViz, auto_cam_size, scene_camera_geometry, scene_mesh_batch, turntable_poses


def _device_of(*seqs):
    for seq in seqs:
        items = [seq] if isinstance(seq, torch.Tensor) else seq
        for t in items:
            if isinstance(t, torch.Tensor) and t.is_cuda:
                return t.device
    return torch.device('cuda', torch.cuda.current_device())


def _png(image):
    import io
    import PIL.Image
    image = np.asarray(image)
    if image.dtype != np.uint8:
        image = np.uint8(255 * image)          # add_scene_cam (viz.py:252-253): truncation
    buf = io.BytesIO()
    PIL.Image.fromarray(image).save(buf, format='PNG')
    return buf.getvalue()


def _rgba(color):
    return np.array(list(np.asarray(color, dtype=np.uint8).reshape(-1)[:3]) + [255], dtype=np.uint8)


def _convert_scene_output_to_glb(outdir, imgs, pts3d, mask, focals, cams2world, cam_size=0.05,
                                 cam_color=None, as_pointcloud=False,
                                 transparent_cams=False, silent=False):
    assert len(pts3d) == len(mask) <= len(imgs) <= len(cams2world) == len(focals)
    device = _device_of(pts3d, mask)
    imgs = to_numpy(imgs)
    focals = to_numpy(focals)
    cams2world = to_numpy(cams2world)

    geo = scene_mesh_batch(imgs[:len(mask)], pts3d, mask, device, as_pointcloud=as_pointcloud)
    outfile = os.path.join(outdir, 'scene.glb')
    if not silent:
        print('(exporting 3D scene to', outfile, ')')
    write_scene_glb(outfile, geo, imgs, focals, cams2world, cam_size=cam_size, cam_color=cam_color, as_pointcloud=as_pointcloud,
                    transparent_cams=transparent_cams)
    return outfile


def write_scene_glb(outfile, geo, imgs, focals, cams2world, cam_size=0.05, cam_color=None, as_pointcloud=False, transparent_cams=False):
    """The host half of the export: `geo` (the dict of viz.scene_mesh_batch) and one camera per row of cams2world (host arrays) into a .glb
    file. Raises ValueError before the file is created when it would not fit the format's uint32 length."""
    glb = GlbBuilder()
    root = np.linalg.inv(cams2world[0] @ OPENGL @ _rot_y180())
    glb.doc['scenes'][0]['nodes'] = [glb.node(name='world', matrix=[float(v) for v in root.T.reshape(-1)])]     # node 0, column-major
    children = []
    color_mat = glb.material(baseColorFactor=[1.0, 1.0, 1.0, 1.0], roughnessFactor=1.0)
    if geo['bounds'] is not None:
        attrs = dict(POSITION=glb.positions(geo['positions'], bounds=geo['bounds']), COLOR_0=glb.colors(geo['colors']))
        if as_pointcloud:
            mesh = glb.mesh(attrs, mode=POINTS, material=color_mat)
        else:
            mesh = glb.mesh(attrs, indices=glb.indices(geo['faces']), mode=TRIANGLES, material=color_mat)
        children.append(glb.node(name='scene', mesh=mesh))

    # cameras (add_scene_cam, viz.py:246-319); the textures are encoded on a thread pool (zlib releases the GIL)
    n_cams = len(cams2world)
    textures = [None] * n_cams
    if not transparent_cams:
        with ThreadPoolExecutor(max(1, min(usable_cpus(), n_cams))) as ex:
            textures = list(ex.map(_png, [imgs[i] for i in range(n_cams)]))
    for i, pose_c2w in enumerate(cams2world):
        if isinstance(cam_color, list):
            camera_edge_color = cam_color[i]
        else:
            camera_edge_color = cam_color or CAM_COLORS[i % len(CAM_COLORS)]
        cam = scene_camera_geometry(pose_c2w, focals[i], imgs[i].shape[1::-1], screen_width=cam_size)
        if textures[i] is not None:
            tex_mat = glb.material(baseColorTexture=dict(index=glb.texture(textures[i])), roughnessFactor=1.0)
            attrs = dict(POSITION=glb.positions(cam['image_vertices']), TEXCOORD_0=glb.accessor(cam['image_uv'], FLOAT, 'VEC2', ARRAY_BUFFER))
            mesh = glb.mesh(attrs, indices=glb.indices(cam['image_faces']), material=tex_mat)
            children.append(glb.node(name=f'camera_{i}_image', mesh=mesh))
        wire = cam['wire_vertices']
        attrs = dict(POSITION=glb.positions(wire), COLOR_0=glb.colors(np.tile(_rgba(camera_edge_color), (len(wire), 1))))
        mesh = glb.mesh(attrs, indices=glb.indices(cam['wire_faces']), material=color_mat)
        children.append(glb.node(name=f'camera_{i}', mesh=mesh))

    glb.doc['nodes'][0]['children'] = children
    return glb.write(outfile)


def _rot_y180():
    from scipy.spatial.transform import Rotation
    rot = np.eye(4)
    rot[:3, :3] = Rotation.from_euler('y', np.deg2rad(180)).as_matrix()
    return rot


def get_3D_model_from_scene(outdir, silent, scene, min_conf_thr=3, as_pointcloud=False, mask_sky=False,
                            clean_depth=False, transparent_cams=False, cam_size=0.05):
    """
    extract 3D_model (glb file) from a reconstructed scene
    """
    if scene is None:
        return None
    if scene.imgs is None:
        raise ValueError('get_3D_model_from_scene needs the scene images: scene.imgs is None (the views given to global_aligner had no "img")')
    # post processes
    if clean_depth:
        scene = scene.clean_pointcloud()
    if mask_sky:
        scene = scene.mask_sky()

    # get optimized values from scene
    with torch.no_grad():
        rgbimg = scene.imgs
        focals = scene.get_focals().cpu()
        cams2world = scene.get_im_poses().cpu()
        # 3D pointcloud from depthmap, poses and intrinsics: the scene's padded stacks go to the mesh kernels as they are
        pts3d = scene.get_pts3d(raw=True)
        scene.min_conf_thr = float(scene.conf_trf(torch.tensor(min_conf_thr)))
        msk = scene.get_masks(raw=True)
    return _convert_scene_output_to_glb(outdir, rgbimg, pts3d, msk, focals, cams2world, as_pointcloud=as_pointcloud,
                                        transparent_cams=transparent_cams, cam_size=cam_size, silent=silent)


def render_turntable(outdir, scene, n_frames=36, size=(1024, 768), as_pointcloud=True, min_conf_thr=3, mask_sky=False, clean_depth=False,
                     point_size=2, focal=None, cam_size=None, transparent_cams=False, elevation_deg=20.0, background=(255, 255, 255), silent=True):
    """n_frames pictures of a reconstructed scene from a circle round it, written as outdir/turntable_000.png ...; returns the file names.
    The same pre-processing switches as get_3D_model_from_scene (clean_depth, mask_sky, min_conf_thr, as_pointcloud: the masked cloud or the
    export's mesh) and the same camera glyphs (wire only; none with transparent_cams). The circle lies about the first camera's "down"
    axis through the centre of the scene's bounds, raised by elevation_deg, at the distance where the bounds fit the frame
    (viz.turntable_poses); focal defaults to 1.1 min(size). All frames are drawn in ONE call of the rasteriser; the PNGs are encoded on a
    thread pool."""
    if scene is None:
        return None
    if scene.imgs is None:
        raise ValueError('render_turntable needs the scene images: scene.imgs is None (the views given to global_aligner had no "img")')
    if clean_depth:
        scene = scene.clean_pointcloud()
    if mask_sky:
        scene = scene.mask_sky()
    with torch.no_grad():
        focals = scene.get_focals().cpu().numpy().reshape(-1)
        cams2world = scene.get_im_poses().cpu().numpy()
        scene.min_conf_thr = float(scene.conf_trf(torch.tensor(min_conf_thr)))
        viz = SceneViz(scene.device)
        if as_pointcloud:
            viz.add_pointcloud(list(scene.get_pts3d()), list(scene.imgs), list(scene.get_masks()))
        else:
            geo = scene_mesh_batch(scene.imgs, scene.get_pts3d(raw=True), scene.get_masks(raw=True), scene.device, to_host=False)
            if len(geo['faces']):
                viz.add_mesh(geo['positions'], geo['faces'], geo['colors'])
        bounds = viz.bounds()
        if bounds is None:
            raise ValueError('render_turntable: no valid point in the scene (lower min_conf_thr)')
        if not transparent_cams:
            viz.add_cameras(cams2world, focals, imsizes=scene.imsizes, colors=[CAM_COLORS[i % len(CAM_COLORS)] for i in range(len(cams2world))],
                            cam_size=auto_cam_size(cams2world) if cam_size is None else cam_size)
        focal = 1.1 * min(size) if focal is None else float(focal)
        poses = turntable_poses(bounds, n_frames, focal, size, down=cams2world[0][:3, 1], elevation_deg=elevation_deg)
        frames = viz.render(poses, focal, size=size, point_size=point_size, background=background)
    os.makedirs(outdir, exist_ok=True)
    names = [os.path.join(outdir, f'turntable_{k:03d}.png') for k in range(n_frames)]

    def write(k):
        with open(names[k], 'wb') as f:
            f.write(_png(frames[k]))
    with ThreadPoolExecutor(max(1, min(usable_cpus(), n_frames))) as ex:
        list(ex.map(write, range(n_frames)))
    if not silent:
        print('(wrote', n_frames, 'frames to', outdir, ')')
    return names


# ---- the gallery -------------------------------------------------------------------------------------------------------------------
# matplotlib's `jet` as its segment data: per channel (x, y below x, y above x)
_JET_SEGMENTS = {
    'red': ((0.00, 0, 0), (0.35, 0, 0), (0.66, 1, 1), (0.89, 1, 1), (1.00, 0.5, 0.5)),
    'green': ((0.000, 0, 0), (0.125, 0, 0), (0.375, 1, 1), (0.640, 1, 1), (0.910, 0, 0), (1.000, 0, 0)),
    'blue': ((0.00, 0.5, 0.5), (0.11, 1, 1), (0.34, 1, 1), (0.65, 0, 0), (1.00, 0, 0)),
}
GALLERY_BAD_ROW = 256


def jet_lut(n=256):
    """The (n, 4) float64 RGBA table of matplotlib's `jet`: its segment data interpolated linearly at linspace(0, 1, n) the way
    LinearSegmentedColormap builds its table, alpha 1."""
    xind = (n - 1) * np.linspace(0, 1, n)
    lut = np.ones((n, 4))
    for c, name in enumerate(('red', 'green', 'blue')):
        data = np.array(_JET_SEGMENTS[name], dtype=np.float64)
        x, y0, y1 = data[:, 0] * (n - 1), data[:, 1], data[:, 2]
        ind = np.searchsorted(x, xind)[1:-1]
        distance = (xind[1:-1] - x[ind - 1]) / (x[ind] - x[ind - 1])
        lut[:, c] = np.clip(np.concatenate([[y1[0]], distance * (y0[ind] - y1[ind - 1]) + y1[ind - 1], [y0[-1]]]), 0.0, 1.0)
    return lut


def gallery_table():
    """The (257, 4) float32 table of d3r_scene_gallery, built in fp64: rows 0-255 = rgb() of jet's colours -- x * 0.5 + 0.5, clipped; the
    reference sends the looked-up float colours through rgb(), which washes them out --, row 256 the same of the "bad" colour (0, 0, 0, 0)."""
    lut = np.concatenate([jet_lut(), np.zeros((1, 4))])
    return np.float32((lut * 0.5 + 0.5).clip(min=0, max=1))


_table_cache = {}


def _device_table(device):
    key = (device.type, device.index)
    if key not in _table_cache:
        _table_cache[key] = torch.from_numpy(gallery_table()).to(device)      # uploaded once per device
    return _table_cache[key]


@torch.no_grad()
def gallery_images(depth, conf, npix):
    """d3r_scene_gallery on padded stacks: depth, conf (n, row) fp32 device tensors (row % 4 == 0), npix (n,) int32 device tensor of pixel
    counts. Returns device tensors: depth_img (n, row), conf_img (n, row, 4) -- what lies behind an image's count is left unwritten -- and
    maxima (2,) = (depth maximum, confidence maximum) over all valid pixels. No synchronisation."""
    _lib.require_device()
    n, row = depth.shape
    device = depth.device
    depth_img = torch.empty((n, row), dtype=torch.float32, device=device)
    conf_img = torch.empty((n, row, 4), dtype=torch.float32, device=device)
    maxima = torch.empty((2,), dtype=torch.float32, device=device)
    work = _lib.workspace(max(1, _lib.lib.d3r_scene_gallery_workspace_bytes(n, row)), device)
    with torch.cuda.device(device):
        _lib.check(_lib.lib.d3r_scene_gallery(n, _lib.ptr(depth), _lib.ptr(conf), _lib.ptr(npix), row, _lib.ptr(_device_table(device)), _lib.ptr(depth_img),
                                              _lib.ptr(conf_img), _lib.ptr(maxima), _lib.ptr(work), _lib.current_stream()), 'scene_gallery')
    return depth_img, conf_img, maxima


@torch.no_grad()
def scene_gallery(scene):
    """The `imgs` that the reference's get_reconstructed_scene returns (dust3r/demo.py:168-184): [rgb_0, depth_0, conf_0, rgb_1, ...] with
    rgb_i = scene.imgs[i], depth_i = rgb(depth / max over all images) as (H, W) float32 and conf_i = rgb(jet(conf / max over all images)) as
    (H, W, 4) -- float32 where the reference returns float64: the values are np.float32 of the reference's. All images in one GPU call.
    (A NaN in any map makes the maximum NaN, as numpy.max does; the reference's python max() over the per-image maxima keeps a NaN only
    when the first image has it.)"""
    if scene.imgs is None:
        raise ValueError('scene_gallery needs the scene images: scene.imgs is None (the views given to global_aligner had no "img")')
    if scene.device.type != 'cuda':
        raise _lib.D3RError('scene_gallery runs on the GPU (dust3r_amd has no CPU execution path)')
    depth_img, conf_img, _ = gallery_images(scene.get_depthmaps(raw=True), scene._im_conf, scene._shape_tables[2])
    host_d, host_c = host_tensor(depth_img.shape), host_tensor(conf_img.shape)
    host_d.copy_(depth_img)
    host_c.copy_(conf_img)
    host_d, host_c = host_d.numpy(), host_c.numpy()
    imgs = []
    for i, (h, w) in enumerate(scene.imshapes):
        imgs.append(scene.imgs[i])
        imgs.append(host_d[i, :h * w].reshape(h, w))
        imgs.append(host_c[i, :h * w].reshape(h, w, 4))
    return imgs


# ---- the reconstruction ---------------------------------------------------------------------------------------------------------------
def get_reconstructed_scene(outdir, model, device, silent, image_size, filelist, schedule, niter, min_conf_thr,
                            as_pointcloud, mask_sky, clean_depth, transparent_cams, cam_size,
                            scenegraph_type, winsize, refid):
    """
    from a list of images, run dust3r inference, global aligner.
    then run get_3D_model_from_scene
    """
    try:
        square_ok = model.square_ok
    except Exception:
        square_ok = False
    imgs = load_images(filelist, size=image_size, verbose=not silent, patch_size=model.patch_size, square_ok=square_ok)
    if len(imgs) == 1:
        imgs = [imgs[0], copy.deepcopy(imgs[0])]
        imgs[1]['idx'] = 1
    if scenegraph_type == 'swin':
        scenegraph_type = scenegraph_type + '-' + str(winsize)
    elif scenegraph_type == 'oneref':
        scenegraph_type = scenegraph_type + '-' + str(refid)

    pairs = make_pairs(imgs, scene_graph=scenegraph_type, prefilter=None, symmetrize=True)
    output = inference(pairs, model, device, batch_size=1, verbose=not silent)

    mode = GlobalAlignerMode.PointCloudOptimizer if len(imgs) > 2 else GlobalAlignerMode.PairViewer
    scene = global_aligner(output, device=device, mode=mode, verbose=not silent)
    lr = 0.01

    if mode == GlobalAlignerMode.PointCloudOptimizer:
        scene.compute_global_alignment(init='mst', niter=niter, schedule=schedule, lr=lr)

    outfile = get_3D_model_from_scene(outdir, silent, scene, min_conf_thr, as_pointcloud, mask_sky,
                                      clean_depth, transparent_cams, cam_size)

    # also return rgb, depth and confidence imgs: depth normalized with the max value for all images, jet on the confidence maps
    return scene, outfile, scene_gallery(scene)


def scenegraph_options(num_files, winsize, refid, scenegraph_type):
    """The rule of the reference's set_scenegraph_options (dust3r/demo.py:189-207) as data: ((value, minimum, maximum, visible) of the
    window-size control, the same of the reference-id control) for num_files input files (None: no input yet, counted as one). Like the
    reference, the incoming winsize / refid do not enter: every change resets the controls."""
    num_files = num_files if num_files is not None else 1
    max_winsize = max(1, math.ceil((num_files - 1) / 2))
    return ((max_winsize, 1, max_winsize, scenegraph_type == 'swin'), (0, 0, num_files - 1, scenegraph_type == 'oneref'))


# ---- the command line -------------------------------------------------------------------------------------------------------------------
def get_args_parser():
    parser = argparse.ArgumentParser(prog='python -m dust3r_amd.demo', description='pictures -> scene.glb, the rgb / depth / confidence gallery, cameras.json')
    parser.add_argument('images', nargs='+', help='image files, or one folder of them')
    parser.add_argument('--outdir', type=str, default='.', help='where scene.glb, gallery/ and cameras.json go')
    parser.add_argument('--image_size', type=int, default=512, choices=[512, 224], help='image size')
    parser_weights = parser.add_mutually_exclusive_group(required=True)
    parser_weights.add_argument('--weights', type=str, help='path to the model weights', default=None)
    parser_weights.add_argument('--model_name', type=str, help='a snapshot directory of the model weights (config.json + model.safetensors), for from_pretrained')
    parser.add_argument('--device', type=str, default='cuda', help='pytorch device')
    parser.add_argument('--silent', action='store_true', default=False, help='silence logs')
    parser.add_argument('--schedule', type=str, default='linear', choices=['linear', 'cosine'], help='learning-rate schedule of the global alignment')
    parser.add_argument('--niter', type=int, default=300, help='iterations of the global alignment')
    parser.add_argument('--min_conf_thr', type=float, default=3.0)
    parser.add_argument('--cam_size', type=float, default=0.05, help='size of the cameras in the exported scene')
    parser.add_argument('--scenegraph_type', type=str, default='complete', choices=['complete', 'swin', 'oneref'], help='how pairs are made')
    parser.add_argument('--winsize', type=int, default=None, help='swin: window size (default: the largest; clamped to the valid range)')
    parser.add_argument('--refid', type=int, default=None, help='oneref: the reference image (default 0; clamped to the valid range)')
    parser.add_argument('--as_pointcloud', action='store_true', default=False)
    parser.add_argument('--mask_sky', action='store_true', default=False)
    parser.add_argument('--clean_depth', action=argparse.BooleanOptionalAction, default=True, help='clean-up depthmaps')
    parser.add_argument('--transparent_cams', action='store_true', default=False)
    parser.add_argument('--turntable', type=int, default=0, metavar='N', help='also render N turntable frames into outdir/turntable')
    parser.add_argument('--fuse', type=float, nargs='?', const=0.0, default=None, metavar='VOXEL',
                        help='fuse the views into one voxel-averaged cloud (scene.fuse) and write it as outdir/scene.ply; VOXEL: the voxel size '
                             '(default: the median pixel footprint)')
    parser.add_argument('--ply', action='store_true', default=False, help='write the fused cloud as outdir/scene.ply (implies --fuse)')
    parser.add_argument('--colmap', action='store_true', default=False, help='write the fused cloud, cameras and images as a COLMAP model in outdir/colmap (implies --fuse)')
    parser.add_argument('--colmap_tracks', action='store_true', default=False,
                        help='with --colmap: also write the 2-D tracks (POINTS2D per image, the track and mean reprojection error per point; '
                             'FusedCloud.build_tracks) and their statistics into cameras.json under "tracks"')
    parser.add_argument('--max_reproj_error', type=float, default=None, metavar='PX',
                        help='with --colmap_tracks: drop observations whose projection lands more than PX pixels from the observing pixel')
    parser.add_argument('--fuse_normals', action='store_true', default=False,
                        help='estimate normals of the fused cloud, turned towards the cameras, and write them into scene.ply (implies --fuse)')
    parser.add_argument('--fuse_outliers', type=float, default=None, metavar='STD_RATIO',
                        help='statistical outlier removal on the fused cloud: drop points whose mean neighbour distance exceeds mean + STD_RATIO std (implies --fuse)')
    parser.add_argument('--fuse_clusters', type=float, nargs='?', const=0.0, default=None, metavar='EPS_IN_VOXELS',
                        help='density clustering (DBSCAN) of the fused cloud: scene.ply gets an int label per point, cameras.json the cluster sizes; '
                             'EPS_IN_VOXELS: the neighbourhood radius in voxels (default 2.5) (implies --fuse)')
    parser.add_argument('--fuse_keep_largest', type=int, default=None, metavar='N',
                        help='keep only the N largest clusters of the fused cloud, which drops dense floaters (implies --fuse_clusters and --fuse)')
    parser.add_argument('--fuse_planes', type=int, nargs='?', const=6, default=None, metavar='N',
                        help='detect the N dominant planes of the fused cloud (default 6): scene.ply gets an int plane per point, cameras.json the '
                             'planes and their sizes (implies --fuse)')
    parser.add_argument('--fuse_upright', action='store_true',
                        help='stand scene.ply on its ground plane (the largest plane with every camera on one side): y up, ground at height 0; '
                             'cameras.json gets the 4x4 motion under "upright" (implies --fuse_planes and --fuse)')
    return parser


def wants_fuse(args):
    """--ply, --colmap, --fuse_normals, --fuse_outliers, --fuse_clusters, --fuse_keep_largest, --fuse_planes and --fuse_upright imply --fuse"""
    return (args.fuse is not None or args.ply or args.colmap or args.fuse_normals or args.fuse_outliers is not None or args.fuse_clusters is not None or
            args.fuse_keep_largest is not None or args.fuse_planes is not None or args.fuse_upright)


def clamp_scenegraph(num_files, winsize, refid, scenegraph_type):
    """--winsize / --refid as the page's sliders would hold them: the control's default when not given, else clamped to its range."""
    (w_value, w_min, w_max, _), (r_value, r_min, r_max, _) = scenegraph_options(num_files, winsize, refid, scenegraph_type)
    winsize = w_value if winsize is None else min(max(int(winsize), w_min), w_max)
    refid = r_value if refid is None else min(max(int(refid), r_min), r_max)
    return winsize, refid


def _input_files(images):
    if len(images) == 1 and os.path.isdir(images[0]):
        root = images[0]
        return [os.path.join(root, name) for name in sorted(os.listdir(root)) if name.lower().endswith(IMAGE_EXTENSIONS)]
    return list(images)


def write_gallery(outdir, imgs):
    """gallery/view{k}_{rgb,depth,conf}.png of the `imgs` of get_reconstructed_scene; returns the file names."""
    os.makedirs(os.path.join(outdir, 'gallery'), exist_ok=True)
    names = [os.path.join(outdir, 'gallery', f'view{k // 3}_{("rgb", "depth", "conf")[k % 3]}.png') for k in range(len(imgs))]

    def write(k):
        with open(names[k], 'wb') as f:
            f.write(_png(imgs[k]))
    with ThreadPoolExecutor(max(1, min(usable_cpus(), len(imgs)))) as ex:
        list(ex.map(write, range(len(imgs))))
    return names


def write_cameras(outdir, scene):
    """cameras.json: per image its cam2world matrix, focal(s) and (width, height)."""
    with torch.no_grad():
        cams2world = scene.get_im_poses().cpu().numpy()
        focals = scene.get_focals().cpu().numpy().reshape(len(cams2world), -1)
    name = os.path.join(outdir, 'cameras.json')
    with open(name, 'w') as f:
        json.dump(dict(cam2world=[m.tolist() for m in cams2world], focals=[[float(v) for v in row] for row in focals],
                       image_sizes=[[int(w), int(h)] for w, h in scene.imsizes]), f, indent=1)
    return name


def write_fused(outdir, scene, voxel_size=None, min_conf_thr=3, mask_sky=False, ply=True, colmap=False, normals=False, outliers=None, tracks=False,
                max_reproj_error=None, clusters=None, keep_largest=None, planes=None, upright=False):
    """outdir/scene.ply and / or outdir/colmap of the scene's fused cloud (scene.fuse; export.write_ply / write_colmap), with the mask of
    get_3D_model_from_scene: min_conf_thr through the scene's confidence transform, the sky on request; normals / outliers / tracks /
    max_reproj_error as for scene.fuse. With tracks, their `stats()` are added to outdir/cameras.json (when it is there) under "tracks".
    clusters: None, or the eps of `FusedCloud.cluster` in voxels (0: its default); keep_largest=N keeps the N largest clusters (and implies
    clusters). The cluster count and the ten largest sizes are added to cameras.json under "clusters"; scene.ply gets an `int label`.
    planes=N: the N dominant planes (`FusedCloud.detect_planes`): scene.ply gets an `int plane`, cameras.json "planes" (the models in the
    scene's frame and their sizes). upright (implies planes=6): scene.ply is written stood on its ground (`FusedCloud.upright`) and the
    motion goes to cameras.json under "upright" when a ground was found; the COLMAP model stays in the scene's frame, where its cameras are.
    Returns the file names."""
    from .export import write_colmap
    if upright and planes is None:
        planes = 6
    if mask_sky:
        scene = scene.mask_sky()
    scene.min_conf_thr = float(scene.conf_trf(torch.tensor(min_conf_thr)))
    voxel_size, cluster_args = voxel_size or None, None
    if clusters is not None or keep_largest is not None:
        cluster_args = True
        if clusters:                 # eps in voxels: the voxel size has to be known before the call
            if voxel_size is None:
                from .viz import default_voxel_size
                voxel_size = default_voxel_size(scene.get_depthmaps(raw=True), [h * w for h, w in scene.imshapes], scene.get_focals())
            if math.isfinite(voxel_size) and voxel_size > 0:             # else: a scene without a valid point, which scene.fuse handles
                cluster_args = dict(eps=float(clusters) * voxel_size)
    cloud = scene.fuse(voxel_size=voxel_size, normals=normals, outliers=outliers, tracks=tracks, max_reproj_error=max_reproj_error, clusters=cluster_args,
                       keep_largest=keep_largest, planes=planes)
    written, motion = [], None
    if upright:
        try:
            stood, motion = cloud.upright(scene=scene)
        except ValueError:                                                # no ground among the planes: the cloud stays as it is
            stood = cloud
    if ply:
        written.append((stood if upright else cloud).save_ply(os.path.join(outdir, 'scene.ply')))
    if colmap:
        written += write_colmap(os.path.join(outdir, 'colmap'), scene, cloud)
    cameras = os.path.join(outdir, 'cameras.json')
    if (tracks or cluster_args is not None or planes is not None) and os.path.isfile(cameras):
        with open(cameras) as f:
            doc = json.load(f)
        if tracks:
            doc['tracks'] = cloud.tracks.stats()
        if cluster_args is not None:
            sizes = [int(s) for s in (cloud.cluster_sizes.tolist() if cloud.cluster_sizes is not None else [])]
            doc['clusters'] = dict(count=len(sizes), largest=sizes[:10], kept=None if keep_largest is None else min(int(keep_largest), len(sizes)))
        if planes is not None:
            doc['planes'] = dict(models=[[float(v) for v in m] for m in cloud.planes], sizes=[int(v) for v in cloud.plane_sizes])
            if motion is not None:
                doc['upright'] = [[float(v) for v in row] for row in motion]
        with open(cameras, 'w') as f:
            json.dump(doc, f, indent=1)
    return written


def main(argv=None):
    from .model import AsymmetricCroCo3DStereo
    parser = get_args_parser()
    args = parser.parse_args(argv)
    if args.colmap_tracks and not args.colmap:
        parser.error('--colmap_tracks needs --colmap')
    if args.max_reproj_error is not None and not args.colmap_tracks:
        parser.error('--max_reproj_error needs --colmap_tracks')
    files = _input_files(args.images)
    if not files:
        raise SystemExit(f'no image in {args.images}')
    winsize, refid = clamp_scenegraph(len(files), args.winsize, args.refid, args.scenegraph_type)
    model = AsymmetricCroCo3DStereo.from_pretrained(args.weights if args.weights is not None else args.model_name).to(args.device)
    os.makedirs(args.outdir, exist_ok=True)
    scene, outfile, imgs = get_reconstructed_scene(args.outdir, model, args.device, args.silent, args.image_size, files, args.schedule, args.niter,
                                                   args.min_conf_thr, args.as_pointcloud, args.mask_sky, args.clean_depth, args.transparent_cams,
                                                   args.cam_size, args.scenegraph_type, winsize, refid)
    written = [outfile, write_cameras(args.outdir, scene)] + write_gallery(args.outdir, imgs)
    if args.turntable > 0:
        written += render_turntable(os.path.join(args.outdir, 'turntable'), scene, n_frames=args.turntable, min_conf_thr=args.min_conf_thr,
                                    mask_sky=args.mask_sky, clean_depth=args.clean_depth, transparent_cams=args.transparent_cams, silent=args.silent)
    if wants_fuse(args):
        written += write_fused(args.outdir, scene, voxel_size=args.fuse, min_conf_thr=args.min_conf_thr, mask_sky=args.mask_sky,
                               ply=args.ply or not args.colmap, colmap=args.colmap, normals=args.fuse_normals, outliers=args.fuse_outliers,
                               tracks=args.colmap_tracks, max_reproj_error=args.max_reproj_error, clusters=args.fuse_clusters,
                               keep_largest=args.fuse_keep_largest, planes=args.fuse_planes, upright=args.fuse_upright)
    if not args.silent:
        print('(wrote', len(written), 'files to', args.outdir, ')')
    return 0


if __name__ == '__main__':
    raise SystemExit(main())
