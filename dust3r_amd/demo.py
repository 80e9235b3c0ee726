"""The export stage of the reference's gradio demo (dust3r/demo.py:66-132): `get_3D_model_from_scene` and `_convert_scene_output_to_glb`,
same signatures, same return value (the path of outdir/scene.glb), without trimesh. The mesh or point cloud is built on the GPU for all
views in one call (viz.scene_mesh_batch), the camera glyphs on the host (viz.scene_camera_geometry), and glb.GlbBuilder writes a glTF 2.0
binary:
- root node: matrix inv(cams2world[0] @ OPENGL @ rot_y180) (the reference's scene.apply_transform), every other node its child; positions
  are the untransformed fp32 points;
- the scene: a TRIANGLES primitive (indices, POSITION, COLOR_0 = the face colours averaged onto the vertices) or, with as_pointcloud, a
  POINTS primitive (POSITION, COLOR_0); left out when nothing is valid;
- one wireframe per camera and, unless transparent_cams, its picture on a textured quad (PNG of np.uint8(255 * img)).
`render_turntable` (new; the reference has no headless output) draws the same scene into PNG frames on the GPU instead."""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from .glb import ARRAY_BUFFER, FLOAT, POINTS, TRIANGLES, GlbBuilder
from .utils.device import to_numpy, usable_cpus
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
        # 3D pointcloud from depthmap, poses and intrinsics: the device tensors go to the mesh kernels as they are
        pts3d = scene.get_pts3d(raw=True)
        scene.min_conf_thr = float(scene.conf_trf(torch.tensor(min_conf_thr)))
        msk = scene.get_masks()
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
        msk = scene.get_masks()
        viz = SceneViz(scene.device)
        if as_pointcloud:
            viz.add_pointcloud(list(scene.get_pts3d()), list(scene.imgs), list(msk))
        else:
            pts3d = scene.get_pts3d(raw=True)
            geo = scene_mesh_batch(scene.imgs, pts3d if isinstance(pts3d, torch.Tensor) else scene.get_pts3d(), msk, scene.device, to_host=False)
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
