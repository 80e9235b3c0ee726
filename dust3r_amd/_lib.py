"""ctypes binding of libdust3r_hip.so (C ABI declared in include/dust3r_hip.h).

The product path has NO CPU fallback: importing this module without the built library raises,
and every compute entry point checks for a gfx950 device (`require_device`) before touching it.
"""
import ctypes as C
import os

import torch  # noqa: F401  (loads torch's libamdhip64.so.7 first so that the engine shares its HIP runtime)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, 'csrc', 'libdust3r_hip.so')

DTYPE_BF16, DTYPE_F16, DTYPE_F32, DTYPE_F16X3, DTYPE_F16F8, DTYPE_F16X2F8 = 0, 1, 2, 3, 4, 5
DTYPES = {'bf16': DTYPE_BF16, 'bfloat16': DTYPE_BF16, 'f16': DTYPE_F16, 'fp16': DTYPE_F16, 'float16': DTYPE_F16,
          'f32': DTYPE_F32, 'fp32': DTYPE_F32, 'float32': DTYPE_F32, 'fp16x3': DTYPE_F16X3, 'f16x3': DTYPE_F16X3,
          'fp16f8': DTYPE_F16F8, 'f16f8': DTYPE_F16F8, 'fp16x2f8': DTYPE_F16X2F8}
TORCH_DTYPE = {DTYPE_BF16: torch.bfloat16, DTYPE_F16: torch.float16, DTYPE_F32: torch.float32}
# the aligner's option, trainability-kind and schedule ids: D3R_<name> of include/dust3r_hip.h
(ALIGNER_OPT_DPP_REDUCE, ALIGNER_OPT_RESET_ADAM, ALIGNER_OPT_OPTIMIZE_PP, ALIGNER_OPT_OPTIMIZE_ADAPTORS, ALIGNER_OPT_GENERIC_SMALL,
 ALIGNER_OPT_EDGE_MEAN_LOSS, ALIGNER_OPT_FX_AND_FY) = 1, 2, 3, 4, 5, 6, 7
ALIGNER_TRAIN_POSES, ALIGNER_TRAIN_FOCALS, ALIGNER_TRAIN_PP = 0, 1, 2
SCHEDULE_COSINE, SCHEDULE_LINEAR = 0, 1
HEAD_ROPE, HEAD_VT, HEAD_PLAIN = 1, 2, 3      # D3R_HEAD_* of include/dust3r_hip.h
TILE_128W8 = 12                               # D3R_TILE_128W8
CONV_RELU, CONV_NOWIDE, DECLINED = 1, 4, 1    # D3R_CONV_RELU / D3R_CONV_NOWIDE (flags of d3r_conv2d_nhwc_x), D3R_DECLINED (d3r_conv_head4)

ERRORS = {0: 'OK', -1: 'invalid argument', -2: 'allocation failed', -3: 'kernel launch failed', -4: 'unknown state-dict key',
          -5: 'shape mismatch', -6: 'bad state (weights missing / no gfx950 device)'}


class D3RError(RuntimeError):
    pass


class ModelConfig(C.Structure):
    _fields_ = [('enc_embed_dim', C.c_int), ('enc_depth', C.c_int), ('enc_num_heads', C.c_int),
                ('dec_embed_dim', C.c_int), ('dec_depth', C.c_int), ('dec_num_heads', C.c_int),
                ('patch_size', C.c_int), ('head_type', C.c_int), ('dtype', C.c_int), ('rope_freq', C.c_float),
                ('dpt_skip_relu_inplace', C.c_int)]


class MatchJob(C.Structure):
    """d3r_match_job (include/dust3r_hip.h)"""
    _fields_ = [('pts_query', C.c_void_p), ('conf_query', C.c_void_p), ('pts_map', C.c_void_p), ('conf_map', C.c_void_p),
                ('valid_map', C.c_void_p), ('n_query', C.c_int), ('n_map', C.c_int), ('conf_thr', C.c_float), ('reserved', C.c_int)]


class PnpRansacJob(C.Structure):
    """d3r_pnp_ransac_job (include/dust3r_hip.h)"""
    _fields_ = [('pts2d', C.c_void_p), ('pts3d', C.c_void_p), ('inlier_mask', C.c_void_p), ('n', C.c_int), ('max_iters', C.c_int),
                ('fx', C.c_float), ('fy', C.c_float), ('cx', C.c_float), ('cy', C.c_float), ('thr', C.c_float), ('confidence', C.c_float),
                ('seed', C.c_ulonglong)]


class CriterionOpts(C.Structure):
    """d3r_criterion_opts (include/dust3r_hip.h)"""
    _fields_ = [('norm_mode', C.c_int), ('gt_scale', C.c_int), ('shift_inv', C.c_int), ('scale_inv', C.c_int), ('center_mode', C.c_int),
                ('use_conf', C.c_int), ('has_dist_clip', C.c_int), ('stop_after', C.c_int), ('dist_clip', C.c_float), ('alpha', C.c_float)]


class ViewPlan(C.Structure):
    """d3r_view_plan (include/dust3r_hip.h)"""
    _fields_ = [('rgb', C.c_void_p), ('depth', C.c_void_p), ('kx', C.c_void_p), ('bx', C.c_void_p), ('ky', C.c_void_p), ('by', C.c_void_p),
                ('tmp_off', C.c_longlong), ('src_w', C.c_int), ('src_h', C.c_int), ('crop_l', C.c_int), ('crop_t', C.c_int), ('crop_w', C.c_int),
                ('crop_h', C.c_int), ('rs_w', C.c_int), ('rs_h', C.c_int), ('kxs', C.c_int), ('kys', C.c_int), ('off_x', C.c_int), ('off_y', C.c_int),
                ('w', C.c_int), ('h', C.c_int), ('row0', C.c_int), ('nrows', C.c_int), ('transpose', C.c_int), ('fu', C.c_float), ('fv', C.c_float),
                ('cu', C.c_float), ('cv', C.c_float), ('pose', C.c_float * 12)]


class PnpRansacParams(C.Structure):
    """d3r_pnp_ransac_params (include/dust3r_hip.h)"""
    _fields_ = [('max_iters', C.c_int), ('max_points', C.c_int)]


def _load():
    if not os.path.exists(LIB_PATH):
        raise ImportError(f'{LIB_PATH} is missing: build it with `python -c "import __graft_entry__ as g; g.build()"` '
                          '(or `python dust3r_amd/build.py`). dust3r_amd has no CPU fallback.')
    lib = C.CDLL(LIB_PATH)
    vp, i, f, fp, ip = C.c_void_p, C.c_int, C.c_float, C.c_void_p, C.c_void_p
    sig = {
        'd3r_version': (C.c_char_p, []),
        'd3r_device_check': (i, []),
        'd3r_rope2d': (i, [vp, vp, i, i, i, i, f, f, i, vp]),
        'd3r_layernorm': (i, [fp, fp, fp, vp, i, i, f, i, vp]),
        'd3r_linear': (i, [vp, vp, fp, vp, fp, i, i, i, i, i, vp]),
        'd3r_linear_x3res': (i, [vp, vp, fp, vp, vp, fp, i, i, i, vp]),
        'd3r_rope_table': (i, [fp, i, f, f, vp]),
        'd3r_linear_heads': (i, [vp, vp, fp, i, i, i, i, ip, vp, i, i, i, i, fp, i, fp, fp, fp, fp, f, fp, C.c_size_t, vp, i, i, vp]),
        'd3r_linear_heads_tile_config': (i, [i, i, i, i, ip, i, i, i, i, i, i]),
        'd3r_ln_finalize': (i, [fp, i, i, f, fp, fp, vp]),
        'd3r_ln_fold_pack': (i, [fp, fp, fp, fp, vp, fp, fp, i, i, i, vp]),
        'd3r_linear_ln': (i, [vp, vp, fp, vp, i, i, i, i, fp, fp, fp, fp, f, vp]),
        'd3r_layernorm_x3rows': (i, [vp, fp, fp, vp, i, i, f, vp]),
        'd3r_conv2d_nhwc': (i, [vp, vp, fp, vp, vp, vp, vp, i, i, i, i, i, i, i, i, i, vp, i, vp]),
        'd3r_conv_k_slice_major': (i, []),
        'd3r_pack_conv_weight': (i, [fp, vp, i, i, i, i, i, i, i, vp]),
        'd3r_pack_convt_bias': (i, [fp, fp, i, i, i, vp]),
        'd3r_conv2d_nhwc_x': (i, [vp, vp, fp, vp, vp, vp, vp, i, i, i, i, i, i, i, i, i, i, i, i, vp, i, vp]),
        'd3r_convt_gemm': (i, [vp, vp, fp, vp, i, i, i, i, i, i, i, i, i, vp]),
        'd3r_conv_head4': (i, [vp, vp, fp, fp, fp, fp, fp, i, i, i, i, i, i, i, i, i, i, i, f, f, vp, i, vp]),
        'd3r_up2_conv_head4': (i, [vp, vp, vp, fp, fp, fp, fp, fp, i, i, i, i, i, i, i, i, i, i, f, f, vp, i, vp]),
        'd3r_up2_conv_route': (i, [i, i, i, i, i, i, i, i]),
        'd3r_up2_conv2d_nhwc_x': (i, [vp, vp, vp, fp, vp, i, i, i, i, i, i, i, i, vp, i, vp]),
        'd3r_head_final': (i, [vp, i, fp, fp, fp, fp, C.c_size_t, i, i, i, i, f, f, i, vp]),
        'd3r_linear_head_post': (i, [fp, fp, fp, i, i, i, i, i, i, i, i, f, f, vp]),
        'd3r_attention': (i, [vp, vp, vp, vp, i, i, i, i, i, f, i, vp]),
        'd3r_attention_rows': (i, [vp, vp, vp, vp, i, i, i, i, i, f, i, i, vp]),
        'd3r_upsample2x_nhwc': (i, [vp, vp, i, i, i, i, i, i, i, vp]),
        'd3r_gemm_set_trace': (i, [vp, C.c_size_t]),
        'd3r_gemm_tile_config': (i, [i, i, i, i, i, i]),
        'd3r_build_has_probes': (i, []),
        'd3r_model_create': (i, [C.POINTER(vp), C.POINTER(ModelConfig)]),
        'd3r_model_destroy': (i, [vp]),
        'd3r_model_load_tensor': (i, [vp, C.c_char_p, fp, i, C.POINTER(C.c_int64)]),
        'd3r_model_load_tensor_device': (i, [vp, C.c_char_p, fp, i, C.POINTER(C.c_int64)]),
        'd3r_model_missing': (i, [vp]),
        'd3r_model_forward': (i, [vp, fp, fp, i, i, i, fp, fp, fp, fp, vp]),
        'd3r_model_forward_mixed': (i, [vp, fp, i, i, fp, i, i, i, fp, fp, fp, fp, vp]),
        'd3r_model_forward_packed': (i, [vp, fp, fp, i, i, i, fp, vp]),
        'd3r_model_device_bytes': (C.c_size_t, [vp]),
        'd3r_model_graph_replays': (C.c_long, [vp]),
        'd3r_model_feature_bytes': (C.c_size_t, [vp, i, i]),
        'd3r_model_encode': (i, [vp, fp, i, i, i, vp, vp]),
        'd3r_model_decode': (i, [vp, vp, i, i, i, fp, fp, fp, fp, vp]),
        'd3r_model_decode_packed': (i, [vp, vp, i, i, i, fp, vp]),
        'd3r_model_debug_read': (i, [vp, i, fp, C.c_size_t, vp]),
        'd3r_model_set_option': (i, [vp, i, i]),
        'd3r_model_set_postprocess': (i, [vp, i, i, f, f]),
        'd3r_model_profile_read': (i, [vp, i, C.POINTER(C.c_int), C.POINTER(C.c_double), C.POINTER(C.c_double)]),
        'd3r_model_profile_launch': (i, [vp, i] + [C.POINTER(C.c_int)] * 4 + [C.POINTER(C.c_double)] * 2),
        'd3r_aligner_create': (i, [C.POINTER(vp), i, i, ip, ip, ip, ip, i, fp, fp, fp, fp, fp, fp, fp, fp, fp, fp, f, f, f,
                                   i, i, i, i, i, vp]),
        'd3r_aligner_destroy': (i, [vp]),
        'd3r_aligner_set_option': (i, [vp, i, i]),
        'd3r_aligner_set_trainable': (i, [vp, i, C.c_char_p]),
        'd3r_aligner_run': (i, [vp, i, i, i, f, f, i, fp, vp]),
        'd3r_aligner_loss_grad': (i, [vp, fp, fp, fp, fp, fp, fp, fp, vp]),
        'd3r_aligner_set_image_range': (i, [vp, i, i]),
        'd3r_aligner_step_begin': (i, [vp, i, i, i, f, f, i, vp]),
        'd3r_aligner_step_end': (i, [vp, i, i, i, f, f, i, vp]),
        'd3r_aligner_reduced_sums': (i, [vp, C.POINTER(vp), C.POINTER(C.c_longlong)]),
        'd3r_aligner_read_losses': (i, [vp, i, fp, vp]),
        'd3r_nearest_neighbors': (i, [fp, i, fp, i, ip, vp]),
        'd3r_clean_pointcloud': (i, [i, fp, fp, fp, fp, fp, ip, ip, i, f, f, vp]),
        'd3r_segment_sky_workspace_bytes': (C.c_size_t, [i, i]),
        'd3r_segment_sky': (i, [i, vp, i, ip, ip, i, vp, vp, vp]),
        'd3r_sky_color_mask': (i, [i, vp, i, ip, ip, i, vp, vp]),
        'd3r_scene_mesh_workspace_bytes': (C.c_size_t, [i, i]),
        'd3r_scene_mesh': (i, [i, vp, vp, vp, i, ip, ip, i, i, vp, vp, vp, vp, vp, vp, vp]),
        'd3r_fuse_bounds_workspace_bytes': (C.c_size_t, [i, i]),
        'd3r_fuse_bounds': (i, [i, fp, vp, fp, ip, ip, i, fp, vp, vp, vp]),
        'd3r_fuse_voxels_workspace_bytes': (C.c_size_t, [i, i, i]),
        'd3r_fuse_voxels': (i, [i, fp, vp, fp, vp, i, ip, ip, i, C.POINTER(C.c_float), f, C.POINTER(C.c_int), i, fp, vp, fp, ip, vp, vp, vp]),
        'd3r_cloud_grid_workspace_bytes': (C.c_size_t, [i, i]),
        'd3r_cloud_grid_build': (i, [i, fp, C.POINTER(C.c_float), f, C.POINTER(C.c_int), vp, vp]),
        'd3r_cloud_nearest': (i, [i, i, fp, f, C.POINTER(C.c_float), f, C.POINTER(C.c_int), i, fp, ip, ip, vp, vp]),
        'd3r_cloud_distance_stats_workspace_bytes': (C.c_size_t, [i]),
        'd3r_cloud_distance_stats': (i, [i, fp, fp, ip, i, C.POINTER(C.c_float), vp, vp, vp, vp]),
        'd3r_cloud_knn': (i, [i, i, fp, i, f, C.POINTER(C.c_float), f, C.POINTER(C.c_int), i, i, fp, ip, ip, vp, vp]),
        'd3r_cloud_knn_distances_workspace_bytes': (C.c_size_t, [i]),
        'd3r_cloud_knn_distances': (i, [i, i, fp, ip, fp, vp, vp, vp, vp]),
        'd3r_cloud_normals': (i, [i, fp, i, fp, i, ip, i, fp, fp, vp]),
        'd3r_cloud_orient_normals': (i, [i, fp, fp, ip, i, fp, fp, fp, fp, fp, ip, ip, i, f, vp]),
        'd3r_cloud_transform': (i, [i, fp, C.POINTER(C.c_float), fp, fp, C.POINTER(C.c_float), fp, vp]),
        'd3r_cloud_icp_sums_workspace_bytes': (C.c_size_t, [i]),
        'd3r_cloud_icp_sums': (i, [i, fp, fp, i, fp, fp, fp, ip, i, f, f, C.POINTER(C.c_float), vp, vp, vp, vp, vp]),
        'd3r_cloud_cluster_workspace_bytes': (C.c_size_t, [i]),
        'd3r_cloud_cluster': (i, [i, f, i, C.POINTER(C.c_float), f, C.POINTER(C.c_int), ip, ip, ip, ip, vp, ip, C.POINTER(vp), vp, vp, vp]),
        'd3r_cloud_grid_heads': (i, [i, ip, ip, vp, vp]),
        'd3r_cloud_spfh': (i, [i, fp, fp, i, ip, vp, vp]),
        'd3r_cloud_fpfh': (i, [i, i, ip, fp, vp, fp, vp]),
        'd3r_feature_nearest': (i, [i, fp, i, fp, fp, ip, vp]),
        'd3r_sim3_ransac_workspace_bytes': (C.c_size_t, [i, i]),
        'd3r_sim3_ransac': (i, [i, fp, fp, C.c_ulonglong, i, f, C.c_double, i, vp, vp, vp, vp]),
        'd3r_cloud_tracks_workspace_bytes': (C.c_size_t, [i]),
        'd3r_cloud_tracks_count': (i, [i, fp, vp, fp, ip, ip, i, i, fp, vp, f, i, C.c_double, ip, vp, vp, vp]),
        'd3r_cloud_tracks_fill': (i, [i, fp, vp, fp, ip, ip, i, i, fp, vp, f, i, C.c_double, ip, vp, C.c_longlong, i, ip, ip, vp, ip, ip, ip, vp, vp]),
        'd3r_scene_gallery_workspace_bytes': (C.c_size_t, [i, i]),
        'd3r_scene_gallery': (i, [i, fp, fp, ip, i, fp, fp, fp, fp, vp, vp]),
        'd3r_scene_gallery_launch_bound': (None, [C.POINTER(C.c_int)] * 3),
        'd3r_selftest_gallery_index_host': (i, [fp, i, ip]),
        'd3r_render_project': (i, [i, fp, i, fp, i, fp, f, ip, vp, vp]),
        'd3r_render_clear': (i, [i, i, i, vp, vp]),
        'd3r_render_points': (i, [i, fp, vp, C.c_uint32, i, fp, i, fp, f, i, i, i, vp, vp, vp]),
        'd3r_render_triangles': (i, [i, vp, i, fp, C.c_uint32, i, fp, i, fp, f, i, i, vp, vp, vp]),
        'd3r_render_resolve': (i, [i, fp, i, fp, f, i, i, vp, i, C.c_uint32, vp, i, C.c_uint32, vp, i, fp, vp, C.c_uint32, vp, fp, ip, vp]),
        'd3r_match_pairs_workspace': (C.c_size_t, [i, i]),
        'd3r_match_pairs': (i, [i, vp, i, vp, ip, ip, vp]),
        'd3r_pnp_ransac_workspace': (C.c_size_t, [i, i]),
        'd3r_pnp_ransac': (i, [i, vp, C.POINTER(PnpRansacParams), vp, fp, ip, ip, ip, vp]),
        'd3r_selftest_p3p_host': (i, [vp, vp, C.c_double, C.c_double, C.c_double, C.c_double, vp]),
        'd3r_selftest_p3p_roots_host': (i, [vp, vp, vp, vp]),
        'd3r_selftest_ransac_iters_host': (i, [C.c_double, C.c_double, i, i]),
        'd3r_selftest_draw_distinct_host': (i, [C.c_ulonglong, i, i, i, ip]),
        'd3r_row_means': (i, [fp, i, i, i, fp, vp]),
        'd3r_similarity_moments_workspace': (C.c_size_t, [i, i]),
        'd3r_similarity_moments': (i, [i, vp, vp, vp, ip, i, vp, vp, vp]),
        'd3r_weiszfeld_focals': (i, [i, vp, ip, ip, i, fp, vp]),
        'd3r_anchor_depth': (i, [i, vp, fp, ip, i, i, fp, vp]),
        'd3r_pnp_job_bytes': (i, []),
        'd3r_pnp_max_hypotheses': (i, []),
        'd3r_pnp_sum_count': (i, []),
        'd3r_pnp_workspace': (C.c_size_t, [i]),
        'd3r_pnp_score': (i, [i, vp, fp, i, f, ip, vp]),
        'd3r_pnp_sums': (i, [i, vp, fp, f, vp, vp, vp]),
        'd3r_pair_criterion_workspace_bytes': (C.c_size_t, [i, i]),
        'd3r_pair_criterion': (i, [i, i, fp, fp, fp, vp, vp, fp, fp, fp, fp, C.POINTER(CriterionOpts), vp, fp, fp, vp, vp]),
        'd3r_pair_criterion_passes': (i, [C.POINTER(CriterionOpts)]),
        'd3r_masked_median': (i, [i, i, fp, fp, vp, vp, vp, vp, vp]),
        'd3r_view_plan_bytes': (i, []),
        'd3r_prepare_views': (i, [i, C.POINTER(ViewPlan), vp, i, i, fp, vp, C.c_size_t, fp, fp, fp, vp, vp]),
        'd3r_selftest_resample_host': (i, [vp, i, i, i, i, i, i, i, i, vp, vp, i, vp, vp, i, vp]),
        'd3r_selftest_depth_host': (i, [C.POINTER(ViewPlan), i, i, fp, fp, vp]),
        'd3r_selftest_aligner_math_host': (i, [i, i, ip, ip, i, i, fp, fp, fp, fp, fp, fp, fp, fp, f, f, vp, vp, vp, vp, vp]),
    }
    for name, (res, args) in sig.items():
        fn = getattr(lib, name)          # AttributeError here = header / library mismatch
        fn.restype = res
        fn.argtypes = args
    return lib, sorted(sig)


lib, EXPORTED = _load()


def check(rc, what=''):
    if rc != 0:
        msg = ERRORS.get(rc, f'hipError {rc - 1000}' if rc >= 1000 else f'error {rc}')
        raise D3RError(f'libdust3r_hip: {what}: {msg}')


_device_ok = None


def require_device():
    """Raise unless a gfx950 GPU is usable. Called by every compute entry point of the package."""
    global _device_ok
    if _device_ok is None:
        _device_ok = torch.cuda.is_available() and lib.d3r_device_check() == 0
    if not _device_ok:
        raise D3RError('dust3r_amd needs an AMD gfx950 (MI355X) device; there is no CPU fallback in the product path')


def ptr(t):
    """Device (or host) address of a contiguous tensor, or NULL."""
    if t is None:
        return None
    assert t.is_contiguous(), 'tensor must be contiguous'
    return C.c_void_p(t.data_ptr())


def workspace(nbytes, device):
    """The uninitialised device buffer of a call's `workspace` argument: nbytes as its *_workspace_bytes export gives it."""
    return torch.empty(int(nbytes), dtype=torch.uint8, device=device)


def current_stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)
