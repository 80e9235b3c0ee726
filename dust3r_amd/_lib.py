"""ctypes binding of libdust3r_hip.so (C ABI declared in include/dust3r_hip.h).

The product path has NO CPU fallback: importing this module without the built library raises,
and every compute entry point checks for a gfx950 device (`require_device`) before touching it.
"""
import ctypes as C
import os
import re

import torch  # noqa: F401  (loads torch's libamdhip64.so.7 first so that the engine shares its HIP runtime)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, 'csrc', 'libdust3r_hip.so')
HEADER_PATH = os.path.join(os.path.dirname(_HERE), 'include', 'dust3r_hip.h')

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


_SCALARS = {'void': None, 'int': C.c_int, 'unsigned': C.c_uint, 'long': C.c_long, 'long long': C.c_longlong, 'unsigned long long': C.c_ulonglong,
            'float': C.c_float, 'double': C.c_double, 'size_t': C.c_size_t, 'int32_t': C.c_int32, 'uint32_t': C.c_uint32, 'int64_t': C.c_int64,
            'uint8_t': C.c_uint8}
# the struct arguments that callers may pass by value (ctypes then takes the address): every other pointer is a plain address
_STRUCTS = {'d3r_model_config': ModelConfig, 'd3r_view_plan': ViewPlan, 'd3r_criterion_opts': CriterionOpts, 'd3r_pnp_ransac_params': PnpRansacParams}


def _ctype(decl, text):
    """ctypes class of one return or parameter type as the header spells it (`const float* const*`, `int`, ...)."""
    words = re.sub(r'\bconst\b', ' ', decl)
    base = ' '.join(words.replace('*', ' ').split())
    if '*' in words:
        if base == 'char' and words.count('*') == 1:
            return C.c_char_p
        return C.POINTER(_STRUCTS[base]) if base in _STRUCTS and words.count('*') == 1 else C.c_void_p
    if base not in _SCALARS:
        raise ImportError(f'include/dust3r_hip.h: unknown type `{decl.strip()}` in `{text}`')
    return _SCALARS[base]


def parse_header(text):
    """{name: (restype, [argtypes])} of every d3r_* prototype of a C header: the signatures are read, not restated."""
    text = re.sub(r'/\*.*?\*/|//[^\n]*', ' ', text, flags=re.S)
    text = re.sub(r'^[ \t]*#(?:.*\\\n)*.*$', '', text, flags=re.M).replace('extern "C" {', '')
    text = re.sub(r'\{[^{}]*\}', ' ', text)                  # struct bodies
    sig = {}
    for stmt in text.split(';'):
        if '(' not in stmt:
            continue                                          # typedefs
        stmt = ' '.join(stmt.split())
        m = re.fullmatch(r'([\w\s*]+?)\b(d3r_\w+) ?\(([^()]*)\)', stmt)
        if not m:
            raise ImportError(f'include/dust3r_hip.h: cannot parse the declaration `{stmt}`')
        args = []
        for a in ([] if m.group(3).strip() == 'void' else m.group(3).split(',')):
            p = re.fullmatch(r'(.*?)\b\w+ ?(\[\w*\])?', a.strip())      # type, parameter name, array suffix
            if not p or not p.group(1).strip():
                raise ImportError(f'include/dust3r_hip.h: cannot parse the parameter `{a.strip()}` of `{stmt}`')
            args.append(_ctype(p.group(1) + ('*' if p.group(2) else ''), stmt))
        sig[m.group(2)] = (_ctype(m.group(1), stmt), args)
    return sig


def _load():
    if not os.path.exists(LIB_PATH):
        raise ImportError(f'{LIB_PATH} is missing: build it with `python -c "import __graft_entry__ as g; g.build()"` '
                          '(or `python dust3r_amd/build.py`). dust3r_amd has no CPU fallback.')
    if not os.path.exists(HEADER_PATH):
        raise ImportError(f'{HEADER_PATH} is missing: the signatures of {os.path.basename(LIB_PATH)} are read from it.')
    lib = C.CDLL(LIB_PATH)
    with open(HEADER_PATH) as fh:
        sig = parse_header(fh.read())
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
