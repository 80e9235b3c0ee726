"""Builds dust3r_amd/csrc/libdust3r_hip.so for gfx950 with hipcc (in-tree, so the library travels
with the repository snapshot). Cross-compiles without a GPU."""
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, 'csrc')
SOURCES = ['gemm.hip', 'gemm_p4.hip', 'gemm_p4_heads.hip', 'gemm_up2.hip', 'attention.hip', 'elementwise.hip', 'aligner.hip', 'bootstrap.hip', 'sky.hip', 'visloc.hip', 'mesh.hip', 'fuse.hip', 'cloud_nn.hip', 'cloud_knn.hip', 'cloud_icp.hip', 'cloud_cluster.hip', 'cloud_features.hip', 'cloud_planes.hip', 'tracks.hip', 'gallery.hip', 'render.hip', 'losses.hip', 'views.hip', 'engine.hip', 'capi.hip']
HEADERS = ['common.hpp', 'reduce.hpp', 'scene_common.hpp', 'kernels.hpp', 'gemm_plan.hpp', 'gemm_p4.hpp', 'gemm_head4.hpp', 'aligner_math.hpp', 'visloc_math.hpp', 'ransac.hpp', 'views_math.hpp', 'gallery_math.hpp', 'fuse_grid.hpp', 'cloud_grid.hpp', os.path.join('..', '..', 'include', 'dust3r_hip.h')]
LIB = os.path.join(CSRC, 'libdust3r_hip.so')
FLAGS = ['--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC', '-Wno-unused-result', '-Wno-inline-asm']
# attention.hip: no SLP vectorisation -- its scalar-VALU softmax slices (attention_x3_kernel<..., SC = true>) must stay v_fma_f32 / v_add_f32
# pairs; hipcc -O3 re-packs adjacent scalar fp32 operations into v_pk_* (an anti-lever beside MFMAs, MI355X_MICROARCH.md). The packed
# variants of the same kernel use explicit 2-vectors and are not affected.
EXTRA_FLAGS = {'attention.hip': ['-fno-slp-vectorize'], 'gemm_p4.hip': ['-fno-slp-vectorize', '-Rpass-analysis=kernel-resource-usage'],     # gemm_p4.hip: its drain's scalar GELU pieces sit between MFMAs too
               'gemm_p4_heads.hip': ['-fno-slp-vectorize', '-Rpass-analysis=kernel-resource-usage'],      # the same kernel body: the same flags
               'gemm_up2.hip': ['-Rpass-analysis=kernel-resource-usage'],     # gemm_up2.hip: its report shows the fused x2 + convolution kernel keeps its accumulators in registers (tests read it)
               'aligner.hip': ['-Rpass-analysis=kernel-resource-usage'],      # aligner.hip: its report pins the registers / scratch of every aligner kernel (tests read it)
               'sky.hip': ['-Rpass-analysis=kernel-resource-usage'],          # sky.hip: its report shows the segmentation kernels use no scratch (tests read it)
               'visloc.hip': ['-Rpass-analysis=kernel-resource-usage'],       # visloc.hip: same for the matching / PnP-RANSAC kernels
               'mesh.hip': ['-Rpass-analysis=kernel-resource-usage'],         # mesh.hip: same for the GLB export kernels
               'fuse.hip': ['-Rpass-analysis=kernel-resource-usage', '-ffp-contract=off'],         # fuse.hip: same for scene.fuse(); its fp32 keys and fp64 sums round as numpy's do
               'cloud_nn.hip': ['-Rpass-analysis=kernel-resource-usage', '-ffp-contract=off'],     # cloud_nn.hip: same for the cloud metrics; its fp32 distances round as numpy's do
               'cloud_knn.hip': ['-Rpass-analysis=kernel-resource-usage', '-ffp-contract=off'],    # cloud_knn.hip: same for the k neighbours, normals and their orientation
               'cloud_icp.hip': ['-Rpass-analysis=kernel-resource-usage', '-ffp-contract=off'],    # cloud_icp.hip: same for the registration's transform and sums; its fp64 terms round as numpy's do
               'cloud_cluster.hip': ['-Rpass-analysis=kernel-resource-usage', '-ffp-contract=off'],    # cloud_cluster.hip: same for the density clustering's walks and its union-find
               'cloud_features.hip': ['-Rpass-analysis=kernel-resource-usage', '-ffp-contract=off'],   # cloud_features.hip: same for the global registration's descriptors, matching and RANSAC
               'cloud_planes.hip': ['-Rpass-analysis=kernel-resource-usage', '-ffp-contract=off'],     # cloud_planes.hip: same for the plane RANSAC and the support's moments
               'tracks.hip': ['-Rpass-analysis=kernel-resource-usage', '-ffp-contract=off'],       # tracks.hip: same for the 2-D tracks; its fp64 projection and fp32 distances round as numpy's do
               'gallery.hip': ['-Rpass-analysis=kernel-resource-usage', '-ffp-contract=off'],      # gallery.hip: same for the demo's gallery; its product and sum round separately, as numpy's do
               'render.hip': ['-Rpass-analysis=kernel-resource-usage'],       # render.hip: same for the rasteriser
               'losses.hip': ['-Rpass-analysis=kernel-resource-usage'],       # losses.hip: same for the criterion / median-selection kernels
               'views.hip': ['-Rpass-analysis=kernel-resource-usage']}        # views.hip: same for the dataset view-preparation kernels


def _hipcc():
    for cand in (os.environ.get('HIPCC'), '/opt/rocm/bin/hipcc', 'hipcc'):
        if cand and (os.path.isabs(cand) and os.path.exists(cand) or not os.path.isabs(cand)):
            return cand
    raise RuntimeError('hipcc not found')


def _stale(target, deps):
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(d) > t for d in deps)


def build(force=False, verbose=True):
    hipcc = _hipcc()
    hdrs = [os.path.join(CSRC, h) for h in HEADERS]
    flags = FLAGS + os.environ.get('D3R_BUILD_DEFINES', '').split()      # development: e.g. -DD3R_GEMM_ONLY_DT=3
    stamp = os.path.join(CSRC, '.build_flags')
    if not os.path.exists(stamp) or open(stamp).read() != ' '.join(flags):      # objects built with other flags: rebuild everything
        force = True
    objs, jobs = [], []
    for src in SOURCES:
        s = os.path.join(CSRC, src)
        o = os.path.join(CSRC, src.replace('.hip', '.o'))
        objs.append(o)
        if force or _stale(o, [s] + hdrs):
            jobs.append([hipcc] + flags + EXTRA_FLAGS.get(src, []) + ['-c', s, '-o', o])

    def run(cmd):
        if verbose:
            print(' '.join(cmd), flush=True)
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError(f'hipcc failed:\n{r.stdout}\n{r.stderr}')
        if '-Rpass-analysis=kernel-resource-usage' in cmd:      # the register / scratch report of the kernels of this file, kept next to the object (tests/test_host_cpu.py reads it)
            with open(os.path.splitext(cmd[-1])[0] + '.resources.txt', 'w') as f:
                f.write('\n'.join(ln for ln in r.stderr.splitlines() if 'remark:' in ln))
        return r

    with ThreadPoolExecutor(max_workers=min(6, max(1, len(jobs)))) as ex:
        list(ex.map(run, jobs))
    if force or jobs or _stale(LIB, objs):
        run([hipcc, '--offload-arch=gfx950', '-shared', '-fPIC', '-o', LIB] + objs)
    with open(stamp, 'w') as f:
        f.write(' '.join(flags))
    return LIB


if __name__ == '__main__':
    print(build(force='--force' in sys.argv))
