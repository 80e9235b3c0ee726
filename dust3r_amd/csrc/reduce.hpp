// dust3r_amd -- the fixed-order primitives of the scene and cloud kernels (bootstrap, losses, sky, visloc, mesh, fuse, the cloud files, tracks,
// gallery): ONE definition of the workgroup reduction, of the wave scan, of the workspace carving and of the grid arithmetic. Every result
// that promises "the same bytes on every run" (and the bytes of a numpy restatement) rests on the order stated here, once:
//   wave    an xor butterfly over the 64 lanes, offsets 32, 16, 8, 4, 2, 1: every lane ends with the same value, the tree
//           ((l, l ^ 32), then ^ 16, ... ^ 1). Lane 0 of a __shfl_down ladder 32..1 computes the same tree.
//   block   lane 0 of wave w leaves the wave's value of column k in lds[w * NV + k]; one barrier; column k is combined over the waves
//           0, 1, ..., NT / 64 - 1 in ascending order, starting from wave 0's value.
// `op` is the caller's: op(a, b) for a wave, op(a, b, k) with the column k for a workgroup (the bounds take a minimum in columns 0-2 and a
// maximum in 3-5). NaN behaviour is therefore the op's, nothing here adds any. Header-only and D3R_DEV: each object keeps its own copies.
// Defined once in the same way, next to what they serve: the fp32 3-vector arithmetic and the finite / usable-normal tests of the cloud
// kernels (fuse_grid.hpp), the sampler and the round scorer of the two RANSACs (ransac.hpp).
#pragma once
#include <algorithm>
#include "common.hpp"

namespace d3r {

struct Sum {
    template <class T> D3R_DEV T operator()(T a, T b, int = 0) const { return a + b; }
};

template <class T, class Op> D3R_DEV T wave_reduce(T v, Op op) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = op(v, __shfl_xor(v, o));
    return v;
}
// NV columns at once, column k with op(a, b, k): the same tree per column
template <int NV, class T, class Op> D3R_DEV void wave_reduce(T (&v)[NV], Op op) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
        for (int k = 0; k < NV; ++k) v[k] = op(v[k], __shfl_xor(v[k], o), k);
    }
}

// the first half of a workgroup reduction: v[k] becomes its wave's value (in every lane), lane 0 leaves it in lds[wave * NV + k]. The caller
// places the barrier, so that reductions of several types (the fp64 and int64 columns of the cloud sums) share one.
template <int NV, class T, class Op> D3R_DEV void block_reduce_stage(T (&v)[NV], T* lds, Op op) {
    wave_reduce(v, op);
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int k = 0; k < NV; ++k) lds[(threadIdx.x >> 6) * NV + k] = v[k];
    }
}

// the second half, behind the barrier: column k over the waves in ascending order
template <int NT, int NV, class T, class Op> D3R_DEV T block_reduce_column(const T* lds, int k, Op op) {
    T r = lds[k];
    for (int w = 1; w < NT / 64; ++w) r = op(r, lds[w * NV + k], k);
    return r;
}

// column k by thread k -> out[k] (NV <= NT). No trailing barrier: lds is the caller's to reuse only behind one of its own.
template <int NT, int NV, class T, class Op> D3R_DEV void block_reduce_columns(T (&v)[NV], T* lds, Op op, T* out) {
    static_assert(NV <= NT, "one thread per column");
    block_reduce_stage(v, lds, op);
    __syncthreads();
    if (threadIdx.x < NV) out[threadIdx.x] = block_reduce_column<NT, NV>(lds, threadIdx.x, op);
}

// every column into v[] of thread 0 (ALL = false: v[] of the other threads holds their wave's value) or of every thread (ALL = true).
// No trailing barrier either.
template <int NT, bool ALL, int NV, class T, class Op> D3R_DEV void block_reduce_gather(T (&v)[NV], T* lds, Op op) {
    block_reduce_stage(v, lds, op);
    __syncthreads();
    if (ALL || threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < NV; ++k) v[k] = block_reduce_column<NT, NV>(lds, k, op);
    }
}

// inclusive scan over the wave (the __shfl_up ladder 1, 2, ..., 32): lane l gets v_0 + ... + v_l. Integers: int and long long.
template <class T> D3R_DEV T wave_scan_inclusive(T v, int lane) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const T t = __shfl_up(v, o);
        if (lane >= o) v += t;
    }
    return v;
}

// ---- a workspace carved into 256-byte aligned arrays, in the order of the calls. A null base gives null pointers and the same bytes,
// which is how every *_workspace_bytes export sizes what its call carves. Host code, and the kernels of visloc.hip that carve their job's record.
struct Carver {
    char* base;
    size_t bytes = 0;
    __host__ __device__ explicit Carver(void* b) : base((char*)b) {}
    template <class T> __host__ __device__ T* take(size_t count) {
        T* r = base ? (T*)(base + bytes) : nullptr;
        bytes += align256(count * sizeof(T));
        return r;
    }
};

// the tiles of `per` elements that cover n, and the grid of a grid-stride launch over them: at least one workgroup, at most cap
static inline long long tiles_of(long long n, int per) { return (n + per - 1) / per; }
static inline int blocks_of(long long tiles, int cap) { return (int)std::max(1LL, std::min(tiles, (long long)cap)); }

}  // namespace d3r
