"""The padded layout: per-view maps of different sizes as rows of one tensor -- what every batched scene kernel takes (d3r_clean_pointcloud,
d3r_segment_sky, d3r_scene_mesh, d3r_scene_gallery) and what a scene keeps (`_im_conf`, `_flat_im_depthmaps`, `get_depthmaps(raw=True)`,
`get_pts3d(raw=True)`). This module is the one place that pads, slices back and builds the shape tables; `viz.ingest_views` is the one
ingestion built on it (images, pointmaps, masks and weights of a batched scene call, lists or ready stacks, to stacks and tables). The contract:
- a stack is a contiguous (n, row, *tail) tensor; view i of shape (h, w) is `stack[i, :h * w]` in raster order;
- row >= every h * w; the rows made here and the scene's are multiples of 4 (the float4 loads of d3r_scene_gallery need that; an explicit
  `row` is taken as given: the mesh and sky kernels take any), and the base address is 16-byte aligned (as every tensor torch allocates);
- WHAT LIES BEHIND A VIEW'S h * w ELEMENTS IS UNSPECIFIED, AND NO CONSUMER MAY READ IT INTO A RESULT. `pad_views` writes zeros there, the
  optimiser's depth rows hold what the last step left, PairViewer's are never written. The kernels bound themselves by the tables:
  clean_pointcloud_kernel by Hs[i] * Ws[i] and 0 <= (u, v) < (Ws[j], Hs[j]); the mesh kernels by area_of / elems_of (a quad's four pixels
  lie inside h * w); the sky kernels by 0 <= y < H, 0 <= x < W; the gallery kernels by npix (lanes of a float4 past it are dropped);
- the tables are int32 device tensors (heights, widths, npix), rows of one (3, n) upload."""
import numpy as np
import torch


def pad_views(maps, device, dtype, tail=(), row=None, shapes=None, name='map'):
    """A list of (H, W, *tail) maps (numpy arrays or tensors, anywhere) -> the zero-padded contiguous (n, row, *tail) stack on `device`, one
    copy per map. row: by default the largest area rounded up to a multiple of 4. shapes: the (h, w) each map must have the elements of,
    when not its own. A map of another size raises a ValueError that says which (`name` and the index). A tensor that already is such a
    stack (one dimension fewer than a stack of maps) is checked against `row` / `shapes` and passed on, converted only where it has to be."""
    tail = tuple(int(t) for t in tail)
    if isinstance(maps, torch.Tensor) and maps.ndim == 2 + len(tail):
        need = max((h * w for h, w in shapes), default=0) if shapes is not None else 0
        if tuple(maps.shape[2:]) != tail or maps.shape[1] != (row or maps.shape[1]) or maps.shape[1] < need:
            raise ValueError(f'{name}: padded stack {tuple(maps.shape)} for rows of {row} and views of up to {need} pixels')
        return maps.detach().to(device=device, dtype=dtype).contiguous()
    maps = [m.detach() if isinstance(m, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(m)) for m in maps]
    shapes = [tuple(m.shape[:2]) for m in maps] if shapes is None else shapes
    areas = [int(h) * int(w) for h, w in shapes]
    for i, (m, a) in enumerate(zip(maps, areas)):
        if m.numel() != a * int(np.prod(tail, dtype=np.int64)):
            raise ValueError(f'{name} {i} has shape {tuple(m.shape)}, its view {tuple(shapes[i]) + tail}')
    if row is None:
        row = -(-max(areas) // 4) * 4
    elif row < max(areas):
        raise ValueError(f'{name}: rows of {row} for views of up to {max(areas)} pixels')
    out = torch.zeros((len(maps), row) + tail, dtype=dtype, device=device)
    for i, (m, a) in enumerate(zip(maps, areas)):
        out[i, :a] = m.reshape((a,) + tail)
    return out


def split_views(stack, shapes):
    """The list of (h, w, *tail) views `stack[i, :h * w]` of a padded stack: no copy, writes go to the stack."""
    return [stack[i, :h * w].view((h, w) + tuple(stack.shape[2:])) for i, (h, w) in enumerate(shapes)]


def zero_padding_(stack, areas):
    """Zeros behind every row's own length, in place: for the stacks whose padding IS specified (the aligner's pixel weights)."""
    for i, a in enumerate(areas):
        if a < stack.shape[1]:
            stack[i, a:] = 0
    return stack


def shape_tables(shapes, device):
    """(heights, widths, npix) of the views as int32 tensors on `device`: one host array, one upload."""
    table = np.array([[h for h, w in shapes], [w for h, w in shapes], [h * w for h, w in shapes]], dtype=np.int32)
    return tuple(torch.from_numpy(table).to(device))
