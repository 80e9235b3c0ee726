"""A glTF 2.0 binary (.glb) writer for the demo's scene export, in plain Python (struct, json, numpy; PIL encodes the textures).

The file is one JSON chunk and one BIN chunk. Every bufferView starts on a 4-byte boundary, both chunks are padded to 4 bytes (the JSON with
spaces, the BIN with zeros), and bulk arrays go to the file straight from their host buffers through memoryview: nothing is concatenated
into one bytes object. The total size is known before the file is opened; past the header's uint32 length it is a ValueError."""
import json
import struct

import numpy as np

GLB_MAGIC = 0x46546C67           # b'glTF'
CHUNK_JSON = 0x4E4F534A
CHUNK_BIN = 0x004E4942
MAX_BYTES = 2 ** 32 - 1          # the header's uint32 length

FLOAT, UNSIGNED_INT, UNSIGNED_BYTE = 5126, 5125, 5121
ARRAY_BUFFER, ELEMENT_ARRAY_BUFFER = 34962, 34963
TRIANGLES, POINTS = 4, 0


def _pad4(n):
    return (n + 3) & ~3


def _as(a, dtype):
    """`a` itself when it already has the dtype (no copy, whatever its strides: the file gets contiguous bytes at write time)"""
    a = np.asarray(a)
    return a if a.dtype == dtype else a.astype(dtype)


class GlbBuilder:
    """Collects nodes, meshes, accessors and binary pieces; `write(path)` lays them out. Arrays are kept by reference until written."""

    def __init__(self):
        self.doc = dict(asset=dict(version='2.0', generator='dust3r_amd'), scene=0, scenes=[dict(nodes=[])], nodes=[], meshes=[],
                        accessors=[], bufferViews=[], buffers=[])
        self.pieces = []            # (byte offset in BIN, array or bytes)
        self.size = 0               # BIN bytes so far (4-byte aligned)

    def _list(self, key):
        return self.doc.setdefault(key, [])

    def buffer_view(self, data, target=None):
        nbytes = data.nbytes if isinstance(data, np.ndarray) else len(data)
        view = dict(buffer=0, byteOffset=self.size, byteLength=int(nbytes))
        if target is not None:
            view['target'] = target
        self.pieces.append((self.size, data))
        self.size = _pad4(self.size + int(nbytes))
        self.doc['bufferViews'].append(view)
        return len(self.doc['bufferViews']) - 1

    def accessor(self, array, component, kind, target=None, normalized=False, bounds=None):
        """array: numpy rows (count x width); bounds: (min, max) written as the accessor's min / max"""
        count = array.shape[0] if kind != 'SCALAR' else array.size
        acc = dict(bufferView=self.buffer_view(array, target), componentType=component, count=int(count), type=kind)
        if normalized:
            acc['normalized'] = True
        if bounds is not None:          # JSON has no inf / NaN: 0 where a component had no finite value (degenerate, NaN pointmaps)
            acc['min'] = [float(v) if np.isfinite(v) else 0.0 for v in bounds[0]]
            acc['max'] = [float(v) if np.isfinite(v) else 0.0 for v in bounds[1]]
        self.doc['accessors'].append(acc)
        return len(self.doc['accessors']) - 1

    def positions(self, xyz, bounds=None):
        xyz = _as(xyz, np.float32)
        if bounds is None:
            bounds = (xyz.min(axis=0), xyz.max(axis=0))
        return self.accessor(xyz, FLOAT, 'VEC3', ARRAY_BUFFER, bounds=bounds)

    def colors(self, rgba):
        return self.accessor(_as(rgba, np.uint8), UNSIGNED_BYTE, 'VEC4', ARRAY_BUFFER, normalized=True)

    def indices(self, faces):
        return self.accessor(_as(faces, np.uint32), UNSIGNED_INT, 'SCALAR', ELEMENT_ARRAY_BUFFER)

    def material(self, **pbr):
        pbr.setdefault('metallicFactor', 0.0)
        self._list('materials').append(dict(pbrMetallicRoughness=pbr))
        return len(self.doc['materials']) - 1

    def texture(self, png_bytes):
        if 'samplers' not in self.doc:
            self.doc['samplers'] = [dict(magFilter=9729, minFilter=9729)]        # LINEAR
        self._list('images').append(dict(bufferView=self.buffer_view(png_bytes), mimeType='image/png'))
        self._list('textures').append(dict(sampler=0, source=len(self.doc['images']) - 1))
        return len(self.doc['textures']) - 1

    def mesh(self, attributes, indices=None, mode=TRIANGLES, material=None):
        prim = dict(attributes=attributes, mode=mode)
        if indices is not None:
            prim['indices'] = indices
        if material is not None:
            prim['material'] = material
        self.doc['meshes'].append(dict(primitives=[prim]))
        return len(self.doc['meshes']) - 1

    def node(self, **kw):
        self.doc['nodes'].append(kw)
        return len(self.doc['nodes']) - 1

    def _json_bytes(self):
        doc = dict(self.doc)
        doc['buffers'] = [dict(byteLength=self.size)] if self.size else []
        for key in ('meshes', 'accessors', 'bufferViews', 'buffers'):
            if not doc[key]:
                del doc[key]
        raw = json.dumps(doc, separators=(',', ':')).encode()
        return raw + b' ' * (_pad4(len(raw)) - len(raw))

    def write(self, path):
        js = self._json_bytes()
        total = 12 + 8 + len(js) + (8 + self.size if self.size else 0)
        if total > MAX_BYTES:
            raise ValueError(f'the GLB file would be {total} bytes, past the format\'s 4 GiB limit ({MAX_BYTES} bytes): export fewer points '
                             f'(as_pointcloud=True, or a higher min_conf_thr)')
        with open(path, 'wb') as f:
            f.write(struct.pack('<III', GLB_MAGIC, 2, total))
            f.write(struct.pack('<II', len(js), CHUNK_JSON))
            f.write(js)
            if self.size:
                f.write(struct.pack('<II', self.size, CHUNK_BIN))
                at = 0
                for off, data in self.pieces:
                    if off > at:
                        f.write(b'\0' * (off - at))
                    mv = memoryview(np.ascontiguousarray(data) if isinstance(data, np.ndarray) else data).cast('B')
                    f.write(mv)
                    at = off + mv.nbytes
                if self.size > at:
                    f.write(b'\0' * (self.size - at))
        return total
