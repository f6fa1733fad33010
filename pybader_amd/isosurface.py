"""Isosurfaces by marching tetrahedra -- no counterpart in the reference.  The fields of the analysis side are looked at as
surfaces: the 0.001 a.u. envelope of the density with its area and its volume, in total and per atom (AIMAll's Vol(0.001)),
the zero envelopes of the Laplacian, the deformation density, the s = 0.5 surface of the NCI index coloured by
sign(lambda2) rho (nci.nci_isosurface).

The triangulation is the Freudenthal one of critical.py: six tetrahedra per cube of the periodic voxel lattice, no ambiguous
case, so the mesh is closed and consistently oriented across tiles and the cell boundary, and its Euler characteristic is twice
the alternating sum of the critical points above the level.  It runs in libbader_hip.so (xb_isosurface, csrc/k_isosurface.h); the
definition is in include/bader_hip.h and DESIGN.md section 21, and tests/test_isosurface_cpu.py restates it in numpy.

    isosurface(field, lattice, level, colour=None, volumes=None, n=0)    a Mesh"""
import numpy as np

from . import _lib, device
from .laplacian import _resident
from .utils import ensure_labels


def cartesian(p, shape, lattice):
    """Cartesian positions of the voxel coordinates `p` (f64[..., 3]), with the expression of critical.positions"""
    lat = np.asarray(lattice, dtype=np.float64).reshape(3, 3)
    p = np.asarray(p, dtype=np.float64)
    pos = np.empty(p.shape, np.float64)
    for j in range(3):
        c = lat[0, j] * p[..., 0] / np.float64(shape[0])
        c = c + lat[1, j] * p[..., 1] / np.float64(shape[1])
        c = c + lat[2, j] * p[..., 2] / np.float64(shape[2])
        pos[..., j] = c
    return pos


class Mesh:
    """A level set of a field on the grid, as triangles:

    shape, level, lattice
    vertices         f64[V, 3]    voxel coordinates, each in the frame of the voxel that owns its lattice edge
    positions        f64[V, 3]    the same, Cartesian
    colour           f64[V]       the second field interpolated onto the vertices, or None
    triangles        int64[T, 3]  vertex ids; the normal in voxel coordinates points from inside (field >= level) to outside
    wrap             uint16[T]    bit 3 corner + axis: that corner lies one cell further along the axis than its vertex says
    cells            int64[T]     the linear index of the cube the triangle lies in (colour or split a mesh by labels[cells])
    area, volume     the surface's area and the volume of the piecewise-linear inside region
    volume_by_label  f64[n]       that volume shared among the labels of the inside corners"""

    def __init__(self, shape, level, lattice, vertices, colour, triangles, wrap, cells, area, volume, volume_by_label):
        self.shape, self.level = tuple(int(s) for s in shape), float(level)
        self.lattice = np.array(lattice, dtype=np.float64).reshape(3, 3)
        self.vertices, self.colour, self.triangles, self.wrap, self.cells = vertices, colour, triangles, wrap, cells
        self.area, self.volume, self.volume_by_label = float(area), float(volume), volume_by_label
        self.positions = cartesian(vertices, self.shape, self.lattice)

    def __len__(self):
        return self.triangles.shape[0]

    def shifts(self):
        """int64[T, 3, 3]: per triangle, corner and axis the 0 / 1 of `wrap`"""
        bits = np.arange(9, dtype=np.uint16).reshape(3, 3)
        return ((self.wrap[:, None, None] >> bits) & 1).astype(np.int64)

    def corners_voxel(self):
        """f64[T, 3, 3]: the corners in voxel coordinates in the frame of the triangle's cube"""
        n = np.array(self.shape, dtype=np.float64)
        p = self.vertices[self.triangles]
        return np.where(self.shifts() != 0, p + n, p)

    def corners(self):
        """f64[T, 3, 3]: the Cartesian corners of every triangle, unwrapped (no triangle spans the cell)"""
        return cartesian(self.corners_voxel(), self.shape, self.lattice)

    @property
    def euler(self):
        """V - E + T, the edges counted as unordered vertex pairs"""
        t = self.triangles
        if t.shape[0] == 0:
            return 0
        e = np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]])
        e.sort(axis=1)
        n_edges = np.unique(e, axis=0).shape[0]
        return int(np.unique(t).shape[0] - n_edges + t.shape[0])

    def write_ply(self, path):
        """binary little-endian PLY of the unwrapped mesh: a vertex is written once per cell shift it is used with"""
        sh = self.shifts().reshape(-1, 3)
        ids = self.triangles.reshape(-1)
        key = ids * 8 + (sh[:, 0] * 4 + sh[:, 1] * 2 + sh[:, 2])
        uniq, inverse = np.unique(key, return_inverse=True)
        if uniq.shape[0] > np.iinfo(np.int32).max:
            raise ValueError(f'write_ply: {uniq.shape[0]} vertices do not fit the 32-bit face indices of the file')
        vid, code = uniq // 8, uniq % 8
        shift = np.stack([(code >> 2) & 1, (code >> 1) & 1, code & 1], axis=1).astype(np.float64)
        pos = cartesian(self.vertices[vid] + shift * np.array(self.shape, dtype=np.float64), self.shape, self.lattice)
        fields = [('x', '<f8'), ('y', '<f8'), ('z', '<f8')] + ([('colour', '<f8')] if self.colour is not None else [])
        v = np.zeros(uniq.shape[0], dtype=fields)
        v['x'], v['y'], v['z'] = pos[:, 0], pos[:, 1], pos[:, 2]
        if self.colour is not None:
            v['colour'] = self.colour[vid]
        f = np.zeros(self.triangles.shape[0], dtype=[('n', 'u1'), ('v', '<i4', (3,))])
        f['n'] = 3
        f['v'] = inverse.reshape(-1, 3)
        header = ['ply', 'format binary_little_endian 1.0', f'comment level {self.level!r}', f'element vertex {v.shape[0]}']
        header += [f'property double {name}' for name, _ in fields]
        header += [f'element face {f.shape[0]}', 'property list uchar int vertex_indices', 'end_header']
        with open(path, 'wb') as out:
            out.write(('\n'.join(header) + '\n').encode('ascii'))
            out.write(v.tobytes())
            out.write(f.tobytes())


def _on_device(ctx, a, what):
    """a float64 C-contiguous device array with the content of `a` (a host array goes through a scratch upload)"""
    if device.is_device_array(a):
        return a
    a = np.ascontiguousarray(a, dtype=np.float64)
    if a.shape != ctx.shape:
        raise ValueError(f'isosurface: the {what} has shape {a.shape}, the grid {ctx.shape}')
    return ctx.device_copy(a)


def isosurface(field, lattice, level, colour=None, volumes=None, n=0, gather=False, density=None):
    """The surface `field` == `level` in the cell `lattice` (a row per axis); inside is field >= level.

    field     host array, or a float32 / float64 device array: it becomes the resident density, as in the other analyses --
              unless `density` names the resident one (inside utils.resident() nothing is uploaded again); then `field` is
              another field on the same grid: a float64 C-contiguous device array is read where it is, a host array goes through
              a scratch upload
    colour    None, or a second field on the same grid (host, or float64 C-contiguous on the device) interpolated onto the vertices
    volumes   with n >= 1: the label map (host or device) whose labels 0 .. n - 1 share the inside volume
    gather    the second implementation: the same results

    A device field or colour is read on the context's stream after everything queued so far on the array's own stream (its
    __cuda_array_interface__ entry, else the one of device.on_stream): a tensor still being made there is waited for.

    -> Mesh (host arrays)"""
    ctx, shape = _resident(field if density is None else density)
    fdev = None
    if density is not None:
        if tuple(int(s) for s in field.shape) != shape:
            raise ValueError(f'isosurface: the field has shape {tuple(field.shape)}, the density {shape}')
        fdev = _on_device(ctx, field, 'field')
    cdev = None if colour is None else _on_device(ctx, colour, 'colour')
    n = int(n)
    if n >= 1:
        if volumes is None or tuple(int(s) for s in volumes.shape) != shape:
            raise ValueError('isosurface: n >= 1 needs a label map of the field\'s shape')
        ensure_labels(ctx, volumes)
    out = ctx.isosurface(lattice, level, fdev, cdev, max(n, 0), gather)
    ctx.isosurface_release()
    return Mesh(shape, level, lattice, *out)
