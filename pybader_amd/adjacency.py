"""Which atoms or Bader volumes share a surface, how large it is, and where the density on it is highest -- no counterpart in
the reference.  The highest point of the surface between two basins is the grid estimate of the bond critical point and of
rho_b; between two Bader volumes it is the barrier a persistence filter of spurious maxima needs.

The sweep runs in libbader_hip.so (xb_adjacency, csrc/k_adjacency.h); the definition is in include/bader_hip.h and DESIGN.md
section 14, and tests/test_adjacency_cpu.py restates it in numpy.  Every number is exact: facet counts are integers, the saddle
is a maximum of existing doubles, ties go to the smallest facet id.

    active_directions(voxel_lattice)                          the facet directions of the voxel lattice and their areas
    adjacency(density, volumes, lattice, n, voxel_offset)     an Adjacency
    persistence(pairs, saddle_density, maxima_density)                        per volume: its maximum minus its highest saddle to a higher volume"""
import numpy as np

from . import _lib
from .utils import ensure_density, ensure_labels
from .weight import _pair_offsets, voronoi_areas


def active_directions(voxel_lattice):
    """-> (dirs int32[K, 3], areas f64[K]): of the 13 offsets d > -d of {-1, 0, 1}^3, in ascending tuple order, those whose facet
    of the voxel lattice's Voronoi cell has an area (weight.voronoi_areas keeps those >= AREA_TOL * V_voxel^(2/3)).  K is 3 for
    an orthogonal cell and at most 7.  Raises ValueError on a lattice too skewed for 26 neighbours."""
    areas = voronoi_areas(voxel_lattice)
    keep = [d for d in _pair_offsets() if areas[tuple(x % 3 for x in d)] > 0.0]
    dirs = np.array(keep, dtype=np.int32).reshape(-1, 3)
    return dirs, np.array([areas[tuple(x % 3 for x in d)] for d in keep], dtype=np.float64)


def key(x):
    """the total order of the definition as uint64: equals < on ordinary values, -0.0 < +0.0, defined for NaN"""
    b = np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)
    return b ^ np.where(b >> np.uint64(63), np.uint64(0xFFFFFFFFFFFFFFFF), np.uint64(1 << 63))


def facet_area(facets, areas):
    """sum_k facets[:, k] * areas[k], left to right in float64"""
    facets = np.asarray(facets, dtype=np.int64)
    area = np.zeros(facets.shape[0], np.float64)
    for k in range(facets.shape[1]):
        term = facets[:, k].astype(np.float64) * np.float64(areas[k])
        area = term if k == 0 else area + term
    return area


def saddle_geometry(saddle_facet, dirs, shape, lattice, voxel_offset=None):
    """facet ids lin(v) * 8 + k -> (voxels int64[P, 2, 3]: v and its neighbour v + d_k, both wrapped;  position f64[P, 3]: the
    midpoint of the two voxel positions before wrapping, Cartesian -- the position of v as utils.surface_dist forms it
    (lat[0] p0 / nx, += lat[1] p1 / ny, += lat[2] p2 / nz) plus half of d_k . voxel_lattice, plus voxel_offset when given)"""
    f = np.asarray(saddle_facet, dtype=np.int64)
    dirs = np.asarray(dirs, dtype=np.int64).reshape(-1, 3)
    shape = tuple(int(s) for s in shape)
    lat = np.asarray(lattice, dtype=np.float64).reshape(3, 3)
    k = f % 8
    v = np.stack(np.unravel_index(f // 8, shape), axis=1).astype(np.int64).reshape(-1, 3)
    d = dirs[k].reshape(-1, 3)
    voxels = np.stack([v, (v + d) % np.array(shape, dtype=np.int64)], axis=1)
    vl = lat / np.array(shape, dtype=np.float64)[:, None]
    p, df = v.astype(np.float64), d.astype(np.float64)
    pos = np.empty((f.shape[0], 3), np.float64)
    for j in range(3):
        c = lat[0, j] * p[:, 0] / np.float64(shape[0])
        c = c + lat[1, j] * p[:, 1] / np.float64(shape[1])
        c = c + lat[2, j] * p[:, 2] / np.float64(shape[2])
        c = c + 0.5 * ((df[:, 0] * vl[0, j] + df[:, 1] * vl[1, j]) + df[:, 2] * vl[2, j])
        if voxel_offset is not None:
            c = c + np.float64(np.asarray(voxel_offset, dtype=np.float64)[j])
        pos[:, j] = c
    return voxels, pos


class Adjacency:
    """The pairs of labels that share a surface, in ascending (a, b) with a < b:

    dirs, areas       the active directions [K, 3] and their facet areas [K]
    pairs             int32[P, 2]
    facets            int64[P, K]   voxel facets of each direction on the surface
    area              f64[P]        sum_k facets[:, k] * areas[k] (in the squared length unit of the lattice)
    saddle_density    f64[P]        the highest value of min(rho[v], rho[u]) over the surface's facets
    saddle_facet      int64[P]      the smallest facet id lin(v) * 8 + k that reaches it
    saddle_voxels     int64[P, 2, 3]  that facet's voxel and its neighbour, wrapped
    saddle_position   f64[P, 3]     the midpoint of the two, Cartesian"""

    def __init__(self, n, dirs, areas, pairs, facets, saddle, saddle_facet, shape, lattice, voxel_offset):
        self.n = int(n)
        self.dirs, self.areas = dirs, areas
        self.pairs, self.facets = pairs, facets
        self.area = facet_area(facets, areas)
        self.saddle_density, self.saddle_facet = saddle, saddle_facet
        self.saddle_voxels, self.saddle_position = saddle_geometry(saddle_facet, dirs, shape, lattice, voxel_offset)

    def __len__(self):
        return self.pairs.shape[0]

    def neighbours(self, a):
        """the labels that share a surface with label `a`"""
        p = self.pairs
        return np.concatenate([p[p[:, 0] == a, 1], p[p[:, 1] == a, 0]])


def adjacency(density, volumes, lattice, n, voxel_offset=None):
    """The surfaces between the labels 0 .. n - 1 of `volumes`.

    density       the field the labels were made from: host array, or a float32 / float64 device array
    volumes       the label map, host or device array; labels < 0 and >= n bound no surface
    lattice       the CELL's lattice, one row per axis
    voxel_offset  Cartesian, added to saddle_position when given

    -> Adjacency; inside utils.resident() nothing is uploaded again."""
    ctx = _lib.default_context()
    shape = tuple(int(s) for s in volumes.shape)
    lattice = np.asarray(lattice, dtype=np.float64).reshape(3, 3)
    dirs, areas = active_directions(lattice / np.array(shape, dtype=np.float64)[:, None])
    if dirs.shape[0] > 8:
        raise ValueError(f'adjacency: {dirs.shape[0]} active directions; a facet id holds 8')
    if ctx.shape != shape:
        ctx.set_grid(shape, np.zeros(27), np.zeros(9))
    ensure_density(ctx, density)
    ensure_labels(ctx, volumes)
    if int(n) < 1:
        pairs, facets = np.zeros((0, 2), np.int32), np.zeros((0, dirs.shape[0]), np.int64)
        saddle, sfacet = np.zeros(0, np.float64), np.zeros(0, np.int64)
    else:
        pairs, facets, saddle, sfacet = ctx.adjacency(dirs, n)
    return Adjacency(n, dirs, areas, pairs, facets, saddle, sfacet, shape, lattice, voxel_offset)


def persistence(pairs, saddle_density, maxima_density):
    """per label m: maxima_density[m] minus the highest saddle (in key order) m shares with a label whose maximum is higher
    (in key order; two maxima of the same bits are not above each other); +inf without such a neighbour"""
    rho = np.asarray(maxima_density, dtype=np.float64)
    kmax = key(rho).tolist()
    out = np.full(rho.shape[0], np.inf)
    best = {}
    sd = np.asarray(saddle_density, dtype=np.float64)
    for (a, b), s, k in zip(np.asarray(pairs).tolist(), sd.tolist(), key(sd).tolist()):
        if kmax[a] == kmax[b]:
            continue
        lower = a if kmax[a] < kmax[b] else b
        if lower not in best or k > best[lower][0]:
            best[lower] = (k, s)
    for m, (_, s) in best.items():
        out[m] = rho[m] - s
    return out
