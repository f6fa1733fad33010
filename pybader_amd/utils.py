"""Host-side mirror of the njit half of pybader/utils.py that sits on the hot path.

Same names, argument order and in-place behaviour as the reference; the sweeps run in
libbader_hip.so on the GPU (no CPU fallback)."""
import numpy as np

from . import _lib, device

def dtype_calc(max_val):
    """utils.dtype_calc (utils.py:15-37): smallest dtype holding max_val; a negative argument asks
    for a signed type able to hold 2*|max_val|."""
    signed = max_val < 0
    if signed:
        max_val *= -2
    width = 0 if max_val <= 255 else 1 if max_val <= 65535 else 2 if max_val <= 4294967295 else 3
    return ('int8', 'int16', 'int32', 'int64')[width] if signed else ('uint8', 'uint16', 'uint32', 'uint64')[width]


# ---- which host array is resident on the device -------------------------------------------------------------
# The reference passes the same `density` ndarray to bader_calc, refine and charge_sum.  By default every call
# uploads it again (about 0.1 s per GiB): nothing is assumed about the content of a host array.  A caller who
# holds the array still for a while says so with `resident(density)`: inside that block the array is uploaded
# once, is read-only (an in-place edit raises instead of being missed) and is recognised by identity (address,
# shape, strides).  The token lives in the Context, and every route that rewrites the device density (upload,
# CHGCAR text parse -- also a failed one --, synthetic generator) clears it; so does a change of the grid's shape,
# which drops the device density (a call that reads no density, such as volume_assign on a map of another shape,
# changes the grid without uploading one).
def _identity(a):
    return (a.ctypes.data, a.shape, a.strides)


class resident:
    """with resident(density): ... -- a promise not to modify `density` inside the block; uploaded at most once."""

    def __init__(self, density, ctx=None):
        self.array = density
        self.ctx = ctx

    def __enter__(self):
        a = self.array
        if device.is_device_array(a):
            # a device array (pybader_amd/device.py): imported once inside the block, recognised by pointer, shape, strides
            # and dtype.  The library cannot make device memory read-only: not writing it is the caller's promise.
            self.ctx = self.ctx or _lib.default_context()
            self._was_writeable = False
            self.ctx.pinned_density = device.describe(a).identity
            return a
        if not (isinstance(a, np.ndarray) and a.dtype == np.float64 and a.flags.c_contiguous):
            raise ValueError('resident(): a C-contiguous float64 ndarray is required')
        self.ctx = self.ctx or _lib.default_context()
        self._was_writeable = bool(a.flags.writeable)
        a.flags.writeable = False
        self.ctx.pinned_density = _identity(a)
        return a

    def __exit__(self, *exc):
        release_labels(self.ctx)
        self.ctx.pinned_density = None
        self.ctx.resident_density = None
        if self._was_writeable:
            self.array.flags.writeable = True
        return False


# ---- device arrays (pybader_amd/device.py) at the same entry points ---------------------------------------------------
# A density that is a device array is imported (device to device) where a host array is uploaded; label maps and masked
# volumes then come back as device.DeviceArray.  A label map is tracked inside resident() like a host one, by identity
# of the object and of its pointer, shape and dtype -- without the read-only flag a host array gets: see device.py.
def dev_reusable(volumes, dtype):
    """can the device array `volumes` take the result in place (as a host array of the right dtype does)?"""
    d = device.describe(volumes)
    return d.dtype == dtype and d.c_contiguous and not d.readonly


def label_dtype(volumes):
    return device.describe(volumes).dtype if device.is_device_array(volumes) else volumes.dtype


# ---- the label array on the device -------------------------------------------------------------------------------
# bader_calc -> refine -> charge_sum -> assign_to_atoms hand the SAME host label array from call to call
# (interface.py:406-416); uploading and downloading it every time made the drop-in PCIe-bound (22.6 ms per
# bader_calc + refine pair at 256^3 against 1 ms resident).  Inside a `resident(density)` block the library keeps track of
# the one host array whose content equals the device labels: it is recognised by identity (address, shape, strides,
# dtype), it is READ-ONLY while the token lives (numpy raises on a write instead of the copy going stale; the library's own
# in-place updates lift the flag for the duration of the download), the context holds a reference to it (its address
# cannot be reused), and every device call that rewrites the labels drops the token.  Outside such a block nothing is
# assumed: every call uploads.
def _lab_identity(a):
    return (a.ctypes.data, a.shape, a.strides, a.dtype.str)


def release_labels(ctx):
    ctx.drop_label_token()


def track_labels(ctx, volumes):
    """the device labels equal `volumes` (just uploaded from it / downloaded into it)"""
    release_labels(ctx)
    if device.is_device_array(volumes):
        d = device.describe(volumes)
        if ctx.pinned_density is not None and d.c_contiguous:
            ctx._labels_host, ctx._labels_was_writeable = volumes, False
            ctx.resident_labels = d.identity
        return
    # (a view of a writeable array is not tracked: a write through its base would leave the device copy stale unnoticed)
    if (ctx.pinned_density is not None and isinstance(volumes, np.ndarray) and volumes.flags.c_contiguous
            and (_lib.pool_owned(volumes) or not (isinstance(volumes.base, np.ndarray) and volumes.base.flags.writeable))):
        ctx._labels_host, ctx._labels_was_writeable = volumes, bool(volumes.flags.writeable)
        volumes.flags.writeable = False
        ctx.resident_labels = _lab_identity(volumes)


def labels_resident(ctx, volumes):
    if device.is_device_array(volumes):
        return (ctx.pinned_density is not None and getattr(ctx, '_labels_host', None) is volumes
                and ctx.resident_labels == device.describe(volumes).identity)
    return (ctx.pinned_density is not None and getattr(ctx, '_labels_host', None) is volumes and not volumes.flags.writeable
            and ctx.resident_labels == _lab_identity(volumes))


def ensure_labels(ctx, volumes):
    """make `volumes` the device labels: uploads unless it is the tracked array"""
    if labels_resident(ctx, volumes):
        return
    if device.is_device_array(volumes):
        ctx.import_labels(volumes)
    else:
        ctx.upload_labels(volumes)
    track_labels(ctx, volumes)


def fetch_labels(ctx, out=None, dtype=None, on_device=False):
    """device labels -> host (in place into `out`, else a new array of `dtype`), and track the result; into the device
    array `out`, or with `on_device` into a new device.DeviceArray, the labels stay on the card"""
    release_labels(ctx)
    if on_device or device.is_device_array(out):
        out = ctx.export_labels(dtype, out=out)
        track_labels(ctx, out)
        return out
    out = ctx.download_labels(out=out) if out is not None else ctx.download_labels(dtype, pooled=True)
    track_labels(ctx, out)
    return out


def ensure_density(ctx, density):
    """Make `density` the device density: uploads, unless the caller pinned this very array with `resident()` and
    it is the one on the device.  A device array is imported instead (any strides, float32 or float64)."""
    if device.is_device_array(density):
        ident = device.describe(density).identity
        if ctx.pinned_density is not None and ctx.pinned_density == ident and ctx.resident_density == ident:
            return density
        ctx.import_density(density)             # clears ctx.resident_density
        if ctx.pinned_density == ident:
            ctx.resident_density = ident
        return density
    density = np.ascontiguousarray(density, dtype=np.float64)
    ident = _identity(density)
    if ctx.pinned_density is not None and ctx.pinned_density == ident and ctx.resident_density == ident:
        return density
    ctx.upload_density(density)                 # clears ctx.resident_density
    if ctx.pinned_density == ident:
        ctx.resident_density = ident
    return density


def remember_density(ctx, density):
    """`density` (a pinned host array) was just downloaded from the context: it is the resident one."""
    if ctx.pinned_density is not None and ctx.pinned_density == _identity(density):
        ctx.resident_density = _identity(density)


def forget_density(ctx):
    ctx.resident_density = None


def vacuum_assign(reference, volumes, vac_tol, density, voxel_volume):
    """utils.vacuum_assign (utils.py:382-401): volumes[reference <= vac_tol] = -1; returns
    (volumes, vacuum charge, vacuum volume).  `volumes` is updated in place.

    With a device array as `density` the map comes back as a device.DeviceArray; `volumes` may then be None (a fresh
    map of dtype_calc(-N), all zero before the vacuum is marked), a host array or a device array."""
    if device.is_device_array(density) or device.is_device_array(reference):
        return _vacuum_assign_device(reference, volumes, vac_tol, density, voxel_volume)
    ctx = _lib.default_context()
    if ctx.shape != tuple(volumes.shape):
        ctx.set_grid(volumes.shape, np.zeros(27), np.zeros(9))
    same = reference is density or (reference.shape == density.shape and np.shares_memory(reference, density))
    ensure_density(ctx, reference)
    release_labels(ctx)
    charge, volume = ctx.vacuum_assign(vac_tol, voxel_volume)
    if not same and volume:
        # vacuum is decided on `reference`, its charge is summed over `density` (utils.py:396-400)
        ensure_density(ctx, density)
        s, n = ctx.label_sum(-1)
        charge, volume = s * voxel_volume, n * voxel_volume
    # the device sets non-vacuum voxels to 0; the reference leaves them untouched
    if _lib.fast_any(volumes):
        keep = volumes.copy()
        ctx.download_labels(out=volumes)
        np.copyto(volumes, keep, where=volumes != -1)
    else:
        if volume:                       # some voxel became vacuum: fetch the -1 marks
            ctx.download_labels(out=volumes)
        track_labels(ctx, volumes)       # all zeros before, so host == device now (also without a download)
    return volumes, charge, volume


def _same_array(a, b):
    if a is b:
        return True
    if device.is_device_array(a) != device.is_device_array(b):
        return False
    if device.is_device_array(a):
        return device.describe(a).identity == device.describe(b).identity
    return a.shape == b.shape and np.shares_memory(a, b)


def _vacuum_assign_device(reference, volumes, vac_tol, density, voxel_volume):
    ctx = _lib.default_context()
    shape = tuple(int(n) for n in density.shape)
    if ctx.shape != shape:
        ctx.set_grid(shape, np.zeros(27), np.zeros(9))
    ensure_density(ctx, reference)
    release_labels(ctx)
    charge, volume = ctx.vacuum_assign(vac_tol, voxel_volume)
    if not _same_array(reference, density) and volume:
        ensure_density(ctx, density)            # utils.py:396-400: the vacuum's charge is summed over `density`
        s, n = ctx.label_sum(-1)
        charge, volume = s * voxel_volume, n * voxel_volume
    if volumes is None:
        dtype, keep = np.dtype(dtype_calc(-int(np.prod(shape)))), None
    else:
        dtype = label_dtype(volumes)
        keep = device.to_host(volumes, ctx) if device.is_device_array(volumes) else volumes
        if not _lib.fast_any(keep):
            keep = None
    if keep is not None:
        # the reference leaves the non-vacuum voxels of a map that already holds labels untouched: merged on the host
        # (no caller on the hot path hands such a map in)
        merged = ctx.download_labels(dtype)
        np.copyto(merged, keep, where=merged != -1)
        ctx.upload_labels(merged)
    out = volumes if device.is_device_array(volumes) and dev_reusable(volumes, dtype) else None
    return fetch_labels(ctx, out, dtype, on_device=True), charge, volume


def charge_sum(charge, volume, voxel_volume, density, volumes):
    """utils.charge_sum (utils.py:235-252): in place on `charge` / `volume` like the reference."""
    ctx = _lib.default_context()
    if ctx.shape != tuple(volumes.shape):
        ctx.set_grid(volumes.shape, np.zeros(27), np.zeros(9))
    ensure_density(ctx, density)
    ensure_labels(ctx, volumes)
    ch, vo = ctx.charge_sum(voxel_volume, charge.shape[0])
    # utils.py:251-252 scales the accumulated charge (whatever it held on entry) by voxel_volume
    charge *= voxel_volume
    charge += ch
    volume += vo


def atom_assign(bader_max, atoms, lattice, i_c=None):
    """utils.atom_assign (utils.py:185-232) -> (assigned_atom int64[N], assigned_distance f64[N])."""
    return _lib.atom_assign(bader_max, atoms, lattice)


def volume_assign(volumes, swap, i_c=None):
    """utils.volume_assign (utils.py:404-421): volumes[v] = swap[volumes[v]] for labels >= 0, in place."""
    ctx = _lib.default_context()
    if ctx.shape != tuple(volumes.shape):
        ctx.set_grid(volumes.shape, np.zeros(27), np.zeros(9))
    ensure_labels(ctx, volumes)
    ctx.volume_assign(swap)
    fetch_labels(ctx, volumes)


def volume_mask(volumes, density, vol_num):
    """utils.volume_mask (utils.py:461-476): `density` where volumes == vol_num, zero elsewhere (a float64
    device.DeviceArray when `density` is a device array)."""
    ctx = _lib.default_context()
    if ctx.shape != tuple(volumes.shape):
        ctx.set_grid(volumes.shape, np.zeros(27), np.zeros(9))
    ensure_density(ctx, density)
    ensure_labels(ctx, volumes)
    if device.is_device_array(density):
        return ctx.export_volume(vol_num)
    return ctx.volume_mask(vol_num)
