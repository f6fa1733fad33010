"""Arrays that already live on the GPU: a density built by PyTorch, CuPy or any other producer that publishes
`__cuda_array_interface__` goes into the library, and label maps and masked volumes come back, without a trip through
host memory.  No counterpart in the reference (its arrays share one address space).  This module never imports torch
or cupy: it reads the interface dictionary and nothing else.

    describe(obj)      pointer, shape, element strides, dtype, read-only flag and stream of a device array
    DeviceArray        a result array the library owns; publishes the interface itself (torch.as_tensor(r, device='cuda')
                       wraps it without a copy and keeps it alive), has shape / dtype / to_host()
    on_stream(handle)  names the caller's stream for the calls inside the block

ORDER.  Every call that reads or writes a device array is queued behind the work already on the caller's stream, and the
caller's stream goes on behind it: no host wait, no torch.cuda.synchronize() before or after.  The caller's stream is
the one `on_stream` names (default: the legacy default stream, which is where torch-ROCm and CuPy work unless told
otherwise); an array whose interface carries a version-3 `stream` entry is ordered against that stream instead.

RESIDENCY.  The library cannot see a write to memory it does not own, so by default every call copies the density again
(device to device).  Inside `utils.resident(density)` it is copied once: the caller promises not to write the array --
nor a label map the library handed out inside the block -- until the block ends."""
import contextlib
import ctypes as C
import threading
import weakref

import numpy as np

from . import _lib
from ._lib import BaderHipError, XB_E_ARG

FLOAT_CODE = {np.dtype(np.float32): 32, np.dtype(np.float64): 64}        # XB_F32 / XB_F64
_SUPPORTED = tuple(FLOAT_CODE) + tuple(_lib.DTYPE_CODE)


def _refuse(msg):
    err = BaderHipError(msg)
    err.code = XB_E_ARG
    return err


def is_device_array(obj):
    """does `obj` publish __cuda_array_interface__ (a host ndarray does not)"""
    return not isinstance(obj, np.ndarray) and hasattr(obj, '__cuda_array_interface__')


class Description:
    """what describe() found: ptr (int), shape (tuple), strides (tuple, in ELEMENTS), dtype (numpy), readonly,
    stream (None: nothing said; else a hipStream_t handle as int, 0 being the legacy default stream)"""
    __slots__ = ('ptr', 'shape', 'strides', 'dtype', 'readonly', 'stream')

    def __init__(self, ptr, shape, strides, dtype, readonly, stream):
        self.ptr, self.shape, self.strides, self.dtype, self.readonly, self.stream = ptr, shape, strides, dtype, readonly, stream

    @property
    def c_contiguous(self):
        want = 1
        for n, s in zip(reversed(self.shape), reversed(self.strides)):
            if n != 1 and s != want:
                return False
            want *= n
        return True

    @property
    def identity(self):
        """how utils.resident() recognises the array again: pointer, shape, strides, dtype"""
        return ('device', self.ptr, self.shape, self.strides, self.dtype.str)


def describe(obj, writable=False):
    """Read obj.__cuda_array_interface__ (versions 2 and 3).  Raises BaderHipError (code XB_E_ARG) for anything the
    library does not take: an unknown version, a dtype other than float32 / float64 / int8 / int16 / int32 / int64,
    byte strides that are no multiple of the item size, a mask, a null pointer with elements behind it -- and, with
    `writable`, a read-only buffer."""
    try:
        cai = obj.__cuda_array_interface__
    except AttributeError:
        raise _refuse(f'{type(obj).__name__} has no __cuda_array_interface__: not a device array') from None
    version = cai.get('version')
    if version not in (2, 3):
        raise _refuse(f'__cuda_array_interface__ version {version!r}: versions 2 and 3 are understood')
    if cai.get('mask') is not None:
        raise _refuse('masked device arrays are not supported')
    try:
        dtype = np.dtype(cai['typestr'])
    except TypeError:
        raise _refuse(f"unsupported typestr {cai.get('typestr')!r}") from None
    if dtype not in _SUPPORTED or dtype.byteorder == '>':
        raise _refuse(f'unsupported dtype {dtype.str} (float32, float64, int8, int16, int32 and int64 are taken)')
    shape = tuple(int(n) for n in cai['shape'])
    if any(n < 0 for n in shape):
        raise _refuse(f'bad shape {shape}')
    ptr, readonly = cai['data']
    ptr = int(ptr or 0)
    if ptr == 0 and int(np.prod(shape, dtype=np.int64)) != 0:
        raise _refuse('null data pointer')
    strides = cai.get('strides')
    if strides is None:                                  # C-contiguous
        strides, run = [], 1
        for n in reversed(shape):
            strides.append(run)
            run *= n
        strides = tuple(reversed(strides))
    else:
        if len(strides) != len(shape):
            raise _refuse(f'{len(strides)} strides for {len(shape)} axes')
        if any(int(s) % dtype.itemsize for s in strides):
            raise _refuse(f'byte strides {tuple(strides)} are no multiples of the item size {dtype.itemsize}')
        strides = tuple(int(s) // dtype.itemsize for s in strides)
    stream = cai.get('stream') if version >= 3 else None
    if stream is not None:
        stream = int(stream)
        if stream == 0:
            raise _refuse("__cuda_array_interface__: 'stream' 0 is disallowed (1: legacy default, 2: per-thread default)")
        if stream == 1:
            stream = 0                                   # the legacy default stream is HIP's null stream
        # (2, the per-thread default stream, is HIP's own handle value for it: hipStreamPerThread)
    if writable and readonly:
        raise _refuse('the device array is read-only: it cannot take a result')
    return Description(ptr, shape, strides, dtype, bool(readonly), stream)


# ---- the caller's stream ---------------------------------------------------------------------------------------------
_tls = threading.local()


def current_stream():
    return getattr(_tls, 'stream', 0)


@contextlib.contextmanager
def on_stream(handle):
    """with on_stream(torch.cuda.current_stream().cuda_stream): ... -- the calls inside are ordered against this
    hipStream_t (an int; None or 0: the legacy default stream)."""
    before = current_stream()
    _tls.stream = int(handle or 0)
    try:
        yield
    finally:
        _tls.stream = before


def stream_for(desc):
    """the stream a call on `desc` is ordered against: the array's own version-3 entry, else on_stream's"""
    return C.c_void_p(desc.stream if desc.stream is not None else current_stream())


# ---- result arrays ---------------------------------------------------------------------------------------------------
def _free(ptr):
    lib = _lib._lib
    if lib is not None:
        lib.xb_device_free(C.c_void_p(ptr))


class DeviceArray:
    """A C-contiguous array in device memory that the library allocated; freed when the last reference is gone (a
    torch tensor made from it with torch.as_tensor holds one)."""

    def __init__(self, ctx, shape, dtype):
        self.ctx = ctx
        self.shape = tuple(int(n) for n in shape)
        self.dtype = np.dtype(dtype)
        self.nbytes = int(np.prod(self.shape, dtype=np.int64)) * self.dtype.itemsize
        p = C.c_void_p()
        _lib.check(ctx.lib.xb_device_alloc(int(ctx.device), max(self.nbytes, 1), C.byref(p)))
        self.ptr = int(p.value)
        self._finalizer = weakref.finalize(self, _free, self.ptr)

    ndim = property(lambda self: len(self.shape))
    size = property(lambda self: int(np.prod(self.shape, dtype=np.int64)))

    @property
    def __cuda_array_interface__(self):
        return {'shape': self.shape, 'typestr': self.dtype.str, 'data': (self.ptr, False), 'version': 2, 'strides': None}

    def to_host(self):
        """a host ndarray with the array's content (ordered behind the caller's stream; waits for the copy)"""
        out = np.empty(self.shape, self.dtype)
        if self.nbytes:
            _lib.check(self.ctx.lib.xb_device_read(self.ctx.h, out.ctypes.data_as(C.c_void_p), C.c_void_p(self.ptr),
                                                   self.nbytes, C.c_void_p(current_stream())))
        return out

    def __repr__(self):
        return f'DeviceArray(shape={self.shape}, dtype={self.dtype.name}, ptr=0x{self.ptr:x})'


def to_host(obj, ctx=None):
    """host copy of any device array (a DeviceArray, or a foreign one through the context's stream)"""
    if isinstance(obj, DeviceArray):
        return obj.to_host()
    d = describe(obj)
    if not d.c_contiguous:
        raise _refuse('to_host: a C-contiguous device array is required')
    ctx = ctx or _lib.default_context()
    out = np.empty(d.shape, d.dtype)
    if out.nbytes:
        _lib.check(ctx.lib.xb_device_read(ctx.h, out.ctypes.data_as(C.c_void_p), C.c_void_p(d.ptr), out.nbytes, stream_for(d)))
    return out
