"""pybader_amd.device without a GPU: how __cuda_array_interface__ is read (versions, strides, dtypes, the read-only flag,
the stream entry), what is and is not a device array, and that the module leaves torch alone."""
import subprocess
import sys

import numpy as np
import pytest

from pybader_amd import _lib, device, utils


class Fake:
    """an object that publishes a hand-made interface dictionary (no memory behind it: describe() only reads)"""

    def __init__(self, shape=(4, 5, 6), typestr='<f8', ptr=0x7f0000001000, readonly=False, version=2, **extra):
        self.__cuda_array_interface__ = {'shape': shape, 'typestr': typestr, 'data': (ptr, readonly), 'version': version, **extra}


def refused(*args, **kwargs):
    with pytest.raises(_lib.BaderHipError) as e:
        device.describe(*args, **kwargs)
    assert e.value.code == _lib.XB_E_ARG
    return str(e.value)


@pytest.mark.parametrize('version', [2, 3])
def test_versions_2_and_3_without_strides_are_c_contiguous(version):
    for extra in ({}, {'strides': None}):
        d = device.describe(Fake(version=version, **extra))
        assert (d.ptr, d.shape, d.strides) == (0x7f0000001000, (4, 5, 6), (30, 6, 1))
        assert d.dtype == np.float64 and d.readonly is False and d.stream is None and d.c_contiguous


def test_other_versions_are_refused():
    for version in (0, 1, 4, None):
        assert 'version' in refused(Fake(version=version))


def test_byte_strides_become_element_strides():
    d = device.describe(Fake(typestr='<f4', strides=(4, 16, 80)))        # a permuted (6, 5, 4) float32 array
    assert d.strides == (1, 4, 20) and d.dtype == np.float32 and not d.c_contiguous
    d = device.describe(Fake(shape=(4, 5, 3), strides=(240, 48, 16)))    # every second z of a (4, 5, 6) float64 array
    assert d.strides == (30, 6, 2) and not d.c_contiguous
    assert device.describe(Fake(strides=(240, 48, 8))).c_contiguous
    assert device.describe(Fake(shape=(1, 5, 6), strides=(8000, 48, 8))).c_contiguous     # (a length-1 axis may have any stride)


def test_strides_that_are_no_multiple_of_the_item_size_are_refused():
    assert 'item size' in refused(Fake(strides=(240, 48, 4)))
    assert 'item size' in refused(Fake(typestr='<i2', strides=(60, 12, 1)))
    assert 'strides' in refused(Fake(strides=(48, 8)))


def test_zero_and_negative_strides():
    d = device.describe(Fake(strides=(0, 48, 8)))                         # an expanded (broadcast) axis
    assert d.strides == (0, 6, 1) and not d.c_contiguous
    d = device.describe(Fake(strides=(240, -48, 8)))                      # a flipped axis
    assert d.strides == (30, -6, 1) and not d.c_contiguous


@pytest.mark.parametrize('typestr, dtype', [('<f4', np.float32), ('<f8', np.float64), ('|i1', np.int8), ('<i2', np.int16),
                                            ('<i4', np.int32), ('<i8', np.int64)])
def test_supported_dtypes(typestr, dtype):
    assert device.describe(Fake(typestr=typestr)).dtype == np.dtype(dtype)


@pytest.mark.parametrize('typestr', ['<f2', '|u1', '<u4', '<c8', '|b1', '>f8', '<V2', 'bfloat16'])
def test_unsupported_typestr_is_refused(typestr):
    refused(Fake(typestr=typestr))


def test_read_only_is_fine_as_input_and_refused_as_output():
    ro = Fake(readonly=True)
    assert device.describe(ro).readonly is True
    assert 'read-only' in refused(ro, writable=True)
    assert device.describe(Fake(), writable=True).readonly is False


def test_stream_entry():
    assert device.describe(Fake(version=3)).stream is None
    assert device.describe(Fake(version=3, stream=None)).stream is None
    assert device.describe(Fake(version=3, stream=1)).stream == 0              # legacy default stream = HIP's null stream
    assert device.describe(Fake(version=3, stream=2)).stream == 2              # per-thread default stream = hipStreamPerThread
    assert device.describe(Fake(version=3, stream=0x55aa00)).stream == 0x55aa00
    assert 'disallowed' in refused(Fake(version=3, stream=0))
    assert device.describe(Fake(version=2, stream=0x55aa00)).stream is None    # version 2 has no such entry


def test_the_stream_of_a_call():
    d2, d3 = device.describe(Fake()), device.describe(Fake(version=3, stream=0x1230))
    assert device.current_stream() == 0 and device.stream_for(d2).value in (None, 0)
    with device.on_stream(0x4560):
        assert device.current_stream() == 0x4560
        assert device.stream_for(d2).value == 0x4560
        assert device.stream_for(d3).value == 0x1230           # the array's own entry wins
        with device.on_stream(None):
            assert device.current_stream() == 0
        assert device.current_stream() == 0x4560
    assert device.current_stream() == 0


def test_mask_and_null_pointer_are_refused():
    refused(Fake(mask=Fake()))
    refused(Fake(ptr=0))
    assert device.describe(Fake(shape=(0, 5, 6), ptr=0)).shape == (0, 5, 6)


def test_what_is_a_device_array():
    assert device.is_device_array(Fake())
    assert not device.is_device_array(np.zeros((3, 3, 3)))
    assert not device.is_device_array([1, 2, 3]) and not device.is_device_array(None)
    refused(object())
    d = device.describe(Fake())
    assert d.identity == device.describe(Fake()).identity != device.describe(Fake(typestr='<f4')).identity


def test_a_host_ndarray_still_takes_the_host_path():
    """utils.ensure_density with an ndarray uploads (never imports); with a device array it imports (never uploads)"""
    calls = []

    class Ctx:
        pinned_density = resident_density = None

        def upload_density(self, a):
            calls.append(('upload', a.dtype, a.flags.c_contiguous))

        def import_density(self, a):
            calls.append(('import', a))

    host = np.arange(27, dtype=np.float32).reshape(3, 3, 3).transpose(2, 1, 0)
    got = utils.ensure_density(Ctx(), host)
    assert calls == [('upload', np.float64, True)] and isinstance(got, np.ndarray)
    fake = Fake(shape=(3, 3, 3))
    assert utils.ensure_density(Ctx(), fake) is fake and calls[1] == ('import', fake)
    ctx = Ctx()
    ctx.pinned_density = device.describe(fake).identity           # inside resident(): imported once
    utils.ensure_density(ctx, fake)
    utils.ensure_density(ctx, fake)
    assert [c[0] for c in calls] == ['upload', 'import', 'import']


def test_label_helpers_recognise_device_arrays():
    assert utils.label_dtype(Fake(typestr='<i2')) == np.int16 and utils.label_dtype(np.zeros(3, np.int8)) == np.int8
    assert utils.dev_reusable(Fake(typestr='<i2'), np.dtype(np.int16))
    assert not utils.dev_reusable(Fake(typestr='<i2'), np.dtype(np.int8))
    assert not utils.dev_reusable(Fake(typestr='<i2', readonly=True), np.dtype(np.int16))
    assert not utils.dev_reusable(Fake(typestr='<i2', strides=(120, 24, 4)), np.dtype(np.int16))


def test_the_package_never_imports_torch():
    code = ("import sys; import pybader_amd.device, pybader_amd.interface, pybader_amd.thread_handlers, pybader_amd.utils; "
            "assert 'torch' not in sys.modules and 'cupy' not in sys.modules")
    subprocess.run([sys.executable, '-c', code], check=True, cwd=str(__import__('pathlib').Path(__file__).resolve().parents[1]))
