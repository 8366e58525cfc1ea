"""CPU test of ``_native.call``, the one idiom every stream-taking entry point is launched through: device guard, tensors as
device addresses, the stream as the last argument, the return code through ``check``.  A stub stands in for the library."""
import contextlib
import ctypes as C

import pytest
import torch

from street_gaussians_amd import _native


class _Struct(C.Structure):
    _fields_ = [("a", C.c_int), ("b", C.c_float)]


class _StubLib:
    def __init__(self, rc):
        self.rc, self.seen = rc, None

    def sgr_stub(self, *args):
        self.seen = args
        return self.rc

    def sgr_last_error(self):
        return b"stub: it went wrong"


@pytest.fixture
def stub(monkeypatch):
    def install(rc):
        lib, guards, stream = _StubLib(rc), [], C.c_void_p(0x5EED)

        @contextlib.contextmanager
        def guard(device):
            guards.append(device)
            yield

        monkeypatch.setattr(_native, "lib", lambda: lib)
        monkeypatch.setattr(_native, "stream", lambda device: stream)
        monkeypatch.setattr(torch.cuda, "device", guard)
        return lib, guards, stream
    return install


def test_call_marshals_arguments_and_appends_the_stream(stub):
    lib, guards, stream = stub(7)
    a, b, s = torch.zeros(4), torch.zeros(2, 3, dtype=torch.int32), _Struct(3, 0.5)
    ref = C.byref(s)
    assert _native.call("sgr_stub", "dev", a, None, 5, b, 2.5, s, ref) == 7  # a non-negative return code comes back
    assert guards == ["dev"]
    ta, none, five, tb, f, st, rf, last = lib.seen
    assert isinstance(ta, C.c_void_p) and ta.value == a.data_ptr()
    assert isinstance(tb, C.c_void_p) and tb.value == b.data_ptr()
    assert none is None  # NULL, as _native.ptr(None)
    assert five == 5 and type(five) is int and f == 2.5 and type(f) is float
    assert st is s and rf is ref
    assert last is stream


def test_call_raises_the_librarys_error_text(stub):
    lib, guards, _ = stub(-1)
    with pytest.raises(_native.SgrError, match="stub: it went wrong"):
        _native.call("sgr_stub", "dev", torch.zeros(1))
    assert guards == ["dev"] and len(lib.seen) == 2
