"""hip_lib.launch, the one marshaller of the Python wrappers, against a recording stand-in for the library (no library, no GPU), and the
shape of the package's source: nothing but hip_lib spells a launch by hand."""
import ctypes
import os
import re

import pytest
import torch

from visualrwkv_amd import hip_lib

STREAM = 0x5EED


class _Lib:
    """Stands in for the ctypes library: every entry records (name, args) and returns `code`; vrwkv_strerror answers as the library does."""

    def __init__(self, code=0):
        self.code, self.calls = code, []

    def vrwkv_strerror(self, code):
        return f"stand-in error {code}".encode()

    def __getattr__(self, name):
        def entry(*args):
            self.calls.append((name, args))
            return self.code
        return entry


@pytest.fixture
def lib(monkeypatch):
    lib = _Lib()
    monkeypatch.setattr(hip_lib, "load", lambda: lib)
    monkeypatch.setattr(hip_lib, "launch_stream", lambda device: STREAM)
    return lib


def _one(lib):
    (call,) = lib.calls
    return call


class _Sub(torch.Tensor):
    pass


def test_name_order_and_stream_last(lib):
    a, b = torch.zeros(3), torch.ones(2)
    hip_lib.launch("vrwkv_x", 7, a, 2.5, b, device="cpu")
    assert _one(lib) == ("vrwkv_x", (7, a.data_ptr(), 2.5, b.data_ptr(), STREAM))


def test_tensor_kinds_arrive_as_pointers(lib):
    t = torch.zeros(4)
    p = torch.nn.Parameter(torch.zeros(5))
    s = torch.zeros(6).as_subclass(_Sub)
    assert type(s) is _Sub
    hip_lib.launch("vrwkv_x", t, p, s, device="cpu")
    args = _one(lib)[1]
    assert args == (t.data_ptr(), p.data_ptr(), s.data_ptr(), STREAM)
    assert all(type(a) is int for a in args)


def test_none_is_null(lib):
    hip_lib.launch("vrwkv_x", None, device="cpu")
    args = _one(lib)[1]
    assert args == (0, STREAM) and type(args[0]) is int


def test_numbers_unchanged(lib):
    hip_lib.launch("vrwkv_x", 3, 1.5, True, False, device="cpu")
    args = _one(lib)[1]
    assert args == (3, 1.5, True, False, STREAM)
    assert [type(a) for a in args[:4]] == [int, float, bool, bool]


@pytest.mark.parametrize("seq", [list, tuple])
def test_tensor_sequence_is_pointer_array(lib, seq):
    a, b = torch.zeros(2), torch.nn.Parameter(torch.zeros(3))
    hip_lib.launch("vrwkv_x", seq((a, None, b)), device="cpu")
    (arr, st) = _one(lib)[1]
    assert isinstance(arr, ctypes.Array) and arr._type_ is ctypes.c_void_p and len(arr) == 3
    assert list(arr) == [a.data_ptr(), None, b.data_ptr()]          # ctypes reads a NULL c_void_p back as None
    assert ctypes.cast(arr, ctypes.POINTER(ctypes.c_size_t))[1] == 0
    assert st == STREAM


def test_int_list_is_int_array(lib):
    hip_lib.launch("vrwkv_x", [5, 0, -7, 64], device="cpu")
    arr = _one(lib)[1][0]
    assert isinstance(arr, ctypes.Array) and arr._type_ is ctypes.c_int and list(arr) == [5, 0, -7, 64]


def test_empty_list_is_empty_array(lib):
    hip_lib.launch("vrwkv_x", [], device="cpu")
    arr = _one(lib)[1][0]
    assert isinstance(arr, ctypes.Array) and len(arr) == 0


def test_ctypes_array_passes_through(lib):
    m3 = (ctypes.c_float * 3)(0.5, 0.25, 0.125)
    hip_lib.launch("vrwkv_x", 1, m3, device="cpu")
    assert _one(lib)[1][1] is m3


def test_nonzero_code_raises(lib):
    lib.code = -3
    with pytest.raises(RuntimeError, match=r"vrwkv_x failed: stand-in error -3 \(code -3\)"):
        hip_lib.launch("vrwkv_x", 1, device="cpu")
    assert len(lib.calls) == 1


def test_allowed_code_is_returned(lib):
    assert hip_lib.launch("vrwkv_x", 1, device="cpu") == 0
    lib.code = hip_lib.ESHAPE
    assert hip_lib.launch("vrwkv_x", 1, device="cpu", allow=(hip_lib.ESHAPE,)) == hip_lib.ESHAPE
    with pytest.raises(RuntimeError, match="vrwkv_x"):
        hip_lib.launch("vrwkv_x", 1, device="cpu", allow=(-5,))


# ---------------------------------------------------------------------------------------------------------------
# The source: launches go through hip_lib.launch; what still calls the library directly and checks its code is listed here by entry
# ---------------------------------------------------------------------------------------------------------------
PKG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "visualrwkv_amd")
# module -> the entries whose code it may hand to hip_lib.check itself: setters, nothing else (sizes are compared, host entries have a check
# of their own)
DIRECT_CHECKS = {
    "wkv7.py": {"vrwkv_wkv7_set_backward_variant", "vrwkv_wkv7_set_forward_variant"},
    "wkv6.py": {"vrwkv_wkv6_set_backward_variant"},
}


def _sources():
    for name in sorted(os.listdir(PKG)):
        if name.endswith(".py") and name != "hip_lib.py":
            with open(os.path.join(PKG, name)) as f:
                yield name, f.read()


def test_no_stream_handles_outside_hip_lib():
    for name, text in _sources():
        for needle in ("launch_stream(", ".cuda_stream"):
            assert needle not in text, f"{name} spells {needle!r}: launches take their stream inside hip_lib.launch"


def test_direct_checks_are_the_listed_non_launches():
    seen = {}
    for name, text in _sources():
        lines = text.splitlines()
        for i, line in enumerate(lines):
            if "hip_lib.check(" not in line:
                continue
            near = " ".join(lines[max(0, i - 3):i + 1])
            entries = set(re.findall(r"vrwkv_\w+", near))
            allowed = DIRECT_CHECKS.get(name, set())
            assert entries and entries <= allowed, f"{name}:{i + 1}: hip_lib.check beside {sorted(entries) or 'no entry name'}: a launch goes through hip_lib.launch"
            seen.setdefault(name, set()).update(entries)
    assert seen == DIRECT_CHECKS            # a listed line that has gone leaves the list too
