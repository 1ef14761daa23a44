"""The ctypes mirror of MvnGroupArgs (csrc/args.h) must match the C struct
(runs on CPU: loading the library does not need a device)."""

import ctypes as C

import pytest

from foremast_amd.ops import _native as nat
from foremast_amd.ops import build


@pytest.fixture(scope="module")
def lib():
    try:
        build.build()
    except RuntimeError as e:  # pragma: no cover
        pytest.skip(f"no HIP toolchain: {e}")
    lib = nat.load()
    if lib is None:
        pytest.skip("library failed to load")
    lib.fm_abi_sizeof.restype = C.c_longlong
    lib.fm_abi_offsetof.restype = C.c_longlong
    return lib


def test_group_struct_size(lib):
    assert lib.fm_abi_sizeof(b"MvnGroupArgs") == C.sizeof(nat.MvnGroupArgs)


@pytest.mark.parametrize("field", ["thr2", "contrib", "anom_val", "kmask"])
def test_group_struct_offsets(lib, field):
    assert lib.fm_abi_offsetof(b"MvnGroupArgs", field.encode()) == getattr(nat.MvnGroupArgs, field).offset
