"""The ctypes mirror of RobustArgs (csrc/args.h) must match the C struct
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


def test_robust_struct_size(lib):
    assert lib.fm_abi_sizeof(b"RobustArgs") == C.sizeof(nat.RobustArgs)


@pytest.mark.parametrize("field", ["det", "mad", "sigma"])
def test_robust_struct_offsets(lib, field):
    assert lib.fm_abi_offsetof(b"RobustArgs", field.encode()) == getattr(nat.RobustArgs, field).offset


def test_robust_symbol_is_bound(lib):
    assert lib.fm_robust_stats.argtypes[0]._type_ is nat.RobustArgs
