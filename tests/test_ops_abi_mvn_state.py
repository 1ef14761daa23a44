"""The ctypes mirrors of MvnFitStateArgs / MvnStateDetectArgs (csrc/args.h) must match the C
structs (runs on CPU: loading the library does not need a device)."""

import ctypes as C

import pytest

from foremast_amd.ops import _native as nat
from foremast_amd.ops import build

FIELDS = {"MvnFitStateArgs": ["groups", "dst", "eps", "chol", "kmask"],
          "MvnStateDetectArgs": ["active", "ld_cur", "min_valid", "contrib", "anom_cap", "kmask"]}


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


@pytest.mark.parametrize("name", sorted(FIELDS))
def test_state_struct_sizes(lib, name):
    assert lib.fm_abi_sizeof(name.encode()) == C.sizeof(getattr(nat, name))


@pytest.mark.parametrize("name,field", [(n, f) for n in sorted(FIELDS) for f in FIELDS[n]])
def test_state_struct_offsets(lib, name, field):
    assert lib.fm_abi_offsetof(name.encode(), field.encode()) == getattr(getattr(nat, name), field).offset


def test_state_entry_points_are_declared(lib):
    assert lib.fm_mvn_fit_state.argtypes[0]._type_ is nat.MvnFitStateArgs
    assert lib.fm_mvn_state_detect.argtypes[0]._type_ is nat.MvnStateDetectArgs
