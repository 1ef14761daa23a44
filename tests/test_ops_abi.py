"""The ctypes argument structs must match the C structs in csrc/args.h
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


@pytest.mark.parametrize("name", ["DetectArgs", "SmoothArgs", "RankArgs", "WindowArgs", "BivArgs"])
def test_struct_sizes(lib, name):
    assert lib.fm_abi_sizeof(name.encode()) == C.sizeof(getattr(nat, name))


@pytest.mark.parametrize("name,field", [
    ("SmoothArgs", "det"), ("SmoothArgs", "season_out"), ("SmoothArgs", "grid"), ("SmoothArgs", "head_dev"), ("SmoothArgs", "season_hb"), ("SmoothArgs", "nvalid_out"),
    ("DetectArgs", "pw_scale"), ("DetectArgs", "app_stats"), ("DetectArgs", "ld_cur"),
    ("DetectArgs", "anom_count"), ("DetectArgs", "anom_cap"), ("DetectArgs", "thr_lut"), ("DetectArgs", "lut_n"),
    ("DetectArgs", "row_out"), ("DetectArgs", "tick_min"), ("DetectArgs", "shift_one_step"),
    ("RankArgs", "pvals"), ("RankArgs", "alpha"), ("RankArgs", "p_friedman"), ("RankArgs", "pods_b"), ("RankArgs", "z_crit"), ("WindowArgs", "det"),
    ("BivArgs", "eps"), ("BivArgs", "app_stats"),
])
def test_struct_offsets(lib, name, field):
    cls = getattr(nat, name)
    assert lib.fm_abi_offsetof(name.encode(), field.encode()) == getattr(cls, field).offset


def test_module_local_struct_sizes(lib):
    """Structs declared next to their kernels (lstm / lstm_train / decompose)."""
    from foremast_amd.ops import kernels, lstm, lstm_train, pack
    for sym, cls in (("fm_lstm_args_size", lstm.LstmArgs), ("fm_lstm_train_args_size", lstm_train.LstmTrainArgs),
                     ("fm_decompose_args_size", kernels.DecompArgs), ("fm_lstm_level_args_size", lstm.LevelArgs),
                     ("fm_hw_state_args_size", kernels.HwStateArgs),
                     ("fm_hw_update_args_size", kernels.HwUpdateArgs), ("fm_pack_args_size", pack.PackArgs)):
        f = getattr(lib, sym)
        f.restype = C.c_longlong
        assert f() == C.sizeof(cls), sym


def test_hw_seq_geometry(lib):
    """Variant 6 (hw_seq.hip) host helpers: threads per series (two grid points per thread up
    to m = 96, one at m = 144; 16..64 threads), the LDS of one workgroup (two fp32 images of
    the padded week plus a count per series) and the seasons it is instantiated for."""
    nat.load()  # argtypes / restype
    assert lib.fm_hw_seq_tpc(72, 64) == 32 and lib.fm_hw_seq_tpc(72, 16) == 16 and lib.fm_hw_seq_tpc(72, 33) == 32
    assert lib.fm_hw_seq_tpc(144, 64) == 64 and lib.fm_hw_seq_tpc(144, 5) == 32
    assert lib.fm_hw_seq_tpc(72, 65) == 0 and lib.fm_hw_seq_tpc(1440, 64) == 0 and lib.fm_hw_seq_tpc(70, 8) == 0
    assert lib.fm_hw_seq_lds_bytes(504, 72, 64) == (2 * 8 * (504 + 4) + 8) * 4
    assert lib.fm_hw_seq_lds_bytes(504, 72, 16) == (2 * 16 * (504 + 4) + 16) * 4
    none = C.c_size_t(-1).value
    assert lib.fm_hw_seq_lds_bytes(500, 72, 64) == none       # not a whole number of seasons
    assert lib.fm_hw_seq_lds_bytes(72, 72, 64) == none        # one season: nothing to fit
    assert lib.fm_hw_seq_lds_bytes(2016, 288, 64) == (2 * 4 * (2016 + 4) + 4) * 4  # one grid point per thread


def test_hw_variant5_lds_bytes(lib):
    """Variant 5 (hw_scan.hip hw_d / hw_dg / hw_q kernels): the LDS of one workgroup, from the
    layout the kernels carve.  Per series and fitted season one fp32 image of 260 floats per
    8-step chunk; then the fixed blocks (validity mask, per-wave sums, flag, last season's
    head, per-wave bests, bounds); the gapped kernel adds its miss masks, per-season gap flags
    and the two valid counts.  2..7 seasons, K = 45 / 9 (32 lanes) and K = 18 (16 lanes)."""
    nat.load()
    none = C.c_size_t(-1).value

    def season(K):
        return 260 * ((K + 7) // 8)

    for K in (45, 9):
        seg = 32 * K
        for nseg in range(2, 8):
            ns1 = nseg - 1
            d = (2 * ns1 * season(K) + 2 * K + 232) * 4
            assert lib.fm_hw_d_lds_bytes(nseg * seg, seg, K) == d, (K, nseg)
            assert lib.fm_hw_dg_lds_bytes(nseg * seg, seg, K) == d + (2 * ns1 * 64 + 2 * ns1 + 2) * 4, (K, nseg)
        for f in (lib.fm_hw_d_lds_bytes, lib.fm_hw_dg_lds_bytes):
            assert f(seg, seg, K) == none and f(8 * seg, seg, K) == none       # 1 or 8 seasons
    K, seg = 18, 288
    for nseg in range(2, 8):
        assert lib.fm_hw_q_lds_bytes(nseg * seg, seg, K) == (4 * (nseg - 1) * season(K) + 4 * 9 + 460) * 4, nseg
    assert lib.fm_hw_q_lds_bytes(seg, seg, K) == none and lib.fm_hw_q_lds_bytes(8 * seg, seg, K) == none
    assert lib.fm_hw_d_lds_bytes(7 * 1440, 1440, 45) == 76168
    assert lib.fm_hw_dg_lds_bytes(7 * 1440, 1440, 45) == 79296
    assert lib.fm_hw_q_lds_bytes(7 * 288, 288, 18) == 76864
    # unsupported K, and the quad layout off its season (seg != 16 K)
    for f in (lib.fm_hw_d_lds_bytes, lib.fm_hw_dg_lds_bytes):
        assert f(7 * 768, 768, 24) == none and f(7 * 576, 576, 18) == none
    assert lib.fm_hw_q_lds_bytes(7 * 288, 288, 9) == none and lib.fm_hw_q_lds_bytes(7 * 1440, 1440, 45) == none
    assert lib.fm_hw_q_lds_bytes(7 * 576, 576, 18) == none
