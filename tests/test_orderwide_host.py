"""Host side of the wide trimmed mean / median: the exports, ``fa_order_mean_wide``'s
argument validation and the plug-ins' caps. No device is touched: every call returns before any HIP call."""
import pytest

from fedn_amd import _abi

PAIRS = [(_abi.FA_F32, _abi.FA_F32), (_abi.FA_F64, _abi.FA_F64), (_abi.FA_F16, _abi.FA_F16), (_abi.FA_BF16, _abi.FA_F32),
         (_abi.FA_I32, _abi.FA_F64), (_abi.FA_I64, _abi.FA_F64)]
WORK = 1 << 20            # fake addresses: the call must return before it touches any of them


def _call(out=16, od=_abi.FA_F32, ups=True, ud=_abi.FA_F32, K=4, trim=1, P=10, work=WORK, null_at=None):
    ptrs = [4096 + 16 * k for k in range(max(1, min(K, 1100)))]
    if null_at is not None:
        ptrs[null_at] = 0
    return _abi.load().fa_order_mean_wide(out, od, _abi.ptr_array(ptrs) if ups else None, ud, K, trim, P, work, None)


def test_exports_and_work_sizes():
    lib, probe = _abi.load(), _abi.load_probe()
    for name in ("fa_order_mean_wide", "fa_order_mean_wide_work", "fa_order_mean_wide_tile"):
        assert name in _abi.EXPORTS and hasattr(lib, name) and hasattr(probe, name)
    assert lib.fa_abi_version() == _abi.ABI_VERSION >= 16 and probe.fa_abi_version() == _abi.ABI_VERSION
    for K in (0, -1, 1025):
        assert lib.fa_order_mean_wide_work(K) == 0
    for K in (1, 64, 65, 1024):
        assert lib.fa_order_mean_wide_work(K) == probe.fa_order_mean_wide_work(K) == 8 * K
    # a client's segment of a tile is 64 bytes at least, and the tile's keys fit the 160 KiB of LDS
    size = {_abi.FA_F32: 4, _abi.FA_F16: 2, _abi.FA_BF16: 2, _abi.FA_I32: 4, _abi.FA_F64: 8, _abi.FA_I64: 8}
    for ud, _ in PAIRS:
        for K, KP in ((1, 128), (128, 128), (129, 256), (257, 512), (513, 1024), (1024, 1024)):
            C = lib.fa_order_mean_wide_tile(ud, K)
            assert C % 4 == 0 and 64 // size[ud] <= C <= 64 and C * (KP * max(4, size[ud]) + 16) <= 160 << 10, (ud, K, C)
    assert lib.fa_order_mean_wide_tile(_abi.FA_I8, 4) == 0 and lib.fa_order_mean_wide_tile(_abi.FA_F32, 1025) == 0


@pytest.mark.parametrize("kw", [dict(out=None), dict(ups=False), dict(work=None), dict(K=0), dict(K=1025), dict(trim=-1),
                                dict(K=4, trim=2), dict(K=1024, trim=512), dict(P=-1), dict(null_at=2),
                                dict(K=1024, trim=511, null_at=1023)],
                         ids=["null_out", "null_updates", "null_work", "K0", "K1025", "trim_neg", "2trim_eq_K",
                              "2trim_eq_1024", "P_neg", "null_client", "null_last_client"])
def test_argument_errors(kw):
    assert _call(**kw) == _abi.FA_EINVAL
    assert _abi.load().fa_last_error().decode().startswith("fa_order_mean_wide")


def test_dtype_errors_come_after_the_argument_checks():
    assert _call(ud=_abi.FA_I8, od=_abi.FA_F64) == _abi.FA_EDTYPE
    assert _call(ud=_abi.FA_F32, od=_abi.FA_F64) == _abi.FA_EDTYPE
    assert _call(ud=_abi.FA_BF16, od=_abi.FA_BF16) == _abi.FA_EDTYPE
    assert _abi.load().fa_last_error().decode()
    assert _call(ud=_abi.FA_I8, od=_abi.FA_F64, K=1025) == _abi.FA_EINVAL


@pytest.mark.parametrize("ud,od", PAIRS)
def test_empty_is_ok(ud, od):
    for K, trim in ((1, 0), (65, 32), (1024, 511)):
        assert _call(ud=ud, od=od, K=K, trim=trim, P=0) == _abi.FA_OK
        assert _call(ud=ud, od=od, K=K, trim=trim, P=0, null_at=0) == _abi.FA_OK, "an empty buffer may be a null pointer"


def test_caps():
    from fedn_amd import ops
    from fedn_amd.aggregators import (bulyan, centeredclip, geomedian, krum, median, median_wide, multikrum, trimmedmean,
                                      trimmedmean_wide)
    assert ops.MAX_WIDE_ORDER_K == 1024 and ops.MAX_ORDER_K == 64
    for mod in (trimmedmean_wide, median_wide):
        assert mod.Aggregator.max_updates == 1024, mod.__name__
    assert issubclass(trimmedmean_wide.Aggregator, trimmedmean.Aggregator)
    assert issubclass(median_wide.Aggregator, median.Aggregator) and median_wide.Aggregator.parameter_schema == {}
    for mod in (trimmedmean, median, krum, multikrum, geomedian, centeredclip, bulyan):
        assert mod.Aggregator.max_updates == 64, mod.__name__
