"""Host side of the wide mean around median: the export, ``fa_median_window_mean_wide``'s
argument validation and the ``meamed`` plug-in's cap, schema and window length. No device is touched: every call
returns before any HIP call."""
import math

import pytest

from fedn_amd import _abi
from test_orderwide_host import PAIRS, WORK

EINVAL, EDTYPE = _abi.FA_EINVAL, _abi.FA_EDTYPE


def _call(out=16, od=_abi.FA_F32, ups=True, ud=_abi.FA_F32, K=4, keep=2, P=10, work=WORK, null_at=None):
    ptrs = [4096 + 16 * k for k in range(max(1, min(K, 1100)))]
    if null_at is not None:
        ptrs[null_at] = 0
    return _abi.load().fa_median_window_mean_wide(out, od, _abi.ptr_array(ptrs) if ups else None, ud, K, keep, P, work,
                                                  None)


def test_export():
    lib, probe = _abi.load(), _abi.load_probe()
    assert "fa_median_window_mean_wide" in _abi.EXPORTS
    assert hasattr(lib, "fa_median_window_mean_wide") and hasattr(probe, "fa_median_window_mean_wide")
    assert lib.fa_abi_version() == _abi.ABI_VERSION >= 17 and probe.fa_abi_version() == _abi.ABI_VERSION


@pytest.mark.parametrize("want,kw", [
    (EINVAL, dict(out=None)), (EINVAL, dict(ups=False)), (EINVAL, dict(work=None)), (EINVAL, dict(K=0)),
    (EINVAL, dict(K=1025)), (EINVAL, dict(keep=0)), (EINVAL, dict(keep=-1)), (EINVAL, dict(K=4, keep=5)),
    (EINVAL, dict(K=1024, keep=1025)), (EINVAL, dict(P=-1)), (EINVAL, dict(null_at=2)),
    (EINVAL, dict(K=1024, keep=1024, null_at=1023)),
    # the dtype pair is looked at after K, keep and P
    (EDTYPE, dict(ud=_abi.FA_I8, od=_abi.FA_F64)), (EDTYPE, dict(od=_abi.FA_F64)), (EDTYPE, dict(ud=_abi.FA_BF16, od=_abi.FA_BF16)),
    (EINVAL, dict(od=_abi.FA_F64, K=1025)), (EINVAL, dict(od=_abi.FA_F64, keep=5)), (EINVAL, dict(od=_abi.FA_F64, P=-1))])
def test_argument_errors(want, kw):
    assert _call(**kw) == want
    assert _abi.load().fa_last_error().decode().startswith("fa_median_window_mean_wide")


@pytest.mark.parametrize("ud,od", PAIRS)
def test_empty_is_ok(ud, od):
    for K in (1, 65, 1024):
        assert _call(ud=ud, od=od, K=K, keep=K // 2 + 1, P=0) == _abi.FA_OK
        assert _call(ud=ud, od=od, K=K, keep=K, P=0, null_at=0) == _abi.FA_OK, "an empty buffer may be a null pointer"


def test_plugin_cap_schema_and_keep():
    from fedn_amd import ops
    from fedn_amd.aggregators import meamed, trimmedmean
    A = meamed.Aggregator
    assert issubclass(A, trimmedmean.Aggregator) and A.max_updates == ops.MAX_WIDE_ORDER_K == 1024
    assert A.parameter_schema == {"byzantine_fraction": float} and A.default_parameters == {"byzantine_fraction": 0.2}
    assert A.fraction_parameter == "byzantine_fraction" and A.fraction_bound == 0.5
    agg, Ks = A(None), (1, 2, 3, 64, 65, 1024)
    for fraction, keeps in ((0.0, list(Ks)), (0.2, [1, 2, 3, 52, 52, 820]), (0.49, [1, 2, 2, 33, 34, 523])):
        assert [agg.keep(K, {"byzantine_fraction": fraction}) for K in Ks] == keeps
        assert keeps == [K - min(math.floor(fraction * K), (K - 1) // 2) for K in Ks]
