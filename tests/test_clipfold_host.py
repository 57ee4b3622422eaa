"""Host side of the chunked clipping fold: the C ABI's argument validation of
``fa_clip_fold``, the plug-ins' admission caps, and the chunk-carried restatement of the fold against the
one-shot oracle tests/cclip_ref.py. No device is touched: every library call here returns before any HIP
call."""
import numpy as np
import pytest

import cclip_ref as cr
import krum_ref as kr
import robust_ref as rr
from fedn_amd import _abi
from robust_fuzz_cases import center_round_updates

SIX = [_abi.FA_F32, _abi.FA_F64, _abi.FA_F16, _abi.FA_BF16, _abi.FA_I32, _abi.FA_I64]
OUT_OF = {_abi.FA_F32: _abi.FA_F32, _abi.FA_F64: _abi.FA_F64, _abi.FA_F16: _abi.FA_F16, _abi.FA_BF16: _abi.FA_F32,
          _abi.FA_I32: _abi.FA_F64, _abi.FA_I64: _abi.FA_F64}
SIZE = {_abi.FA_F32: 4, _abi.FA_F64: 8, _abi.FA_F16: 2, _abi.FA_BF16: 2, _abi.FA_I32: 4, _abi.FA_I64: 8}
C_SIZE = {_abi.FA_F32: 4, _abi.FA_F16: 4, _abi.FA_BF16: 4, _abi.FA_F64: 8, _abi.FA_I32: 8, _abi.FA_I64: 8}

# fake addresses, far apart: the call must return before it touches any of them
OUT, CARRY_OUT, CARRY_IN, CENTER, UPDATES = 1 << 20, 2 << 20, 3 << 20, 4 << 20, 8 << 20
UPD_STRIDE = 1 << 16


def _call(out=OUT, od=None, carry_out=None, carry_in=None, center=CENTER, ups=True, ud=_abi.FA_F32, coef="uniform", K=4,
          P=10, null_at=None, upd_at=None):
    n = max(1, min(K, 80))
    ptrs = [UPDATES + UPD_STRIDE * k for k in range(n)]
    if null_at is not None:
        ptrs[null_at] = 0
    if upd_at is not None:
        ptrs[upd_at[0]] = upd_at[1]
    if isinstance(coef, str):
        coef = [1.0 / n] * n
    od = OUT_OF.get(ud, _abi.FA_F32) if od is None else od
    return _abi.load().fa_clip_fold(out, od, carry_out, carry_in, center, _abi.ptr_array(ptrs) if ups else None, ud,
                                    _abi.double_array(coef) if coef is not None else None, K, P, None)


def _err():
    return _abi.load().fa_last_error().decode()


def test_library_exports_fa_clip_fold():
    lib, probe = _abi.load(), _abi.load_probe()
    assert "fa_clip_fold" in _abi.EXPORTS and hasattr(lib, "fa_clip_fold") and hasattr(probe, "fa_clip_fold")
    assert lib.fa_abi_version() == _abi.ABI_VERSION >= 15
    assert probe.fa_abi_version() == _abi.ABI_VERSION


@pytest.mark.parametrize("kw", [dict(out=None), dict(center=None), dict(coef=None), dict(ups=False), dict(null_at=2),
                                dict(K=0), dict(K=65), dict(K=-1), dict(P=-1),
                                dict(coef=[0.5, -0.25, 0.5, 0.25]), dict(coef=[0.5, float("nan"), 0.5, 0.25]),
                                dict(coef=[0.5, float("inf"), 0.5, 0.25]), dict(coef=[1e39, 0.0, 0.0, 0.0])],
                         ids=["no_output", "null_center", "null_coef", "null_updates", "null_client", "K0", "K65", "K_neg",
                              "P_neg", "coef_negative", "coef_nan", "coef_inf", "coef_inf_in_f32"])
def test_argument_errors(kw):
    assert _call(**kw) == _abi.FA_EINVAL
    assert _err()


def test_one_output_is_enough():
    """out alone, carry_out alone, both: each passes every check up to the client pointers (a null one is
    what refuses these calls); neither is refused first."""
    for kw in (dict(), dict(out=None, carry_out=CARRY_OUT), dict(carry_out=CARRY_OUT), dict(carry_in=CARRY_IN),
               dict(out=None, carry_out=CARRY_OUT, carry_in=CARRY_IN)):
        assert _call(null_at=1, **kw) == _abi.FA_EINVAL and "updates[1] is NULL" in _err(), kw
        assert _call(P=0, **kw) == _abi.FA_OK, kw
    assert _call(out=None, carry_in=CARRY_IN) == _abi.FA_EINVAL and "null pointer" in _err()


def test_coefficients_are_judged_in_the_compute_type():
    coef = [1e39, 0.0, 0.5, 0.0]
    for ud in (_abi.FA_F32, _abi.FA_F16, _abi.FA_BF16):
        assert _call(ud=ud, coef=coef, P=0) == _abi.FA_EINVAL
    for ud in (_abi.FA_F64, _abi.FA_I32, _abi.FA_I64):
        assert _call(ud=ud, coef=coef, P=0) == _abi.FA_OK


@pytest.mark.parametrize("ud", SIX)
def test_all_zero_coefficients_and_empty_buffers_are_legal(ud):
    for K in (1, 4, 64):
        assert _call(ud=ud, K=K, coef=[0.0] * K, P=0) == _abi.FA_OK
        # all zero at P > 0 passes the checks too: refused only by the null client behind them
        assert _call(ud=ud, K=K, coef=[0.0] * K, null_at=0) == _abi.FA_EINVAL and "updates[0] is NULL" in _err()
    assert _call(ud=ud, coef=[1e-60, 0.0, 1e-50, 0.0], P=0) == _abi.FA_OK
    assert _call(ud=ud, K=3, P=0, null_at=1) == _abi.FA_OK, "an empty buffer may be a null pointer"


@pytest.mark.parametrize("ud", [_abi.FA_I8, _abi.FA_I16, _abi.FA_U8, _abi.FA_U16, _abi.FA_U32, _abi.FA_U64, _abi.FA_NONE, 99])
def test_dtype_errors(ud):
    assert _call(ud=ud) == _abi.FA_EDTYPE
    assert _err()
    assert _call(ud=ud, K=65) == _abi.FA_EINVAL, "the argument checks come first"


@pytest.mark.parametrize("ud", SIX)
def test_output_dtype_is_the_tables(ud):
    for od in SIX + [_abi.FA_I8, _abi.FA_NONE]:
        want = _abi.FA_OK if od == OUT_OF[ud] else _abi.FA_EDTYPE
        assert _call(ud=ud, od=od, P=0) == want, (ud, od)
        assert _call(ud=ud, od=od, out=None, carry_out=CARRY_OUT, P=0) == want, "a NULL out still names its dtype"


@pytest.mark.parametrize("ud", SIX)
def test_aliasing(ud):
    """The two legal aliases pass the overlap check (refused only by what comes later, a null client); every
    other overlap among out, the carries, the centre and an update is FA_EINVAL, with extents in each
    buffer's own element size; at P = 0 nothing overlaps."""
    P = 100
    osz, csz, tsz = SIZE[OUT_OF[ud]], C_SIZE[ud], SIZE[ud]

    def legal(**kw):
        assert _call(ud=ud, P=P, null_at=1, **kw) == _abi.FA_EINVAL and "updates[1] is NULL" in _err(), (kw, _err())
        assert _call(ud=ud, P=0, **kw) == _abi.FA_OK, kw

    def illegal(**kw):
        assert _call(ud=ud, P=P, **kw) == _abi.FA_EINVAL
        msg = _err()
        assert "overlap" in msg, (kw, msg)
        assert _call(ud=ud, P=0, **kw) == _abi.FA_OK, kw
        return msg

    legal(out=CENTER)                                                   # in place
    legal(carry_in=CARRY_IN, carry_out=CARRY_IN)                        # the carry handed on in place
    legal(out=CENTER, carry_in=CARRY_IN, carry_out=CARRY_IN)
    legal(out=CENTER + P * osz)                                         # adjacent: disjoint
    legal(out=CENTER - P * osz)
    legal(carry_in=CARRY_IN, carry_out=CARRY_IN + P * csz)
    for off in (osz, (P - 1) * osz, -osz, -(P - 1) * osz):              # out across the centre
        illegal(out=CENTER + off)
    for off in (csz, (P - 1) * csz, -csz, -(P - 1) * csz):              # one carry across the other
        illegal(carry_in=CARRY_IN, carry_out=CARRY_IN + off)
    last_o, last_c, last_t = (P - 1) * osz, (P - 1) * csz, (P - 1) * tsz
    illegal(carry_out=OUT)                                              # out / carry_out
    illegal(carry_out=OUT + last_o)
    illegal(carry_out=OUT - last_c)
    illegal(carry_in=OUT)                                               # out / carry_in
    illegal(carry_in=OUT + last_o)
    illegal(carry_out=CENTER)                                           # a carry / the centre
    illegal(carry_out=CENTER - last_c)
    illegal(carry_in=CENTER + last_o)
    illegal(out=CENTER, carry_in=CENTER)
    for k in (0, 3):                                                    # each of the four / an update
        u = UPDATES + UPD_STRIDE * k
        illegal(out=u)
        illegal(out=u + last_t)
        illegal(out=u - last_o)
        illegal(out=None, carry_out=u)
        illegal(carry_in=u + last_t)
        illegal(center=u)
        illegal(upd_at=(k, CENTER - last_t))
        assert f"updates[{k}]" in illegal(upd_at=(k, OUT + last_o))


# ---- the plug-ins' caps -----------------------------------------------------------------------------
def test_admission_caps():
    from fedn_amd import ops
    from fedn_amd.aggregators import bulyan, centeredclip, dpfedavg, geomedian, krum, median, multikrum, trimmedmean
    assert ops.MAX_CLIP_K == 1024 and ops.MAX_ORDER_K == 64
    assert dpfedavg.Aggregator.max_updates == ops.MAX_CLIP_K == 1024
    for mod in (trimmedmean, median, krum, multikrum, geomedian, centeredclip, bulyan):
        assert mod.Aggregator.max_updates == ops.MAX_ORDER_K == 64, mod.__name__


def test_pipeline_caps_are_per_rule():
    """``_clients`` with the rule's cap, on a pipeline object that never saw a device."""
    from fedn_amd import ops, robust
    pipe = object.__new__(robust.RobustPipeline)
    for K, cap, ok in ((64, None, True), (65, None, False), (65, ops.MAX_CLIP_K, True), (1024, ops.MAX_CLIP_K, True),
                       (1025, ops.MAX_CLIP_K, False), (0, ops.MAX_CLIP_K, False)):
        pipe.updates = [None] * K
        if ok:
            assert (pipe._clients() if cap is None else pipe._clients(cap)) == K
        else:
            with pytest.raises(ValueError, match=f"1..{cap or 64} updates, got {K}"):
                pipe._clients() if cap is None else pipe._clients(cap)


# ---- the chunk-carried restatement --------------------------------------------------------------------
SPEC = [((37, 11), np.float32), ((129,), np.float16), ((5, 7), np.int32), ((1001,), np.float32), ((), np.float16)]
CLIP = 18.0


def carried_step(S, v, coef, cut):
    """``cclip_ref.step`` restated as the chain of ``fa_clip_fold`` launches: chunks of ``cut`` clients, the
    accumulator carried in the compute type, the differences always to the unmoved centre."""
    S, v = np.asarray(S), np.asarray(v)
    C, O = kr.compute_dtype(S.dtype), rr.out_dtype(S.dtype)
    with np.errstate(all="ignore"):
        vc = v.astype(C)
        carry = None
        for c0 in range(0, S.shape[0], cut):
            acc = vc.copy() if carry is None else carry.copy()
            for k in range(c0, min(S.shape[0], c0 + cut)):
                c = C.type(coef[k])
                if c == 0:
                    continue
                acc = acc + c * (S[k].astype(C) - vc)
            carry = np.asarray(acc, dtype=C)
        return carry.astype(O)


def chained_step(S, v, coef, cut):
    """What does NOT work: ``fa_centered_clip_step`` once per chunk, each call rounding the point to O and
    taking the next chunk's differences to the moved point."""
    for c0 in range(0, len(S), cut):
        v = cr.step(S[c0:c0 + cut], v, coef[c0:c0 + cut])
    return v


@pytest.mark.parametrize("K", [64, 65, 129, 200])
def test_carried_fold_is_the_one_shot_step(K):
    ups, _, center = center_round_updates(K, K, 0, SPEC)
    v0 = cr.model_center(ups, center)
    coef = cr.coefficients(cr.model_dists(ups, v0), CLIP)
    assert 0 < sum(c < 1.0 / K for c in coef) < K, "clipped and unclipped clients both exist"
    for i in range(len(SPEC)):
        S, v = cr._rows(ups, i), v0[i].reshape(-1)
        want = cr.step(S, v, coef)
        for cut in (64, 7, 1):
            got = carried_step(S, v, coef, cut)
            assert got.dtype == want.dtype and np.array_equal(got.view(f"u{got.itemsize}"), want.view(f"u{want.itemsize}")), (K, i, cut)
    if K > 64:
        S, v = cr._rows(ups, 0), v0[0].reshape(-1)
        differ = chained_step(S, v, coef, 64) != cr.step(S, v, coef)
        assert differ.mean() > 0.9, "one fa_centered_clip_step per chunk is another rule, not another rounding"
