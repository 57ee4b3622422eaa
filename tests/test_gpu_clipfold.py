"""The chunked clipping fold on the GPU: ``fa_clip_fold`` (kernel ``k_clip_fold``) through
``ops.clip_fold`` against the oracle tests/cclip_ref.py — bit for bit, one launch and chains of launches cut
anywhere, in place as out of place, on and off 16-byte alignment, with nothing written outside the buffers
(tests/guarded_buf.py) and no input changed."""
import numpy as np
import pytest
import torch

import cclip_ref as cr
from guarded_buf import Buf
from robust_checks import same_bits

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
PS = [1, 5, 255, 256, 257, 4099, 65579]
KS = [1, 2, 7, 8, 9, 63, 64]
DTYPES = ["f32", "f64", "f16", "bf16", "i32", "i64"]
NP_DT = {"f32": np.float32, "f64": np.float64, "f16": np.float16, "bf16": np.float32, "i32": np.int32, "i64": np.int64}
TORCH_DT = {"f32": torch.float32, "f64": torch.float64, "f16": torch.float16, "bf16": torch.bfloat16,
            "i32": torch.int32, "i64": torch.int64}
O_NAME = {"f32": "f32", "f64": "f64", "f16": "f16", "bf16": "f32", "i32": "f64", "i64": "f64"}     # the output type
C_NAME = {"f32": "f32", "f64": "f64", "f16": "f32", "bf16": "f32", "i32": "f64", "i64": "f64"}     # the compute type
EV = {"f32": 4, "f64": 2, "f16": 8, "bf16": 8, "i32": 4, "i64": 2}                                  # elements of an item
MAX_BLOCKS, BLOCK = 2048, 256                                                                       # kClipMaxBlocks, kBlock


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device")
    from fedn_amd import _abi
    _abi.load()
    yield
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def _data(rng, name, K, n):
    """K updates close to each other — a base plus small noise — and a centre, the base plus other small
    noise, in the output type. Integer values are not all exact in float64 (int64)."""
    dt = np.dtype(NP_DT[name])
    base = rng.standard_normal(n)
    x = base + 0.05 * rng.standard_normal((K, n))
    v = base + 0.02 * rng.standard_normal(n)
    if dt.kind == "i":
        scale = 2.0 ** 20 if name == "i32" else 2.0 ** 40
        x, v = np.round(x * scale).astype(dt), np.round(v * scale)
        if name == "i64":
            q = max(1, n // 8)
            x[:, :q] += 2 ** 53 + 1
            v[:q] += 2.0 ** 53
        return np.ascontiguousarray(x), np.ascontiguousarray(v)
    x, v = x.astype(dt), v.astype(NP_DT[O_NAME[name]])
    if name == "bf16":
        x = (np.ascontiguousarray(x).view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32)
    return np.ascontiguousarray(x), np.ascontiguousarray(v)


class Ups:
    """K updates as rows of one device matrix, each row 16-byte aligned plus ``shift`` elements; the rows'
    bits are checked unchanged at the end."""

    def __init__(self, S, name, shift=0):
        K, n = S.shape
        row = -(-(n + 1) // 64) * 64
        t = torch.from_numpy(np.ascontiguousarray(S))
        self.m = torch.zeros((K, row), dtype=TORCH_DT[name], device=DEV)
        self.m[:, shift:shift + n].copy_(t.to(DEV).to(TORCH_DT[name]))          # (bf16: exact, the values are bf16's)
        self.shift, self.K = shift, K
        self.bits0 = self._bits()

    def _bits(self):
        return self.m.view({2: torch.int16, 4: torch.int32, 8: torch.int64}[self.m.element_size()]).cpu().numpy()

    def views(self, P, ks=None):
        return [self.m[k, self.shift:self.shift + P] for k in (range(self.K) if ks is None else ks)]

    def check_unchanged(self, what):
        assert np.array_equal(self._bits(), self.bits0), f"{what}: an update was overwritten"


def _coef(rng, K):
    """Random coefficients in (0, 1 / K], one of them exactly 0 (K > 1)."""
    coef = rng.uniform(0.05, 1.0, K) / K
    if K > 1:
        coef[int(rng.integers(0, K))] = 0.0
    return coef.tolist()


def _same(buf, want, what):
    buf.check(what, True)
    want = np.ascontiguousarray(want)
    assert np.array_equal(buf.bits(), want.view(buf.bits().dtype)), f"{what}: bits differ from the oracle"


# ---- one launch ------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("name", DTYPES)
def test_one_launch_is_the_oracle_and_the_fused_kernel(name, K):
    """Every P, everything on and everything one element off 16-byte alignment: ``out`` equals
    ``cclip_ref.step`` and ``ops.centered_clip_step``'s v' bit for bit; so does a chain of two launches through
    a carry; guards untouched, inputs unchanged."""
    from fedn_amd import ops
    rng = np.random.default_rng(100 * DTYPES.index(name) + K)
    S, v = _data(rng, name, K, PS[-1])
    coef = _coef(rng, K)
    zw = cr.step(S, v, coef)                                   # per element: a prefix's step is a prefix of it
    h = (K + 1) // 2
    for shift in (0, 1):
        ups = Ups(S, name, shift)
        for P in PS:
            what = f"{name} K={K} P={P} shift={shift}"
            cen, out = Buf(P, O_NAME[name], shift, data=v[:P]), Buf(P, O_NAME[name], shift)
            got, none = ops.clip_fold(ups.views(P), cen.t, coef, out=out.t)
            assert got is out.t and none is None and ops.last_kernel() == "k_clip_fold"
            _same(out, zw[:P], what)
            z, _ = ops.centered_clip_step(ups.views(P), cen.t, coef)
            same_bits(z.cpu().numpy(), zw[:P], f"{what}: the fused kernel")
            if K > 1:                                          # two launches, the accumulator through a carry
                carry, out2 = Buf(P, C_NAME[name], shift), Buf(P, O_NAME[name], shift)
                ops.clip_fold(ups.views(P, range(h)), cen.t, coef[:h], carry_out=carry.t)
                carry.check(f"{what}: carry", True)
                out2.check(f"{what}: out before the last launch", False)
                ops.clip_fold(ups.views(P, range(h, K)), cen.t, coef[h:], carry_in=carry.t, out=out2.t)
                _same(out2, zw[:P], f"{what}: two launches")
            cen.check_unchanged(what)
        ups.check_unchanged(f"{name} K={K} shift={shift}")


@pytest.mark.parametrize("name", DTYPES)
def test_mixed_alignment_takes_the_element_path(name):
    """One buffer alone off alignment — the centre, out, the carry, one update — gives the same bits."""
    from fedn_amd import ops
    K, P = 9, 4099
    rng = np.random.default_rng(7 + DTYPES.index(name))
    S, v = _data(rng, name, K, P)
    coef = _coef(rng, K)
    zw = cr.step(S, v, coef)
    ups = Ups(S, name)
    odd = Ups(S[4:5], name, 1)
    for s_cen, s_out, s_carry, s_up in [(1, 0, 0, 0), (0, 1, 0, 0), (0, 0, 1, 0), (0, 0, 0, 1)]:
        what = f"{name}: shifts {(s_cen, s_out, s_carry, s_up)}"
        views = ups.views(P)
        if s_up:
            views[4] = odd.views(P)[0]
        cen, out, carry = Buf(P, O_NAME[name], s_cen, data=v), Buf(P, O_NAME[name], s_out), Buf(P, C_NAME[name], s_carry)
        ops.clip_fold(views[:5], cen.t, coef[:5], carry_out=carry.t)
        ops.clip_fold(views[5:], cen.t, coef[5:], carry_in=carry.t, out=out.t)
        carry.check(what, True)
        _same(out, zw, what)
        cen.check_unchanged(what)


@pytest.mark.parametrize("name", DTYPES)
def test_grid_stride_beyond_the_cap(name):
    """A size past the grid's cap, where every lane walks more than two items, ragged at the end."""
    from fedn_amd import ops
    K = 3
    P = 2 * MAX_BLOCKS * BLOCK * EV[name] + 257 * EV[name] + 3
    rng = np.random.default_rng(40 + DTYPES.index(name))
    S, v = _data(rng, name, K, P)
    coef = _coef(rng, K)
    ups = Ups(S, name)
    cen, out = Buf(P, O_NAME[name], data=v), Buf(P, O_NAME[name])
    ops.clip_fold(ups.views(P), cen.t, coef, out=out.t)
    _same(out, cr.step(S, v, coef), f"{name} P={P}")
    ops.clip_fold(ups.views(P), cen.t, coef, out=cen.t)
    _same(cen, cr.step(S, v, coef), f"{name} P={P}: in place")


# ---- aliasing --------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [9, 64])
@pytest.mark.parametrize("name", DTYPES)
def test_in_place_and_carry_in_place(name, K):
    """``out is center`` on the last launch and ``carry_in is carry_out`` on the ones between: the bits of the
    out-of-place chain, aligned and one element off."""
    from fedn_amd import ops
    rng = np.random.default_rng(300 + 10 * DTYPES.index(name) + K)
    S, v = _data(rng, name, K, PS[-1])
    coef = _coef(rng, K)
    zw = cr.step(S, v, coef)
    cuts = [0, K // 3, 2 * K // 3, K]
    for shift in (0, 1):
        ups = Ups(S, name, shift)
        for P in (257, 4099, 65579):
            what = f"{name} K={K} P={P} shift={shift}"
            cen = Buf(P, O_NAME[name], shift, data=v[:P])
            ops.clip_fold(ups.views(P), cen.t, coef, out=cen.t)
            _same(cen, zw[:P], f"{what}: one launch in place")
            cen, carry = Buf(P, O_NAME[name], shift, data=v[:P]), Buf(P, C_NAME[name], shift)
            for i in range(3):
                ks = range(cuts[i], cuts[i + 1])
                ops.clip_fold(ups.views(P, ks), cen.t, coef[cuts[i]:cuts[i + 1]], out=cen.t if i == 2 else None,
                              carry_in=carry.t if i else None, carry_out=carry.t if i < 2 else None)
                if i < 2:
                    cen.check_unchanged(f"{what}: the centre before the last launch")
            carry.check(what, True)
            _same(cen, zw[:P], f"{what}: three launches, the carry and the centre in place")
        ups.check_unchanged(f"{name} K={K} shift={shift}")


# ---- special values --------------------------------------------------------------------------------
@pytest.mark.parametrize("name", DTYPES)
def test_zero_coefficients(name):
    """Zero coefficients first, last, scattered and all; all zero gives O(C(v)), the centre's bits with its
    -0; a zero-coefficient client's NaN and inf are absent from v'."""
    from fedn_amd import ops
    K, P = 9, 257
    rng = np.random.default_rng(500 + DTYPES.index(name))
    S, v = _data(rng, name, K, P)
    v[:4] = [-0.0, 0.0, -1.0, 1.0]
    floating = np.dtype(NP_DT[name]).kind == "f"
    live = rng.uniform(0.05, 1.0, K) / K
    for zero in ([0], [K - 1], [0, K - 1], [1, 4, 5, 7], list(range(1, K)), list(range(K))):
        what = f"{name}: zero coefficients at {zero}"
        coef = live.copy()
        coef[zero] = 0.0
        Sz = S.copy()
        if floating:                                           # poison what must not be read
            Sz[zero, 3] = np.nan
            Sz[zero, 200] = np.inf
        ups = Ups(Sz, name)
        cen, out = Buf(P, O_NAME[name], data=v), Buf(P, O_NAME[name])
        ops.clip_fold(ups.views(P), cen.t, coef.tolist(), out=out.t)
        want = cr.step(Sz, v, coef)
        assert np.isfinite(want).all()
        _same(out, want, what)
        if len(zero) == K:
            _same(out, v, f"{what}: the centre's bits")
            carry = Buf(P, C_NAME[name])
            ops.clip_fold(ups.views(P), cen.t, coef.tolist(), carry_out=carry.t)
            _same(carry, v.astype(NP_DT[C_NAME[name]]), f"{what}: the carry is C(v)")


@pytest.mark.parametrize("name", ["f32", "f64", "f16", "bf16"])
def test_non_finite_values_in_a_live_client(name):
    """A NaN and an inf in a client with a nonzero coefficient reach their own elements only."""
    from fedn_amd import ops
    K, P = 7, 257
    rng = np.random.default_rng(600 + DTYPES.index(name))
    S, v = _data(rng, name, K, P)
    v[8:10] = [-0.0, 0.0]
    S[2, 5], S[4, 129], S[6, 256] = np.nan, np.inf, -np.inf
    coef = (rng.uniform(0.05, 1.0, K) / K).tolist()
    want = cr.step(S, v, coef)
    assert np.isnan(want[5]) and want[129] == np.inf and want[256] == -np.inf
    assert int((~np.isfinite(want)).sum()) == 3
    ups = Ups(S, name)
    cen, out = Buf(P, O_NAME[name], data=v), Buf(P, O_NAME[name])
    ops.clip_fold(ups.views(P), cen.t, coef, out=out.t)
    out.check(name, True)
    got = out.numpy()
    assert np.isnan(got[5]), "the NaN's element"
    keep = np.arange(P) != 5                                   # (a NaN's payload is the hardware's)
    same_bits(got[keep], want[keep], f"{name}: every other element, the infinities included")


# ---- chains ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [65, 128, 129, 200])
@pytest.mark.parametrize("name", DTYPES)
def test_chains_cut_anywhere(name, K):
    """K > 64 clients as chains of launches of 64, of 7 and of 1: all bit-identical to ``cclip_ref.step`` over
    all K. Clients 7 .. 13 have coefficient 0, so one launch of the chain of 7 folds nothing and hands the
    carry on."""
    from fedn_amd import ops
    P = 4099
    rng = np.random.default_rng(700 + 10 * DTYPES.index(name) + K)
    S, v = _data(rng, name, K, P)
    coef = rng.uniform(0.05, 1.0, K) / K
    coef[7:14] = 0.0
    coef[int(rng.integers(64, K))] = 0.0
    coef = coef.tolist()
    zw = cr.step(S, v, coef)
    ups = Ups(S, name)
    cen = Buf(P, O_NAME[name], data=v)
    for cut in (64, 7, 1):
        what = f"{name} K={K} launches of {cut}"
        out, carry = Buf(P, O_NAME[name]), Buf(P, C_NAME[name])
        bounds = list(range(0, K, cut)) + [K]
        for i, (c0, c1) in enumerate(zip(bounds, bounds[1:])):
            first, last = i == 0, c1 == K
            ops.clip_fold(ups.views(P, range(c0, c1)), cen.t, coef[c0:c1], out=out.t if last else None,
                          carry_in=None if first else carry.t, carry_out=None if last else carry.t)
        carry.check(what, True)
        _same(out, zw, what)
    cen.check_unchanged(f"{name} K={K}")
    ups.check_unchanged(f"{name} K={K}")


# ---- refusals --------------------------------------------------------------------------------------
def test_ops_refuses_bad_arguments():
    from fedn_amd import ops
    P = 64
    x = torch.ones(P, device=DEV)
    cen, out, carry = Buf(P, "f32", data=np.zeros(P, np.float32)), Buf(P, "f32"), Buf(P, "f32")
    big = torch.ones(2 * P, device=DEV)
    with pytest.raises(ValueError, match="1..64 updates, got 65"):
        ops.clip_fold([x] * 65, cen.t, [0.01] * 65, out=out.t)
    with pytest.raises(ValueError, match="1..64 updates, got 0"):
        ops.clip_fold([], cen.t, [], out=out.t)
    with pytest.raises(ValueError, match="coefficients"):
        ops.clip_fold([x, x], cen.t, [0.5], out=out.t)
    with pytest.raises(ValueError, match="one of out and carry_out"):
        ops.clip_fold([x], cen.t, [0.5])
    with pytest.raises(TypeError):
        ops.clip_fold([x], cen.t.double(), [0.5], out=out.t)                       # the centre is not in O
    with pytest.raises(TypeError):
        ops.clip_fold([x], cen.t, [0.5], out=out.t.double())
    with pytest.raises(TypeError):
        ops.clip_fold([x], cen.t, [0.5], carry_out=carry.t.double())               # a carry is in C
    with pytest.raises(TypeError):
        ops.clip_fold([x], cen.t, [0.5], out=out.t, carry_in=carry.t.half())
    with pytest.raises(TypeError):
        ops.clip_fold([x.half()], cen.t, [0.5], out=out.t)                         # f16 updates move an f16 centre
    with pytest.raises(TypeError):
        ops.clip_fold([x.to(torch.int8)], cen.t, [0.5], out=out.t)
    with pytest.raises(ValueError):
        ops.clip_fold([x], cen.t, [0.5], out=out.t[:32])
    for kw in (dict(out=big[1:P + 1], center=big[:P]), dict(out=big[:P], carry_out=big[P - 1:2 * P - 1]),
               dict(out=out.t, carry_in=out.t), dict(carry_in=big[:P], carry_out=big[1:P + 1], out=out.t),
               dict(carry_out=cen.t), dict(out=x), dict(carry_out=x), dict(center=x, out=out.t), dict(carry_in=x, out=out.t)):
        kw.setdefault("center", cen.t)
        with pytest.raises(ValueError, match="overlap"):
            ops.clip_fold([x], kw.pop("center"), [0.5], **kw)
    for bad in (-0.5, float("nan"), float("inf"), 1e39):
        with pytest.raises(ops.FedAggError):
            ops.clip_fold([x], cen.t, [bad], out=out.t)
    torch.cuda.synchronize()
    out.check("refusals", False)
    carry.check("refusals", False)
    cen.check_unchanged("refusals")
    assert bool((x == 1).all()) and bool((big == 1).all()), "nothing was written"
    s = np.int32(0x7FA5A5A5)
    assert (out.bits() == s).all() and (carry.bits() == s).all(), "nothing was written"
    empty = torch.zeros(0, device=DEV)
    o, c = ops.clip_fold([empty], empty, [0.5], out=empty)               # P = 0: nothing to launch
    assert o is empty and c is None
