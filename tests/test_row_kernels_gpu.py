"""GPU suite, kernel level: the LayerNorm kernel with the fields a forward sets (gathered residual, device-side row count, reversed walk, e4m3
copy, skip word) against the fp64 LayerNorm, and the fp8 / split-plane conversion kernels against the OCP e4m3 tables of oracle/fp8.py."""
import ctypes as C

import numpy as np
import pytest
import torch

import helpers
from kddcup_2020_multimodalitiesrecall_2nd_place_amd import lib, weights
from oracle import fp8

pytestmark = pytest.mark.gpu

REV, F8, SKIP = 1, 2, 4


def _dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


def _ln_inputs():
    M = 77      # test_layernorm_matches_fp64's inputs
    x = weights.normal("kt/lnx", (M, 768), 3, 2.0, 0.5)
    g = weights.normal("kt/lng", (768,), 3, 0.1, 1.0)
    b = weights.normal("kt/lnb", (768,), 3, 0.1)
    return M, x, g, b


def _ln(x, g, b, resid, r_index, m_live, flags):
    l = lib.load()
    M = x.shape[0]
    out = torch.full((M, 768), 7.0, device="cuda", dtype=torch.float32)
    out8 = torch.full((M, 768), 7.0, device="cuda", dtype=torch.float32)
    hold = [_dev(x), _dev(g), _dev(b), None if resid is None else _dev(resid), None if r_index is None else _dev(r_index.astype(np.int32))]
    p = [None if t is None else t.data_ptr() for t in hold]
    rc = l.mms_dbg_layernorm_ex(p[0], p[1], p[2], M, p[3], 0 if resid is None else resid.shape[0], p[4], m_live, flags, out.data_ptr(),
                                out8.data_ptr() if flags & F8 else None, None)
    assert rc == 0, l.mms_global_error()
    return out.cpu().numpy(), out8.cpu().numpy()


def _ln_ref(x, g, b):
    x64 = x.astype(np.float64)
    mu = x64.mean(-1, keepdims=True)
    return (x64 - mu) / np.sqrt(((x64 - mu) ** 2).mean(-1, keepdims=True) + 1e-12) * g + b


def _split_join(v):
    """what a reader of split planes gets: hi = bf16(v), lo = bf16(v - hi) (the difference is exact in fp32), joined by one fp32 addition"""
    v = np.asarray(v, np.float32)
    hi = weights.round_to_bf16(v)
    return (hi + weights.round_to_bf16(v - hi)).astype(np.float64)


def test_layernorm_with_gathered_residual_row_count_and_direction():
    M, x, g, b = _ln_inputs()
    R = 41
    resid = weights.normal("rk/resid", (R, 768), 3, 1.5)
    r_index = np.random.default_rng(11).integers(0, R, M)            # a gather with repeated entries ...
    r_index[:R] = np.random.default_rng(12).permutation(R)           # ... over a permutation
    ref = _ln_ref((x.astype(np.float64) + _split_join(resid)[r_index]).astype(np.float64), g, b)
    got, _ = _ln(x, g, b, resid, r_index, -1, 0)
    err = np.abs(got - ref).max()
    print("LayerNorm + gathered residual: worst error %.2e (bound 5e-5)" % err)
    assert err < 5e-5
    live = M - 3                                                     # device-side row count: the last three rows are not written
    part, _ = _ln(x, g, b, resid, r_index, live, 0)
    assert np.array_equal(part[:live], got[:live]) and np.all(part[live:] == 0.0)
    for m_live in (-1, live):
        rev, _ = _ln(x, g, b, resid, r_index, m_live, REV)
        assert np.array_equal(rev, got if m_live < 0 else part), m_live
    plain, _ = _ln(x, g, b, None, None, -1, 0)
    assert np.abs(plain - _ln_ref(x, g, b)).max() < 5e-5
    skipped, s8 = _ln(x, g, b, resid, r_index, -1, SKIP | F8)        # the producing GEMM already normalised: nothing is written
    assert np.all(skipped == 0.0) and np.all(s8 == 0.0)


def _ln_rows(x, g, b, resid, rmap, m_live, flags, expect=0):
    """mms_dbg_layernorm_rows: the LayerNorm kernel with LnResid::rmap = {grp, stride, off}"""
    l = lib.load()
    M = x.shape[0]
    out = torch.full((M, 768), 7.0, device="cuda", dtype=torch.float32)
    hold = [_dev(x), _dev(g), _dev(b), _dev(resid)]
    rc = l.mms_dbg_layernorm_rows(hold[0].data_ptr(), hold[1].data_ptr(), hold[2].data_ptr(), M, hold[3].data_ptr(), resid.shape[0], None, m_live, flags,
                                  out.data_ptr(), None, (C.c_int32 * 3)(*rmap), None)
    assert rc == expect, l.mms_global_error()
    return out.cpu().numpy()


def test_layernorm_with_a_row_mapped_residual():
    """LnResid::rmap = {1, 30, 0}: row r adds residual row 30 r (the CLS-only last layer's residual through the dense token stream).  Every residual row the
    map does not address holds NaN; same reference and bound as the r_index case, bit-identical to the r_index launch that names the same rows, with and
    without a live count and reversed; a map that leaves the residual is refused on the host."""
    M, x, g, b = _ln_inputs()
    rmap = (1, 30, 0)
    rows = helpers.rowmap(np.arange(M), *rmap)
    dense = weights.normal("rk/resid_map", (M, 768), 3, 1.5)
    resid = np.full((M * rmap[1], 768), np.nan, np.float32)
    resid[rows] = dense
    ref = _ln_ref(x.astype(np.float64) + _split_join(dense), g, b)
    got = _ln_rows(x, g, b, resid, rmap, -1, 0)
    err = np.abs(got - ref).max()
    print("LayerNorm + row-mapped residual: worst error %.2e (bound 5e-5)" % err)
    assert err < 5e-5
    assert np.array_equal(got, _ln(x, g, b, resid, rows, -1, 0)[0])
    live = M - 3
    for flags in (0, REV):
        part = _ln_rows(x, g, b, resid, rmap, live, flags)
        assert np.array_equal(part[:live], got[:live]) and np.all(part[live:] == 0.0), flags
    short = _ln_rows(x, g, b, resid[:-rmap[1]], rmap, -1, 0, expect=1)      # the last row's residual lies outside: MMS_ERR_ARG before any launch
    assert np.all(short == 7.0)


def test_layernorm_fp8_copy():
    """Precision 4: the row also leaves as e4m3 bytes; checked as the attention context is, with the LayerNorm test's own bound as delta."""
    M, x, g, b = _ln_inputs()
    ref = _ln_ref(x, g, b)
    exc, _, _ = helpers.f8_excused(ref, 5e-5)
    assert exc.mean() <= 0.01, exc.mean()                            # before the device output is looked at
    planes, got8 = _ln(x, g, b, None, None, -1, F8)
    assert np.abs(planes - ref).max() < 5e-5
    helpers.f8_store_check(ref, got8, 5e-5, 0.01, "LayerNorm o_f8")
    part, part8 = _ln(x, g, b, None, None, M - 3, F8 | REV)
    assert np.array_equal(part8[:M - 3], got8[:M - 3]) and np.all(part8[M - 3:] == 0.0) and np.all(part[M - 3:] == 0.0)


def _convert(kind, a, out_dtype):
    l = lib.load()
    n = a.size
    pad = (-n) % 32
    a = np.concatenate([a.ravel(), np.zeros(pad, a.dtype)])
    d = _dev(a)
    out = torch.zeros(a.size, device="cuda", dtype=out_dtype)
    rc = l.mms_dbg_convert(kind, d.data_ptr(), out.data_ptr(), a.size, None)
    assert rc == 0, l.mms_global_error()
    return out.cpu().numpy()[:n]


CODES = np.arange(256, dtype=np.uint8)
VALUES = fp8.e4m3_decode(CODES)
FINITE = np.isfinite(VALUES)


def _decode(b):
    return VALUES[b.astype(np.int64)]


def test_f8_to_f32_decodes_every_code():
    got = _convert(1, CODES, torch.float32)
    assert np.array_equal(got[FINITE].astype(np.float64), VALUES[FINITE])
    assert np.array_equal(np.signbit(got[FINITE]), (CODES[FINITE] & 0x80) != 0)         # -0 keeps its sign
    assert np.isnan(got[0x7F]) and np.isnan(got[0xFF]) and FINITE.sum() == 254


def test_f32_to_f8_rounds_to_nearest_even_and_saturates():
    # every finite code's own value comes back as that code (+-0 included)
    exact = VALUES[FINITE].astype(np.float32)
    assert np.array_equal(_convert(0, exact, torch.uint8), CODES[FINITE])
    # every midpoint of two neighbouring codes: ties to even (the code with mantissa bit 0 clear); 2^-10, half the smallest subnormal, goes to 0
    pos = np.sort(VALUES[:0x7F])                                                         # 0 .. 448
    mids = ((pos[1:] + pos[:-1]) / 2).astype(np.float32)
    assert np.array_equal(mids.astype(np.float64), (pos[1:] + pos[:-1]) / 2)           # the midpoints are fp32 numbers
    for sign in (1.0, -1.0):
        m = (sign * mids).astype(np.float32)
        got = _convert(0, m, torch.uint8)
        lo_code = np.arange(0x7E) | (0x80 if sign < 0 else 0)
        want = np.where(lo_code & 1, lo_code + 1, lo_code)
        assert np.array_equal(got, want), sign
        assert np.array_equal(_decode(got), fp8.e4m3_round(m))
        assert _decode(got[:1])[0] == 0.0 and abs(m[0]) == 2.0 ** -10
        # one fp32 ulp to either side of the tie: the nearer neighbour
        for step in (np.inf, -np.inf):
            near = np.nextafter(m, np.float32(step))
            g2 = _decode(_convert(0, near, torch.uint8))
            assert np.array_equal(g2, fp8.e4m3_round(near)), (sign, step)
            assert np.array_equal(g2, np.where((near > m) == (sign > 0), sign * pos[1:], sign * pos[:-1])), (sign, step)
    # saturation (csrc/common.h pack4_f8): beyond +-448 the largest finite code, infinities included
    big = np.array([448.0, 449.0, 464.0, 1e9, np.inf], np.float32)
    assert np.all(_convert(0, big, torch.uint8) == 0x7E) and np.all(_convert(0, -big, torch.uint8) == 0xFE)
    z = _convert(0, np.array([0.0, -0.0], np.float32), torch.uint8)
    assert list(z) == [0x00, 0x80]


def test_f32_to_f8_nan_saturates():
    """pack4_f8 clamps with fminf(fmaxf(x, -448), 448) before the hardware conversion, and fmaxf returns its non-NaN operand: a NaN becomes -448
    (0xFE), it does NOT stay NaN as oracle.fp8.e4m3_round leaves it.  A NaN activation therefore cannot be seen in precision 4's outputs; the rule is
    documented in common.h, mmscore.h (precision 4) and oracle/fp8.py, and pinned here so that a change of it is a decision."""
    x = np.array([np.nan, 1.0, -np.nan, 2.0], np.float32)
    got = _convert(0, x, torch.uint8)
    print("f32_to_f8(NaN) -> 0x%02X, f32_to_f8(-NaN) -> 0x%02X" % (got[0], got[2]))
    assert list(got) == [0xFE, 0x38, 0xFE, 0x40]
    via_planes = _convert(3, np.array([np.nan, 1.0, 3.0, -2.0], np.float32), torch.uint8)
    print("planes_to_f8(split(NaN)) -> 0x%02X" % via_planes[0])
    assert list(via_planes) == [0xFE, 0x38, 0x44, 0xC0]


def test_split_planes_round_trip():
    v = weights.normal("rk/planes", (4096,), 5, 3.0)
    v[:8] = [1e-20, -1e-20, 1e20, -1e20, 1.0, -1.0, 0.0, 3.0e-5]
    back = _convert(2, v, torch.float32)
    v64 = v.astype(np.float64)
    rel = np.abs(back.astype(np.float64) - v64) / np.where(v64 == 0, 1.0, np.abs(v64))
    print("split planes round trip: worst relative error %.2e (bound 2^-16 = %.2e)" % (rel.max(), 2.0 ** -16))
    assert rel.max() <= 2.0 ** -16
    assert np.array_equal(back.astype(np.float64), _split_join(v))                      # hi = bf16(v), lo = bf16(v - hi), joined in fp32
    exact = weights.round_to_bf16(v)
    assert np.array_equal(_convert(2, exact, torch.float32), exact)                    # bf16 numbers pass unchanged
    # planes -> e4m3: the rounding of the joined value
    got8 = _decode(_convert(3, v, torch.uint8))
    assert np.array_equal(got8, fp8.e4m3_round(back))
