"""GPU: fs_loudness_normalize against the float64 referee (tests/loud_refs.py) on the case table whose gates tests/test_loud_ref_cpu.py
keeps away from ties.  Hop energies (the fs_selftest_loud_hops hook) within the bound derived in loud_refs.py; L within 1e-4 LU (the
product requirement); block counts exact; the peak bit-exact; the gain the f32 rounding of the referee's formula at the device's own L, and
within what 1e-4 LU implies of the referee's gain; the output x * gain bit for bit.  A ragged call of three rows with an empty one in the
middle returns, row by row, what the rows' own calls return, bit for bit.  Every figure is printed before it is asserted."""
import ctypes as C
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import fishrt
from fishrt import _ffi

import loud_refs as R

L_TOL = 1e-4  # LU
G_REL = 10.0 ** (L_TOL / 20.0) - 1.0 + 2.0 ** -23  # what L_TOL moves g_L by, plus the two f32 roundings (2^-24 each)


def _hops(x, rate):
    h = R.hop(rate)
    cap = max(len(x) // h, 1)
    out, n, res = np.full(cap, -1.0, np.float64), C.c_int64(-1), _ffi.LoudResult()
    xs = x if len(x) else np.zeros(1, np.float32)
    _ffi.check(_ffi.lib().fs_selftest_loud_hops(0, xs.ctypes.data_as(C.POINTER(C.c_float)), len(x), rate, out.ctypes.data_as(C.POINTER(C.c_double)),
                                                C.c_size_t(cap), C.byref(n), C.byref(res)))
    assert n.value == len(x) // h
    return out[:n.value], res


@pytest.mark.parametrize("case", R.CASES, ids=R.case_id)
def test_case_against_the_referee(case):
    kind, n, rate, seed = case
    ref = R.reference(case)
    x = ref["x"]
    # hop energies
    s, meas = _hops(x, rate)
    assert s.shape == ref["s"].shape
    fin = np.isfinite(ref["s"])
    assert np.array_equal(np.isnan(s), np.isnan(ref["s"]))  # (a NaN sample: NaN from its hop on, on both sides)
    err, bound = np.abs(s[fin] - ref["s"][fin]), ref["bound"][fin]
    worst = float(np.max(err / np.maximum(bound, 1e-300))) if fin.any() else 0.0
    rel = float(np.max(err / np.maximum(ref["s"][fin], 1e-300))) if fin.any() else 0.0
    print(f"{R.case_id(case)}: hop energy worst error / bound = {worst:.3g}, worst relative error = {rel:.3g}")
    assert np.all(err <= bound), worst
    # the record
    y, info = fishrt.loudness_normalize(x, rate, R.TARGET, return_info=True)
    print(f"  L = {info['lufs']!r} (referee {ref['lufs']!r}, |diff| = {abs(info['lufs'] - ref['lufs']) if math.isfinite(ref['lufs']) else 0.0:.3g} LU), "
          f"gain = {info['gain']!r}, peak = {info['peak']!r}, blocks {info['blocks_kept']} / {info['blocks_total']}")
    assert info["blocks_total"] == ref["blocks_total"] and info["blocks_kept"] == ref["blocks_kept"]
    assert np.float32(info["peak"]) == ref["peak"]
    if math.isfinite(ref["lufs"]):
        assert abs(info["lufs"] - ref["lufs"]) <= L_TOL
    else:
        assert info["lufs"] == -math.inf and info["gain"] == 1.0
    assert meas.lufs == info["lufs"] and meas.gain == 1.0 and np.float32(meas.peak) == ref["peak"]  # measuring only: the same L, gain 1
    assert fishrt.loudness(x, rate) == info["lufs"]
    g_own, g_ref = R.gain(info["lufs"], ref["peak"], R.TARGET), R.gain(ref["lufs"], ref["peak"], R.TARGET)
    assert np.float32(info["gain"]) == g_own, (info["gain"], g_own)
    assert abs(float(info["gain"]) / float(g_ref) - 1.0) <= G_REL
    assert y.dtype == np.float32 and np.array_equal(y, x * np.float32(info["gain"]), equal_nan=True)


def test_clauses_of_the_gain():
    spike, under = R.SIGNALS[4], R.SIGNALS[5]
    r = R.reference(spike)
    y, info = fishrt.loudness_normalize(r["x"], spike[2], R.TARGET, return_info=True)
    assert np.float32(info["gain"]) == np.float32(10.0 ** (R.PEAK_DB / 20.0) / 1.0) and np.abs(y).max() == np.float32(info["gain"])  # the peak clause
    y, info = fishrt.loudness_normalize(r["x"], spike[2], R.TARGET, peak_db=-6.0, return_info=True)
    assert np.float32(info["gain"]) == np.float32(10.0 ** (-6.0 / 20.0))
    r = R.reference(under)
    y, info = fishrt.loudness_normalize(r["x"], under[2], R.TARGET, return_info=True)
    assert np.float32(info["gain"]) == np.float32(10.0 ** (30.0 / 20.0))  # max_gain_db
    y, info = fishrt.loudness_normalize(r["x"], under[2], R.TARGET, max_gain_db=12.0, return_info=True)
    assert np.float32(info["gain"]) == np.float32(10.0 ** (12.0 / 20.0)) and np.array_equal(y, r["x"] * np.float32(info["gain"]))
    y, info = fishrt.loudness_normalize(r["x"], under[2], R.TARGET, max_gain_db=60.0, return_info=True)
    assert np.float32(info["gain"]) == R.gain(info["lufs"], r["peak"], R.TARGET, max_gain_db=60.0) and 300.0 < info["gain"] < 330.0  # the target


def test_ragged_call_rows_equal_their_own_calls():
    cases = (R.SIGNALS[2], R.SIGNALS[1], R.EDGES[14])  # the gap row, a nine-workgroup row, a two-workgroup row: 44.1 kHz all
    assert all(c[2] == 44100 for c in cases)
    xs = [R.reference(cases[0])["x"], np.zeros(0, np.float32), R.reference(cases[1])["x"], R.reference(cases[2])["x"][:4 * 4410 - 1]]
    for rows in ((xs[0], xs[1], xs[2]), (xs[2], xs[3], xs[0])):
        n = max(len(r) for r in rows)
        x = np.zeros((3, n), np.float32)
        for i, r in enumerate(rows):
            x[i, :len(r)] = r
            x[i, len(r):] = 7.0  # (behind a row's end: never read)
        ys, infos = fishrt.loudness_normalize(x, 44100, R.TARGET, lengths=[len(r) for r in rows], return_info=True)
        for i, r in enumerate(rows):
            y1, i1 = fishrt.loudness_normalize(r, 44100, R.TARGET, return_info=True) if len(r) else (r, None)
            if i1 is None:
                assert infos[i] == dict(lufs=-math.inf, peak=0.0, gain=1.0, blocks_total=0, blocks_kept=0) and ys[i].shape == (0,)
                continue
            assert np.float64(infos[i]["lufs"]).tobytes() == np.float64(i1["lufs"]).tobytes() and infos[i] == i1, (i, infos[i], i1)
            assert np.array_equal(ys[i], y1)
        assert fishrt.loudness(x, 44100, lengths=[len(r) for r in rows]) == [i["lufs"] for i in infos]


def test_rates_between_the_table_rates_and_a_2d_call():
    for rate in (11025, 16000, 32000):
        x = R.signal("mix", 6 * R.hop(rate) + 11, rate, rate)
        ref = R.measure(x, rate)
        got = fishrt.loudness(np.stack([x, x]), rate, details=True)
        assert got[0] == got[1] and abs(got[0]["lufs"] - ref["lufs"]) <= L_TOL and got[0]["blocks_kept"] == ref["blocks_kept"] == 3
        assert np.float32(got[0]["peak"]) == ref["peak"] and got[0]["gain"] == 1.0


def _raw(x, rate, params, b=1, stride=None, out_stride=None, n=None, out=True):
    y = np.zeros_like(x)
    res = (_ffi.LoudResult * max(b, 1))()
    ns = (C.c_int64 * max(b, 1))(*([len(x) if n is None else n] * max(b, 1)))
    rc = _ffi.lib().fs_loudness_normalize(0, x.ctypes.data_as(C.POINTER(C.c_float)), b, C.c_size_t(len(x) if stride is None else stride), ns, rate,
                                          C.byref(params) if params is not None else None, y.ctypes.data_as(C.POINTER(C.c_float)) if out else None,
                                          C.c_size_t(len(x) if out_stride is None else out_stride), res)
    return rc, _ffi.lib().fs_last_error().decode()


def test_every_validation_error_names_its_argument():
    x = R.signal("mix", 5000, 8000, 1)
    ok = _ffi.LoudParams(-18.0, -1.0, 30.0)
    assert _raw(x, 8000, ok)[0] == 0
    for rate in (7999, 48001, 0, -44100):
        rc, msg = _raw(x, rate, ok)
        assert rc != 0 and "rate" in msg and "8000 .. 48000" in msg, (rate, msg)
    for t, p, g, word in ((-40.5, -1, 30, "target_lufs"), (-4.0, -1, 30, "target_lufs"), (math.nan, -1, 30, "target_lufs"), (-18, 0.5, 30, "peak_db"),
                          (-18, -math.inf, 30, "peak_db"), (-18, -1, -1, "max_gain_db"), (-18, -1, 61, "max_gain_db")):
        rc, msg = _raw(x, 8000, _ffi.LoudParams(t, p, g))
        assert rc != 0 and "fs_loud_params" in msg and word in msg, (t, p, g, msg)
        with pytest.raises(RuntimeError, match=word):
            fishrt.loudness_normalize(x, 8000, t, peak_db=p, max_gain_db=g)
    rc, msg = _raw(x, 8000, None)
    assert rc != 0 and "params" in msg, msg
    assert _raw(x, 8000, None, out=False)[0] == 0  # measuring needs none
    rc, msg = _raw(x, 8000, ok, b=0)
    assert rc != 0 and "rows" in msg, msg
    rc, msg = _raw(x, 8000, ok, stride=4999)
    assert rc != 0 and "stride" in msg, msg
    rc, msg = _raw(x, 8000, ok, out_stride=4999)
    assert rc != 0 and "out_stride" in msg, msg
    rc, msg = _raw(x, 8000, ok, n=-1)
    assert rc != 0 and "length" in msg, msg
    with pytest.raises(ValueError):
        fishrt.loudness(np.zeros((2, 2, 2), np.float32), 8000)
    assert _raw(x, 8000, ok)[0] == 0
