"""k_resample / k_sample_dist behind fot_resample_predictions and fot_predict_cv, called through ctypes over the
product of what the entry points accept (a seeded pairwise selection: both dtypes in and out, both layouts, small /
staged / device calls, anchor, prepend, S, P, pred_len, staleness classes, parameter sets), against the NumPy
restatement of the reference (tests/prediction_common.py); the properties that hold exactly; and the refusals.

Tolerances (prediction_common.assert_matches_restatement): float64 output rtol = atol = 1e-12, float32 output the
float32 rounding of the restatement +- 1 ulp; float32 inputs are widened exactly and get no allowance.  The rows at the
edge of np.allclose sit 1e-3 (relative) from the bound; tests/test_resample_cpu.py holds restatement and kernel
arithmetic to the same classification of every row generated here."""
import ctypes as C
import itertools

import numpy as np
import pytest

import prediction_common as pc
from integrated_path_planning_amd import _abi, synthetic as syn
from integrated_path_planning_amd.planner import BatchPlanner

pytestmark = pytest.mark.gpu

SMALL_CALL_BYTES = 1 << 20
SENTINEL = -777.25                                  # exactly representable in float32
_dp = C.POINTER(C.c_double)


@pytest.fixture(scope="module")
def engine():
    return BatchPlanner(waypoints=(syn.STRAIGHT_WX, syn.STRAIGHT_WY), **syn.CONFIG3_PLANNER)


def _code(dt):
    return _abi.F32 if np.dtype(dt) == np.dtype(np.float32) else _abi.F64


def _pd(a):
    return None if a is None else a.ctypes.data_as(_dp)


def _torch_dtype(dt):
    import torch
    return torch.float32 if np.dtype(dt) == np.dtype(np.float32) else torch.float64


def _device_out(n, dt):
    """A device tensor of n values plus as many guard values behind them, all SENTINEL."""
    import torch
    buf = torch.full((2 * n,), SENTINEL, dtype=_torch_dtype(dt), device=torch.device("cuda", 0))
    # The fill runs on torch's default stream; the library is handed stream 0 = its OWN stream, which is non-blocking and
    # waits for no other.  Without this the fill can land AFTER the library's kernel and leave the tensor all SENTINEL.
    torch.cuda.synchronize()
    return buf


def _finish_device(buf, n):
    import torch
    torch.cuda.synchronize()
    host = buf.cpu().numpy()
    assert (host[n:] == SENTINEL).all(), "the kernel wrote behind its output tensor"
    return host[:n].copy()


def resample(engine, pred, anchor, current, staleness, sgan_dt, sim_dt, plan_horizon, out_dtype, tmajor=False,
             device=False, want_dist=False):
    """fot_resample_predictions on pred [S, L, P, 2]; returns (out in the layout asked for, sample_dist or None)."""
    import torch
    lib = _abi.lib()
    pred = np.ascontiguousarray(pred)
    S, L, P = pred.shape[:3]
    rp = _abi.ResampleParams(sgan_dt, sim_dt, plan_horizon)
    T = pc.n_dense(sgan_dt, sim_dt, plan_horizon, L) + (0 if current is None else 1)
    shape = (T, S, P, 2) if tmajor else (S, P, T, 2)
    n = int(np.prod(shape))
    anchor = None if anchor is None else np.ascontiguousarray(anchor, dtype=np.float64)
    current = None if current is None else np.ascontiguousarray(current, dtype=np.float64)
    dist = np.full(S, np.nan) if want_dist else None
    t_out = C.c_int32(-1)
    flags = (_abi.OUT_TMAJOR if tmajor else 0) | (_abi.OUT_DEVICE if device else 0)
    if device:
        pred_dev = torch.from_numpy(pred).to(torch.device("cuda", 0))
        buf = _device_out(n, out_dtype)
        stream = torch.cuda.current_stream(torch.device("cuda", 0)).cuda_stream
        rc = lib.fot_resample_predictions(engine._h, C.byref(rp), S, L, P, C.c_void_p(pred_dev.data_ptr()), _code(pred.dtype),
                                          _pd(anchor), _pd(current), float(staleness), C.c_void_p(buf.data_ptr()),
                                          _code(out_dtype), flags, C.byref(t_out), _pd(dist),
                                          C.c_void_p(stream) if stream else None)
        _abi.check(engine._h, rc)
        out = _finish_device(buf, n)
    else:
        out = np.full(n + 64, SENTINEL, dtype=out_dtype)
        rc = lib.fot_resample_predictions(engine._h, C.byref(rp), S, L, P, C.c_void_p(pred.ctypes.data), _code(pred.dtype),
                                          _pd(anchor), _pd(current), float(staleness), C.c_void_p(out.ctypes.data),
                                          _code(out_dtype), flags, C.byref(t_out), _pd(dist), None)
        _abi.check(engine._h, rc)
        assert (out[n:] == SENTINEL).all(), "the library wrote behind the caller's output"
        out = out[:n]
    assert t_out.value == T
    return out.reshape(shape), dist


def predict_cv(engine, last, prev, current, staleness, pred_len, sgan_dt, sim_dt, plan_horizon, out_dtype, tmajor=False,
               device=False):
    """fot_predict_cv on observations [P, 2] of their own dtype; returns out ([P, T, 2], or [T, 1, P, 2] time-major)."""
    lib = _abi.lib()
    last = np.ascontiguousarray(last)
    prev = None if prev is None else np.ascontiguousarray(prev)
    P = last.shape[0]
    rp = _abi.ResampleParams(sgan_dt, sim_dt, plan_horizon)
    T = pc.n_dense(sgan_dt, sim_dt, plan_horizon, pred_len) + (0 if current is None else 1)
    shape = (T, 1, P, 2) if tmajor else (P, T, 2)
    n = int(np.prod(shape))
    current = None if current is None else np.ascontiguousarray(current, dtype=np.float64)
    t_out = C.c_int32(-1)
    flags = (_abi.OUT_TMAJOR if tmajor else 0) | (_abi.OUT_DEVICE if device else 0)
    p_prev = None if prev is None else C.c_void_p(prev.ctypes.data)
    if device:
        import torch
        buf = _device_out(n, out_dtype)
        stream = torch.cuda.current_stream(torch.device("cuda", 0)).cuda_stream
        rc = lib.fot_predict_cv(engine._h, C.byref(rp), pred_len, P, C.c_void_p(last.ctypes.data), p_prev, _code(last.dtype),
                                _pd(current), float(staleness), C.c_void_p(buf.data_ptr()), _code(out_dtype), flags,
                                C.byref(t_out), C.c_void_p(stream) if stream else None)
        _abi.check(engine._h, rc)
        out = _finish_device(buf, n)
    else:
        out = np.full(n + 64, SENTINEL, dtype=out_dtype)
        rc = lib.fot_predict_cv(engine._h, C.byref(rp), pred_len, P, C.c_void_p(last.ctypes.data), p_prev, _code(last.dtype),
                                _pd(current), float(staleness), C.c_void_p(out.ctypes.data), _code(out_dtype), flags,
                                C.byref(t_out), None)
        _abi.check(engine._h, rc)
        assert (out[n:] == SENTINEL).all()
        out = out[:n]
    assert t_out.value == T
    return out.reshape(shape)


def _call_kind(c, b):
    """small / staged / device, by the library's own rule (fot_host_pred.cpp resample_common: a host call whose inputs and
    outputs each fit 1 MiB of pinned memory is a small call)."""
    if c["device"]:
        return "device"
    P, S, L = c["P"], c["S"], c["L"]
    T = pc.n_dense(b["sgan_dt"], b["sim_dt"], b["plan_horizon"], L) + (1 if c["current"] else 0)
    a256 = lambda x: (x + 255) // 256 * 256
    in_b = b["pred"].dtype.itemsize * 2 * P * S * L
    out_b = np.dtype(b["out_dtype"]).itemsize * 2 * S * P * T
    small = 3 * a256(16 * P) + a256(in_b) <= SMALL_CALL_BYTES and out_b + 8 * S <= SMALL_CALL_BYTES
    return "small" if small else "staged"


def _expected(b):
    want = pc.process_samples(b["pred"], b["anchor"], b["staleness"], sgan_dt=b["sgan_dt"], sim_dt=b["sim_dt"],
                              plan_horizon=b["plan_horizon"])
    if b["current"] is not None:
        S, P = want.shape[:2]
        # the prepended row is `current` converted to the output dtype: exact in either tolerance
        cur = b["current"].astype(b["out_dtype"]).astype(np.float64)
        want = np.concatenate([np.broadcast_to(cur[None, :, None, :], (S, P, 1, 2)), want], axis=2)
    return want


def test_pairwise_cases_against_the_restatement(engine):
    cases = pc.resample_cases()
    seen = {name: set() for name in pc.RESAMPLE_AXES}
    seen["call"] = set()
    for index, c in enumerate(cases):
        b = pc.build_resample_case(c, index)
        label = f"case {index} {c}"
        got, dist = resample(engine, b["pred"], b["anchor"], b["current"], b["staleness"], b["sgan_dt"], b["sim_dt"],
                             b["plan_horizon"], b["out_dtype"], tmajor=c["tmajor"], device=c["device"], want_dist=True)
        assert got.dtype == b["out_dtype"]
        ref_layout = np.transpose(got, (1, 2, 0, 3)) if c["tmajor"] else got
        want = _expected(b)
        if c["current"]:
            np.testing.assert_array_equal(ref_layout[:, :, 0, :], want[:, :, 0, :].astype(b["out_dtype"]), err_msg=label)
        pc.assert_matches_restatement(np.ascontiguousarray(ref_layout), want, label)
        # the distances to the sample mean, of the library's own tensor without the prepended row
        own = ref_layout[:, :, 1:] if c["current"] else ref_layout
        d_want = pc.sample_distances(own)
        np.testing.assert_allclose(dist, d_want, rtol=1e-10, atol=0.0, err_msg=label)
        if c["S"] != 2:                      # (two samples are equally far from their mean: no first minimum to ask for)
            assert pc.first_two_gap(d_want) > 1e-8, label
            assert int(np.argmin(dist)) == int(np.argmin(d_want)), label
        for name in pc.RESAMPLE_AXES:
            seen[name].add(c[name])
        seen["call"].add(_call_kind(c, b))
    for name, values in pc.RESAMPLE_AXES.items():
        assert seen[name] == set(values), name
    assert seen["call"] == {"small", "staged", "device"}


def test_staged_float64_call_and_subset_through_the_small_call_path(engine):
    """A host call too large for pinned memory (S = 20, L = 12, P = 3000 float64: 11.5 MB in) against the restatement, and
    pedestrian subsets of it through the small-call path: the same rows bit for bit."""
    rng = np.random.default_rng(77)
    S, L, P = 20, 12, 3000
    pred, anchor, _ = pc.sources_tensor(rng, S, L, P, True, np.float64, 0.4)
    current = rng.uniform(-100, 100, (P, 2))
    kw = dict(sgan_dt=0.4, sim_dt=0.1, plan_horizon=5.0)
    assert pred.nbytes > SMALL_CALL_BYTES
    big, _ = resample(engine, pred, anchor, current, 0.3, out_dtype=np.float64, **kw)
    b = dict(pred=pred, anchor=anchor, current=current, staleness=0.3, out_dtype=np.float64, **kw)
    pc.assert_matches_restatement(big, _expected(b), "staged")
    for sub in (np.arange(0, 40), np.arange(2960, 3000), rng.choice(P, 40, replace=False)):
        part = np.ascontiguousarray(pred[:, :, sub])
        assert part.nbytes + 3 * 1024 < SMALL_CALL_BYTES and S * len(sub) * 51 * 16 + 8 * S < SMALL_CALL_BYTES
        small, _ = resample(engine, part, anchor[sub], current[sub], 0.3, out_dtype=np.float64, **kw)
        np.testing.assert_array_equal(small, big[:, sub])


@pytest.mark.parametrize("in_dtype,out_dtype", list(itertools.product((np.float32, np.float64), repeat=2)))
def test_exact_properties(engine, in_dtype, out_dtype):
    """Time-major = permuted reference layout; device = host; S samples in one call = S single-sample calls; with
    `current`, row 0 is current in the output dtype and the rest is the call without it.  No tolerance."""
    rng = np.random.default_rng(5 + 2 * _code(in_dtype) + _code(out_dtype))
    for (S, L, P), with_anchor in zip(((20, 12, 65), (2, 3, 300), (64, 1, 63), (3, 32, 1)), (True, False, True, False)):
        pred, anchor, _ = pc.sources_tensor(rng, S, L, P, with_anchor, in_dtype, 0.4)
        current = rng.uniform(-100, 100, (P, 2))
        kw = dict(sgan_dt=0.4, sim_dt=0.1, plan_horizon=5.0, out_dtype=out_dtype)
        base, d_base = resample(engine, pred, anchor, None, 0.25, want_dist=True, **kw)
        for device in (False, True):
            for cur in (None, current):
                ref, d_ref = resample(engine, pred, anchor, cur, 0.25, device=device, want_dist=True, **kw)
                tm, d_tm = resample(engine, pred, anchor, cur, 0.25, tmajor=True, device=device, want_dist=True, **kw)
                np.testing.assert_array_equal(tm, np.transpose(ref, (2, 0, 1, 3)))
                np.testing.assert_array_equal(d_tm, d_ref)
                np.testing.assert_array_equal(d_ref, d_base)               # the prepended row is not part of the distance
                if cur is None:
                    np.testing.assert_array_equal(ref, base)               # device = host
                else:
                    np.testing.assert_array_equal(ref[:, :, 0, :],
                                                  np.broadcast_to(cur.astype(out_dtype)[None], (S, P, 2)))
                    np.testing.assert_array_equal(ref[:, :, 1:, :], base)
        for s in range(0, S, max(1, S // 4)):
            one, _ = resample(engine, pred[s:s + 1], anchor, None, 0.25, **kw)
            np.testing.assert_array_equal(one[0], base[s])


def test_time_major_device_output_stays_inside_its_tensor(engine):
    """A small time-major device call whose output tensor is followed by a guard of its own size: the tensor is the
    permuted reference layout and the guard is untouched (an offset computed with the wrong stride lands there)."""
    rng = np.random.default_rng(31)
    pred, anchor, _ = pc.sources_tensor(rng, 4, 12, 9, True, np.float32, 0.4)
    kw = dict(sgan_dt=0.4, sim_dt=0.1, plan_horizon=5.0, out_dtype=np.float32, device=True)
    ref, _ = resample(engine, pred, anchor, anchor + 0.5, 0.1, **kw)
    tm, _ = resample(engine, pred, anchor, anchor + 0.5, 0.1, tmajor=True, **kw)
    np.testing.assert_array_equal(tm, np.transpose(ref, (2, 0, 1, 3)))


def test_dense_length_at_the_limit(engine):
    """n_dense = 256 = FOT_MAX_NT without a prepended row, 255 + 1 with one: the longest rows the entry point takes."""
    rng = np.random.default_rng(8)
    for sim_dt, horizon, cur in ((0.02, 5.12, False), (0.02, 5.1, True)):
        pred, anchor, _ = pc.sources_tensor(rng, 2, 12, 70, True, np.float64, 0.4)
        current = rng.uniform(-100, 100, (70, 2)) if cur else None
        b = dict(pred=pred, anchor=anchor, current=current, staleness=0.04, sgan_dt=0.4, sim_dt=sim_dt,
                 plan_horizon=horizon, out_dtype=np.float64)
        assert pc.n_dense(0.4, sim_dt, horizon, 12) + (1 if cur else 0) == pc.MAX_NT
        for tmajor in (False, True):
            got, _ = resample(engine, pred, anchor, current, 0.04, 0.4, sim_dt, horizon, np.float64, tmajor=tmajor)
            got = np.transpose(got, (1, 2, 0, 3)) if tmajor else got
            pc.assert_matches_restatement(np.ascontiguousarray(got), _expected(b), f"sim_dt {sim_dt} tmajor {tmajor}")


def test_predict_cv_over_its_arguments(engine):
    """Both observation dtypes x obs_prev given / NULL x both output dtypes x both layouts x host / device x prepend,
    P cycling over the wave-stride edges and a staged size, against the restatement."""
    rng = np.random.default_rng(19)
    Ps = itertools.cycle((1, 63, 64, 65, 300, 3000))
    params = itertools.cycle(((12, 0.4, 0.1, 5.0, 0.2), (8, 0.4, 0.1, 3.0, 0.0), (12, 0.4, 0.02, 5.0, 0.04),
                              (1, 0.5, 0.25, 4.0, 0.75), (32, 0.3, 0.13, 6.5, 1.3)))
    n = 0
    for obs_dt, has_prev, out_dt, tmajor, device, with_cur in itertools.product(
            (np.float32, np.float64), (True, False), (np.float32, np.float64), (False, True), (False, True), (False, True)):
        P = next(Ps)
        L, sg, sd, h, stale = next(params)
        last = rng.uniform(-80, 80, (P, 2)).astype(obs_dt)
        prev = (last + rng.normal(0, 0.6, (P, 2))).astype(obs_dt) if has_prev else None
        current = rng.uniform(-100, 100, (P, 2)) if with_cur else None
        got = predict_cv(engine, last, prev, current, stale, L, sg, sd, h, out_dt, tmajor=tmajor, device=device)
        got = np.ascontiguousarray(np.transpose(got[:, 0], (1, 0, 2))) if tmajor else got
        want = pc.predict_cv(last, prev, stale, pred_len=L, sgan_dt=sg, sim_dt=sd, plan_horizon=h)
        if with_cur:
            np.testing.assert_array_equal(got[:, 0, :], current.astype(out_dt))
            want = np.concatenate([current.astype(out_dt).astype(np.float64)[:, None, :], want], axis=1)
        pc.assert_matches_restatement(got, want, f"cv obs {np.dtype(obs_dt)} prev {has_prev} out {np.dtype(out_dt)} "
                                                 f"tmajor {tmajor} device {device} current {with_cur} P {P} L {L}")
        n += 1
    assert n == 64


def test_predict_cv_exact_properties(engine):
    rng = np.random.default_rng(23)
    for obs_dt in (np.float32, np.float64):
        last = rng.uniform(-80, 80, (300, 2)).astype(obs_dt)
        prev = (last + rng.normal(0, 0.6, last.shape)).astype(obs_dt)
        current = rng.uniform(-100, 100, (300, 2))
        for out_dt in (np.float32, np.float64):
            kw = dict(pred_len=12, sgan_dt=0.4, sim_dt=0.1, plan_horizon=5.0, out_dtype=out_dt)
            base = predict_cv(engine, last, prev, None, 0.2, **kw)
            np.testing.assert_array_equal(predict_cv(engine, last, prev, None, 0.2, device=True, **kw), base)
            tm = predict_cv(engine, last, prev, None, 0.2, tmajor=True, **kw)
            np.testing.assert_array_equal(tm[:, 0], np.transpose(base, (1, 0, 2)))
            pre = predict_cv(engine, last, prev, current, 0.2, device=True, **kw)
            np.testing.assert_array_equal(pre[:, 0], current.astype(out_dt))
            np.testing.assert_array_equal(pre[:, 1:], base)
            np.testing.assert_array_equal(predict_cv(engine, last[40:90], prev[40:90], None, 0.2, **kw), base[40:90])


# ---- refusals ---------------------------------------------------------------------------------------------------------
def _raw_resample(engine, rp, S, L, P, pred, in_code, out, out_code, current=None, t_out=None):
    lib = _abi.lib()
    return lib.fot_resample_predictions(engine._h, C.byref(_abi.ResampleParams(*rp)), S, L, P,
                                        None if pred is None else C.c_void_p(pred.ctypes.data), in_code, None,
                                        _pd(current), 0.0, None if out is None else C.c_void_p(out.ctypes.data), out_code,
                                        0, None if t_out is None else C.byref(t_out), None, None)


def _raw_cv(engine, rp, L, P, last, out, obs_code=_abi.F64, out_code=_abi.F64, current=None, t_out=None):
    lib = _abi.lib()
    return lib.fot_predict_cv(engine._h, C.byref(_abi.ResampleParams(*rp)), L, P,
                              None if last is None else C.c_void_p(last.ctypes.data), None, obs_code, _pd(current), 0.0,
                              None if out is None else C.c_void_p(out.ctypes.data), out_code, 0,
                              None if t_out is None else C.byref(t_out), None)


def _good_call(engine):
    """A following good call on the same handle gives the right answer."""
    rng = np.random.default_rng(1)
    pred, anchor, _ = pc.sources_tensor(rng, 2, 12, 5, True, np.float64, 0.4)
    got, _ = resample(engine, pred, anchor, None, 0.1, 0.4, 0.1, 5.0, np.float64)
    pc.assert_matches_restatement(got, pc.process_samples(pred, anchor, 0.1), "after a refusal")
    last = rng.uniform(-5, 5, (5, 2))
    pc.assert_matches_restatement(predict_cv(engine, last, None, None, 0.1, 12, 0.4, 0.1, 5.0, np.float64),
                                  pc.predict_cv(last, None, 0.1), "cv after a refusal")


def test_refusals_leave_the_handle_usable(engine):
    ok = (0.4, 0.1, 5.0)
    nan = float("nan")
    pred = np.zeros((1, pc.MAX_PRED_LEN + 1, 3, 2))
    last = np.zeros((3, 2))
    cur = np.zeros((3, 2))
    out = np.full(2 * 3 * 2 * 700, SENTINEL)
    INV, UNS = _abi.ERR_INVALID, _abi.ERR_UNSUPPORTED
    # 0.02 s steps to 5.12 s: 256 dense rows fit, one prepended row more does not
    assert pc.n_dense(0.4, 0.02, 5.12, 12) == pc.MAX_NT
    checks = [
        ("pred_len 0", lambda: _raw_resample(engine, ok, 1, 0, 3, pred, _abi.F64, out, _abi.F64), INV),
        ("pred_len 33", lambda: _raw_resample(engine, ok, 1, pc.MAX_PRED_LEN + 1, 3, pred, _abi.F64, out, _abi.F64), UNS),
        ("dense + prepend > FOT_MAX_NT", lambda: _raw_resample(engine, (0.4, 0.02, 5.12), 1, 12, 3, pred, _abi.F64, out,
                                                              _abi.F64, current=cur), UNS),
        ("dense > FOT_MAX_NT", lambda: _raw_resample(engine, (0.4, 0.01, 5.0), 1, 12, 3, pred, _abi.F64, out, _abi.F64), UNS),
        ("sim_dt 0", lambda: _raw_resample(engine, (0.4, 0.0, 5.0), 1, 12, 3, pred, _abi.F64, out, _abi.F64), INV),
        ("sim_dt < 0", lambda: _raw_resample(engine, (0.4, -0.1, 5.0), 1, 12, 3, pred, _abi.F64, out, _abi.F64), INV),
        ("sgan_dt 0", lambda: _raw_resample(engine, (0.0, 0.1, 5.0), 1, 12, 3, pred, _abi.F64, out, _abi.F64), INV),
        ("sgan_dt < 0", lambda: _raw_resample(engine, (-0.4, 0.1, 5.0), 1, 12, 3, pred, _abi.F64, out, _abi.F64), INV),
        ("sim_dt NaN", lambda: _raw_resample(engine, (0.4, nan, 5.0), 1, 12, 3, pred, _abi.F64, out, _abi.F64), INV),
        ("sgan_dt NaN", lambda: _raw_resample(engine, (nan, 0.1, 5.0), 1, 12, 3, pred, _abi.F64, out, _abi.F64), INV),
        ("pred dtype", lambda: _raw_resample(engine, ok, 1, 12, 3, pred, 2, out, _abi.F64), INV),
        ("out dtype", lambda: _raw_resample(engine, ok, 1, 12, 3, pred, _abi.F64, out, -1), INV),
        ("pred NULL", lambda: _raw_resample(engine, ok, 1, 12, 3, None, _abi.F64, out, _abi.F64), INV),
        ("out NULL", lambda: _raw_resample(engine, ok, 1, 12, 3, pred, _abi.F64, None, _abi.F64), INV),
        ("S < 0", lambda: _raw_resample(engine, ok, -1, 12, 3, pred, _abi.F64, out, _abi.F64), INV),
        ("cv pred_len 0", lambda: _raw_cv(engine, ok, 0, 3, last, out), INV),
        ("cv pred_len 33", lambda: _raw_cv(engine, ok, pc.MAX_PRED_LEN + 1, 3, last, out), UNS),
        ("cv dense + prepend", lambda: _raw_cv(engine, (0.4, 0.02, 5.12), 12, 3, last, out, current=cur), UNS),
        ("cv sim_dt 0", lambda: _raw_cv(engine, (0.4, 0.0, 5.0), 12, 3, last, out), INV),
        ("cv sgan_dt NaN", lambda: _raw_cv(engine, (nan, 0.1, 5.0), 12, 3, last, out), INV),
        ("cv obs dtype", lambda: _raw_cv(engine, ok, 12, 3, last, out, obs_code=7), INV),
        ("cv out dtype", lambda: _raw_cv(engine, ok, 12, 3, last, out, out_code=7), INV),
        ("cv obs_last NULL", lambda: _raw_cv(engine, ok, 12, 3, None, out), INV),
        ("cv obs_last NULL f32", lambda: _raw_cv(engine, ok, 12, 3, None, out, obs_code=_abi.F32), INV),
        ("cv out NULL", lambda: _raw_cv(engine, ok, 12, 3, last, None), INV),
    ]
    lib = _abi.lib()
    for name, call, code in checks:
        assert call() == code, name
        assert (out == SENTINEL).all(), name
        assert lib.fot_last_error(engine._h), name
        _good_call(engine)
    assert lib.fot_resample_n_dense(C.byref(_abi.ResampleParams(0.4, 0.0, 5.0)), 12) == INV
    assert lib.fot_resample_n_dense(C.byref(_abi.ResampleParams(0.4, 0.1, 5.0)), 0) == INV


def test_empty_calls_set_the_length_and_write_nothing(engine):
    pred = np.zeros((1, 12, 3, 2))
    out = np.full(4096, SENTINEL)
    for S, P in ((0, 3), (1, 0), (0, 0)):
        t_out = C.c_int32(-1)
        assert _raw_resample(engine, (0.4, 0.1, 5.0), S, 12, P, pred, _abi.F64, out, _abi.F64, t_out=t_out) == _abi.OK
        assert t_out.value == 50
        t_out = C.c_int32(-1)
        assert _raw_resample(engine, (0.4, 0.1, 5.0), S, 12, P, pred, _abi.F64, out, _abi.F64, current=np.zeros((3, 2)),
                             t_out=t_out) == _abi.OK
        assert t_out.value == 51
        assert (out == SENTINEL).all()
    t_out = C.c_int32(-1)
    assert _raw_cv(engine, (0.4, 0.1, 3.0), 8, 0, np.zeros((1, 2)), out, t_out=t_out) == _abi.OK
    assert t_out.value == 32 and (out == SENTINEL).all()
    _good_call(engine)
