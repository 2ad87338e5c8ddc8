"""fot_prediction_scores on the GPU: every unit class of the fixture in both layouts, both element types, host and device
tensors, skip 0 / 1, the padding around every block poisoned; batch independence byte for byte; determinism; refusals.

The kernel is held to the NumPy restatement on identical inputs at rtol = SUM_RTOL alone (pred_scores_common), a float32
tensor to the restatement fed the same rounded values, and float64 tensors to the reference's answers at the fixture's
tolerances."""
import numpy as np
import pytest

from integrated_path_planning_amd import _abi, synthetic as syn
from integrated_path_planning_amd.planner import BatchPlanner
from integrated_path_planning_amd.prediction import prediction_scores
from pred_scores_common import (assert_metrics_match_reference, assert_records_close, layouts, load_cases, origin_terms,
                                random_origin, unit_case, unit_metrics)
from test_pred_scores_cpu import UNITS

pytestmark = pytest.mark.gpu
PAD = 7                                                              # poisoned points around every block


@pytest.fixture(scope="module")
def fix():
    return load_cases()


@pytest.fixture(scope="module")
def engine():
    with BatchPlanner(waypoints=(syn.STRAIGHT_WX, syn.STRAIGHT_WY), device=0, **syn.CONFIG3_PLANNER) as bp:
        yield bp


def _packed(blocks, dtype):
    """The blocks one after the other in one flat tensor of points, NaN and 1e30 around each: (tensor, offsets)."""
    parts, offs, n = [], [], 0
    for i, b in enumerate(blocks):
        pad = np.full((PAD, 2), np.nan if i & 1 else 1e30, dtype)
        parts += [pad, np.ascontiguousarray(b, dtype).reshape(-1, 2)]
        offs.append(n + PAD)
        n += PAD + parts[-1].shape[0]
    parts.append(np.full((PAD, 2), np.nan, dtype))
    return np.concatenate(parts), offs


def _dims(blk, t_major):
    return (blk.shape[1], blk.shape[2], blk.shape[0]) if t_major else blk.shape[:3]


@pytest.fixture(scope="module")
def unit_want(fix):
    """The restatement of every unit origin, per element type -- computed once."""
    return {(name, np.dtype(dt).name): origin_terms(unit_case(fix, name)[0].astype(dt), unit_case(fix, name)[1],
                                                    unit_case(fix, name)[2])
            for name in UNITS for dt in (np.float64, np.float32)}


@pytest.mark.parametrize("on_device", [False, True])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("t_major", [False, True])
@pytest.mark.parametrize("skip", [0, 1])
def test_every_unit_class(fix, engine, unit_want, skip, t_major, dtype, on_device):
    """Origins of equal stride and E share a call; their blocks lie in one tensor with poisoned points between them."""
    groups = {}
    for name in UNITS:
        dense, truth, stride, _ = unit_case(fix, name)
        groups.setdefault((stride, truth.shape[1]), []).append(name)
    for (stride, E), names in groups.items():
        blocks = [layouts(unit_case(fix, n)[0], t_major, skip, dtype) for n in names]
        tensor, offs = _packed(blocks, dtype)
        origins = [(o,) + tuple(int(v) for v in _dims(b, t_major)) + (t_major, skip) for o, b in zip(offs, blocks)]
        truth = np.concatenate([unit_case(fix, n)[1] for n in names])
        if on_device:
            import torch
            tensor = torch.from_numpy(tensor).to(torch.device("cuda", 0))
        got = engine.prediction_scores(tensor, origins, truth, stride, E)
        for g, name in zip(got, names):
            label = f"{name} skip={skip} t_major={t_major} {np.dtype(dtype).name} device={on_device}"
            print(label, [float(g[k]) for k in ("ade_scene", "fde_scene", "ade_agent_sum", "fde_agent_sum", "log_lik_sum")])
            assert_records_close(g, unit_want[(name, np.dtype(dtype).name)], label)
            assert not (g["flags"] & _abi.PRED_NONFINITE), label
            if dtype == np.float64:
                assert_metrics_match_reference(unit_metrics(g), unit_case(fix, name)[3], fix["meta"]["nll_atol"], label)


def test_a_record_does_not_depend_on_the_batch(fix, engine):
    """Alone == inside a batch of mixed shapes == in reversed batch order, by bytes; two runs byte-identical."""
    rng = np.random.default_rng(5)
    stride, E = 2, 3
    shapes = [(1, 1), (2, 5), (7, 33), (64, 3), (20, 30), (3, 65), (5, 270), (2, 400), (4, 0), (6, 12)]
    origins = [random_origin(rng, S=S, P=max(P, 1), E=E, stride=stride) for S, P in shapes]
    dense = [d[:, :P] for (d, _, _), (_, P) in zip(origins, shapes)]
    truths = [t[:P] for (_, t, _), (_, P) in zip(origins, shapes)]
    both = prediction_scores(engine, dense, truths, stride)
    again = prediction_scores(engine, dense, truths, stride)
    assert both.tobytes() == again.tobytes()
    rev = prediction_scores(engine, dense[::-1], truths[::-1], stride)
    assert rev[::-1].tobytes() == both.tobytes()
    for i, (d, t) in enumerate(zip(dense, truths)):
        alone = prediction_scores(engine, d, t, stride)
        assert alone.tobytes() == both[i:i + 1].tobytes(), f"origin {i} {shapes[i]}"
        assert_records_close(alone[0], origin_terms(d, t, stride), f"origin {i} {shapes[i]}")
    assert both[8]["n_peds"] == 0 and both[8]["n_samples"] == 4 and both[8]["ade_scene"] == 0.0 and both[8]["flags"] == 0


def test_non_finite_inputs_are_flagged_and_propagate(engine):
    rng = np.random.default_rng(9)
    dense, truth, stride = random_origin(rng, S=5, P=4, E=2, stride=2)
    dense[3, 2, 3, 1] = np.nan                                        # an evaluated entry (k = stride * 2 - 1)
    got = prediction_scores(engine, dense, truth, stride)[0]
    want = origin_terms(dense, truth, stride)
    assert got["flags"] & _abi.PRED_NONFINITE and want["flags"] & _abi.PRED_NONFINITE
    assert_records_close(got, want, "NaN sample")
    assert np.isnan(got["ade_scene"]) and np.isnan(got["fde_agent_sum"])
    dense[3, 2, 3, 1] = 0.0
    dense[:, :, 0, :] = np.inf                                        # not an evaluation index: not read
    got = prediction_scores(engine, dense, truth, stride)[0]
    assert not (got["flags"] & _abi.PRED_NONFINITE)
    assert_records_close(got, origin_terms(np.where(np.isinf(dense), 0.0, dense), truth, stride), "unread inf")


def test_refusals_leave_the_output_untouched(engine):
    lib, h = engine._lib, engine._h
    rng = np.random.default_rng(3)
    dense, truth, stride = random_origin(rng, S=3, P=2, E=2, stride=2)
    T = dense.shape[2]
    tensor = np.ascontiguousarray(dense)
    big = np.zeros((65, 1, T, 2))
    out = np.full(2, 7.0, dtype=BatchPlanner.PRED_SCORE_DT)
    sentinel = out.tobytes()

    def call(S=3, P=2, T_=T, layout=0, skip=0, offset=0, stride_=stride, E=2, dtype=_abi.F64, data=tensor):
        d = np.zeros(1, dtype=BatchPlanner.PRED_ORIGIN_DT)
        d[0] = (offset, S, P, T_, layout, skip, 0)
        return lib.fot_prediction_scores(h, 1, d.ctypes.data, data.ctypes.data, dtype, 0, stride_, E, truth.ctypes.data,
                                         out.ctypes.data, None)

    INV, UNS = _abi.ERR_INVALID, _abi.ERR_UNSUPPORTED
    for kw, code in ((dict(T_=stride * 2 - 1), INV), (dict(T_=stride * 2, skip=1), INV), (dict(S=0), INV), (dict(E=0), INV),
                     (dict(stride_=0), INV), (dict(skip=2), INV), (dict(layout=3), INV), (dict(offset=-1), INV),
                     (dict(dtype=5), INV), (dict(P=-1), INV), (dict(S=65, P=1, data=big), UNS), (dict(E=33, T_=1000), UNS)):
        assert call(**kw) == code, kw
        assert lib.fot_last_error(h)
        assert out.tobytes() == sentinel, kw
    assert call() == _abi.OK and out.tobytes() != sentinel
    # the loop's entry point without a frame that carried a distribution
    rec = np.zeros(1, dtype=BatchPlanner.PRED_SCORE_DT)
    assert lib.fot_loop_prediction_scores(h, 1, stride, 2, truth.ctypes.data, rec.ctypes.data) == INV
    with pytest.raises(ValueError, match="past the tensor"):
        engine.prediction_scores(tensor, [(1, 3, 2, T, False, 0)], truth, stride, 2)
