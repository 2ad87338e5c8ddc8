"""fot_encounters_extract and fidelity.extract_encounters on the GPU, against the NumPy restatement
(tests/encounters_common.py, itself pinned to the reference in tests/test_encounters_cpu.py) -- never against the library
itself.  Every value is held to the same bits: the kernels run csrc/fot_encounter.hpp, the compiler-independent IEEE
sequence the restatement spells in NumPy (contraction off, real divisions, exact joins).

Designed calls at the kernels' edges (column tiles of 64, the four step shares, the selection's stride of 64, spans at the
grid's ends, single missing frames, the threshold and one ulp above it, tied minima, order statistics on duplicates, the
floor's edge, the free-walking mask, the goal's thresholds); the invariances; the fixture's clips end to end; the carried
recorded side against fidelity_batch and inside fidelity_report; every refusal; a fuzz of 40 random clips."""
import ctypes as C
import os

import numpy as np
import pytest

import encounters_common as ec
from integrated_path_planning_amd import _abi, batch, fidelity, synthetic as syn
from integrated_path_planning_amd.planner import BatchPlanner

pytestmark = pytest.mark.gpu
MODES = (None, "median", "quantile", "freewalk")
EDGE = ec.edge_calls()
FUZZ = ec.fuzz_calls()


@pytest.fixture(scope="module")
def engine():
    with BatchPlanner(waypoints=(syn.STRAIGHT_WX, syn.STRAIGHT_WY), device=0, **syn.CONFIG3_PLANNER) as bp:
        yield bp


@pytest.fixture(scope="module")
def fixture():
    return ec.load_fixture()


class OnDevice:
    """a float64 array in device memory, as far as batch.encounters_extract looks at a tensor: through the HIP runtime the
    library is bound to, so that no second framework has to start up for three copies"""

    def __init__(self, array, skew=0):
        _abi.lib()
        self.hip = None
        for name in (_abi.hip_soname(), "libamdhip64.so"):
            try:
                self.hip = C.CDLL(name, mode=getattr(os, "RTLD_NOLOAD", 4) | os.RTLD_NOW)
                break
            except OSError:
                pass
        assert self.hip is not None, "HIP runtime handle not reachable through ctypes"
        self.host = np.ascontiguousarray(array, dtype=np.float64)
        self.shape, self.ndim, self.dtype, self.skew = self.host.shape, self.host.ndim, "float64", skew
        self.base = C.c_void_p()
        assert self.hip.hipMalloc(C.byref(self.base), C.c_size_t(self.host.nbytes + 64)) == 0
        assert self.hip.hipMemcpy(C.c_void_p(self.data_ptr()), C.c_void_p(self.host.ctypes.data), C.c_size_t(self.host.nbytes), 1) == 0

    def data_ptr(self):
        return self.base.value + self.skew

    def is_contiguous(self):
        return True

    def back(self):
        out = np.empty_like(self.host)
        assert self.hip.hipMemcpy(C.c_void_p(out.ctypes.data), C.c_void_p(self.data_ptr()), C.c_size_t(out.nbytes), 2) == 0
        return out

    def free(self):
        assert self.hip.hipFree(self.base) == 0


def run(engine, case, ped_xy=None, ped_vel="same", **kw):
    return engine.encounters_extract(case["ped_xy"] if ped_xy is None else ped_xy, case["ped_vel"] if isinstance(ped_vel, str) else ped_vel,
                                     case["ego_xy"], case["ego_psi"], case["ego_vel"], case["dt"], want_series=True, **dict(case["kw"], **kw))


def expected(case, **kw):
    return ec.expected_call(case["ped_xy"], case["ped_vel"], case["ego_xy"], case["ego_psi"], case["ego_vel"], case["dt"],
                            **dict(case["kw"], **kw))


@pytest.mark.parametrize("case", EDGE, ids=[c["label"] for c in EDGE])
def test_designed_calls(engine, case):
    for mode in MODES:
        ec.assert_call_matches(run(engine, case, cruise=mode), expected(case, cruise=mode), f"{case['label']} {mode}")
    got = run(engine, case, measure_real=False)
    ec.assert_call_matches(got, expected(case, measure_real=False), case["label"])
    assert got["onset_dist"] is None and got["series"] is None


def test_designed_calls_cover_their_edges():
    by = {c["label"]: expected(c, cruise="median") for c in EDGE}
    for A in (1, 63, 64, 65, 256, 257):
        cols = by[f"A={A}"]["cols"]
        assert cols[0] == 0 and cols[-1] == A - 1 and (A < 63 or len(cols) < A)                   # first and last column present
    assert by["L=4"]["spans"]["status"].tolist() == [ec.SHORT] and by["L=5"]["spans"]["status"].tolist() == [ec.KEPT]
    two = by["first and last frame, two spans of one vehicle"]["spans"]
    assert two["vehicle"].tolist() == [0, 0, 1, 1] and two["frame0"][0] == 0 and two["frame1"][1] == 20
    assert by["absent in one frame"]["cols"].tolist() == [4, 5] and by["absent in one frame, fallback velocities"]["cols"].tolist() == [3, 4, 5]
    assert by["the last present frame has no fallback velocity"]["cols"].tolist() == [0, 2]
    at, above = by["min_separation == threshold"]["spans"][0], by["min_separation one ulp above the threshold"]["spans"][0]
    assert at["status"] == ec.KEPT and above["status"] == ec.FAR and at["min_separation"] == above["min_separation"] == 5.0
    assert (at["min_step"], at["min_col"]) == (3, 1)                                             # of (3, 1), (3, 2) and (4, 0)
    order = by["order statistics, q=0.5"]
    assert order["cruise"][2] == ec.FLOOR and order["cruise"][3] == np.nextafter(ec.FLOOR, 1.0) and order["cruise"][5] == ec.FLOOR
    assert order["goals"][4, 1] != 2.0 and order["goals"][5, 1] == 2.0                                              # below 1e-3: the first velocity's way
    free = expected(EDGE[-2], cruise="freewalk")["cruise"][0], expected(EDGE[-1], cruise="freewalk")["cruise"][0]
    speeds = np.abs(EDGE[-1]["ped_vel"][:, 0, 0])
    assert free[0] in speeds and free[1] == np.median(speeds)                                   # one free step; none: the median


def test_invariances(engine):
    rng = np.random.default_rng(77)
    T, A = 40, 70
    xy = ec.absent(rng, ec.walkers(rng, T, A, 0.4, box=8.0), 0.3, 0.3)
    three = ec.drive(T, [(0, 0, 18), (0, 21, 40), (1, 5, 30), (2, 2, 9), (2, 12, 38)], K=3)
    case3 = ec.call("K=3", xy, three, min_sep_threshold=6.0, cruise="freewalk", cruise_q=0.6)
    got3, want3 = run(engine, case3), expected(case3)
    ec.assert_call_matches(got3, want3, "K=3")
    assert np.sum(want3["spans"]["status"] == ec.KEPT) >= 3
    for k in range(3):                                             # a vehicle alone against the same vehicle among three
        alone = run(engine, dict(case3, ego_xy=three[0][k:k + 1], ego_psi=three[1][k:k + 1], ego_vel=three[2][k:k + 1]))
        mine = got3["spans"][got3["spans"]["vehicle"] == k]
        assert len(alone["spans"]) == len(mine)
        for a, b in zip(alone["spans"], mine):
            for f in ("min_separation", "real", "status", "frame0", "frame1", "n_ped", "min_step", "min_col"):
                assert a[f].tobytes() == b[f].tobytes(), (k, f)
            if a["status"] == ec.KEPT:
                ra, rb = (slice(int(s["row_base"]), int(s["row_base"]) + int(s["n_ped"])) for s in (a, b))
                for f in ("cols", "cruise", "goals", "onset_dist", "onset_step"):
                    assert alone[f][ra].tobytes() == got3[f][rb].tobytes(), (k, f)
    # the fallback's values handed in as recorded velocities; the scene in device memory
    vel = ec.velocities(xy, None, 0.4)
    d_xy, d_vel = OnDevice(xy), OnDevice(vel)
    for label, other in (("given velocities", run(engine, case3, ped_vel=vel)), ("device scene", run(engine, case3, ped_xy=d_xy, ped_vel=None)),
                         ("device scene and velocities", run(engine, case3, ped_xy=d_xy, ped_vel=d_vel))):
        assert other["spans"].tobytes() == got3["spans"].tobytes(), label
        for f in ("cols", "cruise", "goals", "onset_dist", "onset_step", "series"):
            assert other[f].tobytes() == got3[f].tobytes(), (label, f)
    assert d_xy.back().tobytes() == xy.tobytes() and d_vel.back().tobytes() == vel.tobytes()     # never written
    d_xy.free()
    d_vel.free()


def test_fixture_clips_end_to_end(engine, fixture):
    clips, meta = fixture
    records = [fidelity.RecordedClip(**clips[n][0]) for n in meta["clips"]]
    got = fidelity.extract_encounters(engine, records, cruise="median")
    assert [e.clip for e in got] == meta["multivehicle"]
    assert [e.clip for e in fidelity.extract_encounters(engine, records, multivehicle=False, measure_real=False)] == meta["single_vehicle_only"]
    flat = [(n, i) for n in meta["clips"] for i in range(len(meta["encounters"][n]))]
    for e, (name, i) in zip(got, flat):
        ref = clips[name][1]
        for f in ("times", "ego_xy", "ego_psi", "ego_vel", "ped_xy", "ped_vel", "ped_ids"):
            assert ec.same(getattr(e, f), ref[f"enc{i}_{f}"]), (name, i, f)
        assert e.min_separation == float(ref[f"enc{i}_min_separation"]) and e.dt == float(ref["ref_dt"]) and e.goals is None
        assert ec.same(e.cruise, ref[f"enc{i}_cruise_median"]) and ec.same(e.far_goals, ref[f"enc{i}_goals"]), (name, i)
    for mode, key, q in (("quantile", "cruise_q85", None), ("freewalk", "cruise_free", None), ("quantile", "cruise_q85", 0.85)):
        other = fidelity.extract_encounters(engine, records, cruise=mode, cruise_q=q, measure_real=False)
        for e, (name, i) in zip(other, flat):
            assert ec.same(e.cruise, clips[name][1][f"enc{i}_{key}"]) and e.real is None, (mode, name, i)
    assert fidelity.extract_encounters(engine, records)[0].cruise is None


def test_carried_recorded_side_equals_fidelity_batch(engine, fixture):
    clips, meta = fixture
    records = [fidelity.RecordedClip(**clips[n][0]) for n in meta["clips"]] + [fidelity.RecordedClip(**c) for c in ec.fuzz_clips(31, 6)]
    encs = fidelity.extract_encounters(engine, records)
    assert len(encs) >= 5
    again = fidelity.fidelity_batch(engine, encs)
    for e, rec, dist, step in zip(encs, again["records"], again["onset_dist"], again["onset_step"]):
        assert e.real["record"].tobytes() == rec.tobytes()
        assert e.real["onset_dist"].tobytes() == dist.tobytes() and e.real["onset_step"].tobytes() == step.tobytes()
        assert np.float64(e.real["record"]["closest"]).tobytes() == np.float64(e.min_separation).tobytes()


def test_report_with_and_without_the_carried_side(engine, fixture, monkeypatch):
    clips, meta = fixture
    records = [fidelity.RecordedClip(**clips[n][0]) for n in meta["clips"]] + [fidelity.RecordedClip(**c) for c in ec.fuzz_clips(31, 6)]
    encs = fidelity.extract_encounters(engine, records)
    bare = fidelity.extract_encounters(engine, records, measure_real=False)
    rng = np.random.default_rng(3)
    sims = [e.ped_xy + rng.normal(0.0, 0.15, e.ped_xy.shape) for e in encs]
    calls = []
    inner = engine.fidelity_eval
    monkeypatch.setattr(engine, "fidelity_eval", lambda *a, **k: (calls.append(1), inner(*a, **k))[1])
    with_real = fidelity.fidelity_report(engine, encs, sims)
    assert len(calls) == 1
    without = fidelity.fidelity_report(engine, bare, sims)
    assert len(calls) == 3
    assert list(with_real) == list(without) == list(fidelity.REPORT_KEYS)
    for k in with_real:
        assert np.array_equal(with_real[k], without[k], equal_nan=True), k
    assert with_real["n_encounters"] == len(encs) and with_real["n_onset_real"] == sum(int(e.real["record"]["n_onset"]) for e in encs)


def test_fuzz(engine):
    counts = ec.call_status_counts(FUZZ)
    assert counts[ec.KEPT] >= 0.1 * counts.sum() and np.all(counts > 0), counts      # (on the CPU: never empty ground)
    assert all(c["ped_xy"].shape[0] <= 120 and c["ped_xy"].shape[1] <= 70 and len(c["ego_xy"]) <= 4 for c in FUZZ)
    for case in FUZZ:
        ec.assert_call_matches(run(engine, case), expected(case), case["label"])


# ---- refusals: every output as it was ------------------------------------------------------------------------------------------
class Raw:
    """the C entry with outputs of the test's own, filled with a pattern"""

    def __init__(self, engine, case, max_spans=16, max_rows=4096, max_steps=4096):
        self.engine, self.case = engine, case
        self.cap = (max_spans, max_rows, max_steps)
        self.out = dict(spans=np.zeros(max_spans, batch.ENCOUNTER_SPAN_DT), cols=np.zeros(max_rows, np.int32), cruise=np.zeros(max_rows),
                        goals=np.zeros((max_rows, 2)), dist=np.zeros(max_rows), step=np.zeros(max_rows, np.int32), series=np.zeros(max_steps),
                        n_spans=np.zeros(1, np.int32), n_rows=np.zeros(1, np.int64))
        for a in self.out.values():
            a.view(np.uint8)[...] = 0xA5
        self.before = {k: a.tobytes() for k, a in self.out.items()}

    def __call__(self, null=(), sizes=None, scene=None, **kw):
        c, o = self.case, self.out
        p = dict(ec.PARAMS, **dict(c["kw"], **kw))
        mode = p["cruise"] if isinstance(p["cruise"], int) else _abi.ENC_CRUISE[p["cruise"]]
        flags = p.get("flags", _abi.ENC_MEASURE_REAL)
        prm = _abi.EncounterParams(p["min_sep_threshold"], p.get("dt", c["dt"]), p["accel_threshold"], p["max_distance"], p["cruise_q"],
                                   p["free_distance"], p["goal_distance"], p["min_len"], mode, flags, 0)
        K, T = c["ego_xy"].shape[:2]
        T, A, K = sizes or (T, c["ped_xy"].shape[1], K)
        args = dict(p=C.byref(prm), ped_xy=c["ped_xy"].ctypes.data if scene is None else scene, ped_vel=None, ego_xy=c["ego_xy"].ctypes.data,
                    ego_psi=c["ego_psi"].ctypes.data, ego_vel=c["ego_vel"].ctypes.data, n_spans=o["n_spans"].ctypes.data,
                    n_rows=o["n_rows"].ctypes.data, spans=o["spans"].ctypes.data, cols=o["cols"].ctypes.data, cruise=o["cruise"].ctypes.data,
                    goals=o["goals"].ctypes.data, dist=o["dist"].ctypes.data, step=o["step"].ctypes.data, series=o["series"].ctypes.data)
        for name in null:
            args[name] = None
        cap = kw.get("cap", self.cap)
        lib, h = self.engine._lib, self.engine._h
        rc = lib.fot_encounters_extract(h, args["p"], T, A, K, args["ped_xy"], args["ped_vel"], args["ego_xy"], args["ego_psi"], args["ego_vel"],
                                        cap[0], cap[1], args["n_spans"], args["n_rows"], args["spans"], args["cols"], args["cruise"],
                                        args["goals"], args["dist"], args["step"], args["series"], cap[2])
        msg = lib.fot_last_error(h)
        return rc, (msg.decode() if msg else "")

    def untouched(self):
        return all(a.tobytes() == self.before[k] for k, a in self.out.items())


def test_refusals_leave_the_outputs_untouched(engine):
    case = next(c for c in EDGE if c["label"] == "first and last frame, two spans of one vehicle")
    raw = Raw(engine, case)
    invalid = [dict(null=("p",)), dict(null=("n_spans",)), dict(null=("n_rows",)), dict(null=("spans",)), dict(null=("cols",)),
               dict(null=("ped_xy",)), dict(null=("ego_xy",)), dict(null=("ego_psi",)), dict(null=("ego_vel",)),
               dict(null=("cruise",), cruise="median"), dict(null=("goals",), cruise="freewalk"),
               dict(sizes=(-1, 11, 2)), dict(sizes=(20, -1, 2)), dict(sizes=(20, 11, -1)), dict(cap=(-1, 10, 10)), dict(cap=(10, -1, 10)),
               dict(dt=0.0), dict(dt=-0.4), dict(dt=np.inf), dict(dt=np.nan), dict(min_len=0),
               dict(min_sep_threshold=np.nan), dict(accel_threshold=np.nan), dict(max_distance=np.nan),
               dict(cruise="quantile", cruise_q=1.0001), dict(cruise="freewalk", cruise_q=-0.5), dict(cruise="quantile", cruise_q=np.nan),
               dict(cruise=4), dict(cruise=-1), dict(flags=4), dict(flags=_abi.ENC_MEASURE_REAL | 8)]
    for kw in invalid:
        rc, msg = raw(**kw)
        assert rc == _abi.ERR_INVALID and raw.untouched(), (kw, rc, msg)
        assert "fot_encounters_extract" in msg or "p" in kw.get("null", ()), (kw, msg)
    skewed = OnDevice(case["ped_xy"], skew=8)
    rc, msg = raw(scene=skewed.data_ptr(), flags=_abi.ENC_SCENE_DEVICE | _abi.ENC_MEASURE_REAL)
    assert rc == _abi.ERR_INVALID and "aligned" in msg and raw.untouched()
    skewed.free()
    # capacities: the need is named, nothing is written
    want = expected(case)
    n_spans, n_rows = len(want["spans"]), len(want["cols"])
    steps = int(np.sum((want["spans"]["frame1"] - want["spans"]["frame0"])[want["spans"]["status"] == ec.KEPT]))
    for cap, need in (((n_spans - 1, 4096, 4096), f"max_spans >= {n_spans}"), ((16, n_rows - 1, 4096), f"max_rows >= {n_rows}"),
                      ((16, 4096, steps - 1), f"max_steps >= {steps}")):
        rc, msg = raw(cap=cap)
        assert rc == _abi.ERR_UNSUPPORTED and need in msg and raw.untouched(), (cap, rc, msg)
    # exactly enough is enough; sizes of 0 succeed with zero spans
    rc, msg = Raw(engine, case, n_spans, n_rows, steps)()
    assert rc == 0, msg
    for sizes in ((0, 11, 2), (20, 0, 2), (20, 11, 0)):
        fresh = Raw(engine, case)
        rc, msg = fresh(sizes=sizes)
        assert rc == 0 and fresh.out["n_spans"][0] == 0 and fresh.out["n_rows"][0] == 0, (sizes, msg)
    with pytest.raises(ValueError):
        engine.encounters_extract(case["ped_xy"], None, case["ego_xy"], case["ego_psi"], case["ego_vel"], 0.4, cruise="mean")
    with pytest.raises(_abi.FotError):
        run(engine, case, max_rows=1)
    ec.assert_call_matches(run(engine, case), want, "after the refusals")
