"""Footprint re-verification on the GPU: fot_footprint_recheck against the reference's answers and the NumPy restatement on
identical inputs, at the shapes where the kernels can go wrong; its byte-identical invariances; its refusals; and the loop's
accumulators (fot_loop_footprint_enable / fot_loop_footprint_obs) against the recheck of the loop's own history, bit for bit.

Tolerances (tests/footprint_obs_common.py, derived there, none taken from what the library gives): distances within
64 * 2^-52 * max(1, M), M the largest coordinate magnitude of the case; headings within 8 * 2^-52 * pi; counts equal.  The
chain to the reference: (1) the library equals the reference's functions on identical inputs within that bound; (2) the
loop's accumulators equal the library's recheck of the loop's own history bit for bit; (3) the loop's history against the
reference's runs is held by the existing episode tests."""
import ctypes as C

import numpy as np
import pytest

import footprint_obs_common as fc
from closed_loop_common import load_episodes, scenario_config
from integrated_path_planning_amd import _abi, safety, synthetic as syn
from integrated_path_planning_amd.closed_loop import BatchedClosedLoop
from integrated_path_planning_amd.planner import BatchPlanner

pytestmark = pytest.mark.gpu
SENTINEL = 0x5A
RECHECK_FROM_RECORD = ("legacy_min_dist", "legacy_collision_steps", "multi_min_dist", "multi_clearance", "multi_violation_steps",
                       "rect_min_surface_dist", "rect_clearance", "rect_violation_steps")
OBS_FROM_RECORD = ("legacy_min_dist", "multi_clearance", "multi_violation_steps", "rect_clearance", "rect_violation_steps")


@pytest.fixture(scope="module")
def fix():
    return fc.load_cases()


@pytest.fixture(scope="module")
def engine():
    with BatchPlanner(waypoints=(syn.STRAIGHT_WX, syn.STRAIGHT_WY), device=0, **syn.CONFIG3_PLANNER) as bp:
        yield bp


def geom_of(geom=None):
    return safety.footprint_geometry(geom)


def call(engine, case, geom=None, reconstruct=False, null=(), n_traj=None, raw_geom=None):
    """fot_footprint_recheck through ctypes with every output pre-filled: (rc, records, series, yaw_out, untouched)."""
    g = raw_geom if raw_geom is not None else geom_of(geom)
    step_off = np.ascontiguousarray(case["step_off"], np.int32)
    ped_off = np.ascontiguousarray(case["ped_off"], np.int32)
    xy, yaw = np.ascontiguousarray(case["xy"], np.float64), np.ascontiguousarray(case["yaw"], np.float64)
    ped = np.ascontiguousarray(case["ped_xy"], np.float64)
    n = len(step_off) - 1 if n_traj is None else n_traj
    steps = len(xy)
    rec = np.frombuffer(bytearray([SENTINEL]) * (64 * max(n, 1)), fc.RECORD_DT).copy()
    series = np.frombuffer(bytearray([SENTINEL]) * (24 * max(steps, 1)), fc.STEP_DT).copy()
    used = np.frombuffer(bytearray([SENTINEL]) * (8 * max(steps, 1)), np.float64).copy()
    ptr = lambda a, name: None if name in null else a.ctypes.data
    rc = _abi.lib().fot_footprint_recheck(
        engine._h, None if "geom" in null else C.byref(g), n, ptr(step_off, "step_off"), ptr(xy, "xy"),
        None if reconstruct else ptr(yaw, "yaw"), ptr(ped_off, "ped_off"), ptr(ped, "ped_xy") if ped.size else None,
        ptr(series, "series"), ptr(used, "yaw_out"), ptr(rec, "out"))
    untouched = all(np.all(a.view(np.uint8) == SENTINEL) for a in (rec, series, used))
    return rc, rec[:max(n, 0)], series[:steps], used[:steps], untouched


def good(engine, case, geom=None, reconstruct=False):
    rc, rec, series, used, _ = call(engine, case, geom, reconstruct)
    assert rc == _abi.OK, _abi.lib().fot_last_error(engine._h)
    return rec, series, used


def case_of(fix, name):
    return fc.golden_case(fix, fix["meta"]["cases"][name]["inputs"])


def rows_of(records, keys):
    return np.array([[float(r[k]) for k in keys] for r in records]).reshape(len(records), len(keys))


# ---- against the reference and the restatement --------------------------------------------------------------------------------
def test_library_matches_the_reference_on_the_fixture(fix, engine):
    """Every stored case -- synthetic scenes at 1, 3, 4, 5 and 8 circles, the reference's ego histories of base, rnd3, walls
    and turn, the threshold cases -- with the stored heading and with the reconstructed one."""
    worst_d, worst_y = 0.0, 0.0
    for name, info in fix["meta"]["cases"].items():
        case, tol = case_of(fix, name), fc.dist_tol(info["M"])
        rec, series, used = good(engine, case, info["geom"])
        assert used.tobytes() == case["yaw"].tobytes()
        got = np.stack([series["legacy"], series["multi"], series["rect"]], axis=1)
        worst_d = max(worst_d, fc.assert_close(got, fix[name + "_series"], tol, f"{name}: per-step values"))
        want = fix[name + "_recheck_stored"]
        rows = rows_of(rec, RECHECK_FROM_RECORD)
        for j, k in enumerate(RECHECK_FROM_RECORD):
            if k.endswith("_steps"):
                assert np.array_equal(rows[:, j], want[:, j]), f"{name} {k}: {rows[:, j]} != {want[:, j]}"
            else:
                worst_d = max(worst_d, fc.assert_close(rows[:, j], want[:, j], tol, f"{name} {k}"))
        obs, want = rows_of(rec, OBS_FROM_RECORD), fix[name + "_obs"]
        for j, k in enumerate(OBS_FROM_RECORD):
            if k.endswith("_steps"):
                assert np.array_equal(obs[:, j], want[:, j]), f"{name} {k}"
            else:
                fc.assert_close(obs[:, j], want[:, j], tol, f"{name} observational {k}")
        assert np.array_equal(rec["steps"], np.diff(case["step_off"]))
        assert np.array_equal(rec["steps_with_peds"], [int(np.sum(np.diff(case["ped_off"][lo:hi + 1]) > 0))
                                                       for lo, hi in zip(case["step_off"][:-1], case["step_off"][1:])])
        if np.all(np.diff(case["step_off"]) >= 2):
            rec, series, used = good(engine, case, info["geom"], reconstruct=True)
            worst_y = max(worst_y, fc.assert_close(used, fix[name + "_yaw_recon"], fc.YAW_TOL, f"{name}: heading"))
            want, rows = fix[name + "_recheck_recon"], rows_of(rec, RECHECK_FROM_RECORD)
            for j, k in enumerate(RECHECK_FROM_RECORD):
                if k.endswith("_steps"):
                    assert np.array_equal(rows[:, j], want[:, j]), f"{name} reconstructed {k}"
                else:
                    worst_d = max(worst_d, fc.assert_close(rows[:, j], want[:, j], tol, f"{name} reconstructed {k}"))
    print(f"largest distance difference {worst_d:.3e}, largest heading difference {worst_y:.3e}")


@pytest.mark.parametrize("geometry", ("legacy", "multi", "rect"))
def test_both_sides_of_every_strict_comparison(fix, engine, geometry):
    """Pose at the origin, yaw = 0: every operation is exact on both sides -- the reference's bytes, and 0, 1, 0 steps for
    a value at the threshold, one ulp below it and one ulp above it."""
    col = {"legacy": "legacy_collision_steps", "multi": "multi_violation_steps", "rect": "rect_violation_steps"}[geometry]
    counts = []
    for side in ("at", "below", "above"):
        name = f"thr_{geometry}_{side}"
        rec, series, _ = good(engine, case_of(fix, name), fix["meta"]["cases"][name]["geom"])
        got = np.stack([series["legacy"], series["multi"], series["rect"]], axis=1)
        assert got.tobytes() == fix[name + "_series"].tobytes()
        assert rows_of(rec, RECHECK_FROM_RECORD).tobytes() == fix[name + "_recheck_stored"].tobytes()
        counts.append(int(rec[0][col]))
    assert counts == [0, 1, 0]


def test_the_moving_comparison_at_its_threshold(fix, engine):
    got = []
    for side in ("at", "below", "above"):
        name = f"moving_{side}"
        _, _, used = good(engine, case_of(fix, name), reconstruct=True)
        fc.assert_close(used, fix[name + "_yaw_recon"], fc.YAW_TOL, name)
        got.append(float(used[1]))
    assert got[2] == 0.0 and abs(got[0] - np.pi / 2) <= fc.YAW_TOL and abs(got[1] - np.pi / 2) <= fc.YAW_TOL


# ---- pedestrians and circles ----------------------------------------------------------------------------------------------
def crowd_case(rng):
    """One trajectory whose steps meet 0, 1, 63, 64, 65 and 257 pedestrians scattered 20 .. 60 m away, then 257 with ONE
    row close to the vehicle: the first row, the last, row 63 and row 64, each once near the rear end (the first circle)
    and once near the front (the last circle).  Returns the case and, per designed step, (row, end)."""
    counts = [0, 1, 63, 64, 65, 257] + [257] * 8
    x, y, heading = fc.drive(rng, len(counts), start=(30.0, -20.0))
    peds, designed = [], {}
    for i, c in enumerate(counts):
        ang, far = rng.uniform(-np.pi, np.pi, c), rng.uniform(20.0, 60.0, c)
        peds.append(np.stack([x[i] + far * np.cos(ang), y[i] + far * np.sin(ang)], axis=1))
    for j, (row, end) in enumerate([(r, e) for r in (0, 256, 63, 64) for e in (-1.0, 1.0)]):
        i = 6 + j
        along, side = end * 3.1, 0.4                                 # beyond the rectangle's end, off its axis
        peds[i][row] = (x[i] + along * np.cos(heading[i]) - side * np.sin(heading[i]),
                        y[i] + along * np.sin(heading[i]) + side * np.cos(heading[i]))
        designed[i] = (row, end)
    return fc.make_case([(x, y, heading, peds)]), designed


@pytest.mark.parametrize("n_circles", (1, 3, 5, 8))
def test_pedestrian_counts_and_circles_around_the_waves_width(engine, n_circles):
    """0, 1, 63, 64, 65 and 257 pedestrians; 8 x 257 pairs is more than one pass of the lane loop; the minimising pedestrian
    in the first row, the last, row 63 and row 64; the minimising circle the first and the last."""
    case, designed = crowd_case(np.random.default_rng(100 + n_circles))
    geom = {"n_circles": n_circles}
    want_rec, want_series, _ = fc.recheck(case, geom)
    # the construction does what it says: per designed step the restatement's minimiser is that row and that circle
    offsets, _ = fc.circle_cover(4.5, 2.0, n_circles)
    for i, (row, end) in designed.items():
        p = case["ped_xy"][case["ped_off"][i]:case["ped_off"][i + 1]]
        centres = case["xy"][i] + offsets[:, None] * np.array([np.cos(case["yaw"][i]), np.sin(case["yaw"][i])])
        d = np.linalg.norm(p[None] - centres[:, None], axis=2)
        k, r = np.unravel_index(np.argmin(d), d.shape)
        assert r == row and k == (0 if end < 0 else n_circles - 1)
        assert int(np.argmin(np.linalg.norm(p - case["xy"][i], axis=1))) == row
    rec, series, _ = good(engine, case, geom)
    tol = fc.dist_tol(fc.magnitude(case["xy"], case["ped_xy"]))
    fc.assert_series_close(series, want_series, tol, f"{n_circles} circles")
    fc.assert_records_close(rec, want_rec, tol, f"{n_circles} circles")
    assert np.isinf(series["legacy"][0]) and np.isinf(series["multi"][0]) and np.isinf(series["rect"][0])
    assert int(rec[0]["steps_with_peds"]) == len(series) - 1


# ---- steps and standstill --------------------------------------------------------------------------------------------------
def test_heading_reconstruction_across_chunks_standstills_and_lead_ins(engine):
    """2, 3, 255, 256, 257 and 600 steps; a standstill of steps 250 .. 262 across the chunk boundary; lead-ins of 1 and of
    300 steps; a trajectory that never moves; the reconstruction's yaw_out fed back as the stored yaw gives the same bytes."""
    case = fc.scan_case()
    rng = np.random.default_rng(12)
    counts = rng.integers(0, 4, len(case["xy"]))
    peds = fc.crowd_near(rng, case["xy"][:, 0], case["xy"][:, 1], counts)
    case = fc.make_case([(case["xy"][lo:hi, 0], case["xy"][lo:hi, 1], case["yaw"][lo:hi], peds[lo:hi])
                         for lo, hi in zip(case["step_off"][:-1], case["step_off"][1:])])
    assert sorted(set(np.diff(case["step_off"]).tolist())) == [2, 3, 40, 255, 256, 257, 600]
    want_rec, want_series, want_yaw = fc.recheck(case, reconstruct=True)
    rec, series, used = good(engine, case, reconstruct=True)
    fc.assert_close(used, want_yaw, fc.YAW_TOL, "heading")
    off = case["step_off"]
    moving = np.concatenate([fc.heading_terms(case["xy"][lo:hi, 0], case["xy"][lo:hi, 1])[2] for lo, hi in zip(off[:-1], off[1:])])
    assert not moving[250:263].any() and moving[249] and moving[263] and np.all(used[250:263] == used[249])
    assert int(np.argmax(moving[off[1]:off[2]])) == 1 and used[off[1]] == used[off[1] + 1]
    assert int(np.argmax(moving[off[2]:off[3]])) == 300 and np.all(used[off[2]:off[2] + 300] == used[off[2] + 300])
    assert not moving[off[3]:off[4]].any() and not used[off[3]:off[4]].any()
    # every held step carries the bytes of the moving step it holds
    for lo, hi in zip(off[:-1], off[1:]):
        m = moving[lo:hi]
        if m.any():
            src = np.maximum.accumulate(np.where(m, np.arange(hi - lo), -1))
            src = np.where(src >= 0, src, int(np.argmax(m)))
            assert used[lo:hi].tobytes() == used[lo:hi][src].tobytes()
    # the records on the library's own heading: the restatement fed with it, and the stored-yaw call fed with it
    tol = fc.dist_tol(fc.magnitude(case["xy"], case["ped_xy"]))
    own = fc.recheck(dict(case, yaw=used))
    fc.assert_series_close(series, own[1], tol, "series on the library's heading")
    fc.assert_records_close(rec, own[0], tol, "records on the library's heading")
    rec2, series2, used2 = good(engine, dict(case, yaw=used))
    assert rec2.tobytes() == rec.tobytes() and series2.tobytes() == series.tobytes() and used2.tobytes() == used.tobytes()


# ---- batching and series -----------------------------------------------------------------------------------------------------
def ragged_case(rng, n):
    steps = [2, 3, 70, 1, 9, 33, 5, 12, 300, 4, 7, 64, 65, 6, 8, 10, 11][:n]
    trajs = []
    for s in steps:
        x, y, heading = fc.drive(rng, s, start=tuple(rng.uniform(-50, 50, 2)), stand=((1, 2),) if s > 8 else ())
        trajs.append((x, y, heading, fc.crowd_near(rng, x, y, rng.integers(0, 40, s), spread=4.0)))
    return fc.make_case(trajs)


@pytest.mark.parametrize("reconstruct", (False, True))
def test_a_trajectory_does_not_depend_on_its_company(engine, reconstruct):
    """1, 2 and 17 ragged trajectories in one call: a trajectory's record and series are byte-identical alone and in company,
    first and last in the call; the series folded on the host is the record."""
    case = ragged_case(np.random.default_rng(21), 17)
    if reconstruct:                                                  # (the one-step trajectory needs its yaw)
        case = fc.sub_case(case, [t for t in range(17) if case["step_off"][t + 1] - case["step_off"][t] >= 2])
    n = len(case["step_off"]) - 1
    rec, series, used = good(engine, case, reconstruct=reconstruct)
    assert fc.fold_series(case, series).tobytes() == rec.tobytes()
    assert np.sum(rec["multi_violation_steps"]) > 0 and np.sum(rec["rect_violation_steps"]) > 0
    for ts in ([0], [n - 1], [8], [n - 1, 0], [8, 3], [5, n - 1]):
        sub = fc.sub_case(case, ts)
        r, s, u = good(engine, sub, reconstruct=reconstruct)
        at = 0
        for j, t in enumerate(ts):
            lo, hi = case["step_off"][t], case["step_off"][t + 1]
            assert r[j].tobytes() == rec[t].tobytes(), (ts, t)
            assert s[at:at + hi - lo].tobytes() == series[lo:hi].tobytes() and u[at:at + hi - lo].tobytes() == used[lo:hi].tobytes()
            at += hi - lo


def test_a_call_past_the_pinned_block_gives_the_same_bytes(engine):
    """More than 1 MiB of inputs goes through device copies instead of the pinned block: a trajectory's bytes are the same
    on both paths."""
    rng = np.random.default_rng(22)
    small = ragged_case(rng, 5)
    x, y, heading = fc.drive(rng, 300)
    big = fc.make_case([(x, y, heading, fc.crowd_near(rng, x, y, [300] * 300, spread=30.0))])
    assert big["ped_xy"].nbytes > (1 << 20) > small["ped_xy"].nbytes + small["xy"].nbytes * 2
    both = fc.make_case([t for c in (small, big, small) for t in
                         [(c["xy"][lo:hi, 0], c["xy"][lo:hi, 1], c["yaw"][lo:hi],
                           [c["ped_xy"][c["ped_off"][i]:c["ped_off"][i + 1]] for i in range(lo, hi)])
                          for lo, hi in zip(c["step_off"][:-1], c["step_off"][1:])]])
    for reconstruct in (False, True):
        if reconstruct:
            keep = [t for t in range(5) if small["step_off"][t + 1] - small["step_off"][t] >= 2]
            s_case = fc.sub_case(small, keep)
            b_case = fc.sub_case(both, keep + [5] + [6 + t for t in keep])
        else:
            s_case, b_case = small, both
        r_s, ser_s, _ = good(engine, s_case, reconstruct=reconstruct)
        r_b, ser_b, _ = good(engine, b_case, reconstruct=reconstruct)
        k = len(r_s)
        assert r_b[:k].tobytes() == r_s.tobytes() == r_b[k + 1:].tobytes()
        assert ser_b[:len(ser_s)].tobytes() == ser_s.tobytes() == ser_b[len(ser_s) + 300:].tobytes()
        want = fc.recheck(fc.sub_case(b_case, [k]), reconstruct=reconstruct)
        if not reconstruct:
            fc.assert_records_close(r_b[k:k + 1], want[0], fc.dist_tol(fc.magnitude(big["xy"], big["ped_xy"])), "the large trajectory")


# ---- refusals ------------------------------------------------------------------------------------------------------------------
def test_refusals_change_nothing_and_a_good_call_follows(engine):
    rng = np.random.default_rng(23)
    case = ragged_case(rng, 4)                                       # steps 2, 3, 70, 1
    ref = good(engine, case)
    two = fc.sub_case(case, [0, 1, 2])
    ref_recon = good(engine, two, reconstruct=True)
    G = _abi.FootprintGeom
    bad_geoms = [G(0.0, 2.0, 0.2, 1.2, 3, 0), G(4.5, -2.0, 0.2, 1.2, 3, 0), G(4.5, 2.0, -0.2, 1.2, 3, 0), G(4.5, 2.0, 0.2, -1.2, 3, 0),
                 G(4.5, 2.0, 0.2, 1.2, 0, 0), G(4.5, 2.0, 0.2, 1.2, 9, 0), G(float("nan"), 2.0, 0.2, 1.2, 3, 0)]
    refusals = [dict(raw_geom=g) for g in bad_geoms]
    refusals += [dict(null=(name,)) for name in ("geom", "step_off", "xy", "ped_off", "ped_xy", "out")]
    refusals += [dict(n_traj=-1)]
    tables = [dict(step_off=[1, 2, 5, 75, 76]), dict(step_off=[0, 2, 5, 4, 76]), dict(step_off=[0, 2, 2, 75, 76]),
              dict(ped_off=np.concatenate([[1], case["ped_off"][1:]])), dict(ped_off=np.concatenate([case["ped_off"][:5], [0], case["ped_off"][6:]]))]
    for kw in refusals:
        rc, _, _, _, untouched = call(engine, case, **kw)
        assert rc == _abi.ERR_INVALID and untouched, kw
        assert good(engine, case)[0].tobytes() == ref[0].tobytes()
    for change in tables:
        rc, _, _, _, untouched = call(engine, dict(case, **{k: np.asarray(v, np.int32) for k, v in change.items()}))
        assert rc == _abi.ERR_INVALID and untouched, change
        got = good(engine, case)
        assert got[0].tobytes() == ref[0].tobytes() and got[1].tobytes() == ref[1].tobytes()
    # a trajectory of one step: served with its yaw, refused without it
    rc, _, _, _, untouched = call(engine, case, reconstruct=True)
    assert rc == _abi.ERR_INVALID and untouched and b"1 step" in _abi.lib().fot_last_error(engine._h)
    got = good(engine, two, reconstruct=True)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got, ref_recon))
    # no trajectory: nothing to do, nothing written
    empty = dict(step_off=np.zeros(1, np.int32), xy=np.zeros((0, 2)), yaw=np.zeros(0), ped_off=np.zeros(1, np.int32), ped_xy=np.zeros((0, 2)))
    rc, _, _, _, untouched = call(engine, empty, null=("xy",))
    assert rc == _abi.OK and untouched


# ---- the Python layer ------------------------------------------------------------------------------------------------------------
def test_footprint_recheck_returns_the_references_rows(fix, engine):
    case = case_of(fix, "synth")
    trajs = []
    for lo, hi in zip(case["step_off"][:-1], case["step_off"][1:]):
        trajs.append(dict(ego_x=case["xy"][lo:hi, 0], ego_y=case["xy"][lo:hi, 1], ego_yaw=case["yaw"][lo:hi],
                          ped_positions=[case["ped_xy"][case["ped_off"][i]:case["ped_off"][i + 1]] for i in range(lo, hi)]))
    cols, tol = fix["meta"]["recheck_cols"], fc.dist_tol(fix["meta"]["cases"]["synth"]["M"])
    for mode, key, source in (("stored", "synth_recheck_stored", "stored"), ("reconstruct", "synth_recheck_recon", "reconstructed")):
        rows = safety.footprint_recheck(engine, trajs, yaw=mode)
        assert [tuple(r) for r in rows] == [safety.RECHECK_KEYS] * len(trajs)
        for t, row in enumerate(rows):
            assert row["yaw_source"] == source and row["steps"] == len(trajs[t]["ego_x"])
            for j, k in enumerate(cols):
                if k.endswith("_steps"):
                    assert row[k] == int(fix[key][t, j])
                else:
                    fc.assert_close(row[k], fix[key][t, j], tol, f"{mode} {t} {k}")
    # a set with and without stored headings: every trajectory keeps the row it has in a call of its own kind
    mixed = [dict(t, ego_yaw=None) if i % 2 else t for i, t in enumerate(trajs)]
    rows = safety.footprint_recheck(engine, mixed)
    stored, recon = safety.footprint_recheck(engine, trajs), safety.footprint_recheck(engine, trajs, yaw="reconstruct")
    assert rows == [recon[i] if i % 2 else stored[i] for i in range(len(trajs))]


# ---- the loop ------------------------------------------------------------------------------------------------------------------
LOOP_NAMES = ("base", "rnd3", "walls", "footprint", "turn")


@pytest.fixture(scope="module")
def episodes():
    return load_episodes()


def build(episodes, names, **kw):
    return BatchedClosedLoop([scenario_config(episodes["meta"], n) for n in names], [episodes[n + "_ped_traj"] for n in names], **kw)


def step_outputs(sim):
    """Every per-step output of the loop, per episode, as bytes (the shape of test_gpu_loop_summary.py's _step_outputs)."""
    out = [[] for _ in sim.episodes]
    for s in sim._steps:
        for e in range(len(sim.episodes)):
            i = int(s["slot"][e])
            if i < 0:
                continue
            kn = int(s["keep"][i])
            out[e].append(b"".join([np.array(s["ego"][i]).tobytes(), np.array(s["jerk"][i]).tobytes(),
                                    np.array(s["state"][i]).tobytes(), np.array(s["stats"][i]).tobytes(),
                                    np.array(s["keep"][i]).tobytes(), np.array(s["has_path"][i]).tobytes(),
                                    np.array(s["after"][i]).tobytes()]
                                   + [np.array(s["paths"][f][i, :kn]).tobytes() for f in _abi.PATH_FIELDS]))
    return out


def history_case(sim):
    """The loop's own history as a recheck case: per episode the new ego state of every lock step it ran and that step's
    pedestrians (the recording row of the step's frame)."""
    trajs = []
    for e in range(len(sim.episodes)):
        x, y, yaw, peds = [], [], [], []
        for s in sim._steps:
            i = int(s["slot"][e])
            if i < 0:
                continue
            x.append(s["ego"][i][0]); y.append(s["ego"][i][1]); yaw.append(s["ego"][i][2])
            peds.append(np.array(s["pos"][int(s["off"][i]):int(s["off"][i + 1])]))
        trajs.append((x, y, yaw, peds))
    return fc.make_case(trajs)


@pytest.fixture(scope="module")
def loops(episodes, engine):
    """base, rnd3, walls, footprint and turn on ONE handle with the footprint metrics on: resident in two chunks with a read
    in between, resident in one piece, and through the one-call step; the same loop without the keyword."""
    out = {}
    with build(episodes, LOOP_NAMES, resident=True, footprint_obs=True) as sim:
        sim.run(60)
        out["mid"] = sim.engine.loop_footprint_obs(len(LOOP_NAMES)).copy()
        out["mid_case"] = history_case(sim)
        sim.run()
        out["chunks"] = sim.engine.loop_footprint_obs(len(LOOP_NAMES)).copy()
        out["metrics"] = sim.footprint_metrics()
        out["chunks_steps"] = step_outputs(sim)
        out["case"] = history_case(sim)
    with build(episodes, LOOP_NAMES, resident=True, footprint_obs={"n_circles": 3}) as sim:
        sim.run()
        out["whole"] = sim.engine.loop_footprint_obs(len(LOOP_NAMES)).copy()
    with build(episodes, LOOP_NAMES, resident=True) as sim:
        sim.run()
        out["plain_steps"] = step_outputs(sim)
        with pytest.raises(ValueError, match="footprint_obs"):
            sim.footprint_metrics()
        with pytest.raises(_abi.FotError):
            sim.engine.loop_footprint_obs(len(LOOP_NAMES))
    with build(episodes, LOOP_NAMES, footprint_obs=True) as sim:
        sim.run()
        out["stepwise"] = sim.engine.loop_footprint_obs(len(LOOP_NAMES)).copy()
        out["stepwise_case"] = history_case(sim)
    return out


def test_loop_accumulators_equal_the_recheck_of_the_loops_own_history(loops, engine):
    rec, series, _ = good(engine, loops["case"])
    assert loops["chunks"].tobytes() == rec.tobytes()
    assert np.sum(rec["steps_with_peds"]) > 0 and np.all(rec["steps"] == np.diff(loops["case"]["step_off"]))
    assert np.sum(rec["multi_violation_steps"]) + np.sum(rec["rect_violation_steps"]) > 0, "the episodes are idle"
    mid, _, _ = good(engine, loops["mid_case"])
    assert loops["mid"].tobytes() == mid.tobytes() and int(np.max(mid["steps"])) == 60
    for m, r in zip(loops["metrics"], rec):
        assert tuple(m) == safety.FOOTPRINT_METRIC_KEYS
        assert all(m[k] == r[k] for k in m)


def test_a_read_between_two_chunks_changes_nothing_and_the_stepwise_loop_gives_the_same_bytes(loops, engine):
    assert loops["chunks"].tobytes() == loops["whole"].tobytes()
    assert loops["stepwise_case"]["xy"].tobytes() == loops["case"]["xy"].tobytes()
    assert loops["stepwise"].tobytes() == loops["chunks"].tobytes()


def test_every_other_output_of_the_loop_is_unchanged_by_the_keyword(loops):
    assert loops["chunks_steps"] == loops["plain_steps"]


def test_a_slots_record_does_not_depend_on_its_company(episodes, loops):
    with build(episodes, ("rnd3", "turn"), resident=True, footprint_obs=True) as sim:
        sim.run()
        pair = sim.engine.loop_footprint_obs(2).copy()
    assert pair[0].tobytes() == loops["chunks"][1].tobytes() and pair[1].tobytes() == loops["chunks"][4].tobytes()


def test_enable_and_read_refusals(episodes, engine):
    lib = _abi.lib()
    rec = np.zeros(2, fc.RECORD_DT)
    g = geom_of()
    # no loop begun on this handle
    assert lib.fot_loop_footprint_enable(engine._h, C.byref(g)) == _abi.ERR_INVALID
    assert lib.fot_loop_footprint_obs(engine._h, 2, rec.ctypes.data) == _abi.ERR_INVALID
    with build(episodes, ("base", "turn"), resident=True, footprint_obs=True) as sim:
        h = sim.engine._h
        assert lib.fot_loop_footprint_obs(h, 3, rec.ctypes.data) == _abi.ERR_INVALID
        assert lib.fot_loop_footprint_obs(h, 2, None) == _abi.ERR_INVALID
        bad = _abi.FootprintGeom(4.5, 2.0, 0.2, 1.2, 9, 0)
        assert lib.fot_loop_footprint_enable(h, C.byref(bad)) == _abi.ERR_INVALID
        assert lib.fot_loop_footprint_enable(h, None) == _abi.OK              # off again ...
        assert lib.fot_loop_footprint_obs(h, 2, rec.ctypes.data) == _abi.ERR_INVALID
        assert lib.fot_loop_footprint_enable(h, C.byref(g)) == _abi.OK        # ... and on
        sim.run(3)
        assert lib.fot_loop_footprint_enable(h, C.byref(g)) == _abi.ERR_INVALID   # after the first step
        assert lib.fot_loop_footprint_enable(h, None) == _abi.ERR_INVALID
        assert lib.fot_loop_footprint_obs(h, 2, rec.ctypes.data) == _abi.OK and np.all(rec["steps"] == 3)
    cfg = scenario_config(episodes["meta"], "base")
    with pytest.raises(ValueError, match="footprint_obs"):
        BatchedClosedLoop(cfg, [episodes["base_ped_traj"]], fused=False, footprint_obs=True)


def test_save_summaries_appends_the_five_columns_only_with_the_keyword(episodes, tmp_path):
    import csv
    heads = {}
    for kw in (dict(), dict(footprint_obs=True)):
        with build(episodes, ("base", "rnd3"), resident=True, summaries=True, **kw) as sim:
            sim.run(40)
            with open(sim.save_summaries(str(tmp_path / ("on" if kw else "off")))) as fh:
                rows = list(csv.reader(fh))
            heads[bool(kw)] = rows
            if kw:
                fm = sim.footprint_metrics()
    off, on = heads[False], heads[True]
    assert on[0] == off[0] + list(safety.FOOTPRINT_METRIC_KEYS)
    for r_off, r_on, m in zip(off[1:], on[1:], fm):
        assert r_on[:len(r_off)] == r_off
        assert r_on[len(r_off):] == [str(m[k]) for k in safety.FOOTPRINT_METRIC_KEYS]
