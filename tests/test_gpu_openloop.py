"""Open-loop prediction evaluation on the GPU (fot_openloop_eval / evaluate_open_loop): constant velocity and the two
generators of tests/golden/openloop/cases.npz end to end against the reference's scene results; the library's records
against the NumPy restatement on the library's OWN raw samples; the shapes at which the gather, the chunks or the
generator's tiles can go wrong; the invariances a window's record keeps, byte for byte; and the refusals.

Tolerances (none taken from what the library gives):
* constant velocity: the existing tests hold fot_predict_cv to the reference within rtol = atol = 1e-12 per coordinate
  (tests/test_gpu_prediction.py); every displacement term is 1-Lipschitz in each point, so ADE / FDE are held to
  SUM_RTOL (the order of summation) plus sqrt(2) (1e-12 max |coordinate| + 1e-12);
* Social-GAN end to end: ADE / FDE (minima of means of point distances: 1-Lipschitz in the largest point distance) within
  the largest point distance ``dist`` between the library's raw samples and the reference's, which itself is held under
  ``sgan_common.accuracy_bound``; ``nll`` within the fixture's slope (largest |d log p / d q|) times ``dist``;
* records against the restatement on identical samples: SUM_RTOL alone (``pred_scores_common``)."""
import ctypes as C
import math

import numpy as np
import pytest

import openloop_common as oc
import sgan_common as sc
from integrated_path_planning_amd import _abi, synthetic as syn
from integrated_path_planning_amd.planner import BatchPlanner
from integrated_path_planning_amd.prediction import SganWeights, evaluate_open_loop, fixed_windows
from pred_scores_common import FLAG_NLL, assert_records_close
from summary_common import SUM_RTOL

pytestmark = pytest.mark.gpu
SENTINEL = 0x5A


@pytest.fixture(scope="module")
def fix():
    return oc.load_cases()


@pytest.fixture(scope="module")
def engine():
    with BatchPlanner(waypoints=(syn.STRAIGHT_WX, syn.STRAIGHT_WY), device=0, **syn.CONFIG3_PLANNER) as bp:
        yield bp


def table_of(fix):
    return fix["win_frame0"], fix["ped_off"], fix["row_col"]


def fixture_weights(method):
    a = oc.MODEL_ARGS[method]
    return SganWeights.from_state_dict(a, sc.seeded_state(a, oc.MODEL_SEED[method], oc.MODEL_SCALE))


def tiny_args(obs_len, pred_len, pooling, nd=2, mix="ped", every=True):
    return dict(obs_len=obs_len, pred_len=pred_len, embedding_dim=4, encoder_h_dim=6, decoder_h_dim=8, mlp_dim=8, bottleneck_dim=4,
                noise_dim=(nd,), num_layers=1, pooling_type=pooling, pool_every_timestep=every, noise_mix_type=mix,
                batch_norm=False, dropout=0.0, noise_type="gaussian")


def load(engine, slot, args, seed=7):
    w = SganWeights.from_state_dict(args, sc.seeded_state(args, seed, 2.0))
    _abi.check(engine._h, _abi.lib().fot_sgan_load_model(engine._h, slot, C.byref(w.desc), w.blob.size, w.blob.ctypes.data))
    return w


def call(engine, xy, table, obs_len, pred_len, method, S=1, model=0, noise=None, seed=3, kind=_abi.NOISE_GAUSSIAN, win_id0=0,
         max_rows=0, dt=0.4, device_scene=False, flags=None, dims=None, scene_dtype=None, want_raw=False):
    """fot_openloop_eval through ctypes with every output pre-filled: (rc, totals record | None, records, raw | None,
    untouched) -- ``untouched``: no output byte changed."""
    import torch
    f0, off, col = (np.ascontiguousarray(v, np.int32) for v in table)
    xy = np.ascontiguousarray(xy)
    code = _abi.F32 if xy.dtype == np.float32 else _abi.F64
    keep, fl = xy, 0
    ptr = xy.ctypes.data
    if device_scene:
        keep = torch.from_numpy(xy).to("cuda:0")
        torch.cuda.synchronize()
        ptr, fl = keep.data_ptr(), _abi.OPENLOOP_SCENE_DEVICE
    n_ptr = None
    if noise is not None and hasattr(noise, "data_ptr"):
        torch.cuda.synchronize()
        n_ptr, fl = noise.data_ptr(), fl | _abi.OPENLOOP_NOISE_DEVICE
    elif noise is not None:
        noise = np.ascontiguousarray(noise, np.float32)
        n_ptr = noise.ctypes.data
    n_frames, n_cols = dims if dims is not None else xy.shape[:2]
    W = len(f0)
    prm = _abi.OpenLoopParams(n_frames, n_cols, W, code if scene_dtype is None else scene_dtype, obs_len, pred_len, method, model, S,
                              kind, win_id0, max_rows, fl if flags is None else flags, 0, dt, seed)
    rec = np.zeros(max(W, 1), BatchPlanner.PRED_SCORE_DT)
    rec.view(np.uint8)[:] = SENTINEL
    tot = np.zeros(1, oc.TOTALS_DT)
    tot.view(np.uint8)[:] = SENTINEL
    rows = max(int(off[-1]), 0) if len(off) else 0
    raw = np.zeros((max(S, 1), max(pred_len, 1), rows, 2), np.float32) if want_raw else None
    if raw is not None:
        raw.view(np.uint8)[:] = SENTINEL
    rc = _abi.lib().fot_openloop_eval(engine._h, C.byref(prm), C.c_void_p(ptr) if xy.size else None, f0.ctypes.data if W else None,
                                      off.ctypes.data, col.ctypes.data if len(col) else None, C.c_void_p(n_ptr) if n_ptr else None,
                                      rec.ctypes.data, raw.ctypes.data if raw is not None and raw.size else None,
                                      C.cast(C.c_void_p(tot.ctypes.data), C.POINTER(_abi.OpenLoopTotals)), None)
    untouched = bool((rec.view(np.uint8) == SENTINEL).all() and (tot.view(np.uint8) == SENTINEL).all()
                     and (raw is None or (raw.view(np.uint8) == SENTINEL).all()))
    return rc, tot[0], rec[:W], raw, untouched


def ok(engine, *a, **kw):
    rc, tot, rec, raw, _ = call(engine, *a, **kw)
    assert rc == _abi.OK, _abi.lib().fot_last_error(engine._h)
    return tot, rec, raw


def edge_scene(rng, pops, obs_len, pred_len):
    """A scene without gaps, one window per entry of ``pops`` on ascending random columns, the last one ending on the last
    frame; float32-exact values (a float32 and a float64 scene then hold the same numbers)."""
    seq = obs_len + pred_len
    n_frames, n_ids = seq + max(len(pops), 1) - 1, max(max(pops, default=0), 1)
    xy = oc.random_scene(rng, n_frames, n_ids).astype(np.float32).astype(np.float64)
    f0 = np.arange(len(pops), dtype=np.int32)
    col = [np.sort(rng.choice(n_ids, P, replace=False)) for P in pops]
    off = np.concatenate([[0], np.cumsum(pops)]).astype(np.int32)
    return xy, (f0, off, np.concatenate(col + [np.zeros(0, np.int64)]).astype(np.int32))


def window_obs(xy, table, obs_len):
    """[obs_len, rows, 2] float32: the windows' observations side by side, as fot_sgan_sample takes them."""
    f0, off, col = table
    return np.concatenate([xy[f:f + obs_len][:, col[lo:hi]] for f, lo, hi in zip(f0, off[:-1], off[1:])]
                          + [np.zeros((obs_len, 0, 2))], axis=1).astype(np.float32)


def sgan_sample(engine, slot, pred_len, off, obs, noise):
    S = noise.shape[0]
    out = np.zeros((S, pred_len, obs.shape[1], 2), np.float32)
    off = np.ascontiguousarray(off, np.int32)
    _abi.check(engine._h, _abi.lib().fot_sgan_sample_model(engine._h, slot, len(off) - 1, off.ctypes.data, obs.ctypes.data, S,
                                                           noise.ctypes.data if noise.size else None, 0, out.ctypes.data, None))
    return out


# ---- against the reference ---------------------------------------------------------------------------------------------------
def test_constant_velocity_matches_the_reference(fix, engine):
    meta = fix["meta"]
    got = evaluate_open_loop(engine, fix["scene"], meta["obs_len"], meta["pred_len"], meta["dt"], "cv", records=True)
    atol = math.sqrt(2.0) * (1e-12 * float(np.nanmax(np.abs(fix["scene"]))) + 1e-12)
    oc.assert_result_close(got, meta["methods"]["cv"]["result"], SUM_RTOL, atol, 0.0, "cv")
    assert np.isnan(got["nll"]) and got["n_windows"] == 11
    for got_t, want_t in zip(got["windows"], table_of(fix)):
        assert np.array_equal(got_t, want_t)
    want = fix["cv_windows"]
    for w, r in enumerate(got["records"]):
        m = oc.window_metrics(r)
        for i, k in enumerate(oc.WINDOW_KEYS[:4]):
            oc.close(float(m[k]), float(want[w, i]), SUM_RTOL, atol, f"cv window {w} {k}")
        assert int(r["n_peds"]) == int(want[w, 4]) and int(r["nll_count"]) == 0 and int(r["n_samples"]) == 1


@pytest.mark.parametrize("method", ("lstm", "sgan"))
def test_social_gan_end_to_end_matches_the_reference(fix, engine, method):
    meta = fix["meta"]
    w = fixture_weights(method)
    got = evaluate_open_loop(engine, fix["scene"], meta["obs_len"], meta["pred_len"], meta["dt"], method, w, num_samples=meta["num_samples"],
                             noise=fix[method + "_noise"], model_slot=0 if method == "lstm" else 1, records=True, raw=True)
    raw32, raw64 = fix[method + "_raw32"], fix[method + "_raw64"]
    assert got["raw"].shape == raw32.shape
    dist = float(np.max(np.linalg.norm(got["raw"].astype(np.float64) - raw32.astype(np.float64), axis=-1)))
    bound = sc.accuracy_bound(raw32, raw64)
    print(f"{method}: largest point distance to the reference's raw samples {dist:.3e} m (bound {bound:.3e})")
    assert dist <= bound
    want = meta["methods"][method]["result"]
    print(f"{method}: got {got['ade']!r} {got['fde']!r} {got['ade_per_agent']!r} {got['fde_per_agent']!r} {got['nll']!r}; reference {want}")
    oc.assert_result_close(got, want, SUM_RTOL, dist, meta["nll_slope"] * dist, method)


@pytest.mark.parametrize("method", ("lstm", "sgan"))
def test_records_match_the_restatement_on_the_librarys_own_samples(fix, engine, method):
    """... and those samples are fot_sgan_sample's of the same windows and noise, bit for bit."""
    meta = fix["meta"]
    slot = 0 if method == "lstm" else 1
    w = fixture_weights(method)
    _abi.check(engine._h, _abi.lib().fot_sgan_load_model(engine._h, slot, C.byref(w.desc), w.blob.size, w.blob.ctypes.data))
    table, noise = table_of(fix), fix[method + "_noise"]
    tot, rec, raw = ok(engine, fix["scene"], table, meta["obs_len"], meta["pred_len"], _abi.OPENLOOP_SGAN, S=meta["num_samples"],
                       model=slot, noise=noise, want_raw=True)
    direct = sgan_sample(engine, slot, meta["pred_len"], table[1], window_obs(fix["scene"], table, meta["obs_len"]), noise)
    assert raw.tobytes() == direct.tobytes()
    want = oc.scene_records(fix["scene"], table, meta["obs_len"], meta["pred_len"], meta["dt"], raw)
    for i, (g, r) in enumerate(zip(rec, want)):
        assert_records_close(g, r, f"{method} window {i}")
    oc.assert_totals_close(tot, oc.fold_windows(want), SUM_RTOL, method)
    assert tot.tobytes() == oc.fold_windows(rec).tobytes()          # the fold: the reference's order on the records, exactly


# ---- shapes ----------------------------------------------------------------------------------------------------------------------
def test_populations_around_wave_tile_and_capacity_in_one_call(engine):
    """1, 2, 63, 64, 65 and 256 rows (k_openloop_rows' tile is 64 rows, the generator's capacity 256) and an empty window;
    chunks of the largest window, of one row less than everything, and everything; 257 rows are refused."""
    rng = np.random.default_rng(41)
    pops = [1, 2, 63, 64, 65, 0, 256]
    load(engine, 2, tiny_args(8, 12, "pool_net"))
    xy, table = edge_scene(rng, pops, 8, 12)
    tot, rec, raw = ok(engine, xy, table, 8, 12, _abi.OPENLOOP_SGAN, S=2, model=2, want_raw=True)
    want = oc.scene_records(xy, table, 8, 12, 0.4, raw)
    for i, (g, r) in enumerate(zip(rec, want)):
        assert_records_close(g, r, f"window {i} (P = {pops[i]})")
    assert [int(r["n_peds"]) for r in rec] == pops and int(tot["traj_count"]) == sum(pops) and int(tot["n_windows"]) == len(pops)
    for max_rows in (256, 450):                                     # (two chunks: 195 rows, then the 256-row window alone)
        t2, r2, raw2 = ok(engine, xy, table, 8, 12, _abi.OPENLOOP_SGAN, S=2, model=2, max_rows=max_rows, want_raw=True)
        assert r2.tobytes() == rec.tobytes() and t2.tobytes() == tot.tobytes() and raw2.tobytes() == raw.tobytes()
    cv_tot, cv_rec, _ = ok(engine, xy, table, 8, 12, _abi.OPENLOOP_CV)
    for i, (g, r) in enumerate(zip(cv_rec, oc.scene_records(xy, table, 8, 12, 0.4))):
        assert_records_close(g, r, f"cv window {i} (P = {pops[i]})")
    xy, table = edge_scene(rng, [3, 257], 8, 12)
    for method in (_abi.OPENLOOP_SGAN, _abi.OPENLOOP_CV):
        rc, _, _, _, untouched = call(engine, xy, table, 8, 12, method, S=2 if method else 1, model=2)
        assert rc == _abi.ERR_UNSUPPORTED and untouched


@pytest.mark.parametrize("obs_len,pred_len,S,pooling", [(1, 1, 1, None), (2, 12, 2, "pool_net"), (8, 32, 64, None), (8, 1, 2, "pool_net"),
                                                        (1, 32, 1, "pool_net")])
def test_lengths_and_sample_counts_at_their_edges(engine, obs_len, pred_len, S, pooling):
    """obs_len 1 (constant velocity: zero velocity), 2, 8; pred_len 1, 12, 32; S 1, 2, 64; the last window ends on the
    scene's last frame; no window and one window."""
    rng = np.random.default_rng(obs_len * 100 + pred_len)
    load(engine, 3, tiny_args(obs_len, pred_len, pooling))
    xy, table = edge_scene(rng, [3, 1, 4], obs_len, pred_len)
    assert table[0][-1] + obs_len + pred_len == xy.shape[0]
    tot, rec, raw = ok(engine, xy, table, obs_len, pred_len, _abi.OPENLOOP_SGAN, S=S, model=3, want_raw=True)
    for i, (g, r) in enumerate(zip(rec, oc.scene_records(xy, table, obs_len, pred_len, 0.4, raw))):
        assert_records_close(g, r, f"window {i}")
    assert all(int(r["n_samples"]) == S for r in rec) and int(tot["nll_count"]) == (8 * pred_len if S >= 2 else 0)
    cv_tot, cv_rec, _ = ok(engine, xy, table, obs_len, pred_len, _abi.OPENLOOP_CV)
    for i, (g, r) in enumerate(zip(cv_rec, oc.scene_records(xy, table, obs_len, pred_len, 0.4))):
        assert_records_close(g, r, f"cv window {i}")
    if obs_len == 1:                                                # zero velocity: the track stays at the observation
        o, t = oc.window_rows(xy, 0, table[2][:3], 1, pred_len)
        want_fde = np.linalg.norm(o[0].astype(np.float64) - t[:, -1], axis=1).mean()
        assert abs(float(cv_rec[0]["fde_scene"]) - want_fde) <= SUM_RTOL * want_fde
    one = (table[0][2:], np.array([0, 4], np.int32), table[2][4:])
    t1, r1, _ = ok(engine, xy, one, obs_len, pred_len, _abi.OPENLOOP_CV)
    assert r1.tobytes() == cv_rec[2:].tobytes() and int(t1["n_windows"]) == 1
    none = (table[0][:0], np.zeros(1, np.int32), table[2][:0])
    for method, s in ((_abi.OPENLOOP_CV, 1), (_abi.OPENLOOP_SGAN, S)):
        t0, r0, _ = ok(engine, xy, none, obs_len, pred_len, method, S=s, model=3)
        assert len(r0) == 0 and t0.tobytes() == np.zeros((), oc.TOTALS_DT).tobytes()


def test_length_and_sample_capacities_are_refused(engine):
    rng = np.random.default_rng(43)
    load(engine, 3, tiny_args(8, 12, None))
    xy, table = edge_scene(rng, [3], 8, 33)
    for kw, rc in ((dict(pred_len=33), _abi.ERR_UNSUPPORTED), (dict(S=65), _abi.ERR_UNSUPPORTED), (dict(obs_len=33, pred_len=8), _abi.ERR_UNSUPPORTED),
                   (dict(S=0), _abi.ERR_INVALID), (dict(pred_len=0), _abi.ERR_INVALID), (dict(obs_len=0), _abi.ERR_INVALID)):
        a = dict(obs_len=8, pred_len=12, S=2)
        a.update(kw)
        got = call(engine, xy, table, a["obs_len"], a["pred_len"], _abi.OPENLOOP_SGAN, S=a["S"], model=3)
        assert got[0] == rc and got[4], kw
    got = call(engine, xy, table, 8, 33, _abi.OPENLOOP_CV)
    assert got[0] == _abi.ERR_UNSUPPORTED and got[4]
    got = call(engine, xy, table, 8, 12, _abi.OPENLOOP_CV, S=2)     # one sample only
    assert got[0] == _abi.ERR_INVALID and got[4]


def test_a_model_without_noise_skips_the_nll(engine):
    rng = np.random.default_rng(44)
    load(engine, 4, tiny_args(8, 12, None, nd=0))
    xy, table = edge_scene(rng, [3, 2], 8, 12)
    tot, rec, raw = ok(engine, xy, table, 8, 12, _abi.OPENLOOP_SGAN, S=4, model=4, want_raw=True)
    assert all(raw[s].tobytes() == raw[0].tobytes() for s in range(4))
    assert int(tot["nll_count"]) == 0 and not any(int(r["flags"]) & FLAG_NLL for r in rec) and int(tot["traj_count"]) == 5
    assert np.isnan(oc.result_of(tot)["nll"]) and all(int(r["n_samples"]) == 4 for r in rec)
    for i, (g, r) in enumerate(zip(rec, oc.scene_records(xy, table, 8, 12, 0.4, raw))):
        assert_records_close(g, r, f"window {i}")


def test_noise_per_scene_is_keyed_by_the_window(engine):
    """A model with noise_mix_type 'global': one noise row per window, the counter's index word 0."""
    rng = np.random.default_rng(45)
    load(engine, 4, tiny_args(8, 12, "pool_net", mix="global", every=False))
    xy, table = edge_scene(rng, [3, 2, 4], 8, 12)
    tot, rec, raw = ok(engine, xy, table, 8, 12, _abi.OPENLOOP_SGAN, S=3, model=4, seed=9, win_id0=5, want_raw=True)
    noise = engine.sgan_noise(9, _abi.NOISE_GAUSSIAN, 3, 2, [5, 6, 7], [0, 0, 0], [0, 0, 0])
    direct = sgan_sample(engine, 4, 12, table[1], window_obs(xy, table, 8), noise)
    assert raw.tobytes() == direct.tobytes()
    t2, r2, _ = ok(engine, xy, table, 8, 12, _abi.OPENLOOP_SGAN, S=3, model=4, noise=noise, max_rows=5)
    assert r2.tobytes() == rec.tobytes() and t2.tobytes() == tot.tobytes()


# ---- what a window's record does not depend on ---------------------------------------------------------------------------------
def test_records_are_byte_identical_across_chunks_company_placement_and_element_type(fix, engine):
    import torch
    meta = fix["meta"]
    obs_len, pred_len, S = meta["obs_len"], meta["pred_len"], 3
    load(engine, 5, tiny_args(obs_len, pred_len, "pool_net"))
    xy = fix["scene"].astype(np.float32).astype(np.float64)
    table = tuple(fixed_windows(xy, obs_len + pred_len))
    pops = np.diff(table[1])
    args = (engine, xy, table, obs_len, pred_len, _abi.OPENLOOP_SGAN)
    tot, rec, raw = ok(*args, S=S, model=5, seed=17, want_raw=True)
    assert int(tot["nll_count"]) == int(pops.sum()) * pred_len
    # chunks: the largest window, 100 rows, everything; a boundary exactly at a window's end and one row short of the next
    for max_rows in (int(pops.max()), 100, 10 ** 6, int(pops[0] + pops[1]), int(pops[0] + pops[1] + pops[2] - 1)):
        t2, r2, raw2 = ok(*args, S=S, model=5, seed=17, max_rows=max_rows, want_raw=True)
        assert r2.tobytes() == rec.tobytes() and t2.tobytes() == tot.tobytes() and raw2.tobytes() == raw.tobytes(), max_rows
    # a window alone under its own win_id0, and a scene split over two calls
    for w in (0, 4, len(pops) - 1):
        lo, hi = table[1][w], table[1][w + 1]
        alone = (table[0][w:w + 1], np.array([0, hi - lo], np.int32), table[2][lo:hi])
        _, r1, _ = ok(engine, xy, alone, obs_len, pred_len, _abi.OPENLOOP_SGAN, S=S, model=5, seed=17, win_id0=w)
        assert r1.tobytes() == rec[w:w + 1].tobytes(), w
    k = 4
    tail = (table[0][k:], table[1][k:] - table[1][k], table[2][table[1][k]:])
    _, r_tail, _ = ok(engine, xy, tail, obs_len, pred_len, _abi.OPENLOOP_SGAN, S=S, model=5, seed=17, win_id0=k)
    assert r_tail.tobytes() == rec[k:].tobytes()
    # host against device scene; float32 against float64 of the same values
    for scene, dev in ((xy, True), (xy.astype(np.float32), False), (xy.astype(np.float32), True)):
        t2, r2, _ = ok(engine, scene, table, obs_len, pred_len, _abi.OPENLOOP_SGAN, S=S, model=5, seed=17, device_scene=dev)
        assert r2.tobytes() == rec.tobytes() and t2.tobytes() == tot.tobytes(), (scene.dtype, dev)
    # counter noise against the same numbers from fot_sgan_noise, from host and from device memory
    slots = np.repeat(np.arange(len(pops)), pops)
    idx = np.concatenate([np.arange(p) for p in pops])
    noise = engine.sgan_noise(17, _abi.NOISE_GAUSSIAN, S, 2, slots, np.zeros(len(slots), np.int64), idx)
    for given in (noise, torch.from_numpy(noise).to("cuda:0")):
        t2, r2, raw2 = ok(*args, S=S, model=5, noise=given, max_rows=7, want_raw=True)
        assert r2.tobytes() == rec.tobytes() and t2.tobytes() == tot.tobytes() and raw2.tobytes() == raw.tobytes()
    # constant velocity keeps the same invariances
    cv_tot, cv_rec, _ = ok(engine, xy, table, obs_len, pred_len, _abi.OPENLOOP_CV)
    for scene, dev, max_rows in ((xy, True, 0), (xy.astype(np.float32), False, int(pops.max())), (xy, False, 100)):
        t2, r2, _ = ok(engine, scene, table, obs_len, pred_len, _abi.OPENLOOP_CV, device_scene=dev, max_rows=max_rows)
        assert r2.tobytes() == cv_rec.tobytes() and t2.tobytes() == cv_tot.tobytes()


# ---- refusals and flags -----------------------------------------------------------------------------------------------------------
def test_every_refusal_leaves_the_outputs_untouched(engine):
    rng = np.random.default_rng(46)
    load(engine, 6, tiny_args(8, 12, None))
    _abi.lib().fot_sgan_unload_model(engine._h, 7)                  # (an empty slot; FOT_ERR_INVALID if it was empty already)
    xy, (f0, off, col) = edge_scene(rng, [3, 5], 8, 12)
    sgan = dict(S=2, model=6)
    bad_col, neg_col, late, early = col.copy(), col.copy(), f0.copy(), f0.copy()
    bad_col[2], neg_col[0], late[1], early[0] = xy.shape[1], -1, f0[1] + 1, -1
    cases = [
        ("column past the scene", (f0, off, bad_col), dict(sgan), _abi.ERR_INVALID),
        ("negative column", (f0, off, neg_col), dict(sgan), _abi.ERR_INVALID),
        ("window past n_frames", (late, off, col), dict(sgan), _abi.ERR_INVALID),
        ("window before frame 0", (early, off, col), dict(sgan), _abi.ERR_INVALID),
        ("offsets decreasing", (f0, np.array([0, 5, 3], np.int32), col), dict(sgan), _abi.ERR_INVALID),
        ("offsets not from 0", (f0, off + 1, np.concatenate([col, col[:1]])), dict(sgan), _abi.ERR_INVALID),
        ("max_rows below the largest window", (f0, off, col), dict(sgan, max_rows=4), _abi.ERR_INVALID),
        ("negative max_rows", (f0, off, col), dict(sgan, max_rows=-1), _abi.ERR_INVALID),
        ("no model loaded", (f0, off, col), dict(S=2, model=7), _abi.ERR_INVALID),
        ("model outside the slots", (f0, off, col), dict(S=2, model=99), _abi.ERR_INVALID),
        ("unknown flag", (f0, off, col), dict(sgan, flags=4), _abi.ERR_INVALID),
        ("unknown noise kind", (f0, off, col), dict(sgan, kind=_abi.NOISE_KINDS), _abi.ERR_INVALID),
        ("raw noise words", (f0, off, col), dict(sgan, kind=_abi.NOISE_RAW), _abi.ERR_INVALID),
        ("unknown dtype", (f0, off, col), dict(sgan, scene_dtype=2), _abi.ERR_INVALID),
        ("negative win_id0", (f0, off, col), dict(sgan, win_id0=-1), _abi.ERR_INVALID),
        ("dt 0", (f0, off, col), dict(sgan, dt=0.0), _abi.ERR_INVALID),
        ("negative n_cols", (f0, off, col), dict(sgan, dims=(xy.shape[0], -1)), _abi.ERR_INVALID),
        ("fewer frames than the window needs", (f0, off, col), dict(sgan, dims=(20, xy.shape[1])), _abi.ERR_INVALID),
    ]
    for label, table, kw, want in cases:
        rc, _, _, _, untouched = call(engine, xy, table, 8, 12, _abi.OPENLOOP_SGAN, want_raw=True, **kw)
        assert rc == want and untouched, label
        assert _abi.lib().fot_last_error(engine._h).decode().startswith("fot_openloop_eval"), label
    rc, _, _, _, untouched = call(engine, xy, (f0, off, col), 8, 12, 2, **sgan)       # an unknown method
    assert rc == _abi.ERR_INVALID and untouched
    rc, _, _, _, untouched = call(engine, xy, (f0, off, col), 7, 12, _abi.OPENLOOP_SGAN, **sgan)   # not the model's obs_len
    assert rc == _abi.ERR_INVALID and untouched
    tot, rec, _ = ok(engine, xy, (f0, off, col), 8, 12, _abi.OPENLOOP_SGAN, **sgan)   # ... and the handle still works
    assert int(tot["n_windows"]) == 2


def test_nonfinite_coordinates_raise_the_flag_and_stay_out_of_the_sums(engine):
    rng = np.random.default_rng(47)
    xy, table = edge_scene(rng, [3, 2], 8, 12)
    xy = np.concatenate([xy, xy[:, :1] + 1.0], axis=1)              # a column only window 0 holds
    table = (table[0], table[1], np.concatenate([[xy.shape[1] - 1], table[2][1:]]).astype(np.int32))
    xy[12, -1] = np.nan                                             # a truth frame of window 0
    tot, rec, _ = ok(engine, xy, table, 8, 12, _abi.OPENLOOP_CV)
    assert int(rec[0]["flags"]) & _abi.PRED_NONFINITE and np.isnan(rec[0]["ade_scene"]) and not int(rec[1]["flags"]) & _abi.PRED_NONFINITE
    assert int(tot["n_windows"]) == 2 and int(tot["traj_count"]) == 2 and int(tot["flags"]) & _abi.PRED_NONFINITE
    assert tot.tobytes() == oc.fold_windows(rec).tobytes()
