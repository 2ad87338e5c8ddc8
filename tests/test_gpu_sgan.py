"""Social-GAN sample generation on the GPU (fot_sgan_sample): every fixture case under the accuracy bound; host and device
placements; a second load on one handle; scenes alone against the same scenes in one launch, bit for bit; the refusals
that need a handle; and a distribution-aware closed loop driven by SganSampler with the samples resident in HBM."""
import ctypes as C

import numpy as np
import pytest

import sgan_common as sc
from integrated_path_planning_amd import _abi, synthetic as syn
from integrated_path_planning_amd.closed_loop import BatchedClosedLoop
from integrated_path_planning_amd.planner import BatchPlanner
from integrated_path_planning_amd.prediction import SganSampler, SganWeights

pytestmark = pytest.mark.gpu
NAMES = tuple(sc.CASES)


@pytest.fixture(scope="module")
def fix():
    return sc.load_fixture()


@pytest.fixture(scope="module")
def engine():
    with BatchPlanner(waypoints=(syn.STRAIGHT_WX, syn.STRAIGHT_WY), device=0, **syn.CONFIG3_PLANNER) as bp:
        yield bp


_weights = {}


def case_weights(name):
    if name not in _weights:
        a = sc.case_args(name)
        _weights[name] = SganWeights.from_state_dict(a, sc.seeded_state(a, sc.case_seed(name), sc.case_scale(name)))
    return _weights[name]


def load(engine, w):
    return _abi.lib().fot_sgan_load(engine._h, C.byref(w.desc), w.blob.size, w.blob.ctypes.data)


def sample_rc(engine, pred_len, off, obs, S, noise, device=(False, False, False), out=None):
    """fot_sgan_sample with obs / noise / out in host or device memory -> (return code, out [S, pred_len, N, 2] on the host)."""
    import torch
    off = np.ascontiguousarray(off, np.int32)
    n = int(off[-1]) if len(off) else 0
    obs, noise = np.ascontiguousarray(obs, np.float32), np.ascontiguousarray(noise, np.float32)
    host_out = np.full((max(S, 0), pred_len, n, 2), np.float32(-77.0)) if out is None else out
    keep, flags, ptr = [], 0, []
    for arr, on_dev, bit in ((obs, device[0], _abi.SGAN_OBS_DEVICE), (noise, device[1], _abi.SGAN_NOISE_DEVICE),
                             (host_out, device[2], _abi.OUT_DEVICE)):
        if on_dev:
            t = torch.from_numpy(arr.copy()).to("cuda:0")
            torch.cuda.synchronize()
            keep.append(t)
            ptr.append(C.c_void_p(t.data_ptr()) if t.numel() else None)
            flags |= bit
        else:
            keep.append(arr)
            ptr.append(C.c_void_p(arr.ctypes.data) if arr.size else None)
    rc = _abi.lib().fot_sgan_sample(engine._h, len(off) - 1, off.ctypes.data, ptr[0], S, ptr[1], flags, ptr[2], None)
    if device[2]:
        host_out = keep[2].cpu().numpy()
    return rc, host_out


def sample(engine, w, off, obs, noise, device=(False, False, False)):
    rc, out = sample_rc(engine, w.desc.pred_len, off, obs, noise.shape[0], noise, device)
    assert rc == _abi.OK, _abi.lib().fot_last_error(engine._h)
    return out


# ---- accuracy ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_every_fixture_case_is_within_the_accuracy_bound(fix, engine, name):
    obs, off, noise, r32, r64 = sc.fixture_case(fix, name)
    w = case_weights(name)
    assert load(engine, w) == _abi.OK
    got = sample(engine, w, off, obs, noise)
    assert got.shape == r64.shape and got.dtype == np.float32
    err, bound = float(np.max(np.abs(got.astype(np.float64) - r64))), sc.accuracy_bound(r32, r64)
    print(f"{name}: error {err:.3e}, bound {bound:.3e}, ratio {err / bound:.3f}")
    assert err <= bound


def test_samples_without_noise_are_identical_and_with_noise_differ(fix, engine):
    for name, same in (("d_plain_step_ped", True), ("a_pool_step_ped_bn", False)):
        obs, off, noise, _, _ = sc.fixture_case(fix, name)
        w = case_weights(name)
        assert load(engine, w) == _abi.OK
        got = sample(engine, w, off, obs, noise)
        assert np.array_equal(got[0], got[1]) == same


# ---- placements, loads, launches -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["a_pool_step_global", "b_none_ped_bn", "a_pool_once_ped"])
def test_host_and_device_placements_agree_bit_for_bit(fix, engine, name):
    obs, off, noise, _, _ = sc.fixture_case(fix, name)
    w = case_weights(name)
    assert load(engine, w) == _abi.OK
    want = sample(engine, w, off, obs, noise)
    for device in ((True, True, True), (True, False, False), (False, True, False), (False, False, True)):
        np.testing.assert_array_equal(sample(engine, w, off, obs, noise, device), want, err_msg=str(device))


def test_a_second_load_on_one_handle_answers(fix, engine):
    first, second = "c_big_pool_step_ped_bn", "b_none_global_bn"          # the larger image first: the smaller one reuses its block
    obs1, off1, noise1, _, _ = sc.fixture_case(fix, first)
    obs2, off2, noise2, r32, r64 = sc.fixture_case(fix, second)
    assert load(engine, case_weights(first)) == _abi.OK
    a = sample(engine, case_weights(first), off1, obs1, noise1)
    assert load(engine, case_weights(second)) == _abi.OK
    b = sample(engine, case_weights(second), off2, obs2, noise2)
    assert np.max(np.abs(b.astype(np.float64) - r64)) <= sc.accuracy_bound(r32, r64)
    assert load(engine, case_weights(first)) == _abi.OK
    np.testing.assert_array_equal(sample(engine, case_weights(first), off1, obs1, noise1), a)
    # a refused load leaves the loaded model in place
    w = case_weights(second)
    assert _abi.lib().fot_sgan_load(engine._h, C.byref(w.desc), w.blob.size - 1, w.blob.ctypes.data) == _abi.ERR_INVALID
    np.testing.assert_array_equal(sample(engine, case_weights(first), off1, obs1, noise1), a)


@pytest.mark.parametrize("name", ["a_pool_step_ped", "a_pool_step_global", "b_pool_once_global", "a_none_step_global_bn",
                                  "b_pool_step_ped_bn"])
def test_scenes_in_one_launch_equal_the_scenes_alone(fix, engine, name):
    obs, off, noise, _, _ = sc.fixture_case(fix, name)
    w = case_weights(name)
    assert load(engine, w) == _abi.OK
    whole = sample(engine, w, off, obs, noise)
    per_scene = w.desc.noise_mix_type == _abi.SGAN_NOISE_GLOBAL
    for i, (lo, hi) in enumerate(zip(off[:-1], off[1:])):
        z = noise[:, i:i + 1] if per_scene else noise[:, lo:hi]
        alone = sample(engine, w, [0, hi - lo], obs[:, lo:hi], z)
        np.testing.assert_array_equal(alone, whole[:, :, lo:hi], err_msg=f"scene {i}")
    # ... and in another order, with an empty scene in between
    order = list(range(len(off) - 1))[::-1]
    cols = [np.arange(off[i], off[i + 1]) for i in order]
    off2 = np.concatenate([[0], np.cumsum([len(cols[0]), 0] + [len(c) for c in cols[1:]])])
    z2 = (np.concatenate([noise[:, order[:1]], np.zeros_like(noise[:, :1]), noise[:, order[1:]]], axis=1) if per_scene
          else noise[:, np.concatenate(cols)])
    again = sample(engine, w, off2, obs[:, np.concatenate(cols)], z2)
    np.testing.assert_array_equal(again, whole[:, :, np.concatenate(cols)])


# ---- refusals ------------------------------------------------------------------------------------------------------------
def test_refusals_change_nothing(fix):
    name = "a_pool_step_ped_bn"
    obs, off, noise, _, _ = sc.fixture_case(fix, name)
    w = case_weights(name)
    L, S = w.desc.pred_len, noise.shape[0]
    with BatchPlanner(waypoints=(syn.STRAIGHT_WX, syn.STRAIGHT_WY), device=0, **syn.CONFIG3_PLANNER) as bp:
        def refused(code, off_, obs_, S_, noise_):
            rc, out = sample_rc(bp, L, off_, obs_, S_, noise_)
            assert rc == code, (rc, _abi.lib().fot_last_error(bp._h))
            assert _abi.lib().fot_last_error(bp._h)
            assert np.all(out == np.float32(-77.0))                  # the output was not touched

        refused(_abi.ERR_INVALID, off, obs, S, noise)                # no model loaded
        d = _abi.SganDesc.from_buffer_copy(bytes(w.desc))
        d.pooling_type = _abi.SGAN_SPOOL
        assert _abi.lib().fot_sgan_load(bp._h, C.byref(d), w.blob.size, w.blob.ctypes.data) == _abi.ERR_UNSUPPORTED
        assert _abi.lib().fot_sgan_load(bp._h, C.byref(w.desc), w.blob.size + 1, w.blob.ctypes.data) == _abi.ERR_INVALID
        refused(_abi.ERR_INVALID, off, obs, S, noise)                # ... still none
        assert load(bp, w) == _abi.OK
        want = sample(bp, w, off, obs, noise)
        refused(_abi.ERR_INVALID, [0, 3, 2, 11], obs, S, noise)      # decreasing offsets
        refused(_abi.ERR_INVALID, [1, 4, 11], obs[:, :11], S, noise) # not starting at 0
        refused(_abi.ERR_INVALID, off, obs, 0, noise[:0])            # S < 1
        many = _abi.MAX_SAMPLES + 1
        refused(_abi.ERR_UNSUPPORTED, off, obs, many, np.zeros((many,) + noise.shape[1:], np.float32))
        wide = _abi.SGAN_MAX_PEDS + 1
        refused(_abi.ERR_UNSUPPORTED, [0, wide], np.zeros((w.desc.obs_len, wide, 2), np.float32), 1,
                np.zeros((1, wide, w.desc.noise_dim), np.float32))
        rc = _abi.lib().fot_sgan_sample(bp._h, 3, np.ascontiguousarray(off, np.int32).ctypes.data, None, S, None, 0, None, None)
        assert rc == _abi.ERR_INVALID                                # NULL tensors
        np.testing.assert_array_equal(sample(bp, w, off, obs, noise), want)
        # no scene, and scenes without pedestrians: nothing to do
        assert sample_rc(bp, L, [0], obs[:, :0], S, noise[:, :0])[0] == _abi.OK
        assert sample_rc(bp, L, [0, 0, 0], obs[:, :0], S, noise[:, :0])[0] == _abi.OK
        assert _abi.lib().fot_sgan_unload(bp._h) == _abi.OK
        refused(_abi.ERR_INVALID, off, obs, S, noise)                # unloaded


# ---- the closed loop --------------------------------------------------------------------------------------------------------
class _RecordingSampler(SganSampler):
    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.record = []

    def sample(self, obs, ped_off, noise=None):
        out = super().sample(obs, ped_off, noise)
        self.record.append((self.last_obs.cpu().numpy(), self.last_ped_off.copy(), self.last_noise.cpu().numpy(), out.cpu().numpy()))
        return out

    __call__ = sample


def test_distribution_aware_closed_loop_with_the_sampler(engine):
    """Three episodes in one lock step -- one ends early (a wall of pedestrians runs into the ego), one has no pedestrians --
    planned against the sampler's distribution, which never leaves HBM.  Every step's tensor is held to the float64
    restatement on the window and noise the sampler recorded; the reference is not at hand there, so e_ref of the bound is
    the restatement's own float32 run against its float64 run on those inputs (the same operations as the reference's
    float32 run; on the fixture the two agree within a factor of two)."""
    from pred_scores_common import load_cases
    fx = load_cases()
    cfg = dict(fx["meta"]["episodes"]["weave_s4"]["config"])
    tracks = [sc.charging_wall_tracks(), fx["weave_s4_ped_traj"][:, :0], fx["weave_s4_ped_traj"]]
    name = "a_pool_step_ped_bn"
    a = sc.case_args(name)
    state = sc.seeded_state(a, sc.case_seed(name), sc.case_scale(name))
    S = 4
    src = _RecordingSampler(engine, case_weights(name), S, seed=5)
    with BatchedClosedLoop(cfg, tracks, sample_source=src, device_samples=True, prediction_scores=True) as sim:
        assert sim._native and sim._device_samples and sim.distribution_aware
        ran = [sim.step() for _ in range(12)]
        assert ran[0] == 3 and ran[-1] == 2 and not sim.alive[0] and sim.episodes[0].termination_reason == "collision"
        assert len(src.record) == 12
        widths = np.array([t.shape[1] for t in tracks])
        seen = set()
        for step, (obs, off, noise, out) in enumerate(src.record):
            n_ep = ran[step]
            want_off = np.concatenate([[0], np.cumsum(widths if n_ep == 3 else widths[1:])])
            np.testing.assert_array_equal(off, want_off)
            assert obs.shape == (cfg["obs_len"], off[-1], 2) and noise.shape == (S, off[-1], a["noise_dim"][0])
            assert out.shape == (S, cfg["pred_len"], off[-1], 2) and np.isfinite(out).all()
            r64 = sc.restate(a, state, obs, off, noise)
            r32 = sc.restate(a, state, obs, off, noise, np.float32)
            err, bound = float(np.max(np.abs(out.astype(np.float64) - r64))), sc.accuracy_bound(r32, r64)
            print(f"step {step}: {n_ep} episodes, error {err:.3e}, bound {bound:.3e}")
            assert err <= bound
            seen.add(noise.tobytes())
        assert len(seen) == 12                                      # fresh noise every step
        assert sim._score_steps
        for sel, _, rec in sim._score_steps:
            assert len(rec) == len(sel)
            for e, r in zip(sel, rec):
                assert all(np.isfinite(float(r[k])) for k in ("ade_scene", "fde_scene", "ade_agent_sum", "fde_agent_sum", "log_lik_sum"))
                assert int(r["n_peds"]) == widths[e] and (widths[e] == 0 or int(r["n_samples"]) == S)
        assert len(sim.prediction_metrics()) == 3
    # the same seed draws the same noise
    again = SganSampler(engine, case_weights(name), S, seed=5)
    obs, off, noise, out = src.record[0]
    np.testing.assert_array_equal(again.sample(obs, off).cpu().numpy(), out)
    np.testing.assert_array_equal(again.last_noise.cpu().numpy(), noise)
    np.testing.assert_array_equal(again.sample(obs, off, noise=noise).cpu().numpy(), out)
