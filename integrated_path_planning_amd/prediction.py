"""the obstacle-tensor producer in front of the planner, on the device.

Mirrors ``TrajectoryPredictor.process_prediction`` / ``predict_cv`` / the closest-to-mean pick of
``predict_single_best`` (reference src/prediction/trajectory_predictor.py:188-353) and the current-position
prepend of ``IntegratedSimulator._update_prediction`` (integrated_simulator.py:503-525): the samples' raw output is
turned into the planner's ``[S, P, T, 2]`` tensor without leaving the GPU.

The Social-GAN forward passes themselves run in the library as well (``SganWeights`` / ``SganSampler`` over
``fot_sgan_sample``): all samples of all scenes in one call, in float32, from weights under the reference's state-dict
names; PyTorch-ROCm only draws the noise.
"""
from __future__ import annotations

import ctypes as C
from typing import NamedTuple, Optional, Tuple

import numpy as np

from . import _abi
from .planner import BatchPlanner

_dp = C.POINTER(C.c_double)


def _host_pd(a):
    return None if a is None else np.ascontiguousarray(a, dtype=np.float64).ctypes.data_as(_dp)


class PredictionResampler:
    def __init__(self, engine: BatchPlanner, pred_len: int = 12, sgan_dt: float = 0.4, sim_dt: float = 0.1,
                 plan_horizon: float = 5.0):
        self.engine = engine
        self.pred_len = int(pred_len)
        self.params = _abi.ResampleParams(float(sgan_dt), float(sim_dt), float(plan_horizon))
        self._lib = _abi.lib()

    @property
    def n_dense(self) -> int:
        return self._lib.fot_resample_n_dense(C.byref(self.params), self.pred_len)

    # -- host tensors in, host tensors out (drop-in for the reference methods) --------------------------
    def process_prediction(self, pred_traj: np.ndarray, anchor_pos: Optional[np.ndarray] = None,
                           staleness: float = 0.0, current: Optional[np.ndarray] = None,
                           want_sample_dist: bool = False):
        """pred_traj [pred_len, P, 2] -> [P, T, 2], or [S, pred_len, P, 2] -> [S, P, T, 2]."""
        pred = np.asarray(pred_traj)
        if pred.size == 0:
            return np.empty((0, 0, 2))
        single = pred.ndim == 3
        if single:
            pred = pred[None]
        if pred.ndim != 4 or pred.shape[-1] != 2:
            raise ValueError(f"Unexpected prediction shape: {np.shape(pred_traj)}")
        dt = np.float32 if pred.dtype == np.float32 else np.float64
        pred = np.ascontiguousarray(pred, dtype=dt)
        S, L, P = pred.shape[0], pred.shape[1], pred.shape[2]
        T = self._lib.fot_resample_n_dense(C.byref(self.params), L) + (0 if current is None else 1)
        out = np.zeros((S, P, T, 2), dtype=dt)
        dist = np.zeros(S) if want_sample_dist else None
        t_out = C.c_int32(0)
        code = _abi.F32 if dt == np.float32 else _abi.F64
        keep = (_host_pd(anchor_pos), _host_pd(current))
        _abi.check(self.engine._h, self._lib.fot_resample_predictions(
            self.engine._h, C.byref(self.params), S, L, P, pred.ctypes.data, code, keep[0], keep[1], float(staleness),
            out.ctypes.data, code, 0, C.byref(t_out), None if dist is None else dist.ctypes.data_as(_dp), None))
        assert t_out.value == T
        res = out[0] if single else out
        return (res, dist) if want_sample_dist else res

    def predict_cv(self, obs_traj: np.ndarray, staleness: float = 0.0, current: Optional[np.ndarray] = None,
                   float32_observations: bool = False):
        """obs_traj [obs_len, P, 2] (absolute) -> [P, T, 2]; velocity from the last two samples (:203-217).

        float32_observations: round the observations to float32 first and form the velocity in float32 -- what the
        reference does when the observer hands over its float tensors (observer.py:134)."""
        dt = np.float32 if float32_observations else np.float64
        obs = np.asarray(obs_traj).astype(dt)
        P = obs.shape[1]
        last = np.ascontiguousarray(obs[-1])
        prev = np.ascontiguousarray(obs[-2]) if obs.shape[0] >= 2 else None
        T = self.n_dense + (0 if current is None else 1)
        out = np.zeros((P, T, 2))
        t_out = C.c_int32(0)
        _abi.check(self.engine._h, self._lib.fot_predict_cv(
            self.engine._h, C.byref(self.params), self.pred_len, P, last.ctypes.data,
            None if prev is None else prev.ctypes.data, _abi.F32 if float32_observations else _abi.F64,
            _host_pd(current), float(staleness), out.ctypes.data, _abi.F64, 0, C.byref(t_out), None))
        return out

    @staticmethod
    def best_sample(sample_dist: np.ndarray) -> int:
        """np.argmin of the distances to the sample mean: first minimum (:349-350)."""
        return int(np.argmin(sample_dist))

    # -- device tensors (what the planner consumes through fot_plan_batch_device) ------------------------
    def resample_device(self, pred_ptr: int, pred_dtype, S: int, P: int, anchor_pos, current, staleness: float,
                        out_ptr: int, out_dtype, stream: Optional[int] = None, want_sample_dist: bool = False,
                        t_major: bool = False) -> Tuple[int, Optional[np.ndarray]]:
        """pred [S][pred_len][P][2] and out [S][P][T][2] are device pointers; returns (T, sample_dist).
        t_major: out is written [T][S][P][2] -- the layout the planner's broad phase reads fully coalesced; hand it on
        with ``PackedBatch(..., dyn_layout_tsp=True)`` / ``_abi.DYN_LAYOUT_TSP`` in ``dyn_dims``."""
        dist = np.zeros(S) if want_sample_dist else None
        t_out = C.c_int32(0)
        code = lambda d: _abi.F32 if np.dtype(d) == np.dtype(np.float32) else _abi.F64
        keep = (_host_pd(anchor_pos), _host_pd(current))
        _abi.check(self.engine._h, self._lib.fot_resample_predictions(
            self.engine._h, C.byref(self.params), S, self.pred_len, P, C.c_void_p(pred_ptr), code(pred_dtype), keep[0],
            keep[1], float(staleness), C.c_void_p(out_ptr), code(out_dtype),
            _abi.OUT_DEVICE | (_abi.OUT_TMAJOR if t_major else 0), C.byref(t_out),
            None if dist is None else dist.ctypes.data_as(_dp), C.c_void_p(stream) if stream else None))
        return t_out.value, dist


def prediction_scores(engine: BatchPlanner, samples, truth, stride: int, t_major: bool = False, skip: int = 0,
                      stream: Optional[int] = None) -> np.ndarray:
    """Score sample predictions on the device: per origin what the reference's ``_standard_ade_fde_details`` and
    ``_kde_nll_details`` (src/core/metrics.py:31-176) add to their totals for it (``fot_prediction_scores``).

    samples: one origin's distribution [S, P, T, 2] ([T, S, P, 2] with ``t_major``) or a sequence of them, NumPy arrays or
    ``torch`` CUDA tensors of one element type (float32 / float64; a float32 tensor gives the scores of the rounded
    samples, the arithmetic is float64 either way); a sequence of device tensors is scored origin by origin where it lies,
    a sequence of arrays in one launch.  truth: per origin [P, E, 2] -- the pedestrians' positions ``stride * j`` steps
    after the origin, j = 1 .. E, compared with dense samples ``stride * j - 1 + skip``.  Returns one record per origin
    (``BatchPlanner.PRED_SCORE_DT``: ade_scene, fde_scene, ade_agent_sum, fde_agent_sum, log_lik_sum, n_peds, n_samples,
    nll_count, flags)."""
    single = hasattr(samples, "shape") and len(samples.shape) == 4
    blocks = [samples] if single else list(samples)
    truths = [np.asarray(truth, dtype=np.float64)] if single else [np.asarray(t, dtype=np.float64) for t in truth]
    if len(blocks) != len(truths):
        raise ValueError("prediction_scores: one truth block per origin")
    E = {t.shape[1] for t in truths}
    if len(E) > 1:
        raise ValueError("prediction_scores: the origins of one call share E")
    E = E.pop() if E else 1

    def dims(b):
        if len(b.shape) != 4 or b.shape[-1] != 2:
            raise ValueError(f"prediction_scores: a distribution is [S, P, T, 2], got {tuple(b.shape)}")
        return (b.shape[1], b.shape[2], b.shape[0]) if t_major else (b.shape[0], b.shape[1], b.shape[2])

    if blocks and hasattr(blocks[0], "data_ptr"):                   # device tensors: each where it lies
        out = [engine.prediction_scores(b, [(0,) + dims(b) + (t_major, skip)], t, stride, E, stream)
               for b, t in zip(blocks, truths)]
        return np.concatenate(out) if out else np.zeros(0, dtype=engine.PRED_SCORE_DT)
    dt = np.float32 if blocks and all(np.asarray(b).dtype == np.float32 for b in blocks) else np.float64
    flat = [np.ascontiguousarray(b, dtype=dt).reshape(-1, 2) for b in blocks]
    off = np.concatenate([[0], np.cumsum([len(f) for f in flat])])
    origins = [(int(off[i]),) + dims(b) + (t_major, skip) for i, b in enumerate(blocks)]
    tensor = np.concatenate(flat) if flat else np.zeros((0, 2), dt)
    tr = np.concatenate([t.reshape(-1, E, 2) for t in truths]) if truths else np.zeros((0, E, 2))
    return engine.prediction_scores(tensor, origins, tr, stride, E, stream)


# ---- Social-GAN sample generation (fot_sgan_*) ---------------------------------------------------------------------------
_POOLING = {None: _abi.SGAN_POOL_NONE, "none": _abi.SGAN_POOL_NONE, "pool_net": _abi.SGAN_POOL_NET, "spool": _abi.SGAN_SPOOL}
_NOISE_MIX = {"ped": _abi.SGAN_NOISE_PED, "global": _abi.SGAN_NOISE_GLOBAL}
_BN_EPS = 1e-5                                                      # nn.BatchNorm1d's default; make_mlp passes no other


def _np64(v):
    return np.asarray(v.detach().cpu().numpy() if hasattr(v, "detach") else v, dtype=np.float64)


def fold_batch_norm(weight, bias, bn_weight, bn_bias, running_mean, running_var, eps: float = _BN_EPS):
    """Linear followed by an eval-mode BatchNorm1d as ONE Linear: y = g (W x + b - mean) / sqrt(var + eps) + beta, in
    float64.  Returns (W', b')."""
    scale = _np64(bn_weight) / np.sqrt(_np64(running_var) + eps)
    return _np64(weight) * scale[:, None], (_np64(bias) - _np64(running_mean)) * scale + _np64(bn_bias)


_NOISE_TYPES = ("gaussian", "uniform")


def _checked_capacity(who: str, n) -> int:
    """A constructor's ``sample_capacity``: what a handle can be raised to."""
    if not _abi.MAX_SAMPLES <= int(n) <= _abi.MAX_PLAN_SAMPLES:
        raise ValueError(f"{who}: {_abi.MAX_SAMPLES} <= sample_capacity <= {_abi.MAX_PLAN_SAMPLES}, got {n}")
    return int(n)


class SganWeights:
    """A Social-GAN generator as ``fot_sgan_load`` takes it: the descriptor and ONE packed float32 blob in the order
    include/fot.h documents, BatchNorm folded into the Linear in front of it."""

    def __init__(self, desc: _abi.SganDesc, blob: np.ndarray, noise_type: str = "gaussian"):
        self.desc, self.blob, self.noise_type = desc, np.ascontiguousarray(blob, dtype=np.float32), noise_type
        n = C.c_int64(0)
        rc = _abi.lib().fot_sgan_weight_count(C.byref(desc), C.byref(n))
        if rc != _abi.OK:
            raise _abi.FotError(rc, (_abi.lib().fot_last_error(None) or b"").decode())
        if n.value != self.blob.size:
            raise ValueError(f"SganWeights: the blob holds {self.blob.size} floats, the descriptor needs {n.value}")

    @staticmethod
    def descriptor(args) -> _abi.SganDesc:
        """The generator's constructor arguments (a checkpoint's ``args``; the reference's names and defaults,
        trajectory_predictor.py:87-104) as a ``fot_sgan_desc``."""
        get = lambda k, default: args[k] if k in args else args.get(k + "_g", default) if hasattr(args, "get") else default
        noise_dim = get("noise_dim", (8,))
        noise_dim = tuple(noise_dim) if hasattr(noise_dim, "__len__") else (int(noise_dim),)
        if len(noise_dim) != 1:
            raise ValueError(f"SganWeights: a noise_dim of one entry, got {noise_dim}")
        pooling = get("pooling_type", "pool_net")
        pooling = pooling.lower() if isinstance(pooling, str) else pooling
        if pooling not in _POOLING:
            raise ValueError(f"SganWeights: unknown pooling_type {pooling!r}")
        mix = get("noise_mix_type", "ped")
        if mix not in _NOISE_MIX:
            raise ValueError(f"SganWeights: unknown noise_mix_type {mix!r}")
        return _abi.SganDesc(int(get("obs_len", 8)), int(get("pred_len", 12)), int(get("embedding_dim", 64)),
                             int(get("encoder_h_dim", 64)), int(get("decoder_h_dim", 128)), int(get("mlp_dim", 1024)),
                             int(get("bottleneck_dim", 1024)), int(noise_dim[0]), int(get("num_layers", 1)), _POOLING[pooling],
                             int(bool(get("pool_every_timestep", True))), _NOISE_MIX[mix], float(get("dropout", 0.0)), 0)

    @classmethod
    def from_state_dict(cls, args, state) -> "SganWeights":
        """args: the generator's constructor arguments (mapping); state: arrays (NumPy or torch) under the reference's
        state-dict names (``encoder.encoder.weight_ih_l0`` ...).  An MLP layer followed by BatchNorm (``<seq>.<i + 1>.
        running_mean`` present) is folded; everything is packed in float64 and rounded to float32 once."""
        d = cls.descriptor(args)
        pooled = d.pooling_type == _abi.SGAN_POOL_NET
        parts = []

        def linear(prefix):
            parts.extend([_np64(state[prefix + ".weight"]), _np64(state[prefix + ".bias"])])

        def lstm(prefix):
            for k in ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0"):
                parts.append(_np64(state[f"{prefix}.{k}"]))

        def mlp(prefix):                                            # make_mlp: Linear [, BatchNorm1d], ReLU, twice
            idx = sorted(int(k[len(prefix) + 1:].split(".")[0]) for k in state
                         if k.startswith(prefix + ".") and k.endswith(".weight") and np.ndim(state[k]) == 2)
            if len(idx) != 2:
                raise KeyError(f"SganWeights: {prefix} is not a two-layer MLP")
            for i in idx:
                w, b = _np64(state[f"{prefix}.{i}.weight"]), _np64(state[f"{prefix}.{i}.bias"])
                bn = f"{prefix}.{i + 1}"
                if bn + ".running_mean" in state:
                    w, b = fold_batch_norm(w, b, state[bn + ".weight"], state[bn + ".bias"], state[bn + ".running_mean"],
                                           state[bn + ".running_var"])
                parts.extend([w, b])

        def pool(prefix):
            linear(prefix + ".spatial_embedding")
            mlp(prefix + ".mlp_pre_pool")

        linear("encoder.spatial_embedding"); lstm("encoder.encoder")
        if pooled:
            pool("pool_net")
        if d.noise_dim > 0 or pooled or d.encoder_h_dim != d.decoder_h_dim:
            mlp("mlp_decoder_context")
        linear("decoder.spatial_embedding"); lstm("decoder.decoder"); linear("decoder.hidden2pos")
        if pooled and d.pool_every_timestep:
            pool("decoder.pool_net"); mlp("decoder.mlp")
        blob = np.concatenate([p.reshape(-1) for p in parts]).astype(np.float32)
        return cls(d, blob, noise_type=args.get("noise_type", "gaussian") if hasattr(args, "get") else "gaussian")

    @classmethod
    def from_checkpoint(cls, path) -> "SganWeights":
        """A released checkpoint file: ``torch.load`` and ``from_state_dict(ckpt['args'], ckpt['g_state'])`` (``g_best_state``
        when there is no ``g_state``), as the reference's loader reads it (trajectory_predictor.py:74, 124-128).

        Tested on files the suite writes itself (``args`` as a mapping and as an object, ``g_state`` and ``g_best_state``,
        the ``_g``-suffixed dimension names); NEVER run on a released checkpoint file: none was available where this was
        written and tested."""
        import torch
        ckpt = torch.load(path, map_location="cpu", weights_only=False)
        args = ckpt["args"]
        args = args if hasattr(args, "get") else vars(args)
        return cls.from_state_dict(args, ckpt["g_state"] if "g_state" in ckpt else ckpt["g_best_state"])


def crowd_scenes(slots, counts, steps, slot_crowd):
    """The sampler's call for running episodes that share crowds (``SganSampler(slot_crowd=...)``,
    ``fot_loop_set_sampler_shared``; csrc/fot_sweep.hpp's ``sweep_crowd_tables`` restated).  slots / counts / steps: slot,
    pedestrian count and step count of every running episode, in frame order; slot_crowd: the crowd of every slot of the
    loop.  A crowd is active when one of its episodes has pedestrians; its representative is its lowest slot among them.

    Returns ``(crowds, rep, noise_slots, cols)``: the active crowds' ids in ascending order; for each the index of its
    representative in ``slots``; the ``slot`` word of its noise -- the crowd's id; and for every pedestrian row of the
    frame its column among the representatives' concatenated rows.  ``ValueError`` where two episodes of a crowd disagree
    in pedestrian count or step count."""
    slots, counts, steps = (np.asarray(v, dtype=np.int64).reshape(-1) for v in (slots, counts, steps))
    slot_crowd = np.asarray(slot_crowd, dtype=np.int64).reshape(-1)
    if not len(slots) == len(counts) == len(steps):
        raise ValueError("crowd_scenes: one pedestrian count and one step count per slot")
    if len(slots) and (slots.min() < 0 or slots.max() >= len(slot_crowd)):
        raise ValueError(f"crowd_scenes: slot_crowd names {len(slot_crowd)} slots, the frame has slot {int(slots.max())}")
    crowd_of = slot_crowd[slots]
    rep_of = {}                                                       # crowd -> index of its lowest slot with pedestrians
    for i in np.argsort(slots, kind="stable"):
        if counts[i] > 0:
            j = rep_of.setdefault(int(crowd_of[i]), int(i))
            if counts[i] != counts[j] or steps[i] != steps[j]:
                raise ValueError(f"crowd_scenes: slots {int(slots[j])} and {int(slots[i])} of crowd {int(crowd_of[i])} differ in "
                                 f"their pedestrian counts ({int(counts[j])}, {int(counts[i])}) or step counts "
                                 f"({int(steps[j])}, {int(steps[i])})")
    crowds = np.array(sorted(rep_of), dtype=np.int64)
    rep = np.array([rep_of[int(c)] for c in crowds], dtype=np.int64)
    first = dict(zip(crowds.tolist(), np.concatenate([[0], np.cumsum(counts[rep])]).tolist()))
    cols = [first[int(c)] + np.arange(P) for c, P in zip(crowd_of, counts) if P > 0]
    return crowds, rep, crowds.copy(), (np.concatenate(cols) if cols else np.zeros(0, np.int64)).astype(np.int64)


def model_scenes(slots, counts, steps, slot_crowd, slot_model):
    """The sampler's calls for running episodes that share crowds and name their models (``SganSampler`` with several
    weights, ``fot_loop_set_sampler_models``; csrc/fot_sweep.hpp's ``sweep_model_tables`` restated).  slots / counts / steps
    as in ``crowd_scenes``; slot_crowd / slot_model: the crowd and the model of every slot of the loop.  A sampling unit is
    a (crowd, model) pair; model m's scenes are ``crowd_scenes`` of the episodes that name m.

    Returns ``(units, row_model, cols)``: for every model id 0 .. max(slot_model) its ``(crowds, rep, noise_slots)`` --
    ``rep`` indexes ``slots`` of the whole frame, all three empty for a model without an active unit --; and for every
    pedestrian row of the frame its model and its column among the rows of that model's representatives."""
    slots, counts, steps = (np.asarray(v, dtype=np.int64).reshape(-1) for v in (slots, counts, steps))
    slot_crowd, slot_model = (np.asarray(v, dtype=np.int64).reshape(-1) for v in (slot_crowd, slot_model))
    if len(slot_crowd) != len(slot_model):
        raise ValueError("model_scenes: one crowd and one model per slot")
    if not len(slots) == len(counts) == len(steps):
        raise ValueError("model_scenes: one pedestrian count and one step count per slot")
    if len(slots) and (slots.min() < 0 or slots.max() >= len(slot_model)):
        raise ValueError(f"model_scenes: slot_model names {len(slot_model)} slots, the frame has slot {int(slots.max())}")
    if len(slot_model) and slot_model.min() < 0:
        raise ValueError("model_scenes: slot_model holds one model id >= 0 per slot")
    n_models = int(slot_model.max()) + 1 if len(slot_model) else 0
    model_of = slot_model[slots]
    row_model = np.repeat(model_of, counts)
    cols = np.zeros(int(counts.sum()), np.int64)
    units = []
    for m in range(n_models):
        idx = np.flatnonzero(model_of == m)
        crowds, rep, noise_slots, sub_cols = crowd_scenes(slots[idx], counts[idx], steps[idx], slot_crowd)
        units.append((crowds, idx[rep], noise_slots))
        cols[row_model == m] = sub_cols
    return units, row_model, cols


def _checked_slot_samples(who: str, slot_samples, num_samples: int):
    """``slot_samples`` of a sample source as an int64 array (None stays None): one count in 1 .. num_samples per slot."""
    if slot_samples is None:
        return None
    counts = np.asarray(slot_samples)
    if counts.ndim != 1 or not np.issubdtype(counts.dtype, np.integer):
        raise ValueError(f"{who}: slot_samples holds one integer sample count per slot")
    counts = counts.astype(np.int64)
    if len(counts) and not 1 <= counts.min() <= counts.max() <= int(num_samples):
        raise ValueError(f"{who}: slot_samples holds one count in 1 .. {int(num_samples)} (num_samples) per slot")
    return counts


class SganSampler:
    """The multi-sample predictor in front of the planner, in the library: ``sample(obs, ped_off)`` gives the raw samples
    [S, pred_len, sum P, 2] of every scene as a float32 ``torch`` device tensor -- what ``fot_loop_frame.dist_raw`` and
    ``resample_device`` read.  A ``sample_source`` of ``BatchedClosedLoop`` (``needs_history``: it is handed the observer's
    whole window).  The noise is drawn on the device from the sampler's own ``torch.Generator`` (``noise_type`` 'gaussian':
    ``randn``; 'uniform': ``rand`` mapped to [-1, 1), models.py:27-32) or supplied.  ``noise_type`` is the loaded weights' own
    (the checkpoint's, as the reference draws: models.py:393) unless the constructor is given one; ``last_noise`` /
    ``last_obs`` / ``last_ped_off`` keep what the most recent call used.

    counter_seed: the counter mode.  The noise is then the library's own (``fot_sgan_noise``: Philox4x32-10 keyed by the
    seed, counted by slot, that slot's step, pedestrian, sample and dimension), not torch's stream -- a row's numbers do
    not depend on which other episodes still run, and ``BatchedClosedLoop(..., resident=True)`` draws the same inside
    the library.  ``sample`` then needs the rows' ``slots`` and ``steps`` (a loop passes them).  The numbers differ from
    ``torch.randn``'s: seeds are not comparable with the reference's runs.
    slot_crowd (with ``counter_seed``): the loop's slots share crowds -- the K conditions of a sweep over one crowd.  One
    crowd id >= 0 per slot; the slots of a crowd replay the same pedestrians.  Every crowd with a running slot is sampled
    ONCE per lock step, its noise keyed by the crowd's id in place of the slot, and all its slots are handed those samples
    (``fot_loop_set_sampler_shared`` in a resident loop; ``sample`` forms the same bytes for a stepwise one).  Crowd c
    draws what slot c of a loop without ``slot_crowd`` draws.
    weights a sequence ``[w0, w1, ...]`` (with ``counter_seed``, ``slot_crowd`` and ``slot_model``): the handle holds several
    models (``fot_sgan_load_model``) and slot e predicts with model ``slot_model[e]`` -- the 'sgan' and 'lstm' conditions of a
    campaign cell in one loop.  Every active (crowd, model) pair is sampled once per lock step, the noise keyed by the
    crowd's id with the model's own dimensions, mix type and ``noise_type`` (``fot_loop_set_sampler_models``; ``sample``
    forms the same bytes through ``fot_sgan_sample_model``): a slot's numbers are those of the loop that holds only its model.
    engine None: the sampler joins the engine of the loop it is handed to (``bind``).
    sample_capacity: more than 64 samples, up to ``_abi.MAX_PLAN_SAMPLES`` (254) -- the engine it runs on needs that
    capacity too (``BatchPlanner(sample_capacity=)``, ``BatchedClosedLoop(sample_capacity=)``).
    slot_samples (with ``counter_seed``): one count in 1 .. ``num_samples`` per slot of a sweep loop -- slot e plans against,
    and is scored on, the FIRST ``slot_samples[e]`` samples of its crowd's draw (``fot_loop_set_slot_samples``): the
    sample-count ablation as slots of one loop.  ``sample`` still hands over all ``num_samples`` samples; the library takes
    each slot's prefix."""
    needs_history = True

    def __init__(self, engine: Optional[BatchPlanner], weights: SganWeights, num_samples: int, seed: Optional[int] = None,
                 noise_type: Optional[str] = None, counter_seed: Optional[int] = None, slot_crowd=None, slot_model=None,
                 sample_capacity: int = _abi.MAX_SAMPLES, slot_samples=None):
        if noise_type is not None and noise_type not in _NOISE_TYPES:
            raise ValueError(f'Unrecognized noise type "{noise_type}"')
        self.sample_capacity = _checked_capacity("SganSampler", sample_capacity)
        if not 1 <= int(num_samples) <= self.sample_capacity:
            raise ValueError(f"SganSampler: 1 <= num_samples <= {self.sample_capacity}")
        self.models = None if isinstance(weights, SganWeights) else list(weights)
        if self.models is not None:
            if not 1 <= len(self.models) <= int(_abi.lib().fot_sgan_max_models()):
                raise ValueError(f"SganSampler: 1 .. {int(_abi.lib().fot_sgan_max_models())} models")
            if counter_seed is None or slot_crowd is None or slot_model is None:
                raise ValueError("SganSampler: several models need counter_seed, slot_crowd and slot_model")
            if noise_type is not None:
                raise ValueError("SganSampler: with several models noise_type is each model's own (SganWeights.noise_type)")
            for w in self.models:
                if w.noise_type not in _NOISE_TYPES:
                    raise ValueError(f'Unrecognized noise type "{w.noise_type}"')
                if (w.desc.obs_len, w.desc.pred_len) != (self.models[0].desc.obs_len, self.models[0].desc.pred_len):
                    raise ValueError("SganSampler: the models of one loop share obs_len and pred_len")
            weights = self.models[0]
        elif slot_model is not None:
            raise ValueError("SganSampler: slot_model names one of several models: weights is then a sequence")
        self.engine, self.weights, self.num_samples, self._noise_type = None, weights, int(num_samples), noise_type
        self.counter_seed = None if counter_seed is None else int(counter_seed) & 0xFFFFFFFFFFFFFFFF
        if slot_crowd is not None and counter_seed is None:
            raise ValueError("SganSampler: slot_crowd keys the counter mode's noise by crowd: it needs counter_seed")
        self.slot_crowd = None if slot_crowd is None else np.asarray(slot_crowd, dtype=np.int64).reshape(-1)
        if self.slot_crowd is not None and len(self.slot_crowd) and self.slot_crowd.min() < 0:
            raise ValueError("SganSampler: slot_crowd holds one crowd id >= 0 per slot")
        self.slot_model = None if slot_model is None else np.asarray(slot_model, dtype=np.int64).reshape(-1)
        if self.slot_model is not None:
            if len(self.slot_model) != len(self.slot_crowd):
                raise ValueError("SganSampler: slot_model and slot_crowd hold one entry per slot")
            if len(self.slot_model) and not 0 <= self.slot_model.min() <= self.slot_model.max() < len(self.models):
                raise ValueError(f"SganSampler: slot_model holds one model id in 0 .. {len(self.models) - 1} per slot")
        self.slot_samples = _checked_slot_samples("SganSampler", slot_samples, self.num_samples)
        if self.slot_samples is not None and self.counter_seed is None:
            raise ValueError("SganSampler: slot_samples takes every slot's first samples of one draw: it needs counter_seed "
                             "(the counter noise is keyed by the sample index)")
        if self.slot_samples is not None and self.slot_crowd is not None and len(self.slot_samples) != len(self.slot_crowd):
            raise ValueError("SganSampler: slot_samples and slot_crowd hold one entry per slot")
        self._seed = seed
        self._lib = _abi.lib()
        self.device = self.generator = None
        self.last_noise = self.last_obs = self.last_ped_off = None
        if self._noise_type is None and weights.noise_type not in _NOISE_TYPES:
            raise ValueError(f'Unrecognized noise type "{weights.noise_type}"')
        if engine is not None:
            self.bind(engine)

    def bind(self, engine: BatchPlanner) -> None:
        """Join ``engine``: its handle gets the model, its device the generator."""
        import torch
        if self.engine is not None and self.engine is not engine:
            raise ValueError("SganSampler: the sampler already belongs to another engine")
        if self.engine is engine:
            return
        self.engine = engine
        if self.models is None:
            self.load(self.weights)
        for m, w in enumerate(self.models or ()):
            _abi.check(engine._h, self._lib.fot_sgan_load_model(engine._h, m, C.byref(w.desc), w.blob.size, w.blob.ctypes.data))
        dev = int(getattr(engine, "device", -1))                    # (fot_create's device < 0: the current one)
        self.device = torch.device("cuda", torch.cuda.current_device() if dev < 0 else dev)
        self.generator = torch.Generator(device=self.device)
        if self._seed is not None:
            self.generator.manual_seed(int(self._seed))

    @property
    def noise_type(self) -> str:
        return self._noise_type if self._noise_type is not None else self.weights.noise_type

    def load(self, weights: SganWeights) -> None:
        """Replace the handle's model."""
        if self.models is not None:
            raise ValueError("SganSampler: a sampler of several models loads them when it joins its engine")
        if self._noise_type is None and weights.noise_type not in _NOISE_TYPES:
            raise ValueError(f'Unrecognized noise type "{weights.noise_type}"')
        _abi.check(self.engine._h, self._lib.fot_sgan_load(self.engine._h, C.byref(weights.desc), weights.blob.size,
                                                           weights.blob.ctypes.data))
        self.weights = weights

    def draw_noise(self, n_rows: int, n_scenes: int):
        import torch
        d = self.weights.desc
        rows = n_scenes if d.noise_mix_type == _abi.SGAN_NOISE_GLOBAL else n_rows
        shape = (self.num_samples, rows, d.noise_dim)
        if self.noise_type == "gaussian":
            return torch.randn(shape, device=self.device, dtype=torch.float32, generator=self.generator)
        return torch.rand(shape, device=self.device, dtype=torch.float32, generator=self.generator).sub_(0.5).mul_(2.0)

    @property
    def noise_kind(self) -> int:
        """The ``fot_sgan_noise`` kind that stands for ``noise_type``."""
        return _abi.NOISE_GAUSSIAN if self.noise_type == "gaussian" else _abi.NOISE_UNIFORM_SYM

    @property
    def model_kinds(self):
        """Several models: the ``fot_sgan_noise`` kind of every model's own ``noise_type``; otherwise None."""
        if self.models is None:
            return None
        return [_abi.NOISE_GAUSSIAN if w.noise_type == "gaussian" else _abi.NOISE_UNIFORM_SYM for w in self.models]

    def _desc(self, model):
        return self.weights.desc if model is None else self.models[model].desc

    def counter_noise(self, slots, steps, counts, kind: Optional[int] = None, model: Optional[int] = None):
        """The counter mode's noise of the scenes ``slots`` (pedestrian counts ``counts``) at their step counts ``steps``,
        from ``fot_sgan_noise`` as a device tensor [S, rows, noise_dim] -- exactly what a resident loop with this seed
        uses for those slots at those steps, whatever else runs beside them.  model: of several models, the one whose
        dimensions, mix type and kind apply (``slots`` are then crowd ids)."""
        import torch
        if self.counter_seed is None:
            raise ValueError("SganSampler: counter_noise needs counter_seed")
        d = self._desc(model)
        if kind is None:
            kind = self.noise_kind if model is None else self.model_kinds[model]
        slots, steps, counts = (np.asarray(v, dtype=np.int64).reshape(-1) for v in (slots, steps, counts))
        if not len(slots) == len(steps) == len(counts):
            raise ValueError("SganSampler: one step and one pedestrian count per slot")
        if d.noise_mix_type == _abi.SGAN_NOISE_GLOBAL:
            row_slot, row_step, row_idx = slots, steps, np.zeros(len(slots), np.int64)
        else:
            row_slot, row_step = np.repeat(slots, counts), np.repeat(steps, counts)
            row_idx = np.concatenate([np.arange(c) for c in counts]) if len(counts) else np.zeros(0, np.int64)
        dtype = torch.int32 if kind == _abi.NOISE_RAW else torch.float32    # (raw words: their bits, as int32)
        out = torch.empty((self.num_samples, len(row_slot), d.noise_dim), device=self.device, dtype=dtype)
        torch.cuda.current_stream(self.device).synchronize()        # (the library writes it on its own stream)
        return self.engine.sgan_noise(self.counter_seed, kind, self.num_samples,
                                      d.noise_dim, row_slot, row_step, row_idx, out=out)

    def sample(self, obs, ped_off, noise=None, slots=None, steps=None, model: Optional[int] = None):
        """obs [obs_len, sum P, 2] absolute positions (NumPy, or a float32 torch device tensor); ped_off [n_scenes + 1];
        slots / steps (counter mode, without ``noise``): the slot and step count of every scene.  model (several models,
        with ``noise``): the scenes go through that model alone, ``fot_sgan_sample_model``."""
        import torch
        if self.models is not None and (noise is None) != (model is None):
            raise ValueError("SganSampler: several models sample by slots and steps, or one `model` under a given `noise`")
        if self.models is None and model is not None:
            raise ValueError("SganSampler: `model` names one of several models")
        d = self._desc(model)
        off = np.ascontiguousarray(ped_off, dtype=np.int32)
        n_scenes, n = len(off) - 1, int(off[-1])
        if hasattr(obs, "data_ptr"):
            obs_t = obs.to(device=self.device, dtype=torch.float32).contiguous()
        else:
            obs_t = torch.from_numpy(np.ascontiguousarray(obs, dtype=np.float32)).to(self.device)
        if tuple(obs_t.shape) != (d.obs_len, n, 2):
            raise ValueError(f"SganSampler: obs is [obs_len = {d.obs_len}, sum P = {n}, 2], got {tuple(obs_t.shape)}")
        if noise is None and self.models is not None:
            # one sampling per active (crowd, model) unit, model by model in ascending id, then every asked slot's columns
            # out of its model's tensor -- the bytes a resident loop forms (fot_loop_set_sampler_models)
            if slots is None or steps is None:
                raise ValueError("SganSampler: the counter mode needs every scene's slot and step count (slots, steps)")
            counts = np.diff(off).astype(np.int64)
            steps = np.asarray(steps, dtype=np.int64).reshape(-1)
            slots = np.asarray(slots, dtype=np.int64).reshape(-1)
            units, row_model, cols = model_scenes(slots, counts, steps, self.slot_crowd, self.slot_model)
            out = torch.empty((self.num_samples, d.pred_len, n, 2), device=self.device, dtype=torch.float32)
            for m, (crowds, rep, noise_slots) in enumerate(units):
                rep_of = dict(zip(crowds.tolist(), rep.tolist()))
                for i in np.flatnonzero(self.slot_model[slots] == m).tolist():
                    j = rep_of.get(int(self.slot_crowd[slots[i]]), i)
                    if counts[i] > 0 and j != i and not torch.equal(obs_t[:, off[i]:off[i + 1]], obs_t[:, off[j]:off[j + 1]]):
                        raise ValueError(f"SganSampler: the slots of crowd {int(self.slot_crowd[slots[i]])} do not observe the "
                                         f"same window (scenes {j} and {i})")
                if len(rep) == 0:                                     # (no active unit: the model is not called)
                    continue
                rows = np.concatenate([np.arange(off[j], off[j + 1]) for j in rep]).astype(np.int64)
                rep_obs = obs_t.index_select(1, torch.as_tensor(rows, device=self.device)).contiguous()
                rep_off = np.concatenate([[0], np.cumsum(counts[rep])]).astype(np.int32)
                raw = self._sample_scenes(rep_obs, rep_off, self.counter_noise(noise_slots, steps[rep], counts[rep], model=m), model=m)
                mine = np.flatnonzero(row_model == m)
                out[:, :, torch.as_tensor(mine, device=self.device)] = raw.index_select(2, torch.as_tensor(cols[mine], device=self.device))
            return out
        if noise is None and self.slot_crowd is not None:
            # one sampling per active crowd: its representative's window under the crowd's noise, then every asked slot's
            # columns out of the crowds' tensor -- the bytes a resident loop forms (fot_loop_set_sampler_shared)
            if slots is None or steps is None:
                raise ValueError("SganSampler: the counter mode needs every scene's slot and step count (slots, steps)")
            counts = np.diff(off).astype(np.int64)
            steps = np.asarray(steps, dtype=np.int64).reshape(-1)
            crowds, rep, noise_slots, cols = crowd_scenes(slots, counts, steps, self.slot_crowd)
            crowd_of = self.slot_crowd[np.asarray(slots, dtype=np.int64).reshape(-1)]
            rep_of = dict(zip(crowds.tolist(), rep.tolist()))
            for i, c in enumerate(crowd_of.tolist()):
                j = rep_of.get(c, i)
                if counts[i] > 0 and j != i and not torch.equal(obs_t[:, off[i]:off[i + 1]], obs_t[:, off[j]:off[j + 1]]):
                    raise ValueError(f"SganSampler: the slots of crowd {c} do not observe the same window (scenes {j} and {i})")
            if len(rep) == 0:                                         # (no running slot has pedestrians)
                return torch.empty((self.num_samples, d.pred_len, 0, 2), device=self.device, dtype=torch.float32)
            rows = np.concatenate([np.arange(off[j], off[j + 1]) for j in rep] + [np.zeros(0, np.int64)]).astype(np.int64)
            rep_obs = obs_t.index_select(1, torch.as_tensor(rows, device=self.device)).contiguous()
            rep_off = np.concatenate([[0], np.cumsum(counts[rep])]).astype(np.int32)
            raw = self._sample_scenes(rep_obs, rep_off, self.counter_noise(noise_slots, steps[rep], counts[rep]))
            return raw.index_select(2, torch.as_tensor(cols, device=self.device)).contiguous()
        if noise is None and self.counter_seed is not None:
            if slots is None or steps is None:
                raise ValueError("SganSampler: the counter mode needs every scene's slot and step count (slots, steps)")
            noise_t = self.counter_noise(slots, steps, np.diff(off))
        elif noise is None:
            noise_t = self.draw_noise(n, n_scenes)
        else:
            noise_t = torch.as_tensor(noise, dtype=torch.float32).to(self.device).contiguous()
            rows = n_scenes if d.noise_mix_type == _abi.SGAN_NOISE_GLOBAL else n
            if tuple(noise_t.shape) != (self.num_samples, rows, d.noise_dim):
                raise ValueError(f"SganSampler: noise is [S, rows, noise_dim] = {(self.num_samples, rows, d.noise_dim)}")
        return self._sample_scenes(obs_t, off, noise_t, model=model)

    def _sample_scenes(self, obs_t, off, noise_t, model: Optional[int] = None):
        """``fot_sgan_sample`` (``fot_sgan_sample_model`` of ``model``) of the scenes ``off`` on device tensors."""
        import torch
        d = self._desc(model)
        n_scenes, n = len(off) - 1, int(off[-1])
        out = torch.empty((self.num_samples, d.pred_len, n, 2), device=self.device, dtype=torch.float32)
        torch.cuda.current_stream(self.device).synchronize()        # (the library reads the tensors on its own stream)
        args = (n_scenes, off.ctypes.data, C.c_void_p(obs_t.data_ptr()), self.num_samples,
                C.c_void_p(noise_t.data_ptr()) if noise_t.numel() else None,
                _abi.OUT_DEVICE | _abi.SGAN_OBS_DEVICE | _abi.SGAN_NOISE_DEVICE, C.c_void_p(out.data_ptr()), None)
        if model is None:
            _abi.check(self.engine._h, self._lib.fot_sgan_sample(self.engine._h, *args))
        else:
            _abi.check(self.engine._h, self._lib.fot_sgan_sample_model(self.engine._h, int(model), *args))
        self.last_noise, self.last_obs, self.last_ped_off = noise_t, obs_t, off
        return out

    __call__ = sample


# ---- open-loop prediction evaluation of a recorded scene (fot_openloop_eval) ---------------------------------------------------
class WindowTable(NamedTuple):
    """The fixed-population windows of a scene as ``fot_openloop_eval`` reads them: window w covers ``seq_len`` frames from
    ``win_frame0[w]`` on and the scene columns ``row_col[ped_off[w]:ped_off[w + 1]]``."""
    win_frame0: np.ndarray
    ped_off: np.ndarray
    row_col: np.ndarray

    @property
    def n_windows(self) -> int:
        return len(self.win_frame0)

    def window(self, scene_xy, w: int, seq_len: int) -> np.ndarray:
        """Window w as the reference's ``extract_fixed_windows`` returns it: [seq_len, N, 2] float64."""
        cols = self.row_col[self.ped_off[w]:self.ped_off[w + 1]]
        f0 = int(self.win_frame0[w])
        return np.asarray(scene_xy)[f0:f0 + int(seq_len)][:, cols].astype(np.float64)


def fixed_windows(scene_xy, seq_len: int, stride: int = 1, min_peds: int = 1, max_windows: Optional[int] = None) -> WindowTable:
    """``extract_fixed_windows`` (reference src/datasets/eth_ucy_loader.py:154-182) on a dense scene: scene_xy [F, ids, 2]
    with NaN where a pedestrian is absent, the columns in ascending id order.  Every start 0, stride, .. <= F - seq_len
    whose window has at least ``min_peds`` pedestrians present in ALL its frames is a window of exactly those pedestrians,
    in column order; ``max_windows`` keeps the first ones.  Vectorised: one cumulative sum over the frames."""
    if int(seq_len) <= 0:
        raise ValueError("seq_len must be positive")
    if int(stride) <= 0:
        raise ValueError("stride must be positive")
    xy = np.asarray(scene_xy)
    if xy.ndim != 3 or xy.shape[2] != 2:
        raise ValueError(f"fixed_windows: a scene is [n_frames, n_ids, 2], got {xy.shape}")
    F, n_ids = xy.shape[0], xy.shape[1]
    starts = np.arange(0, F - int(seq_len) + 1, int(stride), dtype=np.int64)
    present = ~np.isnan(xy).any(axis=2)                               # [F, ids]
    run = np.concatenate([np.zeros((1, n_ids), np.int64), np.cumsum(present, axis=0, dtype=np.int64)])
    full = (run[starts + int(seq_len)] - run[starts]) == int(seq_len) if len(starts) else np.zeros((0, n_ids), bool)
    counts = full.sum(axis=1)
    keep = counts >= int(min_peds)
    if max_windows is not None:
        keep &= np.cumsum(keep) <= int(max_windows)
    w_idx, cols = np.nonzero(full[keep])                              # (row-major: window by window, ascending columns)
    ped_off = np.concatenate([[0], np.cumsum(counts[keep])]).astype(np.int32)
    return WindowTable(starts[keep].astype(np.int32), ped_off, cols.astype(np.int32))


OPEN_LOOP_CSV_COLUMNS = ("scene", "method", "seed", "num_samples", "n_windows", "n_trajectories", "ade", "fde", "ade_per_agent",
                         "fde_per_agent", "nll")                     # the reference's header (run_openloop_prediction.py:216-217)
_OPEN_LOOP_POOLING = {"lstm": _abi.SGAN_POOL_NONE, "sgan": _abi.SGAN_POOL_NET}


def open_loop_result(totals) -> dict:
    """``evaluate_scene``'s result dictionary from the totals of ``fot_openloop_eval`` (run_openloop_prediction.py:143-151):
    NaN where nothing was counted."""
    nan = float("nan")
    n, n_nll = int(totals.traj_count), int(totals.nll_count)
    return {"n_windows": int(totals.n_windows), "n_trajectories": n,
            "ade": totals.sum_ade / n if n else nan, "fde": totals.sum_fde / n if n else nan,
            "ade_per_agent": totals.sum_ade_agent / n if n else nan, "fde_per_agent": totals.sum_fde_agent / n if n else nan,
            "nll": totals.sum_nll / n_nll if n_nll else nan}


def evaluate_open_loop(engine: BatchPlanner, scene_xy, obs_len: int, pred_len: int, dt: float, method: str,
                       weights_or_model=None, num_samples: int = 20, seed: int = 0, stride: int = 1, min_peds: int = 1,
                       max_windows: Optional[int] = None, windows: Optional[WindowTable] = None, noise=None,
                       noise_kind: Optional[int] = None, win_id0: int = 0, max_rows: int = 0, model_slot: int = 0,
                       records: bool = False, raw: bool = False) -> dict:
    """The reference's open-loop prediction evaluation of a scene (examples/run_openloop_prediction.py: ``evaluate_scene``
    over ``extract_fixed_windows``, RQ1a) in one library call, ``fot_openloop_eval``.

    scene_xy [F, ids, 2]: NaN where a pedestrian is absent (a NumPy array; with ``windows`` given also a CUDA tensor, used
    where it lies).  method 'cv' (one sample, ``num_samples`` ignored as in the reference's script), 'lstm' (a generator
    without pooling) or 'sgan' (pool net); weights_or_model: ``SganWeights`` -- loaded into ``model_slot`` --, or the slot of
    a model that is loaded already (``noise_kind`` then says how it draws; default Gaussian).  The no-pooling and the pooled
    model of a scene live side by side in two slots and evaluate the same ``windows`` in two calls.  noise: None -- the
    library's counter noise of ``seed`` (``fot_sgan_noise``; window w's slot word is ``win_id0 + w``) --, or the tensor
    [S, rows, noise_dim].  Returns ``n_windows, n_trajectories, ade, fde, ade_per_agent, fde_per_agent, nll`` as the
    reference does (NaN where it gives NaN); with ``records`` / ``raw`` also ``records`` (one ``PRED_SCORE_DT`` per window)
    and ``windows`` / ``raw`` (the generator's raw samples)."""
    method = str(method).lower()
    if method not in ("cv", "lstm", "sgan"):
        raise ValueError(f"Invalid method '{method}'. Must be one of ['cv', 'lstm', 'sgan']")
    if windows is None:
        windows = fixed_windows(scene_xy, int(obs_len) + int(pred_len), stride=stride, min_peds=min_peds, max_windows=max_windows)
    lib = _abi.lib()
    if method == "cv":
        code, model, S = _abi.OPENLOOP_CV, 0, 1
    else:
        code, S = _abi.OPENLOOP_SGAN, int(num_samples)
        if isinstance(weights_or_model, SganWeights):
            w = weights_or_model
            if w.desc.pooling_type != _OPEN_LOOP_POOLING[method]:     # trajectory_predictor.py:114-121
                raise ValueError(f"method='{method}' requires a {'no-pooling' if method == 'lstm' else 'pool_net'} generator")
            if noise is None and noise_kind is None:
                if w.noise_type not in _NOISE_TYPES:
                    raise ValueError(f'Unrecognized noise type "{w.noise_type}"')
                noise_kind = _abi.NOISE_GAUSSIAN if w.noise_type == "gaussian" else _abi.NOISE_UNIFORM_SYM
            model = int(model_slot)
            _abi.check(engine._h, lib.fot_sgan_load_model(engine._h, model, C.byref(w.desc), w.blob.size, w.blob.ctypes.data))
        elif weights_or_model is None:
            raise ValueError(f"method='{method}' needs SganWeights or the slot of a loaded model")
        else:
            model = int(weights_or_model)
    totals, rec, raw_out = engine.openloop_eval(
        scene_xy, windows.win_frame0, windows.ped_off, windows.row_col, obs_len, pred_len, dt, code, model=model, num_samples=S,
        noise=noise, seed=seed, noise_kind=_abi.NOISE_GAUSSIAN if noise_kind is None else int(noise_kind), win_id0=win_id0,
        max_rows=max_rows, want_records=records, want_raw=raw and method != "cv")
    out = open_loop_result(totals)
    if records:
        out["records"], out["windows"] = rec, windows
    if raw:
        out["raw"] = raw_out
    return out


def append_open_loop_csv(path, scene: str, method: str, seed: int, num_samples: int, result: dict) -> None:
    """Append a result row under the reference's CSV header (run_openloop_prediction.py:213-229): the header goes in when
    the file is absent or empty."""
    import os
    parent = os.path.dirname(os.path.abspath(path))
    os.makedirs(parent, exist_ok=True)
    need_header = not os.path.exists(path) or os.path.getsize(path) == 0
    with open(path, "a") as f:
        if need_header:
            f.write(",".join(OPEN_LOOP_CSV_COLUMNS) + "\n")
        f.write(f"{scene},{method},{seed},{num_samples},{result['n_windows']},{result['n_trajectories']},{result['ade']},"
                f"{result['fde']},{result['ade_per_agent']},{result['fde_per_agent']},{result['nll']}\n")


class RecordedSamples:
    """A multi-sample predictor's output for a whole run, recorded once: ``samples`` ``[n_steps, S, pred_len, sum P, 2]``
    (float32 or float64; a NumPy array or a CUDA ``torch`` tensor), row r the raw samples of lock step ``first_step + r``
    for the pedestrians of ALL episodes in the loop's order.  With replayed pedestrians the observer's window does not
    depend on the ego, so a recording stays exact for every planner configuration run over the same tracks -- the
    reference's own generator under its seed, an LSTM or a scripted source is called once per step of ONE recording run
    (``record_samples``) and every condition of a sweep replays it.

    A ``sample_source`` of ``BatchedClosedLoop``: with ``resident=True`` (and ``device_samples=True``) the tensor goes to
    the library once (``fot_loop_set_samples``; a CUDA tensor is used in place) and the whole run stays there; without, the
    loop calls the object every step with the running episodes' ``slots`` and ``steps`` and gets the step's row cut to
    their columns -- a device tensor with ``device_samples=True``, a host array otherwise.  Rows of steps at which the
    observer is not ready are never read.

    slot_col0: the recording's columns are not the loop's -- pedestrian p of slot e reads column ``slot_col0[e] + p``, and
    several slots may name the same columns: the K conditions of a sweep over one crowd share ONE copy of its samples
    (``fot_loop_set_samples_shared``).  The stepwise call cuts its rows through the same map.
    sample_capacity: more than 64 samples per step, up to ``_abi.MAX_PLAN_SAMPLES`` (254); the loop's engine needs that
    capacity too (``BatchedClosedLoop(sample_capacity=)``).
    slot_samples: one count in 1 .. S per slot of a sweep loop -- slot e plans against, and is scored on, the FIRST
    ``slot_samples[e]`` samples of its columns (``fot_loop_set_slot_samples``): the sample-count ablation over ONE recording.
    The stepwise call still hands over all S samples; the library takes each slot's prefix."""
    needs_history = True
    recorded = True

    def __init__(self, samples, first_step: int = 0, slot_col0=None, sample_capacity: int = _abi.MAX_SAMPLES, slot_samples=None):
        self.sample_capacity = _checked_capacity("RecordedSamples", sample_capacity)
        on_device = hasattr(samples, "data_ptr")
        if on_device:
            import torch
            if samples.dtype not in (torch.float32, torch.float64):
                raise ValueError(f"RecordedSamples: float32 or float64 samples, got {samples.dtype}")
            if not samples.is_cuda:
                samples = samples.detach().cpu().numpy()
                on_device = False
        if not on_device:
            samples = np.asarray(samples)
            if samples.dtype not in (np.float32, np.float64):
                raise ValueError(f"RecordedSamples: float32 or float64 samples, got {samples.dtype}")
        if samples.ndim != 5 or samples.shape[-1] != 2:
            raise ValueError(f"RecordedSamples: samples are [n_steps, S, pred_len, sum P, 2], got {tuple(samples.shape)}")
        if samples.shape[0] < 1 or not 1 <= samples.shape[1] <= self.sample_capacity:
            raise ValueError(f"RecordedSamples: n_steps >= 1 and 1 <= S <= {self.sample_capacity}, got {tuple(samples.shape)}")
        if int(first_step) < 0:
            raise ValueError("RecordedSamples: first_step >= 0")
        self.samples = samples.contiguous() if on_device else np.ascontiguousarray(samples)
        self.first_step = int(first_step)
        self.n_steps, self.num_samples, self.pred_len, self.n_cols = (int(v) for v in samples.shape[:4])
        self.ped_off = None                                            # every slot's pedestrian offsets, once a loop is known
        self.slot_col0 = None if slot_col0 is None else np.asarray(slot_col0, dtype=np.int64).reshape(-1)
        self.slot_samples = _checked_slot_samples("RecordedSamples", slot_samples, self.num_samples)
        self.device_out = on_device                                    # what a stepwise call returns (attach decides)
        self._dev, self._host, self._cols_key, self._cols = None, None, None, None

    def attach(self, ped_off, pred_len: int, device_samples: Optional[bool] = None) -> None:
        """Join a loop: its episodes' pedestrian offsets and the configuration's ``pred_len`` must be the recording's."""
        off = np.asarray(ped_off, dtype=np.int64)
        if self.slot_samples is not None and len(self.slot_samples) != len(off) - 1:
            raise ValueError(f"RecordedSamples: slot_samples names {len(self.slot_samples)} slots, the loop has {len(off) - 1}")
        if self.slot_col0 is not None:                                # every slot's own column range, not the sum
            if len(self.slot_col0) != len(off) - 1:
                raise ValueError(f"RecordedSamples: slot_col0 names {len(self.slot_col0)} slots, the loop has {len(off) - 1}")
            for e, c0 in enumerate(self.slot_col0):
                if c0 < 0 or c0 + (off[e + 1] - off[e]) > self.n_cols:
                    raise ValueError(f"RecordedSamples: slot {e} reads columns {int(c0)} .. {int(c0 + off[e + 1] - off[e]) - 1}, "
                                     f"the recording has {self.n_cols} pedestrian columns")
        elif int(off[-1]) != self.n_cols:
            raise ValueError(f"RecordedSamples: the recording has {self.n_cols} pedestrian columns, the tracks {int(off[-1])}")
        if int(pred_len) != self.pred_len:
            raise ValueError(f"RecordedSamples: the recording has pred_len = {self.pred_len}, the configuration {int(pred_len)}")
        self.ped_off = off
        if device_samples is not None:
            self.device_out = bool(device_samples)

    def _columns(self, slots) -> Optional[np.ndarray]:
        """Columns of the episodes ``slots`` (None: all of them, as they lie)."""
        if self.ped_off is None:
            raise ValueError("RecordedSamples: not attached to a loop's tracks yet (attach)")
        slots = np.asarray(slots, dtype=np.int64).reshape(-1)
        if self.slot_col0 is None and len(slots) == len(self.ped_off) - 1 and np.array_equal(slots, np.arange(len(slots))):
            return None
        key = slots.tobytes()
        if key != self._cols_key:
            self._cols_key = key
            col0 = self.ped_off if self.slot_col0 is None else self.slot_col0
            self._cols = (np.concatenate([col0[e] + np.arange(self.ped_off[e + 1] - self.ped_off[e]) for e in slots])
                          if len(slots) else np.zeros(0, np.int64)).astype(np.int64)
        return self._cols

    def sample(self, obs=None, ped_off=None, slots=None, steps=None):
        """The raw samples [S, pred_len, rows, 2] of the lock step ``steps`` (one value: the episodes run in lock step) for
        the pedestrians of the episodes ``slots``; ``obs`` is not looked at, ``ped_off`` (the frame's offsets) only
        checked."""
        if slots is None or steps is None:
            raise ValueError("RecordedSamples: a recording is read by lock step: pass every running episode's slot and "
                             "step count (slots, steps)")
        steps = np.asarray(steps, dtype=np.int64).reshape(-1)
        if len(steps) == 0 or np.any(steps != steps[0]):
            raise ValueError("RecordedSamples: the running episodes are at one and the same lock step")
        r = int(steps[0]) - self.first_step
        if not 0 <= r < self.n_steps:
            raise IndexError(f"RecordedSamples: lock step {int(steps[0])} predicts, but the recording covers steps "
                             f"{self.first_step} .. {self.first_step + self.n_steps - 1}")
        cols = self._columns(slots)
        n = self.n_cols if cols is None else len(cols)
        if ped_off is not None and int(np.asarray(ped_off)[-1]) != n:
            raise ValueError(f"RecordedSamples: the frame has {int(np.asarray(ped_off)[-1])} pedestrians, the slots' columns {n}")
        stored_on_device = hasattr(self.samples, "data_ptr")
        if self.device_out:
            import torch
            if not stored_on_device and self._dev is None:             # a host recording: uploaded once
                self._dev = torch.from_numpy(self.samples).cuda()
            row = (self.samples if stored_on_device else self._dev)[r]
            if cols is None:
                return row
            return row.index_select(2, torch.as_tensor(cols, device=row.device)).contiguous()
        if stored_on_device and self._host is None:                    # a device recording: fetched once
            self._host = self.samples.detach().cpu().numpy()
        row = (self._host if stored_on_device else self.samples)[r]
        return row if cols is None else np.ascontiguousarray(row[:, :, cols])

    __call__ = sample


def record_samples(config, ped_tracks, sample_source, n_steps: int, dtype=np.float32, device=None,
                   warmup_frames: Optional[int] = None, sample_capacity: Optional[int] = None) -> RecordedSamples:
    """Run the closed loop's observer clock over the replayed tracks -- no ego, no planning -- and record what
    ``sample_source`` predicts at every lock step: the warm-up of ``int(obs_len * sgan_dt / dt)`` frames, then ``n_steps``
    steps; at every step where the observer is ready the source is called for the pedestrians of ALL episodes, as a
    stepwise ``BatchedClosedLoop`` calls it (``(obs_last, obs_prev)``, or the window and the offsets for a
    ``needs_history`` source; ``slots`` / ``steps`` for a counter-seeded one).  Steps before that stay NaN: they are never
    read.  dtype: float32 or float64; device: None -- a host array, else the ``torch`` device the recording is kept on;
    warmup_frames: for a caller of ``fot_loop_set_replay`` with a warm-up of its own (None: the loop's).
    sample_capacity: the recording's (``RecordedSamples(sample_capacity=)``); None: the capacity of the source's engine
    where it has one, else the source's own ``sample_capacity``, else 64."""
    from .closed_loop import Observer, ReplayPedestrians, _Cfg
    if sample_capacity is None:
        sample_capacity = getattr(getattr(sample_source, "engine", None), "sample_capacity", None)
    if sample_capacity is None:
        sample_capacity = getattr(sample_source, "sample_capacity", _abi.MAX_SAMPLES)
    c = _Cfg(config) if isinstance(config, dict) else config
    dtype = np.dtype(dtype)
    if dtype not in (np.dtype(np.float32), np.dtype(np.float64)):
        raise ValueError("record_samples: float32 or float64")
    sgan_dt, dt = 0.4, float(c.dt)                                    # integrated_simulator.py:323-327
    peds = [ReplayPedestrians(tr, dt) for tr in ped_tracks]
    off = np.concatenate([[0], np.cumsum([p.n_peds for p in peds])]).astype(np.int64)
    t_max = max((p.n_frames for p in peds), default=0)
    tracks = np.zeros((t_max, int(off[-1]), 2))                       # (a shorter replay holds its last frame)
    for e, p in enumerate(peds):
        tracks[: p.n_frames, off[e]:off[e + 1]] = p.trajectories
        tracks[p.n_frames:, off[e]:off[e + 1]] = p.trajectories[-1]
    observer = Observer(c.obs_len, dt, sgan_dt)
    frame, ped_time = 0, 0.0

    def advance():
        nonlocal frame, ped_time
        frame += 1
        ped_time += dt
        observer.update(tracks[min(frame, t_max - 1)], ped_time)

    for _ in range(int(c.obs_len * sgan_dt / dt) if warmup_frames is None else int(warmup_frames)):   # integrated_simulator.py:406-422
        advance()
    n, out = len(peds), None
    every, off32 = np.arange(n), off.astype(np.int32)
    keyed = getattr(sample_source, "counter_seed", None) is not None or getattr(sample_source, "recorded", False)
    for k in range(int(n_steps)):
        advance()
        if not observer.is_ready:
            continue
        hist = observer.history
        if getattr(sample_source, "needs_history", False):
            window = np.stack(list(hist), axis=0).astype(np.float32)
            kw = dict(slots=every, steps=np.full(n, k, np.int64)) if keyed else {}
            raw = sample_source(window, off32, **kw)
        else:                                                         # the observer hands over float32 (observer.py:134)
            o32 = np.stack([hist[-2], hist[-1]], axis=0).astype(np.float32).astype(np.float64)
            raw = sample_source(o32[1], o32[0])
        if hasattr(raw, "detach"):
            import torch
            if out is None:
                out = torch.full((int(n_steps),) + tuple(raw.shape), float("nan"),
                                 dtype=torch.float32 if dtype == np.float32 else torch.float64,
                                 device=raw.device if device is None else device)
            elif not hasattr(out, "detach"):
                raw = raw.detach().cpu().numpy()
        if out is None:
            raw = np.asarray(raw)
            out = np.full((int(n_steps),) + raw.shape, np.nan, dtype=dtype)
        if tuple(raw.shape) != tuple(out.shape[1:]):
            raise ValueError(f"record_samples: the source returned {tuple(raw.shape)} after {tuple(out.shape[1:])}")
        if hasattr(out, "detach"):
            import torch
            t = raw if hasattr(raw, "detach") else torch.from_numpy(np.ascontiguousarray(raw))
            out[k] = t.to(device=out.device, dtype=out.dtype)
        else:
            out[k] = raw
    if out is None:
        raise ValueError("record_samples: the observer was never ready in these steps: nothing to record")
    if hasattr(out, "detach") and device is None:
        out = out.cpu().numpy()
    elif not hasattr(out, "detach") and device is not None:
        import torch
        out = torch.from_numpy(out).to(device)
    rec = RecordedSamples(out, first_step=0, sample_capacity=int(sample_capacity))
    rec.attach(off, int(out.shape[2]))
    return rec
