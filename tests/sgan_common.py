"""Shared by the Social-GAN sample-generation tests (test_sgan_cpu.py, test_gpu_sgan.py) and the fixture's generator
(tests/golden/make_golden_sgan.py): the cases, seeded weights under the reference's state-dict names, a NumPy float64
restatement of the generator's forward pass, the accuracy bound, and the emulation's case file."""
import os
import struct
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "sgan", "cases.npz")
EDGE_FIXTURE = os.path.join(HERE, "golden", "sgan", "edges.npz")
OBS_LEN, PRED_LEN = 8, 12
POOL_HIDDEN = 512                                  # PoolHiddenNet's first layer (models.py:159)
BN_EPS = 1e-5

# dimension sets: embedding, encoder h, decoder h, mlp, bottleneck, noise
DIMS = {"a": (16, 32, 32, 64, 8, 8),               # the released checkpoints' shape (as recalled; unverified)
        "b": (12, 20, 28, 40, 6, 4),               # nothing a multiple of anything
        "c": (64, 64, 128, 1024, 1024, 8),         # the capacities
        "d": (16, 32, 32, 64, 8, 0)}               # no noise: without pooling the context MLP is absent
# name: (dims, pooling, pool_every_timestep, noise mix, batch_norm, scenes, S, weight scale).  Every combination of
# pooling x pool_every_timestep x mix x batch_norm appears; scenes [1, 3, 7], [2], [0, 5, 0], [1, 3, 65]; S 1, 3, 64.
CASES = {
    "a_pool_step_ped_bn":     ("a", "pool_net", True,  "ped",    True,  [1, 3, 7],  3,  2.5),
    "a_pool_step_global":     ("a", "pool_net", True,  "global", False, [0, 5, 0],  3,  3.0),
    "a_pool_once_ped":        ("a", "pool_net", False, "ped",    False, [1, 3, 65], 3,  3.0),
    "a_pool_once_global_bn":  ("a", "pool_net", False, "global", True,  [2],        64, 3.0),
    "a_pool_step_ped":        ("a", "pool_net", True,  "ped",    False, [1, 3, 65], 1,  2.5),
    "a_pool_step_global_bn":  ("a", "pool_net", True,  "global", True,  [2],        3,  3.0),
    "a_pool_once_ped_bn":     ("a", "pool_net", False, "ped",    True,  [1, 3, 7],  1,  3.0),
    "a_pool_once_global":     ("a", "pool_net", False, "global", False, [0, 5, 0],  3,  3.0),
    "a_none_ped":             ("a", None,       False, "ped",    False, [1, 3, 7],  3,  3.0),
    "a_none_step_global_bn":  ("a", None,       True,  "global", True,  [1, 3, 65], 3,  3.0),
    "a_none_step_ped_bn":     ("a", None,       True,  "ped",    True,  [2],        64, 2.5),
    "a_none_global":          ("a", None,       False, "global", False, [0, 5, 0],  1,  3.0),
    "b_none_ped_bn":          ("b", None,       False, "ped",    True,  [1, 3, 7],  3,  3.0),
    "b_none_global_bn":       ("b", None,       False, "global", True,  [2],        3,  3.0),
    "d_plain_step_ped":       ("d", None,       True,  "ped",    False, [1, 3, 7],  3,  3.0),
    "d_plain_step_global":    ("d", None,       True,  "global", False, [0, 5, 0],  1,  3.0),
    "b_pool_step_ped_bn":     ("b", "pool_net", True,  "ped",    True,  [1, 3, 7],  3,  2.0),
    "b_pool_once_global":     ("b", "pool_net", False, "global", False, [1, 3, 65], 3,  3.0),
    "c_big_pool_step_ped_bn": ("c", "pool_net", True,  "ped",    True,  [2, 5],     2,  2.0),
}


def _edge(dims, scenes, S=1, pooling="pool_net", every=True, mix="ped", bn=False, obs_len=OBS_LEN, pred_len=PRED_LEN, scale=2.0,
          inputs=None):
    """dims: a key of DIMS or the six numbers; inputs: None, 'stationary', 'coincident' or 'far' (case_inputs)."""
    return dict(dims=DIMS[dims] if isinstance(dims, str) else tuple(dims), dims_name=dims if isinstance(dims, str) else None,
                pooling=pooling, every=every, mix=mix, bn=bn, scenes=list(scenes), S=S, scale=scale, obs_len=obs_len,
                pred_len=pred_len, inputs=inputs)


B_DIMS = DIMS["b"]
# The edges of fot_sgan_sample: the lengths, the dimensions and the scene sizes at which a tile loop of csrc/fot_sgan.hip ends,
# one short of it and one over it (LSTM tile: 16 rows, 4 per thread; pool: 16 neighbours, blocks of 8 outputs; MLP: 4 rows;
# loops strided by 256 threads over 4 H, M and O), and inputs with exact zeros.  Shapes as small as the loop in question allows.
# Weight scale 2: of 1.5 / 2 / 2.5 / 3 the one at which the reference moves 0.3 .. 2 m per step in every case (make_golden_sgan.py --probe).
EDGE_CASES = {
    # lengths (the library accepts 1 .. 32 of both)
    "len_obs1":          _edge("a", [3, 2], S=2, obs_len=1),                    # k_sgan_decode: rel = 0 without a step before
    "len_obs2":          _edge("b", [4], S=2, every=False, mix="global", obs_len=2),
    "len_obs32":         _edge("a", [5], pooling=None, every=False, bn=True, obs_len=32),
    "len_pred1":         _edge("a", [3], S=2, pred_len=1),                      # pooling at every step, never pooled
    "len_pred32_step":   _edge("a", [4, 1], S=2, pred_len=32),                  # 32 launches, the state in HBM
    "len_pred32_once":   _edge("a", [5], S=2, every=False, pred_len=32),        # one launch
    # dimensions
    "dim_all_min":       _edge((1, 1, 2, 1, 1, 1), [3, 1], S=2),
    "dim_b8_scene16":    _edge(B_DIMS[:4] + (8, 4), [16]),
    "dim_b9_scene16":    _edge(B_DIMS[:4] + (9, 4), [16], bn=True),             # padded to 16: seven phantom outputs
    "dim_b1":            _edge(B_DIMS[:4] + (1, 4), [5], S=2, every=False),
    "dim_hd64":          _edge((16, 32, 64, 64, 8, 8), [17]),                   # 4 H = the 256 threads
    "dim_hd65_scene17":  _edge((16, 32, 65, 64, 8, 8), [17]),
    "dim_hd128_he1":     _edge((16, 1, 128, 64, 8, 8), [17], every=False, mix="global"),
    "dim_m256":          _edge((16, 32, 32, 256, 8, 8), [5], pooling=None, every=False),
    "dim_m257_scene15":  _edge((16, 32, 32, 257, 8, 8), [15], S=2),
    "dim_ctx_of_one":    _edge((16, 32, 32, 64, 8, 31), [5], S=2, every=False),  # nd = Hd - 1
    "dim_nd0_he_ne_hd":  _edge((16, 24, 32, 64, 8, 0), [5], S=2, pooling=None, every=False),
    "cap_c_scene17":     _edge("c", [17], bn=True, pred_len=3),
    # scene sizes and rows
    "scn_tiles_step":    _edge("b", [15, 16, 17, 31, 32, 33], pred_len=4),
    "scn_tiles_once":    _edge("b", [15, 16, 17, 31, 32, 33], every=False, mix="global", pred_len=4),
    "scn_256_and_1":     _edge("a", [256, 1], obs_len=2, pred_len=3),           # FOT_SGAN_MAX_PEDS
    "rows_16":           _edge("b", [8], S=2, pred_len=4),                      # S N = one LSTM tile, four MLP tiles
    "rows_17":           _edge("b", [8, 9], pred_len=4),
    "rows_4":            _edge("b", [2], S=2, pred_len=4),
    "rows_5":            _edge("b", [1], S=5, pred_len=4),
    "scn_40_small":      _edge("b", [i * 7 % 3 for i in range(40)], S=3, mix="global", pred_len=4),
    "s64_step_scene17":  _edge("a", [17], S=64, pred_len=3),
    # inputs
    "in_stationary":     _edge("a", [3], S=2, inputs="stationary"),             # every displacement exactly 0
    "in_coincident":     _edge("a", [3], S=2, inputs="coincident"),             # dx = dy = 0 in the pool
    "in_far":            _edge("a", [3, 2], S=2, inputs="far"),                 # 2e4 m from the origin
}


def case(name):
    """A case of either table in the form of _edge()."""
    if name in EDGE_CASES:
        return EDGE_CASES[name]
    dims, pooling, every, mix, bn, scenes, S, scale = CASES[name]
    return _edge(dims, scenes, S=S, pooling=pooling, every=every, mix=mix, bn=bn, scale=scale)


def case_scale(name):
    return case(name)["scale"]


def case_args(name):
    c = case(name)
    e, he, hd, m, b, nd = c["dims"]
    return dict(obs_len=c["obs_len"], pred_len=c["pred_len"], embedding_dim=e, encoder_h_dim=he, decoder_h_dim=hd, mlp_dim=m,
                bottleneck_dim=b, noise_dim=(nd,), num_layers=1, pooling_type=c["pooling"], pool_every_timestep=c["every"],
                noise_mix_type=c["mix"], batch_norm=c["bn"], dropout=0.0, noise_type="gaussian")


def case_seed(name):
    return zlib.crc32(name.encode()) % 1_000_000


def needs_context(a):
    return bool(a["noise_dim"][0] or a["pooling_type"] or a["encoder_h_dim"] != a["decoder_h_dim"])


def pools_every_step(a):
    return bool(a["pool_every_timestep"] and a["pooling_type"])


# ---- seeded weights -------------------------------------------------------------------------------------------------------
def seeded_state(a, seed, scale=3.0):
    """A state dict of the reference's TrajectoryGenerator(**a) filled from NumPy: torch's default initialisation
    (uniform in +-1/sqrt(fan_in); the LSTM: +-1/sqrt(hidden)) times ``scale``, BatchNorm with non-trivial statistics.
    Values are float32 numbers held in float64 arrays."""
    rng = np.random.default_rng(seed)
    st = {}

    def uni(shape, k):
        return (rng.uniform(-k, k, size=shape) * scale).astype(np.float32).astype(np.float64)

    def linear(prefix, n_in, n_out):
        st[prefix + ".weight"], st[prefix + ".bias"] = uni((n_out, n_in), n_in ** -0.5), uni((n_out,), n_in ** -0.5)

    def lstm(prefix, n_in, h):
        st[prefix + ".weight_ih_l0"], st[prefix + ".weight_hh_l0"] = uni((4 * h, n_in), h ** -0.5), uni((4 * h, h), h ** -0.5)
        st[prefix + ".bias_ih_l0"], st[prefix + ".bias_hh_l0"] = uni((4 * h,), h ** -0.5), uni((4 * h,), h ** -0.5)

    def mlp(prefix, dims):
        i = 0
        for n_in, n_out in zip(dims[:-1], dims[1:]):
            linear(f"{prefix}.{i}", n_in, n_out)
            i += 1
            if a["batch_norm"]:
                f32 = lambda lo, hi: rng.uniform(lo, hi, size=n_out).astype(np.float32).astype(np.float64)
                st[f"{prefix}.{i}.weight"], st[f"{prefix}.{i}.bias"] = f32(0.5, 1.5), f32(-0.3, 0.3)
                st[f"{prefix}.{i}.running_mean"], st[f"{prefix}.{i}.running_var"] = f32(-0.3, 0.3), f32(0.5, 2.0)
                st[f"{prefix}.{i}.num_batches_tracked"] = np.asarray(0, dtype=np.int64)
                i += 1
            i += 1                                                 # the ReLU

    def pool(prefix, h):
        linear(prefix + ".spatial_embedding", 2, e)
        mlp(prefix + ".mlp_pre_pool", [e + h, POOL_HIDDEN, b])

    e, he, hd, m, b, nd = (a["embedding_dim"], a["encoder_h_dim"], a["decoder_h_dim"], a["mlp_dim"], a["bottleneck_dim"],
                           a["noise_dim"][0])
    lstm("encoder.encoder", e, he); linear("encoder.spatial_embedding", 2, e)
    lstm("decoder.decoder", e, hd)
    if pools_every_step(a):
        pool("decoder.pool_net", hd)
        mlp("decoder.mlp", [hd + b, m, hd])
    linear("decoder.spatial_embedding", 2, e); linear("decoder.hidden2pos", hd, 2)
    if a["pooling_type"]:
        pool("pool_net", he)
    if needs_context(a):
        mlp("mlp_decoder_context", [he + (b if a["pooling_type"] else 0), m, hd - nd])
    return st


def case_inputs(name):
    """obs [obs_len, N, 2] float32 (walking pedestrians), ped_off, noise [S, rows, nd] float32 -- from the case's seed.  An edge
    case's ``inputs``: 'stationary' -- the first pedestrian stands still; 'coincident' -- the second walks in the first one's
    steps; 'far' -- everything 2e4 m from the origin."""
    c = case(name)
    mix, scenes, S = c["mix"], c["scenes"], c["S"]
    a = case_args(name)
    rng = np.random.default_rng(case_seed(name) + 50_000)
    off = np.concatenate([[0], np.cumsum(scenes)]).astype(np.int32)
    n = int(off[-1])
    start = rng.uniform(-6.0, 6.0, size=(n, 2))
    vel = rng.uniform(-0.6, 0.6, size=(n, 2))
    steps = vel[None] + rng.normal(0.0, 0.05, size=(a["obs_len"], n, 2))
    track = start[None] + np.cumsum(steps, axis=0)
    if c["inputs"] == "stationary":
        track[:, 0] = track[0, 0]
    elif c["inputs"] == "coincident":
        track[:, 1] = track[:, 0]
    elif c["inputs"] == "far":
        track = track + np.array([2.0e4, -2.0e4])
    obs = track.astype(np.float32)
    rows = len(scenes) if mix == "global" else n
    noise = rng.standard_normal(size=(S, rows, a["noise_dim"][0])).astype(np.float32)
    return obs, off, noise


# ---- the forward pass, restated in NumPy ------------------------------------------------------------------------------------
def _sigmoid(x):
    return 1 / (1 + np.exp(-x))


def _mlp(st, prefix, x):
    """make_mlp's Sequential: Linear, BatchNorm1d in eval mode where the state holds one, ReLU -- for every Linear."""
    layers = sorted(int(k[len(prefix) + 1:].split(".")[0]) for k in st
                    if k.startswith(prefix + ".") and k.endswith(".weight") and np.ndim(st[k]) == 2)
    for i in layers:
        x = x @ st[f"{prefix}.{i}.weight"].T + st[f"{prefix}.{i}.bias"]
        bn = f"{prefix}.{i + 1}"
        if bn + ".running_mean" in st:
            x = (x - st[bn + ".running_mean"]) / np.sqrt(st[bn + ".running_var"] + x.dtype.type(BN_EPS)) * st[bn + ".weight"] + st[bn + ".bias"]
        x = np.maximum(x, 0)
    return x


def _lstm(st, prefix, x, h, c):
    g = x @ st[prefix + ".weight_ih_l0"].T + st[prefix + ".bias_ih_l0"] + h @ st[prefix + ".weight_hh_l0"].T + st[prefix + ".bias_hh_l0"]
    i, f, cand, o = np.split(g, 4, axis=-1)
    c = _sigmoid(f) * c + _sigmoid(i) * np.tanh(cand)
    return _sigmoid(o) * np.tanh(c), c


def _linear(st, prefix, x):
    return x @ st[prefix + ".weight"].T + st[prefix + ".bias"]


def _pool(st, prefix, h, pos, off):
    """Per scene and pedestrian i: the maximum over the scene's j of MLP([embedding(pos_j - pos_i) ; h_j])."""
    out = []
    for lo, hi in zip(off[:-1], off[1:]):
        if hi == lo:
            continue
        p, hh = pos[lo:hi], h[lo:hi]
        rel = p[None, :, :] - p[:, None, :]                          # [i, j]
        emb = _linear(st, prefix + ".spatial_embedding", rel)
        x = np.concatenate([emb, np.broadcast_to(hh[None], (hi - lo,) + hh.shape)], axis=-1)
        out.append(_mlp(st, prefix + ".mlp_pre_pool", x).max(axis=1))
    return np.concatenate(out, axis=0)


def restate(a, state, obs, off, noise, dtype=np.float64):
    """TrajectoryGenerator.forward + relative_to_abs in float64: [S, pred_len, N, 2].  ``state`` with or without BatchNorm
    entries (a folded state has none).  dtype=np.float32: the same operations in float32 -- a stand-in for the reference's own
    float32 run where the reference is not at hand."""
    st = {k: np.asarray(v, dtype=dtype) for k, v in state.items() if not k.endswith("num_batches_tracked")}
    obs = np.asarray(obs, dtype=dtype)
    noise = np.asarray(noise, dtype=dtype)
    n, nd, hd = obs.shape[1], a["noise_dim"][0], a["decoder_h_dim"]
    S = noise.shape[0]
    if n == 0:
        return np.zeros((S, a["pred_len"], 0, 2), dtype)
    rel = np.concatenate([np.zeros((1, n, 2), dtype), obs[1:] - obs[:-1]], axis=0)
    h = c = np.zeros((n, a["encoder_h_dim"]), dtype)
    for t in range(obs.shape[0]):
        h, c = _lstm(st, "encoder.encoder", _linear(st, "encoder.spatial_embedding", rel[t]), h, c)
    ctx = h
    if a["pooling_type"]:
        ctx = np.concatenate([h, _pool(st, "pool_net", h, obs[-1], off)], axis=1)
    if needs_context(a):
        ctx = _mlp(st, "mlp_decoder_context", ctx)
    scene_of = np.repeat(np.arange(len(off) - 1), np.diff(off))
    out = np.zeros((S, a["pred_len"], n, 2), dtype)
    for s in range(S):
        z = noise[s][scene_of] if a["noise_mix_type"] == "global" else noise[s]
        h = np.concatenate([ctx, z], axis=1) if nd else ctx
        assert h.shape == (n, hd)
        c = np.zeros((n, hd), dtype)
        x = _linear(st, "decoder.spatial_embedding", rel[-1])
        pos, cum = obs[-1].copy(), np.zeros((n, 2), dtype)
        for t in range(a["pred_len"]):
            h, c = _lstm(st, "decoder.decoder", x, h, c)
            step = _linear(st, "decoder.hidden2pos", h)
            pos = step + pos
            if pools_every_step(a):
                h = _mlp(st, "decoder.mlp", np.concatenate([h, _pool(st, "decoder.pool_net", h, pos, off)], axis=1))
            x = _linear(st, "decoder.spatial_embedding", step)
            cum = cum + step
            out[s, t] = cum + obs[-1]
    return out


# ---- the accuracy bound ---------------------------------------------------------------------------------------------------
def accuracy_bound(ref32, ref64):
    """max(8 e_ref, 16 ulp32 of the largest |coordinate|), e_ref = max |reference float32 - reference float64|: the
    factor covers another summation order and other exp forms, the floor the 12 float32 additions into the absolute
    position when e_ref happens to be small."""
    e_ref = float(np.max(np.abs(ref32.astype(np.float64) - ref64))) if ref64.size else 0.0
    top = float(np.max(np.abs(ref64))) if ref64.size else 1.0
    return max(8.0 * e_ref, 16.0 * float(np.spacing(np.float32(top))))


def load_fixture(path=FIXTURE):
    z = np.load(path, allow_pickle=False)
    return {k: z[k] for k in z.files}


def fixture_case(fix, name):
    """(obs, ped_off, noise, ref32, ref64) of a case."""
    return tuple(fix[f"{name}/{k}"] for k in ("obs", "ped_off", "noise", "out32", "out64"))


# ---- tests/emu/fot_sgan_emu: one case per file ---------------------------------------------------------------------------------
def write_emu_case(path, desc_bytes, blob, off, obs, S, noise):
    """fot_sgan_desc (56 bytes) | int64 n_weights | weights | int32 n_scenes | ped_off | int32 S | obs | noise."""
    with open(path, "wb") as f:
        f.write(desc_bytes)
        f.write(struct.pack("<q", blob.size)); f.write(np.ascontiguousarray(blob, np.float32).tobytes())
        f.write(struct.pack("<i", len(off) - 1)); f.write(np.ascontiguousarray(off, np.int32).tobytes())
        f.write(struct.pack("<i", S))
        f.write(np.ascontiguousarray(obs, np.float32).tobytes())
        f.write(np.ascontiguousarray(noise, np.float32).tobytes())


# ---- closed-loop episodes ----------------------------------------------------------------------------------------------------
def charging_wall_tracks(n_frames=140, warmup_frames=32, speed=3.0, dt=0.1):
    """[n_frames, 3, 2]: three pedestrians abreast across the whole road (y = -1.2, 0, 1.2) running at the ego along -x, 5 m
    ahead of its start (0, 0) when the warm-up ends: whatever the planner does, the episode ends in a collision within two
    seconds -- an episode that ends early by construction."""
    f = np.arange(n_frames, dtype=np.float64)[:, None]
    x = 5.0 + speed * dt * (warmup_frames - f)
    y = np.array([-1.2, 0.0, 1.2])[None, :]
    return np.stack([np.broadcast_to(x, (n_frames, 3)), np.broadcast_to(y, (n_frames, 3))], axis=-1).copy()
