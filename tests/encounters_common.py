"""Cutting encounters out of recorded clips (fot_encounters_extract, fidelity.extract_encounters): a NumPy restatement of
the whole chain -- alignment, candidate spans, populations, closest approach, velocities, cruise speeds and far goals -- the
clips of the fixture (tests/golden/encounters), the random clips of the fuzz and the stand-alone emulation's file format.

The restatement is pinned bit for bit to the reference's answers in tests/test_encounters_cpu.py; the GPU tests compare the
library with the restatement, never with itself.  A clip is a dictionary: name, times [T], ped_xy [T, A, 2], ped_ids [A],
veh_times [Tv], veh_xy [Tv, K, 2], veh_ids [K] and optionally ped_vel [T, A, 2], veh_psi and veh_vel [Tv, K]."""
import json
import os
import struct

import numpy as np

import fidelity_common as fc

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "encounters")
SHORT, NO_PEDS, FAR, KEPT = range(4)
STATUS_NAMES = ("SHORT", "NO_PEDS", "FAR", "KEPT")
MODES = {None: 0, "median": 1, "quantile": 2, "freewalk": 3}
DEFAULT_Q = {"median": 0.5, "quantile": 0.85, "freewalk": 0.5}
FLOOR = 1e-3
CLIP_ARRAYS = ("times", "ped_xy", "ped_ids", "veh_times", "veh_xy", "veh_ids", "ped_vel", "veh_psi", "veh_vel")
SPAN_DT = np.dtype([("min_separation", "<f8"), ("real", fc.ENC_DT), ("row_base", "<i8"), ("status", "<i4"), ("vehicle", "<i4"),
                    ("frame0", "<i4"), ("frame1", "<i4"), ("n_ped", "<i4"), ("min_step", "<i4"), ("min_col", "<i4"), ("_pad", "<i4")])
PARAMS = dict(min_sep_threshold=8.0, min_len=5, accel_threshold=0.3, max_distance=5.0, cruise=None, cruise_q=0.85,
              free_distance=8.0, goal_distance=50.0, measure_real=True)


# ---- alignment --------------------------------------------------------------------------------------------------------------
def channel_on_grid(src_t, src_v, grid, angular=False):
    """a vehicle's channel on the pedestrian grid: its finite samples sorted by time, interpolated inside their span (1e-9 s
    of slack), NaN elsewhere; a heading is unwrapped first and wrapped after"""
    good = np.isfinite(src_t) & np.isfinite(src_v)
    out = np.full(len(grid), np.nan)
    if good.sum() < 2:
        return out
    order = np.argsort(src_t[good])
    t, v = src_t[good][order], src_v[good][order]
    v = np.unwrap(v) if angular else v
    inside = (grid >= t[0] - 1e-9) & (grid <= t[-1] + 1e-9)
    got = np.interp(grid[inside], t, v)
    out[inside] = (got + np.pi) % (2 * np.pi) - np.pi if angular else got
    return out


def align(clip):
    """(ego_xy [K, T, 2], ego_psi [K, T], ego_vel [K, T], dt)"""
    grid = clip["times"]
    dt = float(grid[1] - grid[0]) if len(grid) >= 2 else 0.4
    K = clip["veh_xy"].shape[1]
    xy, psi, vel = [], [], []
    for k in range(K):
        p = np.stack([channel_on_grid(clip["veh_times"], clip["veh_xy"][:, k, c], grid) for c in range(2)], axis=1)
        d = np.gradient(p, dt, axis=0) if len(grid) >= 2 else np.full((len(grid), 2), np.nan)
        psi.append(channel_on_grid(clip["veh_times"], clip["veh_psi"][:, k], grid, angular=True) if clip.get("veh_psi") is not None
                   else np.arctan2(d[:, 1], d[:, 0]))
        vel.append(channel_on_grid(clip["veh_times"], clip["veh_vel"][:, k], grid) if clip.get("veh_vel") is not None
                   else np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]))
        xy.append(p)
    T = len(grid)
    return (np.array(xy).reshape(K, T, 2), np.array(psi).reshape(K, T), np.array(vel).reshape(K, T), dt)


def velocities(ped_xy, ped_vel, dt):
    """the recorded velocities, or forward differences over the whole grid with the last frame repeating the one before"""
    if ped_vel is not None:
        return ped_vel
    vel = np.full(ped_xy.shape, np.nan)
    if len(ped_xy) >= 2:
        vel[:-1] = (ped_xy[1:] - ped_xy[:-1]) / dt
        vel[-1] = vel[-2]
    return vel


# ---- spans, populations, closest approach -----------------------------------------------------------------------------------
def runs(mask):
    """[(start, stop)] of the maximal runs of True"""
    edge = np.diff(np.concatenate([[0], np.asarray(mask, np.int8), [0]]))
    return list(zip(np.flatnonzero(edge == 1).tolist(), np.flatnonzero(edge == -1).tolist()))


def candidate_spans(ped_xy, ped_vel, ego_xy, ego_psi, ego_vel, dt, min_sep_threshold=8.0, min_len=5):
    """one dictionary per candidate span, by vehicle, then by start: status, vehicle, frame0, frame1, cols (the present
    columns), min_separation with its first (step, column) in row-major order"""
    vel = velocities(ped_xy, ped_vel, dt)
    out = []
    for k in range(len(ego_xy)):
        here = np.isfinite(ego_xy[k]).all(axis=1) & np.isfinite(ego_psi[k]) & np.isfinite(ego_vel[k])
        for f0, f1 in runs(here):
            s = dict(status=SHORT, vehicle=k, frame0=f0, frame1=f1, cols=np.zeros(0, np.int64), min_separation=np.nan, min_step=-1,
                     min_col=-1)
            out.append(s)
            if f1 - f0 < min_len:
                continue
            gone = np.isnan(ped_xy[f0:f1]).any(axis=(0, 2)) | np.isnan(vel[f0:f1]).any(axis=(0, 2))
            s["cols"] = np.flatnonzero(~gone)
            if s["cols"].size == 0:
                s.update(status=NO_PEDS, min_separation=np.inf)
                continue
            d = fc.distances(ego_xy[k, f0:f1], ped_xy[f0:f1][:, s["cols"]])                     # [L, N]
            s["min_separation"] = float(np.min(d))
            if not np.isnan(s["min_separation"]):
                s["min_step"], s["min_col"] = (int(i) for i in np.unravel_index(np.argmin(d), d.shape))
            s["status"] = FAR if s["min_separation"] > min_sep_threshold else KEPT
    return out


# ---- boundary conditions ----------------------------------------------------------------------------------------------------
def floor(c):
    return np.where(np.isfinite(c) & (c > FLOOR), c, FLOOR)


def cruise_speeds(ego_xy, ped_xy, ped_vel, mode, q=None, free_distance=8.0):
    """[N] cruise speeds of one encounter: the median, np.quantile's linear quantile, or that quantile over the
    free-walking steps (the all-step median where there are none); floored"""
    q = DEFAULT_Q[mode] if q is None else q
    speeds = fc.dist(ped_vel[..., 0], ped_vel[..., 1])                                          # [L, N]
    if mode == "median":
        return floor(np.array([np.median(speeds[:, j]) for j in range(speeds.shape[1])]))
    if mode == "quantile":
        return floor(np.array([np.quantile(speeds[:, j], q) for j in range(speeds.shape[1])]))
    free = (fc.distances(ego_xy, ped_xy) > free_distance) & np.isfinite(speeds)
    return floor(np.array([np.quantile(speeds[free[:, j], j], q) if free[:, j].any() else np.median(speeds[:, j])
                           for j in range(speeds.shape[1])]))


def far_goals(ped_xy, ped_vel, distance=50.0):
    """[N, 2]: `distance` ahead of the first position along the net displacement, the first velocity or +x"""
    head = ped_xy[-1] - ped_xy[0]
    for j in np.flatnonzero(fc.dist(head[:, 0], head[:, 1]) < FLOOR):
        v = ped_vel[0, j]
        head[j] = v if fc.dist(v[0], v[1]) > FLOOR else (1.0, 0.0)
    return ped_xy[0] + head / fc.dist(head[:, 0], head[:, 1])[:, None] * distance


# ---- one library call, and the chain over clips -----------------------------------------------------------------------------
def expected_call(ped_xy, ped_vel, ego_xy, ego_psi, ego_vel, dt, **kw):
    """what batch.encounters_extract returns for these arguments: spans (SPAN_DT), cols, cruise, goals, onset_dist,
    onset_step, series"""
    p = dict(PARAMS, **kw)
    vel = velocities(ped_xy, ped_vel, dt)
    found = candidate_spans(ped_xy, ped_vel, ego_xy, ego_psi, ego_vel, dt, p["min_sep_threshold"], p["min_len"])
    if ped_xy.shape[0] == 0 or ped_xy.shape[1] == 0:               # (a call without frames or columns has no spans)
        found = []
    spans = np.zeros(len(found), SPAN_DT)
    cols, speed, goal, dist, step, series = [], [], [], [], [], []
    rows = 0
    for rec, s in zip(spans, found):
        for k in ("status", "vehicle", "frame0", "frame1", "min_separation", "min_step", "min_col"):
            rec[k] = s[k]
        rec["n_ped"], rec["row_base"] = len(s["cols"]), -1
        rec["real"]["closest"], rec["real"]["closest_step"] = np.nan, -1
        if s["status"] != KEPT:
            continue
        rec["row_base"] = rows
        rows += len(s["cols"])
        frames = slice(s["frame0"], s["frame1"])
        e_xy, e_ped, e_vel = ego_xy[s["vehicle"], frames], ped_xy[frames][:, s["cols"]], vel[frames][:, s["cols"]]
        cols.append(s["cols"])
        if p["cruise"] is not None:
            speed.append(cruise_speeds(e_xy, e_ped, e_vel, p["cruise"], p["cruise_q"], p["free_distance"]))
            goal.append(far_goals(e_ped, e_vel, p["goal_distance"]))
        if p["measure_real"]:
            r, ser, where, at, _, _ = fc.record(e_xy, e_ped, dt=dt, accel_threshold=p["accel_threshold"], max_distance=p["max_distance"])
            rec["real"] = r
            dist.append(where); step.append(at); series.append(ser)
    cat = lambda parts, dtype, tail=(): np.concatenate(parts).astype(dtype) if parts else np.zeros((0,) + tail, dtype)
    return dict(spans=spans, cols=cat(cols, np.int32), cruise=cat(speed, np.float64) if p["cruise"] else None,
                goals=cat(goal, np.float64, (2,)) if p["cruise"] else None, onset_dist=cat(dist, np.float64) if p["measure_real"] else None,
                onset_step=cat(step, np.int32) if p["measure_real"] else None, series=cat(series, np.float64) if p["measure_real"] else None)


def extract(clips, min_sep_threshold=8.0, min_len=5, multivehicle=True):
    """the encounters of the clips, in the reference's order, as dictionaries with the reference's fields"""
    out = []
    for clip in clips:
        K = clip["veh_xy"].shape[1]
        if K == 0 or (K > 1 and not multivehicle):
            continue
        ego_xy, ego_psi, ego_vel, dt = align(clip)
        vel = velocities(clip["ped_xy"], clip.get("ped_vel"), dt)
        for s in candidate_spans(clip["ped_xy"], clip.get("ped_vel"), ego_xy, ego_psi, ego_vel, dt, min_sep_threshold, min_len):
            if s["status"] != KEPT:
                continue
            k, frames = s["vehicle"], slice(s["frame0"], s["frame1"])
            out.append(dict(clip=clip["name"] + (f"#v{int(clip['veh_ids'][k])}" if K > 1 else ""), times=clip["times"][frames],
                            ego_xy=ego_xy[k, frames], ego_psi=ego_psi[k, frames], ego_vel=ego_vel[k, frames],
                            ped_xy=clip["ped_xy"][frames][:, s["cols"]], ped_vel=vel[frames][:, s["cols"]],
                            ped_ids=clip["ped_ids"][s["cols"]], dt=dt, min_separation=s["min_separation"]))
    return out


def same(got, want):
    """equal bits, a NaN for a NaN"""
    got, want = np.asarray(got), np.asarray(want)
    return got.shape == want.shape and np.array_equal(got, want, equal_nan=got.dtype.kind == "f")


def relative_difference(got, want):
    """the largest |got - want| / |want| (0 where the two are equal, infinite where only `want` is 0 or one side is NaN)"""
    got, want = np.asarray(got, float), np.asarray(want, float)
    if got.shape != want.shape:
        return float("inf")
    equal = (got == want) | (np.isnan(got) & np.isnan(want))
    with np.errstate(divide="ignore", invalid="ignore"):
        rel = np.where(equal, 0.0, np.abs(got - want) / np.abs(want))
    rel = np.where(np.isnan(rel), np.inf, rel)
    return float(np.max(rel, initial=0.0))


def same_spans(got, want):
    """the first field in which two span tables differ, or None"""
    if len(got) != len(want):
        return f"{len(got)} spans, not {len(want)}"
    for k in SPAN_DT.names:
        if k == "_pad":
            continue
        if k == "real":
            for f in fc.ENC_DT.names:
                if not same(got[k][f], want[k][f]):
                    return f"real.{f}: {got[k][f]} != {want[k][f]}"
        elif not same(got[k], want[k]):
            return f"{k}: {got[k]} != {want[k]}"
    return None


def assert_call_matches(got, want, label=""):
    why = same_spans(got["spans"], want["spans"])
    assert why is None, f"{label}: {why}"
    for k in ("cols", "cruise", "goals", "onset_dist", "onset_step", "series"):
        if want[k] is None or got.get(k) is None:
            continue
        assert same(got[k], want[k]), f"{label}: {k}"


# ---- clips ------------------------------------------------------------------------------------------------------------------
def walkers(rng, T, A, dt, speed=1.3, box=12.0):
    """[T, A, 2] pedestrians on noisy straight walks through a box around the origin"""
    start = rng.uniform(-box, box, (A, 2))
    way = rng.uniform(0.0, 2 * np.pi, A)
    v = rng.uniform(0.4, 1.0, A)[:, None] * speed * np.stack([np.cos(way), np.sin(way)], axis=1)
    t = np.arange(T)[:, None, None] * dt
    return start[None] + v[None] * t + np.cumsum(rng.normal(0.0, 0.02, (T, A, 2)), axis=0)


def absent(rng, xy, p_late=0.3, p_early=0.3):
    """NaN before a pedestrian's arrival and after its departure"""
    T, A, _ = xy.shape
    for a in range(A):
        if rng.random() < p_late:
            xy[:rng.integers(1, max(T // 2, 2)), a] = np.nan
        if rng.random() < p_early:
            xy[T - rng.integers(1, max(T // 2, 2)):, a] = np.nan
    return xy


def random_clip(rng, T, A, K, with_vel=None, with_psi=None, fps=2.5):
    """a random clip: K vehicles crossing the box on their own sampling, each over a part of the grid; pedestrians that come
    and go"""
    dt = 1.0 / fps
    times = np.arange(T) * dt
    ped = absent(rng, walkers(rng, T, A, dt), 0.35, 0.35) if A else np.zeros((T, 0, 2))
    Tv = max(int(T * 1.3), 2)
    veh_times = np.linspace(times[0] - 0.2 * dt, times[-1] + 0.2 * dt, Tv) if T > 1 else np.array([times[0] - 0.1, times[0] + 0.1])
    veh = np.full((Tv, K, 2), np.nan)
    for k in range(K):
        a, b = sorted(rng.integers(0, Tv + 1, 2))
        if rng.random() < 0.3:
            a, b = 0, Tv
        n = b - a
        if n == 0:
            continue
        far = rng.random() < 0.25
        y0 = rng.uniform(40.0, 60.0) if far else rng.uniform(-6.0, 6.0)
        s = np.linspace(-15.0, 15.0, n) if n > 1 else np.zeros(1)
        veh[a:b, k] = np.stack([s, y0 + 0.05 * s * rng.normal()], axis=1)
        if n > 6 and rng.random() < 0.4:                           # a hole in the track: two spans, or a bridged gap
            c = rng.integers(a + 2, b - 2)
            veh[c:c + rng.integers(1, 3), k, rng.integers(0, 2)] = np.nan
    clip = dict(name=f"clip{rng.integers(1 << 30)}", times=times, ped_xy=ped, ped_ids=np.arange(A) + 100, veh_times=veh_times,
                veh_xy=veh, veh_ids=np.arange(K) * 3 + 1)
    if rng.random() < 0.5 if with_vel is None else with_vel:
        vel = velocities(ped, None, dt) + rng.normal(0.0, 0.01, ped.shape)
        vel[np.isnan(ped)] = np.nan
        clip["ped_vel"] = vel
    if rng.random() < 0.6 if with_psi is None else with_psi:
        d = np.nan_to_num(np.gradient(np.nan_to_num(veh), axis=0))
        clip["veh_psi"] = np.arctan2(d[..., 1], d[..., 0]) + rng.normal(0.0, 0.01, (Tv, K))
        clip["veh_vel"] = np.abs(rng.normal(6.0, 1.0, (Tv, K)))
    return clip


def fuzz_clips(seed=29, n=40):
    """the 40 random clips of the fuzz: T <= 120, A <= 70, K <= 4"""
    rng = np.random.default_rng(seed)
    return [random_clip(rng, int(rng.integers(2, 121)), int(rng.integers(0, 71)), int(rng.integers(1, 5))) for _ in range(n)]


# ---- the fixture ------------------------------------------------------------------------------------------------------------
def load_fixture():
    """{clip name: (clip dictionary, the reference's answers)} and the meta dictionary"""
    with open(os.path.join(GOLDEN_DIR, "meta.json")) as f:
        meta = json.load(f)
    clips = {}
    for name in meta["clips"]:
        with np.load(os.path.join(GOLDEN_DIR, name + ".npz"), allow_pickle=False) as z:
            arrays = {k: z[k] for k in z.files}
        clip = {k: arrays[k] for k in CLIP_ARRAYS if k in arrays}
        clip["name"] = name
        clips[name] = (clip, {k: v for k, v in arrays.items() if k.startswith(("ref_", "enc"))})
    return clips, meta


# ---- the emulation's files (tests/emu/fot_encounter_emu.cpp) ----------------------------------------------------------------
def write_emu_case(path, ped_xy, ped_vel, ego_xy, ego_psi, ego_vel, dt, **kw):
    p = dict(PARAMS, **kw)
    K, T = ego_xy.shape[:2]
    A = ped_xy.shape[1]
    with open(path, "wb") as f:
        f.write(struct.pack("<7d4i", p["min_sep_threshold"], dt, p["accel_threshold"], p["max_distance"], p["cruise_q"],
                            p["free_distance"], p["goal_distance"], p["min_len"], MODES[p["cruise"]], 2 if p["measure_real"] else 0, 0))
        f.write(struct.pack("<4i", T, A, K, int(ped_vel is not None)))
        for a in (ped_xy, ped_vel, ego_xy, ego_psi, ego_vel):
            if a is not None:
                f.write(np.ascontiguousarray(a, dtype="<f8").tobytes())


def read_emu_out(path):
    """(code, the dictionary of expected_call)"""
    with open(path, "rb") as f:
        raw = f.read()
    code, n_spans, n_rows, n_steps = struct.unpack_from("<iiqq", raw, 0)
    at = 24
    if code != 0:
        return code, None

    def take(dtype, count, shape=None):
        nonlocal at
        a = np.frombuffer(raw, dtype, count, at).copy()
        at += a.nbytes
        return a if shape is None else a.reshape(shape)

    out = dict(spans=take(SPAN_DT, n_spans), cols=take("<i4", n_rows), cruise=take("<f8", n_rows), goals=take("<f8", 2 * n_rows, (n_rows, 2)),
               onset_dist=take("<f8", n_rows), onset_step=take("<i4", n_rows), series=take("<f8", n_steps))
    assert at == len(raw)
    return code, out


# ---- designed calls: the edges of the kernels and of the rules (CPU emulation and GPU alike) ---------------------------------
def drive(T, spans, K=1, dt=0.4, y=0.0, speed=2.0):
    """ego channels [K, T(, 2)] finite exactly on the given (vehicle, frame0, frame1) spans: straight drives along x"""
    xy, psi, vel = np.full((K, T, 2), np.nan), np.full((K, T), np.nan), np.full((K, T), np.nan)
    for k, f0, f1 in spans:
        t = np.arange(f0, f1) * dt
        xy[k, f0:f1] = np.stack([-4.0 + speed * t + 0.5 * k, np.full(f1 - f0, y + 1.5 * k)], axis=1)
        psi[k, f0:f1], vel[k, f0:f1] = 0.01 * k, speed
    return xy, psi, vel


def call(label, ped_xy, ego, dt=0.4, ped_vel=None, **kw):
    return dict(label=label, ped_xy=np.ascontiguousarray(ped_xy, dtype=float), ped_vel=ped_vel, ego_xy=ego[0], ego_psi=ego[1],
                ego_vel=ego[2], dt=dt, kw=kw)


def crowd(rng, T, A, dt=0.4, holes=True):
    """walkers of which column 0 and column A-1 stay and, with holes, about a third of the others miss a frame"""
    xy = walkers(rng, T, A, dt, box=6.0)
    if holes:
        for a in range(1, A - 1):
            if rng.random() < 0.35:
                xy[rng.integers(0, T), a, rng.integers(0, 2)] = np.nan
    return xy


def edge_calls():
    rng = np.random.default_rng(2901)
    out = []
    for A in (1, 63, 64, 65, 256, 257):                            # the column tile, the ballot's turns
        out.append(call(f"A={A}", crowd(rng, 12, A), drive(12, [(0, 0, 12)]), min_sep_threshold=50.0))
    for L in (4, 5, 6):                                            # min_len - 1, min_len, min_len + 1; the step shares
        out.append(call(f"L={L}", crowd(rng, 9, 7, holes=False), drive(9, [(0, 2, 2 + L)]), min_sep_threshold=50.0))
    out.append(call("L=2, min_len=1", crowd(rng, 6, 5, holes=False), drive(6, [(0, 3, 5)]), min_len=1, min_sep_threshold=50.0))
    out.append(call("L=3, min_len=1", crowd(rng, 6, 5, holes=False), drive(6, [(0, 1, 4)]), min_len=1, min_sep_threshold=50.0))
    out.append(call("L=1, min_len=1", crowd(rng, 6, 5, holes=False), drive(6, [(0, 2, 3)]), min_len=1, min_sep_threshold=50.0))
    for L in (63, 64, 65, 130):                                    # the selection's and the fold's strides of 64
        out.append(call(f"L={L}", crowd(rng, L + 2, 9, dt=0.1), drive(L + 2, [(0, 1, L + 1)], dt=0.1), dt=0.1, min_sep_threshold=50.0))
    out.append(call("first and last frame, two spans of one vehicle", crowd(rng, 20, 11),
                    drive(20, [(0, 0, 7), (0, 9, 20), (1, 3, 6), (1, 6 + 1, 20)], K=2), min_sep_threshold=50.0))
    out.append(call("T=1", crowd(rng, 1, 4, holes=False), drive(1, [(0, 0, 1)]), min_len=1, min_sep_threshold=50.0))
    out.append(call("T=1, recorded velocities", crowd(rng, 1, 4, holes=False), drive(1, [(0, 0, 1)]), min_len=1, min_sep_threshold=50.0,
                    ped_vel=rng.normal(0.0, 1.0, (1, 4, 2))))
    # absent in exactly one frame of the span: the first, the last, x only, a NaN velocity only; an infinity is not absence
    xy = crowd(rng, 10, 6, holes=False)
    vel = velocities(xy, None, 0.4) + 0.01
    xy[2, 0], xy[7, 1], xy[4, 2, 0] = np.nan, np.nan, np.nan
    vel[5, 3, 1] = np.nan
    out.append(call("absent in one frame", xy, drive(10, [(0, 2, 8)]), ped_vel=vel, min_sep_threshold=50.0))
    out.append(call("absent in one frame, fallback velocities", xy, drive(10, [(0, 2, 8)]), min_sep_threshold=50.0))
    xy = crowd(rng, 10, 3, holes=False)
    xy[9, 1] = np.nan                                             # leaves at the span's end: the fallback velocity of frame 8 is NaN
    out.append(call("the last present frame has no fallback velocity", xy, drive(10, [(0, 3, 9)]), min_sep_threshold=50.0))
    # the closest approach: exactly the threshold (kept), one ulp above it (far); attained twice
    ego = (np.zeros((1, 6, 2)), np.zeros((1, 6)), np.ones((1, 6)))
    xy = np.full((6, 3, 2), 20.0)
    xy[:, 0], xy[:, 1], xy[:, 2] = [30.0, 0.0], [0.0, 40.0], [6.0, 8.0]
    xy[3, 2], xy[3, 1], xy[4, 0] = [3.0, 4.0], [4.0, 3.0], [-5.0, 0.0]
    out.append(call("min_separation == threshold", xy, ego, min_sep_threshold=5.0))
    out.append(call("min_separation one ulp above the threshold", xy, ego, min_sep_threshold=float(np.nextafter(5.0, 0.0))))
    # order statistics: duplicates, all equal, the floor's edge, the free-walking mask, the goal's thresholds
    T = 8
    still = np.zeros((T, 6, 2)) + np.array([1.0, 2.0])
    vel = np.zeros((T, 6, 2))
    vel[:, 0, 0] = [1.0, 2.0, 2.0, 1.0, 3.0, 2.0, 1.0, 1.0]        # duplicates
    vel[:, 1, 1] = 0.7                                             # all equal
    vel[:, 2, 0] = FLOOR                                           # exactly the floor: floored
    vel[:, 3, 0] = np.nextafter(FLOOR, 1.0)                        # just above: kept
    vel[:, 4] = [[0.3 * t, 0.4] for t in range(T)]
    vel[:, 5] = 0.0
    still[:, 4] = np.array([1.0, 2.0]) + np.stack([np.linspace(0.0, 0.999e-3, T), np.zeros(T)], axis=1)   # net just below 1e-3
    still[:, 5] = np.array([1.0, 2.0]) + np.stack([np.linspace(0.0, 1.001e-3, T), np.zeros(T)], axis=1)   # ... just above
    ego = drive(T, [(0, 0, T)], speed=3.0)
    for q in (0.0, 1.0, 0.5, 0.85):
        out.append(call(f"order statistics, q={q}", still, ego, ped_vel=vel, min_sep_threshold=50.0, cruise_q=q))
    reach = fc.distances(ego[0][0], still)                         # [T, 6]
    order = np.sort(reach[:, 0])
    out.append(call("one free step", still, ego, ped_vel=vel, min_sep_threshold=50.0, cruise_q=0.5, free_distance=float(order[-2])))
    out.append(call("no free step", still, ego, ped_vel=vel, min_sep_threshold=50.0, cruise_q=0.5, free_distance=float(reach.max())))
    return out


def punched(rng, ego_xy, ego_psi, ego_vel):
    """aligned channels with random frames knocked out of one channel or another: several spans a vehicle, short ones too"""
    ego_xy, ego_psi, ego_vel = ego_xy.copy(), ego_psi.copy(), ego_vel.copy()
    K, T = ego_psi.shape
    for k in range(K):
        for _ in range(rng.integers(0, 4)):
            t = rng.integers(0, T)
            (ego_xy[k, :, 0], ego_xy[k, :, 1], ego_psi[k], ego_vel[k])[rng.integers(0, 4)][t:t + rng.integers(1, 3)] = np.nan
    return ego_xy, ego_psi, ego_vel


def fuzz_calls(seed=29, n=40):
    """the fuzz: 40 random clips (T <= 120, A <= 70, K <= 4), aligned, their channels punched"""
    rng = np.random.default_rng(seed + 1)
    out = []
    for i, clip in enumerate(fuzz_clips(seed, n)):
        ego = punched(rng, *align(clip)[:3])
        dt = align(clip)[3]
        mode = (None, "median", "quantile", "freewalk")[i % 4]
        out.append(call(f"fuzz {i}", clip["ped_xy"], ego, dt=dt, ped_vel=clip.get("ped_vel"), cruise=mode, cruise_q=(0.85, 0.5, 0.3)[i % 3],
                        min_sep_threshold=6.0))
    return out


def call_status_counts(calls):
    counts = np.zeros(4, int)
    for c in calls:
        kw = {k: c["kw"][k] for k in ("min_sep_threshold", "min_len") if k in c["kw"]}
        for s in candidate_spans(c["ped_xy"], c["ped_vel"], c["ego_xy"], c["ego_psi"], c["ego_vel"], c["dt"], **kw):
            counts[s["status"]] += 1
    return counts
