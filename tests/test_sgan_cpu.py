"""Social-GAN sample generation (fot_sgan_*), the part that needs no GPU: the NumPy float64 restatement
(tests/sgan_common.py) against the reference fixture; csrc/fot_sgan.hpp -- the arithmetic, the blob layout and the device
image the kernels use -- built with g++ as a stand-alone program, against the fixture under the accuracy bound; BatchNorm
folding; the C ABI; the refusals that need no device; the needs_history hand-over of BatchedClosedLoop."""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest

import sgan_common as sc
from closed_loop_common import OracleEngine, OracleResampler
from conftest import ROOT
from integrated_path_planning_amd import _abi
from integrated_path_planning_amd.closed_loop import BatchedClosedLoop
from integrated_path_planning_amd.prediction import SganWeights, fold_batch_norm

EMU_DIR = os.path.join(ROOT, "tests", "emu")
EMU_EXE = os.path.join(EMU_DIR, "_build", "fot_sgan_emu")
CSRC = os.path.join(ROOT, "integrated_path_planning_amd", "csrc")
NAMES = tuple(sc.CASES)
EDGES = tuple(sc.EDGE_CASES)


@pytest.fixture(scope="module")
def fix():
    return sc.load_fixture()


@pytest.fixture(scope="module")
def edge_fix():
    return sc.load_fixture(sc.EDGE_FIXTURE)


def case_weights(name):
    a = sc.case_args(name)
    return SganWeights.from_state_dict(a, sc.seeded_state(a, sc.case_seed(name), sc.case_scale(name)))


# ---- the fixture and the restatement ---------------------------------------------------------------------------------------
def test_fixture_holds_what_the_tests_need(fix):
    meta = json.loads(str(fix["meta"]))
    assert set(meta) == set(NAMES)
    combos = {(bool(c[1]), c[2], c[3], c[4]) for c in sc.CASES.values()}
    assert len(combos) == 16                                        # pooling x pool_every_timestep x mix x batch_norm
    assert {tuple(c[5]) for c in sc.CASES.values()} >= {(1, 3, 7), (2,), (0, 5, 0), (1, 3, 65)}
    assert {c[6] for c in sc.CASES.values()} >= {1, 3, 64}
    assert {c[0] for c in sc.CASES.values()} == set(sc.DIMS)
    assert sc.CASES["c_big_pool_step_ped_bn"][5:7] == ([2, 5], 2)
    for name in NAMES:
        m = meta[name]
        assert m["seed"] == sc.case_seed(name) and 0.3 <= m["largest_step"] <= 2.0, name
        obs, off, noise, r32, r64 = sc.fixture_case(fix, name)
        want = sc.case_inputs(name)
        for got, w in zip((obs, off, noise), want):
            np.testing.assert_array_equal(got, w)
        assert r32.dtype == np.float32 and r64.dtype == np.float64 and r32.shape == r64.shape
    assert not any("weight" in k for k in fix)                      # the tests rebuild the weights from the seed
    assert os.path.getsize(sc.FIXTURE) < 1_000_000


@pytest.mark.parametrize("name", NAMES)
def test_restatement_matches_the_reference_in_float64(fix, name):
    a = sc.case_args(name)
    obs, off, noise, _, r64 = sc.fixture_case(fix, name)
    got = sc.restate(a, sc.seeded_state(a, sc.case_seed(name), sc.case_scale(name)), obs, off, noise)
    assert got.shape == r64.shape
    assert np.max(np.abs(got - r64)) <= 1e-10


# ---- BatchNorm folding -----------------------------------------------------------------------------------------------------
def folded(state):
    out = {k: v for k, v in state.items()}
    for k in [k for k in state if k.endswith(".running_mean")]:
        bn = k[:-len(".running_mean")]
        seq, i = bn.rsplit(".", 1)
        lin = f"{seq}.{int(i) - 1}"
        out[lin + ".weight"], out[lin + ".bias"] = fold_batch_norm(state[lin + ".weight"], state[lin + ".bias"], state[bn + ".weight"],
                                                                   state[bn + ".bias"], state[bn + ".running_mean"], state[bn + ".running_var"])
        for suffix in (".weight", ".bias", ".running_mean", ".running_var", ".num_batches_tracked"):
            del out[bn + suffix]
    return out


@pytest.mark.parametrize("name", [n for n in NAMES if sc.CASES[n][4]])
def test_batch_norm_folds_into_the_linear_in_front(fix, name):
    a = sc.case_args(name)
    state = sc.seeded_state(a, sc.case_seed(name), sc.case_scale(name))
    plain = folded(state)
    assert not any("running" in k for k in plain) and any("running" in k for k in state)
    obs, off, noise, _, r64 = sc.fixture_case(fix, name)
    assert np.max(np.abs(sc.restate(a, plain, obs, off, noise) - r64)) <= 1e-9
    # the loader folds the same way: the blob of the folded state is the blob of the state with BatchNorm
    np.testing.assert_array_equal(SganWeights.from_state_dict(a, plain).blob, SganWeights.from_state_dict(a, state).blob)
    assert SganWeights.from_state_dict(a, state).blob.dtype == np.float32


# ---- csrc/fot_sgan.hpp on the CPU -----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def emu():
    srcs = [os.path.join(EMU_DIR, "fot_sgan_emu.cpp"), os.path.join(CSRC, "fot_sgan.hpp"), os.path.join(ROOT, "include", "fot.h")]
    if not os.path.exists(EMU_EXE) or os.path.getmtime(EMU_EXE) < max(os.path.getmtime(s) for s in srcs):
        os.makedirs(os.path.dirname(EMU_EXE), exist_ok=True)
        subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-o", EMU_EXE, srcs[0]], check=True)

    def run(w, off, obs, S, noise, tmp_path):
        inp, outp = str(tmp_path / "case.bin"), str(tmp_path / "out.bin")
        sc.write_emu_case(inp, bytes(w.desc), w.blob, off, obs, S, noise)
        subprocess.run([EMU_EXE, inp, outp], check=True)
        return np.fromfile(outp, dtype=np.float32).reshape(S, w.desc.pred_len, int(off[-1]), 2)
    return run


@pytest.mark.parametrize("name", NAMES)
def test_emulation_is_within_the_accuracy_bound(fix, emu, tmp_path, name):
    obs, off, noise, r32, r64 = sc.fixture_case(fix, name)
    got = emu(case_weights(name), off, obs, noise.shape[0], noise, tmp_path)
    err, bound = float(np.max(np.abs(got.astype(np.float64) - r64))), sc.accuracy_bound(r32, r64)
    print(f"{name}: error {err:.3e}, bound {bound:.3e}, ratio {err / bound:.3f}")
    assert err <= bound


def test_emulation_refuses_what_the_library_refuses(emu, tmp_path):
    w = case_weights("a_none_ped")
    obs, off, noise = sc.case_inputs("a_none_ped")
    inp = str(tmp_path / "bad.bin")
    d = _abi.SganDesc.from_buffer_copy(bytes(w.desc))
    d.pooling_type = _abi.SGAN_SPOOL
    sc.write_emu_case(inp, bytes(d), w.blob, off, obs, 1, noise[:1])
    assert subprocess.run([EMU_EXE, inp, str(tmp_path / "o.bin")], capture_output=True).returncode == 3
    sc.write_emu_case(inp, bytes(w.desc), w.blob[:-1], off, obs, 1, noise[:1])
    assert subprocess.run([EMU_EXE, inp, str(tmp_path / "o.bin")], capture_output=True).returncode == 3


# ---- the edge table: lengths, dimensions and scene sizes at the kernels' tile boundaries ------------------------------------
def test_edge_fixture_holds_every_edge_the_kernels_have(edge_fix):
    """The edges of csrc/fot_sgan.hip, by name: an edit of sgan_common.EDGE_CASES cannot drop one unnoticed."""
    meta = json.loads(str(edge_fix["meta"]))
    assert set(meta) == set(EDGES) and not set(EDGES) & set(NAMES)
    E = sc.EDGE_CASES
    step = lambda c: bool(c["every"] and c["pooling"])
    has = lambda pred: any(pred(c) for c in E.values())
    # lengths
    assert {c["obs_len"] for c in E.values()} >= {1, 2, 32} and {c["pred_len"] for c in E.values()} >= {1, 32}
    assert has(lambda c: c["pred_len"] == 32 and step(c)) and has(lambda c: c["pred_len"] == 32 and not step(c))
    # dimensions (embedding, encoder h, decoder h, mlp, bottleneck, noise)
    assert has(lambda c: c["dims"] == (1, 1, 2, 1, 1, 1))
    pooled_b = {c["dims"][4] for c in E.values() if c["pooling"]}
    assert pooled_b >= {1, 8, 9, 1024}
    assert has(lambda c: c["dims"][4] == 9 and step(c) and max(c["scenes"]) >= 16)
    assert {c["dims"][2] for c in E.values()} >= {2, 64, 65, 128} and has(lambda c: c["dims"][1:3] == (1, 128))
    assert has(lambda c: c["dims"][2] == 65 and c["S"] * sum(c["scenes"]) > 16)       # a second LSTM tile at H > 64
    assert {c["dims"][3] for c in E.values()} >= {1, 256, 257, 1024}
    assert has(lambda c: c["dims"][5] == c["dims"][2] - 1 and c["dims"][5] > 1)       # a context of one
    assert has(lambda c: c["dims"][5] == 0 and c["dims"][1] != c["dims"][2] and not c["pooling"])
    assert has(lambda c: c["dims"] == sc.DIMS["c"] and c["scenes"] == [17] and step(c))
    # scene sizes and rows
    assert has(lambda c: c["scenes"] == [15, 16, 17, 31, 32, 33] and step(c))
    assert has(lambda c: c["scenes"] == [15, 16, 17, 31, 32, 33] and not step(c))
    assert has(lambda c: c["scenes"] == [_abi.SGAN_MAX_PEDS, 1] and c["dims"] == sc.DIMS["a"] and c["S"] == 1 and step(c))
    rows = {c["S"] * sum(c["scenes"]) for c in E.values() if step(c)}
    assert rows >= {4, 5, 16, 17} and E["rows_16"]["S"] == 2 and E["rows_16"]["scenes"] == [8]
    small = [c for c in E.values() if len(c["scenes"]) >= 40 and set(c["scenes"]) == {0, 1, 2} and c["mix"] == "global"]
    assert small and small[0]["scenes"][0] == 0 and small[0]["scenes"][-1] == 0
    assert has(lambda c: c["S"] == _abi.MAX_SAMPLES == 64 and c["scenes"] == [17] and step(c))
    assert {c["inputs"] for c in E.values()} == {None, "stationary", "coincident", "far"}
    for name in EDGES:
        m, c = meta[name], E[name]
        assert m["seed"] == sc.case_seed(name) and m["scale"] == c["scale"] in (1.5, 2.0, 2.5, 3.0), name
        assert 0.3 <= m["largest_step"] <= 2.0 and m["e_ref"] > 0.0, name
        assert m["args"] == {**sc.case_args(name), "noise_dim": list(sc.case_args(name)["noise_dim"])}, name
        obs, off, noise, r32, r64 = sc.fixture_case(edge_fix, name)
        for got, w in zip((obs, off, noise), sc.case_inputs(name)):
            np.testing.assert_array_equal(got, w)
        assert r32.dtype == np.float32 and r64.dtype == np.float64
        assert r32.shape == r64.shape == (c["S"], c["pred_len"], sum(c["scenes"]), 2) and obs.shape[0] == c["obs_len"]
        assert np.isfinite(r64).all()
    # the inputs with exact zeros are what they say
    obs = sc.case_inputs("in_stationary")[0]
    assert np.all(obs[:, 0] == obs[0, 0]) and not np.all(obs[:, 1] == obs[0, 1])
    obs = sc.case_inputs("in_coincident")[0]
    assert np.array_equal(obs[:, 0], obs[:, 1]) and not np.array_equal(obs[:, 0], obs[:, 2])
    assert np.min(np.abs(sc.case_inputs("in_far")[0])) > 1.9e4
    assert not any("weight" in k for k in edge_fix)
    assert os.path.getsize(sc.EDGE_FIXTURE) < 1_000_000


@pytest.mark.parametrize("name", EDGES)
def test_edge_restatement_matches_the_reference_in_float64(edge_fix, name):
    a = sc.case_args(name)
    obs, off, noise, _, r64 = sc.fixture_case(edge_fix, name)
    got = sc.restate(a, sc.seeded_state(a, sc.case_seed(name), sc.case_scale(name)), obs, off, noise)
    assert got.shape == r64.shape
    assert np.max(np.abs(got - r64)) <= 1e-10


@pytest.mark.parametrize("name", EDGES)
def test_edge_restatement_in_float32_is_within_the_accuracy_bound(edge_fix, name):
    """The reference's own operations in float32, in NumPy's order instead of torch's, stay under the bound: it is a fair
    one for a float32 implementation at these shapes."""
    a = sc.case_args(name)
    obs, off, noise, r32, r64 = sc.fixture_case(edge_fix, name)
    got = sc.restate(a, sc.seeded_state(a, sc.case_seed(name), sc.case_scale(name)), obs, off, noise, np.float32)
    assert got.dtype == np.float32
    err, bound = float(np.max(np.abs(got.astype(np.float64) - r64))), sc.accuracy_bound(r32, r64)
    print(f"{name}: error {err:.3e}, bound {bound:.3e}, ratio {err / bound:.3f}")
    assert err <= bound


@pytest.mark.parametrize("name", EDGES)
def test_edge_emulation_is_within_the_accuracy_bound(edge_fix, emu, tmp_path, name):
    obs, off, noise, r32, r64 = sc.fixture_case(edge_fix, name)
    got = emu(case_weights(name), off, obs, noise.shape[0], noise, tmp_path)
    err, bound = float(np.max(np.abs(got.astype(np.float64) - r64))), sc.accuracy_bound(r32, r64)
    print(f"{name}: error {err:.3e}, bound {bound:.3e}, ratio {err / bound:.3f}")
    assert err <= bound


def test_edge_blob_lengths():
    for name in EDGES:
        a = sc.case_args(name)
        rc, n = _count(SganWeights.descriptor(a))
        assert rc == _abi.OK and n == _blob_length(a) == case_weights(name).blob.size, name


# ---- the C ABI ----------------------------------------------------------------------------------------------------------------
SGAN_SYMBOLS = ("fot_sgan_weight_count", "fot_sgan_load", "fot_sgan_unload", "fot_sgan_sample")


def test_library_exports_the_sgan_entry_points_and_abi_words():
    lib = _abi.lib()
    header = open(os.path.join(ROOT, "include", "fot.h")).read()
    for sym in SGAN_SYMBOLS:
        assert hasattr(lib, sym), f"{sym} not exported by libfot.so"
        assert sym in _abi.SYMBOLS
        assert re.search(r"\bint\s+" + sym + r"\s*\(", header), f"{sym} not declared in include/fot.h"
    assert _abi.ABI_VERSION == 8 and re.search(r"#define FOT_ABI_VERSION 8\b", header)
    defs = {k: int(v) for k, v in re.findall(r"#define (FOT_[A-Z_]+) (\d+)\b", header)}
    got = (C.c_int32 * 64)()
    n = lib.fot_abi_info(64, got)
    assert n == defs["FOT_ABI_INFO_WORDS"] == len(_abi.ABI_WORD_NAMES) == 35
    words = dict(zip(_abi.ABI_WORD_NAMES, got[:n]))
    assert words["sizeof(fot_sgan_desc)"] == C.sizeof(_abi.SganDesc) == 56
    for name, mirror in (("FOT_SGAN_MAX_EMBEDDING", _abi.SGAN_MAX_EMBEDDING), ("FOT_SGAN_MAX_HIDDEN", _abi.SGAN_MAX_HIDDEN),
                         ("FOT_SGAN_MAX_MLP", _abi.SGAN_MAX_MLP), ("FOT_SGAN_MAX_BOTTLENECK", _abi.SGAN_MAX_BOTTLENECK),
                         ("FOT_SGAN_MAX_OBS_LEN", _abi.SGAN_MAX_OBS_LEN), ("FOT_SGAN_MAX_PEDS", _abi.SGAN_MAX_PEDS),
                         ("FOT_SGAN_POOL_HIDDEN", _abi.SGAN_POOL_HIDDEN)):
        assert words[name] == defs[name] == mirror, name
    assert (defs["FOT_SGAN_MAX_EMBEDDING"], defs["FOT_SGAN_MAX_HIDDEN"], defs["FOT_SGAN_MAX_MLP"], defs["FOT_SGAN_MAX_BOTTLENECK"],
            defs["FOT_SGAN_MAX_OBS_LEN"], defs["FOT_SGAN_POOL_HIDDEN"]) == (64, 128, 1024, 1024, 32, 512)
    assert defs["FOT_SGAN_MAX_PEDS"] >= 128
    for name, mirror in (("FOT_SGAN_POOL_NONE", _abi.SGAN_POOL_NONE), ("FOT_SGAN_POOL_NET", _abi.SGAN_POOL_NET),
                         ("FOT_SGAN_SPOOL", _abi.SGAN_SPOOL), ("FOT_SGAN_NOISE_PED", _abi.SGAN_NOISE_PED),
                         ("FOT_SGAN_NOISE_GLOBAL", _abi.SGAN_NOISE_GLOBAL), ("FOT_SGAN_OBS_DEVICE", _abi.SGAN_OBS_DEVICE),
                         ("FOT_SGAN_NOISE_DEVICE", _abi.SGAN_NOISE_DEVICE), ("FOT_OUT_DEVICE", _abi.OUT_DEVICE)):
        assert defs[name] == mirror, name


def test_ctypes_mirror_of_the_descriptor_matches_c(tmp_path):
    lines = ['  printf("%zu\\n", sizeof(fot_sgan_desc));\n']
    lines += [f'  printf("%zu\\n", offsetof(fot_sgan_desc, {n}));\n' for n, _ in _abi.SganDesc._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "fot.h"\nint main(void) {\n' + "".join(lines) + "  return 0; }\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [C.sizeof(_abi.SganDesc)] + [getattr(_abi.SganDesc, n).offset for n, _ in _abi.SganDesc._fields_]


# ---- refusals that need no device ------------------------------------------------------------------------------------------
def _count(desc):
    n = C.c_int64(-1)
    return _abi.lib().fot_sgan_weight_count(C.byref(desc), C.byref(n)), n.value


def _blob_length(a):
    """The packed blob's length from the documented order (include/fot.h), counted here."""
    e, he, hd, m, nd = a["embedding_dim"], a["encoder_h_dim"], a["decoder_h_dim"], a["mlp_dim"], a["noise_dim"][0]
    b = a["bottleneck_dim"] if a["pooling_type"] else 0
    lstm = lambda h: 3 * e + 4 * h * (e + h) + 8 * h
    pool = lambda h: 3 * e + 512 * (e + h) + 512 + b * 512 + b
    mlp = lambda k, o: m * k + m + o * m + o
    n = lstm(he) + lstm(hd) + 2 * hd + 2
    if a["pooling_type"]:
        n += pool(he)
    if sc.needs_context(a):
        n += mlp(he + b, hd - nd)
    if sc.pools_every_step(a):
        n += pool(hd) + mlp(hd + b, hd)
    return n


def test_weight_count_and_the_refusals_that_need_no_device():
    for name in NAMES:
        a = sc.case_args(name)
        rc, n = _count(SganWeights.descriptor(a))
        assert rc == _abi.OK and n == _blob_length(a) == case_weights(name).blob.size, name
    base = sc.case_args("a_pool_step_ped_bn")
    for change, code in ((dict(pooling_type="spool"), _abi.ERR_UNSUPPORTED), (dict(dropout=0.1), _abi.ERR_UNSUPPORTED),
                         (dict(num_layers=2), _abi.ERR_UNSUPPORTED), (dict(embedding_dim=65), _abi.ERR_UNSUPPORTED),
                         (dict(encoder_h_dim=129), _abi.ERR_UNSUPPORTED), (dict(decoder_h_dim=129), _abi.ERR_UNSUPPORTED),
                         (dict(mlp_dim=1025), _abi.ERR_UNSUPPORTED), (dict(bottleneck_dim=1025), _abi.ERR_UNSUPPORTED),
                         (dict(obs_len=33), _abi.ERR_UNSUPPORTED), (dict(pred_len=_abi.MAX_PRED_LEN + 1), _abi.ERR_UNSUPPORTED),
                         (dict(embedding_dim=0), _abi.ERR_INVALID), (dict(obs_len=0), _abi.ERR_INVALID),
                         (dict(noise_dim=(32,)), _abi.ERR_INVALID), (dict(noise_dim=(-1,)), _abi.ERR_INVALID),
                         (dict(num_layers=0), _abi.ERR_INVALID)):
        rc, n = _count(SganWeights.descriptor({**base, **change}))
        assert rc == code and n == -1, change
        assert _abi.lib().fot_last_error(None)
    # the capacities themselves are accepted
    rc, _ = _count(SganWeights.descriptor({**base, "embedding_dim": 64, "encoder_h_dim": 128, "decoder_h_dim": 128, "mlp_dim": 1024,
                                           "bottleneck_dim": 1024, "obs_len": 32, "pred_len": _abi.MAX_PRED_LEN}))
    assert rc == _abi.OK
    d = SganWeights.descriptor(base)
    d.pooling_type = 3
    assert _count(d)[0] == _abi.ERR_INVALID
    d = SganWeights.descriptor(base)
    d.noise_mix_type = 2
    assert _count(d)[0] == _abi.ERR_INVALID
    lib = _abi.lib()
    assert lib.fot_sgan_weight_count(None, None) == _abi.ERR_INVALID
    # no handle: nothing is read
    off = np.zeros(1, np.int32)
    assert lib.fot_sgan_sample(None, 0, off.ctypes.data, None, 1, None, 0, None, None) == _abi.ERR_INVALID
    assert lib.fot_sgan_load(None, C.byref(SganWeights.descriptor(base)), 0, None) == _abi.ERR_INVALID
    assert lib.fot_sgan_unload(None) == _abi.ERR_INVALID


def test_python_loader_refusals():
    a = sc.case_args("a_none_ped")
    w = case_weights("a_none_ped")
    with pytest.raises(ValueError, match="blob holds"):
        SganWeights(w.desc, w.blob[:-1])
    with pytest.raises(ValueError, match="one entry"):
        SganWeights.descriptor({**a, "noise_dim": (4, 4)})
    with pytest.raises(ValueError, match="pooling_type"):
        SganWeights.descriptor({**a, "pooling_type": "attention"})
    with pytest.raises(_abi.FotError) as e:
        SganWeights(SganWeights.descriptor({**a, "pooling_type": "spool"}), w.blob)
    assert e.value.code == _abi.ERR_UNSUPPORTED
    state = sc.seeded_state(a, 1)
    del state["decoder.hidden2pos.weight"]
    with pytest.raises(KeyError):
        SganWeights.from_state_dict(a, state)
    # a checkpoint's own argument names (trajectory_predictor.py:91-92) and the reference's defaults
    d = SganWeights.descriptor({"encoder_h_dim_g": 48, "decoder_h_dim_g": 96})
    assert (d.encoder_h_dim, d.decoder_h_dim, d.obs_len, d.pred_len, d.embedding_dim, d.mlp_dim, d.bottleneck_dim, d.noise_dim,
            d.pooling_type, d.pool_every_timestep, d.noise_mix_type) == (48, 96, 8, 12, 64, 1024, 1024, 8, _abi.SGAN_POOL_NET, 1, 0)
    assert "never" in SganWeights.from_checkpoint.__doc__.lower()


def test_from_checkpoint_reads_a_file_as_the_reference_loader_does(tmp_path):
    """A file written here with torch.save in the released checkpoints' form: {'args': ..., 'g_state' | 'g_best_state': ...},
    the hidden sizes under their _g-suffixed names (trajectory_predictor.py:91-92), args a mapping or an object."""
    import argparse
    import torch
    name = "dim_nd0_he_ne_hd"                                        # encoder and decoder sizes differ: a swap of the two shows
    a = sc.case_args(name)
    assert a["encoder_h_dim"] != a["decoder_h_dim"]
    state = sc.seeded_state(a, sc.case_seed(name), sc.case_scale(name))
    want = SganWeights.from_state_dict(a, state)
    tensors = {k: torch.from_numpy(np.asarray(v)).to(torch.int64 if np.asarray(v).dtype == np.int64 else torch.float32)
               for k, v in state.items()}
    suffixed = {k: v for k, v in a.items() if k not in ("encoder_h_dim", "decoder_h_dim")}
    suffixed.update(encoder_h_dim_g=a["encoder_h_dim"], decoder_h_dim_g=a["decoder_h_dim"], noise_type="uniform", d_type="local")
    for i, (args, key) in enumerate(((suffixed, "g_state"), (argparse.Namespace(**suffixed), "g_state"),
                                     (suffixed, "g_best_state"), (argparse.Namespace(**a), "g_best_state"))):
        path = tmp_path / f"ckpt{i}.pt"
        torch.save({"args": args, key: tensors, "d_state": {}, "counters": {"t": 3}}, str(path))
        got = SganWeights.from_checkpoint(str(path))
        assert bytes(got.desc) == bytes(want.desc), i
        np.testing.assert_array_equal(got.blob, want.blob)
        assert got.noise_type == ("gaussian" if i == 3 else "uniform")
    # g_state wins where a file holds both (trajectory_predictor.py:124-128)
    other = {k: v + 1 if v.dtype == torch.float32 else v for k, v in tensors.items()}
    torch.save({"args": suffixed, "g_state": tensors, "g_best_state": other}, str(tmp_path / "both.pt"))
    np.testing.assert_array_equal(SganWeights.from_checkpoint(str(tmp_path / "both.pt")).blob, want.blob)
    torch.save({"args": suffixed}, str(tmp_path / "none.pt"))
    with pytest.raises(KeyError):
        SganWeights.from_checkpoint(str(tmp_path / "none.pt"))


# ---- the needs_history hand-over ---------------------------------------------------------------------------------------------
class _WindowSource:
    """A sample source that asks for the observer's window and answers with constant-velocity samples."""
    needs_history = True

    def __init__(self, n_samples, pred_len):
        self.n_samples, self.pred_len, self.calls = n_samples, pred_len, []

    def __call__(self, window, ped_off):
        self.calls.append((window.copy(), np.array(ped_off)))
        vel = window[-1] - window[-2]
        steps = np.arange(1, self.pred_len + 1, dtype=np.float64)[None, :, None, None]
        spread = 1.0 + 0.05 * np.arange(self.n_samples, dtype=np.float64)[:, None, None, None]
        return window[-1][None, None].astype(np.float64) + spread * steps * vel[None, None].astype(np.float64)


def test_a_source_with_needs_history_is_handed_the_window():
    from pred_scores_common import load_cases
    fix = load_cases()
    ep = fix["meta"]["episodes"]["weave_s4"]
    cfg = dict(ep["config"])
    # the wall collides within two seconds; an episode without pedestrians; the recorded episode outlives both
    tracks = [sc.charging_wall_tracks(), fix["weave_s4_ped_traj"][:, :0], fix["weave_s4_ped_traj"]]
    src = _WindowSource(3, cfg["pred_len"])
    sim = BatchedClosedLoop(cfg, tracks, engine=OracleEngine(cfg), resampler=OracleResampler(cfg), sample_source=src)
    widths = [t.shape[1] for t in tracks]
    assert widths[1] == 0 and widths[0] > 0 and widths[2] > 0
    seen_all = seen_fewer = False
    for _ in range(40):
        before = len(src.calls)
        alive = np.flatnonzero(sim.alive)
        if sim.step() == 0:
            break
        if len(src.calls) == before:
            continue                                                # (the observer is still filling)
        window, off = src.calls[-1]
        want_off = np.concatenate([[0], np.cumsum([widths[e] for e in alive])])
        np.testing.assert_array_equal(off, want_off)
        assert off.dtype == np.int32 and window.dtype == np.float32 and window.shape == (cfg["obs_len"], want_off[-1], 2)
        rows = sim._rows_of(alive)
        np.testing.assert_array_equal(window, np.stack([h[rows] for h in sim.observer.history]).astype(np.float32))
        seen_all |= len(alive) == 3
        seen_fewer |= len(alive) == 2 and 0 not in alive
        if seen_fewer:
            break
    assert seen_all and seen_fewer and sim.episodes[0].termination_reason == "collision"


def test_a_source_without_the_attribute_is_called_as_before():
    from pred_scores_common import load_cases
    fix = load_cases()
    cfg = dict(fix["meta"]["episodes"]["s4_eps0"]["config"])
    calls = []

    def source(last, prev):
        calls.append((last.shape, prev.shape))
        return np.stack([last + (k + 1) * (last - prev) for k in range(cfg["pred_len"])])[None].repeat(2, axis=0)

    sim = BatchedClosedLoop(cfg, [fix["s4_eps0_ped_traj"]], engine=OracleEngine(cfg), resampler=OracleResampler(cfg),
                            sample_source=source)
    for _ in range(3):
        sim.step()
    p = fix["s4_eps0_ped_traj"].shape[1]
    assert calls and all(c == ((p, 2), (p, 2)) for c in calls)
