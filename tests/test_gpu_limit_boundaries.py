"""Limits placed at value (1 + delta) of a candidate's own extreme, through plan(): every kinematic and stop decision of
the plan kernels at its threshold -- the counterpart of tests/test_gpu_collision_boundary.py for every other decision.

Random inputs almost never put a candidate within 1e-6 of a limit, and the candidate costs do not see curvature,
lateral acceleration or step length: a limit read from the wrong instance, a rule that reads sample 0, a dropped last
or held sample, a stale predecessor at a cut of the time range or a curvature off by 1e-8 would pass the rest of the
suite.  Here the threshold of a chosen (candidate, rule) is the ORACLE's extreme of the rule's quantity times
(1 + delta), delta in +-{1e-3, 1e-5, 1e-7, 1e-9, 1e-10, 1e-11}; tests/limit_boundaries_common.py says how each threshold
is steered (overrides per instance, scenarios for road width and step length, the ego speed for the brake-ladder gate),
which samples the targets are chosen to be decided at (k = 1, the last kept sample, a held sample of the brake ladder, a
step across a cut of the 4-segment walk -- for both pairwise rules, the step length and the yaw cap --, k >= 64 in the
76-sample scenes; its COVERAGE table lists every reachable (rule, case) and is asserted), and what is left out on purpose (the
0.5 m/s gate of the curvature rule, the singularity and EPS_S_DOT truncations).  All instances of a scene go into ONE
launch, ordered so that neighbours carry different overrides and target candidates.

Judges, per instance, under every evaluation path (EVAL_PATHS) in the lean form ("auto") and the general form forced:
  1. n_cand, n_t, keep and the status table are the oracle's (eps_band.check_status_table); the record matches the
     oracle's, stats included;
  2. the records are byte-identical across all paths and forms;
  3. fot_debug_margins, on every target: the candidate's margin in the rule's group is |delta| to within 1 % of |delta|
     + 2 dev (where, by the oracle's arrays, another comparison of the group on that candidate comes closer to its
     threshold than the target's own, that comparison's margin instead: under a fifth of the targets, asserted).
A delta is used on a target only at |delta| >= 10 dev, dev the relative difference between the library's own value of
the quantity (candidate_path) and the oracle's; every target must keep all |delta| >= 1e-9 (asserted), and in every scene
at least a fifth of the instances change a status against the obstacle-free table (asserted).

Measured on an MI355X (profiles/r16_limit_boundaries.json; no share is asserted for 1e-10 / 1e-11): 686 instances in the
eight scenes and 12 at the gate, 5584 instance evaluations over the paths and forms, 0 differences; every target keeps
every |delta| down to 1e-11 (share retained 1.0 at each delta); worst dev per rule: speed 5.2e-16, accel 1.1e-15,
curvature 2.3e-14, lat_accel 9.7e-14, yaw_cap 6.6e-14, road 4.1e-15, step 1.9e-14, travel 0, v_last 1.0e-14, gate 0;
the target's own comparison decides 92 - 100 % of the margins of a scene.
Each assertion message names scene, instance, rule, candidate, deciding samples, delta, path and form.
"""
import json
import os

import numpy as np
import pytest

import eps_band
import limit_boundaries_common as lb
# (an arc and a line heading 0.4 rad: no path here is exactly straight, so no launch takes a flat kernel -- asserted after
# each plan call -- and helpers' "-noflat" names would repeat "group" and "split-wave")
from helpers import EVAL_PATHS_NEVER_FLAT as EVAL_PATHS, assert_no_flat_launch, assert_record_matches_oracle, set_eval_path
from integrated_path_planning_amd import _abi
from integrated_path_planning_amd.planner import BatchPlanner

pytestmark = pytest.mark.gpu

FORMS = ("auto", "general")


@pytest.fixture(scope="module")
def emu():
    return lb.Emu()                      # (host code only: the tile tables' cut positions)


def rec_bytes(rec):
    return bytes(memoryview(rec).cast("B"))


class Handle:
    """One library handle of a scene: scenario 0 the scene's own planner, one more per distinct scenario of its
    instances."""

    def __init__(self, sc):
        self.sc = sc
        self.bp = BatchPlanner(waypoints=sc.waypoints, **sc.kw)
        self.ids = {}

    def lib_paths(self, req):
        """c -> [15, n_t] of the candidates of `req` as the library's debug path generates them."""
        self.bp.plan_batch([req])
        cache = {}

        def get(c):
            if c not in cache:
                fp = self.bp.candidate_path(c, 0)
                cache[c] = np.array([getattr(fp, f) for f in _abi.PATH_FIELDS])
            return cache[c]
        return get

    def place(self, insts):
        for inst in insts:
            key = tuple(sorted(inst.kw.items()))
            if key and key not in self.ids:
                self.ids[key] = self.bp.add_scenario(waypoints=self.sc.waypoints, **dict(self.sc.kw, **inst.kw))
            inst.req.scenario = self.ids[key] if key else 0

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.bp.close()


def scene_instances(sc, h):
    insts, picked, _ = lb.build(sc, h.lib_paths(sc.request()))
    lb.assert_coverage(sc, insts, picked)
    lists = list(picked.values())
    if "v_last" in sc.rules:
        more, ts = lb.v_last_scene_targets(
            sc, lambda target: h.lib_paths(sc.request(target_speed=target, max_stop_distance=1.0e3)))
        insts, lists = insts + more, lists + [ts]
    h.place(insts)
    return insts, lists


def write_report(name, payload):
    """The scene's figures as JSON into the directory FOT_LIMIT_REPORT_DIR names, if it is set (they are printed anyway)."""
    out = os.environ.get("FOT_LIMIT_REPORT_DIR")
    if not out:
        return
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, f"limit_boundaries_{name}.json"), "w") as f:
        json.dump(payload, f, indent=1)


CAP = 1024                               # candidates per instance the debug queries are sized for (the scenes hold < 450)


class Tables:
    """The debug tables of instance i of the last plan call, fetched once and sized for these scenes.  It stands in for
    the planner in eps_band.check_status_table, which asks it for margins(i): so these instances enter the suite's
    eps-band report -- on purpose: its smallest margins then say how close to a threshold a status has been HELD to
    the oracle's, about 1e-11 in every group steered here (DESIGN section 2 says so next to the regular runs' figures)."""

    def __init__(self, bp, i):
        self.i = i
        self.m = bp.margins(i, cap=CAP)
        _, self.status, self.keep, self.nt = bp.candidates(i, cap=CAP)

    def margins(self, inst):
        assert inst == self.i
        return self.m

    def check(self, label, n_cand, want):
        lb.check_tables(label, (n_cand, self.status, self.keep, self.nt), want,
                        lambda got, exp, l: eps_band.check_status_table(self, self.i, got, exp, l))


def judge(sc, bp, insts, res, lab, applied, first):
    """first: the records of the first (path, form), already held to the oracle's -- byte equality with them then IS the
    record judge of this one."""
    for i, inst in enumerate(insts):
        label = f"{sc.name} inst {i} [{lab}] {inst.label()}"
        tab = Tables(bp, i)
        tab.check(label, res.records[i].n_cand, inst.want)
        if first is None:
            assert_record_matches_oracle(res.records[i], inst.want, label=label)
        else:
            assert rec_bytes(res.records[i]) == first[i], f"{label}: record differs from [{EVAL_PATHS[0]}, {FORMS[0]}]'s"
        lb.check_margins(sc, inst, tab.m, label, applied)


@pytest.mark.parametrize("name", list(lb.SCENES))
def test_limits_at_the_boundary_match_the_oracle(emu, name):
    sc = lb.Scene(name, emu)
    with Handle(sc) as h:
        insts, lists = scene_instances(sc, h)
        share, worst = lb.retained(lists)
        changed = lb.changed_share(sc, insts)
        print(f"\n{name}: {len(insts)} instances, targets retained per |delta| {share}, worst dev per rule {worst}")
        assert changed >= 0.2, f"{name}: {changed:.0%} of the instances change a status"
        for inst in insts:
            lb.check_kind(sc, inst)
        reqs = [inst.req for inst in insts]
        first, applied = None, [0, 0]
        for path in EVAL_PATHS:
            set_eval_path(h.bp, path)
            for form in FORMS:
                h.bp.set_eval_form(form)
                res = h.bp.plan_batch(reqs)
                took = h.bp.last_eval_form()
                lean_ok = form == "auto" and sc.n_total <= 64
                assert took == ("lean" if lean_ok else "general"), f"{name} [{path}, {form}]: the launch took the {took} form"
                assert_no_flat_launch(h.bp, f"{name} [{path}, {form}]")
                judge(sc, h.bp, insts, res, f"{path}, {form}", applied, first)
                if first is None:
                    first = [rec_bytes(res.records[i]) for i in range(len(insts))]
        assert applied[0] >= 0.8 * applied[1], \
            f"{name}: the target's own comparison decides {applied[0]} of {applied[1]} margins only"
        write_report(name, {"scene": name, "instances": len(insts), "targets": sum(len(l) for l in lists),
                            "evaluations": len(insts) * len(EVAL_PATHS) * len(FORMS), "retained_share": share,
                            "worst_dev": worst, "changed_share": changed,
                            "margins_decided_by_the_target": applied[0] / max(applied[1], 1)})


def test_brake_ladder_gate(emu):
    """Ego speeds at which the oracle's s_d is 0.1 (1 + delta), one launch: the ladder (n_cand) is there exactly above
    the gate, the tables are the oracle's."""
    sc = lb.Scene("fast", emu)
    insts = lb.gate_instances(sc)
    assert len(insts) >= 10
    worst, used = 0.0, 0
    with Handle(sc) as h:
        for path in EVAL_PATHS:
            set_eval_path(h.bp, path)
            for form in FORMS:
                h.bp.set_eval_form(form)
                res = h.bp.plan_batch([inst.req for inst in insts])
                assert_no_flat_launch(h.bp, f"gate [{path}, {form}]")
                for i, inst in enumerate(insts):
                    label = f"gate inst {i} [{path}, {form}] {inst.label()}"
                    rec = res.records[i]
                    dev = abs(rec.frenet0[1] - inst.want.frenet0[1]) / 0.1
                    worst = max(worst, dev)
                    assert 10.0 * dev <= lb.FLOOR_MAX, f"{label}: s_d differs from the oracle's by {dev:.3e} relative"
                    if abs(inst.delta) < 10.0 * dev:
                        continue
                    used += 1
                    Tables(h.bp, i).check(label, rec.n_cand, inst.want)
                    assert_record_matches_oracle(rec, inst.want, label=label)
    print(f"\ngate: {len(insts)} instances, {used} evaluations judged, worst dev of s_d {worst:.3e}")
    write_report("gate", {"scene": "gate", "instances": len(insts), "targets": len(insts), "evaluations": used,
                          "retained_share": {}, "worst_dev": {"gate": worst}, "changed_share": 0.5})


def test_mixed_launch_gives_the_per_scene_records(emu):
    """Instances of the road and step-length scenarios and of the override scenes (limits, stop filter, yaw cap) in one
    plan_batch on one handle: byte for byte the records of the per-scene launches."""
    names = ("fast", "stop", "yaw", "yaw_slow", "road", "step")
    scenes = {n: lb.Scene(n, emu) for n in names}
    subsets, want = {}, {}
    for n, sc in scenes.items():
        with Handle(sc) as h:
            insts, _ = scene_instances(sc, h)
            sub = insts[:: max(1, len(insts) // 10)][:12]
            res = h.bp.plan_batch([inst.req for inst in sub])
            subsets[n], want[n] = sub, [rec_bytes(res.records[i]) for i in range(len(sub))]
            for i, inst in enumerate(sub):
                assert_record_matches_oracle(res.records[i], inst.want, label=f"{n} inst {i} {inst.label()}")
    base = scenes["fast"]
    order = []
    for n in names:                       # every scenario of the other scenes, the scene's own planner included
        for j, inst in enumerate(subsets[n]):
            inst.kw = {k: v for k, v in dict(scenes[n].kw, **inst.kw).items() if base.kw.get(k) != v}
            order.append((n, j))
    order = [order[i] for i in np.random.default_rng(5).permutation(len(order))]
    insts = [subsets[n][j] for n, j in order]
    with Handle(base) as mixed:
        mixed.place(insts)
        assert len(mixed.ids) >= 10 and len({inst.req.scenario for inst in insts}) >= 10
        for path in EVAL_PATHS:
            set_eval_path(mixed.bp, path)
            res = mixed.bp.plan_batch([inst.req for inst in insts])
            assert_no_flat_launch(mixed.bp, f"mixed [{path}]")
            for i, (n, j) in enumerate(order):
                assert rec_bytes(res.records[i]) == want[n][j], \
                    f"mixed inst {i} [{path}] = {n} inst {j} {insts[i].label()}: record differs from the per-scene launch's"
