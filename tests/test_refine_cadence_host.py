"""The refinement cadence of the single solve (sleqp_amd/csrc/refine_cadence.h) through hipfact_debug_refine_cadence,
the pure host function that replays a script of events (no GPU): how many correction passes the solve graphs carry,
which solves take a residual, which leave their verdict to the next tree launch.  Every scenario states its outcome by
hand, and `Model` below restates the rule: the library's rows must equal the model's, row by row, on every scenario."""
import ctypes as C

import numpy as np
import pytest

FACTOR, SOLVE, VERDICT, JUDGE, RESET, SET_STEPS, SET_EVERY, SET_BACKOFF, SAVE, RESTORE, DEVICE_RESIDUAL = range(11)
COLS = ("defer", "unchecked", "key", "flush_first", "refine_inline", "inline_probe", "wc_hint", "interval", "since",
        "num_checked", "solve_seq", "ctl_pending", "decide_deferred", "num_refined", "num_passes", "seq_at_factor",
        "hint_seq_seen", "first_factor_seq", "last_checked", "unchecked_ok")
KNOBS = dict(steps=1, adaptive=1, every=8, backoff=2, max=64, lazy=1, hint=1)
GOOD = (1, 0, 0, 0.0, 1.0)  # done, status, iters, omega, tol: the first pass met a quarter of the tolerance


def ev(kind, flag=0, seq=-1, ctl=(0, 0, 0, 0.0, 0.0)):
    return (kind, flag, seq) + tuple(ctl)


def factor(seq=-1, ctl=GOOD, graphed=1):
    return ev(FACTOR, graphed, seq, ctl)


def solve(seq=-1, ctl=GOOD, tree=1, all_checked=0):
    return ev(SOLVE, tree + 2 * all_checked, seq, ctl)


def verdict(ctl=GOOD, continued=0):
    return ev(VERDICT, continued, 0, ctl)


class Model:
    """the rule, restated"""

    def __init__(self, **knobs):
        self.k = dict(KNOBS, **knobs)
        self.refine_inline, self.inline_probe, self.wc_hint = 1, 1, 0
        self.seq_at_factor, self.hint_seq_seen, self.first_factor_seq = 0, -1, -1
        self.interval, self.since, self.last_checked = 0, 0, 1
        self.num_checked = self.num_refined = self.num_passes = 0
        self.ctl_pending = self.decide_deferred = self.solve_seq = 0
        self.saved = None

    @staticmethod
    def sufficed(done, status, iters, omega, tol):
        return bool(done) and status == 0 and iters == 0 and omega <= 0.25 * tol

    def judge(self, well):
        self.wc_hint = int(well)
        self.refine_inline = 0 if well else max(self.refine_inline, min(self.k["steps"], 1))

    def unchecked_ok(self):
        k = self.k
        return int(k["steps"] == 0 or (k["adaptive"] and self.refine_inline == 0 and not self.inline_probe))

    def step(self, e):
        kind, flag, seq, ctl = int(e[0]), int(e[1]), int(e[2]), e[3:]
        k = self.k
        active = k["steps"] > 0 and k["adaptive"]
        defer = unchecked = key = flush = 0
        if kind == FACTOR:
            if flag:
                self.decide_deferred = 0
            self.ctl_pending = 0
            if self.first_factor_seq < 0:
                self.first_factor_seq = self.solve_seq
            if k["hint"] and active and seq > self.first_factor_seq and seq > self.hint_seq_seen:
                self.hint_seq_seen = seq
                self.wc_hint = int(self.sufficed(*ctl))
            self.refine_inline = 0 if (self.wc_hint and k["adaptive"]) else k["steps"]
            self.inline_probe = 1
            self.seq_at_factor = self.solve_seq
            self.since = 0
            self.interval = k["every"]
        elif kind == SOLVE:
            tree, all_checked = flag & 1, flag >> 1
            if active and self.inline_probe and self.solve_seq > self.seq_at_factor and seq == self.solve_seq:
                self.judge(self.sufficed(*ctl))
                self.inline_probe = 0
            defer = int(bool(k["lazy"] and active and self.refine_inline == 0 and tree))
            if self.interval < 1:
                self.interval = k["every"]
            unchecked = int(bool(not all_checked and defer and (not self.inline_probe or self.wc_hint) and self.interval > 1
                                 and self.since % self.interval != 0))
            if not all_checked and not unchecked and k["every"] > 1 and self.since >= self.interval and k["backoff"] > 1:
                self.interval = min(max(k["max"], k["every"]), self.interval * k["backoff"])
            self.since = self.since + 1 if unchecked else 1
            self.num_checked += int(not unchecked and k["steps"] > 0)
            self.last_checked = int(not unchecked)
            flush = int(not tree and self.decide_deferred)
            key = (-2 if defer else self.refine_inline) if k["steps"] > 0 else -1
            if flush:
                self.decide_deferred = 0
            if not unchecked:
                self.decide_deferred = defer
                self.solve_seq += int(k["steps"] > 0)
            self.ctl_pending = int(k["steps"] > 0 and (not unchecked or self.ctl_pending))
        elif kind == VERDICT:
            self.ctl_pending = 0
            if self.inline_probe and active:
                if self.sufficed(*ctl):
                    self.judge(True)
                self.inline_probe = 0
            iters = int(ctl[2])
            self.num_refined += int(iters > 0)
            self.num_passes += iters
            if flag > 0:
                self.refine_inline = min(max(self.refine_inline, iters), 4)
                self.wc_hint = 0
        elif kind == JUDGE:
            self.judge(flag)
        elif kind == RESET:
            self.solve_seq = self.seq_at_factor = self.ctl_pending = 0
        elif kind == SET_STEPS:
            k["steps"] = max(0, flag)
            self.refine_inline = k["steps"]
        elif kind in (SET_EVERY, SET_BACKOFF):
            k["every" if kind == SET_EVERY else "backoff"] = max(1, flag)
            self.interval = 0
        elif kind == SAVE:
            self.saved = (self.refine_inline, self.inline_probe, self.wc_hint, self.interval, self.since, self.last_checked,
                          self.num_checked, self.num_refined, self.num_passes)
        elif kind == RESTORE:
            ri, probe, wc = self.saved[:3]
            if not probe:  # (a factorisation not judged when saved keeps the judgement found since)
                self.refine_inline, self.wc_hint = ri, wc
            (self.interval, self.since, self.last_checked, self.num_checked, self.num_refined, self.num_passes) = self.saved[3:]
        elif kind == DEVICE_RESIDUAL:
            self.solve_seq += 1
        return (defer, unchecked, key, flush, self.refine_inline, self.inline_probe, self.wc_hint, self.interval, self.since,
                self.num_checked, self.solve_seq, self.ctl_pending, self.decide_deferred, self.num_refined, self.num_passes,
                self.seq_at_factor, self.hint_seq_seen, self.first_factor_seq, self.last_checked, self.unchecked_ok())


def run(lib, events, **knobs):
    """rows of the library as dicts, after they have been found equal to the model's"""
    k = dict(KNOBS, **knobs)
    kn = np.array([k[n] for n in ("steps", "adaptive", "every", "backoff", "max", "lazy", "hint")], dtype=np.int32)
    evs = np.ascontiguousarray(np.array(events, dtype=np.float64).reshape(-1, 8))
    out = np.full((len(events), len(COLS)), -77, dtype=np.int64)
    rc = lib.hipfact_debug_refine_cadence(kn.ctypes.data_as(C.c_void_p), len(events), evs.ctypes.data_as(C.c_void_p),
                                          out.ctypes.data_as(C.c_void_p))
    assert rc == 0, rc
    model = Model(**knobs)
    for i, e in enumerate(events):
        want = model.step(e)
        assert tuple(int(v) for v in out[i]) == tuple(int(v) for v in want), (i, e, dict(zip(COLS, out[i])), dict(zip(COLS, want)))
    return [dict(zip(COLS, (int(v) for v in r))) for r in out]


def well_conditioned_plan():
    """a first factorisation whose only solve is judged well-conditioned when its verdict is read: wc_hint is set"""
    return [factor(), solve(), verdict(GOOD)]


def checked_solves(rows):
    return [i + 1 for i, r in enumerate(rows) if not r["unchecked"]]


@pytest.mark.parametrize("backoff,want,interval", [(2, [1, 9, 25, 57, 121, 185], 64), (1, list(range(1, 200, 8)), 8)])
def test_check_interval_and_backoff(hipfact_lib, backoff, want, interval):
    # scenarios 1 and 2 (the figures test_residual_checked_on_every_kth_solve_only asserts on the device)
    head = well_conditioned_plan()
    events = head + [factor()] + [solve(seq=1)] * 200 + [factor()]
    rows = run(hipfact_lib, events, backoff=backoff)
    assert rows[len(head) - 1]["wc_hint"] == 1
    solves = rows[len(head) + 1:-1]
    assert checked_solves(solves) == want and len(want) == (6 if backoff == 2 else 25)
    assert solves[-1]["num_checked"] - rows[len(head)]["num_checked"] == len(want)
    assert solves[-1]["interval"] == interval
    assert all(r["defer"] and r["key"] == -2 and r["refine_inline"] == 0 for r in solves)
    assert rows[-1]["interval"] == 8 and rows[-1]["since"] == 0  # a new factorisation: back to refine_check_every


@pytest.mark.parametrize("late", [0, 1, 2, 3, 4, 5])
def test_first_factorisation_of_a_plan(hipfact_lib, late):
    # scenario 3: solve 1 carries the pass; its verdict is seen by the peek of solve 2 + late
    events = [factor()] + [solve(seq=0)] * (1 + late) + [solve(seq=1)] + [solve(seq=2 + late)] * 200
    rows = run(hipfact_lib, events)
    first = rows[1]
    assert first["key"] == 1 and first["refine_inline"] == 1 and not first["unchecked"] and not first["defer"]
    for r in rows[1:2 + late]:  # every solve before the verdict arrives: checked, with the pass, not deferred
        assert not r["unchecked"] and not r["defer"] and r["key"] == 1 and r["inline_probe"] == 1
    assert rows[2 + late - 1]["solve_seq"] == 1 + late
    # (the peek wants the verdict of the LAST checked solve: seq == solve_seq; with `late` > 0 the verdict of solve 1
    # is stale by then and the probe stays on until a peek matches)
    tail = rows[2 + late:]
    if late == 0:
        assert tail[0]["refine_inline"] == 0 and tail[0]["inline_probe"] == 0 and tail[0]["defer"] == 1
        # from there the cadence of scenario 1, counted from the last checked solve (solve 1)
        assert [i + 2 for i, r in enumerate(tail) if not r["unchecked"]] == [9, 25, 57, 121, 185]
    else:
        assert tail[0]["inline_probe"] == 1 and tail[0]["refine_inline"] == 1 and not tail[0]["unchecked"]
        assert tail[1]["inline_probe"] == 0 and tail[1]["refine_inline"] == 0 and tail[1]["defer"] == 1


@pytest.mark.parametrize("ctl", [(1, 0, 1, 0.0, 1.0), (1, 1, 0, 0.0, 1.0), (1, 0, 0, 0.26, 1.0)], ids=["iters", "status", "omega"])
def test_a_verdict_that_does_not_suffice(hipfact_lib, ctl):
    # scenario 4: one pass stays in the graph, every solve is checked; the next factorisation starts with refine_steps
    events = [factor(), solve()] + [solve(seq=i, ctl=ctl) for i in range(1, 30)] + [factor(seq=30, ctl=ctl)]
    for steps in (1, 2):
        rows = run(hipfact_lib, events, steps=steps)
        for r in rows[1:-1]:
            assert r["refine_inline"] == steps and r["key"] == steps and not r["unchecked"] and not r["defer"]
        assert rows[2]["inline_probe"] == 0 and rows[2]["wc_hint"] == 0
        assert rows[-2]["num_checked"] == 30 and rows[-2]["solve_seq"] == 30
        assert rows[-1]["refine_inline"] == steps and rows[-1]["inline_probe"] == 1 and rows[-1]["hint_seq_seen"] == 30


@pytest.mark.parametrize("old", [0, 1, 3])
@pytest.mark.parametrize("iters", [1, 2, 3, 4, 5, 6])
def test_verdict_read_after_host_continued_passes(hipfact_lib, old, iters):
    # scenario 5
    head = well_conditioned_plan() + [factor(), ev(SET_STEPS, old), solve()]
    rows = run(hipfact_lib, head + [verdict((1, 0, iters, 0.0, 1.0), continued=1)])
    assert rows[-2]["refine_inline"] == old
    last = rows[-1]
    assert last["refine_inline"] == min(max(old, iters), 4) and last["wc_hint"] == 0 and last["ctl_pending"] == 0
    assert last["num_refined"] == 1 and last["num_passes"] == iters
    # ... and without continued rounds the passes in the graph stay
    rows = run(hipfact_lib, head + [verdict((1, 0, iters, 0.0, 1.0), continued=0)])
    assert rows[-1]["refine_inline"] == old and rows[-1]["num_passes"] == iters


def test_factor_hint_peek(hipfact_lib):
    # scenario 6: one solve per factorisation; the verdict of solve k is back when factorisation k + 1 is queued
    events = [factor()]
    for k in range(1, 6):
        events += [solve(), factor(seq=k)]
    rows = run(hipfact_lib, events)
    assert [r["refine_inline"] for r in rows[0::2]] == [1, 0, 0, 0, 0, 0]  # dropped from the second factorisation on
    assert [r["key"] for r in rows[1::2]] == [1, -2, -2, -2, -2]
    assert all(not r["unchecked"] for r in rows[1::2])  # (the first solve of a factorisation is always checked)
    assert rows[-1]["hint_seq_seen"] == 5 and rows[-1]["first_factor_seq"] == 0
    # with the knob off the pass stays
    rows = run(hipfact_lib, events, hint=0)
    assert all(r["refine_inline"] == 1 for r in rows) and rows[-1]["hint_seq_seen"] == -1
    # a verdict not newer than first_factor_seq: the plan's first factorisation comes behind 3 solves of another plan
    # (here: RESET-free, three counted device residuals), whose verdict 3 is not this plan's
    rows = run(hipfact_lib, [ev(DEVICE_RESIDUAL)] * 3 + [factor(seq=3), solve(), factor(seq=3), solve(), factor(seq=4)])
    assert rows[3]["first_factor_seq"] == 3 and rows[3]["hint_seq_seen"] == -1 and rows[3]["refine_inline"] == 1
    assert rows[5]["hint_seq_seen"] == -1 and rows[5]["refine_inline"] == 1  # still nothing of its own
    assert rows[7]["hint_seq_seen"] == 4 and rows[7]["refine_inline"] == 0
    # a verdict not newer than hint_seq_seen is not looked at again: its judgement (bad, then overtaken by a judge(well)
    # of the solves) does not come back
    bad = (1, 0, 2, 0.0, 1.0)
    rows = run(hipfact_lib, [factor(), solve(), factor(seq=1, ctl=bad), ev(JUDGE, 1), factor(seq=1, ctl=bad), factor(seq=2, ctl=bad)])
    assert [r["wc_hint"] for r in rows[2:]] == [0, 1, 1, 0] and [r["refine_inline"] for r in rows[2:]] == [1, 0, 0, 1]


def test_other_knob_settings(hipfact_lib):
    # scenario 7
    script = well_conditioned_plan() + [factor(seq=1)] + [solve(seq=1)] + [solve(seq=2)] * 40
    rows = run(hipfact_lib, script, steps=0)
    assert all(r["key"] == -1 and not r["unchecked"] for r in rows if r["key"] != 0)
    assert all(r["num_checked"] == 0 and r["ctl_pending"] == 0 and r["solve_seq"] == 0 and r["unchecked_ok"] == 1 for r in rows)
    assert [r["key"] for r in rows].count(-1) == 42
    for knobs in (dict(adaptive=0), dict(lazy=0)):
        rows = run(hipfact_lib, script, **knobs)
        assert all(not r["defer"] and not r["unchecked"] and not r["decide_deferred"] for r in rows)
        assert rows[-1]["num_checked"] == 42
    assert all(r["refine_inline"] == 1 for r in run(hipfact_lib, script, adaptive=0))
    # a tree that does not deliver verdicts: never deferred, so never unchecked - and a verdict left by an earlier
    # solve is flushed first
    no_tree = well_conditioned_plan() + [factor(seq=1), solve(seq=1)] + [solve(seq=2, tree=0)] * 20
    rows = run(hipfact_lib, no_tree)
    assert rows[4]["defer"] == 1 and rows[4]["decide_deferred"] == 1
    assert rows[5]["flush_first"] == 1 and rows[5]["decide_deferred"] == 0
    assert all(not r["defer"] and not r["unchecked"] and r["key"] == 0 for r in rows[5:])
    assert all(not r["flush_first"] for r in rows[6:])


def test_save_and_restore_around_columns(hipfact_lib):
    # scenario 8.  Judged when saved: everything goes back, the live part advances
    head = well_conditioned_plan() + [factor(seq=1), solve(seq=1), solve(seq=2), solve(seq=2)]
    cols = [solve(seq=2, all_checked=1), verdict((1, 0, 2, 0.0, 1.0), continued=1), solve(seq=3, all_checked=1), verdict(GOOD)]
    rows = run(hipfact_lib, head + [ev(SAVE)] + cols + [ev(RESTORE)])
    before, inside, after = rows[len(head)], rows[-2], rows[-1]
    assert before["inline_probe"] == 0 and before["refine_inline"] == 0 and before["since"] == 3
    assert inside["refine_inline"] == 2 and inside["wc_hint"] == 0 and inside["num_checked"] == before["num_checked"] + 2
    assert all(not r["unchecked"] for r in rows[len(head) + 1:-1] if r["key"] != 0)
    for name in ("refine_inline", "inline_probe", "wc_hint", "interval", "since", "num_checked", "num_refined", "num_passes",
                 "last_checked"):
        assert after[name] == before[name], name
    assert after["solve_seq"] == before["solve_seq"] + 2 and after["ctl_pending"] == 0
    assert (after["seq_at_factor"], after["hint_seq_seen"]) == (before["seq_at_factor"], before["hint_seq_seen"])
    # the columns are the first solves of the factorisation (not judged when saved): the judgement found since stays,
    # and the probe flag is not put back; the check cadence and the counters do go back
    head = well_conditioned_plan() + [ev(JUDGE, 0), factor()]
    rows = run(hipfact_lib, head + [ev(SAVE), solve(all_checked=1), verdict(GOOD), solve(seq=2, all_checked=1), ev(RESTORE)])
    before, after = rows[len(head)], rows[-1]
    assert before["inline_probe"] == 1 and before["refine_inline"] == 1 and before["wc_hint"] == 0
    assert after["inline_probe"] == 0 and after["refine_inline"] == 0 and after["wc_hint"] == 1
    assert (after["since"], after["num_checked"], after["interval"]) == (before["since"], before["num_checked"], before["interval"])
    assert after["solve_seq"] == before["solve_seq"] + 2 and after["ctl_pending"] == 1 and after["decide_deferred"] == 1
    # ... an all_checked solve never grows the interval
    assert all(r["interval"] == 8 for r in rows[len(head):])


def test_option_setters(hipfact_lib):
    # scenario 9
    head = well_conditioned_plan() + [factor(seq=1), solve(seq=1)] + [solve(seq=2)] * 10
    rows = run(hipfact_lib, head + [ev(SET_EVERY, 3), solve(seq=3), solve(seq=3), solve(seq=3)])
    assert rows[len(head) - 1]["interval"] == 16 and rows[len(head)]["interval"] == 0
    # (3 solves since the last check: the reloaded interval of 3 is up at once, and doubles behind that check)
    assert rows[len(head) - 1]["since"] == 3
    assert [r["interval"] for r in rows[-3:]] == [6, 6, 6] and [r["unchecked"] for r in rows[-3:]] == [0, 1, 1]
    rows = run(hipfact_lib, head + [ev(SET_BACKOFF, 1), solve(seq=3)] + [solve(seq=3)] * 16)
    assert rows[len(head)]["interval"] == 0 and all(r["interval"] == 8 for r in rows[len(head) + 1:])
    assert checked_solves(rows[len(head) + 1:]) == [6, 14]  # (8 solves behind the check at solve 9 of the head, then every 8th)
    rows = run(hipfact_lib, head + [ev(SET_STEPS, 3), solve(seq=3), ev(SET_STEPS, 0), solve(seq=3), ev(SET_EVERY, -4), solve()])
    assert rows[len(head)]["refine_inline"] == 3 and rows[len(head) + 1]["key"] == 3 and not rows[len(head) + 1]["defer"]
    assert rows[len(head) + 2]["refine_inline"] == 0 and rows[len(head) + 3]["key"] == -1
    assert rows[-1]["interval"] == 1  # (the option's clamp)


def test_reset(hipfact_lib):
    # scenario 10
    head = well_conditioned_plan() + [factor(seq=1), solve(seq=1), solve(seq=2), solve(seq=2)]
    rows = run(hipfact_lib, head + [ev(RESET), solve()])
    before, after = rows[len(head) - 1], rows[len(head)]
    assert before["solve_seq"] == 2 and before["seq_at_factor"] == 1 and before["ctl_pending"] == 1
    assert (after["solve_seq"], after["seq_at_factor"], after["ctl_pending"]) == (0, 0, 0)
    for name in COLS[4:]:
        if name not in ("solve_seq", "seq_at_factor", "ctl_pending"):
            assert after[name] == before[name], name


def test_bad_input(hipfact_lib):
    lib = hipfact_lib
    good = np.array([1, 1, 8, 2, 64, 1, 1], dtype=np.int32)
    out = np.zeros((4, len(COLS)), dtype=np.int64)

    def call(knobs, events, n=None, rows=out):
        e = np.ascontiguousarray(np.array(events, dtype=np.float64).reshape(-1, 8))
        return lib.hipfact_debug_refine_cadence(knobs.ctypes.data_as(C.c_void_p) if knobs is not None else None,
                                                len(events) if n is None else n, e.ctypes.data_as(C.c_void_p),
                                                rows.ctypes.data_as(C.c_void_p) if rows is not None else None)

    assert call(good, [factor(), solve()]) == 0
    assert lib.hipfact_debug_refine_cadence(good.ctypes.data_as(C.c_void_p), 0, None, None) == 0
    assert call(None, [factor()]) == -1 and call(good, [factor()], rows=None) == -1 and call(good, [factor()], n=-1) == -1
    for q, v in ((0, -1), (1, 2), (2, 0), (3, 0), (4, 0), (5, 2), (6, -1)):
        bad = good.copy()
        bad[q] = v
        assert call(bad, [factor()]) == -1, (q, v)
    for e in (ev(11), ev(-1), ev(FACTOR, 2), ev(SOLVE, 4), ev(SOLVE, -1), ev(VERDICT, -1), ev(JUDGE, 2), ev(RESTORE),
              ev(0.5), ev(SOLVE, 1, 0.5), ev(SOLVE, 1, 1, (float("nan"), 0, 0, 0.0, 0.0)), ev(SOLVE, 1, float("inf"))):
        assert call(good, [factor(), e]) == -1, e
    assert call(good, [ev(SAVE), ev(RESTORE)]) == 0
