"""CPU: DeviceEngine.execute / execute_idle as a sequence of library calls.

The engine is built without a device (object.__new__) around a library stand-in that answers every launch from a script and appends each
call, with the arguments that matter, to ONE trace; _commit_window, _prefetch and _windowed_fields are stand-ins that append to the same
trace.  Every case writes out the whole trace, the returned statistics (without the three host timers) and ``_sorted_t`` afterwards."""

import logging
import types

import pytest

from parcels_amd import _hip
from parcels_amd.engine import DeviceEngine

INF = float("inf")
PROGRAM, SCLK = 2, 2400.0  # what every scripted launch reports as pk_exec_stats.program / .sclk_mhz


def _k(it, s):
    return (it << 32) | s


def launch(err=0, key=0, found=(), hits=(), paused=0, t_min_live=0.0, t_max_live=0.0, steps=100, attempts=7, kernel_ms=1.0, sort_ms=0.25,
           counts=None, raises=None):
    """One scripted launch: what pk_execute_end / pk_execute_rerun_keys leave in pk_exec_stats (found / hits: pk_execute_twe_report)."""
    return dict(err=err, key=key or (min(found) if found else 0), found=list(found), hits=list(hits), paused=paused, t_min_live=t_min_live,
                t_max_live=t_max_live, steps=steps, attempts=attempts, kernel_ms=kernel_ms, sort_ms=sort_ms, counts=counts or {}, raises=raises)


class _RecordingLib:
    """The library calls of DeviceEngine.execute, answered from a script of launches and recorded in `trace`."""

    def __init__(self, trace, script):
        self.trace, self.script, self.n = trace, list(script), 0

    def _fill(self, st_ref):
        s = self._last = self.script[self.n]
        self.n += 1
        if s["raises"] is not None:
            raise s["raises"]
        st = st_ref._obj
        st.first_error_iter, st.first_time_error_key, st.paused, st.launches = s["err"], s["key"], s["paused"], 1
        st.t_min_live, st.t_max_live, st.steps, st.attempts = s["t_min_live"], s["t_max_live"], s["steps"], s["attempts"]
        st.kernel_ms, st.sort_ms, st.program, st.sclk_mhz = s["kernel_ms"], s["sort_ms"], PROGRAM, SCLK
        for code, n in s["counts"].items():
            st.state_counts[code] = n
        return 0

    def pk_execute_begin(self, h, prm_ref):
        p = prm_ref._obj
        self.trace.append(("begin", p.reset_state, p.have_guess0, p.sort_by_cell, p.horizon_lo, p.horizon_hi, p.max_iters,
                           [p.twe_key[k] for k in range(p.twe_n)]))
        return 0

    def pk_execute_end(self, h, st_ref):
        self.trace.append(("end",))
        return self._fill(st_ref)

    def pk_execute_rerun_keys(self, h, cap, n, keys, st_ref):
        self.trace.append(("rerun_keys", cap, [keys[k] for k in range(n)]))
        return self._fill(st_ref)

    def pk_particles_checkpoint(self, h):
        self.trace.append(("checkpoint",))
        return 0

    def pk_particles_restore(self, h):
        self.trace.append(("restore",))
        return 0


class _ReportingLib(_RecordingLib):
    """... with pk_execute_twe_report: every unlisted failing sample of the last launch and the justification flags of the listed ones."""

    def pk_execute_twe_report(self, h, found, cap, nf, hit, n_listed):
        self.trace.append(("twe_report", n_listed))
        s = self._last
        for i, k in enumerate(s["found"]):
            found[i] = k
        nf._obj.value = len(s["found"])
        for i in range(n_listed):
            hit[i] = int(bool(s["hits"][i]))
        return 0


def _engine(script, report=True, windowed=False, plans=(), prefetched=()):
    """-> (engine, trace).  `plans`: what the _commit_window stand-in returns launch by launch, `prefetched`: the _prefetch stand-in."""
    trace = []
    eng = object.__new__(DeviceEngine)
    eng.lib = (_ReportingLib if report else _RecordingLib)(trace, script)
    eng.ctx = types.SimpleNamespace(check=lambda rc, what=None: None, handle=None)
    eng.fieldset, eng.field_ids = types.SimpleNamespace(fields={}), {}  # (make_params is the real one)
    eng.windowed, eng.exact_error_stop, eng.agree_min, eng.agree_codes, eng.device = windowed, True, None, None, None
    eng._sorted_t = None  # (as after __init__: host order)
    plans, prefetched = list(plans), list(prefetched)

    def commit_window(t_live, sign):
        trace.append(("commit", t_live, sign))
        return plans.pop(0)

    def prefetch(plan):
        trace.append(("prefetch", plan))
        return prefetched.pop(0) if prefetched else False

    def windowed_fields():
        trace.append(("windowed_fields",))
        return [types.SimpleNamespace(model=types.SimpleNamespace(time_flt=[0.0, 50.0, 100.0])),
                types.SimpleNamespace(model=types.SimpleNamespace(time_flt=[0.0, 60.0, 120.0]))]

    eng._commit_window, eng._prefetch, eng._windowed_fields = commit_window, prefetch, windowed_fields
    return eng, trace


def _stats(st):
    """The returned statistics without the three host timers (which must be there)."""
    st = dict(st)
    for k in ("commit_s", "prefetch_s", "wait_s"):
        assert st.pop(k) >= 0.0
    return st


def _expect(steps, attempts, kernel_ms, sort_ms, launches, first_error_iter=0, reran=0, time_error_keys=(), state_counts=None, **more):
    return dict(steps=steps, attempts=attempts, kernel_ms=kernel_ms, sort_ms=sort_ms, launches=launches, first_error_iter=first_error_iter,
                reran=reran, time_error_keys=list(time_error_keys), pack_ms=0.0, packs=0, sclk_mhz=SCLK, program=PROGRAM,
                state_counts=state_counts or {}, **more)


BEGIN0 = ("begin", 1, 0, 0, -INF, INF, 0, [])  # the first launch of a plain call: reset, no guess, no sort, no horizon, no limit, no keys
PF = ("prefetch", None)
END = ("end",)


# ---- 1 ------------------------------------------------------------------------------------------------------------------------------
def test_a_clean_launch_sorts_and_later_calls_within_resort_every_do_not():
    eng, trace = _engine([launch(), launch(), launch(), launch()])
    st = eng.execute([4], endtime=200.0, dt0=1.0, sort_by_cell=1, t_start=100.0, resort_every=500.0)
    assert trace == [("begin", 1, 0, 1, -INF, 600.0, 0, []), PF, END]
    assert _stats(st) == _expect(100, 7, 1.0, 0.25, 1) and eng.last_stats is st and eng._sorted_t == 100.0
    del trace[:]
    st = eng.execute([4], endtime=400.0, dt0=1.0, sort_by_cell=1, t_start=300.0, resort_every=500.0, have_guess0=1)
    assert trace == [("begin", 1, 1, 0, -INF, 800.0, 0, []), PF, END]  # 200 s after the sort: not again
    assert _stats(st) == _expect(100, 7, 1.0, 0.25, 1) and eng._sorted_t == 100.0
    del trace[:]
    eng.execute([4], endtime=800.0, dt0=1.0, sort_by_cell=1, t_start=700.0, resort_every=500.0)
    assert trace == [("begin", 1, 0, 1, -INF, 1200.0, 0, []), PF, END] and eng._sorted_t == 700.0
    del trace[:]
    eng.execute([4], endtime=800.0, dt0=1.0, sort_by_cell=1, resort_every=500.0)  # no t_start: maybe several launches; sorted, at an unknown time
    assert trace == [("checkpoint",), ("begin", 1, 0, 1, -INF, INF, 0, []), PF, END] and eng._sorted_t is None


# ---- 2 ------------------------------------------------------------------------------------------------------------------------------
def test_an_error_stop_repeats_the_launch_from_the_second_column_set():
    eng, trace = _engine([launch(err=3, counts={70: 3, 4: 9}), launch(err=3, counts={70: 1, 4: 11}, steps=30, attempts=2)])
    st = eng.execute([4], endtime=10.0, dt0=1.0)
    assert trace == [BEGIN0, PF, END, ("rerun_keys", 3, [])]
    assert _stats(st) == _expect(30, 2, 2.0, 0.5, 2, first_error_iter=3, reran=1, state_counts={70: 1, 4: 11})
    assert eng._sorted_t is None


# ---- 3 ------------------------------------------------------------------------------------------------------------------------------
def test_in_place_variables_repeat_from_the_checkpoint():
    eng, trace = _engine([launch(err=3), launch(err=3)])
    st = eng.execute([4], endtime=10.0, dt0=1.0, in_place_variables=True, have_guess0=1)
    assert trace == [("checkpoint",), ("begin", 1, 1, 0, -INF, INF, 0, []), PF, END,
                     ("restore",), ("begin", 1, 1, 0, -INF, INF, 3, []), PF, END]
    assert _stats(st) == _expect(100, 7, 2.0, 0.5, 2, first_error_iter=3, reran=1) and eng._sorted_t is None


# ---- 4 ------------------------------------------------------------------------------------------------------------------------------
def test_a_resort_horizon_cuts_the_pass_into_launches_in_both_directions():
    eng, trace = _engine([launch(paused=5, t_min_live=10.0, t_max_live=77.0), launch(steps=50, attempts=1, kernel_ms=2.0, sort_ms=0.5)])
    st = eng.execute([4], endtime=100.0, dt0=1.0, sort_by_cell=1, t_start=0.0, resort_every=10.0)
    assert trace == [("checkpoint",), ("begin", 1, 0, 1, -INF, 10.0, 0, []), PF, END, ("begin", 0, 1, 1, -INF, 20.0, 0, []), PF, END]
    assert _stats(st) == _expect(150, 8, 3.0, 0.75, 2) and eng._sorted_t == 10.0
    eng, trace = _engine([launch(paused=5, t_min_live=-1.0, t_max_live=90.0), launch()])
    eng.execute([4], endtime=0.0, dt0=-1.0, sort_by_cell=1, t_start=100.0, resort_every=10.0)
    assert trace == [("checkpoint",), ("begin", 1, 0, 1, 90.0, INF, 0, []), PF, END, ("begin", 0, 1, 1, 80.0, INF, 0, []), PF, END]
    assert eng._sorted_t == 90.0
    # |dt| and RK45_max_dt are lower bounds of the span; a call no longer than the span is one launch and takes no checkpoint
    eng, trace = _engine([launch()])
    eng.execute([4], endtime=30.0, dt0=5.0, sort_by_cell=1, t_start=0.0, resort_every=10.0, context={"RK45_max_dt": 40.0})
    assert trace == [("begin", 1, 0, 1, -INF, 40.0, 0, []), PF, END]


# ---- 5 ------------------------------------------------------------------------------------------------------------------------------
def test_the_span_doubles_when_the_horizon_stopped_every_particle():
    eng, trace = _engine([launch(paused=5, t_min_live=4.0), launch(paused=5, t_min_live=4.0), launch()])
    st = eng.execute([4], endtime=100.0, dt0=1.0, sort_by_cell=1, t_start=0.0, resort_every=10.0)
    assert trace == [("checkpoint",), ("begin", 1, 0, 1, -INF, 10.0, 0, []), PF, END, ("begin", 0, 1, 1, -INF, 14.0, 0, []), PF, END,
                     ("begin", 0, 1, 1, -INF, 24.0, 0, []), PF, END]
    assert _stats(st) == _expect(300, 21, 3.0, 0.75, 3) and eng._sorted_t == 4.0


# ---- 6 ------------------------------------------------------------------------------------------------------------------------------
def test_a_windowed_pass_commits_before_and_prefetches_during_each_launch():
    eng, trace = _engine([launch(paused=3, t_min_live=40.0), launch()], windowed=True, plans=[{"U": 2}, {"U": None}], prefetched=[True, False])
    st = eng.execute([4], endtime=100.0, dt0=1.0)
    assert trace == [("checkpoint",), ("commit", 0.0, 1), BEGIN0, ("prefetch", {"U": 2}), END,
                     ("commit", 40.0, 1), ("begin", 0, 1, 0, -INF, INF, 0, []), ("prefetch", {"U": None}), END]
    assert _stats(st) == _expect(200, 14, 2.0, 0.5, 2) and eng._sorted_t is None
    # backwards without a start time: from the last level of any windowed field
    eng, trace = _engine([launch()], windowed=True, plans=[{}])
    eng.execute([4], endtime=0.0, dt0=-1.0, t_start=float("nan"))
    assert trace == [("checkpoint",), ("windowed_fields",), ("commit", 120.0, -1), BEGIN0, ("prefetch", {}), END]


def test_a_stalled_pass_without_a_span_is_an_error():
    # nobody moved, but a level was on its way: go on; nobody moved and nothing is on its way: the step does not fit
    script = [launch(paused=3, t_min_live=40.0), launch(paused=3, t_min_live=40.0), launch(paused=3, t_min_live=40.0)]
    eng, trace = _engine(script, windowed=True, plans=[{"U": 2}] * 3, prefetched=[True, True, False])
    with pytest.raises(RuntimeError) as e:
        eng.execute([4], endtime=100.0, dt0=1.0, t_start=5.0)
    assert str(e.value) == ("field window too small: a single step does not fit into the resident time levels; "
                            "increase nslots (FieldSet.to_device(nslots=...))")
    nxt = ("begin", 0, 1, 0, -INF, INF, 0, [])
    assert trace == [("checkpoint",), ("commit", 5.0, 1), BEGIN0, ("prefetch", {"U": 2}), END, ("commit", 40.0, 1), nxt, ("prefetch", {"U": 2}), END,
                     ("commit", 40.0, 1), nxt, ("prefetch", {"U": 2}), END]
    eng, trace = _engine([launch(paused=3, t_min_live=40.0)])
    with pytest.raises(_hip.HipLibraryError) as e:
        eng.execute([4], endtime=100.0, dt0=1.0, t_start=5.0)
    assert str(e.value) == "particles paused although all time levels are resident (internal error)"
    assert trace == [BEGIN0, PF, END]


# ---- 7 ------------------------------------------------------------------------------------------------------------------------------
def test_a_pass_that_will_be_repeated_anyway_is_cut_after_the_launch_that_shows_it():
    k, k2 = _k(5, 1), _k(8, 2)
    script = [launch(found=[k], paused=5, t_min_live=10.0),                  # pass 1 is cut after its first launch
              launch(found=[k2], hits=[False], paused=5, t_min_live=10.0),   # pass 2 too: the listed key counts as justified
              launch(hits=[True, False], paused=5, t_min_live=10.0), launch(hits=[False, True])]  # pass 3: both launches, flags OR-ed
    eng, trace = _engine(script)
    st = eng.execute([4], endtime=100.0, dt0=1.0, sort_by_cell=1, t_start=0.0, resort_every=10.0)
    assert trace == [("checkpoint",), ("begin", 1, 0, 1, -INF, 10.0, 0, []), PF, END, ("twe_report", 0),
                     ("restore",), ("begin", 1, 0, 1, -INF, 10.0, 0, [k]), PF, END, ("twe_report", 1),
                     ("restore",), ("begin", 1, 0, 1, -INF, 10.0, 0, [k, k2]), PF, END, ("twe_report", 2),
                     ("begin", 0, 1, 1, -INF, 20.0, 0, [k, k2]), PF, END, ("twe_report", 2)]
    assert _stats(st) == _expect(200, 14, 4.0, 1.0, 4, reran=2, time_error_keys=[k, k2]) and eng._sorted_t == 10.0
    # an error stop cuts the pass as well (a library without the report: no report call)
    eng, trace = _engine([launch(err=3, paused=5, t_min_live=10.0), launch(err=3)], report=False)
    st = eng.execute([4], endtime=100.0, dt0=1.0, sort_by_cell=1, t_start=0.0, resort_every=10.0)
    assert trace == [("checkpoint",), ("begin", 1, 0, 1, -INF, 10.0, 0, []), PF, END, ("restore",), ("begin", 1, 0, 1, -INF, 10.0, 3, []), PF, END]
    assert _stats(st) == _expect(100, 7, 2.0, 0.5, 2, first_error_iter=3, reran=1)


# ---- 8 ------------------------------------------------------------------------------------------------------------------------------
def test_a_library_without_the_report_lists_one_key_per_pass():
    a, b = _k(9, 1), _k(4, 2)
    eng, trace = _engine([launch(key=a), launch(key=b), launch()], report=False)
    st = eng.execute([4], endtime=10.0, dt0=1.0)
    assert trace == [BEGIN0, PF, END, ("rerun_keys", 0, [a]), ("rerun_keys", 0, [b])]  # the earlier sample drops the later one
    assert _stats(st) == _expect(100, 7, 3.0, 0.75, 3, reran=2, time_error_keys=[b])
    a, b = _k(4, 1), _k(9, 2)
    eng, trace = _engine([launch(key=a), launch(key=b), launch()], report=False)
    st = eng.execute([4], endtime=10.0, dt0=1.0)
    assert trace == [BEGIN0, PF, END, ("rerun_keys", 0, [a]), ("rerun_keys", 0, [a, b])] and st["time_error_keys"] == [a, b]


# ---- 9 ------------------------------------------------------------------------------------------------------------------------------
def test_every_key_of_a_pass_is_listed_at_once_and_validated_by_the_next():
    k1, k2, k3 = _k(5, 0), _k(5, 1), _k(6, 0)
    eng, trace = _engine([launch(found=[k1, k2, k3]), launch(hits=[True, False, True]), launch(hits=[True, True])])
    st = eng.execute([4], endtime=10.0, dt0=1.0)
    assert trace == [BEGIN0, PF, END, ("twe_report", 0), ("rerun_keys", 0, [k1, k2, k3]), ("twe_report", 3),
                     ("rerun_keys", 0, [k1, k3]), ("twe_report", 2)]
    assert _stats(st) == _expect(100, 7, 3.0, 0.75, 3, reran=2, time_error_keys=[k1, k3])
    # without speculation: the first problem of a pass only
    script = [launch(found=[k1, k2, k3]), launch(found=[k2, k3], hits=[True]), launch(found=[k3], hits=[True, True]), launch(hits=[True] * 3)]
    eng, trace = _engine(script)
    saved = DeviceEngine.TWE_SPECULATIVE_PASSES
    DeviceEngine.TWE_SPECULATIVE_PASSES = 0
    try:
        st = eng.execute([4], endtime=10.0, dt0=1.0)
    finally:
        DeviceEngine.TWE_SPECULATIVE_PASSES = saved
    assert trace == [BEGIN0, PF, END, ("twe_report", 0), ("rerun_keys", 0, [k1]), ("twe_report", 1), ("rerun_keys", 0, [k1, k2]), ("twe_report", 2),
                     ("rerun_keys", 0, [k1, k2, k3]), ("twe_report", 3)]
    assert _stats(st) == _expect(100, 7, 4.0, 1.0, 4, reran=3, time_error_keys=[k1, k2, k3])


# ---- 10 -----------------------------------------------------------------------------------------------------------------------------
def test_without_the_exact_error_stop_there_is_one_pass_and_no_agreement():
    agree = _Agreement([])
    eng, trace = _engine([launch(err=3, found=[_k(5, 1)], counts={70: 2})])
    eng.exact_error_stop, eng.agree_min, eng.agree_codes = False, agree, agree.codes
    st = eng.execute([4], endtime=10.0, dt0=1.0, in_place_variables=True)
    assert trace == [BEGIN0, PF, END] and agree.calls == []
    assert _stats(st) == _expect(100, 7, 1.0, 0.25, 1, state_counts={70: 2})  # first_error_iter 0, no codes_any_shard
    assert eng.execute_idle() == dict(steps=0, attempts=0, kernel_ms=0.0, sort_ms=0.0, launches=0, first_error_iter=0, reran=0,
                                      time_error_keys=[], state_counts={}) and agree.calls == []


# ---- 11 -----------------------------------------------------------------------------------------------------------------------------
def test_more_call_wide_time_errors_than_the_library_lists():
    many = [_k(20 + i // 8, i % 8) for i in range(_hip.PK_MAX_TWE)]
    eng, trace = _engine([launch(found=many), launch(found=[_k(999, 0)], hits=[True] * len(many))])
    with pytest.raises(RuntimeError) as e:
        eng.execute([4], endtime=10.0, dt0=1.0)
    assert str(e.value) == "more than 1024 call-wide time errors in one Kernel.execute"
    assert trace == [BEGIN0, PF, END, ("twe_report", 0), ("rerun_keys", 0, many), ("twe_report", len(many))]


# ---- 12 -----------------------------------------------------------------------------------------------------------------------------
class _Agreement:
    """A recording agree_min: answers from a list of agreed (err, key) -- and, `with_keys`, agreed (found, hits) -- values."""

    def __init__(self, mins, keys=None, raises=None):
        self.mins, self.calls, self.raises = list(mins), [], raises
        if keys is not None:
            answers = list(keys)

            def agree_keys(found, hits):
                self.calls.append(("keys", found, list(hits)))
                return answers.pop(0)

            self.keys = agree_keys

    def __call__(self, err, key, failed=False):
        self.calls.append(("min", err, key, failed))
        if failed:
            if self.raises is not None:
                raise self.raises
            return 0, 0
        return self.mins.pop(0)

    def codes(self, present):
        self.calls.append(("codes", list(present)))
        return [1, 0, 0, 0, 0, 1]


K = _k(5, 3)
AGREED = {
    # another rank finds K in pass 1; the validation pass (K listed: no shortcut) finds nothing new, and K is justified elsewhere
    "keys": dict(mins=[(0, K), (0, 0)], keys=[([K], []), ([], [True])], script=[launch(), launch(hits=[False])],
                 calls=[("min", 0, 0, False), ("keys", [], []), ("min", 0, 0, False), ("keys", [], [False]), ("codes", [0] * 6)],
                 trace=[BEGIN0, PF, END, ("rerun_keys", 0, [K]), ("twe_report", 1)], cap=0, listed=[K], reran=1),
    # the same through an agreement of the older form (no .keys): the smallest key only, every listed one taken as justified
    "no_keys": dict(mins=[(0, K), (0, 0)], keys=None, script=[launch(), launch(hits=[False])],
                    calls=[("min", 0, 0, False), ("min", 0, 0, False), ("codes", [0] * 6)],
                    trace=[BEGIN0, PF, END, ("rerun_keys", 0, [K]), ("twe_report", 1)], cap=0, listed=[K], reran=1),
    # .keys that cannot validate (a rank without the report): one key per pass as well
    "unvalidated": dict(mins=[(0, K), (0, 0)], keys=[(None, None), (None, None)], script=[launch(), launch(hits=[False])],
                        calls=[("min", 0, 0, False), ("keys", [], []), ("min", 0, 0, False), ("keys", [], [False]), ("codes", [0] * 6)],
                        trace=[BEGIN0, PF, END, ("rerun_keys", 0, [K]), ("twe_report", 1)], cap=0, listed=[K], reran=1),
    # an error stop elsewhere and no failing sample anywhere: ONE agreement per pass, .keys is never asked
    "shortcut": dict(mins=[(3, 0), (3, 0)], keys=[], script=[launch(), launch()],
                     calls=[("min", 0, 0, False), ("min", 0, 0, False), ("codes", [0] * 6)],
                     trace=[BEGIN0, PF, END, ("rerun_keys", 3, [])], cap=3, listed=[], reran=1),
}


@pytest.mark.parametrize("name", sorted(AGREED))
def test_an_empty_shard_takes_the_same_agreements_as_a_rank_that_finds_nothing(name):
    c = AGREED[name]
    agree = _Agreement(c["mins"], c["keys"])
    eng, trace = _engine(c["script"])
    eng.agree_min, eng.agree_codes = agree, agree.codes
    st = eng.execute([4], endtime=10.0, dt0=1.0)
    assert trace == c["trace"] and agree.calls == c["calls"]
    assert _stats(st) == _expect(100, 7, 2.0, 0.5, 2, first_error_iter=c["cap"], reran=1, time_error_keys=c["listed"], codes_any_shard=[70, 50])

    idle = _Agreement(c["mins"], c["keys"])
    eng, trace = _engine([])
    eng.agree_min, eng.agree_codes = idle, idle.codes
    st = eng.execute_idle()
    assert trace == [] and idle.calls == c["calls"]
    assert st == dict(steps=0, attempts=0, kernel_ms=0.0, sort_ms=0.0, launches=0, first_error_iter=c["cap"], reran=1,
                      time_error_keys=c["listed"], state_counts={}, codes_any_shard=[70, 50])


def test_a_rank_with_particles_hands_its_own_findings_to_the_agreement():
    k1, k2 = _k(5, 0), _k(6, 0)
    agree = _Agreement([(0, k1), (0, 0)], keys=[([k1, k2], []), ([], [True, True])])
    eng, trace = _engine([launch(found=[k2], counts={70: 4}), launch(hits=[False, True], counts={70: 4})])
    eng.agree_min, eng.agree_codes = agree, agree.codes
    st = eng.execute([4], endtime=10.0, dt0=1.0)
    assert agree.calls == [("min", 0, k2, False), ("keys", [k2], []), ("min", 0, 0, False), ("keys", [], [False, True]),
                           ("codes", [1, 0, 0, 0, 0, 0])]
    assert trace == [BEGIN0, PF, END, ("twe_report", 0), ("rerun_keys", 0, [k1, k2]), ("twe_report", 2)]
    assert st["time_error_keys"] == [k1, k2] and st["codes_any_shard"] == [70, 50]
    # a rank whose library cannot report hands None: nothing of its pass validates a listing
    agree = _Agreement([(0, k2), (0, 0)], keys=[(None, None), (None, None)])
    eng, trace = _engine([launch(key=k2), launch()], report=False)
    eng.agree_min, eng.agree_codes = agree, agree.codes
    eng.execute([4], endtime=10.0, dt0=1.0)
    assert agree.calls == [("min", 0, k2, False), ("keys", None, []), ("min", 0, 0, False), ("keys", None, [True]), ("codes", [0] * 6)]


# ---- 13 -----------------------------------------------------------------------------------------------------------------------------
def test_a_pass_that_raises_meets_the_other_ranks_in_the_failure_agreement(caplog):
    boom = ValueError("boom")
    agree = _Agreement([])
    eng, trace = _engine([launch(raises=boom)])
    eng.agree_min, eng.agree_codes = agree, agree.codes
    with pytest.raises(ValueError) as e:
        eng.execute([4], endtime=10.0, dt0=1.0)
    assert e.value is boom and agree.calls == [("min", 0, 0, True)] and trace == [BEGIN0, PF, END]
    # the agreement raises as well: logged, and the first exception is the one that propagates
    agree = _Agreement([], raises=KeyError("second"))
    eng, trace = _engine([launch(raises=boom)])
    eng.agree_min = agree
    with caplog.at_level(logging.WARNING, logger="parcels_amd"):
        with pytest.raises(ValueError) as e:
            eng.execute([4], endtime=10.0, dt0=1.0)
    assert e.value is boom and agree.calls == [("min", 0, 0, True)]
    assert [r.getMessage() for r in caplog.records] == ["the failure agreement of a collective run raised as well: KeyError('second')"]
    # without the exact error stop nobody waits in an agreement
    agree = _Agreement([])
    eng, trace = _engine([launch(raises=boom)])
    eng.agree_min, eng.exact_error_stop = agree, False
    with pytest.raises(ValueError):
        eng.execute([4], endtime=10.0, dt0=1.0)
    assert agree.calls == []
    # only the launches are guarded: what the settlement raises comes after the agreement of the pass, which every rank attended
    many = [_k(20 + i // 8, i % 8) for i in range(_hip.PK_MAX_TWE)]
    agree = _Agreement([(0, many[0]), (0, _k(999, 0))], keys=[(many, []), ([_k(999, 0)], [True] * len(many))])
    eng, trace = _engine([launch(found=many), launch(found=[_k(999, 0)], hits=[True] * len(many))])
    eng.agree_min = agree
    with pytest.raises(RuntimeError, match="more than 1024 call-wide time errors"):
        eng.execute([4], endtime=10.0, dt0=1.0)
    assert [c[:1] + c[3:] for c in agree.calls] == [("min", False), ("keys",), ("min", False), ("keys",)]
