"""Built-in interaction kernels (kernels.AttractTowards, kernels.MergeNearest) on the device-resident particle columns.

A kernel list with a Python function runs in the host loop (parcels_amd/hostkernels.py): every iteration uploads every particle
column, launches the built-in kernels' bodies, downloads every column, and a kernel written on ``pa.neighbors`` sends x, y, z up again
and brings a pair list back.  A list of built-in kernels and interaction tokens needs none of that.  ``launch_device`` drives the same
loop (reference: src/parcels/_core/kernel.py:188-230; hostkernels.execute_hosted lines 192-240 restate it on the host columns) from the
host with every column staying in HBM.  One iteration:

1. prologue kernel (pk_interact_prologue): the ``evaluate_particles`` mask into the column body_only launches read it from, dt clipped
   for every row;
2. runs of built-in kernels: ``pk_execute`` with ``body_only = 1``, as the host loop launches them;
3. an interaction token: cell list built from the device columns of the rows of the mask, then one lane per row (csrc/pk_interact.hip);
4. epilogue kernel (pk_interact_epilogue): position update, ``t += dt``, dt reset, EndofLoop; it returns the histogram of the states
   and what the next prologue would count.

Per iteration a few counters come back; the ``sources`` flags of AttractTowards (one byte per row, a host-only Variable) go up once
per launch.  A row in state Delete simply stops being evaluated; compaction and raising error codes happen after the loop by the route
every device launch takes (Kernel.needs_host_pass / only_deletions).

Rows that do not take part in an iteration are given a NaN x in the cell list, so they have no neighbours and are nobody's neighbour,
and indices stay row numbers.  The view a Python kernel receives numbers the evaluated rows 0, 1, ... in row order; row numbers order
them the same way, so row order, nearest-neighbour ties, the order of the sums and "the lower index keeps" are those of the view.
"""

from __future__ import annotations

import ctypes as C
import time as _time

import numpy as np

from . import kernels as _k
from .statuscodes import StatusCode

__all__ = ["interaction_route", "launch_device"]

_CROCO_IDS = (11, 12)  # PK_KERNEL_ADVECTION_RK2_3D_CROCO, PK_KERNEL_SAMPLE_SIGMA_CROCO
TIMINGS = None  # a dict here collects host-clock seconds per phase of every launch_device call (tools/bench_interaction_kernels.py)


def interaction_route(kernels, *, rk45_mode: bool, on_uxgrid: bool, multi_process: bool):
    """Where a kernel list runs: None without an interaction token (today's routes); "device" when every other kernel is a built-in
    that body_only launches accept, the fieldset is not in RK45 mode, there is no UxGrid, no CROCO kernel and one process; "host"
    otherwise -- the tokens' Python bodies then run in the host loop like any user kernel.  Nothing is refused."""
    if not any(_k.interaction_spec(f) is not None for f in kernels):
        return None
    for f in kernels:
        if _k.interaction_spec(f) is not None:
            continue
        kid = _k.kernel_id(f)
        if kid is None or kid in _CROCO_IDS:
            return "host"
    if rk45_mode or on_uxgrid or multi_process:
        return "host"
    return "device"


def _segments(kernel):
    """The kernel list as runs of built-in kernels and single interaction tokens."""
    segments = []
    for slot, f in enumerate(kernel._kernels):
        if slot in kernel.interactions:
            segments.append(("ia", kernel.interactions[slot], f.__name__))
        elif segments and segments[-1][0] == "dev":
            segments[-1][1].append(_k.kernel_id(f))
            segments[-1][2].append(slot)
        else:
            segments.append(("dev", [_k.kernel_id(f)], [slot]))
    return segments


def _pair_cap(ctx, spec):
    """max_pairs of pa.neighbors: the argument, or what fits into MAX_PAIRS_MEMORY_SHARE of the free device memory."""
    from . import interaction as _i

    if spec["max_pairs"] is not None:
        return int(spec["max_pairs"]), "max_pairs"
    free = ctx.device_info()["free_mem"]
    per = _i.device_bytes_per_pair(spec["z"])
    return int(_i.MAX_PAIRS_MEMORY_SHARE * free) // per, (
        f"the default: {_i.MAX_PAIRS_MEMORY_SHARE:.0%} of the {free} free bytes of device memory at {per} bytes per pair")


def launch_device(kernel, pset, endtime, dt, have_guess0=0, timings=None):
    """Kernel.launch for a list interaction_route sends to the device: advance the BOUND, device-resident columns to ``endtime``.
    Returns the statistics dict of a hosted launch with ``"hosted": False``.  ``timings`` (a dict): host-clock seconds per phase are
    added to it (prologue, body, build, pairs, reduce, merge, epilogue)."""
    from . import _hip, interaction as _i
    from .columns import readonly

    engine = pset._engine()
    ctx, lib, h = engine.ctx, engine.lib, engine.ctx.handle
    engine.set_user_program(None)
    fs = kernel.fieldset
    data = readonly(pset._data)
    if "RK45_tol" in fs.context:  # (set after the Kernel was made: the route was decided without it)
        raise RuntimeError("interaction kernels on the device do not run in RK45 mode (fieldset.context has RK45_tol): build the Kernel again")
    timings = TIMINGS if timings is None else timings
    clock = _time.perf_counter

    def note(key, t0):
        if timings is not None:
            timings[key] = timings.get(key, 0.0) + (clock() - t0)

    # body_only launches and the mask work on host-ordered rows: undo the cell sort an earlier execute left (device gather)
    ctx.check(lib.pk_interact_host_order(h), "pk_interact_host_order")
    engine._sorted_t = None
    segments = _segments(kernel)
    mass_index = {name: k for k, name in enumerate(kernel.device_variables)}
    uploaded = None  # the Variable whose flags the device holds (one name per list: one upload per launch)
    n_ev, n_act, steps_c, total_c = C.c_int64(), C.c_int64(), C.c_int64(), C.c_int64()
    counts_c = (C.c_int64 * _hip.PK_NUM_STATE_CODES)()
    phase3, phase2 = (C.c_double * 3)(), (C.c_double * 2)()
    steps = body_launches = 0
    first_body = True
    t0 = clock()
    ctx.check(lib.pk_interact_prologue(h, float(endtime), float(dt), 1, 0, C.byref(n_ev), C.byref(n_act)), "pk_interact_prologue")  # kernel.py:188
    note("prologue", t0)
    counts = None
    while n_act.value > 0 and n_ev.value > 0:  # :190, :196-197
        t0 = clock()
        ctx.check(lib.pk_interact_prologue(h, float(endtime), float(dt), 0, 1, C.byref(n_ev), C.byref(n_act)), "pk_interact_prologue")
        note("prologue", t0)
        for seg in segments:  # :206-216
            if seg[0] == "dev":
                t0 = clock()
                samples = {k: kernel.samples[s] for k, s in enumerate(seg[2]) if s in kernel.samples}
                prm = engine.make_params(seg[1], endtime=endtime, dt0=dt, context=fs.context, seed=pset.seed, reset_state=int(first_body),
                                         have_guess0=(have_guess0 if first_body else 1), sort_by_cell=0, samples=samples)
                prm.body_only = 1
                st = _hip.ExecStats()
                ctx.check(lib.pk_execute(h, C.byref(prm), C.byref(st)), "pk_execute (body)")
                first_body = False
                body_launches += 1
                note("body", t0)
                continue
            spec, name = seg[1], seg[2]
            sphere = float(spec["sphere"] or 0.0)
            if spec["kind"] == "attract":
                if uploaded != spec["sources"]:
                    flags = np.ascontiguousarray(np.asarray(data[spec["sources"]]) != 0).view(np.uint8)
                    ctx.check(lib.pk_interact_sources(h, flags.ctypes.data_as(C.c_void_p)), "pk_interact_sources")
                    uploaded = spec["sources"]
                cap, why = _pair_cap(ctx, spec)
                cap = min(cap, 2**63 - 1)
                ctx.check(lib.pk_interact_attract(h, spec["radius"], spec["velocity"], sphere, int(spec["z"]), 1, cap, C.byref(total_c), phase3),
                          "pk_interact_attract")
                total = int(total_c.value)
                if total > cap:
                    raise ValueError(f"max_pairs: {total} neighbour pairs exceed the cap of {cap} ({why}); use a smaller radius, neighbor_counts / "
                                     f"nearest_neighbor, or raise max_pairs ({name})")
                if total > _i._MAX_PAIRS_HARD:
                    raise ValueError(f"max_pairs: {total} neighbour pairs exceed the {_i._MAX_PAIRS_HARD} one call can list ({name})")
                if timings is not None:
                    for key, ms in zip(("build", "pairs", "reduce"), phase3):
                        timings[key] = timings.get(key, 0.0) + ms * 1e-3
            else:
                ctx.check(lib.pk_interact_merge(h, spec["radius"], sphere, int(spec["z"]), mass_index[spec["mass"]], phase2), "pk_interact_merge")
                if timings is not None:
                    for key, ms in zip(("build", "merge"), phase2):
                        timings[key] = timings.get(key, 0.0) + ms * 1e-3
        t0 = clock()
        ctx.check(lib.pk_interact_epilogue(h, float(endtime), float(dt), C.byref(steps_c), counts_c, C.byref(n_ev), C.byref(n_act)),
                  "pk_interact_epilogue")  # :219-230
        note("epilogue", t0)
        steps += int(steps_c.value)
        counts = {code: int(counts_c[code]) for code in range(_hip.PK_NUM_STATE_CODES) if counts_c[code]}
        if StatusCode.StopAllExecution in counts or any(code >= StatusCode.Error for code in counts):  # :236-245
            break
    if counts is None:  # no iteration: the states as they are (one 4-byte column; outside the loop)
        engine.d2h(["state"])
        codes, nums = np.unique(np.asarray(data["state"]), return_counts=True)
        counts = {int(c): int(m) for c, m in zip(codes, nums)}
    return {"steps": steps, "attempts": 0, "kernel_ms": 0.0, "sort_ms": 0.0, "launches": body_launches, "program": -1, "hosted": False,
            "first_error_iter": 0, "reran": 0, "state_counts": counts}
