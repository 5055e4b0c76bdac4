"""Engine plumbing of the resident tests: the schedule the plan gives a resident case.  Re-exports tests/resident_cases.py."""
from tests.resident_cases import *  # noqa: F401,F403  (one alias serves a consumer for the cases and the plumbing)
from tests import wide_cases as GW


def resident_schedule(hp, confs, chunk_cols, sched=None, device="cuda:0"):
    """pop.schedule() (or, without a population, the plan query's answer) with the chunk the plan cut the feature segments with and
    the widest unit that gives: a tap of padded width w is cut into units of the largest multiple of 16 that divides w and does
    not exceed the chunk (plan.hip.h: pick_chunk)."""
    from mfas_amd.engine import plan_population
    plan = plan_population(hp, confs, device, chunk_cols)
    out = dict(plan if sched is None else sched)
    out["chunk_cols"] = plan["chunk_cols"]
    used = {GW.ceil16(hp.s_sizes[c[0]]) for conf in confs for c in conf} | {GW.ceil16(hp.v_sizes[c[1]]) for conf in confs for c in conf}
    out["widest_unit"] = max(GW.pick_chunk(w, plan["chunk_cols"]) for w in used)
    out["compute_units"] = plan["compute_units"]
    return out
