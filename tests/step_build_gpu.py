"""Device plumbing of the step-build tests: populations under a build's switches, their trained states and the check against ref64."""
import os
from unittest import mock

from tests import gpu_support as G
from tests import step_build_cases as SB
from tests import train_gpu as GT


SWITCHES = ("MFAS_NT", "MFAS_OCC_BYTES", "MFAS_GROUPS", "MFAS_SAME_GROUP", "MFAS_CHAIN_SPLIT", "MFAS_PERSIST")


def make_pop(row, inp, dev, nt):
    """The row's population under the row's switches and MFAS_NT = nt (None: unset), its schedule asserted against the row's facts."""
    from mfas_amd import Population
    assert not any(s in os.environ for s in SWITCHES), "a schedule switch is set in the test's own environment"
    env = dict(row["env"])
    if nt is not None:
        env["MFAS_NT"] = str(nt)
    os.environ.update(env)
    try:
        pop = Population(inp["ehp"], inp["confs"], dev, drop_seeds=inp["seeds"], chunk_cols=row["cc"])
    finally:
        for key in env:
            os.environ.pop(key, None)
    try:
        s, f = pop.schedule(), row["facts"]
        want = dict(persistent=0, lean_chain=int(f["lean"]), wide=int(f["wide"]), groups=-1 if f["same_group"] else f["groups"],
                    chain_cus=max(1, f["chain_split"]))
        assert {q: s[q] for q in want} == want, (row["id"], s)
    except BaseException:
        pop.close()
        raise
    return pop


def expected_record(row, nt):
    return {SB.named(f, nt) for f in row["forms"]}


def assert_record(row, nt, j, rec):
    """The library's record of a j-step call: nothing for j = 0, else exactly the row's builds, each launched at least once."""
    if j == 0:
        assert rec == {}, (row["id"], nt, j, rec)
        return
    assert set(rec) == expected_record(row, nt), (row["id"], f"NT={nt}", f"{j}-step call", rec)
    assert all(n > 0 for n in rec.values()), (row["id"], nt, j, rec)


def train_states(dev, row, inp, nt, steps):
    """engine_states of the row's population under MFAS_NT = nt, the record of every call asserted; returns (S, ST, pop)."""
    torch = G._torch()
    pop = make_pop(row, inp, dev, nt)
    try:
        tab = G.gpu_table(inp["t"], inp["dtype"], dev)
        seen = 1 if nt is None else nt
        S, ST = GT.engine_states(pop, tab, inp["p0s"], inp["etas"], torch.from_numpy(inp["order"]).to(dev), steps,
                                 after_call=lambda j, p: assert_record(row, seen, j, p.launch_record()))
    except BaseException:
        pop.close()
        raise
    return S, ST, pop, tab


def check_ref64(row, inp, S, ST, steps, taus, tag, rec=None):
    per = inp["ehp"].order_per_candidate
    with mock.patch.dict(GT.TAUS, taus):        # (test_gpu_train_ref64's check reads its module's taus)
        for k, c in enumerate(inp["confs"]):
            GT.check_candidate(S, ST, k, c, inp["hp"], inp["p0s"][k], inp["t"], inp["order"][k] if per else inp["order"], inp["seeds"][k],
                               inp["etas"], f"{row['id']} {tag} cand {k}", rec or f"builds/{row['family']}", steps)
