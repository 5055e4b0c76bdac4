"""Device plumbing of the report tests: populations from a case's inputs.  Re-exports tests/report_cases.py."""
import os

from tests.report_cases import *  # noqa: F401,F403  (one alias serves a consumer for the cases and the plumbing)


# ------------------------------------------------------------------------------------------------ GPU plumbing
def make_population(ehp, confs, dev, seeds, env=None, chunk_cols=0, pos_weight=None):
    from mfas_amd import Population
    env = env or {}
    os.environ.update(env)
    try:
        pop = Population(ehp, confs, dev, drop_seeds=seeds, chunk_cols=chunk_cols)
    finally:
        for k in env:
            os.environ.pop(k, None)
    if pos_weight is not None:
        pop.set_pos_weight(pos_weight)
    return pop


def plane_bytes(pop, k, plane=0):
    return pop.get_params(k, plane).cpu().numpy().tobytes()
