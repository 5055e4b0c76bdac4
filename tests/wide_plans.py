"""Engine plumbing (host side, no GPU): the plans of the wide cases and the baseline geometries.  Re-exports tests/wide_oracle32.py."""
import numpy as np

from tests.wide_oracle32 import *  # noqa: F401,F403  (one alias serves a consumer for the cases and the plumbing)
from oracle import np_oracle as O
from tests.helpers import CONFS, engine_hyper


# ------------------------------------------------------------------------------------------------ the layout query
def plan(hp, confs, chunk_cols=0):
    from mfas_amd.engine import plan_population
    d = plan_population(engine_hyper(hp) if isinstance(hp, O.Hyper) else hp, [np.array(c) for c in confs], "cuda:0", chunk_cols)
    return (int(d["persistent"]), d["resident_units"], d["resident_workgroups"], d["units_per_workgroup"], d["chunk_cols"],
            int(d["lean_chain"]), int(d["wide"]))


def baseline_geometries():
    """(name, hyper, configurations): the search default (R = 16, B = 20), the headline (R = 128, B = 16), the MM-IMDB one."""
    from mfas_amd import Hyper
    from mfas_amd.mmimdb_searchable import MM_IMAGE_SIZES, MM_TEXT_SIZES
    c4 = [CONFS["c4"]]
    out = []
    for K in (1, 16, 64):
        out.append((f"r16_b20_k{K}", O.Hyper(R=16, C=60, B=20, bn=False, drpt=0.5), c4 * K))
        out.append((f"r128_b16_k{K}", O.Hyper(R=128, C=60, B=16, bn=False, drpt=0.5), c4 * K))
        out.append((f"mmimdb_k{K}", Hyper(R=128, C=23, B=32, bn=True, drpt=0.5, loss_mode=1, s_sizes=MM_TEXT_SIZES, v_sizes=MM_IMAGE_SIZES),
                    [CONFS["l2"]] * K))
    return out
