"""Device plumbing of the evaluate tests: the cache of built worlds (one per case and process, shared by both evaluate test modules) and
the calls on it."""
import numpy as np

from tests import evaluate_cases as EC
from tests import gpu_support as G
from tests.report_gpu import make_population


COMBINE = ("prob", "score")


# ------------------------------------------------------------------------------------------------ plumbing
_WORLDS = {}


def world(cid, dev):
    """One population per case with its parameters loaded, the table on the device, and the engine's OWN float32 logits and counts
    of every candidate from forward() — computed once, shared by the tests, never changed."""
    if cid not in _WORLDS:
        from tests.helpers import engine_hyper
        case = EC.EVAL_CASES[EC.EVAL_IDS.index(cid)]
        inp = EC.eval_inputs(case)
        hp = inp["hp"]
        pop = make_population(engine_hyper(hp), inp["confs"], dev, inp["seeds"], pos_weight=G.pos_weight(hp) if hp.loss_mode else None)
        for k, p in enumerate(inp["p0s"]):
            pop.set_state_dict(k, p)
        tab = G.gpu_table(inp["tab"], inp["dtype"], dev)
        fwd = [pop.forward(k, tab, count=True) for k in range(pop.K)]
        inp.update(pop=pop, gtab=tab, Z=np.stack([f[0].cpu().numpy() for f in fwd]), counts=[f[1] for f in fwd], case=case)
        _WORLDS[cid] = inp
    return _WORLDS[cid]


def add_world(cid, build):
    """A world of the caller's own inputs enters the cache as `cid`: build() -> what world() keeps, called only if `cid` is not there yet."""
    if cid not in _WORLDS:
        _WORLDS[cid] = build()


def close_worlds():
    """Every cached population closed and the cache emptied: the teardown of the modules that use world()."""
    for w in _WORLDS.values():
        w["pop"].close()
    _WORLDS.clear()


def evaluate(w, members, weights, combine, **kw):
    lm0 = w["hp"].loss_mode == 0
    return w["pop"].evaluate(w["gtab"], members=members, weights=weights, combine=COMBINE[combine], return_scores=True,
                             return_preds=lm0, **kw)


def outputs(res):
    """Everything k_vote wrote, as bytes / integers (for bit-identity)."""
    return (res["scores"].cpu().numpy().tobytes(), res["preds"].cpu().numpy().tobytes() if "preds" in res else b"",
            np.float64(res["ensemble"]["loss_sum"]).tobytes(), res["ensemble"]["corrects"], res["member_stats"]["dev_corrects"].tolist())
