"""Case module: the sweep-launch forms, natural cases and the launch / row / natural input builders of the step-build tests."""
from tests import ref64_cases as G
from tests import resident_cases as GR
from tests import train_cases as GT
from tests import wide_cases as GW
from tests.ref64_cases import W_A, W_C


FULL = GR.FULL                      # the six-batch train table of resident_cases.py


STEPS = GR.STEPS                    # (1, 2, 3, 5, 6, 7)
SEED0 = 11000
NATURAL_SEED0 = 11500


def named(form, nt):
    return form.replace("N", str(int(nt)))


def plan_states():
    """Every (wide, MB, lean, same_group, chain_split, groups) plan_layout can produce."""
    out = [dict(wide=True, MB=MB, lean=False, same_group=False, chain_split=0, groups=1) for MB in (1, 2, 4)]
    for MB in (1, 2, 4):
        for lean in (False, True):
            for same_group in (False, True):
                for chain_split in (0, 4):
                    for groups in (1, 2):
                        if lean and (MB > 2 or same_group or chain_split):
                            continue
                        if same_group and (MB > 2 or groups == 2):
                            continue
                        if chain_split and (MB != 1 or not (same_group or groups == 2)):
                            continue
                        out.append(dict(wide=False, MB=MB, lean=lean, same_group=same_group, chain_split=chain_split, groups=groups))
    return out


def launch_inputs(st):
    """What the launches of one launch-per-phase epoch hand the choice (launches.hip.h: epoch_launches; train.hip.h: launch_record):
    (has a sweep, has a chain, same-group launch).  The prologue, and a two-group epoch's last launch, are sweeps without a chain; a
    launch without a sweep is the standalone chain."""
    if st["same_group"]:
        return [(1, 0, 0), (1, 1, 1)]
    if st["groups"] == 1:
        return [(1, 0, 0), (0, 1, 0)]
    return [(1, 0, 0), (0, 1, 0), (1, 1, 0)]


# ------------------------------------------------------------------------------------------------ the rows
# candidates: different depths and nonlinearities.  BatchNorm populations keep to two cells (a deeper BatchNorm stack leaves most
# rows of a train batch ambiguous in ref64 itself); the others go to four.
POP_BN = [[[3, 3, 0], [1, 2, 1]], [[0, 3, 2]], [[2, 1, 0], [3, 0, 1]]]
POP_DEEP = [[[3, 3, 0], [1, 2, 1], [0, 0, 2]], [[0, 3, 2]], [[2, 1, 0], [3, 0, 1], [1, 1, 0], [2, 2, 2]]]
WB65 = GW.WIDE_CASES[GW.WIDE_IDS.index("wb65")]          # B = 65: the smallest batch that is wide
POP_WIDE = [GW.POOL[2], GW.POOL[1], [[2, 0, 0], [0, 2, 1]]]


def _row(rid, target, family, R, C, B, widths, confs, flags, env, cc, facts, forms):
    return dict(id=rid, target=target, family=family, R=R, C=C, B=B, widths=widths, confs=confs, flags=flags, env=env, cc=cc,
                facts=facts, forms=set(forms))


def _facts(MB, lean=False, same_group=False, chain_split=0, groups=1, wide=False, over_occ=False):
    return dict(wide=wide, MB=MB, lean=lean, same_group=same_group, chain_split=chain_split, groups=groups, over_occ=over_occ)


# One row per reachable form.  R, C, B and the widths are the smallest at which the form exists (R = 33 / 17 / 11: no multiple of 16;
# R = 113: the first width with eight row blocks, which chain_split needs; B = 7 / 17 / 33 / 65: the first of each batch-tile count with
# a ragged last tile); the same-group rows keep the shapes of ref64_cases.SCHEDULES.  forms: the record the row must leave, chain
# builds included (the prologue, and the last launch of a two-group epoch, are sweeps without a chain: the plain k_step of the MB).
SWEEP_FORMS = [
    _row("step-mb1", "k_step<1,N,4,0,1>", "k_step", 33, 17, 7, W_A, POP_BN, "bn", {"MFAS_GROUPS": "2"}, 0,
         _facts(1, groups=2), ["k_step<1,N,4,0,1>", "k_chain<1,0>"]),
    _row("step-split", "k_step<1,N,4,0,4>", "k_step", 113, 17, 16, W_A, POP_DEEP, "", {"MFAS_GROUPS": "2", "MFAS_SAME_GROUP": "0"}, 0,
         _facts(1, chain_split=4, groups=2), ["k_step<1,N,4,0,4>", "k_step<1,N,4,0,1>", "k_chain<1,0>"]),
    _row("step-mb2-w2", "k_step<2,N,2,0,1>", "k_step", 17, 60, 17, W_A, POP_BN, "bn", {"MFAS_GROUPS": "2"}, 0,
         _facts(2, groups=2), ["k_step<2,N,2,0,1>", "k_step<2,N,4,0,1>", "k_chain<2,0>"]),
    # the same population: every launch with a chain in it now takes the WPE = 4 build, so the WPE = 2 one must be absent
    _row("step-mb2-w4-chain", "k_step<2,N,4,0,1>", "k_step", 17, 60, 17, W_A, POP_BN, "bn", {"MFAS_GROUPS": "2", "MFAS_OCC_BYTES": "0"}, 0,
         _facts(2, groups=2, over_occ=True), ["k_step<2,N,4,0,1>", "k_chain<2,0>"]),
    _row("step-mb4", "k_step<4,N,2,0,1>", "k_step", 17, 17, 33, W_A, POP_DEEP, "", {}, 0,
         _facts(4), ["k_step<4,N,2,0,1>", "k_chain<4,0>"]),
    _row("lean-mb1", "k_step<1,N,4,1,1>", "k_step", 16, 60, 7, W_A, POP_BN, "bn", {"MFAS_PERSIST": "0"}, 0,
         _facts(1, lean=True), ["k_step<1,N,4,1,1>", "k_chain<1,1>"]),
    # two groups: chain_lean runs inside the k_step build (the 128-register one), not only next to it
    _row("lean-mb2", "k_step<2,N,4,1,1>", "k_step", 11, 17, 20, W_A, POP_DEEP, "", {"MFAS_PERSIST": "0", "MFAS_GROUPS": "2"}, 0,
         _facts(2, lean=True, groups=2), ["k_step<2,N,4,1,1>", "k_chain<2,1>"]),
    _row("same-mb1", "k_step_same<1,N,1>", "k_step_same", 128, 60, 16, W_A, POP_BN, "bn", {"MFAS_SAME_GROUP": "2", "MFAS_CHAIN_SPLIT": "0"}, 128,
         _facts(1, same_group=True), ["k_step_same<1,N,1>", "k_step<1,N,4,0,1>"]),
    _row("same-mb2", "k_step_same<2,N,1>", "k_step_same", 65, 17, 20, W_A, POP_DEEP, "", {"MFAS_SAME_GROUP": "2"}, 0,
         _facts(2, same_group=True), ["k_step_same<2,N,1>", "k_step<2,N,4,0,1>"]),
    _row("same-split", "k_step_same<1,N,4>", "k_step_same", 128, 60, 16, W_A, POP_BN, "bn", {"MFAS_SAME_GROUP": "2"}, 128,
         _facts(1, same_group=True, chain_split=4), ["k_step_same<1,N,4>", "k_step<1,N,4,0,1>"]),
    _row("wide", "k_sweep_wide<N>", "k_sweep_wide", WB65[1], WB65[2], WB65[3], WB65[4], POP_WIDE, "bn", {}, 0,
         _facts(4, wide=True), ["k_sweep_wide<N>", "k_chain_wide"]),
]
FORM_IDS = [r["id"] for r in SWEEP_FORMS]
# the rows that also train one epoch with the 83-row dev table under MFAS_NT=1: one per kernel family
DEV_ROWS = ("step-mb2-w2", "same-split", "wide")


# Per-row taus where the float32 oracle itself exceeds a quarter of the project's tau on the row's inputs: four times the oracle's
# measured maximum, rounded up.  {id: {quantity: (tau, measured)}}.  None was needed.
CASE_TAUS = {}
# Row i draws from SEED0 + i + 100 * draw.  Draw 0 unless the float32 oracle and ref64 ALONE refuse it (no engine result was looked
# at): the draws listed here are the first on which test_rows_calibration_margin holds, with what the earlier ones failed.
#   step-mb1 (BatchNorm, ragged batch of 3 rows): draws 0 and 1 leave 1 of the 3 rows ambiguous in ref64 (candidate 0)
#   same-mb1 (BatchNorm at R = 128, C = 60):      draw 0 leaves 7 of 16 rows ambiguous, draw 1 3 of the ragged 8 (candidate 0)
ROW_DRAW = {"step-mb1": 2, "same-mb1": 2}


def case_taus(rid):
    taus = dict(GT.TAUS)
    taus.update({q: float(tau) for q, (tau, _) in CASE_TAUS.get(rid, {}).items()})
    return taus


def row_dtype(rid):
    return G.DTYPES[FORM_IDS.index(rid) % 3]


def row_order_mode(rid):
    return ("shared", "per_candidate")[FORM_IDS.index(rid) % 2]


def _inputs(row, seed, dtype, order_mode, full, extra=""):
    """What a row trains, as numpy (no device)."""
    from tests.helpers import engine_hyper
    fl = set(filter(None, row["flags"].split(",")))
    case = lambda cells: (row["id"], row["R"], row["C"], row["B"], row["widths"], cells, "bn" in fl, 0.5, extra)  # noqa: E731
    hp = G.case_hyper(case(row["confs"][0]))
    confs, p0s = [], []
    for k, cells in enumerate(row["confs"]):
        conf, p0 = G.case_params(case(cells), hp, seed + 10 * k)
        confs.append(conf)
        p0s.append(p0)
    K = len(confs)
    ehp = engine_hyper(hp)
    ehp.order_per_candidate = order_mode == "per_candidate"
    N = GT.train_rows(row["B"], full)
    t = G.case_table(case(None), hp, N, seed, dtype)
    order = GT.make_order(N, seed, K if ehp.order_per_candidate else None)
    return dict(hp=hp, ehp=ehp, confs=confs, seeds=[seed + 3 * k for k in range(K)], p0s=p0s, N=N, t=t, dtype=dtype, order=order,
                etas=GT.step_etas(N, row["B"]), seed=seed, case=case(None))


def row_inputs(row, draw=None):
    rid = row["id"]
    draw = ROW_DRAW.get(rid, 0) if draw is None else draw
    return _inputs(row, SEED0 + FORM_IDS.index(rid) + 100 * draw, row_dtype(rid), row_order_mode(rid), FULL)


# ------------------------------------------------------------------------------------------------ the natural populations
def plane_floats(R, C, widths, confs):
    """plan.hip.h: plane_stride, the floats of ONE of the three planes W / m / v — per candidate the vector block, per cell the padded
    S, V (and from the second cell on OUT) segments, the head, rounded up to 64."""
    Rp, Cp = GW.ceil16(R), GW.ceil16(C)
    vec = (4 * (5 * Rp + 16) + Cp + 63) // 64 * 64
    tot = 0
    for conf in confs:
        n = vec + Cp * Rp
        for i, c in enumerate(conf):
            n += Rp * (GW.ceil16(widths["s"][c[0]]) + GW.ceil16(widths["v"][c[1]]) + (Rp if i else 0))
        tot += (n + 63) // 64 * 64
    return tot


NT_BYTES = 200.0 * 1024 * 1024      # plan_layout: pl.nontemporal = plane_stride * 12 > 200 MiB


BIG = [3, 0]                        # W_C's two widest taps: s2048 + v4100 columns per cell


def _big(*nls):
    return [BIG + [nl] for nl in nls]


# natural_nt: R = 128 (the headline's width), B = 16, six candidates of 4, 3, 4, 4, 3 and 4 cells: 17,673,984 floats per plane,
#   212.1 MB of W / m / v against the 209.7 MB (200 MiB) threshold -> nontemporal; one group (fewer than 8 candidates; 423 MB of state
#   is beyond the same-group launch's 260 MB), so the sweep is k_step<1,1,4,0,1>, the headline build, reached by size alone.
#   Its sibling has one cell fewer (the last candidate: 3 cells): 16,869,120 floats, 202.4 MB -> cached.
# natural_occ: R = 80 (five row blocks: occ_bytes = 250 MB; with B in 17..32 the k-split slabs of six or seven row blocks leave the
#   LDS too little room), B = 17, twelve candidates (two groups with no switch from eight on) of 4, 4, 4, 3, 3, 3 | 4, 4, 4, 3, 3, 3 cells:
#   each group 10,432,800 weights = 250.4 MB of state against 250 MB -> the WPE = 4 build also with a chain in the launch; 20,941,056
#   floats per plane, 251.3 MB of planes -> nontemporal: k_step<2,1,4,0,1>, and no k_step<2,1,2,0,1>.
_OCC_GROUP = [(0, 1, 2, 0), (1, 2, 0, 1), (2, 0, 1, 2), (0, 2, 1), (1, 0, 2), (2, 1, 0)]
NATURAL = {
    "natural_nt": dict(_row("natural_nt", "k_step<1,N,4,0,1>", "k_step", 128, 60, 16, W_C,
                            [_big(0, 1, 2, 0), _big(1, 2, 0), _big(2, 0, 1, 2), _big(0, 0, 1, 1), _big(2, 1, 0), _big(1, 2, 2, 0)], "", {}, 0,
                            _facts(1), ["k_step<1,N,4,0,1>", "k_chain<1,0>"]), nt=1, dtype="bfloat16", order_mode="per_candidate"),
    "natural_occ": dict(_row("natural_occ", "k_step<2,N,4,0,1>", "k_step", 80, 17, 17, W_C,
                             [_big(*n) for n in _OCC_GROUP] + [_big(*n[::-1]) for n in _OCC_GROUP], "", {}, 0,
                             _facts(2, groups=2, over_occ=True), ["k_step<2,N,4,0,1>", "k_chain<2,0>"]), nt=1, dtype="float16", order_mode="shared"),
}
NATURAL_IDS = list(NATURAL)
NATURAL_STEPS = (1, 2, 3)


def natural_sibling(row):
    """natural_nt with one cell fewer: the last candidate loses its last cell."""
    return dict(row, confs=row["confs"][:-1] + [row["confs"][-1][:-1]])


def natural_inputs(name, row=None):
    row = row or NATURAL[name]
    return _inputs(row, NATURAL_SEED0 + NATURAL_IDS.index(name), row["dtype"], row["order_mode"], 1)
