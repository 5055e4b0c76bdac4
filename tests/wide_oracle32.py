"""Case module: the float32 oracle's run of a wide case and the pinned baseline geometries' table."""
import numpy as np

from oracle import np_oracle as O
from tests import ref64 as R64
from tests import ref64_cases as G
from tests import wide_cases as GW


F32 = np.float32


# ------------------------------------------------------------------------------------------------ calibration
def wide_oracle_case(case, k, cells, edit=None, batch_sum_term=False):
    """The float32 oracle and ref64 on the inputs test_gpu_wide_ref64 gives the engine for candidate k: worst ratio per quantity
    (test_ref64_cpu.py::oracle_case for a batch that may be larger than the 83-row dev table; edit and batch_sum_term as there)."""
    bc, dtype = GW.base_case(case, cells), case[9]
    hp = G.case_hyper(bc)
    seed = GW.SEED0 + GW.WIDE_IDS.index(case[0])
    conf, p0 = G.case_params(bc, hp, seed + 10 * k)
    t = G.case_table(bc, hp, G.N_EVAL, seed, dtype)
    tb = t if hp.B <= G.N_EVAL else G.case_table(bc, hp, hp.B, seed + 5, dtype)
    if edit is not None:
        p_in = p0
        p0, t = edit(conf, hp, p_in, t, dtype)
        tb = t if hp.B <= G.N_EVAL else edit(conf, hp, p_in, tb, dtype)[1]
    out = {}
    f = G.feats_of(t)
    lg, Ml, _ = R64.forward(p0, conf, hp, f, False)
    out["forward"] = R64.worst_ratio(O.forward({kk: v.copy() for kk, v in p0.items()}, conf, hp, f, False)[0], lg, Ml)[0]
    for nb in (hp.B, hp.B - 3):
        f = G.feats_of(tb, 0, nb)
        p32 = {kk: v.copy() for kk, v in p0.items()}
        lg32, cache32 = O.forward(p32, conf, hp, f, True, seed=seed + 3 * k, step=3)
        lg, Ml, cache = R64.forward(p0, conf, hp, f, True, seed=seed + 3 * k, step=3, batch_sum_term=batch_sum_term)
        out["forward_train"] = max(out.get("forward_train", 0.0), R64.worst_ratio(lg32, lg, Ml)[0])
        rng = np.random.default_rng(seed + k)
        dl = (rng.standard_normal((nb, hp.C)) / nb).astype(F32)
        dl[rng.random((nb, hp.C)) < 0.1] *= F32(1e-3)
        g32 = O.backward(p32, hp, cache32, dl)
        G64, MG = R64.backward(p0, hp, cache, dl)
        out["backward"] = max([out.get("backward", 0.0)] + [R64.worst_ratio(g32[kk], G64[kk], MG[kk])[0] for kk in g32])
        if hp.bn:
            O.bn_update_running(p32, hp, cache32)
            rs, Mrs = R64.running_stats(p0, hp, cache)
            out["running_stats"] = max([out.get("running_stats", 0.0)] + [R64.worst_ratio(p32[kk], rs[kk], Mrs[kk])[0] for kk in rs])
    return out


# (persistent, resident units, resident workgroups, units per workgroup, chunk columns, lean chain) of mfas_population_plan on a
# device-less host (256 compute units assumed), recorded from a build of the parent commit; the new library gave the same.
PINNED_CASES = {
    "r1a": (1, 4, 4, 1, 256, 1), "r1b": (1, 2, 2, 1, 256, 1), "r16a": (0, 0, 0, 1, 64, 0), "r16b": (1, 14, 14, 1, 256, 1),
    "r17a": (0, 0, 0, 1, 64, 0), "r17b": (0, 0, 0, 1, 64, 0), "r32a": (0, 0, 0, 1, 64, 0), "r32b": (0, 0, 0, 1, 64, 0),
    "r33a": (0, 0, 0, 1, 64, 0), "r33b": (0, 0, 0, 1, 64, 0), "r65a": (0, 0, 0, 1, 64, 0), "r65b": (0, 0, 0, 1, 64, 0),
    "r80a": (0, 0, 0, 1, 64, 0), "r80b": (0, 0, 0, 1, 64, 0), "r128a": (0, 0, 0, 1, 64, 0), "r128b": (0, 0, 0, 1, 64, 0),
    "r129a": (0, 0, 0, 1, 64, 0), "r129b": (0, 0, 0, 1, 64, 0), "r256a": (0, 0, 0, 1, 64, 0), "r256b": (0, 0, 0, 1, 64, 0),
    "r257a": (0, 0, 0, 1, 64, 0), "r257b": (0, 0, 0, 1, 64, 0), "r300": (0, 0, 0, 1, 64, 0), "r320a": (0, 0, 0, 1, 64, 0),
    "r320b": (0, 0, 0, 1, 64, 0), "r448a": (0, 0, 0, 1, 64, 0), "r448b": (0, 0, 0, 1, 64, 0), "r449a": (0, 0, 0, 1, 64, 0),
    "r449b": (0, 0, 0, 1, 64, 0), "r512a": (0, 0, 0, 1, 64, 0), "r512b": (0, 0, 0, 1, 64, 0),
}
PINNED_BASELINE = {
    "r16_b20_k1": (1, 30, 30, 1, 256, 1), "r128_b16_k1": (0, 0, 0, 1, 64, 0), "mmimdb_k1": (0, 0, 0, 1, 64, 0),
    "r16_b20_k16": (1, 480, 240, 2, 256, 1), "r128_b16_k16": (0, 0, 0, 1, 128, 0), "mmimdb_k16": (0, 0, 0, 1, 64, 0),
    "r16_b20_k64": (0, 0, 0, 1, 128, 1), "r128_b16_k64": (0, 0, 0, 1, 64, 0), "mmimdb_k64": (0, 0, 0, 1, 64, 0),
}
