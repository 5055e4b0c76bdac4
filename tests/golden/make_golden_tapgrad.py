#!/usr/bin/env python3
"""Golden tap gradients from the UNCHANGED reference, through the stubs of make_golden.py (build container only, like that script):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_tapgrad.py

The reference's Searchable_Skeleton_Image_Net runs in train mode on the first 8 rows of synth_table(16, 11) with the taps served as
LEAVES THAT REQUIRE GRAD (FeatVisual / FeatSkel hand them through unchanged), BatchNorm without dropout (no Philox stream is involved),
hash-generated parameters; loss = CrossEntropyLoss(logits, label); loss.backward().  One configuration without alphas and one with.
Stored: the expected gradient of every tap the configuration selects (data only), in g24_tap_gradients.npz.
tests/test_tapgrad_cpu.py holds the ref64-derived values to it."""
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import numpy as np
import torch

import make_golden as MG

CONF = [[0, 0, 0], [1, 0, 1], [0, 0, 2]]        # s0 selected by two cells, v0 by three
ROWS = 8
VARIANTS = [("bn", dict(batchnorm=True, drpt=0.0), 2400), ("alpha_bn", dict(batchnorm=True, drpt=0.0, alphas=True), 2401)]


def main():
    out = {}
    t = MG.table(16, 11)
    for vname, kw, seed in VARIANTS:
        args = MG.mkargs(**kw)
        model = MG.ntu.Searchable_Skeleton_Image_Net(args, np.array(CONF))
        MG.load_det(model, CONF, args, seed, perturb_bn=True)
        model.train(True)
        rgb, ske = MG.feats_of(t, slice(0, ROWS))
        used = sorted({f"s{c[0]}" for c in CONF}) + sorted({f"v{c[1]}" for c in CONF})
        for name in used:
            (ske if name[0] == "s" else rgb)[name].requires_grad_(True)
        label = torch.from_numpy(t["label"][:ROWS])
        loss = torch.nn.CrossEntropyLoss()(model((rgb, ske)), label)
        loss.backward()
        out[f"{vname}/loss"] = np.array(loss.item())
        for name in used:
            out[f"{vname}/grad/{name}"] = (ske if name[0] == "s" else rgb)[name].grad.numpy().copy()
    out["conf"] = np.array(CONF)
    out["names"] = np.array([f"{v}/{s}" for v, _, s in VARIANTS])
    MG.save("g24_tap_gradients.npz", **out)


if __name__ == "__main__":
    main()
