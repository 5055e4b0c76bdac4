"""Degenerate and extreme input values for the ref64 tests, as plain numpy.

TEST INFRASTRUCTURE ONLY (nothing under ``mfas_amd/`` imports it).  Every other ref64 test draws its values from one
distribution (``O.synth_table(snr=0.4)`` taps of magnitude about 1, ``O.init_params(perturb_bn=True)`` parameters): logits below
1, no BatchNorm column without batch variance, no softmax far from uniform, no empty target row.  The two functions here change
a table (``edge_table``) or a state dict (``edge_params``) into what a trained network and a real pooled post-ReLU backbone
feature hold.  Both are pure: they return new dicts and leave their arguments alone.

how        what it does                                                        what it reaches
scaled     taps x 64                                                           logits of 30-40, large products in every sweep
tiny       taps x 2^-12                                                        small products next to O(1) biases (taps stay normal)
sparse     max(x, 0), 70 % of the elements +0, every 5th column all zero,      all-zero k-blocks and column chunks, signed zero
           every 7th column -0.0                                               through 16-bit staging
offset     taps + 100                                                          large mean, small relative variance into BatchNorm
dup        every row equals row 0                                              batch variance exactly 0 in every column: rstd = 1/sqrt(eps)
onelabel   every label is C - 1                                                the last valid class next to the padded ones
dead       per cell, fusion bias r = 0 mod 3 set to -DEAD_BIAS and              a ReLU column exactly 0 over the batch, a sigmoid
           r = 1 mod 3 to +DEAD_BIAS                                           column saturated at 0 / 1, a large LeakyReLU column
deadrelu   per cell, fusion bias r = 0 mod 3 set to -DEAD_BIAS, nothing else   the dead half of 'dead' alone: a ReLU column exactly 0 over the
                                                                               batch in the FIRST cell under BatchNorm (var 0, d_y gated off)
bigmean    per cell, fusion bias r = 1 mod 3 set to +DEAD_BIAS, nothing else   the other half alone: a ReLU / LeakyReLU column of n values near 64
                                                                               with a spread of about 1 (the float32 batch sum rounds at the
                                                                               scale of 64 n; ref64 judges it with batch_sum_term), a sigmoid at 1
bighead    classifier weight and bias x 200 (CE heads only)                    |logit| 100-160, a one-hot softmax, CE up to 300 a row
mlrows     multi-label targets: row 0 empty, row 1 full, rows 2..4 one         a row whose F1 denominator is 0; head bias -6, so
           positive (class 0, C - 1, `top`); head bias -6 on every class       nothing is predicted anywhere

DEAD_BIAS = 64: the float32 oracle keeps the x4 margin of tests/test_inputs_cpu.py::test_input_cases_calibration_margin on every
case that uses it (worst ratios at 64: forward 0.51, forward_train 0.74, backward 3.02, running statistics 0.77; train m 0.79,
v 0.17, w 3.66, runstat 0.81).  Sigmoid saturates in float32 from +17 on, and the largest pre-activation of these inputs is about
4, so the columns are dead well before 64.  What limits 'dead' is not the magnitude but where it is put: that file's docstring says
which cases cannot keep the margin at any magnitude, and why.
"""
import numpy as np

from oracle import np_oracle as O

F32 = np.float32
HOWS = ("scaled", "tiny", "sparse", "offset", "dup", "onelabel", "dead", "bighead", "mlrows", "deadrelu", "bigmean")
DEAD_BIAS = 64.0
BIGHEAD = 200.0
MLROWS_BIAS = -6.0


def is_tap(k):
    return k[0] in "sv" and k[1:].isdigit()


def _dequant(a, dtype):
    from tests.ref64_cases import dequant
    return dequant(a, dtype)


def sparse_pattern(x, salt):
    """max(x, 0); 70 % of the elements exact +0 (a hash of the position); every fifth column all zero; every seventh -0.0."""
    n, w = x.shape
    y = np.maximum(np.asarray(x, F32), F32(0)).copy()
    y[O.hash_u01(4242 + salt, n * w).reshape(n, w) < F32(0.7)] = F32(0)
    y[:, 0::5] = F32(0)
    y[:, 3::7] = F32(-0.0)
    return y


def edge_table(t, how, dtype, C=None, top=None):
    """Table t (taps as float32 values, label, optional vlogit / slogit / multilabel) changed `how`, its taps re-quantised to
    `dtype`.  C: the number of classes ('onelabel').  top: the class of row 4's single positive under 'mlrows' (the class with the
    largest logit: the caller, who has the parameters, knows it)."""
    assert how in HOWS, how
    out = {k: np.array(v, copy=True) for k, v in t.items()}
    for j, k in enumerate(sorted(k for k in out if is_tap(k))):
        x = out[k]
        if how == "scaled":
            x = x * F32(64)
        elif how == "tiny":
            x = x * F32(2.0 ** -12)
        elif how == "sparse":
            x = sparse_pattern(x, j)
        elif how == "offset":
            x = x + F32(100)
        elif how == "dup":
            x = np.repeat(x[:1], len(x), 0)
        out[k] = _dequant(x.astype(F32), dtype)
    if how == "onelabel":
        out["label"] = np.full_like(out["label"], int(C) - 1)
    if how == "mlrows":
        z = out["multilabel"]
        C = z.shape[1]
        assert len(z) >= 5 and top is not None
        z[0], z[1] = 0, 1
        for r, c in ((2, 0), (3, C - 1), (4, int(top))):
            z[r] = 0
            z[r, c] = 1
    return out


def edge_params(p, hp, conf, how):
    """State dict p changed `how` (a copy; the table-only transforms return it unchanged)."""
    assert how in HOWS, how
    q = {k: np.array(v, copy=True) for k, v in p.items()}
    if how in ("dead", "deadrelu", "bigmean"):
        for i in range(len(conf)):
            b = q[f"fusion_layers.{i}.0.bias"]
            if how != "bigmean":
                b[0::3] = F32(-DEAD_BIAS)
            if how != "deadrelu":
                b[1::3] = F32(DEAD_BIAS)
    elif how == "bighead":
        assert hp.loss_mode == 0, "bighead saturates a sigmoid head: that is the status tests' subject"
        q["central_classifier.weight"] = (q["central_classifier.weight"] * F32(BIGHEAD)).astype(F32)
        q["central_classifier.bias"] = (q["central_classifier.bias"] * F32(BIGHEAD)).astype(F32)
    elif how == "mlrows":
        assert hp.loss_mode == 1
        q["central_classifier.bias"][:] = F32(MLROWS_BIAS)
    return q


def dead_columns(conf, hp, cell=0):
    """Columns of `cell` that 'dead' leaves with batch variance exactly 0: a ReLU's r = 0 mod 3 (the activation is 0 on every
    row) and a sigmoid's r = 1 mod 3 (it rounds to 1 on every row, in float32 and in float64).  A LeakyReLU cell has none.
    'deadrelu' leaves a ReLU cell the same r = 0 mod 3 columns (and a sigmoid cell none: its r = 0 mod 3 columns are e^-64, not 0)."""
    nl = int(conf[cell][2])
    cols = np.arange(hp.R)
    return cols[cols % 3 == 0] if nl == 0 else (cols[cols % 3 == 1] if nl == 1 else cols[:0])
