"""k_pool (GlobalPooling2D, the kernel that builds the feature tables) against a float64 mean.

test_gpu_mirror.py::test_global_pooling_kernel compares with torch's own float32 mean on zero-mean randn at friendly shapes.
Here the bound comes from the kernel's summation order (pack.hip.h: a serial sum per lane of at most ceil(inner / 64) elements,
six shuffle adds, one division), every rounding at most 2^-24 of the sum of magnitudes:

    |got - mean64(x)| <= (ceil(inner / 64) + 8) * 2^-24 * mean(|x|)          (float32 output)

and for a bf16 / f16 output `got` lies between the round-to-nearest-even roundings of the two ends of that interval.  With
inner = 1 nothing rounds before the output conversion (0 + x and x / 1 are exact), so the output is exactly RNE(x): that pins the
ties of the bf16 rounding, with an even and with an odd lower neighbour.

Shapes: inner in {1, 3, 4, 7, 8, 9, 63, 64, 65, 255, 257, 1001, 8192} (an odd inner puts every second row off the 16-byte grid of
the vector loads), rows = B * C in {1, 3, 4, 5, 130} (not a multiple of the four waves of a block), and every input also as a
view that itself starts one element off a 16-byte boundary.  Values: 100 + randn, the 'sparse' pattern of tests/input_edges.py,
f16 inputs near 6e4 (their sum leaves f16's range, the mean does not).

Observed on the MI355X (4 tests, 3 s), worst fraction of the float32 bound: f32 inputs 0.23 (100 + randn) and 0.24 (sparse);
bf16 inputs 0.07 and 0.10; f16 inputs 0.07, 0.10 and 0.06 (near 6e4).  Every 16-bit output lay inside the rounded interval, every
inner = 1 output was exactly RNE(x).  The kernel did not have to change.
"""
import numpy as np
import pytest

from tests import input_edges as IE
from tests.gpu_support import dev  # noqa: F401
from tests.pool_cases import rne16

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
INNERS = (1, 3, 4, 7, 8, 9, 63, 64, 65, 255, 257, 1001, 8192)
ROWS = {1: (1, 1), 3: (1, 3), 4: (2, 2), 5: (5, 1), 130: (2, 65)}
DTYPES = ("float32", "bfloat16", "float16")
WORST = {}


def check_pool(x, out_dtype, tag):
    """global_pool of the device tensor x (B, C, inner) against float64, by the module docstring's rule."""
    import torch
    from mfas_amd.pooling import global_pool
    inner = x.shape[2]
    got = global_pool(x, getattr(torch, out_dtype)).double().cpu().numpy().ravel()
    x64 = x.double().cpu().numpy().reshape(-1, inner)
    ref = x64.mean(1)
    bound = (-(-inner // 64) + 8) * U * np.abs(x64).mean(1)
    if out_dtype == "float32":
        err = np.abs(got - ref)
        ok = err <= bound
        frac = float(np.max(np.where(err == 0, 0.0, err / np.maximum(bound, 1e-300))))
        WORST[tag[0]] = max(WORST.get(tag[0], 0.0), frac)
    elif inner == 1:
        ok = got == rne16(ref, out_dtype)
    else:
        ok = (rne16(ref - bound, out_dtype) <= got) & (got <= rne16(ref + bound, out_dtype))
    j = int(np.argmin(ok))
    assert ok.all(), f"{tag} -> {out_dtype} inner {inner}: row {j} got {got[j]!r}, mean64 {ref[j]!r}, bound {bound[j]:.3g}"


def views(vals, shape, dt, dev):
    """The values as a (B, C, inner) device tensor of dtype dt: 16-byte aligned, and as a view one element off."""
    import torch
    n = int(np.prod(shape))
    flat = torch.zeros(n + 1, dtype=dt, device=dev)
    flat[1:] = torch.from_numpy(vals.ravel()).to(dev).to(dt)
    off = flat[1:].view(shape)
    assert off.is_contiguous() and off.data_ptr() % 16 == flat.element_size() and off.contiguous().data_ptr() == off.data_ptr()
    al = flat[1:].clone().view(shape)
    assert al.data_ptr() % 16 == 0
    return (("aligned", al), ("off", off))


@pytest.mark.gpu
@pytest.mark.parametrize("in_dtype", DTYPES)
def test_global_pool_vs_float64(dev, in_dtype):
    import torch
    dt = getattr(torch, in_dtype)
    rng = np.random.default_rng(11)
    for inner in INNERS:
        for rows, (B, C) in ROWS.items():
            kinds = {"100+randn": (100.0 + rng.standard_normal((rows, inner))).astype(np.float32),
                     "sparse": IE.sparse_pattern(rng.standard_normal((rows, inner)).astype(np.float32), inner + rows)}
            if in_dtype == "float16":
                kinds["6e4"] = (60000.0 + 4000.0 * rng.random((rows, inner))).astype(np.float32)
            for kind, vals in kinds.items():
                for where, x in views(vals, (B, C, inner), dt, dev):
                    for out_dtype in DTYPES:
                        check_pool(x, out_dtype, (f"{kind}/{in_dtype}", where, rows))
    print(f"\nglobal_pool {in_dtype}: worst fraction of the float32 bound " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(WORST.items())))


@pytest.mark.gpu
def test_global_pool_output_ties(dev):
    """inner = 1, float32 inputs exactly halfway between two bf16 values (and two f16 values), lower neighbour even and odd, both
    signs: the output is exactly the round-to-nearest-even value."""
    import torch
    vals = []
    for base in (1.0, 1.0 + 2.0 ** -7, 3.0, 100.0, 100.5, 2.0 ** -20, 2.0 ** -20 * (1 + 2.0 ** -7)):
        e = 2.0 ** np.floor(np.log2(base))
        for ulp in (e * 2.0 ** -7, e * 2.0 ** -10):              # bf16 and f16 spacing at base
            vals += [base + 0.5 * ulp, base + 1.5 * ulp, -(base + 0.5 * ulp), -(base + 1.5 * ulp)]
    raw = np.array(vals, np.float64)
    vals = raw.astype(np.float32)
    assert np.array_equal(vals.astype(np.float64), raw)                 # (every tie is a float32 value)
    lower = (vals.view(np.uint32) >> np.uint32(16)) & np.uint32(1)
    assert (lower == 0).any() and (lower == 1).any()
    n = len(vals)
    for where, x in views(vals, (1, n, 1), torch.float32, dev):
        for out_dtype in DTYPES:
            check_pool(x, out_dtype, ("ties/float32", where, n))
