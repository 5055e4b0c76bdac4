"""Case module: the golden fixtures' configurations, variants and check."""
import numpy as np

from oracle import np_oracle as O


CONFS = {
    "c4": [[3, 1, 1], [1, 3, 0], [1, 1, 1], [3, 3, 0]],
    "c0": [[2, 2, 0], [1, 0, 1], [3, 2, 0], [3, 1, 1]],
    "l1": [[0, 0, 0]],
    "l2": [[2, 3, 1], [0, 2, 2]],
    "l3": [[1, 0, 2], [3, 3, 1], [0, 1, 0]],
}
VARIANTS = {
    "bn_train": (dict(bn=True, drpt=0.0), True),
    "bn_eval": (dict(bn=True, drpt=0.0), False),
    "bndrop_eval": (dict(bn=True, drpt=0.5), False),
    "drop_eval": (dict(bn=False, drpt=0.5), False),
    "alpha_bn_train": (dict(bn=True, drpt=0.0, alphas=True), True),
    "mt_bn_train": (dict(bn=True, drpt=0.0, multitask=True), True),
}


def check(g, key, arr, rtol, atol, scale_atol=0.0, loose_atol=None):
    """scale_atol: extra absolute tolerance as a fraction of max|expected| (fp32 cancellation noise
    in BN-backward is relative to the tensor's scale, not the element).
    loose_atol: Adam normalises by sqrt(v), so an element whose gradient is at round-off level moves
    by up to ~lr per step in either direction; <=3% of the elements may miss the tight tolerance
    but every element must meet this loose one."""
    full = key in g
    want = g[key] if full else g[key + "#s"]
    got = np.asarray(arr) if full else O.sample_view(arr)
    atol = atol + scale_atol * float(np.abs(want).max())
    if loose_atol is None:
        np.testing.assert_allclose(got, want, rtol=rtol, atol=atol, err_msg=key)
    else:
        bad = np.abs(got - want) > atol + rtol * np.abs(want)
        assert bad.mean() <= 0.03, (key, bad.mean())
        np.testing.assert_allclose(got, want, rtol=rtol, atol=loose_atol, err_msg=key)
    if not full:
        np.testing.assert_allclose(np.asarray(arr, np.float64).sum(), g[key + "#sum"], rtol=2e-3,
                                   atol=atol * arr.size ** 0.5, err_msg=key + "#sum")
