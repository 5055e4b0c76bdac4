"""Case module: round-to-nearest-even to the 16-bit formats."""
import numpy as np


def rne_bf16(x):
    """float64 -> the nearest bfloat16 (ties to even), as float64: rounded once, not through float32."""
    x = np.asarray(x, np.float64)
    a = np.abs(x)
    f = a.astype(np.float32)
    f = np.where(f.astype(np.float64) > a, np.nextafter(f, np.float32(0)), f).astype(np.float32)      # toward zero
    bits = f.view(np.uint32) & np.uint32(0xFFFF0000)
    d = bits.view(np.float32).astype(np.float64)
    u = (bits + np.uint32(0x10000)).view(np.float32).astype(np.float64)
    mid = 0.5 * (d + u)
    even_down = ((bits >> np.uint32(16)) & np.uint32(1)) == 0
    r = np.where(a > mid, u, np.where(a < mid, d, np.where(even_down, d, u)))
    return np.copysign(r, x)


def rne16(x, out_dtype):
    if out_dtype == "bfloat16":
        return rne_bf16(x)
    with np.errstate(over="ignore"):
        return np.asarray(x, np.float64).astype(np.float16).astype(np.float64)
