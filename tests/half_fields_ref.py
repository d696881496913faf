"""numpy references of the two roundings a typed finalise performs, written in integer arithmetic on the fp32 bits so that they share no
code with torch's casts or the kernel: fp32 -> bfloat16 and fp32 -> IEEE binary16, to nearest, ties to even, subnormal results kept."""
import numpy as np


def f32_to_bf16_bits(x) -> np.ndarray:
    """uint16 bits of bfloat16(x).  The carry of the rounding runs into the exponent, which is the correct result (the next binade, or
    infinity).  A NaN becomes the quiet NaN 0x7FC0 (libraries differ there; a finalised field holds none: NaN -> 0 comes first)."""
    b = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    r = (b + 0x7FFF + ((b >> 16) & 1)) >> 16
    nan = (b & 0x7FFFFFFF) > 0x7F800000
    return np.where(nan, 0x7FC0, r).astype(np.uint16)


def f32_to_f16_bits(x) -> np.ndarray:
    """uint16 bits of float16(x): normal results by re-biasing the exponent and rounding 13 mantissa bits away (the carry runs into
    the exponent; from 65520 on the result is infinity); results below 2^-14 are multiples of 2^-24, rounded as integers."""
    xf = np.ascontiguousarray(x, dtype=np.float32)
    b = xf.view(np.uint32).astype(np.uint64)
    sign = (b >> 16) & 0x8000
    a = b & 0x7FFFFFFF
    r = np.where(a >= 0x38800000, a, 0x38800000) - 0x38000000  # (127 - 15) << 23
    normal = np.minimum((r + 0xFFF + ((r >> 13) & 1)) >> 13, 0x7C00)
    with np.errstate(invalid="ignore", over="ignore"):
        sub = np.rint(np.abs(xf.astype(np.float64)) * 2.0 ** 24)  # np.rint: ties to even; exact in float64
    sub = np.where(a < 0x38800000, sub, 0).astype(np.uint64)      # (1024 = 0x0400: a subnormal that rounds up to 2^-14)
    mag = np.where(a > 0x7F800000, 0x7E00, np.where(a >= 0x38800000, normal, sub))
    return (sign | mag).astype(np.uint16)


def isqrt_array(v: np.ndarray) -> np.ndarray:
    s = np.floor(np.sqrt(v.astype(np.float64))).astype(np.int64)
    s = np.where(s * s > v, s - 1, s)
    return np.where((s + 1) * (s + 1) <= v, s + 1, s)


def four_squares(total: int):
    """Four non-negative integers whose squares sum to `total` (Lagrange), the first ones as large as possible."""
    p = int(isqrt_array(np.array([total]))[0])
    while p >= 0:
        rest = total - p * p
        q = int(isqrt_array(np.array([rest]))[0])
        while q >= 0:
            rest2 = rest - q * q
            r = np.arange(int(isqrt_array(np.array([rest2]))[0]) + 1, dtype=np.int64)
            s = isqrt_array(rest2 - r * r)
            hit = np.nonzero(s * s == rest2 - r * r)[0]
            if hit.size:
                return p, q, int(r[hit[-1]]), int(s[hit[-1]])
            q -= 1
        p -= 1
    raise AssertionError(total)


def tie_row(m: int, width: int) -> np.ndarray:
    """A float32 row of `width` >= 5 entries, multiples of 2^-12, whose squares sum to EXACTLY 1 in any order of fp32 additions (every
    partial sum is an integer below 2^24 in units of 2^-24) and whose first entry is m * 2^-12: with d = 1 the finalise returns the
    row unchanged, so an m that lies halfway between two halves reaches the rounding as an exact tie."""
    row = np.zeros(width, dtype=np.float32)
    row[:5] = np.array((m,) + four_squares((1 << 24) - m * m), dtype=np.float64) * 2.0 ** -12
    assert float((row.astype(np.float64) ** 2).sum()) == 1.0
    return row


# first entries (units of 2^-12, the binade [0.5, 1)) that are exact ties: fp16 has 2 units between neighbours there, bfloat16 16
F16_TIES = (2049, 2051)   # -> 2048 (even mantissa below), 2052 (even mantissa above)
BF16_TIES = (2056, 2072)  # -> 2048, 2080
