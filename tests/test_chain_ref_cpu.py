"""tests/chain_ref.py against exact rational arithmetic and against its kernels' headers, on the CPU: the mirror that the GPU tests
of tests/test_gpu_chain_exact.py compare bits with has to be right before a kernel is looked at."""
from fractions import Fraction

import numpy as np
import pytest

import chain_ref as cr

F = np.float32


def bits(x):
    return np.asarray(x, F).view(np.uint32)


def f32(hexbits):
    return np.array([hexbits], np.uint32).view(F)[0]


def round_f32(x):
    """A non-zero Fraction rounded to the nearest float32, ties to even, with subnormals and overflow to infinity."""
    sign, ax = (-1.0 if x < 0 else 1.0), abs(x)
    e = ax.numerator.bit_length() - ax.denominator.bit_length()
    if Fraction(2) ** e > ax:
        e -= 1  # 2^e <= ax < 2^(e + 1)
    quantum = Fraction(2) ** (max(e, -126) - 23)
    n = ax / quantum
    r = n.numerator // n.denominator
    rest = n - r
    if rest > Fraction(1, 2) or (rest == Fraction(1, 2) and r % 2 == 1):
        r += 1
    value = r * quantum
    if value >= Fraction(2) ** 128:
        return F(sign * np.inf)
    return F(sign * float(value))  # (a float32 value: exact in a float)


def fma_exact(a, b, c):
    """IEEE 754 fma of three finite float32 scalars through Fraction."""
    a, b, c = F(a), F(b), F(c)
    p_neg = bool(np.signbit(a)) != bool(np.signbit(b))
    x = Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c))
    if x != 0:
        return round_f32(x)
    if a == 0 or b == 0:  # (+-0) + (+-0): the common sign, or +0
        return F(-0.0) if (p_neg and c == 0 and np.signbit(c)) else F(0.0)
    return F(0.0)  # exact cancellation of non-zero terms


def assert_fma(a, b, c):
    got = cr.fma32(np.asarray(a, F), np.asarray(b, F), np.asarray(c, F))
    want = np.array([fma_exact(x, y, z) for x, y, z in zip(np.ravel(a), np.ravel(b), np.ravel(c))], F)
    wrong = np.nonzero(bits(got) != bits(want))[0]
    assert wrong.size == 0, [(float(np.ravel(a)[i]).hex(), float(np.ravel(b)[i]).hex(), float(np.ravel(c)[i]).hex(),
                              hex(bits(got)[i]), hex(bits(want)[i])) for i in wrong[:5]]


def random_f32(rng, n, lo_exp, hi_exp):
    """n float32 values with a random 24-bit significand, a random sign and an exponent drawn from [lo_exp, hi_exp]."""
    sig = rng.integers(1 << 23, 1 << 24, n).astype(np.float64)
    return (rng.choice([-1.0, 1.0], n) * np.ldexp(sig, rng.integers(lo_exp, hi_exp + 1, n) - 23)).astype(F)


# ---- fma32 --------------------------------------------------------------------------------------------------------------------------
def test_fma32_random_triples_equal_the_rational_result():
    rng = np.random.default_rng(0)
    n = 1500
    # a b and c of comparable size (cancellation and alignment shifts of up to +-30 bits), and standard normals
    a, b = random_f32(rng, n, -20, 20), random_f32(rng, n, -20, 20)
    c = (a.astype(np.float64) * b.astype(np.float64) * np.ldexp(rng.choice([-1.0, 1.0], n), rng.integers(-30, 31, n))).astype(F)
    c = (c.view(np.uint32) ^ rng.integers(0, 4, n).astype(np.uint32)).view(F)  # not the rounded product itself
    assert_fma(a, b, c)
    assert_fma(*(rng.standard_normal(n).astype(F) for _ in range(3)))


def test_fma32_random_halfway_cases():
    """The family of the constructed case: a b = 2^-24 (1 - m^2 2^-46) is half an ulp of c in [1, 2) less m^2 2^-70, which a float64
    sum cannot hold (m < 362), so the two-rounding form lands exactly on the midpoint of two float32 values and, c's last bit
    being odd, rounds away from the true result -- from below with a b > 0, from above with a b < 0."""
    rng = np.random.default_rng(1)
    n = 1000
    m = rng.integers(1, 300, n).astype(np.float64)
    a = (2.0 ** -12 * (1.0 + m * 2.0 ** -23)).astype(F)
    b = (2.0 ** -12 * (1.0 - m * 2.0 ** -23)).astype(F)
    c = (1.0 + np.ldexp(rng.integers(0, 1 << 22, n).astype(np.float64) * 2 + 1, -23)).astype(F)  # odd last bit
    for sa in (1, -1):
        for sc in (1, -1):
            x, z = F(sa) * a, F(sc) * c
            naive = (x.astype(np.float64) * b.astype(np.float64) + z.astype(np.float64)).astype(F)
            assert (bits(naive) != bits(cr.fma32(x, b, z))).mean() > 0.9  # the cases are what they claim to be
            assert_fma(x, b, z)


def test_fma32_constructed_double_rounding_case_and_its_sign_variants():
    a = F(2.0 ** -12 * (1 + 2.0 ** -23))
    b = F(2.0 ** -12 * (1 - 2.0 ** -23))
    c = F(1 + 2.0 ** -23)
    assert bits(cr.fma32(a, b, c)) == 0x3F800001
    two_roundings = F(np.float64(a) * np.float64(b) + np.float64(c))
    assert bits(two_roundings) == 0x3F800002  # what the mirror must not do
    assert bits(cr.fma32(-a, -b, c)) == 0x3F800001
    assert bits(cr.fma32(-a, b, -c)) == 0xBF800001 and bits(cr.fma32(a, -b, -c)) == 0xBF800001
    for sa, sb, sc in [(1, 1, 1), (-1, -1, 1), (-1, 1, -1), (1, -1, -1), (1, -1, 1), (-1, 1, 1), (1, 1, -1), (-1, -1, -1)]:
        assert_fma([F(sa) * a], [F(sb) * b], [F(sc) * c])


def test_fma32_subnormal_results():
    rng = np.random.default_rng(2)
    n = 1000
    a, b = random_f32(rng, n, -80, -60), random_f32(rng, n, -80, -60)  # products around 2^-160 .. 2^-120
    c = random_f32(rng, n, -149, -125)
    c[::3] = 0
    assert_fma(a, b, c)
    sub = rng.integers(1, 1 << 23, n).astype(np.uint32).view(F)  # subnormal operands
    assert_fma(sub, random_f32(rng, n, -2, 2), sub[::-1].copy())
    tiny = f32(0x00000001)
    assert bits(cr.fma32(tiny, F(0.5), F(0))) == 0  # a tie to even: +0
    assert bits(cr.fma32(tiny, F(-0.5), F(0))) == 0x80000000  # underflow keeps the sign
    assert bits(cr.fma32(tiny, F(0.75), F(0))) == 1
    assert bits(cr.fma32(tiny, F(1.5), F(0))) == 2  # a tie to even: up


def test_fma32_overflow_infinities_nan_and_signed_zeros():
    big = f32(0x7F7FFFFF)
    inf, nan = F(np.inf), F(np.nan)
    assert bits(cr.fma32(big, F(2), F(0))) == 0x7F800000 and bits(cr.fma32(big, F(-2), F(0))) == 0xFF800000
    assert bits(cr.fma32(big, F(2), -big)) == 0x7F7FFFFF  # the product alone overflows, the fused sum does not
    half_ulp = f32(0x73000000)  # 2^103: the tie between the largest float32 and 2^128 goes to even, which is the overflow
    assert bits(cr.fma32(big, F(1), half_ulp)) == 0x7F800000 == bits(fma_exact(big, 1, half_ulp))
    assert bits(cr.fma32(big, F(1), np.nextafter(half_ulp, F(0)))) == 0x7F7FFFFF
    assert bits(cr.fma32(F(2.0 ** 100), F(2.0 ** 100), F(1))) == 0x7F800000
    rng = np.random.default_rng(3)
    n = 500
    assert_fma(random_f32(rng, n, 60, 66), random_f32(rng, n, 60, 66), random_f32(rng, n, 120, 127))
    assert bits(cr.fma32(inf, F(1), F(1))) == 0x7F800000 and bits(cr.fma32(F(-1), inf, big)) == 0xFF800000
    assert bits(cr.fma32(F(1), F(1), -inf)) == 0xFF800000 and bits(cr.fma32(big, big, -inf)) == 0xFF800000
    for a, b, c in ((inf, F(0), F(1)), (inf, F(1), -inf), (nan, F(1), F(1)), (F(1), F(1), nan), (F(0), -inf, nan)):
        assert np.isnan(cr.fma32(a, b, c))
    z, nz = F(0.0), F(-0.0)
    for a, b, c, want in ((z, z, z, 0), (z, z, nz, 0), (nz, z, nz, 0x80000000), (nz, z, z, 0), (nz, nz, nz, 0), (z, F(5), nz, 0),
                          (nz, F(5), nz, 0x80000000), (F(3), F(-2), F(6), 0), (F(-3), F(2), F(6), 0), (F(3), F(2), F(-6), 0),
                          (z, z, F(-1.5), 0xBFC00000), (nz, F(7), F(2), 0x40000000)):
        assert bits(cr.fma32(a, b, c)) == want, (a, b, c)
    # vectorised and broadcast, with mixed special values in one call
    a = np.array([[1.0], [np.inf], [0.0]], F)
    b = np.array([2.0, -0.0, np.nan], F)
    got = cr.fma32(a, b, F(-0.0))
    assert got.shape == (3, 3) and got.dtype == F
    assert bits(got[0, 0]) == 0x40000000 and bits(got[0, 1]) == 0x80000000 and np.isnan(got[1, 1]) and np.isnan(got[2, 2])


# ---- chain --------------------------------------------------------------------------------------------------------------------------
def test_chain_in_ascending_order_equals_a_scalar_loop():
    rng = np.random.default_rng(4)
    A, B = rng.standard_normal((5, 37)).astype(F), rng.standard_normal((4, 37)).astype(F)
    got = cr.chain(A, B, range(37))
    assert got.shape == (5, 4) and got.dtype == F
    for g in range(5):
        for j in range(4):
            acc = F(0.0)
            for k in range(37):
                acc = fma_exact(A[g, k], B[j, k], acc)
            assert bits(got[g, j]) == bits(acc)


def test_chain_executes_the_padded_steps_as_products_of_zeros():
    A, B = np.array([[-0.0, 1.0]], F), np.array([[1.0, -0.0]], F)
    assert bits(cr.chain(A, B, [0, 1]))[0, 0] == 0  # from +0: (+0) + (-0) = +0
    A, B = np.array([[1.0, 1.0]], F), np.array([[-1.0, 1.0]], F)
    assert bits(cr.chain(A, B, [0, 1]))[0, 0] == 0
    # a sum that underflows to -0 stays -0 without a padded step and becomes +0 with one
    tiny = f32(0x00000001)
    A, B = np.array([[tiny]], F), np.array([[-0.25]], F)
    assert bits(cr.chain(A, B, [0]))[0, 0] == 0x80000000
    assert bits(cr.chain(A, B, [0, 1]))[0, 0] == 0
    assert bits(cr.chain(A, B, cr.knn_order(1)))[0, 0] == 0


def test_the_documented_order_and_ascending_order_give_different_bits():
    rng = np.random.default_rng(5)
    A, B = rng.standard_normal((40, 100)).astype(F), rng.standard_normal((30, 100)).astype(F)
    a, b = cr.chain(A, B, cr.knn_order(100)), cr.chain(A, B, range(128))
    differ = float((bits(a) != bits(b)).mean())
    print(f"knn_order against ascending k at D = 100: {100 * differ:.1f} % of the entries differ")
    assert differ > 0.3
    assert np.abs(a.astype(np.float64) - A.astype(np.float64) @ B.astype(np.float64).T).max() < 1e-4


# ---- the orders ---------------------------------------------------------------------------------------------------------------------
def pad(n, m):
    return -(-n // m) * m


@pytest.mark.parametrize("gen, length, padded", [(cr.knn_order, [1, 30, 32, 33, 36, 64, 1024, 1028], lambda n: pad(n, 32)),
                                                 (cr.prompt_order, [1, 30, 32, 33, 36, 64, 1024, 1028], lambda n: pad(n, 32)),
                                                 (cr.encode_order, [16, 32, 64, 128, 512, 2048], lambda n: n),
                                                 (cr.decode_y_order, [16, 48, 128], lambda n: n),
                                                 (cr.decode_gr_order, [16, 48, 64, 80, 528, 1040, 2048], lambda n: n),
                                                 (cr.decode_gc_order, [1, 5, 14, 64, 65, 128, 4096], lambda n: pad(n, 64))])
def test_every_order_is_a_permutation_of_its_padded_range(gen, length, padded):
    for n in length:
        order = gen(n)
        assert sorted(order) == list(range(padded(n))), (gen.__name__, n)


BLOCK16 = [0, 4, 8, 12, 1, 5, 9, 13, 2, 6, 10, 14, 3, 7, 11, 15]  # one 16-block: MFMA step i consumes slots q = 0 .. 3 of k = 4 q + i


def test_pinned_orders_written_out_from_the_headers():
    # knn_tile.h: k = 32 c + 16 b + 4 q + i in the order (c, b, i, q); D = 1 pads to one chunk of 32
    first_chunk = [0, 4, 8, 12, 1, 5, 9, 13, 2, 6, 10, 14, 3, 7, 11, 15, 16, 20, 24, 28, 17, 21, 25, 29, 18, 22, 26, 30, 19, 23, 27, 31]
    assert cr.knn_order(1) == first_chunk and cr.knn_order(32) == first_chunk
    assert cr.knn_order(33) == first_chunk + [32 + k for k in first_chunk]
    # query.hip: the same index arithmetic, read off its staging loop
    assert cr.prompt_order(1) == first_chunk and cr.prompt_order(36)[32:40] == [32, 36, 40, 44, 33, 37, 41, 45]
    # encode.hip: k = 16 j + 4 q + i in the order (j, i, q)
    assert cr.encode_order(16) == BLOCK16
    assert cr.encode_order(32) == BLOCK16 + [16, 20, 24, 28, 17, 21, 25, 29, 18, 22, 26, 30, 19, 23, 27, 31]
    # decode_loss.hip, y: for b, for s: k = 16 b + s, 16 b + 4 + s, 16 b + 8 + s, 16 b + 12 + s
    assert cr.decode_y_order(16) == BLOCK16 and cr.decode_y_order(32)[16:20] == [16, 20, 24, 28]
    # GR: j = 64 c + 16 t + r + 0, 4, 8, 12 for t, for r; D = 80 is one whole chunk and one tile of the next
    assert cr.decode_gr_order(16) == BLOCK16
    assert cr.decode_gr_order(80)[:20] == BLOCK16 + [16, 20, 24, 28] and cr.decode_gr_order(80)[64:] == [64 + k for k in BLOCK16]
    # GC: pixel 16 u + r + 0, 4, 8, 12 for u, for r, of 64-pixel blocks
    assert cr.decode_gc_order(1) == BLOCK16 + [16 + k for k in BLOCK16] + [32 + k for k in BLOCK16] + [48 + k for k in BLOCK16]
    assert cr.decode_gc_order(65)[64:68] == [64, 68, 72, 76]
    # the slice plan: 64-pixel blocks, ceil(blocks / 512) blocks per slice
    assert cr.decode_slices(5) == [(0, 5)] and cr.decode_slices(64) == [(0, 64)] and cr.decode_slices(65) == [(0, 64), (64, 65)]
    s = cr.decode_slices(70 * 45)
    assert len(s) == 50 and s[0] == (0, 64) and s[-1] == (3136, 3150)
    s = cr.decode_slices(64 * 512)
    assert len(s) == 512 and s[-1] == (64 * 511, 64 * 512)
    s = cr.decode_slices(64 * 512 + 1)  # 513 blocks: two per slice
    assert len(s) == 257 and s[0] == (0, 128) and s[-1] == (64 * 512, 64 * 512 + 1)


# ---- the operations on top of the chains --------------------------------------------------------------------------------------------
def test_topk_and_assign_follow_the_kernels_tie_rules():
    sc = np.array([[1.0, 3.0, 3.0, -0.0, 0.0, np.inf], [-np.inf, -1.0, -np.inf, -1.0, -2.0, -3.0]], F)
    idx, score = cr.topk(sc, 5)
    assert idx.tolist() == [[5, 1, 2, 0, 3], [1, 3, 4, 5, 0]]
    assert bits(score[0]).tolist() == [0x7F800000, 0x40400000, 0x40400000, 0x3F800000, 0]  # -0 is returned as +0
    label, best = cr.assign(sc[:, :5])
    assert label.tolist() == [1, 1] and bits(best).tolist() == [0x40400000, 0xBF800000]
    label, best = cr.assign(np.array([[-0.0, 0.0], [np.nan, np.nan], [np.nan, -5.0]], F))
    assert label.tolist() == [0, -1, 1] and bits(best)[0] == 0 and np.isnan(best[1]) and best[2] == -5.0
    label, best = cr.assign(np.array([[1.0, 1.0, 1.0]], F), np.array([0.0, 2.0 ** -24, -1.0], F))
    assert label.tolist() == [0] and best[0] == 1.0  # ONE fp32 addition: 1 + 2^-24 rounds to 1, the tie goes to the lowest index


def test_decode_loss_mirror_is_close_to_the_float64_reference():
    import decode_ref
    for loss in ("l1", "l2"):
        R, C, M = decode_ref.kernel_inputs(70, 16, 32, seed=1, loss=loss)
        M[3, 5] = np.inf
        w = np.random.default_rng(6).uniform(0.0, 2.0, 70).astype(F)
        want = decode_ref.reference(R, C, M, loss, 0.125, w)
        GR, GC = cr.decode_loss(R, C, M, loss, 0.125, w)
        assert GR.dtype == F and GC.dtype == F and not GR[3].any()
        assert np.abs(GR - want["GR"]).max() <= 1e-5 * np.abs(want["GR"]).max()
        assert np.abs(GC - want["GC"]).max() <= 1e-5 * np.abs(want["GC"]).max()
