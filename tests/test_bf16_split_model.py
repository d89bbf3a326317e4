"""The numpy model of the bf16 split behind the warm filter's middle products
(dfm_internal.h: x ~ h + m + l; dfm_gemm.hip gemmh_zrm_split_kernel), on the
CPU.  tests/test_gpu_bf16_split.py builds its references with split3 and
SIX, so this file keeps that side honest:

* h + m + l reproduces x to 2^-26 |x|: a round-to-nearest bf16 leaves a
  remainder of at most half a unit of its 8-bit significand, so each plane's
  exponent is at least 9 below the previous one's (a tie is a power of two,
  which the next plane holds exactly), and the third remainder is below
  2^-27 of x's leading power of two;
* the six plane pairs of weight >= 2^-18, accumulated in fp32, are as close to
  the exact product as an fp32 matmul (bound: 2 x fp32's error), and three
  pairs are not.
"""
import numpy as np

# (H plane, Z plane) of the six terms in the kernel's order, small terms first
SIX = ((2, 0), (0, 2), (1, 1), (1, 0), (0, 1), (0, 0))


def bf16_rne(x):
    """double -> bf16 (as double): the fp32 rounding, then round to nearest even on its upper 16 bits."""
    u = np.asarray(x, dtype=np.float64).astype(np.float32).view(np.uint32)
    u = (u + np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1))) & np.uint32(0xFFFF0000)
    return u.view(np.float32).astype(np.float64)


def split3(x):
    """The planes h, m, l of x (doubles holding bf16 values); differences in fp64."""
    x = np.asarray(x, dtype=np.float64)
    h = bf16_rne(x)
    m = bf16_rne(x - h)
    l = bf16_rne(x - h - m)
    return h, m, l


def split_matmul(H, Z, terms=SIX, ks=16):
    """The kernel's arithmetic: per 16-deep k stage and per term one exact
    plane product (a product of two bf16 numbers is exact in fp32; the stage's
    sum is taken in fp64 here), added to an fp32 accumulator."""
    Hp, Zp = split3(H), split3(Z)
    acc = np.zeros((H.shape[0], Z.shape[1]), dtype=np.float32)
    for k0 in range(0, H.shape[1], ks):
        for i, j in terms:
            acc = (acc.astype(np.float64) + Hp[i][:, k0:k0 + ks] @ Zp[j][k0:k0 + ks]).astype(np.float32)
    return acc.astype(np.float64)


def test_three_planes_keep_24_bits():
    rng = np.random.default_rng(1500)
    x = rng.standard_normal(200_000)
    cases = [x, x * rng.uniform(1e-3, 1e3, size=x.size), x * 2.0 ** rng.integers(-60, 60, size=x.size),
             2.0 ** rng.integers(-60, 60, size=1000).astype(np.float64),   # exact powers of two
             np.array([0.0, 1.0, -1.0, 1.0 + 2.0 ** -8, 1.0 + 2.0 ** -9, 1.0 - 2.0 ** -9, 255.0 / 256, 3.0 * 2.0 ** -9])]
    for v in cases:
        h, m, l = split3(v)
        for pl in (h, m, l):   # every plane is a bf16 number
            assert np.array_equal(pl, bf16_rne(pl))
        err = np.abs(v - (h + m + l))
        assert np.all(err <= 2.0 ** -26 * np.abs(v)), (err / np.maximum(np.abs(v), 1e-300)).max()
        assert np.all(np.abs(v - h) <= 2.0 ** -8 * np.abs(v))


def test_six_terms_match_fp32_and_three_do_not():
    T, ncol = 200, 96
    rng = np.random.default_rng(1501)
    E = rng.standard_normal((T, 2 * T)) * rng.uniform(0.2, 3.0, size=(T, 1))
    H = E @ E.T
    H /= H.diagonal().max()
    Z = rng.standard_normal((T, ncol)) * np.exp(rng.uniform(-2.0, 2.0, size=(1, ncol)))
    exact = H @ Z

    def rel(a):
        return np.linalg.norm(a - exact) / np.linalg.norm(exact)

    f32 = rel((H.astype(np.float32) @ Z.astype(np.float32)).astype(np.float64))
    six = rel(split_matmul(H, Z))
    three = rel(split_matmul(H, Z, terms=((1, 0), (0, 1), (0, 0))))
    print(f"fp32 {f32:.3e}  six terms {six:.3e}  three terms {three:.3e}")
    assert six <= 2.0 * f32
    assert three > 2.0 * f32
