"""The error bound behind the first stage of the threshold self-join (join_kernels.h), checked on the CPU the way
tests/test_prefilter_bound.py checks the search's: BOTH rows are rounded to bf16 now, so
|coarse - exact| <= eps2 = 2^-7 + 2^-16 + 4.1 (dim + 8) 2^-24 + 2e-6 for the cosine distance of two bf16-rounded rows
(fp32 accumulation, the rows' stored fp32 norms) against the fp32 distance — on random rows, near neighbours, rows of
scales 1e-6 .. 1e6 and pairs built to sit at the worst case of the rounding (both rows' low mantissa bits 0x7FFF, signs
aligned)."""
import numpy as np

DIM = 768
EPS2 = 2.0 ** -7 + 2.0 ** -16 + 4.1 * (DIM + 8) * 2.0 ** -24 + 2e-6   # (2u + u^2) with u = 2^-8, then the fp32 terms
EPS_SEARCH = 2.0 ** -8 + 4.1 * (DIM + 8) * 2.0 ** -24 + 2e-6            # the search's bound: ONE rounded operand


def bf16_rne(x: np.ndarray) -> np.ndarray:
    u = x.astype(np.float32).view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16
    return r.astype(np.uint32).view(np.float32)


def dot32(a, b):
    """fp32 throughout, chunked like the kernels (any order: that is inside the bound's gamma terms)"""
    acc = np.float32(0)
    for c in range(0, DIM, 64):
        acc = np.float32(acc + np.dot(a[c:c + 64], b[c:c + 64]).astype(np.float32))
    return acc


def exact_dist(x, y):
    x = x.astype(np.float32); y = y.astype(np.float32)
    return np.float32(1) - dot32(x, y) / (np.sqrt(dot32(x, x)) * np.sqrt(dot32(y, y)))


def coarse_dist(x, y):
    """stage 1: the product of the two mirror rows over the square roots of the norms stored beside them (fp32, of the
    unrounded rows)"""
    x = x.astype(np.float32); y = y.astype(np.float32)
    return np.float32(1) - dot32(bf16_rne(x), bf16_rne(y)) / (np.sqrt(dot32(x, x)) * np.sqrt(dot32(y, y)))


def worst_pair(rng, sign):
    """both rows just under half a bf16 ulp above a representable value (low 16 bits 0x7FFF: rounded DOWN by almost
    2^-8 relative), every product of the same sign: the errors of all 768 terms add up"""
    def row():
        base = (0.5 + rng.random(DIM)).astype(np.float32)
        return ((base.view(np.uint32) & np.uint32(0xFFFF0000)) | np.uint32(0x7FFF)).view(np.float32)
    s = np.where(rng.random(DIM) < 0.5, -1.0, 1.0).astype(np.float32)
    return row() * s, row() * s * np.float32(sign)


def test_join_bound_holds_on_random_near_scaled_and_worst_case_pairs():
    rng = np.random.default_rng(0)
    worst = 0.0
    for trial in range(400):
        kind = trial % 4
        if kind == 0:
            x = rng.standard_normal(DIM).astype(np.float32)
            y = rng.standard_normal(DIM).astype(np.float32)
        elif kind == 1:   # a near neighbour: where membership is decided
            x = rng.standard_normal(DIM).astype(np.float32)
            y = (x + 0.05 * rng.standard_normal(DIM)).astype(np.float32)
        elif kind == 2:   # scales 1e-6 .. 1e6, independently for the two rows
            x = rng.standard_normal(DIM).astype(np.float32) * np.float32(10.0 ** rng.integers(-6, 7))
            y = (x * np.float32(10.0 ** rng.integers(-6, 7)) + np.float32(0.1) * np.abs(x).max() * rng.standard_normal(DIM)).astype(np.float32)
        else:
            x, y = worst_pair(rng, 1.0 if trial % 8 == 3 else -1.0)
        err = abs(float(coarse_dist(x, y)) - float(exact_dist(x, y)))
        worst = max(worst, err)
        assert err <= EPS2, (trial, kind, err, EPS2)
    assert worst > 0.5 * 2.0 ** -7      # the constructed pairs do come close to the bound: it is not vacuous
    assert worst > EPS_SEARCH           # ... and the search's own eps (one rounded operand, 2^-8) would be violated


def test_marked_rows_are_what_the_bound_leaves_out():
    """the bound needs finite products and norms: rows the mirror marks (xx = -1) never reach the comparison"""
    x = np.full(DIM, 1e-17, np.float32)
    xx = float(dot32(x, x))
    assert 0.0 < xx < 1e-30   # finite in fp32, outside the mirror's [1e-30, 1e30]: marked, stage 2 decides
    y = np.full(DIM, 1e16, np.float32)
    assert float(dot32(y, y)) > 1e30
    assert float(exact_dist(x, y)) <= 1e-6   # copies in direction: the pair the join must still find
