"""CPU: the numpy restatement of the device noise streams (tests/philox_ref.py) is itself checked -- Philox4x32-10 against Random123's
known answers, the counter layout for distinct streams, the uniforms' edge values, the restated normals under the statistical gates that
tests/test_gpu_rng.py applies to the device (tests/rng_gates.py), and the restated gamma variates against scipy.stats.gamma."""
import functools
import math

import numpy as np
import pytest

from tests import philox_ref as pr
from tests import rng_gates as rg


@functools.lru_cache(maxsize=None)
def stat_stream(**over):
    """The restated statistical set (float64, [B, per]) or one of its sibling streams; computed once per process and left unchanged."""
    a = pr.randn_call(**{**rg.STAT, **over})
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def gamma_ref(k, sample_offset):
    ref = pr.gamma_call(k, rg.GAMMA["B"], rg.GAMMA["per"], rg.GAMMA["seed"], sample_offset, rg.GAMMA["draw"])
    for a in ref:
        a.setflags(write=False)
    return ref


KAT = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
       ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
       ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]


@pytest.mark.parametrize("ctr,key,want", KAT)
def test_philox_known_answers(ctr, key, want):
    """Random123's kat_vectors for philox4x32 at 10 rounds."""
    got = tuple(int(w) for w in pr.philox4x32_10(*ctr, *key))
    assert got == want, [hex(w) for w in got]


def test_philox_is_vectorised_consistently():
    """An array call equals element-by-element calls (the layout helpers rely on broadcasting)."""
    c0 = np.arange(5, dtype=np.uint64)[None, :]
    c2 = (np.uint64(0xFFFFFFFE) + np.arange(3, dtype=np.uint64))[:, None]
    out = pr.philox4x32_10(c0, 7, c2 & pr.M32, c2 >> np.uint64(32), 0x7F4A7C15, 0x9E3779B9)
    for i in range(3):
        for j in range(5):
            one = pr.philox4x32_10(j, 7, int(c2[i, 0]) & 0xFFFFFFFF, int(c2[i, 0]) >> 32, 0x7F4A7C15, 0x9E3779B9)
            assert [int(w[i, j]) for w in out] == [int(w) for w in one]


def test_draw_words_are_distinct_streams():
    """The draw words philox.h lists give pairwise different (c1, c3) for one sample below 2^32 -- and so for any, as c3 only gains the
    sample's (zero) high word.  The documented collision: (sample + 2^32, draw) is the stream of (sample, draw ^ 2^24)."""
    base = list(range(1001)) + [(1 << 32) + k for k in range(1001)]
    words = base + [w | (1 << 39) for w in base] + [1 << 40, (1 << 40) | (1 << 39)]
    assert len(set(words)) == len(words) == 4006
    for sample in (0, 1, (1 << 32) - 1):
        seen = {}
        for w in words:
            c0, c1, c2, c3 = (int(v) for v in pr.counter(sample, w, 5))
            assert (c0, c2) == (5, sample)
            assert seen.setdefault((c1, c3), w) == w, (hex(w), hex(seen[(c1, c3)]))
    for sample, draw in ((3, 0), (3, 1 << 24), (77, (1 << 32) + 9), (0, 1 << 40)):
        a = tuple(int(v) for v in pr.counter(sample + (1 << 32), draw, 5))
        b = tuple(int(v) for v in pr.counter(sample, draw ^ (1 << 24), 5))
        assert a == b
    assert pr.counter(0, 1 << 39, 0)[3] == 1 << 15 and pr.counter(0, 1 << 40, 0)[3] == 1 << 16 and pr.counter(0, 1 << 32, 0)[3] == 1 << 8
    assert pr.counter(0, (1 << 24) - 1, 1 << 32)[1] == 0xFFFFFF00 ^ 1


def test_uniform_edges():
    """(float32(c >> 8) + 0.5f) * 2^-24: exact below 2^23, rounded to even above; the top word gives 1.0, the bottom 2^-25: (0, 1]."""
    c = np.array([0, 255, 256, (1 << 31) - 1, 1 << 31, (1 << 31) | (1 << 8), 0xFFFFFE00, 0xFFFFFF00, 0xFFFFFFFF], dtype=np.uint64)
    u = pr.uniform32(c)
    assert u.dtype == np.float32
    m = [0, 0, 1, (1 << 23) - 1, 1 << 23, (1 << 23) + 1, (1 << 24) - 2, (1 << 24) - 1, (1 << 24) - 1]
    # ties to even: 2^23 + 0.5 -> 2^23, 2^23 + 1.5 -> 2^23 + 2, 2^24 - 1.5 -> 2^24 - 2, 2^24 - 0.5 -> 2^24
    sums = [0.5, 0.5, 1.5, (1 << 23) - 0.5, float(1 << 23), float((1 << 23) + 2), float((1 << 24) - 2), float(1 << 24), float(1 << 24)]
    assert [float(v) for v in u] == [s * 2.0 ** -24 for s in sums], (m, u)
    assert float(u[0]) == 2.0 ** -25 and float(u[-1]) == 1.0


def test_normals_order_and_edges():
    """One counter by hand: (r0 cos, r0 sin, r1 cos, r1 sin) from (u0, u1), (u2, u3); normals32 stays within fp32 evaluation error."""
    seed, sample, draw, e4 = 0x9E3779B97F4A7C15, (1 << 32) + 1, (1 << 32) + 3, 9
    k0, k1 = seed & 0xFFFFFFFF, seed >> 32
    w = pr.philox4x32_10(e4, ((draw << 8) & 0xFFFFFFFF), sample & 0xFFFFFFFF, (sample >> 32) ^ (draw >> 24), k0, k1)
    u = [(math.floor(int(v) / 256) + 0.5) / 2 ** 24 for v in w]
    u = [float(np.float32(v)) for v in u]
    want = [math.sqrt(-2 * math.log(u[0])) * math.cos(2 * math.pi * u[1]), math.sqrt(-2 * math.log(u[0])) * math.sin(2 * math.pi * u[1]),
            math.sqrt(-2 * math.log(u[2])) * math.cos(2 * math.pi * u[3]), math.sqrt(-2 * math.log(u[2])) * math.sin(2 * math.pi * u[3])]
    got = pr.normals(seed, sample, draw, e4)
    assert got.shape == (4,) and np.allclose(got, want, rtol=0, atol=1e-14)
    assert np.abs(pr.normals32(seed, sample, draw, e4) - got).max() < 1e-5


def test_layout_helpers():
    """[B, per]: row b is sample offset + b, the float4 i of a row is counter i; gamma element e of a row reads counters 8 e + j."""
    z = pr.randn_call(3, 8, 5, 10, 2)
    assert z.shape == (3, 8)
    assert np.array_equal(z[2, 4:], pr.normals(5, 12, 2, 1))
    g, att, gap, jmin = pr.gamma_call(3.5, 2, 6, 5, 10, 2)
    one = pr.gamma(3.5, 5, 11, 2, 4)
    assert g.shape == (2, 6) and g[1, 4] == one[0] and att[1, 4] == one[1] and gap[1, 4] == one[2]
    ux, uy, uz, uw = pr.uniforms(5, 11, 2 | (1 << 39), 8 * 4)
    d = 3.5 - 1 / 3
    x = math.sqrt(-2 * math.log(float(ux))) * math.cos(2 * math.pi * float(uy))
    v = (1 + x / math.sqrt(9 * d)) ** 3
    if v > 0 and math.log(float(uz)) < 0.5 * x * x + d - d * v + d * math.log(v):
        assert att[1, 4] == 1 and math.isclose(g[1, 4], d * v, rel_tol=1e-14)
    else:
        assert att[1, 4] > 1


def test_gamma_flip():
    """flip inverts exactly one decision: an accepted first attempt moves on to the second counter, a rejected one is accepted."""
    elem = np.arange(4096, dtype=np.uint64)
    g, att, gap, jmin = pr.gamma(0.6, 3, 0, 1, elem)
    assert att.max() > 1 and att.min() == 1
    g2, att2, _, _ = pr.gamma(0.6, 3, 0, 1, elem, flip=np.zeros(4096, dtype=np.int64))
    first_ok = att == 1
    assert np.all(att2[first_ok] >= 2) and np.all(att2[~first_ok] == 1)
    assert np.all(g2 != g)


def test_restated_normals_pass_the_gates():
    """The gates of the device test (3b), on the restated stream at the same keys."""
    z = stat_stream()
    rg.check("restated normals", rg.normal_gates(z))
    for name, over in rg.OTHER_STREAMS:
        rg.check(f"restated normals vs {name}", rg.pair_gates(z, stat_stream(**over)))


def test_statistical_set_holds_a_unit_uniform():
    """The set contains a u = 1.0 (a Box-Muller radius of exactly 0): the closed end of (0, 1] stays covered by the element-exact test."""
    z = stat_stream().reshape(-1, 4)
    zero_pairs = int(((z[:, 0] == 0) & (z[:, 1] == 0)).sum() + ((z[:, 2] == 0) & (z[:, 3] == 0)).sum())
    print(f"  Box-Muller pairs with radius 0 in the statistical set: {zero_pairs}")
    assert zero_pairs >= 1


@functools.lru_cache(maxsize=None)
def fp32_evaluation_error():
    """max |normals32 - normals| over the statistical set and the |z| it occurs at: what fp32 evaluation costs, from the reference alone."""
    d = np.abs(pr.randn_call(**rg.STAT, fn=pr.normals32).astype(np.float64) - stat_stream())
    i = np.unravel_index(d.argmax(), d.shape)
    return float(d.max()), float(abs(stat_stream()[i]))


def test_fp32_evaluation_error_of_the_normals():
    """The figure that sizes the device tolerance of test_gpu_rng's element-exact test (4 x this): 1.73e-6 at |z| = 0.81 with numpy's
    float32 libm, dominated by the rounding of the angle."""
    dmax, at = fp32_evaluation_error()
    print(f"  max |normals32 - normals| = {dmax:.3e} at |z| = {at:.3f}")
    # 2 pi u is rounded to fp32 (half an ulp of an angle below 8 is 2.4e-7, and fl32(2 pi) is 1.7e-7 off) and multiplied by r <= 5.9
    assert 1e-7 < dmax < 5.9 * (2.4e-7 + 1.8e-7 + 1.2e-7) + 5.9 * 2 ** -24


@pytest.mark.parametrize("case", range(11))
def test_restated_gamma_against_scipy(case):
    """Mean, variance and skew of z = (g - k) / sqrt(k) against theory at every k of the device test (3d), a KS test against
    scipy.stats.gamma for k <= 5000, and the undecidable share under its cap."""
    name, k, theta, off = rg.gamma_params()[case]
    g, att, gap, _ = gamma_ref(k, off)
    rg.check(f"restated gamma, {name} (k = {k:.6g})", rg.gamma_moment_gates(g, k))
    share = (gap < rg.UNDECIDABLE_GAP).mean()
    print(f"  restated gamma, {name}: undecidable share {share:.3e}, attempts mean {att.mean():.4f}, max {att.max()}")
    assert share <= rg.UNDECIDABLE_CAP
