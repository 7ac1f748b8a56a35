"""The statistical and element-wise gates of the noise-stream tests, shared by tests/test_rng_cpu.py (applied to the numpy restatement,
tests/philox_ref.py) and tests/test_gpu_rng.py (applied to the device): the restatement passes every gate before a device is asked to.

All moment and correlation gates are at 6 sigma of the estimator under the ideal distribution (the convention of test_draw_moments); the
seeds are fixed, so the tests are deterministic.  Each gate function returns {name: (value, cap)} with |value| <= cap required; `check`
prints every figure and then asserts."""
import math

import numpy as np
from scipy import stats

# the statistical set: z = randn(B, per, seed, offset, draw)
STAT = dict(B=64, per=65536, seed=7, sample_offset=0, draw=0)
# streams that must be independent of the statistical set: (name, overrides of STAT)
OTHER_STREAMS = [("draw 1", dict(draw=1)), ("draw 2^24", dict(draw=1 << 24)), ("draw 2^32", dict(draw=1 << 32)), ("draw 2^40", dict(draw=1 << 40)),
                 ("seed 8", dict(seed=8)), ("seed 7 + 2^32", dict(seed=7 + (1 << 32))), ("offset 64", dict(sample_offset=64))]
MAX_ABS_Z = math.sqrt(-2.0 * math.log(2.0 ** -25))        # the smallest uniform is 2^-25: 5.887

# gamma cases of mcvd_gamma_noise(raw = NULL): labels of the T = 1000 linear schedule (k_cum, theta_t from the tables) and fixed k at theta = 1
GAMMA_LABELS = (0, 250, 500, 750, 999)
GAMMA_FIXED_K = (5000.0, 3.5, 1.0, 0.6, 0.3)
GAMMA = dict(B=4, per=65536, seed=11, draw=2)
GAMMA_OFFSET_CASE = (500, (1 << 32) - 2)                  # one case whose rows cross the 32-bit boundary of the sample word
UNDECIDABLE_GAP = 1e-3                                    # 250 ulp(d) at the largest k (d = 2.5e10, ulp 3.8e-6); fp64 cancellation noise is a few ulp(d)
UNDECIDABLE_CAP = 2.5e-3                                  # share of elements; the restatement alone has 0.95e-3 .. 1.65e-3 at these k (test_rng_cpu)
KS_MAX_K = 5000.0                                         # above it fp32 quantises g too coarsely for a KS test


def report(title, gates):
    for name, (v, cap) in gates.items():
        print(f"  {title}: {name} {v:+.4e} (cap {cap:.3e})")
    return gates


def check(title, gates, quiet=False):
    if not quiet:
        report(title, gates)
    bad = {name: vc for name, vc in gates.items() if not (abs(vc[0]) <= vc[1])}
    assert not bad, (title, bad)


def _moments(v):
    v = np.asarray(v, dtype=np.float64).ravel()
    m = v.mean()
    c = v - m
    var = (c * c).mean()
    return v.size, m, var, (c ** 3).mean() / var ** 1.5, (c ** 4).mean() / var ** 2 - 3.0


def normal_gates(z):
    """z: [B, per] float array, per a multiple of 4, laid out as mcvd_randn lays it out."""
    z = np.asarray(z, dtype=np.float64)
    n, m, var, skew, kurt = _moments(z)
    g = {"finite": (0.0 if np.isfinite(z).all() else 1.0, 0.0),
         "mean": (m, 6 / math.sqrt(n)),
         "var - 1": (var - 1, 6 * math.sqrt(2 / n)),
         "skew": (skew, 6 * math.sqrt(6 / n)),
         "excess kurtosis": (kurt, 6 * math.sqrt(24 / n)),
         "KS to N(0,1)": (stats.kstest(z.ravel(), "norm").statistic, 1.95 / math.sqrt(n)),      # the alpha = 0.001 point
         "max |z| - 5.887": (max(np.abs(z).max() - MAX_ABS_Z, 0.0), 0.0)}
    for t in (3, 4, 5):
        want = n * 2 * stats.norm.sf(t)
        g[f"count |z| > {t}, in sigma"] = (((np.abs(z) > t).sum() - want) / math.sqrt(want), 6.0)
    q = z.reshape(-1, 4)
    n4 = q.shape[0]
    for a, b in ((0, 1), (0, 2), (1, 3), (2, 3)):
        g[f"float4 mean z{a} z{b}, in sigma"] = ((q[:, a] * q[:, b]).mean() * math.sqrt(n4), 6.0)
    for a, b in ((0, 1), (2, 3)):
        # a Box-Muller pair: squared radius ~ Exp(scale 2) (alpha = 0.01 point, 1.63 / sqrt(m)), angle uniform (alpha = 0.001 point)
        g[f"KS z{a}^2 + z{b}^2 to Exp(2)"] = (stats.kstest(q[:, a] ** 2 + q[:, b] ** 2, "expon", args=(0, 2)).statistic, 1.63 / math.sqrt(n4))
        ang = np.mod(np.arctan2(q[:, b], q[:, a]) / (2 * np.pi), 1.0)
        g[f"KS angle(z{a}, z{b}) to U(0,1)"] = (stats.kstest(ang, "uniform").statistic, 1.95 / math.sqrt(n4))
    g["lag 1 along a row, in sigma"] = _corr(z[:, :-1], z[:, 1:])
    g["lag 4 along a row, in sigma"] = _corr(z[:, :-4], z[:, 4:])
    g["row against next row, in sigma"] = _corr(z[:-1], z[1:])
    return g


def _corr(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return ((a * b).mean() * math.sqrt(a.size), 6.0)


def pair_gates(z, other, near=None):
    """Two streams that must be independent: mean(a b) sqrt(n) within 6, and no element equal.
    The float64 restatement has no equal elements at these keys.  Values rounded to fp32 can coincide by chance: two independent fp32
    normals are equal with probability sum p_i^2 ~ 2e-8, 0.08 expected per pair of 4 194 304 -- against millions if streams were shared.
    near(flat indices) -> bool array says whether the two RESTATED values at those positions are within fp32 evaluation error of each
    other; an equal element counts unless it is such a coincidence of rounding."""
    eq = np.nonzero((np.asarray(z) == np.asarray(other)).ravel())[0]
    unexplained = eq.size if (near is None or eq.size == 0) else int((~near(eq)).sum())
    return {"mean(a b), in sigma": _corr(z, other), f"equal elements ({eq.size}) that are no rounding coincidence": (float(unexplained), 0.0)}


# ---------------------------------------------------------------------------------------------- gamma
def gamma_params():
    """[(name, k, theta, sample_offset)] with k and theta as the float32 values the library is called with: the tiny_gamma tables at
    GAMMA_LABELS (T = 1000 linear schedule), then theta = 1 at GAMMA_FIXED_K, then the offset case."""
    from oracle import synth, unet_ref
    c = unet_ref.hot_cfg(synth.make_config("tiny_gamma"))
    betas, alphas, _ = unet_ref.make_schedule(c)
    _, k_cum, theta_t = unet_ref.gamma_tables(betas, alphas)
    out = [(f"label {t}", float(k_cum[t]), float(theta_t[t]), 0) for t in GAMMA_LABELS]
    out += [(f"k {k:g}", float(np.float32(k)), 1.0, 0) for k in GAMMA_FIXED_K]
    t, off = GAMMA_OFFSET_CASE
    out.append((f"label {t} at offset 2^32 - 2", float(k_cum[t]), float(theta_t[t]), off))
    return out


def gamma_moment_gates(g, k):
    """g: Gamma(k, 1) variates (the device's out / theta, or the restatement's g).  z = (g - k) / sqrt(k) has mean 0, variance 1, skew
    2 / sqrt(k); the variance estimator of a gamma has variance (2 + 6 / k) / n."""
    g = np.asarray(g, dtype=np.float64).ravel()
    n, m, var, skew, _ = _moments((g - k) / math.sqrt(k))
    out = {"min g > 0": (0.0 if g.min() > 0 else 1.0, 0.0),
           "mean z": (m, 6 / math.sqrt(n)),
           "var z - 1": (var - 1, 6 * math.sqrt((2 + 6 / k) / n)),
           "skew z - 2 / sqrt(k)": (skew - 2 / math.sqrt(k), 6 * math.sqrt(6 / n) * (1 + 6 / k))}
    if k <= KS_MAX_K:
        out["KS to Gamma(k)"] = (stats.kstest(g, "gamma", args=(k,)).statistic, 1.95 / math.sqrt(n))
    return out


def ulp32(x):
    return np.spacing(np.abs(np.asarray(x, dtype=np.float32))).astype(np.float64)


def fl32_scaled(theta, g):
    """fl32((double)theta * g): the library's one rounding of a drawn variate."""
    return (np.float64(np.float32(theta)) * np.asarray(g, dtype=np.float64)).astype(np.float32)


def gamma_elementwise(title, ok_fn, ref, alt_fn, assert_cap=True):
    """The element rule.  ref = gamma()'s (g, attempts, gap, jmin); an element is undecidable when gap < UNDECIDABLE_GAP.
    ok_fn(g64, idx) -> bool array: does the device's value at flat indices idx agree with the restated variate g64?
    alt_fn(idx, attempt) -> the restated variates of elements idx with the decision of that attempt inverted.
    Every decidable element must agree; at most UNDECIDABLE_CAP of the elements may be undecidable (a test that excuses more hides
    failures); an undecidable element must agree with the restatement for one of the two outcomes of its closest decision.
    Returns (undecidable, elements)."""
    g, attempts, gap, jmin = (np.asarray(a).ravel() for a in ref)
    und = gap < UNDECIDABLE_GAP
    ok = ok_fn(g, np.arange(g.size))
    bad = ~ok & ~und
    idx = np.nonzero(und & ~ok)[0]
    bad_alt = int((~ok_fn(alt_fn(idx, jmin[idx]), idx)).sum()) if idx.size else 0
    print(f"  {title}: undecidable {int(und.sum())} of {g.size} = {und.mean():.3e} (cap {UNDECIDABLE_CAP:.1e}), decidable mismatches "
          f"{int(bad.sum())}, undecidable that took the other outcome {idx.size}, matching neither {bad_alt}, "
          f"attempts mean {attempts.mean():.4f} max {attempts.max()}")
    assert bad.sum() == 0, (title, "decidable elements disagree", int(bad.sum()), np.nonzero(bad)[0][:8].tolist())
    assert not assert_cap or und.mean() <= UNDECIDABLE_CAP, (title, und.mean())
    assert bad_alt == 0, (title, "undecidable elements match neither outcome", bad_alt)
    return int(und.sum()), g.size
