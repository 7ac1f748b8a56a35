"""A plain numpy restatement of the library's device noise streams, written from the documentation in csrc/kernels/philox.h (tests only).

The generator is counter-based, so every value the device produces can be recomputed here from its key:

    key      = (seed low word, seed high word)
    counter  = (ctr low, ctr high ^ (draw << 8), sample low, sample high ^ (draw >> 24)), each a 32-bit word
    bits     = Philox4x32-10 (Salmon et al. 2011: multipliers D2511F53 / CD9E8D57, key increments 9E3779B9 / BB67AE85)
    uniforms = (float32(c >> 8) + 0.5f) * 2^-24 in float32 -- in (0, 1]: bit-exact in numpy (one conversion, one add, one multiply by
               a power of two); for c >> 8 >= 2^23 the add rounds, and c >> 8 = 2^24 - 1 gives u = 1.0
    normals  = Box-Muller, (r0 cos a0, r0 sin a0, r1 cos a1, r1 sin a1) with r0 from u0, a0 from u1, r1 from u2, a1 from u3;
               ctr = the float4's index within its row
    gamma    = Marsaglia & Tsang (2000) on the stream with bit 39 ORed into the draw word; attempt j of element e has ctr = 8 e + j

`normals` and `gamma` evaluate in float64 from the float32 uniforms: they are the references.  `normals32` evaluates every operation in
float32 and serves only to size a tolerance: its distance from `normals` is what fp32 evaluation costs, measured on the reference alone.
"""
import numpy as np

M32 = np.uint64(0xFFFFFFFF)
GAMMA_BIT = 1 << 39
MAX_ATTEMPTS = 8
TWO_PI = 6.283185307179586


def _w(v):
    """Anything integer-like -> uint64 array masked to 32 bits."""
    return np.asarray(v, dtype=np.uint64) & M32


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Ten rounds of Philox4x32 on uint64 arrays that hold 32-bit words.  Returns the four output words."""
    c0, c1, c2, c3 = np.broadcast_arrays(_w(c0), _w(c1), _w(c2), _w(c3))
    k0, k1 = _w(k0), _w(k1)
    m0, m1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
    w0, w1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
    s32 = np.uint64(32)
    for _ in range(10):
        p0, p1 = m0 * c0, m1 * c2                                     # 32 x 32 -> 64 bits: no overflow in uint64
        c0, c1, c2, c3 = (p1 >> s32) ^ c1 ^ k0, p1 & M32, (p0 >> s32) ^ c3 ^ k1, p0 & M32
        k0, k1 = (k0 + w0) & M32, (k1 + w1) & M32
    return c0, c1, c2, c3


def counter(sample, draw, ctr):
    """The four counter words of (sample, draw, ctr).  `draw` is a Python int; sample and ctr are ints or uint64 arrays."""
    draw = int(draw)
    sample, ctr = np.asarray(sample, dtype=np.uint64), np.asarray(ctr, dtype=np.uint64)
    s32 = np.uint64(32)
    d_lo = np.uint64((draw << 8) & 0xFFFFFFFF)
    d_hi = np.uint64((draw >> 24) & 0xFFFFFFFF)
    return ctr & M32, ((ctr >> s32) & M32) ^ d_lo, sample & M32, ((sample >> s32) & M32) ^ d_hi


def key(seed):
    seed = int(seed)
    return np.uint64(seed & 0xFFFFFFFF), np.uint64((seed >> 32) & 0xFFFFFFFF)


def uniform32(c):
    """A 32-bit word -> the float32 uniform in (0, 1]."""
    return (((c >> np.uint64(8)).astype(np.float32) + np.float32(0.5)) * np.float32(2.0 ** -24)).astype(np.float32)


def uniforms(seed, sample, draw, ctr):
    """The four float32 uniforms of (seed, sample, draw, ctr)."""
    return tuple(uniform32(c) for c in philox4x32_10(*counter(sample, draw, ctr), *key(seed)))


def normals(seed, sample, draw, elem4):
    """Float64 Box-Muller normals [..., 4] from the float32 uniforms of counter elem4."""
    u0, u1, u2, u3 = (u.astype(np.float64) for u in uniforms(seed, sample, draw, elem4))
    r0, r1 = np.sqrt(-2.0 * np.log(u0)), np.sqrt(-2.0 * np.log(u2))
    a0, a1 = 2.0 * np.pi * u1, 2.0 * np.pi * u3
    return np.stack([r0 * np.cos(a0), r0 * np.sin(a0), r1 * np.cos(a1), r1 * np.sin(a1)], axis=-1) + 0.0      # + 0.0: no negative zeros


def normals32(seed, sample, draw, elem4):
    """The same with every operation in numpy float32 (2 pi rounded to float32, the angle rounded, float32 log / sqrt / sin / cos)."""
    f = np.float32
    u0, u1, u2, u3 = uniforms(seed, sample, draw, elem4)
    r0, r1 = np.sqrt(f(-2.0) * np.log(u0)), np.sqrt(f(-2.0) * np.log(u2))
    a0, a1 = f(TWO_PI) * u1, f(TWO_PI) * u3
    out = np.stack([r0 * np.cos(a0), r0 * np.sin(a0), r1 * np.cos(a1), r1 * np.sin(a1)], axis=-1)
    assert out.dtype == np.float32
    return out


def gamma(k, seed, sample, draw, elem, flip=None):
    """Gamma(shape k, scale 1) variates in float64 from the float32 uniforms.

    d = kk - 1/3 with kk = k (k >= 1) or k + 1 (k < 1), c = 1 / sqrt(9 d).  Attempt j = 0..7 of element e reads the uniforms of counter
    8 e + j on the gamma stream: x = sqrt(-2 log u.x) cos(2 pi u.y), v = (1 + c x)^3, candidate g = d max(v, 1e-300), accepted when v > 0
    and log u.z < rhs = x^2 / 2 + d - d v + d log v.  An accepted candidate of k < 1 is multiplied by u.w^(1/k).  After 8 rejections the
    last candidate is kept as it is.  Only elements whose earlier attempts were all rejected are evaluated again.

    Returns (g, attempts, gap, jmin): attempts = the number of attempts evaluated; gap = the smallest |log u.z - rhs| over those attempts
    (inf where v <= 0) and jmin the attempt that has it -- the one decision of the element that a few ulps of fp64 libm could turn.
    flip: None, or per element an attempt index whose decision is inverted (-1: none): the value the element takes if that one
    decision falls the other way."""
    k = float(np.float32(k))
    sample, elem = np.broadcast_arrays(np.asarray(sample, dtype=np.uint64), np.asarray(elem, dtype=np.uint64))
    shape = elem.shape
    sample, elem = sample.ravel(), elem.ravel()
    n = elem.size
    flip = np.full(n, -1, dtype=np.int64) if flip is None else np.asarray(flip, dtype=np.int64).ravel()
    kk = k + 1.0 if k < 1.0 else k
    d = kk - 1.0 / 3.0
    c = 1.0 / np.sqrt(9.0 * d)
    g = np.full(n, d)
    attempts = np.zeros(n, dtype=np.int64)
    gap = np.full(n, np.inf)
    jmin = np.zeros(n, dtype=np.int64)
    live = np.arange(n)
    for j in range(MAX_ATTEMPTS):
        if live.size == 0:
            break
        ux, uy, uz, uw = (u.astype(np.float64) for u in uniforms(seed, sample[live], int(draw) | GAMMA_BIT, elem[live] * np.uint64(8) + np.uint64(j)))
        x = np.sqrt(-2.0 * np.log(ux)) * np.cos(TWO_PI * uy)
        t = 1.0 + c * x
        v = t * t * t
        cand = d * np.maximum(v, 1e-300)
        with np.errstate(invalid="ignore", divide="ignore"):
            rhs = 0.5 * x * x + d - d * v + d * np.log(v)
            lhs = np.log(uz)
            ok = (v > 0.0) & (lhs < rhs)
            gp = np.where(v > 0.0, np.abs(lhs - rhs), np.inf)
        ok = ok ^ (flip[live] == j)
        if k < 1.0:
            cand = np.where(ok, cand * np.power(uw, 1.0 / k), cand)
        g[live] = cand
        attempts[live] = j + 1
        better = gp < gap[live]
        jmin[live] = np.where(better, j, jmin[live])
        gap[live] = np.where(better, gp, gap[live])
        live = live[~ok]
    return g.reshape(shape), attempts.reshape(shape), gap.reshape(shape), jmin.reshape(shape)


# ---------------------------------------------------------------------------------------------- a [B, per] call as the kernels lay it out
def _rows(B, per, sample_offset):
    return (np.uint64(sample_offset) + np.arange(B, dtype=np.uint64))[:, None]


def randn_call(B, per, seed, sample_offset, draw, fn=normals):
    """What mcvd_randn(out:[B, per], seed, sample_offset, draw) holds: element e of the flat buffer has row = e / per and belongs to the
    float4 elem4 = (e - row per) >> 2 of sample sample_offset + row."""
    assert per % 4 == 0
    elem4 = np.arange(per // 4, dtype=np.uint64)[None, :]
    return fn(seed, _rows(B, per, sample_offset), draw, elem4).reshape(B, per)


def gamma_call(k, B, per, seed, sample_offset, draw, flip=None):
    """The Gamma(k, 1) variates behind mcvd_gamma_noise(raw = NULL, out:[B, per]): elem = e - row per of sample sample_offset + row.
    Returns gamma()'s four arrays, each [B, per]."""
    elem = np.arange(per, dtype=np.uint64)[None, :]
    return gamma(k, seed, _rows(B, per, sample_offset), draw, elem, flip=flip)
