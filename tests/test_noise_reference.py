"""oracle/philox_ref.py, the host reference of the native noise generator (no GPU): Random123's published known answers for
philox4x32-10, and the statistical properties that justify the counter layout (group, step, stream) x key (seed) -- every stream
standard normal and serially uncorrelated on its own, streams that differ in one counter or key word uncorrelated with each other,
the four outputs of one counter two independent Box-Muller pairs.  tests/test_gpu_noise.py holds the kernels to this reference."""
import functools

import numpy as np
import pytest
import torch

from oracle import philox_ref as P

N = 1 << 20
BEEF = (0xDEADBEEF << 32) | 5
MAX64 = (1 << 64) - 1
# The caps.  Kolmogorov-Smirnov: sqrt(n) D_n < 1.95 (the limiting distribution puts 1e-3 above 1.95).  Moments and products: 4
# standard errors (6.3e-5 two-sided per figure; 12 streams x 5 figures + 4 pairs + 2 lanes below).
KS_CAP, SE_CAP = 1.95, 4.0
P_TAIL = 0.0026997960632601866          # P(|z| > 3)


@functools.lru_cache(maxsize=None)
def stream(seed, step, stream_id):
    z, r, u = P.normals(N, seed, step, stream_id)
    for a in (z, r, u):
        a.setflags(write=False)
    return z, r, u


def hexwords(ws):
    return ' '.join('%08x' % int(w) for w in ws)


@pytest.mark.parametrize('counter,key,want', [
    ((0, 0, 0, 0), (0, 0), '6627e8d5 e169c58d bc57ac4c 9b00dbd8'),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, '408f276d 41c83b0e a20bc7c6 6d5451fd'),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), 'd16cfe09 94fdcceb 5001e420 24126ea1')])
def test_known_answers_of_random123(counter, key, want):
    """The three philox4x32-10 vectors Random123 publishes (kat_vectors): zeros, ones, digits of pi."""
    assert hexwords(P.philox4x32_10(counter, key)) == want
    # as arrays, broadcast: the same words in every lane
    got = P.philox4x32_10(tuple(np.full(5, c, dtype=np.uint64) for c in counter), key)
    assert all(hexwords([w[i] for w in got]) == want for i in range(5))


def test_layout_of_a_stream():
    """normals(): entry i comes from group i // 4 with the counter (g lo, g hi, step, stream) and the key (seed lo, seed hi); a
    shorter stream is a prefix of a longer one; r and u are the entry's radius and radius uniform."""
    seed, step, sid = BEEF, 3, 9
    z, r, u = P.normals(11, seed, step, sid)
    assert z.shape == r.shape == u.shape == (11,) and z.dtype == np.float64
    for g in range(3):
        c = [int(w) for w in P.philox4x32_10((g, 0, step, sid), (5, 0xDEADBEEF))]
        u0, u1, u2, u3 = ((c[0] >> 8) + 1) / 2 ** 24, (c[1] >> 8) / 2 ** 24, ((c[2] >> 8) + 1) / 2 ** 24, (c[3] >> 8) / 2 ** 24
        r0, r1 = np.sqrt(-2 * np.log(u0)), np.sqrt(-2 * np.log(u2))
        want = [r0 * np.cos(2 * np.pi * u1), r0 * np.sin(2 * np.pi * u1), r1 * np.cos(2 * np.pi * u3), r1 * np.sin(2 * np.pi * u3)]
        k = min(4, 11 - 4 * g)
        assert np.array_equal(z[4 * g:4 * g + k], np.array(want[:k]))
        assert np.array_equal(r[4 * g:4 * g + k], np.array([r0, r0, r1, r1][:k]))
        assert np.array_equal(u[4 * g:4 * g + k], np.array([u0, u0, u2, u2][:k]))
    assert np.array_equal(P.normals(5, seed, step, sid)[0], z[:5])
    # the group's high word is counter word 1: group 2^32 + 1 is not group 1
    lo = P.words(np.array([1], dtype=np.uint64), seed, step, sid)
    hi = P.words(np.array([(1 << 32) + 1], dtype=np.uint64), seed, step, sid)
    assert hexwords(w[0] for w in hi) == hexwords(P.philox4x32_10((1, 1, step, sid), (5, 0xDEADBEEF)))
    assert hexwords(w[0] for w in hi) != hexwords(w[0] for w in lo)
    # step is taken as the kernel takes it: the int32 counter's bits as uint32
    assert np.array_equal(P.normals(8, seed, -1, sid)[0], P.normals(8, seed, 0xFFFFFFFF, sid)[0])


def standard_errors(z):
    """|figure - expectation| / its standard error under N(0,1), independent entries: mean, variance, lag-1 and lag-4 product means,
    share of |z| > 3."""
    n = z.size
    return {'mean': abs(z.mean()) * np.sqrt(n),
            'variance': abs(z.var() - 1.0) / np.sqrt(2.0 / n),
            'lag 1': abs((z[:-1] * z[1:]).mean()) * np.sqrt(n - 1),
            'lag 4': abs((z[:-4] * z[4:]).mean()) * np.sqrt(n - 4),
            'tail': abs((np.abs(z) > 3.0).mean() - P_TAIL) / np.sqrt(P_TAIL * (1 - P_TAIL) / n)}


def ks_scaled(z):
    """sqrt(n) x the Kolmogorov-Smirnov distance of the sample to the standard normal distribution function."""
    n = z.size
    cdf = torch.special.ndtr(torch.from_numpy(np.sort(z))).numpy()
    i = np.arange(1, n + 1, dtype=np.float64)
    return np.sqrt(n) * max((i / n - cdf).max(), (cdf - (i - 1) / n).max())


# a dozen of the 6 x 4 x 4 combinations: every seed (small, both key words non-zero and distinct, all ones), step and stream appears
WITHIN = [(0, 0, 0), (7, 0, 0), (7, 1, 1), (3, 2, 2), (11, (1 << 31) - 1, (1 << 32) - 1), (BEEF, 0, 1), (BEEF, 1, (1 << 32) - 1),
          (BEEF, (1 << 31) - 1, 0), (MAX64, 0, 2), (MAX64, 2, 0), (MAX64, (1 << 31) - 1, 1), (0, 1, (1 << 32) - 1)]


@pytest.mark.parametrize('seed,step,stream_id', WITHIN)
def test_one_stream_is_standard_normal_and_serially_uncorrelated(seed, step, stream_id):
    z, r, u = stream(seed, step, stream_id)
    assert np.isfinite(z).all()
    ks = ks_scaled(z)
    se = standard_errors(z)
    print('KS sqrt(n) D', round(float(ks), 3), {k: round(float(v), 3) for k, v in se.items()})
    assert ks < KS_CAP
    for k, v in se.items():
        assert v < SE_CAP, (k, v)


@pytest.mark.parametrize('other', [(7, 0, 1), (7, 1, 0), (8, 0, 0), (7 | 1 << 32, 0, 0)], ids=['stream', 'step', 'seed lo', 'seed hi'])
def test_streams_that_differ_in_one_word_are_unrelated(other):
    """(seed 7, step 0, stream 0) against the stream one counter word (stream, step) or one key word (seed lo, seed hi) away:
    uncorrelated entry by entry, and no entry in common."""
    z, zo = stream(7, 0, 0)[0], stream(*other)[0]
    corr = abs((z * zo).mean()) * np.sqrt(N)
    print('|mean(z z\')| sqrt(n)', round(float(corr), 3))
    assert corr < SE_CAP
    assert not (z == zo).any()


def test_the_four_outputs_of_one_counter_are_two_independent_pairs():
    """z0^2 + z1^2 = r0^2 and z2^2 + z3^2 = r1^2 to float64 rounding -- cos and sin of the same rounded angle, each within an ulp,
    one rounding each for r c, its square, the sum and r^2: under 6 x 2^-52 relative --, and the two pairs share nothing:
    (z0, z2) and (z1, z3) are uncorrelated."""
    z, r, u = stream(7, 0, 0)
    q = z.reshape(-1, 4)
    rr = r.reshape(-1, 4)
    assert np.array_equal(rr[:, 0], rr[:, 1]) and np.array_equal(rr[:, 2], rr[:, 3])
    assert np.array_equal(rr, np.sqrt(-2.0 * np.log(u.reshape(-1, 4))))
    for a, b in ((0, 1), (2, 3)):
        r2 = rr[:, a] ** 2
        assert (np.abs(q[:, a] ** 2 + q[:, b] ** 2 - r2) <= 6 * 2.0 ** -52 * r2).all()
    for a, b in ((0, 2), (1, 3)):
        corr = abs((q[:, a] * q[:, b]).mean()) * np.sqrt(N // 4)
        print('lanes', a, b, round(float(corr), 3))
        assert corr < SE_CAP


def test_resolution_is_the_move_of_one_uniform_step():
    """q bounds what one step of 2^-24 in either uniform does to an entry (first order), and is inf exactly where r = 0."""
    z, r, u = stream(7, 0, 0)
    q = P.resolution(r, u)
    assert np.isinf(q[r == 0]).all() and np.isfinite(q[r > 0]).all()
    keep = u < 1 - 2.0 ** -10          # (|dr / du| = 1 / (u r) falls with u below exp(-1/2); above, away from u = 1, 1 % covers the curvature)
    du = 2.0 ** -24
    r_up = np.sqrt(-2.0 * np.log(u + du))
    assert (np.abs(r_up - r)[keep] <= 1.01 * (du / (u * r))[keep]).all()
    assert (2 * np.pi * r * du <= q).all()
