"""TEST INFRASTRUCTURE ONLY -- host reference of the native noise generator (csrc/vibo_philox.hpp, vibo_fill_normal).

Philox4x32-10 written from the published algorithm (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3",
SC'11) in numpy on uint64 arrays, then the layout include/vibo_hip.h documents for vibo_fill_normal and Box-Muller in float64.
No GPU and no torch generator: tests/test_noise_reference.py pins it to Random123's published known answers and to the
statistical properties the counter layout has to have, tests/test_gpu_noise.py compares the kernels with it entry by entry.

    round:    hi0:lo0 = M0 * c0,  hi1:lo1 = M1 * c2   (32 x 32 -> 64 bit)
              (c0, c1, c2, c3) <- (hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0)
    key:      (k0, k1) <- (k0 + W0, k1 + W1) mod 2^32 after every round (the Weyl sequence); ten rounds
    counter:  entry i of a stream belongs to group g = i // 4: (g & 0xffffffff, g >> 32, uint32(step), stream_id)
    key:      (seed & 0xffffffff, seed >> 32)
    uniforms: u0 = ((c0 >> 8) + 1) / 2^24 and u2 = ((c2 >> 8) + 1) / 2^24 in (0, 1] (the radii),
              u1 = (c1 >> 8) / 2^24 and u3 = (c3 >> 8) / 2^24 in [0, 1) (the angles, in revolutions)
    normals:  r0 cos 2 pi u1, r0 sin 2 pi u1, r1 cos 2 pi u3, r1 sin 2 pi u3 with r0 = sqrt(-2 ln u0), r1 = sqrt(-2 ln u2)
"""
import numpy as np

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)        # the two round multipliers
W0, W1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)        # the key's Weyl increments (golden ratio, sqrt(3) - 1)
MASK32 = np.uint64(0xFFFFFFFF)
SHIFT32 = np.uint64(32)
ROUNDS = 10
TWO_M24 = 2.0 ** -24


def philox4x32_10(counter, key, rounds=ROUNDS):
    """counter: four and key: two uint64 arrays (or scalars) holding 32-bit words, broadcast against each other
    -> the four output words as uint64 arrays.  A 32 x 32 bit product fits uint64, so no arithmetic here wraps."""
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) & MASK32 for c in counter)
    k0, k1 = (np.asarray(k, dtype=np.uint64) & MASK32 for k in key)
    for _ in range(rounds):
        p0, p1 = M0 * c0, M1 * c2
        c0, c1, c2, c3 = (p1 >> SHIFT32) ^ c1 ^ k0, p1 & MASK32, (p0 >> SHIFT32) ^ c3 ^ k1, p0 & MASK32
        k0, k1 = (k0 + W0) & MASK32, (k1 + W1) & MASK32
    return c0, c1, c2, c3


def words(groups, seed, step, stream_id):
    """The four output words of the counter groups `groups` (uint64 array) of stream `stream_id` of `seed` at `step`."""
    g = np.asarray(groups, dtype=np.uint64)
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    counter = (g & MASK32, g >> SHIFT32, np.uint64(int(step) & 0xFFFFFFFF), np.uint64(int(stream_id) & 0xFFFFFFFF))
    return philox4x32_10(counter, (np.uint64(seed & 0xFFFFFFFF), np.uint64(seed >> 32)))


def normals(n, seed, step, stream_id):
    """-> (z, r, u): float64 arrays [n]; z[i] is entry i of vibo_fill_normal(out, n, seed, &step, stream_id), r[i] the radius
    and u[i] the radius uniform of that entry (entries 4g and 4g + 1 share r0 / u0, entries 4g + 2 and 4g + 3 share r1 / u2)."""
    n = int(n)
    groups = (n + 3) // 4
    c0, c1, c2, c3 = words(np.arange(groups, dtype=np.uint64), seed, step, stream_id)
    eight = np.uint64(8)
    u_r = np.stack([((c0 >> eight).astype(np.float64) + 1.0) * TWO_M24, ((c2 >> eight).astype(np.float64) + 1.0) * TWO_M24], axis=1)
    u_a = np.stack([(c1 >> eight).astype(np.float64) * TWO_M24, (c3 >> eight).astype(np.float64) * TWO_M24], axis=1)
    rad = np.sqrt(-2.0 * np.log(u_r))                         # [groups, 2]
    ang = 2.0 * np.pi * u_a
    z = np.stack([rad * np.cos(ang), rad * np.sin(ang)], axis=2)      # [groups, pair, (cos, sin)]
    r = np.repeat(rad, 2, axis=1)
    u = np.repeat(u_r, 2, axis=1)
    return z.reshape(-1)[:n], r.reshape(-1)[:n], u.reshape(-1)[:n]


def resolution(r, u):
    """q = 2 pi r 2^-24 + 2^-24 / (u r): how far an entry moves when its angle or its radius uniform moves by one step of 2^-24
    (|dz / du_angle| <= 2 pi r, |dz / du_radius| <= 1 / (u r)) -- the generator's own resolution, the unit the kernels' float32
    transform is held to.  r = 0 (u = 1) gives inf: such an entry has to be an exact zero and is checked for that instead."""
    with np.errstate(divide='ignore'):
        return 2.0 * np.pi * r * TWO_M24 + TWO_M24 / (u * r)
