"""TEST INFRASTRUCTURE ONLY -- numpy model of the one-hot x table contractions of csrc/vibo_cmean.hip and their a-priori bounds.

The kernels form  S[p, :] = sum_i [cell (p, i) observed] X[code_pi, i, :]  and the transpose  dX[c, i, :] = sum_p [code_pi == c] G[p, :]
on v_mfma_f32_16x16x32_bf16.  The one-hot operand is exact (entries 2.0); the dense operand goes in as THREE truncated bf16 pieces
hi + mid + lo of 0.5 x, accumulated in fp32, smallest piece first per K-step.  This file restates WHAT that scheme computes (no
lane layout, no LDS image) and derives, from the inputs alone, how far a result may lie from the exact sum.

The pieces (split3 = cm_split3).  bf16 keeps fp32's sign, exponent and the top 7 mantissa bits: 8 significant bits.  hi = the
top 8 bits of h = 0.5 x, mid = the top 8 bits of h - hi, lo = the top 8 bits of h - hi - mid: 24 bits, so  hi + mid + lo == 0.5 x
EXACTLY, and the pieces do not overlap (each is a multiple of its own ulp and below the ulp of the piece before it).  The two
subtractions are exact in fp32.  All three pieces are normal bf16 numbers when ulp(0.5 x) = 2^(E - 24) >= 2^-126, E the exponent
of x: |x| >= 2^-102 (ALL_NORMAL_MIN).  Below that a residual can be an fp32 subnormal: its top 16 bits are then a fixed 2^-133
grid instead of 8 significant bits, the piece is a bf16 subnormal, and the matrix pipe may flush it to zero.  The pieces are
truncations, so what is flushed of 0.5 x is below 2^-126 whichever piece it starts at (kept: below 2^-133), and what an output can
lose per observed term is below  FTZ_ABS = 2^-125  (the one-hot entry is 2.0).  (x itself subnormal: 0.5 x rounds, by at most 2^-150.)

Consequences the GPU tests assert (tests/test_gpu_onehot_contractions.py):
  * a sum over ONE observed cell is that cell's value bit for bit (0 + lo, + mid, + hi: every partial sum is a prefix of the bits
    of one fp32 number -- exact in any rounding mode; adding an exact zero never rounds);
  * values m 2^e with |m| < 2^20 and a common e (class `grid`): any sum of up to 16 of them, and every partial sum of their
    pieces, is an integer below 2^24 times 2^e -- exact as well;
  * everything else is held to sum_bound / grad_bound, with u = 2^-24:

        |S - exact| <= c u sum|terms| (1 + c u) + k FTZ_ABS           k = number of nonzero terms of the output

    c counts the fp32 additions on the output's path that can round.  It depends on k and on fixed tree depths, never on the
    number of items or persons: adding an exact zero does not round.
      C_MFMA = 2 roundings per MFMA accumulate and nonzero product in it.  One MFMA adds 32 products to the accumulator; m of
        them nonzero cost at most m - 1 additions among themselves and one into the accumulator, m + 1 <= 2 m roundings of at
        most u of the running sum each under round-to-nearest.  The matrix pipe's internal rounding mode is not documented for
        this part, hence 2 m and not m + 1.
      forward (cm_forward_kernel, cm_forward_fp32_kernel: `acc = mfma(a, b2, acc); ... b1 ...; ... b0 ...` per K-step):
        3 pieces x C_MFMA x k                                                                       c_forward(k)  = 6 k
      backward records (cm_backward_body: the same three MFMAs per 32-person K-chunk):             6 k
        + the record sums over the person ranges (cm_backward_reduce_kernel / cm_cond_finalize_body: `a[u] += q[...]`, at most
          one rounding per nonzero record, at most k of them; `((a0 + a1) + (a2 + a3)) + ((a4 + a5) + (a6 + a7))`: depth 3):
          k + 3                                                                                     c_backward(k) = 7 k + 3
        + cm_cond_finalize_body only: `v += part[sl * E + tid]` (one more slice at 16 record columns): 1, and the packed form's
          `(sp[k] + sp[pc + k]) + sp[2 * pc + k]`: 2                                             c_cond_backward(k) = 7 k + 6
        (the packed form runs ONE MFMA per K-chunk on three column groups instead of three on one: fewer roundings per group.)

model_sum / model_grad run the scheme in float32 numpy in the kernel's order (each MFMA: its 32 products and the accumulator added
exactly, rounded to fp32 once -- one plausible matrix pipe), with switches for the mutations the bound has to reject: drop the
third piece, drop the second, add a packed column group into the neighbouring column.  `nearest` rounds the pieces to nearest
instead of truncating; that split is exact as well (8 + 8 + 8 signed digits), so it stays inside the bound -- only the
non-overlap property tells the two apart.

Measured by tests/test_onehot_model.py (pytest -s prints them; I = 200, 400 persons, seed 11):
  intact model inside the bound on 100 % of the outputs of every class, forward and backward: worst error / bound 0.13 forward,
  0.05 / 0.07 backward (three MFMAs / packed); 0.10 with the pieces rounded to nearest; 0.97 with bf16 subnormals flushed (`tiny`:
  that loss is what the absolute term is for).
  model without `lo`, share of the outputs outside the bound:
    forward, per cells of the person           hostile  k = 2 / 3 / 8 / 16: 100 / 100 / 100 / 100 %    binades: 96 / 95 / 90 / 80 %
    backward, per observers 2..3 / 4..8 / 9..16  hostile: 100 / 100 / 100 %   binades: 93 / 89 / 84 %   (packed: 100 / 100 / 100, 97 / 90 / 82 %)
    packed form, lo group into the neighbouring column: hostile 100 %, binades 94 %; only two of the three groups added: 100 %, 88 %
  the worst output of the model without `lo` is at 42 x its bound.  Without `mid` more than 95 % of the outputs of EVERY class are
  outside (`tiny` included: mid is ~2^-119 there, the bound k 2^-125; the rest are values whose middle byte is zero).  `tiny` is not
  in the no-`lo` plan -- its lo pieces are the bf16 subnormals the absolute term already gives away (0 %) -- and neither is `grid`
  (87 ... 3 %: small integers often have no third piece), which is asserted EXACT on the GPU instead, so a lost piece shows there too.
"""
import numpy as np

U = 2.0 ** -24
FTZ_ABS = 2.0 ** -125           # per nonzero term: 2.0 x (what flushing bf16 subnormal pieces can lose of 0.5 x, < 2^-126)
ALL_NORMAL_MIN = 2.0 ** -102    # |x| from here on: hi, mid, lo all normal bf16 numbers (or zero)
C_MFMA = 2
KS = (2, 3, 8, 16)              # cells per person of the `few` pattern
CLASSES = ('hostile', 'binades', 'tiny', 'grid')
OBSERVER_BUCKETS = ((1, 1), (2, 3), (4, 8), (9, 16))      # observers of a (code, item) pair, as the backward's shares are reported
DROP_LO_PLAN = [(cls, k) for cls in ('hostile', 'binades') for k in KS]      # (class, k) on which a missing third piece must show


def _top8(v, nearest=False):
    """The bf16 number made of the top 8 significant bits of the float32 v (truncation), or the nearest bf16 (ties to even)."""
    b = np.ascontiguousarray(v, np.float32).view(np.uint32)
    if nearest:
        b = b + np.uint32(0x7fff) + ((b >> np.uint32(16)) & np.uint32(1))
    return (b & np.uint32(0xffff0000)).view(np.float32)


def split3(x, nearest=False):
    """cm_split3 on uint32 views, in float32: -> (hi, mid, lo) of 0.5 x."""
    h = np.float32(0.5) * np.asarray(x, np.float32)
    hi = _top8(h, nearest)
    r = h - hi
    mid = _top8(r, nearest)
    lo = _top8(r - mid, nearest)
    return hi, mid, lo


def flush_bf16_subnormals(p):
    """The piece as a matrix pipe that flushes bf16 subnormals would read it."""
    return np.where(np.abs(p) < np.float32(2.0 ** -126), np.float32(0), p)


def pieces(x, drop=None):
    """The three operand pieces in the order the kernels add them (lo, mid, hi), with the mutation `drop` applied."""
    hi, mid, lo = split3(x, nearest=drop == 'nearest')
    if drop == 'lo':
        lo = np.zeros_like(lo)
    if drop == 'mid':
        mid = np.zeros_like(mid)
    if drop == 'ftz':
        hi, mid, lo = (flush_bf16_subnormals(p) for p in (hi, mid, lo))
    return lo, mid, hi


# ---------------------------------------------------------------------------
# observer patterns and value classes
# ---------------------------------------------------------------------------
def make_pattern(kind, B, I, seed):
    """Cell codes uint8 [B, I] (0 wrong / 1 right / 2 missing).
    single:   B = 2 I; person perm[c I + i] observes item i with code c and nothing else (perm: a seeded permutation).
    few:      B = 2 I; the same first cell, then k - 1 more with k cycling through KS over the persons; the extra cells walk
              through the 16 (lane group, K-step) slots of a 64-item step in a seeded order, in random steps, and no
              (code, item) pair gets more than 16 observers.
    isolated: `single` on items 0 .. I - 2 for the first 2 (I - 1) persons; item I - 1 is observed by nobody and the last
              B - 2 (I - 1) persons observe nothing (B = 2 I + 1: three of them)."""
    rng = np.random.default_rng(seed)
    codes = np.full((B, I), 2, np.uint8)
    if kind == 'isolated':
        n = 2 * (I - 1)
        assert B > n
        codes[:n, :I - 1] = make_pattern('single', n, I - 1, seed)
        return codes
    assert B == 2 * I and kind in ('single', 'few')
    perm = rng.permutation(B)
    pair_c, pair_i = np.arange(B) // I, np.arange(B) % I
    codes[perm, pair_i] = pair_c
    if kind == 'single':
        return codes
    count = np.ones((2, I), np.int64)
    nS = (I + 63) // 64
    for q in range(B):
        p, k = perm[q], KS[q % len(KS)]
        slots = rng.permutation(16)
        have, m, tries = 1, 0, 0
        while have < k:
            g, j = divmod(int(slots[m % 16]), 4)
            item = 64 * int(rng.integers(nS)) + 16 * g + 4 * j + int(rng.integers(4))
            c = int(rng.integers(2))
            tries += 1
            if tries > 64:                   # (the slot has no free cell left: move on to the next one)
                m, tries = m + 1, 0
                continue
            if item >= I or codes[p, item] != 2 or count[c, item] >= 16:
                continue
            codes[p, item] = c
            count[c, item] += 1
            have, m, tries = have + 1, m + 1, 0
    return codes


def _hostile_mantissas(rng, n):
    """23-bit mantissa fields: half with the low byte 0xFF under random upper bits, a quarter all ones, a quarter alternating."""
    kind = rng.integers(0, 8, n)
    m = (rng.integers(0, 1 << 15, n) << 8) | 0xFF
    m = np.where(kind >= 6, 0x7FFFFF, m)
    m = np.where(kind == 4, 0x555555, m)
    m = np.where(kind == 5, 0x2AAAAA, m)
    return m.astype(np.uint32)


def _assemble(sign, exponent, mantissa):
    return ((sign.astype(np.uint32) << np.uint32(31)) | ((exponent + 127).astype(np.uint32) << np.uint32(23)) | mantissa).view(np.float32)


def make_values(cls, shape, seed):
    """float32 operand values of `shape` (last axis = the output column).
    hostile: mantissas as above (all 24 bits kept by the pieces, or lost), exponents -2 .. 2, the sign alternating with the
             column so that one output's terms share it and both signs occur;
    binades: 2^-100 .. 2^100 drawn per value -- mixed inside every 64-item step --, low mantissa byte 0xFF, random signs;
    tiny:    |x| in [2^-110, 2^-109), low mantissa byte 0xFF, random signs;
    grid:    m 2^e, |m| < 2^20 odd, e = e(column) in -20 .. 20."""
    rng = np.random.default_rng(seed)
    n = int(np.prod(shape))
    col = np.broadcast_to(np.arange(shape[-1]), shape).reshape(-1)
    if cls == 'hostile':
        v = _assemble(col & 1, rng.integers(-2, 3, n), _hostile_mantissas(rng, n))
    elif cls == 'binades':
        v = _assemble(rng.integers(0, 2, n), rng.integers(-100, 101, n), ((rng.integers(0, 1 << 15, n) << 8) | 0xFF).astype(np.uint32))
    elif cls == 'tiny':
        v = _assemble(rng.integers(0, 2, n), np.full(n, -110), ((rng.integers(0, 1 << 15, n) << 8) | 0xFF).astype(np.uint32))
    elif cls == 'grid':
        m = (rng.integers(-(1 << 19), 1 << 19, n) * 2 + 1).astype(np.float64)
        v = (m * 2.0 ** ((col * 7) % 41 - 20)).astype(np.float32)
    else:
        raise ValueError(cls)
    return v.reshape(shape)


# ---------------------------------------------------------------------------
# exact sums and bounds (float64: a sum of a few fp32 values is exact in it unless they lie far apart -- `binades` spans 200 binades --
# and then it is off by at most 2^-53 of the largest term, 2^-29 u of the bound)
# ---------------------------------------------------------------------------
def onehots(codes):
    """-> float64 [2, B, I] indicators of code 0 and code 1."""
    return np.stack([(codes == 0), (codes == 1)]).astype(np.float64)


def exact_sum(codes, X):
    """-> (S [B, N], sum|terms| [B, N], k [B]) in float64: S[p] = sum_i [observed] X[code_pi, i]."""
    oh = onehots(codes)
    X = X.astype(np.float64)
    S = oh[0] @ X[0] + oh[1] @ X[1]
    T = oh[0] @ np.abs(X[0]) + oh[1] @ np.abs(X[1])
    return S, T, (codes != 2).sum(1)


def exact_grad(codes, G):
    """-> (dX [2, I, N], sum|terms| [2, I, N], k [2, I]) in float64: dX[c, i] = sum_p [code_pi == c] G[p]."""
    oh = onehots(codes)
    G = G.astype(np.float64)
    D = np.stack([oh[0].T @ G, oh[1].T @ G])
    T = np.stack([oh[0].T @ np.abs(G), oh[1].T @ np.abs(G)])
    return D, T, oh.sum(1).astype(np.int64)


def c_forward(k):
    return 3 * C_MFMA * k                      # `acc = cm_mfma(a, b2, acc)`, `... b1 ...`, `... b0 ...`: 3 MFMAs x 2 per nonzero product


def c_backward(k):
    return 3 * C_MFMA * k + k + 3              # + `a[u] += rp[...]` (<= k nonzero records) + the depth-3 tree of the eight sums


def c_cond_backward(k):
    return c_backward(k) + 1 + 2               # + `v += part[sl * E + tid]` + `(sp[k] + sp[pc + k]) + sp[2 * pc + k]`


def _bound(c, T, k):
    c = np.asarray(c, np.float64)
    return c * U * T * (1.0 + c * U) + k * FTZ_ABS


def sum_bound(T, k):
    """Bound of the forward sums: T = sum|terms| [B, N], k = observed cells [B]."""
    k = np.asarray(k, np.float64)[:, None]
    return _bound(c_forward(k), T, k)


def grad_bound(T, k, cond=False):
    """Bound of the transposed sums: T = sum|terms| [2, I, N], k = observers [2, I].  cond: through cm_cond_finalize_body."""
    k = np.asarray(k, np.float64)[..., None]
    return _bound(c_cond_backward(k) if cond else c_backward(k), T, k)


# ---------------------------------------------------------------------------
# the scheme in float32, in the kernels' order
# ---------------------------------------------------------------------------
def _mfma(acc, prod_sum):
    """One accumulate: the sum of the products plus the accumulator in float64 (a few 8-bit pieces: exact unless they lie more
    than 2^29 apart, where the smaller one is below 2^-29 u of the bound), rounded to fp32 once."""
    return (acc.astype(np.float64) + prod_sum).astype(np.float32)


def model_sum(codes, X, drop=None):
    """The forward in float32: per 64-item step, K-step j = 0 .. 3 covers the items 64 S + 16 g + 4 j + t (g, t = 0 .. 3); per
    K-step the lo, mid and hi pieces are accumulated in that order.  -> S float32 [B, N]."""
    B, I = codes.shape
    N = X.shape[2]
    P = pieces(X, drop)
    acc = np.zeros((B, N), np.float32)
    for S in range((I + 63) // 64):
        for j in range(4):
            items = np.array([64 * S + 16 * g + 4 * j + t for g in range(4) for t in range(4)])
            items = items[items < I]
            if items.size == 0:
                continue
            cc = codes[:, items]
            if not (cc != 2).any():
                continue
            o0, o1 = 2.0 * (cc == 0), 2.0 * (cc == 1)
            for pc in P:
                acc = _mfma(acc, o0 @ pc[0, items].astype(np.float64) + o1 @ pc[1, items].astype(np.float64))
    return acc


def person_ranges(B, nS):
    """cm_ranges: -> (number of person ranges, persons per range) of the backward's records."""
    nR = max(8, (2048 // max(nS, 1) + 7) // 8 * 8)
    per = max(64, (-(-B // nR) + 63) // 64 * 64)
    return -(-B // per), per


def _reduce_records(rec, nsl=1):
    """The fixed-order sum over the person ranges: rec float32 [nR, ...] -> float32 [...] (cm_backward_reduce_kernel; nsl = 2:
    cm_cond_finalize_body at 16 record columns, two interleaved slices added at the end)."""
    nR = rec.shape[0]
    parts = []
    for sl in range(nsl):
        a = [np.zeros(rec.shape[1:], np.float32) for _ in range(8)]
        r = sl
        while r + 7 * nsl < nR:
            for u in range(8):
                a[u] = a[u] + rec[r + u * nsl]
            r += 8 * nsl
        while r < nR:
            a[0] = a[0] + rec[r]
            r += nsl
        parts.append(((a[0] + a[1]) + (a[2] + a[3])) + ((a[4] + a[5]) + (a[6] + a[7])))
    v = parts[0]
    for p in parts[1:]:
        v = v + p
    return v


def model_grad(codes, G, drop=None, packed=False, nsl=1):
    """The backward in float32: records per person range (64-person steps of two 32-person K-chunks, lo, mid, hi per chunk), then
    the fixed-order sum over the ranges.  packed (cm_backward_body's PK, at most 5 columns): the three pieces sit in three column
    groups of one operand -- one MFMA per chunk --, the groups are summed over the ranges separately and added as (hi + mid) + lo;
    drop = 'neighbour' adds the lo group into the next column.  -> dX float32 [2, I, N]."""
    B, I = codes.shape
    N = G.shape[1]
    lo, mid, hi = pieces(G, drop)
    nR, per = person_ranges(B, (I + 63) // 64)
    oh = 2.0 * onehots(codes)                                   # [2, B, I]
    groups = [[hi], [mid], [lo]] if packed else [[lo, mid, hi]]
    sums = []
    for grp in groups:
        rec = np.zeros((nR, 2, I, N), np.float32)
        for r in range(nR):
            for p0 in range(r * per, min(B, (r + 1) * per), 32):
                sl = slice(p0, min(B, p0 + 32))
                if not oh[:, sl].any():
                    continue
                for pc in grp:
                    rec[r] = _mfma(rec[r], np.einsum('cpi,pn->cin', oh[:, sl], pc[sl].astype(np.float64)))
        sums.append(_reduce_records(rec, nsl))
    if not packed:
        return sums[0]
    s_hi, s_mid, s_lo = sums
    if drop == 'neighbour':
        s_lo = np.roll(s_lo, 1, axis=-1)
    if drop == 'two-groups':
        return s_hi + s_mid
    return (s_hi + s_mid) + s_lo
