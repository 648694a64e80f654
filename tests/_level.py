"""numpy restatement of the output level stage, written from the definition and independent of cv2amd/level.py and of
the kernel.  Everything up to the window maximum is float32 arithmetic, which numpy does exactly as the device does (one correctly rounded
operation each), so x, r, d and D are bit-exact against the kernel; the weighted sum is float64 over the float32 weights:

    x[n] = fl(Ge s[n]);  a[n] = |x[n]|, NaN counts as 0;  r[n] = a[n] > c ? fl(c / a[n]) : 1;  d[n] = a[n] > c ? fl(1 - r[n]) : 0
    D[n] = max d[k], k = n .. min(n + L, N - 1)
    acc[n] = sum over j = 0 .. L with n - j >= 0 of w[j] D[n - j],   w[j] = h_j / sum h, h_j = 0.5 - 0.5 cos(2 pi (j + 0.5) / (L + 1))
    g[n] = max(0, min(1 - acc[n], r[n]));  y[n] = clamp(g[n] x[n], -c, c);  a NaN x[n] gives +0, an infinite one +-c

in a one-shot form (the whole signal) and a chunked form (the stream: before the final chunk sample n goes out as soon as
n + L <= n_available - 1; each chunk is computed from the retained samples and the new ones alone).
"""
import numpy as np

F = np.float32
LOOKAHEADS = (24, 120, 240)
U = 2.0 ** -24                                                     # one float32 rounding, relative
_w = {}


def lengths(L):
    return (1, L, L + 1, 1023, 1024, 1025, 2 * 1024 + L + 3)


def weights(L):
    """-> (w float64 [L + 1], the same rounded once to float32)"""
    if L not in _w:
        h = 0.5 - 0.5 * np.cos(2.0 * np.pi * (np.arange(L + 1, dtype=np.float64) + 0.5) / (L + 1))
        w = h / h.sum()
        _w[L] = (w, w.astype(F))
    return _w[L]


def db(v):
    """float32(10 ** (v / 20)), computed in float64 and rounded once"""
    return F(10.0 ** (v / 20.0))


def gain(G, P=None, T=None):
    """Ge: G, or with a peak target fl(G * fl(T / P)) when P > 0"""
    if T is None or not P > 0:
        return F(G)
    return F(F(G) * F(F(T) / F(P)))


def peak(s):
    """P = max |s|, NaN counting as 0"""
    a = np.abs(np.asarray(s, dtype=F))
    return F(np.where(np.isnan(a), F(0), a).max()) if a.size else F(0)


def parts(s, Ge, c):
    """-> (x, a, r, d) in float32"""
    with np.errstate(invalid='ignore', divide='ignore', over='ignore'):
        s, Ge, c = np.asarray(s, dtype=F), F(Ge), F(c)
        x = (Ge * s).astype(F)
        a = np.abs(x)
        a = np.where(np.isnan(a), F(0), a).astype(F)
        over = a > c
        r = np.ones_like(x)
        r[over] = (c / a[over]).astype(F)
        d = np.zeros_like(x)
        d[over] = (F(1) - r[over]).astype(F)
    return x, a, r, d


def _outputs(have, first, n_lim, n_lo, n_hi, Ge, c, L):
    """the samples n_lo .. n_hi - 1; `have` holds the source samples first .. first + len(have) - 1, windows end at n_lim - 1"""
    w64, w32 = weights(L)
    x, a, r, d = parts(have, Ge, c)
    m_lo = max(0, n_lo - L)                                        # D[m] is needed for m = m_lo .. n_hi - 1
    assert n_hi <= n_lo or (m_lo >= first and min(n_hi - 1 + L, n_lim - 1) < first + len(have)), 'an output reads a sample that is not there'
    D = np.zeros(max(0, n_hi - m_lo), dtype=F)
    for m in range(m_lo, n_hi):
        D[m - m_lo] = d[m - first:min(m + L, n_lim - 1) - first + 1].max()
    acc = np.zeros(max(0, n_hi - n_lo), dtype=np.float64)
    for j in range(L + 1):                                         # ascending j, as the device sums (the order is immaterial in float64 at these bounds)
        lo = max(n_lo, j)                                        # n - j >= 0
        if lo < n_hi:
            acc[lo - n_lo:] += np.float64(w32[j]) * D[lo - j - m_lo:n_hi - j - m_lo].astype(np.float64)
    xs, rs = x[n_lo - first:n_hi - first], r[n_lo - first:n_hi - first]
    g = np.maximum(0.0, np.minimum(1.0 - acc, rs.astype(np.float64)))
    with np.errstate(invalid='ignore', over='ignore'):
        y = np.clip(g * xs.astype(np.float64), -np.float64(F(c)), np.float64(F(c)))
    y = np.where(np.isnan(xs), 0.0, y)
    y = np.where(np.isinf(xs), np.copysign(np.float64(F(c)), xs), y)
    return dict(x=xs, r=rs, acc=acc, g=g, y=y)


def level64(s, Ge, c, L):
    """the whole signal at once -> dict(x fp32, r fp32, acc, g, y float64)"""
    return _outputs(np.asarray(s, dtype=F), 0, len(s), 0, len(s), Ge, c, L)


def stream64(s, Ge, c, L, chunks):
    """the stream: -> (y64, per chunk (n0, n_emit, first, n_avail, retained afterwards)); every chunk sees only what the call retained"""
    assert sum(chunks) == len(s)
    s = np.asarray(s, dtype=F)
    tail, first, seen, n0, ys, log = np.zeros(0, dtype=F), 0, 0, 0, [], []
    for k, n_new in enumerate(chunks):
        final = k == len(chunks) - 1
        have = np.concatenate([tail, s[seen:seen + n_new]])
        seen += n_new
        n1 = seen if final else max(n0, seen - L)                  # n + L <= seen - 1
        ys.append(_outputs(have, first, seen, n0, n1, Ge, c, L)['y'])
        keep = seen if final else max(0, n1 - L)
        log.append((n0, n1 - n0, first, seen, seen - keep))
        tail, first, n0 = have[keep - first:], keep, n1
    return np.concatenate(ys) if ys else np.zeros(0), log


def quiet(s, Ge, c, L):
    """samples with no sample over the ceiling within +-L: there acc == 0, g == 1 and y == x bit for bit"""
    a = parts(s, Ge, c)[1]
    q = np.ones(len(a), dtype=bool)
    for n in np.nonzero(a > F(c))[0]:
        q[max(0, n - L):n + L + 1] = False
    return q


# ---- the signals of the tests ----------------------------------------------------------------------------------------------------------
def sine(n, amp=0.3):
    return (amp * np.sin(2.0 * np.pi * 220.0 * np.arange(n) / 24000.0)).astype(F)


def bursts(n):
    """a sine with a 5x burst over its middle fifth and isolated overs at sample 0, at n - 1 and at the tile edges 1023 / 1024"""
    s = sine(n)
    s[2 * n // 5:3 * n // 5] *= F(5)
    for q, v in ((0, 2.0), (n - 1, -2.0), (1023, 3.0), (1024, -1.5)):
        if 0 <= q < n:
            s[q] = F(v)
    return s


def specials(n):
    """NaN and +-Inf samples (and -0) in a sine with an over"""
    s = sine(n)
    for q, v in ((3, np.nan), (n // 3, np.inf), (n // 2, -np.inf), (n // 2 + 7, np.nan), (5, -0.0), (2 * n // 3, 1.7), (n - 2, np.nan)):
        if 0 <= q < n:
            s[q] = F(v)
    return s


def pow2(n, seed=0):
    """magnitudes that are powers of two, 2^-6 .. 2^2, random signs: with c = 0.5 and Ge = 1 every r and d is exact and y / x IS g"""
    rng = np.random.default_rng(seed)
    e = rng.integers(-6, 0, n)
    e[rng.random(n) < 0.02] = 2
    e[rng.random(n) < 0.02] = 0
    return (np.ldexp(1.0, e) * rng.choice([-1.0, 1.0], n)).astype(F)


def ragged(n, pattern=(1, 7, 239, 480, 3, 1024, 25)):
    out, left, k = [], n, 0
    while left:
        c = min(left, pattern[k % len(pattern)])
        out.append(c)
        left -= c
        k += 1
    return out


def chunkings(n, L):
    """whole, 480-sample chunks, ragged (1, 7, 239, ...), chunks shorter than L (with an empty one among them)"""
    short = max(1, L - 7)
    return {'whole': [n], '480-sample chunks': [480] * (n // 480) + ([n % 480] if n % 480 else []), 'ragged': ragged(n),
            'shorter than L': ([0] if n > 1 else []) + [short] * (n // short) + ([n % short] if n % short else [])}
