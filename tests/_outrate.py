"""fp64 numpy restatement of the output resampling, written from the definition and independent of
cv2amd/outrate.py and of the kernel, over the fp32 table K, width = cv2amd.prompt._sinc_kernel(24000, R):

    g = gcd(24000, R), down = 24000 / g, up = R / g;   o = i up + p, 0 <= p < up;   q = i down - width + j
    y[o] = sum over j = 0 .. klen - 1 with 0 <= q < N of K[p][j] s[q]            for o < ceil(N up / down)

in a one-shot form (the whole signal) and a chunked form (the stream: before the final chunk o goes out as soon as
i down - width + klen - 1 <= n_available - 1; each chunk is computed from the retained samples and the new ones alone), and the
int16 rule trunc_toward_zero(y * 32768) saturated to [-32768, 32767], NaN -> 0.
"""
import math

import numpy as np

RATES = (8000, 16000, 22050, 24000, 32000, 44100, 48000)
SHAPES = {8000: (41, 1), 16000: (23, 2), 22050: (174, 147), 32000: (17, 4), 44100: (94, 147), 48000: (15, 2)}     # R -> (klen, phase rows)
LENGTHS = (1, 2, 19, 41, 42, 255, 256, 257, 1000, 4803)
_tab = {}


def table(rate):
    """-> (K fp32 [up][klen] or None at 24000, up, down, klen, width)"""
    if rate not in _tab:
        if rate == 24000:
            _tab[rate] = (None, 1, 1, 1, 0)
        else:
            from cv2amd.prompt import _sinc_kernel
            k, width, down, up = _sinc_kernel(24000, rate)
            g = math.gcd(24000, rate)
            assert k.dtype == np.float32 and (down, up) == (24000 // g, rate // g) and k.shape == (up, 2 * width + down)
            _tab[rate] = (k, up, down, k.shape[1], width)
    return _tab[rate]


def n_out(n, rate):
    _, up, down, _, _ = table(rate)
    return (n * up + down - 1) // down


def _outputs(s, first, n_lim, o_lo, o_hi, rate):
    """y64 and sum |K s| of the outputs o_lo .. o_hi - 1; s holds the samples first .. first + len(s) - 1, taps are those in [0, n_lim)"""
    k, up, down, klen, width = table(rate)
    y, mag = np.zeros(o_hi - o_lo), np.zeros(o_hi - o_lo)
    s = np.asarray(s, dtype=np.float64)
    for o in range(o_lo, o_hi):
        i, p = divmod(o, up)
        base = i * down - width
        j = np.arange(max(0, -base), min(klen, n_lim - base))
        q = base + j
        assert j.size == 0 or (q[0] >= first and q[-1] < first + len(s)), 'the output reads a sample that is not there'
        x = s[q - first]
        if k is None:
            y[o - o_lo], mag[o - o_lo] = x[0], abs(x[0])
        else:
            t = k[p, j].astype(np.float64) * x
            y[o - o_lo], mag[o - o_lo] = t.sum(), np.abs(t).sum()
    return y, mag


def resample64(s, rate, with_mag=False):
    """the whole signal at once -> y64 [ceil(N up / down)] (with_mag: also sum_j |K[p][j] s[q]| per output)"""
    y, mag = _outputs(s, 0, len(s), 0, n_out(len(s), rate), rate)
    return (y, mag) if with_mag else y


def emit_end(n_avail, rate):
    """before the final chunk: one past the last output whose last tap i down - width + klen - 1 is <= n_avail - 1"""
    _, up, down, klen, width = table(rate)
    t = n_avail - klen + width                                    # i goes out iff i down <= t
    i = 0 if t < 0 else t // down + 1
    assert i * down - width + klen - 1 > n_avail - 1 and (i == 0 or (i - 1) * down - width + klen - 1 <= n_avail - 1)
    return i * up


def stream64(s, rate, chunks):
    """the stream: -> (y64, per chunk (o0, n_emit, first, n_avail, retained afterwards)); every chunk sees only what the call retained"""
    _, up, down, klen, width = table(rate)
    assert sum(chunks) == len(s)
    tail, first, seen, o0, ys, log = np.zeros(0), 0, 0, 0, [], []
    for c, n_new in enumerate(chunks):
        final = c == len(chunks) - 1
        have = np.concatenate([tail, np.asarray(s[seen:seen + n_new], dtype=np.float64)])
        seen += n_new
        o1 = n_out(seen, rate) if final else max(o0, emit_end(seen, rate))
        ys.append(_outputs(have, first, seen, o0, o1, rate)[0])
        keep = seen if final else min(max(0, (o1 // up) * down - width), seen)
        log.append((o0, o1 - o0, first, seen, seen - keep))
        tail, first, o0 = have[keep - first:], keep, o1
    return np.concatenate(ys), log


def pcm16(y):
    """the int16 rule of section 1 on an fp32 array"""
    y = np.asarray(y, dtype=np.float32)
    v = (y * np.float32(32768)).astype(np.float64)
    v = np.where(np.isnan(v), 0.0, v)
    return np.trunc(np.clip(v, -32768.0, 32767.0)).astype(np.int16)


def ragged(n, seed, biggest=700):
    rng, left, out = np.random.default_rng(seed), n, []
    while left:
        k = int(rng.integers(1, min(left, biggest) + 1))
        out.append(k)
        left -= k
    return out


def chunkings(n, one_by_one=True):
    """all at once, one sample at a time, 480-sample chunks, seeded ragged chunks"""
    out = {'all at once': [n], '480-sample chunks': [480] * (n // 480) + ([n % 480] if n % 480 else []), 'ragged': ragged(n, n)}
    if one_by_one:
        out['one sample at a time'] = [1] * n
    return out
