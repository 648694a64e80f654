"""numpy restatement of the joined call's definitions (include/cv2_amd.h: cv2_wave_bounds, cv2_wave_join), written from
the definitions and not from cv2amd/join.py: the kept range of every segment, the plan of the joined signal, and the signal itself.  Every
quantity is a maximum, one rounded fp32 product or an integer, so the device must agree exactly."""
import numpy as np

FRAME, KEEP = 240, 480


def gain(trim_db):
    """g = float32(10 ** (-trim_db / 20)): float64, rounded once"""
    return np.float32(10.0 ** (-float(trim_db) / 20.0))


def samples(ms):
    return int(round(ms * 24))


def fade_table(F):
    t = np.arange(F, dtype=np.float64)
    return (0.5 - 0.5 * np.cos(np.pi * (t + 0.5) / F)).astype(np.float32) if F > 0 else np.zeros(0, np.float32)


def peak(seg):
    """P = max over the frames of the frame peak = max |s| with NaN as 0 (float32)"""
    v = np.abs(np.asarray(seg, dtype=np.float32))
    v = np.where(np.isnan(v), np.float32(0), v)
    return np.float32(v.max()) if v.size else np.float32(0)


def bounds(segs, g):
    """[(a_i, b_i)] of the segments (1-D float32 arrays) under the threshold g (None: nothing is trimmed)"""
    k, out = len(segs), []
    for i, s in enumerate(segs):
        s = np.asarray(s, dtype=np.float32)
        n = s.size
        if g is None:
            out.append((0, n))
            continue
        v = np.abs(s)
        v = np.where(np.isnan(v), np.float32(0), v)
        n_frames = -(-n // FRAME)
        peaks = np.array([v[FRAME * f:min(FRAME * f + FRAME, n)].max() for f in range(n_frames)], dtype=np.float32)
        P = np.float32(peaks.max())
        if not P > 0:
            out.append((0, n))
            continue
        thr = np.float32(P * np.float32(g))                                   # one fp32 product
        loud = np.nonzero(peaks >= thr)[0]
        f_lo, f_hi = int(loud[0]), int(loud[-1])
        a = max(0, FRAME * f_lo - KEEP) if i > 0 else 0
        b = min(n, FRAME * (f_hi + 1) + KEEP) if i < k - 1 else n
        out.append((a, b))
    return out


def plan(lengths, bnds, pause, F):
    """-> ([(a, m, dst_off, fade_in, fade_out)], N, [(start, end)])"""
    k, pieces, spans, off = len(lengths), [], [], 0
    for i, n in enumerate(lengths):
        a, b = bnds[i]
        m = b - a
        fades = F > 0 and m >= 2 * F
        pieces.append((a, m, off, fades and i > 0, fades and i < k - 1))
        spans.append((off, off + m))
        off += m
        if i < k - 1:
            off += pause
    return pieces, off, spans


def join(segs, bnds, pause, F):
    """the joined signal (float32) of the kept pieces, `pause` zeros between them, fades of F samples at interior edges"""
    pieces, N, spans = plan([len(s) for s in segs], bnds, pause, F)
    w = fade_table(F)
    out = np.zeros(N, dtype=np.float32)                                       # gaps: +0.0
    for s, (a, m, off, fin, fout) in zip(segs, pieces):
        x = np.array(np.asarray(s, dtype=np.float32)[a:a + m], copy=True)
        if fin:
            x[:F] = x[:F] * w                                                 # one fp32 multiply per sample
        if fout:
            x[m - F:] = x[m - F:] * w[::-1]
        out[off:off + m] = x
    return out, spans
