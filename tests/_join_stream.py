"""numpy restatement of the continuous call's definitions (include/cv2_amd.h: cv2_wave_gate_chunk, cv2_wave_emit_chunk),
written from the definitions and not from cv2amd/join.py, and from WHOLE segment signals: the causal gate, the kept range of every segment,
the call's signal, and how much of it may be out once a given prefix of a segment has arrived.  Every quantity is a maximum, one rounded fp32
product or an integer, so the device and the planner must agree exactly."""
import numpy as np

import _join as R

FRAME, KEEP = R.FRAME, R.KEEP
gain, samples, fade_table = R.gain, R.samples, R.fade_table


def _abs(seg):
    v = np.abs(np.asarray(seg, dtype=np.float32))
    return np.where(np.isnan(v), np.float32(0), v)


def loud_frames(seg, C, g, n=None, ended=True):
    """indices of the loud frames among the frames of seg[:n] that exist (the short last one only once the segment has ended)"""
    v = _abs(seg)[:len(seg) if n is None else n]
    n_frames = -(-v.size // FRAME) if ended else v.size // FRAME
    out, run = [], np.float32(C)
    for f in range(n_frames):
        p = np.float32(v[FRAME * f:min(FRAME * f + FRAME, v.size)].max())
        run = np.float32(max(run, p))                                         # R_i(f)
        if run > 0 and p >= np.float32(run * np.float32(g)):                  # one fp32 product
            out.append(f)
    return out


def carries(segs):
    """C_i = max |s| over every sample of the segments before i"""
    out, c = [], np.float32(0)
    for s in segs:
        out.append(c)
        v = _abs(s)
        c = np.float32(max(c, v.max())) if v.size else c
    return out


def bounds(segs, g):
    """[(a_i, b_i)] under the causal gate (g None: everything is kept)"""
    k, out = len(segs), []
    for i, (s, C) in enumerate(zip(segs, carries(segs))):
        n = len(s)
        loud = [] if g is None else loud_frames(s, C, g)
        if not loud:
            out.append((0, n))
            continue
        a = max(0, FRAME * loud[0] - KEEP) if i > 0 else 0
        b = min(n, FRAME * (loud[-1] + 1) + KEEP) if i < k - 1 else n
        out.append((a, b))
    return out


def stream(segs, g, pause, F):
    """-> (the call's 24 kHz signal, [(start, end)] of the pieces in it): the join's fade rule and table over the gate's ranges"""
    return R.join(segs, bounds(segs, g), pause, F if g is not None else 0)


def emitted(segs, g, pause, F, i, n, ended):
    """samples of the call's signal that are out once segment i has delivered its first n samples (ended: these are all of it)"""
    k = len(segs)
    bn = bounds(segs, g)
    base = sum(b - a for a, b in bn[:i]) + pause * i
    if ended:
        return base + bn[i][1] - bn[i][0] + (pause if i < k - 1 else 0)
    if g is None:
        return base + n
    loud = loud_frames(segs[i], carries(segs)[i], g, n, ended=False)
    if not loud:                                                              # (a piece i > 0: f_lo unknown; piece 0: nothing is loud yet)
        return base
    a = max(0, FRAME * loud[0] - KEEP) if i > 0 else 0
    if i == k - 1:
        return base + n - a
    return base + FRAME * (loud[-1] + 1) - F - a
