"""numpy float64 restatement of the loudness measurement (ITU-R BS.1770-4 at 24 kHz), written from the definition and
independent of cv2amd/loudness.py and of the kernel: sequential biquads, blocks and gates.

    K-weighting: the shelf, then the high-pass, K = tan(pi f0 / fs), a0 = 1 + K / Q + K^2
      shelf      f0 = 1681.974450955533, G = 3.999843853973347 dB, Q = 0.7071752369554196, Vh = 10^(G / 20), Vb = Vh^0.4996667741545416
                 b = [(Vh + Vb K / Q + K^2) / a0, 2 (K^2 - Vh) / a0, (Vh - Vb K / Q + K^2) / a0], a = [1, 2 (K^2 - 1) / a0, (1 - K / Q + K^2) / a0]
      high-pass  f0 = 38.13547087602444, Q = 0.5003270373238773, b = [1, -2, 1], a = [1, 2 (K^2 - 1) / a0, (1 - K / Q + K^2) / a0]
    blocks: hop 2400; block j = y[2400 j .. 2400 j + 9600), J = floor((N - 9600) / 2400) + 1 when N >= 9600 else 0
    z_j = mean y^2, l_j = -0.691 + 10 log10 z_j;  A = {l_j > -70};  Gamma = -0.691 + 10 log10 mean_A z_j - 10;  B = {j in A : l_j > Gamma}
    Lk = -0.691 + 10 log10 mean_B z_j;  no block or A empty: -inf.  A non-finite sample counts as 0.

This is the yardstick, never the device code.  float32 and float64 differ by rounding, so a block that sits on a gate can legitimately flip
between them: measure() also returns the distance in LU of the nearest block from either gate (the gate margin), and every test asserts
that margin on its input before it compares anything.
"""
import math

import numpy as np

HOP, BLOCK, FS = 2400, 9600, 24000
MARGIN = 0.05                                                       # LU: the least gate margin of a test input
WORST_LU = 8.07e-4                                                  # worst |Lk - oracle| measured on an MI355X over the GPU tests' cases (the 20 Hz
#                                                                     tone on a DC offset of 0.5; every other case is below 1e-5 LU)
BAR_LU = 4 * WORST_LU                                               # their bar: 4 x WORST_LU = 3.23e-3, never above 0.01 LU
assert BAR_LU <= 0.01
N_LONG = 73234                                                      # 30 hops and a tail of 1234: 27 blocks


def coefficients(fs=FS):
    K = math.tan(math.pi * 1681.974450955533 / fs)
    Vh = 10.0 ** (3.999843853973347 / 20.0)
    Vb = Vh ** 0.4996667741545416
    Q = 0.7071752369554196
    a0 = 1.0 + K / Q + K * K
    shelf = ((Vh + Vb * K / Q + K * K) / a0, 2.0 * (K * K - Vh) / a0, (Vh - Vb * K / Q + K * K) / a0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0)
    K = math.tan(math.pi * 38.13547087602444 / fs)
    Q = 0.5003270373238773
    a0 = 1.0 + K / Q + K * K
    high = (1.0, -2.0, 1.0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0)
    return shelf, high


def biquad(x, c):
    """direct form I in float64, sample after sample"""
    b0, b1, b2, a1, a2 = c
    y = np.empty(len(x), dtype=np.float64)
    x1 = x2 = y1 = y2 = 0.0
    for i, v in enumerate(x.tolist()):
        w = b0 * v + b1 * x1 + b2 * x2 - a1 * y1 - a2 * y2
        x2, x1, y2, y1 = x1, v, y1, w
        y[i] = w
    return y


def kweight(s, fs=FS):
    x = np.asarray(s, dtype=np.float64)
    x = np.where(np.isfinite(x), x, 0.0)
    shelf, high = coefficients(fs)
    return biquad(biquad(x, shelf), high)


def blocks(n):
    return (n - BLOCK) // HOP + 1 if n >= BLOCK else 0


def measure(s):
    """-> dict: lufs (float, -inf), z (mean square behind it, 0), J, nA, nB (blocks in all, past the absolute gate, past both), margin (LU
    between the nearest block and either gate; inf when there is no block)"""
    hop, blk = HOP, BLOCK
    y = kweight(s)
    J = (len(y) - blk) // hop + 1 if len(y) >= blk else 0
    zj = np.array([np.mean(y[hop * j:hop * j + blk] ** 2) for j in range(J)], dtype=np.float64)
    with np.errstate(divide='ignore'):
        lj = -0.691 + 10.0 * np.log10(zj)
    res = dict(lufs=-math.inf, z=0.0, J=J, nA=0, nB=0, margin=math.inf)
    if J:
        res['margin'] = float(np.min(np.abs(lj + 70.0)))
    A = lj > -70.0
    if not A.any():
        return res
    gamma = -0.691 + 10.0 * math.log10(zj[A].mean()) - 10.0
    B = A & (lj > gamma)
    z = zj[B].mean()
    res.update(lufs=-0.691 + 10.0 * math.log10(z), z=float(z), nA=int(A.sum()), nB=int(B.sum()), gamma=gamma,
               margin=float(min(res['margin'], np.min(np.abs(lj[A] - gamma)))))
    return res


# ---- the seeded inputs of the GPU tests (each chosen on the CPU to keep the gate margin) --------------------------------------------------
def sine(n=N_LONG, amp=0.1, f=997.0):
    return (amp * np.sin(2.0 * np.pi * f * np.arange(n) / FS)).astype(np.float32)


def bursts(n=N_LONG, seed=11):
    """noise bursts of very different levels with a silent second between them: both gates act"""
    g = np.random.default_rng(seed)
    s = np.zeros(n, dtype=np.float64)
    for start, length, amp in ((0, 14000, 0.2), (38000, 9000, 0.012), (47000, 6000, 1e-5), (53000, 20234, 0.06)):
        s[start:start + length] = amp * g.standard_normal(length)
    return s.astype(np.float32)


def rumble(n=N_LONG):
    """a 20 Hz tone on a DC offset of 0.5: the high-pass's long memory shows a wrong state hand-over between hops as a gross error"""
    return (0.5 + 0.1 * np.sin(2.0 * np.pi * 20.0 * np.arange(n) / FS)).astype(np.float32)


def specials(n=N_LONG, seed=5):
    """-> (the signal with NaN and +-inf samples, the same with those samples set to 0)"""
    g = np.random.default_rng(seed)
    clean = (0.05 * g.standard_normal(n)).astype(np.float32)
    idx = g.choice(n, size=60, replace=False)
    clean[idx] = 0.0
    s = clean.copy()
    s[idx[:20]], s[idx[20:40]], s[idx[40:]] = np.nan, np.inf, -np.inf
    return s, clean


def voice(n, seed, amp=0.01):
    """a quiet, speech-like signal: noise under a slow envelope with a pause"""
    g = np.random.default_rng(seed)
    t = np.arange(n) / FS
    env = 0.6 + 0.4 * np.sin(2.0 * np.pi * 1.7 * t)
    s = amp * env * g.standard_normal(n)
    s[n // 3:n // 3 + 9000] = 0.0
    return s.astype(np.float32)
