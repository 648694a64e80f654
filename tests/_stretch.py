"""numpy fp32 restatement of the streaming time-stretch, written from the definition and independent of
cv2amd/stretch.py and of the kernel:

    r = float32(speed);  x_j = max(0, r (j + 0.5) - 0.5) in fp32;  i0 = floor(x_j);  i1 = min(i0 + 1, N - 1);
    w1 = x_j - i0;  w0 = 1 - w1;  out[j] = w0 m[i0] + w1 m[i1]  for j < int(N / speed).

x_j is one fused multiply-add (rounded once), the form torch's CPU interpolation evaluates; here: the exact value in float64 (r and
j + 0.5 carry 24 significant bits each, j < 2^23), rounded to float32.
"""
import numpy as np

SPEEDS = (0.5, 0.8, 1.0, 1.25, 1.6, 2.0)
PLAN_SPEEDS = SPEEDS + (1.9999, 0.7071)


def positions(speed, j):
    """x_j (fp32) for an array of global output indices j."""
    j = np.asarray(j)
    assert j.size == 0 or (j.min() >= 0 and j.max() < 1 << 23)
    x = (np.float64(np.float32(speed)) * (j.astype(np.float64) + 0.5) - 0.5).astype(np.float32)
    return np.maximum(x, np.float32(0))


def index0(speed, j):
    return np.floor(positions(speed, j)).astype(np.int64)


def n_out(n, speed):
    return int(n / speed)


def stretch(m, speed, with_operands=False):
    """m [..., N] fp32 -> [..., int(N / speed)] fp32 (with_operands: also the two products that are summed)."""
    m = np.asarray(m)
    assert m.dtype == np.float32
    n = m.shape[-1]
    j = np.arange(n_out(n, speed))
    x = positions(speed, j)
    i0 = np.floor(x).astype(np.int64)
    i1 = np.minimum(i0 + 1, n - 1)
    w1 = x - i0.astype(np.float32)
    w0 = np.float32(1) - w1
    a, b = w0 * m[..., i0], w1 * m[..., i1]
    out = a + b
    assert out.dtype == np.float32
    return (out, a, b) if with_operands else out


def emittable(speed, j, n_available):
    """before the final chunk: frame j may go out as soon as i0 + 1 <= n_available - 1"""
    return int(index0(speed, [j])[0]) + 1 <= n_available - 1


def chunkings(n, rng, n_random=2):
    """chunk-size lists that sum to n: everything at once, one frame at a time, 50-frame chunks, seeded random ones"""
    out = [[n], [1] * n, [50] * (n // 50) + ([n % 50] if n % 50 else [])]
    for _ in range(n_random):
        left, c = n, []
        while left:
            k = int(rng.integers(1, min(left, 60) + 1))
            c.append(k)
            left -= k
        out.append(c)
    return out
