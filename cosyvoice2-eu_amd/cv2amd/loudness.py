"""Host side of the loudness measurement (ITU-R BS.1770-4 integrated loudness at 24 kHz; DESIGN.md section 1, csrc/loudness.hip).

The K-weighting coefficients and the transition matrix of a hop are computed here in float64 and reach the device rounded once; `measure`
runs the measurement of a list of device signals as ONE cv2_loudness_batch enqueue and leaves the results (the reference amplitude R that
k_level divides a target by, and the loudness Lk in LUFS) on the device.  No GPU and no torch for the tables' values; the device tables
(cached per device) and the launches need both.  There is no CPU fallback.
"""
import ctypes as C
import math

from .level import MODEL_RATE, WaveSeg, _upload
from .sampling import f32

HOP = 2400                                        # samples per hop (100 ms); a block is four hops
SHELF = (1681.974450955533, 3.999843853973347, 0.7071752369554196, 0.4996667741545416)      # f0, G in dB, Q, the exponent of Vb
HIGHPASS = (38.13547087602444, 0.5003270373238773)                                           # f0, Q
G_MAX = f32(10.0 ** (24.0 / 20.0))                # R is clamped to [T / G_MAX, T * G_MAX]: the +-24 dB of gain_db
_tables = {}


def target(loudness_lufs):
    """T = float32(10 ** ((loudness_lufs + 0.691) / 20)): the amplitude whose mean square measures loudness_lufs"""
    return f32(10.0 ** ((loudness_lufs + 0.691) / 20.0))


def coefficients(fs=MODEL_RATE):
    """-> ((b, a) of the shelf, (b, a) of the high-pass), float64, a[0] = 1: the BS.1770 K-weighting for the sample rate fs"""
    f0, G, Q, p = SHELF
    K = math.tan(math.pi * f0 / fs)
    Vh = 10.0 ** (G / 20.0)
    Vb = Vh ** p
    a0 = 1.0 + K / Q + K * K
    shelf = ([(Vh + Vb * K / Q + K * K) / a0, 2.0 * (K * K - Vh) / a0, (Vh - Vb * K / Q + K * K) / a0],
             [1.0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0])
    f0, Q = HIGHPASS
    K = math.tan(math.pi * f0 / fs)
    a0 = 1.0 + K / Q + K * K
    high = ([1.0, -2.0, 1.0], [1.0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0])
    return shelf, high


def transition(fs=MODEL_RATE, steps=HOP):
    """M = A ** steps (4 x 4, float64, rows as lists): A takes the state (s1, s2, t1, t2) of the cascade -- both biquads in transposed direct
    form II -- over one sample of zero input"""
    (_b, a), (_d, c) = coefficients(fs)
    # y = s1; s1' = -a1 y + s2; s2' = -a2 y; w = y + t1; t1' = -2 y - c1 w + t2; t2' = y - c2 w
    A = [[-a[1], 1.0, 0.0, 0.0],
         [-a[2], 0.0, 0.0, 0.0],
         [-2.0 - c[1], 0.0, -c[1], 1.0],
         [1.0 - c[2], 0.0, -c[2], 0.0]]

    def mul(X, Y):
        return [[math.fsum(X[i][k] * Y[k][j] for k in range(4)) for j in range(4)] for i in range(4)]
    M, P, n = [[float(i == j) for j in range(4)] for i in range(4)], A, int(steps)
    while n:
        if n & 1:
            M = mul(M, P)
        P = mul(P, P)
        n >>= 1
    return M


def table_values(fs=MODEL_RATE):
    """the 24 values of the device table in float64: shelf b0 b1 b2 a1 a2, high-pass a1 a2, 0, M row-major"""
    (b, a), (_d, c) = coefficients(fs)
    return b + a[1:] + c[1:] + [0.0] + [v for row in transition(fs) for v in row]


def filter_table(device):
    """the table on `device` (fp32: table_values() rounded once), cached per device"""
    import numpy as np
    import torch
    device = torch.device(device)
    key = (device.type, device.index if device.index is not None else torch.cuda.current_device())
    if key not in _tables:
        _tables[key] = torch.from_numpy(np.asarray(table_values(), dtype=np.float64).astype(np.float32)).to(device)
    return _tables[key]


def blocks(n):
    """J: the 400 ms blocks of a signal of n samples"""
    return (n - 4 * HOP) // HOP + 1 if n >= 4 * HOP else 0


def _bind(lib):
    if getattr(lib, '_loudness_bound', False):
        return
    lib.cv2_loudness_workspace_bytes.argtypes = [C.POINTER(WaveSeg), C.c_int32, C.POINTER(C.c_size_t)]
    lib.cv2_loudness_batch.argtypes = [C.POINTER(WaveSeg), C.c_void_p, C.c_int32, C.POINTER(C.c_float), C.c_void_p, C.c_void_p, C.c_void_p,
                                       C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    lib._loudness_bound = True


def measure(wavs, targets=None, device=None):
    """R and Lk of every signal of `wavs` (1-D fp32 device tensors, the 24 kHz signals as they enter the level stage) on the current HIP
    stream: ONE cv2_loudness_batch enqueue.  targets: None, or one T per signal (target(); None or 0: that R is not clamped).
    -> (R, lufs), float32 [len(wavs)] on the device; nothing is copied to the host."""
    import torch
    from . import lib as L
    lib = L.lib()
    _bind(lib)
    k = len(wavs)
    for x in wavs:
        assert x.dim() == 1 and x.dtype == torch.float32 and x.is_cuda and (x.numel() <= 1 or x.stride(0) == 1)
    dev = device or wavs[0].device
    arr = (WaveSeg * k)(*[WaveSeg(x.data_ptr() if x.numel() else None, x.numel(), 0) for x in wavs])
    table = _upload(arr, dev)
    tg = tg_dev = None
    if targets is not None:
        assert len(targets) == k
        tg = (C.c_float * k)(*[0.0 if t is None else t for t in targets])
        tg_dev = _upload(tg, dev)
    need = C.c_size_t(0)
    L.check(lib.cv2_loudness_workspace_bytes(arr, k, C.byref(need)))
    ws = torch.empty(need.value // 4, dtype=torch.float32, device=dev)
    out = torch.empty(2, k, dtype=torch.float32, device=dev)
    L.check(lib.cv2_loudness_batch(arr, table.data_ptr(), k, tg, None if tg_dev is None else tg_dev.data_ptr(), filter_table(dev).data_ptr(),
                                   out[0].data_ptr(), out[1].data_ptr(), ws.data_ptr() if need.value else None, need.value, L.stream_ptr()))
    return out[0], out[1]
