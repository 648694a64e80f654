"""Host side of joined calls (CosyVoice2.joined(...); DESIGN.md section 1, csrc/join.hip): the 24 kHz waveforms of one call's text segments
written into ONE waveform on the device -- interior silences optionally trimmed, a pause of zeros between the pieces, a short raised-cosine
fade at each trimmed edge -- ahead of the output stage and the one device-to-host copy.

A `Join` value travels with a call from the public surface to CosyVoice2Model.tts_joined.  The planner below only counts, in Python
integers: which samples [a_i, b_i) of segment i are kept (the device finds them: cv2_wave_bounds), where each piece lands in the joined
signal, which edges fade.  The same integers are checked by the entry points before they launch.  No GPU and no torch for the planner; the
bindings at the end need both.  There is no CPU fallback.
"""
import ctypes as C
import math

from .sampling import f32

FIELDS = ('pause_ms', 'trim_db', 'fade_ms')
MODEL_RATE = 24000
FRAME, KEEP = 240, 480                 # csrc/join.hip: samples per frame; samples kept beyond the first / last loud frame
MAX_PIECES = 256                       # CV2_WAVE_MAX_PIECES
FADE_IN, FADE_OUT = 1, 2               # CV2_WAVE_FADE_IN, CV2_WAVE_FADE_OUT
DEFAULT_PAUSE_MS, DEFAULT_FADE_MS = 150, 5
_tables = {}


class Join:
    """pause_ms: silence between two segments (0 .. 5000; 150 when anything else is set); trim_db: interior silences are trimmed to 20 ms
    around the frames within trim_db of the segment's peak (20 .. 80; None: nothing is trimmed); fade_ms: raised-cosine fade at every
    trimmed edge (0 .. 20, only with trim_db; 5 when trim_db is set)."""
    __slots__ = FIELDS

    def __init__(self, pause_ms=None, trim_db=None, fade_ms=None):
        self.pause_ms, self.trim_db, self.fade_ms = pause_ms, trim_db, fade_ms

    def __repr__(self):
        return 'Join(' + ', '.join(f'{k}={getattr(self, k)!r}' for k in FIELDS if getattr(self, k) is not None) + ')'

    def __eq__(self, o):
        return isinstance(o, Join) and all(getattr(self, k) == getattr(o, k) for k in FIELDS)

    def __hash__(self):
        return hash((self.pause_ms, self.trim_db, self.fade_ms))

    def is_default(self):
        """nothing set: the call is not joined and takes the path of a call without settings"""
        return self.pause_ms is None and self.trim_db is None and self.fade_ms is None

    def replace(self, **kw):
        """a copy with the given (non-None) fields replaced"""
        d = {k: getattr(self, k) for k in FIELDS}
        d.update({k: v for k, v in kw.items() if v is not None})
        return Join(**d)

    def check(self):
        """ValueError for anything outside the accepted ranges (before any work); returns self"""
        for name, lo, hi in (('pause_ms', 0, 5000), ('trim_db', 20, 80), ('fade_ms', 0, 20)):
            v = getattr(self, name)
            if v is None:
                continue
            if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v):
                raise ValueError(f'join: {name} must be a finite number, got {v!r}')
            if not lo <= v <= hi:
                raise ValueError(f'join: {name} {v} outside {lo} .. {hi}')
        if self.fade_ms is not None and self.trim_db is None:
            raise ValueError('join: fade_ms needs trim_db (only trimmed edges fade)')
        return self

    def resolve(self):
        """(pause, F, g) the call runs under: pause and fade length in samples at 24 kHz (F = 0 without trim_db), g = the loudness
        threshold relative to the segment's peak as the device holds it (None without trim_db)."""
        pause = round((DEFAULT_PAUSE_MS if self.pause_ms is None else self.pause_ms) * 24)
        if self.trim_db is None:
            return pause, 0, None
        return pause, round((DEFAULT_FADE_MS if self.fade_ms is None else self.fade_ms) * 24), f32(10.0 ** (-self.trim_db / 20.0))


def plan(lengths, bounds, join):
    """-> (pieces, N, spans) for segments of `lengths` samples of which [a_i, b_i) = bounds[i] is kept (bounds None: everything).
    pieces[i] = (src_off, m, dst_off, fade flags) is segment i's record for wave_join, N the length of the joined signal (the pieces with
    `pause` zeros between them), spans[i] = (start, end) of piece i in it.  An edge fades when it may have been trimmed (interior), F > 0
    and the piece holds both fades (m >= 2 F)."""
    pause, F, _g = join.resolve()
    k = len(lengths)
    if not 1 <= k <= MAX_PIECES:
        raise ValueError(f'join: {k} segments, 1 .. {MAX_PIECES} can be joined')
    pieces, spans, off = [], [], 0
    for i, n in enumerate(lengths):
        a, b = (0, n) if bounds is None else (int(bounds[i][0]), int(bounds[i][1]))
        if not 0 <= a <= b <= n:
            raise ValueError(f'join: segment {i}: kept range [{a}, {b}) outside its {n} samples')
        m = b - a
        fade = 0
        if F > 0 and m >= 2 * F:
            fade = (FADE_IN if i > 0 else 0) | (FADE_OUT if i < k - 1 else 0)
        pieces.append((a, m, off, fade))
        spans.append((off, off + m))
        off += m + (pause if i < k - 1 else 0)
    return pieces, off, spans


def fade_table(F):
    """w[t] = 0.5 - 0.5 cos(pi (t + 0.5) / F), t = 0 .. F - 1: float64, rounded once to float32 (numpy array)"""
    import numpy as np
    t = np.arange(F, dtype=np.float64)
    return (0.5 - 0.5 * np.cos(np.pi * (t + 0.5) / F)).astype(np.float32) if F > 0 else np.zeros(0, dtype=np.float32)


# ---- the device side -------------------------------------------------------------------------------------------------------------
class WaveSeg(C.Structure):
    """cv2_wave_seg (16 bytes)"""
    _fields_ = [('src', C.c_void_p), ('n', C.c_int32), ('reserved', C.c_int32)]


class WavePiece(C.Structure):
    """cv2_wave_piece (32 bytes)"""
    _fields_ = [('src', C.c_void_p)] + [(n, C.c_int32) for n in ('n_src', 'src_off', 'm', 'dst_off', 'fade', 'reserved')]


def _bind(lib):
    if getattr(lib, '_join_bound', False):
        return
    lib.cv2_wave_bounds.argtypes = [C.POINTER(WaveSeg), C.c_void_p, C.c_int32, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.cv2_wave_join.argtypes = [C.POINTER(WavePiece), C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p]
    lib._join_bound = True


def _upload(arr, device):
    """the records in device memory (pinned: ordered on the stream, the host goes on)"""
    import torch
    n = C.sizeof(arr)
    host = torch.empty(n, dtype=torch.uint8, pin_memory=True)
    C.memmove(host.data_ptr(), arr, n)
    return host.to(device, non_blocking=True)


def _flat(wavs):
    import torch
    out = []
    for w in wavs:
        x = w.reshape(-1)
        assert x.dtype == torch.float32 and x.is_cuda and (x.numel() <= 1 or x.stride(0) == 1)
        out.append(x)
    return out


def fade_table_dev(device, F):
    """fade_table(F) on `device`, cached per (device, F); None for F = 0"""
    import torch
    device = torch.device(device)
    key = (device.type, device.index if device.index is not None else torch.cuda.current_device(), F)
    if key not in _tables:
        _tables[key] = torch.from_numpy(fade_table(F)).to(device) if F > 0 else None
    return _tables[key]


def wave_bounds(wavs, g):
    """The kept ranges of the segments `wavs` (fp32 device tensors, [n] or [1, n]) under the threshold g, on the current HIP stream: ONE
    cv2_wave_bounds call.  -> (bounds int32 [k, 2], peaks float32 [k]), both on the device: the caller copies the 2 k integers."""
    import torch
    from . import lib as L
    lib = L.lib()
    _bind(lib)
    xs = _flat(wavs)
    k, dev = len(xs), xs[0].device
    arr = (WaveSeg * k)(*[WaveSeg(x.data_ptr(), x.numel(), 0) for x in xs])
    table = _upload(arr, dev)
    bounds = torch.empty(k, 2, dtype=torch.int32, device=dev)
    peaks = torch.empty(k, dtype=torch.float32, device=dev)
    L.check(lib.cv2_wave_bounds(arr, table.data_ptr(), k, g, bounds.data_ptr(), peaks.data_ptr(), L.stream_ptr()))
    return bounds, peaks


def wave_join(wavs, pieces, N, F, dst=None):
    """The joined signal of plan()'s `pieces` over the segments `wavs`, on the current HIP stream: ONE cv2_wave_join launch writes every
    sample of dst (a new float32 [N] device tensor unless given: 1-D, contiguous, aligned to 4 bytes only)."""
    import torch
    from . import lib as L
    lib = L.lib()
    _bind(lib)
    xs = _flat(wavs)
    k, dev = len(xs), xs[0].device
    assert len(pieces) == k
    if dst is None:
        dst = torch.empty(N, dtype=torch.float32, device=dev)
    assert dst.dim() == 1 and dst.dtype == torch.float32 and dst.numel() == N and (N <= 1 or dst.stride(0) == 1)
    arr = (WavePiece * k)(*[WavePiece(x.data_ptr(), x.numel(), a, m, off, fade, 0) for x, (a, m, off, fade) in zip(xs, pieces)])
    table = _upload(arr, dev)
    ft = fade_table_dev(dev, F)
    L.check(lib.cv2_wave_join(arr, table.data_ptr(), k, None if ft is None else ft.data_ptr(), F, dst.data_ptr() if N else None, N, L.stream_ptr()))
    return dst
