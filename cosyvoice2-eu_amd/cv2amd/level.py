"""Host side of the output level (gain_db, peak_db, ceiling_db, lookahead_ms, loudness_lufs; DESIGN.md section 1, k_level in csrc/level.hip).

A `Level` value travels with a call from the public surface (CosyVoice2.level(...)) to the stage just ahead of the output conversion.  The
stage is defined on the global sample index of a call: with L = round(lookahead_ms * 24) sample n's gain depends on the samples n - L .. n + L,
so before the final chunk n can be emitted as soon as n + L <= n_available - 1; the final chunk emits the rest, its windows ending with the
signal.  A stream therefore runs L / 24000 s (5 ms by default) behind its vocoder, and a non-final chunk may come out empty; the last never
does.  The planner below only counts -- which samples a chunk emits, from which source sample on the call retains its input (at most 2 L) --
in Python integers, the same integers the kernel's entry point checks, so the two cannot disagree by a rounding.  No GPU and no torch for the
settings and the planner; the weight tables (cached per device and L) and the launches need both.  There is no CPU fallback.
"""
import ctypes as C
import math

from .sampling import f32

MODEL_RATE = 24000
FIELDS = ('gain_db', 'peak_db', 'ceiling_db', 'lookahead_ms', 'loudness_lufs')
RANGES = {'gain_db': (-24, 24), 'peak_db': (-24, 0), 'ceiling_db': (-12, 0), 'lookahead_ms': (1, 10), 'loudness_lufs': (-40, -5)}
CEILING_DB, LOOKAHEAD_MS = -1.0, 5.0              # what a call with any field set runs under where these two are not
L_MIN, L_MAX = 24, 240
_tables = {}


class Level:
    """gain_db, peak_db, ceiling_db, lookahead_ms, loudness_lufs: None = not set.  With nothing set there is no level stage at all.
    loudness_lufs scales the call to an integrated loudness (ITU-R BS.1770-4, measured on the device: cv2amd/loudness.py) as peak_db
    scales it to a peak; the two exclude each other."""
    __slots__ = FIELDS

    def __init__(self, gain_db=None, peak_db=None, ceiling_db=None, lookahead_ms=None, loudness_lufs=None):
        self.gain_db, self.peak_db, self.ceiling_db, self.lookahead_ms = gain_db, peak_db, ceiling_db, lookahead_ms
        self.loudness_lufs = loudness_lufs

    def __repr__(self):
        return 'Level(' + ', '.join(f'{k}={getattr(self, k)!r}' for k in FIELDS if getattr(self, k) is not None) + ')'

    def __eq__(self, o):
        return isinstance(o, Level) and all(getattr(self, k) == getattr(o, k) for k in FIELDS)

    def __hash__(self):
        return hash(tuple(getattr(self, k) for k in FIELDS))

    def is_default(self):
        """nothing set: no record is made and the call takes the path of a call without settings"""
        return all(getattr(self, k) is None for k in FIELDS)

    def replace(self, **kw):
        """a copy with the given (non-None) fields replaced"""
        d = {k: getattr(self, k) for k in FIELDS}
        d.update({k: v for k, v in kw.items() if v is not None})
        return Level(**d)

    def check(self):
        """ValueError for anything outside the accepted ranges (before any work); returns self"""
        for k in FIELDS:
            v = getattr(self, k)
            if v is None:
                continue
            if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v):
                raise ValueError(f'level: {k} must be a finite number, got {v!r}')
            lo, hi = RANGES[k]
            if not lo <= v <= hi:
                raise ValueError(f'level: {k} {v} outside {lo} .. {hi}')
        if self.peak_db is not None:
            ceiling = CEILING_DB if self.ceiling_db is None else self.ceiling_db
            if self.peak_db > ceiling:
                raise ValueError(f'level: peak_db {self.peak_db} above the ceiling of {ceiling} dBFS')
        if self.loudness_lufs is not None:
            if self.peak_db is not None:
                raise ValueError('level: loudness_lufs and peak_db both scale the call: set one of them')
            ceiling = CEILING_DB if self.ceiling_db is None else self.ceiling_db
            if self.loudness_lufs + 0.691 > ceiling:                          # (k_level takes no reference amplitude above its ceiling)
                raise ValueError(f'level: loudness_lufs {self.loudness_lufs} cannot be met under the ceiling of {ceiling} dBFS')
        return self

    def check_stream(self, stream):
        """a peak or loudness target needs the whole call, known at its end only: refused on a streaming call; returns self"""
        if stream and self.peak_db is not None:
            raise ValueError('level: peak_db needs the whole signal: it is not supported with stream=True (use gain_db)')
        if stream and self.loudness_lufs is not None:
            raise ValueError('level: loudness_lufs needs the whole signal: it is not supported with stream=True (use gain_db)')
        return self

    def resolve(self):
        """-> (G, c, L, T or None) the call runs under: the gain, the ceiling and the peak target as float32 values (computed in float64,
        rounded once), the look-ahead in samples.  Two settings that resolve to equal tuples are the same computation.  With loudness_lufs
        T is the reference amplitude of the loudness target, float32(10 ** ((loudness_lufs + 0.691) / 20)), which the level kernel divides
        by the measured R = sqrt(z) instead of the peak (`loud` tells the two apart)."""
        G = f32(10.0 ** ((0.0 if self.gain_db is None else self.gain_db) / 20.0))
        c = f32(10.0 ** ((CEILING_DB if self.ceiling_db is None else self.ceiling_db) / 20.0))
        L = int(round((LOOKAHEAD_MS if self.lookahead_ms is None else self.lookahead_ms) * 24))
        T = None if self.peak_db is None else min(f32(10.0 ** (self.peak_db / 20.0)), c)      # (peak_db <= ceiling_db; equal dB: equal floats)
        if self.loudness_lufs is not None:
            T = min(f32(10.0 ** ((self.loudness_lufs + 0.691) / 20.0)), c)
        return G, c, L, T

    @property
    def loud(self):
        """the call is scaled to a loudness target (resolve()'s T is then divided by the measured R, not by the peak)"""
        return self.loudness_lufs is not None


def check(level, stream=False):
    """what tts() does with its `level` keyword: None or nothing set -> None, else the checked settings"""
    if level is None or level.is_default():
        return None
    return level.check().check_stream(stream)


def window(L):
    """w[0 .. L] in float64: h_j / sum h, h_j = 0.5 - 0.5 cos(2 pi (j + 0.5) / (L + 1)); the device holds it rounded once to float32"""
    h = [0.5 - 0.5 * math.cos(2.0 * math.pi * (j + 0.5) / (L + 1)) for j in range(L + 1)]
    s = math.fsum(h)
    return [v / s for v in h]


class LevelState:
    """Per-call state: source samples consumed, samples emitted, and the global index of the first source sample still retained
    (the retained tail is the samples first .. consumed - 1; the tensor itself lives with the scheduler)."""
    __slots__ = ('L', 'consumed', 'emitted', 'first', 'final')

    def __init__(self, L):
        if isinstance(L, bool) or not isinstance(L, int) or not L_MIN <= L <= L_MAX:
            raise ValueError(f'level: look-ahead of {L!r} samples outside {L_MIN} .. {L_MAX}')
        self.L = L
        self.consumed = self.emitted = self.first = 0
        self.final = False

    @property
    def n_tail(self):
        return self.consumed - self.first

    def commit(self, n_new, n_emit, first_needed, final=False):
        """The chunk planned by plan(state, n_new, final) has been launched."""
        self.consumed += n_new
        self.emitted += n_emit
        self.first = first_needed
        self.final = final


def plan(state, n_new, final):
    """-> (n0, n_emit, first_needed) for a chunk of n_new further source samples: the chunk emits the samples n0 .. n0 + n_emit - 1;
    afterwards the source samples from first_needed on are retained (at most 2 L).  Does not change the state: see LevelState.commit."""
    if state.final:
        raise ValueError('level: the call has had its final chunk')
    if n_new < 0:
        raise ValueError('level: n_new < 0')
    n0, n_avail = state.emitted, state.consumed + n_new
    if final:
        return n0, n_avail - n0, n_avail
    n_next = max(n0, n_avail - state.L)                # n + L <= n_avail - 1 for n < n_next
    return n0, n_next - n0, max(0, n_next - state.L)


# ---- the device side -------------------------------------------------------------------------------------------------------------
class LevelArgs(C.Structure):
    """cv2_level_args (88 bytes): one call's chunk."""
    _fields_ = [(n, C.c_void_p) for n in ('tail', 'fresh', 'dst', 'weights', 'peak')] + [(n, C.c_int32) for n in
               ('first', 'n_tail', 'n_avail', 'n_final', 'n0', 'n_emit', 'L', 'dst_cap')] + [(n, C.c_float) for n in ('Ge', 'c', 'T')] + [
               ('reserved', C.c_int32)]


class WaveSeg(C.Structure):
    """cv2_wave_seg (16 bytes)"""
    _fields_ = [('src', C.c_void_p), ('n', C.c_int32), ('reserved', C.c_int32)]


def _bind(lib):
    if getattr(lib, '_level_bound', False):
        return
    lib.cv2_level_chunk.argtypes = [C.POINTER(LevelArgs), C.c_void_p]
    lib.cv2_level_chunk_batch.argtypes = [C.POINTER(LevelArgs), C.c_void_p, C.c_int32, C.c_void_p]
    lib.cv2_level_peak_batch.argtypes = [C.POINTER(WaveSeg), C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
    lib._level_bound = True


def weight_table(device, L):
    """w[0 .. L] on `device` (fp32: window(L) rounded once), cached per (device, L)"""
    import numpy as np
    import torch
    device = torch.device(device)
    key = (device.type, device.index if device.index is not None else torch.cuda.current_device(), int(L))
    if key not in _tables:
        _tables[key] = torch.from_numpy(np.asarray(window(L), dtype=np.float64).astype(np.float32)).to(device)
    return _tables[key]


def level_args(state, G, c, tail, fresh, dst, n0, n_emit, final, weights, peak=None, T=None):
    """One call's record for level_chunks: tail / fresh (1-D fp32 device tensors, None or empty: no such samples) are the source samples
    state.first .. state.consumed + len(fresh) - 1, dst (1-D float32 device tensor) receives the samples n0 .. n0 + n_emit - 1.  peak: a
    one-element fp32 device tensor holding the call's peak (level_peaks) with the target T, or None.  The integers come from plan(); the
    samples stay on the device."""
    import torch
    a = LevelArgs()
    for t in (tail, fresh, dst):
        assert t is None or (t.dim() == 1 and t.dtype == torch.float32 and (t.numel() <= 1 or t.stride(0) == 1))
    a.n_tail = 0 if tail is None else tail.numel()
    assert a.n_tail == state.n_tail and weights.numel() == state.L + 1
    if a.n_tail:
        a.tail = tail.data_ptr()
    n_new = 0 if fresh is None else fresh.numel()
    if n_new:
        a.fresh = fresh.data_ptr()
    if dst.numel():
        a.dst = dst.data_ptr()
    a.weights = weights.data_ptr()
    a.first, a.n_avail = state.first, state.consumed + n_new
    a.n_final = a.n_avail if final else -1
    a.n0, a.n_emit, a.dst_cap, a.L = n0, n_emit, dst.numel(), state.L
    a.Ge, a.c = G, c
    if peak is not None:
        assert peak.dtype == torch.float32 and peak.numel() == 1 and T is not None
        a.peak, a.T = peak.data_ptr(), T
    return a


def _upload(arr, device):
    """the records in device memory (pinned: ordered on the stream, the host goes on)"""
    import torch
    n = C.sizeof(arr)
    host = torch.empty(n, dtype=torch.uint8, pin_memory=True)
    C.memmove(host.data_ptr(), arr, n)
    return host.to(device or torch.device('cuda', torch.cuda.current_device()), non_blocking=True)


def level_chunks(args, device=None):
    """The level stage of one or several calls' chunks on the current HIP stream: cv2_level_chunk, or ONE cv2_level_chunk_batch launch
    (gridDim.z = calls) fed by a device table of the records.  The caller keeps the tensors behind the records alive."""
    from . import lib as L
    lib = L.lib()
    _bind(lib)
    if len(args) == 1:
        L.check(lib.cv2_level_chunk(C.byref(args[0]), L.stream_ptr()))
        return
    n = len(args)
    arr = (LevelArgs * n)(*args)
    table = _upload(arr, device)
    L.check(lib.cv2_level_chunk_batch(arr, table.data_ptr(), n, L.stream_ptr()))


def level_peaks(wavs, device=None):
    """P = max |s| (NaN counts as 0) of every signal of `wavs` (1-D fp32 device tensors) on the current HIP stream: ONE cv2_level_peak_batch
    call.  -> float32 [len(wavs)] on the device; nothing is copied to the host."""
    import torch
    from . import lib as L
    lib = L.lib()
    _bind(lib)
    k = len(wavs)
    for x in wavs:
        assert x.dim() == 1 and x.dtype == torch.float32 and x.is_cuda and (x.numel() <= 1 or x.stride(0) == 1)
    arr = (WaveSeg * k)(*[WaveSeg(x.data_ptr() if x.numel() else None, x.numel(), 0) for x in wavs])
    dev = device or wavs[0].device
    table = _upload(arr, dev)
    peaks = torch.empty(k, dtype=torch.float32, device=dev)
    L.check(lib.cv2_level_peak_batch(arr, table.data_ptr(), k, peaks.data_ptr(), L.stream_ptr()))
    return peaks
