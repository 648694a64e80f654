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


# ---- continuous calls: the segments' chunks as ONE stream (CosyVoice2.continuous(...); DESIGN.md section 1, csrc/join_stream.hip) ------------
MAX_STREAM_FADE_MS = 5                 # F <= 120 samples: both fades of a piece fit inside one 240-sample frame


def check_continuous(join):
    """ValueError for settings a continuous view does not take: Join.check(), and fade_ms 0 .. 5; returns join"""
    join.check()
    if join.fade_ms is not None and join.fade_ms > MAX_STREAM_FADE_MS:
        raise ValueError(f'continuous: fade_ms {join.fade_ms} outside 0 .. {MAX_STREAM_FADE_MS}')
    return join


class Emit:
    """One chunk's emission, in positions of the current segment: the samples e0 .. e1 - 1 go out, followed by n_zero zeros; a lead fade
    starts at fade_in_at, a tail fade ends at fade_out_end (-1: none); the samples from keep_from on stay held."""
    __slots__ = ('e0', 'e1', 'fade_in_at', 'fade_out_end', 'n_zero', 'keep_from')

    def __init__(self, e0, e1, fade_in_at, fade_out_end, n_zero, keep_from):
        self.e0, self.e1, self.fade_in_at, self.fade_out_end, self.n_zero, self.keep_from = e0, e1, fade_in_at, fade_out_end, n_zero, keep_from

    @property
    def n_out(self):
        return self.e1 - self.e0 + self.n_zero


class StreamPlan:
    """The planner of a continuous call of k segments under `join`, in Python integers (the entry points check the same integers).  Per
    chunk of the current segment: gate_range(n_new, end) -> the frames the device analyses (None: no analysis is needed), then
    step(n_new, end, f_lo, f_hi) with the segment's first / last loud frame so far (the device's record; -1: none) -> an Emit; the state
    advances.  The gate is causal -- frame f is loud against the running maximum R(f) over everything up to f, not against the segment's
    peak as in .joined() -- so that nothing it decides depends on where the chunks end."""

    def __init__(self, join, k):
        if not 2 <= k <= MAX_PIECES:
            raise ValueError(f'continuous: {k} segments, 2 .. {MAX_PIECES} can be streamed as one')
        self.pause, self.F, self.g = check_continuous(join).resolve()
        self.k, self.i, self.pos, self.spans = k, 0, 0, []
        self._open()

    def _open(self):
        # n: samples received; frames: frames analysed; e: the next sample to go out = the first held one; a: the piece's start, once known
        self.n, self.frames, self.e, self.emitted_any = 0, 0, 0, False
        self.a = 0 if (self.g is None or self.i == 0) else None

    @property
    def done(self):
        return self.i >= self.k

    @property
    def n_held(self):
        return self.n - self.e

    @property
    def gated(self):
        """the current segment still needs the device's analysis: an interior edge of it is still open"""
        return self.g is not None and not (self.i == self.k - 1 and self.a is not None)

    def gate_range(self, n_new, end):
        if not self.gated:
            return None
        n = self.n + n_new
        return self.frames, (-(-n // FRAME) if end else n // FRAME)

    def step(self, n_new, end, f_lo=-1, f_hi=-1):
        if self.done:
            raise ValueError('continuous: the call has had its last segment')
        if n_new < 0:
            raise ValueError('continuous: n_new < 0')
        i, k, F = self.i, self.k, self.F
        gated, last = self.gated, self.i == self.k - 1
        n = self.n + n_new
        if gated:
            self.frames = -(-n // FRAME) if end else n // FRAME
            if not -1 <= f_lo <= f_hi < max(self.frames, 1) or (f_lo < 0) != (f_hi < 0):
                raise ValueError(f'continuous: loud frames {f_lo} .. {f_hi} of {self.frames}')
        else:
            f_hi = -1
        e0 = self.e
        if self.a is None:                                                    # a piece i > 0 whose first loud frame is not known yet
            if f_lo >= 0:
                self.a = e0 = max(0, FRAME * f_lo - KEEP)
            elif end:
                self.a = 0                                                    # no loud frame at all: kept whole
        b = None
        if self.a is None:
            e1 = e0
        elif end:
            b = n if (last or not gated or f_hi < 0) else min(n, FRAME * (f_hi + 1) + KEEP)
            e1 = b
        elif last or not gated:
            e1 = n
        else:                                                                 # the quiet run behind the last loud frame and the fade wait
            e1 = max(e0, FRAME * (f_hi + 1) - F) if f_hi >= 0 else e0
        fades = F > 0 and self.g is not None
        if b is not None:
            fades = fades and b - self.a >= 2 * F                             # the join's rule; a piece with a whole loud frame has 240 >= 2 F
            assert fades or F == 0 or self.g is None or not self.emitted_any
        fade_in_at = self.a if (fades and i > 0 and e1 > e0 and e0 < self.a + F) else -1
        fade_out_end = b if (fades and b is not None and not last) else -1
        n_zero = self.pause if (end and not last) else 0
        em = Emit(e0, e1, fade_in_at, fade_out_end, n_zero, n if end else e1)
        self.emitted_any = self.emitted_any or e1 > e0
        if end:
            self.spans.append((self.pos, self.pos + b - self.a))
            self.pos += b - self.a + n_zero
            self.i += 1
            if not self.done:
                self._open()
        else:
            self.n, self.e = n, e1
        return em


class WaveState(C.Structure):
    """cv2_wave_state (32 bytes)"""
    _fields_ = [('r_bits', C.c_uint32), ('c_bits', C.c_uint32)] + [(n, C.c_int32) for n in ('frames', 'f_lo', 'f_hi', 'n_held', 'held_start', 'reserved')]


class WaveEmit(C.Structure):
    """cv2_wave_emit (88 bytes)"""
    _fields_ = [(n, C.c_void_p) for n in ('held', 'chunk', 'fade_table', 'dst', 'held_dst')] + [(n, C.c_int32) for n in (
        'held_start', 'n_held', 'n_new', 'e0', 'e1', 'fade_in_at', 'fade_out_end', 'F', 'n_zero', 'keep_from', 'held_cap', 'reserved')]


def _bind_stream(lib):
    if getattr(lib, '_join_stream_bound', False):
        return
    lib.cv2_wave_gate_chunk.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                        C.c_float, C.c_void_p, C.c_void_p]
    lib.cv2_wave_emit_chunk.argtypes = [C.c_void_p, C.POINTER(WaveEmit), C.c_void_p]
    lib._join_stream_bound = True


class WaveStream:
    """The device side of one continuous call: its StreamPlan, the cv2_wave_state record and the held samples (two buffers that take
    turns, grown when a quiet run outlasts them).  chunk(wav, end) -> the 24 kHz samples [n] that go out with this chunk of the current
    segment, on the current HIP stream: at most one cv2_wave_gate_chunk, ONE copy of its four integers to the host (the only added
    synchronisation) and one cv2_wave_emit_chunk.  A chunk that goes out whole and unchanged with nothing held is handed on as it is.
    into = (a 1-D float32 device tensor, position): the samples are written there instead (always by the kernel), whatever its alignment."""

    def __init__(self, join, k, device):
        import torch
        self.plan, self.device = StreamPlan(join, k), torch.device(device)
        self.state = torch.zeros(8, dtype=torch.int32, device=self.device)
        self.record = torch.empty(4, dtype=torch.int32, device=self.device)
        self.held, self.spare = None, None
        self.f_lo = self.f_hi = -1
        self.launches = 0                                                      # gate + emit launches so far (diagnostics / tests)

    def close(self):
        self.state = self.record = self.held = self.spare = None

    def chunk(self, wav, end, into=None):
        import torch
        from . import lib as L
        lib = L.lib()
        _bind_stream(lib)
        pl = self.plan
        x = _flat([wav])[0]
        n_new, h0, n_held = x.numel(), pl.e, pl.n_held
        cur = torch.cuda.current_stream()
        for t in (self.state, self.record, self.held, self.spare):
            if t is not None:
                t.record_stream(cur)                                           # (the call's previous chunk may have run on another stream)
        seg_start = pl.n == 0 and pl.frames == 0
        if seg_start:
            self.f_lo = self.f_hi = -1
        fr = pl.gate_range(n_new, end)
        if fr is not None and (fr[1] > fr[0] or seg_start):
            L.check(lib.cv2_wave_gate_chunk(self.state.data_ptr(), self.held.data_ptr() if n_held else None, h0, n_held,
                                            x.data_ptr() if n_new else None, n_new, fr[0], fr[1], int(seg_start), pl.g,
                                            self.record.data_ptr(), L.stream_ptr()))
            self.launches += 1
            if fr[1] > fr[0]:
                self.f_lo, self.f_hi = self.record.cpu().tolist()[:2]         # the one copy of four integers
        em = pl.step(n_new, end, self.f_lo, self.f_hi)
        n_keep = h0 + n_held + n_new - em.keep_from
        if (into is None and n_held == 0 and n_keep == 0 and em.n_zero == 0 and em.e0 == h0 and em.e1 == h0 + n_new
                and (em.fade_in_at < 0 or em.fade_in_at + pl.F <= em.e0) and em.fade_out_end < 0):
            return x
        if into is None:
            dst = torch.empty(em.n_out, dtype=torch.float32, device=self.device)
        else:
            dst = into[0][into[1]:into[1] + em.n_out]
            assert dst.dtype == torch.float32 and dst.dim() == 1 and dst.numel() == em.n_out and dst.is_cuda
        if n_keep and (self.spare is None or self.spare.numel() < n_keep):
            self.spare = torch.empty(max(2 * n_keep, 4096), dtype=torch.float32, device=self.device)
        ft = fade_table_dev(self.device, pl.F)
        a = WaveEmit(self.held.data_ptr() if n_held else None, x.data_ptr() if n_new else None, None if ft is None else ft.data_ptr(),
                     dst.data_ptr() if em.n_out else None, self.spare.data_ptr() if n_keep else None, h0, n_held, n_new, em.e0, em.e1,
                     em.fade_in_at, em.fade_out_end, pl.F, em.n_zero, em.keep_from, self.spare.numel() if n_keep else 0, 0)
        L.check(lib.cv2_wave_emit_chunk(self.state.data_ptr(), C.byref(a), L.stream_ptr()))
        self.launches += 1
        if n_keep:
            self.held, self.spare = self.spare, self.held
        return dst
