"""Sampler settings and seed of ONE call (an extension: the reference has one ras_sampling configuration per model, conf/cosyvoice2.yaml:33-37,
and draws from the process-wide torch RNG).

A `Sampling` value travels with a call from the public surface (CosyVoice2.sampler(...)) to the three places that start LLM requests and to
every vocoder invocation of the call.  Its device form is the slot's cv2_llm_sampling record (include/cv2_amd.h): k_sample keys every Philox
draw of a slot that has one with (stream, step, trial, 0) under the call's seed, where `stream` is the index of the text segment inside the
call -- never the slot, the row of the launch or a counter of earlier calls.  A call with settings but NO seed runs under the model's counter
seed, which the calls started beside it share: the engine writes stream = slot into its record (LLMEngine._record), the keying of a call
without a record, so that such calls never repeat each other's draws.  The vocoder's noise seed of chunk c of segment s is
hift_seed(seed, s, c).  Pure Python: the CPU tests import it without a device.
"""
import math
import struct

from . import philox

DEFAULTS = dict(top_p=0.8, top_k=25, win_size=10, tau_r=0.1)       # conf/cosyvoice2.yaml:33-37, what cv2_llm_create selects for top_k == 0
FIELDS = ('seed', 'temperature', 'top_p', 'top_k', 'win_size', 'tau_r', 'greedy')
HIFT_TAG = 0x48694654                                              # 'HiFT': keeps the vocoder's counters apart from the sampler's (word 3 = 0 there)


def f32(x):
    """x rounded to float32 (round to nearest even), as a Python float"""
    return struct.unpack('<f', struct.pack('<f', x))[0]


def f32_bits(x):
    """bit pattern of float32(x)"""
    return struct.unpack('<I', struct.pack('<f', x))[0]


def f32_mul(a, b):
    """the fp32 product of two float32 values: the exact product fits a double (24 + 24 bits), so one rounding to float32 remains"""
    return f32(f32(a) * f32(b))


def hift_seed(seed, segment, chunk):
    """64-bit noise seed of vocoder invocation `chunk` (0, 1, 2, ... of a streaming call; 0 otherwise) of text segment `segment` of a call
    seeded with `seed`: words 0 and 1 of Philox4x32-10((chunk, segment, 'HiFT', 0), key = seed)."""
    r = philox.philox4x32((chunk & philox.MASK, segment & philox.MASK, HIFT_TAG, 0), (seed & philox.MASK, (seed >> 32) & philox.MASK))
    return r[0] | (r[1] << 32)


class Sampling:
    """seed, temperature, top_p, top_k, win_size, tau_r, greedy: None = the engine's (its yaml constants, the model's counter seed and mode).
    `stream` is not a setting: it numbers the text segments of one call (0 .. k-1) so that they do not repeat each other's draws."""
    __slots__ = FIELDS + ('stream',)

    def __init__(self, seed=None, temperature=None, top_p=None, top_k=None, win_size=None, tau_r=None, greedy=None, stream=0):
        self.seed, self.temperature, self.top_p, self.top_k, self.win_size, self.tau_r, self.greedy = seed, temperature, top_p, top_k, win_size, tau_r, greedy
        self.stream = stream

    def __repr__(self):
        return 'Sampling(' + ', '.join(f'{k}={getattr(self, k)!r}' for k in FIELDS if getattr(self, k) is not None) + ')'

    def __eq__(self, o):
        return isinstance(o, Sampling) and all(getattr(self, k) == getattr(o, k) for k in self.__slots__)

    def is_default(self):
        """nothing set: no record is written, CV2_ST_SAMP stays 0 and the model's counter seed is used"""
        return all(getattr(self, k) is None for k in FIELDS)

    def replace(self, **kw):
        """a copy with the given (non-None) fields replaced"""
        d = {k: getattr(self, k) for k in self.__slots__}
        d.update({k: v for k, v in kw.items() if v is not None})
        return Sampling(**d)

    def for_segment(self, i):
        s = self.replace()
        s.stream = i
        return s

    def check(self):
        """ValueError for anything outside the accepted ranges (before any work); returns self"""
        def num(name, v, integer=False):
            if isinstance(v, bool) or not isinstance(v, (int,) if integer else (int, float)) or (not integer and not math.isfinite(v)):
                raise ValueError(f'sampling: {name} must be {"an integer" if integer else "a finite number"}, got {v!r}')
        if self.seed is not None:
            num('seed', self.seed, True)
            if not 0 <= self.seed < 1 << 64:
                raise ValueError(f'sampling: seed {self.seed} outside 0 .. 2**64 - 1')
        if self.temperature is not None:
            num('temperature', self.temperature)
            if not 0.05 <= self.temperature <= 10:
                raise ValueError(f'sampling: temperature {self.temperature} outside 0.05 .. 10')
        if self.top_p is not None:
            num('top_p', self.top_p)
            if not 0 < self.top_p <= 1:
                raise ValueError(f'sampling: top_p {self.top_p} outside (0, 1]')
        if self.top_k is not None:
            num('top_k', self.top_k, True)
            if not 1 <= self.top_k <= 25:
                raise ValueError(f'sampling: top_k {self.top_k} outside 1 .. 25')
        if self.win_size is not None:
            num('win_size', self.win_size, True)
            if not 1 <= self.win_size <= 64:
                raise ValueError(f'sampling: win_size {self.win_size} outside 1 .. 64')
        if self.tau_r is not None:
            num('tau_r', self.tau_r)
            if self.tau_r < 0:
                raise ValueError(f'sampling: tau_r {self.tau_r} is negative')
        if self.greedy is not None and not isinstance(self.greedy, bool):
            raise ValueError(f'sampling: greedy must be True, False or None, got {self.greedy!r}')
        return self

    def record(self, defaults=None, stream=None):
        """The fields of the slot's cv2_llm_sampling record as a dict: unset fields from `defaults` (the engine's yaml constants: a dict with
        top_p / top_k / win_size / tau_r), inv_temp = float32(1 / temperature) and rep_thr = (float)win_size * (float)tau_r formed in fp32 as
        cv2_llm_create forms the engine's, stream = Philox counter word 0."""
        d = dict(DEFAULTS)
        d.update({k: v for k, v in (defaults or {}).items() if k in DEFAULTS and v is not None})
        top_p = self.top_p if self.top_p is not None else d['top_p']
        top_k = self.top_k if self.top_k is not None else d['top_k']
        win = self.win_size if self.win_size is not None else d['win_size']
        tau = self.tau_r if self.tau_r is not None else d['tau_r']
        temp = self.temperature if self.temperature is not None else 1.0
        return dict(inv_temp=f32(1.0 / temp), top_p=f32(top_p), top_k=int(top_k), win_size=int(win), rep_thr=f32_mul(float(win), tau),
                    stream=(self.stream if stream is None else stream) & 0xFFFFFFFF)
