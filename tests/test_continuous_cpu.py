"""Continuous calls without a GPU: the numpy restatement of the causal gate (tests/_join_stream.py), the planner of
cv2amd/join.py (StreamPlan) fed random chunkings against it, the accepted ranges, the composition of the .continuous() view with the other
views, the refusals before the model is touched, and the FastAPI server's `continuous` field."""
import importlib.util
import os
import re

import numpy as np
import pytest
import torch

import _join as R
import _join_stream as RS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'cosyvoice2-eu_amd')


def crafted(rng, n, quiet=1e-4, loud=0.3, spans=()):
    x = (rng.standard_normal(n) * quiet).astype(np.float32)
    for lo, hi in spans:
        x[lo:hi] = (rng.standard_normal(hi - lo) * loud).astype(np.float32)
    return x


def run_plan(segs, join, cuts):
    """StreamPlan over the segments cut at cuts[i] (ascending positions inside segment i), the device's record taken from the restatement
    and the emit applied in numpy -> (the stream, spans, [(segment, samples seen, ended, samples out so far)], the largest held count)"""
    from cv2amd.join import StreamPlan
    pl = StreamPlan(join, len(segs))
    w = RS.fade_table(pl.F)
    C = RS.carries(segs)
    out, log, held_max = [], [], 0
    for i, s in enumerate(segs):
        edges = [0] + [c for c in cuts[i] if 0 < c < len(s)] + [len(s)]
        for lo, hi in zip(edges[:-1], edges[1:]):
            end = hi == len(s)
            f_lo = f_hi = -1
            fr = pl.gate_range(hi - lo, end)
            if fr is not None:
                assert fr[0] * RS.FRAME >= pl.e                               # every frame still to analyse is held or new
                loud = RS.loud_frames(s, C[i], pl.g, hi, end)
                assert all(f < fr[1] for f in loud)
                if loud:
                    f_lo, f_hi = loud[0], loud[-1]
            h0 = pl.e
            em = pl.step(hi - lo, end, f_lo, f_hi)
            assert h0 <= em.e0 <= em.e1 <= em.keep_from <= hi
            x = np.array(s[em.e0:em.e1], copy=True)
            for q in range(em.e0, em.e1):
                if em.fade_in_at >= 0 and em.fade_in_at <= q < em.fade_in_at + pl.F:
                    x[q - em.e0] = x[q - em.e0] * w[q - em.fade_in_at]
                elif em.fade_out_end >= 0 and em.fade_out_end - pl.F <= q < em.fade_out_end:
                    x[q - em.e0] = x[q - em.e0] * w[em.fade_out_end - 1 - q]
            out += [x, np.zeros(em.n_zero, np.float32)]
            held_max = max(held_max, hi - em.keep_from)
            log.append((i, hi, end, sum(o.size for o in out)))
    assert pl.done
    return np.concatenate(out), pl.spans, log, held_max


def test_the_gate_is_causal_and_carries_the_loudest_sample_forward():
    rng = np.random.default_rng(3)
    g = RS.gain(40)
    a = crafted(rng, 4000, spans=[(1000, 3000)])
    b = crafted(rng, 3000, quiet=1e-8, loud=1e-4, spans=[(700, 1500)])        # quieter than 40 dB below segment a's peak: nothing of it is loud
    c = crafted(rng, 5000, spans=[(2400, 2700)])
    bn = RS.bounds([a, b, c], g)
    assert bn[0] == (0, 240 * 13 + 480) and bn[1] == (0, 3000) and bn[2] == (240 * 10 - 480, 5000)
    assert R.bounds([a, b, c], g)[1] != bn[1]                                  # (the .joined() trim, relative to b's own peak, does cut b)
    assert RS.carries([a, b, c])[1] == np.abs(a).max() == RS.carries([a, b, c])[2]
    # a frame is judged against the running maximum up to ITSELF: a soft start is loud until something louder has been heard
    s = np.concatenate([np.full(480, 1e-3, np.float32), np.zeros(480, np.float32), np.full(480, 0.5, np.float32), np.full(240, 1e-3, np.float32)])
    assert RS.loud_frames(s, 0, g) == [0, 1, 4, 5] and RS.loud_frames(s, 0, g, 1000, ended=False) == [0, 1]
    assert RS.loud_frames(np.zeros(500, np.float32), 0, g) == [] and RS.loud_frames(np.array([np.nan, 0.1], np.float32), 0, g) == [0]
    assert RS.bounds([a, b, c], None) == [(0, 4000), (0, 3000), (0, 5000)]


def test_planner_reproduces_the_restatement_under_random_chunkings():
    from cv2amd.join import Join
    rng = np.random.default_rng(17)
    for trial in range(120):
        k = int(rng.integers(2, 6))
        segs = []
        for _ in range(k):
            n = int(rng.integers(1, 4000))
            kind = trial % 4 if len(segs) != 1 else int(rng.integers(0, 5))
            if kind == 4:
                segs.append(np.zeros(n, np.float32))
                continue
            lo = int(rng.integers(0, n))
            hi = int(rng.integers(lo, n + 1))
            spans = [(lo, hi)] + ([(min(n, hi + 800), min(n, hi + 900))] if kind == 2 else [])
            segs.append(crafted(rng, n, spans=spans))
        trim = trial % 3 != 0
        join = Join(pause_ms=[0, 1 / 24, 7.3, 150][trial % 4], trim_db=[26.5, 40, 60][trial % 3] if trim else None,
                    fade_ms=[0, 1 / 24, 2.5, 5][(trial // 2) % 4] if trim else None)
        pause, F, g = join.resolve()
        want, spans = RS.stream(segs, None if g is None else np.float32(g), pause, F)
        for mode in range(3):
            if mode == 0:
                cuts = [[] for _ in segs]
            elif mode == 1:
                cuts = [sorted(set(rng.integers(1, max(2, len(s)), size=int(rng.integers(1, 12))).tolist())) for s in segs]
            else:
                cuts = [list(range(239, len(s), 240)) if j % 2 else list(range(241, len(s), 241)) for j, s in enumerate(segs)]
            got, got_spans, log, _held = run_plan(segs, join, cuts)
            assert got_spans == spans, (trial, mode)
            assert got.size == want.size and np.array_equal(got.view(np.int32), want.view(np.int32)), (trial, mode)
            for i, n, ended, n_out in log:
                assert n_out == RS.emitted(segs, None if g is None else np.float32(g), pause, F, i, n, ended), (trial, mode, i, n)


def test_a_loud_frame_waits_for_its_own_frame_only_and_the_quiet_tail_is_held():
    from cv2amd.join import Join
    rng = np.random.default_rng(2)
    a = crafted(rng, 4800, spans=[(0, 2400)])                                 # loud frames 0 .. 9, then 10 quiet frames
    b = crafted(rng, 2400, spans=[(0, 2400)])
    join = Join(pause_ms=0, trim_db=40)                                       # F = 120
    _, _, log, held = run_plan([a, b], join, [[2399, 2400, 2401, 4000], []])
    assert [n_out for *_x, n_out in log[:4]] == [240 * 9 - 120, 2400 - 120, 2400 - 120, 2400 - 120]
    assert log[4][3] == 2400 + 480 and held == 4000 - (2400 - 120)           # the tail: cut 480 behind frame 9, faded, at the segment's end


def test_ranges_and_refusals():
    from cv2amd.join import Join, StreamPlan, check_continuous
    for ok in (dict(pause_ms=0), dict(pause_ms=5000), dict(trim_db=20), dict(trim_db=80, fade_ms=5), dict(trim_db=45.5, fade_ms=0, pause_ms=12.5)):
        assert check_continuous(Join(**ok)) is not None
    for bad in (dict(pause_ms=-1), dict(pause_ms=5000.5), dict(trim_db=19.9), dict(trim_db=81), dict(trim_db=40, fade_ms=5.01), dict(trim_db=40, fade_ms=20),
                dict(trim_db=40, fade_ms=-1), dict(pause_ms=float('nan')), dict(pause_ms=True), dict(fade_ms=5), dict(fade_ms=0, pause_ms=100)):
        with pytest.raises(ValueError):
            check_continuous(Join(**bad))
    assert StreamPlan(Join(trim_db=40), 2).F == 120 and StreamPlan(Join(pause_ms=1), 2).pause == 24
    for k in (0, 1, 257):
        with pytest.raises(ValueError):
            StreamPlan(Join(pause_ms=0), k)
    pl = StreamPlan(Join(pause_ms=0), 2)
    pl.step(10, True)
    pl.step(10, True)
    with pytest.raises(ValueError):
        pl.step(1, False)


class _Model:
    def __init__(self):
        self.calls = []

    def tts(self, **kw):
        self.calls.append(('tts', kw))
        yield {'tts_speech': torch.zeros(1, 10)}

    def tts_continuous(self, inputs, join, **kw):
        self.calls.append(('continuous', len(inputs), join, kw))
        yield {'tts_speech': torch.zeros(1, 10), 'segment': 0, 'segments': [(0, 10)]}

    def tts_joined(self, inputs, join, **kw):
        self.calls.append(('joined', len(inputs), join, kw))
        yield {'tts_speech': torch.zeros(1, 10), 'segments': [(0, 10)]}


def _cv(segments=('un', 'deux', 'trois')):
    from cosyvoice.cli.cosyvoice import CosyVoice2
    from cosyvoice.cli.frontend import PrecomputedFrontEnd

    class FE(PrecomputedFrontEnd):
        def text_normalize(self, text, split=True, **kw):
            return list(segments) if split else text

        def frontend_zero_shot(self, text, *a, **kw):
            return {'text': torch.zeros(1, 3, dtype=torch.int32)}
    cv = CosyVoice2.__new__(CosyVoice2)
    cv.output_sample_rate, cv.output_pcm16, cv.model_sample_rate, cv.sampling, cv.model_dir, cv.fp16 = None, False, 24000, None, 'unused', False
    cv.model, cv.frontend = _Model(), FE(lambda t: [1, 2, 3], {})
    return cv


def test_the_view_composes_and_refuses_before_the_model_is_touched():
    from cv2amd.join import Join
    from cv2amd.sampling import Sampling
    from cv2amd.solver import Solver
    cv = _cv()
    assert cv.continuous() is not cv and cv.continuous().stream_join is None  # nothing set: the plain object's behaviour
    list(cv.continuous().inference_zero_shot('x', 'p', None, stream=True))
    assert [c[0] for c in cv.model.calls] == ['tts'] * 3
    del cv.model.calls[:]
    v = cv.continuous(trim_db=40).sampler(seed=7).solver(steps=6).output(sample_rate=16000, pcm16=True).continuous(pause_ms=20)
    assert v.stream_join == Join(pause_ms=20, trim_db=40) and v.join is None
    out = list(v.inference_zero_shot('x', 'p', None, stream=True))
    (kind, n, join, kw), = cv.model.calls
    assert kind == 'continuous' and n == 3 and join == Join(pause_ms=20, trim_db=40) and out[0]['segments'] == [(0, 10)]
    assert kw['sampling'] == [Sampling(seed=7).for_segment(i) for i in range(3)] and kw['solver'] == Solver(steps=6)
    assert kw['output_sample_rate'] == 16000 and kw['pcm16'] is True and kw['speed'] == 1.0
    del cv.model.calls[:]
    with pytest.raises(ValueError, match=r'\.joined\(\)'):                     # stream=False: refused, naming the view that yields one waveform
        next(v.inference_zero_shot('x', 'p', None))
    for bad in (dict(fade_ms=5), dict(trim_db=40, fade_ms=6), dict(pause_ms=-1), dict(trim_db=10)):
        with pytest.raises(ValueError):
            cv.continuous(**bad)
    assert cv.model.calls == []
    # one view is joined or continuous: the later request holds
    j = cv.continuous(pause_ms=5).joined(pause_ms=9)
    assert j.join == Join(pause_ms=9) and j.stream_join is None
    list(j.inference_zero_shot('x', 'p', None))
    assert cv.model.calls[0][0] == 'joined'
    # a text of one segment and a generator text take the plain streaming path
    one = _cv(segments=('un',)).continuous(pause_ms=20)
    list(one.inference_zero_shot('x', 'p', None, stream=True))
    assert [c[0] for c in one.model.calls] == ['tts']
    from cosyvoice2_eu import Cosy2EU
    assert Cosy2EU(cv).continuous(trim_db=30)._model.stream_join == Join(trim_db=30)


def test_the_header_declares_the_entry_points_and_the_abi_revision_stays():
    from cv2amd import lib as L
    from cv2amd import join as J
    import ctypes as C
    hdr = open(os.path.join(ROOT, 'include', 'cv2_amd.h')).read()
    for name in ('cv2_wave_gate_chunk', 'cv2_wave_emit_chunk'):
        assert re.search(r'\bint %s\(' % name, hdr) and name in L.EXPORTS
    assert C.sizeof(J.WaveState) == 32 and C.sizeof(J.WaveEmit) == 88
    assert re.search(r'#define\s+CV2_ABI_VERSION\s+3\b', hdr) and L.ABI_VERSION == 3


def test_the_server_field_selects_the_continuous_view():
    pytest.importorskip('fastapi')
    from cv2amd.join import Join
    spec = importlib.util.spec_from_file_location('cv2_fastapi_server_cont', os.path.join(PKG, 'runtime', 'python', 'fastapi', 'server.py'))
    srv = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(srv)
    cv = _cv()
    assert srv.request_view(cv) is cv
    v = srv.request_view(cv, pause_ms=30, trim_db=40, continuous=True)
    assert v.stream_join == Join(pause_ms=30, trim_db=40) and v.join is None
    assert srv.request_view(cv, continuous=True).stream_join == Join(pause_ms=150)
    assert srv.request_view(cv, pause_ms=30, continuous=False).join == Join(pause_ms=30)
    from fastapi import HTTPException
    with pytest.raises(HTTPException) as e:
        srv.request_view(cv, trim_db=40, fade_ms=10, continuous=True)         # (a fade the joined view takes, the continuous one does not)
    assert e.value.status_code == 422
