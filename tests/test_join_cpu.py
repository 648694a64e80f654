"""Joined calls without a GPU: the planner of cv2amd/join.py against the numpy restatement of the definitions
(tests/_join.py), the accepted ranges, the composition of the .joined() view with the other views, the refusal of stream=True before the
model is touched, and the FastAPI server's `pause_ms` / `trim_db` / `fade_ms` fields."""
import importlib.util
import os

import numpy as np
import pytest
import torch

import _join as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'cosyvoice2-eu_amd')


def test_planner_arithmetic_on_random_lengths():
    from cv2amd.join import Join, plan, fade_table, FADE_IN, FADE_OUT
    rng = np.random.default_rng(5)
    for trial in range(200):
        k = int(rng.integers(1, 12))
        lengths = [int(rng.integers(1, 3000)) for _ in range(k)]
        trim = bool(trial % 2)
        pause_ms = [0, 1 / 24, 0.125, 7.3, 150][trial % 5]
        fade_ms = [0, 1 / 24, 5, 20][trial % 4]
        j = Join(pause_ms=pause_ms, trim_db=40 if trim else None, fade_ms=fade_ms if trim else None)
        bnds = None
        if trim:
            bnds = []
            for n in lengths:
                a = int(rng.integers(0, n + 1))
                bnds.append((a, int(rng.integers(a, n + 1))))
        pause, F = R.samples(pause_ms), (R.samples(fade_ms) if trim else 0)
        assert j.check().resolve()[:2] == (pause, F)
        want_p, want_n, want_s = R.plan(lengths, bnds or [(0, n) for n in lengths], pause, F)
        pieces, n, spans = plan(lengths, bnds, j)
        assert n == want_n and spans == want_s
        assert pieces == [(a, m, off, (FADE_IN if fi else 0) | (FADE_OUT if fo else 0)) for a, m, off, fi, fo in want_p]
        assert n == sum(m for _, m, _, _ in pieces) + (k - 1) * pause
    # defaults: 150 ms once anything is set, 5 ms fades with a trim, none without; g is the float32 of the float64 power
    assert Join(trim_db=40).resolve() == (3600, 120, float(R.gain(40)))
    assert Join(pause_ms=0).resolve() == (0, 0, None)
    assert Join(fade_ms=0, trim_db=33.5).resolve() == (3600, 0, float(R.gain(33.5)))
    for F in (1, 2, 120, 480):
        t = fade_table(F)
        assert t.dtype == np.float32 and np.array_equal(t, R.fade_table(F)) and 0 < t[0] <= t[-1] < 1 and np.all(np.diff(t) >= 0)
    with pytest.raises(ValueError):
        plan([10, 10], [(0, 10), (4, 11)], Join(trim_db=40))
    with pytest.raises(ValueError):
        plan([1] * 257, None, Join(pause_ms=0))


def test_ranges():
    from cv2amd.join import Join
    for ok in (dict(pause_ms=0), dict(pause_ms=5000), dict(trim_db=20), dict(trim_db=80, fade_ms=20), dict(trim_db=45.5, fade_ms=0, pause_ms=12.5)):
        assert Join(**ok).check() is not None
    for bad in (dict(pause_ms=-1), dict(pause_ms=5000.5), dict(trim_db=19.9), dict(trim_db=81), dict(trim_db=40, fade_ms=21), dict(trim_db=40, fade_ms=-1),
                dict(pause_ms=float('nan')), dict(trim_db=float('inf')), dict(pause_ms=True), dict(pause_ms='150'), dict(fade_ms=5), dict(fade_ms=0, pause_ms=100)):
        with pytest.raises(ValueError):
            Join(**bad).check()
    assert Join().is_default() and not Join(pause_ms=0).is_default()
    assert Join(pause_ms=10).replace(trim_db=30) == Join(pause_ms=10, trim_db=30) and Join(pause_ms=10).replace(pause_ms=None) == Join(pause_ms=10)


class _Model:
    """stands where CosyVoice2.model does: records what it was given"""

    def __init__(self):
        self.calls, self.joined_calls = [], []

    def tts(self, **kw):
        self.calls.append(kw)
        yield {'tts_speech': torch.full((1, 4), 0.25)}

    def tts_joined(self, inputs, join, **kw):
        self.joined_calls.append((inputs, join, kw))
        yield {'tts_speech': torch.full((1, 8), 0.25), 'segments': [(0, 4), (4, 8)]}


class _FrontEnd:
    def __init__(self, segments=None):
        self.segments, self.touched = segments, 0

    def text_normalize(self, text, split=True, **kw):
        self.touched += 1
        if not isinstance(text, str):
            return [text]
        return (list(self.segments) if self.segments else [text]) if split else text

    def frontend_zero_shot(self, text, *a, **kw):
        self.touched += 1
        return {'text': text}

    frontend_cross_lingual = frontend_instruct2 = frontend_sft = frontend_zero_shot


def _cv(segments=None, cls=None):
    from cosyvoice.cli.cosyvoice import CosyVoice2
    cls = cls or CosyVoice2
    cv = cls.__new__(cls)
    cv.output_sample_rate, cv.output_pcm16, cv.model_sample_rate, cv.sampling = None, False, 24000, None
    cv.model, cv.frontend = _Model(), _FrontEnd(segments)
    return cv


def test_view_composition_and_nothing_set():
    from cv2amd.join import Join
    from cv2amd.sampling import Sampling
    from cv2amd.solver import Solver
    cv = _cv()
    assert cv.join is None and cv.joined().join is None                      # nothing set: the object's own path
    v = cv.joined(pause_ms=200, trim_db=40).sampler(seed=7).output(sample_rate=16000, pcm16=True).solver(steps=6)
    assert v.join == Join(pause_ms=200, trim_db=40) and v.sampling == Sampling(seed=7) and (v.output_sample_rate, v.output_pcm16) == (16000, True)
    assert v.flow_solver == Solver(steps=6) and v.model is cv.model and cv.join is None
    w = cv.sampler(seed=7).output(sample_rate=16000).joined(pause_ms=0)
    assert w.join == Join(pause_ms=0) and w.sampling == Sampling(seed=7) and w.output_sample_rate == 16000
    assert v.joined(fade_ms=10).join == Join(pause_ms=200, trim_db=40, fade_ms=10) and v.joined().join == v.join
    for bad in (dict(pause_ms=-1), dict(trim_db=10), dict(fade_ms=5), dict(trim_db=40, fade_ms=30)):
        with pytest.raises(ValueError):
            cv.joined(**bad)
    from cosyvoice2_eu import Cosy2EU
    eu = Cosy2EU(cv).joined(pause_ms=100).sampler(seed=3)
    assert eu._model.join == Join(pause_ms=100) and eu._model.sampling == Sampling(seed=3) and eu._model.model is cv.model


def test_joined_view_routes_segments_and_refuses_streaming():
    from cv2amd.join import Join
    from cv2amd.sampling import Sampling
    cv = _cv(segments=('un', 'deux', 'trois'))
    j = cv.joined(pause_ms=100).sampler(seed=9).output(sample_rate=16000)
    for call in (lambda c, **k: c.inference_zero_shot('x', 'p', None, **k), lambda c, **k: c.inference_cross_lingual('x', None, **k),
                 lambda c, **k: c.inference_instruct2('x', 'i', None, **k), lambda c, **k: c.inference_sft('x', 'spk', **k)):
        cv.frontend.touched = 0
        with pytest.raises(ValueError):
            next(call(j, stream=True))
        assert cv.frontend.touched == 0 and cv.model.calls == [] and cv.model.joined_calls == []      # before any work
        (out,) = list(call(j))
        assert out['segments'] == [(0, 4), (4, 8)]
        inputs, join, kw = cv.model.joined_calls.pop()
        assert [i['text'] for i in inputs] == ['un', 'deux', 'trois'] and join == Join(pause_ms=100)
        assert kw['sampling'] == [Sampling(seed=9).for_segment(i) for i in range(3)] and [s.stream for s in kw['sampling']] == [0, 1, 2]
        assert kw['output_sample_rate'] == 16000 and kw['speed'] == 1.0 and cv.model.calls == []
    # the plain view of the same object: one tts() per segment, as before
    assert len(list(cv.inference_zero_shot('x', 'p', None))) == 3 and len(cv.model.calls) == 3 and cv.model.joined_calls == []
    # one segment, or a generator text: exactly the existing path
    one = _cv()
    assert len(list(one.joined(pause_ms=100).inference_zero_shot('x', 'p', None))) == 1
    gen = (t for t in ('a', 'b'))
    assert len(list(one.joined(pause_ms=100).inference_zero_shot(gen, 'p', None))) == 1
    assert len(one.model.calls) == 2 and one.model.joined_calls == [] and one.model.calls[1]['text'] is gen
    # voice conversion is unaffected
    one.frontend.frontend_vc = lambda *a: {}
    assert len(list(one.joined(pause_ms=100).inference_vc(None, None))) == 1 and one.model.joined_calls == []


def _server():
    spec = importlib.util.spec_from_file_location('cv2_fastapi_server_join', os.path.join(PKG, 'runtime', 'python', 'fastapi', 'server.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_request_fields_reach_the_view_and_bad_values_answer_422():
    fastapi = pytest.importorskip('fastapi')
    from cv2amd.join import Join
    from cv2amd.sampling import Sampling
    srv = _server()
    cv = _cv()
    assert srv.request_view(cv) is cv
    v = srv.request_view(cv, pause_ms=250.0, trim_db=40.0, fade_ms=3.0)
    assert v is not cv and v.model is cv.model and v.join == Join(pause_ms=250.0, trim_db=40.0, fade_ms=3.0)
    w = srv.request_view(cv, 16000, seed=9, pause_ms=0.0)                      # composes with the rate and the sampler fields
    assert w.output_sample_rate == 16000 and w.sampling == Sampling(seed=9) and w.join == Join(pause_ms=0.0)
    assert srv.request_view(cv, seed=9).join is None
    for bad in (dict(pause_ms=-1.0), dict(pause_ms=6000.0), dict(trim_db=10.0), dict(trim_db=90.0), dict(fade_ms=5.0), dict(trim_db=40.0, fade_ms=25.0)):
        with pytest.raises(fastapi.HTTPException) as e:
            srv.request_view(cv, **bad)
        assert e.value.status_code == 422 and e.value.detail, bad
    assert cv.model.calls == [] and cv.model.joined_calls == []


def test_form_fields_over_http():
    pytest.importorskip('fastapi')
    pytest.importorskip('httpx')
    try:
        import python_multipart  # noqa: F401
    except ImportError:
        pytest.importorskip('multipart')
    from fastapi.testclient import TestClient
    from cv2amd.join import Join
    srv = _server()
    cv = _cv(segments=('un', 'deux'))
    client = TestClient(srv.build_app(cv))
    r = client.post('/inference_sft', data=dict(tts_text='bonjour', spk_id='fr', pause_ms='200', trim_db='40'))
    assert r.status_code == 200 and len(r.content) == 16                      # ONE waveform of 8 samples as int16
    assert cv.model.joined_calls[0][1] == Join(pause_ms=200.0, trim_db=40.0) and cv.model.calls == []
    r = client.post('/inference_sft', data=dict(tts_text='bonjour', spk_id='fr'))
    assert r.status_code == 200 and len(cv.model.calls) == 2 and len(cv.model.joined_calls) == 1
    for bad in (dict(pause_ms='-1'), dict(trim_db='5'), dict(fade_ms='5'), dict(pause_ms='x')):
        assert client.post('/inference_sft', data=dict(tts_text='bonjour', spk_id='fr', **bad)).status_code == 422
    assert len(cv.model.calls) == 2 and len(cv.model.joined_calls) == 1
