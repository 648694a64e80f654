"""The output level stage without a GPU: the integer planner (cv2amd/level.py) against the restatement's own counting, the settings and
the .level() view (ranges, composition, the plain object when nothing is set, no peak target on a stream), the FastAPI form fields, and the
properties of the numpy restatement of the definition (tests/_level.py) that the device tests then hold the kernel to."""
import importlib.util
import math
import os
import struct

import numpy as np
import pytest
import torch

import _level as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'cosyvoice2-eu_amd')


# ---- the planner ---------------------------------------------------------------------------------------------------------------------
def _plan_all(L, chunks):
    from cv2amd import level as LV
    st, log = LV.LevelState(L), []
    for k, n_new in enumerate(chunks):
        final = k == len(chunks) - 1
        n0, n_emit, first_needed = LV.plan(st, n_new, final)
        assert n0 == st.emitted and n_emit >= 0 and st.first <= first_needed <= st.consumed + n_new
        assert first_needed <= max(0, n0 + n_emit - L) or final, 'a retained sample a later output reads was dropped'
        if not final:
            assert n0 + n_emit - 1 + L <= st.consumed + n_new - 1 or n_emit == 0
            assert n0 + n_emit + L > st.consumed + n_new - 1, 'a sample that could go out was held back'
        st.commit(n_new, n_emit, first_needed, final)
        assert st.n_tail <= 2 * L
        log.append((n0, n_emit, st.first, st.consumed, st.n_tail))
    return st, log


def _random_chunks(rng, n, L):
    out, left = [], n
    while left:
        kind = rng.integers(0, 5)
        c = (0, 1, int(rng.integers(1, L)), 480 * int(rng.integers(1, 4)), int(rng.integers(1, 3000)))[kind]
        c = min(c, left)
        out.append(c)
        left -= c
    if out[-1] == 0:
        out.append(0)
    return out


@pytest.mark.parametrize('L', R.LOOKAHEADS)
def test_planner(L):
    from cv2amd import level as LV
    rng = np.random.default_rng(L)
    for n in (1, L, L + 1, 2 * L + 1, 4803, 24000):
        for trial in range(6):
            chunks = _random_chunks(rng, n, L) if trial else [n]
            if chunks[-1] == 0 and len(chunks) > 1:                            # (an empty final chunk is legal: it flushes what was held back)
                pass
            st, log = _plan_all(L, chunks)
            assert st.emitted == st.consumed == n == sum(e for _n0, e, *_ in log) and st.final and st.n_tail == 0
            assert log[-1][1] > 0, 'the last chunk is never empty'
            # the same integers as the restatement's own counting
            _y, want = R.stream64(np.zeros(n, dtype=np.float32), 1.0, 0.5, L, chunks)
            assert [(a, b, d, e) for a, b, _c, d, e in want] == [(a, b, d, e) for a, b, _c, d, e in log]
            # plans do not depend on the chunking: after the same number of samples, the same number emitted and the same retained
            for n0, n_emit, first, consumed, n_tail in log[:-1]:
                assert n0 + n_emit == max(0, consumed - L) and first == max(0, n0 + n_emit - L)
    st = LV.LevelState(24)
    with pytest.raises(ValueError):
        LV.plan(st, -1, False)
    st.commit(*((10,) + LV.plan(st, 10, True)[1:]), final=True)
    with pytest.raises(ValueError):
        LV.plan(st, 1, False)
    for bad in (23, 241, 24.0, True):
        with pytest.raises(ValueError):
            LV.LevelState(bad)


def test_settings():
    from cv2amd.level import Level, check, window
    assert Level().is_default() and check(None) is None and check(Level()) is None
    G, c, L, T = Level(gain_db=6).resolve()
    assert (G, c, L, T) == (float(R.db(6)), float(R.db(-1)), 120, None), 'ceiling -1 dBFS and 5 ms once any field is set'
    assert Level(lookahead_ms=1).resolve()[2] == 24 and Level(lookahead_ms=10).resolve()[2] == 240 and Level(lookahead_ms=2.5).resolve()[2] == 60
    G, c, L, T = Level(peak_db=-3, ceiling_db=-3, lookahead_ms=1).resolve()
    assert G == 1.0 and T == c == float(R.db(-3)) and L == 24
    for bad in (dict(gain_db=24.1), dict(gain_db=-25), dict(ceiling_db=0.1), dict(ceiling_db=-12.5), dict(lookahead_ms=0.9), dict(lookahead_ms=10.5),
                dict(peak_db=0.5), dict(peak_db=-24.5), dict(peak_db=-0.5), dict(peak_db=-3, ceiling_db=-4), dict(gain_db=float('nan')),
                dict(gain_db=True), dict(ceiling_db='-1'), dict(lookahead_ms=float('inf'))):
        with pytest.raises(ValueError):
            Level(**bad).check()
    assert Level(peak_db=-1).check() and Level(peak_db=0, ceiling_db=0).check()       # (the default ceiling is -1: a peak of -1 is the most it takes)
    with pytest.raises(ValueError):
        check(Level(peak_db=-6), stream=True)
    assert check(Level(gain_db=-6), stream=True) == Level(gain_db=-6) and check(Level(peak_db=-6)) == Level(peak_db=-6)
    for L in R.LOOKAHEADS:
        w64, w32 = R.weights(L)
        assert np.array_equal(np.asarray(window(L)).astype(np.float32), w32) and abs(math.fsum(window(L)) - 1) < 1e-15 and (w32 > 0).all()


# ---- the view ------------------------------------------------------------------------------------------------------------------------
class _Model:
    def __init__(self):
        self.calls = []

    def tts(self, **kw):
        self.calls.append(('tts', kw))
        yield {'tts_speech': torch.full((1, 4), 0.25)}

    def tts_joined(self, inputs, join, **kw):
        self.calls.append(('joined', kw))
        yield {'tts_speech': torch.full((1, 4), 0.25), 'segments': []}

    def tts_continuous(self, inputs, join, **kw):
        self.calls.append(('continuous', kw))
        yield {'tts_speech': torch.full((1, 4), 0.25), 'segment': 0, 'segments': []}


def _cv(segments=('un', 'deux')):
    from cosyvoice.cli.cosyvoice import CosyVoice2

    class FE:
        def text_normalize(self, text, split=True, **kw):
            return list(segments) if split else text

        def frontend_zero_shot(self, text, *a, **kw):
            return {'text': torch.zeros(1, 3, dtype=torch.int32)}
    cv = CosyVoice2.__new__(CosyVoice2)
    cv.output_sample_rate, cv.output_pcm16, cv.model_sample_rate, cv.sampling, cv.model_dir, cv.fp16 = None, False, 24000, None, 'unused', False
    cv.model, cv.frontend = _Model(), FE()
    return cv


def test_view():
    from cv2amd.level import Level
    from cv2amd.join import Join
    from cv2amd.sampling import Sampling
    from cv2amd.solver import Solver
    cv = _cv()
    assert cv.out_level is None and cv.level().out_level is None
    list(cv.level().inference_zero_shot('x', 'p', None))
    assert all('level' not in kw for _k, kw in cv.model.calls) and len(cv.model.calls) == 2, 'nothing set: the plain call'
    del cv.model.calls[:]
    v = cv.level(ceiling_db=-6)
    assert v is not cv and v.model is cv.model and v.out_level == Level(ceiling_db=-6) and cv.out_level is None
    assert v.level(gain_db=3).out_level == Level(gain_db=3, ceiling_db=-6), 'None keeps the setting'
    assert v.level(ceiling_db=-2).out_level == Level(ceiling_db=-2)
    for bad in (dict(gain_db=25), dict(gain_db=-24.5), dict(ceiling_db=1), dict(ceiling_db=-13), dict(lookahead_ms=0), dict(lookahead_ms=11),
                dict(peak_db=1), dict(peak_db=-25), dict(peak_db=-0.5), dict(peak_db=-5, ceiling_db=-6), dict(gain_db=float('nan'))):
        with pytest.raises(ValueError):
            cv.level(**bad)
    with pytest.raises(ValueError):
        v.level(peak_db=-3)                                                    # (above the view's own ceiling of -6)
    assert cv.model.calls == [], 'refused before the model is touched'
    # composes with the other views, in either order
    w = cv.output(sample_rate=16000, pcm16=True).sampler(seed=7).solver(steps=4).level(gain_db=-3, lookahead_ms=2)
    w2 = cv.level(gain_db=-3, lookahead_ms=2).solver(steps=4).sampler(seed=7).output(sample_rate=16000, pcm16=True)
    for x in (w, w2):
        assert (x.out_level, x.sampling, x.flow_solver, x.output_sample_rate, x.output_pcm16) == \
            (Level(gain_db=-3, lookahead_ms=2), Sampling(seed=7), Solver(steps=4), 16000, True)
    list(w.inference_zero_shot('x', 'p', None, stream=True))
    assert [k for k, _ in cv.model.calls] == ['tts', 'tts'] and all(kw['level'] == Level(gain_db=-3, lookahead_ms=2) and kw['stream'] is True and
                                                                   kw['output_sample_rate'] == 16000 for _k, kw in cv.model.calls)
    del cv.model.calls[:]
    j = cv.joined(pause_ms=100).level(peak_db=-3)
    assert j.join == Join(pause_ms=100) and j.out_level == Level(peak_db=-3)
    list(j.inference_zero_shot('x', 'p', None))
    assert cv.model.calls == [('joined', dict(speed=1.0, level=Level(peak_db=-3)))]
    del cv.model.calls[:]
    c = cv.level(gain_db=2).continuous(pause_ms=50)
    list(c.inference_zero_shot('x', 'p', None, stream=True))
    assert cv.model.calls == [('continuous', dict(speed=1.0, level=Level(gain_db=2)))]
    del cv.model.calls[:]
    # a peak target needs the call's end: not with stream=True, on a continuous view neither (whichever came first)
    with pytest.raises(ValueError, match='peak_db'):
        next(cv.level(peak_db=-3).inference_zero_shot('x', 'p', None, stream=True))
    with pytest.raises(ValueError, match='peak_db'):
        cv.continuous(pause_ms=50).level(peak_db=-3)
    with pytest.raises(ValueError, match='peak_db'):
        cv.level(peak_db=-3).continuous(pause_ms=50)
    assert cv.model.calls == []
    list(cv.level(peak_db=-3).inference_zero_shot('x', 'p', None))
    assert len(cv.model.calls) == 2 and all(kw['level'] == Level(peak_db=-3) and kw['stream'] is False for _k, kw in cv.model.calls)


def test_standalone_wrapper():
    from cosyvoice2_eu import Cosy2EU
    from cv2amd.level import Level
    eu = Cosy2EU(_cv())
    v = eu.level(gain_db=-2, ceiling_db=-3)
    assert isinstance(v, Cosy2EU) and v._model.out_level == Level(gain_db=-2, ceiling_db=-3) and eu._model.out_level is None
    with pytest.raises(ValueError):
        eu.level(lookahead_ms=20)


def test_model_keyword_is_checked_before_any_work():
    """CosyVoice2Model.tts / tts_joined / tts_continuous refuse a bad `level` before they touch the device (no model is built here: the
    unbound functions run on a bare object and must raise before they need it)."""
    from cosyvoice.cli.model import CosyVoice2Model
    from cv2amd.level import Level
    from cv2amd.join import Join
    m = CosyVoice2Model.__new__(CosyVoice2Model)
    t = torch.zeros(1, 3, dtype=torch.int32)
    with pytest.raises(ValueError, match='gain_db'):
        next(CosyVoice2Model.tts(m, text=t, level=Level(gain_db=99)))
    with pytest.raises(ValueError, match='peak_db'):
        next(CosyVoice2Model.tts(m, text=t, stream=True, level=Level(peak_db=-3)))
    with pytest.raises(ValueError, match='ceiling_db'):
        next(CosyVoice2Model.tts_joined(m, [dict(text=t), dict(text=t)], Join(pause_ms=10), level=Level(ceiling_db=3)))
    with pytest.raises(ValueError, match='peak_db'):
        next(CosyVoice2Model.tts_continuous(m, [dict(text=t), dict(text=t)], Join(pause_ms=10), level=Level(peak_db=-3)))


# ---- the server ----------------------------------------------------------------------------------------------------------------------
def _server():
    spec = importlib.util.spec_from_file_location('cv2_fastapi_server', os.path.join(PKG, 'runtime', 'python', 'fastapi', 'server.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_request_fields_reach_the_view_and_bad_values_answer_422():
    fastapi = pytest.importorskip('fastapi')
    from cv2amd.level import Level
    srv, cv = _server(), _cv(('un',))
    assert srv.request_view(cv) is cv
    v = srv.request_view(cv, gain_db=-3.0, ceiling_db=-2.0, lookahead_ms=3.0)
    assert v is not cv and v.model is cv.model and v.out_level == Level(gain_db=-3.0, ceiling_db=-2.0, lookahead_ms=3.0)
    w = srv.request_view(cv, 16000, seed=9, peak_db=-3.0, pause_ms=40)         # composes with the request's other fields
    assert w.output_sample_rate == 16000 and w.out_level == Level(peak_db=-3.0) and w.join is not None and w.sampling is not None
    assert srv.request_view(cv, gain_db=1.0, continuous=True).out_level == Level(gain_db=1.0)
    for bad in (dict(gain_db=30.0), dict(ceiling_db=0.5), dict(lookahead_ms=0.5), dict(peak_db=-30.0), dict(peak_db=-0.5), dict(peak_db=-3.0, continuous=True)):
        with pytest.raises(fastapi.HTTPException) as e:
            srv.request_view(cv, **bad)
        assert e.value.status_code == 422 and e.value.detail, bad
    assert cv.model.calls == []


def test_form_fields_over_http():
    pytest.importorskip('fastapi')
    pytest.importorskip('httpx')
    try:
        import python_multipart  # noqa: F401
    except ImportError:
        pytest.importorskip('multipart')
    from fastapi.testclient import TestClient
    from cv2amd.level import Level
    srv, cv = _server(), _cv(('un',))
    client = TestClient(srv.build_app(cv))
    r = client.post('/inference_sft', data=dict(tts_text='bonjour', spk_id='fr', gain_db='-3', peak_db='-6', ceiling_db='-2', lookahead_ms='2.5'))
    assert r.status_code == 200 and r.content == struct.pack('<4h', *[8192] * 4)
    assert cv.model.calls[0][1]['level'] == Level(gain_db=-3.0, peak_db=-6.0, ceiling_db=-2.0, lookahead_ms=2.5)
    r = client.post('/inference_sft', data=dict(tts_text='bonjour', spk_id='fr'))
    assert r.status_code == 200 and 'level' not in cv.model.calls[1][1]
    n = len(cv.model.calls)
    assert client.post('/inference_sft', data=dict(tts_text='bonjour', spk_id='fr', gain_db='30')).status_code == 422
    assert client.post('/inference_sft', data=dict(tts_text='bonjour', spk_id='fr', peak_db='-3', continuous='true')).status_code == 422
    assert client.post('/inference_sft', data=dict(tts_text='bonjour', spk_id='fr', ceiling_db='x')).status_code == 422
    assert len(cv.model.calls) == n


# ---- the restatement's own properties ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('L', R.LOOKAHEADS)
def test_restatement_properties(L):
    c = R.db(-6.0)
    n = 2 * 1024 + L + 3
    for name, s, Ge in (('bursts', R.bursts(n), 1.0), ('specials', R.specials(n), 1.0), ('zeros', np.zeros(n, dtype=np.float32), 1.0),
                        ('under', R.sine(n, 0.45), 1.0), ('gain', R.bursts(1025), R.db(6.5)), ('short', R.bursts(L + 1), 1.0), ('one', R.bursts(1), 1.0)):
        ref = R.level64(s, Ge, c, L)
        y, x = ref['y'], ref['x']
        assert y.shape == s.shape, 'N in, N out'
        assert (np.abs(y) <= float(c)).all(), f'{name}: above the ceiling'
        q = R.quiet(s, Ge, c, L) & np.isfinite(x)
        assert np.array_equal((ref['acc'] == 0) & np.isfinite(x), q)
        assert np.array_equal(y[q].astype(np.float32).view(np.uint32), x[q].view(np.uint32)), f'{name}: the pass-through is not bit-equal'
        if Ge == 1.0:
            assert np.array_equal(x[q].view(np.uint32), s[q].view(np.uint32))
        assert (y[np.isnan(x)] == 0).all() and not np.signbit(y[np.isnan(x)]).any()
        assert np.array_equal(y[np.isinf(x)], np.copysign(float(c), x[np.isinf(x)]))
        if name == 'bursts':
            assert q.sum() > 0 and (~q).sum() > 0
            # the gain is continuous except at the call's first sample (an over there has no look-behind: the min rule takes over)
            steps = np.abs(np.diff(ref['g']))
            assert steps[1:].max() < 8.0 / (L + 1) and ref['g'][0] == ref['r'][0] < 1
        # the stream equals the whole call, whatever the chunking (float64 sums of the same terms in the same order: bit-equal here too)
        for cname, chunks in R.chunkings(len(s), L).items():
            ys, _log = R.stream64(s, Ge, c, L, chunks)
            assert np.array_equal(ys.view(np.uint64), y.view(np.uint64)), f'{name}: "{cname}"'
