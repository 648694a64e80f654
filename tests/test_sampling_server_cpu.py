"""The FastAPI server's per-request sampler fields (runtime/python/fastapi/server.py) without a GPU: the mapping of `seed`, `temperature`,
`top_p`, `top_k` onto CosyVoice2.sampler() and the 422 answer for values out of range -- on the function every endpoint goes through,
and over HTTP where python-multipart (which FastAPI needs for form fields) is installed."""
import importlib.util
import os
import struct

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'cosyvoice2-eu_amd')


def _server():
    spec = importlib.util.spec_from_file_location('cv2_fastapi_server', os.path.join(PKG, 'runtime', 'python', 'fastapi', 'server.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


class _Model:
    """stands where CosyVoice2.model does: records what tts() was given and yields one short chunk"""

    def __init__(self):
        self.calls = []

    def tts(self, **kw):
        self.calls.append(kw)
        yield {'tts_speech': torch.full((1, 4), 0.25)}


class _FrontEnd:
    def text_normalize(self, text, split=True, **kw):
        return [text] if split else text

    def frontend_zero_shot(self, *a, **kw):
        return {}


def _cv(seen):
    """a CosyVoice2 over the stub model whose .sampler() calls are recorded in `seen`"""
    from cosyvoice.cli.cosyvoice import CosyVoice2

    class Spy(CosyVoice2):
        def sampler(self, **kw):
            seen.append(kw)
            return super().sampler(**kw)
    cv = Spy.__new__(Spy)
    cv.output_sample_rate, cv.output_pcm16, cv.model_sample_rate, cv.sampling = None, False, 24000, None
    cv.model, cv.frontend = _Model(), _FrontEnd()
    return cv


def test_request_fields_reach_the_sampler_and_bad_values_answer_422():
    fastapi = pytest.importorskip('fastapi')
    from cv2amd.sampling import Sampling
    srv = _server()
    seen = []
    cv = _cv(seen)
    assert srv.request_view(cv) is cv and seen == []                # nothing asked: the server's own model object, no view
    v = srv.request_view(cv, None, 7, 0.5, 0.9, 3)
    assert seen == [dict(seed=7, temperature=0.5, top_p=0.9, top_k=3)]
    assert v is not cv and v.model is cv.model and v.sampling == Sampling(seed=7, temperature=0.5, top_p=0.9, top_k=3)
    w = srv.request_view(cv, 16000, seed=9)                          # composes with the request's sample rate
    assert w.output_sample_rate == 16000 and w.sampling == Sampling(seed=9) and w.model is cv.model
    assert srv.request_view(cv, top_k=1).sampling == Sampling(top_k=1)
    for bad in (dict(top_k=26), dict(top_k=0), dict(temperature=0.0), dict(top_p=1.5), dict(seed=-1), dict(sample_rate=12345)):
        with pytest.raises(fastapi.HTTPException) as e:
            srv.request_view(cv, **bad)
        assert e.value.status_code == 422 and e.value.detail, bad
    assert cv.model.calls == []                                      # refused before the model is touched


def test_form_fields_over_http():
    pytest.importorskip('fastapi')
    pytest.importorskip('httpx')
    try:
        import python_multipart  # noqa: F401
    except ImportError:
        pytest.importorskip('multipart')
    from fastapi.testclient import TestClient
    from cv2amd.sampling import Sampling
    srv = _server()
    seen = []
    cv = _cv(seen)
    client = TestClient(srv.build_app(cv))
    r = client.post('/inference_sft', data=dict(tts_text='bonjour', spk_id='fr', seed='7', temperature='0.5', top_p='0.9', top_k='3'))
    assert r.status_code == 200 and r.content == struct.pack('<4h', *[8192] * 4)
    assert seen == [dict(seed=7, temperature=0.5, top_p=0.9, top_k=3)]
    assert cv.model.calls[0]['sampling'] == Sampling(seed=7, temperature=0.5, top_p=0.9, top_k=3)
    r = client.post('/inference_sft', data=dict(tts_text='bonjour', spk_id='fr'))
    assert r.status_code == 200 and 'sampling' not in cv.model.calls[1] and len(seen) == 1
    n = len(cv.model.calls)
    assert client.post('/inference_sft', data=dict(tts_text='bonjour', spk_id='fr', top_k='26')).status_code == 422
    assert client.post('/inference_sft', data=dict(tts_text='bonjour', spk_id='fr', temperature='0')).status_code == 422
    assert client.post('/inference_sft', data=dict(tts_text='bonjour', spk_id='fr', seed='x')).status_code == 422
    assert len(cv.model.calls) == n
