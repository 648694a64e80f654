"""Per-call flow solver settings (Euler steps, guidance rate) without a GPU: the oracle under each setting against the reference's own
output (tests/golden/flow_solver.npz, make_golden_solver.py), the library's host schedule against the oracle's t_span bit for bit, the
validation of cv2amd.solver.Solver, the C ABI's new names, the CosyVoice2 / Cosy2EU views and the server's form fields."""
import ctypes
import importlib.util
import os
import re

import numpy as np
import pytest
import torch

import _solver_oracle as SO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'cosyvoice2-eu_amd')


@pytest.mark.parametrize('steps,cfg', SO.SETTINGS)
def test_oracle_under_solver_settings_matches_the_reference(golden, steps, cfg):
    from cv2amd import synth
    gd, ge = golden('flow_solver.npz'), golden('flow_e2e.npz')
    assert [tuple(r) for r in gd['settings'].tolist()] == [(float(n), c) for n, c in SO.SETTINGS]
    inp = synth.synthetic_inputs(prompt_len=int(ge['prompt_len']))
    sd = synth.make_flow()
    tok = torch.from_numpy(ge['token'])
    assert np.array_equal(gd[f't_span_n{steps}'], (1 - torch.cos(torch.linspace(0, 1, steps + 1) * 0.5 * torch.pi)).numpy())
    for tag, streaming, finalize in SO.TAGS:
        ref = torch.from_numpy(gd[SO.key(tag, steps, cfg)])
        got = SO.inference(sd, tok, inp['prompt_token'], inp['prompt_feat'], inp['embedding'], streaming, finalize, steps, cfg)
        assert got.shape == ref.shape
        err = (got - ref).abs().max().item()
        print(f'oracle vs reference, steps {steps} cfg {cfg} {tag}: {err:.3e}')
        assert err < 2e-5, f'{tag}: {err:.3e}'
    # another setting is another mel: the fixture is not the default's under a new name
    assert not np.allclose(gd[SO.key('full', steps, cfg)], ge['mel_full'], atol=1e-3)


@pytest.mark.parametrize('n', [1, 4, 10, 16, 31])
def test_host_schedule_equals_the_oracles_t_span_walk_bit_for_bit(n):
    """cv2_flow_schedule (the helper cv2_flow_create and the per-call tables share) walks t / dt as solve_euler does over
    oracle.flow.t_span(n): same fp32 values, every bit."""
    from cv2amd import lib as L
    from oracle import flow as OF
    cdll = ctypes.CDLL(L.LIB_PATH)
    cdll.cv2_flow_schedule.argtypes = [ctypes.c_int32, ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_float)]
    t, dt = (ctypes.c_float * n)(), (ctypes.c_float * n)()
    assert cdll.cv2_flow_schedule(n, t, dt) == 0
    want_t, want_dt = SO.walk(OF.t_span(n))
    assert np.array_equal(np.frombuffer(t, dtype=np.float32).view(np.uint32), want_t.numpy().view(np.uint32))
    assert np.array_equal(np.frombuffer(dt, dtype=np.float32).view(np.uint32), want_dt.numpy().view(np.uint32))
    for bad in (0, 32, -1):
        assert cdll.cv2_flow_schedule(bad, t, dt) == -1


def test_solver_validation_and_resolve():
    from cv2amd.solver import Solver, resolve
    from cv2amd.sampling import f32

    class Eng:
        n_timesteps, cfg_rate = 10, 0.7
    assert Solver().is_default() and not Solver(steps=4).is_default() and not Solver(cfg_rate=0.0).is_default()
    assert Solver().resolve(Eng) == (10, f32(0.7)) == resolve(None, Eng)
    assert Solver(steps=4).resolve(Eng) == (4, f32(0.7)) and Solver(cfg_rate=1.5).resolve(Eng) == (10, 1.5)
    assert Solver(steps=10, cfg_rate=0.7).resolve(Eng) == Solver().resolve(Eng)          # the explicit engine values are the default computation
    assert Solver(steps=4).replace(cfg_rate=0.2) == Solver(steps=4, cfg_rate=0.2) and Solver(steps=4).replace(steps=None) == Solver(steps=4)
    assert repr(Solver(steps=4)) == 'Solver(steps=4)'
    for ok in (dict(steps=1), dict(steps=31), dict(cfg_rate=0), dict(cfg_rate=0.0), dict(cfg_rate=25.0), dict()):
        assert Solver(**ok).check() == Solver(**ok)
    for bad in (dict(steps=0), dict(steps=32), dict(steps=-3), dict(steps=4.0), dict(steps=True), dict(steps='4'), dict(cfg_rate=-0.1),
                dict(cfg_rate=float('nan')), dict(cfg_rate=float('inf')), dict(cfg_rate=1e39), dict(cfg_rate='0.7'), dict(cfg_rate=True)):
        with pytest.raises(ValueError, match='solver:'):
            Solver(**bad).check()


def test_header_declares_and_library_exports_the_solver_entry_points():
    from cv2amd import lib as L
    hdr = open(os.path.join(ROOT, 'include', 'cv2_amd.h')).read()
    assert re.search(r'#define\s+CV2_ABI_VERSION\s+3\b', hdr) and L.ABI_VERSION == 3
    cdll = ctypes.CDLL(L.LIB_PATH)
    assert cdll.cv2_version() == 3
    assert re.search(r'typedef struct \{\s*int32_t n_timesteps;\s*float cfg_rate;\s*\}\s*cv2_flow_solver;', hdr)
    for name in ('cv2_flow_inference_ex', 'cv2_flow_inference_chunk_ex', 'cv2_flow_cache_bytes_ex', 'cv2_flow_cache_copy_ex', 'cv2_flow_schedule'):
        assert re.search(r'\b(int|size_t) ' + name + r'\(', hdr), name
        assert name in L.EXPORTS and hasattr(cdll, name), name
    assert re.search(r'int cv2_flow_inference_ex\(cv2_flow\* h, const cv2_flow_utt\* utts, const cv2_flow_solver\* solver, int32_t n_utts, int32_t streaming,\s*int32_t finalize, void\* stream\);', hdr)
    assert re.search(r'int cv2_flow_inference_chunk_ex\(cv2_flow\* h, const cv2_flow_utt\* utts, const cv2_flow_cache_ref\* refs, const cv2_flow_solver\* solver,\s*int32_t n_utts, int32_t finalize, void\* stream\);', hdr)
    # the signatures that existed stay
    assert 'int cv2_flow_inference(cv2_flow* h, const cv2_flow_utt* utts, int32_t n_utts, int32_t streaming, int32_t finalize, void* stream);' in hdr
    assert 'size_t cv2_flow_cache_bytes(const cv2_flow* h, int32_t cache_frames);' in hdr
    from cv2amd.flow import FlowSolver
    assert ctypes.sizeof(FlowSolver) == 8 and [f[0] for f in FlowSolver._fields_] == ['n_timesteps', 'cfg_rate']


class _Model:
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


def _cv():
    from cosyvoice.cli.cosyvoice import CosyVoice2
    cv = CosyVoice2.__new__(CosyVoice2)
    cv.output_sample_rate, cv.output_pcm16, cv.model_sample_rate, cv.sampling = None, False, 24000, None
    cv.model, cv.frontend = _Model(), _FrontEnd()
    return cv


def test_solver_views_compose_with_sampler_and_output():
    from cv2amd.sampling import Sampling
    from cv2amd.solver import Solver
    from cosyvoice2_eu import Cosy2EU
    cv = _cv()
    v = cv.solver(steps=4)
    assert v is not cv and v.model is cv.model and v.flow_solver == Solver(steps=4) and cv.flow_solver is None
    assert cv.solver() .flow_solver is None                                   # nothing set: no setting travels
    assert v.solver(cfg_rate=1.5).flow_solver == Solver(steps=4, cfg_rate=1.5) and v.solver(steps=6).flow_solver == Solver(steps=6)
    a = cv.solver(steps=4).sampler(seed=7).output(sample_rate=16000)
    b = cv.output(sample_rate=16000).solver(steps=4).sampler(seed=7)
    c = cv.sampler(seed=7).output(sample_rate=16000).solver(steps=4)
    for w in (a, b, c):
        assert w.flow_solver == Solver(steps=4) and w.sampling == Sampling(seed=7) and w.output_sample_rate == 16000 and w.model is cv.model
    list(a.inference_zero_shot('bonjour', '', None, zero_shot_spk_id='fr'))
    kw = cv.model.calls[-1]
    assert kw['solver'] == Solver(steps=4) and kw['sampling'] == Sampling(seed=7) and kw['output_sample_rate'] == 16000
    list(cv.inference_zero_shot('bonjour', '', None, zero_shot_spk_id='fr'))
    assert 'solver' not in cv.model.calls[-1]                                # the default call passes what it passed before
    for bad in (dict(steps=0), dict(steps=32), dict(cfg_rate=-1.0), dict(cfg_rate=float('nan'))):
        with pytest.raises(ValueError):
            cv.solver(**bad)
    eu = Cosy2EU(cv).solver(steps=4, cfg_rate=0.5)
    assert isinstance(eu, Cosy2EU) and eu._model.flow_solver == Solver(steps=4, cfg_rate=0.5) and eu._model.model is cv.model
    assert Cosy2EU(cv).sampler(seed=1).solver(steps=2)._model.sampling == Sampling(seed=1)


def test_tts_keeps_the_references_signature_and_takes_solver_last():
    import inspect
    from cosyvoice.cli.model import CosyVoice2Model
    names = list(inspect.signature(CosyVoice2Model.tts).parameters)
    assert names[-2:] == ['solver', 'kwargs'] and names[names.index('sampling') + 1] == 'solver'
    assert inspect.signature(CosyVoice2Model.tts).parameters['solver'].default is None


def _server():
    spec = importlib.util.spec_from_file_location('cv2_fastapi_server_solver', os.path.join(PKG, 'runtime', 'python', 'fastapi', 'server.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_server_fields_reach_the_solver_and_bad_values_answer_422():
    fastapi = pytest.importorskip('fastapi')
    from cv2amd.sampling import Sampling
    from cv2amd.solver import Solver
    srv = _server()
    cv = _cv()
    assert srv.request_view(cv) is cv
    v = srv.request_view(cv, flow_steps=4, cfg_rate=0.5)
    assert v is not cv and v.model is cv.model and v.flow_solver == Solver(steps=4, cfg_rate=0.5) and v.sampling is None
    w = srv.request_view(cv, 16000, seed=9, flow_steps=6)
    assert w.output_sample_rate == 16000 and w.sampling == Sampling(seed=9) and w.flow_solver == Solver(steps=6)
    assert srv.request_view(cv, cfg_rate=0.0).flow_solver == Solver(cfg_rate=0.0)
    for bad in (dict(flow_steps=0), dict(flow_steps=32), dict(cfg_rate=-0.5), dict(cfg_rate=float('inf'))):
        with pytest.raises(fastapi.HTTPException) as e:
            srv.request_view(cv, **bad)
        assert e.value.status_code == 422 and e.value.detail, bad
    assert cv.model.calls == []


def test_server_form_fields_over_http():
    pytest.importorskip('fastapi')
    pytest.importorskip('httpx')
    try:
        import python_multipart  # noqa: F401
    except ImportError:
        pytest.importorskip('multipart')
    from fastapi.testclient import TestClient
    from cv2amd.solver import Solver
    srv = _server()
    cv = _cv()
    client = TestClient(srv.build_app(cv))
    r = client.post('/inference_sft', data=dict(tts_text='bonjour', spk_id='fr', flow_steps='4', cfg_rate='0.5'))
    assert r.status_code == 200 and cv.model.calls[0]['solver'] == Solver(steps=4, cfg_rate=0.5)
    r = client.post('/inference_sft', data=dict(tts_text='bonjour', spk_id='fr'))
    assert r.status_code == 200 and 'solver' not in cv.model.calls[1]
    n = len(cv.model.calls)
    for bad in (dict(flow_steps='0'), dict(flow_steps='40'), dict(flow_steps='x'), dict(flow_steps='4.5'), dict(cfg_rate='-1'), dict(cfg_rate='nan')):
        r = client.post('/inference_sft', data=dict(tts_text='bonjour', spk_id='fr', **bad))
        assert 400 <= r.status_code < 500, (bad, r.status_code)
    assert len(cv.model.calls) == n
