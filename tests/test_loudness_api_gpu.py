"""The loudness target through the scheduler (cosyvoice/cli/model.py) and the public surface: a call with `loudness_lufs` carries the
measured loudness of its unlevelled signal and comes out at the target, for tts(), a joined call and the Cosy2EU view; streaming and a peak
target beside it are refused before any work; a call without a target carries no such key and is the call it was.  Synthetic weights and
the fixtures of tests/test_join_api_gpu.py; seeded calls.  The float64 oracle of tests/_loudness.py is the yardstick, the gate margin of
every signal it measures is asserted.  Run with -m gpu."""
import math

import numpy as np
import pytest
import torch

import _loudness as R
from _bars import bar
from test_join_api_gpu import Rig, _cv, _seeds

pytestmark = pytest.mark.gpu
FORCE_LEN = 80                                    # 76 800 samples: 29 blocks


@pytest.fixture(scope='module')
def rig():
    assert torch.cuda.is_available(), 'needs a GPU'
    return Rig()


def _idle(rig):
    return rig.idle() and not rig.mdl.level_dict and not rig.mdl.cont_dict


def _oracle(wav):
    m = R.measure(wav[0].numpy())
    assert m['margin'] >= R.MARGIN and math.isfinite(m['lufs']), f'gate margin {m["margin"]:.4f} LU'
    return m


def _holds(name, base, out, target, gain_db=0.0):
    """`out` is the result of the call whose unlevelled waveform is `base`: its 'loudness_lufs' is the oracle's measure of `base`, and its
    waveform is `base` times the expected gain and measures `target` (the limiter idle: asserted on the oracle's side)"""
    from cv2amd.level import Level
    m = _oracle(base)
    lk = out['loudness_lufs']
    assert isinstance(lk, float) and math.isfinite(lk)
    print(f'{name}: Lk {lk!r}, oracle {m["lufs"]!r}, apart {abs(lk - m["lufs"]):.3e} LU')
    bar(f'loudness_api_{name}_in', abs(lk - m['lufs']), R.BAR_LU)
    c = Level(loudness_lufs=target).resolve()[1]
    g = 10.0 ** ((target + gain_db - m['lufs']) / 20.0)
    assert g < 15.0 and float(base.abs().max()) * g < 0.95 * c, 'the limiter stays idle and the gain is inside +-24 dB'
    want = base.double() * g
    got = out['tts_speech']
    assert got.shape == base.shape and got.dtype == torch.float32
    tol = 10.0 ** (R.BAR_LU / 20.0) - 1.0                                        # the bar as a relative amplitude
    assert float((got.double() - want).abs().max()) <= tol * float(want.abs().max())
    assert abs(_oracle(want.float())['lufs'] - (target + gain_db)) < 1e-6
    o = _oracle(got)
    print(f'{name}: delivered {o["lufs"]!r}, target {target + gain_db}')
    bar(f'loudness_api_{name}_out', abs(o['lufs'] - (target + gain_db)), R.BAR_LU)


def test_tts_call_with_a_loudness_target(rig):
    from cv2amd.level import Level
    mdl, sp = rig.mdl, _seeds(0x10D, 1)[0]
    (base,) = list(mdl.tts(stream=False, force_len=FORCE_LEN, sampling=sp, **rig.kw(0)))
    assert set(base) == {'tts_speech'}, 'a call without a target carries no loudness'
    (out,) = list(mdl.tts(stream=False, force_len=FORCE_LEN, sampling=sp, level=Level(loudness_lufs=-20), **rig.kw(0)))
    assert set(out) == {'tts_speech', 'loudness_lufs'}
    _holds('tts', base['tts_speech'], out, -20.0)
    (out2,) = list(mdl.tts(stream=False, force_len=FORCE_LEN, sampling=sp, level=Level(loudness_lufs=-23, gain_db=2), **rig.kw(0)))
    _holds('tts_gain', base['tts_speech'], out2, -23.0, gain_db=2.0)
    assert out2['loudness_lufs'] == out['loudness_lufs'], 'the measure is of the unlevelled signal'
    assert _idle(rig)


def test_serial_call_with_a_loudness_target(rig):
    """the one-call path (a noise hook keeps the call out of the coalesced batch)"""
    from cv2amd.level import Level
    mdl = rig.mdl

    def run(**extra):
        cnt = [0]

        def hook(T):
            cnt[0] += 1
            return torch.randn(1, 480 * T, 9, generator=torch.Generator().manual_seed(200 + cnt[0]))
        mdl._noise_hook = hook
        try:
            (o,) = list(mdl.tts(stream=False, force_len=57, sampling=_seeds(6, 1)[0], **extra, **rig.kw(1)))
        finally:
            mdl._noise_hook = None
        return o
    base, out = run(), run(level=Level(loudness_lufs=-20))
    assert set(base) == {'tts_speech'}
    _holds('serial', base['tts_speech'], out, -20.0)
    assert _idle(rig)


def test_joined_call_has_one_value(rig):
    from cv2amd.join import Join
    from cv2amd.level import Level
    join, sp = Join(pause_ms=150), _seeds(0x10E2, 3)
    base, _ = rig.joined([0, 1, 2], join, sampling=sp)
    out, _ = rig.joined([0, 1, 2], join, sampling=sp, level=Level(loudness_lufs=-20))
    assert set(base) == {'tts_speech', 'segments'} and set(out) == {'tts_speech', 'segments', 'loudness_lufs'} and out['segments'] == base['segments']
    _holds('joined', base['tts_speech'], out, -20.0)
    rig.mdl._token_log = None
    assert _idle(rig)


def test_public_views(rig):
    from cosyvoice2_eu import Cosy2EU
    cv = _cv(rig, segments=('un', 'deux', 'trois')).sampler(seed=7)
    (base,) = list(cv.joined(pause_ms=150).inference_zero_shot('x', 'salut', None, zero_shot_spk_id='fr'))
    (out,) = list(cv.level(loudness_lufs=-20).joined(pause_ms=150).inference_zero_shot('x', 'salut', None, zero_shot_spk_id='fr'))
    assert 'loudness_lufs' not in base
    _holds('view_joined', base['tts_speech'], out, -20.0)
    eu = Cosy2EU(cv).level(loudness_lufs=-20)
    (out_eu,) = list(eu._model.joined(pause_ms=150).inference_zero_shot('x', 'salut', None, zero_shot_spk_id='fr'))
    assert out_eu['loudness_lufs'] == out['loudness_lufs'] and torch.equal(out_eu['tts_speech'], out['tts_speech'])
    rig.mdl._token_log = None
    assert _idle(rig)


def test_refusals_come_before_any_synthesis(rig, monkeypatch):
    from cv2amd.level import Level
    cv, mdl = _cv(rig), rig.mdl

    def no_work(*a, **k):
        raise AssertionError('refused calls must not reach the scheduler')
    monkeypatch.setattr(mdl, '_tts_coalesced', no_work)
    monkeypatch.setattr(mdl, '_stream_chunks', no_work)
    with pytest.raises(ValueError, match='loudness_lufs'):
        next(cv.level(loudness_lufs=-20).inference_zero_shot('bonjour', 'salut', None, zero_shot_spk_id='fr', stream=True))
    with pytest.raises(ValueError, match='loudness_lufs'):
        next(mdl.tts(stream=True, force_len=FORCE_LEN, level=Level(loudness_lufs=-20), **rig.kw(0)))
    with pytest.raises(ValueError, match='peak_db'):
        cv.level(peak_db=-3, loudness_lufs=-20)
    with pytest.raises(ValueError, match='peak_db'):
        next(mdl.tts(force_len=FORCE_LEN, level=Level(peak_db=-3, loudness_lufs=-20), **rig.kw(0)))
    assert _idle(rig)


def test_call_without_a_target_is_the_call_it_was(rig, monkeypatch):
    """no measurement is launched, no key is added, and the waveform is bit-equal to the same call made before the model ever measured"""
    import cosyvoice.cli.model as M
    from cv2amd.level import Level
    mdl, sp = rig.mdl, _seeds(0x10F, 1)[0]
    fresh = Rig().mdl                                                            # a model that never used the feature
    (want,) = list(fresh.tts(stream=False, force_len=40, sampling=sp, **rig.kw(0)))
    list(mdl.tts(stream=False, force_len=40, sampling=sp, level=Level(loudness_lufs=-20), **rig.kw(0)))

    def no_launch(*a, **k):
        raise AssertionError('a call without a loudness target must not launch the measurement')
    monkeypatch.setattr(M.LD, 'measure', no_launch)
    for kw in (dict(), dict(level=None), dict(level=Level()), dict(level=Level(gain_db=0))):
        (got,) = list(mdl.tts(stream=False, force_len=40, sampling=sp, **kw, **rig.kw(0)))
        assert set(got) == {'tts_speech'}
        if 'level' not in kw or kw['level'] is None or kw['level'].is_default():
            assert torch.equal(got['tts_speech'].view(torch.int32), want['tts_speech'].view(torch.int32))
    assert _idle(rig)
