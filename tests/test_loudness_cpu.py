"""The loudness target without a GPU: the K-weighting coefficients of cv2amd/loudness.py against the BS.1770 table, the float64 oracle
(tests/_loudness.py) against known values, the `loudness_lufs` setting of cv2amd.level.Level (range, exclusivity with peak_db, refusal on a
stream, what resolve() returns with and without it), the float32 constants of the gain, and the FastAPI form field's 422."""
import importlib.util
import math
import os

import numpy as np
import pytest

import _loudness as R
from test_level_cpu import _cv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'cosyvoice2-eu_amd')
# ITU-R BS.1770-4, tables 1 and 2 (48 kHz)
SHELF_48K = ((1.53512485958697, -2.69169618940638, 1.19839281085285), (1.0, -1.69065929318241, 0.73248077421585))
HIGH_48K = ((1.0, -2.0, 1.0), (1.0, -1.99004745483398, 0.99007225036621))


def test_coefficients_at_48k_are_the_standards_table():
    from cv2amd import loudness as LD
    (b, a), (d, c) = LD.coefficients(48000)
    for got, want in ((b, SHELF_48K[0]), (a, SHELF_48K[1]), (d, HIGH_48K[0]), (c, HIGH_48K[1])):
        assert len(got) == 3 and all(abs(g - w) < 1e-12 for g, w in zip(got, want)), (got, want)
    shelf, high = R.coefficients(48000)                                        # the oracle derives its own
    assert all(abs(g - w) < 1e-12 for g, w in zip(shelf, SHELF_48K[0] + SHELF_48K[1][1:]))
    assert all(abs(g - w) < 1e-12 for g, w in zip(high, HIGH_48K[0] + HIGH_48K[1][1:]))


def test_coefficients_at_24k():
    from cv2amd import loudness as LD
    (b, a), (d, c) = LD.coefficients()
    assert abs(b[0] - 1.4879002209622763) < 1e-15 and d == [1.0, -2.0, 1.0] and a[0] == c[0] == 1.0
    shelf, high = R.coefficients()
    assert np.allclose(b + a[1:], shelf, rtol=0, atol=1e-15) and np.allclose(d + c[1:], high, rtol=0, atol=1e-15)
    vals = LD.table_values()
    assert len(vals) == 24 and vals[:7] == b + a[1:] + c[1:] and vals[7] == 0.0


def test_transition_matrix_is_the_hop_of_the_cascade():
    """M s + (the zero-state end state) is the end state from s, over a whole hop, for the transposed direct form II cascade the kernel
    runs (float64 here)"""
    from cv2amd import loudness as LD
    (b, a), (_d, c) = LD.coefficients()
    M = np.array(LD.transition())

    def run(x, s):
        s = list(s)
        for v in x:
            y = b[0] * v + s[0]
            s[0] = b[1] * v - a[1] * y + s[1]
            s[1] = b[2] * v - a[2] * y
            w = y + s[2]
            s[2] = -2.0 * y - c[1] * w + s[3]
            s[3] = y - c[2] * w
        return np.array(s)
    x = np.random.default_rng(1).standard_normal(LD.HOP).tolist()
    s0 = np.array([0.3, -0.2, 0.5, -0.4])
    want, zs = run(x, s0), run(x, [0.0] * 4)
    assert np.allclose(M @ s0 + zs, want, rtol=0, atol=1e-12) and np.abs(M @ s0).max() > 1e-9
    one = np.array(LD.transition(steps=1))
    assert np.allclose(one @ s0, run([0.0], s0), rtol=0, atol=1e-15)
    assert [LD.blocks(n) for n in (0, 9599, 9600, 11999, 12000, 73234)] == [R.blocks(n) for n in (0, 9599, 9600, 11999, 12000, 73234)] == [0, 0, 1, 1, 2, 27]


def test_oracle_sanity():
    s = R.sine(72000, 0.1)                                                      # 997 Hz, amplitude 0.1, 3 s
    m = R.measure(s)
    assert abs(m['lufs'] - (-22.984)) < 1e-3 and m['J'] == 27 == m['nA'] == m['nB'] and m['margin'] > 1
    for k in (0.5, 3.0):
        assert abs(R.measure((k * s.astype(np.float64))).get('lufs') - (m['lufs'] + 20.0 * math.log10(k))) < 1e-9
    z = R.measure(np.zeros(30000, dtype=np.float32))
    assert z['lufs'] == -math.inf and z['J'] == 9 and z['nA'] == 0
    assert R.measure(np.ones(9599, dtype=np.float32))['J'] == 0 and R.measure(np.ones(9599, dtype=np.float32))['lufs'] == -math.inf
    bad, clean = R.specials()
    assert not np.isfinite(bad).all() and R.measure(bad)['lufs'] == R.measure(clean)['lufs']
    b = R.measure(R.bursts())
    assert b['nB'] < b['nA'] < b['J'] and b['margin'] >= R.MARGIN, 'both gates act'


def test_level_setting():
    from cv2amd.level import Level, check
    lv = Level(loudness_lufs=-16)
    assert lv.check() is lv and lv.loud and not lv.is_default() and not Level(gain_db=1).loud
    assert Level(loudness_lufs=-40).check() and Level(loudness_lufs=-5).check()
    for bad in (-40.5, -4.9, 0, float('nan'), float('inf'), True, '−16'):
        with pytest.raises(ValueError, match='loudness_lufs'):
            Level(loudness_lufs=bad).check()
    with pytest.raises(ValueError, match='peak_db'):
        Level(loudness_lufs=-16, peak_db=-3).check()
    with pytest.raises(ValueError, match='ceiling'):
        Level(loudness_lufs=-6, ceiling_db=-12).check()                        # (a reference amplitude above the ceiling)
    with pytest.raises(ValueError, match='loudness_lufs'):
        lv.check_stream(True)
    assert lv.check_stream(False) is lv
    with pytest.raises(ValueError, match='loudness_lufs'):
        check(lv, stream=True)
    assert check(lv) is lv
    # value semantics with the new field
    assert lv == Level(loudness_lufs=-16) and hash(lv) == hash(Level(loudness_lufs=-16)) and lv != Level(loudness_lufs=-17) and lv != Level()
    assert lv.replace(gain_db=2) == Level(gain_db=2, loudness_lufs=-16) and Level(gain_db=2).replace(loudness_lufs=-23).loudness_lufs == -23
    assert lv.replace(loudness_lufs=None) == lv and 'loudness_lufs=-16' in repr(lv) and 'loudness' not in repr(Level(gain_db=1))
    assert Level().is_default() and Level(loudness_lufs=None).is_default()


def test_resolve_is_unchanged_without_the_setting_and_T_is_a_rounded_float64():
    from cv2amd.level import Level
    from cv2amd import loudness as LD
    f = lambda v: float(np.float32(v))                                         # noqa: E731
    assert Level().resolve() == (1.0, f(10.0 ** (-1.0 / 20.0)), 120, None)
    assert Level(gain_db=-3, ceiling_db=-6, lookahead_ms=2).resolve() == (f(10.0 ** (-3 / 20.0)), f(10.0 ** (-6 / 20.0)), 48, None)
    assert Level(peak_db=-3).resolve() == (1.0, f(10.0 ** (-1.0 / 20.0)), 120, f(10.0 ** (-3 / 20.0)))
    for lufs in (-16, -23, -40, -5, -17.3):
        G, c, L, T = Level(loudness_lufs=lufs, gain_db=2).resolve()
        assert T == f(10.0 ** ((lufs + 0.691) / 20.0)) == LD.target(lufs) and T == float(np.float32(T)) and (G, L) == (f(10.0 ** 0.1), 120)
    assert LD.G_MAX == f(10.0 ** (24.0 / 20.0)) == f(15.848931924611133)
    assert abs(20.0 * math.log10(LD.target(-16)) - (-16 + 0.691)) < 1e-6


def test_views_take_the_keyword():
    from cosyvoice2_eu import Cosy2EU
    from cv2amd.level import Level
    cv = _cv()
    v = cv.level(loudness_lufs=-16)
    assert v is not cv and v.out_level == Level(loudness_lufs=-16) and cv.out_level is None
    assert v.level(gain_db=1).out_level == Level(gain_db=1, loudness_lufs=-16), 'None keeps the setting'
    for bad in (dict(loudness_lufs=-3), dict(loudness_lufs=-41), dict(loudness_lufs=-16, peak_db=-3)):
        with pytest.raises(ValueError):
            cv.level(**bad)
    with pytest.raises(ValueError):
        v.level(peak_db=-3)
    with pytest.raises(ValueError, match='loudness_lufs'):
        next(v.inference_zero_shot('x', 'p', None, stream=True))
    with pytest.raises(ValueError):
        v.continuous(pause_ms=50)
    with pytest.raises(ValueError):
        cv.continuous(pause_ms=50).level(loudness_lufs=-16)
    assert cv.model.calls == [], 'refused before the model is touched'
    list(v.inference_zero_shot('x', 'p', None))
    assert len(cv.model.calls) == 2 and all(kw['level'] == Level(loudness_lufs=-16) for _k, kw in cv.model.calls)
    eu = Cosy2EU(cv).level(loudness_lufs=-23, gain_db=-1)
    assert isinstance(eu, Cosy2EU) and eu._model.out_level == Level(gain_db=-1, loudness_lufs=-23)


def test_model_keyword_is_checked_before_any_work():
    import torch
    from cosyvoice.cli.model import CosyVoice2Model
    from cv2amd.level import Level
    from cv2amd.join import Join
    m = CosyVoice2Model.__new__(CosyVoice2Model)
    t = torch.zeros(1, 3, dtype=torch.int32)
    with pytest.raises(ValueError, match='loudness_lufs'):
        next(CosyVoice2Model.tts(m, text=t, level=Level(loudness_lufs=-2)))
    with pytest.raises(ValueError, match='loudness_lufs'):
        next(CosyVoice2Model.tts(m, text=t, stream=True, level=Level(loudness_lufs=-16)))
    with pytest.raises(ValueError, match='loudness_lufs'):
        next(CosyVoice2Model.tts_continuous(m, [dict(text=t), dict(text=t)], Join(pause_ms=10), level=Level(loudness_lufs=-16)))
    with pytest.raises(ValueError, match='peak_db'):
        next(CosyVoice2Model.tts_joined(m, [dict(text=t), dict(text=t)], Join(pause_ms=10), level=Level(loudness_lufs=-16, peak_db=-3)))


def test_header_declares_the_entry_points():
    import re
    from cv2amd import lib as L
    hdr = open(os.path.join(ROOT, 'include', 'cv2_amd.h')).read()
    for name in ('cv2_loudness_workspace_bytes', 'cv2_loudness_batch'):
        assert re.search(r'\bint %s\(' % name, hdr) and name in L.EXPORTS
    src = open(os.path.join(PKG, 'csrc', 'loudness.hip')).read()
    assert 'atomic' not in src.split('#include')[1 + 1], 'the measurement uses no atomics'


def test_server_field_and_422():
    fastapi = pytest.importorskip('fastapi')
    from cv2amd.level import Level
    spec = importlib.util.spec_from_file_location('cv2_fastapi_server_loudness', os.path.join(PKG, 'runtime', 'python', 'fastapi', 'server.py'))
    srv = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(srv)
    cv = _cv(('un',))
    v = srv.request_view(cv, loudness_lufs=-16.0, gain_db=1.0)
    assert v is not cv and v.out_level == Level(gain_db=1.0, loudness_lufs=-16.0)
    assert srv.request_view(cv, 16000, loudness_lufs=-23.0, pause_ms=40).out_level == Level(loudness_lufs=-23.0)
    for bad in (dict(loudness_lufs=-4.0), dict(loudness_lufs=-40.5), dict(loudness_lufs=-16.0, peak_db=-3.0), dict(loudness_lufs=-16.0, continuous=True)):
        with pytest.raises(fastapi.HTTPException) as e:
            srv.request_view(cv, **bad)
        assert e.value.status_code == 422 and e.value.detail, bad
    assert cv.model.calls == []
