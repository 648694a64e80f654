"""Continuous calls through the scheduler and the public surface: synthetic weights (2-layer LLM, full-size flow and
HiFT) and the fixtures of tests/test_join_api_gpu.py; forced lengths of two to three chunks per segment.  Run with -m gpu on an MI355X."""
import threading

import numpy as np
import pytest
import torch

import _join_stream as RS
from test_join_api_gpu import Rig, _cv, _seeds

pytestmark = pytest.mark.gpu
FL = (60, 80, 75)                                                             # speech tokens per segment: 2, 3 and 3 chunks (first chunk 47 tokens, 25 per later one)


@pytest.fixture(scope='module')
def rig():
    assert torch.cuda.is_available(), 'needs a GPU'
    return Rig()


def _idle(rig):
    return rig.idle() and not rig.mdl.cont_dict and not rig.mdl.stretch_dict and not rig.mdl._first_need and not rig.mdl._flow_caches


def _plain_streams(rig, sp, fl=FL, **extra):
    """every segment as a plain seeded streaming call -> ([its chunks], tokens) per segment"""
    out = []
    for i, n in enumerate(fl):
        chunks, (toks,) = rig.logged(lambda: [o['tts_speech'] for o in rig.mdl.tts(stream=True, force_len=n, sampling=sp[i], **extra, **rig.kw(i))])
        out.append((chunks, toks))
    return out


def _continuous(rig, join, sp, fl=FL, **extra):
    res, toks = rig.logged(lambda: list(rig.mdl.tts_continuous([rig.kw(i) for i in range(len(fl))], join, force_len=list(fl), sampling=sp, **extra)))
    return res, toks


@pytest.mark.parametrize('settings,speed', [(dict(pause_ms=7 / 24), 1.0), (dict(pause_ms=20, trim_db=20), 1.0), (dict(pause_ms=0, trim_db=30, fade_ms=2), 1.25)])
def test_segments_are_the_plain_streams_and_the_stream_is_the_restatement(rig, settings, speed):
    from cv2amd.join import Join
    join, sp = Join(**settings), _seeds(0x5EED2025, 3)
    kw = {} if speed == 1.0 else dict(speed=speed)
    plain = _plain_streams(rig, sp, **kw)
    assert [len(c) for c, _ in plain] == [2, 3, 3] and [len(t) for _, t in plain] == list(FL)
    segs = [torch.cat(c, dim=1)[0].numpy() for c, _ in plain]
    res, toks = _continuous(rig, join, sp, **kw)
    assert toks == [t for _, t in plain]
    assert [r['segment'] for r in res] == [0, 0, 1, 1, 1, 2, 2, 2] and all(set(r) == {'tts_speech', 'segment'} for r in res[:-1])
    assert set(res[-1]) == {'tts_speech', 'segment', 'segments'}
    assert all(r['tts_speech'].device.type == 'cpu' and r['tts_speech'].dtype == torch.float32 and r['tts_speech'].dim() == 2 for r in res)
    pause, F, g = join.resolve()
    want, spans = RS.stream(segs, None if g is None else np.float32(g), pause, F)
    got = torch.cat([r['tts_speech'] for r in res], dim=1)[0].numpy()
    assert res[-1]['segments'] == spans
    assert got.size == want.size and np.array_equal(got.view(np.int32), want.view(np.int32))
    if g is None:                                                             # nothing gated: the first segment's chunks go out as they come
        assert torch.equal(res[0]['tts_speech'], plain[0][0][0]) and res[1]['tts_speech'].shape[1] == plain[0][0][1].shape[1] + pause
    rig.mdl._token_log = None
    assert _idle(rig)


@pytest.mark.parametrize('rate,pcm16', [(16000, True), (44100, False)])
def test_one_output_record_serves_the_whole_call(rig, rate, pcm16):
    """The stream equals cv2_out_resample of the whole 24 kHz call signal; the plain per-segment streams, whose filter restarts at every
    seam, do not concatenate to it."""
    from cv2amd.join import Join
    mdl, join, sp = rig.mdl, Join(pause_ms=0), _seeds(77, 3)
    f24, _ = _continuous(rig, join, sp)
    whole = torch.cat([r['tts_speech'] for r in f24], dim=1)
    want = mdl._out_convert([(mdl._Out(rate, pcm16, mdl.device), whole.to(mdl.device), True)])[0].cpu()
    res, _ = _continuous(rig, join, sp, output_sample_rate=rate, pcm16=pcm16)
    got = torch.cat([r['tts_speech'] for r in res], dim=1)
    assert got.dtype == (torch.int16 if pcm16 else torch.float32) and res[-1]['segments'] == f24[-1]['segments']
    assert got.shape == want.shape and torch.equal(got, want)
    # the plain per-segment streams: equal to the call's stream up to the first seam's filter reach, different right behind the seam (the filter
    # restarted there: it saw zeros in place of the previous segment's last samples)
    segs_out = [torch.cat(c, dim=1) for c, _ in _plain_streams(rig, sp, output_sample_rate=rate, pcm16=pcm16)]
    n0, reach = segs_out[0].shape[1], 64
    assert f24[-1]['segments'][0][1] * rate % 24000 == 0                      # (segment 0 ends on an output sample: the streams are aligned behind it)
    assert torch.equal(segs_out[0][:, :n0 - reach], got[:, :n0 - reach])
    assert not torch.equal(segs_out[1][:, :reach], got[:, n0:n0 + reach])
    rig.mdl._token_log = None
    assert _idle(rig)


def test_two_continuous_callers_and_a_plain_stream_run_together_and_an_abandoned_call_leaves_nothing(rig):
    from cv2amd.join import Join
    from cv2amd.sampling import Sampling
    mdl = rig.mdl
    jobs = [lambda: rig.logged(lambda: list(mdl.tts_continuous([rig.kw(i) for i in (0, 1, 2)], Join(pause_ms=10), force_len=[60, 80, 75], sampling=_seeds(101, 3))))[1],
            lambda: rig.logged(lambda: list(mdl.tts_continuous([rig.kw(i) for i in (2, 1, 0)], Join(pause_ms=0, trim_db=30), force_len=[75, 60, 80], sampling=_seeds(202, 3))))[1],
            lambda: rig.logged(lambda: list(mdl.tts(stream=True, force_len=80, sampling=Sampling(seed=303), **rig.kw(1))))[1]]
    alone = [j() for j in jobs]
    assert [len(t) for t in alone[0]] == [60, 80, 75] and [len(t) for t in alone[2]] == [80]
    res, errs = [None] * 3, []

    def work(i):
        try:
            res[i] = jobs[i]()
        except Exception as e:      # noqa: BLE001
            errs.append(e)
    ths = [threading.Thread(target=work, args=(i,)) for i in range(3)]
    [t.start() for t in ths]
    [t.join(300) for t in ths]
    assert not errs, errs
    assert res == alone
    mdl._token_log = None
    assert _idle(rig)
    # abandoned while segment 0 is in work and segment 1 has been looked ahead (segment 0 is one chunk: its LLM has ended before it)
    gen = mdl.tts_continuous([rig.kw(i) for i in (0, 1, 2)], Join(pause_ms=10, trim_db=30), force_len=[40, 80, 75], sampling=_seeds(5, 3))
    first = next(gen)
    assert first['segment'] == 0 and len(mdl.cont_dict) == 1 and len(mdl._slot_free) == mdl.max_batch - 2
    gen.close()
    assert _idle(rig)
    # a look-ahead that fails while it opens segment 1 does not disturb segment 0: the failure is raised at segment 1's turn
    real, n_open = mdl._seg_open, []

    def failing(kw, *a, wait=True):
        n_open.append(wait)
        if not wait:
            raise RuntimeError('segment refused by the test')
        return real(kw, *a, wait=wait)
    mdl._seg_open = failing
    got = []
    try:
        with pytest.raises(RuntimeError, match='refused by the test'):
            for o in mdl.tts_continuous([rig.kw(i) for i in (0, 1, 2)], Join(pause_ms=10), force_len=[60, 80, 75], sampling=_seeds(5, 3)):
                got.append(o['segment'])
    finally:
        del mdl._seg_open
    assert got == [0, 0] and n_open == [True, False] and _idle(rig)
    with pytest.raises(ValueError):
        next(mdl.tts_continuous([rig.kw(0), rig.kw(1)], Join(trim_db=40, fade_ms=6)))
    with pytest.raises(ValueError):
        next(mdl.tts_continuous([rig.kw(0)], Join(pause_ms=1)))
    with pytest.raises(TypeError):
        next(mdl.tts_continuous([rig.kw(0), dict(rig.kw(1), text=(t for t in ()))], Join(pause_ms=1)))
    assert _idle(rig)


def test_the_public_view_streams_one_call(rig):
    cv = _cv(rig, segments=('un', 'deux', 'trois')).sampler(seed=7)
    plain, ptoks = rig.logged(lambda: [o['tts_speech'] for o in cv.inference_zero_shot('x', 'salut', None, zero_shot_spk_id='fr', stream=True)])
    res, ctoks = rig.logged(lambda: list(cv.continuous(pause_ms=0).inference_zero_shot('x', 'salut', None, zero_shot_spk_id='fr', stream=True)))
    assert ctoks == ptoks and len(ctoks) == 3
    assert torch.equal(torch.cat([r['tts_speech'] for r in res], dim=1), torch.cat(plain, dim=1))     # pause 0, nothing gated: the plain chunks
    assert len(res[-1]['segments']) == 3 and res[-1]['segments'][-1][1] == sum(p.shape[1] for p in plain)
    with pytest.raises(ValueError, match='joined'):
        next(cv.continuous(pause_ms=0).inference_zero_shot('x', 'salut', None, zero_shot_spk_id='fr'))
    rig.mdl._token_log = None
    assert _idle(rig)
