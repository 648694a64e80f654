"""The output level through the scheduler (cosyvoice/cli/model.py) and the public surface: a levelled call's chunks are, bit for bit, the
level kernel over the same call's plain 24 kHz signal -- streaming, under an output conversion, serial, coalesced, joined, continuous --, a
peak target lands where the definition puts it, a continuous call has one record, and with nothing set no record is made and nothing is
launched.  Synthetic weights and the fixtures of tests/test_join_api_gpu.py; seeded calls (their tokens and vocoder noise do not depend on
what else runs).  Run with -m gpu."""
import threading

import numpy as np
import pytest
import torch

import _level as R
from test_join_api_gpu import Rig, _cv, _seeds

pytestmark = pytest.mark.gpu
FORCE_LEN = 80          # prompt of 31 tokens -> first chunk 44 tokens, second 25, final 11: three chunks


@pytest.fixture(scope='module')
def rig():
    assert torch.cuda.is_available(), 'needs a GPU'
    return Rig()


def _idle(rig):
    return rig.idle() and not rig.mdl.level_dict and not rig.mdl.cont_dict


def _whole(mdl, level, wav):
    """the level kernel over a whole [1, n] CPU waveform, one launch -> [1, n] CPU"""
    return mdl._level_convert([(mdl._Level(level, mdl.device), wav.to(mdl.device), True)])[0].cpu()


def _stream(rig, sp, **extra):
    return [o['tts_speech'] for o in rig.mdl.tts(stream=True, force_len=FORCE_LEN, sampling=sp, **extra, **rig.kw(0))]


def _peak_is_at(y, s, level):
    """max |y| is fl(fl(T / P) P), the definition's value for G = 1 when nothing is over the ceiling -- within the two roundings (the
    quotient, the product: <= 2^-24 relative each) of T"""
    G, c, L, T = level.resolve()
    P = R.peak(s)
    want = np.float32(R.gain(G, P, T) * P)
    got = float(np.abs(y).max())
    print(f'peak {got!r}, target {T!r}, source peak {float(P)!r}')
    assert P > 0 and got == float(want) and abs(got - T * G) <= 2.001 * R.U * T * G


def test_streaming_call_is_the_level_of_the_plain_call(rig):
    from cv2amd.level import Level
    mdl, sp = rig.mdl, _seeds(0x1E7E1, 1)[0]
    base = _stream(rig, sp)
    whole = torch.cat(base, dim=1)
    assert len(base) == 3 and whole.shape[1] == 960 * FORCE_LEN
    for level in (Level(ceiling_db=-6), Level(gain_db=18, ceiling_db=-12, lookahead_ms=1.5)):       # (the synthetic voice peaks near 0.1: the second is limited often)
        L = level.resolve()[2]
        sizes = []
        real = mdl._run_chunks

        def watch(batch):
            sizes.append(len(mdl.level_dict))
            return real(batch)
        mdl._run_chunks = watch
        try:
            chunks = _stream(rig, sp, level=level)
        finally:
            del mdl._run_chunks
        assert sizes == [1, 1, 1], 'one record per call, made with the call'
        assert [c.shape[1] for c in chunks] == [base[0].shape[1] - L, base[1].shape[1], base[2].shape[1] + L], 'the look-ahead is held back until the end'
        got, want = torch.cat(chunks, dim=1), _whole(mdl, level, whole)
        assert torch.equal(got.view(torch.int32), want.view(torch.int32))
        ref = R.level64(whole[0].numpy(), level.resolve()[0], level.resolve()[1], L)
        print(f'{level}: {(ref["acc"] > 0).mean():.3f} of the samples within the look-ahead of an over')
        assert float(got.abs().max()) <= level.resolve()[1] and (level.gain_db is None or (ref['acc'] > 0).mean() > 0.05)
        # under an output conversion: the output record consumes what the level stage emits
        pcm = _stream(rig, sp, level=level, output_sample_rate=16000, pcm16=True)
        want16 = mdl._out_convert([(mdl._Out(16000, True, mdl.device), want.to(mdl.device), True)])[0].cpu()
        assert all(c.dtype == torch.int16 for c in pcm) and torch.equal(torch.cat(pcm, dim=1), want16)
        assert _idle(rig)


def test_abandoned_stream_and_bad_settings_leave_nothing(rig):
    from cv2amd.level import Level
    mdl = rig.mdl
    g = mdl.tts(stream=True, force_len=FORCE_LEN, level=Level(gain_db=-3), **rig.kw(0))
    first = next(g)['tts_speech']
    assert first.shape[1] > 0 and len(mdl.level_dict) == 1 and list(mdl.level_dict.values())[0].state.emitted == first.shape[1]
    assert list(mdl.level_dict.values())[0].tail.numel() == 240
    g.close()
    assert _idle(rig)
    for bad in (dict(stream=True, level=Level(peak_db=-3)), dict(level=Level(ceiling_db=2))):
        with pytest.raises(ValueError):
            next(mdl.tts(force_len=FORCE_LEN, **bad, **rig.kw(0)))
    assert _idle(rig)


def test_serial_call_with_a_peak_target(rig):
    """the one-call path (a noise hook keeps the call out of the coalesced batch): the result is the level kernel over the plain waveform"""
    from cv2amd.level import Level
    mdl, level = rig.mdl, Level(peak_db=-3)

    def run(**extra):
        cnt = [0]

        def hook(T):
            cnt[0] += 1
            return torch.randn(1, 480 * T, 9, generator=torch.Generator().manual_seed(100 + cnt[0]))
        mdl._noise_hook = hook
        try:
            (o,) = list(mdl.tts(stream=False, force_len=57, sampling=_seeds(5, 1)[0], **extra, **rig.kw(1)))
        finally:
            mdl._noise_hook = None
        return o['tts_speech']
    base, got = run(), run(level=level)
    assert got.shape == base.shape and torch.equal(got.view(torch.int32), _whole(mdl, level, base).view(torch.int32))
    _peak_is_at(got[0].numpy(), base[0].numpy(), level)
    assert _idle(rig)


def test_coalesced_batch_with_peak_targets(rig, monkeypatch):
    """3 concurrent non-streaming calls of different lengths and targets: ONE peak launch and ONE level launch over the batch's ragged
    waveforms (the vocoder's noise is drawn per call, so the plain waveforms are taken where the scheduler hands them to the stage)."""
    import cosyvoice.cli.model as M
    from cv2amd.level import Level
    mdl, seen, launches = rig.mdl, [], []
    real_convert, real_launch, real_peaks = mdl._level_convert, M.LV.level_chunks, M.LV.level_peaks

    def convert(jobs):
        seen.extend(wav.detach().clone().cpu() for _lx, wav, _f in jobs)
        return real_convert(jobs)

    def launch(args, **kw):
        launches.append(('level', len(args)))
        return real_launch(args, **kw)

    def peaks(wavs, **kw):
        launches.append(('peak', len(wavs)))
        return real_peaks(wavs, **kw)
    monkeypatch.setattr(mdl, '_level_convert', convert)
    monkeypatch.setattr(M.LV, 'level_chunks', launch)
    monkeypatch.setattr(M.LV, 'level_peaks', peaks)
    lens, levels, res, errs = (40, 57, 80), (Level(peak_db=-3), Level(peak_db=-9, ceiling_db=-6), Level(gain_db=-4)), [None] * 3, []

    def work(i):
        try:
            res[i] = [o['tts_speech'] for o in mdl.tts(stream=False, force_len=lens[i], level=levels[i], **rig.kw(i))]
        except Exception as e:      # noqa: BLE001
            errs.append(e)
    n0, old = len(mdl.batch_sizes), mdl.coalesce_ms
    mdl.coalesce_ms = 200.0
    try:
        ths = [threading.Thread(target=work, args=(i,)) for i in range(3)]
        [t.start() for t in ths]
        [t.join(300) for t in ths]
    finally:
        mdl.coalesce_ms = old
    assert not errs, errs
    assert mdl.batch_sizes[n0:] == [3] and launches == [('peak', 2), ('level', 3)] and len(seen) == 3
    wavs = {w.shape[1]: w for w in seen}
    monkeypatch.undo()
    for i, n_tok in enumerate(lens):
        (out,) = res[i]
        w = wavs[960 * n_tok]
        assert out.device.type == 'cpu' and out.shape == w.shape and torch.equal(out.view(torch.int32), _whole(mdl, levels[i], w).view(torch.int32))
        if levels[i].peak_db is not None:
            _peak_is_at(out[0].numpy(), w[0].numpy(), levels[i])
    assert _idle(rig)


def test_joined_call_is_levelled_once(rig):
    from cv2amd.join import Join
    from cv2amd.level import Level
    mdl, join, sp, level = rig.mdl, Join(pause_ms=20), _seeds(0x10E1, 3), Level(peak_db=-2, lookahead_ms=10)
    base, _ = rig.joined([0, 1, 2], join, sampling=sp)
    out, _ = rig.joined([0, 1, 2], join, sampling=sp, level=level)
    assert out['segments'] == base['segments'] and out['tts_speech'].shape == base['tts_speech'].shape
    assert torch.equal(out['tts_speech'].view(torch.int32), _whole(mdl, level, base['tts_speech']).view(torch.int32))
    _peak_is_at(out['tts_speech'][0].numpy(), base['tts_speech'][0].numpy(), level)
    pcm, _ = rig.joined([0, 1, 2], join, sampling=sp, level=level, output_sample_rate=8000, pcm16=True)
    want = mdl._out_convert([(mdl._Out(8000, True, mdl.device), out['tts_speech'].to(mdl.device), True)])[0].cpu()
    assert torch.equal(pcm['tts_speech'], want)
    mdl._token_log = None
    assert _idle(rig)


def test_continuous_call_has_one_record(rig):
    from cv2amd.join import Join
    from cv2amd.level import Level
    mdl, join, sp, level, fl = rig.mdl, Join(pause_ms=10), _seeds(0xC0, 2), Level(gain_db=6, ceiling_db=-9), [60, 75]
    base = list(mdl.tts_continuous([rig.kw(0), rig.kw(1)], join, force_len=fl, sampling=sp))
    whole = torch.cat([r['tts_speech'] for r in base], dim=1)
    res, total = [], 0
    for r in mdl.tts_continuous([rig.kw(0), rig.kw(1)], join, force_len=fl, sampling=sp, level=level):
        total += r['tts_speech'].shape[1]
        assert len(mdl.level_dict) == 1 and list(mdl.level_dict.values())[0].state.emitted == total, 'ONE record over the whole signal'
        res.append(r)
    assert len(res) == len(base) and res[-1]['segments'] == base[-1]['segments'] and [r['segment'] for r in res] == [r['segment'] for r in base]
    got = torch.cat([r['tts_speech'] for r in res], dim=1)
    assert torch.equal(got.view(torch.int32), _whole(mdl, level, whole).view(torch.int32))
    with pytest.raises(ValueError):
        next(mdl.tts_continuous([rig.kw(0), rig.kw(1)], join, force_len=fl, level=Level(peak_db=-3)))
    assert _idle(rig)


def test_nothing_set_takes_the_previous_path(rig, monkeypatch):
    import cosyvoice.cli.model as M
    from cv2amd.level import Level
    mdl, sp, sizes = rig.mdl, _seeds(0x1E7E1, 1)[0], []
    base = _stream(rig, sp)

    def no_launch(*a, **k):
        raise AssertionError('a call without level settings must not launch the level stage')
    monkeypatch.setattr(M.LV, 'level_chunks', no_launch)
    monkeypatch.setattr(M.LV, 'level_peaks', no_launch)
    real = mdl._run_chunks

    def watch(batch):
        sizes.append(len(mdl.level_dict))
        return real(batch)
    monkeypatch.setattr(mdl, '_run_chunks', watch)
    for kw in (dict(), dict(level=None), dict(level=Level())):
        sizes.clear()
        chunks = _stream(rig, sp, **kw)
        assert sizes == [0, 0, 0] and not mdl.level_dict
        assert len(chunks) == 3 and all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(chunks, base))
    (a,) = list(mdl.tts(stream=False, force_len=40, sampling=sp, **rig.kw(0)))
    (b,) = list(mdl.tts(stream=False, force_len=40, sampling=sp, level=Level(), **rig.kw(0)))
    assert torch.equal(a['tts_speech'], b['tts_speech'])
    assert _idle(rig)


def test_public_view(rig):
    """CosyVoice2.level(...): the view's streaming call is the level of the plain view's, and with nothing set the view is the plain object"""
    from cv2amd.level import Level
    cv = _cv(rig).sampler(seed=7)
    level = Level(gain_db=3, ceiling_db=-6)
    base = [o['tts_speech'] for o in cv.inference_zero_shot('bonjour', 'salut', None, zero_shot_spk_id='fr', stream=True)]
    same = [o['tts_speech'] for o in cv.level().inference_zero_shot('bonjour', 'salut', None, zero_shot_spk_id='fr', stream=True)]
    got = [o['tts_speech'] for o in cv.level(gain_db=3, ceiling_db=-6).inference_zero_shot('bonjour', 'salut', None, zero_shot_spk_id='fr', stream=True)]
    assert len(same) == len(base) and all(torch.equal(a, b) for a, b in zip(same, base))
    whole = torch.cat(base, dim=1)
    assert torch.equal(torch.cat(got, dim=1).view(torch.int32), _whole(rig.mdl, level, whole).view(torch.int32))
    with pytest.raises(ValueError):
        next(cv.level(peak_db=-3).inference_zero_shot('bonjour', 'salut', None, zero_shot_spk_id='fr', stream=True))
    assert _idle(rig)
