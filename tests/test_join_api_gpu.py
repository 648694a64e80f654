"""Joined calls through the scheduler and the public surface: synthetic weights (2-layer LLM, full-size flow and HiFT),
short texts.  Run with -m gpu on an MI355X."""
import threading

import numpy as np
import pytest
import torch

import _join as R

pytestmark = pytest.mark.gpu
LENS = (40, 57, 80, 33, 61, 30, 72, 45, 50, 38)         # forced speech-token counts of up to 10 segments (960 samples per token)


class Rig:
    def __init__(self):
        from cv2amd import synth
        from cosyvoice.cli.model import CosyVoice2Model
        self.sds = (synth.make_llm(layers=2), synth.make_flow(), synth.make_hift())
        self.mdl = CosyVoice2Model(*self.sds, max_batch=8, max_text=64, max_prompt_tokens=64, max_new_tokens=256, sampling='ras')
        self.inps = [synth.synthetic_inputs(seed=1 + i, text_len=23 - 3 * i, prompt_len=31, prompt_text_len=6) for i in range(3)]
        # voices with a short prompt: 2 * (16 + 33) = 98 frames fit ONE 128-row panel of the flow (see the sharing test)
        self.short = [synth.synthetic_inputs(seed=11 + i, text_len=23 - 3 * i, prompt_len=16, prompt_text_len=6) for i in range(3)]

    def kw(self, i=0, short=False):
        inp = (self.short if short else self.inps)[i % 3]
        return dict(text=inp['text'], flow_embedding=inp['embedding'], llm_embedding=inp['embedding'], prompt_text=inp['prompt_text'],
                    llm_prompt_speech_token=inp['prompt_token'], flow_prompt_speech_token=inp['prompt_token'], prompt_speech_feat=inp['prompt_feat'])

    def logged(self, run):
        """run() with the scheduler's token log on: (its result, the speech tokens of the calls it started in this thread, in order)"""
        mdl, mine, me = self.mdl, [], threading.get_ident()
        mdl._token_log = {} if mdl._token_log is None else mdl._token_log
        old = mdl._on_call

        def on_call(u):
            if threading.get_ident() == me:
                mine.append(u)
            if old is not None:
                old(u)
        mdl._on_call = on_call
        try:
            res = run()
        finally:
            mdl._on_call = old
        return res, [mdl._token_log.get(u) for u in mine]

    def plain(self, i, force_len, **extra):
        """segment i as a plain non-streaming call -> (waveform, tokens)"""
        (out,), (toks,) = self.logged(lambda: list(self.mdl.tts(stream=False, force_len=force_len, **extra, **self.kw(i))))
        return out['tts_speech'], toks

    def joined(self, idx, join, lens=None, **extra):
        """the segments idx as ONE joined call -> (the one dict, tokens per segment)"""
        lens = list(lens or [LENS[j] for j in range(len(idx))])
        (out,), toks = self.logged(lambda: list(self.mdl.tts_joined([self.kw(i) for i in idx], join, force_len=lens, **extra)))
        return out, toks

    def idle(self):
        m = self.mdl
        return (not m.samp_dict and not m.out_dict and not m.hift_cache_dict and not m.solver_dict and not m.tts_speech_token_dict
                and not m.llm_end_dict and not m._pending and sorted(m._slot_free) == list(range(m.max_batch)))


@pytest.fixture(scope='module')
def rig():
    assert torch.cuda.is_available(), 'needs a GPU'
    return Rig()


def _cv(rig, segments=None):
    from cosyvoice.cli.cosyvoice import CosyVoice2
    from cosyvoice.cli.frontend import PrecomputedFrontEnd
    inp = rig.inps[0]
    spk = {'prompt_text': inp['prompt_text'], 'prompt_text_len': torch.tensor([6]), 'llm_prompt_speech_token': inp['prompt_token'],
           'llm_prompt_speech_token_len': torch.tensor([31]), 'flow_prompt_speech_token': inp['prompt_token'],
           'flow_prompt_speech_token_len': torch.tensor([31]), 'prompt_speech_feat': inp['prompt_feat'],
           'prompt_speech_feat_len': torch.tensor([62]), 'llm_embedding': inp['embedding'], 'flow_embedding': inp['embedding']}

    class FE(PrecomputedFrontEnd):
        def text_normalize(self, text, split=True, **kw):
            return list(segments) if (split and segments) else super().text_normalize(text, split=split, **kw)
    cv = CosyVoice2.__new__(CosyVoice2)
    cv.output_sample_rate, cv.output_pcm16, cv.model_sample_rate, cv.sampling, cv.model_dir, cv.fp16 = None, False, 24000, None, 'unused', False
    cv.model, cv.frontend = rig.mdl, FE(lambda t: [1, 2, 3, 4, 5, 6, 7, 8][:5 + len(t)], {'fr': spk})
    return cv


def _seeds(seed, k):
    from cv2amd.sampling import Sampling
    return [Sampling(seed=seed).for_segment(i) for i in range(k)]


def test_three_segments_run_as_one_batch_and_equal_the_plain_calls(rig):
    """A seeded joined call of three segments, pause 0, no trim: ONE batch of three; every segment's tokens are those of the same segment
    as a plain seeded call, and the waveform is torch.cat of the three plain waveforms (a seeded call's draws do not
    depend on what shares its batch).  Through the scheduler with forced lengths, then through the public view, free-running."""
    from cv2amd.join import Join
    mdl = rig.mdl
    sp = _seeds(0x5EED2024, 3)
    want = [rig.plain(i, LENS[i], sampling=sp[i]) for i in range(3)]
    n0 = len(mdl.batch_sizes)
    out, toks = rig.joined([0, 1, 2], Join(pause_ms=0), sampling=sp)
    assert mdl.batch_sizes[n0:] == [3]
    assert toks == [t for _, t in want] and [len(t) for t in toks] == list(LENS[:3])
    assert set(out) == {'tts_speech', 'segments'} and out['tts_speech'].device.type == 'cpu' and out['tts_speech'].dtype == torch.float32
    assert torch.equal(out['tts_speech'], torch.cat([w for w, _ in want], dim=1))
    assert out['segments'] == [(0, 960 * 40), (960 * 40, 960 * 97), (960 * 97, 960 * 177)]
    # the public surface: the plain view yields the segments one by one, the joined view their concatenation
    cv = _cv(rig, segments=('un', 'deux', 'trois')).sampler(seed=7)
    n0 = len(mdl.batch_sizes)
    plain, ptoks = rig.logged(lambda: [o['tts_speech'] for o in cv.inference_zero_shot('x', 'salut', None, zero_shot_spk_id='fr')])
    assert mdl.batch_sizes[n0:] == [1, 1, 1] and len(plain) == 3
    n0 = len(mdl.batch_sizes)
    (one,), jtoks = rig.logged(lambda: list(cv.joined(pause_ms=0).inference_zero_shot('x', 'salut', None, zero_shot_spk_id='fr')))
    assert mdl.batch_sizes[n0:] == [3]
    assert jtoks == ptoks and all(len(t) >= 10 for t in jtoks)
    # (free-running lengths: the batch of three may cross a block-count switch of the flow attention, beyond which DESIGN.md section 1
    # promises the tokens but not the waveform's bits -- the waveform is held bit for bit above, at forced lengths)
    ends = np.cumsum([960 * len(t) for t in jtoks]).tolist()
    assert one['tts_speech'].shape == (1, ends[-1]) and one['segments'] == list(zip([0] + ends[:-1], ends))
    assert [w.shape[1] for w in plain] == [960 * len(t) for t in ptoks]
    mdl._token_log = None
    assert rig.idle()


def test_ten_segments_run_as_two_batches(rig):
    from cv2amd.join import Join
    mdl = rig.mdl
    n0 = len(mdl.batch_sizes)
    res = list(mdl.tts_joined([rig.kw(i) for i in range(10)], Join(pause_ms=12.5), force_len=list(LENS), sampling=_seeds(5, 10), device_output=True))
    assert mdl.batch_sizes[n0:] == [8, 2] and len(res) == 1
    wav, seg = res[0]['tts_speech'], res[0]['segments']
    assert wav.is_cuda and wav.shape == (1, 960 * sum(LENS) + 9 * 300)
    assert len(seg) == 10 and seg[0][0] == 0 and seg[-1][1] == wav.shape[1]
    assert [e - s for s, e in seg] == [960 * n for n in LENS] and all(seg[i + 1][0] - seg[i][1] == 300 for i in range(9))
    gaps = torch.cat([wav[0, seg[i][1]:seg[i + 1][0]] for i in range(9)])
    assert int(gaps.view(torch.int32).abs().sum()) == 0                       # +0.0 exactly
    assert all(bool(wav[0, s:e].abs().max() > 0) for s, e in seg)
    assert rig.idle()


def test_output_conversion_runs_once_over_the_joined_signal(rig):
    from cv2amd.join import Join
    mdl = rig.mdl
    sp, j = _seeds(31, 3), Join(pause_ms=7)
    f24, _ = rig.joined([0, 1, 2], j, sampling=sp)
    conv, calls = [], mdl._out_convert
    mdl._out_convert = lambda jobs: (conv.append(len(jobs)), calls(jobs))[1]
    try:
        out, _ = rig.joined([0, 1, 2], j, sampling=sp, output_sample_rate=16000, pcm16=True)
    finally:
        del mdl._out_convert
    assert conv == [1]                                                        # one record, once
    N = f24['tts_speech'].shape[1]
    assert N == 960 * sum(LENS[:3]) + 2 * 168 and out['segments'] == f24['segments']
    want = mdl._out_convert([(mdl._Out(16000, True, mdl.device), f24['tts_speech'].to(mdl.device), True)])[0].cpu()
    assert out['tts_speech'].dtype == torch.int16 and out['tts_speech'].shape == (1, -(-N * 2 // 3))
    assert torch.equal(out['tts_speech'], want)
    assert rig.idle()


def test_trim_pause_and_fade_equal_the_restatement(rig, monkeypatch):
    """The vocoder replaced by crafted waveforms (silence - speech - silence): the joined call's result is the numpy restatement's."""
    from cv2amd.join import Join
    mdl = rig.mdl
    rng = np.random.default_rng(21)
    segs = []
    for n, lo, hi in ((24000, 3000, 20000), (18001, 4000, 9000), (9999, 0, 5000), (30000, 12000, 30000)):
        x = (rng.standard_normal(n) * 1e-4).astype(np.float32)
        x[lo:hi] = (rng.standard_normal(hi - lo) * 0.3).astype(np.float32)
        segs.append(x)

    def crafted(mels, seeds=None):
        assert len(mels) == len(segs)
        return [(torch.from_numpy(s).to(mdl.device).unsqueeze(0), None) for s in segs]
    monkeypatch.setattr(mdl.hift_pool, 'inference_many', crafted)
    for join, (pause, F, db) in ((Join(pause_ms=20, trim_db=40), (480, 120, 40)), (Join(trim_db=26.5, fade_ms=0), (3600, 0, 26.5)),
                                 (Join(pause_ms=0, trim_db=60, fade_ms=20), (0, 480, 60)), (Join(pause_ms=1), (24, 0, None))):
        out, _ = rig.joined([0, 1, 2, 0], join, lens=[30, 31, 32, 33])
        bnds = R.bounds(segs, None if db is None else R.gain(db))
        want, spans = R.join(segs, bnds, pause, F)
        assert out['segments'] == spans
        assert torch.equal(out['tts_speech'].view(torch.int32), torch.from_numpy(want).view(torch.int32).unsqueeze(0)), join
        if db is not None:                                                    # the seams lost their silence, the call's own edges did not
            assert bnds[0][0] == 0 and bnds[-1][1] == 30000 and bnds[1] == (3840 - 480, 9120 + 480) and want.size < sum(s.size for s in segs)
    assert rig.idle()


def test_one_failing_segment_fails_the_call_and_leaves_nothing_behind(rig, monkeypatch):
    from cv2amd.join import Join
    mdl = rig.mdl
    real = mdl.flow.inference_batch

    def failing(utts, **kw):
        if any(u['token'].shape[1] == 57 for u in utts):
            raise RuntimeError('flow: utterance refused by the test')
        return real(utts, **kw)
    monkeypatch.setattr(mdl.flow, 'inference_batch', failing)
    got = []
    with pytest.raises(RuntimeError, match='refused by the test'):
        for o in mdl.tts_joined([rig.kw(i) for i in range(3)], Join(pause_ms=0), force_len=[40, 57, 80]):
            got.append(o)
    assert got == [] and rig.idle()
    monkeypatch.undo()
    out, _ = rig.joined([0, 1, 2], Join(pause_ms=0))                          # the model serves the next call
    assert out['tts_speech'].shape[1] == 960 * 177 and rig.idle()
    with pytest.raises(ValueError):
        next(mdl.tts_joined([rig.kw(0), rig.kw(1)], Join(trim_db=10)))
    with pytest.raises(ValueError):
        next(mdl.tts_joined([rig.kw(0), rig.kw(1)], Join()))
    assert rig.idle()


def test_two_joined_calls_and_a_plain_call_share_batches(rig):
    """Each call's audio equals the same call run alone, bit for bit.  DESIGN.md section 1 promises a seeded call's waveform whatever
    shares its batch only while the flow batch stays under the attention's block-count switch: the estimator packs every utterance twice
    (both guidance branches) into panels of 128 rows, ceil((frames + 8) / 128) of them, and changes its summation order from 2112 rows on.
    With the 31-token prompt of the other tests an utterance of 30 tokens has 122 frames = two panels, and five of them cross the switch
    (measured: a batch of 4 equals the calls alone, batches of 5, 6 and 7 differ from them by up to 7e-2 in the waveform with equal
    tokens).  So the voices here have a 16-token prompt: 30 .. 33 tokens are at most 98 frames = one panel, and the seven utterances of
    the shared batch are 1792 rows."""
    from cv2amd.join import Join
    from cv2amd.sampling import Sampling
    mdl = rig.mdl
    ja, jb = Join(pause_ms=10), Join(pause_ms=0, trim_db=50)
    jobs = [lambda: list(mdl.tts_joined([rig.kw(i, short=True) for i in (0, 1, 2)], ja, force_len=[30, 31, 32], sampling=_seeds(101, 3)))[0],
            lambda: list(mdl.tts_joined([rig.kw(i, short=True) for i in (2, 1, 0)], jb, force_len=[33, 30, 31], sampling=_seeds(202, 3)))[0],
            lambda: list(mdl.tts(stream=False, force_len=32, sampling=Sampling(seed=303), **rig.kw(1, short=True)))[0]]
    alone = [j() for j in jobs]
    res, errs = [None] * 3, []

    def work(i):
        try:
            res[i] = jobs[i]()
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
    assert sum(mdl.batch_sizes[n0:]) == 7 and len(mdl.batch_sizes[n0:]) < 7
    for a, r in zip(alone, res):
        assert torch.equal(a['tts_speech'], r['tts_speech']) and a.get('segments') == r.get('segments')
    mdl._token_log = None
    assert rig.idle()


def test_one_segment_is_the_plain_call(rig, monkeypatch):
    from cv2amd import join as J
    mdl = rig.mdl
    calls = []
    for name in ('wave_bounds', 'wave_join'):
        real = getattr(J, name)
        monkeypatch.setattr(J, name, lambda *a, _r=real, _n=name, **k: (calls.append(_n), _r(*a, **k))[1])
    cv = _cv(rig).sampler(seed=7)
    (p,) = list(cv.inference_zero_shot('bonjour', 'salut', None, zero_shot_spk_id='fr'))
    n0 = len(mdl.batch_sizes)
    (q,) = list(cv.joined(pause_ms=100, trim_db=40).inference_zero_shot('bonjour', 'salut', None, zero_shot_spk_id='fr'))
    assert set(q) == {'tts_speech'} and torch.equal(p['tts_speech'], q['tts_speech']) and mdl.batch_sizes[n0:] == [1] and calls == []
    with pytest.raises(ValueError):
        next(cv.joined(pause_ms=100).inference_zero_shot('bonjour', 'salut', None, zero_shot_spk_id='fr', stream=True))
    # ... and the wrapped bindings do count: two segments, trimmed
    cv2 = _cv(rig, segments=('un', 'deux')).sampler(seed=7)
    (r,) = list(cv2.joined(pause_ms=100, trim_db=40).inference_zero_shot('x', 'salut', None, zero_shot_spk_id='fr'))
    assert calls == ['wave_bounds', 'wave_join'] and len(r['segments']) == 2
    assert rig.idle()
