"""Per-call sampler settings and seeds through the scheduler and the public surface: synthetic weights (2-layer LLM,
full-size flow and HiFT), short texts.  Run with -m gpu on an MI355X."""
import threading
import time

import pytest
import torch

pytestmark = pytest.mark.gpu
FORCE_LEN = 80          # prompt of 31 tokens -> first chunk 44 tokens, second 25, final 11: three chunks


class Rig:
    def __init__(self):
        from cv2amd import synth
        from cosyvoice.cli.model import CosyVoice2Model
        self.sds = (synth.make_llm(layers=2), synth.make_flow(), synth.make_hift())
        self.mdl = CosyVoice2Model(*self.sds, max_batch=8, max_text=64, max_prompt_tokens=64, max_new_tokens=256, sampling='ras')
        self.inps = [synth.synthetic_inputs(seed=1 + i, text_len=23 - 3 * i, prompt_len=31, prompt_text_len=6) for i in range(3)]

    def kw(self, i=0):
        inp = self.inps[i]
        return dict(text=inp['text'], flow_embedding=inp['embedding'], llm_embedding=inp['embedding'], prompt_text=inp['prompt_text'],
                    llm_prompt_speech_token=inp['prompt_token'], flow_prompt_speech_token=inp['prompt_token'], prompt_speech_feat=inp['prompt_feat'])

    def call(self, i=0, stream=True, force_len=FORCE_LEN, **extra):
        """one tts() call: (chunks, its speech tokens where the scheduler logs them)"""
        mdl, mine = self.mdl, []
        mdl._token_log = {} if mdl._token_log is None else mdl._token_log
        seen = threading.local()
        old = mdl._on_call

        def on_call(u):
            if getattr(seen, 'armed', False):
                mine.append(u)
                seen.armed = False
            if old is not None:
                old(u)
        mdl._on_call = on_call
        seen.armed = True
        try:
            chunks = [o['tts_speech'] for o in mdl.tts(stream=stream, force_len=force_len, **extra, **self.kw(i))]
        finally:
            mdl._on_call = old
        return chunks, mdl._token_log.get(mine[0]) if mine else None

    def together(self, jobs, one_prefill=False):
        """the jobs (dicts of call() arguments) started together from threads; results in order.  one_prefill: the prefill queue is held
        shut until every job has queued its prompt, so that ONE batched prefill serves them all"""
        res, errs = [None] * len(jobs), []
        mdl = self.mdl
        mdl._token_log = {}
        uu = [None] * len(jobs)
        tl = threading.local()
        mdl._on_call = lambda u: uu.__setitem__(tl.i, u)

        def work(i):
            tl.i = i
            try:
                j = dict(jobs[i])
                k = j.pop('i', 0)
                res[i] = [o['tts_speech'] for o in mdl.tts(stream=j.pop('stream', True), force_len=j.pop('force_len', FORCE_LEN), **j, **self.kw(k))]
            except Exception as e:      # noqa: BLE001
                errs.append(e)
        try:
            ths = [threading.Thread(target=work, args=(i,)) for i in range(len(jobs))]
            if one_prefill:
                with mdl._prefill_lock:
                    [t.start() for t in ths]
                    t_end = time.perf_counter() + 60.0
                    while len(mdl._prefill_q) < len(jobs) and not errs and time.perf_counter() < t_end:
                        time.sleep(0.0005)
                    assert len(mdl._prefill_q) == len(jobs) or errs
            else:
                [t.start() for t in ths]
            [t.join(300) for t in ths]
        finally:
            mdl._on_call = None
        assert not errs, errs
        return [(res[i], mdl._token_log.get(uu[i])) for i in range(len(jobs))]

    def idle(self):
        m = self.mdl
        return not m.samp_dict and not m.out_dict and not m.hift_cache_dict and sorted(m._slot_free) == list(range(m.max_batch))


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
    cv.model, cv.frontend = rig.mdl, FE(lambda t: [1, 2, 3, 4, 5, 6, 7, 8], {'fr': spk})
    return cv


def test_seeded_public_call_is_reproducible_and_unseeded_calls_keep_the_counter(rig):
    mdl = rig.mdl
    cv = _cv(rig)
    mdl._token_log = {}
    a = [o['tts_speech'] for o in cv.sampler(seed=7).inference_zero_shot('bonjour', 'salut', None, zero_shot_spk_id='fr', stream=True)]
    b = [o['tts_speech'] for o in cv.sampler(seed=7).inference_zero_shot('bonjour', 'salut', None, zero_shot_spk_id='fr', stream=True)]
    ta, tb = list(mdl._token_log.values())
    assert ta == tb and len(ta) >= 16
    assert len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))
    c = [o['tts_speech'] for o in cv.sampler(seed=8).inference_zero_shot('bonjour', 'salut', None, zero_shot_spk_id='fr', stream=True)]
    assert list(mdl._token_log.values())[2] != ta
    # non-streaming (the coalesced batch): reproducible too, in the 16 kHz int16 view as well
    (p,) = list(cv.sampler(seed=7).inference_zero_shot('bonjour', 'salut', None, zero_shot_spk_id='fr'))
    (q,) = list(cv.sampler(seed=7).inference_zero_shot('bonjour', 'salut', None, zero_shot_spk_id='fr'))
    assert torch.equal(p['tts_speech'], q['tts_speech']) and p['tts_speech'].shape[1] == 960 * len(ta)
    (r,) = list(cv.sampler(seed=7).output(sample_rate=16000, pcm16=True).inference_zero_shot('bonjour', 'salut', None, zero_shot_spk_id='fr'))
    assert r['tts_speech'].dtype == torch.int16 and r['tts_speech'].shape[1] == 640 * len(ta)
    # unseeded calls: the model's counter advances as before, one per LLM start, and consecutive calls differ
    s0 = mdl.seed
    mdl._token_log = {}
    for _ in range(2):
        list(cv.inference_zero_shot('bonjour', 'salut', None, zero_shot_spk_id='fr', stream=True))
    assert mdl.seed == s0 + 2
    u, v = list(mdl._token_log.values())
    assert u != v
    # a seeded call does not consume from the unseeded calls' noise: the counter moved for it as for any call, nothing else
    mdl._token_log = None
    assert rig.idle()
    del c


def test_seeded_stream_alone_and_beside_two_other_streams(rig):
    """The seeded call alone, then started together with two other streaming calls of other voices: equal tokens, chunk boundaries and
    waveform; the same without streaming through a coalesced batch of three.  (By margin, DESIGN.md section 1: logits of different decode
    forms agree to ~5e-6 of the maximum, so a draw on a cdf boundary could differ -- none does for this seed.)"""
    from cv2amd.sampling import Sampling
    mdl = rig.mdl
    sp = Sampling(seed=0x5EED2024)
    alone, toks = rig.call(0, sampling=sp)
    assert len(alone) == 3 and len(toks) == FORCE_LEN
    got = rig.together([dict(i=1), dict(i=0, sampling=sp), dict(i=2, sampling=Sampling(seed=3))])
    chunks, toks2 = got[1]
    assert toks2 == toks
    assert [c.shape for c in chunks] == [c.shape for c in alone]
    assert torch.equal(torch.cat(chunks, dim=1), torch.cat(alone, dim=1))
    assert got[0][1] != toks and got[2][1] != toks
    # non-streaming: alone, then one of a coalesced batch of three
    (one,), _ = rig.call(0, stream=False, sampling=sp)
    n0, old = len(mdl.batch_sizes), mdl.coalesce_ms
    mdl.coalesce_ms = 200.0
    try:
        res = rig.together([dict(i=1, stream=False, force_len=40), dict(i=2, stream=False, force_len=57, sampling=Sampling(top_k=3)),
                            dict(i=0, stream=False, sampling=sp)])
    finally:
        mdl.coalesce_ms = old
    assert mdl.batch_sizes[n0:] == [3]
    assert torch.equal(res[2][0][0], one) and one.shape[1] == 960 * FORCE_LEN
    assert rig.idle()


def test_concurrent_calls_with_settings_but_no_seed_draw_apart(rig):
    """Two calls of the SAME text and voice that set sampler settings but no seed, served by one batched prefill and then by one coalesced
    batch: each group runs under one counter seed of the model, so only the slot in Philox counter word 0 keeps the calls' uniforms
    apart -- their tokens must differ, as those of two calls without any settings do."""
    from cv2amd.sampling import Sampling
    mdl = rig.mdl
    for settings in (dict(temperature=0.8), dict(top_k=25)):
        mdl._sched_log = []
        try:
            (_, ta), (_, tb) = rig.together([dict(i=0, sampling=Sampling(**settings)), dict(i=0, sampling=Sampling(**settings))], one_prefill=True)
            prefills = [info['n'] for _, kind, info in mdl._sched_log if kind == 'prefill']
        finally:
            mdl._sched_log = None
        assert prefills == [2]
        assert len(ta) == len(tb) == FORCE_LEN and ta != tb, settings
        n0, old = len(mdl.batch_sizes), mdl.coalesce_ms
        mdl.coalesce_ms = 200.0
        try:
            (_, ta), (_, tb) = rig.together([dict(i=0, stream=False, sampling=Sampling(**settings)), dict(i=0, stream=False, sampling=Sampling(**settings))])
        finally:
            mdl.coalesce_ms = old
        assert mdl.batch_sizes[n0:] == [2]
        assert len(ta) == len(tb) == FORCE_LEN and ta != tb, settings
    mdl._token_log = None
    assert rig.idle()


def test_two_segments_under_one_seed_do_not_repeat_each_other(rig):
    mdl = rig.mdl
    cv = _cv(rig, segments=('bonjour', 'bonjour'))                 # the same text twice: only the stream index tells the segments apart
    runs = []
    for _ in range(2):
        mdl._token_log = {}
        wavs = [o['tts_speech'] for o in cv.sampler(seed=11).inference_zero_shot('x', 'salut', None, zero_shot_spk_id='fr', stream=True)]
        runs.append((list(mdl._token_log.values()), wavs))
    (t0, w0), (t1, w1) = runs
    assert len(t0) == 2 and t0[0] != t0[1]
    assert t0 == t1 and len(w0) == len(w1) and all(torch.equal(a, b) for a, b in zip(w0, w1))
    mdl._token_log = None


def test_settings_change_the_tokens_of_a_seeded_call(rig):
    from cv2amd.sampling import Sampling
    mdl = rig.mdl
    _, base = rig.call(0, sampling=Sampling(seed=21))
    _, cold = rig.call(0, sampling=Sampling(seed=21, temperature=0.5))
    _, k1a = rig.call(0, sampling=Sampling(seed=21, top_k=1))
    _, k1b = rig.call(0, sampling=Sampling(seed=22, top_k=1))
    assert base != cold and base != k1a
    # top_k = 1 is the per-step argmax of the nucleus: the same across seeds until a repetition re-draw
    n = next((i for i, (x, y) in enumerate(zip(k1a, k1b)) if x != y), len(k1a))
    assert n >= 1 and k1a[:n] == k1b[:n]
    _, g = rig.call(0, sampling=Sampling(greedy=True))
    old = mdl.sampling_mode
    mdl.sampling_mode = 0
    try:
        _, want = rig.call(0)
    finally:
        mdl.sampling_mode = old
    assert g == want
    assert rig.idle()


def test_a_view_with_nothing_set_writes_no_record(rig, monkeypatch):
    from cv2amd import lib as L
    from cv2amd.sampling import Sampling
    mdl = rig.mdl
    calls = []
    real = mdl.llm.lib.cv2_llm_set_sampling

    def counting(*a):
        calls.append(a[1])
        return real(*a)
    monkeypatch.setattr(mdl.llm.lib, 'cv2_llm_set_sampling', counting)
    cv = _cv(rig)
    assert cv.sampler().sampling is None
    mdl.llm.state[:, L.ST_SAMP] = 0                                # (earlier seeded calls left their rows behind; every slot is idle here)
    list(cv.sampler().inference_zero_shot('bonjour', 'salut', None, zero_shot_spk_id='fr', stream=True))
    rig.call(0, sampling=Sampling())
    rig.call(0, stream=False, sampling=Sampling())
    assert calls == [] and int(mdl.llm.state[:, L.ST_SAMP].sum()) == 0
    rig.call(0, sampling=Sampling(seed=1))
    assert len(calls) == 1 and int(mdl.llm.state[calls[0], L.ST_SAMP]) == 1
    with pytest.raises(ValueError):
        next(mdl.tts(stream=True, force_len=FORCE_LEN, sampling=Sampling(top_k=26), **rig.kw(0)))
    assert rig.idle()
