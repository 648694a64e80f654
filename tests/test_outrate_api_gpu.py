"""output_sample_rate / pcm16 through the scheduler (cosyvoice/cli/model.py) and the public surface: a call's converted chunks are,
bit for bit, cv2_resample (the existing kernel) of the same call's default-rate chunks, streaming or not, with speed, batched or alone;
the defaults take the path without the arguments.  Synthetic weights, greedy sampler, vocoder noise injected.  Run with -m gpu."""
import os
import sys
import threading

import numpy as np
import pytest
import torch

import _outrate as R

pytestmark = pytest.mark.gpu

FORCE_LEN = 80          # prompt of 31 tokens -> first chunk 44 tokens, second 25, final 11: three chunks, 160 frames


def _resample(wav, rate):
    """cv2_resample of a whole [1, n] CPU waveform -> [1, ceil(n up / down)] CPU"""
    from cv2amd import lib as L, outrate as O, prompt
    if rate == 24000:
        return wav.clone()
    lib = L.lib()
    prompt._bind(lib)
    up, down, klen, width = O.filter_shape(rate)
    x, k = wav.reshape(-1).cuda().contiguous(), O.kernel_table('cuda', rate)
    out = torch.empty(R.n_out(x.numel(), rate), dtype=torch.float32, device='cuda')
    L.check(lib.cv2_resample(x.data_ptr(), x.numel(), k.data_ptr(), up, down, klen, width, out.data_ptr(), out.numel(), L.stream_ptr()))
    return out.cpu().unsqueeze(0)


def _pcm(wav):
    return torch.from_numpy(R.pcm16(wav.numpy()))


class Rig:
    def __init__(self):
        from cv2amd import synth
        from cosyvoice.cli.model import CosyVoice2Model
        self.sds = (synth.make_llm(layers=2), synth.make_flow(), synth.make_hift())
        self.mdl = CosyVoice2Model(*self.sds, max_batch=8, max_text=64, max_prompt_tokens=64, max_new_tokens=256, sampling='greedy')
        inp = self.inp = synth.synthetic_inputs(seed=1, text_len=23, prompt_len=31, prompt_text_len=6)
        self.kw = dict(flow_embedding=inp['embedding'], llm_embedding=inp['embedding'], prompt_text=inp['prompt_text'],
                       llm_prompt_speech_token=inp['prompt_token'], flow_prompt_speech_token=inp['prompt_token'], prompt_speech_feat=inp['prompt_feat'])
        self._base = {}

    def run(self, stream=True, speed=1.0, **out):
        """one call alone with injected noise: its chunks"""
        mdl, cnt = self.mdl, [0]

        def hook(T):
            cnt[0] += 1
            return torch.randn(1, 480 * T, 9, generator=torch.Generator().manual_seed(100 + cnt[0]))
        mdl._noise_hook, mdl.seed = hook, 1986
        try:
            return [o['tts_speech'] for o in mdl.tts(text=self.inp['text'], stream=stream, speed=speed, force_len=FORCE_LEN, **out, **self.kw)]
        finally:
            mdl._noise_hook = None

    def base(self, stream=True, speed=1.0):
        """the same call at the default rate and format (computed once)"""
        if (stream, speed) not in self._base:
            self._base[(stream, speed)] = self.run(stream, speed)
        return self._base[(stream, speed)]

    def idle(self):
        m = self.mdl
        return not m.out_dict and not m.stretch_dict and not m.hift_cache_dict and sorted(m._slot_free) == list(range(m.max_batch))


@pytest.fixture(scope='module')
def rig():
    assert torch.cuda.is_available(), 'needs a GPU'
    return Rig()


@pytest.mark.parametrize('pcm16', (False, True))
@pytest.mark.parametrize('rate', (16000, 44100))
def test_streaming(rig, rate, pcm16):
    base = rig.base()
    assert len(base) == 3 and all(c.shape[1] > 0 for c in base)
    chunks = rig.run(output_sample_rate=rate, pcm16=pcm16)
    assert len(chunks) == 3 and all(c.dim() == 2 and c.shape[0] == 1 and c.device.type == 'cpu' for c in chunks) and chunks[-1].shape[1] > 0
    got, want = torch.cat(chunks, dim=1), _resample(torch.cat(base, dim=1), rate)
    n = sum(c.shape[1] for c in base)
    _, up, down, _, _ = R.table(rate)
    assert got.shape[1] == -(-n * up // down)
    if pcm16:
        assert all(c.dtype == torch.int16 for c in chunks) and torch.equal(got, _pcm(want))
    else:
        assert all(c.dtype == torch.float32 for c in chunks) and torch.equal(got, want)
    assert rig.idle()


def test_streaming_with_speed_at_8k(rig):
    base = rig.base(speed=1.25)
    chunks = rig.run(speed=1.25, output_sample_rate=8000)
    n = sum(c.shape[1] for c in base)
    assert len(chunks) == len(base) == 3 and n == 480 * int(2 * FORCE_LEN / 1.25)
    got = torch.cat(chunks, dim=1)
    assert got.shape[1] == -(-n // 3) and torch.equal(got, _resample(torch.cat(base, dim=1), 8000))
    assert rig.idle()


def test_non_streaming_single_call(rig):
    base = rig.base(stream=False)
    got = rig.run(stream=False, output_sample_rate=22050, pcm16=True)
    assert len(got) == len(base) == 1 and got[0].dtype == torch.int16 and torch.equal(got[0], _pcm(_resample(base[0], 22050)))
    assert rig.idle()


@pytest.mark.parametrize('device_output', (False, True))
def test_coalesced_batch(rig, monkeypatch, device_output):
    """3 concurrent non-streaming calls of different lengths at 16 kHz: ONE cv2_out_resample_batch launch over the batch's ragged
    waveforms; each result is the conversion of its own default waveform (the vocoder's noise is drawn on the device per call, so the
    default waveforms are taken where the scheduler hands them to the conversion)."""
    import cosyvoice.cli.model as M
    mdl, seen, launches = rig.mdl, [], []
    real_convert, real_launch = mdl._out_convert, M.O.out_resample

    def convert(jobs):
        seen.extend((ox, wav.detach().clone().cpu()) for ox, wav, _f in jobs)
        return real_convert(jobs)

    def launch(args, **kw):
        launches.append(len(args))
        return real_launch(args, **kw)
    monkeypatch.setattr(mdl, '_out_convert', convert)
    monkeypatch.setattr(M.O, 'out_resample', launch)
    lens, res, errs, outs_of = (40, 57, 80), [None] * 3, [], {}

    def work(i):
        try:
            res[i] = [o['tts_speech'] for o in mdl.tts(text=rig.inp['text'], stream=False, force_len=lens[i], output_sample_rate=16000,
                                                       device_output=device_output, **rig.kw)]
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
    assert mdl.batch_sizes[n0:] == [3] and launches == [3] and len(seen) == 3
    wavs = {w.shape[1]: w for _ox, w in seen}
    for i, n_tok in enumerate(lens):
        (out,) = res[i]
        assert out.device.type == ('cuda' if device_output else 'cpu') and out.dtype == torch.float32
        w = wavs[480 * 2 * n_tok]
        assert torch.equal(out.cpu(), _resample(w, 16000)) and out.shape == (1, -(-w.shape[1] * 2 // 3))
    assert rig.idle()


def test_defaults_take_the_previous_path(rig, monkeypatch):
    import cosyvoice.cli.model as M
    mdl, sizes = rig.mdl, []

    def no_launch(*a, **k):
        raise AssertionError('the defaults must not launch the output conversion')
    monkeypatch.setattr(M.O, 'out_resample', no_launch)
    real = mdl._run_chunks

    def watch(batch):
        sizes.append(len(mdl.out_dict))
        return real(batch)
    monkeypatch.setattr(mdl, '_run_chunks', watch)
    for kw in (dict(output_sample_rate=None, pcm16=False), dict(output_sample_rate=24000)):
        sizes.clear()
        chunks = rig.run(**kw)
        assert sizes == [0, 0, 0] and not mdl.out_dict
        assert len(chunks) == 3 and all(torch.equal(a, b) and a.dtype == torch.float32 for a, b in zip(chunks, rig.base()))


def test_pcm16_at_24k_is_the_servers_bytes(rig):
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'cosyvoice2-eu_amd', 'runtime', 'python'))
    import wire
    base, chunks = rig.base(), rig.run(pcm16=True)
    assert len(chunks) == len(base)
    for a, b in zip(chunks, base):
        assert a.dtype == torch.int16 and a.shape == b.shape and a.numpy().tobytes() == wire.pcm16(b) == wire.pcm_bytes(a)
    assert rig.idle()


def test_abandoned_stream_and_bad_rate_leave_nothing(rig):
    mdl = rig.mdl
    g = mdl.tts(text=rig.inp['text'], stream=True, force_len=FORCE_LEN, output_sample_rate=48000, **rig.kw)
    first = next(g)['tts_speech']
    assert first.shape[1] > 0 and len(mdl.out_dict) == 1 and list(mdl.out_dict.values())[0].state.emitted == first.shape[1]
    g.close()
    assert rig.idle()
    with pytest.raises(ValueError):
        next(mdl.tts(text=rig.inp['text'], stream=True, force_len=FORCE_LEN, output_sample_rate=11025, **rig.kw))
    assert rig.idle()


def test_public_surface(rig):
    from cosyvoice.cli.cosyvoice import CosyVoice2
    from cosyvoice.cli.frontend import PrecomputedFrontEnd
    inp, got = rig.inp, []
    spk = {'prompt_text': inp['prompt_text'], 'prompt_text_len': torch.tensor([6]), 'llm_prompt_speech_token': inp['prompt_token'],
           'llm_prompt_speech_token_len': torch.tensor([31]), 'flow_prompt_speech_token': inp['prompt_token'],
           'flow_prompt_speech_token_len': torch.tensor([31]), 'prompt_speech_feat': inp['prompt_feat'],
           'prompt_speech_feat_len': torch.tensor([62]), 'llm_embedding': inp['embedding'], 'flow_embedding': inp['embedding']}

    class FE(PrecomputedFrontEnd):
        def frontend_zero_shot(self, tts_text, prompt_text, prompt_speech_16k, resample_rate, zero_shot_spk_id):
            got.append(resample_rate)
            return super().frontend_zero_shot(tts_text, prompt_text, prompt_speech_16k, resample_rate, zero_shot_spk_id)
    cv = CosyVoice2('unused', final=True, frontend=FE(lambda t: [1, 2, 3, 4, 5, 6, 7, 8], {'fr': spk}), state_dicts=rig.sds, output_sample_rate=16000)
    cv.model.sampling_mode = 0
    assert cv.sample_rate == 16000 and cv.model_sample_rate == 24000
    (ref,) = list(cv.output(sample_rate=24000).inference_zero_shot('bonjour', 'salut', None, zero_shot_spk_id='fr'))      # greedy: the length is the call's
    (out,) = list(cv.inference_zero_shot('bonjour', 'salut', None, zero_shot_spk_id='fr'))
    (pcm,) = list(cv.output(sample_rate=8000, pcm16=True).inference_zero_shot('bonjour', 'salut', None, zero_shot_spk_id='fr'))
    assert got == [24000, 24000, 24000], 'the frontend still receives the model rate'
    n = ref['tts_speech'].shape[1]
    assert n > 0 and ref['tts_speech'].dtype == torch.float32
    assert out['tts_speech'].dtype == torch.float32 and out['tts_speech'].shape == (1, -(-n * 2 // 3))
    assert pcm['tts_speech'].dtype == torch.int16 and pcm['tts_speech'].shape == (1, -(-n // 3))
    assert cv.sample_rate == 16000 and cv.output(sample_rate=8000).sample_rate == 8000 and not cv.model.out_dict
