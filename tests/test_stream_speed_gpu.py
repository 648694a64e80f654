"""Streaming synthesis with speed != 1 through the scheduler (cosyvoice/cli/model.py): the chunk-invariant mel time-stretch between
the flow and the vocoder caches, for one stream, a generator-text call and eight shared streams.  Every yielded chunk is held to a
replay of the speed = 1 chunk logic (mel / source / speech caches, Hamming cross-fade; the reference's model.py:311-334 on the CPU
oracle) fed with the traced flow frames stretched in ONE shot by tests/_stretch.py.  Run with -m gpu."""
import threading

import numpy as np
import pytest
import torch

import _stretch as R

pytestmark = pytest.mark.gpu

FORCE_LEN = 80          # prompt of 31 tokens -> first chunk 44 tokens, second 25, final 11: three chunks, N = 160 frames


def _bistream_sd(layers):
    """synthetic LLM whose fill / EOS decoder biases let generator-text decoding terminate (as tests/golden/make_golden.py builds it)"""
    from cv2amd import synth
    sd = synth.make_llm(layers=layers)
    b = sd['llm_decoder.bias'].clone()
    b[6563] += 6.0
    b[6561] += 14.0
    b[6562] = -30.0
    sd['llm_decoder.bias'] = b
    return sd


class Rig:
    def __init__(self):
        from cv2amd import synth
        from cosyvoice.cli.model import CosyVoice2Model
        self.mdl = CosyVoice2Model(_bistream_sd(2), synth.make_flow(), synth.make_hift(), max_batch=8, max_text=64, max_prompt_tokens=64,
                                   max_new_tokens=256, sampling='greedy')
        inp = self.inp = synth.synthetic_inputs(seed=1, text_len=23, prompt_len=31, prompt_text_len=6)
        self.kw = dict(flow_embedding=inp['embedding'], llm_embedding=inp['embedding'], prompt_text=inp['prompt_text'],
                       llm_prompt_speech_token=inp['prompt_token'], flow_prompt_speech_token=inp['prompt_token'], prompt_speech_feat=inp['prompt_feat'])
        cuts = (0, 3, 10, 15, 23)
        self.pieces = [inp['text'][:, a:b] for a, b in zip(cuts[:-1], cuts[1:])]
        self.hsd = synth.make_hift()
        self.win = torch.from_numpy(np.hamming(2 * 3840)).float()
        self._solo = {}

    def run(self, speed, stream=True, bistream=False, seed=100):
        """one call alone, with injected noise and the trace on: (chunks, trace, token ids)"""
        mdl, cnt = self.mdl, [0]

        def hook(T):
            cnt[0] += 1
            return torch.randn(1, 480 * T, 9, generator=torch.Generator().manual_seed(seed + cnt[0]))
        mdl._noise_hook, mdl._trace, mdl._token_log = hook, [], {}
        try:
            text = (p for p in self.pieces) if bistream else self.inp['text']
            extra = {} if bistream else dict(force_len=FORCE_LEN)
            chunks = [o['tts_speech'] for o in mdl.tts(text=text, stream=stream, speed=speed, **extra, **self.kw)]
            trace, log = mdl._trace, mdl._token_log
        finally:
            mdl._noise_hook, mdl._trace, mdl._token_log = None, None, None
        assert len(log) == 1
        return chunks, trace, list(log.values())[0]

    def solo(self, speed, seed):
        if (speed, seed) not in self._solo:
            self._solo[(speed, seed)] = self.run(speed, seed=seed)
        return self._solo[(speed, seed)]

    def replay(self, trace, speed):
        """-> (reference chunks, N): the frames the scheduler handed on, stretched in one shot, through the speed = 1 chunk logic at
        the boundaries the definition gives (before the final chunk frame j goes out once i0 + 1 <= frames so far - 1)."""
        from oracle import hift as OH
        news = [t[0][:, :, t[1] * 2:] for t in trace]
        m = torch.cat(news, dim=2)
        n = m.shape[2]
        s = m if speed == 1.0 else torch.from_numpy(R.stretch(m.numpy(), speed))
        assert s.shape[2] == R.n_out(n, speed)
        i0 = R.index0(speed, np.arange(s.shape[2] + 4))
        cache, ref, seen, a = None, [], 0, 0
        for new, (_mel, _off, fin, nz, _u) in zip(news, trace):
            seen += new.shape[2]
            b = s.shape[2] if fin else seen if speed == 1.0 else int(np.sum(i0 + 1 <= seen - 1))
            mel, cs = s[:, :, a:b], torch.zeros(1, 1, 0)
            a = b
            if cache is not None:
                mel, cs = torch.cat([cache['mel'], mel], dim=2), cache['source']
            assert nz.shape[1] == 480 * mel.shape[2], 'the noise hook must be asked for the frames the vocoder gets'
            speech, src = OH.inference(self.hsd, mel, cs, torch.zeros(1, 9), nz)
            if cache is not None:
                speech[..., :3840] = speech[..., :3840] * self.win[:3840] + cache['speech'][..., -3840:] * self.win[3840:]
            if not fin:
                cache = {'mel': mel[:, :, -8:], 'source': src[:, :, -3840:], 'speech': speech[:, -3840:]}
                speech = speech[:, :-3840]
            ref.append(speech)
        return ref, n

    def check(self, chunks, trace, speed, what):
        ref, n = self.replay(trace, speed)
        assert len(chunks) == len(ref) == len(trace)
        assert sum(c.shape[1] for c in chunks) == 480 * int(n / speed), f'{what}: {sum(c.shape[1] for c in chunks)} samples for N = {n}'
        for k, (got, want) in enumerate(zip(chunks, ref)):
            assert got.shape == want.shape, f'{what} chunk {k}: {got.shape} vs {want.shape}'
            err = (got - want).abs().max().item()
            assert err < 1e-3, f'{what} chunk {k}: max abs err {err:.3e}'
        return n

    def idle(self):
        m = self.mdl
        return (not m.stretch_dict and not m.hift_cache_dict and not m.tts_speech_token_dict and not m._flow_caches
                and sorted(m._slot_free) == list(range(m.max_batch)))


@pytest.fixture(scope='module')
def rig():
    assert torch.cuda.is_available(), 'needs a GPU'
    return Rig()


@pytest.mark.parametrize('speed', [0.8, 1.25])
def test_stream_with_speed(rig, speed):
    base_chunks, base_trace, base_ids = rig.solo(1.0, 100)
    assert len(base_trace) == 3 and [t[2] for t in base_trace] == [False, False, True] and len(base_ids) == FORCE_LEN
    chunks, trace, ids = rig.run(speed)
    assert ids == base_ids, 'speed must not reach the token generation'
    assert [t[1:3] for t in trace] == [t[1:3] for t in base_trace]
    for t, u in zip(trace, base_trace):                                       # nor the flow: same frames as the speed = 1 call
        assert torch.equal(t[0][:, :, t[1] * 2:], u[0][:, :, u[1] * 2:])
    n = rig.check(chunks, trace, speed, f'speed {speed}')
    assert n == 2 * FORCE_LEN and all(torch.isfinite(c).all() for c in chunks)
    assert rig.idle()


def test_speed_one_stream_is_held_to_the_same_replay(rig):
    chunks, trace, _ = rig.solo(1.0, 100)
    rig.check(chunks, trace, 1.0, 'speed 1.0')


def test_bistream_with_speed(rig):
    b_chunks, b_trace, b_ids = rig.run(1.0, bistream=True)
    chunks, trace, ids = rig.run(1.25, bistream=True)
    assert ids == b_ids and len(ids) >= 50 and len(trace) >= 2
    n = rig.check(chunks, trace, 1.25, 'generator text, speed 1.25')
    assert n == 2 * len(ids)
    assert rig.idle()


def test_speed_outside_the_streaming_range_is_refused_before_any_work(rig):
    mdl = rig.mdl
    mdl._trace = []
    try:
        for bad in (2.5, 0.4):
            with pytest.raises(ValueError):
                next(mdl.tts(text=rig.inp['text'], stream=True, speed=bad, force_len=FORCE_LEN, **rig.kw))
            with pytest.raises(ValueError):
                next(mdl.tts(text=(p for p in rig.pieces), stream=True, speed=bad, **rig.kw))
        assert mdl._trace == [] and rig.idle()
    finally:
        mdl._trace = None


def test_non_streaming_speed_is_untouched(rig):
    """stream=False keeps the reference's one-shot F.interpolate (HiftEngine.change_speed): bit for bit what that path gives."""
    chunks, trace, _ = rig.run(1.25, stream=False)
    assert len(chunks) == 1 and len(trace) == 1
    mel, off, fin, nz, _u = trace[0]
    assert off == 0 and fin
    hift = rig.mdl.hift
    want, _ = hift.inference(hift.change_speed(mel.to(rig.mdl.device), 1.25).contiguous(), None, noise=nz)
    assert chunks[0].shape[1] == 480 * int(mel.shape[2] / 1.25)
    assert torch.equal(chunks[0], want.cpu())
    assert rig.idle()


def test_abandoned_stream_leaves_no_stretcher(rig):
    mdl = rig.mdl
    g = mdl.tts(text=rig.inp['text'], stream=True, speed=1.25, force_len=FORCE_LEN, **rig.kw)
    first = next(g)['tts_speech']
    assert first.shape[1] > 0 and len(mdl.stretch_dict) == 1 and list(mdl.stretch_dict.values())[0].state.emitted > 0
    g.close()
    assert rig.idle()


SPEEDS8 = [1.0, 0.8, 1.25, 2.0, 0.5, 1.0, 1.6, 1.25]


def _eight(rig, speeds):
    """eight calls at once, full rounds (the leader of a round waits for all eight chunks): per stream (chunks, trace, ids)"""
    mdl = rig.mdl
    cnt, lock, uuid_of, tl = {}, threading.Lock(), {}, threading.local()
    index_of = {}

    def hook(T, uuid):
        with lock:
            k = cnt[uuid] = cnt.get(uuid, 0) + 1
        return torch.randn(1, 480 * T, 9, generator=torch.Generator().manual_seed(1000 * (index_of[uuid] + 1) + k))

    def on_call(u):
        uuid_of[tl.i] = u
        index_of[u] = tl.i
    out, errs = [None] * len(speeds), []

    def work(i):
        tl.i = i
        try:
            out[i] = [o['tts_speech'] for o in mdl.tts(text=rig.inp['text'], stream=True, speed=speeds[i], force_len=FORCE_LEN, **rig.kw)]
        except Exception as e:      # noqa: BLE001
            errs.append(e)
    old = mdl.chunk_wave_ms, mdl.chunk_quiet_ms, mdl.prompt_cache_max
    mdl.chunk_wave_ms = mdl.chunk_quiet_ms = 2000.0
    mdl.prompt_cache_max = 0                       # (no prompt cache appears between two runs: both take the same flow path)
    mdl._noise_hook, mdl._noise_hook_takes_uuid, mdl._trace, mdl._token_log, mdl._on_call = hook, True, [], {}, on_call
    try:
        ths = [threading.Thread(target=work, args=(i,)) for i in range(len(speeds))]
        [t.start() for t in ths]
        [t.join(300) for t in ths]
        trace, log = mdl._trace, mdl._token_log
    finally:
        mdl._noise_hook, mdl._noise_hook_takes_uuid, mdl._trace, mdl._token_log, mdl._on_call = None, False, None, None, None
        mdl.chunk_wave_ms, mdl.chunk_quiet_ms, mdl.prompt_cache_max = old
    assert not errs, errs
    assert not any(t.is_alive() for t in ths), 'a call hangs'
    return [(out[i], [t for t in trace if t[4] == uuid_of[i]], log[uuid_of[i]]) for i in range(len(speeds))]


def _device_replay(rig, trace):
    """the traced flow mels and noise of one speed = 1 call through the scheduler's chunk path again, alone on the device"""
    mdl, u, k = rig.mdl, 'replay', [0]

    def hook(T):
        nz = trace[k[0]][3]
        k[0] += 1
        assert nz.shape[1] == 480 * T
        return nz
    mdl._noise_hook, mdl.hift_cache_dict[u] = hook, None
    try:
        return [mdl._mel2wav(t[0].to(mdl.device), t[1], u, t[2], 1.0).cpu() for t in trace]
    finally:
        mdl._noise_hook = None
        mdl.hift_cache_dict.pop(u, None)


def test_eight_streams_at_mixed_speeds(rig):
    mixed = _eight(rig, SPEEDS8)
    for i, (chunks, trace, ids) in enumerate(mixed):
        s_chunks, s_trace, s_ids = rig.solo(SPEEDS8[i], 1000 * (i + 1))       # the same call alone, same noise
        assert ids == s_ids, f'stream {i}'
        assert [c.shape for c in chunks] == [c.shape for c in s_chunks], f'stream {i}'
        rig.check(chunks, trace, SPEEDS8[i], f'stream {i} (speed {SPEEDS8[i]})')
        for k, (t, u) in enumerate(zip(trace, s_trace)):                      # flow frames: batched against single tile shapes
            a, b = t[0][:, :, t[1] * 2:], u[0][:, :, u[1] * 2:]
            rel = ((a - b).abs().max() / b.abs().max()).item()
            assert rel <= 1e-2, f'stream {i} chunk {k}: flow mel differs from the solo run by {rel:.3e}'
    assert rig.idle()
    # The speed = 1 members take exactly the path they take without stretched neighbours.  (1) Their chunks are, bit for bit, what the
    # speed = 1 chunk path gives for the same flow frames and noise with no other call around (_device_replay).  (2) The same eight calls
    # all at speed 1: same ids and chunk shapes for everybody, and a speed = 1 member whose flow frames came out bit-equal in the two runs
    # (the ragged flow batch packs the calls in arrival order) has bit-equal audio.
    plain = _eight(rig, [1.0] * len(SPEEDS8))
    for i, sp in enumerate(SPEEDS8):
        assert mixed[i][2] == plain[i][2]
        if sp != 1.0:
            continue
        for k, (a, b) in enumerate(zip(mixed[i][0], _device_replay(rig, mixed[i][1]))):
            assert torch.equal(a, b), f'stream {i} (speed 1) chunk {k} is not the plain chunk path beside stretched neighbours'
        assert [c.shape for c in mixed[i][0]] == [c.shape for c in plain[i][0]]
        same = all(torch.equal(t[0][:, :, t[1] * 2:], u[0][:, :, u[1] * 2:]) for t, u in zip(mixed[i][1], plain[i][1]))
        print(f'stream {i}: flow frames bit-equal between the mixed and the plain run: {same}')
        if same:
            for k, (a, b) in enumerate(zip(mixed[i][0], plain[i][0])):
                assert torch.equal(a, b), f'stream {i} (speed 1) chunk {k} changed beside stretched neighbours'
    assert rig.idle()


def test_shared_round_stretches_all_chunks_in_one_launch(rig, monkeypatch):
    """Without a noise hook the non-final chunks of a round go through _chunks_batched_hift: every stretched chunk of the round
    in ONE cv2_mel_stretch_batch launch, then the vocoder per (T, cached source) shape.  Lengths are the definition's."""
    import cosyvoice.cli.model as M
    mdl, calls = rig.mdl, []
    real = M.mel_stretch

    def spy(args, **kw):
        calls.append(len(args))
        return real(args, **kw)
    monkeypatch.setattr(M, 'mel_stretch', spy)
    speeds = [0.8, 1.25, 1.0, 1.6]
    out, errs = [None] * len(speeds), []

    def work(i):
        try:
            out[i] = [o['tts_speech'] for o in mdl.tts(text=rig.inp['text'], stream=True, speed=speeds[i], force_len=FORCE_LEN, **rig.kw)]
        except Exception as e:      # noqa: BLE001
            errs.append(e)
    old = mdl.chunk_wave_ms, mdl.chunk_quiet_ms
    mdl.chunk_wave_ms = mdl.chunk_quiet_ms = 2000.0
    try:
        ths = [threading.Thread(target=work, args=(i,)) for i in range(len(speeds))]
        [t.start() for t in ths]
        [t.join(300) for t in ths]
    finally:
        mdl.chunk_wave_ms, mdl.chunk_quiet_ms = old
    assert not errs, errs
    for sp, chunks in zip(speeds, out):
        assert len(chunks) == 3 and all(torch.isfinite(c).all() and c.abs().max() <= 0.99 for c in chunks)
        assert sum(c.shape[1] for c in chunks) == 480 * int(2 * FORCE_LEN / sp)
    assert calls.count(3) == 2, f'two non-final rounds with three stretched chunks each, got launches of {calls}'
    assert rig.idle()
