"""Output rate / PCM16 without a GPU: the host planner cv2amd/outrate.py against the fp64 restatement of the
definition (tests/_outrate.py), the definition itself against an analytic sine and an aliasing tone, the int16 rule against the
servers' wire.pcm16, and the public surface."""
import inspect
import os
import sys

import numpy as np
import pytest

import _outrate as R

PKG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'cosyvoice2-eu_amd')
FILTERED = tuple(r for r in R.RATES if r != 24000)


def test_table_sizes():
    from cv2amd import outrate as O
    assert O.RATES == R.RATES
    for rate, (klen, rows) in R.SHAPES.items():
        k, up, down, kl, width = R.table(rate)
        assert k.shape == (rows, klen) and (up, kl) == (rows, klen)
        assert O.filter_shape(rate) == (up, down, klen, width)
    assert O.filter_shape(24000) == (1, 1, 1, 0) and R.table(24000)[0] is None


@pytest.mark.parametrize('rate', R.RATES)
def test_planner(rate):
    from cv2amd import outrate as O
    _, up, down, klen, width = R.table(rate)
    for n in R.LENGTHS:
        s = np.random.default_rng(n).standard_normal(n).astype(np.float32)
        once = R.resample64(s, rate)
        assert once.shape == (-(-n * up // down),)
        for name, chunks in R.chunkings(n).items():
            what = f'R={rate} N={n} "{name}"'
            st, total = O.OutState(rate), 0
            y, log = R.stream64(s, rate, chunks)
            for c, n_new in enumerate(chunks):
                final = c == len(chunks) - 1
                o0, n_emit, first_needed = O.plan(st, n_new, final)
                n_avail = st.consumed + n_new
                assert o0 == total and n_emit >= 0 and st.first <= first_needed <= n_avail, what
                assert (o0, n_emit, st.first, n_avail, n_avail - first_needed) == log[c], f'{what}: chunk {c} is not the definition\'s'
                if n_emit:                                                     # every in-range tap of every emitted output is there
                    lo = max(0, (o0 // up) * down - width)
                    hi = ((o0 + n_emit - 1) // up) * down - width + klen - 1
                    assert lo >= st.first, what
                    assert (o0 + n_emit == R.n_out(n_avail, rate)) if final else (hi <= n_avail - 1), what
                if not final:                                                  # nothing that could have gone out was held back
                    i_next = (o0 + n_emit) // up
                    assert (o0 + n_emit) % up == 0 and i_next * down - width + klen - 1 > n_avail - 1, what
                assert n_avail - first_needed < klen + down, f'{what}: retains {n_avail - first_needed} samples'
                st.commit(n_new, n_emit, first_needed, final)
                total += n_emit
            assert total == -(-n * up // down) == R.n_out(n, rate) == O.n_out(n, rate), what
            assert chunks[-1] == 0 or log[-1][1] > 0, f'{what}: the last chunk yields nothing'
            assert np.array_equal(y, once), f'{what}: the chunked restatement differs from the one-shot one'
            with pytest.raises(ValueError):
                O.plan(st, 1, False)                                           # the call has had its final chunk


@pytest.mark.parametrize('rate', FILTERED)
def test_definition_resamples_a_sine(rate):
    """1 kHz, 4800 samples: away from the edges the output is the sine at the new rate (the fp64 definition itself gives
    4.7e-5 .. 4.0e-4 over the six rates; the bar leaves room for the table's fp32 rounding)."""
    n = np.arange(4800)
    s = np.sin(2 * np.pi * 1000.0 * n / 24000.0).astype(np.float32)
    y = R.resample64(s, rate)
    o = np.arange(y.size)
    err = np.abs(y - np.sin(2 * np.pi * 1000.0 * o / rate))[200:-200].max()
    print(f'R={rate}: max |y - sine| = {err:.2e}')
    assert y.size == R.n_out(4800, rate) and err <= 1e-3


@pytest.mark.parametrize('rate', (8000, 16000))
def test_definition_rejects_what_would_alias(rate):
    """a tone at 1.25 x the new Nyquist comes out at <= -40 dB (the definition gives -45.3 / -45.2 dB)"""
    n = np.arange(4800)
    s = np.sin(2 * np.pi * (1.25 * rate / 2) * n / 24000.0).astype(np.float32)
    y = R.resample64(s, rate)[200:-200]
    db = 20 * np.log10(np.sqrt(np.mean(y ** 2)) / np.sqrt(np.mean(s.astype(np.float64) ** 2)))
    print(f'R={rate}: {db:.1f} dB')
    assert db <= -40.0


def test_pcm16_rule_is_the_servers():
    sys.path.insert(0, os.path.join(PKG, 'runtime', 'python'))
    import wire
    x = np.random.default_rng(16).uniform(-0.99, 0.99, 10000).astype(np.float32)
    assert np.array_equal(R.pcm16(x), np.frombuffer(wire.pcm16(x[None, :]), dtype=np.int16))
    edge = np.array([1.5, -1.5, 1.0, -1.0, -0.0, np.nan, 32767 / 32768, 0.99999, -0.99999, 1e-6], dtype=np.float32)
    assert R.pcm16(edge).tolist() == [32767, -32768, 32767, -32768, 0, 0, 32767, 32767, -32767, 0]


def test_surface():
    import torch
    from cv2amd import outrate as O
    from cosyvoice.cli.cosyvoice import CosyVoice2
    from cosyvoice.cli.model import CosyVoice2Model
    for bad in (11025, 0, 24001, 16000.0, '16000', True):
        with pytest.raises(ValueError):
            O.OutState(bad)
        with pytest.raises(ValueError):                                        # before any work: the model object is not even touched
            next(CosyVoice2Model.tts(None, text=torch.zeros(1, 3, dtype=torch.int32), output_sample_rate=bad))
        with pytest.raises(ValueError, match='output_sample_rate'):
            CosyVoice2('/nonexistent', output_sample_rate=bad)

    def params(f):
        return [(n, p.default) for n, p in inspect.signature(f).parameters.items() if n != 'self']
    init = params(CosyVoice2.__init__)
    assert init[:12] == [('model_dir', inspect._empty), ('load_jit', False), ('load_trt', False), ('load_vllm', False), ('fp16', False),
                         ('trt_concurrent', 1), ('setting', 'original'), ('llm_run_id', None), ('flow_run_id', None), ('hifigan_run_id', None),
                         ('final', False), ('backbone', None)]
    assert init[12:] == [('frontend', None), ('state_dicts', None), ('output_sample_rate', None), ('output_pcm16', False)]
    tts = params(CosyVoice2Model.tts)
    assert [n for n, _ in tts][:10] == ['text', 'flow_embedding', 'llm_embedding', 'prompt_text', 'llm_prompt_speech_token', 'flow_prompt_speech_token',
                                        'prompt_speech_feat', 'source_speech_token', 'stream', 'speed']
    assert tts[10:13] == [('force_len', None), ('device_output', False), ('output_sample_rate', None)] and tts[13] == ('pcm16', False)
    assert [n for n, _ in params(CosyVoice2.inference_zero_shot)] == ['tts_text', 'prompt_text', 'prompt_speech_16k', 'zero_shot_spk_id', 'stream', 'speed',
                                                                      'text_frontend']


def test_planner_module_stands_alone():
    """cv2amd/outrate.py never imports oracle/, and its planner needs neither torch nor the library"""
    src = open(os.path.join(PKG, 'cv2amd', 'outrate.py')).read()
    assert 'oracle' not in src.replace('no CPU fallback', '')
    head = src.split('# ---- the device side')[0]
    assert 'import torch' not in head and 'lib' not in head.replace('library', '')
